"""Splat tensor container with the accessor names of the reference's ``GaussianModel``
(``src/models/gaussian_model.py:21``) -- the part of it the hot path touches.

Kept (same names / shapes): ``get_xyz (N,3)`` ``:56-57``, ``get_colors (N,3)`` ``:66-67``,
``get_spherical_harmonics (N, 3*((deg+1)^2-1))`` ``:70-71``, ``get_raw_opacity (N,1)`` ``:78-79``,
``get_covariance(1) (N,6)`` ``:89-91``, ``get_full_covariance()`` ``:81-87``, ``from_mixture(model, sh_degree)``
``:141-153``, ``move_to_device`` ``:223-234``, ``clone_gaussian``, ``from_ply`` / ``save_ply`` (``:98-139,169-185``; own
reader/writer in ``utils/ply_io.py``, ``plyfile`` is not needed).  ``from_arrays`` builds level 0 from raw arrays.

``from_mixture`` runs the reference's scaling/rotation rebuild (``:151-153,242-265``: batched ``eigh``, axis matching,
quaternions; the reference's own comment calls it unused) only when asked (``decompose=True`` / ``"reference"`` /
``"exact"``): registration only consumes xyz / covariance.  The rebuild is one device kernel (``csrc/model.hip``).

``transform_gaussian_model`` / ``get_merged_gaussian_point_clouds`` take ``rotate_sh`` (turn the SH coefficients with the cloud) and
run as one device kernel on CUDA tensors (``gsr_model_transform``); ``save_ply`` of a model on the device packs the rows there.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .. import _marshal as _m
from .. import _model_view as _mv
from .gaussian_mixture_level import GaussianMixtureModel


def _t(a, device, shape=None):
    if isinstance(a, torch.Tensor):
        t = a.detach().to(device=device, dtype=torch.float32)
    else:
        t = torch.as_tensor(np.asarray(a, dtype=np.float32), device=device)
    return t.reshape(shape) if shape is not None else t


def _matrices_to_quaternions(R):
    """(N,3,3) -> (N,4) (w, x, y, z), the trace formula the reference uses (``general_utils.py:94-100``; no branch for
    w -> 0, as there)."""
    w = torch.sqrt(1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]) * 0.5
    d = 4.0 * w
    return torch.stack((w, (R[:, 2, 1] - R[:, 1, 2]) / d, (R[:, 0, 2] - R[:, 2, 0]) / d, (R[:, 1, 0] - R[:, 0, 1]) / d), dim=-1)


class GaussianModel:
    def __init__(self, device_name="cpu"):
        self.sh_degree = -1
        self.device_name = device_name
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self._covariance = torch.empty(0)

    # -- accessors (reference names) -------------------------------------------------------------
    @property
    def get_scaling(self):
        return torch.exp(self._scaling)                              # gaussian_model.py:48-50

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._rotation)          # gaussian_model.py:52-54

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_colors(self):
        return self._features_dc.flatten(start_dim=1)

    @property
    def get_spherical_harmonics(self):
        return self._features_rest.flatten(start_dim=1)

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_raw_opacity(self):
        return self._opacity

    @property
    def get_opacity_with_activation(self):
        return torch.sigmoid(self._opacity)

    def get_full_covariance(self, scaling_modifier=1.0):
        c = self._covariance
        full = torch.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], dim=1)
        if scaling_modifier == 1:
            return full
        return full * float(scaling_modifier) ** 2

    def get_covariance(self, scaling_modifier=1):
        if scaling_modifier == 1:
            return self._covariance
        # the reference applies the diagonal scaling twice (gaussian_model.py:93-96): S (S C S^T) S^T
        return self._covariance * float(scaling_modifier) ** 4

    def __len__(self):
        return int(self._xyz.shape[0])

    # -- construction ------------------------------------------------------------------------------
    def from_arrays(self, xyz, colors, opacities, covariance, features, sh_degree):
        """Level 0 from the five arrays the HEM boundary takes (opacity RAW)."""
        n = int(xyz.shape[0])
        self.sh_degree = sh_degree
        k = (sh_degree + 1) ** 2 - 1
        self._xyz = _t(xyz, self.device_name, (n, 3))
        self._features_dc = _t(colors, self.device_name, (n, 1, 3))
        self._features_rest = _t(features, self.device_name, (n, k, 3))
        self._opacity = _t(opacities, self.device_name, (n, 1))
        self._covariance = _t(covariance, self.device_name, (n, 6))
        return self

    def from_ply(self, path_or_arrays, device=None, timing=None):
        """``GaussianModel.from_ply`` (reference ``gaussian_model.py:98-139``) from a file path (own reader,
        ``utils/ply_io.py``) or from the dict ``ply_io.load_gaussian_arrays`` returns.  ``device`` (a CUDA index; default: this
        model's ``device_name`` when that is a CUDA device): the file goes through pinned chunks straight into device SoA
        (``ply_io.load_gaussian_device``) -- the reference, too, loads onto ``cuda:0`` (``file_loader.py:53-66``)."""
        from ..utils import ply_io
        is_path = isinstance(path_or_arrays, (str, bytes)) or hasattr(path_or_arrays, "__fspath__")
        if device is None and is_path and str(self.device_name).startswith("cuda"):
            device = torch.device(self.device_name).index or 0
        if is_path and device is not None:
            self.device_name = f"cuda:{int(device)}"
            try:
                d = ply_io.load_gaussian_device(path_or_arrays, int(device), timing=timing)
            except ValueError:
                # the device loader takes binary little-endian float32 files whose vertex element comes first (what 3DGS writes); anything else the
                # format allows -- ASCII, big-endian, other property types, other element orders -- goes through the host reader, like the
                # reference's plyfile would read it, and is uploaded afterwards (from_arrays below)
                d = ply_io.load_gaussian_arrays(path_or_arrays)
        else:
            d = ply_io.load_gaussian_arrays(path_or_arrays) if is_path else path_or_arrays
        self.from_arrays(d["xyz"], d["color"], d["opacity"], d["cov6"], d["sh"], d["sh_degree"])
        self._scaling = _t(d["scale"], self.device_name)
        self._rotation = _t(d["rot"], self.device_name)
        return self

    def save_ply(self, path):
        """``GaussianModel.save_ply`` (``gaussian_model.py:169-185``)."""
        from ..utils import ply_io
        if self._scaling.numel() == 0:
            raise RuntimeError("save_ply needs scaling/rotation: build the model with from_ply or from_mixture(..., decompose=True)")
        if self._xyz.is_cuda:          # packed on the device and streamed out through pinned chunks: the same bytes, no full-size host copy
            ply_io.save_gaussian_device(path, self._xyz, self.get_colors, self.get_spherical_harmonics, self._opacity, self._scaling, self._rotation)
            return
        c = lambda t: t.detach().cpu().numpy()
        ply_io.save_gaussian_ply(path, c(self._xyz), c(self.get_colors), c(self.get_spherical_harmonics), c(self._opacity),
                                 c(self._scaling), c(self._rotation))

    def from_mixture(self, gaussian_mixture: GaussianMixtureModel, sh_degree: int, decompose=False):
        """``GaussianModel.from_mixture`` (``gaussian_model.py:141-153``).  ``decompose``: ``False`` skips the scaling /
        rotation rebuild (registration consumes xyz / covariance only); ``True`` or ``"reference"`` runs it with the
        reference's arithmetic, ``"exact"`` with a decomposition that really reproduces the covariance (what
        ``save_ply`` of a down-sampled model needs) -- both on the GPU (``csrc/model.hip``)."""
        self.sh_degree = sh_degree
        k = (sh_degree + 1) ** 2 - 1
        self._xyz = _t(gaussian_mixture.xyz, self.device_name)
        n = int(self._xyz.shape[0])
        self._features_dc = _t(gaussian_mixture.colors, self.device_name).view(n, 1, 3)
        self._features_rest = _t(gaussian_mixture.features, self.device_name).view(n, k, 3)
        self._opacity = _t(gaussian_mixture.opacities, self.device_name)
        self._covariance = _t(gaussian_mixture.covariance, self.device_name).view(n, 6)
        if decompose:
            mode = "exact" if decompose == "exact" else "reference"
            if mode == "reference":
                self._scaling, evec = self.decompose_covariance_matrix()
                self._rotation = self._last_quaternions
            else:
                self._scaling, self._rotation, _ = self._decompose(_lib.GSR_DECOMP_EXACT)
        return self

    def _decompose(self, mode):
        """-> (scaling (N,3), quaternions (N,4), matrices (N,3,3)) of ``gsr_decompose_cov`` on the model's covariances."""
        import ctypes as C
        L = _lib.load(require_device=True)
        cov = self._covariance
        n = int(cov.shape[0])
        device = cov.device.index if cov.is_cuda else 0
        p, keep, on = _m.prep(cov, (n, 6), np.float32, device)
        (sc, psc), (q, pq), (mat, pmat) = (_m.out(s, np.float32, device, on) for s in ((n, 3), (n, 4), (n, 3, 3)))
        _lib.check(L.gsr_decompose_cov(p, n, mode, psc, pq, pmat, *_mv.call_tail(device, on)), "gsr_decompose_cov")
        return torch.as_tensor(sc), torch.as_tensor(q), torch.as_tensor(mat)

    def decompose_covariance_matrix(self):
        """Scaling / rotation of every component from its covariance with the reference's arithmetic
        (``gaussian_model.py:242-265``), in ONE device kernel (``gsr_decompose_cov``, ``GSR_DECOMP_REFERENCE``) instead of
        a batched ``torch.linalg.eigh`` plus scatters: eigenpair k goes to the slot of the coordinate axis its eigenvector
        is most aligned with; two claims of one slot overwrite in eigenvalue order, an unclaimed slot stays zero.
        Returns (values (N,3), vectors (N,3,3)); like the reference's, the "scaling" is the eigenvalue itself, not its
        square root or logarithm.  The quaternions of the same call are kept in ``_last_quaternions``."""
        sc, q, mat = self._decompose(_lib.GSR_DECOMP_REFERENCE)
        self._last_quaternions = q
        return sc, mat

    @staticmethod
    def rotate_sh_matrices(rotation, sh_degree):
        """-> (D1 (3,3), D2 (5,5), D3 (7,7)) float64: how the SH-rest coefficients of a splat turn with the rotation ``rotation``
        (3x3), in the basis 3DGS evaluates and the coefficient order of ``_features_rest[n, k, c]`` (``gsr_sh_rotation``; host
        only).  For every direction d: ``basis(R d) . (D c) = basis(d) . c``.  Bands above ``sh_degree`` are the identity."""
        L = _lib.load()
        R = np.ascontiguousarray(np.asarray(rotation, dtype=np.float64).reshape(3, 3))
        B = np.empty(83, np.float64)
        _lib.check(L.gsr_sh_rotation(R.ctypes.data, int(sh_degree), B.ctypes.data), "gsr_sh_rotation")
        return B[:9].reshape(3, 3).copy(), B[9:34].reshape(5, 5).copy(), B[34:].reshape(7, 7).copy()

    def _transform_kernel(self, transformation_matrix, rotate_sh, into=None, similarity=False):
        """``gsr_model_transform`` on this model's arrays (one fused kernel; host tensors are staged by the library).  The
        results go to fresh arrays, or to the first ``len(self)`` rows of the tensors in ``into`` (name -> CUDA tensor).
        Returns name -> tensor for ``_xyz``, ``_covariance``, ``_rotation``, ``_features_rest``; this model is not modified.
        ``similarity``: ``gsr_model_similarity`` instead -- the matrix is ``[c R | t]`` -- and ``_scaling`` (log-scales, shifted by
        ``ln c``) joins the moved arrays when the model carries it."""
        import ctypes as C
        L = _lib.load(require_device=True)
        T = np.ascontiguousarray(np.asarray(transformation_matrix, dtype=np.float64).reshape(4, 4))
        n = len(self)
        K = _mv.sh_count(self)
        on = bool(self._xyz.is_cuda)
        device = self._xyz.device.index if on else 0
        have_rot = self._rotation.numel() > 0
        src = {"_xyz": (self._xyz, (n, 3)), "_covariance": (self._covariance, (n, 6)),
               "_rotation": (self._rotation if have_rot else None, (n, 4)), "_features_rest": (self._features_rest if K else None, (n, K, 3))}
        if similarity:
            src["_scaling"] = (self._scaling if self._scaling.numel() > 0 else None, (n, 3))
        ins, outs, ptr = {}, {}, {}
        for name, (t, shape) in src.items():
            if t is None:
                ins[name], ptr[name] = (None, None), None
                continue
            p, keep, t_on = _m.prep(t, shape, np.float32, device)
            if t_on != on:
                raise RuntimeError("the model's tensors must all live on one device")
            ins[name] = (p, keep)
            if into is not None:
                o = into[name]
                if not (o.is_cuda and o.is_contiguous() and o.dtype == torch.float32 and o.shape[0] >= n and tuple(o.shape[1:]) == tuple(shape[1:])):
                    raise RuntimeError(f"bad destination for {name}")
                outs[name], ptr[name] = o[:n], o.data_ptr()
            else:
                outs[name], ptr[name] = _m.out(shape, np.float32, device, on)
        fn, who = (L.gsr_model_similarity, "gsr_model_similarity") if similarity else (L.gsr_model_transform, "gsr_model_transform")
        _lib.check(fn(T.ctypes.data, n, K, 1 if rotate_sh else 0, *(ins[name][0] for name in src), *(ptr[name] for name in src), 1 if on else 0, device,
                      C.c_void_p(_m.stream_ptr(device, on))), who)          # (src is in the order of the entry points' arrays, inputs then outputs)
        return {name: torch.as_tensor(o) for name, o in outs.items()}

    # -- rigid motion and merge (reference ``gaussian_model.py:198-222,267-290``) ---------------------------------
    def transform_gaussian_model(self, transformation_matrix, rotate_sh=False):
        """Apply a rigid 4x4 to positions, covariances and rotation quaternions, in place.  ``rotate_sh=False``: the SH
        coefficients are left as they are, as in the reference -- the view-dependent colour then stays behind when the cloud
        turns.  ``rotate_sh=True`` turns them too (``rotate_sh_matrices``).  With ``rotate_sh=True`` or with CUDA tensors the
        whole motion is ONE device kernel (``gsr_model_transform``, ``csrc/model.hip``; no GPU: ``RuntimeError``); host tensors
        with the default keep the torch arithmetic below."""
        if rotate_sh or self._xyz.is_cuda:
            for name, t in self._transform_kernel(transformation_matrix, rotate_sh).items():
                setattr(self, name, t)            # the kernel is not in place: the fresh arrays replace the old ones
            return self
        T = torch.as_tensor(transformation_matrix, dtype=torch.float32, device=self._xyz.device)
        R, t = T[:3, :3], T[:3, 3]
        self._xyz = self._xyz @ R.T + t
        n = len(self)
        C = self.get_full_covariance()
        # R C R^T as two (3n x 3) GEMMs (a batched matmul with > 2^24 batches faults on this ROCm build)
        D = (C.reshape(n * 3, 3) @ R.T).reshape(n, 3, 3)
        C = (D.transpose(1, 2).reshape(n * 3, 3) @ R.T).reshape(n, 3, 3).transpose(1, 2)
        self._covariance = torch.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], dim=1)
        if self._rotation.numel():
            qr = _matrices_to_quaternions(R[None])[0]                       # (w, x, y, z) of the motion
            w0, x0, y0, z0 = self._rotation.unbind(-1)
            w1, x1, y1, z1 = qr
            q = torch.stack((w1 * w0 - x1 * x0 - y1 * y0 - z1 * z0,          # Hamilton product, reference operand order (:198-208)
                             w1 * x0 + x1 * w0 + y1 * z0 - z1 * y0,
                             w1 * y0 - x1 * z0 + y1 * w0 + z1 * x0,
                             w1 * z0 + x1 * y0 - y1 * x0 + z1 * w0), dim=-1)
            self._rotation = q / torch.linalg.vector_norm(q, dim=-1, keepdim=True)
        return self

    def similarity_transform_gaussian_model(self, transformation_matrix, rotate_sh=False):
        """Apply a similarity ``[c R | t]`` -- the result of a registration with scaling -- in place: positions ``c R x + t``,
        covariances ``c^2 R C R^T``, rotation quaternions by ``R``, the log-scales ``_scaling`` shifted by ``ln c``, the SH
        coefficients by ``R`` when ``rotate_sh``; opacity and DC colour stay.  Always ONE device kernel (``gsr_model_similarity``;
        host tensors are staged by the library, no GPU: ``RuntimeError``).  A matrix that is not ``c R`` with ``c > 0`` is refused."""
        for name, t in self._transform_kernel(transformation_matrix, rotate_sh, similarity=True).items():
            setattr(self, name, t)
        return self

    def warp_gaussian_model(self, field):
        """Apply a non-rigid ``warp.WarpField`` in place, like ``transform_gaussian_model``: positions
        ``float32(p + d(p))`` and covariances ``F cov F'`` with ``F = I + sum_k U_k grad w_k'`` in ONE device kernel
        (``gsr_model_warp``; host tensors are staged by the library, no GPU: ``RuntimeError``); ``_scaling`` / ``_rotation``, when the
        model carries them, are re-derived from the new covariances (``gsr_decompose_cov``, exact mode).  Opacity, DC colour and the SH
        coefficients stay: the per-splat rotation of the SH by the polar factor of ``F`` is left out.  ``self.warp_n_folded`` counts the
        splats with ``det F <= 0`` (reported, not treated specially).  A field with ``U == 0`` leaves every array's bits."""
        self.warp_n_folded = 0
        if len(self) == 0 or field.is_identity():
            return self
        device = self._xyz.device.index if self._xyz.is_cuda else 0
        xyz, cov, self.warp_n_folded = field.apply_arrays(self._xyz, self._covariance, device=device)
        self._xyz, self._covariance = torch.as_tensor(xyz), torch.as_tensor(cov)
        if _mv.has_scaling_rot(self):
            sc, q, _ = self._decompose(_lib.GSR_DECOMP_EXACT)
            self._scaling, self._rotation = sc.to(self._xyz.device), q.to(self._xyz.device)
        return self

    @staticmethod
    def _warped_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, warp, what=None):
        """``gaussian1`` moved by the matrix, brought to ``gaussian2``'s device and warped by ``warp``: a copy, bit for bit what
        ``clone_gaussian().transform_gaussian_model(T, rotate_sh)`` (``similarity_transform_gaussian_model`` with ``with_scaling``)
        followed by ``warp_gaussian_model(warp)`` gives.  ``what``: the merge that averages rows (fuse, colour matching) and so
        refuses an unrotated SH model under a rotating matrix."""
        g1 = gaussian1.clone_gaussian()
        moves = transformation_matrix is not None and not np.array_equal(np.asarray(transformation_matrix), np.eye(4))
        if moves:
            T = np.asarray(transformation_matrix, dtype=np.float64).reshape(4, 4)
            if what is not None:
                GaussianModel._require_rotate_sh(gaussian1, T, rotate_sh, what)
            if with_scaling:
                g1.similarity_transform_gaussian_model(T, rotate_sh=rotate_sh)
            else:
                g1.transform_gaussian_model(T, rotate_sh=rotate_sh)
        if g1._xyz.device != gaussian2._xyz.device:
            g1.move_to_device(str(gaussian2._xyz.device))
        return g1.warp_gaussian_model(warp)

    @staticmethod
    def fuse_overlap(gaussian1, gaussian2, params):
        """Overlap-aware merge of two models that are ALREADY IN ONE FRAME (``gsr_model_fuse``, ``csrc/fuse.hip``): a splat of
        ``gaussian1`` and a splat of ``gaussian2`` that are each other's best match under the gates of ``params``
        (``FuseOverlapParams``) are replaced by their moment-matched union; every other row is kept bit for bit.  Returns
        ``(model, info)``: the rows of ``gaussian1`` not in a pair, the fused rows, the rows of ``gaussian2`` not in a pair;
        ``info`` holds the report (``n_out``, ``n_pairs``, ``n_a_only``, ``n_b_only``, ``n_invalid_a``, ``n_invalid_b``) and
        ``pairs`` ((n_pairs, 2) int32: row of ``gaussian1``, row of ``gaussian2``), ``gated_pairs`` (the (a, b) that passed all gates),
        ``workspace_bytes`` (device memory the call allocated) and ``phase_ms`` (device events).  The result tensors are views ``[:n_out]`` of
        arrays allocated for ``n1 + n2`` rows.  Host tensors are staged by the library; no GPU: ``RuntimeError``."""
        import ctypes as C
        assert gaussian1.sh_degree == gaussian2.sh_degree
        L = _lib.load(require_device=True)
        n1, n2 = len(gaussian1), len(gaussian2)
        K, with_sr = _mv.layout([gaussian1, gaussian2])
        on, device = _mv.placement([gaussian1, gaussian2])
        keep = []
        va, vb = (_mv.view_of(g, K, with_sr, device, on, keep) for g in (gaussian1, gaussian2))
        vo, outs = _mv.out_view(n1 + n2, K, with_sr, device, on)
        pairs, ppairs = _m.out((min(n1, n2), 2), np.int32, device, on)
        P = _lib.FuseParams(float(params.max_distance), float(params.kld_max), float(params.color_delta))
        R = _lib.FuseReport()
        _lib.check(L.gsr_model_fuse(C.addressof(va), C.addressof(vb), K, C.addressof(P), C.addressof(vo), ppairs, C.addressof(R),
                                    *_mv.call_tail(device, on)), "gsr_model_fuse")
        m = _mv.model_from_arrays(outs, int(R.n_out), K, gaussian1.sh_degree, gaussian2.device_name)
        info = {k: int(getattr(R, k)) for k in ("n_out", "n_pairs", "n_a_only", "n_b_only", "n_invalid_a", "n_invalid_b")}
        info["pairs"] = torch.as_tensor(pairs)[:info["n_pairs"]]
        info["gated_pairs"], info["workspace_bytes"] = int(R.gated_pairs), int(R.workspace_bytes)
        info["phase_ms"] = dict(zip(("prepass_grid", "search", "pair_scan", "write"), (float(x) for x in R.phase_ms)))      # device events of the call
        return m, info

    @staticmethod
    def fuse_overlap_multi(models, params):
        """Overlap-aware merge of N models that are ALREADY IN ONE FRAME, in one pass (``gsr_fuse_multi``, ``csrc/fuse_multi.hip``;
        1 <= N <= 16).  Splats of different models that match under the gates of ``params`` (``FuseOverlapParams``) form GROUPS with at
        most one splat per model; a group is replaced by the moment-matched union of its members, every other row is kept bit for
        bit.  Returns ``(model, info)``: the rows in no group in the order of the models, then the fused rows (ascending by lowest
        member); ``info`` holds the report (``n_out``, ``n_groups``, ``n_grouped_rows``, ``n_invalid``, ``gated_pairs``,
        ``mutual_edges``, ``rejected_edges``, ``rounds``, ``workspace_bytes``, ``groups_of_size``), ``group_of`` ((n_total,) int32: the
        output row of each input row's group, -1 for a copied row) and ``phase_ms`` (device events).  The result tensors are views
        ``[:n_out]`` of arrays allocated for all rows.  Host tensors are staged by the library; no GPU: ``RuntimeError``."""
        import ctypes as C
        models = list(models)
        if not 1 <= len(models) <= _lib.GSR_FUSE_MAX_MODELS:
            raise ValueError(f"{len(models)} models (1 to {_lib.GSR_FUSE_MAX_MODELS})")
        L = _lib.load(require_device=True)
        N, total = len(models), sum(len(g) for g in models)
        K, with_sr = _mv.layout(models)
        on, device = _mv.placement(models)
        keep = []
        views = (_lib.ModelView * N)(*(_mv.view_of(g, K, with_sr, device, on, keep) for g in models))
        out_view, outs = _mv.out_view(total, K, with_sr, device, on)
        group_of, pgroup = _m.out((total,), np.int32, device, on)
        P = _lib.FuseParams(float(params.max_distance), float(params.kld_max), float(params.color_delta))
        R = _lib.FuseMultiReport()
        _lib.check(L.gsr_fuse_multi(C.addressof(views), N, K, C.addressof(P), C.addressof(out_view), pgroup, C.addressof(R),
                                    *_mv.call_tail(device, on)), "gsr_fuse_multi")
        m = _mv.model_from_arrays(outs, int(R.n_out), K, models[0].sh_degree, models[0].device_name)
        info = {k: int(getattr(R, k)) for k in ("n_out", "n_groups", "n_grouped_rows", "n_invalid", "gated_pairs", "mutual_edges", "rejected_edges", "rounds",
                                                "workspace_bytes")}
        info["groups_of_size"] = [int(x) for x in R.groups_of_size]
        info["group_of"] = torch.as_tensor(group_of)
        info["phase_ms"] = dict(zip(("prepass_grid", "search", "edges", "rounds", "write"), (float(x) for x in R.phase_ms)))      # device events of the call
        return m, info

    @staticmethod
    def get_merged_gaussian_point_clouds(gaussian1, gaussian2, transformation_matrix, rotate_sh=False, with_scaling=False, fuse=None, match_colors=None,
                                         match_colors_gate=None, warp=None):
        """``gaussian1`` moved by the registration result, concatenated with ``gaussian2`` (the merged-cloud save).
        ``with_scaling``: the matrix is a similarity (``similarity_transform_gaussian_model``); ``_scaling`` moves too.
        ``rotate_sh``: turn the SH coefficients of ``gaussian1`` with it (``transform_gaussian_model``).  When both models
        live on one CUDA device the merged arrays are allocated once, the kernel writes the moved ``gaussian1`` straight into
        their first rows and ``gaussian2`` is copied behind it: no clone, no ``cat``.  ``gaussian1`` is left as it was.
        ``fuse`` (``FuseOverlapParams``; default ``None``: the plain concatenation above): move, then ``fuse_overlap`` -- the splats
        the two models share are stored once.  Refused (``RuntimeError``) when the model has SH coefficients, the matrix rotates
        and ``rotate_sh`` is false.
        ``match_colors`` (``ColorMatchParams``; default ``None``: colours as they are): move, fit ``gaussian1``'s colour transform
        against ``gaussian2`` (``match_colors``; the correspondences are gated by ``fuse``, else by the ``FuseOverlapParams`` in
        ``match_colors_gate``), apply it, then concatenate or fuse.  The same refusal as for ``fuse``.
        ``warp`` (``warp.WarpField``; default ``None``): ``gaussian1`` is moved, THEN warped (``warp_gaussian_model``), then merged,
        fused or matched as above."""
        assert gaussian1.sh_degree == gaussian2.sh_degree
        if warp is not None:
            g1 = GaussianModel._warped_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, warp,
                                            "fuse" if fuse is not None else ("match_colors" if match_colors is not None else None))
            if fuse is None and match_colors is None and g1._xyz.is_cuda and gaussian2._xyz.is_cuda:      # (nothing moves any more: rows copied into arrays allocated once)
                return GaussianModel.get_merged_gaussian_point_clouds_multi([g1, gaussian2], [np.eye(4), np.eye(4)])
            return GaussianModel.get_merged_gaussian_point_clouds(g1, gaussian2, None, rotate_sh=rotate_sh, fuse=fuse, match_colors=match_colors,
                                                                  match_colors_gate=match_colors_gate)
        if match_colors is not None:
            g1, _ = GaussianModel.move_and_match_colors(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, match_colors,
                                                        fuse if fuse is not None else match_colors_gate)
            if fuse is not None:
                return GaussianModel.fuse_overlap(g1, gaussian2, fuse)[0]
            if g1._xyz.is_cuda and gaussian2._xyz.is_cuda:          # (nothing moves any more: the rows are copied into arrays allocated once)
                return GaussianModel.get_merged_gaussian_point_clouds_multi([g1, gaussian2], [np.eye(4), np.eye(4)])
            return GaussianModel.get_merged_gaussian_point_clouds(g1, gaussian2, None)
        if fuse is not None:
            return GaussianModel.get_fused_gaussian_point_clouds(gaussian1, gaussian2, transformation_matrix, fuse, rotate_sh=rotate_sh,
                                                                 with_scaling=with_scaling)[0]
        moves = transformation_matrix is not None and not np.array_equal(np.asarray(transformation_matrix), np.eye(4))
        x1, x2 = gaussian1._xyz, gaussian2._xyz
        if moves and x1.is_cuda and x2.is_cuda and x1.device == x2.device:
            m = GaussianModel._merged_on_device([gaussian1, gaussian2], [transformation_matrix, np.eye(4)], rotate_sh, [with_scaling, False])
            m.device_name = gaussian2.device_name
            return m
        m = GaussianModel(gaussian2.device_name)
        m.sh_degree = gaussian1.sh_degree
        g1 = gaussian1
        if moves:
            g1 = gaussian1.clone_gaussian()
            if with_scaling:
                g1.similarity_transform_gaussian_model(np.asarray(transformation_matrix, dtype=np.float64), rotate_sh=rotate_sh)
            elif rotate_sh:
                g1.transform_gaussian_model(np.asarray(transformation_matrix, dtype=np.float64), rotate_sh=True)
            else:
                g1.transform_gaussian_model(np.asarray(transformation_matrix, dtype=np.float32))
        for name in _mv.ATTRS:
            setattr(m, name, torch.cat((getattr(g1, name).to(gaussian2.device_name), getattr(gaussian2, name))))
        return m

    @staticmethod
    def get_merged_gaussian_point_clouds_multi(models, poses, rotate_sh=False, fuse=None):
        """N models, each moved by its rigid pose (4x4, the model's frame -> the common frame: the node poses of a multiway
        registration), concatenated in the order given.  The output arrays are allocated once and every model's fused transform
        kernel (``_transform_kernel(..., into=)``) writes straight into the model's rows: no clone, no ``cat``.  Rows
        ``[sum(n_0..n_i-1), sum(n_0..n_i))`` are bit for bit what ``transform_gaussian_model(poses[i], rotate_sh)`` gives for model
        ``i`` alone; a model whose pose is the identity is copied as it is, as in the pairwise merge.  The models stay as they
        were.  All of them must live on one CUDA device, with one SH degree and the same set of arrays.
        ``fuse`` (``FuseOverlapParams``; default ``None``: the plain concatenation above): move, then ``fuse_overlap_multi`` -- a surface
        that k models share is stored once.  Refused (``RuntimeError``) when the models have SH coefficients, a pose rotates and
        ``rotate_sh`` is false.  With the colours of the scenes harmonised on the way: ``get_merged_gaussian_point_clouds_multi_colors``."""
        if fuse is not None:
            return GaussianModel.get_merged_gaussian_point_clouds_fused_multi(models, poses, fuse, rotate_sh=rotate_sh)[0]
        return GaussianModel._merged_on_device(models, poses, rotate_sh, None)

    @staticmethod
    def _merged_on_device(models, poses, rotate_sh, similarity):
        """the plain concatenation of ``get_merged_gaussian_point_clouds_multi``; ``similarity``: per model, whether its pose is a
        similarity ``[c R | t]`` (``gsr_model_similarity``: ``_scaling`` moves too) -- ``None``: all rigid"""
        models, poses = list(models), [np.asarray(p, dtype=np.float64).reshape(4, 4) for p in poses]
        if not models or len(models) != len(poses):
            raise ValueError(f"{len(models)} models and {len(poses)} poses")
        names = _mv.ATTRS
        first = models[0]
        dev = first._xyz.device
        for g in models:
            if g.sh_degree != first.sh_degree:
                raise ValueError("the models differ in SH degree")
            if not g._xyz.is_cuda or g._xyz.device != dev:
                raise RuntimeError("get_merged_gaussian_point_clouds_multi: the models must all live on one CUDA device")
        sizes = [len(g) for g in models]
        total = sum(sizes)
        m = GaussianModel(first.device_name)
        m.sh_degree = first.sh_degree
        for name in names:
            arrays = [getattr(g, name) for g in models]
            if all(a.numel() == 0 and a.dim() < 2 for a in arrays):               # an array no model carries (no decompose)
                setattr(m, name, torch.empty(0, device=dev))
                continue
            if any(a.shape[0] != n or tuple(a.shape[1:]) != tuple(arrays[0].shape[1:]) for a, n in zip(arrays, sizes)):
                raise RuntimeError(f"{name}: the models do not carry it alike")
            setattr(m, name, torch.empty((total,) + tuple(arrays[0].shape[1:]), dtype=torch.float32, device=dev))
        off = 0
        for g, T, n, sim in zip(models, poses, sizes, similarity or [False] * len(models)):
            moves = n > 0 and not np.array_equal(T, np.eye(4))
            moved = ("_xyz", "_covariance", "_rotation", "_features_rest") + (("_scaling",) if sim else ())
            if moves:
                g._transform_kernel(T, rotate_sh, into={k: getattr(m, k)[off:off + n] for k in moved}, similarity=sim)
            for name in names:
                o = getattr(m, name)
                if o.numel() == 0 or o.shape[0] != total:
                    continue
                if not (moves and name in moved):
                    o[off:off + n].copy_(getattr(g, name))
            off += n
        return m

    @staticmethod
    def get_merged_gaussian_point_clouds_multi_colors(models, poses, match_colors, match_colors_gate=None, rotate_sh=False, fuse=None, reference=0):
        """``get_merged_gaussian_point_clouds_multi`` with the colours of the scenes harmonised between the move and the merge
        (the keyword ``match_colors=`` of the other merges, as a function of its own: that one's parameter list is fixed).
        ``match_colors`` (``ColorMatchParams``; ``None``: exactly ``get_merged_gaussian_point_clouds_multi(models, poses, rotate_sh,
        fuse)``): move, fit every model's colour transform jointly against ``models[reference]`` (``match_colors`` over all pairs of
        models; the correspondences are gated by ``fuse``, else by the ``FuseOverlapParams`` in ``match_colors_gate``), apply them, then
        concatenate or fuse.  The same refusal as for ``fuse`` when a pose rotates a model with SH coefficients and ``rotate_sh`` is false."""
        if match_colors is None:
            return GaussianModel.get_merged_gaussian_point_clouds_multi(models, poses, rotate_sh=rotate_sh, fuse=fuse)
        moved, _ = GaussianModel.move_and_match_colors_multi(models, poses, rotate_sh, match_colors, fuse if fuse is not None else match_colors_gate,
                                                             reference=reference)
        if fuse is not None:
            return GaussianModel.fuse_overlap_multi(moved, fuse)[0]
        return GaussianModel.get_merged_gaussian_point_clouds_multi(moved, [np.eye(4)] * len(moved))

    @staticmethod
    def get_merged_gaussian_point_clouds_fused_multi(models, poses, fuse, rotate_sh=False, match_colors=None):
        """Every model moved by its pose, then ``fuse_overlap_multi`` -> ``(model, info)``: what
        ``get_merged_gaussian_point_clouds_multi(..., fuse=params)`` returns the model of, with the report.  The models stay as they
        were; a model whose pose is the identity is used as it is.  ``match_colors`` (``ColorMatchParams``): the colours are
        harmonised between the move and the fusion; ``info["match_colors"]`` is then ``(transforms, info)`` of ``match_colors``."""
        if match_colors is not None:
            moved, colors = GaussianModel.move_and_match_colors_multi(models, poses, rotate_sh, match_colors, fuse)
            m, info = GaussianModel.fuse_overlap_multi(moved, fuse)
            info["match_colors"] = colors
            return m, info
        return GaussianModel.fuse_overlap_multi(GaussianModel._moved_multi(models, poses, rotate_sh, "fuse"), fuse)

    @staticmethod
    def _require_rotate_sh(model, T, rotate_sh, what):
        """a model with SH coefficients under a matrix that rotates (anything but a positive multiple of the identity) needs rotate_sh"""
        A = T[:3, :3]
        rotates = not (np.count_nonzero(A - np.diag(np.diag(A))) == 0 and A[0, 0] == A[1, 1] == A[2, 2] and A[0, 0] > 0)
        if _mv.sh_count(model) > 0 and rotates and not rotate_sh:
            raise RuntimeError(what + " needs rotate_sh=True when the matrix rotates a model with SH coefficients: an average of SH rows "
                               "in two frames means nothing")

    @staticmethod
    def _moved_multi(models, poses, rotate_sh, what):
        """every model in the common frame: a clone moved by its pose, or the model itself where the pose is the identity"""
        models, poses = list(models), [np.asarray(p, dtype=np.float64).reshape(4, 4) for p in poses]
        if not models or len(models) != len(poses):
            raise ValueError(f"{len(models)} models and {len(poses)} poses")
        moved = []
        for g, T in zip(models, poses):
            if len(g) == 0 or np.array_equal(T, np.eye(4)):
                moved.append(g)
                continue
            GaussianModel._require_rotate_sh(g, T, rotate_sh, what)
            moved.append(g.clone_gaussian().transform_gaussian_model(T, rotate_sh=rotate_sh))
        return moved

    @staticmethod
    def get_fused_gaussian_point_clouds(gaussian1, gaussian2, transformation_matrix, fuse, rotate_sh=False, with_scaling=False, match_colors=None, warp=None):
        """``gaussian1`` moved by the matrix, then ``fuse_overlap`` with ``gaussian2`` -> ``(model, info)``: what
        ``get_merged_gaussian_point_clouds(..., fuse=params)`` returns the model of, with the report.  As in the plain merge,
        ``gaussian1`` is left as it was and may live on another device than ``gaussian2``: its moved copy goes to ``gaussian2``'s.
        ``match_colors`` (``ColorMatchParams``): the colours of ``gaussian1`` are harmonised with ``gaussian2``'s between the move and
        the fusion; ``info["match_colors"]`` is then ``(transforms, info)`` of ``match_colors``.
        ``warp`` (``warp.WarpField``): ``gaussian1`` is warped between the move and everything else."""
        if warp is not None:
            g1 = GaussianModel._warped_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, warp, "fuse")
            return GaussianModel.get_fused_gaussian_point_clouds(g1, gaussian2, None, fuse, rotate_sh=rotate_sh, match_colors=match_colors)
        if match_colors is not None:
            g1, colors = GaussianModel.move_and_match_colors(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, match_colors, fuse)
            m, info = GaussianModel.fuse_overlap(g1, gaussian2, fuse)
            info["match_colors"] = colors
            return m, info
        return GaussianModel.fuse_overlap(GaussianModel._moved_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, "fuse"), gaussian2, fuse)

    @staticmethod
    def _moved_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, what):
        """``gaussian1`` in ``gaussian2``'s frame and on its device: a moved clone, or the model itself where nothing moves"""
        g1 = gaussian1
        moves = transformation_matrix is not None and not np.array_equal(np.asarray(transformation_matrix), np.eye(4))
        if moves:
            T = np.asarray(transformation_matrix, dtype=np.float64).reshape(4, 4)
            GaussianModel._require_rotate_sh(gaussian1, T, rotate_sh, what)
            g1 = gaussian1.clone_gaussian()
            if with_scaling:
                g1.similarity_transform_gaussian_model(T, rotate_sh=rotate_sh)
            else:
                g1.transform_gaussian_model(T, rotate_sh=rotate_sh)
        if g1._xyz.device != gaussian2._xyz.device:
            if g1 is gaussian1:
                g1 = gaussian1.clone_gaussian()
            g1.move_to_device(str(gaussian2._xyz.device))
        return g1

    # -- colour harmonisation (csrc/harmonize.hip; the reference has no such step) ---------------------------
    @staticmethod
    def match_colors(models, fuse_params, params=None, edges="all", reference=0):
        """The colour transforms that bring N models, ALREADY IN ONE FRAME, into agreement with ``models[reference]`` ->
        ``(transforms, info)``: ``harmonize.match_colors``.  ``params``: a ``ColorMatchParams`` (default: its defaults)."""
        from .. import harmonize
        return harmonize.match_colors(models, fuse_params, params, edges=edges, reference=reference)

    def apply_color_transform(self, P):
        """-> a new model whose colours are ``M x + b`` of this one's for ``P = [M | b]`` (3, 4), in every view direction (DC and every
        SH coefficient; ``gsr_model_color_apply``).  Every other tensor is shared with this model.  Colours are not clamped."""
        from .. import harmonize
        return harmonize.apply_colors(self, P)

    @staticmethod
    def _apply_solved(models, transforms):
        """a model whose solved transform is exactly [I|0] is not run through the kernel, as the merge does for an identity pose"""
        from .. import harmonize
        return [g if harmonize.is_identity(P) or len(g) == 0 else g.apply_color_transform(P) for g, P in zip(models, transforms)]

    @staticmethod
    def move_and_match_colors(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, match_colors, gate, warp=None):
        """What the pairwise merges do first when ``match_colors`` (``ColorMatchParams``) is set -> ``(model, (transforms, info))``:
        ``gaussian1`` moved into ``gaussian2``'s frame, its colour transform fitted against ``gaussian2`` (the reference) over the
        correspondences ``gate`` (``FuseOverlapParams``) admits, and applied.  ``transforms`` / ``info``: ``match_colors``'s, scene 0 =
        ``gaussian1``, scene 1 = ``gaussian2``.  ``gaussian1`` is left as it was.  ``warp`` (``warp.WarpField``): ``gaussian1`` is warped
        between the move and the fit."""
        if warp is not None:
            g1 = GaussianModel._warped_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, warp, "match_colors")
            return GaussianModel.move_and_match_colors(g1, gaussian2, None, rotate_sh, False, match_colors, gate)
        if gate is None:
            raise ValueError("match_colors needs the gates of its correspondences: fuse=, or a FuseOverlapParams in match_colors_gate=")
        g1 = GaussianModel._moved_pair(gaussian1, gaussian2, transformation_matrix, rotate_sh, with_scaling, "match_colors")
        colors = GaussianModel.match_colors([g1, gaussian2], gate, match_colors, edges=[(0, 1)], reference=1)
        return GaussianModel._apply_solved([g1], colors[0][:1])[0], colors

    @staticmethod
    def move_and_match_colors_multi(models, poses, rotate_sh, match_colors, gate, reference=0):
        """What the N-way merges do first when ``match_colors`` is set -> ``(models, (transforms, info))``: every model moved by its
        pose, the colour transforms fitted jointly against ``models[reference]`` over every pair of models, and applied."""
        if gate is None:
            raise ValueError("match_colors needs the gates of its correspondences: fuse=, or a FuseOverlapParams in match_colors_gate=")
        moved = GaussianModel._moved_multi(models, poses, rotate_sh, "match_colors")
        colors = GaussianModel.match_colors(moved, gate, match_colors, edges="all", reference=reference)
        return GaussianModel._apply_solved(moved, colors[0]), colors

    # -- cleaning (csrc/clean.hip; the reference has no such step) -------------------------------------------------------------
    def select_by_mask(self, mask):
        """The splats with ``mask != 0`` as a new model, every tensor (``_covariance`` included) bit for bit, in ascending row order;
        ``sh_degree`` is kept.  One ``gsr_model_select``; on the device for CUDA tensors."""
        from .. import clean
        n = len(self)
        K, with_sr = _mv.sh_count(self), _mv.has_scaling_rot(self)
        fields = _mv.carried(K, with_sr)
        device = self._xyz.device.index if self._xyz.is_cuda else 0
        sel, _ = clean.select_rows({f: getattr(self, attr).reshape(n, w) for f, attr, w in fields}, mask, device=device)
        k = int(sel["xyz"].shape[0])
        m = _mv.model_from_arrays({attr: sel[f] for f, attr, _ in fields}, k, K, self.sh_degree, self.device_name)
        m._opacity = m._opacity.view((k,) + tuple(self._opacity.shape[1:]))
        return m

    def remove_floaters(self, params):
        """-> ``(model, info)``: this model without its floaters (``params``: a ``CleanParams``).  ``gsr_outlier_mask`` -- finite test,
        opacity and extent gates, statistical filter, radius filter -- then ``gsr_model_select``, back to back: for a model on the
        device nothing but the report comes to the host.  ``info``: the report of ``clean.outlier_mask``.  This model is left as it
        was.  Applying it twice is NOT the identity: the survivors have a new mean and deviation."""
        from .. import clean
        n = len(self)
        device = self._xyz.device.index if self._xyz.is_cuda else 0
        scaling = self._scaling if self._scaling.numel() > 0 else None
        mask, info = clean.outlier_mask(self._xyz, params, raw_opacity=self._opacity.reshape(n), scaling=scaling, device=device)
        return self.select_by_mask(mask), info

    # -- visibility (csrc/raster.hip; the reference has no such step) --------------------------------------------
    def max_contribution(self, cameras, scale=1.0, radius_clip=0.0):
        """-> ``(n,)`` float32 tensor on the model's device: for every splat the largest blending weight ``alpha T`` it attains on any
        pixel of any of ``cameras`` (``models.camera.Camera``), RadSplat's importance score; 0 for a splat no camera shows.  One
        ``gsr_raster_render_aux`` per camera into one buffer (an integer maximum on the float bits: deterministic).  ``radius_clip`` is
        0 by default, NOT the evaluation's 3 px: with the clip small distant splats would score 0.  Needs a GPU (host tensors are
        uploaded); no GPU: ``RuntimeError``."""
        from .. import raster
        from ..utils.rasterization_util import _camera_args
        _lib.load(require_device=True)
        device = self._xyz.device.index if self._xyz.is_cuda else 0
        score = torch.zeros(len(self), dtype=torch.float32, device=torch.device("cuda", device))
        if len(self) == 0:
            return score.to(self._xyz.device)
        # every array goes to the device once, not once per camera (a model on the device is used where it lies)
        on = lambda t: t.detach().to(device=score.device, dtype=torch.float32).contiguous()
        arrays = (on(self.get_xyz), on(raster.model_cov6(self, scale)), on(self.get_raw_opacity), on(self.get_colors),
                  on(self._features_rest) if self._features_rest.numel() else None)
        ctx = raster.context(device)
        for camera in cameras:
            ctx.render_aux(*arrays, self.sh_degree, *_camera_args(camera), radius_clip=radius_clip, outputs=(), contribution=score)
        return score.to(self._xyz.device)

    def prune_unseen(self, cameras, min_contribution=0.01, scale=1.0, radius_clip=0.0):
        """-> ``(model, info)``: the splats whose ``max_contribution`` over ``cameras`` reaches ``min_contribution`` (RadSplat's
        threshold 0.01), through ``select_by_mask``: rows kept bit for bit, in order.  ``info``: ``n``, ``n_kept``, ``score`` (the
        ``(n,)`` tensor) and ``kept`` (the kept row indices, int64).  This model is left as it was.

        A splat OUTSIDE EVERY FRUSTUM scores 0 and is dropped exactly like one buried behind opaque surfaces: pass the cameras of
        ALL the scenes that were merged into this model, not those of one of them."""
        score = self.max_contribution(cameras, scale=scale, radius_clip=radius_clip)
        mask = score >= float(min_contribution)
        kept = torch.nonzero(mask).reshape(-1)
        model = self.select_by_mask(mask.to(torch.uint8))
        return model, {"n": len(self), "n_kept": int(kept.numel()), "score": score, "kept": kept}

    def clone_gaussian(self):
        m = GaussianModel(self.device_name)
        m.sh_degree = self.sh_degree
        for name in _mv.ATTRS:
            setattr(m, name, getattr(self, name).clone().detach())
        return m

    def move_to_device(self, device_name):
        if self.device_name == device_name:
            return
        self.device_name = device_name
        for name in _mv.ATTRS:
            setattr(self, name, getattr(self, name).to(device_name))
