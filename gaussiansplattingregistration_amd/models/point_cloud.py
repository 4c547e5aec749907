"""Light point-cloud record standing in for ``o3d.geometry.PointCloud`` on the ICP path.

The reference hands Open3D clouds to ``do_icp_registration``; Open3D is an un-vendored wheel, so the
backend uses this record instead: ``points`` (N,3) float64 view, ``colors``, ``covariances`` (N,3,3),
``normals`` (N,3) float64.  The float32 coordinates (``xyz32`` -- what the splats really store,
``point_cloud_converter.py:33`` only widens them) are the primary storage and may be a PyTorch-ROCm
tensor, in which case the ICP kernels read them in place.
"""
from __future__ import annotations

import numpy as np

from .._marshal import is_tensor as _is_tensor

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


class PointCloud:
    def __init__(self, xyz32=None, colors=None, cov6=None, normals=None):
        self.xyz32 = xyz32 if xyz32 is not None else np.zeros((0, 3), np.float32)
        self.colors = colors
        self.cov6 = cov6
        self.normals = normals

    @property
    def device_index(self):
        if _is_tensor(self.xyz32) and self.xyz32.is_cuda:
            return self.xyz32.device.index
        return 0

    def __len__(self):
        return int(self.xyz32.shape[0])

    def __repr__(self):
        return f"PointCloud with {len(self)} points."

    @property
    def points(self):
        if _is_tensor(self.xyz32):
            return self.xyz32.detach().double().cpu().numpy()
        return np.asarray(self.xyz32, dtype=np.float64)

    @property
    def covariances(self):
        if self.cov6 is None:
            return None
        c = self.cov6.detach().double().cpu().numpy() if _is_tensor(self.cov6) else np.asarray(self.cov6, np.float64)
        return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)

    def has_normals(self):
        return self.normals is not None and self.normals.shape[0] == len(self) and len(self) > 0

    def has_covariances(self):
        return self.cov6 is not None

    def estimate_normals(self, knn=30):
        """Open3D ``estimate_normals()``, on the GPU.  A cloud whose covariances are set (every splat cloud,
        ``point_cloud_converter.py:40-43``) gets the smallest-eigenvalue eigenvector of each covariance; a cloud
        without covariances (a sparse input cloud, ``point_cloud_converter.py:9-28``) gets Open3D's default: the
        covariance of each point's ``knn`` = 30 nearest neighbours."""
        from .. import icp
        if self.cov6 is None:
            self.normals = icp.normals_knn(self.xyz32, knn=knn, device=self.device_index)
        else:
            self.normals = icp.normals_from_cov(self.cov6, device=self.device_index)
        return self

    def voxel_down_sample(self, voxel_size):
        """``o3d.geometry.PointCloud.voxel_down_sample``: one point per occupied voxel = the mean of the voxel's points,
        covariances and colours (float64 means, kept here in the record's float32 storage; voxels in ascending index
        order).  Runs on the GPU (``csrc/voxel.hip``)."""
        from .. import voxel
        xyz, cov6, col = voxel.voxel_down_sample(self.xyz32, voxel_size, cov6=self.cov6, color=self.colors, device=self.device_index,
                                                 as_torch=_is_tensor(self.xyz32) and self.xyz32.is_cuda)
        f32 = (lambda a: None if a is None else (a.float() if _is_tensor(a) else a.astype(np.float32)))
        return PointCloud(xyz32=f32(xyz), colors=f32(col), cov6=f32(cov6))

    # -- cleaning (Open3D's names and return pairs; csrc/clean.hip) --------------------------------------------------
    def _rows(self, mask):
        """(cloud of the rows with mask != 0, their indices): every array the record carries goes through one ``gsr_model_select``"""
        from .. import clean
        f32 = lambda a: None if a is None else (a.float() if _is_tensor(a) else np.asarray(a, np.float32))
        arrays = {"xyz": f32(self.xyz32), "dc": f32(self.colors), "cov6": f32(self.cov6)}
        sel, index = clean.select_rows(arrays, mask, device=self.device_index)
        cloud = PointCloud(xyz32=sel["xyz"], colors=sel.get("dc"), cov6=sel.get("cov6"))
        if self.normals is not None:            # float64: not a row of the float32 view; gathered through the index list
            idx = index.long() if _is_tensor(index) else np.asarray(index, np.int64)
            if _is_tensor(self.normals):
                cloud.normals = self.normals[idx.to(self.normals.device) if _is_tensor(idx) else torch.as_tensor(idx, device=self.normals.device)]
            else:
                cloud.normals = np.asarray(self.normals)[idx.cpu().numpy() if _is_tensor(idx) else idx]
        return cloud, index

    def remove_statistical_outlier(self, nb_neighbors, std_ratio):
        """``o3d.geometry.PointCloud.remove_statistical_outlier`` -> ``(cloud, index)``: the points whose mean distance to their
        ``nb_neighbors`` nearest points (the point itself included, as Open3D counts) is positive and below the cloud's mean +
        ``std_ratio`` standard deviations, and their indices.  Points with a non-finite coordinate are dropped first.  On the GPU;
        tensors stay tensors."""
        from .. import clean
        from ..params.clean_parameters import CleanParams
        mask, _ = clean.outlier_mask(self.xyz32, CleanParams(nb_neighbors=nb_neighbors, std_ratio=std_ratio), device=self.device_index)
        return self._rows(mask)

    def remove_radius_outlier(self, nb_points, radius):
        """``o3d.geometry.PointCloud.remove_radius_outlier`` -> ``(cloud, index)``: the points with more than ``nb_points`` points
        (themselves included) strictly within ``radius``."""
        from .. import clean
        from ..params.clean_parameters import CleanParams
        mask, _ = clean.outlier_mask(self.xyz32, CleanParams(nb_neighbors=0, radius=radius, nb_points=nb_points), device=self.device_index)
        return self._rows(mask)

    def select_by_index(self, index, invert=False):
        """``o3d.geometry.PointCloud.select_by_index``: the points listed in ``index`` (``invert``: all the others), in ascending
        order of their index whatever the order of the list."""
        n = len(self)
        if _is_tensor(self.xyz32) and self.xyz32.is_cuda:
            mask = torch.zeros(n, dtype=torch.uint8, device=self.xyz32.device)
            mask[torch.as_tensor(index, device=self.xyz32.device).long()] = 1
        else:
            mask = np.zeros(n, np.uint8)
            mask[index.cpu().numpy() if _is_tensor(index) else np.asarray(index, np.int64)] = 1
        return self._rows(1 - mask if invert else mask)[0]

    def orient_normals_consistent_tangent_plane(self, k, radius=None, reference="centroid"):
        """``o3d.geometry.PointCloud.orient_normals_consistent_tangent_plane(k)``: the normals' signs propagated along the minimum
        spanning forest of the neighbour graph (weight ``1 - |n_i . n_j|``), on the GPU (``csrc/orient.hip``).  The lists are the
        hybrid search's: the ``k`` nearest points within ``radius`` (and the point itself).  A finite ``radius`` is needed: the
        grid search walks ``radius / cell`` rings of cells around every point, so it has no pure k-NN mode.  Unlike Open3D no
        Delaunay edges join pieces further apart than ``radius``: each connected piece is oriented on its own and then takes the
        sign most of its normals need to look towards ``reference``: ``"centroid"`` (the cloud's, as
        ``orient_normals_towards_centroid`` computes it), a point, or ``None`` (the lowest vertex of each piece keeps its sign).
        The normals keep their placement; returns the cloud."""
        from .. import orient
        if not self.has_normals():
            raise RuntimeError("[Open3D Error] No normals in the PointCloud. Call estimate_normals() first.")
        if radius is None or not np.isfinite(radius) or not radius > 0:
            raise ValueError("orient_normals_consistent_tangent_plane needs a finite radius > 0: the neighbour lists come from the grid "
                             "search, which walks radius / cell rings of cells around every point (there is no pure k-NN mode)")
        if int(k) < 1:
            raise ValueError("k must be >= 1")
        nrm, xyz = self.normals, self.xyz32
        on = _is_tensor(nrm) and nrm.is_cuda
        if on != (_is_tensor(xyz) and xyz.is_cuda):                     # the coordinates go where the normals live
            xyz = torch.as_tensor(np.asarray(xyz, np.float32), device=nrm.device) if on else xyz.detach().cpu().numpy()
        if isinstance(reference, str):
            if reference != "centroid":
                raise ValueError(f"reference must be 'centroid', a point or None (got {reference!r})")
            reference = (xyz.detach().double().mean(0).cpu().numpy() if _is_tensor(xyz) else np.asarray(self.points, np.float64).mean(0))
        out, info = orient.orient_normals(xyz, nrm, float(radius), int(k) + 1, reference=reference,
                                          device=nrm.device.index if on else self.device_index, with_component=False)
        self.normals = out.to(nrm.dtype) if _is_tensor(out) else out.astype(np.asarray(nrm).dtype, copy=False)
        self.orient_info = info
        return self

    def transform(self, T):
        """``o3d.geometry.PointCloud.transform``: points p -> R p + t, normals n -> R n, covariances C -> R C R^T (Open3D's
        PointCloud::Transform).  Every array keeps its placement and dtype (a cuda tensor stays a cuda tensor)."""
        T = np.asarray(T, dtype=np.float64)
        R, t = T[:3, :3], T[:3, 3]

        def _pts(a):
            if _is_tensor(a):
                Rt, tt = torch.as_tensor(R, device=a.device), torch.as_tensor(t, device=a.device)
                return (a.detach().double() @ Rt.T + tt).to(a.dtype)
            return (np.asarray(a, np.float64) @ R.T + t).astype(np.asarray(a).dtype)

        def _vec(a):
            if _is_tensor(a):
                return (a.detach().double() @ torch.as_tensor(R, device=a.device).T).to(a.dtype)
            return (np.asarray(a, np.float64) @ R.T).astype(np.asarray(a).dtype)

        def _cov(c):
            idx = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
            if _is_tensor(c):
                Rt = torch.as_tensor(R, device=c.device)
                cd = c.detach().double()
                M = torch.stack([cd[:, idx[0]], cd[:, idx[1]], cd[:, idx[2]]], dim=1)
                M = Rt[None] @ M @ Rt.T[None]
                return torch.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], dim=1).to(c.dtype)
            cd = np.asarray(c, np.float64)
            M = np.stack([cd[:, idx[0]], cd[:, idx[1]], cd[:, idx[2]]], axis=1)
            M = R[None] @ M @ R.T[None]
            return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], axis=1).astype(np.asarray(c).dtype)

        self.xyz32 = _pts(self.xyz32)
        if self.normals is not None:
            self.normals = _vec(self.normals)
        if self.cov6 is not None:
            self.cov6 = _cov(self.cov6)
        return self

    def transform_similarity(self, T):
        """``transform`` for a similarity ``T = [c R | t]`` (a registration with scaling): points p -> c R p + t, normals
        n -> R n (they stay unit vectors), covariances C -> c^2 R C R^T.  ``T`` must pass ``similarity_util.split_similarity``."""
        from ..utils.similarity_util import split_similarity
        c, R, _ = split_similarity(T)
        normals, self.normals = self.normals, None
        self.transform(T)                       # points by A = c R, covariances by A C A^T = c^2 R C R^T
        if normals is not None:
            if _is_tensor(normals):
                normals = (normals.detach().double() @ torch.as_tensor(R, device=normals.device).T).to(normals.dtype)
            else:
                normals = (np.asarray(normals, np.float64) @ R.T).astype(np.asarray(normals).dtype)
        self.normals = normals
        return self
