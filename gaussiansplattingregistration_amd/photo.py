"""Render-based photometric refinement of a rigid registration (``csrc/photo.hip``: ``gsr_photo_accumulate``).

Both models are rendered from the same cameras (``raster.render_model_aux``: colour, expected depth, coverage); the source is seen
through ``viewmat @ T``, so no copy of it is moved.  ``accumulate`` gives one camera's normal equations of the hybrid (intensity +
depth) term; ``PhotometricRefiner`` drives a coarse-to-fine damped Gauss-Newton loop around it, the 6 x 6 solve on the host in
float64.  The increment ``xi = (omega, v)`` acts on the left in the world (target) frame: ``T <- [exp(omega) | v] T``.
No GPU: ``RuntimeError`` -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from . import _marshal as _m

NSUMS = _lib.GSR_PHOTO_SUMS_LEN
_TRIU = [(r, c) for r in range(6) for c in range(r, 6)]
RCOND = 1e-8           # eigenvalues of the damped normal matrix below this share of the largest count as zero


@dataclass
class PhotoCamera:
    """What the refinement needs of a pinhole camera: ``viewmat`` (4, 4) float64 world -> camera, intrinsics, image size."""
    viewmat: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    image_name: str = ""

    @staticmethod
    def of(camera, scale=1):
        """from a ``models.camera.Camera`` (or anything with its attributes, or a ``PhotoCamera``), its image ``scale`` times smaller:
        ``width // scale`` x ``height // scale`` pixels (at least one), the intrinsics divided by ``scale``"""
        vm = camera.viewmat
        vm = vm.detach().cpu().numpy() if _m.is_tensor(vm) else np.asarray(vm)
        V = np.array(vm, np.float64).reshape(-1, 4, 4)[0]
        s = int(scale)
        if s < 1:
            raise ValueError(f"pyramid scale {scale} must be a positive integer")
        return PhotoCamera(V, float(camera.fx) / s, float(camera.fy) / s, float(camera.cx) / s, float(camera.cy) / s, max(1, int(camera.width) // s),
                           max(1, int(camera.height) // s), str(getattr(camera, "image_name", "")))


def unpack(sums):
    """-> (H (6, 6), b (6,), e_I, e_D, n) of the 30 sums of ``gsr_photo_accumulate``"""
    H = np.zeros((6, 6))
    for k, (r, c) in enumerate(_TRIU):
        H[r, c] = H[c, r] = sums[k]
    return H, np.array(sums[21:27], np.float64), float(sums[27]), float(sums[28]), int(round(float(sums[29])))


def accumulate_sums(source_maps, target_maps, camera, params, device=None):
    """the 30 float64 sums of one camera (``include/gsr_hip.h``).  ``source_maps`` / ``target_maps``: dicts with ``image (H, W, 3)``,
    ``depth (H, W)``, ``alpha (H, W)`` float32, all six host arrays or all six CUDA tensors; ``camera``: the camera the TARGET was
    rendered from (the source through ``viewmat @ T``) at the maps' resolution; ``params``: ``PhotometricParams``."""
    L = _lib.load(require_device=True)
    cam = camera if isinstance(camera, PhotoCamera) else PhotoCamera.of(camera)
    if params.max_depth_diff is None:
        raise ValueError("PhotometricParams.max_depth_diff has no default (scenes have no common unit): set it")
    maps = [source_maps["image"], source_maps["depth"], source_maps["alpha"], target_maps["image"], target_maps["depth"], target_maps["alpha"]]
    H, W = (int(s) for s in tuple(maps[1].shape)[-2:])
    if (W, H) != (cam.width, cam.height):
        raise ValueError(f"the maps are {W} x {H}, the camera renders {cam.width} x {cam.height}")
    on = [_m.is_cuda(a) for a in maps]
    if any(on) != all(on):
        raise ValueError("accumulate: the six maps must be all host arrays or all CUDA tensors")
    if device is None:
        device = maps[0].device.index if on[0] else 0
    shapes = [(H, W, 3), (H, W), (H, W)] * 2
    ptrs, keep = [], []
    for a, shape in zip(maps, shapes):
        if tuple(a.shape) != shape:
            raise ValueError(f"accumulate: a map is {tuple(a.shape)}, expected {shape}")
        p, k, _ = _m.prep(a, shape, np.float32, device)
        ptrs.append(p)
        keep.append(k)
    V = (C.c_double * 16)(*np.asarray(cam.viewmat, np.float64).reshape(16))
    out = (C.c_double * NSUMS)()
    _lib.check(L.gsr_photo_accumulate(*ptrs, H, W, V, cam.fx, cam.fy, cam.cx, cam.cy, float(params.lambda_depth), float(params.tau),
                                      float(params.max_depth_diff), 1 if on[0] else 0, out, device, C.c_void_p(_m.stream_ptr(device, on[0]))),
               "gsr_photo_accumulate")
    return np.array(out[:], np.float64)


def accumulate(source_maps, target_maps, camera, params, device=None):
    """-> ``(H (6, 6), b (6,), e_I, e_D, n)``: the normal matrix, the right-hand side, the two sums of squared residuals and the number
    of counted pixels of one camera (``accumulate_sums`` has the arguments)."""
    return unpack(accumulate_sums(source_maps, target_maps, camera, params, device))


def solve_step(H, b, mu):
    """``-(H + mu I)^+ b`` in float64: eigenvalues below ``RCOND`` of the largest count as zero, so that a motion the images do not
    constrain (a rank-deficient system) is left alone instead of being divided by rounding noise"""
    w, Q = np.linalg.eigh(np.asarray(H, np.float64) + float(mu) * np.eye(6))
    keep = w > RCOND * max(float(w.max()), 0.0)
    inv = np.where(keep, 1.0 / np.where(keep, w, 1.0), 0.0)
    return -(Q @ (inv * (Q.T @ np.asarray(b, np.float64))))


def se3_exp(xi):
    """the 4 x 4 matrix ``[exp(omega) | v]`` of an increment ``xi = (omega, v)`` (Rodrigues; the translation is ``v`` itself)"""
    w, v = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        R = np.eye(3) + K
    else:
        R = np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, v
    return T


@dataclass
class PhotometricResult:
    transformation: np.ndarray
    energy_initial: float = None        # E = sum(e_I + e_D) / n over the cameras at the start, at the LAST level's resolution
    energy_final: float = None          # the same at the returned transform
    n_pixels: int = 0                   # counted pixels over all cameras at the returned transform (last level)
    n_pixels_per_camera: list = field(default_factory=list)
    iterations: int = 0                 # source evaluations after each level's first, over all levels (rejected steps included)
    trace: list = field(default_factory=list)       # per level: scale, width / height of the first camera, iterations, accepted, energies, mu
    error_list: list = field(default_factory=list)


class PhotometricRefiner:
    """Refines ``init`` (source -> target, rigid 4 x 4) so that the renders of ``source`` through ``viewmat @ T`` agree with those of
    ``target`` in intensity and depth, from every camera of ``cameras`` (``models.camera.Camera`` or ``PhotoCamera``; they live in the
    target's frame).  ``params``: ``PhotometricParams``.  ``run()`` -> ``PhotometricResult``, or ``None`` when cancelled
    (``cancel()``; polled between iterations).  The two models are left as they were."""

    def __init__(self, source, target, cameras, params, init=None, device=0):
        self.signal_cancel = False
        self.source, self.target = source, target
        self.cameras = list(cameras)
        self.params = params
        self.init = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
        self.device = int(device)
        self.current_progress = 0
        self.max_progress = len(tuple(params.scales)) * int(params.max_iteration)

    def cancel(self):
        self.signal_cancel = True

    # ---- renders
    def _render(self, model, cam, viewmat):
        from . import raster
        return raster.render_model_aux(model, viewmat, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height, radius_clip=float(self.params.radius_clip),
                                       device=self.device)

    def _evaluate(self, cams, targets, T, per_camera=None):
        """the sums of ``cams`` at ``T`` added in camera order -> (H, b, E, n); ``per_camera`` (a list) receives every camera's count"""
        total = np.zeros(NSUMS)
        for cam, tg in zip(cams, targets):
            sums = accumulate_sums(self._render(self.source, cam, cam.viewmat @ T), tg, cam, self.params, self.device)
            if per_camera is not None:
                per_camera.append(int(round(sums[29])))
            total += sums
        H, b, e_I, e_D, n = unpack(total)
        return H, b, ((e_I + e_D) / n if n else float("inf")), n

    def _models_on_device(self):
        dev = f"cuda:{self.device}"
        out = []
        for m in (self.source, self.target):
            if m.device_name != dev:
                m = m.clone_gaussian()
                m.move_to_device(dev)
            out.append(m)
        self.source, self.target = out

    def run(self):
        P = self.params
        if P.max_depth_diff is None:
            raise ValueError("PhotometricParams.max_depth_diff has no default (scenes have no common unit): set it")
        scales = [int(s) for s in P.scales]
        if not scales or min(scales) < 1:
            raise ValueError(f"PhotometricParams.scales {tuple(P.scales)} must be positive integers, coarse to fine")
        _lib.load(require_device=True)
        self._models_on_device()
        T = self.init.copy()
        result = PhotometricResult(transformation=T.copy())
        errors = result.error_list
        if not self.cameras:
            errors.append("no camera given: the initial transform is returned")
            return result
        levels = {}

        def level(s):
            """the cameras of pyramid level ``s`` and their target maps, rendered once and kept"""
            if s not in levels:
                cams = [PhotoCamera.of(c, s) for c in self.cameras]
                levels[s] = (cams, [self._render(self.target, c, c.viewmat) for c in cams])
            return levels[s]
        name = lambda cams, i: cams[i].image_name or f"camera {i}"
        # the start, judged at the last level's resolution (what energy_final is measured at)
        cams, targets = level(scales[-1])
        counts = []
        _, _, E0, n0 = self._evaluate(cams, targets, T, counts)
        result.n_pixels, result.n_pixels_per_camera = n0, counts
        if n0 == 0:
            errors.append(f"no camera has a counted pixel (coverage >= {P.tau:g} in both renders, depths within {P.max_depth_diff:g}): "
                          "the initial transform is returned")
            return result
        result.energy_initial = result.energy_final = E0
        for s in scales:
            if self.signal_cancel:
                return None
            cams, targets = level(s)
            counts = []
            H, b, E, n = self._evaluate(cams, targets, T, counts)
            used = [i for i, c in enumerate(counts) if c > 0]
            for i, c in enumerate(counts):
                if c == 0:
                    errors.append(f"{name(cams, i)}: no counted pixel at scale {s} ({cams[i].width} x {cams[i].height}); skipped at this level")
            row = dict(scale=s, width=cams[0].width, height=cams[0].height, iterations=0, accepted=0, energies=[E], n_pixels=n, mu=float(P.damping))
            result.trace.append(row)
            if not used:
                continue
            if len(used) < len(cams):
                cams, targets = [cams[i] for i in used], [targets[i] for i in used]
            mu = float(P.damping)
            while row["iterations"] < int(P.max_iteration):
                if self.signal_cancel:
                    return None
                row["iterations"] += 1
                result.iterations += 1
                self.current_progress += 1
                delta = solve_step(H, b, mu)
                Tn = se3_exp(delta) @ T
                Hn, bn, En, nn = self._evaluate(cams, targets, Tn)
                if nn > 0 and En <= E:                     # accepted
                    T, H, b, E, n, mu = Tn, Hn, bn, En, nn, mu / 10.0
                    row["accepted"] += 1
                    row["energies"].append(E)
                    row["n_pixels"] = n
                    if float(np.linalg.norm(delta)) < float(P.min_increment):
                        break
                else:                                      # Levenberg-Marquardt: a step that raises E is rejected and mu is raised
                    if float(np.linalg.norm(delta)) < float(P.min_increment):
                        break                              # ... unless it was already below the increment: the renders' float32 floor
                    mu = max(10.0 * mu, 1e-6 * float(np.diag(H).max()))
            row["mu"] = mu
        cams, targets = level(scales[-1])
        counts = []
        _, _, E1, n1 = self._evaluate(cams, targets, T, counts)
        result.transformation = T
        result.energy_final, result.n_pixels, result.n_pixels_per_camera = (E1 if n1 else None), n1, counts
        return result


# ---- the flags the command-line tools share (scripts/register_ply.py, scripts/evaluate_registration.py) ------------------------------
def add_photo_arguments(ap, with_cameras=True):
    """``--photo-refine CAMERAS.json`` (``with_cameras``; a plain switch for a tool that has its own ``--cameras``) and its options"""
    if with_cameras:
        ap.add_argument("--photo-refine", metavar="CAMERAS.json", help="refine the registration photometrically from these cameras (in the second "
                        "scene's frame) after ICP: renders of both scenes, intensity + depth, damped Gauss-Newton")
    else:
        ap.add_argument("--photo-refine", action="store_true", help="refine the transform photometrically from the cameras before evaluating, and log "
                        "the metrics without and with it")
    ap.add_argument("--photo-max-depth-diff", type=float, metavar="D", help="a pixel counts when the two rendered depths differ by at most D (scene "
                    "units; required with --photo-refine)")
    ap.add_argument("--photo-scales", type=_scales, default=(4, 2, 1), metavar="4,2,1", help="image pyramid, coarse to fine (default 4,2,1)")
    ap.add_argument("--photo-lambda", type=float, default=0.968, metavar="L", help="weight of the depth term, the intensity term has 1 - L (default 0.968)")


def _scales(text):
    try:
        out = tuple(int(t) for t in text.split(","))
    except ValueError:
        out = ()
    if not out or min(out) < 1:
        import argparse
        raise argparse.ArgumentTypeError(f"{text!r} is not a comma-separated list of positive integers")
    return out


def photo_params_from_args(a):
    """-> ``PhotometricParams``, or ``None`` when ``--photo-refine`` was not given"""
    from .params.registration_parameters import PhotometricParams
    if not a.photo_refine:
        return None
    if a.photo_max_depth_diff is None:
        raise SystemExit("--photo-refine needs --photo-max-depth-diff (scenes have no common unit of length)")
    if not (a.photo_max_depth_diff > 0 and np.isfinite(a.photo_max_depth_diff)):
        raise SystemExit("--photo-max-depth-diff must be positive and finite")
    if not 0.0 <= a.photo_lambda <= 1.0:
        raise SystemExit("--photo-lambda must be in [0, 1]")
    return PhotometricParams(max_depth_diff=a.photo_max_depth_diff, scales=tuple(a.photo_scales), lambda_depth=a.photo_lambda)


def report_lines(result):
    """what the command-line tools print of a ``PhotometricResult``"""
    lines = [f"level 1/{r['scale']} ({r['width']} x {r['height']}): {r['iterations']} iterations, {r['accepted']} accepted, "
             f"E {r['energies'][0]:.6g} -> {r['energies'][-1]:.6g}, {r['n_pixels']} pixels" for r in result.trace]
    if result.energy_initial is not None and result.energy_final is not None:
        lines.append(f"E {result.energy_initial:.6g} -> {result.energy_final:.6g} over {result.n_pixels} pixels of {len(result.n_pixels_per_camera)} cameras")
    return lines + list(result.error_list)
