"""NumPy model of the fine-tuner's loss kernel (csrc/imgloss.hip; the contract is in include/gsr_hip.h):
``loss = (1 - lambda) L1 + lambda (1 - SSIM)`` of an ``(H, W, 3)`` image against a target, and its gradient with respect to the image.

``loss_grad(a, b, lam, dtype)`` restates the kernel operation by operation in ``dtype``: the window (taps ``exp(-(j - 5)^2 / 4.5)`` divided
by their ascending sum), the two separable passes (horizontal first, taps ascending, a running sum that starts at 0), the pointwise terms
in the kernel's grouping, the adjoint filter, the combination, and the two sums in the fixed order of csrc/gsr_fold.h (every thread its
own pixel of a 16 x 16 tile over the channels in ascending order, the xor tree over the 64 lanes, the four waves in order, then the tiles
strided over 256 threads and the same tree again).  NumPy's arithmetic is IEEE and the library is built without fused multiply-add, so
with ``dtype=np.float64`` the model gives what the kernel must give up to the one float32 rounding at the store of the gradient, which
the model does not make.  ``np.longdouble`` is the same function one precision higher: what the float64 figures are measured against.
"""
import math
import zlib

import numpy as np

import fold_model as F

WIN, RAD, TILE = 11, 5, 16
SIZES = ("1x1", "3x7", "11x11", "16x16", "17x33", "37x50", "40x21")
SPECIAL = ("identical", "black", "flat", "over_range")
SCENES = SIZES + SPECIAL
LAMBDAS = (0.0, 0.2, 1.0)


def window(dtype=np.float64):
    T = np.dtype(dtype).type
    if T is np.float64:          # the host function of the library: libm's exp, the sum in ascending order
        w = [math.exp(-float((j - RAD) * (j - RAD)) / (2.0 * 1.5 * 1.5)) for j in range(WIN)]
    else:
        w = [np.exp(-T((j - RAD) * (j - RAD)) / (T(2) * T(1.5) * T(1.5))) for j in range(WIN)]
    s = T(0)
    for v in w:
        s = s + T(v)
    return np.array([T(v) / s for v in w], dtype=T)


def _pass(x, w, axis):
    """the zero-padded 11-tap filter along one axis of an (H, W, 3) array: a running sum from 0, taps ascending"""
    pad = [(0, 0)] * 3
    pad[axis] = (RAD, RAD)
    p = np.pad(x, pad)
    n = x.shape[axis]
    out = np.zeros_like(x)
    for j in range(WIN):
        sl = [slice(None)] * 3
        sl[axis] = slice(j, j + n)
        out = out + w[j] * p[tuple(sl)]
    return out


def filt(x, w):
    return _pass(_pass(x, w, 1), w, 0)          # horizontal, then vertical


def fold_tiles(v):
    """(H, W, 3) terms -> their sum in the kernel's order"""
    H, W, _ = v.shape
    ty, tx = (H + TILE - 1) // TILE, (W + TILE - 1) // TILE
    full = np.zeros((ty * TILE, tx * TILE), v.dtype)
    full[:H, :W] = (v[..., 0] + v[..., 1]) + v[..., 2]          # (0 + c0) + c1 + c2: adding to +0 changes nothing
    threads = full.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty * tx, 4, 64, 1)          # thread = 16 ly + lx, tiles row-major
    partials = F.waves_in_order(F.wave_sum(threads, F.XOR))          # [tiles][1]
    s = np.zeros((256, 1), v.dtype)
    for b0 in range(0, len(partials), 256):
        part = partials[b0:b0 + 256]
        s[:len(part)] = s[:len(part)] + part
    return F.waves_in_order(F.wave_sum(s.reshape(4, 64, 1), F.XOR))[0]


def loss_grad(a, b, lam, dtype=np.float64):
    """-> dict(loss, l1, ssim, grad (H, W, 3), grad_l1 (the L1 part of it), scale (H, W, 3)), everything in ``dtype``.  ``scale`` is the sum
    of the absolute values of the gradient's terms, (1 - lam) / N + (lam / N) (G*|D1| + 2 |a| G*|D2| + |b| G*|D3|): what an error of the
    gradient is measured in (the convention of DESIGN.md 26.3).  |D1| stands for the sum of the absolute values of D1's own four terms:
    they cancel where the images agree (``identical``: D1 = 0 in exact arithmetic), and the absolute value of their rounded sum would
    measure an error against its own residue."""
    T = np.dtype(dtype).type
    a, b = np.asarray(a).astype(T), np.asarray(b).astype(T)
    H, W, _ = a.shape
    w = window(T)
    C1, C2 = T(0.01 * 0.01), T(0.03 * 0.03)          # the kernel's float64 constants
    two, one, lam = T(2), T(1), T(lam)
    mu1, mu2, m_aa, m_bb, m_ab = filt(a, w), filt(b, w), filt(a * a, w), filt(b * b, w), filt(a * b, w)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = m_aa - mu1_sq, m_bb - mu2_sq, m_ab - mu12
    A1, A2, B1, B2 = two * mu12 + C1, two * s12 + C2, (mu1_sq + mu2_sq) + C1, (s1 + s2) + C2
    P = B1 * B2
    inv, rB1, rB2 = one / P, one / B1, one / B2
    S = (A1 * A2) / P
    tm2, tm1S = two * mu2, (two * mu1) * S
    D1 = (((tm2 * A2) * inv - (tm2 * A1) * inv) - tm1S * rB1) + tm1S * rB2
    D2 = -(S * rB2)
    D3 = (two * A1) * inv
    N = T(3.0 * H * W)
    c_l1, c_ssim = (one - lam) / N, lam / N
    d = a - b
    conv = (filt(D1, w) + (two * a) * filt(D2, w)) + b * filt(D3, w)
    grad_l1 = c_l1 * np.sign(d)
    grad = grad_l1 - c_ssim * conv
    D1_abs = (np.abs((tm2 * A2) * inv) + np.abs((tm2 * A1) * inv)) + (np.abs(tm1S * rB1) + np.abs(tm1S * rB2))
    scale = c_l1 + c_ssim * ((filt(D1_abs, w) + (two * np.abs(a)) * filt(np.abs(D2), w)) + np.abs(b) * filt(np.abs(D3), w))
    l1, ssim = fold_tiles(np.abs(d)) / N, fold_tiles(S) / N
    loss = (one - lam) * l1 + lam * (one - ssim)
    return dict(loss=loss, l1=l1, ssim=ssim, grad=grad, grad_l1=grad_l1, scale=scale)


def _grid(rng, shape, top=1.0):
    """values on an 11-bit grid in [0, top)"""
    return (rng.integers(0, int(2048 * top), shape) / 2048.0).astype(np.float32)


def build(name):
    """-> (a, b): two (H, W, 3) float32 images.  The sizes: smaller than the window, the window, exactly one tile, one row and one column
    into the next tile (the halo crosses an image edge inside a tile), several tiles with partial ones.  ``a != b`` everywhere except in
    ``identical`` and ``black``, by at least 2^-11: a central difference of step 2^-16 never crosses the kink of |a - b|."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in SIZES:
        h, w = (int(v) for v in name.split("x"))
        top = 1.0
    else:
        h, w = 17, 33
        top = 1.5 if name == "over_range" else 1.0
    if name == "black":
        z = np.zeros((h, w, 3), np.float32)
        return z, z.copy()
    if name == "flat":          # a nearly flat pair: s1 = m_aa - mu1^2 cancels against C2 = 9e-4
        a = np.full((h, w, 3), 0.7, np.float32)
        k = rng.integers(0, 2, (h, w, 3))
        b = np.where(k == 1, np.float32(0.7) + np.float32(1.0 / 256.0), np.float32(0.7) - np.float32(1.0 / 2048.0)).astype(np.float32)
        return a, b
    a = _grid(rng, (h, w, 3), top)
    if name == "identical":
        return a, a.copy()
    b = _grid(rng, (h, w, 3))
    b = np.where(a == b, np.where(b >= 0.5, b - np.float32(1.0 / 2048.0), b + np.float32(1.0 / 2048.0)), b).astype(np.float32)
    return a, b


def tolerance_figures(name, lam):
    """what the float64 arithmetic costs on a scene: the float64 model against the same function in ``np.longdouble``"""
    a, b = build(name)
    lo, hi = loss_grad(a, b, lam, np.float64), loss_grad(a, b, lam, np.longdouble)
    err, scale = np.abs(lo["grad"] - hi["grad"]), hi["scale"]
    assert not err[scale == 0].any()          # (black with lam = 1: every term of the gradient is an exact zero)
    fig = {"grad": float((err[scale > 0] / scale[scale > 0]).max()) if (scale > 0).any() else 0.0}
    for k in ("loss", "l1", "ssim"):
        fig[k] = float(abs(np.longdouble(lo[k]) - hi[k]))
    return fig
