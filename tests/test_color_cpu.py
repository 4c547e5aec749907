"""Colour harmonisation without a GPU: the float64 model (tests/color_model.py) against itself, and gsr_color_solve -- host code --
against the model from sums the model computed.

The bound of the solve.  The model has two honest routes to the same minimiser: the float64 normal equations of the stacked design
and a Householder QR of that design in longdouble.  On an input they differ by delta (printed; DESIGN.md section 21 records the
values).  The library is a third route -- float64 normal equations assembled from the 39 sums -- and may differ from the longdouble
QR by 4 delta, with a floor of 1e-12.
"""
import ctypes as C
import math

import numpy as np
import pytest

import color_model as M
from gaussiansplattingregistration_amd import _lib, harmonize

MODES = ("gain", "channel_gain", "affine")


def make_scene(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.5, (n, 3)).astype(np.float32), rng.normal(0, 2.0, n).astype(np.float32)


def truth(mode, rng):
    P = M.I0.copy()
    if mode == "gain":
        P[:, :3] *= rng.uniform(0.7, 1.3)
    elif mode == "channel_gain":
        P[:, :3] = np.diag(rng.uniform(0.7, 1.3, 3))
    else:
        P += rng.uniform(-0.1, 0.1, (3, 4))
    return P


def two_scenes(mode, n=600, seed=0, noise=0.0):
    """scene 1 is the reference's surface seen through another exposure: the reference (scene 0) shows D applied to scene 1's colours,
    so the fit of scene 1 against the reference is D"""
    rng = np.random.default_rng(seed + 100)
    dc1, op1 = make_scene(n, seed)
    D = truth(mode, rng)
    dc0 = M.distort(D, dc1)
    if noise:
        dc0 = (dc0 + rng.normal(0, noise, dc0.shape)).astype(np.float32)
    op0 = (op1 + rng.normal(0, 0.1, n)).astype(np.float32)
    pairs = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    return [(dc0, op0), (dc1, op1)], [(1, 0)], [pairs], D


def graph_scenes(mode, n=500, seed=0, extra=0):
    """four scenes in a chain 0-1-2-3 with the loop closure 3-0, known transforms D_i (reference 0: identity): scene i's colours are
    D_i^-1 of the common surface's.  `extra` more scenes follow: 4 has no edge, 5 hangs on an edge of 20 pairs."""
    rng = np.random.default_rng(seed + 200)
    surface, op = make_scene(n, seed)
    Ds = [M.I0.copy()] + [truth(mode, rng) for _ in range(3 + extra)]
    cols = []
    for D in Ds:
        A = np.vstack([D, [0, 0, 0, 1]])
        Dinv = np.linalg.inv(A)[:3]
        cols.append((M.distort(Dinv, surface), (op + rng.normal(0, 0.1, n)).astype(np.float32)))
    full = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    edges = [(0, 1), (1, 2), (2, 3), (3, 0)]
    lists = [full[(k * 37) % 50:] for k in range(4)]
    if extra >= 2:
        edges.append((5, 2))
        lists.append(full[:20])
    return cols, edges, lists, Ds


def model_sums(cols, edges, lists, P, k=math.inf):
    return np.array([M.sums(cols[s][0], cols[s][1], cols[t][0], cols[t][1], pl, P[s], P[t], k)[0] for (s, t), pl in zip(edges, lists)])


def bound(delta):
    return max(4 * delta, 1e-12)


# ---------------------------------------------------------------- the model against itself
@pytest.mark.parametrize("mode", MODES)
def test_model_recovers_a_known_transform(mode):
    cols, edges, lists, D = two_scenes(mode)
    for route in ("lstsq", "qr_longdouble", "normal"):
        P, held = M.irls(cols, edges, lists, mode=mode, huber=math.inf, iterations=1, prior=0.0, reference=0, route=route)
        # float32 storage of the distorted colours: 2^-24 relative on values below 4, through a transform with entries near 1
        assert np.abs(P[1] - D).max() < 1e-5, (route, np.abs(P[1] - D).max())
        assert np.array_equal(P[0], M.I0) and list(held) == [True, False]


def test_model_gain_modes_recover_a_pure_gain():
    cols, edges, lists, D = two_scenes("gain", seed=3)
    g = D[0, 0]
    for mode in ("gain", "channel_gain", "affine"):
        P, _ = M.irls(cols, edges, lists, mode=mode, huber=math.inf, iterations=1, prior=0.0, reference=0)
        assert np.abs(P[1] - g * M.I0).max() < 1e-5, mode


def test_model_sums_are_consistent_with_its_fit():
    """the objective assembled from the model's sums has its minimum where the model's design-based fit puts it (affine, N = 2)"""
    cols, edges, lists, D = two_scenes("affine", noise=0.01)
    P = np.tile(M.I0, (2, 1, 1))
    S = model_sums(cols, edges, lists, P)[0]
    Saa = np.zeros((4, 4))
    Saa[np.triu_indices(4)] = S[3:13]
    Saa = Saa + np.triu(Saa, 1).T
    Sab = S[13:29].reshape(4, 4)
    want = np.linalg.solve(Saa, Sab).T                   # rows p with Saa p = Sab[:, c]... for the target held at identity
    got, _ = M.irls(cols, edges, lists, mode="affine", huber=math.inf, iterations=1, prior=0.0, reference=0)
    assert np.abs(got[1] - want[:3]).max() < 1e-9


# ---------------------------------------------------------------- gsr_color_solve against the model
@pytest.mark.parametrize("mode", MODES)
def test_solve_two_scenes_against_model(hip_lib, mode):
    cols, edges, lists, D = two_scenes(mode, noise=0.01)
    P0 = np.tile(M.I0, (2, 1, 1))
    args = dict(mode=mode, huber=math.inf, iterations=1, prior=1e-4, min_pairs=100, reference=0)
    delta, want = M.delta(cols, edges, lists, **args)
    got, info = harmonize.solve_colors(P0, edges, model_sums(cols, edges, lists, P0), mode, 1e-4, 100, 0)
    err = np.abs(got - want).max()
    print(f"N=2 {mode}: delta {delta:.3e} library-model {err:.3e}")
    assert err <= bound(delta), (err, delta)
    assert list(info["held"]) == [True, False] and info["n_free"] == 1 and info["n_unknowns"] == M.MODES[mode]
    assert info["E_final"] <= info["E_initial"] and 0 < info["pivot_min"] <= info["pivot_max"]


@pytest.mark.parametrize("mode", MODES)
def test_solve_loop_graph_against_model(hip_lib, mode):
    cols, edges, lists, Ds = graph_scenes(mode)
    P0 = np.tile(M.I0, (4, 1, 1))
    args = dict(mode=mode, huber=math.inf, iterations=1, prior=1e-4, min_pairs=100, reference=0)
    delta, want = M.delta(cols, edges, lists, **args)
    got, info = harmonize.solve_colors(P0, edges, model_sums(cols, edges, lists, P0), mode, 1e-4, 100, 0)
    err = np.abs(got - want).max()
    print(f"N=4 loop {mode}: delta {delta:.3e} library-model {err:.3e}")
    assert err <= bound(delta), (err, delta)
    assert info["n_free"] == 3 and not info["held"][1:].any()
    for i in range(1, 4):                                 # and the joint fit is the truth, up to the prior's pull and float32 storage
        assert np.abs(got[i] - Ds[i]).max() < 2e-3, (i, np.abs(got[i] - Ds[i]).max())


def test_solve_holds_what_the_reference_does_not_reach(hip_lib):
    cols, edges, lists, Ds = graph_scenes("affine", extra=2)
    rng = np.random.default_rng(5)
    P0 = np.tile(M.I0, (6, 1, 1))
    P0[0] += rng.uniform(-0.05, 0.05, (3, 4))             # the reference is held at its INPUT value, whatever that is
    P0[4] += rng.uniform(-0.05, 0.05, (3, 4))
    P0[5] += rng.uniform(-0.05, 0.05, (3, 4))
    S = model_sums(cols, edges, lists, P0)
    assert S[4][0] == 20
    got, info = harmonize.solve_colors(P0, edges, S, "affine", 1e-4, 100, 0)
    assert list(info["held"]) == [True, False, False, False, True, True]
    for i in (0, 4, 5):
        assert got[i].tobytes() == P0[i].tobytes(), i
    assert not np.array_equal(got[1], P0[1])
    want, held = M.fit(P0, edges, [M.pair_terms(cols[s][0], cols[s][1], cols[t][0], cols[t][1], pl, P0[s], P0[t]) for (s, t), pl in zip(edges, lists)],
                       "affine", 1e-4, 100, 0)
    assert list(held) == list(info["held"])
    assert np.abs(got - want).max() < 1e-9


def test_solve_refusals(hip_lib):
    cols, edges, lists, D = two_scenes("affine")
    P0 = np.tile(M.I0, (2, 1, 1))
    S = model_sums(cols, edges, lists, P0)

    def refused(P=P0, edges=edges, S=S, mode="affine", prior=1e-4, reference=0):
        with pytest.raises(RuntimeError) as e:
            harmonize.solve_colors(P, edges, S, mode, prior, 100, reference)
        msg = str(e.value)
        assert "(-1)" in msg and "gsr_color_solve: " in msg and len(msg.split("gsr_color_solve: ")[-1]) > 0, msg     # GSR_E_INVALID and a message
        return msg

    refused(edges=[(1, 2)])
    refused(edges=[(-1, 0)])
    refused(edges=[(1, 1)])
    bad = P0.copy()
    bad[1, 2, 3] = np.inf
    refused(P=bad)
    bad = S.copy()
    bad[0, 17] = np.nan
    refused(S=bad)
    refused(prior=-1e-3)
    refused(prior=math.nan)
    refused(reference=2)
    # an unknown mode: through the C ABI (the Python front refuses the name itself)
    E = (_lib.ColorEdge * 1)()
    E[0].source, E[0].target = 1, 0
    E[0].sums[:] = S[0].tolist()
    P = P0.copy()
    assert hip_lib.gsr_color_solve(2, P.ctypes.data, 1, C.addressof(E), 3, 1e-4, 100, 0, None, None) == _lib.GSR_E_INVALID
    assert b"mode" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_color_solve(2, P.ctypes.data, 1, C.addressof(E), 2, 1e-4, 100, 0, None, None) == _lib.GSR_OK


def test_solve_singular_without_a_prior(hip_lib):
    """all-grey colours leave the affine transform undetermined: prior = 0 is refused with the advice to raise it, a prior decides"""
    rng = np.random.default_rng(2)
    v = rng.normal(0, 0.5, (400, 1)).astype(np.float32)
    dc = np.repeat(v, 3, 1)
    op = rng.normal(0, 2, 400).astype(np.float32)
    cols = [(dc, op), ((dc * np.float32(0.5)), op)]
    pairs = np.stack([np.arange(400), np.arange(400)], 1).astype(np.int32)
    P0 = np.tile(M.I0, (2, 1, 1))
    S = model_sums(cols, [(1, 0)], [pairs], P0)
    with pytest.raises(RuntimeError, match="raise prior"):
        harmonize.solve_colors(P0, [(1, 0)], S, "affine", 0.0, 100, 0)
    got, _ = harmonize.solve_colors(P0, [(1, 0)], S, "affine", 1e-4, 100, 0)
    assert np.isfinite(got).all()
    got, _ = harmonize.solve_colors(P0, [(1, 0)], S, "gain", 0.0, 100, 0)        # one unknown: determined


def test_new_symbols_are_exported(hip_lib):
    for name in ("gsr_model_match", "gsr_color_sums", "gsr_color_solve", "gsr_model_color_apply"):
        assert hasattr(hip_lib, name), name
        assert name in _lib.SIGNATURES
