"""The HEM level's float-heavy phases -- the per-child sums of wL (k_sumlw, or k_bucket_hist / k_bucket_scatter / k_bucket_sum) and the
M-step (k_mstep_headers, k_mstep<G>, the small-parent path, k_mstep<G, 1, true> with k_mstep_heavy_finish, k_orphan_rows) -- against
the float64 model of tests/hem_mstep_model.py, element by element, on hand-built levels whose parents sit exactly where the kernels
switch: 16 / 17 pairs (MSTEP_SMALL), 63 .. 65 (a wavefront), 127 .. 129 (MSTEP_CHUNK), 2047 .. 2049 and 4097 (MSTEP_SEG), 8200 (the
selection's work item of 8192 candidates), children of 2 .. 300 parents, orphans 0 .. 64 per 64 input rows, the array's last row a
child, likelihoods on both clamps through a subnormal wL, and a parent of weight 0.

Counts, row order and the orphans' rows are exact.  Every float of every parent row obeys

    |got - model| <= K 2^-24 mag,        K = 4 max(K_ref(case, field), K_small(field))

``mag`` the element's expression with absolute values for its terms (the model returns it), K_ref what the reference's float32 arithmetic
in serial order (the CPU oracle) costs against the model on the case, K_small the largest K_ref among the cases whose parents have at
most 16 pairs (the per-pair expression chain alone), both from tests/golden/hem_mstep_tolerance.json (written by the model and the
oracle: tests/test_hem_mstep_cpu.py keeps it current), 4 the margin for another summation order, contracted multiply-adds and the
device expf.  Nothing is calibrated on a kernel's output.  tests/test_hem_mstep_cpu.py shows that a 2049-pair parent losing its last
pair, a child's weight ignored, one of 65 parents missing from a child's sumLw and a forgotten `- dm dm'` each exceed the bound tenfold.
"""
import numpy as np
import pytest
import torch

import hem_mstep_model as M

pytestmark = pytest.mark.gpu

KNOBS = {"mstep_small_off": {"GSR_HEM_MSTEP_SMALL": "0"}, "mstep_split_off": {"GSR_HEM_MSTEP_SPLIT": "0"}, "sh_direct_off": {"GSR_HEM_SH_DIRECT": "0"},
         "sh_direct_on": {"GSR_HEM_SH_DIRECT": "1"}, "sumlw_sort": {"GSR_HEM_SUMLW": "sort"}, "select_np_1": {"GSR_HEM_SELECT_NP": "1"},
         "sparse_gb_0": {"GSR_HEM_SPARSE_GB": "0"}, "zero_copy": {}}
KNOB_CASES = ("ladder", "heavy", "shared", "last_row_child")
DEFAULT_RUNS = [(name, F) for name in M.CASES for F in M.widths(name)]


def _run(name, F, zero_copy=False):
    from gaussiansplattingregistration_amd import hem
    c, cl = M.case(name), M.cloud(name, F)
    p = c["params"]
    with hem.HemMixture(p["rho"], p["delta"], p["kappa"], p["tau"]) as m:
        m.set_level0(cl["xyz"], cl["color"], cl["opacity"], cl["cov6"], cl["sh"])
        m.set_state(parent_mask=c["mask"], weight=c["weight"])
        n_out, dropped = m.run_level(out=m.new_output() if zero_copy else None)
        st = m.stats()
        lv = m.get_level(as_torch=zero_copy, with_state=True)
        got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in lv.items()}
    return got, st, n_out, dropped


def _check(name, F, tag, zero_copy=False):
    got, st, n_out, dropped = _run(name, F, zero_copy)
    mdl, c, cl = M.model(name, F), M.case(name), M.cloud(name, F)
    want = mdl["stats"]
    # ---- exact: counts, the orphans' rows, the row order
    for k in ("parents", "pairs", "orphans", "dropped", "n_out", "max_pairs_of_a_parent"):
        assert st[k] == want[k], (tag, k, st[k], want[k])
    assert (n_out, dropped) == (want["n_out"], want["dropped"]) and got["xyz"].shape[0] == n_out, (tag, n_out, dropped)
    if name == "heavy":
        assert st["heavy_parents"] > 0, st
    p = mdl["n_parent_rows"]
    src = dict(cl, weight=c["weight"])
    for f in M.FIELDS:
        if f == "sh" and F == 0:
            continue
        a, b = np.ascontiguousarray(got[f][p:]), np.ascontiguousarray(src[f][mdl["orphan_in"]])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, f, "orphan rows")
    # ---- per element of every parent row.  A row in the wrong place is off by its distance to its neighbour, 20 radii: the bound sees it
    K = M.bound_constants()[name]
    worst = {}
    for f in M.FIELDS:
        if f == "sh" and F == 0:
            continue
        assert np.isfinite(got[f][:p]).all(), (tag, f)
        worst[f] = M.ratio(got, mdl, f, rows=p)
    print(f"{tag}: worst |got - model| / (2^-24 mag)", " ".join(f"{f} {v:.2f} (K {K[f]:.0f})" for f, v in worst.items()))
    for f, v in worst.items():
        assert v <= K[f], (tag, f, v, K[f])
    return worst


@pytest.mark.parametrize("name,F", DEFAULT_RUNS, ids=[f"{n}-F{F}" for n, F in DEFAULT_RUNS])
def test_level_equals_the_float64_model(name, F):
    """The default configuration, every case at F in {0, 9, 24, 45}; ladder and heavy also at 1, 47, 72, 105, 193, 256 floats per SH
    row (1 .. 32 lanes per row, widths that are no multiple of 4, the unpacked fold, the largest width).  zero_weight_parent and clamps
    expect what the model, which is the oracle (test_hem_mstep_cpu.py), computes: the weight-0 parent's row erased, its own children and
    itself orphans, the shared child wholly the other parent's; responsibilities 0.25 and 0.75 through a subnormal wL."""
    _check(name, F, f"{name} F={F}")


@pytest.mark.parametrize("name", KNOB_CASES)
@pytest.mark.parametrize("knob", sorted(KNOBS))
def test_level_under_the_knobs_equals_the_float64_model(monkeypatch, knob, name):
    """Every path the knobs select -- no small-parent path, heavy parents in one wave, SH rows from the sorted copy / from the level's
    own array (the array's last row a child: sh_tail), sorted instead of bucketed sums, one parent per selection wave, the two-pass
    fallback, the zero-copy output -- against the model itself, not against another run."""
    for k, v in KNOBS[knob].items():
        monkeypatch.setenv(k, v)
    _check(name, 45, f"{name} F=45 {knob}", zero_copy=knob == "zero_copy")
