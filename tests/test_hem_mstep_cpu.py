"""The float64 model of one HEM level (tests/hem_mstep_model.py) and its hand-built cases are checked before they judge the kernels
(test_hem_mstep_gpu.py): every decision of every case is unambiguous in float32, the cases hold what they were built to hold, the
model's counts and row order are the CPU oracle's, the tolerance file is current, and the per-element bound sees the four ways of
being subtly wrong that the whole-array 1e-4 rule of test_hem_gpu.py does not.  Nothing here needs a GPU.
"""
import numpy as np
import pytest

import hem_mstep_model as M

F_CHECK = 9


# ------------------------------------------------------------------------------------------------------------- the cases themselves
@pytest.mark.parametrize("name", M.CASES)
def test_every_decision_has_a_margin(name):
    """Radius, colour, KL and both clamps at least 1e-3 (relative) from their thresholds, every merged covariance's determinant at
    least 1e-3 of the sum of its terms' magnitudes (but for the deliberate 0 / 0 row of zero_weight_parent): float32 rounding of
    about 1e-6 cannot change the pair set, a clamp or the erase."""
    m, c = M.model(name, F_CHECK), M.case(name)
    print(name, {k: f"{v:.3g}" for k, v in m["margins"].items()})
    for k, v in m["margins"].items():
        assert v >= 1e-3, (name, k, v)
    dm = m["det_margin_of"]
    parents = np.nonzero(c["mask"])[0]
    for k, s in enumerate(parents):
        if name == "zero_weight_parent" and s == c["Z"]:
            assert not np.isfinite(dm[k])
        else:
            assert dm[k] >= 1e-3, (name, s, dm[k])


def _pairs(name):
    return sorted(int(v) for v in M.model(name, F_CHECK)["pairs_of"])


def test_ladder_and_heavy_sit_on_the_switch_points():
    assert _pairs("ladder") == sorted(M.LADDER_PAIRS) and len(M.LADDER_PAIRS) == 13          # 13 parents: the last wave of four has one
    assert _pairs("heavy") == sorted(M.HEAVY_PAIRS + M.HEAVY_FILL)
    total = sum(M.HEAVY_PAIRS + M.HEAVY_FILL)
    heavy_from = 16.0 * total / len(M.HEAVY_PAIRS + M.HEAVY_FILL) + 1                            # the selection's rule: 16 x the mean
    assert 4097 < heavy_from < 8192 < max(M.HEAVY_PAIRS)                                      # one heavy parent, more than one work item
    for p in (15, 16, 17, 63, 64, 65, 127, 128, 129):
        assert p in M.LADDER_PAIRS
    for p in (2047, 2048, 2049, 4097, 8200):
        assert p in M.HEAVY_PAIRS
    assert M.case("heavy")["xyz"].shape[0] > 4 * 4096                                         # several buckets of 4096 children
    for name in ("ladder", "heavy"):
        st = M.model(name, F_CHECK)["stats"]
        assert st["orphans"] == 0 and st["dropped"] == 0 and st["pairs"] == M.case(name)["xyz"].shape[0]


def test_shared_children_have_the_intended_parents():
    m, c = M.model("shared", F_CHECK), M.case("shared")
    want = sorted(ch + 1 for par, ch in M.SHARED for _ in range(par))
    assert _pairs("shared") == want
    assert m["stats"]["pairs"] == sum(par * (ch + 1) for par, ch in M.SHARED) and m["stats"]["orphans"] == 0
    assert sorted({par for par, _ in M.SHARED}) == [2, 3, 7, 8, 9, 64, 65, 300]               # parents per child: around 8 lanes, around a wave
    # every child's responsibilities are below 1: a parent's weight exceeds its own by less than the children's weights
    w = c["weight"].astype(np.float64)
    parents = np.nonzero(c["mask"])[0]
    for k, s in enumerate(parents):
        kids = np.nonzero((c["cluster"] == c["cluster"][s]) & (c["mask"] == 0))[0]
        gain = m["weight"][k] - w[s]
        assert 0 < gain < w[kids].sum() * (1 - 1e-9), (s, gain)


def test_orphans_are_where_the_case_says():
    m, c = M.model("orphans", F_CHECK), M.case("orphans")
    n = c["xyz"].shape[0]
    assert np.array_equal(m["orphan_in"], c["orphan_slots"]) and m["orphan_in"][-1] == n - 1
    per_block = np.bincount(m["orphan_in"] // 64, minlength=len(M.ORPHAN_BLOCKS) + 1)
    assert tuple(per_block[:len(M.ORPHAN_BLOCKS)]) == M.ORPHAN_BLOCKS and {0, 1, 4, 5, 64} <= set(per_block.tolist())
    tags = c["tag"][m["orphan_in"]]
    assert {"orphan_far", "orphan_color", "orphan_kl"} == set(tags.tolist())
    assert m["stats"]["max_pairs_of_a_parent"] <= 16 and "orphans" in M.small_cases()
    assert c["params"]["kappa"] == 1.0


def test_last_row_is_a_child_of_the_40_pair_parent():
    m, c = M.model("last_row_child", F_CHECK), M.case("last_row_child")
    n = c["xyz"].shape[0]
    assert c["mask"][n - 1] == 0 and c["tag"][n - 1] == "child0" and 40 in _pairs("last_row_child")
    parents = np.nonzero(c["mask"])[0]
    s = parents[int(np.nonzero(m["pairs_of"] == 40)[0][0])]
    assert c["cluster"][s] == c["cluster"][n - 1] == 0


def test_clamps_case_reaches_both_clamps_through_a_subnormal():
    m, c = M.model("clamps", F_CHECK), M.case("clamps")
    assert c["params"]["tau"] == 0.1
    tiny = np.float32(M.FLT_MIN)
    q, t = np.float32(0.25) * tiny, np.float32(0.75) * tiny
    assert 0 < float(q) < M.FLT_MIN and q + t == tiny and float(q / (q + t)) == 0.25          # subnormal, and exact
    w = c["weight"].astype(np.float64)
    parents = np.nonzero(c["mask"])[0]
    seen = {}
    for k, s in enumerate(parents):
        cl = int(c["cluster"][s])
        kids = np.nonzero((c["cluster"] == cl) & (c["mask"] == 0))[0]
        share = (m["weight"][k] - w[s]) / w[kids].sum()
        seen.setdefault(cl, []).append((float(c["weight"][s]), share))
    assert abs(seen[0][0][1] - 1.0) < 1e-12 and seen[0][0][0] == 1.0                         # one giant parent takes its children whole
    for wt, share in seen[1]:                                                               # two giants: 0.25 and 0.75
        assert wt in (0.25, 0.75) and abs(share - wt) < 1e-12, seen[1]
    assert sorted(wt for wt, _ in seen[1]) == [0.25, 0.75]
    hi = np.nonzero(c["tag"] == "hi")[0]
    big = [s for s in parents if c["cluster"][s] == 2]
    assert len(big) == 1 and np.array_equal(c["cov6"][big[0]], np.array([1e6, 0, 0, 1e6, 0, 1e6], np.float32)) and hi.size == 25
    assert m["stats"]["orphans"] == 0 and m["stats"]["dropped"] == 0


def test_zero_weight_parent_follows_the_reference_rules():
    m, c = M.model("zero_weight_parent", F_CHECK), M.case("zero_weight_parent")
    st = m["stats"]
    assert (st["parents"], st["orphans"], st["dropped"], st["n_out"]) == (3, 3, 1, 5)
    assert c["weight"][c["Z"]] == 0.0
    assert sorted(c["tag"][m["orphan_in"]].tolist()) == ["Z", "z_child", "z_child"] and c["Z"] not in m["parent_in"]
    k = int(np.nonzero(m["parent_in"] == c["O"])[0][0])
    mine = np.nonzero(np.isin(c["tag"], ("O", "o_child", "shared")))[0]
    assert abs(m["weight"][k] - c["weight"][mine].astype(np.float64).sum()) < 1e-12            # the shared child goes wholly to O
    assert int(m["pairs_of"][np.nonzero(np.nonzero(c["mask"])[0] == c["Z"])[0][0]]) == 4          # Z, its two children, the shared child


# ------------------------------------------------------------------------------------------------------------------ model = oracle
@pytest.mark.parametrize("name", M.CASES)
def test_counts_and_order_equal_the_oracle(oracle, name):
    m, c = M.model(name, F_CHECK), M.case(name)
    cl = M.cloud(name, F_CHECK)
    lv, st = M.oracle_level(oracle, name, F_CHECK)
    assert {k: st[k] for k in ("parents", "pairs", "orphans", "dropped")} == {k: m["stats"][k] for k in ("parents", "pairs", "orphans", "dropped")}
    assert lv["xyz"].shape[0] == m["stats"]["n_out"]
    p = m["n_parent_rows"]
    for f, src in (("xyz", cl["xyz"]), ("color", cl["color"]), ("cov6", cl["cov6"]), ("opacity", cl["opacity"]), ("sh", cl["sh"]), ("weight", c["weight"])):
        assert np.array_equal(lv[f][p:], src[m["orphan_in"]]), (name, f)                      # orphans: the input rows, in input order
    # parents in parent input order: every row within 1e-5 of its magnitude of the model's row, and nearer to it than to any other
    for f in M.FIELDS:
        r = M.ratio(lv, m, f, rows=p)
        assert r * M.EPS32 < 1e-4, (name, f, r)
    if p > 1:
        d = np.abs(lv["xyz"][:p, None, :].astype(np.float64) - m["xyz"][None, :p, :]).sum(2)
        assert np.array_equal(d.argmin(1), np.arange(p)), name


def test_tolerance_file_is_current(oracle):
    stored, now = M.load_tolerances(), M.tolerances(oracle)
    assert sorted(stored) == sorted(M.CASES)
    for name in M.CASES:
        print(name, " ".join(f"{f} {now[name][f]:.2f}" for f in M.FIELDS))
        assert sorted(stored[name]) == sorted(M.FIELDS)
        for f in M.FIELDS:
            assert abs(now[name][f] - stored[name][f]) <= 1e-3 * stored[name][f] + 1e-6, (name, f, now[name][f], stored[name][f])
            assert 0.0 < stored[name][f] < 1e4                  # a float32 chain: a few roundings to a few thousand (cov6, far from the origin)
    K = M.bound_constants(stored)
    print("small cases:", M.small_cases())
    for name in M.CASES:
        print("K", name, " ".join(f"{f} {K[name][f]:.0f}" for f in M.FIELDS))


# ---------------------------------------------------------------------------------------------------------------------- the teeth
def _parent_with(name, pairs):
    m, c = M.model(name, 45), M.case(name)
    return int(np.nonzero(c["mask"])[0][int(np.nonzero(m["pairs_of"] == pairs)[0][0])])


def _mutations():
    c = M.case("ladder")
    s = _parent_with("ladder", 257)
    kids = np.nonzero((c["cluster"] == c["cluster"][s]) & (c["mask"] == 0))[0]
    far = int(kids[np.argmax(np.abs(np.log(c["weight"][kids])))])
    sh = M.case("shared")
    cl65 = [k for k, (par, _) in enumerate(M.SHARED) if par == 65][0]
    rows = np.nonzero(sh["cluster"] == cl65)[0]
    par65, kid65 = rows[sh["mask"][rows] == 1], rows[sh["mask"][rows] == 0]
    return {"the 2049-pair parent loses its last pair": ("heavy", {"drop_last_pair_of": _parent_with("heavy", 2049)}),
            "a child of the 257-pair parent counts with weight 1": ("ladder", {"unit_weight_child": far}),
            "one of 65 parents missing from a child's sumLw": ("shared", {"sumlw_skip": (int(kid65[0]), int(par65[17]))}),
            "the mean's offset is not taken out of the covariance": ("ladder", {"no_dm": True})}


@pytest.mark.parametrize("what", ["the 2049-pair parent loses its last pair", "a child of the 257-pair parent counts with weight 1",
                                  "one of 65 parents missing from a child's sumLw", "the mean's offset is not taken out of the covariance"])
def test_the_bound_sees_a_subtly_wrong_mstep(what):
    """Each mutation moves some element by at least 10 x the bound test_hem_mstep_gpu.py allows, K 2^-24 mag with the stored K; printed:
    how far the whole-array rule of test_hem_gpu.py (max |got - want| / max |want| < 1e-4) is from seeing it."""
    name, mut = _mutations()[what]
    F = 45
    good, bad = M.model(name, F), M.mutated(name, F, mut)
    K = M.bound_constants()[name]
    assert bad["xyz"].shape == good["xyz"].shape
    worst, whole = {}, {}
    for f in M.FIELDS:
        worst[f] = M.ratio(bad, good, f) / K[f]
        whole[f] = float(np.abs(bad[f] - good[f]).max() / np.abs(good[f]).max()) / 1e-4
    print(what, "| bound ratios", {f: f"{v:.3g}" for f, v in worst.items()})
    print(what, "| whole-array rule, fraction of its 1e-4", {f: f"{v:.3g}" for f, v in whole.items()})
    assert max(worst.values()) >= 10.0, worst
