"""The device .ply path (k_ply_unpack / k_ply_pack of csrc/model.hip, load_gaussian_device / save_gaussian_device of utils/ply_io.py) on
files the project did not write itself: the layouts, header options, covariance families and non-finite rows of tests/ply_model.py, whose
builder and float64 covariance tests/test_ply_layouts_cpu.py checks on the host.

Sizes run: every layout x K in {0, 3, 15, 24} at n = 3 001 with chunk_rows in {default, 7, 1 024, n, n + 5}; chunk_rows = 1 at n = 1 031
(rows of 4k + 3 bytes); the SH scatter at n = 12 001, K = 15 (540 045 floats, above the 524 288 threads of one grid pass) on rows of
4k + 3 bytes; the geometry loop at n = 524 545, K = 0 on rows of 69 bytes, every row compared; 8 x 4 000 covariance rows, laid out
canonical and in rows of 4k + 3 bytes; the writer at n = 4 099, K = 24 and K = 1.

Device covariance against ``cov6_f64``, worst max|d| / trace per family on the MI355X (printed by test_covariance_families, pytest -s;
bar 2e-6 as on the host, where the float32 restatement reaches 8.4e-7); both layouts give the same bits, so one figure each:
    typical 6.49e-07   needle 7.96e-07   flat 8.31e-07   tiny 7.01e-07   huge 6.49e-07   bigquat 5.65e-07   smallquat 6.87e-07   axisquat 1.35e-07
The whole file takes about four seconds there; the slowest test (the 524 545-row geometry loop) 0.3 s.
"""
import ctypes as C
import filecmp

import numpy as np
import pytest
import torch

import ply_model as M
from gaussiansplattingregistration_amd import _lib
from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
from gaussiansplattingregistration_amd.utils import ply_io

pytestmark = pytest.mark.gpu

N = 3001
FIELDS = ("xyz", "color", "sh", "opacity", "scale", "rot")
GSR_E_INVALID = -1
INT32_MAX = 2 ** 31 - 1


def _write(path, head, v):
    with open(path, "wb") as f:
        f.write(head)
        f.write(v.tobytes())
    return path


def _bits(d):
    """the seven arrays of a loader's result as uint32 on the host"""
    return {k: M.bits(d[k].cpu().numpy()) for k in FIELDS + ("cov6",)}


def _assert_columns(got, cols, what):
    for k in FIELDS:
        assert np.array_equal(got[k], M.bits(cols[k])), (what, k)


def _unpack(hip_lib, raw, n, row_bytes, offsets, K):
    """gsr_ply_unpack on `raw` (n rows of row_bytes bytes) without a file -> dict of host arrays"""
    assert len(raw) == n * row_bytes and all(0 <= o <= row_bytes - 4 for o in offsets[:14]) and (K == 0 or 0 <= offsets[14] <= row_bytes - 12 * K)
    rows = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to("cuda:0")
    shape = {"xyz": (n, 3), "color": (n, 3), "sh": (n, 3 * K), "opacity": (n,), "scale": (n, 3), "rot": (n, 4), "cov6": (n, 6)}
    out = {k: torch.full(s, 7.0, dtype=torch.float32, device="cuda:0") for k, s in shape.items()}
    p = lambda k: C.c_void_p(out[k].data_ptr()) if out[k].numel() else None
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(0).cuda_stream
    _lib.check(hip_lib.gsr_ply_unpack(C.c_void_p(rows.data_ptr()), n, row_bytes, (C.c_int32 * 15)(*offsets), K, p("xyz"), p("color"), p("sh"), p("opacity"),
                                      p("scale"), p("rot"), p("cov6"), 0, C.c_void_p(st)), "gsr_ply_unpack")
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


# ---- loader against the builder -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 3, 15, 24))
@pytest.mark.parametrize("kind", M.LAYOUTS)
def test_loader_returns_the_builders_columns(tmp_path, kind, K):
    spec = M.layout(kind, K, seed=K)
    head, v, cols, k = M.build(spec, N, seed=40 + K)
    path = _write(tmp_path / "f.ply", head, v)
    tm = {}
    d = ply_io.load_gaussian_device(path, 0, timing=tm)
    assert d["sh_degree"] == {0: 0, 3: 1, 15: 3, 24: 4}[K] and tm["splats"] == N and tm["bytes"] == N * v.dtype.itemsize
    assert all(d[f].is_cuda and d[f].dtype == torch.float32 for f in FIELDS + ("cov6",)) and d["sh"].shape == (N, 3 * K) and d["cov6"].shape == (N, 6)
    first = _bits(d)
    _assert_columns(first, cols, "default")
    for chunk_rows in (7, 1024, N, N + 5):          # the same row at another address and alignment: the same bits, cov6 included
        again = _bits(ply_io.load_gaussian_device(path, 0, chunk_rows=chunk_rows))
        for f in first:
            assert np.array_equal(again[f], first[f]), (chunk_rows, f)


def test_one_row_per_chunk_on_unaligned_rows(tmp_path):
    n = 1031
    spec = M.layout("row4k3", 3)
    head, v, cols, _ = M.build(spec, n, seed=5)
    path = _write(tmp_path / "f.ply", head, v)
    one = _bits(ply_io.load_gaussian_device(path, 0, chunk_rows=1))
    _assert_columns(one, cols, "chunk_rows=1")
    assert np.array_equal(one["cov6"], _bits(ply_io.load_gaussian_device(path, 0))["cov6"])


def test_sh_scatter_past_one_grid_pass_on_unaligned_rows(tmp_path):
    n, K = 12001, 15
    assert n * 3 * K > 524288
    spec = M.layout("row4k3", K)
    head, v, cols, _ = M.build(spec, n, seed=6)
    assert v.dtype.itemsize % 4 == 3
    _assert_columns(_bits(ply_io.load_gaussian_device(_write(tmp_path / "f.ply", head, v), 0)), cols, "K=15")


def test_geometry_loop_past_one_grid_pass(hip_lib):
    n = 524288 + 257
    spec = M.layout("row4k1", 0)
    head, v, cols, K = M.build(spec, n, seed=7)
    row_bytes, offsets, _ = M.offsets_of(spec)
    assert row_bytes == 69 and K == 0
    got = _unpack(hip_lib, v.tobytes(), n, row_bytes, offsets, 0)
    for f in FIELDS:
        assert np.array_equal(M.bits(got[f]), M.bits(cols[f])), f         # every row
    err = M.cov_error(got["cov6"], cols["scale"], cols["rot"])
    assert (err <= M.COV_BOUND).all(), float(err.max())


# ---- covariance ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def family_cov(tmp_path_factory):
    """cov6 bits of all families in one file, once per layout -> {layout: (n, 6) float32}, and the rows' (scale, rot)"""
    parts = [M.family(f) for f in M.FAMILIES]
    scale, rot = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    out = {}
    for kind in ("canonical", "row4k3"):
        head, v, cols, _ = M.build(M.layout(kind, 0), len(scale), seed=8, scale=scale, rot=rot)
        d = ply_io.load_gaussian_device(_write(tmp_path_factory.mktemp("fam") / f"{kind}.ply", head, v), 0, chunk_rows=5000)
        assert np.array_equal(M.bits(d["scale"].cpu().numpy()), M.bits(scale)) and np.array_equal(M.bits(d["rot"].cpu().numpy()), M.bits(rot))
        out[kind] = d["cov6"].cpu().numpy()
    return out, scale, rot


@pytest.mark.parametrize("name", M.FAMILIES)
def test_covariance_families(family_cov, name):
    cov, scale, rot = family_cov
    i = M.FAMILIES.index(name)
    rows = slice(i * M.FAMILY_ROWS, (i + 1) * M.FAMILY_ROWS)
    assert np.array_equal(M.bits(cov["canonical"][rows]), M.bits(cov["row4k3"][rows]))
    assert np.isfinite(cov["canonical"][rows]).all()
    err = M.cov_error(cov["canonical"][rows], scale[rows], rot[rows])
    print(f"{name}: device max|d| / trace = {err.max():.2e}")
    assert (err <= M.COV_BOUND).all(), (name, float(err.max()))


def test_nonfinite_table(tmp_path):
    """the finiteness pattern of the float32 host reader entry by entry, its values where finite, and finite rows in between untouched"""
    bad_s, bad_q = M.nonfinite_rows()
    m = len(bad_s)
    fin_s, fin_q = M.family("typical", n=m + 1, seed=77)
    scale, rot = np.empty((2 * m + 1, 3), np.float32), np.empty((2 * m + 1, 4), np.float32)
    scale[0::2], rot[0::2], scale[1::2], rot[1::2] = fin_s, fin_q, bad_s, bad_q
    results = {}
    for what, (s, q) in {"mixed": (scale, rot), "finite": (fin_s, fin_q)}.items():
        for kind in ("canonical", "row4k1"):
            head, v, _, _ = M.build(M.layout(kind, 0), len(s), seed=9, scale=s, rot=q, plant=False)
            path = _write(tmp_path / f"{what}_{kind}.ply", head, v)
            results[what, kind] = ply_io.load_gaussian_device(path, 0)["cov6"].cpu().numpy()
            if what == "mixed" and kind == "canonical":
                with np.errstate(all="ignore"):
                    host = ply_io.load_gaussian_arrays(path)["cov6"]
    got = results["mixed", "canonical"]
    assert np.array_equal(M.bits(got), M.bits(results["mixed", "row4k1"]))
    assert np.array_equal(np.isnan(got), np.isnan(host)) and np.array_equal(np.isposinf(got), np.isposinf(host)) and np.array_equal(np.isneginf(got), np.isneginf(host))
    f64 = M.cov6_f64(scale, rot)
    for (what, _, _, want), g, w64 in zip(M.NONFINITE, got[1::2], f64[1::2]):
        if want is None:
            assert np.isfinite(g).all() and np.abs(g - w64).max() <= M.COV_BOUND * (w64[0] + w64[3] + w64[5]), (what, g)
        else:
            want = np.array(want, np.float32)
            assert np.array_equal(np.isfinite(g), np.isfinite(want)) and np.array_equal(np.isnan(g), np.isnan(want)), (what, g)
            fin = np.isfinite(want)
            assert (np.abs(g[fin] - want[fin]) <= M.COV_BOUND * np.abs(want[fin]).sum()).all(), (what, g)
    for kind in ("canonical", "row4k1"):
        assert np.array_equal(M.bits(results["mixed", kind][0::2]), M.bits(results["finite", kind])), kind
    assert (M.cov_error(got[0::2], fin_s, fin_q) <= M.COV_BOUND).all()


# ---- headers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{"comments": True}, {"crlf": True}, {"synonyms": True}, {"face": True},
                                     {"comments": True, "crlf": True, "synonyms": True, "face": True}], ids=lambda o: "+".join(o))
def test_header_options(tmp_path, options):
    head, v, cols, _ = M.build(M.layout("combo", 3, seed=2), 257, seed=12, **options)
    _assert_columns(_bits(ply_io.load_gaussian_device(_write(tmp_path / "f.ply", head, v), 0, chunk_rows=100)), cols, options)


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.unpacks = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "gsr_ply_unpack":
            return fn

        def counted(*a):
            self.unpacks += 1
            return fn(*a)
        return counted


def test_empty_vertex_element_launches_nothing(tmp_path, hip_lib, monkeypatch):
    spy = _CountingLib(hip_lib)
    monkeypatch.setattr(_lib, "load", lambda require_device=False: spy)
    head, v, cols, _ = M.build(M.layout("row4k3", 3), 0, face=True)
    d = ply_io.load_gaussian_device(_write(tmp_path / "empty.ply", head, v), 0)
    assert spy.unpacks == 0 and d["sh_degree"] == 1
    assert {k: tuple(d[k].shape) for k in FIELDS + ("cov6",)} == {"xyz": (0, 3), "color": (0, 3), "sh": (0, 9), "opacity": (0,), "scale": (0, 3), "rot": (0, 4),
                                                                  "cov6": (0, 6)}
    assert all(d[k].is_cuda for k in FIELDS + ("cov6",))
    head, v, cols, _ = M.build(M.layout("row4k3", 3), 10)                    # the spy does count
    ply_io.load_gaussian_device(_write(tmp_path / "ten.ply", head, v), 0, chunk_rows=4)
    assert spy.unpacks == 3


@pytest.mark.parametrize("keep_bytes,there", [(600 * 103 + 50, 600), (512 * 103, 512), (17, 0), (999 * 103 + 102, 999)])
def test_file_cut_short(tmp_path, keep_bytes, there):
    spec = M.layout("combo", 3)
    head, v, _, _ = M.build(spec, 1000, seed=13)
    assert v.dtype.itemsize == 103
    path = tmp_path / "cut.ply"
    path.write_bytes(head + v.tobytes()[:keep_bytes])
    with pytest.raises(ValueError, match=f"cut.ply: expected 1000 vertices, the file ends after {there}$"):
        ply_io.load_gaussian_device(path, 0, chunk_rows=256)
    torch.cuda.synchronize()


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _model_arrays(g):
    return {"xyz": g.get_xyz, "color": g.get_colors, "sh": g.get_spherical_harmonics, "opacity": g.get_raw_opacity, "cov6": g.get_covariance(1),
            "scale": g._scaling, "rot": g._rotation}


def test_model_falls_back_to_the_host_reader_on_a_double_property(tmp_path, monkeypatch):
    spec = [(n, "double" if n == "opacity" else t) for n, t in M.layout("canonical", 3)]
    head, v, cols, _ = M.build(spec, 501, seed=14)
    path = str(_write(tmp_path / "d.ply", head, v))
    with pytest.raises(ValueError, match="opacity is not float32"):
        ply_io.load_gaussian_device(path, 0)
    calls = []
    host_reader = ply_io.load_gaussian_arrays
    monkeypatch.setattr(ply_io, "load_gaussian_arrays", lambda p: calls.append(p) or host_reader(p))
    g = GaussianModel("cuda:0").from_ply(path)
    assert len(calls) == 1 and g.get_xyz.is_cuda and g.sh_degree == 1
    c = GaussianModel("cpu").from_ply(path)
    for (k, a), b in zip(_model_arrays(g).items(), _model_arrays(c).values()):
        assert a.is_cuda and not b.is_cuda and np.array_equal(M.bits(a.cpu().numpy()), M.bits(b.numpy())), k
    for k in FIELDS:
        assert np.array_equal(M.bits(_model_arrays(g)[k].cpu().numpy()), M.bits(cols[k])), k


def test_model_stays_on_the_device_path_on_a_permuted_unaligned_file(tmp_path, monkeypatch):
    head, v, cols, _ = M.build(M.layout("combo", 8, seed=4), 501, seed=15)
    path = str(_write(tmp_path / "p.ply", head, v))

    def refuse(p):
        raise AssertionError("the host reader was called")
    monkeypatch.setattr(ply_io, "load_gaussian_arrays", refuse)
    g = GaussianModel("cuda:0").from_ply(path)
    assert g.sh_degree == 2 and len(g) == 501
    for k in FIELDS:
        a = _model_arrays(g)[k]
        assert a.is_cuda and np.array_equal(M.bits(a.cpu().numpy()), M.bits(cols[k])), k
    assert (M.cov_error(g.get_covariance(1).cpu().numpy(), cols["scale"], cols["rot"]) <= M.COV_BOUND).all()


# ---- gsr_ply_unpack's own argument checks (n = 0: nothing is launched) ----------------------------------------------------------
def _check_args(hip_lib, row_bytes, offsets, K):
    assert torch.cuda.is_available()
    return hip_lib.gsr_ply_unpack(None, 0, row_bytes, (C.c_int32 * 15)(*offsets), K, None, None, None, None, None, None, None, 0, None)


def test_unpack_refuses_offsets_outside_the_row(hip_lib):
    rb0, base0, _ = M.offsets_of(M.layout("canonical", 0))
    rb3, base3, _ = M.offsets_of(M.layout("canonical", 3))
    assert (rb0, rb3, base3[14]) == (68, 104, 36)
    assert _check_args(hip_lib, rb0, base0, 0) == 0 and _check_args(hip_lib, rb3, base3, 3) == 0
    put = lambda base, i, o: base[:i] + [o] + base[i + 1:]
    for i in range(14):
        for bad in (INT32_MAX, INT32_MAX - 3, INT32_MAX - 4, rb0 - 3, rb0, -1, -(2 ** 31)):
            assert _check_args(hip_lib, rb0, put(base0, i, bad), 0) == GSR_E_INVALID, (i, bad)
            assert b"outside the 68-byte row" in hip_lib.gsr_last_error()
        assert _check_args(hip_lib, rb0, put(base0, i, rb0 - 4), 0) == 0, i
    # the f_rest block: 12 K bytes from offsets[14]
    assert _check_args(hip_lib, rb3, put(base3, 14, 0), 200_000_000) == GSR_E_INVALID          # 12 K wraps in 32 bits
    assert _check_args(hip_lib, rb3, put(base3, 14, 0), 178_956_971) == GSR_E_INVALID          # 12 K = 2^31 + 4 -> negative in 32 bits
    assert _check_args(hip_lib, rb3, put(base3, 14, 0), 1025) == GSR_E_INVALID
    assert _check_args(hip_lib, rb3, put(base3, 14, 0), -1) == GSR_E_INVALID
    for bad in (rb3 + 4 - 36, rb3 - 35, INT32_MAX, INT32_MAX - 35, -1):
        assert _check_args(hip_lib, rb3, put(base3, 14, bad), 3) == GSR_E_INVALID, bad
    assert _check_args(hip_lib, rb3, put(base3, 14, rb3 - 36), 3) == 0                          # rest0 + 12 K = row_bytes
    assert _check_args(hip_lib, 12 * 1024 + 56, [4 * j for j in range(14)] + [56], 1024) == 0   # the largest K
    for any_ in (INT32_MAX, -1, rb0, -(2 ** 31)):                                               # K = 0: offsets[14] is not read
        assert _check_args(hip_lib, rb0, put(base0, 14, any_), 0) == 0, any_
    assert _check_args(hip_lib, 0, base0, 0) == GSR_E_INVALID and _check_args(hip_lib, -68, base0, 0) == GSR_E_INVALID


# ---- writer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (24, 1))
def test_writer_at_other_sh_sizes(tmp_path, hip_lib, K):
    n = 4099
    _, v, cols, _ = M.build(M.layout("canonical", K), n, seed=16 + K)
    want = tmp_path / "host.ply"
    ply_io.save_gaussian_ply(want, *(cols[k] for k in FIELDS))
    d = {k: torch.from_numpy(cols[k]).to("cuda:0") for k in FIELDS}
    for chunk_rows in (1024, n):
        got = tmp_path / f"device_{chunk_rows}.ply"
        ply_io.save_gaussian_device(got, *(d[k] for k in FIELDS), chunk_rows=chunk_rows)
        assert filecmp.cmp(want, got, shallow=False), chunk_rows
        raw = got.read_bytes()
        file_v = ply_io.read_ply_vertices(got)
        for name in v.dtype.names:
            if name not in ("nx", "ny", "nz"):
                assert np.array_equal(M.bits(file_v[name]), M.bits(v[name])), name
            else:
                assert not M.bits(file_v[name]).any()
        if K == 24:
            back = _bits(ply_io.load_gaussian_device(got, 0, chunk_rows=chunk_rows))
        else:       # three f_rest properties are no SH degree: the loaders refuse the file, the kernel reads its rows all the same
            with pytest.raises(ValueError, match="f_rest"):
                ply_io.load_gaussian_device(got, 0)
            row_bytes, offsets, _ = M.offsets_of(M.layout("canonical", K))
            back = {k: M.bits(a) for k, a in _unpack(hip_lib, raw[len(raw) - n * row_bytes:], n, row_bytes, offsets, K).items()}
        _assert_columns(back, cols, (K, chunk_rows))
