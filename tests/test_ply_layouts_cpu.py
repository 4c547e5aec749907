""".ply files of foreign layouts on the host: the file builder and the float64 covariance of tests/ply_model.py decide by themselves what a
loader must return, and the host readers agree with them.  tests/test_ply_layouts_gpu.py then holds the device loader to the same model.

Host reader's float32 covariance against ``cov6_f64``, worst max|d| / trace per family (4 000 rows, seed 20240; bar 2e-6, the bar
of test_device_loader_equals_host_reader):
    typical 6.49e-07   needle 7.96e-07   flat 7.29e-07   tiny 8.37e-07   huge 6.49e-07   bigquat 5.73e-07   smallquat 6.87e-07   axisquat 2.28e-07
(printed by test_cov6_f64_against_the_host_reader, pytest -s): a float32 restatement of the formula uses less than half of the bar.
"""
import numpy as np
import pytest

import ply_model as M
from gaussiansplattingregistration_amd.utils import ply_io

N = 257
HEADER_OPTIONS = [{}, {"comments": True}, {"crlf": True}, {"synonyms": True}, {"face": True},
                  {"comments": True, "crlf": True, "synonyms": True, "face": True}]


def _write(path, head, v):
    with open(path, "wb") as f:
        f.write(head)
        f.write(v.tobytes())
    return path


def _check_host_readers(path, v, cols, K):
    got = ply_io.read_ply_vertices(path)
    assert got.dtype == v.dtype and got.tobytes() == v.tobytes()
    d = ply_io.load_gaussian_arrays(path)
    assert d["sh_degree"] == {0: 0, 3: 1, 8: 2, 15: 3, 24: 4}[K]
    for k, want in cols.items():
        assert d[k].shape == want.shape and np.array_equal(M.bits(d[k]), M.bits(want)), k


@pytest.mark.parametrize("K", M.KS)
@pytest.mark.parametrize("kind", M.LAYOUTS)
def test_host_readers_return_the_builders_columns(tmp_path, kind, K):
    spec = M.layout(kind, K, seed=K)
    head, v, cols, k = M.build(spec, N, seed=3 + K)
    assert k == K and v.dtype.itemsize % 4 == {"row4k1": 1, "row4k2": 2, "row4k3": 3, "combo": 3}.get(kind, 0)
    if K:                                       # the transpose, spelled out: coefficient k, channel c <- f_rest_(c K + k)
        assert np.array_equal(M.bits(cols["sh"].reshape(N, K, 3)[:, K - 1, 1]), M.bits(v[f"f_rest_{1 * K + K - 1}"]))
    _check_host_readers(_write(tmp_path / "f.ply", head, v), v, cols, K)


@pytest.mark.parametrize("options", HEADER_OPTIONS, ids=lambda o: "+".join(o) or "plain")
@pytest.mark.parametrize("kind", ("canonical", "combo"))
def test_host_readers_take_the_header_options(tmp_path, kind, options):
    spec = M.layout(kind, 3, seed=1)
    head, v, cols, K = M.build(spec, N, seed=11, **options)
    assert (b"\r\n" in head) == bool(options.get("crlf")) and (b"float32" in head) == bool(options.get("synonyms"))
    path = _write(tmp_path / "f.ply", head, v)
    _check_host_readers(path, v, cols, K)
    assert ply_io.read_ply_property_names(path) == tuple(n for n, _ in spec)


def test_empty_vertex_element(tmp_path):
    spec = M.layout("row4k3", 3)
    head, v, cols, K = M.build(spec, 0, face=True)
    path = _write(tmp_path / "f.ply", head, v)
    assert ply_io.read_ply_vertices(path).shape == (0,)
    d = ply_io.load_gaussian_arrays(path)
    assert d["xyz"].shape == (0, 3) and d["sh"].shape == (0, 9) and d["cov6"].shape == (0, 6) and d["opacity"].shape == (0,)


# ---- covariance -------------------------------------------------------------------------------------------------------------------
def _host_cov(tmp_path, scale, rot):
    head, v, cols, _ = M.build(M.layout("nonormals", 0), len(scale), seed=1, scale=scale, rot=rot, plant=False)
    with np.errstate(all="ignore"):
        d = ply_io.load_gaussian_arrays(_write(tmp_path / "c.ply", head, v))
    assert np.array_equal(M.bits(d["scale"]), M.bits(scale)) and np.array_equal(M.bits(d["rot"]), M.bits(rot))
    return d["cov6"]


@pytest.mark.parametrize("name", M.FAMILIES)
def test_cov6_f64_against_the_host_reader(tmp_path, name):
    scale, rot = M.family(name)
    assert scale.shape == (M.FAMILY_ROWS, 3) and scale.dtype == rot.dtype == np.float32
    want = M.cov6_f64(scale, rot)
    assert np.isfinite(want).all() and (want[:, [0, 3, 5]] > 0).all()
    err = M.cov_error(_host_cov(tmp_path, scale, rot), scale, rot)
    print(f"{name}: host reader max|d| / trace = {err.max():.2e}")
    assert (err <= M.COV_BOUND).all(), (name, float(err.max()))


def test_the_families_are_what_they_are_called():
    lo, hi = {}, {}
    for name in M.FAMILIES:
        s, q = M.family(name)
        s.sort(1)
        lo[name], hi[name] = s[:, 0], s[:, 2]
        nq = np.linalg.norm(q.astype(np.float64), axis=1)
        if name == "bigquat":
            assert (nq > 1e14).all() and np.isfinite(q).all()
        elif name == "smallquat":
            assert (nq < 1e-14).all() and (nq > 0).all()
        else:
            assert (nq > 1e-3).all()
        if name == "needle":
            assert (s[:, 2] >= -1).all() and (s[:, 1] <= -9).all() and (s[:, 0] >= -12).all()
        if name == "flat":
            assert (s[:, 1] >= -1).all() and (s[:, 0] <= -10).all() and (s[:, 0] >= -14).all()
        if name == "axisquat":
            assert ((q == 0).sum(1) == 3).all() and (np.abs(q).sum(1) == 1).all() and len(np.unique(q, axis=0)) == 8
    assert hi["tiny"].max() <= -15 and lo["tiny"].min() >= -20 and lo["huge"].min() >= 15 and hi["huge"].max() <= 20


def test_nonfinite_table_on_the_host(tmp_path):
    scale, rot = M.nonfinite_rows()
    got = _host_cov(tmp_path, scale, rot)
    f64 = M.cov6_f64(scale, rot)
    for (what, _, _, want), g, w64 in zip(M.NONFINITE, got, f64):
        if want is None:
            assert np.isfinite(g).all() and (np.abs(g - w64).max() <= M.COV_BOUND * (w64[0] + w64[3] + w64[5])), (what, g)
        else:
            assert np.array_equal(g, np.array(want, np.float32), equal_nan=True), (what, g)
    assert {"zero quaternion", "NaN in the quaternion", "infinity in the quaternion", "NaN scale", "scales -104"} <= {r[0] for r in M.NONFINITE}


# ---- what the device loader refuses, without a device -------------------------------------------------------------------------
def _props(spec):
    return [(n, M.NP_OF[t]) for n, t in spec]


@pytest.mark.parametrize("K", M.KS)
@pytest.mark.parametrize("kind", M.LAYOUTS)
def test_device_layout_equals_the_numpy_dtype(kind, K):
    spec = M.layout(kind, K, seed=K)
    assert ply_io._device_layout("binary_little_endian", _props(spec)) == M.offsets_of(spec)


def test_device_layout_refusals():
    ok = M.layout("canonical", 3)
    lay = lambda spec, fmt="binary_little_endian", first=True: ply_io._device_layout(fmt, _props(spec), first, "some.ply")
    assert lay(ok) == (4 * 26, [0, 4, 8, 24, 28, 32, 72, 76, 80, 84, 88, 92, 96, 100, 36], 3)
    with pytest.raises(ValueError, match="binary little-endian"):
        lay(ok, fmt="ascii")
    with pytest.raises(ValueError, match="binary little-endian"):
        lay(ok, fmt="binary_big_endian")
    with pytest.raises(ValueError, match="vertex element first"):
        lay(ok, first=False)
    for name in ("x", "opacity", "rot_3", "scale_1", "f_dc_2"):
        with pytest.raises(ValueError, match=f"some.ply: property {name} is not float32"):
            lay([(n, "double" if n == name else t) for n, t in ok])
        with pytest.raises(ValueError, match=f"missing property {name}"):
            lay([(n, t) for n, t in ok if n != name])
    i = [n for n, _ in ok].index("f_rest_4")
    with pytest.raises(ValueError, match="consecutive float32"):                # something between f_rest_3 and f_rest_4
        lay(ok[:i] + [("gap", "float")] + ok[i:])
    with pytest.raises(ValueError, match="consecutive float32"):                # the block out of order
        lay(ok[:i] + [ok[i + 1], ok[i]] + ok[i + 2:])
    with pytest.raises(ValueError, match="consecutive float32"):                # one of them a double
        lay([(n, "double" if n == "f_rest_4" else t) for n, t in ok])
    for K3 in (1, 3, 6, 10, 44, 46):                                            # not 3 ((d + 1)^2 - 1)
        spec = [p for p in M.layout("canonical", 0) if p[0] != "opacity"] + [(f"f_rest_{j}", "float") for j in range(K3)] + [("opacity", "float")]
        with pytest.raises(ValueError, match="f_rest"):
            lay(spec)
    # an unneeded property may have any type
    assert lay([("flag", "uchar")] + ok + [("stamp", "double")])[0] == 4 * 26 + 9


def test_header_refusals(tmp_path):
    head = M.header(M.layout("canonical", 0), 1)
    cases = {"list in the vertex element": head.replace(b"property float nx\n", b"property list uchar int nx\n"),
             "truncated header": head[: head.index(b"end_header")],
             "no magic": head[1:]}
    for what, text in cases.items():
        p = tmp_path / "h.ply"
        p.write_bytes(text)
        with pytest.raises(ValueError, match="h.ply"):
            with open(p, "rb") as f:
                ply_io._read_header(f, p)
    # a vertex element that is not the first one is reported as such, not refused, by the header reader
    p = tmp_path / "second.ply"
    p.write_bytes(head.replace(b"element vertex 1\n", b"element camera 0\nproperty float fov\nelement vertex 1\n"))
    with open(p, "rb") as f:
        fmt, n, props, first = ply_io._read_header(f, p)
    assert (fmt, n, first) == ("binary_little_endian", 1, False) and props[0] == ("x", "f4") and len(props) == 17
    with pytest.raises(ValueError, match="vertex element first"):
        ply_io._device_layout(fmt, props, first, p)


@pytest.mark.parametrize("type_name", ["half", "float16", "long", "float128", "FLOAT"])
def test_unknown_property_type_is_a_value_error(tmp_path, type_name):
    """(KeyError before: GaussianModel.from_ply catches ValueError alone when it falls back to the host reader)"""
    spec = M.layout("canonical", 0)
    head = M.header(spec, 1).replace(b"property float nx\n", f"property {type_name} nx\n".encode())
    p = tmp_path / "foreign.ply"
    p.write_bytes(head + bytes(M.dtype_of(spec).itemsize))
    for reader in (ply_io.read_ply_vertices, ply_io.load_gaussian_arrays, ply_io.read_ply_property_names):
        with pytest.raises(ValueError, match=f"foreign.ply.*{type_name}"):
            reader(p)
    from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel
    with pytest.raises(ValueError, match=type_name):
        GaussianModel("cpu").from_ply(str(p))
    p.write_bytes(head.replace(b" nx\n", b"\n"))                                 # a property line without a name
    with pytest.raises(ValueError, match="foreign.ply"):
        ply_io.read_ply_property_names(p)
