"""Test model of the 3DGS .ply files the loaders must read, in plain numpy (no GPU, no project imports).

A FILE BUILDER: a layout is an ordered list of (property name, ply type name); ``build`` fills a structured array of that layout from a
seed and returns the header bytes, the array (``header + v.tobytes()`` is the file) and the wanted columns as the float32 arrays a loader
must hand back -- bit for bit, they are copies.  Built on ``numpy.dtype`` and ``tobytes`` alone, so it says independently of
``utils/ply_io.py`` what the bytes of a file mean.

A COVARIANCE REFERENCE: ``cov6_f64`` computes R diag(exp s)^2 R^T in float64 from the float32 scale and quaternion; ``families`` draws the
(scale, quaternion) rows it is tried on, and ``NONFINITE`` is a hand-written table of rows whose float32 result is not finite (or only
just), with the result float32 arithmetic gives.
"""
import numpy as np

NP_OF = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8"}
SYNONYM = {"float": "float32", "uchar": "uint8", "short": "int16", "double": "float64"}
GEOM = ["x", "y", "z", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
LAYOUTS = ("canonical", "nonormals", "permuted", "padded", "row4k1", "row4k2", "row4k3", "combo")
UNALIGNED = ("row4k1", "row4k2", "row4k3", "combo")
KS = (0, 3, 8, 15, 24)


def _f(names):
    return [(n, "float") for n in names]


def layout(kind, K, seed=0):
    """-> [(name, ply type)] of the vertex element"""
    rest = _f([f"f_rest_{i}" for i in range(3 * K)])
    xyz, nrm, dc, tail = _f(["x", "y", "z"]), _f(["nx", "ny", "nz"]), _f(["f_dc_0", "f_dc_1", "f_dc_2"]), _f(GEOM[6:])
    if kind == "canonical":                     # what save_gaussian_ply writes
        return xyz + nrm + dc + rest + tail
    if kind == "nonormals":
        return xyz + dc + rest + tail
    if kind in ("permuted", "combo"):           # the 14 wanted properties shuffled, the f_rest block whole in the middle
        order = [GEOM[i] for i in np.random.default_rng(1000 + seed).permutation(14)]
        spec = _f(order[:7]) + rest + _f(order[7:])
        if kind == "combo":                     # + 1 + 2 + 8 bytes: rows of 4k + 3 bytes, the block at an odd offset
            spec = [("flag", "uchar")] + spec[:4] + [("tag", "short")] + spec[4:-2] + [("stamp", "double")] + spec[-2:]
        return spec
    if kind == "padded":                        # more float properties before, between and after
        return _f(["pad_a"]) + xyz + nrm + _f(["pad_b", "pad_c"]) + dc + rest + _f(["pad_d"]) + tail + _f(["pad_e"])
    if kind == "row4k1":                        # a uchar first: every wanted offset is odd
        return [("flag", "uchar")] + xyz + nrm + dc + rest + tail
    if kind == "row4k2":                        # a short in the middle: x y z f_dc aligned in even rows, the rest never
        return xyz + nrm + dc + [("tag", "short")] + rest + tail
    if kind == "row4k3":                        # a uchar, a short and a double spread out: 11 bytes more
        return [("flag", "uchar")] + xyz + nrm + [("tag", "short")] + dc + rest + _f(["opacity"]) + [("stamp", "double")] + _f(GEOM[7:])
    raise KeyError(kind)


def dtype_of(spec):
    """the packed little-endian structured dtype of a layout"""
    return np.dtype([(n, "<" + NP_OF[t]) for n, t in spec])


def header(spec, n, comments=False, crlf=False, synonyms=False, face=False, fmt="binary_little_endian"):
    """header bytes: optional ``comment`` / ``obj_info`` lines, CRLF line ends, the type synonyms, a trailing empty face element"""
    lines = ["ply", f"format {fmt} 1.0"]
    if comments:
        lines += ["comment made by tests/ply_model.py", "obj_info element vertex 7 is not an element", "comment property float x"]
    lines.append(f"element vertex {n}")
    for i, (name, t) in enumerate(spec):
        lines.append(f"property {SYNONYM.get(t, t) if synonyms else t} {name}")
        if comments and i == 2:
            lines.append("comment between two properties")
    if face:
        lines += ["element face 0", "property list uchar int vertex_indices"]
    lines.append("end_header")
    eol = "\r\n" if crlf else "\n"
    return (eol.join(lines) + eol).encode("ascii")


def build(spec, n, seed=0, scale=None, rot=None, plant=True, **header_options):
    """-> (header bytes, structured array, {"xyz", "color", "sh", "opacity", "scale", "rot"} float32, K).  ``sh`` is (n, 3K)
    coefficient-major as the model keeps it: sh[i, 3 k + c] = f_rest_(c K + k) of row i.  ``scale`` / ``rot``: use these rows instead of
    seeded ones.  ``plant``: -0.0, a denormal, +inf and a NaN with a payload in SH / DC entries (the bits travel, not the values)."""
    rng = np.random.default_rng(seed)
    v = np.zeros(n, dtype_of(spec))
    for name, t in spec:
        if NP_OF[t][0] == "f":
            v[name] = rng.normal(size=n).astype(NP_OF[t])
        else:
            info = np.iinfo(NP_OF[t])
            v[name] = rng.integers(info.min, info.max, size=n, endpoint=True)
    if scale is not None:
        for a in range(3):
            v[f"scale_{a}"] = scale[:, a]
    if rot is not None:
        for a in range(4):
            v[f"rot_{a}"] = rot[:, a]
    K3 = sum(1 for name, _ in spec if name.startswith("f_rest_"))
    K = K3 // 3
    if plant and n >= 4:
        special = np.array([0x80000000, 0x000002CA, 0x7F800000, 0x7FC12345], np.uint32).view(np.float32)
        for i, (name, s) in enumerate(zip(["f_rest_0", f"f_rest_{K3 - 1}", f"f_rest_{K3 // 2}", "f_dc_1"] if K3 else ["f_dc_0", "f_dc_1", "f_dc_2", "f_dc_1"], special)):
            v[name][(i * 7 + 1) % n] = s
    col = lambda names: np.ascontiguousarray(np.stack([v[k] for k in names], 1).astype(np.float32))
    sh = col([f"f_rest_{c * K + k}" for k in range(K) for c in range(3)]) if K else np.zeros((n, 0), np.float32)
    cols = {"xyz": col(["x", "y", "z"]), "color": col(GEOM[3:6]), "sh": sh, "opacity": np.ascontiguousarray(v["opacity"].astype(np.float32)),
            "scale": col(GEOM[7:10]), "rot": col(GEOM[10:14])}
    return header(spec, n, **header_options), v, cols, K


def offsets_of(spec):
    """-> (row_bytes, the 15 byte offsets gsr_ply_unpack takes, K) straight from the numpy dtype"""
    dt = dtype_of(spec)
    K3 = sum(1 for name, _ in spec if name.startswith("f_rest_"))
    return dt.itemsize, [dt.fields[k][1] for k in GEOM] + [dt.fields["f_rest_0"][1] if K3 else 0], K3 // 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


# ---- covariance -----------------------------------------------------------------------------------------------------------------
def cov6_f64(scale, rot):
    """R diag(exp s)^2 R^T (xx xy xz yy yz zz) in float64 from float32 inputs: the quaternion normalised in float64, build_rotation,
    L = R diag(exp s), L L^T"""
    s = np.asarray(scale, np.float32).astype(np.float64)
    q = np.asarray(rot, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
        w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.empty((len(q), 3, 3))
        R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
        R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
        R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
        L = R * np.exp(s)[:, None, :]
        C = L @ L.transpose(0, 2, 1)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)


FAMILIES = ("typical", "needle", "flat", "tiny", "huge", "bigquat", "smallquat", "axisquat")
FAMILY_ROWS, FAMILY_SEED = 4000, 20240
COV_BOUND = 2e-6            # times the trace, per row on the largest entry: the bound of test_device_loader_equals_host_reader


def family(name, n=FAMILY_ROWS, seed=FAMILY_SEED):
    """-> (scale (n,3), rot (n,4)) float32"""
    rng = np.random.default_rng(seed + FAMILIES.index(name))
    scale = rng.normal(-2.5, 0.5, (n, 3))
    rot = rng.normal(size=(n, 4))
    if name in ("needle", "flat"):
        long_ = rng.uniform(-1, 0, (n, 3))
        short = rng.uniform(-12, -9, (n, 3)) if name == "needle" else rng.uniform(-14, -10, (n, 3))
        axis = rng.integers(0, 3, n)
        pick = np.arange(3)[None, :] == axis[:, None]           # needle: the picked axis is long; flat: the picked axis is short
        scale = np.where(pick, long_, short) if name == "needle" else np.where(pick, short, long_)
    elif name == "tiny":
        scale = rng.uniform(-20, -15, (n, 3))
    elif name == "huge":
        scale = rng.uniform(15, 20, (n, 3))
    elif name == "bigquat":
        rot = rot * 1e15
    elif name == "smallquat":
        rot = rot * 1e-15
    elif name == "axisquat":
        rot = np.zeros((n, 4))
        rot[np.arange(n), rng.integers(0, 4, n)] = rng.choice([-1.0, 1.0], n)
    return scale.astype(np.float32), rot.astype(np.float32)


def cov_error(got, scale, rot):
    """per row: max |got - cov6_f64| / trace of cov6_f64"""
    want = cov6_f64(scale, rot)
    return np.abs(np.asarray(got, np.float64) - want).max(1) / (want[:, 0] + want[:, 3] + want[:, 5])


_N, _I = np.nan, np.inf
_NAN6 = [_N] * 6
# (what, scale, quaternion, float32 result: six values, or None = "all six finite")
NONFINITE = [
    ("zero quaternion", [0, 0, 0], [0, 0, 0, 0], _NAN6),
    ("NaN in the quaternion", [-1, -2, -3], [0.5, _N, 0.5, 0.5], _NAN6),
    ("infinity in the quaternion", [-1, -2, -3], [_I, 0, 0, 0], _NAN6),
    ("-infinity in the quaternion", [-1, -2, -3], [0.3, 0.1, -_I, 0.2], _NAN6),
    ("NaN scale", [-1, _N, -3], [0.9, 0.1, -0.2, 0.3], _NAN6),
    ("scale 89, identity quaternion", [89, 0, 0], [1, 0, 0, 0], [_I, _N, _N, _N, _N, _N]),      # exp(89) = inf; 0 * inf off the diagonal
    ("quaternion 1e-23: the squares underflow", [0, 0, 0], [1e-23, 0, 0, 0], _NAN6),             # |q| = 0: inf and 0 / 0
    ("quaternion (1e20, 1, 0, 0): the norm overflows", [0, 0, 0], [1e20, 1, 0, 0], [1, 0, 0, 1, 0, 1]),     # q / inf = 0, R = I
    ("scales -104", [-104, -104, -104], [0.9, 0.1, -0.2, 0.3], [0] * 6),                         # exp(-104) rounds to 0
    ("scale -inf on one axis", [-1, -_I, -2], [0.9, 0.1, -0.2, 0.3], None),
]


def nonfinite_rows():
    """-> (scale (m,3), rot (m,4)) float32 of the table"""
    return (np.array([r[1] for r in NONFINITE], np.float32), np.array([r[2] for r in NONFINITE], np.float32))
