"""gaussiansplattingregistration_amd/_model_view.py without a GPU: the field table, K and the scaling / rot test of a model, the
views and result models the fronts build from them, and the refusals of models that do not go into one call."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gaussiansplattingregistration_amd import _lib, _model_view as mv
from gaussiansplattingregistration_amd.models.gaussian_model import GaussianModel

DEGREE = {0: 0, 3: 1, 15: 3}
WIDTH = {"xyz": 3, "cov6": 6, "dc": 3, "opacity": 1, "scaling": 3, "rot": 4}


def make(n, K, with_sr, seed=0):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.random(shape).astype(np.float32)
    g = GaussianModel("cpu").from_arrays(f(n, 3), f(n, 3), f(n, 1), f(n, 6), f(n, K, 3), DEGREE[K])
    if with_sr:
        g._scaling, g._rotation = torch.from_numpy(f(n, 3)), torch.from_numpy(f(n, 4))
    return g


def test_field_table():
    assert [f for f, _, _ in mv.FIELDS] == [name for name, _ in _lib.ModelView._fields_[1:]]          # the order of gsr_model_view
    assert all(hasattr(GaussianModel("cpu"), a) for a in mv.ATTRS) and len(set(mv.ATTRS)) == 7
    assert [w for _, _, w in mv.carried(15, True)] == [3, 6, 3, 45, 1, 3, 4]
    assert [f for f, _, _ in mv.carried(0, False)] == ["xyz", "cov6", "dc", "opacity"]
    assert [f for f, _, _ in mv.carried(3, True, fields=("xyz", "rot"))] == ["xyz", "rot"]


@pytest.mark.parametrize("with_sr", [False, True])
@pytest.mark.parametrize("K", [0, 3, 15])
@pytest.mark.parametrize("n", [0, 5])
def test_view_and_model(n, K, with_sr):
    g = make(n, K, with_sr)
    assert mv.sh_count(g) == K and mv.has_scaling_rot(g) == (with_sr and n > 0)
    sr = with_sr and n > 0
    keep = []
    v = mv.view_of(g, K, sr, 0, False, keep)
    assert v.n == n
    carried = {f: (a, w) for f, a, w in mv.carried(K, sr)}
    for field, attr, _ in mv.FIELDS:
        p = getattr(v, field)
        if n == 0 or field not in carried:
            assert not p, field                                     # NULL: a model without rows carries no array
            continue
        w = carried[field][1]
        assert w == (3 * K if field == "sh" else WIDTH[field])
        got = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n, w))
        assert np.array_equal(got, getattr(g, attr).numpy().reshape(n, w)), field
    assert len(keep) == (len(carried) if n else 0)
    # the views of an output and the model on its first rows
    vo, arrays = mv.out_view(n + 2, K, sr, 0, False)
    assert vo.n == n + 2 and set(arrays) == {a for a, _ in carried.values()}
    for field, (attr, w) in carried.items():
        assert arrays[attr].shape == (n + 2, w) and getattr(vo, field) == arrays[attr].ctypes.data
        arrays[attr][:n] = getattr(g, attr).numpy().reshape(n, w)
    m = mv.model_from_arrays(arrays, n, K, g.sh_degree, "cpu")
    assert len(m) == n and m.sh_degree == g.sh_degree and mv.sh_count(m) == K and mv.has_scaling_rot(m) == sr
    assert m._features_dc.shape == (n, 1, 3) and m._features_rest.shape == (n, K, 3) and m._opacity.shape == (n, 1)
    for attr in mv.ATTRS:
        if attr in arrays:
            assert torch.equal(getattr(m, attr), getattr(g, attr)), attr
            assert n == 0 or getattr(m, attr).data_ptr() == arrays[attr].ctypes.data            # a view, no copy
    if not sr:
        assert m._scaling.numel() == 0 and m._rotation.numel() == 0
    assert mv.layout([g, m]) == (K, sr) and mv.placement([g, m]) == (False, 0)


def test_view_of_some_fields():
    g = make(5, 3, True)
    v = mv.view_of(g, 0, False, 0, False, [], fields=("xyz", "cov6", "dc", "opacity"))
    assert v.xyz and v.cov6 and v.dc and v.opacity and not v.sh and not v.scaling and not v.rot


def test_models_that_do_not_go_into_one_call():
    a, b = make(5, 3, True), make(5, 15, True)
    b.sh_degree = a.sh_degree
    with pytest.raises(RuntimeError):
        mv.layout([a, b])                                           # mixed K
    with pytest.raises(RuntimeError):
        mv.layout([make(5, 3, True), make(5, 3, False)])            # scaling / rot in one model only
    assert mv.layout([make(5, 3, True), make(0, 3, False)]) == (3, True)        # a model without rows decides nothing
    # mixed host / device: placement reads where _xyz lives, so stand-ins do for models on devices this machine may not have
    at = lambda name: SimpleNamespace(_xyz=SimpleNamespace(is_cuda=name != "cpu", device=torch.device(name)))
    assert mv.placement([a, a]) == (False, 0) and mv.placement([at("cuda:1"), at("cuda:1")]) == (True, 1)
    for models in ([at("cpu"), at("cuda:0")], [at("cuda:0"), at("cpu")], [at("cuda:0"), at("cuda:1")], [at("cpu"), at("cpu"), at("cuda:0")]):
        with pytest.raises(RuntimeError):
            mv.placement(models)
