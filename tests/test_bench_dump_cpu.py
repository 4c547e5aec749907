"""bench.dump_outputs (what `bench.py --dump-outputs DIR` writes) on host tensors shaped like the bench's step: float32 / float64 files
only, a seeded sample of rows that depends on nothing but the level's size, column sums over all rows, under 64 MB at the headline size."""
import numpy as np
import torch

import bench


def _last(sizes, n0, fill):
    def level(n, normals):
        d = {"xyz": fill(n, 3), "color": fill(n, 3), "cov6": fill(n, 6), "opacity": fill(n), "sh": fill(n, 45)}
        if normals:
            d["normals"] = fill(n, 3).double()
        return d
    outputs = [{"levels": [level(n, False) for n in sizes], "normals0": None},
               {"levels": [level(n, True) for n in sizes], "normals0": fill(n0, 3).double()}]
    entries = [{"T": np.eye(4) + 0.01 * k, "iterations": 50 - k, "fitness": 0.9 + 0.01 * k, "rmse": 0.1 - 0.01 * k} for k in range(4)]
    return {"outputs": outputs, "levels": entries, "T": entries[-1]["T"]}


def test_dump_at_the_headline_size_stays_under_64_mb(tmp_path):
    names = bench.dump_outputs(str(tmp_path), _last((1_668_351, 556_000, 185_000), 5_000_000, lambda *s: torch.zeros(s)))
    files = sorted(tmp_path.iterdir())
    assert sorted(f.stem for f in files) == names
    assert sum(f.stat().st_size for f in files) < 64 << 20
    for f in files:
        assert np.load(f).dtype in (np.float32, np.float64), f.name
    assert np.load(tmp_path / "source_level1_sh.npy").shape == (bench.DUMP_ROWS, 45)
    assert np.load(tmp_path / "target_level0_normals.npy").shape == (bench.DUMP_ROWS, 3)
    assert np.array_equal(np.load(tmp_path / "level_sizes.npy"), [[1_668_351, 556_000, 185_000]] * 2)


def test_dump_samples_fixed_rows_and_sums_all(tmp_path):
    g = torch.Generator().manual_seed(3)
    last = _last((40_000, 9_000, 2_000), 120_000, lambda *s: torch.randn(s, generator=g))
    bench.dump_outputs(str(tmp_path / "a"), last)
    bench.dump_outputs(str(tmp_path / "b"), last)
    for f in (tmp_path / "a").iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / "b" / f.name)), f.name
    xyz = last["outputs"][0]["levels"][0]["xyz"].numpy()
    got = np.load(tmp_path / "a" / "source_level1_xyz.npy")
    rows = [int(np.flatnonzero((xyz == r).all(1))[0]) for r in got[:50]]
    assert rows == sorted(rows) and len(set(rows)) == 50                     # distinct rows, in level order
    assert np.allclose(np.load(tmp_path / "a" / "source_level1_xyz_colsum.npy"), xyz.astype(np.float64).sum(0))
    small = last["outputs"][1]["levels"][2]["opacity"].numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "target_level3_opacity.npy"), small)             # a level under DUMP_ROWS rows: every row
    ent = np.load(tmp_path / "a" / "icp_entry_iterations_fitness_rmse.npy")
    assert ent.shape == (4, 3) and list(ent[:, 0]) == [50, 49, 48, 47]
    assert np.array_equal(np.load(tmp_path / "a" / "icp_transformation.npy"), last["T"])
    assert np.load(tmp_path / "a" / "icp_entry_transformations.npy").shape == (4, 4, 4)
