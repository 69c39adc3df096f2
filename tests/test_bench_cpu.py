"""bench.py's output dump without a GPU: whole arrays under the budget, the same seeded sample of rows above it."""
import numpy as np

import bench


def test_dump_writes_whole_arrays_under_the_budget(tmp_path):
    cb = np.arange(64 * 8, dtype=np.float32).reshape(64, 8)
    ids = np.arange(100, dtype=np.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"codebook": cb, "bmu": ids})
    assert np.array_equal(np.load(tmp_path / "d" / "codebook.npy"), cb)
    got = np.load(tmp_path / "d" / "bmu.npy")
    assert got.dtype == np.float64 and np.array_equal(got, ids)


def test_dump_samples_the_same_rows_in_order_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    cb = np.arange(1000 * 4, dtype=np.float32).reshape(1000, 4)
    ids = np.arange(3000, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"codebook": cb, "bmu": ids})
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("codebook", "bmu")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("codebook", "bmu")}
    assert sum(v.nbytes for v in a.values()) <= 4096
    for n in a:
        assert np.array_equal(a[n], b[n])                     # a fixed seed: the same entries every run
        assert 0 < len(a[n]) < {"codebook": 1000, "bmu": 3000}[n]
    rows = a["codebook"][:, 0] / 4                            # rows of the original, in their order, none twice
    assert np.array_equal(rows, np.sort(rows)) and len(np.unique(rows)) == len(rows)
    assert np.array_equal(a["codebook"], cb[rows.astype(int)])
