"""bench.py --dump-outputs: the file written from the assignment quads
(dtype, shape, the size cap and its seeded row sample).  Pure numpy, no GPU."""
import os

import numpy as np

import bench


def _quads(n_rows):
    return np.arange(n_rows * 4, dtype=np.int32) - 7  # flat, as last_assignments() returns them


def test_dump_below_cap_is_every_row(tmp_path):
    q = _quads(1000)
    d = str(tmp_path / "sub" / "dir")  # created on demand
    bench.dump_outputs(d, q)
    got = np.load(os.path.join(d, "assignments.npy"))
    assert got.dtype == np.float64 and got.shape == (1000, 4)
    assert (got == q.reshape(-1, 4)).all()
    assert os.listdir(d) == ["assignments.npy"]


def test_dump_above_cap_is_a_fixed_sample_in_row_order(tmp_path):
    q = _quads(1000)
    rows = q.reshape(-1, 4)
    cap_rows = 37
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), q, cap_bytes=128 + cap_rows * 32 + 31)  # header + rows; a partial row does not count
    a = np.load(str(tmp_path / "a" / "assignments.npy"))
    b = np.load(str(tmp_path / "b" / "assignments.npy"))
    assert a.dtype == np.float64 and a.shape == (cap_rows, 4) 
    assert os.path.getsize(str(tmp_path / "a" / "assignments.npy")) <= 128 + cap_rows * 32 + 31
    assert (a == b).all()  # the sample does not change from run to run
    # distinct rows of the input, in their original order (row r starts with 4 r - 7)
    idx = ((a[:, 0] + 7) // 4).astype(int)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 1000
    assert (a == rows[idx]).all()


def test_dump_at_the_cap_is_not_sampled(tmp_path):
    q = _quads(64)
    bench.dump_outputs(str(tmp_path), q, cap_bytes=128 + 64 * 32)
    assert (np.load(str(tmp_path / "assignments.npy")) == q.reshape(-1, 4)).all()


def test_default_cap_is_64_mb():
    assert bench.DUMP_CAP_BYTES == 64 * 10**6
