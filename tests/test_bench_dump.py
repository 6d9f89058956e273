"""bench.py --dump-outputs without a GPU: the files dump_outputs() writes from a batch's records and packed traceback strings -- every
trace while they fit in 64 MB, else the same seeded sample of traces whatever the results are."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

NAMES = ["score_fwd", "score_rev", "score_prelim", "slice_begin", "slice_len", "ref_pos", "score_final", "ops_len", "forward"]


def batch(n, seed):
    rng = np.random.default_rng(seed)
    rec = rng.integers(-30000, 30000, size=(n, len(NAMES))).astype(np.int32)
    rec[:, NAMES.index("ops_len")] = rng.integers(0, 1200, size=n)
    ops = rng.integers(0, 256, size=int(rec[:, NAMES.index("ops_len")].sum())).astype(np.uint8)
    return rec, ops


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def strings(rec, ops, idx):
    lens = rec[:, NAMES.index("ops_len")].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    return np.concatenate([ops[off[i]:off[i + 1]] for i in idx])


def test_every_trace_while_it_fits(tmp_path):
    rec, ops = batch(3000, 1)
    bench.dump_outputs(str(tmp_path), NAMES, rec, ops, 2200)
    got = load(str(tmp_path))
    assert set(got) == set(NAMES) | {"ops", "trace_index"}
    assert np.array_equal(got["trace_index"], np.arange(3000))
    for j, k in enumerate(NAMES):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], rec[:, j])
    assert got["ops"].dtype == np.float32 and np.array_equal(got["ops"], ops)


def test_a_large_batch_is_a_fixed_sample_under_the_limit(tmp_path):
    n, cap = 40000, 2200
    rec, ops = batch(n, 2)
    rec2, ops2 = batch(n, 3)  # other results, same batch size: the same traces are sampled
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, NAMES, rec, ops, cap)
    bench.dump_outputs(b, NAMES, rec2, ops2, cap)
    ga, gb = load(a), load(b)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= bench.DUMP_LIMIT
    idx = ga["trace_index"].astype(np.int64)
    assert 0 < len(idx) < n and np.array_equal(idx, gb["trace_index"]) and np.all(np.diff(idx) > 0)
    for j, k in enumerate(NAMES):
        assert np.array_equal(ga[k], rec[idx, j])
    assert np.array_equal(ga["ops"], strings(rec, ops, idx))


def test_strings_that_disagree_with_the_records_are_refused(tmp_path):
    rec, ops = batch(10, 4)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path), NAMES, rec, ops[:-1], 2200)
