"""The HIP path against the committed answer keys (tests/golden/*.npz, written by tests/golden/make_golden.py).

No oracle call: the fixtures hold what the CPU restatement of the reference computed for the benchmark
generator's rows (seed 42) and queries (seed 1337), so these tests stand when the oracle cannot be rebuilt and
would notice the oracle and the kernels drifting together.  Every comparison is of ids and float bits.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assign_of_layout(off, labels, n):
    """the row -> list assignment that a list layout states; rows of a list must sit in ascending row order"""
    asg = np.full(n, -1, np.int64)
    for l in range(len(off) - 1):
        seg = labels[off[l]: off[l + 1]]
        assert np.all(np.diff(seg) > 0), f"list {l} is not in row order"
        asg[seg] = l
    return asg


def test_golden_generator(hiplib):
    from pyrope_amd import generate_synthetic
    g = np.load(os.path.join(GOLDEN, "generator.npz"))
    for seed in (42, 1337):
        got = generate_synthetic(2, 8, seed).reshape(-1)
        assert np.array_equal(_bits(got), _bits(g[f"gen_seed{seed}_first16"]))


@pytest.mark.parametrize("metric,name", [(0, "l2"), (1, "ip"), (2, "cos")])
def test_golden_flat(hiplib, metric, name):
    from pyrope_amd import BruteForceVectorIndex, generate_synthetic
    g = np.load(os.path.join(GOLDEN, "flat_d128.npz"))
    n, d, nq, k = int(g["n"]), int(g["dim"]), int(g["nq"]), int(g["k"])
    x = generate_synthetic(n, d, int(g["base_seed"]))
    q = generate_synthetic(nq, d, int(g["query_seed"]))
    idx = BruteForceVectorIndex(d, metric)
    idx.add_labels(np.arange(n, dtype=np.int64), x)
    s, l, c = idx.search_batch(q, k)
    np.testing.assert_array_equal(c, np.full(nq, k))
    np.testing.assert_array_equal(l, g[f"{name}_keys"])
    assert np.array_equal(_bits(s), _bits(g[f"{name}_scores"]))
    idx.close()


def test_golden_ivf_flat(hiplib):
    """Build (centroid bits, the assignment) and Search on the single-GPU index and on a 3-shard multi index"""
    from pyrope_amd import IvfFlatVectorIndex, SearchOptions, generate_synthetic
    g = np.load(os.path.join(GOLDEN, "ivf_flat.npz"))
    n, d, nl, P, k = int(g["n"]), int(g["dim"]), int(g["nlist"]), int(g["nprobe"]), int(g["k"])
    x = generate_synthetic(n, d, 42)
    q = generate_synthetic(len(g["scores"]), d, 1337)
    for kw in ({}, {"device_mask": 1, "shards": 3}):
        idx = IvfFlatVectorIndex(d, 0, n_list=nl, **kw)
        idx.add_labels(np.arange(n, dtype=np.int64), x)
        idx.build()
        cents = idx.centroids_array()
        assert cents.shape == g["centroids"].shape
        assert np.array_equal(_bits(cents), _bits(g["centroids"]))
        off, labels, live = idx.ivf_layout()
        assert off[-1] == n and bool(np.all(live))
        np.testing.assert_array_equal(_assign_of_layout(off, labels, n), g["assign"])
        s, l, c = idx.search_batch(q, k, SearchOptions(nprobe=P))
        np.testing.assert_array_equal(c, np.full(len(q), k))
        np.testing.assert_array_equal(l, g["labels"])
        assert np.array_equal(_bits(s), _bits(g["scores"]))
        if kw:
            info = idx.shard_info()
            assert info["shards"] == 3 and info["sharded_searches"] == 1 and info["staged_searches"] == 0
        idx.close()


def test_golden_ivf_pq(hiplib):
    from pyrope_amd import IvfPqVectorIndex, SearchOptions, generate_synthetic
    g = np.load(os.path.join(GOLDEN, "ivf_pq.npz"))
    n, d, nl, m, ksub = int(g["n"]), int(g["dim"]), int(g["nlist"]), int(g["m"]), int(g["ksub"])
    P, k = int(g["nprobe"]), int(g["k"])
    x = generate_synthetic(n, d, 42)
    q = generate_synthetic(len(g["scores"]), d, 1337)
    idx = IvfPqVectorIndex(d, 0, m=m, k=ksub, n_list=nl)
    idx.add_labels(np.arange(n, dtype=np.int64), x)
    idx.build()
    assert np.array_equal(_bits(idx.centroids_array()), _bits(g["centroids"]))
    cb, codes, off, labels, live = idx.pq_state()
    assert cb.shape == g["codebooks"].shape
    assert np.array_equal(_bits(cb), _bits(g["codebooks"]))
    assert off[-1] == n and bool(np.all(live))
    np.testing.assert_array_equal(_assign_of_layout(off, labels, n), g["assign"])
    np.testing.assert_array_equal(codes, g["codes"][labels])
    s, l, c = idx.search_batch(q, k, SearchOptions(nprobe=P))
    np.testing.assert_array_equal(c, np.full(len(q), k))
    np.testing.assert_array_equal(l, g["labels"])
    assert np.array_equal(_bits(s), _bits(g["scores"]))
    idx.close()
