"""Dimensions 769 .. 2048 on the stream scan (tile dimensions 1024 / 1536 / 2048, scan.hip).

Dims 769..1024 pad to 1024, 1025..1536 to 1536, 1537..2048 to 2048: 64 queries per item at 1024, one 32-query
group above, the tile's A operands in chunks of 16 k-steps (4 / 6 / 8 chunks).  Each case checks that the stream
path ran (the profiler's sample phase, 9) and that the ids and score bits equal the oracle's, in the style of
test_gpu_dims.py; the two dimension sweeps also bound the exact re-run (phase 8's work) by half the batch -- a
scan whose certificate always failed would pass every parity check while being the exact scan.  On this data
the depth-64 certificate has room at every query: the gap between the 10th and the 64th exact score is at least
2.6, twice the bound at most 2.4 (IP, d = 2048) and at most 1.6 elsewhere (uniform rows, n = 1000 and 3001).
Dims past 2048 keep the exact scan and are checked for parity only.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10
NQ = 24


class _env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _profiled(lib, run):
    """run() with the profiler on: its result, the sample phase's calls (the stream scan ran) and the exact
    re-run's work (queries neither certificate covered)"""
    lib.pyr_profile_reset()
    lib.pyr_profile_enable(1)
    try:
        out = run()
    finally:
        lib.pyr_profile_enable(0)
    ms, calls, work = C.c_double(), C.c_int64(), C.c_int64()
    lib.pyr_profile_get(9, C.byref(ms), C.byref(calls), C.byref(work))
    sampled = calls.value
    lib.pyr_profile_get(8, C.byref(ms), C.byref(calls), C.byref(work))
    return out, sampled, work.value


def _same(s, l, os_, ok):
    np.testing.assert_array_equal(l[: len(ok)], ok)
    assert np.array_equal(s[: len(os_)].view(np.uint32), os_.astype(np.float32).view(np.uint32))


def _bits(a, b):
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[1], b[1])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _flat(dim, metric, n, seed=42):
    from pyrope_amd import BruteForceVectorIndex, generate_synthetic
    x = generate_synthetic(n, dim, seed)
    idx = BruteForceVectorIndex(dim, metric)
    idx.add_labels(np.arange(n, dtype=np.int64), x)
    return idx, x


def _ivf(dim, metric, n=4100, nlist=32, seed=42):
    from pyrope_amd import IvfFlatVectorIndex, generate_synthetic
    x = generate_synthetic(n, dim, seed)
    idx = IvfFlatVectorIndex(dim, metric, n_list=nlist)
    idx.add_labels(np.arange(n, dtype=np.int64), x)
    idx.build()
    return idx, x


def _check_ivf(oracle, idx, x, q, got, k, metric, nprobe, every=1, **kw):
    s, l, c = got
    off, labels, live = idx.ivf_layout()
    rows = x[np.where(labels >= 0, labels, 0)]
    cents = idx.centroids_array()
    for i in range(0, len(q), every):
        os_, ok = oracle.ivf_search(q[i], k, cents, rows, off, live, metric=metric, nprobe=nprobe, **kw)
        assert int(c[i]) == len(os_), (i, c[i], len(os_))
        _same(s[i], l[i], os_, labels[ok])


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("dim", [800, 1024, 1030, 1536, 2000, 2048])
def test_flat_wide_dims_match_oracle(hiplib, oracle, dim, metric):
    from pyrope_amd import generate_synthetic
    idx, x = _flat(dim, metric, 3001)  # 3 chunks of 1,248 rows, the last tile partial
    q = generate_synthetic(NQ, dim, 1337)
    (s, l, c), sampled, reruns = _profiled(hiplib, lambda: idx.search_batch(q, K))
    print(f"\n[wide] FLAT d={dim} metric={metric}: sample calls {sampled}, exact re-runs {reruns} of {NQ}")
    assert sampled >= 1, "the FLAT search must take the stream scan"
    for i in range(NQ):
        os_, ok = oracle.bf_search(x, None, metric, q[i], K)
        _same(s[i], l[i], os_, ok)
    assert reruns <= NQ // 2, f"{reruns} of {NQ} queries failed both certificates"
    idx.close()


@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("dim", [1024, 1530, 2048])
def test_ivf_wide_dims_match_oracle(hiplib, oracle, dim, metric):
    from pyrope_amd import SearchOptions, generate_synthetic
    idx, x = _ivf(dim, metric)
    q = generate_synthetic(NQ, dim, 1337)
    opts = SearchOptions(nprobe=8)
    got, sampled, reruns = _profiled(hiplib, lambda: idx.search_batch(q, K, opts))
    print(f"\n[wide] IVF d={dim} metric={metric}: sample calls {sampled}, exact re-runs {reruns} of {NQ}")
    assert sampled >= 1, "the IVF search must take the stream scan"
    _check_ivf(oracle, idx, x, q, got, K, metric, 8)
    assert reruns <= NQ // 2, f"{reruns} of {NQ} queries failed both certificates"
    idx.close()


@pytest.mark.parametrize("dim", [1024, 2048])
def test_flat_wide_many_queries_per_chunk(hiplib, oracle, dim):
    """150 queries: more than one item per chunk and a partial last query group at 32, 64 or 128 queries per item"""
    from pyrope_amd import generate_synthetic
    idx, x = _flat(dim, 0, 3001)
    q = generate_synthetic(150, dim, 7)
    (s, l, c), sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, K))
    assert sampled >= 1
    for i in range(len(q)):
        os_, ok = oracle.bf_search(x, None, 0, q[i], K)
        _same(s[i], l[i], os_, ok)
    idx.close()


def test_flat_wide_deep_k(hiplib, oracle):
    """k = 100 at d = 1024: the deep refine (depth 128) over the wide tiles' candidates"""
    from pyrope_amd import generate_synthetic
    idx, x = _flat(1024, 0, 3001)
    q = generate_synthetic(NQ, 1024, 92)
    (s, l, c), sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, 100))
    assert sampled >= 1, "FLAT k = 100 must take the stream scan"
    for i in range(NQ):
        os_, ok = oracle.bf_search(x, None, 0, q[i], 100)
        _same(s[i], l[i], os_, ok)
    idx.close()


def test_ivf_wide_deep_k(hiplib, oracle):
    from pyrope_amd import SearchOptions, generate_synthetic
    idx, x = _ivf(1024, 0)
    q = generate_synthetic(NQ, 1024, 82)
    opts = SearchOptions(nprobe=8)
    got, sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, 100, opts))
    assert sampled >= 1, "IVF k = 100 must take the stream scan"
    _check_ivf(oracle, idx, x, q, got, 100, 0, 8)
    idx.close()


def test_ivf_wide_max_scans(hiplib, oracle):
    """MaxScans = 1500 at d = 1536 (the LIM kernels); 16 of 32 lists hold ~2,050 rows, so the budget ends inside
    the probe list"""
    from pyrope_amd import SearchOptions, generate_synthetic
    idx, x = _ivf(1536, 0)
    q = generate_synthetic(NQ, 1536, 52)
    opts = SearchOptions(nprobe=16, max_scans=1500)
    got, sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, K, opts))
    assert sampled >= 1, "a MaxScans search must take the stream scan"
    _check_ivf(oracle, idx, x, q, got, K, 0, 16, max_scans=1500)
    idx.close()


def test_ivf_wide_rows_added_after_build(hiplib, oracle):
    """200 rows added after Build at d = 1024 (50 of them shadow list rows): the buffer's exact top k merged with
    the lists' certified answer"""
    from pyrope_amd import SearchOptions, generate_synthetic
    d, n, P = 1024, 4100, 8
    idx, x = _ivf(d, 0)
    extra = generate_synthetic(200, d, 72)
    new_labels = np.concatenate([np.arange(n, n + 150), np.arange(0, 50)])
    idx.add_labels(new_labels, extra)
    off, labels, live = idx.ivf_layout()
    rows = x[np.where(labels >= 0, labels, 0)]
    cents = idx.centroids_array()
    slot_labels = new_labels.tolist()
    bl = np.ones(len(slot_labels), np.uint8)
    q = generate_synthetic(NQ, d, 73)
    opts = SearchOptions(nprobe=P)
    (s, l, c), sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, K, opts))
    assert sampled >= 1, "the lists must take the stream scan"
    for i in range(NQ):
        os_, ok = oracle.ivf_search(q[i], K, cents, rows, off, live, buf=extra, buf_live=bl, metric=0, nprobe=P,
                                    max_scans=-1)
        exp = np.array([slot_labels[k - oracle.BUFKEY] if k >= oracle.BUFKEY else labels[k] for k in ok], np.int64)
        assert int(c[i]) == len(os_), i
        _same(s[i], l[i], os_, exp)
    idx.close()


def test_flat_wide_deleted_rows(hiplib, oracle):
    """300 deleted rows at d = 1536: tombstones inside the tiles"""
    from pyrope_amd import generate_synthetic
    n = 3001
    idx, x = _flat(1536, 0, n)
    live = np.ones(n, np.uint8)
    for lab in range(3, n, 10):
        assert idx.delete(str(lab))
        live[lab] = 0
    assert int((live == 0).sum()) == 300
    q = generate_synthetic(NQ, 1536, 1337)
    (s, l, c), sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, K))
    assert sampled >= 1
    for i in range(NQ):
        os_, ok = oracle.bf_search(x, live, 0, q[i], K)
        _same(s[i], l[i], os_, ok)
    idx.close()


def test_ivf_wide_snapshot_then_load(hiplib, oracle, tmp_path):
    """the image holds no tiles: a loaded wide-dim index builds them and takes the stream path"""
    from pyrope_amd import IvfFlatVectorIndex, SearchOptions, generate_synthetic
    d = 1024
    idx, x = _ivf(d, 0)
    q = generate_synthetic(NQ, d, 8)
    opts = SearchOptions(nprobe=8)
    ref = idx.search_batch(q, K, opts)
    _check_ivf(oracle, idx, x, q, ref, K, 0, 8, every=5)
    path = str(tmp_path / "ivf_wide")
    idx.snapshot(path)
    other = IvfFlatVectorIndex(d, 0, n_list=32)
    other.load(path)
    got, sampled, _ = _profiled(hiplib, lambda: other.search_batch(q, K, opts))
    assert sampled >= 1, "the loaded index must take the stream scan"
    _bits(got, ref)
    idx.close()
    other.close()


@pytest.mark.parametrize("dim", [1024, 1536])
def test_ivf_wide_item_queues_do_not_change_results(hiplib, oracle, dim):
    """PYR_SCAN_XCD=0 (items in list order, one queue) answers as the default's XCD-affine queues; 150 queries
    on 8 of 32 lists: several items per list"""
    from pyrope_amd import SearchOptions, generate_synthetic
    idx, x = _ivf(dim, 0)
    q = generate_synthetic(150, dim, 7)
    opts = SearchOptions(nprobe=8)
    got, sampled, _ = _profiled(hiplib, lambda: idx.search_batch(q, K, opts))
    assert sampled >= 1
    with _env(PYR_SCAN_XCD=0):
        _bits(idx.search_batch(q, K, opts), got)
    _check_ivf(oracle, idx, x, q, got, K, 0, 8, every=7)
    idx.close()


@pytest.mark.parametrize("kind", ["flat", "ivf"])
def test_wide_every_certificate_fails(hiplib, oracle, kind):
    """PYR_FILTER_CERR=1e30 at d = 2048: every query takes the exact re-run and still matches"""
    from pyrope_amd import SearchOptions, generate_synthetic
    d = 2048
    q = generate_synthetic(NQ, d, 1337)
    if kind == "flat":
        idx, x = _flat(d, 0, 3001)
        with _env(PYR_FILTER_CERR="1e30"):
            (s, l, c), sampled, reruns = _profiled(hiplib, lambda: idx.search_batch(q, K))
        for i in range(NQ):
            os_, ok = oracle.bf_search(x, None, 0, q[i], K)
            _same(s[i], l[i], os_, ok)
    else:
        idx, x = _ivf(d, 0)
        opts = SearchOptions(nprobe=8)
        with _env(PYR_FILTER_CERR="1e30"):
            got, sampled, reruns = _profiled(hiplib, lambda: idx.search_batch(q, K, opts))
        _check_ivf(oracle, idx, x, q, got, K, 0, 8)
    assert sampled >= 1
    assert reruns == NQ, f"{reruns} of {NQ} queries re-ran"
    idx.close()


@pytest.mark.parametrize("dim", [2049, 3072])
def test_flat_past_the_widest_tile(hiplib, oracle, dim):
    """dims past 2048 keep the exact scan: oracle-identical, whichever path serves them"""
    from pyrope_amd import generate_synthetic
    idx, x = _flat(dim, 0, 1500)
    q = generate_synthetic(NQ, dim, 1337)
    s, l, c = idx.search_batch(q, K)
    for i in range(NQ):
        os_, ok = oracle.bf_search(x, None, 0, q[i], K)
        _same(s[i], l[i], os_, ok)
    idx.close()
