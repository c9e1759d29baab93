"""The multi-GPU index (pyr_index_desc.device_mask / shards; csrc/multi.cpp) against the CPU oracle.

tests/test_gpu_multi.py compares the multi index with the single-GPU index at d = 64 and d = 128.  Here every
case checks three things: (i) ids, score bits and counts equal the single-GPU index's for every query, (ii) the
same equal the oracle's (oracle.ivf_search over ivf_layout() + centroids_array()) on every 5th query, and (iii)
shard_info()'s sharded_searches / staged_searches moved by exactly what the case expects -- a case answered
silently by the first-device index fails.  All shards sit on device 0 (the copy transport).  The cases:

 * the dimensions through the list-sharded step (shard_prepare / shard_search / shard_rerun): padded dims
   (20, 100, 200), the chunked-A tile dims (512, 768), the wide tile dims (800, 1024, 1530, 1536, 2048), L2 and
   IP, a default search and a MaxScans search whose budget ends inside a probe list;
 * every certificate forced to fail with 4-failure re-run rounds at d = 100 / 768 / 2048;
 * the certificate must NOT always fail: a sharded step whose certificate always failed would pass every parity
   check while being the exact re-run, so the unforced searches bound last_max_failures by half the home batch.
   That cap is a condition, not a measurement.  The data has the room (scripts/cert_room.py, on the CPU with the
   oracle's lists and probe ranking, n = 4100, nlist 32, nprobe 8, the 50 queries; the gap between the 10th and
   the 64th exact score over the probed lists beside twice the refine certificate's bound, smallest gap /
   largest 2 x bound over the queries; no query of any case is without room):

       L2  d =   20: 0.331 / 0.0099     d =  100: 1.04 / 0.043     d =  200: 1.29 / 0.089
           d =  512: 2.26  / 0.25       d =  768: 2.54 / 0.40      d =  800: 2.90 / 0.46
           d = 1024: 2.78  / 0.60       d = 1530: 4.02 / 1.05      d = 1536: 3.98 / 1.04
           d = 2048: 3.75  / 1.59
       IP  d =  100: 0.782 / 0.053      d =  768: 2.34 / 0.59      d = 2048: 3.45 / 2.48

   Observed last_max_failures of a home of 17 (default search / MaxScans search), beside the single-GPU index's
   exact re-runs of the 50 queries: L2 0 / 0 at d = 20 .. 512, 800 and 1024, 1 / 0 at 768 and 1530, 2 / 0 at 1536,
   1 / 1 at 2048 (single: the same counts, 2 under MaxScans at 2048); IP 1 / 1 at d = 100 and 768 and 0 / 1 at
   d = 2048 (single 0 / 0 at all three).  Two defects this sweep found are fixed and pinned by these caps:
   shard records carried the depth-16 bound only, while the single-GPU index goes on to depth 64 (IP d = 2048:
   12 / 10 of 17 failed the merge certificate where the single index failed 31 / 29 of 50 at depth 16 and none
   at depth 64); and the MaxScans sample pass of the non-native tile dims (scan.hip sample_kernel) ignored the
   pairs' budgets, so T_q came from rows past the budget (MaxScans searches failed 9 / 13 / 10 / 17 / 17 / 17 /
   17 of 17 at d = 512 / 768 / 800 / 1024 / 1530 / 1536 / 2048, on the single-GPU index 22 / 38 / 28 / 46 / 47 /
   45 / 47 of 50);
 * the lifecycle: a snapshot taken after post-Build writes loads with the lists dealt (the buffer only sends the
   searches to the stage until it is empty again), and the same history without the snapshot;
 * stale samples: the shards' replicated samples are the first <= 512 rows of every list at deal time and a
   Delete does not refresh them, so after deleting exactly those rows T_q comes from rows that no longer exist;
   whatever the certificate then decides, the answers stay exact (observed: 1 of a home of 20 fails on the
   default search, 0 under MaxScans -- on uniform rows the stale sample still estimates T_q well; 0 / 0 after
   the rebuild);
 * edge shapes: shards that own no list, k = 1 / 60 / 61, one query on four shards, exact score ties across
   lists, non-finite rows; device buffers on a caller's stream at a wide dim, twice without a host sync.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 10


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


def _pair(data, metric, nl, shards, mask=1, labels=None, cents=None, **env):
    from pyrope_amd import IvfFlatVectorIndex
    labels = np.arange(len(data), dtype=np.int64) if labels is None else labels
    one = IvfFlatVectorIndex(data.shape[1], metric, n_list=nl)
    with _env(**env):  # (PYR_SHARD_FCAP is read when the index is created)
        multi = IvfFlatVectorIndex(data.shape[1], metric, n_list=nl, device_mask=mask, shards=shards)
    for ix in (one, multi):
        if cents is not None:
            ix.set_centroids(cents)
        ix.add_labels(labels, data, track_ids=False)
        ix.build()
    assert multi.shard_info()["shards"] == shards
    return one, multi


def _same(a, b):
    (s1, l1, c1), (s2, l2, c2) = a, b
    np.testing.assert_array_equal(l2, l1)
    assert np.array_equal(s2.view(np.uint32), s1.view(np.uint32))
    np.testing.assert_array_equal(c2, c1)


def _check_ivf(oracle, idx, x, q, got, k, metric, nprobe, every=5, **kw):
    """got against oracle.ivf_search over the index's own layout; x[label] is the row a list entry holds"""
    s, l, c = got
    off, labels, live = idx.ivf_layout()
    rows = x[np.where(labels >= 0, labels, 0)]
    cents = idx.centroids_array()
    for i in range(0, len(q), every):
        os_, ok = oracle.ivf_search(q[i], k, cents, rows, off, live, metric=metric, nprobe=nprobe, **kw)
        assert int(c[i]) == len(os_), (i, c[i], len(os_))
        np.testing.assert_array_equal(l[i][: len(ok)], labels[ok])
        assert np.array_equal(s[i][: len(os_)].view(np.uint32), os_.astype(np.float32).view(np.uint32))


def _counters(multi):
    info = multi.shard_info()
    return info["sharded_searches"], info["staged_searches"]


def _profiled(lib, run):
    """run() with the profiler on: its result and the exact re-run's work (phase 8: the queries no certificate
    covered), as tests/test_gpu_dims_wide.py reads it"""
    lib.pyr_profile_reset()
    lib.pyr_profile_enable(1)
    try:
        out = run()
    finally:
        lib.pyr_profile_enable(0)
    ms, calls, work = C.c_double(), C.c_int64(), C.c_int64()
    lib.pyr_profile_get(8, C.byref(ms), C.byref(calls), C.byref(work))
    return out, work.value


def _remove(ix, labels):
    from pyrope_amd._lib import check
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    check(ix._L.pyr_index_remove(ix._h, labels.ctypes.data_as(C.POINTER(C.c_int64)), len(labels), None))


def _home(nq, shards):
    return (nq + shards - 1) // shards


# ---- a / c: the dimension sweep through the sharded step, and the certificate's failures ----
N, NLIST, SHARDS, NQ = 4100, 32, 3, 50  # 50 queries on 3 shards: homes of 17, the last one padded
XCD_DIMS = (1024, 1536)  # also searched with PYR_SCAN_XCD=0 (items in list order, one queue): the same bits
SWEEP = [(d, 0) for d in (20, 100, 200, 512, 768, 800, 1024, 1530, 1536, 2048)] + [(100, 1), (768, 1), (2048, 1)]
_SWEEP_FAILS = {}  # (dim, metric) -> last_max_failures of the default and of the MaxScans search, then the
# single-GPU index's exact re-runs of the same two searches


def _sweep_case(hiplib, oracle, dim, metric):
    """One default search and one MaxScans search at this dim, each against the single-GPU index, the oracle and
    the counters; returns the two searches' last_max_failures and the single-GPU index's exact re-runs (run once
    per case, shared by the tests below)"""
    if (dim, metric) in _SWEEP_FAILS:
        return _SWEEP_FAILS[(dim, metric)]
    from pyrope_amd import SearchOptions, generate_synthetic
    x = generate_synthetic(N, dim, 42)
    one, multi = _pair(x, metric, NLIST, SHARDS)
    q = generate_synthetic(NQ, dim, 1337)
    sharded0, staged0 = _counters(multi)
    home = _home(NQ, SHARDS)
    xcd_off = dim in XCD_DIMS
    fails, single = [], []
    # nprobe 16 for the MaxScans run: 16 lists of ~128 rows hold ~2,050 rows, so 1,500 ends inside a probe list
    for nprobe, ms in ((8, None), (16, 1500)):
        opts = SearchOptions(nprobe=nprobe, max_scans=ms)
        ref, reruns = _profiled(hiplib, lambda: one.search_batch(q, K, opts))
        got = multi.search_batch(q, K, opts)
        info = multi.shard_info()
        fails.append(info["last_max_failures"])
        single.append(reruns)
        print(f"\n[multi] d={dim} metric={metric} nprobe={nprobe} max_scans={ms}: last_max_failures {fails[-1]} of a "
              f"home of {home} (extra rounds {info['last_extra_rounds']}); unsharded exact re-runs {reruns} of {NQ}")
        _same(ref, got)
        _check_ivf(oracle, multi, x, q, got, K, metric, nprobe, max_scans=-1 if ms is None else ms)
        sharded0 += 1
        assert _counters(multi) == (sharded0, staged0), "the list-sharded step must answer"
        if xcd_off:
            with _env(PYR_SCAN_XCD=0):
                _same(got, multi.search_batch(q, K, opts))
            sharded0 += 1
            assert _counters(multi) == (sharded0, staged0)
    one.close()
    multi.close()
    _SWEEP_FAILS[(dim, metric)] = tuple(fails + single)
    return _SWEEP_FAILS[(dim, metric)]


@pytest.mark.parametrize("dim,metric", SWEEP)
def test_multi_dims_through_the_sharded_step(hiplib, oracle, dim, metric):
    """ids, score bits, counts and counters of both searches (the failure counts: the two tests below)"""
    _sweep_case(hiplib, oracle, dim, metric)


@pytest.mark.parametrize("dim,metric", SWEEP)
def test_multi_default_search_certificates_within_the_cap(hiplib, oracle, dim, metric):
    fails = _sweep_case(hiplib, oracle, dim, metric)[0]
    home = _home(NQ, SHARDS)
    assert fails <= home // 2, f"{fails} of a home of {home} failed the merge certificate"


@pytest.mark.parametrize("dim,metric", SWEEP)
def test_multi_max_scans_certificates_within_the_cap(hiplib, oracle, dim, metric):
    fails = _sweep_case(hiplib, oracle, dim, metric)[1]
    home = _home(NQ, SHARDS)
    assert fails <= home // 2, f"{fails} of a home of {home} failed the merge certificate under MaxScans"


@pytest.mark.parametrize("dim,metric", SWEEP)
def test_single_index_certificates_within_the_cap(hiplib, oracle, dim, metric):
    """the single-GPU index on the same two searches: its exact re-runs (profile phase 8) within half the batch.
    The MaxScans search is the one that was not: the sample pass of the non-native tile dims ignored the budget"""
    for reruns, what in zip(_sweep_case(hiplib, oracle, dim, metric)[2:], ("default", "MaxScans")):
        assert reruns <= NQ // 2, f"{reruns} of {NQ} queries of the {what} search took the exact re-run"


# ---- b: forced certificate failures, several re-run rounds, at non-native dims ----
@pytest.mark.parametrize("dim", [100, 768, 2048])
def test_multi_every_certificate_fails_at_other_dims(hiplib, oracle, dim):
    """PYR_FILTER_CERR=1e15 with 4-failure rounds: a home of 17 takes 4 further rounds of shard_rerun + merge"""
    from pyrope_amd import SearchOptions, generate_synthetic
    x = generate_synthetic(N, dim, 42)
    one, multi = _pair(x, 0, NLIST, SHARDS, PYR_SHARD_FCAP=4)
    q = generate_synthetic(NQ, dim, 1337)
    home = _home(NQ, SHARDS)
    sharded0, staged0 = _counters(multi)
    for n_run, (nprobe, ms) in enumerate(((8, None), (16, 1500))):
        opts = SearchOptions(nprobe=nprobe, max_scans=ms)
        ref = one.search_batch(q, K, opts)
        with _env(PYR_FILTER_CERR="1e15"):
            got = multi.search_batch(q, K, opts)
        _same(ref, got)
        _check_ivf(oracle, multi, x, q, got, K, 0, nprobe, max_scans=-1 if ms is None else ms)
        info = multi.shard_info()
        assert info["last_max_failures"] == home
        assert info["last_extra_rounds"] == (home - 1) // 4
        assert _counters(multi) == (sharded0 + n_run + 1, staged0)
    one.close()
    multi.close()


# ---- d: post-Build writes, snapshot / load, and the buffer emptied again ----
@pytest.mark.parametrize("via_snapshot", [True, False])
def test_multi_buffer_writes_then_sharded_again(hiplib, oracle, tmp_path, via_snapshot):
    """Build, Upsert of 100 built ids and Add of 100 new ids (a non-empty buffer: the stage answers), then --
    through Snapshot and Load into a fresh 3-shard index, or directly -- Delete of those 200 ids: the buffer is
    empty again and the next search must be list-sharded.  (A loaded image's buffer rows used to keep the lists
    from being dealt at all: every later search ran on one GPU until the next Build.)"""
    from pyrope_amd import IvfFlatVectorIndex, SearchOptions, generate_synthetic
    n, d, nl = 20_000, 64, 32
    data = generate_synthetic(n, d, 23)
    one, multi = _pair(data, 0, nl, 2)
    q = generate_synthetic(60, d, 24)
    opts = (SearchOptions(nprobe=6), SearchOptions(nprobe=6, max_scans=2500))
    _same(one.search_batch(q, K, opts[0]), multi.search_batch(q, K, opts[0]))
    assert _counters(multi) == (1, 0)
    new = generate_synthetic(200, d, 25)
    labs = np.concatenate([np.arange(5, 2005, 20), np.arange(n, n + 100)]).astype(np.int64)  # 100 built, 100 new
    for ix in (one, multi):
        ix.add_labels(labs, new, track_ids=False)
    if via_snapshot:
        p = str(tmp_path / "m.idx")
        multi.snapshot(p)
        back = IvfFlatVectorIndex(d, 0, n_list=nl, device_mask=1, shards=3)
        back.load(p)
        multi.close()
        multi = back
        assert multi.shard_info()["shards"] == 3
    sharded0, staged0 = _counters(multi)
    for o in opts:  # the buffer holds 200 rows: the first-device index answers
        _same(one.search_batch(q, K, o), multi.search_batch(q, K, o))
    assert _counters(multi) == (sharded0, staged0 + 2)
    for ix in (one, multi):
        _remove(ix, labs)
    for n_run, o in enumerate(opts):
        got = multi.search_batch(q, K, o)
        assert _counters(multi) == (sharded0 + n_run + 1, staged0 + 2), "an empty buffer: the list-sharded step"
        _same(one.search_batch(q, K, o), got)
        _check_ivf(oracle, multi, data, q, got, K, 0, 6, max_scans=-1 if o.max_scans is None else o.max_scans)
    off, labels, live = multi.ivf_layout()
    assert int(live.sum()) == n - 100  # the upserted ids left the lists with their buffer rows
    one.close()
    multi.close()


# ---- e: stale samples ----
def test_multi_stale_samples_stay_exact(hiplib, oracle):
    """The first 512 live rows of every list (the rows the shards' samples were taken from) deleted in one call:
    the searches stay list-sharded and exact whatever the stale T_q does to the certificate (the failure count
    is printed, not bounded: 1 / 0 of a home of 20 observed), and after a rebuild it is within the cap"""
    from pyrope_amd import SearchOptions, generate_synthetic
    n, d, nl, shards, nq = 24_000, 64, 16, 3, 60
    data = generate_synthetic(n, d, 26)
    one, multi = _pair(data, 0, nl, shards)
    off, labels, live = multi.ivf_layout()
    assert bool(np.all(live)) and int(np.diff(off).min()) > 512
    gone = np.concatenate([labels[off[l]: off[l] + 512] for l in range(nl)])
    for ix in (one, multi):
        _remove(ix, gone)
    q = generate_synthetic(nq, d, 27)
    home = _home(nq, shards)
    runs = ((4, None), (4, 2000))
    for n_run, (nprobe, ms) in enumerate(runs):
        opts = SearchOptions(nprobe=nprobe, max_scans=ms)
        got = multi.search_batch(q, K, opts)
        info = multi.shard_info()
        print(f"\n[multi] stale samples, max_scans={ms}: last_max_failures {info['last_max_failures']} of a home "
              f"of {home}, extra rounds {info['last_extra_rounds']}")
        assert _counters(multi) == (n_run + 1, 0)
        _same(one.search_batch(q, K, opts), got)
        _check_ivf(oracle, multi, data, q, got, K, 0, nprobe, max_scans=-1 if ms is None else ms)
    for ix in (one, multi):
        ix.build()
    for n_run, (nprobe, ms) in enumerate(runs):
        opts = SearchOptions(nprobe=nprobe, max_scans=ms)
        got = multi.search_batch(q, K, opts)
        fails = multi.shard_info()["last_max_failures"]
        print(f"\n[multi] rebuilt, max_scans={ms}: last_max_failures {fails} of a home of {home}")
        assert _counters(multi) == (len(runs) + n_run + 1, 0)
        _same(one.search_batch(q, K, opts), got)
        _check_ivf(oracle, multi, data, q, got, K, 0, nprobe, max_scans=-1 if ms is None else ms)
        assert fails <= home // 2, f"{fails} of a home of {home} failed after the rebuild"
    one.close()
    multi.close()


# ---- f: edge shapes ----
@pytest.mark.parametrize("metric", [0, 1])
def test_multi_shards_without_lists(hiplib, oracle, metric):
    """3 lists on 4 shards: at least one shard owns no list; nprobe 1, 2 and 3 (= nlist)"""
    from pyrope_amd import SearchOptions, generate_synthetic
    n, d = 600, 32
    x = generate_synthetic(n, d, 28)
    one, multi = _pair(x, metric, 3, 4)
    q = generate_synthetic(10, d, 29)
    for n_run, nprobe in enumerate((1, 2, 3)):
        opts = SearchOptions(nprobe=nprobe)
        got = multi.search_batch(q, K, opts)
        _same(one.search_batch(q, K, opts), got)
        _check_ivf(oracle, multi, x, q, got, K, metric, nprobe, every=1)
        assert _counters(multi) == (n_run + 1, 0)
    one.close()
    multi.close()


def test_multi_k_1_60_61(hiplib, oracle):
    """k = 1 and k = 60 (the deepest the stream scan's refine certifies with its margin of 4) are list-sharded;
    k = 61 is the first-device index's"""
    from pyrope_amd import SearchOptions, generate_synthetic
    n, d, nl = 6000, 64, 16
    x = generate_synthetic(n, d, 30)
    one, multi = _pair(x, 0, nl, 3)
    q = generate_synthetic(30, d, 31)
    opts = SearchOptions(nprobe=4)
    expect = (0, 0)
    for k, sharded in ((1, True), (60, True), (61, False)):
        got = multi.search_batch(q, k, opts)
        expect = (expect[0] + 1, expect[1]) if sharded else (expect[0], expect[1] + 1)
        assert _counters(multi) == expect, f"k = {k}"
        _same(one.search_batch(q, k, opts), got)
        _check_ivf(oracle, multi, x, q, got, k, 0, 4)
    one.close()
    multi.close()


def test_multi_one_query_on_four_shards(hiplib, oracle):
    from pyrope_amd import SearchOptions, generate_synthetic
    n, d, nl = 6000, 64, 16
    x = generate_synthetic(n, d, 32)
    one, multi = _pair(x, 0, nl, 4)
    q = generate_synthetic(1, d, 33)
    for n_run, (nprobe, ms) in enumerate(((4, None), (4, 700))):
        opts = SearchOptions(nprobe=nprobe, max_scans=ms)
        got = multi.search_batch(q, K, opts)
        _same(one.search_batch(q, K, opts), got)
        _check_ivf(oracle, multi, x, q, got, K, 0, nprobe, every=1, max_scans=-1 if ms is None else ms)
        assert _counters(multi) == (n_run + 1, 0)
    one.close()
    multi.close()


def test_multi_exact_ties_across_lists(hiplib, oracle):
    """Rows at exactly equal distance from a query in different lists (often on different shards): on a grid of
    multiples of 2^-6 the reflection 2q - x of a row x about q is exact, so |q - x|^2 ties bit for bit.  The
    merged order is (score, list, position) and must be the single-GPU index's storage-slot order."""
    from pyrope_amd import SearchOptions, generate_synthetic
    n, d, nl, k, nq = 20_000, 64, 32, 20, 64
    data = np.round(generate_synthetic(n, d, 7) * 64) / 64
    qh = (np.round(generate_synthetic(2 * nq, d, 9) * 64) / 64).astype(np.float32)
    refl = []
    for qv in qh[:nq]:  # the 6 nearest rows of half of the queries, reflected about the query
        near = np.argsort(((data - qv) ** 2).sum(1))[:6]
        refl.append(2 * qv - data[near])
    data = np.concatenate([data] + refl).astype(np.float32)
    one, multi = _pair(data, 0, nl, 3)
    opts = SearchOptions(nprobe=nl)
    ref = one.search_batch(qh, k, opts)
    assert sum(len(set(r.tolist())) < k for r in ref[0][:nq]) > nq // 2  # exact ties inside the top k
    got = multi.search_batch(qh, k, opts)
    assert _counters(multi) == (1, 0)
    _same(ref, got)
    _check_ivf(oracle, multi, data, qh, got, k, 0, nl)
    one.close()
    multi.close()


@pytest.mark.parametrize("metric", [0, 1])
def test_multi_non_finite_rows(hiplib, metric):
    """One all-NaN row and one row holding +Inf (quantizer trained on the finite rows): the list-sharded answer
    equals the single-GPU index's exact path (PYR_FILTER=0); the NaN row never appears, and for IP the +Inf row
    ranks as the single-GPU index ranks it"""
    from pyrope_amd import SearchOptions, generate_synthetic, kmeans_train
    n, d, nl = 6000, 64, 16
    x = generate_synthetic(n, d, 34)
    cents = kmeans_train(x, nl, metric, 8, 42)
    x[3] = np.nan
    x[7, 3] = np.inf
    one, multi = _pair(x, metric, nl, 3, cents=cents)
    q = generate_synthetic(40, d, 35)
    for n_run, nprobe in enumerate((4, nl)):
        opts = SearchOptions(nprobe=nprobe)
        with _env(PYR_FILTER=0):
            ref = one.search_batch(q, K, opts)
        got = multi.search_batch(q, K, opts)
        assert _counters(multi) == (n_run + 1, 0)
        _same(ref, got)
        assert 3 not in got[1]
        np.testing.assert_array_equal(got[1] == 7, ref[1] == 7)
        if metric == 1 and nprobe == nl:  # every list probed: score +Inf, first for every query
            assert (got[1][:, 0] == 7).all() and np.isposinf(got[0][:, 0]).all()
    one.close()
    multi.close()


# ---- g: device buffers on the caller's stream at a wide dim ----
def test_multi_device_search_wide_dim_back_to_back(hiplib, oracle):
    """d = 1024, search_device on a non-default torch stream, twice with no host sync between the calls: the
    second step reuses the first one's shard buffers and streams while its copies may still be in flight"""
    import torch

    from pyrope_amd import SearchOptions, generate_synthetic
    d, nq = 1024, NQ
    x = generate_synthetic(N, d, 42)
    one, multi = _pair(x, 0, NLIST, SHARDS)
    qh = generate_synthetic(nq, d, 36)
    q = torch.from_numpy(qh).cuda()
    out = [(torch.empty((nq, K), dtype=torch.float32, device="cuda"),
            torch.empty((nq, K), dtype=torch.int64, device="cuda"),
            torch.empty((nq,), dtype=torch.int32, device="cuda")) for _ in range(2)]
    opts = SearchOptions(nprobe=8)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for s, lab, cnt in out:
            multi.search_device(q.data_ptr(), nq, K, s.data_ptr(), lab.data_ptr(), cnt.data_ptr(), st.cuda_stream, opts)
    st.synchronize()
    assert _counters(multi) == (2, 0)
    first, second = [tuple(t.cpu().numpy() for t in o) for o in out]
    _same(first, second)
    _same(one.search_batch(qh, K, opts), first)
    _check_ivf(oracle, multi, x, qh, first, K, 0, 8)
    one.close()
    multi.close()
