"""Search batches that the host cuts into several device launches.

Every entry point splits a large batch into chunks (a workspace budget, or the 65 535 grid-dimension limit) and launches
the same kernels again with shifted query, `qq`, output and `ActiveMask::base` pointers over reused workspaces.  Each case
below restates its entry point's chunk formula (citing the source), asserts that the batch crosses at least one chunk
boundary with a partial last chunk, and, where the library counts launches (IvfPqIndex / IvfFlatIndex `scan_launches`
with profile = 1, FlatIndex `gemm_launches` with profile = True), asserts the count.  Then:
  * the same call with profiling off (the production path) returns identical results;
  * every query equals the same query served by calls that each fit in one chunk, some of them straddling the big
    call's chunk boundaries;
  * a seeded sample -- the first and last query of every chunk (so both sides of each boundary) and a few random ones --
    equals the CPU oracle (or the restatements of tests/test_gpu_ivf_flat.py / tests/test_gpu_multivec.py) with ==;
  * host I/O and device I/O (DeviceArray: the GPU tests keep torch out of the test process) both.
"""
import numpy as np
import pytest

import lancedb_amd
from lancedb_amd import _abi
from oracle import train
from tests.test_gpu_ivf_flat import _dataset, _expected, _f64_bar, _probe_oracle
from tests.test_gpu_ivf_flat import _same as _same_ivf_flat
from tests.test_gpu_multivec import assert_same as assert_same_multivec
from tests.test_gpu_multivec import restate

pytestmark = pytest.mark.gpu
DA = lancedb_amd.DeviceArray
CAND = 16                     # sizeof(Cand), csrc/device_common.h
WORKSPACE = 2048 << 20        # MI355_WORKSPACE_MB default (ann_flat.hip:124, ann_index.hip:267)
SECOND_PASS_WS = 512 << 20    # SearchPlan::ws_mb of the maximum_nprobes pass (ann_index_search.hip:193)
LUT_IMAGE_BUDGET = 16384 << 20  # MI355_LUT_IMAGES_MB default (ann_index.hip:280)
GRID_Z = 65535


# ---- the chunk formulas, restated ------------------------------------------------------------------------------------
def flat_sweep_chunk(n_rows, nq, k):
    """ann_flat.hip:386-390: slices of >= 256 rows (about 2048 of them); candidate slots n_slices * k * 16 B <= 2 GiB."""
    sl = max(256, (n_rows + 2047) // 2048)
    sl = (sl + 255) & ~255
    n_slices = max(1, -(-n_rows // sl))
    return max(1, min(nq, GRID_Z, WORKSPACE // (n_slices * k * CAND)))


def flat_filter_chunk(n_rows, nq):
    """ann_flat.hip:111-126: 128-row tiles for nq <= 128, otherwise 256 (both big schedules); the group-minimum matrix
    n_groups * 4 B per query <= 2 GiB in whole query tiles.  No grid cap: the query tiles are grid.x."""
    bm = 128 if nq <= 128 else 256
    n_groups = -(-n_rows // bm) * (bm // 32)
    return min(-(-nq // bm) * bm, max(bm, WORKSPACE // (n_groups * 4) // bm * bm))


def ivf_chunk(nq, nlist, nprobe, kk, ws=WORKSPACE, lut_pair_bytes=0):
    """ann_index.hip:264-289 with one slice per (query, partition) and no table spill -- the production scan once a
    batch has >= 3 pairs per CU or kk > 256 (ann_index.hip:240, 255), IVF_FLAT from 2048 pairs (ann_index.hip:226) -- and
    the batch-level table images' own 16 GiB budget where they apply."""
    per_q = nlist * 4 + nprobe * kk * CAND
    chunk = min(max(1, min(nq, ws // per_q)), GRID_Z)
    if lut_pair_bytes:
        chunk = min(chunk, max(1, LUT_IMAGE_BUDGET // (nprobe * lut_pair_bytes)))
    return chunk


def lut_pair_bytes(m, dsub):
    """ann_lut.hip:15-16: the image (slabs x 256 codes x M columns, sk_shape in kernels_skew.h) + the residual row
    (kernels_lut.h lut_res_stride)."""
    n_slabs = (m + 95) // 96
    per = -(-m // n_slabs)
    M = max(32, (per + 15) & ~15)
    return n_slabs * 256 * M * 4 + (((m + 1) // 2) * 2 * dsub + 16) * 4


def multivec_chunk(n_rows, nq, k):
    """ann_multivec.hip:195-201: row distances 4 B * n_rows <= 1 GiB, candidate slots <= 2 GiB, <= 65 535 sets."""
    sl = max(256, (n_rows + 2047) // 2048)
    sl = (sl + 255) & ~255
    n_slices = max(1, -(-n_rows // sl))
    by_dist = (1 << 30) // max(16, 4 * n_rows)
    by_cand = WORKSPACE // (n_slices * k * CAND)
    return max(1, min(nq, GRID_Z, by_dist, by_cand))


def crossed(nq, chunk):
    """-> [(q0, q1)] of the chunks; at least two, the last one partial."""
    bounds = [(q0, min(nq, q0 + chunk)) for q0 in range(0, nq, chunk)]
    assert len(bounds) >= 2, f"{nq} queries in chunks of {chunk}: one chunk, the boundary is not crossed"
    assert bounds[-1][1] - bounds[-1][0] < chunk, "the last chunk is not partial"
    return bounds


def small_calls(nq, chunk):
    """Calls of 3/4 of a chunk each: every one fits in one chunk, and some straddle the big call's boundaries."""
    s = max(1, 3 * chunk // 4)
    calls = [(a, min(nq, a + s)) for a in range(0, nq, s)]
    assert any(a < b0 < b for a, b in calls for b0, _ in crossed(nq, chunk)[1:])
    return calls


def sample(bounds, nq, seed, n_random=3):
    """The first and last query of every chunk (both sides of each boundary) and a few seeded random ones."""
    s = {q for a, b in bounds for q in (a, b - 1)}
    s |= {int(i) for i in np.random.default_rng(seed).choice(nq, size=n_random, replace=False)}
    return np.array(sorted(s), dtype=np.int64)


# ---- results ---------------------------------------------------------------------------------------------------------
def host(res):
    """A device-I/O SearchResult as numpy (ids u64, distances f32, counts u32)."""
    return lancedb_amd.SearchResult(res.rowids.numpy().view(np.uint64), res.distances.numpy(),
                                    res.counts.numpy().view(np.uint32))


def cat(parts):
    return lancedb_amd.SearchResult(*(np.concatenate([np.asarray(getattr(p, a)) for p in parts])
                                      for a in ("rowids", "distances", "counts")))


def same(a, b, what=""):
    """== on counts, ids (padding included) and the distances of the returned rows."""
    ca, cb = np.asarray(a.counts).astype(np.uint32), np.asarray(b.counts).astype(np.uint32)
    assert ca.shape == cb.shape, what
    bad = np.nonzero(ca != cb)[0]
    assert bad.size == 0, f"{what}: counts differ at queries {bad[:8]}"
    ia, ib = np.asarray(a.rowids).astype(np.uint64), np.asarray(b.rowids).astype(np.uint64)
    bad = np.nonzero((ia != ib).any(axis=1))[0]
    assert bad.size == 0, f"{what}: row ids differ at queries {bad[:8]}"
    live = np.arange(ia.shape[1])[None, :] < ca[:, None]
    da, db = np.asarray(a.distances), np.asarray(b.distances)
    bad = np.nonzero(((da != db) & live).any(axis=1))[0]
    assert bad.size == 0, f"{what}: distances differ at queries {bad[:8]}"


def same_oracle(got, rows, exp, what=""):
    """rows `rows` of `got` against an oracle's (ids, dist, cnt, status)."""
    ids, dist, cnt, st = exp
    assert st == 0
    sub = lancedb_amd.SearchResult(np.asarray(got.rowids)[rows], np.asarray(got.distances)[rows],
                                   np.asarray(got.counts)[rows])
    same(sub, lancedb_amd.SearchResult(ids, dist, cnt), what)


def dev_out(nq, k):
    return DA((nq, k), np.int64), DA((nq, k), np.float32), DA((nq,), np.int32)


_OPENED = []


@pytest.fixture(autouse=True)
def _close_handles():
    """every handle a test opens is closed when the test ends, passed or failed (not by the interpreter's finalisers)"""
    yield
    while _OPENED:
        _OPENED.pop().close()


def _keep(h):
    _OPENED.append(h)
    return h


def _bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# ---- flat ------------------------------------------------------------------------------------------------------------
def _flat_big(fl, q, k, path, launches=None):
    """host and device I/O, profiled and not: all identical; -> the host-I/O result"""
    fl.configure(path=path, profile=True)
    ref = fl.search(q, k=k)
    st = fl.stats()
    assert fl.info()[0] == (1 if path == "filter" else 2)
    if launches is not None:
        assert st["gemm_launches"] == launches, st
        assert st["fallback_queries"] == 0, st  # random data: the filter itself did the work
    fl.configure(path=path, profile=False)
    same(fl.search(q, k=k), ref, f"{path} host I/O, profiling off")
    out = dev_out(len(q), k)
    g = fl.search(DA.from_numpy(q), k=k, out=out)
    fl.sync()
    same(host(g), ref, f"{path} device I/O")
    if launches is not None:
        fl.configure(path=path, profile=True)
        g = fl.search(DA.from_numpy(q), k=k, out=dev_out(len(q), k))
        fl.sync()
        assert fl.stats()["gemm_launches"] == launches
        same(host(g), ref, f"{path} device I/O, profiled")
        fl.configure(path=path, profile=False)
    return ref


def _flat_one_chunk_calls(fl, q, k, path, calls, chunk_of):
    fl.configure(path=path, profile=False)
    parts = []
    for a, b in calls:
        assert chunk_of(b - a) >= b - a  # one chunk each
        parts.append(fl.search(q[a:b], k=k))
    return cat(parts)


def test_f1_flat_sweep_candidate_slot_chunks(oracle):
    n, dim, k, nq = 524_288, 16, 1024, 150
    rng = np.random.default_rng(101)
    v = rng.standard_normal(size=(n, dim), dtype=np.float32)
    q = rng.standard_normal(size=(nq, dim), dtype=np.float32)
    chunk = flat_sweep_chunk(n, nq, k)
    bounds = crossed(nq, chunk)  # 64, 64, 22 at HEAD
    fl = _keep(lancedb_amd.FlatIndex(v))
    ref = _flat_big(fl, q, k, "sweep")
    same(ref, _flat_one_chunk_calls(fl, q, k, "sweep", small_calls(nq, chunk), lambda c: flat_sweep_chunk(n, c, k)),
         "one-chunk calls")
    rows = sample(bounds, nq, seed=1)
    same_oracle(ref, rows, oracle.flat_search(v, q[rows], k=k), "oracle")


def test_f2_flat_filter_group_minimum_chunks(oracle):
    n, dim, k, nq = 4_194_304, 32, 10, 9000
    rng = np.random.default_rng(102)
    bits = _bf16_bits(rng.standard_normal(size=(n, dim), dtype=np.float32))
    q = rng.standard_normal(size=(nq, dim), dtype=np.float32)
    chunk = flat_filter_chunk(n, nq)
    bounds = crossed(nq, chunk)  # 4096, 4096, 808 at HEAD
    fl = _keep(lancedb_amd.FlatIndex(bits, dtype=_abi.DTYPE_BF16))
    assert fl.info()[1] == 1, "the column carries no filter data"
    ref = _flat_big(fl, q, k, "filter", launches=len(bounds))
    same(ref, _flat_one_chunk_calls(fl, q, k, "filter", small_calls(nq, chunk), lambda c: flat_filter_chunk(n, c)),
         "one-chunk calls")
    rows = sample(bounds, nq, seed=2)
    same_oracle(ref, rows, oracle.flat_search(bits, q[rows], k=k, dtype=_abi.DTYPE_BF16), "oracle")


def test_f3_flat_beyond_the_grid_limit(oracle):
    n, dim, k, nq = 5000, 24, 10, 70_000
    rng = np.random.default_rng(103)
    v = rng.standard_normal(size=(n, dim), dtype=np.float32)
    q = rng.standard_normal(size=(nq, dim), dtype=np.float32)
    fl = _keep(lancedb_amd.FlatIndex(v))
    # the sweep caps a chunk at 65 535 queries (grid.z)
    chunk = flat_sweep_chunk(n, nq, k)
    bounds = crossed(nq, chunk)
    calls = small_calls(nq, chunk)
    sweep = _flat_big(fl, q, k, "sweep")
    same(sweep, _flat_one_chunk_calls(fl, q, k, "sweep", calls, lambda c: flat_sweep_chunk(n, c, k)), "sweep one-chunk calls")
    # the MFMA filter has no such cap: ONE launch of 70 144 padded queries, pinned with the same checks
    fc = flat_filter_chunk(n, nq)
    assert fc >= nq and fc % 256 == 0
    filt = _flat_big(fl, q, k, "filter", launches=1)
    same(filt, _flat_one_chunk_calls(fl, q, k, "filter", calls, lambda c: flat_filter_chunk(n, c)), "filter one-chunk calls")
    same(filt, sweep, "filter against sweep")
    rows = sample(bounds, nq, seed=3)
    same_oracle(sweep, rows, oracle.flat_search(v, q[rows], k=k), "oracle")


# ---- IVF-PQ / IVF_FLAT -----------------------------------------------------------------------------------------------
def _ivf_big(ix, q, launches, filter_dev=None, **kw):
    """host and device I/O, profiled (launch count) and not: all identical; -> the host-I/O result"""
    dev_kw = dict(kw)
    if filter_dev is not None:
        dev_kw["allow_rowids"] = filter_dev
    ix.configure(profile=1)
    ref = ix.search(q, **kw)
    st = ix.stats()
    assert st["scan_launches"] == launches[0], st
    ix.configure(profile=0)
    same(ix.search(q, **kw), ref, "host I/O, profiling off")
    dq = DA.from_numpy(q)
    ix.configure(profile=1)
    g = ix.search(dq, out=dev_out(len(q), kw["k"]), **dev_kw)
    ix.sync()
    st = ix.stats()
    assert st["scan_launches"] == launches[1], st
    same(host(g), ref, "device I/O, profiled")
    ix.configure(profile=0)
    g = ix.search(dq, out=dev_out(len(q), kw["k"]), **dev_kw)
    ix.sync()
    same(host(g), ref, "device I/O, profiling off")
    return ref


def _ivf_one_chunk_calls(ix, q, calls, launches_of, **kw):
    """each call profiled: its launch count proves it was one chunk per pass"""
    ix.configure(profile=1)
    parts = []
    for a, b in calls:
        parts.append(ix.search(q[a:b], **kw))
        assert ix.stats()["scan_launches"] == launches_of(a, b), (a, b)
    ix.configure(profile=0)
    return cat(parts)


def _near(rng, s, parts, noise, dim):
    return (s["centroids"][parts] + noise * rng.normal(size=(len(parts), dim))).astype(np.float32)


def test_i1_ivfpq_first_pass_chunks_with_refine_and_deferred_refine(oracle):
    n, dim, nlist, m = 100_000, 64, 256, 8
    nprobe, k, rf, nq = 128, 100, 20, 1200
    kk = k * rf
    s = train.synthetic_index(n, dim, nlist, m, seed=111)
    rng = np.random.default_rng(11)
    raw = rng.standard_normal(size=(n, dim), dtype=np.float32)
    q = _near(rng, s, rng.integers(0, nlist, nq), 0.5, dim)
    assert kk > 256  # (one slice per pair: ann_index.hip:255)
    chunk = ivf_chunk(nq, nlist, nprobe, kk)
    bounds = crossed(nq, chunk)  # 524, 524, 152 at HEAD
    kw = dict(k=k, nprobe_min=nprobe, nprobe_max=nprobe, refine_factor=rf)
    ix = _keep(lancedb_amd.IvfPqIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"],
                                      raw_vectors=raw, raw_host_mapped=True))
    ix.configure(graph=False, coalesce=False)
    ref = _ivf_big(ix, q, (len(bounds), len(bounds)), **kw)
    assert ix.stats()["scan_variant"] == 2, "the production scan did not run"
    # device I/O with the deferred re-rank on: a batch of several chunks keeps the serial re-rank (ann_index.hip:303-304)
    ix.configure(defer_refine=True)
    dq = DA.from_numpy(q)
    g = ix.search(dq, out=dev_out(nq, k), **kw)
    ix.sync()
    same(host(g), ref, "device I/O, deferred refine asked for, several chunks")
    # then one single-chunk call on the same handle, which does defer: still exact
    a, b = bounds[0][1] - 200, bounds[0][1] + 200
    assert ivf_chunk(b - a, nlist, nprobe, kk) >= b - a
    g = ix.search(DA.from_numpy(q[a:b]), out=dev_out(b - a, k), **kw)
    ix.sync()
    same(host(g), cat([lancedb_amd.SearchResult(*(np.asarray(x)[a:b] for x in ref))]), "single-chunk deferred call")
    ix.configure(defer_refine=False)
    same(ref, _ivf_one_chunk_calls(ix, q, small_calls(nq, chunk), lambda a, b: 1, **kw), "one-chunk calls")
    rows = sample(bounds, nq, seed=11)
    o = oracle.OracleIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"], raw_vectors=raw)
    same_oracle(ref, rows, o.search(q[rows], **kw), "oracle")


def test_i2_ivfpq_lut_image_chunks(oracle):
    n, dim, nlist, m = 100_000, 768, 256, 48
    nprobe, k, nq = 128, 10, 6000
    s = train.synthetic_index(n, dim, nlist, m, seed=112)
    rng = np.random.default_rng(12)
    q = _near(rng, s, rng.integers(0, nlist, nq), 0.5, dim)
    chunk = ivf_chunk(nq, nlist, nprobe, k, lut_pair_bytes=lut_pair_bytes(m, dim // m))
    bounds = crossed(nq, chunk)  # 2566, 2566, 868 at HEAD
    kw = dict(k=k, nprobe_min=nprobe, nprobe_max=nprobe)
    ix = _keep(lancedb_amd.IvfPqIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"]))
    ix.configure(graph=False, coalesce=False)
    ref = _ivf_big(ix, q, (len(bounds), len(bounds)), **kw)
    assert ix.stats()["lut_images"] == 1, "the batch-level table kernel did not run"

    def one(a, b):
        assert ix.stats()["lut_images"] == 1
        return 1
    same(ref, _ivf_one_chunk_calls(ix, q, small_calls(nq, chunk), one, **kw), "one-chunk calls")
    rows = sample(bounds, nq, seed=12)
    o = oracle.OracleIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"])
    same_oracle(ref, rows, o.search(q[rows], **kw), "oracle")


def test_i3_ivfpq_beyond_the_grid_limit(oracle):
    n, dim, nlist, m = 20_000, 64, 64, 8
    nprobe, k, rf, nq = 8, 10, 2, 70_000
    s = train.synthetic_index(n, dim, nlist, m, seed=113)
    rng = np.random.default_rng(13)
    raw = rng.standard_normal(size=(n, dim), dtype=np.float32)
    q = _near(rng, s, rng.integers(0, nlist, nq), 0.5, dim)
    chunk = ivf_chunk(nq, nlist, nprobe, k * rf)  # (dsub 8: no table images)
    assert chunk == GRID_Z
    bounds = crossed(nq, chunk)
    kw = dict(k=k, nprobe_min=nprobe, nprobe_max=nprobe, refine_factor=rf)
    ix = _keep(lancedb_amd.IvfPqIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"],
                                      raw_vectors=raw))
    ix.configure(graph=False, coalesce=False)
    ref = _ivf_big(ix, q, (len(bounds), len(bounds)), **kw)
    assert ix.stats()["lut_images"] == 0
    same(ref, _ivf_one_chunk_calls(ix, q, small_calls(nq, chunk), lambda a, b: 1, **kw), "one-chunk calls")
    rows = sample(bounds, nq, seed=13)
    o = oracle.OracleIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"], raw_vectors=raw)
    same_oracle(ref, rows, o.search(q[rows], **kw), "oracle")


def _second_pass_queries(rng, s, nlist, dim, n_long, n_short):
    """An allow list of the rows of a few partitions of >= 120 rows; n_long queries next to those partitions (the first
    pass finds k = 100 rows) and n_short next to others (it does not), shuffled together."""
    lens = np.diff(s["part_offsets"].astype(np.int64))
    big = np.nonzero(lens >= 120)[0]
    allowed = np.sort(rng.choice(big, size=24, replace=False))
    others = np.setdiff1d(np.arange(nlist), allowed)
    po = s["part_offsets"].astype(np.int64)
    allow = np.sort(np.concatenate([s["row_ids"][po[p]:po[p + 1]] for p in allowed])).astype(np.uint64)
    parts = np.concatenate([rng.choice(allowed, n_long), rng.choice(others, n_short)])
    q = _near(rng, s, rng.permutation(parts), 0.3, dim)
    return q, allow


def _second_pass_case(ix, q, allow, short, nlist, k, variant):
    """-> (host-I/O result, chunk bounds of the device-I/O second pass, of the host-I/O one in query order)"""
    nq = len(q)
    n_short = int(short.sum())
    assert 0 < n_short < nq
    first = ivf_chunk(nq, nlist, 4, k)
    assert first >= nq  # the first pass is one chunk
    # host I/O: the second pass runs over exactly the short queries, compacted in query order (k_compact_short)
    c_host = ivf_chunk(n_short, nlist, nlist, k, ws=SECOND_PASS_WS)
    slots = crossed(n_short, c_host)  # 326 per chunk at HEAD
    # device I/O: all nq slots behind the ActiveMask (active ones at the front: the later chunks are partly or wholly idle)
    c_dev = ivf_chunk(nq, nlist, nlist, k, ws=SECOND_PASS_WS)
    dev_bounds = crossed(nq, c_dev)
    assert n_short < dev_bounds[-1][0], "no wholly inactive chunk"
    kw = dict(k=k, nprobe_min=4, nprobe_max=0, allow_rowids=allow)
    ref = _ivf_big(ix, q, (1 + len(slots), 1 + len(dev_bounds)), filter_dev=DA.from_numpy(allow), **kw)
    st = ix.stats()
    assert st["n_queries"] == nq + n_short, "the second pass did not run"
    assert st["scan_variant"] == variant
    sq = np.nonzero(short)[0]
    by_query = [(int(sq[a]), int(sq[b - 1]) + 1) for a, b in slots]

    def one(a, b):  # one chunk per pass: the first, and the second if the call has a short query
        ns = int(short[a:b].sum())
        assert ivf_chunk(b - a, nlist, nlist, k, ws=SECOND_PASS_WS) >= b - a
        return 1 + (ns > 0)
    same(ref, _ivf_one_chunk_calls(ix, q, small_calls(nq, min(c_host, c_dev)), one, **kw), "one-chunk calls")
    return ref, by_query


def test_i4_ivfpq_second_pass_across_chunks(oracle):
    n, dim, nlist, m, k = 200_000, 64, 1024, 8, 100
    s = train.synthetic_index(n, dim, nlist, m, seed=114)
    rng = np.random.default_rng(14)
    q, allow = _second_pass_queries(rng, s, nlist, dim, 500, 1000)
    o = oracle.OracleIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"])
    ids, dist, cnt, st = o.search(q, k=k, nprobe_min=4, nprobe_max=4, allow_rowids=allow)
    assert st == 0
    short = cnt < k
    ix = _keep(lancedb_amd.IvfPqIndex(s["centroids"], s["codebook"], s["part_offsets"], s["codes"], s["row_ids"]))
    ix.configure(graph=False, coalesce=False)
    ref, by_query = _second_pass_case(ix, q, allow, short, nlist, k, variant=2)  # the production scan
    rows = np.union1d(sample([(0, len(q))] + by_query, len(q), seed=14), np.nonzero(~short)[0][:3])
    same_oracle(ref, rows, o.search(q[rows], k=k, nprobe_min=4, nprobe_max=0, allow_rowids=allow), "oracle")


def test_i5_ivf_flat_second_pass_across_chunks(oracle):
    n, dim, nlist, k, metric = 200_000, 64, 1024, 100, "l2"
    s = _dataset(n, dim, nlist, seed=115, empty=8)
    rng = np.random.default_rng(15)
    q, allow = _second_pass_queries(rng, s, nlist, dim, 500, 1000)
    o = _probe_oracle(oracle, s, metric)
    first = _expected(oracle, o, s, q, metric, k, 4, 4, allow_rowids=allow)
    short = first[2] < k
    ix = _keep(lancedb_amd.IvfFlatIndex(s["centroids"], s["part_offsets"], s["raw"], s["row_ids"], metric=metric))
    ix.configure(graph=False, coalesce=False)
    ref, by_query = _second_pass_case(ix, q, allow, short, nlist, k, variant=_abi.SCAN_IVF_FLAT)
    rows = np.union1d(sample([(0, len(q))] + by_query, len(q), seed=15), np.nonzero(~short)[0][:3])
    sub = lancedb_amd.SearchResult(*(np.asarray(x)[rows] for x in (ref.rowids, ref.distances, ref.counts)))
    _same_ivf_flat(sub, _expected(oracle, o, s, q[rows], metric, k, 4, 0, allow_rowids=allow), "restatement")
    _f64_bar(s, q[rows], sub, metric)


# ---- multivector -----------------------------------------------------------------------------------------------------
def _f64_maxsim_bar(vec, off, qsets, res):
    """every returned distance within 1e-4 relative of sum_i min_j (1 - cos(q_i, v_j)) in float64"""
    off = np.asarray(off, dtype=np.int64)
    worst = 0.0
    for b, qs in enumerate(qsets):
        qn = qs.astype(np.float64)
        qn /= np.linalg.norm(qn, axis=1, keepdims=True)
        for j in range(int(res.counts[b])):
            r = int(res.rowids[b, j])
            v = vec[off[r]:off[r + 1]].astype(np.float64)
            v /= np.linalg.norm(v, axis=1, keepdims=True)
            ref = float((1.0 - qn @ v.T).min(axis=1).sum())
            worst = max(worst, abs(float(res.distances[b, j]) - ref) / max(abs(ref), 1e-30))
    assert worst <= 1e-4, worst


def _multivec_case(vec, off, q, k, seed):
    n_rows = len(off) - 1
    nq = len(q)
    chunk = multivec_chunk(n_rows, nq, k)
    bounds = crossed(nq, chunk)
    mv = _keep(lancedb_amd.MultiVectorFlat(vec, off))
    ref = mv.search(q, k=k)
    g = mv.search(DA.from_numpy(q), k=k, out=dev_out(nq, k))
    mv.sync()
    same(host(g), ref, "device I/O")
    parts = []
    for a, b in small_calls(nq, chunk):
        assert multivec_chunk(n_rows, b - a, k) >= b - a
        parts.append(mv.search(q[a:b], k=k))
    same(ref, cat(parts), "one-chunk calls")
    rows = sample(bounds, nq, seed=seed)
    sub = lancedb_amd.SearchResult(*(np.asarray(x)[rows] for x in (ref.rowids, ref.distances, ref.counts)))
    assert_same_multivec(sub, restate(vec, _abi.DTYPE_F32, off, q[rows], k))
    _f64_maxsim_bar(vec, off, q[rows], sub)
    return bounds


def test_m1_multivector_row_distance_chunks():
    n_rows, dim, nqv, k, nq = 1_048_576, 16, 4, 10, 600
    rng = np.random.default_rng(121)
    lens = rng.integers(0, 4, size=n_rows)
    off = np.zeros(n_rows + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    vec = rng.standard_normal(size=(int(off[-1]), dim), dtype=np.float32)
    q = rng.standard_normal(size=(nq, nqv, dim), dtype=np.float32)
    bounds = _multivec_case(vec, off, q, k, seed=21)
    assert len(bounds) == 3  # 256, 256, 88 at HEAD: the row-distance budget


def test_m2_multivector_beyond_the_grid_limit():
    n_rows, dim, nqv, k, nq = 500, 8, 2, 10, 70_000
    rng = np.random.default_rng(122)
    lens = rng.integers(0, 4, size=n_rows)
    off = np.zeros(n_rows + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    vec = rng.standard_normal(size=(int(off[-1]), dim), dtype=np.float32)
    q = rng.standard_normal(size=(nq, nqv, dim), dtype=np.float32)
    bounds = _multivec_case(vec, off, q, k, seed=22)
    assert bounds[0] == (0, GRID_Z)
