"""IVF_FLAT indexes on the GPU (MI355_INDEX_IVF_FLAT, k_ivf_flat_scan).  The expected result is composed from the
CPU oracle: the probes of an IVF-PQ index with the same centroids and metric (OracleIndex.coarse + select_probes over
dummy m = 1 PQ arrays, with the maximum_nprobes second pass when the first returns fewer than k rows), then
oracle.flat_search over the rows of those partitions with their row ids.  Counts, ids and distances are compared
with ==; the distances are also held to the 1e-4 float64 bar of tests/test_gpu_float_bar.py."""
import numpy as np
import pytest

import lancedb_amd
from lancedb_amd import _abi
from lancedb_amd.distributed import Comm, ShardedSearcher, run_ranks

pytestmark = pytest.mark.gpu
U64 = np.uint64(0xFFFFFFFFFFFFFFFF)
DTYPES = {"f32": _abi.DTYPE_F32, "bf16": _abi.DTYPE_BF16, "f16": _abi.DTYPE_F16}


def _dataset(n, dim, nlist, seed, dtype="f32", empty=3):
    """Centroids, partition offsets (`empty` partitions without rows), raw rows near their centroid in index order
    (f32, or the u16 bits of bf16 / f16) and unique non-identity row ids."""
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(nlist, dim)).astype(np.float32)
    w = rng.gamma(1.0, size=nlist)
    w[rng.choice(nlist, size=empty, replace=False)] = 0.0
    lens = np.floor(w / w.sum() * n).astype(np.int64)
    lens[np.argmax(lens)] += n - lens.sum()
    po = np.zeros(nlist + 1, np.uint64)
    po[1:] = np.cumsum(lens)
    part = np.repeat(np.arange(nlist), lens)
    x = (cen[part] + 0.6 * rng.normal(size=(n, dim))).astype(np.float32)
    if dtype == "bf16":
        raw = (x.view(np.uint32) >> 16).astype(np.uint16)
    elif dtype == "f16":
        raw = x.astype(np.float16).view(np.uint16)
    else:
        raw = x
    ids = (rng.permutation(3 * n)[:n] + 7).astype(np.uint64)
    return dict(centroids=cen, part_offsets=po, raw=raw, row_ids=ids, dtype=dtype)


def _decode(raw, dtype):
    if dtype == "bf16":
        return (raw.astype(np.uint32) << 16).view(np.float32)
    if dtype == "f16":
        return raw.view(np.float16).astype(np.float32)
    return raw


def _probe_oracle(oracle, s, metric):
    nlist, dim = s["centroids"].shape
    n = int(s["part_offsets"][-1])
    return oracle.OracleIndex(s["centroids"], np.zeros((1, 256, dim), np.float32), s["part_offsets"],
                              np.zeros((n, 1), np.uint8), s["row_ids"], metric=metric)


def _expected(oracle, o, s, q, metric, k, nprobe_min, nprobe_max, **flt):
    """Per query: the probes of the IVF-PQ oracle (second pass at nprobe_max when the first has fewer than k rows),
    then the flat search over those partitions' rows."""
    nlist = s["centroids"].shape[0]
    po = s["part_offsets"].astype(np.int64)
    nmin = min(nprobe_min, nlist)
    nmax = nlist if not nprobe_max or nprobe_max > nlist else nprobe_max
    nq = q.shape[0]
    ids = np.full((nq, k), U64, np.uint64)
    dist = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.uint32)
    for i in range(nq):
        c = o.coarse(q[i])
        for npr in ((nmin, nmax) if nmax > nmin else (nmin,)):
            probes = o.select_probes(c, npr)
            rows = np.concatenate([np.arange(po[p], po[p + 1]) for p in probes])
            if rows.size:
                fi, fd, fc, st = oracle.flat_search(s["raw"][rows], q[i:i + 1], k=k, metric=_abi.METRIC_NAMES[metric],
                                                    row_ids=s["row_ids"][rows], dtype=DTYPES[s["dtype"]], **flt)
                assert st == 0
                ids[i], dist[i], cnt[i] = fi[0], fd[0], fc[0]
            else:
                ids[i], dist[i], cnt[i] = U64, np.inf, 0
            if cnt[i] >= k:
                break
    return ids, dist, cnt


def _same(got, exp, what=""):
    ids, dist, cnt = exp
    gi, gd, gc = (np.asarray(a) for a in (got.rowids, got.distances, got.counts))
    assert (gc == cnt).all(), what
    for i in range(len(cnt)):
        n = int(cnt[i])
        assert (gi[i, :n].astype(np.uint64) == ids[i, :n]).all(), f"{what} query {i}"
        assert (gd[i, :n] == dist[i, :n]).all(), f"{what} query {i}"
        assert (gi[i, n:].astype(np.uint64) == U64).all(), f"{what} query {i} padding"


def _f64_bar(s, q, got, metric):
    """every returned distance within 1e-4 relative of a float64 evaluation of the metric"""
    pos_of = {int(r): j for j, r in enumerate(s["row_ids"])}
    x = _decode(s["raw"], s["dtype"]).astype(np.float64)
    worst = 0.0
    for i in range(q.shape[0]):
        n = int(np.asarray(got.counts)[i])
        if n == 0:
            continue
        rows = np.array([pos_of[int(r)] for r in np.asarray(got.rowids)[i, :n].astype(np.uint64)])
        v, qq = x[rows], q[i].astype(np.float64)
        if metric == "l2":
            ref = ((v - qq) ** 2).sum(1)
        elif metric == "dot":
            ref = 1.0 - v @ qq
        else:
            ref = 1.0 - (v @ qq) / (np.sqrt((qq * qq).sum()) * np.sqrt((v * v).sum(1)))
        d = np.asarray(got.distances)[i, :n].astype(np.float64)
        worst = max(worst, float(np.max(np.abs(d - ref) / np.maximum(np.abs(ref), 1e-30))))
    assert worst <= 1e-4, worst


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


def _open(s, metric, **kw):
    return _keep(lancedb_amd.IvfFlatIndex(s["centroids"], s["part_offsets"], s["raw"], s["row_ids"], metric=metric,
                                          raw_dtype=DTYPES[s["dtype"]], **kw))


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_ivf_flat_equals_probes_plus_flat_search(oracle, metric, dtype):
    dim, nlist, n = 64, 40, 12000
    s = _dataset(n, dim, nlist, seed=11 + len(dtype) + len(metric), dtype=dtype)
    rng = np.random.default_rng(5)
    q = (s["centroids"][rng.integers(0, nlist, 8)] + 0.8 * rng.normal(size=(8, dim))).astype(np.float32)
    o = _probe_oracle(oracle, s, metric)
    ix = _open(s, metric)
    assert ix.info() == (n, int((np.diff(s["part_offsets"].astype(np.int64)) > 0).sum()))
    for k in (1, 10, 100, 300):
        for npr in (1, 20, 0):  # 0 = all partitions
            kw = dict(k=k, nprobe_min=npr or nlist, nprobe_max=npr)
            got = ix.search(q, **kw)
            _same(got, _expected(oracle, o, s, q, metric, **kw), f"{metric} {dtype} {kw}")
            if k == 10:
                _f64_bar(s, q, got, metric)
    st = ix.stats()
    assert st["scan_variant"] == _abi.SCAN_IVF_FLAT
    assert st["vectors_scanned"] > 0
    assert st["code_bytes_scanned"] == st["vectors_scanned"] * dim * (4 if dtype == "f32" else 2)


def test_ranges_filters_second_pass_and_refine(oracle):
    dim, nlist, n, metric = 48, 32, 10000, "l2"
    s = _dataset(n, dim, nlist, seed=3, empty=4)
    rng = np.random.default_rng(9)
    q = (s["centroids"][rng.integers(0, nlist, 16)] + 0.8 * rng.normal(size=(16, dim))).astype(np.float32)
    o = _probe_oracle(oracle, s, metric)
    ix = _open(s, metric)
    base = _expected(oracle, o, s, q, metric, k=30, nprobe_min=8, nprobe_max=8)
    lo, hi = float(np.median(base[1][:, 5])), float(np.median(base[1][:, 25]))
    # an allow list from the rows of a few partitions: most queries come back short from 2 probes and take the second pass
    po = s["part_offsets"].astype(np.int64)
    allow = np.sort(np.concatenate([s["row_ids"][po[p]:po[p + 1]] for p in (1, 7, 19)]))
    block = np.sort(rng.choice(s["row_ids"], size=n // 3, replace=False))
    cases = [dict(k=20, nprobe_min=8, nprobe_max=8, upper_bound=hi),
             dict(k=20, nprobe_min=8, nprobe_max=8, lower_bound=lo, upper_bound=hi),
             dict(k=10, nprobe_min=2, nprobe_max=16, allow_rowids=allow),   # min < max: the second pass
             dict(k=15, nprobe_min=5, nprobe_max=5, block_rowids=block),
             dict(k=20, nprobe_min=2, nprobe_max=0, upper_bound=hi)]         # second pass over all partitions
    for kw in cases:
        flt = {a: kw[a] for a in ("lower_bound", "upper_bound", "allow_rowids", "block_rowids") if a in kw}
        exp = _expected(oracle, o, s, q, metric, kw["k"], kw["nprobe_min"], kw["nprobe_max"], **flt)
        _same(ix.search(q, **kw), exp, str({a: v for a, v in kw.items() if not a.endswith("rowids")}))
        if "allow_rowids" in kw:
            assert ix.stats()["n_queries"] > len(q)  # the allow list did force a second pass
    # refine_factor is accepted and changes nothing: the distances are exact already
    r0 = ix.search(q, k=10, nprobe_min=8, nprobe_max=8)
    r5 = ix.search(q, k=10, nprobe_min=8, nprobe_max=8, refine_factor=5)
    for a, b in zip(r0, r5):
        assert (np.asarray(a) == np.asarray(b)).all()
    with pytest.raises(lancedb_amd.InvalidInput, match="IVF_FLAT"):
        ix.attach_raw_vectors(np.zeros((n, dim), np.float32))
    with pytest.raises(lancedb_amd.InvalidInput):
        ix.detach_raw_vectors()


@pytest.mark.parametrize("nq", [1, 8, 64, 2048])
def test_batch_sizes(oracle, nq):
    dim, nlist, n, metric = 32, 64, 40000, "l2"
    s = _dataset(n, dim, nlist, seed=21)
    rng = np.random.default_rng(nq)
    q = (s["centroids"][rng.integers(0, nlist, nq)] + 0.8 * rng.normal(size=(nq, dim))).astype(np.float32)
    o = _probe_oracle(oracle, s, metric)
    ix = _open(s, metric)
    _same(ix.search(q, k=10, nprobe_min=20, nprobe_max=20), _expected(oracle, o, s, q, metric, 10, 20, 20), f"nq {nq}")


def test_probe_entry_points_and_device_column(oracle):
    """coarse_topn / search_probes on an IVF_FLAT handle, and a column that stays in the caller's device memory
    (DeviceArray: the GPU tests keep torch out of the test process)."""
    DA = lancedb_amd.DeviceArray
    dim, nlist, n, metric = 64, 48, 15000, "cosine"
    s = _dataset(n, dim, nlist, seed=31)
    rng = np.random.default_rng(2)
    q = (s["centroids"][rng.integers(0, nlist, 12)] + 0.8 * rng.normal(size=(12, dim))).astype(np.float32)
    o = _probe_oracle(oracle, s, metric)
    exp = _expected(oracle, o, s, q, metric, 25, 12, 12)
    ix = _open(s, metric)
    pid, pd, pc = ix.coarse_topn(q, 12)
    assert (pc == 12).all()
    for i in range(len(q)):
        assert sorted(pid[i].astype(np.int64)) == sorted(o.select_probes(o.coarse(q[i]), 12).astype(np.int64))
    _same(ix.search_probes(q, pid, k=25), exp, "search_probes")
    d_raw = DA.from_numpy(s["raw"])
    dev = _keep(lancedb_amd.IvfFlatIndex(DA.from_numpy(s["centroids"]), s["part_offsets"], d_raw,
                                         DA.from_numpy(s["row_ids"]), metric=metric))
    _same(dev.search(q, k=25, nprobe_min=12, nprobe_max=12), exp, "borrowed device column")
    out = (DA((12, 25), np.int64), DA((12, 25), np.float32), DA((12,), np.int32))
    g = dev.search(DA.from_numpy(q), k=25, nprobe_min=12, nprobe_max=12, out=out)  # device I/O
    dev.sync()
    _same(lancedb_amd.SearchResult(g.rowids.numpy().view(np.uint64), g.distances.numpy(), g.counts.numpy()), exp, "device I/O")
    dev.close()  # (before the column it borrows is freed)
    del d_raw


def test_loopback_shards_equal_the_unsharded_index(oracle):
    world, dim, nlist, n, metric = 2, 64, 40, 16000, "dot"
    s = _dataset(n, dim, nlist, seed=41)
    rng = np.random.default_rng(4)
    q = (s["centroids"][rng.integers(0, nlist, 24)] + 0.8 * rng.normal(size=(24, dim))).astype(np.float32)
    with _open(s, metric) as whole:
        cases = [dict(k=10, nprobe_min=10, nprobe_max=10), dict(k=100, nprobe_min=5, nprobe_max=5, refine_factor=3),
                 dict(k=20, nprobe_min=2, nprobe_max=12, upper_bound=float(whole.search(q, k=20).distances[0, 3]))]
        exp = [whole.search(q, **kw) for kw in cases]
    o = _probe_oracle(oracle, s, metric)
    _same(exp[0], _expected(oracle, o, s, q, metric, 10, 10, 10), "unsharded")
    shards = [_open(s, metric, shard_count=world, shard_rank=r) for r in range(world)]
    assert sum(sh.info()[0] for sh in shards) == n
    comms = Comm.loopback(world)
    try:
        got = run_ranks([lambda r=r: [ShardedSearcher(shards[r], comms[r]).search(q, _abi.make_params(**kw)) for kw in cases]
                         for r in range(world)])
    finally:  # (released here, not by the interpreter's finalisers)
        for h in shards + comms:
            h.close()
    for r in range(world):
        for kw, g, e in zip(cases, got[r], exp):
            for a, b in zip(g, e):
                assert (np.asarray(a) == np.asarray(b)).all(), f"rank {r} {kw}"


def test_built_index_uses_the_pq_encoders_assignment(oracle):
    dim, n, metric = 32, 20000, "l2"
    rng = np.random.default_rng(8)
    x = (rng.normal(size=(16, dim))[rng.integers(0, 16, n)] + 0.5 * rng.normal(size=(n, dim))).astype(np.float32)
    b = lancedb_amd.IvfFlatBuilder(num_partitions=16, max_iterations=5)
    ix = _keep(b.build(x))
    cen = b.train(x)
    po, order, assign = lancedb_amd.ivf_flat_assign(x, cen, return_assign=True)
    cb = rng.normal(size=(dim // 16, 256, 16)).astype(np.float32)
    po2, _, order2, assign2 = lancedb_amd.ivfpq_encode(x, cen, cb, return_assign=True)
    assert (po == po2).all() and (order == order2).all() and (assign == assign2).all()
    s = dict(centroids=cen, part_offsets=po, raw=x[order.astype(np.int64)], row_ids=order.astype(np.uint64), dtype="f32")
    q = x[:32] + np.float32(0.1)
    o = _probe_oracle(oracle, s, metric)
    _same(ix.search(q, k=10, nprobe_min=4, nprobe_max=4), _expected(oracle, o, s, q, metric, 10, 4, 4), "built index")
    # through the table layer: the same rows as the handle
    t = lancedb_amd.VectorTable(index=ix)
    got = t.query_nearest_to(q[0]).limit(10).nprobes(4).to_list()
    assert [int(r["_rowid"]) for r in got] == [int(v) for v in ix.search(q[:1], k=10, nprobe_min=4, nprobe_max=4).rowids[0]]
