"""Exact multivector (late-interaction / MaxSim) search on the GPU (include/mi355_ann.h mi355_multivec_*).

Expected results come from the restatement below, built on the oracle's flat cosine search: the oracle's distance
of query vector i against every stored vector is the contract's pair(i, j); the row minima are np.fmin.reduceat over
the row offsets (NaN for a row without vectors), summed over i in float32, i ascending.  Ids and distances are
compared with ==."""
import numpy as np
import pytest

import lancedb_amd
from lancedb_amd import _abi
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _bf16_bits(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _stored(vec_f32, dtype):
    """The column as the engine stores it: f32, or uint16 bits of bf16 / f16."""
    if dtype == _abi.DTYPE_F32:
        return np.ascontiguousarray(vec_f32, dtype=np.float32)
    if dtype == _abi.DTYPE_BF16:
        return _bf16_bits(vec_f32)
    return np.ascontiguousarray(vec_f32, dtype=np.float16).view(np.uint16)


def row_distances(stored, dtype, offsets, qset):
    """dist(r) of one query set [n_qvec, dim] over every row (NaN: no vectors / NaN sum)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    n_rows, n_vec = len(offsets) - 1, int(offsets[-1])
    lens = np.diff(offsets)
    total = np.full(n_rows, np.nan, np.float32)
    if n_vec == 0:
        return total
    ids, dist, cnt, st = orc.flat_search(stored, qset, k=n_vec, metric=_abi.METRIC_COSINE, row_ids=np.arange(n_vec),
                                         dtype=dtype)
    assert st == 0
    nz = lens > 0
    for i in range(qset.shape[0]):
        pair = np.full(n_vec, np.nan, np.float32)
        pair[ids[i, :cnt[i]].astype(np.int64)] = dist[i, :cnt[i]]
        m = np.full(n_rows, np.nan, np.float32)
        m[nz] = np.fmin.reduceat(pair, offsets[:-1][nz])
        total = m if i == 0 else (total + m).astype(np.float32)
    return total


def restate(stored, dtype, offsets, queries, k, row_ids=None, lower=None, upper=None, allow=None, block=None):
    """-> per query set (ids u64, distances f32): the k smallest rows by (dist, row id)."""
    n_rows = len(offsets) - 1
    rid = np.arange(n_rows, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, dtype=np.uint64)
    out = []
    for qset in np.asarray(queries, dtype=np.float32):
        d = row_distances(stored, dtype, offsets, qset)
        keep = ~np.isnan(d)
        if lower is not None:
            keep &= d >= np.float32(lower)
        if upper is not None:
            keep &= d < np.float32(upper)
        if allow is not None:
            keep &= np.isin(rid, np.asarray(allow, dtype=np.uint64))
        if block is not None:
            keep &= ~np.isin(rid, np.asarray(block, dtype=np.uint64))
        ids, dd = rid[keep], d[keep]
        order = np.lexsort((ids, dd))[:k]
        out.append((ids[order], dd[order]))
    return out


def assert_same(res, expect):
    assert len(res.counts) == len(expect)
    for b, (ids, dist) in enumerate(expect):
        n = int(res.counts[b])
        assert n == len(ids), (b, n, len(ids))
        assert (np.asarray(res.rowids[b, :n], dtype=np.uint64) == ids).all(), b
        assert (np.asarray(res.distances[b, :n]) == dist).all(), b


def ragged_offsets(rng, n_rows, max_len=64, long_row=None, empty_every=9):
    lens = rng.integers(1, max_len + 1, size=n_rows)
    lens[::empty_every] = 0
    if long_row is not None:
        lens[n_rows // 2] = long_row
    off = np.zeros(n_rows + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    return off


# ---- the reference's own test (python/python/tests/test_query.py:790-820) -------------------------------------------
@pytest.mark.parametrize("vt", ["float16", "float32"])
def test_reference_multivector_fixture(vt):
    import pyarrow as pa
    t = pa.list_(pa.list_(getattr(pa, vt)(), 2))
    col = pa.array([[[i, i + 1], [i + 2, i + 3]] for i in range(256)], type=t)
    table = lancedb_amd.VectorTable(flat=lancedb_amd.MultiVectorFlat.from_arrow(col))
    rs = table.search([1, 2]).execute()
    rs2 = table.search([[1, 2], [1, 2]]).execute()
    assert "query_index" not in rs2
    assert len(rs2["_rowid"]) == len(rs["_rowid"]) == 10
    assert (rs2["_rowid"] == rs["_rowid"]).all()
    assert (rs2["_distance"] == rs["_distance"] * 2).all()
    with pytest.raises(lancedb_amd.InvalidInput):
        table.search([1, 2, 3]).execute()
    with pytest.raises(lancedb_amd.InvalidInput):
        table.search([[1, 2], [1, 2, 3]]).execute()
    # and the restatement
    vec, off, dt = lancedb_amd.multivector_from_arrow(col)
    st = _stored(vec, dt) if dt != _abi.DTYPE_F16 else vec.view(np.uint16)
    exp = restate(st, dt, off, np.array([[[1, 2], [1, 2]]], np.float32), 10)
    assert (rs2["_rowid"] == exp[0][0]).all() and (rs2["_distance"] == exp[0][1]).all()


# ---- the restatement over ragged columns, dims, dtypes, query-set sizes, batches and k ------------------------------
CASES = [
    # dim, dtype, n_qvec, batch, k
    (2, _abi.DTYPE_F32, 1, 1, 10),
    (3, _abi.DTYPE_F16, 7, 5, 1),
    (96, _abi.DTYPE_BF16, 32, 5, 10),
    (128, _abi.DTYPE_F32, 33, 5, 300),
    (128, _abi.DTYPE_BF16, 7, 64, 10),
    (768, _abi.DTYPE_F16, 33, 1, 10),
    (768, _abi.DTYPE_F32, 300, 1, 300),
    (96, _abi.DTYPE_F32, 1, 64, 1),
]


@pytest.mark.parametrize("dim,dtype,n_qvec,batch,k", CASES)
def test_matches_the_restatement(dim, dtype, n_qvec, batch, k):
    rng = np.random.default_rng(dim * 1000 + n_qvec * 10 + batch)
    off = ragged_offsets(rng, 420, long_row=2100)
    n_vec = int(off[-1])
    vec = rng.normal(size=(n_vec, dim)).astype(np.float32)
    stored = _stored(vec, dtype)
    q = rng.normal(size=(batch, n_qvec, dim)).astype(np.float32)
    with lancedb_amd.MultiVectorFlat(stored, off, dtype=dtype) as mv:
        assert mv.info() == (420, n_vec)
        res = mv.search(q, k=k)
    assert_same(res, restate(stored, dtype, off, q, k))


def test_filters_range_and_offset_through_the_table():
    rng = np.random.default_rng(7)
    dim = 64
    off = ragged_offsets(rng, 500, long_row=2000)
    vec = rng.normal(size=(int(off[-1]), dim)).astype(np.float32)
    row_ids = (np.arange(500, dtype=np.uint64) * 3 + 11)
    q = rng.normal(size=(5, dim)).astype(np.float32)
    mv = lancedb_amd.MultiVectorFlat(vec, off, row_ids=row_ids)
    t = lancedb_amd.VectorTable(flat=mv)
    full = restate(vec, _abi.DTYPE_F32, off, q[None], 500, row_ids=row_ids)[0]
    allow = row_ids[rng.choice(500, 150, replace=False)]
    block = row_ids[rng.choice(500, 200, replace=False)]
    for kw, qb in ((dict(allow=allow), lambda x: x.only_if_rowids(allow=allow)),
                   (dict(block=block), lambda x: x.only_if_rowids(block=block))):
        out = qb(t.search(q).limit(20)).execute()
        exp = restate(vec, _abi.DTYPE_F32, off, q[None], 20, row_ids=row_ids, **kw)[0]
        assert (out["_rowid"] == exp[0]).all() and (out["_distance"] == exp[1]).all()
    lo, hi = float(full[1][30]), float(full[1][80])
    out = t.search(q).distance_range(lo, hi).limit(100).execute()
    exp = restate(vec, _abi.DTYPE_F32, off, q[None], 100, row_ids=row_ids, lower=lo, upper=hi)[0]
    assert (out["_rowid"] == exp[0]).all() and (out["_distance"] == exp[1]).all() and len(exp[0]) == 50
    out = t.search(q).offset(7).limit(13).execute()
    assert (out["_rowid"] == full[0][7:20]).all() and (out["_distance"] == full[1][7:20]).all()
    with pytest.raises(lancedb_amd.NotSupported):
        t.search(q).distance_type("l2").execute()


def test_device_io_and_a_borrowed_device_column():
    """(DeviceArray: the GPU tests keep torch out of the test process.)"""
    DA = lancedb_amd.DeviceArray
    rng = np.random.default_rng(3)
    dim = 128
    off = ragged_offsets(rng, 300, long_row=2200)
    vec = rng.normal(size=(int(off[-1]), dim)).astype(np.float32)
    bits = _bf16_bits(vec)
    q = rng.normal(size=(5, 32, dim)).astype(np.float32)
    host = lancedb_amd.MultiVectorFlat(bits, off, dtype=_abi.DTYPE_BF16)
    ref = host.search(q, k=40)
    dev = lancedb_amd.MultiVectorFlat(DA.from_numpy(bits), DA.from_numpy(off), dtype=_abi.DTYPE_BF16)
    got = dev.search(DA.from_numpy(q), k=40)
    dev.sync()
    assert (got.counts.numpy() == ref.counts).all()
    assert (got.rowids.numpy().view(np.uint64) == ref.rowids).all()
    assert (got.distances.numpy() == ref.distances).all()
    assert_same(ref, restate(bits, _abi.DTYPE_BF16, off, q, 40))
    # a single query set on the device: one result row
    one = dev.search(DA.from_numpy(q[2]), k=40)
    dev.sync()
    assert one.counts.numpy().tolist() == [ref.counts[2]] and (one.rowids.numpy().view(np.uint64)[0] == ref.rowids[2]).all()


def test_one_vector_per_row_equals_the_flat_cosine_search():
    rng = np.random.default_rng(11)
    n, dim = 6000, 128
    vec = rng.normal(size=(n, dim)).astype(np.float32)
    q = rng.normal(size=(8, dim)).astype(np.float32)
    off = np.arange(n + 1, dtype=np.uint64)
    mv = lancedb_amd.MultiVectorFlat(vec, off)
    got = mv.search(q[:, None, :], k=50)
    fl = lancedb_amd.FlatIndex(vec)
    for path in ("filter", "sweep"):
        fl.configure(path=path)
        ref = fl.search(q, k=50, metric=_abi.METRIC_COSINE)
        assert (got.counts == ref.counts).all()
        assert (got.rowids == ref.rowids).all() and (got.distances == ref.distances).all()


def test_zero_vectors_and_nan_elements_are_never_returned():
    rng = np.random.default_rng(5)
    dim = 16
    off = ragged_offsets(rng, 60, max_len=5)
    vec = rng.normal(size=(int(off[-1]), dim)).astype(np.float32)
    lens = np.diff(off.astype(np.int64))
    starts = off[:-1].astype(np.int64)
    # rows whose every vector is zero (0/0 pairs: NaN) and rows with a NaN element in every vector
    zero_rows = [r for r in range(60) if lens[r] > 0][:6]
    nan_rows = [r for r in range(60) if lens[r] > 0][6:10]
    for r in zero_rows:
        vec[starts[r]:starts[r] + lens[r]] = 0
    for r in nan_rows:
        vec[starts[r]:starts[r] + lens[r], 3] = np.nan
    # and a row where only one vector is NaN: its other vectors still give a minimum
    mixed = [r for r in range(60) if lens[r] > 1][-1]
    vec[starts[mixed], 0] = np.nan
    q = rng.normal(size=(3, 4, dim)).astype(np.float32)
    eligible = int(((lens > 0).sum()) - len(zero_rows) - len(nan_rows))
    with lancedb_amd.MultiVectorFlat(vec, off) as mv:
        res = mv.search(q, k=100)
    assert (res.counts == eligible).all()
    bad = set(zero_rows) | set(nan_rows) | {r for r in range(60) if lens[r] == 0}
    for b in range(3):
        assert not bad & set(res.rowids[b, :res.counts[b]].tolist())
        assert mixed in res.rowids[b, :res.counts[b]].tolist()
    assert_same(res, restate(vec, _abi.DTYPE_F32, off, q, 100))


def test_a_larger_column_on_a_sample_of_queries():
    """200 k rows of 16-48 vectors (mean 32), 128-d, 16 query sets of 8 vectors; two query sets restated."""
    rng = np.random.default_rng(2026)
    n_rows, dim = 200_000, 128
    lens = rng.integers(16, 49, size=n_rows)
    off = np.zeros(n_rows + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    vec = rng.standard_normal(size=(int(off[-1]), dim), dtype=np.float32)
    q = rng.normal(size=(16, 8, dim)).astype(np.float32)
    mv = lancedb_amd.MultiVectorFlat(lancedb_amd.DeviceArray.from_numpy(vec), lancedb_amd.DeviceArray.from_numpy(off))
    res = mv.search(q, k=10)
    assert (res.counts == 10).all()
    for b in (0, 13):
        exp = restate(vec, _abi.DTYPE_F32, off, q[b:b + 1], 10)[0]
        assert (res.rowids[b] == exp[0]).all() and (res.distances[b] == exp[1]).all()


def test_wire_query_with_a_list_of_vectors_is_one_result_set():
    from lancedb_amd import wire
    rng = np.random.default_rng(9)
    off = ragged_offsets(rng, 200)
    vec = rng.normal(size=(int(off[-1]), 8)).astype(np.float32)
    t = lancedb_amd.VectorTable(flat=lancedb_amd.MultiVectorFlat(vec, off))
    q = rng.normal(size=(3, 8)).astype(np.float32)
    ctype, data = wire.handle_query(t, {"vector": q.tolist(), "k": 7})
    cols = wire.response_from_ipc(data)
    assert "query_index" not in cols
    exp = restate(vec, _abi.DTYPE_F32, off, q[None], 7)[0]
    assert (cols["_rowid"] == exp[0]).all() and (cols["_distance"] == exp[1]).all()
