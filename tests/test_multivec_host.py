"""Multivector columns (mi355_multivec_*) on the host side: descriptor and argument checks that run before any device
is touched, the Arrow conversion, the restatement's own properties, the table / plan surface and the kernel unit's
scratch check.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lancedb_amd
from lancedb_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_multivec.h")
MV_SYMBOLS = ("mi355_multivec_open", "mi355_multivec_close", "mi355_multivec_set_stream", "mi355_multivec_sync",
              "mi355_multivec_info", "mi355_multivec_search")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _desc(**over):
    """A valid descriptor over host arrays: 3 rows of 2, 0 and 1 vectors, dim 4."""
    vec = np.zeros((3, 4), np.float32)
    off = np.array([0, 2, 2, 3], np.uint64)
    d = _abi.MultivecDesc()
    d.struct_size = C.sizeof(_abi.MultivecDesc)
    d.dim, d.n_rows, d.n_vectors, d.dtype, d.mem, d.metric = 4, 3, 3, _abi.DTYPE_F32, _abi.MEM_HOST, _abi.METRIC_COSINE
    d.vectors = vec.ctypes.data_as(C.c_void_p)
    d.offsets = off.ctypes.data_as(C.c_void_p)
    keep = [vec, off]
    for k, v in over.items():
        if k == "offsets" and v is not None:
            v = np.ascontiguousarray(v, dtype=np.uint64)
            keep.append(v)
            v = v.ctypes.data_as(C.c_void_p)
        setattr(d, k, v)
    return d, keep


def test_abi_version_stays_6_and_the_struct_matches_the_header(tmp_path):
    assert lancedb_amd.lib().mi355_abi_version() == _abi.ABI_VERSION == 6
    c = tmp_path / "sz.c"
    c.write_text('#include "mi355_multivec.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %u\\n",'
                 'sizeof(mi355_multivec_desc), offsetof(mi355_multivec_desc, offsets), offsetof(mi355_multivec_desc, device),'
                 ' MI355_MULTIVEC_MAX_QVEC);return 0;}')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(c), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = _abi.MultivecDesc
    assert out == [C.sizeof(D), D.offsets.offset, D.device.offset, _abi.MULTIVEC_MAX_QVEC]
    assert _abi.MULTIVEC_MAX_QVEC >= 1024


def test_export_list_and_header_agree(L):
    declared = set(re.findall(r"\b(mi355_multivec_[a-z_]+)\s*\(", open(HEADER).read()))
    assert declared == set(MV_SYMBOLS)
    assert set(MV_SYMBOLS) == set(_abi.MULTIVEC_SYMBOLS)
    for name in MV_SYMBOLS:
        assert getattr(L, name) is not None


@pytest.mark.parametrize("over,status,needle", [
    (dict(struct_size=8), _abi.ERR_INVALID_INPUT, "struct_size"),
    (dict(dim=0), _abi.ERR_INVALID_INPUT, "dim must be > 0"),
    (dict(vectors=None), _abi.ERR_INVALID_INPUT, "vectors is NULL"),
    (dict(offsets=None), _abi.ERR_INVALID_INPUT, "offsets is NULL"),
    (dict(offsets=[1, 2, 2, 3]), _abi.ERR_INVALID_INPUT, "offsets[0] = 1, must be 0"),
    (dict(offsets=[0, 2, 1, 3]), _abi.ERR_INVALID_INPUT, "offsets decrease at row 1"),
    (dict(offsets=[0, 2, 2, 2]), _abi.ERR_INVALID_INPUT, "offsets[n_rows] = 2 != n_vectors 3"),
    (dict(dtype=3), _abi.ERR_INVALID_INPUT, "unknown dtype 3"),
    (dict(mem=2), _abi.ERR_INVALID_INPUT, "unknown mem 2"),
    (dict(metric=_abi.METRIC_L2), _abi.ERR_NOT_SUPPORTED, "only the cosine metric, not l2"),
    (dict(metric=_abi.METRIC_DOT), _abi.ERR_NOT_SUPPORTED, "only the cosine metric, not dot"),
    (dict(metric=7), _abi.ERR_INVALID_INPUT, "unknown metric 7"),
    (dict(n_vectors=0xFFFFFFF0), _abi.ERR_NOT_SUPPORTED, "2^32-16"),
])
def test_descriptor_rejections(L, over, status, needle):
    d, keep = _desc(**over)
    h = C.c_void_p()
    assert L.mi355_multivec_open(C.byref(d), C.byref(h)) == status
    assert needle in _lib.last_error()
    assert not h.value


def test_valid_descriptors_reach_the_device_check(L):
    """Every host check passes (cosine and the default metric, with and without row ids); without a GPU the open fails
    only because there is no device."""
    if lancedb_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    rid = np.arange(3, dtype=np.uint64)
    for over in (dict(), dict(metric=_abi.METRIC_DEFAULT), dict(row_ids=rid.ctypes.data_as(C.c_void_p))):
        d, keep = _desc(**over)
        h = C.c_void_p()
        assert L.mi355_multivec_open(C.byref(d), C.byref(h)) == _abi.ERR_RUNTIME
        assert "no HIP device" in _lib.last_error()
    with pytest.raises(lancedb_amd.EngineError, match="no HIP device"):
        lancedb_amd.MultiVectorFlat(np.zeros((3, 4), np.float32), np.array([0, 2, 2, 3], np.uint64))


@pytest.mark.parametrize("n_qvec,metric,status,needle", [
    (0, _abi.METRIC_DEFAULT, _abi.ERR_INVALID_INPUT, "n_qvec must be 1..1024, got 0"),
    (1025, _abi.METRIC_COSINE, _abi.ERR_INVALID_INPUT, "n_qvec must be 1..1024, got 1025"),
    (4, _abi.METRIC_L2, _abi.ERR_NOT_SUPPORTED, "not l2"),
    (4, _abi.METRIC_DOT, _abi.ERR_NOT_SUPPORTED, "not dot"),
    (4, 9, _abi.ERR_INVALID_INPUT, "unknown metric 9"),
    (4, _abi.METRIC_COSINE, _abi.ERR_INVALID_INPUT, "handle is NULL"),
    (1024, _abi.METRIC_DEFAULT, _abi.ERR_INVALID_INPUT, "handle is NULL"),
])
def test_search_arguments_are_checked_before_the_handle(L, n_qvec, metric, status, needle):
    p = _abi.make_params(k=10, metric=metric)
    q = np.zeros((1, max(n_qvec, 1), 4), np.float32)
    ids = np.zeros((1, 10), np.uint64)
    dist = np.zeros((1, 10), np.float32)
    cnt = np.zeros(1, np.uint32)
    s = L.mi355_multivec_search(None, q.ctypes.data_as(C.c_void_p), C.c_uint32(1), C.c_uint32(n_qvec), C.byref(p),
                                ids.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                                cnt.ctypes.data_as(C.c_void_p))
    assert s == status and needle in _lib.last_error()


# ---- Arrow conversion ------------------------------------------------------------------------------------------------
def _column(list_type, value_type, rows):
    import pyarrow as pa
    dim = 3
    return pa.array(rows, type=list_type(pa.list_(value_type, dim)))


ROWS = [[[1, 2, 3], [4, 5, 6]], None, [], [[7, 8, 9]], None, [[10, 11, 12], [13, 14, 15], [16, 17, 18]]]


@pytest.mark.parametrize("list_type", ["list_", "large_list"])
@pytest.mark.parametrize("vt,np_dt,dtype", [("float16", np.float16, _abi.DTYPE_F16), ("float32", np.float32, _abi.DTYPE_F32),
                                            ("float64", np.float32, _abi.DTYPE_F32)])
def test_from_arrow(list_type, vt, np_dt, dtype):
    import pyarrow as pa
    col = _column(getattr(pa, list_type), getattr(pa, vt)(), ROWS)
    vec, off, dt = lancedb_amd.multivector_from_arrow(col)
    assert dt == dtype and vec.dtype == np_dt and off.dtype == np.uint64
    assert off.tolist() == [0, 2, 2, 2, 3, 3, 6]  # null rows become empty rows
    assert (vec == np.arange(1, 19, dtype=np_dt).reshape(6, 3)).all()
    # a slice with a non-zero offset, starting at a null row
    vec, off, dt = lancedb_amd.multivector_from_arrow(col.slice(1, 4))
    assert off.tolist() == [0, 0, 0, 1, 1] and (vec == np.array([[7, 8, 9]], np_dt)).all()
    vec, off, dt = lancedb_amd.multivector_from_arrow(col.slice(3))
    assert off.tolist() == [0, 1, 1, 4] and (vec == np.arange(7, 19, dtype=np_dt).reshape(4, 3)).all()
    # a chunked column
    vec, off, dt = lancedb_amd.multivector_from_arrow(pa.chunked_array([col.slice(0, 2), col.slice(2)]))
    assert off.tolist() == [0, 2, 2, 2, 3, 3, 6]


def test_from_arrow_narrows_float64_and_rejects_other_types():
    import pyarrow as pa
    col = pa.array([[[1.0 + 2 ** -40, 2.0]]], type=pa.list_(pa.list_(pa.float64(), 2)))
    vec, off, dt = lancedb_amd.multivector_from_arrow(col)
    assert vec.dtype == np.float32 and vec[0, 0] == np.float32(1.0)
    with pytest.raises(lancedb_amd.InvalidInput):
        lancedb_amd.multivector_from_arrow(pa.array([[1.0, 2.0]], type=pa.list_(pa.float32())))
    with pytest.raises(lancedb_amd.InvalidInput):
        lancedb_amd.multivector_from_arrow(pa.array([[[1, 2]]], type=pa.list_(pa.list_(pa.int32(), 2))))


# ---- the restatement the GPU tests compare against -------------------------------------------------------------------
def _restatement():
    from tests import test_gpu_multivec
    return test_gpu_multivec


def test_restatement_doubles_for_a_repeated_query_vector():
    """[q, q] gives exactly 2x the distances of [q] in the same row order (python/python/tests/test_query.py:808-813)."""
    t = _restatement()
    rng = np.random.default_rng(1)
    off = t.ragged_offsets(rng, 50, max_len=6)
    vec = rng.normal(size=(int(off[-1]), 8)).astype(np.float32)
    q = rng.normal(size=(1, 8)).astype(np.float32)
    one = t.restate(vec, _abi.DTYPE_F32, off, q[None], 20)[0]
    two = t.restate(vec, _abi.DTYPE_F32, off, np.stack([q, q], 1).reshape(1, 2, 8), 20)[0]
    assert (one[0] == two[0]).all() and (two[1] == one[1] * 2).all()


def test_restatement_with_one_vector_per_row_is_the_flat_cosine_search():
    from oracle import oracle as orc
    t = _restatement()
    rng = np.random.default_rng(2)
    vec = rng.normal(size=(300, 16)).astype(np.float32)
    vec[5] = 0  # a zero row: NaN, dropped by both
    q = rng.normal(size=(3, 16)).astype(np.float32)
    off = np.arange(301, dtype=np.uint64)
    got = t.restate(vec, _abi.DTYPE_F32, off, q[:, None, :], 40)
    ids, dist, cnt, st = orc.flat_search(vec, q, k=40, metric=_abi.METRIC_COSINE)
    for b in range(3):
        assert (got[b][0] == ids[b, :cnt[b]]).all() and (got[b][1] == dist[b, :cnt[b]]).all()
        assert 5 not in got[b][0]


# ---- the table and its plan ------------------------------------------------------------------------------------------
def _unopened(dim):
    mv = lancedb_amd.MultiVectorFlat.__new__(lancedb_amd.MultiVectorFlat)
    lancedb_amd.index._Handle.__init__(mv)
    mv.dim = dim
    return mv


def test_table_takes_a_multivector_column_as_one_query_set():
    t = lancedb_amd.VectorTable(flat=_unopened(2))
    q = t.search([[1, 2], [3, 4], [5, 6]]).limit(5)
    assert len(q.request.query_vector) == 3
    plan = q.create_plan()
    assert plan.output_columns() == ["_rowid", "_distance"]  # no query_index: ONE result set
    text = q.explain_plan()
    assert "KNNVectorDistance: multivector, metric=cosine, n_qvec=3" in text and "UnionExec" not in text
    with pytest.raises(lancedb_amd.InvalidInput):
        t.search([1, 2, 3])
    with pytest.raises(lancedb_amd.InvalidInput):
        t.search([[1, 2], [1, 2, 3]])
    with pytest.raises(lancedb_amd.NotSupported):
        lancedb_amd.VectorTable(index=object(), flat=_unopened(2))


def test_wire_body_with_a_list_of_vectors_is_one_multivector_query():
    from lancedb_amd import wire
    t = lancedb_amd.VectorTable(flat=_unopened(2))
    req = wire.request_from_json({"vector": [[1.0, 2.0], [3.0, 4.0]], "k": 4})
    plan = lancedb_amd.VectorQuery(t, req).create_plan()
    assert plan.queries.shape == (2, 2) and plan.output_columns() == ["_rowid", "_distance"]


def test_kernel_unit_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_scratch.py"),
                        os.path.join(ROOT, "lancedb_amd", "csrc", "ann_multivec.hip")],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kernels with scratch outside the allow-list: 0" in r.stdout
