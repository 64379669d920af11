"""IVF_FLAT indexes (MI355_INDEX_IVF_FLAT) on the host side: descriptor checks that run before any device is
touched, the assign-only encode's argument checks, the builder's defaults and the table / plan surface.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import lancedb_amd
from lancedb_amd import _abi, _lib


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _flat_desc(**over):
    """A valid IVF_FLAT descriptor over host arrays: 4 partitions of one row each, dim 8."""
    cen = np.zeros((4, 8), np.float32)
    po = np.array([0, 1, 2, 3, 4], np.uint64)
    raw = np.zeros((4, 8), np.float32)
    cb = np.zeros((2, 256, 4), np.float32)
    codes = np.zeros((4, 2), np.uint8)
    d = _abi.IndexDesc()
    d.struct_size = C.sizeof(_abi.IndexDesc)
    d.dim, d.nlist, d.m, d.nbits, d.metric, d.n_rows = 8, 4, 0, 0, 0, 4
    d.flags = _abi.INDEX_IVF_FLAT
    d.centroids = cen.ctypes.data_as(C.c_void_p)
    d.part_offsets = po.ctypes.data_as(C.c_void_p)
    d.raw_vectors = raw.ctypes.data_as(C.c_void_p)
    d.raw_dtype = _abi.DTYPE_F32
    d.shard_count = 1
    for k, v in over.items():
        if v == "codebook":
            v = cb.ctypes.data_as(C.c_void_p)
        elif v == "codes":
            v = codes.ctypes.data_as(C.c_void_p)
        setattr(d, k, v)
    return d, (cen, po, raw, cb, codes)


def test_abi_constants():
    assert lancedb_amd.lib().mi355_abi_version() == _abi.ABI_VERSION == 6
    assert (_abi.INDEX_IVF_FLAT, _abi.SCAN_IVF_FLAT) == (8, 3)


@pytest.mark.parametrize("over,status,needle", [
    (dict(m=2), _abi.ERR_INVALID_INPUT, "m must be 0"),
    (dict(codebook="codebook"), _abi.ERR_INVALID_INPUT, "codebook and codes NULL"),
    (dict(codes="codes"), _abi.ERR_INVALID_INPUT, "codebook and codes NULL"),
    (dict(raw_vectors=None), _abi.ERR_INVALID_INPUT, "needs raw_vectors"),
    (dict(flags=_abi.INDEX_IVF_FLAT | _abi.INDEX_GENERIC_SCAN), _abi.ERR_INVALID_INPUT, "MI355_INDEX_GENERIC_SCAN"),
    (dict(flags=_abi.INDEX_IVF_FLAT | _abi.INDEX_RAW_HOST_MAPPED), _abi.ERR_NOT_SUPPORTED, "MI355_INDEX_RAW_HOST_MAPPED"),
    (dict(flags=_abi.INDEX_IVF_FLAT | 64), _abi.ERR_INVALID_INPUT, "unknown index flags"),
    (dict(n_rows=5), _abi.ERR_INVALID_INPUT, "part_offsets"),
    (dict(metric=9), _abi.ERR_INVALID_INPUT, "metric"),
    (dict(raw_dtype=7), _abi.ERR_INVALID_INPUT, "raw_dtype"),
])
def test_ivf_flat_descriptor_rejections(L, over, status, needle):
    d, keep = _flat_desc(**over)
    h = C.c_void_p()
    assert L.mi355_index_open(C.byref(d), C.byref(h)) == status
    assert needle in _lib.last_error()
    assert not h.value


def test_valid_ivf_flat_descriptor_reaches_the_device_check(L):
    """A valid IVF_FLAT descriptor passes every host check; without a GPU it fails only because there is no device
    (before this flag existed it was rejected as 'unknown index flags')."""
    if lancedb_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    for nbits in (0, 8):  # (nbits is ignored by an IVF_FLAT descriptor)
        d, keep = _flat_desc(nbits=nbits)
        h = C.c_void_p()
        assert L.mi355_index_open(C.byref(d), C.byref(h)) == _abi.ERR_RUNTIME
        assert "no HIP device" in _lib.last_error()
    with pytest.raises(lancedb_amd.EngineError, match="no HIP device"):
        lancedb_amd.IvfFlatIndex(np.zeros((4, 8), np.float32), np.array([0, 1, 2, 3, 4], np.uint64),
                                 np.zeros((4, 8), np.float32))


def test_assign_only_encode_validates_before_touching_a_device(L):
    cent = np.zeros((4, 8), np.float32)
    cb = np.zeros((2, 256, 4), np.float32)
    po = np.zeros(5, np.uint64)
    order = np.zeros(3, np.uint64)
    x = np.zeros((3, 8), np.float32)
    codes = np.zeros((3, 2), np.uint8)

    def call(n=0, out_codes=None, out_order=None, **over):
        f = dict(struct_size=C.sizeof(_abi.EncodeDesc), dim=8, nlist=4, m=0, nbits=0, metric=0, mem=0, device=0,
                 centroids=cent.ctypes.data, codebook=None)
        f.update(over)
        d = _abi.EncodeDesc(**f)
        return L.mi355_ivfpq_encode(C.byref(d), C.c_void_p(x.ctypes.data), C.c_uint64(n), C.c_void_p(po.ctypes.data),
                                    out_codes, out_order, None)

    # m = 0 is assign-only only with no codebook and no codes
    assert call(codebook=cb.ctypes.data) == _abi.ERR_INVALID_INPUT and "assign-only" in _lib.last_error()
    assert call(out_codes=C.c_void_p(codes.ctypes.data)) == _abi.ERR_INVALID_INPUT and "assign-only" in _lib.last_error()
    assert call(centroids=None) == _abi.ERR_INVALID_INPUT and "NULL" in _lib.last_error()
    assert call(n=3) == _abi.ERR_INVALID_INPUT and "NULL" in _lib.last_error()  # order is still required
    assert call(metric=7) == _abi.ERR_INVALID_INPUT
    if lancedb_amd.device_count() == 0:
        assert call(n=3, out_order=C.c_void_p(order.ctypes.data)) == _abi.ERR_RUNTIME and "no HIP device" in _lib.last_error()
    with pytest.raises(ValueError):
        lancedb_amd.ivf_flat_assign(x, np.zeros((4, 6), np.float32))


def test_ivf_flat_builder_defaults_follow_the_reference():
    """IvfFlatIndexBuilder::default() (rust/lancedb/src/index/vector.rs:194-204): l2, no partition count / size,
    sample_rate 256, max_iterations 50."""
    b = lancedb_amd.IvfFlatBuilder()
    assert (b.distance_type, b.num_partitions, b.target_partition_size, b.sample_rate, b.max_iterations) == \
        ("l2", None, None, 256, 50)
    with pytest.raises(ValueError):
        lancedb_amd.IvfFlatBuilder(num_partitions=20).train(np.zeros((10, 16), np.float32))


def _unopened_flat_index(dim):
    """An IvfFlatIndex object without a device handle (enough for the table's construction and the plan)."""
    ix = lancedb_amd.IvfFlatIndex.__new__(lancedb_amd.IvfFlatIndex)
    lancedb_amd.index._Handle.__init__(ix)
    ix.dim, ix.nlist, ix.m, ix.metric = dim, 4, 0, _abi.METRIC_L2
    return ix


def test_vector_table_accepts_an_ivf_flat_index_and_names_it_in_the_plan():
    ix = _unopened_flat_index(8)
    t = lancedb_amd.VectorTable(index=ix)
    assert t.index is ix and t.dim == 8
    q = t.query_nearest_to(np.ones(8, np.float32)).limit(5).refine_factor(3)
    text = q.explain_plan()
    assert "ANNSubIndex: name=mi355_ivf_flat, k=5" in text and "mi355_ivf_pq" not in text
    assert "KNNVectorDistance: refine" not in text  # exact distances already: refine_factor changes nothing
