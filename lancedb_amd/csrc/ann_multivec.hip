// ann_multivec.hip — the multivector (List<FixedSizeList>) handle behind include/mi355_multivec.h: exact late-interaction
// search (sum over the query vectors of the minimum cosine distance to a row's vectors).  Replaces the reference's
// KNNVectorDistance over a multivector column + SortExec TopK (rust/lancedb/src/table/query.rs:169-199).
// The entry points are those of the companion header include/mi355_multivec.h (mi355_ann.h, the v6 surface, is
// unchanged); they take their C linkage from its extern "C" declarations.  Each is a function-try-block closed by
// MI355_MV_ABI_GUARD, i.e. MI355_ABI_GUARD with the entry point's full name: tests/test_multivec_abi.py checks the
// barrier from the source and the exported names from the library, as tests/test_abi.py does for mi355_ann.h.
#include "ann_internal.h"
#include "kernels_multivec.h"
#include "../../include/mi355_multivec.h"

#define MI355_MV_ABI_GUARD(suffix) MI355_ABI_GUARD("mi355_multivec_" suffix)

struct mi355_multivec {
  int32_t device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::mutex mu;
  uint32_t dim = 0, dtype = 0;
  uint64_t n_rows = 0, n_vectors = 0, n_tiles = 0;
  const void* col = nullptr;  // the column the scan reads: `vectors` (copied) or the caller's device array
  DevBuf vectors, vv, offsets, tile_row0, row_ids;
  bool has_row_ids = false;
  DevBuf w_q, w_qq, w_dist, w_cand, w_ids, w_dist_out, w_cnt, w_filter;
};

static const char* metric_name(uint32_t m) {
  return m == MI355_METRIC_L2 ? "l2" : m == MI355_METRIC_DOT ? "dot" : m == MI355_METRIC_COSINE ? "cosine" : "unknown";
}

// cosine only (lance: "only cosine similarity is supported for multi-vectors"); DEFAULT means cosine
static int32_t check_multivec_metric(uint32_t metric) {
  if (metric == MI355_METRIC_COSINE || metric == MI355_METRIC_DEFAULT) return MI355_OK;
  if (metric == MI355_METRIC_L2 || metric == MI355_METRIC_DOT)
    return fail(MI355_ERR_NOT_SUPPORTED, "multivector search supports only the cosine metric, not %s", metric_name(metric));
  return fail(MI355_ERR_INVALID_INPUT, "unknown metric %u", metric);
}

static int32_t check_offsets(const uint64_t* off, uint64_t n_rows, uint64_t n_vectors) {
  if (off[0] != 0) return fail(MI355_ERR_INVALID_INPUT, "offsets[0] = %llu, must be 0", (unsigned long long)off[0]);
  for (uint64_t r = 0; r < n_rows; ++r)
    if (off[r + 1] < off[r])
      return fail(MI355_ERR_INVALID_INPUT, "offsets decrease at row %llu (%llu > %llu)", (unsigned long long)r,
                  (unsigned long long)off[r], (unsigned long long)off[r + 1]);
  if (off[n_rows] != n_vectors)
    return fail(MI355_ERR_INVALID_INPUT, "offsets[n_rows] = %llu != n_vectors %llu", (unsigned long long)off[n_rows],
                (unsigned long long)n_vectors);
  return MI355_OK;
}

int32_t mi355_multivec_open(const mi355_multivec_desc* d, mi355_multivec** out) try {
  if (!out) return fail(MI355_ERR_INVALID_INPUT, "out is NULL");
  *out = nullptr;
  if (!d) return fail(MI355_ERR_INVALID_INPUT, "desc is NULL");
  if (d->struct_size != sizeof(mi355_multivec_desc))
    return fail(MI355_ERR_INVALID_INPUT, "mi355_multivec_desc.struct_size %u != %zu (ABI mismatch)", d->struct_size,
                sizeof(mi355_multivec_desc));
  if (d->dim == 0) return fail(MI355_ERR_INVALID_INPUT, "dim must be > 0");
  if (d->dtype > MI355_DTYPE_F16) return fail(MI355_ERR_INVALID_INPUT, "unknown dtype %u", d->dtype);
  if (d->mem > MI355_MEM_DEVICE) return fail(MI355_ERR_INVALID_INPUT, "unknown mem %u", d->mem);
  ST_TRY(check_multivec_metric(d->metric));
  if (!d->offsets) return fail(MI355_ERR_INVALID_INPUT, "offsets is NULL");
  if (d->n_vectors && !d->vectors) return fail(MI355_ERR_INVALID_INPUT, "vectors is NULL");
  if (d->n_vectors >= 0xFFFFFFF0ull || d->n_rows >= 0xFFFFFFF0ull)
    return fail(MI355_ERR_NOT_SUPPORTED, "multivector column limited to 2^32-16 vectors and rows");
  if ((size_t)d->dim * 4 > 60u * 1024) return fail(MI355_ERR_NOT_SUPPORTED, "dim %u too large", d->dim);
  if (d->mem == MI355_MEM_HOST) ST_TRY(check_offsets(d->offsets, d->n_rows, d->n_vectors));
  ST_TRY(need_device(d->device));
  mi355_multivec* h = new (std::nothrow) mi355_multivec();
  if (!h) return fail(MI355_ERR_RUNTIME, "out of host memory");
  h->device = d->device;
  h->dim = d->dim;
  h->dtype = d->dtype;
  h->n_rows = d->n_rows;
  h->n_vectors = d->n_vectors;
  auto bail = [&](int32_t s) {
    mi355_multivec_close(h);
    return s;
  };
  if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess)
    return bail(fail(MI355_ERR_RUNTIME, "hipStreamCreate failed"));
  h->stream = h->own_stream;
  // the offsets on the host: checked (device arrays are read back first) and cut into tiles of whole rows
  std::vector<uint64_t> off(d->n_rows + 1);
  if (d->mem == MI355_MEM_DEVICE) {
    if (hipMemcpy(off.data(), d->offsets, sizeof(uint64_t) * off.size(), hipMemcpyDeviceToHost) != hipSuccess)
      return bail(fail(MI355_ERR_RUNTIME, "read-back of the offsets failed"));
    int32_t s = check_offsets(off.data(), d->n_rows, d->n_vectors);
    if (s) return bail(s);
  } else {
    memcpy(off.data(), d->offsets, sizeof(uint64_t) * off.size());
  }
  // a tile: up to MV_MAXR rows and MV_VT vectors, or one row longer than MV_VT
  std::vector<uint64_t> tiles;
  for (uint64_t r = 0; r < d->n_rows;) {
    tiles.push_back(r);
    uint64_t nv = 0;
    uint32_t nr = 0;
    while (r < d->n_rows && nr < MV_MAXR) {
      const uint64_t len = off[r + 1] - off[r];
      if (nr > 0 && nv + len > MV_VT) break;
      nv += len;
      ++nr;
      ++r;
      if (len > MV_VT) break;
    }
  }
  h->n_tiles = tiles.size();
  tiles.push_back(d->n_rows);
  const size_t vb = dtype_size(d->dtype) * (size_t)d->dim * d->n_vectors;
  int32_t s;
  if (d->mem == MI355_MEM_DEVICE) {
    h->col = d->vectors;  // scanned where it lives
  } else {
    s = h->vectors.ensure(std::max<size_t>(vb, 16));
    if (s) return bail(s);
    if (copy_in(h->vectors.p, d->vectors, vb, d->mem, h->stream) != hipSuccess)
      return bail(fail(MI355_ERR_RUNTIME, "upload of the vector column failed"));
    h->col = h->vectors.p;
  }
  s = h->offsets.ensure(sizeof(uint64_t) * off.size());
  if (s) return bail(s);
  s = h->tile_row0.ensure(sizeof(uint64_t) * tiles.size());
  if (s) return bail(s);
  s = h->vv.ensure(std::max<size_t>(sizeof(float) * d->n_vectors, 16));
  if (s) return bail(s);
  if (hipMemcpyAsync(h->offsets.p, off.data(), sizeof(uint64_t) * off.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
      hipMemcpyAsync(h->tile_row0.p, tiles.data(), sizeof(uint64_t) * tiles.size(), hipMemcpyHostToDevice, h->stream) != hipSuccess)
    return bail(fail(MI355_ERR_RUNTIME, "upload of the offsets failed"));
  if (d->row_ids) {
    s = h->row_ids.ensure(std::max<size_t>(sizeof(uint64_t) * d->n_rows, 16));
    if (s) return bail(s);
    if (copy_in(h->row_ids.p, d->row_ids, sizeof(uint64_t) * d->n_rows, d->mem, h->stream) != hipSuccess)
      return bail(fail(MI355_ERR_RUNTIME, "upload of row ids failed"));
    h->has_row_ids = true;
  }
  if (d->n_vectors) {
    hipLaunchKernelGGL(k_multivec_norms, dim3((uint32_t)((d->n_vectors + 255) / 256)), dim3(256), 0, h->stream, h->col,
                       d->dtype, d->n_vectors, d->dim, h->vv.as<float>());
    if (hipGetLastError() != hipSuccess) return bail(fail(MI355_ERR_RUNTIME, "launch of k_multivec_norms failed"));
  }
  // (the host staging vectors above are released on return: wait for their copies)
  if (hipStreamSynchronize(h->stream) != hipSuccess) return bail(fail(MI355_ERR_RUNTIME, "building the column failed"));
  *out = h;
  return MI355_OK;
} MI355_MV_ABI_GUARD("open")

int32_t mi355_multivec_close(mi355_multivec* h) try {
  if (!h) return MI355_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  DevBuf* bufs[] = {&h->vectors, &h->vv,    &h->offsets, &h->tile_row0, &h->row_ids, &h->w_q,      &h->w_qq,
                    &h->w_dist,  &h->w_cand, &h->w_ids,  &h->w_dist_out, &h->w_cnt, &h->w_filter};
  for (DevBuf* b : bufs) b->release();
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
  return MI355_OK;
} MI355_MV_ABI_GUARD("close")

int32_t mi355_multivec_set_stream(mi355_multivec* h, void* hip_stream) try {
  if (!h) return fail(MI355_ERR_INVALID_INPUT, "multivector handle is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  return MI355_OK;
} MI355_MV_ABI_GUARD("set_stream")

int32_t mi355_multivec_sync(mi355_multivec* h) try {
  if (!h) return fail(MI355_ERR_INVALID_INPUT, "multivector handle is NULL");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return MI355_OK;
} MI355_MV_ABI_GUARD("sync")

int32_t mi355_multivec_info(const mi355_multivec* h, uint64_t* out_rows, uint64_t* out_vectors) try {
  if (!h) return fail(MI355_ERR_INVALID_INPUT, "multivector handle is NULL");
  if (out_rows) *out_rows = h->n_rows;
  if (out_vectors) *out_vectors = h->n_vectors;
  return MI355_OK;
} MI355_MV_ABI_GUARD("info")

// the device work of a search over device-resident query sets (h->mu held by the caller; stream work only)
static int32_t run_multivec_device(mi355_multivec* h, const float* d_q, uint32_t nq, uint32_t n_qvec,
                                   const mi355_search_params* p, uint64_t* d_ids, float* d_dist, uint32_t* d_cnt) {
  hipStream_t st = h->stream;
  const uint32_t k = p->k;
  const int kpl = kpl_for(k);  // k > 256: the selection runs in passes of 256 rows
  RowFilter flt;
  ST_TRY(make_row_filter(p, h->w_filter, st, &flt));
  const uint64_t n_qv = (uint64_t)nq * n_qvec;
  ST_TRY(h->w_qq.ensure(sizeof(float) * n_qv));
  hipLaunchKernelGGL(k_multivec_prep, dim3((uint32_t)((n_qv + 255) / 256)), dim3(256), 0, st, d_q, n_qv, h->dim,
                     h->w_qq.as<float>());
  HIP_TRY(hipGetLastError());
  // selection work items as the flat sweep cuts them: at least 256 rows, about 2048 items per query set
  uint32_t slice = (uint32_t)std::max<uint64_t>(256, (h->n_rows + 2047) / 2048);
  slice = (slice + 255u) & ~255u;
  const uint32_t n_slices = (uint32_t)std::max<uint64_t>(1, (h->n_rows + slice - 1) / slice);
  // query sets per pass: the row distances ([chunk, n_rows] f32) within ~1 GiB, the candidate slots within ~2 GiB
  const size_t by_dist = ((size_t)1 << 30) / std::max<size_t>(16, sizeof(float) * h->n_rows);
  const size_t by_cand = ((size_t)2048 << 20) / ((size_t)n_slices * k * sizeof(Cand));
  const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min(nq, 65535u), std::min(by_dist, by_cand)));
  ST_TRY(h->w_dist.ensure(std::max<size_t>(16, sizeof(float) * (size_t)chunk * h->n_rows)));
  ST_TRY(h->w_cand.ensure(sizeof(Cand) * (size_t)chunk * n_slices * k));
  for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
    const uint32_t n = std::min(chunk, nq - q0);
    if (h->n_tiles) {
      MultivecScanArgs sa;
      sa.vectors = h->col;
      sa.dtype = h->dtype;
      sa.dim = h->dim;
      sa.vv = h->vv.as<float>();
      sa.offsets = h->offsets.as<uint64_t>();
      sa.tile_row0 = h->tile_row0.as<uint64_t>();
      sa.q = d_q + (size_t)q0 * n_qvec * h->dim;
      sa.qq = h->w_qq.as<float>() + (size_t)q0 * n_qvec;
      sa.nb = n;
      sa.n_qvec = n_qvec;
      sa.n_rows = h->n_rows;
      sa.dist = h->w_dist.as<float>();
      hipLaunchKernelGGL(k_multivec_scan, dim3((uint32_t)h->n_tiles), dim3(256), 0, st, sa);
      HIP_TRY(hipGetLastError());
    }
    MultivecSelectArgs xa;
    xa.dist = h->w_dist.as<float>();
    xa.row_ids = h->has_row_ids ? h->row_ids.as<uint64_t>() : nullptr;
    xa.n_rows = h->n_rows;
    xa.slice_rows = slice;
    xa.n_slices = n_slices;
    xa.kk = k;
    xa.range.has_lower = p->has_lower_bound;
    xa.range.has_upper = p->has_upper_bound;
    xa.range.lower = p->lower_bound;
    xa.range.upper = p->upper_bound;
    xa.filter = flt;
    xa.cand = h->w_cand.as<Cand>();
    launch_by_kpl(kpl, k_multivec_select<1>, k_multivec_select<2>, k_multivec_select<4>, dim3(n_slices, 1, n), dim3(256), 0,
                  st, xa);
    HIP_TRY(hipGetLastError());
    MergeArgs ma = merge_args_dense(h->w_cand.as<Cand>(), n_slices, k, n, k);
    ma.out_ids = d_ids + (size_t)q0 * k;
    ma.out_dist = d_dist + (size_t)q0 * k;
    ma.out_cnt = d_cnt + q0;
    launch_by_kpl(kpl, k_merge_cands<1>, k_merge_cands<2>, k_merge_cands<4>, dim3(n), dim3(64), 0, st, ma);
    HIP_TRY(hipGetLastError());
  }
  return MI355_OK;
}

int32_t mi355_multivec_search(mi355_multivec* h, const float* queries, uint32_t n_queries, uint32_t n_qvec,
                                         const mi355_search_params* p, uint64_t* out_rowids, float* out_dist,
                                         uint32_t* out_counts) try {
  // (the query-set shape and the metric are checked before the handle: they need no device)
  if (n_qvec == 0 || n_qvec > MI355_MULTIVEC_MAX_QVEC)
    return fail(MI355_ERR_INVALID_INPUT, "n_qvec must be 1..%u, got %u", MI355_MULTIVEC_MAX_QVEC, n_qvec);
  ST_TRY(validate_params(p));
  ST_TRY(check_multivec_metric(p->metric));
  if (!h) return fail(MI355_ERR_INVALID_INPUT, "multivector handle is NULL");
  if (n_queries == 0) return MI355_OK;
  if (!queries || !out_counts || (p->k && (!out_rowids || !out_dist)))
    return fail(MI355_ERR_INVALID_INPUT, "NULL query / output buffer");
  const uint32_t k = p->k;
  std::lock_guard<std::mutex> lk(h->mu);
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const bool host_io = p->io_mem == MI355_MEM_HOST;
  if (k == 0) {
    if (host_io) memset(out_counts, 0, sizeof(uint32_t) * n_queries);
    else HIP_TRY(hipMemsetAsync(out_counts, 0, sizeof(uint32_t) * n_queries, st));
    return MI355_OK;
  }
  auto t_start = std::chrono::steady_clock::now();
  const float* d_q = queries;
  uint64_t* d_ids = out_rowids;
  float* d_dist = out_dist;
  uint32_t* d_cnt = out_counts;
  if (host_io) {
    const size_t q_bytes = sizeof(float) * (size_t)n_queries * n_qvec * h->dim;
    ST_TRY(h->w_q.ensure(q_bytes));
    ST_TRY(h->w_ids.ensure(sizeof(uint64_t) * (size_t)n_queries * k));
    ST_TRY(h->w_dist_out.ensure(sizeof(float) * (size_t)n_queries * k));
    ST_TRY(h->w_cnt.ensure(sizeof(uint32_t) * n_queries));
    HIP_TRY(hipMemcpyAsync(h->w_q.p, queries, q_bytes, hipMemcpyHostToDevice, st));
    d_q = h->w_q.as<float>();
    d_ids = h->w_ids.as<uint64_t>();
    d_dist = h->w_dist_out.as<float>();
    d_cnt = h->w_cnt.as<uint32_t>();
  }
  ST_TRY(run_multivec_device(h, d_q, n_queries, n_qvec, p, d_ids, d_dist, d_cnt));
  if (host_io) {
    HIP_TRY(hipMemcpyAsync(out_rowids, d_ids, sizeof(uint64_t) * (size_t)n_queries * k, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_dist, d_dist, sizeof(float) * (size_t)n_queries * k, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_counts, d_cnt, sizeof(uint32_t) * n_queries, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (p->timeout_ms) {
      auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_start).count();
      if (ms > (long long)p->timeout_ms)
        return fail(MI355_ERR_TIMEOUT, "Query timeout: %lld ms > %u ms", (long long)ms, p->timeout_ms);
    }
  }
  return MI355_OK;
} MI355_MV_ABI_GUARD("search")
