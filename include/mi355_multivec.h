/*
 * mi355_multivec.h — multivector (List<FixedSizeList>) columns: the companion header of mi355_ann.h.
 *
 * The same library (libmi355_ann.so) and the same conventions as include/mi355_ann.h: int32 statuses
 * (lancedb::Error variants), no exception crosses the boundary, the caller owns every buffer, plain
 * pointers and sizes only.  This header adds one handle type and its entry points; it changes nothing
 * declared in mi355_ann.h.  Rust bindings: integration/mi355_multivec_sys.rs (generated from this file).
 */
#ifndef MI355_MULTIVEC_H
#define MI355_MULTIVEC_H

#include "mi355_ann.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * ---- multivector columns (List<FixedSizeList<float, dim>>: ColBERT / ColPali late-interaction
 *      embeddings; python/python/lancedb/embeddings/colpali.py, pydantic.py:135-205) ----------------
 * Exact (flat) late-interaction search.  Additive to ABI version 6: a new handle type and new entry
 * points in this companion header; include/mi355_ann.h is unchanged, so MI355_ANN_ABI_VERSION stays 6.
 *
 * A row r holds n_r >= 0 vectors x_{r,0..n_r-1}; a query set holds n_qvec >= 1 vectors q_0..q_{n_qvec-1}:
 *   pair(i, j) = mi355_flat_search's cosine distance of q_i against x_{r,j} (d-ascending fmaf chains of
 *                q.x and x.x over the widened elements, qq the chain of q_i.q_i,
 *                1 - qv / (sqrt(qq) * sqrt(vv)) with IEEE divide / sqrt)
 *   m_i(r)     = fminf over j of pair(i, j)           (NaN ignored unless every pair is NaN)
 *   dist(r)    = ((m_0 + m_1) + m_2) + ...           (plain f32 adds, i ascending)
 * i.e. n_qvec - sum of MaxSim.  Per query set the k smallest rows by (dist, rowid); a row whose dist is
 * NaN, a row without vectors (a null row included) is never returned; [lower, upper) and the prefilter
 * apply to dist.  refine_factor, the nprobe fields and approx_mode are ignored (the result is exact).
 * Cosine only (lance: "only cosine similarity is supported for multi-vectors"): metric DEFAULT means
 * cosine, L2 / DOT are NotSupported.
 * PARITY: pinned to the reference's additivity test (querying with [q, q] returns exactly twice the
 * distances of [q], in the same row order: python/python/tests/test_query.py:790-820) and to this
 * repository's restatement of the formula above.  lance's own multivector arithmetic is [EXT] and not
 * vendored; no bit-exact claim against it is made.
 */
typedef struct mi355_multivec mi355_multivec; /* multivector column resident on one GPU */

/* the largest query set (vectors per query) mi355_multivec_search takes (ColPali: 1024 patches) */
#define MI355_MULTIVEC_MAX_QVEC 1024u

typedef struct mi355_multivec_desc {
  uint32_t struct_size;       /* sizeof(mi355_multivec_desc) */
  uint32_t dim;
  uint64_t n_rows;
  uint64_t n_vectors;         /* offsets[n_rows] */
  uint32_t dtype;             /* MI355_DTYPE_F32 / BF16 / F16 */
  uint32_t mem;               /* MI355_MEM_HOST: copied to HBM at open; DEVICE: scanned in place (the caller keeps
                                 vectors alive until close; offsets / row_ids are copied) */
  const void *vectors;        /* [n_vectors, dim], the rows' vectors back to back */
  const uint64_t *offsets;    /* [n_rows + 1], offsets[0] = 0, non-decreasing (Arrow list offsets) */
  const uint64_t *row_ids;    /* [n_rows] or NULL = identity */
  uint32_t metric;            /* MI355_METRIC_COSINE or MI355_METRIC_DEFAULT */
  int32_t device;
} mi355_multivec_desc;

/* Checks that run before any device is touched: dim 0, NULL vectors (n_vectors > 0) or offsets, host offsets
   that do not start at 0, decrease or do not end at n_vectors, an unknown dtype / mem, a metric other than
   cosine / default, n_rows or n_vectors >= 2^32 - 16.  Device offsets are checked after they are read back. */
int32_t mi355_multivec_open(const mi355_multivec_desc *desc, mi355_multivec **out);
int32_t mi355_multivec_close(mi355_multivec *mv);
int32_t mi355_multivec_set_stream(mi355_multivec *mv, void *hip_stream);
int32_t mi355_multivec_sync(mi355_multivec *mv);
/* rows and stored vectors of the handle */
int32_t mi355_multivec_info(const mi355_multivec *mv, uint64_t *out_rows, uint64_t *out_vectors);
/* Replaces KNNVectorDistance over a multivector column + SortExec TopK.  `queries` is a batch of n_queries
   query sets of n_qvec vectors each ([n_queries, n_qvec, dim] f32); n_qvec is 1 .. MI355_MULTIVEC_MAX_QVEC
   (checked, with the metric, before the handle).  Outputs, host / device I/O, k (any k), the prefilter and
   timeout_ms follow mi355_flat_search: out_rowids / out_dist are [n_queries, k], out_counts [n_queries]. */
int32_t mi355_multivec_search(mi355_multivec *mv, const float *queries, uint32_t n_queries,
                              uint32_t n_qvec, const mi355_search_params *params,
                              uint64_t *out_rowids, float *out_dist, uint32_t *out_counts);

#ifdef __cplusplus
}
#endif
#endif /* MI355_MULTIVEC_H */
