// kernels_multivec.h — exact late-interaction (MaxSim) search over a multivector column (List<FixedSizeList>): the
// kernels behind mi355_multivec_search (include/mi355_ann.h, contract there).  Reference: the multivector query of
// rust/lancedb/src/table/query.rs:169-199 (N query vectors concatenated into ONE query) and
// python/python/tests/test_query.py:790-820.
//
//   k_multivec_norms   at open: vv[j] = the d-ascending fmaf chain of x_j . x_j (dist_step's vv chain)
//   k_multivec_prep    per call: qq of every query vector (the same chain)
//   k_multivec_scan    one workgroup per tile of whole rows: every (query vector, stored vector) dot product on
//                      v_mfma_f32_32x32x2_f32, the cosine epilogue, per-(query vector, row) minima, the i-ascending
//                      sum -> dist[query set][row]
//   k_multivec_select  k_flat_scan's selection over those row distances ([lower, upper), prefilter, WaveTopK) into
//                      the candidate slots k_merge_cands reduces
#pragma once
#include "kernels_ivfpq.h"

#define MV_QT 32     // query vectors per tile: one MFMA side
#define MV_VT 128    // stored vectors per chunk: 4 waves x 32
#define MV_K 32      // K staged per LDS round
#define MV_MAXR 128  // rows per tile (a tile is cut at row boundaries; a row of > MV_VT vectors is a tile of its own)

typedef __attribute__((ext_vector_type(16))) float mv_f32x16;
typedef __attribute__((ext_vector_type(4))) float mv_f32x4;

// the d-ascending fmaf chain of v . v over the widened elements of one stored vector (= dist_step's vv chain)
static __global__ __launch_bounds__(256) void k_multivec_norms(const void* __restrict__ vectors, uint32_t dtype,
                                                               uint64_t n_vectors, uint32_t dim, float* __restrict__ vv) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_vectors) return;
  const uint64_t base = j * dim;
  float acc = 0.f;
  for (uint32_t d = 0; d < dim; ++d) {
    const float v = load_elem(vectors, dtype, base + d);
    acc = __fmaf_rn(v, v, acc);
  }
  vv[j] = acc;
}

// qq of every query vector of the call (the chain k_flat_scan computes for its query)
static __global__ __launch_bounds__(256) void k_multivec_prep(const float* __restrict__ q, uint64_t n, uint32_t dim,
                                                              float* __restrict__ qq) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = q + i * dim;
  float acc = 0.f;
  for (uint32_t d = 0; d < dim; ++d) acc = __fmaf_rn(p[d], p[d], acc);
  qq[i] = acc;
}

struct MultivecScanArgs {
  const void* vectors;        // [n_vectors, dim] per dtype
  uint32_t dtype, dim;
  const float* vv;            // [n_vectors]
  const uint64_t* offsets;    // [n_rows + 1]
  const uint64_t* tile_row0;  // [n_tiles + 1] first row of every tile
  const float* q;             // [nb, n_qvec, dim]
  const float* qq;            // [nb, n_qvec]
  uint32_t nb, n_qvec;
  uint64_t n_rows;
  float* dist;                // [nb, n_rows]
};

// One workgroup per tile of whole rows (<= MV_MAXR rows, <= MV_VT vectors, or one longer row), walking every query set
// of the batch, so the tile is read from HBM once and from the caches after that.  Per query set the query vectors are
// taken 32 at a time (ascending) and the tile's vectors 128 at a time: each wave computes one 32 x 32 block of q . x on
// v_mfma_f32_32x32x2_f32, which chains two fmas per step into ONE accumulator that starts at +0 and runs K ascending —
// the contract's d-ascending fmaf chain, bit for bit (as k_coarse_mfma; no split-K).  K is staged 32 at a time through
// LDS, widened to f32 (exact) and zero-padded past dim and past the last vector / query vector.  Epilogue: the cosine
// of dist_finish (IEEE divide / sqrt), fminf into per-(query vector, row) minima in LDS across chunks, and after each
// query tile the i-ascending f32 sum of its minima into the per-row distance.  A row without vectors keeps NaN.
static __global__ __launch_bounds__(256) void k_multivec_scan(MultivecScanArgs a) {
  __shared__ float sa[MV_QT][MV_K + 1];     // query tile, one K round (rows padded: conflict-free column reads)
  __shared__ float sb[MV_VT][MV_K + 1];     // stored vectors, one K round
  __shared__ float spair[MV_QT][MV_VT + 1]; // pair distances of the chunk
  __shared__ float smin[MV_MAXR][MV_QT + 1];// running minima per (row, query vector)
  __shared__ float ssum[MV_MAXR];
  __shared__ float sqq[MV_QT];
  __shared__ uint32_t soff[MV_MAXR + 1];    // the tile's row offsets, relative to its first vector
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int fi = lane & 31, fk = lane >> 5;
  const uint64_t r0 = a.tile_row0[blockIdx.x];
  const uint32_t nr = (uint32_t)(a.tile_row0[blockIdx.x + 1] - r0);
  const uint64_t vbase = a.offsets[r0];
  for (uint32_t r = tid; r <= nr; r += 256) soff[r] = (uint32_t)(a.offsets[r0 + r] - vbase);
  __syncthreads();
  const uint32_t nv = soff[nr];
  const uint32_t dim = a.dim;
  for (uint32_t b = 0; b < a.nb; ++b) {
    const float* qb = a.q + (size_t)b * a.n_qvec * dim;
    for (uint32_t qt0 = 0; qt0 < a.n_qvec; qt0 += MV_QT) {
      const uint32_t nqt = min((uint32_t)MV_QT, a.n_qvec - qt0);
      for (uint32_t e = tid; e < nr * MV_QT; e += 256) smin[e >> 5][e & 31] = __builtin_nanf("");
      if (tid < MV_QT) sqq[tid] = (uint32_t)tid < nqt ? a.qq[(size_t)b * a.n_qvec + qt0 + tid] : 0.f;
      __syncthreads();
      for (uint32_t c0 = 0; c0 < nv; c0 += MV_VT) {
        const uint32_t ncv = min((uint32_t)MV_VT, nv - c0);
        mv_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        // staging: the query tile is 32 x 32 elements (4 per thread), the chunk 128 x 32 (16 per thread); the next
        // round's loads are issued before this round's MFMAs (register prefetch)
        mv_f32x4 ra;
        mv_f32x16 rb;
        auto fetch = [&](uint32_t k0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t idx = tid + e * 256, r = idx >> 5, k = k0 + (idx & 31);
            ra[e] = (r < nqt && k < dim) ? qb[(size_t)(qt0 + r) * dim + k] : 0.f;
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const uint32_t idx = tid + e * 256, r = idx >> 5, k = k0 + (idx & 31);
            rb[e] = (r < ncv && k < dim) ? load_elem(a.vectors, a.dtype, (vbase + c0 + r) * dim + k) : 0.f;
          }
        };
        auto stash = [&]() {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t idx = tid + e * 256;
            sa[idx >> 5][idx & 31] = ra[e];
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const uint32_t idx = tid + e * 256;
            sb[idx >> 5][idx & 31] = rb[e];
          }
        };
        fetch(0);
        for (uint32_t k0 = 0; k0 < dim; k0 += MV_K) {
          stash();
          __syncthreads();
          if (k0 + MV_K < dim) fetch(k0 + MV_K);
          // K steps of 2 up to dim rounded up to even (the zero padding of an odd dim adds fma(0, 0, acc) = acc)
          const uint32_t kn = min((uint32_t)MV_K, ((dim + 1u) & ~1u) - k0);
          if (kn == MV_K) {
#pragma unroll
            for (int kk = 0; kk < MV_K; kk += 2)
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[fi][kk + fk], sb[wid * 32 + fi][kk + fk], acc, 0, 0, 0);
          } else {
            for (uint32_t kk = 0; kk < kn; kk += 2)
              acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[fi][kk + fk], sb[wid * 32 + fi][kk + fk], acc, 0, 0, 0);
          }
          __syncthreads();
        }
        // D: col = lane & 31 (stored vector j of this wave's 32), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        const uint32_t j = wid * 32 + fi;
        const float svv = ieee_sqrtf(j < ncv ? a.vv[vbase + c0 + j] : 0.f);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const uint32_t i = (reg & 3) + 8 * (reg >> 2) + 4 * fk;
          spair[i][j] = 1.0f - ieee_divf(acc[reg], ieee_sqrtf(sqq[i]) * svv);
        }
        __syncthreads();
        // fminf over each row's vectors inside this chunk, folded into the running minimum (order-free: no pair is -0)
        for (uint32_t e = tid; e < nr * MV_QT; e += 256) {
          const uint32_t i = e & 31, r = e >> 5;
          if (i >= nqt) continue;
          const uint32_t j0 = max(soff[r], c0), j1 = min(soff[r + 1], c0 + ncv);
          float m = smin[r][i];
          for (uint32_t jj = j0; jj < j1; ++jj) m = fminf(m, spair[i][jj - c0]);
          smin[r][i] = m;
        }
        __syncthreads();
      }
      // dist(r) = ((m_0 + m_1) + m_2) + ...: this tile's minima, i ascending, after those of the tiles before
      for (uint32_t r = tid; r < nr; r += 256) {
        float s = qt0 == 0 ? smin[r][0] : ssum[r] + smin[r][0];
        for (uint32_t i = 1; i < nqt; ++i) s = s + smin[r][i];
        ssum[r] = s;
      }
      __syncthreads();
    }
    for (uint32_t r = tid; r < nr; r += 256) a.dist[(size_t)b * a.n_rows + r0 + r] = ssum[r];
    __syncthreads();
  }
}

struct MultivecSelectArgs {
  const float* dist;        // [nq, n_rows]
  const uint64_t* row_ids;  // or nullptr
  uint64_t n_rows;
  uint32_t slice_rows, n_slices, kk;
  RangeFilter range;
  RowFilter filter;
  Cand* cand;               // [nq, n_slices, kk]
};

// k_flat_scan's selection with the row distance read instead of computed: one workgroup per (slice, query set), one
// row per thread, a WaveTopK per wave, the four lists reduced by wave 0; kk > 64 * KPL in passes above a floor.
template <int KPL>
__global__ __launch_bounds__(256) void k_multivec_select(MultivecSelectArgs a) {
  __shared__ Cand stage[3 * KPL * MI355_WAVE];
  __shared__ PassFloor s_floor;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t s = blockIdx.x, b = blockIdx.z;
  const float* dist = a.dist + (size_t)b * a.n_rows;
  const uint64_t v0 = (uint64_t)s * a.slice_rows;
  const uint64_t v1 = min(a.n_rows, v0 + (uint64_t)a.slice_rows);
  Cand* out = a.cand + ((size_t)b * a.n_slices + s) * a.kk;
  constexpr uint32_t C = KPL * MI355_WAVE;
  bool fl_on = false;
  float fl_d = 0.f;
  uint64_t fl_id = 0;
  for (uint32_t base = 0; base < a.kk; base += C) {
    const uint32_t c = min(a.kk - base, C);
    WaveTopK<KPL> top;
    top.init(c, lane);
    top.set_floor(fl_on, fl_d, (uint32_t)fl_id, (uint32_t)(fl_id >> 32));
    for (uint64_t i0 = v0; i0 < v1; i0 += 256) {
      const uint64_t i = i0 + tid;
      bool ok = i < v1;
      float d = 0.f;
      if (ok) {
        d = dist[i];
        ok = d <= top.thr_d && in_range(d, a.range);
      }
      if (__any(ok)) {
        uint64_t id = 0;
        if (ok) id = a.row_ids ? a.row_ids[i] : i;
        if (a.filter.mode != MI355_FILTER_NONE && ok) ok = row_permitted(id, a.filter);
        top.offer(ok, d, (uint32_t)i, id, lane);
      }
    }
    if (wid > 0) top.store(stage + (size_t)(wid - 1) * c, lane);
    __syncthreads();
    if (wid == 0) {
      const uint32_t n = 3 * c;
      for (uint32_t t0 = 0; t0 < n; t0 += MI355_WAVE) {
        const uint32_t t = t0 + lane;
        Cand cd;
        cd.d = 0.f;
        cd.pos = CAND_EMPTY_POS;
        cd.id = 0;
        if (t < n) cd = stage[t];
        top.offer(t < n && cd.pos != CAND_EMPTY_POS, cd.d, cd.pos, cd.id, lane);
      }
      top.store(out + base, lane);
      // the slice's pass is full iff its worst kept slot is a real row: the next pass starts above it
      const bool full = !(top.thr_d == __builtin_huge_valf() && top.thr_lo == 0xFFFFFFFFu && top.thr_hi == 0xFFFFFFFFu);
      if (lane == 0) {
        s_floor.on = full ? 1u : 0u;
        s_floor.d = top.thr_d;
        s_floor.id = ((uint64_t)top.thr_hi << 32) | top.thr_lo;
      }
    }
    __syncthreads();
    if (!s_floor.on) {  // fewer rows than asked for: the remaining slots are empty
      for (uint32_t g = base + c + tid; g < a.kk; g += 256) {
        Cand e;
        e.d = __builtin_huge_valf();
        e.pos = CAND_EMPTY_POS;
        e.id = ~0ull;
        out[g] = e;
      }
      break;
    }
    fl_on = true;
    fl_d = s_floor.d;
    fl_id = s_floor.id;
    __syncthreads();  // stage is rewritten by the next pass
  }
}
