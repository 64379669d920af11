// kernels_ivf_flat.h — the scan of an IVF_FLAT handle (MI355_INDEX_IVF_FLAT): exact distances over the RAW rows of
// every probed partition.  Reference: Index::IvfFlat (rust/lancedb/src/index.rs:80, index/vector.rs:170-210), lowered
// to lance's VectorIndexParams::with_ivf_flat_params (table/create_index.rs:252-262).
//
// Everything around it is the IVF-PQ pipeline (coarse stage, probe selection, maximum_nprobes second pass, merge):
// this kernel takes the place of the distance tables and the ADC scan and writes the same Cand slots
// ([query][probe][slice][kk]) that k_merge_cands reduces.
#pragma once
#include "kernels_ivfpq.h"

struct IvfFlatArgs {
  IndexView ix;             // raw = the handle's column in local row order, raw_dtype its element type
  const float* q;           // [nq, dim] the CALLER's queries (cosine is not normalised first: flat search's distance)
  const uint32_t* probes;   // [nq, nprobe]
  uint32_t nprobe;
  uint32_t slice_rows;      // rows per work item (multiple of 256)
  uint32_t n_slices;        // work items per (query, probe): grid.x = nprobe * n_slices
  uint32_t kk;
  RangeFilter range;
  RowFilter filter;
  Cand* cand;               // [nq, nprobe, n_slices, kk]
  DevCtl* ctl;              // deadline of the call
  ActiveMask act;           // device-side batch size (second pass of maximum_nprobes)
};

// LDS of one work item: the query + the three other waves' lists of a pass
static inline size_t ivf_flat_lds(uint32_t dim, uint32_t kk) {
  const size_t c = kk < 256u ? kk : 256u;
  return (((size_t)dim * 4 + 15) & ~(size_t)15) + 3 * c * sizeof(Cand);
}

// One workgroup per (query, probed partition, slice); grid = (nprobe * n_slices, nq).  One row per thread: its
// distance is exact_distance — the very chain of mi355_flat_search's k_flat_scan (d-ascending fmaf, q.x / x.x chains
// for cosine, 16-B row pieces), so the bits are the flat search's.  Each wave keeps a WaveTopK whose running worst
// key rejects most rows with one compare; the four lists are reduced by wave 0.  kk > 64 * KPL: the slice is swept
// once per pass of 64 * KPL rows above the last row of the pass before (WaveTopK floor), as in k_flat_scan.
template <int KPL>
__global__ __launch_bounds__(256) void k_ivf_flat_scan(IvfFlatArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const IndexView& ix = a.ix;
  float* sq = (float*)smem;  // [dim]
  Cand* stage = (Cand*)(smem + (((size_t)ix.dim * 4 + 15) & ~(size_t)15));  // [3][min(kk, 64 KPL)]
  __shared__ float s_qq;
  __shared__ PassFloor s_floor;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t r = blockIdx.x / a.n_slices, s = blockIdx.x % a.n_slices, b = blockIdx.y;
  if (!a.act.on(b)) return;
  if (ctl_expired(a.ctl)) return;  // (a timed-out call's results are undefined)
  Cand* out = a.cand + (((size_t)b * a.nprobe + r) * a.n_slices + s) * a.kk;
  const uint32_t p = a.probes[(size_t)b * a.nprobe + r];
  const uint32_t len = p < ix.nlist ? ix.plen[p] : 0u;  // out-of-range probe ids (search_probes) are empty items
  const uint32_t v0 = s * a.slice_rows;
  if (v0 >= len) {
    for (uint32_t g = tid; g < a.kk; g += 256) {
      Cand c;
      c.d = __builtin_huge_valf();
      c.pos = CAND_EMPTY_POS;
      c.id = ~0ull;
      out[g] = c;
    }
    return;
  }
  const uint32_t v1 = min(len, v0 + a.slice_rows);
  const uint32_t lrow0 = ix.lrow0[p];
  const uint64_t grow0 = ix.grow0[p];
  const float* q = a.q + (size_t)b * ix.dim;
  for (uint32_t d = tid; d < ix.dim; d += 256) sq[d] = q[d];
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    for (uint32_t d = 0; d < ix.dim; ++d) acc = __fmaf_rn(sq[d], sq[d], acc);
    s_qq = acc;
  }
  __syncthreads();
  const float qq = s_qq;
  constexpr uint32_t C = KPL * MI355_WAVE;
  bool fl_on = false;
  float fl_d = 0.f;
  uint64_t fl_id = 0;
  for (uint32_t base = 0; base < a.kk; base += C) {
    const uint32_t c = min(a.kk - base, C);
    WaveTopK<KPL> top;
    top.init(c, lane);
    top.set_floor(fl_on, fl_d, (uint32_t)fl_id, (uint32_t)(fl_id >> 32));
    // (block-uniform trip count: the body uses wave collectives)
    for (uint32_t i0 = v0; i0 < v1; i0 += 256) {
      const uint32_t i = i0 + tid;
      bool ok = i < v1;
      float d = 0.f;
      const uint32_t pos = lrow0 + i;
      if (ok) {
        d = exact_distance(sq, ix.raw, ix.raw_dtype, pos, ix.dim, ix.metric, qq);
        ok = d <= top.thr_d && in_range(d, a.range);
      }
      if (__any(ok)) {
        uint64_t id = 0;
        if (ok) id = ix.row_ids ? ix.row_ids[pos] : grow0 + i;
        if (a.filter.mode != MI355_FILTER_NONE && ok) ok = row_permitted(id, a.filter);
        top.offer(ok, d, pos, id, lane);
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
      // the item's pass is full iff its worst kept slot is a real row: the next pass starts above it
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
