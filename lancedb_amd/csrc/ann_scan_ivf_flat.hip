// ann_scan_ivf_flat.hip — launcher of the IVF_FLAT scan (kernels_ivf_flat.h: exact distances over the raw rows of
// every probed partition).  Its own translation unit so that the kernel families compile in parallel.
#include "ann_internal.h"
#include "kernels_ivf_flat.h"

int32_t launch_scan_ivf_flat(const IvfFlatArgs& a, uint32_t nq, hipStream_t st) {
  const uint64_t items = (uint64_t)a.nprobe * a.n_slices;
  if (items > 0x7FFFFFFFull || nq > 65535u)
    return fail(MI355_ERR_NOT_SUPPORTED, "%llu work items per query x %u queries exceed one IVF_FLAT scan launch",
                (unsigned long long)items, nq);
  const size_t lds = ivf_flat_lds(a.ix.dim, a.kk);
  if (lds > 160u * 1024) return fail(MI355_ERR_NOT_SUPPORTED, "IVF_FLAT scan work item needs %zu B of LDS (> 160 KiB)", lds);
  const int kpl = kpl_for(a.kk);
  const void* kern = kpl == 1 ? (const void*)k_ivf_flat_scan<1> : kpl == 2 ? (const void*)k_ivf_flat_scan<2> : (const void*)k_ivf_flat_scan<4>;
  if (lds > 48u * 1024) HIP_TRY(ensure_dyn_lds(kern, lds));
  launch_by_kpl(kpl, k_ivf_flat_scan<1>, k_ivf_flat_scan<2>, k_ivf_flat_scan<4>, dim3((uint32_t)items, nq), dim3(256), lds, st, a);
  HIP_TRY(hipGetLastError());
  return MI355_OK;
}
