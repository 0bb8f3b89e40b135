// Included by isp_stream_p{0..3}.hip with PAT_PR, PAT_PC and PAT_FN defined: instantiates the stream
// kernels of one CFA pattern (both work types, all epilogues) and their launcher.
#include "isp_stream.h"
#include "isp_stream_resize.h"

namespace strm {

template <class E>
static int launch_e(const SArgs& a, int epi, hipStream_t s) {
  const dim3 grid(a.n_blocks, epi == S_STORE && a.n_batch > 0 ? a.n_batch : 1), block(THREADS);
  if (a.t.levels) {                                // sensor levels (mi_isp_load_packed_levels): the load's store pass only
    if (epi != S_STORE) { mi_set_error("stream: sensor levels take the store pass only"); return 1; }
    if (a.t.shading) hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_STORE, 3>), grid, block, 0, s, a);
    else if (a.t.levels == 1) hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_STORE, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_STORE, 2>), grid, block, 0, s, a);
    MI_LAUNCH_CHECK();
    return 0;
  }
  switch (epi) {
    case S_STORE: hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_STORE>), grid, block, 0, s, a); break;
    case S_BOUNDS: hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_BOUNDS>), grid, block, 0, s, a); break;
    case S_STATS: hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_STATS>), grid, block, 0, s, a); break;
    case S_RH_MINMAX: hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_RH_MINMAX>), grid, block, 0, s, a); break;
    case S_RH_STORE: hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_RH_STORE>), grid, block, 0, s, a); break;
    case S_STORE_BOUNDS: hipLaunchKernelGGL((stream_kernel<E, PAT_PR, PAT_PC, S_STORE_BOUNDS>), grid, block, 0, s, a); break;
    default: mi_set_error("stream: bad epilogue %d", epi); return 1;
  }
  MI_LAUNCH_CHECK();
  return 0;
}

int PAT_FN(const SArgs& a, int work_dtype, int epi, hipStream_t s) {
  return work_dtype == MI_F16 ? launch_e<half_t>(a, epi, s) : launch_e<float>(a, epi, s);
}

int PAT_SUB_FN(const SubArgs& a, int work_dtype, hipStream_t s) {
  const dim3 grid(a.n_blocks, a.n_batch), block(THREADS);
  if (a.t.levels == 1) {
    if (work_dtype == MI_F16) hipLaunchKernelGGL((sub_kernel<half_t, PAT_PR, PAT_PC, 1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sub_kernel<float, PAT_PR, PAT_PC, 1>), grid, block, 0, s, a);
  } else if (a.t.levels == 2) {
    if (work_dtype == MI_F16) hipLaunchKernelGGL((sub_kernel<half_t, PAT_PR, PAT_PC, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sub_kernel<float, PAT_PR, PAT_PC, 2>), grid, block, 0, s, a);
  } else if (work_dtype == MI_F16) {
    hipLaunchKernelGGL((sub_kernel<half_t, PAT_PR, PAT_PC>), grid, block, 0, s, a);
  } else {
    hipLaunchKernelGGL((sub_kernel<float, PAT_PR, PAT_PC>), grid, block, 0, s, a);
  }
  MI_LAUNCH_CHECK();
  return 0;
}

}  // namespace strm

namespace rstrm {
int PAT_FN(const RSArgs& a, hipStream_t s) {
  const dim3 grid(a.n_blocks, a.n_batch > 0 ? a.n_batch : 1);
  // sensor levels: 1 in the decode table, 2 per site in registers; lens shading: 3 (per site, then the gain)
  switch (a.t.shading ? 3 : a.t.levels) {
    case 0: hipLaunchKernelGGL((resize_kernel<PAT_PR, PAT_PC>), grid, dim3(THREADS), 0, s, a); break;
    case 3: hipLaunchKernelGGL((resize_kernel<PAT_PR, PAT_PC, 3>), grid, dim3(THREADS), 0, s, a); break;
    case 1: hipLaunchKernelGGL((resize_kernel<PAT_PR, PAT_PC, 1>), grid, dim3(THREADS), 0, s, a); break;
    default: hipLaunchKernelGGL((resize_kernel<PAT_PR, PAT_PC, 2>), grid, dim3(THREADS), 0, s, a); break;
  }
  MI_LAUNCH_CHECK();
  return 0;
}
}  // namespace rstrm
