// Included by isp_tile_p{0..3}.hip with PAT_PR, PAT_PC and PAT_FN defined: instantiates the tile
// kernels of one CFA pattern (both work types, all epilogues) and their launcher.
#include "isp_tile.h"
#include "isp_resize_tile.h"

namespace tile {

template <class E>
static int launch_e(const Params& p, int epi, hipStream_t s) {
  const dim3 grid(num_tiles(p.H, p.W)), block(THREADS);
  if (p.levels) {                  // a packed source with sensor levels (mi_isp_load_packed_levels): the general fill
    if (epi != EPI_STORE) { mi_set_error("tile: sensor levels take the store epilogue only"); return 1; }
    if (p.shading) hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE, 0, true, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE, 0, true>), grid, block, 0, s, p);
    MI_LAUNCH_CHECK();
    return 0;
  }
  switch (hot_spec(p, dtype_code<E>(), epi)) {
    case 1:
      if (epi == EPI_STORE) hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE, 1>), grid, block, 0, s, p);
      else hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE_MINMAX, 1>), grid, block, 0, s, p);
      MI_LAUNCH_CHECK();
      return 0;
    case 2:
      hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE, 2>), grid, block, 0, s, p);
      MI_LAUNCH_CHECK();
      return 0;
    case 3:
      hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE, 3>), grid, block, 0, s, p);
      MI_LAUNCH_CHECK();
      return 0;
    default: break;
  }
  switch (epi) {
    case EPI_STORE: hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE>), grid, block, 0, s, p); break;
    case EPI_MINMAX: hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_MINMAX>), grid, block, 0, s, p); break;
    case EPI_STATS: hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STATS>), grid, block, 0, s, p); break;
    case EPI_RH_MINMAX: hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_RH_MINMAX>), grid, block, 0, s, p); break;
    case EPI_RH_STORE: hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_RH_STORE>), grid, block, 0, s, p); break;
    case EPI_STORE_MINMAX: hipLaunchKernelGGL((tile_kernel<E, PAT_PR, PAT_PC, EPI_STORE_MINMAX>), grid, block, 0, s, p); break;
    default: mi_set_error("tile: bad epilogue %d", epi); return 1;
  }
  MI_LAUNCH_CHECK();
  return 0;
}

#if PAT_PR == 0 && PAT_PC == 0
// measurement aid: blocks per CU the runtime admits for the f16 RGGB kernels
int occupancy_rggb(int epi) {
  int n = -1;
  hipError_t e;
  switch (epi) {
    case EPI_MINMAX: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tile_kernel<half_t, 0, 0, EPI_MINMAX>, THREADS, 0); break;
    case EPI_STATS: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tile_kernel<half_t, 0, 0, EPI_STATS>, THREADS, 0); break;
    case EPI_RH_MINMAX: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tile_kernel<half_t, 0, 0, EPI_RH_MINMAX>, THREADS, 0); break;
    case EPI_RH_STORE: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tile_kernel<half_t, 0, 0, EPI_RH_STORE>, THREADS, 0); break;
    default: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tile_kernel<half_t, 0, 0, EPI_STORE>, THREADS, 0); break;
  }
  return e == hipSuccess ? n : -1;
}
#endif

int PAT_FN(const Params& p, int work_dtype, int epi, hipStream_t s) {
  return work_dtype == MI_F16 ? launch_e<half_t>(p, epi, s) : launch_e<float>(p, epi, s);
}

}  // namespace tile

#define MI_CAT2(a, b) a##b
#define MI_CAT(a, b) MI_CAT2(a, b)
namespace rtile {
int PAT_FN(const RParams& p, int work_dtype, hipStream_t s) {
  const dim3 grid(num_tiles(p.Hd, p.Wd)), block(THREADS);
  if (p.t.shading) {                 // lens shading (with the per-site levels decode): the general fill
    if (work_dtype == MI_F16) hipLaunchKernelGGL((resize_tile_kernel<half_t, PAT_PR, PAT_PC, false, true, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((resize_tile_kernel<float, PAT_PR, PAT_PC, false, true, true>), grid, block, 0, s, p);
  } else if (p.t.levels) {
    if (work_dtype == MI_F16) hipLaunchKernelGGL((resize_tile_kernel<half_t, PAT_PR, PAT_PC, false, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((resize_tile_kernel<float, PAT_PR, PAT_PC, false, true>), grid, block, 0, s, p);
  } else if (hot_ok(p)) {
    if (work_dtype == MI_F16) hipLaunchKernelGGL((resize_tile_kernel<half_t, PAT_PR, PAT_PC, true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((resize_tile_kernel<float, PAT_PR, PAT_PC, true>), grid, block, 0, s, p);
  } else {
    if (work_dtype == MI_F16) hipLaunchKernelGGL((resize_tile_kernel<half_t, PAT_PR, PAT_PC, false>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((resize_tile_kernel<float, PAT_PR, PAT_PC, false>), grid, block, 0, s, p);
  }
  MI_LAUNCH_CHECK();
  return 0;
}
}  // namespace rtile
