// Included by isp_cam_p{0..3}.hip with PAT_PR, PAT_PC, PAT_FN and PAT_OCC defined: the camera-group kernel of one CFA pattern.
#include "isp_mega_cam.h"

namespace mega {

int PAT_FN(const CBatch& cb, hipStream_t s) {
  switch (cb.m.s.t.levels) {                         // sensor levels: 1 in the decode table, 2 per site in registers
    case 0: hipLaunchKernelGGL((camera_kernel<PAT_PR, PAT_PC>), dim3(cb.m.s.n_blocks), dim3(THREADS), 0, s, cb); break;
    case 1: hipLaunchKernelGGL((camera_kernel<PAT_PR, PAT_PC, 1>), dim3(cb.m.s.n_blocks), dim3(THREADS), 0, s, cb); break;
    default: hipLaunchKernelGGL((camera_kernel<PAT_PR, PAT_PC, 2>), dim3(cb.m.s.n_blocks), dim3(THREADS), 0, s, cb); break;
  }
  MI_LAUNCH_CHECK();
  return 0;
}

// blocks of this pattern's kernel (levels instantiation lv) the runtime admits per CU (the grid barrier needs every
// block resident)
int PAT_OCC(int lv) {
  int n = 0;
  hipError_t e;
  switch (lv) {
    case 0: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, camera_kernel<PAT_PR, PAT_PC>, THREADS, 0); break;
    case 1: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, camera_kernel<PAT_PR, PAT_PC, 1>, THREADS, 0); break;
    default: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, camera_kernel<PAT_PR, PAT_PC, 2>, THREADS, 0); break;
  }
  return e == hipSuccess ? n : 0;
}

}  // namespace mega
