// The plane copy of the u8 output filters' YUV 4:2:0 forms (isp_u8_stage.h).
#include "isp_u8_stage.h"

namespace u8 {

struct CopyArgs {
  Image im[MAX_IMAGES];
};

// bytes [first, first + count) of every image, as they are; grid (blocks, n)
__global__ void __launch_bounds__(THREADS) copy_bytes_kernel(const CopyArgs a, size_t first, size_t count) {
  const Image im = a.im[blockIdx.y];
  const uint8_t* s = im.src + first;
  uint8_t* d = im.dst + first;
  const size_t i0 = (size_t)blockIdx.x * THREADS + threadIdx.x, step = (size_t)gridDim.x * THREADS;
  if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d) | count) & 15) == 0) {
    for (size_t i = i0; i < count / 16; i += step) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
  } else {
    for (size_t i = i0; i < count; i += step) d[i] = s[i];
  }
}

int launch_copy(const Image* im, int n, size_t first, size_t count, hipStream_t stream) {
  if (n <= 0 || count == 0) return 0;
  CopyArgs a = {};
  for (int i = 0; i < n; ++i) a.im[i] = im[i];
  const size_t blocks = (count / 16 + THREADS - 1) / THREADS;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks)), (unsigned)n);
  hipLaunchKernelGGL(copy_bytes_kernel, grid, dim3(THREADS), 0, stream, a, first, count);
  MI_LAUNCH_CHECK();
  return 0;
}

}  // namespace u8
