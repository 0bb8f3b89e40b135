// Luma noise reduction (mi_isp_luma_denoise; DESIGN.md 3, "Luma noise reduction"): an edge-preserving mean of the luma over
// a (2r + 1)^2 window of a u8 image, interleaved RGB (H x W x 3; the same delta is added to R, G and B) or the Y plane of a
// planar YUV 4:2:0 image.  The filter is stated in integer arithmetic, so the kernel's output is the contract's bit for bit.
// One launch takes up to u8::MAX_IMAGES images of one geometry, their pointers in the kernel arguments.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YDN_HD __host__ __device__ inline
#else
#define YDN_HD inline
#endif

namespace ydn {

// m of the contract, floor((2 s + n) / (2 n)): the mean of n lumas with sum s (1 <= n <= 49, 0 <= s <= 255 n), ties rounded
// up, given rcp within 4 ulp of 1 / n.  Compiles for the host as well: tests/check_luma_denoise_div.cpp compares it with
// integer division for every such n and s and for every rcp within 4 ulp of RN(1 / n), which covers the division of the
// host and the device's v_rcp_f32 (1 ulp).
//   (2 s + n) / (2 n) = (s + n / 2) / n.  x = s + n / 2 + 1 / 4 is exact in f32 (below 2^14, a multiple of 1 / 4), and x / n
//   = (2 s + n + 1 / 2) / (2 n) is no integer and at least 1 / (4 n) away from one.  RN(x rcp) is within a relative 2^-24
//   (RN(1 / n)) + 4 * 2^-23 (rcp) + 2^-24 (the product) < 2^-20 of x / n <= 256, so within 2^-12 < 1 / (4 * 49) of it: its
//   truncation is floor(x / n) = floor((2 s + n) / (2 n)).
YDN_HD int mean_ties_up_rcp(int s, int n, float rcp) { return (int)(((float)s + 0.5f * (float)n + 0.25f) * rcp); }

YDN_HD int mean_ties_up(int s, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float rcp = __builtin_amdgcn_rcpf((float)n);
#else
  const float rcp = 1.0f / (float)n;
#endif
  return mean_ties_up_rcp(s, n, rcp);
}

// T of the contract: the threshold of a pixel with luma L0, from t0 in the dark toward t1 in the bright (>>: floor)
YDN_HD int threshold_at(int t0, int t1, int L0) { return t0 + (((t1 - t0) * L0 + 128) >> 8); }

}  // namespace ydn

#if defined(__HIPCC__)
#include "isp_u8_stage.h"

namespace ydn {

constexpr int ROWS = 8;                     // output rows per thread, one below the other: 8 strips to a u8::TILE_H tile

struct Args {
  int H, W;                                 // of the RGB image, or of the Y plane
  int t0, t1;                               // threshold, threshold_bright: luma codes 0 .. 255
  int strength_q6;                          // S = floor(strength * 64 + 0.5), 0 .. 64
  int n_images;
  u8::Image im[u8::MAX_IMAGES];
};
static_assert(sizeof(Args) == 536 && offsetof(Args, im) == 24, "the kernel arguments' layout");

// one launch (a.n_images images): rgb (interleaved, 3 bytes per pixel) or a plane (1 byte per pixel), radius 1, 2 or 3
int launch(const Args& a, bool rgb, int radius, hipStream_t stream);

}  // namespace ydn
#endif
