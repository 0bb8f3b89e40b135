// 3D colour LUT (mi_isp_color_lut; DESIGN.md 3, "Colour LUT"): tetrahedral interpolation in an N x N x N table of packed RGB
// dwords on an interleaved u8 RGB image (H x W x 3), stated in integer arithmetic, so the kernel's output is the contract's
// bit for bit.  The operator is pointwise: src == dst is allowed.  One launch takes up to u8::MAX_IMAGES images of one
// geometry, their pointers in the kernel arguments.
//
// Per pixel, v_c the input codes (c = R, G, B), T the table (entry (r * N + g) * N + b = R | G << 8 | B << 16), S = strength_q6:
//   p_c = v_c (N - 1);  i_c = p_c // 255;  f_c = p_c - 255 i_c;  j_c = min(i_c + 1, N - 1)
//   a, b, d = the axes ordered so that f_a >= f_b >= f_d (ties: either order, the corner that differs has weight 0)
//   C0 = T[i];  C1 = C0's index with axis a at j_a;  C2 = C1's with axis b at j_b;  C3 = T[j]
//   y_c = (C0_c (255 - f_a) + C1_c (f_a - f_b) + C2_c (f_b - f_d) + C3_c f_d + 127) // 255
//   out_c = v_c + (((y_c - v_c) S + 32) >> 6)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "isp_u8_stage.h"
#define CLUT_HD __host__ __device__ inline
#else
#define CLUT_HD inline
#endif

namespace clut {

// a * b for a, b < 2^24 whose product fits 32 bits: on the device the full-rate 24-bit multiply (v_mul_u32_u24; a 32-bit
// v_mul_lo_u32 runs at a quarter of the rate, and the kernel is bound by its VALU instructions)
CLUT_HD uint32_t mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, b);
#else
  return a * b;
#endif
}

// x // 255 for 0 <= x <= 65025 + 127 (the largest numerator of y_c; p_c <= 255 * 64 lies inside).  Compiles for the host as
// well: tests/check_color_lut_div.cpp compares it with the division over the whole range.
CLUT_HD uint32_t div255(uint32_t x) { return mul24(x, 0x8081u) >> 23; }

constexpr int MIN_POINTS = 2, MAX_POINTS = 65;      // N
constexpr int LDS_POINTS_SMALL = 17;                // the small LDS instance holds N <= 17: 4913 dwords, 19 652 bytes
constexpr int LDS_POINTS = 33;                      // the large one N <= 33: 35 937 dwords, 143 748 bytes of a CU's 160 KiB
constexpr int PIXELS_PER_THREAD = 4;                // 4 pixels = 3 dwords on the dword path
constexpr int LDS_THREADS = 1024;                   // the LDS instances: 16 waves, one block per CU at N = 33, two at N <= 17
constexpr int GLOBAL_THREADS = 256;
constexpr int LDS_CHUNK = LDS_THREADS * PIXELS_PER_THREAD;          // pixels a block takes per trip of its chunk loop: 4096
constexpr int GLOBAL_CHUNK = GLOBAL_THREADS * PIXELS_PER_THREAD;    // 1024

enum Path { PATH_AUTO = 0, PATH_LDS = 1, PATH_GLOBAL = 2 };

// The dispatcher (measured): true when the launch keeps the table in LDS.  Every block of an LDS launch reads
// the whole table out of L2 before its first pixel; on six 3072 x 4096 and on six 1440 x 1920 images that is paid back at
// N = 17 and at N = 33, on a natural scene and on random bytes, so the rule is the table's size alone.
CLUT_HD bool lds_wins(int n_points) { return n_points <= LDS_POINTS; }

}  // namespace clut

#if defined(__HIPCC__)
namespace clut {

struct Args {
  uint32_t pixels;                                  // H * W of one image (< 2^31)
  int dword_rows;                                   // W * 3 % 4 == 0: with 4-byte aligned images, the dword path
  int n_points;                                     // N
  int strength_q6;                                  // S = floor(strength * 64 + 0.5), 0 .. 64
  int n_images;
  const uint32_t* table;                            // N^3 dwords on the device
  u8::Image im[u8::MAX_IMAGES];
};
static_assert(sizeof(Args) == 544 && offsetof(Args, im) == 32, "the kernel arguments' layout");

// one launch (a.n_images images) on `path` (PATH_LDS needs N <= LDS_POINTS); n_cus: the device's CU count
int launch(const Args& a, Path path, int n_cus, hipStream_t stream);

}  // namespace clut
#endif
