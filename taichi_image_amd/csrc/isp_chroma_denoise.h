// Chroma noise reduction (mi_isp_chroma_denoise; DESIGN.md 3, "Chroma noise reduction"): a luma-guided mean of the chroma
// on the grid of 2 x 2 pixel cells of a u8 image, interleaved RGB (H x W x 3) or planar YUV 4:2:0 (the U and V planes are
// that grid).  The filter is stated in integer arithmetic, so the kernel's output is the contract's bit for bit.  One
// launch takes up to u8::MAX_IMAGES images of one geometry, their pointers in the kernel arguments.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CDN_HD __host__ __device__ inline
#else
#define CDN_HD inline
#endif

namespace cdn {

// floor(num / (512 n)) for 1 <= n <= 49 and |num| <= 2^24 + 256 * 49 (the contract's db and dr).  Compiles for the host as
// well: tests/check_chroma_denoise_div.cpp compares it with floor division for every such num and n.
//   m = num >> 9 = floor(num / 512), and floor(floor(x / a) / b) = floor(x / (a b)) for positive a, b.
//   |m| <= 2^15 + 25 and n are exact in f32.  t = RN(m RN(1 / n)) is within |m / n| 2^-22 < 2^-7 of m / n, and a quotient
//   that is no integer is at least 1 / 49 > 2^-7 away from one, so trunc(t) is floor(m / n), or one above it (m < 0), or
//   one below it (an integral quotient whose t fell short): one step either way on the remainder settles it.
CDN_HD int floor_div_512n(int num, int n) {
  const int m = num >> 9;
  int q = (int)((float)m * (1.0f / (float)n));
  int rem = m - q * n;
  if (rem < 0) { q -= 1; rem += n; }
  if (rem >= n) q += 1;
  return q;
}

// dg of the contract: keeps 77 dr + 150 dg + 29 db near 0 (437 / 65536 ~ 1 / 150)
CDN_HD int green_delta(int dr, int db) { return ((-(77 * dr + 29 * db)) * 437 + 32768) >> 16; }

}  // namespace cdn

#if defined(__HIPCC__)
#include "isp_u8_stage.h"

namespace cdn {

constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_CW = 64;                 // tile, in cells: 32 pairs of cells (one pair = 4 pixels per lane of a half wave) ...
constexpr int TILE_CH = 32;                 // ... by 8 strips of ROWS cell rows: 128 x 64 pixels
constexpr int ROWS = 4;                     // cell rows per thread, one below the other

struct Args {
  int H, W;                                 // of the RGB image, or of the Y plane
  int tl4, tc4;                             // 4 luma_threshold, 4 chroma_threshold
  int strength_q6;                          // S = floor(strength * 64 + 0.5), 0 .. 64
  int n_images;
  u8::Image im[u8::MAX_IMAGES];
};
static_assert(sizeof(Args) == 536 && offsetof(Args, im) == 24, "the kernel arguments' layout");

// one launch (a.n_images images): rgb (interleaved, 3 bytes per pixel) or planar YUV 4:2:0 (only U and V are written: the Y
// rows are the caller's to copy), radius 1, 2 or 3
int launch(const Args& a, bool rgb, int radius, hipStream_t stream);

}  // namespace cdn
#endif
