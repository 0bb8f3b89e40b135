// What the filters on the u8 outputs share on the device (output sharpening shp, local contrast lc, chroma noise
// reduction cdn, luma noise reduction ydn, the colour LUT clut): the image pointers of a launch, the byte helpers, the dword
// path's predicate, the plane copy of the YUV 4:2:0 forms, and for the kernels that take one 256-thread block per 128 x 64
// pixels with four pixels of a row per thread the dword path (what the loaders' images take) of the luma staging of sharpening
// and luma noise reduction (stage_luma) and of the write-back of four pixels that take one delta each (store_delta4: those two
// and local contrast's apply kernel).
// Left alone: the byte path of that staging and of that write-back stays written out in each kernel.  As part of a shared
// inline function the compiler lays it out differently and makes the column tests of a thread's four pixels once in front of
// its rows, where the dword path executes them too; written out, every kernel is the code it was before the helpers existed.
// And, because they are different code: chroma noise reduction stages 2 x 2 cells and writes a delta per channel, local
// contrast's histogram kernel loads a tile's strip and not a surround, the colour LUT is pointwise.
#pragma once
#include "isp_common.h"

namespace u8 {

constexpr int MAX_IMAGES = 32;              // images per launch, their pointers in the kernel arguments
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 128;                 // output tile: 32 groups of 4 columns (one group per lane of a half wave) ...
constexpr int TILE_H = 64;                  // ... by 8 strips of 8 rows
constexpr int LG = TILE_W / 4 + 2;          // 4-pixel groups per staged luma row: the tile's and one on either side (r <= 4)

struct Image {
  const uint8_t* src;
  uint8_t* dst;
};

// ---- byte helpers ----------------------------------------------------------------------------------------------------
MI_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
MI_DEV int min3(int a, int b, int c) { return min(min(a, b), c); }
MI_DEV int max3(int a, int b, int c) { return max(max(a, b), c); }
MI_DEV uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_udot4(a, b, c, false); }

// the lumas of four RGB pixels held in three dwords (bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3), packed into one
// (each sum is below 2^16, so its luma is its byte 1: v_perm_b32 gathers them; selector bytes 0-3 pick from the second
// operand, 4-7 from the first, 0x0c gives zero)
MI_DEV uint32_t luma4(uint32_t d0, uint32_t d1, uint32_t d2) {
  const uint32_t s0 = dot4(d0, 0x001D964Du, 128u);
  const uint32_t s1 = dot4(d1, 0x00001D96u, dot4(d0, 0x4D000000u, 128u));
  const uint32_t s2 = dot4(d2, 0x0000001Du, dot4(d1, 0x964D0000u, 128u));
  const uint32_t s3 = dot4(d2, 0x1D964D00u, 128u);
  const uint32_t l01 = __builtin_amdgcn_perm(s1, s0, 0x0c0c0501u), l23 = __builtin_amdgcn_perm(s3, s2, 0x0c0c0501u);
  return l01 | (l23 << 16);
}

MI_DEV int byte_of(uint32_t d, int b) { return (int)((d >> (8 * b)) & 0xffu); }

typedef short short2_t __attribute__((ext_vector_type(2)));

// the low halves of two deltas as a pair (|delta| <= 2040 fits 16 bits)
MI_DEV short2_t pair(int lo, int hi) {
  return __builtin_bit_cast(short2_t, __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u));
}

// the four bytes of d plus (a.x, a.y, b.x, b.y), each saturated to a byte: two bytes widen to a 16-bit pair (v_perm_b32),
// one packed add, v_sat_pk_u8_i16 saturates and packs the pair again
MI_DEV uint32_t add_sat4(uint32_t d, short2_t a, short2_t b) {
  const short2_t lo = __builtin_bit_cast(short2_t, __builtin_amdgcn_perm(0u, d, 0x0c010c00u)) + a;
  const short2_t hi = __builtin_bit_cast(short2_t, __builtin_amdgcn_perm(0u, d, 0x0c030c02u)) + b;
  uint32_t r0, r1;
  asm("v_sat_pk_u8_i16 %0, %1" : "=v"(r0) : "v"(lo));
  asm("v_sat_pk_u8_i16 %0, %1" : "=v"(r1) : "v"(hi));
  return r0 | (r1 << 16);
}

// ---- four pixels of a row per thread ---------------------------------------------------------------------------------
// the dword path: every 4-pixel group of a row is then wholly inside the image or wholly outside, and its bytes are aligned
MI_DEV bool rows_are_dwords(const Image& im, int W) {
  return (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(im.src) | reinterpret_cast<uintptr_t>(im.dst)) & 3) == 0;
}

// The dword path of the luma staging: the luma of the TILE_W x TILE_H tile at (r0, c0) and of four columns and R rows around
// it into lum, four pixels to a dword, coordinates clamped into the image: row lr = image row r0 - R + lr, dword lg = columns
// c0 - 4 + 4 lg ..  Every load of the thread is issued before the first is used (the staging waits for memory, not for
// arithmetic): a group outside the image loads the edge group of its row, and with REPEAT_EDGE it repeats that group's edge
// pixel (without: the group is staged as loaded - for a filter that never takes such a pixel as a tap).  The caller's barrier
// follows.
template <bool RGB, int R, bool REPEAT_EDGE>
MI_DEV void stage_luma(uint32_t (&lum)[(TILE_H + 2 * R) * LG], const Image& im, int H, int W, int r0, int c0) {
  constexpr int CH = RGB ? 3 : 1;                     // bytes per pixel
  constexpr int LH = TILE_H + 2 * R;                  // staged rows
  constexpr int ITER = (LH * LG + THREADS - 1) / THREADS;
  const size_t pitch = (size_t)W * CH;
  uint32_t q[ITER][CH];
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int u = threadIdx.x + it * THREADS, lr = u / LG, lg = u - lr * LG;
    const int r = clampi(r0 - R + lr, 0, H - 1), c = clampi(c0 - 4 + 4 * lg, 0, W - 4);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(im.src + (size_t)r * pitch + (size_t)c * CH);
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) q[it][ch] = p[ch];
  }
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int u = threadIdx.x + it * THREADS, lr = u / LG, lg = u - lr * LG;
    const int c = c0 - 4 + 4 * lg;
    uint32_t l4;
    if constexpr (RGB) l4 = luma4(q[it][0], q[it][1], q[it][2]);
    else l4 = q[it][0];
    if constexpr (REPEAT_EDGE) {
      if (c < 0) l4 = (l4 & 0xffu) * 0x01010101u;
      else if (c >= W) l4 = (l4 >> 24) * 0x01010101u;
    }
    if (u < LH * LG) lum[u] = l4;
  }
}

// The dword path of the write-back: four pixels of a row, each plus its delta and saturated to a byte.  px, the three dwords
// (one for a plane) the thread read from the source, take the deltas as packed 16-bit adds and go to dst as dwords.
template <bool RGB>
MI_DEV void store_delta4(uint8_t* dst, const uint32_t (&px)[RGB ? 3 : 1], const int (&delta)[4]) {
  uint32_t* dp = reinterpret_cast<uint32_t*>(dst);
  if constexpr (RGB) {
    dp[0] = add_sat4(px[0], pair(delta[0], delta[0]), pair(delta[0], delta[1]));     // R0 G0 B0 R1
    dp[1] = add_sat4(px[1], pair(delta[1], delta[1]), pair(delta[2], delta[2]));     // G1 B1 R2 G2
    dp[2] = add_sat4(px[2], pair(delta[2], delta[3]), pair(delta[3], delta[3]));     // B2 R3 G3 B3
  } else {
    dp[0] = add_sat4(px[0], pair(delta[0], delta[1]), pair(delta[2], delta[3]));
  }
}

// bytes [first, first + count) of the n <= MAX_IMAGES images of im copied from src to dst (the untouched plane of a planar
// YUV 4:2:0 image); isp_u8_stage.hip
int launch_copy(const Image* im, int n, size_t first, size_t count, hipStream_t stream);

}  // namespace u8
