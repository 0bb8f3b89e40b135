// Output sharpening (mi_isp_sharpen; DESIGN.md 3, "Output sharpening"): an integer unsharp mask on the luma of a u8 image,
// interleaved RGB (H x W x 3; the same delta is added to R, G and B) or the Y plane of a planar YUV 4:2:0 image.  The
// filter is stated in integer arithmetic, so the kernel's output is the contract's bit for bit.  One launch takes up to
// MAX_IMAGES images of one geometry, their pointers in the kernel arguments.
#pragma once
#include "isp_common.h"

namespace shp {

constexpr int MAX_IMAGES = 32;              // images per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 128;                 // output tile: 32 groups of 4 columns (one group per lane of a half wave) ...
constexpr int TILE_H = 64;                  // ... by 8 strips of ROWS rows
constexpr int ROWS = 8;                     // output rows per thread, one below the other
constexpr int LG = TILE_W / 4 + 2;          // 4-pixel groups per staged luma row: the tile's and one on either side

struct Image {
  const uint8_t* src;
  uint8_t* dst;
};

struct Args {
  int H, W;                                 // of the RGB image, or of the Y plane
  int amount_q6;                            // A = floor(amount * 64 + 0.5), 0 .. 512
  int threshold;                            // coring, luma codes 0 .. 255
  int overshoot;                            // halo clamp 0 .. 255, or -1: none
  int n_images;
  Image im[MAX_IMAGES];
};

// ---- byte helpers of the u8 output filters (this one and isp_local_contrast.hip) -------------------------------------
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

// one launch (a.n_images images): rgb (interleaved, 3 bytes per pixel) or a plane (1 byte per pixel), radius 1 or 2
int launch(const Args& a, bool rgb, int radius, hipStream_t stream);
// bytes [first, first + count) of every image copied from src to dst (the chroma rows of a planar YUV 4:2:0 image)
int launch_copy(const Args& a, size_t first, size_t count, hipStream_t stream);

}  // namespace shp
