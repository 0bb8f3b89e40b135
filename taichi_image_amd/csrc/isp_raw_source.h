// The raw stages' front end: what raw noise reduction (dn), highlight reconstruction (hl), chromatic aberration (ca),
// temporal noise reduction (tn) and exposure merge (em) share in front of their operators.  Every stage reads the f32
// value x a loader computes before shading and the cast, from one of the sources of Src, by the ONE decode below (the
// loaders' own arithmetic: every loader-parity guarantee of the stages rests on it).  Source holds the kernel arguments
// of that decode, of the shading / AWB gain and of the defect mask; each stage's Args derives from it and adds its
// operator's members and its frames.
#pragma once
#include <type_traits>

#include "isp_common.h"
#include "isp_tile.h"

namespace raw {

// the sources the kernels decode (x is the loader's pre-shading, pre-cast f32 value)
enum Src {
  SRC_P12 = 0,                              // packed 12-bit, standard layout: levels (or the plain decode)
  SRC_P12_IDS = 1,                          // packed 12-bit, IDS layout
  SRC_P16 = 2,                              // packed 16-bit little-endian
  SRC_U16 = 3,                              // load_16u: u16 codes / 65535, or levels with a true division
  SRC_U16F = 4,                             // load_16f: f32(u16)
  SRC_F32 = 5,                              // load_32f: the f32 value
  SRC_CFA_F16 = 6,                          // the _cfa entry points: a normalised f16 CFA
  SRC_CFA_F32 = 7,                          // the _cfa entry points: a normalised f32 CFA
};

// the first 80 bytes of every stage's kernel arguments (8-byte aligned, no tail padding: a derived Args continues at 80)
struct Source {
  int H, W;
  // decode: packed sources use x = f32(max(v - black[s], 0)) * k[s] (black 0, k = k_decode without levels); SRC_U16
  // with levels uses f32(max(v - black[s], 0)) / k[s] (k the denominators white - black), without them f32(v) / 65535
  int levels;
  int black[4];
  float k[4];
  // lens shading / AWB gain (the members shade_gain reads); shading 0: gain 1
  int shading;
  const float* sh_gain;
  int sh_sites, sh_gh, sh_gw;
  float sh_sy, sh_sx;
  int mask_w;
};

struct Frame {
  const void* src;
  void* dst;                                // H x W CFA: the work dtype, or f32 for a plain output
  const uint32_t* mask;                     // defect mask (H rows x mask_w words, bit c & 31 of word c >> 5), or NULL
};

// x of raw pixels (r, c) and (r, c + 1), c even, row r inside the frame; two: c + 1 is inside the frame
template <int SRC>
MI_DEV void decode_pair(const Source& a, const void* src, int r, int c, bool two, float& x0, float& x1) {
  const bool odd = (r & 1) != 0;                     // (selects: a run-time index would put the arrays in scratch)
  const int b0 = odd ? a.black[2] : a.black[0], b1 = odd ? a.black[3] : a.black[1];
  const float k0 = odd ? a.k[2] : a.k[0], k1 = odd ? a.k[3] : a.k[1];
  if constexpr (SRC == SRC_P12 || SRC == SRC_P12_IDS) {
    const uint8_t* q = static_cast<const uint8_t*>(src) + (size_t)r * ((size_t)a.W * 3 / 2) + (size_t)(c >> 1) * 3;
    uint32_t p0, p1;
    tile::unpack_pair(q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), SRC == SRC_P12_IDS, p0, p1);
    x0 = tile::level_x(p0, b0, k0);
    x1 = tile::level_x(p1, b1, k1);
  } else if constexpr (SRC == SRC_P16) {
    const uint8_t* q = static_cast<const uint8_t*>(src) + ((size_t)r * a.W + c) * 2;
    x0 = tile::level_x(q[0] | ((uint32_t)q[1] << 8), b0, k0);
    x1 = two ? tile::level_x(q[2] | ((uint32_t)q[3] << 8), b1, k1) : 0.f;
  } else if constexpr (SRC == SRC_U16) {
    const uint16_t* q = static_cast<const uint16_t*>(src) + (size_t)r * a.W + c;
    const uint32_t v0 = q[0], v1 = two ? q[1] : 0u;
    if (a.levels) {                                   // load_u16_levels_kernel's quotient
      const int d0 = (int)v0 - b0, d1 = (int)v1 - b1;
      x0 = (float)(d0 > 0 ? d0 : 0) / k0;
      x1 = (float)(d1 > 0 ? d1 : 0) / k1;
    } else {                                          // load_convert_kernel's
      x0 = (float)v0 / 65535.0f;
      x1 = (float)v1 / 65535.0f;
    }
  } else if constexpr (SRC == SRC_U16F) {
    const uint16_t* q = static_cast<const uint16_t*>(src) + (size_t)r * a.W + c;
    x0 = (float)q[0];
    x1 = two ? (float)q[1] : 0.f;
  } else if constexpr (SRC == SRC_F32 || SRC == SRC_CFA_F32) {
    const float* q = static_cast<const float*>(src) + (size_t)r * a.W + c;
    x0 = q[0];
    x1 = two ? q[1] : 0.f;
  } else {
    const half_t* q = static_cast<const half_t*>(src) + (size_t)r * a.W + c;
    x0 = (float)q[0];
    x1 = two ? (float)q[1] : 0.f;
  }
}

// x of the one raw pixel (r, c) inside the frame: a kernel decodes a listed centre pixel again (rare), as the pair's member
template <int SRC>
MI_DEV float decode_one(const Source& a, const void* src, int r, int c) {
  float p0, p1;
  decode_pair<SRC>(a, src, r, c & ~1, (c | 1) < a.W, p0, p1);
  return (c & 1) ? p1 : p0;
}

// The tile at (r0, c0) and its halo, decoded once by the block's THREADS threads into xs (TILE_H + 2 HALO_R rows of
// TILE_W + 2 HALO_C floats): x, or -inf for a tap that is outside the frame or a listed defect.  Pairs start on even frame
// columns (c0 and HALO_C are even), so a pair's two sites and its mask bits are those of (c, c + 1).  The caller
// synchronises the block.  (src and mask by reference: they are kernel arguments, read where the loop uses them.)
template <int SRC, int TILE_H, int TILE_W, int HALO_R, int HALO_C, int THREADS>
MI_DEV void stage_tile(const Source& a, const void* const& src, const uint32_t* const& mask, int r0, int c0,
                       float (&xs)[(TILE_H + 2 * HALO_R) * (TILE_W + 2 * HALO_C)]) {
  constexpr int LW = TILE_W + 2 * HALO_C;             // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO_R;
  constexpr int LP = LW / 2;                          // column pairs per LDS row
  static_assert(HALO_C % 2 == 0 && TILE_W % 2 == 0, "pairs start on even columns");
  const int H = a.H, W = a.W;
  for (int u = threadIdx.x; u < LH * LP; u += THREADS) {
    const int lr = u / LP, lp = u - lr * LP;
    const int r = r0 - HALO_R + lr, c = c0 - HALO_C + 2 * lp;
    float x0 = -INFINITY, x1 = -INFINITY;
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const bool two = c + 1 < W;
      decode_pair<SRC>(a, src, r, c, two, x0, x1);
      if (!two) x1 = -INFINITY;
      if (mask) {
        const uint32_t m = mask[(size_t)r * a.mask_w + (c >> 5)] >> (c & 31);
        if (m & 1u) x0 = -INFINITY;
        if (m & 2u) x1 = -INFINITY;
      }
    }
    *reinterpret_cast<float2*>(&xs[lr * LW + 2 * lp]) = make_float2(x0, x1);
  }
}

// f(std::integral_constant<int, SRC>{}) for the run-time source kind src: every stage instantiates its kernels for all
// eight sources through one generic lambda
template <class F>
int dispatch_src(int src, F&& f) {
  switch (src) {
    case SRC_P12: return f(std::integral_constant<int, SRC_P12>{});
    case SRC_P12_IDS: return f(std::integral_constant<int, SRC_P12_IDS>{});
    case SRC_P16: return f(std::integral_constant<int, SRC_P16>{});
    case SRC_U16: return f(std::integral_constant<int, SRC_U16>{});
    case SRC_U16F: return f(std::integral_constant<int, SRC_U16F>{});
    case SRC_F32: return f(std::integral_constant<int, SRC_F32>{});
    case SRC_CFA_F16: return f(std::integral_constant<int, SRC_CFA_F16>{});
    default: return f(std::integral_constant<int, SRC_CFA_F32>{});
  }
}

}  // namespace raw
