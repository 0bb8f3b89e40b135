// Raw-domain noise reduction (mi_isp_denoise; DESIGN.md 3, "Raw noise reduction"): an edge-preserving bilateral filter
// over same-site neighbours, adapted to the sensor's noise model, on the f32 value x each loader computes before shading
// and the cast.  The kernel writes the filtered, gained, cast CFA of the work dtype; the demosaic and everything after it
// then run unchanged on that CFA.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_common.h"

namespace dn {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows of parity w & 1 in half (w >> 1)
constexpr int PX = TILE_H / 4;              // output pixels per lane, two rows apart

// the sources the kernel decodes (x is the loader's pre-shading, pre-cast f32 value)
enum Src {
  SRC_P12 = 0,                              // packed 12-bit, standard layout: levels (or the plain decode)
  SRC_P12_IDS = 1,                          // packed 12-bit, IDS layout
  SRC_P16 = 2,                              // packed 16-bit little-endian
  SRC_U16 = 3,                              // load_16u: u16 codes / 65535, or levels with a true division
  SRC_U16F = 4,                             // load_16f: f32(u16)
  SRC_F32 = 5,                              // load_32f: the f32 value
  SRC_CFA_F16 = 6,                          // denoise_cfa: a normalised f16 CFA
  SRC_CFA_F32 = 7,                          // denoise_cfa: a normalised f32 CFA
};

struct Frame {
  const void* src;
  void* dst;                                // H x W work-dtype CFA
  const uint32_t* mask;                     // defect mask (H rows x mask_w words, bit c & 31 of word c >> 5), or NULL
};

struct Args {
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
  // the filter: var = gain * max(x, 0) + rn2; kl = min(c2 / var, FLT_MAX) (c2 = log2(e) / (2 strength^2));
  // w = exp2(-(x(q) - x(p))^2 * kl - sp[i*i + j*j]), sp[d] = d * log2(e) / (2 spatial_sigma^2)
  float gain, rn2, c2;
  float sp[9];
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of Src, work dtype MI_F16 / MI_F32, radius 1 or 2
int launch(const Args& a, int src, int work_dtype, int radius, hipStream_t stream);

}  // namespace dn
