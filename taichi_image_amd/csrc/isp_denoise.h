// Raw-domain noise reduction (mi_isp_denoise; DESIGN.md 3, "Raw noise reduction"): an edge-preserving bilateral filter
// over same-site neighbours, adapted to the sensor's noise model, on the f32 value x each loader computes before shading
// and the cast.  The kernel writes the filtered, gained, cast CFA of the work dtype; the demosaic and everything after it
// then run unchanged on that CFA.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_raw_source.h"

namespace dn {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows of parity w & 1 in half (w >> 1)
constexpr int PX = TILE_H / 4;              // output pixels per lane, two rows apart

typedef raw::Frame Frame;                   // {src, dst, mask}; dst the work-dtype CFA

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the filter: var = gain * max(x, 0) + rn2; kl = min(c2 / var, FLT_MAX) (c2 = log2(e) / (2 strength^2));
  // w = exp2(-(x(q) - x(p))^2 * kl - sp[i*i + j*j]), sp[d] = d * log2(e) / (2 spatial_sigma^2)
  float gain, rn2, c2;
  float sp[9];
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of raw::Src, work dtype MI_F16 / MI_F32, radius 1 or 2
int launch(const Args& a, int src, int work_dtype, int radius, hipStream_t stream);

}  // namespace dn
