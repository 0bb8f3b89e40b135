// Lateral chromatic aberration correction (mi_isp_chromatic; DESIGN.md 3, "Chromatic aberration"): the red and the blue
// site planes of the CFA are resampled radially about the optical centre (bilinear within the plane, a scale that is a
// polynomial in the squared radius), green is left alone, on the f32 value x each loader computes before shading and the
// cast.  The kernel writes the gained, cast CFA of the work dtype (or the plain f32 y for the next raw stage to take); the
// demosaic and everything after it then run unchanged on that CFA.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include <cmath>
#include "isp_raw_source.h"
#include "isp_highlights.h"

namespace ca {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows 16 w .. 16 w + 15
constexpr int PX = TILE_H / 4;              // output pixels per lane
constexpr int HALO = 12;                    // the largest halo (rows and columns): a shift of MAX_SHIFT, the second tap of the
                                            // site plane (2 more), slack for the f32 rounding of the sampling position; even,
                                            // as the decode's pairs.  A launch stages the halo its own settings need (halo_for)
constexpr double HALO_SLACK = 0.5;          // raw pixels: the f32 rounding of vs / us, the shift between the sampled radii
constexpr double MAX_SHIFT = 8.0;           // the largest shift (raw pixels) the host accepts
constexpr int SHIFT_SAMPLES = 1025;         // radii at which the host evaluates the shift

typedef raw::Frame Frame;                   // {src, dst, mask}; dst the work dtype, or f32 for hl::OUT_PLAIN

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the operator: the centre, 1 / norm_radius^2 and (k0 - 1, k1, k2) of red and of blue, each rounded once from the
  // host's doubles; colour[s] of CFA site s = (row & 1) * 2 + (col & 1) under the demosaic pattern
  float cy, cx, iR2;
  float dr[3], db[3];
  int halo;                                 // staged halo rows and columns: halo_for(the largest shift on the frame)
  int colour[4];
  int n_frames;
  Frame f[MAX_FRAMES];
};

// the halo that covers every tap of a shift of at most `shift` raw pixels: the taps of non-zero weight lie fewer than
// shift + 2 rows from the pixel and have its parity (at most the even ceiling of shift), a shift that is an even integer
// adds a tap of weight 0 two rows further out; even, 4 .. HALO
inline int halo_for(double shift) {
  const int h = 2 * (int)std::ceil((shift + HALO_SLACK) / 2.0) + 2;
  return h < 4 ? 4 : (h > HALO ? HALO : h);
}

// one launch (a.n_frames frames): src one of raw::Src, out one of hl::Out
int launch(const Args& a, int src, int out, hipStream_t stream);

}  // namespace ca
