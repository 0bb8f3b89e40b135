// Green equalisation (mi_isp_green_equalize; DESIGN.md 3, "Green equalisation"): the two green sites of a Bayer quad (Gr
// beside red, Gb beside blue) differ by a few per cent on many sensors, which the demosaics turn into a one-pixel
// checkerboard.  Every green pixel moves towards the mean of the other green phase around it by half the difference of the
// two phases' local means - where that difference is small enough to be imbalance and both phases are flat enough not to be
// an edge or texture - on the f32 value x each loader computes before shading and the cast.  The kernel writes the gained,
// cast CFA of the work dtype (or the plain f32 y).  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_raw_source.h"
#include "isp_highlights.h"

namespace geq {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (32 pairs; a lane takes a pair, one green site) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows 16 w .. 16 w + 15, two rows per step
constexpr int STEPS = TILE_H / 4 / 2;       // steps per wave
// the halo of radius R: the farthest taps are 2 (R = 1) or 3 (R = 2) pixels away; the decode takes pairs that start on
// even columns, so 3 columns become 4
constexpr int halo_r(int R) { return R == 1 ? 2 : 3; }
constexpr int halo_c(int R) { return R == 1 ? 2 : 4; }

typedef raw::Frame Frame;                   // {src, dst, mask}; dst the work dtype, or f32 for hl::OUT_PLAIN

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the operator: lim = t + s max(O, S), e = edge lim, y = x + hs d with hs = f32(strength) 0.5f; (r, c) is green iff
  // ((r + c) & 1) == gp
  float t, s, edge, hs;
  int gp;
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of raw::Src, out one of hl::Out, radius 1 or 2
int launch(const Args& a, int src, int out, int radius, hipStream_t stream);

}  // namespace geq
