// Lens distortion correction (mi_isp_lens; DESIGN.md 3, "Lens distortion"): a bilinear remap of an RGB image through
// OpenCV's pinhole model with radial / tangential distortion (the analytic form), or through a table of source
// coordinates.  One launch takes up to MAX_CAMS frames of one geometry, each with its own pointers and lens.
#pragma once
#include "isp_common.h"

namespace lens {

constexpr int MAX_CAMS = 32;                // frames per launch (the argument block stays under 4 KB)
constexpr int THREADS = 256;
constexpr int PX = 4;                       // output pixels per lane, THREADS apart

// the f32 lens parameters of one frame, rounded once from the host's doubles
struct Model {
  float fx, fy, cx, cy;                     // K: source pixels from normalised distorted coordinates
  float ncx, ncy, ifx, ify;                 // new_K: cx', cy', f32(1 / fx'), f32(1 / fy')
  float k1, k2, k3, k4, k5, k6, p1, p2;     // k3 = 0 for 4 coefficients; k4..k6 only read when rational
  int rational;
};

struct Cam {
  const void* src;
  void* dst;
  const float* table;                       // (Hd, Wd, 2) (us, vs) of the table form, else NULL
  Model m;
};

struct Args {
  int H, W, Hd, Wd;
  float s0, s1;                             // output scale (row, col): u = f32(c) / s1, v = f32(r) / s0
  float intensity;                          // scale(out) / scale(in), as the resize
  int n_cams;
  Cam cam[MAX_CAMS];
};

// one launch (a.n_cams frames, grid.y = frame); table: the table form; border: MI_BORDER_*
int launch(const Args& a, int in_dtype, int out_dtype, bool table, int border, hipStream_t stream);

}  // namespace lens
