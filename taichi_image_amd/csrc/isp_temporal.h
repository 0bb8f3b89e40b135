// Temporal noise reduction (mi_isp_temporal; DESIGN.md 3, "Temporal noise reduction"): every raw pixel is blended with
// the same camera's previous output where the scene has not moved - the mean absolute difference to the history over the
// pixel's 3 x 3 same-site window, measured against the sensor's noise model - and returned untouched where it has, on the
// f32 value x each loader computes before shading and the cast.  The kernel writes the new history plane (the plain f32 y)
// and the gained, cast CFA of the work dtype; with the plain output the history plane is the only write, and the next raw
// stage reads it.  One launch takes up to MAX_FRAMES frames of one geometry, each with its own two history planes.
#pragma once
#include "isp_raw_source.h"

namespace tn {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows of parity w & 1 in half (w >> 1)
constexpr int PX = TILE_H / 4;              // output pixels per lane, two rows apart
constexpr int HALO = 2;                     // the taps are one same-site step (two pixels) away

enum Out { OUT_F16 = 0, OUT_F32 = 1, OUT_PLAIN = 2 };   // work-dtype CFA with gain and cast, or the history plane alone

struct Frame {
  const void* src;
  void* dst;                                // H x W work-dtype CFA (unused for OUT_PLAIN)
  const float* hist_in;                     // H x W f32: the previous output, or NULL for an empty history
  float* hist_out;                          // H x W f32: this frame's y
  const uint32_t* mask;                     // defect mask (H rows x mask_w words, bit c & 31 of word c >> 5), or NULL
};

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the operator: var = gain * max(h, 0) + rn2; qv = (m * m) / (c * var); w = wmax * max(1 - qv, 0);
  // m = D * rcp_n[n], rcp_n[n] = f32(1 / n) for n = 1 .. 9 (rcp_n[0] is not used)
  float gain, rn2, c, wmax;
  float rcp_n[10];
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of raw::Src, out one of Out
int launch(const Args& a, int src, int out, hipStream_t stream);

}  // namespace tn
