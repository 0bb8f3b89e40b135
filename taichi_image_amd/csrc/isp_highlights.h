// Highlight reconstruction (mi_isp_highlights; DESIGN.md 3, "Highlight reconstruction"): raw pixels at the sensor's clip
// level are raised to the brightest white-balanced mean of their unclipped neighbour colours ("rebuild"), or every pixel is
// limited to the balanced clip level ("clip"), on the f32 value x each loader computes before shading and the cast.  The
// kernel writes the gained, cast CFA of the work dtype (or the plain f32 y for raw noise reduction to filter); the demosaic
// and everything after it then run unchanged on that CFA.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_raw_source.h"

namespace hl {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows 16 w .. 16 w + 15
constexpr int PX = TILE_H / 4;              // output pixels per lane
constexpr int HALO_R = 1;                   // halo rows: the taps are one pixel away ...
constexpr int HALO_C = 2;                   // ... and the decode takes pairs that start on even columns

enum Mode { MODE_REBUILD = 0, MODE_CLIP = 1 };
enum Out { OUT_F16 = 0, OUT_F32 = 1, OUT_PLAIN = 2 };   // work-dtype CFA with gain and cast, or the plain f32 y

typedef raw::Frame Frame;                   // {src, dst, mask}; dst the work dtype, or f32 for OUT_PLAIN

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the operator: t = f32(clip); the balance gains of R, G, B (wb_dev, when not NULL, overrides wb: 3 f32 on the device,
  // read by the kernel); colour[s] of CFA site s = (row & 1) * 2 + (col & 1) under the demosaic pattern
  int mode;
  float t;
  float wb[3];
  const float* wb_dev;
  int colour[4];
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of raw::Src, out one of Out
int launch(const Args& a, int src, int out, hipStream_t stream);

}  // namespace hl
