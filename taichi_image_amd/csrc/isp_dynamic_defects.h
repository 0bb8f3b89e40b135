// Dynamic defective-pixel correction (mi_isp_dynamic_defects; DESIGN.md 3, "Dynamic defects"): a raw pixel that stands out
// of its eight same-site neighbours at distance 2 by more than a threshold that grows with the signal is replaced by the
// mean of the neighbour pair that agrees best, clamped to the neighbours' range - without a calibrated map, and whatever
// the Bayer pattern - on the f32 value x each loader computes before shading and the cast.  The kernel writes the gained,
// cast CFA of the work dtype (or the plain f32 y for the next raw stage to take) and, optionally, the plane of flagged
// pixels in the defect mask's layout.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_raw_source.h"
#include "isp_highlights.h"

namespace ddp {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows 16 w .. 16 w + 15
constexpr int PX = TILE_H / 4;              // output pixels per lane
constexpr int HALO_R = 2;                   // the taps are two pixels away, in rows ...
constexpr int HALO_C = 2;                   // ... and in columns (even, as the decode's pairs)

struct Frame {
  const void* src;
  void* dst;                                // H x W CFA: the work dtype, or f32 for hl::OUT_PLAIN
  const uint32_t* mask;                     // defect mask (H rows x mask_w words), or NULL
  uint32_t* flags;                          // the flagged pixels (H rows x mask_w words, every word written), or NULL
};

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the operator: T(v) = t + s max(v, 0); k = tolerate (0 or 1) of a pixel's neighbours may be defective themselves
  float t, s;
  int tolerate, hot, dead;
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of raw::Src, out one of hl::Out
int launch(const Args& a, int src, int out, hipStream_t stream);

}  // namespace ddp
