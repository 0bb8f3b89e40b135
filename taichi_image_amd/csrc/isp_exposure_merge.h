// Exposure merge (mi_isp_exposure_merge; DESIGN.md 3, "Exposure merge"): E raw frames of one camera and one instant, the
// shortest exposure first, become one linear raw frame y in the units of the shortest: every long frame, scaled back by
// its exposure ratio, is weighted by its inverse variance where it is usable - fading out towards saturation, and dropped
// completely where its 3 x 3 same-site window disagrees with the shortest frame beyond the sensor's noise model - on the
// f32 values x_e each loader computes before shading and the cast.  The kernel writes the gained, cast CFA of the work
// dtype, or the plain f32 y for the next raw stage.  One launch takes up to MAX_BRACKETS brackets of one geometry.
#pragma once
#include "isp_raw_source.h"

namespace em {

constexpr int MAX_BRACKETS = 16;            // brackets per launch (grid.z)
constexpr int MAX_E = 4;                    // exposures per bracket
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (a column pair per lane, two rows per wave and step) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: half-wave g owns rows of parity g & 1 in quarter (g >> 1)
constexpr int PX = TILE_H / 8;              // output rows per lane, two rows apart (2 PX pixels)
constexpr int HALO = 2;                     // the taps are one same-site step (two pixels) away

enum Out { OUT_F16 = 0, OUT_F32 = 1, OUT_PLAIN = 2 };   // work-dtype CFA with gain and cast, or the plain f32 y

struct Bracket {
  const void* src[MAX_E];                   // the E frames, shortest exposure first
  void* dst;                                // H x W work-dtype CFA, or the plain f32 y
  const uint32_t* mask;                     // defect mask (H rows x mask_w words, bit c & 31 of word c >> 5), or NULL
};

struct Args : raw::Source {                 // the decode, the gain and the mask: isp_raw_source.h
  // the operator: inv[e] = f32(1 / ratio_e), i2[e] = f32(1 / ratio_e^2), rn2 = read_noise^2,
  // c = threshold^2, rf = 1 / (saturation * knee), rcp_n[n] = f32(1 / n) for n = 1 .. 9 (rcp_n[0] is not used)
  int E;
  float inv[MAX_E], i2[MAX_E];
  float gain, rn2, c, sat, rf;
  float rcp_n[10];
  int n_brackets;
  Bracket b[MAX_BRACKETS];
};

// one launch (a.n_brackets brackets): src one of raw::Src, out one of Out
int launch(const Args& a, int src, int out, hipStream_t stream);

}  // namespace em
