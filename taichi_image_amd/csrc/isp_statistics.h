// Frame statistics (mi_isp_statistics; DESIGN.md 3, "Frame statistics"): the exposure and focus measurements of raw frames -
// per zone and CFA site the count, the sum, the clipped and the dark pixels, per zone a focus measure (the squared
// same-site Laplacian of the green pixels), per site a 256-bin histogram - on the f32 value x each loader computes before
// shading and the cast.  A read-only side output: integers only, so the result does not depend on the launch geometry or
// the order of the atomics.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_raw_source.h"

namespace st {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // tile: 64 columns (one per lane) ...
constexpr int TILE_H = 64;                  // ... by 64 rows: wave w owns rows 16 w .. 16 w + 15
constexpr int PX = TILE_H / 4;              // pixels per lane and tile
constexpr int HALO_R = 2;                   // the focus taps are two pixels away
constexpr int HALO_C = 2;
constexpr int MAX_STRIP = 16;               // a block takes up to 16 consecutive tiles of one tile row
constexpr int CELLS = 16;                   // zone cells of the block's LDS table; a strip that spans more adds to global memory
constexpr int CELL_WORDS = 18;              // 4 sites x {count, sum, clipped, dark}, then {sum of L^2, count}
constexpr int BINS = 256;
constexpr int HIST_COPIES = 4;              // LDS copies of the histogram (lanes of one site spread over them)
constexpr int MAX_ZONES = 32;               // per axis
constexpr long long MAX_PIXELS = 1ll << 26; // sum of L^2 <= 2^36 H W / 2 stays inside an int64

// the words of one frame's result: Z (gh, gw, 4, 4), F (gh, gw, 2), Hist (4, 256)
inline long long words(int gh, int gw) { return (long long)gh * gw * CELL_WORDS + 4 * BINS; }

// zone of pixel row / column x under n zones over `half` quads (n <= half: no zone is empty)
__host__ __device__ inline int zone_of(int x, int n, int half) { return ((x >> 1) * n) / half; }

// true when the block of strip `bx` in tile row `by` keeps its zone cells in LDS: the cells its pixels touch fit the table
__host__ __device__ inline bool lds_route(int H, int W, int gh, int gw, int strip, int bx, int by) {
  const int r0 = by * TILE_H, c0 = bx * strip * TILE_W;
  const int r1 = r0 + TILE_H - 1 < H - 1 ? r0 + TILE_H - 1 : H - 1;
  const int c1 = c0 + strip * TILE_W - 1 < W - 1 ? c0 + strip * TILE_W - 1 : W - 1;
  const int ni = zone_of(r1, gh, H / 2) - zone_of(r0, gh, H / 2) + 1;
  const int nj = zone_of(c1, gw, W / 2) - zone_of(c0, gw, W / 2) + 1;
  return ni * nj <= CELLS;
}

struct Frame {
  const void* src;
  unsigned long long* out;                  // words(gh, gw) int64: Z, F, Hist
  const uint32_t* mask;                     // defect mask (isp_raw_source.h), or NULL
};

struct Args : raw::Source {                 // the decode and the mask: isp_raw_source.h (no shading: the sensor's values)
  int gh, gw;                               // zones
  float clip, dark;                         // clipped: x >= clip; dark: x <= dark
  int gp;                                   // (r, c) is green iff ((r + c) & 1) == gp
  int strip;                                // tiles per block (strip_of)
  int n_frames;
  Frame f[MAX_FRAMES];
};

// tiles per block for n frames of H x W: about 2048 blocks per launch, the strips of a tile row of equal length
inline int strip_of(int H, int W, int n) {
  const long long tx = (W + TILE_W - 1) / TILE_W, ty = (H + TILE_H - 1) / TILE_H;
  long long s = tx * ty * n / 2048;
  s = s < 1 ? 1 : (s > MAX_STRIP ? MAX_STRIP : s);
  const long long nbx = (tx + s - 1) / s;
  return (int)((tx + nbx - 1) / nbx);
}

// one launch (a.n_frames frames): clears every frame's words on the stream, then accumulates; src one of raw::Src
int launch(const Args& a, int src, hipStream_t stream);

}  // namespace st
