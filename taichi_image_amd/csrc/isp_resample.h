// Antialiased resize (mi_isp_resample_*; DESIGN.md 3, "Antialiased resize", and 5.17): a separable resize driven by one
// table per axis (built on the host: rs::taps / rs::table), both passes in one launch.  A block owns an output tile of up to
// OW x OH pixels and walks the source rows the tile needs in increasing order, ROWS at a time: it copies their segments
// into LDS in 16-byte units, filters them horizontally into an f32 ring of LDS rows and emits every output row whose last
// tap row is in.  The horizontally filtered image never exists in memory.
#pragma once
#include "isp_common.h"

namespace rs {

constexpr int MAX_TAPS = MI_RESAMPLE_MAX_TAPS;  // taps per axis
constexpr int OW = 64;                      // output tile: 64 columns (a thread takes one channel of one column) ...
constexpr int OH = 32;                      // ... by 32 rows
constexpr int THREADS = OW * 3;             // 192: 3 waves
constexpr int ROWS = 4;                     // source rows a step stages and filters
constexpr int SEG_PX = 512;                 // source pixels of a row the LDS segment holds: a tile whose columns span more
                                            // (area and triangle below scale 0.13) reads its taps from memory instead
constexpr int MAX_IMAGES = 32;              // images per launch (grid.z)

struct Axis {
  int taps;                                 // T
  const int32_t* start;                     // D starts (device)
  const float* weight;                      // D x T weights (device)
};

struct Image {
  const void* src;
  void* dst;
};

struct Args {
  int Hs, Ws, Hd, Wd;
  Axis rows, cols;                          // the vertical (S = Hs, D = Hd) and the horizontal axis
  int n_images;
  Image im[MAX_IMAGES];
};

// the LDS bytes of a block for these tap counts and source element size
size_t lds_bytes(int taps_y, int taps_x, int in_size);

// T of an axis, or -1 with the error set (host only)
int taps(int filter, int S, int D, double scale, const char* who);
// the table of an axis (host only): start[D], weight[D * T]
int table(int filter, int S, int D, double scale, int32_t* start, float* weight, const char* who);

// one launch (a.n_images images); in / out MI_F16 or MI_F32
int launch(const Args& a, int in_dtype, int out_dtype, hipStream_t stream);

}  // namespace rs
