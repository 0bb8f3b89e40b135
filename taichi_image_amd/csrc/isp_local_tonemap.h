// Local tone mapping (mi_isp_local_tonemap; DESIGN.md 3, "Local tone mapping"): every pixel of a work-dtype RGB image
// (H x W x 3, f16 or f32, interleaved) times a gain that depends only on an edge-aware local mean of its log-luminance,
// read from a bilateral grid: splat, blur, slice.  The operator is stated in integer and single f32 operations (the
// logarithm and the exponential are the piecewise-linear ones of the float's bit pattern), so the kernels' output is the
// contract's bit for bit.  Three plain launches ordered by the stream: splat, blur, apply; each takes up to MAX_IMAGES
// images of one geometry, their pointers in the kernel arguments.
#pragma once
#include "isp_common.h"

namespace ltm {

constexpr int MAX_IMAGES = 32;              // images per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int MAX_SIDE = 32768;             // image rows / columns
constexpr int MAX_BINS = 32;
constexpr int GROUP = 4;                    // pixels per thread and load group, side by side
constexpr int ROW_GROUPS = 16;              // groups per row of a block's region: 64 columns
constexpr int REGION = GROUP * ROW_GROUPS;  // the largest region side of the splat, the tile side of the apply kernel
constexpr int PASSES = REGION / (THREADS / ROW_GROUPS);   // rows of a region per thread: 4, 16 rows apart
constexpr int SPLAT_CELLS = 16;             // cells of a splat region: 4 x 4 of 8 or 16 pixels, 2 x 2 of 32, 1 of 64
constexpr int WAVES = THREADS / 64;         // bin replicas of the splat: one per wave (the decision: DESIGN.md 5.7, 5.14)
// LDS: splat 16 KB of bins (a 64-bit (count, sum) word per wave, cell and bin); apply (ny x nx x bins) (N, S) pairs, dynamic,
// at most 25600 B; for f32 both add 12 KB of staging for the row exchange (isp_local_tonemap.hip, "wave-cooperative rows")

struct Args {
  int H, W;
  int GH, GW;                               // grid nodes: ceil(H / cell), ceil(W / cell)
  int cell, cell_shift, bins;
  int n_images;
  float floor_v, white;                     // the clamp of Y
  int floor_bits;                           // bits(floor)
  float zs;                                 // f32((bins - 1) / li(white))
  float kq;                                 // f32(strength * 4096)
  float la;                                 // f32(li(anchor))
  float inv_cell;                           // 1 / cell
  uint32_t* cnt;                            // the planes of the launch's first image, [GH][GW][bins] each
  uint32_t* sum;
  float* nb;
  float* sb;
  size_t plane;                             // elements from an image's plane to the next image's (0: one image)
  void* im[MAX_IMAGES];
};

// nodes of one image's grid, and the bytes of the four planes of n images (each plane 16-byte aligned)
inline size_t grid_nodes(int H, int W, int cell, int bins) {
  return (size_t)((H + cell - 1) / cell) * ((W + cell - 1) / cell) * bins;
}
inline size_t plane_elems(int H, int W, int cell, int bins) { return (grid_nodes(H, W, cell, bins) + 3) & ~(size_t)3; }
inline size_t workspace_bytes(int n, int H, int W, int cell, int bins) { return 4 * (size_t)n * plane_elems(H, W, cell, bins) * 4; }

// the passes for a.n_images images: `from` .. `to` of splat (0), blur (1), apply (2)
int launch(const Args& a, int dtype, int from, int to, hipStream_t stream);

}  // namespace ltm
