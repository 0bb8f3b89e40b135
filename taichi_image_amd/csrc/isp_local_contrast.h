// Local contrast (mi_isp_local_contrast; DESIGN.md 3, "Local contrast"): contrast-limited adaptive histogram equalisation
// of the luma of a u8 image, interleaved RGB (H x W x 3; the same delta is added to R, G and B) or the Y plane of a planar
// YUV 4:2:0 image.  The operator is stated in integer arithmetic, so the kernels' output is the contract's bit for bit.
// Four plain launches ordered by the stream: clear, histograms, LUTs, apply; each takes up to u8::MAX_IMAGES images of one
// geometry, their pointers in the kernel arguments.
#pragma once
#include "isp_u8_stage.h"

namespace lc {

constexpr int THREADS = 256;                // 4 waves
constexpr int MAX_TILES = 16;               // tiles per axis
constexpr int MAX_SIDE = 32768;             // image rows / columns
constexpr int BLOCK_W = 128;                // apply block: 32 groups of 4 columns (one group per lane of a half wave) ...
constexpr int BLOCK_H = 64;                 // ... by 8 strips of ROWS rows
constexpr int ROWS = 8;                     // rows per thread of the apply kernel, one below the other
constexpr int LDS_CELLS = 16;               // 2 x 2 LUT cells an apply block keeps in LDS (1 KB each); more: LUTs from L2
constexpr int STRIP_PIXELS = 8192;          // pixels of a tile that one histogram work-group counts

struct Args {
  int H, W;                                 // of the RGB image, or of the Y plane
  int Ty, Tx;                               // tile rows x tile columns
  int clip_q8;                              // C = floor(clip_limit * 256 + 0.5), 0: no clip
  int strength_q6;                          // S = floor(strength * 64 + 0.5), 0 .. 64
  int strip_rows;                           // rows of a tile per histogram work-group
  int n_images;
  uint32_t* hist;                           // [n_images][Ty * Tx][256], 16-byte aligned
  uint8_t* lut;                             // [n_images][Ty * Tx][256]
  u8::Image im[u8::MAX_IMAGES];
};
static_assert(sizeof(Args) == 560 && offsetof(Args, im) == 48, "the kernel arguments' layout");

// workspace of n_images images: the histograms, then the LUTs
inline size_t hist_bytes(int n_images, int Ty, int Tx) { return (size_t)n_images * Ty * Tx * 256 * sizeof(uint32_t); }
inline size_t lut_bytes(int n_images, int Ty, int Tx) { return (size_t)n_images * Ty * Tx * 256; }

// the four launches for a.n_images images: rgb (interleaved, 3 bytes per pixel) or a plane (1 byte per pixel); fills
// a.strip_rows
int launch(Args& a, bool rgb, hipStream_t stream);

}  // namespace lc
