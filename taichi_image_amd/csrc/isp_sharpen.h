// Output sharpening (mi_isp_sharpen; DESIGN.md 3, "Output sharpening"): an integer unsharp mask on the luma of a u8 image,
// interleaved RGB (H x W x 3; the same delta is added to R, G and B) or the Y plane of a planar YUV 4:2:0 image.  The
// filter is stated in integer arithmetic, so the kernel's output is the contract's bit for bit.  One launch takes up to
// MAX_IMAGES images of one geometry, their pointers in the kernel arguments.
#pragma once
#include "isp_common.h"

namespace shp {

constexpr int MAX_IMAGES = 32;              // images per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 128;                 // output tile: 32 groups of 4 columns (one group per lane of a half wave) ...
constexpr int TILE_H = 64;                  // ... by 8 strips of ROWS rows
constexpr int ROWS = 8;                     // output rows per thread, one below the other
constexpr int LG = TILE_W / 4 + 2;          // 4-pixel groups per staged luma row: the tile's and one on either side

struct Image {
  const uint8_t* src;
  uint8_t* dst;
};

struct Args {
  int H, W;                                 // of the RGB image, or of the Y plane
  int amount_q6;                            // A = floor(amount * 64 + 0.5), 0 .. 512
  int threshold;                            // coring, luma codes 0 .. 255
  int overshoot;                            // halo clamp 0 .. 255, or -1: none
  int n_images;
  Image im[MAX_IMAGES];
};

// one launch (a.n_images images): rgb (interleaved, 3 bytes per pixel) or a plane (1 byte per pixel), radius 1 or 2
int launch(const Args& a, bool rgb, int radius, hipStream_t stream);
// bytes [first, first + count) of every image copied from src to dst (the chroma rows of a planar YUV 4:2:0 image)
int launch_copy(const Args& a, size_t first, size_t count, hipStream_t stream);

}  // namespace shp
