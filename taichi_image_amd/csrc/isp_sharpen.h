// Output sharpening (mi_isp_sharpen; DESIGN.md 3, "Output sharpening"): an integer unsharp mask on the luma of a u8 image,
// interleaved RGB (H x W x 3; the same delta is added to R, G and B) or the Y plane of a planar YUV 4:2:0 image.  The
// filter is stated in integer arithmetic, so the kernel's output is the contract's bit for bit.  One launch takes up to
// u8::MAX_IMAGES images of one geometry, their pointers in the kernel arguments.
#pragma once
#include "isp_u8_stage.h"

namespace shp {

constexpr int ROWS = 8;                     // output rows per thread, one below the other: 8 strips to a u8::TILE_H tile

struct Args {
  int H, W;                                 // of the RGB image, or of the Y plane
  int amount_q6;                            // A = floor(amount * 64 + 0.5), 0 .. 512
  int threshold;                            // coring, luma codes 0 .. 255
  int overshoot;                            // halo clamp 0 .. 255, or -1: none
  int n_images;
  u8::Image im[u8::MAX_IMAGES];
};
static_assert(sizeof(Args) == 536 && offsetof(Args, im) == 24, "the kernel arguments' layout");

// one launch (a.n_images images): rgb (interleaved, 3 bytes per pixel) or a plane (1 byte per pixel), radius 1 or 2
int launch(const Args& a, bool rgb, int radius, hipStream_t stream);

}  // namespace shp
