// Direction-adaptive demosaic (mi_isp_demosaic_directional_*; DESIGN.md 3, "Directional demosaic"): an alternative to the
// 13-tap filter of isp_tile.h that interpolates green along the direction in which the colour differences vary least, and
// red and blue from the colour differences of that green.  The kernel takes any source of isp_raw_source.h (a normalised
// CFA, or a raw frame with levels and a shading / AWB gain, which it stages as the loaders' CFA, bit for bit) and writes
// the RGB image through mi_isp_demosaic's epilogue.  One launch takes up to MAX_FRAMES frames of one geometry.
#pragma once
#include "isp_raw_source.h"

namespace dd {

constexpr int MAX_FRAMES = 32;              // frames per launch (grid.z)
constexpr int THREADS = 256;                // 4 waves
constexpr int TILE_W = 64;                  // output tile: 64 columns (a lane takes a column pair: 32 lanes a row) ...
constexpr int TILE_H = 32;                  // ... by 32 rows
// the stencil of an output pixel (r, c) on the mirror-extended CFA X (derived in DESIGN.md 3): step 5 reads R - B of the
// green sites one pixel away, those read G of the red / blue sites one further (|dr| + |dc| <= 2), and G of a site
// (r', c') reads X over rows r' - 2 .. r' + 6 and columns c' - 2 .. c' + 6 (the classifier's windows start at the site and
// its differences look two pixels ahead): rows r - 4 .. r + 8, columns c - 4 .. c + 8
constexpr int HALO_B = 4;                   // halo before the tile (rows above, columns left)
constexpr int HALO_A = 8;                   // halo after it
constexpr int LW = TILE_W + HALO_B + HALO_A;    // LDS plane: 76 floats a row ...
constexpr int LH = TILE_H + HALO_B + HALO_A;    // ... by 44 rows; three planes: 40128 bytes, four blocks a CU

// the decode-only kernel (mi_isp_raw_cfa_batch): a block takes CFA_TILE_W x CFA_TILE_H pixels, a lane a column pair
constexpr int CFA_TILE_W = 128;
constexpr int CFA_TILE_H = 32;

struct Frame {
  const void* src;
  void* dst;                                // H x W x 3 RGB (the demosaic) or the H x W work-dtype CFA (the decode)
};

struct Args : raw::Source {                 // the decode and the gain: isp_raw_source.h (mask_w is not used)
  int green_par;                            // (row + col) & 1 of the green sites under the pattern
  int red_par;                              // row & 1 of the rows that hold red
  int has_ccm;
  float ccm[9];
  float out_scale;                          // scale_factor of the output dtype
  int n_frames;
  Frame f[MAX_FRAMES];
};

// one launch (a.n_frames frames): src one of raw::Src, work MI_F16 / MI_F32 (the CFA's dtype), out the image's MI_* dtype
// (a raw source writes the work dtype)
int launch(const Args& a, int src, int work, int out, hipStream_t stream);
// the decode alone: the work-dtype CFA of a raw source
int launch_cfa(const Args& a, int src, int work, hipStream_t stream);

}  // namespace dd
