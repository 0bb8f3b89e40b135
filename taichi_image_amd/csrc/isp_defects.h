// Defective pixel correction (mi_isp_defects; DESIGN.md 3, "Defective pixels"): sparse fix-ups launched right after a
// load on the same stream.  The dense load kernels are not touched: the packed route recomputes only the listed output
// pixels (those whose value reads a defective raw site), straight from the packed bytes; the convert route patches the
// defective sites of the work-dtype CFA in place before the demosaic.
#pragma once
#include "isp_tile.h"

namespace dfx {

constexpr int MAX_CAMS = 32;                // cameras per fix-up launch (the kernel argument block stays under 2 KB)
constexpr int THREADS = 256;

// one camera of a packed fix-up: its frame, outputs, defect mask and output list
struct Cam {
  const uint8_t* src;
  void* dst;
  void* sub;                                // the metering subsample, or NULL
  const uint32_t* mask;                     // H rows x mask_w words, bit (c & 31) of word c >> 5
  const int32_t* list;                      // output pixel indices (row * Wd + col), unique
  int start;                                // first lane of this camera in the launch
  int n;                                    // entries of list
};

struct Args {
  tile::Params t;                           // the loader's decode (levels: always the per-site arrays), ccm, pattern
  int Hd, Wd;
  int resize;                               // 1: the fused bilinear resize with scale s (interpolate.py:24-34)
  float s;
  int st, sub_w;                            // metering stride and subsample row length
  int pr, pc;                               // pattern row / column phase (KIDX = ((r + pr) & 1) + 2 ((c + pc) & 1))
  int mask_w;
  int n_cams, total;
  Cam cam[MAX_CAMS];
};

// the packed fix-up for work dtype MI_F16 / MI_F32 (a.total > 0)
int launch_packed(const Args& a, int work_dtype, hipStream_t stream);
// the in-place CFA fix-up of the convert route: the n sites of coords (row, col pairs) of an H x W work-dtype CFA
int launch_cfa(void* cfa, int H, int W, int work_dtype, const int32_t* coords, int n, const uint32_t* mask,
               hipStream_t stream);

}  // namespace dfx
