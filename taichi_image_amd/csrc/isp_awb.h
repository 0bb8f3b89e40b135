// Automatic white balance ("Auto white balance"): gray-world statistics gathered from the raw frames every
// load call, and the one-workgroup update that turns them into gains and the effective shading grid E the loaders apply.
// The statistics are integers (u64 sums of fixed-point values), so they are exact and do not depend on the order in
// which blocks arrive.
#pragma once
#include "isp_common.h"

namespace awb {

constexpr int MAX_FRAMES = 32;              // packed frames per statistics launch (grid.y = frame)
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 128;             // blocks per frame; each lane walks its frame's quads THREADS * blocks apart
constexpr int PENDING = 5;                  // P[0..3] per CFA site, then the quad count n

// the quad filter and the shading of the user's grid (shade_gain reads the H, W and sh_* members)
struct Stats {
  int H, W, stride;
  float clip, floor;
  // per-site levels of the loader's pre-cast value x: packed sources x = level_x(v, black[s], k[s]); u16 CFAs
  // x = f32(max(v - black[s], 0)) / den[s] with levels, f32(v) / 65535 without
  int black[4];
  float k[4];
  int has_levels;                           // (CFA sources only)
  int shading;
  const float* sh_gain;
  int sh_sites, sh_gh, sh_gw;
  float sh_sy, sh_sx;
  unsigned long long* pending;              // PENDING u64 values
};

struct PackedArgs {
  Stats s;
  int bits, ids;
  int n_frames;
  const uint8_t* src[MAX_FRAMES];
};

// one launch over a.n_frames packed frames; one launch over one CFA (mode: MI_LOAD_16U / 32F / 16F)
int launch_packed(const PackedArgs& a, hipStream_t stream);
int launch_cfa(const Stats& s, const void* cfa, int mode, hipStream_t stream);

// the update: gathered (world x PENDING i64 rows, may be `pending` itself) summed, the gray-world state and gains moved,
// pending zeroed, E rebuilt.  gathered == NULL: rebuild E from the gains only.  user: the user's grid or NULL (then E is a
// 4 x 2 x 2 grid of the gains).
struct Update {
  const long long* gathered;
  int world;
  unsigned long long* pending;
  int site_colour[4];                        // 0 R, 1 G, 2 B of each CFA site under the demosaic pattern
  double t;
  double* state;                             // S_R, S_G, S_B, valid (0 before the first update with n > 0)
  float* gains;                              // g_R, g_G, g_B
  const float* user;
  int user_sites, gh, gw;
  float* effective;                          // 4 x gh x gw
};
int launch_update(const Update& u, hipStream_t stream);

}  // namespace awb
