// Highlight reconstruction kernels (isp_highlights.h; the contract is DESIGN.md 3, "Highlight reconstruction").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value, site s(p) = (r & 1) * 2 + (c & 1), w[s] the f32
// balance gain of the site's colour, b(q) = x(q) * w[s(q)] and t the clip level:
//   rebuild: p with x(p) >= t takes e = the larger of the means of b over its two tap groups (R / B site: the four G
//            neighbours, the four diagonal neighbours; G site: the row neighbours, the column neighbours; taps inside the
//            frame and not in the defect mask, summed in the listed order, divided by their count) and, when e > b(p),
//            y = max(x(p), e / w[s(p)]); every other pixel keeps y = x(p), the same bits
//   clip:    y = min(x(p), (t * min(w)) / w[s(p)])   (a listed defect keeps x(p) in both modes: the fix-up replaces it)
//   cfa = cast_work(y * g(p))   (g the shading / AWB gain, 1 without a grid), or the plain f32 y
// Every operation is one f32 rounding (no contraction, IEEE divisions): the output is the contract's bit for bit.
//
// One 256-thread block per 64 x 64 output tile of one frame (grid.z): the tile plus a halo of one row and two columns (the
// decode takes the pairs of isp_raw_source.h, which start on even columns) is decoded ONCE into LDS as f32 x, excluded taps
// (outside the frame, or listed defects) as -inf.  Lane l of wave w then takes column l of rows 16 w .. 16 w + 15.  Almost
// every wave of a real frame holds no clipped pixel, so the neighbour arithmetic sits behind a wave-uniform branch (a
// ballot of x >= t): the common case is decode, gain, cast and store.
#include "isp_highlights.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace hl {

// one tap group: the f32 sum of the kept taps' balanced values in the order given, starting from the first kept tap
struct Group { float S; int n; };
MI_DEV void tap(Group& g, float x, float w) {
  if (x != -INFINITY) {                               // (an excluded tap)
    const float b = x * w;
    g.S = g.n ? g.S + b : b;
    ++g.n;
  }
}

template <int OUT> struct OutType { typedef float type; };
template <> struct OutType<OUT_F16> { typedef half_t type; };

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, int OUT>
__global__ void __launch_bounds__(THREADS) highlights_kernel(const Args a) {
  typedef typename OutType<OUT>::type TO;
  constexpr int LW = TILE_W + 2 * HALO_C;             // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO_R;
  __shared__ float xs[LH * LW];

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo, decoded once: x, or -inf for a tap that is outside the frame or a listed defect
  raw::stage_tile<SRC, TILE_H, TILE_W, HALO_R, HALO_C, THREADS>(a, fr.src, fr.mask, r0, c0, xs);
  __syncthreads();

  // 2. lane = tile column; the balance gains of the lane's own sites (ws) and of the other column parity (wo), per row parity
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  const bool cp = (lane & 1) != 0;                    // (c0 is even: the column parity)
  const float wR = a.wb_dev ? a.wb_dev[0] : a.wb[0];
  const float wG = a.wb_dev ? a.wb_dev[1] : a.wb[1];
  const float wB = a.wb_dev ? a.wb_dev[2] : a.wb[2];
  auto of = [&](int colour) { return colour == 0 ? wR : (colour == 1 ? wG : wB); };
  const float w0 = of(a.colour[0]), w1 = of(a.colour[1]), w2 = of(a.colour[2]), w3 = of(a.colour[3]);
  const float ws[2] = {cp ? w1 : w0, cp ? w3 : w2};
  const float wo[2] = {cp ? w0 : w1, cp ? w2 : w3};
  const bool green[2] = {(cp ? a.colour[1] : a.colour[0]) == 1, (cp ? a.colour[3] : a.colour[2]) == 1};
  const float t = a.t;
  const bool clip_mode = a.mode == MODE_CLIP;
  float lim[2] = {0.f, 0.f};
  if (clip_mode) {
    const float top = t * fminf(fminf(wR, wG), wB);
    lim[0] = top / ws[0];
    lim[1] = top / ws[1];
  }
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);

  for (int k2 = 0; k2 < PX / 2; ++k2) {
#pragma unroll
    for (int par = 0; par < 2; ++par) {               // (r0 and 16 wave are even: the row parity)
      const int tr = wave * PX + 2 * k2 + par;        // tile row
      const int r = r0 + tr;
      const bool inside = r < H && c < W;
      const float* row = &xs[(tr + HALO_R) * LW + lane + HALO_C];
      float xp = row[0];
      const bool listed = xp == -INFINITY && inside;
      if (listed) xp = raw::decode_one<SRC>(a, fr.src, r, c);      // a listed defect keeps its own value (rare)
      float y = xp;
      if (clip_mode) {
        y = (xp > lim[par] && !listed) ? lim[par] : xp;
      } else {
        const bool clipped = row[0] >= t;             // (an excluded centre is -inf, a NaN compares false)
        if (__builtin_amdgcn_ballot_w64(clipped) != 0) {
          if (clipped) {
            const bool g = green[par];
            const float wself = ws[par], wrow = wo[par], wcol = ws[par ^ 1], wdiag = wo[par ^ 1];
            const float up = row[-LW], dn = row[LW];
            // one straight line for both kinds of site (the lanes of a wave alternate between them).  Group A in the
            // order (r-1,c) (r,c-1) (r,c+1) (r+1,c): a G site keeps the row taps only.  Group B: the four diagonal taps,
            // or the column taps of a G site.
            Group A = {0.f, 0}, B = {0.f, 0};
            tap(A, g ? -INFINITY : up, wcol); tap(A, row[-1], wrow); tap(A, row[1], wrow); tap(A, g ? -INFINITY : dn, wcol);
            const float wb = g ? wcol : wdiag;
            tap(B, g ? up : row[-LW - 1], wb); tap(B, g ? dn : row[-LW + 1], wb);
            tap(B, g ? -INFINITY : row[LW - 1], wb); tap(B, g ? -INFINITY : row[LW + 1], wb);
            float e = 0.f;
            bool have = false;
            if (A.n) { e = A.S / (float)A.n; have = true; }
            if (B.n) {
              const float m = B.S / (float)B.n;
              e = have ? fmaxf(e, m) : m;
              have = true;
            }
            if (have && e > xp * wself) y = fmaxf(xp, e / wself);
          }
        }
      }
      if constexpr (OUT != OUT_PLAIN) {
        if (a.shading) y = y * shade_gain(a, r, c);   // (shade_axis clamps the pixel into the frame)
      }
      if (inside) dst[(size_t)r * W + c] = cast_out<TO>(y);
    }
  }
}

template <int SRC>
static int launch_src(const Args& a, int out, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  if (out == OUT_F16)
    hipLaunchKernelGGL((highlights_kernel<SRC, OUT_F16>), grid, dim3(THREADS), 0, stream, a);
  else if (out == OUT_F32)
    hipLaunchKernelGGL((highlights_kernel<SRC, OUT_F32>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((highlights_kernel<SRC, OUT_PLAIN>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int out, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, out, stream); });
}

}  // namespace hl
