// Temporal noise reduction kernels (isp_temporal.h; the contract is DESIGN.md 3, "Temporal noise reduction").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value, h(p) the history plane (the previous y) and T(p)
// its 3 x 3 same-site window q = (r + 2i, c + 2j), |i|, |j| <= 1, inside the frame and not in the defect mask, in the
// order i = -1, 0, 1 and within a row j = -1, 0, 1, n = |T(p)|:
//   D = sum over T(p) of |x(q) - h(q)|;  m = D * R[n]  (R[n] = f32(1 / n));  var = gain * max(h(p), 0) + rn2
//   qv = (m * m) / (c * var);  k = max(1 - qv, 0);  w = wmax * k
//   y = x(p) when n == 0 or w == 0 (selected), else x(p) + w * (h(p) - x(p));  h'(p) = y;  cfa = cast_work(y * g(p))
// Every operation is one f32 rounding (no contraction, an IEEE division): the output is the contract's bit for bit.  A
// frame without a history gives y = x.  (|x - h| >= +0 and the sum starts at +0, so adding +0 for an excluded tap leaves
// the sum of the kept terms, started from the first of them, unchanged: the sum is branch-free.)
//
// One 256-thread block per 64 x 64 output tile of one frame (grid.z): the tile plus a 2-pixel halo of x is decoded ONCE
// into LDS as f32, excluded taps (outside the frame, or listed defects) as -inf, and the same cells of h are staged beside
// it.  Lane l of wave w then takes column l, rows (w >> 1) * 32 + (w & 1) + 2k, k < 16: same-site rows, so a 3 x 3
// register window of |x - h| slides down the column and each step reads one new window row (3 + 3 ds_read_b32,
// consecutive lanes on consecutive banks).  Per pixel: 9 adds and 9 maxes for D, 9 compare-and-counts for n, one LDS
// read for R[n], five multiplies, one division, and the blend.
#include "isp_temporal.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace tn {

template <int OUT> struct OutType { typedef float type; };
template <> struct OutType<OUT_F16> { typedef half_t type; };

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, int OUT>
__global__ void __launch_bounds__(THREADS) temporal_kernel(const Args a) {
  typedef typename OutType<OUT>::type TO;
  constexpr int LW = TILE_W + 2 * HALO;               // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO;
  constexpr int LP = LW / 2;                          // column pairs per LDS row
  __shared__ float xs[LH * LW];
  __shared__ float hs[LH * LW];
  __shared__ float rcp_n[16];

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;
  const float* __restrict__ hin = fr.hist_in;         // (NULL: an empty history, uniform over the block)

  // 1. the tile and its halo, decoded once: x, or -inf for a tap that is outside the frame or a listed defect, and h of
  // the same cells.  Pairs start on even frame columns (c0 and HALO are even), so a pair's two sites and its mask bits
  // are those of (c, c + 1).
  if (threadIdx.x == 0) {                             // (constant indices: a run-time one would put the table in scratch)
#pragma unroll
    for (int i = 0; i < 10; ++i) rcp_n[i] = a.rcp_n[i];
  }
  for (int u = threadIdx.x; u < LH * LP; u += THREADS) {
    const int lr = u / LP, lp = u - lr * LP;
    const int r = r0 - HALO + lr, c = c0 - HALO + 2 * lp;
    float x0 = -INFINITY, x1 = -INFINITY, h0 = 0.f, h1 = 0.f;
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const bool two = c + 1 < W;
      raw::decode_pair<SRC>(a, fr.src, r, c, two, x0, x1);
      if (!two) x1 = -INFINITY;
      if (hin) {
        const float* q = hin + (size_t)r * W + c;
        h0 = q[0];
        h1 = two ? q[1] : 0.f;
      }
      if (fr.mask) {
        const uint32_t m = fr.mask[(size_t)r * a.mask_w + (c >> 5)] >> (c & 31);
        if (m & 1u) x0 = -INFINITY;
        if (m & 2u) x1 = -INFINITY;
      }
    }
    *reinterpret_cast<float2*>(&xs[lr * LW + 2 * lp]) = make_float2(x0, x1);
    if (hin) *reinterpret_cast<float2*>(&hs[lr * LW + 2 * lp]) = make_float2(h0, h1);
  }
  __syncthreads();

  // 2. the blend: lane = tile column, the wave's rows two apart
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rb = (wave >> 1) * (TILE_H / 2) + (wave & 1);   // first tile row of the wave
  const int c = c0 + lane;
  const float gain = a.gain, rn2 = a.rn2, cc = a.c, wmax = a.wmax;
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);
  float* __restrict__ hout = fr.hist_out;

  auto finish = [&](int r, bool inside, float y) {    // h' = y; cfa = cast_work(y * g)
    if (inside) hout[(size_t)r * W + c] = y;
    if constexpr (OUT != OUT_PLAIN) {
      if (a.shading) y = y * shade_gain(a, r, c);     // (shade_axis clamps the pixel into the frame)
      if (inside) dst[(size_t)r * W + c] = cast_out<TO>(y);
    }
  };
  auto own_x = [&](float xp, int r, bool inside) {    // a listed defect is filtered with its own value (rare)
    return (xp == -INFINITY && inside) ? raw::decode_one<SRC>(a, fr.src, r, c) : xp;
  };

  if (!hin) {                                         // an empty history: y = x
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      const int r = r0 + rb + 2 * k;
      const bool inside = r < H && c < W;
      finish(r, inside, own_x(xs[(rb + 2 * k + HALO) * LW + lane + HALO], r, inside));
    }
    return;
  }

  float win[3][3];                                    // win[m][n] = |x - h| at tile row (row of the pixel) + 2 (m - 1),
  float cx[3], ch[3];                                 //   tile column lane + 2 (n - 1), -1 for an excluded tap; cx, ch: x
  auto load_row = [&](int m, int lr) {                //   and h of the window rows' centre column
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const float x = xs[lr * LW + lane + 2 * n], h = hs[lr * LW + lane + 2 * n];
      win[m][n] = x == -INFINITY ? -1.f : fabsf(x - h);
      if (n == 1) { cx[m] = x; ch[m] = h; }
    }
  };
  load_row(0, rb);
  load_row(1, rb + 2);
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    load_row(2, rb + 2 * (k + 2));
    const int r = r0 + rb + 2 * k;
    const bool inside = r < H && c < W;
    const float xp = own_x(cx[1], r, inside), hp = ch[1];
    float D = 0.f;
    int n = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        D = D + fmaxf(win[i][j], 0.f);                // (an excluded tap adds +0: see the head of the file)
        n += win[i][j] >= 0.f ? 1 : 0;
      }
    const float m = D * rcp_n[n];
    const float var = gain * fmaxf(hp, 0.f) + rn2;
    const float qv = (m * m) / (cc * var);
    const float kk = fmaxf(1.f - qv, 0.f);
    const float w = wmax * kk;
    const float t = w * (hp - xp);
    const float y = (n == 0 || w == 0.f) ? xp : xp + t;
    finish(r, inside, y);
#pragma unroll
    for (int n2 = 0; n2 < 3; ++n2) {
      win[0][n2] = win[1][n2];
      win[1][n2] = win[2][n2];
    }
    cx[0] = cx[1]; cx[1] = cx[2];
    ch[0] = ch[1]; ch[1] = ch[2];
  }
}

template <int SRC>
static int launch_src(const Args& a, int out, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  if (out == OUT_F16)
    hipLaunchKernelGGL((temporal_kernel<SRC, OUT_F16>), grid, dim3(THREADS), 0, stream, a);
  else if (out == OUT_F32)
    hipLaunchKernelGGL((temporal_kernel<SRC, OUT_F32>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((temporal_kernel<SRC, OUT_PLAIN>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int out, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, out, stream); });
}

}  // namespace tn
