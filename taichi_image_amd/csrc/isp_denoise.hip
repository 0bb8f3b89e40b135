// Raw noise reduction kernels (isp_denoise.h; the contract is DESIGN.md 3, "Raw noise reduction").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value and T(p) its same-site neighbours
// q = (r + 2i, c + 2j), |i|, |j| <= R, (i, j) != (0, 0), inside the frame and not in the defect mask:
//   var = gain * max(x(p), 0) + rn^2;  w(q) = exp(-(x(q) - x(p))^2 / (2 strength^2 var) - (i^2 + j^2) / (2 sigma^2))
//   y = (x(p) + sum w(q) x(q)) / (1 + sum w(q));  cfa = cast_work(y * g(p))   (g the shading / AWB gain, 1 without a grid)
// evaluated as y = x(p) - (sum w(q) (x(p) - x(q))) * rcp(1 + sum w(q)) with the hardware exp2 and rcp: within one unit of
// the work dtype of an f64 evaluation.  All off-centre weights 0 (spatial_sigma = 0.05) give y = x(p) bit for bit, so the
// output is then the loader's own cast_work(x(p) * g(p)).
//
// One 256-thread block per 64 x 64 output tile of one frame (grid.z): the tile plus a 2R-pixel halo is decoded ONCE into
// LDS as f32 x, excluded taps (outside the frame, or listed defects) as -inf.  Lane l of wave w then filters column l,
// rows (w >> 1) * 32 + (w & 1) + 2k, k < 16: same-site rows, so a (2R+1) x (2R+1) register window slides down the column
// and each step reads one new window row (2R+1 ds_read_b32, consecutive lanes on consecutive banks).  Per tap: a sub, a
// mul, an fma, one v_exp_f32, a min (an excluded tap's infinite difference times its zero weight must not give NaN), an
// fma and an add.  Per pixel: one v_rcp_f32 for k, one for the normalisation.
#include "isp_denoise.h"
#include "isp_tile.h"

#include <float.h>

#pragma clang fp contract(off)

namespace dn {

// keep a wave-uniform constant in a VGPR: a VALU instruction with an SGPR operand issues at half rate (isp_tile.h)
MI_DEV float in_vgpr(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, class TO, int R>
__global__ void __launch_bounds__(THREADS) denoise_kernel(const Args a) {
  constexpr int HALO = 2 * R;
  constexpr int LW = TILE_W + 2 * HALO;               // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO;
  constexpr int N = 2 * R + 1;                        // window side
  __shared__ float xs[LH * LW];

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo, decoded once: x, or -inf for a tap that is outside the frame or a listed defect
  raw::stage_tile<SRC, TILE_H, TILE_W, HALO, HALO, THREADS>(a, fr.src, fr.mask, r0, c0, xs);
  __syncthreads();

  // 2. the filter: lane = tile column, the wave's rows two apart
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rb = (wave >> 1) * (TILE_H / 2) + (wave & 1);   // first tile row of the wave
  const int c = c0 + lane;
  float nsp[9];                                       // -(i^2 + j^2) * log2(e) / (2 sigma^2), in VGPRs
#pragma unroll
  for (int d = 1; d < 9; ++d) nsp[d] = in_vgpr(-a.sp[d]);
  const float gain = a.gain, rn2 = a.rn2, c2 = a.c2;
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);

  float win[N][N];                                    // win[m][n] = x at tile row (row of the pixel) + 2 (m - R),
  auto load_row = [&](float(&row)[N], int lr) {       //   tile column lane + 2 (n - R)
#pragma unroll
    for (int n = 0; n < N; ++n) row[n] = xs[lr * LW + lane + 2 * n];
  };
#pragma unroll
  for (int m = 0; m < N - 1; ++m) load_row(win[m], rb + 2 * m);
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    load_row(win[N - 1], rb + 2 * (k + N - 1));
    const int r = r0 + rb + 2 * k;
    const bool inside = r < H && c < W;
    float xp = win[R][R];
    // a listed defect is filtered with its own value (rare)
    if (xp == -INFINITY && inside) xp = raw::decode_one<SRC>(a, fr.src, r, c);
    const float var = __builtin_fmaf(gain, fmaxf(xp, 0.f), rn2);
    const float nkl = -fminf(c2 * __builtin_amdgcn_rcpf(var), FLT_MAX);   // (var 0: k = FLT_MAX, not inf * 0)
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int i = -R; i <= R; ++i)
#pragma unroll
      for (int j = -R; j <= R; ++j) {
        if (i == 0 && j == 0) continue;
        const float d = xp - win[i + R][j + R];
        const float w = __builtin_amdgcn_exp2f(__builtin_fmaf(d * d, nkl, nsp[i * i + j * j]));
        num = __builtin_fmaf(w, fminf(d, FLT_MAX), num);                   // (an excluded tap: 0 * FLT_MAX)
        den = den + w;
      }
    // (num is +0 when every weight is 0, and xp - +0 == xp for every xp, -0 included)
    float y = xp - num * __builtin_amdgcn_rcpf(1.f + den);
    if (a.shading) y = y * shade_gain(a, r, c);       // (shade_axis clamps the pixel into the frame)
    if (inside) dst[(size_t)r * W + c] = cast_out<TO>(y);
#pragma unroll
    for (int m = 0; m < N - 1; ++m)
#pragma unroll
      for (int n = 0; n < N; ++n) win[m][n] = win[m + 1][n];
  }
}

template <int SRC, class TO>
static int launch_r(const Args& a, int radius, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  if (radius == 1)
    hipLaunchKernelGGL((denoise_kernel<SRC, TO, 1>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((denoise_kernel<SRC, TO, 2>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int work_dtype, int radius, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) {
    constexpr int SRC = decltype(s)::value;
    return work_dtype == MI_F16 ? launch_r<SRC, half_t>(a, radius, stream) : launch_r<SRC, float>(a, radius, stream);
  });
}

}  // namespace dn
