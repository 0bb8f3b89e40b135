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

// x of raw pixels (r, c) and (r, c + 1), c even, row r inside the frame; two: c + 1 is inside the frame
template <int SRC>
MI_DEV void decode_pair(const Args& a, const void* src, int r, int c, bool two, float& x0, float& x1) {
  const bool odd = (r & 1) != 0;                     // (selects: a run-time index would put the arrays in scratch)
  const int b0 = odd ? a.black[2] : a.black[0], b1 = odd ? a.black[3] : a.black[1];
  const float k0 = odd ? a.k[2] : a.k[0], k1 = odd ? a.k[3] : a.k[1];
  if constexpr (SRC == SRC_P12 || SRC == SRC_P12_IDS) {
    const uint8_t* q = static_cast<const uint8_t*>(src) + (size_t)r * ((size_t)a.W * 3 / 2) + (size_t)(c >> 1) * 3;
    uint32_t p0, p1;
    tile::unpack_pair(q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), SRC == SRC_P12_IDS, p0, p1);
    x0 = tile::level_x(p0, b0, k0);
    x1 = tile::level_x(p1, b1, k1);
  } else if constexpr (SRC == SRC_P16) {
    const uint8_t* q = static_cast<const uint8_t*>(src) + ((size_t)r * a.W + c) * 2;
    x0 = tile::level_x(q[0] | ((uint32_t)q[1] << 8), b0, k0);
    x1 = two ? tile::level_x(q[2] | ((uint32_t)q[3] << 8), b1, k1) : 0.f;
  } else if constexpr (SRC == SRC_U16) {
    const uint16_t* q = static_cast<const uint16_t*>(src) + (size_t)r * a.W + c;
    const uint32_t v0 = q[0], v1 = two ? q[1] : 0u;
    if (a.levels) {                                   // load_u16_levels_kernel's quotient
      const int d0 = (int)v0 - b0, d1 = (int)v1 - b1;
      x0 = (float)(d0 > 0 ? d0 : 0) / k0;
      x1 = (float)(d1 > 0 ? d1 : 0) / k1;
    } else {                                          // load_convert_kernel's
      x0 = (float)v0 / 65535.0f;
      x1 = (float)v1 / 65535.0f;
    }
  } else if constexpr (SRC == SRC_U16F) {
    const uint16_t* q = static_cast<const uint16_t*>(src) + (size_t)r * a.W + c;
    x0 = (float)q[0];
    x1 = two ? (float)q[1] : 0.f;
  } else if constexpr (SRC == SRC_F32 || SRC == SRC_CFA_F32) {
    const float* q = static_cast<const float*>(src) + (size_t)r * a.W + c;
    x0 = q[0];
    x1 = two ? q[1] : 0.f;
  } else {
    const half_t* q = static_cast<const half_t*>(src) + (size_t)r * a.W + c;
    x0 = (float)q[0];
    x1 = two ? (float)q[1] : 0.f;
  }
}

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, class TO, int R>
__global__ void __launch_bounds__(THREADS) denoise_kernel(const Args a) {
  constexpr int HALO = 2 * R;
  constexpr int LW = TILE_W + 2 * HALO;               // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO;
  constexpr int LP = LW / 2;                          // column pairs per LDS row
  constexpr int N = 2 * R + 1;                        // window side
  __shared__ float xs[LH * LW];

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo, decoded once: x, or -inf for a tap that is outside the frame or a listed defect.  Pairs
  // start on even frame columns (c0 and HALO are even), so a pair's two sites and its mask bits are those of (c, c + 1).
  for (int u = threadIdx.x; u < LH * LP; u += THREADS) {
    const int lr = u / LP, lp = u - lr * LP;
    const int r = r0 - HALO + lr, c = c0 - HALO + 2 * lp;
    float x0 = -INFINITY, x1 = -INFINITY;
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const bool two = c + 1 < W;
      decode_pair<SRC>(a, fr.src, r, c, two, x0, x1);
      if (!two) x1 = -INFINITY;
      if (fr.mask) {
        const uint32_t m = fr.mask[(size_t)r * a.mask_w + (c >> 5)] >> (c & 31);
        if (m & 1u) x0 = -INFINITY;
        if (m & 2u) x1 = -INFINITY;
      }
    }
    *reinterpret_cast<float2*>(&xs[lr * LW + 2 * lp]) = make_float2(x0, x1);
  }
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
    if (xp == -INFINITY && inside) {                  // a listed defect is filtered with its own value (rare)
      float p0, p1;
      decode_pair<SRC>(a, fr.src, r, c & ~1, (c | 1) < W, p0, p1);
      xp = (c & 1) ? p1 : p0;
    }
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

template <int SRC>
static int launch_src(const Args& a, int work_dtype, int radius, hipStream_t stream) {
  return work_dtype == MI_F16 ? launch_r<SRC, half_t>(a, radius, stream) : launch_r<SRC, float>(a, radius, stream);
}

int launch(const Args& a, int src, int work_dtype, int radius, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  switch (src) {
    case SRC_P12: return launch_src<SRC_P12>(a, work_dtype, radius, stream);
    case SRC_P12_IDS: return launch_src<SRC_P12_IDS>(a, work_dtype, radius, stream);
    case SRC_P16: return launch_src<SRC_P16>(a, work_dtype, radius, stream);
    case SRC_U16: return launch_src<SRC_U16>(a, work_dtype, radius, stream);
    case SRC_U16F: return launch_src<SRC_U16F>(a, work_dtype, radius, stream);
    case SRC_F32: return launch_src<SRC_F32>(a, work_dtype, radius, stream);
    case SRC_CFA_F16: return launch_src<SRC_CFA_F16>(a, work_dtype, radius, stream);
    default: return launch_src<SRC_CFA_F32>(a, work_dtype, radius, stream);
  }
}

}  // namespace dn
