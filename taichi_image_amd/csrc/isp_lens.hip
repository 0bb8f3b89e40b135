// Lens distortion correction kernels (isp_lens.h; the contract is DESIGN.md 3, "Lens distortion").
//
// Output pixel (r, c) of an Hd x Wd image at output scale (s0, s1) reads source coordinates (us, vs) of the H x W image:
// from the table, or from OpenCV's model with every step one f32 operation, rounded to nearest, left to right, none
// contracted (the build's -ffp-contract=off and the pragma below), divisions correctly rounded:
//   u = f32(c) / s1, v = f32(r) / s0;  x = (u - cx') * ifx', y = (v - cy') * ify';  r2 = x*x + y*y
//   num = 1 + r2*(k1 + r2*(k2 + r2*k3));  radial = num, or num / (1 + r2*(k4 + r2*(k5 + r2*k6))) (rational)
//   xd = x*radial + (2*p1)*x*y + p2*(r2 + 2*x*x);  yd = y*radial + p1*(r2 + 2*y*y) + (2*p2)*x*y
//   us = fx*xd + cx, vs = fy*yd + cy
// then samples it bilinearly as the resize does (interpolate.py:24-34): constant border 0 outside [0, H-1] x [0, W-1]
// (NaN included), or replicate (the coordinates clamped first; NaN clamps to 0); i = floor(vs), fr = vs - f32(i), the
// same for j, fc; taps i, i+1, j, j+1, the +1 taps clamped to the frame; rows mixed first, then columns, * intensity, cast.
//
// Consecutive lanes own consecutive output pixels of (mostly) one row: the taps of a wave fall in two or three nearby
// source rows served by L1 / L2.  (PX consecutive pixels per lane with vector stores spread each gather instruction over
// 4x the bytes and ran 1.5x slower: DESIGN.md 5.)  The analytic warp is ~25 VALU operations per pixel, cheaper than
// reading an 8-byte table entry, so it builds no table.
#include "isp_lens.h"

#pragma clang fp contract(off)

namespace lens {

// (us, vs) of output pixel (r, c) under the model; v is the row's f32(r) / s0
MI_DEV void warp(const Model& m, float u, float v, float& us, float& vs) {
  const float x = (u - m.ncx) * m.ifx, y = (v - m.ncy) * m.ify;
  const float r2 = x * x + y * y;
  const float num = 1.f + r2 * (m.k1 + r2 * (m.k2 + r2 * m.k3));
  const float radial = m.rational ? num / (1.f + r2 * (m.k4 + r2 * (m.k5 + r2 * m.k6))) : num;
  const float p1x2 = 2.f * m.p1, p2x2 = 2.f * m.p2;            // exact
  const float xd = x * radial + p1x2 * x * y + m.p2 * (r2 + 2.f * x * x);
  const float yd = y * radial + m.p1 * (r2 + 2.f * y * y) + p2x2 * x * y;
  us = m.fx * xd + m.cx;
  vs = m.fy * yd + m.cy;
}

// the bilinear sample at (us, vs), * intensity, before the cast
template <class TI, int BORDER>
MI_DEV void sample(const TI* __restrict__ src, int H, int W, float us, float vs, float intensity, float (&o)[3]) {
  const float hm = (float)(H - 1), wm = (float)(W - 1);
  if constexpr (BORDER == MI_BORDER_CONSTANT) {
    if (!(vs >= 0.f && vs <= hm && us >= 0.f && us <= wm)) {      // (false for NaN)
      o[0] = o[1] = o[2] = 0.f;
      return;
    }
  } else {
    vs = fminf(fmaxf(vs, 0.f), hm);                                 // fmaxf(NaN, 0) == 0
    us = fminf(fmaxf(us, 0.f), wm);
  }
  const int i = (int)vs, j = (int)us;                               // floor: both are >= 0 here
  const float fr = vs - (float)i, fc = us - (float)j;
  const int i1 = min(i + 1, H - 1), j1 = min(j + 1, W - 1);
  const TI* a = src + ((size_t)i * W + j) * 3;
  const TI* b = src + ((size_t)i1 * W + j) * 3;
  const TI* cc = src + ((size_t)i * W + j1) * 3;
  const TI* d = src + ((size_t)i1 * W + j1) * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float y1 = (float)a[ch] * (1.0f - fr) + (float)b[ch] * fr;
    const float y2 = (float)cc[ch] * (1.0f - fr) + (float)d[ch] * fr;
    o[ch] = (y1 * (1.0f - fc) + y2 * fc) * intensity;
  }
}

// grid (ceil(Hd * Wd / (THREADS * PX)), n_cams): block y is the frame.  Lane t of a block owns pixels base + k * THREADS
// + t: each gather instruction of a wave reads the taps of 64 consecutive output pixels (a few cache lines) and each store
// instruction writes 64 consecutive pixels' channel.
template <class TI, class TO, bool TABLE, int BORDER>
__global__ void __launch_bounds__(THREADS) remap_kernel(const Args a) {
  const Cam& cm = a.cam[blockIdx.y];                                // (a wave-uniform index: scalar loads)
  const uint32_t n = (uint32_t)a.Hd * (uint32_t)a.Wd;
  const uint32_t base = blockIdx.x * (THREADS * PX) + threadIdx.x;
  const TI* __restrict__ src = static_cast<const TI*>(cm.src);
  TO* __restrict__ dst = static_cast<TO*>(cm.dst);
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const uint32_t e = base + k * THREADS;
    if (e >= n) break;
    float us, vs;
    if constexpr (TABLE) {
      const float2 t = reinterpret_cast<const float2*>(cm.table)[e];
      us = t.x;
      vs = t.y;
    } else {
      const uint32_t r = e / (uint32_t)a.Wd, c = e - r * (uint32_t)a.Wd;
      warp(cm.m, (float)(int)c / a.s1, (float)(int)r / a.s0, us, vs);
    }
    float px[3];
    sample<TI, BORDER>(src, a.H, a.W, us, vs, a.intensity, px);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) dst[(size_t)e * 3 + ch] = cast_out<TO>(px[ch]);
  }
}

template <class F> static int dispatch(int dtype, F&& f) {
  switch (dtype) {
    case MI_U8: return f((uint8_t)0);
    case MI_U16: return f((uint16_t)0);
    case MI_F16: return f((half_t)0);
    default: return f((float)0);
  }
}

template <bool TABLE, int BORDER>
static int launch_form(const Args& a, int in_dtype, int out_dtype, hipStream_t stream) {
  const int64_t n = (int64_t)a.Hd * a.Wd;
  const dim3 grid((unsigned)((n + (int64_t)THREADS * PX - 1) / ((int64_t)THREADS * PX)), (unsigned)a.n_cams);
  return dispatch(in_dtype, [&](auto ti) {
    using TI = decltype(ti);
    return dispatch(out_dtype, [&](auto to) {
      using TO = decltype(to);
      hipLaunchKernelGGL((remap_kernel<TI, TO, TABLE, BORDER>), grid, dim3(THREADS), 0, stream, a);
      MI_LAUNCH_CHECK();
      return 0;
    });
  });
}

int launch(const Args& a, int in_dtype, int out_dtype, bool table, int border, hipStream_t stream) {
  if (a.n_cams <= 0 || (int64_t)a.Hd * a.Wd == 0) return 0;
  if (table)
    return border == MI_BORDER_CONSTANT ? launch_form<true, MI_BORDER_CONSTANT>(a, in_dtype, out_dtype, stream)
                                        : launch_form<true, MI_BORDER_REPLICATE>(a, in_dtype, out_dtype, stream);
  return border == MI_BORDER_CONSTANT ? launch_form<false, MI_BORDER_CONSTANT>(a, in_dtype, out_dtype, stream)
                                      : launch_form<false, MI_BORDER_REPLICATE>(a, in_dtype, out_dtype, stream);
}

}  // namespace lens
