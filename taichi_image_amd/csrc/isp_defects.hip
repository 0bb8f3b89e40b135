// Defective pixel correction kernels (isp_defects.h; the contract is DESIGN.md 3, "Defective pixels").
//
// Corrected value of a defective raw site (r, c), x(q) the work-dtype value the loader gives pixel q:
//   kept = [(r-2,c), (r+2,c), (r,c-2), (r,c+2)] inside the frame and not defective; if empty, the four diagonals at
//   distance 2 under the same rule; y = cast_E(((x1 + x2) + x3 + x4) / f32(n)), or x(r, c) itself when n == 0.
// Only non-defective values are read, so the result does not depend on the order of the corrections.
//
// Every operation below is one f32 rounding, none contracted, divisions correctly rounded: the demosaic is the oracle's
// (tap order of bayer.py:15-27, c / t with t the in-bounds weight sum, ccm as a sequential dot, clamp, cast) and the
// bilinear mix is interpolate.py:24-34 on the work-dtype full-resolution values.
#include "isp_defects.h"

#pragma clang fp contract(off)

namespace dfx {

MI_DEV bool is_defect(const uint32_t* mask, int mask_w, int r, int c) {
  return ((mask[(size_t)r * mask_w + (c >> 5)] >> (c & 31)) & 1u) != 0;
}

// (selects, no run-time index into the parameter arrays: that would send them through scratch)
MI_DEV int site_black(const tile::Params& p, int s) {
  return s == 0 ? p.lv_black[0] : s == 1 ? p.lv_black[1] : s == 2 ? p.lv_black[2] : p.lv_black[3];
}
MI_DEV float site_k(const tile::Params& p, int s) {
  return s == 0 ? p.lv_k[0] : s == 1 ? p.lv_k[1] : s == 2 ? p.lv_k[2] : p.lv_k[3];
}

// x(r, c) of a packed frame: the code, its levels (black 0 and k_decode without levels: the plain decode), the lens
// shading gain, rounded to E and widened back - the value the load kernels stage for the demosaic
template <class E> MI_DEV float packed_x(const tile::Params& p, const uint8_t* src, int r, int c) {
  uint32_t v;
  if (p.src_kind == tile::SRC_PACKED16) {
    const uint8_t* q = src + ((size_t)r * p.W + c) * 2;
    v = q[0] | ((uint32_t)q[1] << 8);
  } else {
    const uint8_t* q = src + (size_t)r * ((size_t)p.W * 3 / 2) + (size_t)(c >> 1) * 3;
    uint32_t p0, p1;
    tile::unpack_pair(q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16), p.src_kind == tile::SRC_PACKED12_IDS, p0, p1);
    v = (c & 1) ? p1 : p0;
  }
  const int s = (r & 1) * 2 + (c & 1);
  float x = tile::level_x(v, site_black(p, s), site_k(p, s));
  if (p.shading) x = x * shade_gain(p, r, c);
  return (float)cast_out<E>(x);
}

// the candidate offsets of the contract: axial first, then diagonal
__device__ constexpr int8_t CAND_DR[8] = {-2, 2, 0, 0, -2, -2, 2, 2};
__device__ constexpr int8_t CAND_DC[8] = {0, 0, -2, 2, -2, 2, -2, 2};

// y(r, c) of an in-frame site: x itself, or the correction of a defective site; X(r, c) gives x
template <class E, class X>
MI_DEV float corrected(int H, int W, const uint32_t* mask, int mask_w, int r, int c, X&& x) {
  if (!is_defect(mask, mask_w, r, c)) return x(r, c);
  float sum = 0.f;
  int n = 0;
  for (int set = 0; set < 2 && n == 0; ++set)
    for (int k = 4 * set; k < 4 * set + 4; ++k) {
      const int rr = r + CAND_DR[k], cc = c + CAND_DC[k];
      if (rr < 0 || rr >= H || cc < 0 || cc >= W || is_defect(mask, mask_w, rr, cc)) continue;
      sum = sum + x(rr, cc);
      ++n;
    }
  if (n == 0) return x(r, c);
  return (float)cast_out<E>(sum / (float)n);
}

// the demosaiced, colour-corrected, clamped pixel (r, c) of the corrected CFA (bayer.py:138-155), before the cast
template <class E>
MI_DEV void demosaic_px(const Args& a, const Cam& cm, int r, int c, float (&o)[3]) {
  const tile::Params& p = a.t;
  const int K = ((r + a.pr) & 1) + 2 * ((c + a.pc) & 1);
  auto x = [&](int rr, int cc) { return packed_x<E>(p, cm.src, rr, cc); };
  float acc[3] = {0.f, 0.f, 0.f};
  int t[3] = {0, 0, 0};
  for (int tap = 0; tap < 13; ++tap) {
    const int rr = r + tile::TAP_DR[tap], cc = c + tile::TAP_DC[tap];
    if (rr < 0 || rr >= p.H || cc < 0 || cc >= p.W) continue;     // the zero padding adds 0 * w: no change
    const float v = corrected<E>(p.H, p.W, cm.mask, a.mask_w, rr, cc, x);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int w = tile::KW[K][tap][ch];
      if (w != 0) {
        acc[ch] = acc[ch] + v * (float)w;
        t[ch] += w;
      }
    }
  }
  float d[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) d[ch] = acc[ch] / (float)t[ch];    // in_scale 1: the decoded CFA is f16 / f32
  if (p.has_ccm) {
    const float r0 = d[0], g0 = d[1], b0 = d[2];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) d[ch] = (p.ccm[3 * ch] * r0 + p.ccm[3 * ch + 1] * g0) + p.ccm[3 * ch + 2] * b0;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch] = fminf(fmaxf(d[ch], 0.f), 1.f);
}

// one lane per listed output pixel of every camera of the launch
template <class E>
__global__ void __launch_bounds__(THREADS) fix_packed_kernel(const Args a) {
  const int g = blockIdx.x * THREADS + threadIdx.x;
  if (g >= a.total) return;
  // the lane's camera, every index static (a run-time index into the argument block would copy it to scratch)
  Cam cm = a.cam[0];
#pragma unroll
  for (int k = 1; k < MAX_CAMS; ++k)
    if (k < a.n_cams && g >= a.cam[k].start) cm = a.cam[k];
  const int e = cm.list[g - cm.start];
  if (e < 0 || e >= a.Hd * a.Wd) return;                          // (a list built for another geometry)
  const int i = e / a.Wd, j = e - i * a.Wd;
  const tile::Params& p = a.t;
  float o[3];
  if (!a.resize) {
    float v[3];
    demosaic_px<E>(a, cm, i, j, v);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch] = v[ch];
  } else {
    // sample_bilinear (interpolate.py:24-34): p = (i / s, j / s), taps clamped into the frame, rows mixed first
    const float pr = (float)i / a.s, pc = (float)j / a.s;
    const int ir = (int)pr, ic = (int)pc;
    const float fr = pr - (float)ir, fc = pc - (float)ic;
    const int ra = min(ir, p.H - 1), rb = min(ir + 1, p.H - 1);
    const int ca = min(ic, p.W - 1), cb = min(ic + 1, p.W - 1);
    float q00[3], q10[3], q01[3], q11[3];
    demosaic_px<E>(a, cm, ra, ca, q00);
    demosaic_px<E>(a, cm, rb, ca, q10);
    demosaic_px<E>(a, cm, ra, cb, q01);
    demosaic_px<E>(a, cm, rb, cb, q11);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      // the reference stores the full-resolution RGB in the work dtype before resizing
      const float v00 = (float)cast_out<E>(q00[ch]), v10 = (float)cast_out<E>(q10[ch]);
      const float v01 = (float)cast_out<E>(q01[ch]), v11 = (float)cast_out<E>(q11[ch]);
      const float y1 = v00 * (1.0f - fr) + v10 * fr;
      const float y2 = v01 * (1.0f - fr) + v11 * fr;
      o[ch] = y1 * (1.0f - fc) + y2 * fc;                          // intensity 1 (same dtype)
    }
  }
  E* dst = static_cast<E*>(cm.dst) + (size_t)e * 3;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) dst[ch] = cast_out<E>(o[ch]);
  if (cm.sub && i % a.st == 0 && j % a.st == 0) {
    E* s = static_cast<E*>(cm.sub) + ((size_t)(i / a.st) * a.sub_w + j / a.st) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s[ch] = cast_out<E>(o[ch]);
  }
}

// the convert route: one lane per defective site, in place (writes only sites in D, reads only sites outside it)
template <class E>
__global__ void __launch_bounds__(THREADS) fix_cfa_kernel(E* cfa, int H, int W, const int32_t* coords, int n,
                                                          const uint32_t* mask, int mask_w) {
  const int g = blockIdx.x * THREADS + threadIdx.x;
  if (g >= n) return;
  const int r = coords[2 * g], c = coords[2 * g + 1];
  if (r < 0 || r >= H || c < 0 || c >= W) return;
  auto x = [&](int rr, int cc) { return (float)cfa[(size_t)rr * W + cc]; };
  const float y = corrected<E>(H, W, mask, mask_w, r, c, x);
  cfa[(size_t)r * W + c] = cast_out<E>(y);
}

int launch_packed(const Args& a, int work_dtype, hipStream_t stream) {
  if (a.total <= 0) return 0;
  const dim3 grid((unsigned)((a.total + THREADS - 1) / THREADS));
  if (work_dtype == MI_F16)
    hipLaunchKernelGGL(fix_packed_kernel<half_t>, grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(fix_packed_kernel<float>, grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch_cfa(void* cfa, int H, int W, int work_dtype, const int32_t* coords, int n, const uint32_t* mask,
               hipStream_t stream) {
  if (n <= 0) return 0;
  const dim3 grid((unsigned)((n + THREADS - 1) / THREADS));
  const int mask_w = (W + 31) / 32;
  if (work_dtype == MI_F16)
    hipLaunchKernelGGL(fix_cfa_kernel<half_t>, grid, dim3(THREADS), 0, stream, static_cast<half_t*>(cfa), H, W, coords, n,
                       mask, mask_w);
  else
    hipLaunchKernelGGL(fix_cfa_kernel<float>, grid, dim3(THREADS), 0, stream, static_cast<float*>(cfa), H, W, coords, n,
                       mask, mask_w);
  MI_LAUNCH_CHECK();
  return 0;
}

}  // namespace dfx
