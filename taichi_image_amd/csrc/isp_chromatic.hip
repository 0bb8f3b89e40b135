// Lateral chromatic aberration kernels (isp_chromatic.h; the contract is DESIGN.md 3, "Chromatic aberration").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value and site s(p) = (r & 1) * 2 + (c & 1): a green
// site keeps y = x(p); a red or blue site of parity (r0, c0), whose site plane P has nr x nc cells, takes
//   dy = f32(r) - cy;  dx = f32(c) - cx;  q = (dx dx + dy dy) iR2;  e = d0 + q (d1 + q d2)      (d of its channel)
//   vs = f32(r) + dy e;  us = f32(c) + dx e;  a = (vs - f32(r0)) 0.5;  b = (us - f32(c0)) 0.5
//   i = floor(a), fr = a - i;  j = floor(b), fc = b - j;  rows i, i + 1 and columns j, j + 1 clamped into the plane
//   y = mix(mix(P00, P01, fc), mix(P10, P11, fc), fr),  mix(u, v, t) = u (1 - t) + v t
// or, when one of the four taps is a listed defect, the weighted mean N / S of the other taps (x(p) when S is not > 0);
//   cfa = cast_work(y * g(p))   (g the shading / AWB gain at p, 1 without a grid), or the plain f32 y.
// Every operation is one f32 rounding (no contraction, IEEE division): the output is the contract's bit for bit.
//
// One 256-thread block per 64 x 64 output tile of one frame (grid.z): the tile plus a halo of a.halo rows and columns (what
// the settings' largest shift on this frame needs, at most HALO: the decode front end is most of the kernel's time) is
// decoded ONCE into LDS as f32 x (a listed defect as -inf, pixels outside the frame as 0: the clamps keep every tap in the
// frame).  Lane l of wave w then takes column l of rows 16 w .. 16 w + 15, a row pair at a time: one of the pair's two
// pixels is the lane's red or blue one, which it resamples (its channel, row parity, dx and dx dx are fixed), the other its
// green one, which it copies; every lane runs the same straight line, no sample is computed and dropped.  The host bounds
// the shift by ca::MAX_SHIFT and sizes the halo by it, so every tap lies in the staged tile; the clamps of the tap indices
// are nevertheless taken against the staged cells too (the same instructions with other bounds), so no coefficient can
// index outside LDS.
#include "isp_chromatic.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace ca {

MI_DEV float mix(float u, float v, float omt, float t) { return u * omt + v * t; }

// the renormalised sums over the kept taps: each starts from its first kept term
struct Sums { float S, N; bool any; };
MI_DEV void tap(Sums& s, float w, float x) {
  if (x != -INFINITY) {                               // (a listed tap)
    const float wx = w * x;
    s.S = s.any ? s.S + w : w;
    s.N = s.any ? s.N + wx : wx;
    s.any = true;
  }
}

template <int OUT> struct OutType { typedef float type; };
template <> struct OutType<hl::OUT_F16> { typedef half_t type; };

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, int OUT>
__global__ void __launch_bounds__(THREADS) chromatic_kernel(const Args a) {
  typedef typename OutType<OUT>::type TO;
  constexpr int LW = TILE_W + 2 * HALO;               // LDS row pitch (floats), and the rows, of the largest halo
  constexpr int LH = TILE_H + 2 * HALO;
  __shared__ float xs[LH * LW];
  const int halo = a.halo;                            // (wave-uniform, even, 4 .. HALO)
  const int lp = (TILE_W + 2 * halo) / 2;             // staged column pairs per row = site-plane cells per row
  const int lq = (TILE_H + 2 * halo) / 2;             // staged site-plane cells per column

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo, decoded once: x, -inf for a listed defect, 0 outside the frame.  Pairs start on even frame
  // columns (c0 and halo are even), so a pair's two sites and its mask bits are those of (c, c + 1).
  const float inv_lp = 1.f / (float)lp;
  for (int u = threadIdx.x; u < 2 * lq * lp; u += THREADS) {
    const int lr = (int)(((float)u + 0.5f) * inv_lp), pr = u - lr * lp;     // (u / lp: exact for these few thousand)
    const int r = r0 - halo + lr, c = c0 - halo + 2 * pr;
    float x0 = 0.f, x1 = 0.f;
    if (r >= 0 && r < H && c >= 0 && c < W) {
      const bool two = c + 1 < W;
      raw::decode_pair<SRC>(a, fr.src, r, c, two, x0, x1);
      if (!two) x1 = 0.f;
      if (fr.mask) {
        const uint32_t m = fr.mask[(size_t)r * a.mask_w + (c >> 5)] >> (c & 31);
        if (m & 1u) x0 = -INFINITY;
        if ((m & 2u) && two) x1 = -INFINITY;
      }
    }
    *reinterpret_cast<float2*>(&xs[lr * LW + 2 * pr]) = make_float2(x0, x1);
  }
  __syncthreads();

  // 2. lane = tile column, rows in pairs.  Of the two pixels a lane holds in a row pair one is red or blue and one is green
  // (the tile origin and 16 w are even): the lane's channel, its d, its row parity ph and the clamps of its site plane are
  // fixed, so a lane resamples ONE pixel per row pair and copies the other; no lane computes a sample it throws away.
  // The site plane of parity (ph, cp) has cell (i, j) at LDS (ph + 2 (i - I0), cp + 2 (j - J0)); the tap indices are
  // clamped into the plane and into the staged cells at once.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  const bool cp = (lane & 1) != 0;                    // (c0 is even: the column parity)
  const int col_even = cp ? a.colour[1] : a.colour[0], col_odd = cp ? a.colour[3] : a.colour[2];
  const int ph = col_even == 1 ? 1 : 0;               // the row parity of the lane's red / blue site
  const bool blue = (ph ? col_odd : col_even) == 2;
  const float d0 = blue ? a.db[0] : a.dr[0], d1 = blue ? a.db[1] : a.dr[1], d2 = blue ? a.db[2] : a.dr[2];
  const int I0 = (r0 - halo) / 2, J0 = (c0 - halo) / 2;       // (both even numerators: exact)
  const int nr = (H - ph + 1) >> 1, nc = (W - (cp ? 1 : 0) + 1) >> 1;
  const float ilo = (float)(I0 > 0 ? I0 : 0), ihi = (float)(nr - 1 < I0 + lq - 1 ? nr - 1 : I0 + lq - 1);
  const float jlo = (float)(J0 > 0 ? J0 : 0), jhi = (float)(nc - 1 < J0 + lp - 1 ? nc - 1 : J0 + lp - 1);
  const float cy = a.cy, iR2 = a.iR2;
  const float fcol = (float)c, fcp = cp ? 1.f : 0.f, fph = (float)ph;
  const float dx = fcol - a.cx;
  const float dx2 = dx * dx;
  const bool inside = c < W;
  const float* plane = &xs[ph * LW + (cp ? 1 : 0)];  // cell (0, 0) of the staged part of the lane's site plane
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);

  for (int k2 = 0; k2 < PX / 2; ++k2) {
    const int tr = wave * PX + 2 * k2;                // the even tile row of the pair
    if (r0 + tr >= H) break;                          // (wave-uniform; no barrier follows)
    const int r = r0 + tr + ph, rg = r0 + tr + 1 - ph;     // the lane's red / blue pixel, its green pixel
    float xp = xs[(tr + ph + halo) * LW + lane + halo];
    float xg = xs[(tr + 1 - ph + halo) * LW + lane + halo];
    // the sampling position and the four taps
    const float frow = (float)r;
    const float dy = frow - cy;
    const float r2 = dx2 + dy * dy;
    const float q = r2 * iR2;
    const float e = d0 + q * (d1 + q * d2);
    const float vs = frow + dy * e, us = fcol + dx * e;
    const float av = (vs - fph) * 0.5f, bv = (us - fcp) * 0.5f;
    const float fi = floorf(av), fj = floorf(bv);
    const float tr_ = av - fi, tc_ = bv - fj;
    // (max last: a NaN, and an empty range, give the lower bound, which is always a staged cell)
    const int i0 = (int)fmaxf(fminf(fi, ihi), ilo) - I0;
    const int i1 = (int)fmaxf(fminf(fi + 1.f, ihi), ilo) - I0;
    const int j0 = (int)fmaxf(fminf(fj, jhi), jlo) - J0;
    const int j1 = (int)fmaxf(fminf(fj + 1.f, jhi), jlo) - J0;
    const float* row0 = plane + 2 * i0 * LW;
    const float* row1 = plane + 2 * i1 * LW;
    const float t00 = row0[2 * j0], t01 = row0[2 * j1], t10 = row1[2 * j0], t11 = row1[2 * j1];
    const float omr = 1.f - tr_, omc = 1.f - tc_;
    float y = mix(mix(t00, t01, omc, tc_), mix(t10, t11, omc, tc_), omr, tr_);
    // listed defects among the taps, or one of the lane's own pixels (rare): behind a wave-uniform branch
    const bool masked = t00 == -INFINITY || t01 == -INFINITY || t10 == -INFINITY || t11 == -INFINITY;
    const bool listed = xp == -INFINITY, listed_g = xg == -INFINITY;      // (only pixels inside the frame are listed)
    if (__builtin_amdgcn_ballot_w64(masked || listed || listed_g) != 0) {
      if (listed || listed_g) {                       // a listed pixel's own value, decoded again
        float p0, p1;
        raw::decode_pair<SRC>(a, fr.src, listed ? r : rg, c & ~1, (c | 1) < W, p0, p1);
        if (listed) xp = cp ? p1 : p0;
        if (listed && listed_g) raw::decode_pair<SRC>(a, fr.src, rg, c & ~1, (c | 1) < W, p0, p1);
        if (listed_g) xg = cp ? p1 : p0;
      }
      if (masked) {
        Sums s = {0.f, 0.f, false};
        tap(s, omr * omc, t00); tap(s, omr * tc_, t01); tap(s, tr_ * omc, t10); tap(s, tr_ * tc_, t11);
        y = (s.any && s.S > 0.f) ? s.N / s.S : xp;
      }
    }
    float yg = xg;
    if constexpr (OUT != hl::OUT_PLAIN) {
      if (a.shading) {                                // (the gain at p; shade_axis clamps the pixel into the frame)
        y = y * shade_gain(a, r, c);
        yg = yg * shade_gain(a, rg, c);
      }
    }
    // row by row, so that a wave's store covers 64 consecutive pixels
    const size_t o = (size_t)(r0 + tr) * W + c;
    if (inside) dst[o] = cast_out<TO>(ph ? yg : y);
    if (inside && r0 + tr + 1 < H) dst[o + W] = cast_out<TO>(ph ? y : yg);
  }
}

template <int SRC>
static int launch_src(const Args& a, int out, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  if (out == hl::OUT_F16)
    hipLaunchKernelGGL((chromatic_kernel<SRC, hl::OUT_F16>), grid, dim3(THREADS), 0, stream, a);
  else if (out == hl::OUT_F32)
    hipLaunchKernelGGL((chromatic_kernel<SRC, hl::OUT_F32>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((chromatic_kernel<SRC, hl::OUT_PLAIN>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int out, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, out, stream); });
}

}  // namespace ca
