// Exposure merge kernels (isp_exposure_merge.h; the contract is DESIGN.md 3, "Exposure merge").
//
// For raw pixel p = (r, c), x_e(p) the f32 pre-shading, pre-cast value of frame e (e = 0 the shortest exposure) and T(p)
// its 3 x 3 same-site window q = (r + 2i, c + 2j), |i|, |j| <= 1, inside the frame and not in the defect mask, in the
// order i = -1, 0, 1 and within a row j = -1, 0, 1, n = |T(p)|:
//   s0 = x_0(p);  v0 = gain * max(s0, 0) + rn2;  a0 = 1 / v0;  num = a0 * s0;  den = a0
//   for e = 1 .. E - 1:  se(q) = x_e(q) * inv_e;  D = sum over T(p) of |se(q) - x_0(q)|;  m = D * R[n]
//     ve = (gain * max(x_e(p), 0) + rn2) * i2_e;  qv = (m * m) / (c * (v0 + ve));  k = max(1 - qv, 0)
//     u = min(max((sat - x_e(p)) * rf, 0), 1);  w = (u * k) / ve;  if w > 0: num = num + w * se(p), den = den + w
//   y = x_0(p) when n == 0 or no frame was used (selected), else num / den;  cfa = cast_work(y * g(p))
// Every operation is one f32 rounding (no contraction, IEEE divisions): the output is the contract's bit for bit.
// (|se - x_0| >= +0 and the sum starts at +0, so adding +0 for an excluded tap leaves the sum of the kept terms, started
// from the first of them, unchanged: the sum is branch-free.)
//
// One 256-thread block per 64 x 64 output tile of one bracket (grid.z): the tile plus a 2-pixel halo of x_0 is decoded
// ONCE into LDS as f32, excluded taps (outside the frame, or listed defects) as -inf.  Then, one long frame after the
// other with a barrier between, the same cells of x_e are decoded into a second plane (LDS does not grow with E) and
// every lane updates the num, den and used bit of its pixels, which stay in registers.  A lane owns a column pair: lane
// l of wave w takes tile columns 2 (l & 31), + 1 and rows 16 w + (l >> 5) + 2k, k < 8: same-site rows, so a 3 x 6
// register window of |se - x_0| slides down the pair and each step reads one new window row (3 + 3 ds_read_b64), and a
// wave's step stores two whole tile rows, 4 (f16) or 8 (f32) bytes per lane.
#include "isp_exposure_merge.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace em {

template <int OUT> struct OutType { typedef float type; };
template <> struct OutType<OUT_F16> { typedef half_t type; };
template <class T> struct alignas(2 * sizeof(T)) Pair { T v[2]; };

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_brackets)
template <int SRC, int OUT>
__global__ void __launch_bounds__(THREADS) merge_kernel(const Args a) {
  typedef typename OutType<OUT>::type TO;
  constexpr int LW = TILE_W + 2 * HALO;               // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO;
  constexpr int LP = LW / 2;                          // column pairs per LDS row
  __shared__ float xs[LH * LW];                       // x_0, or -inf for an excluded tap
  __shared__ float ls[LH * LW];                       // x_e of the long frame at hand (0 outside the frame)
  __shared__ float rcp_n[16];

  const Bracket& br = a.b[blockIdx.z];                // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo of the shortest frame, decoded once: x_0, or -inf for a tap that is outside the frame or a
  // listed defect
  if (threadIdx.x == 0) {                             // (constant indices: a run-time one would put the table in scratch)
#pragma unroll
    for (int i = 0; i < 10; ++i) rcp_n[i] = a.rcp_n[i];
  }
  raw::stage_tile<SRC, TILE_H, TILE_W, HALO, HALO, THREADS>(a, br.src[0], br.mask, r0, c0, xs);
  __syncthreads();

  // 2. the lane's pixels: a column pair, rows two apart
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lp = lane & 31;                           // the tile's column pair
  const int rb = wave * (2 * PX) + (lane >> 5);       // first tile row of the lane
  const int c = c0 + 2 * lp;                          // (even)
  const bool in0 = c < W, in1 = c + 1 < W;
  const float gain = a.gain, rn2 = a.rn2, cc = a.c, sat = a.sat, rf = a.rf;

  // x_0 of the lane's pair in row r, from its LDS cells: a listed defect is merged from its own values (rare)
  auto own = [&](float& p0, float& p1, int r) {
    if ((p0 == -INFINITY || p1 == -INFINITY) && r < H && in0) {
      float d0, d1;
      raw::decode_pair<SRC>(a, br.src[0], r, c, in1, d0, d1);
      if (p0 == -INFINITY) p0 = d0;
      if (p1 == -INFINITY) p1 = d1;
    }
  };
  float num[PX][2], den[PX][2];                       // (constant indices throughout: registers; x_0 and v0 are not
  uint32_t used = 0;                                  //  kept: each frame's window reads x_0 again)
#pragma unroll                                        // used, bit 2k + t: some long frame entered pixel t of row k
  for (int k = 0; k < PX; ++k) {
    const float2 v = *reinterpret_cast<const float2*>(&xs[(rb + 2 * k + HALO) * LW + 2 * lp + HALO]);
    float s0[2] = {v.x, v.y};
    own(s0[0], s0[1], r0 + rb + 2 * k);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float v0 = gain * fmaxf(s0[t], 0.f) + rn2;
      const float a0 = 1.f / v0;
      num[k][t] = a0 * s0[t];
      den[k][t] = a0;
    }
  }

  // 3. one long frame after the other
  for (int e = 1; e < a.E; ++e) {                     // (wave-uniform)
    const float inv = e == 1 ? a.inv[1] : (e == 2 ? a.inv[2] : a.inv[3]);      // (selects, as in decode_pair)
    const float i2 = e == 1 ? a.i2[1] : (e == 2 ? a.i2[2] : a.i2[3]);
    const void* src = e == 1 ? br.src[1] : (e == 2 ? br.src[2] : br.src[3]);
    __syncthreads();                                  // (the plane of the frame before has been read)
    for (int u = threadIdx.x; u < LH * LP; u += THREADS) {
      const int lr = u / LP, p = u - lr * LP;
      const int r = r0 - HALO + lr, cq = c0 - HALO + 2 * p;
      float x0 = 0.f, x1 = 0.f;
      if (r >= 0 && r < H && cq >= 0 && cq < W) raw::decode_pair<SRC>(a, src, r, cq, cq + 1 < W, x0, x1);
      *reinterpret_cast<float2*>(&ls[lr * LW + 2 * p]) = make_float2(x0, x1);
    }
    __syncthreads();

    const float* xw = xs;                             // (laundered per frame: x_0's window is loop-invariant, and hoisted
    asm volatile("" : "+v"(xw));                      //  out of the loop it would hold 60 registers across the decode)
    float win[3][6];                                  // win[m][n] = |se - x_0| at tile row (row of the pixels) + 2 (m - 1),
    float cl[3][2], cx[3][2];                         //   LDS column 2 lp + n, -1 for an excluded tap; cl, cx: x_e and x_0
    auto load_row = [&](int m, int lr) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float2 x = *reinterpret_cast<const float2*>(&xw[lr * LW + 2 * lp + 2 * j]);
        const float2 l = *reinterpret_cast<const float2*>(&ls[lr * LW + 2 * lp + 2 * j]);
        win[m][2 * j] = x.x == -INFINITY ? -1.f : fabsf(l.x * inv - x.x);
        win[m][2 * j + 1] = x.y == -INFINITY ? -1.f : fabsf(l.y * inv - x.y);
        if (j == 1) { cl[m][0] = l.x; cl[m][1] = l.y; cx[m][0] = x.x; cx[m][1] = x.y; }
      }
    };
    load_row(0, rb);
    load_row(1, rb + 2);
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      load_row(2, rb + 2 * (k + 2));
      float s0[2] = {cx[1][0], cx[1][1]};
      own(s0[0], s0[1], r0 + rb + 2 * k);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float D = 0.f;
        int n = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            D = D + fmaxf(win[i][t + 2 * j], 0.f);    // (an excluded tap adds +0: see the head of the file)
            n += win[i][t + 2 * j] >= 0.f ? 1 : 0;
          }
        const float xe = cl[1][t];
        const float m = D * rcp_n[n];
        const float v0 = gain * fmaxf(s0[t], 0.f) + rn2;
        const float ve = (gain * fmaxf(xe, 0.f) + rn2) * i2;
        const float qv = (m * m) / (cc * (v0 + ve));
        const float kk = fmaxf(1.f - qv, 0.f);
        const float uu = fminf(fmaxf((sat - xe) * rf, 0.f), 1.f);
        const float w = (uu * kk) / ve;
        const float ws = w * (xe * inv);
        const bool take = w > 0.f && n > 0;           // (n == 0: y = x_0 whatever the weights)
        num[k][t] = take ? num[k][t] + ws : num[k][t];
        den[k][t] = take ? den[k][t] + w : den[k][t];
        used |= take ? 1u << (2 * k + t) : 0u;
        asm volatile("" : "+v"(num[k][t]), "+v"(den[k][t]));       // (pinned here: sunk to their use after the loop, every
                                                                    //  row's window would be live at once)
      }
#pragma unroll
      for (int n2 = 0; n2 < 6; ++n2) {
        win[0][n2] = win[1][n2];
        win[1][n2] = win[2][n2];
      }
      cl[0][0] = cl[1][0]; cl[0][1] = cl[1][1];
      cl[1][0] = cl[2][0]; cl[1][1] = cl[2][1];
      cx[0][0] = cx[1][0]; cx[0][1] = cx[1][1];
      cx[1][0] = cx[2][0]; cx[1][1] = cx[2][1];
    }
  }

  // 4. y, the gain and the cast: a pair per lane and row, in one store where the row pitch and the pointer allow it
  TO* __restrict__ dst = static_cast<TO*>(br.dst);
  const bool wide = (W & 1) == 0 && (reinterpret_cast<uintptr_t>(dst) & (2 * sizeof(TO) - 1)) == 0;
#pragma unroll
  for (int k = 0; k < PX; ++k) {
    const int r = r0 + rb + 2 * k;
    const float2 v = *reinterpret_cast<const float2*>(&xs[(rb + 2 * k + HALO) * LW + 2 * lp + HALO]);
    float s0[2] = {v.x, v.y};
    own(s0[0], s0[1], r);
    float y0 = (used >> (2 * k)) & 1u ? num[k][0] / den[k][0] : s0[0];
    float y1 = (used >> (2 * k + 1)) & 1u ? num[k][1] / den[k][1] : s0[1];
    if constexpr (OUT != OUT_PLAIN) {
      if (a.shading) {                                // (shade_axis clamps the pixel into the frame)
        y0 = y0 * shade_gain(a, r, c);
        y1 = y1 * shade_gain(a, r, c + 1);
      }
    }
    if (r < H && in0) {
      TO* q = dst + (size_t)r * W + c;
      if (wide) {                                     // (W even: c + 1 is inside the frame)
        Pair<TO> o;
        o.v[0] = cast_out<TO>(y0);
        o.v[1] = cast_out<TO>(y1);
        *reinterpret_cast<Pair<TO>*>(q) = o;
      } else {
        q[0] = cast_out<TO>(y0);
        if (in1) q[1] = cast_out<TO>(y1);
      }
    }
  }
}

template <int SRC>
static int launch_src(const Args& a, int out, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_brackets);
  if (out == OUT_F16)
    hipLaunchKernelGGL((merge_kernel<SRC, OUT_F16>), grid, dim3(THREADS), 0, stream, a);
  else if (out == OUT_F32)
    hipLaunchKernelGGL((merge_kernel<SRC, OUT_F32>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((merge_kernel<SRC, OUT_PLAIN>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int out, hipStream_t stream) {
  if (a.n_brackets <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, out, stream); });
}

}  // namespace em
