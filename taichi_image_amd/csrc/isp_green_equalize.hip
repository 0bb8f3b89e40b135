// Green equalisation kernels (isp_green_equalize.h; the contract is DESIGN.md 3, "Green equalisation").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value; p is green iff ((r + c) & 1) == gp.  The taps of
// a green p, in this order:
//   radius 1: group O (the other green phase) (r-1,c-1) (r-1,c+1) (r+1,c-1) (r+1,c+1);
//             group S (p's own phase) (r,c) (r-2,c) (r,c-2) (r,c+2) (r+2,c)
//   radius 2: group O (r+dy, c+dx) for dy in (-3,-1,1,3), for dx in (-3,-1,1,3), row-major;
//             group S (r,c), then (r+dy, c+dx) for dy in (-2,0,2), for dx in (-2,0,2), without (0,0), row-major
// A tap is kept when it is inside the frame, not in the defect mask and finite.  Per group: the f32 sum of the kept taps in
// the listed order starting from the first kept one, their count n, their maximum and minimum.
//   O = sumO / f32(nO)   S = sumS / f32(nS)   d = O - S   lim = t + s max(O, S)   e = edge lim
//   apply iff nO >= 1 and |d| <= lim and maxO - minO <= e and maxS - minS <= e (and p itself is a kept tap)
//   y = x(p) + (f32(strength) 0.5f) d if apply; every other pixel - not green, listed, not finite - keeps y = x(p), the same bits
//   cfa = cast_work(y * g(p))   (g the shading / AWB gain, 1 without a grid), or the plain f32 y
// Every operation is one f32 rounding (no contraction, IEEE divisions): the output is the contract's bit for bit.
//
// One 256-thread block per 64 x 64 output tile of one frame (grid.z): the tile plus its halo (2 rows and 2 columns at radius
// 1; 3 rows and 4 columns at radius 2, the decode's pairs start on even columns) is decoded ONCE into LDS as f32 x, and
// every value that is no tap - outside the frame, listed, or not finite - is then marked there as a NaN: the hardware's
// median of three skips a NaN, so the extrema need no test per tap.
// Only every other pixel of a row is green, so a lane takes a column PAIR - one green site and one pixel that passes
// through - and a wave two rows per step: lanes 0-15 and 32-47 the 32 pairs of the even row, lanes 16-31 and 48-63 those of
// the odd row.  Every lane then does the arithmetic of one green site, and within each group of 32 lanes that the LDS
// serves at once the even row's lanes read the columns of one parity and the odd row's those of the other (the row pitch
// is even, the green column alternates with the row): 32 different banks whatever the tap.
#include "isp_green_equalize.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace geq {

MI_DEV bool finite(float v) { return fabsf(v) < INFINITY; }            // (false for a NaN)
MI_DEV float med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }   // (with a NaN: the minimum of the others)
// max(a, b) of finite values, b possibly a NaN (then a): one v_med3_f32 (no operand is an infinite constant: the compiler
// would rewrite such a median as a maximum that returns the constant for a NaN)
constexpr float LARGEST = 3.402823466e38f;
MI_DEV float max_of(float a, float b) { return med3(a, b, LARGEST); }

// one tap group over NaN-marked taps: the sum from -0 (-0 + v is v, bit for bit, and v + -0 too: a skipped tap adds -0),
// the count, the maximum and the negated minimum, each from -LARGEST, which no kept tap is below
struct Group { float sum; int n; float mx, nmn; };
MI_DEV void tap(Group& g, float v) {
  const bool kept = v == v;
  g.sum = g.sum + (kept ? v : -0.f);
  g.n += kept ? 1 : 0;
  g.mx = max_of(g.mx, v);
  g.nmn = max_of(g.nmn, -v);
}

template <int OUT> struct OutType { typedef float type; };
template <> struct OutType<hl::OUT_F16> { typedef half_t type; };
template <class TO> struct alignas(2 * sizeof(TO)) Pair2 { TO a, b; };   // two pixels in one store

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, int OUT, int R>
__global__ void __launch_bounds__(THREADS) green_equalize_kernel(const Args a) {
  typedef typename OutType<OUT>::type TO;
  constexpr int HR = halo_r(R), HC = halo_c(R);
  constexpr int LW = TILE_W + 2 * HC;                 // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HR;
  static_assert(LW % 2 == 0 && (LH * LW) % 2 == 0, "the rows hold whole pairs");
  __shared__ float xs[LH * LW];

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo, decoded once: x, or -inf for a tap that is outside the frame or a listed defect; then every
  // value that is not finite becomes a NaN (stage_tile's thread u wrote the pair at floats 2 u, 2 u + 1: the same thread
  // reads it back, no barrier in between)
  raw::stage_tile<SRC, TILE_H, TILE_W, HR, HC, THREADS>(a, fr.src, fr.mask, r0, c0, xs);
  for (int u = threadIdx.x; u < LH * LW / 2; u += THREADS) {
    float2 v = reinterpret_cast<float2*>(xs)[u];
    v.x = finite(v.x) ? v.x : NAN;
    v.y = finite(v.y) ? v.y : NAN;
    reinterpret_cast<float2*>(xs)[u] = v;
  }
  __syncthreads();

  // 2. lane = a column pair of one of the step's two rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = (lane >> 4) & 1;                      // the row of the step: its parity too (r0, 16 wave, 2 i are even)
  const int pr = (lane & 15) | ((lane >> 5) << 4);    // the pair of the row, 0 .. 31
  const int j = a.gp ^ h;                             // the green column of the pair (c0 and 2 pr are even)
  const int c = c0 + 2 * pr;                          // the pair's first column
  const int cg = c + j, cn = c + (j ^ 1);
  const float t = a.t, s = a.s, edge = a.edge, hs = a.hs;
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);
  const bool vec = (W & 1) == 0 && (reinterpret_cast<uintptr_t>(fr.dst) & (2 * sizeof(TO) - 1)) == 0;   // (a pair is aligned)

  for (int i = 0; i < STEPS; ++i) {
    const int tr = wave * (2 * STEPS) + 2 * i + h;    // tile row
    const int r = r0 + tr;
    const float* ctr = &xs[(tr + HR) * LW + HC + 2 * pr];
    const float2 both = *reinterpret_cast<const float2*>(ctr);
    const float xg = j ? both.y : both.x, xn = j ? both.x : both.y;   // (NaNs outside the frame, listed or not finite)
    const float* g = ctr + j;
    Group O = {-0.f, 0, -LARGEST, -LARGEST}, S = {-0.f, 0, -LARGEST, -LARGEST};
    if constexpr (R == 1) {
      tap(O, g[-LW - 1]); tap(O, g[-LW + 1]); tap(O, g[LW - 1]); tap(O, g[LW + 1]);
      tap(S, xg); tap(S, g[-2 * LW]); tap(S, g[-2]); tap(S, g[2]); tap(S, g[2 * LW]);
    } else {
#pragma unroll
      for (int dy = -3; dy <= 3; dy += 2)
#pragma unroll
        for (int dx = -3; dx <= 3; dx += 2) tap(O, g[dy * LW + dx]);
      tap(S, xg);
#pragma unroll
      for (int dy = -2; dy <= 2; dy += 2)
#pragma unroll
        for (int dx = -2; dx <= 2; dx += 2)
          if (dy != 0 || dx != 0) tap(S, g[dy * LW + dx]);
    }
    // (with no kept tap a mean is -0 / 0, a NaN: every comparison below is written so that a NaN makes it false)
    const float mO = O.sum / (float)O.n, mS = S.sum / (float)S.n;
    const float d = mO - mS;
    const float lim = t + s * fmaxf(mO, mS);
    const float e = edge * lim;
    const bool apply = xg == xg && O.n >= 1 && fabsf(d) <= lim && O.mx + O.nmn <= e && S.mx + S.nmn <= e;
    float yg = apply ? xg + hs * d : xg, yn = xn;
    if ((xg != xg || xn != xn) && r < H) {            // a listed or non-finite pixel keeps its own value (rare)
      if (xg != xg && cg < W) yg = raw::decode_one<SRC>(a, fr.src, r, cg);
      if (xn != xn && cn < W) yn = raw::decode_one<SRC>(a, fr.src, r, cn);
    }
    if constexpr (OUT != hl::OUT_PLAIN) {
      if (a.shading) {                                // (shade_axis clamps the pixel into the frame)
        yg = yg * shade_gain(a, r, cg);
        yn = yn * shade_gain(a, r, cn);
      }
    }
    const TO o0 = cast_out<TO>(j ? yn : yg), o1 = cast_out<TO>(j ? yg : yn);
    if (r < H && c < W) {
      TO* p = dst + (size_t)r * W + c;
      if (vec) {                                      // (W is even: c + 1 is inside too)
        *reinterpret_cast<Pair2<TO>*>(p) = Pair2<TO>{o0, o1};
      } else {
        p[0] = o0;
        if (c + 1 < W) p[1] = o1;
      }
    }
  }
}

template <int SRC, int OUT>
static void launch_out(const Args& a, int radius, dim3 grid, hipStream_t stream) {
  if (radius == 1)
    hipLaunchKernelGGL((green_equalize_kernel<SRC, OUT, 1>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((green_equalize_kernel<SRC, OUT, 2>), grid, dim3(THREADS), 0, stream, a);
}

template <int SRC>
static int launch_src(const Args& a, int out, int radius, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  if (out == hl::OUT_F16)
    launch_out<SRC, hl::OUT_F16>(a, radius, grid, stream);
  else if (out == hl::OUT_F32)
    launch_out<SRC, hl::OUT_F32>(a, radius, grid, stream);
  else
    launch_out<SRC, hl::OUT_PLAIN>(a, radius, grid, stream);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int out, int radius, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, out, radius, stream); });
}

}  // namespace geq
