// Dynamic defective-pixel correction kernels (isp_dynamic_defects.h; the contract is DESIGN.md 3, "Dynamic defects").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value, the taps q0 .. q7 are the eight same-site
// neighbours (r-2,c-2) (r-2,c) (r-2,c+2) (r,c-2) (r,c+2) (r+2,c-2) (r+2,c) (r+2,c+2); a tap is kept when it is inside the
// frame, not in the defect mask and finite; n is the number of kept taps, k = tolerate:
//   detect:  hi / lo = the (k+1)-th largest / smallest kept tap; T(v) = t + s max(v, 0); p is a candidate when n >= 2k + 1,
//            x(p) is finite and p is not listed; hot when x(p) - hi > T(hi), dead when lo - x(p) > T(lo)
//   replace: of the pairs (q1,q6) (q3,q4) (q0,q7) (q2,q5) with both taps kept, the one of the smallest |a - b| (the earlier
//            on a tie) gives m = (a + b) 0.5; hot: y = min(m, hi), or hi without a pair; dead: y = max(m, lo), or lo; every
//            other pixel keeps y = x(p), the same bits (a listed defect too: the fix-up replaces it)
//   cfa = cast_work(y * g(p))   (g the shading / AWB gain, 1 without a grid), or the plain f32 y
// Every operation is one f32 rounding (no contraction): the output is the contract's bit for bit.
//
// One 256-thread block per 64 x 64 output tile of one frame (grid.z): the tile plus a halo of two rows and two columns is
// decoded ONCE into LDS as f32 x (68 floats a row: the lanes of a wave read 64 consecutive floats whatever the tap, one
// bank each), and every value that is no tap - outside the frame, listed, or not finite - is then marked there as a NaN:
// the hardware's median and minimum of three skip a NaN, so the rank selection needs no test per tap.  Lane l of wave w
// takes column l of rows 16 w .. 16 w + 15 in two passes.
//   pass 1, every pixel: the two largest and the two smallest taps (32 v_med3_f32 over eight LDS reads),
//     the two threshold tests, the ballot of hot | dead - the row's two words of the flag plane, a tile starting on a
//     multiple of 64 columns - and the store of x(p) g(p).  The count n is not kept: with too few taps the tests can only
//     err towards a flag, so n is counted behind a wave-uniform branch on the ballot, for the lanes that would flag.
//   pass 2, flagged pixels only: each lane walks the rows it flagged (a bit mask), reads the taps again, selects the
//     pair and stores y g(p) over pass 1's value.  The walk costs the wave as many steps as its busiest lane has flagged
//     rows, where a branch inside pass 1 would cost every row segment that holds a flagged pixel the whole selection.
#include "isp_dynamic_defects.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace ddp {

MI_DEV bool finite(float v) { return fabsf(v) < INFINITY; }            // (false for a NaN)
MI_DEV float med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }   // (with a NaN: the minimum of the others)
// max(a, b) of finite values, b possibly a NaN (then a): one v_med3_f32, where fmaxf would quiet its operands first (a
// v_max_f32 of each with itself).  No operand of a median here is an infinite constant: the compiler rewrites such a median
// as a minimum or maximum that returns the constant for a NaN, where the instruction returns the minimum of the others.
constexpr float LARGEST = 3.402823466e38f;
MI_DEV float max_of(float a, float b) { return med3(a, b, LARGEST); }

// the two largest taps (h1 >= h2) and the negated two smallest (g1 >= g2), each from -LARGEST, which no kept tap is below:
// with fewer than two taps the start value stays.  A NaN tap leaves all four.
struct Rank { float h1, h2, g1, g2; };
MI_DEV void tap(Rank& k, float v) {
  k.h2 = med3(k.h1, k.h2, v);                         // h1 >= h2: the middle one is the new second largest
  k.h1 = max_of(k.h1, v);
  k.g2 = med3(k.g1, k.g2, -v);
  k.g1 = max_of(k.g1, -v);
}
MI_DEV Rank rank(const float (&q)[8]) {
  Rank k = {-LARGEST, -LARGEST, -LARGEST, -LARGEST};
#pragma unroll
  for (int j = 0; j < 8; ++j) tap(k, q[j]);
  return k;
}

// the usable pair (neither tap a NaN) of the smallest |a - b| so far (the earlier on a tie) and its mean; d a NaN: none yet
struct Pair { float d, m; };
MI_DEV void pair(Pair& p, float a, float b) {
  const float d = fabsf(a - b);                       // (a NaN iff a tap is one: kept taps are finite)
  const bool take = d == d && !(p.d <= d);
  p.d = take ? d : p.d;
  p.m = take ? (a + b) * 0.5f : p.m;
}

template <int OUT> struct OutType { typedef float type; };
template <> struct OutType<hl::OUT_F16> { typedef half_t type; };

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, int OUT>
__global__ void __launch_bounds__(THREADS) dynamic_defects_kernel(const Args a) {
  typedef typename OutType<OUT>::type TO;
  constexpr int LW = TILE_W + 2 * HALO_C;             // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO_R;
  static_assert(PX <= 32, "a lane's flagged rows are the bits of one word");
  __shared__ float xs[LH * LW];

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;

  // 1. the tile and its halo, decoded once: x, or -inf for a tap that is outside the frame or a listed defect; then every
  // value that is not finite becomes a NaN (stage_tile's thread u wrote the pair at floats 2 u, 2 u + 1: the same thread
  // reads it back, no barrier in between)
  raw::stage_tile<SRC, TILE_H, TILE_W, HALO_R, HALO_C, THREADS>(a, fr.src, fr.mask, r0, c0, xs);
  for (int u = threadIdx.x; u < LH * LW / 2; u += THREADS) {
    float2 v = reinterpret_cast<float2*>(xs)[u];
    v.x = finite(v.x) ? v.x : NAN;
    v.y = finite(v.y) ? v.y : NAN;
    reinterpret_cast<float2*>(xs)[u] = v;
  }
  __syncthreads();

  // 2. lane = tile column
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  const float t = a.t, s = a.s;
  const bool second = a.tolerate != 0, do_hot = a.hot != 0, do_dead = a.dead != 0;
  const int need = second ? 3 : 1;                    // n >= 2 k + 1
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);
  uint32_t* __restrict__ flags = fr.flags;
  const int word = (c0 >> 5) + lane;                  // lanes 0 and 1 write the row's two flag words
  auto taps = [&](int tr, float (&q)[8]) -> float {   // the taps q0 .. q7 and x(p) of tile row tr, as LDS holds them
    const float* row = &xs[(tr + HALO_R) * LW + lane + HALO_C];
    q[0] = row[-2 * LW - 2]; q[1] = row[-2 * LW]; q[2] = row[-2 * LW + 2]; q[3] = row[-2]; q[4] = row[2];
    q[5] = row[2 * LW - 2]; q[6] = row[2 * LW]; q[7] = row[2 * LW + 2];
    return row[0];
  };
  uint32_t pending = 0, pending_hot = 0;              // the rows this lane flagged, and which of them as hot

  // pass 1
  for (int i = 0; i < PX; ++i) {
    const int tr = wave * PX + i;                     // tile row
    const int r = r0 + tr;
    const bool inside = r < H && c < W;
    float q[8];
    const float xp = taps(tr, q);                     // (a NaN outside the frame, for a listed centre and a non-finite one)
    const Rank k = rank(q);
    const float hi = second ? k.h2 : k.h1, lo = second ? -k.g2 : -k.g1;
    // with n < 2 k + 1 taps hi is the start value, or (k = 1, n = 2) the smaller of the two: the tests can only err towards a
    // flag, and n decides below
    const bool cand = xp == xp;
    const bool is_hot = cand && do_hot && xp - hi > t + s * max_of(hi, 0.f);
    const bool is_dead = cand && do_dead && lo - xp > t + s * max_of(lo, 0.f);
    bool flagged = is_hot || is_dead;
    if (__builtin_amdgcn_ballot_w64(flagged) != 0) {
      if (flagged) {
        const bool missing = (q[0] != q[0] || q[1] != q[1]) || (q[2] != q[2] || q[3] != q[3]) ||
                             (q[4] != q[4] || q[5] != q[5]) || (q[6] != q[6] || q[7] != q[7]);
        if (missing) {                                // a tap is missing: count them
          int n = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) n += q[j] == q[j] ? 1 : 0;
          flagged = n >= need;
        }
      }
    }
    const unsigned long long found = __builtin_amdgcn_ballot_w64(flagged);
    pending |= flagged ? 1u << i : 0u;
    pending_hot |= flagged && is_hot ? 1u << i : 0u;
    if (flags && lane < 2 && r < H && word < a.mask_w)
      flags[(size_t)r * a.mask_w + word] = lane ? (uint32_t)(found >> 32) : (uint32_t)found;
    float y = xp;
    if (xp != xp && inside) y = raw::decode_one<SRC>(a, fr.src, r, c);   // a listed or non-finite pixel keeps its own value (rare)
    if constexpr (OUT != hl::OUT_PLAIN) {
      if (a.shading) y = y * shade_gain(a, r, c);     // (shade_axis clamps the pixel into the frame)
    }
    if (inside) dst[(size_t)r * W + c] = cast_out<TO>(y);
  }

  // pass 2: a flagged pixel is inside the frame
  while (__builtin_amdgcn_ballot_w64(pending != 0) != 0) {
    if (pending != 0) {
      const int i = __builtin_ctz(pending);
      const bool is_hot = (pending_hot >> i & 1u) != 0;
      pending &= pending - 1;
      const int tr = wave * PX + i;
      const int r = r0 + tr;
      float q[8];
      taps(tr, q);
      const Rank k = rank(q);
      const float hi = second ? k.h2 : k.h1, lo = second ? -k.g2 : -k.g1;
      Pair p = {NAN, 0.f};
      pair(p, q[1], q[6]); pair(p, q[3], q[4]); pair(p, q[0], q[7]); pair(p, q[2], q[5]);
      const bool have = p.d == p.d;
      float y;
      if (is_hot) y = have ? fminf(p.m, hi) : hi;
      else y = have ? fmaxf(p.m, lo) : lo;
      if constexpr (OUT != hl::OUT_PLAIN) {
        if (a.shading) y = y * shade_gain(a, r, c);
      }
      dst[(size_t)r * W + c] = cast_out<TO>(y);
    }
  }
}

template <int SRC>
static int launch_src(const Args& a, int out, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  if (out == hl::OUT_F16)
    hipLaunchKernelGGL((dynamic_defects_kernel<SRC, hl::OUT_F16>), grid, dim3(THREADS), 0, stream, a);
  else if (out == hl::OUT_F32)
    hipLaunchKernelGGL((dynamic_defects_kernel<SRC, hl::OUT_F32>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((dynamic_defects_kernel<SRC, hl::OUT_PLAIN>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, int out, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, out, stream); });
}

}  // namespace ddp
