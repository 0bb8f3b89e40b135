// Direction-adaptive demosaic kernels (isp_demosaic_dir.h; the contract is DESIGN.md 3, "Directional demosaic").
//
// X(r, c): the f32 value of the work-dtype CFA, extended over the plane by the mirror that does not repeat the edge sample
// (index i folds with period 2 (n - 1); the Bayer phase is kept).  Every line one f32 operation, in the order written:
//   1. eh = (X(r,c-1) + X(r,c+1)) * 0.5 + ((X + X) - (X(r,c-2) + X(r,c+2))) * 0.25, ev the same along the column;
//      red / blue site: CH = X - eh, CV = X - ev; green site: CH = eh - X, CV = ev - X
//   2. DH(r,c) = |CH(r,c) - CH(r,c+2)|, DV(r,c) = |CV(r,c) - CV(r+2,c)|;
//      dH = DH(r-2,c) + DH(r-2,c+2) + DH(r-1,c+1) + 3 DH(r,c) + 3 DH(r,c+2) + DH(r+1,c+1) + DH(r+2,c) + DH(r+2,c+2), summed
//      left to right; dV its transpose; the site is horizontal when dV >= dH
//   3. red / blue site: G = horizontal ? eh : ev
//   4. green site: K = X + ((X(q0) - G(q0)) + (X(q1) - G(q1))) * 0.5 for the row's chroma K from the row neighbours q, the
//      other chroma from the column neighbours
//   5. red / blue site: d = (RB(q0) + RB(q1)) * 0.5 over the green neighbours along the decision, RB = R - B of step 4;
//      blue site R = X + d, red site B = X - d
//   6. mi_isp_demosaic's epilogue: (m0 r + m1 g) + m2 b, clamp01, * scale(out), the cast
//
// One 256-thread block per 64 x 32 output tile of one frame (grid.z).  The block stages the tile and its halo (4 before, 8
// after) ONCE as f32 X into LDS plane P0 - decoded at the folded coordinates, gained and rounded to the work dtype: the
// loaders' CFA - and then works through three planes with barriers in between:
//   B. CH -> P1, CV -> P2 at every staged site that a classifier window reads (a lane a column: conflict-free)
//   C. the decision and G of every red / blue site within two pixels of the tile, held in registers across a barrier and
//      then written over the dead planes: G -> P1 (at red / blue sites), horizontal -> P2
//   D. R - B of every green site within one pixel of the tile -> P1 (at green sites: no lane reads them in this phase)
//   E. a lane takes a column pair - one green, one red / blue pixel: steps 4 - 6 - and stores its six values at once
// No phase has a border case: the fold at staging is the only place that knows the frame's edge.
#include "isp_demosaic_dir.h"
#include "isp_math.h"

#pragma clang fp contract(off)

namespace dd {

// index i of the mirror extension of n >= 2 samples, p = 2 (n - 1)
MI_DEV int fold(int i, int n, int p) {
  if ((unsigned)i < (unsigned)n) return i;            // (inside the frame: every tap of an interior tile)
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

// the loaders' CFA value at frame pixel (r, c) from the decoded x: cast_work(x * g)
template <class WT>
MI_DEV float cfa_value(const Args& a, float x, int r, int c) {
  if (a.shading) x = x * shade_gain(a, r, c);
  return (float)cast_out<WT>(x);
}

// the CFA values of the extended pixels (er, ec) and (er, ec + 1), ec even
template <int SRC, class WT>
MI_DEV float2 staged_pair(const Args& a, const void* src, int er, int ec) {
  const int r = fold(er, a.H, 2 * (a.H - 1));
  const int p = 2 * (a.W - 1);
  const int c0 = fold(ec, a.W, p), c1 = fold(ec + 1, a.W, p);
  float x0, x1;
  if (c1 == c0 + 1 && (c0 & 1) == 0) {                // a pair of the frame
    raw::decode_pair<SRC>(a, src, r, c0, true, x0, x1);
  } else {                                            // across a mirror: each from its own pair
    x0 = raw::decode_one<SRC>(a, src, r, c0);
    x1 = raw::decode_one<SRC>(a, src, r, c1);
  }
  return make_float2(cfa_value<WT>(a, x0, r, c0), cfa_value<WT>(a, x1, r, c1));
}

MI_DEV float estimate(float m1, float p1, float x, float m2, float p2) {
  return (m1 + p1) * 0.5f + ((x + x) - (m2 + p2)) * 0.25f;
}

// six consecutive output elements (two pixels) at p, which is aligned to two elements when `vec`
template <class TO>
MI_DEV void store6(TO* p, const TO (&v)[6], bool vec) {
  if constexpr (sizeof(TO) == 1) {
    if (vec) {
      typedef uint16_t u16a __attribute__((aligned(2)));
      uint16_t w[3];
      __builtin_memcpy(w, v, 6);
      u16a* q = reinterpret_cast<u16a*>(p);
      q[0] = w[0]; q[1] = w[1]; q[2] = w[2];
      return;
    }
  } else {
    if (vec) {
      constexpr int N = (int)sizeof(TO) * 6 / 4;      // 3 or 6 dwords, which the compiler merges into wide stores
      uint32_t w[N];
      __builtin_memcpy(w, v, sizeof(w));
      uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
      for (int j = 0; j < N; ++j) q[j] = w[j];
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) p[j] = v[j];
}

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_frames)
template <int SRC, class WT, class TO>
__global__ void __launch_bounds__(THREADS) demosaic_dir_kernel(const Args a) {
  __shared__ float P0[LH * LW], P1[LH * LW], P2[LH * LW];
  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;   // (even: tile parities are frame parities)
  const int gp = a.green_par, rp = a.red_par;
  const int t = threadIdx.x;
  // tile coordinates (tr, tc) of a staged site: rows -HALO_B .. TILE_H + HALO_A - 1, likewise the columns
  auto at = [](int tr, int tc) { return (tr + HALO_B) * LW + tc + HALO_B; };

  // A. the tile and its halo: the loaders' CFA at the folded coordinates, a lane a column pair
  {
    constexpr int LP = LW / 2;
    for (int u = t; u < LH * LP; u += THREADS) {
      const int lr = u / LP, lp = u - lr * LP;
      const float2 v = staged_pair<SRC, WT>(a, fr.src, r0 - HALO_B + lr, c0 - HALO_B + 2 * lp);
      *reinterpret_cast<float2*>(&P0[lr * LW + 2 * lp]) = v;
    }
  }
  __syncthreads();

  // B. step 1 wherever a classifier window reads it: CH over rows -4 .. TILE_H + 3, columns -2 .. TILE_W + 5; CV over rows
  //    -2 .. TILE_H + 5, columns -4 .. TILE_W + 3 (the taps stay inside the staged plane)
  {
    constexpr int NR = TILE_H + 10, NC = TILE_W + 10;
    for (int u = t; u < NR * NC; u += THREADS) {
      const int q = u / NC;
      const int tr = q - HALO_B, tc = u - q * NC - HALO_B;
      const int i = at(tr, tc);
      const float x = P0[i];
      const bool green = ((tr + tc) & 1) == gp;
      if (tc >= -2 && tr < TILE_H + 4) {
        const float eh = estimate(P0[i - 1], P0[i + 1], x, P0[i - 2], P0[i + 2]);
        P1[i] = green ? eh - x : x - eh;
      }
      if (tr >= -2 && tc < TILE_W + 4) {
        const float ev = estimate(P0[i - LW], P0[i + LW], x, P0[i - 2 * LW], P0[i + 2 * LW]);
        P2[i] = green ? ev - x : x - ev;
      }
    }
  }
  __syncthreads();

  // C. steps 2 and 3 at the red / blue sites of rows -2 .. TILE_H + 1, columns -2 .. TILE_W + 1.  The region is taken in
  //    2 x 2 quads, each with one red / blue site per row, on columns of opposite parity: lanes 0 .. 15 of a 32-lane LDS
  //    group take the upper sites of 16 consecutive quads, lanes 16 .. 31 the lower ones, so the 32 addresses of every tap
  //    fall on 32 banks (the row pitch is even: a row down keeps the bank parity)
  constexpr int CP = (TILE_W + 4) / 2;                // quad columns of the region
  constexpr int CQ = (TILE_H + 4) / 2 * CP;           // its quads
  constexpr int CK = ((CQ + 15) / 16 * 32 + THREADS - 1) / THREADS;   // sites per lane
  // site u of a region of NQ quads whose first row is row_0: (quad, row bit) -> (tr, tc) of the red / blue (rb 1) or green site
  auto quad_site = [&](int u, int row_0, int rb_site, int& tr, int& tc) {
    const int q = ((u >> 5) << 4) | (u & 15);
    const int qr = q / CP;
    tr = 2 * qr + row_0 + ((u >> 4) & 1);
    tc = 2 * (q - qr * CP) - 2 + ((tr ^ gp ^ rb_site) & 1);
    return q;
  };
  float g_keep[CK];
  bool h_keep[CK];
#pragma unroll
  for (int k = 0; k < CK; ++k) {
    const int u = t + k * THREADS;
    g_keep[k] = 0.f;
    h_keep[k] = false;
    int tr, tc;
    if (quad_site(u, -2, 1, tr, tc) < CQ) {
      const int i = at(tr, tc);
      const float* ch = &P1[i];
      const float* cv = &P2[i];
      auto dh = [&](int dr, int dc) { return fabsf(ch[dr * LW + dc] - ch[dr * LW + dc + 2]); };
      auto dv = [&](int dr, int dc) { return fabsf(cv[dr * LW + dc] - cv[(dr + 2) * LW + dc]); };
      float sH = dh(-2, 0);
      sH = sH + dh(-2, 2);
      sH = sH + dh(-1, 1);
      sH = sH + 3.f * dh(0, 0);
      sH = sH + 3.f * dh(0, 2);
      sH = sH + dh(1, 1);
      sH = sH + dh(2, 0);
      sH = sH + dh(2, 2);
      float sV = dv(0, -2);
      sV = sV + dv(2, -2);
      sV = sV + dv(1, -1);
      sV = sV + 3.f * dv(0, 0);
      sV = sV + 3.f * dv(2, 0);
      sV = sV + dv(1, 1);
      sV = sV + dv(0, 2);
      sV = sV + dv(2, 2);
      const bool hz = sV >= sH;
      const float x = P0[i];
      const float e = hz ? estimate(P0[i - 1], P0[i + 1], x, P0[i - 2], P0[i + 2])
                         : estimate(P0[i - LW], P0[i + LW], x, P0[i - 2 * LW], P0[i + 2 * LW]);
      g_keep[k] = e;
      h_keep[k] = hz;
    }
  }
  __syncthreads();                                    // (every window has been read: CH and CV are dead)
#pragma unroll
  for (int k = 0; k < CK; ++k) {
    const int u = t + k * THREADS;
    int tr, tc;
    if (quad_site(u, -2, 1, tr, tc) < CQ) {
      P1[at(tr, tc)] = g_keep[k];
      P2[at(tr, tc)] = h_keep[k] ? 1.f : 0.f;
    }
  }
  __syncthreads();

  // step 4 at the green site i (tile row tr): R and B from the chroma K - G of its row and column neighbours
  auto green_rb = [&](int i, int tr, float& R, float& B) {
    const float x = P0[i];
    const float krow = x + ((P0[i - 1] - P1[i - 1]) + (P0[i + 1] - P1[i + 1])) * 0.5f;
    const float kcol = x + ((P0[i - LW] - P1[i - LW]) + (P0[i + LW] - P1[i + LW])) * 0.5f;
    const bool red_row = (tr & 1) == rp;
    R = red_row ? krow : kcol;
    B = red_row ? kcol : krow;
  };

  // D. R - B at the green sites of rows -1 .. TILE_H, columns -1 .. TILE_W (P1 holds G at the red / blue sites only)
  {
    constexpr int DQ = (TILE_H + 2) / 2 * CP;         // quads, from row -1 (the same lane mapping as phase C)
    for (int u = t; u < (DQ + 15) / 16 * 32; u += THREADS) {
      int tr, tc;
      if (quad_site(u, -1, 0, tr, tc) < DQ && tc >= -1 && tc <= TILE_W) {
        float R, B;
        green_rb(at(tr, tc), tr, R, B);
        P1[at(tr, tc)] = R - B;
      }
    }
  }
  __syncthreads();

  // E. the output: a lane takes the column pair (2 l, 2 l + 1) of a row, 8 rows a pass
  TO* __restrict__ dst = static_cast<TO*>(fr.dst);
  const bool vec = (reinterpret_cast<uintptr_t>(dst) & (sizeof(TO) == 1 ? 1 : 3)) == 0;
  const int pc = t & 31, sub = t >> 5;
#pragma unroll 1
  for (int pass = 0; pass < TILE_H / 8; ++pass) {
    const int tr = pass * 8 + sub;
    const int r = r0 + tr, c = c0 + 2 * pc;
    if (r >= H || c >= W) continue;                   // (W is even: the pair is inside or outside as one)
    const int og = (tr ^ gp) & 1;                     // the green pixel of the pair
    const int ig = at(tr, 2 * pc + og), ic = at(tr, 2 * pc + (og ^ 1));
    float px[2][3];
    {                                                 // the green pixel
      float R, B;
      green_rb(ig, tr, R, B);
      px[0][0] = R; px[0][1] = P0[ig]; px[0][2] = B;
    }
    {                                                 // the red / blue pixel
      const float x = P0[ic];
      const bool hz = P2[ic] != 0.f;
      const float d = hz ? (P1[ic - 1] + P1[ic + 1]) * 0.5f : (P1[ic - LW] + P1[ic + LW]) * 0.5f;
      const bool red = (tr & 1) == rp;
      px[1][0] = red ? x : x + d;
      px[1][1] = P1[ic];
      px[1][2] = red ? x - d : x;
    }
    TO o[6];
#pragma unroll
    for (int k = 0; k < 2; ++k) {                     // k: the pixel at column 2 l + k
      const int s = k ^ og;                           // (0: the green one)
      float v0 = s ? px[1][0] : px[0][0], v1 = s ? px[1][1] : px[0][1], v2 = s ? px[1][2] : px[0][2];
      if (a.has_ccm) {                                // the sequential f32 dot of mi_isp_demosaic
        const float e0 = (a.ccm[0] * v0 + a.ccm[1] * v1) + a.ccm[2] * v2;
        const float e1 = (a.ccm[3] * v0 + a.ccm[4] * v1) + a.ccm[5] * v2;
        const float e2 = (a.ccm[6] * v0 + a.ccm[7] * v1) + a.ccm[8] * v2;
        v0 = e0; v1 = e1; v2 = e2;
      }
      o[3 * k] = cast_out<TO>(clamp01(v0) * a.out_scale);
      o[3 * k + 1] = cast_out<TO>(clamp01(v1) * a.out_scale);
      o[3 * k + 2] = cast_out<TO>(clamp01(v2) * a.out_scale);
    }
    store6<TO>(dst + ((size_t)r * W + c) * 3, o, vec);
  }
}

// the decode alone: grid (ceil(W / CFA_TILE_W), ceil(H / CFA_TILE_H), n_frames), a lane a column pair, 4 rows a pass
template <int SRC, class WT>
__global__ void __launch_bounds__(THREADS) raw_cfa_kernel(const Args a) {
  const Frame& fr = a.f[blockIdx.z];
  const int H = a.H, W = a.W;
  WT* __restrict__ dst = static_cast<WT*>(fr.dst);
  const bool vec = (reinterpret_cast<uintptr_t>(dst) & (2 * sizeof(WT) - 1)) == 0;
  const int c = blockIdx.x * CFA_TILE_W + 2 * (threadIdx.x & 63);
  if (c >= W) return;
  for (int k = 0; k < CFA_TILE_H / 4; ++k) {
    const int r = blockIdx.y * CFA_TILE_H + 4 * k + (threadIdx.x >> 6);
    if (r >= H) return;
    float x0, x1;
    raw::decode_pair<SRC>(a, fr.src, r, c, true, x0, x1);
    const WT v0 = cast_out<WT>(a.shading ? x0 * shade_gain(a, r, c) : x0);
    const WT v1 = cast_out<WT>(a.shading ? x1 * shade_gain(a, r, c + 1) : x1);
    WT* p = dst + (size_t)r * W + c;
    if (vec) {
      WT pair[2] = {v0, v1};
      typedef typename std::conditional<sizeof(WT) == 2, uint32_t, uint2>::type U;
      U w;
      __builtin_memcpy(&w, pair, sizeof(w));
      *reinterpret_cast<U*>(p) = w;
    } else {
      p[0] = v0;
      p[1] = v1;
    }
  }
}

template <int SRC, class WT, class TO>
static int launch_one(const Args& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  hipLaunchKernelGGL((demosaic_dir_kernel<SRC, WT, TO>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

// a CFA source fixes the work dtype and takes every output dtype; a raw source writes its work dtype
template <int SRC>
static int launch_src(const Args& a, int work, int out, hipStream_t stream) {
  if constexpr (SRC == raw::SRC_CFA_F16 || SRC == raw::SRC_CFA_F32) {
    typedef typename std::conditional<SRC == raw::SRC_CFA_F16, half_t, float>::type WT;
    switch (out) {
      case MI_U8: return launch_one<SRC, WT, uint8_t>(a, stream);
      case MI_U16: return launch_one<SRC, WT, uint16_t>(a, stream);
      case MI_F16: return launch_one<SRC, WT, half_t>(a, stream);
      default: return launch_one<SRC, WT, float>(a, stream);
    }
  } else {
    if (work == MI_F16) return launch_one<SRC, half_t, half_t>(a, stream);
    return launch_one<SRC, float, float>(a, stream);
  }
}

int launch(const Args& a, int src, int work, int out, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, work, out, stream); });
}

template <int SRC>
static int launch_cfa_src(const Args& a, int work, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + CFA_TILE_W - 1) / CFA_TILE_W), (unsigned)((a.H + CFA_TILE_H - 1) / CFA_TILE_H),
                  (unsigned)a.n_frames);
  if constexpr (SRC == raw::SRC_CFA_F16 || SRC == raw::SRC_CFA_F32) {
    return 0;                                         // (a CFA is its own decode: no entry point asks for it)
  } else {
    if (work == MI_F16)
      hipLaunchKernelGGL((raw_cfa_kernel<SRC, half_t>), grid, dim3(THREADS), 0, stream, a);
    else
      hipLaunchKernelGGL((raw_cfa_kernel<SRC, float>), grid, dim3(THREADS), 0, stream, a);
    MI_LAUNCH_CHECK();
    return 0;
  }
}

int launch_cfa(const Args& a, int src, int work, hipStream_t stream) {
  if (a.n_frames <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_cfa_src<decltype(s)::value>(a, work, stream); });
}

}  // namespace dd
