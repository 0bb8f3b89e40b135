// Chroma noise reduction kernels (isp_chroma_denoise.h; the contract is DESIGN.md 3, "Chroma noise reduction").
//
// The image is a grid of Hc x Wc cells of 2 x 2 pixels (the last row / column counted twice at an odd edge).  Per cell:
//   SL = sum of the four lumas, SB = sum of B - SL, SR = sum of R - SL      (YUV 4:2:0: the four Y, 4 U, 4 V)
//   T = the cells q of the (2r + 1)^2 window inside the grid with |SL(q) - SL| <= 4 tl, |SB(q) - SB| <= 4 tc, |SR(q) - SR| <= 4 tc
//   n = |T|, DB = sum over T of SB(q) - SB, DR likewise;  db = floor((2 DB S + 256 n) / (512 n)), dr likewise, dg from both
//   out_c = clamp(I_c + d_c, 0, 255) on the cell's pixels                  (YUV 4:2:0: U + db, V + dr)
//
// One 256-thread block per tile of 64 x 32 cells (128 x 64 pixels) of one image (grid.z).  1. The cells of the tile and of
// r rows and 2 or 4 columns around it are computed ONCE from the image into LDS, a cell one dword (SL 10 bits, SB + 1020
// and SR + 1020 11 bits each: the bias cancels in every difference and makes the fields unsigned): where the rows allow
// (W % 4 == 0 and 4-byte aligned images) a thread reads two cells as 2 x 3 dwords (two dwords and two half words for
// YUV) and sums their bytes with dot products, every load of the thread issued before the first is used; everything else
// goes byte by byte.  Even and odd cell columns lie in separate halves of an LDS row, so that the half wave, whose lane g
// owns cells 2g and 2g + 1, reads consecutive dwords.  2. A thread owns 2 x 4 cells, one row of two after the other.  It
// walks the 2r + 1 staged rows of the pair's windows: each of a row's 2r + 2 staged cells is read and unpacked once and
// tested against both cells (three v_sad_u32, a v_max3, a shift, two v_mad_u32_u24 and an add per tap).  A cell outside
// the grid is no tap: a block whose staged cells all lie inside the grid runs without the test, the others give such a
// cell a luma no threshold accepts.  3. The pair's pixels, read as three dwords per row before its windows were walked,
// take the deltas as packed 16-bit adds with a saturating pack (isp_u8_stage.h); byte by byte on the other path.
#include "isp_chroma_denoise.h"

namespace cdn {

using u8::clampi;
using u8::dot4;

constexpr uint32_t BIAS = 1020;                       // SB, SR in -1020 .. 1020

MI_DEV uint32_t pack_cell(uint32_t sl, uint32_t sb_biased, uint32_t sr_biased) { return sl | (sb_biased << 10) | (sr_biased << 21); }

// |a - b| + c
MI_DEV int sad(uint32_t a, uint32_t b, int c) {
  int r;
  asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
  return r;
}

// grid (ceil(Wc / TILE_CW), ceil(Hc / TILE_CH), n_images)
template <bool RGB, int R>
__global__ void __launch_bounds__(THREADS) chroma_denoise_kernel(const Args a) {
  constexpr int CH = RGB ? 3 : 1;                     // bytes per pixel of the rows the cells are summed from
  constexpr int HG = (R + 1) / 2;                     // staged pairs of cell columns on either side of the tile
  constexpr int LW = TILE_CW + 4 * HG;                // staged cell columns: staged column lc = cell column cb0 - 2 HG + lc
  constexpr int LH = TILE_CH + 2 * R;                 // staged cell rows: staged row lr = cell row ca0 - R + lr
  constexpr int HALF = LW / 2;                        // a staged row: its even columns, then its odd ones
  constexpr int N = 2 * R + 1;                        // window side
  __shared__ uint32_t cells[LH * LW];

  const u8::Image im = a.im[blockIdx.z];             // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
  const int cb0 = blockIdx.x * TILE_CW, ca0 = blockIdx.y * TILE_CH;
  const size_t pitch = (size_t)W * CH;
  const size_t plane = (size_t)H * W;                 // YUV: U starts here, V a quarter of it further
  const int Wh = W >> 1;                              // YUV: the pitch of U and V
  // the dword path: every pair of cells is then wholly inside the image or wholly outside, and its bytes are aligned
  const bool fast = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(im.src) | reinterpret_cast<uintptr_t>(im.dst)) & 3) == 0;

  // 1. the cells of the tile and its surround.  A cell outside the grid is never a tap: its loads are clamped into the
  // image and what they give is not used.
  if (fast) {
    constexpr int UNITS = LH * HALF;                  // pairs of cells
    constexpr int ITER = (UNITS + THREADS - 1) / THREADS;
    constexpr int NQ = RGB ? 6 : 4;
    uint32_t q[ITER][NQ];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int u = threadIdx.x + it * THREADS, lr = u / HALF, lu = u - lr * HALF;
      const int ca = clampi(ca0 - R + lr, 0, Hc - 1), c = clampi(2 * (cb0 - 2 * HG + 2 * lu), 0, W - 4);
      const int ra = 2 * ca, rb = min(2 * ca + 1, H - 1);
      const uint32_t* pa = reinterpret_cast<const uint32_t*>(im.src + (size_t)ra * pitch + (size_t)c * CH);
      const uint32_t* pb = reinterpret_cast<const uint32_t*>(im.src + (size_t)rb * pitch + (size_t)c * CH);
      if constexpr (RGB) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { q[it][ch] = pa[ch]; q[it][3 + ch] = pb[ch]; }
      } else {
        const size_t uo = plane + (size_t)ca * Wh + (size_t)(c >> 1);
        q[it][0] = pa[0]; q[it][1] = pb[0];
        q[it][2] = *reinterpret_cast<const uint16_t*>(im.src + uo);
        q[it][3] = *reinterpret_cast<const uint16_t*>(im.src + uo + plane / 4);
      }
    }
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
      const int u = threadIdx.x + it * THREADS, lr = u / HALF, lu = u - lr * HALF;
      uint32_t c0, c1;
      if constexpr (RGB) {
        // a row's four pixels: bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3; cell 0 holds pixels 0 and 1, cell 1 pixels 2 and 3
        const uint32_t* d = q[it];
        const uint32_t la = u8::luma4(d[0], d[1], d[2]), lb = u8::luma4(d[3], d[4], d[5]);
        const uint32_t sl0 = dot4(la, 0x00000101u, dot4(lb, 0x00000101u, 0u));
        const uint32_t sl1 = dot4(la, 0x01010000u, dot4(lb, 0x01010000u, 0u));
        const uint32_t r0 = dot4(d[0], 0x01000001u, dot4(d[3], 0x01000001u, BIAS));
        const uint32_t b0 = dot4(d[0], 0x00010000u, dot4(d[1], 0x00000100u, dot4(d[3], 0x00010000u, dot4(d[4], 0x00000100u, BIAS))));
        const uint32_t r1 = dot4(d[1], 0x00010000u, dot4(d[2], 0x00000100u, dot4(d[4], 0x00010000u, dot4(d[5], 0x00000100u, BIAS))));
        const uint32_t b1 = dot4(d[2], 0x01000001u, dot4(d[5], 0x01000001u, BIAS));
        c0 = pack_cell(sl0, b0 - sl0, r0 - sl0);
        c1 = pack_cell(sl1, b1 - sl1, r1 - sl1);
      } else {
        const uint32_t sl0 = dot4(q[it][0], 0x00000101u, dot4(q[it][1], 0x00000101u, 0u));
        const uint32_t sl1 = dot4(q[it][0], 0x01010000u, dot4(q[it][1], 0x01010000u, 0u));
        c0 = pack_cell(sl0, 4 * (q[it][2] & 0xffu) + BIAS, 4 * (q[it][3] & 0xffu) + BIAS);
        c1 = pack_cell(sl1, 4 * (q[it][2] >> 8) + BIAS, 4 * (q[it][3] >> 8) + BIAS);
      }
      if (u < UNITS) {
        cells[lr * LW + lu] = c0;
        cells[lr * LW + HALF + lu] = c1;
      }
    }
  } else {
    for (int u = threadIdx.x; u < LH * LW; u += THREADS) {
      const int lr = u / LW, pos = u - lr * LW;
      const int lc = pos < HALF ? 2 * pos : 2 * (pos - HALF) + 1;
      const int ca = clampi(ca0 - R + lr, 0, Hc - 1), cb = clampi(cb0 - 2 * HG + lc, 0, Wc - 1);
      uint32_t sl = 0, sb = BIAS, sr = BIAS;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint8_t* p = im.src + (size_t)min(2 * ca + i, H - 1) * pitch + (size_t)min(2 * cb + j, W - 1) * CH;
          if constexpr (RGB) {
            sl += (77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8;
            sr += p[0];
            sb += p[2];
          } else {
            sl += p[0];
          }
        }
      if constexpr (RGB) {
        sb -= sl;
        sr -= sl;
      } else {
        const size_t uo = plane + (size_t)ca * Wh + (size_t)cb;
        sb += 4u * im.src[uo];
        sr += 4u * im.src[uo + plane / 4];
      }
      cells[u] = pack_cell(sl, sb, sr);
    }
  }
  __syncthreads();

  // 2. the filter: cells (ca + k, cb + e), k < ROWS, e < 2, per thread
  const int g = threadIdx.x & 31, strip = threadIdx.x >> 5;
  const int cb = cb0 + 2 * g, ca = ca0 + strip * ROWS;
  if (cb >= Wc || ca >= Hc) return;                   // (no barrier follows)
  // staged column of cell column cb - R + j is 2 g + CO + j
  constexpr int CO = 2 * HG - R;
  auto at = [&](int lr, int c) __attribute__((always_inline)) {         // staged row lr, staged column 2 g + c
    return cells[lr * LW + (c & 1) * HALF + g + (c >> 1)];
  };
  const int ntl = -a.tl4 - 1, ntc = -a.tc4 - 1;       // |d| <= t  <=>  |d| - t - 1 < 0
  const int S = a.strength_q6;
  // (block-uniform) every staged cell the block's windows reach lies inside the grid
  const bool interior = ca0 - R >= 0 && ca0 + TILE_CH + R <= Hc && cb0 - R >= 0 && cb0 + TILE_CW + R <= Wc;

  // the loops over the thread's cell rows and over a window's rows stay loops: unrolled, the scheduler lifts every LDS
  // read to the top and the kernel spills
#pragma unroll 1
  for (int k = 0; k < ROWS; ++k) {
    const int ck = ca + k;
    if (ck >= Hc) break;
    // the two rows of the thread's own pixels on the RGB dword path, asked for before the window is walked (a row below
    // the image: the last row's)
    uint32_t px[2][3];
    if constexpr (RGB) {
      if (fast) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const uint32_t* sp = reinterpret_cast<const uint32_t*>(im.src + (size_t)min(2 * ck + i, H - 1) * pitch + (size_t)cb * 6);
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) px[i][ch] = sp[ch];
        }
      }
    }
    uint32_t pl[2], pb[2], pr[2];                     // the thread's two cells of this row, unpacked
    uint32_t cnt[2] = {0, 0}, sumb[2] = {0, 0}, sumr[2] = {0, 0};       // n, and the sums of the biased SB and SR over T
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const uint32_t v = at(strip * ROWS + k + R, CO + R + e);
      pl[e] = v & 0x3ffu; pb[e] = (v >> 10) & 0x7ffu; pr[e] = v >> 21;
    }
    auto window = [&]<bool EDGE>() __attribute__((always_inline)) {
#pragma unroll 1
      for (int i = 0; i < N; ++i) {                   // staged row strip ROWS + k + i = cell row ck - R + i
        const bool row_in = (unsigned)(ck - R + i) < (unsigned)Hc;
#pragma unroll
        for (int j = 0; j < N + 1; ++j) {             // cell column cb - R + j
          const uint32_t v = at(strip * ROWS + k + i, CO + j);
          uint32_t ql = v & 0x3ffu;
          const uint32_t qb = (v >> 10) & 0x7ffu, qr = v >> 21;
          if constexpr (EDGE) {
            if (!(row_in && (unsigned)(cb - R + j) < (unsigned)Wc)) ql = 1u << 20;      // no threshold accepts it
          }
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            if (j - e < 0 || j - e >= N) continue;    // (compile-time) outside cell e's window
            const int m = max(max(sad(ql, pl[e], ntl), sad(qb, pb[e], ntc)), sad(qr, pr[e], ntc));
            const uint32_t ok = (uint32_t)m >> 31;    // 1: the tap passes
            cnt[e] += ok;
            sumb[e] = __umul24(qb, ok) + sumb[e];
            sumr[e] = __umul24(qr, ok) + sumr[e];
          }
        }
      }
    };
    if (interior) window.template operator()<false>();
    else window.template operator()<true>();

    // 3. the deltas and the pixels
    int db[2], dr[2], dg[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int n = max((int)cnt[e], 1);              // (the cell itself always passes; a cell outside the grid has none)
      const int DB = (int)sumb[e] - n * (int)pb[e], DR = (int)sumr[e] - n * (int)pr[e];
      db[e] = floor_div_512n(2 * DB * S + 256 * n, n);
      dr[e] = floor_div_512n(2 * DR * S + 256 * n, n);
      dg[e] = green_delta(dr[e], db[e]);
    }
    if constexpr (RGB) {
      if (fast) {
        using u8::add_sat4;
        using u8::pair;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int r = 2 * ck + i;
          if (r >= H) continue;
          uint32_t* dp = reinterpret_cast<uint32_t*>(im.dst + (size_t)r * pitch + (size_t)cb * 6);
          dp[0] = add_sat4(px[i][0], pair(dr[0], dg[0]), pair(db[0], dr[0]));   // R0 G0 B0 R1
          dp[1] = add_sat4(px[i][1], pair(dg[0], db[0]), pair(dr[1], dg[1]));   // G1 B1 R2 G2
          dp[2] = add_sat4(px[i][2], pair(db[1], dr[1]), pair(dg[1], db[1]));   // B2 R3 G3 B3
        }
      } else {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          if (cb + e >= Wc) continue;
          const int d3[3] = {dr[e], dg[e], db[e]};
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              const int r = 2 * ck + i, c = 2 * (cb + e) + j;
              if (r >= H || c >= W) continue;
              const size_t off = (size_t)r * pitch + (size_t)c * 3;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) im.dst[off + ch] = (uint8_t)clampi((int)im.src[off + ch] + d3[ch], 0, 255);
            }
        }
      }
    } else {
      // U and V of the thread's two cells (their own values are the staged SB / 4 and SR / 4)
      const size_t uo = plane + (size_t)ck * Wh + (size_t)cb;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if (cb + e >= Wc) continue;
        im.dst[uo + e] = (uint8_t)clampi((int)((pb[e] - BIAS) >> 2) + db[e], 0, 255);
        im.dst[uo + plane / 4 + e] = (uint8_t)clampi((int)((pr[e] - BIAS) >> 2) + dr[e], 0, 255);
      }
    }
  }
}

template <bool RGB>
static int launch_r(const Args& a, int radius, hipStream_t stream) {
  const int Hc = (a.H + 1) / 2, Wc = (a.W + 1) / 2;
  const dim3 grid((unsigned)((Wc + TILE_CW - 1) / TILE_CW), (unsigned)((Hc + TILE_CH - 1) / TILE_CH), (unsigned)a.n_images);
  if (radius == 1)
    hipLaunchKernelGGL((chroma_denoise_kernel<RGB, 1>), grid, dim3(THREADS), 0, stream, a);
  else if (radius == 2)
    hipLaunchKernelGGL((chroma_denoise_kernel<RGB, 2>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((chroma_denoise_kernel<RGB, 3>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, bool rgb, int radius, hipStream_t stream) {
  if (a.n_images <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return rgb ? launch_r<true>(a, radius, stream) : launch_r<false>(a, radius, stream);
}

}  // namespace cdn
