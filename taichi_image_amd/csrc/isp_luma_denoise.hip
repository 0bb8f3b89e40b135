// Luma noise reduction kernels (isp_luma_denoise.h; the contract is DESIGN.md 3, "Luma noise reduction").
//
// For pixel p of a u8 image, every value a signed 32-bit integer, >> arithmetic:
//   L = (77 R + 150 G + 29 B + 128) >> 8                       (the Y byte itself for a plane)
//   T = t0 + (((t1 - t0) L(p) + 128) >> 8)
//   n, s = the count and the luma sum of the taps q of the (2r + 1)^2 window INSIDE the image with |L(q) - L(p)| <= T
//   m = floor((2 s + n) / (2 n));  delta = (S (m - L(p)) + 32) >> 6;  out_c = clamp(I_c + delta, 0, 255)
//
// One 256-thread block per 128 x 64 output tile of one image (grid.z).  1. The luma of the tile and of four columns and r
// rows around it is staged ONCE into LDS, four pixels to a dword, as the sharpening kernel stages it (u8::stage_luma):
// three dwords per four pixels and six byte dot products where the rows allow (W % 4 == 0 and 4-byte aligned images),
// every load of the thread issued before the first is used; byte by byte otherwise.  A pixel outside the image is staged
// from a clamped address and never used as a tap.  2. Lane g of a half wave owns columns 4g .. 4g + 3, the block's 8
// strips 8 rows each.  Per pair of output rows the thread walks the 2r + 2 staged rows of their windows: three ds_read_b32
// at consecutive dwords over the half wave (no bank conflict) give the 4 + 2r lumas the windows share.  The taps run on
// 16-bit pairs: the thread's pixels e and e + 1 take their tap j from the staged pixels e + j and e + j + 1, which one
// v_perm_b32 widens to a pair, so a packed instruction serves two taps.  A tap counts when lo <= L(q) <= lo + 2 T with lo =
// L(p) - T, which in wrapping 16-bit arithmetic is (L(q) - lo) <= 2 T: v_pk_sub_u16, v_pk_sub_u16 clamp (2 T + 1 minus
// that, saturating at 0) and v_pk_min_u16 with 1 give the pair of 0 / 1, v_pk_mad_u16 adds the counting lumas (s <= 49 x
// 255 fits 16 bits) and v_pk_add_u16 the counts: five instructions for two taps.  No branch looks at a tap.  A block whose
// windows all stay inside the image runs without the inside test; the others give a pixel outside the image the value
// 0x7fff, which no threshold accepts (one v_or3_b32 per pair).  3. The four pixels, read as three dwords (one for a plane)
// before the window is walked, take the deltas as packed 16-bit adds with a saturating pack (u8::store_delta4); byte by byte
// on the other path.
#include "isp_luma_denoise.h"

namespace ydn {

using namespace u8;                                   // the images, the tile, the byte helpers, the staging and the write-back

constexpr uint32_t OUTSIDE = 0x7fffu;                 // a pixel outside the image, as a 16-bit luma: 0x7fff - lo > 2 T always

// two taps, every operand a pair of 16-bit values: ok = (v - lo) mod 2^16 <= lim - 1 ? 1 : 0, sum += ok v, cnt += ok.  One
// statement, so that the compiler neither turns the 0 / 1 into compares and selects nor pads between the five
// instructions (plain VALU results feeding plain VALU operands need no wait states).
MI_DEV void tap2(uint32_t& sum, uint32_t& cnt, uint32_t v, uint32_t lo, uint32_t lim, uint32_t one) {
  uint32_t t;
  asm("v_pk_sub_u16 %2, %3, %4\n\t"
      "v_pk_sub_u16 %2, %5, %2 clamp\n\t"
      "v_pk_min_u16 %2, %2, %6\n\t"
      "v_pk_mad_u16 %0, %2, %3, %0\n\t"
      "v_pk_add_u16 %1, %1, %2"
      : "+v"(sum), "+v"(cnt), "=&v"(t)
      : "v"(v), "v"(lo), "v"(lim), "v"(one));
}

// bytes B and B + 1 of the twelve bytes d[0] d[1] d[2], widened to a 16-bit pair (selector bytes 0-3 pick from the second
// operand of v_perm_b32, 4-7 from the first, 0x0c gives zero)
template <int B>
MI_DEV uint32_t pair_at(const uint32_t (&d)[3]) {
  constexpr int A = B + 1;
  constexpr uint32_t hi = (A >> 2) != (B >> 2) ? 4u : (uint32_t)(A & 3);
  return __builtin_amdgcn_perm(d[A >> 2], d[B >> 2], 0x0c000c00u | (hi << 16) | (uint32_t)(B & 3));
}

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_images)
template <bool RGB, int R>
__global__ void __launch_bounds__(THREADS) luma_denoise_kernel(const Args a) {
  constexpr int CH = RGB ? 3 : 1;                     // bytes per pixel
  constexpr int LH = TILE_H + 2 * R;                  // staged rows
  constexpr int N = 2 * R + 1;                        // window side
  constexpr int NQ = 3 + 2 * R;                       // pairs of neighbouring staged pixels that the thread's windows use
  __shared__ uint32_t lum[LH * LG];                   // row lr = image row r0 - R + lr, dword lg = columns c0 - 4 + 4 lg ..

  const Image im = a.im[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;
  const size_t pitch = (size_t)W * CH;
  const bool fast = rows_are_dwords(im, W);

  // 1. the luma of the tile and its surround.  A pixel outside the image is never a tap: its load is clamped into the
  // image and what it gives is not used.
  if (fast) {
    stage_luma<RGB, R, false>(lum, im, H, W, r0, c0);
  } else {
    for (int u = threadIdx.x; u < LH * LG; u += THREADS) {
      const int lr = u / LG, lg = u - lr * LG;
      const int r = clampi(r0 - R + lr, 0, H - 1), c = c0 - 4 + 4 * lg;
      const uint8_t* row = im.src + (size_t)r * pitch;
      uint32_t l4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* p = row + (size_t)clampi(c + j, 0, W - 1) * CH;
        uint32_t l;
        if constexpr (RGB) l = (77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8;
        else l = p[0];
        l4 |= l << (8 * j);
      }
      lum[u] = l4;
    }
  }
  __syncthreads();

  // 2. the filter: four columns per thread, ROWS rows one below the other
  const int g = threadIdx.x & 31, strip = threadIdx.x >> 5;
  const int c = c0 + 4 * g, rs = r0 + strip * ROWS;   // the thread's first pixel
  if (c >= W || rs >= H) return;                      // (no barrier follows)
  const int t0 = a.t0, t1 = a.t1, S = a.strength_q6;
  // (block-uniform) every staged pixel the block's windows reach lies inside the image
  const bool interior = r0 - R >= 0 && r0 + TILE_H + R <= H && c0 - R >= 0 && c0 + TILE_W + R <= W;
  // pair t of a staged row: columns c - R + t and c - R + t + 1; a column outside the image takes OUTSIDE
  uint32_t colbad[NQ];
#pragma unroll
  for (int t = 0; t < NQ; ++t)
    colbad[t] = ((unsigned)(c - R + t) < (unsigned)W ? 0u : OUTSIDE) | ((unsigned)(c - R + t + 1) < (unsigned)W ? 0u : OUTSIDE << 16);

  // The thread takes its rows two at a time: the windows of rows r and r + 1 share 2 R of their 2 R + 1 staged rows, so
  // one walk over 2 R + 2 staged rows reads and widens each row once for both (the first row serves r alone, the last
  // r + 1 alone).  The loops over the pairs of rows and over the staged rows stay loops, as in the chroma kernel
  // (isp_chroma_denoise.hip), which spilled when they were unrolled.
#pragma unroll 1
  for (int k = 0; k < ROWS; k += 2) {
    const int r = rs + k;
    if (r >= H) break;
    const bool second = r + 1 < H;                    // (a row below the image is computed from staged rows and not stored)
    const size_t off = (size_t)r * pitch + (size_t)c * CH;
    // the thread's own pixels of the dword path, asked for before the window is walked
    uint32_t px[2][CH];
    if (fast) {
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const uint32_t* sp = reinterpret_cast<const uint32_t*>(im.src + (v && second ? off + pitch : off));
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) px[v][ch] = sp[ch];
      }
    }
    int L0[2][4];
    uint32_t lo[2][2], lim[2][2], cnt[2][2], sum[2][2];                 // per row, 16-bit pairs of pixels (0, 1) and (2, 3):
#pragma unroll                                                          // L(p) - T, 2 T + 1, n, s
    for (int v = 0; v < 2; ++v) {
      const uint32_t ctr = lum[(strip * ROWS + k + v + R) * LG + g + 1];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int T[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          L0[v][2 * h + e] = byte_of(ctr, 2 * h + e);
          T[e] = threshold_at(t0, t1, L0[v][2 * h + e]);
        }
        lo[v][h] = (uint32_t)((L0[v][2 * h] - T[0]) & 0xffff) | (uint32_t)(L0[v][2 * h + 1] - T[1]) << 16;
        lim[v][h] = (uint32_t)(2 * T[0] + 1) | (uint32_t)(2 * T[1] + 1) << 16;
        cnt[v][h] = sum[v][h] = 0;
      }
    }
    // staged row strip ROWS + k + i = image row r - R + i, for the rows v of the pair with FIRST <= v <= LAST
    auto staged_row = [&]<bool EDGE, int FIRST, int LAST>(int i) __attribute__((always_inline)) {
      const uint32_t* p = &lum[(strip * ROWS + k + i) * LG + g];
      const uint32_t d[3] = {p[0], p[1], p[2]};       // the lumas of columns c - 4 .. c + 7, a byte each
      uint32_t q[NQ];                                 // pair t: staged pixels t and t + 1, bytes 4 - R + t and 5 - R + t
      if constexpr (R == 1) {
        q[0] = pair_at<3>(d); q[1] = pair_at<4>(d); q[2] = pair_at<5>(d); q[3] = pair_at<6>(d); q[4] = pair_at<7>(d);
      } else if constexpr (R == 2) {
        q[0] = pair_at<2>(d); q[1] = pair_at<3>(d); q[2] = pair_at<4>(d); q[3] = pair_at<5>(d); q[4] = pair_at<6>(d);
        q[5] = pair_at<7>(d); q[6] = pair_at<8>(d);
      } else {
        q[0] = pair_at<1>(d); q[1] = pair_at<2>(d); q[2] = pair_at<3>(d); q[3] = pair_at<4>(d); q[4] = pair_at<5>(d);
        q[5] = pair_at<6>(d); q[6] = pair_at<7>(d); q[7] = pair_at<8>(d); q[8] = pair_at<9>(d);
      }
      if constexpr (EDGE) {
        const uint32_t rowbad = (unsigned)(r - R + i) < (unsigned)H ? 0u : OUTSIDE | OUTSIDE << 16;
#pragma unroll
        for (int t = 0; t < NQ; ++t) q[t] |= colbad[t] | rowbad;
      }
#pragma unroll
      for (int v = FIRST; v <= LAST; ++v)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < N; ++j) tap2(sum[v][h], cnt[v][h], q[2 * h + j], lo[v][h], lim[v][h], 0x00010001u);      // tap j of both pixels
    };
    auto window = [&]<bool EDGE>() __attribute__((always_inline)) {
      staged_row.template operator()<EDGE, 0, 0>(0);
#pragma unroll 1
      for (int i = 1; i < N; ++i) staged_row.template operator()<EDGE, 0, 1>(i);
      staged_row.template operator()<EDGE, 1, 1>(N);
    };
    if (interior) window.template operator()<false>();
    else window.template operator()<true>();

#pragma unroll
    for (int v = 0; v < 2; ++v) {
      if (v && !second) break;
      int delta[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int sh = 16 * (e & 1);                  // (a pixel outside the image has n = 0: its m is not used)
        const int m = mean_ties_up((int)(sum[v][e >> 1] >> sh & 0xffffu), (int)(cnt[v][e >> 1] >> sh & 0xffffu));
        delta[e] = (__mul24(S, m - L0[v][e]) + 32) >> 6;                // floor: an arithmetic shift
      }
      // 3. the pixels
      const size_t o = v ? off + pitch : off;
      if (fast) {
        store_delta4<RGB>(im.dst + o, px[v], delta);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < W) {
#pragma unroll
            for (int ch = 0; ch < CH; ++ch)
              im.dst[o + j * CH + ch] = (uint8_t)clampi((int)im.src[o + j * CH + ch] + delta[j], 0, 255);
          }
      }
    }
  }
}

template <bool RGB>
static int launch_r(const Args& a, int radius, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_images);
  if (radius == 1)
    hipLaunchKernelGGL((luma_denoise_kernel<RGB, 1>), grid, dim3(THREADS), 0, stream, a);
  else if (radius == 2)
    hipLaunchKernelGGL((luma_denoise_kernel<RGB, 2>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((luma_denoise_kernel<RGB, 3>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, bool rgb, int radius, hipStream_t stream) {
  if (a.n_images <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return rgb ? launch_r<true>(a, radius, stream) : launch_r<false>(a, radius, stream);
}

}  // namespace ydn
