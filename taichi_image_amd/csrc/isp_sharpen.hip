// Output sharpening kernels (isp_sharpen.h; the contract is DESIGN.md 3, "Output sharpening").
//
// For pixel (y, x) of a u8 image, every value a signed 32-bit integer, >> arithmetic, coordinates clamped into the image:
//   L = (77 R + 150 G + 29 B + 128) >> 8                       (the Y byte itself for a plane)
//   Bl = sum_ij b[i] b[j] L(y + i - r, x + j - r)              b = (1, 2, 1) or (1, 4, 6, 4, 1); S = (sum b)^2 = 16 or 256
//   d = S L - Bl;  d' = sign(d) max(|d| - threshold S, 0);  delta = (A d' + (1 << (k - 1))) >> k,  k = 6 + log2 S
//   with a halo clamp: delta = clamp(L + delta, min3x3(L) - overshoot, max3x3(L) + overshoot) - L
//   out_c = clamp(I_c + delta, 0, 255)
//
// One 256-thread block per 128 x 64 output tile of one image (grid.z).  1. The luma of the tile and of four columns and r
// rows around it is staged ONCE into LDS, four pixels to a dword: where the row allows (W % 4 == 0 and 4-byte aligned
// images) a thread reads four pixels as three dwords and takes their lumas with six byte dot products, every load of the
// thread issued before the first is used (the kernel waits for memory, not for arithmetic: DESIGN.md 5.6); everything
// else goes byte by byte through the clamp.  2. Lane g of a half wave owns columns 4g .. 4g + 3, the block's 8 strips 8
// rows each: per staged row a thread reads three dwords (ds_read_b32 at consecutive dwords over the half wave: no bank
// conflict), forms the horizontal blur of its four columns with byte dot products on the packed lumas (and, with the halo
// clamp on, their 3-wide min and max), and a window of 2r + 1 such rows slides down the strip for the vertical pass - the
// 25 products are never formed.  3. The four pixels, read as three dwords (one for a plane) before the filter started,
// take the deltas as packed 16-bit adds with a saturating pack and leave as three dwords; byte by byte on the other path.
#include "isp_sharpen.h"

namespace shp {

using namespace u8;                                   // the images, the tile, the byte helpers, the staging and the write-back

// what one staged row gives a thread's four columns: their lumas (packed), the horizontal blur and the horizontal 3-wide
// min / max of each
struct RowV {
  uint32_t l4;
  int h[4], mn[4], mx[4];
};

// grid (ceil(W / TILE_W), ceil(H / TILE_H), n_images)
template <bool RGB, int R>
__global__ void __launch_bounds__(THREADS) sharpen_kernel(const Args a) {
  constexpr int CH = RGB ? 3 : 1;                     // bytes per pixel
  constexpr int LH = TILE_H + 2 * R;                  // staged rows
  constexpr int N = 2 * R + 1;                        // window side
  constexpr int LOG2S = 4 * R;                        // S = 16 or 256
  constexpr int K = 6 + LOG2S;
  __shared__ uint32_t lum[LH * LG];                   // row lr = image row r0 - R + lr, dword lg = columns c0 - 4 + 4 lg ..

  const Image im = a.im[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W;
  const int c0 = blockIdx.x * TILE_W, r0 = blockIdx.y * TILE_H;
  const size_t pitch = (size_t)W * CH;
  const bool fast = rows_are_dwords(im, W);

  // 1. the luma of the tile and its surround, coordinates clamped into the image
  if (fast) {
    stage_luma<RGB, R, true>(lum, im, H, W, r0, c0);
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

  // 2. the filter: four columns per thread, a window of N staged rows sliding down the strip
  const int g = threadIdx.x & 31, strip = threadIdx.x >> 5;
  const int c = c0 + 4 * g, rs = r0 + strip * ROWS;   // the thread's first pixel
  if (c >= W || rs >= H) return;                      // (no barrier follows)
  const bool halo = a.overshoot >= 0;                 // (wave-uniform)
  const int A = a.amount_q6, t = a.threshold << LOG2S, os = a.overshoot;
  // the thread's own pixels of the dword path, asked for before the filter runs (rows below the image: the last row's)
  uint32_t px[ROWS][CH];
  if (fast) {
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const uint32_t* sp = reinterpret_cast<const uint32_t*>(im.src + (size_t)min(rs + k, H - 1) * pitch + (size_t)c * CH);
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) px[k][ch] = sp[ch];
    }
  }

  auto load_row = [&](int lr) __attribute__((always_inline)) {
    RowV o;
    const uint32_t* p = &lum[lr * LG + g];
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];   // the lumas of columns c - 4 .. c + 7, a byte each
    o.l4 = d1;
    // the horizontal blur as byte dot products: the taps of one column lie in at most two of the dwords
    if constexpr (R == 1) {
      o.h[0] = (int)dot4(d1, 0x00000102u, dot4(d0, 0x01000000u, 0u));
      o.h[1] = (int)dot4(d1, 0x00010201u, 0u);
      o.h[2] = (int)dot4(d1, 0x01020100u, 0u);
      o.h[3] = (int)dot4(d2, 0x00000001u, dot4(d1, 0x02010000u, 0u));
    } else {
      o.h[0] = (int)dot4(d1, 0x00010406u, dot4(d0, 0x04010000u, 0u));
      o.h[1] = (int)dot4(d1, 0x01040604u, dot4(d0, 0x01000000u, 0u));
      o.h[2] = (int)dot4(d2, 0x00000001u, dot4(d1, 0x04060401u, 0u));
      o.h[3] = (int)dot4(d2, 0x00000104u, dot4(d1, 0x06040100u, 0u));
    }
    if (halo) {
      const int v[6] = {byte_of(d0, 3), byte_of(d1, 0), byte_of(d1, 1), byte_of(d1, 2), byte_of(d1, 3), byte_of(d2, 0)};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o.mn[j] = min3(v[j], v[j + 1], v[j + 2]);
        o.mx[j] = max3(v[j], v[j + 1], v[j + 2]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) o.mn[j] = o.mx[j] = 0;
    }
    return o;
  };

  RowV win[N];                                        // win[m]: image row (row of the pixel) + m - R
#pragma unroll
  for (int m = 0; m < N - 1; ++m) win[m] = load_row(strip * ROWS + m);
#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    win[N - 1] = load_row(strip * ROWS + k + N - 1);
    const int r = rs + k;
    int delta[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int bl;
      if constexpr (R == 1) bl = win[0].h[j] + 2 * win[1].h[j] + win[2].h[j];
      else bl = (win[0].h[j] + win[4].h[j]) + 4 * (win[1].h[j] + win[3].h[j]) + 6 * win[2].h[j];
      const int L = byte_of(win[R].l4, j);
      const int d = (L << LOG2S) - bl;
      const int m = max(abs(d) - t, 0);               // soft coring
      const int dc = d < 0 ? -m : m;
      int dl = (A * dc + (1 << (K - 1))) >> K;        // floor: an arithmetic shift
      if (halo) {
        const int lo = min3(win[R - 1].mn[j], win[R].mn[j], win[R + 1].mn[j]) - os;
        const int hi = max3(win[R - 1].mx[j], win[R].mx[j], win[R + 1].mx[j]) + os;
        dl = clampi(L + dl, lo, hi) - L;
      }
      delta[j] = dl;
    }
    // 3. the pixels
    if (r < H) {
      const size_t off = (size_t)r * pitch + (size_t)c * CH;
      if (fast) {
        store_delta4<RGB>(im.dst + off, px[k], delta);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < W) {
#pragma unroll
            for (int ch = 0; ch < CH; ++ch)
              im.dst[off + j * CH + ch] = (uint8_t)clampi((int)im.src[off + j * CH + ch] + delta[j], 0, 255);
          }
      }
    }
#pragma unroll
    for (int m = 0; m < N - 1; ++m) {
      win[m].l4 = win[m + 1].l4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        win[m].h[j] = win[m + 1].h[j];
        win[m].mn[j] = win[m + 1].mn[j];
        win[m].mx[j] = win[m + 1].mx[j];
      }
    }
  }
}

template <bool RGB>
static int launch_r(const Args& a, int radius, hipStream_t stream) {
  const dim3 grid((unsigned)((a.W + TILE_W - 1) / TILE_W), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_images);
  if (radius == 1)
    hipLaunchKernelGGL((sharpen_kernel<RGB, 1>), grid, dim3(THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL((sharpen_kernel<RGB, 2>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, bool rgb, int radius, hipStream_t stream) {
  if (a.n_images <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return rgb ? launch_r<true>(a, radius, stream) : launch_r<false>(a, radius, stream);
}

}  // namespace shp
