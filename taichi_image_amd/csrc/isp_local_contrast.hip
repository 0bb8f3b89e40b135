// Local contrast kernels (isp_local_contrast.h; the contract is DESIGN.md 3, "Local contrast").
//
// For a u8 image of H x W pixels in Ty x Tx tiles, every value a signed integer, >> arithmetic, / floor division:
//   L = (77 R + 150 G + 29 B + 128) >> 8                       (the Y byte itself for a plane)
//   tile (i, j) = rows [i H / Ty, (i + 1) H / Ty) x columns [j W / Tx, (j + 1) W / Tx), n pixels, h[v] = #{L == v}
//   C != 0: c = max(1, (C n) >> 16); e = sum max(h[v] - c, 0); h[v] = min(h[v], c) + (e >> 8);
//           r = e & 255, s = max(256 / r, 1): h[k s] += 1 for k < r
//   lut[v] = (2 * 255 * cdf[v] + n) / (2 n)
//   per axis: N = (2 m + 1) T - M, i0 = N / (2 M), w = (256 (N - 2 M i0)) / (2 M), a = clamp(i0), b = clamp(i0 + 1)
//   E = the (wy, wx) blend of the four LUTs at L, + 32768 >> 16;  delta = ((E - L) S + 32) >> 6;  out_c = clamp(I_c + delta)
//
// 0. zero_kernel clears the histograms of the launch.
// 1. hist_kernel: a work-group counts a strip of rows of one tile into LDS (one histogram per wave, equal neighbours of a
//    thread's four pixels folded into one add) and adds its non-empty bins to the tile's u32[256] in the workspace.
// 2. lut_kernel: one 256-thread block per (image, tile): clip, closed-form redistribution, prefix sum, LUT as u8.
// 3. apply_kernel: a 128 x 64 block; the 2 x 2 LUT cells its pixels can touch go to LDS packed four bytes to a dword
//    (lut[ay][ax], lut[ay][bx], lut[by][ax], lut[by][bx] at one L), so a pixel takes ONE LDS read; the (cell, w) of its 64
//    rows and 128 columns come from one exact 32-bit integer division each.  Integer adds in 1. make the histograms
//    independent of the arrival order; no block waits for another.
#include "isp_local_contrast.h"

namespace lc {

using u8::byte_of;
using u8::clampi;
using u8::Image;
using u8::luma4;

constexpr int HIST_COPIES = THREADS / 64;          // one histogram per wave (the decision: DESIGN.md 5.7)

// the first row / column of tile i of an axis of M pixels in T tiles (tile T: one past the last)
MI_DEV int tile_edge(int i, int M, int T) { return i * M / T; }

// counts the up to four lumas of l4 whose bit in `valid` is set into h
MI_DEV void count4(uint32_t* h, uint32_t l4, uint32_t valid) {
  int prev = -1;
  uint32_t run = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if ((valid >> j) & 1u) {
      const int v = byte_of(l4, j);
      if (v == prev) {
        ++run;
      } else {
        if (run) atomicAdd(&h[prev], run);
        prev = v;
        run = 1;
      }
    }
  }
  if (run) atomicAdd(&h[prev], run);
}

// the histograms of a launch set to zero, 16 bytes per thread.  A kernel and not hipMemsetAsync: with the memset (ROCm
// 7.2.0, the step captured by torch.cuda.graph) test_graph_capture_of_a_step passed its first replay and failed its second
// with the LUTs of doubled counts, in one run; the cause in the runtime was not looked for, and a kernel node needs none
__global__ void __launch_bounds__(THREADS) zero_kernel(uint4* p, size_t n16) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// grid (strips of a tile, Ty * Tx, n_images)
template <bool RGB>
__global__ void __launch_bounds__(THREADS) hist_kernel(const Args a) {
  constexpr int CH = RGB ? 3 : 1;
  constexpr int UNR = 4;                              // loads in flight per thread
  __shared__ uint32_t hist[HIST_COPIES][256];
  for (int k = 0; k < HIST_COPIES; ++k) hist[k][threadIdx.x] = 0;
  __syncthreads();

  const Image im = a.im[blockIdx.z];
  const int H = a.H, W = a.W;
  const int ti = blockIdx.y / a.Tx, tj = blockIdx.y - ti * a.Tx;
  const int x0 = tile_edge(tj, W, a.Tx), x1 = tile_edge(tj + 1, W, a.Tx);
  const int y0 = tile_edge(ti, H, a.Ty) + blockIdx.x * a.strip_rows;
  const int y1 = min(y0 + a.strip_rows, tile_edge(ti + 1, H, a.Ty));
  const int rows = y1 - y0;                           // (block-uniform; <= 0: a strip past the tile's last row)
  uint32_t* h = hist[threadIdx.x >> 6];
  const size_t pitch = (size_t)W * CH;

  if (rows > 0) {
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(im.src) & 3) == 0) {
      // the dword path: 4-pixel groups at multiples of 4 columns (aligned, wholly inside the row), the groups that
      // straddle the tile's first and last column counted under a mask; work item u = row * G + g, stepped without dividing
      const int g0 = x0 >> 2, G = ((x1 + 3) >> 2) - g0, total = rows * G;
      const int qs = THREADS / G, rs = THREADS - qs * G;
      int row = threadIdx.x / G, g = threadIdx.x - row * G;
      for (int base = 0; base < total; base += THREADS * UNR) {
        uint32_t q[UNR][CH];
        int xg[UNR];
        bool ok[UNR];
#pragma unroll
        for (int k = 0; k < UNR; ++k) {
          ok[k] = row < rows;
          xg[k] = (g0 + g) * 4;
          const uint32_t* p =
              reinterpret_cast<const uint32_t*>(im.src + (size_t)(y0 + (ok[k] ? row : 0)) * pitch + (size_t)xg[k] * CH);
#pragma unroll
          for (int ch = 0; ch < CH; ++ch) q[k][ch] = p[ch];
          row += qs;
          g += rs;
          if (g >= G) {
            g -= G;
            ++row;
          }
        }
#pragma unroll
        for (int k = 0; k < UNR; ++k) {
          uint32_t l4;
          if constexpr (RGB) l4 = luma4(q[k][0], q[k][1], q[k][2]);
          else l4 = q[k][0];
          uint32_t valid = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) valid |= (uint32_t)(ok[k] && xg[k] + j >= x0 && xg[k] + j < x1) << j;
          count4(h, l4, valid);
        }
      }
    } else {
      const int tw = x1 - x0, total = rows * tw;
      const int qs = THREADS / tw, rs = THREADS - qs * tw;
      int row = threadIdx.x / tw, c = threadIdx.x - row * tw;
      for (int base = 0; base < total; base += THREADS) {
        const bool ok = row < rows;
        uint32_t l = 0;
        if (ok) {
          const uint8_t* p = im.src + (size_t)(y0 + row) * pitch + (size_t)(x0 + c) * CH;
          if constexpr (RGB) l = (77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8;
          else l = p[0];
        }
        count4(h, l, ok ? 1u : 0u);
        row += qs;
        c += rs;
        if (c >= tw) {
          c -= tw;
          ++row;
        }
      }
    }
  }
  __syncthreads();
  uint32_t sum = 0;
  for (int k = 0; k < HIST_COPIES; ++k) sum += hist[k][threadIdx.x];
  if (sum) atomicAdd(&a.hist[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * 256 + threadIdx.x], sum);
}

// grid (Ty * Tx, n_images); thread v owns bin v
__global__ void __launch_bounds__(THREADS) lut_kernel(const Args a) {
  __shared__ uint32_t s[2][256];
  const int v = threadIdx.x;
  const int ti = blockIdx.x / a.Tx, tj = blockIdx.x - ti * a.Tx;
  const uint32_t n = (uint32_t)((tile_edge(ti + 1, a.H, a.Ty) - tile_edge(ti, a.H, a.Ty)) *
                                (tile_edge(tj + 1, a.W, a.Tx) - tile_edge(tj, a.W, a.Tx)));
  const size_t at = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + v;
  uint32_t h = a.hist[at];
  if (a.clip_q8) {
    const uint64_t cn = ((uint64_t)(uint32_t)a.clip_q8 * n) >> 16;
    const uint32_t c = cn < 1 ? 1u : (uint32_t)cn;    // (C <= 16384: c <= n / 4)
    s[0][v] = h > c ? h - c : 0u;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {      // e <= n < 2^31
      if (v < step) s[0][v] += s[0][v + step];
      __syncthreads();
    }
    const uint32_t e = s[0][0];
    __syncthreads();
    h = min(h, c) + (e >> 8);
    const uint32_t r = e & 255u;
    if (r) {
      const uint32_t st = 256u / r;                   // >= 1 as r <= 255
      const uint32_t k = (uint32_t)v / st;
      if (k * st == (uint32_t)v && k < r) ++h;
    }
  }
  // inclusive prefix sum over the 256 bins
  int cur = 0;
  s[0][v] = h;
  __syncthreads();
  for (int step = 1; step < 256; step <<= 1) {
    s[cur ^ 1][v] = s[cur][v] + (v >= step ? s[cur][v - step] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  const uint64_t cdf = s[cur][v];
  a.lut[at] = (uint8_t)((2u * 255u * cdf + n) / (2u * (uint64_t)n));
}

// (i0 + 1) * 256 + w of position m of an axis of M pixels in T tiles: N + 2 M = 2 M (i0 + 1) + rem with 0 <= rem < 2 M,
// so floor(256 (N + 2 M) / (2 M)) = 256 (i0 + 1) + floor(256 rem / (2 M)); 256 (N + 2 M) < 2^30
MI_DEV uint32_t axis_q(int m, int M, int T) {
  const uint32_t n2 = (uint32_t)((2 * m + 1) * T + M);
  return (n2 * 256u) / (2u * (uint32_t)M);
}

// grid (ceil(W / BLOCK_W), ceil(H / BLOCK_H), n_images)
template <bool RGB>
__global__ void __launch_bounds__(THREADS) apply_kernel(const Args a) {
  constexpr int CH = RGB ? 3 : 1;
  __shared__ uint32_t cell[LDS_CELLS * 256];          // cell (cy, cx), luma L: the four LUT bytes its blend reads
  __shared__ uint32_t qrow[BLOCK_H], qcol[BLOCK_W];   // axis_q of the block's rows and columns

  const Image im = a.im[blockIdx.z];
  const int H = a.H, W = a.W, Ty = a.Ty, Tx = a.Tx;
  const int c0 = blockIdx.x * BLOCK_W, r0 = blockIdx.y * BLOCK_H;
  const size_t pitch = (size_t)W * CH;
  const uint8_t* lut = a.lut + (size_t)blockIdx.z * Ty * Tx * 256;
  const bool fast = u8::rows_are_dwords(im, W);

  if (threadIdx.x < BLOCK_H) qrow[threadIdx.x] = axis_q(min(r0 + (int)threadIdx.x, H - 1), H, Ty);
  else if (threadIdx.x < BLOCK_H + BLOCK_W) qcol[threadIdx.x - BLOCK_H] = axis_q(min(c0 + (int)threadIdx.x - BLOCK_H, W - 1), W, Tx);
  // the cells of the block: i0 + 1 of its first and last row and column (axis_q grows with m)
  const int cy0 = (int)(axis_q(r0, H, Ty) >> 8), cy1 = (int)(axis_q(min(r0 + BLOCK_H, H) - 1, H, Ty) >> 8);
  const int cx0 = (int)(axis_q(c0, W, Tx) >> 8), cx1 = (int)(axis_q(min(c0 + BLOCK_W, W) - 1, W, Tx) >> 8);
  const int ncx = cx1 - cx0 + 1, ncells = (cy1 - cy0 + 1) * ncx;
  const bool in_lds = ncells <= LDS_CELLS;            // (block-uniform)
  if (in_lds) {
    // work item: four consecutive lumas of one cell: a dword of each of its four LUTs, transposed into four cell dwords
    for (int u = threadIdx.x; u < ncells * 64; u += THREADS) {
      const int ci = u >> 6, l = (u & 63) * 4;
      const int cy = ci / ncx, cx = ci - cy * ncx;
      const int ay = clampi(cy0 + cy - 1, 0, Ty - 1), by = clampi(cy0 + cy, 0, Ty - 1);
      const int ax = clampi(cx0 + cx - 1, 0, Tx - 1), bx = clampi(cx0 + cx, 0, Tx - 1);
      const uint32_t d00 = *reinterpret_cast<const uint32_t*>(lut + (ay * Tx + ax) * 256 + l);
      const uint32_t d01 = *reinterpret_cast<const uint32_t*>(lut + (ay * Tx + bx) * 256 + l);
      const uint32_t d10 = *reinterpret_cast<const uint32_t*>(lut + (by * Tx + ax) * 256 + l);
      const uint32_t d11 = *reinterpret_cast<const uint32_t*>(lut + (by * Tx + bx) * 256 + l);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        cell[ci * 256 + l + j] = (uint32_t)byte_of(d00, j) | ((uint32_t)byte_of(d01, j) << 8) |
                                 ((uint32_t)byte_of(d10, j) << 16) | ((uint32_t)byte_of(d11, j) << 24);
    }
  }
  __syncthreads();

  const int g = threadIdx.x & 31, strip = threadIdx.x >> 5;
  const int c = c0 + 4 * g, rs = r0 + strip * ROWS;   // the thread's first pixel
  if (c >= W || rs >= H) return;                      // (no barrier follows)
  const int S = a.strength_q6;
  uint32_t px[ROWS][CH];
  if (fast) {
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      const uint32_t* sp = reinterpret_cast<const uint32_t*>(im.src + (size_t)min(rs + k, H - 1) * pitch + (size_t)c * CH);
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) px[k][ch] = sp[ch];
    }
  }
  uint32_t qx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) qx[j] = qcol[4 * g + j];

#pragma unroll
  for (int k = 0; k < ROWS; ++k) {
    const int r = rs + k;
    if (r >= H) break;
    const uint32_t qy = qrow[strip * ROWS + k];
    const int wy = (int)(qy & 255u), cy = (int)(qy >> 8);
    const size_t off = (size_t)r * pitch + (size_t)c * CH;
    uint32_t l4;
    if (fast) {
      if constexpr (RGB) l4 = luma4(px[k][0], px[k][1], px[k][2]);
      else l4 = px[k][0];
    } else {
      l4 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < W) {
          const uint8_t* p = im.src + off + j * CH;
          uint32_t l;
          if constexpr (RGB) l = (77u * p[0] + 150u * p[1] + 29u * p[2] + 128u) >> 8;
          else l = p[0];
          l4 |= l << (8 * j);
        }
    }
    int delta[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int L = byte_of(l4, j);
      const int wx = (int)(qx[j] & 255u), cx = (int)(qx[j] >> 8);
      uint32_t t;
      if (in_lds) {
        t = cell[((cy - cy0) * ncx + (cx - cx0)) * 256 + L];
      } else {
        const int ay = clampi(cy - 1, 0, Ty - 1), by = clampi(cy, 0, Ty - 1);
        const int ax = clampi(cx - 1, 0, Tx - 1), bx = clampi(cx, 0, Tx - 1);
        t = (uint32_t)lut[(ay * Tx + ax) * 256 + L] | ((uint32_t)lut[(ay * Tx + bx) * 256 + L] << 8) |
            ((uint32_t)lut[(by * Tx + ax) * 256 + L] << 16) | ((uint32_t)lut[(by * Tx + bx) * 256 + L] << 24);
      }
      const int l00 = byte_of(t, 0), l01 = byte_of(t, 1), l10 = byte_of(t, 2), l11 = byte_of(t, 3);
      const int top = (l00 << 8) + wx * (l01 - l00);  // (256 - wx) l00 + wx l01
      const int bot = (l10 << 8) + wx * (l11 - l10);
      const int E = ((top << 8) + wy * (bot - top) + 32768) >> 16;
      delta[j] = ((E - L) * S + 32) >> 6;             // floor: an arithmetic shift
    }
    if (fast) {
      u8::store_delta4<RGB>(im.dst + off, px[k], delta);
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
}

template <bool RGB>
static int launch_c(Args& a, hipStream_t stream) {
  const int T = a.Ty * a.Tx;
  const int tw = (a.W + a.Tx - 1) / a.Tx, th = (a.H + a.Ty - 1) / a.Ty;          // the largest tile
  a.strip_rows = STRIP_PIXELS / tw < 1 ? 1 : (STRIP_PIXELS / tw > th ? th : STRIP_PIXELS / tw);
  const size_t n16 = hist_bytes(a.n_images, a.Ty, a.Tx) / 16;
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)((n16 + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                     reinterpret_cast<uint4*>(a.hist), n16);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(hist_kernel<RGB>, dim3((unsigned)((th + a.strip_rows - 1) / a.strip_rows), (unsigned)T, (unsigned)a.n_images),
                     dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(lut_kernel, dim3((unsigned)T, (unsigned)a.n_images), dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  hipLaunchKernelGGL(apply_kernel<RGB>,
                     dim3((unsigned)((a.W + BLOCK_W - 1) / BLOCK_W), (unsigned)((a.H + BLOCK_H - 1) / BLOCK_H), (unsigned)a.n_images),
                     dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(Args& a, bool rgb, hipStream_t stream) {
  if (a.n_images <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return rgb ? launch_c<true>(a, stream) : launch_c<false>(a, stream);
}

}  // namespace lc
