// Frame statistics kernels (isp_statistics.h; the contract is DESIGN.md 3, "Frame statistics").
//
// For raw pixel p = (r, c) with x(p) its f32 pre-shading, pre-cast value, valid when it is inside the frame, not a listed
// defect and x > -inf:  v = i32(rint(min(max(x, 0), 1) * 65536)), site s = (r & 1) * 2 + (c & 1), zone (i, j) =
// (((r >> 1) gh) / (H / 2), ((c >> 1) gw) / (W / 2)), clipped x >= clip, dark x <= dark.
//   Z[i, j, s, 0..3] += 1, v, clipped, dark                    for every valid pixel
//   Hist[s, min(v >> 8, 255)] += 1                              for every valid pixel
//   F[i, j, 0..1] += L^2, 1 with L = 4 v(p) - sum of v(taps)    for every green p whose taps (r +- 2, c), (r, c +- 2) are
//                                                               valid and p and the taps have x < clip
// All sums are integers: the result does not depend on the launch geometry or on the order of the atomics.
//
// One 256-thread block per strip of a.strip consecutive 64 x 64 tiles of one tile row of one frame (grid.z).  Per tile the
// tile plus a halo of two is decoded ONCE into LDS (raw::stage_tile) and, behind a barrier, turned in place into
// words: v and the flags valid, clipped, dark and "below clip" - so a focus tap costs one LDS read and one AND.  Lane l of
// wave w takes column l of rows 16 w .. 16 w + 15 and keeps its sums in registers ACROSS the tiles of the strip, for as long
// as its zone cell stays the same: the flags of a pixel go into three 10-bit counters with one multiply.  The histogram
// takes one LDS atomic per pixel, into one of HIST_COPIES copies.  A lane whose cell changes, and every lane at the end of
// the strip, adds its registers to the block's cell table in LDS (64-bit LDS atomics) - or, when the strip spans more than
// CELLS cells (zones of a few quads), to global memory directly.  The block ends with one 64-bit global atomic per word
// of its table and per histogram bin that is not zero.
#include "isp_statistics.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace st {

typedef unsigned long long u64;

// the word of a staged pixel: bits 0 .. 16 v; an excluded pixel is 0
constexpr uint32_t V_MASK = 0x1FFFFu, VALID = 1u << 17, CLIPPED = 1u << 18, DARK = 1u << 19, BELOW = 1u << 20;
// (valid, clipped, dark) -> bits 0, 10, 20: flags * (1 + 2^9 + 2^18) puts flag k at bits k, k + 9, k + 18
constexpr uint32_t SPREAD = 0x40201u, SPREAD_MASK = 0x100401u;
static_assert(MAX_STRIP * (PX / 2) < (1 << 10), "a lane's counters are 10 bits wide");
static_assert(TILE_H * TILE_W <= (1 << 16) && (long long)MAX_STRIP * TILE_H * TILE_W * 65536 < (1ll << 62), "sums");

MI_DEV uint32_t encode(float x, float clip, float dark) {
  if (!(x > -INFINITY)) return 0u;                    // outside, a listed defect, -inf or a NaN
  const float u = fminf(fmaxf(x, 0.f), 1.f);
  const uint32_t v = (uint32_t)(int)rintf(u * 65536.f);             // (an exact product; ties to even)
  return v | VALID | (x >= clip ? CLIPPED : BELOW) | (x <= dark ? DARK : 0u);
}

// word w of zone cell `cell` in one frame's result
MI_DEV u64* cell_word(u64* out, int cell, int w, int n_cells) {
  return w < 16 ? out + (size_t)cell * 16 + w : out + (size_t)n_cells * 16 + (size_t)cell * 2 + (w - 16);
}

// grid (n_words / THREADS rounded up, n_frames): every frame's result cleared
__global__ void __launch_bounds__(THREADS) clear_kernel(const Args a, int n_words) {
  const int u = blockIdx.x * THREADS + threadIdx.x;
  if (u < n_words) a.f[blockIdx.y].out[u] = 0ull;
}

// grid (strips per tile row, ceil(H / TILE_H), n_frames)
template <int SRC>
__global__ void __launch_bounds__(THREADS) statistics_kernel(const Args a) {
  constexpr int LW = TILE_W + 2 * HALO_C;             // LDS row pitch (floats)
  constexpr int LH = TILE_H + 2 * HALO_R;
  constexpr int LP = LW / 2;
  __shared__ float xs[LH * LW];                       // x, then the words
  __shared__ uint32_t hist[HIST_COPIES * 4 * BINS];
  __shared__ u64 cells[CELLS * CELL_WORDS];
  __shared__ int zrow[TILE_H];                        // zone row of each tile row

  const Frame& fr = a.f[blockIdx.z];                  // (a wave-uniform index: scalar loads)
  const int H = a.H, W = a.W, gh = a.gh, gw = a.gw, Ha = H >> 1, Wa = W >> 1;
  const int n_cells = gh * gw;
  const int r0 = blockIdx.y * TILE_H;
  const int tiles = (W + TILE_W - 1) / TILE_W;
  const int t0 = blockIdx.x * a.strip, t1 = t0 + a.strip < tiles ? t0 + a.strip : tiles;
  const bool lds = lds_route(H, W, gh, gw, a.strip, blockIdx.x, blockIdx.y);
  const int i0 = zone_of(r0, gh, Ha), j0 = zone_of(t0 * TILE_W, gw, Wa);
  const int c_last = t1 * TILE_W - 1 < W - 1 ? t1 * TILE_W - 1 : W - 1;
  const int nj = zone_of(c_last, gw, Wa) - j0 + 1;
  u64* const out = fr.out;

  for (int u = threadIdx.x; u < HIST_COPIES * 4 * BINS; u += THREADS) hist[u] = 0u;
  for (int u = threadIdx.x; u < CELLS * CELL_WORDS; u += THREADS) cells[u] = 0ull;
  if (threadIdx.x < TILE_H) {
    const int r = r0 + threadIdx.x < H - 1 ? r0 + threadIdx.x : H - 1;
    zrow[threadIdx.x] = zone_of(r, gh, Ha);
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cp = lane & 1;                            // (tile columns start even: the column parity)
  const int gpar = a.gp ^ cp;                         // the row parity of the lane's green pixels
  const int hbase = ((lane >> 1) & (HIST_COPIES - 1)) * (4 * BINS) + cp * BINS;
  const float clip = a.clip, dark = a.dark;

  // the lane's sums since its last flush, for cell cur_g (cur_l in the block's table)
  int cur_g = -1, cur_l = 0;
  uint32_t sum[2] = {0u, 0u}, flags[2] = {0u, 0u}, fcnt = 0u;
  u64 fsum = 0ull;
  auto emit = [&](int w, u64 v) {
    if (v == 0ull) return;
    if (lds)
      atomicAdd(&cells[cur_l * CELL_WORDS + w], v);
    else
      atomicAdd(cell_word(out, cur_g, w, n_cells), v);
  };
  auto flush = [&]() {
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      const int w = (par * 2 + cp) * 4;
      emit(w, flags[par] & 0x3FFu);
      emit(w + 1, sum[par]);
      emit(w + 2, (flags[par] >> 10) & 0x3FFu);
      emit(w + 3, flags[par] >> 20);
      sum[par] = 0u; flags[par] = 0u;
    }
    emit(16, fsum);
    emit(17, fcnt);
    fsum = 0ull; fcnt = 0u;
  };

  for (int t = t0; t < t1; ++t) {
    const int c0 = t * TILE_W;
    // 1. the tile and its halo, decoded once, then turned into words in place
    raw::stage_tile<SRC, TILE_H, TILE_W, HALO_R, HALO_C, THREADS>(a, fr.src, fr.mask, r0, c0, xs);
    __syncthreads();                                  // (whichever thread staged a pair: the pass below does not rely on it)
    for (int u = threadIdx.x; u < LH * LP; u += THREADS) {
      const int lr = u / LP, lp = u - lr * LP;
      float2* q = reinterpret_cast<float2*>(&xs[lr * LW + 2 * lp]);
      const float2 x = *q;
      *q = make_float2(__uint_as_float(encode(x.x, clip, dark)), __uint_as_float(encode(x.y, clip, dark)));
    }
    __syncthreads();                                  // (also orders the clears above before the first adds)

    // 2. lane = tile column
    const int c = c0 + lane < W - 1 ? c0 + lane : W - 1;
    const int zj = zone_of(c, gw, Wa);
    for (int k2 = 0; k2 < PX / 2; ++k2) {
      const int tr = wave * PX + 2 * k2;              // the quad's first tile row (r0 and 16 wave are even)
      const int zi = zrow[tr];                        // (a quad is never split between zones)
      const int g = zi * gw + zj;
      if (g != cur_g) {
        flush();
        cur_g = g;
        cur_l = (zi - i0) * nj + (zj - j0);
      }
      const float* row = &xs[(tr + HALO_R) * LW + lane + HALO_C];
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const uint32_t w = __float_as_uint(row[par * LW]);
        const uint32_t v = w & V_MASK;
        sum[par] += v;
        flags[par] += (((w >> 17) & 7u) * SPREAD) & SPREAD_MASK;
        if (w & VALID) {
          const uint32_t bin = (v >> 8) < (uint32_t)(BINS - 1) ? (v >> 8) : (uint32_t)(BINS - 1);
          atomicAdd(&hist[hbase + par * 2 * BINS + bin], 1u);
        }
      }
      // the lane's green pixel of the quad
      const float* gq = row + gpar * LW;
      const uint32_t wc = __float_as_uint(gq[0]), wu = __float_as_uint(gq[-2 * LW]), wd = __float_as_uint(gq[2 * LW]);
      const uint32_t wl = __float_as_uint(gq[-2]), wr = __float_as_uint(gq[2]);
      if (wc & wu & wd & wl & wr & BELOW) {
        const int L = 4 * (int)(wc & V_MASK) - (int)((wu & V_MASK) + (wd & V_MASK) + (wl & V_MASK) + (wr & V_MASK));
        fsum += (u64)((long long)L * (long long)L);
        fcnt += 1u;
      }
    }
    __syncthreads();                                  // (the next tile overwrites xs)
  }
  flush();
  __syncthreads();

  // 3. the block's table and histogram: one global atomic per word that is not zero
  for (int u = threadIdx.x; u < CELLS * CELL_WORDS; u += THREADS) {
    const u64 v = cells[u];
    if (v != 0ull) {
      const int l = u / CELL_WORDS, w = u - l * CELL_WORDS;
      const int i = i0 + l / nj, j = j0 + l % nj;
      if (i < gh && j < gw) atomicAdd(cell_word(out, i * gw + j, w, n_cells), v);
    }
  }
  for (int u = threadIdx.x; u < 4 * BINS; u += THREADS) {
    u64 v = 0ull;
#pragma unroll
    for (int k = 0; k < HIST_COPIES; ++k) v += hist[k * 4 * BINS + u];
    if (v != 0ull) atomicAdd(out + (size_t)n_cells * CELL_WORDS + u, v);
  }
}

template <int SRC>
static int launch_src(const Args& a, hipStream_t stream) {
  const int tiles = (a.W + TILE_W - 1) / TILE_W;
  const dim3 grid((unsigned)((tiles + a.strip - 1) / a.strip), (unsigned)((a.H + TILE_H - 1) / TILE_H), (unsigned)a.n_frames);
  hipLaunchKernelGGL((statistics_kernel<SRC>), grid, dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int src, hipStream_t stream) {
  if (a.n_frames <= 0) return 0;
  const int n_words = (int)words(a.gh, a.gw);
  hipLaunchKernelGGL(clear_kernel, dim3((unsigned)((n_words + THREADS - 1) / THREADS), (unsigned)a.n_frames), dim3(THREADS), 0,
                     stream, a, n_words);
  MI_LAUNCH_CHECK();
  if (a.H <= 0 || a.W <= 0) return 0;
  return raw::dispatch_src(src, [&](auto s) { return launch_src<decltype(s)::value>(a, stream); });
}

}  // namespace st
