// Antialiased resize: the host's table builder and the one-launch separable kernel (isp_resample.h; DESIGN.md 3,
// "Antialiased resize", and 5.17).
#include <cmath>
#include <vector>

#include "isp_resample.h"

namespace rs {

// ---- the tables (host) --------------------------------------------------------------------------------------------------
// include/mi_isp.h states every double operation and its order; tests/resample_ref.py restates them in Python.

static const char* filter_name(int filter) {
  return filter == MI_RESAMPLE_AREA ? "area" : (filter == MI_RESAMPLE_TRIANGLE ? "triangle" : "lanczos3");
}

// the smallest scale a filter takes at any phase: T <= 32 (an interval of length widen meets widen + 1 samples, an open
// one of length 2 widen or 6 widen holds that many)
static double smallest_scale(int filter) {
  return filter == MI_RESAMPLE_AREA ? 1.0 / 31.0 : (filter == MI_RESAMPLE_TRIANGLE ? 1.0 / 16.0 : 3.0 / 16.0);
}

static double sinc(double x) {
  if (x == 0.0) return 1.0;
  if (x == std::nearbyint(x)) return 0.0;
  const double px = 3.14159265358979323846 * x;
  return std::sin(px) / px;
}

struct Tap { int k; double w; };

// the taps of output sample d in increasing k
static void taps_of(int filter, double s, int d, std::vector<Tap>& out) {
  out.clear();
  const double widen = s < 1.0 ? 1.0 / s : 1.0;
  const double c = (double)d / s;
  const double R = filter == MI_RESAMPLE_AREA ? widen / 2.0 + 0.5 : (filter == MI_RESAMPLE_TRIANGLE ? widen : 3.0 * widen);
  const long long k0 = (long long)std::floor(c - R), k1 = (long long)std::ceil(c + R);
  for (long long k = k0; k <= k1; ++k) {
    double w;
    bool tap;
    if (filter == MI_RESAMPLE_LANCZOS3) {
      const double x = ((double)k - c) / widen;
      w = std::fabs(x) < 3.0 ? sinc(x) * sinc(x / 3.0) : 0.0;
      tap = w != 0.0;
    } else if (filter == MI_RESAMPLE_AREA && s < 1.0) {
      const double hi = std::fmin((double)k + 0.5, c + widen / 2.0), lo = std::fmax((double)k - 0.5, c - widen / 2.0);
      w = hi - lo;
      tap = w > 0.0;
    } else {
      w = 1.0 - std::fabs((double)k - c) / widen;
      tap = w > 0.0;
    }
    if (tap) out.push_back({(int)k, w});
  }
}

static int check_axis(int filter, int S, int D, double scale, const char* who) {
  MI_REQUIRE(filter >= MI_RESAMPLE_AREA && filter <= MI_RESAMPLE_LANCZOS3, "%s: resample filter %d is none of area (1), "
             "triangle (2), lanczos3 (3)", who, filter);
  MI_REQUIRE(S > 0 && D > 0 && S <= 32768 && D <= 32768, "%s: resample axis of %d source and %d output samples outside "
             "1 .. 32768", who, S, D);
  MI_REQUIRE(std::isfinite(scale) && scale >= 1.0 / 4096.0 && scale <= 4096.0, "%s: resample scale %g outside "
             "[1 / 4096, 4096]", who, scale);
  return 0;
}

// T before the limit is applied
static int span_of(int filter, int S, int D, double scale) {
  std::vector<Tap> t;
  int span = 1;
  for (int d = 0; d < D; ++d) {
    taps_of(filter, scale, d, t);
    if (!t.empty() && t.back().k - t.front().k + 1 > span) span = t.back().k - t.front().k + 1;
  }
  return span < S ? span : S;
}

int taps(int filter, int S, int D, double scale, const char* who) {
  if (check_axis(filter, S, D, scale, who)) return -1;
  const int T = span_of(filter, S, D, scale);
  if (T > MAX_TAPS) {
    mi_set_error("%s: resample filter '%s' does not take scale %.9g on an axis of %d samples: %d taps, at most %d (its "
                 "smallest scale is %.6g)", who, filter_name(filter), scale, S, T, MAX_TAPS, smallest_scale(filter));
    return -1;
  }
  return T;
}

int table(int filter, int S, int D, double scale, int32_t* start, float* weight, const char* who) {
  const int T = taps(filter, S, D, scale, who);
  if (T < 0) return 1;
  MI_REQUIRE(start && weight, "%s: null resample table", who);
  std::vector<Tap> t;
  std::vector<double> row((size_t)T);
  for (int d = 0; d < D; ++d) {
    taps_of(filter, scale, d, t);
    MI_REQUIRE(!t.empty(), "%s: resample output sample %d has no tap", who, d);
    const int first = t.front().k;
    const int st = first < 0 ? 0 : (first > S - T ? S - T : first);
    for (int j = 0; j < T; ++j) row[j] = 0.0;
    for (const Tap& tap : t) {
      const int k = tap.k < 0 ? 0 : (tap.k > S - 1 ? S - 1 : tap.k);
      row[k - st] += tap.w;
    }
    double sum = row[0];
    for (int j = 1; j < T; ++j) sum = sum + row[j];
    start[d] = st;
    for (int j = 0; j < T; ++j) weight[(size_t)d * T + j] = (float)(row[j] / sum);
  }
  return 0;
}

// ---- the kernel ---------------------------------------------------------------------------------------------------------
// LDS of a block, in this order: ROWS segments of the source rows (raw bytes, 16-byte units), the ring of horizontally
// filtered f32 rows of THREADS values, the tile's horizontal weights (OW x Tx) and vertical weights (OH x Ty), its starts
// (OW + OH), per output row the ring slot of its first tap row, the source row that completes it and every row before it
// (`ready`: the prefix maximum of start + Ty) and the lowest row it or a later row reads (`lowest`: the suffix minimum of
// start), and five words of extents.
template <class TI> constexpr int seg_stride() { return SEG_PX * 3 * (int)sizeof(TI) + 16; }

// The ring holds every row between `lowest` and `ready` of the next output row while a step adds ROWS more: a tile whose
// window ready - lowest is at most ring_rows - ROWS + 1 runs through it.  The starts of a table of the contract rise with
// the output index, so its window is Ty, except for lanczos3 at scale >= 1 (Ty <= 7), whose rows that sit on a sample
// have one tap and start up to 3 later than their neighbours'.  Any other tile is evaluated tap by tap from memory.
__host__ __device__ static inline int ring_rows_of(int taps_y) {
  const int want = taps_y + ROWS - 1 + 4;
  return want < MAX_TAPS + ROWS ? want : MAX_TAPS + ROWS;
}

size_t lds_bytes(int taps_y, int taps_x, int in_size) {
  return (size_t)ROWS * (SEG_PX * 3 * in_size + 16) + (size_t)ring_rows_of(taps_y) * THREADS * 4 + (size_t)OW * taps_x * 4 +
         (size_t)OH * taps_y * 4 + (OW + 4 * OH + 5) * 4;
}

MI_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <class TI, class TO>
__global__ __launch_bounds__(THREADS) void resample_kernel(const Args a) {
  extern __shared__ uint4 lds_units[];
  constexpr int SEG = seg_stride<TI>();
  const int Tx = a.cols.taps, Ty = a.rows.taps;
  const int ring_rows = ring_rows_of(Ty);
  unsigned char* seg = reinterpret_cast<unsigned char*>(lds_units);
  float* ring = reinterpret_cast<float*>(seg + ROWS * SEG);
  float* wx = ring + ring_rows * THREADS;
  float* wy = wx + OW * Tx;
  int* sx = reinterpret_cast<int*>(wy + OH * Ty);
  int* sy = sx + OW;
  int* slot = sy + OH;
  int* ready = slot + OH;
  int* lowest = ready + OH;
  int* ext = lowest + OH;                    // min sx, max sx + Tx, min sy, max sy + Ty of the tile, its widest window

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * OW, y0 = blockIdx.y * OH;
  const int nx = a.Wd - x0 < OW ? a.Wd - x0 : OW, ny = a.Hd - y0 < OH ? a.Hd - y0 : OH;
  const TI* __restrict__ src = static_cast<const TI*>(a.im[blockIdx.z].src);
  TO* __restrict__ dst = static_cast<TO*>(a.im[blockIdx.z].dst);

  // the tile's tables; a start is clamped into [0, S - T], so no table makes a tap leave the image
  for (int i = tid; i < nx; i += THREADS) sx[i] = clampi(a.cols.start[x0 + i], 0, a.Ws - Tx);
  for (int i = tid; i < ny; i += THREADS) sy[i] = clampi(a.rows.start[y0 + i], 0, a.Hs - Ty);
  for (int i = tid; i < nx * Tx; i += THREADS) wx[i] = a.cols.weight[(size_t)x0 * Tx + i];
  for (int i = tid; i < ny * Ty; i += THREADS) wy[i] = a.rows.weight[(size_t)y0 * Ty + i];
  if (tid == 0) { ext[0] = a.Ws; ext[1] = 0; ext[2] = a.Hs; ext[3] = 0; }
  __syncthreads();
  for (int i = tid; i < nx; i += THREADS) { atomicMin(&ext[0], sx[i]); atomicMax(&ext[1], sx[i] + Tx); }
  for (int i = tid; i < ny; i += THREADS) { atomicMin(&ext[2], sy[i]); atomicMax(&ext[3], sy[i] + Ty); }
  if (tid == 0) {
    int hi = 0, lo = a.Hs, window = 0;
    for (int i = 0; i < ny; ++i) { hi = hi > sy[i] + Ty ? hi : sy[i] + Ty; ready[i] = hi; }
    for (int i = ny - 1; i >= 0; --i) {
      lo = lo < sy[i] ? lo : sy[i];
      lowest[i] = lo;
      window = window > ready[i] - lo ? window : ready[i] - lo;
    }
    ext[4] = window;
  }
  __syncthreads();
  const int seg0 = ext[0], seg1 = ext[1], row_lo = ext[2], row_hi = ext[3];
  for (int i = tid; i < ny; i += THREADS) slot[i] = (sy[i] - row_lo) % ring_rows;
  const bool staged = seg1 - seg0 <= SEG_PX;                     // (block-uniform)
  const size_t seg_bytes = (size_t)(seg1 - seg0) * 3 * sizeof(TI);

  const int px = tid / 3, ch = tid - px * 3;
  const bool active = tid < nx * 3;
  const int my_sx = active ? sx[px] : seg0;
  if (ext[4] > ring_rows - ROWS + 1) {                           // (block-uniform) a window the ring does not hold:
    if (active) {                                                // every output from memory, in the same order
      const float* w = wx + px * Tx;
      for (int r = 0; r < ny; ++r) {
        const float* v = wy + r * Ty;
        float acc = 0.f;
        for (int j = 0; j < Ty; ++j) {
          const TI* s = src + ((size_t)(sy[r] + j) * a.Ws + my_sx) * 3 + ch;
          float h = w[0] * (float)s[0];
          for (int k = 1; k < Tx; ++k) h = h + w[k] * (float)s[3 * k];
          acc = j == 0 ? v[0] * h : acc + v[j] * h;
        }
        dst[((size_t)(y0 + r) * a.Wd + x0) * 3 + tid] = cast_out<TO>(acc);
      }
    }
    return;
  }
  int top_slot = 0, r_next = 0;
  for (int top = row_lo; top < row_hi; top += ROWS) {
    const int nr = row_hi - top < ROWS ? row_hi - top : ROWS;
    if (staged) {
      // the rows' segments [seg0, seg1) into LDS as the 16-byte units of memory that hold them; a unit that is not whole
      // inside the segment (so possibly not inside the image) is copied element by element
      for (int rr = 0; rr < nr; ++rr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(src + ((size_t)(top + rr) * a.Ws + seg0) * 3);
        const uintptr_t hi = lo + seg_bytes;
        const uintptr_t u0 = lo & ~(uintptr_t)15;
        const int n_units = (int)((hi - u0 + 15) >> 4);
        unsigned char* row = seg + rr * SEG;
        for (int u = tid; u < n_units; u += THREADS) {
          const uintptr_t g = u0 + (uintptr_t)u * 16;
          if (g >= lo && g + 16 <= hi) {
            reinterpret_cast<uint4*>(row)[u] = *reinterpret_cast<const uint4*>(g);
          } else {
#pragma unroll
            for (int j = 0; j < 16 / (int)sizeof(TI); ++j) {
              const uintptr_t e = g + j * sizeof(TI);
              if (e >= lo && e < hi) reinterpret_cast<TI*>(row + u * 16)[j] = *reinterpret_cast<const TI*>(e);
            }
          }
        }
      }
      __syncthreads();
    }
    // horizontal: the rows' Tx taps in order, one rounded multiply and one rounded add each, into the ring.  The step's
    // rows go through the tap loop together, so a weight is read once for all of them (a row past the last is the last
    // again, computed and dropped)
    if (active) {
      const float* w = wx + px * Tx;
      const TI* s[ROWS];
      float acc[ROWS];
#pragma unroll
      for (int rr = 0; rr < ROWS; ++rr) {
        const int row = rr < nr ? rr : nr - 1;
        if (staged) {
          const uintptr_t lo = reinterpret_cast<uintptr_t>(src + ((size_t)(top + row) * a.Ws + seg0) * 3);
          s[rr] = reinterpret_cast<const TI*>(seg + row * SEG + (lo & 15)) + (my_sx - seg0) * 3 + ch;
        } else {
          s[rr] = src + ((size_t)(top + row) * a.Ws + my_sx) * 3 + ch;
        }
        acc[rr] = w[0] * (float)s[rr][0];
      }
      for (int k = 1; k < Tx; ++k) {
        const float wk = w[k];
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) acc[rr] = acc[rr] + wk * (float)s[rr][3 * k];
      }
      int sl = top_slot;
#pragma unroll
      for (int rr = 0; rr < ROWS; ++rr) {
        if (rr < nr) ring[sl * THREADS + tid] = acc[rr];
        if (++sl == ring_rows) sl = 0;
      }
    }
    top_slot += nr;
    if (top_slot >= ring_rows) top_slot -= ring_rows;
    __syncthreads();
    // vertical: every output row whose last tap row is in
    int r_end = r_next;
    while (r_end < ny && ready[r_end] <= top + nr) ++r_end;
    if (active) {
      for (int r = r_next; r < r_end; ++r) {
        const float* w = wy + r * Ty;
        int sl = slot[r];
        float acc = w[0] * ring[sl * THREADS + tid];
        for (int j = 1; j < Ty; ++j) {
          if (++sl == ring_rows) sl = 0;
          acc = acc + w[j] * ring[sl * THREADS + tid];
        }
        dst[((size_t)(y0 + r) * a.Wd + x0) * 3 + tid] = cast_out<TO>(acc);
      }
    }
    r_next = r_end;
    __syncthreads();
  }
}

template <class TI, class TO> static int launch_t(const Args& a, hipStream_t stream) {
  const dim3 grid((a.Wd + OW - 1) / OW, (a.Hd + OH - 1) / OH, a.n_images);
  const size_t lds = lds_bytes(a.rows.taps, a.cols.taps, (int)sizeof(TI));
  hipLaunchKernelGGL((resample_kernel<TI, TO>), grid, dim3(THREADS), lds, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, int in_dtype, int out_dtype, hipStream_t stream) {
  if (in_dtype == MI_F16) return out_dtype == MI_F16 ? launch_t<half_t, half_t>(a, stream) : launch_t<half_t, float>(a, stream);
  return out_dtype == MI_F16 ? launch_t<float, half_t>(a, stream) : launch_t<float, float>(a, stream);
}

}  // namespace rs
