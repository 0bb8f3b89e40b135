// Automatic white balance kernels (isp_awb.h; the contract is DESIGN.md 3, "Auto white balance").
//
// Statistics: lane by lane over the sampled 2x2 quads of a frame (quad (a, b) covers raw rows 2a, 2a+1 and columns 2b, 2b+1;
// only a % stride == 0 and b % stride == 0 are sampled).  Each raw value x is the loader's pre-cast value (tile::level_x
// for packed sources, load_shading_kernel's quotient for CFA tensors); a quad is kept when all four x < clip and
// max(x) >= floor, and then adds q = u64(rint(min(max(x * g_user, 0), 2^15) * 2^24)) to its site's sum.  The lanes keep
// their sums in u64 registers, reduce them across the wave with shuffles and across the block's waves through LDS, and
// lanes 0..4 of the block's first wave add the block's five values to the pending buffer with 64-bit integer atomics: one
// contiguous 40-byte atomic instruction per block, an exact, order-independent total.
//
// Update: one workgroup.  Lane 0 sums the gathered rows, moves the gray-world state and the gains in f64 (no contraction)
// and zeroes the pending buffer; then every lane writes its share of E = U * g (at most 4 x 64 x 64 floats).
#include "isp_awb.h"
#include "isp_tile.h"

#pragma clang fp contract(off)

namespace awb {

// the sums of one lane -> the block's, added to the pending buffer (every lane of the block calls it)
MI_DEV void flush(unsigned long long (&v)[PENDING], unsigned long long* pending) {
  __shared__ unsigned long long red[THREADS / 64][PENDING];
#pragma unroll
  for (int k = 0; k < PENDING; ++k)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < PENDING; ++k) red[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x < PENDING) {
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) s += red[w][threadIdx.x];
    if (s) atomicAdd(pending + threadIdx.x, s);
  }
}

// one quad's four x (sites 0..3 = (r0, c0), (r0, c1), (r1, c0), (r1, c1)) into the lane's sums
MI_DEV void add_quad(const Stats& s, int r, int c, const float (&x)[4], unsigned long long (&v)[PENDING]) {
  const bool below = x[0] < s.clip && x[1] < s.clip && x[2] < s.clip && x[3] < s.clip;
  const bool lit = x[0] >= s.floor || x[1] >= s.floor || x[2] >= s.floor || x[3] >= s.floor;
  if (!(below && lit)) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float xs = s.shading ? x[k] * shade_gain(s, r + (k >> 1), c + (k & 1)) : x[k];
    const float q = __builtin_rintf(fminf(fmaxf(xs, 0.f), 32768.f) * 16777216.f);
    v[k] += (unsigned long long)q;
  }
  v[4] += 1;
}

__global__ __launch_bounds__(THREADS) void stats_packed_kernel(const PackedArgs a) {
  const Stats& s = a.s;
  const uint8_t* __restrict__ src = a.src[blockIdx.y];
  const int QA = (s.H / 2 + s.stride - 1) / s.stride, QB = (s.W / 2 + s.stride - 1) / s.stride;
  const long long nq = (long long)QA * QB;
  const size_t row_bytes = a.bits == 12 ? (size_t)s.W / 2 * 3 : (size_t)s.W * 2;
  const bool ids = a.ids != 0;
  unsigned long long v[PENDING] = {0, 0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < nq; i += (long long)gridDim.x * THREADS) {
    const int r = (int)(i / QB) * s.stride * 2, c = (int)(i % QB) * s.stride * 2;
    uint32_t code[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint8_t* p = src + (size_t)(r + h) * row_bytes + (a.bits == 12 ? (size_t)c / 2 * 3 : (size_t)c * 2);
      if (a.bits == 12) {
        tile::unpack_pair((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16), ids, code[2 * h],
                          code[2 * h + 1]);
      } else {
        code[2 * h] = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
        code[2 * h + 1] = (uint32_t)p[2] | ((uint32_t)p[3] << 8);
      }
    }
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = tile::level_x(code[k], s.black[k], s.k[k]);
    add_quad(s, r, c, x, v);
  }
  flush(v, s.pending);
}

__global__ __launch_bounds__(THREADS) void stats_cfa_kernel(const Stats s, const void* __restrict__ cfa, int mode) {
  const int QA = (s.H / 2 + s.stride - 1) / s.stride, QB = (s.W / 2 + s.stride - 1) / s.stride;
  const long long nq = (long long)QA * QB;
  unsigned long long v[PENDING] = {0, 0, 0, 0, 0};
  for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < nq; i += (long long)gridDim.x * THREADS) {
    const int r = (int)(i / QB) * s.stride * 2, c = (int)(i % QB) * s.stride * 2;
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t at = (size_t)(r + (k >> 1)) * s.W + c + (k & 1);
      if (mode == MI_LOAD_16U) {
        const uint16_t u = static_cast<const uint16_t*>(cfa)[at];
        if (s.has_levels) {                          // load_shading_kernel's quotient (k[] holds the denominators)
          const int d = (int)u - s.black[k];
          x[k] = (float)(d > 0 ? d : 0) / s.k[k];
        } else {
          x[k] = (float)u / 65535.0f;
        }
      } else if (mode == MI_LOAD_32F) {
        x[k] = static_cast<const float*>(cfa)[at];
      } else {
        x[k] = (float)static_cast<const uint16_t*>(cfa)[at];
      }
    }
    add_quad(s, r, c, x, v);
  }
  flush(v, s.pending);
}

__global__ __launch_bounds__(THREADS) void update_kernel(const Update u) {
  __shared__ float g[3];
  if (threadIdx.x == 0) {
    float gr = u.gains[0], gg = u.gains[1], gb = u.gains[2];
    if (u.gathered) {
      unsigned long long P[PENDING] = {0, 0, 0, 0, 0};
      for (int w = 0; w < u.world; ++w)
        for (int k = 0; k < PENDING; ++k) P[k] += (unsigned long long)u.gathered[w * PENDING + k];
      for (int k = 0; k < PENDING; ++k) u.pending[k] = 0;     // (after every read: gathered may be pending itself)
      if (P[4] != 0) {
        const double n = (double)P[4];
        double m[4], c[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < 4; ++k) m[k] = ((double)P[k] * 0x1p-24) / n;
        for (int k = 0; k < 4; ++k) {
          if (u.site_colour[k] == 1) c[1] += m[k];
          else c[u.site_colour[k]] = m[k];
        }
        c[1] = c[1] * 0.5;
        const double t = u.state[3] != 0.0 ? u.t : 0.0;
        double S[3];
        for (int k = 0; k < 3; ++k) {
          S[k] = c[k] + t * (u.state[k] - c[k]);
          u.state[k] = S[k];
        }
        u.state[3] = 1.0;
        if (S[1] > 0.0 && S[0] > 0.0) gr = (float)fmin(fmax(S[1] / S[0], 0.125), 8.0);
        if (S[1] > 0.0 && S[2] > 0.0) gb = (float)fmin(fmax(S[1] / S[2], 0.125), 8.0);
        gg = 1.f;
        u.gains[0] = gr; u.gains[1] = gg; u.gains[2] = gb;
      }
    }
    g[0] = gr; g[1] = gg; g[2] = gb;
  }
  __syncthreads();
  const int cell = u.gh * u.gw;
  for (int i = threadIdx.x; i < 4 * cell; i += THREADS) {
    const int s = i / cell, j = i - s * cell;
    const int col = u.site_colour[s];
    const float gc = col == 0 ? g[0] : (col == 1 ? g[1] : g[2]);
    u.effective[i] = u.user ? u.user[(u.user_sites == 4 ? s : 0) * cell + j] * gc : gc;
  }
}

static int blocks_for(long long nq) {
  const long long b = (nq + THREADS - 1) / THREADS;
  return (int)(b < MAX_BLOCKS ? (b < 1 ? 1 : b) : MAX_BLOCKS);
}

int launch_packed(const PackedArgs& a, hipStream_t stream) {
  const long long nq = (long long)((a.s.H / 2 + a.s.stride - 1) / a.s.stride) * ((a.s.W / 2 + a.s.stride - 1) / a.s.stride);
  if (nq == 0 || a.n_frames == 0) return 0;
  hipLaunchKernelGGL(stats_packed_kernel, dim3(blocks_for(nq), a.n_frames), dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch_cfa(const Stats& s, const void* cfa, int mode, hipStream_t stream) {
  const long long nq = (long long)((s.H / 2 + s.stride - 1) / s.stride) * ((s.W / 2 + s.stride - 1) / s.stride);
  if (nq == 0) return 0;
  hipLaunchKernelGGL(stats_cfa_kernel, dim3(blocks_for(nq)), dim3(THREADS), 0, stream, s, cfa, mode);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch_update(const Update& u, hipStream_t stream) {
  hipLaunchKernelGGL(update_kernel, dim3(1), dim3(THREADS), 0, stream, u);
  MI_LAUNCH_CHECK();
  return 0;
}

}  // namespace awb
