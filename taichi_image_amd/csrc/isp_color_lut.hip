// 3D colour LUT kernels (isp_color_lut.h; the contract is DESIGN.md 3, "Colour LUT").
//
// The images of a launch are cut into chunks of THREADS * 4 consecutive pixels (an image is contiguous, so a chunk is a run
// of bytes; the last chunk of an image is short), numbered image by image.  Block b takes chunks b, b + gridDim.x, ...: a
// thread owns 4 pixels of each.
//  - The LDS instances (CAP > 0 dwords; N^3 <= CAP is the launcher's to guarantee): the block first copies the whole table
//    from global memory into LDS, once, and every pixel is then four ds_read_b32.  1024 threads; the grid is at most one
//    block per CU at CAP = 33^3 (143 748 bytes of the CU's 160 KiB) and two per CU at CAP = 17^3, so a block takes many
//    chunks and the table is read out of L2 gridDim.x times per launch, not once per chunk.
//  - The global instance (CAP = 0): the same arithmetic, the four gathers go through L2.  256 threads, one chunk per block.
//  - Pixel I / O: where the rows allow (W * 3 % 4 == 0 and 4-byte aligned images) a thread reads its 4 pixels as 3 dwords
//    (bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3) and writes them so; everything else goes byte by byte.  A thread reads
//    its pixels before it writes them and no other thread touches them: src == dst is fine.
//  - Addresses: i_c <= N - 1 always (v_c <= 255), and the step to the next point of an axis is 0 at i_c = N - 1 (the
//    contract's min(i_c + 1, N - 1)), so every index is below N^3 whatever the weights are.
#include "isp_color_lut.h"

namespace clut {

using u8::byte_of;

// one compare-exchange of the sort by descending fraction: the index step travels with its fraction
MI_DEV void order(uint32_t& fa, uint32_t& sa, uint32_t& fb, uint32_t& sb) {
  const bool swap = fa < fb;
  const uint32_t f = swap ? fb : fa, s = swap ? sb : sa;
  fb = swap ? fa : fb; sb = swap ? sa : sb;
  fa = f; sa = s;
}

struct Taps {
  uint32_t idx[4];                                  // the four corners of the pixel's tetrahedron
  uint32_t w[4];                                    // their weights, 255 in all
};

MI_DEV Taps taps(int vr, int vg, int vb, int N) {
  const uint32_t n1 = (uint32_t)(N - 1);
  const uint32_t pr = mul24(vr, n1), pg = mul24(vg, n1), pb = mul24(vb, n1);
  const uint32_t ir = div255(pr), ig = div255(pg), ib = div255(pb);
  uint32_t f0 = pr - mul24(255u, ir), f1 = pg - mul24(255u, ig), f2 = pb - mul24(255u, ib);
  // the steps to j_c = min(i_c + 1, N - 1): none at the last point
  uint32_t s0 = ir < n1 ? mul24(N, N) : 0u, s1 = ig < n1 ? (uint32_t)N : 0u, s2 = ib < n1 ? 1u : 0u;
  order(f0, s0, f1, s1);
  order(f1, s1, f2, s2);
  order(f0, s0, f1, s1);                            // f0 >= f1 >= f2
  Taps t;
  t.idx[0] = mul24(mul24(ir, N) + ig, N) + ib;
  t.idx[1] = t.idx[0] + s0;
  t.idx[2] = t.idx[1] + s1;
  t.idx[3] = t.idx[2] + s2;
  t.w[0] = 255u - f0; t.w[1] = f0 - f1; t.w[2] = f1 - f2; t.w[3] = f2;
  return t;
}

// a * b + c for a, b < 2^24 (stated as the instruction: the compiler turns a 24-bit multiply whose operand it knows to be a
// byte back into a 32-bit one, which runs at a quarter of the rate)
MI_DEV uint32_t mad24(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// out_c of channel value v and the interpolated y
MI_DEV int blend(int v, uint32_t y, int S) { return v + ((__mul24((int)y - v, S) + 32) >> 6); }

// the pixel's output R | G << 8 | B << 16 from its four table entries: R and B share one multiply (each sum stays below
// 2^16: the weights add up to 255)
MI_DEV uint32_t shade(int vr, int vg, int vb, const uint32_t c[4], const uint32_t w[4], int S) {
  uint32_t rb = 0x007f007fu, g = 127u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    rb = mad24(c[k] & 0x00ff00ffu, w[k], rb);         // (below 2^24 times below 2^8)
    g = mad24((c[k] >> 8) & 0xffu, w[k], g);
  }
  const int r = blend(vr, div255(rb & 0xffffu), S), gg = blend(vg, div255(g), S), b = blend(vb, div255(rb >> 16), S);
  return (uint32_t)r | ((uint32_t)gg << 8) | ((uint32_t)b << 16);
}

// grid: min(chunks of the launch, what the launcher allows); CAP: the table's LDS dwords, 0: it stays in global memory
template <int CAP, int THREADS>
__global__ void __launch_bounds__(THREADS) color_lut_kernel(const Args a) {
  constexpr uint32_t CHUNK = THREADS * PIXELS_PER_THREAD;
  __shared__ uint32_t lut[CAP > 0 ? CAP : 1];
  const int N = a.n_points, S = a.strength_q6;
  if constexpr (CAP > 0) {
    const int n3 = N * N * N;                         // <= CAP
#pragma unroll 8
    for (int i = threadIdx.x; i < n3; i += THREADS) lut[i] = a.table[i];
    __syncthreads();
  }
  auto entry = [&](uint32_t i) __attribute__((always_inline)) {
    if constexpr (CAP > 0) return lut[i];
    else return a.table[i];
  };
  const uint32_t P = a.pixels;
  const uint32_t per_image = (P + CHUNK - 1) / CHUNK, total = per_image * (uint32_t)a.n_images;

  for (uint32_t chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const uint32_t k = chunk / per_image;             // (block-uniform: scalar loads of the image's pointers)
    const u8::Image im = a.im[k];
    const uint32_t p0 = (chunk - k * per_image) * CHUNK + threadIdx.x * PIXELS_PER_THREAD;
    if (p0 >= P) continue;                            // (no barrier inside the loop)
    const bool fast = a.dword_rows && ((reinterpret_cast<uintptr_t>(im.src) | reinterpret_cast<uintptr_t>(im.dst)) & 3) == 0;
    if (fast) {                                       // P % 4 == 0: the thread's 4 pixels are all inside
      const uint32_t* sp = reinterpret_cast<const uint32_t*>(im.src + (size_t)p0 * 3);
      const uint32_t d0 = sp[0], d1 = sp[1], d2 = sp[2];
      const int v[4][3] = {{byte_of(d0, 0), byte_of(d0, 1), byte_of(d0, 2)},
                           {byte_of(d0, 3), byte_of(d1, 0), byte_of(d1, 1)},
                           {byte_of(d1, 2), byte_of(d1, 3), byte_of(d2, 0)},
                           {byte_of(d2, 1), byte_of(d2, 2), byte_of(d2, 3)}};
      Taps t[4];
      uint32_t c[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = taps(v[q][0], v[q][1], v[q][2], N);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[q][j] = entry(t[q].idx[j]);
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = shade(v[q][0], v[q][1], v[q][2], c[q], t[q].w, S);
      uint32_t* dp = reinterpret_cast<uint32_t*>(im.dst + (size_t)p0 * 3);
      dp[0] = o[0] | (o[1] << 24);
      dp[1] = (o[1] >> 8) | (o[2] << 16);
      dp[2] = (o[2] >> 16) | (o[3] << 8);
    } else {
#pragma unroll
      for (int q = 0; q < PIXELS_PER_THREAD; ++q) {
        if (p0 + q >= P) break;
        const size_t off = (size_t)(p0 + q) * 3;
        const int vr = im.src[off], vg = im.src[off + 1], vb = im.src[off + 2];
        const Taps t = taps(vr, vg, vb, N);
        uint32_t c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = entry(t.idx[j]);
        const uint32_t o = shade(vr, vg, vb, c, t.w, S);
        im.dst[off] = (uint8_t)o;
        im.dst[off + 1] = (uint8_t)(o >> 8);
        im.dst[off + 2] = (uint8_t)(o >> 16);
      }
    }
  }
}

template <int CAP, int THREADS>
static int launch_inst(const Args& a, uint32_t max_blocks, hipStream_t stream) {
  constexpr uint32_t CHUNK = THREADS * PIXELS_PER_THREAD;
  const uint32_t chunks = (a.pixels + CHUNK - 1) / CHUNK * (uint32_t)a.n_images;
  const uint32_t grid = max_blocks && chunks > max_blocks ? max_blocks : chunks;
  hipLaunchKernelGGL((color_lut_kernel<CAP, THREADS>), dim3(grid), dim3(THREADS), 0, stream, a);
  MI_LAUNCH_CHECK();
  return 0;
}

int launch(const Args& a, Path path, int n_cus, hipStream_t stream) {
  if (a.n_images <= 0 || a.pixels == 0) return 0;
  constexpr int N17 = LDS_POINTS_SMALL, N33 = LDS_POINTS;
  if (n_cus <= 0) n_cus = 256;
  const bool lds = path == PATH_LDS || (path == PATH_AUTO && lds_wins(a.n_points));
  if (lds && a.n_points <= N17) return launch_inst<N17 * N17 * N17, LDS_THREADS>(a, 2u * (uint32_t)n_cus, stream);
  if (lds && a.n_points <= N33) return launch_inst<N33 * N33 * N33, LDS_THREADS>(a, (uint32_t)n_cus, stream);
  return launch_inst<0, GLOBAL_THREADS>(a, 0, stream);
}

}  // namespace clut
