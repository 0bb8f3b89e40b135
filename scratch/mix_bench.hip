// Mixed-stream issue benchmark: the instruction mix of the whole-frame kernel's phases A and C (per row of a wave, class
// counts = profiles/r03_whole_frame_census.txt / 12), once with scalar v_fmac/v_mul/v_add and once with the packable share
// as v_pk_fma/mul/add_f32.  Two waves per SIMD from two different blocks (64 KB of LDS per block: two blocks per CU),
// independent chains, the s_setprio turns of mega::prio_turn.  class_bench.hip measures pure streams; this one asks
// whether a wave that issues FEWER instructions for the same arithmetic gets through the mix sooner.
// The loops as compiled hold 420 / 340 (A) and 272 / 227 (C) instructions per row: the class counts below plus loop control
// and one s_nop 0 per ~7 instructions that the compiler puts between asm statements - the same number in both variants.
//   hipcc -O3 --offload-arch=gfx950 scratch/mix_bench.hip -o mix_bench && ./mix_bench
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <algorithm>
typedef float f2 __attribute__((ext_vector_type(2)));

struct Regs {
  float a[24];        // scalar accumulators / pixel values
  f2 pa[12];          // the same as pairs {K, K + 4}
  float x[16];        // window values, weights, uniform operands
  f2 px[8];
  f2 pw[4];           // weights, two per pair (broadcast with op_sel)
  uint32_t m[8];      // integer / packed-f16 side
  float s[6];         // statistics
  uint32_t addr;      // LDS address of the lane
  uint32_t sc;        // an SGPR counter
};

#define V1(op, d, s0) asm volatile(op " %0, %1" : "+v"(d) : "v"(s0))
#define V2(op, d, s0, s1) asm volatile(op " %0, %1, %2" : "+v"(d) : "v"(s0), "v"(s1))
#define V3(op, d, s0, s1, s2) asm volatile(op " %0, %1, %2, %3" : "+v"(d) : "v"(s0), "v"(s1), "v"(s2))
#define SALU(R) asm volatile("s_add_u32 %0, %0, 1" : "+s"(R.sc) : : "scc")   /* (it writes SCC: the loop's compare lives there) */
#define NOP() asm volatile("s_nop 0")

// ---- phase A, one row: decode, 24 accumulation chains of 1 mul + 6 fmac, f16 pack, bounds, gray, statistics ----
// scalar: 25 int + 11 lds + 4 waitcnt + 20 mov + 24 mul + 144 fmac + 12 cvt_pk + 12 pk_min3/max3_f16 + 24 fma_mix + 8 max
//         + 4 min3 + 4 max3 + 9 add + 7 mul + 1 log + 14 cvt + 2 s_nop + 20 salu = 345 (census: 4165 / 12 = 347)
// packed: 24 mul + 144 fmac -> 12 pk_mul + 72 pk_fma, + 4 mov (the window row's duplicated columns) = 265
template <bool PK> __device__ __forceinline__ void row_a(Regs& R, const float* lds) {
#pragma unroll
  for (int i = 0; i < 25; ++i) {
    if (i & 1) asm volatile("v_and_b32_e32 %0, 0xfff, %1" : "+v"(R.m[i & 7]) : "v"(R.m[(i + 3) & 7]));
    else asm volatile("v_lshrrev_b32_e32 %0, 12, %1" : "+v"(R.m[i & 7]) : "v"(R.m[(i + 3) & 7]));
  }
  float t[11];
#pragma unroll
  for (int i = 0; i < 11; ++i) {
    asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(t[i]) : "v"(R.addr), "n"(i * 256));
    if (i % 3 == 2) SALU(R);
  }
#pragma unroll
  for (int i = 0; i < 11; ++i) {
    if (i % 3 == 0) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(10 - i > 8 ? 8 : 10 - i));
    V1("v_mov_b32_e32", R.x[i], t[i]);
  }
#pragma unroll
  for (int i = 0; i < 9 + (PK ? 4 : 0); ++i) V1("v_mov_b32_e32", R.x[(i + 11) & 15], R.x[i & 7]);
  NOP();
  if constexpr (!PK) {
#pragma unroll
    for (int t6 = 0; t6 < 7; ++t6)
#pragma unroll
      for (int i = 0; i < 24; ++i) {
        if (t6 == 0) asm volatile("v_mul_f32_e32 %0, %1, %2" : "=v"(R.a[i]) : "v"(R.x[(i + t6) & 15]), "v"(R.x[(i + 5) & 15]));
        else asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(R.a[i]) : "v"(R.x[(i + t6) & 15]), "v"(R.x[(i + 5) & 15]));
        if (i == 23) SALU(R);
      }
  } else {
#pragma unroll
    for (int t6 = 0; t6 < 7; ++t6)
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        // weight = the low or the high half of a weight pair, for both results
        if (t6 == 0) {
          if (i & 1) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(R.pa[i]) : "v"(R.px[(i + t6) & 7]), "v"(R.pw[i & 3]));
          else asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(R.pa[i]) : "v"(R.px[(i + t6) & 7]), "v"(R.pw[i & 3]));
        } else {
          if (i & 1) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(R.pa[i]) : "v"(R.px[(i + t6) & 7]), "v"(R.pw[(i + t6) & 3]));
          else asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(R.pa[i]) : "v"(R.px[(i + t6) & 7]), "v"(R.pw[(i + t6) & 3]));
        }
        if (i == 11) SALU(R);
      }
  }
  // the 24 values of the row: a[] or the halves of pa[] (sub-registers: no copy)
  float* v = R.a;
#define VAL(j) (PK ? ((j) % 8 < 4 ? R.pa[(j) / 8 * 4 + (j) % 4].x : R.pa[(j) / 8 * 4 + (j) % 4].y) : v[j])
  uint32_t pk[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) asm volatile("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(pk[j]) : "v"(VAL(2 * j)), "v"(VAL(2 * j + 1)));
#undef VAL
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    asm volatile("v_pk_minimum3_f16 %0, %0, %1, %2" : "+v"(R.m[0]) : "v"(pk[2 * j]), "v"(pk[2 * j + 1]));
    asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(R.m[1]) : "v"(pk[2 * j]), "v"(pk[2 * j + 1]));
  }
  float g[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    asm volatile("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(g[k]) : "v"(pk[k]), "v"(R.x[0]));
    asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(g[k]) : "v"(pk[k]), "v"(R.x[1]));
    asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,0,0]" : "+v"(g[k]) : "v"(pk[k + 4]), "v"(R.x[2]));
    if (k & 1) SALU(R);
  }
  float c[8];
#pragma unroll
  for (int k = 0; k < 8; k += 2) {
    asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(R.s[0]) : "v"(g[k]), "v"(g[k + 1]));
    asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(R.s[1]) : "v"(g[k]), "v"(g[k + 1]));
    asm volatile("v_max_f32 %0, 0x38d1b717, %1" : "=v"(c[k]) : "v"(g[k]));
    asm volatile("v_max_f32 %0, 0x38d1b717, %1" : "=v"(c[k + 1]) : "v"(g[k + 1]));
    V2("v_add_f32_e32", R.s[2], R.s[2], g[k]);
    V2("v_add_f32_e32", R.s[2], R.s[2], g[k + 1]);
    SALU(R);
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) V2("v_mul_f32_e32", c[(k + 1) & 7], c[(k + 1) & 7], c[k]);
  NOP();
  V1("v_log_f32_e32", c[0], c[7]);
  V2("v_add_f32_e32", R.s[3], R.s[3], c[0]);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    asm volatile("v_cvt_f32_f16_e32 %0, %1" : "=v"(c[k]) : "v"(pk[k]));
    asm volatile("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(g[k]) : "v"(pk[k]));
    SALU(R);
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) asm volatile("" ::"v"(c[k]), "v"(g[k]));
}

// ---- phase C, one row of eight pixels: gray, adaptation, pow, three maps per pixel, bounds ----
// scalar per pixel: mul fma fma | sub fma mul | log mul exp | 3 add | 3 rcp | 3 mul | min3 max3 x 1.5; per row besides:
//   7 fma_mix + 10 cvt + 15 mov + 12 s_nop + 15 salu + 2 lds = 45 mul + 29 add/sub + 17 fma + 37 trans + 24 min/max + ... = 215
//   (census: 2588 / 12 = 216)
// packed: pixels k and k + 4 as a pair through everything but the transcendentals and min / max:
//   45 mul -> 22 pk + 1, 29 add -> 14 pk + 1, 17 fma -> 8 pk + 1 = 170
template <bool PK> __device__ __forceinline__ void row_c(Regs& R, const float* lds) {
  float t[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(t[i]) : "v"(R.addr), "n"(i * 256));
#pragma unroll
  for (int i = 0; i < 15; ++i) { V1("v_mov_b32_e32", R.x[(i + 9) & 15], R.x[i & 7]); if (i % 3 == 0) SALU(R); }
  asm volatile("s_waitcnt lgkmcnt(0)");
  uint32_t h = R.m[2];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    asm volatile("v_cvt_f32_f16_e32 %0, %1" : "=v"(R.a[k]) : "v"(h));
    asm volatile("v_cvt_f32_f16_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(R.a[8 + k]) : "v"(h));
    SALU(R);
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) asm volatile("v_fma_mix_f32 %0, %1, %2, %0 op_sel_hi:[1,0,0]" : "+v"(R.a[16 + k]) : "v"(h), "v"(R.x[1]));
  // a[0..7] r, a[8..15] g, a[16..23] b of the eight pixels; pa[0..3] r, pa[4..7] g, pa[8..11] b of the four pairs
  if constexpr (!PK) {
    float gy[8], ad[8], q[24];
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("v_mul_f32_e32 %0, %1, %2" : "=v"(gy[k]) : "v"(R.a[8 + k]), "v"(R.x[0]));
#pragma unroll
    for (int k = 0; k < 8; ++k) V2("v_fmac_f32_e32", gy[k], R.a[k], R.x[1]);
#pragma unroll
    for (int k = 0; k < 8; ++k) V2("v_fmac_f32_e32", gy[k], R.a[16 + k], R.x[2]);
#pragma unroll
    for (int k = 0; k < 8; ++k) V2("v_sub_f32_e32", gy[k], gy[k], R.x[3]);
#pragma unroll
    for (int k = 0; k < 8; ++k) asm volatile("v_fma_f32 %0, %1, %0, %2" : "+v"(gy[k]) : "v"(R.x[4]), "v"(R.x[3]));
#pragma unroll
    for (int k = 0; k < 8; ++k) V2("v_mul_f32_e32", gy[k], R.x[5], gy[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) { V1("v_log_f32_e32", ad[k], gy[k]); if (k & 1) NOP(); }
#pragma unroll
    for (int k = 0; k < 8; ++k) V2("v_mul_f32_e32", ad[k], R.x[6], ad[k]);
#pragma unroll
    for (int k = 0; k < 8; ++k) { V1("v_exp_f32_e32", ad[k], ad[k]); if (k & 1) NOP(); }
#pragma unroll
    for (int j = 0; j < 21; ++j) asm volatile("v_add_f32_e32 %0, %1, %2" : "=v"(q[j]) : "v"(ad[j & 7]), "v"(R.a[j]));
#pragma unroll
    for (int j = 0; j < 21; ++j) { V1("v_rcp_f32_e32", q[j], q[j]); if (j % 5 == 4) NOP(); if (j % 4 == 3) SALU(R); }
#pragma unroll
    for (int j = 0; j < 21; ++j) V2("v_mul_f32_e32", q[j], R.a[j], q[j]);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(R.s[0]) : "v"(q[j]), "v"(q[(j + 9) % 21]));
      asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(R.s[1]) : "v"(q[j]), "v"(q[(j + 9) % 21]));
    }
  } else {
    // the halves of pa[] are what the conversions above wrote (a[] and pa[] are separate registers here: the packed
    // variant's sources are simply pa[], values do not matter to the issue rate)
    f2 gy[4], ad[4], q[11];
    const f2 u0 = R.px[0], u1 = R.px[1], u2 = R.px[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(gy[k]) : "v"(R.pa[4 + k]), "v"(u0));
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(gy[k]) : "v"(R.pa[k]), "v"(u0));
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(gy[k]) : "v"(R.pa[8 + k]), "v"(u1));
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_add_f32 %0, %0, %1 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "+v"(gy[k]) : "v"(u1));
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_fma_f32 %0, %1, %0, %1 op_sel:[0,0,1] op_sel_hi:[0,1,1]" : "+v"(gy[k]) : "v"(u2));
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_mul_f32 %0, %0, %1 op_sel_hi:[1,0]" : "+v"(gy[k]) : "v"(u2));
    asm volatile("v_fma_f32 %0, %1, %0, %2" : "+v"(R.a[0]) : "v"(R.x[4]), "v"(R.x[3]));   // the odd ones out
    V2("v_mul_f32_e32", R.a[1], R.x[5], R.a[1]);
    V2("v_add_f32_e32", R.a[2], R.x[5], R.a[2]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      asm volatile("v_log_f32_e32 %0, %1" : "=v"(ad[k].x) : "v"(gy[k].x));
      asm volatile("v_log_f32_e32 %0, %1" : "=v"(ad[k].y) : "v"(gy[k].y));
      NOP();
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) asm volatile("v_pk_mul_f32 %0, %0, %1 op_sel_hi:[1,0]" : "+v"(ad[k]) : "v"(u0));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      asm volatile("v_exp_f32_e32 %0, %1" : "=v"(gy[k].x) : "v"(ad[k].x));
      asm volatile("v_exp_f32_e32 %0, %1" : "=v"(gy[k].y) : "v"(ad[k].y));
      NOP();
    }
#pragma unroll
    for (int j = 0; j < 11; ++j) asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(q[j]) : "v"(gy[j & 3]), "v"(R.pa[j]));
    // the reciprocals go into the halves of the pair they came from (21 of the 22 halves)
#pragma unroll
    for (int j = 0; j < 21; ++j) {
      if (j & 1) asm volatile("v_rcp_f32_e32 %0, %0" : "+v"(q[j / 2].y));
      else asm volatile("v_rcp_f32_e32 %0, %0" : "+v"(q[j / 2].x));
      if (j % 5 == 4) NOP();
      if (j % 4 == 3) SALU(R);
    }
#pragma unroll
    for (int j = 0; j < 11; ++j) asm volatile("v_pk_mul_f32 %0, %1, %0" : "+v"(q[j]) : "v"(R.pa[j]));
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(R.s[0]) : "v"(q[j].x), "v"(q[(j + 5) % 11].y));
      asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(R.s[1]) : "v"(q[j].x), "v"(q[(j + 5) % 11].y));
      asm volatile("v_min3_f32 %0, %0, %1, %2" : "+v"(R.s[0]) : "v"(q[j].y), "v"(q[(j + 3) % 11].x));
      asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(R.s[1]) : "v"(q[j].y), "v"(q[(j + 3) % 11].x));
    }
  }
}

template <int PHASE, bool PK>
__global__ __launch_bounds__(256, 2) void k(float* out, int rows, int n_blocks) {
  __shared__ float lds[16000];                        // 64 000 B: two blocks per CU, one wave of each on every SIMD
  for (int e = threadIdx.x; e < 16000; e += 256) lds[e] = 1.0f + 1e-6f * e;
  __syncthreads();
  Regs R;
#pragma unroll
  for (int i = 0; i < 24; ++i) R.a[i] = 1.0f + 0.001f * threadIdx.x + i;
#pragma unroll
  for (int i = 0; i < 12; ++i) R.pa[i] = f2{R.a[i], R.a[i + 12]};
#pragma unroll
  for (int i = 0; i < 16; ++i) R.x[i] = 0.5f + 1e-3f * (threadIdx.x + i);
#pragma unroll
  for (int i = 0; i < 8; ++i) R.px[i] = f2{R.x[i], R.x[i + 8]};
#pragma unroll
  for (int i = 0; i < 4; ++i) R.pw[i] = f2{0.25f + i, 0.125f * i};
#pragma unroll
  for (int i = 0; i < 8; ++i) R.m[i] = 0x3c003800u + threadIdx.x * 7u + i;
#pragma unroll
  for (int i = 0; i < 6; ++i) R.s[i] = 0.f;
  R.addr = (threadIdx.x & 63) * 4 + (threadIdx.x >> 6) * 12288;
  R.sc = 0;
  const bool younger = (int)blockIdx.x >= (n_blocks >> 1);
  for (int r = 0; r < rows; ++r) {
    if (((r & 1) != 0) == younger) asm volatile("s_setprio 1");
    else asm volatile("s_setprio 0");
    if constexpr (PHASE == 0) row_a<PK>(R, lds);
    else row_c<PK>(R, lds);
  }
  float s = (float)R.sc;
#pragma unroll
  for (int i = 0; i < 24; ++i) s += R.a[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) s += R.pa[i].x + R.pa[i].y;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += R.x[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) s += (float)R.m[i];
#pragma unroll
  for (int i = 0; i < 6; ++i) s += R.s[i];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int PHASE, bool PK> float run(float* out, int n_blocks, int rows) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0);
  hipLaunchKernelGGL((k<PHASE, PK>), dim3(n_blocks), dim3(256), 0, 0, out, rows, n_blocks);
  (void)hipEventRecord(e1);
  (void)hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return ms;
}

int main() {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { printf("no device\n"); return 1; }
  const int n_blocks = 2 * prop.multiProcessorCount, rows = 12 * 400;
  float* out;
  if (hipMalloc(&out, (size_t)n_blocks * 256 * 4) != hipSuccess) return 1;
  const int n_scalar[2] = {420, 272}, n_packed[2] = {340, 227};   // the loops as compiled (see the head of the file)
  printf("# scratch/mix_bench.hip on %s: %d blocks x 4 waves (2 waves per SIMD), %d rows per wave; us per 12 rows (one wave's phase)\n",
         prop.gcnArchName, n_blocks, rows);
  for (int ph = 0; ph < 2; ++ph) {
    float ts[6], tp[6];
    for (int rep = 0; rep < 6; ++rep) {                // alternating; rep 0 is the warm-up
      ts[rep] = ph == 0 ? run<0, false>(out, n_blocks, rows) : run<1, false>(out, n_blocks, rows);
      tp[rep] = ph == 0 ? run<0, true>(out, n_blocks, rows) : run<1, true>(out, n_blocks, rows);
    }
    const char* name = ph == 0 ? "phase A mix" : "phase C mix";
    for (int v = 0; v < 2; ++v) {
      float* t = v == 0 ? ts : tp;
      const int n = v == 0 ? n_scalar[ph] : n_packed[ph];
      printf("%s %-6s (%3d instr/row):", name, v == 0 ? "scalar" : "packed", n);
      for (int rep = 1; rep < 6; ++rep) printf(" %7.3f", t[rep] * 1e3 / (rows / 12));
      std::sort(t + 1, t + 6);
      printf("  median %7.3f us, spread %.3f; %.2f cycles per instruction and wave at 2.1 GHz\n", t[3] * 1e3 / (rows / 12),
             (t[5] - t[1]) * 1e3 / (rows / 12), t[3] * 1e6 * 2.1 / ((double)rows * n));
    }
  }
  (void)hipFree(out);
  return 0;
}
