// Local tone mapping kernels (isp_local_tonemap.h; the contract is DESIGN.md 3, "Local tone mapping").
//
// Every line one operation; f32 operations round once and are never contracted (the library builds with
// -ffp-contract=off), divisions are IEEE, >> is arithmetic, float-to-int conversions truncate:
//   li(t)  = (bits(min(max(t, floor), white)) - bits(floor)) >> 12
//   Y = ((r + b) * 0.25) + (g * 0.5);  l = li(Y);  z = f32(l) * zs
//   splat: zi = min(int(z + 0.5), bins - 1);  cnt[y / cell, x / cell, zi] += 1;  sum[...] += l
//   blur:  Nb = f32(B(cnt)), Sb = f32(B(sum)), B = [1 2 1] along the three axes, zero outside, exact in 64 bits
//   slice: gy = clamp((y + 0.5) * (1 / cell) - 0.5, 0, GH - 1), y0 = min(int(gy), max(GH - 2, 0)), y1 = min(y0 + 1, GH - 1),
//          fy = gy - y0, the same for x; z0 = min(int(z), bins - 2), fz = z - z0; lerp(a, b, f) = a + ((b - a) * f) along x,
//          then y, then z, for Nb and Sb separately; base = S / N when N > 0, else f32(l)
//   gain = float_from_bits(0x3F800000 + int((f32(li(anchor)) - base) * kq));  out_c = cast(v_c * gain)
//
// 1. splat_kernel: a work-group owns a square region of whole cells (SPLAT_CELLS at most), so it stores its cells' bins
//    with plain stores: no clear pass, no global atomics.  A thread takes GROUP pixels side by side, folds equal bins
//    among them and adds each run to its wave's replica of the bins in LDS with one 64-bit add.
// 2. blur_kernel: a thread per grid node, 27 taps from L2, 64-bit sums, two f32 planes.
// 3. apply_kernel: a work-group owns a REGION x REGION pixel tile; the grid nodes the tile can touch go to LDS as (N, S)
//    pairs, a thread slices its GROUP pixels of PASSES rows and rewrites them in place.  A row segment is read and
//    written by the lanes that own its pixels, each work-group its own tile: in place is safe.
// Both image kernels read (and 3. writes) the rows with accesses contiguous across the lanes: row_load / to_pixels below.
#include "isp_local_tonemap.h"

namespace ltm {

template <class T> struct Wide { typedef uint4 type; };            // 12 elements of T = three of these
template <> struct Wide<half_t> { typedef uint2 type; };

// ---- wave-cooperative rows ------------------------------------------------------------------------------------------
// A thread owns GROUP pixels side by side = 12 elements = three units of Wide<T>.  Accessed directly that is three wide
// accesses per lane at a 3-unit lane stride, which the memory pipeline serves at 3.7 TB/s against 6.2 TB/s for accesses
// that are contiguous across the lanes (isp_common.h, "wave-cooperative IO").  So on the wide path (whole groups per
// row, aligned rows) the `gpr` lanes of a row segment move its 3 * gpr units together - lane g takes units g, gpr + g and
// 2 gpr + g - and exchange them through the segment's LDS staging (the lanes of a segment share a wave, whose LDS
// operations execute in order: wave barriers only).  Off the wide path a lane moves its own pixels element by element.
// Measured (profiles/local_tonemap_timing.txt): with 16-byte units (f32) the exchange takes the apply kernel from 469 to
// 309 us per six 4K images; with 8-byte units (f16) both kernels are slower with it (apply 320 -> 351 us, splat 129 -> 176:
// they are bound by instruction issue, not by the loads), so f16 lanes take their own three units directly.
template <class T> struct Units { typename Wide<T>::type u[3]; };
template <class T> constexpr bool EXCHANGE = sizeof(T) == 4;

// the units of the row segment at seg: n_units of them lie inside the row (wide), or the lane's own n_px pixels at p
template <class T> MI_DEV void row_load(const T* seg, const T* p, bool wide, int g, int gpr, int n_units, int n_px, Units<T>& r) {
  typedef typename Wide<T>::type U;
  if (wide && EXCHANGE<T>) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int uj = j * gpr + g;
      if (uj < n_units) r.u[j] = reinterpret_cast<const U*>(seg)[uj];
    }
  } else if (wide) {                                               // (a whole group: one condition for the three loads)
    if (n_px > 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) r.u[j] = reinterpret_cast<const U*>(p)[j];
    }
  } else {
    T e[GROUP * 3];
#pragma unroll
    for (int j = 0; j < GROUP * 3; ++j) e[j] = j < n_px * 3 ? p[j] : (T)0.f;
    __builtin_memcpy(&r, e, sizeof(r));
  }
}

template <class T> MI_DEV void row_store(T* seg, T* p, bool wide, int g, int gpr, int n_units, int n_px, const Units<T>& r) {
  typedef typename Wide<T>::type U;
  if (wide && EXCHANGE<T>) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int uj = j * gpr + g;
      if (uj < n_units) reinterpret_cast<U*>(seg)[uj] = r.u[j];
    }
  } else if (wide) {
    if (n_px > 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) reinterpret_cast<U*>(p)[j] = r.u[j];
    }
  } else {
    T e[GROUP * 3];
    __builtin_memcpy(e, &r, sizeof(r));
#pragma unroll
    for (int j = 0; j < GROUP * 3; ++j)
      if (j < n_px * 3) p[j] = e[j];
  }
}

// the lane's own pixels from the units it loaded (st: the segment's staging, 3 * gpr units), and back
template <class T> MI_DEV void to_pixels(typename Wide<T>::type* st, bool wide, int g, int gpr, const Units<T>& r, T (&e)[GROUP * 3]) {
  Units<T> mine = r;
  if (wide && EXCHANGE<T>) {
#pragma unroll
    for (int j = 0; j < 3; ++j) st[j * gpr + g] = r.u[j];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 3; ++k) mine.u[k] = st[3 * g + k];
    __builtin_amdgcn_wave_barrier();
  }
  __builtin_memcpy(e, &mine, sizeof(mine));
}

template <class T> MI_DEV void from_pixels(typename Wide<T>::type* st, bool wide, int g, int gpr, const T (&e)[GROUP * 3], Units<T>& r) {
  Units<T> mine;
  __builtin_memcpy(&mine, e, sizeof(mine));
  r = mine;
  if (wide && EXCHANGE<T>) {
#pragma unroll
    for (int k = 0; k < 3; ++k) st[3 * g + k] = mine.u[k];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < 3; ++j) r.u[j] = st[j * gpr + g];
    __builtin_amdgcn_wave_barrier();
  }
}

// l = li(Y) of one pixel
MI_DEV int log_luma(const Args& a, float r, float g, float b) {
  const float rb = r + b;
  const float Y = (rb * 0.25f) + (g * 0.5f);
  const float c = fminf(fmaxf(Y, a.floor_v), a.white);
  return (__builtin_bit_cast(int, c) - a.floor_bits) >> 12;
}

// the fast path of an image: rows of whole groups that the wide accesses can take
template <class T> MI_DEV bool is_wide(const Args& a, const void* im) {
  return (a.W % GROUP) == 0 && (reinterpret_cast<uintptr_t>(im) % sizeof(typename Wide<T>::type)) == 0;
}

// grid (ceil(W / RS), ceil(H / RS), n_images), RS = the region side: 32 pixels for cell 8, else 64
template <class T>
__global__ void __launch_bounds__(THREADS) splat_kernel(const Args a) {
  // per wave, cell and bin: the count in the high word, the sum in the low one (a cell's sum is below 2^28: no carry),
  // so a run costs ONE LDS add
  __shared__ unsigned long long lds[WAVES][SPLAT_CELLS][MAX_BINS];
  {
    uint4* z = reinterpret_cast<uint4*>(&lds[0][0][0]);
    constexpr int N16 = (int)(sizeof(lds) / 16);
    for (int i = threadIdx.x; i < N16; i += THREADS) z[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();

  const T* im = static_cast<const T*>(a.im[blockIdx.z]);
  const int H = a.H, W = a.W, bins = a.bins;
  const int cs = a.cell == 64 ? 1 : (a.cell == 32 ? 2 : 4);        // cells per side of the region
  const int RS = cs << a.cell_shift;                               // 32 or 64
  const int gpr = RS / GROUP, rpp = THREADS / gpr;                 // groups per row, rows per pass
  const int g = threadIdx.x % gpr, rt = threadIdx.x / gpr;
  const int x = blockIdx.x * RS + g * GROUP;
  const int ry = blockIdx.y * RS;
  const bool wide = is_wide<T>(a, im);
  const int n_px = min(W - x, GROUP);                              // (<= 0: a group past the row)
  const int cxl = (g * GROUP) >> a.cell_shift;
  unsigned long long (*mine)[MAX_BINS] = lds[threadIdx.x >> 6];
  __shared__ typename Wide<T>::type stage[EXCHANGE<T> ? THREADS * 3 : 1];
  typename Wide<T>::type* st = stage + (threadIdx.x - g) * 3;      // (the segment's)
  const int x_seg = blockIdx.x * RS;
  const int n_units = min(3 * gpr, (W - x_seg) * 3 / 4);           // units of the segment inside the row (4 elements each)

  Units<T> raw[PASSES];
  bool ok[PASSES];                                                 // (a row of the region and of the image)
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int row = p * rpp + rt, y = ry + row;
    ok[p] = row < RS && y < H;
    if (ok[p]) row_load<T>(im + ((size_t)y * W + x_seg) * 3, im + ((size_t)y * W + x) * 3, wide, g, gpr, n_units, n_px, raw[p]);
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    if (!ok[p]) continue;
    T e[GROUP * 3];
    to_pixels<T>(st, wide, g, gpr, raw[p], e);
    if (n_px <= 0) continue;
    const int row = p * rpp + rt;
    unsigned long long* c = mine[(row >> a.cell_shift) * cs + cxl];
    int prev = -1;
    uint32_t rc = 0, rs = 0;
#pragma unroll
    for (int j = 0; j < GROUP; ++j) {
      if (j < n_px) {
        const int l = log_luma(a, (float)e[3 * j], (float)e[3 * j + 1], (float)e[3 * j + 2]);
        const float z = (float)l * a.zs;
        const int zi = min((int)(z + 0.5f), bins - 1);
        if (zi == prev) {
          ++rc;
          rs += (uint32_t)l;
        } else {
          if (rc) atomicAdd(&c[prev], ((unsigned long long)rc << 32) | rs);
          prev = zi;
          rc = 1;
          rs = (uint32_t)l;
        }
      }
    }
    if (rc) atomicAdd(&c[prev], ((unsigned long long)rc << 32) | rs);
  }
  __syncthreads();
  // the region's cells inside the grid, every bin of them: the sum of the waves' replicas, stored
  const size_t at = (size_t)blockIdx.z * a.plane;
  for (int i = threadIdx.x; i < cs * cs * bins; i += THREADS) {
    const int cl = i / bins, b = i - cl * bins;
    const int cy = blockIdx.y * cs + cl / cs, cx = blockIdx.x * cs + cl % cs;
    if (cy < a.GH && cx < a.GW) {
      unsigned long long v = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) v += lds[w][cl][b];
      const size_t o = at + ((size_t)cy * a.GW + cx) * bins + b;
      a.cnt[o] = (uint32_t)(v >> 32);
      a.sum[o] = (uint32_t)v;
    }
  }
}

// grid (ceil(GH * GW * bins / THREADS), 1, n_images)
__global__ void __launch_bounds__(THREADS) blur_kernel(const Args a) {
  const int GH = a.GH, GW = a.GW, bins = a.bins;
  const size_t nodes = (size_t)GH * GW * bins;
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= nodes) return;
  const int z = (int)(i % bins);
  const size_t yx = i / bins;
  const int gx = (int)(yx % GW), gy = (int)(yx / GW);
  const size_t at = (size_t)blockIdx.z * a.plane;
  const uint32_t* cnt = a.cnt + at;
  const uint32_t* sum = a.sum + at;
  uint64_t n = 0, s = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const int y = gy + dy;
    if (y < 0 || y >= GH) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int x = gx + dx;
      if (x < 0 || x >= GW) continue;
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz) {
        const int zz = z + dz;
        if (zz < 0 || zz >= bins) continue;
        const int sh = (dy == 0) + (dx == 0) + (dz == 0);          // weight 1, 2, 4 or 8
        const size_t o = ((size_t)y * GW + x) * bins + zz;
        n += (uint64_t)cnt[o] << sh;
        s += (uint64_t)sum[o] << sh;
      }
    }
  }
  a.nb[at + i] = (float)n;
  a.sb[at + i] = (float)s;
}

struct Axis {
  int i0, i1;
  float f;
};
// the two nodes and the weight of pixel p along an axis of G nodes
MI_DEV Axis axis_of(int p, float inv_cell, int G) {
  const float c = (float)p + 0.5f;
  const float q = c * inv_cell;
  const float g = fminf(fmaxf(q - 0.5f, 0.f), (float)(G - 1));
  const int i0 = min((int)g, max(G - 2, 0));
  return {i0, min(i0 + 1, G - 1), g - (float)i0};
}

MI_DEV float lerp(float a, float b, float f) {
  const float d = b - a;
  return a + (d * f);
}
// the same on an (N, S) pair: packed f32 instructions, each half rounded as the scalar operation
typedef float pair_t __attribute__((ext_vector_type(2)));
MI_DEV pair_t lerp2(pair_t a, pair_t b, float f) {
  const pair_t d = b - a;
  return a + (d * f);
}

// grid (ceil(W / REGION), ceil(H / REGION), n_images); dynamic LDS: the (N, S) pairs of the tile's nodes
template <class T>
__global__ void __launch_bounds__(THREADS) apply_kernel(const Args a) {
  extern __shared__ pair_t node[];                                 // [ny][nx][bins], (N, S)
  T* im = static_cast<T*>(a.im[blockIdx.z]);
  const int H = a.H, W = a.W, bins = a.bins;
  const int g = threadIdx.x % ROW_GROUPS, rt = threadIdx.x / ROW_GROUPS;
  const int c0 = blockIdx.x * REGION, r0 = blockIdx.y * REGION;
  const int x = c0 + g * GROUP;
  const bool wide = is_wide<T>(a, im);
  const int n_px = min(W - x, GROUP);

  __shared__ typename Wide<T>::type stage[EXCHANGE<T> ? THREADS * 3 : 1];
  typename Wide<T>::type* st = stage + (threadIdx.x - g) * 3;      // (the segment's)
  const int n_units = min(3 * ROW_GROUPS, (W - c0) * 3 / 4);       // units of the segment inside the row (4 elements each)

  Units<T> raw[PASSES];
  bool ok[PASSES];                                                 // (a row of the image)
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int y = r0 + p * (THREADS / ROW_GROUPS) + rt;
    ok[p] = y < H;
    if (ok[p]) row_load<T>(im + ((size_t)y * W + c0) * 3, im + ((size_t)y * W + x) * 3, wide, g, ROW_GROUPS, n_units, n_px, raw[p]);
  }

  // the nodes of the tile: the first node of its first row / column to the second node of its last (axis_of grows with p)
  const int ylo = axis_of(r0, a.inv_cell, a.GH).i0, yhi = axis_of(min(r0 + REGION, H) - 1, a.inv_cell, a.GH).i1;
  const int xlo = axis_of(c0, a.inv_cell, a.GW).i0, xhi = axis_of(min(c0 + REGION, W) - 1, a.inv_cell, a.GW).i1;
  const int nx = xhi - xlo + 1, rowlen = nx * bins, total = (yhi - ylo + 1) * rowlen;
  const size_t at = (size_t)blockIdx.z * a.plane;
  for (int i = threadIdx.x; i < total; i += THREADS) {
    const int iy = i / rowlen, r = i - iy * rowlen;                // (r: the node's x and bin, contiguous in the planes)
    const size_t o = at + ((size_t)(ylo + iy) * a.GW + xlo) * bins + r;
    node[i] = pair_t{a.nb[o], a.sb[o]};
  }
  __syncthreads();

  Axis ax[GROUP];
#pragma unroll
  for (int j = 0; j < GROUP; ++j) ax[j] = axis_of(min(x + j, W - 1), a.inv_cell, a.GW);

#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    if (!ok[p]) continue;
    const int y = r0 + p * (THREADS / ROW_GROUPS) + rt;
    const Axis ay = axis_of(y, a.inv_cell, a.GH);
    const int row0 = (ay.i0 - ylo) * rowlen, row1 = (ay.i1 - ylo) * rowlen;
    T e[GROUP * 3], out[GROUP * 3];
    to_pixels<T>(st, wide, g, ROW_GROUPS, raw[p], e);
#pragma unroll
    for (int j = 0; j < GROUP; ++j) {
      const float v0 = (float)e[3 * j], v1 = (float)e[3 * j + 1], v2 = (float)e[3 * j + 2];
      const int l = log_luma(a, v0, v1, v2);
      const float z = (float)l * a.zs;
      const int z0 = min((int)z, bins - 2);
      const float fz = z - (float)z0;
      const int col0 = (ax[j].i0 - xlo) * bins + z0, col1 = (ax[j].i1 - xlo) * bins + z0;
      pair_t q[2][2];                                              // [y][z], lerped along x
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int row = k ? row1 : row0;
#pragma unroll
        for (int d = 0; d < 2; ++d) q[k][d] = lerp2(node[row + col0 + d], node[row + col1 + d], ax[j].f);
      }
      const pair_t ns = lerp2(lerp2(q[0][0], q[1][0], ay.f), lerp2(q[0][1], q[1][1], ay.f), fz);
      const float N = ns.x, S = ns.y;
      const float base = N > 0.f ? S / N : (float)l;
      const float d = a.la - base;
      const int ei = (int)(d * a.kq);
      const float gain = __builtin_bit_cast(float, 0x3F800000 + ei);
      out[3 * j] = cast_out<T>(v0 * gain);
      out[3 * j + 1] = cast_out<T>(v1 * gain);
      out[3 * j + 2] = cast_out<T>(v2 * gain);
    }
    Units<T> done;
    from_pixels<T>(st, wide, g, ROW_GROUPS, out, done);
    row_store<T>(im + ((size_t)y * W + c0) * 3, im + ((size_t)y * W + x) * 3, wide, g, ROW_GROUPS, n_units, n_px, done);
  }
}

template <class T>
static int launch_t(const Args& a, int from, int to, hipStream_t stream) {
  const unsigned n = (unsigned)a.n_images;
  if (from <= 0 && to >= 0) {
    const int rs = a.cell == 8 ? 32 : REGION;
    hipLaunchKernelGGL(splat_kernel<T>, dim3((unsigned)((a.W + rs - 1) / rs), (unsigned)((a.H + rs - 1) / rs), n),
                       dim3(THREADS), 0, stream, a);
    MI_LAUNCH_CHECK();
  }
  if (from <= 1 && to >= 1) {
    const size_t nodes = (size_t)a.GH * a.GW * a.bins;
    hipLaunchKernelGGL(blur_kernel, dim3((unsigned)((nodes + THREADS - 1) / THREADS), 1, n), dim3(THREADS), 0, stream, a);
    MI_LAUNCH_CHECK();
  }
  if (from <= 2 && to >= 2) {
    const int most = REGION / a.cell + 2;                          // nodes a tile can touch along an axis
    const int ny = most < a.GH ? most : a.GH, nx = most < a.GW ? most : a.GW;
    const size_t lds = (size_t)ny * nx * a.bins * sizeof(pair_t);  // <= 25600 bytes
    hipLaunchKernelGGL(apply_kernel<T>, dim3((unsigned)((a.W + REGION - 1) / REGION), (unsigned)((a.H + REGION - 1) / REGION), n),
                       dim3(THREADS), lds, stream, a);
    MI_LAUNCH_CHECK();
  }
  return 0;
}

int launch(const Args& a, int dtype, int from, int to, hipStream_t stream) {
  if (a.n_images <= 0 || a.H <= 0 || a.W <= 0) return 0;
  return dtype == MI_F16 ? launch_t<half_t>(a, from, to, stream) : launch_t<float>(a, from, to, stream);
}

}  // namespace ltm
