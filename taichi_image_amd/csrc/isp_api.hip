// C ABI of the tile-based entry points (demosaic, fused load, fused config-2 pipeline) plus the
// library-wide plumbing (version, error string, workspace size).
#include <stdarg.h>
#include <stdlib.h>
#include <cmath>

#include "isp_elementwise.h"
#include "isp_tile.h"
#include "isp_resize_tile.h"
#include "isp_stream.h"
#include "isp_mega.h"
#include "isp_mega_cam.h"
#include "isp_stream_resize.h"
#include "isp_defects.h"
#include "isp_lens.h"
#include "isp_awb.h"
#include "isp_denoise.h"
#include "isp_highlights.h"
#include "isp_dynamic_defects.h"
#include "isp_green_equalize.h"
#include "isp_statistics.h"
#include "isp_demosaic_dir.h"
#include "isp_chromatic.h"
#include "isp_temporal.h"
#include "isp_exposure_merge.h"
#include "isp_sharpen.h"
#include "isp_chroma_denoise.h"
#include "isp_luma_denoise.h"
#include "isp_color_lut.h"
#include "isp_local_contrast.h"
#include "isp_local_tonemap.h"
#include "isp_resample.h"
#include <mutex>
#include <atomic>

static thread_local char g_err[512] = "";

void mi_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" int mi_isp_version(void) { return 1900; }  // 0.1.0 -> major*1e4 + minor*1e3 ... (monotone)
extern "C" const char* mi_isp_last_error(void) { return g_err; }

extern "C" int mi_isp_bayer_weights(int32_t out[4 * 13 * 3]) {
  MI_REQUIRE(out, "bayer_weights: null pointer");
  // host copy of the table the kernels are compiled with (isp_tile.h: tile::KW)
  static const int8_t kw[4][13][3] = {
      {{0, -2, -3}, {0, 0, 4}, {0, 4, 0}, {0, 0, 4}, {0, -2, -3}, {0, 4, 0}, {16, 8, 12},
       {0, 4, 0}, {0, -2, -3}, {0, 0, 4}, {0, 4, 0}, {0, 0, 4}, {0, -2, -3}},
      {{-2, 0, 1}, {-2, 0, -2}, {8, 0, 0}, {-2, 0, -2}, {1, 0, -2}, {0, 0, 8}, {10, 16, 10},
       {0, 0, 8}, {1, 0, -2}, {-2, 0, -2}, {8, 0, 0}, {-2, 0, -2}, {-2, 0, 1}},
      {{1, 0, -2}, {-2, 0, -2}, {0, 0, 8}, {-2, 0, -2}, {-2, 0, 1}, {8, 0, 0}, {10, 16, 10},
       {8, 0, 0}, {-2, 0, 1}, {-2, 0, -2}, {0, 0, 8}, {-2, 0, -2}, {1, 0, -2}},
      {{-3, -2, 0}, {4, 0, 0}, {0, 4, 0}, {4, 0, 0}, {-3, -2, 0}, {0, 4, 0}, {12, 8, 16},
       {0, 4, 0}, {-3, -2, 0}, {4, 0, 0}, {0, 4, 0}, {4, 0, 0}, {-3, -2, 0}}};
  for (int k = 0; k < 4; ++k)
    for (int t = 0; t < 13; ++t)
      for (int c = 0; c < 3; ++c) out[(k * 13 + t) * 3 + c] = kw[k][t][c];
  return 0;
}

extern "C" size_t mi_isp_workspace_bytes(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
#ifdef MI_STREAM_STAMPS
  return (size_t)(FP_COUNT + ((size_t)strm::PART_ROWS + 16) * (size_t)mi_partial_cap(H, W)) * sizeof(float);
#endif
  return (size_t)(FP_COUNT + (size_t)strm::PART_ROWS * (size_t)mi_partial_cap(H, W)) * sizeof(float);
}

// ---------------------------------------------------------------------------------------------
static int fill_common(tile::Params& p, int H, int W, int pattern, const float* ccm9, const char* who) {
  MI_REQUIRE(H > 0 && W > 0, "%s: bad shape %dx%d", who, H, W);
  MI_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: image must be even size, got %dx%d", who, H, W);  // bayer.py:206
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: bad pattern %d", who, pattern);
  p.H = H; p.W = W;
  p.has_ccm = ccm9 != nullptr;
  for (int i = 0; i < 9; ++i) p.ccm[i] = ccm9 ? ccm9[i] : (i % 4 == 0 ? 1.f : 0.f);
  p.gamma_inv = 1.f; p.la = 1.f; p.ca = 0.f;
  tile::set_weights(p);
  return 0;
}

static int vec_store_ok(const void* dst, int W, int out_dtype) {
  // a strip row is 24 contiguous elements at element offset (r*W + c)*3, c % 8 == 0
  return W % 8 == 0 && mi_aligned(dst, out_dtype == MI_U8 ? 8 : 16);
}

extern "C" int mi_isp_demosaic(const void* cfa, void* rgb, int H, int W, int in_dtype, int out_dtype, int pattern,
                               const float* ccm9, void* stream) {
  MI_REQUIRE(cfa && rgb, "demosaic: null pointer");
  MI_REQUIRE(mi_valid_dtype(in_dtype) && mi_valid_dtype(out_dtype), "demosaic: bad dtype");
  tile::Params p = {};
  if (int rc = fill_common(p, H, W, pattern, ccm9, "demosaic")) return rc;
  p.src = cfa; p.dst = rgb;
  p.src_kind = in_dtype;                       // SRC_CFA_* share the MI_* numbering
  p.out_dtype = out_dtype;
  p.vec_store = vec_store_ok(rgb, W, out_dtype);
  p.in_scale = mi_scale_factor(in_dtype);
  p.out_scale = mi_scale_factor(out_dtype);
  // work type: f16 holds u8 and f16 inputs exactly; u16 / f32 need f32
  const int work = (in_dtype == MI_U8 || in_dtype == MI_F16) ? MI_F16 : MI_F32;
  return tile::launch(p, work, pattern, tile::EPI_STORE, (hipStream_t)stream);
}

static int packed_params(tile::Params& p, const uint8_t* packed, int H, int W, int bits, int ids_format,
                         int work_dtype, const char* who) {
  MI_REQUIRE(packed, "%s: null packed pointer", who);
  MI_REQUIRE(bits == 12 || bits == 16, "%s: bits must be 12 or 16, got %d", who, bits);
  MI_REQUIRE(work_dtype == MI_F16 || work_dtype == MI_F32, "%s: work dtype must be f16 or f32", who);
  p.src = packed;
  p.src_kind = bits == 16 ? tile::SRC_PACKED16 : (ids_format ? tile::SRC_PACKED12_IDS : tile::SRC_PACKED12);
  p.src_fast = bits == 16 ? (W % 8 == 0 && mi_aligned(packed, 16)) : (W % 8 == 0 && mi_aligned(packed, 4));
  p.in_scale = 1.f;                            // the decoded CFA is f16/f32 in [0, 1]
  p.k_decode = (float)(1.0 / (bits == 16 ? 65535.0 : 4095.0));   // packed.py:99,140 with scale 1.0
  return 0;
}

// sensor levels (mi_isp_levels) of a packed source: NULL leaves Params::levels 0 (the kernels without levels)
static int apply_levels(tile::Params& p, const mi_isp_levels* lv, int bits, const char* who) {
  if (!lv) { p.levels = 0; return 0; }
  if (int rc = mi_check_levels(lv, bits == 16 ? 65535 : 4095, who, p.lv_black)) return rc;
  bool uniform = true;
  for (int s = 0; s < 4; ++s) {
    p.lv_k[s] = (float)(1.0 / (double)(lv->white - lv->black[s]));       // S = 1 for the f16 / f32 work dtypes
    uniform = uniform && lv->black[s] == lv->black[0];
  }
  p.levels = uniform ? 1 : 2;
  return 0;
}

// sensor levels and lens shading of a packed source.  A shading grid always takes the per-site register decode
// (levels 2): without levels it decodes with black 0 and k_decode, which is the plain decode.
static int apply_levels_shading(tile::Params& p, const mi_isp_levels* lv, const mi_isp_shading* sh, int bits,
                                const char* who) {
  if (int rc = apply_levels(p, lv, bits, who)) return rc;
  if (int rc = apply_shading(p, sh, p.H, p.W, who)) return rc;
  if (p.shading) {
    if (p.levels == 0)
      for (int s = 0; s < 4; ++s) { p.lv_black[s] = 0; p.lv_k[s] = p.k_decode; }
    p.levels = 2;
  }
  return 0;
}

// the _shading twins check their grid first, before any other argument (apply_shading again fills it per frame)
static int check_shading(const mi_isp_shading* sh, const char* who) {
  tile::Params p = {};
  return apply_shading(p, sh, 2, 2, who);
}

#ifdef MI_STREAM_STAMPS
// measurement build only: a home for the in-kernel stamps of the kernels that take no workspace (16 words per wave)
static float* stamp_buffer() {
  static float* buf = nullptr;
  if (!buf && hipMalloc(&buf, 4096 * 16 * 4) == hipSuccess) (void)hipMemset(buf, 0, 4096 * 16 * 4);
  return buf;
}
extern "C" int mi_isp_debug_read_stamps(void* host_out, int n_waves) {
  MI_REQUIRE(host_out && n_waves > 0 && n_waves <= 4096, "debug_read_stamps: bad arguments");
  MI_HIP(hipDeviceSynchronize());
  MI_HIP(hipMemcpy(host_out, stamp_buffer(), (size_t)n_waves * 16 * 4, hipMemcpyDeviceToHost));
  MI_HIP(hipMemset(stamp_buffer(), 0, 4096 * 16 * 4));
  return 0;
}
#endif

// The streaming kernels (isp_stream.h) take the standard 12-bit layout with aligned rows and whole 8-pixel units and
// store through 16-byte units; everything else stays with the tile kernels.  MI_ISP_MEASURE builds can switch them
// off (MI_ISP_NO_STREAM=1) to time the tile path.
static bool use_stream(const tile::Params& p, int work_dtype, const void* out, int out_dtype) {
#ifdef MI_ISP_MEASURE
  static const bool off = getenv("MI_ISP_NO_STREAM") != nullptr;
  if (off) return false;
#endif
  return strm::supported(p, work_dtype) && (!out || vec_store_ok(out, p.W, out_dtype)) &&
         (int64_t)p.H * p.W * 3 * (int64_t)mi_dtype_size(out_dtype) < (int64_t)strm::INVALID_OFF;
}

static int load_packed_impl(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                            int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                            void* sub, int sub_stride, const mi_isp_levels* lv, const mi_isp_shading* sh,
                            void* stream) {
  MI_REQUIRE(rgb, "load_packed: null output");
  tile::Params p = {};
  if (int rc = fill_common(p, H, W, pattern, ccm9, "load_packed")) return rc;
  if (int rc = packed_params(p, packed, H, W, bits, ids_format, work_dtype, "load_packed")) return rc;
  if (int rc = apply_levels_shading(p, lv, sh, bits, "load_packed")) return rc;
  p.dst = rgb; p.out_dtype = work_dtype; p.out_scale = 1.f;
  if (scale > 0.f) {
    // unpack -> demosaic -> bilinear fused (isp_resize_tile.h); the caller checks the scale first
    MI_REQUIRE(Hd > 0 && Wd > 0 && H >= 2 && W >= 2, "load_packed: bad output shape %dx%d", Hd, Wd);
    if (use_stream(p, work_dtype, nullptr, work_dtype) && rstrm::supported(p, work_dtype, rgb, Hd, Wd, scale, scale)) {
      rstrm::RSArgs ra = {};
      ra.t = p; ra.Hd = Hd; ra.Wd = Wd; ra.s0 = scale; ra.s1 = scale;
      rstrm::geometry(H, W, ra);
#ifdef MI_STREAM_STAMPS
      ra.t.partials = stamp_buffer(); ra.t.part_stride = 0;      // this entry point has no workspace: a buffer of the build
#endif
      if (int rc = rstrm::launch(ra, pattern, (hipStream_t)stream)) return rc;
      if (sub) return ew::subsample(rgb, sub, Hd, Wd, sub_stride, work_dtype, (hipStream_t)stream);
      return 0;
    }
    MI_REQUIRE(rtile::scales_fit(scale, scale), "load_packed: scale %g is outside the fused kernel's range "
               "(mi_isp_load_packed_scale_supported); resize separately", (double)scale);
    rtile::RParams rp = {};
    rp.t = p; rp.Hd = Hd; rp.Wd = Wd; rp.s0 = scale; rp.s1 = scale;
    if (int rc = rtile::launch(rp, work_dtype, pattern, (hipStream_t)stream)) return rc;
    if (sub) return ew::subsample(rgb, sub, Hd, Wd, sub_stride, work_dtype, (hipStream_t)stream);
    return 0;
  }
  MI_REQUIRE(Hd == H && Wd == W, "load_packed: output shape must equal the frame when scale <= 0");
  p.vec_store = vec_store_ok(rgb, W, work_dtype);
  if (use_stream(p, work_dtype, rgb, work_dtype)) {
    strm::SArgs a = {};
    a.t = p;
    strm::geometry(H, W, a);
    if (sub && sub_stride == 8) { a.sub = sub; a.sub_w = (W + 7) / 8; }   // the metering subsample on the way
    if (int rc = strm::launch(a, work_dtype, pattern, strm::S_STORE, (hipStream_t)stream)) return rc;
    if (sub && sub_stride != 8) return ew::subsample(rgb, sub, H, W, sub_stride, work_dtype, (hipStream_t)stream);
    return 0;
  }
  if (int rc = tile::launch(p, work_dtype, pattern, tile::EPI_STORE, (hipStream_t)stream)) return rc;
  if (sub) return ew::subsample(rgb, sub, H, W, sub_stride, work_dtype, (hipStream_t)stream);
  return 0;
}

extern "C" int mi_isp_load_packed(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                  int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                                  void* stream) {
  return load_packed_impl(packed, rgb, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale, nullptr, 0,
                          nullptr, nullptr, stream);
}

extern "C" int mi_isp_load_packed_levels(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                         int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                                         const mi_isp_levels* levels, void* stream) {
  return load_packed_impl(packed, rgb, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale, nullptr, 0,
                          levels, nullptr, stream);
}

extern "C" int mi_isp_load_packed_shading(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                          int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                                          const mi_isp_levels* levels, const mi_isp_shading* shading, void* stream) {
  if (int rc = check_shading(shading, "load_packed")) return rc;
  return load_packed_impl(packed, rgb, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale, nullptr, 0,
                          levels, shading, stream);
}

// The cameras of a group in ONE launch per 8 (grid.y = camera): dispatch, decode table, first loads and drain are paid per
// launch instead of per camera (the load kernels take 23 - 30 us each, ~4 us of that is launch overhead: config 3, six
// cameras, 43.0 -> ~39.5 us per frame).  Same arithmetic, same bits as n calls of mi_isp_load_packed[_metered].
static int load_packed_batch_impl(const uint8_t* const* packed, void* const* rgb, void* const* subs, int n, int H, int W,
                                  int bits, int ids_format, int pattern, const float* ccm9, int work_dtype, int Hd,
                                  int Wd, float scale, int sub_stride, const mi_isp_levels* lv, const mi_isp_shading* sh,
                                  void* stream) {
  MI_REQUIRE(packed && rgb, "load_packed_batch: null pointer");
  MI_REQUIRE(n >= 0, "load_packed_batch: negative frame count");
  for (int i = 0; i < n; ++i) MI_REQUIRE(packed[i] && rgb[i] && (!subs || subs[i]), "load_packed_batch: frame %d has a null buffer", i);
  if (n == 0) return 0;
  MI_REQUIRE(!subs || sub_stride >= 1, "load_packed_batch: bad subsample stride");
  // does every frame take the same streaming kernel?  (alignment is per buffer)
  tile::Params p0 = {};
  bool same = true, resize = scale > 0.f;
  for (int i = 0; i < n && same; ++i) {
    tile::Params p = {};
    if (int rc = fill_common(p, H, W, pattern, ccm9, "load_packed_batch")) return rc;
    if (int rc = packed_params(p, packed[i], H, W, bits, ids_format, work_dtype, "load_packed_batch")) return rc;
    if (int rc = apply_levels_shading(p, lv, sh, bits, "load_packed_batch")) return rc;
    p.dst = rgb[i]; p.out_dtype = work_dtype; p.out_scale = 1.f;
    if (resize) {
      same = Hd > 0 && Wd > 0 && H >= 2 && W >= 2 && use_stream(p, work_dtype, nullptr, work_dtype) &&
             rstrm::supported(p, work_dtype, rgb[i], Hd, Wd, scale, scale);
    } else {
      p.vec_store = vec_store_ok(rgb[i], W, work_dtype);
      same = Hd == H && Wd == W && use_stream(p, work_dtype, rgb[i], work_dtype) && (!subs || sub_stride == 8);
    }
    if (i == 0) p0 = p;
  }
  if (!same) {                                               // some frame needs another kernel: one by one
    for (int i = 0; i < n; ++i)
      if (int rc = load_packed_impl(packed[i], rgb[i], H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale,
                                    subs ? subs[i] : nullptr, sub_stride, lv, sh, stream))
        return rc;
    return 0;
  }
  for (int i0 = 0; i0 < n; i0 += strm::LOAD_BATCH) {
    const int m = n - i0 < strm::LOAD_BATCH ? n - i0 : strm::LOAD_BATCH;
    if (resize) {
      rstrm::RSArgs ra = {};
      ra.t = p0; ra.Hd = Hd; ra.Wd = Wd; ra.s0 = scale; ra.s1 = scale;
      rstrm::geometry(H, W, ra);
      ra.n_batch = m;
      for (int i = 0; i < m; ++i) { ra.srcs[i] = packed[i0 + i]; ra.dsts[i] = rgb[i0 + i]; }
#ifdef MI_STREAM_STAMPS
      ra.t.partials = stamp_buffer(); ra.t.part_stride = 0;
#endif
      if (int rc = rstrm::launch(ra, pattern, (hipStream_t)stream)) return rc;
      if (subs)
        for (int i = 0; i < m; ++i)
          if (int rc = ew::subsample(rgb[i0 + i], subs[i0 + i], Hd, Wd, sub_stride, work_dtype, (hipStream_t)stream)) return rc;
    } else {
      strm::SArgs a = {};
      a.t = p0;
      strm::geometry(H, W, a);
      a.n_batch = m; a.sub_w = (W + 7) / 8;
      for (int i = 0; i < m; ++i) { a.srcs[i] = packed[i0 + i]; a.dsts[i] = rgb[i0 + i]; a.subs[i] = subs ? subs[i0 + i] : nullptr; }
      if (int rc = strm::launch(a, work_dtype, pattern, strm::S_STORE, (hipStream_t)stream)) return rc;
    }
  }
  return 0;
}

extern "C" int mi_isp_load_packed_batch(const uint8_t* const* packed, void* const* rgb, void* const* subs, int n, int H, int W,
                                        int bits, int ids_format, int pattern, const float* ccm9, int work_dtype, int Hd,
                                        int Wd, float scale, int sub_stride, void* stream) {
  return load_packed_batch_impl(packed, rgb, subs, n, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale,
                                sub_stride, nullptr, nullptr, stream);
}

extern "C" int mi_isp_load_packed_batch_levels(const uint8_t* const* packed, void* const* rgb, void* const* subs, int n, int H,
                                               int W, int bits, int ids_format, int pattern, const float* ccm9,
                                               int work_dtype, int Hd, int Wd, float scale, int sub_stride,
                                               const mi_isp_levels* levels, void* stream) {
  return load_packed_batch_impl(packed, rgb, subs, n, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale,
                                sub_stride, levels, nullptr, stream);
}

extern "C" int mi_isp_load_packed_batch_shading(const uint8_t* const* packed, void* const* rgb, void* const* subs, int n,
                                                int H, int W, int bits, int ids_format, int pattern, const float* ccm9,
                                                int work_dtype, int Hd, int Wd, float scale, int sub_stride,
                                                const mi_isp_levels* levels, const mi_isp_shading* shading, void* stream) {
  if (int rc = check_shading(shading, "load_packed_batch")) return rc;
  return load_packed_batch_impl(packed, rgb, subs, n, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale,
                                sub_stride, levels, shading, stream);
}

extern "C" int mi_isp_load_packed_metered_is_fused(int H, int W, int bits, int ids_format, int work_dtype, int sub_stride) {
  if (bits != 12 || ids_format || sub_stride != 8 || H <= 0 || W <= 0) return 0;
  tile::Params p = {};
  p.H = H; p.W = W; p.src_kind = tile::SRC_PACKED12; p.src_fast = ((int64_t)W * 3 / 2) % 4 == 0; p.in_scale = 1.f;
  return strm::supported(p, work_dtype) && (int64_t)H * W * 3 * (int64_t)mi_dtype_size(work_dtype) < (int64_t)strm::INVALID_OFF ? 1 : 0;
}

extern "C" int mi_isp_load_packed_metered(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                          int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                                          void* sub, int sub_stride, void* stream) {
  MI_REQUIRE(sub && sub_stride >= 1, "load_packed_metered: need a subsample buffer and a positive stride");
  return load_packed_impl(packed, rgb, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale, sub, sub_stride,
                          nullptr, nullptr, stream);
}

extern "C" int mi_isp_load_packed_metered_levels(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                                 int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                                                 void* sub, int sub_stride, const mi_isp_levels* levels, void* stream) {
  MI_REQUIRE(sub && sub_stride >= 1, "load_packed_metered: need a subsample buffer and a positive stride");
  return load_packed_impl(packed, rgb, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale, sub, sub_stride,
                          levels, nullptr, stream);
}

extern "C" int mi_isp_load_packed_metered_shading(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                                  int pattern, const float* ccm9, int work_dtype, int Hd, int Wd,
                                                  float scale, void* sub, int sub_stride, const mi_isp_levels* levels,
                                                  const mi_isp_shading* shading, void* stream) {
  if (int rc = check_shading(shading, "load_packed_metered")) return rc;
  MI_REQUIRE(sub && sub_stride >= 1, "load_packed_metered: need a subsample buffer and a positive stride");
  return load_packed_impl(packed, rgb, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale, sub, sub_stride,
                          levels, shading, stream);
}

extern "C" int mi_isp_load_packed_scale_supported(float scale) { return rtile::scales_fit(scale, scale) ? 1 : 0; }

// ---- defective pixel correction (mi_isp_defects) ---------------------------------------------------------
static int check_defects(const mi_isp_defects* d, const char* who) {
  MI_REQUIRE(d, "%s: null defect map", who);
  MI_REQUIRE(d->n >= 0, "%s: negative defect count %d", who, (int)d->n);
  MI_REQUIRE(d->n == 0 || (d->coords_dev && d->mask_dev), "%s: %d defects without coordinates or mask", who, (int)d->n);
  return 0;
}

// the fix-up of n packed frames sharing one geometry: camera i (maps[i] may be NULL: no correction) recomputes the
// n_outputs[i] pixels of outputs[i]; one launch per MAX_CAMS cameras that have outputs
static int defects_fix_packed_impl(const uint8_t* const* packed, void* const* rgb, void* const* subs, int n, int H, int W,
                                   int bits, int ids_format, int pattern, const float* ccm9, int work_dtype, int Hd,
                                   int Wd, float scale, int sub_stride, const mi_isp_levels* lv, const mi_isp_shading* sh,
                                   const mi_isp_defects* const* maps, const int32_t* const* outputs,
                                   const int32_t* n_outputs, void* stream, const char* who) {
  MI_REQUIRE(n >= 0, "%s: negative frame count", who);
  if (n == 0) return 0;
  MI_REQUIRE(packed && rgb && maps && outputs && n_outputs, "%s: null pointer", who);
  if (sh)
    if (int rc = check_shading(sh, who)) return rc;
  dfx::Args a = {};
  if (int rc = fill_common(a.t, H, W, pattern, ccm9, who)) return rc;
  if (int rc = packed_params(a.t, packed[0], H, W, bits, ids_format, work_dtype, who)) return rc;
  if (int rc = apply_levels_shading(a.t, lv, sh, bits, who)) return rc;
  if (a.t.levels == 0)                                     // the plain decode through the per-site arrays
    for (int s = 0; s < 4; ++s) { a.t.lv_black[s] = 0; a.t.lv_k[s] = a.t.k_decode; }
  MI_REQUIRE(Hd > 0 && Wd > 0, "%s: bad output shape %dx%d", who, Hd, Wd);
  MI_REQUIRE(scale > 0.f || (Hd == H && Wd == W), "%s: output shape must equal the frame when scale <= 0", who);
  MI_REQUIRE(!subs || sub_stride >= 1, "%s: bad subsample stride %d", who, sub_stride);
  a.Hd = Hd; a.Wd = Wd; a.resize = scale > 0.f; a.s = scale;
  a.st = subs ? sub_stride : 1; a.sub_w = subs ? (Wd + sub_stride - 1) / sub_stride : 0;
  a.pr = pattern >> 1; a.pc = pattern & 1;                 // RGGB 0, GRBG 1, GBRG 2, BGGR 3
  a.mask_w = (W + 31) / 32;
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(packed[i] && rgb[i] && (!subs || subs[i]), "%s: frame %d has a null buffer", who, i);
    if (!maps[i]) continue;
    if (int rc = check_defects(maps[i], who)) return rc;
    MI_REQUIRE(n_outputs[i] >= 0 && (int64_t)n_outputs[i] <= (int64_t)Hd * Wd, "%s: frame %d lists %d outputs of %dx%d",
               who, i, (int)n_outputs[i], Hd, Wd);
    MI_REQUIRE(n_outputs[i] == 0 || (outputs[i] && maps[i]->n > 0), "%s: frame %d lists outputs without them or a map",
               who, i);
  }
  for (int i = 0; i < n; ++i) {
    if (maps[i] && n_outputs[i] > 0) {
      dfx::Cam& c = a.cam[a.n_cams++];
      c.src = packed[i]; c.dst = rgb[i]; c.sub = subs ? subs[i] : nullptr; c.mask = maps[i]->mask_dev;
      c.list = outputs[i]; c.start = a.total; c.n = n_outputs[i];
      MI_REQUIRE((int64_t)a.total + c.n < (int64_t)INT32_MAX, "%s: too many outputs in one launch", who);
      a.total += c.n;
    }
    if (a.n_cams == dfx::MAX_CAMS || (i == n - 1 && a.n_cams > 0)) {
      if (int rc = dfx::launch_packed(a, work_dtype, (hipStream_t)stream)) return rc;
      a.n_cams = 0; a.total = 0;
    }
  }
  return 0;
}

extern "C" int mi_isp_defects_fix_packed(const uint8_t* packed, void* rgb, int H, int W, int bits, int ids_format,
                                         int pattern, const float* ccm9, int work_dtype, int Hd, int Wd, float scale,
                                         void* sub, int sub_stride, const mi_isp_levels* levels,
                                         const mi_isp_shading* shading, const mi_isp_defects* defects,
                                         const int32_t* outputs, int n_outputs, void* stream) {
  MI_REQUIRE(packed && rgb, "defects_fix_packed: null pointer");
  if (int rc = check_defects(defects, "defects_fix_packed")) return rc;
  void* const subs[1] = {sub};
  const mi_isp_defects* const maps[1] = {defects};
  const int32_t* const outs[1] = {outputs};
  const int32_t counts[1] = {n_outputs};
  return defects_fix_packed_impl(&packed, &rgb, sub ? subs : nullptr, 1, H, W, bits, ids_format, pattern, ccm9,
                                 work_dtype, Hd, Wd, scale, sub_stride, levels, shading, maps, outs, counts, stream,
                                 "defects_fix_packed");
}

extern "C" int mi_isp_defects_fix_packed_batch(const uint8_t* const* packed, void* const* rgb, void* const* subs, int n,
                                               int H, int W, int bits, int ids_format, int pattern, const float* ccm9,
                                               int work_dtype, int Hd, int Wd, float scale, int sub_stride,
                                               const mi_isp_levels* levels, const mi_isp_shading* shading,
                                               const mi_isp_defects* const* defects, const int32_t* const* outputs,
                                               const int32_t* n_outputs, void* stream) {
  return defects_fix_packed_impl(packed, rgb, subs, n, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd, scale,
                                 sub_stride, levels, shading, defects, outputs, n_outputs, stream,
                                 "defects_fix_packed_batch");
}

extern "C" int mi_isp_defects_fix_cfa(void* cfa, int H, int W, int work_dtype, const mi_isp_defects* defects,
                                      void* stream) {
  MI_REQUIRE(cfa, "defects_fix_cfa: null pointer");
  MI_REQUIRE(H > 0 && W > 0, "defects_fix_cfa: bad shape %dx%d", H, W);
  MI_REQUIRE(work_dtype == MI_F16 || work_dtype == MI_F32, "defects_fix_cfa: work dtype must be f16 or f32");
  if (int rc = check_defects(defects, "defects_fix_cfa")) return rc;
  MI_REQUIRE((int64_t)defects->n <= (int64_t)H * W, "defects_fix_cfa: %d defects in a %dx%d frame", (int)defects->n, H, W);
  return dfx::launch_cfa(cfa, H, W, work_dtype, defects->coords_dev, defects->n, defects->mask_dev, (hipStream_t)stream);
}

// ---- lens distortion correction (mi_isp_lens) ------------------------------------------------------------
static int check_remap_shape(int H, int W, int Hd, int Wd, int in_dtype, int out_dtype, const char* who) {
  MI_REQUIRE(H > 0 && W > 0 && Hd >= 0 && Wd >= 0, "%s: bad lens shape %dx%d -> %dx%d", who, H, W, Hd, Wd);
  MI_REQUIRE(H < (1 << 24) && W < (1 << 24), "%s: lens source %dx%d too large", who, H, W);
  MI_REQUIRE((int64_t)Hd * Wd < ((int64_t)1 << 31) / 3, "%s: lens output %dx%d too large", who, Hd, Wd);
  MI_REQUIRE(mi_valid_dtype(in_dtype) && mi_valid_dtype(out_dtype), "%s: bad lens dtype %d -> %d", who, in_dtype,
             out_dtype);
  return 0;
}

// the f32 model of a lens (every value rounded once from double; 1 / fx', 1 / fy' in double, then rounded)
static int lens_model(const mi_isp_lens* l, lens::Model& m, const char* who) {
  MI_REQUIRE(l, "%s: null lens", who);
  MI_REQUIRE(l->n_dist == 4 || l->n_dist == 5 || l->n_dist == 8, "%s: lens takes 4, 5 or 8 distortion coefficients, "
             "got %d", who, (int)l->n_dist);
  MI_REQUIRE(l->border == MI_BORDER_CONSTANT || l->border == MI_BORDER_REPLICATE, "%s: bad lens border %d", who,
             (int)l->border);
  const double k[8] = {l->fx, l->fy, l->cx, l->cy, l->new_fx, l->new_fy, l->new_cx, l->new_cy};
  for (double v : k) MI_REQUIRE(std::isfinite(v) && std::isfinite((float)v), "%s: lens camera matrix value %g is not finite", who, v);
  for (int i = 0; i < l->n_dist; ++i)
    MI_REQUIRE(std::isfinite(l->dist[i]) && std::isfinite((float)l->dist[i]), "%s: lens coefficient %d (%g) is not finite", who, i,
               l->dist[i]);
  MI_REQUIRE(l->fx > 0 && l->fy > 0 && l->new_fx > 0 && l->new_fy > 0 && (float)l->fx > 0.f && (float)l->fy > 0.f,
             "%s: lens focal lengths must be positive (fx %g, fy %g, fx' %g, fy' %g)", who, l->fx, l->fy, l->new_fx,
             l->new_fy);
  const double ifx = 1.0 / l->new_fx, ify = 1.0 / l->new_fy;
  MI_REQUIRE(std::isfinite((float)ifx) && std::isfinite((float)ify), "%s: lens focal length too small", who);
  m = {};
  m.fx = (float)l->fx; m.fy = (float)l->fy; m.cx = (float)l->cx; m.cy = (float)l->cy;
  m.ncx = (float)l->new_cx; m.ncy = (float)l->new_cy; m.ifx = (float)ifx; m.ify = (float)ify;
  m.k1 = (float)l->dist[0]; m.k2 = (float)l->dist[1]; m.p1 = (float)l->dist[2]; m.p2 = (float)l->dist[3];
  m.k3 = l->n_dist >= 5 ? (float)l->dist[4] : 0.f;
  m.rational = l->n_dist == 8;
  if (m.rational) { m.k4 = (float)l->dist[5]; m.k5 = (float)l->dist[6]; m.k6 = (float)l->dist[7]; }
  return 0;
}

static int undistort_impl(const void* const* src, void* const* dst, int n, int H, int W, int Hd, int Wd, float s0,
                          float s1, int in_dtype, int out_dtype, const mi_isp_lens* const* lenses, void* stream,
                          const char* who) {
  MI_REQUIRE(n >= 0, "%s: negative lens frame count %d", who, n);
  if (n == 0) return 0;
  MI_REQUIRE(src && dst && lenses, "%s: null lens argument", who);
  if (int rc = check_remap_shape(H, W, Hd, Wd, in_dtype, out_dtype, who)) return rc;
  MI_REQUIRE(s0 > 0.f && s1 > 0.f && std::isfinite(s0) && std::isfinite(s1), "%s: lens output scale (%g, %g) must be positive", who,
             s0, s1);
  lens::Args a[2] = {};                                    // per border mode
  for (int b = 0; b < 2; ++b) {
    a[b].H = H; a[b].W = W; a[b].Hd = Hd; a[b].Wd = Wd; a[b].s0 = s0; a[b].s1 = s1;
    a[b].intensity = (float)((double)mi_scale_factor(out_dtype) / (double)mi_scale_factor(in_dtype));
  }
  for (int i = 0; i < n; ++i) {                            // every check before the first launch
    MI_REQUIRE(src[i] && dst[i], "%s: lens frame %d has a null buffer", who, i);
    lens::Model m;
    if (int rc = lens_model(lenses[i], m, who)) return rc;
  }
  if ((int64_t)Hd * Wd == 0) return 0;
  for (int i = 0; i < n; ++i) {
    lens::Args& g = a[lenses[i]->border];
    lens::Cam& c = g.cam[g.n_cams++];
    c.src = src[i]; c.dst = dst[i]; c.table = nullptr;
    lens_model(lenses[i], c.m, who);
    for (int b = 0; b < 2; ++b)
      if (a[b].n_cams == lens::MAX_CAMS || (i == n - 1 && a[b].n_cams > 0)) {
        if (int rc = lens::launch(a[b], in_dtype, out_dtype, false, b, (hipStream_t)stream)) return rc;
        a[b].n_cams = 0;
      }
  }
  return 0;
}

extern "C" int mi_isp_undistort(const void* src, void* dst, int H, int W, int Hd, int Wd, float s0, float s1, int in_dtype,
                                int out_dtype, const mi_isp_lens* lens, void* stream) {
  MI_REQUIRE(lens, "undistort: null lens");
  return undistort_impl(&src, &dst, 1, H, W, Hd, Wd, s0, s1, in_dtype, out_dtype, &lens, stream, "undistort");
}

extern "C" int mi_isp_undistort_batch(const void* const* src, void* const* dst, int n, int H, int W, int Hd, int Wd,
                                      float s0, float s1, int in_dtype, int out_dtype, const mi_isp_lens* const* lenses,
                                      void* stream) {
  return undistort_impl(src, dst, n, H, W, Hd, Wd, s0, s1, in_dtype, out_dtype, lenses, stream, "undistort_batch");
}

extern "C" int mi_isp_remap(const void* src, void* dst, const float* map, int H, int W, int Hd, int Wd, int in_dtype,
                            int out_dtype, int border, void* stream) {
  MI_REQUIRE(src && dst && map, "remap: null lens argument");
  if (int rc = check_remap_shape(H, W, Hd, Wd, in_dtype, out_dtype, "remap")) return rc;
  MI_REQUIRE(border == MI_BORDER_CONSTANT || border == MI_BORDER_REPLICATE, "remap: bad lens border %d", border);
  MI_REQUIRE(mi_aligned(map, 8), "remap: the lens table must be 8-byte aligned");
  lens::Args a = {};
  a.H = H; a.W = W; a.Hd = Hd; a.Wd = Wd; a.s0 = 1.f; a.s1 = 1.f;
  a.intensity = (float)((double)mi_scale_factor(out_dtype) / (double)mi_scale_factor(in_dtype));
  a.n_cams = 1;
  a.cam[0].src = src; a.cam[0].dst = dst; a.cam[0].table = map;
  return lens::launch(a, in_dtype, out_dtype, true, border, (hipStream_t)stream);
}

// ---- automatic white balance (isp_awb.h; DESIGN.md 3, "Auto white balance") ---------------------------------------
static int awb_filter(awb::Stats& s, int H, int W, float clip, float floor_, int stride, void* pending, const char* who) {
  MI_REQUIRE(pending, "%s: null awb pending buffer", who);
  MI_REQUIRE(H >= 0 && W >= 0, "%s: bad shape %dx%d", who, H, W);
  MI_REQUIRE(stride >= 1, "%s: awb stride %d < 1", who, stride);
  MI_REQUIRE(std::isfinite(clip) && std::isfinite(floor_) && 0.f < floor_ && floor_ < clip,
             "%s: awb needs 0 < floor < clip, both finite (floor %g, clip %g)", who, (double)floor_, (double)clip);
  s.H = H; s.W = W; s.stride = stride; s.clip = clip; s.floor = floor_;
  s.pending = static_cast<unsigned long long*>(pending);
  return 0;
}

extern "C" int mi_isp_awb_stats_packed(const uint8_t* const* packed, int n, int H, int W, int bits, int ids_format,
                                       const mi_isp_levels* lv, const mi_isp_shading* sh, float clip, float floor_,
                                       int stride, void* pending, void* stream) {
  const char* who = "awb_stats_packed";
  MI_REQUIRE(packed || n == 0, "%s: null frame list", who);
  MI_REQUIRE(n >= 0, "%s: negative frame count", who);
  for (int i = 0; i < n; ++i) MI_REQUIRE(packed[i], "%s: frame %d is null", who, i);
  MI_REQUIRE(bits == 12 || bits == 16, "%s: bits must be 12 or 16, got %d", who, bits);
  MI_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: image must be even size, got %dx%d", who, H, W);
  awb::PackedArgs a = {};
  if (int rc = awb_filter(a.s, H, W, clip, floor_, stride, pending, who)) return rc;
  tile::Params p = {};
  p.k_decode = (float)(1.0 / (bits == 16 ? 65535.0 : 4095.0));
  if (int rc = apply_levels(p, lv, bits, who)) return rc;
  for (int s = 0; s < 4; ++s) {                       // the per-site decode of the shading path (apply_levels_shading)
    a.s.black[s] = p.levels ? p.lv_black[s] : 0;
    a.s.k[s] = p.levels ? p.lv_k[s] : p.k_decode;
  }
  if (int rc = apply_shading(a.s, sh, H, W, who)) return rc;
  a.bits = bits; a.ids = bits == 12 && ids_format;
  for (int i0 = 0; i0 < n; i0 += awb::MAX_FRAMES) {
    a.n_frames = n - i0 < awb::MAX_FRAMES ? n - i0 : awb::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i) a.src[i] = packed[i0 + i];
    if (int rc = awb::launch_packed(a, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_awb_stats_cfa(const void* cfa, int H, int W, int mode, const mi_isp_levels* lv,
                                    const mi_isp_shading* sh, float clip, float floor_, int stride, void* pending,
                                    void* stream) {
  const char* who = "awb_stats_cfa";
  MI_REQUIRE(cfa, "%s: null CFA", who);
  MI_REQUIRE(mode >= MI_LOAD_16U && mode <= MI_LOAD_16F, "%s: bad mode %d", who, mode);
  awb::Stats s = {};
  if (int rc = awb_filter(s, H, W, clip, floor_, stride, pending, who)) return rc;
  if (lv) {                                           // mi_isp_load_convert_shading's levels: k[] holds the denominators
    MI_REQUIRE(mode == MI_LOAD_16U, "%s: levels apply to u16 codes only (mode %d)", who, mode);
    if (int rc = mi_check_levels(lv, 65535, who, s.black)) return rc;
    for (int k = 0; k < 4; ++k) s.k[k] = (float)(lv->white - lv->black[k]);
    s.has_levels = 1;
  }
  if (int rc = apply_shading(s, sh, H, W, who)) return rc;
  return awb::launch_cfa(s, cfa, mode, (hipStream_t)stream);
}

// the colour (0 R, 1 G, 2 B) of each CFA site under a demosaic pattern, and the user grid of E
static int awb_grid(awb::Update& u, int pattern, const mi_isp_shading* user, float* effective, const char* who) {
  static const int colours[4][4] = {{0, 1, 1, 2}, {1, 0, 2, 1}, {1, 2, 0, 1}, {2, 1, 1, 0}};   // RGGB GRBG GBRG BGGR
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: bad pattern %d", who, pattern);
  MI_REQUIRE(effective, "%s: null awb effective grid", who);
  for (int s = 0; s < 4; ++s) u.site_colour[s] = colours[pattern][s];
  u.effective = effective;
  if (!user) { u.user = nullptr; u.user_sites = 1; u.gh = 2; u.gw = 2; return 0; }
  tile::Params p = {};
  if (int rc = apply_shading(p, user, 2, 2, who)) return rc;
  u.user = user->gains_dev; u.user_sites = user->sites; u.gh = user->grid_h; u.gw = user->grid_w;
  return 0;
}

extern "C" int mi_isp_awb_update(const int64_t* gathered, int world, void* pending, int pattern, double t, double* state,
                                 float* gains, const mi_isp_shading* user, float* effective, void* stream) {
  const char* who = "awb_update";
  MI_REQUIRE(gathered && pending && state && gains, "%s: null awb buffer", who);
  MI_REQUIRE(world >= 1, "%s: awb world %d < 1", who, world);
  MI_REQUIRE(std::isfinite(t), "%s: awb t must be finite", who);
  awb::Update u = {};
  if (int rc = awb_grid(u, pattern, user, effective, who)) return rc;
  u.gathered = reinterpret_cast<const long long*>(gathered); u.world = world;
  u.pending = static_cast<unsigned long long*>(pending);
  u.t = t; u.state = state; u.gains = gains;
  return awb::launch_update(u, (hipStream_t)stream);
}

extern "C" int mi_isp_awb_rebuild(int pattern, float* gains, const mi_isp_shading* user, float* effective, void* stream) {
  const char* who = "awb_rebuild";
  MI_REQUIRE(gains, "%s: null awb gains", who);
  awb::Update u = {};
  if (int rc = awb_grid(u, pattern, user, effective, who)) return rc;
  u.gains = gains;
  return awb::launch_update(u, (hipStream_t)stream);
}

// ---- the raw stages' shared source (isp_raw_source.h) ----------------------------------------------------------------
// How a stage words the errors of the shared checks, "<who>: <prefix><text>": its noun, the prefix (raw noise reduction has
// none) and what its frame lists count.  The texts are the entry points' behaviour: tests/test_raw_stage_errors_cpu.py.
struct RawStage { const char* noun; const char* prefix; const char* item; };
static const RawStage kDenoise = {"denoise", "", "frame"}, kHighlights = {"highlights", "highlights: ", "frame"},
                      kChromatic = {"chromatic aberration", "chromatic aberration: ", "frame"},
                      kTemporal = {"temporal", "temporal: ", "frame"}, kMerge = {"exposure merge", "exposure merge: ", "bracket"};

static int raw_geometry(int H, int W, int work_dtype, const RawStage& st, const char* who) {
  MI_REQUIRE(H >= 0 && W >= 0, "%s: bad %s shape %dx%d", who, st.noun, H, W);
  MI_REQUIRE(H < (1 << 22) && W < (1 << 24), "%s: %s frame %dx%d too large", who, st.noun, H, W);
  MI_REQUIRE(work_dtype == MI_F16 || work_dtype == MI_F32, "%s: %s work dtype must be f16 or f32", who, st.noun);
  return 0;
}

static int raw_kind(int kind, const RawStage& st, const char* who) {
  MI_REQUIRE(kind >= MI_RAW_PACKED12 && kind <= MI_RAW_16F, "%s: bad %s source kind %d", who, st.noun, kind);
  return 0;
}

// the rules that need no levels: the plain f32 output takes no grid, packed frames are even, IDS is a packed-12 layout
static int raw_source_rules(int H, int W, int kind, int ids_format, const mi_isp_shading* shading, int plain,
                            const RawStage& st, const char* who) {
  const bool packed = kind == MI_RAW_PACKED12 || kind == MI_RAW_PACKED16;
  MI_REQUIRE(!plain || !shading, "%s: %sthe plain f32 output takes no shading grid", who, st.prefix);
  MI_REQUIRE(!packed || (H % 2 == 0 && W % 2 == 0), "%s: %spacked frames must be even size, got %dx%d", who, st.prefix, H, W);
  MI_REQUIRE(!ids_format || kind == MI_RAW_PACKED12, "%s: %sthe IDS layout is a packed-12 layout", who, st.prefix);
  return 0;
}

// fills a (the shape, the decode of `kind` under the levels, the grid, mask_w) and src_kind, and checks the n defect maps
static int raw_source_setup(raw::Source& a, int& src_kind, int H, int W, int kind, int ids_format,
                            const mi_isp_levels* levels, const mi_isp_shading* shading,
                            const mi_isp_defects* const* defects, int n, const RawStage& st, const char* who) {
  a.H = H; a.W = W;
  if (kind == MI_RAW_PACKED12 || kind == MI_RAW_PACKED16) {
    tile::Params p = {};
    const int bits = kind == MI_RAW_PACKED12 ? 12 : 16;
    p.k_decode = (float)(1.0 / (bits == 16 ? 65535.0 : 4095.0));
    if (int rc = apply_levels(p, levels, bits, who)) return rc;
    for (int s = 0; s < 4; ++s) {                     // the per-site decode of the shading path (apply_levels_shading)
      a.black[s] = p.levels ? p.lv_black[s] : 0;
      a.k[s] = p.levels ? p.lv_k[s] : p.k_decode;
    }
    src_kind = bits == 16 ? raw::SRC_P16 : (ids_format ? raw::SRC_P12_IDS : raw::SRC_P12);
  } else {
    if (levels) {                                     // load_u16_levels_kernel's levels: k[] holds the denominators
      MI_REQUIRE(kind == MI_RAW_16U, "%s: %slevels apply to u16 codes only (source kind %d)", who, st.prefix, kind);
      if (int rc = mi_check_levels(levels, 65535, who, a.black)) return rc;
      for (int s = 0; s < 4; ++s) a.k[s] = (float)(levels->white - levels->black[s]);
      a.levels = 1;
    }
    src_kind = kind == MI_RAW_16U ? raw::SRC_U16 : (kind == MI_RAW_32F ? raw::SRC_F32 : raw::SRC_U16F);
  }
  if (int rc = apply_shading(a, shading, H, W, who)) return rc;
  a.mask_w = (W + 31) / 32;
  for (int i = 0; i < n; ++i)
    if (defects && defects[i]) {
      MI_REQUIRE(defects[i]->n >= 0, "%s: %snegative defect count %d", who, st.prefix, (int)defects[i]->n);
      MI_REQUIRE(defects[i]->n == 0 || defects[i]->mask_dev, "%s: %s%s %d: defects without a mask", who, st.prefix, st.item,
                 i);
    }
  return 0;
}

// the mask a kernel reads for frame i: a map with no listed pixel needs none
static const uint32_t* mask_of(const mi_isp_defects* const* defects, int i) {
  const mi_isp_defects* m = defects ? defects[i] : nullptr;
  return (m && m->n > 0) ? m->mask_dev : nullptr;
}

// ---- raw noise reduction (isp_denoise.h; DESIGN.md 3, "Raw noise reduction") ----------------------------------------
// the filter's settings, checked on the host; fills the filter members of a
static int denoise_settings(dn::Args& a, const mi_isp_denoise* d, const char* who) {
  MI_REQUIRE(d, "%s: null denoise settings", who);
  MI_REQUIRE(d->radius == 1 || d->radius == 2, "%s: denoise radius %d (1 or 2)", who, (int)d->radius);
  MI_REQUIRE(std::isfinite(d->gain) && d->gain >= 0.f, "%s: denoise gain %g must be finite and >= 0", who,
             (double)d->gain);
  MI_REQUIRE(std::isfinite(d->read_noise) && d->read_noise > 0.f, "%s: denoise read_noise %g must be finite and > 0",
             who, (double)d->read_noise);
  MI_REQUIRE(std::isfinite(d->strength) && d->strength > 0.f, "%s: denoise strength %g must be finite and > 0", who,
             (double)d->strength);
  MI_REQUIRE(std::isfinite(d->spatial_sigma) && d->spatial_sigma > 0.f,
             "%s: denoise spatial_sigma %g must be finite and > 0", who, (double)d->spatial_sigma);
  const double log2e = 1.4426950408889634, rn = d->read_noise, st = d->strength, sg = d->spatial_sigma;
  a.gain = d->gain;
  a.rn2 = (float)(rn * rn);
  a.c2 = (float)(log2e / (2.0 * st * st));
  for (int k = 0; k < 9; ++k) a.sp[k] = (float)((double)k * log2e / (2.0 * sg * sg));
  return 0;
}

// n raw frames of one geometry: every frame's pointers (and defect mask) in the kernel arguments, 32 per launch
static int denoise_raw_impl(const void* const* src, void* const* cfa, int n, int H, int W, int kind, int ids_format,
                            int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                            const mi_isp_defects* const* defects, const mi_isp_denoise* d, void* stream, const char* who) {
  dn::Args a = {};
  if (int rc = denoise_settings(a, d, who)) return rc;
  if (int rc = raw_geometry(H, W, work_dtype, kDenoise, who)) return rc;
  if (int rc = raw_kind(kind, kDenoise, who)) return rc;
  MI_REQUIRE(n >= 0 && (src || n == 0) && (cfa || n == 0), "%s: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && cfa[i], "%s: frame %d has a null pointer", who, i);
    MI_REQUIRE(src[i] != cfa[i], "%s: frame %d: the CFA must not overwrite its source", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, 0, kDenoise, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kDenoise, who))
    return rc;
  for (int i0 = 0; i0 < n; i0 += dn::MAX_FRAMES) {
    a.n_frames = n - i0 < dn::MAX_FRAMES ? n - i0 : dn::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i) a.f[i] = {src[i0 + i], cfa[i0 + i], mask_of(defects, i0 + i)};
    if (int rc = dn::launch(a, src_kind, work_dtype, d->radius, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_denoise_raw(const void* src, void* cfa, int H, int W, int kind, int ids_format, int work_dtype,
                                  const mi_isp_levels* levels, const mi_isp_shading* shading,
                                  const mi_isp_defects* defects, const mi_isp_denoise* denoise, void* stream) {
  MI_REQUIRE(src && cfa, "denoise_raw: null pointer");
  return denoise_raw_impl(&src, &cfa, 1, H, W, kind, ids_format, work_dtype, levels, shading, &defects, denoise, stream,
                          "denoise_raw");
}

extern "C" int mi_isp_denoise_raw_batch(const void* const* src, void* const* cfa, int n, int H, int W, int kind,
                                        int ids_format, int work_dtype, const mi_isp_levels* levels,
                                        const mi_isp_shading* shading, const mi_isp_defects* const* defects,
                                        const mi_isp_denoise* denoise, void* stream) {
  return denoise_raw_impl(src, cfa, n, H, W, kind, ids_format, work_dtype, levels, shading, defects, denoise, stream,
                          "denoise_raw_batch");
}

extern "C" int mi_isp_denoise_cfa(const void* in, void* out, int H, int W, int dtype, const mi_isp_denoise* denoise,
                                  void* stream) {
  const char* who = "denoise_cfa";
  dn::Args a = {};
  if (int rc = denoise_settings(a, denoise, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kDenoise, who)) return rc;
  MI_REQUIRE(in && out, "%s: null pointer", who);
  MI_REQUIRE(in != out, "%s: the output must not overwrite the input", who);
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {in, out, nullptr};
  return dn::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype, denoise->radius, (hipStream_t)stream);
}

// ---- highlight reconstruction (isp_highlights.h; DESIGN.md 3, "Highlight reconstruction") ----------------------------
// the operator's settings and the demosaic pattern, checked on the host; fills the operator members of a
static int highlights_settings(hl::Args& a, const mi_isp_highlights* h, int pattern, const char* who) {
  static const int colours[4][4] = {{0, 1, 1, 2}, {1, 0, 2, 1}, {1, 2, 0, 1}, {2, 1, 1, 0}};   // RGGB GRBG GBRG BGGR
  MI_REQUIRE(h, "%s: null highlights settings", who);
  MI_REQUIRE(h->mode == MI_HIGHLIGHTS_REBUILD || h->mode == MI_HIGHLIGHTS_CLIP, "%s: highlights mode %d (0 rebuild, 1 clip)",
             who, (int)h->mode);
  MI_REQUIRE(std::isfinite(h->clip) && h->clip > 0.f, "%s: highlights clip %g must be finite and > 0", who,
             (double)h->clip);
  if (!h->wb_dev)
    for (int k = 0; k < 3; ++k)
      MI_REQUIRE(std::isfinite(h->wb[k]) && h->wb[k] > 0.f, "%s: highlights balance gain %d (%g) must be finite and > 0",
                 who, k, (double)h->wb[k]);
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: bad highlights pattern %d", who, pattern);
  a.mode = h->mode == MI_HIGHLIGHTS_CLIP ? hl::MODE_CLIP : hl::MODE_REBUILD;
  a.t = h->clip;
  for (int k = 0; k < 3; ++k) a.wb[k] = h->wb_dev ? 1.f : h->wb[k];
  a.wb_dev = h->wb_dev;
  for (int s = 0; s < 4; ++s) a.colour[s] = colours[pattern][s];
  return 0;
}

// n raw frames of one geometry: every frame's pointers (and defect mask) in the kernel arguments, 32 per launch
static int highlights_raw_impl(const void* const* src, void* const* cfa, int n, int H, int W, int kind, int ids_format,
                               int work_dtype, int pattern, const mi_isp_levels* levels, const mi_isp_shading* shading,
                               const mi_isp_defects* const* defects, const mi_isp_highlights* h, int plain, void* stream,
                               const char* who) {
  hl::Args a = {};
  if (int rc = highlights_settings(a, h, pattern, who)) return rc;
  if (int rc = raw_geometry(H, W, work_dtype, kHighlights, who)) return rc;
  if (int rc = raw_kind(kind, kHighlights, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: highlights with %d frames", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  MI_REQUIRE(src && cfa, "%s: highlights: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && cfa[i], "%s: highlights: frame %d has a null pointer", who, i);
    MI_REQUIRE(src[i] != cfa[i], "%s: highlights: frame %d: the CFA must not overwrite its source", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, plain, kHighlights, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kHighlights, who))
    return rc;
  const int out = plain ? hl::OUT_PLAIN : (work_dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32);
  for (int i0 = 0; i0 < n; i0 += hl::MAX_FRAMES) {
    a.n_frames = n - i0 < hl::MAX_FRAMES ? n - i0 : hl::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i) a.f[i] = {src[i0 + i], cfa[i0 + i], mask_of(defects, i0 + i)};
    if (int rc = hl::launch(a, src_kind, out, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_highlights_raw(const void* src, void* cfa, int H, int W, int kind, int ids_format, int work_dtype,
                                     int pattern, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                     const mi_isp_defects* defects, const mi_isp_highlights* highlights, int out_f32_plain,
                                     void* stream) {
  return highlights_raw_impl(&src, &cfa, 1, H, W, kind, ids_format, work_dtype, pattern, levels, shading, &defects,
                             highlights, out_f32_plain, stream, "highlights_raw");
}

extern "C" int mi_isp_highlights_raw_batch(const void* const* src, void* const* cfa, int n, int H, int W, int kind,
                                           int ids_format, int work_dtype, int pattern, const mi_isp_levels* levels,
                                           const mi_isp_shading* shading, const mi_isp_defects* const* defects,
                                           const mi_isp_highlights* highlights, int out_f32_plain, void* stream) {
  return highlights_raw_impl(src, cfa, n, H, W, kind, ids_format, work_dtype, pattern, levels, shading, defects, highlights,
                             out_f32_plain, stream, "highlights_raw_batch");
}

extern "C" int mi_isp_highlights_cfa(const void* in, void* out, int H, int W, int dtype, int pattern,
                                     const mi_isp_highlights* highlights, void* stream) {
  const char* who = "highlights_cfa";
  hl::Args a = {};
  if (int rc = highlights_settings(a, highlights, pattern, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kHighlights, who)) return rc;
  if (H == 0 || W == 0) return 0;
  MI_REQUIRE(in && out, "%s: highlights: null pointer", who);
  MI_REQUIRE(in != out, "%s: highlights: the output must not overwrite the input", who);
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {in, out, nullptr};
  return hl::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32,
                    (hipStream_t)stream);
}

// ---- dynamic defects (isp_dynamic_defects.h; DESIGN.md 3, "Dynamic defects") -----------------------------------------
static const RawStage kDynamicDefects = {"dynamic defects", "dynamic defects: ", "frame"};

// the operator's settings, checked on the host; fills the operator members of a
static int dynamic_defects_settings(ddp::Args& a, const mi_isp_dynamic_defects* d, const char* who) {
  MI_REQUIRE(d, "%s: null dynamic defects settings", who);
  MI_REQUIRE(std::isfinite(d->threshold) && d->threshold > 0.f, "%s: dynamic defects threshold %g must be finite and > 0",
             who, (double)d->threshold);
  MI_REQUIRE(std::isfinite(d->slope) && d->slope >= 0.f, "%s: dynamic defects slope %g must be finite and >= 0", who,
             (double)d->slope);
  MI_REQUIRE(d->tolerate == 0 || d->tolerate == 1, "%s: dynamic defects tolerate %d (0 or 1)", who, (int)d->tolerate);
  MI_REQUIRE(d->hot || d->dead, "%s: dynamic defects with neither hot nor dead pixels to look for", who);
  a.t = d->threshold;
  a.s = d->slope;
  a.tolerate = d->tolerate;
  a.hot = d->hot != 0;
  a.dead = d->dead != 0;
  return 0;
}

// n raw frames of one geometry: every frame's pointers (defect mask and flag plane) in the kernel arguments, 32 per launch
static int dynamic_defects_raw_impl(const void* const* src, void* const* cfa, int n, int H, int W, int kind, int ids_format,
                                    int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                    const mi_isp_defects* const* defects, const mi_isp_dynamic_defects* d, int plain,
                                    uint32_t* const* flags, void* stream, const char* who) {
  ddp::Args a = {};
  if (int rc = dynamic_defects_settings(a, d, who)) return rc;
  if (int rc = raw_geometry(H, W, work_dtype, kDynamicDefects, who)) return rc;
  if (int rc = raw_kind(kind, kDynamicDefects, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: dynamic defects with %d frames", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  MI_REQUIRE(src && cfa, "%s: dynamic defects: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && cfa[i], "%s: dynamic defects: frame %d has a null pointer", who, i);
    MI_REQUIRE(src[i] != cfa[i], "%s: dynamic defects: frame %d: the CFA must not overwrite its source", who, i);
    MI_REQUIRE(!flags || (flags[i] != src[i] && flags[i] != cfa[i]),
               "%s: dynamic defects: frame %d: the flags must not overwrite the source or the CFA", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, plain, kDynamicDefects, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kDynamicDefects, who))
    return rc;
  const int out = plain ? hl::OUT_PLAIN : (work_dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32);
  for (int i0 = 0; i0 < n; i0 += ddp::MAX_FRAMES) {
    a.n_frames = n - i0 < ddp::MAX_FRAMES ? n - i0 : ddp::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i)
      a.f[i] = {src[i0 + i], cfa[i0 + i], mask_of(defects, i0 + i), flags ? flags[i0 + i] : nullptr};
    if (int rc = ddp::launch(a, src_kind, out, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_dynamic_defects_raw(const void* src, void* cfa, int H, int W, int kind, int ids_format,
                                          int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                          const mi_isp_defects* defects, const mi_isp_dynamic_defects* dynamic,
                                          int out_f32_plain, void* stream, uint32_t* flags) {
  return dynamic_defects_raw_impl(&src, &cfa, 1, H, W, kind, ids_format, work_dtype, levels, shading, &defects, dynamic,
                                  out_f32_plain, flags ? &flags : nullptr, stream, "dynamic_defects_raw");
}

extern "C" int mi_isp_dynamic_defects_raw_batch(const void* const* src, void* const* cfa, int n, int H, int W, int kind,
                                                int ids_format, int work_dtype, const mi_isp_levels* levels,
                                                const mi_isp_shading* shading, const mi_isp_defects* const* defects,
                                                const mi_isp_dynamic_defects* dynamic, int out_f32_plain, void* stream,
                                                uint32_t* const* flags) {
  return dynamic_defects_raw_impl(src, cfa, n, H, W, kind, ids_format, work_dtype, levels, shading, defects, dynamic,
                                  out_f32_plain, flags, stream, "dynamic_defects_raw_batch");
}

extern "C" int mi_isp_dynamic_defects_cfa(const void* in, void* out, int H, int W, int dtype,
                                          const mi_isp_dynamic_defects* dynamic, void* stream, uint32_t* flags) {
  const char* who = "dynamic_defects_cfa";
  ddp::Args a = {};
  if (int rc = dynamic_defects_settings(a, dynamic, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kDynamicDefects, who)) return rc;
  if (H == 0 || W == 0) return 0;
  MI_REQUIRE(in && out, "%s: dynamic defects: null pointer", who);
  MI_REQUIRE(in != out, "%s: dynamic defects: the output must not overwrite the input", who);
  MI_REQUIRE(!flags || ((const void*)flags != in && (void*)flags != out),
             "%s: dynamic defects: the flags must not overwrite the input or the output", who);
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {in, out, nullptr, flags};
  return ddp::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32,
                     (hipStream_t)stream);
}

// ---- green equalisation (isp_green_equalize.h; DESIGN.md 3, "Green equalisation") ------------------------------------
static const RawStage kGreenEqualize = {"green equalize", "green equalize: ", "frame"};

// the operator's settings and the demosaic pattern, checked on the host; fills the operator members of a
static int green_equalize_settings(geq::Args& a, const mi_isp_green_equalize* g, int pattern, const char* who) {
  static const int colours[4][4] = {{0, 1, 1, 2}, {1, 0, 2, 1}, {1, 2, 0, 1}, {2, 1, 1, 0}};   // RGGB GRBG GBRG BGGR
  MI_REQUIRE(g, "%s: null green equalize settings", who);
  MI_REQUIRE(std::isfinite(g->threshold) && g->threshold >= 0.f, "%s: green equalize threshold %g must be finite and >= 0",
             who, (double)g->threshold);
  MI_REQUIRE(std::isfinite(g->slope) && g->slope >= 0.f, "%s: green equalize slope %g must be finite and >= 0", who,
             (double)g->slope);
  MI_REQUIRE(g->strength >= 0.f && g->strength <= 1.f, "%s: green equalize strength %g must be in [0, 1]", who,
             (double)g->strength);
  MI_REQUIRE(g->radius == 1 || g->radius == 2, "%s: green equalize radius %d (1 or 2)", who, (int)g->radius);
  MI_REQUIRE(std::isfinite(g->edge) && g->edge >= 0.f, "%s: green equalize edge %g must be finite and >= 0", who,
             (double)g->edge);
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: bad green equalize pattern %d", who, pattern);
  a.t = g->threshold;
  a.s = g->slope;
  a.edge = g->edge;
  a.hs = g->strength * 0.5f;
  a.gp = colours[pattern][0] == 1 ? 0 : 1;            // (r, c) is green iff ((r + c) & 1) == gp: site (0, 0) tells
  return 0;
}

// n raw frames of one geometry: every frame's pointers (and defect mask) in the kernel arguments, 32 per launch
static int green_equalize_raw_impl(const void* const* src, void* const* cfa, int n, int H, int W, int kind, int ids_format,
                                   int work_dtype, int pattern, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                   const mi_isp_defects* const* defects, const mi_isp_green_equalize* g, int plain,
                                   void* stream, const char* who) {
  geq::Args a = {};
  if (int rc = green_equalize_settings(a, g, pattern, who)) return rc;
  if (int rc = raw_geometry(H, W, work_dtype, kGreenEqualize, who)) return rc;
  if (int rc = raw_kind(kind, kGreenEqualize, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: green equalize with %d frames", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  MI_REQUIRE(src && cfa, "%s: green equalize: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && cfa[i], "%s: green equalize: frame %d has a null pointer", who, i);
    MI_REQUIRE(src[i] != cfa[i], "%s: green equalize: frame %d: the CFA must not overwrite its source", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, plain, kGreenEqualize, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kGreenEqualize, who))
    return rc;
  const int out = plain ? hl::OUT_PLAIN : (work_dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32);
  for (int i0 = 0; i0 < n; i0 += geq::MAX_FRAMES) {
    a.n_frames = n - i0 < geq::MAX_FRAMES ? n - i0 : geq::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i) a.f[i] = {src[i0 + i], cfa[i0 + i], mask_of(defects, i0 + i)};
    if (int rc = geq::launch(a, src_kind, out, g->radius, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_green_equalize_raw(const void* src, void* cfa, int H, int W, int kind, int ids_format,
                                         int work_dtype, int pattern, const mi_isp_levels* levels,
                                         const mi_isp_shading* shading, const mi_isp_defects* defects,
                                         const mi_isp_green_equalize* green, int out_f32_plain, void* stream) {
  return green_equalize_raw_impl(&src, &cfa, 1, H, W, kind, ids_format, work_dtype, pattern, levels, shading, &defects,
                                 green, out_f32_plain, stream, "green_equalize_raw");
}

extern "C" int mi_isp_green_equalize_raw_batch(const void* const* src, void* const* cfa, int n, int H, int W, int kind,
                                               int ids_format, int work_dtype, int pattern, const mi_isp_levels* levels,
                                               const mi_isp_shading* shading, const mi_isp_defects* const* defects,
                                               const mi_isp_green_equalize* green, int out_f32_plain, void* stream) {
  return green_equalize_raw_impl(src, cfa, n, H, W, kind, ids_format, work_dtype, pattern, levels, shading, defects, green,
                                 out_f32_plain, stream, "green_equalize_raw_batch");
}

extern "C" int mi_isp_green_equalize_cfa(const void* in, void* out, int H, int W, int dtype, int pattern,
                                         const mi_isp_green_equalize* green, void* stream) {
  const char* who = "green_equalize_cfa";
  geq::Args a = {};
  if (int rc = green_equalize_settings(a, green, pattern, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kGreenEqualize, who)) return rc;
  if (H == 0 || W == 0) return 0;
  MI_REQUIRE(in && out, "%s: green equalize: null pointer", who);
  MI_REQUIRE(in != out, "%s: green equalize: the output must not overwrite the input", who);
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {in, out, nullptr};
  return geq::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32,
                     green->radius, (hipStream_t)stream);
}

// ---- frame statistics (isp_statistics.h; DESIGN.md 3, "Frame statistics") --------------------------------------------
static const RawStage kStatistics = {"statistics", "statistics: ", "frame"};

// the settings and the demosaic pattern, checked on the host; fills the members of a that need no shape
static int statistics_settings(st::Args& a, const mi_isp_statistics* s, int pattern, const char* who) {
  static const int first_colour[4] = {0, 1, 1, 2};   // of site (0, 0): RGGB GRBG GBRG BGGR
  MI_REQUIRE(s, "%s: null statistics settings", who);
  MI_REQUIRE(s->zones_h >= 1 && s->zones_h <= st::MAX_ZONES && s->zones_w >= 1 && s->zones_w <= st::MAX_ZONES,
             "%s: statistics zones %dx%d outside 1 .. %d", who, (int)s->zones_h, (int)s->zones_w, st::MAX_ZONES);
  MI_REQUIRE(std::isfinite(s->clip) && s->clip > 0.f, "%s: statistics clip %g must be finite and > 0", who, (double)s->clip);
  MI_REQUIRE(std::isfinite(s->dark) && s->dark >= 0.f && s->dark < s->clip,
             "%s: statistics dark %g must be finite, >= 0 and below clip %g", who, (double)s->dark, (double)s->clip);
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: bad statistics pattern %d", who, pattern);
  a.gh = s->zones_h; a.gw = s->zones_w;
  a.clip = s->clip; a.dark = s->dark;
  a.gp = first_colour[pattern] == 1 ? 0 : 1;          // (r, c) is green iff ((r + c) & 1) == gp: site (0, 0) tells
  return 0;
}

// the shape rules of a frame with pixels: even, at most 2^26 pixels, no zone empty
static int statistics_shape(const st::Args& a, int H, int W, const char* who) {
  MI_REQUIRE(H % 2 == 0 && W % 2 == 0, "%s: statistics: frames must be even size, got %dx%d", who, H, W);
  MI_REQUIRE((long long)H * W <= st::MAX_PIXELS, "%s: statistics: frame %dx%d has more than 2^26 pixels", who, H, W);
  MI_REQUIRE((H + st::TILE_H - 1) / st::TILE_H <= 65535, "%s: statistics: frame %dx%d has more than 65535 tile rows", who, H,
             W);
  MI_REQUIRE(a.gh <= H / 2 && a.gw <= W / 2, "%s: statistics: zones %dx%d exceed the %dx%d quads of the frame", who, a.gh,
             a.gw, H / 2, W / 2);
  return 0;
}

static int statistics_raw_impl(const void* const* src, int64_t* const* out, int n, int H, int W, int kind, int ids_format,
                               int pattern, const mi_isp_levels* levels, const mi_isp_defects* const* defects,
                               const mi_isp_statistics* s, void* stream, const char* who) {
  st::Args a = {};
  if (int rc = statistics_settings(a, s, pattern, who)) return rc;
  if (int rc = raw_geometry(H, W, MI_F32, kStatistics, who)) return rc;
  if (int rc = raw_kind(kind, kStatistics, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: statistics with %d frames", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  if (int rc = statistics_shape(a, H, W, who)) return rc;
  MI_REQUIRE(src && out, "%s: statistics: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && out[i], "%s: statistics: frame %d has a null pointer", who, i);
    MI_REQUIRE((uintptr_t)out[i] % 8 == 0, "%s: statistics: the output of frame %d is not aligned to 8 bytes", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, nullptr, 0, kStatistics, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, nullptr, defects, n, kStatistics, who)) return rc;
  for (int i0 = 0; i0 < n; i0 += st::MAX_FRAMES) {
    a.n_frames = n - i0 < st::MAX_FRAMES ? n - i0 : st::MAX_FRAMES;
    a.strip = st::strip_of(H, W, a.n_frames);
    for (int i = 0; i < a.n_frames; ++i)
      a.f[i] = {src[i0 + i], reinterpret_cast<unsigned long long*>(out[i0 + i]), mask_of(defects, i0 + i)};
    if (int rc = st::launch(a, src_kind, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int64_t mi_isp_statistics_words(const mi_isp_statistics* s) {
  if (!s || s->zones_h < 1 || s->zones_h > st::MAX_ZONES || s->zones_w < 1 || s->zones_w > st::MAX_ZONES) {
    mi_set_error("statistics_words: statistics zones outside 1 .. %d", st::MAX_ZONES);
    return -1;
  }
  return st::words(s->zones_h, s->zones_w);
}

extern "C" int mi_isp_statistics_geometry(int32_t out[4]) {
  MI_REQUIRE(out, "statistics_geometry: null pointer");
  out[0] = st::TILE_H; out[1] = st::TILE_W; out[2] = st::CELLS; out[3] = st::MAX_STRIP;
  return 0;
}

extern "C" int mi_isp_statistics_strip(int n, int H, int W) {
  if (n <= 0 || n > st::MAX_FRAMES || H <= 0 || W <= 0) {
    mi_set_error("statistics_strip: statistics: a launch of %d frames of %dx%d", n, H, W);
    return -1;
  }
  return st::strip_of(H, W, n);
}

extern "C" int mi_isp_statistics_direct_blocks(int n, int H, int W, const mi_isp_statistics* s) {
  const char* who = "statistics_direct_blocks";
  st::Args a = {};
  if (statistics_settings(a, s, MI_RGGB, who) || raw_geometry(H, W, MI_F32, kStatistics, who)) return -1;
  if (n > st::MAX_FRAMES) {
    mi_set_error("%s: statistics: a launch takes at most %d frames, got %d", who, st::MAX_FRAMES, n);
    return -1;
  }
  if (n <= 0 || H == 0 || W == 0) return 0;
  if (statistics_shape(a, H, W, who)) return -1;
  const int strip = st::strip_of(H, W, n);
  const int tiles = (W + st::TILE_W - 1) / st::TILE_W, nbx = (tiles + strip - 1) / strip, nby = (H + st::TILE_H - 1) / st::TILE_H;
  int direct = 0;
  for (int by = 0; by < nby; ++by)
    for (int bx = 0; bx < nbx; ++bx) direct += st::lds_route(H, W, a.gh, a.gw, strip, bx, by) ? 0 : 1;
  return direct;
}

extern "C" int mi_isp_statistics_raw(const void* src, int64_t* out, int H, int W, int kind, int ids_format, int pattern,
                                     const mi_isp_levels* levels, const mi_isp_defects* defects,
                                     const mi_isp_statistics* statistics, void* stream) {
  return statistics_raw_impl(&src, &out, 1, H, W, kind, ids_format, pattern, levels, &defects, statistics, stream,
                             "statistics_raw");
}

extern "C" int mi_isp_statistics_raw_batch(const void* const* src, int64_t* const* out, int n, int H, int W, int kind,
                                           int ids_format, int pattern, const mi_isp_levels* levels,
                                           const mi_isp_defects* const* defects, const mi_isp_statistics* statistics,
                                           void* stream) {
  return statistics_raw_impl(src, out, n, H, W, kind, ids_format, pattern, levels, defects, statistics, stream,
                             "statistics_raw_batch");
}

extern "C" int mi_isp_statistics_cfa(const void* cfa, int64_t* out, int H, int W, int dtype, int pattern,
                                     const mi_isp_defects* defects, const mi_isp_statistics* statistics, void* stream) {
  const char* who = "statistics_cfa";
  st::Args a = {};
  if (int rc = statistics_settings(a, statistics, pattern, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kStatistics, who)) return rc;
  if (H == 0 || W == 0) return 0;
  if (int rc = statistics_shape(a, H, W, who)) return rc;
  MI_REQUIRE(cfa && out, "%s: statistics: null pointer", who);
  MI_REQUIRE((uintptr_t)out % 8 == 0, "%s: statistics: the output of frame 0 is not aligned to 8 bytes", who);
  if (defects) {
    MI_REQUIRE(defects->n >= 0, "%s: statistics: negative defect count %d", who, (int)defects->n);
    MI_REQUIRE(defects->n == 0 || defects->mask_dev, "%s: statistics: frame 0: defects without a mask", who);
  }
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.strip = st::strip_of(H, W, 1);
  a.f[0] = {cfa, reinterpret_cast<unsigned long long*>(out), mask_of(&defects, 0)};
  return st::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, (hipStream_t)stream);
}

// ---- directional demosaic (isp_demosaic_dir.h; DESIGN.md 3, "Directional demosaic") ---------------------------------
static const RawStage kDirectional = {"demosaic_directional", "demosaic_directional: ", "frame"};

// the shape, the pattern and the colour matrix, checked on the host; fills the operator members of a
static int directional_settings(dd::Args& a, int H, int W, int pattern, const float* ccm9, int out_dtype, const char* who) {
  MI_REQUIRE(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "%s: demosaic_directional: the frame must be of even size >= 2, got %dx%d",
             who, H, W);
  MI_REQUIRE(H <= dd::TILE_H * 65535 && W < (1 << 24), "%s: demosaic_directional: frame %dx%d too large", who, H, W);
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: demosaic_directional: bad pattern %d", who, pattern);
  a.green_par = (pattern == MI_RGGB || pattern == MI_BGGR) ? 1 : 0;
  a.red_par = (pattern == MI_RGGB || pattern == MI_GRBG) ? 0 : 1;
  a.has_ccm = ccm9 != nullptr;
  for (int i = 0; i < 9; ++i) a.ccm[i] = ccm9 ? ccm9[i] : (i % 4 == 0 ? 1.f : 0.f);
  a.out_scale = mi_scale_factor(out_dtype);
  return 0;
}

extern "C" int mi_isp_demosaic_directional_cfa(const void* cfa, void* rgb, int H, int W, int in_dtype, int out_dtype,
                                               int pattern, const float* ccm9, void* stream) {
  const char* who = "demosaic_directional_cfa";
  MI_REQUIRE(cfa && rgb, "%s: demosaic_directional: null pointer", who);
  MI_REQUIRE(in_dtype == MI_F16 || in_dtype == MI_F32, "%s: demosaic_directional: the CFA must be f16 or f32 (dtype %d)", who,
             in_dtype);
  MI_REQUIRE(mi_valid_dtype(out_dtype), "%s: demosaic_directional: bad output dtype %d", who, out_dtype);
  MI_REQUIRE(mi_aligned(cfa, mi_dtype_size(in_dtype)) && mi_aligned(rgb, mi_dtype_size(out_dtype)),
             "%s: demosaic_directional: the CFA or the image not aligned to its element", who);
  dd::Args a = {};
  if (int rc = directional_settings(a, H, W, pattern, ccm9, out_dtype, who)) return rc;
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {cfa, rgb};
  return dd::launch(a, in_dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, in_dtype, out_dtype, (hipStream_t)stream);
}

// n raw frames of one geometry through the demosaic (rgb) or the decode alone (!rgb): MAX_FRAMES frames per launch
static int directional_raw_impl(const void* const* src, void* const* dst, int n, int H, int W, int kind, int ids_format,
                                int work_dtype, int pattern, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                const float* ccm9, bool rgb, void* stream, const char* who) {
  dd::Args a = {};
  MI_REQUIRE(work_dtype == MI_F16 || work_dtype == MI_F32, "%s: demosaic_directional: work dtype must be f16 or f32 (dtype %d)",
             who, work_dtype);
  if (int rc = directional_settings(a, H, W, rgb ? pattern : MI_RGGB, ccm9, work_dtype, who)) return rc;
  if (int rc = raw_kind(kind, kDirectional, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: demosaic_directional with %d frames", who, n);
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, 0, kDirectional, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, nullptr, 0, kDirectional, who))
    return rc;
  if (n == 0) return 0;
  MI_REQUIRE(src && dst, "%s: demosaic_directional: null frame list", who);
  // a typed source (16U, 16F: 2 bytes; 32F: 4) and the output stand on their element; packed bytes stand anywhere
  const size_t src_align = kind == MI_RAW_32F ? 4 : (kind == MI_RAW_16U || kind == MI_RAW_16F ? 2 : 1);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && dst[i], "%s: demosaic_directional: frame %d has a null pointer", who, i);
    MI_REQUIRE(mi_aligned(src[i], src_align) && mi_aligned(dst[i], mi_dtype_size(work_dtype)),
               "%s: demosaic_directional: frame %d not aligned to its element", who, i);
    MI_REQUIRE(src[i] != dst[i], "%s: demosaic_directional: frame %d: the output must not overwrite its source", who, i);
  }
  for (int i0 = 0; i0 < n; i0 += dd::MAX_FRAMES) {
    a.n_frames = n - i0 < dd::MAX_FRAMES ? n - i0 : dd::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i) a.f[i] = {src[i0 + i], dst[i0 + i]};
    if (int rc = rgb ? dd::launch(a, src_kind, work_dtype, work_dtype, (hipStream_t)stream)
                     : dd::launch_cfa(a, src_kind, work_dtype, (hipStream_t)stream))
      return rc;
  }
  return 0;
}

extern "C" int mi_isp_demosaic_directional_raw_batch(const void* const* src, void* const* rgb, int n, int H, int W, int kind,
                                                     int ids_format, int work_dtype, int pattern,
                                                     const mi_isp_levels* levels, const mi_isp_shading* shading,
                                                     const float* ccm9, void* stream) {
  return directional_raw_impl(src, rgb, n, H, W, kind, ids_format, work_dtype, pattern, levels, shading, ccm9, true, stream,
                              "demosaic_directional_raw_batch");
}

extern "C" int mi_isp_raw_cfa_batch(const void* const* src, void* const* cfa, int n, int H, int W, int kind, int ids_format,
                                    int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                    void* stream) {
  return directional_raw_impl(src, cfa, n, H, W, kind, ids_format, work_dtype, MI_RGGB, levels, shading, nullptr, false, stream,
                              "raw_cfa_batch");
}

// ---- chromatic aberration (isp_chromatic.h; DESIGN.md 3, "Chromatic aberration") --------------------------------------
// the largest shift |(k0 - 1) + q (k1 + q k2)| r of a channel over an H x W frame, in double: at ca::SHIFT_SAMPLES equally
// spaced radii from 0 to the distance of the farthest corner pixel from the centre, q = r^2 / norm_radius^2
static double chromatic_max_shift(const mi_isp_chromatic* s, const double k[3], int H, int W) {
  const double ry = std::fmax(std::fabs(s->cy), std::fabs((double)(H - 1) - s->cy));
  const double rx = std::fmax(std::fabs(s->cx), std::fabs((double)(W - 1) - s->cx));
  const double rmax = std::sqrt(ry * ry + rx * rx), n2 = s->norm_radius * s->norm_radius;
  double worst = 0.0;
  for (int i = 0; i < ca::SHIFT_SAMPLES; ++i) {
    const double r = rmax * (double)i / (double)(ca::SHIFT_SAMPLES - 1);
    const double q = r * r / n2;
    const double shift = std::fabs((k[0] - 1.0) + q * (k[1] + q * k[2])) * r;
    if (!(shift <= worst)) worst = shift;            // (a NaN is kept, and rejected by the caller)
  }
  return worst;
}

// the operator's settings, the demosaic pattern and the frame shape, checked on the host; fills the operator members of a
static int chromatic_settings(ca::Args& a, const mi_isp_chromatic* s, int pattern, int H, int W, int dtype,
                              const char* who) {
  static const int colours[4][4] = {{0, 1, 1, 2}, {1, 0, 2, 1}, {1, 2, 0, 1}, {2, 1, 1, 0}};   // RGGB GRBG GBRG BGGR
  MI_REQUIRE(s, "%s: null chromatic aberration settings", who);
  MI_REQUIRE(std::isfinite(s->cy) && std::isfinite(s->cx), "%s: chromatic aberration centre (%g, %g) must be finite", who,
             s->cy, s->cx);
  MI_REQUIRE(std::isfinite(s->norm_radius) && s->norm_radius > 0.0, "%s: chromatic aberration norm_radius %g must be finite and > 0",
             who, s->norm_radius);
  for (int k = 0; k < 3; ++k)
    MI_REQUIRE(std::isfinite(s->red[k]) && std::isfinite(s->blue[k]),
               "%s: chromatic aberration coefficient %d (red %g, blue %g) must be finite", who, k, s->red[k], s->blue[k]);
  MI_REQUIRE(pattern >= MI_RGGB && pattern <= MI_BGGR, "%s: bad chromatic aberration pattern %d", who, pattern);
  MI_REQUIRE(H >= 0 && W >= 0, "%s: bad chromatic aberration shape %dx%d", who, H, W);
  MI_REQUIRE(H < (1 << 22) && W < (1 << 22), "%s: chromatic aberration frame %dx%d too large", who, H, W);
  MI_REQUIRE(dtype == MI_F16 || dtype == MI_F32, "%s: chromatic aberration work dtype must be f16 or f32", who);
  a.cy = (float)s->cy; a.cx = (float)s->cx;
  a.iR2 = (float)(1.0 / (s->norm_radius * s->norm_radius));
  a.dr[0] = (float)(s->red[0] - 1.0); a.dr[1] = (float)s->red[1]; a.dr[2] = (float)s->red[2];
  a.db[0] = (float)(s->blue[0] - 1.0); a.db[1] = (float)s->blue[1]; a.db[2] = (float)s->blue[2];
  bool finite = std::isfinite(a.cy) && std::isfinite(a.cx) && std::isfinite(a.iR2);
  for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(a.dr[k]) && std::isfinite(a.db[k]);
  MI_REQUIRE(finite, "%s: chromatic aberration settings overflow f32", who);
  if (H > 0 && W > 0) {
    const double mr = chromatic_max_shift(s, s->red, H, W), mb = chromatic_max_shift(s, s->blue, H, W);
    MI_REQUIRE(mr <= ca::MAX_SHIFT && mb <= ca::MAX_SHIFT,
               "%s: chromatic aberration shift (red %g, blue %g raw pixels on a %dx%d frame) exceeds %g", who, mr, mb, H, W,
               ca::MAX_SHIFT);
    a.halo = ca::halo_for(mr > mb ? mr : mb);
  }
  for (int k = 0; k < 4; ++k) a.colour[k] = colours[pattern][k];
  return 0;
}

// n raw frames of one geometry: every frame's pointers (and defect mask) in the kernel arguments, 32 per launch
static int chromatic_raw_impl(const void* const* src, void* const* cfa, int n, int H, int W, int kind, int ids_format,
                              int work_dtype, int pattern, const mi_isp_levels* levels, const mi_isp_shading* shading,
                              const mi_isp_defects* const* defects, const mi_isp_chromatic* s, int plain, void* stream,
                              const char* who) {
  ca::Args a = {};
  if (int rc = chromatic_settings(a, s, pattern, H, W, work_dtype, who)) return rc;
  if (int rc = raw_kind(kind, kChromatic, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: chromatic aberration with %d frames", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  MI_REQUIRE(src && cfa, "%s: chromatic aberration: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && cfa[i], "%s: chromatic aberration: frame %d has a null pointer", who, i);
    MI_REQUIRE(src[i] != cfa[i], "%s: chromatic aberration: frame %d: the CFA must not overwrite its source", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, plain, kChromatic, who)) return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kChromatic, who))
    return rc;
  const int out = plain ? hl::OUT_PLAIN : (work_dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32);
  for (int i0 = 0; i0 < n; i0 += ca::MAX_FRAMES) {
    a.n_frames = n - i0 < ca::MAX_FRAMES ? n - i0 : ca::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i) a.f[i] = {src[i0 + i], cfa[i0 + i], mask_of(defects, i0 + i)};
    if (int rc = ca::launch(a, src_kind, out, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_chromatic_raw(const void* src, void* cfa, int H, int W, int kind, int ids_format, int work_dtype,
                                    int pattern, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                    const mi_isp_defects* defects, const mi_isp_chromatic* chromatic, int out_f32_plain,
                                    void* stream) {
  return chromatic_raw_impl(&src, &cfa, 1, H, W, kind, ids_format, work_dtype, pattern, levels, shading, &defects,
                            chromatic, out_f32_plain, stream, "chromatic_raw");
}

extern "C" int mi_isp_chromatic_raw_batch(const void* const* src, void* const* cfa, int n, int H, int W, int kind,
                                          int ids_format, int work_dtype, int pattern, const mi_isp_levels* levels,
                                          const mi_isp_shading* shading, const mi_isp_defects* const* defects,
                                          const mi_isp_chromatic* chromatic, int out_f32_plain, void* stream) {
  return chromatic_raw_impl(src, cfa, n, H, W, kind, ids_format, work_dtype, pattern, levels, shading, defects, chromatic,
                            out_f32_plain, stream, "chromatic_raw_batch");
}

extern "C" int mi_isp_chromatic_cfa(const void* in, void* out, int H, int W, int dtype, int pattern,
                                    const mi_isp_chromatic* chromatic, void* stream) {
  const char* who = "chromatic_cfa";
  ca::Args a = {};
  if (int rc = chromatic_settings(a, chromatic, pattern, H, W, dtype, who)) return rc;
  if (H == 0 || W == 0) return 0;
  MI_REQUIRE(in && out, "%s: chromatic aberration: null pointer", who);
  MI_REQUIRE(in != out, "%s: chromatic aberration: the output must not overwrite the input", who);
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {in, out, nullptr};
  return ca::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype == MI_F16 ? hl::OUT_F16 : hl::OUT_F32,
                    (hipStream_t)stream);
}

// ---- temporal noise reduction (isp_temporal.h; DESIGN.md 3, "Temporal noise reduction") ------------------------------
// the operator's settings, checked on the host; fills the operator members of a (each rounded once from double)
static int temporal_settings(tn::Args& a, const mi_isp_temporal* t, const char* who) {
  MI_REQUIRE(t, "%s: null temporal settings", who);
  MI_REQUIRE(std::isfinite(t->gain) && t->gain >= 0.f, "%s: temporal gain %g must be finite and >= 0", who, (double)t->gain);
  MI_REQUIRE(std::isfinite(t->read_noise) && t->read_noise > 0.f, "%s: temporal read_noise %g must be finite and > 0", who,
             (double)t->read_noise);
  MI_REQUIRE(std::isfinite(t->threshold) && t->threshold > 0.f, "%s: temporal threshold %g must be finite and > 0", who,
             (double)t->threshold);
  MI_REQUIRE(std::isfinite(t->max_weight) && t->max_weight >= 0.f && t->max_weight < 1.f,
             "%s: temporal max_weight %g must be in [0, 1)", who, (double)t->max_weight);
  const double rn = t->read_noise, th = t->threshold;
  a.gain = t->gain;
  a.rn2 = (float)(rn * rn);
  a.c = (float)(th * th);
  a.wmax = t->max_weight;
  MI_REQUIRE(std::isfinite(a.rn2) && a.rn2 > 0.f, "%s: temporal read_noise %g: its square must be finite and > 0 in f32", who,
             rn);
  MI_REQUIRE(std::isfinite(a.c) && a.c > 0.f, "%s: temporal threshold %g: its square must be finite and > 0 in f32", who, th);
  a.rcp_n[0] = 0.f;
  for (int n = 1; n < 10; ++n) a.rcp_n[n] = (float)(1.0 / (double)n);
  return 0;
}

static bool ranges_overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return p && q && a < b + nq && b < a + np;
}

// no frame's new history plane may overlap a plane that any frame of the call reads or writes
static int temporal_overlaps(const void* const* src, size_t src_bytes, const float* const* hin, float* const* hout,
                             void* const* cfa, size_t cfa_bytes, int n, size_t plane, const char* who) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      MI_REQUIRE(!ranges_overlap(hout[i], plane, src[j], src_bytes),
                 "%s: temporal: the new history of frame %d overlaps the source of frame %d", who, i, j);
      MI_REQUIRE(!(hin && ranges_overlap(hout[i], plane, hin[j], plane)),
                 "%s: temporal: the new history of frame %d overlaps the history of frame %d", who, i, j);
      MI_REQUIRE(!(cfa && ranges_overlap(hout[i], plane, cfa[j], cfa_bytes)),
                 "%s: temporal: the new history of frame %d overlaps the CFA of frame %d", who, i, j);
      MI_REQUIRE(i == j || !ranges_overlap(hout[i], plane, hout[j], plane),
                 "%s: temporal: the new histories of frames %d and %d overlap", who, i, j);
    }
  return 0;
}

// n raw frames of one geometry: every frame's pointers (and defect mask) in the kernel arguments, 32 per launch
static int temporal_raw_impl(const void* const* src, const float* const* hin, float* const* hout, void* const* cfa, int n,
                             int H, int W, int kind, int ids_format, int work_dtype, const mi_isp_levels* levels,
                             const mi_isp_shading* shading, const mi_isp_defects* const* defects, const mi_isp_temporal* t,
                             int plain, void* stream, const char* who) {
  tn::Args a = {};
  if (int rc = temporal_settings(a, t, who)) return rc;
  if (int rc = raw_geometry(H, W, work_dtype, kTemporal, who)) return rc;
  if (int rc = raw_kind(kind, kTemporal, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: temporal with %d frames", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  MI_REQUIRE(src && hout && (cfa || plain), "%s: temporal: null frame list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && hout[i], "%s: temporal: frame %d has a null pointer", who, i);
    MI_REQUIRE(plain || cfa[i], "%s: temporal: frame %d has a null CFA", who, i);
    MI_REQUIRE(plain || src[i] != cfa[i], "%s: temporal: frame %d: the CFA must not overwrite its source", who, i);
  }
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, plain, kTemporal, who)) return rc;
  const size_t px = (size_t)H * (size_t)W;
  const size_t src_bytes = kind == MI_RAW_PACKED12 ? px * 3 / 2 : (kind == MI_RAW_32F ? px * 4 : px * 2);
  if (int rc = temporal_overlaps(src, src_bytes, hin, hout, plain ? nullptr : cfa, px * mi_dtype_size(work_dtype), n, px * 4,
                                 who))
    return rc;
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kTemporal, who))
    return rc;
  const int out = plain ? tn::OUT_PLAIN : (work_dtype == MI_F16 ? tn::OUT_F16 : tn::OUT_F32);
  for (int i0 = 0; i0 < n; i0 += tn::MAX_FRAMES) {
    a.n_frames = n - i0 < tn::MAX_FRAMES ? n - i0 : tn::MAX_FRAMES;
    for (int i = 0; i < a.n_frames; ++i)
      a.f[i] = {src[i0 + i], plain ? nullptr : cfa[i0 + i], hin ? hin[i0 + i] : nullptr, hout[i0 + i],
                mask_of(defects, i0 + i)};
    if (int rc = tn::launch(a, src_kind, out, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_temporal_raw(const void* src, const float* hist_in, float* hist_out, void* cfa, int H, int W, int kind,
                                   int ids_format, int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                   const mi_isp_defects* defects, const mi_isp_temporal* temporal, int out_f32_plain,
                                   void* stream) {
  return temporal_raw_impl(&src, &hist_in, &hist_out, &cfa, 1, H, W, kind, ids_format, work_dtype, levels, shading, &defects,
                           temporal, out_f32_plain, stream, "temporal_raw");
}

extern "C" int mi_isp_temporal_raw_batch(const void* const* src, const float* const* hist_in, float* const* hist_out,
                                         void* const* cfa, int n, int H, int W, int kind, int ids_format, int work_dtype,
                                         const mi_isp_levels* levels, const mi_isp_shading* shading,
                                         const mi_isp_defects* const* defects, const mi_isp_temporal* temporal,
                                         int out_f32_plain, void* stream) {
  return temporal_raw_impl(src, hist_in, hist_out, cfa, n, H, W, kind, ids_format, work_dtype, levels, shading, defects,
                           temporal, out_f32_plain, stream, "temporal_raw_batch");
}

extern "C" int mi_isp_temporal_cfa(const void* in, const float* hist_in, float* hist_out, void* out, int H, int W, int dtype,
                                   const mi_isp_temporal* temporal, void* stream) {
  const char* who = "temporal_cfa";
  tn::Args a = {};
  if (int rc = temporal_settings(a, temporal, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kTemporal, who)) return rc;
  if (H == 0 || W == 0) return 0;
  MI_REQUIRE(in && out && hist_out, "%s: temporal: null pointer", who);
  MI_REQUIRE(in != out, "%s: temporal: the output must not overwrite the input", who);
  const size_t px = (size_t)H * (size_t)W;
  const float* hins[1] = {hist_in};
  if (int rc = temporal_overlaps(&in, px * mi_dtype_size(dtype), hins, &hist_out, &out, px * mi_dtype_size(dtype), 1, px * 4,
                                 who))
    return rc;
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_frames = 1;
  a.f[0] = {in, out, hist_in, hist_out, nullptr};
  return tn::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype == MI_F16 ? tn::OUT_F16 : tn::OUT_F32,
                    (hipStream_t)stream);
}

// ---- exposure merge (isp_exposure_merge.h; DESIGN.md 3, "Exposure merge") --------------------------------------------
// the operator's settings, checked on the host; fills the operator members of a (each rounded once from double)
static int merge_settings(em::Args& a, const mi_isp_exposure_merge* m, const char* who) {
  MI_REQUIRE(m, "%s: null exposure merge settings", who);
  MI_REQUIRE(m->n >= 2 && m->n <= em::MAX_E, "%s: exposure merge takes 2 to 4 exposures, got %d", who, (int)m->n);
  MI_REQUIRE(m->ratio[0] == 1.f, "%s: exposure merge ratio[0] %g must be 1 (the shortest exposure first)", who,
             (double)m->ratio[0]);
  for (int e = 1; e < m->n; ++e)
    MI_REQUIRE(std::isfinite(m->ratio[e]) && m->ratio[e] > m->ratio[e - 1] && m->ratio[e] <= 65536.f,
               "%s: exposure merge ratio[%d] %g must be finite, above ratio[%d] and <= 65536", who, e, (double)m->ratio[e],
               e - 1);
  MI_REQUIRE(std::isfinite(m->gain) && m->gain >= 0.f, "%s: exposure merge gain %g must be finite and >= 0", who,
             (double)m->gain);
  MI_REQUIRE(std::isfinite(m->read_noise) && m->read_noise > 0.f, "%s: exposure merge read_noise %g must be finite and > 0",
             who, (double)m->read_noise);
  MI_REQUIRE(std::isfinite(m->saturation) && m->saturation > 0.f, "%s: exposure merge saturation %g must be finite and > 0",
             who, (double)m->saturation);
  MI_REQUIRE(std::isfinite(m->knee) && m->knee > 0.f && m->knee <= 1.f, "%s: exposure merge knee %g must be in (0, 1]", who,
             (double)m->knee);
  MI_REQUIRE(std::isfinite(m->threshold) && m->threshold > 0.f, "%s: exposure merge threshold %g must be finite and > 0", who,
             (double)m->threshold);
  const double rn = m->read_noise, th = m->threshold;
  a.E = m->n;
  for (int e = 0; e < em::MAX_E; ++e) {
    const double q = e < m->n ? (double)m->ratio[e] : 1.0;
    a.inv[e] = (float)(1.0 / q);
    a.i2[e] = (float)(1.0 / (q * q));
    MI_REQUIRE(std::isfinite(a.inv[e]) && a.inv[e] > 0.f && std::isfinite(a.i2[e]) && a.i2[e] > 0.f,
               "%s: exposure merge ratio[%d] %g: 1 / ratio and 1 / ratio^2 must be finite and > 0 in f32", who, e, q);
  }
  a.gain = m->gain;
  a.rn2 = (float)(rn * rn);
  a.c = (float)(th * th);
  a.sat = m->saturation;
  a.rf = (float)(1.0 / ((double)m->saturation * (double)m->knee));
  MI_REQUIRE(std::isfinite(a.rn2) && a.rn2 > 0.f, "%s: exposure merge read_noise %g: its square must be finite and > 0 in f32",
             who, rn);
  MI_REQUIRE(std::isfinite(a.c) && a.c > 0.f, "%s: exposure merge threshold %g: its square must be finite and > 0 in f32", who,
             th);
  MI_REQUIRE(std::isfinite(a.rf) && a.rf > 0.f,
             "%s: exposure merge: 1 / (saturation * knee) must be finite and > 0 in f32 (saturation %g, knee %g)", who,
             (double)m->saturation, (double)m->knee);
  a.rcp_n[0] = 0.f;
  for (int n = 1; n < 10; ++n) a.rcp_n[n] = (float)(1.0 / (double)n);
  return 0;
}

// n brackets of one geometry (src: n * E pointers, bracket-major): every bracket's pointers (and defect mask) in the kernel
// arguments, 16 per launch
static int merge_raw_impl(const void* const* src, void* const* out, int n, int H, int W, int kind, int ids_format,
                          int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                          const mi_isp_defects* const* defects, const mi_isp_exposure_merge* m, int plain, void* stream,
                          const char* who) {
  em::Args a = {};
  if (int rc = merge_settings(a, m, who)) return rc;
  if (int rc = raw_geometry(H, W, work_dtype, kMerge, who)) return rc;
  if (int rc = raw_kind(kind, kMerge, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: exposure merge with %d brackets", who, n);
  if (n == 0 || H == 0 || W == 0) return 0;
  MI_REQUIRE(src && out, "%s: exposure merge: null bracket list", who);
  const int E = a.E;
  if (int rc = raw_source_rules(H, W, kind, ids_format, shading, plain, kMerge, who)) return rc;
  const size_t px = (size_t)H * (size_t)W;
  const size_t src_bytes = kind == MI_RAW_PACKED12 ? px * 3 / 2 : (kind == MI_RAW_32F ? px * 4 : px * 2);
  const size_t out_bytes = plain ? px * 4 : px * mi_dtype_size(work_dtype);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(out[i], "%s: exposure merge: bracket %d has a null output", who, i);
    for (int e = 0; e < E; ++e)
      MI_REQUIRE(src[(size_t)i * E + e], "%s: exposure merge: bracket %d has a null frame %d", who, i, e);
  }
  for (int i = 0; i < n; ++i)                         // no output may overlap a frame any bracket of the call reads
    for (int j = 0; j < n; ++j) {
      for (int e = 0; e < E; ++e)
        MI_REQUIRE(!ranges_overlap(out[i], out_bytes, src[(size_t)j * E + e], src_bytes),
                   "%s: exposure merge: the output of bracket %d overlaps frame %d of bracket %d", who, i, e, j);
      MI_REQUIRE(i == j || !ranges_overlap(out[i], out_bytes, out[j], out_bytes),
                 "%s: exposure merge: the outputs of brackets %d and %d overlap", who, i, j);
    }
  int src_kind;
  if (int rc = raw_source_setup(a, src_kind, H, W, kind, ids_format, levels, shading, defects, n, kMerge, who))
    return rc;
  const int o = plain ? em::OUT_PLAIN : (work_dtype == MI_F16 ? em::OUT_F16 : em::OUT_F32);
  for (int i0 = 0; i0 < n; i0 += em::MAX_BRACKETS) {
    a.n_brackets = n - i0 < em::MAX_BRACKETS ? n - i0 : em::MAX_BRACKETS;
    for (int i = 0; i < a.n_brackets; ++i) {
      em::Bracket& b = a.b[i];
      b = {};
      for (int e = 0; e < E; ++e) b.src[e] = src[(size_t)(i0 + i) * E + e];
      b.dst = out[i0 + i];
      b.mask = mask_of(defects, i0 + i);
    }
    if (int rc = em::launch(a, src_kind, o, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_merge_raw(const void* const* src, void* out, int H, int W, int kind, int ids_format, int work_dtype,
                                const mi_isp_levels* levels, const mi_isp_shading* shading, const mi_isp_defects* defects,
                                const mi_isp_exposure_merge* merge, int out_f32_plain, void* stream) {
  return merge_raw_impl(src, &out, 1, H, W, kind, ids_format, work_dtype, levels, shading, &defects, merge, out_f32_plain,
                        stream, "merge_raw");
}

extern "C" int mi_isp_merge_raw_batch(const void* const* src, void* const* out, int n, int H, int W, int kind, int ids_format,
                                      int work_dtype, const mi_isp_levels* levels, const mi_isp_shading* shading,
                                      const mi_isp_defects* const* defects, const mi_isp_exposure_merge* merge,
                                      int out_f32_plain, void* stream) {
  return merge_raw_impl(src, out, n, H, W, kind, ids_format, work_dtype, levels, shading, defects, merge, out_f32_plain,
                        stream, "merge_raw_batch");
}

extern "C" int mi_isp_merge_cfa(const void* const* in, void* out, int H, int W, int dtype,
                                const mi_isp_exposure_merge* merge, void* stream) {
  const char* who = "merge_cfa";
  em::Args a = {};
  if (int rc = merge_settings(a, merge, who)) return rc;
  if (int rc = raw_geometry(H, W, dtype, kMerge, who)) return rc;
  if (H == 0 || W == 0) return 0;
  MI_REQUIRE(in && out, "%s: exposure merge: null pointer", who);
  const size_t bytes = (size_t)H * (size_t)W * mi_dtype_size(dtype);
  for (int e = 0; e < a.E; ++e) {
    MI_REQUIRE(in[e], "%s: exposure merge: null frame %d", who, e);
    MI_REQUIRE(!ranges_overlap(out, bytes, in[e], bytes), "%s: exposure merge: the output overlaps frame %d", who, e);
  }
  a.H = H; a.W = W; a.mask_w = (W + 31) / 32;
  a.n_brackets = 1;
  a.b[0] = {};
  for (int e = 0; e < a.E; ++e) a.b[0].src[e] = in[e];
  a.b[0].dst = out;
  return em::launch(a, dtype == MI_F16 ? raw::SRC_CFA_F16 : raw::SRC_CFA_F32, dtype == MI_F16 ? em::OUT_F16 : em::OUT_F32,
                    (hipStream_t)stream);
}

// ---- local tone mapping (isp_local_tonemap.h; DESIGN.md 3, "Local tone mapping") -------------------------------------
static int32_t f32_bits(float v) {
  int32_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

// the settings checked, and the constants of the contract from them into a (H, W, the planes and the images are the
// caller's)
static int local_tonemap_settings(const mi_isp_local_tonemap* s, ltm::Args& a, const char* who) {
  MI_REQUIRE(s, "%s: null local_tonemap settings", who);
  MI_REQUIRE(std::isfinite(s->strength) && s->strength >= 0.f && s->strength <= 1.f,
             "%s: local_tonemap strength %g outside [0, 1]", who, (double)s->strength);
  MI_REQUIRE(std::isfinite(s->white) && s->white > 0.f, "%s: local_tonemap white %g must be finite and > 0", who,
             (double)s->white);
  MI_REQUIRE(std::isnormal(s->floor) && s->floor > 0.f && s->floor < s->white,
             "%s: local_tonemap floor %g must be a normal f32 within (0, white = %g)", who, (double)s->floor, (double)s->white);
  MI_REQUIRE((double)s->white / (double)s->floor <= 16777216.0, "%s: local_tonemap white / floor = %g above 2^24", who,
             (double)s->white / (double)s->floor);
  MI_REQUIRE(std::isfinite(s->anchor) && s->anchor >= s->floor && s->anchor <= s->white,
             "%s: local_tonemap anchor %g outside [floor = %g, white = %g]", who, (double)s->anchor, (double)s->floor,
             (double)s->white);
  MI_REQUIRE(s->cell == 8 || s->cell == 16 || s->cell == 32 || s->cell == 64, "%s: local_tonemap cell %d not 8, 16, 32 or 64",
             who, (int)s->cell);
  MI_REQUIRE(s->bins >= 2 && s->bins <= ltm::MAX_BINS, "%s: local_tonemap bins %d outside 2 .. %d", who, (int)s->bins,
             ltm::MAX_BINS);
  const int32_t fb = f32_bits(s->floor);
  const int32_t span = (f32_bits(s->white) - fb) >> 12;
  MI_REQUIRE(span >= 1, "%s: local_tonemap white %g within 2^-11 stops of floor %g", who, (double)s->white, (double)s->floor);
  a.cell = s->cell;
  a.cell_shift = s->cell == 8 ? 3 : (s->cell == 16 ? 4 : (s->cell == 32 ? 5 : 6));
  a.bins = s->bins;
  a.floor_v = s->floor; a.white = s->white; a.floor_bits = fb;
  a.zs = (float)((double)(s->bins - 1) / (double)span);
  a.kq = (float)((double)s->strength * 4096.0);
  a.la = (float)((f32_bits(s->anchor) - fb) >> 12);
  a.inv_cell = 1.0f / (float)s->cell;
  return 0;
}

static int local_tonemap_shape(int H, int W, int dtype, const char* who) {
  MI_REQUIRE(H >= 0 && W >= 0 && H <= ltm::MAX_SIDE && W <= ltm::MAX_SIDE, "%s: local_tonemap image %dx%d outside 0 .. %d", who,
             H, W, ltm::MAX_SIDE);
  MI_REQUIRE(dtype == MI_F16 || dtype == MI_F32, "%s: local_tonemap takes MI_F16 or MI_F32 images, got dtype %d", who, dtype);
  return 0;
}

extern "C" size_t mi_isp_local_tonemap_workspace_bytes(int n, int H, int W, const mi_isp_local_tonemap* s) {
  ltm::Args a = {};
  if (n <= 0 || H <= 0 || W <= 0 || H > ltm::MAX_SIDE || W > ltm::MAX_SIDE ||
      local_tonemap_settings(s, a, "local_tonemap_workspace_bytes"))
    return 0;
  return ltm::workspace_bytes(n, H, W, s->cell, s->bins);
}

extern "C" int mi_isp_local_tonemap_batch(void* const* images, int n, int H, int W, int dtype, const mi_isp_local_tonemap* s,
                                          void* ws, void* stream) {
  const char* who = "local_tonemap_batch";
  ltm::Args a = {};
  if (int rc = local_tonemap_settings(s, a, who)) return rc;
  MI_REQUIRE(n >= 0, "%s: local_tonemap with %d images", who, n);
  if (int rc = local_tonemap_shape(H, W, dtype, who)) return rc;
  if (n == 0 || (size_t)H * (size_t)W == 0) return 0;
  MI_REQUIRE(images, "%s: null local_tonemap image list", who);
  MI_REQUIRE(ws && mi_aligned(ws, 16), "%s: local_tonemap workspace null or not 16-byte aligned", who);
  for (int i = 0; i < n; ++i)
    MI_REQUIRE(images[i] && mi_aligned(images[i], mi_dtype_size(dtype)),
               "%s: local_tonemap image %d null or not aligned to its element", who, i);
  a.H = H; a.W = W;
  a.GH = (H + s->cell - 1) / s->cell; a.GW = (W + s->cell - 1) / s->cell;
  a.plane = ltm::plane_elems(H, W, s->cell, s->bins);
  uint32_t* base = static_cast<uint32_t*>(ws);
  for (int i0 = 0; i0 < n; i0 += ltm::MAX_IMAGES) {
    a.n_images = n - i0 < ltm::MAX_IMAGES ? n - i0 : ltm::MAX_IMAGES;
    // the four planes of the workspace, n images each; this launch's images start at i0
    a.cnt = base + (0 * (size_t)n + i0) * a.plane;
    a.sum = base + (1 * (size_t)n + i0) * a.plane;
    a.nb = reinterpret_cast<float*>(base + (2 * (size_t)n + i0) * a.plane);
    a.sb = reinterpret_cast<float*>(base + (3 * (size_t)n + i0) * a.plane);
    for (int i = 0; i < a.n_images; ++i) a.im[i] = images[i0 + i];
    if (int rc = ltm::launch(a, dtype, 0, 2, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_local_tonemap_grids(const void* image, int H, int W, int dtype, const mi_isp_local_tonemap* s,
                                          uint32_t* cnt, uint32_t* sum, float* nb, float* sb, void* stream) {
  const char* who = "local_tonemap_grids";
  ltm::Args a = {};
  if (int rc = local_tonemap_settings(s, a, who)) return rc;
  if (int rc = local_tonemap_shape(H, W, dtype, who)) return rc;
  if ((size_t)H * (size_t)W == 0) return 0;
  MI_REQUIRE(image && mi_aligned(image, mi_dtype_size(dtype)), "%s: local_tonemap image null or not aligned to its element", who);
  MI_REQUIRE(cnt && sum && nb && sb, "%s: null local_tonemap plane", who);
  MI_REQUIRE(mi_aligned(cnt, 4) && mi_aligned(sum, 4) && mi_aligned(nb, 4) && mi_aligned(sb, 4),
             "%s: local_tonemap plane not 4-byte aligned", who);
  const size_t bytes = ltm::grid_nodes(H, W, s->cell, s->bins) * 4;
  const uintptr_t p[4] = {(uintptr_t)cnt, (uintptr_t)sum, (uintptr_t)nb, (uintptr_t)sb};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      MI_REQUIRE(p[i] + bytes <= p[j] || p[j] + bytes <= p[i], "%s: local_tonemap planes %d and %d overlap", who, i, j);
  a.H = H; a.W = W;
  a.GH = (H + s->cell - 1) / s->cell; a.GW = (W + s->cell - 1) / s->cell;
  a.plane = 0;
  a.n_images = 1;
  a.cnt = cnt; a.sum = sum; a.nb = nb; a.sb = sb;
  a.im[0] = const_cast<void*>(image);
  return ltm::launch(a, dtype, 0, 1, (hipStream_t)stream);
}

// ---- antialiased resize (isp_resample.h; DESIGN.md 3, "Antialiased resize") -----------------------------------------
extern "C" int mi_isp_resample_taps(int filter, int S, int D, double scale) {
  return rs::taps(filter, S, D, scale, "resample_taps");
}

extern "C" int mi_isp_resample_table(int filter, int S, int D, double scale, int32_t* start, float* weight) {
  return rs::table(filter, S, D, scale, start, weight, "resample_table");
}

static int resample_axis(const mi_isp_resample_axis* t, int S, const char* what, const char* who) {
  MI_REQUIRE(t, "%s: null resample %s table", who, what);
  MI_REQUIRE(t->taps >= 1 && t->taps <= rs::MAX_TAPS && t->taps <= S, "%s: resample %s table with %d taps outside "
             "1 .. min(%d, %d source samples)", who, what, (int)t->taps, rs::MAX_TAPS, S);
  MI_REQUIRE(t->start_dev && t->weight_dev, "%s: resample %s table without starts or weights", who, what);
  MI_REQUIRE(mi_aligned(t->start_dev, 4) && mi_aligned(t->weight_dev, 4), "%s: resample %s table not 4-byte aligned", who,
             what);
  return 0;
}

// n images of one geometry: every image's pointers in the kernel arguments, 32 per launch
extern "C" int mi_isp_resample_batch(const void* const* srcs, void* const* dsts, int n, int Hs, int Ws, int Hd, int Wd,
                                     int in_dtype, int out_dtype, const mi_isp_resample_axis* rows,
                                     const mi_isp_resample_axis* cols, void* stream) {
  const char* who = "resample_batch";
  MI_REQUIRE(n >= 0, "%s: resample with %d images", who, n);
  MI_REQUIRE(Hs > 0 && Ws > 0 && Hs <= 32768 && Ws <= 32768, "%s: resample source %d x %d outside 1 .. 32768", who, Hs, Ws);
  MI_REQUIRE(Hd >= 0 && Wd >= 0 && Hd <= 32768 && Wd <= 32768, "%s: resample output %d x %d outside 0 .. 32768", who, Hd, Wd);
  MI_REQUIRE((in_dtype == MI_F16 || in_dtype == MI_F32) && (out_dtype == MI_F16 || out_dtype == MI_F32),
             "%s: resample takes MI_F16 / MI_F32 images, got dtypes %d -> %d", who, in_dtype, out_dtype);
  if (int rc = resample_axis(rows, Hs, "row", who)) return rc;
  if (int rc = resample_axis(cols, Ws, "column", who)) return rc;
  if (n == 0 || (size_t)Hd * (size_t)Wd == 0) return 0;
  MI_REQUIRE(srcs && dsts, "%s: null resample image list", who);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(srcs[i] && dsts[i], "%s: resample image %d has a null pointer", who, i);
    MI_REQUIRE(mi_aligned(srcs[i], mi_dtype_size(in_dtype)) && mi_aligned(dsts[i], mi_dtype_size(out_dtype)),
               "%s: resample image %d not aligned to its element", who, i);
    MI_REQUIRE(srcs[i] != dsts[i], "%s: resample image %d: the filter cannot run in place", who, i);
  }
  rs::Args a = {};
  a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
  a.rows = {rows->taps, rows->start_dev, rows->weight_dev};
  a.cols = {cols->taps, cols->start_dev, cols->weight_dev};
  for (int i0 = 0; i0 < n; i0 += rs::MAX_IMAGES) {
    a.n_images = n - i0 < rs::MAX_IMAGES ? n - i0 : rs::MAX_IMAGES;
    for (int i = 0; i < a.n_images; ++i) a.im[i] = {srcs[i0 + i], dsts[i0 + i]};
    if (int rc = rs::launch(a, in_dtype, out_dtype, (hipStream_t)stream)) return rc;
  }
  return 0;
}

// ---- the filters on the u8 outputs (isp_u8_stage.h): one front end ----------------------------------------------------------
// n u8 images of one geometry (rgb: H x W x 3; else planar YUV 4:2:0 with an H x W Y plane, whose untouched rows are copied):
// every image's pointers in the kernel arguments, 32 per launch.  Where the five stages' rules differ, they differ here: the
// texts name the stage by its noun, and the order of an entry point's checks is the order of its calls.  So whether the
// empty return (u8_nothing) comes before or after the list check is no field here: it is where the entry point puts that
// line, because local contrast's tile and workspace checks sit between the two and a flag could not say that.
struct U8Stage {
  const char* noun;
  bool one_image;                 // n == 0 is an error (else: nothing to do)
  bool even_width;                // the Y plane of the YUV form must have an even width as well as an even height
  bool in_place;                  // src[i] == dst[i] exactly is allowed: the one exception to the overlap rule of u8_images
};
static const U8Stage kSharpen = {"sharpen", true, false, false},
                     kLocalContrast = {"local_contrast", false, true, true},
                     kChromaDenoise = {"chroma_denoise", false, true, false},
                     kLumaDenoise = {"luma_denoise", false, true, false},
                     kColorLut = {"color_lut", false, false, true};    // (RGB only: no evenness rule applies)

// one 256-thread block per 128 x 64 pixels: the launch's work-items per image must stay below 2^32
static_assert(2 * cdn::TILE_CW == u8::TILE_W && 2 * cdn::TILE_CH == u8::TILE_H, "the chroma_denoise tile in pixels");
static bool u8_tiles_fit(int H, int W) {
  return H < (1 << 22) && W < (1 << 24) &&
         (uint64_t)((W + u8::TILE_W - 1) / u8::TILE_W) * (uint64_t)((H + u8::TILE_H - 1) / u8::TILE_H) < (1u << 24);
}

static bool u8_nothing(int n, int H, int W) { return n == 0 || (size_t)H * (size_t)W == 0; }
static size_t u8_bytes(bool rgb, int H, int W) { return rgb ? (size_t)H * W * 3 : (size_t)H * W * 3 / 2; }    // of one image

// the count, the shape, the stage's size limit (fits) and the evenness of the YUV form
static int u8_shape(int n, int H, int W, bool rgb, bool fits, const U8Stage& st, const char* who) {
  if (st.one_image) MI_REQUIRE(n >= 1, "%s: %s needs at least one image, got %d", who, st.noun, n);
  else MI_REQUIRE(n >= 0, "%s: %s with %d images", who, st.noun, n);
  MI_REQUIRE(H >= 0 && W >= 0, "%s: bad %s shape %dx%d", who, st.noun, H, W);
  MI_REQUIRE(fits, "%s: %s image %dx%d too large", who, st.noun, H, W);
  if (st.even_width)
    MI_REQUIRE(rgb || (H % 2 == 0 && W % 2 == 0), "%s: the Y plane of a %s YUV 4:2:0 image must have even sides, got %dx%d",
               who, st.noun, H, W);
  MI_REQUIRE(rgb || H % 2 == 0, "%s: the Y plane of a %s YUV 4:2:0 image must have an even height, got %d", who, st.noun, H);
  return 0;
}

static int u8_list(const uint8_t* const* src, uint8_t* const* dst, const U8Stage& st, const char* who) {
  MI_REQUIRE(src && dst, "%s: null %s image list", who, st.noun);
  return 0;
}

// the n images' pointers; bytes: of one image.  Every block of a launch reads while others write, so for every stage a written
// image overlaps no read image and no other written image of the call; a stage that may run in place takes dst[i] == src[i]
// exactly, and nothing else (a shifted address, or another image's source, is read by blocks other than the one that writes it).
static int u8_images(const uint8_t* const* src, uint8_t* const* dst, int n, size_t bytes, const U8Stage& st, const char* who) {
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(src[i] && dst[i], "%s: %s image %d has a null pointer", who, st.noun, i);
    MI_REQUIRE(st.in_place || src[i] != dst[i], "%s: %s image %d: the filter cannot run in place", who, st.noun, i);
  }
  for (int i = 0; i < n; ++i) {
    const uintptr_t d = (uintptr_t)dst[i];
    for (int j = 0; j < n; ++j) {
      const uintptr_t sj = (uintptr_t)src[j], dj = (uintptr_t)dst[j];
      MI_REQUIRE(d + bytes <= sj || sj + bytes <= d || (st.in_place && i == j && d == sj), "%s: %s output %d overlaps input %d",
                 who, st.noun, i, j);
      MI_REQUIRE(i == j || d + bytes <= dj || dj + bytes <= d, "%s: %s outputs %d and %d overlap", who, st.noun, i, j);
    }
  }
  return 0;
}

// The launches: a.im and a.n_images filled 32 images at a time, launch(i0) for the group that starts at image i0, then, for
// the YUV form, bytes [first, first + count) of the group's images that are not filtered in place copied as they are
// (count 0: the RGB form, no copy).
struct U8Plane { size_t first, count; };
static U8Plane u8_chroma_rows(bool rgb, int H, int W) { return {(size_t)H * W, rgb ? 0 : (size_t)H * W / 2}; }

template <class Args, class Launch>
static int for_each_group(const uint8_t* const* src, uint8_t* const* dst, int n, Args& a, U8Plane plane, void* stream,
                          Launch launch) {
  for (int i0 = 0; i0 < n; i0 += u8::MAX_IMAGES) {
    a.n_images = n - i0 < u8::MAX_IMAGES ? n - i0 : u8::MAX_IMAGES;
    u8::Image moved[u8::MAX_IMAGES];
    int n_moved = 0;
    for (int i = 0; i < a.n_images; ++i) {
      a.im[i] = {src[i0 + i], dst[i0 + i]};
      if (plane.count && src[i0 + i] != dst[i0 + i]) moved[n_moved++] = a.im[i];
    }
    if (int rc = launch(i0)) return rc;
    if (int rc = u8::launch_copy(moved, n_moved, plane.first, plane.count, (hipStream_t)stream)) return rc;
  }
  return 0;
}

// ---- output sharpening (isp_sharpen.h; DESIGN.md 3, "Output sharpening") ---------------------------------------------
static int sharpen_impl(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W, const mi_isp_sharpen* s,
                        bool rgb, void* stream, const char* who) {
  MI_REQUIRE(s, "%s: null sharpen settings", who);
  MI_REQUIRE(s->radius == 1 || s->radius == 2, "%s: sharpen radius %d (1 or 2)", who, (int)s->radius);
  MI_REQUIRE(s->amount_q6 >= 0 && s->amount_q6 <= 512, "%s: sharpen amount_q6 %d outside 0 .. 512", who,
             (int)s->amount_q6);
  MI_REQUIRE(s->threshold >= 0 && s->threshold <= 255, "%s: sharpen threshold %d outside 0 .. 255", who,
             (int)s->threshold);
  MI_REQUIRE(s->overshoot >= -1 && s->overshoot <= 255, "%s: sharpen overshoot %d outside 0 .. 255 (-1: none)", who,
             (int)s->overshoot);
  if (int rc = u8_shape(n, H, W, rgb, u8_tiles_fit(H, W), kSharpen, who)) return rc;
  if (int rc = u8_list(src, dst, kSharpen, who)) return rc;
  if (u8_nothing(n, H, W)) return 0;
  if (int rc = u8_images(src, dst, n, u8_bytes(rgb, H, W), kSharpen, who)) return rc;
  shp::Args a = {};
  a.H = H; a.W = W;
  a.amount_q6 = s->amount_q6; a.threshold = s->threshold; a.overshoot = s->overshoot;
  return for_each_group(src, dst, n, a, u8_chroma_rows(rgb, H, W), stream,
                        [&](int) { return shp::launch(a, rgb, s->radius, (hipStream_t)stream); });
}

extern "C" int mi_isp_sharpen_rgb_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                        const mi_isp_sharpen* sharpen, void* stream) {
  return sharpen_impl(src, dst, n, H, W, sharpen, true, stream, "sharpen_rgb_batch");
}

extern "C" int mi_isp_sharpen_yuv420_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                           const mi_isp_sharpen* sharpen, void* stream) {
  return sharpen_impl(src, dst, n, H, W, sharpen, false, stream, "sharpen_yuv420_batch");
}

// ---- local contrast (isp_local_contrast.h; DESIGN.md 3, "Local contrast") ----------------------------------------------
static int local_contrast_settings(const mi_isp_local_contrast* s, const char* who) {
  MI_REQUIRE(s, "%s: null local_contrast settings", who);
  MI_REQUIRE(s->tiles_y >= 1 && s->tiles_y <= lc::MAX_TILES && s->tiles_x >= 1 && s->tiles_x <= lc::MAX_TILES,
             "%s: local_contrast tiles %d x %d outside 1 .. %d", who, (int)s->tiles_y, (int)s->tiles_x, lc::MAX_TILES);
  MI_REQUIRE(s->clip_q8 == 0 || (s->clip_q8 >= 256 && s->clip_q8 <= 64 * 256),
             "%s: local_contrast clip_q8 %d outside 256 .. 16384 (0: no clip)", who, (int)s->clip_q8);
  MI_REQUIRE(s->strength_q6 >= 0 && s->strength_q6 <= 64, "%s: local_contrast strength_q6 %d outside 0 .. 64", who,
             (int)s->strength_q6);
  return 0;
}

extern "C" size_t mi_isp_local_contrast_workspace_bytes(int n, const mi_isp_local_contrast* s) {
  if (n <= 0 || local_contrast_settings(s, "local_contrast_workspace_bytes")) return 0;
  return lc::hist_bytes(n, s->tiles_y, s->tiles_x) + lc::lut_bytes(n, s->tiles_y, s->tiles_x);
}

// (nothing to do returns before the tile fit, the list and the workspace are looked at; the chroma rows are copied for the
// images not filtered in place)
static int local_contrast_impl(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                               const mi_isp_local_contrast* s, void* ws, bool rgb, void* stream, const char* who) {
  if (int rc = local_contrast_settings(s, who)) return rc;
  if (int rc = u8_shape(n, H, W, rgb, true, kLocalContrast, who)) return rc;
  if (u8_nothing(n, H, W)) return 0;
  MI_REQUIRE(H >= s->tiles_y && W >= s->tiles_x, "%s: local_contrast image %dx%d smaller than its %d x %d tiles", who, H, W,
             (int)s->tiles_y, (int)s->tiles_x);
  MI_REQUIRE(H <= lc::MAX_SIDE && W <= lc::MAX_SIDE, "%s: local_contrast image %dx%d larger than %d", who, H, W, lc::MAX_SIDE);
  if (int rc = u8_list(src, dst, kLocalContrast, who)) return rc;
  MI_REQUIRE(ws && mi_aligned(ws, 16), "%s: local_contrast workspace null or not 16-byte aligned", who);
  if (int rc = u8_images(src, dst, n, u8_bytes(rgb, H, W), kLocalContrast, who)) return rc;
  const size_t per_image = (size_t)s->tiles_y * s->tiles_x * 256;
  uint32_t* hist = static_cast<uint32_t*>(ws);
  uint8_t* lut = static_cast<uint8_t*>(ws) + lc::hist_bytes(n, s->tiles_y, s->tiles_x);
  lc::Args a = {};
  a.H = H; a.W = W; a.Ty = s->tiles_y; a.Tx = s->tiles_x;
  a.clip_q8 = s->clip_q8; a.strength_q6 = s->strength_q6;
  return for_each_group(src, dst, n, a, u8_chroma_rows(rgb, H, W), stream, [&](int i0) {
    a.hist = hist + i0 * per_image;
    a.lut = lut + i0 * per_image;
    return lc::launch(a, rgb, (hipStream_t)stream);
  });
}

extern "C" int mi_isp_local_contrast_rgb_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                               const mi_isp_local_contrast* lc_host, void* ws, void* stream) {
  return local_contrast_impl(src, dst, n, H, W, lc_host, ws, true, stream, "local_contrast_rgb_batch");
}

extern "C" int mi_isp_local_contrast_yuv420_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                                  const mi_isp_local_contrast* lc_host, void* ws, void* stream) {
  return local_contrast_impl(src, dst, n, H, W, lc_host, ws, false, stream, "local_contrast_yuv420_batch");
}

// ---- chroma noise reduction (isp_chroma_denoise.h; DESIGN.md 3, "Chroma noise reduction") -----------------------------
// (the planar form writes U and V: the Y rows are copied)
static int chroma_denoise_impl(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                               const mi_isp_chroma_denoise* s, bool rgb, void* stream, const char* who) {
  MI_REQUIRE(s, "%s: null chroma_denoise settings", who);
  MI_REQUIRE(s->radius >= 1 && s->radius <= 3, "%s: chroma_denoise radius %d (1, 2 or 3)", who, (int)s->radius);
  MI_REQUIRE(s->luma_threshold >= 0 && s->luma_threshold <= 255, "%s: chroma_denoise luma_threshold %d outside 0 .. 255", who,
             (int)s->luma_threshold);
  MI_REQUIRE(s->chroma_threshold >= 0 && s->chroma_threshold <= 255, "%s: chroma_denoise chroma_threshold %d outside 0 .. 255",
             who, (int)s->chroma_threshold);
  MI_REQUIRE(s->strength_q6 >= 0 && s->strength_q6 <= 64, "%s: chroma_denoise strength_q6 %d outside 0 .. 64", who,
             (int)s->strength_q6);
  if (int rc = u8_shape(n, H, W, rgb, u8_tiles_fit(H, W), kChromaDenoise, who)) return rc;
  if (int rc = u8_list(src, dst, kChromaDenoise, who)) return rc;
  if (u8_nothing(n, H, W)) return 0;
  if (int rc = u8_images(src, dst, n, u8_bytes(rgb, H, W), kChromaDenoise, who)) return rc;
  cdn::Args a = {};
  a.H = H; a.W = W;
  a.tl4 = 4 * s->luma_threshold; a.tc4 = 4 * s->chroma_threshold; a.strength_q6 = s->strength_q6;
  return for_each_group(src, dst, n, a, U8Plane{0, rgb ? 0 : (size_t)H * W}, stream,
                        [&](int) { return cdn::launch(a, rgb, s->radius, (hipStream_t)stream); });
}

extern "C" int mi_isp_chroma_denoise_rgb_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                               const mi_isp_chroma_denoise* settings, void* stream) {
  return chroma_denoise_impl(src, dst, n, H, W, settings, true, stream, "chroma_denoise_rgb_batch");
}

extern "C" int mi_isp_chroma_denoise_yuv420_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                                  const mi_isp_chroma_denoise* settings, void* stream) {
  return chroma_denoise_impl(src, dst, n, H, W, settings, false, stream, "chroma_denoise_yuv420_batch");
}

// ---- luma noise reduction (isp_luma_denoise.h; DESIGN.md 3, "Luma noise reduction") -----------------------------------
static int luma_denoise_impl(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                             const mi_isp_luma_denoise* s, bool rgb, void* stream, const char* who) {
  MI_REQUIRE(s, "%s: null luma_denoise settings", who);
  MI_REQUIRE(s->radius >= 1 && s->radius <= 3, "%s: luma_denoise radius %d (1, 2 or 3)", who, (int)s->radius);
  MI_REQUIRE(s->threshold >= 0 && s->threshold <= 255, "%s: luma_denoise threshold %d outside 0 .. 255", who,
             (int)s->threshold);
  MI_REQUIRE(s->threshold_bright >= 0 && s->threshold_bright <= 255, "%s: luma_denoise threshold_bright %d outside 0 .. 255",
             who, (int)s->threshold_bright);
  MI_REQUIRE(s->strength_q6 >= 0 && s->strength_q6 <= 64, "%s: luma_denoise strength_q6 %d outside 0 .. 64", who,
             (int)s->strength_q6);
  if (int rc = u8_shape(n, H, W, rgb, u8_tiles_fit(H, W), kLumaDenoise, who)) return rc;
  if (int rc = u8_list(src, dst, kLumaDenoise, who)) return rc;
  if (u8_nothing(n, H, W)) return 0;
  if (int rc = u8_images(src, dst, n, u8_bytes(rgb, H, W), kLumaDenoise, who)) return rc;
  ydn::Args a = {};
  a.H = H; a.W = W;
  a.t0 = s->threshold; a.t1 = s->threshold_bright; a.strength_q6 = s->strength_q6;
  return for_each_group(src, dst, n, a, u8_chroma_rows(rgb, H, W), stream,
                        [&](int) { return ydn::launch(a, rgb, s->radius, (hipStream_t)stream); });
}

extern "C" int mi_isp_luma_denoise_rgb_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                             const mi_isp_luma_denoise* settings, void* stream) {
  return luma_denoise_impl(src, dst, n, H, W, settings, true, stream, "luma_denoise_rgb_batch");
}

extern "C" int mi_isp_luma_denoise_yuv420_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                                const mi_isp_luma_denoise* settings, void* stream) {
  return luma_denoise_impl(src, dst, n, H, W, settings, false, stream, "luma_denoise_yuv420_batch");
}

// ---- 3D colour LUT (isp_color_lut.h; DESIGN.md 3, "Colour LUT") ------------------------------------------------------------
// n interleaved u8 RGB images of one geometry through one table; path: clut::Path (the dispatcher's choice, or one path forced)
static int color_lut_impl(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W, const uint32_t* table,
                          const mi_isp_color_lut* s, int path, void* stream, const char* who) {
  MI_REQUIRE(s, "%s: null color_lut settings", who);
  MI_REQUIRE(s->n_points >= clut::MIN_POINTS && s->n_points <= clut::MAX_POINTS, "%s: color_lut n_points %d outside %d .. %d",
             who, (int)s->n_points, clut::MIN_POINTS, clut::MAX_POINTS);
  MI_REQUIRE(s->strength_q6 >= 0 && s->strength_q6 <= 64, "%s: color_lut strength_q6 %d outside 0 .. 64", who,
             (int)s->strength_q6);
  MI_REQUIRE(path == clut::PATH_AUTO || path == clut::PATH_GLOBAL || (path == clut::PATH_LDS && s->n_points <= clut::LDS_POINTS),
             "%s: color_lut path %d (0: the dispatcher's, 1: LDS, n_points <= %d, 2: global)", who, path, clut::LDS_POINTS);
  if (int rc = u8_shape(n, H, W, true, (uint64_t)H * (uint64_t)W < (1ull << 31), kColorLut, who)) return rc;
  MI_REQUIRE(table, "%s: null color_lut table", who);
  if (int rc = u8_list(src, dst, kColorLut, who)) return rc;
  if (u8_nothing(n, H, W)) return 0;
  if (int rc = u8_images(src, dst, n, u8_bytes(true, H, W), kColorLut, who)) return rc;
  int dev = 0;
  MI_HIP(hipGetDevice(&dev));
  clut::Args a = {};
  a.pixels = (uint32_t)((size_t)H * (size_t)W);
  a.dword_rows = W % 4 == 0;
  a.n_points = s->n_points; a.strength_q6 = s->strength_q6;
  a.table = table;
  return for_each_group(src, dst, n, a, U8Plane{0, 0}, stream,
                        [&](int) { return clut::launch(a, (clut::Path)path, ew::device_cus(dev), (hipStream_t)stream); });
}

extern "C" int mi_isp_color_lut_rgb_batch(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                          const uint32_t* table, const mi_isp_color_lut* settings, void* stream) {
  return color_lut_impl(src, dst, n, H, W, table, settings, clut::PATH_AUTO, stream, "color_lut_rgb_batch");
}

extern "C" int mi_isp_color_lut_rgb_batch_path(const uint8_t* const* src, uint8_t* const* dst, int n, int H, int W,
                                               const uint32_t* table, const mi_isp_color_lut* settings, int path,
                                               void* stream) {
  return color_lut_impl(src, dst, n, H, W, table, settings, path, stream, "color_lut_rgb_batch_path");
}

// ---- measurement aid: HIP events around each data pass, on the stream it runs on ---------------------
#include <vector>
static struct {
  std::mutex mu;                  // the ABI is callable from several threads (one per stream)
  bool on = false;
  std::vector<hipEvent_t> ev;     // 8 per sampled frame: (start, stop) x 4 passes
  size_t used = 0;
  int every = 1;                  // every n-th frame is sampled (events between launches cost gaps)
  long frames_seen = 0;
  std::vector<int> npass;         // passes recorded per sampled frame (4; 1 for a whole-frame launch)
} g_prof;

extern "C" int mi_isp_profile_enable(int max_frames, int every) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
  g_prof.ev.clear();
  g_prof.used = 0;
  g_prof.on = max_frames > 0;
  g_prof.every = every > 0 ? every : 1;
  g_prof.frames_seen = 0;
  g_prof.npass.assign(max_frames > 0 ? max_frames : 0, 4);
  for (int i = 0; i < 8 * max_frames; ++i) {
    hipEvent_t e;
    MI_HIP(hipEventCreate(&e));
    g_prof.ev.push_back(e);
  }
  return 0;
}

extern "C" int mi_isp_profile_collect(float avg_us[4], int* count) {
  MI_REQUIRE(avg_us && count, "profile_collect: null pointer");
  std::lock_guard<std::mutex> lock(g_prof.mu);
  double sum[4] = {0, 0, 0, 0};
  int n = 0;
  for (size_t f = 0; f + 8 <= g_prof.used; f += 8, ++n) {
    for (int k = 0; k < g_prof.npass[f / 8]; ++k) {
      float ms = 0.f;
      MI_HIP(hipEventSynchronize(g_prof.ev[f + 2 * k + 1]));
      MI_HIP(hipEventElapsedTime(&ms, g_prof.ev[f + 2 * k], g_prof.ev[f + 2 * k + 1]));
      sum[k] += ms * 1e3;
    }
  }
  for (int k = 0; k < 4; ++k) avg_us[k] = n ? (float)(sum[k] / n) : 0.f;
  *count = n;
  g_prof.used = 0;
  return 0;
}

// RAII-less helper: events of pass k of the frame whose slots start at `base` (or nothing)
struct PassTimer {
  size_t base; bool on; hipStream_t s;
  int begin(int k) const { if (on) MI_HIP(hipEventRecord(g_prof.ev[base + 2 * k], s)); return 0; }
  int end(int k) const { if (on) MI_HIP(hipEventRecord(g_prof.ev[base + 2 * k + 1], s)); return 0; }
};
static PassTimer pass_timer(hipStream_t s, int npass = 4) {
  std::lock_guard<std::mutex> lock(g_prof.mu);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (g_prof.on) (void)hipStreamIsCapturing(s, &cap);
  if (cap != hipStreamCaptureStatusNone) return PassTimer{0, false, s};   // events inside a graph cannot be timed
  const bool sampled = g_prof.on && (g_prof.frames_seen++ % g_prof.every) == 0;
  PassTimer t = {g_prof.used, sampled && g_prof.used + 8 <= g_prof.ev.size(), s};
  if (t.on) { g_prof.npass[g_prof.used / 8] = npass; g_prof.used += 8; }
  return t;
}

// One frame of the fused config-2 chain, recompute variant (output dtype != work dtype): four tile passes over
// the packed frame + three finalize launches.
static int pipeline_frame(tile::Params p, int pattern, int work_dtype, float intensity, float* ws, hipStream_t s) {
  float* fp = ws;
  float* partials = ws + FP_COUNT;
  const int cap = mi_partial_cap(p.H, p.W);
  const int nb = tile::num_tiles(p.H, p.W);
  p.fp = fp; p.partials = partials; p.part_stride = cap;
  ew::FinArgs fa = {};
  fa.partials = partials; fa.stride = cap; fa.nblocks = nb; fa.fp = fp;
  fa.n_px = (float)((int64_t)p.H * p.W); fa.intensity = intensity; fa.la = p.la; fa.ca = p.ca;
  fa.bounds_post = work_dtype == MI_F16 ? 2 : 1;
  const PassTimer tm = pass_timer(s);
  static const int epis[4] = {tile::EPI_MINMAX, tile::EPI_STATS, tile::EPI_RH_MINMAX, tile::EPI_RH_STORE};
  static const int fins[3] = {ew::FIN_BOUNDS, ew::FIN_STATS, ew::FIN_BOUNDS2};   // tonemap.py:146, :147-149, :150-153, :154
  for (int k = 0; k < 4; ++k) {
    if (int rc = tm.begin(k)) return rc;
    if (int rc = tile::launch(p, work_dtype, pattern, epis[k], s)) return rc;
    if (int rc = tm.end(k)) return rc;
    if (k < 3)
      if (int rc = ew::finalize(fins[k], fa, s)) return rc;
  }
  return 0;
}

// The "cached" variant of the same chain, used when the output has the work dtype (f16 -> f16,
// f32 -> f32): the first pass writes the demosaiced work-dtype image INTO THE OUTPUT BUFFER while
// reducing its bounds; the three tonemap passes then run elementwise on that image, the last one in
// place.  One demosaic instead of four (the path is vector-issue-bound) at the price
// of re-reading the 6 B/px image three times (it stays resident in the 256 MB Infinity Cache).
// which: -1 = the whole chain; 0..3 = only that data pass (measurement aid).
// `image`: where the work-dtype image lives between the passes (H * W * 3 work-dtype elements) - the output
// buffer itself when the output has the work dtype, a caller-provided buffer otherwise; `out` / `out_dtype`:
// the final destination of pass 3.
static int pipeline_frame_cached(tile::Params p, int pattern, int work_dtype, float gamma, float intensity,
                                 float* ws, int which, hipStream_t s, void* image, void* out, int out_dtype,
                                 bool stream0) {
  float* fp = ws;
  float* partials = ws + FP_COUNT;
  const int cap = mi_partial_cap(p.H, p.W);
  p.fp = fp; p.partials = partials; p.part_stride = cap;
  p.dst = image; p.vec_store = vec_store_ok(image, p.W, work_dtype);
  p.out_dtype = work_dtype; p.out_scale = 1.f;
  const PassTimer tm = which < 0 ? pass_timer(s) : PassTimer{0, false, s};
  if (int rc = tm.begin(0)) return rc;
  int n_bounds = tile::num_tiles(p.H, p.W);
  if (stream0) {
    strm::SArgs a = {};
    a.t = p;
    strm::geometry(p.H, p.W, a);
    n_bounds = a.n_blocks;
    if (which < 0 || which == 0)
      if (int rc = strm::launch(a, work_dtype, pattern, strm::S_STORE_BOUNDS, s)) return rc;
  } else if (which < 0 || which == 0) {
    if (int rc = tile::launch(p, work_dtype, pattern, tile::EPI_STORE_MINMAX, s)) return rc;   // bayer.py + tonemap.py:146
  }
  if (int rc = tm.end(0)) return rc;
  if (which == 0) return 0;
  const ew::PullSrc bounds = {partials, cap, n_bounds, work_dtype == MI_F16 ? 2 : 1};
  if (which > 0)
    return ew::tonemap_reinhard_tail(image, out, p.H, p.W, work_dtype, out_dtype, gamma, intensity, p.la, p.ca, ws,
                                     which, bounds, s);
  for (int k = 1; k <= 3; ++k) {
    if (int rc = tm.begin(k)) return rc;
    if (int rc = ew::tonemap_reinhard_tail(image, out, p.H, p.W, work_dtype, out_dtype, gamma, intensity, p.la,
                                           p.ca, ws, k, bounds, s))
      return rc;
    if (int rc = tm.end(k)) return rc;
  }
  return 0;
}

// ---- the whole-frame kernel (isp_mega.h) --------------------------------------------------------------------------
// Two whole-frame grids must never share the chip: each needs every one of its blocks resident for its grid barriers,
// and two half-resident grids would wait for each other (the kernel's bounded poll would turn that into an error flag,
// not a hang - but the frames would be lost).  Launches on ONE stream are ordered by the stream.  Across streams the
// library orders them itself: under one lock per process it makes the new stream wait for an event the library
// recorded right behind the previous whole-frame launch, launches, and records that event again - the lock is held
// over all three, so two threads cannot interleave (round 2 released it before the launch: a second thread could
// record "done" ahead of the first thread's kernel).  The previous caller's stream handle is only ever compared, never
// used.  Launches captured by the CALLER into a graph of his own are not ordered by the library (nothing can be waited
// for at capture time): he must keep them off parallel branches, and replays of such a graph must not run beside
// direct launches on other streams.  Other PROCESSES on the same GPU are invisible to all of this: a foreign kernel that
// holds CUs makes the barrier time out - which is what the fault word, the mailbox and the multi-pass fallback are for.
// Round 4: the order, its lock, the event and the mailbox page are those of ALL resident-grid kernels of the library
// (ew::resident_launch, isp_elementwise.h) - the one-launch metering and the camera-group kernel take part in the same order.
static struct {
  int per_cu[4] = {-1, -1, -1, -1};          // per CFA pattern: the allocator's outcome differs per instantiation
  int sabotage_block = -1;                   // tests: this block never posts at barrier 0 of a launch's first frame
  std::atomic<uint32_t> launches{0};         // the host's part of a launch's tag (isp_mega.h)
} g_mega;
static inline std::mutex& mega_mu() { return ew::resident_order().mu; }

static bool mega_fits(const tile::Params& p, int work_dtype, const void* out, int out_dtype, int pattern, strm::SArgs& a) {
  if (work_dtype != MI_F16 || mi_dtype_size(out_dtype) > 2) return false;
  if (!use_stream(p, work_dtype, out, out_dtype) || !p.vec_store) return false;
  if (pattern < 0 || pattern > 3) return false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
  std::lock_guard<std::mutex> lock(mega_mu());
  if (g_mega.per_cu[pattern] < 0) g_mega.per_cu[pattern] = mega::blocks_per_cu(pattern);
  const int n_cus = ew::device_cus(dev);
  // fewer than two resident blocks per CU (a spilling or fatter instantiation) would deadlock the barrier: refuse
  return n_cus > 0 && g_mega.per_cu[pattern] >= 2 && mega::geometry(p.H, p.W, n_cus, a);
}

// One launch for frames [0, n): same geometry and parameters, frame i reads srcs[i], writes dsts[i] and owns the workspace
// ws + i * ws_floats.  Ordered against the previous whole-frame launch of this process on this device (see above).
static int mega_launch_frames(tile::Params p, strm::SArgs a, int pattern, float intensity, const uint8_t* const* srcs,
                              void* const* dsts, float* ws, size_t ws_floats, int n, hipStream_t s) {
  p.src = nullptr; p.dst = nullptr; p.fp = nullptr; p.partials = nullptr;
  p.part_stride = mi_partial_cap(p.H, p.W);
  a.t = p;
  a.n_px = (float)((int64_t)p.H * p.W); a.intensity = intensity; a.fp_w = nullptr; a.bounds_post = 2;
  int dev = 0;
  MI_HIP(hipGetDevice(&dev));
  MI_REQUIRE(dev >= 0 && dev < 16, "whole-frame kernel: device index %d out of range", dev);
  return ew::resident_launch(dev, s, ew::MAILBOX_WHOLE_FRAME, ew::CAPTURED_UNORDERED,
                             [&](unsigned* mailbox, unsigned limit, bool direct) {
    mega::MBatch mb = {};
    mb.m.s = a;
    mb.m.spin_limit = limit ? limit : 100000;                  // ~100 ms of polling before a wave gives up
    mb.m.l2_first = 1;
    mb.m.poll_sleep = 0;                                       // extra 512-cycle naps between two polls (swept: 0 is best)
    mb.m.mailbox = mailbox;
    mb.m.sabotage_block = g_mega.sabotage_block;
#ifdef MI_ISP_MEASURE
    if (getenv("MI_ISP_POLL_SLEEP")) mb.m.poll_sleep = (unsigned)atoi(getenv("MI_ISP_POLL_SLEEP"));
    if (getenv("MI_ISP_L2_FIRST")) mb.m.l2_first = (unsigned)atoi(getenv("MI_ISP_L2_FIRST"));
#endif
    const PassTimer tm0 = direct ? pass_timer(s, 1) : PassTimer{0, false, s};   // measurement aid: a launch as "pass 0"
    for (int i0 = 0; i0 < n; i0 += mega::MAX_BATCH) {
      mb.n_frames = n - i0 < mega::MAX_BATCH ? n - i0 : mega::MAX_BATCH;
      // the host's part of the launch's tag: a block of an EARLIER launch that comes to life late (a foreign kernel held
      // its CU) must not post records a later launch takes for its own (the workspace's own count covers graph replays,
      // whose arguments are frozen)
      mb.m.launch_id = g_mega.launches.fetch_add(1, std::memory_order_relaxed) + 1u;
      for (int i = 0; i < mb.n_frames; ++i) {
        mb.io[i].src = srcs[i0 + i];
        mb.io[i].dst = dsts[i0 + i];
        mb.io[i].ws = ws + (size_t)(i0 + i) * ws_floats;
      }
      // (events around the first launch of the call only: a call of more than 64 frames is several launches)
      const PassTimer tm = i0 == 0 ? tm0 : PassTimer{0, false, s};
      if (int rc = tm.begin(0)) return rc;
      if (int rc = mega::launch(mb, pattern, s)) return rc;
      if (int rc = tm.end(0)) return rc;
    }
    return 0;
  });
}

extern "C" size_t mi_isp_workspace_error_offset(int H, int W) {
  if (H <= 0 || W <= 0) return 0;
  return (size_t)mega::FP_ERROR * sizeof(float);
}

extern "C" int mi_isp_whole_frame_set_poll_limit(unsigned polls) { return ew::set_poll_limit(ew::MAILBOX_WHOLE_FRAME, polls); }

// Test hook: block `block` of every later whole-frame launch does not post its record at barrier 0 of the launch's first
// frame (-1: off) - the one fault a test can provoke that looks like a block which is not resident: everybody else waits
// the FULL poll budget for it.
extern "C" int mi_isp_whole_frame_set_sabotage(int block) {
  std::lock_guard<std::mutex> lock(mega_mu());
  g_mega.sabotage_block = block;
  return 0;
}

extern "C" int mi_isp_whole_frame_faults(int clear) { return ew::faults(ew::MAILBOX_WHOLE_FRAME, clear); }

extern "C" int mi_isp_workspace_check(void* ws_dev, int n_frames, int H, int W, int* failed_host, int* n_failed,
                                      void* stream) {
  MI_REQUIRE(ws_dev && n_failed, "workspace_check: null pointer");
  MI_REQUIRE(n_frames >= 0, "workspace_check: negative frame count");
  const size_t ws_bytes = mi_isp_workspace_bytes(H, W);
  MI_REQUIRE(ws_bytes > 0, "workspace_check: bad frame size");
  MI_HIP(hipStreamSynchronize((hipStream_t)stream));
  int bad = 0;
  for (int i = 0; i < n_frames; ++i) {
    unsigned* w = reinterpret_cast<unsigned*>(static_cast<char*>(ws_dev) + (size_t)i * ws_bytes) + mega::FP_ERROR;
    unsigned v = 0;
    MI_HIP(hipMemcpy(&v, w, sizeof(v), hipMemcpyDeviceToHost));
    if (failed_host) failed_host[i] = v != 0;
    if (v != 0) {
      ++bad;
      v = 0;
      MI_HIP(hipMemcpy(w, &v, sizeof(v), hipMemcpyHostToDevice));   // the word is sticky in the kernel: cleared here
      // and the barrier records of a failed frame are wiped: whatever a block that came to life late has left there can
      // then never carry the tag of a later launch (a graph replay repeats the host's part of the tag)
      float* partials = reinterpret_cast<float*>(static_cast<char*>(ws_dev) + (size_t)i * ws_bytes) + FP_COUNT;
      const size_t stride = (size_t)mi_partial_cap(H, W);
      MI_HIP(hipMemset(partials + (size_t)mega::MROW_BAR0 * stride, 0,
                       (size_t)(mega::MROW_END - mega::MROW_BAR0) * stride * sizeof(float)));
    }
  }
  *n_failed = bad;
  return 0;
}

// The same chain on the streaming kernels: every pass re-derives the demosaiced image from the packed frame
// (18.9 MB, served by L2 / Infinity Cache after the first pass) instead of writing and re-reading a 6 B/px
// intermediate; HBM sees the packed frame in and the output out.  Pass A (S_BOUNDS) also accumulates the statistics
// of tonemap.py:147-149 under the assumption that the bounds are exactly (0, 1) - true for every frame with a clipped
// pixel at both ends - and pass B (S_STATS) returns at once when that held, so the usual frame costs three data
// passes; any other frame gets the statistics from pass B.  The finalize steps are pulled into the consumers.
// which: -1 = whole chain, 0..3 = one pass (measurement aid; the partials of a full run must be in the workspace).
static int pipeline_frame_stream(tile::Params p, int pattern, int work_dtype, float intensity, float* ws, int which,
                                 hipStream_t s) {
  strm::SArgs a = {};
  p.fp = ws; p.partials = ws + FP_COUNT; p.part_stride = mi_partial_cap(p.H, p.W);
  a.t = p;
  strm::geometry(p.H, p.W, a);
  a.n_px = (float)((int64_t)p.H * p.W); a.intensity = intensity; a.fp_w = ws;
  a.bounds_post = work_dtype == MI_F16 ? 2 : 1;
  static const int epis[4] = {strm::S_BOUNDS, strm::S_STATS, strm::S_RH_MINMAX, strm::S_RH_STORE};
  const PassTimer tm = which < 0 ? pass_timer(s) : PassTimer{0, false, s};
  for (int k = 0; k < 4; ++k) {
    if (which >= 0 && which != k) continue;
    if (int rc = tm.begin(k)) return rc;
    if (int rc = strm::launch(a, work_dtype, pattern, epis[k], s)) return rc;
    if (int rc = tm.end(k)) return rc;
  }
  return 0;
}

// measurement aid: MI_ISP_PIPELINE=cached times the store-and-re-read chain on the same build
static bool force_cached() {
#ifdef MI_ISP_MEASURE
  static const bool on = getenv("MI_ISP_PIPELINE") && !strcmp(getenv("MI_ISP_PIPELINE"), "cached");
  return on;
#else
  return false;
#endif
}

static bool no_cached_pipeline() {
#ifdef MI_ISP_MEASURE
  static const bool off = getenv("MI_ISP_NO_CACHED_PIPELINE") != nullptr;   // measurement aid: the recompute tile chain
  return off;
#else
  return false;
#endif
}

// Which chain of kernels a frame of the multi-pass chain takes (mi_isp.h: MI_ISP_ROUTE_*).  The one place that decides:
// pipeline12_frame and mi_isp_pipeline12_pass launch what it says, mi_isp_pipeline12_route reports it.  Host arithmetic
// on the arguments' values only.  p: pipeline_params + packed_params, dst = out, vec_store = vec_store_ok(out).
// *image: where the cached routes keep the work-dtype image (the output itself when it has the work dtype).
static int pipeline12_route(const tile::Params& p, int work_dtype, void* out, int out_dtype, void* work_image,
                            void** image) {
  *image = nullptr;
  if (use_stream(p, work_dtype, out, out_dtype) && p.vec_store && !force_cached()) return MI_ISP_ROUTE_STREAM;
  void* im = work_dtype == out_dtype ? out : work_image;
  if (!no_cached_pipeline() && im && vec_store_ok(im, p.W, work_dtype)) {
    *image = im;
    return use_stream(p, work_dtype, im, work_dtype) ? MI_ISP_ROUTE_CACHED_STREAM : MI_ISP_ROUTE_CACHED_TILE;
  }
  return MI_ISP_ROUTE_RECOMPUTE;
}

static int pipeline_params(tile::Params& p, int H, int W, int ids_format, int pattern, const float* ccm9,
                           int work_dtype, int out_dtype, float gamma, float la, float ca) {
  if (int rc = fill_common(p, H, W, pattern, ccm9, "pipeline12_reinhard")) return rc;
  MI_REQUIRE(mi_valid_dtype(out_dtype), "pipeline12_reinhard: bad output dtype");
  MI_REQUIRE(gamma > 0.f, "pipeline12_reinhard: gamma must be positive");
  MI_REQUIRE(work_dtype == MI_F16 || work_dtype == MI_F32, "pipeline12_reinhard: work dtype must be f16/f32");
  (void)ids_format;
  p.out_dtype = out_dtype;
  p.out_scale = mi_scale_factor(out_dtype);
  p.gamma_inv = 1.0f / gamma; p.la = la; p.ca = ca;
  return 0;
}

// One frame: the cached variant when there is a place for the work-dtype image (the output itself when it has the
// work dtype, else `work_image`), the recompute variant otherwise.
// whole_frame: 0 = the multi-pass chain, 1 = the single-launch whole-frame kernel (an error when the frame does not fit)
static int pipeline12_frame(const uint8_t* packed, void* out, void* work_image, int H, int W, int ids_format,
                            int pattern, const float* ccm9, int work_dtype, int out_dtype, float gamma,
                            float intensity, float light_adapt, float color_adapt, float* ws, hipStream_t s,
                            const char* who, int whole_frame = 0) {
  tile::Params p = {};
  if (int rc = pipeline_params(p, H, W, ids_format, pattern, ccm9, work_dtype, out_dtype, gamma, light_adapt,
                               color_adapt))
    return rc;
  if (int rc = packed_params(p, packed, H, W, 12, ids_format, work_dtype, who)) return rc;
  p.dst = out;
  p.vec_store = vec_store_ok(out, W, out_dtype);
  if (whole_frame) {
    strm::SArgs ma = {};
    MI_REQUIRE(mega_fits(p, work_dtype, out, out_dtype, pattern, ma),
               "%s: the whole-frame kernel takes f16 work dtype, u8 / u16 / f16 outputs, the standard 12-bit layout with "
               "W %% 8 == 0 and 16-byte aligned buffers, and at most 2 x CUs x 4 waves of 512 x 12 pixels (4096 x 3072 on "
               "MI355X); use mi_isp_pipeline12_reinhard for this frame", who);
    const uint8_t* srcs[1] = {packed};
    void* dsts[1] = {out};
    return mega_launch_frames(p, ma, pattern, intensity, srcs, dsts, ws, 0, 1, s);
  }
  void* image = nullptr;
  switch (pipeline12_route(p, work_dtype, out, out_dtype, work_image, &image)) {
    case MI_ISP_ROUTE_STREAM: return pipeline_frame_stream(p, pattern, work_dtype, intensity, ws, -1, s);
    case MI_ISP_ROUTE_CACHED_STREAM:
      return pipeline_frame_cached(p, pattern, work_dtype, gamma, intensity, ws, -1, s, image, out, out_dtype, true);
    case MI_ISP_ROUTE_CACHED_TILE:
      return pipeline_frame_cached(p, pattern, work_dtype, gamma, intensity, ws, -1, s, image, out, out_dtype, false);
    default: return pipeline_frame(p, pattern, work_dtype, intensity, ws, s);
  }
}

extern "C" int mi_isp_pipeline12_reinhard(const uint8_t* packed, void* out, void* work_image, int H, int W,
                                          int ids_format, int pattern, const float* ccm9, int work_dtype,
                                          int out_dtype, float gamma, float intensity, float light_adapt,
                                          float color_adapt, void* ws, void* stream) {
  MI_REQUIRE(out && ws, "pipeline12_reinhard: null pointer");
  return pipeline12_frame(packed, out, work_image, H, W, ids_format, pattern, ccm9, work_dtype, out_dtype, gamma,
                          intensity, light_adapt, color_adapt, static_cast<float*>(ws), (hipStream_t)stream,
                          "pipeline12_reinhard");
}

extern "C" int mi_isp_pipeline12_route(const uint8_t* packed, void* out, void* work_image, int H, int W, int ids_format,
                                       int work_dtype, int out_dtype, mi_isp_route* route) {
  MI_REQUIRE(route, "pipeline12_route: null result");
  MI_REQUIRE(out, "pipeline12_route: null pointer");
  *route = mi_isp_route{};
  tile::Params p = {};
  if (int rc = pipeline_params(p, H, W, ids_format, MI_RGGB, nullptr, work_dtype, out_dtype, 1.f, 1.f, 0.f)) return rc;
  if (int rc = packed_params(p, packed, H, W, 12, ids_format, work_dtype, "pipeline12_route")) return rc;
  p.dst = out;
  p.vec_store = vec_store_ok(out, W, out_dtype);
  void* image = nullptr;
  route->route = pipeline12_route(p, work_dtype, out, out_dtype, work_image, &image);
  if (route->route == MI_ISP_ROUTE_CACHED_TILE) {             // the Params of pipeline_frame_cached's first pass
    p.dst = image; p.vec_store = vec_store_ok(image, W, work_dtype); p.out_dtype = work_dtype; p.out_scale = 1.f;
    route->hot = tile::hot_spec(p, work_dtype, tile::EPI_STORE_MINMAX);
  }
  if (route->route == MI_ISP_ROUTE_STREAM || route->route == MI_ISP_ROUTE_CACHED_STREAM) {
    strm::SArgs a = {};
    strm::geometry(H, W, a);
    route->rows_per_wave = a.rows_per_wave; route->bands_x = a.bands_x; route->n_blocks = a.n_blocks;
  } else {
    route->n_blocks = tile::num_tiles(H, W);
  }
  return 0;
}

extern "C" int mi_isp_pipeline12_reinhard_whole_frame(const uint8_t* packed, void* out, int H, int W, int ids_format,
                                                      int pattern, const float* ccm9, int out_dtype, float gamma,
                                                      float intensity, float light_adapt, float color_adapt, void* ws,
                                                      void* stream) {
  MI_REQUIRE(out && ws, "pipeline12_reinhard_whole_frame: null pointer");
  return pipeline12_frame(packed, out, nullptr, H, W, ids_format, pattern, ccm9, MI_F16, out_dtype, gamma, intensity,
                          light_adapt, color_adapt, static_cast<float*>(ws), (hipStream_t)stream,
                          "pipeline12_reinhard_whole_frame", 1);
}

extern "C" int mi_isp_pipeline12_whole_frame_fits(int H, int W, int out_dtype) {
  tile::Params p = {};
  p.H = H; p.W = W; p.src_kind = tile::SRC_PACKED12; p.src_fast = 1; p.in_scale = 1.f; p.vec_store = 1;
  strm::SArgs a = {};
  // asked without a pattern: all four instantiations must be launchable
  if (!(H > 0 && W > 0 && H % 2 == 0 && mi_valid_dtype(out_dtype))) return 0;
  for (int pat = 0; pat < 4; ++pat)
    if (!mega_fits(p, MI_F16, nullptr, out_dtype, pat, a)) return 0;
  return 1;
}

// n_frames frames through ONE launch of the whole-frame kernel per 64 frames (isp_mega.h: the grid stays resident and
// walks through the frames), in order, on `stream`.
extern "C" int mi_isp_pipeline12_reinhard_whole_frame_batch(const uint8_t* const* packed, void* const* out, int n_frames,
                                                            int H, int W, int ids_format, int pattern, const float* ccm9,
                                                            int out_dtype, float gamma, float intensity, float light_adapt,
                                                            float color_adapt, void* ws, void* stream) {
  const char* who = "pipeline12_reinhard_whole_frame_batch";
  MI_REQUIRE(packed && out && ws, "%s: null pointer", who);
  MI_REQUIRE(n_frames >= 1, "%s: need at least one frame", who);
  tile::Params p = {};
  strm::SArgs ma = {};
  for (int i = 0; i < n_frames; ++i) {
    MI_REQUIRE(packed[i] && out[i], "%s: frame %d has a null buffer", who, i);
    tile::Params pi = {};
    if (int rc = pipeline_params(pi, H, W, ids_format, pattern, ccm9, MI_F16, out_dtype, gamma, light_adapt, color_adapt)) return rc;
    if (int rc = packed_params(pi, packed[i], H, W, 12, ids_format, MI_F16, who)) return rc;
    pi.dst = out[i];
    pi.vec_store = vec_store_ok(out[i], W, out_dtype);
    MI_REQUIRE(mega_fits(pi, MI_F16, out[i], out_dtype, pattern, ma),
               "%s: frame %d does not fit the whole-frame kernel (see mi_isp_pipeline12_reinhard_whole_frame)", who, i);
    if (i == 0) p = pi;
  }
  return mega_launch_frames(p, ma, pattern, intensity, packed, out, static_cast<float*>(ws),
                            mi_isp_workspace_bytes(H, W) / sizeof(float), n_frames, (hipStream_t)stream);
}

extern "C" int mi_isp_pipeline12_reinhard_batch(const uint8_t* const* packed, void* const* out,
                                                void* const* work_images, int n_frames, int H, int W,
                                                int ids_format, int pattern, const float* ccm9, int work_dtype,
                                                int out_dtype, float gamma, float intensity, float light_adapt,
                                                float color_adapt, void* ws, void* const* streams, int n_streams) {
  MI_REQUIRE(packed && out && ws, "pipeline12_reinhard_batch: null pointer");
  MI_REQUIRE(n_frames >= 0, "pipeline12_reinhard_batch: negative frame count");
  MI_REQUIRE(n_streams >= 1 && streams, "pipeline12_reinhard_batch: need at least one stream");
  const size_t ws_floats = mi_isp_workspace_bytes(H, W) / sizeof(float);
  for (int i = 0; i < n_frames; ++i) {
    MI_REQUIRE(out[i], "pipeline12_reinhard_batch: output %d is null", i);
    float* wsi = static_cast<float*>(ws) + (size_t)i * ws_floats;
    if (int rc = pipeline12_frame(packed[i], out[i], work_images ? work_images[i] : nullptr, H, W, ids_format, pattern,
                                  ccm9, work_dtype, out_dtype, gamma, intensity, light_adapt, color_adapt, wsi,
                                  (hipStream_t)streams[i % n_streams], "pipeline12_reinhard_batch"))
      return rc;
  }
  return 0;
}

// ---- one camera group, packed bytes -> u8 outputs, in one call -----------------------------------------------------------
// ISP.load_packed12 / load_packed16 per camera (camera_isp.py:333-347, resize fused when scale > 0), the rolling
// metering over the group (:376-385, :142-175), then ISP.tonemap_reinhard or tonemap_linear (:394-413) with the
// orientation transform folded into the u8 store: what a frame group costs a C caller is this one call on its stream.
extern "C" int mi_isp_metering(const void* const* images, int n_images, int H, int W, int stride, int dtype, float* state9,
                               float alpha, void* ws, void* stream);
extern "C" int mi_isp_metering_to(const void* const* images, int n_images, int H, int W, int stride, int dtype,
                                  const float* prev9, float* state9, float alpha, void* ws, void* stream);
extern "C" int mi_isp_reinhard_batch(void* const* images, uint8_t* const* outs, int n, int H, int W, int dtype,
                                     const float* state9, float gamma, float intensity, float light_adapt,
                                     float color_adapt, int transform, void* ws, void* stream);
extern "C" int mi_isp_linear_batch(const void* const* images, uint8_t* const* outs, int n, int H, int W, int dtype,
                                   const float* state9, float gamma, int transform, void* ws, void* stream);

extern "C" int mi_isp_camera_frame_batch(const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n,
                                         int H, int W, int bits, int ids_format, int pattern, const float* ccm9,
                                         int work_dtype, int Hd, int Wd, float scale, int metering_stride,
                                         float* state9, float alpha, int tonemap, float gamma, float intensity,
                                         float light_adapt, float color_adapt, int transform, void* ws, void* stream) {
  MI_REQUIRE(packed && images && outs && state9 && ws, "camera_frame_batch: null pointer");
  MI_REQUIRE(n >= 1, "camera_frame_batch: need at least one camera");
  MI_REQUIRE(tonemap == 0 || tonemap == 1, "camera_frame_batch: tonemap must be 0 (reinhard) or 1 (linear)");
  MI_REQUIRE(metering_stride >= 1, "camera_frame_batch: bad metering stride");
  // (what the tonemap entries would reject, rejected before the metering moves state9)
  MI_REQUIRE(gamma > 0.f, "camera_frame_batch: gamma must be positive");
  MI_REQUIRE(transform >= MI_T_NONE && transform <= MI_T_TRANSVERSE, "camera_frame_batch: bad transform");
  MI_REQUIRE(transform != MI_T_TRANSVERSE || Hd == Wd, "camera_frame_batch: transverse needs a square image");
  for (int i = 0; i < n; ++i) MI_REQUIRE(packed[i] && images[i] && outs[i], "camera_frame_batch: camera %d has a null buffer", i);
  if (int rc = mi_isp_load_packed_batch(packed, images, nullptr, n, H, W, bits, ids_format, pattern, ccm9, work_dtype, Hd, Wd,
                                        scale, 0, stream))
    return rc;
  if (int rc = mi_isp_metering(const_cast<const void* const*>(images), n, Hd, Wd, metering_stride, work_dtype, state9,
                               alpha, ws, stream))
    return rc;
  if (tonemap == 0)
    return mi_isp_reinhard_batch(images, outs, n, Hd, Wd, work_dtype, state9, gamma, intensity, light_adapt, color_adapt,
                                 transform, ws, stream);
  return mi_isp_linear_batch(const_cast<const void* const*>(images), outs, n, Hd, Wd, work_dtype, state9, gamma, transform,
                             ws, stream);
}

// ---- one camera group at full resolution: subsample, metering, ONE persistent launch (isp_mega_cam.h) -------------------
// What the reference's bench does per step (bench/camera_isp.py:19-28: load_packed12 per camera, tonemap_reinhard over the
// list, the loaded images dropped): the stride-8 subsample of every camera straight from its packed frame
// (strm::sub_kernel), the rolling metering over the subsamples (mi_isp_metering: camera_isp.py:376-385 -> :142-175), then
// mega::camera_kernel walks through the cameras - demosaic, Reinhard, max_out at a grid barrier, u8 out - with the image
// resident on the chip.  images == NULL: p is not stored (the bench drops it); else images[i] receives what the reference
// leaves in the loaded image (camera_isp.py:211).
static int g_cam_per_cu[3][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}, {-1, -1, -1, -1}};   // [levels][pattern]

// lv: the levels instantiation (tile::Params::levels) whose occupancy counts
static bool camera_group_fits(int H, int W, int pattern, strm::SArgs& a, int lv = 0) {
  if (pattern < 0 || pattern > 3 || H <= 0 || W <= 0) return false;
  tile::Params p = {};
  p.H = H; p.W = W; p.src_kind = tile::SRC_PACKED12; p.src_fast = ((int64_t)W * 3 / 2) % 4 == 0; p.in_scale = 1.f; p.vec_store = 1;
  if (!strm::supported(p, MI_F16) || (int64_t)H * W * 6 >= (int64_t)strm::INVALID_OFF) return false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
  std::lock_guard<std::mutex> lock(mega_mu());
  if (lv < 0 || lv > 2) return false;
  if (g_cam_per_cu[lv][pattern] < 0) g_cam_per_cu[lv][pattern] = mega::cam_blocks_per_cu(pattern, lv);
  const int n_cus = ew::device_cus(dev);
  return n_cus > 0 && g_cam_per_cu[lv][pattern] >= 2 && mega::geometry(H, W, n_cus, a);
}

// the instantiation a call with these levels takes (0 without), or -1 for levels apply_levels refuses
static int levels_mode(const mi_isp_levels* lv) {
  tile::Params p = {};
  return apply_levels(p, lv, 12, "camera_group") ? -1 : p.levels;
}

extern "C" int mi_isp_camera_group_fits(int H, int W, int pattern, int work_dtype, int metering_stride) {
  strm::SArgs a = {};
  return work_dtype == MI_F16 && metering_stride == 8 && camera_group_fits(H, W, pattern, a) ? 1 : 0;
}

extern "C" int mi_isp_camera_group_fits_levels(int H, int W, int pattern, int work_dtype, int metering_stride,
                                               const mi_isp_levels* levels) {
  strm::SArgs a = {};
  const int lv = levels_mode(levels);
  return lv >= 0 && work_dtype == MI_F16 && metering_stride == 8 && camera_group_fits(H, W, pattern, a, lv) ? 1 : 0;
}

extern "C" size_t mi_isp_camera_group_scratch_bytes(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0) return 0;
  const size_t per = (size_t)((H + 7) / 8) * (size_t)((W + 7) / 8) * 3 * sizeof(half_t);
  return (size_t)n * ((per + 255) / 256 * 256);
}

extern "C" int mi_isp_camera_group_set_poll_limit(unsigned polls) { return ew::set_poll_limit(ew::MAILBOX_CAMERA_GROUP, polls); }

extern "C" int mi_isp_camera_group_faults(int clear) { return ew::faults(ew::MAILBOX_CAMERA_GROUP, clear); }

// the frames' common parameters, checked per camera
static int camera_group_params(tile::Params& p, const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n,
                               int H, int W, int pattern, const float* ccm9, const mi_isp_levels* lv, const char* who) {
  MI_REQUIRE(packed, "%s: null pointer", who);
  MI_REQUIRE(n >= 1 && n <= mega::MAX_BATCH, "%s: 1 .. %d cameras per call", who, mega::MAX_BATCH);
  for (int i = 0; i < n; ++i) {
    MI_REQUIRE(packed[i] && (!outs || outs[i]) && (!images || images[i]), "%s: camera %d has a null buffer", who, i);
    MI_REQUIRE((!outs || ((uintptr_t)outs[i] & 7) == 0) && (!images || ((uintptr_t)images[i] & 15) == 0),
               "%s: camera %d: outputs must be 8-byte, images 16-byte aligned", who, i);
    tile::Params pi = {};
    if (int rc = fill_common(pi, H, W, pattern, ccm9, who)) return rc;
    if (int rc = packed_params(pi, packed[i], H, W, 12, 0, MI_F16, who)) return rc;
    if (int rc = apply_levels(pi, lv, 12, who)) return rc;
    MI_REQUIRE(strm::supported(pi, MI_F16), "%s: camera %d: the packed frame does not take the streaming kernels "
               "(standard 12-bit layout, W %% 8 == 0, even H, 4-byte aligned rows)", who, i);
    if (i == 0) p = pi;
  }
  p.src = nullptr; p.dst = nullptr; p.fp = nullptr; p.partials = nullptr;
  return 0;
}

// step 1: image[::8, ::8] of every camera's (never materialised) image, (ceil(H / 8), ceil(W / 8), 3) f16 each, in scratch
static int camera_group_subsample_impl(const uint8_t* const* packed, int n, int H, int W, int pattern, const float* ccm9,
                                       void* scratch, const mi_isp_levels* lv, void* stream) {
  const char* who = "camera_group_subsample";
  MI_REQUIRE(scratch, "%s: null pointer", who);
  tile::Params p = {};
  if (int rc = camera_group_params(p, packed, nullptr, nullptr, n, H, W, pattern, ccm9, lv, who)) return rc;
  const size_t sub_bytes = mi_isp_camera_group_scratch_bytes(1, H, W);
  for (int i0 = 0; i0 < n; i0 += strm::LOAD_BATCH) {
    strm::SubArgs sa = {};
    sa.t = p;
    strm::sub_geometry(H, W, sa);
    sa.n_batch = n - i0 < strm::LOAD_BATCH ? n - i0 : strm::LOAD_BATCH;
    for (int i = 0; i < sa.n_batch; ++i) { sa.srcs[i] = packed[i0 + i]; sa.subs[i] = static_cast<char*>(scratch) + (size_t)(i0 + i) * sub_bytes; }
    if (int rc = strm::launch_sub(sa, MI_F16, pattern, (hipStream_t)stream)) return rc;
  }
  return 0;
}

extern "C" int mi_isp_camera_group_subsample(const uint8_t* const* packed, int n, int H, int W, int pattern, const float* ccm9,
                                             void* scratch, void* stream) {
  return camera_group_subsample_impl(packed, n, H, W, pattern, ccm9, scratch, nullptr, stream);
}

extern "C" int mi_isp_camera_group_subsample_levels(const uint8_t* const* packed, int n, int H, int W, int pattern,
                                                    const float* ccm9, void* scratch, const mi_isp_levels* levels,
                                                    void* stream) {
  return camera_group_subsample_impl(packed, n, H, W, pattern, ccm9, scratch, levels, stream);
}

// step 3: the cameras through one resident launch, with the Reinhard scalars of state9 (read on the device)
static int camera_group_tonemap_impl(const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n, int H,
                                     int W, int pattern, const float* ccm9, const float* state9, float gamma,
                                     float intensity, float light_adapt, float color_adapt, void* ws,
                                     const mi_isp_levels* lv, void* stream) {
  const char* who = "camera_group_tonemap";
  MI_REQUIRE(outs && state9 && ws, "%s: null pointer", who);
  MI_REQUIRE(gamma > 0.f, "%s: gamma must be positive", who);
  hipStream_t s = (hipStream_t)stream;
  tile::Params p = {};
  if (int rc = camera_group_params(p, packed, images, outs, n, H, W, pattern, ccm9, lv, who)) return rc;
  strm::SArgs ma = {};
  MI_REQUIRE(camera_group_fits(H, W, pattern, ma, p.levels),
             "%s: the frame does not fit the resident grid (mi_isp_camera_group_fits); use mi_isp_camera_frame_batch", who);
  p.out_dtype = MI_U8; p.out_scale = 255.f; p.gamma_inv = 1.0f / gamma; p.la = light_adapt; p.ca = color_adapt;
  p.part_stride = mi_partial_cap(H, W);
  ma.t = p;
  ma.n_px = (float)((int64_t)H * W); ma.intensity = intensity; ma.fp_w = nullptr; ma.bounds_post = 0;
  const size_t ws_floats = mi_isp_workspace_bytes(H, W) / sizeof(float);
  int dev = 0;
  MI_HIP(hipGetDevice(&dev));
  MI_REQUIRE(dev >= 0 && dev < 16, "%s: device index %d out of range", who, dev);
  return ew::resident_launch(dev, s, ew::MAILBOX_CAMERA_GROUP, ew::CAPTURED_UNORDERED,
                             [&](unsigned* mailbox, unsigned limit, bool) {
    mega::CBatch cb = {};
    cb.m.s = ma;
    cb.m.spin_limit = limit ? limit : 100000;
    cb.m.l2_first = 1;
    cb.m.poll_sleep = 0;
    cb.m.mailbox = mailbox;
    cb.m.sabotage_block = -1;
    cb.m.launch_id = g_mega.launches.fetch_add(1, std::memory_order_relaxed) + 1u;
    cb.state9 = state9;
    cb.gamma_inv = 1.0f / gamma;
    cb.n_frames = n;
    for (int i = 0; i < n; ++i) {
      cb.io[i].src = packed[i];
      cb.io[i].p_out = images ? images[i] : nullptr;
      cb.io[i].out = outs[i];
      cb.io[i].ws = static_cast<float*>(ws) + (size_t)i * ws_floats;
    }
    return mega::launch_cam(cb, pattern, s);
  });
}

extern "C" int mi_isp_camera_group_tonemap(const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n, int H,
                                           int W, int pattern, const float* ccm9, const float* state9, float gamma,
                                           float intensity, float light_adapt, float color_adapt, void* ws, void* stream) {
  return camera_group_tonemap_impl(packed, images, outs, n, H, W, pattern, ccm9, state9, gamma, intensity, light_adapt,
                                   color_adapt, ws, nullptr, stream);
}

extern "C" int mi_isp_camera_group_tonemap_levels(const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n,
                                                  int H, int W, int pattern, const float* ccm9, const float* state9,
                                                  float gamma, float intensity, float light_adapt, float color_adapt,
                                                  void* ws, const mi_isp_levels* levels, void* stream) {
  return camera_group_tonemap_impl(packed, images, outs, n, H, W, pattern, ccm9, state9, gamma, intensity, light_adapt,
                                   color_adapt, ws, levels, stream);
}

static int camera_group_reinhard_impl(const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n,
                                      int H, int W, int pattern, const float* ccm9, const float* prev9, float* state9,
                                      float alpha, float gamma, float intensity, float light_adapt, float color_adapt,
                                      void* scratch, void* ws, const mi_isp_levels* lv, void* stream) {
  const char* who = "camera_group_reinhard";
  MI_REQUIRE(packed && outs && prev9 && state9 && scratch && ws, "%s: null pointer", who);
  MI_REQUIRE(n >= 1 && n <= mega::MAX_BATCH, "%s: 1 .. %d cameras per call", who, mega::MAX_BATCH);
  {                                                          // refuse before anything is launched
    const int mode = levels_mode(lv);
    if (mode < 0) return 1;                                  // (apply_levels set the message)
    strm::SArgs ma = {};
    MI_REQUIRE(camera_group_fits(H, W, pattern, ma, mode),
               "%s: the frame does not fit the resident grid (mi_isp_camera_group_fits); use mi_isp_camera_frame_batch", who);
  }
  // 1. the subsample of every camera, straight from its packed frame
  if (int rc = camera_group_subsample_impl(packed, n, H, W, pattern, ccm9, scratch, lv, stream)) return rc;
  // 2. the rolling metering over the group (its own workspace: the last of the n + 1)
  const int Hs = (H + 7) / 8, Ws = (W + 7) / 8;
  const size_t sub_bytes = mi_isp_camera_group_scratch_bytes(1, H, W);
  const void* subs[mega::MAX_BATCH];
  for (int i = 0; i < n; ++i) subs[i] = static_cast<char*>(scratch) + (size_t)i * sub_bytes;
  const size_t ws_floats = mi_isp_workspace_bytes(H, W) / sizeof(float);
  float* ws_meter = static_cast<float*>(ws) + (size_t)n * ws_floats;
  if (int rc = mi_isp_metering_to(subs, n, Hs, Ws, 1, MI_F16, prev9, state9, alpha, ws_meter, stream)) return rc;
  // 3. the cameras through one resident launch
  return camera_group_tonemap_impl(packed, images, outs, n, H, W, pattern, ccm9, state9, gamma, intensity, light_adapt,
                                   color_adapt, ws, lv, stream);
}

extern "C" int mi_isp_camera_group_reinhard(const uint8_t* const* packed, void* const* images, uint8_t* const* outs, int n,
                                            int H, int W, int pattern, const float* ccm9, const float* prev9, float* state9,
                                            float alpha, float gamma, float intensity, float light_adapt, float color_adapt,
                                            void* scratch, void* ws, void* stream) {
  return camera_group_reinhard_impl(packed, images, outs, n, H, W, pattern, ccm9, prev9, state9, alpha, gamma, intensity,
                                    light_adapt, color_adapt, scratch, ws, nullptr, stream);
}

extern "C" int mi_isp_camera_group_reinhard_levels(const uint8_t* const* packed, void* const* images, uint8_t* const* outs,
                                                   int n, int H, int W, int pattern, const float* ccm9, const float* prev9,
                                                   float* state9, float alpha, float gamma, float intensity,
                                                   float light_adapt, float color_adapt, void* scratch, void* ws,
                                                   const mi_isp_levels* levels, void* stream) {
  return camera_group_reinhard_impl(packed, images, outs, n, H, W, pattern, ccm9, prev9, state9, alpha, gamma, intensity,
                                    light_adapt, color_adapt, scratch, ws, levels, stream);
}

// ---- a batch as a HIP graph: capture once, replay per step ---------------------------------------------------------
// What BatchPipeline(use_graph=True) has, for C callers: the step - fork to `n_streams` internal streams, the launches of
// every frame (frame i on stream i % n_streams), join - is captured into a graph bound to the given buffers; a replay
// has no launch gaps between the dependent kernels of a stream.  whole_frame: every frame through the single-launch
// kernel, one after the other on one stream (two of them must not overlap).
struct BatchGraph {
  bool whole_frame = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
};

static void batch_graph_free(BatchGraph* b) {
  if (!b) return;
  if (b->exec) (void)hipGraphExecDestroy(b->exec);
  if (b->graph) (void)hipGraphDestroy(b->graph);
  for (hipEvent_t e : b->events) (void)hipEventDestroy(e);
  for (hipStream_t s : b->streams) (void)hipStreamDestroy(s);
  delete b;
}

extern "C" int mi_isp_pipeline12_whole_frame_fits(int H, int W, int out_dtype);
extern "C" int mi_isp_pipeline12_graph_create(const uint8_t* const* packed, void* const* out, void* const* work_images,
                                              int n_frames, int H, int W, int ids_format, int pattern,
                                              const float* ccm9, int work_dtype, int out_dtype, float gamma,
                                              float intensity, float light_adapt, float color_adapt, void* ws,
                                              int n_streams, int whole_frame, void** handle) {
  MI_REQUIRE(packed && out && ws && handle, "pipeline12_graph_create: null pointer");
  MI_REQUIRE(n_frames > 0 && n_streams >= 1, "pipeline12_graph_create: need at least one frame and one stream");
  if (whole_frame) {
    n_streams = 1;
    (void)mi_isp_pipeline12_whole_frame_fits(H, W, out_dtype);   // device queries happen outside the capture
  }
  BatchGraph* b = new BatchGraph();
  b->whole_frame = whole_frame != 0;
  bool capturing = false;
  auto fail = [&](int rc) {
    if (capturing) {                                         // a capture must be ended (and its graph dropped) before its stream goes
      hipGraph_t dead = nullptr;
      (void)hipStreamEndCapture(b->streams[0], &dead);
      if (dead) (void)hipGraphDestroy(dead);
      (void)hipGetLastError();
    }
    batch_graph_free(b);
    return rc;
  };
#define MI_HIP_G(expr)                                                                              \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) {                                                                         \
      mi_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);     \
      return fail(2);                                                                               \
    }                                                                                               \
  } while (0)
  for (int i = 0; i < n_streams; ++i) {
    hipStream_t s;
    MI_HIP_G(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    b->streams.push_back(s);
  }
  for (int i = 0; i < n_streams; ++i) {
    hipEvent_t e;
    MI_HIP_G(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    b->events.push_back(e);
  }
  hipStream_t s0 = b->streams[0];
  MI_HIP_G(hipStreamBeginCapture(s0, hipStreamCaptureModeThreadLocal));
  capturing = true;
  MI_HIP_G(hipEventRecord(b->events[0], s0));                                   // fork
  for (int i = 1; i < n_streams; ++i) MI_HIP_G(hipStreamWaitEvent(b->streams[i], b->events[0], 0));
  const size_t ws_floats = mi_isp_workspace_bytes(H, W) / sizeof(float);
  int rc = 0;
  if (whole_frame) {
    rc = mi_isp_pipeline12_reinhard_whole_frame_batch(packed, out, n_frames, H, W, ids_format, pattern, ccm9, out_dtype, gamma,
                                                      intensity, light_adapt, color_adapt, ws, s0);
  } else {
    for (int i = 0; i < n_frames && rc == 0; ++i) {
      float* wsi = static_cast<float*>(ws) + (size_t)i * ws_floats;
      rc = pipeline12_frame(packed[i], out[i], work_images ? work_images[i] : nullptr, H, W, ids_format, pattern, ccm9,
                            work_dtype, out_dtype, gamma, intensity, light_adapt, color_adapt, wsi,
                            b->streams[i % n_streams], "pipeline12_graph_create", 0);
    }
  }
  for (int i = 1; i < n_streams; ++i) {                                          // join
    (void)hipEventRecord(b->events[i], b->streams[i]);
    (void)hipStreamWaitEvent(s0, b->events[i], 0);
  }
  hipGraph_t g = nullptr;
  const hipError_t ec = hipStreamEndCapture(s0, &g);
  capturing = false;
  b->graph = g;
  if (rc != 0) return fail(rc);
  if (ec != hipSuccess) { mi_set_error("pipeline12_graph_create: capture failed: %s", hipGetErrorString(ec)); return fail(2); }
  MI_HIP_G(hipGraphInstantiate(&b->exec, b->graph, nullptr, nullptr, 0));
#undef MI_HIP_G
  *handle = b;
  return 0;
}

extern "C" int mi_isp_pipeline12_graph_launch(void* handle, void* stream) {
  MI_REQUIRE(handle, "pipeline12_graph_launch: null handle");
  BatchGraph* b = static_cast<BatchGraph*>(handle);
  if (b->whole_frame) {                                      // its grids need the chip to themselves, like a direct launch
    int dev = 0;
    MI_HIP(hipGetDevice(&dev));
    MI_REQUIRE(dev >= 0 && dev < 16, "pipeline12_graph_launch: device index %d out of range", dev);
    hipStream_t s = (hipStream_t)stream;
    return ew::resident_launch(dev, s, ew::MAILBOX_WHOLE_FRAME, ew::CAPTURED_UNORDERED, [&](unsigned*, unsigned, bool) {
      MI_HIP(hipGraphLaunch(b->exec, s));
      return 0;
    });
  }
  MI_HIP(hipGraphLaunch(b->exec, (hipStream_t)stream));
  return 0;
}

extern "C" int mi_isp_pipeline12_graph_destroy(void* handle) {
  batch_graph_free(static_cast<BatchGraph*>(handle));
  return 0;
}

extern "C" int mi_isp_pipeline12_pass(const uint8_t* packed, void* out, int H, int W, int ids_format, int pattern,
                                      const float* ccm9, int work_dtype, int out_dtype, float gamma,
                                      float light_adapt, float color_adapt, int pass, void* ws, void* stream) {
  MI_REQUIRE(out && ws, "pipeline12_pass: null pointer");
#ifdef MI_ISP_MEASURE
  const int debug_skip = pass >> 4;      // measurement aid (see tile::Params::debug_skip); MI_ISP_MEASURE builds only
#else
  const int debug_skip = 0;
#endif
  pass &= 15;
  MI_REQUIRE(pass >= 0 && pass <= 3, "pipeline12_pass: pass must be 0..3");
  tile::Params p = {};
  if (int rc = pipeline_params(p, H, W, ids_format, pattern, ccm9, work_dtype, out_dtype, gamma, light_adapt,
                               color_adapt))
    return rc;
  if (int rc = packed_params(p, packed, H, W, 12, ids_format, work_dtype, "pipeline12_pass")) return rc;
  p.dst = out;
  p.vec_store = vec_store_ok(out, W, out_dtype);
  float* fp = static_cast<float*>(ws);
  // (no work image here: an output of another dtype than the work dtype recomputes; debug_skip times the tile kernel)
  void* image = nullptr;
  const int route = debug_skip != 0 ? (int)MI_ISP_ROUTE_RECOMPUTE
                                    : pipeline12_route(p, work_dtype, out, out_dtype, nullptr, &image);
  if (route == MI_ISP_ROUTE_STREAM)
    return pipeline_frame_stream(p, pattern, work_dtype, 1.0f, fp, pass, (hipStream_t)stream);
  if (route == MI_ISP_ROUTE_CACHED_STREAM || route == MI_ISP_ROUTE_CACHED_TILE)
    return pipeline_frame_cached(p, pattern, work_dtype, gamma, 1.0f, fp, pass, (hipStream_t)stream, image, out, out_dtype,
                                 route == MI_ISP_ROUTE_CACHED_STREAM);
  p.fp = fp; p.partials = fp + FP_COUNT; p.part_stride = mi_partial_cap(H, W);
  p.debug_skip = debug_skip & 63;
  static const int epi[4] = {tile::EPI_MINMAX, tile::EPI_STATS, tile::EPI_RH_MINMAX, tile::EPI_RH_STORE};
  const int e = (debug_skip & 64) ? tile::EPI_STORE_MINMAX : epi[pass];   // bit 64: the cached pipeline's pass 0
  return tile::launch(p, work_dtype, pattern, e, (hipStream_t)stream);
}

namespace tile { int occupancy_rggb(int epi); }
extern "C" int mi_isp_debug_occupancy(int epi) { return tile::occupancy_rggb(epi); }
