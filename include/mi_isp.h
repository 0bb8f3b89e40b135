/*
 * mi_isp.h -- C ABI of libmi355_isp.so: the MI355X (gfx950) camera-ISP hot path.
 *
 * This is the drop-in boundary.  The reference (uc-vision/taichi_image) exposes this path as
 * Python functions that launch Taichi-JIT kernels on torch/numpy buffers; there is no FFI in
 * the reference, so each entry point below cites the reference Python function / Taichi
 * kernel it replaces (paths relative to /root/reference/taichi_image/).  A maintainer of the
 * reference would bind these with ctypes exactly as taichi_image_amd/_native.py does
 * (see INTEGRATION.md).
 *
 * Conventions
 *  - every pointer named *_dev is a device (HBM) pointer owned by the caller; the library never
 *    allocates or frees user-visible memory and never synchronises the stream;
 *  - images are C-contiguous, [row][col] or [row][col][3] interleaved RGB;
 *  - `stream` is a hipStream_t (NULL = the default stream); all work is stream-ordered;
 *  - every function returns 0 on success, non-zero on failure; the message for the calling
 *    thread is available from mi_isp_last_error();
 *  - `ws_dev` is a scratch buffer of at least mi_isp_workspace_bytes(H, W) bytes, private to
 *    one in-flight call (use one per stream / per frame in flight).  It must be ZERO-FILLED once
 *    before its first use (hipMemset): the whole-frame kernel of mi_isp_pipeline12_reinhard keeps the
 *    launch count of the workspace and the tagged records of its grid barriers there (a record
 *    counts when its tag equals the launch count + 1, so stale memory must not look like one).
 */
#ifndef MI_ISP_H
#define MI_ISP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types (types.py:12-18 scale factors: u8 255, u16 65535, f16 1, f32 1) */
enum { MI_U8 = 0, MI_U16 = 1, MI_F16 = 2, MI_F32 = 3 };
/* bayer.py:75-79 BayerPattern values */
enum { MI_RGGB = 0, MI_GRBG = 1, MI_GBRG = 2, MI_BGGR = 3 };
/* interpolate.py:9-17 ImageTransform, in declaration order */
enum {
  MI_T_NONE = 0, MI_T_ROTATE_90 = 1, MI_T_ROTATE_180 = 2, MI_T_ROTATE_270 = 3,
  MI_T_TRANSPOSE = 4, MI_T_FLIP_HORIZ = 5, MI_T_FLIP_VERT = 6, MI_T_TRANSVERSE = 7
};
/* camera_isp.py:82-99 loaders */
enum { MI_LOAD_16U = 0, MI_LOAD_32F = 1, MI_LOAD_16F = 2 };

int mi_isp_version(void);
const char* mi_isp_last_error(void);

/* The 4x13x3 integer demosaic weight tables compiled into the kernels (bayer.py:30-55,
 * tap order of bayer.py:15-27).  Host-only; used by the tests to pin the tables. */
int mi_isp_bayer_weights(int32_t out[4 * 13 * 3]);

/* Scratch bytes needed by the calls that take ws_dev, for an H x W frame. */
size_t mi_isp_workspace_bytes(int H, int W);

/* Byte offset inside ws_dev of a uint32 that the whole-frame kernel of mi_isp_pipeline12_reinhard sets to 1
 * when one of its grid barriers timed out (a block of the launch never became resident, e.g. because the
 * caller captured two frames onto parallel branches of one HIP graph).  The frame's output is then invalid.
 * Stays 0 otherwise; hosts that want the check copy these 4 bytes back after synchronising. */
size_t mi_isp_workspace_error_offset(int H, int W);

/* ---- packed.py ------------------------------------------------------------------------ */
/* decode12_kernel (packed.py:92-131): 3 bytes -> two 12-bit values; n_px must be even.
 * scaled: out = cast(f32(v) * f32(scale(out)/4095)).  ids_format: packed.py:37-44 layout. */
int mi_isp_decode12(const uint8_t* enc_dev, void* out_dev, int64_t n_px, int out_dtype,
                    int scaled, int ids_format, void* stream);
/* decode16_kernel (packed.py:135-172): little-endian byte pairs. */
int mi_isp_decode16(const uint8_t* enc_dev, void* out_dev, int64_t n_px, int out_dtype,
                    int scaled, void* stream);
/* encode12_kernel (packed.py:60-89); scaled: v = round_half_away(f32(x) * f32(4095/scale(in))). */
int mi_isp_encode12(const void* values_dev, uint8_t* enc_dev, int64_t n_px, int in_dtype,
                    int scaled, int ids_format, void* stream);

/* ---- camera_isp.py loaders (camera_isp.py:82-99) ---------------------------------------- */
int mi_isp_load_convert(const void* src_dev, void* dst_dev, int64_t n, int mode, int out_dtype,
                        void* stream);

/* ---- bayer.py ------------------------------------------------------------------------- */
/* bayer_to_rgb_kernel (bayer.py:115-190): 13-tap diamond demosaic with border
 * renormalisation; ccm9_host = row-major 3x3 or NULL (host pointer, passed by value). */
int mi_isp_demosaic(const void* cfa_dev, void* rgb_dev, int H, int W, int in_dtype, int out_dtype,
                    int pattern, const float* ccm9_host, void* stream);
/* rgb_to_bayer_kernel (bayer.py:101-112). */
int mi_isp_mosaic(const void* rgb_dev, void* cfa_dev, int H, int W, int dtype, int pattern,
                  void* stream);

/* ---- color/yuv_420.py (the step after the path) ----------------------------------------- */
/* rgb_yuv420_kernel (yuv_420.py:39-66): (H, W, 3) RGB -> (H * 3 / 2, W) planar 4:2:0: rows [0, H) = Y,
 * then two (H/2, W/2) planes, plane 0 = yuv.z, plane 1 = yuv.y.  H, W even.  Reference quirks kept:
 * the matrix sees rgb.bgr, and clamp(0, 1, x) is min(1, x). */
int mi_isp_rgb_to_yuv420(const void* rgb_dev, void* yuv_dev, int H, int W, int in_dtype, int out_dtype,
                         void* stream);
/* 1 if mi_isp_rgb_to_yuv420 runs its vector kernel on these arguments (W % 16 == 0, both pointers 16-byte aligned, a
 * chroma plane of a multiple of 16 bytes), 0 for the kernel of one thread per 2x2 block.  Host only: the pointers'
 * values are read, nothing is launched or dereferenced; the launch asks the same predicate.  Negative with a message
 * for arguments mi_isp_rgb_to_yuv420 refuses. */
int mi_isp_rgb_to_yuv420_is_vector(const void* rgb_dev, const void* yuv_dev, int H, int W, int out_dtype);
/* yuv420_rgb_kernel (yuv_420.py:68-92): the inverse; H, W are the RGB image's. */
int mi_isp_yuv420_to_rgb(const void* yuv_dev, void* rgb_dev, int H, int W, int in_dtype, int out_dtype,
                         void* stream);

/* ---- interpolate.py -------------------------------------------------------------------- */
/* bilinear_kernel (interpolate.py:19-34,59-86): dst (Hd,Wd,3) <- src (Hs,Ws,3);
 * p = (r/scale0, c/scale1), clamp-to-edge taps, out * scale(out)/scale(in). */
int mi_isp_resize_bilinear(const void* src_dev, void* dst_dev, int Hs, int Ws, int Hd, int Wd,
                           float scale0, float scale1, int in_dtype, int out_dtype, void* stream);
/* transform_kernel (interpolate.py:36-54,93-125); dst is (Ws,Hs,3) for rot90/rot270/transpose. */
int mi_isp_transform(const void* src_dev, void* dst_dev, int Hs, int Ws, int dtype, int transform,
                     void* stream);

/* ---- camera_isp.py: rolling metering + tonemap (stateful ISP semantics) ----------------- */
/* metering_kernel + metering_images (camera_isp.py:142-175): stride-subsampled statistics of
 * n_images (H,W,3) images, blended into state9_dev (f32[9]) with weight alpha.
 * images_host: host array of n_images device pointers.
 * One launch for up to 64 images (a grid barrier inside: at most one block per CU, so it needs no more of the chip than
 * any kernel; a barrier that times out sets the workspace's fault word, mi_isp_workspace_check).  MI_ISP_METERING_LAUNCHES=4
 * in the environment selects the four-launch path (bounds pass, finalize, statistics pass, finalize). */
int mi_isp_metering(const void* const* images_host, int n_images, int H, int W, int stride,
                    int dtype, float* state9_dev, float alpha, void* ws_dev, void* stream);
/* The same with the previous state only READ and the new one only WRITTEN (camera_isp.py:172-173 clones the previous
 * state and lets the kernel update the clone; this form needs no copy).  prev9_dev == state9_dev is mi_isp_metering.
 * After a barrier timeout state9_dev holds the previous state. */
int mi_isp_metering_to(const void* const* images_host, int n_images, int H, int W, int stride, int dtype,
                       const float* prev9_dev, float* state9_dev, float alpha, void* ws_dev, void* stream);
/* The two data passes of the same kernel, split so that a cross-GPU reduction can be
 * inserted between them (one process per GPU, see taichi_image_amd/distributed.py):
 *  bounds: raw (min, max) of the subsample                          -> out2_dev  (f32[2])
 *  sums  : given blended bounds, [log_min, log_max, sum_log, sum_gray, sum_r, sum_g, sum_b, n]
 *                                                                    -> out8_dev  (f32[8]) */
int mi_isp_metering_bounds(const void* const* images_host, int n_images, int H, int W, int stride,
                           int dtype, float* out2_dev, void* ws_dev, void* stream);
int mi_isp_metering_sums(const void* const* images_host, int n_images, int H, int W, int stride,
                         int dtype, const float* bounds2_dev, float* out8_dev, void* ws_dev,
                         void* stream);
/* The sharded batch after an all-gather of the ranks' partials (one all-gather per round, then one of these):
 *  combine_bounds: gathered_dev = n_ranks x [min, max] -> bounds2_out_dev = the blended bounds of camera_isp.py:156-157
 *  combine_sums  : gathered_dev = n_ranks x the 8 floats of mi_isp_metering_sums -> state9_dev updated in place
 *                  (camera_isp.py:131-134,164-166), equal to what mi_isp_metering computes over all ranks' images. */
int mi_isp_metering_combine_bounds(const float* gathered_dev, int n_ranks, const float* state9_dev, float alpha,
                                   float* bounds2_out_dev, void* stream);
int mi_isp_metering_combine_sums(const float* gathered_dev, int n_ranks, const float* bounds2_dev, float* state9_dev,
                                 float alpha, void* stream);
/* reinhard_kernel (camera_isp.py:177-218): pass 1 writes p back into image_dev IN PLACE (as the
 * reference does) and reduces max(p); pass 2 writes u8.  transform != NONE applies
 * interpolate.transform (camera_isp.py:403) while storing; out_dev is then the transformed shape. */
int mi_isp_reinhard(void* image_dev, uint8_t* out_dev, int H, int W, int dtype,
                    const float* state9_dev, float gamma, float intensity, float light_adapt,
                    float color_adapt, int transform, void* ws_dev, void* stream);
/* tonemap_reinhard of a list of images straight to planar YUV 4:2:0 (u8, layout of mi_isp_rgb_to_yuv420): the
 * second Reinhard pass (camera_isp.py:215-218) fused with color/yuv_420.py:39-66; equals
 * mi_isp_rgb_to_yuv420(mi_isp_reinhard_batch(...)) without writing and re-reading the u8 RGB images.
 * Like the reference's pass 1 it overwrites the input images.  H even, W % 16 == 0, no orientation transform. */
int mi_isp_reinhard_batch_yuv420(void* const* images_host, uint8_t* const* yuv_outs_host, int n, int H, int W,
                                 int dtype, const float* state9_dev, float gamma, float intensity,
                                 float light_adapt, float color_adapt, void* ws_dev, void* stream);

/* The per-image loop of ISP.tonemap_reinhard / tonemap_linear (camera_isp.py:399-403,409-413) in
 * one call: n images of the same shape, 4 (Reinhard) or 2 (linear) launches in total instead of per
 * image.  images_host / outs_host: host arrays of device pointers. */
int mi_isp_reinhard_batch(void* const* images_host, uint8_t* const* outs_host, int n, int H, int W,
                          int dtype, const float* state9_dev, float gamma, float intensity,
                          float light_adapt, float color_adapt, int transform, void* ws_dev,
                          void* stream);
/* Extension - NOT the reference's semantics: the u8 outputs of mi_isp_reinhard_batch, bit for bit, without overwriting the
 * images with the mapped values (camera_isp.py:211 does overwrite them).  Pass 1 only reduces, pass 2 recomputes p from the
 * untouched image and rounds it to the image dtype as the write-back would have: a third of the two passes' bytes stays
 * where it is.  For callers that drop the images after the tonemap, or want them as loaded. */
int mi_isp_reinhard_batch_keep(const void* const* images_host, uint8_t* const* outs_host, int n_images, int H, int W,
                               int dtype, const float* state9_dev, float gamma, float intensity, float light_adapt,
                               float color_adapt, int transform, void* ws_dev, void* stream);
int mi_isp_linear_batch(const void* const* images_host, uint8_t* const* outs_host, int n, int H,
                        int W, int dtype, const float* state9_dev, float gamma, int transform,
                        void* ws_dev, void* stream);
/* linear_kernel (camera_isp.py:220-227 -> tonemap.py:12-17). */
int mi_isp_linear(const void* image_dev, uint8_t* out_dev, int H, int W, int dtype,
                  const float* state9_dev, float gamma, int transform, void* ws_dev, void* stream);

/* ---- tonemap.py (stateless, per-image statistics) --------------------------------------- */
/* linear_kernel (tonemap.py:27-46). */
int mi_isp_tonemap_linear(const void* src_dev, void* dst_dev, int H, int W, int in_dtype,
                          int out_dtype, float gamma, void* ws_dev, void* stream);
/* reinhard_kernel (tonemap.py:135-168): bounds -> normalise -> metering -> Reinhard -> bounds ->
 * gamma; the f32 `temp` image of the reference is recomputed per pass, never materialised. */
int mi_isp_tonemap_reinhard(const void* src_dev, void* dst_dev, int H, int W, int in_dtype,
                            int out_dtype, float gamma, float intensity, float light_adapt,
                            float color_adapt, void* ws_dev, void* stream);
/* What mi_isp_tonemap_linear / mi_isp_tonemap_reinhard launch on these arguments, from the shape, the dtypes and the
 * pointers' values alone (host only; the launches read the same function).  One group is 8 pixels; a pass whose source
 * and destination are aligned (16 bytes, u8: 8) runs whole waves of 64 whole groups on its straight-line FULL path and the
 * rest - the groups behind the last whole wave, a ragged last group, every group of an unaligned view - on the general
 * one.  out_host[0]: blocks of a storing pass (and of the first bounds pass), [1]: blocks of tonemap_reinhard's
 * statistics and second bounds passes, [2]: FULL groups of a storing pass, [3]: its general groups, a ragged one
 * included.  Non-zero with a message for arguments the tonemaps refuse. */
int mi_isp_tonemap_pass_geometry(int H, int W, int in_dtype, int out_dtype, const void* src_dev, const void* dst_dev,
                                 int64_t out_host[4]);

/* ---- fused hot path ---------------------------------------------------------------------- */
/* ISP.load_packed12 / load_packed16 (camera_isp.py:333-347,371-373,302-315) in one pass over
 * the packed frame: unpack (bits = 12|16) -> demosaic (+ccm) -> [bilinear resize] -> rgb_dev
 * (Hd,Wd,3) of work_dtype (MI_F16 = Camera16, MI_F32 = Camera32).  scale <= 0: no resize
 * (Hd,Wd must equal H,W).  The intermediate CFA / full-resolution RGB are rounded to
 * work_dtype exactly where the reference stores them. */
int mi_isp_load_packed(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits,
                       int ids_format, int pattern, const float* ccm9_host, int work_dtype,
                       int Hd, int Wd, float scale, void* stream);
/* The same, and the image's metering subsample on the way: sub_dev receives rgb[::sub_stride, ::sub_stride] as a dense
 * (ceil(Hd / sub_stride), ceil(Wd / sub_stride), 3) image of work_dtype - what ISP.update_metering reads of every image
 * (camera_isp.py:168-170).  mi_isp_metering(..) on these buffers with stride 1 gives the bits of mi_isp_metering on the
 * images with stride sub_stride (same samples, same order) without the strided gather over the full-size images.  With
 * sub_stride 8 and no resize the subsample is written by the load kernel itself; otherwise by a small gather behind it. */
int mi_isp_load_packed_metered(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits,
                               int ids_format, int pattern, const float* ccm9_host, int work_dtype,
                               int Hd, int Wd, float scale, void* sub_dev, int sub_stride, void* stream);
/* n frames of one size (the cameras of a group: one ISP.load_packed12 / 16 each, camera_isp.py:333-347) in ONE launch
 * per 8 frames - same arithmetic and bits as n calls of mi_isp_load_packed[_metered], without n - 1 launches' dispatch,
 * table build and drain.  packed_host / rgb_host / subs_host: host arrays of n device pointers; subs_host may be NULL (no
 * metering subsamples); frames the streaming kernels do not take are loaded one by one. */
int mi_isp_load_packed_batch(const uint8_t* const* packed_host, void* const* rgb_host, void* const* subs_host, int n,
                             int H, int W, int bits, int ids_format, int pattern, const float* ccm9_host, int work_dtype,
                             int Hd, int Wd, float scale, int sub_stride, void* stream);
/* 1 if mi_isp_load_packed_metered (scale <= 0, 16-byte aligned buffers) writes the subsample from inside the load
 * kernel, 0 if it would need the gather behind it (then the caller may as well let mi_isp_metering gather). */
int mi_isp_load_packed_metered_is_fused(int H, int W, int bits, int ids_format, int work_dtype, int sub_stride);
/* 1 if mi_isp_load_packed can fuse a resize by `scale` (its LDS tile holds the source region of a
 * 64x16 destination tile for scale >= ~0.39, any upscale); otherwise demosaic at full size and
 * call mi_isp_resize_bilinear.
 * This is the bound of the tile kernel, which takes MI_F32 and the frames the streaming kernel
 * does not.  MI_F16 frames that the streaming kernel takes - 12 bit in the standard layout, W a
 * multiple of 8, H >= 4, a packed frame below 1 GiB, an output that is 8-byte aligned and smaller
 * than 4 GiB - accept ANY positive scale, bit-exact like the others (the streaming resize keeps
 * whole source rows, so no scale outgrows it; below 1/3 it skips source rows, below 1/4 its bands
 * end on ragged destination columns).  Every other call with a scale outside the bound returns
 * non-zero and launches nothing. */
int mi_isp_load_packed_scale_supported(float scale);

/* ---- sensor black and white levels ------------------------------------------------------------------------------------
 * A raw code v at CFA site s = (row & 1) * 2 + (col & 1) of the raw frame (whatever the pattern) decodes to
 *   cast_work(f32(max(v - black[s], 0)) * k[s]),  k[s] = f32(S / (white - black[s])) (computed in double, rounded once),
 * S the work dtype's scale; no upper clamp (as the unscaled decode).  black[s] = 0 with the container's full scale as
 * white (4095 packed-12, 65535 packed-16 / u16) is bit-identical to the entry points without levels.  Levels must hold
 * 0 <= black[s] < white <= 2^bits - 1.  A NULL levels pointer means "no levels": exactly the call without _levels.
 * One black level for every site is folded into the packed-12 kernels' decode table; four distinct ones are applied in
 * registers. */
typedef struct { int32_t black[4]; int32_t white; } mi_isp_levels;
int mi_isp_load_packed_levels(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits, int ids_format,
                              int pattern, const float* ccm9_host, int work_dtype, int Hd, int Wd, float scale,
                              const mi_isp_levels* levels_host, void* stream);
int mi_isp_load_packed_metered_levels(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits, int ids_format,
                                      int pattern, const float* ccm9_host, int work_dtype, int Hd, int Wd, float scale,
                                      void* sub_dev, int sub_stride, const mi_isp_levels* levels_host, void* stream);
int mi_isp_load_packed_batch_levels(const uint8_t* const* packed_host, void* const* rgb_host, void* const* subs_host,
                                    int n, int H, int W, int bits, int ids_format, int pattern, const float* ccm9_host,
                                    int work_dtype, int Hd, int Wd, float scale, int sub_stride,
                                    const mi_isp_levels* levels_host, void* stream);
/* mi_isp_load_convert with levels (mode MI_LOAD_16U only, 16-bit codes, row-major H x W frame for the sites): as that
 * loader divides - cast_work(f32(max(v - black[s], 0)) / f32(white - black[s])) - instead of multiplying by k[s], so
 * that black 0 / white 65535 keeps its bits. */
int mi_isp_load_convert_levels(const void* src_dev, void* dst_dev, int H, int W, int mode, int out_dtype,
                               const mi_isp_levels* levels_host, void* stream);

/* ---- lens shading (flat-field / vignetting correction) ----------------------------------------------------------------
 * A gain grid of f32 on the device: sites = 1 (one grid for every site) or 4 (one per CFA site s = (row & 1) * 2 +
 * (col & 1) of the raw frame, whatever the pattern), each grid_h x grid_w row-major, 2 <= grid_h, grid_w <= 64; the
 * gains must be finite and within [0, 16] (the Python layer checks them; the library reads them on the device only).
 * Node (i, j) sits at raw pixel (i * (H-1)/(grid_h-1), j * (W-1)/(grid_w-1)).  For raw pixel (r, c), every step one f32
 * operation rounded to nearest, none contracted:
 *   sy = f32((grid_h - 1) / (H - 1)), sx = f32((grid_w - 1) / (W - 1))   (in double on the host; 0 for H or W == 1)
 *   v = f32(r) * sy; i = min(floor(v), grid_h - 2); ty = v - f32(i)    (u, j, tx the same along the columns)
 *   a = G[i][j] + ty * (G[i+1][j] - G[i][j]);  b = G[i][j+1] + ty * (G[i+1][j+1] - G[i][j+1]);  g = a + tx * (b - a)
 *   cfa = cast_work(x * g), x the f32 value the loader rounds to the work dtype without shading (with levels included).
 * A grid of ones gives the bits of the call without shading.  The _shading twins take both a levels and a shading
 * pointer; either may be NULL, and NULL / NULL is exactly the plain call.  They accept every case the plain entry point
 * accepts and take the same path (mi_isp_load_packed_metered_is_fused, mi_isp_load_packed_scale_supported). */
typedef struct { const float* gains_dev; int32_t sites; int32_t grid_h, grid_w; } mi_isp_shading;
int mi_isp_load_packed_shading(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits, int ids_format,
                               int pattern, const float* ccm9_host, int work_dtype, int Hd, int Wd, float scale,
                               const mi_isp_levels* levels_host, const mi_isp_shading* shading_host, void* stream);
int mi_isp_load_packed_metered_shading(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits, int ids_format,
                                       int pattern, const float* ccm9_host, int work_dtype, int Hd, int Wd, float scale,
                                       void* sub_dev, int sub_stride, const mi_isp_levels* levels_host,
                                       const mi_isp_shading* shading_host, void* stream);
int mi_isp_load_packed_batch_shading(const uint8_t* const* packed_host, void* const* rgb_host, void* const* subs_host,
                                     int n, int H, int W, int bits, int ids_format, int pattern, const float* ccm9_host,
                                     int work_dtype, int Hd, int Wd, float scale, int sub_stride,
                                     const mi_isp_levels* levels_host, const mi_isp_shading* shading_host, void* stream);
/* mi_isp_load_convert with levels and / or shading on a row-major H x W frame: levels need MI_LOAD_16U (as
 * mi_isp_load_convert_levels); shading takes every mode, x being the f32 value the mode converts. */
int mi_isp_load_convert_shading(const void* src_dev, void* dst_dev, int H, int W, int mode, int out_dtype,
                                const mi_isp_levels* levels_host, const mi_isp_shading* shading_host, void* stream);
/* ---- defective pixel correction (hot, stuck or dead sites) -------------------------------------------------------------
 * A defect map of one H x W raw frame: n (row, col) int32 pairs on the device and a bit mask of H rows x ceil(W / 32)
 * uint32 words (bit (col & 31) of word row * ceil(W / 32) + (col >> 5) set for every listed site).  x(q) is the
 * work-dtype value the loader gives raw pixel q (levels and shading included).  A listed site (r, c) reads
 * y = cast_work(((x1 + x2) + x3 + x4) / f32(n)) over the candidates (r-2,c), (r+2,c), (r,c-2), (r,c+2) that are inside
 * the frame and not listed - or, if none is, the four diagonals at distance 2 under the same rule - summed in that
 * order in f32, the division correctly rounded; with no candidate y = x(r, c).  Everything downstream (demosaic, ccm,
 * resize, metering subsample) reads y at listed sites.  The fix-ups run after the load on the same stream:
 *  - mi_isp_defects_fix_packed recomputes, from the packed frame, the n_outputs output pixels listed in outputs_dev
 *    (indices row * Wd + col of the loader's output, unique; every pixel whose value reads a listed site must be
 *    listed - its 5 x 5 demosaic footprint, through the bilinear taps with scale > 0) and the metering subsample
 *    entries among them (sub_dev, stride sub_stride; NULL: none).  The other arguments are the loader's.
 *  - the _batch twin does it for n frames in one launch per 32 frames with outputs; defects_host[i] may be NULL.
 *  - mi_isp_defects_fix_cfa corrects a work-dtype (MI_F16 / MI_F32) H x W CFA in place (load_16u / 16f / 32f).
 * Host-side checks: NULL pointers with n > 0, negative counts, output counts beyond Hd x Wd. */
typedef struct { const int32_t* coords_dev; int32_t n; const uint32_t* mask_dev; } mi_isp_defects;
int mi_isp_defects_fix_packed(const uint8_t* packed_dev, void* rgb_dev, int H, int W, int bits, int ids_format,
                              int pattern, const float* ccm9_host, int work_dtype, int Hd, int Wd, float scale,
                              void* sub_dev, int sub_stride, const mi_isp_levels* levels_host,
                              const mi_isp_shading* shading_host, const mi_isp_defects* defects_host,
                              const int32_t* outputs_dev, int n_outputs, void* stream);
int mi_isp_defects_fix_packed_batch(const uint8_t* const* packed_host, void* const* rgb_host, void* const* subs_host,
                                    int n, int H, int W, int bits, int ids_format, int pattern, const float* ccm9_host,
                                    int work_dtype, int Hd, int Wd, float scale, int sub_stride,
                                    const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                                    const mi_isp_defects* const* defects_host, const int32_t* const* outputs_host,
                                    const int32_t* n_outputs_host, void* stream);
int mi_isp_defects_fix_cfa(void* cfa_dev, int H, int W, int work_dtype, const mi_isp_defects* defects_host,
                           void* stream);
/* ---- lens distortion correction (geometric undistortion, a bilinear remap) ------------------------------------------
 * OpenCV's pinhole model: K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] of the distorted source (fx, fy > 0, no skew),
 * new_K = [[fx', 0, cx'], [0, fy', cy'], [0, 0, 1]] of the undistorted output, dist in OpenCV order: (k1, k2, p1, p2),
 * (k1, k2, p1, p2, k3) or the rational (k1, k2, p1, p2, k3, k4, k5, k6) (n_dist 4, 5 or 8; unused entries ignored).
 * Every value must be finite.  The library rounds each once from double to f32, and ifx' = 1 / fx', ify' = 1 / fy' are
 * computed in double and rounded.  Output pixel (r, c) of an Hd x Wd image at output scale (s0, s1) (1 without a
 * resize; no half-pixel offset) reads, every step one f32 operation rounded to nearest, left to right, never contracted:
 *   u = f32(c) / s1, v = f32(r) / s0;  x = (u - cx') * ifx', y = (v - cy') * ify';  r2 = x*x + y*y
 *   num = 1 + r2*(k1 + r2*(k2 + r2*k3));  radial = num, or rational: num / (1 + r2*(k4 + r2*(k5 + r2*k6)))
 *   xd = x*radial + (2*p1)*x*y + p2*(r2 + 2*x*x);  yd = y*radial + p1*(r2 + 2*y*y) + (2*p2)*x*y
 *   us = fx*xd + cx, vs = fy*yd + cy
 * and samples the H x W source RGB at (us, vs): border MI_BORDER_CONSTANT gives 0 outside [0, H-1] x [0, W-1] (and for
 * NaN); MI_BORDER_REPLICATE clamps vs and us into that range first (NaN to 0).  i = floor(vs), fr = vs - f32(i), j and fc
 * the same; taps i, i+1, j, j+1 with the +1 taps clamped to the frame; mix(x, y, a) = x*(1-a) + y*a over rows, then
 * columns, then * scale(out) / scale(in) and the cast - the bilinear resize's arithmetic (mi_isp_resize_bilinear).
 *  - mi_isp_undistort: one image; mi_isp_undistort_batch: n images of one geometry, each with its own lens (one launch
 *    per 32 images and border mode); lens_host[i] must not be NULL.
 *  - mi_isp_remap: the table form - map_dev holds Hd x Wd (us, vs) f32 pairs (OpenCV's map_x / map_y interleaved),
 *    8-byte aligned - sampled by the same rule.
 * Host-side checks (error text names "lens"): NULL pointers, shapes, dtypes, border, n_dist, non-finite values,
 * non-positive focal lengths or output scales. */
enum { MI_BORDER_CONSTANT = 0, MI_BORDER_REPLICATE = 1 };
typedef struct {
  double fx, fy, cx, cy;                  /* K */
  double new_fx, new_fy, new_cx, new_cy;  /* new_K */
  double dist[8];                         /* k1, k2, p1, p2, k3, k4, k5, k6 */
  int32_t n_dist;                         /* 4, 5 or 8 */
  int32_t border;                         /* MI_BORDER_* */
} mi_isp_lens;
int mi_isp_undistort(const void* src_dev, void* dst_dev, int H, int W, int Hd, int Wd, float s0, float s1, int in_dtype,
                     int out_dtype, const mi_isp_lens* lens_host, void* stream);
int mi_isp_undistort_batch(const void* const* src_host, void* const* dst_host, int n, int H, int W, int Hd, int Wd,
                           float s0, float s1, int in_dtype, int out_dtype, const mi_isp_lens* const* lens_host,
                           void* stream);
int mi_isp_remap(const void* src_dev, void* dst_dev, const float* map_dev, int H, int W, int Hd, int Wd, int in_dtype,
                 int out_dtype, int border, void* stream);
/* ---- automatic white balance (gray world; DESIGN.md 3, "Auto white balance") ----------------------------------------
 * Statistics: a quad is the 2x2 block at raw rows 2a, 2a+1 and columns 2b, 2b+1, sampled when a % stride == 0 and
 * b % stride == 0.  x of each pixel is the f32 value the loader rounds to the work dtype without shading (the decode and
 * levels of a packed source; the conversion of mi_isp_load_convert_shading for a CFA), xs = f32(x * g) with g the
 * pixel's gain under shading_host (1 for NULL).  A quad is kept when all four x < clip and max(x) >= floor (f32 compares:
 * a NaN quad drops out); it adds u64(rint(min(max(xs, 0), 2^15) * 2^24)) to P[s] of each site s = (row & 1) * 2 +
 * (col & 1), and 1 to n.  pending_dev holds P[0..3], n as u64 and is added to with integer atomics (exact, order-free).
 *  - mi_isp_awb_stats_packed: n packed frames (12 or 16 bits, as mi_isp_load_packed_batch_shading) in one launch per 32.
 *  - mi_isp_awb_stats_cfa: one H x W CFA of mode MI_LOAD_16U / 32F / 16F (levels with MI_LOAD_16U only).
 * Update: gathered_dev holds world rows of 5 i64 (P, n; the ranks' pending rows, or pending_dev itself); their sum with
 * n == 0 changes nothing, otherwise in f64: m_s = (P_s * 2^-24) / n, R = m of the pattern's red site, G = the mean of
 * its two green sites' m, B likewise; S = c + t' * (S_prev - c) with t' = t after the first update (state_dev[3] != 0)
 * and 0 before; g_R = f32(clamp(S_G / S_R, 1/8, 8)), g_B the same, g_G = 1, a gain whose S_c or S_G is <= 0 kept.
 * pending_dev is zeroed.  state_dev: S_R, S_G, S_B, valid (f64); gains_dev: g_R, g_G, g_B (f32).
 * Both the update and mi_isp_awb_rebuild write effective_dev = E[s][i][j] = f32(U[s'][i][j] * g_colour(s)), 4 x Gh x Gw
 * f32, with U the user's grid (s' = s for 4 sites, 0 for 1) or a 2 x 2 grid of ones for NULL.  One workgroup each.
 * Host-side checks (error text names "awb"): NULL pointers, shapes, bits, modes, levels, grids, stride >= 1,
 * 0 < floor < clip (finite), world >= 1, pattern, a finite t. */
int mi_isp_awb_stats_packed(const uint8_t* const* packed_host, int n, int H, int W, int bits, int ids_format,
                            const mi_isp_levels* levels_host, const mi_isp_shading* shading_host, float clip,
                            float floor_, int stride, void* pending_dev, void* stream);
int mi_isp_awb_stats_cfa(const void* cfa_dev, int H, int W, int mode, const mi_isp_levels* levels_host,
                         const mi_isp_shading* shading_host, float clip, float floor_, int stride, void* pending_dev,
                         void* stream);
int mi_isp_awb_update(const int64_t* gathered_dev, int world, void* pending_dev, int pattern, double t, double* state_dev,
                      float* gains_dev, const mi_isp_shading* user_host, float* effective_dev, void* stream);
int mi_isp_awb_rebuild(int pattern, float* gains_dev, const mi_isp_shading* user_host, float* effective_dev,
                       void* stream);
/* ---- raw noise reduction ("Raw noise reduction") -----------------------------------------------------
 * An edge-preserving bilateral filter over same-site neighbours, adapted to the sensor's noise model.  x(p) of raw pixel p
 * is the f32 value the loader computes before shading and the cast (the decode with or without levels, load_16u's true
 * division, the value load_16f / load_32f convert).  For p = (r, c), T(p) = the pixels q = (r + 2i, c + 2j), |i|, |j| <=
 * radius, (i, j) != (0, 0), inside the frame and not set in the defect mask:
 *   var = gain * max(x(p), 0) + read_noise^2;  k = 1 / (2 strength^2 var)
 *   w(q) = exp(-(x(q) - x(p))^2 k - (i^2 + j^2) / (2 spatial_sigma^2));  y = (x(p) + sum w(q) x(q)) / (1 + sum w(q))
 *   cfa = cast_work(y * g(p))      (g the lens shading gain of shading_host, 1 for NULL)
 * in f32 with the hardware exp and rcp: within one unit of the work dtype of an f64 evaluation (f32: or 1e-5 relative).
 * The noise model is in the units of x.  Source kinds: MI_RAW_PACKED12 (ids_format selects the IDS layout) and
 * MI_RAW_PACKED16 with levels as mi_isp_load_packed_levels (H and W even); MI_RAW_16U / 32F / 16F the modes of
 * mi_isp_load_convert_shading (levels with MI_RAW_16U only).  Only the mask of a defect map is read.  The output is an
 * H x W work-dtype CFA (MI_F16 / MI_F32) that must not overlap the source.
 *  - mi_isp_denoise_raw_batch: n frames of one geometry, defects_host NULL or one map (or NULL) per frame; one launch per
 *    32 frames.
 *  - mi_isp_denoise_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "denoise"): radius 1 or 2, gain finite >= 0, read_noise, strength
 * and spatial_sigma finite > 0, shapes, dtypes, kinds, levels, grids, NULL pointers. */
typedef struct { float gain, read_noise, strength, spatial_sigma; int32_t radius; } mi_isp_denoise;
enum { MI_RAW_PACKED12 = 0, MI_RAW_PACKED16 = 1, MI_RAW_16U = 2, MI_RAW_32F = 3, MI_RAW_16F = 4 };
int mi_isp_denoise_raw(const void* src_dev, void* cfa_dev, int H, int W, int src_kind, int ids_format, int work_dtype,
                       const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                       const mi_isp_defects* defects_host, const mi_isp_denoise* denoise_host, void* stream);
int mi_isp_denoise_raw_batch(const void* const* src_host, void* const* cfa_host, int n, int H, int W, int src_kind,
                             int ids_format, int work_dtype, const mi_isp_levels* levels_host,
                             const mi_isp_shading* shading_host, const mi_isp_defects* const* defects_host,
                             const mi_isp_denoise* denoise_host, void* stream);
int mi_isp_denoise_cfa(const void* in_dev, void* out_dev, int H, int W, int dtype, const mi_isp_denoise* denoise_host,
                       void* stream);
/* ---- highlight reconstruction ("Highlight reconstruction") ----------------------------------------------
 * Clipped raw pixels rebuilt from their neighbours' white-balanced values, in f32 with one rounding per operation: the
 * output is the contract's bit for bit.  x(p) is the value raw noise reduction filters (above); s(p) = (row & 1) * 2 +
 * (col & 1); w[s] the balance gain (wb[0..2] = R, G, B; wb_dev, when not NULL, 3 f32 on the device that override wb and
 * are read by the kernel) of the site's colour under `pattern`; b(q) = x(q) * w[s(q)]; t = clip.
 *   MI_HIGHLIGHTS_REBUILD: p with x(p) >= t: for each of its two tap groups (R / B site: (r-1,c) (r,c-1) (r,c+1) (r+1,c),
 *     then (r-1,c-1) (r-1,c+1) (r+1,c-1) (r+1,c+1); G site: (r,c-1) (r,c+1), then (r-1,c) (r+1,c)) with n >= 1 taps inside
 *     the frame and not set in the defect mask, m = (the sum of their b in that order) / n; e = the larger m; when
 *     e > b(p): y = max(x(p), e / w[s(p)]).  Every other pixel: y = x(p).
 *   MI_HIGHLIGHTS_CLIP: y = min(x(p), (t * min(w)) / w[s(p)]).
 *   cfa = cast_work(y * g(p))      (g the lens shading gain of shading_host, 1 for NULL)
 * Source kinds, levels, grids, defect maps and outputs as mi_isp_denoise_raw(_batch).  out_f32_plain != 0: the output is
 * the H x W f32 y itself, without gain or cast (shading_host must be NULL), for mi_isp_denoise_raw_batch to take as
 * MI_RAW_32F.
 *  - mi_isp_highlights_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "highlights"): the mode, clip finite > 0, host gains finite > 0
 * (device gains are the caller's), the pattern, shapes, dtypes, kinds, levels, grids, NULL pointers.  n == 0 and
 * H * W == 0 are successful no-ops. */
typedef struct { int32_t mode; float clip; float wb[3]; const float* wb_dev; } mi_isp_highlights;
enum { MI_HIGHLIGHTS_REBUILD = 0, MI_HIGHLIGHTS_CLIP = 1 };
int mi_isp_highlights_raw(const void* src_dev, void* cfa_dev, int H, int W, int src_kind, int ids_format, int work_dtype,
                          int pattern, const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                          const mi_isp_defects* defects_host, const mi_isp_highlights* highlights_host, int out_f32_plain,
                          void* stream);
int mi_isp_highlights_raw_batch(const void* const* src_host, void* const* cfa_host, int n, int H, int W, int src_kind,
                                int ids_format, int work_dtype, int pattern, const mi_isp_levels* levels_host,
                                const mi_isp_shading* shading_host, const mi_isp_defects* const* defects_host,
                                const mi_isp_highlights* highlights_host, int out_f32_plain, void* stream);
int mi_isp_highlights_cfa(const void* in_dev, void* out_dev, int H, int W, int dtype, int pattern,
                          const mi_isp_highlights* highlights_host, void* stream);
/* ---- dynamic defects ("Dynamic defects") ----------------------------------------------------------------------
 * Defective-pixel correction without a map, whatever the Bayer pattern.  x(p) is the f32 value a loader computes before
 * shading and the cast.  The taps of p = (r, c) are its eight same-site neighbours, in this order:
 *   q0 .. q7 = (r-2,c-2) (r-2,c) (r-2,c+2) (r,c-2) (r,c+2) (r+2,c-2) (r+2,c) (r+2,c+2)
 * A tap is kept when it is inside the frame, not listed in the frame's defect mask and its x is finite; n counts them.
 * With k = tolerate (0 or 1), hi / lo the (k+1)-th largest / smallest kept tap and T(v) = threshold + slope max(v, 0)
 * (every operation one f32 rounding, never contracted):
 *   p is a candidate when n >= 2k + 1, x(p) is finite and p is not listed
 *   p is hot  when it is a candidate, hot  != 0 and x(p) - hi > T(hi)
 *   p is dead when it is a candidate, dead != 0 and lo - x(p) > T(lo)
 *   of the pairs (q1,q6) (q3,q4) (q0,q7) (q2,q5) with both taps kept, the one of the smallest |a - b| (the earlier on a
 *   tie) gives m = (a + b) 0.5; a hot pixel gets y = min(m, hi), or hi without such a pair; a dead one y = max(m, lo), or
 *   lo; every other pixel (a listed one too) keeps y = x(p), the same bits
 *   cfa = cast_work(y * g(p))      (g the lens shading gain of shading_host, 1 for NULL)
 * Source kinds, levels, grids, defect maps and outputs as mi_isp_highlights_raw(_batch), out_f32_plain included (the
 * output is the H x W f32 y itself; shading_host must be NULL).  flags (flags_host: one pointer per frame), when not NULL,
 * takes H rows of (W + 31) / 32 u32 words on the device in the layout of mi_isp_defects.mask_dev: bit c & 31 of word
 * c >> 5 is set iff pixel (r, c) was hot or dead; every word is written.
 *  - mi_isp_dynamic_defects_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "dynamic defects"): threshold finite > 0, slope finite >= 0,
 * tolerate 0 or 1, hot or dead set, shapes, dtypes, kinds, levels, grids, NULL pointers.  n == 0 and H * W == 0 are
 * successful no-ops. */
typedef struct { float threshold, slope; int32_t tolerate, hot, dead; } mi_isp_dynamic_defects;
int mi_isp_dynamic_defects_raw(const void* src_dev, void* cfa_dev, int H, int W, int src_kind, int ids_format,
                               int work_dtype, const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                               const mi_isp_defects* defects_host, const mi_isp_dynamic_defects* dynamic_host,
                               int out_f32_plain, void* stream, uint32_t* flags_dev);
int mi_isp_dynamic_defects_raw_batch(const void* const* src_host, void* const* cfa_host, int n, int H, int W, int src_kind,
                                     int ids_format, int work_dtype, const mi_isp_levels* levels_host,
                                     const mi_isp_shading* shading_host, const mi_isp_defects* const* defects_host,
                                     const mi_isp_dynamic_defects* dynamic_host, int out_f32_plain, void* stream,
                                     uint32_t* const* flags_host);
int mi_isp_dynamic_defects_cfa(const void* in_dev, void* out_dev, int H, int W, int dtype,
                               const mi_isp_dynamic_defects* dynamic_host, void* stream, uint32_t* flags_dev);
/* ---- green equalisation ("Green equalisation") ----------------------------------------------------------------
 * Correction of the imbalance between the two green sites of a Bayer quad (Gr beside red, Gb beside blue).  x(p) is the
 * f32 value a loader computes before shading and the cast.  p = (r, c) is a green site iff ((r + c) & 1) == gp, gp = 1
 * for MI_RGGB and MI_BGGR and 0 for MI_GRBG and MI_GBRG (`pattern`: the demosaic pattern).  The taps of a green p, in
 * this order:
 *   radius 1: group O (the other phase) (r-1,c-1) (r-1,c+1) (r+1,c-1) (r+1,c+1)
 *             group S (the own phase)   (r,c) (r-2,c) (r,c-2) (r,c+2) (r+2,c)
 *   radius 2: group O (r+dy, c+dx) for dy in (-3,-1,1,3), for dx in (-3,-1,1,3), row-major: 16 taps
 *             group S (r,c), then (r+dy, c+dx) for dy in (-2,0,2), for dx in (-2,0,2), without (0,0), row-major: 9 taps
 * A tap is kept when it is inside the frame, not listed in the frame's defect mask and its x is finite.  For each group:
 * the f32 sum of the kept taps in the listed order, starting from the first kept tap; their count n; their maximum and
 * their minimum.  Every operation is one f32 rounding, in the order written, never contracted; the divisions are IEEE:
 *   O = sumO / f32(nO)        S = sumS / f32(nS)        d = O - S
 *   lim = threshold + slope * max(O, S)                   e = edge * lim
 *   apply  iff  nO >= 1  and  |d| <= lim  and  maxO - minO <= e  and  maxS - minS <= e     (a NaN makes a comparison false)
 *   y = x(p) + (f32(strength) * 0.5f) * d      if apply
 *   y = x(p), the same bits                    otherwise
 *   cfa = cast_work(y * g(p))      (g the lens shading gain of shading_host, 1 for NULL)
 * A site that is not green, a listed defect (the fix-up replaces it afterwards) and a pixel whose x(p) is not finite keep
 * x(p), the same bits.
 * Source kinds, levels, grids, defect maps and outputs as mi_isp_highlights_raw(_batch), out_f32_plain included (the
 * output is the H x W f32 y itself; shading_host must be NULL).
 *  - mi_isp_green_equalize_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "green equalize"): threshold, slope and edge finite >= 0, strength
 * in [0, 1], radius 1 or 2, pattern, shapes, dtypes, kinds, levels, grids, NULL pointers.  n == 0 and H * W == 0 are
 * successful no-ops. */
typedef struct { float threshold, slope, strength; int32_t radius; float edge; } mi_isp_green_equalize;
int mi_isp_green_equalize_raw(const void* src_dev, void* cfa_dev, int H, int W, int src_kind, int ids_format, int work_dtype,
                              int pattern, const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                              const mi_isp_defects* defects_host, const mi_isp_green_equalize* green_host,
                              int out_f32_plain, void* stream);
int mi_isp_green_equalize_raw_batch(const void* const* src_host, void* const* cfa_host, int n, int H, int W, int src_kind,
                                    int ids_format, int work_dtype, int pattern, const mi_isp_levels* levels_host,
                                    const mi_isp_shading* shading_host, const mi_isp_defects* const* defects_host,
                                    const mi_isp_green_equalize* green_host, int out_f32_plain, void* stream);
int mi_isp_green_equalize_cfa(const void* in_dev, void* out_dev, int H, int W, int dtype, int pattern,
                              const mi_isp_green_equalize* green_host, void* stream);
/* ---- frame statistics ("Frame statistics") ---------------------------------------------------------------
 * Exposure and focus measurements of raw frames: a read-only side output, exact in integers (the result depends neither
 * on the launch geometry nor on the order of the atomics).  x(p) is the f32 value a loader computes before shading, AWB
 * gain and the cast (levels applied where the source has them); H and W are even.  Pixel p = (r, c) is valid when it is
 * inside the frame, not listed in the frame's defect mask and x(p) > -inf (a NaN and -inf drop out).  For a valid pixel:
 *   v = i32(rint(min(max(x, 0), 1) * 65536))   (one exact f32 product, ties to even)      site s = (r & 1) * 2 + (c & 1)
 *   clipped iff x >= f32(clip)                  dark iff x <= f32(dark)
 *   zone (i, j) = (((r >> 1) * zones_h) / (H / 2), ((c >> 1) * zones_w) / (W / 2))   (integer divisions; a quad is never
 *   split; zones_h <= H / 2 and zones_w <= W / 2, so no zone is empty)
 * One frame's result is one contiguous buffer of mi_isp_statistics_words() int64, which the entry points clear on the
 * stream themselves (what it held before does not matter):
 *   Z[zones_h][zones_w][4][4]   per zone and site, over its valid pixels: their count, the sum of v, the clipped, the dark
 *   F[zones_h][zones_w][2]      per zone: the sum of L * L and the count, over the valid green pixels p (((r + c) & 1) == gp,
 *                               gp = 1 for MI_RGGB and MI_BGGR, 0 for MI_GRBG and MI_GBRG; `pattern`: the demosaic pattern)
 *                               whose four taps (r - 2, c), (r + 2, c), (r, c - 2), (r, c + 2) are valid, p and the taps
 *                               all with x < f32(clip) (a clipped plateau's rim is not detail):  L = 4 v(p) - sum of v(taps)
 *   Hist[4][256]                per site: every valid pixel adds 1 to bin min(v >> 8, 255)
 * |L| <= 2^18, so the sum of L * L stays inside an int64 for H * W <= 2^26; larger frames are refused.
 * Source kinds, ids_format, levels and defect maps as mi_isp_highlights_raw(_batch); there is no shading argument: the
 * statistics describe the sensor.
 *  - mi_isp_statistics_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels), with an optional defect map.
 *  - mi_isp_statistics_words (host only): the int64 count per frame, zones_h * zones_w * 18 + 1024; -1 for bad zones.
 *  - mi_isp_statistics_geometry (host only): {tile rows, tile columns, zone cells of a block's LDS table, the largest
 *    number of consecutive tiles a block takes}.  mi_isp_statistics_strip (host only): the consecutive tiles a block takes
 *    in ONE launch of n frames, 1 <= n <= 32 (a call of more frames is launches of 32 and one of the rest, each with its
 *    own strip); -1 on an error.  A block whose tiles span more zone cells than the table holds adds to global memory
 *    directly; mi_isp_statistics_direct_blocks (host only) counts such blocks per frame for one launch of n frames, 0 <= n
 *    <= 32 (-1 on an error).
 * Host-side checks before any launch (error text names "statistics"): zones 1 .. 32 each and no larger than the quad
 * grid, clip finite > 0, dark finite >= 0 and < clip, pattern, odd H or W, H * W > 2^26, more than 65535 tile rows, kinds, levels, NULL pointers, an
 * output that is not aligned to 8 bytes.  n == 0 and H * W == 0 are successful no-ops. */
typedef struct { int32_t zones_h, zones_w; float clip, dark; } mi_isp_statistics;
int64_t mi_isp_statistics_words(const mi_isp_statistics* statistics_host);
int mi_isp_statistics_geometry(int32_t out[4]);
int mi_isp_statistics_strip(int n, int H, int W);
int mi_isp_statistics_direct_blocks(int n, int H, int W, const mi_isp_statistics* statistics_host);
int mi_isp_statistics_raw(const void* src_dev, int64_t* out_dev, int H, int W, int src_kind, int ids_format, int pattern,
                          const mi_isp_levels* levels_host, const mi_isp_defects* defects_host,
                          const mi_isp_statistics* statistics_host, void* stream);
int mi_isp_statistics_raw_batch(const void* const* src_host, int64_t* const* out_host, int n, int H, int W, int src_kind,
                                int ids_format, int pattern, const mi_isp_levels* levels_host,
                                const mi_isp_defects* const* defects_host, const mi_isp_statistics* statistics_host,
                                void* stream);
int mi_isp_statistics_cfa(const void* cfa_dev, int64_t* out_dev, int H, int W, int dtype, int pattern,
                          const mi_isp_defects* defects_host, const mi_isp_statistics* statistics_host, void* stream);
/* ---- directional demosaic ("Directional demosaic") --------------------------------------------------------
 * A direction-adaptive alternative to mi_isp_demosaic's 13-tap filter, in f32 with one rounding per operation, in the
 * order written, never contracted: the output is the contract's bit for bit.  X(r, c) is the f32 value of the H x W CFA
 * in the work dtype (H, W even and >= 2), extended over the plane by the mirror that does not repeat the edge sample:
 * index i folds with period 2 (n - 1), -1 -> 1, n -> n - 2, repeatedly for small n, which keeps the Bayer phase.  Every
 * quantity is defined on that plane.
 *   1. eh = (X(r,c-1) + X(r,c+1)) * 0.5 + ((X(r,c) + X(r,c)) - (X(r,c-2) + X(r,c+2))) * 0.25; ev the same along the column.
 *      Red or blue site: GH = eh, GV = ev, CH = X - eh, CV = X - ev.  Green site: CH = eh - X, CV = ev - X.
 *   2. DH(r,c) = |CH(r,c) - CH(r,c+2)|, DV(r,c) = |CV(r,c) - CV(r+2,c)|.  dH(r,c) = DH(r-2,c) + DH(r-2,c+2) + DH(r-1,c+1)
 *      + 3 * DH(r,c) + 3 * DH(r,c+2) + DH(r+1,c+1) + DH(r+2,c) + DH(r+2,c+2), accumulated in that order; dV is its
 *      transpose (weights, window and order).  A site is horizontal when dV >= dH.
 *   3. Red or blue site: G = GH when horizontal, else GV.
 *   4. Green site, K the chroma of its row neighbours: K = X + ((K(r,c-1) - G(r,c-1)) + (K(r,c+1) - G(r,c+1))) * 0.5; the
 *      other chroma the same from the neighbours above and below.
 *   5. Red or blue site: d = (RB(r,c-1) + RB(r,c+1)) * 0.5 when horizontal, else the same along the column, RB = R - B of
 *      the green site from step 4.  Blue site: R = X + d.  Red site: B = X - d.
 *   6. mi_isp_demosaic's epilogue: the optional matrix as (m0 * r + m1 * g) + m2 * b, clamp01, * scale(out), the cast.
 * An output pixel reads X over rows r - 4 .. r + 8 and columns c - 4 .. c + 8.
 *  - mi_isp_demosaic_directional_cfa: a normalised CFA of in_dtype MI_F16 / MI_F32; out_dtype any of MI_U8 .. MI_F32.
 *  - mi_isp_demosaic_directional_raw_batch: n raw frames of one geometry (source kinds, ids_format, levels and grids as
 *    mi_isp_denoise_raw_batch; levels_host and shading_host may each be NULL); X is the loaders' CFA cast_work(x * g), the
 *    output is in the work dtype.  One launch per 32 frames.
 *  - mi_isp_raw_cfa_batch: the decode alone: that CFA, H x W of the work dtype, written to cfa_host[i].
 * Host-side checks before any launch (error text names "demosaic_directional"): NULL pointers, odd or non-positive sizes,
 * dtypes, the pattern, the kind, n < 0, levels and grids, and an output, a CFA or a typed source (MI_RAW_16U, MI_RAW_16F,
 * MI_RAW_32F) that is not aligned to its element (packed bytes stand anywhere).  An output that is aligned to its element
 * only is stored element by element.  n == 0 is a successful no-op. */
int mi_isp_demosaic_directional_cfa(const void* cfa_dev, void* rgb_dev, int H, int W, int in_dtype, int out_dtype,
                                    int pattern, const float* ccm9_host, void* stream);
int mi_isp_demosaic_directional_raw_batch(const void* const* srcs_host, void* const* rgbs_host, int n, int H, int W,
                                          int src_kind, int ids_format, int work_dtype, int pattern,
                                          const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                                          const float* ccm9_host, void* stream);
int mi_isp_raw_cfa_batch(const void* const* srcs_host, void* const* cfas_host, int n, int H, int W, int src_kind,
                         int ids_format, int work_dtype, const mi_isp_levels* levels_host,
                         const mi_isp_shading* shading_host, void* stream);
/* ---- chromatic aberration("Chromatic aberration") ------------------------------------------------------
 * Lateral chromatic aberration corrected on the CFA: the red and the blue site planes are resampled radially about the
 * optical centre, green is left alone; in f32 with one rounding per operation, left to right, never contracted: the
 * output is the contract's bit for bit.  x(p) is the value raw noise reduction filters (above); s(p) = (row & 1) * 2 +
 * (col & 1); the colour of a site follows `pattern`.  The library rounds once from double to f32: cy, cx, iR2 = 1 /
 * norm_radius^2, and per channel d0 = k0 - 1, d1 = k1, d2 = k2 (red[] / blue[] = k0, k1, k2).
 *   green site: y = x(p).
 *   red / blue site p = (r, c) of parity (r0, c0), site plane P of nr x nc cells, d of its channel:
 *     dy = f32(r) - cy;  dx = f32(c) - cx;  r2 = dx dx + dy dy;  q = r2 iR2;  e = d0 + q (d1 + q d2)
 *     vs = f32(r) + dy e;  us = f32(c) + dx e;  a = (vs - f32(r0)) 0.5;  b = (us - f32(c0)) 0.5
 *     i = floor(a), fr = a - f32(i);  j = floor(b), fc = b - f32(j)
 *     i0 = clamp(i, 0, nr - 1), i1 = clamp(i + 1, 0, nr - 1), j0, j1 likewise;  mix(u, v, t) = u (1 - t) + v t
 *     y = mix(mix(P[i0,j0], P[i0,j1], fc), mix(P[i1,j0], P[i1,j1], fc), fr)
 *     when one of the four taps is set in the defect mask: w00 = (1 - fr)(1 - fc), w01 = (1 - fr) fc, w10 = fr (1 - fc),
 *     w11 = fr fc; S, N the sums of w and of w x over the unmasked taps in the order 00, 01, 10, 11, each from its first
 *     kept term; y = N / S when S > 0, else x(p)
 *   cfa = cast_work(y * g(p))      (g the lens shading gain of shading_host at p, 1 for NULL)
 * Source kinds, levels, grids, defect maps and outputs as mi_isp_highlights_raw(_batch), out_f32_plain included (the
 * output is the H x W f32 y itself; shading_host must be NULL).
 *  - mi_isp_chromatic_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "chromatic"): every setting finite (in f32 too), norm_radius > 0,
 * the shift limit - max |(k0 - 1) + q (k1 + q k2)| r <= 8 raw pixels for both channels, in double at 1025 equally spaced
 * radii r from 0 to the distance of the farthest corner pixel from the centre, q = r^2 / norm_radius^2 - the pattern,
 * shapes, dtypes, kinds, levels, grids, NULL pointers.  n == 0 and H * W == 0 are successful no-ops. */
typedef struct { double cy, cx, norm_radius; double red[3], blue[3]; } mi_isp_chromatic;
int mi_isp_chromatic_raw(const void* src_dev, void* cfa_dev, int H, int W, int src_kind, int ids_format, int work_dtype,
                         int pattern, const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                         const mi_isp_defects* defects_host, const mi_isp_chromatic* chromatic_host, int out_f32_plain,
                         void* stream);
int mi_isp_chromatic_raw_batch(const void* const* src_host, void* const* cfa_host, int n, int H, int W, int src_kind,
                               int ids_format, int work_dtype, int pattern, const mi_isp_levels* levels_host,
                               const mi_isp_shading* shading_host, const mi_isp_defects* const* defects_host,
                               const mi_isp_chromatic* chromatic_host, int out_f32_plain, void* stream);
int mi_isp_chromatic_cfa(const void* in_dev, void* out_dev, int H, int W, int dtype, int pattern,
                         const mi_isp_chromatic* chromatic_host, void* stream);
/* ---- temporal noise reduction ("Temporal noise reduction") ----------------------------------------------
 * Every raw pixel blended with the same camera's previous output where the scene has not moved, and returned untouched
 * where it has; in f32 with one rounding per operation, left to right, never contracted: the output is the contract's
 * bit for bit.  x(p) is the value raw noise reduction filters (above); h(p) the history plane hist_in, an H x W f32 plane
 * that holds this stage's previous y for the same camera.  From the f32 settings the library computes, in double and
 * rounded once to f32: rn2 = read_noise^2, c = threshold^2 and R[n] = 1 / n for n = 1 .. 9; wmax = max_weight.  T(p) = the taps (r + 2i, c + 2j),
 * |i|, |j| <= 1, inside the frame and not set in the defect mask (the centre is a tap unless it is listed), in the order
 * i = -1, 0, 1 and within a row j = -1, 0, 1; n = |T(p)|.
 *   D = the sum over T(p), in that order, from its first kept term, of |x(q) - h(q)|;  m = D R[n]
 *   var = gain max(h(p), 0) + rn2;  qv = (m m) / (c var)   (an IEEE division);  k = max(1 - qv, 0);  w = wmax k
 *   y = x(p) when n == 0 or w == 0 (selected, not computed), else x(p) + w (h(p) - x(p))
 *   hist_out(p) = y;  cfa = cast_work(y * g(p))      (g the lens shading gain of shading_host at p, 1 for NULL)
 * hist_in NULL is an empty history: y = x(p) everywhere.  Finite inputs only.  Source kinds, levels, grids and defect maps
 * as mi_isp_denoise_raw(_batch).  out_f32_plain != 0: there is no gain and no cast (shading_host must be NULL), hist_out
 * is the plain f32 y for the next raw stage to take as MI_RAW_32F, and cfa is not written and may be NULL: the frame is
 * written once.  hist_out must not overlap hist_in, the source, the CFA or another frame's
 * planes.  One launch per 32 frames.
 *  - mi_isp_temporal_raw_batch: n frames of one geometry; hist_in_host NULL, or one entry per frame (NULL: empty).
 *  - mi_isp_temporal_cfa: a normalised H x W CFA of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "temporal"): gain finite >= 0, read_noise and threshold finite
 * > 0 with squares that are finite and > 0 in f32, max_weight in [0, 1), shapes, dtypes, kinds, levels, grids, NULL
 * pointers, overlaps.  n == 0 and H * W == 0 are successful no-ops. */
typedef struct { float gain, read_noise, threshold, max_weight; } mi_isp_temporal;
int mi_isp_temporal_raw(const void* src_dev, const float* hist_in_dev, float* hist_out_dev, void* cfa_dev, int H, int W,
                        int src_kind, int ids_format, int work_dtype, const mi_isp_levels* levels_host,
                        const mi_isp_shading* shading_host, const mi_isp_defects* defects_host,
                        const mi_isp_temporal* temporal_host, int out_f32_plain, void* stream);
int mi_isp_temporal_raw_batch(const void* const* src_host, const float* const* hist_in_host, float* const* hist_out_host,
                              void* const* cfa_host, int n, int H, int W, int src_kind, int ids_format, int work_dtype,
                              const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                              const mi_isp_defects* const* defects_host, const mi_isp_temporal* temporal_host,
                              int out_f32_plain, void* stream);
int mi_isp_temporal_cfa(const void* in_dev, const float* hist_in_dev, float* hist_out_dev, void* out_dev, int H, int W,
                        int dtype, const mi_isp_temporal* temporal_host, void* stream);
/* ---- exposure merge ("Exposure merge") ------------------------------------------------------------------
 * E raw frames of one camera and one instant (2 <= E = n <= 4, the shortest exposure first, ratio[0] == 1, ratios
 * strictly increasing and <= 65536) merged into one linear raw frame y in the units of the shortest; in f32 with one
 * rounding per operation, left to right, never contracted, IEEE divisions: the output is the contract's bit for bit.
 * x_e(p) is the value raw noise reduction filters (above) of frame e.  gain, read_noise: the noise model in the units of
 * the shortest frame's x; saturation (in the units of x): a long frame's value at or above it is not used; knee: the
 * usable weight falls linearly from 1 at saturation (1 - knee) to 0 at saturation; threshold: the mean absolute
 * difference to the shortest frame, in noise standard deviations, at which a long frame is dropped.  From the f32
 * settings the library computes, in double and rounded once to f32: inv_e = 1 / ratio_e, i2_e = 1 / ratio_e^2,
 * rn2 = read_noise^2, c = threshold^2, rf = 1 / (saturation knee) and R[n] = 1 / n for n = 1 .. 9.  T(p) = the taps
 * (r + 2i, c + 2j), |i|, |j| <= 1, inside the frame and not set in the defect mask, in the order i = -1, 0, 1 and within
 * a row j = -1, 0, 1; n = |T(p)|.
 *   s0 = x_0(p);  v0 = gain max(s0, 0) + rn2;  a0 = 1 / v0;  num = a0 s0;  den = a0
 *   for e = 1 .. E - 1:  se(q) = x_e(q) inv_e;  D = the sum over T(p), from its first kept term, of |se(q) - x_0(q)|
 *     m = D R[n];  ve = (gain max(x_e(p), 0) + rn2) i2_e;  qv = (m m) / (c (v0 + ve));  k = max(1 - qv, 0)
 *     u = min(max((saturation - x_e(p)) rf, 0), 1);  w = (u k) / ve;  if w > 0: num = num + w se(p), den = den + w
 *   y = x_0(p) when n == 0 or no long frame had w > 0 (selected, not computed), else num / den
 *   out = cast_work(y * g(p))                        (g the lens shading gain of shading_host at p, 1 for NULL)
 * Finite inputs only.  Source kinds, levels, grids and defect maps as mi_isp_denoise_raw(_batch); one defect map per
 * bracket.  out_f32_plain != 0: there is no gain and no cast (shading_host must be NULL) and out is the plain f32 y for
 * the next raw stage to take as MI_RAW_32F.  The output must not overlap a source frame or another bracket's output.
 * One launch per 16 brackets.
 *  - mi_isp_merge_raw: one bracket; src_host holds its n device pointers.
 *  - mi_isp_merge_raw_batch: n_brackets brackets of one geometry; src_host holds n_brackets * n device pointers,
 *    bracket-major; out_host and defects_host one entry per bracket.
 *  - mi_isp_merge_cfa: n normalised H x W CFAs of dtype MI_F16 / MI_F32 (no levels, gain or mask), out of the same dtype.
 * Host-side checks before any launch (error text names "exposure merge"): the settings above, every computed constant
 * finite and > 0 in f32, shapes, dtypes, kinds, levels, grids, NULL pointers, overlaps.  n_brackets == 0 and H * W == 0
 * are successful no-ops. */
typedef struct { int32_t n; float ratio[4]; float gain, read_noise, saturation, knee, threshold; } mi_isp_exposure_merge;
int mi_isp_merge_raw(const void* const* src_host, void* out_dev, int H, int W, int src_kind, int ids_format, int work_dtype,
                     const mi_isp_levels* levels_host, const mi_isp_shading* shading_host,
                     const mi_isp_defects* defects_host, const mi_isp_exposure_merge* merge_host, int out_f32_plain,
                     void* stream);
int mi_isp_merge_raw_batch(const void* const* src_host, void* const* out_host, int n_brackets, int H, int W, int src_kind,
                           int ids_format, int work_dtype, const mi_isp_levels* levels_host,
                           const mi_isp_shading* shading_host, const mi_isp_defects* const* defects_host,
                           const mi_isp_exposure_merge* merge_host, int out_f32_plain, void* stream);
int mi_isp_merge_cfa(const void* const* in_host, void* out_dev, int H, int W, int dtype,
                     const mi_isp_exposure_merge* merge_host, void* stream);
/* ---- local tone mapping ("Local tone mapping") ------------------------------------------------------------
 * Every pixel of a work-dtype RGB image (H x W x 3 interleaved, MI_F16 or MI_F32) times a gain that depends only on an
 * edge-aware local mean of its log-luminance, read from a bilateral grid (splat, blur, slice).  Integer and single f32
 * operations only (the logarithm and the exponential are the piecewise-linear ones of the f32 bit pattern), so the output
 * is the contract's bit for bit.  Every line one operation; f32 operations round to nearest and are never contracted,
 * divisions are IEEE, bits() is the f32 bit pattern as int32, >> arithmetic, float-to-int truncates toward zero,
 * integer-to-f32 rounds to nearest even:
 *   li(t) = (bits(min(max(t, floor), white)) - bits(floor)) >> 12
 *   span = li(white);  zs = f32((bins - 1) / span);  kq = f32(strength * 4096)         (in double, rounded once)
 *   Y = ((r + b) * 0.25) + (g * 0.5);  l = li(Y);  z = f32(l) * zs
 *   splat: zi = min(int(z + 0.5), bins - 1);  cnt[y / cell, x / cell, zi] += 1;  sum[same] += l           (u32, exact)
 *   blur:  Nb = f32(B(cnt)), Sb = f32(B(sum));  B = the separable [1 2 1] filter along all three axes, zero outside the
 *          grid, accumulated exactly in 64-bit integers, converted once
 *   slice: gy = clamp((y + 0.5) * (1 / cell) - 0.5, 0, GH - 1);  y0 = min(int(gy), max(GH - 2, 0));  y1 = min(y0 + 1, GH - 1)
 *          fy = gy - y0;  the same for x;  z0 = min(int(z), bins - 2);  fz = z - z0;  lerp(a, b, f) = a + ((b - a) * f)
 *          for Nb and for Sb separately: along x on the four (y, z) rows, then along y, then along z
 *          base = S / N when N > 0, f32(l) otherwise
 *   gain = float_from_bits(0x3F800000 + int((f32(li(anchor)) - base) * kq));  out_c = cast(v_c * gain) for c = r, g, b
 * GH = ceil(H / cell), GW = ceil(W / cell); the planes cnt, sum (u32) and Nb, Sb (f32) are [GH][GW][bins].  Inputs must be
 * finite.  Settings: 0 <= strength <= 1; white > 0; 0 < floor < white with floor a normal f32, white / floor <= 2^24 and
 * li(white) >= 1; floor <= anchor <= white; cell 8, 16, 32 or 64; 2 <= bins <= 32; every value finite.
 *  - mi_isp_local_tonemap_workspace_bytes: the bytes of ws_dev for n images of H x W (0 for bad arguments).
 *  - mi_isp_local_tonemap_batch: n images of one geometry, in place; three launches (splat, blur, apply) per 32 images,
 *    ordered by the stream, no host synchronisation.  images_host: n device pointers, read on the host, each aligned to
 *    its element; ws_dev: 16-byte aligned device memory, contents irrelevant before and after the call.
 *  - mi_isp_local_tonemap_grids: splat and blur of one image into the caller's four planes (GH * GW * bins elements each,
 *    4-byte aligned, not overlapping); the image is not written.  For tests and measurements.
 * Host-side checks before any launch (error text names "local_tonemap"): the settings, n >= 0, 0 <= H, W <= 32768, the
 * dtype, NULL pointers, alignment.  n == 0 and H * W == 0 are successful no-ops. */
typedef struct { float strength, white, floor, anchor; int32_t cell, bins; } mi_isp_local_tonemap;
size_t mi_isp_local_tonemap_workspace_bytes(int n, int H, int W, const mi_isp_local_tonemap* settings_host);
int mi_isp_local_tonemap_batch(void* const* images_host, int n, int H, int W, int dtype,
                               const mi_isp_local_tonemap* settings_host, void* ws_dev, void* stream);
int mi_isp_local_tonemap_grids(const void* image_dev, int H, int W, int dtype, const mi_isp_local_tonemap* settings_host,
                               uint32_t* cnt_dev, uint32_t* sum_dev, float* nb_dev, float* sb_dev, void* stream);
/* ---- antialiased resize ("Antialiased resize") ---------------------------------------------------------
 * A separable, table-driven resize of work-dtype RGB images (H x W x 3 interleaved, MI_F16 or MI_F32 in, MI_F16 or MI_F32
 * out): one table per axis, built on the host; the kernel evaluates the tables and decides nothing itself.
 * The table of an axis with S source and D output samples at scale s (output / source), every operation one IEEE double
 * operation in the order written; filter MI_RESAMPLE_AREA / _TRIANGLE / _LANCZOS3:
 *   widen = s < 1 ? 1 / s : 1;  c = d / s                                         (the geometry of mi_isp_resize_bilinear)
 *   radius R = widen / 2 + 0.5 (area), widen (triangle), 3 * widen (lanczos3); candidates k = floor(c - R) .. ceil(c + R)
 *   area, s < 1:    w = min(k + 0.5, c + widen / 2) - max(k - 0.5, c - widen / 2)
 *   triangle, and area at s >= 1:  w = 1 - |k - c| / widen
 *   lanczos3:       x = (k - c) / widen;  w = |x| < 3 ? sinc(x) * sinc(x / 3) : 0;  sinc(0) = 1, sinc of another integer
 *                   is 0, else sinc(x) = sin(pi * x) / (pi * x) with pi * x one product
 *   a candidate is a tap when w > 0 (area, triangle) or w != 0 (lanczos3); first / last: the lowest / highest tap index
 *   T = min(max over d of (last - first + 1), S);  start[d] = min(max(first, 0), S - T)
 *   row d: T doubles, zero; for the taps in increasing k: row[min(max(k, 0), S - 1) - start[d]] += w    (replicate border)
 *   sum = ((row[0] + row[1]) + ...) + row[T - 1];  weight[d][j] = f32(row[j] / sum)
 * so at s >= 1 area and triangle hold the bilinear weights (1 - frac, frac), and at s == 1 every filter is one tap of
 * weight 1.  T <= 32, or the filter does not take the scale.
 * The image, f32 with one rounding per operation and no contraction, per channel:
 *   h[y][x] = (..((wx[x][0] * f32(src[y][sx[x]])) + wx[x][1] * f32(src[y][sx[x] + 1])) + ..) over the Tx taps in order
 *   o[r][x] = the same over h[sy[r] + j][x] with wy[r][j], j = 0 .. Ty - 1;  dst[r][x] = cast(o[r][x])
 * h is never rounded to f16, a zero weight still multiplies its (padded) tap, and nothing is clamped.
 *  - mi_isp_resample_taps: T of the axis (host only, nothing is launched), or -1 with the error set (a bad filter, S or D
 *    not positive, a scale that is not finite and > 0, T > 32: the text names the filter and the smallest scale it takes).
 *  - mi_isp_resample_table: the table of the axis into start_host (D int32) and weight_host (D x T f32); host only.
 *  - mi_isp_resample_batch: n images of one geometry in ONE launch per 32 images, both passes in it (the horizontally
 *    filtered rows exist in LDS only).  rows / cols: the tables of the vertical (S = Hs, D = Hd) and the horizontal axis on
 *    the device, 0 <= start[d] <= S - taps (the kernel clamps a start into that range, so no table makes it read
 *    outside the image; starts that do not rise with d are evaluated all the same, tap by tap from memory).  srcs_host / dsts_host: n device pointers each, read on the host, each
 *    aligned to its element; an output must not overlap a source.
 * Host-side checks before any launch (error text names "resample"): NULL pointers, n < 0, sizes that are not positive
 * (Hd or Wd == 0 and n == 0 are successful no-ops that launch nothing), taps outside 1 .. min(32, S), the dtypes. */
#define MI_RESAMPLE_AREA 1
#define MI_RESAMPLE_TRIANGLE 2
#define MI_RESAMPLE_LANCZOS3 3
#define MI_RESAMPLE_MAX_TAPS 32
typedef struct { int32_t taps; const int32_t* start_dev; const float* weight_dev; } mi_isp_resample_axis;
int mi_isp_resample_taps(int filter, int S, int D, double scale);
int mi_isp_resample_table(int filter, int S, int D, double scale, int32_t* start_host, float* weight_host);
int mi_isp_resample_batch(const void* const* srcs_host, void* const* dsts_host, int n, int Hs, int Ws, int Hd, int Wd,
                          int in_dtype, int out_dtype, const mi_isp_resample_axis* rows_host,
                          const mi_isp_resample_axis* cols_host, void* stream);
/* ---- output sharpening ("Output sharpening") ----------------------------------------------------------
 * An unsharp mask on the luma of a u8 image, in integer arithmetic: the output is the contract's bit for bit.  All values
 * signed 32-bit, >> arithmetic, coordinates outside the image clamped to the edge; b = (1, 2, 1) for radius 1 and
 * (1, 4, 6, 4, 1) for radius 2, S = (sum b)^2 (16 or 256), k = 6 + log2 S, A = amount_q6 (the amount times 64, 0 .. 512):
 *   L = (77 R + 150 G + 29 B + 128) >> 8;  Bl = sum_ij b[i] b[j] L(y + i - r, x + j - r);  d = S L - Bl
 *   d' = sign(d) max(|d| - threshold S, 0);  delta = (A d' + (1 << (k - 1))) >> k
 *   overshoot >= 0:  delta = clamp(L + delta, min3x3(L) - overshoot, max3x3(L) + overshoot) - L
 *   out_c = clamp(I_c + delta, 0, 255) for c = R, G, B
 *  - mi_isp_sharpen_rgb_batch: n interleaved H x W x 3 images of one geometry, one launch per 32 images.
 *  - mi_isp_sharpen_yuv420_batch: n planar YUV 4:2:0 images (H * 3 / 2 rows of W bytes; H, W of the Y plane, H even): the
 *    filter with L = Y, out = clamp(Y + delta, 0, 255); the chroma rows are copied.
 * src_host / dst_host: n device pointers each, read on the host.  The stencil cannot run in place: src[i] != dst[i], and
 * no output (H * W * 3 bytes, H * W * 3 / 2 for the planar form) may overlap an input or another output of the call.
 * Host-side checks before any launch (error text names "sharpen"): the settings' ranges, n >= 1, H, W >= 0, NULL
 * pointers, src == dst, overlapping images.  H * W == 0 is a successful no-op. */
typedef struct { int32_t amount_q6, radius, threshold, overshoot /* -1: none */; } mi_isp_sharpen;
int mi_isp_sharpen_rgb_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                             const mi_isp_sharpen* sharpen_host, void* stream);
int mi_isp_sharpen_yuv420_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                const mi_isp_sharpen* sharpen_host, void* stream);
/* ---- local contrast ("Local contrast") -----------------------------------------------------------------
 * Contrast-limited adaptive histogram equalisation (CLAHE) of the luma of a u8 image, in integer arithmetic: the output
 * is the contract's bit for bit.  All values signed integers, >> arithmetic, / floor division; C = clip_q8 (the clip limit
 * times 256, 256 .. 16384, or 0: no clip), S = strength_q6 (the strength times 64, 0 .. 64), the image in tiles_y x
 * tiles_x tiles (1 .. 16 each):
 *   L = (77 R + 150 G + 29 B + 128) >> 8
 *   tile (i, j) = rows [i H / Ty, (i + 1) H / Ty) x columns [j W / Tx, (j + 1) W / Tx), n pixels;  h[v] = #{L == v}
 *   C != 0:  c = max(1, (C n) >> 16);  e = sum_v max(h[v] - c, 0);  h[v] = min(h[v], c) + (e >> 8)
 *            r = e & 255 > 0:  s = max(256 / r, 1);  h[k s] += 1 for k = 0 .. r - 1
 *   lut_ij[v] = (2 * 255 * (h[0] + ... + h[v]) + n) / (2 n)
 *   per axis (m, M, T = y, H, Ty or x, W, Tx):  N = (2 m + 1) T - M;  i0 = N / (2 M);  w = (256 (N - 2 M i0)) / (2 M)
 *            a = clamp(i0, 0, T - 1);  b = clamp(i0 + 1, 0, T - 1)
 *   E = ((256 - wy) ((256 - wx) lut[ay][ax][L] + wx lut[ay][bx][L])
 *            + wy ((256 - wx) lut[by][ax][L] + wx lut[by][bx][L]) + 32768) >> 16
 *   delta = ((E - L) S + 32) >> 6;  out_c = clamp(I_c + delta, 0, 255) for c = R, G, B
 *  - mi_isp_local_contrast_rgb_batch: n interleaved H x W x 3 images of one geometry; four launches (clear, histograms, LUTs,
 *    apply) per 32 images, ordered by the stream.
 *  - mi_isp_local_contrast_yuv420_batch: n planar YUV 4:2:0 images (H * 3 / 2 rows of W bytes; H, W of the Y plane, both
 *    even): the operator with L = Y, out = clamp(Y + delta, 0, 255); the chroma rows are copied when src[i] != dst[i].
 * src_host / dst_host: n device pointers each, read on the host.  src[i] == dst[i] exactly is allowed (the apply step is
 * pointwise); otherwise no output (H * W * 3 bytes, H * W * 3 / 2 for the planar form) may overlap an input - its own
 * source at a shifted address or another image's - or another output of the call.  ws_dev: mi_isp_local_contrast_workspace_bytes(n, lc) bytes of
 * device memory, 16-byte aligned, contents irrelevant before and after the call (0 bytes for bad settings or n <= 0).
 * Host-side checks before any launch (error text names "local_contrast"): the settings' ranges, n >= 0, H, W >= 0,
 * H >= tiles_y and W >= tiles_x and both <= 32768 (unless H * W == 0), NULL pointers, overlapping images.  n == 0 and
 * H * W == 0 are successful no-ops. */
typedef struct { int32_t tiles_y, tiles_x, clip_q8 /* 0: no clip */, strength_q6; } mi_isp_local_contrast;
size_t mi_isp_local_contrast_workspace_bytes(int n, const mi_isp_local_contrast* lc_host);
int mi_isp_local_contrast_rgb_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                    const mi_isp_local_contrast* lc_host, void* ws_dev, void* stream);
int mi_isp_local_contrast_yuv420_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                       const mi_isp_local_contrast* lc_host, void* ws_dev, void* stream);
/* ---- chroma noise reduction ("Chroma noise reduction") ---------------------------------------------------
 * A luma-guided mean of the chroma on the grid of 2 x 2 pixel cells of a u8 image, in integer arithmetic: the output is the
 * contract's bit for bit.  All values signed integers, >> arithmetic, // floor division; tl = luma_threshold and tc =
 * chroma_threshold (0 .. 255), S = strength_q6 (the strength times 64, 0 .. 64), r = radius (1, 2 or 3).  Cell (a, b), a <
 * (H + 1) / 2, b < (W + 1) / 2, holds pixels (min(2a + i, H - 1), min(2b + j, W - 1)), i, j in {0, 1}:
 *   L = (77 R + 150 G + 29 B + 128) >> 8;  SL = sum of the cell's four L;  SB = sum of its four B - SL;  SR likewise with R
 *   T(p) = the cells q = p + (i, j), |i|, |j| <= r, inside the grid (a cell outside it is no tap) with
 *          |SL(q) - SL(p)| <= 4 tl, |SB(q) - SB(p)| <= 4 tc and |SR(q) - SR(p)| <= 4 tc
 *   n = |T(p)|;  DB = sum over T(p) of SB(q) - SB(p);  DR likewise
 *   db = (2 DB S + 256 n) // (512 n);  dr = (2 DR S + 256 n) // (512 n);  dg = ((-(77 dr + 29 db)) * 437 + 32768) >> 16
 *   out_c = clamp(I_c + d_c, 0, 255) for each of the cell's pixels, c = R, G, B
 *  - mi_isp_chroma_denoise_rgb_batch: n interleaved H x W x 3 images of one geometry, one launch per 32 images.
 *  - mi_isp_chroma_denoise_yuv420_batch: n planar YUV 4:2:0 images (H * 3 / 2 rows of W bytes: the Y rows, the U plane, the
 *    V plane; H, W of the Y plane, both even): SL = the sum of the cell's four Y, SB = 4 U(a, b), SR = 4 V(a, b);
 *    U' = clamp(U + db, 0, 255), V' = clamp(V + dr, 0, 255); the Y rows are copied.
 * src_host / dst_host: n device pointers each, read on the host.  The stencil cannot run in place: src[i] != dst[i], and
 * no output may overlap an input or another output of the call.  Host-side checks before any launch (error text names
 * "chroma_denoise"): the settings' ranges, n >= 0, H, W >= 0 (both even for the planar form), NULL pointers, src == dst,
 * overlapping images.  n == 0 and H * W == 0 are successful no-ops. */
typedef struct { int32_t radius, luma_threshold, chroma_threshold, strength_q6; } mi_isp_chroma_denoise;
int mi_isp_chroma_denoise_rgb_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                    const mi_isp_chroma_denoise* settings_host, void* stream);
int mi_isp_chroma_denoise_yuv420_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                       const mi_isp_chroma_denoise* settings_host, void* stream);
/* ---- luma noise reduction ("Luma noise reduction") ---------------------------------------------------------
 * An edge-preserving mean of the luma over a (2r + 1)^2 window of a u8 image, in integer arithmetic: the output is the
 * contract's bit for bit.  All values signed integers, >> arithmetic, // floor division; t0 = threshold and t1 =
 * threshold_bright (0 .. 255 luma codes), S = strength_q6 (the strength times 64, 0 .. 64), r = radius (1, 2 or 3).  Per
 * pixel p:
 *   L = (77 R + 150 G + 29 B + 128) >> 8;  T = t0 + (((t1 - t0) L(p) + 128) >> 8)
 *   the taps q = p + (i, j), |i|, |j| <= r, INSIDE the image (a pixel outside it is no tap: no padding) with
 *   |L(q) - L(p)| <= T;  n = their number (the centre always counts), s = the sum of their L
 *   m = (2 s + n) // (2 n);  delta = (S (m - L(p)) + 32) >> 6;  out_c = clamp(I_c + delta, 0, 255) for c = R, G, B
 *  - mi_isp_luma_denoise_rgb_batch: n interleaved H x W x 3 images of one geometry, one launch per 32 images.
 *  - mi_isp_luma_denoise_yuv420_batch: n planar YUV 4:2:0 images (H * 3 / 2 rows of W bytes; H, W of the Y plane, both
 *    even): the filter with L = Y, out = clamp(Y + delta, 0, 255); the chroma rows are copied.
 * src_host / dst_host: n device pointers each, read on the host.  The stencil cannot run in place: src[i] != dst[i], and
 * no output may overlap an input or another output.  Host-side checks before any launch (error text names
 * "luma_denoise"): the settings' ranges, n >= 0, H, W >= 0 (both even for the planar form), NULL pointers, src == dst,
 * overlapping images.  n == 0 and H * W == 0 are successful no-ops.  No host synchronisation; the launches run on
 * `stream`. */
typedef struct { int32_t radius, threshold, threshold_bright, strength_q6; } mi_isp_luma_denoise;
int mi_isp_luma_denoise_rgb_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                  const mi_isp_luma_denoise* settings_host, void* stream);
int mi_isp_luma_denoise_yuv420_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                     const mi_isp_luma_denoise* settings_host, void* stream);
/* ---- 3D colour LUT ("Colour LUT") --------------------------------------------------------------------------
 * Tetrahedral interpolation in an N x N x N table on interleaved u8 RGB images, in integer arithmetic: the output is the
 * contract's bit for bit.  The table T[r][g][b] holds the output colour (u8 R, G, B) at input (255 r, 255 g, 255 b) / (N - 1);
 * table_dev: N^3 dwords on the device, entry (r * N + g) * N + b = R | G << 8 | B << 16.  N = n_points (2 .. 65), S =
 * strength_q6 (the strength times 64, 0 .. 64).  All values signed integers, // floor division, >> arithmetic.  Per pixel,
 * v_c its input codes, c = R, G, B:
 *   p_c = v_c (N - 1);  i_c = p_c // 255;  f_c = p_c - 255 i_c  (0 .. 254; v_c = 255 gives i_c = N - 1, f_c = 0)
 *   j_c = min(i_c + 1, N - 1)
 *   a, b, d = the three axes ordered so that f_a >= f_b >= f_d (the order of tied fractions does not matter: the corner that
 *             differs has weight 0)
 *   C0 = T[i_R][i_G][i_B];  C1 = C0's index with axis a moved to j_a;  C2 = C1's with axis b moved to j_b;  C3 = T[j_R][j_G][j_B]
 *   y_c = (C0_c (255 - f_a) + C1_c (f_a - f_b) + C2_c (f_b - f_d) + C3_c f_d + 127) // 255
 *   out_c = v_c + (((y_c - v_c) S + 32) >> 6)        (between v_c and y_c: no clamp; S = 64 gives y_c, S = 0 gives v_c)
 * Every table index stays inside the table whatever its weight is (the min above).
 *  - mi_isp_color_lut_rgb_batch: n H x W x 3 images of one geometry, one launch per 32 images.  The table is kept in LDS
 *    (N <= 33) or read through L2, whichever is faster for the launch's size; the output does not depend
 *    on it.
 *  - mi_isp_color_lut_rgb_batch_path: the same with the path given (for measurements and tests): 0 the dispatcher's choice,
 *    1 the table in LDS (n_points <= 33), 2 the table in global memory.
 * src_host / dst_host: n device pointers each, read on the host.  The operator is pointwise: src[i] == dst[i] exactly is
 * allowed; otherwise no output (H * W * 3 bytes) may overlap an input - its own source at a shifted address or another
 * image's - or another output of the call.  Host-side checks before any launch (error text names "color_lut"): the
 * settings' ranges, the path, n >= 0, H, W >= 0, NULL pointers, overlapping images.  n == 0 and H * W == 0 are successful
 * no-ops.  No host synchronisation; the
 * launches run on `stream`. */
typedef struct { int32_t n_points, strength_q6; } mi_isp_color_lut;
int mi_isp_color_lut_rgb_batch(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                               const uint32_t* table_dev, const mi_isp_color_lut* settings_host, void* stream);
int mi_isp_color_lut_rgb_batch_path(const uint8_t* const* src_host, uint8_t* const* dst_host, int n, int H, int W,
                                    const uint32_t* table_dev, const mi_isp_color_lut* settings_host, int path, void* stream);
/* The stateless chain of test/pipeline.py:26-32 (BASELINE config 2) fused:
 * decode12(scaled, work_dtype) -> bayer_to_rgb -> tonemap_reinhard(dtype=out_dtype) in four data passes.
 * The demosaiced work-dtype image is kept between the passes in out_dev itself when out_dtype ==
 * work_dtype, else in work_image_dev (H * W * 3 work-dtype elements, 16-byte aligned, caller-owned scratch);
 * with work_image_dev == NULL and different dtypes every pass re-derives it from the packed frame
 * (minimal HBM traffic, about 1.5x the time). */
int mi_isp_pipeline12_reinhard(const uint8_t* packed_dev, void* out_dev, void* work_image_dev, int H, int W,
                               int ids_format, int pattern, const float* ccm9_host,
                               int work_dtype, int out_dtype, float gamma, float intensity,
                               float light_adapt, float color_adapt, void* ws_dev, void* stream);
/* Which chain of kernels mi_isp_pipeline12_reinhard[_batch] runs for these arguments, without launching anything: the
 * library's own decision (the function that answers here is the one the launches go through), from the pointers'
 * VALUES, the shape, the layout and the dtypes alone.  Nothing is dereferenced and no device is touched: made-up
 * addresses are fine, and no GPU is needed.
 *   MI_ISP_ROUTE_STREAM          the streaming kernels, four passes over the packed frame: the standard layout, W % 8 == 0,
 *                                H >= 4, packed rows 4-byte aligned, the output 16-byte (u8: 8-byte) aligned
 *   MI_ISP_ROUTE_CACHED_STREAM   such a frame whose OUTPUT is not aligned, with an aligned work-dtype image (work_image_dev,
 *                                or the output when it has the work dtype): the streaming kernel stores the image and
 *                                reduces its bounds, three elementwise passes follow
 *   MI_ISP_ROUTE_CACHED_TILE     any other frame with W % 8 == 0 and an aligned work-dtype image: the tile kernel as the
 *                                first pass (hot = 1: its specialisation for aligned packed rows; 0: the generic kernel)
 *   MI_ISP_ROUTE_RECOMPUTE       everything else (W % 8 != 0, no aligned work-dtype image): four tile passes over the
 *                                packed frame and three finalize launches
 * rows_per_wave, bands_x: the streaming kernels' geometry (0 on the tile routes); n_blocks: the blocks (= partial results)
 * of the route's first pass.  Non-zero with a message for arguments mi_isp_pipeline12_reinhard refuses. */
enum { MI_ISP_ROUTE_STREAM = 0, MI_ISP_ROUTE_CACHED_STREAM = 1, MI_ISP_ROUTE_CACHED_TILE = 2, MI_ISP_ROUTE_RECOMPUTE = 3 };
typedef struct { int32_t route, hot, rows_per_wave, bands_x, n_blocks; } mi_isp_route;
int mi_isp_pipeline12_route(const uint8_t* packed_dev, void* out_dev, void* work_image_dev, int H, int W, int ids_format,
                            int work_dtype, int out_dtype, mi_isp_route* route_host);
/* One camera group from packed bytes to u8 outputs in one call on the caller's stream (ISP.load_packed12/16 per
 * camera, camera_isp.py:333-347; the rolling metering over the group, :376-385 -> :142-175; ISP.tonemap_reinhard or
 * tonemap_linear, :394-413, with the orientation transform folded into the store).
 *   packed_host / images_host / outs_host: host arrays of n device pointers; images are (Hd, Wd, 3) work-dtype buffers
 *   owned by the caller - after the call they hold what the reference leaves in them (the loaded image for the linear
 *   map, the Reinhard-mapped p for Reinhard, camera_isp.py:211); outs are u8 (Hd, Wd, 3), or the transformed shape.
 *   bits 12 / 16; scale > 0: demosaic + bilinear resize fused (Hd, Wd = ISP.resize_image's size; the scale must
 *   satisfy mi_isp_load_packed_scale_supported), scale <= 0: Hd == H, Wd == W.
 *   state9_dev: the ISP's metering 9-vector (in/out); alpha: 0 for the first group, 1 - moving_alpha afterwards
 *   (camera_isp.py:376-385).  tonemap: 0 = Reinhard (gamma, intensity, light_adapt, color_adapt), 1 = linear (gamma). */
int mi_isp_camera_frame_batch(const uint8_t* const* packed_host, void* const* images_host, uint8_t* const* outs_host,
                              int n, int H, int W, int bits, int ids_format, int pattern, const float* ccm9_host,
                              int work_dtype, int Hd, int Wd, float scale, int metering_stride, float* state9_dev,
                              float alpha, int tonemap, float gamma, float intensity, float light_adapt,
                              float color_adapt, int transform, void* ws_dev, void* stream);

/* One FULL-RESOLUTION camera group from packed bytes to u8 outputs without the image in between - what the reference's
 * bench does per step (taichi_image/bench/camera_isp.py:19-28, Processor.__call__: ISP.load_packed12 per camera,
 * camera_isp.py:333-340; ISP.tonemap_reinhard over the list, :394-403 -> update_metering :376-385 + reinhard_kernel :177-218;
 * the loaded images are dropped).  Three steps on `stream`: the stride-8 subsample of every camera straight from its
 * packed frame (only the rows r % 8 == 0 are demosaiced), the rolling metering over the subsamples (mi_isp_metering), and
 * ONE persistent launch that walks through the cameras: demosaic -> the f16 pixels resident on the chip -> Reinhard and
 * its maximum -> grid barrier (max_out, :213) -> u8 = 255 (p / max_out)^(1 / gamma).  HBM sees the packed frame in and the
 * u8 image out.  Same bits as mi_isp_camera_frame_batch(scale <= 0, tonemap 0, no transform) in outs, state9 and images.
 *   packed_host / outs_host: host arrays of n device pointers (12-bit standard layout; u8 (H, W, 3), 8-byte aligned).
 *   images_host: NULL (the bench's case: p is not stored anywhere), or n device pointers to (H, W, 3) f16 buffers
 *     (16-byte aligned) that receive what the reference leaves in its loaded images: p, camera_isp.py:211.
 *   prev9_dev -> state9_dev, alpha: the metering state before and after this group (mi_isp_metering_to; the two may be the
 *     same buffer), alpha as mi_isp_camera_frame_batch.  Metering stride 8, f16 work dtype (Camera16), 1 <= n <= 64.
 *   scratch_dev: mi_isp_camera_group_scratch_bytes(n, H, W) bytes (the subsamples).
 *   ws_dev: (n + 1) x mi_isp_workspace_bytes(H, W) bytes, zero-filled once (a workspace per camera + the metering's).
 * mi_isp_camera_group_fits: 1 if the frame fits the resident grid (as mi_isp_pipeline12_whole_frame_fits) with this
 *   pattern, work dtype (MI_F16 only) and metering stride (8 only); otherwise use mi_isp_camera_frame_batch.
 * A grid barrier that times out (a foreign kernel holding CUs) sets the camera's workspace fault word and the device's
 * camera-group mailbox word: mi_isp_camera_group_faults(clear) reads it (a host read, no synchronisation); the outputs of
 * that call are invalid.  mi_isp_camera_group_set_poll_limit(polls): poll budget of later launches (0 = default; tests: 1).
 * Launched in the one order of the library's resident-grid kernels (see mi_isp_whole_frame_set_sabotage). */
int mi_isp_camera_group_reinhard(const uint8_t* const* packed_host, void* const* images_host, uint8_t* const* outs_host,
                                 int n, int H, int W, int pattern, const float* ccm9_host, const float* prev9_dev,
                                 float* state9_dev, float alpha, float gamma, float intensity, float light_adapt,
                                 float color_adapt, void* scratch_dev, void* ws_dev, void* stream);
/* The same in its steps, for callers that put something between them (taichi_image_amd: the sharded metering of a
 * multi-GPU group, two all-gathers between the subsample and the tone map):
 *   mi_isp_camera_group_subsample: image[::8, ::8] of every camera's (never materialised) image - (ceil(H / 8), ceil(W / 8), 3)
 *     f16 each, camera i at scratch_dev + i * mi_isp_camera_group_scratch_bytes(1, H, W) - for mi_isp_metering (stride 1);
 *   mi_isp_camera_group_tonemap: the persistent launch, with the Reinhard scalars of state9_dev (read on the device);
 *     ws_dev: n x mi_isp_workspace_bytes(H, W). */
int mi_isp_camera_group_subsample(const uint8_t* const* packed_host, int n, int H, int W, int pattern, const float* ccm9_host,
                                  void* scratch_dev, void* stream);
int mi_isp_camera_group_tonemap(const uint8_t* const* packed_host, void* const* images_host, uint8_t* const* outs_host, int n,
                                int H, int W, int pattern, const float* ccm9_host, const float* state9_dev, float gamma,
                                float intensity, float light_adapt, float color_adapt, void* ws_dev, void* stream);
int mi_isp_camera_group_fits(int H, int W, int pattern, int work_dtype, int metering_stride);
size_t mi_isp_camera_group_scratch_bytes(int n, int H, int W);
int mi_isp_camera_group_faults(int clear);
int mi_isp_camera_group_set_poll_limit(unsigned polls);
/* The camera group with sensor levels (mi_isp_levels above; NULL = the calls without _levels): the subsample and the
 * persistent launch decode with the levels, one black level folded into the decode table, four applied in registers.
 * mi_isp_camera_group_fits_levels: as mi_isp_camera_group_fits for the kernel these levels take (0 for invalid levels). */
int mi_isp_camera_group_reinhard_levels(const uint8_t* const* packed_host, void* const* images_host, uint8_t* const* outs_host,
                                        int n, int H, int W, int pattern, const float* ccm9_host, const float* prev9_dev,
                                        float* state9_dev, float alpha, float gamma, float intensity, float light_adapt,
                                        float color_adapt, void* scratch_dev, void* ws_dev, const mi_isp_levels* levels_host,
                                        void* stream);
int mi_isp_camera_group_subsample_levels(const uint8_t* const* packed_host, int n, int H, int W, int pattern,
                                         const float* ccm9_host, void* scratch_dev, const mi_isp_levels* levels_host,
                                         void* stream);
int mi_isp_camera_group_tonemap_levels(const uint8_t* const* packed_host, void* const* images_host, uint8_t* const* outs_host,
                                       int n, int H, int W, int pattern, const float* ccm9_host, const float* state9_dev,
                                       float gamma, float intensity, float light_adapt, float color_adapt, void* ws_dev,
                                       const mi_isp_levels* levels_host, void* stream);
int mi_isp_camera_group_fits_levels(int H, int W, int pattern, int work_dtype, int metering_stride,
                                    const mi_isp_levels* levels_host);

/* The same chain (test/pipeline.py:26-32) as ONE persistent launch (csrc/isp_mega.h): the frame is demosaiced once,
 * the f16 RGB image stays in registers and LDS, the three global dependencies of tonemap.py:146-154 are grid
 * barriers inside the kernel; HBM sees the packed frame in and the output out.  f16 work dtype; out_dtype u8 / u16 /
 * f16; frames up to 2 x CUs x 4 waves of 512 x 12 pixels (4096 x 3072 on MI355X) - mi_isp_pipeline12_whole_frame_fits
 * tells.  Results are within the tonemap tolerance of mi_isp_pipeline12_reinhard (same per-pixel functions).
 * The kernel occupies the whole device: launches on different streams of one device are serialised by the library;
 * do not capture two of them onto parallel branches of one HIP graph (the kernel would time out, set the error
 * word of mi_isp_workspace_error_offset and leave an invalid frame - it never hangs). */
int mi_isp_pipeline12_reinhard_whole_frame(const uint8_t* packed_dev, void* out_dev, int H, int W, int ids_format,
                                           int pattern, const float* ccm9_host, int out_dtype, float gamma,
                                           float intensity, float light_adapt, float color_adapt, void* ws_dev,
                                           void* stream);
int mi_isp_pipeline12_whole_frame_fits(int H, int W, int out_dtype);
/* n_frames frames (same size, parameters and pattern) through ONE launch of that kernel per 64 frames: the grid stays
 * resident and walks through the frames, so dispatch, the decode table, drain and launch gap are paid per launch, not
 * per frame (test/pipeline.py:26-32 per frame, as above).  packed_host / out_host: host arrays of n_frames device
 * pointers; ws_dev: n_frames consecutive workspaces (mi_isp_workspace_bytes each, zero-filled once), one per frame. */
int mi_isp_pipeline12_reinhard_whole_frame_batch(const uint8_t* const* packed_host, void* const* out_host, int n_frames,
                                                 int H, int W, int ids_format, int pattern, const float* ccm9_host,
                                                 int out_dtype, float gamma, float intensity, float light_adapt,
                                                 float color_adapt, void* ws_dev, void* stream);
/* What happens when the whole-frame kernel cannot have the chip to itself (a foreign kernel, another process): a wave
 * whose peers do not arrive within the poll budget gives up - the frame is INVALID, nothing hangs - and says so twice:
 *   - the frame's workspace: the 32-bit word at mi_isp_workspace_error_offset() is set (sticky until cleared);
 *   - a host-mapped mailbox word per device, visible to the host WITHOUT synchronising: mi_isp_whole_frame_faults().
 * mi_isp_workspace_check: synchronises `stream`, reports per frame whether its word is set (failed_host[i] = 0 / 1, may
 *   be NULL), clears the set words and returns their number in *n_failed.  The caller re-issues the failed frames
 *   through mi_isp_pipeline12_reinhard (the multi-pass chain needs no co-residency); taichi_image_amd.pipeline does.
 * mi_isp_whole_frame_faults(clear): the mailbox of the current device - non-zero when any whole-frame launch of this
 *   process on this device has timed out since it was last cleared; a plain host read.
 * mi_isp_whole_frame_set_poll_limit(polls): the poll budget of the following launches (0 = the default, ~100 ms);
 *   a diagnostic knob - tests/ use a budget of 1 to provoke the fault path. */
int mi_isp_workspace_check(void* ws_dev, int n_frames, int H, int W, int* failed_host, int* n_failed, void* stream);
int mi_isp_whole_frame_faults(int clear);
int mi_isp_whole_frame_set_poll_limit(unsigned polls);
/* Round 4.  A block one of whose barriers has timed out polls every later barrier of the launch ONCE: it walks through
 * the frames that are left (posting, so that nobody waits for it; marking the fault word of every frame whose records it
 * does not find), so a launch that lost one block ends after about one poll budget (~0.1 - 0.2 s) instead of one budget
 * per remaining barrier; mi_isp_workspace_check also wipes the barrier records of the frames it reports.
 * mi_isp_whole_frame_set_sabotage(block): test hook - that block of every later launch does not post its record at the
 *   first barrier of the launch's first frame (what a block that is not resident looks like to the others); -1 = off.
 * The resident-grid kernels of the library (this one, the one-launch metering, the camera group) are launched in
 * ONE order per device and process: a launch on another stream than the previous one waits for an event recorded behind
 * that one. */
int mi_isp_whole_frame_set_sabotage(int block);
/* The one-launch update_metering (mi_isp_metering) when ITS barrier times out: state9 is left exactly as it was, the
 * workspace's fault word is set and the device's metering mailbox word is stored to.
 * mi_isp_metering_faults(clear): that mailbox word of the current device - a plain host read, no synchronisation.
 * mi_isp_metering_set_poll_limit(polls): poll budget of the following launches (0 = default, ~1 s; tests use 1). */
int mi_isp_metering_faults(int clear);
int mi_isp_metering_set_poll_limit(unsigned polls);

/* The same for n_frames independent frames, frame i on streams_host[i % n_streams]
 * (one frame per stream in flight); ws_dev holds n_frames consecutive workspaces;
 * work_images_host: one scratch image per frame, or NULL. */
int mi_isp_pipeline12_reinhard_batch(const uint8_t* const* packed_host, void* const* out_host,
                                     void* const* work_images_host, int n_frames, int H, int W,
                                     int ids_format, int pattern,
                                     const float* ccm9_host, int work_dtype, int out_dtype,
                                     float gamma, float intensity, float light_adapt,
                                     float color_adapt, void* ws_dev, void* const* streams_host,
                                     int n_streams);


/* A batch of the chain above as a HIP graph (what hipStreamBeginCapture around mi_isp_pipeline12_reinhard_batch gives,
 * done inside the library): create() captures the step for the given buffers - fork to n_streams internal streams,
 * frame i on stream i % n_streams, join - and instantiates it; launch() replays it on `stream` (stream-ordered like any
 * other call; a replay has no launch gaps between the dependent kernels of a stream); destroy() frees it.  The buffers
 * must keep their addresses for the lifetime of the graph; ws_dev holds n_frames workspaces (zero-filled once).
 * whole_frame != 0: the frames through mi_isp_pipeline12_reinhard_whole_frame_batch (one launch, frames one after the other). */
int mi_isp_pipeline12_graph_create(const uint8_t* const* packed_dev, void* const* out_dev, void* const* work_images_dev,
                                   int n_frames, int H, int W, int ids_format, int pattern, const float* ccm9_host,
                                   int work_dtype, int out_dtype, float gamma, float intensity, float light_adapt,
                                   float color_adapt, void* ws_dev, int n_streams, int whole_frame, void** handle);
int mi_isp_pipeline12_graph_launch(void* handle, void* stream);
int mi_isp_pipeline12_graph_destroy(void* handle);

/* ---- measurement aid ----------------------------------------------------------------------- */
/* Launches ONE data pass (0 = demosaic + bounds, 1 = metering sums, 2 = Reinhard bounds, 3 = final
 * map + store) of mi_isp_pipeline12_reinhard, so that bench.py can time each kernel in isolation with
 * events on its own stream.  ws_dev must hold the scalars and per-block partials left by a previous
 * full mi_isp_pipeline12_reinhard call on the same frame (passes 1-3 fold their predecessor's
 * partials in their prologue). */
int mi_isp_pipeline12_pass(const uint8_t* packed_dev, void* out_dev, int H, int W, int ids_format,
                           int pattern, const float* ccm9_host, int work_dtype, int out_dtype,
                           float gamma, float light_adapt, float color_adapt, int pass,
                           void* ws_dev, void* stream);

/* Events around the four data passes of following mi_isp_pipeline12_reinhard[_batch] frames,
 * recorded on the stream each pass runs on.  enable(n, every): time every `every`-th frame, up to n
 * frames (n = 0: off); an event between two launches costs a gap on the stream, so sampling keeps
 * the measured run representative.  collect(): waits for the recorded events; avg_us[k] = average
 * duration of pass k in microseconds, *count = frames timed. */
int mi_isp_profile_enable(int max_frames, int every);
int mi_isp_profile_collect(float avg_us[4], int* count);

#ifdef __cplusplus
}
#endif
#endif /* MI_ISP_H */
