/*
 * vcf_amd.h -- C ABI of libvcf_amd.so, the MI355X (gfx950) implementation of
 * VCF's per-frame transform -> quantize hot path.
 *
 * The reference (Sistemas-Multimedia/VCF) is pure Python; its hot path is the
 * sequence of numpy/scipy calls inside src/2D-DCT.py encode_fn/decode_fn.
 * Each entry point below replaces a span of those calls and is what a
 * reference-side ctypes binding would bind:
 *
 *   vcf_dct_dz_encode  replaces src/2D-DCT.py:276-361
 *       astype(float32), pad_and_center (:187-229), -= 128 (:292),
 *       YCoCg.from_RGB (:298), DCT2D analyze_image (:303), -p weighting
 *       (:313-327), get_subbands (:333-336), deadzone quantize_fn
 *       (:343 -> src/deadzone.py:95-102), += 128 and astype(uint8) (:348,361)
 *   vcf_dct_dz_decode  replaces src/2D-DCT.py:399-466
 *       astype(int16) - 128 (:399-403), dequantize (:411 ->
 *       src/deadzone.py:107-117), get_blocks (:416), -p de-weighting
 *       (:421-435), DCT2D synthesize_image (:440), remove_padding (:444),
 *       YCoCg.to_RGB (:449), += 128 (:454), clip/astype(uint8) (:466)
 *
 * Conventions
 *   - Plain C, no C++ or torch types.  Every function returns VCF_OK (0) or a
 *     negative status; vcf_last_error() describes the last failure of the
 *     calling thread.
 *   - Buffers are caller-owned.  Pointers named *_dev are device (HBM)
 *     pointers, e.g. from vcf_malloc; the library never frees caller memory
 *     and keeps no reference after a call returns.
 *   - Frames are stored back to back.  An RGB frame is H x W x 3 uint8
 *     (row-major, channels interleaved, exactly the ndarray the reference's
 *     encode_read_fn returns).  A coefficient frame is Hp x Wp x 3 uint8 with
 *     Hp, Wp = H, W rounded up to the block size (vcf_dct_padded_shape): the
 *     array the reference hands to its entropy codec (2D-DCT.py:364).
 *   - Work is enqueued on `stream` (a hipStream_t, NULL = default stream)
 *     and is asynchronous; synchronise with vcf_stream_sync.  A call may run
 *     part of its work on library-owned streams, forked from and joined to
 *     `stream`, and may block the host while a workspace the library shares
 *     between calls grows.
 *   - Alignment and extents.  A byte-typed frame pointer (uint8_t *: images,
 *     index frames, luma workspaces) needs no alignment: a pointer into the
 *     middle of a larger allocation gives the same bytes, the kernels taking
 *     their byte paths where the address does not allow a wider access.  A
 *     typed pointer (int16_t, uint16_t, int32_t, float, double, int64_t)
 *     needs the alignment of its element; a misaligned one is VCF_ERR_INVALID
 *     before any device work, nothing written.  Every call writes only the
 *     bytes of the output extent its entry states, n_frames x the frame size
 *     from the pointer on unless said otherwise.  Stated per entry point for
 *     every transform, IPP, VQ and pixel entry below.  The 2D-DWT entries are
 *     the exception to the first rule: their kernels choose dword and wider
 *     accesses from the shape, so their three pointers need 16 bytes.
 */
#ifndef VCF_AMD_H
#define VCF_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VCF_OK 0
#define VCF_ERR_INVALID (-1)     /* bad argument (reference: ValueError)   */
#define VCF_ERR_HIP (-2)         /* HIP runtime failure                    */
#define VCF_ERR_UNSUPPORTED (-3) /* option not implemented on this path    */
#define VCF_ERR_TIMEOUT (-4)     /* a cross-rank exchange did not finish in time
                                    (the communicator is aborted)          */

/* element types of the stand-alone quantizer */
#define VCF_DTYPE_F32 0
#define VCF_DTYPE_F64 1
#define VCF_DTYPE_I16 2
#define VCF_DTYPE_I32 3
#define VCF_DTYPE_U8 4
#define VCF_DTYPE_U16 5

/* flags of the DCT path */
#define VCF_DCT_NO_SUBBANDS 1u   /* -x, --disable_subbands  (2D-DCT.py:40)  */
#define VCF_DCT_PERCEPTUAL 2u    /* -p, --perceptual_quantization (:38)    */

/* ---- runtime ----------------------------------------------------------- */
const char *vcf_last_error(void);
int vcf_version(int *major, int *minor);
int vcf_device_count(int *n);
int vcf_set_device(int device);
int vcf_get_device(int *device);
int vcf_device_sync(void);
int vcf_malloc(void **ptr_dev, size_t bytes);
int vcf_free(void *ptr_dev);
int vcf_host_alloc(void **ptr_host, size_t bytes); /* pinned */
int vcf_host_free(void *ptr_host);
int vcf_memcpy_htod(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int vcf_memcpy_dtoh(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int vcf_memcpy_dtod(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int vcf_memset(void *dst_dev, int value, size_t bytes, void *stream);
int vcf_stream_create(void **stream);
int vcf_stream_destroy(void *stream);
int vcf_stream_sync(void *stream);
int vcf_event_create(void **event);
int vcf_event_destroy(void *event);
int vcf_event_record(void *event, void *stream);
int vcf_event_sync(void *event);
/* n_pieces device copies in one launch: piece p moves table_dev[3p + 2] bytes
 * from src_dev + table_dev[3p] to dst_dev + table_dev[3p + 1] (int64 table in
 * device memory); e.g. per-frame code-streams packed for the gather */
int vcf_copy_pieces(const uint8_t *src_dev, const int64_t *table_dev, int64_t n_pieces, uint8_t *dst_dev,
                    void *stream);
/* later work on `stream` waits for `event` (hipStreamWaitEvent) */
int vcf_stream_wait_event(void *stream, void *event);
int vcf_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---- DCT + deadzone path (2D-DCT.py, deadzone.py, YCoCg.py) ---------------- */

/* Hp, Wp for an H x W frame: 2D-DCT.py:208-209. */
int vcf_dct_padded_shape(int32_t H, int32_t W, int32_t block_size, int32_t *Hp, int32_t *Wp);

/* n_frames RGB frames (H x W x 3 u8 each) -> n_frames coefficient frames
 * (Hp x Wp x 3 u8 each, k + 128 modulo 256, subband layout unless
 * VCF_DCT_NO_SUBBANDS).  block_size is the -B option (2D-DCT.py:29): 8 runs
 * the fused 8x8 kernels, the other supported sizes (vcf_dct_block_size_supported)
 * the generic-B kernels; VCF_DCT_PERCEPTUAL takes any supported B (B != 8
 * through vcf_dct_perceptual_tables' resized tables).  Q >= 1 is the
 * deadzone quantization step (-q).  rgb_dev and k_dev need no alignment (the
 * 8x8 kernels move 8-byte RGB words only when rgb_dev is 8-byte aligned and
 * 16-byte index chunks only when k_dev is 16-byte aligned, bytes otherwise);
 * writes the n_frames * Hp * Wp * 3 bytes at k_dev. */
int vcf_dct_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W,
                      int32_t block_size, int32_t Q, uint32_t flags, uint8_t *k_dev,
                      void *stream);



/* Inverse: n_frames coefficient frames (Hp x Wp x 3) -> RGB frames (H x W x 3),
 * the padding removed.  1 <= Q <= 32767 (the dequantizer works in int16).
 * k_dev and rgb_dev need no alignment, as for the encode; writes the n_frames *
 * H * W * 3 bytes at rgb_dev. */
int vcf_dct_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W,
                      int32_t block_size, int32_t Q, uint32_t flags, uint8_t *rgb_dev,
                      void *stream);

/* ---- lapped 2D-MDCT + deadzone path (2D-MDCT.py) ---------------------------- */

/* Padded shape and the pads stored in {out}_shape.bin (2D-MDCT.py:446-476):
 * Hp = ceil((H + 2B) / B) * B (one extra block of context per side), pad_top =
 * (Hp - H) / 2, likewise for the width.  Host only.  2 <= block_size <= 64,
 * else VCF_ERR_UNSUPPORTED. */
int vcf_mdct_padded_shape(int32_t H, int32_t W, int32_t block_size, int32_t *Hp, int32_t *Wp, int32_t *pad_top,
                          int32_t *pad_left);

/* The launch plan vcf_mdct_dz_encode (decode = 0) or vcf_mdct_dz_decode (decode
 * != 0) uses for this shape, block size and flags: the workgroup's tile in
 * blocks (decode: output segments) TX x TY, the LDS class (0, 1, 2: 40, 80,
 * 156 KiB per workgroup) and the number of tiles each way.  Computed by the
 * code the launches call.  Host only; the shape, block size and flag rules of
 * vcf_mdct_dz_encode. */
int vcf_mdct_tile_plan(int32_t H, int32_t W, int32_t block_size, uint32_t flags, int32_t decode, int32_t *TX,
                       int32_t *TY, int32_t *lds_class, int32_t *tiles_x, int32_t *tiles_y);

/* 2D-MDCT.py encode_fn :498-582 between the image read and the entropy codec:
 * n_frames RGB frames (H x W x 3 u8) -> coefficient frames (Hp x Wp x 3 u8 of
 * vcf_mdct_padded_shape): centred symmetric pad, -128, YCoCg, Malvar's lapped
 * transform (rows, then columns, float64), / scale, deadzone with step Q,
 * +128, CLIPPED to [0, 255] (not the DCT path's wrap); subband layout unless
 * VCF_DCT_NO_SUBBANDS.  Every 2 <= block_size <= 64 (else VCF_ERR_UNSUPPORTED),
 * H, W >= 1 (frames smaller than a block are legal), 1 <= Q <= 32767.
 * VCF_DCT_PERCEPTUAL is taken at block_size 8 only, where the reference's
 * cv2.resize of the JPEG tables is the identity; at other sizes it returns
 * VCF_ERR_UNSUPPORTED: cv2 is not available to pin the resized tables.
 * Argument errors are reported before any device work.  The frames need no
 * alignment (byte loads and stores); writes the n_frames * Hp * Wp * 3 bytes
 * at k_dev. */
int vcf_mdct_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                       int32_t Q, uint32_t flags, uint8_t *k_dev, void *stream);

/* The inverse, 2D-MDCT.py decode_fn :587-666: coefficient frames -> RGB frames
 * with the padding removed (int16 dequantizer, synthesis columns first, then
 * rows, no boundary extension, * scale, RGB in float32, +128, clip, truncate).
 * Same argument rules as vcf_mdct_dz_encode; the frames need no alignment;
 * writes the n_frames * H * W * 3 bytes at rgb_dev. */
int vcf_mdct_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                       int32_t Q, uint32_t flags, uint8_t *rgb_dev, void *stream);

/* ---- 2D-KLT (2D-KLT.py) --------------------------------------------------
 * A Karhunen-Loeve basis of the B x B blocks, learned per frame and colour
 * channel: D = B * B values per block, N blocks per frame after the pad.
 * Common to the three device entry points: arguments are checked before any
 * device work; 2 <= block_size <= 16 (17 and up: VCF_ERR_UNSUPPORTED; 1, where
 * the reference's covariance is a scalar: VCF_ERR_INVALID); H, W >= 1 with
 * N >= 2 (a frame of one block has no covariance: VCF_ERR_INVALID);
 * n_frames >= 1; work is enqueued on the caller's stream. */

/* Padded frame shape of 2D-KLT.py:393-411: Hp = ceil(H / B) * B, centred zero
 * pad with pad_top = (Hp - H) / 2 (the rest below), likewise for the width.
 * Host only. */
int vcf_klt_padded_shape(int32_t H, int32_t W, int32_t block_size, int32_t *Hp, int32_t *Wp, int32_t *pad_top,
                         int32_t *pad_left);

/* Exact second moments of the blocks: per frame and channel S1 (int64[D]) =
 * sum of s and S2 (int64[D][D], full symmetric) = sum of s s^T over the N
 * blocks, s = 4 x, x = the YCoCg value after the zero pad and -128 (s is an
 * integer, |s| <= 512).  s1_dev: n_frames x 3 x D, s2_dev: n_frames x 3 x D x
 * D.  Integer arithmetic throughout: the result does not depend on tiling,
 * order or batch.  The covariance is (S2 - S1 S1^T / N) / (16 (N - 1)).
 * rgb_dev needs no alignment; s1_dev and s2_dev must be 8-byte aligned
 * (VCF_ERR_INVALID before any device work) and are written whole, nothing else. */
int vcf_klt_moments(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                    int64_t *s1_dev, int64_t *s2_dev, void *stream);

/* 2D-KLT.py encode_fn :515-628 between the image read and the entropy codec,
 * with the basis given: weights_f64_dev is n_frames x 3 x D x D float64, row k
 * = basis vector k.  Zero pad, -128, YCoCg, coef[k] = sum_j W[k][j] x[j] in
 * float64 (j ascending, FMA), / Q (float64 division), truncated, +128,
 * WRAPPED to u8 (not clipped); subband layout unless VCF_DCT_NO_SUBBANDS (the
 * only flag).  1 <= Q <= 32767.  k_dev: n_frames x Hp x Wp x 3, the bytes
 * written.  The frames need no alignment; weights_f64_dev must be 8-byte
 * aligned (VCF_ERR_INVALID before any device work). */
int vcf_klt_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const double *weights_f64_dev, uint8_t *k_dev, void *stream);

/* The inverse, 2D-KLT.py decode_fn :738-809: weights_f32_dev is n_frames x 3 x
 * D x D float32 as stored in {out}_weights.npz, widened on the device;
 * rec[j] = sum_k W[k][j] (Q (k - 128)) (int16 dequantizer; k ascending, FMA),
 * inverse YCoCg and +128 in float64, clip, truncate, padding removed.  The
 * frames need no alignment; weights_f32_dev must be 4-byte aligned
 * (VCF_ERR_INVALID before any device work); writes the n_frames * H * W * 3
 * bytes at rgb_dev. */
int vcf_klt_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const float *weights_f32_dev, uint8_t *rgb_dev, void *stream);

/* ---- 2D-LBT (2D-LBT.py) --------------------------------------------------
 * A linear autoencoder of the B x B blocks (D = B * B), trained per frame with
 * Adam on mean((x^ - x)^2) + lambda mean_j log(var_j(y) + 1e-6); the rows are
 * the blocks of all three YCoCg channels minus one scalar mean.  The model is
 * linear, so the training reads the frame once (the moments) and then works
 * on D x D matrices.  2 <= block_size <= 8 (else VCF_ERR_UNSUPPORTED);
 * arguments are checked before any device work; work is enqueued on the
 * caller's stream.  The padded shape is vcf_klt_padded_shape's. */

/* The launch plan for this shape and block size, computed by the code the
 * launches call: TB, the blocks of a frame and channel that one workgroup of
 * vcf_lbt_dz_encode (decode = 0) or vcf_lbt_dz_decode (decode != 0) owns; the
 * LDS class of that kernel (0, 1, 2: 48, 80, 156 KiB per workgroup); the
 * workgroups (tiles) per frame; and for vcf_lbt_moments the workgroups per
 * frame and channel (chunks of 2048 blocks) and the blocks one of them stages
 * in LDS at a time.  Host only; the shape and block size rules of
 * vcf_lbt_dz_encode. */
int vcf_lbt_tile_plan(int32_t H, int32_t W, int32_t block_size, int32_t decode, int32_t *TB, int32_t *lds_class,
                      int32_t *tiles, int32_t *moment_chunks, int32_t *moment_stage_blocks);

/* Per frame, pooled over the three channels: s1_dev (n_frames x D float64) =
 * sum of x, s2_dev (n_frames x D x D float64, full symmetric) = sum of x x^T
 * over the 3 N blocks, x = the YCoCg values after the zero pad and -128.
 * Every partial sum is an integer multiple of 1/16 below 2^53: exact, in any
 * order.  Each frame is read once; no float copy of it is written.  rgb_dev
 * needs no alignment; s1_dev and s2_dev must be 8-byte aligned (VCF_ERR_INVALID
 * before any device work) and are written whole, nothing else. */
int vcf_lbt_moments(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                    double *s1_dev, double *s2_dev, void *stream);

/* 2D-LBT.py:94-128 from the moments: `epochs` steps of torch.optim.Adam
 * (defaults; learning rate lr) over both matrices, all in one launch, one
 * workgroup per frame.  rows = 3 N, the number of blocks the moments were
 * summed over.  we_dev / wd_dev: n_frames x D x D float32, the initial weights
 * in, the trained ones out (nn.Linear layout: y = We x, x^ = Wd y).  mean_dev:
 * n_frames float32, the scalar mean.  loss_dev: n_frames x 3 float32: the
 * loss at the final weights, its MSE term and mean_j log(var_j + 1e-6).
 * float32 products on the matrix cores, inner index ascending. */
int vcf_lbt_train(const double *s1_dev, const double *s2_dev, int64_t n_frames, int32_t block_size, int64_t rows,
                  int32_t epochs, double lr, double lambda, float *we_dev, float *wd_dev, float *mean_dev,
                  float *loss_dev, void *stream);

/* 2D-LBT.py encode_fn :364-452 with the encoder matrix given: zero pad, -128,
 * YCoCg, x - mean (float32), y[k] = sum_j We[k][j] x[j] (float32 FMAs, j
 * ascending), with VCF_DCT_PERCEPTUAL * (QSSs / 121 or 99) as a float64
 * product rounded to float32, / Q (float32), truncated, +128, clipped to
 * 0..255; subband layout unless VCF_DCT_NO_SUBBANDS.  we_dev: n_frames x D x D,
 * mean_dev: n_frames.  k_dev: n_frames x Hp x Wp x 3, the bytes written.  The
 * frames need no alignment; we_dev and mean_dev must be 4-byte aligned
 * (VCF_ERR_INVALID before any device work). */
int vcf_lbt_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const float *we_dev, const float *mean_dev, uint8_t *k_dev, void *stream);

/* The inverse, 2D-LBT.py decode_fn :476-563 with the stored decoder matrix as
 * it is: Q (k - 128) in int16 (with VCF_DCT_PERCEPTUAL divided by the weight
 * in float64 and truncated back into int16), x[j] = sum_k Wd[j][k] y[k]
 * (float32 FMAs, k ascending), + mean, crop, inverse YCoCg and +128 in
 * float32, clip, truncate.  The frames need no alignment; wd_dev and mean_dev
 * must be 4-byte aligned (VCF_ERR_INVALID before any device work); writes the
 * n_frames * H * W * 3 bytes at rgb_dev. */
int vcf_lbt_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const float *wd_dev, const float *mean_dev, uint8_t *rgb_dev, void *stream);

/* 1 if block_size has a HIP transform: every 1 <= B <= 4096 -- compiled
 * kernels for the 38 5-smooth B <= 128 (every -L candidate 2, 4, ..., 128,
 * 2D-DCT.py:536), run-time-length kernels for the rest: rfftp plans with the
 * generic radfg/radbg passes, and the lengths pocketfft_r plans with
 * Bluestein (191, 199, 211, ...: fftblue over cfftp).  0 for B > 4096. */
int vcf_dct_block_size_supported(int32_t block_size);

/* -p's quantization tables for block size B (host only): the JPEG luma /
 * chroma tables of 2D-DCT.py:66-84 resized to B x B as :85-90 does
 * (cv2.resize, INTER_AREA for B < 8, INTER_LINEAR otherwise), B*B bytes each.
 * cv2 is not installed here: OpenCV's scalar resize code paths are restated,
 * unpinned by any reference output (parity unpinned for -p with B != 8). */
int vcf_dct_perceptual_tables(int32_t block_size, uint8_t *y_qss, uint8_t *c_qss);

/* The generic-B kernels for any supported block size, B = 8 included (tests
 * and A/B checks against the fused 8x8 kernels); same contract as
 * vcf_dct_dz_encode / vcf_dct_dz_decode, alignment (none needed: byte loads and
 * stores) and output extent included. */
int vcf_dct_dz_encode_any(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                          int32_t Q, uint32_t flags, uint8_t *k_dev, void *stream);
int vcf_dct_dz_decode_any(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                          int32_t Q, uint32_t flags, uint8_t *rgb_dev, void *stream);

/* The -L rate-distortion search's own analysis/synthesis
 * (2D-DCT.py optimize_block_size :533-579), which differs from
 * encode_fn/decode_fn in its integer types and offset.  The search runs from
 * CoDec.__init__ (:99-103) before the deadzone offset 128 is assigned
 * (:106-109), so its self.offset is YCoCg's [0, 0, 0] (YCoCg.py:28-29):
 *   encode_k32: astype(float32) (no -128), from_RGB, analyze, get_subbands,
 *     quantize (:536-545) -> the int32 k array (Hp x Wp x 3 int32);
 *   decode_k32: Q*k in int32 (:561), get_blocks, the IDCT stored into int32,
 *     to_RGB in int32 (no +128), clip, uint8 (:562-568).
 * No VCF_DCT_PERCEPTUAL (the reference refuses -L with -p, :100-105).  The u8
 * frames need no alignment; the int32 k_dev must be 4-byte aligned
 * (VCF_ERR_INVALID before any device work).  Written: n_frames * Hp * Wp * 3
 * int32 at k_dev, or n_frames * H * W * 3 bytes at rgb_dev. */
int vcf_dct_dz_encode_k32(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                          int32_t Q, uint32_t flags, int32_t *k_dev, void *stream);
int vcf_dct_dz_decode_k32(const int32_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                          int32_t Q, uint32_t flags, uint8_t *rgb_dev, void *stream);

/* encode_fn / decode_fn with a quantizer other than deadzone (-a LloydMax):
 * 2D-DCT.py:106-109 sets self.offset = 0, so there is no -128 before the
 * colour transform and no +128 on the pixels; the quantizer sees the float32
 * coefficients (subband layout unless -x, -p weights applied, :313-340) and
 * hands back int16 coefficients (:399-410).  Replaces the same spans as
 * vcf_dct_dz_encode/decode minus the deadzone quantizer; any supported B.  The
 * u8 frames need no alignment; coef_dev must be aligned to its element, 4
 * bytes (float, encode) or 2 (int16, decode), else VCF_ERR_INVALID before any
 * device work.  Written: n_frames * Hp * Wp * 3 floats at coef_dev, or n_frames
 * * H * W * 3 bytes at rgb_dev. */
int vcf_dct_raw_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                       uint32_t flags, float *coef_dev, void *stream);
int vcf_dct_raw_decode(const int16_t *coef_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                       uint32_t flags, uint8_t *rgb_dev, void *stream);



/* ---- 2D-DWT + deadzone path (2D-DWT.py, deadzone.py, YCoCg.py) ---------------- */

/* Index of a pywt wavelet name ("db5", "bior4.4", ... -- the -w option,
 * 2D-DWT.py:45) in the library's filter table. */
int vcf_wavelet_index(const char *name, int32_t *index);

/* Subband shapes (level l = 1..levels in sub_h[l-1], sub_w[l-1]; mode 'per'
 * halves with ceil), bytes of one frame's packed subbands, and the device
 * workspace one frame needs.  Any output pointer may be NULL. */
int vcf_dwt_layout(int32_t H, int32_t W, int32_t levels, int32_t *sub_h, int32_t *sub_w, int64_t *packed_bytes,
                   int64_t *workspace_bytes_per_frame);

/* n_frames RGB frames -> n_frames packed subband sets, each laid out in the
 * order 2D-DWT.py's write_decom_fn (:162-200) writes its files: LL_L
 * (uint16 little-endian, h_L x w_L x 3, k + 128 wrapped), then for r = L..1
 * LH_r, HL_r, HH_r (uint8, h_r x w_r x 3, k + 128 wrapped).  Replaces
 * 2D-DWT.py:57-78 up to the TIFF writer: astype(int16), from_RGB (:62),
 * pywt.wavedec2 mode 'per' per channel (:64), quantize_decom_fn (:67).
 * workspace_dev: n_frames * workspace_bytes_per_frame bytes.  rgb_dev,
 * packed_dev and workspace_dev must be 16-byte aligned (VCF_ERR_INVALID before
 * any device work); frames follow at the frame size and the packed size, odd
 * sizes included (a frame's u16 LL band at an odd address is moved by bytes).
 * Writes the n_frames * packed_bytes bytes at packed_dev and the workspace. */
int vcf_dwt_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t wavelet,
                      int32_t levels, int32_t Q, uint8_t *packed_dev, void *workspace_dev, void *stream);

/* Inverse: packed subbands -> RGB frames of 2*ceil(H/2) x 2*ceil(W/2) x 3
 * (what pywt.waverec2 returns; the reference writes that size too).
 * Replaces 2D-DWT.py:80-101 after the TIFF reader.  1 <= Q <= 32767.
 * Coarsest subbands shorter than filter_length/2 (pywt's short-input code
 * path) run on the separable kernels.  packed_dev, rgb_dev and workspace_dev
 * must be 16-byte aligned (VCF_ERR_INVALID before any device work), as for the
 * encode; writes the n_frames * 2*ceil(H/2) * 2*ceil(W/2) * 3 bytes at rgb_dev
 * and the workspace. */
int vcf_dwt_dz_decode(const uint8_t *packed_dev, int64_t n_frames, int32_t H, int32_t W, int32_t wavelet,
                      int32_t levels, int32_t Q, uint8_t *rgb_dev, void *workspace_dev, void *stream);

/* What vcf_dwt_dz_encode / _decode launch for a call of these arguments, from
 * the code the launches themselves consult (host only, no device work).  For
 * level l = 1..levels, enc_kind[l-1] / dec_kind[l-1] is the kernel family
 * below (a kernel that covers two levels is reported on both), and enc_ct[l-1]
 * / dec_ct[l-1] the compile-time tap set of the instantiation: 0 = taps read
 * at run time, 1 = bior4.4's, 2 = db5's.  n_frames is validated as the calls
 * validate it; the families do not depend on it. */
#define VCF_DWT_ENC_SEPARABLE 0        /* column pass + row pass, any filter length */
#define VCF_DWT_ENC_FUSED 1            /* one tile kernel per level, F <= 18 */
#define VCF_DWT_ENC_STRIP 2            /* sliding-window strips, F <= 10, levels between first and last */
#define VCF_DWT_ENC_BAND12 3           /* levels 1 + 2 in one launch */
#define VCF_DWT_DEC_SEPARABLE 0
#define VCF_DWT_DEC_SEPARABLE_SHORT 1  /* separable, this level's subbands shorter than F/2 (pywt's short-input branch) */
#define VCF_DWT_DEC_FUSED 2
#define VCF_DWT_DEC_LINE 3             /* line-based inverse level */
#define VCF_DWT_DEC_BAND21 4           /* inverse levels 2 + 1 in one launch */
int vcf_dwt_plan(int32_t H, int32_t W, int32_t wavelet, int32_t levels, int64_t n_frames, int32_t *enc_kind,
                 int32_t *enc_ct, int32_t *dec_kind, int32_t *dec_ct);

/* Opt-in lifting form of the two calls above for bior4.4 (CDF 9/7) only
 * (VCF_ERR_INVALID for other wavelets): same arguments, buffers, layout and
 * workspace, four lifting steps per axis in place of pywt's convolution.
 * NOT bit-exact: every index and decoded byte lies within +-1 of
 * vcf_dwt_dz_encode / _decode's (measured, DESIGN.md §4.5, the lifting form).  No counterpart
 * in the reference -- an extension for callers who accept that tolerance.
 * Alignment (16 bytes for the three pointers) and output extents as for
 * vcf_dwt_dz_encode / _decode. */
int vcf_dwt_dz_encode_lift(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t wavelet,
                           int32_t levels, int32_t Q, uint8_t *packed_dev, void *workspace_dev, void *stream);
int vcf_dwt_dz_decode_lift(const uint8_t *packed_dev, int64_t n_frames, int32_t H, int32_t W, int32_t wavelet,
                           int32_t levels, int32_t Q, uint8_t *rgb_dev, void *workspace_dev, void *stream);
/* Diagnostic of the lifting form's precision (one frame, bior4.4): its float64
 * subband coefficients before quantization.  coef_dev receives, for levels
 * l = 1..levels, the details [LH, HL, HH][Y, Co, Cg][h_l x w_l] (the shapes of
 * vcf_dwt_layout), then LL_levels [Y, Co, Cg][h x w]; packed_dev (packed bytes
 * of vcf_dwt_layout) and workspace_dev are scratch. */
int vcf_dwt_lift_analyze_f64(const uint8_t *rgb_dev, int32_t H, int32_t W, int32_t levels, double *coef_dev,
                             uint8_t *packed_dev, void *workspace_dev, void *stream);



/* ---- IPP temporal tools (IPP_DCT.py) --------------------------------------------- */

/* Motion field of cur against ref (H x W x 3 u8 each): IPP.block_matching
 * (IPP_DCT.py:344-376) -- cv2 RGB2GRAY (A10), then per bs x bs block of the
 * full-block area the (dx, dy) of the full search (fast = 0,
 * _process_block_row :207-246) or the three-step search (fast = 1,
 * _three_step_search :159-204) over [-sr, sr].  mv_dev: (H/bs) x (W/bs) x 2
 * float32; gray_workspace_dev: 2*H*W bytes.  bs <= 64, sr <= 32.
 * Kernels: the full search runs on 4-pixel words (v_alignbyte + v_sad_u8,
 * one lane per candidate) when bs % 4 == 0 and byte by byte otherwise; the
 * three-step search runs its 8 neighbours in parallel rounds for bs = 16 and
 * one candidate at a time otherwise.  Identical motion fields either way
 * (vcf_ipp_block_match_variant of the A/B library picks per call).  The frames
 * and gray_workspace_dev need no alignment (the bs = 16 three-step kernel reads
 * whole luma words only from a 4-byte aligned workspace); mv_dev must be
 * 4-byte aligned (VCF_ERR_INVALID before any device work).  Written: the
 * (H/bs) * (W/bs) * 2 floats at mv_dev and the 2*H*W workspace bytes. */
int vcf_ipp_block_match(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                        int32_t sr, int32_t fast, float *mv_dev, uint8_t *gray_workspace_dev, void *stream);

/* IPP.motion_compensate (IPP_DCT.py:378-395).  The frames need no alignment;
 * mv_dev must be 4-byte aligned (VCF_ERR_INVALID before any device work);
 * writes the H * W * 3 bytes at out_rgb_dev. */
int vcf_ipp_motion_compensate(const uint8_t *ref_rgb_dev, const float *mv_dev, int32_t H, int32_t W, int32_t bs,
                              uint8_t *out_rgb_dev, void *stream);

/* Sub-pel motion (--subpel; not in the reference).  Integers throughout.
 * Vectors are in quarter-pel units q = (qx, qy), stored as float32 q / 4
 * (exact).  A block at (i, j) of side bs reads the reference from
 * X = 4 j + qx: ix = X >> 2 (arithmetic shift: floor), fx = X & 3; iy, fy the
 * same from 4 i + qy.  Prediction sample (luma and each RGB channel alike),
 * with a = r[y, x], b = r[y, x+1], c = r[y+1, x], d = r[y+1, x+1]:
 *   p = ((4-fx)(4-fy) a + fx (4-fy) b + (4-fx) fy c + fx fy d + 8) >> 4;
 * a tap whose weight is 0 is not read, fx = fy = 0 is the plain copy.  A
 * vector is valid iff every sample it reads lies in the frame: ix >= 0,
 * ix + bs + (fx ? 1 : 0) <= W, and the same for y with H.
 * Search for precision N = subpel in {1, 2, 4}: stage 0 is
 * vcf_ipp_block_match's integer search (same kernels, same tie rule); its
 * vector times 4 is the centre.  N >= 2: a stage with step = 2 scans the 8
 * neighbours centre + (ddx, ddy), ddx, ddy in {-step, 0, +step}, ddy outer
 * and ddx inner; invalid neighbours are skipped; a neighbour's SAD is the
 * interpolated reference luma (the u8 luma of the gray pass, interpolated)
 * against the current luma; the winner is the argmin of (SAD, index) with the
 * centre at index 0 and the neighbours 1..8 in scan order.  N = 4: a second
 * stage with step = 1 around the first stage's winner.  N = 1 writes exactly
 * what vcf_ipp_block_match writes.
 * Kernel: one wave per block after the integer search, the block and the
 * (bs + 2)^2 luma window around the integer winner in LDS, both stages in the
 * one launch.  Limits and alignment as vcf_ipp_block_match: bs <= 64,
 * sr <= 32, mv_dev 4-byte aligned, the frames and the workspace unaligned;
 * a violation, or subpel outside {1, 2, 4}, is VCF_ERR_INVALID before any
 * device work.  Written: the (H/bs) * (W/bs) * 2 floats at mv_dev and the
 * 2*H*W workspace bytes. */
int vcf_ipp_block_match_subpel(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                               int32_t sr, int32_t fast, int32_t subpel, float *mv_dev, uint8_t *gray_workspace_dev,
                               void *stream);

/* Hierarchical motion search (--me_levels; not in the reference).  Integers
 * throughout; it changes only which vectors the encoder chooses.
 * Level 0 is the u8 luma plane of the gray pass (A10), H_0 = H, W_0 = W.
 * Level l + 1 has H_{l+1} = H_l >> 1, W_{l+1} = W_l >> 1 and
 *   g_{l+1}[y, x] = (g_l[2y, 2x] + g_l[2y, 2x+1] + g_l[2y+1, 2x] + g_l[2y+1, 2x+1] + 2) >> 2
 * (an odd last row or column is dropped); ref and cur both get a pyramid.
 * levels = L in 0..3; L > 0 needs bs % (1 << L) == 0 and (bs >> L) >= 2.
 * Block (by, bx) has side b_l = bs >> l and origin (by b_l, bx b_l) at level
 * l; the field is the usual (H/bs) x (W/bs).  Every level-l block of a full
 * level-0 block lies inside plane l: (by + 1) bs <= H gives
 * (by + 1) b_l = ((by + 1) bs) >> l <= H >> l = H_l (bs is a multiple of 2^l),
 * columns alike.  A candidate (dx, dy) at level l is valid iff the displaced
 * b_l x b_l block lies inside plane l (H_l, W_l).
 * Top level L: vcf_ipp_block_match's full search (same kernels, candidate
 * order dy outer / dx inner from -sr, validity and first-strict-minimum tie
 * rule) on the level-L planes with block side b_L and range sr -> v_L.
 * Level l = L-1 .. 0: the centre is c = 2 v_{l+1}; it is valid, because
 * 0 <= y and y + b_{l+1} <= H_{l+1} give 0 <= 2y and 2y + b_l <= 2 H_{l+1} <= H_l.
 * The candidates are c + (ddx, ddy), ddx, ddy in {-1, 0, 1}; the winner v_l is
 * the argmin of (SAD, index) with the centre at index 0 and the 8 neighbours
 * 1..8 in ddy-outer / ddx-inner order, invalid neighbours skipped; SAD is the
 * sum of |g^ref_l - g^cur_l| over the block.  v_0 is written as float32
 * (dx, dy): it lies within +-(sr 2^L + 2^L - 1).  subpel in {2, 4}: 4 v_0 is
 * the centre of the sub-pel stages above, which do not change.  L = 0 writes
 * exactly what vcf_ipp_block_match (fast = 0) / vcf_ipp_block_match_subpel
 * write.  The three-step search is not offered under L > 0.
 * Workspace (vcf_ipp_hier_workspace_bytes; VCF_ERR_INVALID for H, W <= 0 or
 * levels outside 0..3): sum over l = 0..L of 2 H_l W_l bytes -- level by
 * level, ref's plane then cur's, back to back without padding, so the first
 * 2*H*W bytes are the two gray planes as in vcf_ipp_block_match.  No
 * per-level vectors are kept: the top level writes its field to mv_dev and
 * the refinement rewrites it in place.
 * Kernels: one pyramid launch per level (both frames; 4 output bytes per lane
 * from two rows of 8, read as words where aligned), the full-search kernels
 * on the top planes, one refinement launch for all of L-1 .. 0 (one wave per
 * block; the block and the (b_l + 2)^2 window in LDS as words, v_alignbyte +
 * v_sad_u8 where b_l % 4 == 0 and bytes otherwise, the 9 sums reduced three
 * to a 64-bit word), then the sub-pel kernel when subpel > 1.
 * Limits and alignment as vcf_ipp_block_match_subpel: bs <= 64, sr <= 32
 * (at the top level), mv_dev 4-byte aligned, the frames and the workspace
 * unaligned.  VCF_ERR_INVALID before any device work for a violation, levels
 * outside 0..3, a bad bs / levels pair, subpel outside {1, 2, 4},
 * workspace_bytes below the size function's, or a null pointer.  Written: the
 * (H/bs) * (W/bs) * 2 floats at mv_dev and the first
 * vcf_ipp_hier_workspace_bytes bytes of the workspace; an empty field (H < bs
 * or W < bs) is legal and writes nothing. */
int vcf_ipp_hier_workspace_bytes(int32_t H, int32_t W, int32_t levels, int64_t *bytes);
int vcf_ipp_block_match_hier(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                             int32_t sr, int32_t levels, int32_t subpel, float *mv_dev, uint8_t *workspace_dev,
                             int64_t workspace_bytes, void *stream);

/* Compensation of an arbitrary float field under the sub-pel rule above:
 * q = lrintf(4 m) per component; an invalid vector falls back to the
 * co-located block, pixels outside the full-block area are 0 (both as
 * vcf_ipp_motion_compensate); for integer-valued fields the output equals
 * vcf_ipp_motion_compensate's bit for bit.  The frames need no alignment (a
 * 4-byte aligned reference is read in words, an aligned output written in
 * words); mv_dev must be 4-byte aligned (VCF_ERR_INVALID before any device
 * work); H <= 65535.  Writes the H * W * 3 bytes at out_rgb_dev. */
int vcf_ipp_motion_compensate_qpel(const uint8_t *ref_rgb_dev, const float *mv_dev, int32_t H, int32_t W, int32_t bs,
                                   uint8_t *out_rgb_dev, void *stream);

/* Overlapped block motion compensation (--obmc; not in the reference).
 * Integers throughout.  r is the H x W x 3 u8 reference, mv the (H/bs) x (W/bs)
 * x 2 float32 field (dx, dy), bs in {4, 8, 16, 32, 64}; nby = H / bs,
 * nbx = W / bs.
 * 1. Block vectors in quarter pels: q = rint(4 m) per component (half to even),
 *    clamped to +-2^28, a NaN gives -2^28 (as vcf_ipp_motion_compensate_qpel).
 *    The vector of block (by, bx) is valid iff it is valid under "Sub-pel
 *    motion" for the block's own origin (i, j) = (by bs, bx bs), X = 4 j + qx,
 *    Y = 4 i + qy.  An invalid vector is replaced by (0, 0) everywhere the
 *    block contributes.
 * 2. Sample: P(q; y, x) is the bilinear sample of "Sub-pel motion" at
 *    X = 4 x + qx, Y = 4 y + qy: ix = X >> 2, fx = X & 3, iy, fy alike, weights
 *    (4-fx)(4-fy), fx (4-fy), (4-fx) fy, fx fy, rounded with + 8 >> 4.  Each of
 *    the four tap coordinates is clamped to the frame: rows clamp(iy, 0, H-1)
 *    and clamp(iy+1, 0, H-1), columns alike with W.  A valid vector at a pixel
 *    of its own block never clamps, so P equals the sub-pel compensator's sample
 *    there; a neighbour's vector, applied up to bs/2 pixels outside its own
 *    block, may clamp.
 * 3. Contributors of pixel (y, x) of block (by, bx), v = y - by bs,
 *    u = x - bx bs: the horizontal neighbour is block column bx - 1 if
 *    u < bs/2, else bx + 1, clamped to [0, nbx-1] (at a frame-border block the
 *    neighbour is the block itself); the vertical neighbour row alike from v
 *    and nby; the diagonal contributor is the block at (vertical neighbour row,
 *    horizontal neighbour column).
 * 4. Weights: the own weight is wx = bs + 2u + 1 if u < bs/2, else
 *    3 bs - 2u - 1; the neighbour's is 2 bs - wx.  wy alike from v.
 * 5. Blend, per channel: acc = sum over the four (row a, column b) choices of
 *    wy_a wx_b P(q[a, b]; y, x); out = (acc + 2 bs^2) >> (2 log2(bs) + 2).
 *    acc <= 255 * 4 * 64^2 fits in 32 bits.
 * 6. Pixels with y >= nby bs or x >= nbx bs are 0, as in the other compensators.
 * Where the four contributors of a pixel carry the same vector the output
 * equals vcf_ipp_motion_compensate_qpel's; a uniform valid field, or a
 * single-block frame, reproduces that compensator byte for byte.
 * Kernel: a thread makes 4 consecutive bytes of a row, as the quarter-pel
 * kernel does; a workgroup first resolves step 1 for its two block rows into
 * LDS, once per block; samples come from aligned words where the reference is
 * 4-byte aligned and no tap clamps, else byte by byte.
 * The frames need no alignment; mv_dev must be 4-byte aligned.
 * VCF_ERR_INVALID before any device work for a null buffer, a misaligned
 * mv_dev, H or W <= 0, or bs outside {4, 8, 16, 32, 64}; VCF_ERR_UNSUPPORTED
 * for H > 65535.  Writes the H * W * 3 bytes at out_rgb_dev; an empty field
 * (nby or nbx = 0) yields a zero frame and mv_dev is not read. */
int vcf_ipp_motion_compensate_obmc(const uint8_t *ref_rgb_dev, const float *mv_dev, int32_t H, int32_t W, int32_t bs,
                                   uint8_t *out_rgb_dev, void *stream);

/* Coded motion fields (--mvc, --mv_lambda; not in the reference).  Integers
 * throughout.  A vector is q = (qx, qy) in quarter pels, stored as float32
 * q / 4 as above; step = 4 / subpel for subpel in {1, 2, 4}; a field F is
 * nby x nbx = (H/bs) x (W/bs) vectors.  A float field entry becomes quarter
 * pels as in the compensators: q = lrintf(4 m), clamped to +-2^28, a NaN gives
 * -2^28.
 * Predictor p(by, bx) of F: in the first row (by = 0) p = F[0, bx-1] if
 * bx > 0, else (0, 0).  Below it p is the component-wise median of
 *   A = F[by, bx-1] if bx > 0, else (0, 0);
 *   B = F[by-1, bx];
 *   C = F[by-1, bx+1] if bx + 1 < nbx, else F[by-1, bx-1] if bx > 0, else (0, 0).
 * Bits: for an integer d, k = 2 d - 1 if d > 0, else -2 d, and
 * len(d) = 2 floor(log2(k + 1)) + 1;
 *   R(q, p) = len((qx - px) / step) + len((qy - py) / step),
 * the division C's (truncating toward zero; exact for fields on the step grid).
 * Coder (host code, vcf_mvc.cpp): vcf_mv_encode writes, block by block in
 * raster order, the code of dx = (qx - px) / step, then of dy: signed
 * exp-Golomb of order 0, that is floor(log2(k + 1)) zero bits, then k + 1 in
 * binary.  Bits go MSB first; the last byte is padded with zero bits.  q holds
 * nby * nbx * 2 int32 (x then y).  vcf_mv_decode inverts it block by block, the
 * predictor reading vectors already decoded; the stream must be exactly the
 * encoder's bytes.  vcf_mv_encode_bound gives a capacity that always suffices
 * (70 bits per block).  VCF_ERR_INVALID: a null pointer, negative nby or nbx,
 * step outside {1, 2, 4}, on encode |q| > 2^15 or q % step != 0 or a cap below
 * the stream; on decode a stream that ends early, a prefix of more than 17
 * zeros (|d| <= 2^16 needs no more), a decoded |q| > 2^15, non-zero padding or
 * bytes after the last code.  Nothing is read or written out of bounds on a
 * corrupt stream; on an error the contents of out / q are unspecified.
 * Refinement (vcf_ipp_mv_refine, vcf_ipp_mvrefine.hip): `iterations` passes
 * over the field at mv_dev, in and out.  One pass maps F_in to F_out and every
 * block reads only F_in, so the result does not depend on scheduling.  For
 * block (by, bx), with p its predictor from F_in, the candidates in index
 * order are 0 the block's own vector, 1 p, 2 the left block's vector, 3 the
 * top block's, 4 the right block's (by, bx+1), 5 the bottom block's
 * (by+1, bx), 6 (0, 0).  A candidate whose neighbour lies outside the field is
 * skipped; so is one that is invalid under "Sub-pel motion" (zero is always
 * valid).  J = SAD + lambda R(c, p), with SAD the u8 luma of the reference,
 * interpolated bilinearly at c, against the current luma, as in the sub-pel
 * search; the winner is the argmin of (J, index).  J fits 32 bits:
 * SAD <= 64*64*255, R <= 122, lambda <= 1024.  After the last pass the winners
 * are written as float32 q / 4.
 * Kernel: one launch per pass, one wave per block, the block's luma in LDS; a
 * duplicate of a lower-indexed candidate is not evaluated (it cannot win the
 * tie); where fx = fy = 0 the SAD runs on words (v_alignbyte + v_sad_u8, for
 * bs % 4 == 0 and a 4-byte aligned workspace), else pixel by pixel.  The passes
 * ping-pong between mv_dev and a second field in the workspace so that the
 * last one writes mv_dev (an odd count starts with a copy into the workspace).
 * Workspace (vcf_ipp_mv_refine_workspace_bytes): 2*H*W + 3 + 8 (H/bs)(W/bs)
 * bytes -- the two gray planes as in vcf_ipp_block_match, then the second
 * field at the first 4-byte aligned address at or after workspace_dev + 2*H*W.
 * lambda in 0..1024, iterations in 1..4; limits and alignment as
 * vcf_ipp_block_match_subpel: bs <= 64, mv_dev 4-byte aligned, the frames and
 * the workspace unaligned; at most 65535 block rows.  VCF_ERR_INVALID before
 * any device work for a violation, subpel outside {1, 2, 4}, workspace_bytes
 * below the size function's, or a null pointer.  Written: the (H/bs) * (W/bs)
 * * 2 floats at mv_dev, the 2*H*W gray bytes and the second field's
 * 8 (H/bs)(W/bs) bytes; an empty field (H < bs or W < bs) is legal and writes
 * nothing. */
int vcf_mv_encode_bound(int32_t nby, int32_t nbx, int64_t *bytes);
int vcf_mv_encode(const int32_t *q, int32_t nby, int32_t nbx, int32_t step, uint8_t *out, int64_t cap, int64_t *nbytes);
int vcf_mv_decode(const uint8_t *in, int64_t nbytes, int32_t nby, int32_t nbx, int32_t step, int32_t *q);
int vcf_ipp_mv_refine_workspace_bytes(int32_t H, int32_t W, int32_t bs, int64_t *bytes);
int vcf_ipp_mv_refine(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                      int32_t subpel, int32_t lambda, int32_t iterations, float *mv_dev, uint8_t *workspace_dev,
                      int64_t workspace_bytes, void *stream);

/* residual_shifted = clip(cur - comp + 128, 0, 255) (IPP_DCT.py:547-551).  No
 * pointer needs alignment; writes the n bytes at out_dev. */
int vcf_ipp_residual(const uint8_t *cur_dev, const uint8_t *comp_dev, int64_t n, uint8_t *out_dev, void *stream);

/* recon = clip(comp + rec - 128, 0, 255) (IPP_DCT.py:559-561, 788-790).  No
 * pointer needs alignment; writes the n bytes at out_dev. */
int vcf_ipp_reconstruct(const uint8_t *comp_dev, const uint8_t *rec_dev, int64_t n, uint8_t *out_dev, void *stream);

/* -R block-level RDO of IPP.temporal_filter (IPP_DCT.py:441-536): for every
 * full bs x bs block, IPP.rdo_block_decision (:290-342) on the cv2 RGB2GRAY
 * luma of cur and of its motion compensation comp -- float64 pocketfft DCT,
 * round(x / Q) to int16, float32 dequantization and IDCT, numpy-pairwise
 * mean squared error, get_rate (:265-288) -- and the mode with the smaller
 * D + lambda R (ties to inter).  modes_dev: (H/bs) x (W/bs) u8, 1 = I
 * (intra), 0 = P; costs_dev (NULL or 4 doubles per block): D_inter,
 * R_inter, D_intra, R_intra.  bs in {2, 4, 8, 12, 16, 24, 32}.  The frames and
 * modes_dev need no alignment; costs_dev must be 8-byte aligned
 * (VCF_ERR_INVALID before any device work).  Written: (H/bs) * (W/bs) bytes at
 * modes_dev and, if given, 4 doubles per block at costs_dev. */
int vcf_ipp_rdo_modes(const uint8_t *cur_dev, const uint8_t *comp_dev, int32_t H, int32_t W, int32_t bs, int32_t Q,
                      double lambda, uint8_t *modes_dev, double *costs_dev, void *stream);

/* The frame -R hands to the spatial codec (:489-505): P blocks
 * clip(cur - comp + 128), I blocks cur, pixels outside full blocks 128.  No
 * pointer needs alignment; writes the H * W * 3 bytes at out_dev. */
int vcf_ipp_rdo_residual(const uint8_t *cur_dev, const uint8_t *comp_dev, const uint8_t *modes_dev, int32_t H,
                         int32_t W, int32_t bs, uint8_t *out_dev, void *stream);

/* Mode-aware reconstruction (:512-526, decoder :770-790): P blocks
 * clip(comp + rec - 128), I blocks rec, pixels outside full blocks 0.  No
 * pointer needs alignment; writes the H * W * 3 bytes at out_dev. */
int vcf_ipp_rdo_reconstruct(const uint8_t *comp_dev, const uint8_t *rec_dev, const uint8_t *modes_dev, int32_t H,
                            int32_t W, int32_t bs, uint8_t *out_dev, void *stream);

/* B-frames (--bframes; not in the reference).  Integers throughout.  cur is the
 * frame to code, cf and cb the compensations of the past and of the future
 * anchor's reconstruction (H x W x 3 u8 each, as the compensators write them:
 * 0 outside the full-block area).  Candidates per byte: p0 = cf, p1 = cb,
 * p2 = (cf + cb + 1) >> 1.  For every full bs x bs block SAD_m is the sum of
 * |cur - p_m| over the block's bs * bs * 3 bytes and the block's mode is the
 * argmin of (SAD_m, m): ties go to the lower m.  pred is the winner inside
 * each full block and 0 outside the full-block area.
 * vcf_ipp_bipred_residual writes the (H/bs) x (W/bs) mode bytes at modes_dev
 * and clip(cur - pred + 128, 0, 255) over all H * W * 3 bytes at res_dev, in
 * one launch that reads each source once; pred itself is never written.
 * Limits: 1 <= bs <= 64, H <= 65535, H * W * 3 < 2^31; a violation or a null
 * frame is VCF_ERR_INVALID before any device work.  No pointer needs
 * alignment (4-byte aligned frames with W * 3 a multiple of 4 are read and
 * written in words).  An empty field (H < bs or W < bs) is legal: modes_dev
 * may be NULL, nothing is written there, and the residual follows from
 * pred = 0.  Written: (H/bs) * (W/bs) bytes at modes_dev and H * W * 3 bytes at
 * res_dev. */
int vcf_ipp_bipred_residual(const uint8_t *cur_dev, const uint8_t *cf_dev, const uint8_t *cb_dev, int32_t H, int32_t W,
                            int32_t bs, uint8_t *modes_dev, uint8_t *res_dev, void *stream);

/* The decoder's side of the rule above: pred rebuilt from cf, cb and the mode
 * map, then clip(pred + rec - 128, 0, 255) over all H * W * 3 bytes.  A mode
 * byte above 2 is the caller's error and behaves as mode 0.  Limits, alignment
 * and the empty field as vcf_ipp_bipred_residual (modes_dev is only read).
 * Written: H * W * 3 bytes at out_dev. */
int vcf_ipp_bipred_reconstruct(const uint8_t *cf_dev, const uint8_t *cb_dev, const uint8_t *modes_dev,
                               const uint8_t *rec_dev, int32_t H, int32_t W, int32_t bs, uint8_t *out_dev, void *stream);

/* ---- CBAAC entropy codec (CBAAC.py), host code --------------------------------- */

/* Worst-case code-stream bytes for n symbols. */
int64_t vcf_cbaac_bound(int64_t n_symbols);

/* Context-based adaptive arithmetic coding of n byte symbols with a model of
 * the previous `order` symbols (0..8): CBAAC.CoDec._encode (CBAAC.py:114-131)
 * with AdaptiveModel/ContextManager (:17-69) exactly and the A8 coder.  Host
 * pointers.  Writes the big-endian bit stream (zero padded) the reference
 * appends after its header (:81-95); *out_bytes / *out_bits receive its
 * length. */
int vcf_cbaac_encode(const uint8_t *symbols, int64_t n, int32_t order, uint8_t *out, int64_t out_capacity,
                     int64_t *out_bytes, int64_t *out_bits);

/* Inverse (CBAAC.py:133-150): n symbols from nbytes of code-stream. */
int vcf_cbaac_decode(const uint8_t *bytes, int64_t nbytes, int64_t n, int32_t order, uint8_t *symbols_out);

/* The model alone: the (low, high, total) triple given to the coder for each
 * symbol (3*n int32), for parity checks against the reference's model. */
int vcf_cbaac_model_trace(const uint8_t *symbols, int64_t n, int32_t order, int32_t *triples);

/* ---- tiled CBAAC on the GPU ------------------------------
 * The flattened symbols split into consecutive segments of seg_len symbols
 * (a multiple of 256); each segment is coded exactly as vcf_cbaac_encode
 * codes it alone: CBAAC.CoDec._encode (CBAAC.py:114-131) with a fresh
 * ContextManager (:49-69) and history per segment.
 * Orders 0 and 1 (VCF_ERR_UNSUPPORTED above).  Device pointers; the
 * container (segment sizes + payload) is vcf_amd/tcbaac.py's.
 * Kernels (every vcf_cbaac_tiled_encode* / _decode* below; same bytes): one
 * segment per wave (64 lanes share one model: a shorter time per segment),
 * except that order 0 codes one segment per LANE (64 segments per wave, each
 * with its own model in LDS) once a call has at least 4608 segments to
 * encode / 6144 to decode, over all frames of the call.  The A/B library's
 * *_variant twins (include/vcf_amd_ab.h) take the choice per call. */
int64_t vcf_cbaac_tiled_segments(int64_t n, int64_t seg_len);
/* scratch bytes (ws_dev) for vcf_cbaac_tiled_encode / _trace */
int64_t vcf_cbaac_tiled_workspace(int64_t n, int64_t seg_len);
/* an out_capacity that always suffices */
int64_t vcf_cbaac_tiled_bound(int64_t n, int64_t seg_len);
/* Segments packed back to back into out_dev; seg_bytes_dev (segments + 1
 * int64) receives each segment's byte count and, last, the total (> capacity
 * means the output was cut: retry with vcf_cbaac_tiled_bound bytes). */
int vcf_cbaac_tiled_encode(const uint8_t *sym_dev, int64_t n, int32_t order, int64_t seg_len, uint8_t *out_dev,
                           int64_t out_capacity, int64_t *seg_bytes_dev, void *ws_dev, void *stream);
/* The model alone: the (low, high, total) triple handed to the coder for
 * every symbol (3*n int32), segment by segment (parity checks). */
int vcf_cbaac_tiled_trace(const uint8_t *sym_dev, int64_t n, int32_t order, int64_t seg_len, int32_t *triples_dev,
                          int64_t *seg_bytes_dev, void *ws_dev, void *stream);
/* Inverse: segment s's bytes are in_dev[offs[s] .. offs[s+1]) (segments + 1
 * int64 byte offsets, device); n symbols out. */
int vcf_cbaac_tiled_decode(const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n, int32_t order,
                           int64_t seg_len, uint8_t *sym_dev, void *stream);
/* Prior-seeded segments, orders 0 and 1 (container version 2; not in the
 * reference, which starts every model from 256 ones): the frame's order-0
 * prior f[s] = 1 + floor(hist[s] * 8192 / n) (256 uint16 in prior_dev,
 * 8-byte aligned; hist_dev = 256 uint32 of scratch) seeds every model of
 * every segment (order 1: all 256 contexts), which then adapts by
 * CBAAC.py:32-36.  Each segment's bytes equal vcf_cbaac_encode_prior of that
 * segment alone. */
int vcf_cbaac_tiled_prior(const uint8_t *sym_dev, int64_t n, uint16_t *prior_dev, uint32_t *hist_dev, void *stream);
int vcf_cbaac_tiled_encode_prior(const uint8_t *sym_dev, int64_t n, int32_t order, const uint16_t *prior_dev,
                                 int64_t seg_len, uint8_t *out_dev, int64_t out_capacity, int64_t *seg_bytes_dev,
                                 void *ws_dev, void *stream);
int vcf_cbaac_tiled_decode_prior(const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n, int32_t order,
                                 const uint16_t *prior_dev, int64_t seg_len, uint8_t *sym_dev, void *stream);
/* Batches of frames, each coded exactly as the single-frame calls code it,
 * in one launch per stage (a frame's segments alone fill few waves): n_frames
 * (<= 65535) frames of frame_symbols symbols, frame f's symbols at sym_dev +
 * f * frame_stride (any alignment); priors_dev = n_frames x 256 uint16 (frame
 * f's prior at priors_dev + 256 f; NULL = fresh models, container version 1),
 * hist_dev = n_frames x 256 uint32 of scratch; frame f's packed segments at
 * out_dev + f * out_frame_capacity, its segment byte counts and total at
 * seg_bytes_dev + f * (segments + 1); ws_dev = vcf_cbaac_tiled_frames_workspace
 * bytes.  Decode: frame f's segment offsets at seg_offsets_dev + f * (segments
 * + 1), offsets into in_dev; its symbols to sym_dev + f * out_frame_stride. */
int64_t vcf_cbaac_tiled_frames_workspace(int64_t n_frames, int64_t frame_symbols, int64_t seg_len);
int vcf_cbaac_tiled_prior_frames(const uint8_t *sym_dev, int64_t n_frames, int64_t frame_symbols,
                                 int64_t frame_stride, uint16_t *priors_dev, uint32_t *hist_dev, void *stream);
int vcf_cbaac_tiled_encode_frames(const uint8_t *sym_dev, int64_t n_frames, int64_t frame_symbols,
                                  int64_t frame_stride, int32_t order, const uint16_t *priors_dev, int64_t seg_len,
                                  uint8_t *out_dev, int64_t out_frame_capacity, int64_t *seg_bytes_dev, void *ws_dev,
                                  void *stream);
int vcf_cbaac_tiled_decode_frames(const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n_frames,
                                  int64_t frame_symbols, int32_t order, const uint16_t *priors_dev, int64_t seg_len,
                                  uint8_t *sym_dev, int64_t out_frame_stride, void *stream);
/* Prior classes (container version 3; not in the reference): nclass
 * (1 .. 256) prior rows per frame instead of one.  Segment s of a frame's
 * `segments` takes row floor(s * nclass / segments) -- consecutive runs of
 * segments share a row, so for DCT indices in the subband layout and nclass =
 * 8 a row is (about) one subband row i, whose statistics differ the most --
 * and row c = 1 + floor(hist_c[s] * 8192 / n_c) over the symbols of class c's
 * segments (nclass = 1: the version-2 prior).  priors_dev = n_frames x nclass
 * x 256 uint16 (frame f, class c at + 256 (f nclass + c); 8-byte aligned),
 * hist_dev = as many uint32 of scratch; the rest as the _frames calls.  Each
 * segment's bytes equal vcf_cbaac_encode_prior of that segment alone with
 * its class's row. */
int vcf_cbaac_tiled_prior_classes(const uint8_t *sym_dev, int64_t n_frames, int64_t frame_symbols,
                                  int64_t frame_stride, int64_t seg_len, int32_t nclass, uint16_t *priors_dev,
                                  uint32_t *hist_dev, void *stream);
int vcf_cbaac_tiled_encode_classes(const uint8_t *sym_dev, int64_t n_frames, int64_t frame_symbols,
                                   int64_t frame_stride, int32_t order, const uint16_t *priors_dev, int32_t nclass,
                                   int64_t seg_len, uint8_t *out_dev, int64_t out_frame_capacity,
                                   int64_t *seg_bytes_dev, void *ws_dev, void *stream);
int vcf_cbaac_tiled_decode_classes(const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n_frames,
                                   int64_t frame_symbols, int32_t order, const uint16_t *priors_dev, int32_t nclass,
                                   int64_t seg_len, uint8_t *sym_dev, int64_t out_frame_stride, void *stream);
/* host: version 3's container pieces for a batch of frames -- the segment
 * sizes of each row as unsigned LEB128 varints (row r's bytes end at
 * out[row_end[r]]), and each frame's nclass prior rows stored sparsely
 * (uint32 nclass; per row uint16 m, the m symbols with a frequency != 1, their
 * m uint16 frequencies; frame f's bytes end at out[frame_end[f]]). */
int vcf_leb128_encode_rows(const int64_t *v, int64_t rows, int64_t cols, uint8_t *out, int64_t capacity,
                           int64_t *row_end);
int vcf_prior_rows_sparse(const uint16_t *priors, int64_t frames, int32_t nclass, uint8_t *out, int64_t capacity,
                          int64_t *frame_end);
/* host, orders 0 / 1: vcf_cbaac_encode / _decode with every model seeded by prior (256 uint16, each >= 1) */
int vcf_cbaac_encode_prior(const uint8_t *symbols, int64_t n, int32_t order, const uint16_t *prior, uint8_t *out,
                           int64_t out_capacity, int64_t *out_bytes, int64_t *out_bits);
int vcf_cbaac_decode_prior(const uint8_t *bytes, int64_t nbytes, int64_t n, int32_t order, const uint16_t *prior,
                           uint8_t *symbols_out);

/* ---- tiled CBAAC with a two-dimensional context (container version 4; not in
 * the reference) ----------------------------------------------------------------
 * A (H, W, C) u8 frame is coded plane by plane in th x tw tiles (edge tiles
 * cropped; tile t = (c ty + r) tx + q for tile row r, tile column q of plane
 * c, ty x tx tiles per plane).  A tile's symbols go in raster order through
 * the A8 coder, flushed at the tile's end, each through one of 16
 * AdaptiveModels (CBAAC.py:17-47): ctx = 4 q(|left - 128|) + q(|up - 128|),
 * q(v) = min(v, 3), a neighbour outside the tile counting as 0.  Tile t of a
 * plane's ty tx takes prior class floor(t_in_plane nclass / (ty tx)); the
 * tile's 16 models start from the class's 16 rows, row (class, ctx) = 1 +
 * floor(hist[s] * 8192 / n) over the class's symbols in that context (all
 * ones where there are none).  priors = nclass x 16 x 256 uint16.
 *
 * Host (one frame; the yardstick of the GPU coder and the CPU path): */
int64_t vcf_cbaac2d_tiles(int64_t H, int64_t W, int64_t C, int64_t th, int64_t tw);
int vcf_cbaac2d_prior(const uint8_t *sym, int64_t H, int64_t W, int64_t C, int64_t th, int64_t tw, int32_t nclass,
                      uint16_t *priors);
/* tiles back to back in out; tile_bytes (tiles int64) their sizes */
int vcf_cbaac2d_encode(const uint8_t *sym, int64_t H, int64_t W, int64_t C, int64_t th, int64_t tw, int32_t nclass,
                       const uint16_t *priors, uint8_t *out, int64_t out_capacity, int64_t *tile_bytes,
                       int64_t *out_bytes);
/* tile t's bytes are bytes[tile_offsets[t] .. tile_offsets[t+1]) */
int vcf_cbaac2d_decode(const uint8_t *bytes, const int64_t *tile_offsets, int64_t H, int64_t W, int64_t C, int64_t th,
                       int64_t tw, int32_t nclass, const uint16_t *priors, uint8_t *sym_out);
/* GPU, batches of n_frames (<= 65535) frames, one wave per tile, th * tw <=
 * 65536 and tw <= 256 (VCF_ERR_UNSUPPORTED above); every tile's bytes equal
 * the host coder's.  Device pointers, the caller's stream.  Frame f's symbols
 * at sym_dev + f * frame_stride; priors_dev = n_frames x nclass x 16 x 256
 * uint16 (8-byte aligned), hist_dev = as many uint32 of scratch; frame f's
 * packed tiles at out_dev + f * out_frame_capacity (vcf_cbaac_tiled2d_bound
 * always suffices), its tile byte counts and their total at tile_bytes_dev +
 * f * (tiles + 1); ws_dev = vcf_cbaac_tiled2d_workspace bytes.  Decode: frame
 * f's tile offsets at tile_offsets_dev + f * (tiles + 1), offsets into
 * in_dev; its symbols to sym_dev + f * out_frame_stride. */
int64_t vcf_cbaac_tiled2d_tiles(int64_t H, int64_t W, int64_t C, int64_t th, int64_t tw);
int64_t vcf_cbaac_tiled2d_workspace(int64_t n_frames, int64_t H, int64_t W, int64_t C, int64_t th, int64_t tw);
int64_t vcf_cbaac_tiled2d_bound(int64_t H, int64_t W, int64_t C, int64_t th, int64_t tw);
int vcf_cbaac_tiled2d_prior_frames(const uint8_t *sym_dev, int64_t n_frames, int64_t H, int64_t W, int64_t C,
                                   int64_t frame_stride, int64_t th, int64_t tw, int32_t nclass, uint16_t *priors_dev,
                                   uint32_t *hist_dev, void *stream);
int vcf_cbaac_tiled2d_encode_frames(const uint8_t *sym_dev, int64_t n_frames, int64_t H, int64_t W, int64_t C,
                                    int64_t frame_stride, const uint16_t *priors_dev, int32_t nclass, int64_t th,
                                    int64_t tw, uint8_t *out_dev, int64_t out_frame_capacity, int64_t *tile_bytes_dev,
                                    void *ws_dev, void *stream);
int vcf_cbaac_tiled2d_decode_frames(const uint8_t *in_dev, const int64_t *tile_offsets_dev, int64_t n_frames, int64_t H,
                                    int64_t W, int64_t C, const uint16_t *priors_dev, int32_t nclass, int64_t th,
                                    int64_t tw, uint8_t *sym_dev, int64_t out_frame_stride, void *stream);
/* GPU, plane lists: n_arrays (1 .. 2^20) arrays of different sizes anywhere
 * in one device buffer of buf_bytes bytes (the packed subbands of a batch of
 * 2D-DWT frames), every 64 x 64 tile of every array in one launch per stage.
 * Array a is H x W x C symbols (H, W, C >= 1, channels interleaved) from byte
 * `base`; tile0 = the tiles of the arrays before it, so the launch's n_tiles
 * tiles are numbered array by array, each array's as the frame entry points
 * number a frame's.  Array a's code-stream is, byte for byte, what the frame
 * entry points (and the host coder) give for that array alone: its prior rows
 * are rows a * nclass * 16 .. of priors_dev (n_arrays x nclass x 16 x 256
 * uint16, 8-byte aligned; hist_dev as many uint32), its tiles' bytes
 * out_dev[offset(tile0) .. offset(tile0 + tiles)), the packed tiles of all
 * arrays back to back; tile_bytes_dev takes the n_tiles byte counts and their
 * total.  desc_host and desc_dev hold the same n_arrays descriptors: the host
 * copy is checked (sizes, tile0, every array inside buf_bytes) before
 * anything is launched, the kernels read the device copy.  Decode:
 * tile_offsets_dev = n_tiles + 1 offsets into in_dev; array a's symbols are
 * written at its base. */
typedef struct vcf_plane_desc {
    int64_t base;
    int32_t H, W, C;
    int32_t tile0;
} vcf_plane_desc;
int64_t vcf_cbaac_tiled2d_planes_workspace(int64_t n_tiles, int64_t th, int64_t tw);
int64_t vcf_cbaac_tiled2d_planes_bound(int64_t n_tiles, int64_t th, int64_t tw);
int vcf_cbaac_tiled2d_prior_planes(const uint8_t *buf_dev, int64_t buf_bytes, const vcf_plane_desc *desc_host,
                                   const vcf_plane_desc *desc_dev, int64_t n_arrays, int64_t n_tiles, int64_t th,
                                   int64_t tw, int32_t nclass, uint16_t *priors_dev, uint32_t *hist_dev, void *stream);
int vcf_cbaac_tiled2d_encode_planes(const uint8_t *buf_dev, int64_t buf_bytes, const vcf_plane_desc *desc_host,
                                    const vcf_plane_desc *desc_dev, int64_t n_arrays, int64_t n_tiles,
                                    const uint16_t *priors_dev, int32_t nclass, int64_t th, int64_t tw,
                                    uint8_t *out_dev, int64_t out_capacity, int64_t *tile_bytes_dev, void *ws_dev,
                                    void *stream);
int vcf_cbaac_tiled2d_decode_planes(const uint8_t *in_dev, const int64_t *tile_offsets_dev,
                                    const vcf_plane_desc *desc_host, const vcf_plane_desc *desc_dev, int64_t n_arrays,
                                    int64_t n_tiles, const uint16_t *priors_dev, int32_t nclass, int64_t th, int64_t tw,
                                    uint8_t *buf_dev, int64_t buf_bytes, void *stream);

/* ---- CBAHC entropy codec (CBAHC.py), host code --------------------------------- */

/* Worst-case code-stream bytes for n symbols. */
int64_t vcf_cbahc_bound(int64_t n_symbols);

/* Context-based adaptive Huffman coding of n byte symbols (order 0..7):
 * CBAHC.CoDec.compress_fn (CBAHC.py:169-221) bit for bit -- per symbol a
 * Huffman tree from the context's counts (:38-78), its code (:81-106), then
 * the count update.  Big-endian bits, zero padded; *out_bits = exact count
 * (the reference keeps it in its side file). */
int vcf_cbahc_encode(const uint8_t *symbols, int64_t n, int32_t order, uint8_t *out, int64_t out_capacity,
                     int64_t *out_bytes, int64_t *out_bits);

/* Inverse (CBAHC.py:226-276): n symbols from the first nbits bits. */
int vcf_cbahc_decode(const uint8_t *bytes, int64_t nbits, int64_t n, int32_t order, uint8_t *symbols_out);

/* ---- frame ingest: PNG reader (host code) ------------------------------------ */

/* Size of a PNG in memory and whether vcf_png_decode_rgb covers it (bit
 * depth 8, colour type 0/2/3/4/6, not interlaced). */
int vcf_png_info(const uint8_t *data, int64_t nbytes, int32_t *H, int32_t *W, int32_t *supported);

/* PNG bytes -> H x W x 3 RGB u8 (host buffer of out_capacity bytes): what
 * EIC.encode_read_fn reads (entropy_image_coding.py:51-65; A9: PIL's
 * convert("RGB") -- gray replicated, alpha dropped, palette looked up).
 * VCF_ERR_UNSUPPORTED for PNGs outside vcf_png_info's set (the caller falls
 * back to another reader), VCF_ERR_INVALID for corrupt files. */
int vcf_png_decode_rgb(const uint8_t *data, int64_t nbytes, uint8_t *rgb_out, int64_t out_capacity);

/* RGB u8 (H x W x 3, host) -> PNG file bytes: 8-bit truecolour, Up-filtered
 * scanlines, one zlib stream at `level` deflated in 1 MiB pieces on up to
 * `threads` threads (pigz's construction: each piece primed with the previous
 * 32 KiB, sync-flushed, adler32 combined).  The writer of the decode side's
 * PNGs (EIC.decode_write_fn, entropy_image_coding.py:101-112) and of IPP's
 * frame dumps: pixel-exact, not byte-identical to other PNG writers.
 * out_capacity >= vcf_png_encode_bound(H, W) always suffices; *out_bytes
 * receives the file size. */
int vcf_png_encode_rgb(const uint8_t *rgb, int32_t H, int32_t W, int32_t level, int32_t threads, uint8_t *out,
                       int64_t out_capacity, int64_t *out_bytes);
int64_t vcf_png_encode_bound(int32_t H, int32_t W);

/* ---- TIFF strip deflate on the GPU (TIFF.py:23-31, the default -c) ----------
 * zlib.compress(strip, level) for every strip of a batch of frames, byte for
 * byte (zlib 1.2.11 deflate_slow, windowBits 15, memLevel 8): what
 * tifffile.imwrite(..., compression='zlib') stores per RowsPerStrip strip
 * (TIFF.py:29; host path vcf_amd/codec/tiff.py _deflate_strips).  Frame f is
 * in_dev[f*frame_bytes, (f+1)*frame_bytes), cut into strips of strip_bytes
 * (the last one shorter; in_dev, frame_bytes and strip_bytes need no
 * alignment); strip s = f*spf + k, spf = vcf_zlib_strip_count,
 * is written to out_dev + s*slot_bytes and its length to sizes_dev[s]
 * (-1: slot too small).  level 4..9 (VCF_ERR_UNSUPPORTED otherwise);
 * strip_bytes <= 65536 (tifffile's strips for rows up to 64 KB);
 * slot_bytes a multiple of 4 >= vcf_zlib_bound(strip_bytes); ws_dev holds
 * vcf_zlib_workspace(total strips) bytes (16-byte aligned; out_dev and
 * sizes_dev 4-byte aligned) -- ~1.15 MB per strip, at most the workspace
 * budget whatever the batch: past that the strips are coded in rounds that
 * reuse it.  The budget is fixed per device on first use: a quarter of the
 * memory free then, clamped to 3.9..40 GB; vcf_zlib_set_workspace_budget(b)
 * sets it for the current device (0 restores the default; b at least one
 * strip's workspace), after which vcf_zlib_workspace must be asked again.  The call is asynchronous on `stream`;
 * internally part of each round runs on library streams forked from and
 * joined back to it, so the caller sees ordinary stream semantics. */
int64_t vcf_zlib_bound(int64_t strip_bytes);
int64_t vcf_zlib_workspace(int64_t n_strips);
int vcf_zlib_set_workspace_budget(int64_t bytes);
/* the largest strip_bytes vcf_zlib_strips takes (65536: frames with rows of
 * more than 64 KB -- 1-row strips past 21845 RGB pixels -- stay on the host writer) */
int32_t vcf_zlib_max_strip(void);
int64_t vcf_zlib_strip_count(int64_t frame_bytes, int32_t strip_bytes);
int vcf_zlib_strips(const uint8_t *in_dev, int64_t n_frames, int64_t frame_bytes, int32_t strip_bytes, int32_t level,
                    uint8_t *out_dev, int64_t slot_bytes, int32_t *sizes_dev, void *ws_dev, void *stream);

/* ---- TIFF strip inflate on the GPU (TIFF.py:33-39, the decode side of -c TIFF)
 * zlib.decompress for every strip of a batch: strip s is comp_len_dev[s] bytes
 * of a zlib stream at comp_dev + comp_off_dev[s], inflated to
 * out_dev + out_off_dev[s], which must come to exactly out_len_dev[s] bytes
 * (the TIFF's rows per strip x row bytes).  status_dev[s] = 0, or < 0 when the
 * stream is not one zlib accepts with that length (-1 header, -2 block, -3
 * code, -4 distance, -5 length, -6 adler32, -7 input overrun, -8 an
 * over-subscribed or incomplete code-length set, -9 no end-of-block code,
 * -10 a negative length: nothing read or written).  Device arrays, which the
 * kernel trusts: offsets and lengths must lie inside comp_dev and out_dev
 * (vcf_amd/zlib_gpu.py checks them on the host first); RFC 1950/1951,
 * stored, fixed and dynamic blocks. */
int vcf_inflate_strips(const uint8_t *comp_dev, const int64_t *comp_off_dev, const int32_t *comp_len_dev,
                       int64_t n_strips, uint8_t *out_dev, const int64_t *out_off_dev, const int32_t *out_len_dev,
                       int32_t *status_dev, void *stream);

/* ---- deadzone quantizer plug-in (deadzone.py:95-117, assumption A5) ---------- */

/* k[i] = (int32)(x[i] / Q), truncation toward zero; the division is float32
 * for VCF_DTYPE_F32 input and float64 for every other input type (numpy true
 * division).  Replaces deadzone.CoDec.quantize_fn (deadzone.py:95-102).  x_dev
 * must be aligned to its element and k_dev to 4 bytes (VCF_ERR_INVALID before
 * any device work); writes the n int32 at k_dev. */
int vcf_deadzone_quantize(const void *x_dev, int32_t x_dtype, int64_t n, int32_t Q, int32_t *k_dev,
                          void *stream);

/* y[i] = Q * k[i] in k's type (VCF_DTYPE_I16 or VCF_DTYPE_I32), wrapping.
 * Replaces deadzone.CoDec.dequantize_fn (deadzone.py:107-117).  k_dev and y_dev
 * must be aligned to the element (VCF_ERR_INVALID before any device work);
 * writes the n elements at y_dev. */
int vcf_deadzone_dequantize(const void *k_dev, int32_t k_dtype, int64_t n, int32_t Q, void *y_dev,
                            void *stream);

/* ---- §8(f) row 4: the YCrCb and LloydMax plug-ins ------------------------------
 * YCrCb (src/YCrCb.py:25-72): the stand-alone pixel codec.  Its transform,
 * color_transforms.YCrCb, is not vendored: OpenCV's integer RGB<->YCrCb on
 * uint8 is assumed (A12; parity unpinned).  n_px pixels of 3 interleaved
 * channels.  Note: 2D-DCT.py / 2D-DWT.py with -t YCrCb still convert with
 * YCoCg (they bind from_RGB/to_RGB from color_transforms.YCoCg, 2D-DCT.py:22-23,
 * 2D-DWT.py:19-20), so they use the YCoCg entry points above.  For these and
 * the pixel codecs below: u8 pointers need no alignment (words where the
 * address allows, bytes elsewhere); uint16 and int16 arrays must be 2-byte
 * aligned (VCF_ERR_INVALID before any device work); the output written is the
 * n_px * 3 (or n) elements at the output pointer. */
int vcf_ycrcb_from_rgb(const uint8_t *rgb_dev, int64_t n_px, uint8_t *ycrcb_dev, void *stream);
int vcf_ycrcb_to_rgb(const uint8_t *ycrcb_dev, int64_t n_px, uint8_t *rgb_dev, void *stream);
/* YCrCb.encode (:33-51) with -a deadzone: from_RGB, int16, (x / Q) truncated, uint16. */
int vcf_ycrcb_dz_encode(const uint8_t *rgb_dev, int64_t n_px, int32_t Q, uint16_t *k_dev, void *stream);
/* YCrCb.decode (:53-72): Q * k in uint16, int16, uint8, to_RGB, clip. */
int vcf_ycrcb_dz_decode(const uint16_t *k_dev, int64_t n_px, int32_t Q, uint8_t *rgb_dev, void *stream);

/* ---- the stand-alone pixel codecs YCoCg.py and deadzone.py -------------------
 * YCoCg.encode (src/YCoCg.py:33-56) with -a deadzone: img.astype(int16),
 * from_RGB into int16 (A4, truncated toward zero), += offset 0 (:27-28),
 * deadzone (x / Q) truncated (A5), astype(uint16).  n_px pixels of 3
 * interleaved channels; k_dev n_px * 3 uint16. */
int vcf_ycocg_dz_encode(const uint8_t *rgb_dev, int64_t n_px, int32_t Q, uint16_t *k_dev, void *stream);
/* YCoCg.decode (:58-85): astype(int16), Q * k in int16 (1 <= Q <= 32767, else
 * VCF_ERR_UNSUPPORTED), to_RGB in int16 (A4, wrapping), clip(0, 255), uint8. */
int vcf_ycocg_dz_decode(const uint16_t *k_dev, int64_t n_px, int32_t Q, uint8_t *rgb_dev, void *stream);
/* YCoCg.py with -a LloydMax (:29-30, offset [-128, 0, 0]): the int16 YCoCg
 * image (A4) with offset0 added to Y, for the LloydMax entry points below; and
 * back: Y - offset0, to_RGB in int16, clip(0, 255), uint8. */
int vcf_ycocg_i16_from_rgb(const uint8_t *rgb_dev, int64_t n_px, int32_t offset0, int16_t *out_dev, void *stream);
int vcf_ycocg_i16_to_rgb(const int16_t *in_dev, int64_t n_px, int32_t offset0, uint8_t *rgb_dev, void *stream);
/* deadzone.encode (src/deadzone.py:67-79): astype(int16), (x / Q) truncated,
 * astype(uint8), elementwise over n bytes. */
int vcf_dz_u8_encode(const uint8_t *x_dev, int64_t n, int32_t Q, uint8_t *k_dev, void *stream);
/* deadzone.decode (:81-93): Q * k in uint8 (wrapping; 1 <= Q <= 255, the
 * Python-int-times-uint8 result type, else VCF_ERR_UNSUPPORTED). */
int vcf_dz_u8_decode(const uint8_t *k_dev, int64_t n, int32_t Q, uint8_t *y_dev, void *stream);

/* LloydMax (src/LloydMax.py:75-143).  Per channel c of an n_px x channels
 * array: counts = numpy.histogram(x[..., c], bins=max-min+1, range=(min, max))
 * (numpy 1.26's arithmetic; int64 counts, channel-major, zeroed here), the
 * glue's +1, the Lloyd-Max design of scalar_quantization's LloydMax_Quantizer
 * (un-vendored; A13, unpinned: the textbook design, oracle/plugins.py),
 * k = searchsorted(thresholds, x, 'right') stored with a C cast into k's type,
 * y = centroids[k] truncated into y's integer type.  dtypes: VCF_DTYPE_U8,
 * I16, U16, F32 (histogram/encode input, encode output).  vcf_lm_levels returns
 * the number of levels N = ceil((max - min + 1) / Q) or an error (< 0). */
int vcf_lm_levels(int32_t Q_step, int32_t min_val, int32_t max_val);
int vcf_lm_histogram(const void *x_dev, int32_t x_dtype, int64_t n_px, int32_t channels, int32_t min_val,
                     int32_t max_val, int64_t *counts_dev, void *stream);
/* (vcf_lm_histogram, _encode, _decode: x, k and y arrays must be aligned to their
 * element, counts_dev and centroids_dev to 8 bytes, bad_dev to 4, else
 * VCF_ERR_INVALID before any device work; written: channels * (max - min + 1)
 * int64 at counts_dev, n_px * channels elements at k_dev / y_dev.)
 * Host memory: counts (n_bins, already +1) -> centroids (N doubles); returns N or an error. */
int vcf_lm_design(const int64_t *counts, int32_t n_bins, int32_t Q_step, int32_t min_val, double *centroids);
/* centroids_dev: channels x n_levels doubles (channel-major). */
int vcf_lm_encode(const void *x_dev, int32_t x_dtype, int64_t n_px, int32_t channels, const double *centroids_dev,
                  int32_t n_levels, void *k_dev, int32_t k_dtype, void *stream);
/* *bad_dev is set to 1 when an index is outside [-N, N) (numpy's IndexError); the caller zeroes it. */
int vcf_lm_decode(const void *k_dev, int32_t k_dtype, int64_t n_px, int32_t channels, const double *centroids_dev,
                  int32_t n_levels, void *y_dev, int32_t y_dtype, int32_t *bad_dev, void *stream);

/* ---- vector quantization (src/VQ.py, src/color-VQ.py) ---------------------------
 * k-means as sklearn.cluster.KMeans(algorithm="lloyd", n_init=1) runs it, on the
 * blocks of one u8 frame of H x W x C samples, 1 <= C <= 4.  The block size BS
 * is 1..16 and divides H and W (else VCF_ERR_INVALID: the reference's reshape
 * raises there).  Vector n is block (n / (W/BS), n % (W/BS)) in raster order,
 * img[y:y+BS, x:x+BS, :] flattened row-major (channel fastest): D = BS*BS*C
 * values, N = (H/BS)*(W/BS) vectors.  1 <= K <= min(N, 4096); labels are
 * uint16, centroids K x D float64 (row-major).  Every argument is checked
 * before any device work; the work is enqueued on `stream`.  vcf_vq_init_pp and
 * vcf_vq_fit run host-driven loops: they synchronise `stream` and have finished
 * when they return; the other three only enqueue.  For vcf_vq_assign,
 * _accumulate and _decode: img_dev needs no alignment; labels must be 2-byte,
 * centroids, distances, sums and counts 8-byte and bad_dev 4-byte aligned
 * (VCF_ERR_INVALID before any device work); written: N labels (and N
 * distances), K * D sums and K counts, or the Hl*BS x Wl*BS x C image bytes.
 *
 * vcf_vq_assign: labels[n] = argmin_j dist(n, j), the lowest j on a tie (strict
 * `<` while j ascends), and, when dist_dev is not NULL, that least distance.
 * The arithmetic is the direct difference form in float64,
 *     dist = 0;  for d = 0 .. D-1:  t = x_d - c_jd;  dist = dist + t * t;
 * with x_d converted exactly and three separate roundings per term (subtract,
 * multiply, add: no FMA, the library is built with -ffp-contract=off), on the
 * vector ALU.  numpy restates it bit for bit, ties included.  The centroids
 * pass through LDS in tiles of KT centroids (KT * D * 8 bytes <= 32 KiB, at
 * least 8 centroids, so at most 64 KiB when D = 1024); tiling changes no
 * result, each distance is one chain over d. */
int vcf_vq_assign(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size,
                  const double *centroids_dev, int32_t K, uint16_t *labels_dev, double *dist_dev, void *stream);
/* sums[j][d] = sum of x_d over the vectors labelled j, counts[j] = their number:
 * int64, zeroed here, integer arithmetic throughout (the result depends on no
 * order, tiling or atomic).  A vector whose label is >= K is left out. */
int vcf_vq_accumulate(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size,
                      const uint16_t *labels_dev, int32_t K, int64_t *sums_dev, int64_t *counts_dev, void *stream);
/* Greedy k-means++ (sklearn's _kmeans_plusplus) in exact integers.  Candidates
 * are data vectors, so every squared distance and potential is an int64.
 *     u(step, trial) = mix(seed + 0x9E3779B97F4A7C15 * (16 * step + trial + 1))   (mod 2^64)
 *     mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *             return z ^ (z >> 31)                       (splitmix64's output function)
 *     mulhi64(a, b) = (a * b) >> 64
 *   step 0: id_0 = mulhi64(u(0, 0), N);  closest[n] = |x_n - x_id0|^2
 *   step c = 1 .. K-1, with T = 2 + floor(ln K) trials:
 *     pot = sum(closest);  r_t = mulhi64(u(c, t), pot);
 *     candidate_t = the first index whose running sum closest[0] + ... + closest[i]
 *                   exceeds r_t  (vector 0 when pot = 0);
 *     pot_t = sum_n min(closest[n], |x_n - x_candidate_t|^2);
 *     id_c = the candidate of least pot_t (the lowest t on a tie);
 *     closest[n] = min(closest[n], |x_n - x_id_c|^2)
 * centroids[c] = x_id_c.  ids_host (host memory, K int64, may be NULL) receives
 * the chosen indices.  Per step only T candidate indices and the partial sums of
 * 256-vector chunks cross to the host; being integers, no launch geometry
 * changes a result. */
int vcf_vq_init_pp(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size, int32_t K,
                   uint64_t seed, double *centroids_dev, int64_t *ids_host, void *stream);
/* The host-side report of vcf_vq_fit. */
#define VCF_VQ_STOP_STRICT 0   /* the labels did not change */
#define VCF_VQ_STOP_TOL 1      /* the summed squared centre shift fell to tol_abs or under */
#define VCF_VQ_STOP_MAX_ITER 2
typedef struct vcf_vq_report {
    int32_t n_iter;
    int32_t stop_reason;
    int64_t relocations;   /* vectors handed to empty clusters, over all iterations */
    double inertia;        /* sum over n, in index order, of dist(n, labels[n]) to the returned centroids */
    double tol_abs;        /* tol * mean_d((N * S2_d - S1_d^2) / N^2), exact integer moments, one division per d */
} vcf_vq_report;
/* Lloyd's iteration with sklearn's semantics (_kmeans_single_lloyd), started
 * from init_centroids_dev (K x D float64; it may be centroids_dev itself) or,
 * when that is NULL, from vcf_vq_init_pp(seed).  Per iteration: assign,
 * accumulate, centroid = (double)sum / (double)count (one division).  An empty
 * cluster takes the vector farthest from its own centroid (largest distance,
 * the lowest index on a tie, successive empty clusters in ascending order the
 * next farthest); the vector leaves its old cluster's sum and count; the labels
 * of that iteration stay.  When the farthest distance left is 0 the cluster
 * stays empty, and a cluster without members keeps its centroid.  The loop ends
 * when the labels equal the previous iteration's (strict), else when the sum
 * over all j, d of (new - old)^2 is <= tol_abs, else after max_iter (>= 1)
 * iterations; unless strict, one more assign makes the labels match the
 * returned centroids.  *report is host memory. */
int vcf_vq_fit(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size, int32_t K, uint64_t seed,
               int32_t max_iter, double tol, const double *init_centroids_dev, double *centroids_dev,
               uint16_t *labels_dev, vcf_vq_report *report, void *stream);
/* labels (Hl x Wl) and centroids -> the u8 image (Hl*BS x Wl*BS x C): each
 * sample is the centroid value truncated into int16 and then its low byte
 * (VQ.py:125-137 and .astype(np.uint8); values outside int32 saturate first).
 * A label >= K sets *bad_dev to 1 (the caller zeroes it; numpy's IndexError)
 * and writes 0; nothing is read out of bounds. */
int vcf_vq_decode(const uint16_t *labels_dev, int32_t Hl, int32_t Wl, int32_t C, int32_t block_size,
                  const double *centroids_dev, int32_t K, uint8_t *img_dev, int32_t *bad_dev, void *stream);

/* ---- distortion between two sets of u8 frames (src/RDE.py) -----------------------
 *
 * What RDE.py's calculate_rmse needs, as exact integers.  a_dev and b_dev hold
 * n_frames contiguous frames of H x W x C uint8 samples each (channel fastest),
 * 1 <= C <= 4; out_dev receives n_frames x C records, record f * C + c for
 * frame f and channel c, with d = |a - b| over the H * W samples of that
 * channel:
 *     sse = sum d * d,   sad = sum d,   max_abs = max d,   pad = 0.
 * Integer arithmetic throughout: 32-bit partial sums are widened to 64 bits long
 * before they could overflow, and the 64-bit sums and the maximum depend on no
 * launch geometry and on no order.  The call zeroes the records itself (on
 * `stream`, before the kernel), so a repeated call into the same out_dev gives
 * the same records.  out_dev is 8-byte aligned; the frames need no alignment
 * (frames whose addresses differ by a multiple of 16 bytes, as two hipMalloc'd
 * sets always do, run at full speed; others are read bytewise).  C outside
 * 1..4, a negative size, a null or misaligned pointer: VCF_ERR_INVALID before
 * any device work.  n_frames = 0 or H * W = 0: VCF_OK, nothing is enqueued and
 * out_dev is left untouched.  Otherwise the work is enqueued on `stream`.
 * RMSE = sqrt((double)(sum of sse over c) / (H * W * C)) (vcf_amd/distortion.py). */
typedef struct vcf_distortion_record {
    uint64_t sse;
    uint64_t sad;
    uint32_t max_abs;
    uint32_t pad;
} vcf_distortion_record;
int vcf_distortion_u8(const uint8_t *a_dev, const uint8_t *b_dev, int64_t n_frames, int32_t H, int32_t W, int32_t C,
                      vcf_distortion_record *out_dev, void *stream);

/* ---- SSIM between two sets of u8 frames, exact by construction ---
 *
 * a_dev and b_dev hold n_frames contiguous frames of H x W x C uint8 samples each
 * (channel fastest), C = 1 or 3, H and W at least 11; out_dev receives n_frames x C
 * records, record f * C + c for frame f and channel c.  The window is Wang et
 * al.'s 11 x 11 Gaussian (sigma 1.5), separable, each axis scaled to sum 256 and
 * rounded: w = {0, 2, 9, 28, 55, 68, 55, 28, 9, 2, 0} (the outer taps round to 0:
 * the support is 9 x 9 inside the 11 x 11 footprint), 2-D weight sum S = 2^16.
 * Only the (H - 10) * (W - 10) windows that lie wholly inside the frame count.
 * Per window, with x from a and y from b, as exact integers:
 *     A = sum w_i w_j x,  B = sum w_i w_j y,
 *     XX = sum w_i w_j x^2,  YY = sum w_i w_j y^2,  XY = sum w_i w_j x y,
 *     f1 = 2 A B + C1,            f2 = 2 (S XY - A B) + C2,
 *     f3 = A^2 + B^2 + C1,        f4 = S XX - A^2 + S YY - B^2 + C2,
 * C1 = 27928024842 = round(6.5025 * 2^32), C2 = 251352223580 = round(58.5225 * 2^32).
 * Every factor is below 2^50 in magnitude, so its conversion to double is exact;
 *     q = ((double)f1 * (double)f2) / ((double)f3 * (double)f4)
 * is two IEEE multiplications and one IEEE division (round to nearest), and
 *     k = (int64) rint(q * 2^30)          (ties to even; k can be negative).
 * sum_k and min_k are the sum and the minimum of k over the windows; windows is
 * their number.  SSIM = sum_k / (windows * 2^30), divided on the host.  Integer
 * sums and minima depend on no launch geometry and on no order.  The call sets
 * the records itself (on `stream`, before the kernel).  out_dev is 8-byte
 * aligned; the frames need no alignment.  A null pointer, n_frames < 1, C other
 * than 1 or 3, H < 11 or W < 11, a misaligned out_dev: VCF_ERR_INVALID before any
 * device work, and nothing is written.  Otherwise the work is enqueued on
 * `stream`. */
#define VCF_SSIM_WINDOW 11
#define VCF_SSIM_ONE (1 << 30)
typedef struct vcf_ssim_record {
    int64_t sum_k;
    uint64_t windows;
    int64_t min_k;
} vcf_ssim_record;
int vcf_ssim_u8(const uint8_t *a_dev, const uint8_t *b_dev, int64_t n_frames, int32_t H, int32_t W, int32_t C,
                vcf_ssim_record *out_dev, void *stream);
/* The edge, in windows, of the square tile one workgroup of vcf_ssim_u8 takes (for tests and benchmarks). */
int vcf_ssim_tile(void);

/* ---- deblocking post-filter of the block-transform decoders ------
 *
 * Not in the reference.  in_dev holds n_frames decoded frames of H x W x 3 uint8
 * (channel fastest), frame f at in_dev + f * frame_stride_bytes; out_dev receives
 * the filtered frames at the same stride.  Every channel is filtered on its own.
 * All arithmetic is int32, >> is an arithmetic shift, clip255 saturates to 0..255.
 * The block grid has period B and starts `left` columns and `top` rows outside
 * the frame (what the decoder cropped): a vertical edge lies between columns
 * x - 1 and x iff 0 < x < W and (x + left) % B == 0, a horizontal one between
 * rows y - 1 and y iff 0 < y < H and (y + top) % B == 0.
 *   Pass V, vertical edges, along rows, every read from the input: per edge x, row
 *     and channel, p2 p1 p0 = in[x-3] in[x-2] in[x-1], q0 q1 q2 = in[x] in[x+1]
 *     in[x+2]; a line with x - 3 < 0 or x + 2 > W - 1 is left as it is.
 *   Pass H, horizontal edges, the same rule down columns, reading pass V's result.
 *   Per line:  dp = |p2 - 2 p1 + p0|, dq = |q2 - 2 q1 + q0|; unchanged if
 *     dp + dq >= beta.  delta = (9 (q0 - p0) - 3 (q1 - p1) + 8) >> 4; unchanged if
 *     |delta| >= 10 tc.  delta = clip(-tc, tc, delta); p0' = clip255(p0 + delta),
 *     q0' = clip255(q0 - delta).  side = (beta + (beta >> 1)) >> 3, h = tc >> 1;
 *     if dp < side: p1' = clip255(p1 + clip(-h, h, (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1));
 *     if dq < side: q1' = clip255(q1 + clip(-h, h, (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1)).
 *     p2 and q2 are never written.  (HEVC's normal filter, decided per line.)
 * With B >= 4 no two lines of a pass write the same sample.  A frame without an
 * interior edge is copied.  Only the H * W * 3 bytes of each frame are written;
 * the bytes between frames that frame_stride_bytes leaves are not touched.  The
 * frames need no alignment (where out_dev - in_dev is a multiple of 16 the stores
 * are 16 bytes wide, otherwise bytes).  Out of place: in_dev == out_dev or
 * overlapping extents, B < 4, top or left outside [0, B), negative beta, tc or
 * size, frame_stride_bytes < H * W * 3, a null pointer: VCF_ERR_INVALID before
 * any device work.  n_frames = 0 or H * W = 0: VCF_OK and nothing is enqueued.
 * Otherwise one kernel per 65535 frames is enqueued on `stream`; no workspace. */
int vcf_deblock_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int32_t H, int32_t W,
                   int64_t frame_stride_bytes, int32_t B, int32_t top, int32_t left, int32_t beta, int32_t tc,
                   void *stream);

/* ---- histograms of index planes (the rate estimate of vcf_amd/rate.py) -----------
 *
 * idx_dev holds n_frames contiguous index frames of H x W x 3 uint8 (channel
 * fastest), as vcf_dct_dz_encode writes them with H = Hp, W = Wp.  The rows x
 * cols grid cuts every frame into regions of (H / rows) x (W / cols) pixels,
 * region r = i * cols + j at pixel (i * H / rows, j * W / cols): 1 x 1 is the
 * whole plane, B x B the subbands of the DCT's subband layout.  counts_dev
 * receives n_frames x rows * cols x 3 x 256 uint32 counters,
 *     counts[((f * rows * cols + r) * 3 + c) * 256 + v]
 *         = the samples of channel c in region r of frame f that equal v.
 * Integer adds: the counts depend on no launch geometry and on no order.  The
 * call zeroes the counters it writes itself (on `stream`, before the kernel).
 * idx_dev needs no alignment (16-byte loads from the first 16-byte boundary of
 * every row segment, bytes around them); counts_dev is 4-byte aligned.
 * counts_capacity is the number of uint32 counters at counts_dev: only the
 * first n_frames * rows * cols * 768 are written, and a smaller capacity is
 * VCF_ERR_INVALID.  So are a null or misaligned pointer, a negative size, rows
 * or cols < 1 and a grid that does not divide the frame (H % rows, W % cols);
 * rows or cols > 16 and frames of more than 2^31 - 1 bytes are
 * VCF_ERR_UNSUPPORTED; all before any device work, nothing written.
 * n_frames = 0: VCF_OK, nothing enqueued.  H * W = 0: the counters are zeroed.
 * Batches of more than 65535 frames run in launches of 65535. */
int vcf_index_hist_u8(const uint8_t *idx_dev, int64_t n_frames, int32_t H, int32_t W, int32_t rows, int32_t cols,
                      uint32_t *counts_dev, int64_t counts_capacity, void *stream);

/* ---- rate-distortion optimised quantization of the 8x8 DCT encode (vcf_amd/rdoq.py) ----
 *
 * vcf_dct_dz_encode with one more step per coefficient: where the bits saved are
 * worth more than the distortion added, an index is lowered towards zero.  Input,
 * output, padding and layouts (VCF_DCT_NO_SUBBANDS) are vcf_dct_dz_encode's, and
 * the output is an ordinary index frame: every decoder reads it.  Encoder side
 * only, and not in the reference.
 *
 * cost_dev: float64 [cost_frames][64][3][256], cost_frames = 1 (one table for
 * every frame) or n_frames; entry [f][8 i + j][ch][(k + 128) & 255] is the cost
 * in bits of index k at row i, column j of a block in channel ch of frame f (the
 * position in the block, in both layouts).  For a coefficient c (the float32
 * value vcf_dct_dz_encode divides by Q) with deadzone index k0 = trunc(c / Q),
 * s = sign(k0), and
 *     J(k) = d * d + lambda * cost[..][(k + 128) & 255],  d = (double)c - (double)(Q * k),
 * in float64, every operation rounded on its own:
 *   1. k0 == 0, k0 < -128 or k0 > 127: the index is k0 (and wraps modulo 256 as in
 *      vcf_dct_dz_encode);
 *   2. otherwise best = k0; k0 - s replaces it if J(k0 - s) <= J(best); then, if
 *      k0 - s != 0, 0 replaces it if J(0) <= J(best);
 *   3. the byte is (best + 128) & 255.
 * So no magnitude grows, lambda = 0 gives vcf_dct_dz_encode's bytes, and the sum of
 * J under a given table is never above the plain encode's.
 *
 * block_size != 8 and VCF_DCT_PERCEPTUAL: VCF_ERR_UNSUPPORTED.  A null pointer,
 * n_frames < 1, cost_frames other than 1 or n_frames, cost_capacity (doubles at
 * cost_dev) below cost_frames * 64 * 3 * 256, a cost_dev off 8 bytes, a lambda that
 * is negative or not finite, Q < 1: VCF_ERR_INVALID; all before any device work,
 * nothing written.  rgb_dev and k_dev need no alignment, as for vcf_dct_dz_encode;
 * writes the n_frames * Hp * Wp * 3 bytes at k_dev and reads the table in place.
 * The work is enqueued on `stream`; the call keeps no state.  Batches of more than
 * 65535 frames run in launches of 65535. */
int vcf_dct_dz_encode_rdoq(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                           int32_t Q, uint32_t flags, const double *cost_dev, int64_t cost_frames,
                           int64_t cost_capacity, double lambda, uint8_t *k_dev, void *stream);
/* The blocks one workgroup of vcf_dct_dz_encode_rdoq takes (for tests and benchmarks). */
int vcf_dct_rdoq_tile(void);

/* ---- cross-rank exchange on RCCL over xGMI -------------------
 * Frames shard across one process per GPU with no collective on the data
 * path; the one exchange step of the III / IPP drivers is after coding: an
 * all-gather of the per-frame code-stream sizes and a gather of the
 * variable-length payloads to rank 0.  It replaces the point where the
 * reference's sequential frame loop has every coded frame in one process
 * (src/III.py:77-115 encode, :132-144 decode).  librccl is opened on first
 * use (dlopen); without it these return VCF_ERR_UNSUPPORTED.  Buffers are
 * device pointers, work is enqueued on `stream`. */
#define VCF_COMM_ID_BYTES 128
#define VCF_COMM_SUM 0
#define VCF_COMM_MAX 1
#define VCF_COMM_MIN 2
typedef struct vcf_comm *vcf_comm_t;

/* One rank creates the id (ncclGetUniqueId) and hands it to the others
 * out of band (vcf_amd/comm.py: a TCP host group). */
int vcf_comm_unique_id(uint8_t *id, size_t capacity);
/* Collective over `world` processes, each with its device already set
 * (vcf_set_device).  The communicator is non-blocking (ncclConfig_t
 * blocking = 0): initialisation and every enqueue below are polled against
 * a deadline of timeout_ms (<= 0: VCF_COMM_TIMEOUT_MS from the environment,
 * else 120000); past it the communicator is aborted (ncclCommAbort) and the
 * call returns VCF_ERR_TIMEOUT instead of hanging.  vcf_comm_init =
 * vcf_comm_init_timeout(..., 0). */
int vcf_comm_init(vcf_comm_t *comm, const uint8_t *id, int rank, int world);
int vcf_comm_init_timeout(vcf_comm_t *comm, const uint8_t *id, int rank, int world, int64_t timeout_ms);
/* Wait until everything enqueued on `stream` has finished, within the
 * communicator's timeout; past it (or on an asynchronous RCCL error) the
 * communicator is aborted and VCF_ERR_TIMEOUT (VCF_ERR_HIP) returned. */
int vcf_comm_wait(vcf_comm_t comm, void *stream);
int vcf_comm_destroy(vcf_comm_t comm);
int vcf_comm_rank(vcf_comm_t comm, int *rank, int *world);
/* recv_dev[r * count + i] = rank r's send_dev[i] (ncclAllGather, int64). */
int vcf_comm_allgather_i64(vcf_comm_t comm, const int64_t *send_dev, int64_t count, int64_t *recv_dev,
                           void *stream);
/* Element-wise VCF_COMM_SUM / MAX / MIN over ranks (ncclAllReduce, float64). */
int vcf_comm_allreduce_f64(vcf_comm_t comm, const double *send_dev, double *recv_dev, int64_t count, int op,
                           void *stream);
/* Gather with per-rank byte counts: rank r sends counts[r] bytes (= send_bytes)
 * and the root receives them packed in rank order in recv_dev.  counts (host,
 * `world` entries, the same on every rank -- e.g. from the size all-gather).
 * One grouped ncclSend per peer, P-1 concurrent ncclRecv on the root: each
 * xGMI peer uses its own link to the root (RCCL has no gatherv). */
int vcf_comm_gatherv(vcf_comm_t comm, const void *send_dev, int64_t send_bytes, void *recv_dev,
                     const int64_t *counts, int root, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VCF_AMD_H */
