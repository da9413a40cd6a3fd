// vcf_internal.h -- helpers shared by the translation units of libvcf_amd.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace vcf {
int set_error(int code, const char *fmt, ...);
int hip_check(hipError_t e, const char *what);

// A batch whose frames are a grid's y or z dimension, in launches of at most 65535 of them (the
// dimension's limit): launch(f0, nf) enqueues frames f0 .. f0 + nf - 1, `what` names it in the
// error.  Returns the first launch's error, or 0.
template <typename Launch>
int for_frame_chunks(int64_t n_frames, const char *what, Launch launch)
{
    for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {
        launch(f0, (unsigned)std::min<int64_t>(65535, n_frames - f0));
        const int rc = hip_check(hipGetLastError(), what);
        if (rc != 0) return rc;
    }
    return 0;
}

// block sizes other than 8 (vcf_dct_any.hip)
int dct_any_encode_u8(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t B, int32_t Q,
                      uint32_t flags, uint8_t *k_dev, void *stream);
int dct_any_decode_u8(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t B, int32_t Q,
                      uint32_t flags, uint8_t *rgb_dev, void *stream);

// The entries that choose between two kernels, the choice in front of the product signature: the
// product names pass 0 (the rule), the A/B library's *_variant twins (ab/vcf_kernel_choice.hip,
// include/vcf_amd_ab.h) the caller's.  Tiled CBAAC (vcf_cbaac_gpu.hip), kernel: 0 = order 0 codes a
// lane per segment from 4608 segments to encode / 6144 to decode on, 1 = a wave per segment,
// 2 = a lane per segment for order 0.
int cbaac_tiled_encode(int32_t kernel, const uint8_t *sym_dev, int64_t n, int32_t order, int64_t seg_len,
                       uint8_t *out_dev, int64_t out_capacity, int64_t *seg_bytes_dev, void *ws_dev, void *stream);
int cbaac_tiled_decode(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n, int32_t order,
                       int64_t seg_len, uint8_t *sym_dev, void *stream);
int cbaac_tiled_encode_prior(int32_t kernel, const uint8_t *sym_dev, int64_t n, int32_t order,
                             const uint16_t *prior_dev, int64_t seg_len, uint8_t *out_dev, int64_t out_capacity,
                             int64_t *seg_bytes_dev, void *ws_dev, void *stream);
int cbaac_tiled_decode_prior(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n,
                             int32_t order, const uint16_t *prior_dev, int64_t seg_len, uint8_t *sym_dev, void *stream);
int cbaac_tiled_encode_frames(int32_t kernel, const uint8_t *sym_dev, int64_t n_frames, int64_t frame_symbols,
                              int64_t frame_stride, int32_t order, const uint16_t *priors_dev, int64_t seg_len,
                              uint8_t *out_dev, int64_t out_frame_capacity, int64_t *seg_bytes_dev, void *ws_dev,
                              void *stream);
int cbaac_tiled_decode_frames(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n_frames,
                              int64_t frame_symbols, int32_t order, const uint16_t *priors_dev, int64_t seg_len,
                              uint8_t *sym_dev, int64_t out_frame_stride, void *stream);
int cbaac_tiled_encode_classes(int32_t kernel, const uint8_t *sym_dev, int64_t n_frames, int64_t frame_symbols,
                               int64_t frame_stride, int32_t order, const uint16_t *priors_dev, int32_t nclass,
                               int64_t seg_len, uint8_t *out_dev, int64_t out_frame_capacity, int64_t *seg_bytes_dev,
                               void *ws_dev, void *stream);
int cbaac_tiled_decode_classes(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n_frames,
                               int64_t frame_symbols, int32_t order, const uint16_t *priors_dev, int32_t nclass,
                               int64_t seg_len, uint8_t *sym_dev, int64_t out_frame_stride, void *stream);
// Block matching (vcf_ipp.hip), variant: 0 = the word kernels where the block size allows, 1 = the byte kernels
int ipp_block_match(int32_t variant, const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W,
                    int32_t bs, int32_t sr, int32_t fast, float *mv_dev, uint8_t *gray_workspace_dev, void *stream);
}  // namespace vcf
