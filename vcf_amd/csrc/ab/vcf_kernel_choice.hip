// vcf_kernel_choice.hip -- the product entries that choose between two kernels,
// with the choice as a leading argument (include/vcf_amd_ab.h): the tiled CBAAC
// coders (a wave or a lane per segment) and the IPP block matching (word or byte
// kernels).  No kernel is built here: the twins call the product's own entries
// (vcf_internal.h; csrc/vcf_cbaac_gpu.hip and csrc/vcf_ipp.hip are linked into
// this library), which check every argument but the choice.
#include "vcf_amd.h"
#include "vcf_amd_ab.h"
#include "vcf_internal.h"

using namespace vcf;

static int check_kernel(int32_t kernel)
{
    if (kernel < 0 || kernel > 2) return set_error(VCF_ERR_INVALID, "tiled CBAAC variant %d (0, 1, 2)", kernel);
    return VCF_OK;
}

extern "C" {

int vcf_cbaac_tiled_encode_variant(int32_t kernel, const uint8_t *sym_dev, int64_t n, int32_t order, int64_t seg_len,
                                   uint8_t *out_dev, int64_t out_capacity, int64_t *seg_bytes_dev, void *ws_dev,
                                   void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_encode(kernel, sym_dev, n, order, seg_len, out_dev, out_capacity, seg_bytes_dev, ws_dev, stream);
}

int vcf_cbaac_tiled_decode_variant(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev, int64_t n,
                                   int32_t order, int64_t seg_len, uint8_t *sym_dev, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_decode(kernel, in_dev, seg_offsets_dev, n, order, seg_len, sym_dev, stream);
}

int vcf_cbaac_tiled_encode_prior_variant(int32_t kernel, const uint8_t *sym_dev, int64_t n, int32_t order,
                                         const uint16_t *prior_dev, int64_t seg_len, uint8_t *out_dev,
                                         int64_t out_capacity, int64_t *seg_bytes_dev, void *ws_dev, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_encode_prior(kernel, sym_dev, n, order, prior_dev, seg_len, out_dev, out_capacity, seg_bytes_dev,
                                    ws_dev, stream);
}

int vcf_cbaac_tiled_decode_prior_variant(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev,
                                         int64_t n, int32_t order, const uint16_t *prior_dev, int64_t seg_len,
                                         uint8_t *sym_dev, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_decode_prior(kernel, in_dev, seg_offsets_dev, n, order, prior_dev, seg_len, sym_dev, stream);
}

int vcf_cbaac_tiled_encode_frames_variant(int32_t kernel, const uint8_t *sym_dev, int64_t n_frames,
                                          int64_t frame_symbols, int64_t frame_stride, int32_t order,
                                          const uint16_t *priors_dev, int64_t seg_len, uint8_t *out_dev,
                                          int64_t out_frame_capacity, int64_t *seg_bytes_dev, void *ws_dev, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_encode_frames(kernel, sym_dev, n_frames, frame_symbols, frame_stride, order, priors_dev, seg_len,
                                     out_dev, out_frame_capacity, seg_bytes_dev, ws_dev, stream);
}

int vcf_cbaac_tiled_decode_frames_variant(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev,
                                          int64_t n_frames, int64_t frame_symbols, int32_t order,
                                          const uint16_t *priors_dev, int64_t seg_len, uint8_t *sym_dev,
                                          int64_t out_frame_stride, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_decode_frames(kernel, in_dev, seg_offsets_dev, n_frames, frame_symbols, order, priors_dev, seg_len,
                                     sym_dev, out_frame_stride, stream);
}

int vcf_cbaac_tiled_encode_classes_variant(int32_t kernel, const uint8_t *sym_dev, int64_t n_frames,
                                           int64_t frame_symbols, int64_t frame_stride, int32_t order,
                                           const uint16_t *priors_dev, int32_t nclass, int64_t seg_len,
                                           uint8_t *out_dev, int64_t out_frame_capacity, int64_t *seg_bytes_dev,
                                           void *ws_dev, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_encode_classes(kernel, sym_dev, n_frames, frame_symbols, frame_stride, order, priors_dev, nclass,
                                      seg_len, out_dev, out_frame_capacity, seg_bytes_dev, ws_dev, stream);
}

int vcf_cbaac_tiled_decode_classes_variant(int32_t kernel, const uint8_t *in_dev, const int64_t *seg_offsets_dev,
                                           int64_t n_frames, int64_t frame_symbols, int32_t order,
                                           const uint16_t *priors_dev, int32_t nclass, int64_t seg_len,
                                           uint8_t *sym_dev, int64_t out_frame_stride, void *stream)
{
    if (int s = check_kernel(kernel)) return s;
    return cbaac_tiled_decode_classes(kernel, in_dev, seg_offsets_dev, n_frames, frame_symbols, order, priors_dev, nclass,
                                      seg_len, sym_dev, out_frame_stride, stream);
}

int vcf_ipp_block_match_variant(int32_t variant, const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H,
                                int32_t W, int32_t bs, int32_t sr, int32_t fast, float *mv_dev,
                                uint8_t *gray_workspace_dev, void *stream)
{
    if (variant < 0 || variant > 1) return set_error(VCF_ERR_INVALID, "unknown full-search variant %d", variant);
    return ipp_block_match(variant, ref_rgb_dev, cur_rgb_dev, H, W, bs, sr, fast, mv_dev, gray_workspace_dev, stream);
}

}  // extern "C"
