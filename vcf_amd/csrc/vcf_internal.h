// vcf_internal.h -- helpers shared by the translation units of libvcf_amd.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace vcf {
int set_error(int code, const char *fmt, ...);
int hip_check(hipError_t e, const char *what);

// Pointer alignment (include/vcf_amd.h, "Alignment and extents"): byte-typed frames need none, so an
// entry point takes its vector path only where aligned_to() allows it; a typed pointer off its
// element's alignment is an argument error (VCF_ERR_INVALID before any device work).
inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// A little-endian u16 inside a byte-typed buffer (the packed LL band of the 2D-DWT): one 16-bit
// access at an even address, two bytes at an odd one -- a frame of a batch starts at an odd address
// whenever the packed frame size is odd.  Device code only.  The buffer form keeps the callers' dropped stores dropped:
// an offset with bit 31 set stays past the buffer at offset + 1.
#if defined(__HIP__)
__device__ __forceinline__ uint16_t load_u16_le(const uint8_t *p)
{
    if ((reinterpret_cast<uintptr_t>(p) & 1) == 0) return *reinterpret_cast<const uint16_t *>(p);
    return (uint16_t)(p[0] | (p[1] << 8));
}
__device__ __forceinline__ void buffer_store_u16_le(uint16_t v, __amdgpu_buffer_rsrc_t rs, const uint8_t *base,
                                                    uint32_t off)
{
    if (((reinterpret_cast<uintptr_t>(base) + off) & 1) == 0) {
        __builtin_amdgcn_raw_buffer_store_b16(v, rs, off, 0, 0);
    } else {
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)v, rs, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(v >> 8), rs, off + 1, 0, 0);
    }
}
#endif
#define VCF_REQUIRE_ALIGNED(p, a)                                                                    \
    do {                                                                                             \
        if ((p) && !vcf::aligned_to((p), (a)))                                                       \
            return vcf::set_error(VCF_ERR_INVALID, #p " must be %d-byte aligned", (int)(a));         \
    } while (0)

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
// Its two steps, for the hierarchical search (vcf_ipp_hier.hip): the gray pass of both frames (ref's
// luma at gray_dev, cur's at gray_dev + H * W) and the search on two H x W luma planes; and the
// sub-pel refinement of an integer field on two luma planes (vcf_ipp_subpel.hip).  Launches only:
// the caller has checked the arguments and that the field is not empty.
void ipp_gray_planes(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, uint8_t *gray_dev,
                     void *stream);
void ipp_plane_search(int32_t variant, const uint8_t *ref_gray_dev, const uint8_t *cur_gray_dev, int32_t H, int32_t W,
                      int32_t bs, int32_t sr, int32_t fast, float *mv_dev, void *stream);
void ipp_subpel_refine(const uint8_t *ref_gray_dev, const uint8_t *cur_gray_dev, int32_t H, int32_t W, int32_t bs,
                       int32_t subpel, float *mv_dev, void *stream);

// The kernel schedule of one 2D-DWT call (vcf_dwt.hip); the defaults are the library's rules.  The
// product entry points pass DwtSchedule{}; the A/B library's vcf_dwt_dz_*_sched twins
// (ab/vcf_dwt_sched.hip, include/vcf_amd_ab.h) pass a caller's.  Every setting gives the same bytes.
struct DwtSchedule {
    int enc_bands = 0;        // bands of the level 1 + 2 kernel (0 = the cost model)
    int dec_line_bands = 0;   // bands of each inverse line launch (0 = the cost model)
    int dec21_brows = 0;      // level-1 rows per band of the inverse levels 2 + 1 kernel (0 = its rule)
    int enc_pipe = -1;        // the encode as a frame pipeline: -1 = the rule, 0 off, 1 on where pipeline_default
    int dec_pipe = -1;        // the decode likewise (the rule: off)
    int band21 = 1;           // inverse levels 2 and 1 in one launch where band21_ok
    int lift_fused = 1;       // the lifting form's level pairs in one launch
};
int dwt_encode(const DwtSchedule &sc, const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t wavelet,
               int32_t levels, int32_t Q, uint8_t *packed_dev, void *workspace_dev, void *stream);
int dwt_decode(const DwtSchedule &sc, const uint8_t *packed_dev, int64_t n_frames, int32_t H, int32_t W,
               int32_t wavelet, int32_t levels, int32_t Q, uint8_t *rgb_dev, void *workspace_dev, void *stream);
int dwt_encode_lift(const DwtSchedule &sc, const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W,
                    int32_t wavelet, int32_t levels, int32_t Q, uint8_t *packed_dev, void *workspace_dev,
                    void *stream);
int dwt_decode_lift(const DwtSchedule &sc, const uint8_t *packed_dev, int64_t n_frames, int32_t H, int32_t W,
                    int32_t wavelet, int32_t levels, int32_t Q, uint8_t *rgb_dev, void *workspace_dev,
                    void *stream);
}  // namespace vcf
