// vcf_dwt_sched.hip -- the product 2D-DWT (csrc/vcf_dwt.hip: the same kernels
// and launch code) built for the A/B library with the kernel schedule as an
// argument: vcf_dwt_dz_*_sched take a vcf_dwt_schedule (include/vcf_amd_ab.h)
// in front of the product signature.  Under VCF_DWT_SCHED_BUILD vcf_dwt.hip
// leaves out its extern "C" names (ab/vcf_dwt_ab.hip defines vcf_dwt_dz_encode,
// _decode, vcf_dwt_layout and vcf_wavelet_index in this library).  Every
// schedule gives the product's bytes (tests/test_dwt_gpu.py); the A/B runs are
// scripts/dwt_sched_ab.py.
#define VCF_DWT_SCHED_BUILD 1
#include "vcf_amd_ab.h"
#include "vcf_dwt.hip"

// NULL = the library's rules
static DwtSchedule schedule_of(const vcf_dwt_schedule *p)
{
    if (!p) return DwtSchedule{};
    return DwtSchedule{p->enc_bands, p->dec_line_bands, p->dec21_brows, p->enc_pipe, p->dec_pipe, p->band21, p->lift_fused};
}

extern "C" {

int vcf_dwt_dz_encode_sched(const vcf_dwt_schedule *sched, const uint8_t *rgb_dev, int64_t n_frames, int32_t H,
                            int32_t W, int32_t wavelet, int32_t levels, int32_t Q, uint8_t *packed_dev,
                            void *workspace_dev, void *stream)
{
    return dwt_encode(schedule_of(sched), rgb_dev, n_frames, H, W, wavelet, levels, Q, packed_dev, workspace_dev, stream);
}

int vcf_dwt_dz_decode_sched(const vcf_dwt_schedule *sched, const uint8_t *packed_dev, int64_t n_frames, int32_t H,
                            int32_t W, int32_t wavelet, int32_t levels, int32_t Q, uint8_t *rgb_dev,
                            void *workspace_dev, void *stream)
{
    return dwt_decode(schedule_of(sched), packed_dev, n_frames, H, W, wavelet, levels, Q, rgb_dev, workspace_dev, stream);
}

int vcf_dwt_dz_encode_lift_sched(const vcf_dwt_schedule *sched, const uint8_t *rgb_dev, int64_t n_frames, int32_t H,
                                 int32_t W, int32_t wavelet, int32_t levels, int32_t Q, uint8_t *packed_dev,
                                 void *workspace_dev, void *stream)
{
    return dwt_encode_lift(schedule_of(sched), rgb_dev, n_frames, H, W, wavelet, levels, Q, packed_dev, workspace_dev,
                           stream);
}

int vcf_dwt_dz_decode_lift_sched(const vcf_dwt_schedule *sched, const uint8_t *packed_dev, int64_t n_frames, int32_t H,
                                 int32_t W, int32_t wavelet, int32_t levels, int32_t Q, uint8_t *rgb_dev,
                                 void *workspace_dev, void *stream)
{
    return dwt_decode_lift(schedule_of(sched), packed_dev, n_frames, H, W, wavelet, levels, Q, rgb_dev, workspace_dev,
                           stream);
}

}  // extern "C"
