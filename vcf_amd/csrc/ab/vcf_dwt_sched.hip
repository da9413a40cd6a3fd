// vcf_dwt_sched.hip -- the product 2D-DWT entries with a vcf_dwt_schedule
// (include/vcf_amd_ab.h) in front of the product signature.  No kernel is built
// here: the twins call the product's own entries (vcf_internal.h; csrc/vcf_dwt.hip
// is linked into this library).  Every schedule gives the product's bytes
// (tests/test_dwt_gpu.py); the A/B runs are scripts/dwt_sched_ab.py.
#include "vcf_amd_ab.h"
#include "vcf_internal.h"

using namespace vcf;

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
