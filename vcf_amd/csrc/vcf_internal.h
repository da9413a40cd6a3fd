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
}  // namespace vcf
