// vcf_ipp_qpel.h -- the quarter-pel arithmetic that the sub-pel compensator
// (vcf_ipp_subpel.hip) and the overlapped one (vcf_ipp_obmc.hip) share: the
// bilinear sample, a vector's validity along one axis, the float -> quarter-pel
// rounding and the 7-byte read through aligned words.  The rule is stated in
// include/vcf_amd.h ("Sub-pel motion").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vcf {

__device__ __forceinline__ uint32_t bilinear(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t fx, uint32_t fy)
{
    return ((4 - fx) * (4 - fy) * a + fx * (4 - fy) * b + (4 - fx) * fy * c + fx * fy * d + 8) >> 4;
}

// ix >= 0 and ix + bs + (fx ? 1 : 0) <= n for X = 4 ix + fx
__device__ __forceinline__ bool axis_valid(long long X, int bs, int n)
{
    const long long ix = X >> 2;
    return ix >= 0 && ix + bs + ((X & 3) ? 1 : 0) <= n;
}

// q = lrintf(4 m), clamped far outside any frame first (NaN and huge values end invalid)
__device__ __forceinline__ int quarter_pels(float m)
{
    const float f = fminf(fmaxf(rintf(4.f * m), -268435456.f), 268435456.f);   // +-2^28; fmaxf drops a NaN
    return (int)f;
}

// bytes s .. s + 3 and s + 3 .. s + 6 of the frame out of the three aligned words that hold them
__device__ __forceinline__ void seven_bytes(const uint8_t *__restrict__ ref, long long s, uint32_t &lo, uint32_t &hi)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(ref + (s & ~3LL));
    const uint32_t o = (uint32_t)(s & 3);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    lo = __builtin_amdgcn_alignbyte(w1, w0, o);
    hi = __builtin_amdgcn_alignbyte(__builtin_amdgcn_alignbyte(w2, w1, o), lo, 3);
}

}  // namespace vcf
