// vcf_mvc.h -- the integer rule that the motion-field coder (vcf_mvc.cpp, host)
// and the rate-aware refinement (vcf_ipp_mvrefine.hip, device) share: the median
// predictor of a field of quarter-pel vectors and the length of a signed
// exp-Golomb code.  The rule is stated in include/vcf_amd.h ("Coded motion
// fields").
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VCF_MVC_HD __host__ __device__ inline
#else
#define VCF_MVC_HD inline
#endif

namespace vcf {

struct MvQ {
    int32_t x, y;
};

VCF_MVC_HD int32_t mv_median3(int32_t a, int32_t b, int32_t c)
{
    const int32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : (c > hi ? hi : c);
}

// p(by, bx) of the field q (rows of nbx vectors, x then y): the left vector in
// the first row, else the component-wise median of left, top and top right
// (top left in the last column); a neighbour outside the field is (0, 0).
VCF_MVC_HD MvQ mv_predictor(const int32_t *q, int32_t nbx, int32_t by, int32_t bx)
{
    const MvQ zero = {0, 0};
    const int32_t *v = q + ((int64_t)by * nbx + bx) * 2;
    const MvQ a = bx > 0 ? MvQ{v[-2], v[-1]} : zero;
    if (by == 0) return a;
    const int32_t *t = v - (int64_t)nbx * 2;
    const MvQ b = {t[0], t[1]};
    const MvQ c = bx + 1 < nbx ? MvQ{t[2], t[3]} : (bx > 0 ? MvQ{t[-2], t[-1]} : zero);
    return {mv_median3(a.x, b.x, c.x), mv_median3(a.y, b.y, c.y)};
}

// k = 2 d - 1 for d > 0, else -2 d
VCF_MVC_HD uint32_t mv_code_index(int32_t d) { return d > 0 ? 2u * (uint32_t)d - 1u : 2u * (uint32_t)(-(int64_t)d); }

// len(d) = 2 floor(log2(k + 1)) + 1; |d| < 2^30
VCF_MVC_HD int32_t mv_code_length(int32_t d) { return 2 * (31 - __builtin_clz(mv_code_index(d) + 1u)) + 1; }

// R(q, p): the division is C's, truncating toward zero
VCF_MVC_HD int32_t mv_rate(MvQ q, MvQ p, int32_t step)
{
    return mv_code_length((q.x - p.x) / step) + mv_code_length((q.y - p.y) / step);
}

}  // namespace vcf
