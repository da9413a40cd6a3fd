// vcf_ipp_mvrefine.hip -- the rate-aware refinement of a motion field
// (--mv_lambda, not in the reference): every block re-decides its vector among
// its own, the coder's predictor, its four neighbours' and zero by
// J = SAD + lambda * R, with R the bits the motion-field coder (vcf_mvc.cpp)
// would spend; vcf_ipp_mv_refine and vcf_ipp_mv_refine_workspace_bytes of the C
// ABI.  The rule is stated in include/vcf_amd.h ("Coded motion fields") and
// restated in numpy by tests/mvc_ref.py; everything is integer arithmetic, so
// the GPU and the numpy restatement agree bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"
#include "vcf_ipp_qpel.h"   // bilinear, axis_valid, quarter_pels
#include "vcf_mvc.h"        // mv_median3, mv_rate

namespace vcf {
namespace {

constexpr int kMaxBs = 64;
constexpr int kMaxLambda = 1024;
constexpr int kMaxIterations = 4;
constexpr int kCandidates = 7;

// the field inside the workspace: the first 4-byte aligned address after the two gray planes
inline float *second_field(uint8_t *ws, int32_t H, int32_t W)
{
    return reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(ws) + 2ULL * H * W + 3) & ~(uintptr_t)3);
}

__device__ __forceinline__ MvQ load_q(const float *__restrict__ f, int nbx, int by, int bx)
{
    const float *m = f + ((long long)by * nbx + bx) * 2;
    return {quarter_pels(m[0]), quarter_pels(m[1])};
}

// One iteration, f_in -> f_out: one wave per block.  The block of cur sits in
// LDS (as words); lane 0 lists the candidates (present, valid and no duplicate
// of a lower index, which could not win the tie) with their rate term, then the
// wave takes them one at a time: where fx = fy = 0 and whole words can be read
// (bs % 4 == 0, the reference plane 4-byte aligned) a lane compares 4 pixels
// with v_alignbyte + v_sad_u8, else pixel by pixel through the bilinear sample,
// whose zero-weight taps are not read.  The scan for the first strict minimum of
// J is wave-uniform.
__global__ __launch_bounds__(64) void ipp_mv_refine_kernel(const uint8_t *__restrict__ ref,
                                                           const uint8_t *__restrict__ cur, int H, int W, int bs,
                                                           int step, int lambda, int ref_words,
                                                           const float *__restrict__ f_in, float *__restrict__ f_out)
{
    __shared__ uint32_t cbw[kMaxBs * kMaxBs / 4];
    __shared__ int cand[kCandidates][4];   // qx, qy, lambda * R, evaluate
    uint8_t *cb = reinterpret_cast<uint8_t *>(cbw);
    const int bx = blockIdx.x, by = blockIdx.y, lane = threadIdx.x;
    const int nbx = gridDim.x, nby = gridDim.y;
    const int i = by * bs, j = bx * bs;
    for (int t = lane; t < bs * bs; t += 64) cb[t] = cur[(long long)(i + t / bs) * W + j + t % bs];
    if (lane == 0) {
        const MvQ zero = {0, 0};
        const MvQ own = load_q(f_in, nbx, by, bx);
        const MvQ left = bx > 0 ? load_q(f_in, nbx, by, bx - 1) : zero;
        const MvQ top = by > 0 ? load_q(f_in, nbx, by - 1, bx) : zero;
        MvQ p = left;
        if (by > 0) {
            const MvQ c = bx + 1 < nbx ? load_q(f_in, nbx, by - 1, bx + 1)
                                       : (bx > 0 ? load_q(f_in, nbx, by - 1, bx - 1) : zero);
            p = {mv_median3(left.x, top.x, c.x), mv_median3(left.y, top.y, c.y)};
        }
        MvQ c[kCandidates] = {own, p, left, top, zero, zero, zero};
        bool have[kCandidates] = {true, true, bx > 0, by > 0, bx + 1 < nbx, by + 1 < nby, true};
        if (have[4]) c[4] = load_q(f_in, nbx, by, bx + 1);
        if (have[5]) c[5] = load_q(f_in, nbx, by + 1, bx);
        for (int k = 0; k < kCandidates; ++k) {
            bool go = have[k] && axis_valid(4LL * j + c[k].x, bs, W) && axis_valid(4LL * i + c[k].y, bs, H);
            for (int e = 0; e < k; ++e) go = go && !(have[e] && c[e].x == c[k].x && c[e].y == c[k].y);
            cand[k][0] = c[k].x;
            cand[k][1] = c[k].y;
            cand[k][2] = go ? lambda * mv_rate(c[k], p, step) : 0;
            cand[k][3] = go;
        }
    }
    __syncthreads();
    uint32_t best = 0xFFFFFFFFu;
    int wx = 0, wy = 0;
    const int wpr = bs >> 2;   // words per block row on the word path
#pragma unroll 1
    for (int k = 0; k < kCandidates; ++k) {
        if (!__builtin_amdgcn_readfirstlane(cand[k][3])) continue;
        const int qx = __builtin_amdgcn_readfirstlane(cand[k][0]), qy = __builtin_amdgcn_readfirstlane(cand[k][1]);
        const int X = 4 * j + qx, Y = 4 * i + qy;   // valid: inside the frame
        const uint32_t fx = (uint32_t)(X & 3), fy = (uint32_t)(Y & 3);
        const uint8_t *r0 = ref + (long long)(Y >> 2) * W + (X >> 2);
        uint32_t s = 0;
        if (fx == 0 && fy == 0 && ref_words && (bs & 3) == 0) {
            for (int t = lane; t < wpr * bs; t += 64) {
                const int y = t / wpr, x = (t - y * wpr) * 4;
                const uintptr_t a = reinterpret_cast<uintptr_t>(r0 + (long long)y * W + x);
                // the word after the last pixels' lies in cur's plane, which follows ref's
                const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
                s = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(a & 3)), cbw[t], s);
            }
        } else {
            for (int t = lane; t < bs * bs; t += 64) {
                const int y = t / bs, x = t - y * bs;
                const uint8_t *p = r0 + (long long)y * W + x;
                const uint32_t a = p[0], b = fx ? p[1] : 0u, c = fy ? p[W] : 0u, d = (fx && fy) ? p[W + 1] : 0u;
                s += (uint32_t)abs((int)cb[t] - (int)bilinear(a, b, c, d, fx, fy));
            }
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const uint32_t J = s + (uint32_t)__builtin_amdgcn_readfirstlane(cand[k][2]);   // <= 64*64*255 + 1024*122
        if (J < best) {
            best = J;
            wx = qx;
            wy = qy;
        }
    }
    if (lane == 0) {   // candidate 6, (0, 0), is always valid: there is a winner
        float *m = f_out + ((long long)by * nbx + bx) * 2;
        m[0] = (float)wx * 0.25f;   // exact: a valid vector is far below 2^24
        m[1] = (float)wy * 0.25f;
    }
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_ipp_mv_refine_workspace_bytes(int32_t H, int32_t W, int32_t bs, int64_t *bytes)
{
    if (!bytes) return set_error(VCF_ERR_INVALID, "null pointer");
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad frame shape");
    if (bs < 1 || bs > kMaxBs) return set_error(VCF_ERR_INVALID, "block size %d (1..%d)", bs, kMaxBs);
    *bytes = 2LL * H * W + 3 + 8LL * (H / bs) * (W / bs);
    return VCF_OK;
}

int vcf_ipp_mv_refine(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                      int32_t subpel, int32_t lambda, int32_t iterations, float *mv_dev, uint8_t *workspace_dev,
                      int64_t workspace_bytes, void *stream)
{
    if (!ref_rgb_dev || !cur_rgb_dev || !mv_dev || !workspace_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(mv_dev, 4);
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad frame shape");
    if (subpel != 1 && subpel != 2 && subpel != 4)
        return set_error(VCF_ERR_INVALID, "sub-pel precision %d (1, 2 or 4)", subpel);
    if (bs < 1 || bs > kMaxBs) return set_error(VCF_ERR_INVALID, "block size %d (1..%d)", bs, kMaxBs);
    if (lambda < 0 || lambda > kMaxLambda) return set_error(VCF_ERR_INVALID, "lambda %d (0..%d)", lambda, kMaxLambda);
    if (iterations < 1 || iterations > kMaxIterations)
        return set_error(VCF_ERR_INVALID, "%d iterations (1..%d)", iterations, kMaxIterations);
    const int nbx = W / bs, nby = H / bs;
    if (nby > 65535) return set_error(VCF_ERR_INVALID, "%d block rows (at most 65535)", nby);
    const long long need = 2LL * H * W + 3 + 8LL * nby * nbx;
    if (workspace_bytes < need)
        return set_error(VCF_ERR_INVALID, "workspace of %lld bytes (vcf_ipp_mv_refine_workspace_bytes: %lld)",
                         (long long)workspace_bytes, need);
    if (nbx == 0 || nby == 0) return VCF_OK;
    hipStream_t s = (hipStream_t)stream;
    ipp_gray_planes(ref_rgb_dev, cur_rgb_dev, H, W, workspace_dev, stream);
    // ping-pong between mv_dev and the workspace's field so that the last iteration writes mv_dev
    float *other = second_field(workspace_dev, H, W);
    float *src = mv_dev, *dst = other;
    if (iterations & 1) {
        const int rc = hip_check(hipMemcpyAsync(other, mv_dev, 8ULL * nby * nbx, hipMemcpyDeviceToDevice, s),
                                 "ipp mv refine field copy");
        if (rc != VCF_OK) return rc;
        src = other;
        dst = mv_dev;
    }
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(ipp_mv_refine_kernel, dim3(nbx, nby), dim3(64), 0, s, workspace_dev,
                           workspace_dev + (long long)H * W, H, W, bs, 4 / subpel, lambda,
                           (int)aligned_to(workspace_dev, 4), src, dst);
        float *t = src;
        src = dst;
        dst = t;
    }
    return hip_check(hipGetLastError(), "ipp mv refinement launch");
}

}  // extern "C"
