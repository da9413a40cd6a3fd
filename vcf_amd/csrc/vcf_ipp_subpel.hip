// vcf_ipp_subpel.hip -- half- and quarter-pel motion for the IPP loop (--subpel,
// not in the reference): the refinement of the integer block match and the
// bilinear compensator; vcf_ipp_block_match_subpel and
// vcf_ipp_motion_compensate_qpel of the C ABI.  The rule is stated in
// include/vcf_amd.h ("Sub-pel motion") and restated in numpy by
// tests/subpel_ref.py; everything is integer arithmetic, so the GPU and the
// numpy restatement agree bit for bit.
//
// Vectors are in quarter-pel units q; a block at (i, j) reads the reference
// from X = 4 j + qx: ix = X >> 2, fx = X & 3 (same for y), and a sample is
//   p = ((4-fx)(4-fy) a + fx (4-fy) b + (4-fx) fy c + fx fy d + 8) >> 4
// over a = r[y, x], b = r[y, x+1], c = r[y+1, x], d = r[y+1, x+1].  A vector
// is valid iff every sample with a non-zero weight lies in the frame.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"
#include "vcf_ipp_qpel.h"   // bilinear, axis_valid, quarter_pels, seven_bytes

namespace vcf {
namespace {

constexpr int kMaxBs = 64;
constexpr int kMaxSr = 32;

// Refinement around the integer winner that mv holds: one wave per block.  The
// block of cur and the (bs + 2)^2 luma window of ref around the integer winner
// sit in LDS: a candidate is at most 3 quarter-pels from the winner, so it
// reads columns ix0 - 1 .. ix0 + bs (rows alike); window entries outside the
// frame are 0 and belong only to invalid candidates or to zero weights.  Per
// stage the lanes go over the block's pixels once and keep one partial SAD per
// neighbour (8, and the centre's in the first stage), then a wave reduction per
// candidate; the scan for the first strict minimum is wave-uniform.
__global__ __launch_bounds__(64) void ipp_subpel_refine_kernel(const uint8_t *__restrict__ ref,
                                                               const uint8_t *__restrict__ cur, int H, int W, int bs,
                                                               int subpel, float *__restrict__ mv)
{
    __shared__ uint8_t cb[kMaxBs * kMaxBs];
    __shared__ uint8_t win[(kMaxBs + 2) * (kMaxBs + 2)];
    const int bx = blockIdx.x, by = blockIdx.y, lane = threadIdx.x;
    const int i = by * bs, j = bx * bs;
    float *m = mv + ((long long)by * gridDim.x + bx) * 2;
    const int ry = i + (int)m[1], rx = j + (int)m[0];   // the integer winner: in bounds by construction
    const int wp = bs + 2;
    for (int t = lane; t < bs * bs; t += 64) cb[t] = cur[(long long)(i + t / bs) * W + j + t % bs];
    for (int t = lane; t < wp * wp; t += 64) {
        const int y = ry - 1 + t / wp, x = rx - 1 + t % wp;
        win[t] = (y >= 0 && y < H && x >= 0 && x < W) ? ref[(long long)y * W + x] : 0;
    }
    __syncthreads();
    int cox = 0, coy = 0;          // the centre, in quarter-pels from the integer winner
    uint32_t best = 0;
    for (int step = 2; step >= (subpel == 4 ? 1 : 2); step >>= 1) {
        const bool first = step == 2;
        bool valid[8];
        int off[8];
        uint32_t fxs[8], fys[8], s[9];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int kk = k + (k >= 4);   // scan order ddy outer, ddx inner, the centre skipped
            const int ox = cox + (kk % 3 - 1) * step, oy = coy + (kk / 3 - 1) * step;
            valid[k] = axis_valid(4LL * rx + ox, bs, W) && axis_valid(4LL * ry + oy, bs, H);
            off[k] = ((oy >> 2) + 1) * wp + (ox >> 2) + 1;
            fxs[k] = (uint32_t)(ox & 3);
            fys[k] = (uint32_t)(oy & 3);
            s[k] = 0;
        }
        s[8] = 0;
        for (int t = lane; t < bs * bs; t += 64) {
            const int y = t / bs, x = t - y * bs;
            const int c = cb[t];
            const uint8_t *w = win + y * wp + x;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (!valid[k]) continue;   // wave-uniform
                const uint8_t *p = w + off[k];
                s[k] += (uint32_t)abs(c - (int)bilinear(p[0], p[1], p[wp], p[wp + 1], fxs[k], fys[k]));
            }
            if (first) s[8] += (uint32_t)abs(c - (int)w[wp + 1]);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k)
            for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_xor(s[k], o, 64);
        if (first) best = s[8];
        int win_k = -1;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (valid[k] && s[k] < best) {
                best = s[k];
                win_k = k;
            }
        if (win_k >= 0) {
            const int kk = win_k + (win_k >= 4);
            cox += (kk % 3 - 1) * step;
            coy += (kk / 3 - 1) * step;
        }
    }
    if (lane == 0) {
        m[0] = (float)(4 * (rx - j) + cox) * 0.25f;   // exact: |q| < 2^24
        m[1] = (float)(4 * (ry - i) + coy) * 0.25f;
    }
}

// The block of pixel (y, x): its reference origin in quarter-pels, or the
// co-located block for an invalid vector.  q = lrintf(4 m), clamped far outside
// any frame first (NaN and huge values end invalid).
struct QpelBlock {
    int iy, ix;
    uint32_t fy, fx;
};

__device__ __forceinline__ QpelBlock qpel_block(const float *__restrict__ mv, int nbx, int by, int bx, int bs, int H,
                                                int W)
{
    const float *m = mv + ((long long)by * nbx + bx) * 2;
    const int i = by * bs, j = bx * bs;
    const long long X = 4LL * j + quarter_pels(m[0]), Y = 4LL * i + quarter_pels(m[1]);
    if (axis_valid(X, bs, W) && axis_valid(Y, bs, H))
        return {(int)(Y >> 2), (int)(X >> 2), (uint32_t)(Y & 3), (uint32_t)(X & 3)};
    return {i, j, 0u, 0u};
}

// one byte of the compensated frame: byte e of row y (pixel e / 3, channel e % 3)
__device__ uint8_t qpel_byte(const uint8_t *__restrict__ ref, const float *__restrict__ mv, int H, int W, int bs, int y,
                             int e)
{
    const int x = e / 3;
    const int nbx = W / bs, nby = H / bs;
    const int by = y / bs, bx = x / bs;
    if (by >= nby || bx >= nbx) return 0;   // outside the full-block area
    const QpelBlock b = qpel_block(mv, nbx, by, bx, bs, H, W);
    const long long rb = (long long)W * 3;
    const uint8_t *s = ref + (long long)(b.iy + y - by * bs) * rb + (long long)(b.ix - bx * bs) * 3 + e;
    // taps with weight 0 are not read: they may lie outside the frame
    const uint32_t a = s[0], t1 = b.fx ? s[3] : 0u, t2 = b.fy ? s[rb] : 0u, t3 = (b.fx && b.fy) ? s[rb + 3] : 0u;
    return (uint8_t)bilinear(a, t1, t2, t3, b.fx, b.fy);
}

// Compensation: a thread makes 4 consecutive bytes of one output row (grid.y =
// row).  Where the 4 bytes lie in one block and the reference is 4-byte aligned,
// the 7 reference bytes per tap row (4 samples and their right neighbours, 3
// bytes on) come from 3 aligned words through v_alignbyte; else byte by byte.
// The 4 bytes leave as one word where the output address is aligned.
__global__ __launch_bounds__(256) void ipp_mc_qpel_kernel(const uint8_t *__restrict__ ref,
                                                          const float *__restrict__ mv, int H, int W, int bs,
                                                          uint8_t *__restrict__ out, int ref_words)
{
    const int y = blockIdx.y;
    const long long rb = (long long)W * 3;
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e0 >= rb) return;
    const int ne = (int)(rb - e0 < 4 ? rb - e0 : 4);
    uint8_t *o = out + y * rb + e0;
    const int nbx = W / bs, nby = H / bs;
    const int x0 = (int)(e0 / 3), bx = x0 / bs, by = y / bs;
    uint32_t v = 0;
    bool done = false;
    if (ne == 4 && by < nby && bx < nbx && (int)((e0 + 3) / 3) < (bx + 1) * bs) {
        const QpelBlock b = qpel_block(mv, nbx, by, bx, bs, H, W);
        const long long s = (long long)(b.iy + y - by * bs) * rb + (long long)(b.ix - bx * bs) * 3 + e0;
        // the last tap row's three words end 12 bytes past its first aligned address
        const long long last = ((s + (b.fy ? rb : 0)) & ~3LL) + 12;
        if (ref_words && last <= (long long)H * rb) {
            uint32_t a, r, c = 0, d = 0;
            seven_bytes(ref, s, a, r);
            if (b.fy) seven_bytes(ref, s + rb, c, d);
#pragma unroll
            for (int n = 0; n < 4; ++n)
                v |= bilinear((a >> (8 * n)) & 0xFFu, (r >> (8 * n)) & 0xFFu, (c >> (8 * n)) & 0xFFu,
                              (d >> (8 * n)) & 0xFFu, b.fx, b.fy)
                     << (8 * n);
            done = true;
        }
    }
    if (!done)
        for (int n = 0; n < ne; ++n) v |= (uint32_t)qpel_byte(ref, mv, H, W, bs, y, (int)e0 + n) << (8 * n);
    if (ne == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(o) = v;
    } else {
        for (int n = 0; n < ne; ++n) o[n] = (uint8_t)(v >> (8 * n));
    }
}

}  // namespace

void ipp_subpel_refine(const uint8_t *ref_gray_dev, const uint8_t *cur_gray_dev, int32_t H, int32_t W, int32_t bs,
                       int32_t subpel, float *mv_dev, void *stream)
{
    hipLaunchKernelGGL(ipp_subpel_refine_kernel, dim3(W / bs, H / bs), dim3(64), 0, (hipStream_t)stream, ref_gray_dev,
                       cur_gray_dev, H, W, bs, subpel, mv_dev);
}
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_ipp_block_match_subpel(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                               int32_t sr, int32_t fast, int32_t subpel, float *mv_dev, uint8_t *gray_workspace_dev,
                               void *stream)
{
    if (subpel != 1 && subpel != 2 && subpel != 4)
        return set_error(VCF_ERR_INVALID, "sub-pel precision %d (1, 2 or 4)", subpel);
    if (bs < 1 || bs > kMaxBs) return set_error(VCF_ERR_INVALID, "block size %d (1..%d)", bs, kMaxBs);
    if (sr < 0 || sr > kMaxSr) return set_error(VCF_ERR_INVALID, "search range %d (0..%d)", sr, kMaxSr);
    const int rc = ipp_block_match(0, ref_rgb_dev, cur_rgb_dev, H, W, bs, sr, fast, mv_dev, gray_workspace_dev, stream);
    if (rc != VCF_OK || subpel == 1) return rc;
    const int nbx = W / bs, nby = H / bs;
    if (nbx == 0 || nby == 0) return VCF_OK;
    ipp_subpel_refine(gray_workspace_dev, gray_workspace_dev + (long long)H * W, H, W, bs, subpel, mv_dev, stream);
    return hip_check(hipGetLastError(), "ipp sub-pel refinement launch");
}

int vcf_ipp_motion_compensate_qpel(const uint8_t *ref_rgb_dev, const float *mv_dev, int32_t H, int32_t W, int32_t bs,
                                   uint8_t *out_rgb_dev, void *stream)
{
    if (!ref_rgb_dev || !mv_dev || !out_rgb_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(mv_dev, 4);
    if (H <= 0 || W <= 0 || bs < 1) return set_error(VCF_ERR_INVALID, "bad arguments");
    if (H > 65535) return set_error(VCF_ERR_UNSUPPORTED, "frame height %d (at most 65535 rows)", H);
    const unsigned per_row = (unsigned)(((long long)W * 3 + 3) / 4);
    hipLaunchKernelGGL(ipp_mc_qpel_kernel, dim3((per_row + 255) / 256, H), dim3(256), 0, (hipStream_t)stream,
                       ref_rgb_dev, mv_dev, H, W, bs, out_rgb_dev, (int)aligned_to(ref_rgb_dev, 4));
    return hip_check(hipGetLastError(), "ipp qpel mc launch");
}

}  // extern "C"
