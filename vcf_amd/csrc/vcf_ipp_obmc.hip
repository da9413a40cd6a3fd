// vcf_ipp_obmc.hip -- overlapped block motion compensation for the IPP loop
// (--obmc, not in the reference): vcf_ipp_motion_compensate_obmc of the C ABI.
// The rule is stated in include/vcf_amd.h ("Overlapped block motion
// compensation") and restated in numpy by tests/obmc_ref.py; everything is
// integer arithmetic, so the GPU and the numpy restatement agree bit for bit.
//
// A pixel (y, x) of block (by, bx), at (v, u) inside it, is predicted from four
// vectors: its own block's, the nearer horizontal neighbour's, the nearer
// vertical neighbour's and the diagonal one's (neighbours clamped to the field).
// The own weights are wx = bs + 2u + 1 (u < bs/2) or 3 bs - 2u - 1, wy alike
// from v; a neighbour gets 2 bs - w.  Every vector samples the reference at the
// pixel's own position (bilinear, the four taps clamped to the frame) and
//   out = (sum wy_a wx_b P_ab + 2 bs^2) >> (2 log2 bs + 2).
// An invalid vector (its own block would read outside the frame) counts as 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"
#include "vcf_ipp_qpel.h"

namespace vcf {
namespace {

constexpr int kThreads = 256;
// A workgroup makes 4 * kThreads consecutive bytes of one row: at most 343 pixels, so at most
// 87 blocks of side >= 4, and one neighbour column on either side.
constexpr int kCols = 96;

// step 1 of the rule for block (by, bx): the vector in quarter pels, (0, 0) if it is invalid
__device__ __forceinline__ int2 resolve(const float *__restrict__ mv, int nbx, int by, int bx, int bs, int H, int W)
{
    const float *m = mv + ((long long)by * nbx + bx) * 2;
    const int qx = quarter_pels(m[0]), qy = quarter_pels(m[1]);
    const bool ok = axis_valid(4LL * bx * bs + qx, bs, W) && axis_valid(4LL * by * bs + qy, bs, H);
    return ok ? make_int2(qx, qy) : make_int2(0, 0);
}

// one axis of steps 3 and 4 for offset u in block b of n: the neighbour block and the own weight
__device__ __forceinline__ void overlap(int b, int u, int bs, int n, int &nb, uint32_t &w)
{
    const bool low = u < (bs >> 1);
    nb = min(max(b + (low ? -1 : 1), 0), n - 1);
    w = (uint32_t)(low ? bs + 2 * u + 1 : 3 * bs - 2 * u - 1);
}

// A pixel's two contributing block columns (as columns of the workgroup's table) and their weights.
struct Px {
    int col[2];
    uint32_t w[2];
    bool in;   // inside the full-block area
};

// Compensation: a thread makes 4 consecutive bytes of one output row (grid.y =
// row), as the quarter-pel kernel does.  The row's block row and its vertical
// neighbour are the same for the whole workgroup, which first resolves the
// vectors of those two block rows over its own columns and one more on either
// side into LDS, once per block.  The 4 bytes belong to two pixels, x0 and
// x0 + 1.  Under one vector the thread samples all 4 bytes: from 3 aligned words
// per tap row (v_alignbyte) where the reference is 4-byte aligned and no tap of
// either pixel clamps, else byte by byte with clamped taps.  Where both pixels
// have the same contributors (the same half of one block) the four samples
// serve both, each byte weighted for its own pixel; else the second pixel
// takes four samples of its own.
__global__ __launch_bounds__(kThreads) void ipp_mc_obmc_kernel(const uint8_t *__restrict__ ref,
                                                               const float *__restrict__ mv, int H, int W, int lg,
                                                               uint8_t *__restrict__ out, int ref_words)
{
    __shared__ int2 tab[2][kCols];   // [0]: the row's own block row, [1]: its vertical neighbour
    const int bs = 1 << lg;
    const int y = blockIdx.y;
    const long long rb = (long long)W * 3;
    const long long g0 = (long long)blockIdx.x * (4 * kThreads);   // the workgroup's first byte of the row
    const int nbx = W >> lg, nby = H >> lg;
    const int by = y >> lg;
    const bool row_in = by < nby;
    int nrow = 0;
    uint32_t wy[2] = {0u, 0u};
    if (row_in) {
        overlap(by, y - (by << lg), bs, nby, nrow, wy[0]);
        wy[1] = 2u * bs - wy[0];
    }
    // the block columns this workgroup's pixels and their neighbours lie in
    const long long last_byte = g0 + 4 * kThreads - 1 < rb - 1 ? g0 + 4 * kThreads - 1 : rb - 1;
    const int c0 = max((int)((g0 / 3) >> lg) - 1, 0);
    const int c1 = min((int)((last_byte / 3) >> lg) + 1, nbx - 1);
    const int ncols = min(c1 - c0 + 1, kCols);
    if (row_in)
        for (int t = threadIdx.x; t < 2 * ncols; t += kThreads) {
            const int a = t >= ncols, c = t - a * ncols;
            tab[a][c] = resolve(mv, nbx, a ? nrow : by, c0 + c, bs, H, W);
        }
    __syncthreads();
    const long long e0 = g0 + threadIdx.x * 4;
    if (e0 >= rb) return;
    const int ne = (int)(rb - e0 < 4 ? rb - e0 : 4);
    const int x0 = (int)(e0 / 3);
    const int n0 = 3 * (x0 + 1) - (int)e0;   // bytes 0 .. n0 - 1 are pixel x0's, the rest pixel x0 + 1's
    Px px[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int x = x0 + k, bx = x >> lg;
        px[k].in = row_in && bx < nbx;
        int nb = 0;
        uint32_t w = 0;
        if (px[k].in) overlap(bx, x - (bx << lg), bs, nbx, nb, w);
        px[k].col[0] = bx - c0;
        px[k].col[1] = nb - c0;
        px[k].w[0] = w;
        px[k].w[1] = 2u * bs - w;
    }
    const bool same = px[0].in && px[1].in && px[0].col[0] == px[1].col[0] && px[0].col[1] == px[1].col[1];
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < 2; ++k) {
        if (!px[k].in || (k && same)) continue;
#pragma unroll
        for (int ab = 0; ab < 4; ++ab) {
            const int a = ab >> 1, b = ab & 1;
            const int2 q = tab[a][px[k].col[b]];
            // the weight of this sample in the bytes of pixel x0 and in those of pixel x0 + 1
            const uint32_t w_lo = k ? 0u : wy[a] * px[0].w[b];
            const uint32_t w_hi = k ? wy[a] * px[1].w[b] : (same ? wy[a] * px[1].w[b] : 0u);
            const int dy = q.y >> 2, dx = q.x >> 2;
            const uint32_t fy = (uint32_t)(q.y & 3), fx = (uint32_t)(q.x & 3);
            const int iy = y + dy, ix = x0 + dx;   // |q| <= 4 max(H, W) after resolve()
            uint32_t ta = 0, tb = 0, tc = 0, td = 0;   // the four taps of the 4 bytes, a byte each
            bool words = false;
            if (ref_words && iy >= 0 && iy + 1 < H && ix >= 0 && ix + 2 < W) {
                // no tap of x0 or x0 + 1 clamps; the lower tap row's three words end 12 bytes past
                // its first aligned address
                const long long s = (long long)iy * rb + e0 + 3LL * dx;
                if (((s + rb) & ~3LL) + 12 <= (long long)H * rb) {
                    seven_bytes(ref, s, ta, tb);
                    seven_bytes(ref, s + rb, tc, td);
                    words = true;
                }
            }
            if (!words) {
                const uint8_t *r0 = ref + (long long)min(max(iy, 0), H - 1) * rb;
                const uint8_t *r1 = ref + (long long)min(max(iy + 1, 0), H - 1) * rb;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const int x = x0 + (n >= n0), c = (int)e0 + n - 3 * x;
                    const int xa = min(max(x + dx, 0), W - 1) * 3 + c, xb = min(max(x + dx + 1, 0), W - 1) * 3 + c;
                    ta |= (uint32_t)r0[xa] << (8 * n);
                    tb |= (uint32_t)r0[xb] << (8 * n);
                    tc |= (uint32_t)r1[xa] << (8 * n);
                    td |= (uint32_t)r1[xb] << (8 * n);
                }
            }
#pragma unroll
            for (int n = 0; n < 4; ++n)
                acc[n] += (n < n0 ? w_lo : w_hi) * bilinear((ta >> (8 * n)) & 0xFFu, (tb >> (8 * n)) & 0xFFu,
                                                            (tc >> (8 * n)) & 0xFFu, (td >> (8 * n)) & 0xFFu, fx, fy);
        }
    }
    // bytes outside the full-block area kept acc = 0, and 2 bs^2 >> (2 lg + 2) is 0
    uint32_t v = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) v |= ((acc[n] + 2u * bs * bs) >> (2 * lg + 2)) << (8 * n);
    uint8_t *o = out + y * rb + e0;
    if (ne == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t *>(o) = v;
    } else {
        for (int n = 0; n < ne; ++n) o[n] = (uint8_t)(v >> (8 * n));
    }
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_ipp_motion_compensate_obmc(const uint8_t *ref_rgb_dev, const float *mv_dev, int32_t H, int32_t W, int32_t bs,
                                   uint8_t *out_rgb_dev, void *stream)
{
    if (!ref_rgb_dev || !mv_dev || !out_rgb_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(mv_dev, 4);
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad arguments");
    int lg = 2;
    while (lg < 6 && (1 << lg) != bs) ++lg;
    if ((1 << lg) != bs) return set_error(VCF_ERR_INVALID, "block size %d (4, 8, 16, 32 or 64)", bs);
    if (H > 65535) return set_error(VCF_ERR_UNSUPPORTED, "frame height %d (at most 65535 rows)", H);
    const unsigned per_row = (unsigned)(((long long)W * 3 + 3) / 4);
    hipLaunchKernelGGL(ipp_mc_obmc_kernel, dim3((per_row + kThreads - 1) / kThreads, H), dim3(kThreads), 0,
                       (hipStream_t)stream, ref_rgb_dev, mv_dev, H, W, lg, out_rgb_dev, (int)aligned_to(ref_rgb_dev, 4));
    return hip_check(hipGetLastError(), "ipp obmc launch");
}

}  // extern "C"
