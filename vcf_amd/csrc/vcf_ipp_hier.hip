// vcf_ipp_hier.hip -- hierarchical (coarse-to-fine) motion search for the IPP
// loop (--me_levels, not in the reference): a luma pyramid of both frames, the
// full search of vcf_ipp.hip on its top level and a +-1 refinement per finer
// level; vcf_ipp_hier_workspace_bytes and vcf_ipp_block_match_hier of the C
// ABI.  The rule is stated in include/vcf_amd.h ("Hierarchical motion search")
// and restated in numpy by tests/hier_ref.py; everything is integer
// arithmetic, so the GPU and the restatement agree bit for bit.
//
// Launches for levels = L > 0: the two gray passes, L pyramid launches (one
// per level, both frames in it: level l + 1 needs all of level l, and a launch
// boundary is the cheapest grid-wide step; the planes shrink by 4 per level, so
// the later launches are short), the top-level search, one refinement launch
// for all of L - 1 .. 0 (a block's chain touches no other block's vector), and
// the sub-pel refinement of vcf_ipp_subpel.hip when subpel > 1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"

namespace vcf {
namespace {

constexpr int kMaxBs = 64;
constexpr int kMaxSr = 32;
constexpr int kMaxLevels = 3;

// Plane l of the workspace: levels 0 .. L back to back, per level ref's plane then cur's.
__host__ __device__ inline long long level_offset(int H, int W, int l)
{
    long long off = 0;
    for (int k = 0; k < l; ++k) off += 2LL * (H >> k) * (W >> k);
    return off;
}

// 4 output bytes from two rows of 8: per 16-bit half the sums of an even byte, the odd byte after
// it and the two below, + 2, >> 2 (at most 1022 >> 2 = 255: the halves cannot carry into each other)
__device__ __forceinline__ uint32_t halve8(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1)
{
    constexpr uint32_t M = 0x00FF00FFu;
    const uint32_t t0 = (((a0 & M) + ((a0 >> 8) & M) + (b0 & M) + ((b0 >> 8) & M) + 0x00020002u) >> 2) & M;
    const uint32_t t1 = (((a1 & M) + ((a1 >> 8) & M) + (b1 & M) + ((b1 >> 8) & M) + 0x00020002u) >> 2) & M;
    return ((t0 | (t0 >> 8)) & 0xFFFFu) | ((t1 | (t1 >> 8)) << 16);
}

// One pyramid step for both frames (blockIdx.z: 0 ref, 1 cur): the Hs x Ws plane at src halves into
// the (Hs >> 1) x (Ws >> 1) plane at dst; the planes of a level lie back to back.  A lane makes 4
// consecutive bytes of an output row (blockIdx.y, strided) from 8 bytes of each of the two rows above it:
// two words per row where the row's address is 4-byte aligned (the workspace and odd widths may
// leave it anywhere), bytes otherwise and in a row's last, partial group.
__global__ __launch_bounds__(256) void ipp_pyramid_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                          int Hs, int Ws)
{
    const int Hd = Hs >> 1, Wd = Ws >> 1;
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (x0 >= Wd) return;
    const int ne = Wd - x0 < 4 ? Wd - x0 : 4;
    const uint8_t *s = src + (long long)blockIdx.z * Hs * Ws;
    for (int y = blockIdx.y; y < Hd; y += gridDim.y) {
        uint8_t *o = dst + (long long)blockIdx.z * Hd * Wd + (long long)y * Wd + x0;
        const uint8_t *ra = s + (long long)(2 * y) * Ws + 2 * x0, *rb = ra + Ws;
        if (ne == 4) {
            uint32_t a0, a1, b0, b1;
            if (((reinterpret_cast<uintptr_t>(ra) | reinterpret_cast<uintptr_t>(rb)) & 3) == 0) {
                a0 = reinterpret_cast<const uint32_t *>(ra)[0];
                a1 = reinterpret_cast<const uint32_t *>(ra)[1];
                b0 = reinterpret_cast<const uint32_t *>(rb)[0];
                b1 = reinterpret_cast<const uint32_t *>(rb)[1];
            } else {
                a0 = (uint32_t)ra[0] | ((uint32_t)ra[1] << 8) | ((uint32_t)ra[2] << 16) | ((uint32_t)ra[3] << 24);
                a1 = (uint32_t)ra[4] | ((uint32_t)ra[5] << 8) | ((uint32_t)ra[6] << 16) | ((uint32_t)ra[7] << 24);
                b0 = (uint32_t)rb[0] | ((uint32_t)rb[1] << 8) | ((uint32_t)rb[2] << 16) | ((uint32_t)rb[3] << 24);
                b1 = (uint32_t)rb[4] | ((uint32_t)rb[5] << 8) | ((uint32_t)rb[6] << 16) | ((uint32_t)rb[7] << 24);
            }
            const uint32_t v = halve8(a0, a1, b0, b1);
            if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
                *reinterpret_cast<uint32_t *>(o) = v;
            } else {
                for (int n = 0; n < 4; ++n) o[n] = (uint8_t)(v >> (8 * n));
            }
        } else {
            for (int n = 0; n < ne; ++n)
                o[n] = (uint8_t)(((uint32_t)ra[2 * n] + ra[2 * n + 1] + rb[2 * n] + rb[2 * n + 1] + 2u) >> 2);
        }
    }
}

// 9 SADs of at most 64 * 64 * 255 < 2^21 each, three to a 64-bit word: one wave reduction serves three
struct Sad9 {
    unsigned long long p[3];
};

__device__ __forceinline__ Sad9 wave_sum(const uint32_t (&s)[9])
{
    Sad9 r;
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        unsigned long long v = (unsigned long long)s[3 * g] | ((unsigned long long)s[3 * g + 1] << 21) |
                               ((unsigned long long)s[3 * g + 2] << 42);
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        r.p[g] = v;
    }
    return r;
}

__device__ __forceinline__ uint32_t sad_of(const Sad9 &r, int k)   // k = 3 (ddy + 1) + ddx + 1
{
    return (uint32_t)(r.p[k / 3] >> (21 * (k % 3))) & 0x1FFFFFu;
}

// Refinement of the top-level field that mv holds, all levels top - 1 .. 0 in one launch: one wave
// per block.  Per level the block of cur (side b = bs >> l) and the (b + 2)^2 window of ref around
// the centre 2 v sit in LDS; window entries outside the plane are 0 and belong only to invalid
// candidates.  b % 4 == 0: both as words (a window row is b / 4 + 1 words from column rx - 1 on); a
// lane takes words of the block, reads the 6 window words under and beside each and forms the 9
// candidates' words at byte offsets 0, 1, 2 with v_alignbyte for v_sad_u8.  Otherwise bytes, a lane
// per pixel.  The 9 partial sums are reduced packed (wave_sum), and the scan for the first strict
// minimum after the centre is wave-uniform.
__global__ __launch_bounds__(64) void ipp_hier_refine_kernel(const uint8_t *__restrict__ ws, int H, int W, int bs,
                                                             int top, float *__restrict__ mv)
{
    constexpr int kWinWords = (kMaxBs + 2) * (kMaxBs / 4 + 1);
    __shared__ uint32_t cbw[kMaxBs * kMaxBs / 4];
    __shared__ uint32_t winw[kWinWords];
    const int bx = blockIdx.x, by = blockIdx.y, lane = threadIdx.x;
    float *m = mv + ((long long)by * gridDim.x + bx) * 2;
    int vx = (int)m[0], vy = (int)m[1];
    for (int l = top - 1; l >= 0; --l) {
        const int Hl = H >> l, Wl = W >> l, b = bs >> l;
        const uint8_t *ref = ws + level_offset(H, W, l), *cur = ref + (long long)Hl * Wl;
        const int i = by * b, j = bx * b;
        const int cx = 2 * vx, cy = 2 * vy;
        const int ry = i + cy, rx = j + cx;   // the centre's block: inside the plane (vcf_amd.h)
        uint32_t s[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = 0;
        __syncthreads();   // the level before has read its LDS
        if ((b & 3) == 0) {
            const int wq = b >> 2, wp = wq + 1;
            for (int t = lane; t < b * wq; t += 64) {
                const int y = t / wq, q = t - y * wq;
                const uint8_t *p = cur + (long long)(i + y) * Wl + j + 4 * q;
                cbw[t] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            }
            for (int t = lane; t < (b + 2) * wp; t += 64) {
                const int r = t / wp, q = t - r * wp;
                const int y = ry - 1 + r, x = rx - 1 + 4 * q;
                uint32_t v = 0;
                if (y >= 0 && y < Hl) {
                    const uint8_t *p = ref + (long long)y * Wl;
#pragma unroll
                    for (int n = 0; n < 4; ++n)
                        if (x + n >= 0 && x + n < Wl) v |= (uint32_t)p[x + n] << (8 * n);
                }
                winw[t] = v;
            }
            __syncthreads();
            for (int t = lane; t < b * wq; t += 64) {
                const int y = t / wq, q = t - y * wq;
                const uint32_t c = cbw[t];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const uint32_t lo = winw[(y + d) * wp + q], hi = winw[(y + d) * wp + q + 1];
                    s[3 * d] = __builtin_amdgcn_sad_u8(c, lo, s[3 * d]);
                    s[3 * d + 1] = __builtin_amdgcn_sad_u8(c, __builtin_amdgcn_alignbyte(hi, lo, 1u), s[3 * d + 1]);
                    s[3 * d + 2] = __builtin_amdgcn_sad_u8(c, __builtin_amdgcn_alignbyte(hi, lo, 2u), s[3 * d + 2]);
                }
            }
        } else {
            uint8_t *cb = reinterpret_cast<uint8_t *>(cbw), *win = reinterpret_cast<uint8_t *>(winw);
            const int wp = b + 2;
            for (int t = lane; t < b * b; t += 64) cb[t] = cur[(long long)(i + t / b) * Wl + j + t % b];
            for (int t = lane; t < wp * wp; t += 64) {
                const int y = ry - 1 + t / wp, x = rx - 1 + t % wp;
                win[t] = (y >= 0 && y < Hl && x >= 0 && x < Wl) ? ref[(long long)y * Wl + x] : 0;
            }
            __syncthreads();
            for (int t = lane; t < b * b; t += 64) {
                const int y = t / b, x = t - y * b;
                const int c = cb[t];
                const uint8_t *w = win + y * wp + x;
#pragma unroll
                for (int k = 0; k < 9; ++k) s[k] += (uint32_t)abs(c - (int)w[(k / 3) * wp + k % 3]);
            }
        }
        const Sad9 r = wave_sum(s);
        uint32_t best = sad_of(r, 4);   // the centre: index 0 of the (SAD, index) order
        int win_k = 4;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (k == 4) continue;
            const int y = ry + k / 3 - 1, x = rx + k % 3 - 1;
            const bool valid = y >= 0 && y + b <= Hl && x >= 0 && x + b <= Wl;
            const uint32_t sk = sad_of(r, k);
            if (valid && sk < best) {
                best = sk;
                win_k = k;
            }
        }
        vx = cx + win_k % 3 - 1;
        vy = cy + win_k / 3 - 1;
    }
    if (lane == 0) {
        m[0] = (float)vx;
        m[1] = (float)vy;
    }
}

int check_levels(int32_t H, int32_t W, int32_t levels)
{
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad frame shape");
    if (levels < 0 || levels > kMaxLevels) return set_error(VCF_ERR_INVALID, "levels %d (0..%d)", levels, kMaxLevels);
    return VCF_OK;
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_ipp_hier_workspace_bytes(int32_t H, int32_t W, int32_t levels, int64_t *bytes)
{
    if (!bytes) return set_error(VCF_ERR_INVALID, "null pointer");
    const int rc = check_levels(H, W, levels);
    if (rc != VCF_OK) return rc;
    *bytes = level_offset(H, W, levels + 1);
    return VCF_OK;
}

int vcf_ipp_block_match_hier(const uint8_t *ref_rgb_dev, const uint8_t *cur_rgb_dev, int32_t H, int32_t W, int32_t bs,
                             int32_t sr, int32_t levels, int32_t subpel, float *mv_dev, uint8_t *workspace_dev,
                             int64_t workspace_bytes, void *stream)
{
    if (!ref_rgb_dev || !cur_rgb_dev || !mv_dev || !workspace_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(mv_dev, 4);
    int rc = check_levels(H, W, levels);
    if (rc != VCF_OK) return rc;
    if (subpel != 1 && subpel != 2 && subpel != 4)
        return set_error(VCF_ERR_INVALID, "sub-pel precision %d (1, 2 or 4)", subpel);
    if (bs < 1 || bs > kMaxBs) return set_error(VCF_ERR_INVALID, "block size %d (1..%d)", bs, kMaxBs);
    if (sr < 0 || sr > kMaxSr) return set_error(VCF_ERR_INVALID, "search range %d (0..%d)", sr, kMaxSr);
    if (levels > 0 && (bs % (1 << levels) != 0 || (bs >> levels) < 2))
        return set_error(VCF_ERR_INVALID, "block size %d with %d levels: a multiple of %d, at least %d", bs, levels,
                         1 << levels, 2 << levels);
    if (workspace_bytes < level_offset(H, W, levels + 1))
        return set_error(VCF_ERR_INVALID, "workspace of %lld bytes (vcf_ipp_hier_workspace_bytes: %lld)",
                         (long long)workspace_bytes, level_offset(H, W, levels + 1));
    if (levels == 0) {
        rc = ipp_block_match(0, ref_rgb_dev, cur_rgb_dev, H, W, bs, sr, 0, mv_dev, workspace_dev, stream);
        if (rc != VCF_OK || subpel == 1 || W / bs == 0 || H / bs == 0) return rc;
        ipp_subpel_refine(workspace_dev, workspace_dev + (long long)H * W, H, W, bs, subpel, mv_dev, stream);
        return hip_check(hipGetLastError(), "ipp sub-pel refinement launch");
    }
    const int nbx = W / bs, nby = H / bs;
    if (nbx == 0 || nby == 0) return VCF_OK;
    hipStream_t s = (hipStream_t)stream;
    ipp_gray_planes(ref_rgb_dev, cur_rgb_dev, H, W, workspace_dev, stream);
    for (int l = 0; l < levels; ++l) {
        const int Hs = H >> l, Ws = W >> l, Hd = Hs >> 1, Wd = Ws >> 1;
        const unsigned per_row = (unsigned)((Wd + 3) / 4);
        hipLaunchKernelGGL(ipp_pyramid_kernel, dim3((per_row + 255) / 256, Hd < 65535 ? Hd : 65535, 2), dim3(256), 0, s,
                           workspace_dev + level_offset(H, W, l), workspace_dev + level_offset(H, W, l + 1), Hs, Ws);
    }
    // the top level: the field has (H >> L) / (bs >> L) = H / bs rows, and columns alike
    const int Ht = H >> levels, Wt = W >> levels;
    const uint8_t *top = workspace_dev + level_offset(H, W, levels);
    ipp_plane_search(0, top, top + (long long)Ht * Wt, Ht, Wt, bs >> levels, sr, 0, mv_dev, stream);
    hipLaunchKernelGGL(ipp_hier_refine_kernel, dim3(nbx, nby), dim3(64), 0, s, workspace_dev, H, W, bs, levels, mv_dev);
    if (subpel > 1)
        ipp_subpel_refine(workspace_dev, workspace_dev + (long long)H * W, H, W, bs, subpel, mv_dev, stream);
    return hip_check(hipGetLastError(), "ipp hierarchical block match launch");
}

}  // extern "C"
