// vcf_block_tile.h -- what the block-transform codecs with a dense D x D matrix (2D-KLT,
// vcf_klt_dz.hip; 2D-LBT, vcf_lbt.hip) share around their products: the frame's cut into
// blocks, the workgroup tiles and their LDS, the index maps between a tile, the coefficient
// frame and the pixels, the loops that move a tile with them, and the second-moment tiling
// (which vcf_klt_dz.hip restates for its own kernel).
//
// A frame is cut into N blocks of B x B samples (D = B * B values per block, raster order of
// blocks, row-major inside a block) after a centred zero pad.  A workgroup of encode or
// decode owns TB consecutive blocks: the staged samples (or indices) of a channel in LDS,
// one row of stage_stride(D) elements per block, and behind them the bytes of all three
// channels, one row of out_stride(D) bytes per block, which leave in contiguous runs.
//
// The geometry, the plan and the index maps are host+device, so that tests/cpu compiles
// exactly this code with g++ and walks every tile on a CPU-only machine; the loops and the
// moments tiling are device code.  Everything is inline: two translation units include it.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "vcf_dct8.h"   // VCF_HD

namespace vcf {

constexpr int kTileThreads = 512;   // encode / decode
constexpr int kMomThreads = 256;    // moments
constexpr int kMomChunk = 2048;     // blocks per workgroup: 2048 * 512 * 512 = 2^29 fits int32
constexpr int kMomLds = 16384;      // int16 values of one staged tile
constexpr int kBlockLds[3] = {48 * 1024, 80 * 1024, 156 * 1024};   // 3, 2, 1 workgroups per CU (160 KiB LDS)

struct BlockGeom {
    int H, W, Hp, Wp, top, left;
    int B, D;
    int nbx, nby, N;    // blocks per row / column / frame (and channel)
    int TB;             // blocks per workgroup tile (encode, decode)
    long long rgb_stride, k_stride;
};

// the kernels address within a frame, padded or not, with 32-bit arithmetic
VCF_HD bool frame_fits_int32(int32_t H, int32_t W, int32_t B)
{
    return ((long long)H + B) * ((long long)W + B) * 3 < (1LL << 31);
}

VCF_HD BlockGeom make_block_geom(int32_t H, int32_t W, int32_t B)
{
    BlockGeom g;
    g.H = H;
    g.W = W;
    g.B = B;
    g.D = B * B;
    g.Hp = (H + B - 1) / B * B;
    g.Wp = (W + B - 1) / B * B;
    g.top = (g.Hp - H) / 2;
    g.left = (g.Wp - W) / 2;
    g.nbx = g.Wp / B;
    g.nby = g.Hp / B;
    g.N = g.nbx * g.nby;
    // a tile of about 8192 values (16384 where a block alone has more than 128), whole waves of blocks
    const int budget = g.D > 128 ? 16384 : 8192;
    const int tb = budget / g.D / 64 * 64;
    g.TB = tb < 64 ? 64 : (tb > 1024 ? 1024 : tb);
    g.rgb_stride = (long long)H * W * 3;
    g.k_stride = (long long)g.Hp * g.Wp * 3;
    return g;
}

VCF_HD int align16(int x) { return (x + 15) & ~15; }
VCF_HD int stage_stride(int D) { return D | 1; }      // odd row stride of the staged tile, in elements
VCF_HD int out_stride(int D) { return D * 3 + 4; }    // row stride of the collected bytes
// one channel's staged tile, elements of elem_bytes (2: int16, 4: float)
VCF_HD int stage_bytes(const BlockGeom &g, int elem_bytes) { return align16(g.TB * stage_stride(g.D) * elem_bytes); }
VCF_HD int enc_lds_bytes(const BlockGeom &g, int elem_bytes) { return stage_bytes(g, elem_bytes) + g.TB * out_stride(g.D); }
// decode stages the int16 indices of all three channels
VCF_HD int dec_lds_bytes(const BlockGeom &g) { return 3 * stage_bytes(g, 2) + g.TB * out_stride(g.D); }

VCF_HD int lds_class(int bytes)
{
    for (int c = 0; c < 3; ++c)
        if (bytes <= kBlockLds[c]) return c;
    return -1;
}

// f(std::integral_constant<int, kBlockLds[cls]>()): the kernels take their LDS size as a template argument
template <typename F>
void with_lds_class(int cls, F f)
{
    if (cls == 0) f(std::integral_constant<int, kBlockLds[0]>());
    else if (cls == 1) f(std::integral_constant<int, kBlockLds[1]>());
    else f(std::integral_constant<int, kBlockLds[2]>());
}

// What the launches use, and what vcf_lbt_tile_plan reports: the encode (or decode) grid and LDS
// class, and the moments kernel's chunks per frame and blocks per staged tile.
struct BlockPlan {
    int cls;       // index into kBlockLds, -1: the tile does not fit
    int tiles;     // encode / decode workgroups per frame
    int nt, T;     // moments: 8-wide coefficient groups, and their upper-triangle pairs
    int chunks;    // moments: workgroups per frame and channel
    int tbm;       // moments: blocks staged in LDS at a time
};

VCF_HD BlockPlan make_block_plan(const BlockGeom &g, bool decode, int elem_bytes)
{
    BlockPlan p;
    p.cls = lds_class(decode ? dec_lds_bytes(g) : enc_lds_bytes(g, elem_bytes));
    p.tiles = (g.N + g.TB - 1) / g.TB;
    p.nt = (g.D + 7) / 8;
    p.T = p.nt * (p.nt + 1) / 2;
    p.chunks = (g.N + kMomChunk - 1) / kMomChunk;
    const int tbm = kMomLds / (p.nt * 8);
    p.tbm = tbm < kMomChunk ? tbm : kMomChunk;
    return p;
}

// ---------------------------------------------------------------------------
// index maps
// ---------------------------------------------------------------------------
VCF_HD void block_yx(const BlockGeom &g, int b, int &by, int &bx)
{
    by = b / g.nbx;
    bx = b - by * g.nbx;
}

// Coefficient k of block b in the padded coefficient frame, in pixels (3 bytes each).  Subband
// layout: subband (ky, kx) holds coefficient (ky, kx) of every block, runs of 3 bytes per block;
// block layout: coefficient (ky, kx) of block (by, bx) at (by B + ky, bx B + kx), runs of 3 B bytes.
VCF_HD long long coef_pos(const BlockGeom &g, int b, int k, int sub)
{
    int by, bx;
    block_yx(g, b, by, bx);
    const int ky = k / g.B, kx = k - ky * g.B;
    return sub ? ((long long)(ky * g.nby + by) * g.Wp + kx * g.nbx + bx)
               : ((long long)(by * g.B + ky) * g.Wp + bx * g.B + kx);
}

// Element e of a tile's 3 D tbv bytes as (block in the tile, coefficient or sample, channel), in
// the two orders the kernels walk them: a block's bytes together, or a coefficient's (the
// subbands' runs; tbv: blocks in this tile).
VCF_HD void elem_by_block(int D, int e, int &bl, int &k, int &c)
{
    bl = e / (D * 3);
    const int q = e - bl * (D * 3);
    k = q / 3;
    c = q - k * 3;
}

VCF_HD void elem_by_coef(int tbv, int e, int &bl, int &k, int &c)
{
    c = e % 3;
    const int t = e / 3;
    k = t / tbv;
    bl = t - k * tbv;
}

// Sample j of block b as (y, x) of the cropped frame; outside it (in_frame) the sample lies in the
// pad.
VCF_HD void pixel_yx(const BlockGeom &g, int b, int j, int &y, int &x)
{
    int by, bx;
    block_yx(g, b, by, bx);
    const int ky = j / g.B, kx = j - ky * g.B;
    y = by * g.B + ky - g.top;
    x = bx * g.B + kx - g.left;
}

VCF_HD bool in_frame(const BlockGeom &g, int y, int x) { return y >= 0 && y < g.H && x >= 0 && x < g.W; }

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------
// device: a tile's way in and out.  b0: the tile's first block, tbv: its blocks.
// ---------------------------------------------------------------------------
// s = 4 x of channel c at padded position (py, px): zero pad, -128, YCoCg
__device__ __forceinline__ int sample4(const uint8_t *__restrict__ src, const BlockGeom &g, int py, int px, int c)
{
    const int y = py - g.top, x = px - g.left;
    int R = -128, G = -128, Bl = -128;
    if (y >= 0 && y < g.H && x >= 0 && x < g.W) {
        const uint8_t *p = src + ((long long)y * g.W + x) * 3;
        R += p[0];
        G += p[1];
        Bl += p[2];
    }
    return c == 0 ? R + 2 * G + Bl : (c == 1 ? 2 * R - 2 * Bl : 2 * G - R - Bl);
}

// X[bl][d] = conv(s) of channel c
template <typename T, typename Conv>
__device__ __forceinline__ void stage_samples(const uint8_t *__restrict__ src, T *X, const BlockGeom &g, int b0, int tbv,
                                              int c, Conv conv)
{
    const int D = g.D, B = g.B, XS = stage_stride(D);
    for (int e = threadIdx.x; e < tbv * D; e += kTileThreads) {
        const int bl = e / D, d = e - bl * D;
        int by, bx;
        block_yx(g, b0 + bl, by, bx);
        const int ky = d / B, kx = d - ky * B;
        X[bl * XS + d] = conv(sample4(src, g, by * B + ky, bx * B + kx, c));
    }
}

// the collected index bytes O[bl][k][c] -> the coefficient frame
__device__ __forceinline__ void scatter_indices(const uint8_t *O, uint8_t *__restrict__ dst, const BlockGeom &g, int b0,
                                                int tbv, int sub)
{
    const int D = g.D, OS = out_stride(D), total = tbv * D * 3;
    int bl, k, c;
    if (!sub) {
        for (int e = threadIdx.x; e < total; e += kTileThreads) {
            elem_by_block(D, e, bl, k, c);
            dst[coef_pos(g, b0 + bl, k, 0) * 3 + c] = O[bl * OS + k * 3 + c];
        }
    } else {
        for (int e = threadIdx.x; e < total; e += kTileThreads) {
            elem_by_coef(tbv, e, bl, k, c);
            dst[coef_pos(g, b0 + bl, k, 1) * 3 + c] = O[bl * OS + k * 3 + c];
        }
    }
}

// the coefficient frame -> Y[c][bl][k] = post(Q (u8 - 128) as int16 (wrapping), c, k); ys: one
// channel's tile, in elements.  This loop and crop_pixels spell out elem_by_coef, elem_by_block,
// coef_pos, pixel_yx and in_frame, take no __restrict__ pointers, and this one takes the geometry by
// value: so written the decode kernels compile to the instructions they had before the loops were
// shared (klt_decode_kernel exactly).  Composed from the map functions they compile to the same
// number of instructions in another order, and both decodes measured 0.2 to 0.3 % slower.  The maps
// above remain the definition that tests/test_block_tile.py checks; keep these two loops equal to them.
template <typename Post>
__device__ __forceinline__ void gather_indices(const uint8_t *src, short *Y, int ys, const BlockGeom g,
                                               int b0, int tbv, int sub, int Q, Post post)
{
    const int D = g.D, B = g.B, XS = stage_stride(D);
    for (int e = threadIdx.x; e < tbv * D * 3; e += kTileThreads) {
        int c, bl, k;
        if (sub) {
            c = e % 3;
            const int t = e / 3;
            k = t / tbv;
            bl = t - k * tbv;
        } else {
            bl = e / (D * 3);
            const int q = e - bl * (D * 3);
            k = q / 3;
            c = q - k * 3;
        }
        const int ky = k / B, kx = k - ky * B;
        const int b = b0 + bl, by = b / g.nbx, bx = b - by * g.nbx;
        const long long at = sub ? ((long long)(ky * g.nby + by) * g.Wp + kx * g.nbx + bx)
                                 : ((long long)(by * B + ky) * g.Wp + bx * B + kx);
        Y[c * ys + bl * XS + k] = post((short)(Q * ((int)src[at * 3 + c] - 128)), c, k);
    }
}

// the collected pixel bytes O[bl][j][c] -> the frame, cropped: runs of 3 B bytes
__device__ __forceinline__ void crop_pixels(const uint8_t *O, uint8_t *dst, const BlockGeom &g, int b0, int tbv)
{
    const int D = g.D, B = g.B, OS = out_stride(D);
    for (int e = threadIdx.x; e < tbv * D * 3; e += kTileThreads) {
        const int bl = e / (D * 3), q = e - bl * (D * 3);
        const int j = q / 3, ky = j / B, kx = j - ky * B;
        const int b = b0 + bl, by = b / g.nbx, bx = b - by * g.nbx;
        const int y = by * B + ky - g.top, x = bx * B + kx - g.left;
        if (y < 0 || y >= g.H || x < 0 || x >= g.W) continue;
        dst[((long long)y * g.W + x) * 3 + (q - j * 3)] = O[bl * OS + q];
    }
}

// ---------------------------------------------------------------------------
// device: second moments.  S1 += sum s, S2 += sum s s^T over the blocks of chunk `chunk` of
// channel c, s = 4 x: integers with |s| <= 512, so the int32 partial sums over at most kMomChunk
// blocks are exact.  A thread owns an 8 x 8 tile of the upper triangle of S2 (and mirrors it on
// the way out); where D is small the spare threads split the blocks of a staged tile.  The
// partial sums join s1[D] and s2[D][D] (zeroed by the caller) through atomics as term(v, first):
// what the int32 partial v adds to a sum of type S, first = true for S1.  lbt_moments_kernel runs
// it; klt_moments_kernel keeps the same tiling in its own file (see there).
// ---------------------------------------------------------------------------
template <typename S, typename Term>
__device__ __forceinline__ void moments_tiles(const uint8_t *__restrict__ src, S *s1, S *s2, const BlockGeom &g, int nt,
                                              int T, int tbm, int chunk, int c, Term term)
{
    __shared__ __attribute__((aligned(16))) short X[kMomLds];
    const int D = g.D, B = g.B, DP = nt * 8;
    const int tid = threadIdx.x;
    const int b_lo = chunk * kMomChunk, b_hi = min(g.N, b_lo + kMomChunk);
    const int tpp = min(T, kMomThreads), Z = kMomThreads / tpp;   // tiles per pass, block slices
    const int tl = tid % tpp, z = tid / tpp;

    for (int p0 = 0; p0 < T; p0 += tpp) {
        const int t = p0 + tl;
        const bool active = t < T && z < Z;
        // tile t of the upper triangle, row-major: (ti, tj), ti <= tj
        int ti = 0, rem = min(t, T - 1);
        while (rem >= nt - ti) {
            rem -= nt - ti;
            ++ti;
        }
        const int tj = ti + rem;
        int acc[8][8], a1[8];
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            a1[a] = 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) acc[a][b] = 0;
        }
        for (int t0 = b_lo; t0 < b_hi; t0 += tbm) {
            const int nb = min(tbm, b_hi - t0);
            __syncthreads();
            for (int e = tid; e < nb * DP; e += kMomThreads) {
                const int bl = e / DP, d = e - bl * DP;
                int v = 0;
                if (d < D) {
                    int by, bx;
                    block_yx(g, t0 + bl, by, bx);
                    const int ky = d / B, kx = d - ky * B;
                    v = sample4(src, g, by * B + ky, bx * B + kx, c);
                }
                X[e] = (short)v;
            }
            __syncthreads();
            if (active) {
                // kept scalar: vectorised over pairs of blocks it costs 35 VGPRs and a wave per SIMD
#pragma clang loop vectorize(disable)
                for (int bl = z; bl < nb; bl += Z) {
                    const short *r = X + bl * DP;
                    int si[8], sj[8];
#pragma unroll
                    for (int a = 0; a < 8; ++a) {
                        si[a] = r[ti * 8 + a];
                        sj[a] = r[tj * 8 + a];
                    }
#pragma unroll
                    for (int a = 0; a < 8; ++a) {
                        a1[a] += si[a];
#pragma unroll
                        for (int b = 0; b < 8; ++b) acc[a][b] += si[a] * sj[b];
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int a = 0; a < 8; ++a) {
                const int i = ti * 8 + a;
                if (i >= D) continue;
                if (ti == tj) atomicAdd(s1 + i, term(a1[a], true));
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const int j = tj * 8 + b;
                    if (j >= D) continue;
                    const S v = term(acc[a][b], false);
                    atomicAdd(s2 + (long long)i * D + j, v);
                    if (ti != tj) atomicAdd(s2 + (long long)j * D + i, v);
                }
            }
        }
    }
}
#endif  // __HIPCC__

}  // namespace vcf
