// vcf_dct_tile.h -- the memory side of the fused 8x8 encode kernels: the frame geometry, a
// workgroup's tile of kTile blocks, the input loads and the copy-out of the LDS image of the
// output.  Shared by the translation units that have such a kernel (vcf_dct_dz.hip: deadzone
// encode and the decode's staging; vcf_dct_rdoq.hip: the rate-distortion optimised encode), each
// of which gets its own copy (everything here is inline or a template).  The per-block arithmetic
// is vcf_dct_block.h; DESIGN.md §3 has the layout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vcf_internal.h"

namespace vcf {
namespace dct_tile {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kTile = 256;                   // blocks (= lanes) per workgroup; a full tile's (i, j)
                                             // subband run is kTile * 3 bytes, its LDS image 48 KiB

struct Geom {
    int H, W, Hp, Wp, top, left, nbx, nby, tiles_per_row;
    int nblocks, tiles_per_frame;      // raster tiles: kTile consecutive blocks of a frame
    long long in_stride, out_stride;   // bytes per frame (RGB, coefficients)
    int vec;                           // 16-B path valid for the coefficient frames
};

// Raster tiles (encode variants 1/4, decode): a tile is kTile consecutive
// blocks of a frame in raster order and may wrap into the next block rows, so
// only a frame's last tile is partial.  Each lane publishes where its block's
// bytes start in the frame (`rowbase`: (by*Wp + bx)*3, or (by*8*Wp + bx*8)*3
// for -x); output run `seg` of the LDS image then maps to rowbase[block] +
// segment base.  With nbx % 16 == 0 block-row ends fall on 16-block
// boundaries of the tile, so a 16-byte chunk never straddles one.
__device__ __forceinline__ void tile_block(const Geom &g, int n, int &by, int &bx)
{
    by = n / g.nbx;
    bx = n - by * g.nbx;
}

template <bool SUB>
__device__ __forceinline__ uint32_t block_rowbase(const Geom &g, int by, int bx)
{
    return SUB ? ((uint32_t)by * (uint32_t)g.Wp + (uint32_t)bx) * 3u
               : ((uint32_t)by * 8u * (uint32_t)g.Wp + (uint32_t)bx * 8u) * 3u;
}

template <bool SUB>
__device__ __forceinline__ uint32_t seg_base(const Geom &g, int seg)
{
    if (!SUB) return (uint32_t)seg * (uint32_t)g.Wp * 3u;
    const uint32_t i = seg >> 3, j = seg & 7;
    return (i * (uint32_t)g.nby * (uint32_t)g.Wp + j * (uint32_t)g.nbx) * 3u;
}

template <bool SUB, bool TO_GLOBAL, int T = kTile>
__device__ __forceinline__ void move_runs_tab(const Geom &g, uint8_t *stage, const uint32_t *rowbase,
                                              uint8_t *frame, int nvalid)
{
    constexpr int nseg = SUB ? 64 : 8;
    constexpr int bpb = SUB ? 3 : 24;                  // bytes per block in a run
    constexpr int lds_stride = SUB ? T * 3 : T * 24;
    const int tid = threadIdx.x;
    if (g.vec) {
        const int cps = (nvalid * bpb) >> 4;           // nvalid is a multiple of 16
        // stage bytes are the low bytes of k: XOR 0x80 == +128 mod 256 (2D-DCT.py:348,361)
        const int total = nseg * cps;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int q = tid; q < total; q += T) {
            const int seg = q / cps;
            const int off = (q - seg * cps) << 4;
            const int blk = off / bpb;
            const uint32_t go = rowbase[blk] + seg_base<SUB>(g, seg) + (uint32_t)(off - blk * bpb);
            u32x4 *lp = reinterpret_cast<u32x4 *>(stage + seg * lds_stride + off);
            u32x4 *gp = reinterpret_cast<u32x4 *>(frame + go);
            if (TO_GLOBAL) __builtin_nontemporal_store(*lp ^ 0x80808080u, gp);   // k -> k + 128
            else *lp = __builtin_nontemporal_load(gp);
        }
    } else {
        const int seg_len = nvalid * bpb, total = nseg * seg_len;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int q = tid; q < total; q += T) {
            const int seg = q / seg_len;
            const int off = q - seg * seg_len;
            const int blk = off / bpb;
            const uint32_t go = rowbase[blk] + seg_base<SUB>(g, seg) + (uint32_t)(off - blk * bpb);
            if (TO_GLOBAL) frame[go] = stage[seg * lds_stride + off] ^ 0x80;
            else stage[seg * lds_stride + off] = frame[go];
        }
    }
}

// Copy-out of a full tile (nvalid == kTile, g.vec): compile-time chunk
// geometry (12 16-byte chunks per lane), every LDS read issued before the
// stores -- the generic loop above waits on each read in turn (4-5 % of the
// encode).  Plain stores, so the 128-byte lines a tile shares
// with its neighbours at run joins stay in the XCD's L2 until the neighbour's
// half arrives (the tile order keeps neighbours on one XCD, see
// dct_dz_encode_kernel); non-temporal stores wrote those lines twice, half at
// a time (2 % slower).  The chunk -> (run, offset, block) divisions are 24-bit
// multiply-shifts and the run bases come from two per-launch constants
// (full-rate v_mul_u32_u24 instead of quarter-rate 32-bit multiplies and
// 64-bit address arithmetic) whenever the frame's subband stride fits 24 bits.
// multiply-shift division q / cps for q < 64 cps (tiles of T = 256 blocks; 384- and
// 512-block tiles, m/s = 3641/18 and 2731/18, measured slower: DESIGN.md §6)
template <int T>
struct DivCps;
template <>
struct DivCps<256> { static constexpr uint32_t m = 2731, s = 17; };   // / 48

template <bool SUB, int T = kTile>
__device__ __forceinline__ void move_runs_full(const Geom &g, const uint8_t *stage, const uint32_t *rowbase,
                                               uint8_t *frame)
{
    constexpr int nseg = SUB ? 64 : 8;
    constexpr int bpb = SUB ? 3 : 24;
    constexpr int lds_stride = SUB ? T * 3 : T * 24;
    constexpr int cps = (T * bpb) >> 4;
    constexpr int per_lane = nseg * cps / T;
    static_assert(nseg * cps % T == 0, "whole stores per lane");
    const int tid = threadIdx.x;
    u32x4 v[per_lane];
    uint32_t go[per_lane];
    const uint32_t segA = (uint32_t)g.nby * (uint32_t)g.Wp * 3u, segB = (uint32_t)g.nbx * 3u;
    if (SUB && segA < (1u << 24)) {
        static_assert(!SUB || bpb == 3, "multiply-shift constants");
#pragma unroll
        for (int r = 0; r < per_lane; ++r) {
            const int q = tid + r * T;                                                  // < 64 cps
            const int seg = (int)(__umul24((uint32_t)q, DivCps<T>::m) >> DivCps<T>::s);   // q / cps
            const int off = (q - seg * cps) << 4;                                       // < 3 T
            const int blk = (int)(__umul24((uint32_t)off, 683u) >> 11);                 // off / 3
            go[r] = rowbase[blk] + __umul24((uint32_t)(seg >> 3), segA) + __umul24((uint32_t)(seg & 7), segB) +
                    (uint32_t)(off - blk * bpb);
            v[r] = *reinterpret_cast<const u32x4 *>(stage + seg * lds_stride + off);
        }
    } else {
#pragma unroll
        for (int r = 0; r < per_lane; ++r) {
            const int q = tid + r * T;
            const int seg = q / cps;
            const int off = (q - seg * cps) << 4;
            const int blk = off / bpb;
            go[r] = rowbase[blk] + seg_base<SUB>(g, seg) + (uint32_t)(off - blk * bpb);
            v[r] = *reinterpret_cast<const u32x4 *>(stage + seg * lds_stride + off);
        }
    }
#pragma unroll
    for (int r = 0; r < per_lane; ++r) *reinterpret_cast<u32x4 *>(frame + go[r]) = v[r] ^ 0x80808080u;   // k + 128
}

// Make raw[] look redefined *after* `dep` exists, so a channel's byte
// extractions can neither be CSE'd with the previous channel's nor hoisted
// above it (either keeps 2-3 channels' inputs live at once and spills).
__device__ __forceinline__ void opaque(uint32_t (&raw)[8][6], uint32_t dep)
{
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int w = 0; w < 6; ++w) asm volatile("" : "+v"(raw[y][w]) : "v"(dep));
}

// The 192 bytes of block (by, bx), row y in raw[y][0..5] (little-endian);
// the padding (2D-DCT.py:187-229) reads as zero bytes like the reference's.
// Plain loads (non-temporal ones measured 2.7 % slower); the
// compiler merges each row's three 8-byte loads into one 16-byte and one
// 8-byte load.
template <bool PAD>
__device__ __forceinline__ void load_block(const Geom &g, const uint8_t *src, int by, int bx,
                                           uint32_t (&raw)[8][6])
{
    if (!PAD) {
        // one 64-bit block address, the rows at uniform (scalar) offsets y * 3W
        const uint8_t *blk = src + ((long long)by * 8 * g.W + bx * 8) * 3;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const u32x2 *p = reinterpret_cast<const u32x2 *>(blk + (long long)y * (3LL * g.W));
            const u32x2 a = p[0], b = p[1], c = p[2];
            raw[y][0] = a.x; raw[y][1] = a.y; raw[y][2] = b.x;
            raw[y][3] = b.y; raw[y][4] = c.x; raw[y][5] = c.y;
        }
    } else {
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const int sy = by * 8 + y - g.top;
#pragma unroll
            for (int w = 0; w < 6; ++w) raw[y][w] = 0;
#pragma unroll
            for (int n = 0; n < 24; ++n) {
                const int sx = bx * 8 + n / 3 - g.left;
                uint32_t b = 0;
                if (sy >= 0 && sy < g.H && sx >= 0 && sx < g.W)
                    b = src[((long long)sy * g.W + sx) * 3 + n % 3];
                raw[y][n >> 2] |= b << ((n & 3) * 8);
            }
        }
    }
}

// A wave's own part of rows 2..7 of the LDS image, zeroed with 16-byte
// writes.  The 64 blocks of wave w own bytes [192 w, 192 w + 192) of each of
// the 48 subband runs (i, j), i >= 2 -- 12 chunks per run, written by lanes
// (run & 3, chunk) = (lane >> 4, lane & 15 < 12), 12 runs each -- or, for -x,
// bytes [1536 w, 1536 w + 1536) of each of the 6 pixel rows i >= 2: 96 chunks
// per row, lanes 0..63 and again lanes 0..31.  Every offset after the lane's
// base is a compile-time constant.  Only the wave itself writes these bytes
// afterwards (its blocks' index bytes), and a wave's LDS operations execute in
// order, so a wave-level fence for the compiler is all that orders the two --
// no workgroup barrier.
template <bool SUB, int T>
__device__ __forceinline__ void zero_wave_rows(uint8_t *stage, int tid)
{
    const int w = tid >> 6, l = tid & 63;
    const u32x4 z = {0u, 0u, 0u, 0u};
    if (SUB) {
        if ((l & 15) < 12) {
            uint8_t *p = stage + (16 + (l >> 4)) * (T * 3) + w * 192 + (l & 15) * 16;
#pragma unroll
            for (int r = 0; r < 12; ++r) *reinterpret_cast<u32x4 *>(p + r * 4 * (T * 3)) = z;
        }
    } else {
        uint8_t *p = stage + 2 * (T * 24) + w * 1536 + l * 16;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            *reinterpret_cast<u32x4 *>(p + i * (T * 24)) = z;
            if (l < 32) *reinterpret_cast<u32x4 *>(p + i * (T * 24) + 1024) = z;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The tile a workgroup takes and the frame it lies in.  Each XCD takes a contiguous range of
// tiles (workgroups are dealt round robin), so neighbouring tiles -- which share partial lines at
// run joins -- meet in one L2.  grid = (tiles per frame, frames).
__device__ __forceinline__ void tile_of_workgroup(long long &frame, int &tile)
{
    const unsigned n = gridDim.x * gridDim.y, gid = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned q = n >> 3, r = n & 7, xcd = gid & 7;
    const unsigned t = xcd * q + min(xcd, r) + (gid >> 3);
    frame = t / gridDim.x;
    tile = (int)(t - (unsigned)frame * gridDim.x);
}

// k_dev = the call's coefficient frames: the 16-byte copies of move_runs_tab / move_runs_full and of
// the decode's staging loop run at k_dev + multiples of 16, so they also need the pointer's low
// four bits clear.  An aligned pointer leaves every field as the shape alone gives it.
inline void make_geom(int32_t H, int32_t W, const uint8_t *k_dev, Geom &g)
{
    g.H = H;
    g.W = W;
    g.Hp = (H + 7) / 8 * 8;
    g.Wp = (W + 7) / 8 * 8;
    g.top = (g.Hp - H) / 2;
    g.left = (g.Wp - W) / 2;
    g.nbx = g.Wp / 8;
    g.nby = g.Hp / 8;
    g.tiles_per_row = (g.nbx + kTile - 1) / kTile;
    g.nblocks = g.nbx * g.nby;
    g.tiles_per_frame = (g.nblocks + kTile - 1) / kTile;
    g.in_stride = (long long)H * W * 3;
    g.out_stride = (long long)g.Hp * g.Wp * 3;
    // every subband run starts 16-B aligned and spans whole 16-B chunks iff
    // nbx % 16 == 0 (then Wp*3, nbx*3, 768 and the frame size are multiples of 16)
    g.vec = (g.nbx % 16 == 0 && aligned_to(k_dev, 16)) ? 1 : 0;
}

// The PAD = false instantiations move a block row's 24 RGB bytes as three 8-byte words
// (load_block, the decode epilogues); an RGB pointer off 8 bytes takes the PAD = true ones, whose
// byte loads and stores are as valid with top = left = 0.
inline bool rgb_needs_bytes(const Geom &g, const uint8_t *rgb_dev)
{
    return g.Hp != g.H || g.Wp != g.W || !aligned_to(rgb_dev, 8);
}

}  // namespace dct_tile
}  // namespace vcf
