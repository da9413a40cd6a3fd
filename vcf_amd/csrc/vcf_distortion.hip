// vcf_distortion.hip -- what src/RDE.py measures between an original and a decoded image, as
// exact integers per frame and channel: the sum of squared differences, the sum of absolute
// differences and the largest absolute difference of two sets of u8 frames.  The arithmetic is
// stated in include/vcf_amd.h (vcf_distortion_u8).
//
// The kernel streams two bytes per sample and stores nothing but its sums, so its time is the
// HBM read of both frame sets.  A lane takes spans of kSpan = 48 bytes, three 16-byte loads from
// each frame: 48 is a multiple of lcm(16, C) for every C of 1..4, so byte j of every span belongs
// to the same channel class j % C, a compile-time constant, and the per-channel sums need no
// division and no per-byte branch.  Spans start at the first 16-byte boundary of frame a (frames
// of H*W*C bytes need not be multiples of 16); the `head` bytes in front of it and the tail of
// less than one span behind the last one are read by byte loads, so nothing is read outside a
// frame.  Class i is channel (head + i) % C; that rotation happens once, at the atomics.
//
// Per dword pair: the four absolute differences in two packed 16-bit halves (even and odd bytes;
// v_pk_max/min/sub_u16), recombined to four packed bytes d; then per channel class with a byte in
// that dword, dm = d & mask, v_sad_u8(dm, 0) for the absolute sum and v_dot4_u32_u8(d, dm) for
// the squares; the largest difference is a running v_pk_max_u16 of the halves.  A lane's 32-bit
// sums cover one tile (kUnroll spans: at most 96 samples of 255^2 a class) and are then added to
// its 64-bit sums, far below the 66 051 samples at which 32 bits would overflow.  Wave reduction
// by shuffles, the four waves through LDS, then three 64-bit atomics per workgroup and channel:
// add for the two sums, max for {max_abs, pad} read as one word.  Integer sums and maxima do not
// depend on the order of the atomics nor on the grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"

namespace {

using vcf::hip_check;
using vcf::set_error;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSpan = 48;                          // bytes per lane and step
constexpr int kUnroll = 2;                         // spans per lane and tile: 12 16-byte loads in flight
constexpr int kTileSpans = kThreads * kUnroll;     // a workgroup's share per step: 24 576 bytes
constexpr int kTargetBlocks = 2048;                // 256 CUs x 8 workgroups

static_assert(sizeof(vcf_distortion_record) == 24, "record layout is part of the ABI");
static_assert(kSpan % 16 == 0 && kSpan % 3 == 0 && kSpan % 4 == 0, "kSpan must be a multiple of lcm(16, C)");

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// mask of the bytes of dword j of a span whose class (byte offset % C) is c
template <int C>
__device__ __forceinline__ constexpr uint32_t class_mask(int j, int c)
{
    uint32_t m = 0;
    for (int k = 0; k < 4; ++k)
        if ((4 * j + k) % C == c) m |= 0xFFu << (8 * k);
    return m;
}

// dwords after which the byte classes of a dword repeat: lcm(4, C) / 4
template <int C> constexpr int kPeriod = C == 3 ? 3 : 1;

template <int C>
struct Sums {
    uint32_t sse[C], sad[C];
};

// One dword of a and of b (dword j of a span) into the tile's 32-bit sums and the running maxima.
template <int C>
__device__ __forceinline__ void add_dword(int j, uint32_t a, uint32_t b, Sums<C> &t, us2 (&me)[kPeriod<C>],
                                          us2 (&mo)[kPeriod<C>])
{
    const us2 ae = __builtin_bit_cast(us2, a & 0x00FF00FFu), be = __builtin_bit_cast(us2, b & 0x00FF00FFu);
    const us2 ao = __builtin_bit_cast(us2, (a >> 8) & 0x00FF00FFu), bo = __builtin_bit_cast(us2, (b >> 8) & 0x00FF00FFu);
    const us2 de = __builtin_elementwise_max(ae, be) - __builtin_elementwise_min(ae, be);
    const us2 dd = __builtin_elementwise_max(ao, bo) - __builtin_elementwise_min(ao, bo);
    me[j % kPeriod<C>] = __builtin_elementwise_max(me[j % kPeriod<C>], de);
    mo[j % kPeriod<C>] = __builtin_elementwise_max(mo[j % kPeriod<C>], dd);
    const uint32_t d = __builtin_bit_cast(uint32_t, de) | (__builtin_bit_cast(uint32_t, dd) << 8);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const uint32_t m = class_mask<C>(j, c);
        if (m == 0) continue;
        const uint32_t dm = d & m;
        t.sad[c] = __builtin_amdgcn_sad_u8(dm, 0u, t.sad[c]);
        t.sse[c] = __builtin_amdgcn_udot4(d, dm, t.sse[c], false);
    }
}

// 16 bytes of a frame: one load where the address is 16-byte aligned, byte loads otherwise
template <bool kAligned>
__device__ __forceinline__ uint4 load16(const uint8_t *p)
{
    if constexpr (kAligned) {
        return *reinterpret_cast<const uint4 *>(p);
    } else {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) |
                   ((uint32_t)p[4 * i + 3] << 24);
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor(v, o, 64));
    return v;
}

// grid: x = workgroups of one frame (tiles are dealt to them in turn), y = frame f0 + y.
// kBAligned: frame b's spans start on 16-byte boundaries where frame a's do ((a - b) % 16 == 0).
template <int C, bool kBAligned>
__global__ __launch_bounds__(kThreads) void distortion_kernel(const uint8_t *__restrict__ a,
                                                              const uint8_t *__restrict__ b, int64_t F, int64_t f0,
                                                              vcf_distortion_record *__restrict__ out)
{
    constexpr int P = kPeriod<C>;
    const int tid = threadIdx.x;
    const int64_t f = f0 + blockIdx.y;
    const uint8_t *af = a + f * F, *bf = b + f * F;
    const int64_t to_boundary = (int64_t)((16 - (reinterpret_cast<uintptr_t>(af) & 15)) & 15);
    const int64_t head = to_boundary < F ? to_boundary : F;
    const int64_t n_spans = (F - head) / kSpan;

    uint64_t sse[C], sad[C];
    us2 me[P], mo[P];
#pragma unroll
    for (int c = 0; c < C; ++c) sse[c] = sad[c] = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) me[p] = mo[p] = us2{0, 0};

    for (int64_t tile = blockIdx.x; tile * kTileSpans < n_spans; tile += gridDim.x) {
        Sums<C> t;
#pragma unroll
        for (int c = 0; c < C; ++c) t.sse[c] = t.sad[c] = 0;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t s = tile * kTileSpans + u * kThreads + tid;
            if (s < n_spans) {
                const int64_t off = head + s * kSpan;   // < F - 47: the span lies inside the frame
                uint4 va[3], vb[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) va[i] = load16<true>(af + off + 16 * i);
#pragma unroll
                for (int i = 0; i < 3; ++i) vb[i] = load16<kBAligned>(bf + off + 16 * i);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    add_dword<C>(4 * i + 0, va[i].x, vb[i].x, t, me, mo);
                    add_dword<C>(4 * i + 1, va[i].y, vb[i].y, t, me, mo);
                    add_dword<C>(4 * i + 2, va[i].z, vb[i].z, t, me, mo);
                    add_dword<C>(4 * i + 3, va[i].w, vb[i].w, t, me, mo);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) sse[c] += t.sse[c], sad[c] += t.sad[c];
    }

    // the running maxima of the halves, by class: even half p holds bytes 0 and 2 of dword p, odd half bytes 1 and 3
    uint32_t mx[C];
#pragma unroll
    for (int c = 0; c < C; ++c) mx[c] = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        mx[(4 * p + 0) % C] = max(mx[(4 * p + 0) % C], (uint32_t)me[p].x);
        mx[(4 * p + 1) % C] = max(mx[(4 * p + 1) % C], (uint32_t)mo[p].x);
        mx[(4 * p + 2) % C] = max(mx[(4 * p + 2) % C], (uint32_t)me[p].y);
        mx[(4 * p + 3) % C] = max(mx[(4 * p + 3) % C], (uint32_t)mo[p].y);
    }

    // the bytes outside the spans (at most 15 in front, 47 behind), one per lane of the frame's first wave
    if (blockIdx.x == 0 && tid < 64) {
        const int64_t p = tid < head ? (int64_t)tid : head + n_spans * kSpan + (tid - head);
        if (p < F) {
            const int cls = (int)(((p - head) % C + C) % C);
            const int va = af[p], vb = bf[p];
            const uint32_t d = (uint32_t)(va > vb ? va - vb : vb - va);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (c == cls) {
                    sse[c] += d * d;
                    sad[c] += d;
                    mx[c] = max(mx[c], d);
                }
            }
        }
    }

    __shared__ uint64_t red[kWaves][3 * C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const uint64_t s2 = wave_sum(sse[c]), s1 = wave_sum(sad[c]);
        const uint32_t m = wave_max(mx[c]);
        if ((tid & 63) == 0) {
            red[tid >> 6][3 * c + 0] = s2;
            red[tid >> 6][3 * c + 1] = s1;
            red[tid >> 6][3 * c + 2] = m;
        }
    }
    __syncthreads();
    if (tid < C) {
        uint64_t s2 = 0, s1 = 0, m = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            s2 += red[w][3 * tid + 0];
            s1 += red[w][3 * tid + 1];
            m = red[w][3 * tid + 2] > m ? red[w][3 * tid + 2] : m;
        }
        vcf_distortion_record *r = out + f * C + (int)((head + tid) % C);
        atomicAdd(reinterpret_cast<unsigned long long *>(&r->sse), (unsigned long long)s2);
        atomicAdd(reinterpret_cast<unsigned long long *>(&r->sad), (unsigned long long)s1);
        // {max_abs, pad} as one little-endian word: pad stays 0, so the word's maximum is max_abs's
        atomicMax(reinterpret_cast<unsigned long long *>(&r->max_abs), (unsigned long long)m);
    }
}

template <int C>
int launch(const uint8_t *a, const uint8_t *b, int64_t n_frames, int64_t F, vcf_distortion_record *out, hipStream_t s)
{
    const bool b_aligned = ((reinterpret_cast<uintptr_t>(a) - reinterpret_cast<uintptr_t>(b)) & 15) == 0;
    const int64_t tiles = (F / kSpan + kTileSpans - 1) / kTileSpans;
    return vcf::for_frame_chunks(n_frames, "distortion kernel", [&](int64_t f0, unsigned nf) {
        const int64_t per_frame = std::max<int64_t>(1, std::min<int64_t>(tiles, kTargetBlocks / nf));
        const dim3 grid((unsigned)per_frame, nf);
        if (b_aligned)
            hipLaunchKernelGGL((distortion_kernel<C, true>), grid, dim3(kThreads), 0, s, a, b, F, f0, out);
        else
            hipLaunchKernelGGL((distortion_kernel<C, false>), grid, dim3(kThreads), 0, s, a, b, F, f0, out);
    });
}

}  // namespace

extern "C" {

int vcf_distortion_u8(const uint8_t *a_dev, const uint8_t *b_dev, int64_t n_frames, int32_t H, int32_t W, int32_t C,
                      vcf_distortion_record *out_dev, void *stream)
{
    if (C < 1 || C > 4) return set_error(VCF_ERR_INVALID, "1 <= C <= 4 (got %d)", C);
    if (n_frames < 0 || H < 0 || W < 0)
        return set_error(VCF_ERR_INVALID, "negative size (n_frames = %lld, H = %d, W = %d)", (long long)n_frames, H, W);
    if (!a_dev || !b_dev || !out_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    if (reinterpret_cast<uintptr_t>(out_dev) & 7) return set_error(VCF_ERR_INVALID, "out_dev must be 8-byte aligned");
    if ((int64_t)H * W > INT64_MAX / C) return set_error(VCF_ERR_INVALID, "H * W * C overflows 64 bits");
    const int64_t F = (int64_t)H * W * C;
    if (n_frames == 0 || F == 0) return VCF_OK;
    if (n_frames > INT64_MAX / F) return set_error(VCF_ERR_INVALID, "n_frames * H * W * C overflows 64 bits");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = hip_check(hipMemsetAsync(out_dev, 0, (size_t)n_frames * C * sizeof(vcf_distortion_record), s),
                       "hipMemsetAsync(distortion records)");
    if (rc != 0) return rc;
    switch (C) {
    case 1: return launch<1>(a_dev, b_dev, n_frames, F, out_dev, s);
    case 2: return launch<2>(a_dev, b_dev, n_frames, F, out_dev, s);
    case 3: return launch<3>(a_dev, b_dev, n_frames, F, out_dev, s);
    default: return launch<4>(a_dev, b_dev, n_frames, F, out_dev, s);
    }
}

}  // extern "C"
