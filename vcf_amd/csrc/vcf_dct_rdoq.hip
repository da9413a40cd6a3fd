// vcf_dct_rdoq.hip -- the fused DCT(B=8) + deadzone encode with a rate-distortion optimised
// quantizer (RDOQ), and the vcf_dct_dz_encode_rdoq entry of the C ABI (include/vcf_amd.h has the
// rule).  Encoder side only: the output is an ordinary index frame of
// vcf_dct_dz_encode's layout, and every decoder reads it.  Not in the reference.
//
// The kernel is dct_dz_encode_kernel of vcf_dct_dz.hip with one step between the quotient and its
// byte: a block per lane, the same loads (load_block), the same transforms (vcf_dct_block.h: the
// packed path with the zero-row skip for a power-of-two Q, the scalar one otherwise), the same LDS
// image and copy-out (vcf_dct_tile.h).  The transforms hand over the quotient q whose truncation
// is the deadzone index k0, and the coefficient c in the reference's units comes back from it
// exactly: c = q * Q for a power-of-two Q (the folded constants only moved a power of two), and
// c = t * 2^-e from the undivided output t otherwise.  Every index byte first goes into the image
// as the plain kernel writes it; a coefficient whose k0 is zero -- nearly all of them -- pays half
// an OR on top.  After each row pair, a wave that has a non-zero index in it runs the decision
// (rdoq_row_pair) for those positions only: the lanes concerned read the cost table (float64, in
// the caller's HBM buffer: the costs of k0, k0 - sign and 0, three independent loads), compare three
// float64 costs and rewrite their byte where the index drops.  A row pair the wave proves zero is
// skipped as in the plain kernel: a zero k0 is never a candidate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "vcf_amd.h"
#include "vcf_dct8.h"
#include "vcf_dct_block.h"
#include "vcf_dct_tile.h"
#include "vcf_internal.h"

namespace vcf {
namespace {

using namespace dct_tile;

constexpr int64_t kCostFrame = 64 * 3 * 256;   // doubles of one frame's table: [region][channel][byte]

struct RdoqArgs {
    const double *cost;       // the table of the launch's first frame
    long long frame_stride;   // doubles from a frame's table to the next one's: kCostFrame, or 0 for one table
    double lambda;
    int Q;
    float Qf;                 // (float)Q, exact for the power-of-two Q that use it
};

// The index of coefficient c whose deadzone index k0 is not zero; bits = the 256 costs of its
// region and channel.  J(k) = d * d + lambda * bits[(k + 128) & 255], d = c - Q k, each operation
// rounded on its own (the library is built with -ffp-contract=off).  k0 - sign replaces k0 at
// J <= J, then 0 replaces the better of the two at J <= J; where k0 - sign is 0 itself the second
// comparison is of J(0) with either J(0) or a smaller value, so it decides nothing and needs no
// branch.  An index outside [-128, 127] wraps modulo 256 in the byte as in the plain kernel.
__device__ __forceinline__ int rdoq_choose(float c, int k0, const RdoqArgs &R, const double *__restrict__ bits)
{
    if ((uint32_t)(k0 + 128) > 255u) return k0;
    const int k1 = k0 - (k0 > 0 ? 1 : -1);
    const double b0 = bits[k0 + 128], b1 = bits[k1 + 128], bz = bits[128];
    const double cd = (double)c;
    const double d0 = cd - (double)(R.Q * k0), d1 = cd - (double)(R.Q * k1);
    double best_j = d0 * d0 + R.lambda * b0;
    int best = k0;
    const double j1 = d1 * d1 + R.lambda * b1;
    if (j1 <= best_j) {
        best_j = j1;
        best = k1;
    }
    const double jz = cd * cd + R.lambda * bz;   // d = c - 0
    if (jz <= best_j) best = 0;
    return best;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The decision for the two rows 2 p, 2 p + 1 of channel C, after their plain index bytes went into
// the LDS image: acc[8 (i & 1) + j] is what the row pass left at (i, j) -- the quotient q for a
// power-of-two Q, else the undivided output t = c * 2^e, e = qexp<C>(i, j).  One copy of the
// decision per row pair instead of one per coefficient (192 inline copies tripled the kernel's
// code, past the instruction cache, and spilled): a loop over the positions at which some lane of
// the wave has a non-zero index, the position wave-uniform, so acc is read by a scalar register
// index and the table's row by a scalar base.  A lane takes part where its own index is not zero,
// and rewrites its byte of the image where the decision lowers it.
template <int C, bool POW2, bool SUB, int T>
__device__ __forceinline__ void rdoq_row_pair(int p, const f32x16 &acc, const EncConsts &K, const RdoqArgs &R,
                                              const double *__restrict__ cost, uint8_t *stage, int tid)
{
    // bit n: this lane's index at position n is not zero.  |q| >= 1, or |t| >= the divisor: both
    // floats, so a t below the divisor is at most its predecessor and the quotient rounds below 1
    uint32_t m = 0;
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        const float thr = POW2 ? 1.0f : K.qd[qexp<C>(2 * p + (n >> 3), n & 7) - 3];
        m |= abs_f(acc[n]) >= thr ? (1u << n) : 0u;
    }
    for (;;) {
        const uint64_t act = __builtin_amdgcn_ballot_w64(m != 0);
        if (act == 0) break;
        const uint32_t mm = __builtin_amdgcn_readlane(m, (int)__builtin_ctzll(act));
        const int n = __builtin_ctz(mm);                  // wave-uniform
        const int i = 2 * p + (n >> 3), j = n & 7;
        const bool mine = (m >> n) & 1u;
        m &= ~(1u << n);
        const float a = acc[n];
        float q, c;
        if (POW2) {
            q = a;
            c = a * R.Qf;
        } else {
            const int e = qexp<C>(i, j);
            const float d = e == 3 ? K.qd[0] : e == 4 ? K.qd[1] : e == 5 ? K.qd[2] : K.qd[3];
            q = quant_div<false>(a, d);
            c = a * (1.0f / (float)(1 << e));
        }
        const int k0 = cvt_trunc_i32(q);
        if (mine && k0 != 0) {
            const int k = rdoq_choose(c, k0, R, cost + ((i * 8 + j) * 3 + C) * 256);
            if (k != k0) {
                if (SUB) stage[(i * 8 + j) * (T * 3) + tid * 3 + C] = (uint8_t)k;
                else stage[i * (T * 24) + tid * 24 + j * 3 + C] = (uint8_t)k;
            }
        }
    }
}

template <bool POW2, bool SUB, int T>
__device__ __forceinline__ void encode_block_rdoq(uint32_t (&raw)[8][6], const EncConsts &K, const FinalK &rowk,
                                                  const RdoqArgs &R, const double *__restrict__ cost,
                                                  uint8_t *stage, int tid)
{
    auto channel = [&](auto Cc) {
        constexpr int C = decltype(Cc)::value;
        f32x16 acc;
        uint32_t any = 0;
        // the plain kernel's sink, the row pass's output kept until its row pair is complete
        auto sink = [&](int i, int j, float a, float q) {
            const uint32_t k = (uint32_t)cvt_trunc_i32(q);
            if (SUB) stage[(i * 8 + j) * (T * 3) + tid * 3 + C] = (uint8_t)k;
            else stage[i * (T * 24) + tid * 24 + j * 3 + C] = (uint8_t)k;
            acc[(i & 1) * 8 + j] = a;
            any |= k;
            if ((i & 1) && j == 7) {
                if (!wave_all(any == 0)) rdoq_row_pair<C, POW2, SUB, T>(i >> 1, acc, K, R, cost, stage, tid);
                any = 0;
            }
        };
        // rows 2..7 of the image are zero already: a row pair that the wave proves zero hands over nothing
        if constexpr (POW2)
            encode_block_channel_pk_q<C, 2>(raw, rowk, K.qd[0], [&](int i, int j, float q) { sink(i, j, q, q); });
        else
            encode_block_channel_fold_q<C, false, false, true>(raw, rowk, K.qd, sink);
    };
    channel(std::integral_constant<int, 0>{});
    opaque(raw, (uint32_t)tid);
    channel(std::integral_constant<int, 1>{});
    opaque(raw, (uint32_t)tid);
    channel(std::integral_constant<int, 2>{});
}

// Three waves per SIMD like the plain kernel (its LDS image allows no more): left alone the
// register allocator spreads the float64 temporaries of the decision over 200 VGPRs, two waves.
template <bool POW2, bool SUB, bool PAD, int T = kTile>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(3))) void dct_dz_encode_rdoq_kernel(const uint8_t *__restrict__ rgb,
                                                               uint8_t *__restrict__ kout, Geom g, EncConsts K,
                                                               FinalK rowk, RdoqArgs R)
{
    __shared__ __attribute__((aligned(16))) uint8_t stage[64 * T * 3];
    __shared__ uint32_t rowbase[T];
    const int tid = threadIdx.x;
    long long frame;
    int tile;
    tile_of_workgroup(frame, tile);
    const int n0 = tile * T;
    const int nvalid = min(T, g.nblocks - n0);
    uint32_t raw[8][6];
    if (tid < nvalid) {
        int by, bx;
        tile_block(g, n0 + tid, by, bx);
        rowbase[tid] = block_rowbase<SUB>(g, by, bx);
        __builtin_amdgcn_s_setprio(3);
        load_block<PAD>(g, rgb + frame * g.in_stride, by, bx, raw);
        __builtin_amdgcn_s_setprio(0);
    }
    if constexpr (POW2) zero_wave_rows<SUB, T>(stage, tid);
    if (tid < nvalid) encode_block_rdoq<POW2, SUB, T>(raw, K, rowk, R, R.cost + frame * R.frame_stride, stage, tid);
    __syncthreads();
    __builtin_amdgcn_s_setprio(3);
    if (nvalid == T && g.vec) move_runs_full<SUB, T>(g, stage, rowbase, kout + frame * g.out_stride);
    else move_runs_tab<SUB, true, T>(g, stage, rowbase, kout + frame * g.out_stride, nvalid);
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_dct_rdoq_tile(void) { return kTile; }

int vcf_dct_dz_encode_rdoq(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                           int32_t Q, uint32_t flags, const double *cost_dev, int64_t cost_frames,
                           int64_t cost_capacity, double lambda, uint8_t *k_dev, void *stream)
{
    if (!rgb_dev || !k_dev || !cost_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    if (n_frames < 1) return set_error(VCF_ERR_INVALID, "n_frames = %lld: at least one frame", (long long)n_frames);
    if (H <= 0 || W <= 0)
        return set_error(VCF_ERR_INVALID, "Input image must be a 3D array (height, width, channels).");
    if (Q < 1) return set_error(VCF_ERR_INVALID, "quantization step %d out of range", Q);
    if (flags & ~(VCF_DCT_NO_SUBBANDS | VCF_DCT_PERCEPTUAL))
        return set_error(VCF_ERR_INVALID, "unknown flags 0x%x", flags);
    if (cost_frames != 1 && cost_frames != n_frames)
        return set_error(VCF_ERR_INVALID, "cost_frames = %lld: 1 or n_frames = %lld", (long long)cost_frames,
                         (long long)n_frames);
    if (cost_frames > INT64_MAX / kCostFrame || cost_capacity < cost_frames * kCostFrame)
        return set_error(VCF_ERR_INVALID, "cost_capacity = %lld: %lld costs are read", (long long)cost_capacity,
                         (long long)(cost_frames * kCostFrame));
    VCF_REQUIRE_ALIGNED(cost_dev, 8);
    if (!std::isfinite(lambda) || lambda < 0.0) return set_error(VCF_ERR_INVALID, "lambda = %g: finite and >= 0", lambda);
    // the kernels address within a frame with 32-bit offsets
    if ((long long)((H + 7) & ~7) * ((W + 7) & ~7) * 3 >= (1LL << 31))
        return set_error(VCF_ERR_INVALID, "frame too large");
    if (block_size != 8)
        return set_error(VCF_ERR_UNSUPPORTED, "block_size %d: the RDOQ encode has the 8x8 kernel only", block_size);
    if (flags & VCF_DCT_PERCEPTUAL) return set_error(VCF_ERR_UNSUPPORTED, "the RDOQ encode has no -p");
    const bool pow2 = (Q & (Q - 1)) == 0;
    // the fp32 divisor Q*2^6 must be exact for a general (non power-of-two) Q
    if (!pow2 && Q > (1 << 18)) return set_error(VCF_ERR_UNSUPPORTED, "quantization step %d too large", Q);

    Geom g;
    make_geom(H, W, k_dev, g);
    const bool sub = !(flags & VCF_DCT_NO_SUBBANDS);
    const bool pad = rgb_needs_bytes(g, rgb_dev);
    EncConsts K;
    make_enc_consts(K, Q);
    const FinalK rowk = pow2 ? row_final_k(Q) : final_k(1.0f, 1.0f);
    const long long stride = cost_frames == 1 ? 0 : kCostFrame;
    return for_frame_chunks(n_frames, "dct_dz_encode_rdoq_kernel launch", [&](int64_t f0, unsigned nf) {
        const dim3 grid(g.tiles_per_frame, nf);
        const uint8_t *in = rgb_dev + f0 * g.in_stride;
        uint8_t *out = k_dev + f0 * g.out_stride;
        const RdoqArgs R{cost_dev + f0 * stride, stride, lambda, (int)Q, (float)Q};
#define VCF_RDOQ(P2, SB, PD)                                                                                 \
        if (pow2 == P2 && sub == SB && pad == PD)                                                            \
            hipLaunchKernelGGL((dct_dz_encode_rdoq_kernel<P2, SB, PD>), grid, dim3(kTile), 0,               \
                               (hipStream_t)stream, in, out, g, K, rowk, R);
        VCF_RDOQ(true, true, false) else VCF_RDOQ(true, true, true)
        else VCF_RDOQ(true, false, false) else VCF_RDOQ(true, false, true)
        else VCF_RDOQ(false, true, false) else VCF_RDOQ(false, true, true)
        else VCF_RDOQ(false, false, false) else VCF_RDOQ(false, false, true)
#undef VCF_RDOQ
    });
}

}  // extern "C"
