// vcf_klt_dz.hip -- the 2D-KLT codec's hot span (2D-KLT.py encode_fn / decode_fn) for
// gfx950: the exact second moments the basis is trained from, u8 RGB -> u8 indices with a
// given basis, and back, one launch per batch of frames.
//
// A frame is cut into N blocks of B x B samples (D = B * B values per block, raster order
// of blocks, row-major inside a block) after a centred zero pad and -128; per colour
// channel of YCoCg the codec learns an orthonormal D x D basis W (rows = eigenvectors of
// the blocks' covariance) and codes coef = W x.  The eigenproblem stays on the host; this
// file has
//
//   moments  S1 = sum s, S2 = sum s s^T over the blocks of a frame, s = 4 x: integers with
//            |s| <= 512, so int32 partial sums over at most 2048 blocks and int64 integer
//            atomics between workgroups give the exact result in any order.  A thread owns
//            an 8 x 8 tile of the upper triangle of S2 (and mirrors it on the way out);
//            where D is small the spare threads split the blocks of a tile.
//   encode   a workgroup owns TB consecutive blocks and walks the channels: s of the tile
//            in LDS as int16; a wave's lanes are 64 blocks, a work item is 8 consecutive
//            coefficients k, the rows W[k][.] are wave-uniform (scalar loads, float64 from
//            global memory, 4 columns at a time), the float64 dense D-term sums are FMAs
//            in registers.  / 4 (exact) / Q (float64 division), truncate, +128, wrap to
//            u8; the three channels' bytes are collected in LDS and stored in contiguous
//            runs (subband or block layout).  The float64 coefficients never leave the CU.
//   decode   the same tile; Q (k - 128) as int16 of all three channels in LDS; a work item
//            is 8 consecutive samples j of a lane's block in all three channels, the
//            float32 rows W[k][j .. j + 7] are wave-uniform and widened, the sums, the
//            inverse YCoCg and +128 are float64; clip, truncate, crop.
//
// The tiles, their LDS, the index maps and the loops that move a tile in and out are
// vcf_block_tile.h's, shared with vcf_lbt.hip; the products and the moments kernel are here.
//
// Rounding contract ("2D-KLT"): the sums run over j (decode: k) ascending with
// FMAs from zero; the encoder sums W[k][j] * s[j] and multiplies by 1/4 at the end, which
// is bit-identical to summing W[k][j] * x[j] (a power-of-two scale commutes with every
// rounding).  No result depends on the tile, the lane or the batch position.
#include <hip/hip_runtime.h>

#include "vcf_amd.h"
#include "vcf_block_tile.h"
#include "vcf_internal.h"

namespace vcf {
namespace {

constexpr int kMinB = 2, kMaxB = 16;

// ---------------------------------------------------------------------------
// moments: int64 integer atomics, a matrix per channel.  The tiling is that of
// vcf_block_tile.h's moments_tiles, kept here in full: through the shared body the compiler
// orders this kernel's instructions otherwise, and at B = 16 it measured 0.8 % slower.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kMomThreads) void klt_moments_kernel(const uint8_t *__restrict__ rgb,
                                                                 unsigned long long *__restrict__ S1,
                                                                 unsigned long long *__restrict__ S2, BlockGeom g,
                                                                 int nt, int T, int tbm)
{
    __shared__ __attribute__((aligned(16))) short X[kMomLds];
    const int D = g.D, B = g.B, DP = nt * 8;
    const int c = blockIdx.y, tid = threadIdx.x;
    const uint8_t *src = rgb + (long long)blockIdx.z * g.rgb_stride;
    unsigned long long *s1 = S1 + ((long long)blockIdx.z * 3 + c) * D;
    unsigned long long *s2 = S2 + ((long long)blockIdx.z * 3 + c) * D * D;
    const int b_lo = blockIdx.x * kMomChunk, b_hi = min(g.N, b_lo + kMomChunk);
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
                    const int b = t0 + bl, by = b / g.nbx, bx = b - by * g.nbx;
                    const int ky = d / B, kx = d - ky * B;
                    v = sample4(src, g, by * B + ky, bx * B + kx, c);
                }
                X[e] = (short)v;
            }
            __syncthreads();
            if (active) {
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
                if (ti == tj) atomicAdd(s1 + i, (unsigned long long)(long long)a1[a]);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const int j = tj * 8 + b;
                    if (j >= D) continue;
                    const unsigned long long v = (unsigned long long)(long long)acc[a][b];
                    atomicAdd(s2 + (long long)i * D + j, v);
                    if (ti != tj) atomicAdd(s2 + (long long)j * D + i, v);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
template <int LDSB>
__global__ __launch_bounds__(kTileThreads) void klt_encode_kernel(const uint8_t *__restrict__ rgb,
                                                                 uint8_t *__restrict__ kout,
                                                                 const double *__restrict__ wts, BlockGeom g, double Qd,
                                                                 int sub)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDSB];
    const int D = g.D, TB = g.TB;
    const int XS = stage_stride(D), OS = out_stride(D);
    short *X = reinterpret_cast<short *>(smem);
    uint8_t *O = smem + stage_bytes(g, 2);

    const int b0 = blockIdx.x * TB, tbv = min(TB, g.N - b0);
    const uint8_t *src = rgb + (long long)blockIdx.y * g.rgb_stride;
    uint8_t *dst = kout + (long long)blockIdx.y * g.k_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = kTileThreads >> 6;
    const int nkg = (D + 7) >> 3, nbc = (tbv + 63) >> 6;

    for (int c = 0; c < 3; ++c) {
        const double *Wc = wts + ((long long)blockIdx.y * 3 + c) * D * D;
        stage_samples(src, X, g, b0, tbv, c, [](int v) { return (short)v; });
        __syncthreads();
        for (int it = wave; it < nbc * nkg; it += nw) {
            const int kg = it % nkg, bc = it / nkg;
            const int bl = bc * 64 + lane;
            const short *xp = X + min(bl, tbv - 1) * XS;
            const double *w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = Wc + (long long)min(kg * 8 + i, D - 1) * D;
            double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int j = 0;
            for (; j + 4 <= D; j += 4) {
                const double x0 = (double)xp[j], x1 = (double)xp[j + 1], x2 = (double)xp[j + 2],
                             x3 = (double)xp[j + 3];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    acc[i] = __builtin_fma(w[i][j], x0, acc[i]);
                    acc[i] = __builtin_fma(w[i][j + 1], x1, acc[i]);
                    acc[i] = __builtin_fma(w[i][j + 2], x2, acc[i]);
                    acc[i] = __builtin_fma(w[i][j + 3], x3, acc[i]);
                }
            }
            for (; j < D; ++j) {
                const double x0 = (double)xp[j];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = __builtin_fma(w[i][j], x0, acc[i]);
            }
            if (bl < tbv) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int k = kg * 8 + i;
                    if (k >= D) continue;
                    const int q = (int)((acc[i] * 0.25) / Qd) + 128;   // |coef / Q| <= 128 * 256
                    O[bl * OS + k * 3 + c] = (uint8_t)(q & 255);
                }
            }
        }
        __syncthreads();   // X is staged again for the next channel
    }
    scatter_indices(O, dst, g, b0, tbv, sub);
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
// acc[c][jj] += W_c[k][j0 + jj] * y_c[k] over k ascending; TAIL clamps the columns of the last,
// partial group (the loads of a full group are contiguous and wave-uniform)
template <bool TAIL>
__device__ inline void klt_synth(const float *__restrict__ W0, const short *y0, int ys, int D, int j0,
                                 double (&acc)[3][8])
{
    const long long DD = (long long)D * D;
    for (int k = 0; k < D; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float *wr = W0 + c * DD + (long long)k * D;
            const double y = (double)y0[c * ys + k];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int j = TAIL ? min(j0 + jj, D - 1) : j0 + jj;
                acc[c][jj] = __builtin_fma((double)wr[j], y, acc[c][jj]);
            }
        }
    }
}

template <int LDSB>
__global__ __launch_bounds__(kTileThreads) void klt_decode_kernel(const uint8_t *__restrict__ kin,
                                                                 uint8_t *__restrict__ rgb,
                                                                 const float *__restrict__ wts, BlockGeom g, int Q, int sub)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDSB];
    const int D = g.D, TB = g.TB;
    const int XS = stage_stride(D), OS = out_stride(D);
    const int ys = align16(TB * XS * 2) / 2;   // one channel's int16 tile, in elements
    short *Y = reinterpret_cast<short *>(smem);
    uint8_t *O = smem + 3 * ys * 2;

    const int b0 = blockIdx.x * TB, tbv = min(TB, g.N - b0);
    const uint8_t *src = kin + (long long)blockIdx.y * g.k_stride;
    uint8_t *dst = rgb + (long long)blockIdx.y * g.rgb_stride;
    const float *W0 = wts + (long long)blockIdx.y * 3 * D * D;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = kTileThreads >> 6;
    const int njg = (D + 7) >> 3, nbc = (tbv + 63) >> 6;

    // u8 -> int16 - 128 -> Q k (int16, wrapping) -> block layout
    gather_indices(src, Y, ys, g, b0, tbv, sub, Q, [](short y, int, int) { return y; });
    __syncthreads();
    for (int it = wave; it < nbc * njg; it += nw) {
        const int jg = it % njg, bc = it / njg;
        const int bl = bc * 64 + lane, j0 = jg * 8;
        const short *y0 = Y + min(bl, tbv - 1) * XS;
        double acc[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[c][jj] = 0.0;
        if (j0 + 8 <= D) klt_synth<false>(W0, y0, ys, D, j0, acc);
        else klt_synth<true>(W0, y0, ys, D, j0, acc);
        if (bl < tbv) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int j = j0 + jj;
                if (j >= D) continue;
                const double Yv = acc[0][jj], Co = acc[1][jj], Cg = acc[2][jj];
                const double R = (Yv + Co) - Cg + 128.0, G = (Yv + Cg) + 128.0, Bv = (Yv - Co) - Cg + 128.0;
                uint8_t *o = O + bl * OS + j * 3;
                o[0] = (uint8_t)(int)fmin(fmax(R, 0.0), 255.0);
                o[1] = (uint8_t)(int)fmin(fmax(G, 0.0), 255.0);
                o[2] = (uint8_t)(int)fmin(fmax(Bv, 0.0), 255.0);
            }
        }
    }
    __syncthreads();
    crop_pixels(O, dst, g, b0, tbv);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int check_shape(int32_t H, int32_t W, int32_t B)
{
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad shape %d x %d", H, W);
    if (B > kMaxB) return set_error(VCF_ERR_UNSUPPORTED, "block size %d: the KLT kernels cover 2 <= B <= 16", B);
    if (B < kMinB)
        return set_error(VCF_ERR_INVALID, "block size %d: blocks of one sample have no covariance matrix", B);
    if (!frame_fits_int32(H, W, B)) return set_error(VCF_ERR_INVALID, "frame too large");
    return VCF_OK;
}

int check_args(const void *a, const void *b, const void *c, int64_t n_frames, int32_t H, int32_t W, int32_t B,
               int32_t Q, uint32_t flags, BlockGeom &g)
{
    if (!a || !b || !c) return set_error(VCF_ERR_INVALID, "null buffer");
    if (n_frames < 1) return set_error(VCF_ERR_INVALID, "n_frames < 1");
    const int rc = check_shape(H, W, B);
    if (rc != VCF_OK) return rc;
    if (Q < 1 || Q > 32767) return set_error(VCF_ERR_INVALID, "quantization step %d out of range", Q);
    if (flags & ~VCF_DCT_NO_SUBBANDS) return set_error(VCF_ERR_INVALID, "unknown flags 0x%x", flags);
    g = make_block_geom(H, W, B);
    if (g.N < 2) return set_error(VCF_ERR_INVALID, "a frame of one block has no covariance matrix");
    return VCF_OK;
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_klt_padded_shape(int32_t H, int32_t W, int32_t block_size, int32_t *Hp, int32_t *Wp, int32_t *pad_top,
                         int32_t *pad_left)
{
    if (!Hp || !Wp || !pad_top || !pad_left) return set_error(VCF_ERR_INVALID, "null pointer");
    const int rc = check_shape(H, W, block_size);
    if (rc != VCF_OK) return rc;
    const BlockGeom g = make_block_geom(H, W, block_size);
    *Hp = g.Hp;
    *Wp = g.Wp;
    *pad_top = g.top;
    *pad_left = g.left;
    return VCF_OK;
}

int vcf_klt_moments(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                    int64_t *s1_dev, int64_t *s2_dev, void *stream)
{
    BlockGeom g;
    int rc = check_args(rgb_dev, s1_dev, s2_dev, n_frames, H, W, block_size, 1, 0, g);
    if (rc != VCF_OK) return rc;
    VCF_REQUIRE_ALIGNED(s1_dev, 8);
    VCF_REQUIRE_ALIGNED(s2_dev, 8);
    const long long D = g.D;
    rc = hip_check(hipMemsetAsync(s1_dev, 0, (size_t)(n_frames * 3 * D * 8), (hipStream_t)stream), "hipMemsetAsync(S1)");
    if (rc != VCF_OK) return rc;
    rc = hip_check(hipMemsetAsync(s2_dev, 0, (size_t)(n_frames * 3 * D * D * 8), (hipStream_t)stream),
                   "hipMemsetAsync(S2)");
    if (rc != VCF_OK) return rc;
    const BlockPlan p = make_block_plan(g, false, 2);
    return for_frame_chunks(n_frames, "klt_moments_kernel launch", [&](int64_t f0, unsigned nf) {
        hipLaunchKernelGGL(klt_moments_kernel, dim3((unsigned)p.chunks, 3, nf), dim3(kMomThreads), 0, (hipStream_t)stream,
                           rgb_dev + f0 * g.rgb_stride, (unsigned long long *)s1_dev + f0 * 3 * D,
                           (unsigned long long *)s2_dev + f0 * 3 * D * D, g, p.nt, p.T, p.tbm);
    });
}

int vcf_klt_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const double *weights_f64_dev, uint8_t *k_dev, void *stream)
{
    BlockGeom g;
    const int rc = check_args(rgb_dev, weights_f64_dev, k_dev, n_frames, H, W, block_size, Q, flags, g);
    if (rc != VCF_OK) return rc;
    VCF_REQUIRE_ALIGNED(weights_f64_dev, 8);
    const BlockPlan p = make_block_plan(g, false, 2);
    if (p.cls < 0) return set_error(VCF_ERR_UNSUPPORTED, "block size %d: tile does not fit the LDS", block_size);
    const int sub = (flags & VCF_DCT_NO_SUBBANDS) ? 0 : 1;
    const long long DD = (long long)g.D * g.D;
    return for_frame_chunks(n_frames, "klt_encode_kernel launch", [&](int64_t f0, unsigned nf) {
        with_lds_class(p.cls, [&](auto lds) {
            hipLaunchKernelGGL((klt_encode_kernel<decltype(lds)::value>), dim3((unsigned)p.tiles, nf), dim3(kTileThreads),
                               0, (hipStream_t)stream, rgb_dev + f0 * g.rgb_stride, k_dev + f0 * g.k_stride,
                               weights_f64_dev + f0 * 3 * DD, g, (double)Q, sub);
        });
    });
}

int vcf_klt_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const float *weights_f32_dev, uint8_t *rgb_dev, void *stream)
{
    BlockGeom g;
    const int rc = check_args(k_dev, weights_f32_dev, rgb_dev, n_frames, H, W, block_size, Q, flags, g);
    if (rc != VCF_OK) return rc;
    VCF_REQUIRE_ALIGNED(weights_f32_dev, 4);
    const BlockPlan p = make_block_plan(g, true, 2);
    if (p.cls < 0) return set_error(VCF_ERR_UNSUPPORTED, "block size %d: tile does not fit the LDS", block_size);
    const int sub = (flags & VCF_DCT_NO_SUBBANDS) ? 0 : 1;
    const long long DD = (long long)g.D * g.D;
    return for_frame_chunks(n_frames, "klt_decode_kernel launch", [&](int64_t f0, unsigned nf) {
        with_lds_class(p.cls, [&](auto lds) {
            hipLaunchKernelGGL((klt_decode_kernel<decltype(lds)::value>), dim3((unsigned)p.tiles, nf), dim3(kTileThreads),
                               0, (hipStream_t)stream, k_dev + f0 * g.k_stride, rgb_dev + f0 * g.rgb_stride,
                               weights_f32_dev + f0 * 3 * DD, g, (int)Q, sub);
        });
    });
}

}  // extern "C"
