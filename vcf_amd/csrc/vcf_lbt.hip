// vcf_lbt.hip -- the 2D-LBT codec's hot span (2D-LBT.py encode_fn / decode_fn) for gfx950:
// a linear autoencoder of the B x B blocks, trained per frame with Adam, and the deadzone
// chain around it.  One launch per batch of frames for each of
//
//   moments  S1 = sum x, S2 = sum x x^T over the 3 N blocks of a frame (the three YCoCg
//            channels pooled), x the D = B * B values of a block after the centred zero
//            pad and -128.  The kernel works on s = 4 x (integers, |s| <= 512) with int32
//            partial sums over at most 2048 blocks (vcf_block_tile.h's moments_tiles) and adds
//            them to the float64 results with atomics: every partial and every total is
//            an integer below 2^53 (scaled by the exact 1/4 and 1/16), so the float64
//            sums are exact in any order.
//   train    one workgroup (4 waves) per frame, every epoch on the device in one launch.
//            The model is linear, so loss and gradients are functions of the D x D second
//            moments alone (below); per epoch six 64 x 64 x 64 float32 products on
//            v_mfma_f32_32x32x2_f32, one 32 x 32 output tile per wave.  C, S, both weight
//            matrices and three scratch matrices live in LDS (7 x 16.25 KiB); the Adam
//            moments and the gradients live in registers in the MFMA output layout.
//   encode   vcf_block_tile.h's tiles, as vcf_klt_dz.hip, in float32: a workgroup owns TB blocks,
//            a lane a block, a work item 8 coefficients; rows of We are wave-uniform.
//   decode   likewise, with the stored float32 decoder matrix.
//
// Training in moment form.  X: the 3 N x D blocks minus the scalar mean mu, C = X^T X / rows,
// m = the column means of X, S = C - m m^T, A = We^T Wd^T, E = A - I:
//   mse   = tr(E^T C E) / D                       G = C E
//   var_j = we_j^T S we_j                         P = We S
//   dWe   = (2 / D) (G Wd)^T + (2 lambda / D) diag(1 / (var + 1e-6)) P
//   dWd   = (2 / D) (We G)^T
// D is padded to 64 with zero rows and columns: the padding has zero gradient and stays zero.
//
// Rounding contract ("2D-LBT"): every product sums over its inner index
// ascending in float32 FMAs from zero (the f32 MFMA is an fmaf chain); encode and decode sum
// over j (decode: k) ascending.  No result depends on the tile, the lane or the batch
// position.
#include <hip/hip_runtime.h>

#include "vcf_amd.h"
#include "vcf_block_tile.h"
#include "vcf_internal.h"

namespace vcf {
namespace {

constexpr int kTrainThreads = 256; // train: one wave per SIMD
constexpr int kMinB = 2, kMaxB = 8;
constexpr int kDP = 64;            // the training matrices' padded dimension
constexpr int kLD = 65;            // and their LDS row stride (odd: column reads hit 32 banks)
constexpr int kMat = kDP * kLD;

// -p: Y_QSSs / 121 and C_QSSs / 99 (float64) per coefficient
struct LbtScale {
    int on;
    double t[2][kDP];
};

// ---------------------------------------------------------------------------
// moments: float64 atomics of the exact 1/4 and 1/16; the three channels add into one matrix
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kMomThreads) void lbt_moments_kernel(const uint8_t *__restrict__ rgb,
                                                                 double *__restrict__ S1, double *__restrict__ S2,
                                                                 BlockGeom g, int nt, int T, int tbm)
{
    const int D = g.D;
    moments_tiles(rgb + (long long)blockIdx.z * g.rgb_stride, S1 + (long long)blockIdx.z * D,
                  S2 + (long long)blockIdx.z * D * D, g, nt, T, tbm, blockIdx.x, blockIdx.y,
                  // v sums s = 4 x (S1) or s s^T = 16 x x^T (S2): the exact 1/4 and 1/16 give the sums of x
                  [](int v, bool first) { return (double)v * (first ? 0.25 : 0.0625); });
}

// ---------------------------------------------------------------------------
// train
// ---------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

// element r of a lane's 16 of a 32 x 32 MFMA output tile
__device__ inline int tile_row(int lane, int r) { return (r >> 2) * 8 + (lane >> 5) * 4 + (r & 3); }
__device__ inline int tile_col(int lane) { return lane & 31; }

// acc[i][j] += sum over k ascending of L(i, k) R(k, j) for the wave's tile at (i0, j0):
// L(i, k) = L[i * LSI + k * LSK], R(k, j) = R[k * RSK + j * RSJ]
template <int LSI, int LSK, int RSK, int RSJ>
__device__ inline void mm_tile(f32x16 &acc, const float *L, const float *R, int i0, int j0, int lane)
{
    const float *lp = L + (i0 + (lane & 31)) * LSI + (lane >> 5) * LSK;
    const float *rp = R + (lane >> 5) * RSK + (j0 + (lane & 31)) * RSJ;
#pragma unroll 8
    for (int k = 0; k < kDP; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(lp[k * LSK], rp[k * RSK], acc, 0, 0, 0);
}

__device__ inline float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kTrainThreads) void lbt_train_kernel(const double *__restrict__ S1,
                                                                 const double *__restrict__ S2,
                                                                 float *__restrict__ We_g, float *__restrict__ Wd_g,
                                                                 float *__restrict__ mean_out,
                                                                 float *__restrict__ loss_out, int D, double rows,
                                                                 int epochs, double lr, float lambda)
{
    __shared__ float sm[7 * kMat];
    __shared__ float rinv[kDP];
    __shared__ float red[8];
    float *We = sm, *Wd = sm + kMat, *C = sm + 2 * kMat, *S = sm + 3 * kMat, *E = sm + 4 * kMat, *G = sm + 5 * kMat,
          *P = sm + 6 * kMat;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = (wave >> 1) * 32, j0 = (wave & 1) * 32;
    const long long f = blockIdx.x;
    const double *s1 = S1 + f * D, *s2 = S2 + f * D * D;
    float *we_g = We_g + f * D * D, *wd_g = Wd_g + f * D * D;

    // the scalar mean (2D-LBT.py:101), a float32 value; every thread sums the same D terms
    double tot = 0.0;
    for (int d = 0; d < D; ++d) tot += s1[d];
    const float mu = (float)(tot / (rows * (double)D));
    const double mud = (double)mu;
    for (int e = tid; e < kDP * kDP; e += kTrainThreads) {
        const int i = e >> 6, j = e & 63;
        float c = 0.f, s = 0.f, we = 0.f, wd = 0.f;
        if (i < D && j < D) {
            const double cd = (s2[i * D + j] - mud * (s1[i] + s1[j]) + rows * mud * mud) / rows;
            const double mi = s1[i] / rows - mud, mj = s1[j] / rows - mud;
            c = (float)cd;
            s = (float)(cd - mi * mj);
            we = we_g[i * D + j];
            wd = wd_g[i * D + j];
        }
        C[i * kLD + j] = c;
        S[i * kLD + j] = s;
        We[i * kLD + j] = we;
        Wd[i * kLD + j] = wd;
    }

    f32x16 mE, vE, mD, vD;
#pragma unroll
    for (int r = 0; r < 16; ++r) mE[r] = vE[r] = mD[r] = vD[r] = 0.f;
    const float Df = (float)D;
    const float c2 = 2.f / Df, c3 = 2.f * lambda / Df;
    const float b2 = 0.999f, eps = 1e-8f;
    const float omb1 = (float)(1.0 - 0.9), omb2 = (float)(1.0 - 0.999);   // 1 - beta in double, as torch forms them
    double b1t = 1.0, b2t = 1.0;
    const int col = j0 + tile_col(lane);
    float mse = 0.f, gain = 0.f;

    for (int t = 1;; ++t) {
        __syncthreads();   // the weights of this epoch are in LDS
        f32x16 e, p;
#pragma unroll
        for (int r = 0; r < 16; ++r) e[r] = p[r] = 0.f;
        mm_tile<1, kLD, 1, kLD>(e, We, Wd, i0, j0, lane);    // A[a][b] = sum_k We[k][a] Wd[b][k]
        mm_tile<kLD, 1, kLD, 1>(p, We, S, i0, j0, lane);     // P[j][a] = sum_c We[j][c] S[c][a]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + tile_row(lane, r);
            if (row == col && row < D) e[r] -= 1.f;
            E[row * kLD + col] = e[r];
            P[row * kLD + col] = p[r];
        }
        __syncthreads();
        f32x16 g;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = 0.f;
        mm_tile<kLD, 1, kLD, 1>(g, C, E, i0, j0, lane);      // G[a][b] = sum_c C[a][c] E[c][b]
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            G[(i0 + tile_row(lane, r)) * kLD + col] = g[r];
            part = fmaf(e[r], g[r], part);
        }
        part = wave_sum(part);
        if (lane == 0) red[wave] = part;
        if (wave == 0) {
            // var_j = sum_a P[j][a] We[j][a]; the true variance is not negative
            float v = 0.f;
            for (int a = 0; a < kDP; ++a) v = fmaf(P[lane * kLD + a], We[lane * kLD + a], v);
            v = fmaxf(v, 0.f) + 1e-6f;
            rinv[lane] = lane < D ? __fdiv_rn(1.f, v) : 0.f;
            const float lg = wave_sum(lane < D ? logf(v) : 0.f);
            if (lane == 0) red[4] = lg;
        }
        __syncthreads();
        mse = (((red[0] + red[1]) + red[2]) + red[3]) / Df;
        gain = red[4] / Df;
        if (t > epochs) break;

        f32x16 de, dd;
#pragma unroll
        for (int r = 0; r < 16; ++r) de[r] = dd[r] = 0.f;
        mm_tile<1, kLD, 1, kLD>(de, Wd, G, i0, j0, lane);    // (G Wd)^T[k][a] = sum_b Wd[b][k] G[a][b]
        mm_tile<1, kLD, 1, kLD>(dd, G, We, i0, j0, lane);    // (We G)^T[b][k] = sum_a G[a][b] We[k][a]

        // torch.optim.Adam, defaults (single-tensor form)
        b1t *= 0.9;
        b2t *= 0.999;
        const float step = (float)(lr / (1.0 - b1t));
        const float bc2s = (float)sqrt(1.0 - b2t);
        float we_new[16], wd_new[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + tile_row(lane, r);
            const float gE = c2 * de[r] + c3 * (p[r] * rinv[row]);
            const float gD = c2 * dd[r];
            mE[r] = mE[r] + (gE - mE[r]) * omb1;
            mD[r] = mD[r] + (gD - mD[r]) * omb1;
            vE[r] = vE[r] * b2 + (omb2 * gE) * gE;
            vD[r] = vD[r] * b2 + (omb2 * gD) * gD;
            const float dnE = __fdiv_rn(__fsqrt_rn(vE[r]), bc2s) + eps;
            const float dnD = __fdiv_rn(__fsqrt_rn(vD[r]), bc2s) + eps;
            we_new[r] = We[row * kLD + col] - step * __fdiv_rn(mE[r], dnE);
            wd_new[r] = Wd[row * kLD + col] - step * __fdiv_rn(mD[r], dnD);
        }
        __syncthreads();   // every wave has read the old weights and G
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i0 + tile_row(lane, r);
            We[row * kLD + col] = we_new[r];
            Wd[row * kLD + col] = wd_new[r];
        }
    }

    for (int e = tid; e < D * D; e += kTrainThreads) {
        const int i = e / D, j = e - i * D;
        we_g[e] = We[i * kLD + j];
        wd_g[e] = Wd[i * kLD + j];
    }
    if (tid == 0) {
        mean_out[f] = mu;
        loss_out[f * 3] = mse + lambda * gain;
        loss_out[f * 3 + 1] = mse;
        loss_out[f * 3 + 2] = gain;
    }
}

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
template <int LDSB>
__global__ __launch_bounds__(kTileThreads) void lbt_encode_kernel(const uint8_t *__restrict__ rgb,
                                                                 uint8_t *__restrict__ kout,
                                                                 const float *__restrict__ wts,
                                                                 const float *__restrict__ means, BlockGeom g, float Qf,
                                                                 int sub, LbtScale pq)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDSB];
    const int D = g.D, TB = g.TB;
    const int XS = stage_stride(D), OS = out_stride(D);
    float *X = reinterpret_cast<float *>(smem);
    uint8_t *O = smem + stage_bytes(g, 4);

    const int b0 = blockIdx.x * TB, tbv = min(TB, g.N - b0);
    const uint8_t *src = rgb + (long long)blockIdx.y * g.rgb_stride;
    uint8_t *dst = kout + (long long)blockIdx.y * g.k_stride;
    const float *Wf = wts + (long long)blockIdx.y * D * D;
    const float mu = means[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = kTileThreads >> 6;
    const int nkg = (D + 7) >> 3, nbc = (tbv + 63) >> 6;

    for (int c = 0; c < 3; ++c) {
        stage_samples(src, X, g, b0, tbv, c, [mu](int v) { return (float)v * 0.25f - mu; });
        __syncthreads();
        for (int it = wave; it < nbc * nkg; it += nw) {
            const int kg = it % nkg, bc = it / nkg;
            const int bl = bc * 64 + lane;
            const float *xp = X + min(bl, tbv - 1) * XS;
            const float *w[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) w[i] = Wf + min(kg * 8 + i, D - 1) * D;
            float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < D; ++j) {
                const float x0 = xp[j];
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] = fmaf(w[i][j], x0, acc[i]);
            }
            if (bl < tbv) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int k = kg * 8 + i;
                    if (k >= D) continue;
                    float y = acc[i];
                    if (pq.on) y = (float)((double)y * pq.t[c ? 1 : 0][k]);   // :413-415, float64 product
                    const int q = (int)__fdiv_rn(y, Qf) + 128;
                    O[bl * OS + k * 3 + c] = (uint8_t)min(max(q, 0), 255);
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
// acc[c][jj] += Wd[j0 + jj][k] * y_c[k] over k ascending; TAIL clamps the rows of the last group
template <bool TAIL>
__device__ inline void lbt_synth(const float *__restrict__ Wf, const short *y0, int ys, int D, int j0,
                                 float (&acc)[3][8])
{
    const float *wr[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) wr[jj] = Wf + (TAIL ? min(j0 + jj, D - 1) : j0 + jj) * D;
    for (int k = 0; k < D; ++k) {
        float w[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) w[jj] = wr[jj][k];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float y = (float)y0[c * ys + k];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[c][jj] = fmaf(w[jj], y, acc[c][jj]);
        }
    }
}

template <int LDSB>
__global__ __launch_bounds__(kTileThreads) void lbt_decode_kernel(const uint8_t *__restrict__ kin,
                                                                 uint8_t *__restrict__ rgb,
                                                                 const float *__restrict__ wts,
                                                                 const float *__restrict__ means, BlockGeom g, int Q,
                                                                 int sub, LbtScale pq)
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
    const float *Wf = wts + (long long)blockIdx.y * D * D;
    const float mu = means[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = kTileThreads >> 6;
    const int njg = (D + 7) >> 3, nbc = (tbv + 63) >> 6;

    // u8 -> int16 - 128 -> Q k (int16, wrapping) [-> / the -p weight, back into int16] -> block layout
    gather_indices(src, Y, ys, g, b0, tbv, sub, Q, [&pq](short y16, int c, int k) {
        if (pq.on) y16 = (short)(int)((double)y16 / pq.t[c ? 1 : 0][k]);   // :518-526
        return y16;
    });
    __syncthreads();
    for (int it = wave; it < nbc * njg; it += nw) {
        const int jg = it % njg, bc = it / njg;
        const int bl = bc * 64 + lane, j0 = jg * 8;
        const short *y0 = Y + min(bl, tbv - 1) * XS;
        float acc[3][8];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[c][jj] = 0.f;
        if (j0 + 8 <= D) lbt_synth<false>(Wf, y0, ys, D, j0, acc);
        else lbt_synth<true>(Wf, y0, ys, D, j0, acc);
        if (bl < tbv) {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int j = j0 + jj;
                if (j >= D) continue;
                const float Yv = acc[0][jj] + mu, Co = acc[1][jj] + mu, Cg = acc[2][jj] + mu;
                const float R = ((Yv + Co) - Cg) + 128.f, G = (Yv + Cg) + 128.f, Bv = ((Yv - Co) - Cg) + 128.f;
                uint8_t *o = O + bl * OS + j * 3;
                o[0] = (uint8_t)(int)fminf(fmaxf(R, 0.f), 255.f);
                o[1] = (uint8_t)(int)fminf(fmaxf(G, 0.f), 255.f);
                o[2] = (uint8_t)(int)fminf(fmaxf(Bv, 0.f), 255.f);
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
    if (B < kMinB || B > kMaxB)
        return set_error(VCF_ERR_UNSUPPORTED, "block size %d: the LBT kernels cover 2 <= B <= 8", B);
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
    if (flags & ~(VCF_DCT_NO_SUBBANDS | VCF_DCT_PERCEPTUAL)) return set_error(VCF_ERR_INVALID, "unknown flags 0x%x", flags);
    g = make_block_geom(H, W, B);
    return VCF_OK;
}

int make_scale(int32_t B, uint32_t flags, LbtScale &pq)
{
    pq.on = (flags & VCF_DCT_PERCEPTUAL) ? 1 : 0;
    for (int i = 0; i < kDP; ++i) pq.t[0][i] = pq.t[1][i] = 1.0;
    if (!pq.on) return VCF_OK;
    uint8_t ty[kDP], tc[kDP];
    const int rc = vcf_dct_perceptual_tables(B, ty, tc);
    if (rc != VCF_OK) return rc;
    for (int i = 0; i < B * B; ++i) {
        pq.t[0][i] = (double)ty[i] / 121.0;
        pq.t[1][i] = (double)tc[i] / 99.0;
    }
    return VCF_OK;
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_lbt_tile_plan(int32_t H, int32_t W, int32_t block_size, int32_t decode, int32_t *TB, int32_t *lds_class,
                      int32_t *tiles, int32_t *moment_chunks, int32_t *moment_stage_blocks)
{
    if (!TB || !lds_class || !tiles || !moment_chunks || !moment_stage_blocks)
        return set_error(VCF_ERR_INVALID, "null pointer");
    const int rc = check_shape(H, W, block_size);
    if (rc != VCF_OK) return rc;
    const BlockGeom g = make_block_geom(H, W, block_size);
    const BlockPlan p = make_block_plan(g, decode != 0, 4);
    if (p.cls < 0) return set_error(VCF_ERR_UNSUPPORTED, "block size %d: tile does not fit the LDS", block_size);
    *TB = g.TB;
    *lds_class = p.cls;
    *tiles = p.tiles;
    *moment_chunks = p.chunks;
    *moment_stage_blocks = p.tbm;
    return VCF_OK;
}

int vcf_lbt_moments(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                    double *s1_dev, double *s2_dev, void *stream)
{
    BlockGeom g;
    int rc = check_args(rgb_dev, s1_dev, s2_dev, n_frames, H, W, block_size, 1, 0, g);
    if (rc != VCF_OK) return rc;
    VCF_REQUIRE_ALIGNED(s1_dev, 8);
    VCF_REQUIRE_ALIGNED(s2_dev, 8);
    const long long D = g.D;
    rc = hip_check(hipMemsetAsync(s1_dev, 0, (size_t)(n_frames * D * 8), (hipStream_t)stream), "hipMemsetAsync(S1)");
    if (rc != VCF_OK) return rc;
    rc = hip_check(hipMemsetAsync(s2_dev, 0, (size_t)(n_frames * D * D * 8), (hipStream_t)stream), "hipMemsetAsync(S2)");
    if (rc != VCF_OK) return rc;
    const BlockPlan p = make_block_plan(g, false, 4);
    return for_frame_chunks(n_frames, "lbt_moments_kernel launch", [&](int64_t f0, unsigned nf) {
        hipLaunchKernelGGL(lbt_moments_kernel, dim3((unsigned)p.chunks, 3, nf), dim3(kMomThreads), 0, (hipStream_t)stream,
                           rgb_dev + f0 * g.rgb_stride, s1_dev + f0 * D, s2_dev + f0 * D * D, g, p.nt, p.T, p.tbm);
    });
}

int vcf_lbt_train(const double *s1_dev, const double *s2_dev, int64_t n_frames, int32_t block_size, int64_t rows,
                  int32_t epochs, double lr, double lambda, float *we_dev, float *wd_dev, float *mean_dev,
                  float *loss_dev, void *stream)
{
    if (!s1_dev || !s2_dev || !we_dev || !wd_dev || !mean_dev || !loss_dev)
        return set_error(VCF_ERR_INVALID, "null buffer");
    if (n_frames < 1) return set_error(VCF_ERR_INVALID, "n_frames < 1");
    if (block_size < kMinB || block_size > kMaxB)
        return set_error(VCF_ERR_UNSUPPORTED, "block size %d: the LBT kernels cover 2 <= B <= 8", block_size);
    if (rows < 1) return set_error(VCF_ERR_INVALID, "rows < 1");
    if (epochs < 0) return set_error(VCF_ERR_INVALID, "epochs < 0");
    if (!(lr > 0.0) || !(lambda >= 0.0)) return set_error(VCF_ERR_INVALID, "lr must be > 0 and lambda >= 0");
    const long long D = block_size * block_size;
    return for_frame_chunks(n_frames, "lbt_train_kernel launch", [&](int64_t f0, unsigned nf) {
        hipLaunchKernelGGL(lbt_train_kernel, dim3(nf), dim3(kTrainThreads), 0, (hipStream_t)stream, s1_dev + f0 * D,
                           s2_dev + f0 * D * D, we_dev + f0 * D * D, wd_dev + f0 * D * D, mean_dev + f0,
                           loss_dev + f0 * 3, (int)D, (double)rows, (int)epochs, lr, (float)lambda);
    });
}

int vcf_lbt_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const float *we_dev, const float *mean_dev, uint8_t *k_dev, void *stream)
{
    BlockGeom g;
    int rc = check_args(rgb_dev, we_dev, k_dev, n_frames, H, W, block_size, Q, flags, g);
    if (rc != VCF_OK) return rc;
    if (!mean_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(we_dev, 4);
    VCF_REQUIRE_ALIGNED(mean_dev, 4);
    LbtScale pq;
    rc = make_scale(block_size, flags, pq);
    if (rc != VCF_OK) return rc;
    const BlockPlan p = make_block_plan(g, false, 4);
    if (p.cls < 0) return set_error(VCF_ERR_UNSUPPORTED, "block size %d: tile does not fit the LDS", block_size);
    const int sub = (flags & VCF_DCT_NO_SUBBANDS) ? 0 : 1;
    const long long DD = (long long)g.D * g.D;
    return for_frame_chunks(n_frames, "lbt_encode_kernel launch", [&](int64_t f0, unsigned nf) {
        with_lds_class(p.cls, [&](auto lds) {
            hipLaunchKernelGGL((lbt_encode_kernel<decltype(lds)::value>), dim3((unsigned)p.tiles, nf), dim3(kTileThreads),
                               0, (hipStream_t)stream, rgb_dev + f0 * g.rgb_stride, k_dev + f0 * g.k_stride,
                               we_dev + f0 * DD, mean_dev + f0, g, (float)Q, sub, pq);
        });
    });
}

int vcf_lbt_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size, int32_t Q,
                      uint32_t flags, const float *wd_dev, const float *mean_dev, uint8_t *rgb_dev, void *stream)
{
    BlockGeom g;
    int rc = check_args(k_dev, wd_dev, rgb_dev, n_frames, H, W, block_size, Q, flags, g);
    if (rc != VCF_OK) return rc;
    if (!mean_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(wd_dev, 4);
    VCF_REQUIRE_ALIGNED(mean_dev, 4);
    LbtScale pq;
    rc = make_scale(block_size, flags, pq);
    if (rc != VCF_OK) return rc;
    const BlockPlan p = make_block_plan(g, true, 4);
    if (p.cls < 0) return set_error(VCF_ERR_UNSUPPORTED, "block size %d: tile does not fit the LDS", block_size);
    const int sub = (flags & VCF_DCT_NO_SUBBANDS) ? 0 : 1;
    const long long DD = (long long)g.D * g.D;
    return for_frame_chunks(n_frames, "lbt_decode_kernel launch", [&](int64_t f0, unsigned nf) {
        with_lds_class(p.cls, [&](auto lds) {
            hipLaunchKernelGGL((lbt_decode_kernel<decltype(lds)::value>), dim3((unsigned)p.tiles, nf), dim3(kTileThreads),
                               0, (hipStream_t)stream, k_dev + f0 * g.k_stride, rgb_dev + f0 * g.rgb_stride,
                               wd_dev + f0 * DD, mean_dev + f0, g, (int)Q, sub, pq);
        });
    });
}

}  // extern "C"
