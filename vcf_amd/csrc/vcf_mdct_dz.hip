// vcf_mdct_dz.hip -- the lapped 2D-MDCT codec's hot span (2D-MDCT.py encode_fn / decode_fn)
// for gfx950: u8 RGB -> u8 indices and back, one launch per batch of frames.
//
// Malvar's lapped transform: analysis block b of a line takes the 2N samples
// [(b-1)N, (b+1)N) (N = the block size, the line extended symmetrically by N
// on both sides), multiplies them by the sine window and forms N coefficients
// with the N x 2N cosine matrix; rows first, then columns, in float64 with no
// rounding in between.  Synthesis (columns first, then rows) gives every block
// back as 2N samples (dot * 2 / N, then the window) and overlap-adds them into
// a zero line: segment s of a line is the second half of block s plus the
// first half of block s + 1 (nothing for the last segment: the reference
// extends no boundary there).
//
// Kernel form: the direct 2N-term sums, fp64 FMAs.  A workgroup owns a tile of
// TY x TX blocks (segments, on decode) of one frame and walks the three
// channels.  Per channel: stage the tile and its halo of N samples per side in
// LDS, first pass into an LDS float64 image, second pass from it -- the
// float64 intermediate never leaves the CU.  Each wave takes work items that
// fix 8 consecutive output coefficients and spreads its 64 lanes over the
// lines of the tile, so the cosine rows and the window are wave-uniform
// (scalar loads from the table in global memory, no LDS or VGPR traffic for
// them) and each LDS sample read feeds 8 (decode: 16) FMAs.  The u8 results
// of the three channels are collected in LDS and written in contiguous runs.
//
// Rounding contract ("2D-MDCT"): tables are computed in float64 on
// the host with the reference's expression order; window product first, then
// the sum; on synthesis * 2 / N, then the window, then the add.  The float32
// steps (scale, -p weights, deadzone division, YCoCg, +128) are single
// correctly rounded operations; the build's -ffp-contract=off keeps them
// apart.  Inside the float64 sums the order is n (k) ascending with FMAs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#include "vcf_amd.h"
#include "vcf_internal.h"

namespace vcf {
namespace {

constexpr int kThreads = 512;
constexpr int kMinB = 2, kMaxB = 64;

struct MdctGeom {
    int H, W, Hp, Wp, top, left;
    int N, NP;          // block size; N rounded up to 8 (row length of the analysis table)
    int nbx, nby;       // blocks per row / column of the padded frame
    int TX, TY;         // tile, in blocks (encode) or segments (decode)
    int tiles_x, tiles_y;
    int sx_lo, sy_lo, nsx, nsy;   // decode: first segment and number of segments that meet the crop
    long long rgb_stride, k_stride;
};

// table layout (doubles): win[WN] | analysis cos, n-major [2N][NP] | synthesis cos, k-major [N][ND]
__host__ __device__ inline int tab_wn(int N) { return (2 * N + 7) / 8 * 8; }
__host__ __device__ inline int tab_np(int N) { return (N + 7) / 8 * 8; }
__host__ __device__ inline int tab_nd(int N) { return 2 * N + 8; }

// JPEG luminance / chrominance tables of -p (B = 8); weight = QSS / max in float32
__constant__ uint8_t c_y_qss[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                    14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                    18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__constant__ uint8_t c_c_qss[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// a / b in float32, correctly rounded (the double quotient of two floats rounds to it)
__device__ inline float fdiv(float a, float b) { return (float)((double)a / (double)b); }

__device__ inline float pweight(int c, int ky, int kx)
{
    return c == 0 ? fdiv((float)c_y_qss[ky * 8 + kx], 121.0f) : fdiv((float)c_c_qss[ky * 8 + kx], 99.0f);
}

// index into a line of L samples extended symmetrically by at most L on each side
__device__ inline int ext_index(int i, int L) { return i < 0 ? -1 - i : (i >= L ? 2 * L - 1 - i : i); }

// padded position p -> source index in [0, n): np.pad(mode='symmetric'), reflecting as often as needed
__device__ inline int pad_index(int p, int pad, int n)
{
    int m = (p - pad) % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

__device__ inline int align16(int x) { return (x + 15) & ~15; }

// ---------------------------------------------------------------------------
// encode
// ---------------------------------------------------------------------------
template <int LDSB>
__global__ __launch_bounds__(kThreads) void mdct_encode_kernel(const uint8_t *__restrict__ rgb,
                                                              uint8_t *__restrict__ kout,
                                                              const double *__restrict__ tab, MdctGeom g,
                                                              float scale, float Qf, int sub, int perc)
{
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDSB];
    const int N = g.N, NP = g.NP;
    const int SS = ((g.TX + 1) * N) | 1;   // odd strides: lanes that walk rows hit distinct banks
    const int TS = (g.TX * N) | 1;
    const int OW = g.TX * N;
    float *S = reinterpret_cast<float *>(smem);
    double *T = reinterpret_cast<double *>(smem + align16((g.TY + 1) * N * SS * 4));
    uint8_t *O = reinterpret_cast<uint8_t *>(T) + align16((g.TY + 1) * N * TS * 8);
    const double *win = tab;
    const double *cosA = tab + tab_wn(N);

    const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
    const int by0 = tyi * g.TY, bx0 = txi * g.TX;
    const int tyv = min(g.TY, g.nby - by0), txv = min(g.TX, g.nbx - bx0);
    const int rows = (tyv + 1) * N, cols = (txv + 1) * N;
    const uint8_t *src = rgb + (long long)blockIdx.y * g.rgb_stride;
    uint8_t *dst = kout + (long long)blockIdx.y * g.k_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = kThreads >> 6;
    const int ng = NP / 8;

    for (int c = 0; c < 3; ++c) {
        // the tile and its halo: pad (centred, symmetric), -128, YCoCg; every value is a multiple of 1/4
        for (int e = tid; e < rows * cols; e += kThreads) {
            const int r = e / cols, x = e - r * cols;
            const int sy = pad_index(ext_index((by0 - 1) * N + r, g.Hp), g.top, g.H);
            const int sx = pad_index(ext_index((bx0 - 1) * N + x, g.Wp), g.left, g.W);
            const uint8_t *p = src + ((long long)sy * g.W + sx) * 3;
            const float R = (float)p[0] - 128.0f, G = (float)p[1] - 128.0f, B = (float)p[2] - 128.0f;
            float v;
            if (c == 0) v = R / 4 + G / 2 + B / 4;
            else if (c == 1) v = R / 2 - B / 2;
            else v = -R / 4 + G / 2 - B / 4;
            S[r * SS + x] = v;
        }
        __syncthreads();
        // rows: T[r][bxl N + k] = sum_n cos[k][n] (S[r][bxl N + n] win[n]); lanes over r
        {
            const int rch = (rows + 63) >> 6, items = txv * ng * rch;
            for (int it = wave; it < items; it += nw) {
                const int rc = it % rch, t = it / rch, gk = t % ng, bxl = t / ng;
                const int r = rc * 64 + lane;
                const float *sp = S + min(r, rows - 1) * SS + bxl * N;
                const double *ct = cosA + gk * 8;
                double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
                for (int n = 0; n < 2 * N; ++n) {
                    const double xw = (double)sp[n] * win[n];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fma(ct[n * NP + j], xw, acc[j]);
                }
                if (r < rows) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (gk * 8 + j < N) T[r * TS + bxl * N + gk * 8 + j] = acc[j];
                }
            }
        }
        __syncthreads();
        // columns, then float32, scale, -p, deadzone, +128, clip; lanes over x
        {
            const int xw_ = txv * N, xch = (xw_ + 63) >> 6, items = tyv * ng * xch;
            for (int it = wave; it < items; it += nw) {
                const int xc = it % xch, t = it / xch, gk = t % ng, byl = t / ng;
                const int x = xc * 64 + lane;
                const double *tp = T + byl * N * TS + min(x, xw_ - 1);
                const double *ct = cosA + gk * 8;
                double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 2
                for (int n = 0; n < 2 * N; ++n) {
                    const double tw = tp[n * TS] * win[n];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fma(ct[n * NP + j], tw, acc[j]);
                }
                if (x < xw_) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = gk * 8 + j;
                        if (k >= N) continue;
                        float f = fdiv((float)acc[j], scale);
                        if (perc) f = f * pweight(c, k, x & 7);
                        const int q = (int)fdiv(f, Qf) + 128;
                        O[((byl * N + k) * OW + x) * 3 + c] = (uint8_t)min(max(q, 0), 255);
                    }
                }
            }
        }
        // no barrier here: the next channel's staging writes S only (last read before the barrier
        // above), and T is written again only after the barrier that follows the staging
    }
    __syncthreads();
    const int run = txv * N * 3;
    if (!sub) {
        for (int e = tid; e < tyv * N * run; e += kThreads) {
            const int r = e / run, q = e - r * run;
            dst[((long long)(by0 * N + r) * g.Wp + bx0 * N) * 3 + q] = O[r * OW * 3 + q];
        }
    } else {
        // subband (ky, kx) holds coefficient (ky, kx) of every block: runs of txv * 3 bytes
        for (int e = tid; e < tyv * N * run; e += kThreads) {
            const int c = e % 3;
            int t = e / 3;
            const int bxl = t % txv;
            t /= txv;
            const int kx = t % N;
            t /= N;
            const int byl = t % tyv, ky = t / tyv;
            dst[((long long)(ky * g.nby + by0 + byl) * g.Wp + kx * g.nbx + bx0 + bxl) * 3 + c] =
                O[((byl * N + ky) * OW + bxl * N + kx) * 3 + c];
        }
    }
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
template <int LDSB, bool PERC>
__global__ __launch_bounds__(kThreads) void mdct_decode_kernel(const uint8_t *__restrict__ kin,
                                                              uint8_t *__restrict__ rgb,
                                                              const double *__restrict__ tab, MdctGeom g,
                                                              float scale, int Q, int sub, int pow2)
{
    typedef typename std::conditional<PERC, float, int16_t>::type DT;   // dequantized coefficients
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDSB];
    const int N = g.N, NP = g.NP, ND = tab_nd(N);
    const int DS = ((g.TX + 1) * N) | 1, US = DS;
    const int PW = g.TX * N, PH = g.TY * N;
    DT *D = reinterpret_cast<DT *>(smem);
    double *U = reinterpret_cast<double *>(smem + align16((g.TY + 1) * N * DS * (int)sizeof(DT)));
    float *P = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(U) + align16(PH * US * 8));
    const double *win = tab;
    const double *cosS = tab + tab_wn(N) + 2 * N * NP;
    const double Nd = (double)N, inv = 2.0 / Nd;

    const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
    const int sy0 = g.sy_lo + tyi * g.TY, sx0 = g.sx_lo + txi * g.TX;
    const int tyv = min(g.TY, g.sy_lo + g.nsy - sy0), txv = min(g.TX, g.sx_lo + g.nsx - sx0);
    const int cby = min(tyv + 1, g.nby - sy0), cbx = min(txv + 1, g.nbx - sx0);   // coefficient blocks read
    const uint8_t *src = kin + (long long)blockIdx.y * g.k_stride;
    uint8_t *dst = rgb + (long long)blockIdx.y * g.rgb_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = kThreads >> 6;
    const int ng = NP / 8;

    for (int c = 0; c < 3; ++c) {
        // u8 -> int16 - 128 -> Q k (int16, wrapping) -> block layout -> -p
        {
            const int rows = cby * N, cols = cbx * N;
            for (int e = tid; e < rows * cols; e += kThreads) {
                const int r = e / cols, x = e - r * cols;
                const int byl = r / N, ky = r - byl * N, bxl = x / N, kx = x - bxl * N;
                const int by = sy0 + byl, bx = sx0 + bxl;
                const long long at = sub ? ((long long)(ky * g.nby + by) * g.Wp + kx * g.nbx + bx)
                                         : ((long long)(by * N + ky) * g.Wp + bx * N + kx);
                const int16_t y = (int16_t)(Q * ((int)src[at * 3 + c] - 128));
                if constexpr (PERC) D[r * DS + x] = fdiv((float)y, pweight(c, ky, kx));
                else D[r * DS + x] = y;
            }
        }
        __syncthreads();
        // columns: U[sl N + m][X] = (dot(block sl)[N + m] 2 / N) win[N + m] + (dot(block sl + 1)[m] 2 / N) win[m]
        {
            const int cols = cbx * N, xch = (cols + 63) >> 6, items = tyv * ng * xch;
            for (int it = wave; it < items; it += nw) {
                const int xc = it % xch, t = it / xch, gm = t % ng, sl = t / ng;
                const int X = xc * 64 + lane;
                const bool two = sl + 1 < cby;
                const DT *d1 = D + sl * N * DS + min(X, cols - 1);
                const DT *d2 = two ? d1 + N * DS : d1;
                const double *cd = cosS + gm * 8;
                double a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int k = 0; k < N; ++k) {
                    const double v1 = (double)d1[k * DS], v2 = (double)d2[k * DS];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        a[j] = __builtin_fma(cd[k * ND + N + j], v1, a[j]);
                        b[j] = __builtin_fma(cd[k * ND + j], v2, b[j]);
                    }
                }
                if (X < cols) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int m = gm * 8 + j;
                        if (m >= N) continue;
                        double v = (pow2 ? a[j] * inv : a[j] * 2.0 / Nd) * win[N + m];
                        if (two) v = v + (pow2 ? b[j] * inv : b[j] * 2.0 / Nd) * win[m];
                        U[(sl * N + m) * US + X] = v;
                    }
                }
            }
        }
        __syncthreads();
        // rows, then float32 and * scale; lanes over the tile's rows
        {
            const int rows = tyv * N, ich = (rows + 63) >> 6, items = txv * ng * ich;
            for (int it = wave; it < items; it += nw) {
                const int ic = it % ich, t = it / ich, gm = t % ng, sxl = t / ng;
                const int i = ic * 64 + lane;
                const bool two = sxl + 1 < cbx;
                const double *u1 = U + min(i, rows - 1) * US + sxl * N;
                const double *u2 = two ? u1 + N : u1;
                const double *cd = cosS + gm * 8;
                double a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int k = 0; k < N; ++k) {
                    const double v1 = u1[k], v2 = u2[k];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        a[j] = __builtin_fma(cd[k * ND + N + j], v1, a[j]);
                        b[j] = __builtin_fma(cd[k * ND + j], v2, b[j]);
                    }
                }
                if (i < rows) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int m = gm * 8 + j;
                        if (m >= N) continue;
                        double v = (pow2 ? a[j] * inv : a[j] * 2.0 / Nd) * win[N + m];
                        if (two) v = v + (pow2 ? b[j] * inv : b[j] * 2.0 / Nd) * win[m];
                        P[(c * PH + i) * PW + sxl * N + m] = (float)v * scale;
                    }
                }
            }
        }
        // no barrier here: D was last read before the barrier above, U is written again only after the next one
    }
    __syncthreads();
    // to_RGB in float32, crop, +128, clip, truncate
    for (int e = tid; e < tyv * N * txv * N; e += kThreads) {
        const int i = e / (txv * N), x = e - i * (txv * N);
        const int gy = sy0 * N + i - g.top, gx = sx0 * N + x - g.left;
        if (gy < 0 || gy >= g.H || gx < 0 || gx >= g.W) continue;
        const float Y = P[i * PW + x], Co = P[(PH + i) * PW + x], Cg = P[(2 * PH + i) * PW + x];
        const float R = (Y + Co) - Cg + 128.0f, G = (Y + Cg) + 128.0f, B = (Y - Co) - Cg + 128.0f;
        uint8_t *p = dst + ((long long)gy * g.W + gx) * 3;
        p[0] = (uint8_t)(int)fminf(fmaxf(R, 0.0f), 255.0f);
        p[1] = (uint8_t)(int)fminf(fmaxf(G, 0.0f), 255.0f);
        p[2] = (uint8_t)(int)fminf(fmaxf(B, 0.0f), 255.0f);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int kLds[3] = {40 * 1024, 80 * 1024, 156 * 1024};   // 4, 2, 1 workgroups per CU (160 KiB LDS)

long long enc_lds(int N, int TX, int TY)
{
    const long long SS = ((TX + 1) * N) | 1, TS = (TX * N) | 1;
    auto a16 = [](long long x) { return (x + 15) & ~15LL; };
    return a16((TY + 1) * N * SS * 4) + a16((TY + 1) * N * TS * 8) + (long long)TY * N * TX * N * 3;
}

long long dec_lds(int N, int TX, int TY, bool perc)
{
    const long long DS = ((TX + 1) * N) | 1;
    auto a16 = [](long long x) { return (x + 15) & ~15LL; };
    return a16((TY + 1) * N * DS * (perc ? 4 : 2)) + a16((long long)TY * N * DS * 8) + 3LL * TY * N * TX * N * 4;
}

// The tile that wastes least: halo work (TY + 1) / TY or (TX + 1) / TX on the first pass, idle lanes
// when a pass's line count is no multiple of 64, fewer workgroups per CU for more LDS.  lx / ly:
// which pass spreads its lanes over which extent (in units of N): encode rows over (TY + 1), columns
// over TX; decode columns over (TX + 1), rows over TY.
void pick_tile(int N, int ext_x, int ext_y, bool decode, bool perc, int &TX, int &TY, int &lds_class)
{
    double best = -1;
    TX = TY = 1;
    lds_class = 2;
    for (int ty = 1; ty <= std::min(ext_y, 32); ++ty)
        for (int tx = 1; tx <= std::min(ext_x, 64); ++tx) {
            const long long lds = decode ? dec_lds(N, tx, ty, perc) : enc_lds(N, tx, ty);
            if (lds > kLds[2]) break;
            const int cls = lds <= kLds[0] ? 0 : (lds <= kLds[1] ? 1 : 2);
            const int l1 = (decode ? tx + 1 : ty + 1) * N, l2 = (decode ? ty : tx) * N;
            const double u1 = (double)l1 / ((l1 + 63) / 64 * 64), u2 = (double)l2 / ((l2 + 63) / 64 * 64);
            const double halo1 = decode ? (double)tx / (tx + 1) : (double)ty / (ty + 1);
            // cost per useful coefficient: first pass (with halo) + second pass
            const double eff = 2.0 / (1.0 / (u1 * halo1) + 1.0 / u2);
            // covering the extent with whole tiles
            const double cover = ((double)ext_x / ((ext_x + tx - 1) / tx * tx)) * ((double)ext_y / ((ext_y + ty - 1) / ty * ty));
            const double occ = cls == 0 ? 1.0 : (cls == 1 ? 0.95 : 0.8);
            const double score = eff * cover * occ;
            if (score > best) {
                best = score;
                TX = tx;
                TY = ty;
                lds_class = cls;
            }
        }
}

void make_geom(int32_t H, int32_t W, int32_t B, MdctGeom &g)
{
    g.H = H;
    g.W = W;
    g.N = B;
    g.NP = tab_np(B);
    g.Hp = (H + 2 * B + B - 1) / B * B;
    g.Wp = (W + 2 * B + B - 1) / B * B;
    g.top = (g.Hp - H) / 2;
    g.left = (g.Wp - W) / 2;
    g.nbx = g.Wp / B;
    g.nby = g.Hp / B;
    g.sy_lo = g.top / B;
    g.sx_lo = g.left / B;
    g.nsy = (g.top + H - 1) / B - g.sy_lo + 1;
    g.nsx = (g.left + W - 1) / B - g.sx_lo + 1;
    g.rgb_stride = (long long)H * W * 3;
    g.k_stride = (long long)g.Hp * g.Wp * 3;
}

// the tile and LDS class of one launch: over the blocks on encode, over the segments that meet the
// crop on decode
int plan_tiles(MdctGeom &g, bool decode, bool perc)
{
    int cls;
    const int ext_x = decode ? g.nsx : g.nbx, ext_y = decode ? g.nsy : g.nby;
    pick_tile(g.N, ext_x, ext_y, decode, perc, g.TX, g.TY, cls);
    g.tiles_x = (ext_x + g.TX - 1) / g.TX;
    g.tiles_y = (ext_y + g.TY - 1) / g.TY;
    return cls;
}

float scale_factor(int B)
{
    // 2D-MDCT.py:412-421, computed in double as there, used as float32
    if (B <= 8) return (float)((double)B / 2.0);
    if (B >= 32) return (float)((double)B / 4.0);
    const double t = (double)(B - 8) / (32 - 8);
    return (float)(4.0 + t * (8.0 - 4.0));
}

std::mutex g_tab_mu;
double *g_tab[64][kMaxB + 1] = {};

// window and cosine tables of block size N, uploaded once per device
int device_tables(int N, const double *&tab)
{
    int dev = 0;
    int rc = hip_check(hipGetDevice(&dev), "hipGetDevice");
    if (rc != VCF_OK) return rc;
    if (dev < 0 || dev >= 64) return set_error(VCF_ERR_INVALID, "device %d", dev);
    std::lock_guard<std::mutex> lk(g_tab_mu);
    double *&p = g_tab[dev][N];
    if (!p) {
        const int WN = tab_wn(N), NP = tab_np(N), ND = tab_nd(N);
        std::vector<double> h((size_t)WN + 2 * N * NP + N * ND, 0.0);
        const double n0 = (N + 1) / 2.0;
        for (int n = 0; n < 2 * N; ++n) h[n] = std::sin(M_PI * (n + 0.5) / (2 * N));
        for (int n = 0; n < 2 * N; ++n)
            for (int k = 0; k < N; ++k) {
                const double v = std::cos(M_PI / N * (n + n0) * (k + 0.5));
                h[(size_t)WN + n * NP + k] = v;
                h[(size_t)WN + 2 * N * NP + k * ND + n] = v;
            }
        rc = hip_check(hipMalloc((void **)&p, h.size() * sizeof(double)), "hipMalloc(mdct tables)");
        if (rc != VCF_OK) return rc;
        rc = hip_check(hipMemcpy(p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice), "mdct tables upload");
        if (rc != VCF_OK) {
            (void)hipFree(p);
            p = nullptr;
            return rc;
        }
    }
    tab = p;
    return VCF_OK;
}

// what the host-only queries accept
int check_shape(int32_t H, int32_t W, int32_t B)
{
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad shape %d x %d", H, W);
    if (B < kMinB || B > kMaxB)
        return set_error(VCF_ERR_UNSUPPORTED, "block size %d: the MDCT kernels cover 2 <= B <= 64", B);
    if ((long long)H + 3LL * B > INT32_MAX || (long long)W + 3LL * B > INT32_MAX)
        return set_error(VCF_ERR_INVALID, "bad shape %d x %d", H, W);
    return VCF_OK;
}

int check_args(const void *a, const void *b, int64_t n_frames, int32_t H, int32_t W, int32_t B, int32_t Q,
               uint32_t flags)
{
    if (!a || !b) return set_error(VCF_ERR_INVALID, "null buffer");
    if (n_frames < 0) return set_error(VCF_ERR_INVALID, "n_frames < 0");
    if (H <= 0 || W <= 0)
        return set_error(VCF_ERR_INVALID, "Input image must be a 3D array (height, width, channels).");
    if (B < kMinB || B > kMaxB)
        return set_error(VCF_ERR_UNSUPPORTED, "block size %d: the MDCT kernels cover 2 <= B <= 64", B);
    if (Q < 1 || Q > 32767) return set_error(VCF_ERR_INVALID, "quantization step %d out of range", Q);
    if (flags & ~(VCF_DCT_NO_SUBBANDS | VCF_DCT_PERCEPTUAL))
        return set_error(VCF_ERR_INVALID, "unknown flags 0x%x", flags);
    if ((flags & VCF_DCT_PERCEPTUAL) && B != 8)
        return set_error(VCF_ERR_UNSUPPORTED, "perceptual quantization with block size %d: only B = 8 is pinned", B);
    // the kernels address within a frame with 32-bit block arithmetic
    if (((long long)H + 3 * B) * ((long long)W + 3 * B) * 3 >= (1LL << 31))
        return set_error(VCF_ERR_INVALID, "frame too large");
    return VCF_OK;
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_mdct_padded_shape(int32_t H, int32_t W, int32_t block_size, int32_t *Hp, int32_t *Wp, int32_t *pad_top,
                          int32_t *pad_left)
{
    if (!Hp || !Wp || !pad_top || !pad_left) return set_error(VCF_ERR_INVALID, "null pointer");
    const int rc = check_shape(H, W, block_size);
    if (rc != VCF_OK) return rc;
    MdctGeom g;
    make_geom(H, W, block_size, g);
    *Hp = g.Hp;
    *Wp = g.Wp;
    *pad_top = g.top;
    *pad_left = g.left;
    return VCF_OK;
}

int vcf_mdct_tile_plan(int32_t H, int32_t W, int32_t block_size, uint32_t flags, int32_t decode, int32_t *TX,
                       int32_t *TY, int32_t *lds_class, int32_t *tiles_x, int32_t *tiles_y)
{
    if (!TX || !TY || !lds_class || !tiles_x || !tiles_y) return set_error(VCF_ERR_INVALID, "null pointer");
    // no buffers, one frame, Q = 1: the shape, block size and flag rules of the launches
    int rc = check_shape(H, W, block_size);
    if (rc == VCF_OK) rc = check_args(&rc, &rc, 1, H, W, block_size, 1, flags);
    if (rc != VCF_OK) return rc;
    MdctGeom g;
    make_geom(H, W, block_size, g);
    *lds_class = plan_tiles(g, decode != 0, decode != 0 && (flags & VCF_DCT_PERCEPTUAL) != 0);
    *TX = g.TX;
    *TY = g.TY;
    *tiles_x = g.tiles_x;
    *tiles_y = g.tiles_y;
    return VCF_OK;
}

int vcf_mdct_dz_encode(const uint8_t *rgb_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                       int32_t Q, uint32_t flags, uint8_t *k_dev, void *stream)
{
    int rc = check_args(rgb_dev, k_dev, n_frames, H, W, block_size, Q, flags);
    if (rc != VCF_OK) return rc;
    if (n_frames == 0) return VCF_OK;
    MdctGeom g;
    make_geom(H, W, block_size, g);
    const int cls = plan_tiles(g, false, false);
    const double *tab = nullptr;
    if ((rc = device_tables(g.N, tab)) != VCF_OK) return rc;
    const float scale = scale_factor(g.N);
    const int sub = (flags & VCF_DCT_NO_SUBBANDS) ? 0 : 1, perc = (flags & VCF_DCT_PERCEPTUAL) ? 1 : 0;
    return for_frame_chunks(n_frames, "mdct_encode_kernel launch", [&](int64_t f0, unsigned nf) {
        const dim3 grid(g.tiles_x * g.tiles_y, nf);
        const uint8_t *in = rgb_dev + f0 * g.rgb_stride;
        uint8_t *out = k_dev + f0 * g.k_stride;
#define VCF_MDCT_ENC(C)                                                                                          \
        hipLaunchKernelGGL((mdct_encode_kernel<kLds[C]>), grid, dim3(kThreads), 0, (hipStream_t)stream, in, out, \
                           tab, g, scale, (float)Q, sub, perc)
        if (cls == 0) VCF_MDCT_ENC(0);
        else if (cls == 1) VCF_MDCT_ENC(1);
        else VCF_MDCT_ENC(2);
#undef VCF_MDCT_ENC
    });
}

int vcf_mdct_dz_decode(const uint8_t *k_dev, int64_t n_frames, int32_t H, int32_t W, int32_t block_size,
                       int32_t Q, uint32_t flags, uint8_t *rgb_dev, void *stream)
{
    int rc = check_args(k_dev, rgb_dev, n_frames, H, W, block_size, Q, flags);
    if (rc != VCF_OK) return rc;
    if (n_frames == 0) return VCF_OK;
    MdctGeom g;
    make_geom(H, W, block_size, g);
    const bool perc = (flags & VCF_DCT_PERCEPTUAL) != 0;
    const int cls = plan_tiles(g, true, perc);
    const double *tab = nullptr;
    if ((rc = device_tables(g.N, tab)) != VCF_OK) return rc;
    const float scale = scale_factor(g.N);
    const int sub = (flags & VCF_DCT_NO_SUBBANDS) ? 0 : 1, pow2 = (g.N & (g.N - 1)) == 0 ? 1 : 0;
    return for_frame_chunks(n_frames, "mdct_decode_kernel launch", [&](int64_t f0, unsigned nf) {
        const dim3 grid(g.tiles_x * g.tiles_y, nf);
        const uint8_t *in = k_dev + f0 * g.k_stride;
        uint8_t *out = rgb_dev + f0 * g.rgb_stride;
#define VCF_MDCT_DEC(C, PC)                                                                                      \
        hipLaunchKernelGGL((mdct_decode_kernel<kLds[C], PC>), grid, dim3(kThreads), 0, (hipStream_t)stream, in,  \
                           out, tab, g, scale, (int)Q, sub, pow2)
        if (perc) {
            if (cls == 0) VCF_MDCT_DEC(0, true);
            else if (cls == 1) VCF_MDCT_DEC(1, true);
            else VCF_MDCT_DEC(2, true);
        } else {
            if (cls == 0) VCF_MDCT_DEC(0, false);
            else if (cls == 1) VCF_MDCT_DEC(1, false);
            else VCF_MDCT_DEC(2, false);
        }
#undef VCF_MDCT_DEC
    });
}

}  // extern "C"
