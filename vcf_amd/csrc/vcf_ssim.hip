// vcf_ssim.hip -- the integer-window SSIM of two sets of u8 frames, per frame and channel, as an
// exact integer sum: every intermediate is an exact integer or one correctly rounded float64
// operation, so the records equal a numpy restatement bit for bit and depend on no launch geometry
// and on no order of the atomics.  The arithmetic is stated in include/vcf_amd.h (vcf_ssim_u8) and
// in DESIGN.md §4.15.
//
// Bounds, for u8 input (tests/test_ssim.py asserts them on the extreme inputs):
//   one axis of the window sums 256, both axes S = 2^16;
//   row sums:    A, B <= 255 * 256 = 65 280 (16 bits);  XX, YY, XY <= 65025 * 256 = 16 646 400 (24 bits);
//   window sums: A, B <= 255 * 2^16 (24 bits);  XX, YY, XY <= 65025 * 2^16 = 4 261 478 400: that
//                fits uint32 and not int32, so the planes and the sums are unsigned;
//   factors:     A B, A^2 <= 255^2 * 2^32 < 2^48;  S XX <= 65025 * 2^32 < 2^48;  S (XX + YY) < 2^49;
//                with C2 < 2^38 every factor is below 2^50 in magnitude, so int64 -> double is exact.
//                An axis sum of 2^9 would put S (XX + YY) at 2^53: that is why it is 2^8.
//   q in [-1, 1] (2 A B <= A^2 + B^2, and |S XY - A B| <= ((S XX - A^2) + (S YY - B^2)) / 2 by
//                Cauchy-Schwarz; rounding is monotone), so k = rint(q * 2^30) fits int32.
//
// One workgroup takes a tile of kT x kT windows of one frame, all channels.  The outer taps of the
// 11-tap window are 0, so a window at (y, x) reads pixels (y + 1 .. y + 9, x + 1 .. x + 9): the
// tile needs (kT + 8)^2 pixels, not (kT + 10)^2.
//   1. Staging: the (kT + 8) rows of (kT + 8) * C bytes of both frames go to LDS in 16-byte pieces
//      cut at the 16-byte boundaries of the global address (frames, rows and tiles start at any
//      byte, W * C being arbitrary): a piece wholly inside the frame is one 16-byte load, any other
//      is read bytewise with every byte outside the frame taken as 0.  Nothing outside a frame is
//      read.  Bytes of a piece beyond the tile's columns are the row's next pixels or the next
//      row's first ones; no window that counts uses them.
//   2. Horizontal pass, once per staged row: a lane takes four neighbouring pixels of one channel,
//      reads their twelve inputs of x and of y, forms x^2, y^2 and x y once per input, and writes
//      four entries {A | B << 16, XX, YY, XY} of the row-sum planes (one uint4 per row and byte
//      column).  A and B go through one packed 16-bit multiply-add; the other three are 24-bit ones.
//   3. Vertical pass: lane (px, rg) takes pixel column px and rows rg, rg + 8, ... of the tile, so
//      the channel is a compile-time constant of the inner loop; nine 16-byte LDS reads (lanes of a
//      wave read consecutive pixels: a stride of C entries, conflict-free for C = 1 and 3) and 45
//      24-bit multiply-adds give the five window sums, then the factors in int64, two double
//      products, one double division (hipcc's `/` on double is the correctly rounded sequence; the
//      library is built without fast-math and with -ffp-contract=off, and no sum follows a product
//      here anyway), rint, and the lane's int64 sum and int32 minimum per channel.
// Wave reduction by shuffles, the four waves through LDS, then one 64-bit integer atomic add and
// one 64-bit signed atomic min per workgroup and channel.  A kernel before it sets the records
// (sum 0, the window count, min INT64_MAX).
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
constexpr int kT = 32;                  // tile edge in windows
constexpr int kS = kT + 8;              // staged rows, and staged pixels per row
constexpr int kTaps = 9;                // the non-zero taps: offsets 1..9 of the 11-tap window
constexpr int kGroup = 4;               // horizontal pass: neighbouring outputs per lane
constexpr int kRowGroups = kThreads / kT;
constexpr int64_t kC1 = 27928024842LL;  // round(6.5025 * 2^32)
constexpr int64_t kC2 = 251352223580LL; // round(58.5225 * 2^32)

static_assert(sizeof(vcf_ssim_record) == 24, "record layout is part of the ABI");
static_assert(VCF_SSIM_WINDOW == kTaps + 2, "two zero taps around nine");
static_assert(kThreads % kT == 0 && kT % kRowGroups == 0 && kT % kGroup == 0, "tile and workgroup shapes");

__host__ __device__ __forceinline__ constexpr uint32_t tap(int t)
{
    constexpr uint32_t w[kTaps] = {2, 9, 28, 55, 68, 55, 28, 9, 2};
    return w[t];
}
static_assert(2 * (tap(0) + tap(1) + tap(2) + tap(3)) + tap(4) == 256, "an axis sums 2^8");

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

template <int C>
struct Geo {
    static constexpr int kRowBytes = kS * C;                    // a staged row of the tile
    static constexpr int kChunks = (kRowBytes + 15 + 15) / 16;  // 16-byte pieces covering it from any of 16 offsets
    static constexpr int kStride = kChunks * 16;                // LDS bytes per staged row
    static constexpr int kCols = kT * C;                        // byte columns of the planes
};

// a * b + acc for a < 2^24, b < 2^24
__device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t acc) { return (uint32_t)__umul24(a, b) + acc; }

// kS rows of a frame of F bytes into dst (kS rows of Geo::kStride bytes): row r starts `first + r * pitch` bytes into
// the frame, and its first byte lands at dst[r * kStride + lead], lead = its global address mod 16 (row_lead below).
template <int C>
__device__ __forceinline__ void stage(const uint8_t *__restrict__ fr, int64_t F, int64_t first, int64_t pitch,
                                      uint4 *__restrict__ dst, int tid)
{
    using G = Geo<C>;
    const uintptr_t base = reinterpret_cast<uintptr_t>(fr);
    for (int it = tid; it < kS * G::kChunks; it += kThreads) {
        const int r = it / G::kChunks, ch = it % G::kChunks;
        const int64_t row = first + r * pitch;                         // offset of the row's first byte in the frame
        const int64_t off = row - (int64_t)((base + (uintptr_t)row) & 15) + 16 * ch;   // 16-byte aligned address
        uint4 v;
        if (off >= 0 && off + 16 <= F) {
            v = *reinterpret_cast<const uint4 *>(fr + off);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t o = off + 4 * i + j;
                    if (o >= 0 && o < F) w[i] |= (uint32_t)fr[o] << (8 * j);
                }
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        dst[r * G::kChunks + ch] = v;
    }
}

__device__ __forceinline__ int row_lead(const uint8_t *fr, int64_t first, int64_t pitch, int r)
{
    return (int)((reinterpret_cast<uintptr_t>(fr) + (uintptr_t)(first + r * pitch)) & 15);
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int32_t wave_min(int32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ void ssim_init_kernel(vcf_ssim_record *__restrict__ out, int64_t n_records, uint64_t windows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_records) {
        out[i].sum_k = 0;
        out[i].windows = windows;
        out[i].min_k = INT64_MAX;
    }
}

// grid: x = tile (tiles_x * tiles_y of them, row-major), y = frame f0 + y
template <int C>
__global__ __launch_bounds__(kThreads) void ssim_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                        int64_t F, int64_t f0, int32_t H, int32_t W, int32_t tiles_x,
                                                        vcf_ssim_record *__restrict__ out)
{
    using G = Geo<C>;
    __shared__ uint4 planes[kS * G::kCols];
    __shared__ uint4 staged[2][kS * G::kChunks];
    __shared__ int64_t red_sum[kWaves][C];
    __shared__ int32_t red_min[kWaves][C];

    const int tid = threadIdx.x;
    const int64_t f = f0 + blockIdx.y;
    const uint8_t *af = a + f * F, *bf = b + f * F;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kT, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kT;
    const int64_t pitch = (int64_t)W * C;
    const int64_t first = ((int64_t)(y0 + 1) * W + (x0 + 1)) * C;      // pixel (y0 + 1, x0 + 1): the first non-zero tap

    stage<C>(af, F, first, pitch, staged[0], tid);
    stage<C>(bf, F, first, pitch, staged[1], tid);
    __syncthreads();

    // horizontal pass: item = (row r, group g of kGroup pixels, channel c), c fastest
    const uint8_t *sa = reinterpret_cast<const uint8_t *>(staged[0]), *sb = reinterpret_cast<const uint8_t *>(staged[1]);
    for (int it = tid; it < kS * (kT / kGroup) * C; it += kThreads) {
        const int c = it % C, g = (it / C) % (kT / kGroup), r = it / (C * (kT / kGroup));
        // staged pixels g * kGroup .. g * kGroup + kGroup + kTaps - 2 (at most kS - 1), channel c
        const uint8_t *pa = sa + r * G::kStride + row_lead(af, first, pitch, r) + g * kGroup * C + c;
        const uint8_t *pb = sb + r * G::kStride + row_lead(bf, first, pitch, r) + g * kGroup * C + c;
        us2 xy[kGroup + kTaps - 1];
        uint32_t xx[kGroup + kTaps - 1], yy[kGroup + kTaps - 1], xyp[kGroup + kTaps - 1];
#pragma unroll
        for (int j = 0; j < kGroup + kTaps - 1; ++j) {
            const uint32_t x = pa[j * C], y = pb[j * C];
            xy[j] = us2{(unsigned short)x, (unsigned short)y};
            xx[j] = x * x;
            yy[j] = y * y;
            xyp[j] = x * y;
        }
#pragma unroll
        for (int u = 0; u < kGroup; ++u) {
            us2 ab = us2{0, 0};                                         // A and B: at most 65 280 each
            uint32_t sxx = 0, syy = 0, sxy = 0;                         // at most 16 646 400 < 2^24
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                ab += us2{(unsigned short)tap(t), (unsigned short)tap(t)} * xy[u + t];
                sxx = mad24(tap(t), xx[u + t], sxx);
                syy = mad24(tap(t), yy[u + t], syy);
                sxy = mad24(tap(t), xyp[u + t], sxy);
            }
            planes[r * G::kCols + (g * kGroup + u) * C + c] = make_uint4(__builtin_bit_cast(uint32_t, ab), sxx, syy, sxy);
        }
    }
    __syncthreads();

    // vertical pass: lane (px, rg) takes windows (rg + kRowGroups * i, px), every channel
    const int px = tid % kT, rg = tid / kT;
    const bool col_ok = x0 + px < W - 10;
    int64_t sum[C];
    int32_t mn[C];
#pragma unroll
    for (int c = 0; c < C; ++c) sum[c] = 0, mn[c] = INT32_MAX;
#pragma unroll
    for (int i = 0; i < kT / kRowGroups; ++i) {
        const int r = rg + kRowGroups * i;
        if (!col_ok || y0 + r >= H - 10) continue;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            uint32_t A = 0, B = 0, XX = 0, YY = 0, XY = 0;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) {
                const uint4 v = planes[(r + t) * G::kCols + px * C + c];   // r + t <= kT - 1 + 8 = kS - 1
                A = mad24(tap(t), v.x & 0xFFFFu, A);
                B = mad24(tap(t), v.x >> 16, B);
                XX = mad24(tap(t), v.y, XX);
                YY = mad24(tap(t), v.z, YY);
                XY = mad24(tap(t), v.w, XY);
            }
            const int64_t ab = (int64_t)((uint64_t)A * B), aa = (int64_t)((uint64_t)A * A), bb = (int64_t)((uint64_t)B * B);
            const int64_t f1 = 2 * ab + kC1;
            const int64_t f2 = 2 * (((int64_t)XY << 16) - ab) + kC2;
            const int64_t f3 = aa + bb + kC1;
            const int64_t f4 = ((int64_t)XX << 16) - aa + ((int64_t)YY << 16) - bb + kC2;
            // |f| < 2^50: the conversions are exact; two products, one division, each rounded to nearest
            const double num = (double)f1 * (double)f2;
            const double den = (double)f3 * (double)f4;
            const double q = num / den;
            const int32_t k = (int32_t)rint(q * 1073741824.0);          // q * 2^30 is exact; rint ties to even
            sum[c] += k;
            mn[c] = min(mn[c], k);
        }
    }

#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int64_t s = wave_sum(sum[c]);
        const int32_t m = wave_min(mn[c]);
        if ((tid & 63) == 0) {
            red_sum[tid >> 6][c] = s;
            red_min[tid >> 6][c] = m;
        }
    }
    __syncthreads();
    if (tid < C) {
        int64_t s = 0;
        int32_t m = INT32_MAX;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            s += red_sum[w][tid];
            m = min(m, red_min[w][tid]);
        }
        // window (0, 0) of every tile counts, so m is a k of this tile
        vcf_ssim_record *r = out + f * C + tid;
        atomicAdd(reinterpret_cast<unsigned long long *>(&r->sum_k), (unsigned long long)s);   // two's complement
        atomicMin(reinterpret_cast<long long *>(&r->min_k), (long long)m);
    }
}

template <int C>
int launch(const uint8_t *a, const uint8_t *b, int64_t n_frames, int64_t F, int32_t H, int32_t W, vcf_ssim_record *out,
           hipStream_t s)
{
    const int32_t tiles_x = (W - 10 + kT - 1) / kT, tiles_y = (H - 10 + kT - 1) / kT;
    return vcf::for_frame_chunks(n_frames, "ssim kernel", [&](int64_t f0, unsigned nf) {
        hipLaunchKernelGGL((ssim_kernel<C>), dim3((unsigned)((int64_t)tiles_x * tiles_y), nf), dim3(kThreads), 0, s, a, b, F,
                           f0, H, W, tiles_x, out);
    });
}

}  // namespace

extern "C" {

int vcf_ssim_tile(void) { return kT; }

int vcf_ssim_u8(const uint8_t *a_dev, const uint8_t *b_dev, int64_t n_frames, int32_t H, int32_t W, int32_t C,
                vcf_ssim_record *out_dev, void *stream)
{
    if (C != 1 && C != 3) return set_error(VCF_ERR_INVALID, "C is 1 or 3 (got %d)", C);
    if (n_frames < 1) return set_error(VCF_ERR_INVALID, "n_frames >= 1 (got %lld)", (long long)n_frames);
    if (H < VCF_SSIM_WINDOW || W < VCF_SSIM_WINDOW)
        return set_error(VCF_ERR_INVALID, "the SSIM window is %d x %d: frames of %d x %d hold none", VCF_SSIM_WINDOW,
                         VCF_SSIM_WINDOW, H, W);
    if (!a_dev || !b_dev || !out_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    if (reinterpret_cast<uintptr_t>(out_dev) & 7) return set_error(VCF_ERR_INVALID, "out_dev must be 8-byte aligned");
    const int64_t F = (int64_t)H * W * C;                              // < 2^31 * 2^31 * 3: no overflow
    if (n_frames > INT64_MAX / F) return set_error(VCF_ERR_INVALID, "n_frames * H * W * C overflows 64 bits");
    const int64_t tiles = (int64_t)((W - 10 + kT - 1) / kT) * ((H - 10 + kT - 1) / kT);
    if (tiles > INT32_MAX) return set_error(VCF_ERR_INVALID, "%lld tiles a frame are beyond one grid", (long long)tiles);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n_records = n_frames * C;
    hipLaunchKernelGGL(ssim_init_kernel, dim3((unsigned)((n_records + 255) / 256)), dim3(256), 0, s, out_dev, n_records,
                       (uint64_t)(H - 10) * (uint64_t)(W - 10));
    const int rc = hip_check(hipGetLastError(), "ssim records");
    if (rc != 0) return rc;
    return C == 1 ? launch<1>(a_dev, b_dev, n_frames, F, H, W, out_dev, s)
                  : launch<3>(a_dev, b_dev, n_frames, F, H, W, out_dev, s);
}

}  // extern "C"
