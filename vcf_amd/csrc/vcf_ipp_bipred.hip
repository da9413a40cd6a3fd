// vcf_ipp_bipred.hip -- bidirectionally predicted B-frames for the IPP loop
// (--bframes, not in the reference): the per-block three-way decision with its
// residual, and the matching reconstruction; vcf_ipp_bipred_residual and
// vcf_ipp_bipred_reconstruct of the C ABI.  The rule is stated in
// include/vcf_amd.h ("B-frames") and restated in numpy by tests/bipred_ref.py;
// everything is integer arithmetic.
//
// Per full bs x bs block the candidates are p0 = cf, p1 = cb and
// p2 = (cf + cb + 1) >> 1 per byte; the mode is the argmin of (SAD_m, m) over
// the block's bs * bs * 3 bytes; pred is the winner inside full blocks and 0
// outside them.
//
// Mapping (both kernels): grid.y is the band of bs rows, grid.x a strip of G
// whole block columns, so no block is shared between workgroups.  A thread
// owns one 4-byte unit of the strip's row bytes and every R-th row of it: its
// column, and with it the one or two blocks its bytes lie in, is fixed, so the
// byte masks and the block numbers are worked out once.  The encoder loads its
// units of cur, cf and cb once into registers, adds its partial SADs
// (v_sad_u8 on masked words) to the strip's per-block sums in LDS, and after
// the barrier reads the three sums of its blocks, picks the mode and writes the
// residual from the registers; the prediction never exists in memory.  Integer
// sums: the result does not depend on G, R or the order of the additions.
// Units are aligned words of the frame where every pointer is 4-byte aligned
// and the row pitch is a multiple of 4, else 4 bytes from the strip's first
// byte, loaded and stored one by one; the arithmetic is the same.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"

namespace vcf {
namespace {

constexpr int kMaxBs = 64;
constexpr int kThreads = 256;
constexpr int kMaxStripBlocks = 340;   // units(G) <= 256 at bs = 1
constexpr int kRowsHeld = 4;           // the rows a thread holds where the split can choose
constexpr int kMaxRowsHeld = 13;       // bs = 64, one block per strip: 49 units, 5 rows at a time

// the most 4-byte units a row of a strip of G blocks spans (an unaligned first byte costs one more)
__host__ __device__ constexpr int strip_units(int G, int bs) { return (G * bs * 3 + 3) / 4 + 1; }

// the rows a thread holds in a strip of G blocks of side bs
constexpr int rows_held(int G, int bs)
{
    const int R = kThreads / strip_units(G, bs);
    return R ? (bs + R - 1) / R : 1 << 30;
}

constexpr int most_rows_held_one_block_per_strip()
{
    int k = 0;
    for (int bs = 1; bs <= kMaxBs; ++bs) k = rows_held(1, bs) > k ? rows_held(1, bs) : k;
    return k;
}
static_assert(most_rows_held_one_block_per_strip() <= kMaxRowsHeld, "the widest instantiation holds every block size");

struct Split {
    int G, R, K;   // block columns per strip, rows in flight per workgroup, rows per thread
};

// The widest strip whose threads hold at most kRowsHeld rows each; one block per strip where no strip does.
inline Split choose_split(int bs, int block_columns)
{
    int G = 1;
    while (G < block_columns && G < kMaxStripBlocks && rows_held(G + 1, bs) <= kRowsHeld) ++G;
    return {G, kThreads / strip_units(G, bs), rows_held(G, bs)};
}

// bytes a .. b - 1 of a word as 0xFF each, 0 <= a, b <= 4
__host__ __device__ inline uint32_t byte_mask(int a, int b)
{
    if (a >= b) return 0u;
    return (uint32_t)(((1ull << (8 * b)) - 1) & ~((1ull << (8 * a)) - 1));
}

struct Lane {
    int e0, r0;            // first byte of the unit in its row; first row in the band
    uint32_t ms, ma, mb;   // bytes of this strip; of them, those in full block A / B
    int ba, bb;            // the block columns of A and B
};

// The thread's unit: false for a thread without one.
template <bool WORDS>
__host__ __device__ inline bool lane_setup(int W, int bs, int G, int R, int nbx, bool full_band, int strip, int tid,
                                           Lane &l)
{
    const int rb = W * 3;
    const int sb0 = strip * G * bs * 3;
    const int sb1 = sb0 + G * bs * 3 < rb ? sb0 + G * bs * 3 : rb;
    const int u0 = WORDS ? (sb0 & ~3) : sb0;
    const int units = (sb1 - u0 + 3) / 4;
    if (tid >= units * R) return false;
    l.r0 = tid / units;
    l.e0 = u0 + 4 * (tid - l.r0 * units);
    const int lo = l.e0 > sb0 ? l.e0 : sb0, hi = l.e0 + 4 < sb1 ? l.e0 + 4 : sb1;   // lo < hi
    l.ms = byte_mask(lo - l.e0, hi - l.e0);
    l.ba = (lo / 3) / bs;
    l.bb = ((hi - 1) / 3) / bs;
    const int cut = l.bb * bs * 3;   // the first byte of block B
    l.ma = (full_band && l.ba < nbx) ? byte_mask(lo - l.e0, (l.ba == l.bb ? hi : cut) - l.e0) : 0u;
    l.mb = (full_band && l.bb != l.ba && l.bb < nbx) ? byte_mask(cut - l.e0, hi - l.e0) : 0u;
    return true;
}

template <bool WORDS>
__host__ __device__ inline uint32_t load_unit(const uint8_t *row, const Lane &l)
{
    if (WORDS) return *reinterpret_cast<const uint32_t *>(row + l.e0);
    uint32_t v = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n)
        if ((l.ms >> (8 * n)) & 1u) v |= (uint32_t)row[l.e0 + n] << (8 * n);
    return v;
}

template <bool WORDS>
__host__ __device__ inline void store_unit(uint8_t *row, const Lane &l, uint32_t v)
{
    if (WORDS && l.ms == 0xFFFFFFFFu) {
        *reinterpret_cast<uint32_t *>(row + l.e0) = v;
        return;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
        if ((l.ms >> (8 * n)) & 1u) row[l.e0 + n] = (uint8_t)(v >> (8 * n));
}

__host__ __device__ inline uint32_t sad4(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int n = 0; n < 4; ++n) {
        const int d = (int)((a >> (8 * n)) & 255u) - (int)((b >> (8 * n)) & 255u);
        acc += (uint32_t)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

// (a + b + 1) >> 1 in each byte
__host__ __device__ inline uint32_t avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7F7F7F7Fu); }

__host__ __device__ inline uint32_t candidate(uint32_t f, uint32_t b, int mode)
{
    return mode == 1 ? b : (mode == 2 ? avg4(f, b) : f);   // a mode byte above 2 behaves as 0
}

// argmin of (SAD_m, m)
__host__ __device__ inline int pick_mode(const uint32_t *s)
{
    int m = 0;
    uint32_t best = s[0];
    if (s[1] < best) { best = s[1]; m = 1; }
    if (s[2] < best) m = 2;
    return m;
}

// clip(x - p + 128) (SIGN = -1) or clip(p + x - 128) (SIGN = +1) in each byte
template <int SIGN>
__host__ __device__ inline uint32_t shift_clip4(uint32_t x, uint32_t p)
{
    uint32_t out = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int a = (int)((x >> (8 * n)) & 255u), q = (int)((p >> (8 * n)) & 255u);
        const int v = SIGN < 0 ? a - q + 128 : q + a - 128;
        out |= (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * n);
    }
    return out;
}

// a unit's partial SADs of the three candidates over the bytes of mask m
__host__ __device__ inline void add_sads(uint32_t c, uint32_t f, uint32_t b, uint32_t m, uint32_t *s)
{
    c &= m;
    s[0] = sad4(c, f & m, s[0]);
    s[1] = sad4(c, b & m, s[1]);
    s[2] = sad4(c, avg4(f, b) & m, s[2]);
}

template <int K, bool WORDS>
__global__ __launch_bounds__(kThreads) void ipp_bipred_residual_kernel(const uint8_t *__restrict__ cur,
                                                                       const uint8_t *__restrict__ cf,
                                                                       const uint8_t *__restrict__ cb, int H, int W,
                                                                       int bs, int G, int R,
                                                                       uint8_t *__restrict__ modes,
                                                                       uint8_t *__restrict__ res)
{
    __shared__ uint32_t sums[3 * kMaxStripBlocks];
    const int tid = threadIdx.x, strip = blockIdx.x, band = blockIdx.y;
    const int nbx = W / bs, nby = H / bs, bx0 = strip * G;
    const bool full = band < nby;
    const int rows = H - band * bs < bs ? H - band * bs : bs;
    const long long rb = (long long)W * 3, base = (long long)band * bs * rb;
    for (int t = tid; t < 3 * G; t += kThreads) sums[t] = 0;
    __syncthreads();
    Lane l;
    const bool on = lane_setup<WORDS>(W, bs, G, R, nbx, full, strip, tid, l);
    const bool predicted = on && (l.ma | l.mb);   // else every byte of the unit has pred = 0
    uint32_t c[K], f[K], b[K];
    if (on) {
        uint32_t sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int row = l.r0 + k * R;
            c[k] = f[k] = b[k] = 0;
            if (row >= rows) continue;
            const long long o = base + row * rb;
            c[k] = load_unit<WORDS>(cur + o, l);
            if (!predicted) continue;
            f[k] = load_unit<WORDS>(cf + o, l);
            b[k] = load_unit<WORDS>(cb + o, l);
            add_sads(c[k], f[k], b[k], l.ma, sa);
            if (l.mb) add_sads(c[k], f[k], b[k], l.mb, sb);
        }
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            if (l.ma) atomicAdd(&sums[3 * (l.ba - bx0) + m], sa[m]);
            if (l.mb) atomicAdd(&sums[3 * (l.bb - bx0) + m], sb[m]);
        }
    }
    __syncthreads();
    if (full)
        for (int t = tid; t < G && bx0 + t < nbx; t += kThreads)
            modes[(long long)band * nbx + bx0 + t] = (uint8_t)pick_mode(sums + 3 * t);
    if (!on) return;
    const int mode_a = l.ma ? pick_mode(sums + 3 * (l.ba - bx0)) : 0;
    const int mode_b = l.mb ? pick_mode(sums + 3 * (l.bb - bx0)) : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int row = l.r0 + k * R;
        if (row >= rows) continue;
        const uint32_t pred = (candidate(f[k], b[k], mode_a) & l.ma) | (candidate(f[k], b[k], mode_b) & l.mb);
        store_unit<WORDS>(res + base + row * rb, l, shift_clip4<-1>(c[k], pred));
    }
}

template <bool WORDS>
__global__ __launch_bounds__(kThreads) void ipp_bipred_reconstruct_kernel(const uint8_t *__restrict__ cf,
                                                                          const uint8_t *__restrict__ cb,
                                                                          const uint8_t *__restrict__ modes,
                                                                          const uint8_t *__restrict__ rec, int H,
                                                                          int W, int bs, int G, int R,
                                                                          uint8_t *__restrict__ out)
{
    const int tid = threadIdx.x, strip = blockIdx.x, band = blockIdx.y;
    const int nbx = W / bs, nby = H / bs;
    const int rows = H - band * bs < bs ? H - band * bs : bs;
    const long long rb = (long long)W * 3, base = (long long)band * bs * rb;
    Lane l;
    if (!lane_setup<WORDS>(W, bs, G, R, nbx, band < nby, strip, tid, l)) return;
    const int mode_a = l.ma ? modes[(long long)band * nbx + l.ba] : 0;
    const int mode_b = l.mb ? modes[(long long)band * nbx + l.bb] : 0;
    // a source no byte of the unit predicts from is not read
    const bool need_f = (l.ma && mode_a != 1) || (l.mb && mode_b != 1);
    const bool need_b = (l.ma && (mode_a == 1 || mode_a == 2)) || (l.mb && (mode_b == 1 || mode_b == 2));
    for (int row = l.r0; row < rows; row += R) {
        const long long o = base + row * rb;
        const uint32_t r = load_unit<WORDS>(rec + o, l);
        const uint32_t f = need_f ? load_unit<WORDS>(cf + o, l) : 0u;
        const uint32_t b = need_b ? load_unit<WORDS>(cb + o, l) : 0u;
        const uint32_t pred = (candidate(f, b, mode_a) & l.ma) | (candidate(f, b, mode_b) & l.mb);
        store_unit<WORDS>(out + o, l, shift_clip4<+1>(r, pred));
    }
}

int check_bipred(const void *a, const void *b, const void *c, const void *d, int H, int W, int bs)
{
    if (!a || !b || !c || !d) return set_error(VCF_ERR_INVALID, "null buffer");
    if (H <= 0 || W <= 0) return set_error(VCF_ERR_INVALID, "bad frame %d x %d", H, W);
    if (bs < 1 || bs > kMaxBs) return set_error(VCF_ERR_INVALID, "block size %d (1..%d)", bs, kMaxBs);
    if (H > 65535) return set_error(VCF_ERR_INVALID, "frame height %d (at most 65535 rows)", H);
    if ((long long)H * W * 3 >= (1LL << 31)) return set_error(VCF_ERR_INVALID, "frame too large");
    return VCF_OK;
}

// bands of bs rows (the last may be short) x strips of G block columns (the last block column may be partial)
dim3 bipred_grid(int H, int W, int bs, const Split &s)
{
    const int block_columns = (W + bs - 1) / bs;
    return dim3((unsigned)((block_columns + s.G - 1) / s.G), (unsigned)((H + bs - 1) / bs));
}

template <bool WORDS>
void launch_residual(const Split &s, dim3 grid, hipStream_t st, const uint8_t *cur, const uint8_t *cf,
                     const uint8_t *cb, int H, int W, int bs, uint8_t *modes, uint8_t *res)
{
    if (s.K <= kRowsHeld)
        hipLaunchKernelGGL((ipp_bipred_residual_kernel<kRowsHeld, WORDS>), grid, dim3(kThreads), 0, st, cur, cf, cb, H,
                           W, bs, s.G, s.R, modes, res);
    else if (s.K <= 8)
        hipLaunchKernelGGL((ipp_bipred_residual_kernel<8, WORDS>), grid, dim3(kThreads), 0, st, cur, cf, cb, H, W, bs,
                           s.G, s.R, modes, res);
    else
        hipLaunchKernelGGL((ipp_bipred_residual_kernel<kMaxRowsHeld, WORDS>), grid, dim3(kThreads), 0, st, cur, cf, cb,
                           H, W, bs, s.G, s.R, modes, res);
}

}  // namespace
}  // namespace vcf

using namespace vcf;

extern "C" {

int vcf_ipp_bipred_residual(const uint8_t *cur_dev, const uint8_t *cf_dev, const uint8_t *cb_dev, int32_t H, int32_t W,
                            int32_t bs, uint8_t *modes_dev, uint8_t *res_dev, void *stream)
{
    const int rc = check_bipred(cur_dev, cf_dev, cb_dev, res_dev, H, W, bs);
    if (rc != VCF_OK) return rc;
    if (!modes_dev && H / bs > 0 && W / bs > 0) return set_error(VCF_ERR_INVALID, "null mode map");
    const Split s = choose_split(bs, (W + bs - 1) / bs);
    const dim3 grid = bipred_grid(H, W, bs, s);
    const bool words = aligned_to(cur_dev, 4) && aligned_to(cf_dev, 4) && aligned_to(cb_dev, 4) &&
                       aligned_to(res_dev, 4) && (W * 3) % 4 == 0;
    if (words)
        launch_residual<true>(s, grid, (hipStream_t)stream, cur_dev, cf_dev, cb_dev, H, W, bs, modes_dev, res_dev);
    else
        launch_residual<false>(s, grid, (hipStream_t)stream, cur_dev, cf_dev, cb_dev, H, W, bs, modes_dev, res_dev);
    return hip_check(hipGetLastError(), "ipp bipred residual launch");
}

int vcf_ipp_bipred_reconstruct(const uint8_t *cf_dev, const uint8_t *cb_dev, const uint8_t *modes_dev,
                               const uint8_t *rec_dev, int32_t H, int32_t W, int32_t bs, uint8_t *out_dev, void *stream)
{
    const int rc = check_bipred(cf_dev, cb_dev, rec_dev, out_dev, H, W, bs);
    if (rc != VCF_OK) return rc;
    if (!modes_dev && H / bs > 0 && W / bs > 0) return set_error(VCF_ERR_INVALID, "null mode map");
    const Split s = choose_split(bs, (W + bs - 1) / bs);
    const dim3 grid = bipred_grid(H, W, bs, s);
    const bool words = aligned_to(cf_dev, 4) && aligned_to(cb_dev, 4) && aligned_to(rec_dev, 4) &&
                       aligned_to(out_dev, 4) && (W * 3) % 4 == 0;
    if (words)
        hipLaunchKernelGGL((ipp_bipred_reconstruct_kernel<true>), grid, dim3(kThreads), 0, (hipStream_t)stream, cf_dev,
                           cb_dev, modes_dev, rec_dev, H, W, bs, s.G, s.R, out_dev);
    else
        hipLaunchKernelGGL((ipp_bipred_reconstruct_kernel<false>), grid, dim3(kThreads), 0, (hipStream_t)stream,
                           cf_dev, cb_dev, modes_dev, rec_dev, H, W, bs, s.G, s.R, out_dev);
    return hip_check(hipGetLastError(), "ipp bipred reconstruct launch");
}

}  // extern "C"
