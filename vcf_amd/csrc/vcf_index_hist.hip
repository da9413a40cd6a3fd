// vcf_index_hist.hip -- histograms of the u8 index planes the encode kernels write, per frame,
// region and channel, as exact integer counts (include/vcf_amd.h, vcf_index_hist_u8).  They are
// what the rate estimate of vcf_amd/rate.py is computed from, so a probe of the rate control costs
// one read of the indices instead of an entropy-coding pass.
//
// A frame is H x W x 3 interleaved bytes; the caller's rows x cols grid cuts it into rectangles of
// (H / rows) x (W / cols) pixels: the whole plane (1 x 1) or the B x B subbands of the DCT's
// subband layout.  One workgroup takes one slice of rows of one region of one frame (grid x =
// region * splits + slice, grid y = frame), so its LDS is the same 12 KiB for every grid: kWaves
// private tables of 3 x 256 counters, one per wave.  (A workgroup per whole stripe of regions would
// need cols such sets, 192 KiB at cols = 16.)  A slice is a list of row segments of S = 3 W / cols
// bytes, RB = 3 W bytes apart -- one segment of rows * RB bytes where cols = 1.  Segments start on a
// pixel, so byte p of a segment is channel p % 3.
//
// Per segment: spans of kSpan = 48 bytes from its first 16-byte boundary on, three 16-byte loads a
// lane.  48 is a multiple of 3, so byte j of every span of a segment is channel (head + j) % 3, the
// rotation `head % 3` being wave-uniform per item; the bytes in front of the first span (at most
// 15) and behind the last (at most 47) are read by byte loads, one per lane, so nothing is read
// outside the segment.  The lanes of a wave instruction all add to one channel's table, and index
// planes are mostly the zero index kHot = 128: those bytes are counted in registers (three counters a
// lane, rotated to channels per item) and only the others go to the LDS atomics, whose lanes then
// spread over the table.  Any content gives the same counts; only the speed assumes the peak.
//
// After the slice: hot counters by wave shuffles into the wave's table, a barrier, then each of the
// 768 bins summed over the waves by one thread and added to the output with one global atomic
// where it is not zero (256 consecutive counters per wave instruction).  Integer adds commute: the
// counts depend on no launch geometry and on no order.
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
constexpr int kSpan = 48;                 // bytes per lane and item: a multiple of lcm(16, 3)
constexpr int kBins = 3 * 256;            // one table: channel-major
constexpr uint32_t kHot = 128;            // the deadzone's zero index
constexpr int kTargetBlocks = 2048;       // 256 CUs x 8 workgroups
constexpr int64_t kMinSlice = 32768;      // bytes a slice should have before a region is cut further
constexpr int kMaxGrid = 16;              // rows, cols: the DCT's subbands up to B = 16

// The twelve dwords of a span: bytes equal to kHot into h[class], the others into the tables.
// t[c] is the table of class c (byte offset in the span % 3).
__device__ __forceinline__ void add_span(const uint4 (&v)[3], uint32_t *const (&t)[3], uint32_t (&h)[3])
{
    const uint32_t w[12] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                            v[2].x, v[2].y, v[2].z, v[2].w};
#pragma unroll
    for (int d = 0; d < 12; ++d) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t b = (w[d] >> (8 * q)) & 0xFFu;
            const int c = (4 * d + q) % 3;
            if (b == kHot)
                ++h[c];
            else
                atomicAdd(t[c] + b, 1u);
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid: x = region * splits + slice, y = frame f0 + y.  F = H * RB bytes a frame (< 2^31), rh rows and
// S bytes a region, `slice_rows` rows a slice.  kLinear: cols = 1, a slice is one segment.
template <bool kLinear>
__global__ __launch_bounds__(kThreads) void index_hist_kernel(const uint8_t *__restrict__ idx, int64_t f0, uint32_t F,
                                                              uint32_t RB, uint32_t S, uint32_t rh, uint32_t cols,
                                                              uint32_t splits, uint32_t slice_rows,
                                                              uint32_t n_regions, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t table[kWaves][kBins];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t region = blockIdx.x / splits, slice = blockIdx.x % splits;
    const uint32_t r0 = slice * slice_rows;
    const int64_t f = f0 + blockIdx.y;
    if (r0 >= rh) return;     // the last slices of a region whose rows do not fill them: uniform per workgroup
    const uint32_t nrows = min(slice_rows, rh - r0);
    const uint32_t y0 = (region / cols) * rh + r0, x0 = (region % cols) * S;
    // segments: n_seg of seg_len bytes, RB apart, the first at byte `first` of the frame
    const uint32_t n_seg = kLinear ? 1u : nrows;
    const uint32_t seg_len = kLinear ? nrows * RB : S;
    const uint8_t *base = idx + f * (int64_t)F + ((int64_t)y0 * RB + x0);

    for (uint32_t i = tid; i < kWaves * kBins; i += kThreads) (&table[0][0])[i] = 0;
    __syncthreads();

    uint32_t *const mine = table[wave];
    uint32_t hot[3] = {0, 0, 0};
    const uint32_t slots = seg_len / kSpan;      // spans a segment can hold at most
    if (slots != 0) {
        const uint32_t items = n_seg * slots;    // <= F / 48
        for (uint32_t item = tid; item < items; item += kThreads) {
            const uint32_t seg = kLinear ? 0u : item / slots, s = kLinear ? item : item % slots;
            const uint8_t *p = base + (int64_t)seg * RB;
            const uint32_t head = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15);   // < 48 <= seg_len
            if (s < (seg_len - head) / kSpan) {
                const uint4 *q = reinterpret_cast<const uint4 *>(p + head + s * kSpan);   // inside the segment
                const uint4 v[3] = {q[0], q[1], q[2]};
                const uint32_t ph = head % 3;    // class c is channel (ph + c) % 3
                uint32_t *const t[3] = {mine + 256 * ph, mine + 256 * ((ph + 1) % 3), mine + 256 * ((ph + 2) % 3)};
                uint32_t h[3] = {0, 0, 0};
                add_span(v, t, h);
                hot[0] += ph == 0 ? h[0] : ph == 1 ? h[2] : h[1];
                hot[1] += ph == 0 ? h[1] : ph == 1 ? h[0] : h[2];
                hot[2] += ph == 0 ? h[2] : ph == 1 ? h[1] : h[0];
            }
        }
    }
    // the bytes outside the spans, a segment per wave in turn and a byte per lane: at most 15 in front, 47 behind
    for (uint32_t seg = wave; seg < n_seg; seg += kWaves) {
        const uint8_t *p = base + (int64_t)seg * RB;
        const uint32_t to_boundary = (uint32_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15);
        const uint32_t head = min(to_boundary, seg_len);
        const uint32_t body = (seg_len - head) / kSpan * kSpan;
        const uint32_t o = lane < head ? lane : head + body + (lane - head);
        if (o < seg_len) atomicAdd(mine + 256 * (o % 3) + p[o], 1u);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t s = wave_sum(hot[c]);
        if (lane == 0 && s != 0) atomicAdd(mine + 256 * c + kHot, s);
    }
    __syncthreads();

    uint32_t *out = counts + (f * n_regions + region) * kBins;
    for (uint32_t i = tid; i < kBins; i += kThreads) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += table[w][i];
        if (s != 0) atomicAdd(out + i, s);
    }
}

}  // namespace

extern "C" {

int vcf_index_hist_u8(const uint8_t *idx_dev, int64_t n_frames, int32_t H, int32_t W, int32_t rows, int32_t cols,
                      uint32_t *counts_dev, int64_t counts_capacity, void *stream)
{
    if (!idx_dev || !counts_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    if (n_frames < 0 || H < 0 || W < 0)
        return set_error(VCF_ERR_INVALID, "negative size (n_frames = %lld, H = %d, W = %d)", (long long)n_frames, H, W);
    if (rows < 1 || cols < 1) return set_error(VCF_ERR_INVALID, "region grid %d x %d: rows, cols >= 1", rows, cols);
    if (rows > kMaxGrid || cols > kMaxGrid)
        return set_error(VCF_ERR_UNSUPPORTED, "region grid %d x %d: at most %d x %d", rows, cols, kMaxGrid, kMaxGrid);
    if (H % rows != 0 || W % cols != 0)
        return set_error(VCF_ERR_INVALID, "region grid %d x %d does not divide the %d x %d frame", rows, cols, H, W);
    VCF_REQUIRE_ALIGNED(counts_dev, 4);
    if ((int64_t)H * W * 3 > INT32_MAX)
        return set_error(VCF_ERR_UNSUPPORTED, "frames of %d x %d x 3: at most 2^31 - 1 bytes a frame", H, W);
    const int64_t n_regions = (int64_t)rows * cols;
    if (n_frames > INT64_MAX / (n_regions * kBins * 4) || (H > 0 && W > 0 && n_frames > INT64_MAX / ((int64_t)H * W * 3)))
        return set_error(VCF_ERR_INVALID, "n_frames = %lld overflows 64 bits", (long long)n_frames);
    const int64_t need = n_frames * n_regions * kBins;
    if (counts_capacity < need)
        return set_error(VCF_ERR_INVALID, "counts_capacity = %lld: %lld counters are written", (long long)counts_capacity,
                         (long long)need);
    if (n_frames == 0) return VCF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = hip_check(hipMemsetAsync(counts_dev, 0, (size_t)need * sizeof(uint32_t), s), "hipMemsetAsync(index counts)");
    if (rc != 0 || H == 0 || W == 0) return rc;

    const uint32_t RB = (uint32_t)W * 3, F = (uint32_t)H * RB;
    const uint32_t rh = (uint32_t)(H / rows), S = RB / (uint32_t)cols;
    return vcf::for_frame_chunks(n_frames, "index histogram kernel", [&](int64_t f0, unsigned nf) {
        // slices a region: enough workgroups for the chip, none under kMinSlice bytes, at least a row each
        const int64_t by_grid = (kTargetBlocks + (int64_t)nf * n_regions - 1) / ((int64_t)nf * n_regions);
        const int64_t by_size = std::max<int64_t>(1, (int64_t)rh * S / kMinSlice);
        const uint32_t want = (uint32_t)std::max<int64_t>(1, std::min<int64_t>({by_grid, by_size, (int64_t)rh}));
        const uint32_t slice_rows = (rh + want - 1) / want;
        const uint32_t splits = (rh + slice_rows - 1) / slice_rows;
        const dim3 grid((unsigned)n_regions * splits, nf);
        if (cols == 1)
            hipLaunchKernelGGL((index_hist_kernel<true>), grid, dim3(kThreads), 0, s, idx_dev, f0, F, RB, S, rh,
                               (uint32_t)cols, splits, slice_rows, (uint32_t)n_regions, counts_dev);
        else
            hipLaunchKernelGGL((index_hist_kernel<false>), grid, dim3(kThreads), 0, s, idx_dev, f0, F, RB, S, rh,
                               (uint32_t)cols, splits, slice_rows, (uint32_t)n_regions, counts_dev);
    });
}

}  // extern "C"
