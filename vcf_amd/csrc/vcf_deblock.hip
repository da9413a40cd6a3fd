// vcf_deblock.hip -- the deblocking post-filter of the block-transform decoders (-f deblock;
// DESIGN.md §4.19).  The rule is stated in include/vcf_amd.h (vcf_deblock_u8): pass V filters
// across the vertical block edges along rows and reads the input, pass H filters across the
// horizontal edges down columns and reads pass V's result; per line HEVC's normal filter.
//
// One kernel runs both passes through an LDS tile, so the batch is read once and written once.
// A frame is H rows of RB = 3 W bytes.  A workgroup owns kTileRows x kTileBytes output bytes
// (160 pixels: a multiple of 3 and of 16 bytes).  A line changes samples up to 2 from its edge
// and reads up to 3 from it, so an output sample depends on pass-V values up to 4 rows away and
// those on input up to 4 pixels away: the tile is staged with a halo of kHalo = 4 rows and
// 4 pixels = 12 bytes, and pass V is recomputed on the halo rows.
//
//   1. stage   rows r0 - 4 .. r0 + 59, bytes b0 - 12 .. b0 + 491, clipped to the frame.  LDS row
//              lr keeps byte column c at lr * kPitch + kFront + s + (c - b0), s = the low four
//              address bits of the row's byte b0: LDS offsets and global addresses agree mod 16,
//              so a 16-byte global chunk is one aligned 16-byte LDS store whatever the base and
//              the row pitch are.  A chunk that lies wholly inside the frame is one 16-byte load;
//              the chunks that cross the frame's first or last byte are read by byte loads.
//   2. pass V  a lane per (row, channel) walks the row's edges from left to right, in place.
//   3. pass H  a lane per byte column walks the tile's edges from top to bottom, in place.
//   4. store   rows r0 .. r0 + 55, bytes b0 .. b0 + 479: 16-byte stores of the chunks wholly
//              inside the tile's own bytes where out - in is a multiple of 16 (two hipMalloc'd
//              sets, or equal offsets into them), the row ends by bytes; byte stores otherwise.
//
// In place is safe although a pass reads the samples it has not yet changed: the edges of a pass
// are B >= 4 apart, a line writes x - 2 .. x + 1 and reads x - 3 .. x + 2, so the only sample one
// line writes and another reads is, at B = 4, q1 of edge x = p2 of edge x + 4.  The walking lane
// keeps the q1 it read and hands it to the next line as its p2; q2 of edge x is p1 of edge x + 4,
// which the walk has not reached.  No other lane touches the lane's row (column).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vcf_amd.h"
#include "vcf_internal.h"

namespace {

using vcf::hip_check;
using vcf::set_error;

constexpr int kThreads = 256;
constexpr int kTileRows = 56;                       // output rows of a tile
constexpr int kHalo = 4;                            // rows (and pixels) staged around it
constexpr int kRows = kTileRows + 2 * kHalo;        // 64 LDS rows
constexpr int kTilePx = 160;                        // output pixels of a tile row
constexpr int kTileBytes = 3 * kTilePx;             // 480: a multiple of 16
constexpr int kHaloBytes = 3 * kHalo;               // 12
constexpr int kFront = 32;                          // LDS bytes in front of byte b0 of a row (>= 12 + 15, multiple of 16)
constexpr int kPitch = kTileBytes + 80;             // 560 >= kFront + 15 + kTileBytes + kHaloBytes + 15, multiple of 16
constexpr int kLoadChunks = (15 + kTileBytes + 2 * kHaloBytes + 15) / 16;   // 16-byte chunks that can cover a staged row
constexpr int kStoreChunks = (15 + kTileBytes + 15) / 16;                   // ... a tile row
// strengths above these change nothing (|delta| <= 191, dp + dq <= 1020): the entry clamps to them
constexpr int kMaxBeta = 8192;
constexpr int kMaxTc = 1024;

static_assert(kTileBytes % 16 == 0 && kPitch % 16 == 0 && kFront % 16 == 0, "16-byte LDS stores");
static_assert(kFront >= kHaloBytes + 15 && kPitch >= kFront + 15 + kTileBytes + kHaloBytes + 15, "a staged row fits its LDS row");
static_assert(kRows * 3 <= kThreads, "pass V: a lane per row and channel");

struct Args {
    const uint8_t *in;
    uint8_t *out;
    int64_t stride;       // bytes from one frame to the next, in and out alike
    int64_t f0;           // first frame of this launch
    int64_t tiles_x;
    int32_t H, W, B, top, left, beta, tc;
};

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// One line: true and the four new samples if it is filtered.
__device__ __forceinline__ bool filter_line(int p2, int &p1, int &p0, int &q0, int &q1, int q2, int beta, int tc)
{
    const int dp = abs(p2 - 2 * p1 + p0), dq = abs(q2 - 2 * q1 + q0);
    if (dp + dq >= beta) return false;
    int delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4;
    if (abs(delta) >= 10 * tc) return false;
    delta = min(max(delta, -tc), tc);
    const int side = (beta + (beta >> 1)) >> 3, h = tc >> 1;
    const int n1 = dp < side ? clip255(p1 + min(max((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1, -h), h)) : p1;
    const int m1 = dq < side ? clip255(q1 + min(max((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1, -h), h)) : q1;
    p0 = clip255(p0 + delta);
    q0 = clip255(q0 - delta);
    p1 = n1;
    q1 = m1;
    return true;
}

// the first x >= lo with (x + phase) % B == 0
__device__ __forceinline__ int64_t first_edge(int64_t lo, int phase, int B)
{
    const int m = (int)((lo + phase) % B);
    return m ? lo + (B - m) : lo;
}

// grid: x = the frame's tiles (row of tiles by row), z = frame f0 + z
template <bool kVecStore>
__global__ __launch_bounds__(kThreads) void deblock_kernel(const Args a)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[kRows * kPitch];
    const int tid = threadIdx.x;
    const int64_t f = a.f0 + blockIdx.z;
    const uint8_t *in = a.in + f * a.stride;
    uint8_t *out = a.out + f * a.stride;
    const int64_t H = a.H, W = a.W, RB = 3 * W, F = RB * H;
    const int B = a.B, beta = a.beta, tc = a.tc;
    const int64_t b0 = (int64_t)(blockIdx.x % a.tiles_x) * kTileBytes;     // first byte column of the tile
    const int64_t r0 = (int64_t)(blockIdx.x / a.tiles_x) * kTileRows;      // first row
    const int64_t rlo = r0 - kHalo;                                        // the row LDS row 0 holds
    const int64_t clo = max(b0 - kHaloBytes, (int64_t)0), chi = min(b0 + kTileBytes + kHaloBytes, RB);   // staged columns
    const int64_t ain = (int64_t)reinterpret_cast<uintptr_t>(in);
    // LDS row lr: the low address bits of its byte b0 are (s0 + lr * ds) & 15
    const int s0 = (int)((ain + rlo * RB + b0) & 15), ds = (int)(RB & 15);
    const auto rowpos = [&](int lr) { return lr * kPitch + kFront + ((s0 + lr * ds) & 15); };

    // 1. stage
    for (int i = tid; i < kRows * kLoadChunks; i += kThreads) {
        const int lr = i / kLoadChunks, k = i % kLoadChunks;
        const int64_t r = rlo + lr;
        if (r < 0 || r >= H) continue;
        const int64_t row = r * RB, lo = row + clo, hi = row + chi;         // frame offsets
        const int64_t co = (((ain + lo) & ~(int64_t)15) - ain) + 16 * k;    // this chunk's: 16-byte aligned as an address
        if (co >= hi) continue;
        const int lp = rowpos(lr) + (int)(co - row - b0);                   // a multiple of 16, inside LDS row lr
        if (co >= 0 && co + 16 <= F) {
            *reinterpret_cast<uint4 *>(tile + lp) = *reinterpret_cast<const uint4 *>(in + co);
        } else {
            for (int j = 0; j < 16; ++j)
                if (co + j >= lo && co + j < hi) tile[lp + j] = in[co + j];
        }
    }
    __syncthreads();

    // 2. pass V: the edges whose lines write into, or are read from, the tile's columns
    if (tid < kRows * 3) {
        const int lr = tid / 3, ch = tid % 3;
        const int64_t r = rlo + lr;
        if (r >= 0 && r < H) {
            const int64_t px0 = b0 / 3, px1 = min(px0 + kTilePx, W);
            const int64_t x_lo = max(px0 - 1, (int64_t)3), x_hi = min(px1 + 1, W - 3);   // x - 3 >= 0, x + 2 <= W - 1
            uint8_t *rowp = tile + rowpos(lr) + ch;
            bool have = false;
            int prev_q1 = 0;
            for (int64_t x = first_edge(x_lo, a.left, B); x <= x_hi; x += B) {
                uint8_t *q = rowp + (int)(3 * x - b0);
                int p2 = q[-9], p1 = q[-6], p0 = q[-3], q0 = q[0], q1 = q[3];
                const int q2 = q[6];
                if (B == 4 && have) p2 = prev_q1;       // the sample the line before this one wrote
                prev_q1 = q1;
                have = true;
                if (filter_line(p2, p1, p0, q0, q1, q2, beta, tc)) {
                    q[-6] = (uint8_t)p1;
                    q[-3] = (uint8_t)p0;
                    q[0] = (uint8_t)q0;
                    q[3] = (uint8_t)q1;
                }
            }
        }
    }
    __syncthreads();

    // 3. pass H: the edges whose lines write into the tile's rows
    const int ncols = (int)min((int64_t)kTileBytes, RB - b0);
    const int64_t rend = min(r0 + kTileRows, H);
    {
        const int64_t y_lo = max(r0 - 1, (int64_t)3), y_hi = min(rend + 1, H - 3);
        const int64_t y_first = first_edge(y_lo, a.top, B);
        for (int j = tid; j < ncols; j += kThreads) {
            bool have = false;
            int prev_q1 = 0;
            for (int64_t y = y_first; y <= y_hi; y += B) {
                const int lr = (int)(y - rlo);          // 3 <= lr <= kRows - 3
                uint8_t *s[6];
#pragma unroll
                for (int d = 0; d < 6; ++d) s[d] = tile + rowpos(lr - 3 + d) + j;
                int p2 = *s[0], p1 = *s[1], p0 = *s[2], q0 = *s[3], q1 = *s[4];
                const int q2 = *s[5];
                if (B == 4 && have) p2 = prev_q1;
                prev_q1 = q1;
                have = true;
                if (filter_line(p2, p1, p0, q0, q1, q2, beta, tc)) {
                    *s[1] = (uint8_t)p1;
                    *s[2] = (uint8_t)p0;
                    *s[3] = (uint8_t)q0;
                    *s[4] = (uint8_t)q1;
                }
            }
        }
    }
    __syncthreads();

    // 4. store the tile's own rows and columns
    const int nrows = (int)(rend - r0);
    if constexpr (kVecStore) {
        for (int i = tid; i < nrows * kStoreChunks; i += kThreads) {
            const int lr = kHalo + i / kStoreChunks, k = i % kStoreChunks;
            const int64_t row = (rlo + lr) * RB, lo = row + b0, hi = lo + ncols;
            const int64_t co = (((ain + lo) & ~(int64_t)15) - ain) + 16 * k;
            if (co >= hi) continue;
            const int lp = rowpos(lr) + (int)(co - lo);
            if (co >= lo && co + 16 <= hi) {
                *reinterpret_cast<uint4 *>(out + co) = *reinterpret_cast<const uint4 *>(tile + lp);
            } else {
                for (int j = 0; j < 16; ++j)
                    if (co + j >= lo && co + j < hi) out[co + j] = tile[lp + j];
            }
        }
    } else {
        for (int i = tid; i < nrows * ncols; i += kThreads) {
            const int lr = kHalo + i / ncols, j = i % ncols;
            out[(rlo + lr) * RB + b0 + j] = tile[rowpos(lr) + j];
        }
    }
}

}  // namespace

extern "C" {

int vcf_deblock_u8(const uint8_t *in_dev, uint8_t *out_dev, int64_t n_frames, int32_t H, int32_t W,
                   int64_t frame_stride_bytes, int32_t B, int32_t top, int32_t left, int32_t beta, int32_t tc,
                   void *stream)
{
    if (n_frames < 0 || H < 0 || W < 0)
        return set_error(VCF_ERR_INVALID, "negative size (n_frames = %lld, H = %d, W = %d)", (long long)n_frames, H, W);
    if (B < 4) return set_error(VCF_ERR_INVALID, "B >= 4 (got %d): the lines of two edges would overlap", B);
    if (top < 0 || top >= B || left < 0 || left >= B)
        return set_error(VCF_ERR_INVALID, "0 <= top, left < B (got top = %d, left = %d, B = %d)", top, left, B);
    if (beta < 0 || tc < 0) return set_error(VCF_ERR_INVALID, "beta >= 0 and tc >= 0 (got %d, %d)", beta, tc);
    if (!in_dev || !out_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    if (W > 0 && (int64_t)H > INT64_MAX / 3 / W) return set_error(VCF_ERR_INVALID, "H * W * 3 overflows 64 bits");
    const int64_t F = (int64_t)H * W * 3;
    if (frame_stride_bytes < F)
        return set_error(VCF_ERR_INVALID, "frame_stride_bytes %lld is less than a frame's %lld bytes",
                         (long long)frame_stride_bytes, (long long)F);
    if (n_frames > 1 && frame_stride_bytes > (INT64_MAX - F) / (n_frames - 1))
        return set_error(VCF_ERR_INVALID, "n_frames * frame_stride_bytes overflows 64 bits");
    const int64_t extent = n_frames > 0 ? (n_frames - 1) * frame_stride_bytes + F : 0;
    const uintptr_t pi = reinterpret_cast<uintptr_t>(in_dev), po = reinterpret_cast<uintptr_t>(out_dev);
    if (pi == po || (extent > 0 && pi < po + (uintptr_t)extent && po < pi + (uintptr_t)extent))
        return set_error(VCF_ERR_INVALID, "in_dev and out_dev overlap: the filter is out of place");
    if (n_frames == 0 || F == 0) return VCF_OK;

    const int64_t tiles_x = ((int64_t)W * 3 + kTileBytes - 1) / kTileBytes, tiles_y = ((int64_t)H + kTileRows - 1) / kTileRows;
    if (tiles_y > INT32_MAX / tiles_x)
        return set_error(VCF_ERR_UNSUPPORTED, "a frame of %d x %d is more tiles than one launch takes", H, W);
    Args a{in_dev, out_dev, frame_stride_bytes, 0, tiles_x, H, W, B, top, left, std::min(beta, kMaxBeta), std::min(tc, kMaxTc)};
    const bool vec = ((pi - po) & 15) == 0;    // a frame's in and out addresses then agree mod 16
    hipStream_t s = static_cast<hipStream_t>(stream);
    return vcf::for_frame_chunks(n_frames, "deblock kernel", [&](int64_t f0, unsigned nf) {
        a.f0 = f0;
        const dim3 grid((unsigned)(tiles_x * tiles_y), 1, nf);
        if (vec)
            hipLaunchKernelGGL(deblock_kernel<true>, grid, dim3(kThreads), 0, s, a);
        else
            hipLaunchKernelGGL(deblock_kernel<false>, grid, dim3(kThreads), 0, s, a);
    });
}

}  // extern "C"
