// vcf_vq.hip -- the vector quantizer of src/VQ.py and src/color-VQ.py: k-means
// (sklearn.cluster.KMeans, algorithm="lloyd", n_init=1) on BS x BS x C pixel
// blocks.  The arithmetic of every entry point is stated in include/vcf_amd.h.
//
// Vectors are read straight from the u8 frame (vector n = block (n / Wb, n % Wb),
// element d = row d / (BS*C), byte d % (BS*C) of that row), so no entry point
// needs a gathered copy of the image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "vcf_amd.h"
#include "vcf_internal.h"

namespace {

using vcf::hip_check;
using vcf::set_error;

constexpr int kThreads = 256;
constexpr int kVT = 2;                 // vectors per thread of the assign kernel
constexpr int kJT = 8;                 // centroids per register group of the assign kernel
constexpr int kTileBytes = 32 * 1024;  // LDS budget of one K-tile (a tile of 8 centroids may take up to 64 KiB)
constexpr int kMaxKT = 512;
constexpr int kAccVectors = 2048;      // vectors per block of the accumulate and moments kernels
constexpr int kAccLdsBytes = 48 * 1024;
constexpr int kMaxTrials = 16;         // 2 + floor(ln 4096) = 10
constexpr int kMaxD = 16 * 16 * 4;
constexpr int kMaxK = 4096;

struct Geo {
    int32_t H, W, C, BS;
    int32_t Wb;       // blocks per row
    int32_t D;        // BS * BS * C
    int32_t rowlen;   // BS * C: bytes of one block row
    int64_t N;        // vectors
    int64_t pitch;    // W * C: bytes of one image row
};

int make_geo(int32_t H, int32_t W, int32_t C, int32_t BS, Geo *g)
{
    if (H < 1 || W < 1) return set_error(VCF_ERR_INVALID, "H and W must be at least 1 (got %d x %d)", H, W);
    if (C < 1 || C > 4) return set_error(VCF_ERR_INVALID, "1 <= C <= 4 (got %d)", C);
    if (BS < 1 || BS > 16) return set_error(VCF_ERR_INVALID, "1 <= block size <= 16 (got %d)", BS);
    if (H % BS || W % BS)
        return set_error(VCF_ERR_INVALID, "%d x %d is not a whole number of %d x %d blocks", H, W, BS, BS);
    g->H = H, g->W = W, g->C = C, g->BS = BS;
    g->Wb = W / BS;
    g->D = BS * BS * C;
    g->rowlen = BS * C;
    g->N = (int64_t)(H / BS) * g->Wb;
    g->pitch = (int64_t)W * C;
    return VCF_OK;
}

int check_k(const Geo &g, int32_t K)
{
    if (K < 1 || K > kMaxK || K > g.N)
        return set_error(VCF_ERR_INVALID, "1 <= K <= min(N, %d) (got K = %d, N = %lld)", kMaxK, K, (long long)g.N);
    return VCF_OK;
}

__device__ __forceinline__ int64_t vec_base(const Geo &g, int64_t n)
{
    const int64_t by = n / g.Wb, bx = n - by * g.Wb;
    return by * g.BS * g.pitch + bx * g.rowlen;
}

__device__ __forceinline__ int64_t elem_offset(const Geo &g, int32_t d)
{
    const int32_t r = d / g.rowlen;
    return r * g.pitch + (d - r * g.rowlen);
}

// ---- assign -------------------------------------------------------------------
// One thread holds kVT vectors and, per pass, kJT running distances for each.
// The K-tile sits in LDS transposed ([d][KT]) so that the kJT centroids of a
// pass are 64 contiguous bytes at one address for the whole wave (a broadcast
// read).  Per (vector, centroid): acc = acc + (x - c) * (x - c), d ascending,
// three separate roundings (the library is built with -ffp-contract=off).
__global__ __launch_bounds__(kThreads) void vq_assign_kernel(const uint8_t *__restrict__ img, Geo g,
                                                             const double *__restrict__ cent, int32_t K, int32_t KT,
                                                             uint16_t *__restrict__ labels, double *__restrict__ dist,
                                                             unsigned int *__restrict__ changed)
{
    extern __shared__ double tile[];
    const int64_t n0 = (int64_t)blockIdx.x * (kThreads * kVT) + threadIdx.x;
    const uint8_t *px[kVT];
    double best[kVT];
    int32_t bestj[kVT];
#pragma unroll
    for (int v = 0; v < kVT; ++v) {
        const int64_t n = min(n0 + (int64_t)v * kThreads, g.N - 1);   // tail threads recompute the last vector
        px[v] = img + vec_base(g, n);
        best[v] = INFINITY;
        bestj[v] = 0;
    }
    const int32_t D = g.D;
    for (int32_t k0 = 0; k0 < K; k0 += KT) {
        const int32_t kt = min(KT, K - k0);
        __syncthreads();
        for (int32_t i = threadIdx.x; i < KT * D; i += kThreads) {
            const int32_t j = i / D, d = i - j * D;
            tile[d * KT + j] = j < kt ? cent[(int64_t)(k0 + j) * D + d] : 0.0;
        }
        __syncthreads();
        for (int32_t jg = 0; jg < kt; jg += kJT) {   // KT is a multiple of kJT: the group stays inside the tile
            double acc[kVT][kJT];
#pragma unroll
            for (int v = 0; v < kVT; ++v)
#pragma unroll
                for (int jj = 0; jj < kJT; ++jj) acc[v][jj] = 0.0;
            const double *tp = tile + jg;
            for (int32_t r = 0; r < g.BS; ++r) {
                const int64_t ro = r * g.pitch;
                for (int32_t e = 0; e < g.rowlen; ++e, tp += KT) {
                    double c[kJT];
#pragma unroll
                    for (int q = 0; q < kJT / 2; ++q) {
                        const double2 two = reinterpret_cast<const double2 *>(tp)[q];
                        c[2 * q] = two.x;
                        c[2 * q + 1] = two.y;
                    }
#pragma unroll
                    for (int v = 0; v < kVT; ++v) {
                        const double x = (double)px[v][ro + e];
#pragma unroll
                        for (int jj = 0; jj < kJT; ++jj) {
                            const double t = x - c[jj];
                            acc[v][jj] = acc[v][jj] + t * t;
                        }
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < kJT; ++jj) {
                if (jg + jj < kt) {
#pragma unroll
                    for (int v = 0; v < kVT; ++v) {
                        if (acc[v][jj] < best[v]) {   // strict: the lowest j wins a tie
                            best[v] = acc[v][jj];
                            bestj[v] = k0 + jg + jj;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < kVT; ++v) {
        const int64_t n = n0 + (int64_t)v * kThreads;
        if (n < g.N) {
            if (changed && labels[n] != (uint16_t)bestj[v]) atomicAdd(changed, 1u);
            labels[n] = (uint16_t)bestj[v];
            if (dist) dist[n] = best[v];
        }
    }
}

int assign_tile(int32_t K, int32_t D)
{
    int kt = (kTileBytes / (8 * D)) & ~(kJT - 1);
    kt = std::max(kt, kJT);
    kt = std::min(kt, kMaxKT);
    return std::min(kt, (K + kJT - 1) & ~(kJT - 1));
}

int launch_assign(const uint8_t *img, const Geo &g, const double *cent, int32_t K, uint16_t *labels, double *dist,
                  unsigned int *changed, hipStream_t s)
{
    const int KT = assign_tile(K, g.D);
    const size_t lds = (size_t)KT * g.D * sizeof(double);   // <= 64 KiB: D <= 1024 with KT = 8
    if (lds > 48 * 1024) {
        const int rc = hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(vq_assign_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                                 "vq_assign_kernel LDS size");
        if (rc) return rc;
    }
    const int64_t per_block = (int64_t)kThreads * kVT;
    const int64_t blocks = (g.N + per_block - 1) / per_block;
    hipLaunchKernelGGL(vq_assign_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, s, img, g, cent, K, KT, labels,
                       dist, changed);
    return hip_check(hipGetLastError(), "vq_assign_kernel launch");
}

// dist[n] = the distance of vector n to the centroid its label names, in the assign kernel's arithmetic
__global__ __launch_bounds__(kThreads) void vq_label_dist_kernel(const uint8_t *__restrict__ img, Geo g,
                                                                 const double *__restrict__ cent, int32_t K,
                                                                 const uint16_t *__restrict__ labels,
                                                                 double *__restrict__ dist)
{
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= g.N) return;
    const int32_t lab = labels[n];
    if (lab >= K) {
        dist[n] = 0.0;
        return;
    }
    const uint8_t *p = img + vec_base(g, n);
    const double *c = cent + (int64_t)lab * g.D;
    double acc = 0.0;
    for (int32_t r = 0; r < g.BS; ++r)
        for (int32_t e = 0; e < g.rowlen; ++e) {
            const double t = (double)p[r * g.pitch + e] - c[r * g.rowlen + e];
            acc = acc + t * t;
        }
    dist[n] = acc;
}

// ---- accumulate ---------------------------------------------------------------
// Lanes run over the flattened (vector, element) pairs of the block's vectors, so
// neighbouring lanes add into different addresses.  Small codebooks (K * (D + 1)
// uint32 in LDS) are summed per block first -- a block holds at most kAccVectors
// vectors, so 255 * kAccVectors fits -- and flushed with one 64-bit atomic per
// non-zero entry; larger ones add into the global sums directly.
template <bool kLds>
__global__ __launch_bounds__(kThreads) void vq_accumulate_kernel(const uint8_t *__restrict__ img, Geo g,
                                                                 const uint16_t *__restrict__ labels, int32_t K,
                                                                 unsigned long long *__restrict__ sums,
                                                                 unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned int part[];   // K * D sums, then K counts
    const int32_t D = g.D;
    const int64_t n_begin = (int64_t)blockIdx.x * kAccVectors;
    const int32_t nv = (int32_t)min((int64_t)kAccVectors, g.N - n_begin);
    const int32_t entries = K * D + K;
    if (kLds) {
        for (int32_t i = threadIdx.x; i < entries; i += kThreads) part[i] = 0;
        __syncthreads();
    }
    for (int32_t i = threadIdx.x; i < nv * D; i += kThreads) {
        const int32_t v = i / D, d = i - v * D;
        const int64_t n = n_begin + v;
        const int32_t lab = labels[n];
        if (lab >= K) continue;
        const unsigned int x = img[vec_base(g, n) + elem_offset(g, d)];
        if (kLds) {
            atomicAdd(&part[lab * D + d], x);
            if (d == 0) atomicAdd(&part[K * D + lab], 1u);
        } else {
            atomicAdd(&sums[(int64_t)lab * D + d], (unsigned long long)x);
            if (d == 0) atomicAdd(&counts[lab], 1ull);
        }
    }
    if (kLds) {
        __syncthreads();
        for (int32_t i = threadIdx.x; i < entries; i += kThreads) {
            const unsigned int p = part[i];
            if (p) atomicAdd(i < K * D ? &sums[i] : &counts[i - K * D], (unsigned long long)p);
        }
    }
}

int launch_accumulate(const uint8_t *img, const Geo &g, const uint16_t *labels, int32_t K, int64_t *sums,
                      int64_t *counts, hipStream_t s)
{
    int rc = hip_check(hipMemsetAsync(sums, 0, (size_t)K * g.D * sizeof(int64_t), s), "hipMemsetAsync(sums)");
    if (rc) return rc;
    rc = hip_check(hipMemsetAsync(counts, 0, (size_t)K * sizeof(int64_t), s), "hipMemsetAsync(counts)");
    if (rc) return rc;
    const int64_t blocks = (g.N + kAccVectors - 1) / kAccVectors;
    const size_t lds = ((size_t)K * g.D + K) * sizeof(unsigned int);
    auto *us = reinterpret_cast<unsigned long long *>(sums);
    auto *uc = reinterpret_cast<unsigned long long *>(counts);
    if (lds <= (size_t)kAccLdsBytes)
        hipLaunchKernelGGL(vq_accumulate_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), lds, s, img, g, labels,
                           K, us, uc);
    else
        hipLaunchKernelGGL(vq_accumulate_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, img, g, labels,
                           K, us, uc);
    return hip_check(hipGetLastError(), "vq_accumulate_kernel launch");
}

// per-feature sum and sum of squares: m[d] = sum x, m[D + d] = sum x * x
__global__ __launch_bounds__(kThreads) void vq_moments_kernel(const uint8_t *__restrict__ img, Geo g,
                                                              unsigned long long *__restrict__ m)
{
    __shared__ unsigned long long part[2 * kMaxD];
    const int32_t D = g.D;
    const int64_t n_begin = (int64_t)blockIdx.x * kAccVectors;
    const int32_t nv = (int32_t)min((int64_t)kAccVectors, g.N - n_begin);
    for (int32_t i = threadIdx.x; i < 2 * D; i += kThreads) part[i] = 0;
    __syncthreads();
    for (int32_t i = threadIdx.x; i < nv * D; i += kThreads) {
        const int32_t v = i / D, d = i - v * D;
        const unsigned long long x = img[vec_base(g, n_begin + v) + elem_offset(g, d)];
        atomicAdd(&part[d], x);
        atomicAdd(&part[D + d], x * x);
    }
    __syncthreads();
    for (int32_t i = threadIdx.x; i < 2 * D; i += kThreads)
        if (part[i]) atomicAdd(&m[i], part[i]);
}

// ---- decode -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void vq_decode_kernel(const uint16_t *__restrict__ labels, Geo g,
                                                             const double *__restrict__ cent, int32_t K,
                                                             uint8_t *__restrict__ out, int32_t *__restrict__ bad)
{
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)g.H * g.pitch) return;
    const int64_t y = idx / g.pitch;
    const int32_t rem = (int32_t)(idx - y * g.pitch);
    const int32_t xp = rem / g.C, ch = rem - xp * g.C;
    const int64_t by = y / g.BS;
    const int32_t r = (int32_t)(y - by * g.BS);
    const int32_t bx = xp / g.BS;
    const int32_t e = (xp - bx * g.BS) * g.C + ch;
    const int32_t lab = labels[by * g.Wb + bx];
    if (lab >= K) {
        *bad = 1;
        out[idx] = 0;
        return;
    }
    const double c = cent[(int64_t)lab * g.D + r * g.rowlen + e];
    out[idx] = (uint8_t)(int16_t)(int32_t)c;   // truncation into int16, then the low byte
}

// ---- k-means++ ----------------------------------------------------------------
// A chunk is kThreads consecutive vectors (one block); every quantity is an
// integer, so no result depends on the chunking.
__device__ __forceinline__ int32_t int_dist(const uint8_t *p, const Geo &g, const uint8_t *cand)
{
    int32_t acc = 0;   // <= 255^2 * 1024
    for (int32_t r = 0; r < g.BS; ++r)
        for (int32_t e = 0; e < g.rowlen; ++e) {
            const int32_t t = (int32_t)p[r * g.pitch + e] - (int32_t)cand[r * g.rowlen + e];
            acc += t * t;
        }
    return acc;
}

// closest[n] = (first ? dist : min(closest[n], dist)) to vector `id`; chunk_sums[block] = sum of the chunk
__global__ __launch_bounds__(kThreads) void vq_pp_update_kernel(const uint8_t *__restrict__ img, Geo g, int64_t id,
                                                                int32_t first, int64_t *__restrict__ closest,
                                                                int64_t *__restrict__ chunk_sums)
{
    __shared__ uint8_t cand[kMaxD];
    __shared__ unsigned long long total;
    const int64_t cb = vec_base(g, id);
    for (int32_t d = threadIdx.x; d < g.D; d += kThreads) cand[d] = img[cb + elem_offset(g, d)];
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n < g.N) {
        int64_t v = int_dist(img + vec_base(g, n), g, cand);
        if (!first) v = min(v, closest[n]);
        closest[n] = v;
        atomicAdd(&total, (unsigned long long)v);
    }
    __syncthreads();
    if (threadIdx.x == 0 && chunk_sums) chunk_sums[blockIdx.x] = (int64_t)total;
}

struct LocateArgs {
    int64_t chunk[kMaxTrials];   // -1: no draw to locate (the potential is 0), the candidate is vector 0
    int64_t resid[kMaxTrials];   // the draw minus the sum of the chunks before
};

// cand[t] = the first index of chunk[t] whose running sum exceeds resid[t]
__global__ void vq_pp_locate_kernel(const int64_t *__restrict__ closest, int64_t N, LocateArgs a, int32_t T,
                                    int64_t *__restrict__ cand)
{
    const int32_t t = threadIdx.x;
    if (t >= T) return;
    if (a.chunk[t] < 0) {
        cand[t] = 0;
        return;
    }
    const int64_t lo = a.chunk[t] * kThreads, hi = min(N, lo + kThreads);
    int64_t run = 0, found = hi - 1;
    for (int64_t i = lo; i < hi; ++i) {
        run += closest[i];
        if (run > a.resid[t]) {
            found = i;
            break;
        }
    }
    cand[t] = found;
}

// partials[t * chunks + block] = sum over the chunk of min(closest[n], dist(x_n, x_cand[t]))
__global__ __launch_bounds__(kThreads) void vq_pp_trial_kernel(const uint8_t *__restrict__ img, Geo g,
                                                               const int64_t *__restrict__ closest,
                                                               const int64_t *__restrict__ cand, int32_t T,
                                                               int64_t *__restrict__ partials)
{
    extern __shared__ uint8_t cvec[];   // T * D candidate bytes
    __shared__ unsigned long long total[kMaxTrials];
    const int32_t D = g.D;
    for (int32_t i = threadIdx.x; i < T * D; i += kThreads) {
        const int32_t t = i / D, d = i - t * D;
        cvec[i] = img[vec_base(g, cand[t]) + elem_offset(g, d)];
    }
    if (threadIdx.x < kMaxTrials) total[threadIdx.x] = 0;
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n < g.N) {
        const uint8_t *p = img + vec_base(g, n);
        const int64_t cl = closest[n];
        for (int32_t t = 0; t < T; ++t) {
            const int64_t v = min(cl, (int64_t)int_dist(p, g, cvec + t * D));
            atomicAdd(&total[t], (unsigned long long)v);
        }
    }
    __syncthreads();
    if ((int32_t)threadIdx.x < T) partials[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = (int64_t)total[threadIdx.x];
}

// cent[c][d] = x[ids[c]][d]
__global__ __launch_bounds__(kThreads) void vq_gather_kernel(const uint8_t *__restrict__ img, Geo g,
                                                             const int64_t *__restrict__ ids, int32_t K,
                                                             double *__restrict__ cent)
{
    const int32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= K * g.D) return;
    const int32_t c = i / g.D, d = i - c * g.D;
    cent[i] = (double)img[vec_base(g, ids[c]) + elem_offset(g, d)];
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf()
    {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes) { return hip_check(hipMalloc(&p, bytes ? bytes : 1), "hipMalloc"); }
    template <class T>
    T *as() const
    {
        return static_cast<T *>(p);
    }
};

int to_host(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    const int rc = hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(D2H)");
    return rc ? rc : hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
}

uint64_t vq_draw(uint64_t seed, uint64_t step, uint64_t trial)
{
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (step * 16 + trial + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint64_t mulhi64(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }

int init_pp(const uint8_t *img, const Geo &g, int32_t K, uint64_t seed, double *cent_dev, int64_t *ids_host,
            hipStream_t s)
{
    const int T = 2 + (int)std::log((double)K);
    const int64_t chunks = (g.N + kThreads - 1) / kThreads;
    DevBuf closest, step_buf, ids_dev;   // step_buf: T candidate ids, then T * chunks partial sums
    int rc;
    if ((rc = closest.alloc((size_t)g.N * 8)) || (rc = step_buf.alloc((size_t)(T + T * chunks) * 8)) ||
        (rc = ids_dev.alloc((size_t)K * 8)))
        return rc;
    int64_t *cand_dev = step_buf.as<int64_t>(), *part_dev = cand_dev + T;
    std::vector<int64_t> host((size_t)(T + T * chunks)), sums((size_t)chunks), ids((size_t)K);

    ids[0] = (int64_t)mulhi64(vq_draw(seed, 0, 0), (uint64_t)g.N);
    hipLaunchKernelGGL(vq_pp_update_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, s, img, g, ids[0], 1,
                       closest.as<int64_t>(), part_dev);
    if ((rc = hip_check(hipGetLastError(), "vq_pp_update_kernel launch"))) return rc;
    if ((rc = to_host(sums.data(), part_dev, (size_t)chunks * 8, s))) return rc;

    for (int32_t c = 1; c < K; ++c) {
        int64_t pot = 0;
        for (int64_t v : sums) pot += v;
        LocateArgs la;
        for (int t = 0; t < kMaxTrials; ++t) la.chunk[t] = -1, la.resid[t] = 0;
        if (pot > 0) {
            for (int t = 0; t < T; ++t) {
                int64_t r = (int64_t)mulhi64(vq_draw(seed, (uint64_t)c, (uint64_t)t), (uint64_t)pot);   // in [0, pot)
                int64_t k = 0;
                while (r >= sums[(size_t)k]) r -= sums[(size_t)k++];   // ends: r < pot = sum of all chunks
                la.chunk[t] = k, la.resid[t] = r;
            }
        }
        hipLaunchKernelGGL(vq_pp_locate_kernel, dim3(1), dim3(64), 0, s, closest.as<int64_t>(), g.N, la, T, cand_dev);
        if ((rc = hip_check(hipGetLastError(), "vq_pp_locate_kernel launch"))) return rc;
        hipLaunchKernelGGL(vq_pp_trial_kernel, dim3((unsigned)chunks), dim3(kThreads), (size_t)T * g.D, s, img, g,
                           closest.as<int64_t>(), cand_dev, T, part_dev);
        if ((rc = hip_check(hipGetLastError(), "vq_pp_trial_kernel launch"))) return rc;
        if ((rc = to_host(host.data(), cand_dev, host.size() * 8, s))) return rc;
        int best = 0;
        int64_t best_pot = 0;
        for (int t = 0; t < T; ++t) {
            int64_t p = 0;
            for (int64_t k = 0; k < chunks; ++k) p += host[(size_t)(T + t * chunks + k)];
            if (t == 0 || p < best_pot) best = t, best_pot = p;
        }
        ids[(size_t)c] = host[(size_t)best];
        if (ids[(size_t)c] < 0 || ids[(size_t)c] >= g.N) return set_error(VCF_ERR_HIP, "k-means++ candidate out of range");
        std::copy_n(host.begin() + T + (int64_t)best * chunks, chunks, sums.begin());
        hipLaunchKernelGGL(vq_pp_update_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, s, img, g, ids[(size_t)c], 0,
                           closest.as<int64_t>(), (int64_t *)nullptr);
        if ((rc = hip_check(hipGetLastError(), "vq_pp_update_kernel launch"))) return rc;
    }
    if ((rc = hip_check(hipMemcpyAsync(ids_dev.p, ids.data(), (size_t)K * 8, hipMemcpyHostToDevice, s),
                        "hipMemcpyAsync(H2D)")))
        return rc;
    hipLaunchKernelGGL(vq_gather_kernel, dim3((unsigned)((K * g.D + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       img, g, ids_dev.as<int64_t>(), K, cent_dev);
    if ((rc = hip_check(hipGetLastError(), "vq_gather_kernel launch"))) return rc;
    if ((rc = hip_check(hipStreamSynchronize(s), "hipStreamSynchronize"))) return rc;   // ids is read by the copy
    if (ids_host) std::copy(ids.begin(), ids.end(), ids_host);
    return VCF_OK;
}

// tol * mean over d of var_d, var_d = (N * S2_d - S1_d^2) / N^2 from the integer moments
int abs_tolerance(const uint8_t *img, const Geo &g, double tol, double *out, hipStream_t s)
{
    DevBuf m;
    int rc;
    if ((rc = m.alloc((size_t)2 * g.D * 8))) return rc;
    if ((rc = hip_check(hipMemsetAsync(m.p, 0, (size_t)2 * g.D * 8, s), "hipMemsetAsync(moments)"))) return rc;
    const int64_t blocks = (g.N + kAccVectors - 1) / kAccVectors;
    hipLaunchKernelGGL(vq_moments_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, img, g,
                       m.as<unsigned long long>());
    if ((rc = hip_check(hipGetLastError(), "vq_moments_kernel launch"))) return rc;
    std::vector<uint64_t> h((size_t)2 * g.D);
    if ((rc = to_host(h.data(), m.p, h.size() * 8, s))) return rc;
    const unsigned __int128 n = (unsigned __int128)(uint64_t)g.N;
    const double nn = (double)(n * n);
    double total = 0.0;
    for (int32_t d = 0; d < g.D; ++d) {
        const unsigned __int128 num = n * h[(size_t)(g.D + d)] - (unsigned __int128)h[(size_t)d] * h[(size_t)d];
        total = total + (double)num / nn;
    }
    *out = tol * (total / (double)g.D);
    return VCF_OK;
}

}  // namespace

extern "C" {

int vcf_vq_assign(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size,
                  const double *centroids_dev, int32_t K, uint16_t *labels_dev, double *dist_dev, void *stream)
{
    Geo g;
    int rc;
    if ((rc = make_geo(H, W, C, block_size, &g)) || (rc = check_k(g, K))) return rc;
    if (!img_dev || !centroids_dev || !labels_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(centroids_dev, 8);
    VCF_REQUIRE_ALIGNED(labels_dev, 2);
    VCF_REQUIRE_ALIGNED(dist_dev, 8);
    return launch_assign(img_dev, g, centroids_dev, K, labels_dev, dist_dev, nullptr, (hipStream_t)stream);
}

int vcf_vq_accumulate(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size,
                      const uint16_t *labels_dev, int32_t K, int64_t *sums_dev, int64_t *counts_dev, void *stream)
{
    Geo g;
    int rc;
    if ((rc = make_geo(H, W, C, block_size, &g)) || (rc = check_k(g, K))) return rc;
    if (!img_dev || !labels_dev || !sums_dev || !counts_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(labels_dev, 2);
    VCF_REQUIRE_ALIGNED(sums_dev, 8);
    VCF_REQUIRE_ALIGNED(counts_dev, 8);
    return launch_accumulate(img_dev, g, labels_dev, K, sums_dev, counts_dev, (hipStream_t)stream);
}

int vcf_vq_init_pp(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size, int32_t K,
                   uint64_t seed, double *centroids_dev, int64_t *ids_host, void *stream)
{
    Geo g;
    int rc;
    if ((rc = make_geo(H, W, C, block_size, &g)) || (rc = check_k(g, K))) return rc;
    if (!img_dev || !centroids_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    return init_pp(img_dev, g, K, seed, centroids_dev, ids_host, (hipStream_t)stream);
}

int vcf_vq_fit(const uint8_t *img_dev, int32_t H, int32_t W, int32_t C, int32_t block_size, int32_t K, uint64_t seed,
               int32_t max_iter, double tol, const double *init_centroids_dev, double *centroids_dev,
               uint16_t *labels_dev, vcf_vq_report *report, void *stream)
{
    Geo g;
    int rc;
    if ((rc = make_geo(H, W, C, block_size, &g)) || (rc = check_k(g, K))) return rc;
    if (max_iter < 1) return set_error(VCF_ERR_INVALID, "max_iter must be at least 1 (got %d)", max_iter);
    if (!(tol >= 0.0)) return set_error(VCF_ERR_INVALID, "tol must be non-negative");
    if (!img_dev || !centroids_dev || !labels_dev || !report) return set_error(VCF_ERR_INVALID, "null buffer");
    const hipStream_t s = (hipStream_t)stream;
    const int32_t D = g.D;
    const size_t KD = (size_t)K * D;

    double tol_abs = 0.0;
    if ((rc = abs_tolerance(img_dev, g, tol, &tol_abs, s))) return rc;
    if (init_centroids_dev) {
        if (init_centroids_dev != centroids_dev &&
            (rc = hip_check(hipMemcpyAsync(centroids_dev, init_centroids_dev, KD * 8, hipMemcpyDeviceToDevice, s),
                            "hipMemcpyAsync(D2D)")))
            return rc;
    } else if ((rc = init_pp(img_dev, g, K, seed, centroids_dev, nullptr, s))) {
        return rc;
    }

    DevBuf sums_dev, counts_dev, dist_dev, changed_dev;
    if ((rc = sums_dev.alloc(KD * 8)) || (rc = counts_dev.alloc((size_t)K * 8)) ||
        (rc = dist_dev.alloc((size_t)g.N * 8)) || (rc = changed_dev.alloc(4)))
        return rc;
    std::vector<double> cent(KD), fresh(KD), dist;
    std::vector<int64_t> sums(KD), counts((size_t)K);
    std::vector<uint16_t> labels;
    std::vector<uint8_t> image;   // fetched only when a cluster is empty
    if ((rc = to_host(cent.data(), centroids_dev, KD * 8, s))) return rc;

    int32_t n_iter = 0, reason = VCF_VQ_STOP_MAX_ITER;
    int64_t relocations = 0;
    for (int32_t it = 0; it < max_iter; ++it) {
        unsigned int changed = 0;
        if ((rc = hip_check(hipMemsetAsync(changed_dev.p, 0, 4, s), "hipMemsetAsync(changed)"))) return rc;
        // the first pass has no labels to compare with: it always counts as changed
        if ((rc = launch_assign(img_dev, g, centroids_dev, K, labels_dev, dist_dev.as<double>(),
                                it ? changed_dev.as<unsigned int>() : nullptr, s)))
            return rc;
        if ((rc = launch_accumulate(img_dev, g, labels_dev, K, sums_dev.as<int64_t>(), counts_dev.as<int64_t>(), s)))
            return rc;
        if ((rc = hip_check(hipMemcpyAsync(sums.data(), sums_dev.p, KD * 8, hipMemcpyDeviceToHost, s), "D2H sums")) ||
            (rc = hip_check(hipMemcpyAsync(counts.data(), counts_dev.p, (size_t)K * 8, hipMemcpyDeviceToHost, s),
                            "D2H counts")) ||
            (rc = to_host(&changed, changed_dev.p, 4, s)))
            return rc;
        if (it == 0) changed = 1;

        // empty clusters take the vectors farthest from their own centroids (_relocate_empty_clusters_dense)
        std::vector<int32_t> empty;
        for (int32_t j = 0; j < K; ++j)
            if (counts[(size_t)j] == 0) empty.push_back(j);
        if (!empty.empty()) {
            dist.resize((size_t)g.N);
            labels.resize((size_t)g.N);
            if ((rc = to_host(dist.data(), dist_dev.p, (size_t)g.N * 8, s)) ||
                (rc = to_host(labels.data(), labels_dev, (size_t)g.N * 2, s)))
                return rc;
            if (image.empty()) {
                image.resize((size_t)g.H * (size_t)g.pitch);
                if ((rc = to_host(image.data(), img_dev, image.size(), s))) return rc;
            }
            std::vector<int64_t> order((size_t)g.N);
            std::iota(order.begin(), order.end(), (int64_t)0);
            const size_t take = std::min(empty.size(), order.size());
            std::partial_sort(order.begin(), order.begin() + (int64_t)take, order.end(), [&](int64_t a, int64_t b) {
                return dist[(size_t)a] > dist[(size_t)b] || (dist[(size_t)a] == dist[(size_t)b] && a < b);
            });
            for (size_t i = 0; i < take; ++i) {
                const int64_t far = order[i];
                if (!(dist[(size_t)far] > 0.0)) break;   // nothing left to take: the cluster keeps its centroid
                const int32_t to = empty[i], from = labels[(size_t)far];
                const int64_t by = far / g.Wb, bx = far - by * g.Wb;
                const uint8_t *p = image.data() + by * g.BS * g.pitch + bx * g.rowlen;
                for (int32_t d = 0; d < D; ++d) {
                    const int64_t x = p[(d / g.rowlen) * g.pitch + d % g.rowlen];
                    sums[(size_t)from * D + d] -= x;
                    sums[(size_t)to * D + d] = x;
                }
                counts[(size_t)to] = 1;
                counts[(size_t)from] -= 1;
                ++relocations;
            }
        }

        double shift = 0.0;
        for (int32_t j = 0; j < K; ++j)
            for (int32_t d = 0; d < D; ++d) {
                const size_t i = (size_t)j * D + d;
                fresh[i] = counts[(size_t)j] > 0 ? (double)sums[i] / (double)counts[(size_t)j] : cent[i];
                const double t = fresh[i] - cent[i];
                shift = shift + t * t;
            }
        cent.swap(fresh);
        if ((rc = hip_check(hipMemcpyAsync(centroids_dev, cent.data(), KD * 8, hipMemcpyHostToDevice, s), "H2D centroids")) ||
            (rc = hip_check(hipStreamSynchronize(s), "hipStreamSynchronize")))
            return rc;
        n_iter = it + 1;
        if (!changed) {
            reason = VCF_VQ_STOP_STRICT;
            break;
        }
        if (shift <= tol_abs) {
            reason = VCF_VQ_STOP_TOL;
            break;
        }
    }
    if (reason != VCF_VQ_STOP_STRICT &&
        (rc = launch_assign(img_dev, g, centroids_dev, K, labels_dev, dist_dev.as<double>(), nullptr, s)))
        return rc;
    // the inertia: distances to the returned centroids under the returned labels, summed in index order
    hipLaunchKernelGGL(vq_label_dist_kernel, dim3((unsigned)((g.N + kThreads - 1) / kThreads)), dim3(kThreads), 0, s,
                       img_dev, g, centroids_dev, K, labels_dev, dist_dev.as<double>());
    if ((rc = hip_check(hipGetLastError(), "vq_label_dist_kernel launch"))) return rc;
    dist.resize((size_t)g.N);
    if ((rc = to_host(dist.data(), dist_dev.p, (size_t)g.N * 8, s))) return rc;
    double inertia = 0.0;
    for (double v : dist) inertia = inertia + v;
    report->n_iter = n_iter;
    report->stop_reason = reason;
    report->relocations = relocations;
    report->inertia = inertia;
    report->tol_abs = tol_abs;
    return VCF_OK;
}

int vcf_vq_decode(const uint16_t *labels_dev, int32_t Hl, int32_t Wl, int32_t C, int32_t block_size,
                  const double *centroids_dev, int32_t K, uint8_t *img_dev, int32_t *bad_dev, void *stream)
{
    if (Hl < 1 || Wl < 1 || block_size < 1 || block_size > 16 || Hl > INT32_MAX / block_size ||
        Wl > INT32_MAX / block_size)
        return set_error(VCF_ERR_INVALID, "bad label shape %d x %d for block size %d", Hl, Wl, block_size);
    Geo g;
    int rc;
    if ((rc = make_geo(Hl * block_size, Wl * block_size, C, block_size, &g))) return rc;
    if (K < 1 || K > kMaxK) return set_error(VCF_ERR_INVALID, "1 <= K <= %d (got %d)", kMaxK, K);
    if (!labels_dev || !centroids_dev || !img_dev || !bad_dev) return set_error(VCF_ERR_INVALID, "null buffer");
    VCF_REQUIRE_ALIGNED(labels_dev, 2);
    VCF_REQUIRE_ALIGNED(centroids_dev, 8);
    VCF_REQUIRE_ALIGNED(bad_dev, 4);
    const int64_t n = (int64_t)g.H * g.pitch;
    hipLaunchKernelGGL(vq_decode_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, labels_dev, g, centroids_dev, K, img_dev, bad_dev);
    return hip_check(hipGetLastError(), "vq_decode_kernel launch");
}

}  // extern "C"
