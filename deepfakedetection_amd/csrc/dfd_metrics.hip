// dfd_metrics.hip — exact evaluation metrics on the device (ABI 146): the ROC curve of sorted scores with its Mann-Whitney rank
// statistic, a threshold sweep over that curve, and a confusion matrix.  Everything here is integer counting, so every result is
// exact and independent of the order in which workgroups finish; the only atomics are integer adds.  The block scan, the workgroup
// sum, the counter flush and the tie-group rule are dfd_count.h's.
//
// No workgroup ever waits for another one: whatever depends on another workgroup's result is a later launch on the same stream.
//   dfd_roc_curve   k_roc_tile_sums   one workgroup per tile of DFD_ROC_TILE scores: positives, negatives, group ends, non-finite
//                   k_roc_scan        ONE workgroup of DFD_ROC_SCAN_WIDTH threads: exclusive prefix of the tile totals in place (a loop
//                                     with a carry when there are more tiles than threads), P / N / G / nonfinite, two_u = 0
//                   k_roc_write       one workgroup per tile: block scan of the three flags, the compacted thr / cum_pos / cum_neg
//                   k_roc_two_u       grid-stride over the G groups (G read on the device), one 64-bit integer add per workgroup
//   dfd_roc_sweep   k_roc_sweep       one thread per cut: lower bound in thr[0..G) in f64
//   dfd_confusion   k_confusion_lds   J <= DFD_CONFUSION_LDS_MAX_J: int32 histogram in LDS per workgroup, flushed with 64-bit adds
//                   k_confusion_glb   above: one 64-bit add per sample
// A tile is 256 threads x 8 consecutive scores.  The loads are lane-strided (coalesced); each thread then reads the flag bytes of its
// own 8 consecutive scores from LDS as one 8-byte word, so the scan runs over 256 thread totals: one wave scan and a 4-entry sum.
#include "dfd_count.h"

#define ROC_THREADS 256
#define ROC_PER_THREAD (DFD_ROC_TILE / ROC_THREADS)
static_assert(ROC_PER_THREAD == 8, "a thread reads its flags as one 8-byte word");
static_assert(DFD_ROC_SCAN_WIDTH % 64 == 0 && DFD_ROC_SCAN_WIDTH <= 1024, "whole waves, one workgroup");

#define ROC_F_POS 1u
#define ROC_F_NEG 2u
#define ROC_F_END 4u
#define ROC_F_NONFINITE 8u

// the flags of score i (i < n): which class it counts for, whether its tie group ends with it, whether it is NaN or +-inf
static __device__ __forceinline__ unsigned roc_flags(const float* __restrict__ score, const int64_t* __restrict__ label, int i, int n,
                                                     int64_t positive) {
    const float s = score[i];
    const bool last = i == n - 1;
    unsigned f = label[i] == positive ? ROC_F_POS : ROC_F_NEG;
    if (tie_group_ends(s, last ? 0.f : score[i + 1], last)) f |= ROC_F_END;
    if (f32_nonfinite(s)) f |= ROC_F_NONFINITE;
    return f;
}

// ws: int32 [4][ntiles] = positives, negatives, group ends, non-finite scores of every tile
__global__ void __launch_bounds__(ROC_THREADS)
k_roc_tile_sums(const float* __restrict__ score, const int64_t* __restrict__ label, int n, int64_t positive, int* __restrict__ ws,
                int ntiles) {
    __shared__ int red[4 * 4];
    const int t = threadIdx.x, base = blockIdx.x * DFD_ROC_TILE;
    int c[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < ROC_PER_THREAD; ++j) {
        const int i = base + j * ROC_THREADS + t;
        if (i < n) {
            const unsigned f = roc_flags(score, label, i, n, positive);
            c[0] += f & 1u; c[1] += (f >> 1) & 1u; c[2] += (f >> 2) & 1u; c[3] += (f >> 3) & 1u;
        }
    }
    int total[4];
    block_scan_excl<4, ROC_THREADS / 64>(c, total, red);
    if (t < 4) ws[t * ntiles + blockIdx.x] = total[t];
}

__global__ void __launch_bounds__(DFD_ROC_SCAN_WIDTH)
k_roc_scan(int* __restrict__ ws, int ntiles, int64_t* __restrict__ stats) {
    __shared__ int red[(DFD_ROC_SCAN_WIDTH / 64) * 4];
    const int t = threadIdx.x;
    int carry[4] = {0, 0, 0, 0};
    for (int base = 0; base < ntiles; base += DFD_ROC_SCAN_WIDTH) {        // uniform trip count: the barriers inside are safe
        const int i = base + t;
        int v[4], total[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i < ntiles ? ws[k * ntiles + i] : 0;
        block_scan_excl<4, DFD_ROC_SCAN_WIDTH / 64>(v, total, red);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i < ntiles) ws[k * ntiles + i] = carry[k] + v[k];
            carry[k] += total[k];
        }
    }
    if (t < 4) stats[t] = carry[t];                                        // P, N, G, nonfinite
    if (t == 4) stats[4] = 0;                                              // two_u: k_roc_two_u adds to it
}

__global__ void __launch_bounds__(ROC_THREADS)
k_roc_write(const float* __restrict__ score, const int64_t* __restrict__ label, int n, int64_t positive, const int* __restrict__ ws,
            int ntiles, float* __restrict__ thr, int64_t* __restrict__ cum_pos, int64_t* __restrict__ cum_neg) {
    __shared__ __attribute__((aligned(8))) unsigned char flags[DFD_ROC_TILE];
    __shared__ float tile[DFD_ROC_TILE];
    __shared__ int red[4 * 3];
    const int t = threadIdx.x, base = blockIdx.x * DFD_ROC_TILE;
#pragma unroll
    for (int j = 0; j < ROC_PER_THREAD; ++j) {
        const int e = j * ROC_THREADS + t, i = base + e;
        unsigned f = 0;
        float s = 0.f;
        if (i < n) { f = roc_flags(score, label, i, n, positive); s = score[i]; }
        flags[e] = (unsigned char)f;
        tile[e] = s;
    }
    __syncthreads();
    const unsigned long long mine = *reinterpret_cast<const unsigned long long*>(flags + t * ROC_PER_THREAD);
    int c[3] = {0, 0, 0}, total[3];
#pragma unroll
    for (int j = 0; j < ROC_PER_THREAD; ++j) {
        const unsigned f = (unsigned)(mine >> (8 * j)) & 0xffu;
        c[0] += f & 1u; c[1] += (f >> 1) & 1u; c[2] += (f >> 2) & 1u;
    }
    block_scan_excl<3, ROC_THREADS / 64>(c, total, red);
    int pos = ws[blockIdx.x] + c[0], neg = ws[ntiles + blockIdx.x] + c[1], g = ws[2 * ntiles + blockIdx.x] + c[2];
#pragma unroll
    for (int j = 0; j < ROC_PER_THREAD; ++j) {
        const unsigned f = (unsigned)(mine >> (8 * j)) & 0xffu;
        pos += f & 1u;
        neg += (f >> 1) & 1u;
        if (f & ROC_F_END) {                                               // only set for i < n, and then g < G <= n
            thr[g] = tile[t * ROC_PER_THREAD + j];
            cum_pos[g] = pos;
            cum_neg[g] = neg;
            ++g;
        }
    }
}

// two_u = sum over groups of p_g * (cum_neg[g - 1] + cum_neg[g]); below 2^56 for n <= 2^28
__global__ void __launch_bounds__(ROC_THREADS)
k_roc_two_u(const int64_t* __restrict__ cum_pos, const int64_t* __restrict__ cum_neg, int64_t* __restrict__ stats, int cap) {
    __shared__ unsigned long long red[ROC_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t G64 = stats[2];
    const int G = (int)(G64 < 0 ? 0 : (G64 > cap ? cap : G64));
    unsigned long long acc = 0;
    for (int g = blockIdx.x * ROC_THREADS + t; g < G; g += gridDim.x * ROC_THREADS) {
        const int64_t p0 = g ? cum_pos[g - 1] : 0, n0 = g ? cum_neg[g - 1] : 0;
        acc += (unsigned long long)(cum_pos[g] - p0) * (unsigned long long)(n0 + cum_neg[g]);
    }
    acc = block_sum<ROC_THREADS / 64>(acc, red);
    if (t == 0) count_add(stats + 4, acc);
}

extern "C" size_t dfd_roc_ws(int n) {
    if (n < 0 || n > DFD_ROC_MAX_N) return 0;
    const size_t ntiles = ((size_t)n + DFD_ROC_TILE - 1) / DFD_ROC_TILE;
    return (ntiles ? ntiles : 1) * 4 * sizeof(int);
}

extern "C" int dfd_roc_curve(const float* score, const int64_t* label, int n, int64_t positive, void* ws, size_t ws_bytes, float* thr,
                             int64_t* cum_pos, int64_t* cum_neg, int64_t* stats, dfd_stream stream) {
    if (n < 0 || n > DFD_ROC_MAX_N || !ws || !stats) return DFD_EINVAL;
    if (n > 0 && (!score || !label || !thr || !cum_pos || !cum_neg)) return DFD_EINVAL;
    if (ws_bytes < dfd_roc_ws(n)) return DFD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (n + DFD_ROC_TILE - 1) / DFD_ROC_TILE;
    int* w = (int*)ws;
    if (n > 0) hipLaunchKernelGGL(k_roc_tile_sums, dim3(ntiles), dim3(ROC_THREADS), 0, st, score, label, n, positive, w, ntiles);
    hipLaunchKernelGGL(k_roc_scan, dim3(1), dim3(DFD_ROC_SCAN_WIDTH), 0, st, w, ntiles, stats);
    if (n > 0) {
        hipLaunchKernelGGL(k_roc_write, dim3(ntiles), dim3(ROC_THREADS), 0, st, score, label, n, positive, (const int*)w, ntiles, thr,
                           cum_pos, cum_neg);
        const int blocks = (n + ROC_THREADS - 1) / ROC_THREADS;
        hipLaunchKernelGGL(k_roc_two_u, dim3(blocks < 1024 ? blocks : 1024), dim3(ROC_THREADS), 0, st, (const int64_t*)cum_pos,
                           (const int64_t*)cum_neg, stats, n);
    }
    return DFD_CHECK_LAUNCH();
}

// tp[k] = #{positive, score >= cut[k]} = P - cum_pos[lo - 1], lo = the first group whose score, promoted to f64, is >= cut[k]
__global__ void __launch_bounds__(256)
k_roc_sweep(const float* __restrict__ thr, const int64_t* __restrict__ cum_pos, const int64_t* __restrict__ cum_neg,
            const int64_t* __restrict__ stats, int cap, const double* __restrict__ cuts, int T, int64_t* __restrict__ tp,
            int64_t* __restrict__ fp) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= T) return;
    const int64_t P = stats[0], N = stats[1], G64 = stats[2];
    const int G = (int)(G64 < 0 ? 0 : (G64 > cap ? cap : G64));
    const double cut = cuts[k];
    int lo = 0, hi = G;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((double)thr[mid] >= cut) hi = mid; else lo = mid + 1;
    }
    tp[k] = P - (lo ? cum_pos[lo - 1] : 0);
    fp[k] = N - (lo ? cum_neg[lo - 1] : 0);
}

extern "C" int dfd_roc_sweep(const float* thr, const int64_t* cum_pos, const int64_t* cum_neg, const int64_t* stats, int cap,
                             const double* cuts, int T, int64_t* tp, int64_t* fp, dfd_stream stream) {
    if (T < 1 || T > DFD_ROC_MAX_CUTS || cap < 0 || cap > DFD_ROC_MAX_N || !stats || !cuts || !tp || !fp) return DFD_EINVAL;
    if (cap > 0 && (!thr || !cum_pos || !cum_neg)) return DFD_EINVAL;
    hipLaunchKernelGGL(k_roc_sweep, dim3((T + 255) / 256), dim3(256), 0, (hipStream_t)stream, thr, cum_pos, cum_neg, stats, cap, cuts, T,
                       tp, fp);
    return DFD_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ confusion matrix
#define CONF_THREADS 256
#define CONF_PER_BLOCK (CONF_THREADS * 16)
#define CONF_MAX_BLOCKS 512

__global__ void __launch_bounds__(CONF_THREADS)
k_confusion_zero(int64_t* __restrict__ counts, int cells, int64_t* __restrict__ oob) {
    const int i = blockIdx.x * CONF_THREADS + threadIdx.x;
    if (i < cells) counts[i] = 0;
    if (i == 0) *oob = 0;
}

// int32 cells in LDS: a workgroup sees fewer than 2^31 samples
__global__ void __launch_bounds__(CONF_THREADS)
k_confusion_lds(const int64_t* __restrict__ truth, const int64_t* __restrict__ pred, int n, int J, int64_t* __restrict__ counts,
                int64_t* __restrict__ oob) {
    extern __shared__ __attribute__((aligned(16))) int hist[];
    const int t = threadIdx.x, cells = J * J;
    for (int i = t; i < cells; i += CONF_THREADS) hist[i] = 0;
    __syncthreads();
    int bad = 0;
    for (long i = (long)blockIdx.x * CONF_THREADS + t; i < n; i += (long)gridDim.x * CONF_THREADS) {
        const int64_t a = truth[i], b = pred[i];
        if (a < 0 || a >= J || b < 0 || b >= J) ++bad;
        else atomicAdd(&hist[(int)a * J + (int)b], 1);
    }
    count_add(oob, bad);
    __syncthreads();
    for (int i = t; i < cells; i += CONF_THREADS) count_add(counts + i, hist[i]);
}

__global__ void __launch_bounds__(CONF_THREADS)
k_confusion_glb(const int64_t* __restrict__ truth, const int64_t* __restrict__ pred, int n, int J, int64_t* __restrict__ counts,
                int64_t* __restrict__ oob) {
    int bad = 0;
    for (long i = (long)blockIdx.x * CONF_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * CONF_THREADS) {
        const int64_t a = truth[i], b = pred[i];
        if (a < 0 || a >= J || b < 0 || b >= J) ++bad;
        else count_add(counts + (long)a * J + b, 1);
    }
    count_add(oob, bad);
}

extern "C" int dfd_confusion(const int64_t* truth, const int64_t* pred, int n, int J, int64_t* counts, int64_t* oob, dfd_stream stream) {
    if (n < 0 || J < 1 || J > DFD_CONFUSION_MAX_J || !counts || !oob) return DFD_EINVAL;
    if (n > 0 && (!truth || !pred)) return DFD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int cells = J * J;
    hipLaunchKernelGGL(k_confusion_zero, dim3((cells + CONF_THREADS - 1) / CONF_THREADS), dim3(CONF_THREADS), 0, st, counts, cells, oob);
    if (n > 0) {
        int blocks = (n + CONF_PER_BLOCK - 1) / CONF_PER_BLOCK;
        if (blocks > CONF_MAX_BLOCKS) blocks = CONF_MAX_BLOCKS;
        if (J <= DFD_CONFUSION_LDS_MAX_J) {
            dfd_allow_lds_once<k_confusion_lds>(DFD_CONFUSION_LDS_MAX_J * DFD_CONFUSION_LDS_MAX_J * (int)sizeof(int));
            hipLaunchKernelGGL(k_confusion_lds, dim3(blocks), dim3(CONF_THREADS), (size_t)cells * sizeof(int), st, truth, pred, n, J,
                               counts, oob);
        } else {
            hipLaunchKernelGGL(k_confusion_glb, dim3(blocks), dim3(CONF_THREADS), 0, st, truth, pred, n, J, counts, oob);
        }
    }
    return DFD_CHECK_LAUNCH();
}
