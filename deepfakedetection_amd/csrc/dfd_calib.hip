// dfd_calib.hip — calibration of the classifier's probabilities on the device (ABI 150): the reliability bins of the top-label
// confidence with the Brier sum, and the negative log-likelihood of temperature-scaled logits with its first two derivatives in
// beta = 1 / T for many beta at once.  (Softmax / arg max of beta * z, dfd_softmax_argmax_t, is dfd_misc.hip's softmax kernel.)
//
// Both entry points are two-stage sums over rows (dfd_rowred.h: the row layouts, the launch shape, stage 2, the order of every sum):
//   dfd_calib_bins       k_rowred_zero   bins[M][3] and stats[4] = 0
//                        k_calib_bins    stage 1: int32 / 64-bit histogram in LDS per workgroup, flushed with dfd_count.h's count_add; the
//                                        workgroup's f64 Brier partial into ws[block]
//                        k_rowred_sum    stage 2
//   dfd_calib_nll        k_calib_nll     stage 1: every row is read once and held in registers while the beta loop runs; the
//                                        workgroup's f64 partials of {nll, g, h} per beta and its two int64 row counts into ws
//                        k_rowred_sum    stage 2
// J <= DFD_CALIB_THREAD_MAX_J takes the thread layout, wider rows the wave layout; at most DFD_CALIB_MAX_BLOCKS workgroups.
#include "dfd_count.h"

#define CALIB_WAVE_COLS (DFD_CALIB_MAX_J / 64)                      // columns a lane holds of the widest row
static_assert(DFD_CALIB_MAX_J % 64 == 0 && DFD_CALIB_THREAD_MAX_J <= 64, "a lane holds whole column strides");

static rowred_plan_t calib_plan(int n, int J) { return rowred_plan(n, J <= DFD_CALIB_THREAD_MAX_J, DFD_CALIB_MAX_BLOCKS); }

// One valid row into the workgroup's histogram: cc[b] += 1 (low word, rows) and, when the prediction is right, 2^32 (high word);
// sq[b] += q.  A workgroup sees fewer than 2^31 rows, so the low word never carries into the high one.
static __device__ __forceinline__ void calib_bin_row(float conf, bool right, const double* __restrict__ edge, int M,
                                                     unsigned long long* __restrict__ cc, unsigned long long* __restrict__ sq) {
    const double c = (double)conf;
    int lo = 0, hi = M - 1;                                             // the number of k in 1..M-1 with c > k / M: edge[] ascends
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c > edge[mid]) lo = mid; else hi = mid - 1;
    }
    atomicAdd(&cc[lo], right ? 0x100000001ull : 1ull);
    atomicAdd(&sq[lo], (unsigned long long)llrint(c * 4294967296.0));
}

template <int LAYOUT>
__global__ void __launch_bounds__(ROWRED_THREADS)
k_calib_bins(const float* __restrict__ probs, const int64_t* __restrict__ targets, int n, int J, int M, int64_t* __restrict__ bins,
             int64_t* __restrict__ stats, double* __restrict__ ws) {
    __shared__ double edge[DFD_CALIB_MAX_BINS];
    __shared__ unsigned long long cc[DFD_CALIB_MAX_BINS], sq[DFD_CALIB_MAX_BINS];
    __shared__ double red[ROWRED_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t < M) { edge[t] = (double)t / (double)M; cc[t] = 0; sq[t] = 0; }
    __syncthreads();
    long valid = 0, nonfinite = 0, oob = 0;
    double brier = 0.0;
    if (LAYOUT == DFD_CALIB_LAYOUT_THREAD) {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_THREAD; base < n; base += (long)gridDim.x * ROWRED_ROWS_THREAD) {
            const long i = base + t;
            if (i >= n) continue;
            const float* __restrict__ row = probs + i * J;
            const int64_t y = targets[i];
            float conf = row[0];
            int pred = 0;
            bool bad = f32_nonfinite(conf);
            for (int j = 1; j < J; ++j) {
                const float p = row[j];
                bad |= f32_nonfinite(p);
                if (p > conf) { conf = p; pred = j; }
            }
            if (bad) { ++nonfinite; continue; }
            if (y < 0 || y >= J) { ++oob; continue; }
            double b = 0.0;
            for (int j = 0; j < J; ++j) {
                const double d = (double)row[j] - (j == (int)y ? 1.0 : 0.0);
                b += d * d;
            }
            brier += b;
            ++valid;
            calib_bin_row(conf, pred == (int)y, edge, M, cc, sq);
        }
    } else {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_WAVE; base < n; base += (long)gridDim.x * ROWRED_ROWS_WAVE) {
            for (int r = 0; r < ROWRED_WAVE_ROWS; ++r) {
                const long i = base + w * ROWRED_WAVE_ROWS + r;              // wave-uniform
                if (i >= n) break;
                const float* __restrict__ row = probs + i * J;
                const int64_t y = targets[i];
                float conf = -INFINITY;
                int pred = 0x7fffffff;
                bool bad = false;
                for (int j = lane; j < J; j += 64) {
                    const float p = row[j];
                    bad |= f32_nonfinite(p);
                    if (p > conf) { conf = p; pred = j; }
                }
                if (__any(bad)) { if (lane == 0) ++nonfinite; continue; }
                if (y < 0 || y >= J) { if (lane == 0) ++oob; continue; }
                wave_first_argmax(conf, pred);
                for (int j = lane; j < J; j += 64) {                        // the lane's columns of every row: summed at the end
                    const double d = (double)row[j] - (j == (int)y ? 1.0 : 0.0);
                    brier += d * d;
                }
                if (lane == 0) {
                    ++valid;
                    calib_bin_row(conf, pred == (int)y, edge, M, cc, sq);
                }
            }
        }
    }
    brier = wave_sum(brier);
    valid = wave_sum(valid); nonfinite = wave_sum(nonfinite); oob = wave_sum(oob);
    if (lane == 0) {
        red[w] = brier;
        count_add(stats + 0, valid); count_add(stats + 1, nonfinite); count_add(stats + 2, oob);
    }
    __syncthreads();
    if (t == 0) {
        double s = red[0];
        for (int u = 1; u < ROWRED_WAVES; ++u) s += red[u];
        ws[blockIdx.x] = s;
    }
    if (t < M) {
        const unsigned long long c = cc[t];
        count_add(bins + t * 3 + 0, c & 0xffffffffull);
        count_add(bins + t * 3 + 1, c >> 32);
        count_add(stats + 3, c >> 32);
        count_add(bins + t * 3 + 2, sq[t]);
    }
}

extern "C" int dfd_calib_plan(int n, int J, int* out) {
    if (n < 0 || n > DFD_CALIB_MAX_N || J < 1 || J > DFD_CALIB_MAX_J || !out) return DFD_EINVAL;
    const rowred_plan_t p = calib_plan(n, J);
    out[0] = p.layout; out[1] = p.rows; out[2] = p.blocks; out[3] = p.trips;
    return DFD_OK;
}

extern "C" size_t dfd_calib_bins_ws(int n, int J) {
    if (n < 0 || n > DFD_CALIB_MAX_N || J < 1 || J > DFD_CALIB_MAX_J) return 0;
    return (size_t)calib_plan(n, J).blocks * sizeof(double);
}

extern "C" int dfd_calib_bins(const float* probs, const int64_t* targets, int n, int J, int M, void* ws, size_t ws_bytes, int64_t* bins,
                              int64_t* stats, double* brier, dfd_stream stream) {
    if (n < 0 || n > DFD_CALIB_MAX_N || J < 1 || J > DFD_CALIB_MAX_J || M < 1 || M > DFD_CALIB_MAX_BINS) return DFD_EINVAL;
    if (!ws || !bins || !stats || !brier || (n > 0 && (!probs || !targets))) return DFD_EINVAL;
    if (ws_bytes < dfd_calib_bins_ws(n, J)) return DFD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const rowred_plan_t p = calib_plan(n, J);
    double* part = (double*)ws;
    hipLaunchKernelGGL(k_rowred_zero<ROWRED_THREADS>, dim3(1), dim3(ROWRED_THREADS), 0, st, bins, M * 3, stats, 4, (int64_t*)nullptr, 0);
    if (p.layout == DFD_CALIB_LAYOUT_THREAD)
        hipLaunchKernelGGL(k_calib_bins<DFD_CALIB_LAYOUT_THREAD>, dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, probs, targets, n, J, M, bins,
                           stats, part);
    else
        hipLaunchKernelGGL(k_calib_bins<DFD_CALIB_LAYOUT_WAVE>, dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, probs, targets, n, J, M, bins,
                           stats, part);
    hipLaunchKernelGGL(k_rowred_sum<ROWRED_THREADS>, dim3(1), dim3(ROWRED_THREADS), 0, st, (const double*)part, 1, (const int64_t*)nullptr, 0,
                       p.blocks, p.trips, brier, (int64_t*)nullptr);
    return DFD_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ NLL(beta), dNLL/dbeta, d2NLL/dbeta2
// The terms of one row at one beta, from the lane's share (e, e z, e z^2 summed over its columns) of the wave-wide or thread-local sums
static __device__ __forceinline__ void calib_nll_terms(double s0, double s1, double s2, double m, double beta, double zy, double& t_nll,
                                                       double& t_g, double& t_h) {
    const double mean1 = s1 / s0, mean2 = s2 / s0;
    t_nll = m + log(s0) - beta * zy;
    t_g = mean1 - zy;
    t_h = mean2 - mean1 * mean1;
}

struct calib_betas_t { double v[DFD_CALIB_MAX_BETAS]; };                // by value in the launch: the caller's array is host memory

// acc: each wave's running sums [K][3] in LDS; after the butterfly every lane holds the trip's sum and lane c < 3 adds term c
template <int LAYOUT>
__global__ void __launch_bounds__(ROWRED_THREADS)
k_calib_nll(const float* __restrict__ logits, const int64_t* __restrict__ targets, int n, int J, const calib_betas_t betas, int K,
            double* __restrict__ part, int64_t* __restrict__ ipart) {
    __shared__ double acc[ROWRED_WAVES][DFD_CALIB_MAX_BETAS][3];
    __shared__ double sbeta[DFD_CALIB_MAX_BETAS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < ROWRED_WAVES * DFD_CALIB_MAX_BETAS * 3; i += ROWRED_THREADS) (&acc[0][0][0])[i] = 0.0;
    if (t < K) sbeta[t] = betas.v[t];
    __syncthreads();
    long nonfinite = 0, oob = 0;
    if (LAYOUT == DFD_CALIB_LAYOUT_THREAD) {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_THREAD; base < n; base += (long)gridDim.x * ROWRED_ROWS_THREAD) {
            const long i = base + t;                                        // the trip count is wave-uniform: base < n for the wave
            float z[DFD_CALIB_THREAD_MAX_J];
            bool ok = i < n;
            double zy = 0.0, zmax = 0.0;
            if (ok) {
                const float* __restrict__ row = logits + i * J;
                const int64_t y = targets[i];
                bool bad = false;
                float mx = -INFINITY, fy = 0.f;
#pragma unroll
                for (int j = 0; j < DFD_CALIB_THREAD_MAX_J; ++j) {
                    z[j] = j < J ? row[j] : 0.f;
                    if (j < J) { bad |= f32_nonfinite(z[j]); mx = fmaxf(mx, z[j]); if (j == (int)y) fy = z[j]; }
                }
                if (bad) { ++nonfinite; ok = false; }
                else if (y < 0 || y >= J) { ++oob; ok = false; }
                zy = (double)fy; zmax = (double)mx;
            }
            if (!__any(ok)) continue;
            for (int k = 0; k < K; ++k) {
                const double beta = sbeta[k];
                double t_nll = 0.0, t_g = 0.0, t_h = 0.0;
                if (ok) {
                    const double m = beta * zmax;                           // beta > 0: the largest beta * z_j is beta * max z
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
                    for (int j = 0; j < DFD_CALIB_THREAD_MAX_J; ++j) {
                        if (j < J) {
                            const double zj = (double)z[j], e = exp(beta * zj - m);
                            s0 += e; s1 += e * zj; s2 += e * (zj * zj);
                        }
                    }
                    calib_nll_terms(s0, s1, s2, m, beta, zy, t_nll, t_g, t_h);
                }
                t_nll = wave_sum(t_nll); t_g = wave_sum(t_g); t_h = wave_sum(t_h);
                if (lane < 3) acc[w][k][lane] += lane == 0 ? t_nll : (lane == 1 ? t_g : t_h);
            }
        }
    } else {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_WAVE; base < n; base += (long)gridDim.x * ROWRED_ROWS_WAVE) {
            for (int r = 0; r < ROWRED_WAVE_ROWS; ++r) {
                const long i = base + w * ROWRED_WAVE_ROWS + r;              // wave-uniform
                if (i >= n) break;
                const float* __restrict__ row = logits + i * J;
                const int64_t y = targets[i];
                float z[CALIB_WAVE_COLS];
                bool bad = false;
                float mx = -INFINITY;
#pragma unroll
                for (int c = 0; c < CALIB_WAVE_COLS; ++c) {
                    const int j = lane + 64 * c;
                    z[c] = j < J ? row[j] : 0.f;
                    if (j < J) { bad |= f32_nonfinite(z[c]); mx = fmaxf(mx, z[c]); }
                }
                if (__any(bad)) { if (lane == 0) ++nonfinite; continue; }
                if (y < 0 || y >= J) { if (lane == 0) ++oob; continue; }
                mx = wave_max(mx);
                const double zmax = (double)mx, zy = (double)row[y];
                for (int k = 0; k < K; ++k) {
                    const double beta = sbeta[k], m = beta * zmax;
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
                    for (int c = 0; c < CALIB_WAVE_COLS; ++c) {
                        if (lane + 64 * c < J) {
                            const double zj = (double)z[c], e = exp(beta * zj - m);
                            s0 += e; s1 += e * zj; s2 += e * (zj * zj);
                        }
                    }
                    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
                    double t_nll, t_g, t_h;
                    calib_nll_terms(s0, s1, s2, m, beta, zy, t_nll, t_g, t_h);
                    if (lane < 3) acc[w][k][lane] += lane == 0 ? t_nll : (lane == 1 ? t_g : t_h);
                }
            }
        }
    }
    __shared__ long icount[ROWRED_WAVES][2];
    rowred_stage1_store(acc, icount, K * 3, 3, nonfinite, oob, part, ipart);
}

extern "C" size_t dfd_calib_nll_ws(int n, int J, int K) {
    if (n < 0 || n > DFD_CALIB_MAX_N || J < 1 || J > DFD_CALIB_MAX_J || K < 1 || K > DFD_CALIB_MAX_BETAS) return 0;
    return (size_t)calib_plan(n, J).blocks * (size_t)(3 * K + 2) * 8;
}

extern "C" int dfd_calib_nll(const float* logits, const int64_t* targets, int n, int J, const double* betas, int K,
                             void* ws, size_t ws_bytes, double* out, int64_t* stats, dfd_stream stream) {
    if (n < 0 || n > DFD_CALIB_MAX_N || J < 1 || J > DFD_CALIB_MAX_J || K < 1 || K > DFD_CALIB_MAX_BETAS) return DFD_EINVAL;
    if (!betas || !ws || !out || !stats || (n > 0 && (!logits || !targets))) return DFD_EINVAL;
    for (int k = 0; k < K; ++k)
        if (!(betas[k] > 0.0) || !__builtin_isfinite(betas[k])) return DFD_EINVAL;
    if (ws_bytes < dfd_calib_nll_ws(n, J, K)) return DFD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const rowred_plan_t p = calib_plan(n, J);
    double* part = (double*)ws;
    int64_t* ipart = (int64_t*)(part + (size_t)p.blocks * 3 * K);
    calib_betas_t bv;
    for (int k = 0; k < DFD_CALIB_MAX_BETAS; ++k) bv.v[k] = k < K ? betas[k] : 1.0;
    if (p.layout == DFD_CALIB_LAYOUT_THREAD)
        hipLaunchKernelGGL(k_calib_nll<DFD_CALIB_LAYOUT_THREAD>, dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, logits, targets, n, J, bv, K,
                           part, ipart);
    else
        hipLaunchKernelGGL(k_calib_nll<DFD_CALIB_LAYOUT_WAVE>, dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, logits, targets, n, J, bv, K,
                           part, ipart);
    hipLaunchKernelGGL(k_rowred_sum<ROWRED_THREADS>, dim3(1), dim3(ROWRED_THREADS), 0, st, (const double*)part, 3 * K, (const int64_t*)ipart, 2,
                       p.blocks, p.trips, out, stats);
    return DFD_CHECK_LAUNCH();
}
