// dfd_calib.hip — calibration of the classifier's probabilities on the device (ABI 150): the reliability bins of the top-label
// confidence with the Brier sum, the negative log-likelihood of temperature-scaled logits with its first two derivatives in
// beta = 1 / T for many beta at once, and softmax / arg max of beta * z.
//
// No workgroup ever waits for another one: whatever depends on another workgroup's result is a later launch on the same stream.
//   dfd_calib_bins       k_calib_zero    bins[M][3] and stats[4] = 0
//                        k_calib_bins    stage 1: int32 / 64-bit histogram in LDS per workgroup, flushed with 64-bit integer adds; the
//                                        workgroup's f64 Brier partial into ws[block]
//                        k_calib_sum     stage 2, ONE workgroup: the partials in index order
//   dfd_calib_nll        k_calib_nll     stage 1: every row is read once and held in registers while the beta loop runs; the
//                                        workgroup's f64 partials of {nll, g, h} per beta and its two int64 row counts into ws
//                        k_calib_sum     stage 2, ONE workgroup: the partials in index order
//   dfd_softmax_argmax_t k_softmax_argmax_t   dfd_softmax_argmax's kernel with one multiplication by beta in front of each exp
// Row layouts (calib_plan): J <= DFD_CALIB_THREAD_MAX_J gives every thread one row of a chunk of CALIB_ROWS_THREAD rows; above
// it every wave takes CALIB_WAVE_ROWS consecutive rows of a chunk of CALIB_ROWS_WAVE, lane l holding columns l, l + 64, ...
// Stage 1 runs min(chunks, DFD_CALIB_MAX_BLOCKS) workgroups, workgroup b taking chunks b, b + blocks, ...  The integer results
// are sums of integers; the f64 results are summed in an order that (n, J) alone fixes: lanes by an xor butterfly, trips and
// waves in index order, workgroups by k_calib_sum.  Equal inputs give equal bits.
#include "dfd_common.h"

#define CALIB_THREADS 256
#define CALIB_WAVES (CALIB_THREADS / 64)
#define CALIB_ROWS_THREAD CALIB_THREADS                             // rows per chunk, one thread per row
#define CALIB_WAVE_ROWS 8                                           // consecutive rows per wave and chunk, one wave per row
#define CALIB_ROWS_WAVE (CALIB_WAVES * CALIB_WAVE_ROWS)
#define CALIB_WAVE_COLS (DFD_CALIB_MAX_J / 64)                      // columns a lane holds of the widest row
static_assert(DFD_CALIB_MAX_J % 64 == 0 && DFD_CALIB_THREAD_MAX_J <= 64, "a lane holds whole column strides");
static_assert(DFD_CALIB_STAGE2_WIDTH == 64, "stage 2 sums one output per wave trip");

struct calib_plan_t { int layout, rows, blocks, trips; };

static calib_plan_t calib_plan(int n, int J) {
    calib_plan_t p;
    p.layout = J <= DFD_CALIB_THREAD_MAX_J ? DFD_CALIB_LAYOUT_THREAD : DFD_CALIB_LAYOUT_WAVE;
    p.rows = p.layout == DFD_CALIB_LAYOUT_THREAD ? CALIB_ROWS_THREAD : CALIB_ROWS_WAVE;
    const long chunks = ((long)n + p.rows - 1) / p.rows;
    p.blocks = (int)(chunks < 1 ? 1 : (chunks > DFD_CALIB_MAX_BLOCKS ? DFD_CALIB_MAX_BLOCKS : chunks));
    p.trips = (p.blocks + DFD_CALIB_STAGE2_WIDTH - 1) / DFD_CALIB_STAGE2_WIDTH;
    return p;
}

static __device__ __forceinline__ bool calib_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

static __device__ __forceinline__ double wave_sum_f64(double v) {       // every lane ends with the same bits: a + b == b + a
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
static __device__ __forceinline__ long wave_sum_i64(long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(CALIB_THREADS)
k_calib_zero(int64_t* __restrict__ bins, int cells, int64_t* __restrict__ stats) {
    const int t = threadIdx.x;
    if (t < cells) bins[t] = 0;
    if (t < 4) stats[t] = 0;
}

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
__global__ void __launch_bounds__(CALIB_THREADS)
k_calib_bins(const float* __restrict__ probs, const int64_t* __restrict__ targets, int n, int J, int M, int64_t* __restrict__ bins,
             int64_t* __restrict__ stats, double* __restrict__ ws) {
    __shared__ double edge[DFD_CALIB_MAX_BINS];
    __shared__ unsigned long long cc[DFD_CALIB_MAX_BINS], sq[DFD_CALIB_MAX_BINS];
    __shared__ double red[CALIB_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t < M) { edge[t] = (double)t / (double)M; cc[t] = 0; sq[t] = 0; }
    __syncthreads();
    long valid = 0, nonfinite = 0, oob = 0;
    double brier = 0.0;
    if (LAYOUT == DFD_CALIB_LAYOUT_THREAD) {
        for (long base = (long)blockIdx.x * CALIB_ROWS_THREAD; base < n; base += (long)gridDim.x * CALIB_ROWS_THREAD) {
            const long i = base + t;
            if (i >= n) continue;
            const float* __restrict__ row = probs + i * J;
            const int64_t y = targets[i];
            float conf = row[0];
            int pred = 0;
            bool bad = calib_nonfinite(conf);
            for (int j = 1; j < J; ++j) {
                const float p = row[j];
                bad |= calib_nonfinite(p);
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
        for (long base = (long)blockIdx.x * CALIB_ROWS_WAVE; base < n; base += (long)gridDim.x * CALIB_ROWS_WAVE) {
            for (int r = 0; r < CALIB_WAVE_ROWS; ++r) {
                const long i = base + w * CALIB_WAVE_ROWS + r;              // wave-uniform
                if (i >= n) break;
                const float* __restrict__ row = probs + i * J;
                const int64_t y = targets[i];
                float conf = -INFINITY;
                int pred = 0x7fffffff;
                bool bad = false;
                for (int j = lane; j < J; j += 64) {
                    const float p = row[j];
                    bad |= calib_nonfinite(p);
                    if (p > conf) { conf = p; pred = j; }
                }
                if (__any(bad)) { if (lane == 0) ++nonfinite; continue; }
                if (y < 0 || y >= J) { if (lane == 0) ++oob; continue; }
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const float oc = __shfl_xor(conf, o, 64);
                    const int op = __shfl_xor(pred, o, 64);
                    if (oc > conf || (oc == conf && op < pred)) { conf = oc; pred = op; }
                }
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
    brier = wave_sum_f64(brier);
    valid = wave_sum_i64(valid); nonfinite = wave_sum_i64(nonfinite); oob = wave_sum_i64(oob);
    if (lane == 0) {
        red[w] = brier;
        if (valid) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 0), (unsigned long long)valid);
        if (nonfinite) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 1), (unsigned long long)nonfinite);
        if (oob) atomicAdd(reinterpret_cast<unsigned long long*>(stats + 2), (unsigned long long)oob);
    }
    __syncthreads();
    if (t == 0) {
        double s = red[0];
        for (int u = 1; u < CALIB_WAVES; ++u) s += red[u];
        ws[blockIdx.x] = s;
    }
    if (t < M) {
        const unsigned long long c = cc[t], q = sq[t];
        if (c & 0xffffffffull) atomicAdd(reinterpret_cast<unsigned long long*>(bins + t * 3 + 0), c & 0xffffffffull);
        if (c >> 32) {
            atomicAdd(reinterpret_cast<unsigned long long*>(bins + t * 3 + 1), c >> 32);
            atomicAdd(reinterpret_cast<unsigned long long*>(stats + 3), c >> 32);
        }
        if (q) atomicAdd(reinterpret_cast<unsigned long long*>(bins + t * 3 + 2), q);
    }
}

// Stage 2, one workgroup: out[o] = the sum over b < blocks of part[o * blocks + b], o < nf (f64) — wave w takes o = w, w + 4, ...,
// its lanes the partials lane, lane + 64, ... in `trips` trips, then the butterfly — and iout[o] likewise over ipart (int64), o < ni.
__global__ void __launch_bounds__(CALIB_THREADS)
k_calib_sum(const double* __restrict__ part, int nf, const int64_t* __restrict__ ipart, int ni, int blocks, int trips,
            double* __restrict__ out, int64_t* __restrict__ iout) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = w; o < nf; o += CALIB_WAVES) {
        double s = 0.0;
        for (int trip = 0; trip < trips; ++trip) {
            const int b = trip * DFD_CALIB_STAGE2_WIDTH + lane;
            if (b < blocks) s += part[(long)o * blocks + b];
        }
        s = wave_sum_f64(s);
        if (lane == 0) out[o] = s;
    }
    for (int o = w; o < ni; o += CALIB_WAVES) {
        long s = 0;
        for (int trip = 0; trip < trips; ++trip) {
            const int b = trip * DFD_CALIB_STAGE2_WIDTH + lane;
            if (b < blocks) s += ipart[(long)o * blocks + b];
        }
        s = wave_sum_i64(s);
        if (lane == 0) iout[o] = s;
    }
}

extern "C" int dfd_calib_plan(int n, int J, int* out) {
    if (n < 0 || n > DFD_CALIB_MAX_N || J < 1 || J > DFD_CALIB_MAX_J || !out) return DFD_EINVAL;
    const calib_plan_t p = calib_plan(n, J);
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
    const calib_plan_t p = calib_plan(n, J);
    double* part = (double*)ws;
    hipLaunchKernelGGL(k_calib_zero, dim3(1), dim3(CALIB_THREADS), 0, st, bins, M * 3, stats);
    if (p.layout == DFD_CALIB_LAYOUT_THREAD)
        hipLaunchKernelGGL(k_calib_bins<DFD_CALIB_LAYOUT_THREAD>, dim3(p.blocks), dim3(CALIB_THREADS), 0, st, probs, targets, n, J, M, bins,
                           stats, part);
    else
        hipLaunchKernelGGL(k_calib_bins<DFD_CALIB_LAYOUT_WAVE>, dim3(p.blocks), dim3(CALIB_THREADS), 0, st, probs, targets, n, J, M, bins,
                           stats, part);
    hipLaunchKernelGGL(k_calib_sum, dim3(1), dim3(CALIB_THREADS), 0, st, (const double*)part, 1, (const int64_t*)nullptr, 0, p.blocks,
                       p.trips, brier, (int64_t*)nullptr);
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
__global__ void __launch_bounds__(CALIB_THREADS)
k_calib_nll(const float* __restrict__ logits, const int64_t* __restrict__ targets, int n, int J, const calib_betas_t betas, int K,
            double* __restrict__ part, int64_t* __restrict__ ipart) {
    __shared__ double acc[CALIB_WAVES][DFD_CALIB_MAX_BETAS][3];
    __shared__ double sbeta[DFD_CALIB_MAX_BETAS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < CALIB_WAVES * DFD_CALIB_MAX_BETAS * 3; i += CALIB_THREADS) (&acc[0][0][0])[i] = 0.0;
    if (t < K) sbeta[t] = betas.v[t];
    __syncthreads();
    long nonfinite = 0, oob = 0;
    if (LAYOUT == DFD_CALIB_LAYOUT_THREAD) {
        for (long base = (long)blockIdx.x * CALIB_ROWS_THREAD; base < n; base += (long)gridDim.x * CALIB_ROWS_THREAD) {
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
                    if (j < J) { bad |= calib_nonfinite(z[j]); mx = fmaxf(mx, z[j]); if (j == (int)y) fy = z[j]; }
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
                t_nll = wave_sum_f64(t_nll); t_g = wave_sum_f64(t_g); t_h = wave_sum_f64(t_h);
                if (lane < 3) acc[w][k][lane] += lane == 0 ? t_nll : (lane == 1 ? t_g : t_h);
            }
        }
    } else {
        for (long base = (long)blockIdx.x * CALIB_ROWS_WAVE; base < n; base += (long)gridDim.x * CALIB_ROWS_WAVE) {
            for (int r = 0; r < CALIB_WAVE_ROWS; ++r) {
                const long i = base + w * CALIB_WAVE_ROWS + r;              // wave-uniform
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
                    if (j < J) { bad |= calib_nonfinite(z[c]); mx = fmaxf(mx, z[c]); }
                }
                if (__any(bad)) { if (lane == 0) ++nonfinite; continue; }
                if (y < 0 || y >= J) { if (lane == 0) ++oob; continue; }
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
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
                    s0 = wave_sum_f64(s0); s1 = wave_sum_f64(s1); s2 = wave_sum_f64(s2);
                    double t_nll, t_g, t_h;
                    calib_nll_terms(s0, s1, s2, m, beta, zy, t_nll, t_g, t_h);
                    if (lane < 3) acc[w][k][lane] += lane == 0 ? t_nll : (lane == 1 ? t_g : t_h);
                }
            }
        }
    }
    nonfinite = wave_sum_i64(nonfinite); oob = wave_sum_i64(oob);
    __shared__ long icount[CALIB_WAVES][2];
    if (lane == 0) { icount[w][0] = nonfinite; icount[w][1] = oob; }
    __syncthreads();
    const int blocks = gridDim.x;
    for (int o = t; o < K * 3; o += CALIB_THREADS) {
        const int k = o / 3, c = o - 3 * k;
        double s = acc[0][k][c];
        for (int u = 1; u < CALIB_WAVES; ++u) s += acc[u][k][c];
        part[(long)o * blocks + blockIdx.x] = s;
    }
    if (t < 2) {
        long s = 0;
        for (int u = 0; u < CALIB_WAVES; ++u) s += icount[u][t];
        ipart[(long)t * blocks + blockIdx.x] = s;
    }
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
    const calib_plan_t p = calib_plan(n, J);
    double* part = (double*)ws;
    int64_t* ipart = (int64_t*)(part + (size_t)p.blocks * 3 * K);
    calib_betas_t bv;
    for (int k = 0; k < DFD_CALIB_MAX_BETAS; ++k) bv.v[k] = k < K ? betas[k] : 1.0;
    if (p.layout == DFD_CALIB_LAYOUT_THREAD)
        hipLaunchKernelGGL(k_calib_nll<DFD_CALIB_LAYOUT_THREAD>, dim3(p.blocks), dim3(CALIB_THREADS), 0, st, logits, targets, n, J, bv, K,
                           part, ipart);
    else
        hipLaunchKernelGGL(k_calib_nll<DFD_CALIB_LAYOUT_WAVE>, dim3(p.blocks), dim3(CALIB_THREADS), 0, st, logits, targets, n, J, bv, K,
                           part, ipart);
    hipLaunchKernelGGL(k_calib_sum, dim3(1), dim3(CALIB_THREADS), 0, st, (const double*)part, 3 * K, (const int64_t*)ipart, 2, p.blocks,
                       p.trips, out, stats);
    return DFD_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ softmax / arg max of beta * z
static __device__ __forceinline__ float calib_block_reduce(float v, float* sm, bool is_max) {       // dfd_misc.hip's block_reduce
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = is_max ? fmaxf(v, __shfl_xor(v, o)) : v + __shfl_xor(v, o);
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    float r = sm[0];
    for (int i = 1; i < DFD_THREADS / 64; ++i) r = is_max ? fmaxf(r, sm[i]) : r + sm[i];
    return r;
}

// k_softmax_argmax (dfd_misc.hip) statement for statement, with (z - max) * beta where that one has z - max: at beta == 1 the
// product is exact and the two kernels return the same bits
__global__ void __launch_bounds__(DFD_THREADS)
k_softmax_argmax_t(const float* __restrict__ logits, int J, float beta, float* __restrict__ probs, int64_t* __restrict__ preds) {
    __shared__ float sm[4];
    __shared__ int si[4];
    const int n = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const float* lr = logits + (long)n * J;
    float mx = -INFINITY;
    for (int j = t; j < J; j += DFD_THREADS) mx = fmaxf(mx, lr[j]);
    mx = calib_block_reduce(mx, sm, true);
    float se = 0.f;
    for (int j = t; j < J; j += DFD_THREADS) se += __expf((lr[j] - mx) * beta);
    se = calib_block_reduce(se, sm, false);
    const float inv = 1.f / se;
    float bp = -1.f; int bi = 0;
    for (int j = t; j < J; j += DFD_THREADS) {
        const float p = __expf((lr[j] - mx) * beta) * inv;
        if (probs) probs[(long)n * J + j] = p;
        if (p > bp) { bp = p; bi = j; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float op = __shfl_xor(bp, o);
        const int oi = __shfl_xor(bi, o);
        if (op > bp || (op == bp && oi < bi)) { bp = op; bi = oi; }
    }
    __syncthreads();
    if (lane == 0) { sm[wave] = bp; si[wave] = bi; }
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < 4; ++i)
            if (sm[i] > bp || (sm[i] == bp && si[i] < bi)) { bp = sm[i]; bi = si[i]; }
        preds[n] = bi;
    }
}

extern "C" int dfd_softmax_argmax_t(const float* logits, int N, int J, float inv_temperature, float* probs, int64_t* preds,
                                    dfd_stream stream) {
    if (!logits || !preds || N < 1 || J < 1) return DFD_EINVAL;
    if (!(inv_temperature > 0.f) || !__builtin_isfinite(inv_temperature)) return DFD_EINVAL;
    hipLaunchKernelGGL(k_softmax_argmax_t, dim3(N), dim3(DFD_THREADS), 0, (hipStream_t)stream, logits, J, inv_temperature, probs, preds);
    return DFD_CHECK_LAUNCH();
}
