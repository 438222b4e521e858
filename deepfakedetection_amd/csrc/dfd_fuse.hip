// dfd_fuse.hip — the ensemble of K models on the device (ABI 151): the fused scores of a logit pool (log-linear) or a probability
// pool (linear), the negative log-likelihood of the logit pool with its gradient and Hessian in the K coefficients for many
// coefficient vectors at once, and the right / wrong agreement tables of the members' predictions.
//
// Every member's logits are an f32 [n][J] buffer of its own; the K device addresses travel by value in the launch (fuse_ptrs_t).
// dfd_fuse_scores and dfd_fuse_nll use the row layouts and the launch shape of dfd_rowred.h; dfd_fuse_nll is the two-stage sum
// described there, with the order of every sum (equal inputs give equal bits):
//   dfd_fuse_scores      k_rowred_zero   stats[0] = 0
//                        k_fuse_scores   one row per thread or per wave: f64 throughout, one rounding to f32 on store
//   dfd_fuse_nll         k_fuse_nll      stage 1: the workgroup's f64 partials of {nll, g[K], H[K(K+1)/2]} per candidate and its two
//                                        int64 row counts into ws
//                        k_rowred_sum    stage 2
//   dfd_fuse_agree       k_rowred_zero   pair, hist and stats = 0
//                        k_fuse_agree    an LDS histogram of the 2^K right / wrong patterns per workgroup, from which the workgroup
//                                        adds its share of every table cell with dfd_count.h's count_add
// K J <= DFD_FUSE_THREAD_MAX_KJ takes the thread layout (in k_fuse_nll the K rows of a sample are read once into LDS and serve
// every candidate), wider inputs the wave layout, a lane reading its columns again per candidate; at most DFD_FUSE_MAX_BLOCKS
// workgroups.
#include "dfd_count.h"

#define FUSE_K DFD_FUSE_MAX_MODELS
#define FUSE_TRI (FUSE_K * (FUSE_K + 1) / 2)
static_assert(DFD_FUSE_MAX_TERMS == 1 + FUSE_K + FUSE_TRI, "nll, the gradient and the upper triangle of the Hessian");
static_assert((1 << FUSE_K) == ROWRED_THREADS, "k_fuse_agree keeps one pattern count per thread");

static rowred_plan_t fuse_plan(int n, int J, int K) { return rowred_plan(n, K * J <= DFD_FUSE_THREAD_MAX_KJ, DFD_FUSE_MAX_BLOCKS); }

static bool fuse_shape_ok(int n, int J, int K) {
    return n >= 0 && n <= DFD_FUSE_MAX_N && J >= 1 && J <= DFD_FUSE_MAX_J && K >= 1 && K <= DFD_FUSE_MAX_MODELS;
}

// by value in the launch: the callers' arrays are host memory
struct fuse_ptrs_t { const void* p[FUSE_K]; };
struct fuse_coef_t { double v[FUSE_K]; };
struct fuse_cands_t { double v[DFD_FUSE_MAX_CANDS][FUSE_K]; };

// ------------------------------------------------------------------ fused scores
// sum_k a_k z_k[off] in the order k = 0, 1, ...: the one form of the pooled logit in this file
static __device__ __forceinline__ double fuse_pool(const fuse_ptrs_t& zp, const double* a, int K, long off) {
    double f = 0.0;
#pragma unroll
    for (int k = 0; k < FUSE_K; ++k)
        if (k < K) f += a[k] * (double)((const float*)zp.p[k])[off];
    return f;
}

static __device__ __forceinline__ bool fuse_row_bad(const fuse_ptrs_t& zp, int K, long first, int J, int j0, int step) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < FUSE_K; ++k)
        if (k < K)
            for (int j = j0; j < J; j += step) bad |= f32_nonfinite(((const float*)zp.p[k])[first + j]);
    return bad;
}

// A row's columns j0, j0 + step, ... (the whole row of a thread: 0, 1; a lane's share of a wave's row: lane, 64) -> probs, logits_out
// and the lane's first arg max of the stored f32 probabilities.  WAVE: the maxima and sums run over the wave.
template <int MODE, bool WAVE>
static __device__ __forceinline__ void fuse_row(const fuse_ptrs_t& zp, const fuse_coef_t& coef, const fuse_coef_t& beta, int K, long first,
                                                int J, int j0, int step, float* __restrict__ probs, float* __restrict__ logits_out,
                                                float& best, int& arg) {
    best = -1.f; arg = 0x7fffffff;
    if (MODE == DFD_FUSE_LOGIT) {
        double m = -INFINITY, s = 0.0;
        for (int j = j0; j < J; j += step) m = fmax(m, fuse_pool(zp, coef.v, K, first + j));
        if (WAVE) m = wave_max(m);
        for (int j = j0; j < J; j += step) s += exp(fuse_pool(zp, coef.v, K, first + j) - m);
        if (WAVE) s = wave_sum(s);
        for (int j = j0; j < J; j += step) {
            const double f = fuse_pool(zp, coef.v, K, first + j);
            const float p = (float)(exp(f - m) / s);
            if (probs) probs[first + j] = p;
            if (logits_out) logits_out[first + j] = (float)f;
            if (p > best) { best = p; arg = j; }
        }
    } else {
        double mk[FUSE_K], sk[FUSE_K];
#pragma unroll
        for (int k = 0; k < FUSE_K; ++k) {
            mk[k] = -INFINITY; sk[k] = 0.0;
            if (k < K) {
                const float* __restrict__ z = (const float*)zp.p[k] + first;
                for (int j = j0; j < J; j += step) mk[k] = fmax(mk[k], beta.v[k] * (double)z[j]);
                if (WAVE) mk[k] = wave_max(mk[k]);
                for (int j = j0; j < J; j += step) sk[k] += exp(beta.v[k] * (double)z[j] - mk[k]);
                if (WAVE) sk[k] = wave_sum(sk[k]);
            }
        }
        for (int j = j0; j < J; j += step) {
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < FUSE_K; ++k)
                if (k < K) q += coef.v[k] * (exp(beta.v[k] * (double)((const float*)zp.p[k])[first + j] - mk[k]) / sk[k]);
            const float p = (float)q;
            if (probs) probs[first + j] = p;
            if (logits_out) logits_out[first + j] = (float)log(q);
            if (p > best) { best = p; arg = j; }
        }
    }
}

template <int LAYOUT, int MODE>
__global__ void __launch_bounds__(ROWRED_THREADS)
k_fuse_scores(const fuse_ptrs_t zp, int K, int n, int J, const fuse_coef_t coef, const fuse_coef_t beta, float* __restrict__ probs,
              float* __restrict__ logits_out, int64_t* __restrict__ preds, int64_t* __restrict__ stats) {
    __shared__ long red[ROWRED_WAVES];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    long nonfinite = 0;
    if (LAYOUT == DFD_FUSE_LAYOUT_THREAD) {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_THREAD; base < n; base += (long)gridDim.x * ROWRED_ROWS_THREAD) {
            const long i = base + t;
            if (i >= n) continue;
            const long first = i * J;
            if (fuse_row_bad(zp, K, first, J, 0, 1)) {
                for (int j = 0; j < J; ++j) {
                    if (probs) probs[first + j] = NAN;
                    if (logits_out) logits_out[first + j] = NAN;
                }
                preds[i] = 0;
                ++nonfinite;
                continue;
            }
            float best; int arg;
            fuse_row<MODE, false>(zp, coef, beta, K, first, J, 0, 1, probs, logits_out, best, arg);
            preds[i] = arg;
        }
    } else {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_WAVE; base < n; base += (long)gridDim.x * ROWRED_ROWS_WAVE) {
            for (int r = 0; r < ROWRED_WAVE_ROWS; ++r) {
                const long i = base + w * ROWRED_WAVE_ROWS + r;               // wave-uniform
                if (i >= n) break;
                const long first = i * J;
                if (__any(fuse_row_bad(zp, K, first, J, lane, 64))) {
                    for (int j = lane; j < J; j += 64) {
                        if (probs) probs[first + j] = NAN;
                        if (logits_out) logits_out[first + j] = NAN;
                    }
                    if (lane == 0) { preds[i] = 0; ++nonfinite; }
                    continue;
                }
                float best; int arg;
                fuse_row<MODE, true>(zp, coef, beta, K, first, J, lane, 64, probs, logits_out, best, arg);
                wave_first_argmax(best, arg);
                if (lane == 0) preds[i] = arg;
            }
        }
    }
    nonfinite = block_sum<ROWRED_WAVES>(nonfinite, red);
    if (t == 0) count_add(stats, nonfinite);
}

extern "C" int dfd_fuse_plan(int n, int J, int K, int* out) {
    if (!fuse_shape_ok(n, J, K) || !out) return DFD_EINVAL;
    const rowred_plan_t p = fuse_plan(n, J, K);
    out[0] = p.layout; out[1] = p.rows; out[2] = p.blocks; out[3] = p.trips;
    return DFD_OK;
}

static bool fuse_take_ptrs(const void* const* ptrs, int K, bool may_be_null, fuse_ptrs_t& zp) {
    for (int k = 0; k < FUSE_K; ++k) {
        zp.p[k] = k < K ? ptrs[k] : nullptr;
        if (k < K && !zp.p[k] && !may_be_null) return false;
    }
    return true;
}

#define FUSE_LAUNCH_SCORES(LAYOUT, MODE)                                                                                          \
    hipLaunchKernelGGL((k_fuse_scores<LAYOUT, MODE>), dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, zp, K, n, J, cv, bv, probs, logits_out, \
                       preds, stats)

extern "C" int dfd_fuse_scores(const float* const* ptrs, int K, int n, int J, int mode, const double* coef, const double* beta,
                               float* probs, float* logits_out, int64_t* preds, int64_t* stats, dfd_stream stream) {
    if (!fuse_shape_ok(n, J, K) || (mode != DFD_FUSE_LOGIT && mode != DFD_FUSE_PROB)) return DFD_EINVAL;
    if (!ptrs || !coef || !stats || (mode == DFD_FUSE_PROB && !beta) || (n > 0 && !preds)) return DFD_EINVAL;
    fuse_ptrs_t zp;
    if (!fuse_take_ptrs((const void* const*)ptrs, K, n == 0, zp)) return DFD_EINVAL;
    fuse_coef_t cv, bv;
    double total = 0.0;
    for (int k = 0; k < FUSE_K; ++k) {
        cv.v[k] = k < K ? coef[k] : 0.0;
        bv.v[k] = k < K && mode == DFD_FUSE_PROB ? beta[k] : 1.0;
        if (!__builtin_isfinite(cv.v[k]) || !__builtin_isfinite(bv.v[k])) return DFD_EINVAL;
        if (mode == DFD_FUSE_PROB && (cv.v[k] < 0.0 || !(bv.v[k] > 0.0))) return DFD_EINVAL;
        total += cv.v[k];
    }
    if (mode == DFD_FUSE_PROB && !(__builtin_fabs(total - 1.0) <= 1e-12)) return DFD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const rowred_plan_t p = fuse_plan(n, J, K);
    hipLaunchKernelGGL(k_rowred_zero<ROWRED_THREADS>, dim3(1), dim3(ROWRED_THREADS), 0, st, stats, 1, (int64_t*)nullptr, 0, (int64_t*)nullptr, 0);
    if (n > 0) {
        if (p.layout == DFD_FUSE_LAYOUT_THREAD) {
            if (mode == DFD_FUSE_LOGIT) FUSE_LAUNCH_SCORES(DFD_FUSE_LAYOUT_THREAD, DFD_FUSE_LOGIT);
            else FUSE_LAUNCH_SCORES(DFD_FUSE_LAYOUT_THREAD, DFD_FUSE_PROB);
        } else {
            if (mode == DFD_FUSE_LOGIT) FUSE_LAUNCH_SCORES(DFD_FUSE_LAYOUT_WAVE, DFD_FUSE_LOGIT);
            else FUSE_LAUNCH_SCORES(DFD_FUSE_LAYOUT_WAVE, DFD_FUSE_PROB);
        }
    }
    return DFD_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ NLL(a), its gradient and its Hessian in a
// With f_j = sum_k a_k z_kj, m = max_j f_j, e_j = exp(f_j - m): s = sum_j e_j, s1[k] = sum_j e_j z_kj, s2[k][l] = sum_j e_j z_kj z_kl
// (l >= k).  A row adds m + log s - f_y to nll, s1[k] / s - z_ky to g[k] and s2[k][l] / s - (s1[k] / s)(s1[l] / s) to H[k][l].
struct fuse_sums_t { double s, s1[FUSE_K], s2[FUSE_TRI]; };

static __host__ __device__ constexpr int fuse_tri(int k, int l) { return k * FUSE_K - k * (k - 1) / 2 + (l - k); }    // l >= k, K = 8

static __device__ __forceinline__ void fuse_sums_add(fuse_sums_t& u, const double* zk, double e, int K) {
    u.s += e;
#pragma unroll
    for (int k = 0; k < FUSE_K; ++k) {
        if (k < K) {
            u.s1[k] += e * zk[k];
#pragma unroll
            for (int l = k; l < FUSE_K; ++l)
                if (l < K) u.s2[fuse_tri(k, l)] += e * (zk[k] * zk[l]);
        }
    }
}

// Every lane holds a row's term (or 0): their sum over the wave joins the wave's running sum of candidate c, term o
static __device__ __forceinline__ void fuse_acc(double* __restrict__ acc, int o, double v, int lane) {
    v = wave_sum(v);
    if (lane == 0) acc[o] += v;
}

// The terms of one row (`live`: the lane holds one; u: the row's sums) into acc[DFD_FUSE_MAX_TERMS] in the packed order
// {nll, g[0..K), H[0][0..K), H[1][1..K), ...}.  ONE_ROW: every lane holds the same row, which counts once.
template <bool ONE_ROW>
static __device__ __forceinline__ void fuse_terms(double* __restrict__ acc, const fuse_sums_t& u, double m, double fy, const double* zy,
                                                  int K, bool live, int lane) {
    const double t_nll = live ? m + log(u.s) - fy : 0.0;
    if (ONE_ROW) { if (lane == 0) acc[0] += t_nll; } else fuse_acc(acc, 0, t_nll, lane);
    int o = 1 + K;
#pragma unroll
    for (int k = 0; k < FUSE_K; ++k) {
        if (k < K) {
            const double mk = u.s1[k] / u.s;
            const double t_g = live ? mk - zy[k] : 0.0;
            if (ONE_ROW) { if (lane == 0) acc[1 + k] += t_g; } else fuse_acc(acc, 1 + k, t_g, lane);
#pragma unroll
            for (int l = k; l < FUSE_K; ++l) {
                if (l < K) {
                    const double t_h = live ? u.s2[fuse_tri(k, l)] / u.s - mk * (u.s1[l] / u.s) : 0.0;
                    if (ONE_ROW) { if (lane == 0) acc[o] += t_h; } else fuse_acc(acc, o, t_h, lane);
                    ++o;
                }
            }
        }
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(ROWRED_THREADS)
k_fuse_nll(const fuse_ptrs_t zp, const int64_t* __restrict__ targets, int n, int J, int K, const fuse_cands_t cands, int C, int terms,
           double* __restrict__ part, int64_t* __restrict__ ipart) {
    __shared__ double acc[ROWRED_WAVES][DFD_FUSE_MAX_CANDS][DFD_FUSE_MAX_TERMS];
    __shared__ double sa[DFD_FUSE_MAX_CANDS][FUSE_K];
    __shared__ float zs[LAYOUT == DFD_FUSE_LAYOUT_THREAD ? DFD_FUSE_THREAD_MAX_KJ : 1][ROWRED_THREADS];      // [k J + j][thread]
    __shared__ long icount[ROWRED_WAVES][2];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < ROWRED_WAVES * DFD_FUSE_MAX_CANDS * DFD_FUSE_MAX_TERMS; i += ROWRED_THREADS) (&acc[0][0][0])[i] = 0.0;
    if (t < DFD_FUSE_MAX_CANDS * FUSE_K) (&sa[0][0])[t] = cands.v[t / FUSE_K][t % FUSE_K];
    __syncthreads();
    long nonfinite = 0, oob = 0;
    if (LAYOUT == DFD_FUSE_LAYOUT_THREAD) {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_THREAD; base < n; base += (long)gridDim.x * ROWRED_ROWS_THREAD) {
            const long i = base + t;                                        // the trip count is wave-uniform: base < n for the wave
            bool ok = i < n;
            int y = 0;
            if (ok) {
                bool bad = false;
#pragma unroll
                for (int k = 0; k < FUSE_K; ++k) {
                    if (k < K) {
                        const float* __restrict__ row = (const float*)zp.p[k] + i * J;
                        for (int j = 0; j < J; ++j) {
                            const float v = row[j];
                            bad |= f32_nonfinite(v);
                            zs[k * J + j][t] = v;                           // k J + j < K J <= DFD_FUSE_THREAD_MAX_KJ; read by this thread only
                        }
                    }
                }
                const int64_t yy = targets[i];
                if (bad) { ++nonfinite; ok = false; }
                else if (yy < 0 || yy >= J) { ++oob; ok = false; }
                else y = (int)yy;
            }
            if (!__any(ok)) continue;
            for (int c = 0; c < C; ++c) {
                fuse_sums_t u;
                u.s = 0.0;
#pragma unroll
                for (int k = 0; k < FUSE_K; ++k) u.s1[k] = 0.0;
#pragma unroll
                for (int q = 0; q < FUSE_TRI; ++q) u.s2[q] = 0.0;
                double zy[FUSE_K], m = -INFINITY, fy = 0.0;
#pragma unroll
                for (int k = 0; k < FUSE_K; ++k) zy[k] = 0.0;
                if (ok) {
                    for (int j = 0; j < J; ++j) {
                        double f = 0.0;
#pragma unroll
                        for (int k = 0; k < FUSE_K; ++k)
                            if (k < K) f += sa[c][k] * (double)zs[k * J + j][t];
                        m = fmax(m, f);
                        if (j == y) fy = f;
                    }
                    for (int j = 0; j < J; ++j) {
                        double zk[FUSE_K], f = 0.0;
#pragma unroll
                        for (int k = 0; k < FUSE_K; ++k) {
                            zk[k] = k < K ? (double)zs[k * J + j][t] : 0.0;
                            if (k < K) f += sa[c][k] * zk[k];
                        }
                        fuse_sums_add(u, zk, exp(f - m), K);
                    }
#pragma unroll
                    for (int k = 0; k < FUSE_K; ++k)
                        if (k < K) zy[k] = (double)zs[k * J + y][t];
                } else {
                    u.s = 1.0; m = 0.0;                                     // a lane without a row adds zeros
                }
                fuse_terms<false>(acc[w][c], u, m, fy, zy, K, ok, lane);
            }
        }
    } else {
        for (long base = (long)blockIdx.x * ROWRED_ROWS_WAVE; base < n; base += (long)gridDim.x * ROWRED_ROWS_WAVE) {
            for (int r = 0; r < ROWRED_WAVE_ROWS; ++r) {
                const long i = base + w * ROWRED_WAVE_ROWS + r;               // wave-uniform
                if (i >= n) break;
                const long first = i * J;
                const int64_t y = targets[i];
                if (__any(fuse_row_bad(zp, K, first, J, lane, 64))) { if (lane == 0) ++nonfinite; continue; }
                if (y < 0 || y >= J) { if (lane == 0) ++oob; continue; }
                double zy[FUSE_K];
#pragma unroll
                for (int k = 0; k < FUSE_K; ++k) zy[k] = k < K ? (double)((const float*)zp.p[k])[first + y] : 0.0;
                for (int c = 0; c < C; ++c) {
                    double m = -INFINITY, fy = 0.0;
                    for (int j = lane; j < J; j += 64) m = fmax(m, fuse_pool(zp, sa[c], K, first + j));
                    m = wave_max(m);
#pragma unroll
                    for (int k = 0; k < FUSE_K; ++k)
                        if (k < K) fy += sa[c][k] * zy[k];                  // fuse_pool's arithmetic at column y
                    fuse_sums_t u;
                    u.s = 0.0;
#pragma unroll
                    for (int k = 0; k < FUSE_K; ++k) u.s1[k] = 0.0;
#pragma unroll
                    for (int q = 0; q < FUSE_TRI; ++q) u.s2[q] = 0.0;
                    for (int j = lane; j < J; j += 64) {
                        double zk[FUSE_K], f = 0.0;
#pragma unroll
                        for (int k = 0; k < FUSE_K; ++k) {
                            zk[k] = k < K ? (double)((const float*)zp.p[k])[first + j] : 0.0;
                            if (k < K) f += sa[c][k] * zk[k];
                        }
                        fuse_sums_add(u, zk, exp(f - m), K);
                    }
                    u.s = wave_sum(u.s);
#pragma unroll
                    for (int k = 0; k < FUSE_K; ++k) {
                        if (k < K) {
                            u.s1[k] = wave_sum(u.s1[k]);
#pragma unroll
                            for (int l = k; l < FUSE_K; ++l)
                                if (l < K) u.s2[fuse_tri(k, l)] = wave_sum(u.s2[fuse_tri(k, l)]);
                        }
                    }
                    fuse_terms<true>(acc[w][c], u, m, fy, zy, K, true, lane);
                }
            }
        }
    }
    rowred_stage1_store(acc, icount, C * terms, terms, nonfinite, oob, part, ipart);
}

static int fuse_terms_of(int K) { return 1 + K + K * (K + 1) / 2; }

extern "C" size_t dfd_fuse_nll_ws(int n, int J, int K, int C) {
    if (!fuse_shape_ok(n, J, K) || C < 1 || C > DFD_FUSE_MAX_CANDS) return 0;
    return (size_t)fuse_plan(n, J, K).blocks * (size_t)(C * fuse_terms_of(K) + 2) * 8;
}

extern "C" int dfd_fuse_nll(const float* const* ptrs, int K, const int64_t* targets, int n, int J, const double* cands, int C, void* ws,
                            size_t ws_bytes, double* out, int64_t* stats, dfd_stream stream) {
    if (!fuse_shape_ok(n, J, K) || C < 1 || C > DFD_FUSE_MAX_CANDS) return DFD_EINVAL;
    if (!ptrs || !cands || !ws || !out || !stats || (n > 0 && !targets)) return DFD_EINVAL;
    fuse_ptrs_t zp;
    if (!fuse_take_ptrs((const void* const*)ptrs, K, n == 0, zp)) return DFD_EINVAL;
    fuse_cands_t cv;
    for (int c = 0; c < DFD_FUSE_MAX_CANDS; ++c)
        for (int k = 0; k < FUSE_K; ++k) {
            cv.v[c][k] = c < C && k < K ? cands[c * K + k] : 0.0;
            if (!__builtin_isfinite(cv.v[c][k])) return DFD_EINVAL;
        }
    if (ws_bytes < dfd_fuse_nll_ws(n, J, K, C)) return DFD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const rowred_plan_t p = fuse_plan(n, J, K);
    const int terms = fuse_terms_of(K);
    double* part = (double*)ws;
    int64_t* ipart = (int64_t*)(part + (size_t)p.blocks * C * terms);
    if (p.layout == DFD_FUSE_LAYOUT_THREAD)
        hipLaunchKernelGGL(k_fuse_nll<DFD_FUSE_LAYOUT_THREAD>, dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, zp, targets, n, J, K, cv, C, terms,
                           part, ipart);
    else
        hipLaunchKernelGGL(k_fuse_nll<DFD_FUSE_LAYOUT_WAVE>, dim3(p.blocks), dim3(ROWRED_THREADS), 0, st, zp, targets, n, J, K, cv, C, terms,
                           part, ipart);
    hipLaunchKernelGGL(k_rowred_sum<ROWRED_THREADS>, dim3(1), dim3(ROWRED_THREADS), 0, st, (const double*)part, C * terms, (const int64_t*)ipart,
                       2, p.blocks, p.trips, out, stats);
    return DFD_CHECK_LAUNCH();
}

// ------------------------------------------------------------------ agreement of the members' predictions
// Bit k of a row's pattern: member k predicted the target.  cnt[pattern] per workgroup in LDS; then cell (a, b, q) of pair is the
// sum of cnt over the patterns whose bits a and b read q = {11, 10, 01, 00}[q], and hist[c] the sum over those with c bits set.
__global__ void __launch_bounds__(ROWRED_THREADS)
k_fuse_agree(const fuse_ptrs_t pp, const int64_t* __restrict__ targets, int n, int J, int K, int64_t* __restrict__ pair,
             int64_t* __restrict__ hist, int64_t* __restrict__ stats) {
    __shared__ unsigned int cnt[1 << FUSE_K];
    __shared__ long red[ROWRED_WAVES];
    const int t = threadIdx.x;
    cnt[t] = 0;
    __syncthreads();
    long oob = 0;
    for (long i = (long)blockIdx.x * ROWRED_THREADS + t; i < n; i += (long)gridDim.x * ROWRED_THREADS) {
        const int64_t y = targets[i];
        if (y < 0 || y >= J) { ++oob; continue; }
        unsigned int pattern = 0;
#pragma unroll
        for (int k = 0; k < FUSE_K; ++k)
            if (k < K) pattern |= (unsigned int)(((const int64_t*)pp.p[k])[i] == y) << k;
        atomicAdd(&cnt[pattern], 1u);                                       // fewer than 2^32 rows in all (DFD_FUSE_MAX_N)
    }
    oob = block_sum<ROWRED_WAVES>(oob, red);                                // its barriers also publish cnt[]
    const int patterns = 1 << K;
    for (int o = t; o < K * K * 4; o += ROWRED_THREADS) {
        const int q = o & 3, b = (o >> 2) % K, a = (o >> 2) / K;
        const unsigned int want_a = q < 2, want_b = (q & 1) == 0;
        long s = 0;
        for (int m = 0; m < patterns; ++m)
            if (((m >> a) & 1u) == want_a && ((m >> b) & 1u) == want_b) s += cnt[m];
        count_add(pair + o, s);
    }
    if (t <= K) {
        long s = 0;
        for (int m = 0; m < patterns; ++m)
            if (__popc(m) == t) s += cnt[m];
        count_add(hist + t, s);
    }
    if (t == ROWRED_THREADS - 1) {
        long valid = 0;
        for (int m = 0; m < patterns; ++m) valid += cnt[m];
        count_add(stats + 0, valid); count_add(stats + 1, oob);
    }
}

extern "C" int dfd_fuse_agree(const int64_t* const* pred_ptrs, int K, const int64_t* targets, int n, int J, int64_t* pair, int64_t* hist,
                              int64_t* stats, dfd_stream stream) {
    if (!fuse_shape_ok(n, J, K)) return DFD_EINVAL;
    if (!pred_ptrs || !pair || !hist || !stats || (n > 0 && !targets)) return DFD_EINVAL;
    fuse_ptrs_t pp;
    if (!fuse_take_ptrs((const void* const*)pred_ptrs, K, n == 0, pp)) return DFD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long chunks = ((long)n + ROWRED_THREADS - 1) / ROWRED_THREADS;
    const int blocks = (int)(chunks > DFD_FUSE_MAX_BLOCKS ? DFD_FUSE_MAX_BLOCKS : chunks);
    hipLaunchKernelGGL(k_rowred_zero<ROWRED_THREADS>, dim3(1), dim3(ROWRED_THREADS), 0, st, pair, K * K * 4, hist, K + 1, stats, 2);
    if (blocks > 0)
        hipLaunchKernelGGL(k_fuse_agree, dim3(blocks), dim3(ROWRED_THREADS), 0, st, pp, targets, n, J, K, pair, hist, stats);
    return DFD_CHECK_LAUNCH();
}
