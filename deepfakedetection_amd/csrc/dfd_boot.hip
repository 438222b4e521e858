// dfd_boot.hip — bootstrap resamples of the ROC statistics on the device (ABI 153, the cluster bootstrap ABI 154; the contract is in
// include/dfd_hip.h).
//
// A resample is a vector of multiplicities c[i] over the samples in the caller's order; the scores stay sorted as they are, so no
// resample sorts.  Everything is integer counting: the draws add 1 to uint32 counts, the sweep adds the counts up, and the only
// atomics are integer adds, so every output is independent of arrival order and launch geometry.
//   LDS tier      k_boot_lds     one workgroup per resample: zero the counts in LDS, draw, class totals, sweep every member
//   global tier   k_count_zero   counts uint32 [R][n] in the workspace
//                 k_boot_draw    one workgroup per (resample, tile of DFD_BOOT_DRAW_TILE draws): global adds without return
//                 k_boot_glb     one workgroup per (resample, member): class totals, sweep
// The sweep walks the sorted order in tiles of BOOT_THREADS x BOOT_PER positions, a thread owning BOOT_PER consecutive ones.  Per tile
// it needs two of dfd_count.h's block scans: the sum of the weighted positives / negatives before the thread, and the cumulative
// pair at the last tie-group end before the thread.  Both cumulatives never decrease along the order, so "the last one" is a
// maximum.  With the pair at a group's two ends the thread adds the group's term of two_u and tests whether the equal-error segment
// ends there.  P and N do not depend on the member (the labels are shared), so a pass over the counts in sample order supplies them
// before the sweep, and the sweep is one pass.  The tie-group ends (dfd_count.h's rule, dfd_roc_curve's too) compare neighbouring
// scores the sweep has loaded anyway.
// The cluster bootstrap (dfd_boot_stats_grouped) draws G groups instead of n samples: the counts have G entries, and the totals and
// the sweep read a sample's weight as counts[group[i]] (BootGrouped) where the plain bootstrap reads counts[i] (BootDirect).  The
// kernels are templates on that weight and differ in nothing else; zero and draw run over G unchanged.
#include "dfd_count.h"
#include "dfd_philox.h"

#define BOOT_THREADS 1024
#define BOOT_NW (BOOT_THREADS / 64)
#define BOOT_PER 8
#define BOOT_TILE (BOOT_THREADS * BOOT_PER)
#define BOOT_DRAW_THREADS 256
#define BOOT_DRAW_PER (DFD_BOOT_DRAW_TILE / 4 / BOOT_DRAW_THREADS)      // Philox blocks (of four draws) per thread
static_assert(BOOT_DRAW_PER * 4 * BOOT_DRAW_THREADS == DFD_BOOT_DRAW_TILE, "whole Philox blocks per thread");

#define BOOT_F_POS 1u
#define BOOT_F_END 2u
#define BOOT_F_CUT 4u

struct BootMembers {
    const float* score[DFD_BOOT_MAX_MEMBERS];
    const int* perm[DFD_BOOT_MAX_MEMBERS];
    double cut[DFD_BOOT_MAX_MEMBERS];
};

struct BootScratch {
    int scan[BOOT_NW * 2];
    unsigned long long red[BOOT_NW * 2];
    int eer[4];                                                         // f0, t0, f1, t1: written by the one thread that finds the segment
};
static_assert(sizeof(BootScratch) <= DFD_BOOT_SCRATCH_BYTES, "the scratch in front of the LDS counts");
static_assert(DFD_BOOT_SCRATCH_BYTES + 4 * DFD_BOOT_LDS_MAX_N <= 160 * 1024, "one workgroup's LDS");
static_assert(DFD_BOOT_MAX_N <= (1 << 24), "weighted totals stay below 2^25: int32 scans, two_u below 2^50");

// draws 4 q .. 4 q + 3 of resample b: counts[idx] += 1 each (LDS or global, by the address space of `counts`)
static __device__ __forceinline__ void boot_draw4(uint32_t* counts, int n, uint32_t q, uint32_t b, uint32_t k0, uint32_t k1) {
    uint32_t c[4] = {q, b, 0u, DFD_BOOT_STREAM};
    philox4x32_10(c, k0, k1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((long)q * 4 + j < n) {
            const uint32_t idx = (uint32_t)(((uint64_t)c[j] * (uint64_t)(uint32_t)n) >> 32);           // < n
            atomicAdd(counts + idx, 1u);
        }
    }
}

// how often sample i counts in a resample: its own count, or the count of its group (an id outside [0, G) counts for nothing)
struct BootDirect {
    const uint32_t* c;
    __device__ __forceinline__ uint32_t operator()(int i) const { return c[i]; }
};
struct BootGrouped {
    const uint32_t* c;
    const int* __restrict__ group;
    int G;
    __device__ __forceinline__ uint32_t operator()(int i) const {
        const int g = group[i];
        return (unsigned)g < (unsigned)G ? c[g] : 0u;
    }
};

// P, N and hits of the resample in which sample i counts c(i) times, in sample order
template <typename W>
static __device__ __forceinline__ void boot_totals(const W c, const unsigned char* __restrict__ is_positive,
                                                   const unsigned char* __restrict__ hit, int n, BootScratch* sc, int& P, int& N, int& hits) {
    unsigned long long v[2] = {0, 0};                                   // P | N << 32, hits
    for (int i = threadIdx.x; i < n; i += BOOT_THREADS) {
        const unsigned long long w = c(i);
        v[0] += is_positive[i] ? w : (w << 32);
        if (hit && hit[i]) v[1] += w;
    }
    block_sum<2, BOOT_NW>(v, sc->red);
    P = (int)(v[0] & 0xffffffffull);
    N = (int)(v[0] >> 32);
    hits = (int)v[1];
}

// one member's statistics of the resample in which sample i counts c(i) times: out[DFD_BOOT_STATS_LEN]
template <typename W>
static __device__ __forceinline__ void boot_sweep(const W c, const float* __restrict__ score, const int* __restrict__ perm,
                                                  const unsigned char* __restrict__ is_positive, double cut, int n, int P, int N, int hits,
                                                  BootScratch* sc, int64_t* __restrict__ out) {
    const int t = threadIdx.x;
    if (t < 4) sc->eer[t] = 0;
    __syncthreads();
    const long long PN = (long long)P * N;
    int carry_p = 0, carry_n = 0, carry_ep = 0, carry_en = 0;           // cumulative pair at the tile's start / at the last group end before it
    unsigned long long two_u = 0;
    int tp = 0, fp = 0;
    for (int base = 0; base < n; base += BOOT_TILE) {                   // uniform trip count: the barriers inside are safe
        const int first = base + t * BOOT_PER;
        int w[BOOT_PER];
        unsigned f[BOOT_PER];
        int sp = 0, sn = 0, ep = 0, en = 0;
        bool has_end = false;
        float s = first < n ? score[first] : 0.f;
#pragma unroll
        for (int j = 0; j < BOOT_PER; ++j) {
            const int i = first + j;
            w[j] = 0;
            f[j] = 0;
            if (i < n) {
                const float s_next = i + 1 < n ? score[i + 1] : 0.f;
                const int idx = perm[i];
                const bool ok = (unsigned)idx < (unsigned)n;
                const int wt = ok ? (int)c(idx) : 0;
                unsigned fl = ok && is_positive[idx] ? BOOT_F_POS : 0u;
                if (tie_group_ends(s, s_next, i == n - 1)) fl |= BOOT_F_END;
                if ((double)s >= cut) fl |= BOOT_F_CUT;                 // false for a NaN cut
                if (fl & BOOT_F_POS) sp += wt; else sn += wt;
                if (fl & BOOT_F_END) { ep = sp; en = sn; has_end = true; }
                w[j] = wt;
                f[j] = fl;
                s = s_next;
            }
        }
        int v[2] = {sp, sn}, total[2];
        block_scan_excl<2, BOOT_NW, false>(v, total, sc->scan);
        int p = carry_p + v[0], nn = carry_n + v[1];
        int e[2] = {has_end ? p + ep : 0, has_end ? nn + en : 0}, etotal[2];
        block_scan_excl<2, BOOT_NW, true>(e, etotal, sc->scan);
        int bp = max(carry_ep, e[0]), bn = max(carry_en, e[1]);         // the pair at the group end before this thread, or (0, 0)
#pragma unroll
        for (int j = 0; j < BOOT_PER; ++j) {
            const unsigned fl = f[j];
            if (fl & BOOT_F_POS) p += w[j]; else nn += w[j];
            if (fl & BOOT_F_CUT) { if (fl & BOOT_F_POS) tp += w[j]; else fp += w[j]; }
            if (fl & BOOT_F_END) {                                      // only set for a position below n
                two_u += (unsigned long long)(p - bp) * (unsigned long long)(bn + nn);
                // with thresholds descending the curve passes (N - nn, P - p) and then (N - bn, P - bp); fps P + tps N - P N >= 0 there
                // reads bn P + bp N <= P N, which holds from some group end downwards: the segment is where it starts to hold
                const long long below = (long long)bn * P + (long long)bp * N, above = (long long)nn * P + (long long)p * N;
                if (below <= PN && above > PN) {
                    sc->eer[0] = N - nn; sc->eer[1] = P - p; sc->eer[2] = N - bn; sc->eer[3] = P - bp;
                }
                bp = p;
                bn = nn;
            }
        }
        carry_p += total[0];
        carry_n += total[1];
        carry_ep = max(carry_ep, etotal[0]);
        carry_en = max(carry_en, etotal[1]);
    }
    unsigned long long r[2] = {two_u, (unsigned long long)tp | ((unsigned long long)fp << 32)};
    block_sum<2, BOOT_NW>(r, sc->red);                                  // its barriers also publish eer[]
    if (t == 0) {
        out[0] = P; out[1] = N; out[2] = (int64_t)r[0];
        out[3] = (int64_t)(r[1] & 0xffffffffull); out[4] = (int64_t)(r[1] >> 32); out[5] = hits;
        out[6] = sc->eer[0]; out[7] = sc->eer[1]; out[8] = sc->eer[2]; out[9] = sc->eer[3];
    }
    __syncthreads();                                                    // eer[] is reset by the next member's sweep
}


// a kernel's weight over the counts c of its resample: BootDirect reads neither group nor G
template <typename W>
static __device__ __forceinline__ W boot_weight(const uint32_t* c, const int* group, int G) {
    if constexpr (std::is_same<W, BootDirect>::value) return {c};
    else return {c, group, G};
}

// nc: the counts of a resample, n with W = BootDirect and the G group counts with W = BootGrouped
template <typename W>
__global__ void __launch_bounds__(BOOT_THREADS)
k_boot_lds(BootMembers mem, int M, const unsigned char* __restrict__ is_positive, const unsigned char* __restrict__ hit,
           const int* __restrict__ group, int n, int nc, int B, uint32_t k0, uint32_t k1, int64_t* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) uint32_t boot_lds[];
    BootScratch* sc = reinterpret_cast<BootScratch*>(boot_lds);
    uint32_t* c = boot_lds + DFD_BOOT_SCRATCH_BYTES / 4;
    const int t = threadIdx.x, b = blockIdx.x;
    for (int i = t; i < nc; i += BOOT_THREADS) c[i] = 0;
    __syncthreads();
    const int nq = (nc + 3) / 4;
    for (int q = t; q < nq; q += BOOT_THREADS) boot_draw4(c, nc, (uint32_t)q, (uint32_t)b, k0, k1);
    __syncthreads();
    int P, N, hits;
    const W w = boot_weight<W>(c, group, nc);
    boot_totals(w, is_positive, hit, n, sc, P, N, hits);
    for (int m = 0; m < M; ++m)
        boot_sweep(w, mem.score[m], mem.perm[m], is_positive, mem.cut[m], n, P, N, hits, sc,
                   stats + ((size_t)m * B + b) * DFD_BOOT_STATS_LEN);
}

// grid (R, tiles): resample b0 + blockIdx.x, draws blockIdx.y * DFD_BOOT_DRAW_TILE ...
__global__ void __launch_bounds__(BOOT_DRAW_THREADS)
k_boot_draw(uint32_t* __restrict__ counts, int n, int b0, uint32_t k0, uint32_t k1) {
    uint32_t* c = counts + (size_t)blockIdx.x * n;
    const int nq = (n + 3) / 4;
#pragma unroll
    for (int k = 0; k < BOOT_DRAW_PER; ++k) {
        const int q = ((int)blockIdx.y * BOOT_DRAW_PER + k) * BOOT_DRAW_THREADS + threadIdx.x;
        if (q < nq) boot_draw4(c, n, (uint32_t)q, (uint32_t)(b0 + blockIdx.x), k0, k1);
    }
}

// grid (R, M): resample b0 + blockIdx.x of member blockIdx.y, over counts uint32 [R][nc]
template <typename W>
__global__ void __launch_bounds__(BOOT_THREADS)
k_boot_glb(BootMembers mem, const uint32_t* __restrict__ counts, const unsigned char* __restrict__ is_positive,
           const unsigned char* __restrict__ hit, const int* __restrict__ group, int n, int nc, int B, int b0,
           int64_t* __restrict__ stats) {
    __shared__ BootScratch sc;
    const int m = blockIdx.y, b = b0 + blockIdx.x;
    int P, N, hits;
    const W w = boot_weight<W>(counts + (size_t)blockIdx.x * nc, group, nc);
    boot_totals(w, is_positive, hit, n, &sc, P, N, hits);
    boot_sweep(w, mem.score[m], mem.perm[m], is_positive, mem.cut[m], n, P, N, hits, &sc, stats + ((size_t)m * B + b) * DFD_BOOT_STATS_LEN);
}

static bool boot_shape_ok(int n, int B) { return n >= 0 && n <= DFD_BOOT_MAX_N && B >= 1 && B <= DFD_BOOT_MAX_REPLICATES; }

extern "C" size_t dfd_boot_ws(int n, int B) {
    if (!boot_shape_ok(n, B) || n <= DFD_BOOT_LDS_MAX_N) return 0;
    return (size_t)B * (size_t)n * sizeof(uint32_t);
}

extern "C" int dfd_boot_plan(int n, int B, int M, size_t ws_bytes, int* plan) {
    if (!boot_shape_ok(n, B) || M < 1 || M > DFD_BOOT_MAX_MEMBERS || !plan) return DFD_EINVAL;
    const int tiles = (n + DFD_BOOT_DRAW_TILE - 1) / DFD_BOOT_DRAW_TILE;
    if (n <= DFD_BOOT_LDS_MAX_N) {
        plan[0] = DFD_BOOT_TIER_LDS; plan[1] = B; plan[2] = 1; plan[3] = tiles;
        return DFD_OK;
    }
    const size_t fit = ws_bytes / ((size_t)n * sizeof(uint32_t));
    if (fit < 1) return DFD_EINVAL;
    const int R = fit < (size_t)B ? (int)fit : B;
    plan[0] = DFD_BOOT_TIER_GLOBAL; plan[1] = R; plan[2] = (B + R - 1) / R; plan[3] = tiles;
    return DFD_OK;
}

static void boot_launch_counts(int n, int b0, int R, uint64_t seed, uint32_t* counts, hipStream_t st) {
    count_zero<256>(counts, (size_t)R * (size_t)n, nullptr, 0, st);
    const int tiles = (n + DFD_BOOT_DRAW_TILE - 1) / DFD_BOOT_DRAW_TILE;                               // at most 4096
    hipLaunchKernelGGL(k_boot_draw, dim3(R, tiles), dim3(BOOT_DRAW_THREADS), 0, st, counts, n, b0, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

extern "C" int dfd_boot_counts(int n, int b0, int R, uint64_t seed, uint32_t* counts, dfd_stream stream) {
    if (n < 0 || n > DFD_BOOT_MAX_N || b0 < 0 || R < 1 || R > DFD_BOOT_MAX_REPLICATES || b0 > DFD_BOOT_MAX_REPLICATES - R) return DFD_EINVAL;
    if (n == 0) return DFD_OK;
    if (!counts) return DFD_EINVAL;
    boot_launch_counts(n, b0, R, seed, counts, (hipStream_t)stream);
    return DFD_CHECK_LAUNCH();
}

// The launches of `plan` over resamples of nc counts (n with W = BootDirect, G with BootGrouped), after the caller's own checks
template <typename W>
static int boot_run(const int* plan, const float* const* score_ptrs, const int* const* perm_ptrs, int M, const unsigned char* is_positive,
                    const unsigned char* hit, const double* cuts, const int* group, int n, int nc, int B, uint64_t seed, void* ws,
                    int64_t* stats, hipStream_t st) {
    BootMembers mem = {};
    for (int m = 0; m < M; ++m) {
        if (n > 0 && (!score_ptrs[m] || !perm_ptrs[m])) return DFD_EINVAL;
        mem.score[m] = n > 0 ? score_ptrs[m] : nullptr;
        mem.perm[m] = n > 0 ? perm_ptrs[m] : nullptr;
        mem.cut[m] = cuts ? cuts[m] : __builtin_nan("");
    }
    if (plan[0] == DFD_BOOT_TIER_LDS) {
        dfd_allow_lds_once<k_boot_lds<W>>(160 * 1024);
        hipLaunchKernelGGL(k_boot_lds<W>, dim3(B), dim3(BOOT_THREADS), DFD_BOOT_SCRATCH_BYTES + (size_t)nc * sizeof(uint32_t), st, mem, M,
                           is_positive, hit, group, n, nc, B, (uint32_t)seed, (uint32_t)(seed >> 32), stats);
        return DFD_CHECK_LAUNCH();
    }
    if (!ws) return DFD_EINVAL;
    const int R = plan[1];
    for (int b0 = 0; b0 < B; b0 += R) {
        const int r = B - b0 < R ? B - b0 : R;
        boot_launch_counts(nc, b0, r, seed, (uint32_t*)ws, st);
        hipLaunchKernelGGL(k_boot_glb<W>, dim3(r, M), dim3(BOOT_THREADS), 0, st, mem, (const uint32_t*)ws, is_positive, hit, group, n, nc, B,
                           b0, stats);
    }
    return DFD_CHECK_LAUNCH();
}

extern "C" int dfd_boot_stats(const float* const* score_ptrs, const int* const* perm_ptrs, int M, const unsigned char* is_positive,
                              const unsigned char* hit, const double* cuts, int n, int B, uint64_t seed, void* ws, size_t ws_bytes,
                              int64_t* stats, dfd_stream stream) {
    int plan[4];
    if (dfd_boot_plan(n, B, M, ws_bytes, plan) != DFD_OK || !stats) return DFD_EINVAL;
    if (n > 0 && (!score_ptrs || !perm_ptrs || !is_positive)) return DFD_EINVAL;
    return boot_run<BootDirect>(plan, score_ptrs, perm_ptrs, M, is_positive, hit, cuts, nullptr, n, n, B, seed, ws, stats, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------- cluster bootstrap
static bool boot_grouped_ok(int n, int G, int max_size, int B) {
    return boot_shape_ok(n, B) && G >= 1 && G <= n && max_size >= 1 && max_size <= n &&
           (uint64_t)G * (uint64_t)max_size <= DFD_BOOT_GROUPED_MAX_WEIGHT;
}

extern "C" size_t dfd_boot_ws_grouped(int n, int G, int B) {
    if (!boot_shape_ok(n, B) || G < 1 || G > n || G <= DFD_BOOT_LDS_MAX_N) return 0;
    return (size_t)B * (size_t)G * sizeof(uint32_t);
}

extern "C" int dfd_boot_plan_grouped(int n, int G, int max_size, int B, int M, size_t ws_bytes, int* plan) {
    if (!boot_grouped_ok(n, G, max_size, B)) return DFD_EINVAL;
    return dfd_boot_plan(G, B, M, ws_bytes, plan);                      // the tiers, passes and draw tiles of G counts
}

extern "C" int dfd_boot_stats_grouped(const float* const* score_ptrs, const int* const* perm_ptrs, int M, const unsigned char* is_positive,
                                      const unsigned char* hit, const double* cuts, const int* group, int n, int G, int max_size, int B,
                                      uint64_t seed, void* ws, size_t ws_bytes, int64_t* stats, dfd_stream stream) {
    int plan[4];
    if (dfd_boot_plan_grouped(n, G, max_size, B, M, ws_bytes, plan) != DFD_OK || !stats) return DFD_EINVAL;
    if (!score_ptrs || !perm_ptrs || !is_positive || !group) return DFD_EINVAL;
    return boot_run<BootGrouped>(plan, score_ptrs, perm_ptrs, M, is_positive, hit, cuts, group, n, G, B, seed, ws, stats, (hipStream_t)stream);
}
