// dfd_count.h — the integer-counting toolkit of the evaluation kernels (dfd_metrics.hip, dfd_boot.hip, dfd_group.hip and the counter
// tails of dfd_calib.hip and dfd_fuse.hip): the exclusive block scan, the workgroup sum of 64-bit words, the counter flush, the
// tie-group rule of sorted scores and the zeroing kernel.  The wave reductions and f32_nonfinite come from dfd_rowred.h.
//
// The determinism contract.  Everything here is an integer: counts, scans and 64-bit sums of integers, and the only atomics are
// integer adds.  a + b == b + a holds exactly, so no result depends on the order in which lanes, waves or workgroups arrive, on
// the tier or on the launch geometry.  Equal inputs give equal bits.
#pragma once
#include "dfd_rowred.h"

template <bool MAX>
__device__ __forceinline__ int count_op(int a, int b) { return MAX ? max(a, b) : a + b; }

// Exclusive scan of K non-negative ints per thread over a workgroup of NW waves, by + or by max (identity 0 for both): v becomes
// the combination over the threads before this one, total over all of them.  lds holds NW * K ints; the trailing barrier lets the
// caller reuse it at once.
template <int K, int NW, bool MAX = false>
__device__ __forceinline__ void block_scan_excl(int (&v)[K], int (&total)[K], int* lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int excl[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int x = v[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x = count_op<MAX>(x, y);
        }
        if (lane == 63) lds[w * K + k] = x;
        const int before = __shfl_up(x, 1, 64);
        excl[k] = lane ? before : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int before = 0, all = 0;
        for (int u = 0; u < NW; ++u) {
            const int s = lds[u * K + k];
            all = count_op<MAX>(all, s);
            if (u < w) before = count_op<MAX>(before, s);
        }
        v[k] = count_op<MAX>(before, excl[k]);
        total[k] = all;
    }
    __syncthreads();
}

// The sum of K 64-bit words (long or unsigned long long) per thread over a workgroup of NW waves, in every thread.  lds holds
// NW * K words; the first barrier also publishes what the caller wrote to LDS before the call, the trailing one frees lds.
template <int K, int NW, typename T>
__device__ __forceinline__ void block_sum(T (&v)[K], T* lds) {
    static_assert(sizeof(T) == 8, "64-bit integer words");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const T x = wave_sum(v[k]);
        if (lane == 0) lds[w * K + k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T s = 0;
        for (int u = 0; u < NW; ++u) s += lds[u * K + k];
        v[k] = s;
    }
    __syncthreads();
}
template <int NW, typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
    T one[1] = {v};
    block_sum<1, NW>(one, lds);
    return one[0];
}

// The counter flush: *p += v with one 64-bit integer atomic, none when v == 0.  The one place where the signed int64 counters of
// the ABI meet the unsigned atomic: two's complement, the same bits.
__device__ __forceinline__ void count_add(unsigned long long* p, unsigned long long v) {
    if (v) atomicAdd(p, v);
}
__device__ __forceinline__ void count_add(int64_t* p, long v) { count_add(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// The tie-group rule of sorted scores: a group ends at the last score and wherever the next score differs.  Float comparison, so
// -0.0 == +0.0 and a NaN ends its own group.  s_next is not read for the last score.
__device__ __forceinline__ bool tie_group_ends(float s, float s_next, bool is_last) { return is_last || !(s == s_next); }

// A static template like the kernels of dfd_rowred.h: only a file that launches it holds it.
// words[0..n) = 0 grid-stride, and workgroup 0 clears tail[0..ntail) as well
template <int THREADS>
static __global__ void __launch_bounds__(THREADS)
k_count_zero(uint32_t* __restrict__ words, size_t n, int64_t* __restrict__ tail, int ntail) {
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * THREADS) words[i] = 0;
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < ntail; i += THREADS) tail[i] = 0;
}

// 16 words per thread, at most 4096 workgroups
template <int THREADS>
static inline void count_zero(uint32_t* words, size_t n, int64_t* tail, int ntail, hipStream_t st) {
    size_t blocks = (n + THREADS * 16 - 1) / (THREADS * 16);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_count_zero<THREADS>, dim3((unsigned)blocks), dim3(THREADS), 0, st, words, n, tail, ntail);
}
