// dfd_rowred.h — the row-reduction toolkit of the evaluation kernels (dfd_calib.hip, dfd_fuse.hip, the softmax / loss kernels of
// dfd_misc.hip): wave and workgroup reductions, the first arg max of a wave, and the two-stage sum over the rows of an [n][J] input.
//
// The two-stage sum.  A row layout (rowred_plan) gives every thread one row of a chunk of ROWRED_ROWS_THREAD rows, or every wave
// ROWRED_WAVE_ROWS consecutive rows of a chunk of ROWRED_ROWS_WAVE, lane l holding columns l, l + 64, ...  Stage 1 runs
// min(chunks, cap) workgroups of ROWRED_THREADS threads, workgroup b taking chunks b, b + blocks, ...; its waves keep running sums
// in LDS and rowred_stage1_store writes the workgroup's partials.  Stage 2 (k_rowred_sum) is ONE workgroup in a later launch on the
// same stream: no workgroup ever waits for another one.
//
// The determinism contract.  Integer results are sums of integers.  The f64 results are summed in an order that the shape alone
// fixes: lanes by an xor butterfly (o = 32..1), trips and waves in index order, workgroups by k_rowred_sum.  Equal inputs give
// equal bits.
#pragma once
#include "dfd_common.h"

#define ROWRED_THREADS 256
#define ROWRED_WAVES (ROWRED_THREADS / 64)
#define ROWRED_ROWS_THREAD ROWRED_THREADS                           // rows per chunk, one thread per row
#define ROWRED_WAVE_ROWS 8                                          // consecutive rows per wave and chunk, one wave per row
#define ROWRED_ROWS_WAVE (ROWRED_WAVES * ROWRED_WAVE_ROWS)
#define ROWRED_STAGE2_WIDTH 64                                      // stage 2 sums one output per wave trip
#define ROWRED_LAYOUT_THREAD 0
#define ROWRED_LAYOUT_WAVE 1
static_assert(DFD_CALIB_STAGE2_WIDTH == ROWRED_STAGE2_WIDTH && DFD_FUSE_STAGE2_WIDTH == ROWRED_STAGE2_WIDTH, "one stage-2 kernel");
static_assert(DFD_CALIB_LAYOUT_THREAD == ROWRED_LAYOUT_THREAD && DFD_FUSE_LAYOUT_THREAD == ROWRED_LAYOUT_THREAD, "one row plan");
static_assert(DFD_CALIB_LAYOUT_WAVE == ROWRED_LAYOUT_WAVE && DFD_FUSE_LAYOUT_WAVE == ROWRED_LAYOUT_WAVE, "one row plan");
static_assert(DFD_CALIB_MAX_BLOCKS == DFD_FUSE_MAX_BLOCKS, "one size of the stage-2 loop");

// ------------------------------------------------------------------ a wave: every lane ends with the same bits (a + b == b + a)
template <typename T>                                               // float, double, long
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// The first arg max of the lanes' (value, index) pairs, lowest index on ties
__device__ __forceinline__ void wave_first_argmax(float& best, int& arg) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
}

__device__ __forceinline__ bool f32_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// Sum or max over a workgroup of DFD_THREADS threads, in every thread; sm: 4 floats of LDS, which the next call may take again
__device__ __forceinline__ float block_reduce(float v, float* sm, bool is_max) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    float r = sm[0];
    for (int i = 1; i < DFD_THREADS / 64; ++i) r = is_max ? fmaxf(r, sm[i]) : r + sm[i];
    return r;
}

// ------------------------------------------------------------------ the two-stage sum
struct rowred_plan_t { int layout, rows, blocks, trips; };

static inline rowred_plan_t rowred_plan(int n, bool thread_layout, int max_blocks) {
    rowred_plan_t p;
    p.layout = thread_layout ? ROWRED_LAYOUT_THREAD : ROWRED_LAYOUT_WAVE;
    p.rows = thread_layout ? ROWRED_ROWS_THREAD : ROWRED_ROWS_WAVE;
    const long chunks = ((long)n + p.rows - 1) / p.rows;
    p.blocks = (int)(chunks < 1 ? 1 : (chunks > max_blocks ? max_blocks : chunks));
    p.trips = (p.blocks + ROWRED_STAGE2_WIDTH - 1) / ROWRED_STAGE2_WIDTH;
    return p;
}

// The kernels are templates so that only a file that launches one holds it, and static so that each such file holds its own.
// One workgroup of THREADS threads: three int64 ranges = 0
template <int THREADS>
static __global__ void __launch_bounds__(THREADS)
k_rowred_zero(int64_t* __restrict__ a, int na, int64_t* __restrict__ b, int nb, int64_t* __restrict__ c, int nc) {
    for (int i = threadIdx.x; i < na; i += THREADS) a[i] = 0;
    for (int i = threadIdx.x; i < nb; i += THREADS) b[i] = 0;
    for (int i = threadIdx.x; i < nc; i += THREADS) c[i] = 0;
}

// The end of a stage-1 kernel.  acc: the waves' running sums in LDS, wave u's sum of output o = g * group + q (q < group) at
// acc[u][g][q]; nonfinite, oob: the thread's two row counts, icount: LDS for the waves'.  part[o * blocks + b] = workgroup b's sum
// of output o, the waves added in the order 0, 1, 2, 3, and ipart[t * blocks + b] its row count t < 2.
template <int GROUPS, int GROUP_STRIDE>
__device__ __forceinline__ void rowred_stage1_store(const double (&acc)[ROWRED_WAVES][GROUPS][GROUP_STRIDE], long (&icount)[ROWRED_WAVES][2],
                                                    int outputs, int group, long nonfinite, long oob, double* __restrict__ part,
                                                    int64_t* __restrict__ ipart) {
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    nonfinite = wave_sum(nonfinite); oob = wave_sum(oob);
    if (lane == 0) { icount[w][0] = nonfinite; icount[w][1] = oob; }
    __syncthreads();
    const int blocks = gridDim.x;
    for (int o = t; o < outputs; o += ROWRED_THREADS) {
        const int g = o / group, q = o - g * group;
        double s = acc[0][g][q];
        for (int u = 1; u < ROWRED_WAVES; ++u) s += acc[u][g][q];
        part[(long)o * blocks + blockIdx.x] = s;
    }
    if (t < 2) {
        long s = 0;
        for (int u = 0; u < ROWRED_WAVES; ++u) s += icount[u][t];
        ipart[(long)t * blocks + blockIdx.x] = s;
    }
}

// Stage 2, one workgroup: out[o] = the sum over b < blocks of part[o * blocks + b], o < nf (f64) — wave w takes o = w, w + 4, ...,
// its lanes the partials lane, lane + 64, ... in `trips` trips, then the butterfly — and iout[o] likewise over ipart (int64), o < ni.
template <int THREADS>
static __global__ void __launch_bounds__(THREADS)
k_rowred_sum(const double* __restrict__ part, int nf, const int64_t* __restrict__ ipart, int ni, int blocks, int trips,
             double* __restrict__ out, int64_t* __restrict__ iout) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = w; o < nf; o += THREADS / 64) {
        double s = 0.0;
        for (int trip = 0; trip < trips; ++trip) {
            const int b = trip * ROWRED_STAGE2_WIDTH + lane;
            if (b < blocks) s += part[(long)o * blocks + b];
        }
        s = wave_sum(s);
        if (lane == 0) out[o] = s;
    }
    for (int o = w; o < ni; o += THREADS / 64) {
        long s = 0;
        for (int trip = 0; trip < trips; ++trip) {
            const int b = trip * ROWRED_STAGE2_WIDTH + lane;
            if (b < blocks) s += ipart[(long)o * blocks + b];
        }
        s = wave_sum(s);
        if (lane == 0) iout[o] = s;
    }
}
