// dfd_group.hip — pool the rows of a group (the frames of a video) into one row on the device (ABI 154; the contract is in
// include/dfd_hip.h).
//
// Everything that is summed is an integer: a probability becomes q = llrint(p 2^32), a vote is 2^32, and the (group, class) cells
// are uint64 sums; the max mode keeps one uint64 key per group under an integer max.  The only atomics are integer adds and maxima,
// so every output is independent of arrival order, tier and launch geometry (dfd_count.h: the contract, the counter flush, zeroing).
//   k_count_zero     the workspace and info
//   k_group_lds      LDS tier: a workgroup accumulates its rows into a private copy of the cells with LDS atomics, then adds its
//                    nonzero cells to the workspace with one global atomic each
//   k_group_glb      global tier: a wave takes 64 consecutive rows, merges each run of equal ids with a segmented scan over the
//                    lanes, and the run's last lane issues one global atomic per cell
//   k_group_finish   one thread per group: the division (or the gather of the winning row), the first arg max, target, size
// The workspace holds, for G groups of J classes: cells uint64 [G][J] (max mode: the key in cell [g] of the flat array), then
// uint32 size [G], lo [G] = max over members of J - target, hi [G] = max of target + 1; zero means "no member" in all of them.
#include "dfd_count.h"

#define GROUP_THREADS 256
#define GROUP_ROWS_PER_BLOCK 4096                                       // rows a workgroup takes at least before another one is added

struct GroupWs {
    unsigned long long* cell;
    uint32_t* size;
    uint32_t* lo;
    uint32_t* hi;
};

static __host__ __device__ __forceinline__ GroupWs group_ws(void* base, int G, int J) {
    GroupWs w;
    w.cell = reinterpret_cast<unsigned long long*>(base);
    w.size = reinterpret_cast<uint32_t*>(w.cell + (size_t)G * J);
    w.lo = w.size + G;
    w.hi = w.lo + G;
    return w;
}

// What one row contributes.  ok: the row is valid and its id lies in [0, G).  am: the first arg max of the row.
struct GroupRow {
    bool ok;
    int g, t, am;
};

// classify row i; counts an invalid row in bad and a valid row with an id out of range in oob
static __device__ __forceinline__ GroupRow group_row(const float* __restrict__ probs, const int* __restrict__ group,
                                                     const int64_t* __restrict__ targets, int i, int n, int G, int J, int& bad, int& oob) {
    GroupRow r = {false, -1, 0, 0};
    if (i >= n) return r;
    const float* row = probs + (size_t)i * J;
    const int64_t t = targets[i];
    bool valid = t >= 0 && t < J;
    float best = row[0];
    for (int j = 0; j < J; ++j) {
        const float p = row[j];
        if (!(p >= 0.f && p <= 1.f)) valid = false;                    // false for a NaN
        if (p > best) { best = p; r.am = j; }
    }
    if (!valid) { ++bad; return r; }
    const int g = group[i];
    if (g < 0 || g >= G) { ++oob; return r; }
    r.ok = true; r.g = g; r.t = (int)t;
    return r;
}

// cell j of a row: mean adds q, vote adds 2^32 to the cell of the arg max
static __device__ __forceinline__ unsigned long long group_q(const float* __restrict__ row, int j, int mode, int am) {
    if (mode == DFD_GROUP_VOTE) return j == am ? 0x100000000ull : 0ull;
    return (unsigned long long)llrint((double)row[j] * 4294967296.0);
}

// the max mode's key: the orderable bits of probs[i][positive] (-0.0 ties with 0.0) above the inverted row index; never 0
static __device__ __forceinline__ unsigned long long group_key(float p, int i) {
    const uint32_t bits = __float_as_uint(p + 0.f) | 0x80000000u;      // p >= 0: the bits ascend with the value
    return ((unsigned long long)bits << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
}

static __device__ __forceinline__ void group_count_flush(int bad, int oob, int64_t* __restrict__ info) {
    bad = wave_sum(bad); oob = wave_sum(oob);
    if ((threadIdx.x & 63) == 0) { count_add(info + 0, bad); count_add(info + 1, oob); }
}

__global__ void __launch_bounds__(GROUP_THREADS)
k_group_lds(const float* __restrict__ probs, const int* __restrict__ group, const int64_t* __restrict__ targets, int n, int G, int J,
            int mode, int positive, void* __restrict__ ws, int64_t* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) uint32_t group_lds[];
    const size_t words = ((size_t)G * J * 8 + (size_t)G * 12) / 4;
    for (size_t k = threadIdx.x; k < words; k += GROUP_THREADS) group_lds[k] = 0;
    __syncthreads();
    const GroupWs l = group_ws(group_lds, G, J), w = group_ws(ws, G, J);
    int bad = 0, oob = 0;
    for (int i = blockIdx.x * GROUP_THREADS + threadIdx.x; i < n; i += gridDim.x * GROUP_THREADS) {
        const GroupRow r = group_row(probs, group, targets, i, n, G, J, bad, oob);
        if (!r.ok) continue;
        const float* row = probs + (size_t)i * J;
        if (mode == DFD_GROUP_MAX) {
            atomicMax(&l.cell[r.g], group_key(row[positive], i));
        } else {
            for (int j = 0; j < J; ++j) {
                const unsigned long long q = group_q(row, j, mode, r.am);
                if (q) atomicAdd(&l.cell[(size_t)r.g * J + j], q);
            }
        }
        atomicAdd(&l.size[r.g], 1u);
        atomicMax(&l.lo[r.g], (uint32_t)(J - r.t));
        atomicMax(&l.hi[r.g], (uint32_t)(r.t + 1));
    }
    __syncthreads();
    const size_t cells = mode == DFD_GROUP_MAX ? (size_t)G : (size_t)G * J;
    for (size_t k = threadIdx.x; k < cells; k += GROUP_THREADS) {
        const unsigned long long v = l.cell[k];
        if (mode != DFD_GROUP_MAX) count_add(&w.cell[k], v);
        else if (v) atomicMax(&w.cell[k], v);
    }
    for (int g = threadIdx.x; g < G; g += GROUP_THREADS) {
        const uint32_t s = l.size[g];
        if (s) {
            atomicAdd(&w.size[g], s);
            atomicMax(&w.lo[g], l.lo[g]);
            atomicMax(&w.hi[g], l.hi[g]);
        }
    }
    group_count_flush(bad, oob, info);
}

// inclusive scan of x over the lanes start .. lane of this lane's run, by + or by max
template <bool MAX, typename T>
static __device__ __forceinline__ T group_seg_scan(T x, int lane, int start) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane - d >= start) x = MAX ? (y > x ? y : x) : x + y;
    }
    return x;
}

__global__ void __launch_bounds__(GROUP_THREADS)
k_group_glb(const float* __restrict__ probs, const int* __restrict__ group, const int64_t* __restrict__ targets, int n, int G, int J,
            int mode, int positive, void* __restrict__ ws, int64_t* __restrict__ info) {
    const GroupWs w = group_ws(ws, G, J);
    const int lane = threadIdx.x & 63;
    int bad = 0, oob = 0;
    // every lane of a wave runs the same trips: the shuffles below need all 64
    for (long base = (long)blockIdx.x * GROUP_THREADS; base < n; base += (long)gridDim.x * GROUP_THREADS) {
        const long at = base + threadIdx.x;
        const int i = at < n ? (int)at : n;
        const GroupRow r = group_row(probs, group, targets, i, n, G, J, bad, oob);
        const int before = __shfl_up(r.g, 1, 64), after = __shfl_down(r.g, 1, 64);
        const bool head = lane == 0 || before != r.g, tail = lane == 63 || after != r.g;
        const unsigned long long heads = __ballot(head) & (~0ull >> (63 - lane));      // the heads at or below this lane
        const int start = 63 - __clzll((long long)heads);
        const bool issue = r.ok && tail;                                // a run of rows that do not count has g = -1
        const float* row = probs + (size_t)(r.ok ? i : 0) * J;
        const uint32_t size = group_seg_scan<false>(r.ok ? 1u : 0u, lane, start);
        const uint32_t lo = group_seg_scan<true>(r.ok ? (uint32_t)(J - r.t) : 0u, lane, start);
        const uint32_t hi = group_seg_scan<true>(r.ok ? (uint32_t)(r.t + 1) : 0u, lane, start);
        if (mode == DFD_GROUP_MAX) {
            const unsigned long long key = group_seg_scan<true>(r.ok ? group_key(row[positive], i) : 0ull, lane, start);
            if (issue) atomicMax(&w.cell[r.g], key);
        } else {
            for (int j = 0; j < J; ++j) {
                const unsigned long long q = group_seg_scan<false>(r.ok ? group_q(row, j, mode, r.am) : 0ull, lane, start);
                if (issue) count_add(&w.cell[(size_t)r.g * J + j], q);
            }
        }
        if (issue) {
            atomicAdd(&w.size[r.g], size);
            atomicMax(&w.lo[r.g], lo);
            atomicMax(&w.hi[r.g], hi);
        }
    }
    group_count_flush(bad, oob, info);
}

__global__ void __launch_bounds__(GROUP_THREADS)
k_group_finish(const float* __restrict__ probs, int G, int J, int mode, const void* __restrict__ ws, float* __restrict__ out_probs,
               int64_t* __restrict__ out_preds, int64_t* __restrict__ out_targets, int* __restrict__ sizes, int64_t* __restrict__ info) {
    const GroupWs w = group_ws(const_cast<void*>(ws), G, J);
    const int g = blockIdx.x * GROUP_THREADS + threadIdx.x;
    const bool live = g < G;
    const uint32_t size = live ? w.size[g] : 0u;
    bool mixed = false;
    if (live) {
        float* out = out_probs + (size_t)g * J;
        int am = 0;
        if (size == 0) {
            for (int j = 0; j < J; ++j) out[j] = 0.f;
        } else {
            const float* src = mode == DFD_GROUP_MAX ? probs + (size_t)(0xffffffffu - (uint32_t)(w.cell[g] & 0xffffffffull)) * J : nullptr;
            const double den = (double)size * 4294967296.0;
            float best = 0.f;
            for (int j = 0; j < J; ++j) {
                const float v = src ? src[j] : (float)((double)w.cell[(size_t)g * J + j] / den);
                out[j] = v;
                if (j == 0 || v > best) { best = v; am = j; }
            }
            mixed = (int)w.hi[g] - 1 != J - (int)w.lo[g];
        }
        out_preds[g] = am;
        out_targets[g] = size ? (int64_t)(J - (int)w.lo[g]) : -1;
        sizes[g] = (int)size;
    }
    const int n_mixed = __popcll(__ballot(mixed)), n_empty = __popcll(__ballot(live && size == 0));
    if ((threadIdx.x & 63) == 0) { count_add(info + 2, n_mixed); count_add(info + 3, n_empty); }
}

static bool group_shape_ok(int n, int G, int J) { return G >= 1 && G <= n && n <= DFD_GROUP_MAX_N && J >= 1 && J <= DFD_GROUP_MAX_J; }

extern "C" size_t dfd_group_ws(int n, int G, int J) {
    if (!group_shape_ok(n, G, J)) return 0;
    return (size_t)G * J * 8 + (size_t)G * 12;
}

extern "C" int dfd_group_plan(int n, int G, int J, int* plan) {
    if (!group_shape_ok(n, G, J) || !plan) return DFD_EINVAL;
    const size_t bytes = dfd_group_ws(n, G, J);
    const bool lds = bytes <= DFD_GROUP_LDS_BYTES;
    const int cap = lds ? DFD_GROUP_LDS_MAX_BLOCKS : DFD_GROUP_GLOBAL_MAX_BLOCKS;
    const int per = lds ? GROUP_ROWS_PER_BLOCK : GROUP_THREADS;
    int blocks = (n + per - 1) / per;
    if (blocks > cap) blocks = cap;
    plan[0] = lds ? DFD_GROUP_TIER_LDS : DFD_GROUP_TIER_GLOBAL;
    plan[1] = blocks;
    plan[2] = lds ? (int)bytes : 0;
    plan[3] = (G + GROUP_THREADS - 1) / GROUP_THREADS;
    return DFD_OK;
}

extern "C" int dfd_group_pool(const float* probs, const int* group, const int64_t* targets, int n, int G, int J, int mode, int positive,
                              void* ws, size_t ws_bytes, float* out_probs, int64_t* out_preds, int64_t* out_targets, int* sizes,
                              int64_t* info, dfd_stream stream) {
    int plan[4];
    if (dfd_group_plan(n, G, J, plan) != DFD_OK) return DFD_EINVAL;
    if (mode < DFD_GROUP_MEAN || mode > DFD_GROUP_MAX || positive < 0 || positive >= J) return DFD_EINVAL;
    if (!probs || !group || !targets || !ws || !out_probs || !out_preds || !out_targets || !sizes || !info) return DFD_EINVAL;
    const size_t need = dfd_group_ws(n, G, J);
    if (ws_bytes < need || ((uintptr_t)ws & 7)) return DFD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    count_zero<GROUP_THREADS>((uint32_t*)ws, need / 4, info, 4, st);
    if (plan[0] == DFD_GROUP_TIER_LDS) {
        dfd_allow_lds_once<k_group_lds>(DFD_GROUP_LDS_BYTES);
        hipLaunchKernelGGL(k_group_lds, dim3(plan[1]), dim3(GROUP_THREADS), (size_t)plan[2], st, probs, group, targets, n, G, J, mode,
                           positive, ws, info);
    } else
        hipLaunchKernelGGL(k_group_glb, dim3(plan[1]), dim3(GROUP_THREADS), 0, st, probs, group, targets, n, G, J, mode, positive, ws, info);
    hipLaunchKernelGGL(k_group_finish, dim3(plan[3]), dim3(GROUP_THREADS), 0, st, probs, G, J, mode, (const void*)ws, out_probs, out_preds,
                       out_targets, sizes, info);
    return DFD_CHECK_LAUNCH();
}
