// dfd_mix.hip — Mixup / CutMix of an f32 image batch in place, plus its soft targets (mix.BatchMixer; timm data/mixup.py Mixup).
//
// dfd_mix_batch
//   The partner of sample i is j = N - 1 - i (timm's x.flip(0)).  One job per sample, DFD_MIX_JOB_WORDS 32-bit words
//   {mode, w0, w1, y0, y1, x0, x1, pad}; w0, w1 are f32 bit patterns:
//     DFD_MIX_KEEP    picture untouched, y[i] = onehot(labels[i])
//     DFD_MIX_MIXUP   x[i] = fl(fl(x_i * w0) + fl(x_j * w1))        three f32 roundings in this order, no FMA
//     DFD_MIX_CUTMIX  pixels with y0 <= row < y1 and x0 <= col < x1 take the partner's value, all channels
//   targets of the two mixing modes: zeros, y[i][labels[i]] = w0, then y[i][labels[j]] += w1.
//   x_i, x_j are the values BEFORE the launch, and the two jobs of a pair may differ, so one lane owns the same position of
//   both pictures: it loads both, then stores both.  Workgroups are dealt to pairs (i < j; an odd N's middle sample is its
//   own partner and is always kept): `bpp` per pair, grid = pairs * bpp capped near 2048 workgroups, the rest strided.
//
//   Bytes.  Both jobs keep: the workgroups of the pair leave after reading the two jobs.  No mixup in the pair: a wave per
//   64 slots of a row of the bounding rectangle of the two boxes; a lane whose 16 bytes lie in neither box touches no
//   memory, so loads and stores stay inside the union.  Only mixup / keep: one flat pass over the picture (the layout does not matter), a
//   kept side is loaded but not stored.  Mixup on one side and cutmix on the other: the same over whole picture rows.
//
//   Access width.  A lane owns one 16-byte-aligned slot of four floats.  A slot that lies wholly inside the span moves as
//   one 16-byte load and store per picture; the slots at a span's ends (a box row in NHWC starts at 3 * x0 floats) go float
//   by float.  That needs both pictures at the same address modulo 16, which holds whenever 3 * H * W is a multiple of
//   four; otherwise every slot goes float by float.
//
//   Box coordinates are clamped to the picture and the targets are written by comparing class numbers, so no job and no
//   label can make the kernel leave x or y.
#include "dfd_common.h"

#pragma clang fp contract(off)

namespace {

// one side of a pair, for the span at hand: [lo, hi) are the picture-relative floats that take the partner's value
struct MixSide {
    int pmode;                  // what happens to the picture: cutmix with an empty box, or an unknown mode, keeps it
    float w0, w1;
    int y0, y1, x0, x1;
    int lo, hi;
};

__device__ __forceinline__ MixSide mix_load_job(const int32_t* __restrict__ jobs, int n, int H, int W, int& mode) {
    const int32_t* r = jobs + (long)n * DFD_MIX_JOB_WORDS;
    MixSide s;
    mode = r[0];
    s.w0 = __int_as_float(r[1]);
    s.w1 = __int_as_float(r[2]);
    s.y0 = max(r[3], 0); s.y1 = min(r[4], H);
    s.x0 = max(r[5], 0); s.x1 = min(r[6], W);
    s.pmode = mode == DFD_MIX_MIXUP ? DFD_MIX_MIXUP
            : (mode == DFD_MIX_CUTMIX && s.y1 > s.y0 && s.x1 > s.x0) ? DFD_MIX_CUTMIX : DFD_MIX_KEEP;
    s.lo = s.hi = 0;
    return s;
}

__device__ __forceinline__ float mix_val(float own, float other, int p, const MixSide& s) {
    if (s.pmode == DFD_MIX_MIXUP) {
        const float a = own * s.w0;
        const float b = other * s.w1;
        return a + b;
    }
    return (p >= s.lo && p < s.hi) ? other : own;
}
__device__ __forceinline__ bool mix_touches(const MixSide& s, int a, int b) {
    return s.pmode == DFD_MIX_MIXUP || (a < s.hi && b > s.lo);
}

// the 16-byte slot that starts `lo` floats into both pictures, cut to the span [s, e)
__device__ __forceinline__ void mix_slot(float* __restrict__ pi, float* __restrict__ pj, int lo, int s, int e, bool vec_ok,
                                         const MixSide& si, const MixSide& sj) {
    const int a = max(lo, s), b = min(lo + 4, e);
    if (a >= b) return;
    const bool ti = mix_touches(si, a, b), tj = mix_touches(sj, a, b);
    if (!ti && !tj) return;
    if (vec_ok && b - a == 4) {
        const float4 vi = *reinterpret_cast<const float4*>(pi + lo);
        const float4 vj = *reinterpret_cast<const float4*>(pj + lo);
        if (ti) {
            float4 o;
            o.x = mix_val(vi.x, vj.x, lo, si); o.y = mix_val(vi.y, vj.y, lo + 1, si);
            o.z = mix_val(vi.z, vj.z, lo + 2, si); o.w = mix_val(vi.w, vj.w, lo + 3, si);
            *reinterpret_cast<float4*>(pi + lo) = o;
        }
        if (tj) {
            float4 o;
            o.x = mix_val(vj.x, vi.x, lo, sj); o.y = mix_val(vj.y, vi.y, lo + 1, sj);
            o.z = mix_val(vj.z, vi.z, lo + 2, sj); o.w = mix_val(vj.w, vi.w, lo + 3, sj);
            *reinterpret_cast<float4*>(pj + lo) = o;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = lo + k;
        if (p < a || p >= b) continue;
        const float vi = pi[p], vj = pj[p];
        if (ti) pi[p] = mix_val(vi, vj, p, si);
        if (tj) pj[p] = mix_val(vj, vi, p, sj);
    }
}

__device__ __forceinline__ float mix_target(int c, int own, int other, int mode, float w0, float w1) {
    if (mode != DFD_MIX_MIXUP && mode != DFD_MIX_CUTMIX) return c == own ? 1.f : 0.f;
    return (c == own ? w0 : 0.f) + (c == other ? w1 : 0.f);
}

__global__ void __launch_bounds__(DFD_THREADS)
k_mix_batch(float* __restrict__ x, const int64_t* __restrict__ labels, const int32_t* __restrict__ jobs,
            float* __restrict__ y, int N, int H, int W, int J, int nchw, int bpp) {
    const int pair = blockIdx.x / bpp, sub = blockIdx.x - pair * bpp;
    const int i = pair, j = N - 1 - pair;
    const int t = threadIdx.x;
    int mode_i, mode_j;
    MixSide si = mix_load_job(jobs, i, H, W, mode_i);
    MixSide sj = mix_load_job(jobs, j, H, W, mode_j);
    if (i == j) {                                   // the middle sample of an odd batch has no partner
        mode_i = mode_j = DFD_MIX_KEEP;
        si.pmode = sj.pmode = DFD_MIX_KEEP;
    }
    if (sub == 0) {
        const int li = (int)labels[i], lj = (int)labels[j];
        for (int c = t; c < J; c += DFD_THREADS) {
            y[(long)i * J + c] = mix_target(c, li, lj, mode_i, si.w0, si.w1);
            if (j != i) y[(long)j * J + c] = mix_target(c, lj, li, mode_j, sj.w0, sj.w1);
        }
    }
    if (si.pmode == DFD_MIX_KEEP && sj.pmode == DFD_MIX_KEEP) return;

    const int n = 3 * H * W;
    float* pi = x + (long)i * n;
    float* pj = x + (long)j * n;
    const uintptr_t ai = reinterpret_cast<uintptr_t>(pi), aj = reinterpret_cast<uintptr_t>(pj);
    const bool vec_ok = ((ai ^ aj) & 15) == 0;
    const int mis = (int)((ai >> 2) & 3);           // slot k starts 4 * k - mis floats into the picture
    const bool any_mixup = si.pmode == DFD_MIX_MIXUP || sj.pmode == DFD_MIX_MIXUP;
    const bool any_cut = si.pmode == DFD_MIX_CUTMIX || sj.pmode == DFD_MIX_CUTMIX;

    if (!any_cut) {                                 // mixup / keep: the picture is one span
        const int nslots = (n + mis + 3) >> 2;
        for (int k = sub * DFD_THREADS + t; k < nslots; k += bpp * DFD_THREADS)
            mix_slot(pi, pj, 4 * k - mis, 0, n, vec_ok, si, sj);
        return;
    }
    // a wave per 64 slots of a row: all rows and columns when one side is a mixup, else the bounding rectangle of the boxes
    int R0 = 0, R1 = H, X0 = 0, X1 = W;
    if (!any_mixup) {
        const bool ci = si.pmode == DFD_MIX_CUTMIX, cj = sj.pmode == DFD_MIX_CUTMIX;
        R0 = min(ci ? si.y0 : H, cj ? sj.y0 : H); R1 = max(ci ? si.y1 : 0, cj ? sj.y1 : 0);
        X0 = min(ci ? si.x0 : W, cj ? sj.x0 : W); X1 = max(ci ? si.x1 : 0, cj ? sj.x1 : 0);
    }
    const int nr = R1 - R0, planes = nchw ? 3 : 1, mul = nchw ? 1 : 3;
    const int cpr = (((X1 - X0) * mul + 3) / 4 + 1 + 63) / 64;         // 64-slot chunks that cover any row's slots
    const int lane = t & 63, wave = sub * (DFD_THREADS / 64) + (t >> 6), nwaves = bpp * (DFD_THREADS / 64);
    for (int u = wave; u < nr * planes * cpr; u += nwaves) {
        const int q = u / cpr, chunk = u - q * cpr;
        const int c = q / nr, r = R0 + (q - c * nr);
        const int base = nchw ? (c * H + r) * W : r * W * 3;
        const int s = base + X0 * mul, e = base + X1 * mul;
        const bool ri = si.pmode == DFD_MIX_CUTMIX && r >= si.y0 && r < si.y1;
        const bool rj = sj.pmode == DFD_MIX_CUTMIX && r >= sj.y0 && r < sj.y1;
        si.lo = ri ? base + si.x0 * mul : 0; si.hi = ri ? base + si.x1 * mul : 0;
        sj.lo = rj ? base + sj.x0 * mul : 0; sj.hi = rj ? base + sj.x1 * mul : 0;
        const int k = ((s + mis) >> 2) + chunk * 64 + lane;
        if (k < ((e + mis + 3) >> 2)) mix_slot(pi, pj, 4 * k - mis, s, e, vec_ok, si, sj);
    }
}

}  // namespace

extern "C" int dfd_mix_batch(float* x, const int64_t* labels, const int32_t* jobs, float* y, int N, int H, int W, int J,
                             int layout, dfd_stream stream) {
    if (!x || !labels || !jobs || !y || N < 1 || J < 1 || H < 1 || W < 1) return DFD_EINVAL;
    if (layout != DFD_MIX_NHWC && layout != DFD_MIX_NCHW) return DFD_EINVAL;
    if (3L * H * W > 0x7fffff00L) return DFD_EINVAL;            // picture offsets are ints
    const int npairs = (N + 1) / 2;
    // memory-bound: about four slots a thread, and about 2048 workgroups at the most; the rest is strided
    const long slots = (3L * H * W + 3) / 4;
    const long want = (slots + 4 * DFD_THREADS - 1) / (4 * DFD_THREADS);
    const long cap = npairs >= 2048 ? 1 : 2048 / npairs;
    const int bpp = (int)(want < cap ? want : cap);
    hipLaunchKernelGGL(k_mix_batch, dim3((unsigned)npairs * (unsigned)bpp), dim3(DFD_THREADS), 0, (hipStream_t)stream,
                       x, labels, jobs, y, N, H, W, J, layout == DFD_MIX_NCHW ? 1 : 0, bpp);
    return DFD_CHECK_LAUNCH();
}
