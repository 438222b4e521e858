// dfd_augment.hip — RandomRotation + ColorJitter of the reference's default 224-pixel training pipeline on the device
// (/root/reference/trainers/efficientnet.py:173-181: transforms.RandomRotation(10), transforms.ColorJitter(0.2, 0.2, 0.2, 0.05)),
// between the resize / crop kernel (dfd_resize.hip) and the flip / to-float / normalise / erase kernel (dfd_image_prep).
//
// BYTE work, restated from Pillow (which torchvision calls for PIL images) so that the result equals the CPU pipeline of data.py bit
// for bit — oracle/image_ref.py is the same arithmetic in numpy, pinned against Pillow itself:
//   rotate     Image.rotate(angle, NEAREST, expand=False) = Geometry.c affine_fixed: 16.16 fixed point, the six coefficients are
//              formed on the host in double precision exactly as Image.rotate forms them (data.rotate_plan); fill 0;
//   blends     ImageEnhance.{Brightness, Contrast, Color}.enhance(f) = Blend.c: (int)a + alpha * ((int)b - (int)a) evaluated in f32
//              (a multiply and an add, no fused multiply-add: built with -ffp-contract=off), truncated for 0 <= f <= 1, clipped
//              otherwise; Contrast's degenerate is the ROUNDED MEAN of convert("L") of the image AS IT IS when the operation runs
//              (after the operations that precede it in the drawn order), an integer reduction over the picture;
//   hue        convert("HSV") -> (h + delta) mod 256 -> convert("RGB"): Convert.c's float / double mix, spelled out.
// One 1024-thread workgroup per picture, the picture resident in LDS (H * W * 3 <= 156 KB: up to 228 x 228) for all of it: one
// read and one write of the batch for rotation + four colour operations + the reduction.
#include "dfd_common.h"

#define AUG_THREADS 1024
#define AUG_MAX_BYTES (156 * 1024)

__device__ __forceinline__ unsigned char aug_blend(int d, int v, float alpha, bool interp) {
    const float temp = (float)d + alpha * (float)(v - d);
    if (interp) return (unsigned char)(int)temp;
    if (temp <= 0.f) return 0;
    if (temp >= 255.f) return 255;
    return (unsigned char)(int)temp;
}
__device__ __forceinline__ int aug_l(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ void aug_rgb2hsv(int r, int g, int b, int& uh, int& us, int& uv) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    uv = maxc;
    if (minc == maxc) { uh = 0; us = 0; return; }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
    uh = aug_clip8((int)((double)h * 255.0));
    us = aug_clip8((int)((double)s * 255.0));
}
__device__ __forceinline__ void aug_hsv2rgb(int h, int s, int v, int& r, int& g, int& b) {
    if (s == 0) { r = g = b = v; return; }
    const double hd = (double)(float)h * 6.0 / 255.0;
    const int i = (int)floor(hd);
    const double f = (double)(float)(hd - (double)(float)i);
    const double fs = (double)(float)((double)(float)s / 255.0);
    const double vd = (double)(float)v;
    const int p = aug_clip8((int)floor(vd * (1.0 - fs) + 0.5));
    const int q = aug_clip8((int)floor(vd * (1.0 - fs * f) + 0.5));
    const int t = aug_clip8((int)floor(vd * (1.0 - fs * (1.0 - f)) + 0.5));
    switch (i % 6) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// The job as each kernel reads it: dfd_augment_job, or dfd_augment_policy_job, which starts with one.
template <bool POLICY> struct aug_job_of { typedef dfd_augment_job type; };
template <> struct aug_job_of<true> { typedef dfd_augment_policy_job type; };
__device__ __forceinline__ const dfd_augment_job& aug_base(const dfd_augment_job& j) { return j; }
__device__ __forceinline__ const dfd_augment_job& aug_base(const dfd_augment_policy_job& j) { return j.base; }

// Source pixel of output pixel (x, y) under a rotate_plan / shear_plan / translate_plan mode; false: outside the picture (fill 0).
__device__ __forceinline__ bool aug_source(int mode, const int* a, int x, int y, int H, int W, int& sx, int& sy) {
    sx = x; sy = y;
    if (mode == 1) {
        const long long xx = (long long)a[2] + (long long)y * a[1] + (long long)x * a[0];
        const long long yy = (long long)a[5] + (long long)y * a[4] + (long long)x * a[3];
        sx = (int)(xx >> 16); sy = (int)(yy >> 16);
        return sx >= 0 && sx < W && sy >= 0 && sy < H;
    }
    if (mode == 2) { sx = W - 1 - x; sy = H - 1 - y; }
    else if (mode == 3) { sy = x; sx = W - 1 - y; }
    else if (mode == 4) { sy = H - 1 - x; sx = y; }
    return true;
}

__device__ __forceinline__ void aug_brightness(unsigned char* img, int npx, int t, float a) {
    const bool interp = a >= 0.f && a <= 1.f;
    for (int i = t; i < npx * 3; i += AUG_THREADS) img[i] = aug_blend(0, img[i], a, interp);
}
// (every thread of the workgroup calls it: the mean is a reduction over the picture)
__device__ __forceinline__ void aug_contrast(unsigned char* img, int npx, int t, float a, int* red, int* mean_sh) {
    int part = 0;
    for (int p = t; p < npx; p += AUG_THREADS) part += aug_l(img[3 * p], img[3 * p + 1], img[3 * p + 2]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if ((t & 63) == 0) red[t >> 6] = part;
    __syncthreads();
    if (t == 0) {
        long long sum = 0;
        for (int k = 0; k < AUG_THREADS / 64; ++k) sum += red[k];
        *mean_sh = (int)((double)sum / (double)npx + 0.5);
    }
    __syncthreads();
    const int mean = *mean_sh;
    const bool interp = a >= 0.f && a <= 1.f;
    for (int i = t; i < npx * 3; i += AUG_THREADS) img[i] = aug_blend(mean, img[i], a, interp);
}
__device__ __forceinline__ void aug_color(unsigned char* img, int npx, int t, float a) {
    const bool interp = a >= 0.f && a <= 1.f;
    for (int p = t; p < npx; p += AUG_THREADS) {
        const int r = img[3 * p], g = img[3 * p + 1], b = img[3 * p + 2];
        const int l = aug_l(r, g, b);
        img[3 * p] = aug_blend(l, r, a, interp); img[3 * p + 1] = aug_blend(l, g, a, interp); img[3 * p + 2] = aug_blend(l, b, a, interp);
    }
}

// ---- the automatic augmentation policies (RandAugment / TrivialAugmentWide, ABI 139; tests/_randaug_ref.py restates these in numpy
// and is pinned against Pillow): ShearX/Y, TranslateX/Y and Rotate are the 16.16 gather above over the RESIDENT picture (an integer
// translation through Geometry.c ImagingScaleAffine is a plain shift, which the fixed-point form with unit scale reproduces exactly);
// Brightness, Color and Contrast are the blends above.
// One channel of ImageFilter.SMOOTH at an interior pixel (byte index i, `row` bytes per picture row): Filter.c ImagingFilter3x3 with
// the kernel (1,1,1; 1,5,1; 1,1,1) divided by 13 in f32; the row below, the row itself, the row above, each ((l * k + c * k) + r * k),
// added in that order onto the rounding 0.5; clip8.
__device__ __forceinline__ int aug_smooth(const unsigned char* img, int i, int row) {
    const float k1 = 1.f / 13.f, k5 = 5.f / 13.f;
    float ss = 0.5f;
    ss += ((float)img[i + row - 3] * k1 + (float)img[i + row] * k1) + (float)img[i + row + 3] * k1;
    ss += ((float)img[i - 3] * k1 + (float)img[i] * k5) + (float)img[i + 3] * k1;
    ss += ((float)img[i - row - 3] * k1 + (float)img[i - row] * k1) + (float)img[i - row + 3] * k1;
    return ss <= 0.f ? 0 : (ss >= 255.f ? 255 : (int)ss);
}

// The operations that read other pixels than the one they write: the nearest-neighbour gathers and Sharpness (the blend against
// SMOOTH, border pixels copied unfiltered).  The picture has no second LDS copy to spare, so each thread parks its new pixels in ITS
// OWN slots of `out` (this picture's part of the destination batch, which nothing reads before the final store), the workgroup
// meets, and each thread takes the same bytes back: a thread reading what it wrote itself needs program order only.  The caller's
// barrier follows.
__device__ __noinline__ void aug_neighbour_op(unsigned char* img, unsigned char* out, int op, int mode, float fp, const int* coef, int H, int W, int t) {
    const int npx = H * W;
    if (op == DFD_AUG_SHARPNESS) {
        const float a = fp;
        const bool interp = a >= 0.f && a <= 1.f;
        const int row = 3 * W;
        for (int p = t; p < npx; p += AUG_THREADS) {
            const int y = p / W, x = p - y * W;
            const bool inner = x >= 1 && x < W - 1 && y >= 1 && y < H - 1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * p + c, v = img[i];
                out[i] = aug_blend(inner ? aug_smooth(img, i, row) : v, v, a, interp);
            }
        }
    } else {
        for (int p = t; p < npx; p += AUG_THREADS) {
            const int y = p / W, x = p - y * W;
            int sx, sy;
            unsigned char r = 0, g = 0, b = 0;
            if (aug_source(mode, coef, x, y, H, W, sx, sy)) { const int q = 3 * (sy * W + sx); r = img[q]; g = img[q + 1]; b = img[q + 2]; }
            out[3 * p] = r; out[3 * p + 1] = g; out[3 * p + 2] = b;
        }
    }
    __syncthreads();
    for (int p = t; p < npx; p += AUG_THREADS) { img[3 * p] = out[3 * p]; img[3 * p + 1] = out[3 * p + 1]; img[3 * p + 2] = out[3 * p + 2]; }
}

// AutoContrast / Equalize: per-channel histograms with LDS atomics, then ImageOps' look-up table built over each histogram in place
// (one thread per channel walks its 256 bins in order: a bin is read before its table entry replaces it), then the table applied.
__device__ __noinline__ void aug_histogram_op(unsigned char* img, int* hist, int op, int npx, int t) {
    for (int i = t; i < 768; i += AUG_THREADS) hist[i] = 0;
    __syncthreads();
    for (int p = t; p < npx; p += AUG_THREADS) {
        atomicAdd(&hist[img[3 * p]], 1); atomicAdd(&hist[256 + img[3 * p + 1]], 1); atomicAdd(&hist[512 + img[3 * p + 2]], 1);
    }
    __syncthreads();
    if (t < 3) {
        int* h = hist + 256 * t;
        if (op == DFD_AUG_AUTOCONTRAST) {
            int lo = 0, hi = 255;
            while (lo < 255 && !h[lo]) ++lo;
            while (hi > 0 && !h[hi]) --hi;
            if (hi <= lo) { for (int i = 0; i < 256; ++i) h[i] = i; }
            else {
                const double scale = 255.0 / (double)(hi - lo), offset = (double)(-lo) * scale;
                for (int i = 0; i < 256; ++i) h[i] = aug_clip8((int)((double)i * scale + offset));
            }
        } else {
            int total = 0, last = 0, bins = 0;
            for (int i = 0; i < 256; ++i) if (h[i]) { total += h[i]; last = h[i]; ++bins; }
            const int step = bins <= 1 ? 0 : (total - last) / 255;
            if (!step) { for (int i = 0; i < 256; ++i) h[i] = i; }
            else {
                int n = step / 2;
                for (int i = 0; i < 256; ++i) { const int c = h[i]; h[i] = min(n / step, 255); n += c; }     // Image.point stores 8 bits, clipped
            }
        }
    }
    __syncthreads();
    for (int p = t; p < npx; p += AUG_THREADS) {
        img[3 * p] = (unsigned char)hist[img[3 * p]]; img[3 * p + 1] = (unsigned char)hist[256 + img[3 * p + 1]];
        img[3 * p + 2] = (unsigned char)hist[512 + img[3 * p + 2]];
    }
}

// POLICY false: dfd_augment_u8.  POLICY true: dfd_augment_policy_u8 — the horizontal flip folded into the first gather (the PIL
// pipeline flips AFTER the rotation: output pixel x is the rotated picture's pixel W - 1 - x), rotation and ColorJitter as before, then
// the policy's operations in their drawn order over the resident picture.
template <bool POLICY>
__global__ void __launch_bounds__(AUG_THREADS)
k_augment_u8(const unsigned char* __restrict__ src, const typename aug_job_of<POLICY>::type* __restrict__ jobs, unsigned char* __restrict__ dst,
             int H, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char img[];
    __shared__ int red[AUG_THREADS / 64];
    __shared__ int mean_sh;
    const int n = blockIdx.x, t = threadIdx.x;
    const dfd_augment_job jb = aug_base(jobs[n]);
    const int npx = H * W;
    const unsigned char* in = src + (long)n * npx * 3;
    bool flip = false;
    if constexpr (POLICY) flip = jobs[n].flip != 0;
    // ---- rotation (or copy): gather from global memory into the LDS picture
    for (int p = t; p < npx; p += AUG_THREADS) {
        const int y = p / W, x = p - y * W;
        int sx, sy;
        const bool ok = aug_source(jb.mode, jb.a, flip ? W - 1 - x : x, y, H, W, sx, sy);
        unsigned char r = 0, g = 0, b = 0;
        if (ok) { const unsigned char* q = in + ((long)sy * W + sx) * 3; r = q[0]; g = q[1]; b = q[2]; }
        img[3 * p] = r; img[3 * p + 1] = g; img[3 * p + 2] = b;
    }
    __syncthreads();
    // ---- the colour operations in the drawn order
    for (int slot = 0; slot < 4; ++slot) {
        const int op = jb.order[slot];
        if (op < 0 || op > 3 || !((jb.enable >> op) & 1)) continue;
        if (op == 0) aug_brightness(img, npx, t, jb.fb);
        else if (op == 1) aug_contrast(img, npx, t, jb.fc, red, &mean_sh);
        else if (op == 2) aug_color(img, npx, t, jb.fs);
        else {
            for (int p = t; p < npx; p += AUG_THREADS) {
                int h, s, v, r, g, b;
                aug_rgb2hsv(img[3 * p], img[3 * p + 1], img[3 * p + 2], h, s, v);
                h = (h + jb.dh) & 255;
                aug_hsv2rgb(h, s, v, r, g, b);
                img[3 * p] = (unsigned char)r; img[3 * p + 1] = (unsigned char)g; img[3 * p + 2] = (unsigned char)b;
            }
        }
        __syncthreads();
    }
    unsigned char* out = dst + (long)n * npx * 3;
    if constexpr (POLICY) {
        // ---- the policy's operations (3 KiB of histograms: 156 KiB + this + the reduction scratch stay within the CU's 160 KiB)
        __shared__ int hist[768];
        const int nops = min(max(jobs[n].nops, 0), DFD_AUG_MAX_OPS);
        for (int k = 0; k < nops; ++k) {
            const dfd_augment_op* o = &jobs[n].ops[k];          // in global memory, the same for every lane
            const int code = o->op, ip = o->ip;
            const float fp = o->fp;
            switch (code) {
                case DFD_AUG_SHEAR_X: case DFD_AUG_SHEAR_Y: case DFD_AUG_TRANSLATE_X: case DFD_AUG_TRANSLATE_Y: case DFD_AUG_ROTATE:
                    if (ip != 0) aug_neighbour_op(img, out, code, ip, fp, o->a, H, W, t);
                    break;
                case DFD_AUG_SHARPNESS: aug_neighbour_op(img, out, code, ip, fp, o->a, H, W, t); break;
                case DFD_AUG_BRIGHTNESS: aug_brightness(img, npx, t, fp); break;
                case DFD_AUG_COLOR: aug_color(img, npx, t, fp); break;
                case DFD_AUG_CONTRAST: aug_contrast(img, npx, t, fp, red, &mean_sh); break;
                case DFD_AUG_POSTERIZE:
                    for (int i = t; i < npx * 3; i += AUG_THREADS) img[i] = (unsigned char)(img[i] & ip);
                    break;
                case DFD_AUG_SOLARIZE:
                    for (int i = t; i < npx * 3; i += AUG_THREADS) { const int v = img[i]; img[i] = (unsigned char)((float)v < fp ? v : 255 - v); }
                    break;
                case DFD_AUG_AUTOCONTRAST: case DFD_AUG_EQUALIZE: aug_histogram_op(img, hist, code, npx, t); break;
                default: break;                                                     // DFD_AUG_IDENTITY
            }
            __syncthreads();
        }
    }
    for (int i = t; i < npx * 3; i += AUG_THREADS) out[i] = img[i];
}

extern "C" int dfd_augment_u8(const unsigned char* src, const dfd_augment_job* jobs_dev, unsigned char* dst, int N, int H, int W,
                              dfd_stream stream) {
    if (!src || !jobs_dev || !dst || N < 1 || H < 1 || W < 1 || src == dst) return DFD_EINVAL;
    const long bytes = (long)H * W * 3;
    if (bytes > AUG_MAX_BYTES || H >= 32768 || W >= 32768) return DFD_EUNSUPPORTED;        // the picture must fit one CU's LDS
    dfd_allow_lds_once<k_augment_u8<false>>(AUG_MAX_BYTES);
    hipLaunchKernelGGL(k_augment_u8<false>, dim3(N), dim3(AUG_THREADS), (size_t)((bytes + 15) / 16 * 16), (hipStream_t)stream, src, jobs_dev, dst, H, W);
    return DFD_CHECK_LAUNCH();
}

// The jobs are checked HERE, before anything is launched (an operation count or code outside the table, a transpose mode on a
// picture that is not square, which would gather outside it), so they come in host memory as well as on the device: `jobs_host` and
// `jobs_dev` are the same N records, and the copy behind `jobs_dev` may still be in flight on `stream`.
extern "C" int dfd_augment_policy_u8(const unsigned char* src, const dfd_augment_policy_job* jobs_host,
                                     const dfd_augment_policy_job* jobs_dev, unsigned char* dst, int N, int H, int W, dfd_stream stream) {
    if (!src || !jobs_host || !jobs_dev || !dst || N < 1 || H < 1 || W < 1 || src == dst) return DFD_EINVAL;
    const long bytes = (long)H * W * 3;
    if (bytes > AUG_MAX_BYTES || H >= 32768 || W >= 32768) return DFD_EUNSUPPORTED;        // the picture must fit one CU's LDS
    for (int n = 0; n < N; ++n) {
        const dfd_augment_policy_job& j = jobs_host[n];
        if (j.nops < 0 || j.nops > DFD_AUG_MAX_OPS || j.base.mode < 0 || j.base.mode > 4) return DFD_EINVAL;
        if (j.base.mode >= 3 && H != W) return DFD_EINVAL;
        for (int k = 0; k < j.nops; ++k) {
            const dfd_augment_op& o = j.ops[k];
            if (o.op < 0 || o.op >= DFD_AUG_NUM_OPS) return DFD_EINVAL;
            if (o.op >= DFD_AUG_SHEAR_X && o.op <= DFD_AUG_ROTATE && (o.ip < 0 || o.ip > 4 || (o.ip >= 3 && H != W))) return DFD_EINVAL;
        }
    }
    dfd_allow_lds_once<k_augment_u8<true>>(AUG_MAX_BYTES);
    hipLaunchKernelGGL(k_augment_u8<true>, dim3(N), dim3(AUG_THREADS), (size_t)((bytes + 15) / 16 * 16), (hipStream_t)stream, src, jobs_dev, dst, H, W);
    return DFD_CHECK_LAUNCH();
}
