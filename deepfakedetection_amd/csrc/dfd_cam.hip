// dfd_cam.hip — Grad-CAM heatmaps and overlays on the device (reference web_ui.py:275-282: pytorch_grad_cam.GradCAM with one
// target layer, then show_cam_on_image(rgb, mask, use_rgb=True) with image_weight 0.5).
//
// dfd_gradcam_map   (GradCAM.get_cam_weights + get_cam_image + np.maximum(cam, 0))
//   w[c]   = (sum_p grad[n,p,c]) / HW                       np.mean over (H, W): sum, then divide
//   cam[p] = max(0, sum_c w[c] * act[n,p,c])
//   One workgroup per image.  Step 1: thread t owns channels t, t+1024, ... and sums the HW rows in order; the weights go to
//   LDS.  Step 2: wave v owns pixels v, v+16, ...; lane l sums channels l, l+64, ... in order, then a fixed xor butterfly.
//   Every sum has one order: bitwise reproducible.  Bytes: 2 N HW C elt in, N HW 4 out — one pass over act and grad.
//
// dfd_cam_render    (scale_cam_image with the resize, aggregate_multi_layers, show_cam_on_image)
//   cam  = (cam - min) / (1e-7 + max)                       on the h x w map
//   cam  = cv2.resize(cam, (W, H)) INTER_LINEAR, f32        half-pixel centres, edge clamping, horizontal pass then vertical
//   heat = relu(cam), then (heat - min) / (1e-7 + max)      the [N][H][W] f32 heatmap
//   img  = clamp(x * std + mean, 0, 1)                      web_ui._tensor_to_rgb on the normalised NCHW f32 input
//   o    = (1 - iw) * lut[uint8(255 heat)] / 255 + iw * img, o /= max(o), overlay = uint8(255 o)
//   One workgroup per image, one launch: the horizontal pass goes to the workspace ([N][h][W] f32), the vertical pass writes
//   the unscaled heat to heat_out, and each later phase re-reads only what the same thread wrote.  Every phase that needs a
//   per-image min / max ends in a block reduction (min / max are exact in any order).
//   Operation by operation the f32 arithmetic of numpy (tests/_cam_ref.py): contraction is off (here and in build.FLAGS) and
//   every division is the correctly rounded one.  The cv2 coefficients follow resize(): scale = 1 / (W / w) in double,
//   fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), f = fx - sx; sx < 0 or sx >= w - 1 clamp with f = 0.
#include "dfd_rowred.h"

#pragma clang fp contract(off)

#define CAM_MAP_THREADS 1024
#define CAM_RENDER_THREADS 1024
#define CAM_MAX_C 16384              // step-1 weights live in LDS: 64 KiB

template <typename T> __device__ __forceinline__ float cam_ld(const T* p, long i);
template <> __device__ __forceinline__ float cam_ld<float>(const float* p, long i) { return p[i]; }
template <> __device__ __forceinline__ float cam_ld<bf16>(const bf16* p, long i) { return bf2f(p[i].x); }

template <typename T>
__global__ void __launch_bounds__(CAM_MAP_THREADS)
k_gradcam_map(const T* __restrict__ act, const T* __restrict__ grad, int HW, int C, float* __restrict__ cam) {
    extern __shared__ float w_sh[];
    const int n = blockIdx.x, tid = threadIdx.x;
    const long base = (long)n * HW * C;
    const float inv_div = (float)HW;
    for (int c = tid; c < C; c += CAM_MAP_THREADS) {
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s = s + cam_ld(grad, base + (long)p * C + c);
        w_sh[c] = __fdiv_rn(s, inv_div);
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int p = wave; p < HW; p += CAM_MAP_THREADS / 64) {
        float acc = 0.f;
        const long row = base + (long)p * C;
        for (int c = lane; c < C; c += 64) acc = acc + w_sh[c] * cam_ld(act, row + c);
        acc = wave_sum(acc);
        if (lane == 0) cam[(long)n * HW + p] = acc < 0.f ? 0.f : acc;
    }
}

// min and max over the workgroup; every thread gets both
__device__ __forceinline__ void cam_block_minmax(float& mn, float& mx, float* red) {
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                               // red[] may still be read by the previous reduction
    if ((threadIdx.x & 63) == 0) { red[2 * wave] = mn; red[2 * wave + 1] = mx; }
    __syncthreads();
    mn = red[0]; mx = red[1];
    for (int v = 1; v < CAM_RENDER_THREADS / 64; ++v) { mn = fminf(mn, red[2 * v]); mx = fmaxf(mx, red[2 * v + 1]); }
}

// cv2 INTER_LINEAR source index pair and weights of destination index d (resize() of imgproc/resize.cpp, ksize 2)
__device__ __forceinline__ void cam_coeff(int d, double scale, int in, int& s0, int& s1, float& a0, float& a1) {
    const float fx = (float)((d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    float f = fx - (float)sx;
    if (sx < 0) { sx = 0; f = 0.f; }
    if (sx >= in - 1) { sx = in - 1; f = 0.f; }
    s0 = sx;
    s1 = sx + 1 < in ? sx + 1 : in - 1;
    a0 = 1.f - f;
    a1 = f;
}

__device__ __forceinline__ float cam_overlay(float heat, int c, float xin, const float* __restrict__ mean_std,
                                             const unsigned char* __restrict__ lut, float wl, float wi) {
    int idx = (int)(255.f * heat);                 // np.uint8(255 * mask): truncation; heat is in [0, 1]
    idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);
    const float l = __fdiv_rn((float)lut[idx * 3 + c], 255.f);
    float im = xin * mean_std[3 + c] + mean_std[c];
    im = fminf(fmaxf(im, 0.f), 1.f);
    return wl * l + wi * im;
}

__global__ void __launch_bounds__(CAM_RENDER_THREADS)
k_cam_render(const float* __restrict__ cam, int h, int w, int H, int W, double sx_scale, double sy_scale,
             const float* __restrict__ image, const float* __restrict__ mean_std, const unsigned char* __restrict__ lut,
             float wl, float wi, float* __restrict__ heat_out, unsigned char* __restrict__ overlay_out, float* __restrict__ tmp_ws) {
    __shared__ float red[2 * (CAM_RENDER_THREADS / 64)];
    const int n = blockIdx.x, tid = threadIdx.x;
    const long HWo = (long)H * W;
    const float* S = cam + (long)n * h * w;
    float* tmp = tmp_ws + (long)n * h * W;
    float* heat = heat_out + (long)n * HWo;

    // 1. min-max of the low-resolution map
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < h * w; i += CAM_RENDER_THREADS) { const float v = S[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    cam_block_minmax(mn, mx, red);
    const float lmin = mn, lden = 1e-7f + (mx - mn);       // max(cam - min) == fl(max - min): rounding is monotonic

    // 2. horizontal pass on the scaled map -> tmp [h][W]
    for (long i = tid; i < (long)h * W; i += CAM_RENDER_THREADS) {
        const int y = (int)(i / W), dx = (int)(i % W);
        int s0, s1; float a0, a1;
        cam_coeff(dx, sx_scale, w, s0, s1, a0, a1);
        const float v0 = __fdiv_rn(S[y * w + s0] - lmin, lden);
        const float v1 = __fdiv_rn(S[y * w + s1] - lmin, lden);
        tmp[i] = v0 * a0 + v1 * a1;
    }
    __syncthreads();

    // 3. vertical pass, ReLU -> heat (unscaled); min / max
    mn = INFINITY; mx = -INFINITY;
    for (long i = tid; i < HWo; i += CAM_RENDER_THREADS) {
        const int dy = (int)(i / W), x = (int)(i % W);
        int s0, s1; float b0, b1;
        cam_coeff(dy, sy_scale, h, s0, s1, b0, b1);
        float v = tmp[(long)s0 * W + x] * b0 + tmp[(long)s1 * W + x] * b1;
        v = v < 0.f ? 0.f : v;
        heat[i] = v;
        mn = fminf(mn, v); mx = fmaxf(mx, v);
    }
    cam_block_minmax(mn, mx, red);
    const float hmin = mn, hden = 1e-7f + (mx - mn);

    // 4. scaled heatmap; max of the blend
    const float* x_img = image + (long)n * 3 * HWo;
    float omax = -INFINITY, unused = INFINITY;
    for (long i = tid; i < HWo; i += CAM_RENDER_THREADS) {
        const float v = __fdiv_rn(heat[i] - hmin, hden);
        heat[i] = v;
        if (overlay_out)
            for (int c = 0; c < 3; ++c) omax = fmaxf(omax, cam_overlay(v, c, x_img[c * HWo + i], mean_std, lut, wl, wi));
    }
    if (!overlay_out) return;                      // uniform across the launch
    cam_block_minmax(unused, omax, red);

    // 5. overlay = uint8(255 * (o / max(o)))
    unsigned char* o8 = overlay_out + (long)n * HWo * 3;
    for (long i = tid; i < HWo; i += CAM_RENDER_THREADS) {
        const float v = heat[i];
        for (int c = 0; c < 3; ++c) {
            const float o = cam_overlay(v, c, x_img[c * HWo + i], mean_std, lut, wl, wi);
            const float q = 255.f * __fdiv_rn(o, omax);
            o8[i * 3 + c] = (unsigned char)(q < 0.f ? 0.f : (q > 255.f ? 255.f : q));
        }
    }
}

extern "C" int dfd_gradcam_map(const void* act, const void* grad, int dtype, int N, int HW, int C, float* cam_out,
                               dfd_stream stream) {
    if (!act || !grad || !cam_out || N < 1 || HW < 1 || C < 1 || C > CAM_MAX_C || (dtype != DFD_F32 && dtype != DFD_BF16))
        return DFD_EINVAL;
    const size_t lds = (size_t)C * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == DFD_F32) {
        dfd_allow_lds_once<k_gradcam_map<float>>((int)(CAM_MAX_C * sizeof(float)));
        hipLaunchKernelGGL(k_gradcam_map<float>, dim3(N), dim3(CAM_MAP_THREADS), lds, s, (const float*)act, (const float*)grad,
                           HW, C, cam_out);
    } else {
        dfd_allow_lds_once<k_gradcam_map<bf16>>((int)(CAM_MAX_C * sizeof(float)));
        hipLaunchKernelGGL(k_gradcam_map<bf16>, dim3(N), dim3(CAM_MAP_THREADS), lds, s, (const bf16*)act, (const bf16*)grad,
                           HW, C, cam_out);
    }
    return hipGetLastError() == hipSuccess ? DFD_OK : DFD_ELAUNCH;
}

extern "C" size_t dfd_cam_render_ws(int N, int h, int w, int H, int W) {
    (void)w; (void)H;
    if (N < 1 || h < 1 || W < 1) return 0;
    return (size_t)N * h * W * sizeof(float);
}

extern "C" int dfd_cam_render(const float* cam, int N, int h, int w, int H, int W, const float* image, const float* mean_std,
                              const unsigned char* lut, double image_weight, float* heat_out, unsigned char* overlay_out,
                              void* workspace, size_t ws_bytes, dfd_stream stream) {
    if (!cam || !heat_out || N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return DFD_EINVAL;
    if ((long)H * W > (1L << 26) || (long)h * w > (1L << 26)) return DFD_EINVAL;
    if (overlay_out && (!image || !mean_std || !lut || !(image_weight >= 0.0 && image_weight <= 1.0))) return DFD_EINVAL;
    if (!workspace || ws_bytes < dfd_cam_render_ws(N, h, w, H, W)) return DFD_EWORKSPACE;
    // cv2: inv_scale = dsize / ssize, scale = 1 / inv_scale (double); the blend weights as numpy forms them from Python floats
    const double sx_scale = 1.0 / ((double)W / (double)w), sy_scale = 1.0 / ((double)H / (double)h);
    const float wl = (float)(1.0 - image_weight), wi = (float)image_weight;
    hipLaunchKernelGGL(k_cam_render, dim3(N), dim3(CAM_RENDER_THREADS), 0, (hipStream_t)stream, cam, h, w, H, W, sx_scale, sy_scale,
                       image, mean_std, lut, wl, wi, heat_out, overlay_out, (float*)workspace);
    return hipGetLastError() == hipSuccess ? DFD_OK : DFD_ELAUNCH;
}
