// dfd_blur.hip — Gaussian-blur augmentation on the device (ABI 144): every selected picture of a uint8 [N][H][W][3] batch is
// replaced by what Image.filter(ImageFilter.GaussianBlur(radius=sigma)) gives, byte for byte.  Pillow approximates the Gaussian by
// three extended box blurs along x and then three along y, each rounded to a byte; once the box radius is known (data.blur_plan,
// the only floating point) a pass is unsigned 32-bit integer arithmetic with replicated edges:
//   out[x] = (ww * sum_{|d| <= r} in[x + d] + fw * (in[x - r - 1] + in[x + r + 1]) + 2^23) >> 24,
// where (2r + 1) * ww + 2 * fw <= 2^24, so the sum stays below 2^32 and the direct evaluation of the 2r + 3 taps equals Pillow's
// running sum (tests/_blur_ref.py is the same in numpy, pinned against Pillow itself).
// One launch, one workgroup per (picture, channel): the channel's H x W plane is gathered into LDS, the six passes ping-pong between
// two planes there (2 x 228 x 228 = 104 KB of the CU's 160 KB), and the last pass writes the interleaved output.  Lanes run along
// the pixel index in both directions: along x a wave reads consecutive bytes, along y consecutive bytes of one row per tap, so
// neither direction meets a bank twice.  A job that is not selected (ww == 0) or whose radius is outside 0..DFD_BLUR_MAX_RADIUS
// copies its channel from src to out and touches no LDS.
#include "dfd_common.h"

#define BLUR_THREADS 1024
#define BLUR_PLANE(npx) (((npx) + 15) / 16 * 16)

// one box pass over the plane: pixel i = (y, x) sums along x (ALONG_Y false) or along y
template <bool ALONG_Y>
static __device__ __forceinline__ unsigned blur_tap_sum(const unsigned char* __restrict__ in, int y, int x, int H, int W, int r,
                                                        unsigned ww, unsigned fw) {
    const int pos = ALONG_Y ? y : x, len = ALONG_Y ? H : W, stride = ALONG_Y ? W : 1;
    const unsigned char* line = in + (ALONG_Y ? x : y * W);
    unsigned acc = 0;
    for (int d = -r; d <= r; ++d) acc += line[min(max(pos + d, 0), len - 1) * stride];
    const unsigned edge = (unsigned)line[max(pos - r - 1, 0) * stride] + (unsigned)line[min(pos + r + 1, len - 1) * stride];
    return (ww * acc + fw * edge + (1u << 23)) >> 24;
}

template <bool ALONG_Y>
static __device__ __forceinline__ void blur_pass(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int H, int W,
                                                 int r, unsigned ww, unsigned fw) {
    const int npx = H * W;
    for (int i = threadIdx.x; i < npx; i += BLUR_THREADS) {
        const int y = i / W, x = i - y * W;
        out[i] = (unsigned char)blur_tap_sum<ALONG_Y>(in, y, x, H, W, r, ww, fw);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(BLUR_THREADS)
k_blur_u8(const unsigned char* __restrict__ src, const int* __restrict__ jobs, unsigned char* __restrict__ dst, int H, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char planes[];
    const int n = blockIdx.x / 3, c = blockIdx.x - n * 3, t = threadIdx.x;
    const int npx = H * W;
    const int r = jobs[n * 4];
    const unsigned ww = (unsigned)jobs[n * 4 + 1], fw = (unsigned)jobs[n * 4 + 2];
    const unsigned char* in = src + (long)n * npx * 3 + c;
    unsigned char* out = dst + (long)n * npx * 3 + c;
    if (ww == 0 || r < 0 || r > DFD_BLUR_MAX_RADIUS) {                     // uniform over the workgroup
        for (int i = t; i < npx; i += BLUR_THREADS) out[i * 3] = in[i * 3];
        return;
    }
    unsigned char* a = planes;
    unsigned char* b = planes + BLUR_PLANE(npx);
    for (int i = t; i < npx; i += BLUR_THREADS) a[i] = in[i * 3];
    __syncthreads();
    blur_pass<false>(a, b, H, W, r, ww, fw);
    blur_pass<false>(b, a, H, W, r, ww, fw);
    blur_pass<false>(a, b, H, W, r, ww, fw);
    blur_pass<true>(b, a, H, W, r, ww, fw);
    blur_pass<true>(a, b, H, W, r, ww, fw);
    for (int i = t; i < npx; i += BLUR_THREADS) {
        const int y = i / W, x = i - y * W;
        out[i * 3] = (unsigned char)blur_tap_sum<true>(b, y, x, H, W, r, ww, fw);
    }
}

extern "C" int dfd_blur_u8(const unsigned char* src, const int* jobs_dev, unsigned char* out, int N, int H, int W, dfd_stream stream) {
    if (!src || !jobs_dev || !out || N < 1 || H < 1 || W < 1 || src == out) return DFD_EINVAL;
    if ((long)H * W > DFD_BLUR_MAX_PIXELS || (long)N * 3 > 0x7fffffffL) return DFD_EINVAL;   // two planes of one channel must fit one CU's LDS
    dfd_allow_lds_once<k_blur_u8>(2 * DFD_BLUR_MAX_PIXELS);
    hipLaunchKernelGGL(k_blur_u8, dim3(N * 3), dim3(BLUR_THREADS), (size_t)(2 * BLUR_PLANE(H * W)), (hipStream_t)stream, src, jobs_dev,
                       out, H, W);
    return DFD_CHECK_LAUNCH();
}
