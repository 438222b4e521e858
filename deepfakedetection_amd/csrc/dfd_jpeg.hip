// dfd_jpeg.hip — JPEG-compression augmentation on the device (ABI 142): every selected picture of a uint8 [N][H][W][3] batch is
// replaced by what Image.save(buf, "JPEG", quality=q) followed by Image.open(buf) gives, byte for byte.  A JPEG round trip is pure
// integer arithmetic once the lossless entropy coding is left out, so this file restates libjpeg's defaults as Pillow uses them, in
// signed 32-bit integers with arithmetic shifts (tests/_jpeg_ref.py is the same in numpy, pinned against Pillow itself):
//   colour in   jccolor's 16.16 fixed-point RGB -> YCbCr;
//   sampling    4:2:0: Y padded to multiples of 8 by edge replication; chroma: the input's columns and rows replicated, the 2x2 box
//               (a + b + c + d + bias) >> 2 with bias 1 on even and 2 on odd output columns, then the last DOWNSAMPLED row replicated;
//   tables      Annex K, scaled by the quality and clamped to 1..255 (baseline);
//   transform   jfdctint (rows, then columns; 8 times the DCT), the quantiser's rounded division of the magnitude, the dequantiser,
//               jidctint (columns, then rows), + 128, clamped;
//   chroma up   the "fancy" h2v2 triangle filter over the real ceil(H/2) x ceil(W/2) samples;
//   colour out  jdcolor's 16.16 fixed-point YCbCr -> RGB, clamped.
// Two launches.  k_jpeg_code: one 192-thread workgroup per (picture, row of MCUs, strip of 4 MCUs): 16 x 64 pixels = 16 Y + 4 Cb +
// 4 Cr blocks, 8 lanes per block (one per row, then one per column; the column lane runs forward DCT, quantiser, dequantiser and
// inverse DCT of its column in registers, since jfdctint ends with the columns and jidctint starts with them).  It writes the
// reconstructed planes as bytes into the workspace.  k_jpeg_finish: one thread per output pixel, upsampling and colour conversion.
// A job's quality 0 copies the picture through (mirrored if its flip flag says so) and costs the first launch nothing.
#include "dfd_common.h"

#define JPEG_THREADS 192
#define JPEG_BLOCKS 24                              // 16 Y + 4 Cb + 4 Cr
#define JPEG_ROW 9                                  // ints per block row in LDS: 8 + 1, so that a column pass does not sit on one bank
#define JPEG_BLK (8 * JPEG_ROW + 1)
#define JPEG_FIN_THREADS 256

#define JF_0298 2446
#define JF_0390 3196
#define JF_0541 4433
#define JF_0765 6270
#define JF_0899 7373
#define JF_1175 9633
#define JF_1501 12299
#define JF_1847 15137
#define JF_1961 16069
#define JF_2053 16819
#define JF_2562 20995
#define JF_3072 25172
#define JPEG_CONST_BITS 13
#define JPEG_PASS1_BITS 2

__constant__ unsigned char jpeg_base[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

__device__ __forceinline__ int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int jpeg_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// FIX(x) = (int)(x * 65536 + 0.5)
__device__ __forceinline__ int jpeg_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int jpeg_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int jpeg_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// jfdctint's one-dimensional pass over d[0..7]; FIRST: the row pass (results scaled up by PASS1_BITS).
template <bool FIRST>
__device__ __forceinline__ void jpeg_fdct8(int* d) {
    const int n = FIRST ? JPEG_CONST_BITS - JPEG_PASS1_BITS : JPEG_CONST_BITS + JPEG_PASS1_BITS;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { d[0] = (t10 + t11) << JPEG_PASS1_BITS; d[4] = (t10 - t11) << JPEG_PASS1_BITS; }
    else { d[0] = jpeg_descale(t10 + t11, JPEG_PASS1_BITS); d[4] = jpeg_descale(t10 - t11, JPEG_PASS1_BITS); }
    int z1 = (t12 + t13) * JF_0541;
    d[2] = jpeg_descale(z1 + t13 * JF_0765, n);
    d[6] = jpeg_descale(z1 + t12 * (-JF_1847), n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * JF_1175;
    t4 *= JF_0298; t5 *= JF_2053; t6 *= JF_3072; t7 *= JF_1501;
    z1 *= -JF_0899; z2 *= -JF_2562; z3 = z3 * (-JF_1961) + z5; z4 = z4 * (-JF_0390) + z5;
    d[7] = jpeg_descale(t4 + z1 + z3, n);
    d[5] = jpeg_descale(t5 + z2 + z4, n);
    d[3] = jpeg_descale(t6 + z2 + z3, n);
    d[1] = jpeg_descale(t7 + z1 + z4, n);
}

// jidctint's one-dimensional pass over d[0..7], descaled by n bits.
__device__ __forceinline__ void jpeg_idct8(int* d, int n) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * JF_0541;
    int t2 = z1 + z3 * (-JF_1847), t3 = z1 + z2 * JF_0765;
    int t0 = (d[0] + d[4]) << JPEG_CONST_BITS, t1 = (d[0] - d[4]) << JPEG_CONST_BITS;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7]; t1 = d[5]; t2 = d[3]; t3 = d[1];
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * JF_1175;
    t0 *= JF_0298; t1 *= JF_2053; t2 *= JF_3072; t3 *= JF_1501;
    z1 *= -JF_0899; z2 *= -JF_2562; z3 = z3 * (-JF_1961) + z5; z4 = z4 * (-JF_0390) + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    d[0] = jpeg_descale(t10 + t3, n); d[7] = jpeg_descale(t10 - t3, n);
    d[1] = jpeg_descale(t11 + t2, n); d[6] = jpeg_descale(t11 - t2, n);
    d[2] = jpeg_descale(t12 + t1, n); d[5] = jpeg_descale(t12 - t1, n);
    d[3] = jpeg_descale(t13 + t0, n); d[4] = jpeg_descale(t13 - t0, n);
}

// Workspace of one picture: Y [H][W], Cb [ch][cw], Cr [ch][cw] bytes, ch = ceil(H/2), cw = ceil(W/2).
__device__ __host__ __forceinline__ long jpeg_picture_ws(int H, int W) { return (long)H * W + 2L * ((H + 1) / 2) * ((W + 1) / 2); }

__global__ void __launch_bounds__(JPEG_THREADS)
k_jpeg_code(const unsigned char* __restrict__ src, const int* __restrict__ jobs, unsigned char* __restrict__ ws, int H, int W,
            int strips, int mrows) {
    __shared__ int blk[JPEG_BLOCKS * JPEG_BLK];
    __shared__ int qt[2][64];
    const int t = threadIdx.x;
    unsigned int bid = blockIdx.x;
    const int strip = (int)(bid % (unsigned)strips); bid /= (unsigned)strips;
    const int mrow = (int)(bid % (unsigned)mrows);
    const int n = (int)(bid / (unsigned)mrows);
    int quality = jobs[2 * n];
    if (quality <= 0) return;                                   // copied through by k_jpeg_finish (the same for the whole workgroup)
    quality = min(quality, 100);
    const bool flip = jobs[2 * n + 1] != 0;
    const int x0 = strip * 64, y0 = mrow * 16;
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const unsigned char* in = src + (long)n * H * W * 3;

    if (t < 128) {
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        qt[t >> 6][t & 63] = min(max(((int)jpeg_base[t >> 6][t & 63] * scale + 50) / 100, 1), 255);
    }
    // ---- Y - 128 of the 16 x 64 pixels, rows and columns beyond the picture replicated from its edge
    for (int i = t; i < 16 * 64; i += JPEG_THREADS) {
        const int ly = i >> 6, lx = i & 63;
        const int gy = min(y0 + ly, H - 1), gx = min(x0 + lx, W - 1);
        const unsigned char* p = in + ((long)gy * W + (flip ? W - 1 - gx : gx)) * 3;
        blk[((ly >> 3) * 8 + (lx >> 3)) * JPEG_BLK + (ly & 7) * JPEG_ROW + (lx & 7)] = jpeg_y(p[0], p[1], p[2]) - 128;
    }
    // ---- Cb, Cr - 128 of the 8 x 32 downsampled samples: rows beyond the last real downsampled row repeat IT (not the input's last row)
    for (int i = t; i < 8 * 32; i += JPEG_THREADS) {
        const int ly = i >> 5, lx = i & 31;
        const int cy = min((y0 >> 1) + ly, ch - 1), cx = (x0 >> 1) + lx;
        const int r0 = 2 * cy, r1 = min(2 * cy + 1, H - 1), c0 = min(2 * cx, W - 1), c1 = min(2 * cx + 1, W - 1);
        const int a0 = flip ? W - 1 - c0 : c0, a1 = flip ? W - 1 - c1 : c1;
        const unsigned char* p00 = in + ((long)r0 * W + a0) * 3;
        const unsigned char* p01 = in + ((long)r0 * W + a1) * 3;
        const unsigned char* p10 = in + ((long)r1 * W + a0) * 3;
        const unsigned char* p11 = in + ((long)r1 * W + a1) * 3;
        const int bias = (lx & 1) ? 2 : 1;                                   // x0 / 2 is even: the parity of lx is that of cx
        const int cb = jpeg_cb(p00[0], p00[1], p00[2]) + jpeg_cb(p01[0], p01[1], p01[2]) + jpeg_cb(p10[0], p10[1], p10[2]) +
                       jpeg_cb(p11[0], p11[1], p11[2]);
        const int cr = jpeg_cr(p00[0], p00[1], p00[2]) + jpeg_cr(p01[0], p01[1], p01[2]) + jpeg_cr(p10[0], p10[1], p10[2]) +
                       jpeg_cr(p11[0], p11[1], p11[2]);
        const int at = (lx >> 3) * JPEG_BLK + ly * JPEG_ROW + (lx & 7);
        blk[16 * JPEG_BLK + at] = ((cb + bias) >> 2) - 128;
        blk[20 * JPEG_BLK + at] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    int* mine = blk + (t >> 3) * JPEG_BLK;                      // 8 lanes per block
    const int lane = t & 7;
    const int* table = qt[(t >> 3) < 16 ? 0 : 1];
    int d[8];
    // ---- forward DCT, rows
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = mine[lane * JPEG_ROW + k];
    jpeg_fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[lane * JPEG_ROW + k] = d[k];
    __syncthreads();
    // ---- forward DCT, columns; quantise; dequantise; inverse DCT, columns
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = mine[k * JPEG_ROW + lane];
    jpeg_fdct8<false>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int q = table[k * 8 + lane];
        const unsigned int div = (unsigned)q << 3, mag = (unsigned)(d[k] < 0 ? -d[k] : d[k]);
        const int level = (int)((mag + (div >> 1)) / div);                  // exact: an integer division of the magnitude
        d[k] = (d[k] < 0 ? -level : level) * q;
    }
    jpeg_idct8(d, JPEG_CONST_BITS - JPEG_PASS1_BITS);
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[k * JPEG_ROW + lane] = d[k];
    __syncthreads();
    // ---- inverse DCT, rows
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = mine[lane * JPEG_ROW + k];
    jpeg_idct8(d, JPEG_CONST_BITS + JPEG_PASS1_BITS + 3);
#pragma unroll
    for (int k = 0; k < 8; ++k) mine[lane * JPEG_ROW + k] = jpeg_clip8(d[k] + 128);
    __syncthreads();
    // ---- the part of the three planes that lies inside the picture
    unsigned char* wy = ws + (long)n * jpeg_picture_ws(H, W);
    unsigned char* wcb = wy + (long)H * W;
    unsigned char* wcr = wcb + (long)ch * cw;
    for (int i = t; i < 16 * 64; i += JPEG_THREADS) {
        const int ly = i >> 6, lx = i & 63, gy = y0 + ly, gx = x0 + lx;
        if (gy < H && gx < W)
            wy[(long)gy * W + gx] = (unsigned char)blk[((ly >> 3) * 8 + (lx >> 3)) * JPEG_BLK + (ly & 7) * JPEG_ROW + (lx & 7)];
    }
    for (int i = t; i < 8 * 32; i += JPEG_THREADS) {
        const int ly = i >> 5, lx = i & 31, cy = (y0 >> 1) + ly, cx = (x0 >> 1) + lx;
        if (cy < ch && cx < cw) {
            const int at = (lx >> 3) * JPEG_BLK + ly * JPEG_ROW + (lx & 7);
            wcb[(long)cy * cw + cx] = (unsigned char)blk[16 * JPEG_BLK + at];
            wcr[(long)cy * cw + cx] = (unsigned char)blk[20 * JPEG_BLK + at];
        }
    }
}

// One thread per output pixel, a workgroup per 64 x 4 tile.
__global__ void __launch_bounds__(JPEG_FIN_THREADS)
k_jpeg_finish(const unsigned char* __restrict__ src, const int* __restrict__ jobs, const unsigned char* __restrict__ ws,
              unsigned char* __restrict__ out, int H, int W, int tiles_x, int tiles_y) {
    unsigned int bid = blockIdx.x;
    const int tx = (int)(bid % (unsigned)tiles_x); bid /= (unsigned)tiles_x;
    const int ty = (int)(bid % (unsigned)tiles_y);
    const int n = (int)(bid / (unsigned)tiles_y);
    const int x = tx * 64 + (threadIdx.x & 63), y = ty * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int quality = jobs[2 * n];
    unsigned char* o = out + (((long)n * H + y) * W + x) * 3;
    if (quality <= 0) {
        const int sx = jobs[2 * n + 1] != 0 ? W - 1 - x : x;
        const unsigned char* p = src + (((long)n * H + y) * W + sx) * 3;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        return;
    }
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1;
    const unsigned char* wy = ws + (long)n * jpeg_picture_ws(H, W);
    const unsigned char* wc = wy + (long)H * W;
    const int cy = y >> 1, cx = x >> 1;
    const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);          // the far row, clamped to the real rows
    const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);          // the neighbouring column: itself at either end
    const int round = (x & 1) ? 7 : 8;
    int c[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const unsigned char* pl = wc + (long)k * ch * cw;
        const int s0 = 3 * (int)pl[(long)cy * cw + cx] + (int)pl[(long)fy * cw + cx];
        const int s1 = 3 * (int)pl[(long)cy * cw + nx] + (int)pl[(long)fy * cw + nx];
        c[k] = ((3 * s0 + s1 + round) >> 4) - 128;
    }
    const int yy = wy[(long)y * W + x], cb = c[0], cr = c[1];
    o[0] = (unsigned char)jpeg_clip8(yy + ((91881 * cr + 32768) >> 16));
    o[1] = (unsigned char)jpeg_clip8(yy + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    o[2] = (unsigned char)jpeg_clip8(yy + ((116130 * cb + 32768) >> 16));
}

extern "C" size_t dfd_jpeg_ws(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return (size_t)N * (size_t)jpeg_picture_ws(H, W);
}

extern "C" int dfd_jpeg_u8(const unsigned char* src, const int* jobs_dev, void* ws, unsigned char* out, int N, int H, int W,
                           dfd_stream stream) {
    if (!src || !jobs_dev || !ws || !out || N < 1 || H < 1 || W < 5 || src == out) return DFD_EINVAL;
    const long strips = (W + 63) / 64, mrows = (H + 15) / 16, tiles_x = (W + 63) / 64, tiles_y = (H + 3) / 4;
    if (strips * mrows * N > 0x7fffffffL || tiles_x * tiles_y * N > 0x7fffffffL) return DFD_EUNSUPPORTED;      // one grid dimension
    hipLaunchKernelGGL(k_jpeg_code, dim3((unsigned)(strips * mrows * N)), dim3(JPEG_THREADS), 0, (hipStream_t)stream, src, jobs_dev,
                       (unsigned char*)ws, H, W, (int)strips, (int)mrows);
    if (hipGetLastError() != hipSuccess) return DFD_ELAUNCH;
    hipLaunchKernelGGL(k_jpeg_finish, dim3((unsigned)(tiles_x * tiles_y * N)), dim3(JPEG_FIN_THREADS), 0, (hipStream_t)stream, src,
                       jobs_dev, (const unsigned char*)ws, out, H, W, (int)tiles_x, (int)tiles_y);
    return DFD_CHECK_LAUNCH();
}
