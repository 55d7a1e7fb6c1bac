// Input preprocessing on the GPU: the step before Model.forward in the reference's demo (demo.py:27-51 open_image =
// PIL ImageOps.contain (bicubic, aspect-preserving) + ImageOps.pad (centre, black) + utils/image.py:12-24 normalize_rgb).
//
// The resample is Pillow's 8-bit two-pass separable convolution restated exactly: horizontal pass to uint8, vertical pass
// to uint8, both in fixed point (coefficients pre-quantised to 22 fractional bits by the host, accumulator seeded with
// 1 << 21, arithmetic shift, clip to 0..255), so the result is bit-identical to PIL's; the ImageNet normalisation is a
// 3 x 256 lookup table the host fills with the reference's own numpy expression (float32 divide, float64 mean/std, cast).
// Byte/integer streaming work: HBM-bound, one thread per output pixel, no LDS needed (taps overlap in L1/L2).
// mhmr_preprocess_u8_batch runs the same per-pixel bodies for B images of different sizes in two launches over (block, image).
// mhmr_preprocess_u8_batch_oriented reads each source through a rotation / mirror (the training loader's closeup rotation and random
// flip) instead of from an oriented copy: same arithmetic, another source address.  A mirrored row is a row read backwards; a rotated
// image's row is a source COLUMN, so there the horizontal pass puts adjacent lanes on adjacent oriented rows (adjacent source bytes)
// and turns the 64 x 64 tile of results through LDS, so that the writes of tmp are row segments too.
#include "mhmr_common.h"
#include "mhmr_internal.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// tmp[y][ox][c] = clip8(sum_t img[y0 + y][xmin(ox) + t][c] * kh[ox][t])      (rows y0 .. y0 + rows - 1 of the source only)
// One body for the one-image and the batch kernel: i = the thread's pixel of tmp, i < rows * ow checked by the caller.
__device__ __forceinline__ void resample_h_pixel(const uint8_t* __restrict__ img, int W, int y0, const int* __restrict__ kh,
                                                 const int* __restrict__ bh, int ksh, int ow, uint8_t* __restrict__ tmp, int i) {
    const int y = i / ow, ox = i - y * ow;
    const int xmin = bh[2 * ox], xmax = bh[2 * ox + 1];
    const int* k = kh + (size_t)ox * ksh;
    const uint8_t* p = img + ((size_t)(y0 + y) * W + xmin) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < xmax; ++t) {
        const int kk = k[t];
        s0 += p[3 * t] * kk;
        s1 += p[3 * t + 1] * kk;
        s2 += p[3 * t + 2] * kk;
    }
    uint8_t* o = tmp + (size_t)i * 3;
    o[0] = (uint8_t)clip8(s0);
    o[1] = (uint8_t)clip8(s1);
    o[2] = (uint8_t)clip8(s2);
}

// out[c][Y][X] = lut[c][ inside ? clip8(sum_t tmp[ymin(oy) - y0 + t][ox][c] * kv[oy][t]) : 0 ],  (ox, oy) = (X - pad_x, Y - pad_y)
// i = the thread's pixel of one [S][S] plane, i < S * S checked by the caller.
__device__ __forceinline__ void resample_v_norm_pixel(const uint8_t* __restrict__ tmp, int y0, const int* __restrict__ kv,
                                                      const int* __restrict__ bv, int ksv, int ow, int oh, int S, int pad_x, int pad_y,
                                                      const float* __restrict__ lut, float* __restrict__ out, int i) {
    const int Y = i / S, X = i - Y * S;
    const int ox = X - pad_x, oy = Y - pad_y;
    int v0 = 0, v1 = 0, v2 = 0;
    if (ox >= 0 && ox < ow && oy >= 0 && oy < oh) {
        const int ymin = bv[2 * oy], ymax = bv[2 * oy + 1];
        const int* k = kv + (size_t)oy * ksv;
        const uint8_t* p = tmp + ((size_t)(ymin - y0) * ow + ox) * 3;
        int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < ymax; ++t) {
            const int kk = k[t];
            const uint8_t* q = p + (size_t)t * ow * 3;
            s0 += q[0] * kk;
            s1 += q[1] * kk;
            s2 += q[2] * kk;
        }
        v0 = clip8(s0); v1 = clip8(s1); v2 = clip8(s2);
    }
    out[i] = lut[v0];
    out[(size_t)S * S + i] = lut[256 + v1];
    out[(size_t)2 * S * S + i] = lut[512 + v2];
}

__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ img, int W, int y0, int rows,
                                                         const int* __restrict__ kh, const int* __restrict__ bh, int ksh,
                                                         int ow, uint8_t* __restrict__ tmp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * ow) return;
    resample_h_pixel(img, W, y0, kh, bh, ksh, ow, tmp, i);
}

__global__ __launch_bounds__(256) void resample_v_norm_kernel(const uint8_t* __restrict__ tmp, int y0,
                                                              const int* __restrict__ kv, const int* __restrict__ bv, int ksv,
                                                              int ow, int oh, int S, int pad_x, int pad_y,
                                                              const float* __restrict__ lut, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * S) return;
    resample_v_norm_pixel(tmp, y0, kv, bv, ksv, ow, oh, S, pad_x, pad_y, lut, out, i);
}

// The batch forms: blockIdx.y = image, its descriptor read from device memory (uniform over the block); the grid's x extent is
// the largest image's, so the blocks past an image's own pixel count exit.
__global__ __launch_bounds__(256) void resample_h_batch_kernel(const mhmr_pre_image* __restrict__ desc) {
    const mhmr_pre_image& d = desc[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.rows * d.ow) return;
    resample_h_pixel((const uint8_t*)d.img, d.W, d.y0, d.kh, d.bh, d.ksh, d.ow, (uint8_t*)d.tmp, i);
}

template <typename Desc>      // mhmr_pre_image or mhmr_pre_image_o: tmp holds the oriented image's rows either way
__global__ __launch_bounds__(256) void resample_v_norm_batch_kernel(const Desc* __restrict__ desc, int S,
                                                                    const float* __restrict__ lut, float* __restrict__ out) {
    const Desc& d = desc[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S * S) return;
    resample_v_norm_pixel((const uint8_t*)d.tmp, d.y0, d.kv, d.bv, d.ksv, d.ow, d.oh, S, d.pad_x, d.pad_y, lut,
                          out + (size_t)blockIdx.y * 3 * S * S, i);
}

// ---- oriented sources.  The oriented image (what PIL holds after rotate(-90, expand=True) and / or ImageOps.mirror) is
// or[y][x] = src[H - 1 - x'][y] if rotated else src[y][x'],  x' = oW - 1 - x if mirrored else x,  oW = rotated ? H : W
// (H, W: the stored buffer).  One step in oriented x is `step` bytes of the source.
struct OrientedSource {
    const uint8_t* origin;     // or[0][0]
    ptrdiff_t step_x, step_y;  // bytes per oriented column / row
};

__device__ __forceinline__ OrientedSource oriented_source(const uint8_t* img, int H, int W, int orient) {
    const bool mirror = orient & MHMR_ORIENT_MIRROR, rot = orient & MHMR_ORIENT_ROT90;
    OrientedSource o;
    if (rot) {                 // x' walks the source rows upwards, y the source columns
        o.step_x = mirror ? (ptrdiff_t)W * 3 : -(ptrdiff_t)W * 3;
        o.step_y = 3;
        o.origin = img + (mirror ? (size_t)0 : (size_t)(H - 1) * W * 3);
    } else {
        o.step_x = mirror ? -3 : 3;
        o.step_y = (ptrdiff_t)W * 3;
        o.origin = img + (mirror ? (size_t)(W - 1) * 3 : (size_t)0);
    }
    return o;
}

// resample_h_pixel's sum for the pixel (y, ox) of tmp, read through the orientation; the three bytes packed b0 | b1 << 8 | b2 << 16
__device__ __forceinline__ unsigned resample_h_oriented(const OrientedSource& src, int y0, const int* __restrict__ kh,
                                                        const int* __restrict__ bh, int ksh, int y, int ox) {
    const int xmin = bh[2 * ox], xmax = bh[2 * ox + 1];
    const int* k = kh + (size_t)ox * ksh;
    const uint8_t* p = src.origin + (ptrdiff_t)(y0 + y) * src.step_y + (ptrdiff_t)xmin * src.step_x;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < xmax; ++t, p += src.step_x) {
        const int kk = k[t];
        s0 += p[0] * kk;
        s1 += p[1] * kk;
        s2 += p[2] * kk;
    }
    return (unsigned)clip8(s0) | (unsigned)clip8(s1) << 8 | (unsigned)clip8(s2) << 16;
}

__device__ __forceinline__ void store_rgb(uint8_t* o, unsigned v) {
    o[0] = (uint8_t)v;
    o[1] = (uint8_t)(v >> 8);
    o[2] = (uint8_t)(v >> 16);
}

constexpr int OT = 64;         // the rotated form's tile of tmp: OT rows x OT columns per block

// Horizontal pass of the oriented batch.  Unrotated images: one thread per pixel of tmp, lanes along ox, as resample_h_batch_kernel.
// Rotated images: block = one OT x OT tile of tmp; lane = row of the tile (adjacent source bytes), wave w computes columns
// 16 w .. 16 w + 15 (tables and taps uniform over the wave), results cross LDS (row pitch OT + 1 dwords: the 32 lanes of a write group
// hit 32 banks) and leave as rows of tmp.  Blocks past an image's own count exit whole, so every thread of a block reaches the barrier.
__global__ __launch_bounds__(256) void resample_h_batch_oriented_kernel(const mhmr_pre_image_o* __restrict__ desc) {
    __shared__ unsigned tile[OT][OT + 1];
    const mhmr_pre_image_o& d = desc[blockIdx.y];
    const OrientedSource src = oriented_source((const uint8_t*)d.img, d.H, d.W, d.orient);
    uint8_t* tmp = (uint8_t*)d.tmp;
    if (!(d.orient & MHMR_ORIENT_ROT90)) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i >= d.rows * d.ow) return;
        const int y = i / d.ow, ox = i - y * d.ow;
        store_rgb(tmp + (size_t)i * 3, resample_h_oriented(src, d.y0, d.kh, d.bh, d.ksh, y, ox));
        return;
    }
    const int tiles_y = (d.rows + OT - 1) / OT, tiles_x = (d.ow + OT - 1) / OT;
    if ((int)blockIdx.x >= tiles_y * tiles_x) return;
    const int tx0 = (blockIdx.x / tiles_y) * OT, ty0 = (blockIdx.x % tiles_y) * OT;
    const int ly = threadIdx.x & (OT - 1), w = threadIdx.x / OT;
    if (ty0 + ly < d.rows)
        for (int c = w * 16; c < w * 16 + 16 && tx0 + c < d.ow; ++c)
            tile[ly][c] = resample_h_oriented(src, d.y0, d.kh, d.bh, d.ksh, ty0 + ly, tx0 + c);
    __syncthreads();
    for (int j = threadIdx.x; j < OT * OT; j += 256) {
        const int ry = j / OT, rx = j - ry * OT;
        if (ty0 + ry < d.rows && tx0 + rx < d.ow) store_rgb(tmp + ((size_t)(ty0 + ry) * d.ow + tx0 + rx) * 3, tile[ry][rx]);
    }
}

// the shape conditions of one image (shared by the entry points)
bool bad_image_shape(int H, int W, int ow, int oh, int ksh, int ksv, int y0, int rows, int S, int pad_x, int pad_y) {
    if (H <= 0 || W <= 0 || ow <= 0 || oh <= 0 || ow > S || oh > S || ksh <= 0 || ksv <= 0) return true;
    return y0 < 0 || rows <= 0 || y0 + rows > H || pad_x < 0 || pad_y < 0 || pad_x + ow > S || pad_y + oh > S;
}

}  // namespace

extern "C" int mhmr_preprocess_u8(const void* img, int H, int W, const int* kh, const int* bh, int ksh, const int* kv,
                                  const int* bv, int ksv, int ow, int oh, int y0, int rows, int S, int pad_x, int pad_y,
                                  const float* lut, void* tmp, float* out, void* stream) {
    if (bad_image_shape(H, W, ow, oh, ksh, ksv, y0, rows, S, pad_x, pad_y)) return MHMR_ERR_BAD_SHAPE;
    if (!img || !kh || !bh || !kv || !bv || !lut || !tmp || !out) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int n1 = rows * ow, n2 = S * S;
    hipLaunchKernelGGL(resample_h_kernel, dim3((n1 + 255) / 256), dim3(256), 0, s, (const uint8_t*)img, W, y0, rows, kh, bh, ksh, ow,
                       (uint8_t*)tmp);
    hipLaunchKernelGGL(resample_v_norm_kernel, dim3((n2 + 255) / 256), dim3(256), 0, s, (const uint8_t*)tmp, y0, kv, bv, ksv, ow, oh, S,
                       pad_x, pad_y, lut, out);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_preprocess_u8_batch(const mhmr_pre_image* host, const mhmr_pre_image* dev, int B, int S, const float* lut,
                                        float* out, void* stream) {
    if (B <= 0 || B > 65535 || S <= 0) return MHMR_ERR_BAD_SHAPE;
    if (!host || !dev || !lut || !out) return MHMR_ERR_BAD_ARG;
    int n1 = 0;
    for (int b = 0; b < B; ++b) {
        const mhmr_pre_image& d = host[b];
        if (bad_image_shape(d.H, d.W, d.ow, d.oh, d.ksh, d.ksv, d.y0, d.rows, S, d.pad_x, d.pad_y)) return MHMR_ERR_BAD_SHAPE;
        if (!d.img || !d.kh || !d.bh || !d.kv || !d.bv || !d.tmp) return MHMR_ERR_BAD_ARG;
        n1 = d.rows * d.ow > n1 ? d.rows * d.ow : n1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int n2 = S * S;
    hipLaunchKernelGGL(resample_h_batch_kernel, dim3((n1 + 255) / 256, B), dim3(256), 0, s, dev);
    hipLaunchKernelGGL(resample_v_norm_batch_kernel<mhmr_pre_image>, dim3((n2 + 255) / 256, B), dim3(256), 0, s, dev, S, lut, out);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" int mhmr_preprocess_u8_batch_oriented(const mhmr_pre_image_o* host, const mhmr_pre_image_o* dev, int B, int S,
                                                 const float* lut, float* out, void* stream) {
    if (B <= 0 || B > 65535 || S <= 0) return MHMR_ERR_BAD_SHAPE;
    if (!host || !dev || !lut || !out) return MHMR_ERR_BAD_ARG;
    int blocks = 0;
    for (int b = 0; b < B; ++b) {
        const mhmr_pre_image_o& d = host[b];
        if (d.orient & ~(MHMR_ORIENT_MIRROR | MHMR_ORIENT_ROT90)) return MHMR_ERR_BAD_ARG;
        const bool rot = d.orient & MHMR_ORIENT_ROT90;
        // y0, rows and the tables are the oriented image's, H x W the stored buffer's
        if (bad_image_shape(rot ? d.W : d.H, rot ? d.H : d.W, d.ow, d.oh, d.ksh, d.ksv, d.y0, d.rows, S, d.pad_x, d.pad_y)) return MHMR_ERR_BAD_SHAPE;
        if (!d.img || !d.kh || !d.bh || !d.kv || !d.bv || !d.tmp) return MHMR_ERR_BAD_ARG;
        const int n = rot ? ((d.rows + OT - 1) / OT) * ((d.ow + OT - 1) / OT) : (d.rows * d.ow + 255) / 256;
        blocks = n > blocks ? n : blocks;
    }
    hipStream_t s = (hipStream_t)stream;
    const int n2 = S * S;
    hipLaunchKernelGGL(resample_h_batch_oriented_kernel, dim3(blocks, B), dim3(256), 0, s, dev);
    hipLaunchKernelGGL(resample_v_norm_batch_kernel<mhmr_pre_image_o>, dim3((n2 + 255) / 256, B), dim3(256), 0, s, dev, S, lut, out);
    MHMR_CHECK_LAUNCH();
    return 0;
}
