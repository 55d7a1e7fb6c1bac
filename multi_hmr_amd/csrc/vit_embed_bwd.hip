// Backward of the token embedding: the derivative of the fp32 function
//     tokens[b] = [ patchify(x[b]) W^T + bias + pos_G[1:],  cls + pos_G[0] ],    pos_G = interpolate(pos_embed)
// with respect to W (the patch convolution, flattened [C, 588], k = ch * 196 + py * 14 + px), bias, cls and pos_embed, taken at the fp32
// master parameters and the fp32 image, against g_stream [B * Tp, C], the cotangent of the residual stream entering block 0 (what
// mhmr_vit_tail_backward leaves when it runs every block).  The forward's 16-bit roundings of the image patches and of W are
// straight-through.  Token rows follow the forward: image b owns rows b * Tp ..., the N = G * G patch rows first (n = gy * G + gx), the
// class row at b * Tp + N; rows behind it are never read.
//
// Rules (DESIGN.md sections 17-22): sums that cross rows are fp64 or fp32 MFMA chains (v_mfma_f32_16x16x4_f32) of a shape fixed by the
// sizes alone; no floating-point atomics, no LDS, no scratch; every element of every output is written; two calls give the same bits.
//   g_patch_w   linear_bwd_weight_kernel's shape (hph_bwd.hip): one wave = 16 channels x 32 k, four waves along k, the B * N patch rows
//               in index order as a BlockedSum2 chain (256 / 4096); the X operand is gathered from the image, no im2col is stored
//   g_patch_b   fp64 column sums over the patch rows (row_sums.h's two fixed stages)
//   g_cls       fp64 sum of the class rows in image order; g_pos[0] is the same number
//   g_pos[1:]   interp^T (sum_b g_patch) interp per channel in fp64: over the images, then along x, then along y, each sum in index
//               order, rounded to fp32 once.  interp [G, M] is packing.pos_embed_matrix: the identity for G == M.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "hph_shared.h"
#include "row_sums.h"

namespace {

constexpr int PATCH_PX = 14;                               // the patch edge
constexpr int PATCH_K = 3 * PATCH_PX * PATCH_PX;           // 588 = a row of the flattened convolution weight
constexpr int PB_SLICE = 32;                               // rows per first-stage slice of the bias column sums
constexpr int EMBED_MAX_GRID = 1024, EMBED_MAX_TABLE = 4096;      // G and M: every element count below stays far inside 64 bits
constexpr long long EMBED_MAX_ROWS = 16LL * 65535;         // B * Tp, the block backward's own limit (vit_bwd.hip block_shape_rc)

// dW[n][k] = sum over the patch rows m = (b, gy, gx) of g_stream[b Tp + gy G + gx][n] * x[b][ch][14 gy + py][14 gx + px].
// Lane group g takes row m + g of every four: its (b, gy, gx) advances by four rows per step, digit by digit, so the loop holds no
// division.  A row past the last one (b == B) contributes an exact zero; its addresses are those of the last row.
__global__ __launch_bounds__(256) void patch_weight_bwd_kernel(const float* __restrict__ gs, const float* __restrict__ x, float* __restrict__ dW,
                                                               int B, int S, int G, int Tp, int C) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int n0 = blockIdx.y * 16, k0 = blockIdx.x * 128 + w * 32;
    if (k0 >= PATCH_K) return;
    const int na = n0 + l15;                                                  // C % 16 == 0: no clamp
    const int kc0 = min(k0 + l15, PATCH_K - 1), kc1 = min(k0 + 16 + l15, PATCH_K - 1);
    const size_t plane = (size_t)S * S;
    auto patch_offset = [&](int k) {                                          // of element k inside a patch, from the patch's first pixel
        const int ch = k / (PATCH_PX * PATCH_PX), r = k - ch * (PATCH_PX * PATCH_PX), py = r / PATCH_PX;
        return (size_t)ch * plane + (size_t)py * S + (size_t)(r - py * PATCH_PX);
    };
    const size_t o0 = patch_offset(kc0), o1 = patch_offset(kc1);
    const int M = B * G * G;
    int b = 0, gy = 0, gx = g;
    auto carry = [&]() {
        while (gx >= G) { gx -= G; ++gy; }
        while (gy >= G) { gy -= G; ++b; }
    };
    carry();
    BlockedSum2 sum;
    for (int m2 = 0; m2 < M; m2 += BLOCKED_SUM_L1 * BLOCKED_SUM_L2) {
        const int m2end = min(M, m2 + BLOCKED_SUM_L1 * BLOCKED_SUM_L2);
        for (int m1 = m2; m1 < m2end; m1 += BLOCKED_SUM_L1) {
            const int m1end = min(M, m1 + BLOCKED_SUM_L1);
#pragma unroll 4
            for (int m = m1; m < m1end; m += 4) {
                const bool live = b < B;
                const int bc = live ? b : B - 1, yc = live ? gy : G - 1, xc = live ? gx : G - 1;
                float a = gs[((size_t)bc * Tp + (size_t)(yc * G + xc)) * C + na];
                if (!live) a = 0.f;
                const float* xp = x + ((size_t)bc * 3 * S + (size_t)yc * PATCH_PX) * S + (size_t)xc * PATCH_PX;
                sum.acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xp[o0], sum.acc0, 0, 0, 0);
                sum.acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xp[o1], sum.acc1, 0, 0, 0);
                gx += 4;
                carry();
            }
            sum.flush1();
        }
        sum.flush2();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k = k0 + 16 * t + l15;
        if (k >= PATCH_K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) dW[(size_t)(n0 + 4 * g + r) * PATCH_K + k] = t == 0 ? sum.top0[r] : sum.top1[r];
    }
}

// the term of the bias column sums: patch row r = (b, n) of the stream cotangent; the second sum is not used
struct PatchRowTerm {
    const float* gs; int N, Tp, C;
    __device__ __forceinline__ double operator()(int r, int, int c, double (&ta)[1], double (&tb)[1]) const {
        const int b = r / N, n = r - b * N;
        ta[0] = (double)gs[((size_t)b * Tp + n) * C + c];
        tb[0] = 0.0;
        return 0.0;
    }
};

// g_cls[c] = g_pos[0][c] = sum_b g_stream[b Tp + N][c], fp64, images in index order; one thread per channel
__global__ __launch_bounds__(64) void cls_sum_kernel(const float* __restrict__ gs, float* __restrict__ g_cls, float* __restrict__ g_pos0, int B,
                                                     int N, int Tp, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)gs[((size_t)b * Tp + N) * C + c];
    g_cls[c] = g_pos0[c] = (float)s;
}

// sum[n][c] = sum_b g_stream[b Tp + n][c] for the patch rows n < N, fp64, images in index order
__global__ __launch_bounds__(256) void image_sum_kernel(const float* __restrict__ gs, double* __restrict__ sum, int B, int N, int Tp, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * C) return;
    const size_t n = i / C, c = i - n * C;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)gs[((size_t)b * Tp + n) * C + c];
    sum[i] = s;
}

// tmp[y][q][c] = sum_x interp[x][q] sum[y G + x][c]: the adjoint of the resampling along x, x in index order
__global__ __launch_bounds__(256) void pos_adjoint_x_kernel(const double* __restrict__ sum, const double* __restrict__ interp,
                                                            double* __restrict__ tmp, int G, int M, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)G * M * C) return;
    const size_t c = i % C, yq = i / C, y = yq / M, q = yq - y * M;
    double s = 0.0;
    for (int xx = 0; xx < G; ++xx) s += interp[(size_t)xx * M + q] * sum[(y * G + xx) * C + c];
    tmp[i] = s;
}

// g_pos[1 + a M + q][c] = sum_y interp[y][a] tmp[y][q][c]: along y, y in index order, then the one rounding to fp32
__global__ __launch_bounds__(256) void pos_adjoint_y_kernel(const double* __restrict__ tmp, const double* __restrict__ interp,
                                                            float* __restrict__ g_pos, int G, int M, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M * M * C) return;
    const size_t c = i % C, aq = i / C, a = aq / M, q = aq - a * M;
    double s = 0.0;
    for (int y = 0; y < G; ++y) s += interp[(size_t)y * M + a] * tmp[((size_t)y * M + q) * C + c];
    g_pos[(size_t)C + i] = (float)s;
}

// MHMR_ERR_BAD_ARG: a negative count; MHMR_ERR_BAD_SHAPE: the channel rules and the launch limits
int embed_shape_rc(int B, int G, int M, int C) {
    if (B < 0 || G < 0 || M < 0 || C < 0) return MHMR_ERR_BAD_ARG;
    if (B == 0 || G == 0 || M < 1 || C == 0 || C % 64 || C > 2048 || G > EMBED_MAX_GRID || M > EMBED_MAX_TABLE) return MHMR_ERR_BAD_SHAPE;
    if ((long long)B * G * G > EMBED_MAX_ROWS) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

// the workspace: the slices of the bias sums, the unused second output of their last stage, the image sums and the half-resampled table
struct EmbedLayout { int nsl; long long part, spare, sum, tmp, total; };
EmbedLayout embed_layout(int B, int G, int M, int C) {
    EmbedLayout L;
    WsCursor ws;
    const long long rows = (long long)B * G * G;
    L.nsl = (int)((rows + PB_SLICE - 1) / PB_SLICE);
    L.part = ws.take((long long)L.nsl * C * 2 * (long long)sizeof(double));
    L.spare = ws.take((long long)C * (long long)sizeof(float));
    L.sum = ws.take((long long)G * G * C * (long long)sizeof(double));
    L.tmp = ws.take((long long)G * M * C * (long long)sizeof(double));
    L.total = ws.at;
    return L;
}

}  // namespace

extern "C" {

long long mhmr_vit_embed_backward_workspace_bytes(int B, int G, int M, int C) {
    TRY(embed_shape_rc(B, G, M, C));
    return embed_layout(B, G, M, C).total;
}

int mhmr_vit_embed_backward(const mhmr_vit_embed_backward_desc* d, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int B = d->B, S = d->S, G = d->G, M = d->M, Tp = d->Tp, C = d->C;
    if (S < 0 || Tp < 0) return MHMR_ERR_BAD_ARG;
    TRY(embed_shape_rc(B, G, M, C));
    if (S != PATCH_PX * G || Tp % 64 || Tp < G * G + 1 || (long long)B * Tp > EMBED_MAX_ROWS) return MHMR_ERR_BAD_SHAPE;
    if (!d->x || !d->g_stream || !d->interp || !d->g_patch_w || !d->g_patch_b || !d->g_cls || !d->g_pos) return MHMR_ERR_BAD_ARG;
    const EmbedLayout L = embed_layout(B, G, M, C);
    if (!d->workspace || !aligned16(d->workspace) || d->workspace_bytes < L.total || (uintptr_t)d->interp % sizeof(double)) return MHMR_ERR_BAD_ARG;

    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    const int N = G * G, rows = B * N;
    double *part = (double*)(ws + L.part), *sum = (double*)(ws + L.sum), *tmp = (double*)(ws + L.tmp);
    float* spare = (float*)(ws + L.spare);
    hipLaunchKernelGGL(patch_weight_bwd_kernel, dim3((PATCH_K + 127) / 128, C / 16), dim3(256), 0, s, d->g_stream, d->x, d->g_patch_w, B, S, G, Tp, C);
    hipLaunchKernelGGL((col_sums1_kernel<PB_SLICE, 1, PatchRowTerm>), dim3(C / 64, L.nsl), dim3(64), 0, s, PatchRowTerm{d->g_stream, N, Tp, C}, part,
                       (double*)nullptr, 0, 0, rows, C);
    hipLaunchKernelGGL(col_sums2_kernel, dim3(C / 64), dim3(64), 0, s, (const double*)part, (const double*)nullptr, (const float*)nullptr,
                       d->g_patch_b, spare, (float*)nullptr, L.nsl, C);
    hipLaunchKernelGGL(cls_sum_kernel, dim3(C / 64), dim3(64), 0, s, d->g_stream, d->g_cls, d->g_pos, B, N, Tp, C);
    hipLaunchKernelGGL(image_sum_kernel, dim3(blocks256((size_t)N * C)), dim3(256), 0, s, d->g_stream, sum, B, N, Tp, C);
    hipLaunchKernelGGL(pos_adjoint_x_kernel, dim3(blocks256((size_t)G * M * C)), dim3(256), 0, s, (const double*)sum, d->interp, tmp, G, M, C);
    hipLaunchKernelGGL(pos_adjoint_y_kernel, dim3(blocks256((size_t)M * M * C)), dim3(256), 0, s, (const double*)tmp, d->interp, d->g_pos, G, M, C);
    MHMR_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
