// Backward of one ViT block: the derivative of the fp32 function
//     x -> x + ls1 * proj(MHSA(norm1(x))),   x -> x + ls2 * fc2(gelu(fc1(norm2(x))))
// with the fp32 master weights, at the block input the inference forward produced.  The block's activations are recomputed from that
// input in fp32 (the tape); none of the forward's 16-bit workspaces is read, so the forward's 16-bit roundings are straight-through.
//
// Rules (DESIGN.md sections 17-22): sums that cross rows are fp64 or fp32 MFMA chains (v_mfma_f32_16x16x4_f32) of a shape fixed by the
// sizes alone; no floating-point atomics; every element of every output is written; results are bit-reproducible call to call.
//
// Attention.  The block calls a tape / backward pair through mhmr_internal.h: the exact-fp32 pair of attention_f32.hip with
// attention_precision = MHMR_ATTN_F32 and in the entries without the argument, the bf16-operand pair of attention_bf16.hip with
// MHMR_ATTN_BF16 of the `_a` entries.  The linears are switched the same way by the descriptor's linear_precision.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "row_sums.h"

namespace {

constexpr int LS_SLICE = 32;                               // rows per first-stage slice of the LayerScale / bias column sums

// ------------------------------------------------------------------------------------------------------------ the block's small kernels
// g0 = g_out with the rows >= T of every image replaced by zeros: the one place where padding rows leave the backward
__global__ __launch_bounds__(256) void mask_rows_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n, int C, int T, int Tp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t row = i / (size_t)C;
    out[i] = (int)(row % (size_t)Tp) < T ? in[i] : 0.f;
}

// mixed-precision mode: dh <- dh * gelu'(z) in fp32, in place, in front of the plain bf16 products (the erf form's
// derivative, the expression of hph_bwd.hip's dact)
__global__ __launch_bounds__(256) void gelu_bwd_inplace_kernel(float* __restrict__ dh, const float* __restrict__ z, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = z[i];
    dh[i] *= 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

__global__ __launch_bounds__(256) void gelu_f32_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gelu_erf(in[i]);
}

// LayerScale + residual of the tape: out = x + ls * y
__global__ __launch_bounds__(256) void layerscale_resid_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ ls, float* __restrict__ out, size_t n, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = x[i] + ls[i % (size_t)C] * y[i];
}

// LayerScale backward, elementwise part: dy = g * ls
__global__ __launch_bounds__(256) void layerscale_bwd_kernel(const float* __restrict__ g, const float* __restrict__ ls, float* __restrict__ dy,
                                                             size_t n, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dy[i] = g[i] * ls[i % (size_t)C];
}

// the two addends of (row, column) of the LayerScale sums (row_sums.h): (g y, g) -> d ls = sum g y, d bias = ls sum g
struct LsTerm {
    const float *g, *y; int C;
    __device__ __forceinline__ double operator()(int r, int, int c, double (&ta)[1], double (&tb)[1]) const {
        const float gv = g[(size_t)r * C + c];
        ta[0] = (double)gv * (double)y[(size_t)r * C + c];
        tb[0] = (double)gv;
        return 0.0;
    }
};

// the stream cotangent behind the final norm: dy[b*Tp + t] = g_feat[b*N + t] for the patch rows t < N, zeros for the class and padding rows
__global__ __launch_bounds__(256) void scatter_patch_rows_kernel(const float* __restrict__ g_feat, float* __restrict__ dy, size_t n, int C, int N,
                                                                 int Tp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t row = i / (size_t)C, b = row / (size_t)Tp;
    const int t = (int)(row - b * (size_t)Tp);
    dy[i] = t < N ? g_feat[(b * (size_t)N + t) * (size_t)C + (i - row * (size_t)C)] : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ shapes and layouts
int block_shape_rc(int B, int T, int Tp, int C, int H) {
    TRY(mhmr_attention_shape_rc(B, T, Tp, C, H));
    if (C > 2048 || ((long long)B * Tp + 15) / 16 > 65535) return MHMR_ERR_BAD_SHAPE;      // LayerNorm kernels; row tiles of the linears
    return 0;
}

// the block's workspace: the tape, the cotangents, the statistics and the scratch of the kernels it calls
struct BlockLayout {
    int nsl;
    long long xn1, qkv, att, y1, x1, xn2, z1, h, y2, g0, dy, dh, dxn, g1, datt, lse, attn, ln, part, lin, attn16, total;
};
// precision MHMR_BWD_BF16 appends the workspace of the widest bf16 linear (fc1: [M, 4C] x [4C, C]), which serves all four
// linears in their three products, one after the other
// attention MHMR_ATTN_BF16 appends, behind that, the workspace of the bf16 attention pair (attention_bf16.hip): the tape's bf16 copy of
// qkv stays there for the backward
BlockLayout block_layout(int B, int Tp, int C, int precision, int attention) {
    BlockLayout L;
    WsCursor ws;
    const long long M = (long long)B * Tp, row = M * C * (long long)sizeof(float);
    L.nsl = (int)((M + LS_SLICE - 1) / LS_SLICE);
    L.xn1 = ws.take(row); L.qkv = ws.take(3 * row); L.att = ws.take(row); L.y1 = ws.take(row); L.x1 = ws.take(row);
    L.xn2 = ws.take(row); L.z1 = ws.take(4 * row); L.h = ws.take(4 * row); L.y2 = ws.take(row);
    L.g0 = ws.take(row); L.dy = ws.take(row); L.dh = ws.take(4 * row);      // dh: cotangent of h, later dqkv (3 C wide)
    L.dxn = ws.take(row); L.g1 = ws.take(row); L.datt = ws.take(row);
    L.lse = ws.take(M * (C / 64) * (long long)sizeof(float));
    L.attn = ws.take(mhmr_attention_f32_bwd_bytes(B, Tp, C));
    L.ln = ws.take(mhmr_layernorm_f32_backward_workspace_bytes((int)M, C));
    L.part = ws.take((long long)L.nsl * C * 2 * (long long)sizeof(double));
    L.lin = ws.at;
    if (precision == MHMR_BWD_BF16) L.lin = ws.take(mhmr_linear_bf16_bytes(M, 4 * C, C));
    L.attn16 = ws.at;
    if (attention == MHMR_ATTN_BF16) L.attn16 = ws.take(mhmr_attention_bf16_bytes(B, Tp, C));
    L.total = ws.at;
    return L;
}
inline bool precision_ok(int p) { return p == MHMR_BWD_F32 || p == MHMR_BWD_BF16; }
inline bool attention_ok(int a) { return a == MHMR_ATTN_F32 || a == MHMR_ATTN_BF16; }

// the tail's workspace: the scattered cotangent of the final norm, the second of the two stream cotangents, LayerNorm scratch, one block
struct TailLayout { long long dy, gy, ln, block, total; };
TailLayout tail_layout(int B, int Tp, int C, int precision, int attention) {
    TailLayout L;
    WsCursor ws;
    const long long M = (long long)B * Tp, row = M * C * (long long)sizeof(float);
    L.dy = ws.take(row); L.gy = ws.take(row);
    L.ln = ws.take(mhmr_layernorm_f32_backward_workspace_bytes((int)M, C));
    L.block = ws.take(block_layout(B, Tp, C, precision, attention).total);
    L.total = ws.at;
    return L;
}

// the six workspace-size entries: the bytes of a block's or of the tail's workspace for Tp-row images, or the error of the sizes
long long backward_bytes(int B, int Tp, int C, int precision, int attention, bool tail) {
    if (B < 0 || Tp < 0 || C < 0 || !precision_ok(precision) || !attention_ok(attention)) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return tail ? tail_layout(B, Tp, C, precision, attention).total : block_layout(B, Tp, C, precision, attention).total;
}

// the pointers of a block descriptor that the block backward reads or writes besides x_in / g_out / g_in / workspace
bool block_tensors_given(const mhmr_vit_block_backward_desc* d) {
    const void* const p[] = {d->ln1_w, d->ln1_b, d->qkv_w, d->qkv_b, d->proj_w, d->proj_b, d->ls1, d->ln2_w, d->ln2_b, d->fc1_w, d->fc1_b,
                             d->fc2_w, d->fc2_b, d->ls2, d->g_ln1_w, d->g_ln1_b, d->g_qkv_w, d->g_qkv_b, d->g_proj_w, d->g_proj_b, d->g_ls1,
                             d->g_ln2_w, d->g_ln2_b, d->g_fc1_w, d->g_fc1_b, d->g_fc2_w, d->g_fc2_b, d->g_ls2};
    for (const void* q : p)
        if (!q) return false;
    return aligned16(d->qkv_w) && aligned16(d->proj_w) && aligned16(d->fc1_w) && aligned16(d->fc2_w);
}
// the bf16 linears read their bias as 16-byte vectors
bool block_biases_aligned(const mhmr_vit_block_backward_desc* d) {
    return aligned16(d->qkv_b) && aligned16(d->proj_b) && aligned16(d->fc1_b) && aligned16(d->fc2_b);
}

// d ls = sum_rows g y, d bias = ls sum_rows g (fp64, two fixed stages), dy = g ls
int launch_layerscale_bwd(const float* g, const float* y, const float* ls, float* dy, float* d_ls, float* d_bias, int M, int C, int nsl,
                          double* part, hipStream_t s) {
    const size_t n = (size_t)M * C;
    hipLaunchKernelGGL(layerscale_bwd_kernel, dim3(blocks256(n)), dim3(256), 0, s, g, ls, dy, n, C);
    hipLaunchKernelGGL((col_sums1_kernel<LS_SLICE, 1, LsTerm>), dim3(C / 64, nsl), dim3(64), 0, s, LsTerm{g, y, C}, part, (double*)nullptr, 0, 0,
                       M, C);
    hipLaunchKernelGGL(col_sums2_kernel, dim3(C / 64), dim3(64), 0, s, (const double*)part, (const double*)nullptr, ls, d_ls, d_bias,
                       (float*)nullptr, nsl, C);
    MHMR_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

long long mhmr_vit_block_backward_workspace_bytes(int B, int Tp, int C) {
    return backward_bytes(B, Tp, C, MHMR_BWD_F32, MHMR_ATTN_F32, false);
}
long long mhmr_vit_block_backward_workspace_bytes_p(int B, int Tp, int C, int precision) {
    return backward_bytes(B, Tp, C, precision, MHMR_ATTN_F32, false);
}
long long mhmr_vit_block_backward_workspace_bytes_pa(int B, int Tp, int C, int linear_precision, int attention_precision) {
    return backward_bytes(B, Tp, C, linear_precision, attention_precision, false);
}

int mhmr_vit_block_backward(const mhmr_vit_block_backward_desc* d, void* stream) { return mhmr_vit_block_backward_a(d, MHMR_ATTN_F32, stream); }

int mhmr_vit_block_backward_a(const mhmr_vit_block_backward_desc* d, int attention_precision, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int B = d->B, T = d->T, Tp = d->Tp, C = d->C, H = d->H;
    TRY(block_shape_rc(B, T, Tp, C, H));
    if (!precision_ok(d->linear_precision) || !attention_ok(attention_precision)) return MHMR_ERR_BAD_ARG;
    const bool abf = attention_precision == MHMR_ATTN_BF16;
    const bool bf = d->linear_precision == MHMR_BWD_BF16;
    if (!block_tensors_given(d) || !d->x_in || !d->g_out || !d->g_in || !aligned16(d->x_in)) return MHMR_ERR_BAD_ARG;
    if (bf && !block_biases_aligned(d)) return MHMR_ERR_BAD_ARG;
    const BlockLayout L = block_layout(B, Tp, C, d->linear_precision, attention_precision);
    if (!d->workspace || !aligned16(d->workspace) || d->workspace_bytes < L.total || d->g_in == d->g_out) return MHMR_ERR_BAD_ARG;

    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    const int M = B * Tp;
    const size_t n = (size_t)M * C;
    float *xn1 = (float*)(ws + L.xn1), *qkv = (float*)(ws + L.qkv), *att = (float*)(ws + L.att), *y1 = (float*)(ws + L.y1);
    float *x1 = (float*)(ws + L.x1), *xn2 = (float*)(ws + L.xn2), *z1 = (float*)(ws + L.z1), *h = (float*)(ws + L.h), *y2 = (float*)(ws + L.y2);
    float *g0 = (float*)(ws + L.g0), *dy = (float*)(ws + L.dy), *dh = (float*)(ws + L.dh), *dxn = (float*)(ws + L.dxn), *g1 = (float*)(ws + L.g1);
    float *datt = (float*)(ws + L.datt), *lse = (float*)(ws + L.lse), *dqkv = dh;
    void* lnws = ws + L.ln;
    const long long lnbytes = mhmr_layernorm_f32_backward_workspace_bytes(M, C);
    double* part = (double*)(ws + L.part);
    const float eps = 1e-6f;
    // the three products of a linear without activation, in the descriptor's precision: Y [M, N] = X W^T + bias, dW [N, K] (+ db), dX [M, K]
    void* lin = ws + L.lin;
    auto fwd = [&](const float* X, const float* W, const float* bias, float* Y, int N, int K) {
        return bf ? mhmr_launch_linear_bf16(X, K, W, K, bias, Y, N, M, N, K, lin, s)
                  : mhmr_launch_linear_f32(X, K, nullptr, W, K, bias, nullptr, 0, Y, N, M, N, K, MHMR_ACT_NONE, s);
    };
    auto bwd_w = [&](const float* dY, const float* X, float* dW, float* db, int N, int K) {
        return bf ? mhmr_launch_linear_bf16_bwd_weight(dY, N, X, K, dW, K, db, M, N, K, lin, s)
                  : mhmr_linear_f32_backward_weight(dY, N, nullptr, 0, X, K, dW, K, db, M, N, K, MHMR_ACT_NONE, s);
    };
    auto bwd_x = [&](const float* dY, const float* W, float* dX, int N, int K) {
        return bf ? mhmr_launch_linear_bf16_bwd_input(dY, N, W, K, nullptr, 0, dX, K, M, N, K, lin, s)
                  : mhmr_linear_f32_backward_input(dY, N, nullptr, nullptr, 0, W, K, nullptr, 0, dX, K, M, N, K, MHMR_ACT_NONE, s);
    };
    // the attention pair in attention_precision: qkv -> (att, lse), and datt -> dqkv (the bf16 tape leaves its copy of qkv for the backward)
    auto attn_tape = [&]() {
        return abf ? mhmr_launch_attention_bf16_tape(qkv, att, lse, B, T, Tp, C, H, ws + L.attn16, s)
                   : mhmr_launch_attention_f32_tape(qkv, att, lse, B, T, Tp, C, H, s);
    };
    auto attn_bwd = [&]() {
        return abf ? mhmr_launch_attention_bf16_bwd(qkv, att, lse, datt, C, dqkv, B, T, Tp, C, H, ws + L.attn16, true, s)
                   : mhmr_launch_attention_f32_bwd(qkv, att, lse, datt, C, dqkv, B, T, Tp, C, H, ws + L.attn, s);
    };

    // ---- the tape: the block's forward in fp32, from x_in
    TRY(mhmr_launch_layernorm_f32(d->x_in, d->ln1_w, d->ln1_b, xn1, M, C, eps, s));
    TRY(fwd(xn1, d->qkv_w, d->qkv_b, qkv, 3 * C, C));
    TRY(attn_tape());
    TRY(fwd(att, d->proj_w, d->proj_b, y1, C, C));
    hipLaunchKernelGGL(layerscale_resid_kernel, dim3(blocks256(n)), dim3(256), 0, s, d->x_in, (const float*)y1, d->ls1, x1, n, C);
    TRY(mhmr_launch_layernorm_f32(x1, d->ln2_w, d->ln2_b, xn2, M, C, eps, s));
    TRY(fwd(xn2, d->fc1_w, d->fc1_b, z1, 4 * C, C));
    hipLaunchKernelGGL(gelu_f32_kernel, dim3(blocks256(4 * n)), dim3(256), 0, s, (const float*)z1, h, 4 * n);
    TRY(fwd(h, d->fc2_w, d->fc2_b, y2, C, 4 * C));

    // ---- the MLP branch: x2 = x1 + ls2 * fc2(gelu(fc1(norm2(x1))))
    hipLaunchKernelGGL(mask_rows_kernel, dim3(blocks256(n)), dim3(256), 0, s, d->g_out, g0, n, C, T, Tp);
    TRY(launch_layerscale_bwd(g0, y2, d->ls2, dy, d->g_ls2, d->g_fc2_b, M, C, L.nsl, part, s));
    TRY(bwd_w(dy, h, d->g_fc2_w, nullptr, C, 4 * C));
    TRY(bwd_x(dy, d->fc2_w, dh, C, 4 * C));
    if (bf) {
        // the GELU derivative in fp32 in front of plain products: the rounded operand does not depend on where erf is evaluated
        hipLaunchKernelGGL(gelu_bwd_inplace_kernel, dim3(blocks256(4 * n)), dim3(256), 0, s, dh, (const float*)z1, 4 * n);
        TRY(bwd_w(dh, xn2, d->g_fc1_w, d->g_fc1_b, 4 * C, C));
        TRY(bwd_x(dh, d->fc1_w, dxn, 4 * C, C));
    } else {
        TRY(mhmr_linear_f32_backward_weight(dh, 4 * C, z1, 4 * C, xn2, C, d->g_fc1_w, C, d->g_fc1_b, M, 4 * C, C, MHMR_ACT_GELU, s));
        TRY(mhmr_linear_f32_backward_input(dh, 4 * C, nullptr, z1, 4 * C, d->fc1_w, C, nullptr, 0, dxn, C, M, 4 * C, C, MHMR_ACT_GELU, s));
    }
    TRY(mhmr_layernorm_f32_backward(x1, d->ln2_w, dxn, g0, g1, d->g_ln2_w, d->g_ln2_b, M, C, eps, lnws, lnbytes, s));

    // ---- the attention branch: x1 = x + ls1 * proj(MHSA(norm1(x)))
    TRY(launch_layerscale_bwd(g1, y1, d->ls1, dy, d->g_ls1, d->g_proj_b, M, C, L.nsl, part, s));
    TRY(bwd_w(dy, att, d->g_proj_w, nullptr, C, C));
    TRY(bwd_x(dy, d->proj_w, datt, C, C));
    TRY(attn_bwd());
    TRY(bwd_w(dqkv, xn1, d->g_qkv_w, d->g_qkv_b, 3 * C, C));
    TRY(bwd_x(dqkv, d->qkv_w, dxn, 3 * C, C));
    TRY(mhmr_layernorm_f32_backward(d->x_in, d->ln1_w, dxn, g1, d->g_in, d->g_ln1_w, d->g_ln1_b, M, C, eps, lnws, lnbytes, s));
    MHMR_CHECK_LAUNCH();
    return 0;
}

long long mhmr_vit_tail_backward_workspace_bytes(int B, int Tp, int C) {
    return backward_bytes(B, Tp, C, MHMR_BWD_F32, MHMR_ATTN_F32, true);
}
long long mhmr_vit_tail_backward_workspace_bytes_p(int B, int Tp, int C, int precision) {
    return backward_bytes(B, Tp, C, precision, MHMR_ATTN_F32, true);
}
long long mhmr_vit_tail_backward_workspace_bytes_pa(int B, int Tp, int C, int linear_precision, int attention_precision) {
    return backward_bytes(B, Tp, C, linear_precision, attention_precision, true);
}

int mhmr_vit_tail_backward(const mhmr_vit_tail_backward_desc* d, void* stream) { return mhmr_vit_tail_backward_a(d, MHMR_ATTN_F32, stream); }

int mhmr_vit_tail_backward_a(const mhmr_vit_tail_backward_desc* d, int attention_precision, void* stream) {
    if (!d) return MHMR_ERR_BAD_ARG;
    const int B = d->B, T = d->T, Tp = d->Tp, C = d->C, H = d->H, n = d->n;
    if (d->N < 0 || n < 0) return MHMR_ERR_BAD_ARG;
    TRY(block_shape_rc(B, T, Tp, C, H));
    if (n == 0 || d->N != T - 1) return MHMR_ERR_BAD_SHAPE;
    if (!precision_ok(d->linear_precision) || !attention_ok(attention_precision)) return MHMR_ERR_BAD_ARG;
    if (!d->norm_w || !d->norm_b || !d->blocks || !d->tap || !d->resid || !d->g_feat || !d->g_norm_w || !d->g_norm_b || !d->g_stream)
        return MHMR_ERR_BAD_ARG;
    const TailLayout L = tail_layout(B, Tp, C, d->linear_precision, attention_precision);
    if (!d->workspace || !aligned16(d->workspace) || d->workspace_bytes < L.total || !aligned16(d->tap) || !aligned16(d->g_stream))
        return MHMR_ERR_BAD_ARG;
    for (int i = 0; i < n; ++i)
        if (!block_tensors_given(&d->blocks[i]) || (d->linear_precision == MHMR_BWD_BF16 && !block_biases_aligned(&d->blocks[i])))
            return MHMR_ERR_BAD_ARG;

    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)d->workspace;
    const int M = B * Tp;
    const size_t rows = (size_t)M * C;
    float *dy = (float*)(ws + L.dy), *gy = (float*)(ws + L.gy);
    // the stream cotangent alternates between g_stream and gy so that the last block writes g_stream
    auto cur = [&](int k) { return (n - k) % 2 == 0 ? d->g_stream : gy; };
    hipLaunchKernelGGL(scatter_patch_rows_kernel, dim3(blocks256(rows)), dim3(256), 0, s, d->g_feat, dy, rows, C, d->N, Tp);
    TRY(mhmr_layernorm_f32_backward(d->resid, d->norm_w, dy, nullptr, cur(0), d->g_norm_w, d->g_norm_b, M, C, 1e-6f, ws + L.ln,
                                    mhmr_layernorm_f32_backward_workspace_bytes(M, C), s));
    for (int k = 0; k < n; ++k) {
        mhmr_vit_block_backward_desc b = d->blocks[n - 1 - k];
        b.B = B; b.T = T; b.Tp = Tp; b.C = C; b.H = H;
        b.linear_precision = d->linear_precision;      // the tail's own value: the blocks' field is ignored, like their shapes
        b.x_in = d->tap + (size_t)(n - 1 - k) * rows;
        b.g_out = cur(k);
        b.g_in = cur(k + 1);
        b.workspace = ws + L.block;
        b.workspace_bytes = L.total - L.block;
        TRY(mhmr_vit_block_backward_a(&b, attention_precision, s));
    }
    MHMR_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
