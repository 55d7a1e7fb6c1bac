// Backward of one ViT block: the derivative of the fp32 function
//     x -> x + ls1 * proj(MHSA(norm1(x))),   x -> x + ls2 * fc2(gelu(fc1(norm2(x))))
// with the fp32 master weights, at the block input the inference forward produced.  The block's activations are recomputed from that
// input in fp32 (the tape); none of the forward's 16-bit workspaces is read, so the forward's 16-bit roundings are straight-through.
//
// Rules (DESIGN.md sections 17-22): sums that cross rows are fp64 or fp32 MFMA chains (v_mfma_f32_16x16x4_f32) of a shape fixed by the
// sizes alone; no floating-point atomics; every element of every output is written; results are bit-reproducible call to call.
//
// Attention.  The tape kernel is attention_f32.hip's kernel with an fp32 output and the per-query log-sum lse = max + log2(sum) of the
// exp2-domain logits s = (q MHMR_ATTN_QSCALE) . k.  The backward is two passes, so that no sum crosses a workgroup; in both one wave
// owns 16 rows of one (image, head), a workgroup is 4 waves = 64 consecutive rows, the other side streams past in tiles of 16 straight
// from global memory (the waves of a workgroup and the workgroups of a head share the rows through L1 / L2; no LDS).  With
// c = lane & 15, g = lane >> 4 and the fragment geometry of attention_f32.hip's header:
//   query pass  S^T = K Q^T and dP^T = V dO^T   A = K | V [key c][d = 16 g + s]      B = Q^T | dO^T [d = 16 g + s][query c]
//               D: lane holds [key 4 g + i][query c]; p = exp2(s - lse) r, dS = p (dP - D_query); r = 1 / sum exp2(s - lse) and
//               D = sum p dP come from a first loop over the keys with these two products alone
//               dQ^T = K^T dS^T                 A = K^T[d = 4 c + db][key 4 g + i]   B = the lane's own dS_i
//               D: lane holds dQ^T[d = 16 g + 4 i' + db][query c]: 16 consecutive d of one query
//   key pass    S = Q K^T and dP = dO V^T       A = Q | dO [query c][d = 16 g + s]   B = K^T | V^T [d = 16 g + s][key c]
//               D: lane holds [query 4 g + i][key c]      (the same products in the same order as the query pass: the same p)
//               dV^T = dO^T P, dK^T = Q^T dS    A = dO^T | Q^T [d = 4 c + db][query 4 g + i]   B = the lane's own p_i | dS_i
// A column of an MFMA result depends on that column of B alone, so a row >= T inside a tile (any finite values) reaches no real row: its
// own p and dS are replaced by zeros where it is the summed index, and its own result is stored as zeros.  dQ and dK carry the factor
// head_dim^-0.5 = 1/8, exact.
// attention_precision = MHMR_ATTN_BF16 of the `_a` entries replaces this pair, inside the block, by the bf16-operand
// pair of attention_bf16.hip; MHMR_ATTN_F32, and the entries without the argument, issue exactly the launches described here.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "row_sums.h"

namespace {

constexpr float ATTN_SCALE = 0.125f;                       // head_dim^-0.5 for head_dim = 64
constexpr int LS_SLICE = 32;                               // rows per first-stage slice of the LayerScale / bias column sums

__device__ __forceinline__ void load16(const float* p, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = *(const f32x4*)(p + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * j + e] = t[e];
    }
}

// ------------------------------------------------------------------------------------------------------------ attention tape
__global__ __launch_bounds__(256) void attn_tape_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse, int T,
                                                        int Tp, int C, int H) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * 64 + 16 * w;
    const size_t ld = 3 * (size_t)C;
    const float* img = qkv + (size_t)b * Tp * ld + (size_t)h * 64;
    float* orow = out + ((size_t)b * Tp + q0 + c) * (size_t)C + h * 64 + 16 * g;
    float* lrow = lse + ((size_t)b * H + h) * Tp + q0 + c;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    if (q0 >= T) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)(orow + 4 * j) = zero;
        if (g == 0) *lrow = 0.f;
        return;
    }
    float qf[16];
    load16(img + (size_t)(q0 + c) * ld + 16 * g, qf);
#pragma unroll
    for (int s = 0; s < 16; ++s) qf[s] *= MHMR_ATTN_QSCALE;
    const float* kbase = img + C + (size_t)c * ld + 16 * g;             // K[key0 + c][16 g ..]
    const float* vbase = img + 2 * C + (size_t)(4 * g) * ld + 4 * c;    // V[key0 + 4 g + i][4 c ..]

    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = zero;
    float m_run = -INFINITY, l_run = 0.f;
    const int ntile = (T + 15) >> 4;
    for (int t = 0; t < ntile; ++t) {
        const int key0 = 16 * t;
        float kf[16];
        f32x4 vf[4];
        load16(kbase + (size_t)key0 * ld, kf);
#pragma unroll
        for (int i = 0; i < 4; ++i) vf[i] = *(const f32x4*)(vbase + (size_t)(key0 + i) * ld);
        f32x4 s = zero;
#pragma unroll
        for (int e = 0; e < 16; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[e], s, 0, 0, 0);
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (key0 + 4 * g + i >= T) s[i] = -INFINITY;
            mx = fmaxf(mx, s[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);                  // finite from tile 0 on (key 0 is real)
        const float scale = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        float p[4], ps = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            p[i] = __builtin_amdgcn_exp2f(s[i] - m_new);
            ps += p[i];
        }
        l_run = l_run * scale + ps;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[db][e] *= scale;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i][db], p[i], o[db], 0, 0, 0);
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    const bool real = q0 + c < T;
    const float inv = real ? 1.0f / l_run : 0.f;
    // lane (c, g): query q0 + c, d = 16 g + 4 i' + db  (o[db][i'])
#pragma unroll
    for (int ip = 0; ip < 4; ++ip) {
        f32x4 v;
#pragma unroll
        for (int db = 0; db < 4; ++db) v[db] = real ? o[db][ip] * inv : 0.f;
        *(f32x4*)(orow + 4 * ip) = v;
    }
    if (g == 0) *lrow = real ? m_run + log2f(l_run) : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ attention backward, query pass
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ lse, const float* __restrict__ dO, int lddo,
                                                         float* __restrict__ dqkv, float* __restrict__ Dws, float* __restrict__ Rws, int T, int Tp, int C,
                                                         int H) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * 64 + 16 * w;
    const size_t ld = 3 * (size_t)C;
    const float* img = qkv + (size_t)b * Tp * ld + (size_t)h * 64;
    const size_t qrow = (size_t)b * Tp + q0 + c;
    float* dqrow = dqkv + qrow * ld + h * 64 + 16 * g;
    const size_t stat = ((size_t)b * H + h) * Tp + q0 + c;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    if (q0 >= T) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)(dqrow + 4 * j) = zero;
        if (g == 0) { Dws[stat] = 0.f; Rws[stat] = 0.f; }
        return;
    }
    const bool real = q0 + c < T;
    float qf[16], dof[16];
    load16(img + (size_t)(q0 + c) * ld + 16 * g, qf);
#pragma unroll
    for (int s = 0; s < 16; ++s) qf[s] *= MHMR_ATTN_QSCALE;
    load16(dO + qrow * (size_t)lddo + h * 64 + 16 * g, dof);
    const float lq = lse[stat];
    const float* kbase = img + C + (size_t)c * ld + 16 * g;             // K[key0 + c][16 g ..]
    const float* vbase = img + 2 * C + (size_t)c * ld + 16 * g;         // V[key0 + c][16 g ..]
    const float* kabase = img + C + (size_t)(4 * g) * ld + 4 * c;       // K[key0 + 4 g + i][4 c ..]

    const int ntile = (T + 15) >> 4;
    // First pass over the keys: the query's normaliser and its D.
    //   rq  lse is ONE fp32 number, so exp2(s - lse) carries its rounding (|lse| 2^-24, absolute, in the exponent) as a factor common to
    //       the query's row of P.  rq = 1 / sum_keys exp2(s - lse) takes it out again: P = exp2(s - lse) rq sums to one, as a softmax
    //       normalised by its own sum does.
    //   D   = sum_keys P dP, from the very P and dP that form dS = P (dP - D) below -- not dO . O of the tape: with few keys or a peaked
    //       row, dP - D cancels, and only a D made of the same rounded numbers cancels with them (measured on the CPU in fp32 at T = 2: dQ
    //       and dK 3.5x the error of torch's own fp32 softmax backward with dO . O, 1.3x with this form).  out32 is therefore not read.
    // The key pass reads both from the workspace.
    float rq = 0.f, Dq = 0.f;
    for (int t = 0; t < ntile; ++t) {
        const int key0 = 16 * t;
        float kf[16], vf[16];
        load16(kbase + (size_t)key0 * ld, kf);
        load16(vbase + (size_t)key0 * ld, vf);
        f32x4 s = zero, dp = zero;
#pragma unroll
        for (int e = 0; e < 16; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[e], s, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[e], dof[e], dp, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float pe = key0 + 4 * g + i < T ? __builtin_amdgcn_exp2f(s[i] - lq) : 0.f;
            rq += pe;
            Dq += key0 + 4 * g + i < T ? pe * dp[i] : 0.f;
        }
    }
    rq += __shfl_xor(rq, 16);
    rq += __shfl_xor(rq, 32);
    Dq += __shfl_xor(Dq, 16);
    Dq += __shfl_xor(Dq, 32);
    rq = 1.0f / rq;
    Dq *= rq;

    f32x4 dq[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) dq[db] = zero;
    for (int t = 0; t < ntile; ++t) {
        const int key0 = 16 * t;
        float kf[16], vf[16];
        f32x4 ka[4];
        load16(kbase + (size_t)key0 * ld, kf);
        load16(vbase + (size_t)key0 * ld, vf);
#pragma unroll
        for (int i = 0; i < 4; ++i) ka[i] = *(const f32x4*)(kabase + (size_t)(key0 + i) * ld);
        f32x4 s = zero, dp = zero;
#pragma unroll
        for (int e = 0; e < 16; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[e], s, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[e], dof[e], dp, 0, 0, 0);
        float ds[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float p = __builtin_amdgcn_exp2f(s[i] - lq) * rq;
            ds[i] = key0 + 4 * g + i < T ? p * (dp[i] - Dq) : 0.f;      // keys >= T (the tail of the last tile) are masked
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int db = 0; db < 4; ++db) dq[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[i][db], ds[i], dq[db], 0, 0, 0);
    }
#pragma unroll
    for (int ip = 0; ip < 4; ++ip) {
        f32x4 v;
#pragma unroll
        for (int db = 0; db < 4; ++db) v[db] = real ? dq[db][ip] * ATTN_SCALE : 0.f;
        *(f32x4*)(dqrow + 4 * ip) = v;
    }
    if (g == 0) { Dws[stat] = real ? Dq : 0.f; Rws[stat] = real ? rq : 0.f; }
}

// ------------------------------------------------------------------------------------------------------------ attention backward, key pass
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                          const float* __restrict__ dO, int lddo, float* __restrict__ dqkv,
                                                          const float* __restrict__ Dws, const float* __restrict__ Rws, int T, int Tp, int C,
                                                          int H) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y;
    const int k0 = blockIdx.x * 64 + 16 * w;                 // the wave's first key row inside the image
    const size_t ld = 3 * (size_t)C;
    const float* img = qkv + (size_t)b * Tp * ld + (size_t)h * 64;
    float* dkrow = dqkv + ((size_t)b * Tp + k0 + c) * ld + C + h * 64 + 16 * g;
    float* dvrow = dkrow + C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    if (k0 >= T) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { *(f32x4*)(dkrow + 4 * j) = zero; *(f32x4*)(dvrow + 4 * j) = zero; }
        return;
    }
    const bool real = k0 + c < T;
    float kf[16], vf[16];
    load16(img + C + (size_t)(k0 + c) * ld + 16 * g, kf);
    load16(img + 2 * C + (size_t)(k0 + c) * ld + 16 * g, vf);
    const float* qbase = img + (size_t)c * ld + 16 * g;                                      // Q[q0 + c][16 g ..]
    const float* qtbase = img + (size_t)(4 * g) * ld + 4 * c;                                // Q[q0 + 4 g + i][4 c ..]
    const float* dobase = dO + ((size_t)b * Tp + c) * (size_t)lddo + h * 64 + 16 * g;        // dO[q0 + c][16 g ..]
    const float* dotbase = dO + ((size_t)b * Tp + 4 * g) * (size_t)lddo + h * 64 + 4 * c;    // dO[q0 + 4 g + i][4 c ..]
    const float* lbase = lse + ((size_t)b * H + h) * Tp + 4 * g;
    const float* dbase = Dws + ((size_t)b * H + h) * Tp + 4 * g;
    const float* rbase = Rws + ((size_t)b * H + h) * Tp + 4 * g;

    f32x4 dk[4], dv[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) dk[db] = dv[db] = zero;
    const int ntile = (T + 15) >> 4;
    for (int t = 0; t < ntile; ++t) {
        const int q0 = 16 * t;
        float qa[16], da[16];
        f32x4 qt[4], dt[4];
        load16(qbase + (size_t)q0 * ld, qa);
#pragma unroll
        for (int s = 0; s < 16; ++s) qa[s] *= MHMR_ATTN_QSCALE;
        load16(dobase + (size_t)q0 * lddo, da);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            qt[i] = *(const f32x4*)(qtbase + (size_t)(q0 + i) * ld);
            dt[i] = *(const f32x4*)(dotbase + (size_t)(q0 + i) * lddo);
        }
        const f32x4 l4 = *(const f32x4*)(lbase + q0), d4 = *(const f32x4*)(dbase + q0), r4 = *(const f32x4*)(rbase + q0);
        f32x4 s = zero, dp = zero;
#pragma unroll
        for (int e = 0; e < 16; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[e], kf[e], s, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 16; ++e) dp = __builtin_amdgcn_mfma_f32_16x16x4f32(da[e], vf[e], dp, 0, 0, 0);
        float p[4], ds[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool qreal = q0 + 4 * g + i < T;            // queries >= T (the tail of the last tile) are masked
            const float pe = __builtin_amdgcn_exp2f(s[i] - l4[i]) * r4[i];
            p[i] = qreal ? pe : 0.f;
            ds[i] = qreal ? pe * (dp[i] - d4[i]) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int db = 0; db < 4; ++db) {
                dv[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[i][db], p[i], dv[db], 0, 0, 0);
                dk[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[i][db], ds[i], dk[db], 0, 0, 0);
            }
    }
#pragma unroll
    for (int ip = 0; ip < 4; ++ip) {
        f32x4 vk, vv;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            vk[db] = real ? dk[db][ip] * ATTN_SCALE : 0.f;
            vv[db] = real ? dv[db][ip] : 0.f;
        }
        *(f32x4*)(dkrow + 4 * ip) = vk;
        *(f32x4*)(dvrow + 4 * ip) = vv;
    }
}

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

inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

// ------------------------------------------------------------------------------------------------------------ shapes and layouts
int attn_shape_rc(int B, int T, int Tp, int C, int H) {
    if (B < 0 || T < 0 || Tp < 0 || C < 0 || H < 0) return MHMR_ERR_BAD_ARG;
    if (B == 0 || T == 0 || Tp % 64 || Tp < T || C != 64 * H || H > 65535 || B > 65535) return MHMR_ERR_BAD_SHAPE;
    return 0;
}
inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }
inline long long attn_stat_bytes(int B, int Tp, int H) { return align256((long long)B * H * Tp * (long long)sizeof(float)); }
inline long long attn_bwd_bytes(int B, int Tp, int H) { return 2 * attn_stat_bytes(B, Tp, H); }      // D | r, [B, H, Tp] each

int launch_attn_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, hipStream_t s) {
    hipLaunchKernelGGL(attn_tape_kernel, dim3(Tp / 64, H, B), dim3(256), 0, s, qkv, out32, lse, T, Tp, C, H);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_attn_bwd(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T, int Tp, int C,
                    int H, float* Dws, hipStream_t s) {
    const dim3 grid(Tp / 64, H, B);
    float* Rws = (float*)((char*)Dws + attn_stat_bytes(B, Tp, H));
    hipLaunchKernelGGL(attn_bwd_q_kernel, grid, dim3(256), 0, s, qkv, lse, dO, lddo, dqkv, Dws, Rws, T, Tp, C, H);
    hipLaunchKernelGGL(attn_bwd_kv_kernel, grid, dim3(256), 0, s, qkv, lse, dO, lddo, dqkv, (const float*)Dws, (const float*)Rws, T, Tp, C, H);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int block_shape_rc(int B, int T, int Tp, int C, int H) {
    TRY(attn_shape_rc(B, T, Tp, C, H));
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
BlockLayout block_layout(int B, int Tp, int C, int precision = MHMR_BWD_F32, int attention = MHMR_ATTN_F32) {
    BlockLayout L;
    WsCursor ws;
    const long long M = (long long)B * Tp, row = M * C * (long long)sizeof(float);
    L.nsl = (int)((M + LS_SLICE - 1) / LS_SLICE);
    L.xn1 = ws.take(row); L.qkv = ws.take(3 * row); L.att = ws.take(row); L.y1 = ws.take(row); L.x1 = ws.take(row);
    L.xn2 = ws.take(row); L.z1 = ws.take(4 * row); L.h = ws.take(4 * row); L.y2 = ws.take(row);
    L.g0 = ws.take(row); L.dy = ws.take(row); L.dh = ws.take(4 * row);      // dh: cotangent of h, later dqkv (3 C wide)
    L.dxn = ws.take(row); L.g1 = ws.take(row); L.datt = ws.take(row);
    L.lse = ws.take(M * (C / 64) * (long long)sizeof(float));
    L.attn = ws.take(attn_bwd_bytes(B, Tp, C / 64));
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
TailLayout tail_layout(int B, int Tp, int C, int precision = MHMR_BWD_F32, int attention = MHMR_ATTN_F32) {
    TailLayout L;
    WsCursor ws;
    const long long M = (long long)B * Tp, row = M * C * (long long)sizeof(float);
    L.dy = ws.take(row); L.gy = ws.take(row);
    L.ln = ws.take(mhmr_layernorm_f32_backward_workspace_bytes((int)M, C));
    L.block = ws.take(block_layout(B, Tp, C, precision, attention).total);
    L.total = ws.at;
    return L;
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

int mhmr_attention_f32_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* stream) {
    TRY(attn_shape_rc(B, T, Tp, C, H));
    if (!qkv || !out32 || !lse || !aligned16(qkv) || !aligned16(out32)) return MHMR_ERR_BAD_ARG;
    return launch_attn_tape(qkv, out32, lse, B, T, Tp, C, H, (hipStream_t)stream);
}

long long mhmr_attention_f32_backward_workspace_bytes(int B, int Tp, int H) {
    if (B < 0 || Tp < 0 || H < 0) return MHMR_ERR_BAD_ARG;
    if (B == 0 || Tp == 0 || H == 0 || Tp % 64 || H > 65535 || B > 65535) return MHMR_ERR_BAD_SHAPE;
    return attn_bwd_bytes(B, Tp, H);
}

int mhmr_attention_f32_backward(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                int Tp, int C, int H, void* workspace, long long workspace_bytes, void* stream) {
    TRY(attn_shape_rc(B, T, Tp, C, H));
    if (lddo < C || lddo % 4) return MHMR_ERR_BAD_SHAPE;
    if (!qkv || !out32 || !lse || !dO || !dqkv || !workspace || workspace_bytes < attn_bwd_bytes(B, Tp, H)) return MHMR_ERR_BAD_ARG;
    if (!aligned16(qkv) || !aligned16(out32) || !aligned16(lse) || !aligned16(dO) || !aligned16(dqkv) || !aligned16(workspace))
        return MHMR_ERR_BAD_ARG;
    return launch_attn_bwd(qkv, out32, lse, dO, lddo, dqkv, B, T, Tp, C, H, (float*)workspace, (hipStream_t)stream);
}

long long mhmr_vit_block_backward_workspace_bytes(int B, int Tp, int C) {
    if (B < 0 || Tp < 0 || C < 0) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return block_layout(B, Tp, C).total;
}

long long mhmr_vit_block_backward_workspace_bytes_p(int B, int Tp, int C, int precision) {
    if (B < 0 || Tp < 0 || C < 0 || !precision_ok(precision)) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return block_layout(B, Tp, C, precision).total;
}

long long mhmr_vit_block_backward_workspace_bytes_pa(int B, int Tp, int C, int linear_precision, int attention_precision) {
    if (B < 0 || Tp < 0 || C < 0 || !precision_ok(linear_precision) || !attention_ok(attention_precision)) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return block_layout(B, Tp, C, linear_precision, attention_precision).total;
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
    float* Dws = (float*)(ws + L.attn);
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

    // ---- the tape: the block's forward in fp32, from x_in
    TRY(mhmr_launch_layernorm_f32(d->x_in, d->ln1_w, d->ln1_b, xn1, M, C, eps, s));
    TRY(fwd(xn1, d->qkv_w, d->qkv_b, qkv, 3 * C, C));
    if (abf) TRY(mhmr_launch_attention_bf16_tape(qkv, att, lse, B, T, Tp, C, H, ws + L.attn16, s));
    else TRY(launch_attn_tape(qkv, att, lse, B, T, Tp, C, H, s));
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
    if (abf) TRY(mhmr_launch_attention_bf16_bwd(qkv, att, lse, datt, C, dqkv, B, T, Tp, C, H, ws + L.attn16, true, s));
    else TRY(launch_attn_bwd(qkv, att, lse, datt, C, dqkv, B, T, Tp, C, H, Dws, s));
    TRY(bwd_w(dqkv, xn1, d->g_qkv_w, d->g_qkv_b, 3 * C, C));
    TRY(bwd_x(dqkv, d->qkv_w, dxn, 3 * C, C));
    TRY(mhmr_layernorm_f32_backward(d->x_in, d->ln1_w, dxn, g1, d->g_in, d->g_ln1_w, d->g_ln1_b, M, C, eps, lnws, lnbytes, s));
    MHMR_CHECK_LAUNCH();
    return 0;
}

long long mhmr_vit_tail_backward_workspace_bytes(int B, int Tp, int C) {
    if (B < 0 || Tp < 0 || C < 0) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return tail_layout(B, Tp, C).total;
}

long long mhmr_vit_tail_backward_workspace_bytes_p(int B, int Tp, int C, int precision) {
    if (B < 0 || Tp < 0 || C < 0 || !precision_ok(precision)) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return tail_layout(B, Tp, C, precision).total;
}

long long mhmr_vit_tail_backward_workspace_bytes_pa(int B, int Tp, int C, int linear_precision, int attention_precision) {
    if (B < 0 || Tp < 0 || C < 0 || !precision_ok(linear_precision) || !attention_ok(attention_precision)) return MHMR_ERR_BAD_ARG;
    if (C == 0 || C % 64) return MHMR_ERR_BAD_SHAPE;
    TRY(block_shape_rc(B, Tp, Tp, C, C / 64));
    return tail_layout(B, Tp, C, linear_precision, attention_precision).total;
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
