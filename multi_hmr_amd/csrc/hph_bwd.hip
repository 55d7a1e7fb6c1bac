// Backward of the fp32 person-head decoder stack (hph.hip): the derivative of mhmr_xattn_layers_forward as its
// kernels evaluate it.  Operands are fp32 except the context operand ctx16 and to_kv16, which are 16-bit values taken as exact numbers
// (the gradient of to_kv is that of the rounded weight: straight-through).
//
// Rules (DESIGN.md sections 17-19): sums that cross rows, persons or tiles are fp64 or fp32 MFMA chains (v_mfma_f32_16x16x4_f32 == an
// fmaf chain) of a shape fixed by the sizes and tables alone; no floating-point atomics; every element of every output is written;
// results are bit-reproducible call to call.
//
//   linear, input side    dX[m][k] = sum_n dZ[row(m)][n] W[n][k] (+ dR[m][k]),  dZ = dY * act'(Z)       (Z = TAPED pre-activation);
//                         the n range split over the four waves of a workgroup, partial sums added in wave order
//   linear, weight side   dW[n][k] = sum_m dZ[m][n] X[m][k]  (MFMA chain over m, zero-padded to a multiple of 4, blocked: one chain per
//                         256 rows, added up in two further levels -- the rows are persons here and B Tp token rows in vit_bwd.hip),
//                         db[n] = fp64 sum
//   LayerNorm             dx one wave per row (+ dR: the residual stream's cotangent); d gamma, d beta: fp64, two fixed stages
//   self-attention        (q) lane = query: lse, D = dO . O, dq;  (kv) lane = key: dK, dV over the group's queries in index order
//   cross-attention       (a) lse and D per (query, head), (b) dq with the forward's lane / wave split of the keys, (c) dkv with
//                         lane = key over the image's queries in index order.  Rows of images WITHOUT queries are written as zeros,
//                         so the to_kv reduction may run over all B N rows.
//   to_kv gradient        dWkv[n][c] = sum_rows dkv[row][n] ctx16[row][c]: fp32 MFMA, the row range split into <= 16 slices whose
//                         partial products are added in slice order (fp64) by a finishing pass; columns c >= cvalid are exact zeros.
//   feature cotangent     (nullable g_feat) g_feat[m][c] = sum over the layers of dkv_l[m] . to_kv16_l[:, c] for every
//                         context row (rows times weight of row_sums.h: the first layer visited writes, the others add), then
//                         g_zc + g_token added at the persons' own rows.
// The sliced outer product of the to_kv gradient, the two stages of the LayerNorm parameter sums and the workspace cursor are those of
// row_sums.h, which detect_bwd.hip shares; this file holds the LayerNorm term, the launchers and the layouts.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "hph_shared.h"
#include "row_sums.h"

namespace {

constexpr int LN_SLICE = 32;                              // rows per first-stage slice of the LayerNorm parameter sums

__device__ __forceinline__ float dact(float z, int act) {
    if (act == MHMR_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == MHMR_ACT_GELU) return 0.5f * (1.0f + erff(z * 0.70710678118654752440f)) + z * 0.39894228040143267794f * expf(-0.5f * z * z);
    return 1.f;
}

// ------------------------------------------------------------------------------------------------------------
// Linear backward, input side.  One workgroup = one 16 (m) x 32 (k) tile; the reduction over n runs in steps of 16 (lane group g takes
// n + 4 g .. n + 4 g + 3; columns >= N contribute an exact zero) and is split over the four waves as evenly as the steps go, the four
// partial sums added in wave order through LDS (as linear_f32_splitk_kernel: deterministic, and four short chains round less than one).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_bwd_input_kernel(const float* __restrict__ dY, int lddy, const int* __restrict__ row_idx,
                                                               const float* __restrict__ Z, int ldz, const float* __restrict__ W, int ldw,
                                                               const float* dR, int lddr, float* dX, int lddx, int M, int N, int K,
                                                               int act) {
    __shared__ f32x4 part[3][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int m0 = blockIdx.y * 16, k0 = blockIdx.x * 32;
    int mrow = min(m0 + l15, M - 1);
    if (row_idx) mrow = row_idx[mrow];
    const float* yp = dY + (size_t)mrow * lddy;
    const float* zp = Z ? Z + (size_t)mrow * ldz : nullptr;
    const int kc0 = min(k0 + l15, K - 1), kc1 = min(k0 + 16 + l15, K - 1);
    const int nch = (N + 15) >> 4, cb = nch >> 2, cr = nch & 3;
    const int n_lo = 16 * (w * cb + min(w, cr)), n_hi = n_lo + 16 * (cb + (w < cr ? 1 : 0));
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int n = n_lo; n < n_hi; n += 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int nn = n + 4 * g + e, nc = min(nn, N - 1);
            float a = yp[nc];
            if (zp) a *= dact(zp[nc], act);
            if (nn >= N) a = 0.f;
            const float* wp = W + (size_t)nc * ldw;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[kc0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wp[kc1], acc1, 0, 0, 0);
        }
    }
    if (w > 0) { part[w - 1][0][lane] = acc0; part[w - 1][1][lane] = acc1; }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const f32x4 p0 = part[q][0][lane], p1 = part[q][1][lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc0[r] += p0[r]; acc1[r] += p1[r]; }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k = k0 + 16 * t + l15;
        if (k >= K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 4 * g + r;
            if (m >= M) continue;
            float v = t == 0 ? acc0[r] : acc1[r];
            if (dR) v += dR[(size_t)m * lddr + k];
            dX[(size_t)m * lddx + k] = v;
        }
    }
}

// Linear backward, weight side.  One wave = 16 (n) x 32 (k); block = 4 waves along k.  The sum runs over the rows m (persons in the
// heads, B Tp token rows in the backbone blocks) in index order, four per MFMA (lane group g takes row m + g; rows >= M contribute an
// exact zero), as a blocked chain (BlockedSum2 of hph_shared.h): one MFMA chain per 256 rows, flushed into a second accumulator, and that into a third
// every 4096 rows.  Up to 256 rows this is the single chain, bit for bit; a single chain over all rows is good to a few hundred rows only
// (measured against fp32 CPU torch: 1.9x its relative L2 error at 640 rows, 4.5x at 4 160, 12x at 133 120).
__global__ __launch_bounds__(256) void linear_bwd_weight_kernel(const float* __restrict__ dY, int lddy, const float* __restrict__ Z, int ldz,
                                                                const float* __restrict__ X, int ldx, float* __restrict__ dW, int lddw,
                                                                int M, int N, int K, int act) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int n0 = blockIdx.y * 16, k0 = blockIdx.x * 128 + w * 32;
    if (k0 >= K) return;
    const int na = min(n0 + l15, N - 1);
    const int kc0 = min(k0 + l15, K - 1), kc1 = min(k0 + 16 + l15, K - 1);
    BlockedSum2 sum;
    for (int m2 = 0; m2 < M; m2 += BLOCKED_SUM_L1 * BLOCKED_SUM_L2) {
        const int m2end = min(M, m2 + BLOCKED_SUM_L1 * BLOCKED_SUM_L2);
        for (int m1 = m2; m1 < m2end; m1 += BLOCKED_SUM_L1) {
            const int m1end = min(M, m1 + BLOCKED_SUM_L1);
#pragma unroll 4
            for (int m = m1; m < m1end; m += 4) {
                const int mm = m + g, mc = min(mm, M - 1);
                float a = dY[(size_t)mc * lddy + na];
                if (Z) a *= dact(Z[(size_t)mc * ldz + na], act);
                if (mm >= M) a = 0.f;
                const float* xp = X + (size_t)mc * ldx;
                sum.acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xp[kc0], sum.acc0, 0, 0, 0);
                sum.acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xp[kc1], sum.acc1, 0, 0, 0);
            }
            sum.flush1();
        }
        sum.flush2();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int k = k0 + 16 * t + l15;
        if (k >= K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * g + r;
            if (n < N) dW[(size_t)n * lddw + k] = t == 0 ? sum.top0[r] : sum.top1[r];
        }
    }
}

// db[n] = sum_m dZ[m][n] in fp64, persons in index order; one thread per column.
__global__ __launch_bounds__(64) void linear_bwd_bias_kernel(const float* __restrict__ dY, int lddy, const float* __restrict__ Z, int ldz,
                                                             float* __restrict__ db, int M, int N, int act) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int m = 0; m < M; ++m) {
        float a = dY[(size_t)m * lddy + n];
        if (Z) a *= dact(Z[(size_t)m * ldz + n], act);
        s += (double)a;
    }
    db[n] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------
// LayerNorm backward.  dx: one wave per row, the statistics recomputed by the forward's own ln_row_stats and left in stats[row] =
// (mean, rstd) for the parameter sums.  dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ dR),  g = dy gamma.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layernorm_bwd_dx_kernel(const float* __restrict__ in, const float* __restrict__ gw,
                                                               const float* __restrict__ dy, const float* dR, float* dx,
                                                               float* __restrict__ stats, int rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* dp = dy + (size_t)row * C;
    float v[32], gq[32], mean, rstd;
    const int n = C / 64;
    ln_row_stats(in + (size_t)row * C, lane, C, eps, v, mean, rstd);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) {
            v[i] *= rstd;
            gq[i] = dp[i * 64 + lane] * gw[i * 64 + lane];
            s1 += gq[i];
            s2 += gq[i] * v[i];
        }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) {
            float o = rstd * (gq[i] - s1 - v[i] * s2);
            if (dR) o += dR[(size_t)row * C + i * 64 + lane];
            dx[(size_t)row * C + i * 64 + lane] = o;
        }
    if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// the two addends of (row, column) of the parameter sums (row_sums.h: stage 1 over slices of LN_SLICE rows, one column per thread; stage
// 2 the slices in index order): (dy xhat, dy)
struct LnParamTerm {
    const float *in, *dy, *stats; int C;
    __device__ __forceinline__ double operator()(int r, int, int c, double (&ta)[1], double (&tb)[1]) const {
        const float xh = (in[(size_t)r * C + c] - stats[2 * r]) * stats[2 * r + 1];
        const float d = dy[(size_t)r * C + c];
        ta[0] = (double)d * (double)xh;
        tb[0] = (double)d;
        return 0.0;
    }
};

// ------------------------------------------------------------------------------------------------------------
// Self-attention backward, query side: lane = one query (the forward's grid).  Pass 1 is the forward's self_attn_row (lse, O),
// D = dO . O; pass 2 streams the keys again: p = exp(s - lse), dq = scale sum_j p (dO . v_j - D) k_j.  lse_d[row][h] = (lse, D).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void self_attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                             const int* __restrict__ gstart, float* __restrict__ dqkv,
                                                             float* __restrict__ lse_d, int inner, float scale) {
    const int g = blockIdx.x, h = blockIdx.y, heads = inner >> 5;
    const int s0 = gstart[g], n = gstart[g + 1] - s0;
    const int qi = blockIdx.z * 64 + threadIdx.x;
    if (blockIdx.z * 64 >= n) return;
    const bool active = qi < n;
    const int ld = 3 * inner;
    const size_t row = (size_t)(s0 + (active ? qi : 0));
    float q[32], o[32], go[32], m, l;
#pragma unroll
    for (int d = 0; d < 32; ++d) go[d] = dO[row * inner + h * 32 + d];
    self_attn_row(qkv, qkv + row * ld + h * 32, s0, n, inner, h, scale, q, o, m, l);
    const float inv = 1.0f / l, lse = m + logf(l);
    float D = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) { D += go[d] * (o[d] * inv); o[d] = 0.f; }
    for (int j = 0; j < n; ++j) {
        const float* kp = qkv + (size_t)(s0 + j) * ld + inner + h * 32;
        const float* vp = kp + inner;
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) { s += q[d] * kp[d]; dp += go[d] * vp[d]; }
        const float ds = expf(s - lse) * (dp - D);
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] += ds * kp[d];
    }
    if (active) {
        float* op = dqkv + row * ld + h * 32;
#pragma unroll
        for (int d = 0; d < 32; ++d) op[d] = o[d] * scale;
        lse_d[(row * heads + h) * 2] = lse;
        lse_d[(row * heads + h) * 2 + 1] = D;
    }
}

// Key side: lane = one key of the group; the group's queries in index order at wave-uniform addresses.
__global__ __launch_bounds__(64) void self_attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                              const int* __restrict__ gstart, float* __restrict__ dqkv,
                                                              const float* __restrict__ lse_d, int inner, float scale) {
    const int g = blockIdx.x, h = blockIdx.y, heads = inner >> 5;
    const int s0 = gstart[g], n = gstart[g + 1] - s0;
    const int kj = blockIdx.z * 64 + threadIdx.x;
    if (blockIdx.z * 64 >= n) return;
    const bool active = kj < n;
    const int ld = 3 * inner;
    const size_t row = (size_t)(s0 + (active ? kj : 0));
    const float* kp = qkv + row * ld + inner + h * 32;
    float k[32], v[32], dk[32], dv[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) { k[d] = kp[d]; v[d] = kp[inner + d]; dk[d] = 0.f; dv[d] = 0.f; }
    for (int i = 0; i < n; ++i) {
        const size_t qrow = (size_t)(s0 + i);
        const float* qp = qkv + qrow * ld + h * 32;
        const float* gp = dO + qrow * inner + h * 32;
        const float lse = lse_d[(qrow * heads + h) * 2], D = lse_d[(qrow * heads + h) * 2 + 1];
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) { s += (qp[d] * scale) * k[d]; dp += gp[d] * v[d]; }
        const float p = expf(s - lse), ds = p * (dp - D);
#pragma unroll
        for (int d = 0; d < 32; ++d) { dv[d] += p * gp[d]; dk[d] += ds * (qp[d] * scale); }
    }
    if (active) {
        float* op = dqkv + row * ld + inner + h * 32;
#pragma unroll
        for (int d = 0; d < 32; ++d) { op[d] = dk[d]; op[inner + d] = dv[d]; }
    }
}

// ------------------------------------------------------------------------------------------------------------
// Cross-attention backward (a): the forward's cross_attn_row, ending in lse_d[q][h] = (log-sum-exp of the N scores, dO . O).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * CA_WAVES) void cross_attn_bwd_stats_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                  const float* __restrict__ dO, const int* __restrict__ chunks, int ncap,
                                                                  float* __restrict__ lse_d, int inner, int N, float scale) {
    CrossAttnItem it;
    float mt, lt, o[32];
    if (!cross_attn_row(q, kv, chunks, ncap, inner, N, scale, it, mt, lt, o)) return;
    const float inv = 1.0f / lt;
    const float* gp = dO + it.qrow * inner + it.h * 32;
    float D = 0.f;
#pragma unroll
    for (int d = 0; d < 32; ++d) D += gp[d] * (o[d] * inv);
    float* sp = lse_d + (it.qrow * (inner >> 5) + it.h) * 2;
    sp[0] = mt + logf(lt);
    sp[1] = D;
}

// (b) dq: the same split of the keys over lanes and waves; the 8 slices of a wave are added by xor shuffles, the waves through LDS in
// wave order.
__global__ __launch_bounds__(64 * CA_WAVES) void cross_attn_bwd_q_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                              const float* __restrict__ dO, const int* __restrict__ chunks, int ncap,
                                                              const float* __restrict__ lse_d, float* __restrict__ dq, int inner, int N,
                                                              float scale) {
    CrossAttnItem it;
    if (!cross_attn_item(chunks, ncap, inner, it)) return;
    __shared__ float part[CA_WAVES][8][33];
    const int heads = inner >> 5, h = it.h, wv = it.wv, qi = it.qi, sl = it.sl;
    const size_t qrow = it.qrow;
    const float* qp = q + qrow * inner + h * 32;
    const float* gp = dO + qrow * inner + h * 32;
    float qv[32], go[32], acc[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) { qv[d] = qp[d] * scale; go[d] = gp[d]; acc[d] = 0.f; }
    const float lse = lse_d[(qrow * heads + h) * 2], D = lse_d[(qrow * heads + h) * 2 + 1];
    const int ld = 2 * inner;
    const float* kbase = cross_attn_kbase(kv, it, inner, N);
    for (int j = sl + 8 * wv; j < N; j += 8 * CA_WAVES) {
        const float* kp = kbase + (size_t)j * ld;
        const float* vp = kp + inner;
        float kk[32];
#pragma unroll
        for (int d = 0; d < 32; d += 4) *(f32x4*)(kk + d) = *(const f32x4*)(kp + d);
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) s += qv[d] * kk[d];
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            const f32x4 vv = *(const f32x4*)(vp + d);
            dp += go[d] * vv[0]; dp += go[d + 1] * vv[1]; dp += go[d + 2] * vv[2]; dp += go[d + 3] * vv[3];
        }
        const float ds = expf(s - lse) * (dp - D);
#pragma unroll
        for (int d = 0; d < 32; ++d) acc[d] += ds * kk[d];
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
#pragma unroll
        for (int d = 0; d < 32; ++d) acc[d] += __shfl_xor(acc[d], off);
    }
    if (sl == 0) {
#pragma unroll
        for (int d = 0; d < 32; ++d) part[wv][qi][d] = acc[d];
    }
    __syncthreads();
    if (it.finishes()) {
        float* op = dq + qrow * inner + h * 32;
#pragma unroll
        for (int d = 0; d < 32; ++d) {
            float t = part[0][qi][d];
#pragma unroll
            for (int w2 = 1; w2 < CA_WAVES; ++w2) t += part[w2][qi][d];
            op[d] = t * scale;
        }
    }
}

// (c) dkv: lane = one key of image blockIdx.y; the image's work items are found by a scan of the work list (items of one image are
// consecutive, in person order), its queries looped in index order at wave-uniform addresses.  An image without queries gets zeros.
__global__ __launch_bounds__(256) void cross_attn_bwd_kv_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                const float* __restrict__ dO, const int* __restrict__ chunks, int nchunks,
                                                                const float* __restrict__ lse_d, float* __restrict__ dkv, int inner, int N,
                                                                float scale) {
    const int b = blockIdx.y, h = blockIdx.z, heads = inner >> 5;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const bool active = j < N;
    const int ld = 2 * inner;
    const size_t row = (size_t)b * N + (active ? j : 0);
    const float* kp = kv + row * ld + h * 32;
    float k[32], v[32], dk[32], dv[32];
#pragma unroll
    for (int d = 0; d < 32; d += 4) {
        *(f32x4*)(k + d) = *(const f32x4*)(kp + d);
        *(f32x4*)(v + d) = *(const f32x4*)(kp + inner + d);
    }
#pragma unroll
    for (int d = 0; d < 32; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
    for (int c = 0; c < nchunks; ++c) {
        const int cb = chunks[3 * c], q0 = chunks[3 * c + 1], nq = chunks[3 * c + 2];
        if (nq <= 0 || cb != b) continue;
        for (int i = 0; i < nq; ++i) {
            const size_t qrow = (size_t)(q0 + i);
            const float* qp = q + qrow * inner + h * 32;
            const float* gp = dO + qrow * inner + h * 32;
            const float lse = lse_d[(qrow * heads + h) * 2], D = lse_d[(qrow * heads + h) * 2 + 1];
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d) { s += (qp[d] * scale) * k[d]; dp += gp[d] * v[d]; }
            const float p = expf(s - lse), ds = p * (dp - D);
#pragma unroll
            for (int d = 0; d < 32; ++d) { dv[d] += p * gp[d]; dk[d] += ds * (qp[d] * scale); }
        }
    }
    if (active) {
        float* op = dkv + row * ld + h * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            *(f32x4*)(op + d) = *(const f32x4*)(dk + d);
            *(f32x4*)(op + inner + d) = *(const f32x4*)(dv + d);
        }
    }
}

// op16 [n] -> fp32 (to_kv16 as the exact numbers it holds: the context cotangent goes through the fp32 input-side linear)
template <int DT>
__global__ __launch_bounds__(256) void op16_to_f32_kernel(const void* __restrict__ in_, float* __restrict__ out, size_t n) {
    typedef typename Op<DT>::T T;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)((const T*)in_)[i];
}

// The four learned tables of hph_inputs_kernel: table t, row r, channel c = sum over the persons whose key (det_y for the *_x tables,
// det_x for the *_y tables: the forward's quirk) is r, in person order, fp64.  Rows nobody indexes are written as zeros.  Two persons in
// one cell of one image are outside the contract (as for the reference's indexed assignment): the second write of the context row wins
// in the forward, both would be counted here.
__global__ __launch_bounds__(256) void table_grads_kernel(const float* __restrict__ g_token, int ldt, const float* __restrict__ g_ctx, int ldc,
                                                          const int* __restrict__ det_y, const int* __restrict__ det_x,
                                                          float* __restrict__ g_cq_x, float* __restrict__ g_cq_y, float* __restrict__ g_cv_x,
                                                          float* __restrict__ g_cv_y, int P, int Cc) {
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, t = blockIdx.z;
    if (c >= Cc) return;
    const int* key = (t & 1) ? det_x : det_y;
    const float* src = t < 2 ? g_token : g_ctx;
    const int ld = t < 2 ? ldt : ldc;
    double s = 0.0;
    for (int p = 0; p < P; ++p)
        if (key[p] == r) s += (double)src[(size_t)p * ld + c];
    float* out = t == 0 ? g_cq_x : t == 1 ? g_cq_y : t == 2 ? g_cv_x : g_cv_y;
    out[(size_t)r * Cc + c] = (float)s;
}

// ---------------------------------------------------------------- launchers (arguments validated by the entries below)
int launch_linear_bwd_input(const float* dY, int lddy, const int* row_idx, const float* Z, int ldz, const float* W, int ldw, const float* dR,
                            int lddr, float* dX, int lddx, int M, int N, int K, int act, hipStream_t s) {
    hipLaunchKernelGGL(linear_bwd_input_kernel, dim3((K + 31) / 32, (M + 15) / 16), dim3(256), 0, s, dY, lddy, row_idx,
                       act == MHMR_ACT_NONE ? nullptr : Z, ldz, W, ldw, dR, lddr, dX, lddx, M, N, K, act);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_linear_bwd_weight(const float* dY, int lddy, const float* Z, int ldz, const float* X, int ldx, float* dW, int lddw, float* db, int M,
                             int N, int K, int act, hipStream_t s) {
    const float* z = act == MHMR_ACT_NONE ? nullptr : Z;
    if (dW) hipLaunchKernelGGL(linear_bwd_weight_kernel, dim3((K + 127) / 128, (N + 15) / 16), dim3(256), 0, s, dY, lddy, z, ldz, X, ldx, dW, lddw, M, N, K, act);
    if (db) hipLaunchKernelGGL(linear_bwd_bias_kernel, dim3((N + 63) / 64), dim3(64), 0, s, dY, lddy, z, ldz, db, M, N, act);
    MHMR_CHECK_LAUNCH();
    return 0;
}

struct LnLayout { int nsl; long long stats, part, total; };      // slices of stage 1; (mean, rstd) per row | stage 1's partials
inline LnLayout ln_layout(int rows, int C) {
    WsCursor ws;
    const int nsl = (rows + LN_SLICE - 1) / LN_SLICE;
    const long long stats = ws.take((long long)rows * 2 * sizeof(float)), part = ws.take((long long)nsl * C * 2 * sizeof(double));
    return {nsl, stats, part, ws.at};
}
inline long long ln_bwd_bytes(int rows, int C) { return ln_layout(rows, C).total; }

int launch_layernorm_bwd(const float* x, const float* w, const float* dy, const float* dR, float* dx, float* dw, float* db, int rows, int C,
                         float eps, void* ws, hipStream_t s) {
    const LnLayout L = ln_layout(rows, C);
    float* stats = (float*)((char*)ws + L.stats);
    double* part = (double*)((char*)ws + L.part);
    hipLaunchKernelGGL(layernorm_bwd_dx_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, w, dy, dR, dx, stats, rows, C, eps);
    hipLaunchKernelGGL((col_sums1_kernel<LN_SLICE, 1, LnParamTerm>), dim3(C / 64, L.nsl), dim3(64), 0, s, LnParamTerm{x, dy, stats, C}, part,
                       (double*)nullptr, 0, 0, rows, C);
    hipLaunchKernelGGL(col_sums2_kernel, dim3(C / 64), dim3(64), 0, s, part, (const double*)nullptr, (const float*)nullptr, dw, db,
                       (float*)nullptr, L.nsl, C);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_self_attn_bwd(const float* qkv, const float* dO, const int* gstart, float* dqkv, float* lse_d, int ngroups, int nmax, int heads,
                         hipStream_t s) {
    const dim3 grid(ngroups, heads, (nmax + 63) / 64);
    hipLaunchKernelGGL(self_attn_bwd_q_kernel, grid, dim3(64), 0, s, qkv, dO, gstart, dqkv, lse_d, heads * 32, HPH_ATT_SCALE);
    hipLaunchKernelGGL(self_attn_bwd_kv_kernel, grid, dim3(64), 0, s, qkv, dO, gstart, dqkv, lse_d, heads * 32, HPH_ATT_SCALE);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_cross_attn_bwd(const float* q, const float* kv, const float* dO, const int* chunks, int nchunks, float* dq, float* dkv, float* lse_d,
                          int heads, int N, int B, hipStream_t s) {
    for_each_work_list_launch(nchunks, [&](int c0, int n) {
        hipLaunchKernelGGL(cross_attn_bwd_stats_kernel, dim3(n * heads), dim3(64 * CA_WAVES), 0, s, q, kv, dO, chunks + 3 * c0, n, lse_d,
                           heads * 32, N, HPH_ATT_SCALE);
        if (dq)
            hipLaunchKernelGGL(cross_attn_bwd_q_kernel, dim3(n * heads), dim3(64 * CA_WAVES), 0, s, q, kv, dO, chunks + 3 * c0, n, lse_d, dq,
                               heads * 32, N, HPH_ATT_SCALE);
    });
    if (dkv)
        hipLaunchKernelGGL(cross_attn_bwd_kv_kernel, dim3((N + 255) / 256, B, heads), dim3(256), 0, s, q, kv, dO, chunks, nchunks, lse_d, dkv,
                           heads * 32, N, HPH_ATT_SCALE);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_grad_ctx_gemm(const float* G, int ldg, const void* op16, int ld16, float* dW, int rows, int Nn, int Kc, int cvalid, int dtype,
                         void* ws, hipStream_t s) {
    const int nsl = row_slices_or_one(rows);      // rows == 0: one empty slice, the product still runs
    const int srows = slice_rows(rows, nsl);
    const dim3 grid((Kc + 127) / 128, (Nn + 63) / 64, nsl);
    const LeftF32 left{G, ldg};
    if (dtype == MHMR_DT_F16)
        hipLaunchKernelGGL((row_outer_kernel<MHMR_DT_F16, LeftF32, true>), grid, dim3(256), 0, s, left, op16, ld16, (float*)ws, rows, Nn, Kc, srows);
    else
        hipLaunchKernelGGL((row_outer_kernel<MHMR_DT_BF16, LeftF32, true>), grid, dim3(256), 0, s, left, op16, ld16, (float*)ws, rows, Nn, Kc, srows);
    const long long total = (long long)Nn * Kc;
    hipLaunchKernelGGL(row_outer_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)ws, (const float*)nullptr,
                       dW, nsl, Nn, Kc, cvalid);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_table_grads(const float* g_token, int ldt, const float* g_ctx, int ldc, const int* det_y, const int* det_x, float* g_cq_x,
                       float* g_cq_y, float* g_cv_x, float* g_cv_y, int P, int G, int Cc, hipStream_t s) {
    hipLaunchKernelGGL(table_grads_kernel, dim3((Cc + 255) / 256, G, 4), dim3(256), 0, s, g_token, ldt, g_ctx, ldc, det_y, det_x, g_cq_x, g_cq_y,
                       g_cv_x, g_cv_y, P, Cc);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int launch_op16_to_f32(const void* in, float* out, size_t n, int dtype, hipStream_t s) {
    const dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == MHMR_DT_F16) hipLaunchKernelGGL((op16_to_f32_kernel<MHMR_DT_F16>), grid, dim3(256), 0, s, in, out, n);
    else hipLaunchKernelGGL((op16_to_f32_kernel<MHMR_DT_BF16>), grid, dim3(256), 0, s, in, out, n);
    MHMR_CHECK_LAUNCH();
    return 0;
}

// dense cotangent of the context's first Cout columns (row_sums.h: rows times weight), layer by layer: the first call writes, the others add
int launch_dense_ctx_grad(const float* dkv, int ldk, const void* to_kv16, int ldw, float* g_feat, int ldf, int rows, int Nn, int Cout,
                          bool accumulate, int dtype, hipStream_t s) {
    const LeftF32 left{dkv, ldk};
    if (dtype == MHMR_DT_F16) return launch_rows_times_weight<MHMR_DT_F16>(left, to_kv16, ldw, g_feat, ldf, rows, Nn, Cout, accumulate, s);
    return launch_rows_times_weight<MHMR_DT_BF16>(left, to_kv16, ldw, g_feat, ldf, rows, Nn, Cout, accumulate, s);
}

// g_feat[det_row[p]][c] += g_zc[p][c] + g_token[p][c]: the persons' own rows (distinct cells per image: one writer per element)
__global__ __launch_bounds__(256) void person_rows_add_kernel(const float* __restrict__ g_zc, const float* __restrict__ g_token, int ldt,
                                                              const int* __restrict__ det_row, float* g_feat, int ldf, int rows, int C) {
    const int p = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x;
    const int row = det_row[p];
    if (c >= C || row < 0 || row >= rows) return;
    float* op = g_feat + (size_t)row * ldf + c;
    *op = *op + (g_zc[(size_t)p * C + c] + g_token[(size_t)p * ldt + c]);
}

int launch_person_rows_add(const float* g_zc, const float* g_token, int ldt, const int* det_row, float* g_feat, int ldf, int rows, int C, int P,
                           hipStream_t s) {
    hipLaunchKernelGGL(person_rows_add_kernel, dim3(P, (C + 255) / 256), dim3(256), 0, s, g_zc, g_token, ldt, det_row, g_feat, ldf, rows, C);
    MHMR_CHECK_LAUNCH();
    return 0;
}

// the B N rows of g_feat as zeros (no person, or no layer: nothing else writes them)
int zero_feature_grad(float* g_feat, int ldf, int rows, int C, hipStream_t s) {
    if (rows <= 0) return 0;
    return (int)hipMemset2DAsync(g_feat, (size_t)ldf * 4, 0, (size_t)C * 4, (size_t)rows, s);
}

// the rules of a dense feature cotangent [B N, ldf] of Cout columns beside a context of Kc columns
int feature_grad_shape_rc(int B, int N, int heads, int Kc, int Cout, int ldf) {
    if (Cout <= 0 || Cout > Kc || ldf < Cout) return MHMR_ERR_BAD_SHAPE;
    if ((long long)B * N > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;
    return rows_times_weight_shape_rc(B * N, 64 * heads, Cout);
}

// ---------------------------------------------------------------- the stack's workspace: tape + scratch, every piece 256-byte aligned
struct StackLayout {
    long long xs, qkv, o_sa, q, o_ca, z1, h1;        // tape, per layer (xs: 3 per layer)
    long long xn, ga, gb, t_big, t_inner, kv, dkv, lse, ln, ctx, w32, total;
    long long s_x, s_qkv, s_inner, s_mlp;            // bytes of one [P, dim] / [P, 3 inner] / [P, inner] / [P, mlp] piece
};

bool stack_layout(int depth, int dim, int heads, int mlp, int Kc, int N, int B, int P, StackLayout* L) {
    if (depth < 0 || P < 0 || B <= 0 || N <= 0 || heads <= 0 || dim <= 0 || mlp <= 0 || Kc <= 0) return false;
    const long long inner = 32LL * heads, rows = (long long)B * N, Mctx = (rows + 127) / 128 * 128;
    if (rows > 0x7fffffffLL - 128 || inner > 65535LL * 32) return false;
    L->s_x = align256((long long)P * dim * 4);
    L->s_qkv = align256((long long)P * 3 * inner * 4);
    L->s_inner = align256((long long)P * inner * 4);
    L->s_mlp = align256((long long)P * mlp * 4);
    WsCursor ws;
    L->xs = ws.take(3LL * depth * L->s_x);
    L->qkv = ws.take(depth * L->s_qkv);
    L->o_sa = ws.take(depth * L->s_inner);
    L->q = ws.take(depth * L->s_inner);
    L->o_ca = ws.take(depth * L->s_inner);
    L->z1 = ws.take(depth * L->s_mlp);
    L->h1 = ws.take(depth * L->s_mlp);
    L->xn = ws.take(L->s_x);
    L->ga = ws.take(L->s_x);
    L->gb = ws.take(L->s_x);
    const long long big = 3 * inner > mlp ? 3 * inner : mlp;
    L->t_big = ws.take((long long)P * big * 4);
    L->t_inner = ws.take(L->s_inner);
    L->kv = ws.take(Mctx * 2 * inner * 4);
    L->dkv = ws.take(rows * 2 * inner * 4);
    L->lse = ws.take((long long)P * heads * 2 * 4);
    L->ln = ws.take(ln_bwd_bytes(P, dim));
    L->ctx = ws.take((long long)row_slices_or_one((int)rows) * 2 * inner * Kc * 4);
    L->w32 = ws.take(2 * inner * Kc * 4);
    L->total = ws.at;
    return true;
}

int stack_shape_rc(int dim, int heads, int mlp, int Kc, int B) {
    if (heads <= 0 || heads > 65535 || B <= 0 || B > 65535) return MHMR_ERR_BAD_SHAPE;
    return mhmr_hph_stack_shape_ok(dim, heads, mlp, Kc) ? 0 : MHMR_ERR_BAD_SHAPE;
}

}  // namespace

extern "C" {

int mhmr_linear_f32_backward_input(const float* dY, int lddy, const int* row_idx, const float* Z, int ldz, const float* W, int ldw,
                                   const float* dR, int lddr, float* dX, int lddx, int M, int N, int K, int act, void* stream) {
    if (M < 0) return MHMR_ERR_BAD_ARG;
    if (N <= 0 || K <= 0 || act < MHMR_ACT_NONE || act > MHMR_ACT_GELU || lddy < N || ldw < K || lddx < K || (dR && lddr < K) ||
        (act != MHMR_ACT_NONE && ldz < N) || (M + 15) / 16 > 65535)
        return MHMR_ERR_BAD_SHAPE;
    if (M == 0) return 0;
    if (!dY || !W || !dX || (act != MHMR_ACT_NONE && !Z)) return MHMR_ERR_BAD_ARG;
    return launch_linear_bwd_input(dY, lddy, row_idx, Z, ldz, W, ldw, dR, lddr, dX, lddx, M, N, K, act, (hipStream_t)stream);
}

int mhmr_linear_f32_backward_weight(const float* dY, int lddy, const float* Z, int ldz, const float* X, int ldx, float* dW, int lddw,
                                    float* db, int M, int N, int K, int act, void* stream) {
    if (M < 0) return MHMR_ERR_BAD_ARG;
    if (N <= 0 || K <= 0 || act < MHMR_ACT_NONE || act > MHMR_ACT_GELU || lddy < N || ldx < K || (dW && lddw < K) ||
        (act != MHMR_ACT_NONE && ldz < N) || (N + 15) / 16 > 65535)
        return MHMR_ERR_BAD_SHAPE;
    if (!dW && !db) return MHMR_ERR_BAD_ARG;
    if (M > 0 && (!dY || !X || (act != MHMR_ACT_NONE && !Z))) return MHMR_ERR_BAD_ARG;
    // M == 0: the sums are empty, the outputs are still written (zeros)
    return launch_linear_bwd_weight(dY, lddy, Z, ldz, X, ldx, dW, lddw, db, M, N, K, act, (hipStream_t)stream);
}

long long mhmr_layernorm_f32_backward_workspace_bytes(int rows, int C) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (C <= 0 || C % 64 || C > 2048 || rows > LN_SLICE * 65535) return MHMR_ERR_BAD_SHAPE;
    return ln_bwd_bytes(rows, C);
}

int mhmr_layernorm_f32_backward(const float* x, const float* w, const float* dy, const float* dR, float* dx, float* dw, float* db, int rows,
                                int C, float eps, void* workspace, long long workspace_bytes, void* stream) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (C <= 0 || C % 64 || C > 2048 || rows > LN_SLICE * 65535) return MHMR_ERR_BAD_SHAPE;      // the slices are gridDim.y of stage 1
    if (rows == 0) return 0;
    if (!x || !w || !dy || !dx || !dw || !db || !workspace || workspace_bytes < ln_bwd_bytes(rows, C)) return MHMR_ERR_BAD_ARG;
    return launch_layernorm_bwd(x, w, dy, dR, dx, dw, db, rows, C, eps, workspace, (hipStream_t)stream);
}

int mhmr_hph_self_attn_backward(const float* qkv, const float* dOut, const int* gstart, float* dqkv, float* lse_d, int ngroups, int nmax,
                                int heads, void* stream) {
    if (ngroups < 0 || nmax < 0) return MHMR_ERR_BAD_ARG;
    if (heads <= 0 || heads > 65535 || (nmax + 63) / 64 > 65535) return MHMR_ERR_BAD_SHAPE;
    if (ngroups == 0 || nmax == 0) return 0;
    if (!qkv || !dOut || !gstart || !dqkv || !lse_d) return MHMR_ERR_BAD_ARG;
    return launch_self_attn_bwd(qkv, dOut, gstart, dqkv, lse_d, ngroups, nmax, heads, (hipStream_t)stream);
}

int mhmr_hph_cross_attn_backward(const float* q, const float* kv, const float* dOut, const int* chunks, int nchunks, float* dq, float* dkv,
                                 float* lse_d, int heads, int N, int B, void* stream) {
    if (nchunks < 0) return MHMR_ERR_BAD_ARG;
    if (heads <= 0 || heads > 65535 || N <= 0 || B <= 0 || B > 65535 || (long long)B * N > 0x7fffffffLL) return MHMR_ERR_BAD_SHAPE;
    if (!kv || (!dq && !dkv)) return MHMR_ERR_BAD_ARG;
    if (nchunks > 0 && (!q || !dOut || !chunks || !lse_d)) return MHMR_ERR_BAD_ARG;
    // nchunks == 0: no image has queries; dkv is still written (zeros)
    return launch_cross_attn_bwd(q, kv, dOut, chunks, nchunks, dq, dkv, lse_d, heads, N, B, (hipStream_t)stream);
}

long long mhmr_grad_ctx_gemm_workspace_bytes(int rows, int Nn, int Kc) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (Nn <= 0 || Kc <= 0) return MHMR_ERR_BAD_SHAPE;
    return (long long)row_slices_or_one(rows) * Nn * Kc * (long long)sizeof(float);
}

int mhmr_grad_ctx_gemm(const float* G, int ldg, const void* op16, int ld16, float* dW, int rows, int Nn, int Kc, int cvalid, int dtype,
                       void* workspace, long long workspace_bytes, void* stream) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (Nn <= 0 || Kc <= 0 || ldg < Nn || ld16 < Kc || cvalid < 0 || cvalid > Kc || (Nn + 63) / 64 > 65535 ||
        (dtype != MHMR_DT_F16 && dtype != MHMR_DT_BF16))
        return MHMR_ERR_BAD_SHAPE;
    if (!dW || !workspace || workspace_bytes < mhmr_grad_ctx_gemm_workspace_bytes(rows, Nn, Kc) || (rows > 0 && (!G || !op16)))
        return MHMR_ERR_BAD_ARG;
    // rows == 0: an empty sum, dW is written as zeros
    return launch_grad_ctx_gemm(G, ldg, op16, ld16, dW, rows, Nn, Kc, cvalid, dtype, workspace, (hipStream_t)stream);
}

long long mhmr_xattn_layers_backward_workspace_bytes(int depth, int dim, int heads, int mlp, int Kc, int N, int B, int P) {
    if (depth < 0 || P < 0) return MHMR_ERR_BAD_ARG;
    if (N <= 0) return MHMR_ERR_BAD_SHAPE;
    const int rc = stack_shape_rc(dim, heads, mlp, Kc, B);
    if (rc) return rc;
    StackLayout L;
    if (!stack_layout(depth, dim, heads, mlp, Kc, N, B, P, &L)) return MHMR_ERR_BAD_SHAPE;
    return L.total;
}

// The stack's backward.  The forward overwrites x in place, so the layers are first re-run by the forward's own layer function, out of
// place, into the tape (the inputs of the three sub-blocks, qkv, q, both attention outputs, the feed-forward's pre-activation Z and gelu(Z));
// kv is recomputed per layer from ctx16 on the way back.
int mhmr_xattn_layers_backward(const mhmr_xattn_backward_desc* d, void* stream) {
    if (!d || d->P < 0 || d->depth < 0) return MHMR_ERR_BAD_ARG;
    if (d->N <= 0) return MHMR_ERR_BAD_SHAPE;
    TRY(stack_shape_rc(d->dim, d->heads, d->mlp, d->Kc, d->B));
    if (d->dtype != MHMR_DT_F16 && d->dtype != MHMR_DT_BF16) return MHMR_ERR_BAD_SHAPE;
    if (d->ngroups < 0 || d->nmax < 0 || d->nchunks < 0) return MHMR_ERR_BAD_ARG;
    if ((d->nmax + 63) / 64 > 65535 || (d->P + 15) / 16 > 65535 || d->ctx_valid < 0 || d->ctx_valid > d->Kc) return MHMR_ERR_BAD_SHAPE;
    StackLayout L;
    if (!stack_layout(d->depth, d->dim, d->heads, d->mlp, d->Kc, d->N, d->B, d->P, &L)) return MHMR_ERR_BAD_SHAPE;
    if (d->g_feat) TRY(feature_grad_shape_rc(d->B, d->N, d->heads, d->Kc, d->feat_cols, d->ld_feat));
    if (d->P == 0) return d->g_feat ? zero_feature_grad(d->g_feat, d->ld_feat, d->B * d->N, d->feat_cols, (hipStream_t)stream) : 0;
    if (d->ngroups == 0 || d->nmax == 0 || d->nchunks == 0) return MHMR_ERR_BAD_ARG;      // persons without groups or without work items
    if (!d->layers || !d->grads || !d->x0 || !d->ctx16 || !d->gstart || !d->chunks || !d->g_x_out || !d->g_x0 || !d->workspace ||
        d->workspace_bytes < L.total || (d->g_ctx && !d->det_row))
        return MHMR_ERR_BAD_ARG;
    for (int l = 0; l < d->depth; ++l) {
        const mhmr_hph_layer& W = d->layers[l];
        const mhmr_hph_layer_grads& G = d->grads[l];
        const void* wp[] = {W.ln_sa_w, W.ln_sa_b, W.to_qkv, W.sa_out_w, W.sa_out_b, W.ln_ca_w, W.ln_ca_b, W.to_kv16, W.to_q, W.ca_out_w,
                            W.ca_out_b, W.ln_ff_w, W.ln_ff_b, W.ff1_w, W.ff1_b, W.ff2_w, W.ff2_b};
        const void* gp[] = {G.ln_sa_w, G.ln_sa_b, G.to_qkv, G.sa_out_w, G.sa_out_b, G.ln_ca_w, G.ln_ca_b, G.to_kv, G.to_q, G.ca_out_w,
                            G.ca_out_b, G.ln_ff_w, G.ln_ff_b, G.ff1_w, G.ff1_b, G.ff2_w, G.ff2_b};
        for (int i = 0; i < 17; ++i)
            if (!wp[i] || !gp[i]) return MHMR_ERR_BAD_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int P = d->P, dim = d->dim, heads = d->heads, mlp = d->mlp, Kc = d->Kc, N = d->N, B = d->B, inner = heads * 32;
    const int rows = B * N;
    char* ws = (char*)d->workspace;
    auto F = [&](long long off) { return (float*)(ws + off); };
    auto xs = [&](int i) { return F(L.xs + (long long)i * L.s_x); };
    float *xn = F(L.xn), *tbig = F(L.t_big), *tin = F(L.t_inner), *kv = F(L.kv), *dkv = F(L.dkv), *lse = F(L.lse);
    void* lnws = ws + L.ln;
    void* ctxws = ws + L.ctx;

    // ---- the forward again, out of place
    const HphStack t{dim, heads, mlp, Kc, N, B, d->dtype, P, d->ctx16, d->gstart, d->ngroups, d->nmax, d->chunks, d->nchunks};
    for (int l = 0; l < d->depth; ++l) {
        const HphLayerBufs b{l == 0 ? d->x0 : xs(3 * l - 1), xs(3 * l), xs(3 * l + 1),
                             l + 1 < d->depth ? xs(3 * l + 2) : nullptr,      // the last layer's output is not needed
                             xn, F(L.qkv + l * L.s_qkv), F(L.o_sa + l * L.s_inner), F(L.q + l * L.s_inner), F(L.o_ca + l * L.s_inner), kv,
                             F(L.h1 + l * L.s_mlp), F(L.z1 + l * L.s_mlp)};
        TRY(mhmr_launch_hph_layer(t, d->layers[l], b, s));
    }

    // ---- and back
    const float* g = d->g_x_out;
    float* gbuf[2] = {F(L.ga), F(L.gb)};
    int gi = 0;
    if (d->depth == 0 && d->g_feat) TRY(zero_feature_grad(d->g_feat, d->ld_feat, rows, d->feat_cols, s));
    if (d->depth == 0) return (int)hipMemcpyAsync(d->g_x0, d->g_x_out, (size_t)P * dim * 4, hipMemcpyDeviceToDevice, s);
    for (int l = d->depth - 1; l >= 0; --l) {
        const mhmr_hph_layer& W = d->layers[l];
        const mhmr_hph_layer_grads& G = d->grads[l];
        const float* x_sa = l == 0 ? d->x0 : xs(3 * l - 1);
        const float *x_ca = xs(3 * l), *x_ff = xs(3 * l + 1);
        const float *qkv = F(L.qkv + l * L.s_qkv), *o_sa = F(L.o_sa + l * L.s_inner), *q = F(L.q + l * L.s_inner), *o_ca = F(L.o_ca + l * L.s_inner);
        const float *z1 = F(L.z1 + l * L.s_mlp), *h1 = F(L.h1 + l * L.s_mlp);
        // feed-forward
        TRY(mhmr_launch_layernorm_f32(x_ff, W.ln_ff_w, W.ln_ff_b, xn, P, dim, HPH_LN_EPS, s));
        TRY(launch_linear_bwd_weight(g, dim, nullptr, 0, h1, mlp, G.ff2_w, mlp, G.ff2_b, P, dim, mlp, MHMR_ACT_NONE, s));
        TRY(launch_linear_bwd_input(g, dim, nullptr, nullptr, 0, W.ff2_w, mlp, nullptr, 0, tbig, mlp, P, dim, mlp, MHMR_ACT_NONE, s));
        TRY(launch_linear_bwd_weight(tbig, mlp, z1, mlp, xn, dim, G.ff1_w, dim, G.ff1_b, P, mlp, dim, MHMR_ACT_GELU, s));
        TRY(launch_linear_bwd_input(tbig, mlp, nullptr, z1, mlp, W.ff1_w, dim, nullptr, 0, xn, dim, P, mlp, dim, MHMR_ACT_GELU, s));
        // (xn is read by the weight side before the input side overwrites it: stream order)
        float* g1 = gbuf[gi]; gi ^= 1;
        TRY(launch_layernorm_bwd(x_ff, W.ln_ff_w, xn, g, g1, G.ln_ff_w, G.ln_ff_b, P, dim, HPH_LN_EPS, lnws, s));
        // cross-attention
        TRY(mhmr_launch_to_kv(t, W, kv, s));
        TRY(mhmr_launch_layernorm_f32(x_ca, W.ln_ca_w, W.ln_ca_b, xn, P, dim, HPH_LN_EPS, s));
        TRY(launch_linear_bwd_weight(g1, dim, nullptr, 0, o_ca, inner, G.ca_out_w, inner, G.ca_out_b, P, dim, inner, MHMR_ACT_NONE, s));
        TRY(launch_linear_bwd_input(g1, dim, nullptr, nullptr, 0, W.ca_out_w, inner, nullptr, 0, tin, inner, P, dim, inner, MHMR_ACT_NONE, s));
        TRY(launch_cross_attn_bwd(q, kv, tin, d->chunks, d->nchunks, tbig, dkv, lse, heads, N, B, s));
        TRY(launch_grad_ctx_gemm(dkv, 2 * inner, d->ctx16, Kc, G.to_kv, rows, 2 * inner, Kc, d->ctx_valid > 0 ? d->ctx_valid : Kc, d->dtype,
                                 ctxws, s));
        if (d->g_feat)       // the dense cotangent of the features, every row: g_feat (+)= dkv . to_kv16[:, :feat_cols], layers in this order
            TRY(launch_dense_ctx_grad(dkv, 2 * inner, W.to_kv16, Kc, d->g_feat, d->ld_feat, rows, 2 * inner, d->feat_cols, l != d->depth - 1,
                                      d->dtype, s));
        if (d->g_ctx) {      // context cotangent at the detected cells: g_ctx[p] (+)= dkv[det_row[p]] . Wkv, layers in this (descending) order
            TRY(launch_op16_to_f32(W.to_kv16, F(L.w32), (size_t)2 * inner * Kc, d->dtype, s));
            TRY(launch_linear_bwd_input(dkv, 2 * inner, d->det_row, nullptr, 0, F(L.w32), Kc, l == d->depth - 1 ? nullptr : d->g_ctx, Kc, d->g_ctx,
                                        Kc, P, 2 * inner, Kc, MHMR_ACT_NONE, s));
        }
        TRY(launch_linear_bwd_weight(tbig, inner, nullptr, 0, xn, dim, G.to_q, dim, nullptr, P, inner, dim, MHMR_ACT_NONE, s));
        TRY(launch_linear_bwd_input(tbig, inner, nullptr, nullptr, 0, W.to_q, dim, nullptr, 0, xn, dim, P, inner, dim, MHMR_ACT_NONE, s));
        float* g2 = gbuf[gi]; gi ^= 1;
        TRY(launch_layernorm_bwd(x_ca, W.ln_ca_w, xn, g1, g2, G.ln_ca_w, G.ln_ca_b, P, dim, HPH_LN_EPS, lnws, s));
        // self-attention
        TRY(mhmr_launch_layernorm_f32(x_sa, W.ln_sa_w, W.ln_sa_b, xn, P, dim, HPH_LN_EPS, s));
        TRY(launch_linear_bwd_weight(g2, dim, nullptr, 0, o_sa, inner, G.sa_out_w, inner, G.sa_out_b, P, dim, inner, MHMR_ACT_NONE, s));
        TRY(launch_linear_bwd_input(g2, dim, nullptr, nullptr, 0, W.sa_out_w, inner, nullptr, 0, tin, inner, P, dim, inner, MHMR_ACT_NONE, s));
        TRY(launch_self_attn_bwd(qkv, tin, d->gstart, tbig, lse, d->ngroups, d->nmax, heads, s));
        TRY(launch_linear_bwd_weight(tbig, 3 * inner, nullptr, 0, xn, dim, G.to_qkv, dim, nullptr, P, 3 * inner, dim, MHMR_ACT_NONE, s));
        TRY(launch_linear_bwd_input(tbig, 3 * inner, nullptr, nullptr, 0, W.to_qkv, dim, nullptr, 0, xn, dim, P, 3 * inner, dim, MHMR_ACT_NONE, s));
        float* g3 = l == 0 ? d->g_x0 : gbuf[gi];
        TRY(launch_layernorm_bwd(x_sa, W.ln_sa_w, xn, g2, g3, G.ln_sa_w, G.ln_sa_b, P, dim, HPH_LN_EPS, lnws, s));
        g = g3;
        // gbuf[gi] now holds g; the next two writes go to the other buffer, then to this one's partner: g1 must not alias g
        gi ^= 1;
    }
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- the whole head: mhmr_hph_forward up to the read-out
namespace {

struct HeadLayout {
    long long x0, gx, gx0, z1, h1, dh, gctx, stack, total;
};

void head_layout(const mhmr_hph_desc* f, int P, HeadLayout* H, long long stack_bytes) {
    WsCursor ws;
    H->x0 = ws.take((long long)P * f->dim * 4);
    H->gx = ws.take((long long)P * f->dim * 4);
    H->gx0 = ws.take((long long)P * f->dim * 4);
    H->z1 = ws.take((long long)P * f->C * 4);
    H->h1 = ws.take((long long)P * f->C * 4);
    H->dh = ws.take((long long)P * f->C * 4);
    H->gctx = ws.take((long long)P * f->Kc * 4);
    H->stack = ws.take(stack_bytes);
    H->total = ws.at;
}

int head_shape_rc(const mhmr_hph_desc* f, int B) {
    if (!mhmr_hph_head_shape_ok(f) || f->C <= 0 || f->G <= 0 || f->N <= 0 || f->Ndec != 318 + f->nb + 13) return MHMR_ERR_BAD_SHAPE;
    const int E = f->cam_dim > 0 ? f->cam_dim : 99;
    if (E < 3 || f->C + E > f->Kc || f->C + E + 318 + f->nb + 3 > f->Ktok) return MHMR_ERR_BAD_SHAPE;
    return stack_shape_rc(f->dim, f->heads, f->mlp, f->Kc, B);
}

}  // namespace

extern "C" {

long long mhmr_hph_backward_workspace_bytes(const mhmr_hph_desc* f, int B, int P) {
    if (!f || P < 0 || f->depth < 0) return MHMR_ERR_BAD_ARG;
    const int rc = head_shape_rc(f, B);
    if (rc) return rc;
    const long long sb = mhmr_xattn_layers_backward_workspace_bytes(f->depth, f->dim, f->heads, f->mlp, f->Kc, f->N, B, P);
    if (sb < 0) return sb;
    HeadLayout H;
    head_layout(f, P, &H, sb);
    return H.total;
}

// Order: dec linear, the stack (which also sums the context cotangent of the detected cells over the layers), the token embedding, the
// four tables, mlp_offset.  The forward left zc, token and x (the stack's OUTPUT) in the descriptor's workspaces; the stack's input x0 and
// the mlp_offset hidden layer are recomputed with the forward's launcher.
int mhmr_hph_backward(const mhmr_hph_backward_desc* d, void* stream) {
    if (!d || !d->fwd || d->P < 0 || d->fwd->depth < 0) return MHMR_ERR_BAD_ARG;
    const mhmr_hph_desc* f = d->fwd;
    TRY(head_shape_rc(f, d->B));
    if (f->dtype != MHMR_DT_F16 && f->dtype != MHMR_DT_BF16) return MHMR_ERR_BAD_SHAPE;
    if (d->ngroups < 0 || d->nmax < 0 || d->nchunks < 0) return MHMR_ERR_BAD_ARG;
    if (d->ldg < f->Ndec || (d->nmax + 63) / 64 > 65535 || (d->P + 15) / 16 > 65535) return MHMR_ERR_BAD_SHAPE;
    const long long need = mhmr_hph_backward_workspace_bytes(f, d->B, d->P);
    if (need < 0) return (int)need;
    if (d->g_feat) TRY(feature_grad_shape_rc(d->B, f->N, f->heads, f->Kc, f->C, d->ld_feat));
    if (d->P == 0) return d->g_feat ? zero_feature_grad(d->g_feat, d->ld_feat, d->B * f->N, f->C, (hipStream_t)stream) : 0;
    if (d->ngroups == 0 || d->nmax == 0 || d->nchunks == 0) return MHMR_ERR_BAD_ARG;      // persons without groups or without work items
    const void* req[] = {f->off1_w, f->off1_b, f->off2_w, f->off2_b, f->tok_w, f->tok_b, f->layers, f->dec_w, f->zc, f->token, f->x, f->det_row,
                         d->ctx16, d->det_y, d->det_x, d->gstart, d->chunks, d->g_readout, d->g_offset, d->g_off1_w, d->g_off1_b, d->g_off2_w,
                         d->g_off2_b, d->g_tok_w, d->g_tok_b, d->g_dec_w, d->g_dec_b, d->g_cq_x, d->g_cq_y, d->g_cv_x, d->g_cv_y, d->layer_grads,
                         d->g_zc, d->g_token, d->workspace};
    for (const void* p : req)
        if (!p) return MHMR_ERR_BAD_ARG;
    if (d->workspace_bytes < need) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int P = d->P, C = f->C, dim = f->dim, Ktok = f->Ktok, Kc = f->Kc, Ndec = f->Ndec, G = f->G;
    const int E = f->cam_dim > 0 ? f->cam_dim : 99, Cc = C + E;
    HeadLayout H;
    head_layout(f, P, &H, mhmr_xattn_layers_backward_workspace_bytes(f->depth, dim, f->heads, f->mlp, Kc, f->N, d->B, P));
    char* ws = (char*)d->workspace;
    auto F = [&](long long off) { return (float*)(ws + off); };
    float *x0 = F(H.x0), *gx = F(H.gx), *gx0 = F(H.gx0), *z1 = F(H.z1), *h1 = F(H.h1), *dh = F(H.dh), *gctx = F(H.gctx);

    // read-out linear
    TRY(launch_linear_bwd_weight(d->g_readout, d->ldg, nullptr, 0, f->x, dim, d->g_dec_w, dim, d->g_dec_b, P, Ndec, dim, MHMR_ACT_NONE, s));
    TRY(launch_linear_bwd_input(d->g_readout, d->ldg, nullptr, nullptr, 0, f->dec_w, dim, nullptr, 0, gx, dim, P, Ndec, dim, MHMR_ACT_NONE, s));
    // the stack, from its recomputed input
    TRY(mhmr_launch_linear_f32(f->token, Ktok, nullptr, f->tok_w, Ktok, f->tok_b, nullptr, 0, x0, dim, P, dim, Ktok, MHMR_ACT_NONE, s));
    mhmr_xattn_backward_desc sd;
    sd.layers = f->layers; sd.grads = d->layer_grads;
    sd.depth = f->depth; sd.dim = dim; sd.heads = f->heads; sd.mlp = f->mlp; sd.Kc = Kc; sd.N = f->N; sd.B = d->B; sd.dtype = f->dtype;
    sd.P = P; sd.ngroups = d->ngroups; sd.nmax = d->nmax; sd.nchunks = d->nchunks; sd.ctx_valid = Cc;
    sd.x0 = x0; sd.ctx16 = d->ctx16; sd.gstart = d->gstart; sd.chunks = d->chunks; sd.g_x_out = gx; sd.g_x0 = gx0;
    sd.det_row = f->det_row; sd.g_ctx = gctx;
    sd.g_feat = d->g_feat; sd.ld_feat = d->ld_feat; sd.feat_cols = C;
    sd.workspace = ws + H.stack; sd.workspace_bytes = d->workspace_bytes - H.stack;
    TRY(mhmr_xattn_layers_backward(&sd, stream));
    if (f->depth == 0) TRY((int)hipMemsetAsync(gctx, 0, (size_t)P * Kc * 4, s));
    // token embedding (the bias gradient is also pos_embedding[0, 0]'s); token's padding columns are zeros, so are g_tok_w's
    TRY(launch_linear_bwd_weight(gx0, dim, nullptr, 0, f->token, Ktok, d->g_tok_w, Ktok, d->g_tok_b, P, dim, Ktok, MHMR_ACT_NONE, s));
    TRY(launch_linear_bwd_input(gx0, dim, nullptr, nullptr, 0, f->tok_w, Ktok, nullptr, 0, d->g_token, Ktok, P, dim, Ktok, MHMR_ACT_NONE, s));
    // the four tables
    TRY(launch_table_grads(d->g_token, Ktok, gctx, Kc, d->det_y, d->det_x, d->g_cq_x, d->g_cq_y, d->g_cv_x, d->g_cv_y, P, G, Cc, s));
    // mlp_offset
    TRY(mhmr_launch_linear_f32(f->zc, C, nullptr, f->off1_w, C, f->off1_b, nullptr, 0, z1, C, P, C, C, MHMR_ACT_NONE, s));
    TRY(mhmr_launch_linear_f32(f->zc, C, nullptr, f->off1_w, C, f->off1_b, nullptr, 0, h1, C, P, C, C, MHMR_ACT_RELU, s));
    TRY(launch_linear_bwd_weight(d->g_offset, 2, nullptr, 0, h1, C, d->g_off2_w, C, d->g_off2_b, P, 2, C, MHMR_ACT_NONE, s));
    TRY(launch_linear_bwd_input(d->g_offset, 2, nullptr, nullptr, 0, f->off2_w, C, nullptr, 0, dh, C, P, 2, C, MHMR_ACT_NONE, s));
    TRY(launch_linear_bwd_weight(dh, C, z1, C, f->zc, C, d->g_off1_w, C, d->g_off1_b, P, C, C, MHMR_ACT_RELU, s));
    TRY(launch_linear_bwd_input(dh, C, nullptr, z1, C, f->off1_w, C, nullptr, 0, d->g_zc, C, P, C, C, MHMR_ACT_RELU, s));
    // the persons' own rows of the feature cotangent, on top of the dense term the stack has written
    if (d->g_feat) TRY(launch_person_rows_add(d->g_zc, d->g_token, Ktok, f->det_row, d->g_feat, d->ld_feat, d->B * f->N, C, P, s));
    return 0;
}

}  // extern "C"
