// The exact-fp32 attention over all tokens of an image: the forward of the "f16x3" precision mode and, for training
// (DESIGN.md section 28), the tape and the backward.  Every product runs on v_mfma_f32_16x16x4_f32 -- exact fp32 multiply-adds, the f32
// VECTOR rate (157 TF/s dense): ~1/16 of the 16-bit kernel's rate, which is what the f16x3 mode costs (a checkpoint whose softmax logits
// are too steep for 16-bit Q / K / P, pack-time statistic vit.logit_gain).
//
//   qkv   [B*Tp, 3C] fp32 = (Q | K | V) rows as the QKV linear leaves them (bias included, NOT scaled); head h = columns h*64 .. +63
//   out   op16 PAIR [B*Tp, 2C]: column h*64 + d holds hi = op16(o), column C + h*64 + d holds lo = op16(o - hi): the A operand of the
//         three-product output projection (GemmArgs::a_k with K = 3 a_k)
//
// One wave = 16 queries, one workgroup = 4 waves = 64 consecutive query rows of one (image, head); keys in tiles of 16, K / V rows read
// straight from global memory into MFMA operand registers (the four waves of a workgroup and the workgroups of a head share them
// through L1 / L2; no LDS).  Fragment geometry (c = lane & 15, g = lane >> 4):
//   S^T = K Q^T   A = K  [key c ][d = 16 g + s]   B = Q^T [d = 16 g + s][query c]   s = 0..15      (any d order is a dot product)
//                 D: lane holds S^T[key 4 g + i][query c], i = 0..3            -> a lane owns ONE query, four of the tile's keys
//   O^T = V^T P^T A = V^T[d = 4 c + db][key 4 g + i]   B = P^T[key 4 g + i][query c] = the lane's own p_i     (i = 0..3, db = 0..3)
//                 D: lane holds O^T[d = 4 (4 g + i') + db][query c]            -> 16 consecutive d of one query per lane
// Online softmax in the exp2 domain; the row maximum / row sum of a query close over its four lanes with two lane exchanges.
//
// The tape kernel is the forward kernel with an fp32 output and the per-query log-sum lse = max + log2(sum) of the exp2-domain logits
// s = (q MHMR_ATTN_QSCALE) . k: both run attn_key_tile on every tile of keys, so they form the same fp32 o and sum from the same chain.
//
// The backward is two passes, so that no sum crosses a workgroup; in both one wave owns 16 rows of one (image, head), a workgroup is
// 4 waves = 64 consecutive rows, the other side streams past in tiles of 16 straight from global memory, as in the forward:
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
// Rules of the training kernels (DESIGN.md sections 17-22): sums that cross rows are fp32 MFMA chains of a shape fixed by the sizes alone;
// no floating-point atomics; every element of every output is written; results are bit-reproducible call to call.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "row_sums.h"

namespace {

constexpr float ATTN_SCALE = 0.125f;                       // head_dim^-0.5 for head_dim = 64

__device__ __forceinline__ void load16(const float* p, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x4 t = *(const f32x4*)(p + 4 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * j + e] = t[e];
    }
}

// the 16-step chain over a lane's sixteen d of two [16 rows][64 d] fragments: D[A row 4 g + i][B row c]
__device__ __forceinline__ f32x4 dot16(const float (&a)[16], const float (&b)[16]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 16; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
    return acc;
}

// One tile of 16 keys of the online softmax, for the forward and the tape alike: kf = K[key0 + c][16 g ..], vf[i] = V[key0 + 4 g + i][4 c ..],
// qf the lane's scaled Q fragment; o, m_run, l_run the running O^T, maximum and (per lane, not yet closed over the query's four) sum.
__device__ __forceinline__ void attn_key_tile(const float (&kf)[16], const f32x4 (&vf)[4], const float (&qf)[16], int key0, int T, int g,
                                              f32x4 (&o)[4], float& m_run, float& l_run) {
    f32x4 s = dot16(kf, qf);
    // keys >= T (the tail of the last tile) are masked
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

// ------------------------------------------------------------------------------------------------------------ forward (f16x3 mode)
template <int DT>
__global__ __launch_bounds__(256) void attn_f32_kernel(const float* __restrict__ qkv, void* __restrict__ out_, int T, int Tp, int C) {
    typedef typename Op<DT>::T Tt;
    typedef typename Op<DT>::V8 V8;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * 64 + 16 * w;                 // the wave's first query row inside the image
    const size_t ld = 3 * (size_t)C;
    const float* img = qkv + (size_t)b * Tp * ld + (size_t)h * 64;
    Tt* orow = (Tt*)out_ + ((size_t)b * Tp + q0 + c) * (size_t)(2 * C) + h * 64 + 16 * g;

    if (q0 >= T) {            // sixteen padding rows: zeros (no dependence on how the caller allocated `out`)
        V8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (Tt)0.f;
        *(V8*)orow = z; *(V8*)(orow + 8) = z; *(V8*)(orow + C) = z; *(V8*)(orow + C + 8) = z;
        return;
    }

    // Q fragment, pre-scaled by head_dim^-0.5 * log2(e) in fp32
    float qf[16];
    load16(img + (size_t)(q0 + c) * ld + 16 * g, qf);
#pragma unroll
    for (int s = 0; s < 16; ++s) qf[s] *= MHMR_ATTN_QSCALE;
    const float* kbase = img + C + (size_t)c * ld + 16 * g;             // K[key0 + c][16 g ..]
    const float* vbase = img + 2 * C + (size_t)(4 * g) * ld + 4 * c;    // V[key0 + 4 g + i][4 c ..]

    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    const int ntile = (T + 15) >> 4;
    float kn[16];
    load16(kbase, kn);
    for (int t = 0; t < ntile; ++t) {
        const int key0 = 16 * t;
        float kf[16];
        f32x4 vf[4];
#pragma unroll
        for (int e = 0; e < 16; ++e) kf[e] = kn[e];
#pragma unroll
        for (int i = 0; i < 4; ++i) vf[i] = *(const f32x4*)(vbase + (size_t)(key0 + i) * ld);
        // next tile's K rows (the last iteration re-reads its own: rows < Tp either way)
        load16(kbase + (size_t)(t + 1 < ntile ? key0 + 16 : key0) * ld, kn);
        attn_key_tile(kf, vf, qf, key0, T, g, o, m_run, l_run);
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_run;
    // lane (c, g): query q0 + c, d = 16 g + 4 i' + db  (o[db][i'])
    V8 hi[2], lo[2];
#pragma unroll
    for (int ip = 0; ip < 4; ++ip)
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            // v is ONE fp32 number, opaque to the optimiser.  Left to fold the product into the conversions, the f16 build measured lo against
            // op16 of the UNROUNDED product (v_fma_mixlo_f16) but stored op16 of the rounded one (v_cvt_pk_f16_f32): where fl32(o * inv) fell
            // exactly between two f16 values the two differed by an ulp, and hi + lo was off by 2^-11 relative -- one weight in ~10^4
            // (tests/test_gpu_attention_keys.py; `#pragma clang fp contract(off)` does not stop that fold)
            float v = o[db][ip] * inv;
            asm volatile("" : "+v"(v));
            const int j = 4 * ip + db;
            const Tt hv = (Tt)v;
            hi[j >> 3][j & 7] = hv;
            lo[j >> 3][j & 7] = (Tt)(v - (float)hv);
        }
    *(V8*)orow = hi[0]; *(V8*)(orow + 8) = hi[1];
    *(V8*)(orow + C) = lo[0]; *(V8*)(orow + C + 8) = lo[1];
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
        attn_key_tile(kf, vf, qf, key0, T, g, o, m_run, l_run);
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
        const f32x4 s = dot16(kf, qf), dp = dot16(vf, dof);
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
        const f32x4 s = dot16(kf, qf), dp = dot16(vf, dof);
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
        const f32x4 s = dot16(qa, kf), dp = dot16(da, vf);
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

// the backward's workspace: D | r, [B, H, Tp] fp32 each
inline long long attn_stat_bytes(int B, int Tp, int H) { return align256((long long)B * H * Tp * (long long)sizeof(float)); }

}  // namespace

int mhmr_launch_attention_f32(const float* qkv, void* out, int B, int T, int Tp, int C, int H, int dtype, hipStream_t s) {
    if (B <= 0 || T <= 0 || Tp % 64 || Tp < T || C != 64 * H) return MHMR_ERR_BAD_SHAPE;
    const dim3 grid(Tp / 64, H, B);
    prof_begin(PROF_ATTN, s);
    if (dtype == MHMR_DT_F16) hipLaunchKernelGGL((attn_f32_kernel<MHMR_DT_F16>), grid, dim3(256), 0, s, qkv, out, T, Tp, C);
    else hipLaunchKernelGGL((attn_f32_kernel<MHMR_DT_BF16>), grid, dim3(256), 0, s, qkv, out, T, Tp, C);
    prof_end(PROF_ATTN, s, 4.0 * B * H * (double)T * T * 64);
    MHMR_CHECK_LAUNCH();
    return 0;
}

long long mhmr_attention_f32_bwd_bytes(int B, int Tp, int C) { return 2 * attn_stat_bytes(B, Tp, C / 64); }

int mhmr_launch_attention_f32_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, hipStream_t s) {
    hipLaunchKernelGGL(attn_tape_kernel, dim3(Tp / 64, H, B), dim3(256), 0, s, qkv, out32, lse, T, Tp, C, H);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int mhmr_launch_attention_f32_bwd(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                  int Tp, int C, int H, void* ws, hipStream_t s) {
    const dim3 grid(Tp / 64, H, B);
    float *Dws = (float*)ws, *Rws = (float*)((char*)ws + attn_stat_bytes(B, Tp, H));
    hipLaunchKernelGGL(attn_bwd_q_kernel, grid, dim3(256), 0, s, qkv, lse, dO, lddo, dqkv, Dws, Rws, T, Tp, C, H);
    hipLaunchKernelGGL(attn_bwd_kv_kernel, grid, dim3(256), 0, s, qkv, lse, dO, lddo, dqkv, (const float*)Dws, (const float*)Rws, T, Tp, C, H);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" {

int mhmr_attention_f32_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* stream) {
    TRY(mhmr_attention_shape_rc(B, T, Tp, C, H));
    if (!qkv || !out32 || !lse || !aligned16(qkv) || !aligned16(out32)) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_attention_f32_tape(qkv, out32, lse, B, T, Tp, C, H, (hipStream_t)stream);
}

long long mhmr_attention_f32_backward_workspace_bytes(int B, int Tp, int H) {
    if (B < 0 || Tp < 0 || H < 0) return MHMR_ERR_BAD_ARG;
    if (B == 0 || Tp == 0 || H == 0 || Tp % 64 || H > 65535 || B > 65535) return MHMR_ERR_BAD_SHAPE;
    return 2 * attn_stat_bytes(B, Tp, H);
}

int mhmr_attention_f32_backward(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                int Tp, int C, int H, void* workspace, long long workspace_bytes, void* stream) {
    TRY(mhmr_attention_shape_rc(B, T, Tp, C, H));
    if (lddo < C || lddo % 4) return MHMR_ERR_BAD_SHAPE;
    if (!qkv || !out32 || !lse || !dO || !dqkv || !workspace || workspace_bytes < 2 * attn_stat_bytes(B, Tp, H)) return MHMR_ERR_BAD_ARG;
    if (!aligned16(qkv) || !aligned16(out32) || !aligned16(lse) || !aligned16(dO) || !aligned16(dqkv) || !aligned16(workspace))
        return MHMR_ERR_BAD_ARG;
    return mhmr_launch_attention_f32_bwd(qkv, out32, lse, dO, lddo, dqkv, B, T, Tp, C, H, workspace, (hipStream_t)stream);
}

}  // extern "C"
