// Attention tape and backward with bf16 operands and fp32 accumulation: the mixed-precision form of
// attention_f32.hip's tape and backward.  Every tensor at the interface is fp32 in the layouts of mhmr_attention_f32_tape / _backward;
// r() is round-to-nearest-even fp32 -> bf16.  Per (image, head), over the T real rows:
//     S_ij  = MHMR_ATTN_QSCALE * sum_d r(Q_i[d]) r(K_j[d])        lse_i = log2 sum_j exp2(S_ij)        P_ij = exp2(S_ij - lse_i)
//     O_i   = sum_j r(P_ij) r(V_j)                                D_i   = sum_d dO_i[d] O_i[d]  (unrounded, fp32, fixed order)
//     dP_ij = sum_d r(dO_i[d]) r(V_j[d])                          dS_ij = P_ij (dP_ij - D_i)
//     dV_j  = sum_i r(P_ij) r(dO_i)      dQ_i = 0.125 sum_j r(dS_ij) r(K_j)      dK_j = 0.125 sum_i r(dS_ij) r(Q_i)
// The rounded probability is the NORMALISED one, a function of the inputs alone: the tape sweeps the keys twice (S and the online
// log-sum first; S again, r(exp2(S - lse)) and the product with V second; no final division), and the backward recomputes S by the
// same products in the same order and uses the tape's lse.  S itself is never rounded.
//
// Operands.  Convert kernels (linear_bf16.hip's) write bf16 copies into the workspace once per call, each in the layouts that make
// every product contiguous along its summed index: qkv as it lies [B*Tp, 3C], dO [B*Tp, C], and transposed [C, B*Tp] copies of V (tape),
// K (query pass), Q and dO (key pass).
//
// Three MFMA kernels on v_mfma_f32_16x16x32_bf16, no sum crosses a workgroup, nothing is atomic.  A workgroup = 4 waves owns 64
// consecutive rows of one (image, head), a wave 16 of them; the other side streams past in tiles of 64 rows staged through LDS (144-byte
// row pitch; the next tile's global loads are issued before the current tile's MFMAs).  With c = lane & 15, g = lane >> 4:
//   scores      A = streamed tile [row 16 a + c][d = 32 ks + 8 g ..]    B = the wave's own rows [d = 32 ks + 8 g ..][row c]
//               D: lane holds [streamed row 16 a + 4 g + r][own row c], a = 0..3, r = 0..3: a lane owns ONE of its wave's rows
//   products    with P / dS: the lane's own sixteen values are the B operand of the next MFMA without leaving their registers.  The
//               MFMA's summed index 8 g + e of the 32-row group G stands for the streamed row 32 G + 4 g + e (e < 4) or
//               32 G + 16 + 4 g + e - 4 (e >= 4) -- a permutation of the summed index is still the dot product -- and the A operand
//               [d = 16 db + c][streamed rows] is read from the transposed tile as two 8-byte pieces in that same order.
//               D: lane holds [d = 16 db + 4 g + r][own row c]: four consecutive d of one row, stored as 16 bytes.
// A column of an MFMA result depends on that column of B alone, so an own row >= T (any finite values) reaches no real row and is
// stored as zeros; a streamed row >= T contributes a P / dS of exact zero.  (Finite means finite as bf16: below 3.39e38.)
// Accumulation order: ascending streamed tiles, fixed by (T, Tp) alone.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "row_sums.h"

namespace {

constexpr int TR = 64;                     // rows per tile, own and streamed
constexpr int LDT = 64 + 8;                // LDS row pitch in elements: 144 bytes
constexpr float ATTN_SCALE = 0.125f;       // head_dim^-0.5 for head_dim = 64

// a 64 x 64 bf16 tile is 512 pieces of 16 bytes; thread t moves pieces t and t + 256: row (t >> 3) + 32 e, elements 8 (t & 7) ..
__device__ __forceinline__ void tile_load(const __bf16* __restrict__ base, size_t pitch, int t, bf16x8 (&r)[2]) {
#pragma unroll
    for (int e = 0; e < 2; ++e) r[e] = *(const bf16x8*)(base + (size_t)((t >> 3) + 32 * e) * pitch + (t & 7) * 8);
}
__device__ __forceinline__ void tile_store(__bf16* s, int t, const bf16x8 (&r)[2]) {
#pragma unroll
    for (int e = 0; e < 2; ++e) *(bf16x8*)(s + ((t >> 3) + 32 * e) * LDT + (t & 7) * 8) = r[e];
}

// s[a][r] = sum_d tile[16 a + 4 g + r][d] own[c][d]
__device__ __forceinline__ void scores(const __bf16* tile, const bf16x8 (&own)[2], int c, int g, f32x4 (&s)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) s[a] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bf16x8 f = *(const bf16x8*)(tile + (16 * a + c) * LDT + 32 * ks + 8 * g);
            s[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, own[ks], s[a], 0, 0, 0);
        }
}

// acc[db][r] += sum over the tile's rows j of tileT[16 db + 4 g + r][j] w[j], the lane's w in pb (header: the summed-index order)
__device__ __forceinline__ void weighted(const __bf16* tileT, const bf16x8 (&pb)[2], int c, int g, f32x4 (&acc)[4]) {
#pragma unroll
    for (int G = 0; G < 2; ++G)
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const __bf16* p = tileT + (16 * db + c) * LDT + 32 * G + 4 * g;
            const bf16x4 lo = *(const bf16x4*)p, hi = *(const bf16x4*)(p + 16);
            const bf16x8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f, pb[G], acc[db], 0, 0, 0);
        }
}

// the lane's value of streamed row 16 a + 4 g + r goes to element 4 (a & 1) + r of group a >> 1
__device__ __forceinline__ void put(bf16x8 (&pb)[2], int a, int r, float v) { pb[a >> 1][4 * (a & 1) + r] = (__bf16)v; }

// ------------------------------------------------------------------------------------------------------------ tape
// grid (Tp / 64, H, B).  qkvb [M, 3C] bf16, vt [C, M] bf16 (M = B Tp)
__global__ __launch_bounds__(256, 2) void attn16_tape_kernel(const __bf16* __restrict__ qkvb, const __bf16* __restrict__ vt, float* __restrict__ out,
                                                             float* __restrict__ lse, int T, int Tp, int C, int H, size_t M) {
    __shared__ __attribute__((aligned(16))) __bf16 sK[TR * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 sV[TR * LDT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, r0 = blockIdx.x * TR;
    const size_t ld = 3 * (size_t)C, rowbase = (size_t)b * Tp;
    const int q = r0 + 16 * w + c;                                          // the lane's query row inside the image
    float* orow = out + (rowbase + q) * (size_t)C + h * 64 + 4 * g;
    float* lrow = lse + ((size_t)b * H + h) * Tp + q;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (r0 >= T) {            // sixty-four padding rows
#pragma unroll
        for (int db = 0; db < 4; ++db) *(f32x4*)(orow + 16 * db) = zero;
        if (g == 0) *lrow = 0.f;
        return;
    }
    bf16x8 qf[2];
    {
        const __bf16* qp = qkvb + (rowbase + q) * ld + h * 64 + 8 * g;
        qf[0] = *(const bf16x8*)qp;
        qf[1] = *(const bf16x8*)(qp + 32);
    }
    const __bf16* kbase = qkvb + rowbase * ld + C + h * 64;                 // K rows of the image, pitch ld
    const __bf16* vtbase = vt + (size_t)(h * 64) * M + rowbase;             // V^T rows d of the head, pitch M
    const int ntile = (T + TR - 1) / TR;

    // first sweep: the log-sum of the query's logits (online maximum)
    bf16x8 rk[2], rv[2];
    tile_load(kbase, ld, t, rk);
    float m_run = -INFINITY, l_run = 0.f;
    for (int tile = 0; tile < ntile; ++tile) {
        tile_store(sK, t, rk);
        __syncthreads();
        if (tile + 1 < ntile) tile_load(kbase + (size_t)(tile + 1) * TR * ld, ld, t, rk);
        f32x4 s[4];
        scores(sK, qf, c, g, s);
        float mx = -INFINITY;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = tile * TR + 16 * a + 4 * g + r < T ? s[a][r] * MHMR_ATTN_QSCALE : -INFINITY;      // keys >= T are masked
                s[a][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);                  // finite from tile 0 on (key 0 is real)
        float ps = 0.f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) ps += __builtin_amdgcn_exp2f(s[a][r] - m_new);
        l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + ps;
        m_run = m_new;
        __syncthreads();
    }
    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    const float lq = m_run + log2f(l_run);

    // second sweep: O = r(exp2(S - lse)) r(V)
    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = zero;
    tile_load(kbase, ld, t, rk);
    tile_load(vtbase, M, t, rv);
    for (int tile = 0; tile < ntile; ++tile) {
        tile_store(sK, t, rk);
        tile_store(sV, t, rv);
        __syncthreads();
        if (tile + 1 < ntile) {
            tile_load(kbase + (size_t)(tile + 1) * TR * ld, ld, t, rk);
            tile_load(vtbase + (size_t)(tile + 1) * TR, M, t, rv);
        }
        f32x4 s[4];
        scores(sK, qf, c, g, s);
        bf16x8 pb[2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[a][r] * MHMR_ATTN_QSCALE - lq);
                put(pb, a, r, tile * TR + 16 * a + 4 * g + r < T ? p : 0.f);
            }
        weighted(sV, pb, c, g, o);
        __syncthreads();
    }
    const bool real = q < T;
#pragma unroll
    for (int db = 0; db < 4; ++db) *(f32x4*)(orow + 16 * db) = real ? o[db] : zero;
    if (g == 0) *lrow = real ? lq : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ D = rowsum(dO . O)
// sixteen lanes per (row, head): four products each in index order, then the xor butterfly; rows >= T: zero
__global__ __launch_bounds__(256) void attn16_rowdot_kernel(const float* __restrict__ dO, int lddo, const float* __restrict__ out32,
                                                            float* __restrict__ D, size_t n, int T, int Tp, int C, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;                                       // n is a multiple of 16: the sixteen lanes of a sum leave together
    const int sub = (int)(i & 15);
    const size_t pair = i >> 4, row = pair / (size_t)H;
    const int h = (int)(pair - row * (size_t)H);
    const size_t b = row / (size_t)Tp;
    const int tok = (int)(row - b * (size_t)Tp);
    const f32x4 a = *(const f32x4*)(dO + row * (size_t)lddo + h * 64 + 4 * sub);
    const f32x4 o = *(const f32x4*)(out32 + row * (size_t)C + h * 64 + 4 * sub);
    float v = a[0] * o[0];
    v = __builtin_fmaf(a[1], o[1], v);
    v = __builtin_fmaf(a[2], o[2], v);
    v = __builtin_fmaf(a[3], o[3], v);
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off);
    if (sub == 0) D[(b * H + h) * (size_t)Tp + tok] = tok < T ? v : 0.f;
}

// ------------------------------------------------------------------------------------------------------------ backward, query pass
// dob [M, C] bf16, kt [C, M] bf16
__global__ __launch_bounds__(256, 2) void attn16_bwd_q_kernel(const __bf16* __restrict__ qkvb, const __bf16* __restrict__ dob,
                                                              const __bf16* __restrict__ kt, const float* __restrict__ lse,
                                                              const float* __restrict__ Dws, float* __restrict__ dqkv, int T, int Tp, int C, int H,
                                                              size_t M) {
    __shared__ __attribute__((aligned(16))) __bf16 sK[TR * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 sV[TR * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 sKT[TR * LDT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, r0 = blockIdx.x * TR;
    const size_t ld = 3 * (size_t)C, rowbase = (size_t)b * Tp;
    const int q = r0 + 16 * w + c;
    float* dqrow = dqkv + (rowbase + q) * ld + h * 64 + 4 * g;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (r0 >= T) {
#pragma unroll
        for (int db = 0; db < 4; ++db) *(f32x4*)(dqrow + 16 * db) = zero;
        return;
    }
    bf16x8 qf[2], dof[2];
    {
        const __bf16* qp = qkvb + (rowbase + q) * ld + h * 64 + 8 * g;
        const __bf16* gp = dob + (rowbase + q) * (size_t)C + h * 64 + 8 * g;
        qf[0] = *(const bf16x8*)qp;
        qf[1] = *(const bf16x8*)(qp + 32);
        dof[0] = *(const bf16x8*)gp;
        dof[1] = *(const bf16x8*)(gp + 32);
    }
    const size_t stat = ((size_t)b * H + h) * Tp + q;
    const float lq = lse[stat], Dq = Dws[stat];
    const __bf16* kbase = qkvb + rowbase * ld + C + h * 64;
    const __bf16* vbase = kbase + C;
    const __bf16* ktbase = kt + (size_t)(h * 64) * M + rowbase;
    const int ntile = (T + TR - 1) / TR;

    f32x4 dq[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) dq[db] = zero;
    bf16x8 rk[2], rv[2], rt[2];
    tile_load(kbase, ld, t, rk);
    tile_load(vbase, ld, t, rv);
    tile_load(ktbase, M, t, rt);
    for (int tile = 0; tile < ntile; ++tile) {
        tile_store(sK, t, rk);
        tile_store(sV, t, rv);
        tile_store(sKT, t, rt);
        __syncthreads();
        if (tile + 1 < ntile) {
            tile_load(kbase + (size_t)(tile + 1) * TR * ld, ld, t, rk);
            tile_load(vbase + (size_t)(tile + 1) * TR * ld, ld, t, rv);
            tile_load(ktbase + (size_t)(tile + 1) * TR, M, t, rt);
        }
        f32x4 s[4], dp[4];
        scores(sK, qf, c, g, s);
        scores(sV, dof, c, g, dp);
        bf16x8 dsb[2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[a][r] * MHMR_ATTN_QSCALE - lq);
                put(dsb, a, r, tile * TR + 16 * a + 4 * g + r < T ? p * (dp[a][r] - Dq) : 0.f);      // keys >= T are masked
            }
        weighted(sKT, dsb, c, g, dq);
        __syncthreads();
    }
    const bool real = q < T;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = real ? dq[db][r] * ATTN_SCALE : 0.f;
        *(f32x4*)(dqrow + 16 * db) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ backward, key pass
// qt, gt [C, M] bf16: Q^T and dO^T
__global__ __launch_bounds__(256, 2) void attn16_bwd_kv_kernel(const __bf16* __restrict__ qkvb, const __bf16* __restrict__ dob,
                                                               const __bf16* __restrict__ qt, const __bf16* __restrict__ gt,
                                                               const float* __restrict__ lse, const float* __restrict__ Dws,
                                                               float* __restrict__ dqkv, int T, int Tp, int C, int H, size_t M) {
    __shared__ __attribute__((aligned(16))) __bf16 sQ[TR * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 sG[TR * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 sQT[TR * LDT];
    __shared__ __attribute__((aligned(16))) __bf16 sGT[TR * LDT];
    __shared__ __attribute__((aligned(16))) float sL[TR];
    __shared__ __attribute__((aligned(16))) float sD[TR];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, r0 = blockIdx.x * TR;
    const size_t ld = 3 * (size_t)C, rowbase = (size_t)b * Tp;
    const int k = r0 + 16 * w + c;                                          // the lane's key row inside the image
    float* dkrow = dqkv + (rowbase + k) * ld + C + h * 64 + 4 * g;
    float* dvrow = dkrow + C;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (r0 >= T) {
#pragma unroll
        for (int db = 0; db < 4; ++db) { *(f32x4*)(dkrow + 16 * db) = zero; *(f32x4*)(dvrow + 16 * db) = zero; }
        return;
    }
    bf16x8 kf[2], vf[2];
    {
        const __bf16* kp = qkvb + (rowbase + k) * ld + C + h * 64 + 8 * g;
        kf[0] = *(const bf16x8*)kp;
        kf[1] = *(const bf16x8*)(kp + 32);
        vf[0] = *(const bf16x8*)(kp + C);
        vf[1] = *(const bf16x8*)(kp + C + 32);
    }
    const __bf16* qbase = qkvb + rowbase * ld + h * 64;
    const __bf16* gbase = dob + rowbase * (size_t)C + h * 64;
    const __bf16* qtbase = qt + (size_t)(h * 64) * M + rowbase;
    const __bf16* gtbase = gt + (size_t)(h * 64) * M + rowbase;
    // threads 0 .. 63 carry the tile's lse, 64 .. 127 its D
    const float* stbase = (t < 64 ? lse : Dws) + ((size_t)b * H + h) * Tp + (t & 63);
    const int ntile = (T + TR - 1) / TR;

    f32x4 dk[4], dv[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) dk[db] = dv[db] = zero;
    bf16x8 rq[2], rg[2], rqt[2], rgt[2];
    float rs = 0.f;
    tile_load(qbase, ld, t, rq);
    tile_load(gbase, (size_t)C, t, rg);
    tile_load(qtbase, M, t, rqt);
    tile_load(gtbase, M, t, rgt);
    if (t < 128) rs = *stbase;
    for (int tile = 0; tile < ntile; ++tile) {
        tile_store(sQ, t, rq);
        tile_store(sG, t, rg);
        tile_store(sQT, t, rqt);
        tile_store(sGT, t, rgt);
        if (t < 64) sL[t] = rs;
        else if (t < 128) sD[t - 64] = rs;
        __syncthreads();
        if (tile + 1 < ntile) {
            tile_load(qbase + (size_t)(tile + 1) * TR * ld, ld, t, rq);
            tile_load(gbase + (size_t)(tile + 1) * TR * C, (size_t)C, t, rg);
            tile_load(qtbase + (size_t)(tile + 1) * TR, M, t, rqt);
            tile_load(gtbase + (size_t)(tile + 1) * TR, M, t, rgt);
            if (t < 128) rs = stbase[(size_t)(tile + 1) * TR];
        }
        f32x4 s[4], dp[4];
        scores(sQ, kf, c, g, s);                              // [query 16 a + 4 g + r][key c]
        scores(sG, vf, c, g, dp);
        bf16x8 pb[2], dsb[2];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const f32x4 l4 = *(const f32x4*)(sL + 16 * a + 4 * g), d4 = *(const f32x4*)(sD + 16 * a + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool qreal = tile * TR + 16 * a + 4 * g + r < T;      // queries >= T are masked
                const float p = __builtin_amdgcn_exp2f(s[a][r] * MHMR_ATTN_QSCALE - l4[r]);
                put(pb, a, r, qreal ? p : 0.f);
                put(dsb, a, r, qreal ? p * (dp[a][r] - d4[r]) : 0.f);
            }
        }
        weighted(sGT, pb, c, g, dv);
        weighted(sQT, dsb, c, g, dk);
        __syncthreads();
    }
    const bool real = k < T;
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        f32x4 vk;
#pragma unroll
        for (int r = 0; r < 4; ++r) vk[r] = real ? dk[db][r] * ATTN_SCALE : 0.f;
        *(f32x4*)(dkrow + 16 * db) = vk;
        *(f32x4*)(dvrow + 16 * db) = real ? dv[db] : zero;
    }
}

// the workspace: qkv as it lies, dO as it lies, three transposed copies (tr0 = V^T in the tape, K^T in the backward), D
struct Attn16Layout { long long qkvb, dob, tr0, qt, gt, D, total; };
Attn16Layout attn16_layout(long long B, long long Tp, long long C) {
    Attn16Layout L;
    WsCursor ws;
    const long long mc = B * Tp * C * 2;
    L.qkvb = ws.take(3 * mc); L.dob = ws.take(mc); L.tr0 = ws.take(mc); L.qt = ws.take(mc); L.gt = ws.take(mc);
    L.D = ws.take(B * (C / 64) * Tp * (long long)sizeof(float));
    L.total = ws.at;
    return L;
}

int attn16_shape_rc(int B, int T, int Tp, int C, int H) {
    TRY(mhmr_attention_shape_rc(B, T, Tp, C, H));
    if ((long long)B * Tp / 64 > 65535) return MHMR_ERR_BAD_SHAPE;           // row tiles of the transposing convert kernel
    return 0;
}

}  // namespace

long long mhmr_attention_bf16_bytes(int B, int Tp, int C) { return attn16_layout(B, Tp, C).total; }

int mhmr_launch_attention_bf16_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* ws_, hipStream_t s) {
    const Attn16Layout L = attn16_layout(B, Tp, C);
    char* ws = (char*)ws_;
    const int M = B * Tp;
    __bf16 *qkvb = (__bf16*)(ws + L.qkvb), *vt = (__bf16*)(ws + L.tr0);
    mhmr_launch_to_bf16(qkv, 3 * C, qkvb, M, 3 * C, false, s);
    mhmr_launch_to_bf16(qkv + 2 * C, 3 * C, vt, M, C, true, s);              // V^T [C, M]
    hipLaunchKernelGGL(attn16_tape_kernel, dim3(Tp / TR, H, B), dim3(256), 0, s, (const __bf16*)qkvb, (const __bf16*)vt, out32, lse, T, Tp, C, H,
                       (size_t)M);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int mhmr_launch_attention_bf16_bwd(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                   int Tp, int C, int H, void* ws_, bool qkv_ready, hipStream_t s) {
    const Attn16Layout L = attn16_layout(B, Tp, C);
    char* ws = (char*)ws_;
    const int M = B * Tp;
    __bf16 *qkvb = (__bf16*)(ws + L.qkvb), *dob = (__bf16*)(ws + L.dob), *kt = (__bf16*)(ws + L.tr0), *qt = (__bf16*)(ws + L.qt);
    __bf16* gt = (__bf16*)(ws + L.gt);
    float* D = (float*)(ws + L.D);
    if (!qkv_ready) mhmr_launch_to_bf16(qkv, 3 * C, qkvb, M, 3 * C, false, s);
    mhmr_launch_to_bf16(qkv, 3 * C, qt, M, C, true, s);                      // Q^T [C, M]
    mhmr_launch_to_bf16(qkv + C, 3 * C, kt, M, C, true, s);                  // K^T
    mhmr_launch_to_bf16(dO, lddo, dob, M, C, false, s);
    mhmr_launch_to_bf16(dO, lddo, gt, M, C, true, s);                        // dO^T
    const size_t n = (size_t)M * H * 16;
    hipLaunchKernelGGL(attn16_rowdot_kernel, dim3(blocks256(n)), dim3(256), 0, s, dO, lddo, out32, D, n, T, Tp, C, H);
    const dim3 grid(Tp / TR, H, B);
    hipLaunchKernelGGL(attn16_bwd_q_kernel, grid, dim3(256), 0, s, (const __bf16*)qkvb, (const __bf16*)dob, (const __bf16*)kt, lse, (const float*)D,
                       dqkv, T, Tp, C, H, (size_t)M);
    hipLaunchKernelGGL(attn16_bwd_kv_kernel, grid, dim3(256), 0, s, (const __bf16*)qkvb, (const __bf16*)dob, (const __bf16*)qt, (const __bf16*)gt,
                       lse, (const float*)D, dqkv, T, Tp, C, H, (size_t)M);
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" {

long long mhmr_attention_bf16_workspace_bytes(int B, int Tp, int C, int H) {
    TRY(attn16_shape_rc(B, Tp, Tp, C, H));
    return attn16_layout(B, Tp, C).total;
}

int mhmr_attention_bf16_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* workspace,
                             long long workspace_bytes, void* stream) {
    TRY(attn16_shape_rc(B, T, Tp, C, H));
    if (!qkv || !out32 || !lse || !workspace || workspace_bytes < attn16_layout(B, Tp, C).total) return MHMR_ERR_BAD_ARG;
    if (!aligned16(qkv) || !aligned16(out32) || !aligned16(workspace)) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_attention_bf16_tape(qkv, out32, lse, B, T, Tp, C, H, workspace, (hipStream_t)stream);
}

int mhmr_attention_bf16_backward(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                 int Tp, int C, int H, void* workspace, long long workspace_bytes, void* stream) {
    TRY(attn16_shape_rc(B, T, Tp, C, H));
    if (lddo < C || lddo % 4) return MHMR_ERR_BAD_SHAPE;
    if (!qkv || !out32 || !lse || !dO || !dqkv || !workspace || workspace_bytes < attn16_layout(B, Tp, C).total) return MHMR_ERR_BAD_ARG;
    if (!aligned16(qkv) || !aligned16(out32) || !aligned16(lse) || !aligned16(dO) || !aligned16(dqkv) || !aligned16(workspace))
        return MHMR_ERR_BAD_ARG;
    return mhmr_launch_attention_bf16_bwd(qkv, out32, lse, dO, lddo, dqkv, B, T, Tp, C, H, workspace, false, (hipStream_t)stream);
}

}  // extern "C"
