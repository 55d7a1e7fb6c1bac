// Dense linears with bf16 operands and fp32 accumulation: the mixed-precision form of the block backward's
// products.  The inputs are fp32; r() is round-to-nearest-even fp32 -> bf16 (what torch.Tensor.bfloat16() does):
//     forward        Y[m][n]  = sum_k r(X[m][k])  r(W[n][k]) + bias[n]
//     input side     dX[m][k] = sum_n r(dY[m][n]) r(W[n][k]) (+ dR[m][k])
//     weight side    dW[n][k] = sum_m r(dY[m][n]) r(X[m][k]),   db[n] = sum_m dY[m][n]  (fp64, the UNROUNDED dY)
// A product of two bf16 numbers is exact in fp32, so against the fp64 product of the rounded operands the only error is the order of the
// fp32 accumulation.
//
// Structure.  One MFMA kernel computes C[i][j] = sum_s P[i][s] Q[j][s] for two bf16 matrices that are both contiguous along the summed
// index s (v_mfma_f32_16x16x32_bf16; workgroup = 128 x 128 outputs, four waves of 64 x 64 = 4 x 4 MFMA tiles; 64 summed indices per step,
// staged through LDS with 144-byte rows).  A convert kernel writes the bf16 copy of an fp32 matrix as it lies or transposed: the input
// side needs W^T, the weight side dY^T and X^T.  The three launchers below are convert + product.
//
// The shape of every sum is fixed by (M, N, K) alone: an accumulator chain runs over at most CHAIN = 256 summed indices and is then added
// into a second accumulator (the idea of BlockedSum2, hph_shared.h); the weight side, which sums over the M rows, is further cut into
// slices of WSLICE = 4096 rows whose fp32 partial products live in the workspace and are added in slice order in fp64, rounded once.
// Slices and chains start at fixed row indices, so rows of exact zeros behind the last row change no bit (x + 0 is exact).  No
// floating-point atomics, every element of every output is written, two calls give the same bits; nothing allocates or synchronises.
// Partial tiles: M and N are multiples of 64, the tile is 128: row and column addresses are clamped into the matrix, stores are guarded.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "row_sums.h"

namespace {

constexpr int BT = 128;                    // output tile edge
constexpr int BK = 64;                     // summed indices per step
constexpr int LDT = BK + 8;                // LDS row pitch in elements: 144 bytes, so that the 16 rows of a fragment read spread over the banks
constexpr int CHAIN = 256;                 // summed indices per first-level accumulator chain
constexpr int WSLICE = 4096;               // rows per slice of the weight side's sum over M
constexpr int DB_SLICE = 32;               // rows per first-stage slice of the bias column sums (row_sums.h)

// ---------------------------------------------------------------- C[i][j] = sum_s P[i][s] Q[j][s]  (+ bias[j]) (+ R[i][j])
// grid.x = row tiles x column tiles (column tiles of one row tile neighbours on an XCD), grid.z = slices of the summed index: slice z
// covers [z sslice, min(S, (z + 1) sslice)) and writes out + z zstride.  The MFMA takes Q's fragment as its A operand and P's as its B
// operand, so a lane holds C[i = lane & 15][j = 4 (lane >> 4) + r]: four consecutive j, stored (and bias / R read) as 16 bytes.
// Two workgroups per CU (236 registers, no spill; 36 KiB of LDS each): one computes while the other waits at its barrier.
__global__ __launch_bounds__(256, 2) void nt_bf16_kernel(const __bf16* __restrict__ P, int ldp, const __bf16* __restrict__ Q, int ldq, float* out,
                                                      int ldo, long long zstride, int I, int J, int S, int sslice,
                                                      const float* __restrict__ bias, const float* R, int ldr, int ntj) {
    __shared__ __attribute__((aligned(16))) __bf16 smem[2 * BT * LDT];
    __bf16* sP = smem;
    __bf16* sQ = smem + BT * LDT;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int l15 = lane & 15, g = lane >> 4;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int ti = bid / ntj, tj = bid - ti * ntj;
    const int i0 = ti * BT, j0 = tj * BT;
    const int s0 = blockIdx.z * sslice, s1 = min(S, s0 + sslice);
    // staging: a 128 x 64 tile is 1024 pieces of 16 bytes; thread t moves pieces t + 256 e: row (t >> 3) + 32 e, elements 8 (t & 7) ..
    const int srow = t >> 3, sch = (t & 7) * 8;
    const __bf16 *pp[4], *qp[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pp[e] = P + (size_t)min(i0 + srow + 32 * e, I - 1) * ldp + sch;
        qp[e] = Q + (size_t)min(j0 + srow + 32 * e, J - 1) * ldq + sch;
    }
    bf16x8 rp[4], rq[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        rp[e] = *(const bf16x8*)(pp[e] + s0);
        rq[e] = *(const bf16x8*)(qp[e] + s0);
    }
    const int wi = (w & 1) * 64, wj = (w >> 1) * 64;
    f32x4 acc[4][4], top[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = top[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = s0; s < s1; s += BK) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            *(bf16x8*)(sP + (srow + 32 * e) * LDT + sch) = rp[e];
            *(bf16x8*)(sQ + (srow + 32 * e) * LDT + sch) = rq[e];
        }
        __syncthreads();
        if (s + BK < s1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rp[e] = *(const bf16x8*)(pp[e] + s + BK);
                rq[e] = *(const bf16x8*)(qp[e] + s + BK);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fp[4], fq[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                fp[a] = *(const bf16x8*)(sP + (wi + 16 * a + l15) * LDT + 32 * ks + 8 * g);
                fq[a] = *(const bf16x8*)(sQ + (wj + 16 * a + l15) * LDT + 32 * ks + 8 * g);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fq[b], fp[a], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
        if ((s + BK - s0) % CHAIN == 0 || s + BK >= s1) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) { top[a][b][r] += acc[a][b][r]; acc[a][b][r] = 0.f; }
        }
    }
    float* o = out + (size_t)blockIdx.z * zstride;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + wi + 16 * a + l15;
        if (i >= I) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + wj + 16 * b + 4 * g;
            if (j >= J) continue;
            f32x4 v = top[a][b];
            if (bias) {
                const f32x4 bv = *(const f32x4*)(bias + j);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += bv[r];
            }
            if (R) {
                const f32x4 rv = *(const f32x4*)(R + (size_t)i * ldr + j);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += rv[r];
            }
            *(f32x4*)(o + (size_t)i * ldo + j) = v;
        }
    }
}

// ---------------------------------------------------------------- fp32 -> bf16 copies (rows and cols multiples of 64)
// as it lies: out[r][c] = r(in[r][c]), four elements per thread
__global__ __launch_bounds__(256) void to_bf16_kernel(const float* __restrict__ in, int ld, __bf16* __restrict__ out, int ldo, size_t n4, int cols4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const size_t r = i / (size_t)cols4;
    const int c = (int)(i - r * (size_t)cols4) * 4;
    const f32x4 v = *(const f32x4*)(in + r * (size_t)ld + c);
    bf16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
    *(bf16x4*)(out + r * (size_t)ldo + c) = o;
}

// transposed: out[c][r] = r(in[r][c]); one workgroup moves a 64 x 64 tile through LDS (fp32, pitch 65)
__global__ __launch_bounds__(256) void to_bf16_t_kernel(const float* __restrict__ in, int ld, __bf16* __restrict__ out, int ldo) {
    __shared__ float tile[64][65];
    const int t = threadIdx.x;
    const size_t r0 = (size_t)blockIdx.y * 64, c0 = (size_t)blockIdx.x * 64;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = (t >> 4) + 16 * e, c = (t & 15) * 4;
        const f32x4 v = *(const f32x4*)(in + (r0 + r) * (size_t)ld + c0 + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) tile[r][c + u] = v[u];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = (t >> 3) + 32 * e, r = (t & 7) * 8;
        bf16x8 o;
#pragma unroll
        for (int u = 0; u < 8; ++u) o[u] = (__bf16)tile[r + u][c];
        *(bf16x8*)(out + (c0 + c) * (size_t)ldo + r0 + r) = o;
    }
}

// dW[n][k] = the slices in index order (fp64), rounded once
__global__ __launch_bounds__(256) void slices_finish_kernel(const float* __restrict__ part, float* __restrict__ dW, int lddw, int nsl, int N, int K) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)N * K;
    if (i >= total) return;
    double s = 0.0;
    for (int sl = 0; sl < nsl; ++sl) s += (double)part[(size_t)sl * total + i];
    const size_t n = i / (size_t)K;
    dW[n * (size_t)lddw + (i - n * (size_t)K)] = (float)s;
}

// the addends of (row, column) of the bias sums (row_sums.h): (dY, 0)
struct BiasTerm {
    const float* dY; int ld;
    __device__ __forceinline__ double operator()(int r, int, int c, double (&ta)[1], double (&tb)[1]) const {
        ta[0] = (double)dY[(size_t)r * ld + c];
        tb[0] = 0.0;
        return 0.0;
    }
};

inline int weight_slices(long long M) { return (int)((M + WSLICE - 1) / WSLICE); }

// the workspace of one linear: the two bf16 operands, the weight side's partial products and the scratch of the bias sums
struct LinLayout { long long opa, opb, part, dbp, dbz, total; };
LinLayout lin_layout(long long M, long long N, long long K) {
    LinLayout L;
    WsCursor ws;
    const long long nk = N > K ? N : K;
    L.opa = ws.take(M * nk * 2);                                             // X | dY | dY^T
    L.opb = ws.take((N * K > M * nk ? N * K : M * nk) * 2);                  // W | W^T | X^T
    L.part = ws.take((long long)weight_slices(M) * N * K * (long long)sizeof(float));
    L.dbp = ws.take((M + DB_SLICE - 1) / DB_SLICE * N * 2 * (long long)sizeof(double));
    L.dbz = ws.take(N * (long long)sizeof(float));
    L.total = ws.at;
    return L;
}

int shape_rc(long long M, int N, int K) {
    if (M < 0 || N < 0 || K < 0) return MHMR_ERR_BAD_ARG;
    if (M < 64 || N < 64 || K < 64 || M % 64 || N % 64 || K % 64 || M > 16ll * 65535) return MHMR_ERR_BAD_SHAPE;
    return 0;
}
inline bool ld_ok(int ld, int row) { return ld >= row && ld % 4 == 0; }

}  // namespace

void mhmr_launch_to_bf16(const float* in, int ld, __bf16* out, int rows, int cols, bool transposed, hipStream_t s) {
    if (transposed) hipLaunchKernelGGL(to_bf16_t_kernel, dim3(cols / 64, rows / 64), dim3(256), 0, s, in, ld, out, rows);
    else {
        const size_t n4 = (size_t)rows * (cols / 4);
        hipLaunchKernelGGL(to_bf16_kernel, dim3(blocks256(n4)), dim3(256), 0, s, in, ld, out, cols, n4, cols / 4);
    }
}

namespace {

// ready bf16 operands: out[z][i][j] = sum over slice z of P[i][s] Q[j][s] (+ bias[j]) (+ R[i][j]); nsl == 1: the whole sum
void launch_nt(const __bf16* P, int ldp, const __bf16* Q, int ldq, float* out, int ldo, int I, int J, int S, int nsl, int sslice,
               const float* bias, const float* R, int ldr, hipStream_t s) {
    const int nti = (I + BT - 1) / BT, ntj = (J + BT - 1) / BT;
    hipLaunchKernelGGL(nt_bf16_kernel, dim3(nti * ntj, 1, nsl), dim3(256), 0, s, P, ldp, Q, ldq, out, ldo, (long long)I * ldo, I, J, S, sslice, bias, R,
                       ldr, ntj);
}

}  // namespace

long long mhmr_linear_bf16_bytes(long long M, int N, int K) { return lin_layout(M, N, K).total; }

int mhmr_launch_linear_bf16(const float* X, int ldx, const float* W, int ldw, const float* bias, float* Y, int ldy, int M, int N, int K, void* ws_,
                            hipStream_t s) {
    const LinLayout L = lin_layout(M, N, K);
    char* ws = (char*)ws_;
    __bf16 *xb = (__bf16*)(ws + L.opa), *wb = (__bf16*)(ws + L.opb);
    mhmr_launch_to_bf16(X, ldx, xb, M, K, false, s);
    mhmr_launch_to_bf16(W, ldw, wb, N, K, false, s);
    launch_nt(xb, K, wb, K, Y, ldy, M, N, K, 1, K, bias, nullptr, 0, s);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int mhmr_launch_linear_bf16_bwd_input(const float* dY, int lddy, const float* W, int ldw, const float* dR, int lddr, float* dX, int lddx, int M, int N,
                                      int K, void* ws_, hipStream_t s) {
    const LinLayout L = lin_layout(M, N, K);
    char* ws = (char*)ws_;
    __bf16 *gb = (__bf16*)(ws + L.opa), *wt = (__bf16*)(ws + L.opb);
    mhmr_launch_to_bf16(dY, lddy, gb, M, N, false, s);
    mhmr_launch_to_bf16(W, ldw, wt, N, K, true, s);                          // W^T [K, N]
    launch_nt(gb, N, wt, N, dX, lddx, M, K, N, 1, N, nullptr, dR, lddr, s);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int mhmr_launch_linear_bf16_bwd_weight(const float* dY, int lddy, const float* X, int ldx, float* dW, int lddw, float* db, int M, int N, int K,
                                       void* ws_, hipStream_t s) {
    const LinLayout L = lin_layout(M, N, K);
    char* ws = (char*)ws_;
    if (dW) {
        __bf16 *gt = (__bf16*)(ws + L.opa), *xt = (__bf16*)(ws + L.opb);
        float* part = (float*)(ws + L.part);
        const int nsl = weight_slices(M);
        mhmr_launch_to_bf16(dY, lddy, gt, M, N, true, s);                    // dY^T [N, M]
        mhmr_launch_to_bf16(X, ldx, xt, M, K, true, s);                      // X^T  [K, M]
        launch_nt(gt, M, xt, M, part, K, N, K, M, nsl, WSLICE, nullptr, nullptr, 0, s);
        hipLaunchKernelGGL(slices_finish_kernel, dim3(blocks256((size_t)N * K)), dim3(256), 0, s, (const float*)part, dW, lddw, nsl, N, K);
    }
    if (db) {
        const int nsl = (M + DB_SLICE - 1) / DB_SLICE;
        double* dbp = (double*)(ws + L.dbp);
        hipLaunchKernelGGL((col_sums1_kernel<DB_SLICE, 1, BiasTerm>), dim3(N / 64, nsl), dim3(64), 0, s, BiasTerm{dY, lddy}, dbp, (double*)nullptr, 0,
                           0, M, N);
        hipLaunchKernelGGL(col_sums2_kernel, dim3(N / 64), dim3(64), 0, s, (const double*)dbp, (const double*)nullptr, (const float*)nullptr, db,
                           (float*)(ws + L.dbz), (float*)nullptr, nsl, N);
    }
    MHMR_CHECK_LAUNCH();
    return 0;
}

extern "C" {

long long mhmr_linear_bf16_workspace_bytes(int M, int N, int K) {
    TRY(shape_rc(M, N, K));
    return lin_layout(M, N, K).total;
}

int mhmr_linear_bf16(const float* X, int ldx, const float* W, int ldw, const float* bias, float* Y, int ldy, int M, int N, int K, void* workspace,
                     long long workspace_bytes, void* stream) {
    TRY(shape_rc(M, N, K));
    if (!ld_ok(ldx, K) || !ld_ok(ldw, K) || !ld_ok(ldy, N)) return MHMR_ERR_BAD_SHAPE;
    if (!X || !W || !Y || !workspace || workspace_bytes < lin_layout(M, N, K).total) return MHMR_ERR_BAD_ARG;
    if (!aligned16(X) || !aligned16(W) || !aligned16(Y) || !aligned16(bias) || !aligned16(workspace)) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_linear_bf16(X, ldx, W, ldw, bias, Y, ldy, M, N, K, workspace, (hipStream_t)stream);
}

int mhmr_linear_bf16_backward_input(const float* dY, int lddy, const float* W, int ldw, const float* dR, int lddr, float* dX, int lddx, int M, int N,
                                    int K, void* workspace, long long workspace_bytes, void* stream) {
    TRY(shape_rc(M, N, K));
    if (!ld_ok(lddy, N) || !ld_ok(ldw, K) || !ld_ok(lddx, K) || (dR && !ld_ok(lddr, K))) return MHMR_ERR_BAD_SHAPE;
    if (!dY || !W || !dX || !workspace || workspace_bytes < lin_layout(M, N, K).total) return MHMR_ERR_BAD_ARG;
    if (!aligned16(dY) || !aligned16(W) || !aligned16(dX) || !aligned16(dR) || !aligned16(workspace)) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_linear_bf16_bwd_input(dY, lddy, W, ldw, dR, lddr, dX, lddx, M, N, K, workspace, (hipStream_t)stream);
}

int mhmr_linear_bf16_backward_weight(const float* dY, int lddy, const float* X, int ldx, float* dW, int lddw, float* db, int M, int N, int K,
                                     void* workspace, long long workspace_bytes, void* stream) {
    TRY(shape_rc(M, N, K));
    if (!ld_ok(lddy, N) || !ld_ok(ldx, K) || (dW && !ld_ok(lddw, K))) return MHMR_ERR_BAD_SHAPE;
    if (!dW && !db) return MHMR_ERR_BAD_ARG;
    if (!dY || !X || !workspace || workspace_bytes < lin_layout(M, N, K).total) return MHMR_ERR_BAD_ARG;
    if (!aligned16(dY) || !aligned16(X) || !aligned16(dW) || !aligned16(workspace)) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_linear_bf16_bwd_weight(dY, lddy, X, ldx, dW, lddw, db, M, N, K, workspace, (hipStream_t)stream);
}

}  // extern "C"
