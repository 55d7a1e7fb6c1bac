// The sums over rows that the backward files (hph_bwd.hip, detect_bwd.hip) share, defined once: the sliced outer product
// dW[n][c] = sum_rows left[row][n] * op16[row][c] and the two-stage fp64 column sums, with their slice geometry and the workspace cursor.
// Its sibling without a sum over rows lives here too: rows times weight, out[m][c] = sum_n left[m][n] * w16[n][c], the product that
// carries a cotangent back to the features for every row, with the same left operands.
// These carry the determinism rules (DESIGN.md sections 17-22): a sum that crosses rows is an fp32 MFMA chain or an fp64 sum whose shape the
// sizes alone fix, slices are added in index order, no floating-point atomics, every output element is written.  Changing a slice
// length, a clamp or an order here changes every user together; nothing here may be copied into a kernel.
#pragma once
#include "mhmr_common.h"

namespace {

// ---------------------------------------------------------------- host helpers of the launchers
inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }      // workgroups of 256 threads over n elements
inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

// ---------------------------------------------------------------- workspace cursor: every piece 256-byte aligned
inline long long align256(long long v) { return (v + 255) / 256 * 256; }
struct WsCursor {
    long long at = 0;
    long long take(long long bytes) { const long long o = at; at += align256(bytes); return o; }
};

// ---------------------------------------------------------------- slice geometry of the outer product
constexpr int ROW_SLICE_CAP = 16;                         // upper bound of the row slices
constexpr int ROW_SLICE_GRAIN = 512;                      // no slice is cut below this many rows
// min(16, ceil(rows / 512)); rows == 0 has NO slice: nothing is launched over rows and the finishing pass writes zeros
inline int row_slices(int rows) { return (rows + ROW_SLICE_GRAIN - 1) / ROW_SLICE_GRAIN < ROW_SLICE_CAP ? (rows + ROW_SLICE_GRAIN - 1) / ROW_SLICE_GRAIN : ROW_SLICE_CAP; }
// the same with ONE (empty) slice for rows == 0, for a caller that launches the product regardless: its partial is written as zeros
inline int row_slices_or_one(int rows) { return rows <= 0 ? 1 : row_slices(rows); }
inline int slice_rows(int rows, int nsl) { return ((rows + nsl - 1) / nsl + 3) / 4 * 4; }      // a multiple of the four rows of one MFMA

// ---------------------------------------------------------------- left operands of the outer product: a[t] = left[rc][na[t]]
// (rc: the row, clamped into the slice; live: the row lies in the slice -- a row past it contributes an exact zero)
// quad<VEC>: the four consecutive columns n0 .. n0 + 3 (n0 % 4 == 0) for the rows-times-weight product -- the same values as two calls
// of operator(); VEC reads them with one vector load per operand, which vec_ok() (host) allows when pitches and pointers are aligned.
struct LeftF32 {                                          // an fp32 matrix G [rows, ld]
    const float* G; int ld;
    __device__ __forceinline__ void operator()(int rc, bool live, const int (&na)[2], float (&a)[2]) const {
        const float* gp = G + (size_t)rc * ld;
#pragma unroll
        for (int t = 0; t < 2; ++t) a[t] = live ? gp[na[t]] : 0.f;
    }
    template <bool VEC>
    __device__ __forceinline__ void quad(int rc, bool live, int n0, float (&a)[4]) const {
        if constexpr (VEC) {
            const f32x4 v = *(const f32x4*)(G + (size_t)rc * ld + n0);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = live ? v[e] : 0.f;
        } else {
            const int n01[2] = {n0, n0 + 1}, n23[2] = {n0 + 2, n0 + 3};
            float lo[2], hi[2];
            (*this)(rc, live, n01, lo);
            (*this)(rc, live, n23, hi);
            a[0] = lo[0]; a[1] = lo[1]; a[2] = hi[0]; a[3] = hi[1];
        }
    }
    bool vec_ok() const { return ld % 4 == 0 && (uintptr_t)G % 16 == 0; }
};
template <int DT>
struct LeftReluMask {                                     // hid16[row][n] > 0 ? dl[row] : 0, formed in registers
    const void* hid; int ld; const float* dl;
    __device__ __forceinline__ void operator()(int rc, bool live, const int (&na)[2], float (&a)[2]) const {
        const typename Op<DT>::T* hp = (const typename Op<DT>::T*)hid + (size_t)rc * ld;
        const float d = live ? dl[rc] : 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) a[t] = (float)hp[na[t]] > 0.f ? d : 0.f;
    }
};
template <int DT>
struct LeftReluMaskW2 {                                   // hid16[row][n] > 0 ? dl[row] * w2[n] : 0: the hidden layer's cotangent, in registers
    const void* hid; int ld; const float* dl; const float* w2;
    __device__ __forceinline__ void operator()(int rc, bool live, const int (&na)[2], float (&a)[2]) const {
        const typename Op<DT>::T* hp = (const typename Op<DT>::T*)hid + (size_t)rc * ld;
        const float d = live ? dl[rc] : 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) a[t] = (float)hp[na[t]] > 0.f ? d * w2[na[t]] : 0.f;
    }
    template <bool VEC>
    __device__ __forceinline__ void quad(int rc, bool live, int n0, float (&a)[4]) const {
        if constexpr (VEC) {
            const typename Op<DT>::V4 h = *(const typename Op<DT>::V4*)((const typename Op<DT>::T*)hid + (size_t)rc * ld + n0);
            const f32x4 w = *(const f32x4*)(w2 + n0);
            const float d = live ? dl[rc] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = (float)h[e] > 0.f ? d * w[e] : 0.f;
        } else {
            const int n01[2] = {n0, n0 + 1}, n23[2] = {n0 + 2, n0 + 3};
            float lo[2], hi[2];
            (*this)(rc, live, n01, lo);
            (*this)(rc, live, n23, hi);
            a[0] = lo[0]; a[1] = lo[1]; a[2] = hi[0]; a[3] = hi[1];
        }
    }
    bool vec_ok() const { return ld % 4 == 0 && (uintptr_t)hid % 8 == 0 && (uintptr_t)w2 % 16 == 0; }
};

// ---------------------------------------------------------------- rows times weight: out[m][c] (+)= sum_n left[m][n] * w16[n][c]
// The product that carries a cotangent from the output of a 16-bit linear back to its input, for every row: no sum crosses rows, so a
// row's result depends on that row alone (any number of rows gives a row the same bits).  Workgroup = 64 (m) x 128 (c), four waves of
// 32 x 64 (2 x 4 MFMA tiles).  A lane owns four CONSECUTIVE columns, c0 + 4 l15 + u (tile u of the wave holds the columns c0 + 4 j + u),
// so the weight comes in as one 8-byte load per reduction index and the result leaves as 16-byte stores.  The reduction runs in steps of
// 16: lane group g holds n + 4 g .. n + 4 g + 3, MFMA e of a step takes the e-th of them from every group; even and odd e go to
// accumulators of their own (two chains of half the length round less than one), added once at the end.  Rows past `rows` contribute
// nothing and are not stored (their addresses are clamped to the last row).  ACC: out = out + product, one more rounding -- the bits of
// a write followed by an fp32 add.  VEC: vector loads and stores (aligned pitches and pointers: the launcher decides); without it the
// same values move one by one, so both forms give the same bits.  The workgroups are numbered so that the column tiles of one row tile
// share an L2 (xcd_remap).  Nn % 16 == 0 and Cout % 128 == 0 (the caller checks).
constexpr int RTW_ROWS = 64, RTW_COLS = 128;
constexpr long long RTW_MAX_WORKGROUPS = 0xFFFFFF;       // 256 threads each: the launch's thread count stays below 2^32

template <int DT, typename Left, bool ACC, bool VEC>
__global__ __launch_bounds__(256) void rows_times_weight_kernel(Left left, const void* __restrict__ w16_, int ldw, float* out, int ldo, int rows,
                                                                int Nn, int ncol) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V4 V4;
    const T* w16 = (const T*)w16_;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int rt = bid / ncol, ct = bid - rt * ncol;
    const int m0 = rt * RTW_ROWS + (w & 1) * 32, cl = ct * RTW_COLS + (w >> 1) * 64 + 4 * l15;
    int ra[2];
    bool live[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int rr = m0 + 16 * t + l15;
        live[t] = rr < rows;
        ra[t] = min(rr, rows - 1);
    }
    f32x4 acc[2][2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[h][t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < Nn; n += 16) {
        const int nb = n + 4 * g;
        float a[2][4], bb[4][4];
#pragma unroll
        for (int t = 0; t < 2; ++t) left.template quad<VEC>(ra[t], live[t], nb, a[t]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const T* wp = w16 + (size_t)(nb + e) * ldw + cl;
            if constexpr (VEC) {
                const V4 v = *(const V4*)wp;
#pragma unroll
                for (int u = 0; u < 4; ++u) bb[e][u] = (float)v[u];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) bb[e][u] = (float)wp[u];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[e & 1][t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][e], bb[e][u], acc[e & 1][t][u], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * t + 4 * g + r;
            if (m >= rows) continue;
            float* op = out + (size_t)m * ldo + cl;
            f32x4 v;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = acc[0][t][u][r] + acc[1][t][u][r];
            if constexpr (VEC) {
                if (ACC) {
                    const f32x4 old = *(const f32x4*)op;
#pragma unroll
                    for (int u = 0; u < 4; ++u) v[u] = old[u] + v[u];
                }
                *(f32x4*)op = v;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) op[u] = ACC ? op[u] + v[u] : v[u];
            }
        }
}

// MHMR_ERR_BAD_ARG: rows < 0; MHMR_ERR_BAD_SHAPE: the tile rules and the launch limit
inline int rows_times_weight_shape_rc(int rows, int Nn, int Cout) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (Nn <= 0 || Nn % 16 || Cout <= 0 || Cout % RTW_COLS) return MHMR_ERR_BAD_SHAPE;
    if (((long long)rows + RTW_ROWS - 1) / RTW_ROWS * (Cout / RTW_COLS) > RTW_MAX_WORKGROUPS) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

// (arguments validated by the caller: rows_times_weight_shape_rc, ldw >= Cout, ldo >= Cout).  rows == 0: nothing to write.
template <int DT, typename Left>
int launch_rows_times_weight(Left left, const void* w16, int ldw, float* out, int ldo, int rows, int Nn, int Cout, bool accumulate, hipStream_t s) {
    if (rows == 0) return 0;
    const int ncol = Cout / RTW_COLS;
    const dim3 grid((unsigned)((rows + RTW_ROWS - 1) / RTW_ROWS * ncol));
    const bool vec = left.vec_ok() && ldw % 4 == 0 && (uintptr_t)w16 % 8 == 0 && ldo % 4 == 0 && (uintptr_t)out % 16 == 0;
#define RTW_LAUNCH(ACC, VEC) \
    hipLaunchKernelGGL((rows_times_weight_kernel<DT, Left, ACC, VEC>), grid, dim3(256), 0, s, left, w16, ldw, out, ldo, rows, Nn, ncol)
    if (accumulate) { if (vec) RTW_LAUNCH(true, true); else RTW_LAUNCH(true, false); }
    else { if (vec) RTW_LAUNCH(false, true); else RTW_LAUNCH(false, false); }
#undef RTW_LAUNCH
    MHMR_CHECK_LAUNCH();
    return 0;
}

// Sliced outer product: part[slice][n][c] = sum over the slice's rows of left[row][n] * op16[row][c].  Workgroup = 64 (n) x 128 (c), four
// waves of 32 x 64 (2 x 4 MFMA tiles); four rows per MFMA, rows in index order; rows past the slice's end contribute an exact zero (their
// addresses are clamped into the slice, so nothing behind `rows` is read).  EDGE: Nn % 64 or Kc % 128 may be nonzero -- columns are clamped
// into Nn / Kc once, before the loop, and the stores are guarded; without it (the caller guarantees whole tiles) a row's loads share one
// address, which measured 8 % on the detection head's product.
template <int DT, typename Left, bool EDGE>
__global__ __launch_bounds__(256) void row_outer_kernel(Left left, const void* __restrict__ op16_, int ld16, float* __restrict__ part, int rows,
                                                        int Nn, int Kc, int slice_rows) {
    typedef typename Op<DT>::T T;
    const T* op16 = (const T*)op16_;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int n0 = blockIdx.y * 64 + (w & 1) * 32, c0 = blockIdx.x * 128 + (w >> 1) * 64;
    const int r0 = blockIdx.z * slice_rows, r1 = min(r0 + slice_rows, rows);
    int na[2], ca[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) na[t] = EDGE ? min(n0 + 16 * t + l15, Nn - 1) : n0 + 16 * t + l15;
#pragma unroll
    for (int u = 0; u < 4; ++u) ca[u] = EDGE ? min(c0 + 16 * u + l15, Kc - 1) : c0 + 16 * u + l15;
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; r += 4) {
        const int rr = r + g, rc = min(rr, r1 - 1);
        const T* cp = op16 + (size_t)rc * ld16;
        float a[2], bb[4];
        left(rc, rr < r1, na, a);
#pragma unroll
        for (int u = 0; u < 4; ++u) bb[u] = (float)cp[ca[u]];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bb[u], acc[t][u], 0, 0, 0);
    }
    float* pp = part + (size_t)blockIdx.z * Nn * Kc;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 16 * u + l15;
            if (EDGE && c >= Kc) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 16 * t + 4 * g + r;
                if (!EDGE || n < Nn) pp[(size_t)n * Kc + c] = acc[t][u][r];
            }
        }
}

// finishing pass: the slices in index order (fp64), times factor[n] (if any) in fp64 before the one rounding; columns c >= cvalid are exact
// zeros.  nsl == 0 (no rows) writes zeros and does not read factor.
__global__ __launch_bounds__(256) void row_outer_finish_kernel(const float* __restrict__ part, const float* __restrict__ factor,
                                                               float* __restrict__ dW, int nsl, int Nn, int Kc, int cvalid) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)Nn * Kc;
    if (i >= total) return;
    double s = 0.0;
    for (int sl = 0; sl < nsl; ++sl) s += (double)part[(size_t)sl * total + i];
    const size_t n = i / Kc;
    if (factor && nsl > 0) s *= (double)factor[n];
    dW[i] = (int)(i - n * Kc) < cvalid ? (float)s : 0.f;
}

// Column sums, stage 1, slices sl0 + blockIdx.y of SLICE rows each: part[slice][c] = (sum ta, sum tb) over the slice's rows in index order
// (fp64), where term(row, row - row0, c, ta, tb) gives the two addends of the thread's CPT columns c .. c + CPT - 1 and returns the row's
// own scalar; the slice's sum of those scalars goes to psum[slice] (if any).  A thread block is 64 threads = 64 CPT columns.
template <int SLICE, int CPT, typename Term>
__global__ __launch_bounds__(64) void col_sums1_kernel(Term term, double* __restrict__ part, double* __restrict__ psum, int sl0, int row0,
                                                       int rows, int C) {
    const int c = (blockIdx.x * 64 + threadIdx.x) * CPT, sl = sl0 + blockIdx.y;
    const int r0 = sl * SLICE, r1 = min(r0 + SLICE, rows);
    double a[CPT], b[CPT], sd = 0.0;
#pragma unroll
    for (int e = 0; e < CPT; ++e) a[e] = b[e] = 0.0;
    for (int r = r0; r < r1; ++r) {
        double ta[CPT], tb[CPT];
        sd += term(r, r - row0, c, ta, tb);
#pragma unroll
        for (int e = 0; e < CPT; ++e) { a[e] += ta[e]; b[e] += tb[e]; }
    }
    double* pp = part + ((size_t)sl * C + c) * 2;
#pragma unroll
    for (int e = 0; e < CPT; ++e) { pp[2 * e] = a[e]; pp[2 * e + 1] = b[e]; }
    if (psum && blockIdx.x == 0 && threadIdx.x == 0) psum[sl] = sd;
}

// stage 2: the slices in index order; the second sum times factor_b[c] (if any) in fp64; out_s[0] = the sum of psum (if any).  nsl == 0
// (no rows) writes zeros and does not read factor_b.
__global__ __launch_bounds__(64) void col_sums2_kernel(const double* __restrict__ part, const double* __restrict__ psum,
                                                       const float* __restrict__ factor_b, float* __restrict__ out_a,
                                                       float* __restrict__ out_b, float* __restrict__ out_s, int nsl, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int sl = 0; sl < nsl; ++sl) {
        a += part[((size_t)sl * C + c) * 2];
        b += part[((size_t)sl * C + c) * 2 + 1];
    }
    if (factor_b && nsl > 0) b *= (double)factor_b[c];
    out_a[c] = (float)a;
    out_b[c] = (float)b;
    if (out_s && c == 0) {
        double s = 0.0;
        for (int sl = 0; sl < nsl; ++sl) s += psum[sl];
        out_s[0] = (float)s;
    }
}

}  // namespace
