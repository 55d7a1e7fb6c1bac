// Backward of the detection head mlp_classif: the derivative of the two steps Model._front runs,
//   hid16 = op16(relu(ctx16[:, :C] . cls0_w16^T + b1))  (mhmr_gemm16, EPI_OP16_RELU)   and   scores = clamp(sigmoid(hid16 . w2 + b2))  (score_kernel),
// as those kernels evaluate them.  hid16, ctx16 and the rounded first-layer weight are exact numbers (straight-through); the ReLU mask is
// hid16[m][n] > 0, read from the stored bits; only the M = B N real rows are summed.  With gs the cotangent of scores:
//   dl_m = in_m ? gs_m p_m (1 - p_m) : 0,   p_m = sigmoid(s_m),  s_m = score_dot (the forward's own) + b2,  in_m = torch.clamp's mask
//   db2 = sum dl_m        dw2[n] = sum dl_m hid16[m][n]        db1[n] = w2[n] sum dl_m [hid16[m][n] > 0]
//   dW1[n][c] = w2[n] sum dl_m [hid16[m][n] > 0] ctx16[m][c]
// The [M, C] cotangent of the hidden layer never exists in memory: the left operand of the dW1 product is formed in registers from dl and
// the 16-bit hid16 tile.  w2[n] multiplies in the finishing passes, in fp64, so every output is rounded once.
//
// Rules (DESIGN.md sections 17-20): sums that cross rows are fp64 or fp32 MFMA chains (v_mfma_f32_16x16x4_f32 == an fmaf chain) of a shape
// fixed by the sizes alone; no floating-point atomics; every element of every output is written; two calls give the same bits.
// The kernels that carry those rules -- the sliced outer product of dW1 with its finishing pass and the two stages of the column sums --
// are those of row_sums.h, which hph_bwd.hip shares; this file holds the row pass, the column sums' term, the layout and the launcher.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "hph_shared.h"
#include "row_sums.h"

namespace {

constexpr int COL_SLICE = 512;                            // rows per first-stage slice of the column sums
constexpr float CLAMP_LO = 1e-4f, CLAMP_HI = 1.0f - 1e-4f;    // score_kernel's bounds

// ------------------------------------------------------------------------------------------------------------
// Row pass over the rows row0 .. row1 - 1, one wave per row (score_kernel's grid and its dot product): dl[m] in fp32 for the dW1 product
// and, unrounded, dl64[m - row0] for the column sums -- the sum of 8300 fp32 rounding errors of dl measured 1.3e-6 on a db2 of 2.48, six
// units in its last place, so the column sums do not see them.
// ------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void detect_dl_kernel(const void* __restrict__ hid_, int ld, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, const float* __restrict__ gs, float* __restrict__ dl,
                                                        double* __restrict__ dl64, int row0, int row1, int C, int clamped) {
    const int lane = threadIdx.x & 63;
    const int row = row0 + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row1) return;
    const float s = score_dot<DT>(hid_, ld, w2, row, lane, C) + b2[0];
    const float p = 1.0f / (1.0f + expf(-s));                     // score_kernel's expression: the clamp decision is the forward's
    const bool in = !clamped || (p >= CLAMP_LO && p <= CLAMP_HI);
    // dl is evaluated in fp64 at the forward's fp32 s.  p (1 - p) = t / (1 + t)^2 with t = exp(-|s|) <= 1: no
    // cancellation in 1 - p for a saturated row (unclamped, |s| = 12: 1.0f - p carries a relative error of 1e-2), no overflow for any s
    if (lane == 0) {
        const double t = exp(-fabs((double)s)), u = 1.0 + t;
        const double d = in ? (double)gs[row] * (t / (u * u)) : 0.0;
        dl[row] = (float)d;
        if (dl64) dl64[row - row0] = d;      // (no column sums follow the feature cotangent: it passes no scratch)
    }
}

// Column sums (row_sums.h: stage 1 over slices of COL_SLICE rows, one 16-bit column pair per thread, from the fp64 dl of the rows row0 ...;
// stage 2 the slices in index order, db1 taking its factor w2[n] there): the addends of (row, column) are (dl hid16, dl [hid16 > 0]), the
// row's scalar is dl (its sum is db2).
template <int DT>
struct DetectColTerm {
    const void* hid; int ld; const double* dl64;
    __device__ __forceinline__ double operator()(int r, int i, int c, double (&ta)[2], double (&tb)[2]) const {
        typedef typename Op<DT>::V2 V2;
        const V2 h = *(const V2*)((const typename Op<DT>::T*)hid + (size_t)r * ld + c);
        const double d = dl64[i];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float hv = (float)h[e];
            ta[e] = d * (double)hv;
            tb[e] = hv > 0.f ? d : 0.0;
        }
        return d;
    }
};

inline int col_slices(int rows) { return (rows + COL_SLICE - 1) / COL_SLICE; }

// workspace: the dW1 slice partials | dl [rows] | the column sums' slice partials (2 C + 1 doubles per slice).  Until the dW1 product
// runs, the region of its partials is the scratch of dl64: at least C C 4 >= 65536 bytes per slice of 512 rows, so it holds the fp64 dl
// of chunk_rows() >= 8192 rows at a time (of all rows unless rows > 8 C C), and the row pass and stage 1 go chunk by chunk.
struct Layout { long long part, dl, cols, pb2, total; };
inline Layout layout(int rows, int C) {
    Layout L;
    WsCursor ws;
    L.part = ws.take((long long)row_slices(rows) * C * C * 4);
    L.dl = ws.take(4LL * rows);
    L.cols = ws.take((long long)col_slices(rows) * C * 2 * 8);
    L.pb2 = ws.take(8LL * col_slices(rows));
    L.total = ws.at;
    return L;
}

inline int chunk_rows(int rows, int C) {      // a multiple of COL_SLICE: the slices and their sums do not depend on the chunking
    const long long cap = (long long)row_slices(rows) * C * C * 4 / 8 / COL_SLICE * COL_SLICE;
    return (int)(cap < rows ? cap : (long long)(rows + COL_SLICE - 1) / COL_SLICE * COL_SLICE);
}

int shape_rc(int rows, int C) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (C <= 0 || C % 128 || C > 16384 || rows > COL_SLICE * 65535) return MHMR_ERR_BAD_SHAPE;      // the column slices are gridDim.y of stage 1
    return 0;
}

template <int DT>
int launch(const void* hid16, int ldh, const void* ctx16, int ldx, const float* w2, const float* b2, const float* gs, int rows, int C,
           int clamped, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* ws, hipStream_t s) {
    const Layout L = layout(rows, C);
    float* part = (float*)((char*)ws + L.part);
    float* dl = (float*)((char*)ws + L.dl);
    double* cols = (double*)((char*)ws + L.cols);
    double* pb2 = (double*)((char*)ws + L.pb2);
    const int nsl = row_slices(rows), ncs = col_slices(rows);
    if (rows > 0) {
        const int chunk = chunk_rows(rows, C);
        for (int row0 = 0; row0 < rows; row0 += chunk) {
            const int row1 = row0 + chunk < rows ? row0 + chunk : rows;
            hipLaunchKernelGGL((detect_dl_kernel<DT>), dim3((row1 - row0 + 3) / 4), dim3(256), 0, s, hid16, ldh, w2, b2, gs, dl, (double*)part, row0,
                               row1, C, clamped);
            hipLaunchKernelGGL((col_sums1_kernel<COL_SLICE, 2, DetectColTerm<DT>>), dim3(C / 128, col_slices(row1 - row0)), dim3(64), 0, s,
                               DetectColTerm<DT>{hid16, ldh, (const double*)part}, cols, pb2, row0 / COL_SLICE, row0, rows, C);
        }
        hipLaunchKernelGGL((row_outer_kernel<DT, LeftReluMask<DT>, false>), dim3(C / 128, C / 64, nsl), dim3(256), 0, s, LeftReluMask<DT>{hid16, ldh, dl},
                           ctx16, ldx, part, rows, C, C, slice_rows(rows, nsl));
    }
    // rows == 0: no slices, neither finishing pass reads w2
    hipLaunchKernelGGL(col_sums2_kernel, dim3(C / 64), dim3(64), 0, s, cols, pb2, w2, g_w2, g_b1, g_b2, ncs, C);
    hipLaunchKernelGGL(row_outer_finish_kernel, dim3((unsigned)((size_t)C * C / 256)), dim3(256), 0, s, part, w2, g_w1, nsl, C, C, C);
    MHMR_CHECK_LAUNCH();
    return 0;
}

// The cotangent of the features: g_feat[m][c] = sum_n (hid16[m][n] > 0 ? dl_m w2[n] : 0) cls0_w16[n][c].  The row
// pass above leaves dl [rows] fp32 in the workspace; the product is row_sums.h's rows times weight with the hidden layer's cotangent as
// its left operand, formed in registers (one rounded fp32 product dl_m w2[n] per element, as if the array had been stored).
template <int DT>
int launch_feature_grad(const void* hid16, int ldh, const void* w16, int ldw, const float* w2, const float* b2, const float* gs, int rows, int C,
                        int clamped, float* g_feat, int ldg, float* dl, hipStream_t s) {
    hipLaunchKernelGGL((detect_dl_kernel<DT>), dim3((rows + 3) / 4), dim3(256), 0, s, hid16, ldh, w2, b2, gs, dl, (double*)nullptr, 0, rows, C, clamped);
    MHMR_CHECK_LAUNCH();
    return launch_rows_times_weight<DT>(LeftReluMaskW2<DT>{hid16, ldh, dl, w2}, w16, ldw, g_feat, ldg, rows, C, C, false, s);
}

}  // namespace

extern "C" {

long long mhmr_detect_feature_grad_workspace_bytes(int rows) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    return align256(4LL * rows);
}

int mhmr_detect_feature_grad(const void* hid16, int ldh, const void* cls0_w16, int ldw, const float* w2, const float* b2, const float* g_scores,
                             int rows, int C, int clamped, int dtype, float* g_feat, int ldg, void* workspace, long long workspace_bytes,
                             void* stream) {
    TRY(shape_rc(rows, C));
    TRY(rows_times_weight_shape_rc(rows, C, C));
    if (ldh < C || ldh % 2 || ldw < C || ldg < C || (dtype != MHMR_DT_F16 && dtype != MHMR_DT_BF16)) return MHMR_ERR_BAD_SHAPE;
    if (rows == 0) return 0;
    if (!hid16 || !cls0_w16 || !w2 || !b2 || !g_scores || !g_feat || !workspace || workspace_bytes < align256(4LL * rows)) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MHMR_DT_F16)
        return launch_feature_grad<MHMR_DT_F16>(hid16, ldh, cls0_w16, ldw, w2, b2, g_scores, rows, C, clamped, g_feat, ldg, (float*)workspace, s);
    return launch_feature_grad<MHMR_DT_BF16>(hid16, ldh, cls0_w16, ldw, w2, b2, g_scores, rows, C, clamped, g_feat, ldg, (float*)workspace, s);
}

long long mhmr_detect_backward_workspace_bytes(int rows, int C) {
    const int rc = shape_rc(rows, C);
    if (rc) return rc;
    return layout(rows, C).total;
}

int mhmr_detect_backward(const void* hid16, int ldh, const void* ctx16, int ldx, const float* w2, const float* b2, const float* g_scores,
                         int rows, int C, int clamped, int dtype, float* g_w1, float* g_b1, float* g_w2, float* g_b2, void* workspace,
                         long long workspace_bytes, void* stream) {
    TRY(shape_rc(rows, C));
    if (ldh < C || ldh % 2 || ldx < C || (dtype != MHMR_DT_F16 && dtype != MHMR_DT_BF16)) return MHMR_ERR_BAD_SHAPE;
    const long long need = layout(rows, C).total;
    if (!g_w1 || !g_b1 || !g_w2 || !g_b2 || workspace_bytes < need || (need > 0 && !workspace)) return MHMR_ERR_BAD_ARG;
    if (rows > 0 && (!hid16 || !ctx16 || !w2 || !b2 || !g_scores)) return MHMR_ERR_BAD_ARG;
    // rows == 0: empty sums, the four outputs are written as zeros
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MHMR_DT_F16)
        return launch<MHMR_DT_F16>(hid16, ldh, ctx16, ldx, w2, b2, g_scores, rows, C, clamped, g_w1, g_b1, g_w2, g_b2, workspace, s);
    return launch<MHMR_DT_BF16>(hid16, ldh, ctx16, ldx, w2, b2, g_scores, rows, C, clamped, g_w1, g_b1, g_w2, g_b2, workspace, s);
}

}  // extern "C"
