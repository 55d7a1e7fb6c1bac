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
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "hph_shared.h"

namespace {

constexpr int COL_SLICE = 512;                            // rows per first-stage slice of the column sums
constexpr int W1_SLICES = 16;                             // upper bound of the row slices of the dW1 product
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
        dl64[row - row0] = d;
    }
}

// ------------------------------------------------------------------------------------------------------------
// Column sums, stage 1, slices sl0 + blockIdx.y: part[slice][c] = (sum dl hid16, sum dl [hid16 > 0]) over the slice's COL_SLICE rows in
// index order (fp64, from dl64 of the rows row0 ...); one thread per column pair.  Thread 0 of column block 0 also leaves the slice's sum
// of dl in pb2[slice].
// ------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(64) void detect_cols1_kernel(const void* __restrict__ hid_, int ld, const double* __restrict__ dl64,
                                                          double* __restrict__ part, double* __restrict__ pb2, int sl0, int row0, int rows,
                                                          int C) {
    typedef typename Op<DT>::T T;
    typedef typename Op<DT>::V2 V2;
    const int c = blockIdx.x * 128 + threadIdx.x * 2, sl = sl0 + blockIdx.y;
    const int r0 = sl * COL_SLICE, r1 = min(r0 + COL_SLICE, rows);
    const T* hp = (const T*)hid_ + c;
    double aw[2] = {0.0, 0.0}, ab[2] = {0.0, 0.0}, sd = 0.0;
    for (int r = r0; r < r1; ++r) {
        const V2 h = *(const V2*)(hp + (size_t)r * ld);
        const double d = dl64[r - row0];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float hv = (float)h[e];
            aw[e] += d * (double)hv;
            ab[e] += hv > 0.f ? d : 0.0;
        }
        sd += d;
    }
    double* pp = part + ((size_t)sl * C + c) * 2;
    pp[0] = aw[0]; pp[1] = ab[0]; pp[2] = aw[1]; pp[3] = ab[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) pb2[sl] = sd;
}

// stage 2: the slices in index order; db1 takes its factor w2[n] here.  nsl == 0 (no rows) writes zeros.
__global__ __launch_bounds__(64) void detect_cols2_kernel(const double* __restrict__ part, const double* __restrict__ pb2,
                                                          const float* __restrict__ w2, float* __restrict__ g_w2, float* __restrict__ g_b1,
                                                          float* __restrict__ g_b2, int nsl, int C) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int sl = 0; sl < nsl; ++sl) {
        a += part[((size_t)sl * C + c) * 2];
        b += part[((size_t)sl * C + c) * 2 + 1];
    }
    g_w2[c] = (float)a;
    g_b1[c] = nsl > 0 ? (float)((double)w2[c] * b) : 0.f;
    if (c == 0) {
        double s = 0.0;
        for (int sl = 0; sl < nsl; ++sl) s += pb2[sl];
        g_b2[0] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------------------
// dW1 product: part[slice][n][c] = sum over the slice's rows of (hid16[row][n] > 0 ? dl[row] : 0) * ctx16[row][c].  grad_ctx_gemm_kernel's
// form: workgroup = 64 (n) x 128 (c), four waves of 32 x 64 (2 x 4 MFMA tiles); four rows per MFMA, rows in index order; rows past the
// slice's end contribute an exact zero (their addresses are clamped into the slice, so nothing behind `rows` is read).
// ------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void detect_w1_gemm_kernel(const void* __restrict__ hid_, int ldh, const void* __restrict__ ctx_, int ldx,
                                                             const float* __restrict__ dl, float* __restrict__ part, int rows, int C,
                                                             int slice_rows) {
    typedef typename Op<DT>::T T;
    const T* hid = (const T*)hid_;
    const T* ctx = (const T*)ctx_;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, l15 = lane & 15;
    const int n0 = blockIdx.y * 64 + (w & 1) * 32, c0 = blockIdx.x * 128 + (w >> 1) * 64;      // C % 128 == 0: no column is out of range
    const int r0 = blockIdx.z * slice_rows, r1 = min(r0 + slice_rows, rows);
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; r += 4) {
        const int rr = r + g, rc = min(rr, r1 - 1);
        const T* hp = hid + (size_t)rc * ldh + n0 + l15;
        const T* cp = ctx + (size_t)rc * ldx + c0 + l15;
        const float d = rr < r1 ? dl[rc] : 0.f;
        float a[2], bb[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) a[t] = (float)hp[16 * t] > 0.f ? d : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) bb[u] = (float)cp[16 * u];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bb[u], acc[t][u], 0, 0, 0);
    }
    float* pp = part + (size_t)blockIdx.z * C * C;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + 16 * u + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) pp[(size_t)(n0 + 16 * t + 4 * g + r) * C + c] = acc[t][u][r];
        }
}

// finishing pass: the slices in index order (fp64), times w2[n].  nsl == 0 (no rows) writes zeros.
__global__ __launch_bounds__(256) void detect_w1_finish_kernel(const float* __restrict__ part, const float* __restrict__ w2,
                                                               float* __restrict__ g_w1, int nsl, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)C * C;      // C % 128 == 0: total % 256 == 0
    double s = 0.0;
    for (int sl = 0; sl < nsl; ++sl) s += (double)part[(size_t)sl * total + i];
    g_w1[i] = nsl > 0 ? (float)((double)w2[i / C] * s) : 0.f;
}

inline long long align256(long long v) { return (v + 255) / 256 * 256; }
inline int w1_slices(int rows) { return (rows + 511) / 512 < W1_SLICES ? (rows + 511) / 512 : W1_SLICES; }      // 0 for rows == 0
inline int col_slices(int rows) { return (rows + COL_SLICE - 1) / COL_SLICE; }

// workspace: the dW1 slice partials | dl [rows] | the column sums' slice partials (2 C + 1 doubles per slice).  Until the dW1 product
// runs, the region of its partials is the scratch of dl64: at least C C 4 >= 65536 bytes per slice of 512 rows, so it holds the fp64 dl
// of chunk_rows() >= 8192 rows at a time (of all rows unless rows > 8 C C), and the row pass and stage 1 go chunk by chunk.
struct Layout { long long part, dl, cols, pb2, total; };
inline Layout layout(int rows, int C) {
    Layout L;
    L.part = 0;
    L.dl = align256((long long)w1_slices(rows) * C * C * 4);
    L.cols = L.dl + align256(4LL * rows);
    L.pb2 = L.cols + (long long)col_slices(rows) * C * 2 * 8;
    L.total = L.pb2 + align256(8LL * col_slices(rows));
    return L;
}

inline int chunk_rows(int rows, int C) {      // a multiple of COL_SLICE: the slices and their sums do not depend on the chunking
    const long long cap = (long long)w1_slices(rows) * C * C * 4 / 8 / COL_SLICE * COL_SLICE;
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
    const int nsl = w1_slices(rows), ncs = col_slices(rows);
    if (rows > 0) {
        const int chunk = chunk_rows(rows, C);
        for (int row0 = 0; row0 < rows; row0 += chunk) {
            const int row1 = row0 + chunk < rows ? row0 + chunk : rows;
            hipLaunchKernelGGL((detect_dl_kernel<DT>), dim3((row1 - row0 + 3) / 4), dim3(256), 0, s, hid16, ldh, w2, b2, gs, dl, (double*)part, row0,
                               row1, C, clamped);
            hipLaunchKernelGGL((detect_cols1_kernel<DT>), dim3(C / 128, col_slices(row1 - row0)), dim3(64), 0, s, hid16, ldh, (const double*)part,
                               cols, pb2, row0 / COL_SLICE, row0, rows, C);
        }
        const int slice_rows = ((rows + nsl - 1) / nsl + 3) / 4 * 4;
        hipLaunchKernelGGL((detect_w1_gemm_kernel<DT>), dim3(C / 128, C / 64, nsl), dim3(256), 0, s, hid16, ldh, ctx16, ldx, dl, part, rows, C,
                           slice_rows);
    }
    hipLaunchKernelGGL(detect_cols2_kernel, dim3(C / 64), dim3(64), 0, s, cols, pb2, w2, g_w2, g_b1, g_b2, ncs, C);
    hipLaunchKernelGGL(detect_w1_finish_kernel, dim3((unsigned)((size_t)C * C / 256)), dim3(256), 0, s, part, w2, g_w1, nsl, C);
    MHMR_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" {

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
