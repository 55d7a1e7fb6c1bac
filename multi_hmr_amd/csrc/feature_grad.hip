// Heads from stored features: the entry that puts a caller's features where the backbone would have left them,
// and the plain form of the product that carries the heads' cotangents back to the features.
//   mhmr_features_to_context   feat32 = features, ctx16[:, :C] = op16(features): the two buffers everything behind the backbone reads
//   mhmr_rows_times_weight     out[m][c] (+)= sum_n left[m][n] w16[n][c], the kernel of row_sums.h with an fp32 left operand
// The decoder's dense term (hph_bwd.hip) and the detector's (detect_bwd.hip) launch the same kernel template with their own left operands.
#include "mhmr_common.h"
#include "mhmr_internal.h"
#include "row_sums.h"

namespace {

// one thread per element; the conversion is the cast the final LayerNorm applies to the stored fp32 value (round to nearest even)
template <int DT>
__global__ __launch_bounds__(256) void features_to_context_kernel(const float* features, float* feat32, void* __restrict__ ctx16_, int ldctx,
                                                                  size_t total, int C, bool copy) {
    typedef typename Op<DT>::T T;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / C;
    const int c = (int)(i - row * C);
    const float v = features[i];
    if (copy) feat32[i] = v;
    ((T*)ctx16_)[row * ldctx + c] = (T)v;
}

}  // namespace

extern "C" {

int mhmr_features_to_context(const float* features, float* feat32, void* ctx16, int ldctx, int rows, int C, int dtype, void* stream) {
    if (rows < 0) return MHMR_ERR_BAD_ARG;
    if (C <= 0 || ldctx < C || (dtype != MHMR_DT_F16 && dtype != MHMR_DT_BF16)) return MHMR_ERR_BAD_SHAPE;
    const unsigned long long total = (unsigned long long)rows * (unsigned long long)C;
    if (total >= 0xFFFFFF00ULL) return MHMR_ERR_BAD_SHAPE;      // one thread per element: the launch's thread count stays below 2^32
    if (rows == 0) return 0;
    if (!features || !feat32 || !ctx16) return MHMR_ERR_BAD_ARG;
    const bool copy = features != feat32;
    if (copy) {      // the same buffer is fine (nothing to copy); any other overlap would read what this launch writes
        const char *a = (const char*)features, *b = (const char*)feat32;
        if (a < b + total * 4 && b < a + total * 4) return MHMR_ERR_BAD_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == MHMR_DT_F16)
        hipLaunchKernelGGL((features_to_context_kernel<MHMR_DT_F16>), grid, dim3(256), 0, s, features, feat32, ctx16, ldctx, (size_t)total, C, copy);
    else
        hipLaunchKernelGGL((features_to_context_kernel<MHMR_DT_BF16>), grid, dim3(256), 0, s, features, feat32, ctx16, ldctx, (size_t)total, C, copy);
    MHMR_CHECK_LAUNCH();
    return 0;
}

int mhmr_rows_times_weight(const float* left, int ldl, const void* w16, int ldw, float* out, int ldo, int rows, int n, int C, int accumulate,
                           int dtype, void* stream) {
    TRY(rows_times_weight_shape_rc(rows, n, C));
    if (ldl < n || ldw < C || ldo < C || (dtype != MHMR_DT_F16 && dtype != MHMR_DT_BF16)) return MHMR_ERR_BAD_SHAPE;
    if (rows == 0) return 0;
    if (!left || !w16 || !out) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    const LeftF32 lf{left, ldl};
    if (dtype == MHMR_DT_F16) return launch_rows_times_weight<MHMR_DT_F16>(lf, w16, ldw, out, ldo, rows, n, C, accumulate != 0, s);
    return launch_rows_times_weight<MHMR_DT_BF16>(lf, w16, ldw, out, ldo, rows, n, C, accumulate != 0, s);
}

}  // extern "C"
