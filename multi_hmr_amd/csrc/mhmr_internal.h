// Internal (non-ABI) declarations shared by the translation units of libmhmr.so: the launch-argument structs and, at the end, the ONLY
// declaration of every function that one .hip file defines and another calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mhmr.h"

enum GemmEpilogue {
    EPI_OP16 = 0,       // out16[m][n] = acc + bias
    EPI_OP16_GELU = 1,  // out16[m][n] = gelu(acc + bias)
    EPI_OP16_RELU = 2,  // out16[m][n] = relu(acc + bias)
    EPI_RESID = 3,      // out32[m][n] += gamma[n] * (acc + bias[n])        (LayerScale + residual, in place)
    EPI_PATCH = 4,      // out32[row(m)][n] = acc + bias + pos[1 + m % Np][n],  row(m) = (m / Np) * Tp + 1 + m % Np
    EPI_F32 = 5,        // out32[m][n] = acc (+ bias)
    EPI_VT = 6,         // vt[b][h][d][swap23(t)] = acc + bias               (V^T for the attention kernel)
    EPI_OP16_QK = 7,    // out16[m][n] = (acc + bias) * (n < N/2 ? MHMR_ATTN_QSCALE : 1)   (Q | K projection, softmax scale folded into Q)
};

struct GemmArgs {
    const void* A; int lda;
    const void* W; int ldw;
    int M, N, K;
    const float* bias;
    const float* gamma;
    void* out; int ldo;
    const float* pos;
    int Np, Tp, H, Mvalid;
    int epi;
    int stagger_ticks = 0;   // gemm256: CU quarter q starts q * stagger_ticks (100 MHz wall clock) late
    // Token-row map of the activation / output rows (ViT blocks): logical row m = b * img_rows + n lives at physical row
    // b * img_stride + n.  The big linears then run over the B * N patch rows only (exactly 8 / 16 / 32 rounds of 256 tiles at
    // 896^2 x 32) and skip the class + padding rows of every image (vit_cls.hip computes the class rows).  0 = rows are physical.
    int img_rows = 0, img_stride = 0;
    unsigned img_magic = 0;  // floor(2^32 / (img_rows / 256)) + 1 (0 when img_rows == 256), set by mhmr_launch_gemm: image of row tile tm = umulhi(tm, img_magic)
    // Low-half weight pass: W = [W_hi | W_lo] along k (ldw >= K, K = 2 * a_k): k tiles >= a_k / 64 re-read the activation's k tiles
    // from the start, so acc = A . W_hi^T + A . W_lo^T in one accumulator chain.  0 = off.
    // K = 3 * a_k (the f16x3 precision mode): W = [W_hi | W_lo | W_hi], A = [A_hi | A_lo] (lda >= 2 a_k): the k tiles of the third range
    // read the activation's SECOND a_k columns, so acc = A_hi W_hi^T + A_hi W_lo^T + A_lo W_hi^T -- three 16-bit products per term.
    int a_k = 0;
    // fp8 low-half range (gemm256 only; the weight's LOW half needs three significant bits, not eleven).  lo8 != 0: BOTH operand rows are
    // [a_k op16 values | a_k bytes of fp8] (lda, ldw >= K = a_k + a_k / 2 in 16-bit units), and the k tiles behind a_k are 128-deep fp8 tiles
    // on v_mfma_scale_f32_16x16x128_f8f6f4 (twice the 16-bit rate) -- same 16 KiB half-tile slots, same copies, same fragment reads, no
    // activation wrap-around: only the MFMA differs.  Weight bytes: e4m3 of W_lo * 2^-e with w8_scale = 127 + e (E8M0); activation bytes:
    // bf8 (e5m2) of the SAME values as the 16-bit part, unscaled, written by the activation's producer (x8_off below; attention's out8).
    int lo8 = 0;
    int w8_scale = 127;
    // producer side (EPI_RESID with x16): row pitch of x16 in elements (0 = ldo) and, if x8_off > 0, the byte offset inside an x16 row where
    // the bf8 copy of the row's N values goes (the next linear's fp8 low-half range)
    int ldx16 = 0, x8_off = 0;
    int colgroup = 0;        // gemm256: column-group tile order for wide outputs: log2 of the weight column panels an XCD keeps (2 = four panels, 3 = eight; 0 = off); set by mhmr_launch_gemm, MHMR_COLGROUP overrides
    // LayerNorm folded into the neighbouring GEMMs (gemm256 only): the LayerNorm pass of its own disappears.
    //   producer (EPI_RESID): besides the fp32 residual rows it writes x16 = their 16-bit copy (RAW, un-normalised: the next linear's A
    //   operand) and pstats[row][N / 64][2] = (sum, sum of squares) of every 64-column block of the row (summed over the row by
    //   ln_stats_kernel -> rowstats[row] = (mean, rstd));
    //   consumer (EPI_OP16_QK / EPI_VT / EPI_OP16_GELU with rowstats != null): W carries the LayerNorm weight (W' = W diag(w_ln)),
    //   out = rstd_m * (acc - mean_m * colsum_n) + fbias_n,  colsum_n = sum_k W'[n][k],  fbias = b + W . b_ln;  `bias` must be null.
    void* x16 = nullptr;
    float* pstats = nullptr;
    const float* rowstats = nullptr;
    const float* colsum = nullptr;
    const float* fbias = nullptr;
    // Split-k (gemm256 only, EPI_F32, no bias): ksplit > 0 = k tiles (of 64) per slice, nslices slices; slice s writes its fp32 partial
    // product into out + s * M * ldo (ldo == N).  For launches of fewer tiles than half the CUs (mhmr_splitk_plan, capi.hip).
    int ksplit = 0, nslices = 0;
    // Masked output width (gemm256 only, EPI_RESID / EPI_VT): n_valid > 0 and != N: the real width, N - 128 (N = roundup(n_valid, 256));
    // W and every per-column array (bias, gamma, colsum, fbias) must be readable -- zero-padded -- up to N; `out`, x16 and pstats have the
    // real width (ldo = n_valid or wider; pstats[row][n_valid / 64][2]); the V^T output has n_valid / 64 heads.
    int n_valid = 0;
    // Merged qkv linear (gemm256 only, EPI_OP16_QK): out2 != null: output columns >= split_col go row-major to out2 [M, ldo2] (column
    // n - split_col), the others to out; the softmax scale applies to columns < qcols.
    void* out2 = nullptr;
    int ldo2 = 0, split_col = 0, qcols = 0;
};

// physical row of logical activation row m (see GemmArgs::img_rows)
__host__ __device__ inline long long mhmr_phys_row(int m, int img_rows, int img_stride) {
    return img_rows > 0 ? (long long)(m / img_rows) * img_stride + (m % img_rows) : (long long)m;
}

// Per-DEVICE one-time kernel attributes (hipFuncAttributeMaxDynamicSharedMemorySize is a property of the function ON A DEVICE: a process
// that drives a second GPU must set it there too).  One bit per device id in a launcher-local mask; setting an attribute twice from two
// host threads is harmless, so a relaxed fetch_or is enough.  Device ids >= 64 set the attribute on every call.
#include <atomic>
struct DeviceOnce {
    std::atomic<uint64_t> done{0};
    // -> the current device id if the caller must (re)apply its attribute there, -1 if already applied, -2 on a HIP error
    int need(int* dev_out) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return -2;
        *dev_out = dev;
        if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_relaxed) >> dev) & 1ull)) return -1;
        return dev;
    }
    void mark(int dev) { if (dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_relaxed); }
};
// "Any-order" launches (hipExtAnyOrderLaunch: the AQL packet goes out WITHOUT the barrier bit, so the command processor does not wait for
// the previous kernel of the stream to finish before dispatching this one).  capi.hip sets the thread-local flag around launches whose
// inputs were complete before the PREVIOUS launch started and whose outputs nothing touches until the next ordinary launch (which waits
// for everything before it): the V projection behind the Q | K projection, the class-row linears behind the big GEMM of the same
// linear.  MEASURED (round 6, tools/ubench/anyorder.hip + a kernel trace of the forward, profiles/r06_session_a.txt / _b.txt): on gfx950 /
// ROCm 7.2 such a kernel starts about when the kernel in front of it ends -- a persistent GEMM holds every CU until then, so nothing
// overlaps for long (the trace shows ~8 boundaries per forward where the next kernel starts 0.1-0.2 us BEFORE its predecessor's end;
// hip_ext.h calls the flag "not supported on GFX9xx") -- but the ordering IS relaxed: a class-row launch that also read the block sums
// of the GEMM in front of it, launched this way by mistake for one session, returned wrong, run-to-run different statistics.  The
// headline step is 0.1-0.8 % faster in six of six interleaved A/B pairs.  On by default, ONLY for launches independent of their predecessor.  MHMR_ANYORDER=0 switches it off (A/B measurements); never set while a stream is being captured.
extern thread_local int g_mhmr_anyorder;
#include <hip/hip_ext.h>
template <typename F, typename... Args>
inline void mhmr_launch_kernel(F kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    if (g_mhmr_anyorder) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, s, nullptr, nullptr, hipExtAnyOrderLaunch, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

// The class-row linear (vit_cls.hip): the kernels' argument.
struct ClsArgs {
    const void* A = nullptr; long long a_stride = 0;      // activation row b at A + b * a_stride (elements); k contiguous
    const void* W = nullptr; int ldw = 0;                 // [N][ldw] weight rows (k contiguous)
    int B = 0, N = 0, K = 0, a_k = 0;                     // K = total k (2 * a_k with a low-half weight pass: A's k index wraps at a_k), K % 128 == 0
    const float* bias = nullptr; const float* gamma = nullptr;
    void* out = nullptr; long long o_stride = 0;          // output row b at out + b * o_stride (elements of the output type)
    int n_base = 0, C = 0;                                // CLS_QKV: global column of local column 0; embed dim (column regions Q | K | V)
    void* vt = nullptr; int H = 0, Tp = 0, vcol = 0;      // CLS_QKV: V^T [B][H][64][Tp], the (already key-permuted) column of the class token
    // LayerNorm fold (GemmArgs above): consumer side -- rowstats (mean, rstd) of row b at rowstats + b * rs_stride floats,
    // out = rstd * (acc - mean * colsum_n) + fbias_n (bias null); producer side (CLS_RESID) -- x16: 16-bit copy of the updated rows
    const float* rowstats = nullptr; long long rs_stride = 0; const float* colsum = nullptr; const float* fbias = nullptr;
    void* x16 = nullptr; long long x_stride = 0;
    // Row statistics carried by the class-row launches (round 6).  Class-row block sums: CLS_RESID writes cls_pstats[row][N / 16][2]; a
    // consumer (CLS_QKV / CLS_GELU) with cls_pstats != null takes (mean, rstd) of its rows from them (cls_nblk = the producing linear's
    // N / 16 = embed_dim / 16, cls_C = embed_dim) instead of from `rowstats`
    float* cls_pstats = nullptr; int cls_nblk = 0, cls_C = 0; float cls_eps = 1e-6f;
    // statistics role (CLS_RESID only): the patch rows' statistics as st_blocks extra workgroups at blockIdx.x >= N / 16, which run
    // ln_stats_patch_rows over st_B images x st_N patch rows of st_Tp-row images (st_pstats = the big GEMM's block sums, st_rowstats = its
    // consumers' (mean, rstd)).  st_blocks is derived by mhmr_launch_cls_linear.
    const float* st_pstats = nullptr; float* st_rowstats = nullptr; int st_blocks = 0, st_B = 0, st_N = 0, st_Tp = 0, st_C = 0;
};
// epilogues of the class-row linear: CLS_QKV = Q | K | V projection of the class rows (Q pre-scaled, V scattered into column `vcol` of V^T),
// CLS_RESID = out32 += gamma * (acc + bias), CLS_GELU = out16 = gelu(acc + bias)
enum { CLS_QKV = 0, CLS_RESID = 1, CLS_GELU = 2 };

// ---- per-kernel-family hipEvent profiling (bench.py roofline leg) ----
enum ProfKind { PROF_GEMM = 0, PROF_ATTN = 1, PROF_LBS = 2, PROF_KINDS = 3 };

#define TRY(expr)                   \
    do {                            \
        int rc__ = (expr);          \
        if (rc__ != 0) return rc__; \
    } while (0)

// The shape rule of the training attention (tape and backward, fp32 and bf16) and of the block backward around it: heads of 64, Tp rows
// per image in workgroups of 64, (Tp / 64, H, B) as the launch grid.  Each entry point adds its own.
inline int mhmr_attention_shape_rc(int B, int T, int Tp, int C, int H) {
    if (B < 0 || T < 0 || Tp < 0 || C < 0 || H < 0) return MHMR_ERR_BAD_ARG;
    if (B == 0 || T == 0 || Tp % 64 || Tp < T || C != 64 * H || H > 65535 || B > 65535) return MHMR_ERR_BAD_SHAPE;
    return 0;
}

// ================================================================================================================================
// Every function one translation unit defines and another calls, by defining file.  Default arguments live here, once.
// ================================================================================================================================
// ---- capi.hip
void prof_begin(int kind, hipStream_t s);
void prof_end(int kind, hipStream_t s, double work);

// ---- gemm.hip
int mhmr_launch_gemm(const GemmArgs& g, int dtype, hipStream_t s);
int mhmr_cu_count();      // multiProcessorCount of the CURRENT device (cached per device id)
bool mhmr_splitk_plan(int M, int N, int K, int* ksplit, int* nslices);
bool mhmr_splitk_plan_on(int ncu, int M, int N, int K, int* ksplit, int* nslices);

// ---- gemm256.hip
bool mhmr_gemm256_eligible(const GemmArgs& g);
int mhmr_launch_gemm256(const GemmArgs& g, int dtype, hipStream_t s);

// ---- attention.hip
int mhmr_launch_attention(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, int* flags, hipStream_t s,
                          int ldo = 0, int o8 = 0);
int mhmr_launch_attention_ex(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, float limit_log2,
                             int variant, int* flags, hipStream_t s);
int mhmr_attention_flag_count_impl(int B, int Tp, int H);

// ---- attention_f32.hip
int mhmr_launch_attention_f32(const float* qkv, void* out, int B, int T, int Tp, int C, int H, int dtype, hipStream_t s);
// the exact-fp32 attention tape and backward; arguments validated by the caller as the extern "C" entries do; ws holds
// mhmr_attention_f32_bwd_bytes(B, Tp, C)
long long mhmr_attention_f32_bwd_bytes(int B, int Tp, int C);
int mhmr_launch_attention_f32_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, hipStream_t s);
int mhmr_launch_attention_f32_bwd(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                  int Tp, int C, int H, void* ws, hipStream_t s);

// ---- vit_misc.hip
int mhmr_launch_im2col(const float* x, void* a, int B, int S, int G, int Kp, int dtype, hipStream_t s);
int mhmr_launch_im2col_pair(const float* x, void* a, int B, int S, int G, int Kp, int dtype, hipStream_t s);
int mhmr_launch_init_rows(float* resid, const float* cls_pos0, int B, int T, int Tp, int C, hipStream_t s);
int mhmr_launch_layernorm(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype, hipStream_t s);
int mhmr_launch_layernorm_pitch(const float* in, const float* w, const float* b, void* out16, int ld16, int o8, int rows, int C, float eps,
                                int dtype, hipStream_t s);
int mhmr_launch_layernorm_pair(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype,
                               hipStream_t s);
int mhmr_launch_gelu_pair(const float* in, void* out, long long M, int N, int dtype, hipStream_t s);
int mhmr_launch_vt_transpose(const void* v, int ldv, void* vt, int B, int Tp, int H, int dtype, hipStream_t s);
int mhmr_launch_splitk_resid(const float* part, int nslices, int rows, int C, const float* bias, const float* gamma, float* resid, void* x16,
                             int ldx, float* rowstats, float eps, int dtype, hipStream_t s);
int mhmr_launch_ln_stats(const float* pstats, const float* resid, float* rowstats, int B, int N, int Tp, int C, float eps, hipStream_t s);
int mhmr_launch_final_norm(const float* resid, const float* w, const float* b, void* ctx16, int ldctx, float* feat32, int B, int Np, int Tp,
                           int C, float eps, int dtype, hipStream_t s);

// ---- vit_cls.hip
int mhmr_launch_cls_linear(const ClsArgs& a, int epi, int dtype, hipStream_t s);

// ---- hph.hip (the person head; its extern "C" entry points are defined there too)
int mhmr_launch_linear_f32(const float* X, int ldx, const int* row_idx, const float* W, int ldw, const float* bias, const float* R, int ldr,
                           float* Y, int ldy, int M, int N, int K, int act, hipStream_t s);
int mhmr_launch_layernorm_f32(const float* in, const float* w, const float* b, float* out, int rows, int C, float eps, hipStream_t s);
// ---- linear_bf16.hip (bf16 operands, fp32 accumulation; arguments validated by the caller: M, N, K multiples of 64, leading dimensions
// multiples of 4, 16-byte aligned pointers; ws holds mhmr_linear_bf16_bytes(M, N, K), which grows with each of M, N and K)
long long mhmr_linear_bf16_bytes(long long M, int N, int K);
// the bf16 copy of an fp32 matrix [rows, cols] (multiples of 64; ld % 4 == 0): as it lies, out [rows, cols], or transposed, out [cols, rows]
void mhmr_launch_to_bf16(const float* in, int ld, __bf16* out, int rows, int cols, bool transposed, hipStream_t s);
int mhmr_launch_linear_bf16(const float* X, int ldx, const float* W, int ldw, const float* bias, float* Y, int ldy, int M, int N, int K, void* ws,
                            hipStream_t s);
int mhmr_launch_linear_bf16_bwd_input(const float* dY, int lddy, const float* W, int ldw, const float* dR, int lddr, float* dX, int lddx, int M, int N,
                                      int K, void* ws, hipStream_t s);
int mhmr_launch_linear_bf16_bwd_weight(const float* dY, int lddy, const float* X, int ldx, float* dW, int lddw, float* db, int M, int N, int K, void* ws,
                                       hipStream_t s);

// ---- attention_bf16.hip (the attention tape and backward with bf16 operands; arguments validated by the caller as the extern "C" entries
// do; ws holds mhmr_attention_bf16_bytes(B, Tp, C).  qkv_ready: the tape has run on this workspace with this qkv, its bf16 copy is kept)
long long mhmr_attention_bf16_bytes(int B, int Tp, int C);
int mhmr_launch_attention_bf16_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* ws, hipStream_t s);
int mhmr_launch_attention_bf16_bwd(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv, int B, int T,
                                   int Tp, int C, int H, void* ws, bool qkv_ready, hipStream_t s);

// ---- hph.hip, continued
// The shape rules of the decoder stack and of the whole head that forward and backward share (each entry point adds its own).
bool mhmr_hph_stack_shape_ok(int dim, int heads, int mlp, int Kc);
bool mhmr_hph_head_shape_ok(const mhmr_hph_desc* d);
// One decoder layer, for the forward (in place: the x_* all alias, the temporaries are reused) and for the backward's tape (distinct
// buffers).  z1 != null: also the feed-forward's pre-activation (a second ff1 launch without GELU); x_out == null: no ff2.
struct HphStack {
    int dim, heads, mlp, Kc, N, B, dtype, P;
    const void* ctx16;
    const int* gstart; int ngroups, nmax;
    const int* chunks; int nchunks;
};
struct HphLayerBufs {
    const float* x_sa;                  // inputs of the three sub-blocks
    float *x_ca, *x_ff, *x_out;
    float *xn, *qkv, *o_sa, *q, *o_ca, *kv, *h1, *z1;
};
int mhmr_launch_hph_layer(const HphStack& t, const mhmr_hph_layer& W, const HphLayerBufs& b, hipStream_t s);
int mhmr_launch_to_kv(const HphStack& t, const mhmr_hph_layer& W, float* kv, hipStream_t s);      // kv [roundup(B N, 128), 2 inner] = ctx16 . to_kv16^T
