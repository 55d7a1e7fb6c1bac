// extern "C" entry points of libmhmr.so (declared in include/mhmr.h): the ViT forward orchestration (pure launch sequences on the
// caller's stream, no allocation, no synchronisation) and the hipEvent profiler.  The person head's entry points are in hph.hip.
#include <vector>
#include <mutex>
#include "mhmr_common.h"
#include <stdlib.h>
#include "mhmr_internal.h"
#include "vit_plan.h"

thread_local int g_mhmr_anyorder = 0;        // mhmr_internal.h: the next launches of this host thread go out without the AQL barrier bit
#ifndef MHMR_ANYORDER_DEFAULT
#define MHMR_ANYORDER_DEFAULT 1      // +0.1 ... +0.8 % on the headline step in six of six interleaved A/B pairs (profiles/r06_session_a.txt, _c.txt)
#endif
namespace {
struct AnyOrder {       // scope guard
    explicit AnyOrder(bool on) { g_mhmr_anyorder = on ? 1 : 0; }
    ~AnyOrder() { g_mhmr_anyorder = 0; }
};
}  // namespace

// ------------------------------------------------------------------------------------------------ profiler
namespace {
struct Prof {
    int kind = -1;
    std::vector<hipEvent_t> pool;   // start/stop pairs
    size_t used = 0;
    double work = 0.0;
    std::mutex mu;
} g_prof;

inline hipEvent_t prof_event() {
    if (g_prof.used == g_prof.pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        g_prof.pool.push_back(e);
    }
    return g_prof.pool[g_prof.used++];
}
}  // namespace

void prof_begin(int kind, hipStream_t s) {
    if (g_prof.kind != kind) return;
    hipEvent_t e = prof_event();
    if (e) (void)hipEventRecord(e, s);
}
void prof_end(int kind, hipStream_t s, double work) {
    if (g_prof.kind != kind) return;
    hipEvent_t e = prof_event();
    if (e) (void)hipEventRecord(e, s);
    g_prof.work += work;
}

extern "C" {

int mhmr_version(void) { return MHMR_VERSION; }

#ifndef MHMR_SOURCE_HASH
#define MHMR_SOURCE_HASH "unknown"
#endif
// (the marker prefix lets _lib.built_source_hash() find the value in the file without loading it)
static const char g_source_hash[] = "MHMR_SOURCE_HASH=" MHMR_SOURCE_HASH;
const char* mhmr_source_hash(void) { return g_source_hash + 17; }

int mhmr_prof_enable(int kind) {
    if (kind >= PROF_KINDS) return MHMR_ERR_BAD_ARG;
    g_prof.kind = kind;
    g_prof.used = 0;
    g_prof.work = 0.0;
    return 0;
}

int mhmr_prof_collect(int* launches, double* total_ms, double* total_work) {
    double ms = 0.0;
    const size_t n = g_prof.used / 2;
    for (size_t i = 0; i < n; ++i) {
        hipError_t e = hipEventSynchronize(g_prof.pool[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        float t = 0.f;
        e = hipEventElapsedTime(&t, g_prof.pool[2 * i], g_prof.pool[2 * i + 1]);
        if (e != hipSuccess) return (int)e;
        ms += t;
    }
    if (launches) *launches = (int)n;
    if (total_ms) *total_ms = ms;
    if (total_work) *total_work = g_prof.work;
    g_prof.used = 0;
    g_prof.work = 0.0;
    return 0;
}

int mhmr_gemm16(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, const float* gamma,
                void* out, int ldo, const float* pos, int Np, int Tp, int H, int Mvalid, int epi, int dtype, void* stream) {
    GemmArgs g{A, lda, W, ldw, M, N, K, bias, gamma, out, ldo, pos, Np, Tp, H, Mvalid, epi};
    return mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
}

int mhmr_gemm16_ex(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, const float* gamma,
                   void* out, int ldo, const float* pos, int Np, int Tp, int H, int Mvalid, int epi, int dtype, int img_rows, int img_stride,
                   int a_k, void* stream) {
    GemmArgs g{A, lda, W, ldw, M, N, K, bias, gamma, out, ldo, pos, Np, Tp, H, Mvalid, epi};
    g.img_rows = img_rows;
    g.img_stride = img_stride;
    g.a_k = a_k;
    return mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
}

int mhmr_gemm16_ln(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias, const float* gamma, void* out,
                   int ldo, int Tp, int H, int epi, int dtype, int img_rows, int img_stride, int a_k, void* x16, float* pstats,
                   const float* rowstats, const float* colsum, const float* fbias, void* stream) {
    GemmArgs g{A, lda, W, ldw, M, N, K, bias, gamma, out, ldo, nullptr, 0, Tp, H, M, epi};
    g.img_rows = img_rows;
    g.img_stride = img_stride;
    g.a_k = a_k;
    g.x16 = x16;
    g.pstats = pstats;
    g.rowstats = rowstats;
    g.colsum = colsum;
    g.fbias = fbias;
    return mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
}

int mhmr_gemm16_lo8(const void* A, int lda, const void* W, int ldw, int M, int N, int a_k, int lo8, int w8_scale, const float* bias,
                    const float* gamma, void* out, int ldo, int Tp, int H, int epi, int dtype, int img_rows, int img_stride, void* x16,
                    int ldx16, int x8_off, float* pstats, const float* rowstats, const float* colsum, const float* fbias, void* stream) {
    const int K = lo8 ? a_k + a_k / 2 : a_k;
    GemmArgs g{A, lda, W, ldw, M, N, K, bias, gamma, out, ldo, nullptr, 0, Tp, H, M, epi};
    g.img_rows = img_rows;
    g.img_stride = img_stride;
    g.a_k = lo8 ? a_k : 0;
    g.lo8 = lo8;
    g.w8_scale = w8_scale;
    g.x16 = x16;
    g.ldx16 = ldx16;
    g.x8_off = x8_off;
    g.pstats = pstats;
    g.rowstats = rowstats;
    g.colsum = colsum;
    g.fbias = fbias;
    return mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
}

// mhmr_gemm16_ln with a masked output width (GemmArgs::n_valid): N = n_valid + 128 padded columns that are computed and not stored
int mhmr_gemm16_masked(const void* A, int lda, const void* W, int ldw, int M, int N, int n_valid, int K, int a_k, const float* bias,
                       const float* gamma, void* out, int ldo, int Tp, int H, int epi, int dtype, void* x16, float* pstats,
                       const float* rowstats, const float* colsum, const float* fbias, void* stream) {
    GemmArgs g{A, lda, W, ldw, M, N, K, bias, gamma, out, ldo, nullptr, 0, Tp, H, M, epi};
    g.a_k = a_k;
    g.n_valid = n_valid;
    g.x16 = x16;
    g.pstats = pstats;
    g.rowstats = rowstats;
    g.colsum = colsum;
    g.fbias = fbias;
    if (n_valid <= 0 || n_valid >= N) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
}

// The whole qkv linear of a short batch as ONE launch (gemm256.hip QKV) + the transpose of its V rows: qk [M, 2C] = (Q scaled | K),
// v16 [M, C] (scratch), vt [B][H][64][Tp] key-permuted; M = B * Tp.  rowstats / colsum / fbias: the LayerNorm-fold consumer form (bias NULL).
int mhmr_qkv16(const void* A, int lda, const void* W, int ldw, int B, int Tp, int C, int H, const float* bias, void* qk, void* v16, void* vt,
               int dtype, const float* rowstats, const float* colsum, const float* fbias, void* stream) {
    if (!A || !W || !qk || !v16 || !vt || B <= 0 || C != 64 * H) return MHMR_ERR_BAD_ARG;
    const int M = B * Tp;
    GemmArgs g{A, lda, W, ldw, M, 3 * C, C, bias, nullptr, qk, 2 * C, nullptr, 0, Tp, H, M, EPI_OP16_QK};
    g.out2 = v16; g.ldo2 = C; g.split_col = 2 * C; g.qcols = C;
    g.rowstats = rowstats; g.colsum = colsum; g.fbias = fbias;
    int rc = mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
    if (rc) return rc;
    return mhmr_launch_vt_transpose(v16, C, vt, B, Tp, H, dtype, (hipStream_t)stream);
}

long long mhmr_splitk_workspace_bytes(int M, int N, int K) {
    int ks = 0, S = 0;
    return mhmr_splitk_plan(M, N, K, &ks, &S) ? (long long)S * M * N * 4 : 0;
}

// out32 += gamma * (A . W^T + bias) as a split-k linear (a SHORT launch: mhmr_splitk_workspace_bytes(M, N, K) > 0) + the reduction that also
// leaves x16 / rowstats (either may be NULL)
int mhmr_gemm16_splitk_resid(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int a_k, const float* bias, const float* gamma,
                             float* out32, void* x16, int ldx16, float* rowstats, float eps, float* ws, long long ws_bytes, int dtype,
                             void* stream) {
    int ks = 0, S = 0;
    if (!A || !W || !out32 || !ws) return MHMR_ERR_BAD_ARG;
    if (!mhmr_splitk_plan(M, N, K, &ks, &S)) return MHMR_ERR_BAD_SHAPE;
    if ((long long)S * M * N * 4 > ws_bytes) return MHMR_ERR_BAD_ARG;
    GemmArgs g{A, lda, W, ldw, M, N, K, nullptr, nullptr, ws, N, nullptr, 0, 128, 1, M, EPI_F32};
    g.a_k = a_k;
    g.ksplit = ks;
    g.nslices = S;
    int rc = mhmr_launch_gemm(g, dtype, (hipStream_t)stream);
    if (rc) return rc;
    return mhmr_launch_splitk_resid(ws, S, M, N, bias, gamma, out32, x16, ldx16 > 0 ? ldx16 : N, rowstats, eps, dtype, (hipStream_t)stream);
}

int mhmr_attention16_pitch(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, int* flags, int ldo,
                           int o8, void* stream) {
    if (!flags) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_attention(qk, vt, out, B, T, Tp, C, H, dtype, flags, (hipStream_t)stream, ldo, o8);
}

int mhmr_layernorm16_pitch(const float* in, const float* w, const float* b, void* out16, int ld16, int o8, int rows, int C, float eps,
                           int dtype, void* stream) {
    return mhmr_launch_layernorm_pitch(in, w, b, out16, ld16, o8, rows, C, eps, dtype, (hipStream_t)stream);
}

int mhmr_ln_stats(const float* pstats, const float* resid, float* rowstats, int B, int N, int Tp, int C, float eps, void* stream) {
    return mhmr_launch_ln_stats(pstats, resid, rowstats, B, N, Tp, C, eps, (hipStream_t)stream);
}

int mhmr_cls_linear16(const void* A, long long a_stride, const void* W, int ldw, int B, int N, int K, int a_k, const float* bias,
                      const float* gamma, void* out, long long o_stride, int n_base, int C, void* vt, int H, int Tp, int vcol, int epi,
                      int dtype, void* stream) {
    const ClsArgs a{A, a_stride, W, ldw, B, N, K, a_k, bias, gamma, out, o_stride, n_base, C, vt, H, Tp, vcol};
    return mhmr_launch_cls_linear(a, epi, dtype, (hipStream_t)stream);
}

int mhmr_attention16(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, void* stream) {
    return mhmr_launch_attention(qk, vt, out, B, T, Tp, C, H, dtype, nullptr, (hipStream_t)stream);
}

int mhmr_attention16_ex(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, float limit_log2,
                        int variant, int* flags, void* stream) {
    return mhmr_launch_attention_ex(qk, vt, out, B, T, Tp, C, H, dtype, limit_log2, variant, flags, (hipStream_t)stream);
}

int mhmr_attention_flag_count(int B, int Tp, int H) { return mhmr_attention_flag_count_impl(B, Tp, H); }

int mhmr_layernorm16(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype,
                     void* stream) {
    return mhmr_launch_layernorm(in, w, b, out16, rows, C, eps, dtype, (hipStream_t)stream);
}

int mhmr_attention_f32(const float* qkv, void* out, int B, int T, int Tp, int C, int H, int dtype, void* stream) {
    if (!qkv || !out) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_attention_f32(qkv, out, B, T, Tp, C, H, dtype, (hipStream_t)stream);
}

int mhmr_layernorm16_pair(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype, void* stream) {
    return mhmr_launch_layernorm_pair(in, w, b, out16, rows, C, eps, dtype, (hipStream_t)stream);
}
int mhmr_gelu16_pair(const float* in, void* out16, long long M, int N, int dtype, void* stream) {
    return mhmr_launch_gelu_pair(in, out16, M, N, dtype, (hipStream_t)stream);
}

// The f16x3 precision mode (include/mhmr.h, mhmr_vit_desc.x3): the same block structure with every linear as three 16-bit products per
// term over operand PAIRS, fp32 LayerNorm / GELU / attention / residual.  All B * Tp rows go through every linear (no token-row map, no
// LayerNorm fold, no class-row kernel): this mode buys accuracy, at ~3x the matrix work and a 1/16-rate attention.
// The tap (include/mhmr.h, mhmr_vit_desc.tap): before block l >= tap_first the residual stream goes into slot l - tap_first.  An ordinary
// stream operation: it waits for every launch in front of it, any-order launches included.  NULL: nothing is issued.
static int vit_tap(const mhmr_vit_desc* d, int l, hipStream_t s) {
    if (!d->tap || l < d->tap_first) return 0;
    const size_t n = (size_t)d->B * d->Tp * d->C;
    const hipError_t e = hipMemcpyAsync(d->tap + (size_t)(l - d->tap_first) * n, d->resid, n * sizeof(float), hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : (int)e;
}

static int vit_forward_x3(const mhmr_vit_desc* d, const float* x, float* feat32, void* ctx16, int ldctx, hipStream_t s) {
    const int dt = d->dtype, B = d->B, C = d->C, Tp = d->Tp, M = B * Tp, Kp = d->Kp;
    const int Mp = (B * d->N + 127) / 128 * 128;
    if (!d->qkv32 || !d->hid32 || !d->a_patch || !d->resid || !d->xn || !d->att || !d->hid) return MHMR_ERR_BAD_ARG;
    if (Tp % 128 || Kp % 128) return MHMR_ERR_BAD_SHAPE;
    TRY(mhmr_launch_im2col_pair(x, d->a_patch, B, d->S, d->G, Kp, dt, s));
    TRY(mhmr_launch_init_rows(d->resid, d->cls_pos0, B, d->T, Tp, C, s));
    {
        GemmArgs g{d->a_patch, 2 * Kp, d->patch_w, 3 * Kp, Mp, C, 3 * Kp, d->patch_b, nullptr, d->resid, C, d->pos, d->N, Tp, d->H,
                   B * d->N, EPI_PATCH};
        g.a_k = Kp;
        TRY(mhmr_launch_gemm(g, dt, s));
    }
    for (int l = 0; l < d->L; ++l) {
        const mhmr_vit_block& k = d->blocks[l];
        if (k.flags || k.v_w2 || k.proj_w2) return MHMR_ERR_BAD_ARG;
        TRY(vit_tap(d, l, s));
        // x = x + ls1 * proj(MHSA(norm1(x)))
        TRY(mhmr_launch_layernorm_pair(d->resid, k.ln1_w, k.ln1_b, d->xn, M, C, 1e-6f, dt, s));
        {
            GemmArgs g{d->xn, 2 * C, k.qkv_w, 3 * C, M, 3 * C, 3 * C, k.qkv_b, nullptr, d->qkv32, 3 * C, nullptr, 0, Tp, d->H, M, EPI_F32};
            g.a_k = C;
            TRY(mhmr_launch_gemm(g, dt, s));
        }
        TRY(mhmr_launch_attention_f32(d->qkv32, d->att, B, d->T, Tp, C, d->H, dt, s));
        {
            GemmArgs g{d->att, 2 * C, k.proj_w, 3 * C, M, C, 3 * C, k.proj_b, k.ls1, d->resid, C, nullptr, 0, Tp, d->H, M, EPI_RESID};
            g.a_k = C;
            TRY(mhmr_launch_gemm(g, dt, s));
        }
        // x = x + ls2 * fc2(gelu(fc1(norm2(x))))
        TRY(mhmr_launch_layernorm_pair(d->resid, k.ln2_w, k.ln2_b, d->xn, M, C, 1e-6f, dt, s));
        {
            GemmArgs g{d->xn, 2 * C, k.fc1_w, 3 * C, M, 4 * C, 3 * C, k.fc1_b, nullptr, d->hid32, 4 * C, nullptr, 0, Tp, d->H, M, EPI_F32};
            g.a_k = C;
            TRY(mhmr_launch_gemm(g, dt, s));
        }
        TRY(mhmr_launch_gelu_pair(d->hid32, d->hid, (long long)M, 4 * C, dt, s));
        {
            GemmArgs g{d->hid, 8 * C, k.fc2_w, 12 * C, M, C, 12 * C, k.fc2_b, k.ls2, d->resid, C, nullptr, 0, Tp, d->H, M, EPI_RESID};
            g.a_k = 4 * C;
            TRY(mhmr_launch_gemm(g, dt, s));
        }
    }
    return mhmr_launch_final_norm(d->resid, d->norm_w, d->norm_b, ctx16, ldctx, feat32, B, d->N, Tp, C, 1e-6f, dt, s);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ mhmr_vit_forward: decide, then launch
// vit_switches (the environment) -> vit_form (vit_plan.h: everything decided before the block loop) -> per block: vit_block_ops (which
// weights, which low halves, which launches merge) -> vit_launch (the launches, in stream order).
namespace {

inline bool env_not_zero(const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); }

// (the three layout switches of VitSwitches are the caller's: the forward finds their outcome in the description)
VitSwitches vit_switches() {
    static const VitSwitches once = [] {
        VitSwitches w{};
        w.rowmap = env_not_zero("MHMR_ROWMAP");
        w.gemm128 = getenv("MHMR_GEMM128") != nullptr;
        w.lnfold = env_not_zero("MHMR_LNFOLD");
        w.lo8 = env_not_zero("MHMR_LO8");
        w.anyorder = getenv("MHMR_ANYORDER") ? atoi(getenv("MHMR_ANYORDER")) != 0 : MHMR_ANYORDER_DEFAULT != 0;
        w.qkv_merge = env_not_zero("MHMR_QKV_MERGE");
        w.fc1_rowmap = env_not_zero("MHMR_FC1_ROWMAP");
        return w;
    }();
    VitSwitches w = once;
    w.cls_stats = env_not_zero("MHMR_CLS_STATS");      // (read per call: tests switch it in-process)
    return w;
}

// Any-order launches (mhmr_internal.h) need a stream whose packets the runtime queues as they come: not while the stream is being
// captured, not inside a profiling window (the hipEvent brackets are ordinary packets)
bool stream_takes_anyorder(hipStream_t s) {
    if (g_prof.kind >= 0) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone;
}

// A weight whose rows may carry the low halves behind the high ones ([W_hi | W_lo] along k, one accumulator chain): k = the whole k
// extent (and the row pitch), a_k = where the activation's k index wraps (0: no low half)
struct WeightK { const void* w; int k, a_k; };

// The operands of one block.
struct VitBlockOps {
    int rc = 0;
    bool f1 = false, f2 = false;         // norm1 folded into qkv, norm2 into fc1
    bool vlo8 = false, plo8 = false;     // the V / output projection runs its low half as an fp8 range (v_w8 / proj_w8)
    bool next_f1 = false;                // the next block folds its norm1: this block's fc2 leaves the statistics for it
    bool next_vlo8 = false;              // the next block's V has an fp8 range: this block's fc2 leaves the bf8 copy of its rows
    bool qkv_merged = false, fc1map = false;
    WeightK v{}, proj{};                 // big GEMM: fp8 range, or a second 16-bit range (v_w2 / proj_w2), or the plain weight
    WeightK v_cls{}, proj_cls{};         // the class-row kernel keeps the 16-bit low halves
};

VitBlockOps vit_block_ops(const mhmr_vit_desc* d, const VitForm& f, int l) {
    VitBlockOps o;
    const mhmr_vit_block& k = d->blocks[l];
    const int C = d->C;
    o.rc = MHMR_ERR_BAD_ARG;
    if (!f.fold && k.flags) return o;               // folded weights cannot run through the plain LayerNorm path
    // block 0's norm1 follows the patch embedding, whose epilogue leaves no row statistics: it cannot be folded (include/mhmr.h);
    // a folded linear needs its column sums
    if (l == 0 && (k.flags & 1)) return o;
    if (((k.flags & 1) && !k.qkv_colsum) || ((k.flags & 2) && !k.fc1_colsum)) return o;
    o.rc = 0;
    const bool last = l + 1 == d->L;
    o.f1 = f.fold && (k.flags & 1);
    o.f2 = f.fold && (k.flags & 2);
    o.next_f1 = !last && f.fold && (d->blocks[l + 1].flags & 1);
    o.vlo8 = f.lo8_ranges && k.v_w8;
    o.plo8 = f.lo8_ranges && k.proj_w8;
    o.next_vlo8 = !last && f.lo8_ranges && d->blocks[l + 1].v_w8;
    const void* v_hi = (const char*)k.qkv_w + (size_t)2 * C * C * 2;      // the V rows of the 16-bit qkv weight
    o.v_cls = k.v_w2 ? WeightK{k.v_w2, 2 * C, C} : WeightK{v_hi, C, 0};
    o.proj_cls = k.proj_w2 ? WeightK{k.proj_w2, 2 * C, C} : WeightK{k.proj_w, C, 0};
    o.v = o.vlo8 ? WeightK{k.v_w8, f.pit, C} : o.v_cls;
    o.proj = o.plo8 ? WeightK{k.proj_w8, f.pit, C} : o.proj_cls;
    o.qkv_merged = f.qkv_merge && !k.v_w2 && !o.vlo8;
    o.fc1map = f.fc1map && o.f2;
    return o;
}

// A [B * Tp, ld] activation buffer of esz-byte elements, as the class-row kernel sees it: the class row of image b
struct TokenBuf { void* base; int ld, esz; };
// where the (mean, rstd) / block sums of a class-row launch come from and go to
enum ClsRowStats {
    CLS_ROWS_PLAIN,          // none: bias epilogue
    CLS_ROWS_CONSUME,        // folded LayerNorm: (mean, rstd) of the class rows from rowstats, or (cst) from the class rows' own block sums
    CLS_ROWS_PRODUCE,        // residual epilogue: leaves (cst) the class rows' block sums
    CLS_ROWS_PRODUCE_PATCH,  // ... and extra workgroups turn the block sums of the big GEMM IN FRONT of it into the patch rows' (mean, rstd)
};

// "The class row of every image through one linear": out = epi(in . w^T) over the B class rows of two token buffers.
// bias: the linear's bias (with CLS_ROWS_CONSUME its folded form, beside colsum); gamma: CLS_RESID
ClsArgs cls_rows_linear(const mhmr_vit_desc* d, const VitForm& f, int epi, TokenBuf in, WeightK w, int n, const float* bias,
                        const float* colsum, const float* gamma, TokenBuf out, ClsRowStats st) {
    const int C = d->C, Tp = d->Tp;
    auto cls_row = [&](TokenBuf t) { return (char*)t.base + (size_t)f.cls_row * t.ld * t.esz; };
    ClsArgs a;
    a.A = cls_row(in); a.a_stride = (long long)Tp * in.ld;
    a.W = w.w; a.ldw = w.k; a.B = d->B; a.N = n; a.K = w.k; a.a_k = w.a_k;
    a.bias = bias; a.gamma = gamma;
    a.out = cls_row(out); a.o_stride = (long long)Tp * out.ld;
    a.C = C; a.H = d->H; a.Tp = Tp;
    if (epi == CLS_QKV) { a.vt = d->vt; a.vcol = f.vcol; }
    if (epi == CLS_RESID && f.fold) { a.x16 = cls_row({d->xn, f.pit, 2}); a.x_stride = (long long)Tp * f.pit; }
    if (st == CLS_ROWS_CONSUME) {
        a.bias = nullptr; a.fbias = bias; a.colsum = colsum;
        if (!f.cst) { a.rowstats = d->rowstats + (size_t)f.cls_row * 2; a.rs_stride = 2LL * Tp; }     // (mean, rstd) of image b's class row: + b * 2 Tp
    }
    if (f.cst && st != CLS_ROWS_PLAIN) { a.cls_pstats = d->cls_pstats; a.cls_nblk = C / 16; a.cls_C = C; }
    if (st == CLS_ROWS_PRODUCE_PATCH) {
        a.st_pstats = d->pstats; a.st_rowstats = d->rowstats;
        a.st_B = d->B; a.st_N = d->N; a.st_Tp = Tp; a.st_C = C;
    }
    return a;
}

// ANY_ORDER_IF(on, launch): `launch` goes out without the AQL barrier bit when `on` (mhmr_internal.h).  The ONLY way a launch of the
// forward gets that flag, so this name at a call is the complete list of the launches that may run beside their predecessor: each must
// be independent of the launch in front of it, and nothing may read its output before the next ordinary launch.
#define ANY_ORDER_IF(on, launch) ([&]() -> int { AnyOrder scope(on); return (launch); }())

int vit_launch(const mhmr_vit_desc* d, const VitForm& f, const float* x, float* feat32, void* ctx16, int ldctx, hipStream_t s) {
    const int dt = d->dtype, B = d->B, C = d->C, N = d->N, Tp = d->Tp, M = B * Tp, Mg = f.Mg, pit = f.pit;
    const int Mp = (B * N + 127) / 128 * 128;
    const TokenBuf xn{d->xn, pit, 2}, qk{d->qk, 2 * C, 2}, att{d->att, pit, 2}, hid{d->hid, 4 * C, 2}, resid{d->resid, C, 4};
    // Everything is launched on the caller's stream: the call is re-entrant across streams and capturable.
    // tokens: patch embedding (im2col + GEMM with bias / pos-embed epilogue), class + padding rows
    TRY(mhmr_launch_im2col(x, d->a_patch, B, d->S, d->G, d->Kp, dt, s));
    TRY(mhmr_launch_init_rows(d->resid, d->cls_pos0, B, d->T, Tp, C, s));
    {
        GemmArgs g{d->a_patch, d->Kp, d->patch_w, d->Kp, Mp, C, d->Kp, d->patch_b, nullptr, d->resid, C, d->pos, d->N, Tp, d->H,
                   B * d->N, EPI_PATCH};
        TRY(mhmr_launch_gemm(g, dt, s));
    }
    auto rows = [&](GemmArgs& g) { g.img_rows = f.img_rows; g.img_stride = f.img_stride; };
    auto masked = [&](GemmArgs& g) { if (f.nmask) { g.N = f.Cp; g.n_valid = C; } };
    auto ln_stats = [&]() { return f.rowmap ? mhmr_launch_ln_stats(d->pstats, d->resid, d->rowstats, B, N, Tp, C, 1e-6f, s)
                                            : mhmr_launch_ln_stats(d->pstats, d->resid, d->rowstats, 1, M, M, C, 1e-6f, s); };
    bool stats_fresh = false;            // rowstats already hold the statistics of the current residual rows
    auto resid_linear = [&](GemmArgs& g) -> int {
        int ks = 0, S = 0;
        stats_fresh = false;
        if (f.splitk && !g.lo8 && g.n_valid == 0 && g.x16 && g.ldx16 == 0 && mhmr_splitk_plan(g.M, g.N, g.K, &ks, &S) &&
            (long long)S * g.M * g.N * 4 <= d->splitk_bytes) {
            GemmArgs gs{g.A, g.lda, g.W, g.ldw, g.M, g.N, g.K, nullptr, nullptr, d->splitk, g.N, nullptr, 0, Tp, d->H, g.M, EPI_F32};
            gs.a_k = g.a_k;
            gs.ksplit = ks;
            gs.nslices = S;
            TRY(mhmr_launch_gemm(gs, dt, s));
            TRY(mhmr_launch_splitk_resid(d->splitk, S, g.M, g.N, g.bias, g.gamma, (float*)g.out, g.x16, g.N, d->rowstats, 1e-6f, dt, s));
            stats_fresh = true;
            return 0;
        }
        return mhmr_launch_gemm(g, dt, s);
    };
    // the residual linears under the fold also leave the 16-bit copy of their rows (the next linear's operand) and its block sums
    auto produces = [&](GemmArgs& g) { if (f.fold) { g.x16 = d->xn; g.pstats = d->pstats; g.ldx16 = f.lo8 ? pit : 0; } };
    for (int l = 0; l < d->L; ++l) {
        const mhmr_vit_block& k = d->blocks[l];
        const VitBlockOps b = vit_block_ops(d, f, l);
        if (b.rc) return b.rc;
        TRY(vit_tap(d, l, s));

        // ---- x = x + ls1 * proj(MHSA(norm1(x)))
        if (b.f1) { if (!stats_fresh) TRY(ln_stats()); }
        else TRY(mhmr_launch_layernorm_pitch(d->resid, k.ln1_w, k.ln1_b, d->xn, pit, b.vlo8 ? f.o8 : 0, M, C, 1e-6f, dt, s));
        {
            GemmArgs g{d->xn, pit, k.qkv_w, C, Mg, 2 * C, C, k.qkv_b, nullptr, d->qk, 2 * C, nullptr, 0, Tp, d->H, Mg, EPI_OP16_QK};
            GemmArgs gv{d->xn, pit, b.v.w, b.v.k, Mg, C, b.v.k, k.qkv_b + 2 * C, nullptr, d->vt, 0, nullptr, 0, Tp, d->H, Mg, EPI_VT};
            gv.a_k = b.v.a_k;
            if (b.vlo8) { gv.lo8 = 1; gv.w8_scale = k.v_w8_scale; }
            rows(g); rows(gv);
            masked(gv);
            if (b.f1) {
                g.bias = nullptr; g.rowstats = d->rowstats; g.colsum = k.qkv_colsum; g.fbias = k.qkv_b;
                gv.bias = nullptr; gv.rowstats = d->rowstats; gv.colsum = k.qkv_colsum + 2 * C; gv.fbias = k.qkv_b + 2 * C;
            }
            if (b.qkv_merged) {
                g.N = 3 * C;
                g.out2 = d->v16; g.ldo2 = C; g.split_col = 2 * C; g.qcols = C;
                TRY(mhmr_launch_gemm(g, dt, s));
                TRY(mhmr_launch_vt_transpose(d->v16, C, d->vt, B, Tp, d->H, dt, s));
            } else {
                // V and the class rows of Q | K | V: beside the Q | K projection
                TRY(mhmr_launch_gemm(g, dt, s));
                TRY(ANY_ORDER_IF(f.ao, mhmr_launch_gemm(gv, dt, s)));
                if (f.rowmap) {
                    const ClsRowStats st = b.f1 ? CLS_ROWS_CONSUME : CLS_ROWS_PLAIN;
                    // (Q | K and V separately when V carries a low half: different k extents)
                    const int nqk = k.v_w2 ? 2 * C : 3 * C;
                    const ClsArgs c = cls_rows_linear(d, f, CLS_QKV, xn, {k.qkv_w, C, 0}, nqk, k.qkv_b, k.qkv_colsum, nullptr, qk, st);
                    TRY(ANY_ORDER_IF(f.ao, mhmr_launch_cls_linear(c, CLS_QKV, dt, s)));
                    if (k.v_w2) {
                        ClsArgs cv = cls_rows_linear(d, f, CLS_QKV, xn, b.v_cls, C, k.qkv_b + 2 * C, b.f1 ? k.qkv_colsum + 2 * C : nullptr, nullptr,
                                                     qk, st);
                        cv.n_base = 2 * C;
                        TRY(ANY_ORDER_IF(f.ao, mhmr_launch_cls_linear(cv, CLS_QKV, dt, s)));
                    }
                }
            }
        }
        TRY(mhmr_launch_attention(d->qk, d->vt, d->att, B, d->T, Tp, C, d->H, dt, d->attn_flags, s, pit, b.plo8 ? f.o8 : 0));
        {
            GemmArgs g{d->att, pit, b.proj.w, b.proj.k, Mg, C, b.proj.k, k.proj_b, k.ls1, d->resid, C, nullptr, 0, Tp, d->H, Mg, EPI_RESID};
            g.a_k = b.proj.a_k;
            if (b.plo8) { g.lo8 = 1; g.w8_scale = k.proj_w8_scale; }
            rows(g);
            produces(g);
            masked(g);
            TRY(resid_linear(g));
            if (f.rowmap) {
                // (with cst: + the patch rows' statistics for norm2, when the next linear consumes them.  THAT launch reads the block sums
                // the GEMM in front of it has just written: an ordinary launch, not an any-order one -- session D of round 6 shipped it
                // any-order for one GPU session and the full-size goldens caught the race: scores 2.5e-3, results differing run to run)
                const bool patch_stats = f.cst && b.f2;
                const ClsArgs c = cls_rows_linear(d, f, CLS_RESID, att, b.proj_cls, C, k.proj_b, nullptr, k.ls1, resid,
                                                  patch_stats ? CLS_ROWS_PRODUCE_PATCH : CLS_ROWS_PRODUCE);
                TRY(ANY_ORDER_IF(f.ao && !patch_stats, mhmr_launch_cls_linear(c, CLS_RESID, dt, s)));
                if (patch_stats) stats_fresh = true;
            }
        }

        // ---- x = x + ls2 * fc2(gelu(fc1(norm2(x))))
        if (b.f2) { if (!stats_fresh) TRY(ln_stats()); }
        else TRY(mhmr_launch_layernorm_pitch(d->resid, k.ln2_w, k.ln2_b, d->xn, pit, 0, M, C, 1e-6f, dt, s));
        {
            GemmArgs g{d->xn, pit, k.fc1_w, C, Mg, 4 * C, C, k.fc1_b, nullptr, d->hid, 4 * C, nullptr, 0, Tp, d->H, Mg, EPI_OP16_GELU};
            rows(g);
            if (b.fc1map) { g.M = B * N; g.Mvalid = B * N; g.img_rows = N; g.img_stride = Tp; }
            if (b.f2) { g.bias = nullptr; g.rowstats = d->rowstats; g.colsum = k.fc1_colsum; g.fbias = k.fc1_b; }
            TRY(mhmr_launch_gemm(g, dt, s));
            if (f.rowmap || b.fc1map) {
                const ClsArgs c = cls_rows_linear(d, f, CLS_GELU, xn, {k.fc1_w, C, 0}, 4 * C, k.fc1_b, k.fc1_colsum, nullptr, hid,
                                                  b.f2 ? CLS_ROWS_CONSUME : CLS_ROWS_PLAIN);
                TRY(ANY_ORDER_IF(f.ao, mhmr_launch_cls_linear(c, CLS_GELU, dt, s)));
            }
            GemmArgs g2{d->hid, 4 * C, k.fc2_w, 4 * C, Mg, C, 4 * C, k.fc2_b, k.ls2, d->resid, C, nullptr, 0, Tp, d->H, Mg, EPI_RESID};
            rows(g2);
            produces(g2);
            // the rows this epilogue leaves are the NEXT block's qkv operand: with their bf8 copy if that block's V has an fp8 range
            if (f.fold) g2.x8_off = b.next_vlo8 ? f.o8 : 0;
            masked(g2);
            TRY(resid_linear(g2));
            if (f.rowmap) {
                // (with cst: + the patch rows' statistics for the NEXT block's norm1, when that block folds it: an ordinary launch then)
                const bool patch_stats = f.cst && b.next_f1;
                const ClsArgs c = cls_rows_linear(d, f, CLS_RESID, hid, {k.fc2_w, 4 * C, 0}, C, k.fc2_b, nullptr, k.ls2, resid,
                                                  patch_stats ? CLS_ROWS_PRODUCE_PATCH : CLS_ROWS_PRODUCE);
                TRY(ANY_ORDER_IF(f.ao && !patch_stats, mhmr_launch_cls_linear(c, CLS_RESID, dt, s)));
                if (patch_stats) stats_fresh = true;
            }
        }
    }
    return mhmr_launch_final_norm(d->resid, d->norm_w, d->norm_b, ctx16, ldctx, feat32, B, d->N, Tp, C, 1e-6f, dt, s);
}

// The shape rules of a description and its form: what mhmr_vit_forward runs and what mhmr_vit_form_bits reports.
int vit_form_of(const mhmr_vit_desc* d, hipStream_t s, VitForm* f) {
    if (d->S % 14 || d->G * 14 != d->S || d->N != d->G * d->G || d->T != d->N + 1 || d->Tp % 64 || d->Tp < d->T ||
        d->C != d->H * 64 || d->Kp % 64 || d->Kp < 588 || (d->C != 384 && d->C != 768 && d->C != 1024))
        return MHMR_ERR_BAD_SHAPE;
    if (d->tap && (d->tap_first < 0 || d->tap_first > d->L || !d->resid)) return MHMR_ERR_BAD_ARG;
    if (d->x3) { *f = VitForm{}; f->x3 = true; return 0; }      // vit_forward_x3: none of the choices below exists there
    const VitSwitches w = vit_switches();
    const VitLayout lay{d->B, d->C, d->N, d->Tp, d->cpad, d->lo8, d->pstats && d->rowstats, d->cls_pstats != nullptr, d->splitk != nullptr,
                        d->v16 != nullptr};
    *f = vit_form(lay, w, mhmr_cu_count(), w.anyorder && stream_takes_anyorder(s));
    return f->rc;
}

}  // namespace

extern "C" {

int mhmr_vit_forward(const mhmr_vit_desc* d, const float* x, float* feat32, void* ctx16, int ldctx, void* stream) {
    if (!d || !x || !feat32 || !ctx16) return MHMR_ERR_BAD_ARG;
    hipStream_t s = (hipStream_t)stream;
    VitForm f;
    const int rc = vit_form_of(d, s, &f);
    if (rc) return rc;
    if (f.x3) return vit_forward_x3(d, x, feat32, ctx16, ldctx, s);
    return vit_launch(d, f, x, feat32, ctx16, ldctx, s);
}

int mhmr_vit_form_bits(const mhmr_vit_desc* d, void* stream, unsigned* bits) {
    if (!d || !bits) return MHMR_ERR_BAD_ARG;
    VitForm f;
    const int rc = vit_form_of(d, (hipStream_t)stream, &f);
    if (rc) return rc;
    *bits = vit_form_bits(f);
    return 0;
}

int mhmr_vit_plan(const mhmr_vit_plan_request* rq, mhmr_vit_plan_result* out) {
    if (!rq || !out || rq->B < 0 || rq->C <= 0 || rq->C != 64 * rq->H || rq->N <= 0 || rq->ncu < 0) return MHMR_ERR_BAD_ARG;
    const VitSwitches w = vit_switches_of_mask(rq->switches);
    const VitPack p{rq->C, rq->N, rq->N + 1, rq->B, rq->fold != 0, rq->x3 != 0, rq->lo8 != 0, rq->cpad};
    const int B = p.B, C = p.C, ncu = rq->ncu > 0 || B == 0 ? rq->ncu : mhmr_cu_count();
    mhmr_vit_plan_result r{};
    r.fold_eligible = vit_fold_eligible(C, p.N, w);
    r.lo8_eligible = vit_lo8_eligible(C, w);
    r.Tp = vit_rows_per_image(p, w);
    r.row_map = vit_row_map(p, w);
    r.tiny_batch = vit_tiny_batch(p);
    r.pitch = vit_pitch(p);
    r.need_pstats = vit_need_pstats(p);
    r.need_cls_pstats = vit_need_cls_pstats(p, w);
    if (vit_may_splitk(p, w))
        for (int K = C; K <= 4 * C; K *= 2) {
            int ks = 0, S = 0;
            const long long M = (long long)B * r.Tp;
            if (mhmr_splitk_plan_on(ncu, (int)M, C, K, &ks, &S) && S * M * C * 4 > r.splitk_bytes) r.splitk_bytes = S * M * C * 4;
        }
    r.need_v16 = r.splitk_bytes > 0;      // the merged qkv launch of a short batch leaves the V rows there
    r.attn_flags = p.x3 ? 0 : mhmr_attention_flag_count_impl(B, r.Tp, rq->H);
    // the form: vit_form itself, on a description that offers exactly these workspaces
    VitForm f;
    f.x3 = p.x3;
    if (!p.x3) f = vit_form(VitLayout{B, C, p.N, r.Tp, p.cpad, p.lo8, r.need_pstats != 0, r.need_cls_pstats != 0, r.splitk_bytes > 0, r.need_v16 != 0}, w, ncu, false);
    if (f.rc) return f.rc;
    r.form_bits = vit_form_bits(f);
    *out = r;
    return 0;
}

}  // extern "C"
