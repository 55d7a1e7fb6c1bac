// extern "C" entry points of libmhmr.so (declared in include/mhmr.h): the ViT and HPH forward orchestration
// (pure launch sequences on the caller's stream, no allocation, no synchronisation) and the hipEvent profiler.
#include <vector>
#include <mutex>
#include "mhmr_common.h"
#include <stdlib.h>
#include "mhmr_internal.h"

// launchers defined in the other translation units
int mhmr_launch_attention(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, int* flags, hipStream_t s, int ldo = 0, int o8 = 0);
int mhmr_launch_layernorm_pitch(const float* in, const float* w, const float* b, void* out16, int ld16, int o8, int rows, int C, float eps, int dtype, hipStream_t s);
bool mhmr_gemm256_eligible(const GemmArgs& g);
int mhmr_launch_attention_ex(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, float limit_log2, int variant, int* flags, hipStream_t s);
int mhmr_attention_flag_count_impl(int B, int Tp, int H);
int mhmr_launch_im2col(const float* x, void* a, int B, int S, int G, int Kp, int dtype, hipStream_t s);
int mhmr_launch_init_rows(float* resid, const float* cls_pos0, int B, int T, int Tp, int C, hipStream_t s);
int mhmr_launch_layernorm(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype, hipStream_t s);
int mhmr_launch_final_norm(const float* resid, const float* w, const float* b, void* ctx16, int ldctx, float* feat32, int B, int Np, int Tp, int C, float eps, int dtype, hipStream_t s);
int mhmr_launch_linear_f32(const float* X, int ldx, const int* row_idx, const float* W, int ldw, const float* bias, const float* R, int ldr, float* Y, int ldy, int M, int N, int K, int act, hipStream_t s);
int mhmr_launch_layernorm_f32(const float* in, const float* w, const float* b, float* out, int rows, int C, float eps, hipStream_t s);
int mhmr_launch_scores(const void* hid, int ld, const float* w2, const float* b2, float* scores, int rows, int C, int dtype, hipStream_t s);
int mhmr_launch_detect_count(const float* scores, int B, int G, int nms_kernel, float thr, int* counts, hipStream_t s);
int mhmr_launch_detect_write(const float* scores, int B, int G, int nms_kernel, float thr, const int* base, int* det_b, int* det_y, int* det_x, float* det_score, int cap, hipStream_t s);
int mhmr_launch_person_groups(const int* counts, const int* det_b, int P, int B, int cap, int* base, int* gstart, int ngcap, int* chunks, int nccap, int* info, hipStream_t s);
int mhmr_launch_camera_embed(const float* Kmat, const float* freq, int B, int G, int patch, float* zK, void* ctx16, int Kc, int C, int dtype, int nbands, hipStream_t s);
int mhmr_launch_hph_inputs(const float* feat32, const float* zK, const int* det_b, const int* det_y, const int* det_x, const float* cq_x, const float* cq_y, const float* cv_x, const float* cv_y, const float* init_tail, int ntail, float* zc, float* token, int Ktok, void* ctx16, int Kc, int* det_row, int P, int G, int C, int dtype, const int* nvalid, int cam_dim, hipStream_t s);
int mhmr_launch_hph_self_attn(const float* qkv, const int* gstart, float* out, int ngroups, int nmax, int heads, hipStream_t s);
int mhmr_launch_hph_cross_attn(const float* q, const float* kv, const int* chunks, int nchunks, float* out, int heads, int N, hipStream_t s);
int mhmr_launch_hph_decode(const float* dec, int ldd, int nb, const float* Kmat, const int* det_b, float fn, int nearness, float* rotmat, float* rotvec, float* betas, float* expr, float* dist_pp, float* dist, int P, hipStream_t s);
int mhmr_launch_cls_linear(const void* A, long long a_stride, const void* W, int ldw, int B, int N, int K, int a_k, const float* bias,
                           const float* gamma, void* out, long long o_stride, int n_base, int C, void* vt, int H, int Tp, int vcol, int epi,
                           int dtype, hipStream_t s);
int mhmr_launch_cls_linear_fold(const void* A, long long a_stride, const void* W, int ldw, int B, int N, int K, int a_k, const float* bias,
                                const float* gamma, void* out, long long o_stride, int n_base, int C, void* vt, int H, int Tp, int vcol, int epi,
                                int dtype, const float* rowstats, long long rs_stride, const float* colsum, const float* fbias, void* x16,
                                long long x_stride, hipStream_t s, const ClsStats* st = nullptr);
int mhmr_launch_ln_stats(const float* pstats, const float* resid, float* rowstats, int B, int N, int Tp, int C, float eps, hipStream_t s);
int mhmr_launch_attention_f32(const float* qkv, void* out, int B, int T, int Tp, int C, int H, int dtype, hipStream_t s);
int mhmr_launch_im2col_pair(const float* x, void* a, int B, int S, int G, int Kp, int dtype, hipStream_t s);
int mhmr_launch_layernorm_pair(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype, hipStream_t s);
int mhmr_launch_gelu_pair(const float* in, void* out, long long M, int N, int dtype, hipStream_t s);
int mhmr_launch_splitk_resid(const float* part, int nslices, int rows, int C, const float* bias, const float* gamma, float* resid, void* x16,
                             int ldx, float* rowstats, float eps, int dtype, hipStream_t s);
bool mhmr_splitk_plan(int M, int N, int K, int* ksplit, int* nslices);
int mhmr_launch_vt_transpose(const void* v, int ldv, void* vt, int B, int Tp, int H, int dtype, hipStream_t s);
int mhmr_launch_loc(const float* offset, const int* det_y, const int* det_x, int patch, float* loc, int P, hipStream_t s);

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

#define TRY(expr)                 \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != 0) return rc__; \
    } while (0)

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
    return mhmr_launch_cls_linear(A, a_stride, W, ldw, B, N, K, a_k, bias, gamma, out, o_stride, n_base, C, vt, H, Tp, vcol, epi, dtype,
                                  (hipStream_t)stream);
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

int mhmr_vit_forward(const mhmr_vit_desc* d, const float* x, float* feat32, void* ctx16, int ldctx, void* stream) {
    if (!d || !x || !feat32 || !ctx16) return MHMR_ERR_BAD_ARG;
    if (d->S % 14 || d->G * 14 != d->S || d->N != d->G * d->G || d->T != d->N + 1 || d->Tp % 64 || d->Tp < d->T ||
        d->C != d->H * 64 || d->Kp % 64 || d->Kp < 588 || (d->C != 384 && d->C != 768 && d->C != 1024))
        return MHMR_ERR_BAD_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (d->x3) return vit_forward_x3(d, x, feat32, ctx16, ldctx, s);
    const int dt = d->dtype, B = d->B, C = d->C, N = d->N, Tp = d->Tp, M = B * Tp;
    const int Mp = (B * N + 127) / 128 * 128;
    // Token rows of an image: patches 0..N-1, the class token at row N, zero padding up to Tp (vit_misc.hip).  When the patch rows of
    // an image are whole 256-row tiles and every linear runs on the 256x256 kernel, the five big GEMMs of a block cover the B * N
    // patch rows only (GemmArgs::img_rows: exact tile rounds) and the B class rows go through the skinny kernel (vit_cls.hip);
    // otherwise one GEMM covers all B * Tp rows.  MHMR_ROWMAP=0 forces the latter (A/B measurements).  Everything is launched on the
    // caller's stream: the call is re-entrant across streams and capturable.
    static const bool rowmap_env = !(getenv("MHMR_ROWMAP") && atoi(getenv("MHMR_ROWMAP")) == 0) && !getenv("MHMR_GEMM128");
    // (Tp a multiple of 256 where N is one too -- the row map's own padding is N + 64 -- is the caller saying "all rows": multi_hmr_amd/vit.py
    // pads tiny batches that way, whose launches are latency-bound and not worth six class-row launches per block)
    const bool rowmap = rowmap_env && C % 256 == 0 && N % 256 == 0 && Tp % 256 != 0 && (uint64_t)M * (uint64_t)C * 4u < (1ull << 32);
    const int Mg = rowmap ? B * N : M, ir = rowmap ? N : 0, is = rowmap ? Tp : 0;
    const size_t esz = 2;
    const long long cls_row = (long long)N;                          // the class row inside an image
    const int vcol = (N & ~12) | ((N & 4) << 1) | ((N & 8) >> 1);    // its (key-permuted) V^T column

    // tokens: patch embedding (im2col + GEMM with bias / pos-embed epilogue), class + padding rows
    TRY(mhmr_launch_im2col(x, d->a_patch, B, d->S, d->G, d->Kp, dt, s));
    TRY(mhmr_launch_init_rows(d->resid, d->cls_pos0, B, d->T, Tp, C, s));
    {
        GemmArgs g{d->a_patch, d->Kp, d->patch_w, d->Kp, Mp, C, d->Kp, d->patch_b, nullptr, d->resid, C, d->pos, d->N, Tp, d->H,
                   B * d->N, EPI_PATCH};
        TRY(mhmr_launch_gemm(g, dt, s));
    }
    auto rows = [&](GemmArgs& g) { g.img_rows = ir; g.img_stride = is; };
    // LayerNorm fold (GemmArgs in mhmr_internal.h): needs the token-row map (every block linear on the 256x256 kernel) and the two workspaces
    static const bool fold_env = !(getenv("MHMR_LNFOLD") && atoi(getenv("MHMR_LNFOLD")) == 0);
    // ... or, without the row map (N not a multiple of 256: 1288^2, 518^2), every block linear on the 256x256 kernel over ALL B * Tp rows
    // (Tp a multiple of 256: vit.padded_tokens): the class and padding rows are rows like any other, with block sums of their own
    // (C = 384, ViT-S: the three linears whose output is C wide -- V, proj, fc2 -- run as N = Cp = 512 with the last 128 columns masked,
    // GemmArgs::n_valid; the caller says with mhmr_vit_desc.cpad that their weights and per-column vectors are zero-padded for it)
    const int Cp = (C + 255) / 256 * 256;
    const bool allrows256 = !rowmap && rowmap_env && (C % 256 == 0 || (C % 128 == 0 && d->cpad == Cp)) && M % 256 == 0 &&
                            (uint64_t)M * (uint64_t)C * 4u < (1ull << 32);
    const bool nmask = allrows256 && C % 256 != 0;
    auto masked = [&](GemmArgs& g) { if (nmask) { g.N = Cp; g.n_valid = C; } };
    const bool fold = (rowmap || allrows256) && fold_env && d->pstats && d->rowstats;
    auto ln_stats = [&]() { return rowmap ? mhmr_launch_ln_stats(d->pstats, d->resid, d->rowstats, B, N, Tp, C, 1e-6f, s)
                                          : mhmr_launch_ln_stats(d->pstats, d->resid, d->rowstats, 1, M, M, C, 1e-6f, s); };
    const long long rowC = (long long)Tp * C;
    const float* cls_stats = fold ? d->rowstats + (size_t)cls_row * 2 : nullptr;      // (mean, rstd) of image b's class row: + b * 2 Tp
    // fp8 low-half ranges (mhmr_vit_desc.lo8): the rows of `xn` and `att` are 3C/2 elements wide (the bf8 copy of a row behind its C values)
    static const bool lo8_env = !(getenv("MHMR_LO8") && atoi(getenv("MHMR_LO8")) == 0);
    const bool lo8 = d->lo8 != 0 && C % 256 == 0;
    if (d->lo8 && !lo8) return MHMR_ERR_BAD_SHAPE;
    const int pit = lo8 ? C + C / 2 : C;                        // row pitch of xn / att in elements
    const long long rowP = (long long)Tp * pit;
    const int o8 = 2 * C;                                       // byte offset of the bf8 copy inside such a row
    // does this block's V / output projection run its low half as an fp8 range?  (needs the 256x256 kernel for that launch; MHMR_LO8=0: A/B)
    auto v8 = [&](const mhmr_vit_block& k) { return lo8 && lo8_env && k.v_w8 && (rowmap || allrows256); };
    auto p8 = [&](const mhmr_vit_block& k) { return lo8 && lo8_env && k.proj_w8 && (rowmap || allrows256); };
    // Split-k residual linears (a batch of one: all rows through the 256x256 kernel, 68 / 40 tiles on 256 CUs): the k range is cut so that
    // tiles x slices fill the chip, and the reduction that follows (vit_misc.hip splitk_resid_kernel) runs the residual epilogue AND leaves
    // the row statistics, so the ln_stats launch behind such a linear disappears.  Needs the workspace mhmr_vit_desc.splitk.
    // Any-order launches (mhmr_internal.h): the V projection and the class-row linears are independent of the big GEMM launched right in
    // front of them and nothing reads their outputs before the next ordinary launch; not while the stream is being captured, not inside
    // a profiling window (the hipEvent brackets are ordinary packets)
    static const bool ao_env = getenv("MHMR_ANYORDER") ? atoi(getenv("MHMR_ANYORDER")) != 0 : MHMR_ANYORDER_DEFAULT != 0;
    bool ao = ao_env && g_prof.kind < 0;
    if (ao) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) ao = false;
    }
    // Row statistics inside the class-row launches (vit_cls.hip, round 6): with mhmr_vit_desc.cls_pstats the residual class-row launch of
    // proj / fc2 also carries the patch rows' statistics (extra workgroups) and leaves block sums of the class rows, from which the class-row
    // consumers take (mean, rstd) themselves: no ln_stats launch at all under the token-row map.  MHMR_CLS_STATS=0: the separate launches.
    const bool cls_stats_env = !(getenv("MHMR_CLS_STATS") && atoi(getenv("MHMR_CLS_STATS")) == 0);     // (read per call: tests switch it in-process)
    const bool cst = cls_stats_env && rowmap && fold && !lo8 && d->cls_pstats && C % 128 == 0 && C <= 1024;
    ClsStats cs_consume, cs_produce, cs_produce_stats;
    if (cst) {
        cs_consume.cls_pstats = d->cls_pstats; cs_consume.cls_nblk = C / 16; cs_consume.cls_C = C;
        cs_produce = cs_consume;
        cs_produce_stats = cs_consume;
        cs_produce_stats.st_pstats = d->pstats; cs_produce_stats.st_rowstats = d->rowstats;
        cs_produce_stats.st_B = B; cs_produce_stats.st_N = N; cs_produce_stats.st_Tp = Tp; cs_produce_stats.st_C = C;
    }
    bool stats_fresh = false;            // rowstats already hold the statistics of the current residual rows
    auto resid_linear = [&](GemmArgs& g) -> int {
        int ks = 0, S = 0;
        stats_fresh = false;
        if (allrows256 && fold && d->splitk && !g.lo8 && g.n_valid == 0 && g.x16 && g.ldx16 == 0 && mhmr_splitk_plan(g.M, g.N, g.K, &ks, &S) &&
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
    for (int l = 0; l < d->L; ++l) {
        const mhmr_vit_block& k = d->blocks[l];
        if (!fold && k.flags) return MHMR_ERR_BAD_ARG;               // folded weights cannot run through the plain LayerNorm path
        // block 0's norm1 follows the patch embedding, whose epilogue leaves no row statistics: it cannot be folded (include/mhmr.h);
        // a folded linear needs its column sums
        if (l == 0 && (k.flags & 1)) return MHMR_ERR_BAD_ARG;
        if (((k.flags & 1) && !k.qkv_colsum) || ((k.flags & 2) && !k.fc1_colsum)) return MHMR_ERR_BAD_ARG;
        const bool f1 = fold && (k.flags & 1), f2 = fold && (k.flags & 2);
        // the V and output projections may carry the low halves of their weights ([W_hi | W_lo] along k, one accumulator chain): as an
        // fp8 range of 128-deep k tiles (v_w8 / proj_w8) or as a second 16-bit range (v_w2 / proj_w2)
        const bool vlo8 = v8(k), plo8 = p8(k);
        const void* v_w = vlo8 ? k.v_w8 : k.v_w2 ? k.v_w2 : (const void*)((const char*)k.qkv_w + (size_t)2 * C * C * esz);
        const int v_k = vlo8 ? pit : k.v_w2 ? 2 * C : C, v_ak = (vlo8 || k.v_w2) ? C : 0;
        const void* p_w = plo8 ? k.proj_w8 : k.proj_w2 ? k.proj_w2 : k.proj_w;
        const int p_k = plo8 ? pit : k.proj_w2 ? 2 * C : C, p_ak = (plo8 || k.proj_w2) ? C : 0;
        // the class-row kernel keeps the 16-bit low halves
        const void* v_wc = k.v_w2 ? k.v_w2 : (const void*)((const char*)k.qkv_w + (size_t)2 * C * C * esz);
        const int v_kc = k.v_w2 ? 2 * C : C, v_akc = k.v_w2 ? C : 0;
        const void* p_wc = k.proj_w2 ? k.proj_w2 : k.proj_w;
        const int p_kc = k.proj_w2 ? 2 * C : C, p_akc = k.proj_w2 ? C : 0;
        // x = x + ls1 * proj(MHSA(norm1(x)))
        if (f1) { if (!stats_fresh) TRY(ln_stats()); }
        else TRY(mhmr_launch_layernorm_pitch(d->resid, k.ln1_w, k.ln1_b, d->xn, pit, vlo8 ? o8 : 0, M, C, 1e-6f, dt, s));
        {
            GemmArgs g{d->xn, pit, k.qkv_w, C, Mg, 2 * C, C, k.qkv_b, nullptr, d->qk, 2 * C, nullptr, 0, Tp, d->H, Mg, EPI_OP16_QK};
            GemmArgs gv{d->xn, pit, v_w, v_k, Mg, C, v_k, k.qkv_b + 2 * C, nullptr, d->vt, 0, nullptr, 0, Tp, d->H, Mg, EPI_VT};
            gv.a_k = v_ak;
            if (vlo8) { gv.lo8 = 1; gv.w8_scale = k.v_w8_scale; }
            rows(g); rows(gv);
            masked(gv);
            if (f1) {
                g.bias = nullptr; g.rowstats = d->rowstats; g.colsum = k.qkv_colsum; g.fbias = k.qkv_b;
                gv.bias = nullptr; gv.rowstats = d->rowstats; gv.colsum = k.qkv_colsum + 2 * C; gv.fbias = k.qkv_b + 2 * C;
            }
            // A short batch (all rows, the whole qkv linear at most one round of tiles): ONE launch for Q | K | V + a transpose of the V rows
            // (gemm256.hip QKV), instead of two launches of half a round each.  Needs mhmr_vit_desc.v16 and a V without a low half.
            static const bool qkv_env = !(getenv("MHMR_QKV_MERGE") && atoi(getenv("MHMR_QKV_MERGE")) == 0);
            if (qkv_env && allrows256 && !nmask && d->v16 && !k.v_w2 && !vlo8 && (M / 256) * (3 * C / 256) <= mhmr_cu_count()) {
                g.N = 3 * C;
                g.out2 = d->v16; g.ldo2 = C; g.split_col = 2 * C; g.qcols = C;
                TRY(mhmr_launch_gemm(g, dt, s));
                TRY(mhmr_launch_vt_transpose(d->v16, C, d->vt, B, Tp, d->H, dt, s));
            } else {
            TRY(mhmr_launch_gemm(g, dt, s));
            AnyOrder ao_scope(ao);           // V and the class rows of Q | K | V: beside the Q | K projection
            TRY(mhmr_launch_gemm(gv, dt, s));
            if (rowmap) {
                const char* xr = (const char*)d->xn + (size_t)cls_row * pit * esz;
                char* qr = (char*)d->qk + (size_t)cls_row * 2 * C * esz;
                const float* st = (f1 && !cst) ? cls_stats : nullptr;
                const ClsStats* cs = (f1 && cst) ? &cs_consume : nullptr;
                // (Q | K and V separately when V carries a low half: different k extents)
                const int nqk = k.v_w2 ? 2 * C : 3 * C;
                TRY(mhmr_launch_cls_linear_fold(xr, rowP, k.qkv_w, C, B, nqk, C, 0, f1 ? nullptr : k.qkv_b, nullptr, qr, 2 * rowC, 0, C, d->vt, d->H,
                                                Tp, vcol, 0, dt, st, 2LL * Tp, k.qkv_colsum, k.qkv_b, nullptr, 0, s, cs));
                if (k.v_w2)
                    TRY(mhmr_launch_cls_linear_fold(xr, rowP, v_wc, v_kc, B, C, v_kc, v_akc, f1 ? nullptr : k.qkv_b + 2 * C, nullptr, qr, 2 * rowC, 2 * C, C,
                                                    d->vt, d->H, Tp, vcol, 0, dt, st, 2LL * Tp, f1 ? k.qkv_colsum + 2 * C : nullptr,
                                                    k.qkv_b + 2 * C, nullptr, 0, s, cs));
            }
            }
        }
        TRY(mhmr_launch_attention(d->qk, d->vt, d->att, B, d->T, Tp, C, d->H, dt, d->attn_flags, s, pit, plo8 ? o8 : 0));
        {
            GemmArgs g{d->att, pit, p_w, p_k, Mg, C, p_k, k.proj_b, k.ls1, d->resid, C, nullptr, 0, Tp, d->H, Mg, EPI_RESID};
            g.a_k = p_ak;
            if (plo8) { g.lo8 = 1; g.w8_scale = k.proj_w8_scale; }
            rows(g);
            if (fold) { g.x16 = d->xn; g.pstats = d->pstats; g.ldx16 = lo8 ? pit : 0; }
            masked(g);
            TRY(resid_linear(g));
            if (rowmap) {
                // (with cst: + the patch rows' statistics for norm2, when the next linear consumes them.  THAT launch reads the block sums
                // the GEMM in front of it has just written: an ordinary launch, not an any-order one -- session D of round 6 shipped it
                // any-order for one GPU session and the full-size goldens caught the race: scores 2.5e-3, results differing run to run)
                const ClsStats* cs = !cst ? nullptr : f2 ? &cs_produce_stats : &cs_produce;
                AnyOrder ao_scope(ao && !(cst && f2));
                TRY(mhmr_launch_cls_linear_fold((const char*)d->att + (size_t)cls_row * pit * esz, rowP, p_wc, p_kc, B, C, p_kc, p_akc, k.proj_b, k.ls1,
                                                d->resid + (size_t)cls_row * C, rowC, 0, C, nullptr, d->H, Tp, 0, 1, dt, nullptr, 0, nullptr, nullptr,
                                                fold ? (char*)d->xn + (size_t)cls_row * pit * esz : nullptr, rowP, s, cs));
                if (cst && f2) stats_fresh = true;
            }
        }
        // x = x + ls2 * fc2(gelu(fc1(norm2(x))))
        if (f2) { if (!stats_fresh) TRY(ln_stats()); }
        else TRY(mhmr_launch_layernorm_pitch(d->resid, k.ln2_w, k.ln2_b, d->xn, pit, 0, M, C, 1e-6f, dt, s));
        {
            GemmArgs g{d->xn, pit, k.fc1_w, C, Mg, 4 * C, C, k.fc1_b, nullptr, d->hid, 4 * C, nullptr, 0, Tp, d->H, Mg, EPI_OP16_GELU};
            rows(g);
            // One 896^2 image over all rows is 17 row tiles x 16 column tiles = 272 tiles: one round of the chip + 16 tiles that cost a second.
            // When the PATCH rows alone fit one round (16 x 16 = 256), fc1 -- and only fc1 -- takes the token-row map and its class rows the
            // skinny kernel; the padding rows of `hid` are then never written (they stay as allocated: zero) and nobody reads what the
            // padding rows of the residual stream become.
            static const bool fc1map_env = !(getenv("MHMR_FC1_ROWMAP") && atoi(getenv("MHMR_FC1_ROWMAP")) == 0);
            const int ncu = mhmr_cu_count();
            const bool fc1map = fc1map_env && allrows256 && !nmask && f2 && N % 256 == 0 && (M / 256) * (4 * C / 256) > ncu &&
                                (B * N / 256) * (4 * C / 256) <= ncu;
            if (fc1map) { g.M = B * N; g.Mvalid = B * N; g.img_rows = N; g.img_stride = Tp; }
            if (f2) { g.bias = nullptr; g.rowstats = d->rowstats; g.colsum = k.fc1_colsum; g.fbias = k.fc1_b; }
            TRY(mhmr_launch_gemm(g, dt, s));
            if (rowmap || fc1map) {
                AnyOrder ao_scope(ao);
                TRY(mhmr_launch_cls_linear_fold((const char*)d->xn + (size_t)cls_row * pit * esz, rowP, k.fc1_w, C, B, 4 * C, C, 0, f2 ? nullptr : k.fc1_b,
                                                nullptr, (char*)d->hid + (size_t)cls_row * 4 * C * esz, 4 * rowC, 0, C, nullptr, d->H, Tp, 0, 2, dt,
                                                (f2 && !cst) ? cls_stats : nullptr, 2LL * Tp, k.fc1_colsum, k.fc1_b, nullptr, 0, s,
                                                (f2 && cst) ? &cs_consume : nullptr));
            }
            GemmArgs g2{d->hid, 4 * C, k.fc2_w, 4 * C, Mg, C, 4 * C, k.fc2_b, k.ls2, d->resid, C, nullptr, 0, Tp, d->H, Mg, EPI_RESID};
            rows(g2);
            if (fold) {
                // the rows this epilogue leaves are the NEXT block's qkv operand: with their bf8 copy if that block's V has an fp8 range
                g2.x16 = d->xn; g2.pstats = d->pstats; g2.ldx16 = lo8 ? pit : 0;
                g2.x8_off = (l + 1 < d->L && v8(d->blocks[l + 1])) ? o8 : 0;
            }
            masked(g2);
            TRY(resid_linear(g2));
            if (rowmap) {
                // (with cst: + the patch rows' statistics for the NEXT block's norm1, when that block folds it: an ordinary launch then)
                const bool next_f1 = l + 1 < d->L && fold && (d->blocks[l + 1].flags & 1);
                const ClsStats* cs = !cst ? nullptr : next_f1 ? &cs_produce_stats : &cs_produce;
                AnyOrder ao_scope2(ao && !(cst && next_f1));
                TRY(mhmr_launch_cls_linear_fold((const char*)d->hid + (size_t)cls_row * 4 * C * esz, 4 * rowC, k.fc2_w, 4 * C, B, C, 4 * C, 0, k.fc2_b,
                                                k.ls2, d->resid + (size_t)cls_row * C, rowC, 0, C, nullptr, d->H, Tp, 0, 1, dt, nullptr, 0, nullptr,
                                                nullptr, fold ? (char*)d->xn + (size_t)cls_row * pit * esz : nullptr, rowP, s, cs));
                if (cst && next_f1) stats_fresh = true;
            }
        }
    }
    return mhmr_launch_final_norm(d->resid, d->norm_w, d->norm_b, ctx16, ldctx, feat32, B, d->N, Tp, C, 1e-6f, dt, s);
}

int mhmr_detect_scores(const void* hid16, int ld, const float* w2, const float* b2, float* scores, int rows, int C, int dtype,
                       void* stream) {
    return mhmr_launch_scores(hid16, ld, w2, b2, scores, rows, C, dtype, (hipStream_t)stream);
}
int mhmr_detect_count(const float* scores, int B, int G, int nms_kernel, float thr, int* counts, void* stream) {
    if (nms_kernel < 1 || B <= 0) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_detect_count(scores, B, G, nms_kernel, thr, counts, (hipStream_t)stream);
}
int mhmr_detect_write(const float* scores, int B, int G, int nms_kernel, float thr, const int* base, int* det_b, int* det_y,
                      int* det_x, float* det_score, void* stream) {
    if (nms_kernel < 1 || B <= 0) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_detect_write(scores, B, G, nms_kernel, thr, base, det_b, det_y, det_x, det_score, 0x7fffffff, (hipStream_t)stream);
}
int mhmr_detect_write_cap(const float* scores, int B, int G, int nms_kernel, float thr, const int* base, int* det_b, int* det_y,
                          int* det_x, float* det_score, int cap, void* stream) {
    if (nms_kernel < 1 || B <= 0 || cap < 0) return MHMR_ERR_BAD_ARG;
    return mhmr_launch_detect_write(scores, B, G, nms_kernel, thr, base, det_b, det_y, det_x, det_score, cap, (hipStream_t)stream);
}
int mhmr_person_groups(const int* counts, const int* det_b, int P, int B, int cap, int* base, int* gstart, int ngroups_cap, int* chunks,
                       int nchunks_cap, int* info, void* stream) {
    return mhmr_launch_person_groups(counts, det_b, P, B, cap, base, gstart, ngroups_cap, chunks, nchunks_cap, info, (hipStream_t)stream);
}
int mhmr_camera_embed(const float* K, const float* freq, int B, int G, int patch, float* zK, void* ctx16, int ldctx, int C,
                      int dtype, int num_bands, void* stream) {
    return mhmr_launch_camera_embed(K, freq, B, G, patch, zK, ctx16, ldctx, C, dtype, num_bands, (hipStream_t)stream);
}
int mhmr_linear_f32(const float* X, int ldx, const int* row_idx, const float* W, int ldw, const float* bias, const float* R,
                    int ldr, float* Y, int ldy, int M, int N, int K, int act, void* stream) {
    return mhmr_launch_linear_f32(X, ldx, row_idx, W, ldw, bias, R, ldr, Y, ldy, M, N, K, act, (hipStream_t)stream);
}
int mhmr_layernorm_f32(const float* in, const float* w, const float* b, float* out, int rows, int C, float eps, void* stream) {
    return mhmr_launch_layernorm_f32(in, w, b, out, rows, C, eps, (hipStream_t)stream);
}
int mhmr_hph_self_attn(const float* qkv, const int* gstart, float* out, int ngroups, int nmax, int heads, void* stream) {
    if (heads <= 0) return MHMR_ERR_BAD_SHAPE;
    return mhmr_launch_hph_self_attn(qkv, gstart, out, ngroups, nmax, heads, (hipStream_t)stream);
}
int mhmr_hph_cross_attn(const float* q, const float* kv, const int* chunks, int nchunks, float* out, int heads, int N, void* stream) {
    if (heads <= 0 || N <= 0) return MHMR_ERR_BAD_SHAPE;
    return mhmr_launch_hph_cross_attn(q, kv, chunks, nchunks, out, heads, N, (hipStream_t)stream);
}
int mhmr_hph_decode(const float* dec, int ldd, int nb, const float* K, const int* det_b, float fn, int nearness, float* rotmat,
                    float* rotvec, float* betas, float* expr, float* dist_pp, float* dist, int P, void* stream) {
    if (nb < 0 || nb > 64 || ldd < 318 + nb + 3 + 10) return MHMR_ERR_BAD_SHAPE;      // one thread per beta in a 64-thread block
    return mhmr_launch_hph_decode(dec, ldd, nb, K, det_b, fn, nearness, rotmat, rotvec, betas, expr, dist_pp, dist, P, (hipStream_t)stream);
}

// `depth` x (pre-norm self-attention among the queries of one image, cross-attention over that image's N context
// tokens, GELU feed-forward), each with a residual.  Shared by the Multi-HMR HPH (dim 1024, 8 heads, mlp 1024, depth 2,
// blocks/cross_attn_transformer.py:239-261) and the Anny HPH (dim 512, 16 heads, mlp 2048, depth 8,
// multi_hmr_anny/hph.py:114-151).  Queries are ragged groups (no padding), so the reference's mask arithmetic vanishes.
int mhmr_xattn_layers_forward(const mhmr_hph_layer* layers, int depth, int dim, int heads, int mlp, int Kc, int N, int B,
                              int dtype, float* x, float* xn, float* t1, float* t2, float* kv, const void* ctx16,
                              const int* gstart, int ngroups, int nmax, const int* chunks, int nchunks, int P, void* stream) {
    if (!layers || P < 0 || depth < 0) return MHMR_ERR_BAD_ARG;
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int inner = heads * 32;
    if (Kc % 64 || dim % 64 || dim > 2048 || mlp % 16 || (2 * inner) % 128) return MHMR_ERR_BAD_SHAPE;
    const int Mctx = (B * N + 127) / 128 * 128;
    for (int l = 0; l < depth; ++l) {
        const mhmr_hph_layer& L = layers[l];
        // self-attention among the queries of one image
        TRY(mhmr_launch_layernorm_f32(x, L.ln_sa_w, L.ln_sa_b, xn, P, dim, 1e-5f, s));
        TRY(mhmr_launch_linear_f32(xn, dim, nullptr, L.to_qkv, dim, nullptr, nullptr, 0, t1, 3 * inner, P, 3 * inner, dim, MHMR_ACT_NONE, s));
        TRY(mhmr_launch_hph_self_attn(t1, gstart, t2, ngroups, nmax, heads, s));
        TRY(mhmr_launch_linear_f32(t2, inner, nullptr, L.sa_out_w, inner, L.sa_out_b, x, dim, x, dim, P, dim, inner, MHMR_ACT_NONE, s));
        // cross-attention over the (un-normalised) per-image context
        {
            GemmArgs g{ctx16, Kc, L.to_kv16, Kc, Mctx, 2 * inner, Kc, nullptr, nullptr, kv, 2 * inner, nullptr, 0, 128, 1, Mctx, EPI_F32};
            TRY(mhmr_launch_gemm(g, dtype, s));
        }
        TRY(mhmr_launch_layernorm_f32(x, L.ln_ca_w, L.ln_ca_b, xn, P, dim, 1e-5f, s));
        TRY(mhmr_launch_linear_f32(xn, dim, nullptr, L.to_q, dim, nullptr, nullptr, 0, t1, inner, P, inner, dim, MHMR_ACT_NONE, s));
        TRY(mhmr_launch_hph_cross_attn(t1, kv, chunks, nchunks, t2, heads, N, s));
        TRY(mhmr_launch_linear_f32(t2, inner, nullptr, L.ca_out_w, inner, L.ca_out_b, x, dim, x, dim, P, dim, inner, MHMR_ACT_NONE, s));
        // feed-forward
        TRY(mhmr_launch_layernorm_f32(x, L.ln_ff_w, L.ln_ff_b, xn, P, dim, 1e-5f, s));
        TRY(mhmr_launch_linear_f32(xn, dim, nullptr, L.ff1_w, dim, L.ff1_b, nullptr, 0, t1, mlp, P, mlp, dim, MHMR_ACT_GELU, s));
        TRY(mhmr_launch_linear_f32(t1, mlp, nullptr, L.ff2_w, mlp, L.ff2_b, x, dim, x, dim, P, dim, mlp, MHMR_ACT_NONE, s));
    }
    return 0;
}

int mhmr_hph_forward(const mhmr_hph_desc* d, const float* feat32, const float* zK, void* ctx16, const int* det_b,
                     const int* det_y, const int* det_x, int P, const int* gstart, int ngroups, int nmax, const int* chunks,
                     int nchunks, const float* K, int B, float* offset, float* loc, float* rotmat, float* rotvec, float* betas,
                     float* expr, float* dist_pp, float* dist, void* stream) {
    if (!d || P < 0) return MHMR_ERR_BAD_ARG;
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int C = d->C, dim = d->dim, inner = d->heads * 32, mlp = d->mlp;
    if (d->Ktok % 16 || d->Kc % 64 || C % 16 || dim % 64 || mlp % 16 || (2 * inner) % 128) return MHMR_ERR_BAD_SHAPE;
    if (d->nb < 0 || d->nb > 64) return MHMR_ERR_BAD_SHAPE;          // the decode writes betas with one thread each of 64
    const int Mctx = (B * d->N + 127) / 128 * 128;

    // queries, mlp_offset input, context rows of the detected cells  (model.py:255-265, 500-517, 541-552)
    TRY(mhmr_launch_hph_inputs(feat32, zK, det_b, det_y, det_x, d->cq_x, d->cq_y, d->cv_x, d->cv_y, d->init_tail,
                               318 + d->nb + 3, d->zc, d->token, d->Ktok, ctx16, d->Kc, d->det_row, P, d->G, C, d->dtype, d->nvalid,
                               d->cam_dim > 0 ? d->cam_dim : 99, s));
    // mlp_offset (model.py:258) and loc (272-275)
    TRY(mhmr_launch_linear_f32(d->zc, C, nullptr, d->off1_w, C, d->off1_b, nullptr, 0, d->t1, C, P, C, C, MHMR_ACT_RELU, s));
    TRY(mhmr_launch_linear_f32(d->t1, C, nullptr, d->off2_w, C, d->off2_b, nullptr, 0, offset, 2, P, 2, C, MHMR_ACT_NONE, s));
    TRY(mhmr_launch_loc(offset, det_y, det_x, d->patch, loc, P, s));
    // token embedding (+ pos_embedding folded into the bias)  (cross_attn_transformer.py:352-357)
    TRY(mhmr_launch_linear_f32(d->token, d->Ktok, nullptr, d->tok_w, d->Ktok, d->tok_b, nullptr, 0, d->x, dim, P, dim, d->Ktok,
                               MHMR_ACT_NONE, s));
    (void)Mctx; (void)inner; (void)mlp;
    TRY(mhmr_xattn_layers_forward(d->layers, d->depth, dim, d->heads, d->mlp, d->Kc, d->N, B, d->dtype, d->x, d->xn, d->t1, d->t2, d->kv,
                                  ctx16, gstart, ngroups, nmax, chunks, nchunks, P, stream));
    // read-outs + init (model.py:571-575), 6D -> rotmat -> rotvec, distance post-processing
    TRY(mhmr_launch_linear_f32(d->x, dim, nullptr, d->dec_w, dim, d->dec_b, nullptr, 0, d->dec, d->Ndec, P, d->Ndec, dim, MHMR_ACT_NONE, s));
    return mhmr_launch_hph_decode(d->dec, d->Ndec, d->nb, K, det_b, d->fn, d->nearness, rotmat, rotvec, betas, expr, dist_pp,
                                  dist, P, s);
}

}  // extern "C"
