/* libmhmr.so -- C ABI of the MI355X-native Multi-HMR batched-inference path.
 *
 * The reference (naver/multi-hmr) has no FFI / operator layer: its only seam is the Python class
 * model.Model (reference model.py:30-349) whose forward dispatches PyTorch library kernels.  This header is
 * the boundary a maintainer would bind instead; every entry point names the reference code it replaces.
 *
 * Conventions: extern "C"; raw DEVICE pointers (tensor.data_ptr()) and explicit int shapes; caller-allocated
 * outputs and workspaces; `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 * no allocation, no hidden synchronisation, no exceptions: every call returns 0 on success, a negative
 * MHMR_ERR_* for argument errors or a positive hipError_t.  All matrices are row-major.  "op16" means the 16-bit
 * MFMA operand type selected by `dtype` (MHMR_DT_BF16 or MHMR_DT_F16; fp32 accumulation either way).
 */
#ifndef MHMR_H
#define MHMR_H

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with hidden visibility: the declarations of this header are its whole export surface */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define MHMR_VERSION 106   /* 106 (later, additive: mhmr_pre_image, mhmr_preprocess_u8_batch; mhmr_pre_image_o, mhmr_preprocess_u8_batch_oriented; mhmr_render_desc, mhmr_render_workspace_bytes, mhmr_render_meshes; mhmr_hph_self_attn, mhmr_hph_cross_attn, mhmr_hph_decode; mhmr_render_views_workspace_bytes, mhmr_render_views; mhmr_scene_pack; mhmr_body_consts, mhmr_body_forward, mhmr_sparse_regress, mhmr_gt_targets, mhmr_rotvec_to_rotmat, mhmr_project_points; mhmr_vit_plan; mhmr_render_maps_desc, mhmr_render_maps, mhmr_point_visibility_desc, mhmr_render_point_visibility, mhmr_render_amodal_workspace_bytes, mhmr_render_amodal; mhmr_contact_desc, mhmr_contact_workspace_bytes, mhmr_contact_check_faces, mhmr_contact); 106: mhmr_attention16_ex variant 10 (class query on workgroups of its own; opt-in); the fc1 epilogue's GELU is max(x,0) - |x| exp2(P5(|x|)) (6.4e-7 absolute; was Abramowitz-Stegun 7.1.25, 2.6e-5); 105: mhmr_vit_desc.cls_pstats (row statistics inside the class-row launches); mhmr_vit_desc.v16 (merged qkv launch of a short batch); mhmr_vit_desc.cpad (ViT-S on the 256x256 kernel: C-wide linears as N = 512 with masked columns); mhmr_vit_desc.{splitk, splitk_bytes}, mhmr_splitk_workspace_bytes, mhmr_gemm16_splitk_resid: split-k residual linears for launches that fill less than half the chip (a batch of one); 104: mhmr_vit_desc.{x3, qkv32, hid32}: the f16x3 precision mode (three 16-bit products per term in every backbone linear, fp32 attention); mhmr_gemm16_ex a_k with K = 3 a_k; mhmr_attention_f32; 103: mhmr_attention16_ex variant 6 (the default of mhmr_vit_forward); mhmr_camera_embed(num_bands), mhmr_hph_desc.cam_dim; mhmr_lbs_consts.basis16 layout (high halves for k < Kb - 64); mhmr_person_groups, mhmr_detect_write_cap, mhmr_hph_desc.nvalid (no host round trip for the person set; group / chunk counts of mhmr_hph_forward are upper bounds); 102: mhmr_lbs_consts: extra joints as virtual vertex tiles (Vl, xbary); 101: class token LAST in the token rows, mhmr_vit_block.{v_w2,proj_w2}, mhmr_gemm16_ex, mhmr_cls_linear16, mhmr_attention16_ex variants 4 / 5 */

#define MHMR_OK 0
#define MHMR_ERR_BAD_ARG (-1)
#define MHMR_ERR_BAD_SHAPE (-2)

#define MHMR_DT_BF16 0
#define MHMR_DT_F16 1

#define MHMR_ACT_NONE 0
#define MHMR_ACT_RELU 1
#define MHMR_ACT_GELU 2

/* GEMM epilogues of mhmr_gemm16 */
#define MHMR_EPI_OP16 0      /* out16 = acc + bias                                           */
#define MHMR_EPI_OP16_GELU 1 /* out16 = gelu(acc + bias), erf form, 3-term A&S 7.1.25 erfc: |abs err| < 2.6e-5 (Mlp fc1) */
#define MHMR_EPI_OP16_RELU 2 /* out16 = relu(acc + bias)                (regression_mlp, model.py:596-609) */
#define MHMR_EPI_RESID 3     /* out32 += gamma * (acc + bias)           (LayerScale + residual) */
#define MHMR_EPI_PATCH 4     /* patch-embed: + bias + pos-embed, scattered to token rows     */
#define MHMR_EPI_F32 5       /* out32 = acc (+ bias)                    (HPH to_kv)          */
#define MHMR_EPI_VT 6        /* V^T[b][h][d][swap23(t)] = acc + bias    (attention V operand) */
#define MHMR_EPI_OP16_QK 7   /* out16 = (acc + bias) * (n < N/2 ? MHMR_ATTN_QSCALE : 1): the Q | K projection (N = 2C) with the
                                softmax scale and the exp -> exp2 change of base folded into Q in fp32, before the one rounding */
/* head_dim^-0.5 * log2(e) for head_dim = 64 (DINOv2 Attention: softmax((q * scale) k^T)) */
#define MHMR_ATTN_QSCALE 0.18033688011112042f

int mhmr_version(void);
/* sha256 prefix (16 hex digits) of the sources + compile flags this library was built from (multi_hmr_amd/_lib.py::source_hash);
 * "unknown" for a build that did not pass it.  Evidence files (profiles/) are keyed by it. */
const char* mhmr_source_hash(void);

/* ------------------------------------------------------------------------------------------------------------
 * ViT backbone.  Replaces blocks/dinov2.py:16-26 -> torch.hub DinoVisionTransformer.get_intermediate_layers
 * (patch embed + cls + interpolated pos-embed, L pre-norm blocks with LayerScale, final LayerNorm, cls dropped).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *ln1_w, *ln1_b;   /* [C]                                  blocks.i.norm1            */
    const void* qkv_w;            /* op16 [3C, C]                         blocks.i.attn.qkv.weight  */
    const float* qkv_b;           /* [3C]                                                            */
    const void* proj_w;           /* op16 [C, C]                          blocks.i.attn.proj        */
    const float *proj_b, *ls1;    /* [C], [C] (ls1.gamma)                                           */
    const float *ln2_w, *ln2_b;   /* [C]                                  blocks.i.norm2            */
    const void* fc1_w;            /* op16 [4C, C]                         blocks.i.mlp.fc1          */
    const float* fc1_b;           /* [4C]                                                            */
    const void* fc2_w;            /* op16 [C, 4C]                         blocks.i.mlp.fc2          */
    const float *fc2_b, *ls2;     /* [C], [C] (ls2.gamma)                                           */
    /* Optional low halves of the two projections whose one-time weight rounding dominates the 1e-3 parity budget:
     * op16 [C, 2C] = [W_hi | W_lo] along k with W_hi = op16(W), W_lo = op16(W - W_hi); NULL = single pass over qkv_w[2C:3C] / proj_w. */
    const void* v_w2;             /* blocks.i.attn.qkv.weight[2C:3C] as hi | lo, or NULL              */
    const void* proj_w2;          /* blocks.i.attn.proj.weight as hi | lo, or NULL                    */
    /* LayerNorm folded into the consuming linear (used when mhmr_vit_desc.pstats / rowstats are given and the token-row map is on):
     * flags bit 0: norm1 -> qkv (never for blocks[0]: the patch embedding leaves no row statistics, MHMR_ERR_BAD_ARG), bit 1: norm2 -> fc1;
     * a set bit needs its *_colsum (MHMR_ERR_BAD_ARG otherwise).  A folded linear's weight is W diag(w_ln) (v_w2 likewise), its bias is
     * b + W b_ln, and *_colsum[n] = sum_k of the ROUNDED folded weight row (hi + lo where there is a low half), fp32. */
    int flags;
    const float* qkv_colsum;      /* [3C] or NULL */
    const float* fc1_colsum;      /* [4C] or NULL */
    /* The same low halves for the fp8 low-half range of the big GEMMs (mhmr_vit_desc.lo8; round 5): rows of 3C BYTES = [W_hi: C op16 values |
     * e4m3(W_lo * 2^-e): C bytes], *_w8_scale = 127 + e (the E8M0 scale byte).  The weight's low half corrects the high half's 2^-12
     * rounding: it needs three significant bits, not eleven, and the fp8 matrix pipe runs at twice the 16-bit rate.  NULL = that linear
     * keeps the op16 low half (v_w2 / proj_w2, which the class-row kernel uses in either case).  For a folded V the rows hold W diag(w_ln). */
    const void* v_w8;
    const void* proj_w8;
    int v_w8_scale, proj_w8_scale;
} mhmr_vit_block;

typedef struct {
    int dtype;              /* MHMR_DT_*                                                                  */
    int B, S, C, H, L;      /* images, image size (S % 14 == 0), embed dim (= 64 H), heads, depth         */
    int G, N, T, Tp;        /* S/14, G*G, N+1, rows per image: T rounded up to a multiple of 64 (128 when a linear
                               of the encoder runs on the 128x128 kernel: B*Tp or C not a multiple of 256) -- mhmr_vit_plan says which.
                               Token rows of image b: patch n (= y*G + x) at row b*Tp + n, the CLASS token at row b*Tp + N
                               (last: attention is permutation-equivariant), zeros behind it */
    int Kp;                 /* 588 rounded up to a multiple of 64 (= 640)                                 */
    const void* patch_w;    /* op16 [C, Kp]      patch_embed.proj.weight flattened (c,py,px), zero padded */
    const float* patch_b;   /* [C]                                                                        */
    const float* cls_pos0;  /* [C]               cls_token + pos[0]                                       */
    const float* pos;       /* [1+N, C]          pos_embed bicubically interpolated to G x G (host, once) */
    const mhmr_vit_block* blocks; /* HOST array of L block descriptors                                    */
    const float *norm_w, *norm_b; /* [C]          final norm                                              */
    /* workspaces (device) */
    void* a_patch;          /* op16 [roundup(B*N,128), Kp]   rows >= B*N must be zero                     */
    float* resid;           /* [B*Tp, C]        fp32 residual stream                                      */
    void* xn;               /* op16 [B*Tp, C]                                                             */
    void* qk;               /* op16 [B*Tp, 2C]  (Q | K)                                                   */
    void* vt;               /* op16 [B, H, 64, Tp]                                                        */
    void* att;              /* op16 [B*Tp, C]                                                             */
    void* hid;              /* op16 [B*Tp, 4C]                                                            */
    int* attn_flags;        /* [mhmr_attention_flag_count(B, Tp, H)] or NULL (then the self-contained attention form runs) */
    /* LayerNorm fold workspaces, or NULL (then every LayerNorm is a pass of its own and no block may have flags set): the residual
     * epilogues of proj / fc2 leave the 16-bit copy of the raw residual rows in `xn` and per-row block sums in `pstats`; row statistics
     * are finished by a small kernel into `rowstats`; the consuming linears normalise in their epilogues. */
    float* pstats;          /* [B*Tp, C/64, 2]  (sum, sum of squares) of every 64-column block of a residual row               */
    float* rowstats;        /* [B*Tp, 2]        (mean, rstd)                                                                  */
    /* x3 != 0: the "f16x3" precision mode -- for checkpoints whose statistics a single 16-bit rounding per operand does not survive
     * (multi_hmr_amd/vit.py logit_gain).  Every operand of every backbone linear is an op16 PAIR (hi = op16(v), lo =
     * op16(v - hi): 22 significant bits for f16) and every term is three products (a_hi w_hi + a_hi w_lo + a_lo w_hi) in one fp32
     * accumulator chain of the same MFMA kernels (mhmr_gemm16_ex: K = 3 a_k); LayerNorm, GELU (exact erf), the residual stream and the
     * WHOLE attention (mhmr_attention_f32) are fp32.  Layout changes against the fields above:
     *   patch_w op16 [C, 3 Kp] and every block weight op16 [N, 3 K] = [W_hi | W_lo | W_hi] along k (qkv_w [3C, 3C], proj_w [C, 3C],
     *   fc1_w [4C, 3C], fc2_w [C, 12C]); v_w2 / proj_w2 NULL, flags 0;  Tp % 128 == 0 (Tp % 256 for C % 256 == 0: every linear on the
     *   256x256 kernel); a_patch op16 [roundup(B*N,128), 2 Kp], xn / att op16 [B*Tp, 2C], hid op16 [B*Tp, 8C] = [hi | lo];
     *   qk, vt, attn_flags, pstats, rowstats unused (may be NULL). */
    /* lo8 != 0: `xn` and `att` are op16 [B*Tp, 3C/2] -- every row = [C op16 values | C bytes: the bf8 (e5m2) copy of the same values],
     * written by their producers (LayerNorm kernel, residual epilogue, attention) where the next linear has an fp8 low-half range
     * (blocks[i].v_w8 / proj_w8); C % 256 == 0.  lo8 == 0: rows of C op16 values, v_w8 / proj_w8 ignored. */
    int lo8;
    int x3;
    float* qkv32;           /* x3: [B*Tp, 3C] fp32  (Q | K | V), bias included                                                 */
    float* hid32;           /* x3: [B*Tp, 4C] fp32  fc1 output before the GELU                                                 */
    /* Split-k workspace, or NULL.  When every row goes through the 256x256 kernel (Tp % 256 == 0 with N % 256 == 0: the "all rows" form a
     * caller picks for tiny batches) and a residual linear (proj / fc2) has at most half as many 256x256 tiles as the device has CUs, its k
     * range is cut into slices whose fp32 partial tiles go here -- mhmr_splitk_workspace_bytes(B*Tp, C, 4C) bytes cover every linear -- and
     * a row-wise kernel sums them in slice order, applies bias / LayerScale / residual and leaves xn and rowstats (no ln_stats launch).
     * Deterministic; the summation order differs from the unsplit linear's, i.e. from the same image inside a large batch, at the 16-bit
     * noise level -- as the all-rows form itself already does. */
    float* splitk;
    long long splitk_bytes;
    /* C = 384 (ViT-S) on the 256x256 kernel.  cpad = 512 says: Tp % 256 == 0, pstats / rowstats given, and every array indexed by the
     * output channel of the three C-wide linears is zero-padded to 512 entries -- qkv_w [2C + 512, C] (the V rows are its last C rows + 128
     * zero rows), qkv_b and qkv_colsum [2C + 512], v_w2 [512, 2C], proj_w / proj_w2 [512, C | 2C], fc2_w [512, 4C], proj_b, ls1, fc2_b,
     * ls2 [512].  Those linears then run as N = 512 with the last 128 output columns masked (GemmArgs::n_valid), every block linear is
     * on the 256x256 kernel and the LayerNorm fold applies.  0 = C-wide linears of such a model run on the 128x128 kernel, no fold. */
    int cpad;
    /* op16 [B*Tp, C] or NULL.  Given (with Tp % 256 == 0, all rows through the 256x256 kernel) and the whole qkv linear at most one round
     * of 256x256 tiles (B*Tp/256 * 3C/256 <= CUs): blocks whose V has no low half run Q | K | V as ONE launch -- V row-major into this
     * buffer -- followed by a transpose into `vt`, instead of a Q | K and a V launch of half a round each. */
    void* v16;
    /* [B, C/16, 2] fp32 or NULL.  Given (with pstats / rowstats, under the token-row map): the class-row launches of proj / fc2 also run the
     * patch rows' row statistics (extra workgroups of the same launch) and leave block sums of the class rows here, which the class-row
     * launches of qkv / fc1 turn into (mean, rstd) themselves -- the forward then issues no statistics launch of its own (47 fewer
     * launches per ViT-L forward).  NULL = mhmr_ln_stats-style launches as before. */
    float* cls_pstats;
    /* The tap, or NULL: before block l >= tap_first the fp32 residual stream is copied into slot l - tap_first of
     * `tap`, [L - tap_first][B*Tp, C] fp32 -- the block inputs mhmr_vit_tail_backward differentiates at.  One hipMemcpyAsync per slot on
     * the caller's stream (capturable).  NULL issues exactly the launches of a forward without it; with or without a tap feat32, ctx16 and
     * mhmr_vit_form_bits are the same bit for bit, and `resid` holds the stream the final norm read.  0 <= tap_first <= L
     * (MHMR_ERR_BAD_ARG otherwise). */
    float* tap;
    int tap_first;
} mhmr_vit_desc;

/* x: [B,3,S,S] fp32 (ImageNet-normalised).  feat32: [B*N, C] fp32 patch features (token n = y*G + x).
 * ctx16: op16 [>= B*N rows, ldctx]; columns [0, C) receive the 16-bit copy of feat32.                       */
int mhmr_vit_forward(const mhmr_vit_desc* d, const float* x, float* feat32, void* ctx16, int ldctx, void* stream);

/* Which launch sequence mhmr_vit_forward runs for this description on this stream, on this device, under the environment switches of this
 * process: decided by the very function the forward calls, so the answer is what a forward issued now would run.  Host only: launches
 * nothing and reads no device memory (tests assert the form they meant to exercise; a NULL optional workspace steps a form down silently
 * otherwise).  Returns what mhmr_vit_forward would return before its first launch (MHMR_ERR_BAD_SHAPE / MHMR_ERR_BAD_ARG). */
#define MHMR_VIT_FORM_ROWMAP 0x001u      /* block GEMMs over the B*N patch rows, class rows through mhmr_cls_linear16's kernel  */
#define MHMR_VIT_FORM_ALLROWS256 0x002u  /* every block linear on the 256x256 kernel over all B*Tp rows                          */
#define MHMR_VIT_FORM_NMASK 0x004u       /* C = 384: C-wide linears as N = 512 with masked columns (cpad)                        */
#define MHMR_VIT_FORM_FOLD 0x008u        /* LayerNorm folded into the consuming linears                                          */
#define MHMR_VIT_FORM_LO8_RANGES 0x010u  /* fp8 low-half ranges of v_w8 / proj_w8 run                                            */
#define MHMR_VIT_FORM_CST 0x020u         /* row statistics inside the class-row launches (cls_pstats)                            */
#define MHMR_VIT_FORM_AO 0x040u          /* any-order launches                                                                   */
#define MHMR_VIT_FORM_SPLITK 0x080u      /* split-k residual linears                                                             */
#define MHMR_VIT_FORM_QKV_MERGE 0x100u   /* Q | K | V as one launch + transpose (blocks whose V has no low half)                 */
#define MHMR_VIT_FORM_FC1MAP 0x200u      /* fc1 alone under the token-row map                                                    */
#define MHMR_VIT_FORM_X3 0x400u          /* the f16x3 forward: none of the other bits                                            */
int mhmr_vit_form_bits(const mhmr_vit_desc* d, void* stream, unsigned* bits);

/* How to lay out the workspaces of a mhmr_vit_desc, BEFORE there is one: rows per image, row pitch, which optional workspaces to allocate,
 * and the form mhmr_vit_forward then runs.  The one statement of the rule (csrc/vit_plan.h): mhmr_vit_forward decides its form from the
 * same file.  Host only: no stream, no device memory; with ncu > 0 it runs on a machine without a GPU.
 * Rows per image (Tp), T = N + 1 tokens, in the order the rule is applied:
 *   x3:                                T rounded up to 256 (C % 256 == 0) or 128: all rows through every linear.
 *   fold, and no token-row map:        T rounded up to 256 -- cpad packs (C = 384), N % 256 != 0, and TINY batches, whose narrowest
 *                                      linear (B * roundup(T, 256) / 256 * C / 256 tiles of 256x256) is at most 128 tiles: half a round
 *                                      of the 256 CUs the rule was measured on, a fixed number of the rule and not of the device.
 *   token-row map, or all 256-tiles:   T rounded up to 64 -- C % 256 == 0 and N % 256 == 0 (the block GEMMs cover the B * N patch rows,
 *                                      the class rows go through the class-row kernel), or C % 256 == 0 and B * roundup(T, 64) % 256
 *                                      == 0; B * Tp * C * 4 < 2^32 either way (32-bit residual offsets of the 256x256 kernel).
 *   otherwise:                         T rounded up to 128, the row tile of the 128x128 kernel.
 * Where N % 256 == 0 the rule returns a multiple of 256 exactly when the token-row map is off: that is how mhmr_vit_forward tells the
 * all-rows form from the row map, so a caller must not pad such a description to a multiple of 256 for any other reason.
 * Every workspace of a mhmr_vit_desc must be ZERO-INITIALISED ONCE by the caller, `att` and `hid` in particular: under the token-row
 * map (and for fc1 under MHMR_VIT_FORM_FC1MAP) the padding rows of `att` / `hid` (rows > N of an image) are never written -- attention
 * skips workgroups whose queries are all padding, the class-row launches write row N alone -- while a linear that covers all rows (fc2
 * under MHMR_VIT_FORM_FC1MAP) reads them, row-locally: NaN / Inf bit patterns there would be carried into the padding rows of the
 * residual stream, whose keys the attention masks only as long as they are finite. */
#define MHMR_PLAN_ROWMAP 0x001u          /* clear = MHMR_ROWMAP=0: no token-row map, no 256x256 all-rows form                     */
#define MHMR_PLAN_GEMM128 0x002u         /* SET = MHMR_GEMM128: the 128x128 kernel everywhere (clear by default, as VITS_256 and LO8) */
#define MHMR_PLAN_LNFOLD 0x004u          /* clear = MHMR_LNFOLD=0: no LayerNorm fold                                              */
#define MHMR_PLAN_LO8 0x008u             /* fold-/lo8_eligible: "pack fp8 low-half rows" (a packer opts in); form_bits: "use them" */
#define MHMR_PLAN_ANYORDER 0x010u        /* (any-order launches: not part of a plan; form_bits never has MHMR_VIT_FORM_AO)        */
#define MHMR_PLAN_QKV_MERGE 0x020u       /* clear = MHMR_QKV_MERGE=0                                                              */
#define MHMR_PLAN_FC1_ROWMAP 0x040u      /* clear = MHMR_FC1_ROWMAP=0                                                             */
#define MHMR_PLAN_CLS_STATS 0x080u       /* clear = MHMR_CLS_STATS=0                                                              */
#define MHMR_PLAN_TINY_ALLROWS 0x100u    /* clear = MHMR_TINY_ALLROWS=0: tiny batches of a folded pack keep the token-row map     */
#define MHMR_PLAN_LNFOLD_ALLROWS 0x200u  /* clear = MHMR_LNFOLD_ALLROWS=0: no fold where it needs the all-rows padding            */
#define MHMR_PLAN_VITS_256 0x400u        /* SET = MHMR_VITS_256=1: C = 384 with folded LayerNorms on the 256x256 kernel (cpad)    */
#define MHMR_PLAN_DEFAULT 0x3f5u         /* an empty environment (MHMR_PLAN_LO8 clear: nobody packed fp8 rows)                    */
typedef struct {
    int C, H, N, B;         /* embed dim (= 64 H), heads, patch tokens per image, images (0: only the two *_eligible answers are valid) */
    int fold, x3, lo8, cpad;/* the pack's choices: blocks carry folded LayerNorms; f16x3; fp8 low-half rows; mhmr_vit_desc.cpad   */
    unsigned switches;      /* MHMR_PLAN_*: the entry reads no environment                                                        */
    int ncu;                /* compute units the launches are planned for; 0 = those of the current device (no device: nothing
                               that depends on them is planned -- no split-k workspace, no v16; Tp, row_map, pitch do not)       */
} mhmr_vit_plan_request;
typedef struct {
    int Tp;                 /* rows per image                                                                                     */
    int row_map;            /* the token-row map: block GEMMs over the B * N patch rows                                           */
    int tiny_batch;         /* the batch is "tiny" in the sense of the rule above (whether or not that changed the layout)          */
    int pitch;              /* row pitch of xn / att in elements (C; 3C/2 with lo8; 2C with x3)                                   */
    int need_pstats;        /* allocate pstats and rowstats                                                                       */
    int need_cls_pstats;    /* allocate cls_pstats                                                                                */
    int need_v16;           /* allocate v16                                                                                       */
    long long splitk_bytes; /* allocate splitk of this many bytes (0: none)                                                       */
    int attn_flags;         /* mhmr_attention_flag_count(B, Tp, H) (0 with x3)                                                    */
    int fold_eligible;      /* pack time: fold LayerNorms into the linears of a (C, N) encoder                                    */
    int lo8_eligible;       /* pack time: add fp8 low-half rows                                                                   */
    unsigned form_bits;     /* MHMR_VIT_FORM_* (never _AO) of a description that offers exactly these workspaces                  */
} mhmr_vit_plan_result;
/* MHMR_ERR_BAD_ARG: NULL, B < 0, C <= 0, C != 64 H, N <= 0 or ncu < 0; MHMR_ERR_BAD_SHAPE: lo8 with C % 256 != 0. */
int mhmr_vit_plan(const mhmr_vit_plan_request* rq, mhmr_vit_plan_result* out);

/* Building blocks, exported for unit tests and bisecting. */
int mhmr_gemm16(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                const float* gamma, void* out, int ldo, const float* pos, int Np, int Tp, int H, int Mvalid, int epi,
                int dtype, void* stream);
/* The same with (a) a token-row map: logical activation / output row m = b * img_rows + n lives at physical row b * img_stride + n
 * (img_rows % 256 == 0; 0 = rows are physical), so a GEMM can cover the patch rows of every image and skip its class / padding rows;
 * (b) a low-half weight pass: W = [W_hi | W_lo] along k, K = 2 * a_k, the activation's k index wraps at a_k (0 = off);
 * (c) K = 3 * a_k: W = [W_hi | W_lo | W_hi], A = [A_hi | A_lo] (lda >= 2 a_k): the third k range reads the activation's second a_k
 *     columns -- three 16-bit products per term (the f16x3 mode).                                                                   */
int mhmr_gemm16_ex(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                   const float* gamma, void* out, int ldo, const float* pos, int Np, int Tp, int H, int Mvalid, int epi,
                   int dtype, int img_rows, int img_stride, int a_k, void* stream);
/* mhmr_gemm16_ex with the LayerNorm fold (csrc/gemm256.hip; M, N % 256 == 0, K % 128 == 0 only).  Producer (epi = MHMR_EPI_RESID): x16 !=
 * NULL receives the op16 copy of the updated residual rows [rows, N] and pstats [rows, N/64, 2] the (sum, sum of squares) of each
 * 64-column block.  Consumer (epi = MHMR_EPI_OP16_QK / _VT / _OP16_GELU, bias = NULL): out = rstd_m (acc - mean_m colsum_n) + fbias_n
 * with rowstats [rows, 2] = (mean, rstd) as mhmr_ln_stats leaves them.                                                              */
int mhmr_gemm16_ln(const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                   const float* gamma, void* out, int ldo, int Tp, int H, int epi, int dtype, int img_rows, int img_stride,
                   int a_k, void* x16, float* pstats, const float* rowstats, const float* colsum, const float* fbias, void* stream);
/* mhmr_gemm16_ln for an output width that is a multiple of 128 but not of 256 (ViT-S: 384), on the 256x256 kernel: N = n_valid + 128, W
 * [N, K] and every per-column vector (bias, gamma, colsum, fbias) zero-padded to N entries by the caller; the last 128 columns are
 * computed and not stored.  epi = MHMR_EPI_RESID (out32 [M, ldo >= n_valid], x16 / pstats [M, n_valid / 64, 2] optional) or MHMR_EPI_VT
 * (n_valid / 64 heads; rowstats / colsum / fbias optional: the LayerNorm-fold consumer).  M % 256 == 0, K % 128 == 0. */
int mhmr_gemm16_masked(const void* A, int lda, const void* W, int ldw, int M, int N, int n_valid, int K, int a_k, const float* bias,
                       const float* gamma, void* out, int ldo, int Tp, int H, int epi, int dtype, void* x16, float* pstats,
                       const float* rowstats, const float* colsum, const float* fbias, void* stream);
/* The qkv linear of a SHORT batch as one launch + a transpose (what mhmr_vit_forward runs when mhmr_vit_desc.v16 is given): W [3C, K = C],
 * qk [B*Tp, 2C] = (Q * MHMR_ATTN_QSCALE | K), vt [B][H][64][Tp] with the key permutation of MHMR_EPI_VT, v16 [B*Tp, C] scratch.
 * B*Tp % 256 == 0, C % 256 == 0, Tp % 64 == 0.  rowstats / colsum [3C] / fbias [3C]: the LayerNorm-fold consumer form (then bias = NULL). */
int mhmr_qkv16(const void* A, int lda, const void* W, int ldw, int B, int Tp, int C, int H, const float* bias, void* qk, void* v16, void* vt,
               int dtype, const float* rowstats, const float* colsum, const float* fbias, void* stream);
/* Split-k residual linear (csrc/gemm256.hip SPLITK + csrc/vit_misc.hip splitk_resid_kernel): out32 += gamma * (A . W^T + bias) for a launch
 * that would otherwise occupy at most half of the CUs.  mhmr_splitk_workspace_bytes: bytes of fp32 partial tiles the pair needs for an
 * [M, N] output over K (0 = such a problem is not split: M, N % 256, K % 128, tiles <= CUs / 2, K >= 512).  a_k as in mhmr_gemm16_ex.
 * x16 (row pitch ldx16 elements, 0 = N) receives the op16 copy of the updated rows and rowstats [M, 2] their (mean, rstd) with the centred
 * variance (eps inside the square root); either may be NULL.  N must be 256, 512, 768 or 1024 (one wave per row in the reduction). */
long long mhmr_splitk_workspace_bytes(int M, int N, int K);
int mhmr_gemm16_splitk_resid(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int a_k, const float* bias,
                             const float* gamma, float* out32, void* x16, int ldx16, float* rowstats, float eps, float* ws,
                             long long ws_bytes, int dtype, void* stream);
/* rowstats[b*Tp + n] = (mean, rstd) of residual row (b, n): n < N from the block sums pstats[b*Tp + n][C/64][2], n == N (the class row)
 * from the fp32 row resid[b*Tp + N][C] itself.                                                                                       */
/* mhmr_gemm16_ln with an fp8 low-half range (csrc/gemm256.hip, GemmArgs::lo8; epi = MHMR_EPI_VT or MHMR_EPI_RESID only): A rows = [a_k op16 |
 * a_k bytes bf8 (e5m2) of the same values] (lda >= 3 a_k / 2), W rows = [a_k op16 | a_k bytes e4m3 of W_lo * 2^-e], w8_scale = 127 + e;
 * K is implied (a_k + a_k / 2 in 16-bit units), a_k % 256 == 0.  Producer side (MHMR_EPI_RESID, x16 != NULL): ldx16 = row pitch of x16 in
 * elements (0 = ldo) and x8_off > 0 = byte offset inside an x16 row for the bf8 copy of the new residual values.  lo8 = 0 makes it
 * mhmr_gemm16_ln with the producer's pitch options (then K = a_k, one pass). */
int mhmr_gemm16_lo8(const void* A, int lda, const void* W, int ldw, int M, int N, int a_k, int lo8, int w8_scale, const float* bias,
                    const float* gamma, void* out, int ldo, int Tp, int H, int epi, int dtype, int img_rows, int img_stride, void* x16,
                    int ldx16, int x8_off, float* pstats, const float* rowstats, const float* colsum, const float* fbias, void* stream);
int mhmr_ln_stats(const float* pstats, const float* resid, float* rowstats, int B, int N, int Tp, int C, float eps, void* stream);
/* The class-token rows of a block linear (csrc/vit_cls.hip): B rows, a_stride / o_stride elements apart.  epi 0: Q | K | V projection
 * (columns n_base + [0, N) of [Q * MHMR_ATTN_QSCALE | K | V]; Q, K -> out16 row, V -> column vcol of vt [B,H,64,Tp]); epi 1: out32 +=
 * gamma * (acc + bias); epi 2: out16 = gelu(acc + bias).  N % 16 == 0, K % 128 == 0, a_k as in mhmr_gemm16_ex.                     */
int mhmr_cls_linear16(const void* A, long long a_stride, const void* W, int ldw, int B, int N, int K, int a_k, const float* bias,
                      const float* gamma, void* out, long long o_stride, int n_base, int C, void* vt, int H, int Tp, int vcol,
                      int epi, int dtype, void* stream);
/* qk: op16 [B*Tp, 2C] = (Q * MHMR_ATTN_QSCALE | K), head h at columns h*64; vt: op16 [B,H,64,Tp] key-permuted V^T
 * (MHMR_EPI_VT); out: op16 [B*Tp, C] = softmax_2(Q K^T) V over the T real keys of each image.
 * `out` (here, in mhmr_attention16_ex and as mhmr_vit_desc.att) must be ZERO-INITIALISED ONCE by the caller: a 128-query workgroup whose
 * rows are all padding (rows >= T of an image) returns without storing, so those rows keep what was allocated; the linears behind read
 * them (row-local: real rows never depend on them) and NaN / Inf bit patterns there would be carried along.
 * Padding cannot reach a real row, bit for bit: keys >= T are masked behind the matrix pipe (their K rows and V^T columns may hold any
 * finite values), and a QUERY row >= T that shares a wave with real rows is computed with Q = 0 whatever the buffer holds there (its output
 * row is the finite mean of V), so it can neither move the wave's reference level nor flag its workgroup for the textbook pass.
 * Every row < T is written on every call, whatever `out` held before.                                                              */
int mhmr_attention16(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype,
                     void* stream);
/* The attention kernel forms (csrc/attention.hip), for tests and A/B measurements.  Every form subtracts a per-query reference
 * level from the scores inside the matrix pipe; they differ in how the level follows the row maximum:
 *   variant 6  (what mhmr_vit_forward runs since round 4) the arithmetic and flag protocol of variant 0 on v_mfma_f32_16x16x32 (a query's
 *              keys spread over four lanes; the 32x32x16 shape of the other forms costs 5-8 % more power per flop on this chip).
 *   variant 0  level = exact row maximum of key tile 0, no maximum afterwards; a workgroup in which
 *              a lane's tile sum of exp2(score - level) exceeded 2^limit_log2 (0 <= limit_log2 <= 15; 15 = "would leave the
 *              16-bit range", 0 = nearly every workgroup) sets its entries of `flags` and is recomputed by variant 1, launched
 *              right behind it on the same stream.  flags: int workspace of mhmr_attention_flag_count(B, Tp, H) entries (four
 *              per 128-query workgroup); the call writes every entry, the caller need not clear them.  T = 64 n + 1: the lone
 *              key of the last tile is folded in as a rank-1 update.
 *   variant 1  textbook online softmax (running maximum + subtract every tile).        flags unused (NULL)
 *   variant 2  level moves when the running maximum leaves a +-8 band (what mhmr_attention16 runs).   flags unused (NULL)
 *   variant 3  variant 2 with 8-wave workgroups.                                        flags unused (NULL)
 *   variant 4 / 5  the arithmetic of variant 0 with 64 queries per wave (two 32-query blocks: a wave's softmax of one block issues in
 *              the shadow of its MFMAs on the other; 256-query workgroups, 3- / 2-slot K/V ring); flags as for variant 0.
 *   variant 7 / 8 / 9  round-6 experiment forms of variant 6 (the next tile's copies in front of the score MFMAs, a three-slot K / V^T
 *              ring, both): same results, none faster inside the forward.
 *   variant 10 variant 6 with the lone query of T = 128 n + 1 (the class token, the last token row) on workgroups of its own -- vector
 *              ALU, exact online softmax in fp32 -- instead of a 128-query workgroup with one real row; any other T runs variant 6's
 *              launch.  Measured slower than variant 6 (round 6): kept for tests and A/B measurements.                                   */
int mhmr_attention16_ex(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype,
                        float limit_log2, int variant, int* flags, void* stream);
int mhmr_attention_flag_count(int B, int Tp, int H);
/* variant 6 of mhmr_attention16_ex into rows of pitch ldo elements (>= C), with the bf8 (e5m2) copy of every output row at byte offset
 * o8 of the row (0 = none; 2C <= o8, o8 + C <= 2 ldo): the A operand of an output projection with an fp8 low-half range. */
int mhmr_attention16_pitch(const void* qk, const void* vt, void* out, int B, int T, int Tp, int C, int H, int dtype, int* flags, int ldo,
                           int o8, void* stream);
/* mhmr_layernorm16 into rows of pitch ld16 elements, with the bf8 copy at byte offset o8 (0 = none). */
int mhmr_layernorm16_pitch(const float* in, const float* w, const float* b, void* out16, int ld16, int o8, int rows, int C, float eps,
                           int dtype, void* stream);
/* The attention of the f16x3 mode (csrc/attention_f32.hip, which also holds mhmr_attention_f32_tape / _backward below): qkv fp32 [B*Tp, 3C] = (Q | K | V) un-scaled, head h at columns h*64;
 * out op16 PAIR [B*Tp, 2C] = [hi | lo] of softmax(Q K^T / 8) V over the T real keys; every product on v_mfma_f32_16x16x4_f32 (exact fp32).
 * Rows >= T of an image are written as zeros or as the (finite) attention of a padding row: never left unwritten.   Tp % 64 == 0.
 * hi and lo are taken from ONE fp32 value of o: hi + lo = o to 2^-22 (f16) / 2^-16 (bf16) relative, ties of op16(o) included. */
int mhmr_attention_f32(const float* qkv, void* out, int B, int T, int Tp, int C, int H, int dtype, void* stream);
/* Producers of operand PAIRS in the f16x3 mode: out16 rows of 2 C (2 N) values = [hi = op16(y) | lo = op16(y - hi)].
 * mhmr_layernorm16_pair: y = LayerNorm(in row) (C in {384, 768, 1024}); mhmr_gelu16_pair: y = gelu_erf(in[m][n]), in fp32 [M, N], N % 4 == 0. */
int mhmr_layernorm16_pair(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps, int dtype,
                          void* stream);
int mhmr_gelu16_pair(const float* in, void* out16, long long M, int N, int dtype, void* stream);
int mhmr_layernorm16(const float* in, const float* w, const float* b, void* out16, int rows, int C, float eps,
                     int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Detection head.  Replaces Model.detection (model.py:133-158): mlp_classif -> sigmoid clamp (641-643) ->
 * max-pool NMS (620-638) -> threshold (612-617) -> (b, y, x) coordinates in torch.where order.
 * ---------------------------------------------------------------------------------------------------------- */
/* scores[m] = clamp(sigmoid(hid16[m] . w2 + b2), 1e-4, 1 - 1e-4); hid16 = relu(mlp_classif.0(features)) from
 * mhmr_gemm16(..., MHMR_EPI_OP16_RELU).                                                                      */
int mhmr_detect_scores(const void* hid16, int ld, const float* w2, const float* b2, float* scores, int rows, int C,
                       int dtype, void* stream);
/* pass 1: counts[b] = number of cells with nms(score) >= thr.  pass 2 (after the host prefix sum `base`):
 * ordered compaction into det_b/det_y/det_x/det_score.
 * The NMS window of cell (y, x) is (y - pad .. y - pad + k - 1) x (x - pad .. x - pad + k - 1), clipped to the image, pad = (k - 1) / 2
 * for odd k.  For k = 2 and k = 4 the reference pads its max-pool by 1 and 2 and crops the larger output top-left, so the window is
 * anchored up / left: k = 2 sees (y - 1 .. y) x (x - 1 .. x), k = 4 sees (y - 2 .. y + 1) x (x - 2 .. x + 1) -- a larger neighbour two
 * cells above suppresses a cell at k = 4, one two cells below does not.  A cell that equals its window's maximum keeps its score (ties
 * all survive); every other cell compares as score +0 against the threshold, so thr <= 0 returns EVERY cell, the suppressed ones with
 * det_score 0 (heat * keep >= thr in the reference).  Even k > 4: the reference raises (pad = (k - 1) / 2 makes its max-pool output
 * SMALLER than the map and the comparison with the map fails); these entry points do not refuse it and apply the same anchored window
 * with pad = (k - 1) / 2 -- untested, and nothing to compare it with.  nms_kernel < 1 or B <= 0 (or cap < 0): MHMR_ERR_BAD_ARG,
 * nothing is launched.                                                                                         */
int mhmr_detect_count(const float* scores, int B, int G, int nms_kernel, float thr, int* counts, void* stream);
int mhmr_detect_write(const float* scores, int B, int G, int nms_kernel, float thr, const int* base, int* det_b,
                      int* det_y, int* det_x, float* det_score, void* stream);
/* The same into buffers of `cap` entries: detections whose position is >= cap are dropped (the caller compares info[3] of
 * mhmr_person_groups with cap afterwards). */
int mhmr_detect_write_cap(const float* scores, int B, int G, int nms_kernel, float thr, const int* base, int* det_b,
                          int* det_y, int* det_x, float* det_score, int cap, void* stream);
/* The person set's bookkeeping ON THE DEVICE -- what the reference does on the host after torch.where (model.py:146-151) and in
 * rebatch / pad_to_max (utils/tensor_manip.py:7-45): per-image counts -> base[b] (exclusive prefix sums, nullable), gstart
 * [ngroups_cap + 1], chunks [3 * nchunks_cap] as mhmr_hph_forward reads them (unused tail entries = empty groups / count-0 items) and
 * info[4] = {persons kept = min(total, cap), groups, chunks, total}.  counts [B] from mhmr_detect_count, or NULL: the counts are the
 * histogram of det_b[0..P) (training hook: the caller's idx, sorted by image).  Sufficient bounds: ngroups_cap = min(B, cap),
 * nchunks_cap = cap / 8 + min(B, cap).  One workgroup builds the tables in LDS: (2 B + ngroups_cap + 1 + 3 nchunks_cap) ints must fit
 * 60 KB (B <= 8192 and, e.g., 2048 images with 16 persons each), MHMR_ERR_BAD_SHAPE otherwise. */
int mhmr_person_groups(const int* counts, const int* det_b, int P, int B, int cap, int* base, int* gstart, int ngroups_cap,
                       int* chunks, int nchunks_cap, int* info, void* stream);

/* Camera embedding.  Replaces Model.embedd_camera (model.py:160-187) + inverse_perspective_projection
 * (utils/camera.py:30-48) + FourierPositionEncoding (blocks/camera_embed.py:9-58) with num_bands frequency bands per ray component
 * (model.py:39 camera_embedding_num_bands; <= 20): E = 3 + 6 num_bands channels (99 for the released checkpoints' 16).  zK: [B*N, E]
 * fp32; also writes op16 copies to ctx16[:, C:C+E] and zeros ctx16[:, C+E:ldctx] (ldctx - C <= 128).  freq: [3*num_bands] =
 * linspace(1, max_resolution / 2, num_bands) x3.                                                                     */
int mhmr_camera_embed(const float* K, const float* freq, int B, int G, int patch, float* zK, void* ctx16, int ldctx,
                      int C, int dtype, int num_bands, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Human Perception Head.  Replaces HPH.cross_attn_inputs / HPH.forward (model.py:479-593), TransformerDecoder
 * (blocks/cross_attn_transformer.py:302-359), rot6d_to_rotmat (utils/humans.py:12-22), roma.rotmat_to_rotvec
 * (model.py:291), Model.to_euclidean_dist (model.py:189-203), mlp_offset + loc (model.py:258, 272-275).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *ln_sa_w, *ln_sa_b;  /* layers.l.0.norm                                  */
    const float* to_qkv;             /* [3*inner, dim]      layers.l.0.fn.to_qkv.weight  */
    const float *sa_out_w, *sa_out_b;/* [dim, inner],[dim]  layers.l.0.fn.to_out.0       */
    const float *ln_ca_w, *ln_ca_b;  /* layers.l.1.norm                                  */
    const void* to_kv16;             /* op16 [2*inner, Kc]  layers.l.1.fn.to_kv.weight, zero-padded columns */
    const float* to_q;               /* [inner, dim]        layers.l.1.fn.to_q.weight    */
    const float *ca_out_w, *ca_out_b;/* [dim, inner],[dim]  layers.l.1.fn.to_out.0       */
    const float *ln_ff_w, *ln_ff_b;  /* layers.l.2.norm                                  */
    const float *ff1_w, *ff1_b;      /* [mlp, dim],[mlp]    layers.l.2.fn.net.0          */
    const float *ff2_w, *ff2_b;      /* [dim, mlp],[dim]    layers.l.2.fn.net.3          */
} mhmr_hph_layer;

typedef struct {
    int dtype;
    int C, G, N;                 /* backbone dim, grid, tokens per image                                      */
    int Kc;                      /* context operand width: C + E (E = cam_dim) rounded up to a multiple of 64 */
    int dim, heads, mlp, depth;  /* 1024, xat_num_heads, 1024, xat_depth (model.py:122-126)                   */
    int nb;                      /* num_betas                                                                */
    int Ktok;                    /* token width C + E + 318 + nb + 3 rounded up to a multiple of 16          */
    int Ndec;                    /* 318 + nb + 3 + 10                                                        */
    int patch;                   /* 14                                                                       */
    int nearness;                /* model.py:196                                                             */
    float fn;                    /* S / (2 tan(30 deg)): focal length of the normalising 60-degree camera (utils/camera.py:71-77) */
    const float *off1_w, *off1_b, *off2_w, *off2_b; /* mlp_offset.{0,2}: [C,C],[C],[2,C],[2]                  */
    const float *cq_x, *cq_y, *cv_x, *cv_y;         /* cross_{queries,values}_{x,y}: [G, C+E]                 */
    const float* init_tail;      /* [318 + nb + 3] = init_body_pose | init_betas | init_cam                   */
    const float *tok_w, *tok_b;  /* to_token_embedding: [dim, Ktok] (zero padded), [dim] (+ pos_embedding[:,0]) */
    const mhmr_hph_layer* layers;/* HOST array of `depth`                                                    */
    const float *dec_w, *dec_b;  /* [Ndec, dim], [Ndec]: decpose|decshape|deccam|decexpression stacked, bias has the init_* added */
    /* workspaces for P persons (device, fp32 unless noted) */
    float* zc;      /* [P, C]        */
    float* token;   /* [P, Ktok]     */
    float* x;       /* [P, dim]      */
    float* xn;      /* [P, dim]      */
    float* t1;      /* [P, max(3*inner, mlp, C)] */
    float* t2;      /* [P, inner]    */
    float* kv;      /* [Mctx, 2*inner], Mctx = roundup(B*N, 128) */
    float* dec;     /* [P, Ndec]     */
    int* det_row;   /* [P]           */
    /* fixed-capacity callers (P = a capacity, the person count known on the device only): DEVICE pointer to the number of real persons
     * (mhmr_person_groups' info[0]); rows behind it are padding -- computed like persons, never allowed to touch the context operand.
     * NULL = all P rows are persons. */
    const int* nvalid;
    int cam_dim;    /* camera embedding channels E = 3 + 6 num_bands (0 = 99): context width C + E <= Kc, zK rows of E floats */
} mhmr_hph_desc;

/* Inputs: feat32 [B*N, C], zK [B*N, E], ctx16 op16 [Mctx, Kc] (features | camera | 0), detections det_{b,y,x}
 * [P] (sorted by (b, y, x)), gstart [ngroups+1] = person offsets of the non-empty images, chunks [nchunks*3] =
 * (image b, first person, count <= 8) cross-attention work items, K [B,3,3].  ngroups / nmax / nchunks size the launches and may be
 * UPPER BOUNDS when the tables come from mhmr_person_groups (empty groups and count-0 work items return at once).
 * Outputs: offset [P,2], loc [P,2], rotmat [P,53,3,3], rotvec [P,53,3], betas [P,nb], expr [P,10],
 * dist_pp [P] (raw), dist [P] (post-processed).                                                              */
int mhmr_hph_forward(const mhmr_hph_desc* d, const float* feat32, const float* zK, void* ctx16, const int* det_b,
                     const int* det_y, const int* det_x, int P, const int* gstart, int ngroups, int nmax,
                     const int* chunks, int nchunks, const float* K, int B, float* offset, float* loc, float* rotmat,
                     float* rotvec, float* betas, float* expr, float* dist_pp, float* dist, void* stream);

/* The decoder layer stack alone: `depth` x (self-attention among the queries of one image, cross-attention over the
 * image's N context tokens, GELU feed-forward), pre-norm, residual.  Replaces TransformerCrossAttn.forward of BOTH
 * blocks/cross_attn_transformer.py:239-261 (dim 1024 / 8 heads / mlp 1024 / depth 2) and the Anny variant
 * multi_hmr_anny/hph.py:114-151 (dim 512 / 16 heads / mlp 2048 / depth 8, context_dim = dim).  x [P, dim] is updated in
 * place; ctx16 op16 [roundup(B*N,128), Kc]; workspaces xn [P,dim], t1 [P, max(3*32*heads, mlp)], t2 [P, 32*heads],
 * kv [roundup(B*N,128), 64*heads] fp32; gstart / chunks as in mhmr_hph_forward.                                   */
int mhmr_xattn_layers_forward(const mhmr_hph_layer* layers, int depth, int dim, int heads, int mlp, int Kc, int N, int B,
                              int dtype, float* x, float* xn, float* t1, float* t2, float* kv, const void* ctx16,
                              const int* gstart, int ngroups, int nmax, const int* chunks, int nchunks, int P, void* stream);

/* Building blocks (unit tests). */
int mhmr_linear_f32(const float* X, int ldx, const int* row_idx, const float* W, int ldw, const float* bias,
                    const float* R, int ldr, float* Y, int ldy, int M, int N, int K, int act, void* stream);
int mhmr_layernorm_f32(const float* in, const float* w, const float* b, float* out, int rows, int C, float eps,
                       void* stream);
/* The three person-head kernels behind mhmr_xattn_layers_forward / mhmr_hph_forward, with caller-chosen tables (inner = 32 heads):
 *   mhmr_hph_self_attn:  qkv [P, 3 inner] (q | k | v) -> out [P, inner], softmax over the queries of each group gstart[g] .. gstart[g+1]
 *                        (ngroups / nmax may be upper bounds: repeated gstart entries are empty groups).
 *   mhmr_hph_cross_attn: q [P, inner], kv [B N, 2 inner] (k | v) -> out [P, inner] for the rows of the work items chunks[3 nchunks] =
 *                        (image, first query, count <= 8; count-0 padding items only at the tail); rows of no work item are not
 *                        written.
 *   mhmr_hph_decode:     dec [P, ldd] = [pose6d(318) | betas(nb) | cam(3) | expr(10)] -> rotmat, rotvec, betas, expr, dist_pp, dist
 *                        as in mhmr_hph_forward (K [B,3,3], det_b [P]).
 * MHMR_ERR_BAD_SHAPE for heads <= 0, N <= 0, nb outside [0, 64] or ldd < 318 + nb + 3 + 10, before any launch. */
int mhmr_hph_self_attn(const float* qkv, const int* gstart, float* out, int ngroups, int nmax, int heads, void* stream);
int mhmr_hph_cross_attn(const float* q, const float* kv, const int* chunks, int nchunks, float* out, int heads, int N, void* stream);
int mhmr_hph_decode(const float* dec, int ldd, int nb, const float* K, const int* det_b, float fn, int nearness,
                    float* rotmat, float* rotvec, float* betas, float* expr, float* dist_pp, float* dist, int P, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Backward of the decoder layer stack: the derivative of mhmr_xattn_layers_forward as its kernels
 * evaluate it, fp32; ctx16 and to_kv16 are 16-bit values taken as exact numbers (the gradient of to_kv is that of the
 * rounded weight).  Sums across persons, rows or tiles are fp64 or fp32 MFMA chains of a shape fixed by the sizes and
 * tables alone, there are no floating-point atomics, every element of every output is written, and two calls give the
 * same bits.  No entry allocates or synchronises; all validation happens before any launch.
 *
 * Building blocks (act = MHMR_ACT_*; Z = the TAPED pre-activation of the linear, read only when act != NONE):
 *   mhmr_linear_f32_backward_input:   dX[m][k] = sum_n dZ[row(m)][n] W[n][k] (+ dR[m][k]),  dZ = dY * act'(Z).  W [N, K];
 *       row_idx (nullable) gathers the rows of dY and Z; dR (nullable) is a residual cotangent added in the epilogue.
 *   mhmr_linear_f32_backward_weight:  dW[n][k] = sum_m dZ[m][n] X[m][k] (persons in index order, zero-padded to a
 *       multiple of 4), db[n] = sum_m dZ[m][n] in fp64.  dW or db may be NULL (not both).  M == 0 writes zeros.
 *   mhmr_layernorm_f32_backward:      dx (+ dR, nullable) of mhmr_layernorm_f32, one wave per row; dw, db = fp64 sums over
 *       the rows through two fixed stages.  C % 64 == 0, C <= 2048.
 *   mhmr_hph_self_attn_backward:      qkv [P, 3 inner], dOut [P, inner] -> dqkv [P, 3 inner] for the groups of gstart
 *       (as mhmr_hph_self_attn: groups of any size, empty groups allowed); lse_d [P, heads, 2] is scratch.
 *   mhmr_hph_cross_attn_backward:     q [P, inner], kv [B N, 2 inner], dOut [P, inner], chunks as mhmr_hph_cross_attn
 *       (count <= 8, count-0 padding items only at the tail; any number of items: one launch per 512) -> dq [P, inner] (rows
 *       of no work item are not written) and dkv [B N, 2 inner] (ALL rows written; rows of images without queries hold
 *       zeros).  dq or dkv may be NULL (not both).  lse_d [P, heads, 2] is scratch.  Items of one image must be
 *       consecutive and in person order (as mhmr_person_groups emits them).
 *   mhmr_grad_ctx_gemm:               dW[n][c] = sum_rows G[row][n] * op16[row][c], [Nn, Kc]; the row range is split into
 *       at most 16 slices whose partial products are added in slice order; columns c >= cvalid are exact zeros.
 * Return codes: MHMR_ERR_BAD_ARG for a negative count (M, rows, P, ngroups, nmax, nchunks), a NULL pointer that would be read
 * or written, or a short workspace; MHMR_ERR_BAD_SHAPE for the shape rules above, a leading dimension smaller than its row,
 * heads, B or a row-tile count above 65535 (launch limits: M > 16 * 65535 on the input side, LayerNorm rows > 32 * 65535),
 * B N >= 2^31.  An empty problem (M, rows, P == 0) returns 0.
 * ---------------------------------------------------------------------------------------------------------- */
int mhmr_linear_f32_backward_input(const float* dY, int lddy, const int* row_idx, const float* Z, int ldz, const float* W,
                                   int ldw, const float* dR, int lddr, float* dX, int lddx, int M, int N, int K, int act,
                                   void* stream);
int mhmr_linear_f32_backward_weight(const float* dY, int lddy, const float* Z, int ldz, const float* X, int ldx, float* dW,
                                    int lddw, float* db, int M, int N, int K, int act, void* stream);
long long mhmr_layernorm_f32_backward_workspace_bytes(int rows, int C);
int mhmr_layernorm_f32_backward(const float* x, const float* w, const float* dy, const float* dR, float* dx, float* dw,
                                float* db, int rows, int C, float eps, void* workspace, long long workspace_bytes,
                                void* stream);
int mhmr_hph_self_attn_backward(const float* qkv, const float* dOut, const int* gstart, float* dqkv, float* lse_d,
                                int ngroups, int nmax, int heads, void* stream);
int mhmr_hph_cross_attn_backward(const float* q, const float* kv, const float* dOut, const int* chunks, int nchunks,
                                 float* dq, float* dkv, float* lse_d, int heads, int N, int B, void* stream);
long long mhmr_grad_ctx_gemm_workspace_bytes(int rows, int Nn, int Kc);
int mhmr_grad_ctx_gemm(const float* G, int ldg, const void* op16, int ld16, float* dW, int rows, int Nn, int Kc,
                       int cvalid, int dtype, void* workspace, long long workspace_bytes, void* stream);

/* One gradient buffer per field of mhmr_hph_layer, in the field's shape; to_kv is fp32 [2 inner, Kc]. */
typedef struct {
    float *ln_sa_w, *ln_sa_b, *to_qkv, *sa_out_w, *sa_out_b, *ln_ca_w, *ln_ca_b, *to_kv, *to_q, *ca_out_w, *ca_out_b,
          *ln_ff_w, *ln_ff_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b;
} mhmr_hph_layer_grads;

typedef struct {
    const mhmr_hph_layer* layers;       /* HOST array of `depth`: the weights mhmr_xattn_layers_forward ran with */
    const mhmr_hph_layer_grads* grads;  /* HOST array of `depth`: outputs                                       */
    int depth, dim, heads, mlp, Kc, N, B, dtype;
    int P, ngroups, nmax, nchunks;      /* as mhmr_xattn_layers_forward                                          */
    int ctx_valid;                      /* columns >= ctx_valid of every g_to_kv are exact zeros (0 = Kc)        */
    const float* x0;                    /* [P, dim] the stack's INPUT (the forward overwrote its copy)           */
    const void* ctx16;                  /* op16 [roundup(B N, 128), Kc]                                          */
    const int *gstart, *chunks;
    const float* g_x_out;               /* [P, dim] cotangent of the stack's output                              */
    float* g_x0;                        /* [P, dim] out: cotangent of x0                                         */
    const int* det_row;                 /* [P] context row of each person (needed with g_ctx), else NULL         */
    float* g_ctx;                       /* [P, Kc] out, nullable: sum over the layers of dkv[det_row[p]] . to_kv */
    void* workspace;
    long long workspace_bytes;
    /* appended (additive): the DENSE cotangent of the context's first feat_cols columns, for every row */
    float* g_feat;                      /* [B N, ld_feat] out, nullable: sum over the layers of dkv . to_kv16[:, :feat_cols] */
    int ld_feat, feat_cols;
} mhmr_xattn_backward_desc;

/* The forward overwrites x in place, so the backward first re-runs the forward's own launchers, out of place, into a tape
 * inside the workspace (the inputs of the three sub-blocks, qkv, q, both attention outputs, the feed-forward's
 * pre-activation and its GELU), and recomputes kv per layer from ctx16 on the way back.  The workspace also holds dkv
 * [B N, 2 inner]: at 32 images of 4096 tokens and 8 heads that is 268 MB of the total.  The cotangent of the context is
 * returned only at the persons' own cells (g_ctx with det_row; straight-through past the 16-bit rounding), not for the
 * other rows.  mhmr_xattn_layers_backward_workspace_bytes: bytes for these shapes (monotone in P and depth); negative =
 * MHMR_ERR_BAD_ARG (depth, P < 0) or MHMR_ERR_BAD_SHAPE (the forward's shape rules, heads or B above 65535).
 * mhmr_xattn_layers_backward: MHMR_ERR_BAD_ARG for a NULL descriptor, a NULL pointer in it or in layers / grads, P < 0,
 * a short workspace, or P > 0 with ngroups, nmax or nchunks == 0 (persons that no group or no work item covers);
 * MHMR_ERR_BAD_SHAPE as above and for P > 16 * 65535; P == 0 launches nothing and returns 0. */
long long mhmr_xattn_layers_backward_workspace_bytes(int depth, int dim, int heads, int mlp, int Kc, int N, int B, int P);
int mhmr_xattn_layers_backward(const mhmr_xattn_backward_desc* d, void* stream);

/* The whole of mhmr_hph_forward up to the read-out, from g_readout [P, ldg >= Ndec] and g_offset [P, 2]: the dec linear, the stack, the
 * token embedding (g_tok_b is also the gradient of pos_embedding[0, 0], which the forward folds into that bias; the padding columns of
 * g_tok_w are zeros), the four tables of the HPH inputs and mlp_offset.  `fwd` is the descriptor mhmr_hph_forward ran with for THESE
 * persons: the backward reads its weights and the workspaces zc, token, x (the stack's output) and det_row as that call left them, and
 * ctx16 as it left it (context rows of the detected cells included) -- so it must run before the next forward into the same buffers.
 * Gradient buffers have the packed shapes: g_off1_w [C, C], g_off1_b [C], g_off2_w [2, C], g_off2_b [2], g_tok_w [dim, Ktok], g_tok_b
 * [dim], g_dec_w [Ndec, dim], g_dec_b [Ndec] (the init_* added into dec_b are buffers and get nothing), g_cq_x / g_cq_y / g_cv_x /
 * g_cv_y [G, C + E] (the *_x tables are indexed by the ROW y, the *_y tables by the COLUMN x, as in the forward; rows nobody indexes
 * are zeros), layer_grads as in mhmr_xattn_layers_backward.  g_zc [P, C] and g_token [P, Ktok] are the cotangents of the gathered
 * features, returned for a backbone backward.  Every row of fwd is a person (fwd->nvalid is not read).  Two persons in one cell of one
 * image are outside the contract, as they are for the reference's indexed assignment; nothing checks for them.
 * MHMR_ERR_BAD_ARG: NULL descriptor / fwd / pointer, P < 0, short workspace, P > 0 with ngroups, nmax or nchunks == 0; MHMR_ERR_BAD_SHAPE: the forward's shape rules, Ndec !=
 * 318 + nb + 13, ldg < Ndec, the launch limits of mhmr_xattn_layers_backward.  P == 0 launches nothing and returns 0. */
typedef struct {
    const mhmr_hph_desc* fwd;
    const void* ctx16;
    const int *det_y, *det_x;           /* [P]                                                                   */
    const int *gstart, *chunks;
    int ngroups, nmax, nchunks, P, B;   /* as mhmr_hph_forward                                                   */
    const float* g_readout;             /* [P, ldg]                                                              */
    int ldg;
    const float* g_offset;              /* [P, 2]                                                                */
    float *g_off1_w, *g_off1_b, *g_off2_w, *g_off2_b, *g_tok_w, *g_tok_b, *g_dec_w, *g_dec_b, *g_cq_x, *g_cq_y, *g_cv_x, *g_cv_y;
    const mhmr_hph_layer_grads* layer_grads;  /* HOST array of fwd->depth                                        */
    float *g_zc, *g_token;
    void* workspace;
    long long workspace_bytes;
    /* appended (additive): the cotangent of feat32 itself, every row of every image */
    float* g_feat;                      /* [B N, ld_feat >= C] out, nullable                                     */
    int ld_feat;
} mhmr_hph_backward_desc;
long long mhmr_hph_backward_workspace_bytes(const mhmr_hph_desc* fwd, int B, int P);
int mhmr_hph_backward(const mhmr_hph_backward_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The cotangent of the features: what the heads send back to feat32 [B N, C], straight-through past the
 * 16-bit rounding of the context operand and of the detector's hidden layer; the rounded 16-bit weights are exact numbers.
 *
 *   g_feat[m][c] =  sum over the persons p whose cell is row m of g_zc[p][c] + g_token[p][c]
 *                 + sum over the decoder layers l, in the order the backward visits them, of sum_n dkv_l[m][n] to_kv16_l[n][c]
 *                 + sum_n (hid16[m][n] > 0 ? dl_m w2[n] : 0) cls0_w16[n][c]                       (the detector; dl as mhmr_detect_backward)
 *
 * The first two lines are mhmr_hph_backward_desc.g_feat (mhmr_xattn_backward_desc.g_feat is the second line alone, for its first
 * feat_cols columns): the first layer visited WRITES every element of the B N rows, the later layers add, the persons' rows are added
 * last; rows of images without queries hold exact zeros; P == 0 (or depth == 0) writes zeros.  NULL changes nothing.  With g_feat,
 * C (feat_cols) % 128 == 0, C <= Kc and ld_feat >= C, MHMR_ERR_BAD_SHAPE otherwise.  The context row of a detected cell is
 * op16(feat32 + cv_x + cv_y): its derivative with respect to feat32 is the identity, so the dense line covers those rows and g_ctx
 * is not added again.  The third line is mhmr_detect_feature_grad.
 *
 * Both dense lines are one product, mhmr_rows_times_weight: out[m][c] (+)= sum_n left[m][n] w16[n][c] with left fp32 [rows, ldl >= n],
 * w16 op16 [n, ldw >= C], out fp32 [rows, ldo >= C]; n % 16 == 0, C % 128 == 0.  Exact-fp32 MFMA (an fmaf chain per output element, of
 * a shape the sizes alone fix); no sum crosses rows, so a row's bits do not depend on the other rows or on their number; no atomics;
 * every element of the `rows` rows is written (pitch columns >= C are not touched); two calls give the same bits.  accumulate != 0:
 * out = out + product (the bits of a write followed by an fp32 add).
 * mhmr_detect_feature_grad forms the left operand of the detector's line in registers (the [rows, C] cotangent of the hidden layer is
 * never stored) and writes g_feat [rows, ldg >= C]; rows outside the clamp (clamped != 0) and rows with a zero cotangent are exact
 * zeros.  Its workspace is dl [rows] fp32 (mhmr_detect_feature_grad_workspace_bytes), left in place: dl_m as the product used it.
 * mhmr_features_to_context: feat32 [rows, C] = features (skipped when features == feat32; any other overlap of the two is
 * MHMR_ERR_BAD_ARG) and ctx16[m][c] = op16(features[m][c]) for c < C, round to nearest even -- what the final LayerNorm of
 * mhmr_vit_forward leaves in those two buffers for the same fp32 values.  `features` is only read.
 * MHMR_ERR_BAD_ARG: rows < 0, a NULL pointer that would be read or written, a short workspace; MHMR_ERR_BAD_SHAPE: the size rules
 * above, a leading dimension smaller than its row, ldh odd, an unknown dtype, more than 2^24 - 1 workgroups of 64 rows x 128 columns
 * (a launch limit), rows C >= 2^32 - 256 (mhmr_features_to_context), rows > 512 * 65535 (mhmr_detect_feature_grad).  rows == 0
 * launches nothing and returns 0.  No allocation, no synchronisation; all validation happens before any launch.
 * ---------------------------------------------------------------------------------------------------------- */
int mhmr_rows_times_weight(const float* left, int ldl, const void* w16, int ldw, float* out, int ldo, int rows, int n, int C,
                           int accumulate, int dtype, void* stream);
long long mhmr_detect_feature_grad_workspace_bytes(int rows);
int mhmr_detect_feature_grad(const void* hid16, int ldh, const void* cls0_w16, int ldw, const float* w2, const float* b2,
                             const float* g_scores, int rows, int C, int clamped, int dtype, float* g_feat, int ldg,
                             void* workspace, long long workspace_bytes, void* stream);
int mhmr_features_to_context(const float* features, float* feat32, void* ctx16, int ldctx, int rows, int C, int dtype,
                             void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Backward of the detection head mlp_classif (csrc/detect_bwd.hip): the derivative of
 * mhmr_gemm16(EPI_OP16_RELU) -> mhmr_detect_scores (clamped = 1) or mhmr_anny_scores (clamped = 0) as those kernels
 * evaluate them.  hid16 [rows, ldh] (the stored ReLU output), ctx16 [rows, ldx] (columns < C are read) and the rounded
 * first-layer weight are exact numbers (straight-through); the ReLU mask is hid16 > 0.  With p = sigmoid(hid16[m] . w2 + b2)
 * (the forward's dot product) and dl_m = g_scores[m] p (1 - p), or 0 where clamped and p lies outside [1e-4, 1 - 1e-4]:
 *   g_b2 [1] = sum dl_m    g_w2 [C] = sum dl_m hid16[m][n]    g_b1 [C] = w2[n] sum dl_m [hid16[m][n] > 0]
 *   g_w1 [C, C]: g_w1[n][c] = w2[n] sum dl_m [hid16[m][n] > 0] ctx16[m][c]
 * over the `rows` real rows only.  The column sums are fp64 in two fixed stages (slices of 512 rows) over the unrounded fp64 dl; g_w1 is an fp32 MFMA
 * chain over the rows in index order, the row range cut into min(16, ceil(rows / 512)) slices whose partial products are
 * added in slice order in fp64.  The hidden layer's [rows, C] cotangent is never stored: the workspace is at most
 * 16 C C 4 + 4 rows + 16 C ceil(rows / 512) bytes (+ alignment).  No atomics; two calls give the same bits; every element
 * of the four outputs is written (rows == 0: zeros).
 * MHMR_ERR_BAD_ARG: rows < 0, a NULL pointer that would be read or written, a short workspace; MHMR_ERR_BAD_SHAPE:
 * C <= 0, C % 128, C > 16384, ldh < C, ldh odd, ldx < C, an unknown dtype, rows > 512 * 65535 (a launch limit).
 * ---------------------------------------------------------------------------------------------------------- */
long long mhmr_detect_backward_workspace_bytes(int rows, int C);
int mhmr_detect_backward(const void* hid16, int ldh, const void* ctx16, int ldx, const float* w2, const float* b2,
                         const float* g_scores, int rows, int C, int clamped, int dtype, float* g_w1, float* g_b1,
                         float* g_w2, float* g_b2, void* workspace, long long workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * SMPL-X layer.  Replaces SMPL_Layer.forward (blocks/smpl_layer.py:47-155) -> smplx.SMPLX.forward / lbs,
 * roma.rotvec_to_rotmat (:107), inverse_perspective_projection (:117-123), perspective_projection (:143-144).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int V, Vp, Vl;        /* 10475; columns of the vertex kernel's operands: V rounded up to a multiple of 48 (= Vl, the kernel's tile) + the
                             tiles of the 72 extra joints (21 picked vertices + 51 barycentric landmarks) as VIRTUAL vertices: extra
                             joint e = 16 t + i owns column Vl + 48 t + 16 k + i, k = 0..2 = copies of its three corner vertices' columns
                             (a picked vertex: three copies of itself), Vp = Vl + 48 * 5                                       */
    int Kb;               /* 486 + nb + 10 rounded up to a multiple of 32 (width of the feature rows F); the vertex kernel is built for
                             Kb == 512, i.e. num_betas <= 16 (MHMR_ERR_BAD_SHAPE otherwise)                     */
    int nb, Kinf;         /* num_betas, max skinning influences per vertex                                   */
    int center_joint;     /* JOINT_NAMES.index(person_center) = 15 ('head'); < 0 = person_center None: nothing is
                             recentred and the pelvis is added to the translation (smpl_layer.py:128-130)       */
    const void* basis16;  /* f16, 1024 x [posedirs(486) | shapedirs(nb) | exprdirs(10) | 0], tile-major (the slice of a 48-vertex tile is
                             one contiguous block of 82944 values): [Vp/48]{ [Kb/8 - 8][3][48][8] the HIGH halves of k < Kb - 64 (pose
                             correctives: one product per term in the kernel), then [8][2][3][48][8] hi + lo of the last 64 k (the last
                             pose columns, every shape / expression direction: fp32 accuracy) }                              */
    const float* vtemp;   /* [3][Vp]           v_template, fp32                                                */
    const float* J0;      /* [55*3]            J_regressor . v_template                                      */
    const float* JS;      /* [55*3][nb+10]     J_regressor . [shapedirs | exprdirs]                          */
    const int* parents;   /* [55]                                                                            */
    const int* skin_idx;  /* [V][Kinf]         K-sparse skinning list (kept for tools; the kernel reads skin16)        */
    const float* skin_w;  /* [V][Kinf]                                                                       */
    const void* skin16;   /* f16 [Vp/48][8][2][48][8]: the DENSE skinning weights w[v][j] (joints 55..63 zero), hi + lo,
                             j = 8 * block + lane-local index: the B operand of the skinning GEMM            */
    const float* xbary;   /* [72*3]            corner weights of the extra joints: (1, 0, 0) for joints 55..75 (vertices picked by id),
                             lmk_bary_coords for 76..126 (faces[lmk_faces_idx] are the corners)                 */
    /* (105) The kinematic tree's level schedule, or NULL (then the pose kernel derives it from `parents` at run time).  int32 [16][256]:
     * pose_tasks[level][lane] = joint | parent << 8 (parent 0xff = a root) for lane = 12 * (position of the joint in its level's list, in
     * joint order) + element (0..8 of the rotation, 9..11 of the translation), -1 where the level has no such lane; pose_levels = number of
     * tree levels.  Only for trees of at most 16 levels with at most 21 joints per level (SMPL-X: 10 levels, <= 13 joints). */
    const int* pose_tasks;
    int pose_levels;
} mhmr_lbs_consts;

/* rotvec [P,53,3], betas [P,nb], expr [P,10], loc [P,2], dist [P], K [B,3,3], det_b [P] (image of each person).
 * Workspaces (fp32-sized, contents are f16 operand matrices): ws_F [roundup(P,16), Kb], ws_A [roundup(P,16), 768], ws_xf [P,24].
 * Outputs: v3d [P,V,3], v2d [P,V,2], j3d [P,127,3], j2d [P,127,2], transl [P,3]  (transl_pelvis = j3d[:,0]). */
int mhmr_lbs_forward(const mhmr_lbs_consts* c, const float* rotvec, const float* betas, const float* expr,
                     const float* loc, const float* dist, const float* K, const int* det_b, int P, float* ws_F,
                     float* ws_A, float* ws_xf, float* v3d, float* v2d, float* j3d, float* j2d, float* transl,
                     void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Anny variant read-outs; the backbone, the detection head and the decoder stack reuse
 * mhmr_vit_forward / mhmr_detect_* / mhmr_xattn_layers_forward.
 *   mhmr_anny_camera: multi_hmr_anny/encoder.py:47-56 -- fov = fov_max * sigmoid(logit), focal = (S/2) / tan(fov/2),
 *                     K [B][3][3] with the principal point at S/2.
 *   mhmr_anny_decode: multi_hmr_anny/multi_hmr.py:144-177 -- per person: loc, dist = focal / clamp(exp(d), 1e-5),
 *                     transl = K^-1 [loc,1] dist (utils/camera.py:30-48), J 6D rotations (rows of (3,2)) ->
 *                     roma.special_gramschmidt -> identity where useful[j] == 0 -> roma.rotmat_to_rotvec,
 *                     shape = sigmoid(shape_logit).  The body model (anny package) is outside this library.
 * ---------------------------------------------------------------------------------------------------------- */
/* encoder.py:57-58: logits = hid16 . w2 + b2, scores = sigmoid(logits) (no clamp); hid16 as for mhmr_detect_scores. */
int mhmr_anny_scores(const void* hid16, int ld, const float* w2, const float* b2, float* scores, float* logits, int rows,
                     int C, int dtype, void* stream);
int mhmr_anny_camera(const float* fov_logit, int B, int img_size, float fov_max, float* fov, float* K, void* stream);
int mhmr_anny_decode(const float* rot6d, const float* useful, int J, const float* shape_logit, int nb,
                     const float* dist_logit, const float* offset, const int* det_b, const int* det_y, const int* det_x,
                     const float* K, int patch, int P, float* rotmat, float* rotvec, float* shape, float* loc, float* dist,
                     float* transl, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input preprocessing, the step before Model.forward:
 *   demo.py:27-51 open_image  = PIL ImageOps.contain(img, (S,S)) [bicubic, aspect kept] + ImageOps.pad(.., (S,S))
 *                               [centred, black] + utils/image.py:12-24 normalize_rgb.
 * img: decoded uint8 RGB [H][W][3] on the device.  The resample is Pillow's 8-bit two-pass convolution in its
 * own fixed point (22 fractional bits), bit-identical to PIL: the host passes Pillow's coefficient tables
 * (multi_hmr_amd/preprocess.py: kh [ow][ksh] / kv [oh][ksv] int32, bounds bh [ow][2] / bv [oh][2] = (first tap,
 * tap count)) and the 3 x 256 normalisation table lut (the reference's numpy expression evaluated on 0..255).
 * Only source rows y0 .. y0+rows-1 (those the vertical taps touch) are resampled horizontally into tmp
 * [rows][ow][3] uint8.  out: [3][S][S] fp32, the resized image at (pad_x, pad_y), lut[c][0] elsewhere.
 * ---------------------------------------------------------------------------------------------------------- */
int mhmr_preprocess_u8(const void* img, int H, int W, const int* kh, const int* bh, int ksh, const int* kv,
                       const int* bv, int ksv, int ow, int oh, int y0, int rows, int S, int pad_x, int pad_y,
                       const float* lut, void* tmp, float* out, void* stream);

/* The same for B images of different sizes in TWO launches (horizontal pass, vertical pass + pad + lut, each over a
 * (block, image) grid; B <= 65535) -> out [B][3][S][S] fp32, the tensor Model.forward takes.  Per pixel the arithmetic is
 * mhmr_preprocess_u8's, so image b of the batch is bit-identical to the one-image call (and to PIL).
 * One descriptor per image: its geometry exactly as the arguments of mhmr_preprocess_u8, and DEVICE pointers of the
 * decoded image (anywhere on the device: a tensor of its own, a slice of a staging buffer, a decoder's frame), of the
 * tables of its geometry (two images of one size may share them) and of its own tmp [rows][ow][3] slice (slices of
 * two images must not overlap).
 * The descriptors are passed twice: `host` [B] is read by this function to validate every image before any launch
 * and to size the grids; `dev` [B] is a device copy of the same bytes, which the kernels read.  The caller makes that
 * copy on `stream` (or otherwise before the call in stream order) and keeps both alive: `host` until the call returns,
 * `dev` until the work has run.  B <= 0, S <= 0, B > 65535 or a per-image shape condition of mhmr_preprocess_u8 ->
 * MHMR_ERR_BAD_SHAPE; a null pointer (arguments or descriptor fields) -> MHMR_ERR_BAD_ARG. */
typedef struct {
    const void* img;                                   /* uint8 [H][W][3], device */
    int H, W, ow, oh, y0, rows, pad_x, pad_y, ksh, ksv;
    const int *kh, *bh, *kv, *bv;                      /* device; formats as for mhmr_preprocess_u8 */
    void* tmp;                                         /* uint8 [rows][ow][3], device */
} mhmr_pre_image;
int mhmr_preprocess_u8_batch(const mhmr_pre_image* host, const mhmr_pre_image* dev, int B, int S, const float* lut,
                             float* out, void* stream);

/* mhmr_preprocess_u8_batch for sources that are read through a rotation and / or a mirror, as the training loaders orient
 * them (datasets/bedlam.py:222-229: img.rotate(-90, expand=True) for the "closeup" sequences, then ImageOps.mirror for
 * the random flip, then contain + pad): no oriented copy of the source is made, the horizontal pass addresses the stored
 * buffer through the permutation.  orient: bit 0 (MHMR_ORIENT_MIRROR) = mirror, applied AFTER the rotation; bit 1
 * (MHMR_ORIENT_ROT90) = rotate by 90 degrees clockwise (PIL's Transpose.ROTATE_270).  With (oW, oH) = (H, W) if rotated,
 * (W, H) otherwise, the ORIENTED image is
 *     or[y][x] = rotated ? img[H - 1 - x'][y] : img[y][x'],    x' = mirrored ? oW - 1 - x : x,    0 <= x < oW, 0 <= y < oH.
 * H and W describe the STORED buffer img [H][W][3]; everything else -- the tables kh / bh / kv / bv, ow, oh, y0, rows,
 * pad_x, pad_y and tmp [rows][ow][3] -- describes the oriented image, exactly as mhmr_preprocess_u8 would be given them
 * for an oW x oH source (y0 + rows <= oH).  Per output pixel the arithmetic is mhmr_preprocess_u8's; with orient = 0 the
 * output equals mhmr_preprocess_u8_batch's bit for bit.  Two launches, one descriptor per image, host / dev as above; no
 * allocation, no synchronisation, no atomics.  A bit of orient other than 0 and 1 -> MHMR_ERR_BAD_ARG; the other conditions
 * and codes are those of mhmr_preprocess_u8_batch; every descriptor is checked before the first launch. */
#define MHMR_ORIENT_MIRROR 1
#define MHMR_ORIENT_ROT90 2
typedef struct {
    const void* img;                                   /* uint8 [H][W][3] as stored, device */
    int H, W, ow, oh, y0, rows, pad_x, pad_y, ksh, ksv;
    const int *kh, *bh, *kv, *bv;                      /* device; tables of the oriented image */
    void* tmp;                                         /* uint8 [rows][ow][3], device */
    int orient;                                        /* MHMR_ORIENT_* bits */
} mhmr_pre_image_o;
int mhmr_preprocess_u8_batch_oriented(const mhmr_pre_image_o* host, const mhmr_pre_image_o* dev, int B, int S,
                                      const float* lut, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Accuracy metrics of the reference's evaluation loop, train.py:372-395 (PVE, PA-PVE) and
 * 415-423 (MPJPE, PA-MPJPE): for M matched pairs of V points, pred / gt [M][V][3] fp32, optionally recentred by
 * pred_center / gt_center [M][3] (the pelvis translations; NULL = none):
 *   pve[m]    = mean_n |gt_n - pred_n| * 1000
 *   pa_pve[m] = mean_n |gt_n - (s R pred_n + t)| * 1000,  (R, t, s) = roma.rigid_points_registration(pred, gt,
 *               compute_scaling=True)  (proper rotation; scale = tr(R^T M) / sum |pred - mean|^2)
 * Rts (nullable) [M][13] receives R (row-major 9), t (3), s.
 * ---------------------------------------------------------------------------------------------------------- */
int mhmr_eval_mesh_errors(const float* pred, const float* gt, const float* pred_center, const float* gt_center, int M,
                          int V, float* pve, float* pa_pve, float* Rts, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluation of a whole batch on the device: the reference's greedy 2D matching
 * (utils/training.py:26-147, the form its evaluation calls: valid=None, every joint valid) image by image, and the
 * metrics above read through the matcher's pair list.  Nothing is copied back and nothing synchronises.
 *
 * mhmr_eval_match.  Predictions pred_j2d: P rows, pred_stride floats apart (>= 2 J), of which the first J joints
 * (x, y) are read; pred_img [P] the image of each row, ascending, in [0, B).  Ground truth gt_j2d [G][J][2] and
 * gt_img [G], likewise.  One workgroup per image; an image may have no prediction, no ground truth, or neither.
 *   cost(p, g)  np.linalg.norm(D, 2), the SPECTRAL norm of the [J][2] matrix D = pred - gt formed in fp32: with
 *               a = sum dx^2, b = sum dx dy, c = sum dy^2 accumulated in fp64 in joint order,
 *               cost = sqrt((a + c) / 2 + sqrt(((a - c) / 2)^2 + b^2)).
 *   iou(p, g)   get_bbx_overlap of the two boxes over all J joints, in fp32 in the host code's operation order
 *               (inclusive +1 pixel convention; every operation rounded on its own), compared as fp32 with
 *               iou_thresh.
 *   loop        while assigned_gt < nG and assigned_pred + fp_rounds < nP: take the remaining pair of lowest
 *               cost (lowest flat index p nG + g on ties, as np.argmin) and remove it; both members free and
 *               iou >= iou_thresh: a match; iou < iou_thresh, whatever the members' state: one false-positive
 *               round (the loop's own counter); otherwise go on.  When the pairs run out the loop stops.
 * Outputs.  Image i owns min(nP_i, nG_i) consecutive slots of pair_pred / pair_gt [min(P, G)], in image order;
 * its matches fill them in the order the loop finds them, as indices into the P and G rows; every other slot is
 * -1.  pred_fp [P] / gt_miss [G]: 1 for a prediction / ground truth without a match, else 0.  counters [4] int64
 * {count, miss, fp, matched} (count = ground truths, miss / fp = the two flags' sums): ADDED to; the images'
 * partial counts are summed by one thread in image order.  status [1]: STICKY (ORed into), bits MHMR_EVAL_*:
 *   DEGENERATE_BOX  an image with pairs has a person whose box has no width or no height (the host's assert);
 *   NONFINITE       a keypoint among the J of a row is NaN or infinite;
 *   BAD_IMAGE_IDS   an image column is not ascending or leaves [0, B): the whole call matches nothing.
 * An image with one of the first two bits is left out: its slots -1, its flags 0, nothing counted; the other
 * images of the call are unaffected.  workspace: mhmr_eval_match_workspace_bytes(P, G, B) bytes, 8-byte aligned
 * (the fp64 cost slabs [sum_i nP_i nG_i <= P G], the boxes, the images' segments and partial counts): there is no
 * per-image capacity.  P, G <= MHMR_EVAL_MAX_PERSONS, B <= MHMR_EVAL_MAX_IMAGES (MHMR_ERR_BAD_SHAPE); P = 0 and
 * G = 0 are ordinary inputs (their pointers may be NULL).  Three launches on `stream`.
 *
 * mhmr_eval_mesh_errors_indexed.  mhmr_eval_mesh_errors with pair m's point sets read at pred[pair_pred[m]]
 * ([P][V][3]) and gt[pair_gt[m]] ([G][V][3]); the centres ([P][3] / [G][3], NULL = none) are indexed the same
 * way.  The arithmetic of a pair is that entry's (one device function): pve[m] / pa_pve[m] carry the bits it
 * gives on gathered copies.  A slot whose index is outside [0, P) / [0, G) (the matcher's -1) writes 0.
 * sums (nullable) [2] fp64: a second launch of one workgroup adds the valid slots' pve / pa_pve in slot order, in
 * fp64, and ADDS the two totals to sums; n_valid (nullable, needs sums) [1] int64 gains the number of valid slots.
 * M == 0 launches nothing.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_EVAL_DEGENERATE_BOX 1
#define MHMR_EVAL_NONFINITE 2
#define MHMR_EVAL_BAD_IMAGE_IDS 4
#define MHMR_EVAL_MAX_PERSONS 8192
#define MHMR_EVAL_MAX_IMAGES 65535
long long mhmr_eval_match_workspace_bytes(int P, int G, int B);
int mhmr_eval_match(const float* pred_j2d, long long pred_stride, const int* pred_img, int P, const float* gt_j2d,
                    const int* gt_img, int G, int J, int B, float iou_thresh, void* workspace, long long workspace_bytes,
                    int* pair_pred, int* pair_gt, int* pred_fp, int* gt_miss, long long* counters, int* status,
                    void* stream);
int mhmr_eval_mesh_errors_indexed(const float* pred, const float* gt, const float* pred_center, const float* gt_center,
                                  const int* pair_pred, const int* pair_gt, int P, int G, int M, int V, float* pve,
                                  float* pa_pve, double* sums, long long* n_valid, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ground truth for the evaluation loop: what the reference's Trainer.prepare_gt (train.py:58-182)
 * and the 3DPW branch of its evaluate (train.py:383-429) compute with the smplx package and dense matrices.
 *
 * mhmr_body_forward: smplx.lbs.lbs (pose2rot=True) for a body model described by data -- SMPL (6890 vertices, 24
 * joints), SMPL-X (10475, 55) or any other member of the family -- in fp32 throughout, with fp32 constants:
 *   pose [G][J][3] rotation vectors, joint 0 = the global orientation (applied about the rest pelvis, as upstream);
 *   batch_rodrigues' convention angle = |v + 1e-8|;  coef [G][nc] = [betas | expression];  transl [G][3] (NULL = 0)
 *   added to vertices and joints;  K [G][3][3] (NULL = no projection; utils/camera.py:14-27 otherwise).
 *   vertices [G][V][3];  joints [G][J + E + L][3] = the posed joints, E vertices picked by id, L barycentric
 *   landmarks (sum_f bary[l][f] * vertex lmk_idx[l][f]);  v2d [G][V][2], j2d [G][J + E + L][2] when K is given.
 * Workspaces: ws_F [ceil(G / 8)][K][8] floats, ws_A [G][J][12] floats.  Three launches on `stream`, no allocation,
 * no synchronisation.  J > 64, K != nc + 9 (J - 1), K > 1536 or Vp not a multiple of 64 -> MHMR_ERR_BAD_SHAPE;
 * G == 0 launches nothing.  parents[i] < i for i > 0 is the caller's duty (multi_hmr_amd/bodymodel.py checks it); a table
 * that breaks it is not refused here: see `parents` below.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int V, Vp;                /* vertices; V rounded up to a multiple of 64 (columns of the operands, zero-padded)   */
    int J, nc, K;             /* joints; shape + expression directions; K = nc + 9 (J - 1) rows of the basis          */
    int E, L;                 /* picked-vertex joints, landmarks (either may be 0)                                    */
    const float* vtemp;       /* [3][Vp]       v_template                                                             */
    const float* basis;       /* [K][3][Vp]    [shapedirs(nb) | exprdirs(ne) | posedirs(9 (J - 1))]                  */
    const float* J0;          /* [J*3]         J_regressor . v_template                                               */
    const float* JS;          /* [J*3][nc]     J_regressor . dirs                                                     */
    const int* parents;       /* [J]           parents[0] is ignored; for i > 0 mhmr_body_forward and mhmr_body_backward both
                                               read parents[i] clamped into [0, i - 1], so a malformed table is walked as
                                               the same tree in both directions (a well-formed one is read as it stands)     */
    const float* weights;     /* [J][Vp]       dense skinning weights, joint-major                                    */
    const int* extra_idx;     /* [E]                                                                                  */
    const int* lmk_idx;       /* [L][3]        faces[lmk_faces_idx]                                                   */
    const float* lmk_bary;    /* [L][3]                                                                               */
} mhmr_body_consts;

int mhmr_body_forward(const mhmr_body_consts* c, const float* pose, const float* coef, const float* transl, const float* K, int G,
                      float* ws_F, float* ws_A, float* vertices, float* joints, float* v2d, float* j2d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Backward of mhmr_body_forward: cotangents of the outputs -> gradients of pose, coef and
 * transl.  K and the model constants get no gradient.
 *   saved from the forward of the SAME (c, G): its inputs pose, coef, transl, K and what it wrote: ws_F, ws_A,
 *   vertices, joints;
 *   cotangents g_vertices [G][V][3], g_joints [G][J + E + L][3], g_v2d [G][V][2], g_j2d [G][J + E + L][2]: any
 *   may be NULL (= zero); the 2D ones need K;
 *   outputs g_pose [G][J][3], g_coef [G][nc], g_transl [G][3]: any may be NULL (not wanted); g_transl needs transl.
 * The picked-vertex joints and landmarks reach the vertices through mhmr_body_bwd_consts: their table inverted
 * once at load time, CSR by vertex -- the entries of vertex v are inv_ptr[v] .. inv_ptr[v + 1], each an output
 * joint (J <= joint < J + E + L) and its weight (1 for a picked vertex, the barycentric weight for a landmark
 * corner), sorted by joint; n = E + 3 L entries.
 * Two launches on `stream`, no allocation, no synchronisation, no floating-point atomic: sums over the 64 vertices
 * of a tile are fp32 in a fixed tree, every sum above that is fp64 in an order that depends on (V, G) only, each
 * output is rounded once.  Two calls give the same bits; a person's gradient does not depend on the other persons
 * of the batch.  The pose gradient differentiates batch_rodrigues as the forward evaluates it (angle = |v + 1e-8|):
 * a zero rotation vector is an ordinary input.
 * Validated before any launch: d, c, a required pointer or the workspace NULL, G < 0, workspace_bytes too small,
 * g_v2d / g_j2d without K, g_transl without transl, bc->n != E + 3 L -> MHMR_ERR_BAD_ARG; the shape limits of
 * mhmr_body_forward -> MHMR_ERR_BAD_SHAPE; G == 0 launches nothing.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int n;                    /* E + 3 L                                                                              */
    const int* inv_ptr;       /* [V + 1]                                                                              */
    const int* inv_joint;     /* [n]                                                                                  */
    const float* inv_w;       /* [n]                                                                                  */
} mhmr_body_bwd_consts;

typedef struct {
    const mhmr_body_consts* c;
    const mhmr_body_bwd_consts* bc;
    int G;
    const float *pose, *coef, *transl, *K;
    const float *ws_F, *ws_A, *vertices, *joints;
    const float *g_vertices, *g_joints, *g_v2d, *g_j2d;
    float *g_pose, *g_coef, *g_transl;
    void* workspace;
    long long workspace_bytes;
} mhmr_body_backward_desc;

/* bytes of the fp64 partial sums mhmr_body_backward needs: a function of the shapes in c and of G only (the number
 * of tile ranges per group of 8 persons grows when there are few groups); written before it is read.  A negative
 * value is MHMR_ERR_BAD_ARG (c NULL, G < 0) or MHMR_ERR_BAD_SHAPE. */
long long mhmr_body_backward_workspace_bytes(const mhmr_body_consts* c, int G);
int mhmr_body_backward(const mhmr_body_backward_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Differentiable prediction decode: from the HPH read-out row
 *   readout [P][ldr] = [pose6d(318) | betas(nb) | cam(3) | expr(10)]  (decoder output + init, reference model.py:571-575)
 * and the 2-vector of mlp_offset to the training-mode outputs, and the cotangents of those outputs back.
 *
 * mhmr_heads_decode: the forward, for given readout / offset / det_* / K [B][3][3] -- reference model.py:272-275
 *   (loc = (cell + 0.5 + offset) patch), utils/humans.py:12-22 + roma.special_gramschmidt (6D -> rotmat),
 *   model.py:287-298 + roma.rotmat_to_rotvec, utils/camera.py:71-90 + model.py:196-203 (distance: focal
 *   normalisation, exp, clamp to [0, 50]).  It launches the kernels of mhmr_hph_forward, so loc, rotmat [P][53][3][3],
 *   rotvec [P][53][3], shape [P][nb], expression [P][10], dist_postprocessed [P], dist [P] are bit-equal to what
 *   that entry leaves for the same read-out.
 * mhmr_heads_place_backward: the derivative of the SMPL-X layer's placement, blocks/smpl_layer.py:116-144 --
 *   x = u - u_joint[center_joint] + transl for the V vertices and NJ output joints u of mhmr_body_forward run
 *   without transl and K (center_joint < 0: x = u + transl, :128-130), v2d / j2d = utils/camera.py:14-27 of x with
 *   K[det_b[p]] (det_b NULL: K[p]).  Cotangents g_v3d [P][V][3], g_j3d [P][NJ][3], g_v2d [P][V][2], g_j2d [P][NJ][2],
 *   g_transl [P][3]: any may be NULL (= zero).  Written: gx_v [P][V][3], gx_j [P][NJ][3] (the cotangents of u: feed
 *   them to mhmr_body_backward as g_vertices / g_joints) and g_transl_total [P][3] = sum of a person's gx + g_transl.
 *   One streaming pass + a finishing launch; elements fp32, sums fp64 in an order that depends on (V, NJ) only
 *   (lane in index order, wave butterfly, waves in index order, tiles in index order), no floating-point atomic:
 *   two calls give the same bits and a person's numbers do not depend on the rest of the batch.
 * mhmr_heads_decode_backward: the derivative of mhmr_heads_decode joined with transl = dist K^-1 [loc; 1]
 *   (utils/camera.py:30-48, smpl_layer.py:117-123).  The decode is recomputed from readout in fp64 and that evaluation
 *   is differentiated (quaternion branch by the argmax of R00, R11, R22, trace; the w < 0 flip; the series of the
 *   scale for |angle| <= 1e-3); every output is rounded to fp32 once.  Cotangents (any may be NULL): g_rotmat,
 *   g_rotvec (the caller's own plus what the body backward sends to the 53 rotations), g_shape, g_expression,
 *   g_dist [P], g_dist_postprocessed [P], g_transl [P][3] (g_transl_total above), g_loc [P][2], g_offset_direct [P][2].
 *   Written: g_readout [P][318 + nb + 13] (cam[1:3] exactly 0; the clamp passes the gradient for 0 <= d <= 50) and
 *   g_offset [P][2].  An exact identity 6D is an ordinary input; a degenerate 6D is NaN as in the forward.
 * Validated before any launch: a NULL descriptor or required pointer, P < 0, 2D cotangents without K, a short
 * workspace, center_joint >= NJ -> MHMR_ERR_BAD_ARG; nb outside [0, 64], ldr < 318 + nb + 13, P > 65535 (placement)
 * -> MHMR_ERR_BAD_SHAPE; P == 0 launches nothing and returns 0.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int P, nb, ldr, patch, nearness;
    float fn;
    const float *readout, *offset, *K;
    const int *det_b, *det_y, *det_x;
    float *loc, *rotmat, *rotvec, *shape, *expression, *dist_postprocessed, *dist;
} mhmr_heads_decode_desc;

typedef struct {
    int P, V, NJ, center_joint;
    const float *verts_u, *joints_u, *transl, *K;
    const int* det_b;
    const float *g_v3d, *g_j3d, *g_v2d, *g_j2d, *g_transl;
    float *gx_v, *gx_j, *g_transl_total;
    void* workspace;
    long long workspace_bytes;
} mhmr_heads_place_desc;

typedef struct {
    int P, nb, ldr, patch, nearness;
    double fn;                /* the normalising focal length in full precision (the forward's float is its rounding) */
    const float *readout, *offset, *K;
    const int *det_b, *det_y, *det_x;
    const float *g_rotmat, *g_rotvec, *g_shape, *g_expression, *g_dist, *g_dist_postprocessed, *g_transl, *g_loc, *g_offset_direct;
    float *g_readout, *g_offset;
} mhmr_heads_decode_backward_desc;

int mhmr_heads_decode(const mhmr_heads_decode_desc* d, void* stream);
/* bytes of the per-tile fp64 sums of the placement backward: 24 per (person, tile of 1024 points); negative = MHMR_ERR_BAD_ARG */
long long mhmr_heads_place_workspace_bytes(int V, int NJ, int P);
int mhmr_heads_place_backward(const mhmr_heads_place_desc* d, void* stream);
int mhmr_heads_decode_backward(const mhmr_heads_decode_backward_desc* d, void* stream);

/* Sparse vertex regressor: out [M][R][3] = A . (in [M][Vin][3] - center [M][3]) for A in CSR form (rowptr [R + 1],
 * col, val); center NULL = none.  Each row is summed in the order of its entries (the loaders sort them by column) in
 * fp64 and rounded once: deterministic.  A row without entries gives zeros; an entry whose column is outside
 * [0, Vin) is skipped. */
int mhmr_sparse_regress(const int* rowptr, const int* col, const float* val, int R, int Vin, const float* in, const float* center,
                        int M, float* out, void* stream);

/* Detection targets of train.py:136-158 for n humans listed in (image, human) order: joints [n][NJ][3], K [n][3][3],
 * img [n] (image of each human, 0 <= img < B), the grid is Gp x Gp cells of `patch` pixels:
 *   loc [n][2] = projection of joint `center_joint`;  pk_idx [n][2] = clamp(floor(loc / patch), 0, Gp - 1) as (x, y);
 *   offset = (loc - (pk_idx + 0.5) patch) / patch;
 *   dist_pp [n] = (nearness ? log(z_pelvis + 1e-10) : z_pelvis) * fn / K[0][0]  (utils/camera.py:62-84);
 *   scores [B][Gp][Gp] indexed [image][y][x]: 1 in every claimed cell;  visible [n]: of several humans in one cell the
 *   first of the list stays visible (atomicMin of the list index per cell, then a compare: the result does not depend on
 *   execution order).  ws_owner: B Gp Gp ints.  scores and ws_owner are (re)initialised by the call. */
int mhmr_gt_targets(const float* joints, int NJ, int center_joint, const float* K, const int* img, int n, int B, int Gp, int patch,
                    float fn, int nearness, float* loc, int* pk_idx, float* offset, float* dist_pp, float* scores, int* visible,
                    int* ws_owner, void* stream);

/* utils/camera.py:14-27 perspective_projection: pts [n][N][3], K [n][3][3] -> out [n][N][2] = (K (x / x_z))[:2]. */
int mhmr_project_points(const float* pts, const float* K, int n, int N, float* out, void* stream);

/* roma.rotvec_to_rotmat (train.py:165): rotvec [n][3] -> rotmat [n][3][3], axis = v / max(|v|, 1e-6). */
int mhmr_rotvec_to_rotmat(const float* rotvec, int n, float* rotmat, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Mesh overlay (reference demo.py:128-158 overlay_human_meshes -> utils/render.py:175-315 render_meshes, which
 * draws with pyrender / OpenGL): P meshes sharing one face array [F][3], person p drawn into image
 * image_index[p], blended over uint8 RGB images [B][H][W][3].  One sample per pixel.  The render is defined by
 * multi_hmr_amd/render.py (the contract) and restated in numpy by tests/render_oracle.py:
 *   camera X = R x + t (OpenCV: X right, Y down, Z forward), u = fx X / Z + cx, v = fy Y / Z + cy, pixel (r, c)
 *   sampled at (c + 0.5, r + 0.5); faces with a vertex at Z < znear are dropped; back faces
 *   (dot((b-a) x (c-a), a) >= 0) culled if cull_back; coverage: edge functions > 0, or == 0 on a top-left edge;
 *   the winner of a pixel is the smallest key (float_bits(Z) << 32) | (p F + f), Z perspective-correct, kept
 *   only if znear <= (float)Z <= zfar (the fp32 depth of the key against the fp32 fields below); glTF
 *   metallic-roughness shading with one directional light along the view axis plus ambient; the reference's 3x3
 *   mask smoothing; the fp32 alpha blend, every operation rounded.
 * Geometry (transform, projection, edge functions, depth) is fp64; shading and the blend are fp32.
 * verts: person p's vertex v at verts[p * vstride + 3 v + axis] (vstride >= 3 V: the v3d block is read in place).
 * adj_off [V + 1] / adj: for every vertex the (3 face + corner) entries of its incident faces, ascending
 * (smooth normals only; may be NULL when smooth == 0).  Rt [B][3][4] = [R | t] or NULL (identity, zero).
 * key_out [B][H][W] (~0 where nothing is drawn) and rgb_out [B][H][W][3] (the shaded colour before the blend,
 * 0 where nothing is drawn) are optional.  img_out may equal img_in.  P F < 2^32 - 1, B <= 65535,
 * MHMR_ERR_BAD_SHAPE otherwise; the workspace holds the camera-space vertices and normals, the key buffer and a
 * list of the faces whose bounding box is large.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int B, H, W;
    int P, V, F;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* adj_off;
    const int* adj;
    const int* image_index;
    const float* K;
    const float* Rt;
    const float* colors;
    float alpha, intensity, ambient, metallic, roughness, znear, zfar;
    int smooth, cull_back;
    const unsigned char* img_in;
    unsigned char* img_out;
    void* workspace;
    long long workspace_bytes;
    unsigned long long* key_out;
    unsigned char* rgb_out;
} mhmr_render_desc;

long long mhmr_render_workspace_bytes(const mhmr_render_desc* d);
int mhmr_render_meshes(const mhmr_render_desc* d, void* stream);

/* Multi-view form: every image b is drawn from nviews >= 1 cameras, view (b, v) with K[b] and its own extrinsics
 * view_Rt[b][v] = [R | t] ([B][nviews][3][4], NULL = identity in every view); mesh p is drawn into every view of
 * image image_index[p], and every view of image b is blended over img_in[b].  img_out [B][nviews][H][W][3],
 * key_out [B][nviews][H][W] and rgb_out [B][nviews][H][W][3] hold B nviews images; img_out may equal img_in only
 * when nviews == 1.  Each view follows the contract above with its own [R | t] and is bit-identical to a
 * mhmr_render_meshes call with d->Rt = that view's extrinsics; mhmr_render_meshes is the nviews == 1 case of the
 * same kernels.  The vertex normals are computed once per mesh, whatever nviews is.  d->Rt must be NULL
 * (MHMR_ERR_BAD_ARG otherwise); nviews >= 1, B nviews <= 65535 and nviews P F < 2^32 - 1, MHMR_ERR_BAD_SHAPE
 * otherwise.  The workspace holds per view the camera-space vertices and normals, the key buffers and the
 * large-face list, plus the fp64 world normals when nviews > 1. */
long long mhmr_render_views_workspace_bytes(const mhmr_render_desc* d, int nviews);
int mhmr_render_views(const mhmr_render_desc* d, int nviews, const float* view_Rt, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Per-pixel maps and per-person statistics from the rasteriser's keys (csrc/render_maps.hip; multi_hmr_amd/maps.py
 * is the Python surface, tests/maps_oracle.py the numpy restatement).  keys [B][NV][H][W] is key_out of
 * mhmr_render_meshes (NV = 1) or mhmr_render_views of the same scene: (float_bits(Z) << 32) | (p F + f), ~0 where
 * nothing is drawn.  P, F and image_index [P] are that call's; face_label [F] (uint8, each < L, L <= 255) is
 * optional.  A pixel whose key is ~0, or names a person >= P, or a person p with image_index[p] != its image b, is
 * background.  Every output is optional (NULL = skipped):
 *   person [B][NV][H][W] int32   low32(key) / F                          background -1
 *   face   [B][NV][H][W] int32   low32(key) % F                          background -1
 *   depth  [B][NV][H][W] fp32    the key's high word, reinterpreted      background 0 (as pyrender's depth map)
 *   label  [B][NV][H][W] uint8   face_label[face]                        background 255
 * and per person p and view v of image image_index[p]:
 *   visible_px [P][NV] int32     pixels of view (image_index[p], v) that p wins            0 when none
 *   bbox [P][NV][4] int32        x0, y0, x1, y1 of those pixels, inclusive                 W, H, -1, -1 when none
 *   zmin [P][NV] fp32            their smallest depth                                      +inf when none
 *   label_px [P][NV][L] int32    their count per label (labels >= L are not counted)       0
 * A person whose image_index is outside [0, B) wins no pixel in the renderer and has the empty statistics here.
 * The statistics are initialised inside the call and reduced with integer add / min / max only (zmin through the
 * unsigned bit pattern: Z >= znear > 0), pre-reduced per wave and per workgroup: the same bits on every call.
 * label and label_px need face_label (MHMR_ERR_BAD_ARG), label_px needs L >= 1.  B NV <= 65535 and P F < 2^32 - 1 as
 * in the renderer, L in [0, 255], P >= 0, F >= 1 when P > 0: MHMR_ERR_BAD_SHAPE otherwise.  P == 0 is legal (every
 * pixel is background).  No workspace, no allocation, no synchronisation; the launches go to `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int B, NV, H, W;
    int P, F;
    const unsigned long long* keys;
    const int* image_index;
    const unsigned char* face_label;
    int L;
    int* person;
    int* face;
    float* depth;
    unsigned char* label;
    int* visible_px;
    int* bbox;
    float* zmin;
    int* label_px;
} mhmr_render_maps_desc;

int mhmr_render_maps(const mhmr_render_maps_desc* d, void* stream);

/* Visibility of 3D points against the keys: points [P][N][3] fp32, person p's point n at points[p * pstride + 3 n + axis]
 * (pstride >= 3 N: the v3d and j3d blocks are read in place), out [P][NV][N] uint8:
 *   0 occluded, 1 visible, 2 projects outside the image, 3 Z < znear or a non-finite coordinate.
 * In fp64, every step rounded on its own: X = R x + t with the renderer's expression ((R0 x0 + R1 x1) + R2 x2) + t and
 * view convention (K[b], view_Rt[b][v], b = image_index[p]; NULL = identity); a non-finite x or X, or Z < znear,
 * gives 3; u = fx X / Z + cx, v = fy Y / Z + cy; the pixel is (r, c) = (floor(v), floor(u)), outside [0, H) x [0, W)
 * gives 2; a pixel whose key is ~0 gives 1; otherwise 1 iff Z <= (double)fp32_depth_of_key + (double)tau, else 0.
 * tau (metres, >= 0) is the caller's margin: a few centimetres for vertices, about a limb's radius for joints.  A
 * person whose image_index is outside [0, B) gets 2 everywhere.  znear <= 0 or tau < 0 (or NaN): MHMR_ERR_BAD_ARG;
 * shapes as above, P N < 2^31: MHMR_ERR_BAD_SHAPE.  P N == 0 launches nothing. */
typedef struct {
    int B, NV, H, W;
    int P, N;
    const float* points;
    long long pstride;
    const int* image_index;
    const float* K;
    const float* view_Rt;
    const unsigned long long* keys;
    float znear, tau;
    unsigned char* out;
} mhmr_point_visibility_desc;

int mhmr_render_point_visibility(const mhmr_point_visibility_desc* d, void* stream);

/* Amodal area: amodal_px [P][nviews] int32 = the number of pixels person p would win in view v of image
 * image_index[p] if they were alone in it: by definition the count of drawn keys of a mhmr_render_views call that
 * holds only that person, so face drop, cull (d->cull_back), coverage and the znear / zfar test of the fp32 depth are
 * the renderer's (the same code, csrc/render_shared.h).  0 for a person whose image_index is outside [0, B).  Read
 * from d: B, H, W, P, V, F, verts, vstride, faces, image_index, K, znear, zfar, cull_back, workspace,
 * workspace_bytes; the image inputs and outputs, colours, normals and shading fields are not read; d->Rt must be
 * NULL (MHMR_ERR_BAD_ARG), view_Rt [B][nviews][3][4] or NULL as in mhmr_render_views.  Persons are taken in passes of
 * as many as the workspace holds (a coverage bit per pixel and view, a list of the faces with a large pixel box):
 * mhmr_render_amodal_workspace_bytes(d, nviews, n) is what passes of n persons need, linear in n and independent of
 * P; a workspace smaller than the answer for n = 1 is MHMR_ERR_BAD_SHAPE.  The result does not depend on the pass
 * size.  P == 0 launches nothing. */
long long mhmr_render_amodal_workspace_bytes(const mhmr_render_desc* d, int nviews, int persons_per_pass);
int mhmr_render_amodal(const mhmr_render_desc* d, int nviews, const float* view_Rt, int* amodal_px, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Differentiable read-out of the keys: depth, barycentrics and interpolated vertex attributes per pixel, and their
 * gradient with respect to the vertices and the attribute table (csrc/raster_grad.hip; multi_hmr_amd/raster.py is
 * the Python surface, tests/raster_oracle.py the numpy / torch restatement).  This comment is the contract.
 * Inputs.  The scene as to mhmr_render_views: verts (person p's vertex n at verts[p * vstride + 3 n + axis],
 * vstride >= 3 V), faces [F][3], image_index [P], K [B][3][3], view_Rt [B][NV][3][4] or NULL (identity), H, W, znear,
 * cull_back; keys [B][NV][H][W] as in mhmr_render_maps; optional per-vertex attributes attr, fp32: person p's vertex
 * n has channel c at attr[p * astride + C n + c], C in [0, 16], astride = 0 (one table serves every person) or
 * >= C V.
 * Forward, per pixel (b, v, r, c), in fp64 and in the operation order of csrc/render_shared.h, every step rounded
 * on its own:  the pixel is background exactly as in mhmr_render_maps (key ~0, person >= P, image_index[p] != b).
 * Otherwise (p, f) = low32(key) / F, % F; X_i = view_position(R, T, x_i) of the face's corners; tri_setup and
 * tri_cover at the centre (c + 0.5, r + 0.5) give e_i; w_i = (e_i / area) / Z_i, Z = 1 / ((w0 + w1) + w2),
 * b_i = w_i Z (the perspective-correct barycentrics).  The pixel is STALE when the setup fails, the pixel lies
 * outside the face's pixel box or its centre is not covered, or a face index is outside [0, V) (never
 * dereferenced): keys that belong to other vertices.  A stale pixel is background and contributes to no gradient;
 * it is never an error and never a division by zero.
 * Outputs, each optional (NULL = skipped), 0 at background pixels:
 *   depth    [B][NV][H][W]     fp32  (float)Z: for keys rendered from these vertices, the key's high word bit for bit
 *   bary     [B][NV][H][W][3]  fp32  (float)b_i
 *   out_attr [B][NV][H][W][C]  fp32  (float)((b0 a0c + b1 a1c) + b2 a2c)
 * Backward (mhmr_raster_backward): the derivative of exactly that map with the keys held fixed and K, Rt constant.
 * Cotangents g_depth, g_bary, g_out_attr in the outputs' layouts, each optional (NULL = zero); at background and
 * stale pixels they are NOT READ (a NaN there changes no bit).  Per owned pixel, with g^_i = g_bary_i +
 * sum_c g_out_attr_c a_ic and M = [X0 X1 X2]:  g_w_i = Z (g^_i - sum_j g^_j b_j) - g_depth Z^2,  M^T h = g_w,
 * g_X_i = -w_i h,  g_x_i = R^T g_X_i,  g_a_ic = b_i g_out_attr_c.
 * Results g_verts [P][V][3] and g_attr [P][V][C] (optional), fp32, contiguous, every element written: zero for a
 * vertex no owned pixel touches and for a person whose image_index is outside [0, B).  The sums over pixels,
 * incident faces (ascending, as adj) and views (ascending) are fp64 in an order fixed by the shapes and the keys
 * (not by scheduling) and rounded to fp32 once: two calls give the same bits.  No floating-point atomics.
 * adj_off [V + 1], adj: vertex -> incident 3 f + corner entries, ascending (as mhmr_render_desc); read by the
 * backward only.  The backward takes persons in passes of as many as the workspace holds (9 + 3 C doubles per face
 * and view, and a list of the faces with a large pixel box): mhmr_raster_workspace_bytes(d, n) is what passes of n
 * persons need, linear in n and independent of P; the result does not depend on the pass size.
 * Refused before any launch: B NV > 65535, P F or NV P F >= 2^32 - 1, P V >= 2^31, C outside [0, 16], astride
 * between 1 and C V - 1, a workspace too small for one person per pass (MHMR_ERR_BAD_SHAPE); znear <= 0, a missing
 * pointer, attr present without an attribute output (forward: out_attr; backward: g_out_attr or g_attr) or absent
 * with one (MHMR_ERR_BAD_ARG).  P == 0 is legal: the forward launches only the background fill, the backward
 * nothing.  No allocation, no synchronisation; the launches go to `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int B, NV, H, W;
    int P, V, F, C;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* adj_off;
    const int* adj;
    const int* image_index;
    const float* K;
    const float* view_Rt;
    const unsigned long long* keys;
    const float* attr;
    long long astride;
    float znear;
    int cull_back;
    float* depth;
    float* bary;
    float* out_attr;
    const float* g_depth;
    const float* g_bary;
    const float* g_out_attr;
    float* g_verts;
    float* g_attr;
    void* workspace;
    long long workspace_bytes;
} mhmr_raster_desc;

long long mhmr_raster_workspace_bytes(const mhmr_raster_desc* d, int persons_per_pass);
int mhmr_raster_interpolate(const mhmr_raster_desc* d, void* stream);
int mhmr_raster_backward(const mhmr_raster_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exact squared Euclidean distance and nearest-pixel maps (csrc/silhouette.hip; multi_hmr_amd/silhouette.py
 * distance_transform is the Python surface, tests/silhouette_oracle.py the numpy restatement).  This comment is the
 * contract.  src [N][H][W] uint8, nonzero = "on"; R = max_dist, an integer cap in pixels, 0 = no cap.  With
 * d2(y, x) = the minimum over the on-pixels (y', x') of the map of (x - x')^2 + (y - y')^2:
 *   dist2   [N][H][W] int32   d2, and R R + 1 where d2 > R R (R > 0)
 *   nearest [N][H][W] int32   y' W + x' of the minimiser; when several on-pixels tie, the smallest y' W + x' among
 *                             ALL of them
 * Where the map has no on-pixel, or d2 > R R with R > 0: dist2 = 0x7fffffff (R == 0) or R R + 1 (R > 0), nearest =
 * -1.  Each output is optional (NULL = skipped; with both NULL nothing is launched).  Integer arithmetic only: the
 * result does not depend on the algorithm and is the same on every call.  The workspace holds one int32 per pixel
 * (each pixel's nearest on-row of its own column): mhmr_distance_transform_workspace_bytes(d).
 * 1 <= H, W <= 4096, N >= 0, N max(H, 16) < 2^31, a workspace below that answer: MHMR_ERR_BAD_SHAPE; R < 0 or
 * R > 46340 (R R + 1 must fit), src or workspace NULL with N > 0: MHMR_ERR_BAD_ARG; both before any launch.
 * N == 0 launches nothing.  No allocation, no synchronisation; the launches go to `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int N, H, W;
    const unsigned char* src;
    int max_dist;
    int* dist2;
    int* nearest;
    void* workspace;
    long long workspace_bytes;
} mhmr_distance_transform_desc;

long long mhmr_distance_transform_workspace_bytes(const mhmr_distance_transform_desc* d);
int mhmr_distance_transform(const mhmr_distance_transform_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Silhouette term: how far each person's mesh is from lying inside, and from covering, that person's segmentation
 * mask, and the gradient of both with respect to the vertices (csrc/silhouette.hip; multi_hmr_amd/silhouette.py
 * silhouette_loss is the Python surface, tests/silhouette_oracle.py the numpy / torch restatement).  This comment is
 * the contract.
 * Inputs.  The scene as to mhmr_raster_desc with one view: B, H, W (<= 4096), P, V, F, verts (person p's vertex n at
 * verts[p * vstride + 3 n + axis], vstride >= 3 V), faces [F][3], image_index [P], K [B][3][3], Rt [B][3][4] or
 * NULL (identity), znear, zfar, cull_back.  mask [P][H][W] uint8 (nonzero = the person's segment); allowed
 * [P][H][W] uint8 (where the person may project without cost; NULL = mask); sigma > 0 (pixels); robust
 * (MHMR_FIT_L2: rho(s) = s, MHMR_FIT_GMOF: rho(s) = s / (1 + s)); R = max_dist >= 1 (pixels, integer).
 * Projection of vertex n of person p, in fp64, every step rounded on its own (the rule of
 * mhmr_point_visibility_desc): X = ((R0 x0 + R1 x1) + R2 x2) + t; a non-finite x or X, or Z < znear, makes the
 * vertex unprojectable; u = fx X / Z + cx, v = fy Y / Z + cy; its pixel is (floor(v), floor(u)), and a vertex whose
 * pixel is outside [0, H) x [0, W) is outside.  Unprojectable and outside vertices, and every vertex of a person
 * whose image_index is outside [0, B), contribute to neither term and get gradient 0.  Below, "vertices" are the
 * others.
 * Term 0, "outside".  phi_p = sqrt((double)dist2) of mhmr_distance_transform of allowed[p] with cap R, sampled
 * bilinearly on the pixel-centre grid at (su, sv) = (u - 0.5, v - 0.5) clamped to [0, W - 1] x [0, H - 1]:
 * x0 = floor(su), x1 = min(x0 + 1, W - 1), tx = su - x0 (rows likewise), phi = (1 - ty) ((1 - tx) phi00 + tx phi10)
 * + ty ((1 - tx) phi01 + tx phi11).  terms[p][0] = sum over the vertices of rho(phi^2 / sigma^2); counts[p][0] = how
 * many of them have phi > 0.  Its gradient is the exact derivative of that piecewise-smooth expression through the
 * projection, K and Rt constant (g_x = R^T g_X); along an axis whose coordinate is clamped (u - 0.5 not inside
 * (0, W - 1)) the derivative is 0.  Occluded vertices are included: occlusion is the caller's business, through
 * `allowed`.
 * Term 1, "uncovered".  cover_p = the pixels mhmr_render_amodal counts for person p (same face drop, cull, coverage
 * and znear / zfar rule).  The splat map S_p: pixel (floor(v), floor(u)) is owned by the SMALLEST index among the
 * vertices of p that fall into it.  U_p = the pixels x with mask[p](x) != 0, x not in cover_p and
 * d2(x, S_p) <= R R; v(x) = the owner of nearest_{S_p}(x) (mhmr_distance_transform's tie rule).  With pi(n) = (u, v)
 * of vertex n and c(x) = (x + 0.5, y + 0.5):  terms[p][1] = sum over x in U_p of |pi(v(x)) - c(x)|^2 / sigma^2,
 * counts[p][1] = |U_p|.  It is evaluated through per-vertex integer moments over the pixels assigned to the vertex
 * (moments [P][V][4] int64: n, sum (2x + 1), sum (2y + 1), sum ((2x + 1)^2 + (2y + 1)^2), integer atomics):
 * value = (n |pi|^2 - pi . (Sx, Sy) + Sq / 4) / sigma^2 and d / d pi = (2 n pi - (Sx, Sy)) / sigma^2, formed after
 * shifting the moments, exactly and in integers, to the centre of the vertex's own pixel so that nothing cancels.
 * THE ASSIGNMENT v(x), THE SET U_p AND THE COVER ARE HELD FIXED (as the correspondences of ICP): the gradient is that
 * of the value with them constant, and nothing flows through coverage, K or Rt.
 * Outputs, each optional (NULL = skipped): terms [P][2] fp64; counts [P][2] int32; g_verts [2][P][V][3] fp32, the
 * gradient of each term on its own, every element written; and for tests and tools splat [P][H][W] int32 (the
 * owner, -1 where no vertex falls) and moments [P][V][4] int64.  The per-person sums are fp64 in an order the
 * shapes fix (thread t of 256 adds its vertices t, t + 256, ... ascending, then a binary tree over the threads);
 * the gradients are rounded to fp32 once.  No floating-point atomics: two calls give the same bits.
 * Persons are taken in passes of as many as the workspace holds (per person four int32 maps -- the transform of
 * `allowed`, the splat map, its nearest map, the column scratch -- the coverage bits, the large-face list and the
 * moments): mhmr_silhouette_workspace_bytes(d, n) is what passes of n persons need, linear in n and independent of
 * P; the result does not depend on the pass size.
 * Refused before any launch: B outside [1, 65535], H or W outside [1, 4096], P < 0, V or F < 1 or vstride < 3 V
 * with P > 0, P F >= 2^32 - 1, P V >= 2^31, a workspace below the answer for n = 1 (MHMR_ERR_BAD_SHAPE); znear <= 0,
 * zfar <= znear, sigma not positive and finite, robust not MHMR_FIT_*, R < 1 or > 46340, a missing pointer
 * (MHMR_ERR_BAD_ARG).  P == 0 launches nothing.  No allocation, no synchronisation; the launches go to `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int B, H, W;
    int P, V, F;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* image_index;
    const float* K;
    const float* Rt;
    float znear, zfar;
    int cull_back;
    const unsigned char* mask;
    const unsigned char* allowed;
    float sigma;
    int robust;
    int max_dist;
    double* terms;
    int* counts;
    float* g_verts;
    int* splat;
    long long* moments;
    void* workspace;
    long long workspace_bytes;
} mhmr_silhouette_desc;

long long mhmr_silhouette_workspace_bytes(const mhmr_silhouette_desc* d, int persons_per_pass);
int mhmr_silhouette(const mhmr_silhouette_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Contacts between persons: signed distances from every vertex to the other persons' surfaces, penetration and
 * contact counts (csrc/contact.hip; multi_hmr_amd/contact.py is the Python surface, tests/contact_oracle.py the
 * numpy restatement).  This comment is the contract.
 * Inputs.  verts [P][V][3] fp32, person p's vertex n at verts[p * vstride + 3 n + axis], vstride >= 3 V (the
 * forward's v3d block is read in place, as mhmr_point_visibility_desc.pstride); image_index [P]; faces [F][3] int32,
 * shared by all persons; the margins max_dist >= 0 (finite) and 0 <= tau <= max_dist, in metres.  Both margins are
 * CONVENTIONS of the caller, not measurements: max_dist is how far the search looks, tau what counts as touching.
 * Validity and boxes.  A person is valid when every coordinate is finite.  aabb[p] = (min xyz, max xyz) in fp32
 * (comparisons only: exact).  An invalid person takes no part, neither as a nor as b, has the empty values below,
 * valid[p] = 0 and aabb[p] = (+inf x 3, -inf x 3).
 * Pairs.  The ordered pair (a, b) is evaluated iff a != b, both are valid, image_index[a] == image_index[b], and the
 * two boxes, EACH inflated by max_dist (lo - max_dist, hi + max_dist: one fp32 operation per bound), intersect:
 * lo_a' <= hi_b' and lo_b' <= hi_a' on every axis.  Inside an evaluated pair, vertex v of a is evaluated iff
 * lo_b' <= v <= hi_b' on every axis; every other vertex is "farther than max_dist" from b.  The cull is part of the
 * result (the corner regions of the inflated box are farther than max_dist and are dropped by the s <= max_dist rule
 * below; nothing nearer than max_dist is ever culled).
 * Faces.  A face whose fp32 normal (b - a) x (c - a), every difference and product rounded on its own
 * (n_x = fl(fl(u_y v_z) - fl(u_z v_y)) and cyclic), is the zero vector is skipped for the distance and for the
 * winding number; so is, on the device, a face with an index outside [0, V) (it is never dereferenced).
 * mhmr_contact cannot read device memory before a launch: mhmr_contact_check_faces(faces_host, F, V) is the host
 * check, MHMR_ERR_BAD_SHAPE for an index outside [0, V); the Python layer runs it once per face array.
 * Per evaluated (v, b), over b's non-skipped faces in ascending order:
 *   closest point: per face by the region method (vertex / edge / interior; Ericson, Real-Time Collision Detection
 *     5.1.5) as c_f = a + s (b - a) + t (c - a); the face's squared distance is |(v - a) - s (b - a) - t (c - a)|^2,
 *     formed from the closest point's offset, never as a difference of squared lengths (which cancels near the
 *     surface).  nearest face = the lowest face index attaining the smallest squared distance (the square root is
 *     monotone: it is the smallest distance), c = its c_f, d = sqrt of its squared distance.
 *   winding number: w = (1 / 4 pi) sum_f 2 atan2(A . (B x C), |A||B||C| + (A . B)|C| + (B . C)|A| + (C . A)|B|), A, B,
 *     C the face's corners minus v.  The kernel splits the faces over eight waves (wave k takes the k-th eighth of
 *     every tile of 512 faces, ascending) and adds the eight partial sums in the order ((w0 + w1) + w2) + ... + w7.
 *   v is INSIDE b iff lo_b <= v <= hi_b on every axis (the UN-inflated box) and |w| > 0.5.  The absolute value makes
 *     a mirrored (inward-oriented) mesh behave like the upright one; the box test costs nothing for a mesh without
 *     boundary edges (w = 0 outside its convex hull) and saves the sum for every vertex beside the box.
 *   signed distance: s = inside ? -d : d.
 * Outputs.  Every output is optional (NULL = skipped) and initialised inside the call:
 *   sdf [P][V] fp32               the smallest s over the evaluated b, if <= max_dist            else +inf
 *   nearest_person [P][V] int32   that b (b ascending, strict <: the lowest b on a tie)           else -1
 *   nearest_face [P][V] int32     its nearest face                                               else -1
 *   closest [P][V][3] fp32        its closest point c                                            else the vertex itself
 *   penetration_depth [P] fp32    max_v max(0, -sdf)                                             0
 *   inside_count [P] int32        vertices with sdf < 0                                          0
 *   contact_count [P] int32       vertices with |sdf| <= tau                                     0
 *   pair_distance [P][P] fp32     [a][b]: smallest s of a's evaluated vertices against b,
 *                                 kept only when <= max_dist (NOT symmetric: vertex-to-surface
 *                                 from a's side)                                                 else +inf
 *   pair_inside [P][P] int32      [a][b]: vertices of a inside b                                 0
 *   aabb [P][6] fp32, valid [P] uint8   as above
 * Determinism.  Per-vertex results come from one fixed-order loop; per-person and per-pair results are reduced with
 * integer add / min / max only (floats through an integer whose order is theirs): two calls give the same bits.
 * Call.  Everything goes to `stream`; no host synchronisation, no allocation, no host-built pair list (a workgroup
 * decides from the device-side boxes whether it has work).  workspace: mhmr_contact_workspace_bytes(P, V) bytes (the
 * boxes and, per person, the ascending list of the vertices that lie in some partner's inflated box: about 36 + 4 V
 * bytes per person), contents irrelevant on entry.  P == 0 launches nothing; P > 0 with no evaluated pair
 * is legal.  NULL descriptor, a needed pointer NULL, a negative, NaN or infinite margin or tau > max_dist:
 * MHMR_ERR_BAD_ARG.  P, V or F < 0, P V >= 2^31, P^2 >= 2^31, vstride < 3 V, a workspace too small:
 * MHMR_ERR_BAD_SHAPE.  All of it is checked before the first launch.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int P, V, F;
    const float* verts;
    long long vstride;
    const int* image_index;
    const int* faces;
    float max_dist, tau;
    void* workspace;
    long long workspace_bytes;
    float* sdf;
    int* nearest_person;
    int* nearest_face;
    float* closest;
    float* penetration_depth;
    int* inside_count;
    int* contact_count;
    float* pair_distance;
    int* pair_inside;
    float* aabb;
    unsigned char* valid;
} mhmr_contact_desc;

long long mhmr_contact_workspace_bytes(int P, int V);
int mhmr_contact_check_faces(const int* faces_host, int F, int V);
int mhmr_contact(const mhmr_contact_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Scene packing for the 3D export (reference utils/render.py:62-173 create_scene, demo.py:371-384): P meshes
 * sharing one face array, laid out as a glTF binary chunk holds them, in ONE launch (multi_hmr_amd/scene.py writes
 * the file; tests/scene_oracle.py restates this contract in numpy):
 *   out [P][2][V][3] fp32: per person the transformed positions, then the transformed unit normals, so the persons
 *     p0 .. p1 of one image are one contiguous byte range; bounds [P][2][3] fp32: per person the component-wise
 *     minimum, then maximum, of the positions just written (glTF requires them on a POSITION accessor).
 *   Position: X = R x + t in fp64, summed as ((R0 x0 + R1 x1) + R2 x2) + t, rounded once to fp32.
 *   Normal: the angle-weighted vertex normal of render contract item 6 (incident non-degenerate faces in ascending
 *     face order, corner angle x unit face normal, normalised, fp64; the sum order is the CSR's, no atomics),
 *     rotated by R, rounded once to fp32.  A vertex with no non-degenerate incident face gets (0, 0, 1), not
 *     rotated.
 *   Bounds: the exact min / max of the fp32 positions (order-independent, hence deterministic).
 * transform [3][4] fp32 = [R | t], R taken to be a rotation (not checked); NULL = diag(-1, -1, 1), t = 0: what
 * create_scene applies to the whole scene (OpenCV camera axes -> glTF's y up, z towards the viewer).  It is a
 * rotation, so the faces keep their winding and one index buffer serves every person.
 * verts, vstride, faces, adj_off, adj as in mhmr_render_desc (faces with an index outside [0, V) contribute
 * nothing); F == 0: no face is read and every normal is (0, 0, 1).
 * V <= 0, F < 0, P < 0, vstride < 3 V with P > 1, out == NULL with P > 0 -> MHMR_ERR_BAD_SHAPE; another null
 * pointer that would be read or written -> MHMR_ERR_BAD_ARG; both before any launch.  P == 0 launches nothing and
 * returns 0.  No allocation, no workspace, no synchronisation; the launch goes to `stream`; re-entrant.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int P, V, F;
    const float* verts;
    long long vstride;
    const int* faces;
    const int* adj_off;
    const int* adj;
    const float* transform;
    float* out;
    float* bounds;
} mhmr_scene_desc;

int mhmr_scene_pack(const mhmr_scene_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Training loss (reference loss.py:8-40 _neg_loss, 47-115 Loss.forward) and its gradient with respect to the
 * predictions, DESIGN.md section 17.  Eleven values in the reference's dict_loss order:
 *   0 total, 1 bce, 2 offset, 3 rotmat, 4 shape, 5 dist, 6 transl, 7 j3d, 8 v3d, 9 j2d, 10 v2d.
 * Tensors (fp32, contiguous; `*_hat` = prediction): scores [B][G][G] (the target counts as positive where >= 1),
 * offset [P][2], rotmat [P][nrot] (53 * 9), shape_hat [P][nb_hat] / shape [P][nb_gt] (the first min(nb_hat, nb_gt)
 * columns are compared), dist [P] (dist_postprocessed), transl [P][3], pelvis [P][3] (transl_pelvis), j3d [P][J][3],
 * v3d [P][V][3], j2d [P][J][2], v2d [P][V][2].  P == 0 is legal (the person pointers are not read: the person
 * terms are 0, bce is computed).
 * Arithmetic: every element |a - b| is formed in fp32 with the reference's operations in its order, no FMA --
 * (y - pelvis) - (y_hat - pelvis_hat) for j3d / v3d, y_hat - y elsewhere; a 2D point counts when both target
 * coordinates are > 0 and < img_size; every sum is fp64, combined in a fixed order (lane, wave, workgroup, then a
 * launch that walks the workgroup partials by index: no floating-point atomics, bit-reproducible); the focal term
 * is fp64 throughout from the fp32 score (eps 1e-7; num_pos == 0 -> -neg_loss, decided on the device); the
 * normalisers (P, P J, P V, the in-frame counts), nan_to_num (a NaN / +-inf term becomes 0), the alpha weights
 * and the epoch gate (use_2d) are applied in fp64 and each value is rounded to fp32 once.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    const float *scores_hat, *offset_hat, *rotmat_hat, *shape_hat, *dist_hat, *transl_hat, *pelvis_hat, *j3d_hat, *v3d_hat, *j2d_hat,
        *v2d_hat;
    const float *scores, *offset, *rotmat, *shape, *dist, *transl, *pelvis, *j3d, *v3d, *j2d, *v2d;
    int B, G, P, V, J, nrot, nb_hat, nb_gt;
    float img_size;
    int use_2d;               /* epoch >= start_2d_epoch (loss.py:96) */
    double alpha[10];         /* alpha_bce, _offset, _rotmat, _shape, _dist, _transl, _j3d, _v3d, _j2d, _v2d (loss.py:121-136) */
} mhmr_loss_desc;

/* gradient outputs of mhmr_loss_backward, shaped like the predictions; NULL = not wanted */
typedef struct {
    float *scores, *offset, *rotmat, *shape, *dist, *transl, *pelvis, *j3d, *v3d, *j2d, *v2d;
} mhmr_loss_grads;

/* the device block `out` of mhmr_loss_forward: 32 four-byte words --
 *   [0..10] fp32 the eleven values;  [12] int num_pos, [13] int in-frame j2d points, [14] int in-frame v2d points;
 *   [16 + i] int: 1 if term i was finite before nan_to_num, 0 if it was replaced by 0 ([16] = 1). */
#define MHMR_LOSS_OUT_BYTES 128

/* bytes of the fp64 workgroup partials mhmr_loss_forward needs (the same for every shape: the grid is fixed) */
long long mhmr_loss_workspace_bytes(void);
/* loss.py:49-113.  Two launches on `stream`; ws is written before it is read (no clearing needed).  Validated
 * before any launch: d, ws, out NULL or ws_bytes too small, a NULL scores pointer, a NULL person pointer with P > 0
 * -> MHMR_ERR_BAD_ARG; B, G, V, J, nrot, nb_hat, nb_gt < 1, P < 0, or a tensor of 2^31 or more elements ->
 * MHMR_ERR_BAD_ARG. */
int mhmr_loss_forward(const mhmr_loss_desc* d, void* ws, long long ws_bytes, void* out, void* stream);
/* d total / d prediction = grad_total (device scalar, the upstream gradient of `total`) * alpha_term * sign(element)
 * / normaliser, for every non-NULL pointer of g; `out` is the block the forward of the SAME d left (normalisers,
 * flags).  Signs are recomputed in fp32 as in the forward (sign(0) = 0); out-of-frame 2D points and shape columns
 * >= min(nb_hat, nb_gt) get 0; the 2D gradients are 0 when use_2d == 0; pelvis[p][a] = -(sum_j j3d[p][j][a] +
 * sum_v v3d[p][v][a]) from integer sign sums, scaled once in fp64 (exact, order-free); the score gradient is the
 * analytic derivative of the focal term in fp64, rounded once.  A term whose finite flag is 0 has ALL its gradients
 * 0 (torch: 0 behind an inf, NaN behind a NaN).  The gradient of the targets is never produced.  Validation as
 * for the forward (plus out, grad_total, g NULL), before any launch. */
int mhmr_loss_backward(const mhmr_loss_desc* d, const void* out, const float* grad_total, const mhmr_loss_grads* g, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fused Adam step over a table of segments that also rewrites the packed copy of every element it updates
 * (csrc/optim.hip).  One segment = one fp32 parameter tensor (contiguous, n elements) with
 * its two moments, its gradient, and the place of its packed copy: element i of the parameter is element
 * (i / cols) * pitch + i % cols of `packed` (cols == pitch: a plain copy; pitch > cols: a padded pitch whose
 * padding is never written; `packed` may point into the middle of a larger buffer: a row offset).
 *   packed_kind  MHMR_ADAM_PACK_NONE: nothing is written;  _F32: packed = p;  _F16 / _BF16: packed = the 16-bit
 *                round-to-nearest-even cast of p;
 *   addend       non-NULL (fp32, n elements, read only): packed = p + addend[i]      (dec_b = bias + init_*)
 *   param2 ...   non-NULL (all four of param2, exp_avg2, exp_avg_sq2, grad2): a second parameter of n elements
 *                updated by the same thread from its own gradient and moments; packed = p + p2
 *                (tok_b = bias + pos_embedding[0, 0]).  Not together with addend.
 *   grad         NULL: the segment is skipped -- parameter, moments and packed copy keep their bits.
 *   step_size, bc2_sqrt (and *2 for param2): lr / (1 - beta1^t) and sqrt(1 - beta2^t) of THIS tensor's step
 *                count t >= 1 after the increment, computed by the caller in double and rounded once.
 *   chunk0       first chunk of the segment: chunk0 of segment 0 is 0, of segment s + 1 it is chunk0[s] +
 *                ceil(n[s] / MHMR_ADAM_CHUNK).  One workgroup per chunk; skipped segments keep their chunks.
 * Per element, in fp32, in the order of torch's single-tensor Adam (fma: one rounding; every other operation rounded on its own):
 *   g' = g * coef (coef = 1 without clipping);  m = fma(w1, g' - m, m);  v = v * beta2;  v = fma(w2 * g', g', v);
 *   p = p + (-step_size * m) / (sqrt(v) / bc2_sqrt + eps),     w1 = (float)(1 - beta1), w2 = (float)(1 - beta2), the
 * differences taken in double.  No weight decay, no amsgrad, no maximize.
 * Clipping (max_norm > 0): a first launch writes one fp64 partial sum of g^2 per chunk (0 for skipped segments;
 * g and g2 both count), a second adds the partials in chunk order and leaves norm = (float)sqrt(sum) in
 * norm_out[0]; coef = min(1, max_norm / (norm + 1e-6)).  `partials` holds at least the total chunk count.  No
 * atomics: two calls give the same bits.  max_norm <= 0: one launch, partials / norm_out are not touched.
 * `segs_host` and `segs_dev` are the SAME nsegs entries in host and in device memory: the host copy is validated
 * before the first launch, the kernels read the device copy (which the caller has enqueued on `stream` before
 * the call).  MHMR_ERR_BAD_ARG: nsegs < 0, a NULL table, a NULL param, NULL moments beside a gradient, an incomplete
 * second parameter, addend together with a second parameter, a packed_kind outside the four values or without a
 * `packed` pointer, a wrong chunk0, packed ranges of two segments that overlap, betas outside [0, 1), eps < 0, a
 * step_size or bc2_sqrt that is not finite and positive, clipping without partials / norm_out or with
 * partials_count below the chunk count.  MHMR_ERR_BAD_SHAPE: n < 1, cols < 1, pitch < cols, n % cols != 0, more
 * than 2^31 - 1 chunks.  nsegs == 0 launches nothing.  16-byte loads and stores where every pointer of the segment
 * and the pitch allow them, element by element otherwise: the same bits.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_ADAM_CHUNK 2048
#define MHMR_ADAM_PACK_NONE 0
#define MHMR_ADAM_PACK_F32 1
#define MHMR_ADAM_PACK_F16 2
#define MHMR_ADAM_PACK_BF16 3
typedef struct {
    float* param;
    float* exp_avg;
    float* exp_avg_sq;
    const float* grad;
    float* param2;
    float* exp_avg2;
    float* exp_avg_sq2;
    const float* grad2;
    void* packed;
    const float* addend;
    long long n;
    int cols, pitch, packed_kind, chunk0;
    float step_size, bc2_sqrt, step_size2, bc2_sqrt2;
} mhmr_adam_segment;
int mhmr_adam_step(const mhmr_adam_segment* segs_host, const mhmr_adam_segment* segs_dev, int nsegs, double beta1, double beta2, double eps,
                   double max_norm, double* partials, long long partials_count, float* norm_out, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device re-pack of the DERIVED encoder operands (csrc/encoder_pack.hip): with mhmr_adam_step
 * over the whole model it replaces the reference's optimizer.step() (train.py:304) plus the host re-pack after it.
 * A table of jobs; all MHMR_PACK_ROW jobs first, then the MHMR_PACK_POS jobs; one launch per kind.
 *
 * MHMR_PACK_ROW -- what vit.pack_block derives from one fp32 linear w [N, K] (K % 4 == 0), one wave per row n:
 *   Wf[n][k]  = w[n][k] * ln_w[k] (ONE fp32 multiply) with ln_w / ln_b non-NULL (the LayerNorm fold), else w[n][k]
 *   w16       non-NULL: row n at w16 + n * pitch16 (elements) = round16(Wf[n]), dtype MHMR_ADAM_PACK_F16 / _BF16,
 *             round to nearest even, f16 subnormals kept; columns K .. pitch16 are never written
 *   lo        lo_form MHMR_PACK_LO_PAIR: rows lo_row0 .. lo_row0 + lo_rows - 1 of w also get row n - lo_row0 of lo,
 *             [hi | lo] = [round16(Wf) | round16(Wf - (float)hi)], the sections lo_section (>= K) elements apart, the
 *             rows lo_pitch apart; MHMR_PACK_LO_TRIPLE: [hi | lo | hi] (the f16x3 operand); _NONE: lo must be NULL
 *   bias_out  non-NULL (needs bias and the fold): bias_out[n] = (float)((double)bias[n] + sum_k (double)w[n][k] * ln_b[k])
 *   colsum    non-NULL: colsum[n] = (float)(sum_k hi[n][k] (+ lo[n][k] on the rows of a _PAIR low half)), in fp64
 *   Both sums: lane l of the wave adds the elements k with (k / 4) % 64 == l in ascending k (hi before lo), then the 64
 *   lanes are added as a butterfly (l with l ^ 32, ^ 16, ..., ^ 1): the order depends on K alone.
 *   row0      cumulative N of the row jobs before this one (0 for the first).
 * MHMR_PACK_POS -- packing.interpolate_pos_embed + the class row of vit.pack_embeddings: pos_embed fp32 [1 + M*M][C],
 *   cls_token [C] -> pos [1 + G*G][C], cls_pos0 [C] = cls_token + pos[0] (fp32 add).  tap_w fp64 [G][4] / tap_i int
 *   [G][4]: the separable bicubic weights and clipped source indices of packing._cubic_taps (device memory, made on
 *   the host once per pack).  pos[1 + y*G + x][c] = (float) sum_b tap_w[x][b] * (sum_a tap_w[y][a] *
 *   grid[tap_i[y][a]][tap_i[x][b]][c]), fp64, both sums in tap order, rounded once.  G == M copies the table (the
 *   taps may be NULL).  row0: cumulative 1 + G*G of the position jobs before this one.
 * Every element has one writer; no atomics: two calls give the same bits.  `jobs_host` / `jobs_dev` as the two
 * tables of mhmr_adam_step.  Validated on the host copy before any launch -- MHMR_ERR_BAD_ARG: njobs < 0, a NULL
 * table, an unknown kind or a row job behind a position job, a NULL w, a dtype that is not _F16 / _BF16, ln_w
 * without ln_b (or the reverse), bias_out without bias or without the fold, lo_form set with lo NULL (or the
 * reverse), a row job that writes nothing, a wrong row0, NULL position tensors, NULL taps with G != M, two
 * targets of the table that overlap.  MHMR_ERR_BAD_SHAPE: N, K, M, G, C < 1, K % 4 != 0, pitch16 < K, lo rows
 * outside [0, N), lo_section < K, a lo_pitch that does not hold the sections, 2^31 or more rows.  njobs == 0
 * launches nothing.  No device allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_PACK_ROW 0
#define MHMR_PACK_POS 1
#define MHMR_PACK_LO_NONE 0
#define MHMR_PACK_LO_PAIR 1
#define MHMR_PACK_LO_TRIPLE 2
typedef struct {
    const float* w;
    const float* ln_w;
    const float* ln_b;
    const float* bias;
    void* w16;
    void* lo;
    float* bias_out;
    float* colsum;
    const float* pos_embed;
    const float* cls_token;
    const double* tap_w;
    const int* tap_i;
    float* pos;
    float* cls_pos0;
    int kind, dtype, row0, N, K, pitch16, lo_form, lo_row0, lo_rows, lo_section, lo_pitch, M, G, C;
} mhmr_pack_job;
int mhmr_vit_repack(const mhmr_pack_job* jobs_host, const mhmr_pack_job* jobs_dev, int njobs, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fit persons to 2D keypoints (csrc/fit.hip): Adam on the read-out row r = [pose6d 318 | betas nb |
 * cam 3 | expr 10] and the offset o [2] of every person, from the anchors r0, o0 (the network's prediction), against
 * targets kp [NJ][2] in pixels with weights c [NJ] >= 0 (c = 0: the joint is not given), NJ = J + E + L of the body model.
 * The objective is separable per person -- no sum crosses persons:
 *   (loc, rotvec, shape, expression, dist) = mhmr_heads_decode(r, o, det, K)                          unchanged, fp32
 *   u_j    = joints of mhmr_body_forward(pose55(rotvec), [shape | expression], transl = NULL, K = NULL)
 *   transl = dist K_b^-1 [loc; 1],  x_j = (u_j - u_center) + transl,  j2d_j = project(x_j, K_b),  b = det_b[p]
 *   s_j    = |j2d_j - kp_j|^2 / sigma^2,   rho(s) = s (MHMR_FIT_L2)  or  s / (1 + s) (MHMR_FIT_GMOF)
 *   E_p    = sum_j c_j rho(s_j) + lambda_pose |r_pose6d - r0_pose6d|^2 + lambda_shape |r_betas - r0_betas|^2
 *            + lambda_depth (r_cam0 - r0_cam0)^2 + lambda_expr |r_expr - r0_expr|^2 + lambda_loc |o - o0|^2
 * Elements are fp32; the sum over the joints and each prior sum are fp64 in index order, each rounded once; E_p = the data term
 * plus lambda * sum of the five priors in that order, in fp64, rounded once.  A joint with c_j = 0 (or a NaN weight) is a SELECT:
 * exact zeros in the value and the gradient, whatever its target holds (NaN, Inf).  The cotangent
 * g_j2d_j = 2 c_j rho'(s_j) (j2d_j - kp_j) / sigma^2 (rho' = 1, or 1 / (1 + s)^2) goes through mhmr_heads_place_backward,
 * mhmr_body_backward (g_vertices = NULL) and mhmr_heads_decode_backward; the prior terms 2 lambda (r - r0) are added in fp32 and
 * the result is multiplied by the 0/1 column mask [318 + nb + 13 + 2] (read-out columns, then the two offset columns).
 * cam[1:3] keep their exact-zero gradient (no prior reads them); a masked column's parameter and moments are never written.
 * Per step: the Adam element of mhmr_adam_step (the same function, csrc/adam_element.h; no clipping) in place on readout, offset,
 * exp_avg and exp_avg_sq [P][318 + nb + 13 + 2], with lr / (1 - beta1^t) and sqrt(1 - beta2^t) of t = step0 + 1, step0 + 2, ...
 * taken in double on the host and rounded once: a second call with step0 = the steps done and the same moments continues the
 * first, bit for bit.
 * The entry enqueues, `steps` times: decode -> stage -> body forward -> objective -> placement backward -> body backward ->
 * stage back -> decode backward -> update, then one more evaluation without the update for objective[steps] and grad (skipped
 * when both are NULL).  steps = 0 is "value and gradient only".  objective [steps + 1][P] (nullable): E_p at every iterate,
 * the last included.  grad [P][318 + nb + 13 + 2] (nullable): the masked gradient at the last iterate.
 * The body model may be any (c, bc) pair whose chain is SMPL-X's (J = 55, nc = nb + 10): the full model, or the gathered model
 * of BodyModel.keypoint_model(), which holds the <= E + 3 L vertices the output joints read.  readout0 has readout's pitch ldr.
 * No atomics, no allocation, no synchronisation; every output element is written; two calls give the same bits; person p of a
 * batch gets the bits it gets alone.  Validated before the first launch: a NULL descriptor, model or required pointer, P < 0,
 * steps < 0, step0 < 0, sigma, fn or (steps > 0) lr not finite and positive, a negative or non-finite lambda, robust outside the
 * two kinds, betas outside [0, 1), eps < 0, center_joint >= NJ, patch <= 0, bc->n != E + 3 L, a short workspace ->
 * MHMR_ERR_BAD_ARG; J != 55, nb != nc - 10, nb outside [0, 64], ldr < 318 + nb + 13, P > 65535, NJ > 8192, the shape limits of
 * mhmr_body_forward -> MHMR_ERR_BAD_SHAPE; P == 0 launches nothing and returns 0.
 * mhmr_fit_keypoints_workspace_bytes: bytes for (c, P), monotone in P; negative = the error code.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_FIT_L2 0
#define MHMR_FIT_GMOF 1
typedef struct {
    const mhmr_body_consts* c;
    const mhmr_body_bwd_consts* bc;
    int P, nb, ldr, patch, nearness, center_joint;   /* center_joint < 0: no recentring (x = u + transl)                  */
    double fn;                                       /* normalising focal length (the decode reads its float rounding)    */
    float *readout, *offset;                         /* in/out [P][ldr], [P][2]                                           */
    const float *readout0, *offset0;                 /* anchors [P][ldr], [P][2]                                          */
    const int *det_b, *det_y, *det_x;                /* [P]                                                               */
    const float* K;                                  /* [B][3][3]                                                         */
    const float *keypoints, *confidence;             /* [P][NJ][2], [P][NJ]                                               */
    float sigma;
    int robust;                                      /* MHMR_FIT_*                                                        */
    float lambda_pose, lambda_shape, lambda_depth, lambda_expr, lambda_loc;
    const float* mask;                               /* [318 + nb + 13 + 2] of 0 / 1                                      */
    int steps, step0;
    double lr, beta1, beta2, eps;
    float *exp_avg, *exp_avg_sq;                     /* in/out [P][318 + nb + 13 + 2] (may be NULL when steps == 0)       */
    float* objective;                                /* [steps + 1][P] or NULL                                            */
    float* grad;                                     /* [P][318 + nb + 13 + 2] or NULL                                    */
    void* workspace;
    long long workspace_bytes;
} mhmr_fit_desc;
long long mhmr_fit_keypoints_workspace_bytes(const mhmr_body_consts* c, int P);
int mhmr_fit_keypoints(const mhmr_fit_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Backward of one ViT block: the derivative of the fp32 function
 *     x -> x + ls1 * proj(MHSA(norm1(x))),  then  x -> x + ls2 * fc2(gelu(fc1(norm2(x))))
 * (attention scale head_dim^-0.5, erf GELU, LayerNorm eps 1e-6) with the fp32 master weights in torch layout,
 * evaluated at the block input x_in that the inference forward produced.  The backward recomputes the block's
 * activations from x_in in fp32 (the tape) and reads none of the forward's 16-bit workspaces: the 16-bit roundings of
 * the forward are straight-through.  Sums across rows are fp64 or fp32 MFMA chains whose shape the sizes alone fix,
 * there are no floating-point atomics, every element of every output is written, two calls give the same bits; no
 * entry allocates or synchronises, and all validation happens before the first launch.
 *
 *   mhmr_attention_f32_tape:      qkv [B*Tp, 3C] fp32 = (Q | K | V), un-scaled, head h at columns h*64 (the input of
 *       mhmr_attention_f32) -> out32 [B*Tp, C] fp32 and lse [B, H, Tp] = max + log2(sum) of a query's logits in the
 *       exp2 domain (logit = q.k * MHMR_ATTN_QSCALE).  Keys at rows >= T are masked; rows >= T of out32 and lse are zeros.
 *   mhmr_attention_f32_backward:  qkv, out32, lse as above, dO [B*Tp, lddo] (head h at columns h*64) -> dqkv [B*Tp, 3C]
 *       with respect to the un-scaled Q, K and V.  Every product on v_mfma_f32_16x16x4_f32.  Two passes, no sum crosses a
 *       workgroup: a query-tile pass over the keys (per query r = 1 / sum exp2(s - lse) and D = sum P dP with
 *       P = exp2(s - lse) r, then dQ) and a key-tile pass over the queries (dK, dV).  D is summed from the P and dP that
 *       form dS = P (dP - D) -- closer to fp64 than dO . O where dP - D cancels -- so out32 must be given but is not read.
 *       Keys and queries at rows >= T are masked: whatever finite numbers qkv, dO and out32 hold there moves no bit of a
 *       real row, and rows >= T of dqkv are exact zeros.  workspace: D | r, [B, H, Tp] each.
 *   mhmr_vit_block_backward:      recomputes the tape, then the backward.  Only the T real rows of an image contribute
 *       to the parameter gradients (rows >= T of g_out are not read as cotangents); rows >= T of g_in are zeros.
 * Shapes: B, T >= 1, Tp % 64 == 0, Tp >= T, C == 64 H (C <= 2048 for the block), lddo >= C and lddo % 4 == 0, H and B at
 * most 65535, B * Tp at most 16 * 65535 for the block, MHMR_ERR_BAD_SHAPE otherwise (negative counts: MHMR_ERR_BAD_ARG).  A NULL pointer,
 * a pointer of the attention entries that is not 16-byte aligned, or a short workspace: MHMR_ERR_BAD_ARG.
 * ---------------------------------------------------------------------------------------------------------- */
int mhmr_attention_f32_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* stream);
long long mhmr_attention_f32_backward_workspace_bytes(int B, int Tp, int H);
int mhmr_attention_f32_backward(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv,
                                int B, int T, int Tp, int C, int H, void* workspace, long long workspace_bytes, void* stream);

typedef struct {
    int B, T, Tp, C, H;
    /* the fp32 master tensors of blocks.i, torch layout: qkv_w [3C, C], proj_w [C, C], fc1_w [4C, C], fc2_w [C, 4C] */
    const float* ln1_w;
    const float* ln1_b;
    const float* qkv_w;
    const float* qkv_b;
    const float* proj_w;
    const float* proj_b;
    const float* ls1;
    const float* ln2_w;
    const float* ln2_b;
    const float* fc1_w;
    const float* fc1_b;
    const float* fc2_w;
    const float* fc2_b;
    const float* ls2;
    const float* x_in;  /* [B*Tp, C] the residual stream entering the block               */
    const float* g_out; /* [B*Tp, C] cotangent of the block's output                       */
    float* g_in;        /* [B*Tp, C] cotangent of x_in (may not alias g_out)               */
    /* one gradient buffer per master tensor, of its shape */
    float* g_ln1_w;
    float* g_ln1_b;
    float* g_qkv_w;
    float* g_qkv_b;
    float* g_proj_w;
    float* g_proj_b;
    float* g_ls1;
    float* g_ln2_w;
    float* g_ln2_b;
    float* g_fc1_w;
    float* g_fc1_b;
    float* g_fc2_w;
    float* g_fc2_b;
    float* g_ls2;
    void* workspace;
    long long workspace_bytes; /* >= mhmr_vit_block_backward_workspace_bytes(B, Tp, C); with linear_precision 1: ..._bytes_p(B, Tp, C, 1) */
    int linear_precision;      /* MHMR_BWD_F32 (0, a zeroed field): the exact fp32 linears; MHMR_BWD_BF16 (1): bf16 operands (below) */
} mhmr_vit_block_backward_desc;
long long mhmr_vit_block_backward_workspace_bytes(int B, int Tp, int C);
long long mhmr_vit_block_backward_workspace_bytes_p(int B, int Tp, int C, int precision);
int mhmr_vit_block_backward(const mhmr_vit_block_backward_desc* d, void* stream);

/* The backbone tail: the backward of the final LayerNorm -- patch rows only: g_feat [B*N, C] is the cotangent of feat32, the class
 * row and the padding rows of the stream cotangent are zeros -- then mhmr_vit_block_backward for the last n blocks, last block first,
 * each at its tapped input.  The gradient stops at the input of block L - n (g_stream); with n == L that is the token embedding's
 * output, which mhmr_vit_embed_backward (below) differentiates.  blocks: HOST array of n descriptors in block order (L - n first) of which the fourteen master tensors and the fourteen
 * gradient buffers are read; their shapes, x_in, g_out, g_in and workspace fields are ignored.  tap: [n][B*Tp, C], slot i = the stream
 * entering block L - n + i (mhmr_vit_desc.tap with tap_first = L - n); resid: the stream the final norm read.
 * n >= 1, N == T - 1, and the shape rules of the block (MHMR_ERR_BAD_SHAPE); NULL pointers, a short workspace: MHMR_ERR_BAD_ARG. */
typedef struct {
    int B, N, T, Tp, C, H, n;
    const float* norm_w;
    const float* norm_b;
    const mhmr_vit_block_backward_desc* blocks;
    const float* tap;
    const float* resid;
    const float* g_feat;
    float* g_norm_w;
    float* g_norm_b;
    float* g_stream; /* [B*Tp, C] cotangent of the stream entering block L - n; rows >= T are zeros */
    void* workspace;
    long long workspace_bytes; /* >= mhmr_vit_tail_backward_workspace_bytes(B, Tp, C); with linear_precision 1: ..._bytes_p(B, Tp, C, 1) */
    int linear_precision;      /* MHMR_BWD_*: handed to every block (the blocks' own field is ignored, like their shapes) */
} mhmr_vit_tail_backward_desc;
long long mhmr_vit_tail_backward_workspace_bytes(int B, int Tp, int C);
long long mhmr_vit_tail_backward_workspace_bytes_p(int B, int Tp, int C, int precision);
int mhmr_vit_tail_backward(const mhmr_vit_tail_backward_desc* d, void* stream);

/* ----------------------------------------------------------------------------------------------------------
 * Mixed-precision backbone training: dense linears with bf16 operands and fp32 accumulation on
 * v_mfma_f32_16x16x32_bf16 -- what torch autocast makes of an nn.Linear, in both directions.  r() is round-to-nearest-even
 * fp32 -> bf16 (torch.Tensor.bfloat16()); every tensor here is fp32, row-major, W [N, K] in torch layout:
 *   mhmr_linear_bf16:                  Y[m][n]  = sum_k r(X[m][k]) r(W[n][k]) + bias[n]           (bias may be NULL)
 *   mhmr_linear_bf16_backward_input:   dX[m][k] = sum_n r(dY[m][n]) r(W[n][k]) (+ dR[m][k])       (dR may be NULL; added in fp32)
 *   mhmr_linear_bf16_backward_weight:  dW[n][k] = sum_m r(dY[m][n]) r(X[m][k]);  db[n] = sum_m dY[m][n] in fp64 from the
 *                                      UNROUNDED dY, two fixed stages.  dW or db may be NULL, not both.
 * There is no activation argument: a GELU derivative is applied in fp32 in front of these products (the block does so).
 * A product of two bf16 numbers is exact in fp32; the fp32 accumulation runs in chains of 256 summed indices that are added
 * into a second accumulator, and the weight side's sum over M is cut into slices of 4096 rows whose partial products (in the
 * workspace) are added in slice order in fp64 and rounded once.  The shape of every sum is fixed by (M, N, K) alone: no
 * floating-point atomics, two calls give the same bits, rows of exact zeros appended to dY change no bit of dW.  Every
 * element of every output is written; no allocation, no synchronisation; everything is validated before the first launch.
 * Shapes: M, N, K multiples of 64 and at least 64, M <= 16 * 65535; every leading dimension at least its row length and a
 * multiple of 4 (MHMR_ERR_BAD_SHAPE otherwise).  MHMR_ERR_BAD_ARG: a negative count, a NULL pointer that would be read or
 * written, a pointer that is not 16-byte aligned (db excepted), a workspace below mhmr_linear_bf16_workspace_bytes(M, N, K)
 * -- one size for all three products.
 * In mhmr_vit_block_backward / mhmr_vit_tail_backward, linear_precision = MHMR_BWD_BF16 sends the four linears of the tape and
 * their eight backward products through these kernels (dh <- dh * gelu'(z1) by an fp32 kernel in front of fc1's two).  The
 * LayerNorms, the attention tape and backward, LayerScale, GELU, the row mask and every fp64 column sum are the fp32 mode's,
 * and so are its invariants: rows >= T of g_in / g_stream are exact zeros, finite values in rows >= T of x_in / g_out move no
 * bit, an image's g_in does not depend on the other images.  Any other value of linear_precision: MHMR_ERR_BAD_ARG.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_BWD_F32 0
#define MHMR_BWD_BF16 1
long long mhmr_linear_bf16_workspace_bytes(int M, int N, int K);
int mhmr_linear_bf16(const float* X, int ldx, const float* W, int ldw, const float* bias, float* Y, int ldy, int M, int N, int K,
                     void* workspace, long long workspace_bytes, void* stream);
int mhmr_linear_bf16_backward_input(const float* dY, int lddy, const float* W, int ldw, const float* dR, int lddr, float* dX,
                                    int lddx, int M, int N, int K, void* workspace, long long workspace_bytes, void* stream);
int mhmr_linear_bf16_backward_weight(const float* dY, int lddy, const float* X, int ldx, float* dW, int lddw, float* db, int M,
                                     int N, int K, void* workspace, long long workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------------------
 * Attention with bf16 operands for mixed-precision training: the tape and the backward of the
 * self-attention on v_mfma_f32_16x16x32_bf16.  Every tensor is fp32 in the layouts of mhmr_attention_f32_tape / _backward;
 * r() is round-to-nearest-even fp32 -> bf16.  Per (image, head), over the T real rows:
 *     S_ij  = MHMR_ATTN_QSCALE * sum_d r(Q_i[d]) r(K_j[d])     fp32 accumulation, S is NOT rounded
 *     lse_i = log2 sum_j exp2(S_ij)                            P_ij = exp2(S_ij - lse_i): normalised by the final lse
 *     O_i   = sum_j r(P_ij) r(V_j)                             -> out32 (fp32, not rounded)
 *     D_i   = sum_d dO_i[d] O_i[d]                             fp32, the UNROUNDED dO and the tape's out32, fixed order
 *     dP_ij = sum_d r(dO_i[d]) r(V_j[d])                       dS_ij = P_ij (dP_ij - D_i)
 *     dV_j  = sum_i r(P_ij) r(dO_i)     dQ_i = 0.125 sum_j r(dS_ij) r(K_j)     dK_j = 0.125 sum_i r(dS_ij) r(Q_i)
 * The rounded probability is the normalised one -- a function of the inputs, not of a tile order: the tape sweeps the keys
 * twice (S and the log-sum, then S again, r(exp2(S - lse)) and the product with V), and the backward recomputes S with the
 * same products and uses the tape's lse.  Against torch autocast, which rounds q k^T to 16 bits in front of the softmax, S
 * stays fp32: a deviation on the accurate side.  D is the row sum of dO . O, so out32 IS read by this backward.
 *   mhmr_attention_bf16_workspace_bytes: one size for both entries (the bf16 copies of qkv and dO, as they lie and
 *       transposed, and D [B, H, Tp]).
 *   mhmr_attention_bf16_tape:     qkv [B*Tp, 3C] -> out32 [B*Tp, C], lse [B, H, Tp].
 *   mhmr_attention_bf16_backward: qkv, out32, lse, dO [B*Tp, lddo] -> dqkv [B*Tp, 3C].  Converts on its own: it does not need
 *       the tape to have run on the same workspace.
 * Invariants (those of the fp32 pair): keys and queries at rows >= T are masked; whatever finite values (finite as bf16) qkv,
 * dO and out32 hold at rows >= T moves no bit of a real row; rows >= T of out32, lse and dqkv are exact zeros; every element
 * of every output is written; no floating-point atomics; the order of every fp32 accumulation (ascending tiles of 64 keys or
 * queries) is fixed by (T, Tp) alone, so two calls give the same bits and an image does not depend on the others; no
 * allocation, no synchronisation, all validation before the first launch.
 * Shapes and errors: those of the fp32 pair, and B * Tp at most 64 * 65535; a workspace below
 * mhmr_attention_bf16_workspace_bytes(B, Tp, C, H) or not 16-byte aligned: MHMR_ERR_BAD_ARG.
 *
 * In the block and the tail the switch is an argument of appended entries (the descriptors are closed):
 * mhmr_vit_block_backward(d, s) == mhmr_vit_block_backward_a(d, MHMR_ATTN_F32, s), likewise the tail, which hands its value to
 * every block; with MHMR_ATTN_BF16 the attention tape and backward of the block are the two entries above and the workspace must
 * hold ..._workspace_bytes_pa(B, Tp, C, linear_precision, MHMR_ATTN_BF16); ..._pa(.., p, MHMR_ATTN_F32) == ..._p(.., p).  The two
 * switches are independent.  Any other attention_precision: MHMR_ERR_BAD_ARG.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_ATTN_F32 0
#define MHMR_ATTN_BF16 1
long long mhmr_attention_bf16_workspace_bytes(int B, int Tp, int C, int H);
int mhmr_attention_bf16_tape(const float* qkv, float* out32, float* lse, int B, int T, int Tp, int C, int H, void* workspace,
                             long long workspace_bytes, void* stream);
int mhmr_attention_bf16_backward(const float* qkv, const float* out32, const float* lse, const float* dO, int lddo, float* dqkv,
                                 int B, int T, int Tp, int C, int H, void* workspace, long long workspace_bytes, void* stream);
long long mhmr_vit_block_backward_workspace_bytes_pa(int B, int Tp, int C, int linear_precision, int attention_precision);
long long mhmr_vit_tail_backward_workspace_bytes_pa(int B, int Tp, int C, int linear_precision, int attention_precision);
int mhmr_vit_block_backward_a(const mhmr_vit_block_backward_desc* d, int attention_precision, void* stream);
int mhmr_vit_tail_backward_a(const mhmr_vit_tail_backward_desc* d, int attention_precision, void* stream);

/* The token embedding: the derivative of the fp32 function
 *     tokens[b] = [ patchify(x[b]) W^T + bias + pos_G[1:],  cls + pos_G[0] ],   pos_G = interpolate(pos_embed)
 * at the fp32 master parameters and the fp32 image, against g_stream, the cotangent of the stream entering block 0 (what
 * mhmr_vit_tail_backward writes with n == L).  The forward's 16-bit roundings of the patches and of W are straight-through.
 * S = 14 G; N = G*G patch rows of image b at rows b*Tp + n (n = gy*G + gx), its class row at b*Tp + N; the position table has
 * 1 + M*M rows.  Only the patch rows enter g_patch_w, g_patch_b and g_pos[1:], only the class rows enter g_cls and g_pos[0]
 * (the same number); rows > N of an image are never read.  interp: DEVICE [G, M] fp64, the bicubic resampling matrix
 * (pos_G[1 + y*G + x] = sum_a sum_q interp[y][a] interp[x][q] pos[1 + a*M + q]; the identity for G == M).
 * g_patch_w is an fp32 MFMA chain (v_mfma_f32_16x16x4_f32) over the B*N patch rows in index order, blocked 256 / 4096; every
 * other sum is fp64 in a fixed index order, rounded once.  No atomics, every element of every output is written, two calls
 * give the same bits; no allocation, no synchronisation, all validation before the first launch.
 * MHMR_ERR_BAD_ARG: a NULL pointer, a negative count, a workspace that is short or not 16-byte aligned.  MHMR_ERR_BAD_SHAPE:
 * S != 14 G, Tp % 64, Tp < G*G + 1, C % 64, C > 2048, B == 0, G == 0, M < 1, or the launch limits (G <= 1024, M <= 4096,
 * B * Tp <= 16 * 65535). */
typedef struct {
    int B, S, G, M, Tp, C;
    const float* x;         /* [B, 3, S, S] fp32, the forward's input                                  */
    const float* g_stream;  /* [B*Tp, C] cotangent of the stream entering block 0                      */
    const double* interp;   /* [G, M] the bicubic resampling matrix                                    */
    float* g_patch_w;       /* [C, 588], k = c*196 + py*14 + px (torch's conv weight, flattened)       */
    float* g_patch_b;       /* [C]                                                                     */
    float* g_cls;           /* [C]                                                                     */
    float* g_pos;           /* [1 + M*M, C]                                                            */
    void* workspace;
    long long workspace_bytes; /* >= mhmr_vit_embed_backward_workspace_bytes(B, G, M, C) */
} mhmr_vit_embed_backward_desc;
long long mhmr_vit_embed_backward_workspace_bytes(int B, int G, int M, int C);
int mhmr_vit_embed_backward(const mhmr_vit_embed_backward_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Track persons across video frames and smooth them (csrc/track.hip).  One call consumes the
 * person rows of F consecutive frames -- img_id [P] int64 non-decreasing with values in [0, F) (the order the forward
 * emits), idx_y, idx_x [P] int64, transl [P][3], readout [P][D] with D = 318 + nb + 13, offset [P][2] = (x, y) -- and
 * a table of `capacity` slots that lives in a caller-owned device buffer of mhmr_track_state_bytes(capacity, D)
 * bytes.  A zero-filled buffer is the empty tracker; the call reads and writes the table, and two calls of F1 and
 * F2 frames leave the table and the outputs that one call of F1 + F2 frames leaves, bit for bit.  Frames without
 * rows are ordinary; P == 0 lets F frames of time pass.  Everything is fp32, every operation rounded on its own
 * (no fused multiply-add); there are no atomics, no allocation and no synchronisation, every element of every
 * output is written by every call, the inputs are never written, two calls give the same bits.
 *
 * The table (all 4-byte aligned; D' = D: the read-out without cam[1:3], plus the two location columns):
 *   byte 0        long long next_id, then 56 reserved bytes (zero)
 *   byte 64       long long id [capacity]
 *   then          float pos [capacity][3] (metres), float vel [capacity][3] (metres per frame)
 *   then          int missed [capacity], int hits [capacity]         (hits > 0 <=> the slot is live)
 *   then          float x [capacity][D'], float dx [capacity][D']    (the filter state)
 * Freeing a slot sets hits = 0 and nothing else.
 *
 * Association, frame by frame in order.  For every (detection d = row within the frame, live slot t):
 *   k = missed_t + 1,  p = pos_t + vel_t * k,  e = transl_d - p,  c = (e_x^2 + e_y^2) + e_z^2;
 * the pair is gated in when c <= max_dist * max_dist (the float product).  The assignment is the one obtained by
 * sweeping the gated pairs in ascending order of (bits of c, d, t) and taking a pair when neither its detection nor
 * its slot is taken: GREEDY, not Hungarian, because it has an exact tie rule and an exact restatement on the CPU
 * (DESIGN.md section 33).  A NaN cost is never gated in.  Then, in this order:
 *   1. matched:      vel = (transl_d - pos) / k,  pos = transl_d,  missed = 0,  hits += 1
 *   2. unmatched live slots:  missed += 1; freed when missed > max_age
 *   3. unmatched detections, in row order: the lowest free slot (those freed in step 2 of this frame included) with
 *      id = next_id++, pos = transl_d, vel = 0, missed = 0, hits = 1
 *   4. no free slot: track_id = -1, hits = 0, the row's outputs are its inputs' bits, the table is not touched.
 *
 * Filter: a One-Euro filter per column of z = [readout[:318+nb+1] | readout[318+nb+3:] | u | v] of the matched row,
 * u = ((float)idx_x + 0.5) + offset_x and v likewise with y: the absolute location in patch cells, so a person who
 * crosses a cell border is continuous.  cam[1:3] are passed through.  With kf = (float)k, dt = kf / fps and
 * alpha(fc) = 1 / (1 + (1 / (2 pi fc)) / dt), 2 pi the float nearest to it:
 *   e = z - x,  d = e / dt,  dx <- dx + alpha(dcutoff) * (d - dx),  fc = mincutoff_g + beta_g * |dx|,  x <- x + alpha(fc) * e
 * with g the column's group: pose (the 318 6D numbers), shape (betas), depth (cam[0]), expr, loc (u, v).  A group
 * whose bit in `groups` is clear is a SELECT: its columns keep the input's bits and its state is never written.
 * readout_s is x scattered back into the row, offset_s = (u^ - ((float)idx_x + 0.5), v^ - ((float)idx_y + 0.5)).  A new
 * track (hits == 1) sets x = z, dx = 0 and its output rows are the input's bits, the offset included.
 *
 * track_id [P] int64, hits [P] int32 (after the update), status [1] int32 on the device: 0 = ok, 1 = img_id decreases
 * or leaves [0, F): then every id is -1, every hits 0, the rows pass through and the table is untouched.
 * Refused before the first launch: a NULL descriptor, state, workspace or status, a NULL input or output with P > 0,
 * F < 1, P < 0, capacity outside 1 ... 1024, max_age < 0, fps, dcutoff or the mincutoff of a selected group not finite
 * and positive, max_dist or a selected beta negative or not finite, bits of `groups` above the five, a short or
 * misaligned (8 bytes) state or workspace -> MHMR_ERR_BAD_ARG; P > 65535, nb not 10 or 11 -> MHMR_ERR_BAD_SHAPE.
 * mhmr_track_state_bytes(capacity, D), mhmr_track_workspace_bytes(F, capacity): monotone in each argument;
 * negative = the error code.  The workspace holds the journal [F][capacity] (row or none, k, new) that the
 * association kernel hands to the filter kernel.
 * ---------------------------------------------------------------------------------------------------------- */
#define MHMR_TRACK_POSE 1
#define MHMR_TRACK_SHAPE 2
#define MHMR_TRACK_DEPTH 4
#define MHMR_TRACK_EXPR 8
#define MHMR_TRACK_LOC 16
#define MHMR_TRACK_MAX_CAPACITY 1024
typedef struct {
    int F, P, nb, capacity;
    const long long *img_id, *idx_y, *idx_x;         /* [P]                                                               */
    const float *transl, *readout, *offset;          /* [P][3], [P][318 + nb + 13], [P][2]                                */
    float fps, max_dist;
    int max_age;
    int groups;                                      /* MHMR_TRACK_* bits of the filtered groups                          */
    float dcutoff;
    float mincutoff_pose, mincutoff_shape, mincutoff_depth, mincutoff_expr, mincutoff_loc;
    float beta_pose, beta_shape, beta_depth, beta_expr, beta_loc;
    void* state;
    long long state_bytes;
    void* workspace;
    long long workspace_bytes;
    long long* track_id;                             /* [P]                                                               */
    int* hits;                                       /* [P]                                                               */
    float *readout_s, *offset_s;                     /* [P][318 + nb + 13], [P][2]                                        */
    int* status;                                     /* [1]                                                               */
} mhmr_track_desc;
long long mhmr_track_state_bytes(int capacity, int D);
long long mhmr_track_workspace_bytes(int F, int capacity);
int mhmr_track_update(const mhmr_track_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Measurement: hipEvent brackets around every launch of one kernel family (0 = GEMM, 1 = attention, 2 = LBS
 * vertex kernel), recorded on the launch stream.  enable(kind >= 0) starts a fresh window, enable(-1) stops;
 * collect() synchronises the recorded events and returns launches, summed milliseconds and summed work
 * (FLOPs for 0/1, persons for 2).
 * ---------------------------------------------------------------------------------------------------------- */
int mhmr_prof_enable(int kind);
int mhmr_prof_collect(int* launches, double* total_ms, double* total_work);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* MHMR_H */
