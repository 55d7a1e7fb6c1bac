// The layout rule of the ViT forward, once: how many rows an image takes in the token-major workspaces, which optional workspaces a
// (pack, batch) needs, and which launch sequence mhmr_vit_forward then runs (vit_form).  Host only: plain C++ and integers, no HIP types --
// capi.hip includes it for mhmr_vit_forward / mhmr_vit_form_bits / mhmr_vit_plan, and it compiles with the host compiler alone.
//
// Two halves that must agree, one under the other:
//   * the CALLER's side (vit_row_map, vit_rows_per_image, vit_need_*): given a pack (C, T, fold, x3, lo8, cpad) and a batch B, how the
//     workspace is laid out.  mhmr_vit_plan answers it; multi_hmr_amd/vit.py asks.
//   * the FORWARD's side (vit_form): given a description (mhmr_vit_desc: B, C, N, Tp, which optional pointers are there), which form runs.
// INVARIANT that ties them (mhmr_vit_desc has no field for the caller's intent): where N % 256 == 0, vit_rows_per_image returns a
// multiple of 256 exactly when vit_row_map is false -- the row map's own padding is roundup(N + 1, 64) = N + 64, never a multiple of
// 256 -- so vit_form reads "Tp % 256 == 0 where N % 256 == 0" as the caller saying "all rows".
#ifndef MHMR_VIT_PLAN_H
#define MHMR_VIT_PLAN_H

#include <stdint.h>
#include "../../include/mhmr.h"

namespace {

// The environment switches of the forward and of its layout: A/B measurements and bisecting.  One MHMR_PLAN_* bit each (include/mhmr.h).
struct VitSwitches {
    bool rowmap;        // MHMR_ROWMAP=0: no token-row map and no 256x256 all-rows form: one GEMM over all B * Tp rows
    bool gemm128;       // MHMR_GEMM128 set (gemm.hip forces the 128x128 kernel everywhere): the same
    bool lnfold;        // MHMR_LNFOLD=0: LayerNorm as launches of its own
    bool lo8;           // MHMR_LO8: the forward reads "=0: the fp8 low-half ranges of a lo8 pack are not used" (on by default); a packing
                        // caller reads "=1: pack the fp8 rows" (opt-in, vit_lo8_eligible).  The bit is whichever question is being asked.
    bool anyorder;      // MHMR_ANYORDER=0 / 1 (default MHMR_ANYORDER_DEFAULT)
    bool qkv_merge;     // MHMR_QKV_MERGE=0: Q | K and V as two launches in a short batch too
    bool fc1_rowmap;    // MHMR_FC1_ROWMAP=0: fc1 of a short batch over all rows
    bool cls_stats;     // MHMR_CLS_STATS=0: row statistics as ln_stats launches
    bool tiny_allrows;  // MHMR_TINY_ALLROWS=0: tiny batches of a folded pack keep the token-row map
    bool lnfold_allrows;// MHMR_LNFOLD_ALLROWS=0: no LayerNorm fold where it needs the all-rows padding (N not a multiple of 256, ViT-S)
    bool vits_256;      // MHMR_VITS_256=1 (opt-in): ViT-S (C = 384) with folded LayerNorms on the 256x256 kernel (masked columns, cpad)
};

inline VitSwitches vit_switches_of_mask(unsigned m) {
    VitSwitches w{};
    w.rowmap = m & MHMR_PLAN_ROWMAP; w.gemm128 = m & MHMR_PLAN_GEMM128; w.lnfold = m & MHMR_PLAN_LNFOLD; w.lo8 = m & MHMR_PLAN_LO8;
    w.anyorder = m & MHMR_PLAN_ANYORDER; w.qkv_merge = m & MHMR_PLAN_QKV_MERGE; w.fc1_rowmap = m & MHMR_PLAN_FC1_ROWMAP;
    w.cls_stats = m & MHMR_PLAN_CLS_STATS; w.tiny_allrows = m & MHMR_PLAN_TINY_ALLROWS; w.lnfold_allrows = m & MHMR_PLAN_LNFOLD_ALLROWS;
    w.vits_256 = m & MHMR_PLAN_VITS_256;
    return w;
}

// ------------------------------------------------------------------------------------------------ the caller's side
// A pack's choices and a batch: everything the layout depends on.  T = N + 1 tokens per image; B = 0 asks the pack-time questions only.
struct VitPack { int C, N, T, B; bool fold, x3, lo8; int cpad; };

inline long long vit_roundup(long long v, long long m) { return (v + m - 1) / m * m; }

// The narrowest block linear (N = embed_dim) of the whole batch is at most HALF a round of 256x256 tiles on the chip (896^2: one image;
// 672^2: up to three).  Such a launch is latency, not throughput: exact tile rounds buy nothing, while the class-row kernels the token-row
// map needs are six more launches per block (~25 % of a batch-1 forward together with the row statistics).
// 128 = half of the 256 CUs the rule was measured on, and a FIXED property of the layout rule, not of the device it runs on: the rows per
// image of a pack must not depend on where it is planned.  (fc1map and qkv_merge, which only choose launches, use the device's CU count.)
inline bool vit_tiny_batch(const VitPack& p) {
    return p.C % 256 == 0 && (p.B * vit_roundup(p.T, 256) / 256) * (p.C / 256) <= 128;
}

// The five big GEMMs of a block run over the B * N patch rows only (the class rows through vit_cls.hip) when an image's patch rows are
// whole 256-row tiles of the 256x256 kernel -- except for tiny batches with folded LayerNorms, which run ALL rows (class and padding rows
// included, Tp a multiple of 256: the invariant above) through the big GEMMs and launch no class-row kernel at all.
inline bool vit_row_map(const VitPack& p, const VitSwitches& w) {
    return !p.x3 && w.rowmap && !w.gemm128 && p.C % 256 == 0 && (p.T - 1) % 256 == 0 &&
           p.B * vit_roundup(p.T, 64) * p.C * 4 < (1ll << 32) && !(p.fold && vit_tiny_batch(p) && w.tiny_allrows);
}

// Rows per image in the token-major workspaces (patch tokens, the class token, zero padding).  A multiple of 64 (the attention key tile,
// the V^T row granularity) when every linear of the encoder stays on the 256x256 kernel -- the GEMMs cover the patch rows only
// (vit_row_map), or embed_dim and B * Tp are multiples of 256; otherwise a multiple of 128, the row tile of the 128x128 kernel.
// 896^2: 4160 instead of 4224 rows per image.
inline int vit_rows_per_image(const VitPack& p, const VitSwitches& w) {
    if (p.x3) return (int)vit_roundup(p.T, p.C % 256 == 0 ? 256 : 128);     // all rows through every linear: whole tiles for every batch size
    const bool rm = vit_row_map(p, w);
    if (p.fold && (p.cpad || (p.T - 1) % 256 || (!rm && vit_tiny_batch(p) && w.rowmap && !w.gemm128)))
        return (int)vit_roundup(p.T, 256);   // folded LayerNorms without the row map: whole 256-row tiles of all rows, for every batch size
    const long long t64 = vit_roundup(p.T, 64), t128 = vit_roundup(p.T, 128);
    // the predicate of gemm256.hip mhmr_gemm256_eligible for the residual GEMMs over all B * Tp rows (32-bit residual offsets), and the
    // switch that forces the 128x128 kernel everywhere
    const bool all_rows_256 = p.C % 256 == 0 && (p.B * t64) % 256 == 0 && p.B * t64 * p.C * 4 < (1ll << 32) && !w.gemm128;
    return (int)((rm && !w.gemm128) || all_rows_256 ? t64 : t128);
}

// Row pitch of xn / att in elements: operand pairs under f16x3; with lo8 a row carries its bf8 copy behind its C values
inline int vit_pitch(const VitPack& p) { return p.x3 ? 2 * p.C : p.lo8 ? p.C + p.C / 2 : p.C; }

// The optional workspaces: pstats + rowstats (the LayerNorm fold), cls_pstats (block sums of the class rows, vit_cls.hip: under the row
// map), splitk + v16 (only the all-rows form of a tiny batch has launches short enough to be split: mhmr_splitk_plan says how many bytes)
inline bool vit_need_pstats(const VitPack& p) { return p.fold; }
inline bool vit_need_cls_pstats(const VitPack& p, const VitSwitches& w) { return p.fold && !p.x3 && vit_row_map(p, w); }
inline bool vit_may_splitk(const VitPack& p, const VitSwitches& w) {
    return p.fold && !p.x3 && !p.lo8 && vit_rows_per_image(p, w) % 256 == 0 && !vit_row_map(p, w) &&
           !w.gemm128;       // (split-k is a form of the 256x256 kernel: mhmr_splitk_plan refuses under that switch)
}

// Pack time.  fp8 low-half ranges need the 256x256 kernel's 128-deep fp8 k tiles in whole pairs: embed_dim a multiple of 256 (ViT-B / ViT-L)
inline bool vit_lo8_eligible(int C, const VitSwitches& w) { return C % 256 == 0 && w.lo8 && !w.gemm128; }

// The LayerNorm fold (gemm256.hip, GemmArgs::pstats / rowstats) needs every block linear on the 256x256 kernel: embed_dim a multiple of
// 256 (ViT-B / ViT-L), and either the token-row map (N a multiple of 256) or, for any other N (1288^2: 8464), the rows of an image padded to
// a multiple of 256 so that the GEMMs cover whole tiles of ALL rows (vit_rows_per_image).  ViT-S (C = 384): its C-wide linears run as
// N = 512 with masked columns (mhmr_vit_desc.cpad), always over all rows -- opt-in (vits_256): measured slower at 16 images of 672^2.
inline bool vit_fold_eligible(int C, int N, const VitSwitches& w) {
    const bool wide = C % 256 == 0;
    const bool narrow = C % 128 == 0 && w.vits_256 && w.lnfold_allrows;
    return w.lnfold && w.rowmap && !w.gemm128 && ((wide && (N % 256 == 0 || w.lnfold_allrows)) || (!wide && narrow));
}

// ------------------------------------------------------------------------------------------------ the forward's side
// What vit_form reads of a mhmr_vit_desc: the scalars, and which optional workspaces are there
struct VitLayout { int B, C, N, Tp, cpad, lo8; bool stats, cls_pstats, splitk, v16; };

// The form of one forward: everything that is decided before the block loop.
struct VitForm {
    int rc = 0;              // MHMR_ERR_*: this description cannot run
    // Token rows of an image: patches 0..N-1, the class token at row N, zero padding up to Tp (vit_misc.hip).  When the patch rows of
    // an image are whole 256-row tiles and every linear runs on the 256x256 kernel, the five big GEMMs of a block cover the B * N
    // patch rows only (GemmArgs::img_rows: exact tile rounds) and the B class rows go through the skinny kernel (vit_cls.hip);
    // otherwise one GEMM covers all B * Tp rows.
    bool rowmap = false;
    int Mg = 0, img_rows = 0, img_stride = 0;      // rows of a block GEMM; its token-row map (0, 0: rows are physical)
    long long cls_row = 0;   // the class row inside an image
    int vcol = 0;            // its (key-permuted) V^T column
    // ... or, without the row map (N not a multiple of 256: 1288^2, 518^2), every block linear on the 256x256 kernel over ALL B * Tp rows
    // (Tp a multiple of 256: vit_rows_per_image): the class and padding rows are rows like any other, with block sums of their own
    bool allrows256 = false;
    // (C = 384, ViT-S: the three linears whose output is C wide -- V, proj, fc2 -- run as N = Cp = 512 with the last 128 columns masked,
    // GemmArgs::n_valid; the caller says with mhmr_vit_desc.cpad that their weights and per-column vectors are zero-padded for it)
    bool nmask = false;
    int Cp = 0;
    // LayerNorm fold (GemmArgs in mhmr_internal.h): needs every block linear on the 256x256 kernel and the two workspaces
    bool fold = false;
    // fp8 low-half ranges (mhmr_vit_desc.lo8): the rows of `xn` and `att` are 3C/2 elements wide (the bf8 copy of a row behind its C values)
    bool lo8 = false;
    bool lo8_ranges = false; // ... and a block's v_w8 / proj_w8 run as such a range (needs the 256x256 kernel for that launch)
    int pit = 0;             // row pitch of xn / att in elements
    int o8 = 0;              // byte offset of the bf8 copy inside such a row
    // Row statistics inside the class-row launches (vit_cls.hip, round 6): with mhmr_vit_desc.cls_pstats the residual class-row launch of
    // proj / fc2 also carries the patch rows' statistics (extra workgroups) and leaves block sums of the class rows, from which the class-row
    // consumers take (mean, rstd) themselves: no ln_stats launch at all under the token-row map.
    bool cst = false;
    // Any-order launches (mhmr_internal.h): the V projection and the class-row linears are independent of the big GEMM launched right in
    // front of them and nothing reads their outputs before the next ordinary launch
    bool ao = false;
    // Split-k residual linears (a batch of one: all rows through the 256x256 kernel, 68 / 40 tiles on 256 CUs): the k range is cut so that
    // tiles x slices fill the chip, and the reduction that follows (vit_misc.hip splitk_resid_kernel) runs the residual epilogue AND leaves
    // the row statistics, so the ln_stats launch behind such a linear disappears.  Needs the workspace mhmr_vit_desc.splitk.
    bool splitk = false;
    // A short batch (all rows, the whole qkv linear at most one round of tiles): ONE launch for Q | K | V + a transpose of the V rows
    // (gemm256.hip QKV), instead of two launches of half a round each.  Needs mhmr_vit_desc.v16 (and, per block, a V without a low half).
    bool qkv_merge = false;
    // One 896^2 image over all rows is 17 row tiles x 16 column tiles = 272 tiles: one round of the chip + 16 tiles that cost a second.
    // When the PATCH rows alone fit one round (16 x 16 = 256), fc1 -- and only fc1, and only with its LayerNorm folded -- takes the
    // token-row map and its class rows the skinny kernel; the padding rows of `hid` are then never written (they stay as allocated:
    // zero) and nobody reads what the padding rows of the residual stream become.
    bool fc1map = false;
    // mhmr_vit_desc.x3: the f16x3 forward (vit_forward_x3) runs, and nothing above applies
    bool x3 = false;
};

inline VitForm vit_form(const VitLayout& d, const VitSwitches& w, int ncu, bool anyorder_stream) {
    VitForm f;
    const int B = d.B, C = d.C, N = d.N, Tp = d.Tp, M = B * Tp;
    const bool k256 = w.rowmap && !w.gemm128;
    const bool fits = (uint64_t)M * (uint64_t)C * 4u < (1ull << 32);
    // (Tp a multiple of 256 where N is one too is the caller saying "all rows" -- the invariant at the top of this file: vit_rows_per_image
    // pads tiny batches that way, whose launches are latency-bound and not worth six class-row launches per block)
    f.rowmap = k256 && C % 256 == 0 && N % 256 == 0 && Tp % 256 != 0 && fits;
    f.Mg = f.rowmap ? B * N : M;
    f.img_rows = f.rowmap ? N : 0;
    f.img_stride = f.rowmap ? Tp : 0;
    f.cls_row = (long long)N;
    f.vcol = (N & ~12) | ((N & 4) << 1) | ((N & 8) >> 1);
    f.Cp = (C + 255) / 256 * 256;
    f.allrows256 = !f.rowmap && k256 && (C % 256 == 0 || (C % 128 == 0 && d.cpad == f.Cp)) && M % 256 == 0 && fits;
    f.nmask = f.allrows256 && C % 256 != 0;
    f.fold = (f.rowmap || f.allrows256) && w.lnfold && d.stats;
    f.lo8 = d.lo8 != 0 && C % 256 == 0;
    if (d.lo8 && !f.lo8) { f.rc = MHMR_ERR_BAD_SHAPE; return f; }
    f.lo8_ranges = f.lo8 && w.lo8 && (f.rowmap || f.allrows256);
    f.pit = f.lo8 ? C + C / 2 : C;
    f.o8 = 2 * C;
    f.cst = w.cls_stats && f.rowmap && f.fold && !f.lo8 && d.cls_pstats && C % 128 == 0 && C <= 1024;
    f.ao = w.anyorder && anyorder_stream;
    f.splitk = f.allrows256 && f.fold && d.splitk;
    f.qkv_merge = w.qkv_merge && f.allrows256 && !f.nmask && d.v16 && (M / 256) * (3 * C / 256) <= ncu;
    f.fc1map = w.fc1_rowmap && f.allrows256 && !f.nmask && N % 256 == 0 && (M / 256) * (4 * C / 256) > ncu && (B * N / 256) * (4 * C / 256) <= ncu;
    return f;
}

// MHMR_VIT_FORM_*: what mhmr_vit_form_bits reports
inline unsigned vit_form_bits(const VitForm& f) {
    return (f.rowmap ? MHMR_VIT_FORM_ROWMAP : 0u) | (f.allrows256 ? MHMR_VIT_FORM_ALLROWS256 : 0u) | (f.nmask ? MHMR_VIT_FORM_NMASK : 0u) |
           (f.fold ? MHMR_VIT_FORM_FOLD : 0u) | (f.lo8_ranges ? MHMR_VIT_FORM_LO8_RANGES : 0u) | (f.cst ? MHMR_VIT_FORM_CST : 0u) |
           (f.ao ? MHMR_VIT_FORM_AO : 0u) | (f.splitk ? MHMR_VIT_FORM_SPLITK : 0u) | (f.qkv_merge ? MHMR_VIT_FORM_QKV_MERGE : 0u) |
           (f.fc1map ? MHMR_VIT_FORM_FC1MAP : 0u) | (f.x3 ? MHMR_VIT_FORM_X3 : 0u);
}

}  // namespace
#endif
