"""The layout rule of the ViT forward as multi_hmr_amd/vit.py stated it before the rule moved into the library (csrc/vit_plan.h,
``mhmr_vit_plan``): the bodies of ``tiny_batch``, ``row_map``, ``padded_tokens``, ``fold_eligible`` and ``lo8_eligible`` and the allocation
conditions of ``WorkspaceCache.get``, moved here verbatim.  The only change: every ``os.environ`` read is a lookup in ``sw``, a dict of
``_lib.PLAN_SWITCHES`` name -> bool (``switches(mask)``), and the device's split-k answer (``mhmr_splitk_workspace_bytes``, which asks the
current device) is ``vit_forms.splitk_slices`` on ``ncu`` compute units.  tests/test_vit_plan_host.py holds the library against it."""
from multi_hmr_amd import _lib
from multi_hmr_amd.packing import roundup

import vit_forms as vf


def switches(mask: int) -> dict:
    return {n: bool(mask & bit) for n, bit in _lib.PLAN.items()}


def lo8_eligible(C: int, sw: dict) -> bool:
    return C % 256 == 0 and sw["lo8"] and not sw["gemm128"]


def fold_eligible(C: int, N: int, sw: dict) -> bool:
    wide = C % 256 == 0
    narrow = C % 128 == 0 and sw["vits_256"] and sw["lnfold_allrows"]
    return (sw["lnfold"] and sw["rowmap"] and not sw["gemm128"] and
            ((wide and (N % 256 == 0 or sw["lnfold_allrows"])) or (not wide and narrow)))


def tiny_batch(P: dict, B: int) -> bool:
    return P["C"] % 256 == 0 and (B * roundup(P["T"], 256) // 256) * (P["C"] // 256) <= 128


def row_map(P: dict, B: int, sw: dict) -> bool:
    T = P["T"]
    return (not P.get("x3") and sw["rowmap"] and not sw["gemm128"] and P["C"] % 256 == 0 and (T - 1) % 256 == 0 and
            B * roundup(T, 64) * P["C"] * 4 < 2 ** 32 and not (P.get("fold") and tiny_batch(P, B) and sw["tiny_allrows"]))


def padded_tokens(P: dict, B: int, sw: dict) -> int:
    if P.get("x3"):
        return roundup(P["T"], 256 if P["C"] % 256 == 0 else 128)      # all rows through every linear: whole tiles for every batch size
    if P.get("fold") and (P.get("cpad") or (P["T"] - 1) % 256 or (not row_map(P, B, sw) and tiny_batch(P, B) and sw["rowmap"] and
                                                                  not sw["gemm128"])):
        return roundup(P["T"], 256)        # folded LayerNorms without the row map: whole 256-row tiles of all rows, for every batch size
    t64, t128 = roundup(P["T"], 64), roundup(P["T"], 128)
    # the predicate of csrc/gemm256.hip mhmr_gemm256_eligible for the residual GEMMs over all B * Tp rows (32-bit residual offsets),
    # and the switch that forces the 128x128 kernel everywhere
    all_rows_256 = (P["C"] % 256 == 0 and (B * t64) % 256 == 0 and B * t64 * P["C"] * 4 < 2 ** 32 and not sw["gemm128"])
    return t64 if (row_map(P, B, sw) and not sw["gemm128"]) or all_rows_256 else t128


def workspaces(P: dict, Bh: int, sw: dict, ncu: int) -> dict:
    """What ``WorkspaceCache.get`` allocated for one image block of Bh images, as the fields of ``mhmr_vit_plan_result``."""
    Cd, H = P["C"], P["H"]
    Tp = padded_tokens(P, Bh, sw)
    x3 = bool(P.get("x3"))
    out = dict(Tp=Tp, row_map=int(bool(row_map(P, Bh, sw))))
    if x3:
        out["pitch"], out["attn_flags"] = 2 * Cd, 0
    else:
        pit = Cd + Cd // 2 if P.get("lo8") else Cd       # lo8: a row of xn / att carries its bf8 copy behind its C values
        out["pitch"], out["attn_flags"] = pit, 4 * ((Tp + 127) // 128) * H * Bh      # csrc/attention.hip mhmr_attention_flag_count_impl
    out["need_pstats"] = int(bool(P.get("fold")))
    out["need_cls_pstats"] = int(bool(P.get("fold") and not x3 and row_map(P, Bh, sw)))
    # split-k residual linears (csrc/capi.hip): only the all-rows form of a tiny batch has launches short enough to be split
    skb = 0
    if P.get("fold") and not x3 and not P.get("lo8") and Tp % 256 == 0 and not row_map(P, Bh, sw):
        # (mhmr_splitk_workspace_bytes answers 0 under MHMR_GEMM128: an environment read like the others)
        skb = 0 if sw["gemm128"] else max(vf.splitk_slices(Bh * Tp, Cd, kk, ncu) * Bh * Tp * Cd * 4 for kk in (Cd, 2 * Cd, 4 * Cd))
    out["splitk_bytes"], out["need_v16"] = skb, int(skb > 0)
    return out
