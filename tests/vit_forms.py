"""The ViT forward, form by form: fp64 truth, a rounding model, the case table and the harness of tests/test_gpu_vit_forms.py,
tests/test_vit_forms_host.py and tests/vit_forms_child.py.  Not a conftest and no fixtures: plain functions.

``mhmr_vit_forward`` (csrc/vit_plan.h vit_form -> csrc/capi.hip vit_block_ops -> vit_launch) picks one of about ten launch sequences per call.  Every case
below names one of them, says how it is selected (only through switches Python reads per call, ``pack_encoder`` arguments and NULLed
optional workspace pointers -- never through the switches C++ reads once per process) and which bits ``mhmr_vit_form_bits`` must report.

Two references, neither of which runs a project kernel:
  * ``fp64_stream``      oracle.dinov2_ref in fp64: the residual stream after the patch embedding and after every block, in the kernels' row
                         order (patch n at row n, class token at row N), and the final-norm features of every depth;
  * ``rounding_model``   the same fp64 arithmetic with values rounded to the operand type exactly where the HIP path stores or multiplies
                         16-bit values.  Its distance from the truth is the noise floor that CORRECT 16-bit arithmetic leaves; the gate
                         of a form is a multiple of it (``GATE``), never a number taken from the kernels.
"""
from __future__ import annotations

import copy
import ctypes as C
import functools
import math

import torch

import parity
import synthetic
from multi_hmr_amd import _lib, vit
from multi_hmr_amd.packing import roundup
from oracle import dinov2_ref

IMG = 224                    # G = 16, N = 256, T = 257: the smallest size at which the token-row map exists (N a multiple of 256)
DEPTH = 3                    # block 0 unfolded, block 1 folded, the last block without a next_f1
PATCH = 14
QSCALE = 64 ** -0.5 * math.log2(math.e)       # include/mhmr.h MHMR_ATTN_QSCALE
#: worst row of the kernels <= GATE x worst row of the rounding model: 2x for what a maximum moves between two draws of rounding order
#: (tests/parity.py), 2x for what the model leaves out (fp32 accumulation, exp2 / erf approximations, the fold's acc - mean colsum)
GATE = 4.0
X3_FLOOR = 1e-5              # f16x3: the fp32-operand model, floored
SEEDS = {"dinov2_vits14": 301, "dinov2_vitb14": 302, "dinov2_vitl14": 303}
BITS = _lib.VIT_FORM_BITS
#: pointers ``run_form(null=...)`` may clear, with what goes with them
NULLABLE = {"cls_pstats": (), "splitk": ("splitk_bytes",), "v16": (), "pstats": (), "rowstats": ()}

_ROW = {"env": {"MHMR_TINY_ALLROWS": "0"}}
#: name -> backbone, B, env (switches Python reads per call), pack (pack_encoder arguments), null (cleared pointers), want (bit -> bool)
CASES = {
    "plain128": dict(backbone="dinov2_vits14", B=2, want=dict(rowmap=0, allrows256=0, fold=0, x3=0)),
    "rowmap_nofold": dict(backbone="dinov2_vitb14", B=3, pack=dict(lnfold=False), want=dict(rowmap=1, fold=0)),
    "rowmap_fold_lnstats": dict(backbone="dinov2_vitb14", B=3, null=("cls_pstats",), want=dict(rowmap=1, fold=1, cst=0), **_ROW),
    "rowmap_fold_cst": dict(backbone="dinov2_vitb14", B=3, want=dict(rowmap=1, fold=1, cst=1), **_ROW),
    "rowmap_fold_cst_vitl": dict(backbone="dinov2_vitl14", B=3, want=dict(rowmap=1, fold=1, cst=1), **_ROW),
    # class-row Q | K | V as Q | K + V in block 0 (V low half, unfolded) and as one launch behind it; as one launch everywhere; and
    # Q | K + V in the FOLDED block 1 (the V slice of the folded column sums in the class-row kernel)
    "rowmap_fold_cst_wlo_b0": dict(backbone="dinov2_vitb14", B=3, pack=dict(wlo="v+proj@0"), want=dict(rowmap=1, fold=1, cst=1), **_ROW),
    "rowmap_fold_cst_wlo_none": dict(backbone="dinov2_vitb14", B=3, pack=dict(wlo=""), want=dict(rowmap=1, fold=1, cst=1), **_ROW),
    "rowmap_fold_cst_wlo_b1": dict(backbone="dinov2_vitb14", B=3, pack=dict(wlo="v+proj@1"), want=dict(rowmap=1, fold=1, cst=1), **_ROW),
    "rowmap_fold_lo8": dict(backbone="dinov2_vitb14", B=3, env={"MHMR_LO8": "1", "MHMR_TINY_ALLROWS": "0"},
                            want=dict(rowmap=1, fold=1, lo8_ranges=1, cst=0)),
    # (vit.py pads an unfolded pack to N + 64 rows, the token-row map; Tp = 512 with unfolded weights is the caller saying "all rows")
    "allrows_nofold": dict(backbone="dinov2_vitb14", B=1, pack=dict(lnfold=False), tp_all_rows=True,
                           null=("pstats", "rowstats", "splitk", "v16"), want=dict(rowmap=0, allrows256=1, fold=0, splitk=0, qkv_merge=0)),
    "allrows_fold_unsplit": dict(backbone="dinov2_vitb14", B=1, null=("splitk", "v16"), want=dict(allrows256=1, fold=1, splitk=0, qkv_merge=0)),
    # block 0's V has a low half (Q | K and V as two launches), blocks 1 and 2 run the merged launch
    "allrows_splitk_merge": dict(backbone="dinov2_vitb14", B=1, pack=dict(wlo="v+proj@0"), want=dict(allrows256=1, fold=1, splitk=1, qkv_merge=1)),
    "allrows_splitk_merge_vitl": dict(backbone="dinov2_vitl14", B=1, pack=dict(wlo="v+proj@0"),
                                      want=dict(allrows256=1, fold=1, splitk=1, qkv_merge=1)),
    "allrows_fc1map": dict(backbone="dinov2_vitb14", B="fc1map", want=dict(allrows256=1, fold=1, fc1map=1)),
    "masked_vits": dict(backbone="dinov2_vits14", B=2, env={"MHMR_VITS_256": "1"}, want=dict(allrows256=1, nmask=1, fold=1)),
    "f16x3": dict(backbone="dinov2_vits14", B=2, precision="f16x3", want=dict(x3=1)),
}
BF16_CASES = ("rowmap_fold_cst", "allrows_splitk_merge", "plain128")
#: the cases whose padding rows of `att` / `hid` nobody writes: they must stay as allocated (zero)
PADDING_STAYS = ("rowmap_nofold", "rowmap_fold_lnstats", "rowmap_fold_cst", "rowmap_fold_cst_vitl", "rowmap_fold_cst_wlo_b0",
                 "rowmap_fold_cst_wlo_none", "rowmap_fold_cst_wlo_b1", "rowmap_fold_lo8", "allrows_fc1map")
ANYORDER_CASES = ("rowmap_fold_cst", "rowmap_fold_lnstats", "allrows_splitk_merge", "allrows_fc1map")
#: switches the cases set; a test clears the others so that a case never inherits a neighbour's
ENV_SWITCHES = ("MHMR_TINY_ALLROWS", "MHMR_LO8", "MHMR_VITS_256")


def case_env(name: str) -> dict:
    """Every switch of ENV_SWITCHES -> its value for this case (None: unset)."""
    env = CASES[name].get("env", {})
    return {k: env.get(k) for k in ENV_SWITCHES}


def case_precision(name: str, precision: str = "f16") -> str:
    return CASES[name].get("precision", precision)


def fc1map_batch(ncu: int, Cd: int = 768, N: int = 256, Tp: int = 512) -> int:
    """The smallest tiny batch for which csrc/vit_plan.h vit_form takes fc1 alone under the token-row map on a device of ncu CUs: all rows
    of fc1 are more 256x256 tiles than CUs, the patch rows alone are not."""
    for B in range(1, 129):
        if (B * Tp // 256) * (4 * Cd // 256) > ncu and (B * N // 256) * (4 * Cd // 256) <= ncu and (B * Tp // 256) * (Cd // 256) <= 128:
            return B
    raise ValueError(f"no fc1map batch on {ncu} CUs")


def case_batch(name: str, ncu: int = 256) -> int:
    B = CASES[name]["B"]
    return fc1map_batch(ncu) if B == "fc1map" else B


# ------------------------------------------------------------------------------------------------ weights and inputs
@functools.lru_cache(maxsize=None)
def make_encoder(backbone: str):
    """A depth-3 DINOv2 encoder (the oracle's module, fp32) with seeded weights: a seed per backbone."""
    sd = synthetic.make_state_dict(backbone, IMG, seed=SEEDS[backbone], depth_override=DEPTH)
    enc = dinov2_ref.build(backbone, depth_override=DEPTH)
    pre = "backbone.encoder."
    enc.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)
    return enc.eval().requires_grad_(False)


def make_images(B: int, seed: int = 0) -> torch.Tensor:
    """[B, 3, 224, 224] fp32, a different image in every slot; image b is the same for every B."""
    out = []
    for b in range(B):
        g = torch.Generator().manual_seed(7919 * seed + 1000 + b)
        out.append(torch.empty(3, IMG, IMG).normal_(0.0, 1.0, generator=g) + 0.3 * torch.empty(3, 1, 1).normal_(0.0, 1.0, generator=g))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------ references
def _kernel_order(t):
    """[B, 1 + N, C] class token first -> class token last (row N)"""
    return torch.cat([t[:, 1:], t[:, :1]], dim=1)


@torch.no_grad()
def fp64_stream(enc, x):
    """-> (stream, feats): stream[l] [B, T, C] fp64 = the residual stream after the patch embedding (l = 0) and after block l, in the
    kernels' row order; feats[l] [B, N, C] = the final norm of stream[l] without the class token (feats[-1]: the encoder's output)."""
    e = copy.deepcopy(enc).double()
    t = e.prepare_tokens(x.double())
    outs = [t]
    for blk in e.blocks:
        t = blk(t)
        outs.append(t)
    return [_kernel_order(t) for t in outs], [e.norm(t)[:, 1:] for t in outs]


@torch.no_grad()
def rounding_model(enc, x, tdt, fold: bool = False, wlo: dict | None = None, taps: list | None = None):
    """The fp64 forward with roundings to ``tdt`` where the HIP path stores or multiplies 16-bit values: the im2col patches and the patch
    weight; xn (the LayerNorm output -- under the fold the raw residual copy, with the folded weight W diag(w_ln) rounded after folding
    as vit.pack_encoder.folded does); Q scale | K, V, the probabilities, att, hid after the GELU; every weight (hi + lo where
    ``wlo[block]`` names 'v' / 'proj').  No fp32 effect is modelled.  Same return value as ``fp64_stream``.
    taps: a list that receives, per block, what the attention reads -- dict(q = Q scale, k, v), each [B, T, C] as stored."""
    e = copy.deepcopy(enc).double()
    wlo = wlo or {}
    r = lambda t: t.to(tdt).double()

    def w16(W, lo_rows=None):
        hi = r(W)
        if lo_rows is not None:
            hi[lo_rows] = hi[lo_rows] + r(W[lo_rows] - hi[lo_rows])
        return hi

    B, S = x.shape[0], x.shape[2]
    G, Cd, H = S // PATCH, e.embed_dim, e.num_heads
    N = G * G
    p = x.double().unfold(2, PATCH, PATCH).unfold(3, PATCH, PATCH)                    # [B, 3, G, G, 14, 14]
    p = p.permute(0, 2, 3, 1, 4, 5).reshape(B, N, 3 * PATCH * PATCH)                  # (c, py, px) along k
    pos = dinov2_ref.interpolate_pos_embed(e.pos_embed, G).double()
    tok = r(p) @ w16(e.patch_embed.proj.weight.reshape(Cd, -1)).T + e.patch_embed.proj.bias + pos[:, 1:]
    t = torch.cat([tok, (e.cls_token + pos[:, :1]).expand(B, 1, Cd)], dim=1)
    outs = [t]
    heads = lambda a: a.reshape(B, -1, H, 64).transpose(1, 2)

    def linear_behind_norm(t, norm, lin, folded, lo_rows=None):
        W, b = lin.weight, lin.bias
        if not folded:
            return r(norm(t)) @ w16(W, lo_rows).T + b
        mean = t.mean(-1, keepdim=True)
        rstd = (t.var(-1, unbiased=False, keepdim=True) + norm.eps) ** -0.5
        Wf = w16(W * norm.weight[None, :], lo_rows)
        return rstd * (r(t) @ Wf.T - mean * Wf.sum(1)) + (b + W @ norm.bias)

    all_rows = slice(None)
    for l, blk in enumerate(e.blocks):
        lo = wlo.get(l, ())
        qkv = linear_behind_norm(t, blk.norm1, blk.attn.qkv, fold and l > 0, slice(2 * Cd, 3 * Cd) if "v" in lo else None)
        q, k, v = r(qkv[..., :Cd] * QSCALE), r(qkv[..., Cd:2 * Cd]), r(qkv[..., 2 * Cd:])
        if taps is not None:
            taps.append(dict(q=q, k=k, v=v))
        q, k, v = heads(q), heads(k), heads(v)
        s = q @ k.transpose(-2, -1)                                                    # log2 units
        pr = r(torch.exp2(s - s.amax(-1, keepdim=True)))
        att = r(((pr @ v) / pr.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, -1, Cd))
        t = t + blk.ls1.gamma * (att @ w16(blk.attn.proj.weight, all_rows if "proj" in lo else None).T + blk.attn.proj.bias)
        hid = r(torch.nn.functional.gelu(linear_behind_norm(t, blk.norm2, blk.mlp.fc1, fold)))
        t = t + blk.ls2.gamma * (hid @ w16(blk.mlp.fc2.weight).T + blk.mlp.fc2.bias)
        outs.append(t)
    return outs, [e.norm(t)[:, :N] for t in outs]


_REF = {}


def truth(backbone: str, B: int, seed: int = 0):
    """fp64_stream of the case inputs: computed once, shared, never modified."""
    key = ("truth", backbone, B, seed)
    if key not in _REF:
        _REF[key] = fp64_stream(make_encoder(backbone), make_images(B, seed))
    return _REF[key]


def model_of(backbone: str, B: int, precision: str, fold: bool, wlo: dict, seed: int = 0):
    """rounding_model of the case inputs in the case's operand type ('f16x3': fp32 operands; 'f64': none -- the truth), computed once and
    shared.  -> (stream, feats, taps)"""
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f16x3": torch.float32, "f64": torch.float64}[precision]
    key = ("model", backbone, B, seed, precision, bool(fold), tuple(sorted((i, tuple(v)) for i, v in (wlo or {}).items())))
    if key not in _REF:
        taps = []
        _REF[key] = rounding_model(make_encoder(backbone), make_images(B, seed), tdt, fold=fold, wlo=wlo, taps=taps) + (taps,)
    return _REF[key]


def truth_taps(backbone: str, B: int, seed: int = 0):
    """What the attention of every block reads, in fp64: the taps of the rounding model without any rounding (tests/test_vit_forms_host.py:
    that model is the truth to 1e-12)."""
    return model_of(backbone, B, "f64", False, {}, seed)[2]


def swap23(t):
    """The key permutation of the V^T rows (include/mhmr.h MHMR_EPI_VT): bits 2 and 3 of the token index change places."""
    return (t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)


def attention_operands(ws: dict, P: dict, B: int):
    """Q scale, K, V [B, T, C] as the last block of a forward left them in the workspace (`qk`: Q | K rows; `vt`: V^T [B, H, 64, Tp] with
    permuted keys)."""
    Cd, H, T, Tp = P["C"], P["H"], P["T"], ws["Tp"]
    qk = ws["qk"].view(B, Tp, 2 * Cd)[:, :T]
    cols = swap23(torch.arange(T, device=qk.device))
    v = ws["vt"].view(B, H, 64, Tp)[..., cols].permute(0, 3, 1, 2).reshape(B, T, Cd)
    return dict(q=qk[..., :Cd].clone(), k=qk[..., Cd:].clone(), v=v.clone())


# ------------------------------------------------------------------------------------------------ metric
def row_errors(got, ref):
    """e_r = |got_r - ref_r|_2 / |ref_r|_2 for every token row: [..., rows, C] -> [..., rows] fp64"""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return (got - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)


def worst_rows(got, ref, N: int) -> dict:
    """The maximum of e_r with its image and row, over all rows ('all'), the patch rows ('patch': rows < N) and the class rows ('cls':
    row N, absent from the features).  got, ref: [B, rows, C]."""
    e = row_errors(got, ref)

    def worst(sub, row0):
        if sub.numel() == 0:
            return None
        i = int(sub.argmax())
        return dict(e=float(sub.flatten()[i]), image=i // sub.shape[1], row=row0 + i % sub.shape[1])

    out = dict(all=worst(e, 0), patch=worst(e[:, :N], 0))
    if e.shape[1] > N:
        out["cls"] = worst(e[:, N:], N)
    return out


def gate(model_worst: float, precision: str) -> float:
    """The bound on the kernels' worst row where the rounding model's worst row is model_worst: GATE x the model (f16x3: the fp32-operand
    model floored at X3_FLOOR), and never above GATE x the whole-tensor tolerance of tests/parity.py applied per row."""
    tol = parity.TOL["f16" if precision == "f16x3" else precision]
    if precision == "f16x3":
        model_worst = max(model_worst, X3_FLOOR)
    return min(GATE * model_worst, GATE * tol)


# ------------------------------------------------------------------------------------------------ form bits
def bit_names(bits: int) -> set:
    return {n for i, n in enumerate(BITS) if bits >> i & 1}


def check_want(names: set, want: dict, where=""):
    for bit, on in want.items():
        assert (bit in names) == bool(on), f"{where}: form bit '{bit}' is {'set' if bit in names else 'clear'}, the case needs it " \
                                           f"{'set' if on else 'clear'} (form: {sorted(names)})"


def splitk_slices(M: int, N: int, K: int, ncu: int) -> int:
    """Slices of csrc/gemm.hip mhmr_splitk_plan (0: not split)."""
    if M <= 0 or M % 256 or N % 256 or K % 128 or N > 1024 or ncu <= 0:
        return 0
    tiles, nt = (M // 256) * (N // 256), K // 64
    S = min(ncu // tiles, 8, nt // 4)
    if S < 2:
        return 0
    ks = (nt + S - 1) // S
    ks += ks & 1
    S = (nt + ks - 1) // ks
    return S if S >= 2 else 0


def case_tokens(P: dict, B: int, name: str) -> int:
    """Rows per image of the case's workspace."""
    return vit.padded_tokens(dict(P, fold=True) if CASES[name].get("tp_all_rows") else P, B)


def predict_bits(P: dict, B: int, name: str, ncu: int = 256) -> set:
    """The form of a case from the Python side alone: vit.row_map / padded_tokens / tiny_batch, the optional workspaces that
    vit.WorkspaceCache allocates for this pack and batch, the pointers the case clears.  'ao' is not predicted (a process-wide switch)."""
    if P.get("x3"):
        return {"x3"}
    Cd, N = P["C"], P["N"]
    Tp = case_tokens(P, B, name)
    M = B * Tp
    null = set(CASES[name].get("null", ()))
    rm = vit.row_map(P, B) and not CASES[name].get("tp_all_rows")
    have = set()
    has_fold_ws = P.get("fold") or CASES[name].get("tp_all_rows")
    if has_fold_ws:
        have |= {"pstats", "rowstats"}
        if rm:
            have.add("cls_pstats")
        if not P.get("lo8") and Tp % 256 == 0 and not rm and max(splitk_slices(M, Cd, K, ncu) for K in (Cd, 2 * Cd, 4 * Cd)):
            have |= {"splitk", "v16"}
    have -= null
    out = set()
    rowmap = Cd % 256 == 0 and N % 256 == 0 and Tp % 256 != 0
    assert rowmap == bool(rm), (name, "vit.row_map and the rows per image disagree", rowmap, rm, Tp)
    allrows = not rowmap and (Cd % 256 == 0 or (Cd % 128 == 0 and P.get("cpad") == roundup(Cd, 256))) and M % 256 == 0
    nmask = allrows and Cd % 256 != 0
    fold = (rowmap or allrows) and {"pstats", "rowstats"} <= have
    lo8 = bool(P.get("lo8"))
    flags = dict(rowmap=rowmap, allrows256=allrows, nmask=nmask, fold=fold, lo8_ranges=lo8 and (rowmap or allrows),
                 cst=rowmap and fold and not lo8 and "cls_pstats" in have and Cd <= 1024,
                 splitk=allrows and fold and "splitk" in have,
                 qkv_merge=allrows and not nmask and "v16" in have and (M // 256) * (3 * Cd // 256) <= ncu,
                 fc1map=allrows and not nmask and N % 256 == 0 and (M // 256) * (4 * Cd // 256) > ncu and (B * N // 256) * (4 * Cd // 256) <= ncu)
    return {k for k, v in flags.items() if v}


# ------------------------------------------------------------------------------------------------ harness
def pack_case(name: str, precision: str = "f16", device="cuda:0") -> dict:
    """vit.pack_encoder of the case (its environment switches must be set: ``case_env``)."""
    c = CASES[name]
    return vit.pack_encoder(make_encoder(c["backbone"]), IMG, case_precision(name, precision), device, **c.get("pack", {}))


def _extra(P, B, z):
    # ctx16 with ldctx = C + 64 and 128 rows behind the B * N rows the forward may write
    return dict(ctx16=z(B * P["N"] + 128, P["C"] + 64))


SENTINEL = -7.0
_ALL_ROWS_PACKS = {}         # id(pack) -> (the pack, its copy marked as folded: vit.padded_tokens then pads the rows per image to 256)


def run_form(P: dict, B: int, x, *, L=None, null=(), cache=None, tp_all_rows=False) -> dict:
    """One ``mhmr_vit_forward`` of batch x in the workspace of (P, B) on the current stream, behind ``mhmr_vit_form_bits`` of the same
    description.  L: a smaller depth; null: optional pointers cleared to step the form down; tp_all_rows: the workspace of an unfolded
    pack with rows per image padded as for the all-rows form.  -> feat32 [B, N, C], ctx16 (ldctx = C + 64, pre-filled with SENTINEL),
    resid [B, Tp, C] (all rows), bits (names), and the workspace itself (ws)."""
    lib = _lib.lib()
    cache = cache if cache is not None else vit.WorkspaceCache()
    if tp_all_rows:
        P = _ALL_ROWS_PACKS.setdefault(id(P), (P, dict(P, fold=True)))[1]
    ws = cache.get(P, B, _extra)
    d = _lib.VitDesc.from_buffer_copy(ws["vit_desc"])        # the cached description stays as built
    if L is not None:
        d.L = L
    for n in null:
        setattr(d, n, None)
        for m in NULLABLE[n]:
            setattr(d, m, 0)
    x = x.to(P["device"]).contiguous()
    assert x.shape == (B, 3, P["S"], P["S"]) and x.dtype == torch.float32
    stream = torch.cuda.current_stream(x.device).cuda_stream
    bits = C.c_uint(0)
    _lib.check(lib.mhmr_vit_form_bits(C.byref(d), stream, C.byref(bits)), "mhmr_vit_form_bits")
    ws["ctx16"].fill_(SENTINEL)
    _lib.check(lib.mhmr_vit_forward(C.byref(d), x.data_ptr(), ws["feat32"].data_ptr(), ws["ctx16"].data_ptr(), P["C"] + 64, stream),
               "mhmr_vit_forward")
    torch.cuda.synchronize(x.device)
    Tp = ws["Tp"]
    return dict(feat32=ws["feat32"].view(B, P["N"], P["C"]).clone(), ctx16=ws["ctx16"].clone(), resid=ws["resid"].view(B, Tp, P["C"]).clone(),
                bits=bit_names(bits.value), Tp=Tp, ws=ws)


def run_case(name: str, P: dict, B: int, x, cache, L=None) -> dict:
    c = CASES[name]
    return run_form(P, B, x, L=L, null=c.get("null", ()), cache=cache, tp_all_rows=bool(c.get("tp_all_rows")))


def cu_count() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count
