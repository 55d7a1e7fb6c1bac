"""Oracle of the backbone backward: oracle/dinov2_ref's own Block / LayerNorm modules in a chosen dtype under
torch autograd, a closed-form attention backward for the kernel-level test, one linear's forward and backward in a chosen dtype for the
long-reduction tests, and the per-tensor measure and gate of the tests.

Layouts are the library's: token rows of an image are [T real rows | padding] of ``Tp`` rows, the class token last among the real rows;
``qkv`` is [B*Tp, 3C] = (Q | K | V) un-scaled with head h at columns h*64."""
import torch

from oracle import dinov2_ref

PARAMS = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2")
#: the attribute path of every descriptor field inside dinov2_ref.Block
MODULE_NAMES = dict(ln1_w="norm1.weight", ln1_b="norm1.bias", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", proj_w="attn.proj.weight",
                    proj_b="attn.proj.bias", ls1="ls1.gamma", ln2_w="norm2.weight", ln2_b="norm2.bias", fc1_w="mlp.fc1.weight",
                    fc1_b="mlp.fc1.bias", fc2_w="mlp.fc2.weight", fc2_b="mlp.fc2.bias", ls2="ls2.gamma")


def roundup(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------ attention
def attention_forward(qkv, B, T, Tp, H, dtype=torch.float64):
    """-> (out [B*Tp, C], lse2 [B, H, Tp]) over the T real rows of every image; padding rows are zeros.  lse2 is in the exp2 domain."""
    C = qkv.shape[1] // 3
    q, k, v = (qkv.to(dtype).reshape(B, Tp, 3, H, 64)[:, :T, i].permute(0, 2, 1, 3) for i in range(3))      # [B, H, T, 64]
    s = (q * 0.125) @ k.transpose(-2, -1)
    o = s.softmax(-1) @ v
    out = torch.zeros(B, Tp, C, dtype=dtype)
    out[:, :T] = o.permute(0, 2, 1, 3).reshape(B, T, C)
    lse = torch.zeros(B, H, Tp, dtype=dtype)
    lse[:, :, :T] = torch.logsumexp(s, -1) / torch.log(torch.tensor(2.0, dtype=dtype))
    return out.reshape(B * Tp, C), lse


def attention_backward_closed_form(qkv, dO, B, T, Tp, H, dtype=torch.float64):
    """dqkv [B*Tp, 3C] by the formulas the kernels implement: P = softmax(q k^T / 8), D = rowsum(dO * O), dS = P (dO V^T - D),
    dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO.  Padding rows are zeros."""
    C = qkv.shape[1] // 3
    q, k, v = (qkv.to(dtype).reshape(B, Tp, 3, H, 64)[:, :T, i].permute(0, 2, 1, 3) for i in range(3))
    do = dO.to(dtype).reshape(B, Tp, H, 64)[:, :T].permute(0, 2, 1, 3)
    p = ((q @ k.transpose(-2, -1)) * 0.125).softmax(-1)
    o = p @ v
    d = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-2, -1) - d)
    dq, dk, dv = ds @ k * 0.125, ds.transpose(-2, -1) @ q * 0.125, p.transpose(-2, -1) @ do
    out = torch.zeros(B, Tp, 3, H, 64, dtype=dtype)
    for i, t in enumerate((dq, dk, dv)):
        out[:, :T, i] = t.permute(0, 2, 1, 3)
    return out.reshape(B * Tp, 3 * C)


def attention_backward_autograd(qkv, dO, B, T, Tp, H, dtype=torch.float64):
    """The same cotangent by torch autograd through dinov2_ref.Attention's own expression (scale on q, softmax, @ v)."""
    C = qkv.shape[1] // 3
    x = qkv.to(dtype).clone().requires_grad_()
    t = x.reshape(B, Tp, 3, H, 64)[:, :T].permute(2, 0, 3, 1, 4)
    q, k, v = t[0] * (64 ** -0.5), t[1], t[2]
    o = ((q @ k.transpose(-2, -1)).softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, C)
    (o * dO.to(dtype).reshape(B, Tp, -1)[:, :T, :C]).sum().backward()
    return x.grad


# ------------------------------------------------------------------------------------------------------ one block
def make_block(C, H, seed, dtype=torch.float64):
    """A dinov2_ref.Block with non-trivial LayerNorm / LayerScale parameters and biases (torch's default init leaves them 1 / 0)."""
    g = torch.Generator().manual_seed(seed)
    blk = dinov2_ref.Block(C, H)
    rn = lambda *s: torch.empty(*s).normal_(0, 1, generator=g)
    with torch.no_grad():
        for n in (blk.norm1, blk.norm2):
            n.weight.copy_(1.0 + 0.3 * rn(C))
            n.bias.copy_(0.2 * rn(C))
        for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
            lin.weight.copy_(rn(*lin.weight.shape) * lin.weight.shape[1] ** -0.5)
            lin.bias.copy_(0.1 * rn(*lin.bias.shape))
        blk.attn.qkv.weight[:2 * C] *= 2.0                      # logits with some spread
        blk.ls1.gamma.copy_(0.5 + 0.2 * rn(C))
        blk.ls2.gamma.copy_(0.5 + 0.2 * rn(C))
    return blk.to(dtype)


def block_params(blk):
    """{descriptor field: parameter} of a dinov2_ref.Block (or the package's block module, which has the same names)."""
    named = dict(blk.named_parameters())
    return {k: named[v] for k, v in MODULE_NAMES.items()}


def block_backward(blk, x_in, g_out, B, T, Tp, dtype=torch.float64):
    """Autograd of ``blk`` (a copy in ``dtype``) on the T real rows of x_in [B*Tp, C] against the cotangent g_out [B*Tp, C] (its rows >= T
    are not used) -> dict: g_in [B*Tp, C] (padding rows zero), one gradient per PARAMS name, and ``out`` [B*Tp, C]."""
    import copy
    blk = copy.deepcopy(blk).to(dtype)
    for p in blk.parameters():
        p.grad = None
    C = x_in.shape[1]
    x = x_in.to(dtype).reshape(B, Tp, C)[:, :T].clone().requires_grad_()
    y = blk(x)
    (y * g_out.to(dtype).reshape(B, Tp, C)[:, :T]).sum().backward()
    res = {k: p.grad.clone() for k, p in block_params(blk).items()}
    g_in = torch.zeros(B, Tp, C, dtype=dtype)
    g_in[:, :T] = x.grad
    out = torch.zeros(B, Tp, C, dtype=dtype)
    out[:, :T] = y.detach()
    res["g_in"], res["out"] = g_in.reshape(B * Tp, C), out.reshape(B * Tp, C)
    return res


# ------------------------------------------------------------------------------------------------------ one linear
def linear_forward(X, W, bias, R, dtype=torch.float64):
    """Y = X W^T + bias + R in ``dtype`` (the expression of mhmr_linear_f32 without an activation)."""
    return torch.nn.functional.linear(X.to(dtype), W.to(dtype), bias.to(dtype)) + R.to(dtype)


def linear_backward(dY, Z, X, W, dR, act, dtype=torch.float64):
    """dZ = dY * act'(Z) with Z TAKEN AS GIVEN (the taped pre-activation; ``act`` is "none" or "gelu", erf form), through autograd in
    ``dtype`` -> dict: dW = dZ^T X and db = column sums of dZ (where X is given), dX = dZ W + dR (where W is given)."""
    dZ = dY.to(dtype)
    if act == "gelu":
        z = Z.to(dtype).requires_grad_()
        (dZ,) = torch.autograd.grad((torch.nn.functional.gelu(z) * dY.to(dtype)).sum(), z)
    else:
        assert act == "none"
    out = {}
    if X is not None:
        out["dW"], out["db"] = dZ.T @ X.to(dtype), dZ.sum(0)
    if W is not None:
        out["dX"] = dZ @ W.to(dtype) + dR.to(dtype)
    return out


# ------------------------------------------------------------------------------------------------------ measure and gate
def measure(got, ref64):
    """(relative L2, maximum error over the largest fp64 magnitude) of a whole tensor; a zero fp64 norm is an error of the test."""
    ref64 = ref64.double()
    d = got.detach().cpu().double() - ref64
    n2, mx = float(ref64.norm()), float(ref64.abs().max())
    assert n2 > 0 and mx > 0, "the fp64 reference of a whole tensor is zero: nothing is measured"
    return float(d.norm()) / n2, float(d.abs().max()) / mx


def gate(tag, rows, factor=4.0):
    """rows: (name, kernel tensor, fp32 CPU torch tensor, fp64 tensor).  Prints kernel and yardstick columns, then asserts that the kernel is
    at most ``factor`` times worse than the fp32 CPU yardstick in both measures, per tensor."""
    bad = []
    for name, got, y32, r64 in rows:
        kl2, kmx = measure(got, r64)
        yl2, ymx = measure(y32, r64)
        ok = kl2 <= factor * yl2 and kmx <= factor * ymx
        print(f"[{tag}] {name}: rel L2 kernel {kl2:.3e} fp32 torch {yl2:.3e} | max/|ref|max kernel {kmx:.3e} fp32 torch {ymx:.3e}"
              f"{'' if ok else '  <-- FAILS'}")
        if not ok:
            bad.append(name)
    assert not bad, (tag, bad)
