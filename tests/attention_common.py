"""Shared by test_attention_host.py and test_attention_gpu.py: the window-attention operation of include/vsrlab_hip.h
(``VsrAttnDesc``) restated three ways.

* ``attention_formula``: the header's formula, written out as einsum + logsumexp + softmax + einsum, differentiable, in whatever
  dtype its inputs have.  ``attention_fp64`` evaluates it in fp64 in chunks of windows (no ``B x heads x Nq x Nk`` tensor above
  ``CHUNK_BYTES``) and gets dq / dk / dv / dbias from torch autograd.  Pinned on the CPU against oracle/vrt_attention_oracle.py.
* ``attention_same_precision``: the same formula in fp32 with the passes the kernels make (forward, query-stationary backward,
  key-stationary backward) and, for the bf16 build, a bf16 rounding at exactly the kernels' storage points: q * scale, K and V as
  staged, P before P V, dS before the two dS products, out and dqkv as stored.
* ``run_hip``: one descriptor through the C ABI with ctypes, every operand inside a guard band.

Inputs come from ``make_case``: bf16-representable, so input rounding contributes nothing to either build."""
import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

CHUNK_BYTES = 256 << 20
GUARD = 4096                    # elements on each side of every operand: a multiple of 4, so 16-byte alignment is kept
SENTINEL = -7.25                # finite and exact in bf16: untouched output elements are compared bit for bit


@dataclass
class Case:
    """One VsrAttnDesc and how its mask is made: None, "dense" ({0, -100}), "nonbinary" (uniform in [-3, 0]), "rowmasked" (dense with
    one query row masked on every key) or "packed" ({0, -100}, handed over bit-packed)."""
    name: str
    B: int
    heads: int
    hd: int
    N: int
    Nq: int
    Nk: int
    q0: int = 0
    k0: int = 0
    o0: int = 0
    mask: Optional[str] = None
    nW: int = 1
    Nm: int = 0
    wide: bool = False          # Cout = 2 C with c_off = C (the module's own use) instead of Cout = C, c_off = 0
    bias: bool = True
    qk_gain: float = 1.0        # multiplies q and k (large-score cases)
    seed: int = 0

    @property
    def C(self):
        return self.heads * self.hd

    @property
    def Cout(self):
        return 2 * self.C if self.wide else self.C

    @property
    def c_off(self):
        return self.C if self.wide else 0

    @property
    def scale(self):
        return self.hd ** -0.5

    @property
    def persistent(self):
        return self.Nq == self.Nk and self.Nk in (64, 128)


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def make_mask(kind, nW, Nm, Nq, Nk, gen):
    """fp32 (nW, Nm, Nm).  Only the top-left Nq x Nk block is the operation's input; the driver overwrites the rest."""
    if kind in ("dense", "packed", "rowmasked"):
        m = torch.where(torch.rand(nW, Nm, Nm, generator=gen) < 0.3, -100.0, 0.0)
        idx = torch.arange(min(Nq, Nk))
        m[:, idx, idx] = 0.0                              # compute_mask never masks a token against itself
        if kind == "rowmasked":
            m[nW - 1, Nq // 2 + 1, :] = -100.0
        return m
    assert kind == "nonbinary"
    return -3.0 * torch.rand(nW, Nm, Nm, generator=gen)


def make_case(c: Case):
    """qkv (B, N, 3, heads, hd), dout (B, N, Cout), bias (heads, Nq, Nk), mask (nW, Nm, Nm) or None: fp32 CPU tensors; qkv and dout
    bf16-representable."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    qkv = torch.randn(c.B, c.N, 3, c.heads, c.hd, generator=g)
    qkv[:, :, :2] *= c.qk_gain
    qkv = bf16_round(qkv)
    dout = bf16_round(torch.randn(c.B, c.N, c.Cout, generator=g))
    bias = torch.randn(c.heads, c.Nq, c.Nk, generator=g) if c.bias else None
    mask = make_mask(c.mask, c.nW, c.Nm, c.Nq, c.Nk, g) if c.mask else None
    return qkv, dout, bias, mask


# --------------------------------------------------------------------------------------------------------------------
# the formula
# --------------------------------------------------------------------------------------------------------------------
def attention_formula(qkv, bias, mask, windows, q0, k0, Nq, Nk, scale):
    """out = softmax((q * scale) k^T + bias[head] + mask[window % nW]) v of include/vsrlab_hip.h.
    qkv (b, N, 3, heads, hd); bias (heads, Nq, Nk) or None; mask (nW, Nm, Nm) or None; windows: the window numbers of qkv's rows
    (they choose the mask).  Returns out (b, Nq, heads * hd) and lse (b, heads, Nq)."""
    q, k, v = qkv[:, q0:q0 + Nq, 0], qkv[:, k0:k0 + Nk, 1], qkv[:, k0:k0 + Nk, 2]
    s = torch.einsum("bqhd,bkhd->bhqk", q * scale, k)
    if bias is not None:
        s = s + bias.unsqueeze(0)
    if mask is not None:
        s = s + mask[windows % mask.shape[0], :Nq, :Nk].unsqueeze(1)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v)
    return out.reshape(out.shape[0], Nq, -1), lse


def _chunks(c: Case, itemsize):
    per = max(1, CHUNK_BYTES // (c.heads * c.Nq * c.Nk * itemsize))
    return [(b0, min(c.B, b0 + per)) for b0 in range(0, c.B, per)]


def attention_fp64(c: Case, qkv, dout, bias, mask, backward=True):
    """The fp64 restatement of one descriptor.  dict: out (B, Nq, C), lse (B, heads, Nq), dq (B, Nq, heads, hd), dk, dv (B, Nk, heads,
    hd), dbias (heads, Nq, Nk).  ``dout`` is the full (B, N, Cout) cotangent; its rows [o0, o0+Nq), channels [c_off, c_off+C) count."""
    qkv, bias, mask = qkv.double(), (bias.double() if bias is not None else None), (mask.double() if mask is not None else None)
    do = dout[:, c.o0:c.o0 + c.Nq, c.c_off:c.c_off + c.C].double()
    res = {k: [] for k in ("out", "lse", "dq", "dk", "dv")}
    dbias = torch.zeros_like(bias) if bias is not None else None
    for b0, b1 in _chunks(c, 8):
        x = qkv[b0:b1].clone().requires_grad_(backward)
        bl = bias.clone().requires_grad_(backward) if bias is not None else None
        out, lse = attention_formula(x, bl, mask, torch.arange(b0, b1, device=qkv.device), c.q0, c.k0, c.Nq, c.Nk, c.scale)
        res["out"].append(out.detach())
        res["lse"].append(lse.detach())
        if backward:
            (out * do[b0:b1]).sum().backward()
            res["dq"].append(x.grad[:, c.q0:c.q0 + c.Nq, 0])
            res["dk"].append(x.grad[:, c.k0:c.k0 + c.Nk, 1])
            res["dv"].append(x.grad[:, c.k0:c.k0 + c.Nk, 2])
            if bl is not None:
                dbias += bl.grad
    r = {k: torch.cat(v) for k, v in res.items() if v}
    if backward and dbias is not None:
        r["dbias"] = dbias
    return r


def attention_same_precision(c: Case, qkv, dout, bias, mask, bf16):
    """fp32 evaluation of the same formula, pass by pass as the kernels make them; ``bf16``: round where the bf16 build stores."""
    r = bf16_round if bf16 else (lambda t: t)
    qkv = qkv.float()
    do_all = dout[:, c.o0:c.o0 + c.Nq, c.c_off:c.c_off + c.C].float()
    res = {k: [] for k in ("out", "lse", "dq", "dk", "dv")}
    dbias = torch.zeros_like(bias, dtype=torch.float32) if bias is not None else None
    for b0, b1 in _chunks(c, 4):
        q, k, v = qkv[b0:b1, c.q0:c.q0 + c.Nq, 0], qkv[b0:b1, c.k0:c.k0 + c.Nk, 1], qkv[b0:b1, c.k0:c.k0 + c.Nk, 2]
        do = do_all[b0:b1].reshape(b1 - b0, c.Nq, c.heads, c.hd)
        qs, k, v = r(q * c.scale), r(k), r(v)
        s = torch.einsum("bqhd,bkhd->bhqk", qs, k)
        if bias is not None:
            s = s + bias.float().unsqueeze(0)
        if mask is not None:
            w = torch.arange(b0, b1, device=qkv.device) % mask.shape[0]
            s = s + mask.float()[w, :c.Nq, :c.Nk].unsqueeze(1)
        # forward: one row maximum, unnormalised P rounded before P V, the row sum applied to the fp32 accumulator
        m = s.amax(dim=-1, keepdim=True)
        e = torch.exp(s - m)
        l = e.sum(dim=-1, keepdim=True)
        lse = (m + torch.log(l)).squeeze(-1)
        o = torch.einsum("bhqk,bkhd->bqhd", r(e), v) / l.squeeze(-1).transpose(1, 2).unsqueeze(-1)
        res["out"].append(r(o).reshape(b1 - b0, c.Nq, c.C))
        res["lse"].append(lse)
        # backward: P from the stored lse; delta and dbias from the fp32 P and dP; dS rounded before dS K and dS^T (q * scale)
        p = torch.exp(s - lse.unsqueeze(-1))
        dp = torch.einsum("bqhd,bkhd->bhqk", do, v)
        delta = (p * dp).sum(dim=-1, keepdim=True)
        ds = p * (dp - delta)
        if dbias is not None:
            dbias += ds.sum(dim=0)
        res["dq"].append(r(torch.einsum("bhqk,bkhd->bqhd", r(ds), k) * c.scale))
        res["dk"].append(r(torch.einsum("bhqk,bqhd->bkhd", r(ds), qs)))
        res["dv"].append(r(torch.einsum("bhqk,bqhd->bkhd", r(p), do)))
    out = {k: torch.cat(v) for k, v in res.items()}
    if dbias is not None:
        out["dbias"] = dbias
    return out


# --------------------------------------------------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------------------------------------------------
def _guarded(shape, dtype, dev, fill):
    """A contiguous tensor of ``shape`` that is a view into a buffer with GUARD elements of ``fill`` on each side."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _sync():
    """A HIP error here is a GPU fault: nothing more is started on the card in this session."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit(f"GPU fault in the window attention: {e}", returncode=3)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def host_pack(mask):
    """bits[w][i][j // 32] |= (mask[w][i][j] != 0) << (j % 32), as int32 (nW, Nm, Nm / 32)."""
    nW, Nm, _ = mask.shape
    nz = (mask != 0).reshape(nW, Nm, Nm // 32, 32).to(torch.int64)
    w = (nz << torch.arange(32, device=mask.device)).sum(dim=-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def run_hip(c: Case, qkv, dout, bias, mask, dtype, dev, backward=True, lib=None):
    """One descriptor through vsr_window_attention_fwd / _bwd.  Every input is a view into a larger buffer whose surround is NaN, and
    so is everything inside an input that the descriptor does not name (q rows outside the queries, k / v rows outside the keys, dout
    outside its rows and channels, the mask outside its top-left block): a stray read shows as NaN in a result.  Every output sits in
    a sentinel-filled buffer, and whatever the descriptor does not name is compared with the sentinel bit for bit.
    ``lib``: another build of the library, loaded with ctypes (tools/ab_attention.py); default: the package's own.
    Returns the same dict as ``attention_fp64`` (fp32 CPU tensors)."""
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    lib = _lib.load() if lib is None else lib
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    nan = float("nan")
    H, hd, C = c.heads, c.hd, c.C
    rows_q, rows_k, rows_o = slice(c.q0, c.q0 + c.Nq), slice(c.k0, c.k0 + c.Nk), slice(c.o0, c.o0 + c.Nq)
    chans = slice(c.c_off, c.c_off + C)

    _, g_qkv = _guarded((c.B, c.N, 3, H, hd), tdt, dev, nan)
    g_qkv[:, rows_q, 0] = qkv[:, rows_q, 0].to(dev, tdt)
    g_qkv[:, rows_k, 1:] = qkv[:, rows_k, 1:].to(dev, tdt)
    _, g_do = _guarded((c.B, c.N, c.Cout), tdt, dev, nan)
    g_do[:, rows_o, chans] = dout[:, rows_o, chans].to(dev, tdt)
    g_bias = None
    if bias is not None:
        _, g_bias = _guarded((H, c.Nq, c.Nk), torch.float32, dev, nan)
        g_bias.copy_(bias)
    g_mask, packed, Nm = None, 0, c.Nm
    if mask is not None:
        if c.mask == "packed":
            # the bits outside the top-left block are set at random: nothing may depend on them
            full = torch.where(torch.rand(mask.shape, generator=torch.Generator().manual_seed(5)) < 0.5, -100.0, 0.0)
            full[:, :c.Nq, :c.Nk] = mask[:, :c.Nq, :c.Nk]
            _, g_mask = _guarded((c.nW, Nm, Nm // 32), torch.int32, dev, -1)
            g_mask.copy_(host_pack(full))
            packed = 1
        else:
            _, g_mask = _guarded((c.nW, Nm, Nm), torch.float32, dev, nan)
            g_mask[:, :c.Nq, :c.Nk] = mask[:, :c.Nq, :c.Nk].to(dev)

    b_out, g_out = _guarded((c.B, c.N, c.Cout), tdt, dev, SENTINEL)
    b_lse, g_lse = _guarded((c.B, H, c.Nq), torch.float32, dev, SENTINEL)
    d = _lib.AttnDesc(c.B, c.N, H, hd, c.q0, c.k0, c.o0, c.Nq, c.Nk, c.Cout, c.c_off, c.nW, Nm, c.scale,
                      VF.DT_BF16 if dtype == "bf16" else VF.DT_F32, packed, -100.0 if packed else 0.0)
    st, P = VF._stream(), VF._ptr
    rc = lib.vsr_window_attention_fwd(ctypes.byref(d), P(g_qkv), P(g_bias), P(g_mask), P(g_out), P(g_lse), st)
    assert rc == 0, ("fwd status", rc)
    _sync()
    res = {"out": g_out[:, rows_o, chans].float().cpu(), "lse": g_lse.cpu().clone()}
    g_out[:, rows_o, chans] = SENTINEL
    g_lse.fill_(SENTINEL)
    untouched = {"out": b_out, "lse": b_lse}
    if backward:
        b_dqkv, g_dqkv = _guarded((c.B, c.N, 3, H, hd), tdt, dev, SENTINEL)
        b_delta, g_delta = _guarded((c.B, H, c.Nq), torch.float32, dev, SENTINEL)
        g_lse.copy_(res["lse"])
        g_dbias = None
        if bias is not None:
            b_dbias, g_dbias = _guarded((H, c.Nq, c.Nk), torch.float32, dev, SENTINEL)
            g_dbias.zero_()
        rc = lib.vsr_window_attention_bwd(ctypes.byref(d), P(g_qkv), P(g_bias), P(g_mask), P(g_do), P(g_lse), P(g_delta), P(g_dqkv),
                                          P(g_dbias), st)
        assert rc == 0, ("bwd status", rc)
        _sync()
        res["dq"] = g_dqkv[:, rows_q, 0].float().cpu()
        res["dk"] = g_dqkv[:, rows_k, 1].float().cpu()
        res["dv"] = g_dqkv[:, rows_k, 2].float().cpu()
        assert torch.equal(_bits(g_lse), _bits(res["lse"].to(dev))), "the backward wrote lse"
        g_dqkv[:, rows_q, 0] = SENTINEL
        g_dqkv[:, rows_k, 1:] = SENTINEL
        g_delta.fill_(SENTINEL)
        g_lse.fill_(SENTINEL)
        untouched.update(dqkv=b_dqkv, delta=b_delta)
        if bias is not None:
            res["dbias"] = g_dbias.cpu().clone()
            g_dbias.fill_(SENTINEL)
            untouched["dbias"] = b_dbias
    for k, buf in untouched.items():
        assert torch.equal(_bits(buf), _bits(torch.full_like(buf, SENTINEL))), f"{k}: an element outside the descriptor's ranges was written"
    return res


# --------------------------------------------------------------------------------------------------------------------
# the criterion
# --------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def worst_row(a, b):
    """max over rows of max|a - b| in the row, normalised by the tensor's max|b|."""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
