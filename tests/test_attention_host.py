"""Host-side tests of the window attention (csrc/window_attention.hip): what vsr_window_attention_fwd / _bwd refuse before any GPU
call, and the CPU pin of the fp64 restatement (tests/attention_common.py) that test_attention_gpu.py measures the kernels against.

Every descriptor here is refused by check_args / set_mask, which return before the first launch: the pointers are fake addresses
that are never dereferenced.  (That ``Nq = 160`` is ACCEPTED by the forward needs a launch, so it is asserted, with values, in
test_attention_gpu.py::test_forward_accepts_nq_160.)"""
import ctypes

import pytest
import torch

import attention_common as AC
from helpers import golden, rand

BADARG, UNSUPPORTED = -1, -2
F32, BF16 = 0, 1
A = [0x10000000 + 0x1000000 * i for i in range(10)]        # 16-byte aligned, never dereferenced


def _lib():
    from vsrlab_amd import _lib
    return _lib, _lib.load()


def _desc(**kw):
    L, _ = _lib()
    from vsrlab_amd import functional as VF
    assert (VF.DT_F32, VF.DT_BF16) == (F32, BF16)
    f = dict(B=2, N=128, heads=6, head_dim=20, q0=0, k0=0, o0=0, Nq=128, Nk=128, Cout=120, c_off=0, nW=1, Nm=128, scale=0.25, dtype=F32,
             mask_packed=0, mask_value=0.0)
    f.update(kw)
    return L.AttnDesc(*[f[k] for k, _ in L.AttnDesc._fields_])


def _fwd(d, qkv=A[0], bias=A[1], mask=None, out=A[3], lse=A[4]):
    _, lib = _lib()
    return lib.vsr_window_attention_fwd(ctypes.byref(d) if d is not None else None, qkv, bias, mask, out, lse, None)


def _bwd(d, qkv=A[0], bias=A[1], mask=None, dout=A[3], lse=A[4], delta=A[5], dqkv=A[6], dbias=A[7]):
    _, lib = _lib()
    return lib.vsr_window_attention_bwd(ctypes.byref(d) if d is not None else None, qkv, bias, mask, dout, lse, delta, dqkv, dbias, None)


def _both(d, **kw):
    f, b = _fwd(d, **kw), _bwd(d, **kw)
    assert f == b, (f, b)
    return f


REFUSED = [
    (dict(head_dim=0), UNSUPPORTED), (dict(head_dim=33, Cout=198), UNSUPPORTED),
    (dict(N=320, Nq=320, Nk=320), UNSUPPORTED), (dict(Nk=96), UNSUPPORTED),
    (dict(Nq=16), UNSUPPORTED), (dict(Nq=48), UNSUPPORTED), (dict(N=400, Nq=400, Nk=384), UNSUPPORTED),
    # ranges that leave N
    (dict(q0=1), BADARG), (dict(k0=1), BADARG), (dict(o0=1), BADARG), (dict(q0=-1), BADARG), (dict(k0=-32), BADARG), (dict(o0=-1), BADARG),
    (dict(N=256, Nq=64, Nk=64, q0=224), BADARG), (dict(N=256, Nq=64, Nk=64, k0=193), BADARG), (dict(N=256, Nq=64, Nk=64, o0=200), BADARG),
    # channels that leave Cout
    (dict(Cout=119), BADARG), (dict(Cout=240, c_off=124), BADARG), (dict(c_off=-4), BADARG),
    # an odd head_dim: the persistent kernels stage element pairs and would read one element past each head
    (dict(head_dim=15, Cout=90), UNSUPPORTED), (dict(head_dim=1, Cout=6), UNSUPPORTED), (dict(head_dim=31, Cout=186), UNSUPPORTED),
    (dict(head_dim=15, Cout=90, N=256, Nq=64, Nk=192), UNSUPPORTED),
    # head_dim % 4 == 0: 4-element vector loads / stores of a head's slice of an out / dout row need c_off % 4 == Cout % 4 == 0
    (dict(Cout=122), UNSUPPORTED), (dict(Cout=126, c_off=6), UNSUPPORTED), (dict(Cout=121, c_off=1), UNSUPPORTED),
    # other even head_dim: pairs
    (dict(head_dim=30, Cout=181), UNSUPPORTED), (dict(head_dim=30, Cout=182, c_off=1), UNSUPPORTED),
]


@pytest.mark.parametrize("kw,status", REFUSED, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSED])
def test_descriptor_is_refused_before_any_gpu_call(kw, status):
    for dtype in (F32, BF16):
        assert _both(_desc(dtype=dtype, **kw)) == status


def test_aligned_channel_offsets_pass_the_argument_check():
    """The counterpart of the alignment refusals: the same descriptors with c_off / Cout that keep the vectors whole get past
    check_args (the next refusal, a null ``out`` / ``dout``, is the one reported)."""
    for kw in (dict(Cout=124, c_off=4), dict(Cout=240, c_off=120), dict(head_dim=30, Cout=182, c_off=2), dict(head_dim=2, Cout=14, c_off=2)):
        d = _desc(**kw)
        assert _fwd(d, out=None) == BADARG and _bwd(d, dout=None) == BADARG


def test_null_and_misaligned_pointers_are_refused():
    d = _desc()
    assert _fwd(None) == BADARG and _bwd(None) == BADARG and _both(_desc(dtype=7)) == BADARG
    assert _both(d, qkv=None) == BADARG
    assert _fwd(d, out=None) == BADARG
    for k in ("dout", "lse", "delta", "dqkv"):
        assert _bwd(d, **{k: None}) == BADARG, k
    # every operand is read or written with up to 16-byte vectors from its base
    assert _both(d, qkv=A[0] + 4) == BADARG and _both(d, bias=A[1] + 8) == BADARG
    assert _fwd(d, out=A[3] + 2) == BADARG
    for k in ("dout", "dqkv", "dbias"):
        assert _bwd(d, **{k: A[8] + 4}) == BADARG, k
    assert _both(_desc(Nm=128), mask=A[2] + 4) == BADARG


def test_mask_descriptors_are_refused():
    # bit-packed masks: the persistent kernels (Nq == Nk in {64, 128}) only, whole 32-bit words per row
    assert _both(_desc(N=256, Nq=128, Nk=64, mask_packed=1, Nm=256), mask=A[2]) == UNSUPPORTED
    assert _both(_desc(N=384, Nq=384, Nk=384, Cout=120, mask_packed=1, Nm=384), mask=A[2]) == UNSUPPORTED
    assert _both(_desc(N=256, Nq=192, Nk=192, mask_packed=1, Nm=192), mask=A[2]) == UNSUPPORTED
    assert _both(_desc(mask_packed=1, Nm=144), mask=A[2]) == UNSUPPORTED
    assert _both(_desc(N=64, Nq=64, Nk=64, mask_packed=1, Nm=80), mask=A[2]) == UNSUPPORTED
    # a mask smaller than the block that is read from it; dense rows that float4 loads cannot walk
    assert _both(_desc(Nm=96), mask=A[2]) == BADARG and _both(_desc(mask_packed=1, Nm=96), mask=A[2]) == BADARG
    assert _both(_desc(N=256, Nq=64, Nk=128, k0=128, Nm=64), mask=A[2]) == BADARG
    assert _both(_desc(Nm=130), mask=A[2]) == UNSUPPORTED


def test_nq_160_is_refused_by_the_backward_only():
    """The key-stationary pass stages its queries in chunks that divide Nq: all up to 128, else 128, else 96.  160 has none; the
    forward has no such limit (its acceptance is asserted on the GPU)."""
    for nk, dtype in ((64, F32), (128, BF16), (384, F32)):
        d = _desc(N=384, Nq=160, Nk=nk, dtype=dtype)
        assert _bwd(d) == UNSUPPORTED
        assert _fwd(d, out=None) == BADARG                  # past check_args: only the null ``out`` is refused
    assert _bwd(_desc(N=384, Nq=320, Nk=64)) == UNSUPPORTED and _bwd(_desc(N=384, Nq=224, Nk=64)) == UNSUPPORTED


def test_window_attention_core_refuses_an_odd_head_dim(monkeypatch):
    from vsrlab_amd import functional as VF
    monkeypatch.setattr(VF.attention, "_require_gpu", lambda t: None)        # where window_attention_core looks it up
    qkv = torch.zeros(2, 64, 3 * 3 * 15)
    with pytest.raises(NotImplementedError):
        VF.window_attention_core(qkv, None, torch.zeros(10, 3), torch.zeros(64, 64, dtype=torch.int64), None, 3, 0.25, "fp32")
    with pytest.raises(NotImplementedError):
        VF.window_attention_core(torch.zeros(2, 64, 3 * 3 * 34), None, torch.zeros(10, 3), torch.zeros(64, 64, dtype=torch.int64), None, 3, 0.25, "fp32")


# --------------------------------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_fp64_restatement_equals_the_oracle(tag):
    """attention_fp64, descriptor by descriptor as functional/attention.py issues them (self attention into channels [C, 2C) or [0, C), the two
    mutual attentions into the two halves of the rows), between the oracle's own qkv and proj Linears: the module output of
    oracle/vrt_attention_oracle.window_attention_forward to 1e-10, and with it the reference's golden output."""
    import torch.nn.functional as F
    from oracle import basicvsr_oracle as O
    from oracle import vrt_attention_oracle as V
    from test_vrt_parity import CASES
    from vsrlab_amd.vsr.models.VRT.modules.window_attention import WindowAttention
    dim, ws, mut, B = CASES[tag]
    heads, hd = 6, dim // 6
    m = WindowAttention(dim, ws, heads, qkv_bias=True, mut_attn=mut)
    sd = {k: (O.keyed_tensor(k, tuple(v.shape)).double() if k in dict(m.named_parameters()) else (v.double() if v.is_floating_point() else v))
          for k, v in m.state_dict().items()}
    g = golden("vrt_window_attention")
    N = ws[0] * ws[1] * ws[2]
    x = rand(int(g[f"{tag}__seed_x"]), B, N, dim, lo=-1, hi=1).double()
    mask = V.compute_mask(2 * ws[0], 16, 16, ws, tuple(i // 2 for i in ws))[:2].double() if tag == "a" else None
    want = V.window_attention_forward(sd, x, mask, heads, mut)
    assert float((want - g[f"{tag}__out"]).abs().max() / g[f"{tag}__out"].abs().max()) < 1e-6

    nW, Nm = (mask.shape[0], mask.shape[1]) if mask is not None else (1, 0)
    idx = sd["relative_position_index"][:N, :N]
    bias = sd["relative_position_bias_table"][idx.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1).contiguous()
    out = torch.zeros(B, N, 2 * dim if mut else dim, dtype=torch.float64)
    dummy = torch.zeros(B, N, out.shape[2])

    def call(qkv, q0, k0, o0, n, wide, b):
        c = AC.Case("pin", B, heads, hd, N, n, n, q0, k0, o0, nW=nW, Nm=Nm, wide=wide, bias=b is not None)
        r = AC.attention_fp64(c, qkv.reshape(B, N, 3, heads, hd), dummy, b, mask, backward=False)
        out[:, o0:o0 + n, (dim if wide else 0):(dim if wide else 0) + dim] = r["out"]

    call(F.linear(x, sd["qkv_self.weight"], sd["qkv_self.bias"]), 0, 0, 0, N, mut, bias)
    if mut:
        qm = F.linear(x + sd["position_bias"].repeat(1, 2, 1), sd["qkv_mut.weight"], sd["qkv_mut.bias"])
        call(qm, N // 2, 0, 0, N // 2, False, None)
        call(qm, 0, N // 2, N // 2, N // 2, False, None)
    got = F.linear(out, sd["proj.weight"], sd["proj.bias"])
    assert float((got - want).abs().max()) < 1e-10 * float(want.abs().max())


def test_fp64_restatement_gradients_equal_the_unchunked_formula(monkeypatch):
    """Chunking the windows changes nothing: out, lse and every gradient of a 7-window case evaluated two windows at a time equal
    one autograd pass over the formula."""
    c = AC.Case("chunk", 7, 2, 6, 96, 32, 64, 64, 0, 32, mask="nonbinary", nW=3, Nm=96, wide=True)
    qkv, dout, bias, mask = AC.make_case(c)
    whole = AC.attention_fp64(c, qkv, dout, bias, mask)
    monkeypatch.setattr(AC, "CHUNK_BYTES", 2 * c.heads * c.Nq * c.Nk * 8)
    assert len(AC._chunks(c, 8)) == 4
    parts = AC.attention_fp64(c, qkv, dout, bias, mask)
    for k in whole:
        assert float((whole[k] - parts[k]).abs().max()) <= 1e-13 * float(whole[k].abs().max()), k
    # and the same-precision evaluation is the same function: fp32 against fp64 at fp32 rounding, bf16 at bf16 rounding
    for bf16, tol in ((False, 2e-6), (True, 2e-2)):
        e = AC.attention_same_precision(c, qkv, dout, bias, mask, bf16)
        assert set(e) == set(whole)
        for k in whole:
            assert AC.rel_l2(e[k], whole[k]) < tol, (k, bf16, AC.rel_l2(e[k], whole[k]))


@pytest.mark.parametrize("gain,nq", [(3.6, 128), (3.6, 192)])
def test_restatements_are_finite_at_the_large_score_scale(gain, nq):
    """The large-score GPU cases (scores of about +-60, a -100 mask): both CPU evaluations are finite there, and the scores do
    reach that size."""
    c = AC.Case("big", 2, 2, 20, nq, nq, nq, mask="dense", nW=2, Nm=nq, qk_gain=gain, seed=9)
    qkv, dout, bias, mask = AC.make_case(c)
    s = torch.einsum("bqhd,bkhd->bhqk", qkv[:, :, 0].double() * c.scale, qkv[:, :, 1].double())
    assert 50 < float(s.abs().max()) < 90
    for r in (AC.attention_fp64(c, qkv, dout, bias, mask), AC.attention_same_precision(c, qkv, dout, bias, mask, False),
              AC.attention_same_precision(c, qkv, dout, bias, mask, True)):
        assert all(bool(torch.isfinite(v).all()) for v in r.values())


def test_host_pack_is_the_documented_bit_order():
    m = torch.zeros(1, 32, 32)
    m[0, 3, 0], m[0, 3, 5], m[0, 4, 31] = -100.0, 1e-30, -1e-40
    b = AC.host_pack(m)
    assert b[0, 3, 0] == 1 + 32 and b[0, 4, 0] == -2 ** 31 and int((b != 0).sum()) == 2
