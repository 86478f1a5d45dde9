"""GPU tests of csrc/window_attention.hip against an fp64 restatement, one descriptor at a time through the C ABI
(tests/attention_common.py), at every shape the launch code accepts.

Criterion.  For each of out, lse, dq, dk, dv, dbias the HIP result and a same-precision CPU-style evaluation of the same formula
(fp32, with bf16 roundings at the kernels' storage points for the bf16 build) are both compared with the fp64 restatement.  HIP's
relative-L2 error may exceed max(same-precision error, floor) by at most 1.5 over all tensors concatenated and 2.5 per tensor
(test_hip_parity._noise_floor_check; floors 2e-4 fp32, 1e-3 bf16); the same 2.5 holds for the worst query row (max|err| of a row
over max|ref| of the tensor), which one wrong mask bit or one wrong row moves and relative L2 dilutes; the fp32 build stays under
1e-3 in that measure whatever is measured.  profiles/attention_parity.md records the figures each case printed.

Which test launches which kernel template (both element types each):
  attn_fwd_p / attn_bwd_q_p / attn_bwd_kv_p <NT 8> : test_shape_matrix[p128-*], test_deep_walk[128], test_large_scores[p128], autograd N 256
  attn_fwd_p / attn_bwd_q_p / attn_bwd_kv_p <NT 4> : test_shape_matrix[p64-*], test_deep_walk[64], autograd mask identity
  attn_fwd / attn_bwd_q <NT 4>  : test_shape_matrix[g4-*]          attn_fwd / attn_bwd_q <NT 8>  : test_shape_matrix[g8-*]
  attn_fwd / attn_bwd_q <NT 12> : test_shape_matrix[g12-*], test_large_scores[g12], autograd N 192 / 384 mutual
  attn_fwd / attn_bwd_q <NT 16> : test_shape_matrix[g16-*], autograd N 256     attn_fwd / attn_bwd_q <NT 24> : test_shape_matrix[g24-*]
  attn_bwd_kv (one template for every key count): every g* case; chunks of 32, 64, 96 (one and two), 128 (one, two, three)."""

import pytest
import torch

import attention_common as AC
from attention_common import Case

pytestmark = pytest.mark.gpu

FLOOR = {"fp32": 2e-4, "bf16": 1e-3}
RATIO_GLOBAL, RATIO_TENSOR = 1.5, 2.5
DTYPES = ["fp32", "bf16"]


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _criterion(name, dtype, hip, emu, ref, keys=None):
    """Prints every figure, then asserts."""
    from test_hip_parity import _noise_floor_check
    keys = sorted(ref) if keys is None else keys
    assert set(keys) <= set(hip) and set(keys) <= set(emu)
    floor = FLOOR[dtype]
    rows = []
    for k in keys:
        assert hip[k].shape == ref[k].shape == emu[k].shape, (k, hip[k].shape, ref[k].shape)
        rows.append((k, AC.rel_l2(hip[k], ref[k]), AC.rel_l2(emu[k], ref[k]), AC.worst_row(hip[k], ref[k]), AC.worst_row(emu[k], ref[k])))
    for k, eh, ee, rh, re_ in rows:
        print(f"ATTN_PARITY {name} {dtype} {k} l2_hip {eh:.3e} l2_same {ee:.3e} ratio {eh / max(ee, floor):.2f} "
              f"row_hip {rh:.3e} row_same {re_:.3e} ratio {rh / max(re_, floor):.2f}")
    for k in keys:
        assert bool(torch.isfinite(hip[k]).all()), (name, dtype, k, "not finite")
    sub = lambda d: {k: d[k] for k in keys}
    _noise_floor_check(sub(hip), sub(emu), sub(ref), max_glob_ratio=RATIO_GLOBAL, max_tensor_ratio=RATIO_TENSOR, floor=floor)
    for k, eh, ee, rh, re_ in rows:
        assert rh <= RATIO_TENSOR * max(re_, floor), (name, dtype, k, "worst row", rh, re_)
        if dtype == "fp32":
            assert rh < 1e-3, (name, k, rh)


def _run_case(c, dtype, dev):
    qkv, dout, bias, mask = AC.make_case(c)
    hip = AC.run_hip(c, qkv, dout, bias, mask, dtype, dev)
    on = lambda t: t.to(dev) if t is not None else None
    ref = {k: v.cpu() for k, v in AC.attention_fp64(c, on(qkv), on(dout), on(bias), on(mask)).items()}
    emu = {k: v.cpu() for k, v in AC.attention_same_precision(c, on(qkv), on(dout), on(bias), on(mask), dtype == "bf16").items()}
    assert set(hip) == set(ref)
    _criterion(c.name, dtype, hip, emu, ref)
    return hip, ref


# --------------------------------------------------------------------------------------------------------------------
# (a) the shape matrix
# --------------------------------------------------------------------------------------------------------------------
#          name                  B heads hd   N   Nq   Nk   q0   k0   o0
MATRIX = [
    Case("p128-packed-nw3",      6, 3, 20, 128, 128, 128,   0,   0,   0, mask="packed", nW=3, Nm=128, wide=True),
    Case("p128-hd32-nonbinary",  5, 1, 32, 128, 128, 128,   0,   0,   0, mask="nonbinary", nW=2, Nm=128),
    Case("p128-q128-hd8",        9, 6,  8, 256, 128, 128, 128,   0,   0, mask="dense", nW=3, Nm=256, wide=True),
    Case("p128-k128-hd8",        1, 3,  8, 256, 128, 128,   0, 128, 128, mask="dense", nW=1, Nm=256),
    Case("p64-q64-hd30-packed",  9, 3, 30, 128,  64,  64,  64,   0,   0, mask="packed", nW=3, Nm=128, wide=True),
    Case("p64-k64-hd30-packed",  5, 6, 30, 128,  64,  64,   0,  64,  64, mask="packed", nW=5, Nm=128),
    Case("p64-hd4-rowmasked",    6, 6,  4,  64,  64,  64,   0,   0,   0, mask="rowmasked", nW=2, Nm=64, wide=True),
    Case("g4-nq128",             5, 3, 20, 128, 128,  64,   0,  64,   0, mask="dense", nW=5, Nm=128, wide=True),
    Case("g4-qc96",              1, 6, 30, 160,  96,  64,  64,   0,  32),
    Case("g8-nq64-hd32",         6, 1, 32, 192,  64, 128, 128,   0,  64, mask="dense", nW=2, Nm=192, wide=True),
    Case("g8-two-waves",         9, 3, 20, 160,  32, 128, 128,   0,   0),
    Case("g12-q192-hd30",        5, 1, 30, 384, 192, 192, 192,   0,   0, mask="dense", nW=1, Nm=384, wide=True),
    Case("g12-self-192",         6, 3, 20, 192, 192, 192,   0,   0,   0, mask="dense", nW=2, Nm=192),
    Case("g16-two-chunks",       6, 1, 20, 256, 256, 256,   0,   0,   0, mask="dense", nW=3, Nm=256, wide=True),
    Case("g24-three-chunks",     1, 3,  8, 384, 384, 384,   0,   0,   0, mask="nonbinary", nW=1, Nm=384),
    # added from reading the code: the module's mutual attention has NO bias (the `a.bias` / `a.dbias` null arms of the persistent
    # kernels), and a head_dim of 2 is less than one vector
    Case("p64-nobias-hd2",       5, 6,  2, 128,  64,  64,  64,   0,   0, mask="packed", nW=5, Nm=128, wide=True, bias=False),
]
for _i, _c in enumerate(MATRIX):
    _c.seed = _i


def test_the_matrix_is_the_one_the_kernels_need():
    assert {c.B for c in MATRIX} == {1, 5, 6, 9} and {c.heads for c in MATRIX} == {1, 3, 6}
    assert 2 * sum(c.c_off > 0 and c.Cout > c.C for c in MATRIX) >= len(MATRIX)
    assert {c.Nk for c in MATRIX if not c.persistent} == {64, 128, 192, 256, 384}
    assert {c.Nk for c in MATRIX if c.persistent} == {64, 128}
    assert {c.hd for c in MATRIX} >= {2, 4, 8, 20, 30, 32}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", MATRIX, ids=[c.name for c in MATRIX])
def test_shape_matrix(c, dtype):
    _run_case(c, dtype, _gpu())


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_accepts_nq_160(dtype):
    """Nq = 160 has no key-stationary chunking (the backward refuses it, test_attention_host.py) but the forward takes it: ten
    blocks of 16 queries over eight waves, so two waves make a second trip."""
    dev = _gpu()
    c = Case("g8-fwd-nq160", 5, 3, 20, 192, 160, 128, 32, 64, 0, mask="dense", nW=2, Nm=192, wide=True, seed=40)
    qkv, dout, bias, mask = AC.make_case(c)
    hip = AC.run_hip(c, qkv, dout, bias, mask, dtype, dev, backward=False)
    ref = AC.attention_fp64(c, qkv, dout, bias, mask, backward=False)
    emu = AC.attention_same_precision(c, qkv, dout, bias, mask, dtype == "bf16")
    _criterion(c.name, dtype, hip, emu, ref, keys=["lse", "out"])


# --------------------------------------------------------------------------------------------------------------------
# (b) the persistent kernels' steady state
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [128, 64])
def test_deep_walk(n, dtype):
    """Every workgroup of the persistent kernels walks three or four windows (both LDS buffers reused, a ragged tail), each window
    with its own random data.  (1) out, lse, dq, dk, dv equal, bit for bit, the same data run in slices of six windows, where no
    workgroup sees a second window; (2) dbias, summed in registers over a workgroup's windows and flushed once, meets the criterion
    against the fp64 restatement over all windows."""
    dev = _gpu()
    heads, hd, nW = 32, 4, 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = n // 16                                          # launch_attn_p: one wave per block of 16 queries
    per_cu = 2048 // (waves * 64)
    pp = max(1, (cus * per_cu) // (8 * heads))
    B = 3 * 8 * pp + 5
    pp = max(1, min(pp, (B + 7) // 8))
    nparts = 8 * pp
    assert B > 2 * nparts and B % nparts != 0 and B < 4 * nparts
    c = Case(f"deep{n}", B, heads, hd, n, n, n, mask="packed", nW=nW, Nm=n, wide=True, seed=50 + n)
    qkv, dout, bias, mask = AC.make_case(c)
    deep = AC.run_hip(c, qkv, dout, bias, mask, dtype, dev)
    step = 6
    assert step % nW == 0 and (step + 7) // 8 == 1           # slice starts keep the mask phase; 8 partitions for <= 8 windows
    parts = []
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        s = Case(f"slice{b0}", b1 - b0, heads, hd, n, n, n, mask="packed", nW=nW, Nm=n, wide=True)
        parts.append(AC.run_hip(s, qkv[b0:b1], dout[b0:b1], bias, mask, dtype, dev))
    for k in ("out", "lse", "dq", "dk", "dv"):
        sliced = torch.cat([p[k] for p in parts])
        same = (deep[k] == sliced) | (deep[k].isnan() & sliced.isnan())
        bad = sorted(set((~same).nonzero()[:, 0].tolist()))
        assert not bad, (k, "windows that differ between the deep walk and the slices", bad[:16], "nparts", nparts)
    on = lambda t: t.to(dev)
    ref = AC.attention_fp64(c, on(qkv), on(dout), on(bias), on(mask))
    emu = AC.attention_same_precision(c, on(qkv), on(dout), on(bias), on(mask), dtype == "bf16")
    cpu = lambda d: {k: v.cpu() for k, v in d.items()}
    _criterion(c.name, dtype, deep, cpu(emu), cpu(ref))


# --------------------------------------------------------------------------------------------------------------------
# (c) large scores
# --------------------------------------------------------------------------------------------------------------------
BIG = [Case("big-p128", 5, 3, 20, 128, 128, 128, mask="dense", nW=5, Nm=128, qk_gain=3.6, seed=60),
       Case("big-g12", 5, 3, 20, 192, 192, 192, mask="dense", nW=5, Nm=192, wide=True, qk_gain=3.6, seed=61)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", BIG, ids=[c.name for c in BIG])
def test_large_scores(c, dtype):
    """q and k scaled so that the unmasked scores span about +-60, with a -100 mask: the forward subtracts the row maximum once and
    never rescales.  (test_attention_host.py checks that both CPU evaluations are finite at this scale.)"""
    qkv = AC.make_case(c)[0]
    s = torch.einsum("bqhd,bkhd->bhqk", qkv[:, :, 0].double() * c.scale, qkv[:, :, 1].double())
    assert float(s.max()) > 45 and float(s.min()) < -45
    hip, _ = _run_case(c, dtype, _gpu())                     # asserts finiteness of every tensor before the criterion


# --------------------------------------------------------------------------------------------------------------------
# (d) through autograd: window_attention_core
# --------------------------------------------------------------------------------------------------------------------
def _module_eval(fn, N, B, heads, hd, mut, qs, qm, cot, table, index, mask, table_dtype):
    """[mutual | self] as functional._WindowAttentionFn issues it, each descriptor evaluated by ``fn`` (attention_fp64: autograd on
    the restatement; attention_same_precision).  Returns out, d qkv_self, d qkv_mut, d table."""
    C = heads * hd
    nW, Nm = mask.shape[0], mask.shape[1]
    bias = table.to(table_dtype)[index.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1).contiguous()
    out = torch.zeros(B, N, 2 * C if mut else C, dtype=table_dtype, device=qs.device)
    c = Case("self", B, heads, hd, N, N, N, nW=nW, Nm=Nm, wide=mut)
    r = fn(c, qs.view(B, N, 3, heads, hd), cot, bias, mask)
    out[:, :, c.c_off:c.c_off + C] = r["out"]
    dqs = torch.stack([r["dq"], r["dk"], r["dv"]], dim=2).reshape(B, N, 3 * C)
    dtable = torch.zeros(table.shape, dtype=table_dtype, device=qs.device)
    dtable.index_add_(0, index.reshape(-1), r["dbias"].to(table_dtype).permute(1, 2, 0).reshape(N * N, heads))
    dqm = None
    if mut:
        h2 = N // 2
        dqm = torch.zeros(B, N, 3, heads, hd, dtype=table_dtype, device=qs.device)
        for q0, k0, o0 in ((h2, 0, 0), (0, h2, h2)):
            cm = Case("mut", B, heads, hd, N, h2, h2, q0, k0, o0, nW=nW, Nm=Nm, bias=False)
            r = fn(cm, qm.view(B, N, 3, heads, hd), cot[:, :, :C], None, mask)
            out[:, o0:o0 + h2, :C] = r["out"]
            dqm[:, q0:q0 + h2, 0] = r["dq"]
            dqm[:, k0:k0 + h2, 1] = r["dk"]
            dqm[:, k0:k0 + h2, 2] = r["dv"]
        dqm = dqm.reshape(B, N, 3 * C)
    res = {"out": out, "dqkv_self": dqs, "dtable": dtable}
    if mut:
        res["dqkv_mut"] = dqm
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ws,mut", [((3, 8, 8), False), ((4, 8, 8), False), ((4, 8, 8), True), ((6, 8, 8), True)],
                         ids=["n192-self", "n256-self", "n256-mutual", "n384-mutual"])
def test_window_attention_core_autograd(ws, mut, dtype):
    """The path users take: window_attention_core with a NON-binary mask (so _packed_mask must return no bits and the persistent
    kernels of N 256's mutual attention run their dense-mask arm): out, d qkv_self, d qkv_mut and d table against autograd on the
    fp64 restatement."""
    dev = _gpu()
    from vsrlab_amd import functional as VF
    from vsrlab_amd.vsr.models.VRT.modules.window_attention import WindowAttention
    heads, hd, nW = 3, 20, 2
    B, N, C = 2 * nW, ws[0] * ws[1] * ws[2], heads * hd
    g = torch.Generator().manual_seed(70 + N + int(mut))
    rnd = lambda *s: AC.bf16_round(torch.randn(*s, generator=g)).to(dev)
    qs, qm = rnd(B, N, 3 * C).requires_grad_(True), (rnd(B, N, 3 * C).requires_grad_(True) if mut else None)
    cot = rnd(B, N, 2 * C if mut else C)
    table = (0.5 * torch.randn((2 * ws[0] - 1) * (2 * ws[1] - 1) * (2 * ws[2] - 1), heads, generator=g)).to(dev).requires_grad_(True)
    index = WindowAttention.get_position_index(ws).to(dev)
    mask = (-3.0 * torch.rand(nW, N, N, generator=g)).to(dev)
    assert VF._packed_mask(mask)[1] is None
    out = VF.window_attention_core(qs, qm, table, index, mask, heads, hd ** -0.5, dtype)
    (out * cot).sum().backward()
    hip = {"out": out.detach().cpu(), "dqkv_self": qs.grad.cpu(), "dtable": table.grad.cpu()}
    if mut:
        hip["dqkv_mut"] = qm.grad.cpu()
    args = (N, B, heads, hd, mut, qs.detach(), qm.detach() if mut else None, cot, table.detach(), index, mask)
    ref = _module_eval(AC.attention_fp64, *args, torch.float64)
    emu = _module_eval(lambda c, *a: AC.attention_same_precision(c, *a, dtype == "bf16"), *args, torch.float32)
    _criterion(f"core-n{N}-{'mut' if mut else 'self'}", dtype, hip, emu, ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_attention_core_mask_forms_agree(dtype):
    """One call with compute_mask's own tensor and one with a non-contiguous fp64 view of the same values: the cache key of
    _packed_mask and its fp32 copy.  Both must pack, and agree bit for bit."""
    dev = _gpu()
    from oracle import vrt_attention_oracle as V
    from vsrlab_amd import functional as VF
    heads, hd, N = 3, 20, 128
    C = heads * hd
    mask = V.compute_mask(4, 16, 16, (2, 8, 8), (1, 4, 4)).to(dev)
    nW = mask.shape[0]
    B = 2 * nW
    wide = torch.zeros(nW, N, 2 * N, dtype=torch.float64, device=dev)
    wide[:, :, ::2] = mask
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and torch.equal(view.float(), mask)
    assert VF._packed_mask(mask)[1] is not None and VF._packed_mask(view)[1] is not None
    assert torch.equal(VF._packed_mask(mask)[1], VF._packed_mask(view)[1]) and VF._packed_mask(view)[2] == -100.0
    g = torch.Generator().manual_seed(80)
    qs0, qm0 = AC.bf16_round(torch.randn(B, N, 3 * C, generator=g)).to(dev), AC.bf16_round(torch.randn(B, N, 3 * C, generator=g)).to(dev)
    cot = AC.bf16_round(torch.randn(B, N, 2 * C, generator=g)).to(dev)
    table0 = torch.randn(3 * 15 * 15, heads, generator=g).to(dev)
    index = torch.randint(0, 3 * 15 * 15, (N, N), generator=g).to(dev)
    got = []
    for m in (mask, view):
        qs, qm, table = qs0.clone().requires_grad_(True), qm0.clone().requires_grad_(True), table0.clone().requires_grad_(True)
        out = VF.window_attention_core(qs, qm, table, index, m, heads, hd ** -0.5, dtype)
        (out * cot).sum().backward()
        got.append((out.detach(), qs.grad, qm.grad))
    for a, b in zip(*got):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------------------
# (e) helpers
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nW", [1, 5])
@pytest.mark.parametrize("Nm", [32, 128, 384])
def test_mask_pack_equals_host_packing(Nm, nW):
    """bit = entry != 0, exactly: the non-zeros include -100, tiny normal values of both signs; the zeros include -0.0."""
    dev = _gpu()
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    g = torch.Generator().manual_seed(90 + Nm + nW)
    values = torch.tensor([0.0, -0.0, -100.0, 1.2e-38, -1.2e-38, 1e-30, -3.0, 0.0])
    assert int((values != 0).sum()) == 5
    mask = values[torch.randint(0, len(values), (nW, Nm, Nm), generator=g)]
    _, d_mask = AC._guarded(tuple(mask.shape), torch.float32, dev, float("nan"))
    d_mask.copy_(mask)
    buf, bits = AC._guarded((nW, Nm, Nm // 32), torch.int32, dev, 0x5a5a5a5a)
    assert _lib.load().vsr_mask_pack(VF._ptr(d_mask), VF._ptr(bits), nW, Nm, VF._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits.cpu(), AC.host_pack(mask))
    bits.fill_(0x5a5a5a5a)
    assert bool((buf == 0x5a5a5a5a).all()), "vsr_mask_pack wrote outside its words"


def test_rpb_gather_and_scatter_with_a_row_stride():
    """idx_stride > N: the first 128 rows and columns of the (6,8,8) window's 384 x 384 index, handed over in place (heavy
    duplication: 675 distinct offsets for 16384 pairs).  Gather is exact; scatter against index_add_ in fp64, within the
    rounding of an fp32 sum of that many terms in any order (n * 2^-24 * sum|x| per table row)."""
    dev = _gpu()
    from vsrlab_amd import _lib
    from vsrlab_amd import functional as VF
    from vsrlab_amd.vsr.models.VRT.modules.window_attention import WindowAttention
    lib = _lib.load()
    heads, N, ws = 3, 128, (6, 8, 8)
    full = WindowAttention.get_position_index(ws).contiguous()
    T = (2 * ws[0] - 1) * (2 * ws[1] - 1) * (2 * ws[2] - 1)
    idx = full[:N, :N]
    assert full.shape == (384, 384) and len(idx.unique()) == 3 * 15 * 15
    g = torch.Generator().manual_seed(95)
    table, ddense = torch.randn(T, heads, generator=g), torch.randn(heads, N, N, generator=g)
    d_full, d_table, d_ddense = full.to(dev), table.to(dev), ddense.to(dev)
    buf, dense = AC._guarded((heads, N, N), torch.float32, dev, AC.SENTINEL)
    assert lib.vsr_rpb_gather(VF._ptr(d_table), VF._ptr(d_full), 384, VF._ptr(dense), heads, N, VF._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dense.cpu(), table[idx.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1))
    dense.fill_(AC.SENTINEL)
    assert bool((buf == AC.SENTINEL).all())

    buf, dtable = AC._guarded((T, heads), torch.float32, dev, AC.SENTINEL)
    dtable.fill_(1.0)                                        # the adjoint ACCUMULATES; rows no pair refers to stay exactly 1
    assert lib.vsr_rpb_scatter(VF._ptr(d_ddense), VF._ptr(d_full), 384, VF._ptr(dtable), heads, N, VF._stream()) == 0
    torch.cuda.synchronize()
    src = ddense.permute(1, 2, 0).reshape(N * N, heads).double()
    want = torch.ones(T, heads, dtype=torch.float64).index_add_(0, idx.reshape(-1), src)
    mag = torch.ones(T, heads, dtype=torch.float64).index_add_(0, idx.reshape(-1), src.abs())
    cnt = torch.ones(T, dtype=torch.float64).index_add_(0, idx.reshape(-1), torch.ones(N * N, dtype=torch.float64))
    got = dtable.cpu().double()
    assert bool(((got - want).abs() <= cnt[:, None] * 2.0 ** -24 * mag).all()), float(((got - want).abs() / mag).max())
    unused = cnt == 1
    assert int(unused.sum()) == T - 3 * 15 * 15 and bool((got[unused] == 1.0).all())
    dtable.fill_(AC.SENTINEL)
    assert bool((buf == AC.SENTINEL).all())
