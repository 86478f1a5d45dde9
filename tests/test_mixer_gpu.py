"""GPU checks of the DCT-token MLP-Mixer (csrc/token_mixer.hip through core/token_ops.py and the modules) against the fp64 results
of the reference: the restatement of tests/mixer_common.py in fp64, which tests/test_mixer_host.py pins to the reference's record
(tests/golden/token_mixer.npz) to 1e-12.

The criterion is the project's own (smoke(), tests/test_hip_parity.py): relative L2 against the fp64 result; the HIP result's error
may not exceed 1.5 x the error of a CPU evaluation at the same precision against the same fp64 result -- the restatement in fp32, or
in fp32 with bf16 storage emulated at every fused op's boundary.  A floor keeps a luckily exact CPU run from failing a correct
kernel: fp32 sqrt(K) 2^-24, the random-walk rounding of a K-term fp32 sum, with K the longest dot product of the case (transforms:
ps^2; Mixer: the longest of an axis, its hidden width, and the positions a weight gradient sums over); bf16 2^-9, one storage
rounding.  A gradient that is identically zero in fp64 must be exactly zero.  Every figure is printed before it is asserted."""
import math

import pytest
import torch

import mixer_common as MC
from helpers import golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def gold():
    return golden("token_mixer")


def _w3(gold, ps):
    return torch.cat([gold[f"weight_ps{ps}"]] * 3, dim=0)


_refs = {}


def _cpu(kind, key, tag, gold):
    """fp64 result, and the CPU evaluation at the precision `tag`, of a case: computed once and shared, never modified"""
    if (kind, key, tag) not in _refs:
        dtype, store = {"fp64": (torch.float64, None), "fp32": (torch.float32, None), "bf16": (torch.float32, MC.bf16_store)}[tag]
        if kind == "dct":
            _refs[kind, key, tag] = MC.run_dct_case(key, dtype, _w3(gold, MC.DCT_CASES[key][0]), store)
        else:
            out, dx, grads = MC.run_mixer_case(key, dtype, _w3(gold, MC.E2E_PS), store)
            _refs[kind, key, tag] = {"out": out, "dx": dx, **{"grad " + k: g for k, g in grads.items()}}
    return _refs[kind, key, tag]


def _floor(tag, K):
    return math.sqrt(K) * 2.0 ** -24 if tag == "fp32" else 2.0 ** -9


def _judge(what, got, ref, cpu, floor):
    """the criterion of the module docstring for one tensor"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not ref.any():
        print(f"{what}: identically zero")
        assert not got.any(), what
        return
    e_hip, e_cpu = rel_l2(got, ref), rel_l2(cpu, ref)
    print(f"{what}: HIP rel-L2 {e_hip:.3e}, CPU at this precision {e_cpu:.3e}, floor {floor:.3e}")
    assert e_hip <= 1.5 * max(e_cpu, floor), (what, e_hip, e_cpu, floor)
    zero = ref == 0
    if zero.any():                                      # e.g. the remainder rows and columns of the adjoint
        assert not got.cpu()[zero].any(), what


def _transforms(gold, ps, h, w):
    from vsrlab_amd.core.modules.dct_transforms import DecoderIDCT, EncoderDCT
    enc, dec = EncoderDCT(ps), DecoderIDCT(3, ps, h, w)
    enc.load_state_dict({"dct_conv.weight": _w3(gold, ps)})             # the reference's weight, as a checkpoint brings it
    dec.load_state_dict({"reverse_dct.weight": _w3(gold, ps)})
    return enc.to(DEV), dec.to(DEV)


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("i", range(len(MC.DCT_CASES)))
def test_transforms_match_the_reference(gold, i, tag):
    ps, b, t, h, w = MC.DCT_CASES[i]
    enc, dec = _transforms(gold, ps, h, w)
    assert enc.dct_conv.weight.dtype == torch.float32
    x, cy, tok, cx = (v.to(DEV).to(DTYPES[tag]) for v in MC.dct_inputs(i))
    x.requires_grad_(True), tok.requires_grad_(True)
    y = enc(x)
    assert y.dtype == x.dtype and tuple(y.shape) == (b, t, (h // ps) * (w // ps), 3 * ps * ps) and y.is_contiguous()
    (y * cy).sum().backward()
    img = dec(tok)
    assert img.dtype == tok.dtype and tuple(img.shape) == (b, t, 3, (h // ps) * ps, (w // ps) * ps)
    (img * cx).sum().backward()
    got = {"enc_out": y.detach(), "enc_dx": x.grad, "dec_out": img.detach(), "dec_dtok": tok.grad}
    ref, cpu = _cpu("dct", i, "fp64", gold), _cpu("dct", i, tag, gold)
    for k in got:
        _judge(f"dct{i} {tag} {k}", got[k], ref[k], cpu[k], _floor(tag, ps * ps))
    # the round trip: the basis is orthonormal, so the decoder gives the clip back (its whole blocks)
    with torch.no_grad():
        back = dec(enc(x))
        x64 = x.detach().cpu().double()                 # the clip as it is stored
        w3 = _w3(gold, ps)
        store = MC.bf16_store if tag == "bf16" else None
        cpu_back = MC.decoder(MC.encoder(x.detach().cpu().float(), w3, ps, store), w3, ps, h // ps, w // ps, store)
    crop = x64[..., :(h // ps) * ps, :(w // ps) * ps]
    _judge(f"dct{i} {tag} round trip", back, crop, cpu_back, _floor(tag, ps * ps))
    if tag == "fp32":
        print(f"dct{i} round trip max abs err {float((back.cpu().double() - crop).abs().max()):.3e}")


def _mixer_K(name):
    (patches, channels, time, exp, _), shape = MC.MIXER_CASES[name]
    numel = math.prod(shape)
    return max(max(d * exp, numel // d) for d in (patches, channels, time))


def _run_mixer(gold, name, tag):
    from vsrlab_amd.core.modules.mlp import MlpMixer
    args, shape = MC.MIXER_CASES[name]
    model = MlpMixer(*args)
    model.load_state_dict(MC.mixer_params(name), strict=True)
    model = model.to(DEV)
    x, cot = (v.to(DEV).to(DTYPES[tag]) for v in MC.mixer_inputs(name))
    x.requires_grad_(True)
    if name == "e2e":
        enc, dec = _transforms(gold, MC.E2E_PS, *MC.E2E_CLIP[3:])
        tok = enc(x)
        assert tuple(tok.shape) == shape
        out = dec(model(tok))
    else:
        out = model(x)
        assert out.is_contiguous()
    assert out.dtype == x.dtype and out.shape == x.shape
    (out * cot).sum().backward()
    assert all(p.grad.dtype == torch.float32 for p in model.parameters())
    return {"out": out.detach(), "dx": x.grad, **{"grad " + k: p.grad for k, p in model.named_parameters()}}


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("name", list(MC.MIXER_CASES))
def test_mixer_matches_the_reference(gold, name, tag):
    from vsrlab_amd.core.token_ops import axis_mlp_is_fused
    patches, channels, time, exp, blocks = MC.MIXER_CASES[name][0]
    # which path each axis takes, first: no case can pass by silently taking the other one
    assert tuple(axis_mlp_is_fused(d, exp * d) for d in (channels, patches, time)) == MC.MIXER_FUSED[name]
    got = _run_mixer(gold, name, tag)
    ref, cpu = _cpu("mixer", name, "fp64", gold), _cpu("mixer", name, tag, gold)
    assert set(got) == set(ref) and len(got) == 2 + 12 * blocks
    for k in got:
        _judge(f"{name} {tag} {k}", got[k], ref[k], cpu[k], _floor(tag, _mixer_K(name)))
    again = _run_mixer(gold, name, tag)                 # no atomics: the same bits from run to run
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("tag", list(DTYPES))
def test_mlp_mixes_the_last_axis_without_a_residual(tag):
    """the reference's Mlp.forward; 144 hidden units = four and a half weight chunks, 201 tokens = one and a half workgroups"""
    from vsrlab_amd.core.modules.mlp import Mlp
    torch.manual_seed(5)
    m = Mlp(48, 144)
    x, cot = MC.rand(3001, 3, 67, 48, lo=-1.0), MC.rand(3002, 3, 67, 48, lo=-1.0)
    p = [m.mlp[0].weight, m.mlp[0].bias, m.mlp[2].weight, m.mlp[2].bias]

    def cpu(dtype, store):
        xs, cs = (store(v) if store else v.clone() for v in (x.to(dtype), cot.to(dtype)))
        xs.requires_grad_(True)
        ws = [v.detach().to(dtype).requires_grad_(True) for v in p]
        y = MC._st(MC.mlp(MC._st(xs, store), *ws), store)
        (y * cs).sum().backward()
        return [y.detach(), xs.grad] + [v.grad for v in ws]

    ref = cpu(torch.float64, None)
    same = cpu(torch.float32, MC.bf16_store if tag == "bf16" else None)
    m = m.to(DEV)
    xg = x.to(DEV).to(DTYPES[tag]).detach().requires_grad_(True)
    y = m(xg)
    (y * cot.to(DEV).to(DTYPES[tag])).sum().backward()
    got = [y.detach(), xg.grad] + [q.grad for q in (m.mlp[0].weight, m.mlp[0].bias, m.mlp[2].weight, m.mlp[2].bias)]
    for k, g, r, c in zip(("out", "dx", "dw1", "db1", "dw2", "db2"), got, ref, same):
        _judge(f"mlp {tag} {k}", g, r, c, _floor(tag, 201))


@pytest.mark.parametrize("shape,axis", [((16500, 8), 1), ((3, 8, 5500), 1)])
def test_axis_mlp_with_more_position_tiles_than_workgroups(shape, axis):
    """16,500 positions are 258 tiles of 64 for the weight gradients, which at most 256 workgroups walk: two of them take a second
    tile; staged (inner = 1) and along inner.  K = 16,500, the positions a weight gradient sums over."""
    from vsrlab_amd.core.token_ops import axis_mlp
    x, cot = MC.rand(3101, *shape, lo=-1.0), MC.rand(3102, *shape, lo=-1.0)
    ws = [MC.rand(3103, 16, 8, lo=-0.35, hi=0.35), MC.rand(3104, 16, lo=-0.35, hi=0.35), MC.rand(3105, 8, 16, lo=-0.25, hi=0.25),
          MC.rand(3106, 8, lo=-0.25, hi=0.25)]

    def run(fn, dtype, dev):
        leaves = [v.to(dtype).to(dev).clone().requires_grad_(True) for v in [x] + ws]
        y = fn(leaves[0], axis, *leaves[1:])
        (y * cot.to(dtype).to(dev)).sum().backward()
        return [y.detach()] + [v.grad for v in leaves]

    ref, same = run(MC.axis_mlp, torch.float64, "cpu"), run(MC.axis_mlp, torch.float32, "cpu")
    got = run(axis_mlp, torch.float32, DEV)
    for k, g, r, c in zip(("out", "dx", "dw1", "db1", "dw2", "db2"), got, ref, same):
        _judge(f"many positions {shape} {k}", g, r, c, _floor("fp32", 16500))
    again = run(axis_mlp, torch.float32, DEV)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_refusals_on_the_gpu():
    from vsrlab_amd.core.modules.dct_transforms import EncoderDCT
    from vsrlab_amd.core.modules.mlp import Mlp
    enc = EncoderDCT(4).to(DEV)
    x = torch.rand(1, 1, 3, 8, 8, device=DEV, requires_grad=True)
    y = enc(x)
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad(y.sum(), x, create_graph=True)
    enc.dct_conv.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="frozen"):
        enc(x)
    m = Mlp(8, 16).to(DEV)
    z = m(torch.rand(4, 8, device=DEV, requires_grad=True))
    with pytest.raises(RuntimeError, match="no double backward"):
        torch.autograd.grad(z.sum(), m.mlp[0].weight, create_graph=True)
