"""What the tests of EncoderDCT / DecoderIDCT, Mlp / MixerBlock / MlpMixer and CosineAnnealingLinearWarmup share with
tests/golden/make_golden_mixer.py: the cases of tests/golden/token_mixer.npz (seeded inputs, seeded weights, configurations) and a
restatement of the three modules in plain torch.  The restatement takes any dtype; ``store=bf16_store`` emulates bf16 storage by
rounding at each fused op's boundary, forward and backward, with fp32 arithmetic in between (what the kernels do).  The host test
pins the fp64 restatement to the reference's recorded results; the GPU tests measure the kernels against it.

The record keeps a tensor of at most FULL elements whole.  A larger one is pinned as the other goldens pin theirs
(tests/helpers.py): every stride-th element, and its sum, its L2 norm and its product with a seeded random direction."""
import math

import torch
import torch.nn.functional as F

from helpers import grad_stats, rand

# ---- cases ------------------------------------------------------------------------------------------------------------------------
# (ps, b, t, h, w): a non-square block grid; 192-channel tokens; 12-channel tokens and t = 3; 67 blocks in a row; remainder rows and columns
DCT_CASES = [(4, 1, 2, 8, 12), (8, 1, 1, 8, 16), (2, 1, 3, 6, 10), (4, 1, 1, 4, 268), (4, 1, 1, 10, 9)]
# name -> (MlpMixer arguments (patches, channels, time, exp, blocks), input shape (b, t, p, c))
MIXER_CASES = {
    "fused": ((6, 48, 2, 2, 2), (1, 2, 6, 48)),        # all three axes on the fused kernel: inner = 1, 48 and 288
    "ragged": ((67, 12, 3, 3, 1), (2, 3, 67, 12)),     # outer > 1, odd D, no multiple of any tile; the patch axis on the matmul path
    "e2e": ((15, 12, 3, 2, 1), (1, 3, 15, 12)),        # EncoderDCT(2) on (1, 3, 3, 6, 10) -> mixer -> DecoderIDCT, end to end
}
E2E_CLIP, E2E_PS = (1, 3, 3, 6, 10), 2
# the expected answer of axis_mlp_is_fused per axis (channels, patches, time)
MIXER_FUSED = {"fused": (True, True, True), "ragged": (True, False, True), "e2e": (True, True, True)}
AXES = ("time", "patches", "channels")                 # the order of a block's state_dict

# scheduler cases: (constructor arguments, base rates of the param groups, the step() calls: None = step(), an int = step(epoch))
SCHEDULER_CASES = {
    "restarts": (dict(first_cycle_steps=6, min_lrs=[1e-5], cycle_mult=2, warmup_steps=2, gamma=0.5), [1e-3], [None] * 20),
    "pow_jump": (dict(first_cycle_steps=5, warmup_steps=1, min_lrs_pow=2), [2e-4], [None, None, 7, None, None]),
    "two_groups": (dict(first_cycle_steps=4, min_lrs=[1e-6, 5e-5], warmup_steps=1, gamma=0.9), [1e-3, 4e-4], [None] * 10),
    "mult_jump": (dict(first_cycle_steps=3, min_lrs=[0.0], cycle_mult=2, warmup_steps=1), [1e-2], [None, 11, None, 30, None, 2, None]),
}

FULL, SUBSAMPLES = 256, 128


def dct_inputs(i):
    """case i: clip, cotangent of its tokens, tokens for the decoder, cotangent of the decoded frames"""
    ps, b, t, h, w = DCT_CASES[i]
    P, CK = (h // ps) * (w // ps), 3 * ps * ps
    hh, ww = (h // ps) * ps, (w // ps) * ps
    return (rand(900 + i, b, t, 3, h, w), rand(910 + i, b, t, P, CK, lo=-1.0), rand(920 + i, b, t, P, CK, lo=-1.0),
            rand(930 + i, b, t, 3, hh, ww, lo=-1.0))


def mixer_shapes(args):
    """state_dict key -> shape of MlpMixer(*args), in the reference's order"""
    patches, channels, time, exp, blocks = args
    dims = {"time": time, "patches": patches, "channels": channels}
    out = {}
    for i in range(blocks):
        for axis in AXES:
            d, hid = dims[axis], exp * dims[axis]
            for layer, shape in (("0.weight", (hid, d)), ("0.bias", (hid,)), ("2.weight", (d, hid)), ("2.bias", (d,))):
                out[f"mixer.{i}.{axis}_mlp.mlp.{layer}"] = shape
    return out


def mixer_params(name):
    """seeded fp32 weights of a case: uniform within 1 / sqrt(fan_in), as nn.Linear draws them, biases included"""
    args, _ = MIXER_CASES[name]
    base = 1000 * (1 + list(MIXER_CASES).index(name))
    out = {}
    for n, (key, shape) in enumerate(mixer_shapes(args).items()):
        fan_in = shape[1] if key.endswith("0.weight") or key.endswith("2.weight") else \
            (shape[0] if key.endswith("2.bias") else None)
        if fan_in is None:                                  # 0.bias: the fan-in of its layer is the axis length = hidden / exp
            fan_in = shape[0] // args[3]
        s = 1.0 / math.sqrt(fan_in)
        out[key] = rand(base + n, *shape, lo=-s, hi=s)
    return out


def mixer_inputs(name):
    """input and cotangent of a case ('e2e': the CLIP and the cotangent of the decoded clip)"""
    base = 2000 + 10 * list(MIXER_CASES).index(name)
    shape = E2E_CLIP if name == "e2e" else MIXER_CASES[name][1]
    return rand(base, *shape, lo=-1.0), rand(base + 1, *shape, lo=-1.0)


# ---- restatement ----------------------------------------------------------------------------------------------------------------------
def bf16_store(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _Boundary(torch.autograd.Function):
    """a tensor written to storage and read back: rounded on the way forward, its gradient on the way back"""

    @staticmethod
    def forward(ctx, x, store):
        ctx.store = store
        return store(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.store(g), None


def _st(x, store):
    return x if store is None else _Boundary.apply(x, store)


def encoder(x, w, ps, store=None):
    """(b, t, c, h, w) -> (b, t, P, c ps^2); w: (c ps^2, 1, ps, ps)"""
    b, t, c, h, wd = x.shape
    y = F.conv2d(_st(x, store).reshape(b * t, c, h, wd), w, stride=ps, groups=c)
    return _st(y.permute(0, 2, 3, 1).reshape(b, t, -1, c * ps * ps), store)


def decoder(tok, w, ps, BH, BW, store=None):
    """(b, t, BH BW, c ps^2) -> (b, t, c, BH ps, BW ps)"""
    b, t, p, ck = tok.shape
    y = _st(tok, store).reshape(b * t, BH, BW, ck).permute(0, 3, 1, 2)
    x = F.conv_transpose2d(y, w, stride=ps, groups=ck // (ps * ps))
    return _st(x.reshape(b, t, -1, BH * ps, BW * ps), store)


def mlp(x, w1, b1, w2, b2):
    """the two-layer GELU MLP along the LAST axis, no residual"""
    return F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)


def axis_mlp(x, axis, w1, b1, w2, b2, store=None):
    xm = _st(x, store).movedim(axis, -1)
    return _st((xm + mlp(xm, w1, b1, w2, b2)).movedim(-1, axis), store)


def mixer(x, params, blocks, store=None):
    """(b, t, p, c) -> (b, t, p, c): per block the channel, patch and time axes in turn"""
    for i in range(blocks):
        for axis, name in ((3, "channels"), (2, "patches"), (1, "time")):
            k = f"mixer.{i}.{name}_mlp.mlp."
            x = axis_mlp(x, axis, params[k + "0.weight"], params[k + "0.bias"], params[k + "2.weight"], params[k + "2.bias"], store)
    return x


def run_mixer_case(name, dtype, w_dct=None, store=None):
    """A case on the CPU in `dtype` (weights in `dtype` too): output, d input and every parameter gradient, under the case's
    cotangent.  'e2e' needs the (3 ps^2, 1, ps, ps) transform weight."""
    args, _ = MIXER_CASES[name]
    x, cot = (t.to(dtype) for t in mixer_inputs(name))
    if store is not None:
        x, cot = store(x), store(cot)
    x.requires_grad_(True)
    params = {k: v.to(dtype).requires_grad_(True) for k, v in mixer_params(name).items()}
    if name == "e2e":
        w = w_dct.to(dtype)
        tok = encoder(x, w, E2E_PS, store)
        out = decoder(mixer(tok, params, args[4], store), w, E2E_PS, E2E_CLIP[3] // E2E_PS, E2E_CLIP[4] // E2E_PS, store)
    else:
        out = mixer(x, params, args[4], store)
    (out * cot).sum().backward()
    return out.detach(), x.grad, {k: v.grad for k, v in params.items()}


def run_dct_case(i, dtype, w3, store=None):
    """case i on the CPU in `dtype`: encoder output, d clip, decoder output, d tokens; w3: (3 ps^2, 1, ps, ps)"""
    ps, b, t, h, w = DCT_CASES[i]
    x, cy, tok, cx = (v.to(dtype) for v in dct_inputs(i))
    if store is not None:
        x, cy, tok, cx = (store(v) for v in (x, cy, tok, cx))
    x.requires_grad_(True), tok.requires_grad_(True)
    w3 = w3.to(dtype)
    y = encoder(x, w3, ps, store)
    (y * cy).sum().backward()
    img = decoder(tok, w3, ps, h // ps, w // ps, store)
    (img * cx).sum().backward()
    return {"enc_out": y.detach(), "enc_dx": x.grad, "dec_out": img.detach(), "dec_dtok": tok.grad}


def scheduler_sequence(cls, name):
    """the rates of every param group after construction and after each call of the case: (calls + 1, groups)"""
    kwargs, rates, calls = SCHEDULER_CASES[name]
    opt = torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr} for lr in rates], lr=rates[0])
    sched = cls(opt, **kwargs)
    rows = [[g["lr"] for g in opt.param_groups]]
    for epoch in calls:
        opt.step()
        sched.step() if epoch is None else sched.step(epoch)
        rows.append([g["lr"] for g in opt.param_groups])
    return rows, opt


# ---- the record -----------------------------------------------------------------------------------------------------------------------
def sub_stride(numel):
    return -(-numel // SUBSAMPLES)


def put(store, key, t):
    import numpy as np
    t = t.detach().double()
    if t.numel() <= FULL:
        store[key] = t.numpy().astype(np.float64)
    else:
        store["sub__" + key] = t.flatten()[::sub_stride(t.numel())].numpy().astype(np.float64)
        store["stats__" + key] = grad_stats("mixer." + key, t).numpy()


def golden_mismatch(gold, key, t):
    """the largest deviation of the fp64 tensor `t` from what the record holds under `key`, relative to the record's scale"""
    t = t.detach().double()
    if key in gold:
        want = gold[key]
        assert want.shape == t.shape, (key, want.shape, t.shape)
        return float((t - want).abs().max() / want.abs().max().clamp_min(1e-300))
    sub, stats = gold["sub__" + key], gold["stats__" + key]
    got = t.flatten()[::sub_stride(t.numel())]
    assert got.shape == sub.shape, (key, got.shape, sub.shape)
    e_sub = float((got - sub).abs().max() / sub.abs().max().clamp_min(1e-300))
    # sum, norm and projection, each relative to the norm (a sum may cancel)
    e_stats = float((grad_stats("mixer." + key, t) - stats).abs().max() / stats[1].clamp_min(1e-300))
    return max(e_sub, e_stats)
