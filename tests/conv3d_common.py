"""What the tests of the strided Conv3d (csrc/conv3d.hip), ConvST / ConvSTBlock, PixelShufflePack3D and VRT's Upsample share with
tests/golden/make_golden_conv3d.py: the cases of tests/golden/conv3d.npz (seeded inputs, seeded weights, configurations) and a
restatement of the op and the four modules in plain torch.  The restatement takes any dtype; ``store=bf16_store`` emulates bf16
storage by rounding at each launch boundary, forward and backward, with fp32 arithmetic in between (what the kernels do).  The host
test pins the fp64 restatement to the reference's recorded results; the GPU tests measure the kernels against it.

The record keeps a tensor of at most mixer_common.FULL elements whole and a larger one as a sub-sample plus three statistics."""
import math

import torch
import torch.nn.functional as F

from helpers import rand
from mixer_common import _st, bf16_store, golden_mismatch, put  # noqa: F401  (the boundary, the rounding and the record's two ends)

TAPS = {"133": (1, 3, 3), "311": (3, 1, 1), "333": (3, 3, 3)}

# The smallest shapes at which each mechanism can break.  order: 't' = (b,t,c,h,w), 'c' = (b,c,t,h,w); view: x is a transposed view of
# the other memory order.
OP_CASES = [
    dict(name="one_frame_rgb", B=1, T=1, Cin=3, Cout=16, H=5, W=7, taps="333", order="t", bias=True),
    dict(name="w33_two_clips", B=2, T=3, Cin=16, Cout=16, H=9, W=33, taps="133", order="t"),
    dict(name="t5_ring", B=1, T=5, Cin=64, Cout=64, H=8, W=40, taps="311", order="t"),
    dict(name="conv_first_view", B=1, T=2, Cin=27, Cout=80, H=6, W=10, taps="133", order="c", bias=True, view=True),
    dict(name="upsample_group", B=1, T=2, Cin=64, Cout=256, H=5, W=7, taps="133", order="c", bias=True, shuffle=2, slope=0.1),
    dict(name="conv_last", B=1, T=2, Cin=64, Cout=3, H=6, W=10, taps="133", order="c", bias=True),
    dict(name="c256", B=1, T=3, Cin=256, Cout=256, H=4, W=4, taps="311", order="c"),
    dict(name="hw1", B=1, T=2, Cin=16, Cout=16, H=1, W=1, taps="333", order="t", bias=True, slope=0.01),
]

# name -> (class name, constructor arguments, input shape): ConvST & co. take (b,t,c,h,w), Upsample takes (b,c,t,h,w)
MODULE_CASES = {
    "convst": ("ConvST", (16, 32), (1, 3, 16, 5, 7)),
    "convstblock": ("ConvSTBlock", (2, 3, 16), (1, 2, 3, 5, 7)),
    "psp3d": ("PixelShufflePack3D", (16, 16, 2), (2, 3, 16, 5, 7)),
    "upsample4": ("Upsample", (4, 64), (1, 64, 2, 5, 7)),
    "upsample1": ("Upsample", (1, 64), (1, 64, 2, 5, 7)),
}


def _convst_shapes(prefix, cin, cout):
    return {prefix + "conv_xy.weight": (cout, cin, 1, 3, 3), prefix + "conv_t.weight": (cout, cout, 3, 1, 1)}


def module_shapes(name):
    """state_dict key -> shape, in the reference's order"""
    cls, args, _ = MODULE_CASES[name]
    if cls == "ConvST":
        return _convst_shapes("", *args)
    if cls == "ConvSTBlock":
        blocks, cin, cout = args
        out = {"conv_in.weight": (cout, cin, 3, 3, 3), "conv_in.bias": (cout,)}
        for i in range(blocks):
            out.update(_convst_shapes(f"block.{i}.", cout, cout))
        return out
    if cls == "PixelShufflePack3D":
        return _convst_shapes("mapping.", args[0], args[1] * args[2] ** 2)
    scale, c = args
    out = {}
    for g in range(int(math.log2(scale))):
        out[f"{5 * g}.weight"], out[f"{5 * g}.bias"] = (4 * c, c, 1, 3, 3), (4 * c,)
    last = 5 * int(math.log2(scale))
    out[f"{last}.weight"], out[f"{last}.bias"] = (c, c, 1, 3, 3), (c,)
    return out


def _uniform(seed, shape, fan_in):
    s = 1.0 / math.sqrt(fan_in)
    return rand(seed, *shape, lo=-s, hi=s)


def module_params(name):
    """seeded fp32 parameters of a module case: uniform within 1 / sqrt(fan_in), as nn.Conv3d draws them, biases included"""
    base = 7000 + 100 * list(MODULE_CASES).index(name)
    shapes = module_shapes(name)
    out = {}
    for n, (key, shape) in enumerate(shapes.items()):
        w = shapes[key.rsplit(".", 1)[0] + ".weight"]
        out[key] = _uniform(base + n, shape, w[1] * w[2] * w[3] * w[4])
    return out


def module_inputs(name):
    """input and cotangent of the output"""
    cls, args, shape = MODULE_CASES[name]
    base = 7050 + 100 * list(MODULE_CASES).index(name)
    oshape = list(shape)
    if cls == "ConvST":
        oshape[2] = args[1]
    elif cls == "ConvSTBlock":
        oshape[2] = args[2]
    elif cls == "PixelShufflePack3D":
        oshape[2], oshape[3], oshape[4] = args[1], 2 * shape[3], 2 * shape[4]
    else:
        oshape[3], oshape[4] = args[0] * shape[3], args[0] * shape[4]
    return rand(base, *shape, lo=-1.0), rand(base + 1, *oshape, lo=-1.0)


def op_shapes(case):
    """logical shapes of x and of y in the case's axis order"""
    B, T, Cin, Cout, H, W = (case[k] for k in ("B", "T", "Cin", "Cout", "H", "W"))
    r = case.get("shuffle", 0) or 1
    co, ho, wo = Cout // (r * r), H * r, W * r
    if case["order"] == "t":
        return (B, T, Cin, H, W), (B, T, co, ho, wo)
    return (B, Cin, T, H, W), (B, co, T, ho, wo)


def op_inputs(i):
    """case i: x, weight, bias (or None) and the cotangent of y, fp32"""
    case = OP_CASES[i]
    xs, ys = op_shapes(case)
    k = TAPS[case["taps"]]
    fan_in = case["Cin"] * k[0] * k[1] * k[2]
    w = _uniform(6001 + 10 * i, (case["Cout"], case["Cin"]) + k, fan_in)
    b = _uniform(6002 + 10 * i, (case["Cout"],), fan_in) if case.get("bias") else None
    return rand(6000 + 10 * i, *xs, lo=-1.0), w, b, rand(6003 + 10 * i, *ys, lo=-1.0)


# ---- restatement ----------------------------------------------------------------------------------------------------------------------
def conv3d(x, w, b=None, slope=None, shuffle=0, time_major=False, store=None):
    """one launch: act(conv3d(x, w) + b), the shuffle on the last three axes of the (b,t,c,h,w) order; rounded in and out"""
    x = _st(x, store)
    if time_major:
        x = x.transpose(1, 2)
    y = F.conv3d(x, w, b, padding=tuple(k // 2 for k in w.shape[2:]))
    if shuffle:
        y = F.pixel_shuffle(y.transpose(1, 2), shuffle).transpose(1, 2)
    if slope is not None:
        y = F.leaky_relu(y, slope)
    if time_major:
        y = y.transpose(1, 2)
    return _st(y, store)


def conv_st(x, p, prefix="", shuffle=0, store=None):
    x = conv3d(x, p[prefix + "conv_xy.weight"], time_major=True, store=store)
    return conv3d(x, p[prefix + "conv_t.weight"], shuffle=shuffle, time_major=True, store=store)


def module_forward(name, x, p, store=None):
    cls, args, _ = MODULE_CASES[name]
    if cls == "ConvST":
        return conv_st(x, p, store=store)
    if cls == "ConvSTBlock":
        x = conv3d(x, p["conv_in.weight"], p["conv_in.bias"], time_major=True, store=store)
        for i in range(args[0]):
            x = conv_st(x, p, f"block.{i}.", store=store)
        return x
    if cls == "PixelShufflePack3D":
        return conv_st(x, p, "mapping.", shuffle=2, store=store)
    groups = int(math.log2(args[0]))
    for g in range(groups):
        x = conv3d(x, p[f"{5 * g}.weight"], p[f"{5 * g}.bias"], slope=0.1, shuffle=2, store=store)
    return conv3d(x, p[f"{5 * groups}.weight"], p[f"{5 * groups}.bias"], store=store)


def run_op_case(i, dtype, store=None):
    """case i on the CPU in `dtype` (weights in `dtype` too): out, dx, dw and (with a bias) db under the case's cotangent"""
    case = OP_CASES[i]
    x, w, b, cot = op_inputs(i)
    x, cot = x.to(dtype), cot.to(dtype)
    if store is not None:
        x, cot = store(x), store(cot)
    x.requires_grad_(True)
    w = w.to(dtype).requires_grad_(True)
    b = None if b is None else b.to(dtype).requires_grad_(True)
    y = conv3d(x, w, b, case.get("slope"), case.get("shuffle", 0), case["order"] == "t", store)
    (y * cot).sum().backward()
    out = {"out": y.detach(), "dx": x.grad, "dw": w.grad}
    if b is not None:
        out["db"] = b.grad
    return out


def run_module_case(name, dtype, store=None):
    """output, d input and every parameter gradient by name"""
    x, cot = (t.to(dtype) for t in module_inputs(name))
    if store is not None:
        x, cot = store(x), store(cot)
    x.requires_grad_(True)
    p = {k: v.to(dtype).requires_grad_(True) for k, v in module_params(name).items()}
    y = module_forward(name, x, p, store)
    (y * cot).sum().backward()
    return y.detach(), x.grad, {k: v.grad for k, v in p.items()}
