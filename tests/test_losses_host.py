"""CPU checks of LossPipeline, WL1Loss, rmse_loss and libvsrlab_losses.so: the library's exports and argument checks (every entry
refuses bad arguments before it touches the GPU), LossPipeline's bookkeeping with stub losses, the refusals of CPU tensors, and the
restatement of tests/losses_common.py against the reference's recorded fp64 results (tests/golden/loss_pipeline.npz), and the
numpy restatement of the entry's summation order.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import losses_common as LC
from helpers import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return golden("loss_pipeline")


def _gold_names(key):
    with np.load(os.path.join(GOLDEN, "loss_pipeline.npz"), allow_pickle=False) as z:
        return [str(s) for s in z[key]]


class Const(nn.Module):
    """a loss that returns a constant and records what it was given"""

    def __init__(self, value):
        super().__init__()
        self.value = value
        self.seen = []

    def forward(self, x, y):
        self.seen.append((x, y))
        return self.value


def test_the_losses_library_loads_once_and_types_every_entry():
    from vsrlab_amd import _lib
    lib = _lib.load_losses()
    assert _lib.load_losses() is lib and lib is not _lib.load()
    for name, (res, args) in _lib.LOSSES_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name
    assert lib.vsr_pixel_loss_scratch_floats() > 0


def test_library_exports():
    """the entry points live in a library of their own, which exports what its header declares and nothing else"""
    from vsrlab_amd import _lib
    lib = _lib.load_losses()
    names = {"vsr_pixel_loss_scratch_floats", "vsr_pixel_loss_fwd_bwd", "vsr_resize_bilinear_bwd"}
    assert set(_lib.LOSSES_EXPORTS) == names and not names & set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "vsrlab_losses.h")).read()
    assert set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header)) == names
    from test_hr_tail_host import _exported_vsr_symbols          # the dynamic symbol table, read from the ELF file
    assert _exported_vsr_symbols(_lib.LOSSES_LIB_PATH) == names
    assert not any(hasattr(_lib.load(), n) for n in names) and all(hasattr(lib, n) for n in names)
    assert (_lib.LOSS_L1, _lib.LOSS_MSE) == tuple(int(re.search(rf"#define VSR_LOSS_{k} (\d+)", header).group(1)) for k in ("L1", "MSE"))


def test_every_entry_rejects_bad_arguments_before_touching_the_gpu():
    from vsrlab_amd import _lib
    lib = _lib.load_losses()
    BADARG, UNSUPPORTED = -1, -2
    one = ctypes.c_void_p(256)                                    # a non-null pointer that is never dereferenced: every call below is refused

    def loss(kind=0, x=one, xd=0, y=one, yd=0, dx=one, out=one, scratch=one, n=8):
        return lib.vsr_pixel_loss_fwd_bwd(kind, x, xd, y, yd, dx, out, scratch, n, None)

    for bad in (dict(x=None), dict(y=None), dict(out=None), dict(scratch=None), dict(n=0), dict(n=-5), dict(kind=2), dict(kind=-1),
                dict(xd=2), dict(yd=-1), dict(xd=7, yd=7), dict(x=ctypes.c_void_p(258)), dict(y=ctypes.c_void_p(257), yd=1),
                dict(dx=ctypes.c_void_p(257), xd=1), dict(out=ctypes.c_void_p(258))):
        assert loss(**bad) == BADARG, bad

    def adjoint(dout=one, din=one, planes=2, H=4, W=4, h=2, w=2):
        return lib.vsr_resize_bilinear_bwd(dout, din, planes, H, W, h, w, None)

    for bad in (dict(dout=None), dict(din=None), dict(planes=0), dict(H=0), dict(W=-1), dict(h=0), dict(w=-3)):
        assert adjoint(**bad) == BADARG, bad
    assert adjoint(H=(1 << 22) + 1) == UNSUPPORTED and adjoint(w=(1 << 22) + 1) == UNSUPPORTED
    assert adjoint(planes=1 << 40, H=1 << 22, W=1 << 22) == UNSUPPORTED


def test_pipeline_key_names_totals_and_a_loss_used_twice():
    from vsrlab_amd.core.losses import LossPipeline
    a, b = Const(2.0), Const(0.25)
    pipe = LossPipeline({"b": b, "a": a}, [{"a": {"x": "p", "y": "q"}}, {"b": {"x": "q", "y": "p"}}, {"a": {"x": "p", "y": "p"}}])
    assert list(pipe.keys()) == ["a", "b"]                        # sorted-name order
    p, q = torch.zeros(1), torch.ones(1)
    args = {"p": p, "q": q, "a": 99.0}                            # a stale value is zeroed first
    out = pipe(args)
    assert out is args and out == {"p": p, "q": q, "a": 4.0, "b": 0.25, "loss": 4.25}
    assert [tuple(s) for s in a.seen] == [(p, q), (p, p)] and [tuple(s) for s in b.seen] == [(q, p)]
    for prefix, postfix, names in ((None, None, ("a", "b", "loss")), ("val/", None, ("val/a", "val/b", "val/loss")),
                                   (None, "_d", ("a_d", "b_d", "loss_d")), ("t/", "_g", ("t/a_g", "t/b_g", "t/loss_g"))):
        out = LossPipeline({"a": a, "b": b}, [{"b": {"x": "p", "y": "q"}}], prefix=prefix, postfix=postfix)({"p": p, "q": q})
        assert {k: out[k] for k in names} == dict(zip(names, (0, 0.25, 0.25))) and set(out) == {"p", "q", *names}
    # a loss that no term names keeps its zero; a term with several entries evaluates its last, as the reference's loop does
    out = LossPipeline({"a": a, "b": b}, [{"a": {"x": "p", "y": "q"}, "b": {"x": "q", "y": "q"}}])({"p": p, "q": q})
    assert (out["a"], out["b"], out["loss"]) == (0, 0.25, 0.25)


def test_pipeline_rejects_non_modules_and_duplicate_names():
    from vsrlab_amd.core.losses import LossPipeline
    with pytest.raises(ValueError, match="not an instance"):
        LossPipeline({"a": Const(1.0), "f": lambda x, y: 0.0}, [])
    pipe = LossPipeline({"a": Const(1.0)}, [])
    with pytest.raises(ValueError, match="two losses both named a"):
        pipe.add_losses({"a": Const(2.0)})
    pipe.add_losses({"c": Const(2.0)})
    assert list(pipe.keys()) == ["a", "c"]


def test_clone_is_an_independent_deep_copy():
    """the reference's clone() raises NameError (deepcopy is never imported); here it works"""
    from vsrlab_amd.core.losses import LossPipeline
    lin = nn.Linear(2, 2)
    pipe = LossPipeline({"a": Const(1.5), "lin": lin}, [{"a": {"x": "p", "y": "p"}}], prefix="train/")
    twin = pipe.clone(prefix="val/", postfix="_e")
    assert (pipe.prefix, pipe.postfix) == ("train/", None) and (twin.prefix, twin.postfix) == ("val/", "_e")
    assert twin["a"] is not pipe["a"] and twin["lin"].weight is not lin.weight and torch.equal(twin["lin"].weight, lin.weight)
    assert twin.losses["a"] is twin["a"]
    twin["a"].value = 7.0
    with torch.no_grad():
        twin["lin"].weight.zero_()
    p = torch.zeros(1)
    assert pipe({"p": p})["train/loss"] == 1.5 and twin({"p": p})["val/loss_e"] == 7.0 and bool(lin.weight.abs().sum() > 0)
    same = pipe.clone()
    assert (same.prefix, same.postfix) == ("train/", None) and same is not pipe


def test_match_keys_resize_the_named_side_to_the_other():
    from vsrlab_amd.core import losses
    calls = []

    def fake_resize(x, size):
        calls.append((x, tuple(size)))
        return x.new_zeros(x.shape[:-2] + tuple(size))

    c = Const(1.0)
    pipe = losses.LossPipeline({"c": c}, [{"c": {"x": "small", "y": "match_big"}}, {"c": {"x": "match_small", "y": "big"}}])
    small, big = torch.ones(1, 2, 3, 5, 7), torch.ones(1, 2, 3, 16, 24)
    real, losses.resize = losses.resize, fake_resize
    try:
        pipe({"small": small, "big": big})
    finally:
        losses.resize = real
    assert [(t is big, s) for t, s in calls] == [(True, (5, 7)), (False, (16, 24))]
    assert [(x.shape[-2:], y.shape[-2:]) for x, y in c.seen] == [((5, 7), (5, 7)), ((16, 24), (16, 24))]
    assert c.seen[0][0] is small and c.seen[1][1] is big
    # x is tested first: with both sides marked only x is matched, and y is looked up under its full name
    with pytest.raises(KeyError, match="match_small"):
        losses.LossPipeline({"c": c}, [{"c": {"x": "match_big", "y": "match_small"}}])({"small": small, "big": big, "c": 0})


def test_wl1loss_follows_the_reference_constructor():
    from vsrlab_amd.core.losses import WL1Loss
    m = WL1Loss(2.0, reduction="sum")
    assert isinstance(m, nn.L1Loss) and m.weight == 2.0 and m.reduction == "sum" and m.state_dict() == {}
    assert WL1Loss().weight == 1.0 and WL1Loss().reduction == "mean"
    import vsrlab_amd
    vsrlab_amd.install_as_vsrlab(force=True)
    import importlib
    ref_path = importlib.import_module("vsrlab.core.losses")
    assert ref_path.WL1Loss is WL1Loss and all(hasattr(ref_path, n) for n in ("rmse_loss", "LossPipeline"))


def test_the_new_losses_have_no_cpu_fallback():
    from vsrlab_amd.core.losses import LossPipeline, WL1Loss, rmse_loss
    x, y = LC.single_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WL1Loss()(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rmse_loss(x, y)
    sr, hr, lq = LC.pipeline_inputs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LossPipeline({"c": Const(1.0)}, [{"c": {"x": "lq", "y": "match_hr"}}])({"hr": hr, "lq": lq})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LossPipeline({"c": Const(1.0)}, [{"c": {"x": "match_lq", "y": "hr"}}])({"hr": hr, "lq": lq.requires_grad_(True)})


def test_the_golden_records_the_pipeline_of_losses_common(gold):
    assert _gold_names("pipe__order") == LC.PIPELINE_ORDER == ["charb", "l1", "rmse", "l1"]
    assert sorted(_gold_names("pipe__output_keys")) == sorted(LC.OUTPUT_KEYS)
    assert {"pipe__" + k.replace("/", "|") for k in LC.OUTPUT_KEYS} | {"pipe__dsr", "pipe__dlq"} | \
        {f"{t}__{k}" for t in ("wl1", "rmse") for k in ("value", "dx", "dy")} == set(gold)
    assert all(v.dtype == torch.float64 for v in gold.values())
    assert os.path.getsize(os.path.join(GOLDEN, "loss_pipeline.npz")) < 64 * 1024
    # this package's pipeline zeroes its keys in the reference's order (that of the `losses` dict, then the total)
    from vsrlab_amd.core.losses import LossPipeline
    pipe = LossPipeline({"rmse": Const(0.0), "l1": Const(0.0), "charb": Const(0.0)}, [], prefix=LC.PREFIX, postfix=LC.POSTFIX)
    assert list(pipe({})) == _gold_names("pipe__output_keys")


def test_the_restatement_reproduces_the_reference(gold):
    sr, hr, lq = (t.double() for t in LC.pipeline_inputs())
    sr.requires_grad_(True), lq.requires_grad_(True)
    out = LC.restate_pipeline(sr, hr, lq)
    out[LC.PREFIX + "loss" + LC.POSTFIX].backward()
    for k in LC.OUTPUT_KEYS:
        want = float(gold["pipe__" + k.replace("/", "|")])
        assert abs(float(out[k].detach()) - want) <= 1e-12 * abs(want), k
    for name, g in (("dsr", sr.grad), ("dlq", lq.grad)):
        want = gold["pipe__" + name]
        assert g.shape == want.shape and float((g - want).abs().max()) <= 1e-12 * float(want.abs().max()), name
    for tag, fn in (("wl1", lambda x, y: LC.SINGLE_L1_WEIGHT * LC.l1(x, y)), ("rmse", LC.rmse)):
        x, y = (t.double().requires_grad_(True) for t in LC.single_inputs())
        v = fn(x, y)
        v.backward()
        assert abs(float(v.detach()) - float(gold[f"{tag}__value"])) <= 1e-12 * float(gold[f"{tag}__value"]), tag
        for name, g in (("dx", x.grad), ("dy", y.grad)):
            want = gold[f"{tag}__{name}"]
            assert float((g - want).abs().max()) <= 1e-12 * float(want.abs().max()), (tag, name)
        assert torch.equal(x.grad, -y.grad)


@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_the_order_emulation_is_the_sum_and_tells_the_orders_apart(kind):
    """emulate_pair_loss_order restates the summation order of vsr_pixel_loss_fwd_bwd (csrc/reduce.h) in numpy fp32; the GPU test
    requires the entry's bits to be its bits.  Here: it is a correct sum, and it is sensitive to what it pins.

    Bound: a term passes through at most K roundings -- its own, `trips * vec` additions in its lane and one for the tail, 6 of the
    shuffle tree, 2 of the combiner, the scaling, ceil(blocks / 256) strided additions and 8 of the halving tree -- so the result is
    within (1 + 2^-24)^K - 1 <= 2 K 2^-24 (K 2^-24 << 1) of the exact sum, relative to A = the mean of the terms' magnitudes."""
    for n in LC.ORDER_SIZES:
        x, y = (t.numpy() for t in LC.order_operands(n))
        d = x.astype(np.float64) - y.astype(np.float64)
        exact = float((np.abs(d) if kind == "l1" else d * d).sum() / n)        # the terms are non-negative: A is the value itself
        for aligned in (True, False):
            blocks, vec, trips = LC.pair_loss_launch(n, aligned)
            K = 1 + trips * vec + 1 + 6 + 2 + 1 + -(-blocks // LC.ORDER_BLOCK) + 8
            got = LC.emulate_pair_loss_order(x, y, kind, aligned=aligned)
            assert got.dtype == np.float32 and abs(float(got) - exact) <= 2 * K * 2.0 ** -24 * exact, (n, aligned, float(got), exact)
    assert LC.pair_loss_launch(2051) == (1, 8, 1) and LC.pair_loss_launch(2051, aligned=False) == (9, 1, 1)
    assert LC.pair_loss_launch(2107395) == (1024, 8, 2) and LC.pair_loss_launch(12293) == (6, 8, 1)
    bits = lambda v: np.float32(v).view(np.uint32)
    x, y = (t.numpy() for t in LC.order_operands(2051))
    assert bits(LC.emulate_pair_loss_order(x, y, kind, combine="inorder")) != bits(LC.emulate_pair_loss_order(x, y, kind))
    x, y = (t.numpy() for t in LC.order_operands(2107395))
    assert bits(LC.emulate_pair_loss_order(x, y, kind, final="inorder")) != bits(LC.emulate_pair_loss_order(x, y, kind))


def test_documents_say_what_is_provided():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "LossPipeline" in readme and "WL1Loss" in readme and "rmse_loss" in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "11i" in design and "pixel_losses" in design
    assert "libvsrlab_losses.so" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
