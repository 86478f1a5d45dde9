"""CPU checks of the DCT-token MLP-Mixer and the warm-up scheduler: libvsrlab_mixer.so's exports and argument checks (every entry
refuses bad arguments before it touches the GPU), the modules' constructors, state_dict keys and refusals, the restatement of
tests/mixer_common.py against the reference's recorded fp64 results (tests/golden/token_mixer.npz), and the scheduler's learning-rate
sequences against the recorded ones.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mixer_common as MC
from helpers import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"vsr_block_dct_fwd", "vsr_block_idct_fwd", "vsr_axis_mlp_supported", "vsr_axis_mlp_scratch_bytes", "vsr_axis_mlp_fwd",
         "vsr_axis_mlp_bwd"}


@pytest.fixture(scope="module")
def gold():
    return golden("token_mixer")


def _gold_names(key):
    with np.load(os.path.join(GOLDEN, "token_mixer.npz"), allow_pickle=False) as z:
        return [str(s) for s in z[key]]


def _gold_shapes(tag):
    return dict(zip(_gold_names(tag + "__keys"), (tuple(int(n) for n in s.split(",")) for s in _gold_names(tag + "__shapes"))))


def _w3(gold, ps):
    """the reference's (3 ps^2, 1, ps, ps) weight, from its recorded (ps^2, 1, ps, ps) basis"""
    return torch.cat([gold[f"weight_ps{ps}"]] * 3, dim=0)


# ---- the library --------------------------------------------------------------------------------------------------------------------
def test_the_mixer_library_loads_once_and_types_every_entry():
    from vsrlab_amd import _lib
    lib = _lib.load_mixer()
    assert _lib.load_mixer() is lib and lib is not _lib.load()
    for name, (res, args) in _lib.MIXER_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_library_exports():
    """the entry points live in a library of their own, which exports what its header declares and nothing else"""
    from vsrlab_amd import _lib
    lib = _lib.load_mixer()
    assert set(_lib.MIXER_EXPORTS) == NAMES and not NAMES & set(_lib.EXPORTS)
    header = open(os.path.join(ROOT, "include", "vsrlab_mixer.h")).read()
    assert set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header)) == NAMES
    assert set(re.findall(r"^(?:int|size_t) (vsr_[a-z0-9_]+)\(", header, re.M)) == NAMES
    from test_hr_tail_host import _exported_vsr_symbols          # the dynamic symbol table, read from the ELF file
    assert _exported_vsr_symbols(_lib.MIXER_LIB_PATH) == NAMES
    assert not any(hasattr(_lib.load(), n) for n in NAMES) and all(hasattr(lib, n) for n in NAMES)
    bounds = tuple(int(re.search(rf"#define VSR_AXIS_MLP_MAX_{k} (\d+)", header).group(1)) for k in ("D", "HIDDEN"))
    assert bounds == (_lib.AXIS_MLP_MAX_D, _lib.AXIS_MLP_MAX_HIDDEN) and bounds[0] >= 48 and bounds[1] >= 144
    # the structs as the header lays them out
    assert [f[0] for f in _lib.BlockDctDesc._fields_] == re.search(r"struct VsrBlockDctDesc \{\s*int ([^;]+);", header).group(1).split(", ")
    assert ctypes.sizeof(_lib.AxisMlpDesc) == 40 and _lib.AxisMlpDesc.inner.offset == 16 and _lib.AxisMlpDesc.hidden.offset == 24


def test_block_transform_entries_reject_bad_arguments_before_touching_the_gpu():
    from vsrlab_amd import _lib
    lib = _lib.load_mixer()
    BADARG, UNSUPPORTED = -1, -2
    one = ctypes.c_void_p(256)                                    # a non-null pointer that is never dereferenced: every call below is refused

    def call(fn, a=one, w=one, b=one, desc=True, **kw):
        d = dict(N=1, C=3, H=8, W=8, ps=4, dtype=0)
        d.update(kw)
        return fn(ctypes.byref(_lib.BlockDctDesc(**d)) if desc else None, a, w, b, None)

    for fn in (lib.vsr_block_dct_fwd, lib.vsr_block_idct_fwd):
        for bad in (dict(desc=False), dict(a=None), dict(w=None), dict(b=None), dict(N=0), dict(C=0), dict(H=0), dict(W=-4), dict(ps=0),
                    dict(ps=-2), dict(dtype=2), dict(dtype=-1), dict(a=ctypes.c_void_p(258)), dict(b=ctypes.c_void_p(257), dtype=1),
                    dict(a=ctypes.c_void_p(257), dtype=1), dict(w=ctypes.c_void_p(258))):
            assert call(fn, **bad) == BADARG, (fn.__name__, bad)
        for bad in (dict(ps=3), dict(ps=16), dict(C=17), dict(C=5, ps=8), dict(C=65, ps=2), dict(H=3), dict(W=2),
                    dict(N=1 << 30, H=1 << 20, W=1 << 20), dict(N=1 << 30, C=1, H=1 << 16, W=4)):
            assert call(fn, **bad) == UNSUPPORTED, (fn.__name__, bad)


def test_axis_mlp_entries_reject_bad_arguments_before_touching_the_gpu():
    from vsrlab_amd import _lib
    lib = _lib.load_mixer()
    BADARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)

    def desc(outer=4, D=48, inner=1, hidden=96, dtype=0, residual=1):
        return ctypes.byref(_lib.AxisMlpDesc(outer, D, inner, hidden, dtype, residual))

    def fwd(d=None, x=one, w1=one, b1=one, w2=one, b2=one, y=one, null_desc=False, **kw):
        return lib.vsr_axis_mlp_fwd(None if null_desc else desc(**kw), x, w1, b1, w2, b2, y, None)

    def bwd(x=one, dy=one, w1=one, b1=one, w2=one, b2=one, dx=one, dw1=one, db1=one, dw2=one, db2=one, scratch=one, nbytes=1 << 40,
            null_desc=False, **kw):
        return lib.vsr_axis_mlp_bwd(None if null_desc else desc(**kw), x, dy, w1, b1, w2, b2, dx, dw1, db1, dw2, db2, scratch, nbytes, None)

    shape_bad = (dict(outer=0), dict(D=0), dict(inner=0), dict(hidden=0), dict(outer=-1), dict(inner=-7), dict(dtype=2), dict(dtype=-1))
    shape_unsupported = (dict(D=49), dict(D=67, hidden=201), dict(hidden=_lib.AXIS_MLP_MAX_HIDDEN + 1), dict(outer=1 << 40, inner=1 << 40),
                         dict(outer=1 << 62, inner=1, D=4), dict(outer=1 << 45, inner=1, D=2))
    for bad in (dict(null_desc=True), dict(x=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None), dict(y=None), dict(x=odd),
                dict(y=ctypes.c_void_p(257), dtype=1), dict(w1=odd), dict(b1=odd), dict(w2=odd), dict(b2=odd)) + shape_bad:
        assert fwd(**bad) == BADARG, bad
    for bad in (dict(null_desc=True), dict(x=None), dict(dy=None), dict(w1=None), dict(b1=None), dict(w2=None), dict(b2=None),
                dict(dw1=None), dict(db1=None), dict(dw2=None), dict(db2=None), dict(scratch=None), dict(dy=odd), dict(dx=odd), dict(dw1=odd),
                dict(db2=odd), dict(scratch=odd), dict(x=ctypes.c_void_p(257), dtype=1)) + shape_bad:
        assert bwd(**bad) == BADARG, bad
    for bad in shape_unsupported:
        assert fwd(**bad) == UNSUPPORTED and bwd(**bad) == UNSUPPORTED, bad
        assert lib.vsr_axis_mlp_supported(desc(**bad)) == 0 and lib.vsr_axis_mlp_scratch_bytes(desc(**bad)) == 0
    for bad in shape_bad:
        assert lib.vsr_axis_mlp_supported(desc(**bad)) == 0 and lib.vsr_axis_mlp_scratch_bytes(desc(**bad)) == 0
    assert lib.vsr_axis_mlp_supported(None) == 0 and lib.vsr_axis_mlp_scratch_bytes(None) == 0
    need = lib.vsr_axis_mlp_scratch_bytes(desc())
    assert need == (2 * 48 * 96 + 96 + 48) * 4 and bwd(nbytes=need - 1) == WORKSPACE       # 4 positions: one workgroup, one partial set
    assert lib.vsr_axis_mlp_scratch_bytes(desc(outer=1 << 20)) == 256 * need               # capped at 256 partial sets


def test_the_fused_path_covers_the_stated_shapes():
    from vsrlab_amd import _lib
    from vsrlab_amd.core.token_ops import axis_mlp_is_fused
    lib = _lib.load_mixer()
    for D, hidden, want in ((48, 96, 1), (48, 144, 1), (2, 4, 1), (12, 36, 1), (1, 1, 1), (67, 201, 0)):
        for outer, inner in ((1, 1), (3, 1), (1, 288), (5, 48), (1 << 20, 1 << 10)):
            for dtype in (0, 1):
                assert lib.vsr_axis_mlp_supported(ctypes.byref(_lib.AxisMlpDesc(outer, D, inner, hidden, dtype, 1))) == want, (D, hidden, outer, inner)
        assert axis_mlp_is_fused(D, hidden) is bool(want)


# ---- the modules --------------------------------------------------------------------------------------------------------------------
def test_transform_modules_follow_the_reference(gold):
    from vsrlab_amd.core.modules.dct_transforms import DecoderIDCT, EncoderDCT
    enc, dec = EncoderDCT(4), DecoderIDCT(3, 4, 8, 12)
    for module, tag in ((enc, "encoder"), (dec, "decoder")):
        assert {k: tuple(v.shape) for k, v in module.state_dict().items()} == _gold_shapes(tag)
        assert list(module.state_dict()) == _gold_names(tag + "__keys") and len(module.state_dict()) == 1
        assert not any(p.requires_grad for p in module.parameters())
    assert list(enc.state_dict()) == ["dct_conv.weight"] and list(dec.state_dict()) == ["reverse_dct.weight"]
    assert (dec.h, dec.w) == (2, 3) and EncoderDCT().ps == 4
    for ps in (2, 4, 8):
        want = gold[f"weight_ps{ps}"]
        assert want.dtype == torch.float32
        for module in (EncoderDCT(ps), DecoderIDCT(3, ps, 16, 16)):
            holder = module.dct_conv if isinstance(module, EncoderDCT) else module.reverse_dct
            assert module.weight.dtype == torch.float32 and tuple(module.weight.shape) == (ps * ps, 1, ps, ps)
            assert torch.equal(holder.weight, torch.cat([module.weight] * 3))
            got = module.weight
            assert got.shape == want.shape
            ulp = torch.from_numpy(np.spacing(np.maximum(np.abs(got.numpy()), np.abs(want.numpy()))))
            assert bool(((got - want).abs() <= ulp).all()), ps
        # the basis is orthonormal: the decoder inverts the encoder
        m = torch.from_numpy(EncoderDCT(ps).generate_dct_matrix(ps)).reshape(ps * ps, ps * ps)
        assert m.dtype == torch.float64 and float((m @ m.T - torch.eye(ps * ps, dtype=torch.float64)).abs().max()) < 1e-14
    assert abs(EncoderDCT.build_filter(1, 0, 4) - 0.5) < 1e-15 and abs(DecoderIDCT.build_filter(0, 1, 2) - 0.5 ** 0.5) < 1e-15


def test_transform_modules_refuse_what_they_do_not_provide():
    from vsrlab_amd.core.modules.dct_transforms import DecoderIDCT, EncoderDCT
    from vsrlab_amd.core.token_ops import block_dct
    for out_ch in (1, 2):
        with pytest.raises(NotImplementedError, match="out_ch"):
            DecoderIDCT(out_ch, 4, 8, 8)
    with pytest.raises(ValueError, match="tokens"):
        DecoderIDCT(3, 4, 8, 12)(torch.zeros(1, 2, 5, 48))
    x = torch.zeros(1, 2, 3, 8, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EncoderDCT(4)(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DecoderIDCT(3, 4, 8, 12)(torch.zeros(1, 2, 6, 48))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        block_dct(x[0], EncoderDCT(4).dct_conv.weight, 4)


def test_mixer_modules_follow_the_reference():
    from vsrlab_amd.core.modules.mlp import MixerBlock, Mlp, MlpMixer
    for name, (args, _) in MC.MIXER_CASES.items():
        model = MlpMixer(*args)
        want = _gold_shapes("mixer_" + name)
        assert list(model.state_dict()) == list(want) == list(MC.mixer_shapes(args)) and len(want) == 12 * args[4]
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want == MC.mixer_shapes(args)
        model.load_state_dict(MC.mixer_params(name), strict=True)
        assert all(p.requires_grad for p in model.parameters())
    block = MixerBlock(6, 48, 2, 3)
    assert [tuple(m.mlp[0].weight.shape) for m in (block.time_mlp, block.patches_mlp, block.channels_mlp)] == [(6, 2), (18, 6), (144, 48)]
    assert list(Mlp(5, 7).state_dict()) == ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
    x = torch.zeros(1, 2, 6, 48)
    for module in (Mlp(48, 96), block, MlpMixer(6, 48, 2, 2, 1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            module(x)


def test_axis_mlp_checks_its_weights():
    from vsrlab_amd.core import token_ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        token_ops.axis_mlp(torch.zeros(2, 3), 1, torch.zeros(6, 3), torch.zeros(6), torch.zeros(3, 6), torch.zeros(3))
    assert "GEMM plumbing" in token_ops.axis_mlp.__doc__ and "not a fallback for a missing kernel" in " ".join(token_ops.axis_mlp.__doc__.split())


def test_the_compat_mapping_resolves_the_new_modules():
    import importlib

    import vsrlab_amd
    vsrlab_amd.install_as_vsrlab(force=True)
    from vsrlab_amd.core import schedulers
    from vsrlab_amd.core.modules import dct_transforms, mlp
    assert importlib.import_module("vsrlab.core.modules.dct_transforms").EncoderDCT is dct_transforms.EncoderDCT
    assert importlib.import_module("vsrlab.core.modules.dct_transforms").DecoderIDCT is dct_transforms.DecoderIDCT
    assert importlib.import_module("vsrlab.core.modules.mlp").MlpMixer is mlp.MlpMixer
    assert importlib.import_module("vsrlab.core.schedulers").CosineAnnealingLinearWarmup is schedulers.CosineAnnealingLinearWarmup


def test_the_new_modules_need_no_einops():
    import subprocess
    import sys
    code = ("import sys; sys.modules['einops'] = None\n"
            "from vsrlab_amd.core.modules import dct_transforms, mlp\nfrom vsrlab_amd.core import schedulers, token_ops\n"
            "assert 'einops' not in {m.split('.')[0] for m, v in sys.modules.items() if v is not None}\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ---- the restatement against the reference's record --------------------------------------------------------------------------------------
def test_the_golden_is_small_and_fp64(gold):
    assert os.path.getsize(os.path.join(GOLDEN, "token_mixer.npz")) < 128 * 1024
    assert all(v.dtype == torch.float64 for k, v in gold.items() if not k.startswith("weight_ps"))


@pytest.mark.parametrize("i", range(len(MC.DCT_CASES)))
def test_the_restated_transforms_reproduce_the_reference(gold, i):
    ps = MC.DCT_CASES[i][0]
    got = MC.run_dct_case(i, torch.float64, _w3(gold, ps))
    for k, v in got.items():
        assert MC.golden_mismatch(gold, f"dct{i}__{k}", v) <= 1e-12, (i, k)
    if i == 4:      # (10, 9) in 4 x 4 blocks: the remainder rows and columns get no gradient
        dx = got["enc_dx"]
        assert not dx[..., 8:, :].any() and not dx[..., :, 8:].any() and bool(dx[..., :8, :8].abs().min() > 0)
        assert tuple(got["dec_out"].shape[-2:]) == (8, 8)


@pytest.mark.parametrize("name", list(MC.MIXER_CASES))
def test_the_restated_mixer_reproduces_the_reference(gold, name):
    out, dx, grads = MC.run_mixer_case(name, torch.float64, _w3(gold, MC.E2E_PS))
    assert MC.golden_mismatch(gold, f"{name}__out", out) <= 1e-12
    assert MC.golden_mismatch(gold, f"{name}__dx", dx) <= 1e-12
    assert len(grads) == 12 * MC.MIXER_CASES[name][0][4]
    for k, g in grads.items():
        assert MC.golden_mismatch(gold, f"{name}__grad__{k}", g) <= 1e-12, k


def test_bf16_emulation_rounds_at_the_boundaries_only():
    x = MC.mixer_inputs("fused")[0].requires_grad_(True)
    p = MC.mixer_params("fused")
    k = "mixer.0.channels_mlp.mlp."
    y = MC.axis_mlp(x, 3, p[k + "0.weight"], p[k + "0.bias"], p[k + "2.weight"], p[k + "2.bias"], MC.bf16_store)
    assert torch.equal(y, MC.bf16_store(y)) and not torch.equal(y, MC.axis_mlp(x, 3, *(p[k + s] for s in ("0.weight", "0.bias", "2.weight", "2.bias"))))
    y.sum().backward()
    assert torch.equal(x.grad, MC.bf16_store(x.grad))


# ---- the scheduler ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MC.SCHEDULER_CASES))
def test_scheduler_reproduces_the_recorded_rates(gold, name):
    from vsrlab_amd.core.schedulers import CosineAnnealingLinearWarmup
    rows, opt = MC.scheduler_sequence(CosineAnnealingLinearWarmup, name)
    want = gold["sched__" + name]
    assert want.shape == (len(MC.SCHEDULER_CASES[name][2]) + 1, len(MC.SCHEDULER_CASES[name][1]))
    for r, (got_row, want_row) in enumerate(zip(rows, want.tolist())):
        for got, exp in zip(got_row, want_row):
            assert abs(got - exp) <= 1e-15 * abs(exp), (name, r, got, exp)
    assert len({tuple(r) for r in want.tolist()}) > len(want) // 2               # the record is no constant sequence
    # what core.utils.update_weights hands to the fused Adam step: a float per param group, nothing else
    assert all(type(g["lr"]) is float for g in opt.param_groups)


def test_scheduler_starts_at_the_floor_and_peaks_after_the_warmup():
    from vsrlab_amd.core.schedulers import CosineAnnealingLinearWarmup
    rows, _ = MC.scheduler_sequence(CosineAnnealingLinearWarmup, "restarts")
    flat = [r[0] for r in rows]
    assert flat[0] == 1e-5 and flat[1] == (1e-3 - 1e-5) * 1 / 2 + 1e-5 and abs(flat[2] - 1e-3) < 1e-18   # step 0 is taken by the constructor
    assert abs(flat[8] - 5e-4) < 1e-18 and max(flat[6:]) == flat[8]                               # the second cycle peaks at gamma * peak
    assert flat[6] == 1e-5                                                                        # a restart begins at the floor


def test_scheduler_keeps_the_reference_assertions():
    from vsrlab_amd.core.schedulers import CosineAnnealingLinearWarmup

    def opt():
        return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)

    with pytest.raises(AssertionError, match="Warmup steps should be smaller"):
        CosineAnnealingLinearWarmup(opt(), first_cycle_steps=4, min_lrs=[0.0], warmup_steps=4)
    with pytest.raises(AssertionError, match="Only one of min_lrs and min_lrs_pow"):
        CosineAnnealingLinearWarmup(opt(), first_cycle_steps=4, min_lrs=[0.0], min_lrs_pow=2)
    with pytest.raises(AssertionError, match="Only one of min_lrs and min_lrs_pow"):
        CosineAnnealingLinearWarmup(opt(), first_cycle_steps=4)
    with pytest.raises(ValueError, match="param groups"):
        CosineAnnealingLinearWarmup(opt(), first_cycle_steps=4, min_lrs=[0.0, 0.0])


def test_documents_say_what_is_provided():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert all(n in readme for n in ("EncoderDCT", "DecoderIDCT", "MlpMixer", "CosineAnnealingLinearWarmup"))
    assert "not provided either" not in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "11j" in design and "token_mixer" in design
    assert "libvsrlab_mixer.so" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "vsrlab_mixer.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
