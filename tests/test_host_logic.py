"""CPU tests of the host side: plugin surface, C-ABI exports, no-fallback behaviour, and the
data-parallel (N > 1) plumbing under gloo with world_size 2.  No GPU compute is called."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import basicvsr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_matches_reference_keys_and_shapes():
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    m = BasicVSR(64, 30, 4, False, False)
    want = O.basicvsr_param_shapes(64, 30, 4)           # pinned to the reference by tests/golden
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(s) for k, s in want.items()}
    assert sum(p.numel() for p in m.parameters()) == 6_291_311
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 4_851_011   # frozen SPyNet (basicvsr.py:25-28)
    assert all(("spynet" in k) == (not p.requires_grad) for k, p in m.named_parameters())


def test_parameter_containers_match_the_reference_generated_schema():
    """tests/golden/state_dict_schema.json is written by make_golden.py from the REFERENCE's own modules (keys, shapes, dtypes,
    requires_grad): the vsrlab_amd containers must carry exactly that schema, so a reference checkpoint loads with strict=True."""
    import importlib
    import json
    with open(os.path.join(ROOT, "tests", "golden", "state_dict_schema.json")) as f:
        schema = json.load(f)
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    from vsrlab_amd.vsr.models.RealBasicVSR.realbasicvsr import RealBasicVSR
    from vsrlab_amd.vsr.models.VRT.modules.spynet import SpyNet
    from vsrlab_amd.vsr.models.VRT.modules.tmsa import RTMSA, TMSAG
    disc = importlib.import_module("vsrlab_amd.vsr.models.RealBasicVSR.modules.unet-discriminator").UNetDiscriminator
    built = {
        "BasicVSR(64,30,4,False,False)": BasicVSR(64, 30, 4, False, False),
        "RealBasicVSR(20,mid_channels=64,upscale=4,res_blocks=20)": RealBasicVSR(20, mid_channels=64, upscale=4, res_blocks=20,
                                                                                  pretrained_flow=False, train_flow=False),
        "UNetDiscriminator(3,64)": disc(3, 64),
        "VRT.SpyNet(pretrained=False)": SpyNet(pretrained=False),
        "TMSAG(120,(4,20,16),3,6,[2,8,8])": TMSAG(120, (4, 20, 16), 3, 6, window_size=[2, 8, 8], mut_attn=True, mlp_ratio=2., qkv_bias=True),
        "RTMSA(180,(6,16,16),2,6,[6,8,8])": RTMSA(180, (6, 16, 16), 2, 6, window_size=[6, 8, 8], mlp_ratio=2., qkv_bias=True),
    }
    assert set(built) == set(schema)
    for name, m in built.items():
        want = schema[name]
        req = {k: bool(p.requires_grad) for k, p in m.named_parameters()}
        got = {k: {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", ""), "requires_grad": req.get(k)} for k, v in m.state_dict().items()}
        assert set(got) == set(want), (name, sorted(set(got) ^ set(want))[:6])
        for k in want:
            assert got[k] == want[k], (name, k, got[k], want[k])


def test_vrt_window_helpers_equal_the_references():
    """relative position index, sine position encoding (bit-exact), shift masks (incl. axes with zero shift) and get_window_size of
    vsrlab_amd's window_attention module against tests/golden/vrt_helpers.npz (written from the reference's functions)."""
    import numpy as np
    from vsrlab_amd.vsr.models.VRT.modules import window_attention as M
    g = np.load(os.path.join(ROOT, "tests", "golden", "vrt_helpers.npz"))
    for name in ("a", "b", "c"):
        ws = tuple(int(v) for v in g[f"{name}__ws"])
        assert np.array_equal(M.WindowAttention.get_position_index(ws).numpy(), g[f"{name}__index"])
        assert np.array_equal(M.WindowAttention.get_sine_position_encoding(ws[1:], 60, normalize=True).numpy(), g[f"{name}__sine"])
    for i in range(4):
        a = [int(v) for v in g[f"m{i}__args"]]
        mask = M.compute_mask(a[0], a[1], a[2], tuple(a[3:6]), tuple(a[6:9]), "cpu")
        assert mask.dtype == torch.float32 and np.array_equal(mask.numpy().astype(np.int8), g[f"m{i}__mask"])
    for i in range(3):
        a = [int(v) for v in g[f"w{i}__args"]]
        u, v = M.get_window_size(tuple(a[0:3]), tuple(a[3:6]), tuple(a[6:9]))
        assert list(u) + list(v) == [int(x) for x in g[f"w{i}__out"]]
    x = torch.randn(2, 4, 16, 16, 5)
    win = M.window_partition(x, (2, 8, 8))
    assert win.shape == (2 * 2 * 2 * 2, 128, 5) and torch.equal(M.window_reverse(win.view(-1, 2, 8, 8, 5), (2, 8, 8), 2, 4, 16, 16), x)
    assert torch.equal(win[3, 9], x[0, 0, 8 + 1, 8 + 1])           # window (0, 1, 1), token (0, 1, 1)


def test_realbasicvsr_surface_and_keys():
    from vsrlab_amd.vsr.models.RealBasicVSR.realbasicvsr import RealBasicVSR
    m = RealBasicVSR(2, mid_channels=64, upscale=4, res_blocks=2, pretrained_flow=False, train_flow=False)
    keys = set(m.state_dict())
    assert {"cleaner.resblock.conv.0.weight", "cleaner.resblock.res_block.1.conv2.bias", "cleaner.conv.weight",
            "basicvsr.point_conv.0.weight", "basicvsr.spynet.mean"} <= keys
    assert tuple(m.state_dict()["cleaner.resblock.conv.0.weight"].shape) == (64, 3, 3, 3)
    with pytest.raises(KeyError):
        RealBasicVSR(2, 64)                              # mid_channels must be a keyword: the reference reads kwargs["mid_channels"] (realbasicvsr.py:8)


def test_engine_parameter_order_is_the_abi_order():
    from vsrlab_amd._order import basicvsr_keys, spynet_keys
    keys, n_train = basicvsr_keys(30)
    assert len(keys) == 316 and n_train == 254
    assert keys[0] == "backward_resblocks.conv.0.weight" and keys[2] == "backward_resblocks.res_block.0.conv1.weight"
    assert keys[122] == "forward_resblocks.conv.0.weight" and keys[244] == "point_conv.0.weight"
    assert keys[-2:] == ["spynet.mean", "spynet.std"] and len(spynet_keys()) == 62
    assert set(keys) == set(O.basicvsr_param_shapes(64, 30, 4))


def test_c_abi_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "vsrlab_hip.h")).read()
    declared = set(re.findall(r"\b(vsr_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 15
    from vsrlab_amd import _lib
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    loaded = _lib.load()                                 # sets argtypes for every export
    assert loaded.vsr_abi_version() == 4
    assert loaded.vsr_status_string(-4) == b"workspace too small"


def test_debug_signatures_agree_with_the_hooks_one_declaration():
    """csrc/debug_hooks.h is what the compiler holds every hook's definition (and the host-check programs' calls) to; the ctypes rows
    of _lib.DEBUG_SIGNATURES must say the same, position by position.  No library and no GPU: the header is read as text."""
    from vsrlab_amd import _lib
    text = open(os.path.join(ROOT, "vsrlab_amd", "csrc", "debug_hooks.h")).read()
    text = re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)
    decls = re.findall(r"\bint\s+(vsr_debug_\w+)\s*\(([^)]*)\)\s*;", text)
    names = [n for n, _ in decls]
    assert len(names) == len(set(names)) == 43, sorted(n for n in names if names.count(n) > 1)
    assert set(names) == set(_lib.DEBUG_SIGNATURES) | set(_lib.OTHER_DEBUG_EXPORTS), set(names) ^ (set(_lib.DEBUG_SIGNATURES) | set(_lib.OTHER_DEBUG_EXPORTS))

    def c_class(param):
        if "*" in param:
            return "pointer"
        for words, cls in (("long long", ctypes.c_longlong), ("float", ctypes.c_float), ("double", ctypes.c_double), ("int", ctypes.c_int),
                           ("unsigned", ctypes.c_int)):
            if re.search(rf"\b{words}\b", param):
                return cls
        raise AssertionError(f"unclassified parameter {param!r}")

    def row_class(t):
        return "pointer" if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else t

    for name, params in decls:
        if name not in _lib.DEBUG_SIGNATURES:
            continue
        res, args = _lib.DEBUG_SIGNATURES[name]
        want = [c_class(p) for p in params.split(",") if p.strip() not in ("", "void")]
        assert res is ctypes.c_int and [row_class(t) for t in args] == want, name


def test_workspace_query_and_unsupported_configs_fail_loudly():
    from vsrlab_amd import _lib
    lib = _lib.load()
    d = _lib.BasicVSRDesc(1, 7, 540, 960, 64, 30, 4, _lib.DT_BF16)
    assert lib.vsr_basicvsr_num_params(ctypes.byref(d)) == 316
    train = lib.vsr_basicvsr_workspace_bytes(ctypes.byref(d), 1)
    infer = lib.vsr_basicvsr_workspace_bytes(ctypes.byref(d), 0)
    assert 100e9 < train < 200e9 and 3e9 < infer < 12e9   # sized for 288 GB of HBM3E
    # arena_mode 1 ("diet", ABI 3): <= 70 GiB for BASELINE config 2, i.e. two clips per GPU (round-2 VERDICT #8); inference ignores it
    diet = _lib.BasicVSRDesc(1, 7, 540, 960, 64, 30, 4, _lib.DT_BF16, 1)
    for mode in (1, 2):
        full_b, diet_b = lib.vsr_basicvsr_workspace_bytes(ctypes.byref(d), mode), lib.vsr_basicvsr_workspace_bytes(ctypes.byref(diet), mode)
        assert 0 < diet_b <= 70 * 2 ** 30 and diet_b < 0.65 * full_b, (mode, diet_b / 2 ** 30, full_b / 2 ** 30)
        # the full arena (r04: ONE set of trunk activation gradients for both directions, per-frame gradients into the reconstruction's shuffle layers: 131 -> 113 GiB): two clips fit 288 GB as well
        assert full_b <= 120 * 2 ** 30, (mode, full_b / 2 ** 30)
    assert lib.vsr_basicvsr_workspace_bytes(ctypes.byref(diet), 0) == infer
    assert lib.vsr_basicvsr_workspace_bytes(ctypes.byref(_lib.BasicVSRDesc(1, 7, 540, 960, 64, 30, 4, 1, 2)), 1) == 0
    # upscale 2 (one PixelShufflePack: basicvsr.py:19) is supported since round 4: two tensors fewer, a smaller arena
    up2 = _lib.BasicVSRDesc(1, 7, 540, 960, 64, 30, 2, _lib.DT_BF16)
    assert lib.vsr_basicvsr_num_params(ctypes.byref(up2)) == 314
    assert 0 < lib.vsr_basicvsr_workspace_bytes(ctypes.byref(up2), 1) < train
    for bad in (_lib.BasicVSRDesc(1, 7, 540, 960, 32, 30, 4, 1), _lib.BasicVSRDesc(1, 7, 540, 960, 64, 30, 3, 1),
                _lib.BasicVSRDesc(1, 7, 540, 960, 64, 30, 8, 1), _lib.BasicVSRDesc(1, 7, 540, 960, 64, 0, 4, 1)):
        assert lib.vsr_basicvsr_workspace_bytes(ctypes.byref(bad), 1) == 0


def test_no_cpu_fallback_anywhere():
    from vsrlab_amd import functional as VF
    from vsrlab_amd.core.losses import CharbonnierLoss
    from vsrlab_amd.core.modules.conv import ResidualConv
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.spynet import Spynet, flow_warp
    x = torch.rand(1, 2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BasicVSR(64, 1)(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Spynet()(x[:, 0], x[:, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_warp(torch.rand(1, 64, 8, 8), torch.zeros(1, 8, 8, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ResidualConv(64)(torch.rand(1, 64, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CharbonnierLoss()(torch.rand(4), torch.rand(4))
    assert VF.resolve_dtype("bf16") == 1 and VF.resolve_dtype(None) == 0
    os.environ["VSRLAB_AMD_DTYPE"] = "bf16"
    try:
        assert VF.resolve_dtype(None) == 1
    finally:
        del os.environ["VSRLAB_AMD_DTYPE"]
    with pytest.raises(ValueError):
        VF.resolve_dtype("fp8")


def test_hydra_target_alias_and_instantiate():
    import vsrlab_amd
    vsrlab_amd.install_as_vsrlab(force=True)
    try:
        m = vsrlab_amd.instantiate({"_target_": "vsrlab.vsr.models.RealBasicVSR.realbasicvsr.RealBasicVSR", "cleaning_blocks": 1,
                                    "mid_channels": 64, "upscale": 4, "res_blocks": 1, "pretrained_flow": False,
                                    "train_flow": False})               # conf/train/model/basicvsr.yaml keys
        assert type(m).__module__ == "vsrlab_amd.vsr.models.RealBasicVSR.realbasicvsr"
        sp = vsrlab_amd.instantiate({"_target_": "vsrlab.optical_flow.models.spynet.SpyNet", "k": 6})
        assert len(sp.state_dict()) == 60 and "units.0.module.0.weight" in sp.state_dict()   # optical_flow/models/spynet/model.py:9-80 keys
        vs = vsrlab_amd.instantiate({"_target_": "vsrlab.vsr.models.VRT.modules.spynet.SpyNet", "pretrained": False,
                                     "return_levels": [2, 3, 4, 5]})                          # conf/train/model/spynet.yaml
        assert len(vs.state_dict()) == 62 and "basic_module.0.basic_module.8.weight" in vs.state_dict()
        import importlib
        dmod = importlib.import_module("vsrlab.vsr.models.RealBasicVSR.modules.unet-discriminator")   # conf/train/gan.yaml:17
        d = dmod.UNetDiscriminator(in_ch=3, mid_ch=64)
        assert "conv_3.conv.weight_orig" in d.state_dict() and "conv_3.conv.weight_u" in d.state_dict()
        wa = importlib.import_module("vsrlab.vsr.models.VRT.modules.window_attention")
        assert hasattr(wa, "WindowAttention") and hasattr(wa, "compute_mask")
        grp = vsrlab_amd.instantiate({"_target_": "vsrlab.vsr.models.VRT.modules.tmsa.RTMSA", "dim": 120, "input_resolution": [2, 8, 8],
                                      "depth": 2, "num_heads": 6, "window_size": [2, 8, 8]})     # tmsa.py:204-251
        assert "residual_group.blocks.1.attn.qkv_self.weight" in grp.state_dict() and "linear.bias" in grp.state_dict()
    finally:
        for k in [k for k in sys.modules if k == "vsrlab" or k.startswith("vsrlab.")]:
            del sys.modules[k]


# ---- data-parallel path: stock DDP as in the reference (core/utils.py:147-151), gloo, world_size 2 ----
def _ddp_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from torch.nn.parallel import DistributedDataParallel
        from vsrlab_amd import functional as VF
        from vsrlab_amd.vsr.models.RealBasicVSR.modules import basicvsr as mod

        # CPU stand-in for the engine call, TEST ONLY: same signature, evaluated by the oracle, so that
        # DDP's hooks see the module's real parameter plumbing (order, frozen SPyNet, one autograd node).
        def fake_engine(lrs, params, n_trainable, mid, rb, up, pool, compute_dtype=None):
            from vsrlab_amd._order import basicvsr_keys
            keys, _ = basicvsr_keys(rb, up)
            return O.basicvsr_forward(dict(zip(keys, params)), lrs)

        VF.basicvsr_forward = fake_engine
        torch.manual_seed(100 + rank)                      # different init per rank: DDP must broadcast rank 0's
        m = mod.BasicVSR(64, 1, 4, False, False)
        ddp = DistributedDataParallel(m)
        lrs = torch.rand(1, 2, 3, 8, 8, generator=torch.Generator().manual_seed(7 + rank))   # one distinct clip per rank
        sr = ddp(lrs)
        sr.mean().backward()
        g = torch.cat([p.grad.flatten() for p in m.parameters() if p.requires_grad])
        w = torch.cat([p.detach().flatten() for p in m.parameters()])
        if rank == 0:
            torch.save({"g": g, "w": w, "sd": m.state_dict()}, out)
        gs = [torch.zeros_like(g) for _ in range(world)]
        dist.all_gather(gs, g)
        assert torch.equal(gs[0], gs[1])                   # identical averaged gradient on every rank
        assert all(p.grad is None for k, p in m.named_parameters() if "spynet" in k)
    finally:
        dist.destroy_process_group()


def test_ddp_gloo_world2_gradients_are_the_mean_over_ranks(tmp_path):
    out = str(tmp_path / "rank0.pt")
    port = 29500 + os.getpid() % 2000
    mp.spawn(_ddp_worker, args=(2, port, out), nprocs=2, join=True)
    got = torch.load(out, weights_only=True)
    sd = got["sd"]
    grads = []
    for r in range(2):
        leaves = {k: v.clone().requires_grad_(v.is_floating_point() and "spynet" not in k) for k, v in sd.items()}
        lrs = torch.rand(1, 2, 3, 8, 8, generator=torch.Generator().manual_seed(7 + r))
        O.basicvsr_forward(leaves, lrs).mean().backward()
        from vsrlab_amd._order import basicvsr_keys
        keys, n_train = basicvsr_keys(1)
        order = [k for k in sd if k in set(keys[:n_train])]                # module.parameters() order
        grads.append(torch.cat([leaves[k].grad.flatten() for k in order]))
    want = 0.5 * (grads[0] + grads[1])
    assert float((got["g"] - want).abs().max() / want.abs().max()) < 1e-5


# ---- MI355X-first data-parallel path: ONE all-reduce over the flat gradient arena per optimizer step ----
def _flat_sync_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(2)
        from vsrlab_amd import functional as VF
        from vsrlab_amd.core.utils import update_weights
        from vsrlab_amd.parallel import FlatGradSync
        from vsrlab_amd.vsr.models.RealBasicVSR.modules import basicvsr as mod

        def fake_engine(lrs, params, n_trainable, mid, rb, up, pool, compute_dtype=None):     # TEST ONLY, see _ddp_worker
            from vsrlab_amd._order import basicvsr_keys
            keys, _ = basicvsr_keys(rb, up)
            return O.basicvsr_forward(dict(zip(keys, params)), lrs)

        VF.basicvsr_forward = fake_engine
        torch.manual_seed(200 + rank)                      # different init per rank: the start-up broadcast must fix it
        m = mod.BasicVSR(64, 1, 4, False, False)
        train = [p for p in m.parameters() if p.requires_grad]
        # the arenas FusedAdam builds on the GPU, restated with CPU tensors (the optimizer itself has no CPU path)
        n = sum(p.numel() for p in train)
        flat_p, flat_g = torch.zeros(n), torch.zeros(n)
        o = 0
        with torch.no_grad():
            for p in train:
                flat_p[o:o + p.numel()].copy_(p.reshape(-1))
                p.data = flat_p[o:o + p.numel()].view(p.shape)
                p.grad = flat_g[o:o + p.numel()].view(p.shape)
                o += p.numel()
        sync = FlatGradSync(flat_g, params=flat_p)
        w0 = flat_p.clone()
        opt = torch.optim.SGD(train, lr=0.1)
        opt.zero_grad = lambda *a, **k: flat_g.zero_()    # keep the .grad views (what FusedAdam.zero_grad does)
        num_grad_acc = 2
        for i in range(num_grad_acc):                      # conf/experiment/basic.yaml:26 style accumulation
            lrs = torch.rand(1, 2, 3, 8, 8, generator=torch.Generator().manual_seed(31 + 10 * rank + i))
            loss = m(lrs).mean()
            if i == num_grad_acc - 1:
                g_before = None
            update_weights(m, loss, None, None, opt, num_grad_acc, 1e9, i, grad_sync=sync)
            if i == 0:
                assert sync.num_collectives == 0           # no_sync on the non-final micro-step
        assert sync.num_collectives == 1
        ws = [torch.zeros_like(flat_p) for _ in range(world)]
        dist.all_gather(ws, flat_p)
        assert torch.equal(ws[0], ws[1])                   # replicas stay identical
        if rank == 0:
            torch.save({"w0": w0, "w1": flat_p.clone(), "sd": {k: v.clone() for k, v in m.state_dict().items()}}, out)
    finally:
        dist.destroy_process_group()


def test_flat_grad_sync_gloo_world2_with_accumulation_and_no_sync(tmp_path):
    out = str(tmp_path / "rank0.pt")
    port = 31500 + os.getpid() % 2000
    mp.spawn(_flat_sync_worker, args=(2, port, out), nprocs=2, join=True)
    got = torch.load(out, weights_only=True)
    # expected update: w1 = w0 - lr * mean over ranks of sum over micro-steps of grad(loss / num_grad_acc), from rank 0's weights
    from vsrlab_amd._order import basicvsr_keys
    from vsrlab_amd.vsr.models.RealBasicVSR.modules import basicvsr as mod
    torch.manual_seed(200)
    m = mod.BasicVSR(64, 1, 4, False, False)
    sd0 = m.state_dict()
    keys, n_train = basicvsr_keys(1)
    order = [k for k, p in m.named_parameters() if p.requires_grad]
    total = None
    for r in range(2):
        for i in range(2):
            leaves = {k: v.clone().requires_grad_(k in set(order)) for k, v in sd0.items()}
            lrs = torch.rand(1, 2, 3, 8, 8, generator=torch.Generator().manual_seed(31 + 10 * r + i))
            (O.basicvsr_forward(leaves, lrs).mean() / 2).backward()
            g = torch.cat([leaves[k].grad.flatten() for k in order])
            total = g if total is None else total + g
    upd, want = got["w1"] - got["w0"], -0.1 * (total / 2)
    assert float((upd - want).norm() / want.norm()) < 1e-3            # fp32 noise of two CPU evaluations (2 vs N threads)
    assert float((got["w0"] - torch.cat([sd0[k].flatten() for k in order])).abs().max()) == 0.0   # rank 0's weights were broadcast


def test_training_glue_has_no_cpu_fallback():
    from vsrlab_amd.core.utils import resize
    from vsrlab_amd.optim import FusedAdam
    with pytest.raises(RuntimeError):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(RuntimeError):
        resize(torch.zeros(1, 3, 8, 8), (2, 2))


# ---- round-2 ADVICE: gradients that autograd left outside the arena are gathered BEFORE the exchange ----
def _foreign_grad_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vsrlab_amd.optim import FusedAdam
        from vsrlab_amd.parallel import FlatGradSync
        torch.manual_seed(5)
        lin = torch.nn.Linear(6, 3)
        train = list(lin.parameters())
        n = sum(p.numel() for p in train)
        flat_g = torch.zeros(n)

        class Arena:                                       # FusedAdam's arena bookkeeping on CPU tensors, its REAL gather method
            gather_foreign_grads = FusedAdam.gather_foreign_grads

        arena = Arena()
        arena._params = train
        o = 0
        for p in train:
            p._vsr_grad_slot = flat_g[o:o + p.numel()].view(p.shape)
            p.grad = p._vsr_grad_slot
            o += p.numel()
        sync = FlatGradSync(flat_g, optimizer=arena)
        lin.zero_grad()                                    # nn.Module.zero_grad: set_to_none=True -> autograd will allocate fresh .grad tensors
        assert all(p.grad is None for p in train)
        flat_g.fill_(123.0)                                # stale arena contents that must NOT be exchanged
        x = torch.rand(4, 6, generator=torch.Generator().manual_seed(50 + rank))
        lin(x).square().mean().backward()
        local = torch.cat([p.grad.flatten() for p in train]).clone()
        assert all(p.grad.data_ptr() != p._vsr_grad_slot.data_ptr() for p in train)
        sync.all_reduce()
        assert all(p.grad.data_ptr() == p._vsr_grad_slot.data_ptr() for p in train)      # re-pointed at the arena
        locs = [torch.zeros_like(local) for _ in range(world)]
        dist.all_gather(locs, local)
        want = 0.5 * (locs[0] + locs[1])
        assert float((flat_g - want).abs().max()) < 1e-6, float((flat_g - want).abs().max())
        if rank == 0:
            torch.save({"ok": torch.ones(1)}, out)
    finally:
        dist.destroy_process_group()


def test_flat_grad_sync_gathers_foreign_gradients_before_the_exchange(tmp_path):
    out = str(tmp_path / "ok.pt")
    port = 33500 + os.getpid() % 2000
    mp.spawn(_foreign_grad_worker, args=(2, port, out), nprocs=2, join=True)
    assert os.path.exists(out)


def test_drop_path_is_the_references_stochastic_depth():
    """TMSA(drop_path > 0) (tmsa.py:57,103,110): DropPath restated (stochastic_depth.py:4-23): same CPU-generator draw per sample,
    kept samples scaled by 1 / keep_prob, identity in eval; TMSA / TMSAG accept the argument like the reference's."""
    from vsrlab_amd.vsr.models.VRT.modules.tmsa import DropPath, TMSA, TMSAG
    x = torch.randn(6, 3, 4, 5)
    dp = DropPath(0.4)
    dp.eval()
    assert torch.equal(dp(x), x)
    dp.train()
    torch.manual_seed(11)
    got = dp(x)
    torch.manual_seed(11)
    keep = 0.6
    r = (keep + torch.rand((6, 1, 1, 1))).floor_()          # the reference's formula, verbatim semantics
    assert torch.equal(got, x.div(keep) * r)
    assert 0 < int(r.sum()) < 6                              # the seed drops some samples and keeps some
    blk = TMSA(dim=24, input_resolution=(2, 8, 8), num_heads=2, window_size=(2, 8, 8), drop_path=0.25)
    assert isinstance(blk.drop_path, DropPath) and blk.drop_path.drop_prob == 0.25
    grp = TMSAG(dim=24, input_resolution=(2, 8, 8), depth=2, num_heads=2, window_size=[2, 8, 8], drop_path=[0.0, 0.3])
    assert isinstance(grp.blocks[0].drop_path, torch.nn.Identity) and grp.blocks[1].drop_path.drop_prob == 0.3


def test_chain_work_distribution_hands_out_every_tile_of_every_layer_once():
    """conv3x3_chain.hip, "Work distribution": the position -> (layer, tile) map the chain kernel's workgroups pull their work from,
    evaluated on the host (vsr_debug_chain_item).  For R = 8 regions and R = 1, tile counts from 1 to the 540p frame's 2040
    (also fewer tiles than regions, and a batch of two): every item of every layer exactly once over all regions, -1 behind the
    last layer, and within a region the layer never goes back (the progress argument of the kernel rests on these two)."""
    from vsrlab_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    f = lib.vsr_debug_chain_item
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    for (tiles, ntx, nlayers) in [(1, 1, 3), (5, 2, 4), (8, 2, 2), (9, 3, 3), (16, 2, 5), (61, 30, 2), (275, 11, 3), (2040, 30, 2), (4080, 30, 2)]:
        for R in (1, 8):
            seen = set()
            for own in range(R):
                last_layer, P = 0, 0
                while True:
                    it = f(P, own, R, tiles, ntx, nlayers)
                    if it < 0:
                        break
                    assert 0 <= it < tiles * nlayers and it not in seen, (tiles, ntx, nlayers, R, own, P, it)
                    seen.add(it)
                    assert it // tiles >= last_layer, (tiles, R, own, P)
                    last_layer = it // tiles
                    P += 1
                assert all(f(P + k, own, R, tiles, ntx, nlayers) < 0 for k in range(1, 40))
            assert len(seen) == tiles * nlayers, (tiles, ntx, nlayers, R, len(seen))


def test_chain_abi_rejects_bad_arguments_without_touching_the_gpu():
    from vsrlab_amd import _lib
    lib = _lib.load()
    assert lib.vsr_conv3x3_c64_chain_sync_bytes(0, 1, 8, 8) == 0 and lib.vsr_conv3x3_c64_chain_sync_bytes(65, 1, 8, 8) == 0
    assert lib.vsr_conv3x3_c64_chain_sync_bytes(60, 1, 540, 960) == 1024 + 60 * 2040 * 16
    assert lib.vsr_conv3x3_c64_chain_fwd(None, None, None, 2, 1, 8, 8, None, None) == -1
    # misaligned operands: refused (offsets are in units of 256 bytes from one base), before any launch
    assert lib.vsr_conv3x3_c64_chain_fwd(0x10000100, 0x20000000, 0x30000010, 2, 1, 8, 8, 0x40000000, None) == -2


def test_bench_dump_outputs_writes_float_arrays_within_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: loss (float64), a seeded sample of sr and the flat trainable parameters / Adam exp_avg (float32),
    full below the element caps and the same seeded sample on every call above them; the headline configuration stays < 64 MB."""
    import numpy as np
    import bench
    # BasicVSR(64, 30) with train_flow: 6.29 M trainable values, plus the sr sample and the loss
    assert (bench.DUMP_SR_SAMPLES + 2 * min(6_291_311, bench.DUMP_MAX_ELEMS)) * 4 + 8 < 64e6
    from vsrlab_amd.vsr.models.RealBasicVSR.modules.basicvsr import BasicVSR
    torch.manual_seed(0)
    m = BasicVSR(16, 2, 4, False, False)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-4)
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    sr = torch.rand(1, 3, 3, 512, 512)                   # 2.4 M values > DUMP_SR_SAMPLES
    flat_p = torch.cat([p.detach().reshape(-1) for p in params])
    flat_m = torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in params])

    def dump(d):
        bench.dump_outputs(str(d), torch.tensor(0.25), sr, m, opt)
        return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}

    a = dump(tmp_path / "a")
    assert sorted(a) == ["adam_exp_avg", "loss", "params", "sr_sample"]
    assert a["loss"].dtype == np.float64 and a["loss"].tolist() == [0.25]
    assert all(a[k].dtype == np.float32 for k in ("adam_exp_avg", "params", "sr_sample"))
    assert a["sr_sample"].shape == (bench.DUMP_SR_SAMPLES,) and np.isin(a["sr_sample"], sr.numpy()).all()
    assert np.array_equal(a["params"], flat_p.numpy()) and np.array_equal(a["adam_exp_avg"], flat_m.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    b, c = dump(tmp_path / "b"), dump(tmp_path / "c")
    assert b["params"].shape == (1000,) and np.isin(b["params"], flat_p.numpy()).all()
    assert all(np.array_equal(b[k], c[k]) for k in b) and np.array_equal(a["sr_sample"], b["sr_sample"])


def test_functional_surface_is_the_parents():
    """vsrlab_amd.functional was one module and is a package by op family: tests/golden/functional_names.txt is the module's
    attribute surface as recorded before the split (name and kind; without dunders, imported modules and the standard library's
    typing names; ``_JPEG_DT`` under the name it was given then, ``_STORAGE_DT``).  Every name still resolves on the package with
    its kind, every function and class is defined in a submodule (``BasicVSRDesc``, which the module re-exported from ``_lib``,
    is still that class), and no two submodules define one name."""
    import ast
    import types
    from vsrlab_amd import _lib, functional as VF

    def kind(v):
        if isinstance(v, type):
            return "class"
        if isinstance(v, types.FunctionType):
            return "function"
        return "int" if isinstance(v, int) and not isinstance(v, bool) else "other"

    with open(os.path.join(ROOT, "tests", "golden", "functional_names.txt")) as f:
        listed = [line.split() for line in f.read().splitlines() if line]
    assert len(listed) == 110 and [n for n, _ in listed] == sorted(n for n, _ in listed)
    for name, want in listed:
        v = getattr(VF, name)                                # AttributeError: the name is gone
        assert kind(v) == want, (name, kind(v), want)
        if name == "BasicVSRDesc":
            assert v is _lib.BasicVSRDesc
        elif want in ("function", "class"):
            assert v.__module__.startswith("vsrlab_amd.functional."), (name, v.__module__)
    assert not hasattr(VF, "_JPEG_DT")
    owner = {}
    pkg = os.path.dirname(VF.__file__)
    for fname in sorted(os.listdir(pkg)):
        if not fname.endswith(".py") or fname == "__init__.py":
            continue
        with open(os.path.join(pkg, fname)) as f:
            body = ast.parse(f.read()).body
        for node in body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                names = [node.name]
            elif isinstance(node, ast.Assign):
                names = [t.id for t in node.targets if isinstance(t, ast.Name)]
            elif isinstance(node, ast.AnnAssign):
                names = [node.target.id]
            else:
                names = []
            for n in names:
                assert n not in owner, (n, owner[n], fname)
                owner[n] = fname
    assert {n for n, _ in listed} - {"BasicVSRDesc", "DT_BF16", "DT_F32"} == set(owner)
    # module state has one home: the package reads it there, it holds no copy
    assert owner["_ARENA_MODE"] == "basicvsr.py" and "_ARENA_MODE" not in vars(VF) and "_chain_timeouts_seen" not in vars(VF)
    VF.set_arena_mode("diet")
    try:
        assert VF._ARENA_MODE == VF.basicvsr._ARENA_MODE == 1 and VF.arena_mode() == 1
    finally:
        VF.set_arena_mode(None)
    assert VF._ARENA_MODE is None


def test_the_satellite_loaders_load_once_and_type_every_entry():
    from vsrlab_amd import _lib
    for load, table in ((_lib.load_spatial_corr, _lib.SPATIAL_CORR_SIGNATURES), (_lib.load_jpeg, _lib.JPEG_SIGNATURES),
                        (_lib.load_warp_taps, _lib.WARP_TAPS_SIGNATURES)):
        lib = load()
        assert load() is lib and lib is not _lib.load()
        for name, (res, args) in table.items():
            fn = getattr(lib, name)
            assert fn.restype is res and fn.argtypes == args, name
