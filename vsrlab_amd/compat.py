"""Make the reference's Hydra ``_target_`` strings resolve to this package.

``install_as_vsrlab()`` registers ``vsrlab_amd`` (and its sub-packages) under the name ``vsrlab`` in
``sys.modules`` -- the reference maps ``vsrlab`` to its ``src/`` the same way (setup.py:6-7) -- so
``vsrlab.vsr.models.RealBasicVSR.realbasicvsr.RealBasicVSR`` (conf/train/model/basicvsr.yaml:1)
instantiates the HIP-backed module with no YAML change.  ``instantiate`` is a 10-line stand-in for
``hydra.utils.instantiate(cfg, _recursive_=False)`` (core/utils.py:138) for hosts without Hydra."""
import importlib
import sys


def install_as_vsrlab(force: bool = False) -> None:
    import vsrlab_amd
    if "vsrlab" in sys.modules and sys.modules["vsrlab"] is not vsrlab_amd and not force:
        raise RuntimeError("a different `vsrlab` package is already imported; pass force=True to shadow it")
    sys.modules["vsrlab"] = vsrlab_amd
    for sub in ("core", "core.modules", "core.modules.conv", "core.modules.upsampling", "core.modules.correlation", "core.modules.dct_transforms", "core.modules.mlp",
                "core.schedulers", "core.losses", "vsr", "vsr.models",
                "vsr.models.RealBasicVSR", "vsr.models.RealBasicVSR.realbasicvsr", "vsr.models.RealBasicVSR.modules",
                "vsr.models.RealBasicVSR.modules.basicvsr", "vsr.models.RealBasicVSR.modules.spynet",
                "vsr.models.RealBasicVSR.modules.unet-discriminator", "vsr.models.VRT", "vsr.models.VRT.vrt", "vsr.models.VRT.modules",
                "vsr.models.VRT.modules.spynet", "vsr.models.VRT.modules.window_attention", "vsr.models.VRT.modules.tmsa", "vsr.models.VRT.modules.deform_conv",
                "core.utils", "core.metrics", "core.augmentations", "train_gan", "optical_flow",
                "optical_flow.models", "optical_flow.models.spynet", "optical_flow.models.raft", "optical_flow.models.raft.raft",
                "optical_flow.models.raft.corr", "optical_flow.models.raft.extractor", "optical_flow.models.raft.update",
                "optical_flow.models.raft.utils", "optical_flow.models.irr", "optical_flow.models.irr.pwc_modules"):
        sys.modules["vsrlab." + sub] = importlib.import_module("vsrlab_amd." + sub)


def install_metrics_as_piqa() -> bool:
    """Opt-in: make ``_target_: piqa.PSNR`` / ``piqa.SSIM`` (conf/train/default.yaml:8-14) resolve to ``vsrlab_amd.core.metrics``
    on a host WITHOUT piqa, by registering a module named ``piqa`` that exposes those two classes and nothing else.  Where the
    real piqa can be imported nothing is registered and False is returned; nothing in this package calls this function."""
    import types
    from importlib.util import find_spec
    from .core import metrics
    present = sys.modules.get("piqa")
    if present is not None:
        return getattr(present, "PSNR", None) is metrics.PSNR
    if find_spec("piqa") is not None:
        return False
    mod = types.ModuleType("piqa")
    mod.__doc__ = "vsrlab_amd.core.metrics under piqa's name (vsrlab_amd.compat.install_metrics_as_piqa)"
    mod.PSNR, mod.SSIM = metrics.PSNR, metrics.SSIM
    sys.modules["piqa"] = mod
    return True


def instantiate(cfg: dict):
    """``{'_target_': 'pkg.mod.Class', **kwargs}`` -> ``Class(**kwargs)``."""
    cfg = dict(cfg)
    target = cfg.pop("_target_")
    mod, _, name = target.rpartition(".")
    return getattr(importlib.import_module(mod), name)(**cfg)
