"""Generate tests/golden/token_mixer.npz from the REAL reference (its ``EncoderDCT`` / ``DecoderIDCT``, ``MlpMixer`` and
``CosineAnnealingLinearWarmup``).  Needs a checkout of the reference (santurini/vsrlab) and ``einops``, which its transforms
import; pass its ``src`` directory, from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mixer.py PATH/TO/vsrlab/src

The reference is imported under its ``vsrlab`` alias with the in-memory stubs of make_golden_raft.py.  Everything runs in fp64 on
the CPU on the inputs of tests/mixer_common.py; only the reference's OUTPUTS are stored (tensors above mixer_common.FULL elements as
a sub-sample plus three statistics), under 128 KiB:

(1) per transform case ``dct{i}``: encoder output and d clip, decoder output and d tokens, under seeded cotangents; the transform
    weight per block size (fp32, as the reference holds it); the ``state_dict`` keys and shapes of both modules.
(2) per Mixer case: output, d input and all 12 * blocks parameter gradients with the seeded weights; 'e2e' runs
    ``DecoderIDCT(mixer(EncoderDCT(clip)))``; the ``state_dict`` keys and shapes.
(3) the learning-rate sequences of mixer_common.SCHEDULER_CASES."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import mixer_common as MC  # noqa: E402
from make_golden_raft import import_reference  # noqa: E402


def key_record(store, tag, module):
    sd = module.state_dict()
    store[tag + "__keys"] = np.array(list(sd))
    store[tag + "__shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])


def main(ref_src):
    import_reference(ref_src)
    dct = importlib.import_module("vsrlab.core.modules.dct_transforms")
    mlp = importlib.import_module("vsrlab.core.modules.mlp")
    sched = importlib.import_module("vsrlab.core.schedulers")
    store = {}

    # (1) the transforms
    for i, (ps, b, t, h, w) in enumerate(MC.DCT_CASES):
        enc, dec = dct.EncoderDCT(ps), dct.DecoderIDCT(3, ps, h, w)
        store[f"weight_ps{ps}"] = enc.weight.numpy().astype(np.float32)
        assert torch.equal(enc.dct_conv.weight, dec.reverse_dct.weight) and torch.equal(enc.dct_conv.weight, torch.cat([enc.weight] * 3))
        if i == 0:
            key_record(store, "encoder", enc)
            key_record(store, "decoder", dec)
        enc, dec = enc.double(), dec.double()
        x, cy, tok, cx = (v.double() for v in MC.dct_inputs(i))
        x.requires_grad_(True), tok.requires_grad_(True)
        y = enc(x)
        (y * cy).sum().backward()
        img = dec(tok)
        (img * cx).sum().backward()
        for k, v in (("enc_out", y), ("enc_dx", x.grad), ("dec_out", img), ("dec_dtok", tok.grad)):
            MC.put(store, f"dct{i}__{k}", v)
        print(f"(1) dct{i} ps={ps}: tokens {tuple(y.shape)}, frames {tuple(img.shape)}")

    # (2) the Mixer
    for name, (args, shape) in MC.MIXER_CASES.items():
        model = mlp.MlpMixer(*args)
        key_record(store, "mixer_" + name, model)
        model.load_state_dict(MC.mixer_params(name), strict=True)
        model = model.double()
        x, cot = (v.double() for v in MC.mixer_inputs(name))
        x.requires_grad_(True)
        if name == "e2e":
            enc = dct.EncoderDCT(MC.E2E_PS).double()
            dec = dct.DecoderIDCT(3, MC.E2E_PS, *MC.E2E_CLIP[3:]).double()
            tok = enc(x)
            assert tuple(tok.shape) == shape, tok.shape
            out = dec(model(tok))
        else:
            out = model(x)
        (out * cot).sum().backward()
        MC.put(store, f"{name}__out", out)
        MC.put(store, f"{name}__dx", x.grad)
        for k, p in model.named_parameters():
            MC.put(store, f"{name}__grad__{k}", p.grad)
        print(f"(2) {name}: out {tuple(out.shape)}, {len(list(model.parameters()))} parameter gradients")

    # (3) the scheduler
    for name in MC.SCHEDULER_CASES:
        rows, _ = MC.scheduler_sequence(sched.CosineAnnealingLinearWarmup, name)
        store["sched__" + name] = np.array(rows, dtype=np.float64)
        print(f"(3) {name}: {len(rows)} rows, last {rows[-1]}")

    path = os.path.join(HERE, "token_mixer.npz")
    np.savez_compressed(path, **store)
    print("token_mixer.npz", len(store), "arrays,", os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 128 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
