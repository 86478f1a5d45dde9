"""The flow warp's launches (csrc/elementwise.hip), one at a time, against the fp64 restatement of tests/flow_warp_common.py: every output
element inside the bound stated there (grid family: equal to the reference, or to its bf16 rounding), every input's padding pixels NaN,
the flow in a NaN-filled buffer with images 2HW and 3 x 2HW floats apart whose bits must not change, every output between sentinel
bands, ``dflow`` with sentinel gaps, S all zero after every gather call and the far counter the reference's count.  The launches go through
the ``vsr_debug_warp_*`` hooks (csrc/warp_hooks.hip), i.e. through the launchers the engines and the per-op entries call.

Which case reaches which code:
  warp_fwd_kernel                         test_forward; zeros and border; over the cap at (2,259,261) x 64 channels
  warp_bwd_kernel + add_cast_kernel       test_scatter_adjoint; `a` given and NULL; over the cap at (2,259,261)
  warp_bwd_gather_kernel, warp_bwd_far_kernel    test_gather_adjoint: against fp64 (no other HIP kernel in the comparison), dtop given and NULL,
                                          the hit list and the `cnt > GCAP` rescan at the sink patch, the near / far split at exactly 4.0 (grid
                                          family), bit-identical on a repeat; 4290 tiles and the far kernel's second pass at (1,1030,1030)
  warp_bwd_flow_kernel                    test_flow_gradient; the open border gate at p == 0 and p == dim - 1 (grid family), dflow on the flow's stride
  planar_to_pm_kernel, pm_to_planar_kernel, add_cast_kernel    test_converters_and_add_cast
Shapes (N, H, W): the tail's list, (2,1,45) and (1,9,1) (extent 1: the position is 0 whatever the flow), and the grid family's (2,9,33),
(1,17,65), (1,5,129)."""
import pytest
import torch

import hr_tail_common as T
import flow_warp_common as W

pytestmark = pytest.mark.gpu

places = pytest.mark.parametrize("place", W.PLACES, ids=lambda p: f"{T.sid(p[0])}-{p[1]}-c{p[2]}")


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need an MI355X")
    return torch.device("cuda:0")


def _run_all(hook, place, dev):
    """Every case of the hook at this place in both dtypes (the dtype innermost: the two builds share one cached reference)."""
    shape, fam, C = place
    got = {}
    for c0 in W.hook_cases(hook, shape, C, fam):
        for dt in ("bf16", "fp32"):
            c = W.Case(c0.hook, c0.shape, dt, c0.opts)
            got[c] = W.run_hip(c, dev)
            W.check(c, got[c])
    return got


@places
def test_forward(place):
    _run_all("fwd", place, _gpu())


@places
def test_scatter_adjoint(place):
    """vsr_launch_warp_bwd into a zeroed fp32 accumulator, then vsr_launch_add_cast."""
    _run_all("scatter", place, _gpu())


@places
def test_gather_adjoint(place):
    """The gather form against fp64, and equal to itself on a repeat bit for bit (the far share is fixed point) at every width."""
    dev = _gpu()
    for c, v in _run_all("gather", place, dev).items():
        assert W.same_bits(v, W.run_hip(c, dev)), c.name


@places
def test_flow_gradient(place):
    _run_all("flowgrad", place, _gpu())


@pytest.mark.parametrize("c", W.over_cap_cases(), ids=lambda c: c.name)
def test_over_the_cap(c):
    """One launch each, bf16: more chunks (forward, scatter) or pixels (gather + far, flow gradient) than 4096 workgroups x 256 threads,
    so the grid-stride loops take a second pass.  The fp64 reference of these shapes takes about a second: every row is checked."""
    W.check(c, W.run_hip(c, _gpu()))


@pytest.mark.parametrize("shape", [(2, 13, 37), (1, 3, 66), (1, 9, 31), (1, 17, 100)], ids=T.sid)
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_converters_and_add_cast(shape, dtype):
    """planar_to_pm then pm_to_planar at Cin 3 of 16, 8 of 16 and 64 of 64: the values are the round-to-nearest-even of the input, the
    channels from Cin on are 0, the padding pixels still hold the sentinel.  add_cast with `a` NULL, `s` NULL and both given equals
    T(a + s), the sum in fp32 on the CPU, bit for bit."""
    dev = _gpu()
    n, h, w = shape
    store = T.bf16_round if dtype == "bf16" else (lambda v: v)
    g = torch.Generator().manual_seed(5 + h + w)
    for cin, C in ((3, 16), (8, 16), (64, 64)):
        x = torch.randn(n, cin, h, w, generator=g)
        pm, back, pad_ok = W.run_converters(x, C, dtype, dev)
        want = torch.cat([store(x), torch.zeros(n, C - cin, h, w)], 1)
        assert torch.equal(pm, want) and torch.equal(back, want) and pad_ok, (cin, C)
    for C in (16, 64):
        a, s = T.draw(7 + C, n, C, h, w), torch.randn(n, C, h, w, generator=g)
        for aa, ss in ((None, s), (a, None), (a, s)):
            want = aa if aa is not None else torch.zeros_like(s)        # the kernel: v = a or 0; v += s if s is given
            want = store(want + ss if ss is not None else want)
            got = W.run_add_cast(aa, ss, dtype, dev)
            assert T.same_bits(dict(v=got), dict(v=want)), (C, aa is None, ss is None)
