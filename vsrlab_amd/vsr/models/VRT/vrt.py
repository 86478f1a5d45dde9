"""The front of ``VRT.forward`` (vsrlab ``src/vsr/models/VRT/vrt.py:145-150``) on the HIP path, as module-level functions that mirror
the reference's methods, for the ``VRT`` class to bind when it lands: ``get_flows`` (:189-208), ``get_aligned_image`` (:211-228) and
``aligned_input``, the ``cat([x, x_backward, x_forward], 2)`` of :150 in one launch (csrc/warp_taps.hip).
``Stage``, ``VRT`` and ``TinyVRT`` themselves are not provided (README)."""
from .... import functional as VF
from .modules.spynet import flow_warp  # noqa: F401  (the reference imports it here, :9)

aligned_input = VF.aligned_input


def get_flows(optical_flow, x):
    """Flow between frames t and t+1 of ``x`` (B, D, C, H, W) at every level ``optical_flow`` returns (``VRT.get_flows`` with the
    network passed in place of ``self``): two lists of (B, D - 1, 2, H / 2^i, W / 2^i) views, backward then forward."""
    b, n, c, h, w = x.size()
    x_1 = x[:, :-1, :, :, :].reshape(-1, c, h, w)
    x_2 = x[:, 1:, :, :, :].reshape(-1, c, h, w)
    n_scales = len(optical_flow.return_levels)

    def views(flows):
        flows = flows if isinstance(flows, (list, tuple)) else [flows]      # SpyNet returns the tensor itself for one level
        return [flow.view(b, n - 1, 2, h // (2 ** i), w // (2 ** i)) for flow, i in zip(flows, range(n_scales))]

    flows_backward = views(optical_flow(x_1, x_2))
    flows_forward = views(optical_flow(x_2, x_1))
    return flows_backward, flows_forward


def get_aligned_image(x, flows_backward, flows_forward):
    """``VRT.get_aligned_image`` (static, :211-228): ``[x_backward, x_forward]``, each (B, D, 4 C, H, W): the 'nearest4' warps of the
    neighbouring frames and a zero block at the clip's end.  Both are channel slices of ``aligned_input``'s result: one launch, and
    nothing is copied."""
    c = x.size(2)
    out = aligned_input(x, flows_backward, flows_forward)
    return [out[:, :, c:5 * c], out[:, :, 5 * c:]]
