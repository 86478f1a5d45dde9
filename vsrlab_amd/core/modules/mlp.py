"""``Mlp`` / ``MixerBlock`` / ``MlpMixer`` (reference core/modules/mlp.py) on the fused HIP residual axis MLP
(``core.token_ops.axis_mlp``).

The reference runs ``Linear -> GELU -> Linear -> add -> permute`` three times per block, and every permute leaves a non-contiguous
tensor for the next ``Linear`` to copy.  Here a block is three kernel calls on the one contiguous (b, t, p, c) tensor, each mixing
one axis where it lies.  Constructors and ``state_dict`` keys (``mixer.{i}.{time,patches,channels}_mlp.mlp.{0,2}.{weight,bias}``)
are the reference's."""
import torch.nn as nn

from ..token_ops import axis_mlp


class Mlp(nn.Module):
    def __init__(self, dim, in_dim):
        super(Mlp, self).__init__()
        # the reference's container: the two Linear layers hold the parameters, the kernel does the arithmetic
        self.mlp = nn.Sequential(nn.Linear(dim, in_dim),
                                 nn.GELU(),
                                 nn.Linear(in_dim, dim))

    def mix(self, x, axis, residual=True):
        """``x + mlp(x)`` (or ``mlp(x)``) along ``axis`` of ``x``, in x's layout"""
        return axis_mlp(x, axis, self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight, self.mlp[2].bias, residual=residual)

    def forward(self, x):
        """``mlp(x)`` along the last axis, no residual: what the reference's ``Mlp`` returns"""
        return self.mix(x, -1, residual=False)


class MixerBlock(nn.Module):
    def __init__(self, patches_dim, channels_dim, time_dim, exp):
        super(MixerBlock, self).__init__()
        self.time_mlp = Mlp(time_dim, exp * time_dim)
        self.patches_mlp = Mlp(patches_dim, exp * patches_dim)
        self.channels_mlp = Mlp(channels_dim, exp * channels_dim)

    def forward(self, x):
        """(b, t, p, c) -> (b, t, p, c), contiguous.  The reference returns the same values as a permuted view of a (b, c, p, t)
        tensor; contiguity is the one difference."""
        x = self.channels_mlp.mix(x, 3)
        x = self.patches_mlp.mix(x, 2)
        x = self.time_mlp.mix(x, 1)
        return x


class MlpMixer(nn.Module):
    def __init__(self, patches_dim, channels_dim, time_dim, exp, blocks):
        super().__init__()
        self.mixer = nn.Sequential(*[MixerBlock(patches_dim, channels_dim, time_dim, exp) for _ in range(blocks)])

    def forward(self, x):
        return self.mixer(x)
