"""RAFT-small's feature / context encoder (reference ``raft/extractor.py``: ``BottleneckBlock``, ``SmallEncoder``), same
constructor arguments and ``state_dict`` keys.  The full-size ``BasicEncoder`` belongs to ``RAFT(small=False)``, which is not
offered (no weights exist for it)."""
import torch
import torch.nn as nn


def _norm(norm_fn, planes):
    if norm_fn == 'instance':
        return nn.InstanceNorm2d(planes)
    if norm_fn == 'none':
        return nn.Sequential()
    raise NotImplementedError(f"RAFT-small uses norm_fn 'instance' or 'none', got {norm_fn!r}")


def _init_like_reference(module):
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
        elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
            if m.weight is not None:
                nn.init.constant_(m.weight, 1)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)


class BottleneckBlock(nn.Module):
    """1x1 (planes / 4) -> 3x3 (stride) -> 1x1 (planes), each normalised and rectified, plus the (strided 1x1) identity."""

    def __init__(self, in_planes, planes, norm_fn='instance', stride=1):
        super().__init__()
        mid = planes // 4
        self.conv1 = nn.Conv2d(in_planes, mid, kernel_size=1, padding=0)
        self.conv2 = nn.Conv2d(mid, mid, kernel_size=3, padding=1, stride=stride)
        self.conv3 = nn.Conv2d(mid, planes, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.norm1, self.norm2, self.norm3 = _norm(norm_fn, mid), _norm(norm_fn, mid), _norm(norm_fn, planes)
        self.downsample = None
        if stride != 1:
            self.norm4 = _norm(norm_fn, planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm4)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        y = self.relu(self.norm3(self.conv3(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class SmallEncoder(nn.Module):
    """7x7 stride-2 stem (32) and three pairs of bottleneck blocks (32, 64 / 2, 96 / 2), then a 1x1 to ``output_dim``: 1/8
    resolution.  A list or tuple of two batches is encoded in one pass and split again."""

    def __init__(self, output_dim=128, norm_fn='batch'):
        super().__init__()
        self.norm_fn = norm_fn
        self.norm1 = _norm(norm_fn, 32)
        self.conv1 = nn.Conv2d(3, 32, kernel_size=7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = 32
        self.layer1 = self._make_layer(32, stride=1)
        self.layer2 = self._make_layer(64, stride=2)
        self.layer3 = self._make_layer(96, stride=2)
        self.conv2 = nn.Conv2d(96, output_dim, kernel_size=1)
        _init_like_reference(self)

    def _make_layer(self, dim, stride=1):
        blocks = (BottleneckBlock(self.in_planes, dim, self.norm_fn, stride=stride), BottleneckBlock(dim, dim, self.norm_fn, stride=1))
        self.in_planes = dim
        return nn.Sequential(*blocks)

    def forward(self, x):
        pair = isinstance(x, (tuple, list))
        if pair:
            sizes = [t.shape[0] for t in x]
            x = torch.cat(list(x), dim=0)
        x = self.relu1(self.norm1(self.conv1(x)))
        x = self.conv2(self.layer3(self.layer2(self.layer1(x))))
        return torch.split(x, sizes, dim=0) if pair else x
