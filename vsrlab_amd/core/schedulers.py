"""``CosineAnnealingLinearWarmup``, with the constructor and the semantics of the reference's core/schedulers.py: every cycle warms
up linearly from the floor rate to the cycle's peak and anneals back along half a cosine; from one cycle to the next the annealing
part grows by ``cycle_mult`` and the peak shrinks by ``gamma``.  Pure host code.  It writes one Python float per param group into
``param_group['lr']``, which is what ``core.utils.update_weights`` hands to the fused Adam step.

The optimizer's own rates are the peaks of the first cycle.  The floors are given (``min_lrs``, one per group) or derived
(``min_lrs_pow=k``: peak * 10 ** -k); exactly one of the two is passed.  On construction every group is set to its floor.
``step()`` advances by one; ``step(epoch)`` jumps to an absolute step, locating its cycle in closed form."""
import math
from typing import List, Optional

import torch
from torch.optim.lr_scheduler import _LRScheduler


class CosineAnnealingLinearWarmup(_LRScheduler):
    def __init__(self, optimizer: torch.optim.Optimizer, first_cycle_steps: int, min_lrs: Optional[List[float]] = None,
                 cycle_mult: float = 1., warmup_steps: int = 0, gamma: float = 1., last_epoch: int = -1,
                 min_lrs_pow: Optional[int] = None):
        assert warmup_steps < first_cycle_steps, "Warmup steps should be smaller than first cycle steps"
        assert (min_lrs is None) != (min_lrs_pow is None), "Only one of min_lrs and min_lrs_pow should be specified"
        peaks = [group["lr"] for group in optimizer.param_groups]
        floors = [peak * (10 ** -min_lrs_pow) for peak in peaks] if min_lrs is None else list(min_lrs)
        if len(floors) != len(peaks):
            raise ValueError(f"{len(floors)} minimum rates for {len(peaks)} param groups")
        # attribute names as in the reference: they are the scheduler's state_dict
        self.first_cycle_steps, self.cycle_mult, self.warmup_steps, self.gamma = first_cycle_steps, cycle_mult, warmup_steps, gamma
        self.base_max_lrs = peaks                   # peaks of the first cycle
        self.max_lrs = peaks                        # peaks of the current cycle
        self.min_lrs = floors
        self.cur_cycle_steps = first_cycle_steps    # length of the current cycle
        self.cycle = 0
        self.step_in_cycle = last_epoch
        super().__init__(optimizer, last_epoch)     # (takes one step, to step 0)
        self.init_lr()

    def init_lr(self):
        """every group at its floor, which is also what the warm-up starts from"""
        self.base_lrs = list(self.min_lrs)
        for group, floor in zip(self.optimizer.param_groups, self.base_lrs):
            group["lr"] = floor

    def _rate(self, peak, floor):
        s, warm = self.step_in_cycle, self.warmup_steps
        if s < warm:
            return (peak - floor) * s / warm + floor
        return floor + (peak - floor) * (1 + math.cos(math.pi * (s - warm) / (self.cur_cycle_steps - warm))) / 2

    def get_lr(self):
        if self.step_in_cycle == -1:
            return self.base_lrs
        return [self._rate(peak, floor) for peak, floor in zip(self.max_lrs, self.base_lrs)]

    def _advance(self):
        self.step_in_cycle += 1
        if self.step_in_cycle >= self.cur_cycle_steps:              # a restart: the annealing part grows, the warm-up does not
            self.step_in_cycle -= self.cur_cycle_steps
            self.cycle += 1
            self.cur_cycle_steps = int((self.cur_cycle_steps - self.warmup_steps) * self.cycle_mult) + self.warmup_steps

    def _jump(self, epoch):
        first, mult = self.first_cycle_steps, self.cycle_mult
        if epoch < first:
            self.cur_cycle_steps, self.step_in_cycle = first, epoch
        elif mult == 1.:
            self.cycle, self.step_in_cycle = divmod(epoch, first)
        else:
            # cycles of first * mult^k steps: n whole cycles hold first (mult^n - 1) / (mult - 1) steps
            n = int(math.log(epoch / first * (mult - 1) + 1, mult))
            self.cycle = n
            self.step_in_cycle = epoch - int(first * (mult ** n - 1) / (mult - 1))
            self.cur_cycle_steps = first * mult ** n

    def step(self, epoch=None):
        if epoch is None:
            epoch = self.last_epoch + 1
            self._advance()
        else:
            self._jump(epoch)
        self.max_lrs = [peak * (self.gamma ** self.cycle) for peak in self.base_max_lrs]
        self.last_epoch = math.floor(epoch)
        for group, lr in zip(self.optimizer.param_groups, self.get_lr()):
            group["lr"] = lr
        self._last_lr = [group["lr"] for group in self.optimizer.param_groups]
