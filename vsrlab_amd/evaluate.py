"""The evaluation loop of the reference's ``test.py`` (:123-144) as a function: a video goes through the model in windows of
frames and every window is scored by the metric collection."""
from __future__ import annotations

import torch

from .core.utils import compute_metric, running_metrics


def evaluate_video(model, video_lr: torch.Tensor, video_hr: torch.Tensor, metric, window_size: int = 32):
    """``video_lr`` (b, t, c, h, w) and ``video_hr`` (b, t, c, H, W) -> ``(sr_video, metrics)``.

    The model runs in ``eval()`` mode under ``torch.no_grad()`` on non-overlapping windows of ``window_size`` frames (the last one
    holds what is left); a model that returns a tuple gives its super-resolved clip first (RealBasicVSR returns ``(sr, lq)``).
    ``metrics`` averages the per-window results over the WINDOWS, as ``test.py`` does: every window weighs the same whatever its
    length, so a short last window counts as much as a full one.  ``sr_video`` is the windows' outputs concatenated along t.
    The model is left in eval mode."""
    if window_size < 1:
        raise ValueError(f"window_size must be positive, got {window_size}")
    if video_lr.dim() != 5 or video_hr.dim() != 5 or video_lr.shape[:2] != video_hr.shape[:2] or video_lr.shape[1] == 0:
        raise ValueError(f"expected (b, t, c, h, w) clips of one length, got {tuple(video_lr.shape)} and {tuple(video_hr.shape)}")
    model.eval()
    starts = range(0, video_lr.shape[1], window_size)
    totals, outputs = None, []
    with torch.no_grad():
        for i in starts:
            out = model(video_lr[:, i:i + window_size])
            sr = out[0] if isinstance(out, tuple) else out
            outputs.append(sr)
            hr = video_hr[:, i:i + window_size]
            totals = compute_metric(metric, sr, hr) if totals is None else running_metrics(totals, metric, sr, hr)
    return torch.cat(outputs, dim=1), {k: v / len(starts) for k, v in totals.items()}
