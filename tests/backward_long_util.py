"""Shared by tests/test_gpu_backward_long.py and tests/test_backward_long_cpu.py: the relative-position bias of a window in its COMPACT form,
restated in torch (FV:243-258 + 276-299), so that the device-side reference can differentiate the compact table itself.

    index(q, k) = (yq - yk + w - 1) * (2w - 1) + (xq - xk + w - 1)      for tokens q, k >= ng (the bias window, raster order)
    bias(q, k)  = 0                                                       where q < ng or k < ng (carrier tokens / zero-padded grid part)
"""
import torch


def compact_index(w: int, ng: int, S: int, device=None):
    """(index [S][S] int64, has_bias [S][S] bool) of a w x w bias window behind ``ng`` leading tokens; ng + w * w == S."""
    assert ng >= 0 and ng + w * w == S
    t = torch.arange(S, device=device) - ng
    y, x = torch.div(t, w, rounding_mode="floor"), t % w
    idx = (y[:, None] - y[None, :] + w - 1) * (2 * w - 1) + (x[:, None] - x[None, :] + w - 1)
    has = (t[:, None] >= 0) & (t[None, :] >= 0)
    return torch.where(has, idx, torch.zeros_like(idx)), has


def gather_compact(rel: torch.Tensor, w: int, ng: int, S: int) -> torch.Tensor:
    """rel (heads, (2w-1)^2) -> the dense bias (heads, S, S); differentiable with respect to ``rel``."""
    idx, has = compact_index(w, ng, S, rel.device)
    return torch.where(has[None], rel[:, idx.reshape(-1)].view(rel.shape[0], S, S), rel.new_zeros(()))
