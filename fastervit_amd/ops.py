"""Multi-scale deformable attention (Deformable DETR / DINO) on the gfx950 kernels of csrc/fvit_msda.hip -- DESIGN.md section 13.

Drop-in for the reference's ``models/dino/ops``: ``MSDeformAttnFunction`` (the autograd function, same six arguments, gradients in the same positions),
``ms_deform_attn`` (the same call without the unused step argument) and ``MSDeformAttn`` (the module: same four ``nn.Linear`` parameters under the same
names, same initialisation, same ``forward`` signature, so DINO checkpoints load).

    value                 (N, S, M, D)  fp32, fp16 or bf16; S = sum of H_l * W_l, D in {16, 32, 64, 128}
    spatial_shapes        (L, 2) int64 rows (H, W), L <= 8;     level_start_index  (L,) int64
    sampling_locations    (N, Lq, M, L, P, 2), (x, y) in [0, 1], P <= 16;     attention_weights  (N, Lq, M, L, P)
    -> (N, Lq, M * D) in value's dtype

Locations and weights go to the kernels as fp32 (16-bit ones are widened, their gradients narrowed back); a 16-bit ``value`` goes as it is and halves the
gather traffic.  There is no CPU or eager fallback: a CPU tensor raises, a missing library raises the loader's error.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib

__all__ = ["MSDeformAttnFunction", "ms_deform_attn", "MSDeformAttn"]

_CODE = {torch.float32: _lib.FVIT_F32, torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}


def _prepare(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """Checks what only the Python side can see (device, dtypes, ranks) and returns dense, aligned tensors; sizes are refused by name in the library."""
    who = "ms_deform_attn"
    for name, t in (("value", value), ("sampling_locations", sampling_locations), ("attention_weights", attention_weights)):
        if not t.is_cuda:
            raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); {name} is a {t.device.type} tensor and there is no CPU fallback")
        if t.dtype == torch.float64:
            raise RuntimeError(f"{who}: {name} is float64, which is not supported (value: float32, float16 or bfloat16; locations and weights: float32)")
    if value.dtype not in _CODE:
        raise RuntimeError(f"{who}: value dtype {value.dtype} is not supported (float32, float16 or bfloat16)")
    if value.dim() != 4 or sampling_locations.dim() != 6 or sampling_locations.shape[-1] != 2 or attention_weights.dim() != 5:
        raise RuntimeError(f"{who}: expected value (N, S, M, D), sampling_locations (N, Lq, M, L, P, 2) and attention_weights (N, Lq, M, L, P); got "
                           f"{tuple(value.shape)}, {tuple(sampling_locations.shape)}, {tuple(attention_weights.shape)}")
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_locations.shape
    if tuple(sampling_locations.shape[:3]) != (N, Lq, M) or tuple(attention_weights.shape) != (N, Lq, M, L, P):
        raise RuntimeError(f"{who}: value {tuple(value.shape)}, sampling_locations {tuple(sampling_locations.shape)} and attention_weights "
                           f"{tuple(attention_weights.shape)} do not agree on N, Lq, M, L, P")
    if tuple(spatial_shapes.shape) != (L, 2) or tuple(level_start_index.shape) != (L,):
        raise RuntimeError(f"{who}: spatial_shapes must be ({L}, 2) and level_start_index ({L},); got {tuple(spatial_shapes.shape)}, {tuple(level_start_index.shape)}")
    dev = value.device
    value = value.contiguous()
    if value.data_ptr() % 8:
        value = value.clone()
    shapes = spatial_shapes.to(device=dev, dtype=torch.int64).contiguous()
    starts = level_start_index.to(device=dev, dtype=torch.int64).contiguous()
    loc = sampling_locations.to(device=dev, dtype=torch.float32).contiguous()
    attn = attention_weights.to(device=dev, dtype=torch.float32).contiguous()
    if loc.data_ptr() % 8:
        loc = loc.clone()
    return value, shapes, starts, loc, attn, (N, S, M, D, Lq, L, P)


class MSDeformAttnFunction(Function):
    """``MSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step)``; the step argument is
    accepted and ignored (the kernels have no batch chunking)."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, im2col_step=None):
        ctx.in_dtypes = (sampling_locations.dtype, attention_weights.dtype)
        value, shapes, starts, loc, attn, dims = _prepare(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights)
        N, S, M, D, Lq, L, P = dims
        lib = _lib.lib()
        out = torch.empty(N, Lq, M * D, dtype=value.dtype, device=value.device)
        with torch.cuda.device(value.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(lib.fvit_msda_forward(_CODE[value.dtype], value.data_ptr(), shapes.data_ptr(), starts.data_ptr(), loc.data_ptr(), attn.data_ptr(),
                                             out.data_ptr(), N, S, M, D, Lq, L, P, stream), "fvit_msda_forward")
        ctx.save_for_backward(value, shapes, starts, loc, attn)
        ctx.dims = dims
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, shapes, starts, loc, attn = ctx.saved_tensors
        N, S, M, D, Lq, L, P = ctx.dims
        grad_output = grad_output.to(value.dtype).contiguous()
        grad_value = torch.empty(N, S, M, D, dtype=torch.float32, device=value.device)   # zero-filled by the call, on its stream
        grad_loc = torch.empty_like(loc)
        grad_attn = torch.empty_like(attn)
        with torch.cuda.device(value.device):
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().fvit_msda_backward(_CODE[value.dtype], value.data_ptr(), shapes.data_ptr(), starts.data_ptr(), loc.data_ptr(),
                                                     attn.data_ptr(), grad_output.data_ptr(), grad_value.data_ptr(), grad_loc.data_ptr(),
                                                     grad_attn.data_ptr(), N, S, M, D, Lq, L, P, stream), "fvit_msda_backward")
        loc_dtype, attn_dtype = ctx.in_dtypes
        return grad_value.to(value.dtype), None, None, grad_loc.to(loc_dtype), grad_attn.to(attn_dtype), None


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """out (N, Lq, M * D) = sum over levels and points of attention_weights * bilinear(value at sampling_locations); differentiable once in value,
    sampling_locations and attention_weights."""
    return MSDeformAttnFunction.apply(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, None)


class MSDeformAttn(nn.Module):
    """The multi-scale deformable attention layer of Deformable DETR / DINO around ``ms_deform_attn``.

    Every head of every query looks at ``n_points`` positions in each of ``n_levels`` feature maps: a Linear layer turns the query into offsets from its
    reference point, another into the softmax weights of those n_levels * n_points samples; the samples are read from the projected input and mixed."""

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"d_model ({d_model}) must be a multiple of n_heads ({n_heads})")
        self.im2col_step = 64   # kept for callers that read it; unused
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)
        self._reset_parameters()

    def _reset_parameters(self):
        """Offsets start independent of the query: head h looks along direction 2 pi h / n_heads, scaled onto the border of the unit square, point i at
        i + 1 steps; attention starts uniform; the two projections are Xavier-uniform with zero bias."""
        with torch.no_grad():
            angle = torch.arange(self.n_heads, dtype=torch.float32) * (2.0 * math.pi / self.n_heads)
            direction = torch.stack([angle.cos(), angle.sin()], -1)
            direction = direction / direction.abs().amax(-1, keepdim=True)
            steps = torch.arange(1, self.n_points + 1, dtype=torch.float32)
            bias = direction[:, None, None, :] * steps[None, None, :, None]
            self.sampling_offsets.weight.zero_()
            self.sampling_offsets.bias.copy_(bias.expand(self.n_heads, self.n_levels, self.n_points, 2).reshape(-1))
            self.attention_weights.weight.zero_()
            self.attention_weights.bias.zero_()
            for proj in (self.value_proj, self.output_proj):
                nn.init.xavier_uniform_(proj.weight)
                proj.bias.zero_()

    def sampling_inputs(self, query, reference_points, input_flatten, input_spatial_shapes, input_padding_mask=None):
        """(value, sampling_locations, attention_weights) as ``forward`` hands them to ``ms_deform_attn``."""
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        M, L, P = self.n_heads, self.n_levels, self.n_points
        # (device shapes are not read back: that would synchronise; the kernels ignore samples whose rows fall outside input_flatten)
        if not input_spatial_shapes.is_cuda and int((input_spatial_shapes[:, 0] * input_spatial_shapes[:, 1]).sum()) != S:
            raise ValueError("input_spatial_shapes does not add up to the length of input_flatten")
        value = self.value_proj(input_flatten)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], 0.0)
        value = value.view(N, S, M, self.d_model // M)
        offsets = self.sampling_offsets(query).view(N, Lq, M, L, P, 2)
        weights = self.attention_weights(query).view(N, Lq, M, L * P).softmax(-1).view(N, Lq, M, L, P)
        if reference_points.shape[-1] == 2:      # a point per level: offsets are in pixels of that level
            wh = input_spatial_shapes.flip(-1)   # (W, H) per level
            locations = reference_points[:, :, None, :, None, :] + offsets / wh[None, None, None, :, None, :]
        elif reference_points.shape[-1] == 4:    # a box (cx, cy, w, h) per level: offsets are in units of half the box over n_points
            locations = reference_points[:, :, None, :, None, :2] + offsets / P * reference_points[:, :, None, :, None, 2:] * 0.5
        else:
            raise ValueError(f"reference_points must end in 2 or 4 values, not {reference_points.shape[-1]}")
        return value, locations, weights

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index, input_padding_mask=None):
        """query (N, Lq, C); reference_points (N, Lq, n_levels, 2 or 4) in [0, 1]; input_flatten (N, S, C); input_spatial_shapes (n_levels, 2) = (H, W);
        input_level_start_index (n_levels,); input_padding_mask (N, S), True = padding.  Returns (N, Lq, C).  Under autocast the 16-bit value goes to the
        kernel as it is and the locations and weights as fp32."""
        value, locations, weights = self.sampling_inputs(query, reference_points, input_flatten, input_spatial_shapes, input_padding_mask)
        core = ms_deform_attn(value, input_spatial_shapes, input_level_start_index, locations.float(), weights.float())
        return self.output_proj(core)
