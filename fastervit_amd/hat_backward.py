"""Backward (and train-mode forward) of the HAT stages on the MI355X kernels.

    y = x + gamma * fc2(GELU(fc1(LayerNorm(x))))            Mlp.forward FV:398-407 inside HAT.forward FV:691 / AR:697        mlp_block_backward
    y = x + gamma * proj(attention(qkv(LayerNorm(x))))      WindowAttention.forward FV:557-568 inside HAT.forward FV:690      attn_block_backward
    a whole HAT block, without (stage 3) and WITH carrier tokens (stage 2: FV:662-701 / AR:668-707, incl. the last block's
    carrier propagation FV:697-700)                                                                       local_block_backward / hier_block_backward
    a whole stage (zero padding, TokenInitializer, partition, depth x block, reverse, crop: FV:832-841 / AR:848-869)   local_stage_backward / hier_stage_backward
    the stage as ONE autograd node, eval or TRAIN mode (stochastic depth, FV:630, 652, 690-691)                      HatStageFunction / stage_forward_with_grad

The reference differentiates this with autograd (train.py:820-951, the model wrapped in DDP at train.py:542-551).  Here the backward of ONE
sub-block is a fixed kernel sequence behind the C ABI, checked against torch.autograd (tests/test_gpu_backward.py):

    recompute   xn = LN(x)               fvit_gather_layernorm        a = xn W1^T + b1         fvit_gemm_bias_act
                h  = GELU(a)             fvit_bwd_gelu                z = h W2^T + b2          fvit_gemm_bias_act
    gamma / b2  dz = gamma * dy, column sums of dy * z and dz         fvit_bwd_scale_cols + fvit_bwd_colsum_finish
    fc2         dh  = dz W2              fvit_gemm_bias_act (weight operand = W2^T)
                dW2 += dz^T h            fvit_bwd_transpose16 x 2 + fvit_gemm_residual (fp32 accumulation INTO the gradient buffer)
    GELU / b1   da = dh * GELU'(a), column sums of da                 fvit_bwd_gelu + fvit_bwd_colsum_finish
    fc1         dW1 += da^T xn           fvit_bwd_transpose16 x 2 + fvit_gemm_residual
                dxn = da W1              fvit_gemm_residual into a zeroed fp32 buffer (weight operand = W1^T)
    LayerNorm   dx = dy + LN'(dxn), d ln_w, d ln_b                    fvit_bwd_layernorm + fvit_bwd_colsum_finish

Operands of the GEMMs are 16-bit (fp16 / bf16) with fp32 accumulation, like the forward path; activations are recomputed, nothing is saved by
the forward.  Parameter gradients ACCUMULATE into the buffers of ``MlpGrads`` / ``AttnGrads`` (zero them for a fresh step); no atomics anywhere
(column sums are per-64-row partials added in block order), so gradients are bit-reproducible.  Geometry: head_dim <= 96 (the attention kernels
run on the head_dim padded to 32 / 64 / 96 with zero channels, like the forward path), any C that is a multiple of 16 (a K dimension is zero-padded
to a multiple of 64), windows / carrier grids of at most 64 tokens -- every reference entrypoint at 224 x 224.  What this is NOT: backward KERNELS
for the conv side (PyTorch autograd differentiates those modules) or the optimizer / data loop of train.py; there is no CPU path.

Longer sequences (``FasterViT.enable_hat_backward(True, long_sequences=True)``: the 576 / 1024 / 2304-token windows of faster_vit_4_21k_384 / _512 / _768,
any-res carrier grids above 64 tokens): the sub-block functions take any S.  For S > 64 the attention core is recomputed by the kernel the inference path
uses for that length -- fvit_window_attention with the dense (heads, S, S) table where ``fvit_attention_dense(S, dpad)``, otherwise
fvit_window_attention_long with the COMPACT table (heads, (2w-1)^2) (``CompactBias``) -- and differentiated by fvit_bwd_window_attention_long
(csrc/fvit_attnbwd.hip: tiled, MFMA, no atomics) with the same bias form; ``AttnGrads.bias`` then holds the gradient of that form, and in the compact form
the host differentiates the compact table (16 * sigmoid(cpb_mlp(relative_coords_table)), FV:276-280), so no (heads, S, S) tensor exists for S > 208.
S <= 64 stays on fvit_bwd_window_attention: no gradient computed before changes by a bit.  Not covered above 64 tokens: the attn_drop mask.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from .hat_runtime import FVIT_BF16, FVIT_F16

_CODE = {torch.float16: FVIT_F16, torch.bfloat16: FVIT_BF16}


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass
class MlpGrads:
    """fp32 gradient buffers of one MLP sub-block; ``mlp_block_backward`` adds into them."""
    fc1_w: torch.Tensor
    fc1_b: torch.Tensor
    fc2_w: torch.Tensor
    fc2_b: torch.Tensor
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    gamma: Optional[torch.Tensor]

    @staticmethod
    def zeros(C_: int, hidden: int, device, with_gamma: bool = True) -> "MlpGrads":
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)   # noqa: E731
        return MlpGrads(z(hidden, C_), z(hidden), z(C_, hidden), z(C_), z(C_), z(C_), z(C_) if with_gamma else None)


def _pad_rows(w: torch.Tensor, dt, cols: Optional[int] = None) -> torch.Tensor:
    """16-bit GEMM weight operand: rows zero-padded to a multiple of 128 (fvit_gemm_bias_act's Wt contract), columns (the K dimension) to ``cols``."""
    cols = w.shape[1] if cols is None else cols
    out = torch.zeros(_rup(w.shape[0], 128), cols, dtype=dt, device=w.device)
    out[:w.shape[0], :w.shape[1]] = w.to(dt)
    return out


def _dpad(d: int) -> int:
    """Padded head_dim of the attention kernels (hat_runtime._prepare): 32 / 64 / 96."""
    if d > 96:
        raise RuntimeError(f"head_dim {d} > 96 has no attention kernel instance")
    return 32 if d <= 32 else (64 if d <= 64 else 96)


def _pack_qkv(wq: torch.Tensor, bq: torch.Tensor, heads: int, d: int, dp: int):
    """qkv.weight (3C, C) / bias (3C) -> rows [q|k|v][head][dpad] (zero rows / entries on the padded head channels)."""
    if d == dp:
        return wq, bq
    C_ = wq.shape[1]
    w = wq.new_zeros(3, heads, dp, C_)
    w[:, :, :d] = wq.view(3, heads, d, C_)
    b = bq.new_zeros(3, heads, dp)
    b[:, :, :d] = bq.view(3, heads, d)
    return w.view(3 * heads * dp, C_), b.view(-1)


def _unpack_qkv(g: torch.Tensor, heads: int, d: int, dp: int) -> torch.Tensor:
    """Inverse of ``_pack_qkv`` on dim 0 (gradient rows / bias entries of the real head channels)."""
    if d == dp:
        return g
    return g.view(3, heads, dp, *g.shape[1:])[:, :, :d].reshape(3 * heads * d, *g.shape[1:])


def _pack_proj(wp: torch.Tensor, heads: int, d: int, dp: int, K: int) -> torch.Tensor:
    """proj.weight (C, C) -> (C, K) with columns [head][dpad] (+ zero columns up to K, a multiple of 64)."""
    C_ = wp.shape[0]
    if d == dp and K == C_:
        return wp
    w = wp.new_zeros(C_, K)
    w[:, :heads * dp].view(C_, heads, dp)[:, :, :d] = wp.view(C_, heads, d)
    return w


def _unpack_proj(g: torch.Tensor, heads: int, d: int, dp: int) -> torch.Tensor:
    C_ = g.shape[0]
    if d == dp and g.shape[1] == C_:
        return g
    return g[:, :heads * dp].reshape(C_, heads, dp)[:, :, :d].reshape(C_, heads * d)


class _RS:
    """What scales a sub-block's residual update in TRAIN mode: ``rows`` fp32 [M] = DropPath (one factor per window / image, repeated per row), ``out`` fp32
    [M][C] = the Dropout mask of the sub-block's OUTPUT (0 or 1 / keep: ``Mlp.drop`` after fc2, FV:406; ``WindowAttention.proj_drop``, FV:567), ``hid``
    operand-dtype [M][hidden] = the Dropout mask of GELU(fc1) (``Mlp.drop`` after the activation, FV:404).  y = x + rows * out * gamma * f(x): the output mask is
    an elementwise form of the DropPath factor, so forward and backward treat the two alike; ``hid`` multiplies the hidden activation (and dh in the backward);
    ``attn`` operand-dtype [windows * heads][S][Spad] = the Dropout mask of the softmax probabilities (``WindowAttention.attn_drop``, FV:564), applied inside the
    attention kernels (fvit_window_attention_drop / fvit_bwd_window_attention_drop)."""
    __slots__ = ("rows", "out", "hid", "attn")

    def __init__(self, rows=None, out=None, hid=None, attn=None):
        self.rows, self.out, self.hid, self.attn = rows, out, hid, attn


def _rs(mk: Optional[dict], key: str, group: int) -> _RS:
    """Sub-block ``key`` of one block's ``drop_path_masks`` entry: per-group DropPath factors (one per window / per image) -> one per row, plus its Dropout masks."""
    mk = mk or {}
    scale = mk.get(key)
    return _RS(None if scale is None else scale.repeat_interleave(group), mk.get(key + "_out"), mk.get(key + "_hid"), mk.get(key + "_p"))


def _out_scale(rs: _RS, M: int) -> Optional[torch.Tensor]:
    """fp32 factor of the sub-block's output, broadcastable to [M][C] (None: 1)."""
    sc = None if rs.rows is None else rs.rows.float().view(M, 1)
    if rs.out is not None:
        sc = rs.out.float() if sc is None else sc * rs.out.float()
    return sc


def _lerp_rows(x: torch.Tensor, y0: torch.Tensor, rs: _RS) -> torch.Tensor:
    """Stochastic depth on top of the residual epilogue: y0 = x + f  ->  x + row_scale[m] * f."""
    sc = _out_scale(rs, x.shape[0])
    if sc is None:
        return y0
    return torch.addcmul(x, y0 - x, sc.to(x.dtype).expand_as(x))


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _require_hip(who: str, x: torch.Tensor) -> None:
    if not x.is_cuda:
        raise RuntimeError(f"{who} runs only on a HIP device (libfvit_hip.so kernels); there is no CPU fallback")


def _check_rows(who: str, rows: str, x: torch.Tensor, dy: torch.Tensor) -> None:
    for t, name in ((x, "x"), (dy, "dy")):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(x.shape) or t.device != x.device:
            raise RuntimeError(f"{who}: {name} must be a contiguous fp32 [{rows}][C] tensor on {x.device}")


class _Sub:
    """One sub-block call y = x + gamma * (act W2^T + b2), act = middle(LayerNorm(x) W1^T + b1) -- the steps below are what the MLP and the attention
    sub-block share: library, operand type, stream, the rows ``x`` with their padded sizes (Ck: C as a GEMM K dimension, zero columns beyond C: FasterViT-4's
    784 / 1568), the fp32 LayerNorm / gamma parameters, the row scale and, with ``part_cols`` (the widest column sum of a backward), the per-64-row partial
    sums ``part``.  Every step of a backward finishes its sums from ``part`` before the next step overwrites it: the order of the steps is fixed."""

    def __init__(self, x, ln_w, ln_b, gamma, eps, operand_dtype, row_scale, part_cols: int = 0):
        self.lib, self.code, self.dt, self.dev, self.x, self.eps = _lib.lib(), _CODE[operand_dtype], operand_dtype, x.device, x, eps
        self.M, self.C_ = M, C_ = x.shape
        self.Mp, self.Mk, self.Ck = _rup(M, 128), _rup(M, 64), _rup(C_, 64)
        self.ln_w, self.ln_b, self.g = _f32(ln_w, x.device), _f32(ln_b, x.device), _f32(gamma, x.device) if gamma is not None else None
        self.rs = row_scale if isinstance(row_scale, _RS) else _RS(rows=row_scale)   # None, fp32 [M] DropPath factors or an _RS: one internal form
        self.blocks = self.lib.fvit_bwd_blocks(M)
        self.part = torch.empty(self.blocks * 2 * part_cols, dtype=torch.float32, device=x.device) if part_cols else None
        self.st = torch.cuda.current_stream(x.device).cuda_stream

    def z16(self, r: int, c: int) -> torch.Tensor:
        return torch.zeros(r, c, dtype=self.dt, device=self.dev)


def _recompute(k: _Sub, w: torch.Tensor, b: torch.Tensor, n: int, ldn: int, act: int, name: str):
    """xn = LayerNorm(x) and the first Linear, out[:, :n] = xn w^T + b (``act`` 1: with GELU), as 16-bit rows of stride Ck / ``ldn``."""
    xn, out = k.z16(k.Mp, k.Ck), k.z16(k.Mp, ldn)
    W = _pad_rows(w, k.dt, k.Ck)
    _lib.check(k.lib.fvit_gather_layernorm(k.code, k.x.data_ptr(), k.M, None, 0, None, None, None, None, xn.data_ptr(), k.Ck, k.ln_w.data_ptr(), k.ln_b.data_ptr(),
                                           C.c_float(k.eps), k.M, k.M, k.C_, k.st), "layernorm")
    _lib.check(k.lib.fvit_gemm_bias_act(k.code, xn.data_ptr(), k.Ck, W.data_ptr(), k.Ck, b.data_ptr(), out.data_ptr(), ldn, k.M, n, k.Ck, act, k.st), name)
    return xn, out


def _residual_out(k: _Sub, act: torch.Tensor, lda: int, w: torch.Tensor, b: torch.Tensor, name: str) -> torch.Tensor:
    """The forward's second Linear with the residual epilogue, then stochastic depth: y = x + row_scale * gamma * (act w^T + b)."""
    W = _pad_rows(w, k.dt)
    y = k.x.clone()
    _lib.check(k.lib.fvit_gemm_residual(k.code, act.data_ptr(), lda, W.data_ptr(), lda, b.data_ptr(), _p(k.g), y.data_ptr(), k.C_, k.M, k.C_, lda, k.st), name)
    return _lerp_rows(k.x, y, k.rs)


def _linear_backward(k: _Sub, dout: torch.Tensor, ldo: int, n: int, act: torch.Tensor, lda: int, ka: int, w: torch.Tensor, gw: torch.Tensor, names,
                     narrow: bool) -> torch.Tensor:
    """Backward of out[:, :n] = act[:, :ka] w^T from the 16-bit ``dout`` (row stride ``ldo``): gw (n, ka) += dout^T act (two transposes and a GEMM that
    accumulates in fp32 INTO ``gw``) and the input gradient dout w (weight operand = w^T) -- ``narrow``: 16-bit rows of stride ``lda`` written BEFORE the
    weight gradient (the second Linear), else fp32 [M][C] accumulated into zeros AFTER it (the first Linear).  ``names`` = (input gradient, dout^T, act^T, gw)."""
    lib, code, M, Mk, st, ck = k.lib, k.code, k.M, k.Mk, k.st, _lib.check
    WT = _pad_rows(w.t().contiguous(), k.dt, ldo)
    doutT, actT = k.z16(_rup(n, 128), Mk), k.z16(_rup(ka, 128), Mk)
    if narrow:
        dact = k.z16(k.Mp, lda)
        ck(lib.fvit_gemm_bias_act(code, dout.data_ptr(), ldo, WT.data_ptr(), ldo, None, dact.data_ptr(), lda, M, ka, ldo, 0, st), names[0])
    ck(lib.fvit_bwd_transpose16(code, dout.data_ptr(), ldo, doutT.data_ptr(), Mk, M, n, st), names[1])
    ck(lib.fvit_bwd_transpose16(code, act.data_ptr(), lda, actT.data_ptr(), Mk, M, ka, st), names[2])
    ck(lib.fvit_gemm_residual(code, doutT.data_ptr(), Mk, actT.data_ptr(), Mk, None, None, gw.data_ptr(), ka, n, ka, Mk, st), names[3])
    if not narrow:
        dact = torch.zeros(M, ka, dtype=torch.float32, device=k.dev)
        ck(lib.fvit_gemm_residual(code, dout.data_ptr(), ldo, WT.data_ptr(), ldo, None, None, dact.data_ptr(), ka, M, ka, ldo, st), names[0])
    return dact


def _output_backward(k: _Sub, dy: torch.Tensor, act: torch.Tensor, lda: int, w: torch.Tensor, b: torch.Tensor, g_gamma, g_b: torch.Tensor, g_w: torch.Tensor,
                     names) -> torch.Tensor:
    """From dy back through y = x + row_scale * gamma * z, z = act w^T + b: recompute z, dz = gamma * (what the sub-block sees of dy), the gamma and bias
    gradients (column sums of dy * z and dz), then the Linear.  Returns d act (16-bit).  ``names`` = (z, bias gradient, d act, act^T, weight gradient)."""
    lib, code, M, C_, st, ck = k.lib, k.code, k.M, k.C_, k.st, _lib.check
    W = _pad_rows(w, k.dt)
    z, dz = k.z16(k.Mp, C_), k.z16(k.Mp, k.Ck)
    osc = _out_scale(k.rs, M)
    dyi = dy if osc is None else (dy * osc).contiguous()   # the sub-block sees dy * row_scale, the skip connection sees dy
    ck(lib.fvit_gemm_bias_act(code, act.data_ptr(), lda, W.data_ptr(), lda, b.data_ptr(), z.data_ptr(), C_, M, C_, lda, 0, st), names[0])
    ck(lib.fvit_bwd_scale_cols(code, dyi.data_ptr(), z.data_ptr(), C_, _p(k.g), dz.data_ptr(), k.Ck, k.part.data_ptr(), M, C_, st), "scale_cols")
    if g_gamma is not None:
        ck(lib.fvit_bwd_colsum_finish(k.part.data_ptr(), k.blocks, 2 * C_, g_gamma.data_ptr(), C_, 1, st), "dgamma")
    ck(lib.fvit_bwd_colsum_finish(k.part.data_ptr() + 4 * C_, k.blocks, 2 * C_, g_b.data_ptr(), C_, 1, st), names[1])
    return _linear_backward(k, dz, k.Ck, C_, act, lda, lda, w, g_w, (names[2], "dz^T", names[3], names[4]), narrow=True)


def _layernorm_backward(k: _Sub, dxn: torch.Tensor, dy: torch.Tensor, grads) -> torch.Tensor:
    """dx = dy + LN'(dxn); column sums into grads.ln_w / grads.ln_b."""
    lib, M, C_, st, ck = k.lib, k.M, k.C_, k.st, _lib.check
    dx = torch.empty(M, C_, dtype=torch.float32, device=k.dev)
    stats = torch.empty(M, 2, dtype=torch.float32, device=k.dev)
    ck(lib.fvit_bwd_layernorm(k.x.data_ptr(), dxn.data_ptr(), dy.data_ptr(), k.ln_w.data_ptr(), C.c_float(k.eps), dx.data_ptr(), stats.data_ptr(),
                              k.part.data_ptr(), M, C_, st), "layernorm_bwd")
    ck(lib.fvit_bwd_colsum_finish(k.part.data_ptr(), k.blocks, 2 * C_, grads.ln_w.data_ptr(), C_, 1, st), "dln_w")
    ck(lib.fvit_bwd_colsum_finish(k.part.data_ptr() + 4 * C_, k.blocks, 2 * C_, grads.ln_b.data_ptr(), C_, 1, st), "dln_b")
    return dx


def mlp_block_backward(x: torch.Tensor, dy: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, fc1_w: torch.Tensor, fc1_b: torch.Tensor,
                       fc2_w: torch.Tensor, fc2_b: torch.Tensor, gamma: Optional[torch.Tensor], grads: MlpGrads, eps: float = 1e-5,
                       operand_dtype=torch.float16, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Returns dx (fp32 [M][C]) and adds the parameter gradients of the sub-block into ``grads``.  x, dy: fp32 [M][C] on a HIP device.
    ``row_scale`` (fp32 [M], optional): stochastic depth -- y = x + row_scale[m] * gamma * (...) (timm DropPath: 0 or 1 / keep_prob per sample,
    FV:691 ``self.drop_path(self.gamma4 * self.mlp(...))``): the sub-block sees dy * row_scale, the skip connection sees dy."""
    who = "mlp_block_backward"
    _require_hip(who, x)
    if operand_dtype not in _CODE:
        raise ValueError("operand_dtype must be torch.float16 or torch.bfloat16")
    M, C_ = x.shape
    hid = fc1_w.shape[0]
    if C_ % 16 or hid % 64:
        raise RuntimeError(f"{who}: C = {C_} must be a multiple of 16 and hidden = {hid} a multiple of 64")
    _check_rows(who, "M", x, dy)
    k = _Sub(x, ln_w, ln_b, gamma, eps, operand_dtype, row_scale, max(C_, hid))
    with torch.cuda.device(k.dev):
        lib, code, st, ck = k.lib, k.code, k.st, _lib.check
        w1, w2, b1, b2 = (_f32(t, k.dev) for t in (fc1_w, fc2_w, fc1_b, fc2_b))
        xn, a = _recompute(k, w1, b1, hid, hid, 0, "fc1")
        h, da = k.z16(k.Mp, hid), k.z16(k.Mp, hid)
        ck(lib.fvit_bwd_gelu(code, a.data_ptr(), hid, None, 0, h.data_ptr(), hid, None, M, hid, st), "gelu")
        if k.rs.hid is not None:
            h[:M] *= k.rs.hid        # Dropout on GELU(fc1) (FV:404): the same mask as in the forward
        dh = _output_backward(k, dy, h, hid, w2, b2, grads.gamma, grads.fc2_b, grads.fc2_w, ("fc2", "db2", "dh", "h^T", "dW2"))
        if k.rs.hid is not None:
            dh[:M] *= k.rs.hid       # adjoint of the hidden Dropout
        ck(lib.fvit_bwd_gelu(code, a.data_ptr(), hid, dh.data_ptr(), hid, da.data_ptr(), hid, k.part.data_ptr(), M, hid, st), "gelu_bwd")
        ck(lib.fvit_bwd_colsum_finish(k.part.data_ptr(), k.blocks, hid, grads.fc1_b.data_ptr(), hid, 1, st), "db1")
        dxn = _linear_backward(k, da, hid, hid, xn, k.Ck, C_, w1, grads.fc1_w, ("dxn", "da^T", "xn^T", "dW1"), narrow=False)
        return _layernorm_backward(k, dxn, dy, grads)


def mlp_block_forward(x: torch.Tensor, ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, gamma, eps: float = 1e-5, operand_dtype=torch.float16,
                      row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x + row_scale * gamma * fc2(GELU(fc1(LayerNorm(x)))) through the unit kernels of the forward path (activation recompute for the block-level
    backwards; train-mode forward with DropPath = ``row_scale``)."""
    _require_hip("mlp_block_forward", x)
    hid = fc1_w.shape[0]
    k = _Sub(x, ln_w, ln_b, gamma, eps, operand_dtype, row_scale)
    with torch.cuda.device(k.dev):
        _, h = _recompute(k, _f32(fc1_w, k.dev), _f32(fc1_b, k.dev), hid, hid, 1, "fc1 + GELU")
        if k.rs.hid is not None:
            h[:k.M] *= k.rs.hid      # Dropout on GELU(fc1) (FV:404)
        return _residual_out(k, h, hid, _f32(fc2_w, k.dev), _f32(fc2_b, k.dev), "fc2")


@dataclass
class AttnGrads:
    """fp32 gradient buffers of one attention sub-block; ``attn_block_backward`` adds into them.  ``bias`` is the gradient of the folded
    relative-position bias table (heads, S, S) -- the table is a constant of the inference path (PosEmbMLPSwinv2D folded at load, FV:213-310);
    its own small MLP is differentiated from this on the host."""
    qkv_w: torch.Tensor
    qkv_b: torch.Tensor
    proj_w: torch.Tensor
    proj_b: torch.Tensor
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    gamma: Optional[torch.Tensor]
    bias: Optional[torch.Tensor]

    @staticmethod
    def zeros(C_: int, heads: int, S: int, device, with_gamma: bool = True, with_bias: bool = True, bias_shape=None) -> "AttnGrads":
        """``bias_shape``: shape of the bias gradient when it is not the dense (heads, S, S) one -- (heads, (2w-1)^2) for a ``CompactBias``."""
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=device)   # noqa: E731
        bshape = tuple(bias_shape) if bias_shape is not None else (heads, S, S)
        return AttnGrads(z(3 * C_, C_), z(3 * C_), z(C_, C_), z(C_), z(C_), z(C_), z(C_) if with_gamma else None, z(*bshape) if with_bias else None)


@dataclass
class CompactBias:
    """The relative-position bias of an attention in the form the long-window kernels index arithmetically: ``table`` fp32 (heads, (2w-1)^2) =
    16 * sigmoid(cpb_mlp(relative_coords_table)) before the relative_position_index gather (``PosEmbMLPSwinv2D.rel_table``), ``w`` the side of the bias
    window and ``ng`` the number of leading tokens without bias (ng + w^2 == S).  Accepted as ``bias`` by the attention sub-block functions where
    ``fvit_attention_dense(S, dpad)`` is false; ``AttnGrads.bias`` is then the gradient of ``table``."""
    table: torch.Tensor
    w: int
    ng: int


MAX_SHORT_SEQ = 64   # fvit_bwd_window_attention (one workgroup holds a whole (window, head) in LDS); longer: fvit_bwd_window_attention_long


class _Core:
    """Operands of the attention core of one sub-block call: which forward kernel recomputes it, its bias form, and the matching backward."""

    def __init__(self, lib, who: str, bias, heads: int, S: int, dp: int, dev, pmask):
        self.long = S > MAX_SHORT_SEQ
        self.dense = bool(lib.fvit_attention_dense(S, dp)) if self.long else True
        self.rel, self.w, self.ng, self.btab, self.spad = None, 0, 0, None, 0
        if self.long and pmask is not None:
            raise RuntimeError(f"{who}: an attn_drop mask on a sequence of {S} tokens (the attention-core backward above {MAX_SHORT_SEQ} tokens has no Dropout mask)")
        if isinstance(bias, CompactBias):
            if self.dense:
                raise RuntimeError(f"{who}: S = {S} at padded head_dim {dp} runs on the dense-table attention kernel; pass the (heads, S, S) bias")
            if bias.ng < 0 or bias.ng + bias.w * bias.w != S or tuple(bias.table.shape) != (heads, (2 * bias.w - 1) ** 2):
                raise RuntimeError(f"{who}: compact bias table {tuple(bias.table.shape)} with w = {bias.w}, ng = {bias.ng} does not cover S = {S} tokens of {heads} heads")
            self.rel = _f32(bias.table, dev)
            self.w, self.ng = int(bias.w), int(bias.ng)
            return
        if not self.dense:
            if bias is not None:
                raise RuntimeError(f"{who}: S = {S} at padded head_dim {dp} runs on the long-window attention kernel, which takes the compact bias table "
                                   "(hat_backward.CompactBias), not a dense (heads, S, S) one")
            return
        self.spad = lib.fvit_attention_spad(S)
        self.btab = torch.zeros(heads, self.spad, self.spad, dtype=torch.float32, device=dev)   # fvit_window_attention always takes a table (mask on padded keys)
        if bias is not None:
            self.btab[:, :S, :S] = bias.detach().to(device=dev, dtype=torch.float32)
        self.btab[:, :, S:] = _lib.FVIT_MASK_BIAS

    def forward(self, lib, code, qkv, Kq, o, Kao, nwin, S, heads, dp, scale, pmask, st):
        if self.dense:
            _lib.check(lib.fvit_window_attention_drop(code, qkv.data_ptr(), Kq, o.data_ptr(), Kao, self.btab.data_ptr(), nwin, S, heads, dp, C.c_float(scale),
                                                      _p(pmask), st), "attention")
        else:
            _lib.check(lib.fvit_window_attention_long(code, qkv.data_ptr(), Kq, o.data_ptr(), Kao, _p(self.rel), self.w, self.ng, nwin, S, heads, dp,
                                                      C.c_float(scale), st), "attention (long)")

    def backward(self, lib, code, qkv, Kq, do, Kao, dqkv, dbias, nwin, S, heads, dp, scale, pmask, st):
        """dqkv from dO; the bias gradient is ADDED into ``dbias`` (dense (heads, S, S) or the compact table's shape), summed over the windows in window order."""
        if not self.long:
            part = torch.empty(nwin * heads * S * S, dtype=torch.float32, device=qkv.device) if dbias is not None else None
            _lib.check(lib.fvit_bwd_window_attention_drop(code, qkv.data_ptr(), Kq, do.data_ptr(), Kao, _p(self.btab), self.spad, C.c_float(scale), dqkv.data_ptr(),
                                                          _p(part), nwin, S, heads, dp, _p(pmask), st), "attention_bwd")
            if dbias is not None:
                _lib.check(lib.fvit_bwd_colsum_finish(part.data_ptr(), nwin, heads * S * S, dbias.data_ptr(), heads * S * S, 1, st), "dbias")
            return
        nbytes = lib.fvit_bwd_window_attention_long_workspace(nwin, S, heads, dp, self.w if (self.rel is not None and dbias is not None) else 0)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=qkv.device)
        _lib.check(lib.fvit_bwd_window_attention_long(code, qkv.data_ptr(), Kq, do.data_ptr(), Kao, _p(self.btab), self.spad, _p(self.rel), self.w, self.ng,
                                                      C.c_float(scale), dqkv.data_ptr(), _p(dbias), ws.data_ptr(), nbytes, nwin, S, heads, dp, st), "attention_bwd (long)")


def _attn_geometry(C_: int, heads: int):
    d = C_ // heads
    dp = _dpad(d)
    HD = heads * dp
    return d, dp, HD, 3 * HD, _rup(3 * HD, 64), _rup(HD, 64), _rup(C_, 64)


def _attn_recompute(k: _Sub, who: str, geo, qkv_w, qkv_b, proj_w, bias, heads: int, S: int, qk_scale):
    """What both attention functions start from: qkv / proj weights in the padded head layout ([C3p][C], [C][Kao]), the core for this S and bias form, and
    xn = LayerNorm(x), qkv = xn Wqkv^T + b, o = attention(qkv).  ``run``: the arguments ``_Core.forward`` and ``_Core.backward`` share."""
    d, dp, _, C3p, Kq, Kao, _ = geo
    wq, bq = _pack_qkv(_f32(qkv_w, k.dev), _f32(qkv_b, k.dev) if qkv_b is not None else torch.zeros(3 * k.C_, device=k.dev), heads, d, dp)
    wp = _pack_proj(_f32(proj_w, k.dev), heads, d, dp, Kao)
    core = _Core(k.lib, who, bias, heads, S, dp, k.dev, k.rs.attn)
    xn, qkv = _recompute(k, wq, bq.contiguous(), C3p, Kq, 0, "qkv")
    o = k.z16(k.Mp, Kao)
    run = (k.M // S, S, heads, dp, float(qk_scale) if qk_scale else d ** -0.5, k.rs.attn, k.st)
    core.forward(k.lib, k.code, qkv, Kq, o, Kao, *run)
    return wq, wp, core, xn, qkv, o, run


def attn_block_backward(x: torch.Tensor, dy: torch.Tensor, ln_w: torch.Tensor, ln_b: torch.Tensor, qkv_w: torch.Tensor, qkv_b: Optional[torch.Tensor],
                        proj_w: torch.Tensor, proj_b: torch.Tensor, gamma: Optional[torch.Tensor], bias: Optional[torch.Tensor], heads: int, S: int,
                        grads: AttnGrads, eps: float = 1e-5, qk_scale: Optional[float] = None, operand_dtype=torch.float16,
                        row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Backward of y = x + gamma * proj(softmax(q k^T * scale + bias) v), [q|k|v] = qkv(LayerNorm(x)), per window of S consecutive rows.
    x, dy: fp32 [nwin * S][C]; bias: fp32 (heads, S, S), a ``CompactBias`` (S > 64 beyond the dense-table attention kernel) or None; head_dim = C / heads <= 96
    (the kernels run on the head_dim padded to 32 / 64 / 96, as the forward path does; C a multiple of 16), any S >= 1.  Returns dx; parameter gradients are
    added into ``grads`` (``grads.bias``: the gradient of the bias in the form it was given).  ``row_scale``: see ``mlp_block_backward`` (FV:690
    ``self.drop_path(self.gamma3 * self.attn(...))``).  Kernel sequence as in ``mlp_block_backward`` with fvit_window_attention (recompute) /
    fvit_bwd_window_attention in the middle for S <= 64, and for longer sequences fvit_window_attention or fvit_window_attention_long (whichever the
    inference path runs at that length) / fvit_bwd_window_attention_long; the attn_drop mask of ``row_scale`` is refused above 64 tokens."""
    who = "attn_block_backward"
    _require_hip(who, x)
    if operand_dtype not in _CODE:
        raise ValueError("operand_dtype must be torch.float16 or torch.bfloat16")
    M, C_ = x.shape
    if C_ % 16 or C_ % heads or C_ // heads > 96 or S < 1 or M % S:
        raise RuntimeError(f"{who}: C = {C_}, heads = {heads}, S = {S}, rows = {M}: need head_dim <= 96, C % 16 == 0, S >= 1, rows % S == 0")
    _check_rows(who, "rows", x, dy)
    geo = _attn_geometry(C_, heads)
    d, dp, _, C3p, Kq, Kao, _ = geo
    padded = d != dp or Kao != C_
    k = _Sub(x, ln_w, ln_b, gamma, eps, operand_dtype, row_scale, max(C3p, C_))
    with torch.cuda.device(k.dev):
        lib, code, st, ck = k.lib, k.code, k.st, _lib.check
        wq, wp, core, xn, qkv, o, run = _attn_recompute(k, who, geo, qkv_w, qkv_b, proj_w, bias, heads, S, qk_scale)
        # gradient buffers in the padded layout (the accumulating GEMMs write straight into ``grads`` when no padding is involved)
        gq_w = torch.zeros(C3p, C_, dtype=torch.float32, device=k.dev) if padded else grads.qkv_w
        gq_b = torch.zeros(C3p, dtype=torch.float32, device=k.dev) if padded else grads.qkv_b
        gp_w = torch.zeros(C_, Kao, dtype=torch.float32, device=k.dev) if padded else grads.proj_w
        do = _output_backward(k, dy, o, Kao, wp, _f32(proj_b, k.dev), grads.gamma, grads.proj_b, gp_w, ("proj", "dbproj", "dO", "O^T", "dWproj"))
        dqkv = k.z16(k.Mp, Kq)
        core.backward(lib, code, qkv, Kq, do, Kao, dqkv, grads.bias, *run)
        ck(lib.fvit_bwd_colsum16(code, dqkv.data_ptr(), Kq, k.part.data_ptr(), M, C3p, st), "colsum dqkv")
        ck(lib.fvit_bwd_colsum_finish(k.part.data_ptr(), k.blocks, C3p, gq_b.data_ptr(), C3p, 1, st), "dbqkv")
        dxn = _linear_backward(k, dqkv, Kq, C3p, xn, k.Ck, C_, wq, gq_w, ("dxn", "dqkv^T", "xn^T", "dWqkv"), narrow=False)
        dx = _layernorm_backward(k, dxn, dy, grads)
    if padded:   # the real rows / columns of the padded-layout gradients
        grads.qkv_w += _unpack_qkv(gq_w, heads, d, dp)
        grads.qkv_b += _unpack_qkv(gq_b, heads, d, dp)
        grads.proj_w += _unpack_proj(gp_w, heads, d, dp)
    return dx


def attn_block_forward(x: torch.Tensor, ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, gamma, bias, heads: int, S: int, eps: float = 1e-5,
                       qk_scale: Optional[float] = None, operand_dtype=torch.float16, row_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = x + row_scale * gamma * proj(attention(qkv(LayerNorm(x)))) through the unit kernels of the forward path (LayerNorm, GEMM, attention core, GEMM
    with the residual epilogue): the activation recompute a block-level backward starts from, and the train-mode forward (DropPath = ``row_scale``)."""
    who = "attn_block_forward"
    _require_hip(who, x)
    geo = _attn_geometry(x.shape[1], heads)
    k = _Sub(x, ln_w, ln_b, gamma, eps, operand_dtype, row_scale)
    with torch.cuda.device(k.dev):
        _, wp, _, _, _, o, _ = _attn_recompute(k, who, geo, qkv_w, qkv_b, proj_w, bias, heads, S, qk_scale)
        return _residual_out(k, o, geo[5], wp, _f32(proj_b, k.dev), "proj")


def _attn_args(a: dict):
    """A sub-block's parameter dict as the leading tensor arguments of ``attn_block_forward`` / ``attn_block_backward`` (after x / x, dy)."""
    return a["ln_w"], a["ln_b"], a["qkv_w"], a.get("qkv_b"), a["proj_w"], a["proj_b"], a.get("gamma"), a.get("bias")


def _mlp_args(m: dict):
    return m["ln_w"], m["ln_b"], m["fc1_w"], m["fc1_b"], m["fc2_w"], m["fc2_b"], m.get("gamma")


def local_block_backward(x: torch.Tensor, dy: torch.Tensor, attn: dict, mlp: dict, heads: int, S: int, attn_grads: AttnGrads, mlp_grads: MlpGrads,
                         eps: float = 1e-5, operand_dtype=torch.float16, masks: Optional[dict] = None) -> torch.Tensor:
    """Backward of one HAT block WITHOUT carrier tokens (the stage-3 form, FV:690-691 with ct = None):
         x1 = x + gamma3 * attn(norm1(x));  y = x1 + gamma4 * mlp(norm2(x1)).
    ``attn`` = dict(ln_w, ln_b, qkv_w, qkv_b, proj_w, proj_b, gamma, bias[, scale]), ``mlp`` = dict(ln_w, ln_b, fc1_w, fc1_b, fc2_w, fc2_b, gamma);
    ``masks`` = dict(attn=, mlp=) per-WINDOW DropPath factors or None (train mode).  x1 is recomputed by the forward kernels, then the two sub-block
    backwards run in reverse order.  Returns dx."""
    ra, rm = _rs(masks, "attn", S), _rs(masks, "mlp", S)
    x1 = attn_block_forward(x, *_attn_args(attn), heads, S, eps, attn.get("scale"), operand_dtype, ra)
    dx1 = mlp_block_backward(x1, dy, *_mlp_args(mlp), mlp_grads, eps, operand_dtype, rm)
    return attn_block_backward(x, dx1, *_attn_args(attn), heads, S, attn_grads, eps, attn.get("scale"), operand_dtype, ra)


def _carrier_permutations(sr0: int, sr1: int, cw: int, device):
    """Index form of the reference's carrier-token reshuffles for G = cw^2 * sr0 * sr1 tokens per image (the view / permute chains of ct_dewindow
    AR:97-102 and ct_window AR:105-110 applied to an arange; the two are inverses only on square grids, which is reproduced):
    dewindowed[:, r] = ct[:, dew[r]];  windowed[:, p] = ct2[:, win[p]]."""
    G = cw * cw * sr0 * sr1
    ar = torch.arange(G, device=device)
    dew = ar.view(sr0, sr1, cw, cw).permute(0, 2, 1, 3).reshape(G)
    win = ar.view(sr1, cw, sr0, cw).permute(0, 2, 1, 3).reshape(G)
    return dew, win


def _upsample_index(ws: int, cw: int, device) -> torch.Tensor:
    """nn.Upsample(size=ws, mode='nearest') of the cw x cw carrier grid of a window (FV:656, 699): carrier slot of window token t."""
    near = (torch.arange(ws, device=device) * cw) // ws
    return (near[:, None] * cw + near[None, :]).reshape(ws * ws)


def _hier_forward_parts(x, ct, hat_attn, hat_mlp, attn, mlp, heads, ws, cw, sr, pe_x, pe_ct, eps, od, masks):
    """Forward of one carrier-token HAT block through the unit kernels, keeping the intermediates the backward starts from."""
    Bw, nloc, C_ = x.shape
    B, G, _ = ct.shape
    sr0, sr1 = int(sr[0]), int(sr[1])
    ncw = cw * cw
    S = ncw + nloc
    dev = x.device
    dew, win = _carrier_permutations(sr0, sr1, cw, dev)
    r_ha, r_hm, r_a, r_m = _rs(masks, "hat_attn", G), _rs(masks, "hat_mlp", G), _rs(masks, "attn", S), _rs(masks, "mlp", S)
    x0 = (x + pe_x.to(dev)) if pe_x is not None else x
    ct0 = ct[:, dew]
    if pe_ct is not None:
        ct0 = ct0 + pe_ct.to(dev)
    ct0 = ct0.reshape(B * G, C_).contiguous()
    ct1 = attn_block_forward(ct0, *_attn_args(hat_attn), heads, G, eps, hat_attn.get("scale"), od, r_ha)
    ct2 = mlp_block_forward(ct1, *_mlp_args(hat_mlp), eps, od, r_hm)
    ctw = ct2.view(B, G, C_)[:, win].reshape(Bw, ncw, C_)
    xin = torch.cat((ctw, x0), dim=1).reshape(Bw * S, C_).contiguous()
    y1 = attn_block_forward(xin, *_attn_args(attn), heads, S, eps, attn.get("scale"), od, r_a)
    return dict(ct0=ct0, ct1=ct1, xin=xin, y1=y1, dew=dew, win=win, rows=(r_ha, r_hm, r_a, r_m), S=S, ncw=ncw)


def hier_block_backward(x: torch.Tensor, ct: torch.Tensor, dx_out: torch.Tensor, dct_out: torch.Tensor, hat_attn: dict, hat_mlp: dict, attn: dict, mlp: dict,
                        heads: int, ws: int, cw: int, sr, pe_x: Optional[torch.Tensor], pe_ct: Optional[torch.Tensor], grads: dict, eps: float = 1e-5,
                        operand_dtype=torch.float16, masks: Optional[dict] = None, prop_gamma=None, prop_grad: Optional[torch.Tensor] = None):
    """Backward of one HAT block WITH carrier tokens (HAT.forward FV:662-701 / AR:668-707):
         x (B nW, ws^2, C), ct (B, G, C)  ->  x_out, ct_out  with the carrier branch (ct_dewindow, hat_pos_embed, hat_attn, hat_mlp, ct_window), the
         concatenation [carrier | window] per window, the window attention and MLP sub-blocks, the final split and -- for the LAST block of a stage built
         with ``do_propagation`` (``prop_gamma``: the block's gamma1, a tensor or the number 1; None = no propagation) -- FV:697-700
         x_out += gamma1 * upsample_nearest(carrier tokens of the window).
    ``hat_attn`` / ``attn`` / ``hat_mlp`` / ``mlp``: parameter dicts as in ``local_block_backward`` (bias = the folded relative-position table of that attention);
    ``pe_x`` (ws^2, C) / ``pe_ct`` (G, C or None): the constant-folded 1-D position embeddings (PosEmbMLPSwinv1D, input independent).
    ``grads`` = dict(hat_attn=AttnGrads, hat_mlp=MlpGrads, attn=AttnGrads, mlp=MlpGrads); ``masks`` = per-image (hat_attn, hat_mlp) / per-window (attn, mlp)
    DropPath factors; ``prop_grad`` (fp32 [C], optional) receives the propagation's share of d gamma1.  Returns (dx, dct).
    The sub-block backwards run on the kernels; the carrier reshuffles, the concatenation / split and the propagation are row gathers / scatters applied
    with torch indexing."""
    _require_hip("hier_block_backward", x)
    Bw, nloc, C_ = x.shape
    B, G, _ = ct.shape
    sr0, sr1 = int(sr[0]), int(sr[1])
    nW, ncw = sr0 * sr1, cw * cw
    if nloc != ws * ws or Bw != B * nW or G != ncw * nW:
        raise RuntimeError(f"hier_block_backward: x {tuple(x.shape)} / ct {tuple(ct.shape)} do not match ws={ws} cw={cw} sr={sr}")
    od = operand_dtype
    f = _hier_forward_parts(x, ct, hat_attn, hat_mlp, attn, mlp, heads, ws, cw, sr, pe_x, pe_ct, eps, od, masks)
    S, dew, win = f["S"], f["dew"], f["win"]
    r_ha, r_hm, r_a, r_m = f["rows"]
    # ---- backward ----
    dctw_out = dct_out.reshape(Bw, ncw, C_)
    if prop_gamma is not None:
        # x_out[w, t] = x2[w, t] + gamma1 * ctr[w, up[t]], ctr = the window's carrier rows AFTER the MLP: recompute them
        y2 = mlp_block_forward(f["y1"], *_mlp_args(mlp), eps, od, r_m).view(Bw, S, C_)
        up = _upsample_index(ws, cw, x.device)
        gam = prop_gamma.detach().float().to(x.device) if isinstance(prop_gamma, torch.Tensor) else None
        if prop_grad is not None and gam is not None:
            prop_grad += (dx_out * y2[:, :ncw][:, up]).sum(dim=(0, 1))
        contrib = dx_out if gam is None else dx_out * gam
        dctw_out = dctw_out.clone().index_add_(1, up, contrib)
    dy2 = torch.cat((dctw_out, dx_out), dim=1).reshape(Bw * S, C_).contiguous()
    dy1 = mlp_block_backward(f["y1"], dy2, *_mlp_args(mlp), grads["mlp"], eps, od, r_m)
    dxin = attn_block_backward(f["xin"], dy1, *_attn_args(attn), heads, S, grads["attn"], eps, attn.get("scale"), od, r_a).view(Bw, S, C_)
    dx = dxin[:, ncw:].contiguous()
    dctw = dxin[:, :ncw].reshape(B, G, C_)
    dct2 = torch.empty_like(dctw)
    dct2[:, win] = dctw                                   # adjoint of windowed[:, p] = ct2[:, win[p]]
    dct2 = dct2.reshape(B * G, C_).contiguous()
    dct1 = mlp_block_backward(f["ct1"], dct2, *_mlp_args(hat_mlp), grads["hat_mlp"], eps, od, r_hm)
    dct0 = attn_block_backward(f["ct0"], dct1, *_attn_args(hat_attn), heads, G, grads["hat_attn"], eps, hat_attn.get("scale"), od, r_ha).view(B, G, C_)
    dct = torch.empty_like(dct0)
    dct[:, dew] = dct0                                    # adjoint of dewindowed[:, r] = ct[:, dew[r]]
    return dx, dct


def hier_block_forward(x: torch.Tensor, ct: torch.Tensor, hat_attn: dict, hat_mlp: dict, attn: dict, mlp: dict, heads: int, ws: int, cw: int, sr,
                       pe_x: Optional[torch.Tensor], pe_ct: Optional[torch.Tensor], eps: float = 1e-5, operand_dtype=torch.float16,
                       masks: Optional[dict] = None, prop_gamma=None):
    """Forward of one HAT block with carrier tokens through the unit kernels (the recompute ``hier_block_backward`` starts from; the train-mode forward):
    returns (x_out, ct_out) in the reference's layouts, x (B nW, ws^2, C), ct (B, G, C).  ``prop_gamma``: see ``hier_block_backward``."""
    Bw, nloc, C_ = x.shape
    B, G, _ = ct.shape
    f = _hier_forward_parts(x, ct, hat_attn, hat_mlp, attn, mlp, heads, ws, cw, sr, pe_x, pe_ct, eps, operand_dtype, masks)
    S, ncw = f["S"], f["ncw"]
    y2 = mlp_block_forward(f["y1"], *_mlp_args(mlp), eps, operand_dtype, f["rows"][3]).view(Bw, S, C_)
    xo, cto = y2[:, ncw:].contiguous(), y2[:, :ncw].reshape(B, G, C_).contiguous()
    if prop_gamma is not None:
        up = _upsample_index(ws, cw, x.device)
        ctr = y2[:, :ncw][:, up]
        xo = xo + (ctr * prop_gamma.detach().float().to(x.device) if isinstance(prop_gamma, torch.Tensor) else ctr)
    return xo, cto


def _table_with_grad(mod, *args):
    """The module's folded-table function (PosEmbMLPSwinv1D.table / PosEmbMLPSwinv2D.table: inference code under @torch.no_grad) run WITH autograd, so
    that a table gradient can continue into the small MLP behind it."""
    fn = type(mod).table
    fn = getattr(fn, "__wrapped__", fn)
    with torch.enable_grad():
        return fn(mod, *args)


def _acc_grad(param, g: torch.Tensor) -> None:
    if isinstance(param, torch.nn.Parameter) and param.requires_grad:
        g = g.to(param.dtype).reshape(param.shape)
        param.grad = g.clone() if param.grad is None else param.grad + g


def _emit(sink: Optional[dict], param, g: torch.Tensor) -> None:
    """Hand one parameter gradient over: into ``sink`` (param -> fp32 gradient; the autograd bridge returns these to the engine, so that
    DistributedDataParallel's reducer and post-accumulate hooks fire exactly once, from the OUTER backward) or, for the direct callers of the
    ``*_stage_backward`` functions (sink None), accumulated into ``.grad``."""
    if not (isinstance(param, torch.nn.Parameter) and param.requires_grad):
        return
    if sink is None:
        _acc_grad(param, g)
        return
    g = g.detach().float().reshape(param.shape)
    sink[param] = g.clone() if param not in sink else sink[param] + g


def _params(mods, trainable_only: bool):
    """The distinct parameters of ``mods`` (None entries skipped), in module order."""
    seen, out = set(), []
    for m in mods:
        for prm in (m.parameters() if m is not None else ()):
            if (prm.requires_grad or not trainable_only) and id(prm) not in seen:
                seen.add(id(prm))
                out.append(prm)
    return out


def _table_grads(sink: Optional[dict], outs, gouts, mods) -> None:
    """Gradients of the folded tables continue into the small MLPs behind them (PosEmbMLPSwinv1D / PosEmbMLPSwinv2D, FV:213-367) with
    ``torch.autograd.grad`` -- NOT ``torch.autograd.backward``: a nested backward would run the parameters' AccumulateGrad nodes (and with them
    DDP's reducer hooks) from inside the outer backward, once on a partial gradient and again from the outer pass."""
    live = [(o, g) for o, g in zip(outs, gouts) if o is not None and g is not None and o.requires_grad]
    params = _params(mods, True)
    if not live or not params:
        return
    gs = torch.autograd.grad([o for o, _ in live], params, [g.to(o.dtype) for o, g in live], allow_unused=True)
    for prm, g in zip(params, gs):
        if g is not None:
            _emit(sink, prm, g)


def _emit_sub(sink: Optional[dict], params: dict, gr) -> None:
    """Hand over the gradients of one sub-block: ``gr`` (AttnGrads / MlpGrads) names its buffers as the parameter dict names the parameters.  The bias
    table is no parameter: its gradient continues through ``_table_grads``."""
    for name, g in vars(gr).items():
        if g is not None and name != "bias":
            _emit(sink, params[name], g)


def drop_path_masks(layer, batch: int, windows_per_image: int, device, generator=None, operand_dtype=torch.float16):
    """Per-block stochastic factors of a stage in TRAIN mode: a list with one dict per block.
      * DropPath (timm semantics, FV:630, 652, 690-691: one Bernoulli(keep) / keep draw per sample of the tensor the DropPath is applied to -- per WINDOW for
        the window branch (x is (B nW, S, C)), per IMAGE for the carrier branch): entries ``attn`` / ``mlp`` / ``hat_attn`` / ``hat_mlp``, None where p = 0;
      * Dropout inside the blocks (r05; ``drop_rate`` of the entrypoints -> ``Mlp.drop`` after GELU and after fc2, FV:404-406, and ``WindowAttention.proj_drop``,
        FV:567): elementwise masks ``<key>_out`` fp32 [rows][C] and ``mlp_hid`` / ``hat_mlp_hid`` operand-dtype [rows][hidden], values 0 or 1 / keep, only where p > 0
        and ``attn_p`` / ``hat_attn_p`` operand-dtype [windows * heads][S][Spad] for ``WindowAttention.attn_drop`` (FV:564: Dropout on the softmax probabilities,
        applied inside the attention kernels)."""
    out = []
    for blk in layer.blocks:
        def draw(n, mod):
            p_ = float(getattr(mod, "drop_prob", 0.0) or 0.0)
            if p_ <= 0.0:
                return None
            keep = 1.0 - p_
            return torch.empty(n, dtype=torch.float32, device=device).bernoulli_(keep, generator=generator) / keep

        def unbiased(keep, dt):
            # the kept value 1 / keep is STORED in dt: in bf16 1 / 0.9 rounds to 1.109375 and E[mask] would be 0.9984 instead of 1.  Draw with the
            # keep probability whose reciprocal is exactly representable -- 1 / round_dt(1 / keep), within 2^-9 of the requested one -- so that E[mask] = 1
            inv = torch.tensor(1.0 / keep, dtype=torch.float32).to(dt).float().item()
            return 1.0 / inv, inv

        def elem(rows, cols, mod, dt=torch.float32):
            p_ = float(getattr(mod, "p", 0.0) or 0.0)
            if p_ <= 0.0:
                return None
            keep, inv = unbiased(1.0 - p_, dt)
            return (torch.empty(rows, cols, dtype=torch.float32, device=device).bernoulli_(keep, generator=generator) * inv).to(dt)

        C_, hid = blk.attn.qkv.in_features, blk.mlp.fc1.out_features
        ncw = blk.cr_window ** 2 if blk.do_sr_hat else 0
        rows = batch * windows_per_image * (blk.window_size ** 2 + ncw)
        lib = _lib.lib()
        S_ = blk.window_size ** 2 + ncw
        heads = blk.attn.num_heads

        def pmask(items, S, mod):   # [items][S][Spad]: the attention kernels index the key axis at the padded stride
            p_ = float(getattr(mod, "p", 0.0) or 0.0)
            if p_ <= 0.0:
                return None
            keep, inv = unbiased(1.0 - p_, operand_dtype)
            return (torch.empty(items, S, lib.fvit_attention_spad(S), dtype=torch.float32, device=device).bernoulli_(keep, generator=generator) * inv).to(operand_dtype)

        m = dict(attn=draw(batch * windows_per_image, blk.drop_path), mlp=draw(batch * windows_per_image, blk.drop_path),
                 attn_out=elem(rows, C_, blk.attn.proj_drop), mlp_out=elem(rows, C_, blk.mlp.drop), mlp_hid=elem(rows, hid, blk.mlp.drop, operand_dtype),
                 attn_p=pmask(batch * windows_per_image * heads, S_, blk.attn.attn_drop))
        if blk.do_sr_hat:
            crow = batch * windows_per_image * ncw
            m.update(hat_attn=draw(batch, blk.hat_drop_path), hat_mlp=draw(batch, blk.hat_drop_path),
                     hat_attn_out=elem(crow, C_, blk.hat_attn.proj_drop), hat_mlp_out=elem(crow, C_, blk.hat_mlp.drop),
                     hat_mlp_hid=elem(crow, hid, blk.hat_mlp.drop, operand_dtype),
                     hat_attn_p=pmask(batch * heads, windows_per_image * ncw, blk.hat_attn.attn_drop))
        out.append(m)
    return out


def _window_geometry(shape, ws: int):
    """Window tiling of a (B, C, H, W) map, as (pad, partition, reverse, nh, nw):
      pad        zeros below / right up to a multiple of ``ws``: F.pad of AR:851-853 on the input and, on dy, the adjoint of the output crop (AR:866-867);
      partition  padded map -> (B nW, ws^2, C) rows in window order (window_partition FV:83-87);
      reverse    rows -> map (window_reverse FV:90-93; the two are each other's adjoint), cropped to H x W (on a gradient: the adjoint of the zero padding)."""
    B, C_, H, W = shape
    Hp, Wp = H + (ws - H % ws) % ws, W + (ws - W % ws) % ws
    nh, nw = Hp // ws, Wp // ws

    def pad(t):
        return torch.nn.functional.pad(t, (0, Wp - W, 0, Hp - H)) if (Hp != H or Wp != W) else t

    def partition(t):
        return t.reshape(B, C_, nh, ws, nw, ws).permute(0, 2, 4, 3, 5, 1).reshape(B * nh * nw, ws * ws, C_).contiguous()

    def reverse(r):
        return r.view(B, nh, nw, ws, ws, C_).permute(0, 5, 1, 3, 2, 4).reshape(B, C_, Hp, Wp).contiguous()[:, :, :H, :W]

    return pad, partition, reverse, nh, nw


def _block_masks(masks, bi: int):
    return None if masks is None else masks[bi]


def _gm(v):
    return v if isinstance(v, torch.Tensor) else None


def _long_enabled(layer) -> bool:
    return bool(layer.__dict__.get("hat_backward_long", False))


def _bias_with_grad(attn, S: int):
    """The relative-position bias of ``attn`` over S tokens, differentiable w.r.t. its cpb_mlp, in the form the attention core takes at this length:
    (autograd output, ``bias`` argument of the sub-block functions).  Up to 64 tokens and wherever the inference path uses the dense-table kernel: the folded
    (heads, S, S) table.  Otherwise the COMPACT table (heads, (2w-1)^2) before the index gather (FV:276-280) with the first S - w^2 tokens carrying no bias
    (carrier tokens of a window; the zero-padded part of a non-square carrier grid, FV:282-299): no (heads, S, S) autograd graph exists for those lengths."""
    mod = attn.pos_emb_funct
    if S <= MAX_SHORT_SEQ or _lib.lib().fvit_attention_dense(S, _dpad(attn.qkv.in_features // attn.num_heads)):
        t = _table_with_grad(mod, S)
        return t, t.detach()
    fn = type(mod).rel_table
    fn = getattr(fn, "__wrapped__", fn)
    with torch.enable_grad():
        t, w = fn(mod)
    if S - w * w < 0:
        raise RuntimeError(f"bias window {w}x{w} larger than the sequence ({S} tokens)")
    return t, CompactBias(t.detach(), int(w), S - w * w)


def _attn_dict(norm, at, gamma, bias) -> dict:
    return dict(ln_w=norm.weight, ln_b=norm.bias, qkv_w=at.qkv.weight, qkv_b=at.qkv.bias, proj_w=at.proj.weight, proj_b=at.proj.bias, gamma=_gm(gamma), bias=bias,
                scale=float(at.scale))


def _mlp_dict(norm, ml, gamma) -> dict:
    return dict(ln_w=norm.weight, ln_b=norm.bias, fc1_w=ml.fc1.weight, fc1_b=ml.fc1.bias, fc2_w=ml.fc2.weight, fc2_b=ml.fc2.bias, gamma=_gm(gamma))


def _grid_table_with_grad(pe, h: int, w: int):
    """``hat_runtime.grid_pos_table`` (the detection backbone's position table over an h x w grid, normalised by (h * w) // 2) run WITH autograd, so
    that its gradient continues into the module's cpb_mlp."""
    from . import hat_runtime
    fn = getattr(hat_runtime.grid_pos_table, "__wrapped__", hat_runtime.grid_pos_table)
    with torch.enable_grad():
        return fn(pe, h, w)


def _block_params(blk, S: int, G: Optional[int] = None, grid=None):
    """(parameter dicts of the block's sub-blocks, its folded tables WITH their autograd graphs): attn / mlp and bias (dense (heads, S, S) or compact
    (heads, (2w-1)^2), differentiable w.r.t. cpb_mlp) / pe_x (ws^2, C); with carrier tokens (``G`` per image) also hat_attn / hat_mlp and hat_bias / pe_ct.
    ``grid`` = (hg, wg), the carrier grid of THIS call of a dynamic-grid layer (the detection backbone; (0, 0) for its carrier-free stages): the position
    tables follow the detection formulas (``hat_runtime.grid_pos_table``: (ws, ws) for the window, (hg, wg) for the carriers, square or not) and the carrier
    attention bias, built for the build-time grid, is padded top / left or cropped to G (``PosEmbMLPSwinv2D.table``: F.pad with a negative pad crops)."""
    bias_t, bias_arg = _bias_with_grad(blk.attn, S)
    P = dict(attn=_attn_dict(blk.norm1, blk.attn, blk.gamma3, bias_arg), mlp=_mlp_dict(blk.norm2, blk.mlp, blk.gamma4))
    ws = blk.window_size
    t = dict(bias=bias_t, pe_x=_table_with_grad(blk.pos_embed) if grid is None else _grid_table_with_grad(blk.pos_embed, ws, ws))
    if G is not None:
        hat_t, hat_arg = _bias_with_grad(blk.hat_attn, G)
        P.update(hat_attn=_attn_dict(blk.hat_norm1, blk.hat_attn, blk.gamma1, hat_arg), hat_mlp=_mlp_dict(blk.hat_norm2, blk.hat_mlp, blk.gamma2))
        if grid is None:
            pe_ct = _table_with_grad(blk.hat_pos_embed) if hasattr(blk, "hat_pos_embed") and blk.square else None
        else:
            pe_ct = _grid_table_with_grad(blk.hat_pos_embed, *grid) if hasattr(blk, "hat_pos_embed") else None
        t.update(hat_bias=hat_t, pe_ct=pe_ct)
    return P, t


def _dynamic(layer) -> bool:
    """A layer that takes its window grid from the padded input of every call (``BackboneLayer.dynamic_grid``: the detection backbone)."""
    return bool(getattr(layer, "dynamic_grid", False))


TOKEN_INIT_DYN_MAX_PIXELS = 16384   # fvit_token_init_dyn(_backward): one conv-output plane in LDS


def token_init_dyn_backward(tok, xp: torch.Tensor, dct: torch.Tensor, ws: int):
    """Backward of ``hat_runtime.token_init_dyn`` through fvit_token_init_dyn_backward: ``xp`` the (B, C, Hp, Wp) window-padded map of the forward call
    (any strides; fp32, fp16 or bf16), ``dct`` the fp32 (B, G, C) gradient of the carrier tokens.  Returns (dx fp32 (B, C, Hp, Wp), dweight fp32 (C, 9),
    dbias fp32 (C,)) -- fresh tensors, nothing is accumulated."""
    from . import hat_runtime
    _require_hip("token_init_dyn_backward", xp)
    B, Cc, Hp, Wp = xp.shape
    cw = tok.window_size
    kh, kw, sh, sw, _, _, Hq, Wq = hat_runtime.token_geometry(Hp, Wp, ws, cw)
    if dct.dtype != torch.float32 or not dct.is_contiguous() or dct.numel() != B * Hq * Wq * Cc or dct.device != xp.device:
        raise RuntimeError(f"token_init_dyn_backward: dct must be a contiguous fp32 ({B}, {Hq * Wq}, {Cc}) tensor on {xp.device}")
    with torch.no_grad(), torch.cuda.device(xp.device):
        w, _ = hat_runtime._token_weights(tok, xp)
        dx = torch.empty(B, Cc, Hp, Wp, dtype=torch.float32, device=xp.device)
        dw = torch.empty(Cc, 9, dtype=torch.float32, device=xp.device)
        db = torch.empty(Cc, dtype=torch.float32, device=xp.device)
        part = torch.empty(B * Cc * 10, dtype=torch.float32, device=xp.device)
        rc = _lib.lib().fvit_token_init_dyn_backward(C.byref(hat_runtime._map_view(xp)), w.data_ptr(), dct.data_ptr(), dx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                                     part.data_ptr(), B, Cc, Hp, Wp, kh, kw, sh, sw, cw, torch.cuda.current_stream(xp.device).cuda_stream)
        _lib.check(rc, "fvit_token_init_dyn_backward")
    return dx, dw, db


def _zero_grads(P: dict, t: dict, C_: int, heads: int, S: int, G: Optional[int], dev) -> dict:
    """Fresh gradient buffers for the sub-blocks of ``_block_params``, under the same keys."""
    hid = P["mlp"]["fc1_w"].shape[0]
    ag = lambda key, n, tab: AttnGrads.zeros(C_, heads, n, dev, with_gamma=P[key]["gamma"] is not None, bias_shape=t[tab].shape)   # noqa: E731
    mg = lambda key: MlpGrads.zeros(C_, hid, dev, with_gamma=P[key]["gamma"] is not None)   # noqa: E731
    if G is None:
        return dict(attn=ag("attn", S, "bias"), mlp=mg("mlp"))
    return dict(hat_attn=ag("hat_attn", G, "hat_bias"), attn=ag("attn", S, "bias"), hat_mlp=mg("hat_mlp"), mlp=mg("mlp"))


def _local_stage_run(layer, x: torch.Tensor, operand_dtype, masks=None):
    """Forward of a carrier-free stage through the unit kernels: (output map, per-block inputs, per-block ``_block_params``, geometry)."""
    C_ = x.shape[1]
    blocks = list(layer.blocks)
    if not blocks or any(b.do_sr_hat for b in blocks):
        raise RuntimeError("local stage: the stage must consist of HAT blocks without carrier tokens")
    ws = blocks[0].window_size
    heads, S = blocks[0].attn.num_heads, ws * ws
    if S > 64 and not _long_enabled(layer):
        raise RuntimeError(f"local stage: windows of {S} tokens (the attention-core backward holds at most 64)")
    pad, partition, reverse, _, _ = _window_geometry(x.shape, ws)
    rows = partition(pad(x.float())).view(-1, C_)
    ins, ps = [], []
    grid = (0, 0) if _dynamic(layer) else None
    for bi, blk in enumerate(blocks):
        P, t = _block_params(blk, S, grid=grid)
        mk = _block_masks(masks, bi)
        xin = (rows.view(-1, S, C_) + t["pe_x"].detach().to(rows.dtype)).reshape(-1, C_).contiguous()
        ins.append(xin)
        ps.append((P, t))
        x1 = attn_block_forward(xin, *_attn_args(P["attn"]), heads, S, 1e-5, P["attn"]["scale"], operand_dtype, _rs(mk, "attn", S))
        rows = mlp_block_forward(x1, *_mlp_args(P["mlp"]), 1e-5, operand_dtype, _rs(mk, "mlp", S))
    return reverse(rows), ins, ps, dict(pad=pad, partition=partition, reverse=reverse, heads=heads, S=S)


def local_stage_backward(layer, x: torch.Tensor, dy: torch.Tensor, operand_dtype=torch.float16, sink: Optional[dict] = None, masks=None) -> torch.Tensor:
    """Backward of the transformer branch of a FasterViTLayer WITHOUT carrier tokens (FasterViTLayer.forward FV:832-841 / AR:848-869 with only-local HAT blocks:
    stage 3) -- zero padding to a multiple of the window, window_partition, depth x HAT block, window_reverse, crop -- for the module's own parameters:

      x, dy: (B, C, H, W) fp32 maps;  returns dx and ADDS every parameter gradient of ``layer.blocks`` into ``.grad`` (``sink`` None) or into the dict
      ``sink`` (param -> gradient; nothing is written to ``.grad`` then: the autograd bridge below) -- norm1 / norm2, attn.qkv / attn.proj, mlp.fc1 / fc2,
      gamma3 / gamma4 when they are parameters, and -- through the modules' differentiable ``table()`` functions on the host -- the cpb_mlp of the
      relative-position bias and of the 1-D position embedding, from the table gradients the kernels return.  ``masks``: ``drop_path_masks`` of a
      train-mode forward (the same draws must be passed to the forward and the backward).

    Forward activations are recomputed block by block with the unit kernels (one fp32 row checkpoint per block boundary); the block backwards are
    ``local_block_backward``.  The downsample conv of the layer is not part of this path."""
    _require_hip("local_stage_backward", x)
    C_ = x.shape[1]
    blocks = list(layer.blocks)
    _, ins, ps, gm = _local_stage_run(layer, x, operand_dtype, masks)
    heads, S = gm["heads"], gm["S"]
    d = gm["partition"](gm["pad"](dy.float())).view(-1, C_)
    for bi in range(len(blocks) - 1, -1, -1):
        blk, xin, (P, t) = blocks[bi], ins[bi], ps[bi]
        grads = _zero_grads(P, t, C_, heads, S, None, x.device)
        d = local_block_backward(xin, d, P["attn"], P["mlp"], heads, S, grads["attn"], grads["mlp"], 1e-5, operand_dtype, _block_masks(masks, bi))
        for key, gr in grads.items():
            _emit_sub(sink, P[key], gr)
        # the folded tables are functions of small MLPs: their gradients continue on the host through the modules' own table() code
        _table_grads(sink, [t["bias"], t["pe_x"]], [grads["attn"].bias, d.view(-1, S, C_).sum(0)], [blk.attn.pos_emb_funct, blk.pos_embed])
    return gm["reverse"](d).contiguous()


def _prop_gamma(blk):
    """gamma1 of the last block when the stage propagates carrier tokens into the map (FV:697-700; the reference re-uses gamma1 here), else None."""
    if blk.last and blk.do_propagation and blk.do_sr_hat:
        return blk.gamma1 if isinstance(blk.gamma1, torch.Tensor) else 1.0
    return None


def _hier_stage_run(layer, x: torch.Tensor, operand_dtype, masks=None):
    """Forward of a carrier-token stage through the unit kernels: (output map, per-block (rows, ct) checkpoints, per-block ``_block_params``, geometry)."""
    H, W = x.shape[2:]
    blocks = list(layer.blocks)
    if not blocks or not all(b.do_sr_hat for b in blocks):
        raise RuntimeError("hier stage: the stage must consist of carrier-token HAT blocks")
    b0 = blocks[0]
    ws, cw, sr = b0.window_size, b0.cr_window, tuple(b0.sr_ratio)
    pad, partition, reverse, nh, nw = _window_geometry(x.shape, ws)
    grid = None
    if _dynamic(layer):
        # the detection backbone: the window grid is the one of THIS padded input (b0.sr_ratio is the build-time grid), the carrier grid the tokenizer's
        # (hg, wg) for it, and the tokenizer runs (and is differentiated, hier_stage_backward) on its own kernels -- no host autograd graph
        from . import hat_runtime
        sr = (nh, nw)
        xp_leaf = pad(x.detach().float())
        x_leaf = None
        grid = tuple(hat_runtime.token_geometry(nh * ws, nw * ws, ws, cw)[6:8])
        if grid != (cw * nh, cw * nw):
            raise RuntimeError(f"hier stage: carrier grid {grid[0]}x{grid[1]} of a {nh * ws}x{nw * ws} map does not match {nh}x{nw} windows of {cw}x{cw} carriers")
        ct_init = hat_runtime.token_init_dyn(layer.global_tokenizer, xp_leaf, ws)
    else:
        x_leaf = x.detach().float().requires_grad_(True)
        with torch.enable_grad():
            xp_leaf = pad(x_leaf)                            # the TokenInitializer sees the padded map (AR:851-858)
            if (nh, nw) != sr:
                raise RuntimeError(f"hier stage: map {H}x{W} (padded {nh * ws}x{nw * ws}) does not tile into the stage's {sr[0]}x{sr[1]} windows of {ws}")
            ct_init = layer.global_tokenizer(xp_leaf)
    heads, ncw = b0.attn.num_heads, cw * cw
    G, S = ncw * nh * nw, ncw + ws * ws
    if (S > 64 or G > 64) and not _long_enabled(layer):
        raise RuntimeError(f"hier stage: {S} tokens per window / {G} carrier tokens per image (the attention-core backward holds at most 64)")
    rows, ct = partition(xp_leaf.detach()), ct_init.detach().float().contiguous()
    ckpt, ps = [], []
    for bi, blk in enumerate(blocks):
        P, t = _block_params(blk, S, G, grid=grid)
        ckpt.append((rows, ct))
        ps.append((P, t))
        rows, ct = hier_block_forward(rows, ct, P["hat_attn"], P["hat_mlp"], P["attn"], P["mlp"], heads, ws, cw, sr, t["pe_x"].detach(),
                                      None if t["pe_ct"] is None else t["pe_ct"].detach(), 1e-5, operand_dtype, _block_masks(masks, bi), _prop_gamma(blk))
    return reverse(rows), ckpt, ps, dict(pad=pad, partition=partition, reverse=reverse, heads=heads, S=S, G=G, ws=ws, cw=cw, sr=sr, x_leaf=x_leaf, ct_init=ct_init,
                                         xp=xp_leaf if grid is not None else None)


def hier_stage_backward(layer, x: torch.Tensor, dy: torch.Tensor, operand_dtype=torch.float16, sink: Optional[dict] = None, masks=None) -> torch.Tensor:
    """Backward of the transformer branch of a FasterViTLayer WITH carrier tokens (FasterViTLayer.forward FV:832-841 / AR:848-869: zero padding, TokenInitializer,
    window_partition, depth x hierarchical HAT block incl. the last block's carrier propagation (``do_propagation``: FasterViT-3 and up), window_reverse, crop):
    returns dx (B, C, H, W) and hands over the gradient of every parameter of ``layer.blocks`` and ``layer.global_tokenizer`` (``.grad`` / ``sink`` as in
    ``local_stage_backward``).  The HAT blocks run on the kernels (``hier_block_forward`` checkpoints per block, ``hier_block_backward``); the TokenInitializer
    (one depthwise conv + average pool, FV:704-738) and the four folded tables per block are small torch modules differentiated by autograd on the host side."""
    _require_hip("hier_stage_backward", x)
    B, C_ = x.shape[:2]
    blocks = list(layer.blocks)
    _, ckpt, ps, gm = _hier_stage_run(layer, x, operand_dtype, masks)
    heads, S, G, ws, cw, sr = gm["heads"], gm["S"], gm["G"], gm["ws"], gm["cw"], gm["sr"]
    d = gm["partition"](gm["pad"](dy.float()))
    dct = torch.zeros(B, G, C_, dtype=torch.float32, device=x.device)   # the stage's final carrier tokens are dropped (FV:841)
    dew, _ = _carrier_permutations(sr[0], sr[1], cw, x.device)
    for bi in range(len(blocks) - 1, -1, -1):
        blk, (xb, ctb), (P, t) = blocks[bi], ckpt[bi], ps[bi]
        grads = _zero_grads(P, t, C_, heads, S, G, x.device)
        pg = _prop_gamma(blk)
        prop_grad = torch.zeros(C_, dtype=torch.float32, device=x.device) if isinstance(pg, torch.Tensor) else None
        d, dct = hier_block_backward(xb, ctb, d, dct, P["hat_attn"], P["hat_mlp"], P["attn"], P["mlp"], heads, ws, cw, sr, t["pe_x"].detach(),
                                     None if t["pe_ct"] is None else t["pe_ct"].detach(), grads, 1e-5, operand_dtype, _block_masks(masks, bi), pg, prop_grad)
        if prop_grad is not None:
            _emit(sink, blk.gamma1, prop_grad)
        for key, gr in grads.items():
            _emit_sub(sink, P[key], gr)
        # folded tables -> their small MLPs (host autograd): d pe_x = sum over windows of dx, d pe_ct = sum over images of the dewindowed carrier gradient
        outs, gouts = [t["bias"], t["hat_bias"], t["pe_x"]], [grads["attn"].bias, grads["hat_attn"].bias, d.sum(0)]
        if t["pe_ct"] is not None:
            outs.append(t["pe_ct"])
            gouts.append(dct[:, dew].sum(0))
        _table_grads(sink, outs, gouts, [blk.attn.pos_emb_funct, blk.hat_attn.pos_emb_funct, blk.pos_embed, getattr(blk, "hat_pos_embed", None)])
    if gm["xp"] is not None:
        # ---- dynamic grid: the tokenizer's backward is fvit_token_init_dyn_backward, on the padded map; the crop is the adjoint of the zero padding ----
        tok = layer.global_tokenizer
        dxp, dw, db = token_init_dyn_backward(tok, gm["xp"], dct.contiguous(), ws)
        _emit(sink, tok.pos_embed.weight, dw)
        _emit(sink, tok.pos_embed.bias, db)
        return (gm["reverse"](d) + dxp[:, :, :x.shape[2], :x.shape[3]]).contiguous()
    # ---- the carrier tokens came from the tokenizer: its conv parameters and its share of dx (autograd.grad: no .grad is touched) ----
    x_leaf, ct_init = gm["x_leaf"], gm["ct_init"]
    tok_params = _params([layer.global_tokenizer], True)
    gs = torch.autograd.grad([ct_init], tok_params + [x_leaf], [dct.to(ct_init.dtype)], allow_unused=True)
    for prm, g in zip(tok_params, gs[:-1]):
        if g is not None:
            _emit(sink, prm, g)
    dx_tok = gs[-1]
    dx = gm["reverse"](d)
    return (dx + dx_tok if dx_tok is not None else dx).contiguous()


def stage_forward_train(layer, x: torch.Tensor, operand_dtype=torch.float16, masks=None) -> torch.Tensor:
    """The transformer branch of a FasterViTLayer through the unit kernels with stochastic depth (``masks`` = ``drop_path_masks``): the TRAIN-mode forward
    (the fused inference kernels implement eval semantics).  Same checkpoints as the backward's recompute."""
    fn = _hier_stage_run if layer.blocks[0].do_sr_hat else _local_stage_run
    return fn(layer, x, operand_dtype, masks)[0].to(x.dtype).contiguous()


# --------------------------------------------------------------------------------------------------------------------------------------
# autograd bridge: the transformer branch of a FasterViTLayer as ONE autograd node (forward: fvit_hat_stage_forward, backward: the functions above)
# --------------------------------------------------------------------------------------------------------------------------------------


def operand_torch_dtype(layer) -> torch.dtype:
    """16-bit operand type of the backward kernels for this layer: the type of its forward operand mode (``hat_operand_dtype``; the two- and
    three-term modes recompute and differentiate with single 16-bit terms of the same type)."""
    return torch.bfloat16 if str(getattr(layer, "hat_operand_dtype", "f16")).startswith("bf16") else torch.float16


def backward_unsupported_reason(layer, H: Optional[int] = None, W: Optional[int] = None) -> Optional[str]:
    """None if the kernel-sequence backward (and train-mode forward) covers this stage (and, when given, this map size); otherwise the reason, as text.
    Checked at FORWARD time (``stage_forward_with_grad``) and by ``FasterViT.enable_hat_backward``: a stage that cannot be differentiated must not fail
    from inside ``loss.backward()`` on the autograd engine's thread after a forward that succeeded.
    Covered: head_dim <= 96 (run padded to 32 / 64 / 96), C a multiple of 16, hidden a multiple of 64, windows and carrier grids of at most 64 tokens,
    maps padded up to a multiple of the window, the last block's carrier propagation -- i.e. every reference entrypoint at its native 224 x 224
    resolution; not the 384+ / any-res geometries with longer windows.
    With ``layer.hat_backward_long`` (``FasterViT.enable_hat_backward(True, long_sequences=True)``) windows and carrier grids of ANY length are covered
    (fvit_bwd_window_attention_long); still refused: head_dim > 96, C % 16, hidden % 64, mixed stages, a map that does not tile a fixed-grid stage, and --
    in TRAIN mode -- ``attn_drop`` > 0 on a sequence above 64 tokens (the long backward has no Dropout mask on the probabilities)."""
    blocks = list(layer.blocks)
    if not blocks:
        return None
    b0 = blocks[0]
    C_, heads = b0.attn.qkv.in_features, b0.attn.num_heads
    hid = b0.mlp.fc1.out_features
    ws = b0.window_size
    hier = bool(b0.do_sr_hat)
    if C_ % heads or C_ // heads > 96:
        return f"head_dim {C_ // max(heads, 1)} (the attention kernels cover head_dim <= 96)"
    if C_ % 16 or hid % 64:
        return f"C = {C_} must be a multiple of 16 and hidden = {hid} a multiple of 64"
    if any(bool(b.do_sr_hat) != hier for b in blocks):
        return "mixed hierarchical / local blocks in one stage"
    ncw = b0.cr_window ** 2 if hier else 0
    long = _long_enabled(layer)
    if ws * ws + ncw > 64 and not long:
        return f"windows of {ws * ws + ncw} tokens (the attention-core backward holds at most 64 in LDS)"
    dyn = _dynamic(layer)
    if dyn and hier and H is not None:
        nh_, nw_ = -(-H // ws), -(-W // ws)
        if nh_ * ws * nw_ * ws > TOKEN_INIT_DYN_MAX_PIXELS:
            return (f"map {H}x{W} pads to {nh_ * ws}x{nw_ * ws} = {nh_ * ws * nw_ * ws} pixels (the carrier-token initialiser holds one plane of at most "
                    f"{TOKEN_INIT_DYN_MAX_PIXELS} pixels in LDS)")
    if long and layer.training:
        pd = lambda at: float(getattr(at.attn_drop, "p", 0.0) or 0.0)   # noqa: E731
        G_ = ncw * b0.sr_ratio[0] * b0.sr_ratio[1] if hier else 0
        if dyn and hier:   # the grid of this call; unknown at enable time (H None): checked at forward time
            G_ = ncw * (-(-H // ws)) * (-(-W // ws)) if H is not None else 0
        for b in blocks:
            if ws * ws + ncw > 64 and pd(b.attn) > 0:
                return f"attn_drop = {pd(b.attn)} in train mode on windows of {ws * ws + ncw} tokens (the attention-core backward above 64 tokens has no Dropout mask)"
            if hier and G_ > 64 and pd(b.hat_attn) > 0:
                return f"attn_drop = {pd(b.hat_attn)} in train mode on {G_} carrier tokens per image (the attention-core backward above 64 tokens has no Dropout mask)"
    if hier and not dyn:
        sr = tuple(b0.sr_ratio)
        if ncw * sr[0] * sr[1] > 64 and not long:
            return f"{ncw * sr[0] * sr[1]} carrier tokens per image (at most 64)"
        if H is not None and (-(-H // ws), -(-W // ws)) != sr:
            return f"map {H}x{W} does not pad into the stage's {sr[0]}x{sr[1]} windows of {ws}"
    return None


class HatStageFunction(torch.autograd.Function):
    """y = FasterViTLayer transformer branch (x) with the module's parameters as differentiable inputs.
    Forward: eval mode = the HIP inference path (``fvit_hat_stage_forward``, fused kernels); TRAIN mode = the unit-kernel chain with stochastic depth
    (``stage_forward_train``; the DropPath draws are kept for the backward).  Backward = local_stage_backward / hier_stage_backward, whose parameter
    gradients are collected in a dict and RETURNED to autograd (so hooks such as DistributedDataParallel's fire once, from the outer engine); neither
    ``.grad`` nor any AccumulateGrad node is touched from inside this backward (tables and tokenizer: ``torch.autograd.grad``).

    fp16 operands: every gradient inside the kernel sequence (dz, dO, dqkv, dh, da and their transposes) is narrowed to 16 bits.  The backward is linear
    in dy, so dy is scaled by a power of two that brings its largest entry to ~2^10 and dx / the parameter gradients are scaled back in fp32: a mean-reduced
    loss (dy ~ 1e-6) or a 1e-5 layer scale would otherwise sit in or below the fp16 subnormals (spacing 6e-8).  bf16 operands need no scaling."""

    @staticmethod
    def forward(ctx, x, layer, operand_dtype, *params):
        from . import hat_runtime
        ctx.layer, ctx.operand_dtype, ctx.params = layer, operand_dtype, params
        ctx.save_for_backward(x)
        ctx.masks = None
        if layer.training:
            b0 = layer.blocks[0]
            ws = b0.window_size
            nW = (-(-x.shape[2] // ws)) * (-(-x.shape[3] // ws))
            ctx.masks = drop_path_masks(layer, x.shape[0], nW, x.device, operand_dtype=operand_dtype)
            return stage_forward_train(layer, x.detach(), operand_dtype, ctx.masks)
        tok = None
        if _dynamic(layer) and layer.do_gt and layer.blocks[0].do_sr_hat:   # as BackboneLayer.forward: the tokenizer of this call's geometry
            tok = lambda xp: hat_runtime.token_init_dyn(layer.global_tokenizer, xp, layer.window_size)  # noqa: E731
        return hat_runtime.stage_forward(layer, x.detach(), tokenizer=tok)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        layer, params = ctx.layer, ctx.params
        dy32 = dy.float().contiguous()
        inv = None
        if ctx.operand_dtype == torch.float16:
            amax = dy32.abs().amax().clamp_min(1e-30)
            scale = torch.exp2(torch.floor(torch.log2(1024.0 / amax)))   # 0-dim tensor on the device: no host synchronisation
            dy32 = dy32 * scale
            inv = 1.0 / scale
        sink: dict = {}
        fn = hier_stage_backward if layer.blocks[0].do_sr_hat else local_stage_backward
        dx = fn(layer, x.float().contiguous(), dy32, ctx.operand_dtype, sink=sink, masks=ctx.masks)
        if inv is not None:
            dx = dx * inv
        grads = []
        for prm in params:
            g = sink.get(prm)
            if g is not None and inv is not None:
                g = g * inv
            grads.append(None if g is None else g.to(prm.dtype))
        return (dx.to(x.dtype), None, None, *grads)


def stage_forward_with_grad(layer, x: torch.Tensor, operand_dtype=None) -> torch.Tensor:
    """``hat_runtime.stage_forward`` as a differentiable op (see HatStageFunction); in TRAIN mode the forward has train semantics (stochastic depth).
    ``operand_dtype`` None = the 16-bit type of the layer's forward operand mode.  Unsupported geometries raise HERE, at forward time."""
    if len(layer.blocks) == 0:
        return x
    why = backward_unsupported_reason(layer, x.shape[2], x.shape[3])
    if why is not None:
        raise RuntimeError(f"stage_forward_with_grad: this HAT stage has no kernel-sequence backward / train-mode forward: {why}. Run it forward-only in eval "
                           "mode under torch.no_grad() (model.enable_hat_backward(False)).")
    if operand_dtype is None:
        operand_dtype = operand_torch_dtype(layer)
    stage_mods = [layer.blocks] + ([layer.global_tokenizer] if getattr(layer, "do_gt", False) and hasattr(layer, "global_tokenizer") else [])
    return HatStageFunction.apply(x, layer, operand_dtype, *_params(stage_mods, False))


# --------------------------------------------------------------------------------------------------------------------------------------
# the detection backbone's output tap (crop + eval BatchNorm2d + contiguous NCHW fp32, fvit_feature_tap) as a differentiable op
# --------------------------------------------------------------------------------------------------------------------------------------


def feature_tap_backward(dout: torch.Tensor, x: torch.Tensor, scale: torch.Tensor, H: Optional[int] = None, W: Optional[int] = None):
    """Backward of ``hat_runtime.feature_tap`` through fvit_feature_tap_backward: ``dout`` fp32 (B, C, H, W), ``x`` the (B, C, Hs, Ws) stage map the forward
    read (any strides; fp32, fp16 or bf16; H, W default to its extents), ``scale`` fp32 [C] the folded BatchNorm factor.  Returns (dx, sum_d, sum_dx): dx fp32 in
    x's layout (scale[c] * dout on the crop, zero on the rest of the view) and the per-channel sums of dout and dout * x over the crop."""
    from . import hat_runtime
    _require_hip("feature_tap_backward", x)
    B, Cc, Hs, Ws = x.shape
    H, W = Hs if H is None else int(H), Ws if W is None else int(W)
    if tuple(dout.shape) != (B, Cc, H, W) or dout.device != x.device or not (0 < H <= Hs and 0 < W <= Ws):
        raise RuntimeError(f"feature_tap_backward: dout {tuple(dout.shape)} is not the {H}x{W} crop of the {tuple(x.shape)} map on {x.device}")
    with torch.no_grad(), torch.cuda.device(x.device):
        dout = dout.float().contiguous()
        dx = torch.empty_like(x, dtype=torch.float32)
        rows = B * Hs * (-(-Ws // 64))
        part = torch.empty(2 * rows * Cc, dtype=torch.float32, device=x.device)
        sums = torch.empty(2, Cc, dtype=torch.float32, device=x.device)
        rc = _lib.lib().fvit_feature_tap_backward(dout.data_ptr(), C.byref(hat_runtime._map_view(x)), C.byref(hat_runtime._map_view(dx)), B, Cc, H, W, Hs, Ws,
                                                  scale.data_ptr(), part.data_ptr(), part.numel(), sums.data_ptr(),
                                                  torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(rc, "fvit_feature_tap_backward")
    return dx, sums[0], sums[1]


class FeatureTapFunction(torch.autograd.Function):
    """out = eval BatchNorm2d(x) as contiguous NCHW fp32 (``hat_runtime.feature_tap``) with x and the BatchNorm's weight / bias as differentiable inputs:
    dx = scale[c] * dout, dbias = sum dout, dweight = (sum dout * x - mean * sum dout) * rsqrt(var + eps), the sums from fvit_feature_tap_backward.  The
    gradients are RETURNED to autograd (hooks fire once, from the outer engine)."""

    @staticmethod
    def forward(ctx, x, bn, weight, bias):
        from . import hat_runtime
        ctx.bn = bn
        ctx.save_for_backward(x)
        return hat_runtime.feature_tap(x.detach(), bn)

    @staticmethod
    def backward(ctx, dout):
        from . import hat_runtime
        (x,) = ctx.saved_tensors
        bn = ctx.bn
        scale, _ = hat_runtime._folded_bn(bn, x.device)
        dx, sd, sdx = feature_tap_backward(dout, x, scale)
        gw = gb = None
        if bn.weight is not None and ctx.needs_input_grad[2]:
            gw = ((sdx.double() - bn.running_mean.double() * sd.double()) * torch.rsqrt(bn.running_var.double() + bn.eps)).to(bn.weight.dtype)
        if bn.bias is not None and ctx.needs_input_grad[3]:
            gb = sd.to(bn.bias.dtype)
        return (dx.to(x.dtype) if ctx.needs_input_grad[0] else None), None, gw, gb


def feature_tap_with_grad(x: torch.Tensor, bn) -> torch.Tensor:
    """``hat_runtime.feature_tap(x, bn)`` as a differentiable op (``bn`` in eval mode: running statistics)."""
    _require_hip("feature_tap", x)
    if bn.training:
        raise RuntimeError("feature_tap_with_grad: the BatchNorm2d is in training mode (batch statistics); the fused tap folds the RUNNING statistics -- run the module")
    return FeatureTapFunction.apply(x, bn, bn.weight, bn.bias)
