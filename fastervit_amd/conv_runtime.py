"""Deploy-mode plan for the conv side of FasterViT.

In module mode the convolutions are plain PyTorch-ROCm / MIOpen modules (north_star's drop-in default).  The deploy plan
runs the conv side through this library's own kernels instead and removes everything input-independent from the
per-forward path:

  * BatchNorm (eval) is folded into the preceding conv's weights and bias at load:
        PatchEmbed  conv(no bias)+BN(eps 1e-4)          (FV:458-463)
        ConvBlock   conv1+BN1, conv2+BN2 (+gamma)        (FV:490-512)
        final BN + AdaptiveAvgPool2d(1) + head           (FV:925-927, 953-960) -> one fp32 Linear on the pooled map
    exact in real arithmetic; weights are kept as 16-bit channels_last tensors ([Cout][3][3][Cin] matrices), so there is
    no autocast and no per-forward cast of parameters.
  * every 3x3 convolution (+ folded bias + ReLU / GELU + residual) is ONE hand-written HIP kernel (the driver of csrc/fvit_conv.hip over
    csrc/fvit_conv_gemm.hip: implicit GEMM, fvit_conv_halo.hip: halo-tiled 64-channel conv, fvit_conv_band.hip: row-band 128-channel conv;
    csrc/fvit_stem.hip: fused two-conv stem); channel counts that are not a multiple of 64 are
    zero-padded to one (``pad_channels``).  MIOpen (``F.conv2d``) + the glue passes of csrc/fvit_glue.hip remain only as the
    fallback for shapes those kernels do not cover (``pad_channels = False`` or ``use_hip_conv = False``).
  * timm's LayerNorm2d (Downsample) is one HBM pass (``ln2d_kernel``) -- or, in the 16-bit classifier plan, no pass at all: it runs in the epilogue of
    the kernel that produces the level's last map (the residual conv of the last ConvBlock, the window_reverse of a transformer level), from the
    rounded 16-bit values that kernel would have stored (``fuse_conv_ln2d`` / ``fuse_reverse_ln2d``).  A one-window last level is pooled straight
    from its token rows (``fuse_pool``): the mean over a window's tokens does not depend on their order.
  * The transformer stages are the same ``fvit_hat_stage_forward`` calls as in module mode.

  * ``plan.precise = True`` (r05; ``compile_inference(..., precise=True)``): the plan that meets north_star's ABSOLUTE logits bar on the deep / wide
    variants.  A replay of the fp32 oracle with single roundings placed one at a time (tests/tools/conv_precision_sim.py, FasterViT-4) shows that a
    16-bit conv OPERAND costs 2-8e-5 but a 16-bit STORED stream 3-4e-4 each (the residual stream of levels 0 / 1, the Downsample outputs, the
    transformer levels' output maps), the LayerNorm2d -> strided-conv operand 3.6e-4 and the K = 27 stem conv's weights / image 2.2e-4 / 1.2e-4.
    So here every stream is a TWO-TERM map (two 16-bit planes, value = hi + lo; the hi plane alone is the next conv's MFMA operand) or fp32
    where the consumer is a transformer level; all conv weights are hi + lo; the three Downsample convs and the first stem conv also take their
    input as two terms (hi.hi + hi.lo + lo.hi).  Kernels: ``conv3x3_kernel<.., PX>``, ``ln2d_kernel<.., PX>``, ``stem_conv_kernel<.., PX>``.

Both plans share ONE walk over the levels (``DeployPlan._forward_one``); what differs -- stem, ConvBlocks, the dtype of a transformer level's maps, Downsample,
head -- sits in the per-step methods behind it, which branch on ``precise``.  The folded weights live in ``plan.t`` as NamedTuples (``ConvWeight``, ``StemW``, ...).

Enabled by ``FasterViT.switch_to_deploy()`` (explicit) or automatically for eval-mode forwards under ``torch.autocast`` with grad
disabled (``FasterViT.auto_deploy``); module mode (plain nn.Module forward, any dtype) remains the default so that the
reference's scripts run unchanged.  Logits of the 16-bit plan differ from the fp32 reference by the conv side's 16-bit rounding:
measured 6.5e-4 .. 9.5e-4 max-abs on FasterViT-0 (asserted < 1e-3 in tests/test_gpu_parity.py).
"""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _lib, hat_runtime

_CODE = {torch.float16: _lib.FVIT_F16, torch.bfloat16: _lib.FVIT_BF16}


def _bn_scale_shift(bn):
    s = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
    t = bn.bias.float() - bn.running_mean.float() * s
    return s, t


def _fold(conv, bn, extra_scale=None):
    """conv (+ optional bias) followed by eval-mode BN (and an optional per-channel scale) -> (w, b) fp32."""
    s, t = _bn_scale_shift(bn)
    w = conv.weight.float() * s.view(-1, 1, 1, 1)
    b = t if conv.bias is None else conv.bias.float() * s + t
    if extra_scale is not None:
        w = w * extra_scale.float().view(-1, 1, 1, 1)
        b = b * extra_scale.float()
    return w, b


def frag_pack_conv128(w2d: torch.Tensor) -> torch.Tensor:
    """[128][9 * 128] conv weight (row = output channel, column k = tap * 128 + input channel) -> the fragment-order stream of
    row-band conv kernel (FvitConvWeights.band_frag, include/fvit_hip.h): [wave 4][step 36][ni 2][lane 64][8]; element e of lane 16 g + s of fragment
    (wave, step, ni) = w2d[32 wave + (s >> 2) * 8 + ni * 4 + (s & 3)][step * 32 + 8 g + e]."""
    assert tuple(w2d.shape) == (128, 1152)
    dev = w2d.device
    wave = torch.arange(4, device=dev).view(4, 1, 1)
    ni = torch.arange(2, device=dev).view(1, 2, 1)
    sl = torch.arange(16, device=dev).view(1, 1, 16)
    ch = (32 * wave + (sl >> 2) * 8 + ni * 4 + (sl & 3)).reshape(-1)        # [wave, ni, s]
    t = w2d[ch].view(4, 2, 16, 36, 4, 8)                                      # wave, ni, s, step, g, e
    return t.permute(0, 3, 1, 4, 2, 5).contiguous().view(4, 36, 2, 64, 8)    # wave, step, ni, (g, s), e


class ConvWeight(NamedTuple):
    """One conv's packed weights (``DeployPlan._cw``)."""
    wcl: torch.Tensor                    # channels_last 16-bit tensor for F.conv2d (the MIOpen fallback)
    wk: Optional[torch.Tensor]           # rows of the implicit-GEMM kernel, [Cout][terms][3][3][Cin] or dense-K [Cout][terms][kd]; None: shape not covered
    wband: Optional[torch.Tensor]        # 128 -> 128 channels: the fragment-order stream of the row-band kernel
    terms: int                           # weight terms in wk (2 = hi | lo)
    cv: int                              # channels wk contracts over per tap
    wk_classic: Optional[torch.Tensor]   # beside a dense-K wk: the classic rows, which the patch form of the kernel takes

    def images(self) -> _lib.FvitConvWeights:
        """Every packed image for the conv driver (``fvit_conv3x3``): ``wk`` is the dense image when ``wk_classic`` is set, the classic one otherwise."""
        classic, dense = (self.wk, None) if self.wk_classic is None else (self.wk_classic, self.wk)
        return _lib.FvitConvWeights(_lib.ptr(classic), _lib.ptr(dense), _lib.ptr(self.wband), self.terms, self.cv)


# the entries of ``DeployPlan.t`` (``_build``); biases and LayerNorm2d parameters are fp32, zero-padded to the map layout
StemW = NamedTuple("StemW", [("conv0", ConvWeight), ("bias0", torch.Tensor), ("conv1", ConvWeight), ("bias1", torch.Tensor)])     # t["stem"]
BlockW = NamedTuple("BlockW", [("conv1", ConvWeight), ("bias1", torch.Tensor), ("conv2", ConvWeight), ("bias2", torch.Tensor)])   # t["levels"][i]["blocks"][j]
DownW = NamedTuple("DownW", [("ln_w", torch.Tensor), ("ln_b", torch.Tensor), ("eps", float), ("conv", ConvWeight), ("cin", int)])  # t["levels"][i]["down"]
TokW = NamedTuple("TokW", [("w", torch.Tensor), ("bias", torch.Tensor), ("pool_kernel", object), ("pool_stride", object), ("window", int)])  # t["levels"][i]["tok"]: UNUSED (the stage kernels run the tokenizer: fvit_token_init), kept for the layout of t
HeadW = NamedTuple("HeadW", [("w", torch.Tensor), ("b", torch.Tensor), ("ln", Optional[tuple])])   # t["head"]; ln = (weight, bias, eps) with layer_norm_last


class DeployPlan:
    def __init__(self, model, dtype=torch.float16):
        if dtype not in _CODE:
            raise ValueError("deploy dtype must be torch.float16 or torch.bfloat16")
        self.model = model
        self.dtype = dtype
        self.code = _CODE[dtype]
        self.sig = None
        self.t = None
        self.zeros = None
        self.streams = 1      # > 1: run the batch as that many shards on separate HIP streams
        self.shard_sizes = None        # images per shard (a list that sums to the batch); None = equal chunks
        self.serialize_shards = False  # the shards one after the other on the caller's stream (bench.py's HIP-event pass)
        self.join_from = None          # level in front of which the shards join (_forward_sharded); None = after the head
        self.slot_base = 0             # first stage-workspace slot of this plan (_forward_sharded)
        self._warm_geometries = set()  # shard geometries that have completed one serial pass (_forward_sharded)
        self.side = None
        self.dev = None       # device of the current forward (raw-pointer launches go to torch's current stream on THIS device)
        self.use_hip_conv = True  # fused implicit-GEMM conv kernel where the shape allows; False = MIOpen + glue passes
        # conv-side maps carry their channels padded to a multiple of 64 (zeros), weights / biases / LayerNorm2d parameters are
        # zero-padded to match: every 3x3 conv then runs on the fused HIP kernel (FasterViT-1/2/4: 80 / 96 / 196 / 392 channels
        # would otherwise fall back to MIOpen + glue passes; a 196-channel fp16 pixel is not even 16-byte aligned).  Pad channels
        # stay exactly zero through bias (0), ReLU / GELU (f(0) = 0), residual adds and LayerNorm2d (zero weight / bias there).
        self.pad_channels = True
        # weight terms of the Downsample.reduction convs (FV:435): 2 = hi + lo (r04, opt-in).  These three strided, bias-free convs feed their
        # rounding straight into the next stage; the weight part of it is systematic (the same for every pixel of every image) and makes up
        # 2.4e-4 / 1.7e-4 / 2.1e-4 of FasterViT-0's 4.2e-4 conv-side logits error (per-layer replay on the fp32 oracle).  Measured (A/B x 2 in
        # one box, scripts/r04_calls/call5.sh): logits max-abs 7.5e-4 -> 4.7e-4 (f16), 5.0e-4 -> 3.0e-4 (f16x2), 7.9e-4 -> 6.9e-4 (bf16x2) for
        # 81.0k -> 77.7k images/s (twice the K steps of 3 of the 15 convs).  Default 1 = single rounding: the plan that is timed.
        self.down_weight_terms = int(os.environ.get("FVIT_DOWN_WEIGHT_TERMS", "1"))
        # 2 = two-term weights in EVERY 3x3 conv that runs on the implicit-GEMM kernel (the stem's second conv, the ConvBlock convs, the downsamples;
        # the halo / band / fused-stem kernels take single-term weights, so those shapes fall back to the implicit GEMM): with the x3 HAT modes the
        # "precise deploy" configuration -- 16-bit maps, everything else to ~22 bits
        self.conv_weight_terms = int(os.environ.get("FVIT_CONV_WEIGHT_TERMS", "1"))
        # two-term / fp32 streams + two-term weights everywhere (module docstring): the ABSOLUTE-1e-3 plan of FasterViT-4 / any-res
        self.precise = os.environ.get("FVIT_PRECISE_DEPLOY", "0") == "1"
        # r06: 3x3 convs contract over the REAL input channels only (dense K; include/fvit_hip.h): 29 / 56 K steps instead of 36 / 63 on FasterViT-4's
        # 196- / 392-channel maps (stored as 256 / 448).  Same products in the same order per tap; "0" = the classic [Cout][3][3][Cin padded] matrix
        self.dense_k = os.environ.get("FVIT_CONV_DENSE_K", "1") != "0"
        self.fused_stem = os.environ.get("FVIT_NO_FUSED_STEM", "0") != "1"   # both PatchEmbed convs in one kernel when in_dim == dim == 64 (the 112x112x64 map never reaches HBM)
        # the level-glue fusions of the 16-bit plan (module docstring).  Each is taken only where the map is unpadded (c_valid == C) and
        # its kernel covers the shape; the standalone passes remain everywhere else.  Keys of fuse_conv_ln2d: the level's channel count.
        self.fuse_conv_ln2d = {64: os.environ.get("FVIT_FUSE_CONV64_LN2D", "1") != "0", 128: os.environ.get("FVIT_FUSE_CONV128_LN2D", "1") != "0"}
        self.fuse_reverse_ln2d = os.environ.get("FVIT_FUSE_REVERSE_LN2D", "1") != "0"
        self.fuse_pool = os.environ.get("FVIT_FUSE_POOL", "1") != "0"

    # ---- folding -------------------------------------------------------------------------
    def _signature(self):
        m = self.model
        sig = []
        for name, p in list(m.named_parameters()) + list(m.named_buffers()):
            if ".blocks." in name and name.startswith(("levels.2.", "levels.3.")):
                continue  # HAT parameters are tracked by hat_runtime
            sig.append((p.data_ptr(), p._version))
        sig.append(("options", self.precise, self.conv_weight_terms, self.down_weight_terms, self.dense_k))   # what _build depends on besides the parameters
        try:   # uint8 images (set_input_norm): a change is picked up by the next eager call, like a weight change
            sig.append(("input_norm", m.input_norm()))
        except RuntimeError:   # no default for this in_chans and none set: a uint8 image raises at its call
            sig.append(("input_norm", None))
        return tuple(sig)

    def _cp(self, c):
        """Channel count of a conv-side map holding c real channels."""
        return c if (c % 64 == 0 or c <= 3 or not (self.pad_channels and self.use_hip_conv)) else (c + 63) // 64 * 64

    def _padv(self, v, n):
        """1-D parameter zero-padded to n entries."""
        if v is None or v.numel() == n:
            return v
        out = torch.zeros(n, dtype=v.dtype, device=v.device)
        out[:v.numel()] = v
        return out

    def _cw(self, w, terms: int = 1) -> ConvWeight:
        """``ConvWeight`` of a folded fp32 weight: the channels_last 16-bit tensor for F.conv2d, -- when the fused implicit-GEMM kernel supports
        the shape (3x3, Cin and Cout multiples of 64) -- its [Cout][3][3][Cin] matrix view, and for 128 -> 128 channels the fragment-order
        stream of the row-band kernel.  Both channel counts are zero-padded to the map layout (``_cp``)."""
        co0, ci0 = w.shape[:2]
        cop, cip = self._cp(co0), self._cp(ci0)
        if (cop, cip) != (co0, ci0):
            wp = torch.zeros((cop, cip) + tuple(w.shape[2:]), dtype=w.dtype, device=w.device)
            wp[:co0, :ci0] = w
            w = wp
        wcl = w.to(self.dtype).contiguous(memory_format=torch.channels_last)
        co, ci, kh, kw = w.shape
        wk = wband = None
        cv = ci   # channels the kernel contracts over per tap (== ci: the classic [Cout][3][3][Cin] matrix)
        if self.use_hip_conv and kh == 3 and kw == 3 and ci % 64 == 0 and co % 64 == 0:
            wk = wcl.permute(0, 2, 3, 1).contiguous()
            lo = (w - wcl.float()).to(self.dtype).permute(0, 2, 3, 1).contiguous() if terms == 2 else None
            cv8 = (ci0 + 7) // 8 * 8
            if self.dense_k and cv8 < ci:
                # r06: the pad channels of the INPUT map leave the contraction (dense K, include/fvit_hip.h): [Cout][terms][kd], column t * cv + c
                cv, kd = cv8, (9 * cv8 + 63) // 64 * 64

                def dense(m):   # m: (co, 3, 3, ci)
                    d = torch.zeros((co, kd), dtype=m.dtype, device=m.device)
                    d[:, :9 * cv] = m[..., :cv].reshape(co, 9 * cv)
                    return d
                # (the classic matrix next to the dense one: the patch form of the kernel, which the driver chooses per call from the map size, takes it)
                classic = wk.reshape(co, -1) if lo is None else torch.cat([wk.reshape(co, -1), lo.reshape(co, -1)], dim=1).contiguous()
                wk = dense(wk) if lo is None else torch.cat([dense(wk), dense(lo)], dim=1).contiguous()
                return ConvWeight(wcl, wk, None, terms, cv, classic)
            if terms == 2:   # [Cout][hi (3,3,Cin) | lo (3,3,Cin)]
                wk = torch.cat([wk.reshape(co, -1), lo.reshape(co, -1)], dim=1).contiguous()
                return ConvWeight(wcl, wk, None, 2, cv, None)
            if (co, ci) == (128, 128):   # the fragment-order image the row-band kernel streams (level 1 of FasterViT-0)
                wband = frag_pack_conv128(wk.reshape(128, 1152))
        return ConvWeight(wcl, wk, wband, 1, cv, None)

    # ---- conv launches (both plans) -------------------------------------------------------
    def _zero_page(self, device):
        """Pointer to the zero page the conv kernels read for taps outside the image: created lazily, per device (``_hat_prepared`` asks for it)."""
        if self.zeros is None or self.zeros.device != device:
            self.zeros = torch.zeros(256, dtype=self.dtype, device=device)
        return self.zeros.data_ptr()

    def _launch_conv(self, x, w: ConvWeight, bias, stride, act, x_lo=None, res=None, res_lo=None, out=None, out_lo=None, out_f32=None, px=False,
                     ln: Optional["DownW"] = None):
        """One ``fvit_conv3x3`` launch on the channels_last map x: the driver picks the kernel from the shape and the images of ``w``.  ``ln``: a
        Downsample whose LayerNorm2d the conv should apply in its epilogue -- the driver is asked for its route first, a route without that epilogue
        runs the plain conv.  Returns whether the LayerNorm2d was applied."""
        B, Ci, Hi, Wi = x.shape
        lib, wts = _lib.lib(), w.images()
        ptr = _lib.ptr
        call = _lib.FvitConvCall(x.data_ptr(), ptr(x_lo), ptr(bias), ptr(res), ptr(res_lo), ptr(out), ptr(out_lo), ptr(out_f32), None, None,
                                 self._zero_page(x.device), 0.0, B, Hi, Wi, Ci, w.wk.shape[0], stride, act, int(px))
        if ln is not None:
            call.ln_w, call.ln_b, call.ln_eps = ln.ln_w.data_ptr(), ln.ln_b.data_ptr(), ln.eps
            if not lib.fvit_conv3x3_route_name(lib.fvit_conv3x3_route(self.code, wts, call)).endswith(b"<ln>"):
                call.ln_w = call.ln_b = ln = None
        _lib.check(lib.fvit_conv3x3(self.code, wts, call, _lib.stream_ptr(self.dev)), "fvit_conv3x3")
        return ln is not None

    def _conv(self, x, w: ConvWeight, bias, stride, act, residual=None):
        """act(conv3x3(x, w) + bias) (+ residual): one fused HIP kernel when supported, else MIOpen conv + glue passes."""
        B, Ci, Hi, Wi = x.shape
        if w.wk is not None and x.is_contiguous(memory_format=torch.channels_last):
            out = residual if residual is not None else torch.empty((B, w.wk.shape[0], (Hi - 1) // stride + 1, (Wi - 1) // stride + 1), dtype=self.dtype,
                                                                    device=x.device, memory_format=torch.channels_last)
            self._launch_conv(x, w, bias, stride, act, res=residual, out=out)
            return out
        y = F.conv2d(x, w.wcl, None, stride, 1)
        if residual is not None:
            return self._bias_residual(residual, y, bias)
        return self._bias_act(y, bias, act) if bias is not None else y

    @torch.no_grad()
    def _build(self):
        m = self.model
        t = {}
        pe = m.patch_embed.conv_down
        w0, b0 = _fold(pe[0], pe[1])
        w1, b1 = _fold(pe[3], pe[4])
        ct = 2 if (self.conv_weight_terms == 2 or self.precise) else 1
        t["stem"] = StemW(self._cw(w0), self._padv(b0, self._cp(b0.numel())).contiguous(), self._cw(w1, terms=ct),
                          self._padv(b1, self._cp(b1.numel())).contiguous())
        t["stem_k"] = t["stem_k_lo"] = None
        # precise plan with a non-standard stem (in_dim != 64 or in_chans != 3): the first conv runs as an fp32 PyTorch-ROCm conv (channels padded)
        co0 = self._cp(w0.shape[0])
        w0p = torch.zeros((co0,) + tuple(w0.shape[1:]), dtype=torch.float32, device=w0.device)
        w0p[:w0.shape[0]] = w0
        t["stem0_f32"] = (w0p.contiguous(memory_format=torch.channels_last), self._padv(b0, co0).contiguous(), tuple(pe[0].stride))
        if self.use_hip_conv and tuple(w0.shape) == (64, 3, 3, 3) and pe[0].stride == (2, 2):
            wk = torch.zeros(64, 32, device=w0.device, dtype=torch.float32)
            wk[:, :27] = w0.permute(0, 2, 3, 1).reshape(64, 27)       # k = ky*9 + kx*3 + c
            t["stem_k"] = wk.to(self.dtype).contiguous()
            t["stem_k_lo"] = (wk - t["stem_k"].float()).to(self.dtype).contiguous()   # second term of the K = 27 weights (precise plan)
        t["levels"] = []
        for lvl in m.levels:
            e = {}
            if not lvl.transformer_block:
                blocks = []
                for blk in lvl.blocks:
                    wa, ba = _fold(blk.conv1, blk.norm1)
                    wb, bb = _fold(blk.conv2, blk.norm2, blk.gamma if blk.layer_scale else None)
                    cpd = self._cp(ba.numel())
                    blocks.append(BlockW(self._cw(wa, terms=ct), self._padv(ba, cpd).contiguous(), self._cw(wb, terms=ct), self._padv(bb, cpd).contiguous()))
                e["blocks"] = blocks
            elif getattr(lvl, "do_gt", False):
                tk = lvl.global_tokenizer
                e["tok"] = TokW(self._cw(tk.pos_embed.weight.float()).wcl, tk.pos_embed.bias.to(self.dtype).contiguous(),
                                tk.to_global_feature.pool.kernel_size, tk.to_global_feature.pool.stride, tk.window_size)
            if lvl.downsample is not None:
                ds = lvl.downsample
                cin = ds.norm.weight.numel()
                e["down"] = DownW(self._padv(ds.norm.weight.float(), self._cp(cin)).contiguous(),
                                  self._padv(ds.norm.bias.float(), self._cp(cin)).contiguous(), float(ds.norm.eps),
                                  self._cw(ds.reduction[0].weight.float(), terms=2 if (self.down_weight_terms == 2 or ct == 2) else 1), cin)
            t["levels"].append(e)
        self._build_head(t)
        self.t = t

    def _build_head(self, t):
        """``t["head"]``: final norm + pool + head as one fp32 Linear (+ the LayerNorm2d parameters with layer_norm_last)."""
        m = self.model
        if isinstance(m.head, torch.nn.Linear):
            hw = m.head.weight.float()
            hb = m.head.bias.float() if m.head.bias is not None else torch.zeros(hw.shape[0], device=hw.device)
        else:   # num_classes = 0: nn.Identity head, the pooled (normalised) features are the output (FV:927)
            nf = m.norm.weight.numel()
            hw, hb = torch.eye(nf, device=m.norm.weight.device), torch.zeros(nf, device=m.norm.weight.device)
        if isinstance(m.norm, torch.nn.BatchNorm2d):
            s, sh = _bn_scale_shift(m.norm)
            t["head"] = HeadW((hw * s.view(1, -1)).contiguous(), (hb + hw @ sh).contiguous(), None)
        else:  # layer_norm_last: LayerNorm2d kernel, then pool + head
            t["head"] = HeadW(hw.contiguous(), hb.contiguous(),
                              (m.norm.weight.float().contiguous(), m.norm.bias.float().contiguous(), float(m.norm.eps)))

    # ---- kernels -------------------------------------------------------------------------
    def _bias_act(self, x, bias, act):
        B, C, H, W = x.shape
        assert x.is_contiguous(memory_format=torch.channels_last) and x.dtype == self.dtype
        _lib.check(_lib.lib().fvit_bias_act_cl(self.code, x.data_ptr(), bias.data_ptr(), B * H * W, C, act, _lib.stream_ptr(self.dev)),
                   "fvit_bias_act_cl")
        return x

    def _bias_residual(self, x, y, bias):
        B, C, H, W = x.shape
        assert x.is_contiguous(memory_format=torch.channels_last) and y.is_contiguous(memory_format=torch.channels_last)
        _lib.check(_lib.lib().fvit_bias_residual_cl(self.code, x.data_ptr(), y.data_ptr(), bias.data_ptr(), B * H * W, C,
                                                    _lib.stream_ptr(self.dev)), "fvit_bias_residual_cl")
        return x

    def _pool_head(self, x, hw, hb):
        """AdaptiveAvgPool2d(1) + flatten + head (FV:955-960; final BatchNorm folded into hw / hb) on a channels_last map: fvit_global_avgpool_cl +
        fvit_head_logits (exact-fp32 MFMA) -- no library kernel in the captured graph.  Maps that are not dense channels_last (a strided stage output)
        or whose channel count is not a multiple of 16 take the PyTorch ops."""
        B, C, H, W = x.shape
        if x.dtype in hat_runtime._DT and x.permute(0, 2, 3, 1).is_contiguous() and C % 16 == 0 and hw.shape[1] == C and hw.is_contiguous():
            feat = torch.empty((B, C), dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().fvit_global_avgpool_cl(hat_runtime._DT[x.dtype], x.data_ptr(), feat.data_ptr(), B, H * W, C, _lib.stream_ptr(self.dev)),
                       "fvit_global_avgpool_cl")
            return self._head_logits(feat, hw, hb)
        return F.linear(x.float().mean(dim=(2, 3)), hw, hb)

    def _head_logits(self, feat, hw, hb):
        """The head on (B, C) fp32 pooled features: fvit_head_logits (exact-fp32 MFMA)."""
        B, C = feat.shape
        out = torch.empty((B, hw.shape[0]), dtype=torch.float32, device=feat.device)
        _lib.check(_lib.lib().fvit_head_logits(feat.data_ptr(), hw.data_ptr(), hb.data_ptr(), out.data_ptr(), B, hw.shape[0], C, _lib.stream_ptr(self.dev)),
                   "fvit_head_logits")
        return out

    def _ln2d(self, x, w, b, eps, c_valid=None):
        """LayerNorm2d over the first c_valid (default: all) channels of a channels_last map; pad channels stay zero."""
        B, C, H, W = x.shape
        cv = C if c_valid is None else c_valid
        if C % 8 or not x.is_contiguous(memory_format=torch.channels_last):
            y = torch.zeros_like(x, dtype=torch.float32)
            y[:, :cv] = F.layer_norm(x[:, :cv].permute(0, 2, 3, 1).float(), (cv,), w[:cv], b[:cv], eps).permute(0, 3, 1, 2)
            return y.to(self.dtype).contiguous(memory_format=torch.channels_last)
        out = torch.empty_like(x)
        _lib.check(_lib.lib().fvit_layernorm2d_cl(self.code, x.data_ptr(), out.data_ptr(), w.data_ptr(), b.data_ptr(), eps,
                                                  B * H * W, C, cv, _lib.stream_ptr(self.dev)), "fvit_layernorm2d_cl")
        return out

    # ---- forward -------------------------------------------------------------------------
    @torch.no_grad()
    def _refresh(self):
        sig = self._signature()
        if sig != self.sig:
            with torch.autocast(device_type="cuda", enabled=False):
                self._build()
            self.sig = sig

    def _enter(self, x):
        """Per-call checks: GPU input on the model's device; launches below go to torch's current stream on that device."""
        if not x.is_cuda:
            raise RuntimeError("deploy plan: the input must be on a HIP device (no CPU fallback)")
        p0 = next(self.model.parameters())
        if p0.device != x.device:
            raise RuntimeError(f"deploy plan: model parameters are on {p0.device} but the input is on {x.device}")
        self.dev = x.device

    def _hat_prepared(self, device):
        return self.zeros is not None and self.zeros.device == device and all(
            hat_runtime.is_prepared(lvl, device) for lvl in self.model.levels if lvl.transformer_block and len(lvl.blocks))

    def forward_single(self, x):
        """One shard on the caller's stream and current workspace slot (no sharding)."""
        self._enter(x)
        with torch.cuda.device(x.device):
            self._refresh()
            return self._forward_one(x)

    def forward(self, x):
        self._enter(x)
        with torch.cuda.device(x.device):
            self._refresh()
            return self._forward_sharded(x)

    def _forward_sharded(self, x):
        n = self.streams
        if n <= 1 or x.shape[0] < 2 * n:
            with hat_runtime.workspace_slot(self.slot_base):
                return self._forward_one(x)
        # the batch as n independent shards on n HIP streams (fork / join with events; capturable in a hipGraph): every kernel
        # of this pipeline runs its HBM-bound prologue / epilogue and its MFMA phase in lockstep across workgroups, so two
        # half-size pipelines interleave better than one full-size one
        # slot_base (r06): first workspace slot of this plan; two plans whose forwards are in flight at the same time (inference.PipelinedInference:
        # consecutive steps on alternating streams) must not share the per-(geometry, slot) stage workspaces
        sb, sizes, warm = self.slot_base, self.shard_sizes, self._warm_geometries
        parts = x.split(list(sizes), dim=0) if sizes and sum(sizes) == x.shape[0] and len(sizes) == n else x.chunk(n, dim=0)
        outs = [None] * n
        # weight packing (hat_runtime._prepare) and the zero page are created lazily by the first shard that needs them, on ITS
        # stream; the other streams forked before that work was enqueued and would read half-written packed weights.  Until
        # everything is packed for this device, run the shards one after the other on the caller's stream (first call, or the
        # first call after a weight update).
        # The per-geometry index tables (an H2D copy) and workspaces are created lazily by the first stage call too: the forked form
        # is allowed only for a (device, shard sizes, image size, operand mode) that has completed one serial pass.
        ops = tuple(getattr(lvl, "hat_operand_dtype", "f16") for lvl in self.model.levels if lvl.transformer_block)
        wkey = (str(x.device), tuple(p.shape[0] for p in parts), tuple(x.shape[1:]), ops, self.join_from, sb)
        serial = self.serialize_shards or not self._hat_prepared(x.device) or wkey not in warm
        # join_from = L (r04, ``plan.join_from``; None = off): the shards run levels [0, L) on their own streams, JOIN, and levels
        # [L, end) + head run once on the whole batch on the caller's stream.  The last stage of FasterViT-0 (one 49-token window per
        # image, 512 channels) is 86-workgroup launches per shard that cannot fill the chip; joined it is 196 / 256 workgroups.
        jf = self.join_from if (self.join_from is not None and 0 < self.join_from < len(self.model.levels)) else None
        front = (lambda xi: self._forward_one(xi, 0, jf)) if jf is not None else self._forward_one
        def _cat(xs):   # shards of the precise plan hand on (hi, lo, f32) tuples
            if isinstance(xs[0], tuple):
                return tuple(None if xs[0][k] is None else torch.cat([x_[k] for x_ in xs], dim=0) for k in range(3))
            return torch.cat(xs, dim=0)
        back = (lambda xs: self._forward_one(_cat(xs), jf, None)) if jf is not None else (lambda xs: torch.cat(xs, dim=0))
        if serial:
            # also the measurement aid of bench.py's HIP-event pass: the same shard-sized launches, one after the other on the
            # caller's stream, so that a kernel's event-pair duration is its own and not shared with the other shards' kernels
            for i in range(n):
                with hat_runtime.workspace_slot(sb + i):
                    outs[i] = front(parts[i])
            with hat_runtime.workspace_slot(sb):
                y = back(outs)
            if not torch.cuda.is_current_stream_capturing():
                warm.add(wkey)
            return y
        if self.side is None or len(self.side) != n - 1 or self.side[0].device != x.device:
            self.side = [torch.cuda.Stream(device=x.device) for _ in range(n - 1)]
        main = torch.cuda.current_stream(x.device)
        for i, s in enumerate(self.side):
            s.wait_stream(main)
            with torch.cuda.stream(s), hat_runtime.workspace_slot(sb + i + 1):
                outs[i + 1] = front(parts[i + 1])
        with hat_runtime.workspace_slot(sb):
            outs[0] = front(parts[0])
        for s in self.side:
            main.wait_stream(s)   # join: everything the caller enqueues next (the cat below, its own later work) is ordered after the shards
        with hat_runtime.workspace_slot(sb):
            return back(outs)

    def shard_runner(self, x, n=None):
        """Free-running stream shards for throughput serving: see ``ShardRunner``."""
        return ShardRunner(self, x, n or max(self.streams, 1))

    # ---- the precise plan: two-term / fp32 streams (module docstring) ---------------------------------------------------
    def _conv_px(self, x, x_lo, w: ConvWeight, bias, stride, act, res=None, res_lo=None, want="planes"):
        """conv3x3_kernel<.., PX>: x (+ x_lo) -> act(conv + bias) (+ res + res_lo).  ``want``: 'planes' -> (hi, lo) 16-bit planes (in place over the
        residual planes when given), 'single' -> (hi, None), 'f32' -> one fp32 channels_last map."""
        if w.wk is None or not x.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("precise deploy plan: this conv shape has no implicit-GEMM kernel (channel counts must pad to multiples of 64)")
        B, Ci, Hi, Wi = x.shape
        shape = (B, w.wk.shape[0], (Hi - 1) // stride + 1, (Wi - 1) // stride + 1)
        hi = lo = f32 = None
        if want == "f32":
            f32 = torch.empty(shape, dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        else:
            hi = res if res is not None else torch.empty(shape, dtype=self.dtype, device=x.device, memory_format=torch.channels_last)
            if want == "planes":
                lo = res_lo if res_lo is not None else torch.empty_like(hi)
        self._launch_conv(x, w, bias, stride, act, x_lo=x_lo, res=res, res_lo=res_lo, out=hi, out_lo=lo, out_f32=f32, px=True)
        return f32 if want == "f32" else (hi, lo)

    def _ln2d_px(self, x, x_lo, x_f32, w, b, eps, c_valid):
        """LayerNorm2d of a two-term (x, x_lo) or fp32 (x_f32) channels_last map -> two 16-bit planes."""
        src = x_f32 if x_f32 is not None else x
        B, C, H, W = src.shape
        if C % 8 or not src.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("precise deploy plan: LayerNorm2d needs a channels_last map with C % 8 == 0")
        hi = torch.empty((B, C, H, W), dtype=self.dtype, device=src.device, memory_format=torch.channels_last)
        lo = torch.empty_like(hi)
        _lib.check(_lib.lib().fvit_layernorm2d_px(self.code, x.data_ptr() if x is not None else None, x_lo.data_ptr() if x_lo is not None else None,
                                                  x_f32.data_ptr() if x_f32 is not None else None, hi.data_ptr(), lo.data_ptr(), w.data_ptr(),
                                                  b.data_ptr(), eps, B * H * W, C, c_valid, _lib.stream_ptr(self.dev)), "fvit_layernorm2d_px")
        return hi, lo

    # ---- the level walk ----------------------------------------------------------------------------------------------------
    # The map handed from step to step is one 16-bit channels_last tensor in the 16-bit plan and the tuple ``(hi, lo, f32)`` in the precise plan: two
    # 16-bit planes (value = hi + lo, f32 = None), or -- in front of / behind a transformer level -- one fp32 map (hi = lo = None).
    def _forward_one(self, x, lv_from=0, lv_to=None):
        """Levels [lv_from, lv_to) of the plan; the stem runs in front of level 0, final norm + pool + head after the last level
        (lv_to = None).  A partial call (stream shards + join) returns the map that the next level takes: the (channels_last, 16-bit) tensor, or
        the precise plan's ``(hi, lo, f32)``, whose planes the caller concatenates."""
        levels = self.model.levels
        with torch.autocast(device_type="cuda", enabled=False):
            if lv_from == 0:
                x = self._stem(x)
            for li, (lvl, e) in enumerate(zip(levels, self.t["levels"])):
                if li < lv_from or (lv_to is not None and li >= lv_to):
                    continue
                # normed: the level's kernels already applied the Downsample's LayerNorm2d; pooled: x is the (B, C) pooled features, not a map
                normed = pooled = False
                if "blocks" in e:
                    x, normed = self._conv_level(x, e["blocks"], e.get("down"))
                elif self._pool_tail(lvl, x, last=li + 1 == len(levels) and lv_to is None and "down" not in e):
                    x, pooled = self._hat_level_pooled(lvl, x), True
                else:
                    x, normed = self._hat_level(lvl, x, padded_out="down" in e, down=e.get("down"))
                if "down" in e:
                    x = self._downsample(x, e["down"], f32_out=li + 1 < len(levels) and levels[li + 1].transformer_block, normed=normed)
            if lv_to is not None:
                return x
            return self._head_logits(x, *self.t["head"][:2]) if pooled else self._head(x)

    def _stem(self, x):
        """PatchEmbed: conv + BN + ReLU twice, from the caller's image to the map level 0 takes."""
        t, st = self.t, self.t["stem"]
        u8 = x.dtype == torch.uint8
        if u8 and not (t["stem_k"] is not None and x.shape[1] == 3):
            x, u8 = self.model.normalize_input(x), False   # a stem without a uint8 kernel: one normalisation pass, then the float route
        # a uint8 image on the K = 27 kernels: normalised at their loads with the model's constants, read from host memory at each launch
        norm = self.model.input_norm_array() if u8 else None
        k27 = t["stem_k"] is not None and x.shape[1] == 3 and (u8 or x.dtype in hat_runtime._DT)   # the reference's 3 -> 64 first conv: the K = 27 kernels
        if self.precise:
            if not k27:
                # a stem other than the reference's 3 -> 64 (in_dim / in_chans kwargs): its first conv as an fp32 PyTorch-ROCm conv
                wf, bf, st0 = t["stem0_f32"]
                y = torch.relu(F.conv2d(x.float(), wf, bf, st0, 1)).to(self.dtype).contiguous(memory_format=torch.channels_last)
            else:
                B, _, Hi, Wi = x.shape
                y = torch.empty((B, 64, (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1), dtype=self.dtype, device=x.device, memory_format=torch.channels_last)
                view = hat_runtime._image_view(x)
                args = (self.code, view, t["stem_k"].data_ptr(), t["stem_k_lo"].data_ptr(), st.bias0.data_ptr(), y.data_ptr(), B, Hi, Wi, _lib.stream_ptr(self.dev))
                if u8:
                    _lib.check(_lib.lib().fvit_stem_conv3x3s2_px_u8(*args, norm), "fvit_stem_conv3x3s2_px_u8")
                else:
                    _lib.check(_lib.lib().fvit_stem_conv3x3s2_px(*args), "fvit_stem_conv3x3s2_px")
            return (*self._conv_px(y, None, st.conv1, st.bias1, 2, 1), None)
        wk1 = st.conv1.wk
        if self.fused_stem and k27 and wk1 is not None and st.conv1.terms == 1 and tuple(wk1.shape) == (64, 3, 3, 64):
            B, _, Hi, Wi = x.shape
            H1, W1 = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
            y = torch.empty((B, 64, (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1), dtype=self.dtype, device=x.device,
                            memory_format=torch.channels_last)
            view = hat_runtime._image_view(x)
            args = (self.code, view, t["stem_k"].data_ptr(), st.bias0.data_ptr(), wk1.data_ptr(), st.bias1.data_ptr(), y.data_ptr(), B, Hi, Wi, _lib.stream_ptr(self.dev))
            if u8:
                _lib.check(_lib.lib().fvit_stem_fused_u8(*args, norm), "fvit_stem_fused_u8")
            else:
                _lib.check(_lib.lib().fvit_stem_fused(*args), "fvit_stem_fused")
            return y
        if k27:
            B, _, Hi, Wi = x.shape   # fused stem kernel reads the caller's image in place (any strides, fp32/16-bit)
            y = torch.empty((B, 64, (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1), dtype=self.dtype, device=x.device,
                            memory_format=torch.channels_last)
            view = hat_runtime._image_view(x)
            args = (self.code, view, t["stem_k"].data_ptr(), st.bias0.data_ptr(), y.data_ptr(), B, Hi, Wi, _lib.stream_ptr(self.dev))
            if u8:
                _lib.check(_lib.lib().fvit_stem_conv3x3s2_u8(*args, norm), "fvit_stem_conv3x3s2_u8")
            else:
                _lib.check(_lib.lib().fvit_stem_conv3x3s2(*args), "fvit_stem_conv3x3s2")
            return self._conv(y, st.conv1, st.bias1, 2, 1)
        x = x.to(self.dtype).contiguous(memory_format=torch.channels_last)
        return self._conv(self._conv(x, st.conv0, st.bias0, 2, 1), st.conv1, st.bias1, 2, 1)

    def _conv_level(self, x, blocks, down: Optional["DownW"] = None):
        """The ConvBlocks of a level, in place on the stream -> (map, normed).  ``down``: the following Downsample; where the plan wants it (16-bit plan,
        ``fuse_conv_ln2d``, an unpadded map) and the last conv's kernel can (``_launch_conv``), that conv applies the Downsample's LayerNorm2d in its
        epilogue and ``normed`` is True."""
        if not self.precise:
            normed = False
            for i, b in enumerate(blocks):
                y = self._conv(x, b.conv1, b.bias1, 1, 2)
                if (down is not None and i + 1 == len(blocks) and self.use_hip_conv and self.fuse_conv_ln2d.get(y.shape[1], False) and down.cin == y.shape[1]
                        and b.conv2.wk is not None and y.is_contiguous(memory_format=torch.channels_last)):
                    normed = self._launch_conv(y, b.conv2, b.bias2, 1, 0, res=x, out=x, ln=down)
                else:
                    x = self._conv(y, b.conv2, b.bias2, 1, 0, residual=x)
            return x, normed
        hi, lo, f32 = x
        if hi is None:   # a conv level behind a transformer level (no reference entrypoint does this): split the fp32 map
            hi = f32.to(self.dtype)
            lo = (f32 - hi.float()).to(self.dtype)
        for b in blocks:
            y, _ = self._conv_px(hi, None, b.conv1, b.bias1, 1, 2, want="single")              # conv1 + BN + GELU: an operand, one term
            hi, lo = self._conv_px(y, None, b.conv2, b.bias2, 1, 0, res=hi, res_lo=lo)         # conv2 + BN (+ gamma) + residual, in place on the stream
        return (hi, lo, None), False

    def _pool_tail(self, lvl, x, last):
        """The last level hands its token rows straight to the pool (``hat_runtime.stage_forward(..., pool_out=)``): 16-bit plan, the final norm folded
        into the head (BatchNorm), one window per image, no carrier tokens, unpadded channels."""
        return (last and self.fuse_pool and not self.precise and self.t["head"].ln is None and torch.is_tensor(x) and len(lvl.blocks) > 0
                and x.shape[1] == lvl.blocks[0].attn.qkv.in_features and x.shape[1] % 16 == 0 and self.t["head"].w.shape[1] == x.shape[1]
                and hat_runtime.pool_tail_supported(lvl, x))

    def _hat_level_pooled(self, lvl, x):
        """The last transformer level -> (B, C) fp32 pooled features (``_pool_tail``)."""
        feat = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        return hat_runtime.stage_forward(lvl, x, pool_out=feat)

    def _hat_level(self, lvl, x, padded_out, tokenizer=None, down: Optional["DownW"] = None):
        """A transformer level (``hat_runtime.stage_forward``) on a 16-bit map, or -- precise plan -- from and to an fp32 map -> (map, normed).
        ``tokenizer``: passed on (the detection backbone's per-call TokenInitializer).  ``down``: the following Downsample; on an unpadded 16-bit map
        the stage's window_reverse applies its LayerNorm2d (``normed`` True)."""
        if self.precise:
            hi, lo, x = x
            if x is None:   # a transformer level behind a conv level without a Downsample in between (no reference entrypoint does this)
                x = hi.float() + lo.float()
        # the HIP stage reads / writes its maps through strided views: the padded map's first C channels in, and
        # -- when a Downsample follows -- the first C channels of a zero-initialised padded map out
        creal = lvl.blocks[0].attn.qkv.in_features if len(lvl.blocks) else x.shape[1]
        xin = x[:, :creal] if x.shape[1] != creal else x
        cpo = self._cp(creal) if padded_out else creal
        # (an explicit channels_last output: empty_like of the strided channel slice `xin` would be NCHW-contiguous -- uncoalesced
        # window_reverse stores and no dense [B][HW][C] image for the pool kernel)
        xo = torch.empty((x.shape[0], cpo, x.shape[2], x.shape[3]), dtype=torch.float32 if self.precise else self.dtype, device=x.device,
                         memory_format=torch.channels_last)
        if cpo != creal:
            xo[:, creal:] = 0   # only the pad channels need initialising; the stage writes the first creal
            hat_runtime.stage_forward(lvl, xin, tokenizer=tokenizer, out=xo[:, :creal])  # TokenInitializer: fvit_token_init in both modes
            return ((None, None, xo) if self.precise else xo), False
        if (down is not None and self.fuse_reverse_ln2d and not self.precise and down.cin == creal and len(lvl.blocks)
                and hat_runtime.ln2d_tail_supported(xin, xo)):
            return hat_runtime.stage_forward(lvl, xin, tokenizer=tokenizer, out=xo, ln2d=(down.ln_w, down.ln_b, down.eps)), True
        xo = hat_runtime.stage_forward(lvl, xin, tokenizer=tokenizer, out=xo)
        return ((None, None, xo) if self.precise else xo), False

    def _downsample(self, x, d: DownW, f32_out, normed=False):
        """Downsample: LayerNorm2d + strided bias-free conv.  ``f32_out``: a transformer level follows, which the precise plan feeds an fp32 map.
        ``normed``: the level's last kernel applied the LayerNorm2d already."""
        if not self.precise:
            return self._conv(x if normed else self._ln2d(x, d.ln_w, d.ln_b, d.eps, d.cin), d.conv, None, 2, 0)
        hi, lo, f32 = x
        if f32 is not None and not f32.is_contiguous(memory_format=torch.channels_last):
            f32 = f32.contiguous(memory_format=torch.channels_last)
        nh, nl = self._ln2d_px(hi, lo, f32, d.ln_w, d.ln_b, d.eps, d.cin)
        if f32_out:
            return None, None, self._conv_px(nh, nl, d.conv, None, 2, 0, want="f32")
        return (*self._conv_px(nh, nl, d.conv, None, 2, 0), None)

    def _head(self, x):
        """Final norm + AdaptiveAvgPool2d(1) + head -> fp32 logits."""
        hw, hb, ln = self.t["head"]
        if not self.precise:
            return self._pool_head(x if ln is None else self._ln2d(x, *ln), hw, hb)
        hi, lo, f32 = x
        if f32 is None:
            f32 = hi.float() + lo.float()
        if ln is not None:
            nh, nl = self._ln2d_px(None, None, f32.contiguous(memory_format=torch.channels_last), *ln, f32.shape[1])
            f32 = nh.float() + nl.float()
        return self._pool_head(f32, hw, hb)


class LevelMap(NamedTuple):
    """The map ``BackboneDeployPlan`` hands from level to level: a 16-bit channels_last tensor (channels padded to ``_cp``) whose top-left H x W
    pixels are the level's map.  Behind a padded conv level the tensor is the whole window-padded Hp x Wp map (the ConvBlocks' values in the pad,
    which only they read); everywhere else it is dense (``x.shape[2:] == (H, W)``)."""
    x: torch.Tensor
    H: int
    W: int

    @property
    def dense(self) -> bool:
        return self.x.shape[2] == self.H and self.x.shape[3] == self.W


TapW = NamedTuple("TapW", [("scale", torch.Tensor), ("shift", torch.Tensor), ("channels", int)])   # t["taps"][i]: norm{i} folded (fp32), real channels of level i


class BackboneDeployPlan(DeployPlan):
    """The deploy plan of ``models.backbone.FasterViTBackbone``: ``DeployPlan``'s folded weights, conv / LayerNorm2d / stem launches
    and transformer-level call, under the detection variant's level walk -- every level window-padded and cropped (DET:687-704), the ``out_indices``
    levels' pre-downsample maps returned through ``fvit_feature_tap`` with ``norm{i}`` folded.  Per level:

      conv level         H x W not a window multiple: ``fvit_map_pad_cl`` copies the dense map into a zero-padded Hp x Wp one (one pass), the ConvBlocks
                         run on it in place (the second conv of a block reads the first one's values in the pad, as the reference does); the tap reads
                         the H x W corner through strides and the Downsample's LayerNorm2d reads it through ``fvit_layernorm2d_crop_cl``, so the crop
                         costs no pass.  A window multiple: the classifier's path.
      transformer level  ``hat_runtime.stage_forward`` on the 16-bit map with the per-call tokenizer (it pads and crops itself), the tap, then the dense
                         LayerNorm2d + strided conv.

    ``forward`` returns the tuple of NCHW fp32 maps of ``FasterViTBackbone.forward_features``.  16-bit plan only: the precise plan, two-term conv
    weights and stream shards are refused by name."""

    def __init__(self, model, dtype=torch.float16):
        super().__init__(model, dtype)
        self._check_options()
        for i in model.out_indices:   # a norm{i} without running statistics: refused here, with feature_tap's message
            bn = getattr(model, f"norm{i}")
            hat_runtime._folded_bn(bn, (bn.running_mean if bn.running_mean is not None else next(model.parameters())).device)

    def _check_options(self):
        if self.precise:
            raise NotImplementedError("backbone deploy plan: precise=True is not implemented (there is no two-term feature tap); use the 16-bit plan, "
                                      "or module mode with set_hat_operand_dtype('f16x3')")
        if self.conv_weight_terms != 1 or self.down_weight_terms != 1:
            raise NotImplementedError("backbone deploy plan: two-term conv weights (conv_weight_terms / down_weight_terms = 2) are not implemented")
        if self.streams != 1:
            raise NotImplementedError("backbone deploy plan: streams > 1 (stream shards) is not implemented; detection batches are small")

    def _build_head(self, t):
        """No head: ``t["taps"]`` = the ``out_indices`` levels' ``norm{i}`` folded to scale / shift (``hat_runtime._folded_bn``).  Their tensors are part of
        ``_signature`` (every parameter and buffer outside the HAT blocks), so a change rebuilds them with the conv weights."""
        m = self.model
        dev = next(m.parameters()).device
        t["taps"] = {i: TapW(*hat_runtime._folded_bn(getattr(m, f"norm{i}"), dev), m.num_features[i]) for i in m.out_indices}

    # ---- forward -------------------------------------------------------------------------
    def forward(self, x):
        self._check_options()
        self._enter(x)
        with torch.cuda.device(x.device):
            self._refresh()
            with hat_runtime.workspace_slot(self.slot_base):
                return self._walk(x)

    forward_single = forward

    def _walk(self, x):
        """Stem, then per level: blocks -> tap (``out_indices``) -> Downsample.  ``m`` is the ``LevelMap`` between the steps."""
        levels, taps = self.model.levels, self.t["taps"]
        outs = []
        with torch.autocast(device_type="cuda", enabled=False):
            y = self._stem(x)
            m = LevelMap(y, y.shape[2], y.shape[3])
            for li, (lvl, e) in enumerate(zip(levels, self.t["levels"])):
                if "blocks" in e:
                    m = self._conv_level_padded(m, e["blocks"], lvl.window_size)
                else:
                    m = self._hat_level_dyn(lvl, m, padded_out="down" in e)
                if li in taps:
                    outs.append(self._tap(m, taps[li]))
                if "down" in e:
                    m = self._downsample_crop(m, e["down"])
        return tuple(outs)

    def _conv_level_padded(self, m: LevelMap, blocks, ws: int) -> LevelMap:
        """The ConvBlocks on the window-padded map (DET:687-704), in place; the result keeps the pad around the H x W map."""
        assert m.dense
        B, C, H, W = m.x.shape
        Hp, Wp = H + (ws - H % ws) % ws, W + (ws - W % ws) % ws
        x = m.x
        if (Hp, Wp) != (H, W) and len(blocks):
            x = torch.empty((B, C, Hp, Wp), dtype=self.dtype, device=m.x.device, memory_format=torch.channels_last)
            _lib.check(_lib.lib().fvit_map_pad_cl(self.code, m.x.data_ptr(), x.data_ptr(), B, H, W, Hp, Wp, C, _lib.stream_ptr(self.dev)), "fvit_map_pad_cl")
        return LevelMap(self._conv_level(x, blocks)[0], H, W)

    def _hat_level_dyn(self, lvl, m: LevelMap, padded_out: bool) -> LevelMap:
        """A transformer level with the window grid and TokenInitializer pooling of THIS map size; dense in, dense out."""
        assert m.dense
        tok = None
        if len(lvl.blocks) and lvl.do_gt and lvl.blocks[0].do_sr_hat:
            tok = lambda xp: hat_runtime.token_init_dyn(lvl.global_tokenizer, xp, lvl.window_size)   # noqa: E731
        return LevelMap(self._hat_level(lvl, m.x, padded_out, tokenizer=tok)[0], m.H, m.W)

    def _tap(self, m: LevelMap, tw: TapW) -> torch.Tensor:
        """``norm{i}`` of the H x W corner's real channels -> contiguous NCHW fp32 (fvit_feature_tap reads the crop through strides)."""
        B = m.x.shape[0]
        view = hat_runtime._map_view(m.x[:, :tw.channels, :m.H, :m.W])
        out = torch.empty((B, tw.channels, m.H, m.W), dtype=torch.float32, device=m.x.device)
        _lib.check(_lib.lib().fvit_feature_tap(ctypes.byref(view), B, tw.channels, m.H, m.W, tw.scale.data_ptr(), tw.shift.data_ptr(), out.data_ptr(),
                                               _lib.stream_ptr(self.dev)), "fvit_feature_tap")
        return out

    def _downsample_crop(self, m: LevelMap, d: DownW) -> LevelMap:
        """Downsample of the H x W corner: LayerNorm2d (``fvit_layernorm2d_crop_cl`` on a padded map: the crop costs no pass) + strided conv."""
        if m.dense:
            n = self._ln2d(m.x, d.ln_w, d.ln_b, d.eps, d.cin)
        else:
            B, C, Hp, Wp = m.x.shape
            n = torch.empty((B, C, m.H, m.W), dtype=self.dtype, device=m.x.device, memory_format=torch.channels_last)
            _lib.check(_lib.lib().fvit_layernorm2d_crop_cl(self.code, m.x.data_ptr(), n.data_ptr(), d.ln_w.data_ptr(), d.ln_b.data_ptr(), d.eps,
                                                           B, m.H, m.W, Hp, Wp, C, d.cin, _lib.stream_ptr(self.dev)), "fvit_layernorm2d_crop_cl")
        y = self._conv(n, d.conv, None, 2, 0)
        return LevelMap(y, y.shape[2], y.shape[3])

    # ---- what a captured graph holds by raw pointer ------------------------------------------
    def pinned(self, x_shape, device):
        """Strong references to the per-geometry objects of ``hat_runtime`` (packed weights, tables, workspace of this plan's slot, tokenizer
        weights) that a forward of an input of ``x_shape`` uses, after such a forward has run: ``hat_runtime`` keeps them in a bounded LRU, a captured
        graph holds their addresses.  (The plan owns the folded conv weights, taps and the zero page itself.)"""
        B, _, H, W = x_shape
        for _ in range(2):   # the stem's two stride-2 convs; each Downsample: one more
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        refs = []
        for lvl in self.model.levels:
            if lvl.transformer_block and len(lvl.blocks):
                refs.append(hat_runtime.stage_refs(lvl, device, B, H, W, self.slot_base))
            if lvl.downsample is not None:
                H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return refs


class ShardRunner:
    """Throughput driver for steady-state inference: the batch is split into n shards, each shard's whole forward is captured in its
    OWN hipGraph on its OWN stream, and ``launch()`` enqueues one replay per stream without any fork / join between steps.

    ``DeployPlan.forward`` (fork / join inside one graph) starts all shards of a step together and ends the step when the slowest
    is done, so the shards walk through the network in lockstep: three stems, then three level-0 conv stacks, ..., then three
    carrier-token branches (22 workgroups each) at the same time.  Independent per-stream graphs let consecutive steps of different
    shards overlap: the streams drift apart and an underfilled phase of one shard (carrier branch, stage 3) runs beside a
    chip-filling phase of another (convs).  Images are independent, so there is no data hazard; ``wait()`` joins all streams.
    Results of the LAST launch are in ``outputs()`` (static buffers, as with any graph replay)."""

    def __init__(self, plan, x, n):
        self.plan = plan
        self.n = n = max(1, min(int(n), x.shape[0]))
        self.streams = [torch.cuda.Stream(device=x.device) for _ in range(n)]
        self.inputs = [p.clone() for p in x.chunk(n, dim=0)]
        self.graphs, self.outs = [], []
        torch.cuda.synchronize()
        for i, (st, xi) in enumerate(zip(self.streams, self.inputs)):
            with torch.cuda.stream(st), torch.no_grad(), hat_runtime.workspace_slot(i):
                for _ in range(2):           # warm-up on this stream: packs weights, sizes this slot's workspaces
                    plan.forward_single(xi)
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(g, stream=st), hat_runtime.workspace_slot(i):
                y = plan.forward_single(xi)
            self.graphs.append(g)
            self.outs.append(y)
        torch.cuda.synchronize()

    def set_input(self, x):
        if (x.dtype == torch.uint8) != (self.inputs[0].dtype == torch.uint8):   # a copy_ would turn bytes into unnormalised floats (or back)
            raise RuntimeError(f"ShardRunner: built for {self.inputs[0].dtype} images, set_input got {x.dtype}")
        for dst, src in zip(self.inputs, x.chunk(self.n, dim=0)):
            dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()

    def launch(self):
        for st, g in zip(self.streams, self.graphs):
            with torch.cuda.stream(st):
                g.replay()

    def wait(self):
        for st in self.streams:
            st.synchronize()

    def outputs(self):
        self.wait()
        return torch.cat(self.outs, dim=0)
