"""Multi-scale FasterViT backbone for dense prediction: the detection variant the reference's DINO results use
(``downstream/object_detection/dino/models/dino/fastervit.py`` = DET), same builder, constructor arguments and ``state_dict`` layout, on
the HIP engine of the classifier.

What differs from the classifier (fastervit_amd/models/faster_vit.py) and where it is handled:

* every level returns its PRE-downsample map as well (DET:686-708); ``out_indices`` levels go through ``norm{i}`` (eval BatchNorm2d,
  folded) in one fused HIP pass per level (``fvit_feature_tap``);
* the window grid of a hierarchical stage is taken from the padded input of each call, not from ``sr_ratio`` (``dynamic_grid``): the
  packed weights, gather tables and position tables are cached per geometry in ``fastervit_amd.hat_runtime`` (bounded LRU);
* TokenInitializer (DET:542-592): pool kernel / stride from the padded map of each call, zero pad to a multiple of ct_size, and the raw
  NCHW -> (B, G, C) reshape without the classifier's per-window permute (``fvit_token_init_dyn``);
* position tables (DET:176-203): normalised by (token count) // 2 over an arange(h_g) x arange(w_g) grid -- a rectangular carrier grid
  (``hat_runtime.grid_pos_table``); the carrier attention bias is padded (G > 16) or cropped (G < 16) to G (DET:118-135).

Left out on purpose: DET's ``forward_raw`` applies ``permute(0, 3, 1, 2)`` to an NCHW map (a bug: it scrambles the axes); here
``forward_features`` returns the NCHW maps ``forward`` uses.

Training.  By default the model is inference-only: train mode (with a transformer stage) and gradient requests raise.
``model.enable_hat_backward()`` opts in to fine-tuning it the way DINO does:

* eval mode with grad enabled: every transformer level is ONE autograd node (forward: the fused inference kernels, backward: the kernel sequence
  of ``fastervit_amd.hat_backward`` with the window grid, carrier grid, position tables and padded / cropped carrier bias of THAT call, the
  tokenizer differentiated by ``fvit_token_init_dyn_backward``); the conv levels are PyTorch modules under autograd; every ``norm{i}`` output goes
  through the differentiable tap (``fvit_feature_tap`` / ``fvit_feature_tap_backward``);
* train mode: the transformer levels run the unit-kernel chain with stochastic depth and Dropout (masks sized from the padded grid of the call), the
  conv-side BatchNorms are PyTorch modules, a ``norm{i}`` in training mode runs as ``nn.BatchNorm2d`` on the cropped map (batch statistics), a
  ``norm{i}`` in eval mode (frozen BN) takes the fused tap;
* what the kernels do not cover is refused by name at enable time (head_dim > 96, C % 16, hidden % 64, mixed stages) or at forward time (a padded
  stage map above the tokenizer's 16 384 pixels, ``attn_drop`` in train mode on a window or carrier grid above 64 tokens) -- never from inside
  ``loss.backward()``.  Parameter gradients are returned to autograd (hooks and DistributedDataParallel see each exactly once).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..hat_runtime import InputNorm
from .faster_vit import FasterViTLayer, HatSwitches, PatchEmbed

# DET:853-960, the builder's eight configurations
_BACKBONE_CFGS = {
    "faster_vit_0_224": dict(depths=[2, 3, 6, 5], num_heads=[2, 4, 8, 16], window_size=[7, 7, 7, 7], dim=64, ct_size=2, in_dim=64,
                             mlp_ratio=4, drop_path_rate=0.1, hat=[False, False, True, False]),
    "faster_vit_1_224": dict(depths=[1, 3, 8, 5], num_heads=[2, 4, 8, 16], window_size=[7, 7, 7, 7], dim=80, ct_size=2, in_dim=32,
                             mlp_ratio=4, drop_path_rate=0.1, hat=[False, False, True, False]),
    "faster_vit_2_224": dict(depths=[3, 3, 8, 5], num_heads=[2, 4, 8, 16], window_size=[7, 7, 7, 7], dim=96, ct_size=2, in_dim=64,
                             mlp_ratio=4, drop_path_rate=0.1, hat=[False, False, True, False]),
    "faster_vit_3_224": dict(depths=[3, 3, 12, 5], num_heads=[2, 4, 8, 16], window_size=[7, 7, 7, 7], dim=128, ct_size=2, in_dim=64,
                             mlp_ratio=4, drop_path_rate=0.1, layer_scale=1e-5, hat=[False, False, True, False]),
    "faster_vit_4_224": dict(depths=[3, 3, 12, 5], num_heads=[4, 8, 16, 32], window_size=[7, 7, 7, 7], dim=196, ct_size=2, in_dim=64,
                             mlp_ratio=4, drop_path_rate=0.1, layer_scale=1e-5, hat=[False, False, True, False]),
    "faster_vit_4_21k_224": dict(depths=[3, 3, 12, 5], num_heads=[4, 8, 16, 32], window_size=[7, 7, 14, 7], dim=196, ct_size=2, in_dim=64,
                                 mlp_ratio=4, drop_path_rate=0.1, layer_scale=1e-5, hat=[False, False, False, False]),
    "faster_vit_4_21k_384": dict(depths=[3, 3, 12, 5], num_heads=[4, 8, 16, 32], window_size=[7, 7, 24, 12], dim=196, ct_size=2, in_dim=64,
                                 mlp_ratio=4, drop_path_rate=0.1, layer_scale=1e-5, hat=[False, False, False, False]),
    "faster_vit_4_21k_512": dict(depths=[3, 3, 12, 5], num_heads=[4, 8, 16, 32], window_size=[7, 7, 32, 16], dim=196, ct_size=2, in_dim=64,
                                 mlp_ratio=4, drop_path_rate=0.1, layer_scale=1e-5, hat=[False, False, False, False]),
}
BACKBONE_NAMES = tuple(_BACKBONE_CFGS)


class BackboneLayer(FasterViTLayer):
    """FasterViTLayer of the detection variant (DET:595-708): same modules and keys as the classifier's level; ``forward`` returns
    ``(downsample(x), x)`` with the pre-downsample map, and a hierarchical stage follows the window grid of each input."""

    dynamic_grid = True   # read by fastervit_amd.hat_runtime

    def forward(self, x):
        if self.transformer_block and len(self.blocks) and self.__dict__.get("hat_backward", False) and x.is_cuda and \
                (self.training or torch.is_grad_enabled()):
            # FasterViTBackbone.enable_hat_backward: the stage as one autograd node (eval: fused forward; train: unit-kernel chain with stochastic
            # depth); raises HERE, at forward time, if this call's geometry has no backward
            from .. import hat_backward
            x = hat_backward.stage_forward_with_grad(self, x)
        elif self.transformer_block and len(self.blocks):
            from .. import hat_runtime
            tok = None
            if self.do_gt and self.blocks[0].do_sr_hat:
                tok = lambda xp: hat_runtime.token_init_dyn(self.global_tokenizer, xp, self.window_size)  # noqa: E731
            x = hat_runtime.stage_forward(self, x, tokenizer=tok)
        else:
            # DET:687-704 pads every level to a multiple of its window, the conv levels too (the second conv of a block then reads the
            # first one's values in the pad, not zeros, along the right / bottom edge), and crops after the blocks
            H, W = x.shape[2], x.shape[3]
            ws = self.window_size
            pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
            if pad_r or pad_b:
                x = F.pad(x, (0, pad_r, 0, pad_b))
            for blk in self.blocks:
                x, _ = blk(x, None)
            x = x[:, :, :H, :W]
        return (x if self.downsample is None else self.downsample(x)), x


class FasterViTBackbone(HatSwitches, InputNorm, nn.Module):
    """DET:710-850.  ``forward(tensor_list)`` takes any object with ``.tensors`` (B, 3, H, W) and ``.mask`` (B, H, W) and returns
    ``{k: type(tensor_list)(feature, mask)}`` for the k-th entry of ``out_indices``; ``forward_features(x)`` returns the tuple of NCHW
    fp32 maps.  Any H, W: detection batches change size from call to call.

    uint8 images (``set_input_norm``) stand for their normalised fp32 image, as for the classifier: ``forward_features(u8)`` of a
    deployed backbone normalises inside the stem kernel, every other route runs one normalisation pass first; ``forward(tensor_list)`` passes
    ``tensor_list.mask`` to that pass so that padded pixels are 0, as they are in a float ``NestedTensor`` (DINO pads after normalising)."""

    def __init__(self, dim, in_dim, depths, ct_size, mlp_ratio, num_heads, window_size=(7, 7, 7, 7), resolution=224, drop_path_rate=0.2,
                 in_chans=3, num_classes=1000, qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., layer_scale=None,
                 layer_scale_conv=None, hat=(False, False, True, False), do_propagation=False, norm_layer=nn.BatchNorm2d,
                 out_indices=(0, 1, 2, 3), frozen_stages=-1, **kwargs):
        super().__init__()
        if norm_layer is not nn.BatchNorm2d:
            raise NotImplementedError("the output norms are folded into fvit_feature_tap as eval BatchNorm2d; other norm layers are not implemented")
        self.num_levels = len(depths)
        self.num_features = [int(dim * 2 ** i) for i in range(self.num_levels)]
        self.num_classes = num_classes
        self.patch_embed = PatchEmbed(in_chans=in_chans, in_dim=in_dim, dim=dim)
        n_blocks = sum(depths)
        dpr = [drop_path_rate * i / max(n_blocks - 1, 1) for i in range(n_blocks)]
        if hat is None:
            hat = [True] * len(depths)
        self.levels = nn.ModuleList()
        for i in range(len(depths)):
            r = int(2 ** (-2 - i) * resolution)
            self.levels.append(BackboneLayer(
                dim=int(dim * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size[i], ct_size=ct_size,
                mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, conv=(i < 2), drop=drop_rate, attn_drop=attn_drop_rate,
                drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], downsample=(i < 3), layer_scale=layer_scale,
                layer_scale_conv=layer_scale_conv, input_resolution=[r, r], only_local=not hat[i], do_propagation=do_propagation,
                any_res=False))
        self.out_indices = tuple(out_indices)
        for i in self.out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        if frozen_stages >= 2:
            # DET:807-812 reads self.network, which the reference model does not have (AttributeError)
            raise ValueError(f"frozen_stages={frozen_stages}: only -1, 0 and 1 are supported (the reference fails for >= 2)")
        self.frozen_stages = frozen_stages
        self.hat_operand_dtype = "f16"
        self._freeze_stages()

    def _freeze_stages(self):
        """DET:801-805: frozen_stages >= 0 puts the stem in eval mode and stops its gradients (0 and 1 behave alike)."""
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False

    def train(self, mode: bool = True):
        super().train(mode)
        self._freeze_stages()
        return self

    def enable_hat_backward(self, on: bool = True):
        """Make the backbone differentiable and trainable on the HIP path (off by default: inference-only).  With it on, an eval-mode forward with
        grad enabled (input and / or parameters requiring grad) and every train-mode forward run the transformer levels through
        ``fastervit_amd.hat_backward`` (one autograd node per level, per-call geometry) and the ``norm{i}`` outputs through the differentiable
        feature tap; under ``torch.no_grad()`` in eval mode nothing changes.  Windows and carrier grids of any length are covered (the grids change
        from call to call, so there is no short-only mode: ``hat_backward_long`` is set on every transformer level).  Refused here, by name:
        head_dim > 96, C not a multiple of 16, hidden not a multiple of 64, mixed hierarchical / local stages; size-dependent limits are refused at
        forward time.  ``enable_hat_backward(False)`` restores the inference-only behaviour.  Returns ``self``."""
        # the grids change from call to call: long sequences always on; a refusal leaves the flag on the levels, False
        return self._set_hat_backward(bool(on), bool(on), "backbone", refused_long=False)

    def _wants_grad_path(self, x: torch.Tensor) -> bool:
        if not self.__dict__.get("hat_backward", False):
            return False
        if self.training or any(lvl.training for lvl in self.levels):
            return True
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))

    def _forward_features_grad(self, x: torch.Tensor):
        """``forward_features`` with autograd (``enable_hat_backward``): see the module docstring."""
        from ..hat_backward import feature_tap_with_grad
        from ..hat_runtime import _require_gpu
        _require_gpu(x, "FasterViTBackbone")
        x = self.patch_embed(self.normalize_input(x))
        outs = []
        for idx, level in enumerate(self.levels):
            x, xo = level(x)
            if idx in self.out_indices:
                norm = getattr(self, f"norm{idx}")
                if norm.training:   # batch statistics + running-stat update on the cropped map, as the reference's module call
                    outs.append(norm(xo).float().contiguous())
                else:
                    outs.append(feature_tap_with_grad(xo, norm))
        return tuple(outs)

    def _check_inference(self, x: torch.Tensor) -> None:
        if self.training and any(lvl.transformer_block and len(lvl.blocks) for lvl in self.levels):
            raise RuntimeError("FasterViTBackbone is inference-only: its transformer stages have no backward (carrier grids above 64 tokens); "
                               "call model.eval()")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("FasterViTBackbone is inference-only and its outputs carry no gradient: run it under torch.no_grad() "
                               "(or torch.inference_mode()), or freeze its parameters and detach the input")

    def switch_to_deploy(self, dtype=torch.float16):
        """Opt-in inference plan (``fastervit_amd.conv_runtime.BackboneDeployPlan``): BatchNorm folded into the conv weights, 16-bit
        channels_last conv-side maps on the HIP conv kernels, ``norm{i}`` folded into the feature tap.  ``forward_features`` / ``forward`` use it wherever
        they take the inference branch (eval mode; with ``enable_hat_backward`` on: under ``torch.no_grad()``); the grad and train paths are untouched.
        A weight change is picked up by the next call.  ``dtype``: ``torch.float16`` or ``torch.bfloat16``; ``None`` returns to module mode."""
        if dtype is None:
            self.__dict__.pop("_deploy_plan", None)
            return self
        from ..conv_runtime import BackboneDeployPlan
        self.__dict__["_deploy_plan"] = BackboneDeployPlan(self, dtype)
        return self

    def compile_inference(self, example: torch.Tensor, dtype=torch.float16, graph: bool = True, slot_base: int = 0, streams: int = 1, precise=None):
        """The deploy plan captured ONCE into a hipGraph with static buffers, for ``example``'s device, image size and maximum batch (shorter batches are
        zero-padded; another image size raises): ``runner(x)`` -> the tuple of ``forward_features``, ``runner.forward(tensor_list)`` -> the dict of
        ``forward``.  One runner per input-size bucket.  See ``fastervit_amd.inference.CompiledBackboneInference``."""
        from ..inference import CompiledBackboneInference
        return CompiledBackboneInference(self, example, dtype=dtype, graph=graph, slot_base=slot_base, streams=streams, precise=precise)

    def forward_features(self, x: torch.Tensor):
        """Tuple of the ``out_indices`` levels' normalised pre-downsample maps, NCHW fp32."""
        if self._wants_grad_path(x):
            return self._forward_features_grad(x)
        self._check_inference(x)
        plan = self.__dict__.get("_deploy_plan")
        if plan is None or getattr(self, "_is_replica", False):
            x = self.normalize_input(x)   # module mode has no uint8 stem
        if plan is not None and not getattr(self, "_is_replica", False):
            with torch.no_grad():
                return plan.forward(x)
        from ..hat_runtime import feature_tap
        with torch.no_grad():
            x = self.patch_embed(x)
            outs = []
            for idx, level in enumerate(self.levels):
                x, xo = level(x)
                if idx in self.out_indices:
                    outs.append(feature_tap(xo, getattr(self, f"norm{idx}")))
        return tuple(outs)

    def forward(self, tensor_list):
        # uint8 tensors: normalised here, with the mask, so that padded pixels are the float NestedTensor's zeros (not normalise(0))
        return self._nested(self.forward_features(self.normalize_input(tensor_list.tensors, tensor_list.mask)), tensor_list)

    @staticmethod
    def _nested(outs, tensor_list):
        """``{k: NestedTensor(feature, mask interpolated to the feature's size)}`` of the returned levels."""
        m = tensor_list.mask
        if m is None:
            raise ValueError("FasterViTBackbone.forward: tensor_list.mask is None")
        res = {}
        for idx, out in enumerate(outs):   # DET:839-844: keys count the returned levels, not the level indices
            mask = F.interpolate(m[None].float(), size=out.shape[-2:]).to(torch.bool)[0]
            res[idx] = type(tensor_list)(out, mask)
        return res


def build_fastervit(modelname: str, **kw) -> FasterViTBackbone:
    """DET:853-960: the builder DINO's ``backbone.py`` calls as ``build_fastervit(name, out_indices=..., use_checkpoint=...)``; keyword
    arguments override the configuration (``use_checkpoint`` and other unknown ones are accepted and ignored)."""
    if modelname not in _BACKBONE_CFGS:
        raise ValueError(f"unknown backbone {modelname!r}; choose from {BACKBONE_NAMES}")
    cfg = dict(_BACKBONE_CFGS[modelname])
    cfg.update(kw)
    return FasterViTBackbone(**cfg)
