"""Cases of the multi-scale detection backbone (fastervit_amd.build_fastervit), shared by the golden generator
(tests/golden/make_backbone_golden.py), the CPU tests and the GPU tests.

``name`` + ``kwargs`` is how both the reference builder and ``build_fastervit`` are called; ``hw`` the input size (batch 2 everywhere);
``mask`` names the padding mask of tests/backbone_cases.make_mask.  Reduced widths keep the goldens small (each file < 1 MB): dim 16
gives stages of 64 / 128 channels with head_dim 32.
"""
import torch

SEED = 1234
BATCH = 2
_TINY = dict(depths=[1, 1, 2, 2], num_heads=[1, 1, 2, 4], dim=16, in_dim=16)

BACKBONE_CASES = {
    # FasterViT-0 shape, exact window multiples: stage 2 is 14x14 (2x2 windows, G = 16 = the build-time carrier grid)
    "bb_tiny_exact": dict(name="faster_vit_0_224", kwargs=dict(_TINY, out_indices=(0, 1, 2, 3)), hw=(224, 224), family="stress", mask="none"),
    # odd sizes: every level is padded and cropped; stage 2 is 13x21 -> 14x21 (2x3 windows, G = 24: non-square, > 16); stage 3 7x11 -> 7x14
    "bb_tiny_odd": dict(name="faster_vit_0_224", kwargs=dict(_TINY, out_indices=(1, 2, 3)), hw=(200, 328), family="stress", mask="pad"),
    # stage 2 is 7x14: a 1x2 window grid, G = 8 < 16 (the carrier bias is cropped)
    "bb_tiny_g8": dict(name="faster_vit_0_224", kwargs=dict(_TINY, out_indices=(0, 1, 2, 3)), hw=(112, 224), family="stress", mask="pad"),
    # 2x4 windows (G = 32), layer scale and carrier propagation
    "bb_tiny_wide": dict(name="faster_vit_3_224", kwargs=dict(_TINY, out_indices=(1, 2, 3), do_propagation=True), hw=(224, 448),
                         family="stress", mask="none"),
    # faster_vit_4_21k_384 shape: local 24 / 12 windows, no carrier tokens; stage 2 is 20x22 -> one 24x24 window of 576 tokens
    "bb_tiny_21k_384": dict(name="faster_vit_4_21k_384", kwargs=dict(_TINY, out_indices=(1, 2, 3)), hw=(320, 352), family="stress",
                            mask="pad"),
    # full-width faster_vit_0_224: stage 2 is 10x12 -> 14x14 (2x2 windows)
    "bb_fvit0_160x192": dict(name="faster_vit_0_224", kwargs=dict(out_indices=(1, 2, 3)), hw=(160, 192), family="init", mask="pad"),
}


def make_mask(kind: str, batch: int, H: int, W: int) -> torch.Tensor:
    """(B, H, W) bool padding mask (True = padding), as DINO's NestedTensor carries: 'none' all False; 'pad' image 0 padded on the right
    third, image 1 on the bottom quarter."""
    m = torch.zeros(batch, H, W, dtype=torch.bool)
    if kind == "pad":
        m[0, :, W - W // 3:] = True
        if batch > 1:
            m[1, H - H // 4:, :] = True
    return m
