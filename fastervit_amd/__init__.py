"""fastervit_amd -- MI355X-native FasterViT forward path (drop-in for ``fastervit``'s model API).

>>> from fastervit_amd import create_model
>>> model = create_model('faster_vit_0_224').cuda().eval()

The Hierarchical-Attention stages run in hand-written gfx950 HIP kernels (``csrc/``) behind the C
ABI of ``include/fvit_hip.h``; the conv side is PyTorch-ROCm.  See DESIGN.md / INTEGRATION.md.
"""
from .models import create_model, list_models, is_model, model_entrypoint  # noqa: F401
from .models import FasterViTBackbone, build_fastervit  # noqa: F401  (multi-scale detection backbone)
from .ops import MSDeformAttn, MSDeformAttnFunction, ms_deform_attn  # noqa: F401  (multi-scale deformable attention of the DINO heads)
from .preprocess import ClassifierPreprocess, DetectionPreprocess, NestedTensor, resize_batch  # noqa: F401  (decoded uint8 images -> uint8 batch, on the GPU)
from .detection_ops import (  # noqa: F401  (what comes after the DINO heads: top-k decode, NMS, box IoU / GIoU, the matcher's cost)
    HungarianMatcher, PostProcess, batched_nms, box_cxcywh_to_xyxy, box_iou, box_xyxy_to_cxcywh, generalized_box_iou, hungarian_assign, nms,
    postprocess_launch)
from .criterion import SetCriterion, sigmoid_focal_loss  # noqa: F401  (the DINO training criterion: focal, L1 and GIoU losses, forward and backward)
from .models.registry import load_checkpoint, load_state_dict, register_pip_model  # noqa: F401

__version__ = "0.1.0"
