"""Writes tests/golden/resize_cases.npz: what PIL's Image.resize returns for a dozen small uint8 images, both filters.

    python tests/golden/make_resize_golden.py

Needs Pillow and numpy only (generated with Pillow 12.2.0).  Per case i: img_i (H, W, 3) uint8, bilinear_i / bicubic_i (rh, rw, 3) uint8 = PIL's result;
`sizes` (n, 4) = H, W, rh, rw; `diff_share` (n, 2) = the share of bytes at which the float64 restatement of tests/resize_refs.py differs from PIL (never
by more than one level: PIL's 22-bit fixed-point coefficients decide the ties), recorded here so that tests/test_resize_refs_cpu.py notices a drift.
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import resize_refs as rr  # noqa: E402  (numpy only)

# (kind, H, W, rh, rw): up- and downscales, odd sizes, one unchanged axis each way, a 1x1 source, a 14.4x and a 16x downscale
CASES = [("noise", 9, 7, 5, 4), ("noise", 37, 53, 16, 20), ("smooth", 37, 53, 16, 20), ("noise", 21, 34, 47, 71), ("noise", 20, 31, 45, 70),
         ("noise", 33, 33, 33, 17), ("noise", 17, 29, 40, 29), ("mult8", 6, 6, 13, 11), ("noise", 1, 1, 4, 4), ("noise", 3, 130, 3, 9),
         ("smooth", 64, 48, 24, 24), ("noise", 80, 48, 5, 3)]
PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def main():
    arrays, sizes, shares = {}, [], []
    for i, (kind, H, W, rh, rw) in enumerate(CASES):
        img = rr.make_image(kind, H, W)
        arrays[f"img_{i}"] = img
        sizes.append((H, W, rh, rw))
        row = []
        for name in rr.FILTER_NAMES:
            pil = np.asarray(Image.fromarray(img).resize((rw, rh), PIL_FILTER[name]))
            arrays[f"{name}_{i}"] = pil
            diff = np.abs(pil.astype(np.int32) - rr.reference(img, rh, rw, name).out.astype(np.int32))
            assert diff.max() <= 1, (kind, H, W, rh, rw, name, int(diff.max()))
            row.append(float((diff > 0).mean()))
        shares.append(row)
    arrays["sizes"] = np.asarray(sizes, dtype=np.int32)
    arrays["diff_share"] = np.asarray(shares, dtype=np.float64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resize_cases.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(CASES)} cases, largest share {100 * max(max(r) for r in shares):.2f} %")


if __name__ == "__main__":
    main()
