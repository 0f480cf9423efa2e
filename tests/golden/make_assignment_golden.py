"""Writes tests/golden/assignment_cases.npz: scipy's answer to every case of tests/assignment_refs.py.

    python -m tests.golden.make_assignment_golden

Per case and image b: ``{name}_{b}_src`` / ``_tgt`` (scipy.optimize.linear_sum_assignment of the fp32 block, int64), ``_total`` (fp64) and, except for the
tie cases, ``_margin`` (assignment_refs.margin with scipy as the solver); per case ``{name}_sum``, the checksum of the cost matrix, which is not stored but
drawn again from its seed.  Needs scipy; nothing else.
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import assignment_refs as A


def main():
    out = {}
    for name in A.case_names():
        cost, sizes = A.draw(name)
        out[f"{name}_sum"] = np.float64(A.checksum(cost))
        for b, block in enumerate(A.blocks(cost, sizes)):
            src, tgt = linear_sum_assignment(block)
            out[f"{name}_{b}_src"], out[f"{name}_{b}_tgt"] = src.astype(np.int64), tgt.astype(np.int64)
            out[f"{name}_{b}_total"] = np.float64(A.total(block, src, tgt))
            if name not in A.TIE_CASES:
                m = A.margin(block) if block.shape[1] else np.inf
                out[f"{name}_{b}_margin"] = np.float64(m)
                print(f"{name} image {b}: {block.shape[0]} x {block.shape[1]}, total {out[f'{name}_{b}_total']:.6f}, margin {m:.3g}")
    np.savez_compressed(A.GOLDEN, **out)


if __name__ == "__main__":
    main()
