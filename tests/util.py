"""Helpers shared by the test modules (test infrastructure; may import the oracle)."""
import ast
import contextlib
import glob
import os
import re

import numpy as np
import torch

from tests.cases import CASES, SEED
from tests.synth import synth_input, synth_state_dict

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def build_product_model(name, device="cpu", dtype=None):
    """Product model for a parity case with the case's synthetic weights loaded."""
    import fastervit_amd
    case = CASES[name]
    model = fastervit_amd.create_model(case["entry"], **case["kwargs"]).eval()
    sd = synth_state_dict(model.state_dict(), SEED, case["family"])
    model.load_state_dict(sd, strict=True)
    if dtype is not None:
        model = model.to(dtype)
    return model.to(device), sd


def case_input(name):
    case = CASES[name]
    return synth_input(case["batch"], case["hw"][0], case["hw"][1], SEED)


def max_abs(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return (a - b).abs().max().item()


def rel_err(a, ref):
    """max |a - ref| / max |ref|"""
    ref = torch.as_tensor(ref).double()
    return max_abs(a, ref) / max(ref.abs().max().item(), 1e-30)


CSRC_DIR = os.path.normpath(os.path.join(os.path.dirname(GOLDEN_DIR), "..", "fastervit_amd", "csrc"))
_TUNE_GET = re.compile(r'tune_get\(\s*"([A-Za-z0-9_]+)"\s*,\s*([^()]+?)\s*\)')


def _int_literal(expr):
    """Value of a C integer default such as ``16384``, ``-1`` or ``1 << 30`` (numbers and shifts only)."""
    node = ast.parse(expr, mode="eval").body

    def ev(n):
        if isinstance(n, ast.Constant) and isinstance(n.value, int):
            return n.value
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        if isinstance(n, ast.BinOp) and isinstance(n.op, ast.LShift):
            return ev(n.left) << ev(n.right)
        raise ValueError(f"tune_get default {expr!r} is not an integer literal")
    return ev(node)


def tune_uses(csrc_dir=CSRC_DIR):
    """Every ``tune_get("key", default)`` call in the HIP sources: {key: {default: ["file:line", ...]}}."""
    uses = {}
    for path in sorted(glob.glob(os.path.join(csrc_dir, "*.hip")) + glob.glob(os.path.join(csrc_dir, "*.h"))):
        with open(path) as f:
            for ln, line in enumerate(f, 1):
                for key, expr in _TUNE_GET.findall(line):
                    uses.setdefault(key, {}).setdefault(_int_literal(expr), []).append(f"{os.path.basename(path)}:{ln}")
    return uses


def tune_defaults():
    """{knob: the value fvit_tune's table starts from}: the source default, or the FVIT_TUNE_<knob> environment override the
    library reads on first use (fvit_api.hip: tune_get)."""
    out = {}
    for key, vals in tune_uses().items():
        if len(vals) != 1:
            raise ValueError(f"knob {key!r} has conflicting defaults {vals}")
        env = os.environ.get(f"FVIT_TUNE_{key}")
        out[key] = int(env) if env is not None else next(iter(vals))
    return out


@contextlib.contextmanager
def tuned(**knobs):
    """Set fvit_tune knobs for the body and always restore them to their defaults afterwards.  A key that no
    ``tune_get`` in the HIP sources reads raises (``fvit_tune`` itself accepts any string, so a typo would
    silently test the default path)."""
    from fastervit_amd import _lib
    defaults = tune_defaults()
    unknown = sorted(k for k in knobs if k not in defaults)
    if unknown:
        raise KeyError(f"unknown fvit_tune knob(s) {unknown}")
    try:
        for k, v in knobs.items():
            _lib.tune(k, v)
        yield
    finally:
        for k in knobs:
            _lib.tune(k, defaults[k])
