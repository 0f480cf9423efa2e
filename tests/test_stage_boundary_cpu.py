"""The stage-boundary fusion adds two fvit_tune knobs and no entry point: the knobs default to 1 in the HIP sources and are documented in the public
header, the ABI version the other CPU tests pin is unchanged, and every function the header declares is still bound by the Python loader."""
import os
import re

from fastervit_amd import _lib
from tests.util import tune_defaults

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fvit_hip.h")


def test_knobs_default_on_and_documented():
    d = tune_defaults()
    with open(HEADER) as f:
        text = f.read()
    for knob in ("stage_entry_fused", "stage_exit_fused"):
        assert d[knob] == 1
        assert f'"{knob}"' in text


def test_abi_unchanged_and_header_symbols_bound():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"#define FVIT_ABI_VERSION (\d+)", text).group(1) == "10" and _lib.FVIT_ABI_VERSION == 10
    declared = set(re.findall(r"^\w[\w \*]*?\b(fvit_\w+)\(", text, flags=re.M))
    assert "fvit_hat_stage_forward_tail" in declared
    # the binding reads its signatures from the header: every prototype this regex finds must be one it declares on the handle
    product, diag = _lib.parse_header(text)
    missing = sorted(n for n in declared if n not in product and n not in diag)
    assert not missing, missing
    assert set(product) == set(_lib.EXPORTED_SYMBOLS) and set(diag) == set(_lib.DIAG_SYMBOLS)
    assert len(product["fvit_hat_stage_forward_tail"][1]) == 10
