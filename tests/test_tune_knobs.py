"""The fvit_tune knob table the tests rely on (tests/util.py: tuned), checked against the HIP sources.  CPU only.

``fvit_tune`` accepts any key, so a misspelled knob in a test would silently run the default path; ``tuned`` refuses keys that no
``tune_get`` reads and restores every knob to the default parsed from the sources."""
import glob
import os
import re

import pytest

from tests import test_gpu_determinism, test_gpu_fused_stages
from tests.util import CSRC_DIR, tune_defaults, tune_uses, tuned


def test_every_tune_get_is_parsed_with_one_default():
    loose = set()
    for path in glob.glob(os.path.join(CSRC_DIR, "*.hip")) + glob.glob(os.path.join(CSRC_DIR, "*.h")):
        with open(path) as f:
            loose |= set(re.findall(r'tune_get\(\s*"([A-Za-z0-9_]+)"', f.read()))
    uses = tune_uses()
    assert set(uses) == loose, f"tune_get calls the parser missed: {sorted(loose - set(uses))}"
    assert len(uses) >= 51
    conflicts = {k: v for k, v in uses.items() if len(v) != 1}
    assert not conflicts, f"knobs read with different defaults: {conflicts}"
    d = tune_defaults()
    # spot checks of the dispatch thresholds the fused-stage tests reason about (fvit_api.hip)
    assert d["attn_fused_min_rows"] == 16384 and d["mlp_fused_min_rows"] == 16384 and d["attn_fused512_min_rows"] == 1 << 30
    assert d["ct_fused"] == 1 and d["win_fused"] == 1 and d["win_fused256"] == 0 and d["win_mlp256"] == 2 and d["mlp_variant"] == -1


def test_every_knob_the_gpu_tests_set_exists():
    d = tune_defaults()
    sets = list(test_gpu_determinism.KNOB_SETS) + list(test_gpu_fused_stages.SETTINGS.values())
    for knobs in sets:
        assert set(knobs) <= set(d), f"unknown knob(s) {sorted(set(knobs) - set(d))}"


def test_tuned_refuses_unknown_knobs():
    with pytest.raises(KeyError, match="ct_fuesd"):
        with tuned(ct_fuesd=0):
            pass
