"""The conv driver's route rules, without a GPU: ``fvit_conv3x3_route`` (csrc/fvit_conv.hip: choose_conv_route) over the smallest shapes that
separate the rules, the rows each fvit_tune knob moves, the refusals, and the source properties that keep the choice in one place."""
import os
import re

import pytest

from fastervit_amd import _lib
from tests.util import CSRC_DIR, tuned

P = 0x1000   # a dummy non-null address: the route query never dereferences data pointers
ROUTE_KNOBS = ("conv_halo", "conv_patch", "conv_patch_max_waste_pct", "conv_n128_ragged", "conv128_narrow", "conv64_variant", "conv_band")
LEGACY_CALLS = ("fvit_conv3x3_patch_form", "fvit_conv3x3_c128_band_supported", "fvit_conv3x3_nhwc_dense", "fvit_conv3x3_nhwc_px_dense",
                "fvit_conv3x3_c128_band", "fvit_conv3x3_c64_ln2d", "fvit_conv3x3_c128_band_ln2d")


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def route(lib, cin, cout, hw, stride=1, terms=1, cv=None, images="c", ln=False, px=False, dtype=_lib.FVIT_F16, **call):
    """Route name of a B = 1 call on an hw x hw map; ``images``: which of classic / dense / band_frag are packed; ``px``: a two-term input."""
    w = _lib.FvitConvWeights(P if "c" in images else None, P if "d" in images else None, P if "b" in images else None, terms, cin if cv is None else cv)
    c = _lib.FvitConvCall(in_=P, out=P, zeros=P, B=1, Hi=hw, Wi=hw, Cin=cin, Cout=cout, stride=stride, act=0, **call)
    if ln:
        c.residual, c.ln_w, c.ln_b, c.ln_eps = P, P, P, 1e-5
    if px:
        c.in_lo = P
    r = lib.fvit_conv3x3_route(dtype, w, c)
    return lib.fvit_conv3x3_route_name(r).decode() if r >= 0 else (r, lib.fvit_last_error().decode())


HALO, BAND, PATCH = "conv3x3_c64_halo_kernel", "conv3x3_c128_band_kernel", "conv3x3_kernel<2,2,4,patch>"
T128, T64 = "conv3x3_kernel<2,2,4>", "conv3x3_kernel<2,2,2>"
# row: (arguments of ``route``, route name under the default knobs)
TABLE = {
    "c64": (dict(cin=64, cout=64, hw=16), HALO),
    "c64_ln": (dict(cin=64, cout=64, hw=16, ln=True), HALO + "<ln>"),
    "c64_terms2": (dict(cin=64, cout=64, hw=16, terms=2), T64),
    "c64_s2": (dict(cin=64, cout=64, hw=16, stride=2), T64),
    "c128_14": (dict(cin=128, cout=128, hw=14, images="cb"), BAND),
    "c128_14_ln": (dict(cin=128, cout=128, hw=14, images="cb", ln=True), BAND + "<ln>"),
    "c128_14_nofrag": (dict(cin=128, cout=128, hw=14), T128),          # patch grid: 2 x 128 slots for 196 pixels, 30 % waste > 10 %
    "c128_32": (dict(cin=128, cout=128, hw=32, images="cb"), PATCH),   # too wide for the band (BD_MAXPW = 32 includes two pad columns), patch waste 0
    "c64_128_s2": (dict(cin=64, cout=128, hw=16, stride=2), T128),
    "c128_192_s2": (dict(cin=128, cout=192, hw=16, stride=2), T128),   # ragged last N tile
    "c128_192": (dict(cin=128, cout=192, hw=16), PATCH),
    "c128_64": (dict(cin=128, cout=64, hw=16), T64),
    "d40": (dict(cin=64, cout=64, hw=16, cv=40, images="d"), "conv3x3_kernel<2,2,2,dense>"),
    "d104_14": (dict(cin=128, cout=128, hw=14, cv=104, images="cd"), "conv3x3_kernel<2,2,4,dense>"),
    "d104_16": (dict(cin=128, cout=128, hw=16, cv=104, images="cd"), PATCH),   # reads the classic rows
    "px64": (dict(cin=64, cout=64, hw=16, terms=2, px=True), "conv3x3_kernel<2,2,2,px>"),
    "px128_16": (dict(cin=128, cout=128, hw=16, terms=2, px=True), "conv3x3_kernel<2,2,4,px,patch>"),
    "px128_14": (dict(cin=128, cout=128, hw=14, terms=2, px=True), "conv3x3_kernel<2,2,4,px>"),
    "px_d40": (dict(cin=64, cout=64, hw=16, terms=2, px=True, cv=40, images="d"), "conv3x3_kernel<2,2,2,px,dense>"),
    "px_d104_16": (dict(cin=128, cout=128, hw=16, terms=2, px=True, cv=104, images="d"), "conv3x3_kernel<2,2,4,px,dense>"),
    "px_d104_14": (dict(cin=128, cout=128, hw=14, terms=2, px=True, cv=104, images="cd"), "conv3x3_kernel<2,2,4,px,dense>"),
}
# knob setting -> the rows it moves (every other row keeps its default route)
KNOB_MOVES = {
    ("conv_halo", 0): {"c64": T64, "c64_ln": T64},
    ("conv_band", 0): {"c128_14": T128, "c128_14_ln": T128},
    ("conv_patch", 0): {"c128_32": T128, "c128_192": T128, "d104_16": "conv3x3_kernel<2,2,4,dense>", "px128_16": "conv3x3_kernel<2,2,4,px>"},
    ("conv_patch_max_waste_pct", 31): {"c128_14_nofrag": PATCH, "d104_14": PATCH, "px128_14": "conv3x3_kernel<2,2,4,px,patch>",
                                       "px_d104_14": "conv3x3_kernel<2,2,4,px,patch>"},
    ("conv_n128_ragged", 0): {"c128_192_s2": T64, "c128_192": T64},
    # 128 x 64 tiles instead of every 128-column form of the 16-bit kernels; the two-term-map tiles ignore it, their patch form does not
    ("conv128_narrow", 1): {"c128_14_nofrag": T64, "c128_32": T64, "c64_128_s2": T64, "c128_192_s2": T64, "c128_192": T64,
                            "d104_14": "conv3x3_kernel<2,2,2,dense>", "d104_16": "conv3x3_kernel<2,2,2,dense>", "px128_16": "conv3x3_kernel<2,2,4,px>"},
    ("conv64_variant", 1): {"c64_terms2": "conv3x3_kernel<4,1,4>", "c64_s2": "conv3x3_kernel<4,1,4>", "c128_64": "conv3x3_kernel<4,1,4>"},
}


def test_every_route_knob_is_exercised():
    assert {k for k, _ in KNOB_MOVES} == set(ROUTE_KNOBS)


@pytest.mark.parametrize("dtype", [_lib.FVIT_F16, _lib.FVIT_BF16])
def test_route_table_under_the_default_knobs(lib, dtype):
    got = {row: route(lib, dtype=dtype, **kw) for row, (kw, _) in TABLE.items()}
    assert got == {row: want for row, (_, want) in TABLE.items()}


@pytest.mark.parametrize("knob,value", sorted(KNOB_MOVES))
def test_a_knob_moves_exactly_the_rows_of_its_rule(lib, knob, value):
    want = {row: KNOB_MOVES[(knob, value)].get(row, dflt) for row, (_, dflt) in TABLE.items()}
    with tuned(**{knob: value}):
        got = {row: route(lib, **kw) for row, (kw, _) in TABLE.items()}
    assert got == want
    assert {row: route(lib, **kw) for row, (kw, _) in TABLE.items()} == {row: dflt for row, (_, dflt) in TABLE.items()}   # restored


def test_route_ids_and_names(lib):
    names = [lib.fvit_conv3x3_route_name(i).decode() for i in range(15)]
    assert len(set(names)) == 15 and "?" not in names and {want for _, want in TABLE.values()} <= set(names)
    assert lib.fvit_conv3x3_route_name(15) == b"?" and lib.fvit_conv3x3_route_name(-1) == b"?"
    assert all(len(n) < 40 for n in names)   # FvitProfRecord.name


def test_refusals(lib):
    # the only eligible kernel lacks its image: the map is too wide for the row-band kernel, and nothing else reads a fragment stream
    rc, msg = route(lib, 128, 128, 32, images="b")
    assert rc == -1 and "classic" in msg
    rc, msg = route(lib, 64, 64, 16, cv=40, images="b")
    assert rc == -1 and "dense" in msg
    for kw, word in [(dict(cv=41, images="d"), "cin_valid=41 must be a multiple of 8"), (dict(cv=72, images="d"), "cin_valid=72"),
                     (dict(terms=2, out_f32=P, out_lo=P), "conv3x3_px: unsupported arguments"), (dict(terms=1, px=True), "conv3x3_px: unsupported arguments"),
                     (dict(stride=3), "conv3x3: unsupported arguments"), (dict(dtype=_lib.FVIT_F32), "dtype 0 not supported")]:
        rc, msg = route(lib, 64, 64, 16, **kw)
        assert rc == -1 and word in msg, (kw, msg)
    rc, msg = route(lib, 96, 64, 16)
    assert rc == -1 and "Cin % 64 == 0" in msg
    c = _lib.FvitConvCall(in_=P, out=P, zeros=P, B=1, Hi=16, Wi=16, Cin=64, Cout=64, stride=1, act=2, residual=P, ln_w=P, ln_b=P)
    assert lib.fvit_conv3x3_route(_lib.FVIT_F16, _lib.FvitConvWeights(P, None, None, 1, 64), c) == -1 and b"LayerNorm2d" in lib.fvit_last_error()
    assert lib.fvit_conv3x3_route(_lib.FVIT_F16, None, c) == -1 and lib.fvit_conv3x3(_lib.FVIT_F16, None, None, None) == -1


def test_legacy_queries_follow_the_driver(lib):
    assert lib.fvit_conv3x3_patch_form(1, 32, 32, 128, 128, 1) == 1 and lib.fvit_conv3x3_patch_form(1, 14, 14, 128, 128, 1) == 0
    assert lib.fvit_conv3x3_patch_form(1, 32, 32, 128, 128, 2) == 0 and lib.fvit_conv3x3_patch_form(1, 32, 32, 64, 64, 1) == 0
    assert lib.fvit_conv3x3_c128_band_supported(28, 30) == 1 and lib.fvit_conv3x3_c128_band_supported(28, 31) == 0
    with tuned(conv_band=0, conv_patch=0):
        assert lib.fvit_conv3x3_c128_band_supported(28, 30) == 0 and lib.fvit_conv3x3_patch_form(1, 32, 32, 128, 128, 1) == 0


def test_the_choice_lives_in_one_place():
    src = open(os.path.join(CSRC_DIR, "fvit_conv.hip")).read()
    units = [f for f in sorted(os.listdir(CSRC_DIR)) if f.endswith((".hip", ".h"))]
    assert {"fvit_conv.h", "fvit_conv_gemm.hip", "fvit_conv_halo.hip", "fvit_conv_band.hip", "fvit_stem.hip"} <= set(units)
    everything = "".join(open(os.path.join(CSRC_DIR, f)).read() for f in units)
    for knob in ROUTE_KNOBS:   # read once, in the driver: no kernel unit reads a route knob
        assert len(re.findall(r'tune_get\(\s*"%s"' % knob, src)) == 1, knob
        assert len(re.findall(r'tune_get\(\s*"%s"' % knob, everything)) == 1, knob
    assert "__global__" not in src and everything.count("choose_conv_route(") == src.count("choose_conv_route(")
    rt = open(os.path.join(os.path.dirname(CSRC_DIR), "conv_runtime.py")).read()
    for name in LEGACY_CALLS:
        assert not re.search(r"\b%s\b" % name, rt), name
