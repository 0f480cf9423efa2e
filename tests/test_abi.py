"""C-ABI surface and host logic that do not need a GPU."""
import ctypes
import os
import sys
import re

import pytest
import torch

from fastervit_amd import _lib, hat_runtime
from oracle import hat_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_symbols_are_exported(lib):
    """Every function include/fvit_hip.h declares is exported by libfvit_hip.so (and vice versa for the binding); the fvit_debug_* entry points of
    its #ifdef FVIT_DIAG section are exported ONLY by the diagnosis build libfvit_hip_diag.so."""
    hdr = open(os.path.join(ROOT, "include", "fvit_hip.h")).read()
    a, b = hdr.index("#ifdef FVIT_DIAG"), hdr.index("#endif /* FVIT_DIAG */")
    diag_decl = set(re.findall(r"\b(fvit_debug_[a-z0-9_]+)\s*\(", hdr[a:b]))   # (the comments of that section mention product entry points)
    declared = set(re.findall(r"\b(fvit_[a-z0-9_]+)\s*\(", hdr[:a] + hdr[b:]))
    declared.discard("fvit_stream_t")
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    assert diag_decl == set(_lib.DIAG_SYMBOLS) and all(s.startswith("fvit_debug_") for s in diag_decl)
    shipped = ctypes.CDLL(os.path.join(_lib.CSRC_DIR, "libfvit_hip.so"))
    for s in declared:
        assert hasattr(shipped, s), s
    for s in diag_decl:
        assert not hasattr(shipped, s), f"{s} is exported by the shipped library"
    diag = ctypes.CDLL(os.path.join(_lib.CSRC_DIR, "libfvit_hip_diag.so"))
    for s in declared | diag_decl:
        assert hasattr(diag, s), s


def test_shipped_library_has_no_ablation_knobs():
    """"ablate_skip" / "*_ablate" make kernels skip work (wrong results): the strings must not even be present in the shipped library."""
    blob = open(os.path.join(_lib.CSRC_DIR, "libfvit_hip.so"), "rb").read()
    assert b"ablate_skip" not in blob and b"conv_ablate" not in blob and b"mlp_ablate" not in blob
    assert b"ablate_skip" in open(os.path.join(_lib.CSRC_DIR, "libfvit_hip_diag.so"), "rb").read()


def test_abi_version_and_struct_sizes(lib):
    assert lib.fvit_abi_version() == _lib.FVIT_ABI_VERSION
    assert ctypes.sizeof(_lib.FvitStageDesc) == 20 * 4
    assert ctypes.sizeof(_lib.FvitAttnWeights) == 12 * 8 + 2 * 4
    assert ctypes.sizeof(_lib.FvitMlpWeights) == 9 * 8
    assert ctypes.sizeof(_lib.FvitBlockWeights) == 2 * 104 + 2 * 72 + 16 + 8
    assert ctypes.sizeof(_lib.FvitMapView) == 48
    assert ctypes.sizeof(_lib.FvitConvWeights) == 3 * 8 + 2 * 4
    assert ctypes.sizeof(_lib.FvitConvCall) == 11 * 8 + 4 + 8 * 4 + 4   # 4: tail padding to the pointers' alignment


def _header():
    return open(os.path.join(ROOT, "include", "fvit_hip.h")).read()


def _edit(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


def test_parser_reads_every_prototype():
    """_lib.parse_header skips nothing: its names are those the independent regex of test_header_symbols_are_exported finds, section by section,
    and EXPORTED_SYMBOLS / DIAG_SYMBOLS are those names."""
    hdr = _header()
    a, b = hdr.index("#ifdef FVIT_DIAG"), hdr.index("#endif /* FVIT_DIAG */")
    product, diag = _lib.parse_header(hdr)
    assert set(product) == set(re.findall(r"\b(fvit_[a-z0-9_]+)\s*\(", hdr[:a] + hdr[b:])) - {"fvit_stream_t"}
    assert set(diag) == set(re.findall(r"\b(fvit_debug_[a-z0-9_]+)\s*\(", hdr[a:b])) and diag
    assert _lib.EXPORTED_SYMBOLS == tuple(product) and _lib.DIAG_SYMBOLS == tuple(diag)
    assert not any(s.startswith("fvit_debug_") for s in _lib.EXPORTED_SYMBOLS)


def test_parser_spot_signatures():
    """Six prototypes (and a size_t return, and the one override) against argtypes written out by hand from the header."""
    vp, i32, i64, f32, sz, P = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t, ctypes.POINTER
    product, _ = _lib.parse_header(_header())
    assert product["fvit_ct_block_fused"] == (ctypes.c_int, [i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, f32,
                                                             vp, vp, vp, vp, vp, vp, vp, f32, vp])
    assert len(product["fvit_ct_block_fused"][1]) == 29
    assert product["fvit_sgd_momentum"] == (ctypes.c_int, [vp, vp, vp, i64, f32, f32, f32, vp])
    assert product["fvit_box_nms"] == (ctypes.c_int, [vp, vp, vp, f32, vp, vp, vp, sz, i32, i32, vp])
    assert product["fvit_hat_stage_forward_tail"] == (ctypes.c_int, [
        P(_lib.FvitStageDesc), P(_lib.FvitBlockWeights), P(_lib.FvitStageTables), P(_lib.FvitMapView), vp, P(_lib.FvitMapView),
        P(_lib.FvitStageTail), vp, sz, vp])
    assert product["fvit_bwd_blocks"] == (ctypes.c_int32, [i32])
    assert product["fvit_last_error"] == (ctypes.c_char_p, [])
    assert product["fvit_stage_workspace_bytes"] == (sz, [P(_lib.FvitStageDesc)])
    assert product["fvit_tune"] == (ctypes.c_int, [ctypes.c_char_p, i32])
    # the descriptor array of the resize kernel is DEVICE memory (callers pass data_ptr()): void* by _lib._ARG_OVERRIDES; the host query is typed
    assert product["fvit_image_resize_u8"] == (ctypes.c_int, [vp, i32, P(_lib.FvitMapView), i32, i32, i32, vp, vp])
    assert product["fvit_image_resize_check"] == (ctypes.c_int, [P(_lib.FvitResizeDesc), i32, i32])


def test_parser_follows_header_edits():
    """A changed prototype changes the parse: swapped parameter types, a dropped parameter, a type the binding has no rule for (an error that
    names the function), a prototype moved into the FVIT_DIAG section."""
    i64, f32, vp = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    hdr = _header()
    at = "int64_t n, float lr,"   # of fvit_sgd_momentum
    assert _lib.parse_header(hdr)[0]["fvit_sgd_momentum"][1] == [vp, vp, vp, i64, f32, f32, f32, vp]
    assert _lib.parse_header(_edit(hdr, at, "float n, int64_t lr,"))[0]["fvit_sgd_momentum"][1] == [vp, vp, vp, f32, i64, f32, f32, vp]
    assert _lib.parse_header(_edit(hdr, at, "float lr,"))[0]["fvit_sgd_momentum"][1] == [vp, vp, vp, f32, f32, f32, vp]
    for bad in ("long n, float lr,", "unsigned int n, float lr,", "int64_t n[2], float lr,", "float** n, float lr,", "FvitMapView n, float lr,"):
        with pytest.raises(RuntimeError, match="fvit_sgd_momentum"):
            _lib.parse_header(_edit(hdr, at, bad))
    proto = "int fvit_tune(const char* key, int32_t value);"
    product, diag = _lib.parse_header(_edit(_edit(hdr, proto, ""), "#endif /* FVIT_DIAG */", proto + "\n#endif /* FVIT_DIAG */"))
    assert "fvit_tune" in diag and "fvit_tune" not in product
    assert diag["fvit_tune"] == (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32])


def test_loaded_library_carries_the_header_signatures(lib):
    """After _lib.lib() every product function of the handle has the header's restype and argtypes (the arity check ctypes then makes on every call)."""
    product, _ = _lib.parse_header(_header())
    for name, (restype, argtypes) in product.items():
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes and len(fn.argtypes) == len(argtypes), name


def _header_structs(text):
    """{name: [(field, C type)]} of every `typedef struct ... Name;` of the header, `int32_t H, W;` as two fields, `char tag[24]` as type char[24]."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = [d.strip() for d in decl.split(",")]
            m = re.fullmatch(r"(.*?)(\w+)\s*(\[\d+\])?", first, re.S)
            assert m and all(re.fullmatch(r"\w+", n) for n in more), f"{name}: {decl}"
            ctype = " ".join(m.group(1).split()) + (m.group(3) or "")
            fields += [(n, ctype) for n in [m.group(2)] + more]
        out[name] = fields
    return out


def _field_ctype(ctype, where):
    m = re.fullmatch(r"char\[(\d+)\]", ctype)
    if m:
        return ctypes.c_char * int(m.group(1))
    nested = getattr(_lib, ctype, None)
    if isinstance(nested, type) and issubclass(nested, ctypes.Structure):
        return nested
    return _lib.ctype_of(ctype, where)[0]


def test_structs_mirror_the_header_field_by_field():
    """Every struct of the header (product and diagnosis sections) is a _lib class with the same fields in the same order and of the same types
    (the type rule of the prototypes, plus char[N] and nested structs; `in_` stands for `in`); _lib has no struct the header lacks."""
    structs = _header_structs(_header())
    assert len(structs) >= 15 and structs["FvitStageDesc"][5:7] == [("H", "int32_t"), ("W", "int32_t")]
    assert structs["FvitDebugRowhashRecord"][0] == ("tag", "char[24]")
    for name, fields in structs.items():
        cls = getattr(_lib, name, None)
        assert isinstance(cls, type) and issubclass(cls, ctypes.Structure), f"_lib has no struct {name}"
        want = [(n, _field_ctype(t, f"{name}.{n}")) for n, t in fields]
        got = [(n[:-1] if n.endswith("_") else n, t) for n, t in cls._fields_]
        assert got == want, name
    mine = {n for n, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == _lib.__name__}
    assert mine == set(structs)


def test_constants_match_the_header():
    """Every FVIT_* number of _lib is a #define of the header with the same value."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", _header(), flags=re.S)
    defines = {n: (float(v.rstrip("f")) if "." in v else int(v))
               for n, v in re.findall(r"^[ \t]*#define[ \t]+(FVIT_\w+)[ \t]+\(?(-?[0-9][0-9.]*f?)\)?[ \t]*$", text, re.M)}
    assert len(defines) >= 35 and defines["FVIT_EINVAL"] == -1 and defines["FVIT_MASK_BIAS"] == -30000.0
    carried = {n: v for n, v in vars(_lib).items() if n.startswith("FVIT_") and isinstance(v, (int, float)) and not isinstance(v, bool)}
    assert len(carried) >= 15 and "FVIT_ABI_VERSION" in carried
    for n, v in carried.items():
        assert n in defines, f"_lib.{n} is not a #define of the header"
        assert v == defines[n] and type(v) is type(defines[n]), n


def test_attention_spad(lib):
    for S, want in [(16, 16), (36, 48), (49, 64), (53, 64), (60, 64), (148, 160), (196, 208), (129, 160)]:
        assert lib.fvit_attention_spad(S) == want


def test_workspace_bytes_and_descriptor_validation(lib):
    d = _lib.FvitStageDesc(batch=256, C=256, heads=8, dpad=32, ws=7, H=14, W=14, Hp=14, Wp=14, cw=2, hier=1, square=1,
                           hidden=1024, depth=6, do_propagation=0, operand_dtype=_lib.FVIT_F16, spad=64, gpad=16, weight_terms=1)
    n = lib.fvit_stage_workspace_bytes(ctypes.byref(d))
    d.weight_terms = 2   # hi + lo weight terms: same workspace (activations are single-rounded in every mode)
    assert lib.fvit_stage_workspace_bytes(ctypes.byref(d)) == n
    d.weight_terms = 0
    assert lib.fvit_stage_workspace_bytes(ctypes.byref(d)) == 0 and b"weight_terms" in lib.fvit_last_error()
    d.weight_terms = 1
    rows = 256 * 4 * 53
    assert n >= rows * (256 * 4 + 256 * 2 + 768 * 2 + 256 * 2 + 1024 * 2)
    assert n < 2 * rows * (256 * 4 + 256 * 2 + 768 * 2 + 256 * 2 + 1024 * 2)
    d.spad = 48  # inconsistent with fvit_attention_spad
    assert lib.fvit_stage_workspace_bytes(ctypes.byref(d)) == 0
    assert b"spad" in lib.fvit_last_error()
    d.spad, d.dpad = 64, 16  # dpad must be 32 or 64
    assert lib.fvit_stage_workspace_bytes(ctypes.byref(d)) == 0


@pytest.mark.parametrize("sr0,sr1,ws,cw", [(2, 2, 7, 2), (3, 5, 12, 2), (2, 4, 3, 2), (4, 4, 5, 1)])
def test_index_tables_reproduce_reference_permutations(sr0, sr1, ws, cw):
    """build_tables vs the oracle's ct_dewindow / ct_window / cat / nearest-upsample on tagged tensors."""
    tb = hat_runtime.build_tables(sr0, sr1, ws, cw, True)
    nW, S, G, ncw = tb["nW"], tb["S"], tb["G"], tb["ncw"]
    # X rows tagged with their own index; carrier rows of X hold windowed carrier p at (p // ncw) * S + p % ncw
    X = torch.arange(nW * S, dtype=torch.float32).view(nW * S, 1)
    ct_windowed = torch.stack([X[(p // ncw) * S + p % ncw] for p in range(G)]).view(1, G, 1)
    raster = hr.ct_dewindow(ct_windowed, cw * sr0, cw * sr1, cw)
    assert torch.equal(X[tb["ct_src"].long()].view(1, G, 1), raster)
    # after the carrier branch: R (raster) -> ct_window -> cat in front of the local tokens
    R = torch.arange(1000, 1000 + G, dtype=torch.float32).view(1, G, 1)
    ctw = hr.ct_window(R, cw * sr0, cw * sr1, cw).reshape(nW, ncw, 1)
    xloc = X.view(nW, S, 1)[:, ncw:]
    cat = torch.cat((ctw, xloc), dim=1).reshape(nW * S)
    src = tb["ln1_src"].long()
    got = torch.where(src >= 0, X.view(-1)[src.clamp(min=0)], R.view(-1)[(-src - 1).clamp(min=0)])
    assert torch.equal(got, cat)
    add = tb["ln1_add"].view(nW, S)
    assert (add[:, :ncw] == -1).all() and torch.equal(add[:, ncw:], torch.arange(ws * ws).expand(nW, -1).int())
    # propagation: nearest upsample cw -> ws
    img = torch.arange(ncw, dtype=torch.float32).view(1, 1, cw, cw)
    up = torch.nn.functional.interpolate(img, size=(ws, ws), mode="nearest").reshape(-1)
    assert torch.equal(tb["up_idx"].float(), up)


def test_product_fails_loudly_without_gpu():
    """No CPU fallback: a transformer stage on a CPU tensor raises, it does not silently compute."""
    import fastervit_amd
    m = fastervit_amd.create_model("faster_vit_0_224", depths=[1, 1, 1, 1], dim=16, in_dim=16, num_heads=[1, 1, 2, 4]).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        m(torch.randn(1, 3, 224, 224))
    blk = m.levels[3].blocks[0]
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        blk(torch.randn(1, 49, 128), None)


def test_product_does_not_import_oracle():
    """The shipped package never references oracle/ (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "fastervit_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M), f


def test_kernels_have_no_lds_pipeline_lane_exchange():
    """r02 (profiles/r02_repeatability_hunt.log): a __shfl_xor (ds_bpermute_b32, an LDS-pipeline instruction) issued while LDS-DMA of
    sibling waves was landing returned wrong lane values when kernels of several streams shared a CU.  Lane reductions go through the
    VALU helpers of fvit_common.h (v_permlane16/32_swap + DPP); only the diagnosis row-hash kernel, which has no LDS-DMA beside it,
    still shuffles."""
    csrc = os.path.join(ROOT, "fastervit_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        for ln in open(os.path.join(csrc, f)).read().splitlines():
            code = ln.split("//")[0]
            if re.search(r"__shfl|ds_bpermute|ds_permute|ds_swizzle", code):
                assert f == "fvit_glue.hip" and "h ^=" in code, f"{f}: {ln.strip()}"


def test_registry_api():
    import fastervit_amd
    from fastervit_amd.models import registry
    assert len(fastervit_amd.list_models()) == 22
    assert fastervit_amd.is_model("faster_vit_4_21k_384_any_res")
    assert registry.list_models("faster_vit_[0-6]_224") == [f"faster_vit_{i}_224" for i in range(7)]
    assert registry.is_model_pretrained("faster_vit_0_224")
    m = fastervit_amd.create_model("faster_vit_0_224", depths=[1, 1, 1, 1], dim=16, in_dim=16, num_heads=[1, 1, 2, 4],
                                   num_classes=10)
    assert m.num_classes == 10 and m.head.out_features == 10
    assert m.pretrained_cfg["input_size"] == (3, 224, 224) and m.default_cfg is m.pretrained_cfg
    assert m.no_weight_decay_keywords() == {"rpb"}


def test_checkpoint_roundtrip(tmp_path):
    import fastervit_amd
    kw = dict(depths=[1, 1, 1, 1], dim=16, in_dim=16, num_heads=[1, 1, 2, 4])
    m = fastervit_amd.create_model("faster_vit_0_224", **kw)
    path = str(tmp_path / "ck.pth.tar")
    torch.save({"state_dict": {"module." + k: v for k, v in m.state_dict().items()}}, path)
    m2 = fastervit_amd.create_model("faster_vit_0_224", checkpoint_path=path, **kw)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    m3 = fastervit_amd.create_model("faster_vit_0_224", **kw)
    m3._load_state_dict(path, strict=True)
    assert torch.equal(m3.head.weight, m.head.weight)


def test_committed_pmc_traffic_file_covers_the_default_kernels():
    """bench.py fills roofline.traffic from the committed PMC passes (it cannot sample counters on itself); the file must have been
    produced by the CURRENT default path: a row for every HAT kernel family the FasterViT-0 deploy plan launches (r01: it went stale
    silently after a kernel was replaced)."""
    import json
    import bench
    path = os.path.join(ROOT, bench.PMC_FILE)
    assert os.path.exists(path), path
    rows = json.load(open(path))["kernels"]
    fams = {r["kernel"].split("<")[0] for r in rows}
    for fam in ("winmlp_kernel", "attnblk_kernel", "ctblk8_kernel", "winblk_kernel", "conv3x3_kernel", "conv3x3_c64_halo_kernel", "conv3x3_c128_band_kernel",
                "stem_fused_kernel"):
        assert fam in fams, f"{bench.PMC_FILE} has no row of {fam}: re-run scripts/gpu_r2_evidence.sh and copy the new file"
    dom = [r for r in rows if r["kernel"].startswith("winmlp_kernel<f16,256") and r["workgroups"] == 848]   # whole-batch launches (r06: two steps in flight; r04 / r05: 424 = 128-image shards)
    assert dom and dom[0]["hbm_traffic_mb"] > 0


def test_inference_runners_have_no_cpu_path_and_bench_times_steps_in_flight():
    """compile_inference / pipelined_inference refuse a CPU example (no fallback); bench.py's default launch structure is the r06 one: two whole-batch steps in
    flight (--inflight 2, one stream shard, no join), the r05 structure stays reachable by flags."""
    import fastervit_amd
    import bench
    m = fastervit_amd.create_model("faster_vit_0_224").eval()
    x = torch.zeros(2, 3, 224, 224)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.compile_inference(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.pipelined_inference(x, depth=2)
    old = sys.argv
    try:
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert (a.inflight, a.streams, a.join_from, a.batch, a.model) == (2, 1, 0, 256, "faster_vit_0_224")
        sys.argv = ["bench.py", "--inflight", "1", "--streams", "2", "--join-from", "3"]
        a = bench.parse()
        assert (a.inflight, a.streams, a.join_from) == (1, 2, 3)
    finally:
        sys.argv = old


def test_hat_backward_has_no_cpu_path():
    """fastervit_amd.hat_backward (sub-block backward on the HIP kernels) raises on CPU tensors instead of falling back."""
    from fastervit_amd import hat_backward
    x = torch.zeros(4, 256)
    with pytest.raises(RuntimeError, match="HIP device"):
        hat_backward.mlp_block_backward(x, x, x[0], x[0], torch.zeros(1024, 256), torch.zeros(1024), torch.zeros(256, 1024), torch.zeros(256), None, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        hat_backward.attn_block_backward(x, x, x[0], x[0], torch.zeros(768, 256), None, torch.zeros(256, 256), torch.zeros(256), None, None, 8, 4, None)


def test_enable_hat_backward_flags_and_cpu_behaviour():
    """model.enable_hat_backward() marks the transformer levels only; on CPU tensors the stages still raise (no CPU path), and switching it off restores
    the forward-only contract."""
    import fastervit_amd
    model = fastervit_amd.create_model("faster_vit_0_224").eval()
    assert not any(lvl.__dict__.get("hat_backward", False) for lvl in model.levels)
    assert model.enable_hat_backward(True) is model
    assert [bool(lvl.__dict__.get("hat_backward", False)) for lvl in model.levels] == [False, False, True, True]
    x = torch.randn(1, 3, 224, 224, requires_grad=True)
    with pytest.raises(RuntimeError):
        model(x)                       # HAT stages need the HIP device
    model.enable_hat_backward(False)
    assert not any(lvl.__dict__.get("hat_backward", False) for lvl in model.levels)
