// fvit_conv.hip -- the driver of the 3x3 convolutions (pad 1, stride 1 or 2) on channels-last 16-bit maps, gfx950.  choose_conv_route is the only place
// that asks which kernel runs a 3x3 conv and the only reader of the route knobs; run_conv hands the answer to the launch function of the kernel's unit
// (fvit_conv_halo.hip, fvit_conv_band.hip, fvit_conv_gemm.hip: no kernel lives here).  Every entry point below fills a FvitConvWeights / FvitConvCall for it.
#include "fvit_conv.h"

namespace fvit {
namespace {

constexpr ConvRouteInfo kConvRoutes[CR_COUNT] = {
    {"conv3x3_c64_halo_kernel", 0, 0},         {"conv3x3_c64_halo_kernel<ln>", 0, 0},
    {"conv3x3_c128_band_kernel", 0, 0},        {"conv3x3_c128_band_kernel<ln>", 0, 0},
    {"conv3x3_kernel<2,2,4,patch>", 128, 128}, {"conv3x3_kernel<2,2,4,px,patch>", 128, 128},
    {"conv3x3_kernel<2,2,4>", 128, 128},       {"conv3x3_kernel<2,2,4,dense>", 128, 128},
    {"conv3x3_kernel<2,2,4,px>", 128, 128},    {"conv3x3_kernel<2,2,4,px,dense>", 128, 128},
    {"conv3x3_kernel<2,2,2>", 128, 64},        {"conv3x3_kernel<2,2,2,dense>", 128, 64},
    {"conv3x3_kernel<2,2,2,px>", 128, 64},     {"conv3x3_kernel<2,2,2,px,dense>", 128, 64},
    {"conv3x3_kernel<4,1,4>", 256, 64},
};
inline bool route_is_ln(int r) { return r == CR_HALO64_LN || r == CR_BAND128_LN; }

// The knobs that select a route, read once per call: fvit_tune takes effect from the next call on, nothing is cached
struct ConvKnobs {
    int halo = tune_get("conv_halo", 1), band = tune_get("conv_band", 1);
    int patch = tune_get("conv_patch", 1), patch_max_waste_pct = tune_get("conv_patch_max_waste_pct", 10);
    int n128_ragged = tune_get("conv_n128_ragged", 1), narrow = tune_get("conv128_narrow", 0), variant64 = tune_get("conv64_variant", 0);
};

// Argument validation of every conv entry point (`who` names it in the messages); data pointers are tested, never dereferenced.
int validate_conv(const char* who, int32_t dtype, const FvitConvWeights* w, const FvitConvCall* c) {
    if (!w || !c) { set_error("%s: null weights or call", who); return FVIT_EINVAL; }
    const bool px = call_is_px(*c);
    if (!c->in || !(w->classic || w->dense || w->band_frag) || (!c->out && !c->out_f32) || !c->zeros || c->B <= 0 || c->Hi <= 0 || c->Wi <= 0 ||
        c->Cin <= 0 || c->Cout <= 0 || (c->Cin % 64) || (c->Cout % 64) || (c->stride != 1 && c->stride != 2) || c->act < 0 || c->act > 2 ||
        (w->terms != 1 && w->terms != 2) || (c->in_lo && w->terms != 2) || (c->residual_lo && !c->residual) || (c->out_f32 && c->out_lo) ||
        (c->out_lo && !c->out)) {
        set_error("%s: unsupported arguments Cin=%d Cout=%d stride=%d act=%d weight_terms=%d (need Cin %% 64 == 0, Cout %% 64 == 0, stride 1|2, "
                  "weight_terms 2 with a two-term input, out or out_f32)", who, c->Cin, c->Cout, c->stride, c->act, w->terms);
        return FVIT_EINVAL;
    }
    if (w->cin_valid != c->Cin && (w->cin_valid <= 0 || w->cin_valid > c->Cin || (w->cin_valid % 8))) {
        set_error("%s: cin_valid=%d must be a multiple of 8 in (0, Cin=%d]", who, w->cin_valid, c->Cin);
        return FVIT_EINVAL;
    }
    const int64_t M = (int64_t)c->B * out_size(c->Hi, c->stride) * out_size(c->Wi, c->stride);
    if (M > 0x7fffffff) {
        set_error("%s: %lld output pixels exceed the 32-bit row index", who, (long long)M);
        return FVIT_EINVAL;
    }
    if (c->ln_w && (!c->ln_b || !c->residual || c->stride != 1 || c->act != 0 || px)) {
        set_error("%s: the LayerNorm2d epilogue needs ln_w and ln_b, a residual, stride 1, no activation and 16-bit maps", who);
        return FVIT_EINVAL;
    }
    if (dtype != FVIT_F16 && dtype != FVIT_BF16) {
        set_error("%s: dtype %d not supported (16-bit %s only)", who, dtype, px ? "planes" : "maps");
        return FVIT_EINVAL;
    }
    return FVIT_OK;
}

// The route of a validated call, or CR_NONE with the error message set.  Pure host code.  A route is eligible only if the image it reads is in `w`;
// with the LayerNorm2d parameters set the answer is an <ln> route where a kernel has that epilogue for the shape and the plain route otherwise.
ConvRoute choose_conv_route(const FvitConvCall& c, const FvitConvWeights& w, const ConvKnobs& k) {
    const int Ho = out_size(c.Hi, c.stride), Wo = out_size(c.Wi, c.stride);
    const int64_t M = (int64_t)c.B * Ho * Wo;
    const bool px = call_is_px(c), ln = c.ln_w != nullptr;
    const bool padded = w.cin_valid != c.Cin;   // the map carries pad channels, which only the dense rows leave out of the contraction
    const bool plain16 = c.stride == 1 && w.terms == 1 && !px && !padded;   // what the two single-purpose kernels take
    if (c.Cin == 64 && c.Cout == 64 && plain16 && w.classic && k.halo)
        return ln && M * 64 <= 0x7fffffff ? CR_HALO64_LN : CR_HALO64;
    // level 1 of FasterViT-0: one row band of an image per workgroup, weights streamed in fragment order
    if (c.Cin == 128 && c.Cout == 128 && plain16 && w.band_frag && k.band && band_supported(c.Hi, c.Wi) && M * 128 <= 0x7fffffff)
        return ln ? CR_BAND128_LN : CR_BAND128;
    // 128-column tiles.  r05 (fvit_tune "conv_n128_ragged", default 1): Cout % 128 == 64 (FasterViT-4: 448 / 832 / 1600 padded channels) also takes them, with
    // a RAGGED last N tile (weight rows clamped, the missing 64 channels never stored: 1 / (2 n) of the MFMAs wasted) instead of 128 x 64 tiles: half the
    // workgroups, each weight byte staged for 128 pixels feeds twice the MFMAs, and the weight matrix -- 7.2 MB with two terms at 448 channels, more than an
    // XCD's 4 MB L2 -- is re-streamed from the Infinity Cache per ROUND of resident workgroups: 3 rounds instead of 11 (PMC: 580 MB read per launch)
    const bool n128 = c.Cout % 128 == 0 || (c.Cout > 128 && k.n128_ragged);
    // 128x128 tiles run two workgroups per CU (64 KiB LDS): 512 slots.  A grid just above a multiple of 512 pays a whole extra
    // round for a handful of tiles (527 tiles at 86 images of 28x28: 2 rounds, 42 us, of which one full round for 15 tiles).
    // 128x64 tiles (48 KiB, three per CU: 768 slots) do half the MFMA work per workgroup and soften that cliff in isolation
    // (40.6 vs 44 us at 85-86 images, but 41 vs 30 us at 83), yet end to end they lose (68.1k vs 70.0k images/s: the other stream
    // shards' kernels fill the idle slots of a partial round anyway) => "conv128_narrow" is an opt-in knob only.
    // r06: 8 x 16 output patches with the 10 x 18 halo of a 64-channel chunk in LDS (conv3x3_kernel<.., HALO>): stride 1, classic rows, 128-column tiles, 32-bit
    // element offsets of the halo rows; only where the patch grid wastes little ("conv_patch_max_waste_pct"): call 31, two interleaved rounds -- any-res
    // 576 x 960 (144 x 240 and 72 x 120 maps: 0 / 6.7 % waste) +1.9 % (16-bit plan) / +2.4 % (precise plan); FasterViT-4 224 (56 x 56: 14 % waste, and the
    // classic 36 K steps where the dense-K form walks 29) equal / -0.6 %: stays on the dense-K form
    if (w.classic && k.patch && c.stride == 1 && c.Cout >= 128 && n128 && !k.narrow && (int64_t)c.B * c.Hi * c.Wi * c.Cin < 0x7fffffffLL) {
        const int64_t tiles = (int64_t)c.B * ((Ho + PATCH_H - 1) / PATCH_H) * ((Wo + PATCH_W - 1) / PATCH_W);
        if (tiles * 128 * 100 <= M * (100 + k.patch_max_waste_pct)) return px ? CR_PATCH_PX : CR_PATCH;
    }
    const bool dense = padded && w.dense;
    if (!dense && !w.classic) {
        set_error("conv3x3: no kernel for Cin=%d Cout=%d stride=%d on a %d x %d map reads the weight images given (classic%s rows needed)", c.Cin, c.Cout,
                  c.stride, c.Hi, c.Wi, padded ? " or dense" : "");
        return CR_NONE;
    }
    if (px) return ConvRoute((n128 ? CR_T128_PX : CR_T64_PX) + dense);   // two-term maps: the implicit GEMM only (128 x 128 tiles when Cout allows)
    if (n128 && !k.narrow) return ConvRoute(CR_T128 + dense);
    return k.variant64 == 1 && !dense ? CR_T256X64 : ConvRoute(CR_T64 + dense);
}

// Launches route `r` (from choose_conv_route) of a validated call.  stamps: fvit_debug_conv_band_timeline (CR_BAND128, fp16).
int run_conv(int32_t dtype, ConvRoute r, const FvitConvCall& c, const FvitConvWeights& w, fvit_stream_t stream, void* stamps = nullptr) {
    const char* name = kConvRoutes[r].name;
    if (r == CR_HALO64 || r == CR_HALO64_LN) return launch_conv_halo(dtype, route_is_ln(r), name, c, w, (hipStream_t)stream);
    if (r == CR_BAND128 || r == CR_BAND128_LN) return launch_conv_band(dtype, route_is_ln(r), name, c, w, (hipStream_t)stream, stamps);
    return launch_conv_gemm(dtype, r, kConvRoutes[r], c, w, (hipStream_t)stream);
}

// validate and choose, then launch (`run`: FVIT_OK or a negative error) or answer the route (>= 0, or a negative error)
int conv_entry(int32_t dtype, const FvitConvWeights* w, const FvitConvCall* c, bool run, fvit_stream_t stream) {
    const char* who = c && call_is_px(*c) ? "conv3x3_px" : "conv3x3";
    if (const int rc = validate_conv(who, dtype, w, c)) return rc;
    const ConvRoute r = choose_conv_route(*c, *w, ConvKnobs{});
    if (r == CR_NONE) return FVIT_EINVAL;
    if (!run) return r;
    if (c->ln_w && !route_is_ln(r)) {
        set_error("%s: %s has no LayerNorm2d epilogue (ask fvit_conv3x3_route first and run the LayerNorm2d pass apart)", who, kConvRoutes[r].name);
        return FVIT_EINVAL;
    }
    return run_conv(dtype, r, *c, *w, stream);
}

// the structs of an entry point that is given ONE weight image
FvitConvCall one_call(const void* in, const float* bias, const void* residual, void* out, const void* zeros, int B, int Hi, int Wi, int Cin, int Cout,
                      int stride, int act) {
    FvitConvCall c{};
    c.in = in; c.bias = bias; c.residual = residual; c.out = out; c.zeros = zeros;
    c.B = B; c.Hi = Hi; c.Wi = Wi; c.Cin = Cin; c.Cout = Cout; c.stride = stride; c.act = act;
    return c;
}
int one_image_conv(int32_t dtype, FvitConvCall c, const void* weight, int cin_valid, int terms, fvit_stream_t stream) {
    FvitConvWeights w{};
    (cin_valid == c.Cin ? w.classic : w.dense) = weight;
    w.terms = terms; w.cin_valid = cin_valid;
    return conv_entry(dtype, &w, &c, true, stream);
}
// the row-band / LayerNorm2d entry points name their kernel (`want`): its knob does not switch them off, any other route is their FVIT_EINVAL
int named_conv(const char* who, const char* need, int32_t dtype, FvitConvCall c, const void* classic, const void* band_frag, ConvRoute want, const float* ln_w,
               const float* ln_b, float eps, fvit_stream_t stream, void* stamps = nullptr) {
    const FvitConvWeights w{classic, nullptr, band_frag, 1, c.Cin};
    c.ln_w = ln_w; c.ln_b = ln_b; c.ln_eps = eps;
    ConvKnobs k;
    k.halo = k.band = 1;
    if (validate_conv(who, dtype, &w, &c) == FVIT_OK && choose_conv_route(c, w, k) == want) return run_conv(dtype, want, c, w, stream, stamps);
    if (dtype == FVIT_F16 || dtype == FVIT_BF16) set_error("%s: unsupported arguments B=%d H=%d W=%d act=%d (need %s)", who, c.B, c.Hi, c.Wi, c.act, need);
    return FVIT_EINVAL;
}

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" int fvit_conv3x3(int32_t dtype, const FvitConvWeights* weights, const FvitConvCall* call, fvit_stream_t stream) { return conv_entry(dtype, weights, call, true, stream); }

extern "C" int fvit_conv3x3_route(int32_t dtype, const FvitConvWeights* weights, const FvitConvCall* call) { return conv_entry(dtype, weights, call, false, nullptr); }

extern "C" const char* fvit_conv3x3_route_name(int route) { return route >= 0 && route < CR_COUNT ? kConvRoutes[route].name : "?"; }

extern "C" int fvit_conv3x3_dense_k(int32_t cin_valid) { return cin_valid > 0 && cin_valid % 8 == 0 ? (9 * cin_valid + BK - 1) / BK * BK : -1; }

extern "C" int fvit_conv3x3_nhwc(int32_t dtype, const void* in, const void* weight, const float* bias, const void* residual, void* out,
                                 int32_t B, int32_t Hi, int32_t Wi, int32_t Cin, int32_t Cout, int32_t stride, int32_t act,
                                 const void* zeros, fvit_stream_t stream) {
    return one_image_conv(dtype, one_call(in, bias, residual, out, zeros, B, Hi, Wi, Cin, Cout, stride, act), weight, Cin, 1, stream);
}

extern "C" int fvit_conv3x3_nhwc_terms(int32_t dtype, const void* in, const void* weight, const float* bias, const void* residual, void* out,
                                       int32_t B, int32_t Hi, int32_t Wi, int32_t Cin, int32_t Cout, int32_t stride, int32_t act,
                                       int32_t weight_terms, const void* zeros, fvit_stream_t stream) {
    return one_image_conv(dtype, one_call(in, bias, residual, out, zeros, B, Hi, Wi, Cin, Cout, stride, act), weight, Cin, weight_terms, stream);
}

extern "C" int fvit_conv3x3_nhwc_dense(int32_t dtype, const void* in, const void* weight, const float* bias, const void* residual, void* out,
                                       int32_t B, int32_t Hi, int32_t Wi, int32_t Cin, int32_t cin_valid, int32_t Cout, int32_t stride, int32_t act,
                                       int32_t weight_terms, const void* zeros, fvit_stream_t stream) {
    return one_image_conv(dtype, one_call(in, bias, residual, out, zeros, B, Hi, Wi, Cin, Cout, stride, act), weight, cin_valid, weight_terms, stream);
}

extern "C" int fvit_conv3x3_nhwc_px_dense(int32_t dtype, const void* in, const void* in_lo, const void* weight, const float* bias, const void* residual,
                                          const void* residual_lo, void* out, void* out_lo, float* out_f32, int32_t B, int32_t Hi, int32_t Wi, int32_t Cin,
                                          int32_t cin_valid, int32_t Cout, int32_t stride, int32_t act, int32_t weight_terms, const void* zeros,
                                          fvit_stream_t stream) {
    FvitConvCall c = one_call(in, bias, residual, out, zeros, B, Hi, Wi, Cin, Cout, stride, act);
    c.in_lo = in_lo; c.residual_lo = residual_lo; c.out_lo = out_lo; c.out_f32 = out_f32; c.px = 1;
    return one_image_conv(dtype, c, weight, cin_valid, weight_terms, stream);
}

extern "C" int fvit_conv3x3_nhwc_px(int32_t dtype, const void* in, const void* in_lo, const void* weight, const float* bias, const void* residual,
                                    const void* residual_lo, void* out, void* out_lo, float* out_f32, int32_t B, int32_t Hi, int32_t Wi, int32_t Cin,
                                    int32_t Cout, int32_t stride, int32_t act, int32_t weight_terms, const void* zeros, fvit_stream_t stream) {
    return fvit_conv3x3_nhwc_px_dense(dtype, in, in_lo, weight, bias, residual, residual_lo, out, out_lo, out_f32, B, Hi, Wi, Cin, Cin, Cout, stride, act,
                                      weight_terms, zeros, stream);
}

// given classic rows, does the driver take the patch form for this shape?  (Any non-null address stands for the image.)
extern "C" int fvit_conv3x3_patch_form(int32_t B, int32_t Hi, int32_t Wi, int32_t Cin, int32_t Cout, int32_t stride) {
    const FvitConvWeights w{&w, nullptr, nullptr, 2, Cin};
    const FvitConvCall c = one_call(&w, nullptr, nullptr, (void*)&w, &w, B, Hi, Wi, Cin, Cout, stride, 0);
    return conv_entry(FVIT_F16, &w, &c, false, nullptr) == CR_PATCH ? 1 : 0;
}

extern "C" int fvit_conv3x3_c128_band_supported(int32_t H, int32_t W) {
    const FvitConvWeights w{nullptr, nullptr, &w, 1, 128};
    const FvitConvCall c = one_call(&w, nullptr, nullptr, (void*)&w, &w, 1, H, W, 128, 128, 1, 0);
    return conv_entry(FVIT_F16, &w, &c, false, nullptr) == CR_BAND128 ? 1 : 0;
}

extern "C" int fvit_conv3x3_c128_band(int32_t dtype, const void* in, const void* w_frag, const float* bias, const void* residual, void* out,
                                      int32_t B, int32_t H, int32_t W, int32_t act, const void* zeros, fvit_stream_t stream) {
    return named_conv("conv3x3_c128_band", "W <= 30", dtype, one_call(in, bias, residual, out, zeros, B, H, W, 128, 128, 1, act), nullptr, w_frag, CR_BAND128,
                      nullptr, nullptr, 0.f, stream);
}

extern "C" int fvit_conv3x3_c64_ln2d(int32_t dtype, const void* in, const void* weight, const float* bias, const void* residual, void* out,
                                     const float* ln_w, const float* ln_b, float eps, int32_t B, int32_t H, int32_t W, const void* zeros,
                                     fvit_stream_t stream) {
    return named_conv("conv3x3_c64_ln2d", "a residual and LayerNorm2d parameters", dtype, one_call(in, bias, residual, out, zeros, B, H, W, 64, 64, 1, 0), weight,
                      nullptr, CR_HALO64_LN, ln_w, ln_b, eps, stream);
}

extern "C" int fvit_conv3x3_c128_band_ln2d(int32_t dtype, const void* in, const void* w_frag, const float* bias, const void* residual, void* out,
                                           const float* ln_w, const float* ln_b, float eps, int32_t B, int32_t H, int32_t W, const void* zeros,
                                           fvit_stream_t stream) {
    return named_conv("conv3x3_c128_band_ln2d", "a residual, LayerNorm2d parameters and W <= 30", dtype,
                      one_call(in, bias, residual, out, zeros, B, H, W, 128, 128, 1, 0), nullptr, w_frag, CR_BAND128_LN, ln_w, ln_b, eps, stream);
}

// diagnosis: the fp16 row-band kernel with s_memtime stamps, u64 [B * bands][4 waves][8] (see BandParams.ts); bands = ceil(H / (224 / (W + 2)))
#ifdef FVIT_DIAG
extern "C" int fvit_debug_conv_band_timeline(const void* in, const void* w_frag, const float* bias, const void* residual, void* out, int32_t B,
                                             int32_t H, int32_t W, int32_t act, const void* zeros, void* stamps, fvit_stream_t stream) {
    if (!stamps) { set_error("debug_conv_band_timeline: null stamp buffer"); return FVIT_EINVAL; }
    return named_conv("debug_conv_band_timeline", "W <= 30", FVIT_F16, one_call(in, bias, residual, out, zeros, B, H, W, 128, 128, 1, act), nullptr, w_frag,
                      CR_BAND128, nullptr, nullptr, 0.f, stream, stamps);
}
#endif  // FVIT_DIAG
