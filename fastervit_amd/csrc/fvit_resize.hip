// Resize + crop + pad of a batch of decoded uint8 HWC images into a (B, 3, Ho, Wo) uint8 batch, one launch -- DESIGN.md section 14.
//
// Semantics are PIL's Image.resize (ImagingResample) for 8-bit images: separable, horizontal pass first, the result of each pass rounded and clamped
// to uint8 (t = clamp(floor(sum + 0.5), 0, 255)), an axis whose size does not change skipped.  Along one axis n_in -> n_out:
//   scale = n_in / n_out, fs = max(scale, 1), support = R fs (R = 1 bilinear, 2 bicubic with a = -0.5), c = (j + 0.5) scale,
//   k0 = max(0, trunc(c - support + 0.5)), k1 = min(n_in, trunc(c + support + 0.5)), w_k ~ f((k + 0.5 - c) / fs) normalised to sum 1.
// Both bounds and the filter argument are ratios of small integers ((2 j + 1) n_in, 2 n_out, ...): k0 / k1 come from integer division (32-bit when the numerators fit), so no tap
// appears or vanishes through rounding, and the filter argument is one fp64 division of an exact numerator.  Weights are evaluated and normalised in
// fp64 and rounded once to fp32 (a few hundred per workgroup: nothing beside the passes); the sums are fp32 fmaf chains in tap order: bitwise repeatable.
//
// Work split: a workgroup owns an 8 x 32 tile of ONE destination slot.  It builds the tap tables of its 32 columns and 8 rows in LDS, runs the horizontal
// pass from global memory for exactly the source rows its rows' vertical taps need (an LDS image of uint8 intermediates, RS_ROWS x 96 bytes), then the
// vertical pass out of LDS, and writes window bytes, fill bytes and the mask of its tile with adjacent lanes on adjacent bytes of the destination
// (channel fastest for a channels-last destination, column fastest otherwise).  The per-image descriptors are read from DEVICE memory: the host entry
// point never sees them, allocates nothing and does not synchronise, so a captured launch follows new source bytes and new descriptors.  A descriptor
// the kernel cannot serve (resize_reason != 0, the check the host query makes) turns its slot into fill + mask: no read through it, no out-of-slot write.
#include "fvit_common.h"

namespace fvit {
namespace {

constexpr int RS_TH = 8, RS_TW = 32;          // output tile (rows, columns) of one workgroup
constexpr int RS_MAXT = 66;                   // taps per output along one axis (a 16x bicubic downscale has 65)
constexpr int RS_WSTRIDE = RS_MAXT + 1;       // odd row stride of the weight tables: lanes on adjacent columns read distinct banks
constexpr int RS_ROWS = 192;                  // source rows of the uint8 intermediate image (8 output rows of a 16x bicubic downscale need 177)
constexpr int RS_ROWB = RS_TW * 3;            // bytes per intermediate row
constexpr int RS_THREADS = 256;
constexpr int RS_G = 7;                       // taps the horizontal pass gathers at a time (the classifier's 256 / 375 bicubic has up to 7)

__host__ __device__ inline int filter_radius(int filter) { return filter == FVIT_RESIZE_BICUBIC ? 2 : 1; }

// Both limits without a division (every workgroup evaluates them): floor(a / b) + 1 > k  <=>  a >= k b.
// most taps one output of the axis can have: k1 - k0 <= floor(2 support) + 1 = floor(2 R m / n_out) + 1
__host__ __device__ inline bool axis_taps_exceed(int64_t n_in, int64_t n_out, int R) {
    if (n_in == n_out) return false;
    const int64_t m = n_in > n_out ? n_in : n_out;
    return 2 * R * m >= (int64_t)RS_MAXT * n_out;
}
// most source rows RS_TH consecutive outputs of the axis span: floor((RS_TH - 1) scale + 2 support) + 1
__host__ __device__ inline bool axis_span_exceeds(int64_t n_in, int64_t n_out, int R) {
    if (n_in == n_out) return false;
    const int64_t m = n_in > n_out ? n_in : n_out;
    return (RS_TH - 1) * n_in + 2 * R * m >= (int64_t)RS_ROWS * n_out;
}

// 0, or why the kernel does not serve this descriptor for a slot of Ho x Wo (include/fvit_hip.h: FVIT_RESIZE_E*).  The same function on both sides.
__host__ __device__ inline int resize_reason(const FvitResizeDesc& d, int Ho, int Wo) {
    if (d.H < 1 || d.W < 1 || d.rh < 1 || d.rw < 1 || d.ch < 1 || d.cw < 1) return FVIT_RESIZE_ESIZE;
    if (d.filter != FVIT_RESIZE_BILINEAR && d.filter != FVIT_RESIZE_BICUBIC) return FVIT_RESIZE_EFILTER;
    if (d.top < 0 || d.left < 0 || (int64_t)d.top + d.ch > d.rh || (int64_t)d.left + d.cw > d.rw) return FVIT_RESIZE_EWINDOW;
    if (d.ch > Ho || d.cw > Wo) return FVIT_RESIZE_ESLOT;
    if (d.row_stride < 3 * (int64_t)d.W) return FVIT_RESIZE_ESTRIDE;
    const int R = filter_radius(d.filter);
    if (axis_taps_exceed(d.W, d.rw, R) || axis_taps_exceed(d.H, d.rh, R)) return FVIT_RESIZE_ETAPS;
    if (axis_span_exceeds(d.H, d.rh, R)) return FVIT_RESIZE_ELDS;
    return 0;
}

__device__ __forceinline__ double filter_value(double x, int R) {
    x = fabs(x);
    if (R == 1) return x < 1.0 ? 1.0 - x : 0.0;
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;            // Keys, a = -0.5
    if (x < 2.0) return -0.5 * (((x - 5.0) * x + 8.0) * x - 4.0);
    return 0.0;
}

// taps [k0, k0 + n) of output j and their normalised weights w[0 .. n)
__device__ __forceinline__ void axis_taps(int n_in, int n_out, int R, int j, int& k0, int& n, float* w) {
    if (n_in == n_out) { k0 = j; n = 1; w[0] = 1.0f; return; }   // the axis is skipped: the byte passes through (1.0f * p, rounded, is p)
    const int64_t m = n_in > n_out ? n_in : n_out;       // fs = m / n_out
    const int64_t cn = (int64_t)(2 * j + 1) * n_in;      // c = cn / (2 n_out)
    const int64_t den = 2 * (int64_t)n_out;
    const int64_t lo = cn - 2 * R * m + n_out;           // (c - support + 0.5) * den
    const int64_t hi = cn + 2 * R * m + n_out;           // (c + support + 0.5) * den, positive
    int64_t a, b;                                        // trunc of both
    if (hi < 0x7fffffffLL) {                             // (den < hi) the usual sizes: 32-bit divisions
        a = lo <= 0 ? 0 : (int64_t)((uint32_t)lo / (uint32_t)den);
        b = (int64_t)((uint32_t)hi / (uint32_t)den);
    } else {
        a = lo <= 0 ? 0 : lo / den;
        b = hi / den;
    }
    if (b > n_in) b = n_in;
    k0 = (int)a;
    n = (int)(b - a);
    if (n > RS_MAXT) n = RS_MAXT;                        // cannot happen for a descriptor resize_reason accepts
    const double inv = 1.0 / (double)(2 * m);            // (k + 0.5 - c) / fs = ((2 k + 1) n_out - cn) / (2 m)
    double ww = 0.0;
    for (int t = 0; t < n; ++t) ww += filter_value((double)((2 * (a + t) + 1) * n_out - cn) * inv, R);
    const double norm = ww != 0.0 ? 1.0 / ww : 1.0;
    for (int t = 0; t < n; ++t) w[t] = (float)(filter_value((double)((2 * (a + t) + 1) * n_out - cn) * inv, R) * norm);
}

__device__ __forceinline__ uint8_t round_u8(float s) {
    return (uint8_t)fminf(fmaxf(floorf(s + 0.5f), 0.0f), 255.0f);
}

struct ResizeArgs {
    const FvitResizeDesc* descs;   // [B], device memory
    uint8_t* dst;
    int64_t sb, sc, sh, sw;        // destination strides in bytes
    uint8_t* mask;                 // [B][Ho][Wo] bytes or null
    int Ho, Wo;
    int fill;
    int c_fastest;                 // the channel is the destination's densest axis (channels-last): lanes walk (x, c), otherwise (c, y, x)
};

__global__ __launch_bounds__(RS_THREADS) void resize_u8_kernel(const ResizeArgs a) {
    __shared__ float s_wx[RS_TW * RS_WSTRIDE];
    __shared__ float s_wy[RS_TH * RS_WSTRIDE];
    __shared__ int s_k0x[RS_TW], s_nx[RS_TW], s_k0y[RS_TH], s_ny[RS_TH];
    __shared__ uint8_t s_t[RS_ROWS * RS_ROWB];

    const int tid = threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * RS_TH, x0 = blockIdx.x * RS_TW;
    const FvitResizeDesc d = a.descs[b];
    const int th = min(RS_TH, a.Ho - y0), tw = min(RS_TW, a.Wo - x0);
    const bool ok = d.src != nullptr && resize_reason(d, a.Ho, a.Wo) == 0;
    const int nvy = ok ? max(0, min(th, d.ch - y0)) : 0;   // rows and columns of the tile that lie in the window
    const int nvx = ok ? max(0, min(tw, d.cw - x0)) : 0;
    int rowbase = 0, nrows = 0;

    if (nvy > 0 && nvx > 0) {   // uniform over the workgroup
        const int R = filter_radius(d.filter);
        if (tid < nvx) {
            int k0, n;
            axis_taps(d.W, d.rw, R, d.left + x0 + tid, k0, n, s_wx + tid * RS_WSTRIDE);
            s_k0x[tid] = k0;
            s_nx[tid] = n;
        } else if (tid >= 64 && tid < 64 + nvy) {
            const int y = tid - 64;
            int k0, n;
            axis_taps(d.H, d.rh, R, d.top + y0 + y, k0, n, s_wy + y * RS_WSTRIDE);
            s_k0y[y] = k0;
            s_ny[y] = n;
        }
        __syncthreads();
        // k0 and k0 + n do not decrease with the output index: the tile's rows need source rows [k0 of the first, k0 + n of the last)
        rowbase = s_k0y[0];
        nrows = min(s_k0y[nvy - 1] + s_ny[nvy - 1] - rowbase, RS_ROWS);

        // horizontal pass: (source row, tile column) -> three uint8 intermediates
        const uint8_t* src = (const uint8_t*)d.src + (int64_t)rowbase * d.row_stride;
        for (int e = tid; e < nrows * RS_TW; e += RS_THREADS) {
            const int r = e / RS_TW, x = e - r * RS_TW;
            if (x >= nvx) continue;
            const float* w = s_wx + x * RS_WSTRIDE;
            const int n = s_nx[x];
            // the 3 n bytes of the taps, read as the aligned dwords that hold them (an index past the last dword with a needed byte is clamped to it: no
            // access leaves the pages of the needed bytes) and cut into pixels with v_alignbyte.  RS_G taps at a time: their 21 bytes, starting at
            // byte o <= 3 of the first dword, lie in six dwords, loaded together (independent loads, one wait) into registers with static indices.
            const uintptr_t addr = (uintptr_t)(src + (int64_t)r * d.row_stride + (int64_t)s_k0x[x] * 3);
            const uint32_t* wp = (const uint32_t*)(addr & ~(uintptr_t)3);
            int o = (int)(addr & 3), wbase = 0;
            const int last = (o + 3 * n - 1) >> 2;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int t0 = 0; t0 < n; t0 += RS_G) {
                uint32_t wd[7];
#pragma unroll
                for (int k = 0; k < 6; ++k) wd[k] = wp[min(wbase + k, last)];
                wd[6] = wd[5];   // only ever the unused fourth byte of the last pixel
#pragma unroll
                for (int t = 0; t < RS_G; ++t) {
                    if (t0 + t < n) {
                        const int ob = o + 3 * t, ia = (3 * t) >> 2;   // the pixel starts in dword ia (o + (3 t & 3) < 4) or ia + 1
                        const bool up = (ob >> 2) != ia;
                        const uint32_t lo = up ? wd[ia + 1] : wd[ia], hi = up ? wd[ia + 2] : wd[ia + 1];
                        const uint32_t px = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(ob & 3));
                        const float wt = w[t0 + t];
                        s0 = fmaf(wt, (float)(px & 255u), s0);
                        s1 = fmaf(wt, (float)((px >> 8) & 255u), s1);
                        s2 = fmaf(wt, (float)((px >> 16) & 255u), s2);
                    }
                }
                o += 3 * RS_G;
                wbase += o >> 2;
                o &= 3;
            }
            uint8_t* q = s_t + r * RS_ROWB + x * 3;
            q[0] = round_u8(s0);
            q[1] = round_u8(s1);
            q[2] = round_u8(s2);
        }
        __syncthreads();
    }

    // vertical pass out of LDS for the window's bytes, fill for the rest of the tile, and the tile's mask
    const uint8_t fill = (uint8_t)a.fill;
    uint8_t* dst = a.dst + (int64_t)b * a.sb + (int64_t)y0 * a.sh + (int64_t)x0 * a.sw;
    uint8_t* mask = a.mask ? a.mask + ((int64_t)b * a.Ho + y0) * a.Wo + x0 : nullptr;
    for (int e = tid; e < RS_TH * RS_TW * 3; e += RS_THREADS) {   // the full tile's index space (constant divisors); a ragged tile idles some lanes
        int c, y, x;
        if (a.c_fastest) {
            y = e / RS_ROWB;
            const int rem = e - y * RS_ROWB;
            x = rem / 3;
            c = rem - x * 3;
        } else {
            c = e / (RS_TH * RS_TW);
            const int rem = e - c * (RS_TH * RS_TW);
            y = rem / RS_TW;
            x = rem - y * RS_TW;
        }
        if (y >= th || x >= tw) continue;
        const bool inside = y < nvy && x < nvx;
        uint8_t v = fill;
        if (inside) {
            const int n = s_ny[y];
            const int r0 = s_k0y[y] - rowbase;
            const float* w = s_wy + y * RS_WSTRIDE;
            const uint8_t* q = s_t + r0 * RS_ROWB + x * 3 + c;
            float s = 0.f;
            for (int t = 0; t < n && r0 + t < nrows; ++t) s = fmaf(w[t], (float)q[t * RS_ROWB], s);
            v = round_u8(s);
        }
        dst[(int64_t)c * a.sc + (int64_t)y * a.sh + (int64_t)x * a.sw] = v;
        if (mask && c == 0) mask[(int64_t)y * a.Wo + x] = inside ? 0 : 1;
    }
}

const char* reason_text(int rc) {
    switch (rc) {
        case FVIT_RESIZE_ESIZE: return "size: H, W, rh, rw, ch and cw must all be >= 1";
        case FVIT_RESIZE_EFILTER: return "filter: unknown filter code (FVIT_RESIZE_BILINEAR or FVIT_RESIZE_BICUBIC)";
        case FVIT_RESIZE_EWINDOW: return "window: the window (top, left, ch, cw) does not lie inside the resized image";
        case FVIT_RESIZE_ESLOT: return "slot: the window is larger than the destination slot";
        case FVIT_RESIZE_ESTRIDE: return "stride: the source row stride is smaller than 3 W bytes";
        case FVIT_RESIZE_ETAPS: return "tap limit: more than 66 taps per output (a downscale beyond 16x bicubic / 32x bilinear on one axis)";
        case FVIT_RESIZE_ELDS: return "LDS limit: the source rows of one 8-row output tile exceed the 192-row intermediate image";
        default: return "unknown reason";
    }
}

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" {

int fvit_image_resize_check(const FvitResizeDesc* desc, int32_t Ho, int32_t Wo) {
    if (!desc || Ho < 1 || Wo < 1) { set_error("image_resize_check: null descriptor or Ho=%d Wo=%d < 1", Ho, Wo); return FVIT_EINVAL; }
    const int rc = resize_reason(*desc, Ho, Wo);
    if (rc != 0)
        set_error("image_resize: %s (H=%d W=%d stride=%lld -> rh=%d rw=%d, window top=%d left=%d ch=%d cw=%d, filter=%d, slot %dx%d)", reason_text(rc),
                  desc->H, desc->W, (long long)desc->row_stride, desc->rh, desc->rw, desc->top, desc->left, desc->ch, desc->cw, desc->filter, Ho, Wo);
    return rc;
}

int fvit_image_resize_u8(const FvitResizeDesc* descs, int32_t B, const FvitMapView* out, int32_t Ho, int32_t Wo, int32_t fill, void* mask,
                         fvit_stream_t stream) {
    if (!descs || !out || !out->data || B < 1 || Ho < 1 || Wo < 1) {
        set_error("image_resize_u8: bad arguments B=%d Ho=%d Wo=%d (or a null pointer)", B, Ho, Wo);
        return FVIT_EINVAL;
    }
    if (out->dtype != FVIT_U8) { set_error("image_resize_u8: the destination view must be FVIT_U8 (dtype code %d given)", out->dtype); return FVIT_EINVAL; }
    if (out->stride_c < 1 || out->stride_h < 1 || out->stride_w < 1 || (B > 1 && out->stride_b < 1)) {
        set_error("image_resize_u8: destination strides must be positive (b=%lld c=%lld h=%lld w=%lld)", (long long)out->stride_b,
                  (long long)out->stride_c, (long long)out->stride_h, (long long)out->stride_w);
        return FVIT_EINVAL;
    }
    if (fill < 0 || fill > 255) { set_error("image_resize_u8: fill=%d is not a uint8 value", fill); return FVIT_EINVAL; }
    const int64_t tx = (Wo + RS_TW - 1) / RS_TW, ty = (Ho + RS_TH - 1) / RS_TH;
    if (B > 65535 || ty > 65535) { set_error("image_resize_u8: B=%d or Ho=%d is more than one launch covers (65535 slots, 524280 rows)", B, Ho); return FVIT_EINVAL; }
    ResizeArgs a = {};
    a.descs = descs;
    a.dst = (uint8_t*)out->data;
    a.sb = out->stride_b; a.sc = out->stride_c; a.sh = out->stride_h; a.sw = out->stride_w;
    a.mask = (uint8_t*)mask;
    a.Ho = Ho; a.Wo = Wo;
    a.fill = fill;
    a.c_fastest = out->stride_c < out->stride_w ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const double slot = (double)B * Ho * Wo;
    ProfScope prof(FVIT_K_OTHER, 0.0, slot * (mask ? 4.0 : 3.0), st);   // the source bytes are known to the device alone
    hipLaunchKernelGGL(resize_u8_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)B), dim3(RS_THREADS), 0, st, a);
    prof_note("resize_u8_kernel", (int)(tx * ty * B));
    return check_launch("resize_u8_kernel");
}

}  // extern "C"
