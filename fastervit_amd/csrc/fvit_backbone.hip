// fvit_backbone.hip -- the two memory-bound passes of the multi-scale detection backbone (fastervit_amd/models/backbone.py):
//   * fvit_token_init_dyn : TokenInitializer of the detection variant (DINO fastervit.py:542-592): depthwise 3x3 + bias, average pool with
//                           kernel / stride derived from the padded map on each call, zero pad to a multiple of ct_size, and the raw
//                           NCHW -> (Hq*Wq, C) reshape (no permute) of that module.  One workgroup per (image, channel) plane: the conv
//                           output plane is staged in LDS, the overlapping pool windows read it from there, the pooled plane is written
//                           contiguously (that IS the (B, G, C) row order of the reference reshape).
//   * fvit_feature_tap    : crop + folded eval BatchNorm2d + contiguous NCHW fp32 of one pre-downsample stage map (fastervit.py:835-838),
//                           from any strided view (NCHW, channels_last, a crop of a padded map).  32-channel x 64-pixel tiles through LDS, so
//                           that both the read (along whichever of C / W is unit-stride) and the NCHW write are coalesced.
// and their backwards (fastervit_amd/hat_backward.py: the backbone as a trainable model), fp32, no atomics, fixed summation order:
//   * fvit_token_init_dyn_backward : one workgroup per (image, channel) plane again: the gradient of the conv output (the adjoint of the overlapping
//                           average pool) is staged in LDS, every thread then forms dx of its pixels (the 3x3 correlation with the flipped weight)
//                           and its share of the 9 weight gradients from the same nine LDS values; per-plane partials [10], summed over the images
//                           in order by a second launch.
//   * fvit_feature_tap_backward    : the forward's 32-channel x 64-pixel tiles: dout (NCHW) and x (its own layout) go through LDS, dx is written in
//                           x's layout, the per-channel sums of dout and dout * x are reduced per tile row by one wave and finished by a second launch.
#include "fvit_common.h"

namespace fvit {

namespace {

constexpr int kTokLdsFloats = 16384;   // 64 KiB: conv-output planes up to 16384 pixels (a 128 x 128 stage-2 map, ~2048 x 2048 images)

template <typename IN>
__device__ __forceinline__ float ld_map(const IN* p, int64_t off) { return (float)p[off]; }

struct TokDynParams {
    FvitMapView in;
    const float* w;      // [C][9]
    const float* bias;   // [C]
    float* out;          // (B, C, Hq, Wq) contiguous == the reference's (B, Hq*Wq, C) reshape
    int B, C, Hp, Wp, kh, kw, sh, sw, Ho, Wo, Hq, Wq;
    float inv_area;
};

template <typename IN>
__global__ __launch_bounds__(256) void token_init_dyn_kernel(TokDynParams p) {
    __shared__ float conv[kTokLdsFloats];
    const int plane = blockIdx.x;            // b * C + c
    const int c = plane % p.C, b = plane / p.C;
    const IN* __restrict__ src = (const IN*)p.in.data + (int64_t)b * p.in.stride_b + (int64_t)c * p.in.stride_c;
    float wv[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) wv[j] = p.w[c * 9 + j];
    const float bv = p.bias[c];
    const int npix = p.Hp * p.Wp;
    // depthwise 3x3, zero padding 1 (threads walk the plane along W: unit-stride reads for NCHW maps)
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / p.Wp, x = i - y * p.Wp;
        float acc = bv;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y + ky - 1;
            if (yy < 0 || yy >= p.Hp) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x + kx - 1;
                if (xx < 0 || xx >= p.Wp) continue;
                acc += wv[ky * 3 + kx] * ld_map(src, (int64_t)yy * p.in.stride_h + (int64_t)xx * p.in.stride_w);
            }
        }
        conv[i] = acc;
    }
    __syncthreads();
    // average pool (padding 0, floor mode: divisor kh * kw) + zero pad to Hq x Wq
    float* __restrict__ dst = p.out + (int64_t)plane * p.Hq * p.Wq;
    const int nq = p.Hq * p.Wq;
    for (int i = threadIdx.x; i < nq; i += blockDim.x) {
        const int oy = i / p.Wq, ox = i - oy * p.Wq;
        float s = 0.f;
        if (oy < p.Ho && ox < p.Wo) {
            const int y0 = oy * p.sh, x0 = ox * p.sw;
            for (int dy = 0; dy < p.kh; ++dy) {
                const float* row = conv + (y0 + dy) * p.Wp + x0;
                for (int dx = 0; dx < p.kw; ++dx) s += row[dx];
            }
            s *= p.inv_area;
        }
        dst[i] = s;
    }
}

struct TapParams {
    FvitMapView in;
    const float* scale;   // [C]
    const float* shift;   // [C]
    float* out;           // (B, C, H, W) contiguous
    int B, C, H, W, ctiles, wtiles;
    int c_fast;           // the view is unit-stride along C (channels_last): read with lanes along C
};

template <typename IN>
__global__ __launch_bounds__(256) void feature_tap_kernel(TapParams p) {
    __shared__ float tile[32][65];
    int t = blockIdx.x;
    const int wt = t % p.wtiles; t /= p.wtiles;
    const int ct = t % p.ctiles; t /= p.ctiles;
    const int h = t % p.H, b = t / p.H;
    const int c0 = ct * 32, w0 = wt * 64;
    const IN* __restrict__ src = (const IN*)p.in.data + (int64_t)b * p.in.stride_b + (int64_t)h * p.in.stride_h;
    if (p.c_fast) {
        const int cl = threadIdx.x & 31;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int wl = (threadIdx.x >> 5) + 8 * k;
            const int cc = c0 + cl, ww = w0 + wl;
            tile[cl][wl] = (cc < p.C && ww < p.W) ? ld_map(src, (int64_t)cc * p.in.stride_c + (int64_t)ww * p.in.stride_w) : 0.f;
        }
    } else {
        const int wl = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cl = (threadIdx.x >> 6) + 4 * k;
            const int cc = c0 + cl, ww = w0 + wl;
            tile[cl][wl] = (cc < p.C && ww < p.W) ? ld_map(src, (int64_t)cc * p.in.stride_c + (int64_t)ww * p.in.stride_w) : 0.f;
        }
    }
    __syncthreads();
    const int wl = threadIdx.x & 63, ww = w0 + wl;
    if (ww >= p.W) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cl = (threadIdx.x >> 6) + 4 * k, cc = c0 + cl;
        if (cc < p.C)
            p.out[(((int64_t)b * p.C + cc) * p.H + h) * p.W + ww] = tile[cl][wl] * p.scale[cc] + p.shift[cc];
    }
}


struct TokDynBwdParams {
    FvitMapView in;
    const float* w;      // [C][9]
    const float* dct;    // (B, C, Hq, Wq) contiguous
    float* dx;           // (B, C, Hp, Wp) contiguous
    float* part;         // [B*C][10]: 9 weight-gradient partials + the bias one
    int B, C, Hp, Wp, kh, kw, sh, sw, Ho, Wo, Hq, Wq;
    float inv_area;
};

template <typename IN>
__global__ __launch_bounds__(256) void token_init_dyn_bwd_kernel(TokDynBwdParams p) {
    __shared__ float dconv[kTokLdsFloats];
    const int plane = blockIdx.x;            // b * C + c
    const int c = plane % p.C, b = plane / p.C;
    const IN* __restrict__ src = (const IN*)p.in.data + (int64_t)b * p.in.stride_b + (int64_t)c * p.in.stride_c;
    const float* __restrict__ dq = p.dct + (int64_t)plane * p.Hq * p.Wq;
    const int npix = p.Hp * p.Wp;
    // adjoint of the average pool: a conv-output pixel collects the gradient of every pool window that covers it (windows overlap where
    // kernel > stride; the zero-padded rows / columns of the pooled map, oy >= Ho or ox >= Wo, are never read)
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / p.Wp, x = i - y * p.Wp;
        const int oy1 = min(y / p.sh, p.Ho - 1), ox1 = min(x / p.sw, p.Wo - 1);
        const int oy0 = y < p.kh ? 0 : (y - p.kh) / p.sh + 1, ox0 = x < p.kw ? 0 : (x - p.kw) / p.sw + 1;
        float s = 0.f;
        for (int oy = oy0; oy <= oy1; ++oy)
            for (int ox = ox0; ox <= ox1; ++ox) s += dq[oy * p.Wq + ox];
        dconv[i] = s * p.inv_area;
    }
    __syncthreads();
    float wv[9], acc[10];
#pragma unroll
    for (int j = 0; j < 9; ++j) { wv[j] = p.w[c * 9 + j]; acc[j] = 0.f; }
    acc[9] = 0.f;
    float* __restrict__ dst = p.dx + (int64_t)plane * npix;
    // conv[y][x] = b + sum_k w[ky][kx] in[y + ky - 1][x + kx - 1]: input pixel (y, x) meets w[ky][kx] in conv pixel (y - ky + 1, x - kx + 1)
    for (int i = threadIdx.x; i < npix; i += blockDim.x) {
        const int y = i / p.Wp, x = i - y * p.Wp;
        const float xin = ld_map(src, (int64_t)y * p.in.stride_h + (int64_t)x * p.in.stride_w);
        float g = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int yy = y - ky + 1;
            if (yy < 0 || yy >= p.Hp) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int xx = x - kx + 1;
                if (xx < 0 || xx >= p.Wp) continue;
                const float d = dconv[yy * p.Wp + xx];
                g += wv[ky * 3 + kx] * d;
                acc[ky * 3 + kx] += xin * d;
            }
        }
        acc[9] += dconv[i];
        dst[i] = g;
    }
    // workgroup sums in a fixed order: lanes of a wave (VALU exchanges), then the four waves (through the head of the plane buffer, once every wave is done with it)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const float s = group_sum<64>(acc[j]);
        if (lane == 0) dconv[wave * 10 + j] = s;
    }
    __syncthreads();
    if (threadIdx.x < 10) p.part[(int64_t)plane * 10 + threadIdx.x] = ((dconv[threadIdx.x] + dconv[10 + threadIdx.x]) + dconv[20 + threadIdx.x]) + dconv[30 + threadIdx.x];
}

// dweight[c][j] / dbias[c] = sum over the images, in image order, of the per-plane partials
__global__ __launch_bounds__(256) void token_init_dyn_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ dweight, float* __restrict__ dbias,
                                                                        int B, int C) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= C * 10) return;
    const int c = t / 10, j = t - c * 10;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += part[((int64_t)b * C + c) * 10 + j];
    if (j < 9) dweight[c * 9 + j] = s;
    else dbias[c] = s;
}

struct TapBwdParams {
    FvitMapView x, dx;    // the stage map and its gradient (fp32), both (B, C, Hs, Ws) through their own strides
    const float* dout;    // (B, C, H, W) contiguous
    const float* scale;   // [C]
    float* part;          // [C][rows][2], rows = B * Hs * wtiles
    int B, C, H, W, Hs, Ws, ctiles, wtiles;
    int c_fast;
};

template <typename IN>
__global__ __launch_bounds__(256) void feature_tap_bwd_kernel(TapBwdParams p) {
    __shared__ float td[32][65];
    __shared__ float tx[32][65];
    int t = blockIdx.x;
    const int wt = t % p.wtiles; t /= p.wtiles;
    const int ct = t % p.ctiles; t /= p.ctiles;
    const int h = t % p.Hs, b = t / p.Hs;
    const int c0 = ct * 32, w0 = wt * 64;
    const bool row_in = h < p.H;
    const IN* __restrict__ src = (const IN*)p.x.data + (int64_t)b * p.x.stride_b + (int64_t)h * p.x.stride_h;
    float* __restrict__ dst = (float*)p.dx.data + (int64_t)b * p.dx.stride_b + (int64_t)h * p.dx.stride_h;
    {   // dout: lanes along W
        const int wl = threadIdx.x & 63, ww = w0 + wl;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cl = (threadIdx.x >> 6) + 4 * k, cc = c0 + cl;
            td[cl][wl] = (row_in && cc < p.C && ww < p.W) ? p.dout[(((int64_t)b * p.C + cc) * p.H + h) * p.W + ww] : 0.f;
        }
    }
    // x: lanes along whichever of C / W is unit-stride; zero outside the H x W crop (those pixels have no share in the sums)
    if (p.c_fast) {
        const int cl = threadIdx.x & 31;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int wl = (threadIdx.x >> 5) + 8 * k;
            const int cc = c0 + cl, ww = w0 + wl;
            tx[cl][wl] = (row_in && cc < p.C && ww < p.W) ? ld_map(src, (int64_t)cc * p.x.stride_c + (int64_t)ww * p.x.stride_w) : 0.f;
        }
    } else {
        const int wl = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cl = (threadIdx.x >> 6) + 4 * k;
            const int cc = c0 + cl, ww = w0 + wl;
            tx[cl][wl] = (row_in && cc < p.C && ww < p.W) ? ld_map(src, (int64_t)cc * p.x.stride_c + (int64_t)ww * p.x.stride_w) : 0.f;
        }
    }
    __syncthreads();
    // dx = scale[c] * dout on the crop, zero on whatever else the view exposes, written in x's layout
    if (p.c_fast) {
        const int cl = threadIdx.x & 31, cc = c0 + cl;
        const float sc = cc < p.C ? p.scale[cc] : 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int wl = (threadIdx.x >> 5) + 8 * k, ww = w0 + wl;
            if (cc < p.C && ww < p.Ws) dst[(int64_t)cc * p.dx.stride_c + (int64_t)ww * p.dx.stride_w] = td[cl][wl] * sc;
        }
    } else {
        const int wl = threadIdx.x & 63, ww = w0 + wl;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int cl = (threadIdx.x >> 6) + 4 * k, cc = c0 + cl;
            if (cc < p.C && ww < p.Ws) dst[(int64_t)cc * p.dx.stride_c + (int64_t)ww * p.dx.stride_w] = td[cl][wl] * p.scale[cc];
        }
    }
    // first level of the channel sums: one wave per channel, the 64 pixels of the tile row
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)p.B * p.Hs * p.wtiles;
    const int64_t row = ((int64_t)b * p.Hs + h) * p.wtiles + wt;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int cl = wave + 4 * k, cc = c0 + cl;
        const float d = td[cl][lane];
        const float s0 = group_sum<64>(d), s1 = group_sum<64>(d * tx[cl][lane]);
        if (lane == 0 && cc < p.C) {
            float* q = p.part + ((int64_t)cc * rows + row) * 2;
            q[0] = s0;
            q[1] = s1;
        }
    }
}

// second level: one wave per channel; lane l adds rows l, l + 64, ... in order, then the lanes are combined
__global__ __launch_bounds__(64) void feature_tap_bwd_finish_kernel(const float* __restrict__ part, float* __restrict__ sums, int64_t rows, int C) {
    const int c = blockIdx.x;
    const float2* __restrict__ q = (const float2*)part + (int64_t)c * rows;
    float s0 = 0.f, s1 = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 64) {
        const float2 v = q[r];
        s0 += v.x;
        s1 += v.y;
    }
    s0 = group_sum<64>(s0);
    s1 = group_sum<64>(s1);
    if (threadIdx.x == 0) {
        sums[c] = s0;
        sums[C + c] = s1;
    }
}

}  // namespace

}  // namespace fvit

using namespace fvit;

extern "C" int fvit_token_init_dyn(const FvitMapView* in, const float* weight, const float* bias, float* ct_out, int32_t batch, int32_t C,
                                   int32_t Hp, int32_t Wp, int32_t pool_kh, int32_t pool_kw, int32_t pool_sh, int32_t pool_sw, int32_t cw,
                                   fvit_stream_t stream) {
    if (!in || !in->data || !weight || !bias || !ct_out) { set_error("token_init_dyn: null argument"); return FVIT_EINVAL; }
    TokDynParams p;
    p.in = *in; p.w = weight; p.bias = bias; p.out = ct_out; p.B = batch; p.C = C; p.Hp = Hp; p.Wp = Wp;
    p.kh = pool_kh; p.kw = pool_kw; p.sh = pool_sh; p.sw = pool_sw;
    if (batch <= 0 || C <= 0 || Hp <= 0 || Wp <= 0 || pool_kh <= 0 || pool_kw <= 0 || pool_sh <= 0 || pool_sw <= 0 || cw <= 0 ||
        pool_kh > Hp || pool_kw > Wp) {
        set_error("token_init_dyn: bad geometry B=%d C=%d map %dx%d pool k=%dx%d s=%dx%d cw=%d", batch, C, Hp, Wp, pool_kh, pool_kw, pool_sh,
                  pool_sw, cw);
        return FVIT_EINVAL;
    }
    if ((int64_t)Hp * Wp > kTokLdsFloats) {
        set_error("token_init_dyn: %dx%d map exceeds the %d-pixel LDS plane", Hp, Wp, kTokLdsFloats);
        return FVIT_EINVAL;
    }
    p.Ho = (Hp - pool_kh) / pool_sh + 1;
    p.Wo = (Wp - pool_kw) / pool_sw + 1;
    p.Hq = (p.Ho + cw - 1) / cw * cw;
    p.Wq = (p.Wo + cw - 1) / cw * cw;
    p.inv_area = 1.0f / (float)(pool_kh * pool_kw);
    const int64_t planes = (int64_t)batch * C;
    ProfScope prof(FVIT_K_OTHER, 2.0 * planes * ((double)Hp * Wp * 9 + (double)p.Ho * p.Wo * pool_kh * pool_kw),
                   (double)planes * Hp * Wp * (in->dtype == FVIT_F32 ? 4.0 : 2.0) + 4.0 * planes * p.Hq * p.Wq, (hipStream_t)stream);
    const dim3 grid((unsigned)planes);
    if (in->dtype == FVIT_F32) hipLaunchKernelGGL((token_init_dyn_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (in->dtype == FVIT_F16) hipLaunchKernelGGL((token_init_dyn_kernel<_Float16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (in->dtype == FVIT_BF16) hipLaunchKernelGGL((token_init_dyn_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else { set_error("token_init_dyn: map dtype %d not supported", in->dtype); return FVIT_EINVAL; }
    return check_launch("token_init_dyn_kernel");
}

extern "C" int fvit_feature_tap(const FvitMapView* in, int32_t batch, int32_t C, int32_t H, int32_t W, const float* scale, const float* shift,
                                float* out, fvit_stream_t stream) {
    if (!in || !in->data || !scale || !shift || !out) { set_error("feature_tap: null argument"); return FVIT_EINVAL; }
    if (batch <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("feature_tap: bad shape B=%d C=%d %dx%d", batch, C, H, W); return FVIT_EINVAL; }
    TapParams p;
    p.in = *in; p.scale = scale; p.shift = shift; p.out = out; p.B = batch; p.C = C; p.H = H; p.W = W;
    p.ctiles = (C + 31) / 32; p.wtiles = (W + 63) / 64;
    p.c_fast = (in->stride_c == 1 && in->stride_w != 1) ? 1 : 0;
    const int64_t blocks = (int64_t)batch * H * p.ctiles * p.wtiles;
    if (blocks > 0x7fffffff) { set_error("feature_tap: grid too large"); return FVIT_EINVAL; }
    const double n = (double)batch * C * H * W;
    ProfScope prof(FVIT_K_OTHER, 2.0 * n, n * ((in->dtype == FVIT_F32 ? 4.0 : 2.0) + 4.0), (hipStream_t)stream);
    const dim3 grid((unsigned)blocks);
    if (in->dtype == FVIT_F32) hipLaunchKernelGGL((feature_tap_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (in->dtype == FVIT_F16) hipLaunchKernelGGL((feature_tap_kernel<_Float16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (in->dtype == FVIT_BF16) hipLaunchKernelGGL((feature_tap_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else { set_error("feature_tap: map dtype %d not supported", in->dtype); return FVIT_EINVAL; }
    return check_launch("feature_tap_kernel");
}

extern "C" int fvit_token_init_dyn_backward(const FvitMapView* in, const float* weight, const float* dct, float* dx, float* dweight, float* dbias,
                                            float* partials, int32_t batch, int32_t C, int32_t Hp, int32_t Wp, int32_t pool_kh, int32_t pool_kw,
                                            int32_t pool_sh, int32_t pool_sw, int32_t cw, fvit_stream_t stream) {
    if (!in || !in->data || !weight || !dct || !dx || !dweight || !dbias || !partials) { set_error("token_init_dyn_backward: null argument"); return FVIT_EINVAL; }
    if (batch <= 0 || C <= 0 || Hp <= 0 || Wp <= 0 || pool_kh <= 0 || pool_kw <= 0 || pool_sh <= 0 || pool_sw <= 0 || cw <= 0 || pool_kh > Hp ||
        pool_kw > Wp) {
        set_error("token_init_dyn_backward: bad geometry B=%d C=%d map %dx%d pool k=%dx%d s=%dx%d cw=%d", batch, C, Hp, Wp, pool_kh, pool_kw, pool_sh,
                  pool_sw, cw);
        return FVIT_EINVAL;
    }
    if ((int64_t)Hp * Wp > kTokLdsFloats) {
        set_error("token_init_dyn_backward: %dx%d map exceeds the %d-pixel LDS plane", Hp, Wp, kTokLdsFloats);
        return FVIT_EINVAL;
    }
    TokDynBwdParams p;
    p.in = *in; p.w = weight; p.dct = dct; p.dx = dx; p.part = partials; p.B = batch; p.C = C; p.Hp = Hp; p.Wp = Wp;
    p.kh = pool_kh; p.kw = pool_kw; p.sh = pool_sh; p.sw = pool_sw;
    p.Ho = (Hp - pool_kh) / pool_sh + 1;
    p.Wo = (Wp - pool_kw) / pool_sw + 1;
    p.Hq = (p.Ho + cw - 1) / cw * cw;
    p.Wq = (p.Wo + cw - 1) / cw * cw;
    p.inv_area = 1.0f / (float)(pool_kh * pool_kw);
    const int64_t planes = (int64_t)batch * C;
    if (planes > 0x7fffffff / 10) { set_error("token_init_dyn_backward: grid too large"); return FVIT_EINVAL; }
    ProfScope prof(FVIT_K_OTHER, 2.0 * planes * (double)Hp * Wp * 19,
                   (double)planes * Hp * Wp * ((in->dtype == FVIT_F32 ? 4.0 : 2.0) + 4.0) + 4.0 * planes * p.Hq * p.Wq, (hipStream_t)stream);
    const dim3 grid((unsigned)planes);
    if (in->dtype == FVIT_F32) hipLaunchKernelGGL((token_init_dyn_bwd_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (in->dtype == FVIT_F16) hipLaunchKernelGGL((token_init_dyn_bwd_kernel<_Float16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (in->dtype == FVIT_BF16) hipLaunchKernelGGL((token_init_dyn_bwd_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else { set_error("token_init_dyn_backward: map dtype %d not supported", in->dtype); return FVIT_EINVAL; }
    const int rc = check_launch("token_init_dyn_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(token_init_dyn_bwd_finish_kernel, dim3((unsigned)((C * 10 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, partials, dweight, dbias,
                       batch, C);
    return check_launch("token_init_dyn_bwd_finish_kernel");
}

extern "C" int fvit_feature_tap_backward(const float* dout, const FvitMapView* x, const FvitMapView* dx, int32_t batch, int32_t C, int32_t H, int32_t W,
                                         int32_t Hs, int32_t Ws, const float* scale, float* partials, int64_t partial_floats, float* sums,
                                         fvit_stream_t stream) {
    if (!dout || !x || !x->data || !dx || !dx->data || !scale || !partials || !sums) { set_error("feature_tap_backward: null argument"); return FVIT_EINVAL; }
    if (batch <= 0 || C <= 0 || H <= 0 || W <= 0 || Hs < H || Ws < W) {
        set_error("feature_tap_backward: bad shape B=%d C=%d crop %dx%d of %dx%d", batch, C, H, W, Hs, Ws);
        return FVIT_EINVAL;
    }
    if (dx->dtype != FVIT_F32) { set_error("feature_tap_backward: dx must be fp32"); return FVIT_EINVAL; }
    TapBwdParams p;
    p.x = *x; p.dx = *dx; p.dout = dout; p.scale = scale; p.part = partials; p.B = batch; p.C = C; p.H = H; p.W = W; p.Hs = Hs; p.Ws = Ws;
    p.ctiles = (C + 31) / 32; p.wtiles = (Ws + 63) / 64;
    p.c_fast = (x->stride_c == 1 && x->stride_w != 1) ? 1 : 0;
    const int64_t rows = (int64_t)batch * Hs * p.wtiles;
    const int64_t blocks = rows * p.ctiles;
    if (blocks > 0x7fffffff) { set_error("feature_tap_backward: grid too large"); return FVIT_EINVAL; }
    if (partial_floats < 2 * rows * C) {
        set_error("feature_tap_backward: partials hold %lld floats, need 2 * B * Hs * ceil(Ws / 64) * C = %lld", (long long)partial_floats, (long long)(2 * rows * C));
        return FVIT_EINVAL;
    }
    const double n = (double)batch * C * Hs * Ws;
    ProfScope prof(FVIT_K_OTHER, 4.0 * n, n * ((x->dtype == FVIT_F32 ? 4.0 : 2.0) + 8.0), (hipStream_t)stream);
    const dim3 grid((unsigned)blocks);
    if (x->dtype == FVIT_F32) hipLaunchKernelGGL((feature_tap_bwd_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (x->dtype == FVIT_F16) hipLaunchKernelGGL((feature_tap_bwd_kernel<_Float16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else if (x->dtype == FVIT_BF16) hipLaunchKernelGGL((feature_tap_bwd_kernel<__bf16>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else { set_error("feature_tap_backward: map dtype %d not supported", x->dtype); return FVIT_EINVAL; }
    const int rc = check_launch("feature_tap_bwd_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(feature_tap_bwd_finish_kernel, dim3((unsigned)C), dim3(64), 0, (hipStream_t)stream, partials, sums, rows, C);
    return check_launch("feature_tap_bwd_finish_kernel");
}
