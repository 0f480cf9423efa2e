// Multi-scale deformable attention (Deformable DETR / DINO), forward and backward, for gfx950 -- DESIGN.md section 13.
//
//   out[n][q][m][:] = sum_l sum_p  w[n][q][m][l][p] * bilinear(value_l[n][:][m][:], loc[n][q][m][l][p])
//
// value (N, S, M, D), the levels stacked along S: level l = rows start[l] .. start[l] + H_l W_l - 1, row-major (H_l, W_l); loc = (x, y) in [0, 1];
// pixel coordinate x = loc_x W - 0.5, y = loc_y H - 0.5 (align_corners = False); the four corners around it, each one that lies outside the map contributes
// zero (zero padding).  Whether a corner lies inside is decided on the FLOATING-POINT floor of the coordinate, before any conversion to an integer: a
// location of +-1e9 (or inf / NaN) contributes nothing and overflows nothing.  A row index that would leave value's S rows (inconsistent spatial_shapes /
// level_start_index, which live in device memory and are never seen by the host) is treated like a corner outside the map: the kernels cannot read or
// add out of bounds whatever those two tensors hold.
//
// Work split: lane = channel.  One (n, q, m) "item" is the D channels of one head of one query; a group of G lanes owns it and walks its L * P samples
// in a fixed order, so that the forward and the two per-sample gradients are bitwise repeatable.  The gather is 4 row segments of D elements per sample.
//   forward   G = D / 2 lanes, two adjacent channels per lane (one 4-byte load of a 16-bit value, 8 bytes of fp32)
//   backward  G = min(D, 64) lanes, channels gl (+ 64): every atomic wave-instruction adds 64 / G whole rows of D consecutive floats, i.e. 256 contiguous
//             bytes or two 128-byte segments at D >= 32 (the full-rate shapes of global float atomics); grad_loc / grad_attn are one group_sum<G> each.
// grad_value is a scatter-add with atomicAdd(float*) (one global_atomic_add_f32, no compare-and-swap loop) into an fp32 buffer the entry point zero-fills
// on the call's stream: its last bits depend on the arrival order of the adds -- the only output of this library for which that is so.
#include "fvit_common.h"

namespace fvit {
namespace {

constexpr int MSDA_MAX_L = 8, MSDA_MAX_P = 16;

struct MsdaArgs {
    const void* value;        // T [N][S][M][D]
    const int64_t* shapes;    // [L][2] = (H, W), device memory
    const int64_t* starts;    // [L], device memory
    const float* loc;         // [items][L][P][2]
    const float* attn;        // [items][L][P]
    void* out;                // forward: T [items][D]
    const void* grad_out;     // backward: T [items][D]
    float* grad_value;        // backward: f32 [N][S][M][D], zero on entry
    float* grad_loc;          // backward: f32 [items][L][P][2]
    float* grad_attn;         // backward: f32 [items][L][P]
    int64_t items;            // N * Lq * M, item = (n * Lq + q) * M + m
    int64_t S;
    int Lq, M, L, P;
};

// The four corners of one sample: value row (clamped to a readable row where the corner does not count) and whether it counts; ly / lx = the fractional
// parts.  Returns false when no corner counts (then ly / lx may be anything, NaN included).
struct Corners {
    int64_t row[4];   // (y0, x0), (y0, x1), (y1, x0), (y1, x1)
    bool ok[4];
    float ly, lx;
};
__device__ __forceinline__ bool msda_corners(Corners& c, float locx, float locy, int64_t H, int64_t W, int64_t start, int64_t S) {
    const float Hf = (float)H, Wf = (float)W;
    const float y = locy * Hf - 0.5f, x = locx * Wf - 0.5f;
    const float y0 = floorf(y), x0 = floorf(x), y1 = y0 + 1.0f, x1 = x0 + 1.0f;
    c.ly = y - y0;
    c.lx = x - x0;
    // comparisons in floating point (false for NaN); only a value clamped into [0, n - 1] is converted to an integer
    const bool vy[2] = {y0 >= 0.f && y0 <= Hf - 1.f, y1 >= 0.f && y1 <= Hf - 1.f};
    const bool vx[2] = {x0 >= 0.f && x0 <= Wf - 1.f, x1 >= 0.f && x1 <= Wf - 1.f};
    const int64_t iy[2] = {(int64_t)fminf(fmaxf(y0, 0.f), Hf - 1.f), (int64_t)fminf(fmaxf(y1, 0.f), Hf - 1.f)};
    const int64_t ix[2] = {(int64_t)fminf(fmaxf(x0, 0.f), Wf - 1.f), (int64_t)fminf(fmaxf(x1, 0.f), Wf - 1.f)};
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t r = start + iy[k >> 1] * W + ix[k & 1];
        c.ok[k] = vy[k >> 1] && vx[k & 1] && r >= 0 && r < S;
        c.row[k] = c.ok[k] ? r : 0;
        any |= c.ok[k];
    }
    return any;
}

template <typename T, int N> struct VecOf { typedef T type __attribute__((ext_vector_type(N))); };
template <typename T> struct VecOf<T, 1> { typedef T type; };

// N adjacent channels at p (aligned to N * sizeof(T)) widened to fp32
template <typename T, int N>
__device__ __forceinline__ void load_channels(const T* p, float (&v)[N]) {
    if constexpr (N == 1) {
        v[0] = (float)*p;
    } else {
        const typename VecOf<T, N>::type t = *(const typename VecOf<T, N>::type*)p;
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = (float)t[i];
    }
}
template <typename T> __device__ __forceinline__ T narrow(float x) { return sat16<T>(x); }
template <> __device__ __forceinline__ float narrow<float>(float x) { return x; }

template <typename T, int D>
__global__ __launch_bounds__(256) void msda_fwd_kernel(const MsdaArgs a) {
    constexpr int CPL = 2, G = D / CPL, IPW = 64 / G;   // channels per lane, lanes per item, items per wave
    const int lane = threadIdx.x & 63, gl = lane % G;
    const int64_t item = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * IPW + lane / G;
    if (item >= a.items) return;   // no lane exchange in this kernel
    const int m = (int)(item % a.M);
    const int64_t n = item / a.M / a.Lq;
    const int64_t row_stride = (int64_t)a.M * D;
    const T* vbase = (const T*)a.value + n * a.S * row_stride + (int64_t)m * D + gl * CPL;
    const int LP = a.L * a.P;
    const float* loc = a.loc + item * LP * 2;
    const float* attn = a.attn + item * LP;
    float acc[CPL] = {};
    for (int l = 0; l < a.L; ++l) {
        const int64_t H = a.shapes[2 * l], W = a.shapes[2 * l + 1], start = a.starts[l];
        for (int p = 0; p < a.P; ++p) {
            const int lp = l * a.P + p;
            Corners c;
            if (!msda_corners(c, loc[2 * lp], loc[2 * lp + 1], H, W, start, a.S)) continue;
            const float aw = attn[lp];
            float v[4][CPL];
#pragma unroll
            for (int k = 0; k < 4; ++k) load_channels<T, CPL>(vbase + c.row[k] * row_stride, v[k]);   // unconditional loads of readable rows, selected below
            const float wy[2] = {1.0f - c.ly, c.ly}, wx[2] = {1.0f - c.lx, c.lx};
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += c.ok[k] ? wy[k >> 1] * wx[k & 1] * v[k][i] : 0.f;
                acc[i] += aw * s;
            }
        }
    }
    typename VecOf<T, CPL>::type o;
#pragma unroll
    for (int i = 0; i < CPL; ++i) o[i] = narrow<T>(acc[i]);
    *(typename VecOf<T, CPL>::type*)((T*)a.out + item * D + gl * CPL) = o;
}

template <typename T, int D>
__global__ __launch_bounds__(256) void msda_bwd_kernel(const MsdaArgs a) {
    constexpr int G = D < 64 ? D : 64, CPL = D / G, IPW = 64 / G;   // lanes per item, channels per lane (channel gl + i * G), items per wave
    const int lane = threadIdx.x & 63, gl = lane % G;
    const int64_t item_raw = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * IPW + lane / G;
    const bool live = item_raw < a.items;            // the lanes of a group past the end keep walking (the group sums exchange lanes) and write nothing
    const int64_t item = live ? item_raw : a.items - 1;
    const int m = (int)(item % a.M);
    const int64_t n = item / a.M / a.Lq;
    const int64_t row_stride = (int64_t)a.M * D;
    const int64_t head_off = n * a.S * row_stride + (int64_t)m * D + gl;
    const T* vbase = (const T*)a.value + head_off;
    float* gbase = a.grad_value + head_off;
    const int LP = a.L * a.P;
    const float* loc = a.loc + item * LP * 2;
    const float* attn = a.attn + item * LP;
    float top[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) top[i] = (float)((const T*)a.grad_out)[item * D + gl + i * G];
    float kw = 0.f, kx = 0.f, ky = 0.f;   // lane j of the group keeps the gradients of sample (lp with lp % G == j) until the group stores them together
    for (int l = 0; l < a.L; ++l) {
        const int64_t H = a.shapes[2 * l], W = a.shapes[2 * l + 1], start = a.starts[l];
        for (int p = 0; p < a.P; ++p) {
            const int lp = l * a.P + p;
            Corners c;
            float gw = 0.f, gx = 0.f, gy = 0.f;
            if (msda_corners(c, loc[2 * lp], loc[2 * lp + 1], H, W, start, a.S)) {   // the same for every lane of a group
                const float aw = attn[lp];
                const float wy[2] = {1.0f - c.ly, c.ly}, wx[2] = {1.0f - c.lx, c.lx};
                float v[4][CPL];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int i = 0; i < CPL; ++i) {
                        const float t = (float)vbase[c.row[k] * row_stride + i * G];
                        v[k][i] = c.ok[k] ? t : 0.f;
                    }
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const float val = wy[0] * wx[0] * v[0][i] + wy[0] * wx[1] * v[1][i] + wy[1] * wx[0] * v[2][i] + wy[1] * wx[1] * v[3][i];
                    const float dx = wy[0] * (v[1][i] - v[0][i]) + wy[1] * (v[3][i] - v[2][i]);   // d val / d x (pixels); at lx = 0 the derivative towards x + 1
                    const float dy = wx[0] * (v[2][i] - v[0][i]) + wx[1] * (v[3][i] - v[1][i]);
                    gw += top[i] * val;
                    gx += top[i] * dx;
                    gy += top[i] * dy;
                    const float t = aw * top[i];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c.ok[k] && live) atomicAdd(gbase + c.row[k] * row_stride + i * G, wy[k >> 1] * wx[k & 1] * t);
                }
                gx *= aw * (float)W;
                gy *= aw * (float)H;
            }
            gw = group_sum<G>(gw);
            gx = group_sum<G>(gx);
            gy = group_sum<G>(gy);
            const int slot = lp & (G - 1);
            if (gl == slot) { kw = gw; kx = gx; ky = gy; }
            if (slot == G - 1 || lp == LP - 1) {
                const int64_t at = item * LP + (lp - slot) + gl;
                if (live && gl <= slot) {
                    a.grad_attn[at] = kw;
                    *(float2*)(a.grad_loc + 2 * at) = make_float2(kx, ky);
                }
            }
        }
    }
}

int msda_check(const char* who, int32_t dtype, const void* value, const void* shapes, const void* starts, const void* loc, const void* attn, int32_t N,
               int32_t S, int32_t M, int32_t D, int32_t Lq, int32_t L, int32_t P) {
    if (dtype != FVIT_F32 && dtype != FVIT_F16 && dtype != FVIT_BF16) {
        set_error("%s: value dtype code %d is not supported (fp32, fp16 or bf16; fp64 is not)", who, dtype);
        return FVIT_EINVAL;
    }
    if (D != 16 && D != 32 && D != 64 && D != 128) { set_error("%s: D=%d is not supported (channels per head: 16, 32, 64 or 128)", who, D); return FVIT_EINVAL; }
    if (L < 1 || L > MSDA_MAX_L) { set_error("%s: L=%d is not supported (1 .. %d levels)", who, L, MSDA_MAX_L); return FVIT_EINVAL; }
    if (P < 1 || P > MSDA_MAX_P) { set_error("%s: P=%d is not supported (1 .. %d points)", who, P, MSDA_MAX_P); return FVIT_EINVAL; }
    if (!value || !shapes || !starts || !loc || !attn || N < 1 || S < 1 || M < 1 || Lq < 1) {
        set_error("%s: bad arguments N=%d S=%d M=%d Lq=%d (or a null pointer)", who, N, S, M, Lq);
        return FVIT_EINVAL;
    }
    if (((uintptr_t)value | (uintptr_t)loc) & 7) { set_error("%s: value and sampling_locations must be 8-byte aligned", who); return FVIT_EINVAL; }
    return FVIT_OK;
}

template <typename T>
void msda_launch(bool backward, int D, unsigned grid, const MsdaArgs& a, hipStream_t st) {
#define FVIT_MSDA(D_) do { \
        if (backward) hipLaunchKernelGGL((msda_bwd_kernel<T, D_>), dim3(grid), dim3(256), 0, st, a); \
        else hipLaunchKernelGGL((msda_fwd_kernel<T, D_>), dim3(grid), dim3(256), 0, st, a); } while (0)
    if (D == 16) FVIT_MSDA(16);
    else if (D == 32) FVIT_MSDA(32);
    else if (D == 64) FVIT_MSDA(64);
    else FVIT_MSDA(128);
#undef FVIT_MSDA
}

int msda_run(bool backward, int32_t dtype, MsdaArgs& a, int32_t N, int32_t D, hipStream_t st) {
    const char* who = backward ? "msda_backward" : "msda_forward";
    a.items = (int64_t)N * a.Lq * a.M;
    const int lanes = backward ? (D < 64 ? D : 64) : D / 2;
    const int64_t per_block = 4 * (64 / lanes);
    const int64_t blocks = (a.items + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) { set_error("%s: N * Lq * M = %lld items is more than one launch covers", who, (long long)a.items); return FVIT_EINVAL; }
    const double esz = dtype == FVIT_F32 ? 4.0 : 2.0, samples = (double)a.items * a.L * a.P;
    const double gather = samples * 4.0 * D * esz;   // four corner rows per sample
    ProfScope prof(FVIT_K_OTHER, samples * D * (backward ? 30.0 : 10.0), gather * (backward ? 1.0 + 4.0 / esz : 1.0) + samples * 12.0, st);
    if (backward) {
        const size_t bytes = (size_t)N * a.S * a.M * D * sizeof(float);
        if (hipMemsetAsync(a.grad_value, 0, bytes, st) != hipSuccess) return check_launch("msda_backward: zero-fill of grad_value");
    }
    if (dtype == FVIT_F32) msda_launch<float>(backward, D, (unsigned)blocks, a, st);
    else if (dtype == FVIT_F16) msda_launch<_Float16>(backward, D, (unsigned)blocks, a, st);
    else msda_launch<__bf16>(backward, D, (unsigned)blocks, a, st);
    prof_note(backward ? "msda_bwd_kernel" : "msda_fwd_kernel", (int)blocks);
    return check_launch(backward ? "msda_bwd_kernel" : "msda_fwd_kernel");
}

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" {

int fvit_msda_forward(int32_t value_dtype, const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                      const float* sampling_locations, const float* attention_weights, void* out, int32_t N, int32_t S, int32_t M, int32_t D,
                      int32_t Lq, int32_t L, int32_t P, fvit_stream_t stream) {
    const int rc = msda_check("msda_forward", value_dtype, value, spatial_shapes, level_start_index, sampling_locations, attention_weights, N, S, M, D, Lq, L, P);
    if (rc != FVIT_OK) return rc;
    if (!out || ((uintptr_t)out & 7)) { set_error("msda_forward: out must be a non-null 8-byte aligned pointer"); return FVIT_EINVAL; }
    MsdaArgs a = {};
    a.value = value; a.shapes = spatial_shapes; a.starts = level_start_index; a.loc = sampling_locations; a.attn = attention_weights; a.out = out;
    a.S = S; a.Lq = Lq; a.M = M; a.L = L; a.P = P;
    return msda_run(false, value_dtype, a, N, D, (hipStream_t)stream);
}

int fvit_msda_backward(int32_t value_dtype, const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                       const float* sampling_locations, const float* attention_weights, const void* grad_out, float* grad_value,
                       float* grad_sampling_loc, float* grad_attn_weight, int32_t N, int32_t S, int32_t M, int32_t D, int32_t Lq, int32_t L, int32_t P,
                       fvit_stream_t stream) {
    const int rc = msda_check("msda_backward", value_dtype, value, spatial_shapes, level_start_index, sampling_locations, attention_weights, N, S, M, D, Lq, L, P);
    if (rc != FVIT_OK) return rc;
    if (!grad_out || !grad_value || !grad_sampling_loc || !grad_attn_weight || ((uintptr_t)grad_sampling_loc & 7)) {
        set_error("msda_backward: grad_out, grad_value, grad_sampling_loc (8-byte aligned) and grad_attn_weight must be non-null");
        return FVIT_EINVAL;
    }
    MsdaArgs a = {};
    a.value = value; a.shapes = spatial_shapes; a.starts = level_start_index; a.loc = sampling_locations; a.attn = attention_weights;
    a.grad_out = grad_out; a.grad_value = grad_value; a.grad_loc = grad_sampling_loc; a.grad_attn = grad_attn_weight;
    a.S = S; a.Lq = Lq; a.M = M; a.L = L; a.P = P;
    return msda_run(true, value_dtype, a, N, D, (hipStream_t)stream);
}

}  // extern "C"
