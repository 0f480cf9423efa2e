// The DINO training criterion for gfx950 -- DESIGN.md section 16: the focal label loss with cardinality and top-1 hits, and the L1 + GIoU box loss, each
// forward and backward, for up to 16 output sets (decoder layers, interm, denoising sets) per launch.
//
// The rules of fvit_boxes.hip hold: wave64, fp32 at the ABI, no allocation, no host synchronisation, no atomic on an output.  Every sum is taken in a fixed
// order, so all results are bitwise repeatable call to call, and every entry point can be captured into a graph.
//
//   label forward   grid (workgroups, sets), 4 waves.  A workgroup owns one image's chunk of rows, a wave RW of them, a lane the columns lane, lane + 64, ..
//                   of each: RW * ceil(C / 64) <= 32 terms per lane in sequence (C <= 128: RW = 16 and all of them are loaded before the first is used), then 6 additions
//                   in the wave and 2 across the waves.  The row argmax is a wave max followed by a wave min over the lanes' lowest index at that max.
//                   One 16-byte partial (sum, cardinality, hits) per workgroup; the finish kernel, one wave per set, adds the partials: ceil(P / 64) - 1
//                   per lane in sequence, 6 in the wave.  The one-hot tensor is never formed: t = [c == class(r)].
//   label backward  one element per thread, recomputed from the logits; the incoming gradient is read from device memory.
//   box forward     one workgroup per set, pairs i, i + 256, .. per lane; box backward one pair per thread.
#include "fvit_common.h"

namespace fvit {
namespace {

constexpr int LOSS_THREADS = 256, LOSS_WAVES = 4, LOSS_SEQ = 32, LOSS_ROWS = 16;
constexpr float LOSS_EPS = 1e-6f;

struct LabelArgs {
    FvitDetLabelSet set[FVIT_DET_MAX_SETS];
    int nchunk[FVIT_DET_MAX_SETS];   // workgroups per image
    f4* part;                        // [sets][max_blocks]: (sum, cardinality, hits, -)
    float* loss;
    int32_t* card;
    int32_t* hits;
    const float* grad_loss;
    int C, per_row, rows_per_wave, max_blocks, card_stride, gamma2;
    float alpha, one_minus_alpha, gamma;
};

// one term of the focal sum, or its derivative in x.  e = exp(-|x|) gives sigmoid(|x|) = 1 / (1 + e) and 1 - sigmoid(|x|) = e / (1 + e) without a
// cancelling subtraction; m = 1 - p_t, q = p_t.  d/dx [ce m^g] = sgn m^g (m + g q ce), sgn = -1 for t = 1: ce' = p - t = sgn m and m' = sgn m q.
template <bool GRAD>
__device__ __forceinline__ float focal_term(float x, bool t, const LabelArgs& a) {
    const float e = expf(-fabsf(x));
    const float hi = 1.0f / (1.0f + e), lo = e * hi;
    const float p = x >= 0.0f ? hi : lo, np = x >= 0.0f ? lo : hi;
    const float m = t ? np : p, q = t ? p : np;
    const float ce = fmaxf(x, 0.0f) - (t ? x : 0.0f) + log1pf(e);
    const float mg = a.gamma2 ? m * m : powf(m, a.gamma);
    const float at = a.alpha >= 0.0f ? (t ? a.alpha : a.one_minus_alpha) : 1.0f;
    if (!GRAD) return at * ce * mg;
    return (t ? -at : at) * mg * (m + a.gamma * q * ce);
}

__device__ __forceinline__ int wave_min_i32(int x) {
    x = min(x, __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, false));
    const auto r = __builtin_amdgcn_permlane16_swap((uint32_t)x, (uint32_t)x, false, false);
    x = min((int)r[0], (int)r[1]);
    const auto s = __builtin_amdgcn_permlane32_swap((uint32_t)x, (uint32_t)x, false, false);
    return min((int)s[0], (int)s[1]);
}

constexpr int NO_INDEX = 0x7fffffff;

// PR > 0 (1 or 2): ceil(C / 64) == PR at compile time and a wave owns LOSS_ROWS rows, whose logits are all requested before the first is used.
// PR == 0: any C, the row loop loads as it goes.
template <int PR>
__global__ __launch_bounds__(LOSS_THREADS) void label_loss_kernel(const LabelArgs a) {
    const int s = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FvitDetLabelSet& st = a.set[s];
    const int nchunk = a.nchunk[s];
    if ((int)blockIdx.x >= nchunk * st.B) return;      // uniform: a smaller set than the grid was sized for
    const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
    const int C = a.C, Q = st.Q;
    const int RW = PR ? LOSS_ROWS : a.rows_per_wave;
    const int q0 = (chunk * LOSS_WAVES + wave) * RW;
    const float nan = __uint_as_float(0x7FC00000u);
    float acc = 0.0f;
    int card = 0, hits = 0;
    bool bad = false;

    auto row_end = [&](int cls, float best, int besti) {
        const float wmax = group_max<64>(best);
        const int arg = wave_min_i32(best == wmax ? besti : NO_INDEX);
        card += arg != C - 1;
        hits += cls < C && arg == cls;
    };

    if constexpr (PR > 0) {
        constexpr int ROWS = LOSS_ROWS;
        float v[ROWS][PR ? PR : 1];
        int cl[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int q = q0 + i;
            const int64_t r = (int64_t)b * Q + (q < Q ? q : 0);
            cl[i] = st.classes ? st.classes[r] : C;
#pragma unroll
            for (int u = 0; u < PR; ++u) {
                const int c = lane + 64 * u;
                v[i][u] = (q < Q && c < C) ? st.logits[r * C + c] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int q = q0 + i;
            if (q >= Q) break;                          // uniform per wave
            const int64_t r = (int64_t)b * Q + q;
            const int cls = cl[i];
            bad |= cls < 0 || cls > C;
            float best = -INFINITY;
            int besti = NO_INDEX;
#pragma unroll
            for (int u = 0; u < PR; ++u) {
                const int c = lane + 64 * u;
                if (c < C) {
                    const float x = v[i][u];
                    const bool t = st.targets ? st.targets[r * C + c] != 0.0f : c == cls;
                    acc += focal_term<false>(x, t, a);
                    if (x > best || besti == NO_INDEX) { best = x; besti = c; }
                }
            }
            row_end(cls, best, besti);
        }
    } else {
        for (int i = 0; i < RW; ++i) {
            const int q = q0 + i;
            if (q >= Q) break;                          // uniform per wave
            const int64_t r = (int64_t)b * Q + q;
            const int cls = st.classes ? st.classes[r] : C;
            bad |= cls < 0 || cls > C;
            float best = -INFINITY;
            int besti = NO_INDEX;
            for (int c = lane; c < C; c += 64) {
                const float x = st.logits[r * C + c];
                const bool t = st.targets ? st.targets[r * C + c] != 0.0f : c == cls;
                acc += focal_term<false>(x, t, a);
                if (x > best || besti == NO_INDEX) { best = x; besti = c; }
            }
            row_end(cls, best, besti);
        }
    }
    if (bad) acc = nan;                                 // a class id outside [0, C]: the set's loss is NaN (cls is uniform, so every lane agrees)
    acc = group_sum<64>(acc);
    __shared__ float s_sum[LOSS_WAVES];
    __shared__ int s_card[LOSS_WAVES], s_hits[LOSS_WAVES];
    if (lane == 0) { s_sum[wave] = acc; s_card[wave] = card; s_hits[wave] = hits; }
    __syncthreads();
    if (threadIdx.x == 0) {
        f4 p;
        p[0] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        p[1] = __int_as_float(s_card[0] + s_card[1] + s_card[2] + s_card[3]);
        p[2] = __int_as_float(s_hits[0] + s_hits[1] + s_hits[2] + s_hits[3]);
        p[3] = 0.0f;
        a.part[(int64_t)s * a.max_blocks + blockIdx.x] = p;
    }
}

// one wave per set: the sum of its partials, the per-image cardinality, the hit count
__global__ __launch_bounds__(64) void label_finish_kernel(const LabelArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const FvitDetLabelSet& st = a.set[s];
    const int nchunk = a.nchunk[s], P = nchunk * st.B;
    const f4* part = a.part + (int64_t)s * a.max_blocks;
    float acc = 0.0f;
    int hits = 0;
    for (int i = lane; i < P; i += 64) {
        const f4 p = part[i];
        acc += p[0];
        hits += __float_as_int(p[2]);
    }
    acc = group_sum<64>(acc);
    __shared__ int s_hits;
    if (lane == 0) s_hits = 0;
    __syncthreads();
    if (hits) atomicAdd(&s_hits, hits);                 // an integer sum in LDS: its value does not depend on the order
    for (int b = lane; b < st.B; b += 64) {
        int n = 0;
        for (int k = 0; k < nchunk; ++k) n += __float_as_int(part[(int64_t)b * nchunk + k][1]);
        a.card[(int64_t)s * a.card_stride + b] = n;
    }
    __syncthreads();
    if (lane == 0) {
        a.loss[s] = acc * st.scale;
        a.hits[s] = s_hits;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void label_grad_kernel(const LabelArgs a) {
    const int s = blockIdx.y;
    const FvitDetLabelSet& st = a.set[s];
    const int64_t e = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (e >= (int64_t)st.R * a.C) return;
    const int r = (int)(e / a.C), c = (int)(e - (int64_t)r * a.C);
    const int cls = st.classes ? st.classes[r] : a.C;
    const bool t = st.targets ? st.targets[e] != 0.0f : c == cls;
    const float g = a.grad_loss[s] * st.scale;
    float d = focal_term<true>(st.logits[e], t, a) * g;
    if (cls < 0 || cls > a.C) d = __uint_as_float(0x7FC00000u);
    st.grad_logits[e] = d;
}

// ------------------------------------------------------------------------------------------------------------------------------------------ boxes
struct BoxArgs {
    FvitDetBoxSet set[FVIT_DET_MAX_SETS];
    float* out;              // [sets][4]
    const float* grad_out;   // [sets][4]
};

__device__ __forceinline__ f4 cxcywh_xyxy(const f4& b) {
    f4 r;
    r[0] = b[0] - 0.5f * b[2]; r[1] = b[1] - 0.5f * b[3]; r[2] = b[0] + 0.5f * b[2]; r[3] = b[1] + 0.5f * b[3];
    return r;
}

__global__ __launch_bounds__(LOSS_THREADS) void box_loss_kernel(const BoxArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const FvitDetBoxSet& st = a.set[s];
    float xy = 0.0f, hw = 0.0f, gi = 0.0f;
    for (int i = threadIdx.x; i < st.M; i += LOSS_THREADS) {
        const f4 sb = *(const f4*)(st.src + (int64_t)i * 4), tb = *(const f4*)(st.tgt + (int64_t)i * 4);
        xy += fabsf(sb[0] - tb[0]) + fabsf(sb[1] - tb[1]);
        hw += fabsf(sb[2] - tb[2]) + fabsf(sb[3] - tb[3]);
        const f4 p = cxcywh_xyxy(sb), q = cxcywh_xyxy(tb);
        const float area1 = (p[2] - p[0]) * (p[3] - p[1]), area2 = (q[2] - q[0]) * (q[3] - q[1]);
        const float iw = fmaxf(fminf(p[2], q[2]) - fmaxf(p[0], q[0]), 0.0f), ih = fmaxf(fminf(p[3], q[3]) - fmaxf(p[1], q[1]), 0.0f);
        const float inter = iw * ih, uni = area1 + area2 - inter;
        const float ew = fmaxf(fmaxf(p[2], q[2]) - fminf(p[0], q[0]), 0.0f), eh = fmaxf(fmaxf(p[3], q[3]) - fminf(p[1], q[1]), 0.0f);
        const float earea = ew * eh;
        gi += 1.0f - (inter / (uni + LOSS_EPS) - (earea - uni) / (earea + LOSS_EPS));
    }
    xy = group_sum<64>(xy);
    hw = group_sum<64>(hw);
    gi = group_sum<64>(gi);
    __shared__ float s_v[3][LOSS_WAVES];
    if (lane == 0) { s_v[0][wave] = xy; s_v[1][wave] = hw; s_v[2][wave] = gi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float X = (s_v[0][0] + s_v[0][1]) + (s_v[0][2] + s_v[0][3]);
        const float H = (s_v[1][0] + s_v[1][1]) + (s_v[1][2] + s_v[1][3]);
        const float G = (s_v[2][0] + s_v[2][1]) + (s_v[2][2] + s_v[2][3]);
        float* o = a.out + 4 * s;
        o[0] = X * st.scale; o[1] = H * st.scale; o[2] = G * st.scale; o[3] = (X + H) * st.scale;
    }
}

__device__ __forceinline__ float sign0(float d) { return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f); }
// d min(a, b) / da and d max(a, b) / da by torch's rule: the whole gradient to the smaller (larger), halves at a tie
__device__ __forceinline__ float dmin_da(float a, float b) { return a < b ? 1.0f : (a == b ? 0.5f : 0.0f); }
__device__ __forceinline__ float dmax_da(float a, float b) { return a > b ? 1.0f : (a == b ? 0.5f : 0.0f); }

__global__ __launch_bounds__(LOSS_THREADS) void box_grad_kernel(const BoxArgs a) {
    const int s = blockIdx.y;
    const FvitDetBoxSet& st = a.set[s];
    const int i = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (i >= st.M) return;
    const float* go = a.grad_out + 4 * s;
    const float g_xy = (go[0] + go[3]) * st.scale, g_hw = (go[1] + go[3]) * st.scale, g = -go[2] * st.scale;     // g = d / d(GIoU)
    const f4 sb = *(const f4*)(st.src + (int64_t)i * 4), tb = *(const f4*)(st.tgt + (int64_t)i * 4);
    const f4 p = cxcywh_xyxy(sb), q = cxcywh_xyxy(tb);
    const float w1 = p[2] - p[0], h1 = p[3] - p[1];
    const float area1 = w1 * h1, area2 = (q[2] - q[0]) * (q[3] - q[1]);
    const float iw0 = fminf(p[2], q[2]) - fmaxf(p[0], q[0]), ih0 = fminf(p[3], q[3]) - fmaxf(p[1], q[1]);
    const float iw = fmaxf(iw0, 0.0f), ih = fmaxf(ih0, 0.0f);
    const float inter = iw * ih, uni = area1 + area2 - inter;
    const float ew0 = fmaxf(p[2], q[2]) - fminf(p[0], q[0]), eh0 = fmaxf(p[3], q[3]) - fminf(p[1], q[1]);
    const float ew = fmaxf(ew0, 0.0f), eh = fmaxf(eh0, 0.0f);
    const float earea = ew * eh;
    const float ru = 1.0f / (uni + LOSS_EPS), re = 1.0f / (earea + LOSS_EPS);
    // giou = inter ru - (earea - uni) re
    const float G_uni = g * (re - inter * ru * ru);
    const float G_inter = g * ru - G_uni;               // uni = area1 + area2 - inter
    const float G_earea = -g * (uni + LOSS_EPS) * re * re;
    const float G_iw = iw0 >= 0.0f ? G_inter * ih : 0.0f, G_ih = ih0 >= 0.0f ? G_inter * iw : 0.0f;
    const float G_ew = ew0 >= 0.0f ? G_earea * eh : 0.0f, G_eh = eh0 >= 0.0f ? G_earea * ew : 0.0f;
    const float G_x1 = G_iw * dmin_da(p[2], q[2]) + G_ew * dmax_da(p[2], q[2]) + G_uni * h1;
    const float G_x0 = -G_iw * dmax_da(p[0], q[0]) - G_ew * dmin_da(p[0], q[0]) - G_uni * h1;
    const float G_y1 = G_ih * dmin_da(p[3], q[3]) + G_eh * dmax_da(p[3], q[3]) + G_uni * w1;
    const float G_y0 = -G_ih * dmax_da(p[1], q[1]) - G_eh * dmin_da(p[1], q[1]) - G_uni * w1;
    f4 d;
    d[0] = g_xy * sign0(sb[0] - tb[0]) + (G_x0 + G_x1);
    d[1] = g_xy * sign0(sb[1] - tb[1]) + (G_y0 + G_y1);
    d[2] = g_hw * sign0(sb[2] - tb[2]) + 0.5f * (G_x1 - G_x0);
    d[3] = g_hw * sign0(sb[3] - tb[3]) + 0.5f * (G_y1 - G_y0);
    *(f4*)(st.grad_src + (int64_t)i * 4) = d;
}

bool misaligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) != 0; }

struct LabelPlan {
    int per_row, rows_per_wave, max_blocks, nchunk[FVIT_DET_MAX_SETS];
    int64_t max_elems;
};

// the checks every label entry point makes, and the launch geometry
int label_plan(const char* who, const FvitDetLabelSet* sets, int n_sets, int C, bool backward, LabelPlan& pl) {
    if (n_sets < 1 || n_sets > FVIT_DET_MAX_SETS) { set_error("%s: n_sets=%d is not supported (1 <= n_sets <= %d)", who, n_sets, FVIT_DET_MAX_SETS); return FVIT_EINVAL; }
    if (C < 1) { set_error("%s: C=%d must be >= 1", who, C); return FVIT_EINVAL; }
    if (!sets) { set_error("%s: a null pointer (sets)", who); return FVIT_EINVAL; }
    pl.per_row = (C + 63) / 64;
    pl.rows_per_wave = pl.per_row <= 2 ? LOSS_ROWS : (pl.per_row <= LOSS_SEQ ? LOSS_SEQ / pl.per_row : 1);
    pl.max_blocks = 0;
    pl.max_elems = 0;
    for (int s = 0; s < n_sets; ++s) {
        const FvitDetLabelSet& st = sets[s];
        if (st.R < 1 || st.Q < 1 || st.B < 1 || (int64_t)st.B * st.Q != st.R) {
            set_error("%s: set %d has R=%d Q=%d B=%d (all >= 1 and R == B * Q)", who, s, st.R, st.Q, st.B);
            return FVIT_EINVAL;
        }
        if ((int64_t)st.R * C >= (1LL << 31)) { set_error("%s: set %d has R * C = %lld, which is not supported (must be < 2^31)", who, s, (long long)st.R * C); return FVIT_EINVAL; }
        if (!st.logits || (!st.classes && !st.targets) || (backward && !st.grad_logits)) { set_error("%s: set %d has a null pointer", who, s); return FVIT_EINVAL; }
        if (misaligned(st.logits, 4) || misaligned(st.classes, 4) || misaligned(st.targets, 4) || misaligned(st.grad_logits, 4)) {
            set_error("%s: set %d has a misaligned pointer (4-byte aligned floats and ints)", who, s);
            return FVIT_EINVAL;
        }
        pl.nchunk[s] = (st.Q + pl.rows_per_wave * LOSS_WAVES - 1) / (pl.rows_per_wave * LOSS_WAVES);
        const int64_t blocks = (int64_t)pl.nchunk[s] * st.B;
        if (blocks > 0x7fffffffLL) { set_error("%s: set %d needs more workgroups than one launch covers", who, s); return FVIT_EINVAL; }
        if ((int)blocks > pl.max_blocks) pl.max_blocks = (int)blocks;
        if ((int64_t)st.R * C > pl.max_elems) pl.max_elems = (int64_t)st.R * C;
    }
    return FVIT_OK;
}

void label_args(LabelArgs& a, const FvitDetLabelSet* sets, int n_sets, int C, float alpha, float gamma, const LabelPlan& pl) {
    for (int s = 0; s < n_sets; ++s) { a.set[s] = sets[s]; a.nchunk[s] = pl.nchunk[s]; }
    a.C = C;
    a.per_row = pl.per_row;
    a.rows_per_wave = pl.rows_per_wave;
    a.max_blocks = pl.max_blocks;
    a.gamma2 = gamma == 2.0f ? 1 : 0;
    a.alpha = alpha;
    a.one_minus_alpha = (float)(1.0 - (double)alpha);
    a.gamma = gamma;
}

int box_check(const char* who, const FvitDetBoxSet* sets, int n_sets, bool backward, int& max_m) {
    if (n_sets < 1 || n_sets > FVIT_DET_MAX_SETS) { set_error("%s: n_sets=%d is not supported (1 <= n_sets <= %d)", who, n_sets, FVIT_DET_MAX_SETS); return FVIT_EINVAL; }
    if (!sets) { set_error("%s: a null pointer (sets)", who); return FVIT_EINVAL; }
    max_m = 0;
    for (int s = 0; s < n_sets; ++s) {
        const FvitDetBoxSet& st = sets[s];
        if (st.M < 0) { set_error("%s: set %d has M=%d (M >= 0)", who, s, st.M); return FVIT_EINVAL; }
        if (st.M == 0) continue;
        if (!st.src || !st.tgt || (backward && !st.grad_src)) { set_error("%s: set %d has a null pointer", who, s); return FVIT_EINVAL; }
        if (misaligned(st.src, 16) || misaligned(st.tgt, 16) || misaligned(st.grad_src, 16)) {
            set_error("%s: set %d has a misaligned pointer (boxes must be 16-byte aligned)", who, s);
            return FVIT_EINVAL;
        }
        if (st.M > max_m) max_m = st.M;
    }
    return FVIT_OK;
}

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" {

size_t fvit_det_label_loss_workspace(const FvitDetLabelSet* sets, int32_t n_sets, int32_t C) {
    LabelPlan pl;
    if (label_plan("det_label_loss_workspace", sets, n_sets, C, false, pl) != FVIT_OK) return 0;
    return (size_t)n_sets * pl.max_blocks * sizeof(f4);
}

int fvit_det_label_loss(const FvitDetLabelSet* sets, int32_t n_sets, int32_t C, float alpha, float gamma, float* loss, int32_t* card, int32_t card_stride,
                        int32_t* hits, void* workspace, size_t workspace_bytes, fvit_stream_t stream) {
    LabelPlan pl;
    const int rc = label_plan("det_label_loss", sets, n_sets, C, false, pl);
    if (rc != FVIT_OK) return rc;
    if (!loss || !card || !hits || !workspace) { set_error("det_label_loss: a null pointer (loss, card, hits, workspace)"); return FVIT_EINVAL; }
    if (misaligned(loss, 4) || misaligned(card, 4) || misaligned(hits, 4) || misaligned(workspace, 16)) {
        set_error("det_label_loss: a misaligned pointer (loss, card, hits 4-byte, workspace 16-byte aligned)");
        return FVIT_EINVAL;
    }
    for (int s = 0; s < n_sets; ++s)
        if (card_stride < sets[s].B) { set_error("det_label_loss: card_stride=%d is less than B=%d of set %d", card_stride, sets[s].B, s); return FVIT_EINVAL; }
    const size_t need = (size_t)n_sets * pl.max_blocks * sizeof(f4);
    if (workspace_bytes < need) { set_error("det_label_loss: workspace of %zu bytes is too small (%zu needed)", workspace_bytes, need); return FVIT_EWORKSPACE; }
    LabelArgs a = {};
    label_args(a, sets, n_sets, C, alpha, gamma, pl);
    a.part = (f4*)workspace;
    a.loss = loss;
    a.card = card;
    a.hits = hits;
    a.card_stride = card_stride;
    double elems = 0.0;
    for (int s = 0; s < n_sets; ++s) elems += (double)sets[s].R * C;
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope prof(FVIT_K_OTHER, elems * 20.0, elems * 4.0, st);
        const dim3 grid(pl.max_blocks, n_sets);
        if (pl.per_row == 1) hipLaunchKernelGGL(label_loss_kernel<1>, grid, dim3(LOSS_THREADS), 0, st, a);
        else if (pl.per_row == 2) hipLaunchKernelGGL(label_loss_kernel<2>, grid, dim3(LOSS_THREADS), 0, st, a);
        else hipLaunchKernelGGL(label_loss_kernel<0>, grid, dim3(LOSS_THREADS), 0, st, a);
        prof_note("label_loss_kernel", pl.max_blocks * n_sets);
        const int lrc = check_launch("label_loss_kernel");
        if (lrc != FVIT_OK) return lrc;
    }
    ProfScope prof(FVIT_K_OTHER, 0.0, (double)need, st);
    hipLaunchKernelGGL(label_finish_kernel, dim3(n_sets), dim3(64), 0, st, a);
    prof_note("label_finish_kernel", n_sets);
    return check_launch("label_finish_kernel");
}

int fvit_det_label_loss_backward(const FvitDetLabelSet* sets, int32_t n_sets, int32_t C, float alpha, float gamma, const float* grad_loss,
                                 fvit_stream_t stream) {
    LabelPlan pl;
    const int rc = label_plan("det_label_loss_backward", sets, n_sets, C, true, pl);
    if (rc != FVIT_OK) return rc;
    if (!grad_loss || misaligned(grad_loss, 4)) { set_error("det_label_loss_backward: grad_loss is null or misaligned"); return FVIT_EINVAL; }
    LabelArgs a = {};
    label_args(a, sets, n_sets, C, alpha, gamma, pl);
    a.grad_loss = grad_loss;
    double elems = 0.0;
    for (int s = 0; s < n_sets; ++s) elems += (double)sets[s].R * C;
    const int64_t blocks = (pl.max_elems + LOSS_THREADS - 1) / LOSS_THREADS;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, elems * 24.0, elems * 8.0, st);
    hipLaunchKernelGGL(label_grad_kernel, dim3((unsigned)blocks, n_sets), dim3(LOSS_THREADS), 0, st, a);
    prof_note("label_grad_kernel", (int)blocks * n_sets);
    return check_launch("label_grad_kernel");
}

int fvit_det_box_loss(const FvitDetBoxSet* sets, int32_t n_sets, float* out, fvit_stream_t stream) {
    int max_m = 0;
    const int rc = box_check("det_box_loss", sets, n_sets, false, max_m);
    if (rc != FVIT_OK) return rc;
    if (!out || misaligned(out, 4)) { set_error("det_box_loss: out is null or misaligned"); return FVIT_EINVAL; }
    if (max_m == 0) return FVIT_OK;      // no pair in any set: no launch, nothing written
    BoxArgs a = {};
    double pairs = 0.0;
    for (int s = 0; s < n_sets; ++s) { a.set[s] = sets[s]; pairs += sets[s].M; }
    a.out = out;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, pairs * 50.0, pairs * 32.0, st);
    hipLaunchKernelGGL(box_loss_kernel, dim3(n_sets), dim3(LOSS_THREADS), 0, st, a);
    prof_note("box_loss_kernel", n_sets);
    return check_launch("box_loss_kernel");
}

int fvit_det_box_loss_backward(const FvitDetBoxSet* sets, int32_t n_sets, const float* grad_out, fvit_stream_t stream) {
    int max_m = 0;
    const int rc = box_check("det_box_loss_backward", sets, n_sets, true, max_m);
    if (rc != FVIT_OK) return rc;
    if (!grad_out || misaligned(grad_out, 4)) { set_error("det_box_loss_backward: grad_out is null or misaligned"); return FVIT_EINVAL; }
    if (max_m == 0) return FVIT_OK;
    BoxArgs a = {};
    double pairs = 0.0;
    for (int s = 0; s < n_sets; ++s) { a.set[s] = sets[s]; pairs += sets[s].M; }
    a.grad_out = grad_out;
    const int blocks = (max_m + LOSS_THREADS - 1) / LOSS_THREADS;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, pairs * 90.0, pairs * 48.0, st);
    hipLaunchKernelGGL(box_grad_kernel, dim3(blocks, n_sets), dim3(LOSS_THREADS), 0, st, a);
    prof_note("box_grad_kernel", blocks * n_sets);
    return check_launch("box_grad_kernel");
}

}  // extern "C"
