// Detection post-processing for gfx950 -- DESIGN.md section 15: top-k select + box decode (DINO PostProcess), NMS (torchvision's rule), pairwise
// IoU / GIoU (the reference's util/box_ops.py forms) and the Hungarian matcher's fused cost matrix.
//
// Every kernel is wave64, fp32 at the ABI, allocates nothing, never synchronises with the host and uses no atomic on an output: the only atomics are
// integer adds on LDS histograms / an LDS slot counter of the select kernel, whose results do not depend on their order (counts; a set that is sorted
// afterwards).  All outputs are therefore bitwise repeatable call to call, and every entry point can be captured into a graph.
//
//   select   one 1024-thread workgroup per image.  Every logit gets the 56-bit composite  key(logit) << 24 | (2^24 - 1 - flat index)  with key the
//            order-preserving 32-bit image of the float (NaN above +inf, -0 = +0): composites are pairwise distinct, "larger composite" is exactly
//            "higher score, ties to the lower flat index", and the answer is the K largest.  A radix select (digits of 11, 11, 10, 8, 8, 8 bits, LDS
//            histogram + suffix scan per digit) finds the K-th largest composite and stops as soon as the threshold bin is taken whole -- after the
//            32 key bits unless logits tie at the threshold.  As soon as the composites >= the running threshold number 4096 or fewer (after the first
//            digit for a detector's logits) they are copied into LDS and the later digits read only those; until then every pass reads the logits
//            again (all-equal logits: until the index digits thin them out).  The K composites >= the final threshold are compacted into LDS, sorted
//            there (bitonic, descending) and only those K winners go through the sigmoid and the box decode.
//   nms      mask kernel: one wave per (row block, column block >= row block, group) of 64 x 64 boxes in score order, column boxes staged in LDS, one
//            64-bit suppression word per (row box, column block); the lower triangle is neither written nor read.  resolve kernel: one wave per
//            group walks the diagonal blocks in order, resolves each one sequentially on the scalar unit from lane reads of the 64 row words, then
//            ORs the kept rows' words into the removed set of the blocks to the right, lane = column block.
//   pairwise / matcher cost: one output element per thread, nothing but the output is written.
#include "fvit_common.h"

namespace fvit {
namespace {

constexpr int SEL_THREADS = 1024, SEL_BINS = 2048, SEL_MAX_K = 1024, SEL_CAND = 4096;
constexpr int NMS_MAX_N = 8192, NMS_MAX_BLOCKS = NMS_MAX_N / 64;

// ---------------------------------------------------------------------------------------------------------------------------------- select + decode
// order-preserving key: a > b (floats, NaN largest, -0 == +0)  <=>  key(a) > key(b)
__device__ __forceinline__ uint32_t order_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    const uint32_t u = __float_as_uint(x + 0.0f);   // -0 + 0 = +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t composite(float x, uint32_t idx) { return ((uint64_t)order_key(x) << 24) | (uint64_t)(0xFFFFFFu - idx); }

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

struct SelectArgs {
    const float* logits;   // [B][Q * C]
    const float* boxes;    // [B][Q][4] cxcywh
    const float* sizes;    // [B][2] = (h, w)
    float* scores;         // [B][K]
    int64_t* labels;       // [B][K]
    int64_t* query;        // [B][K]
    float* out_boxes;      // [B][K][4]
    int n, C, K, raw, test;
};

// f(composite) for every logit of the image, eight independent loads in flight per thread
template <typename F>
__device__ __forceinline__ void for_each_logit(const float* lg, int n, int tid, F f) {
    for (int base = 0; base < n; base += 8 * SEL_THREADS) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * SEL_THREADS + tid;
            v[u] = i < n ? lg[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = base + u * SEL_THREADS + tid;
            if (i < n) f(composite(v[u], (uint32_t)i));
        }
    }
}

__global__ __launch_bounds__(SEL_THREADS) void det_select_kernel(const SelectArgs a) {
    __shared__ uint32_t hist[SEL_BINS];
    __shared__ uint32_t scan[SEL_THREADS];
    __shared__ uint64_t sel[SEL_MAX_K];
    __shared__ uint64_t cand[SEL_CAND];
    __shared__ uint32_t s_digit, s_rem, s_bin, s_cnt;
    const int tid = threadIdx.x, n = a.n, K = a.K;
    const float* lg = a.logits + (int64_t)blockIdx.x * n;

    // digits from the top of the 56-bit composite: shift of the digit's lowest bit and its width
    constexpr int NPASS = 6;
    const int shifts[NPASS] = {45, 34, 24, 16, 8, 0}, widths[NPASS] = {11, 11, 10, 8, 8, 8};
    uint64_t prefix = 0;     // the digits chosen so far, right-aligned
    uint64_t thr = 0;        // selected <=> composite >= thr
    uint32_t rem = (uint32_t)K;
    bool in_lds = false;     // the composites >= thr are in cand[0 .. m): the later passes no longer read global memory
    int m = 0;
    for (int pass = 0; pass < NPASS; ++pass) {
        const int sh = shifts[pass], wd = widths[pass];
        hist[tid] = 0;
        hist[tid + SEL_THREADS] = 0;
        __syncthreads();
        auto count = [&](uint64_t c) {
            if ((c >> (sh + wd)) == prefix) atomicAdd(&hist[(uint32_t)(c >> sh) & ((1u << wd) - 1u)], 1u);
        };
        if (in_lds) {
            for (int i = tid; i < m; i += SEL_THREADS) count(cand[i]);
        } else {
            for_each_logit(lg, n, tid, count);
        }
        __syncthreads();
        // inclusive suffix sums over the pairs of bins (2 tid, 2 tid + 1)
        const uint32_t h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
        uint32_t s = h0 + h1;
        scan[tid] = s;
        __syncthreads();
        for (int off = 1; off < SEL_THREADS; off <<= 1) {
            const uint32_t v = tid + off < SEL_THREADS ? scan[tid + off] : 0u;
            __syncthreads();
            s += v;
            scan[tid] = s;
            __syncthreads();
        }
        const uint32_t above1 = s - h0 - h1, above0 = above1 + h1;   // elements in bins above bin 2 tid + 1 / above bin 2 tid
        if (above1 < rem && rem <= above1 + h1) { s_digit = 2 * tid + 1; s_rem = rem - above1; s_bin = h1; }
        if (above0 < rem && rem <= above0 + h0) { s_digit = 2 * tid; s_rem = rem - above0; s_bin = h0; }
        __syncthreads();
        prefix = (prefix << wd) | s_digit;
        rem = s_rem;                       // K - rem composites lie above the chosen bin
        thr = prefix << sh;
        const uint32_t bin = s_bin;
        __syncthreads();                   // s_* are rewritten by the next pass
        if (rem == bin) break;             // the threshold bin is taken whole (always so at the last digit: composites are distinct)
        const uint32_t ge = (uint32_t)K - rem + bin;      // composites >= thr: the only ones that still matter
        if (!in_lds && ge <= (uint32_t)SEL_CAND) {        // uniform
            if (tid == 0) s_cnt = 0;
            __syncthreads();
            for_each_logit(lg, n, tid, [&](uint64_t c) {
                if (c >= thr) {
                    const uint32_t at = atomicAdd(&s_cnt, 1u);
                    if (at < (uint32_t)SEL_CAND) cand[at] = c;     // exactly ge of them; the guard is for the LDS bound alone
                }
            });
            __syncthreads();
            in_lds = true;
            m = (int)ge;
        }
    }

    if (tid == 0) s_cnt = 0;
    __syncthreads();
    auto take = [&](uint64_t c) {
        if (c >= thr) {
            const uint32_t at = atomicAdd(&s_cnt, 1u);
            if (at < (uint32_t)SEL_MAX_K) sel[at] = c;      // exactly K composites are >= thr; the guard is for the LDS bound alone
        }
    };
    if (in_lds) {
        for (int i = tid; i < m; i += SEL_THREADS) take(cand[i]);
    } else {
        for_each_logit(lg, n, tid, take);
    }
    int P2 = 1;
    while (P2 < K) P2 <<= 1;
    if (tid >= K && tid < P2) sel[tid] = 0;                 // below every real composite (key >= 0x007fffff)
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < P2 / 2) {
                const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;
                const uint64_t x = sel[i], y = sel[p];
                const bool desc = (i & k) == 0;
                if ((x < y) == desc) { sel[i] = y; sel[p] = x; }
            }
            __syncthreads();
        }
    }

    if (tid < K) {
        const uint32_t idx = 0xFFFFFFu - (uint32_t)(sel[tid] & 0xFFFFFFu);
        const uint32_t safe = idx < (uint32_t)n ? idx : 0u;
        const int q = (int)(safe / (uint32_t)a.C), c = (int)(safe - (uint32_t)q * (uint32_t)a.C);
        const int64_t o = (int64_t)blockIdx.x * K + tid;
        a.scores[o] = sigmoid_f32(lg[safe]);
        a.labels[o] = c;
        a.query[o] = q;
        const int Q = n / a.C;
        const f4 bx = *(const f4*)(a.boxes + ((int64_t)blockIdx.x * Q + q) * 4);
        float x0 = bx[0], y0 = bx[1], x1 = bx[2], y1 = bx[3];
        if (!a.raw) {
            x0 = bx[0] - 0.5f * bx[2];
            y0 = bx[1] - 0.5f * bx[3];
            x1 = bx[0] + 0.5f * bx[2];
            y1 = bx[1] + 0.5f * bx[3];
            if (a.test) { x1 = x1 - x0; y1 = y1 - y0; }
        }
        const float ih = a.sizes[2 * blockIdx.x], iw = a.sizes[2 * blockIdx.x + 1];
        f4 ob;
        ob[0] = x0 * iw; ob[1] = y0 * ih; ob[2] = x1 * iw; ob[3] = y1 * ih;
        *(f4*)(a.out_boxes + o * 4) = ob;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------------- NMS
struct NmsArgs {
    const float* boxes;     // [G][N][4] xyxy
    const int64_t* order;   // [G][N] or null (identity)
    const int64_t* idxs;    // [G][N] or null
    uint64_t* mask;         // [G][N][nb]
    int64_t* keep;          // [G][N]
    int32_t* count;         // [G]
    float thr;
    int N, nb;
};

// box at sorted position pos of group g; a position past N or an order entry outside [0, N) gives a NaN box, which suppresses nothing
__device__ __forceinline__ void nms_load(const NmsArgs& a, int g, int pos, f4& box, int64_t& cls) {
    const float nan = __uint_as_float(0x7FC00000u);
    box[0] = box[1] = box[2] = box[3] = nan;
    cls = 0;
    if (pos >= a.N) return;
    const int64_t at = a.order ? a.order[(int64_t)g * a.N + pos] : (int64_t)pos;
    if (at < 0 || at >= a.N) return;
    box = *(const f4*)(a.boxes + ((int64_t)g * a.N + at) * 4);
    if (a.idxs) cls = a.idxs[(int64_t)g * a.N + at];
}

__global__ __launch_bounds__(64) void nms_mask_kernel(const NmsArgs a) {
    const int cb = blockIdx.x, rb = blockIdx.y, g = blockIdx.z, lane = threadIdx.x;
    if (cb < rb) return;     // upper triangle only (uniform per workgroup)
    __shared__ f4 cbox[64];
    __shared__ int64_t ccls[64];
    __shared__ float carea[64];
    f4 cj;
    int64_t kj;
    nms_load(a, g, cb * 64 + lane, cj, kj);
    cbox[lane] = cj;
    ccls[lane] = kj;
    carea[lane] = (cj[2] - cj[0]) * (cj[3] - cj[1]);
    __syncthreads();
    const int pos = rb * 64 + lane;
    f4 bi;
    int64_t ki;
    nms_load(a, g, pos, bi, ki);
    const float area_i = (bi[2] - bi[0]) * (bi[3] - bi[1]);
    uint64_t word = 0;
    const int first = cb == rb ? lane + 1 : 0;       // only later boxes can be suppressed by this one
    for (int j = first; j < 64; ++j) {
        const f4 bj = cbox[j];
        const float w = fmaxf(0.0f, fminf(bi[2], bj[2]) - fmaxf(bi[0], bj[0]));
        const float h = fmaxf(0.0f, fminf(bi[3], bj[3]) - fmaxf(bi[1], bj[1]));
        const float inter = w * h;
        const float iou = inter / (area_i + carea[j] - inter);    // 0 / 0 = NaN compares false
        if (iou > a.thr && ccls[j] == ki) word |= 1ull << j;
    }
    if (pos < a.N) a.mask[((int64_t)g * a.N + pos) * a.nb + cb] = word;
}

__device__ __forceinline__ uint64_t read_lane64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void nms_resolve_kernel(const NmsArgs a) {
    const int g = blockIdx.x, lane = threadIdx.x, N = a.N, nb = a.nb;
    const uint64_t* mask = a.mask + (int64_t)g * N * nb;
    int64_t* keep = a.keep + (int64_t)g * N;
    uint64_t removed[NMS_MAX_BLOCKS / 64] = {};    // lane l: the removed sets of column blocks l and 64 + l
    int count = 0;
    for (int d = 0; d < nb; ++d) {
        const int pos = d * 64 + lane;
        const uint64_t word = pos < N ? mask[(int64_t)pos * nb + d] : 0ull;
        uint64_t rem = read_lane64(d < 64 ? removed[0] : removed[1], d & 63);
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const uint64_t w = read_lane64(word, i);
            if (!((rem >> i) & 1ull)) rem |= w;
        }
        const int live = N - d * 64 < 64 ? N - d * 64 : 64;
        const uint64_t valid = live == 64 ? ~0ull : (1ull << live) - 1ull;
        const uint64_t kept = ~rem & valid;
        if ((kept >> lane) & 1ull) {
            const int rank = __popcll(kept & ((1ull << lane) - 1ull));
            keep[count + rank] = a.order ? a.order[(int64_t)g * N + pos] : (int64_t)pos;
        }
        count += __popcll(kept);
        // the kept rows of this block suppress into the blocks to the right: lane = column block
#pragma unroll
        for (int half = 0; half < NMS_MAX_BLOCKS / 64; ++half) {
            const int cbk = half * 64 + lane;
            if (half * 64 + 63 <= d || half * 64 >= nb) continue;      // uniform
            uint64_t acc = 0;
            if (cbk > d && cbk < nb) {
                // unconditional loads of readable rows, selected by the kept bit afterwards.  Unrolled by 16: the compiler keeps 16 loads in flight
                // (48 VGPRs); a full unroll made it serialise them again (19 VGPRs) and the kernel three times slower at N = 4096
#pragma unroll 16
                for (int i = 0; i < 64; ++i) {
                    const int row = i < live ? d * 64 + i : d * 64;
                    const uint64_t w = mask[(int64_t)row * nb + cbk];
                    acc |= ((kept >> i) & 1ull) ? w : 0ull;
                }
            }
            removed[half] |= acc;
        }
    }
    for (int i = count + lane; i < N; i += 64) keep[i] = -1;
    if (lane == 0) a.count[g] = count;
}

// ---------------------------------------------------------------------------------------------------------------------- pairwise IoU / GIoU, cost
// the reference's box_iou / generalized_box_iou on one pair (xyxy), 1e-6 in both quotients
__device__ __forceinline__ float pair_iou(const f4& p, const f4& q, float& uni) {
    const float area1 = (p[2] - p[0]) * (p[3] - p[1]), area2 = (q[2] - q[0]) * (q[3] - q[1]);
    const float w = fmaxf(fminf(p[2], q[2]) - fmaxf(p[0], q[0]), 0.0f), h = fmaxf(fminf(p[3], q[3]) - fmaxf(p[1], q[1]), 0.0f);
    const float inter = w * h;
    uni = area1 + area2 - inter;
    return inter / (uni + 1e-6f);
}
__device__ __forceinline__ float pair_giou(const f4& p, const f4& q) {
    float uni;
    const float iou = pair_iou(p, q, uni);
    const float w = fmaxf(fmaxf(p[2], q[2]) - fminf(p[0], q[0]), 0.0f), h = fmaxf(fmaxf(p[3], q[3]) - fminf(p[1], q[1]), 0.0f);
    const float area = w * h;
    return iou - (area - uni) / (area + 1e-6f);
}

__global__ __launch_bounds__(256) void box_pairwise_kernel(const float* b1, const float* b2, float* out, float* uni_out, int64_t total, int M, int giou) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t i = e / M;
    const int j = (int)(e - i * M);
    const f4 p = *(const f4*)(b1 + i * 4), q = *(const f4*)(b2 + (int64_t)j * 4);
    if (giou) {
        out[e] = pair_giou(p, q);
    } else {
        float uni;
        out[e] = pair_iou(p, q, uni);
        if (uni_out) uni_out[e] = uni;
    }
}

__device__ __forceinline__ f4 to_xyxy(const f4& b) {
    f4 r;
    r[0] = b[0] - 0.5f * b[2]; r[1] = b[1] - 0.5f * b[3]; r[2] = b[0] + 0.5f * b[2]; r[3] = b[1] + 0.5f * b[3];
    return r;
}

struct CostArgs {
    const float* logits;    // [R][C]
    const float* pred;      // [R][4] cxcywh
    const int64_t* ids;     // [T]
    const float* tgt;       // [T][4] cxcywh
    float* cost;            // [R][T]
    int64_t total;
    int C, T;
    float w_class, w_bbox, w_giou, alpha, one_minus_alpha;
};

__global__ __launch_bounds__(256) void matcher_cost_kernel(const CostArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.total) return;
    const int64_t r = e / a.T;
    const int t = (int)(e - r * a.T);
    const int64_t id = a.ids[t];
    if (id < 0 || id >= a.C) { a.cost[e] = __uint_as_float(0x7FC00000u); return; }
    const float p = sigmoid_f32(a.logits[r * a.C + id]);
    const float neg = a.one_minus_alpha * (p * p) * (-logf(1.0f - p + 1e-8f));
    const float pos = a.alpha * ((1.0f - p) * (1.0f - p)) * (-logf(p + 1e-8f));
    const float c_class = pos - neg;
    const f4 pb = *(const f4*)(a.pred + r * 4), tb = *(const f4*)(a.tgt + (int64_t)t * 4);
    const float c_bbox = fabsf(pb[0] - tb[0]) + fabsf(pb[1] - tb[1]) + fabsf(pb[2] - tb[2]) + fabsf(pb[3] - tb[3]);
    const float c_giou = -pair_giou(to_xyxy(pb), to_xyxy(tb));
    a.cost[e] = a.w_bbox * c_bbox + a.w_class * c_class + a.w_giou * c_giou;
}

bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" {

int fvit_det_select(const float* logits, const float* boxes, const float* target_sizes, float* scores, int64_t* labels, int64_t* query, float* out_boxes,
                    int32_t B, int32_t Q, int32_t C, int32_t K, int32_t not_to_xyxy, int32_t test, fvit_stream_t stream) {
    if (B < 1 || Q < 1 || C < 1) { set_error("det_select: B=%d Q=%d C=%d must all be >= 1", B, Q, C); return FVIT_EINVAL; }
    const int64_t n = (int64_t)Q * C;
    if (n >= (1LL << 24)) { set_error("det_select: Q * C = %lld is not supported (must be < 2^24)", (long long)n); return FVIT_EINVAL; }
    if (K < 1 || K > SEL_MAX_K || K > n) {
        set_error("det_select: K=%d is not supported (1 <= K <= min(%d, Q * C = %lld))", K, SEL_MAX_K, (long long)n);
        return FVIT_EINVAL;
    }
    if (test && not_to_xyxy) { set_error("det_select: test needs xyxy boxes (not_to_xyxy must be 0)"); return FVIT_EINVAL; }
    if (!logits || !boxes || !target_sizes || !scores || !labels || !query || !out_boxes) { set_error("det_select: a null pointer"); return FVIT_EINVAL; }
    if (misaligned16(boxes) || misaligned16(out_boxes)) { set_error("det_select: boxes and out_boxes must be 16-byte aligned"); return FVIT_EINVAL; }
    SelectArgs a = {logits, boxes, target_sizes, scores, labels, query, out_boxes, (int)n, C, K, not_to_xyxy ? 1 : 0, test ? 1 : 0};
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, (double)B * n * 8.0, (double)B * (n * 4.0 + K * 56.0), st);
    hipLaunchKernelGGL(det_select_kernel, dim3(B), dim3(SEL_THREADS), 0, st, a);
    prof_note("det_select_kernel", B);
    return check_launch("det_select_kernel");
}

size_t fvit_box_nms_workspace(int32_t G, int32_t N) {
    if (G < 1 || N < 1 || N > NMS_MAX_N) return 0;
    return (size_t)G * N * ((N + 63) / 64) * sizeof(uint64_t);
}

int fvit_box_nms(const float* boxes, const int64_t* order, const int64_t* idxs, float iou_threshold, int64_t* keep, int32_t* count, void* workspace,
                 size_t workspace_bytes, int32_t G, int32_t N, fvit_stream_t stream) {
    if (G < 1 || N < 0) { set_error("box_nms: G=%d N=%d (G >= 1 and N >= 0)", G, N); return FVIT_EINVAL; }
    if (N > NMS_MAX_N) { set_error("box_nms: N=%d boxes per group is not supported (N <= %d)", N, NMS_MAX_N); return FVIT_EINVAL; }
    if (N == 0) return FVIT_OK;    // nothing to keep, nothing to write: no launch (a caller that reads count passes N >= 1 or zeroes it)
    if (!boxes || !keep || !count || !workspace) { set_error("box_nms: a null pointer (boxes, keep, count, workspace)"); return FVIT_EINVAL; }
    if (misaligned16(boxes) || ((uintptr_t)workspace & 7)) { set_error("box_nms: boxes must be 16-byte and workspace 8-byte aligned"); return FVIT_EINVAL; }
    const size_t need = fvit_box_nms_workspace(G, N);
    if (workspace_bytes < need) {
        set_error("box_nms: workspace of %zu bytes is too small (G=%d N=%d needs %zu)", workspace_bytes, G, N, need);
        return FVIT_EWORKSPACE;
    }
    if (G > 65535) { set_error("box_nms: G=%d groups is more than one launch covers (65535)", G); return FVIT_EINVAL; }
    const int nb = (N + 63) / 64;
    NmsArgs a = {boxes, order, idxs, (uint64_t*)workspace, keep, count, iou_threshold, N, nb};
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope prof(FVIT_K_OTHER, (double)G * N * N * 8.0, (double)G * N * (16.0 + nb * 4.0), st);
        hipLaunchKernelGGL(nms_mask_kernel, dim3(nb, nb, G), dim3(64), 0, st, a);
        prof_note("nms_mask_kernel", nb * nb * G);
        const int rc = check_launch("nms_mask_kernel");
        if (rc != FVIT_OK) return rc;
    }
    ProfScope prof(FVIT_K_OTHER, 0.0, (double)G * N * (8.0 + nb * 4.0), st);
    hipLaunchKernelGGL(nms_resolve_kernel, dim3(G), dim3(64), 0, st, a);
    prof_note("nms_resolve_kernel", G);
    return check_launch("nms_resolve_kernel");
}

int fvit_box_pairwise(int32_t mode, const float* boxes1, const float* boxes2, float* out, float* union_out, int32_t N, int32_t M, fvit_stream_t stream) {
    if (mode != FVIT_BOX_IOU && mode != FVIT_BOX_GIOU) { set_error("box_pairwise: mode %d is not FVIT_BOX_IOU or FVIT_BOX_GIOU", mode); return FVIT_EINVAL; }
    if (N < 0 || M < 0) { set_error("box_pairwise: N=%d M=%d must be >= 0", N, M); return FVIT_EINVAL; }
    const int64_t total = (int64_t)N * M;
    if (total == 0) return FVIT_OK;
    if (!boxes1 || !boxes2 || !out) { set_error("box_pairwise: a null pointer (boxes1, boxes2, out)"); return FVIT_EINVAL; }
    if (misaligned16(boxes1) || misaligned16(boxes2)) { set_error("box_pairwise: boxes1 and boxes2 must be 16-byte aligned"); return FVIT_EINVAL; }
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) { set_error("box_pairwise: N * M = %lld pairs is more than one launch covers", (long long)total); return FVIT_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, (double)total * 30.0, (double)total * (union_out && mode == FVIT_BOX_IOU ? 8.0 : 4.0) + (N + M) * 16.0, st);
    hipLaunchKernelGGL(box_pairwise_kernel, dim3((unsigned)blocks), dim3(256), 0, st, boxes1, boxes2, out, union_out, total, M, mode == FVIT_BOX_GIOU ? 1 : 0);
    prof_note("box_pairwise_kernel", (int)blocks);
    return check_launch("box_pairwise_kernel");
}

int fvit_det_matcher_cost(const float* logits, const float* pred_boxes, const int64_t* tgt_ids, const float* tgt_boxes, float* cost, int32_t R, int32_t C,
                          int32_t T, float cost_class, float cost_bbox, float cost_giou, float focal_alpha, fvit_stream_t stream) {
    if (R < 0 || T < 0 || C < 1) { set_error("det_matcher_cost: R=%d C=%d T=%d (R, T >= 0 and C >= 1)", R, C, T); return FVIT_EINVAL; }
    const int64_t total = (int64_t)R * T;
    if (total == 0) return FVIT_OK;
    if (!logits || !pred_boxes || !tgt_ids || !tgt_boxes || !cost) { set_error("det_matcher_cost: a null pointer"); return FVIT_EINVAL; }
    if (misaligned16(pred_boxes) || misaligned16(tgt_boxes)) { set_error("det_matcher_cost: pred_boxes and tgt_boxes must be 16-byte aligned"); return FVIT_EINVAL; }
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) { set_error("det_matcher_cost: R * T = %lld is more than one launch covers", (long long)total); return FVIT_EINVAL; }
    CostArgs a = {logits, pred_boxes, tgt_ids, tgt_boxes, cost, total, C, T, cost_class, cost_bbox, cost_giou, focal_alpha, (float)(1.0 - (double)focal_alpha)};
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, (double)total * 80.0, (double)total * 8.0 + (double)R * 16.0 + (double)T * 24.0, st);
    hipLaunchKernelGGL(matcher_cost_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    prof_note("matcher_cost_kernel", (int)blocks);
    return check_launch("matcher_cost_kernel");
}

}  // extern "C"
