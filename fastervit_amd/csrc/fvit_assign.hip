// The matcher's Hungarian assignment for gfx950 -- DESIGN.md section 17: a batched rectangular linear-sum-assignment solver, one wave64 per problem.
//
// A problem is the block cost[b, :, toff[b]:toff[b + 1]] of one output set's fp32 (B, Q, T) matrix: Q queries x n_b targets.  Grid (B, sets), 64 threads.
// The solver is the shortest augmenting path with dual variables (Jonker-Volgenant as Crouse states it, the form scipy.optimize.linear_sum_assignment
// implements), run over the SHORT side of the block: k = min(Q, n_b) augmentations, each of which walks "rows" of the short side and relaxes
// shortest[j] of every unvisited "column" j of the long side, one column per lane and step (j = lane, lane + 64, ..).
//
//   layout     the long side is contiguous for the lanes.  n_b >= Q: rows are queries and the input's rows are read as they are.  n_b < Q (DINO): rows are
//              targets, whose costs are T floats apart in the input, so the block is first transposed into the workspace ([target][query]); every lane
//              later reads only what it wrote itself.  The same pass looks for non-finite costs.
//   state      u, v, shortest in fp64 and path, row4col, col4row as int16 in LDS (30 bytes per unit of the cap ASSIGN_CAP = 2048: 60 KiB); the visited
//              columns are one bit per column in a 32-bit register of the owning lane.  The rows that were visited are exactly the current row and the
//              row4col of the visited columns, so no row flags are kept.
//   arg-min    lane-local over (shortest, assigned, j) in ascending j, then a wave minimum of the fp64 value (DPP inside a 16-lane row, permlane swaps across)
//              and a wave minimum of the int key (assigned << 16 | j) among the lanes that hold it: lowest cost, then an unassigned column, then the lowest
//              index.  Fixed, so the result is bitwise repeatable; there is no atomic anywhere.
//   bounds     exactly k augmentations; at most k + 1 column visits in each and at most k + 1 steps back along the path.  A solve that runs into a bound
//              (it cannot with finite costs) gives status 2.  Non-finite costs are not solved: status 1.  Offsets that contradict the host's statement
//              (n_b outside [0, max_nb], a target range outside [0, T], pair offsets that are not the prefix sum of k or leave the output arrays) give
//              status 3 and write nothing.  Status 1 and 2 write the identity pairing 0 .. k - 1.
//   output     k pairs at pair_off[b]: src ascending.  Queries on the long side: row4col compacted by ballot, 64 columns a step.
#include "fvit_common.h"

namespace fvit {
namespace {

constexpr int ASSIGN_CAP = 2048;                  // both sides of a block; 32 columns per lane = the bits of the visited mask
constexpr int ASSIGN_NO_KEY = 0x7fffffff;
constexpr int ASSIGN_UNROLL = 8;                  // global loads in flight per lane

struct AssignArgs {
    FvitDetAssignSet set[FVIT_DET_MAX_SETS];
    int64_t ws_off[FVIT_DET_MAX_SETS];            // floats into the workspace: the set's [T][Q] transposed costs
    const int32_t* toff;
    const int32_t* pair_off;
    int32_t* status;                              // [sets][B]
    float* ws;
    int B, max_nb;
};

template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// element [0] of both swaps comes from the same lane of a pair, and so does [1]
__device__ __forceinline__ double min_xor16_f64(double x) {
    const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)__double2loint(x), (uint32_t)__double2loint(x), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)__double2hiint(x), (uint32_t)__double2hiint(x), false, false);
    return fmin(__hiloint2double((int)hi[0], (int)lo[0]), __hiloint2double((int)hi[1], (int)lo[1]));
}
__device__ __forceinline__ double min_xor32_f64(double x) {
    const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)__double2loint(x), (uint32_t)__double2loint(x), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)__double2hiint(x), (uint32_t)__double2hiint(x), false, false);
    return fmin(__hiloint2double((int)hi[0], (int)lo[0]), __hiloint2double((int)hi[1], (int)lo[1]));
}
__device__ __forceinline__ double wave_min_f64(double x) {
    x = fmin(x, dpp_f64<0xB1>(x));
    x = fmin(x, dpp_f64<0x4E>(x));
    x = fmin(x, dpp_f64<0x141>(x));
    x = fmin(x, dpp_f64<0x140>(x));
    x = min_xor16_f64(x);
    return min_xor32_f64(x);
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

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(64) void assign_kernel(const AssignArgs a) {
    __shared__ double s_u[ASSIGN_CAP], s_v[ASSIGN_CAP], s_short[ASSIGN_CAP];
    __shared__ int16_t s_path[ASSIGN_CAP], s_row4col[ASSIGN_CAP], s_col4row[ASSIGN_CAP];
    const int b = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
    const FvitDetAssignSet& st = a.set[s];
    const int Q = st.Q, T = st.T;
    int32_t* status = a.status + (int64_t)s * a.B + b;
    const int t0 = a.toff[b], t1 = a.toff[b + 1], p0 = a.pair_off[b], p1 = a.pair_off[b + 1];
    const int n = t1 - t0;
    const int k = n < Q ? n : Q;
    // what the host could not see: every value is uniform over the wave
    if (t0 < 0 || n < 0 || n > a.max_nb || t1 > T || p0 < 0 || p1 - p0 != k || p1 > st.n_pairs) {
        if (lane == 0) *status = 3;
        return;
    }
    if (n == 0) {
        if (lane == 0) *status = 0;
        return;
    }
    int64_t* src = st.src + p0;
    int64_t* tgt = st.tgt + p0;
    const bool q_long = n < Q;                    // queries are the columns of the solve
    const int nr = k, nc = q_long ? Q : n;
    const float* in = st.cost + (int64_t)b * Q * T + t0;
    const float* rows;                            // cost(i, j) = rows[i * ld + j]
    int64_t ld;
    bool bad = false;
    if (q_long) {
        float* w = a.ws + a.ws_off[s] + (int64_t)t0 * Q;
        for (int q = lane; q < Q; q += 64) {
            const float* r = in + (int64_t)q * T;
            for (int tb = 0; tb < n; tb += ASSIGN_UNROLL) {       // the loads of a group are all requested before the first is stored
                float x[ASSIGN_UNROLL];
#pragma unroll
                for (int e = 0; e < ASSIGN_UNROLL; ++e) x[e] = tb + e < n ? r[tb + e] : 0.0f;
#pragma unroll
                for (int e = 0; e < ASSIGN_UNROLL; ++e) {
                    bad |= !finite32(x[e]);
                    if (tb + e < n) w[(int64_t)(tb + e) * Q + q] = x[e];
                }
            }
        }
        rows = w;
        ld = Q;
    } else {
        for (int q = 0; q < Q; ++q) {
            const float* r = in + (int64_t)q * T;
            for (int t = lane; t < n; t += 64) bad |= !finite32(r[t]);
        }
        rows = in;
        ld = T;
    }
    int code = __ballot(bad) != 0ull ? 1 : 0;

    if (code == 0) {
        for (int j = lane; j < nc; j += 64) { s_v[j] = 0.0; s_row4col[j] = -1; }
        for (int i = lane; i < nr; i += 64) { s_u[i] = 0.0; s_col4row[i] = -1; }
        __syncthreads();
        const int per_lane = (nc - lane + 63) >> 6;        // columns lane, lane + 64, .. below nc
        for (int cur = 0; cur < nr; ++cur) {
            for (int j = lane; j < nc; j += 64) s_short[j] = INFINITY;
            uint32_t visited = 0;
            double min_val = 0.0;
            int i = cur, sink = -1;
            for (int visit = 0; visit <= nr && sink < 0; ++visit) {
                const float* ci = rows + (int64_t)i * ld;
                const double ui = s_u[i];
                double best = INFINITY;
                int best_key = ASSIGN_NO_KEY;
                for (int tb = 0; tb < per_lane; tb += ASSIGN_UNROLL) {      // a group's costs are all requested before the first is used
                    float cv[ASSIGN_UNROLL];
#pragma unroll
                    for (int e = 0; e < ASSIGN_UNROLL; ++e) cv[e] = tb + e < per_lane ? ci[lane + ((tb + e) << 6)] : 0.0f;
#pragma unroll
                    for (int e = 0; e < ASSIGN_UNROLL; ++e) {
                        const int t = tb + e;
                        if (t >= per_lane || ((visited >> t) & 1u)) continue;
                        const int j = lane + (t << 6);
                        const double r = min_val + (double)cv[e] - ui - s_v[j];
                        double sh = s_short[j];
                        if (r < sh) { sh = r; s_short[j] = r; s_path[j] = (int16_t)i; }
                        const int key = (s_row4col[j] >= 0 ? 0x10000 : 0) | j;
                        if (sh < best || (sh == best && key < best_key)) { best = sh; best_key = key; }
                    }
                }
                const double low = wave_min_f64(best);
                const int key = wave_min_i32(best == low ? best_key : ASSIGN_NO_KEY);
                if (!(low < INFINITY) || key == ASSIGN_NO_KEY) break;      // no reachable column: not possible with finite costs
                const int j = key & 0xffff;
                min_val = low;
                if ((j & 63) == lane) visited |= 1u << (j >> 6);
                const int r4c = s_row4col[j];
                if (r4c < 0) sink = j; else i = r4c;
            }
            if (sink < 0) { code = 2; break; }
            // the duals: u of the current row and of the rows behind the visited columns, v of the visited columns
            for (int t = 0; t < per_lane; ++t) {
                if (!((visited >> t) & 1u)) continue;
                const int j = lane + (t << 6);
                const double d = min_val - s_short[j];
                s_v[j] -= d;
                const int r = s_row4col[j];
                if (r >= 0) s_u[r] += d;
            }
            if (lane == 0) s_u[cur] += min_val;
            __syncthreads();
            // back along the path: one lane, at most cur + 1 steps
            bool closed = false;
            if (lane == 0) {
                int j = sink;
                for (int step = 0; step <= nr; ++step) {
                    const int r = s_path[j];
                    s_row4col[j] = (int16_t)r;
                    const int prev = s_col4row[r];
                    s_col4row[r] = (int16_t)j;
                    j = prev;
                    if (r == cur) { closed = true; break; }
                    if (j < 0) break;
                }
            }
            __syncthreads();
            if ((__ballot(closed) & 1ull) == 0ull) { code = 2; break; }
        }
    }

    if (code != 0) {
        for (int i = lane; i < k; i += 64) { src[i] = i; tgt[i] = i; }
    } else if (!q_long) {
        for (int i = lane; i < k; i += 64) { src[i] = i; tgt[i] = s_col4row[i]; }
    } else {
        int base = 0;
        for (int j0 = 0; j0 < nc; j0 += 64) {
            const int j = j0 + lane;
            const int r = j < nc ? (int)s_row4col[j] : -1;
            const unsigned long long m = __ballot(r >= 0);
            if (r >= 0) {
                const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
                if (pos < k) { src[pos] = j; tgt[pos] = r; }
            }
            base += __popcll(m);
        }
    }
    if (lane == 0) *status = code;
}

bool misaligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) != 0; }

int assign_check(const char* who, const FvitDetAssignSet* sets, int n_sets, int B, bool pointers, size_t& need) {
    if (n_sets < 1 || n_sets > FVIT_DET_MAX_SETS) { set_error("%s: n_sets=%d is not supported (1 <= n_sets <= %d)", who, n_sets, FVIT_DET_MAX_SETS); return FVIT_EINVAL; }
    if (B < 1) { set_error("%s: B=%d must be >= 1", who, B); return FVIT_EINVAL; }
    if (!sets) { set_error("%s: a null pointer (sets)", who); return FVIT_EINVAL; }
    need = 0;
    for (int s = 0; s < n_sets; ++s) {
        const FvitDetAssignSet& st = sets[s];
        if (st.Q < 1) { set_error("%s: set %d has Q=%d (Q >= 1)", who, s, st.Q); return FVIT_EINVAL; }
        if (st.T < 0) { set_error("%s: set %d has T=%d (T >= 0)", who, s, st.T); return FVIT_EINVAL; }
        if (st.Q > ASSIGN_CAP) { set_error("%s: set %d has Q=%d above the cap of %d a side (the solver's state is held in LDS)", who, s, st.Q, ASSIGN_CAP); return FVIT_EINVAL; }
        if (st.n_pairs < 0) { set_error("%s: set %d has n_pairs=%d (n_pairs >= 0)", who, s, st.n_pairs); return FVIT_EINVAL; }
        if (pointers && st.T > 0) {
            if (!st.cost || (st.n_pairs > 0 && (!st.src || !st.tgt))) { set_error("%s: set %d has a null pointer", who, s); return FVIT_EINVAL; }
            if (misaligned(st.cost, 4) || misaligned(st.src, 8) || misaligned(st.tgt, 8)) {
                set_error("%s: set %d has a misaligned pointer (cost 4-byte, src and tgt 8-byte aligned)", who, s);
                return FVIT_EINVAL;
            }
        }
        need += (size_t)st.Q * (size_t)st.T * sizeof(float);
    }
    need = (need + 15) & ~(size_t)15;
    if (need == 0) need = 16;
    return FVIT_OK;
}

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" {

size_t fvit_det_assign_workspace(const FvitDetAssignSet* sets, int32_t n_sets, int32_t B) {
    size_t need = 0;
    if (assign_check("det_assign_workspace", sets, n_sets, B, false, need) != FVIT_OK) return 0;
    return need;
}

int fvit_det_assign(const FvitDetAssignSet* sets, int32_t n_sets, int32_t B, const int32_t* toff, const int32_t* pair_off, int32_t max_nb, int32_t* status,
                    void* workspace, size_t workspace_bytes, fvit_stream_t stream) {
    size_t need = 0;
    const int rc = assign_check("det_assign", sets, n_sets, B, true, need);
    if (rc != FVIT_OK) return rc;
    if (max_nb < 0) { set_error("det_assign: max_nb=%d must be >= 0", max_nb); return FVIT_EINVAL; }
    if (max_nb > ASSIGN_CAP) { set_error("det_assign: max_nb=%d, an image's n_b, is above the cap of %d a side (the solver's state is held in LDS)", max_nb, ASSIGN_CAP); return FVIT_EINVAL; }
    int max_t = 0;
    for (int s = 0; s < n_sets; ++s) max_t = sets[s].T > max_t ? sets[s].T : max_t;
    if (max_t == 0) return FVIT_OK;               // no target in any set: no launch, nothing written
    if (!toff || !pair_off || !status || !workspace) { set_error("det_assign: a null pointer (toff, pair_off, status, workspace)"); return FVIT_EINVAL; }
    if (misaligned(toff, 4) || misaligned(pair_off, 4) || misaligned(status, 4) || misaligned(workspace, 16)) {
        set_error("det_assign: a misaligned pointer (toff, pair_off, status 4-byte, workspace 16-byte aligned)");
        return FVIT_EINVAL;
    }
    if (workspace_bytes < need) { set_error("det_assign: workspace of %zu bytes is too small (%zu needed)", workspace_bytes, need); return FVIT_EWORKSPACE; }
    AssignArgs a = {};
    int64_t off = 0;
    double elems = 0.0;
    for (int s = 0; s < n_sets; ++s) {
        a.set[s] = sets[s];
        a.ws_off[s] = off;
        off += (int64_t)sets[s].Q * sets[s].T;
        elems += (double)B * sets[s].Q * sets[s].T;
    }
    a.toff = toff;
    a.pair_off = pair_off;
    a.status = status;
    a.ws = (float*)workspace;
    a.B = B;
    a.max_nb = max_nb;
    hipStream_t st = (hipStream_t)stream;
    ProfScope prof(FVIT_K_OTHER, elems * 8.0, elems * 12.0, st);
    hipLaunchKernelGGL(assign_kernel, dim3(B, n_sets), dim3(64), 0, st, a);
    prof_note("assign_kernel", B * n_sets);
    return check_launch("assign_kernel");
}

}  // extern "C"
