// fvit_attnbwd.hip -- backward of the windowed attention core for ANY sequence length (S >= 1; the training path beyond the 64 tokens that
// attn_bwd_kernel of fvit_bwd.hip holds in LDS), gfx950.  WindowAttention.forward FV:557-568 between the qkv and proj Linears:
//
//     S = q k^T * scale + bias,  P = softmax(S),  O = P v;   given dO:
//     dV = P^T dO,  dP = dO v^T,  dS = P * (dP - rowsum(dP * P)),  dq = scale * dS k,  dk = scale * dS^T q,  dbias = sum over windows of dS
//
// Operand layouts are the forward's (fvit_attn.hip / fvit_attnlong.hip): qkv / dqkv op16 [rows][ld], columns [q|k|v][head][D] (D = padded head_dim
// 32 / 64 / 96), dO op16 [rows][ldo], columns [head][D]; bias either dense f32 [heads][spad][spad] or the compact table f32 [heads][(2w-1)^2] with
// index(q, k) = qbase(q) - kpos(k) and rel_ng leading tokens without bias, exactly as fvit_attnlong.hip evaluates it.
//
// Nothing of size S x S is resident: every phase works on tiles of 64 "own" rows (16 per wave: the B operand of the MFMAs, held in registers) x 32
// "loop" rows (the A operand, fragments read from global / L2), and recomputes the probabilities of a tile from per-row statistics.  All five products
// are v_mfma_f32_16x16x32_{f16,bf16} with fp32 accumulation, in the transposed orientation of the forward kernels (a lane owns ONE own row as the MFMA
// column, so the own side's statistics are per-lane scalars and a score tile is already the B operand of the product that contracts over the loop rows;
// the A operand of that product is the loop-side matrix transposed through LDS, double-buffered, one barrier per tile):
//
//   phase 0  STATS  own = queries, loop = keys    online softmax: lse[q] = max + log(sum) and delta[q] = rowsum(dP * P), both fp32
//   phase 1  DQ     own = queries, loop = keys    P = exp(s - lse), dS = P * (dP - delta) in fp32;  dQ^T += K^T dS^T          -> dq
//   phase 2  DKV    own = keys,    loop = queries the same tile, the other way round;  dK^T += Q^T dS, dV^T += dO^T P           -> dk, dv
//   phase 3  DBIAS  (only when a bias gradient is asked for) a workgroup owns one (head, 64 queries, 32 keys) tile and adds dS over the windows IN
//                   WINDOW ORDER in registers -> dense: dbias[h][q][k] += sum;  compact: dssum[h][q][k] = sum, then
//            GATHER one thread per table entry (head, dy, dx) adds dssum[h][q][q - (dy, dx)] over the queries in raster order -> d_rel_table += sum
//
// A workgroup OWNS what it writes and every sum has a fixed order: no atomics (global or LDS), bit-reproducible results.  The score tile is recomputed
// in each phase (2 + 3 + 4 + 2 tile products against the 5 of the algorithmic count); that is the accepted price of the ownership rule.
//
// Workspace (fvit_bwd_window_attention_long_workspace): 2 * nwin * heads * pad64(S) floats of row statistics, plus -- compact form with a bias
// gradient only -- heads * S * S floats for the window-summed dS.  Neither term grows with nwin * S^2: at S = 576, heads = 16 that is 21 MB for ANY
// number of windows, where fvit_bwd_window_attention's dbias_part would take 21 MB per window.  The dense form needs no bias scratch at all.
#include "fvit_common.h"

namespace fvit {
namespace {

enum { AB_STATS = 0, AB_DQ = 1, AB_DKV = 2, AB_DBIAS = 3 };

struct AttnBwdParams {
    const void* qkv;
    const void* dO;
    void* dqkv;
    const float* bias;        // dense f32 [heads][spad][spad] or null
    const float* rel_table;   // compact f32 [heads][(2w-1)^2] or null
    float* lse;               // f32 [nwin * heads][sst]
    float* delta;             // f32 [nwin * heads][sst]
    float* dsum;              // DBIAS: f32 [heads][S][S]
    int ld, ldo;
    int nwin, S, heads, spad;
    int w, ng;                // compact form: window side, leading tokens without bias
    int sst;                  // pad64(S): row stride of the statistics, entries of the position table
    int nto;                  // 64-row own tiles per (window, head)
    int tab_in_lds;
    int accumulate;           // DBIAS: dsum += (dense gradient buffer) or = (workspace)
    float scale;
};

constexpr int AB_VROW = 40;   // transposed row: 32 loop-row slots + 8 pad elements (16-byte aligned rows, bank stride broken), as LONG_VROW

template <typename T, int DP, int MODE>
__global__ __launch_bounds__(256) void attn_bwd_long_kernel(AttnBwdParams p) {
    typedef typename Op16<T>::v8 v8;
    typedef typename Op16<T>::v4 v4;
    constexpr int KD = DP / 32;   // k-steps over head_dim of the score products
    constexpr int DB = DP / 16;   // channel blocks of the accumulated products
    constexpr int CH = DP / 8;    // 16-byte chunks per row
    constexpr bool OWNQ = MODE != AB_DKV;                                // the own rows are queries
    constexpr int NTR = MODE == AB_DQ ? 1 : (MODE == AB_DKV ? 2 : 0);    // loop-side matrices transposed through LDS
    constexpr int XT = DP * AB_VROW;                                     // elements of one transposed tile
    extern __shared__ __attribute__((aligned(16))) char smem_ab[];
    // layout: [2 buffers x NTR x DP x AB_VROW op16][pos int32 x sst][table f32 x (2w-1)^2]
    T* xt_base = (T*)smem_ab;
    int* pos = (int*)(smem_ab + 2 * NTR * XT * 2);
    float* tab = (float*)(pos + p.sst);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, s = lane & 15;
    const int S = p.S;
    const int HD = p.heads * DP;
    const int tw = 2 * p.w - 1;
    const int ntl = (S + 31) >> 5;

    int head, ot, w0, w1, t0, t1;
    if constexpr (MODE == AB_DBIAS) {
        const int per_head = p.nto * ntl;
        head = blockIdx.x / per_head;
        const int rem = blockIdx.x - head * per_head;
        ot = rem / ntl;
        t0 = rem - ot * ntl; t1 = t0 + 1;
        w0 = 0; w1 = p.nwin;
    } else {
        const int item = blockIdx.x / p.nto;
        ot = blockIdx.x - item * p.nto;
        w0 = item / p.heads; w1 = w0 + 1;
        head = item - w0 * p.heads;
        t0 = 0; t1 = ntl;
    }

    // ---- per-workgroup tables: pos[t] = y * (2w-1) + x of token t inside the bias window, -1 = no bias (carrier token, padding, no compact table) ----
    const float* __restrict__ gtab = p.rel_table ? p.rel_table + (size_t)head * tw * tw : nullptr;
    for (int k = tid; k < p.sst; k += 256) {
        int v = -1;
        if (gtab && k >= p.ng && k < S) {
            const int l = k - p.ng, y = l / p.w;
            v = y * tw + (l - y * p.w);
        }
        pos[k] = v;
    }
    if (gtab && p.tab_in_lds)
        for (int i = tid; i < tw * tw; i += 256) tab[i] = gtab[i];
    __syncthreads();
    const float* __restrict__ btab = p.tab_in_lds ? tab : gtab;
    const int boff = (p.w - 1) * tw + p.w - 1;   // index(q, k) = pos[q] + boff - pos[k]
    const float* __restrict__ dbias = p.bias ? p.bias + (size_t)head * p.spad * p.spad : nullptr;

    const int oc = ot * 64 + wave * 16 + s;      // this lane's own row (MFMA column)
    const int pos_own = pos[oc];                 // oc < nto * 64 = sst

    f4 dsacc[2];                                 // DBIAS: dS of this tile summed over the windows
    dsacc[0] = dsacc[1] = (f4){0.f, 0.f, 0.f, 0.f};

    for (int win = w0; win < w1; ++win) {
        const T* __restrict__ qkv = (const T*)p.qkv + (size_t)win * S * p.ld + head * DP;
        const T* __restrict__ dOp = (const T*)p.dO + (size_t)win * S * p.ldo + head * DP;
        const T* __restrict__ own1 = OWNQ ? qkv : qkv + HD;             // q | k
        const T* __restrict__ own2 = OWNQ ? dOp : qkv + 2 * HD;         // dO | v
        const int ldo2 = OWNQ ? p.ldo : p.ld;
        const T* __restrict__ lp1 = OWNQ ? qkv + HD : qkv;              // k | q
        const T* __restrict__ lp2 = OWNQ ? qkv + 2 * HD : dOp;          // v | dO
        const int ldl2 = OWNQ ? p.ld : p.ldo;
        const size_t srow = ((size_t)win * p.heads + head) * p.sst;

        v8 zero8;
#pragma unroll
        for (int j = 0; j < 8; ++j) zero8[j] = (T)0.f;

        v8 o1[KD], o2[KD];
#pragma unroll
        for (int kd = 0; kd < KD; ++kd) {
            o1[kd] = o2[kd] = zero8;
            if (oc < S) {
                o1[kd] = *(const v8*)(own1 + (size_t)oc * p.ld + kd * 32 + g * 8);
                o2[kd] = *(const v8*)(own2 + (size_t)oc * ldo2 + kd * 32 + g * 8);
            }
        }
        float lse_o = 0.f, del_o = 0.f;
        if constexpr (MODE == AB_DQ || MODE == AB_DBIAS) {
            lse_o = p.lse[srow + oc];
            del_o = p.delta[srow + oc];
        }

        // staging role of this thread: 16-byte chunk e = i * 256 + tid of the tile's 32 x CH chunks -> loop row e / CH, chunk e % CH
        constexpr int NST = (32 * CH + 255) / 256;   // 1 (DP 32, 64) or 2 (DP 96)
        constexpr int NTRA = NTR > 0 ? NTR : 1;
        v8 sreg[NTRA][NST];
        auto load_stage = [&](int t) {
#pragma unroll
            for (int m = 0; m < NTR; ++m)
#pragma unroll
                for (int i = 0; i < NST; ++i) {
                    const int e = i * 256 + tid, row_l = e / CH, ch = e - row_l * CH;
                    const int row = t * 32 + row_l;
                    v8 val = zero8;
                    if (row_l < 32 && row < S) val = *(const v8*)((m == 0 ? lp1 : lp2) + (size_t)row * (m == 0 ? p.ld : ldl2) + ch * 8);
                    sreg[m][i] = val;
                }
        };

        float m_run = -3.0e38f, l_run = 0.f, d_run = 0.f;   // STATS
        f4 acc1[DB], acc2[DB];                              // dQ^T | dK^T, dV^T: [channel db * 16 + g * 4 + r][own row]
#pragma unroll
        for (int db = 0; db < DB; ++db) acc1[db] = acc2[db] = (f4){0.f, 0.f, 0.f, 0.f};

        if constexpr (NTR > 0) load_stage(t0);
        for (int t = t0; t < t1; ++t) {
            T* xt = xt_base + ((t - t0) & 1) * NTR * XT;
            if constexpr (NTR > 0) {
#pragma unroll
                for (int m = 0; m < NTR; ++m)
#pragma unroll
                    for (int i = 0; i < NST; ++i) {
                        const int e = i * 256 + tid, row_l = e / CH, ch = e - row_l * CH;
                        if (row_l < 32) {
                            // slot of loop row jb * 16 + g * 4 + r inside the 32-wide contraction: g * 8 + jb * 4 + r (the B operand built below)
                            const int slot = ((row_l >> 2) & 3) * 8 + ((row_l >> 4) & 1) * 4 + (row_l & 3);
#pragma unroll
                            for (int j = 0; j < 8; ++j) xt[m * XT + (ch * 8 + j) * AB_VROW + slot] = sreg[m][i][j];
                        }
                    }
                __syncthreads();   // tile t staged; the other buffer is free: its readers passed this barrier
                if (t + 1 < t1) load_stage(t + 1);
            }

            // score^T and dP^T tiles: lane holds loop rows t * 32 + jb * 16 + g * 4 + r of own row oc
            f4 sc[2], dp[2];
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const int lrow = t * 32 + jb * 16 + s;
                f4 a = (f4){0.f, 0.f, 0.f, 0.f}, b = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kd = 0; kd < KD; ++kd) {
                    v8 f1 = zero8, f2 = zero8;
                    if (lrow < S) {
                        f1 = *(const v8*)(lp1 + (size_t)lrow * p.ld + kd * 32 + g * 8);
                        f2 = *(const v8*)(lp2 + (size_t)lrow * ldl2 + kd * 32 + g * 8);
                    }
                    a = Op16<T>::mfma(f1, o1[kd], a);
                    b = Op16<T>::mfma(f2, o2[kd], b);
                }
                sc[jb] = a;
                dp[jb] = b;
            }
            // scores: scale, bias, validity
            bool valid[2][4];
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const int l0 = t * 32 + jb * 16 + g * 4;
                const int4 pl = *(const int4*)(pos + l0);
                const int plv[4] = {pl.x, pl.y, pl.z, pl.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = l0 + r;
                    const bool ok = lr < S && oc < S;
                    float bv = 0.f;
                    if (ok) {
                        const int q = OWNQ ? oc : lr, k = OWNQ ? lr : oc;
                        if (dbias) bv = dbias[(size_t)q * p.spad + k];
                        else if (pos_own >= 0 && plv[r] >= 0) bv = btab[OWNQ ? pos_own + boff - plv[r] : plv[r] + boff - pos_own];
                    }
                    valid[jb][r] = ok;
                    sc[jb][r] = sc[jb][r] * p.scale + bv;
                }
            }

            if constexpr (MODE == AB_STATS) {
                float mx = -3.0e38f;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (t * 32 + jb * 16 + g * 4 + r >= S) sc[jb][r] = -3.0e38f;   // padded keys
                        mx = fmaxf(mx, sc[jb][r]);
                    }
                mx = max_xor32(max_xor16(mx));
                const float mn = fmaxf(m_run, mx);
                const float alpha = __expf(m_run - mn);
                m_run = mn;
                float rs = 0.f, rd = 0.f;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __expf(sc[jb][r] - mn);
                        rs += e;
                        rd += e * dp[jb][r];
                    }
                l_run = l_run * alpha + rs;   // per-lane partial sums (alpha is identical in the 4 lanes of a query); reduced at the end
                d_run = d_run * alpha + rd;
            } else {
                // P = exp(s - lse), dS = P * (dP - delta), all fp32; the loop rows' statistics when the own rows are keys
                float lse_l[2][4], del_l[2][4];
                if constexpr (MODE == AB_DKV) {
#pragma unroll
                    for (int jb = 0; jb < 2; ++jb) {
                        const int l0 = t * 32 + jb * 16 + g * 4;   // < pad32(S) <= sst
                        const float4 a = *(const float4*)(p.lse + srow + l0), b = *(const float4*)(p.delta + srow + l0);
                        lse_l[jb][0] = a.x; lse_l[jb][1] = a.y; lse_l[jb][2] = a.z; lse_l[jb][3] = a.w;
                        del_l[jb][0] = b.x; del_l[jb][1] = b.y; del_l[jb][2] = b.z; del_l[jb][3] = b.w;
                    }
                }
                v8 pf = zero8, df = zero8;
#pragma unroll
                for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float lse = MODE == AB_DKV ? lse_l[jb][r] : lse_o;
                        const float del = MODE == AB_DKV ? del_l[jb][r] : del_o;
                        const float pv = valid[jb][r] ? __expf(sc[jb][r] - lse) : 0.f;
                        const float ds = pv * (dp[jb][r] - del);
                        if constexpr (MODE == AB_DBIAS) dsacc[jb][r] += ds;
                        pf[jb * 4 + r] = (T)pv;
                        df[jb * 4 + r] = sat16<T>(ds);
                    }
                if constexpr (NTR > 0) {
#pragma unroll
                    for (int db = 0; db < DB; ++db) {
                        const v8 x1 = *(const v8*)(xt + (db * 16 + s) * AB_VROW + g * 8);
                        acc1[db] = Op16<T>::mfma(x1, df, acc1[db]);
                        if constexpr (MODE == AB_DKV) {
                            const v8 x2 = *(const v8*)(xt + XT + (db * 16 + s) * AB_VROW + g * 8);
                            acc2[db] = Op16<T>::mfma(x2, pf, acc2[db]);
                        }
                    }
                }
            }
        }

        if constexpr (MODE == AB_STATS) {
            l_run = sum_xor32(sum_xor16(l_run));
            d_run = sum_xor32(sum_xor16(d_run));
            if (g == 0) {   // oc < sst always: rows beyond S get zeros
                p.lse[srow + oc] = oc < S ? m_run + __logf(l_run) : 0.f;
                p.delta[srow + oc] = oc < S ? d_run / l_run : 0.f;
            }
        }
        if constexpr (MODE == AB_DQ || MODE == AB_DKV) {
            if (oc < S) {
                T* dst = (T*)p.dqkv + ((size_t)win * S + oc) * p.ld + head * DP + (MODE == AB_DKV ? HD : 0) + g * 4;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    v4 a, b;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        a[r] = sat16<T>(acc1[db][r] * p.scale);
                        b[r] = sat16<T>(acc2[db][r]);
                    }
                    *(v4*)(dst + db * 16) = a;
                    if constexpr (MODE == AB_DKV) *(v4*)(dst + HD + db * 16) = b;
                }
            }
        }
    }

    if constexpr (MODE == AB_DBIAS) {
        if (oc < S) {
            float* out = p.dsum + ((size_t)head * S + oc) * S;
#pragma unroll
            for (int jb = 0; jb < 2; ++jb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = t0 * 32 + jb * 16 + g * 4 + r;
                    if (k < S) out[k] = p.accumulate ? out[k] + dsacc[jb][r] : dsacc[jb][r];
                }
        }
    }
}

// d_table[h][(dy + w - 1) * (2w - 1) + dx + w - 1] += sum over the queries (yq, xq) in raster order of dssum[h][q][k], k = (yq - dy, xq - dx) inside the window
__global__ __launch_bounds__(256) void rel_table_gather_kernel(const float* __restrict__ dssum, float* __restrict__ d_table, int S, int w, int ng) {
    const int tw = 2 * w - 1;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= tw * tw) return;
    const int head = blockIdx.y;
    const int iy = idx / tw, dy = iy - (w - 1), dx = idx - iy * tw - (w - 1);
    const float* __restrict__ src = dssum + (size_t)head * S * S;
    float sum = 0.f;
    for (int yq = max(0, dy); yq < min(w, w + dy); ++yq)
        for (int xq = max(0, dx); xq < min(w, w + dx); ++xq) {
            const int q = ng + yq * w + xq, k = ng + (yq - dy) * w + (xq - dx);
            sum += src[(size_t)q * S + k];
        }
    d_table[(size_t)head * tw * tw + idx] += sum;
}

constexpr size_t AB_LDS_MAX = 150 * 1024;

template <typename T, int DP, int MODE>
int launch_phase(AttnBwdParams& p, int64_t grid, hipStream_t stream) {
    constexpr int NTR = MODE == AB_DQ ? 1 : (MODE == AB_DKV ? 2 : 0);
    const int tw = 2 * p.w - 1;
    const size_t fixed = (size_t)2 * NTR * DP * AB_VROW * 2 + (size_t)p.sst * 4;
    const size_t tabb = p.rel_table ? (size_t)tw * tw * 4 : 0;
    if (fixed > AB_LDS_MAX) {
        set_error("bwd_window_attention_long: %d tokens per window exceed the position table in LDS", p.S);
        return FVIT_EINVAL;
    }
    p.tab_in_lds = tabb > 0 && fixed + tabb <= AB_LDS_MAX;
    const size_t lds = fixed + (p.tab_in_lds ? tabb : 0);
    static DeviceOnce once;   // opt in to > 64 KiB of dynamic LDS, once per device and kernel instance
    if (once.first_on_current_device())
        (void)hipFuncSetAttribute((const void*)attn_bwd_long_kernel<T, DP, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AB_LDS_MAX);
    if (grid <= 0 || grid > 0x7fffffff) {
        set_error("bwd_window_attention_long: grid too large");
        return FVIT_EINVAL;
    }
    hipLaunchKernelGGL((attn_bwd_long_kernel<T, DP, MODE>), dim3((unsigned)grid), dim3(256), lds, stream, p);
    return check_launch("attn_bwd_long_kernel");
}

template <typename T, int DP>
int launch_all(AttnBwdParams& p, float* dbias, float* dssum, hipStream_t stream) {
    const int64_t items = (int64_t)p.nwin * p.heads * p.nto;
    int rc = launch_phase<T, DP, AB_STATS>(p, items, stream);
    if (rc == FVIT_OK) rc = launch_phase<T, DP, AB_DQ>(p, items, stream);
    if (rc == FVIT_OK) rc = launch_phase<T, DP, AB_DKV>(p, items, stream);
    if (rc != FVIT_OK || !dbias) return rc;
    const bool compact = p.rel_table != nullptr;
    p.dsum = compact ? dssum : dbias;
    p.accumulate = compact ? 0 : 1;
    rc = launch_phase<T, DP, AB_DBIAS>(p, (int64_t)p.heads * p.nto * ((p.S + 31) >> 5), stream);
    if (rc != FVIT_OK || !compact) return rc;
    const int tw = 2 * p.w - 1;
    hipLaunchKernelGGL(rel_table_gather_kernel, dim3((tw * tw + 255) / 256, p.heads), dim3(256), 0, stream, (const float*)dssum, dbias, p.S, p.w, p.ng);
    return check_launch("rel_table_gather_kernel");
}

size_t stats_floats(int64_t nwin, int64_t S, int64_t heads) { return (size_t)(2 * nwin * heads * round_up64(S, 64)); }

}  // namespace
}  // namespace fvit

using namespace fvit;

extern "C" {

size_t fvit_bwd_window_attention_long_workspace(int32_t nwin, int32_t S, int32_t heads, int32_t D, int32_t rel_w) {
    (void)D;
    if (nwin <= 0 || S <= 0 || heads <= 0) return 0;
    return (stats_floats(nwin, S, heads) + (rel_w > 0 ? (size_t)heads * S * S : 0)) * sizeof(float);
}

int fvit_bwd_window_attention_long(int32_t dtype, const void* qkv, int32_t ld, const void* dO, int32_t ldo, const float* bias, int32_t spad,
                                   const float* rel_table, int32_t rel_w, int32_t rel_ng, float scale, void* dqkv, float* dbias, void* workspace,
                                   size_t workspace_bytes, int32_t nwin, int32_t S, int32_t heads, int32_t D, fvit_stream_t stream) {
    if (!qkv || !dO || !dqkv || !workspace) {
        set_error("bwd_window_attention_long: qkv, dO, dqkv and workspace must not be null");
        return FVIT_EINVAL;
    }
    if (nwin <= 0 || S < 1 || heads <= 0 || (D != 32 && D != 64 && D != 96) || ld < 3 * heads * D || ldo < heads * D || (ld % 8) || (ldo % 8)) {
        set_error("bwd_window_attention_long: unsupported arguments nwin=%d S=%d heads=%d D=%d ld=%d ldo=%d (padded head_dim 32 / 64 / 96, row strides multiples of 8)",
                  nwin, S, heads, D, ld, ldo);
        return FVIT_EINVAL;
    }
    if (bias && rel_table) {
        set_error("bwd_window_attention_long: give the dense bias table or the compact one, not both");
        return FVIT_EINVAL;
    }
    if (bias && spad < S) {
        set_error("bwd_window_attention_long: dense bias table of stride %d for S=%d tokens", spad, S);
        return FVIT_EINVAL;
    }
    if (rel_table && (rel_w <= 0 || rel_ng < 0 || rel_ng + rel_w * rel_w != S)) {
        set_error("bwd_window_attention_long: bias table geometry w=%d n_g=%d does not cover S=%d tokens (need n_g + w^2 == S)", rel_w, rel_ng, S);
        return FVIT_EINVAL;
    }
    const size_t nstat = stats_floats(nwin, S, heads);
    const bool need_sum = rel_table && dbias;
    const size_t need = (nstat + (need_sum ? (size_t)heads * S * S : 0)) * sizeof(float);
    if (workspace_bytes < need) {
        set_error("bwd_window_attention_long: workspace of %zu bytes, %zu needed (fvit_bwd_window_attention_long_workspace)", workspace_bytes, need);
        return FVIT_EWORKSPACE;
    }
    AttnBwdParams p;
    p.qkv = qkv; p.dO = dO; p.dqkv = dqkv; p.bias = bias; p.rel_table = rel_table;
    p.lse = (float*)workspace; p.delta = p.lse + nstat / 2; p.dsum = nullptr;
    p.ld = ld; p.ldo = ldo; p.nwin = nwin; p.S = S; p.heads = heads; p.spad = bias ? spad : 0;
    p.w = rel_table ? rel_w : 1; p.ng = rel_table ? rel_ng : S;
    p.sst = round_up(S, 64); p.nto = p.sst / 64; p.tab_in_lds = 0; p.accumulate = 0; p.scale = scale;
    float* dssum = (float*)workspace + nstat;
    hipStream_t st = (hipStream_t)stream;
#define FVIT_ABL_D(T_) (D == 32 ? launch_all<T_, 32>(p, dbias, dssum, st) : D == 64 ? launch_all<T_, 64>(p, dbias, dssum, st) : launch_all<T_, 96>(p, dbias, dssum, st))
    if (dtype == FVIT_F16) return FVIT_ABL_D(_Float16);
    if (dtype == FVIT_BF16) return FVIT_ABL_D(__bf16);
#undef FVIT_ABL_D
    set_error("bwd_window_attention_long: operand dtype %d not supported", dtype);
    return FVIT_EINVAL;
}

}  // extern "C"
