// fvit_conv_gemm.hip -- 3x3 convolution (pad 1, stride 1 or 2) on channels-last 16-bit maps as an implicit
// GEMM on the MFMA cores, with the whole conv-side epilogue fused (gfx950):
//
//   out[b,yo,xo,co] = act( sum_{ky,kx,ci} in[b, yo*s+ky-1, xo*s+kx-1, ci] * w[co,ky,kx,ci] + bias[co] ) (+ res[b,yo,xo,co])
//
// Replaces, in deploy mode, the MIOpen convolution + bias/BatchNorm + ReLU/GELU + residual passes of
// PatchEmbed.conv_down[3..5] (FV:462-464), ConvBlock (FV:502-512) and Downsample.reduction (FV:435):
// BatchNorm (eval) and the layer scale are folded into w/bias at load (conv_runtime.py), so one kernel does
// what PyTorch-ROCm spreads over a conv, an OpTensor pass and one or two elementwise passes.
//
// Design: it is the GEMM of fvit_gemm.hip (M = B*Ho*Wo output pixels, N = Cout, K = 9*Cin) whose A tile
// is gathered on the fly: with channels-last input one (ky,kx) tap of one pixel is a contiguous run of
// Cin 16-bit values, so a K step of 64 channels is one 128-byte row per output pixel.  The gather is done
// by the per-lane SOURCE address of the 16-byte global_load_lds (no im2col buffer, no VGPR round trip);
// out-of-image taps read a caller-provided zero page.  Weights in channels-last layout [Cout][3][3][Cin]
// are already the K-major B^T matrix.  Tiles: 64*WM pixels x 64*WN channels per workgroup of 4 waves
// (WM x WN = 2x2 for Cout % 128 == 0, 4x1 = 256 pixels x 64 channels otherwise), BK = 64, double-buffered
// LDS, one barrier per K step, swizzled fragment reads, XCD-aware tile order, 16 consecutive output channels
// per lane in the epilogue (32-byte stores, 16-byte residual loads).
#include "fvit_conv.h"

namespace fvit {
namespace {

struct ConvParams {
    const void* in;
    const void* w;       // [Cout][9*Cin]
    const float* bias;   // [Cout] or null
    const void* res;     // [M][Cout] or null
    void* out;           // [M][Cout]
    const void* zeros;   // >= 128 bytes of zeros
    int B, Hi, Wi, Cin, Cout, Ho, Wo, stride, act;
    int M, tiles_m, tiles_n;
    int ablate;   // experiment knob (wrong results when non-zero): 1 no X gather, 2 no W staging, 4 no MFMA, 8 no epilogue
    int wterms;   // weight terms (conv3x3_kernel only): 2 = rows [hi | lo] of 2 x 9 x Cin columns, every K step of the lo image re-reads the
                  // activation tile of the same (tap, channel) step -- the conv's weights to ~22 bits, its maps still rounded once
    // two-term MAPS (r05, conv3x3_kernel<.., PX = true>; fvit_conv3x3_nhwc_px): a map is a pair of 16-bit planes, value = hi + lo
    const void* in_lo;    // lo plane of the input or null.  With it (needs wterms == 2) K has a third segment: in.w_hi + in.w_lo + in_lo.w_hi
    const void* res_lo;   // lo plane of the residual or null
    void* out_lo;         // lo plane of the output (lo = round(y - hi)) or null
    float* out_f32;       // the output as ONE fp32 map instead of out / out_lo, or null
    int px;               // 1: the two-term-map instance (fvit_conv3x3_nhwc_px)
    // dense K (r06, conv3x3_kernel<.., DENSE = true>; the *_dense entry points): a map whose Cin channels hold only cv real ones (196 of 256, 392 of 448:
    // FasterViT-4) contracts over 9 x cv columns packed back to back -- tap t, channel c at column t * cv + c, the row zero-padded to kd K steps of 64 --
    // instead of 9 x Cin: a 64-wide K step may straddle taps, every lane derives the (tap, channel) of ITS 16-byte chunk.  cv % 8 == 0.
    int cv, kd;
    float inv_cv;
};

__device__ __forceinline__ int swz_x(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int swz_w(int r) { return ((0x78 >> (2 * ((r >> 4) & 3))) & 3) | ((r & 2) << 1); }

// per-wave tile: 64 pixels x 16*NI channels; workgroup tile: 64*WM pixels x 16*NI*WN channels (WM*WN = 4 waves)
// (r06, scripts/r06_calls/call23.sh: a 3-deep ACTIVATION ring -- X(kt + 2) requested while step kt runs, counted vmcnt, 3 x 16 + 2 x 16 KiB = still two
// workgroups per CU -- measured equal to this double buffer on the headline and on FasterViT-4 in both plans: the K step is not waiting for the gather.)
// HALO (r06, stride 1, WM x WN = 2 x 2): the workgroup's 128 pixels are an 8 x 16 PATCH of one image instead of 128 consecutive pixels, and the activation
// operand is staged as the patch's 10 x 18 HALO of one 64-channel chunk -- once per chunk, double buffered -- from which the nine taps (and both weight
// terms) read SHIFTED fragments: LDS row (py + ky) * 18 + px + kx.  The classic form gathers every (tap, chunk) tile separately: each input value crosses
// L2 -> LDS once per tap and per N tile (and per weight term), 3.7 GB per conv at 128 x 56 x 56 x 256 -- 220 of its 650 us
// (profiles/r06_conv3x3_kstep_ablation.log); the halo form moves 180 / 128 = 1.4 x the map per N tile.  K order: plane (hi; PX third segment: lo) > chunk >
// weight term > tap, so the result is not bitwise the classic kernel's (same products, another summation order).  Weights in the classic layout.
constexpr int PHALO_W = PATCH_W + 2, PHALO_ROWS = (PATCH_H + 2) * PHALO_W;   // 180 LDS rows of 128 bytes
constexpr int PHALO_PIECES = (PHALO_ROWS + 7) / 8;      // 23 pieces of 8 rows
constexpr int PHALO_BYTES = PHALO_PIECES * 1024;

template <typename T, int WM, int WN, int NI, bool PX = false, bool DENSE = false, bool HALO = false>
__global__ __launch_bounds__(256, 2) void conv3x3_kernel(ConvParams p) {
    typedef typename Op16<T>::v8 v8;
    static_assert(!HALO || (WM == 2 && WN == 2 && !DENSE), "halo form: 8 x 16 patches on the 2 x 2 wave grid, classic weight layout");
    constexpr int BM = 64 * WM, BN = 16 * NI * WN;
    constexpr int X_BYTES = HALO ? PHALO_BYTES : BM * BK * 2, W_BYTES = BN * BK * 2;
    constexpr int XP = BM / 8 / 4;  // 1-KiB pieces (8 rows) of the X tile each wave stages per K step
    constexpr int HP = (PHALO_PIECES + 3) / 4;   // halo pieces per wave
    constexpr int WPIECES = BN / 8;             // 1-KiB pieces of the W tile (8 rows each)
    constexpr int WP = (WPIECES + 3) / 4;       // per wave (waves beyond WPIECES stage nothing)
    static_assert(2 * (X_BYTES + W_BYTES) <= 80 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) char smem[2 * (X_BYTES + W_BYTES)];   // the two X tiles (halo tiles), then the two W tiles

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;

    const int nblk = gridDim.x, b = blockIdx.x;
    const int q = nblk >> 3, rr = nblk & 7, xcd = b & 7, idx = b >> 3;
    const int v = (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + idx;
    const int tm = v / p.tiles_n, tn = v - tm * p.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;

    const T* __restrict__ In = (const T*)p.in;
    const T* __restrict__ W = (const T*)p.w;
    const T* __restrict__ Z = (const T*)p.zeros;
    const int ldw = DENSE ? p.wterms * p.kd * BK : p.wterms * 9 * p.Cin;

    f4 acc[NI][4];  // [ni][mi]
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    const int g = lane >> 4, s = lane & 15;
    // patch of this workgroup (HALO): image bimg, output rows y0 .. y0 + 7, columns x0 .. x0 + 15 (ragged patches at the right / bottom edges)
    int bimg = 0, y0 = 0, x0 = 0;
    if constexpr (HALO) {
        const int tpx = (p.Wo + PATCH_W - 1) / PATCH_W, tpy = (p.Ho + PATCH_H - 1) / PATCH_H;
        bimg = tm / (tpy * tpx);
        const int rem = tm - bimg * (tpy * tpx);
        const int ty = rem / tpx;
        y0 = ty * PATCH_H;
        x0 = (rem - ty * tpx) * PATCH_W;
    }
    if constexpr (HALO) {
        // ---- per-lane halo state: the HP pieces (8 LDS rows each) this wave stages per (plane, chunk) block; LDS row r = hy * 18 + hx <-> input pixel (y0 - 1 + hy, x0 - 1 + hx) ----
        int hoff[HP];      // element offset of the pixel's channel 0 + this lane's source chunk (valid pixels only)
        int hvalid = 0;    // bit i: piece i of this lane reads a pixel inside the image
        int hchunk[HP];
#pragma unroll
        for (int i = 0; i < HP; ++i) {
            const int piece = wave + 4 * i;
            const int r = piece * 8 + (lane >> 3);
            const int hy = r / PHALO_W, hx = r - hy * PHALO_W;
            const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            const int chunk = ((lane & 7) ^ swz_x(r)) * 8;
            hchunk[i] = chunk;
            const bool ok = piece < PHALO_PIECES && r < PHALO_ROWS && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
            if (ok) hvalid |= 1 << i;
            hoff[i] = ok ? ((bimg * p.Hi + iy) * p.Wi + ix) * p.Cin + chunk : 0;   // (B * H * W * Cin < 2^31: checked by the launcher)
        }
        const int ncc = p.Cin / BK;                            // 64-channel chunks
        const int kpb_hi = p.wterms * 9;                       // K steps of a hi-plane block: weight terms x taps
        const int nblk_hi = ncc, nblk_all = ncc * ((PX && p.in_lo) ? 2 : 1);
        const int nk = nblk_hi * kpb_hi + (nblk_all - nblk_hi) * 9;
        const T* const InLo = (PX && p.in_lo) ? (const T*)p.in_lo : In;
        auto stage_halo = [&](int blk, char* xbuf) {
            const bool lo = blk >= nblk_hi;
            const T* const plane = lo ? InLo : In;
            const int c0 = (lo ? blk - nblk_hi : blk) * BK;
#pragma unroll
            for (int i = 0; i < HP; ++i) {
                const int piece = wave + 4 * i;
                if (piece < PHALO_PIECES) {
                    const T* src = ((hvalid >> i) & 1) ? plane + (hoff[i] + c0) : Z + hchunk[i];
                    glds16(src, xbuf + piece * 1024);
                }
            }
        };
        // weight tile of K step (blk, kin): hi-plane blocks walk [term 0 taps 0..8 | term 1 taps 0..8], lo-plane blocks the hi image's taps
        auto stage_w = [&](int blk, int kin, char* wbuf) {
            const bool lo = blk >= nblk_hi;
            const int c0 = (lo ? blk - nblk_hi : blk) * BK;
            const int col = kin * p.Cin + c0;                  // kin = term * 9 + tap: column term * 9 * Cin + tap * Cin + c0 of the classic [hi | lo] row
#pragma unroll
            for (int i = 0; i < WP; ++i) {
                const int piece = wave * WP + i;
                if (piece < WPIECES) {
                    const int r = piece * 8 + (lane >> 3);
                    const int c = (lane & 7) ^ swz_w(r);
                    glds16(W + (size_t)min(n0 + r, p.Cout - 1) * ldw + col + c * 8, wbuf + piece * 1024);
                }
            }
        };
        char* const wring = smem + 2 * X_BYTES;
        stage_halo(0, smem);
        stage_w(0, 0, wring);
        int rbase[4], wrow[NI];
#pragma unroll
        for (int i = 0; i < 4; ++i) rbase[i] = (wm * 4 + i) * PHALO_W + s;   // LDS row of pixel (patch row wm * 4 + i, column s) for tap (0, 0)
#pragma unroll
        for (int i = 0; i < NI; ++i) wrow[i] = wn * 16 * NI + (s >> 2) * 4 * NI + i * 4 + (s & 3);
        int blk = 0, kin = 0, kpb = kpb_hi, hb = 0;
        for (int kt = 0; kt < nk; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const int cur = kt & 1;
            // next K step: (blk, kin + 1) or the first step of the next block; the next block's halo is requested at the FIRST step of this block
            int nblk_ = blk, nkin = kin + 1;
            if (nkin == kpb) { nblk_ = blk + 1; nkin = 0; }
            if (kt + 1 < nk) stage_w(nblk_, nkin, wring + (cur ^ 1) * W_BYTES);
            if (kin == 0 && blk + 1 < nblk_all) stage_halo(blk + 1, smem + (hb ^ 1) * X_BYTES);
            const char* xt = smem + hb * X_BYTES;
            const char* wt = wring + cur * W_BYTES;
            const int tap = kin >= 9 ? kin - 9 : kin;
            const int ky = (tap * 11) >> 5, kx = tap - ky * 3;
            const int rsh = ky * PHALO_W + kx;
            v8 xf[2][4], wf[2][NI];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int c = kk * 4 + g;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = rbase[i] + rsh;
                    xf[kk][i] = *(const v8*)(xt + r * 128 + ((c ^ swz_x(r)) << 4));
                }
#pragma unroll
                for (int i = 0; i < NI; ++i) wf[kk][i] = *(const v8*)(wt + wrow[i] * 128 + ((c ^ swz_w(wrow[i])) << 4));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = Op16<T>::mfma(wf[kk][ni], xf[kk][mi], acc[ni][mi]);
            blk = nblk_; kin = nkin;
            if (kin == 0) { hb ^= 1; kpb = blk >= nblk_hi ? 9 : kpb_hi; }
        }
    } else {
    // ---- per-lane gather state for the rows this lane stages (fixed for the whole K loop) ----
    int64_t rowoff[XP];     // element offset of in[b][yo*s-1][xo*s-1][0] from the plane's base (may lie outside the image; only used when the tap is valid)
    int rowmask[XP];        // bit ky*3+kx set <=> tap inside the image
    int rowchunk[XP];       // swizzled 16-byte chunk this lane copies
#pragma unroll
    for (int i = 0; i < XP; ++i) {
        const int r = (wave * XP + i) * 8 + (lane >> 3);
        const int m = m0 + r;
        int mask = 0;
        int64_t base = 0;
        if (m < p.M) {
            const int hw = p.Ho * p.Wo;
            const int bb = m / hw, rem = m - bb * hw;
            const int yo = rem / p.Wo, xo = rem - yo * p.Wo;
            const int yi = yo * p.stride - 1, xi = xo * p.stride - 1;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
                    if (yi + ky >= 0 && yi + ky < p.Hi && xi + kx >= 0 && xi + kx < p.Wi) mask |= 1 << (ky * 3 + kx);
            base = (((int64_t)bb * p.Hi + yi) * p.Wi + xi) * p.Cin;
        }
        rowoff[i] = base;
        rowmask[i] = mask;
        rowchunk[i] = ((lane & 7) ^ swz_x(r)) * 8;
    }

    const int cpt = p.Cin / BK;  // K steps per tap
    const int nk1 = DENSE ? p.kd : 9 * cpt;     // K steps of one weight term
    // PX: the third K segment reads the LO plane of the input against the hi weights: the plane's base pointer is chosen per segment, the per-row offsets
    // are plain integers (r05 formed the lo address as `hi pointer + (in_lo - in)`: arithmetic across two allocations)
    const T* const InLo = (PX && p.in_lo) ? (const T*)p.in_lo : In;
    auto stage_x = [&](int kt, char* xbuf) {
        const int seg = kt >= 2 * nk1 ? 2 : (kt >= nk1 ? 1 : 0);
        const int kta = kt - seg * nk1;              // the activation side wraps at every segment
        const T* const plane = (PX && seg == 2) ? InLo : In;
        if constexpr (DENSE) {
            // per-lane (tap, channel) of the lane's 16-byte chunk: k = 64 kta + chunk; tap = floor(k / cv) through the reciprocal ((k + 0.5) / cv is
            // never within 0.5 / cv of an integer: exact in fp32); columns >= 9 cv (the zero-padded tail of the last K step) give tap 9 = never valid
            const int k0 = kta * BK;
#pragma unroll
            for (int i = 0; i < XP; ++i) {
                const int k = k0 + rowchunk[i];
                const int tap = (int)(((float)k + 0.5f) * p.inv_cv);
                const int ci = k - tap * p.cv;
                const int ky = (tap * 11) >> 5, kx = tap - ky * 3;
                const int toff = (ky * p.Wi + kx) * p.Cin + ci;
                const T* src = ((rowmask[i] >> tap) & 1) ? plane + (rowoff[i] + toff) : Z + rowchunk[i];
                glds16(src, xbuf + (wave * XP + i) * 1024);
            }
        } else {
        const int tap = kta / cpt, ci0 = (kta - tap * cpt) * BK;
        const int ky = tap / 3, kx = tap - ky * 3;
        const int64_t toff = (ky * p.Wi + kx) * p.Cin + ci0;
        if (!(p.ablate & 1))
#pragma unroll
        for (int i = 0; i < XP; ++i) {
            const T* src = ((rowmask[i] >> tap) & 1) ? plane + (rowoff[i] + toff + rowchunk[i]) : Z + rowchunk[i];
            glds16(src, xbuf + (wave * XP + i) * 1024);
        }
        }
    };
    auto stage_w = [&](int kt, char* wbuf) {
        const int seg = kt >= 2 * nk1 ? 2 : (kt >= nk1 ? 1 : 0);
        const int ktw = seg == 2 ? kt - 2 * nk1 : kt;   // segments 0 / 1 / 2 meet the weight images hi / lo / hi
        if (!(p.ablate & 2))
#pragma unroll
        for (int i = 0; i < WP; ++i) {
            const int piece = wave * WP + i;
            if (piece < WPIECES) {
                const int r = piece * 8 + (lane >> 3);
                const int c = (lane & 7) ^ swz_w(r);
                glds16(W + (size_t)min(n0 + r, p.Cout - 1) * ldw + ktw * BK + c * 8, wbuf + piece * 1024);   // (ragged last N tile: rows clamped, never stored)
            }
        }
    };

    const int nk = (p.wterms + ((PX && p.in_lo) ? 1 : 0)) * nk1;
    char* const wring = smem + 2 * X_BYTES;
    stage_x(0, smem);
    stage_w(0, wring);

    // weight row for A-row slot s of fragment i: wn*16*NI + (s>>2)*4*NI + i*4 + (s&3)  => lane (g, .) owns the 4*NI
    // consecutive channels wn*16*NI + g*4*NI .. ; with NI = 4 this is the layout of fvit_gemm.hip
    int xrow[4], wrow[NI];
#pragma unroll
    for (int i = 0; i < 4; ++i) xrow[i] = wm * 64 + i * 16 + s;
#pragma unroll
    for (int i = 0; i < NI; ++i) wrow[i] = wn * 16 * NI + (s >> 2) * 4 * NI + i * 4 + (s & 3);

    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int cur = kt & 1;
        if (kt + 1 < nk) { stage_x(kt + 1, smem + (cur ^ 1) * X_BYTES); stage_w(kt + 1, wring + (cur ^ 1) * W_BYTES); }
        const char* xt = smem + cur * X_BYTES;
        const char* wt = wring + cur * W_BYTES;
        // both 32-deep halves of the K step are read up front: one exposed LDS round trip per step instead of three (see fvit_gemm.hip)
        v8 xf[2][4], wf[2][NI];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int c = kk * 4 + g;
#pragma unroll
            for (int i = 0; i < 4; ++i) xf[kk][i] = *(const v8*)(xt + xrow[i] * 128 + ((c ^ swz_x(xrow[i])) << 4));
#pragma unroll
            for (int i = 0; i < NI; ++i) wf[kk][i] = *(const v8*)(wt + wrow[i] * 128 + ((c ^ swz_w(wrow[i])) << 4));
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(p.ablate & 4))
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = Op16<T>::mfma(wf[kk][ni], xf[kk][mi], acc[ni][mi]);
    }
    }
    if (p.ablate & 8) return;

    // ---- epilogue: lane holds out[m][nb .. nb + 4*NI - 1] for 4 pixels m ----
    // output pixel of row fragment mi (linear index into [B][Ho][Wo]; p.M = "no such pixel": ragged patch edge)
    auto rowm = [&](int mi) {
        if constexpr (HALO) {
            const int y = y0 + wm * 4 + mi, x = x0 + s;
            return (y < p.Ho && x < p.Wo) ? (bimg * p.Ho + y) * p.Wo + x : p.M;
        } else {
            return m0 + wm * 64 + mi * 16 + s;
        }
    };
    constexpr int NC = 4 * NI;  // consecutive channels per lane (16 or 8)
    typedef T vout __attribute__((ext_vector_type(NC)));
    const int nb = n0 + wn * 16 * NI + g * NC;
    if (nb >= p.Cout) return;   // ragged last N tile (Cout % 128 == 64 on 128-column tiles): these channels do not exist; no barrier follows
    float bias[NC];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        const f4 t = p.bias ? *(const f4*)(p.bias + nb + j * 4) : (f4){0.f, 0.f, 0.f, 0.f};
        bias[j * 4 + 0] = t[0]; bias[j * 4 + 1] = t[1]; bias[j * 4 + 2] = t[2]; bias[j * 4 + 3] = t[3];
    }
    T* O = (T*)p.out;
    const T* R = (const T*)p.res;
    if constexpr (PX) {
        // two-term maps: the residual is hi + lo (fp32 sum), the result leaves as hi = round(y), lo = round(y - hi) -- or as one fp32 map for a
        // consumer that is not an MFMA operand (the next transformer level's partition).  GELU by gelu_erf (erfc form, a few ulp): the polynomial's 5e-5 is a
        // systematic error of the same size as the roundings this path removes.
        const T* RL = (const T*)p.res_lo;
        T* OL = (T*)p.out_lo;
        float* OF = p.out_f32;
        // the activation is dispatched ONCE (a runtime `act` inside the unrolled per-element loops keeps every body in the instruction stream)
        auto px_epilogue = [&](auto act_tag) {
            constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int m = rowm(mi);
                if (m < p.M) {
                    float y[NC];
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float v = acc[ni][mi][r] + bias[ni * 4 + r];
                            if (ACT == 1) v = fmaxf(v, 0.f);
                            y[ni * 4 + r] = v;
                        }
                    if constexpr (ACT == 2) gelu_erf_each<NC>(y);   // interleaved chains (fvit_common.h), bitwise gelu_erf per value
                    if (R) {
                        const vout rv = *(const vout*)(R + (size_t)m * p.Cout + nb);
#pragma unroll
                        for (int j = 0; j < NC; ++j) y[j] += (float)rv[j];
                        if (RL) {
                            const vout rl = *(const vout*)(RL + (size_t)m * p.Cout + nb);
#pragma unroll
                            for (int j = 0; j < NC; ++j) y[j] += (float)rl[j];
                        }
                    }
                    if (OF) {
#pragma unroll
                        for (int j = 0; j < NC; j += 4) *(f4*)(OF + (size_t)m * p.Cout + nb + j) = (f4){y[j], y[j + 1], y[j + 2], y[j + 3]};
                    } else {
                        vout oh, ol;
#pragma unroll
                        for (int j = 0; j < NC; ++j) {
                            oh[j] = sat16<T>(y[j]);
                            ol[j] = sat16<T>(y[j] - (float)oh[j]);
                        }
                        *(vout*)(O + (size_t)m * p.Cout + nb) = oh;
                        if (OL) *(vout*)(OL + (size_t)m * p.Cout + nb) = ol;
                    }
                }
            }
        };
        if (p.act == 0) px_epilogue(IntTag<0>{});
        else if (p.act == 1) px_epilogue(IntTag<1>{});
        else px_epilogue(IntTag<2>{});
        return;
    }
    dispatch_epilogue(p.act, R != nullptr, [&](auto act_tag, auto res_tag) {
        constexpr int ACT = decltype(act_tag)::value;
        constexpr bool RES = decltype(res_tag)::value != 0;
        // residual rows of all four pixels first (r03): the residual map IS the output map (in-place update), so in one
        // load-update-store loop every store had to stay ahead of the next pixel's load -- four dependent round trips per lane
        vout rvs[4];
        if (RES) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) rvs[mi] = *(const vout*)(R + (size_t)min(rowm(mi), p.M - 1) * p.Cout + nb);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int m = rowm(mi);
            if (m < p.M) {
                vout rv;
                if (RES) rv = rvs[mi];
                vout ov;
                float yv[NI * 4];
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) {
                    const f4 a = acc[ni][mi];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float y = a[r] + bias[ni * 4 + r];
                        if (ACT == 1) y = fmaxf(y, 0.f);
                        yv[ni * 4 + r] = y;
                    }
                }
                if constexpr (ACT == 2) gelu_fast_each<NI * 4>(yv);   // interleaved Horner chains, bitwise gelu_fast
#pragma unroll
                for (int j = 0; j < NI * 4; ++j) ov[j] = (T)(RES ? yv[j] + (float)rv[j] : yv[j]);
                *(vout*)(O + (size_t)m * p.Cout + nb) = ov;
            }
        }
    });
}

using ConvKernel = void (*)(ConvParams);
template <typename T>
ConvKernel gemm_kernel(ConvRoute r) {
    switch (r) {
    case CR_PATCH: return conv3x3_kernel<T, 2, 2, 4, false, false, true>;
    case CR_PATCH_PX: return conv3x3_kernel<T, 2, 2, 4, true, false, true>;
    case CR_T128: return conv3x3_kernel<T, 2, 2, 4, false, false>;
    case CR_T128_DENSE: return conv3x3_kernel<T, 2, 2, 4, false, true>;
    case CR_T128_PX: return conv3x3_kernel<T, 2, 2, 4, true, false>;
    case CR_T128_PX_DENSE: return conv3x3_kernel<T, 2, 2, 4, true, true>;
    case CR_T64: return conv3x3_kernel<T, 2, 2, 2, false, false>;
    case CR_T64_DENSE: return conv3x3_kernel<T, 2, 2, 2, false, true>;
    case CR_T64_PX: return conv3x3_kernel<T, 2, 2, 2, true, false>;
    case CR_T64_PX_DENSE: return conv3x3_kernel<T, 2, 2, 2, true, true>;
    default: return conv3x3_kernel<T, 4, 1, 4>;
    }
}

// dense rows contract over cv real channels per tap, kd K steps; classic rows (cv = 0) over all Cin
template <typename T>
int launch(ConvRoute r, const ConvRouteInfo& info, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream) {
    if (ablate_skip(32)) return FVIT_OK;
    const int Ho = out_size(c.Hi, c.stride), Wo = out_size(c.Wi, c.stride), M = c.B * Ho * Wo;
    const bool px = call_is_px(c), dense = r >= CR_T128 && ((r - CR_T128) & 1), patch = r == CR_PATCH || r == CR_PATCH_PX;
    ConvParams p;
    p.in = c.in; p.w = dense ? w.dense : w.classic; p.bias = c.bias; p.res = c.residual; p.out = c.out; p.zeros = c.zeros;
    p.B = c.B; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.Cin; p.Cout = c.Cout; p.Ho = Ho; p.Wo = Wo; p.stride = c.stride; p.act = c.act; p.M = M;
    p.ablate = px ? 0 : diag_knob("conv_ablate"); p.wterms = w.terms;
    p.in_lo = c.in_lo; p.res_lo = c.residual_lo; p.out_lo = c.out_lo; p.out_f32 = c.out_f32; p.px = px;
    p.cv = dense ? w.cin_valid : 0; p.kd = dense ? (9 * p.cv + BK - 1) / BK : 0; p.inv_cv = dense ? 1.0f / (float)p.cv : 0.f;
    p.tiles_m = patch ? c.B * ((Ho + PATCH_H - 1) / PATCH_H) * ((Wo + PATCH_W - 1) / PATCH_W) : (M + info.bm - 1) / info.bm;
    p.tiles_n = (c.Cout + info.bn - 1) / info.bn;   // 128-column tiles: the last one may be ragged
    const double flops = 2.0 * M * (double)c.Cout * 9.0 * (dense ? p.cv : c.Cin);
    const double bytes = 2.0 * ((double)c.B * c.Hi * c.Wi * c.Cin * (c.in_lo ? 2.0 : 1.0) +
                                (double)M * c.Cout * ((c.residual ? (c.residual_lo ? 2.0 : 1.0) : 0.0) + ((c.out_lo || c.out_f32) ? 2.0 : 1.0)) + 9.0 * w.terms * c.Cin * c.Cout);
    ProfScope prof(FVIT_K_CONV, flops, bytes, stream);   // (the second weight term is a precision cost, not algorithmic FLOPs)
    prof_note(info.name, p.tiles_m * p.tiles_n);
    hipLaunchKernelGGL(gemm_kernel<T>(r), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, stream, p);
    return check_launch(info.name);
}

}  // namespace

int launch_conv_gemm(int dtype, ConvRoute r, const ConvRouteInfo& info, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream) {
    return dtype == FVIT_F16 ? launch<_Float16>(r, info, c, w, stream) : launch<__bf16>(r, info, c, w, stream);
}

}  // namespace fvit
