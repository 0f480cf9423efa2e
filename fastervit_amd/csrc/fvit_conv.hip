// fvit_conv.hip -- 3x3 convolution (pad 1, stride 1 or 2) on channels-last 16-bit maps as an implicit
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
#include "fvit_common.h"

namespace fvit {

namespace {

constexpr int BK = 64;

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

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// The activation and the residual switch are runtime arguments but must not be runtime branches inside the per-element
// epilogue loops (a uniform branch per output value keeps the compiler from interleaving the 32-64 independent
// bias/GELU/convert chains of a lane): dispatch ONCE per tile to a body specialised on both.
template <int V> struct IntTag { static constexpr int value = V; };
template <typename F>
__device__ __forceinline__ void dispatch_epilogue(int act, bool has_res, F&& body) {
    if (has_res) {
        if (act == 0) body(IntTag<0>{}, IntTag<1>{});
        else if (act == 1) body(IntTag<1>{}, IntTag<1>{});
        else body(IntTag<2>{}, IntTag<1>{});
    } else {
        if (act == 0) body(IntTag<0>{}, IntTag<0>{});
        else if (act == 1) body(IntTag<1>{}, IntTag<0>{});
        else body(IntTag<2>{}, IntTag<0>{});
    }
}

// per-wave tile: 64 pixels x 16*NI channels; workgroup tile: 64*WM pixels x 16*NI*WN channels (WM*WN = 4 waves)
// (r06, scripts/r06_calls/call23.sh: a 3-deep ACTIVATION ring -- X(kt + 2) requested while step kt runs, counted vmcnt, 3 x 16 + 2 x 16 KiB = still two
// workgroups per CU -- measured equal to this double buffer on the headline and on FasterViT-4 in both plans: the K step is not waiting for the gather.)
// HALO (r06, stride 1, WM x WN = 2 x 2): the workgroup's 128 pixels are an 8 x 16 PATCH of one image instead of 128 consecutive pixels, and the activation
// operand is staged as the patch's 10 x 18 HALO of one 64-channel chunk -- once per chunk, double buffered -- from which the nine taps (and both weight
// terms) read SHIFTED fragments: LDS row (py + ky) * 18 + px + kx.  The classic form gathers every (tap, chunk) tile separately: each input value crosses
// L2 -> LDS once per tap and per N tile (and per weight term), 3.7 GB per conv at 128 x 56 x 56 x 256 -- 220 of its 650 us
// (profiles/r06_conv3x3_kstep_ablation.log); the halo form moves 180 / 128 = 1.4 x the map per N tile.  K order: plane (hi; PX third segment: lo) > chunk >
// weight term > tap, so the result is not bitwise the classic kernel's (same products, another summation order).  Weights in the classic layout.
constexpr int PATCH_H = 8, PATCH_W = 16, PHALO_W = PATCH_W + 2, PHALO_ROWS = (PATCH_H + 2) * PHALO_W;   // 180 LDS rows of 128 bytes
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
        // consumer that is not an MFMA operand (the next transformer level's partition).  GELU by the 1.5e-7 erf: the polynomial's 5e-5 is a
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


// ------------------------------------------------------------------------------------------------------------
// Stem convolution: 3x3, stride 2, pad 1, Cin = 3 -> Cout = 64, + folded BatchNorm bias + ReLU (PatchEmbed.conv_down[0..2],
// FV:458-460).  K = 27 is padded to one 32-deep MFMA step: lane (g, s) gathers k slots 8g..8g+7 of pixel s's 3x3x3 patch
// straight from the caller's image (any strides / fp32, fp16 or bf16: the NCHW fp32 input of the model needs no
// conversion pass), the 64x32 weight matrix lives in registers (4 fragments), and the 16-bit channels-last output --
// the largest tensor of the network (B x 112 x 112 x 64) -- is written exactly once.  HBM-bound on that write.
// ------------------------------------------------------------------------------------------------------------
struct StemParams {
    FvitMapView in;      // (B, 3, Hi, Wi)
    const void* w;       // op16 [64][32]: k = ky*9 + kx*3 + c, zero for k >= 27
    const float* bias;   // [64]
    void* out;           // [B][Ho][Wo][64]
    int B, Hi, Wi, Ho, Wo, M;
    const void* w_lo;    // PX (fvit_stem_conv3x3s2_px): the second weight term, same layout; the image is split hi + lo in registers
    float nscale[3], nshift[3];   // U8 instances: the image is uint8 and every gathered byte u of channel c becomes fmaf(u, nscale[c], nshift[c])
};

__device__ __forceinline__ float stem_load(const FvitMapView& v, int64_t off) {
    if (v.dtype == FVIT_F32) return ((const float*)v.data)[off];
    if (v.dtype == FVIT_F16) return (float)((const _Float16*)v.data)[off];
    return (float)((const __bf16*)v.data)[off];
}

// U8: the caller's image is uint8 (FVIT_U8) and is normalised at the load; a tap outside the image is a NORMALISED zero (the reference pads after
// normalising), so the mask is applied behind the fmaf.  The k slots are the float kernel's: the MFMA sees the operands the float kernel sees on the
// normalised fp32 image, and the results are the same bits.
template <typename T, bool PX = false, bool U8 = false>
__global__ __launch_bounds__(256) void stem_conv_kernel(StemParams p) {
    typedef typename Op16<T>::v8 v8;
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, s = lane & 15;
    // weights: fragment ni, A-row slot s -> channel (s>>2)*16 + ni*4 + (s&3): lane (g, .) owns channels 16g .. 16g+15
    const T* __restrict__ W = (const T*)p.w;
    v8 wf[4], wl[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) wf[ni] = *(const v8*)(W + ((s >> 2) * 16 + ni * 4 + (s & 3)) * 32 + g * 8);
    if constexpr (PX) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) wl[ni] = *(const v8*)((const T*)p.w_lo + ((s >> 2) * 16 + ni * 4 + (s & 3)) * 32 + g * 8);
    }
    float bias[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f4 t = *(const f4*)(p.bias + g * 16 + j * 4);
        bias[j * 4 + 0] = t[0]; bias[j * 4 + 1] = t[1]; bias[j * 4 + 2] = t[2]; bias[j * 4 + 3] = t[3];
    }
    T* __restrict__ O = (T*)p.out;
    const int hw = p.Ho * p.Wo;
    const int nblk16 = (p.M + 15) >> 4;
    // this lane's 8 taps (k = 8g + e = ky*9 + kx*3 + c): offsets are pixel independent, computed once
    int64_t toff[8];
    int tky[8], tkx[8];
    float nsc[8], nsh[8];   // U8: the normalisation constants of each tap's channel
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = g * 8 + e;
        const int ky = k / 9, r9 = k - ky * 9, kx = r9 / 3, c = r9 - kx * 3;
        tky[e] = k < 27 ? ky : -100000;  // padded k slots can never be in range
        tkx[e] = kx;
        toff[e] = c * p.in.stride_c + ky * p.in.stride_h + kx * p.in.stride_w;
        if constexpr (U8) {
            nsc[e] = c == 0 ? p.nscale[0] : (c == 1 ? p.nscale[1] : p.nscale[2]);
            nsh[e] = c == 0 ? p.nshift[0] : (c == 1 ? p.nshift[1] : p.nshift[2]);
        }
    }
    // grid-stride over blocks of 16 output pixels; one wave per block
    for (int blk = blockIdx.x * 4 + (threadIdx.x >> 6); blk < nblk16; blk += gridDim.x * 4) {
        const int m = blk * 16 + s;
        const bool ok = m < p.M;
        const int mm = ok ? m : p.M - 1;
        const int bb = mm / hw, rem = mm - bb * hw;
        const int yo = rem / p.Wo, xo = rem - yo * p.Wo;
        const int yi = yo * 2 - 1, xi = xo * 2 - 1;
        const int64_t base = bb * p.in.stride_b + yi * p.in.stride_h + xi * p.in.stride_w;
        v8 xf, xl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int y = yi + tky[e], x = xi + tkx[e];
            const bool inb = y >= 0 && y < p.Hi && x >= 0 && x < p.Wi;
            // always issue the load (clamped to the pixel's own centre tap, which is always inside), then mask
            const int64_t off = inb ? base + toff[e] : base + p.in.stride_h + p.in.stride_w;
            float v0;
            if constexpr (U8) v0 = __builtin_fmaf((float)((const uint8_t*)p.in.data)[off], nsc[e], nsh[e]);
            else v0 = stem_load(p.in, off);
            const float v = inb ? v0 : 0.f;
            xf[e] = (T)v;
            if constexpr (PX) xl[e] = (T)(v - (float)xf[e]);
        }
        f4 acc[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            acc[ni] = Op16<T>::mfma(wf[ni], xf, (f4){0.f, 0.f, 0.f, 0.f});
            if constexpr (PX) {   // image and weights as two terms each (the lo.lo product dropped): the K = 27 conv to ~22 bits
                acc[ni] = Op16<T>::mfma(wl[ni], xf, acc[ni]);
                acc[ni] = Op16<T>::mfma(wf[ni], xl, acc[ni]);
            }
        }
        if (ok) {
            v8 o0, o1;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float y = fmaxf(acc[ni][r] + bias[ni * 4 + r], 0.f);
                    if (ni < 2) o0[ni * 4 + r] = (T)y; else o1[(ni - 2) * 4 + r] = (T)y;
                }
            T* po = O + (size_t)m * 64 + g * 16;
            *(v8*)po = o0;
            *(v8*)(po + 8) = o1;
        }
    }
}


// ------------------------------------------------------------------------------------------------------------
// Halo-tiled 3x3 convolution for Cin = Cout = 64, stride 1 (ConvBlock convs of level 0, FV:502-512).
//
// The implicit GEMM above re-reads every input pixel nine times from L2 (once per tap) and the whole 72-KiB
// weight matrix once per 128-pixel tile: ~220 KiB of L2->LDS traffic per 9.4 MFLOP tile, which is what bounds it.
// Here a workgroup owns an 8 x 16 pixel output tile, brings its 10 x 18 pixel halo into LDS ONCE (23 KiB, LDS-DMA,
// double-buffered across a persistent tile loop) and keeps its weights STATIONARY IN REGISTERS: wave (ch, ph) owns
// output channels 32ch .. 32ch+31 (36 A fragments = 144 VGPRs, loaded once per workgroup) and pixel rows
// 4ph .. 4ph+3.  A 16-pixel MFMA column group is one row of 16 consecutive pixels, so the B fragment of tap
// (ky, kx) is the same LDS image read at a shifted address: row (r + ky), column (s + kx).  With chunk position
// c ^ (hx & 6) (hx = halo column) every ds_read_b128 service group touches each bank once for any shift.
// Per tile and wave: 72 ds_read_b128 for 144 MFMAs; L2->LDS traffic drops ~9x, HBM traffic is the map read + write.
// ------------------------------------------------------------------------------------------------------------
struct HaloParams {
    const void* in;
    const void* w;       // [64][9*64]
    const float* bias;   // [64] or null
    const void* res;     // [M][64] or null
    void* out;           // [M][64]
    const void* zeros;
    int B, H, W, act;
    int tiles_x, tiles_y, strips, tiles;   // edge_tiling(H, W): per image tiles_x * tiles_y plain tiles, then `strips` strip tiles
    int buf_bytes;       // LDS bytes per tile buffer: HALO_BYTES (+ HALO_RES_BYTES with a residual)
    int ablate;          // experiment knob (results are wrong when non-zero): 1 no MFMA loop, 2 no halo/residual DMA, 4 no stores, 8 no epilogue math
    const float* ln_w;   // LN instance only (fvit_conv3x3_c64_ln2d): LayerNorm2d weight / bias [64] applied to the stored map
    const float* ln_b;
    float ln_eps;
};

constexpr int HALO_TH = 8, HALO_TW = 16, HALO_PW = HALO_TW + 2, HALO_PH = HALO_TH + 2;
constexpr int HALO_PIECES = (HALO_PH * HALO_PW + 7) / 8;       // 1-KiB pieces of 8 halo pixels
constexpr int HALO_BYTES = HALO_PIECES * 1024;
constexpr int HALO_RES_BYTES = HALO_TH * HALO_TW * 128;         // the tile's residual pixels, staged next to the halo
constexpr int HALO_BUF = HALO_BYTES + HALO_RES_BYTES;

constexpr int HALO_LN_LDS = 1024 + 2 * HALO_BUF + 1024;        // LN instance: 81 920 B, exactly half a CU's LDS (two workgroups per CU)

// Tiling of an H x W map by conv3x3_c64_halo_kernel and stem_fused_kernel (there: of the final map).  Plain tiles are 8 rows x 16 columns.  When the last
// tile column would hold Wr = W mod 16 <= 8 real columns, those columns are instead tiled by a STRIP of transposed tiles, 16 rows x 8 columns: the same
// 10 x 18 halo image and the same MFMA loop with the roles of x and y swapped, half as many tiles for the strip.  Taken only where it lowers the tile count
// (H > 8) and fvit_tune "conv_edge_tiles" (default 1) allows; 56 x 56: 21 + 4 = 25 tiles per image instead of 28.
// Tiles are numbered per image: tiles_x * tiles_y plain tiles (x fastest), then `strips` strip tiles from the top.
struct EdgeTiling { int tiles_x, tiles_y, strips; };
inline EdgeTiling edge_tiling(int H, int W, int edge_tiles) {
    EdgeTiling t{(W + HALO_TW - 1) / HALO_TW, (H + HALO_TH - 1) / HALO_TH, 0};
    const int wr = W % HALO_TW, strips = (H + HALO_TW - 1) / HALO_TW;
    if (edge_tiles && wr >= 1 && wr <= HALO_TH && strips < t.tiles_y) { t.tiles_x = W / HALO_TW; t.strips = strips; }
    return t;
}
// tile -> image, origin of the tile in the map, and its kind (tr: a strip tile: tile pixel (row, s) is map pixel (y0 + s, x0 + row)); wave-uniform
struct TilePos { int b, y0, x0; bool tr; };
__device__ inline TilePos tile_pos(int tile, int tiles_x, int tiles_y, int strips) {
    const int plain = tiles_x * tiles_y, per_img = plain + strips;
    const int b = tile / per_img, t = tile - b * per_img;
    if (t >= plain) return TilePos{b, (t - plain) * HALO_TW, tiles_x * HALO_TW, true};
    const int ty = t / tiles_x;
    return TilePos{b, ty * HALO_TH, (t - ty * tiles_x) * HALO_TW, false};
}

// LN (the conv that ends a level: bias + residual epilogue only): the stored map is LayerNorm2d, over the 64 channels of a pixel, of the map the plain
// instance stores -- statistics in fp32 from the ROUNDED 16-bit values, two passes (mean, then squared deviations), each reduced in-lane (8 channels),
// across the wave's four 16-lane groups (v_permlane swaps) and across the two `ch` waves of a pixel row group through 1 KiB of LDS: pass 1 in a 1-KiB
// area behind the tile buffers, pass 2 in the head of the current tile's halo, which no wave reads once all have passed the barrier of pass 1.  pk[]
// then carries the normalised values through the deferred store.
template <typename T, bool LN = false>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_halo_kernel(HaloParams p) {
    typedef typename Op16<T>::v8 v8;
    // dynamic LDS: [64 floats bias | LN: 64 weight | 64 bias | pad to 1 KiB][2 x (halo + residual tile)][LN: 1 KiB]; without a residual the second
    // part of each buffer is neither allocated nor touched (buffer stride p.buf_bytes)
    extern __shared__ __attribute__((aligned(1024))) char smem_dyn[];
    float* sbias = (float*)smem_dyn;
    char* smem = smem_dyn + 1024;
    if constexpr (LN) {
        if (threadIdx.x >= 64 && threadIdx.x < 128) sbias[threadIdx.x] = p.ln_w[threadIdx.x - 64];
        if (threadIdx.x >= 128 && threadIdx.x < 192) sbias[threadIdx.x] = p.ln_b[threadIdx.x - 128];
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, ph = wave >> 1;
    if (tid < 64) sbias[tid] = p.bias ? p.bias[tid] : 0.f;   // visible after the first barrier of the tile loop
    const int g = lane >> 4, s = lane & 15;

    // XCD-aware persistent schedule: XCD x owns a contiguous range of tiles (neighbouring tiles share halo pixels in
    // that XCD's L2); its workgroups stride through the range together.
    const int nblk = gridDim.x;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int per_xcd = (nblk + 7 - xcd) >> 3;                  // workgroups that landed on this XCD
    const int tq = p.tiles >> 3, tr = p.tiles & 7;
    const int t_begin = xcd * tq + min(xcd, tr);
    const int t_end = t_begin + tq + (xcd < tr ? 1 : 0);

    const T* __restrict__ In = (const T*)p.in;
    const T* __restrict__ W = (const T*)p.w;
    const T* __restrict__ Z = (const T*)p.zeros;
    T* O = (T*)p.out;
    const T* R = (const T*)p.res;   // may alias O (in place): a tile's residual is staged before its output is written

    // ---- stationary weights: wf[tap][kk][ni], A-row slot s of fragment ni -> channel 32ch + (s>>2)*8 + ni*4 + (s&3) ----
    v8 wf[9][2][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
                wf[tap][kk][ni] = *(const v8*)(W + (size_t)(ch * 32 + (s >> 2) * 8 + ni * 4 + (s & 3)) * 576 + tap * 64 + kk * 32 + g * 8);

    const int nb = ch * 32 + g * 8;   // lane's 8 consecutive output channels

    // B-fragment read offsets inside a halo row, per horizontal tap
    int xoff[3];   // K half 1 is the same address with bit 6 flipped (chunk position c ^ 4)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) xoff[kx] = (s + kx) * 128 + ((g ^ ((s + kx) & 6)) << 4);
    // residual read offset: pixel (row, s) of the tile at (row*16 + s)*128, chunk c at position c ^ ((s >> 1) & 7)
    const int roff = HALO_BYTES + (ph * 4 * HALO_TW + s) * 128 + (((ch * 4 + g) ^ ((s >> 1) & 7)) << 4);

    // a strip tile (tr) holds the transposed halo: LDS pixel (hy, hx) is map pixel (y0 + hx, x0 + hy), and likewise its residual pixels
    auto stage = [&](int tile, char* buf) {
        const TilePos tp = tile_pos(tile, p.tiles_x, p.tiles_y, p.strips);
        const bool tr = tp.tr;
        const int y0 = tp.y0 - 1, x0 = tp.x0 - 1;
        const size_t ib = (size_t)tp.b * p.H * p.W * 64;
        // the halo coordinates are tile independent, but keeping 6 x (hy, hx, chunk) live across the MFMA loop costs
        // more registers than the weights leave: recompute them per tile (a handful of VALU ops per 1-KiB piece)
        int lane8 = lane >> 3;
        asm volatile("" : "+v"(lane8));
#pragma unroll
        for (int i = 0; i < (HALO_PIECES + 3) / 4; ++i) {
            const int piece = wave + 4 * i;
            if (piece < HALO_PIECES) {
                const int hp = piece * 8 + lane8;
                const int hy = hp / HALO_PW, hx = hp - hy * HALO_PW;
                const int y = y0 + (tr ? hx : hy), x = x0 + (tr ? hy : hx);
                const bool ok = hy < HALO_PH && y >= 0 && y < p.H && x >= 0 && x < p.W;
                const int c = (lane & 7) ^ (hx & 6);
                const T* src = ok ? In + ib + ((size_t)y * p.W + x) * 64 + c * 8 : Z + c * 8;
                glds16(src, buf + piece * 1024);
            }
        }
        if (R) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int piece = wave * 4 + i;            // 8 pixels of tile row piece >> 1
                const int col = (piece & 1) * 8 + lane8;
                const int y = y0 + 1 + (tr ? col : piece >> 1), x = x0 + 1 + (tr ? piece >> 1 : col);
                const bool ok = y < p.H && x < p.W;
                const int c = (lane & 7) ^ ((col >> 1) & 7);
                const T* src = ok ? R + ib + ((size_t)y * p.W + x) * 64 + c * 8 : Z + c * 8;
                glds16(src, buf + HALO_BYTES + piece * 1024);
            }
        }
    };

    // Outputs are written one tile late: the 16-bit results of tile i wait in 16 VGPRs while tile i+1 is staged, and are
    // stored just before tile i+1's MFMA loop -- so the s_waitcnt vmcnt(0) that guards the NEXT halo finds those stores
    // (and the halo DMA issued with them) long complete instead of exposing the HBM write latency once per tile.
    v8 pk[4];
    int ptile = -1;
    auto flush = [&](int tile) {
        // tile pixel (4ph + mi, s): one address per lane and a wave-uniform step per mi -- a map row, or in a strip tile one pixel
        const TilePos tp = tile_pos(tile, p.tiles_x, p.tiles_y, p.strips);
        const int y = tp.y0 + (tp.tr ? s : ph * 4), x = tp.x0 + (tp.tr ? ph * 4 : s);
        const int dy = tp.tr ? 0 : 1, dx = tp.tr ? 1 : 0;
        T* o = O + (((size_t)tp.b * p.H + y) * p.W + x) * 64 + nb;
        const int step = (tp.tr ? 1 : p.W) * 64;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            if (y + mi * dy < p.H && x + mi * dx < p.W) *(v8*)(o + mi * step) = pk[mi];
    };

    int tile = t_begin + idx;
    if (tile < t_end) stage(tile, smem);
    for (int it = 0; tile < t_end; tile += per_xcd, ++it) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int cur = it & 1;
        if (tile + per_xcd < t_end && !(p.ablate & 2)) stage(tile + per_xcd, smem + (cur ^ 1) * p.buf_bytes);
        if (ptile >= 0 && !(p.ablate & 4)) flush(ptile);
        const char* tb = smem + cur * p.buf_bytes;
        const char* hb = tb + ph * 4 * (HALO_PW * 128);

        f4 acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
        // 18 groups (tap, K half) of 4 B-fragment reads + 8 MFMAs, software pipelined by hand one group ahead; the
        // scheduling barriers keep the compiler from hoisting more reads than that (it otherwise runs out of registers
        // next to the 144 weight VGPRs and spills the read offsets, whose reload would queue behind the LDS-DMA)
        // A strip tile walks the same taps (ky, kx) of the map in the same order with the same weights -- the same sums in the same order -- and reads tap
        // (ky, kx) from its transposed halo at row shift kx, column offset xoff[ky].  Tap (ky, kx) is at hb + ko[0][ky] + ko[1][kx] for both kinds: the kind
        // (wave-uniform) picks the six offsets once per tile, the loop is the same code.  A row shift is a multiple of 256: it leaves bit 6 to the K half.
        static_assert((HALO_PW * 128) % 256 == 0, "a row shift must leave bit 6 of a read offset alone");
        int ko[2][3];
        {
            const bool tr = tile_pos(tile, p.tiles_x, p.tiles_y, p.strips).tr;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                ko[0][k] = tr ? xoff[k] : k * (HALO_PW * 128);
                ko[1][k] = tr ? k * (HALO_PW * 128) : xoff[k];
            }
        }
        v8 xf[2][4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) xf[0][mi] = *(const v8*)(hb + mi * (HALO_PW * 128) + xoff[0]);
        __builtin_amdgcn_sched_barrier(0);
        if (!(p.ablate & 1))
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            const int tap = q >> 1, kk = q & 1;
            if (q + 1 < 18) {
                const int tap1 = (q + 1) >> 1, kk1 = (q + 1) & 1, ky1 = tap1 / 3, kx1 = tap1 - ky1 * 3;
                const int o = (ko[0][ky1] + ko[1][kx1]) ^ (kk1 << 6);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) xf[(q + 1) & 1][mi] = *(const v8*)(hb + mi * (HALO_PW * 128) + o);
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = Op16<T>::mfma(wf[tap][kk][ni], xf[q & 1][mi], acc[ni][mi]);
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- epilogue math: lane holds channels nb .. nb+7 of tile pixels (row 4ph + mi, s): out[b][y0 + row][x0 + s], strip tile out[b][y0 + s][x0 + row] ----
        float bias[8];
        {
            const f4 t0 = *(const f4*)(sbias + nb), t1 = *(const f4*)(sbias + nb + 4);
            bias[0] = t0[0]; bias[1] = t0[1]; bias[2] = t0[2]; bias[3] = t0[3];
            bias[4] = t1[0]; bias[5] = t1[1]; bias[6] = t1[2]; bias[7] = t1[3];
        }
        if constexpr (LN) {
            float stat[4];   // pass 1: the wave's channel sum of pixel (4 ph + mi, s); pass 2: its sum of squared deviations
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const v8 rv = *(const v8*)(tb + roff + mi * (HALO_TW * 128));
                v8 ov;
                float sum = 0.f;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const f4 a = acc[ni][mi];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const T o = (T)(a[r] + bias[ni * 4 + r] + (float)rv[ni * 4 + r]);   // the value the plain instance stores
                        ov[ni * 4 + r] = o;
                        sum += (float)o;
                    }
                }
                pk[mi] = ov;
                stat[mi] = sum_xor32(sum_xor16(sum));
            }
            float mean[4];
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                // [ch][pixel 16 (4 ph + mi) + s]; pass 2 reuses the head of this tile's halo: every wave is past its MFMA loop after the barrier of pass 1
                float* red = (float*)(pass == 0 ? smem + 2 * HALO_BUF : smem + cur * HALO_BUF);
                if (g == 0) {
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) red[ch * 128 + (ph * 4 + mi) * 16 + s] = stat[mi];
                }
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const float* q = red + (ph * 4 + mi) * 16 + s;
                    const float tot = q[0] + q[128];   // the same order in both waves
                    if (pass == 0) {
                        mean[mi] = tot * (1.f / 64.f);
                        float sq = 0.f;
#pragma unroll
                        for (int j = 0; j < 8; ++j) { const float d = (float)pk[mi][j] - mean[mi]; sq += d * d; }
                        stat[mi] = sum_xor32(sum_xor16(sq));
                    } else {
                        stat[mi] = rsqrtf(tot * (1.f / 64.f) + p.ln_eps);
                    }
                }
            }
            float lw[8], lb[8];
            {
                const f4 w0 = *(const f4*)(sbias + 64 + nb), w1 = *(const f4*)(sbias + 64 + nb + 4);
                const f4 b0 = *(const f4*)(sbias + 128 + nb), b1 = *(const f4*)(sbias + 128 + nb + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { lw[j] = w0[j]; lw[4 + j] = w1[j]; lb[j] = b0[j]; lb[4 + j] = b1[j]; }
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                v8 nv;
#pragma unroll
                for (int j = 0; j < 8; ++j) nv[j] = (T)(((float)pk[mi][j] - mean[mi]) * stat[mi] * lw[j] + lb[j]);
                pk[mi] = nv;
            }
        } else
        if (!(p.ablate & 8))
            dispatch_epilogue(p.act, R != nullptr, [&](auto act_tag, auto res_tag) {
                constexpr int ACT = decltype(act_tag)::value;
                constexpr bool RES = decltype(res_tag)::value != 0;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    v8 rv;
                    if (RES) rv = *(const v8*)(tb + roff + mi * (HALO_TW * 128));
                    v8 ov;
                    float yv[8];
#pragma unroll
                    for (int ni = 0; ni < 2; ++ni) {
                        const f4 a = acc[ni][mi];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float y = a[r] + bias[ni * 4 + r];
                            if (ACT == 1) y = fmaxf(y, 0.f);
                            yv[ni * 4 + r] = y;
                        }
                    }
                    if constexpr (ACT == 2) {   // interleaved Horner chains, bitwise gelu_fast; groups of 4: eight chains at once spill here (249 registers)
                        float y0[4] = {yv[0], yv[1], yv[2], yv[3]}, y1[4] = {yv[4], yv[5], yv[6], yv[7]};
                        gelu_fast_n<4>(y0);
                        gelu_fast_n<4>(y1);
#pragma unroll
                        for (int j = 0; j < 4; ++j) { yv[j] = y0[j]; yv[4 + j] = y1[j]; }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) ov[j] = (T)(RES ? yv[j] + (float)rv[j] : yv[j]);
                    pk[mi] = ov;
                }
            });
        ptile = tile;
    }
    if (ptile >= 0) flush(ptile);
}


// ------------------------------------------------------------------------------------------------------------
// Row-band 3x3 convolution for Cin = Cout = 128, stride 1, maps up to 30 pixels wide (ConvBlock convs of level 1 of FasterViT-0:
// 28 x 28 x 128, FV:502-512), r03.
//
// The implicit GEMM above moves ~300 MB from L2 into LDS per launch at 86 images (every input pixel once per tap, the 288-KiB weight
// matrix once per 128-pixel tile): 6.9 TB/s of L2 -> LDS traffic at 44 us per launch -- it is bound by that traffic, not by its MFMAs (0.18).
// Here a workgroup owns a BAND of R full-width output rows of one image (R = 7 at 28 x 28: four bands per image):
//   * the band's input rows plus one halo row above / below and one zero column left / right -- (R + 2) x (W + 2) pixels of 256 B, 68 KiB --
//     are brought into LDS ONCE by LDS-DMA (16-byte chunks, chunk position c ^ (pixel & 15): the 16 lanes of a ds_read_b128 service
//     group read 16 consecutive pixels and hit 16 different chunk positions for any tap shift);
//   * output positions are numbered linearly over the PADDED row pitch, q = r * (W + 2) + x, so the input pixel of tap (ky, kx) is LDS
//     pixel q + ky * (W + 2) + kx for every q: a 16-position MFMA column group is the same LDS image read at a shifted address, and groups
//     run across row ends (the two pad positions per row are computed and dropped: 196 of 224 positions are real at 28 x 28);
//   * the 4 waves split the output channels (32 each) and every wave streams ITS quarter of the weights (72 KiB, pre-packed in MFMA fragment
//     order, one 1-KiB fragment per global_load_dwordx4 per lane) from L2 straight into a register ring -- no weight staging in LDS, so the
//     workgroup's LDS is the band alone and two workgroups share a CU.
// L2 -> CU traffic per launch: 344 x (68 KiB band + 288 KiB weights) = 122 MB instead of 303 MB; per K step a wave issues 14 ds_read_b128 and
// 2 global loads for 28 MFMAs.
// ------------------------------------------------------------------------------------------------------------
struct BandParams {
    const void* in;      // [B][H][W][128]
    const void* wf;      // op16 [4 waves][36 steps][2][64 lanes][8]  (fvit_conv3x3_c128_band's w_frag)
    const float* bias;   // [128] or null
    const void* res;     // [B][H][W][128] or null (may alias out)
    void* out;           // [B][H][W][128]
    const void* zeros;   // >= 256 bytes of zeros
    int B, H, W, act;
    int PW, R, bands;    // padded row pitch W + 2, output rows per band, bands per image
    int npieces;         // 1-KiB pieces (4 pixels) of the band's (R + 2) x PW halo image
    int magic;           // ceil(65536 / PW): n / PW == (n * magic) >> 16 for n < 2048
    const float* ln_w;   // LN instance only (fvit_conv3x3_c128_band_ln2d): LayerNorm2d weight / bias [128] applied to the stored map
    const float* ln_b;
    float ln_eps;
    unsigned long long* ts;   // TS instance only (fvit_debug_conv_band_timeline): s_memtime stamps [workgroup][wave][8]: 0 start, 1 band DMA and
                              // first weight steps requested, 2 band landed (barrier passed), 3 K loop done, 4 residual rows landed, 5 end
};

#ifndef FVIT_BD_DEPTH
#define FVIT_BD_DEPTH 6   // weight steps (2 fragments each) in flight per wave (4 .. 8 and PD 2 .. 5 time the same: profiles/r03_conv_band_*.log)
#endif
#ifndef FVIT_BD_PD
#define FVIT_BD_PD 3      // B-fragment batches requested ahead of the MFMAs
#endif
constexpr int BD_NG = 14;                                   // 16-position column groups per band (R * PW <= 224)
constexpr int BD_MAXPW = 32;
constexpr int BD_PIX = (BD_NG * 16 + 2 * BD_MAXPW + 2 + 3) / 4 * 4;   // LDS pixels a read can touch: 292
constexpr int BD_LDS = BD_PIX * 256;                        // 74 752 B

// LN (the conv that ends a level: bias + residual epilogue only): the stored map is LayerNorm2d, over the 128 channels of a pixel, of the map the plain
// instance stores -- statistics in fp32 from the ROUNDED 16-bit values, two passes (mean, then squared deviations), each reduced in-lane (8 channels),
// across the wave's four 16-lane groups (v_permlane swaps) and across the four waves through the band's LDS, which is dead after the K loop.
template <typename T, bool TS = false, bool LN = false>
__global__ __launch_bounds__(256, 2) void conv3x3_c128_band_kernel(BandParams p) {
    typedef typename Op16<T>::v8 v8;
#define FVIT_BD_STAMP(k) if constexpr (TS) { if ((threadIdx.x & 63) == 0) p.ts[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + (k)] = __builtin_amdgcn_s_memtime(); }
    FVIT_BD_STAMP(0)
    constexpr int NG = BD_NG, HB = NG / 2, DEPTH = FVIT_BD_DEPTH, NSTEP = 36;
    constexpr int BG = 2, NBATCH = NG / BG, PD = FVIT_BD_PD, XR = PD + 1;   // B fragments: batches of BG groups, requested PD batches ahead
    __shared__ __attribute__((aligned(1024))) char smem[BD_LDS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, s = lane & 15;

    // XCD x owns a contiguous range of (image, band) units: the bands of an image share halo rows in that XCD's L2
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7, idx = bid >> 3;
    const int unit = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int img = unit / p.bands, band = unit - img * p.bands;
    const int y0 = band * p.R, PW = p.PW;

    const T* __restrict__ In = (const T*)p.in + (size_t)img * p.H * p.W * 128;
    const T* __restrict__ Z = (const T*)p.zeros;

    // ---- the band's halo image -> LDS (oldest in the vmcnt queue), then the first DEPTH steps of the wave's weight stream ----
    {
        const int lane4 = lane >> 4, j = lane & 15;
#pragma unroll 1
        for (int piece = wave; piece < p.npieces; piece += 4) {
            const int hp = piece * 4 + lane4;
            const int hy = (hp * p.magic) >> 16, hx = hp - hy * PW;
            const int y = y0 - 1 + hy, x = hx - 1;
            const bool ok = hy < p.R + 2 && y >= 0 && y < p.H && x >= 0 && x < p.W;
            const int c = j ^ (hp & 15);
            const T* src = ok ? In + ((size_t)y * p.W + x) * 128 + c * 8 : Z + c * 8;
            glds16(src, smem + piece * 1024);
        }
    }
    const char* Wf = (const char*)p.wf + (size_t)wave * (NSTEP * 2 * 1024) + lane * 16;
    v8 ring[DEPTH][2];
    auto issue = [&](int t) {
        if (t < NSTEP) {
            ring[t % DEPTH][0] = *(const v8*)(Wf + (t * 2 + 0) * 1024);
            ring[t % DEPTH][1] = *(const v8*)(Wf + (t * 2 + 1) * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < DEPTH; ++t) issue(t);
    FVIT_BD_STAMP(1)

    f4 acc[2][NG];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int i = 0; i < NG; ++i) acc[ni][i] = (f4){0.f, 0.f, 0.f, 0.f};

    // the band has landed when only the 2 * DEPTH weight fragments requested after it are still in flight
    // (raw barrier: __syncthreads() would drain the weight ring as well)
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(2 * DEPTH) : "memory");
    FVIT_BD_STAMP(2)

    // B fragment of group i at step (tap, kk): pixel 16 i + s + shift(tap), k slots 8 g .. 8 g + 7 of K quarter kk -> chunk kk * 4 + g.
    // 16 i leaves pixel & 15 alone: one base address per step, the groups at immediate offsets i * 4096.
    auto xbase = [&](int t) {
        const int tap = t >> 2, kk = t & 3, ky = tap / 3, kx = tap - ky * 3;
        const int pix = s + ky * PW + kx;
        return pix * 256 + (((kk * 4 + g) ^ (pix & 15)) << 4);
    };
    // The four waves read the same B fragments: a K step costs the workgroup 56 KiB of LDS reads (~300 cycles at 256 B / cycle incl. the
    // 2-way conflict of the odd tap shifts, SQ_LDS_BANK_CONFLICT = 25 % of SQ_LDS_IDX_ACTIVE) against 448 MFMA cycles per wave.  Batches of
    // BG = 2 groups (4 MFMAs) are requested PD batches ahead.  Measured: the K loop runs at ~0.65 of the MFMA rate whatever the batching
    // (two batches of 7 one ahead, or 2 / 3 / 5 batches of 2 ahead) and whatever the weight ring depth (6 / 8).
    v8 xf[XR][BG];
    auto load_batch = [&](int b) {
        if (b < NSTEP * NBATCH) {
            const char* xb = smem + xbase(b / NBATCH) + (b % NBATCH) * BG * 4096;
#pragma unroll
            for (int i = 0; i < BG; ++i) xf[b % XR][i] = *(const v8*)(xb + i * 4096);
        }
    };
#pragma unroll
    for (int b = 0; b < PD; ++b) load_batch(b);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NSTEP; ++t) {
#pragma unroll
        for (int j = 0; j < NBATCH; ++j) {
            const int b = t * NBATCH + j;
            load_batch(b + PD);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int i = 0; i < BG; ++i)
                    acc[ni][j * BG + i] = Op16<T>::mfma(ring[t % DEPTH][ni], xf[b % XR][i], acc[ni][j * BG + i]);
            __builtin_amdgcn_sched_barrier(0);
        }
        issue(t + DEPTH);
    }
    if constexpr (TS) {   // the stamp must not pass the last MFMAs: make it depend on an accumulator
        asm volatile("s_nop 0" ::"v"(acc[1][NG - 1]) : "memory");
    }
    FVIT_BD_STAMP(3)

    // ---- epilogue: lane holds out[position 16 i + s][32 wave + 8 g .. + 7]; A-row slot 4 g + r of fragment ni is channel 32 wave + 8 g + 4 ni + r ----
    const int nb = wave * 32 + g * 8;
    float bias[8];
    {
        const f4 t0 = p.bias ? *(const f4*)(p.bias + nb) : (f4){0.f, 0.f, 0.f, 0.f};
        const f4 t1 = p.bias ? *(const f4*)(p.bias + nb + 4) : (f4){0.f, 0.f, 0.f, 0.f};
        bias[0] = t0[0]; bias[1] = t0[1]; bias[2] = t0[2]; bias[3] = t0[3];
        bias[4] = t1[0]; bias[5] = t1[1]; bias[6] = t1[2]; bias[7] = t1[3];
    }
    T* O = (T*)p.out + (size_t)img * p.H * p.W * 128 + nb;
    const T* Rs = p.res ? (const T*)p.res + (size_t)img * p.H * p.W * 128 + nb : nullptr;
    if constexpr (LN) {
        // position q = 16 i + s of the band: its pixel's element offset, or -1 for a pad position / a row below the map
        auto pix_off = [&](int i) {
            const int q = i * 16 + s;
            const int r = (q * p.magic) >> 16, x = q - r * PW, y = y0 + r;
            return (r < p.R && y < p.H && x < p.W) ? (y * p.W + x) * 128 : -1;
        };
        v8 ov[NG];        // the map the plain instance stores
        float stat[NG];   // pass 1: the wave's channel sum of the pixel; pass 2: its sum of squared deviations
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v8 rv[HB];
#pragma unroll
            for (int i = 0; i < HB; ++i) rv[i] = *(const v8*)(Rs + max(pix_off(h * HB + i), 0));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < HB; ++i) {
                float sum = 0.f;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const f4 a = acc[ni][h * HB + i];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const T o = (T)(a[r] + bias[ni * 4 + r] + (float)rv[i][ni * 4 + r]);
                        ov[h * HB + i][ni * 4 + r] = o;
                        sum += (float)o;
                    }
                }
                stat[h * HB + i] = sum_xor32(sum_xor16(sum));
            }
        }
        float* red = (float*)smem;   // [2 passes][4 waves][NG * 16 positions]
        float mean[NG];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            float* rp = red + pass * (4 * NG * 16);
            if (pass == 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // every wave has left the K loop: the band image is dead
            if (g == 0) {
#pragma unroll
                for (int i = 0; i < NG; ++i) rp[wave * (NG * 16) + i * 16 + s] = stat[i];
            }
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const float* q = rp + i * 16 + s;
                const float tot = (q[0] + q[NG * 16]) + (q[2 * NG * 16] + q[3 * NG * 16]);   // the same order in every wave
                if (pass == 0) {
                    mean[i] = tot * (1.f / 128.f);
                    float sq = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { const float d = (float)ov[i][j] - mean[i]; sq += d * d; }
                    stat[i] = sum_xor32(sum_xor16(sq));
                } else {
                    stat[i] = rsqrtf(tot * (1.f / 128.f) + p.ln_eps);
                }
            }
        }
        float lw[8], lb[8];
        {
            const f4 w0 = *(const f4*)(p.ln_w + nb), w1 = *(const f4*)(p.ln_w + nb + 4), b0 = *(const f4*)(p.ln_b + nb), b1 = *(const f4*)(p.ln_b + nb + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { lw[j] = w0[j]; lw[4 + j] = w1[j]; lb[j] = b0[j]; lb[4 + j] = b1[j]; }
        }
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            v8 nv;
#pragma unroll
            for (int j = 0; j < 8; ++j) nv[j] = (T)(((float)ov[i][j] - mean[i]) * stat[i] * lw[j] + lb[j]);
            const int off = pix_off(i);
            if (off >= 0) *(v8*)(O + off) = nv;
        }
    } else
    dispatch_epilogue(p.act, Rs != nullptr, [&](auto act_tag, auto res_tag) {
        constexpr int ACT = decltype(act_tag)::value;
        constexpr bool RES = decltype(res_tag)::value != 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int off[HB];      // element offset of the position's pixel, or -1
            v8 rv[HB];
#pragma unroll
            for (int i = 0; i < HB; ++i) {
                const int q = (h * HB + i) * 16 + s;
                const int r = (q * p.magic) >> 16, x = q - r * PW, y = y0 + r;
                const bool ok = r < p.R && y < p.H && x < p.W;
                off[i] = ok ? (y * p.W + x) * 128 : -1;
                if (RES) rv[i] = *(const v8*)(Rs + (ok ? off[i] : 0));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < HB; ++i) {
                v8 ov;
                float yv[8];
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    const f4 a = acc[ni][h * HB + i];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float y = a[r] + bias[ni * 4 + r];
                        if (ACT == 1) y = fmaxf(y, 0.f);
                        yv[ni * 4 + r] = y;
                    }
                }
                if constexpr (ACT == 2) gelu_fast_n<8>(yv);   // interleaved Horner chains, bitwise gelu_fast
#pragma unroll
                for (int j = 0; j < 8; ++j) ov[j] = (T)(RES ? yv[j] + (float)rv[i][j] : yv[j]);
                if (off[i] >= 0) *(v8*)(O + off[i]) = ov;
            }
            if (h == 0) { FVIT_BD_STAMP(4) }
        }
    });
    if constexpr (TS) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    FVIT_BD_STAMP(5)
#undef FVIT_BD_STAMP
}

bool band_supported(int H, int W) { return H >= 1 && W >= 1 && W + 2 <= BD_MAXPW; }


// ------------------------------------------------------------------------------------------------------------
// Fused two-conv stem of PatchEmbed (FV:458-464) for in_dim = dim = 64 (FasterViT-0):
//     out = ReLU(conv2_s2(ReLU(conv1_s2(image) + b1)) + b2),  conv1: 3 -> 64, conv2: 64 -> 64, both 3x3 / stride 2 / pad 1.
// The 112x112x64 map between the two convs is the largest tensor of the network (1.6 MB per image in fp16): written and read
// back it is 3.2 MB of the ~47 MB per image this pipeline moves through HBM.  Here a workgroup owns an 8x16 tile of the FINAL
// 56x56 map: phase A computes the 17x33 conv1 pixels that tile needs (stem_conv_kernel's gather + one 32-deep MFMA step per 16
// pixels, 10 % halo recompute) straight into LDS; phase B is the halo kernel's register-stationary conv over that LDS image.
// Stride 2 would make a 16-pixel MFMA column group read every other LDS pixel, so phase A stores even and odd conv1 columns
// in two planes: tap kx = 0 / 1 / 2 of output column j is plane E pixel j / plane O pixel j / plane E pixel j + 1 -- 16 consecutive
// pixels again, conflict-free with the chunk position c ^ (px & 6) as in conv3x3_c64_halo_kernel.
// ------------------------------------------------------------------------------------------------------------
struct StemFusedParams {
    FvitMapView in;      // (B, 3, Hi, Wi)
    const void* w1;      // op16 [64][32]: k = ky*9 + kx*3 + c, zero for k >= 27
    const float* b1;     // [64]
    const void* w2;      // op16 [64][9*64]
    const float* b2;     // [64]
    void* out;           // [B][H2][W2][64]
    int B, Hi, Wi, H1, W1, H2, W2;
    int tiles_x, tiles_y, strips, tiles;   // edge_tiling(H2, W2)
    unsigned long long* ts;   // TS instance only (fvit_debug_stem_timeline): per wave [workgroup][wave][8] accumulated s_memtime ticks:
                              // 0 phase A (gathers + conv1 + LDS writes), 1 barrier after A, 2 phase B, 3 epilogue, 4 barrier before A, 5 tiles, 6 total
    float nscale[3], nshift[3];   // IN = uint8_t: every gathered byte u of channel c becomes fmaf(u, nscale[c], nshift[c]) (fvit_stem_fused_u8)
};

constexpr int SF_ROWS = 2 * HALO_TH + 1, SF_COLS = 2 * HALO_TW + 1;         // 17 x 33 conv1 pixels per tile
constexpr int SF_PLANE = (HALO_TW + 1) * 128;                                // 17 pixels of 128 B
constexpr int SF_ROWPITCH = 2 * SF_PLANE;                                    // plane E (17 px) then plane O (16 px + 1 unused)
constexpr int SF_LDS = SF_ROWS * SF_ROWPITCH;                                // 73 984 B
constexpr int SF_GROUPS = (SF_ROWS * SF_COLS + 15) / 16;                     // 36 groups of 16 conv1 pixels
constexpr int SF_BATCH = 3;                                                  // groups whose gathers are in flight together (r03: 3 fit since the per-lane gather constants; r01 / r02: 2)

// IN: element type of the caller's image (float / _Float16 / __bf16) -- a compile-time parameter since r03: as a runtime switch it put two
// scalar branches around every gathered element (~40 instructions per element, the whole of phase A: 12 of the 16.6 us a tile took)
// NHWC3 (r06): the caller's image is fp32 channels-last (stride_c = 1, stride_w = 3: validate.py's --channels-last, bench.py).  The nine (kx, c) values of one
// kernel row are then 36 contiguous bytes, and the gather of a conv1 pixel is THREE bounds-checked buffer loads per lane (dwordx4, dwordx4, dword: row
// ky = g of the 3 x 3 patch) instead of eight scalar loads with their index arithmetic -- phase A was 78 % of a tile (profiles/r03_stem_phase_accounting.log).
// The contraction order changes with it: k slot 8g + e = (ky = g, r9 = e) for g < 3, and the ninth value of each row goes to lane group 3 (k slots 24 + ky,
// three VALU lane swaps); the first-conv weights are re-ordered to match, once per workgroup, into LDS.  Rows above / below the image are out of the
// buffer's range and read as zero; the left / right border columns are masked (the run then covers the neighbouring row's pixel).
// IN = uint8_t (fvit_stem_fused_u8): the image is uint8 and is normalised at the load, value = inside ? fmaf(u, nscale[c], nshift[c]) : 0 -- the zero padding
// is applied AFTER the normalisation, as the reference does, so a tap outside the image is masked explicitly (an out-of-range load's 0 would normalise
// to nshift[c]).  Both gathers keep the k slots of their float instance: the MFMA operands, and so the result bits, are those of the float kernel on the
// normalised fp32 image in the same layout.  The general gather is one byte load per element.  NHWC3 (the decoder's HWC: stride_c 1, stride_w 3): the
// nine (kx, c) values of a kernel row are nine contiguous BYTES at any alignment (pixel and W * 3 mod 4 decide it): three aligned dword loads from a
// buffer whose base is the image base rounded down to a dword and whose size is rounded up to one (a dword with a byte of the image in it lies in that
// byte's page), v_alignbyte_b32 by the offset's low two bits, then v_cvt_f32_ubyte0..3 + v_fma per value.
template <typename T, typename IN = float, bool TS = false, bool NHWC3 = false>
__global__ __launch_bounds__(256, 2) void stem_fused_kernel(StemFusedParams p) {
    constexpr bool U8IN = sizeof(IN) == 1;
    static_assert(!NHWC3 || sizeof(IN) == 4 || U8IN, "the contiguous-run gather reads dword-aligned runs (fp32) or aligns byte runs itself (uint8)");
    unsigned long long tsA = 0, tsBar = 0, tsB = 0, tsE = 0, tsBar0 = 0, tsN = 0, tsT0 = 0, tsMark = 0;
    unsigned pf_sink = 0;   // keeps the next-tile touch loads alive
    if constexpr (TS) { tsT0 = __builtin_amdgcn_s_memtime(); }
#define FVIT_SF_MARK(acc) if constexpr (TS) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - tsMark; tsMark = now_; }
    typedef typename Op16<T>::v8 v8;
    extern __shared__ __attribute__((aligned(1024))) char smem_dyn[];
    float* sb1 = (float*)smem_dyn;             // [64]
    float* sb2 = sb1 + 64;                     // [64]
    char* img = smem_dyn + 1024;               // conv1 tile
    T* w1s = (T*)(smem_dyn + 1024 + SF_LDS);   // NHWC3: the first-conv weights [64][32] in the run order of the gather (4 KiB)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = wave & 1, ph = wave >> 1;
    const int g = lane >> 4, s = lane & 15;
    if (tid < 64) { sb1[tid] = p.b1[tid]; sb2[tid] = p.b2[tid]; }
    if constexpr (NHWC3) {
        // w1s[ch][8 gg + e] = w1[ch][k]: gg < 3: k = 9 gg + e (row ky = gg, values r9 = 0 .. 7); gg = 3: k = 9 e + 8 for e < 3 (the ninth value of row e), else 0
        const T* W1g = (const T*)p.w1;
        for (int i = tid; i < 64 * 32; i += 256) {
            const int chn = i >> 5, kk = i & 31, gg = kk >> 3, e = kk & 7;
            const int k = gg < 3 ? 9 * gg + e : (e < 3 ? 9 * e + 8 : 31);   // k = 31 is a zero column of w1
            w1s[i] = W1g[chn * 32 + k];
        }
    }

    const int nblk = gridDim.x;
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int per_xcd = (nblk + 7 - xcd) >> 3;
    const int tq = p.tiles >> 3, tr = p.tiles & 7;
    const int t_begin = xcd * tq + min(xcd, tr);
    const int t_end = t_begin + tq + (xcd < tr ? 1 : 0);

    const T* __restrict__ W1 = (const T*)p.w1;
    const T* __restrict__ W2 = (const T*)p.w2;
    T* __restrict__ O = (T*)p.out;

    // ---- conv2 weights, stationary in registers: wf[tap][kk][ni], slot s of fragment ni -> channel 32ch + (s>>2)*8 + ni*4 + (s&3) ----
    v8 wf[9][2][2];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
                wf[tap][kk][ni] = *(const v8*)(W2 + (size_t)(ch * 32 + (s >> 2) * 8 + ni * 4 + (s & 3)) * 576 + tap * 64 + kk * 32 + g * 8);
    const int nb = ch * 32 + g * 8;

    // phase-B read offsets inside a conv1 row, per horizontal tap: (plane, pixel shift) = (E, 0), (O, 0), (E, 1)
    int xoff[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int px = s + (kx == 2 ? 1 : 0);
        xoff[kx] = (kx == 1 ? SF_PLANE : 0) + px * 128 + ((g ^ (px & 6)) << 4);
    }

    for (int tile = t_begin + idx; tile < t_end; tile += per_xcd) {
        // a strip tile (tr, edge_tiling) holds the transposed conv1 image: the 33 LDS columns with their even / odd planes run along conv1 y, the 17 LDS
        // rows along conv1 x -- LDS pixel (lr, lc) is conv1 pixel (r0 + lc, c0 + lr); its gather and k slots are those of any conv1 pixel
        const TilePos tp = tile_pos(tile, p.tiles_x, p.tiles_y, p.strips);
        const bool tr = tp.tr;
        const int b = tp.b;
        const int r0 = 2 * tp.y0 - 1, c0 = 2 * tp.x0 - 1;      // conv1 coordinates of local (0, 0)
        if constexpr (TS) { tsMark = __builtin_amdgcn_s_memtime(); tsN += 1; }
        __syncthreads();   // every wave is done reading the previous tile's conv1 image (and sb1 / sb2 are visible)
        FVIT_SF_MARK(tsBar0)

        // ================= phase A: conv1 + bias + ReLU of the tile's 17 x 33 conv1 pixels -> LDS =================
        if constexpr (NHWC3) {
            int lane_s = s, lane_g = g;
            asm volatile("" : "+v"(lane_s), "+v"(lane_g));   // keep the per-group index math inside the loop (registers!)
            v8 w1f[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) w1f[ni] = *(const v8*)(w1s + ((lane_s >> 2) * 16 + ni * 4 + (lane_s & 3)) * 32 + lane_g * 8);
            // one buffer per image: every offset outside [0, Hi Wi 12) -- the rows above and below the image, negative offsets included -- reads as zero
            // uint8: base rounded down to a dword (al = the bytes in front of the image), size rounded up to one; every row is masked explicitly below
            const uintptr_t ibase = (uintptr_t)p.in.data + (int64_t)b * p.in.stride_b * (int64_t)sizeof(IN);
            const int al = U8IN ? (int)(ibase & 3) : 0;
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(ibase - al), 0,
                                                                                   U8IN ? ((al + p.Hi * p.Wi * 3 + 3) & ~3) : p.Hi * p.Wi * 12, 0x00020000);
            const int gy = lane_g < 3 ? lane_g : 2;          // lane group 3 repeats group 2's loads; its own values arrive by lane swaps
            for (int g3 = wave; g3 < SF_GROUPS; g3 += 4 * SF_BATCH) {
                f4 la[SF_BATCH], lb[SF_BATCH];
                float lc8[SF_BATCH];
                unsigned d0[SF_BATCH], d1[SF_BATCH], d2[SF_BATCH], bsh[SF_BATCH];   // uint8: the three dwords around the run and its byte shift
                bool rowin[SF_BATCH];                                               // uint8: the run's row is inside the image
                int qv[SF_BATCH], lrv[SF_BATCH], lcv[SF_BATCH];
                bool v1v[SF_BATCH], lft[SF_BATCH], rgt[SF_BATCH];
#pragma unroll
                for (int u = 0; u < SF_BATCH; ++u) {
                    const int q = (g3 + 4 * u) * 16 + lane_s;
                    const int lr = q / SF_COLS, lc = q - lr * SF_COLS;
                    const int R = r0 + (tr ? lc : lr), Cc = c0 + (tr ? lr : lc);
                    const bool v1 = q < SF_ROWS * SF_COLS && R >= 0 && R < p.H1 && Cc >= 0 && Cc < p.W1;
                    const int yi = 2 * R - 1, xi = 2 * Cc - 1;
                    qv[u] = q; lrv[u] = lr; lcv[u] = lc; v1v[u] = v1;
                    lft[u] = xi < 0;                // tap column kx = 0 is left of the image: values 0 .. 2 of the run belong to the previous row
                    rgt[u] = xi + 2 >= p.Wi;        // tap column kx = 2 is right of it: values 6 .. 8 belong to the next row
                    // a pixel outside the conv1 map (v1 false) is stored as zero below whatever it read: point it at the image's first run.  At the left / right
                    // border the run starts one pixel later / earlier (and is shifted back in registers below): no access then straddles the start or the end of
                    // the buffer -- a dwordx4 that is PARTLY out of range comes back as zeros altogether (r06: the image's corner pixels were wrong)
                    const int off = v1 ? ((yi + gy) * p.Wi + xi + (xi < 0 ? 1 : 0) - (xi + 2 >= p.Wi ? 1 : 0)) * (U8IN ? 3 : 12) : 0;
                    if constexpr (U8IN) {
                        const int ob = off + al, a0 = ob & ~3;     // a row above the image: a negative (= huge unsigned) offset, out of range, reads 0
                        rowin[u] = yi + gy >= 0 && yi + gy < p.Hi;
                        bsh[u] = (unsigned)ob & 3u;
                        d0[u] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, a0, 0, 0);
                        d1[u] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, a0 + 4, 0, 0);
                        d2[u] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, a0 + 8, 0, 0);
                    } else {
                        la[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
                        lb[u] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 16, 0, 0));
                        lc8[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + 32, 0, 0));
                    }
                }
#pragma unroll
                for (int u = 0; u < SF_BATCH; ++u) {
                    const int q = qv[u], lr = lrv[u], lc = lcv[u];
                    const bool v1 = v1v[u];
                    float l9[9];
                    if constexpr (U8IN) {
                        const unsigned w3[3] = {__builtin_amdgcn_alignbyte(d1[u], d0[u], bsh[u]), __builtin_amdgcn_alignbyte(d2[u], d1[u], bsh[u]),
                                                __builtin_amdgcn_alignbyte(d2[u], d2[u], bsh[u])};
#pragma unroll
                        for (int e = 0; e < 9; ++e) {
                            const float nv = __builtin_fmaf((float)((w3[e >> 2] >> (8 * (e & 3))) & 0xffu), p.nscale[e % 3], p.nshift[e % 3]);
                            l9[e] = rowin[u] ? nv : 0.f;   // a row above / below the image: the padding's zero, not nshift
                        }
                    } else {
                        l9[0] = la[u][0]; l9[1] = la[u][1]; l9[2] = la[u][2]; l9[3] = la[u][3];
                        l9[4] = lb[u][0]; l9[5] = lb[u][1]; l9[6] = lb[u][2]; l9[7] = lb[u][3]; l9[8] = lc8[u];
                    }
                    float e9[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) {
                        const float sl = e >= 3 ? l9[e - 3] : 0.f;    // left border: the run began at tap column 1
                        const float sr = e < 6 ? l9[e + 3] : 0.f;     // right border: it began one pixel left of tap column 0
                        e9[e] = lft[u] ? sl : (rgt[u] ? sr : l9[e]);
                    }
                    // the ninth value of rows 0 / 1 / 2 (held by lane groups 0 / 1 / 2) -> k slots 24 / 25 / 26 of lane group 3
                    const auto sw16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(e9[8]), __float_as_uint(e9[8]), false, false);   // [0]: odd rows <- the even row below
                    const auto sw32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(e9[8]), __float_as_uint(e9[8]), false, false);   // [0]: lanes 32.. <- lanes 0 .. 31
                    const auto sw3 = __builtin_amdgcn_permlane32_swap(sw16[0], sw16[0], false, false);
                    const float t0 = __uint_as_float(sw3[0]), t1 = __uint_as_float(sw32[0]), t2 = __uint_as_float(sw16[0]);   // in lane group 3: rows 0, 1, 2
                    const bool g3l = lane_g == 3;
                    v8 xf;
                    xf[0] = (T)(g3l ? t0 : e9[0]);
                    xf[1] = (T)(g3l ? t1 : e9[1]);
                    xf[2] = (T)(g3l ? t2 : e9[2]);
#pragma unroll
                    for (int e = 3; e < 8; ++e) xf[e] = (T)(g3l ? 0.f : e9[e]);
                    f4 acc[4];
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[ni] = Op16<T>::mfma(w1f[ni], xf, (f4){0.f, 0.f, 0.f, 0.f});
                    if (q < SF_ROWS * SF_COLS) {
                        v8 o0, o1;
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            const f4 bv = *(const f4*)(sb1 + lane_g * 16 + ni * 4);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float y = v1 ? fmaxf(acc[ni][r] + bv[r], 0.f) : 0.f;   // outside the conv1 map: conv2's zero padding
                                if (ni < 2) o0[ni * 4 + r] = (T)y; else o1[(ni - 2) * 4 + r] = (T)y;
                            }
                        }
                        const int px = lc >> 1;
                        char* dst = img + lr * SF_ROWPITCH + (lc & 1) * SF_PLANE + px * 128;
                        *(v8*)(dst + (((2 * lane_g) ^ (px & 6)) << 4)) = o0;          // channels 16g .. 16g+7   = chunk 2g
                        *(v8*)(dst + (((2 * lane_g + 1) ^ (px & 6)) << 4)) = o1;      // channels 16g+8 .. 16g+15 = chunk 2g + 1
                    }
                }
            }
        } else
        {
            int lane_s = s, lane_g = g;
            asm volatile("" : "+v"(lane_s), "+v"(lane_g));   // keep the per-group index math inside the loop (registers!)
            // first-conv weights: fragment ni, slot s -> channel (s>>2)*16 + ni*4 + (s&3): lane (g, .) owns channels 16g .. 16g+15
            v8 w1f[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) w1f[ni] = *(const v8*)(W1 + ((lane_s >> 2) * 16 + ni * 4 + (lane_s & 3)) * 32 + lane_g * 8);
            // per-image base pointer is wave-uniform (SGPRs); per-lane BYTE offsets inside one image fit 32 bits (unsigned: SGPR base +
            // 32-bit VGPR offset addressing, no 64-bit address arithmetic per element)
            constexpr int esz = (int)sizeof(IN);
            const char* ib = (const char*)p.in.data + (int64_t)b * p.in.stride_b * esz;
            const int sc = (int)p.in.stride_c * esz, sh = (int)p.in.stride_h * esz, sw = (int)p.in.stride_w * esz;
            // per-lane constants of the gather (r03): k slot 8g + e = (ky, kx, c) is fixed per lane, so its input offset and the border
            // cases it can hit are too -- the per-element k / 9, r9 / 3, four compares and the select chain (~35 VALU per element, 78 % of
            // the kernel in phase A: profiles/r03_stem_phase_accounting.log) collapse to one add and one bit test
            int koff[8];
            float nsc3[3], nsh3[3];   // uint8: this lane's normalisation constants
            unsigned m_valid = 0, m_ky0 = 0, m_ky2 = 0, m_kx0 = 0, m_kx2 = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = lane_g * 8 + e;
                const int ky = k / 9, r9 = k - ky * 9, kx = r9 / 3, c = r9 - kx * 3;
                koff[e] = c * sc + ky * sh + kx * sw;
                if constexpr (U8IN) {
                    if (e < 3) {   // k slot 8g + e holds channel (2g + e) % 3: three constants per lane, slot e takes number e % 3
                        nsc3[e] = c == 0 ? p.nscale[0] : (c == 1 ? p.nscale[1] : p.nscale[2]);
                        nsh3[e] = c == 0 ? p.nshift[0] : (c == 1 ? p.nshift[1] : p.nshift[2]);
                    }
                }
                m_valid |= (k < 27 ? 1u : 0u) << e;
                m_ky0 |= (ky == 0 ? 1u : 0u) << e;
                m_ky2 |= (ky == 2 ? 1u : 0u) << e;
                m_kx0 |= (kx == 0 ? 1u : 0u) << e;
                m_kx2 |= (kx == 2 ? 1u : 0u) << e;
            }
            // 9 groups per wave, SF_BATCH at a time: the scalar gathers of a batch are in flight together (with ~250 VGPRs there are
            // only two waves per SIMD to hide their latency; one group at a time costs nine memory round trips per tile)
            // touch the NEXT tile's input patch (r03): the gathers below are the first touch of their lines, i.e. memory-side latency three
            // times per tile and wave (12 of the 16.6 us a tile takes, profiles/r03_stem_phase_accounting.log).  One dword per 128-byte
            // line of the next tile's 35 rows x 3 planes x 67 columns, requested BEFORE this tile's gathers (which wait for the same kind of
            // miss anyway) and folded into a sink after them: a tile later its gathers find their lines in L2.
            unsigned pf0 = 0, pf1 = 0;
            const bool do_pf = false && esz == 4 && sw == esz && tile + per_xcd < t_end;   // measured r03: no gain (the gathers are instruction-bound, not miss-bound): off
            if (do_pf) {
                const TilePos np = tile_pos(tile + per_xcd, p.tiles_x, p.tiles_y, p.strips);   // (a strip tile's patch is 67 rows x 35 columns: not probed as such)
                const int nbi = np.b;
                const int y0 = 4 * np.y0 - 3, x0 = 4 * np.x0 - 3;     // 2 * (2 y0 - 1) - 1
                const unsigned* nib = (const unsigned*)((const char*)p.in.data + (int64_t)nbi * p.in.stride_b * 4);
                const int it0 = tid, it1 = tid + 256;                                  // 105 (row, plane) pairs x 4 column probes = 420 items
                const int rc0 = it0 >> 2, rc1 = it1 >> 2;
                const int xa = min(max(x0 + ((it0 & 3) < 3 ? 32 * (it0 & 3) : 66), 0), p.Wi - 1);
                const int xb = min(max(x0 + ((it1 & 3) < 3 ? 32 * (it1 & 3) : 66), 0), p.Wi - 1);
                const int ya = min(max(y0 + rc0 / 3, 0), p.Hi - 1), yb = min(max(y0 + rc1 / 3, 0), p.Hi - 1);
                pf0 = nib[rc0 < 105 ? ((rc0 % 3) * sc + ya * sh + xa * sw) >> 2 : 0];
                pf1 = nib[rc1 < 105 ? ((rc1 % 3) * sc + yb * sh + xb * sw) >> 2 : 0];
            }
            for (int g3 = wave; g3 < SF_GROUPS; g3 += 4 * SF_BATCH) {
                v8 xfb[SF_BATCH];
                int qv[SF_BATCH], lrv[SF_BATCH], lcv[SF_BATCH];
                bool v1v[SF_BATCH];
#pragma unroll
                for (int u = 0; u < SF_BATCH; ++u) {
                    const int q = (g3 + 4 * u) * 16 + lane_s;
                    const int lr = q / SF_COLS, lc = q - lr * SF_COLS;
                    const int R = r0 + (tr ? lc : lr), Cc = c0 + (tr ? lr : lc);
                    const bool v1 = q < SF_ROWS * SF_COLS && R >= 0 && R < p.H1 && Cc >= 0 && Cc < p.W1;
                    const int yi = 2 * R - 1, xi = 2 * Cc - 1;
                    qv[u] = q; lrv[u] = lr; lcv[u] = lc; v1v[u] = v1;
                    // rows / columns yi .. yi + 2, xi .. xi + 2 leave the image only through the first tap (yi = -1) or the last one
                    unsigned mask = v1 ? m_valid : 0u;
                    if (yi < 0) mask &= ~m_ky0;
                    if (yi + 2 >= p.Hi) mask &= ~m_ky2;
                    if (xi < 0) mask &= ~m_kx0;
                    if (xi + 2 >= p.Wi) mask &= ~m_kx2;
                    const int base = yi * sh + xi * sw;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const bool inb = (mask >> e) & 1u;
                        // always a legal address (the image's first element when masked), then select
                        const unsigned off = inb ? (unsigned)(base + koff[e]) : 0u;
                        float val = (float)*(const IN*)(ib + off);
                        if constexpr (U8IN) val = __builtin_fmaf(val, nsc3[e % 3], nsh3[e % 3]);
                        xfb[u][e] = (T)(inb ? val : 0.f);
                    }
                }
#pragma unroll
                for (int u = 0; u < SF_BATCH; ++u) {
                    const int q = qv[u], lr = lrv[u], lc = lcv[u];
                    const bool v1 = v1v[u];
                    f4 acc[4];
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[ni] = Op16<T>::mfma(w1f[ni], xfb[u], (f4){0.f, 0.f, 0.f, 0.f});
                    if (q < SF_ROWS * SF_COLS) {
                        v8 o0, o1;
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) {
                            const f4 bv = *(const f4*)(sb1 + lane_g * 16 + ni * 4);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float y = v1 ? fmaxf(acc[ni][r] + bv[r], 0.f) : 0.f;   // outside the conv1 map: conv2's zero padding
                                if (ni < 2) o0[ni * 4 + r] = (T)y; else o1[(ni - 2) * 4 + r] = (T)y;
                            }
                        }
                        const int px = lc >> 1;
                        char* dst = img + lr * SF_ROWPITCH + (lc & 1) * SF_PLANE + px * 128;
                        *(v8*)(dst + (((2 * lane_g) ^ (px & 6)) << 4)) = o0;          // channels 16g .. 16g+7   = chunk 2g
                        *(v8*)(dst + (((2 * lane_g + 1) ^ (px & 6)) << 4)) = o1;      // channels 16g+8 .. 16g+15 = chunk 2g + 1
                    }
                }
            }
            pf_sink ^= pf0 ^ pf1;
        }
        FVIT_SF_MARK(tsA)
        __syncthreads();
        FVIT_SF_MARK(tsBar)

        // ================= phase B: conv2 (stride 2) over the LDS image, weights in registers =================
        const char* hb = img + (2 * ph * 4) * SF_ROWPITCH;
        f4 acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
        v8 xf[2][4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) xf[0][mi] = *(const v8*)(hb + (2 * mi) * SF_ROWPITCH + xoff[0]);
        __builtin_amdgcn_sched_barrier(0);
        // as in conv3x3_c64_halo_kernel: tap (ky, kx) is at hb + ko[0][ky] + ko[1][kx]; a strip tile reads it at row shift kx, column offset xoff[ky]
        static_assert(SF_ROWPITCH % 256 == 0, "a row shift must leave bit 6 of a read offset alone");
        int ko[2][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ko[0][k] = tr ? xoff[k] : k * SF_ROWPITCH;
            ko[1][k] = tr ? k * SF_ROWPITCH : xoff[k];
        }
#pragma unroll
        for (int q = 0; q < 18; ++q) {
            const int tap = q >> 1, kk = q & 1;
            if (q + 1 < 18) {
                const int tap1 = (q + 1) >> 1, kk1 = (q + 1) & 1, ky1 = tap1 / 3, kx1 = tap1 - ky1 * 3;
                const int o = (ko[0][ky1] + ko[1][kx1]) ^ (kk1 << 6);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) xf[(q + 1) & 1][mi] = *(const v8*)(hb + (2 * mi) * SF_ROWPITCH + o);
            }
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = Op16<T>::mfma(wf[tap][kk][ni], xf[q & 1][mi], acc[ni][mi]);
            __builtin_amdgcn_sched_barrier(0);
        }

        FVIT_SF_MARK(tsB)
        // ---- epilogue: bias + ReLU of tile pixels (row 4ph + mi, s): out[b][y0 + row][x0 + s][nb .. nb+7], strip tile out[b][y0 + s][x0 + row] ----
        const f4 t0 = *(const f4*)(sb2 + nb), t1 = *(const f4*)(sb2 + nb + 4);
        const float bias[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = ph * 4 + mi;
            const int y = tp.y0 + (tr ? s : row), x = tp.x0 + (tr ? row : s);
            if (y < p.H2 && x < p.W2) {
                v8 ov;
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[ni * 4 + r] = (T)fmaxf(acc[ni][mi][r] + bias[ni * 4 + r], 0.f);
                *(v8*)(O + (((size_t)b * p.H2 + y) * p.W2 + x) * 64 + nb) = ov;
            }
        }
        FVIT_SF_MARK(tsE)
    }
    if (pf_sink == 0x9E3779B1u && p.tiles == -12345) ((unsigned*)p.out)[0] = pf_sink;   // never true
    if constexpr (TS) {
        if (p.ts && lane == 0) {
            unsigned long long* o = p.ts + ((size_t)blockIdx.x * 4 + wave) * 8;
            o[0] = tsA; o[1] = tsBar; o[2] = tsB; o[3] = tsE; o[4] = tsBar0; o[5] = tsN; o[6] = __builtin_amdgcn_s_memtime() - tsT0; o[7] = 0;
        }
    }
#undef FVIT_SF_MARK
}

// ------------------------------------------------------------------------------------------------------------
// The conv driver.  choose_conv_route is the only place that asks which kernel runs a 3x3 conv and the only reader of the route knobs;
// run_conv executes the answer and holds the only launch code.  Every entry point below fills a FvitConvWeights / FvitConvCall for it.
// ------------------------------------------------------------------------------------------------------------
enum ConvRoute : int {
    CR_NONE = -1,
    CR_HALO64, CR_HALO64_LN,       // conv3x3_c64_halo_kernel: 64 -> 64 channels, stride 1, classic single-term rows
    CR_BAND128, CR_BAND128_LN,     // conv3x3_c128_band_kernel: 128 -> 128 channels, stride 1, maps up to 30 wide, the fragment stream
    CR_PATCH, CR_PATCH_PX,         // conv3x3_kernel<.., HALO>: 8 x 16 output patches, classic rows
    CR_T128, CR_T128_DENSE, CR_T128_PX, CR_T128_PX_DENSE,   // the implicit GEMM, 128 pixels x 128 channels (+ 1: dense rows, + 2: two-term maps)
    CR_T64, CR_T64_DENSE, CR_T64_PX, CR_T64_PX_DENSE,       // 128 pixels x 64 channels, 48 KiB LDS: three workgroups per CU
    CR_T256X64,                    // 256 pixels x 64 channels, 80 KiB LDS (fvit_tune "conv64_variant" = 1)
    CR_COUNT
};
// route names = the kernel names of the per-launch profile records (prof_note); bm x bn: the implicit-GEMM tile (pixels x channels)
struct ConvRouteInfo { const char* name; int bm, bn; };
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

inline int out_size(int n, int stride) { return (n + 2 - 3) / stride + 1; }
// the two-term-map kernels (conv3x3_kernel<.., PX>): asked for by name or by any of their planes
inline bool call_is_px(const FvitConvCall& c) { return c.px || c.in_lo || c.residual_lo || c.out_lo || c.out_f32; }

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

// Launches route `r` (from choose_conv_route) of a validated call.  stamps: fvit_debug_conv_band_timeline (CR_BAND128, fp16).
template <typename T>
int run_conv(ConvRoute r, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream, void* stamps = nullptr) {
    const char* name = kConvRoutes[r].name;
    const int Ho = out_size(c.Hi, c.stride), Wo = out_size(c.Wi, c.stride), M = c.B * Ho * Wo;
    const bool ln = route_is_ln(r);   // the chooser checked: residual epilogue, no activation
    if (r == CR_HALO64 || r == CR_HALO64_LN) {
        if (ablate_skip(64)) return FVIT_OK;
        HaloParams p;
        p.ln_w = ln ? c.ln_w : nullptr; p.ln_b = c.ln_b; p.ln_eps = c.ln_eps;
        p.in = c.in; p.w = w.classic; p.bias = c.bias; p.res = c.residual; p.out = c.out; p.zeros = c.zeros;
        p.B = c.B; p.H = c.Hi; p.W = c.Wi; p.act = c.act;
        // Not a route: how the kernel tiles the map.  Not with GELU: a strip tile computes a pixel in another of the epilogue's four unrolled row copies, and
        // hipcc contracts gelu_fast's last step, hx * (z q) + hx with hx = 0.5 x, differently from copy to copy (fma(hx, z q, hx) or fma(0.5, x, hx * (z q)):
        // both are allowed), so a GELU map's bits depend on the pixel's row in its tile -- the bias / ReLU / residual / LayerNorm2d epilogues have no such choice
        const EdgeTiling et = edge_tiling(c.Hi, c.Wi, c.act != 2 && tune_get("conv_edge_tiles", 1));
        p.tiles_x = et.tiles_x; p.tiles_y = et.tiles_y; p.strips = et.strips;
        p.tiles = c.B * (p.tiles_x * p.tiles_y + p.strips);   // <= M, which fits int32
        p.ablate = diag_knob("conv_halo_ablate");
        int maxgrid = tune_get("conv_halo_grid", 512);   // 2 workgroups per CU (230 VGPRs, 46 KiB LDS each)
        if (maxgrid < 8) maxgrid = 8;                    // every XCD's tile range needs at least one workgroup
        // the launch shape is the plain tiling's, with or without the strip (launch records and roofline rows key on kernel name x workgroups): below the cap a
        // strip leaves a few workgroups with an empty tile range
        const EdgeTiling pt = edge_tiling(c.Hi, c.Wi, 0);
        const int plain_tiles = c.B * pt.tiles_x * pt.tiles_y;
        const int grid = plain_tiles < maxgrid ? plain_tiles : maxgrid;
        ProfScope prof(FVIT_K_CONV, 2.0 * M * 64.0 * 576.0, 2.0 * ((double)M * 64 * (c.residual ? 3.0 : 2.0) + 576.0 * 64), stream);
        prof_note(name, grid);
        p.buf_bytes = c.residual ? HALO_BUF : HALO_BYTES;
        // > 64 KiB of dynamic LDS needs the opt-in attribute (once per device and kernel instance)
        const void* kern = ln ? (const void*)conv3x3_c64_halo_kernel<T, true> : (const void*)conv3x3_c64_halo_kernel<T>;
        const size_t lds = ln ? HALO_LN_LDS : 1024 + 2 * (size_t)p.buf_bytes;
        static DeviceOnce once[2];
        if (once[ln].first_on_current_device()) hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, ln ? HALO_LN_LDS : 1024 + 2 * HALO_BUF);
        if (tune_get("conv_halo_debug", 0)) {
            int nb = -1;
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, lds);
            fprintf(stderr, "[fvit] %s: grid %d, tiles %d, dynamic LDS %zu B, resident workgroups/CU %d\n", name, grid, p.tiles, lds, nb);
        }
        if (ln) hipLaunchKernelGGL((conv3x3_c64_halo_kernel<T, true>), dim3(grid), dim3(256), lds, stream, p);
        else hipLaunchKernelGGL((conv3x3_c64_halo_kernel<T>), dim3(grid), dim3(256), lds, stream, p);
        return check_launch(name);
    }
    if (ablate_skip(32)) return FVIT_OK;
    if (r == CR_BAND128 || r == CR_BAND128_LN) {
        BandParams p;
        p.in = c.in; p.wf = w.band_frag; p.bias = c.bias; p.res = c.residual; p.out = c.out; p.zeros = c.zeros;
        p.B = c.B; p.H = c.Hi; p.W = c.Wi; p.act = c.act;
        p.ln_w = ln ? c.ln_w : nullptr; p.ln_b = c.ln_b; p.ln_eps = c.ln_eps;
        p.PW = c.Wi + 2;
        p.R = (BD_NG * 16) / p.PW;
        if (p.R > c.Hi) p.R = c.Hi;
        p.bands = (c.Hi + p.R - 1) / p.R;
        p.npieces = ((p.R + 2) * p.PW + 3) / 4;
        p.magic = (65536 + p.PW - 1) / p.PW;
        p.ts = (unsigned long long*)stamps;
        const dim3 grid(c.B * p.bands);
        ProfScope prof(FVIT_K_CONV, 2.0 * M * 128.0 * 1152.0, 2.0 * ((double)M * 128 * (c.residual ? 3.0 : 2.0) + 1152.0 * 128), stream);
        prof_note(name, c.B * p.bands);
        if (ln) hipLaunchKernelGGL((conv3x3_c128_band_kernel<T, false, true>), grid, dim3(256), 0, stream, p);
        else if (std::is_same<T, _Float16>::value && stamps) hipLaunchKernelGGL((conv3x3_c128_band_kernel<_Float16, true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((conv3x3_c128_band_kernel<T>), grid, dim3(256), 0, stream, p);
        return check_launch(name);
    }
    // the implicit GEMM: dense rows contract over cv real channels per tap, kd K steps; classic rows (cv = 0) over all Cin
    const bool px = call_is_px(c), dense = r >= CR_T128 && ((r - CR_T128) & 1), patch = r == CR_PATCH || r == CR_PATCH_PX;
    ConvParams p;
    p.in = c.in; p.w = dense ? w.dense : w.classic; p.bias = c.bias; p.res = c.residual; p.out = c.out; p.zeros = c.zeros;
    p.B = c.B; p.Hi = c.Hi; p.Wi = c.Wi; p.Cin = c.Cin; p.Cout = c.Cout; p.Ho = Ho; p.Wo = Wo; p.stride = c.stride; p.act = c.act; p.M = M;
    p.ablate = px ? 0 : diag_knob("conv_ablate"); p.wterms = w.terms;
    p.in_lo = c.in_lo; p.res_lo = c.residual_lo; p.out_lo = c.out_lo; p.out_f32 = c.out_f32; p.px = px;
    p.cv = dense ? w.cin_valid : 0; p.kd = dense ? (9 * p.cv + BK - 1) / BK : 0; p.inv_cv = dense ? 1.0f / (float)p.cv : 0.f;
    p.tiles_m = patch ? c.B * ((Ho + PATCH_H - 1) / PATCH_H) * ((Wo + PATCH_W - 1) / PATCH_W) : (M + kConvRoutes[r].bm - 1) / kConvRoutes[r].bm;
    p.tiles_n = (c.Cout + kConvRoutes[r].bn - 1) / kConvRoutes[r].bn;   // 128-column tiles: the last one may be ragged
    const double flops = 2.0 * M * (double)c.Cout * 9.0 * (dense ? p.cv : c.Cin);
    const double bytes = 2.0 * ((double)c.B * c.Hi * c.Wi * c.Cin * (c.in_lo ? 2.0 : 1.0) +
                                (double)M * c.Cout * ((c.residual ? (c.residual_lo ? 2.0 : 1.0) : 0.0) + ((c.out_lo || c.out_f32) ? 2.0 : 1.0)) + 9.0 * w.terms * c.Cin * c.Cout);
    ProfScope prof(FVIT_K_CONV, flops, bytes, stream);   // (the second weight term is a precision cost, not algorithmic FLOPs)
    prof_note(name, p.tiles_m * p.tiles_n);
    hipLaunchKernelGGL(gemm_kernel<T>(r), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, stream, p);
    return check_launch(name);
}

int launch_route(int32_t dtype, ConvRoute r, const FvitConvCall& c, const FvitConvWeights& w, fvit_stream_t stream, void* stamps = nullptr) {
    return dtype == FVIT_F16 ? run_conv<_Float16>(r, c, w, (hipStream_t)stream, stamps) : run_conv<__bf16>(r, c, w, (hipStream_t)stream, stamps);
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
    return launch_route(dtype, r, *c, *w, stream);
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
static_assert(BD_MAXPW == 32, "the W <= 30 in the messages of the row-band entry points");
int named_conv(const char* who, const char* need, int32_t dtype, FvitConvCall c, const void* classic, const void* band_frag, ConvRoute want, const float* ln_w,
               const float* ln_b, float eps, fvit_stream_t stream, void* stamps = nullptr) {
    const FvitConvWeights w{classic, nullptr, band_frag, 1, c.Cin};
    c.ln_w = ln_w; c.ln_b = ln_b; c.ln_eps = eps;
    ConvKnobs k;
    k.halo = k.band = 1;
    if (validate_conv(who, dtype, &w, &c) == FVIT_OK && choose_conv_route(c, w, k) == want) return launch_route(dtype, want, c, w, stream, stamps);
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

// A uint8 image goes through the _u8 entry points only (they carry the normalisation constants) and nothing else does: neither side ever reads
// the caller's bytes as another element type.  norm: scale[3] then shift[3] in HOST memory, copied into the kernel parameters at launch (no device
// allocation, no copy: safe under graph capture).
static bool stem_image_type_ok(const char* entry, const FvitMapView* in, const float* norm, bool u8_entry) {
    if (!u8_entry && in->dtype == FVIT_U8) {
        set_error("%s: a uint8 (FVIT_U8) image needs its normalisation constants: call %s_u8", entry, entry);
        return false;
    }
    if (u8_entry && in->dtype != FVIT_U8) {
        set_error("%s_u8: image dtype %d is not FVIT_U8: call %s", entry, in->dtype, entry);
        return false;
    }
    if (u8_entry && !norm) {
        set_error("%s_u8: null normalisation constants", entry);
        return false;
    }
    return true;
}

static int stem_conv_impl(const char* entry, int32_t dtype, const FvitMapView* in, const void* weight, const void* weight_lo, const float* bias, void* out,
                          int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream, const float* norm, bool u8_entry);

extern "C" int fvit_stem_conv3x3s2(int32_t dtype, const FvitMapView* in, const void* weight, const float* bias, void* out, int32_t B,
                                   int32_t Hi, int32_t Wi, fvit_stream_t stream) {
    return stem_conv_impl("fvit_stem_conv3x3s2", dtype, in, weight, nullptr, bias, out, B, Hi, Wi, stream, nullptr, false);
}

extern "C" int fvit_stem_conv3x3s2_px(int32_t dtype, const FvitMapView* in, const void* weight, const void* weight_lo, const float* bias, void* out,
                                      int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream) {
    return stem_conv_impl("fvit_stem_conv3x3s2_px", dtype, in, weight, weight_lo, bias, out, B, Hi, Wi, stream, nullptr, false);
}

extern "C" int fvit_stem_conv3x3s2_u8(int32_t dtype, const FvitMapView* in, const void* weight, const float* bias, void* out, int32_t B,
                                      int32_t Hi, int32_t Wi, fvit_stream_t stream, const float* norm) {
    return stem_conv_impl("fvit_stem_conv3x3s2", dtype, in, weight, nullptr, bias, out, B, Hi, Wi, stream, norm, true);
}

extern "C" int fvit_stem_conv3x3s2_px_u8(int32_t dtype, const FvitMapView* in, const void* weight, const void* weight_lo, const float* bias, void* out,
                                         int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream, const float* norm) {
    return stem_conv_impl("fvit_stem_conv3x3s2_px", dtype, in, weight, weight_lo, bias, out, B, Hi, Wi, stream, norm, true);
}

static int stem_conv_impl(const char* entry, int32_t dtype, const FvitMapView* in, const void* weight, const void* weight_lo, const float* bias, void* out,
                          int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream, const float* norm, bool u8_entry) {
    if (!in || !in->data || !weight || !bias || !out || B <= 0 || Hi <= 0 || Wi <= 0) {
        set_error("stem_conv: null or empty argument");
        return FVIT_EINVAL;
    }
    if (!stem_image_type_ok(entry, in, norm, u8_entry)) return FVIT_EINVAL;
    const bool u8 = u8_entry;
    StemParams p;
    for (int c = 0; c < 3; ++c) { p.nscale[c] = u8 ? norm[c] : 1.f; p.nshift[c] = u8 ? norm[3 + c] : 0.f; }
    p.in = *in; p.w = weight; p.w_lo = weight_lo; p.bias = bias; p.out = out; p.B = B; p.Hi = Hi; p.Wi = Wi;
    p.Ho = (Hi - 1) / 2 + 1;
    p.Wo = (Wi - 1) / 2 + 1;
    const int64_t M = (int64_t)B * p.Ho * p.Wo;
    if (M > 0x7fffffff) {
        set_error("stem_conv: too many output pixels");
        return FVIT_EINVAL;
    }
    p.M = (int)M;
    const int nblk16 = (p.M + 15) / 16;
    int grid = (nblk16 + 3) / 4;
    if (grid > 256 * 32) grid = 256 * 32;
    const double bytes = (double)B * 3 * Hi * Wi * (u8 ? 1 : in->dtype == FVIT_F32 ? 4 : 2) + 2.0 * M * 64;
    ProfScope prof(FVIT_K_CONV, 2.0 * M * 64 * 27, bytes, (hipStream_t)stream);
    if (u8 && dtype == FVIT_F16 && weight_lo) hipLaunchKernelGGL((stem_conv_kernel<_Float16, true, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (u8 && dtype == FVIT_BF16 && weight_lo) hipLaunchKernelGGL((stem_conv_kernel<__bf16, true, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (u8 && dtype == FVIT_F16) hipLaunchKernelGGL((stem_conv_kernel<_Float16, false, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (u8 && dtype == FVIT_BF16) hipLaunchKernelGGL((stem_conv_kernel<__bf16, false, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (dtype == FVIT_F16 && weight_lo) hipLaunchKernelGGL((stem_conv_kernel<_Float16, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (dtype == FVIT_BF16 && weight_lo) hipLaunchKernelGGL((stem_conv_kernel<__bf16, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (dtype == FVIT_F16) hipLaunchKernelGGL((stem_conv_kernel<_Float16>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else if (dtype == FVIT_BF16) hipLaunchKernelGGL((stem_conv_kernel<__bf16>), dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    else {
        set_error("stem_conv: dtype %d not supported (16-bit output only)", dtype);
        return FVIT_EINVAL;
    }
    return check_launch("stem_conv_kernel");
}

static int stem_fused_impl(int32_t dtype, const FvitMapView* in, const void* w1, const float* b1, const void* w2, const float* b2,
                           void* out, int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream, void* stamps, const float* norm = nullptr, bool u8_entry = false);

extern "C" int fvit_stem_fused(int32_t dtype, const FvitMapView* in, const void* w1, const float* b1, const void* w2, const float* b2,
                               void* out, int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream) {
    return stem_fused_impl(dtype, in, w1, b1, w2, b2, out, B, Hi, Wi, stream, nullptr);
}

extern "C" int fvit_stem_fused_u8(int32_t dtype, const FvitMapView* in, const void* w1, const float* b1, const void* w2, const float* b2,
                                  void* out, int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream, const float* norm) {
    return stem_fused_impl(dtype, in, w1, b1, w2, b2, out, B, Hi, Wi, stream, nullptr, norm, true);
}

// diagnosis: the fp16 kernel with per-wave phase accumulators (u64 [workgroups <= 512][4 waves][8]: ticks in phase A, barrier after A, phase B,
// epilogue, barrier before A, tiles processed, total)
#ifdef FVIT_DIAG
extern "C" int fvit_debug_stem_timeline(const FvitMapView* in, const void* w1, const float* b1, const void* w2, const float* b2, void* out,
                                        int32_t B, int32_t Hi, int32_t Wi, void* stamps, fvit_stream_t stream) {
    if (!stamps) { set_error("debug_stem_timeline: null stamp buffer"); return FVIT_EINVAL; }
    return stem_fused_impl(FVIT_F16, in, w1, b1, w2, b2, out, B, Hi, Wi, stream, stamps);
}
#endif  // FVIT_DIAG

static int stem_fused_impl(int32_t dtype, const FvitMapView* in, const void* w1, const float* b1, const void* w2, const float* b2,
                           void* out, int32_t B, int32_t Hi, int32_t Wi, fvit_stream_t stream, void* stamps, const float* norm, bool u8_entry) {
    if (!in || !in->data || !w1 || !b1 || !w2 || !b2 || !out || B <= 0 || Hi <= 0 || Wi <= 0) {
        set_error("stem_fused: null or empty argument");
        return FVIT_EINVAL;
    }
    if (!stem_image_type_ok("fvit_stem_fused", in, norm, u8_entry)) return FVIT_EINVAL;
    const bool u8 = u8_entry;
    if (fvit::ablate_skip(128)) return FVIT_OK;
    StemFusedParams p;
    p.in = *in; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.out = out; p.B = B; p.Hi = Hi; p.Wi = Wi;
    p.H1 = (Hi - 1) / 2 + 1; p.W1 = (Wi - 1) / 2 + 1;
    p.H2 = (p.H1 - 1) / 2 + 1; p.W2 = (p.W1 - 1) / 2 + 1;
    const fvit::EdgeTiling et = fvit::edge_tiling(p.H2, p.W2, tune_get("conv_edge_tiles", 1));
    p.tiles_x = et.tiles_x; p.tiles_y = et.tiles_y; p.strips = et.strips;
    const int64_t tiles = (int64_t)B * ((int64_t)p.tiles_x * p.tiles_y + p.strips);
    if (tiles > 0x7fffffff || (int64_t)B * p.H2 * p.W2 > 0x7fffffff) {
        set_error("stem_fused: too many output pixels");
        return FVIT_EINVAL;
    }
    p.tiles = (int)tiles;
    p.ts = (unsigned long long*)stamps;
    for (int c = 0; c < 3; ++c) { p.nscale[c] = u8 ? norm[c] : 1.f; p.nshift[c] = u8 ? norm[3 + c] : 0.f; }
    int maxgrid = tune_get("stem_fused_grid", 512);
    if (maxgrid < 8) maxgrid = 8;
    // the launch shape is the plain tiling's (as in run_conv's halo launch): below the cap a strip leaves a few workgroups with an empty tile range
    const fvit::EdgeTiling pt = fvit::edge_tiling(p.H2, p.W2, 0);
    const int64_t plain_tiles = (int64_t)B * pt.tiles_x * pt.tiles_y;   // >= tiles, <= the pixel count checked above
    const int grid = plain_tiles < maxgrid ? (int)plain_tiles : maxgrid;
    // fp32 channels-last image (stride_c 1, stride_w 3, rows and images dword-addressable from the image base with 32-bit offsets): the contiguous-run gather
    // uint8 channels-last (the decoder's HWC): the same gather on nine contiguous bytes (at least two columns: a run never spans more than the row's neighbours)
    const bool nhwc3 = (in->dtype == FVIT_F32 || (u8 && Wi >= 2)) && in->stride_c == 1 && in->stride_w == 3 && in->stride_h == 3 * (int64_t)Wi &&
                       (int64_t)Hi * Wi * 12 < 0x7fffff00 && tune_get("stem_nhwc3", 1);
    if (u8 && !nhwc3 && ((in->stride_c < 0 ? -in->stride_c : in->stride_c) * 2 + (in->stride_h < 0 ? -in->stride_h : in->stride_h) * (int64_t)(Hi + 2) +
                         (in->stride_w < 0 ? -in->stride_w : in->stride_w) * (int64_t)(Wi + 2)) > 0x7fffff00) {
        set_error("stem_fused_u8: one image of the view spans more than 2 GiB");
        return FVIT_EINVAL;
    }
    const size_t lds = 1024 + SF_LDS + (nhwc3 ? 4096 : 0);
    const double M1 = (double)B * p.H1 * p.W1, M2 = (double)B * p.H2 * p.W2;
    const double bytes = (double)B * 3 * Hi * Wi * (u8 ? 1 : in->dtype == FVIT_F32 ? 4 : 2) + 2.0 * M2 * 64;
    ProfScope prof(FVIT_K_CONV, 2.0 * M1 * 64 * 27 + 2.0 * M2 * 64 * 576, bytes, (hipStream_t)stream);
    prof_note("stem_fused_kernel", grid);
#define FVIT_STEM_LAUNCH(T_, IN_, TS_)                                                                                                   \
    do {                                                                                                                                 \
        static DeviceOnce once;                                                                                                          \
        if (once.first_on_current_device())                                                                                              \
            hipFuncSetAttribute((const void*)stem_fused_kernel<T_, IN_, TS_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   \
        hipLaunchKernelGGL((stem_fused_kernel<T_, IN_, TS_>), dim3(grid), dim3(256), lds, (hipStream_t)stream, p);                      \
    } while (0)
#define FVIT_STEM_LAUNCH4(T_, IN_, TS_, N3_)                                                                                             \
    do {                                                                                                                                 \
        static DeviceOnce once;                                                                                                          \
        if (once.first_on_current_device())                                                                                              \
            hipFuncSetAttribute((const void*)stem_fused_kernel<T_, IN_, TS_, N3_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((stem_fused_kernel<T_, IN_, TS_, N3_>), dim3(grid), dim3(256), lds, (hipStream_t)stream, p);                  \
    } while (0)
#define FVIT_STEM_IN(T_)                                                                   \
    do {                                                                                   \
        if (nhwc3 && u8) FVIT_STEM_LAUNCH4(T_, uint8_t, false, true);                       \
        else if (u8) FVIT_STEM_LAUNCH(T_, uint8_t, false);                                  \
        else if (nhwc3) FVIT_STEM_LAUNCH4(T_, float, false, true);                          \
        else if (in->dtype == FVIT_F32) FVIT_STEM_LAUNCH(T_, float, false);                \
        else if (in->dtype == FVIT_F16) FVIT_STEM_LAUNCH(T_, _Float16, false);             \
        else if (in->dtype == FVIT_BF16) FVIT_STEM_LAUNCH(T_, __bf16, false);              \
        else { set_error("stem_fused: input dtype %d not supported", in->dtype); return FVIT_EINVAL; } \
    } while (0)
    if (stamps) {
        if (in->dtype != FVIT_F32) { set_error("debug_stem_timeline: fp32 input only"); return FVIT_EINVAL; }
        FVIT_STEM_LAUNCH(_Float16, float, true);
    } else if (dtype == FVIT_F16) {
        FVIT_STEM_IN(_Float16);
    } else if (dtype == FVIT_BF16) {
        FVIT_STEM_IN(__bf16);
    } else {
        set_error("stem_fused: dtype %d not supported (16-bit output only)", dtype);
        return FVIT_EINVAL;
    }
#undef FVIT_STEM_IN
#undef FVIT_STEM_LAUNCH4
#undef FVIT_STEM_LAUNCH
    return check_launch("stem_fused_kernel");
}
