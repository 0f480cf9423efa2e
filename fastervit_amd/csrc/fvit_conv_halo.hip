// fvit_conv_halo.hip -- routes CR_HALO64 / CR_HALO64_LN of the conv driver (fvit_conv.hip), gfx950.
#include "fvit_conv.h"

namespace fvit {
namespace {

// ------------------------------------------------------------------------------------------------------------
// Halo-tiled 3x3 convolution for Cin = Cout = 64, stride 1 (ConvBlock convs of level 0, FV:502-512).
//
// The implicit GEMM (fvit_conv_gemm.hip) re-reads every input pixel nine times from L2 (once per tap) and the whole 72-KiB
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

constexpr int HALO_PW = HALO_TW + 2, HALO_PH = HALO_TH + 2;
constexpr int HALO_PIECES = (HALO_PH * HALO_PW + 7) / 8;       // 1-KiB pieces of 8 halo pixels
constexpr int HALO_BYTES = HALO_PIECES * 1024;
constexpr int HALO_RES_BYTES = HALO_TH * HALO_TW * 128;         // the tile's residual pixels, staged next to the halo
constexpr int HALO_BUF = HALO_BYTES + HALO_RES_BYTES;

constexpr int HALO_LN_LDS = 1024 + 2 * HALO_BUF + 1024;        // LN instance: 81 920 B, exactly half a CU's LDS (two workgroups per CU)

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

// ln: the chooser checked residual epilogue, no activation
template <typename T>
int launch(bool ln, const char* name, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream) {
    if (ablate_skip(64)) return FVIT_OK;
    const int M = c.B * c.Hi * c.Wi;   // stride 1
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

}  // namespace

int launch_conv_halo(int dtype, bool ln, const char* name, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream) {
    return dtype == FVIT_F16 ? launch<_Float16>(ln, name, c, w, stream) : launch<__bf16>(ln, name, c, w, stream);
}

}  // namespace fvit
