// fvit_conv_band.hip -- routes CR_BAND128 / CR_BAND128_LN of the conv driver (fvit_conv.hip), gfx950.
#include "fvit_conv.h"

namespace fvit {
namespace {

// ------------------------------------------------------------------------------------------------------------
// Row-band 3x3 convolution for Cin = Cout = 128, stride 1, maps up to 30 pixels wide (ConvBlock convs of level 1 of FasterViT-0:
// 28 x 28 x 128, FV:502-512), r03.
//
// The implicit GEMM (fvit_conv_gemm.hip) moves ~300 MB from L2 into LDS per launch at 86 images (every input pixel once per tap, the 288-KiB weight
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

// ln: the chooser checked residual epilogue, no activation.  stamps: the timeline instance (fp16, no LayerNorm2d)
template <typename T>
int launch(bool ln, const char* name, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream, void* stamps) {
    if (ablate_skip(32)) return FVIT_OK;
    const int M = c.B * c.Hi * c.Wi;   // stride 1
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

}  // namespace

static_assert(BD_MAXPW == 32, "the W <= 30 in the messages of the row-band entry points (fvit_conv.hip)");
bool band_supported(int H, int W) { return H >= 1 && W >= 1 && W + 2 <= BD_MAXPW; }

int launch_conv_band(int dtype, bool ln, const char* name, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream, void* stamps) {
    return dtype == FVIT_F16 ? launch<_Float16>(ln, name, c, w, stream, stamps) : launch<__bf16>(ln, name, c, w, stream, stamps);
}

}  // namespace fvit
