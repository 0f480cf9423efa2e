// fvit_stem.hip -- the stem of PatchEmbed on the caller's image (gfx950): the stride-2 3 -> 64 conv and the fused two-conv stem, with their entry points.
#include "fvit_conv.h"

namespace fvit {
namespace {

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

}  // namespace
}  // namespace fvit

using namespace fvit;

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

// one kernel instance: > 64 KiB of dynamic LDS needs the opt-in attribute (once per device and instance; an instance's lds is the same at every call)
template <typename T, typename IN, bool TS, bool NHWC3 = false>
static void stem_fused_launch(const StemFusedParams& p, int grid, size_t lds, fvit_stream_t stream) {
    static DeviceOnce once;
    if (once.first_on_current_device()) hipFuncSetAttribute((const void*)stem_fused_kernel<T, IN, TS, NHWC3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((stem_fused_kernel<T, IN, TS, NHWC3>), dim3(grid), dim3(256), lds, (hipStream_t)stream, p);
}
// the instance of output type T for the caller's image
template <typename T>
static int stem_fused_in(const FvitMapView* in, bool u8, bool nhwc3, const StemFusedParams& p, int grid, size_t lds, fvit_stream_t stream) {
    if (nhwc3 && u8) stem_fused_launch<T, uint8_t, false, true>(p, grid, lds, stream);
    else if (u8) stem_fused_launch<T, uint8_t, false>(p, grid, lds, stream);
    else if (nhwc3) stem_fused_launch<T, float, false, true>(p, grid, lds, stream);
    else if (in->dtype == FVIT_F32) stem_fused_launch<T, float, false>(p, grid, lds, stream);
    else if (in->dtype == FVIT_F16) stem_fused_launch<T, _Float16, false>(p, grid, lds, stream);
    else if (in->dtype == FVIT_BF16) stem_fused_launch<T, __bf16, false>(p, grid, lds, stream);
    else { set_error("stem_fused: input dtype %d not supported", in->dtype); return FVIT_EINVAL; }
    return FVIT_OK;
}

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
    // the launch shape is the plain tiling's (as in launch_conv_halo): below the cap a strip leaves a few workgroups with an empty tile range
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
    if (stamps) {
        if (in->dtype != FVIT_F32) { set_error("debug_stem_timeline: fp32 input only"); return FVIT_EINVAL; }
        stem_fused_launch<_Float16, float, true>(p, grid, lds, stream);
    } else if (dtype == FVIT_F16) {
        if (const int rc = stem_fused_in<_Float16>(in, u8, nhwc3, p, grid, lds, stream)) return rc;
    } else if (dtype == FVIT_BF16) {
        if (const int rc = stem_fused_in<__bf16>(in, u8, nhwc3, p, grid, lds, stream)) return rc;
    } else {
        set_error("stem_fused: dtype %d not supported (16-bit output only)", dtype);
        return FVIT_EINVAL;
    }
    return check_launch("stem_fused_kernel");
}
