// Internal header of the 3x3 conv and stem units: what the conv driver (fvit_conv.hip) and the kernel units (fvit_conv_gemm.hip, fvit_conv_halo.hip,
// fvit_conv_band.hip, fvit_stem.hip) share -- only what at least two of them use.
#pragma once
#include "fvit_common.h"

namespace fvit {

// The routes of the conv driver (choose_conv_route, fvit_conv.hip): one per kernel instance family
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

inline int out_size(int n, int stride) { return (n + 2 - 3) / stride + 1; }
// the two-term-map kernels (conv3x3_kernel<.., PX>): asked for by name or by any of their planes
inline bool call_is_px(const FvitConvCall& c) { return c.px || c.in_lo || c.residual_lo || c.out_lo || c.out_f32; }

// The launch code of a route, one function per kernel unit: each fills its kernel's parameters from a validated call whose route the driver chose.
// dtype: FVIT_F16 or FVIT_BF16; name / info.name: the route's profile name.
int launch_conv_gemm(int dtype, ConvRoute r, const ConvRouteInfo& info, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream);
int launch_conv_halo(int dtype, bool ln, const char* name, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream);
bool band_supported(int H, int W);
// stamps: fvit_debug_conv_band_timeline (no LayerNorm2d, fp16)
int launch_conv_band(int dtype, bool ln, const char* name, const FvitConvCall& c, const FvitConvWeights& w, hipStream_t stream, void* stamps);

namespace {

constexpr int BK = 64;
constexpr int PATCH_H = 8, PATCH_W = 16;   // the output patch of conv3x3_kernel<.., HALO>
constexpr int HALO_TH = 8, HALO_TW = 16;   // the output tile of conv3x3_c64_halo_kernel and stem_fused_kernel

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

}  // namespace
}  // namespace fvit
