// Internal header shared by the HIP translation units of libfvit_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include <stdio.h>

#include "../../include/fvit_hip.h"

namespace fvit {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef __bf16 b4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// 16-bit MFMA operand traits: fp16 (default) or bf16, fp32 accumulate.
template <typename T> struct Op16;
template <> struct Op16<_Float16> {
    typedef h8 v8;
    typedef h4 v4;
    static __device__ __forceinline__ f4 mfma(v8 a, v8 b, f4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Op16<__bf16> {
    typedef b8 v8;
    typedef b4 v4;
    static __device__ __forceinline__ f4 mfma(v8 a, v8 b, f4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// Narrowing of an fp32 activation to the MFMA operand type.  fp16 SATURATES at +-65504 (one v_med3_f32): an activation beyond the
// fp16 range becomes the largest finite value instead of inf, so that no inf - inf / 0 * inf NaN can appear downstream (softmax of
// +-inf scores, a zero-padded weight column times inf) and a checkpoint with out-of-range activations degrades instead of
// poisoning the batch (tests/test_gpu_kernels.py::test_f16_operands_saturate).  bf16 has the fp32 exponent range: plain cast.
template <typename T> __device__ __forceinline__ T sat16(float x);
template <> __device__ __forceinline__ _Float16 sat16<_Float16>(float x) { return (_Float16)__builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f); }
template <> __device__ __forceinline__ __bf16 sat16<__bf16>(float x) { return (__bf16)x; }
// sat16 that keeps a NaN: v_med3_f32 returns the smallest operand when one is a NaN, so sat16<_Float16>(NaN) is -65504 -- a NaN pre-activation would leave a
// 16-bit epilogue as a large finite number.  The unit GEMM epilogues store through this form (tests/test_gpu_gemm_exact.py:
// test_gemm_nan_in_an_operand_comes_back_nan); the fused kernels keep sat16 (one compare and select per stored value on their VALU-bound epilogues).
template <typename T> __device__ __forceinline__ T sat16_nan(float x) { const T r = sat16<T>(x); return x != x ? (T)x : r; }

// Cross-row lane exchanges on the VALU (gfx950 v_permlane16_swap / v_permlane32_swap) instead of __shfl_xor, which is
// ds_bpermute_b32 -- an LDS-pipeline instruction.  r02 finding (profiles/r02_repeatability_hunt.log): in kernels that have LDS-DMA
// (global_load_lds) traffic landing in the workgroup's LDS, a ds_bpermute issued by a wave whose sibling waves' DMA is still in
// flight occasionally returned a wrong lane value when kernels of another stream shared the CU (the LayerNorm row mean of one wave
// off by a partial sum: all 16 rows of that wave shifted, ~1e-3 relative in the kernel's output, different run to run).  The swaps
// touch no LDS hardware, and are two VALU instructions instead of an LDS round trip.
//   v_permlane16_swap v, s: odd 16-lane rows of v <-> even rows of s; with v = s = x, {v, s} afterwards = {own or partner, partner or own}
//   of lane ^ 16 in a fixed order per lane pair, so op(v, s) is bitwise the same in both lanes of a pair for commutative op.
__device__ __forceinline__ float sum_xor16(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float sum_xor32(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float max_xor16(float x) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float max_xor32(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// all-reduce over groups of N consecutive lanes (N a power of two <= 64; every lane of a group gets the result): DPP inside a 16-lane
// row, the swaps above across rows -- no LDS-pipeline instruction.  quad_perm [1,0,3,2] / [2,3,0,1] are lane ^ 1 / lane ^ 2; after them
// every quad is uniform, so row_half_mirror (lane 7 - i of the 8-group) and row_mirror (lane 15 - i) pair each quad / half row with
// the other one exactly like lane ^ 4 / lane ^ 8 would.
template <int CTRL>
__device__ __forceinline__ float dpp_lane(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
template <int N>
__device__ __forceinline__ float group_sum(float x) {
    static_assert(N >= 1 && N <= 64 && (N & (N - 1)) == 0, "group size");
    if constexpr (N >= 2) x += dpp_lane<0xB1>(x);
    if constexpr (N >= 4) x += dpp_lane<0x4E>(x);
    if constexpr (N >= 8) x += dpp_lane<0x141>(x);
    if constexpr (N >= 16) x += dpp_lane<0x140>(x);
    if constexpr (N >= 32) x = sum_xor16(x);
    if constexpr (N >= 64) x = sum_xor32(x);
    return x;
}
template <int N>
__device__ __forceinline__ float group_max(float x) {
    static_assert(N >= 1 && N <= 64 && (N & (N - 1)) == 0, "group size");
    if constexpr (N >= 2) x = fmaxf(x, dpp_lane<0xB1>(x));
    if constexpr (N >= 4) x = fmaxf(x, dpp_lane<0x4E>(x));
    if constexpr (N >= 8) x = fmaxf(x, dpp_lane<0x141>(x));
    if constexpr (N >= 16) x = fmaxf(x, dpp_lane<0x140>(x));
    if constexpr (N >= 32) x = max_xor16(x);
    if constexpr (N >= 64) x = max_xor32(x);
    return x;
}

// Stage-boundary fusion (fvit_api.hip: "stage_entry_fused" / "stage_exit_fused"): a level's 16-bit channels-last map as the row source of the
// block-0 attention kernel, or as the destination of the last MLP kernel, in place of the window_partition / window_reverse passes.
// Unpadded maps only (H == Hp, W == Wp).  data == nullptr: not used.
struct RowMap {
    void* data = nullptr;
    int64_t stride_b = 0, stride_h = 0, stride_w = 0;   // in elements; the channel stride is 1
    int bf16 = 0;                                       // element type: 0 fp16, 1 bf16
    int S = 0, ncw = 0;                                 // rows per window, carrier rows in front of a window's local rows
    int ws = 0, nwx = 0, nw = 0;                        // window side, windows per row of windows, windows per image
};
// token_row of fvit_rows.hip inverted: element offset of the pixel behind row `row` of the window tensor; a carrier row gives -1
__device__ __forceinline__ int64_t rowmap_pixel(const RowMap& m, int64_t row) {
    const int64_t win = row / m.S;
    const int tok = (int)(row - win * m.S) - m.ncw;
    if (tok < 0) return -1;
    const int b = (int)(win / m.nw), wi = (int)(win - (int64_t)b * m.nw);
    const int wy = wi / m.nwx, wx = wi - wy * m.nwx, ty = tok / m.ws, tx = tok - ty * m.ws;
    return b * m.stride_b + (wy * m.ws + ty) * m.stride_h + (wx * m.ws + tx) * m.stride_w;
}
// the pixel's address, or null for a row that has no pixel (the caller then reads its fp32 row source)
__device__ __forceinline__ const char* rowmap_px(const RowMap& m, int64_t row) {
    const int64_t off = rowmap_pixel(m, row);
    return off >= 0 ? (const char*)m.data + 2 * off : nullptr;
}
// four channels of a map pixel (V4 = h4 / b4, 8-byte aligned) widened to fp32: the value window_partition stores
template <typename V4>
__device__ __forceinline__ f4 rowmap_load4(const void* px) {
    const V4 v = *(const V4*)px;
    f4 t;
#pragma unroll
    for (int r = 0; r < 4; ++r) t[r] = (float)v[r];
    return t;
}
// N groups of four channels, group i at channel off(i): ONE branch on the map's element type around the whole batch of loads
template <int N, typename OFF>
__device__ __forceinline__ void rowmap_load_row(f4 (&v)[N], const char* px, int bf16, OFF off) {
    if (bf16) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = rowmap_load4<b4>(px + 2 * off(i));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = rowmap_load4<h4>(px + 2 * off(i));
    }
}
// x rounded to the map type, as fp32: the value window_reverse stores
__device__ __forceinline__ float rowmap_round(float x, int bf16) { return bf16 ? (float)(__bf16)x : (float)(_Float16)x; }

// eight channels narrowed to the map type and stored at a pixel (16-byte aligned)
__device__ __forceinline__ void rowmap_store8(void* px, const float (&y)[8], int bf16) {
    if (bf16) {
        b8 o;
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = (__bf16)y[r];
        *(b8*)px = o;
    } else {
        h8 o;
#pragma unroll
        for (int r = 0; r < 8; ++r) o[r] = (_Float16)y[r];
        *(h8*)px = o;
    }
}

// nn.GELU() (exact-erf form, AR:403) without transcendentals: erf(z) ~ z * Q(z^2) on |z| <= 3 (degree-8 minimax fit,
// |erf error| <= 2.6e-5 incl. the clamp tail 1 - erf(3) = 2.2e-5), GELU absolute error <= 5.4e-5 on |x| <= 10.4 (below) -- an order of
// magnitude below the 16-bit rounding of the value it feeds (scripts/fit_gelu.py reproduces the fit and the bound).
// 14 plain VALU ops (SLP-packable into v_pk_fma_f32) instead of ~23 issue-cycle equivalents with rcp + exp: the fused
// epilogues are VALU-bound, not MFMA-bound, on this term.
// Outside |z| <= 3 the clamp of z leaves hx * (1 + z Q(9)): the positive tail x (1 - 0.52e-5) is a RELATIVE error far below a 16-bit rounding, the
// NEGATIVE tail is -0.52e-5 |x| where GELU is 0 -- inside 5.4e-5 down to x = -10.4, -1.3e-3 at x = -256 (tests/test_gpu_gemm_exact.py found it).
// gelu_fast_clamp_each holds x at -3 sqrt(2) first (the polynomial gives -2.2e-5 there against a true -4.7e-5 that only rises to 0) and meets 5.4e-5
// for every x; the unit GEMM epilogues use it.  The fused MLP and conv epilogues keep the form without it: one more VALU operation per value measured
// -1.2 % images/s on FasterViT-0 (profiles/gemm_attention_exact_tests.log), for pre-activations below -10 that a trained network's fc1 / conv outputs
// do not reach and an error that stays below one 16-bit rounding of the activations next to it down to x = -50.
constexpr float GELU_FAST_XMIN = -4.2426405f;
__device__ __forceinline__ float gelu_fast(float x) {
    const float z = __builtin_amdgcn_fmed3f(x * 0.70710678118654752f, -3.0f, 3.0f);
    const float u = z * z;
    float q = 4.075095461e-08f;
    q = q * u - 1.945139275e-06f;
    q = q * u + 4.106515917e-05f;
    q = q * u - 5.110726343e-04f;
    q = q * u + 4.235583358e-03f;
    q = q * u - 2.510324307e-02f;
    q = q * u + 1.110798195e-01f;
    q = q * u - 3.753151596e-01f;
    q = q * u + 1.128268480e+00f;
    const float hx = 0.5f * x;
    return hx * (z * q) + hx;
}

// gelu_fast over N values at once, every Horner step issued for all N values before the next step (r06).  The per-value form above compiles to
// ONE dependent chain of 15 VALU instructions per value and hipcc emits the values one after the other: the fused MLP kernels ran 32 such chains
// back to back per super-chunk (r05 ISA: 224 v_fmaak + 32 v_fmamk in strict dependence, ~3.5 issue cycles each instead of 2).  Source order alone
// does not survive (the DAG scheduler re-serialises the chains into the register-minimal order, and __builtin_amdgcn_sched_barrier has no data
// edge to them: r06 ISA check): an empty asm that takes all N partial results as read-write operands pins every step.  Same operations in the
// same order per value => bitwise the same results as gelu_fast.
template <int N>
__device__ __forceinline__ void pin_values(float (&q)[N]) {
    static_assert(N == 4 || N == 8, "pin_values: 4 or 8 values");
    // (not volatile: the data dependence alone orders the steps, and the statement stays free to move between independent instructions, e.g. MFMAs)
    if constexpr (N == 4) asm("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]));
    else asm("" : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]));
}
template <int N>
__device__ __forceinline__ void gelu_fast_n(float (&x)[N]) {
    float z[N], u[N], q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) z[i] = __builtin_amdgcn_fmed3f(x[i] * 0.70710678118654752f, -3.0f, 3.0f);
#pragma unroll
    for (int i = 0; i < N; ++i) u[i] = z[i] * z[i];
    pin_values(u);
#pragma unroll
    for (int i = 0; i < N; ++i) q[i] = 4.075095461e-08f * u[i] - 1.945139275e-06f;
#define FVIT_GELU_STEP(c) \
    pin_values(q);        \
    _Pragma("unroll") for (int i = 0; i < N; ++i) q[i] = q[i] * u[i] + (c);
    FVIT_GELU_STEP(4.106515917e-05f)
    FVIT_GELU_STEP(-5.110726343e-04f)
    FVIT_GELU_STEP(4.235583358e-03f)
    FVIT_GELU_STEP(-2.510324307e-02f)
    FVIT_GELU_STEP(1.110798195e-01f)
    FVIT_GELU_STEP(-3.753151596e-01f)
    FVIT_GELU_STEP(1.128268480e+00f)
#undef FVIT_GELU_STEP
    pin_values(q);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float hx = 0.5f * x[i];
        x[i] = hx * (z[i] * q[i]) + hx;
    }
}

// M values (a multiple of 4) in groups of 8 (+ one group of 4)
template <int M>
__device__ __forceinline__ void gelu_fast_each(float (&x)[M]) {
    static_assert(M % 4 == 0, "gelu_fast_each: a multiple of 4 values");
#pragma unroll
    for (int j = 0; j + 8 <= M; j += 8) {
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = x[j + i];
        gelu_fast_n<8>(t);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[j + i] = t[i];
    }
    if constexpr (M % 8 == 4) {
        float t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = x[M - 4 + i];
        gelu_fast_n<4>(t);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[M - 4 + i] = t[i];
    }
}

// gelu_fast_each with x held at GELU_FAST_XMIN first (above): GELU absolute error <= 5.4e-5 for every x.  The hold is a compare and select, NOT fmaxf:
// fmaxf drops a NaN operand (v_max_f32 returns the other one), and a NaN pre-activation -- NaN / Inf in an operand, an overflowed sum -- must leave the
// epilogue as NaN, not as a plausible -2.2e-5 (tests/test_gpu_gemm_exact.py: test_gemm_nan_in_an_operand_comes_back_nan).
template <int M>
__device__ __forceinline__ void gelu_fast_clamp_each(float (&x)[M]) {
#pragma unroll
    for (int i = 0; i < M; ++i) x[i] = x[i] < GELU_FAST_XMIN ? GELU_FAST_XMIN : x[i];
    gelu_fast_each<M>(x);
}

// nn.GELU() for the two-term-activation mode (weight_terms 3), which carries ~22 significant bits through every Linear layer: the polynomial above
// would be its error floor, and so was the Abramowitz-Stegun 7.1.26 erf used before -- its 1.5e-7 is an ABSOLUTE erf error, GELU multiplies it by 0.5 |x| (2.2e-7 at x = -3.25, where GELU
// itself is -1.9e-3), and 1 + erf(z) cancels for z < 0 (tests/test_gpu_gemm_exact.py: test_gemm_two_term_gelu_output).  Written on erfc of |x| / sqrt(2)
// instead, with the library erfcf (a few ulp RELATIVE): x < 0: 0.5 x erfc, x >= 0: x - 0.5 x erfc -- no cancellation on either side, the error is a few
// 2^-24 |GELU| plus one rounding of x.  These epilogues run behind three times the MFMA work of the 16-bit modes.
// Non-finite x: NaN gives NaN; +inf gives +inf and -inf gives -0 (the limits; the products inf * erfc(inf) = inf * 0 would be NaN).
__device__ __forceinline__ float gelu_erf(float x) {
    const float ax = fabsf(x);
    if (ax == __builtin_inff()) return x > 0.0f ? x : -0.0f;
    const float h = 0.5f * x * erfcf(ax * 0.70710678118654752f);
    return x < 0.0f ? h : x - h;
}
// gelu_erf over N values (the two-term-activation epilogues): the same operations per value
template <int N>
__device__ __forceinline__ void gelu_erf_n(float (&x)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = gelu_erf(x[i]);
}
template <int M>
__device__ __forceinline__ void gelu_erf_each(float (&x)[M]) {
    static_assert(M % 4 == 0, "gelu_erf_each: a multiple of 4 values");
#pragma unroll
    for (int j = 0; j + 8 <= M; j += 8) {
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = x[j + i];
        gelu_erf_n<8>(t);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[j + i] = t[i];
    }
    if constexpr (M % 8 == 4) {
        float t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = x[M - 4 + i];
        gelu_erf_n<4>(t);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[M - 4 + i] = t[i];
    }
}

__host__ __device__ constexpr int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline int64_t round_up64(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per DEVICE: remember which devices a kernel instance was opted in on
// (one static DeviceOnce per kernel instance; one process may drive several GPUs, e.g. nn.DataParallel in the reference's validate.py)
struct DeviceOnce {
    std::atomic<uint64_t> mask{0};
    bool first_on_current_device() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return true;   // unknown: just set the attribute again
        const uint64_t bit = 1ull << dev;
        return (mask.fetch_or(bit) & bit) == 0;
    }
};

// ---- error plumbing (thread-local message, negative return codes) ----
void set_error(const char* fmt, ...);
int check_launch(const char* what);

// ---- tuning knobs (A/B experiments inside one process; see fvit_tune in fvit_hip.h) ----
int tune_get(const char* key, int dflt);
// timing ablation (results are WRONG when non-zero; bench A/B only): skip the launches of a kernel family to measure its marginal cost
// inside the concurrent stream shards.  bits: 1 winmlp<256>, 2 winmlp<512>, 4 winblk, 8 attnblk, 16 ctblk, 32 conv3x3 implicit GEMM,
// 64 halo conv, 128 fused stem
// Measurement hazards live only in the DIAGNOSIS build (libfvit_hip_diag.so, -DFVIT_DIAG): the shipped library has no knob that
// can make a kernel skip work and no fvit_debug_* entry point.
#ifdef FVIT_DIAG
inline bool ablate_skip(int bit) { return (tune_get("ablate_skip", 0) & bit) != 0; }
inline int diag_knob(const char* key) { return tune_get(key, 0); }   // per-kernel ablation masks ("conv_ablate", "mlp_ablate", ...): results are WRONG when non-zero
#else
inline bool ablate_skip(int) { return false; }
inline int diag_knob(const char*) { return 0; }
#endif

// ---- diagnostics state (kernel timer records, row-hash / MLP traces, poison sink) is process-global: every access -- including
// the ones inside ProfScope, i.e. on every launch -- takes this mutex, so that host threads driving different devices / streams
// (nn.DataParallel replicas) may launch while a profile or a trace is being recorded.  Uncontended cost: one atomic per launch.
std::recursive_mutex& diag_mutex();

// ---- built-in kernel timer ----
struct ProfScope {
    ProfScope(int kind, double flops, double bytes, hipStream_t stream);
    ~ProfScope();
    int slot_;
    hipStream_t stream_;
};
// names the launch the innermost live ProfScope brackets: kernel family + launch shape (workgroups), so that the per-launch records
// (fvit_prof_records) can be matched with a rocprofv3 kernel trace / PMC row of the same (kernel, grid).  No-op when the timer is off.
void prof_note(const char* kernel, int grid);
bool prof_enabled();   // fvit_prof_enable(1) is active: a launcher that formats its launch name does so only then
#ifdef FVIT_DIAG
void dbg_poison_before_launch(hipStream_t st);   // diagnosis: register / LDS poison kernel in front of every launch (fvit_debug_poison_launches)
void dbg_rowhash(const char* tag, const void* ptr, long long rows, int row_bytes, hipStream_t st);   // no-op unless fvit_debug_rowhash_begin is active
#else
inline void dbg_poison_before_launch(hipStream_t) {}
inline void dbg_rowhash(const char*, const void*, long long, int, hipStream_t) {}
#endif

// ---- launchers (defined in the .hip files) ----
struct GemmCall {
    int dtype;           // FVIT_F16 / FVIT_BF16
    const void* A;       // activations op16 [pad128(M)][lda]
    int lda;
    const void* W;       // weights op16 [pad128(N)][ldw]
    int ldw;
    const float* bias;   // [N] or null
    const float* gamma;  // [N] or null (residual epilogue only)
    void* out;           // op16 [..][ldo] (bias / gelu) or f32 x [..][ldo] (residual)
    int ldo;
    int M, N, K;
    int epilogue;        // 0 bias, 1 bias+gelu, 2 gamma-residual into f32
    // residual epilogue only (optional): after the residual update, x[m][:] += add[add_idx ? add_idx[m % rows_per_image] : m % rows_per_image]
    // (rows of length N; negative index = none).  Used to apply the NEXT block's position embedding (AR:671: x = pos_embed(x)) in
    // the fc2 epilogue of the current block, so that the next block's norm1 has no in-place add and folds into its qkv GEMM.
    const float* add = nullptr;
    const int32_t* add_idx = nullptr;
    int rows_per_image = 1;
    // K-concatenated weight terms (FvitStageDesc.weight_terms): the weight rows hold K columns = terms x ka, the activation rows ka
    // columns that are re-used for every term (column k of the contraction reads A column k >= ka ? k - ka : k).  0 = K.
    // K = 3 ka (weight_terms 3, "x3"): weights [hi | lo | hi], activation rows hold TWO terms [hi | lo] (2 ka columns): the three
    // segments are hi.hi + hi_a.lo_w + lo_a.hi_w, i.e. both operands carried as two 16-bit terms, the lo.lo product dropped.
    int ka = 0;
    // epilogues 0 / 1: > 0 = the output is stored as two terms, hi at column n and lo = round(y - hi) at column out_lo_off + n
    int out_lo_off = 0;
    // residual epilogue: optional fp32 scratch for deterministic split-K (small grids with long K, see fvit_gemm.hip); nullptr = never split
    float* splitk_slab = nullptr;
    size_t splitk_bytes = 0;
};
int launch_gemm(const GemmCall& c, hipStream_t stream);

struct MlpFusedCall {
    int dtype;
    float* x;  // [M][C] f32 in place
    int M, C, hidden;
    const float* ln_w;
    const float* ln_b;
    float eps;
    const void* w1f;  // fragment-major fc1 weight
    const float* b1;
    const void* w2f;  // fragment-major fc2 weight
    const float* b2;
    const float* gamma;
    int terms = 1;    // weight terms (1, or 2 = [hi image | lo image]); fvit_winmlp.hip only
    // fvit_winmlp.hip, C = 512: split the hidden units of every 64-row group over nsplit (2 / 4) workgroups that meet in L2
    float* slab = nullptr;     // f32 [ceil(M / 64)][nsplit][64 x C], scratch
    int* counters = nullptr;   // int32 [ceil(M / 64)], zero before the first launch (the kernel leaves them zero)
    int nsplit = 1;
    void* ts = nullptr;        // diagnosis (fvit_debug_win_mlp_timeline): u64 [workgroups][waves][16] phase stamps
    // stage exit (winmlp_exit_supported): the epilogue rounds x + fc2 to the map type, normalises it over C (LayerNorm2d: out_ln_w / out_ln_b / out_eps)
    // and stores the local rows at their pixels of out_map; x is not written
    RowMap out_map;
    const float* out_ln_w = nullptr;
    const float* out_ln_b = nullptr;
    float out_eps = 0.f;
};
bool winmlp_exit_supported(const MlpFusedCall& c);   // the 4-wave C = 256 form without a layer scale, one or two weight terms
size_t winmlp_split_slab_bytes(int64_t M, int C, int nsplit);
bool mlp_fused_supported(int C, int hidden);
int launch_mlp_fused(const MlpFusedCall& c, hipStream_t stream);
// same contract for C = 512 / hidden 2048: 64-row workgroups whose 8 waves split hidden units / output channels (fvit_winmlp.hip)
bool winmlp_supported(int C, int hidden);
int launch_winmlp(const MlpFusedCall& c, hipStream_t stream);

struct AttnBlkCall {
    int dtype;
    // gather + LayerNorm source (fvit_gather_layernorm semantics)
    const float* srcA;
    int rowsA;
    const float* srcB;
    int rowsB;
    const int32_t* src_idx;
    const int32_t* add_idx;
    const float* add;
    const float* ln_w;
    const float* ln_b;
    float eps;
    int rows_per_image;
    // fragment-major weights
    const void* wqkv_f;
    const float* bqkv;
    const void* wproj_f;
    const float* bproj;
    const float* gamma;
    const float* bias;
    float* x_out;
    int nwin, S, heads, C;
    float scale;
    // fvit_winblk.hip, C = 512: split the heads of every window over two workgroups that meet in L2
    float* slab = nullptr;     // f32 [nwin][nsplit][64 x C], scratch
    int* counters = nullptr;   // int32 [nwin], zero before the first launch (the kernel leaves them zero)
    int nsplit = 1;
    int terms = 1;             // weight terms of the fragment arrays (fvit_winblk.hip, C = 512: 1 or 2; fvit_attnblk.hip: 1)
    void* ts = nullptr;        // fvit_attnblk.hip: stamp buffer of the timeline instance (fvit_debug_attn_block_timeline)
    RowMap map;                // stage entry (*_map_source_supported): rows with src_idx >= 0 (all rows without src_idx) come from this map, srcA is not read
};
bool attnblk_supported(int C, int heads, int S);
bool attnblk_map_source_supported(const AttnBlkCall& c);   // the default C = 256 window forms (one or two weight terms)
bool winblk_map_source_supported(const AttnBlkCall& c);    // every form but the split-heads one
int launch_attnblk(const AttnBlkCall& c, hipStream_t stream);
// r06: the same contract for C = 256 / 8 heads / 49..64-token windows with a wave per (window, head) (fvit_attnblk2.hip); launch_attnblk dispatches to it
bool attnblk2_supported(int C, int heads, int S);
int launch_attnblk2(const AttnBlkCall& c, hipStream_t stream);
// same contract for C = 512 / 16 heads, one 49..64-token window per workgroup, waves split heads / output channels (fvit_winblk.hip)
bool winblk_supported(int C, int heads, int S);
int launch_winblk(const AttnBlkCall& c, hipStream_t stream);
struct AttnCall {
    int dtype;
    const void* qkv;  // op16 [rows][ldq], columns [q|k|v][head][dpad]
    int ldq;
    void* out;        // op16 [rows][ldo], columns [head][dpad]
    int ldo;
    const float* bias;  // f32 [heads][Spad][Spad] (S <= FVIT_MAX_DENSE_SEQ)
    int nwin, S, heads, dpad;
    float scale;
    // S > FVIT_MAX_DENSE_SEQ: compact bias table f32 [heads][(2*rel_w-1)^2] (or null), n_g = rel_ng leading tokens without bias
    const float* rel_table;
    int rel_w, rel_ng;
    int d;  // real head_dim (<= dpad) for the FLOP count of the kernel timer; 0 = unknown (dpad is used)
    // two-term activations (weight_terms 3): qkv rows hold [q|k|v] hi at column 0 and lo at column q_lo_off; scores = qh.kh + qh.kl + ql.kh,
    // P and V as two terms too (P in registers), the output written as hi at column 0 and lo at column o_lo_off.  0 = single terms.
    int q_lo_off = 0, o_lo_off = 0;
    // train mode (r05): Dropout on the softmax probabilities (WindowAttention.attn_drop, FV:564): op16 [nwin * heads][S][Spad], 0 or 1 / keep; null = none
    const void* drop_mask = nullptr;
};
bool attention_dense(int S, int dpad);                               // in-register kernel + dense bias table, else the long kernel
int launch_attention(const AttnCall& c, hipStream_t stream);        // dispatches on attention_dense(S, dpad)
int launch_attention_long(const AttnCall& c, hipStream_t stream);   // fvit_attnlong.hip

struct LnCall {
    int dtype;
    const float* srcA;
    int rowsA;
    const float* srcB;
    int rowsB;
    const int32_t* src_idx;
    const int32_t* add_idx;
    const float* add;
    float* x_out;
    void* n_out;
    int ldn;
    const float* ln_w;
    const float* ln_b;
    float eps;
    int rows, rows_per_image, C;
    int lo_off = 0;   // > 0: n_out holds two terms per row, hi at column c and lo = round(y - hi) at column lo_off + c (ldn >= lo_off + pad64(C))
};
int launch_gather_layernorm(const LnCall& c, hipStream_t stream);

// LayerNorm folded into the A-operand staging of the Linear layer that consumes it (fvit_lngemm.hip); ln.n_out / ln.ldn are unused
// whole carrier-token branch of one HAT block (fvit_ctblk.hip)
struct CtBlkCall {
    int dtype;
    const float* X; int rowsA;        // window tensor, rows per image
    const int32_t* src_idx;           // [G]
    const float* add;                 // hat_pos_embed rows [G][C] or null
    float* R;                         // out [batch * G][C]
    int batch, G, heads, C, hidden;
    const float* ln1_w; const float* ln1_b; const void* wqkv_f; const float* bqkv; const void* wproj_f; const float* bproj; const float* gamma1;
    const float* bias; float scale;
    const float* ln2_w; const float* ln2_b; const void* w1f; const float* b1; const void* w2f; const float* b2; const float* gamma2;
    float eps;
    int terms = 1;   // weight terms of the four fragment arrays (1 or 2)
    void* ts = nullptr;   // stamp buffer of the timeline instance (fvit_debug_ct_block_timeline)
    int src_S = 0, src_ncw = 0;   // stage entry, src_S > 0: X is ct_init (rowsA = G rows per image, windowed order); row src_idx of the window tensor is its
                                  // row (src_idx / src_S) * src_ncw + src_idx % src_S
};
bool ctblk_supported(int C, int heads, int G, int hidden);
int launch_ctblk(const CtBlkCall& c, hipStream_t stream);

struct LnGemmCall {
    LnCall ln;           // row selection + LayerNorm parameters (x_out optional, must not alias the sources)
    const void* W;       // weights op16 [pad128(N)][ldw]
    int ldw;
    const float* bias;   // [N] or null
    void* out;           // op16 [..][ldo]
    int ldo;
    int N;
    int epilogue;        // 0 bias, 1 bias + GELU
};
bool ln_gemm_supported(int C, int N, int ldw, int ldo);
int launch_ln_gemm(const LnGemmCall& c, hipStream_t stream);

struct PartitionCall {
    FvitMapView in;  // (B, C, Hp, Wp)
    int batch, C, Hp, Wp, ws;
    float* x;          // token rows, f32, row length C
    int rows_per_win;  // S: rows reserved per window in x (ws*ws + ncw)
    int row_off;       // ncw: first local-token row inside a window
    const float* ct;   // optional (B, G, C) windowed carrier tokens copied into rows [0, ncw) (or null)
    int ncw;
};
int launch_partition(const PartitionCall& c, hipStream_t stream);

struct ReverseCall {
    const float* x;
    int rows_per_win, row_off;
    int batch, C, Hp, Wp, H, W, ws;
    FvitMapView out;       // (B, C, H, W)
    const float* gamma;    // propagation: out = x + gamma * x[carrier up_idx] (gamma null => 1)
    const int32_t* up_idx; // null => no propagation
};
int launch_reverse(const ReverseCall& c, hipStream_t stream);
// window_reverse with LayerNorm2d over C of the rounded row (16-bit channel-contiguous maps, C <= 512: reverse_ln_supported)
bool reverse_ln_supported(const ReverseCall& c);
int launch_reverse_ln(const ReverseCall& c, const float* ln_w, const float* ln_b, float eps, hipStream_t stream);
// out[b][c] = mean over the `rows` f32 rows of image b of the value rounded through the 16-bit type round_dtype
int launch_rows_avgpool(const float* x, float* out, int batch, int rows, int C, int round_dtype, hipStream_t stream);

// copy f32 rows [rows][C] out of / into the windowed tensor's carrier slots (block-level API)
int launch_ct_copy(float* x, int rows_per_win, int row_off, int ncw, float* ct, int nwin_total, int C, int to_x,
                   hipStream_t stream);
// TokenInitializer: depthwise conv3x3 + bias + AvgPool2d + per-window reorder -> f32 (B, G, C)
int launch_token_init(const FvitMapView& in, const float* w, const float* bias, float* out, int B, int C, int Hp, int Wp, int kh, int kw,
                      int sh, int sw, int cw, hipStream_t stream);
// x[win][ncw + t] += gamma * x[win][up_idx[t]] (block-level API; the stage API fuses this into window_reverse)
int launch_propagate(float* x, const float* gamma, const int32_t* up_idx, int rows_per_win, int ncw, int nloc,
                     int nwin_total, int C, hipStream_t stream);

}  // namespace fvit
