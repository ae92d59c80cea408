// gemm_common.h — device helpers shared by the GEMM-shaped kernel files (gemm_f32 / gemm_split / gemm_probes / gemm_bf16 / gemm_planes /
// rows_bf16 / deform_bf16): vector types, masked loads, the tile order, the three erf-GELU forms and the fp32 epilogue.  Everything lives in
// namespace brn; the files compiled a second time inside brn::hf (gemm_bf16.hip, rows_bf16.hip, deform_bf16.hip) see these names from there.
#pragma once
#include "../brn_kernels.h"
#include "split_planes.h"   // f32x4, the bf16 vector types and the P-layout stores

namespace brn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
// a load the optimiser may not sink under the predicate that later selects its value: hipcc turns `ok ? *p : 0` (and
// `t = *p; ok ? t : 0`) into an exec-branch around the load, and then waits vmcnt(0) before the first use of ANY staged
// register in the loop, draining the prefetched K tiles every iteration.
// So: load from a clamped (always valid) address, remember a ~0 / 0 bit mask, and AND the value with it when the staged
// registers are consumed (at the LDS store) — never a select at the load, never an operation on the data at the load (that
// would wait for it right there).  An integer AND, not a multiply by 0/1: the clamped address holds real data (pixel (0,0) of
// the window, row 0), and Inf * 0 = NaN would leak a non-finite input into every zero-padded border output.
__device__ __forceinline__ f32x4 load4_masked(const float* ptr, bool ok, unsigned& keep) {
    keep = ok ? 0xffffffffu : 0u;
    return *reinterpret_cast<const f32x4*>(ptr);
}
__device__ __forceinline__ f32x4 and4(const f32x4 v, const unsigned keep) {
    return __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, v) & keep);
}

// ---- x.gelu_erf() (candle: 0.5 x (1 + erf(x / sqrt 2)), swin.rs:103) in three forms.  Which one a call site uses is part of its numerics ----
// gelu_erf: the fp32 epilogues (gemm_f32 / gemm_split / splitk_reduce).  Branch-free and with ONE transcendental (round 4):
//     gelu(x) = relu(x) - |x| h(|x|),   h(u) = erfc(u / sqrt 2) / 2 = 2^P(u),
// P a degree-7 polynomial — log2 of the Gaussian tail is nearly a parabola, and one v_exp_f32 undoes it.  1 clamp + 7 fma + v_exp + max
// + fma = 14 issue slots; gelu_erf_as, which it replaced there (v_rcp + v_exp + 7 fma + a select, ~26 slots), cost the fc1 epilogues
// 6 us per 5120 x 3072 GEMM, libm's erff 18.  Neither side of zero cancels: for x >= 0 the result is x minus a term <= 0.17.
// Coefficients: weighted least squares on [0, 8] against scipy's erfc, rounded to fp32, and the whole form re-evaluated in emulated fp32 on
// 3e6 points of [-60, 60]: |gelu error| < 4.9e-7 for |x| <= 6 (the fp32 rounding of the result itself is 2.4e-7 there), half an ulp of x
// beyond.  u is clamped at 8: |x| 2^P(8) < 1e-6 |x| 2^-29.
__device__ __forceinline__ float gelu_erf(float x) {
    float u, r;
    asm("v_min_f32 %0, |%1|, %2" : "=v"(u) : "v"(x), "v"(8.0f));         // (plain v_min / v_max: fminf / fmaxf put a canonicalising
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(0.0f));           // v_max x, x in front of each; x is an MFMA / fma result, never signalling)
    float p = 2.0329723611212103e-06f;
    p = fmaf(p, u, 1.31221850097063e-05f);
    p = fmaf(p, u, -0.0006936025456525385f);
    p = fmaf(p, u, 0.007940512150526047f);
    p = fmaf(p, u, -0.05327853187918663f);
    p = fmaf(p, u, -0.45883336663246155f);
    p = fmaf(p, u, -1.1511898040771484f);
    p = fmaf(p, u, -0.9999935030937195f);
    return fmaf(-fabsf(x), __builtin_amdgcn_exp2f(p), r);
}
// gelu_erf_as: the fp32-out and per-element epilogues of gemm_bf16.hip and all of gemm_planes.hip.  The Abramowitz-Stegun form
// erfc(s) = t (c1 + t (c2 + ...)) exp(-s^2), t = 1 / (1 + 0.3275911 s), with seven refitted coefficients: |erfc error| < 2e-7 as a fit,
// |gelu error| < 6.1e-7 for |x| <= 6 measured like gelu_erf's figure above.  Two transcendentals (v_rcp, v_exp) and a select on the sign.
__device__ __forceinline__ float gelu_erf_as(float x) {
    const float s = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, s, 1.0f));
    float q = -0.29582387555232f;
    q = fmaf(q, t, 1.4920114662361241f);
    q = fmaf(q, t, -2.0596673810742456f);
    q = fmaf(q, t, 2.012361787754068f);
    q = fmaf(q, t, -0.7324354234987704f);
    q = fmaf(q, t, 0.42581723346182204f);
    q = fmaf(q, t, 0.15773620453694617f);
    q = q * t * __expf(-s * s);
    const float one_plus_erf = x < 0.f ? q : 2.0f - q;
    return 0.5f * x * one_plus_erf;
}
// gelu_erf_bf16out: for a result that is rounded to bf16 right away (gemm_bf16.hip: epilogue flavour 0; rows_bf16.hip: the weight-stationary kernel).
// fc1's epilogue is VALU time the persistent workgroup cannot hide behind MFMAs (20 % of an fc1 launch with the round-2 form: erfc by
// Abramowitz-Stegun 7.1.25, 3 terms = 9 VALU + v_rcp + v_exp, |error| < 2.6e-5), so the form is chosen by issue slots.  Round 4: gelu_erf's
// form with P a degree-5 polynomial (P(u) ~ -1 - 1.15 u - 0.46 u^2 ...) — 1 clamp + 5 fma + v_exp + max + fma = 12 issue slots instead of
// 17, and a better fit: weighted least squares on [0, 8] (weights = the tolerance budget below; coefficients rounded to fp32 and the whole
// form re-evaluated in emulated fp32 over 5e6 points of [-40, 40]): |gelu error| < 3.0e-6 absolute and < 5.2e-5 relative for
// |gelu| >= 1e-2 — a hundredth of half a bf16 ulp (a fifth of half an fp16 ulp: the fp16 build, compute mode BRN_F16, keeps the form).
// Beyond u = 8 the clamp holds h at 2^-51.9: |x| h is below 1e-7 for every |x| < 1e9.
__device__ __forceinline__ float gelu_erf_bf16out(float x) {
    const float ax = fabsf(x);
    float u, r;
    asm("v_min_f32 %0, |%1|, %2" : "=v"(u) : "v"(x), "v"(8.0f));
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(0.0f));
    float p = -0.00040414920658804476f;
    p = fmaf(p, u, 0.006561775226145983f);
    p = fmaf(p, u, -0.050444595515728f);
    p = fmaf(p, u, -0.46150773763656616f);
    p = fmaf(p, u, -1.150171160697937f);
    p = fmaf(p, u, -1.0000925064086914f);
    return fmaf(-ax, __builtin_amdgcn_exp2f(p), r);
}

// ---- tile order ----
// first id of the contiguous run XCD `xcd` owns when n ids are dealt over the 8 XCDs (blocks with the same blockIdx % 8 share an XCD's L2)
__device__ __forceinline__ int xcd_run_start(int xcd, int n) {
    const int q = n >> 3, r = n & 7;
    return xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
}
// one workgroup per work item: blocks that share an XCD walk a contiguous run of ids (bijective remap of blockIdx.x over gridDim.x)
__device__ __forceinline__ int xcd_remap() { return xcd_run_start(blockIdx.x & 7, gridDim.x) + (blockIdx.x >> 3); }

// tile id -> (m tile, n tile): N is walked in groups of GN tile columns, M fastest-but-one inside a group, so that while an XCD
// marches down M the GN weight panels of the group stay in its 4 MiB L2 and every A panel is fetched once per group
// (the split-bf16 kernels are bound by L2-miss traffic, not by the matrix pipe).
__device__ __forceinline__ void tile_coords(int tile, int tilesM, int tilesN, int& tm, int& tn) {
    constexpr int GN = 8;
    const int per_group = tilesM * GN;
    const int g = tile / per_group, r = tile - g * per_group;
    const int gw = min(GN, tilesN - g * GN);
    tm = r / gw;
    tn = g * GN + (r - tm * gw);
}

constexpr int BK = 32;      // K elements per tile of the register-staged kernels (gemm_f32_kernel, gemm_split_kernel); K % BK == 0

// What a one-tile-per-workgroup kernel works on. split-K: grid = tiles x splitk; slice s of a tile contracts K tiles
// [s * kts, (s + 1) * kts) = [kt0, nk) of `kstep` elements each and writes raw partial sums.
struct TileSlice { int slice, m0, n0, kt0, nk; };
template <int BM, int BN>
__device__ __forceinline__ TileSlice tile_slice(const GemmParams& p, int kstep) {
    const int tilesM = (p.M + BM - 1) / BM, tilesN = (p.N + BN - 1) / BN;
    const int swz = xcd_remap(), ntiles = tilesN * tilesM;
    TileSlice t;
    t.slice = swz / ntiles;
    int tile_m, tile_n;
    tile_coords(swz - t.slice * ntiles, tilesM, tilesN, tile_m, tile_n);
    t.m0 = tile_m * BM;
    t.n0 = tile_n * BN;
    const int nk_all = p.K / kstep;
    const int kts = (nk_all + p.splitk - 1) / p.splitk;
    t.kt0 = t.slice * kts;
    t.nk = min(nk_all, t.kt0 + kts);
    return t;
}

// Implicit GEMM over channels-last maps: k = (tap, channel), tap = ky * kw + kx.  Cin is a multiple of the K tile, so a K tile lies inside
// one tap: `tap` and its first channel `ci0`; the tap's place in the window is (ky, kx) x the dilation.
struct ConvTap { int tap, ci0, ky, kx; };
__device__ __forceinline__ ConvTap conv_tap_at(const GemmParams& p, int tap, int ci0) {
    const int ky = tap / p.kw;
    return ConvTap{tap, ci0, ky, tap - ky * p.kw};
}
__device__ __forceinline__ ConvTap conv_tap(const GemmParams& p, int k0) {
    const int tap = k0 / p.Cin;
    return conv_tap_at(p, tap, k0 - tap * p.Cin);
}

// Per-row state of a register-staged A loader, fixed over the K loop.  Dense: base = the row's offset.  Channels-last implicit GEMM
// (row m = output pixel (b, oy, ox)): base = the offset of image b's window, (iy, ix) = the input pixel under tap (0, 0).
template <int MODE>
__device__ __forceinline__ void gather_row_init(const GemmParams& p, int m, bool& ok, long& base, int& iy, int& ix) {
    ok = m < p.M;
    iy = 0; ix = 0;
    if (MODE == GEMM_DENSE) {
        base = (long)m * p.lda;
    } else {
        const int hw = p.Hout * p.Wout;
        const int b = m / hw, rem = m - b * hw;
        const int oy = rem / p.Wout, ox = rem - oy * p.Wout;
        iy = oy * p.stride - p.pad;
        ix = ox * p.stride - p.pad;
        base = (long)b * p.Hin * p.Win * p.lda + p.a_coff;
    }
}
// The register-staged A loader of dense and channels-last implicit-GEMM rows (MODE: GEMM_DENSE or GEMM_CONV_NHWC): floats k0 + 4 kq .. + 3 of
// a thread's PA rows.  An unconditional load from a clamped address + the keep mask (load4_masked: no exec branch around the load, so the
// compiler keeps counted vmcnt waits); rows >= M and taps in the padding are masked.
// (The parameters come by address: behind a reference the compiler speculates the loads of p.Hin / p.Win and drops the short circuit of the
// bounds test — other code than the three loaders this replaced, profiles/isa_parity_gemm_split.md.)
template <int MODE, int PA>
__device__ __forceinline__ void gather_rows_load(const GemmParams* pp, int k0, int kq, const bool (&ok)[PA], const long (&base)[PA], const int (&iy)[PA],
                                                 const int (&ix)[PA], f32x4 (&qa)[PA], unsigned (&qm)[PA]) {
    const GemmParams& p = *pp;
    if (MODE == GEMM_DENSE) {
#pragma unroll
        for (int i = 0; i < PA; ++i) qa[i] = load4_masked(p.A + (ok[i] ? base[i] : 0) + k0 + kq * 4, ok[i], qm[i]);
    } else {
        const ConvTap t = conv_tap(p, k0);
        const int dy = t.ky * p.dil, dx = t.kx * p.dil;
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            const int y = iy[i] + dy, x = ix[i] + dx;
            const bool in = ok[i] && (unsigned)y < (unsigned)p.Hin && (unsigned)x < (unsigned)p.Win;
            const long off = in ? base[i] + ((long)y * p.Win + x) * p.lda + t.ci0 : (long)p.a_coff;
            qa[i] = load4_masked(p.A + off + kq * 4, in, qm[i]);
        }
    }
}

// ---- the fp32 epilogue of gemm_f32_kernel and the split kernels, for four consecutive columns n .. n + 3 of one row ----
__device__ __forceinline__ f32x4 act4(f32x4 v, int act) {
    if (act == ACT_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
    } else if (act == ACT_GELU_ERF) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_erf(v[e]);
    }
    return v;
}
// what is fixed over the rows: the launch's uniform switches and the per-column vectors
struct EpiCols {
    bool split, vec;     // split-K partial sums; 16-byte accesses are aligned
    float* part;
    f32x4 bias, sc, sh;
};
__device__ __forceinline__ EpiCols epilogue_cols(const GemmParams& p, int slice, int n) {
    EpiCols c;
    c.split = p.splitk > 1;
    c.part = c.split ? p.part + (long)slice * p.M * p.N : nullptr;
    c.vec = c.split ? ((p.N & 3) == 0)
                    : (((p.N | p.ldc | p.c_coff) & 3) == 0 && (!p.R || ((p.ldr | p.r_coff) & 3) == 0));
    c.bias = zero4(); c.sh = zero4();
    c.sc = f32x4{1.f, 1.f, 1.f, 1.f};
    if (!c.split) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (n + e < p.N) {
                if (p.bias) c.bias[e] = p.bias[n + e];
                if (p.scale) { c.sc[e] = p.scale[n + e]; c.sh[e] = p.shift[n + e]; }
            }
        }
    }
    return c;
}
// v = the accumulators of (m, n .. n + 3), m < M and n < N.  OUT16: the launch may ask for a bf16 / fp16 map (p.c_bf16; the per-wave
// epilogue).  PLANES: it may ask for the P layout (p.c_planes; the tile epilogue).  A kernel family never tests the other's switch.
template <bool OUT16, bool PLANES>
__device__ __forceinline__ void epilogue_row(const GemmParams& p, const EpiCols& c, int m, int n, f32x4 v) {
    if (p.h2) v = v * p.out_scale;           // mode f32_half2: the operands were scaled by powers of two (exact)
    if (c.split) {
        float* dst = c.part + (long)m * p.N + n;
        if (c.vec) *reinterpret_cast<f32x4*>(dst) = v;
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (n + e < p.N) dst[e] = v[e];
        }
        return;
    }
    v = v + c.bias;
    if (p.bbias) {
        const float* bp = p.bbias + (long)(m / p.bbias_rows) * p.N + n;
        if (c.vec) v = v + *reinterpret_cast<const f32x4*>(bp);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (n + e < p.N) v[e] += bp[e];
        }
    }
    if (p.scale) v = v * c.sc + c.sh;
    v = act4(v, p.act);
    float* dst = p.C + (long)m * p.ldc + p.c_coff + n;
    if (OUT16 && p.c_bf16 == 2) {          // compute mode BRN_F16: fp16 map out
        _Float16* db = reinterpret_cast<_Float16*>(p.C) + (long)m * p.ldc + p.c_coff + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (n + e < p.N) db[e] = (_Float16)v[e];
    } else if (OUT16 && p.c_bf16) {        // compute mode BRN_BF16 (deformable gather convs): bf16 map out, no residual on this path
        __bf16* db = reinterpret_cast<__bf16*>(p.C) + (long)m * p.ldc + p.c_coff + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (n + e < p.N) db[e] = (__bf16)v[e];
    } else if (PLANES && p.c_planes) {     // the next GEMM reads the P layout (launch_gemm checked N, c_coff % 32 == 0, no R)
        if (p.h2) store_planes_h(p.C + (long)m * p.ldc, p.c_coff + n, v, p.a_scale);     // (the next GEMM's A scale is this one's: one scale per model)
        else store_planes_n(p.c_planes, p.C + (long)m * p.ldc, p.c_coff + n, v);
    } else if (c.vec) {
        if (p.R) v = v + *reinterpret_cast<const f32x4*>(p.R + (long)m * p.ldr + p.r_coff + n);
        *reinterpret_cast<f32x4*>(dst) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (n + e < p.N) {
                float t = v[e];
                if (p.R) t += p.R[(long)m * p.ldr + p.r_coff + n + e];
                dst[e] = t;
            }
        }
    }
}

// Per-wave epilogue (gemm_f32_kernel, gemm_split_kernel: the same 32x32 C/D register map).
// Each 32x32 accumulator tile is transposed through a wave-private LDS patch (rows of 36 floats) so that the global side
// is row-major float4: 8 lanes cover one 128-byte row segment, residual / per-image-bias loads and the stores are 16 B
// per lane, and only one float4 of temporaries is live per lane.
constexpr int EPI_LD = 36;
constexpr int EPI_WAVE_FLOATS = 32 * EPI_LD;

template <int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x16 (&acc)[TM][TN], int m0, int n0, int wm, int wn, int lane,
                                              int slice, float* patch /* EPI_WAVE_FLOATS floats private to this wave */) {
    const int col = lane & 31, rhalf = (lane >> 5) * 4;      // C/D map: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    const int rrow = lane >> 3, c4 = (lane & 7) * 4;         // read-back map: 8 rows x 8 float4 per pass
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * WTN + j * 32 + c4;
        const EpiCols c = epilogue_cols(p, slice, n);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) patch[((r & 3) + 8 * (r >> 2) + rhalf) * EPI_LD + col] = acc[i][j][r];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // same-wave LDS ops complete in order; make it explicit
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) {
                const int row = ps * 8 + rrow;
                const int m = m0 + wm * WTM + i * 32 + row;
                const f32x4 v = *reinterpret_cast<const f32x4*>(patch + row * EPI_LD + c4);
                if (m >= p.M || n >= p.N) continue;
                epilogue_row<true, false>(p, c, m, n, v);
            }
            __builtin_amdgcn_wave_barrier();   // the patch is rewritten by the next tile
        }
    }
}

// Workgroup-wide epilogue of the warp-specialised kernels: the C tile sits row-major in LDS (LD floats per row); 512 threads,
// thread t owns columns 4*(t&31).. of rows (t>>5) + 16*pass.
template <int BM, int BN, int LD>
__device__ __forceinline__ void gemm_epilogue_tile(const GemmParams& p, const float* ctile, int m0, int n0, int tid, int slice) {
    static_assert(BN == 128, "32 float4 columns per row");
    const int c4 = (tid & 31) * 4, r0 = tid >> 5;
    const int n = n0 + c4;
    if (n >= p.N) return;
    const EpiCols c = epilogue_cols(p, slice, n);
#pragma unroll 2
    for (int ps = 0; ps < BM / 16; ++ps) {
        const int row = ps * 16 + r0;
        const int m = m0 + row;
        if (m >= p.M) break;
        epilogue_row<false, true>(p, c, m, n, *reinterpret_cast<const f32x4*>(ctile + row * LD + c4));
    }
}

}  // namespace brn
