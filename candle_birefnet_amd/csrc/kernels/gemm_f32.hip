// gemm_f32.hip — the one contraction kernel of the path: C = epilogue(A_gather[M,K] x W[N,K]^T) in exact fp32
// on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, 64 FLOP/clk/SIMD).
//
// It replaces every candle Linear / Conv2d the reference's hot path executes:
//   GEMM_DENSE        candle_nn::linear (swin.rs:98-99,130-131,487) and all 1x1 convs (decoder.rs:65, aspp.rs:271,282)
//   GEMM_CONV_NHWC    candle_nn::conv2d 3x3 / 7x7 (decoder.rs:44-45,104,113; aspp.rs:39-45; birefnet.rs:105)
//   GEMM_GATHER_NCHW  the two convs that read the NCHW image directly: PatchEmbed.proj 4x4 s4 (swin.rs:677) and
//                     ipt_blk1.conv1 3x3 (birefnet.rs:189)
//   GEMM_DEFORM_NHWC  the Metal path's deformable_im2col + matmul (aspp.rs:58-165) with the column matrix never
//                     materialised: the bilinear gather * modulator is the A-tile loader
// with bias / folded eval-BatchNorm / ReLU / erf-GELU / residual / concat-slice writes fused into the epilogue.
// The same contractions on the bf16 / fp16 matrix cores (the split modes) live in gemm_split.hip; this file keeps the planner and
// the dispatcher of both (plan_gemm, launch_gemm) and the split-K reduction.  Shared device helpers and the epilogue: gemm_common.h.
//
// Tiling (wave64): block tile BMxBN, BK = 32; WMxWN waves, each owning (BM/WM)x(BN/WN) as 32x32 MFMA tiles.
// The k index inside a BK tile is permuted: lane-half h of an MFMA step s contracts k = 16h + s, so a lane's
// sixteen A (or B) values of a tile are 16 consecutive floats of one LDS row = four ds_read_b128 (row stride
// 36 floats: conflict-free for the b128 lane groups).  Global->LDS goes through registers (one float4 per
// thread per 32 rows) with the next tile's loads in flight during the current tile's 64-cycle MFMAs.
#include <cstdlib>
#include "../brn_kernels.h"
#include "gemm_common.h"

namespace brn {

constexpr int LDS_LD = 36;

template <int BM, int BN, int WM, int WN, int MODE>
__global__ void __launch_bounds__(WM* WN * 64) gemm_f32_kernel(const GemmParams p) {
    constexpr int NT = WM * WN * 64;
    constexpr int RPP = NT / 8;  // tile rows covered by one pass of float4 loads (8 float4 = one 32-float row)
    constexpr int PA = BM / RPP, PB = BN / RPP;
    constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 32, TN = WTN / 32;
    static_assert(PA >= 1 && PB >= 1 && TM >= 1 && TN >= 1, "tile too small for the thread count");

    constexpr int SMEM_MAIN = (BM + BN) * LDS_LD, SMEM_EPI = WM * WN * EPI_WAVE_FLOATS;
    __shared__ __attribute__((aligned(16))) float smem[SMEM_MAIN > SMEM_EPI ? SMEM_MAIN : SMEM_EPI];
    float* As = smem;
    float* Bs = smem + BM * LDS_LD;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;

    // XCD-aware tile order: blocks that share an XCD (same blockIdx % 8) walk a contiguous run of tiles,
    // n fastest, so an A panel is fetched into that XCD's L2 once for all its N tiles (bijective remap).
    const TileSlice ts = tile_slice<BM, BN>(p, BK);
    const int slice = ts.slice, m0 = ts.m0, n0 = ts.n0, kt0 = ts.kt0, nk = ts.nk;

    const int kq = tid & 7, lrow = tid >> 3;

    // ---- per-row gather state (fixed over the K loop) ----
    long a_base[PA];
    int a_iy[PA], a_ix[PA];
    bool a_ok[PA];
    long om_base[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int m = m0 + lrow + i * RPP;
        gather_row_init<MODE>(p, m, a_ok[i], a_base[i], a_iy[i], a_ix[i]);
        if (MODE == GEMM_GATHER_NCHW) a_base[i] = (long)(m / (p.Hout * p.Wout)) * p.Cin * p.Hin * p.Win;
        om_base[i] = MODE == GEMM_DENSE ? 0 : (long)m * p.om_ld;
    }
    const float* wrow = p.W + (long)(n0 + lrow) * p.K + kq * 4;

    f32x4 ra[PA], rb[PB];
    unsigned am[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) am[i] = 0xffffffffu;

    auto gload = [&](int kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < PB; ++i) rb[i] = *reinterpret_cast<const f32x4*>(wrow + (long)i * RPP * p.K + k0);
        if constexpr (MODE == GEMM_DENSE || MODE == GEMM_CONV_NHWC) {
            gather_rows_load<MODE>(&p, k0, kq, a_ok, a_base, a_iy, a_ix, ra, am);
        } else if (MODE == GEMM_GATHER_NCHW && p.kw == 4 && p.stride == 4 && p.pad == 0 && p.dil == 1 && (p.Win & 3) == 0 && (reinterpret_cast<unsigned long long>(p.A) & 15) == 0) {
            // PatchEmbed (swin.rs:677: k 4, s 4, no padding) on an image whose width is a multiple of 4: a lane's four k indices
            // k4 .. k4 + 3 are the four kx of one (channel, ky) = 16 contiguous bytes of the image: one unpredicated float4 load from a
            // clamped address + the bit mask (the per-element form below costs 4 predicated scalar loads and 4 index divisions)
            const int k4 = k0 + kq * 4, khw = p.kh * 4;
            const int c = k4 / khw, ky = (k4 - c * khw) >> 2;
            const bool kin = k4 < p.Kreal;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const int iy = a_iy[i] + ky;
                const bool ok = a_ok[i] && kin && iy < p.Hin;              // (bottom rows of a height that is not a multiple of 4 are zero padding)
                const long off = ok ? a_base[i] + ((long)c * p.Hin + iy) * p.Win + a_ix[i] : 0;
                ra[i] = load4_masked(p.A + off, ok, am[i]);
            }
        } else if (MODE == GEMM_GATHER_NCHW) {
            const int khw = p.kh * p.kw;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = k0 + kq * 4 + e;
                    const int c = k / khw, rem = k - c * khw;
                    const int ky = rem / p.kw, kx = rem - ky * p.kw;
                    const int iy = a_iy[i] + ky * p.dil, ix = a_ix[i] + kx * p.dil;
                    const bool ok = a_ok[i] && k < p.Kreal && (unsigned)iy < (unsigned)p.Hin &&
                                    (unsigned)ix < (unsigned)p.Win;
                    v[e] = ok ? p.A[a_base[i] + ((long)c * p.Hin + iy) * p.Win + ix] : 0.f;
                }
                { f32x4 t = {v[0], v[1], v[2], v[3]}; ra[i] = t; }
            }
        } else {  // GEMM_DEFORM_NHWC: torchvision deform_conv2d sampling, 1 offset group, modulated
            const ConvTap t = conv_tap(p, k0);
            const int tap = t.tap, ci0 = t.ci0;
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                f32x4 r = zero4();
                if (a_ok[i]) {
                    const float* omr = p.om + om_base[i];
                    const float offy = omr[2 * tap], offx = omr[2 * tap + 1];
                    const float mk = omr[p.om_mask_off + tap];
                    const float y = (float)(a_iy[i] + t.ky * p.dil) + offy;
                    const float x = (float)(a_ix[i] + t.kx * p.dil) + offx;
                    if (y > -1.f && y < (float)p.Hin && x > -1.f && x < (float)p.Win) {
                        const int yl = (int)floorf(y), xl = (int)floorf(x);
                        const int yh = yl + 1, xh = xl + 1;
                        const float ly = y - (float)yl, lx = x - (float)xl;
                        const float hy = 1.f - ly, hx = 1.f - lx;
                        const long boff = a_base[i] + ci0 + kq * 4;
                        // compute mode BRN_BF16: the sampled map is bf16 (lda / a_coff in elements either way)
                        auto tap4 = [&](int yy, int xx) -> f32x4 {
                            const long o = boff + ((long)yy * p.Win + xx) * p.lda;
                            if (p.a_bf16 == 2) {               // compute mode BRN_F16: an fp16 map
                                typedef _Float16 f16x4_g __attribute__((ext_vector_type(4)));
                                const f16x4_g h = *reinterpret_cast<const f16x4_g*>(reinterpret_cast<const _Float16*>(p.A) + o);
                                f32x4 r4 = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                                return r4;
                            }
                            if (p.a_bf16) {
                                const bf16x4 h = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(p.A) + o);
                                f32x4 r4 = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                                return r4;
                            }
                            return *reinterpret_cast<const f32x4*>(p.A + o);
                        };
                        f32x4 v1 = zero4(), v2 = v1, v3 = v1, v4 = v1;
                        if (yl >= 0 && xl >= 0) v1 = tap4(yl, xl);
                        if (yl >= 0 && xh <= p.Win - 1) v2 = tap4(yl, xh);
                        if (yh <= p.Hin - 1 && xl >= 0) v3 = tap4(yh, xl);
                        if (yh <= p.Hin - 1 && xh <= p.Win - 1) v4 = tap4(yh, xh);
                        const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
                        r = mk * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
                    }
                }
                ra[i] = r;
            }
        }
    };
    auto lds_store = [&]() {
#pragma unroll
        for (int i = 0; i < PA; ++i)
            *reinterpret_cast<f32x4*>(As + (lrow + i * RPP) * LDS_LD + kq * 4) = and4(ra[i], am[i]);
#pragma unroll
        for (int i = 0; i < PB; ++i)
            *reinterpret_cast<f32x4*>(Bs + (lrow + i * RPP) * LDS_LD + kq * 4) = rb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const float* a_frag = As + (wm * WTM + (lane & 31)) * LDS_LD + (lane >> 5) * 16;
    const float* b_frag = Bs + (wn * WTN + (lane & 31)) * LDS_LD + (lane >> 5) * 16;

    if (kt0 < nk) {
        gload(kt0);
        lds_store();
    }
    __syncthreads();
    for (int kt = kt0; kt < nk; ++kt) {
        if (kt + 1 < nk) gload(kt + 1);
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
            float af[TM][8], bf[TN][8];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(a_frag + i * 32 * LDS_LD + hs * 8);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(a_frag + i * 32 * LDS_LD + hs * 8 + 4);
                af[i][0] = v0.x; af[i][1] = v0.y; af[i][2] = v0.z; af[i][3] = v0.w;
                af[i][4] = v1.x; af[i][5] = v1.y; af[i][6] = v1.z; af[i][7] = v1.w;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(b_frag + j * 32 * LDS_LD + hs * 8);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(b_frag + j * 32 * LDS_LD + hs * 8 + 4);
                bf[j][0] = v0.x; bf[j][1] = v0.y; bf[j][2] = v0.z; bf[j][3] = v0.w;
                bf[j][4] = v1.x; bf[j][5] = v1.y; bf[j][6] = v1.z; bf[j][7] = v1.w;
            }
#pragma unroll
            for (int s = 0; s < 8; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        if (kt + 1 < nk) {
            lds_store();
            __syncthreads();
        }
    }

    gemm_epilogue<TM, TN, WTM, WTN>(p, acc, m0, n0, wm, wn, lane, slice, smem + wave * EPI_WAVE_FLOATS);
}

// split-K second pass: fixed-order sum of the slices (deterministic) + the epilogue of gemm_f32_kernel
__global__ void splitk_reduce_kernel(const GemmParams p) {
    const long total = (long)p.M * p.N;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int m = (int)(idx / p.N), n = (int)(idx - (long)m * p.N);
        float v = 0.f;
        for (int s = 0; s < p.splitk; ++s) v += p.part[(long)s * total + idx];
        if (p.bias) v += p.bias[n];
        if (p.bbias) v += p.bbias[(long)(m / p.bbias_rows) * p.N + n];
        if (p.scale) v = v * p.scale[n] + p.shift[n];
        if (p.act == ACT_RELU) v = fmaxf(v, 0.f);
        else if (p.act == ACT_GELU_ERF) v = gelu_erf(v);
        if (p.R) v += p.R[(long)m * p.ldr + p.r_coff + n];
        p.C[(long)m * p.ldc + p.c_coff + n] = v;
    }
}

template <int BM, int BN, int WM, int WN>
static hipError_t launch_cfg(const GemmParams& p, hipStream_t s) {
    const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN) * p.splitk;
    dim3 grid(tiles), block(WM * WN * 64);
    switch (p.mode) {
        case GEMM_DENSE: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, WM, WN, GEMM_DENSE>), grid, block, 0, s, p); break;
        case GEMM_CONV_NHWC: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, WM, WN, GEMM_CONV_NHWC>), grid, block, 0, s, p); break;
        case GEMM_GATHER_NCHW: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, WM, WN, GEMM_GATHER_NCHW>), grid, block, 0, s, p); break;
        case GEMM_DEFORM_NHWC: hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, WM, WN, GEMM_DEFORM_NHWC>), grid, block, 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// Tile + split-K choice from a small cost model calibrated on MI355X sweeps (tools/gemm_bench.py): a CU's matrix pipe is
// shared by its resident workgroups, so a launch lasts ~ ceil(tiles / 256 CUs) x (tile area / efficiency of the config).
// When even the 64x64 tiling leaves most CUs idle (tall-K convs on small maps, half-scale Swin GEMMs at batch 1) the K
// loop is split so that ~512 workgroups exist.  W is padded to 128 rows so every config may over-read it.
GemmPlan plan_gemm(int M, int N, int K, int planes) {
    struct Cand { int cfg, bm, bn; double eff; };
    static const Cand cands[] = {{0, 128, 128, 1.00}, {1, 128, 64, 0.98}, {2, 64, 64, 0.93}, {5, 128, 128, 1.04}, {4, 256, 128, 1.06}};
    GemmPlan pl{2, 1, 0};
    double best = 1e300;
    for (const Cand& c : cands) {
        const long tiles = (long)((M + c.bm - 1) / c.bm) * ((N + c.bn - 1) / c.bn);
        if ((c.cfg == 5 || c.cfg == 4) && tiles < 1024) continue;      // the 8-wave tiles only pay on large grids
        const double cost = (double)((tiles + 255) / 256) * c.bm * c.bn / c.eff;
        if (cost < best) { best = cost; pl.cfg = c.cfg; }
    }
    const long t64 = (long)((M + 63) / 64) * ((N + 63) / 64);
    const int nk = K / BK;
    if (planes > 0 && N >= 128) {
        // split-bf16 modes: the warp-specialised 128x128 kernel beats the 4-wave tiles by 1.3-1.5x whenever its tiles are
        // mostly full (measured, tools/gemm_sk_sweep.py), two workgroups per CU = 512 slots; under ~200 tiles the K loop is
        // cut so that ~480 workgroups exist, but never below 24 K tiles per slice (the reduce pass costs more than it buys)
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
        const double waste = (double)t128 * 128.0 * 128.0 / ((double)M * N);
        if (waste <= 1.35) {          // N = 192 (1.33) still wins on the warp-specialised kernel: 214 vs 183 TF/s-eq at 81920 x 192 x 768
            pl.cfg = 0; pl.splitk = 1; pl.ws_floats = 0;
            static const int sk_t128 = getenv("BRN_SK_T128") ? atoi(getenv("BRN_SK_T128")) : 200;
            if (t128 < sk_t128) {
                int s = (int)(480 / t128);
                if (s > nk / 24) s = nk / 24;
                if (s > 8) s = 8;
                if (s > 1) { pl.splitk = s; pl.ws_floats = (size_t)s * M * N; }
            }
            return pl;
        }
    }
    if (t64 < 384 && nk >= 8) {
        pl.cfg = 2;
        int s = (int)((768 + t64 - 1) / t64);
        if (s > nk / 4) s = nk / 4;
        if (s > 64) s = 64;
        if (s > 1) { pl.splitk = s; pl.ws_floats = (size_t)s * M * N; }
    }
    return pl;
}

// The plan of a two-plane split-mode dense GEMM whose consumer is a LayerNorm that sums the slices itself (LayerNormParams::part): no reduce
// pass, so a cut costs only the extra slice traffic (S x M x N floats written and read back, L2-resident at the model's sizes).  Where
// plan_gemm already cuts, its slices are kept.  Beyond that, a launch of one round with one workgroup per CU (129 .. 256 tiles) is cut in
// two, so that two workgroups share every CU like in the full-grid launches, with at least LN_SK_MIN_KT K tiles per slice.  Three planes keep
// plan_gemm's launches: their 32-deep stage is one workgroup per CU whatever the grid, and without the reduce passes alone f32_split3 did not
// separate from its own run-to-run spread.  Measurements: DESIGN.md 3.1b.
constexpr int LN_SK_MIN_KT = 48;
GemmPlan plan_gemm_ln(int M, int N, int K, int planes) {
    GemmPlan pl = plan_gemm(M, N, K, planes);
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    const double waste = (double)t128 * 128.0 * 128.0 / ((double)M * N);
    if (planes != 2 || N < 128 || (N & 3) || waste > 1.35) { pl.splitk = 1; pl.ws_floats = 0; return pl; }    // (not the two-plane warp-specialised kernel's shapes)
    if (pl.splitk == 1 && t128 > 128 && t128 <= 256 && K / BK / 2 >= LN_SK_MIN_KT) { pl.splitk = 2; pl.ws_floats = (size_t)2 * M * N; }
    pl.raw = pl.splitk > 1;
    return pl;
}

// A deformable conv whose weights carry planes runs on the split kernels too (gemm_split.hip, DeformLoader): fp32 maps in and out, whole
// K tiles inside a tap, and the batch of sampled maps within the loader's 32-bit byte offsets.  Everything else — mode f32, the 16-bit modes'
// fallback shapes, the diag build's one-plane mode — keeps gemm_f32_kernel.
static bool deform_on_split(const GemmParams& p) {
    return p.mode == GEMM_DEFORM_NHWC && p.planes >= 2 && p.Wp && p.om && !p.a_bf16 && !p.c_bf16 && (p.Cin % 32) == 0 && p.K == p.kh * p.kw * p.Cin &&
           ((p.lda | p.a_coff) & 3) == 0 && p.Hin + p.pad < 32768 && p.Win + p.pad < 32768 &&       // (a row's window origin is kept as two 16-bit halves)
           ((double)p.M / ((double)p.Hout * p.Wout) + 1.0) * p.Hin * p.Win * p.lda * 4.0 < 2147483648.0;
}
// How it is launched: as the plain conv of the same mode and shape would be — plan_gemm with the planes: the same tile class (the warp-specialised
// 128 x 128 kernel, or a 4-wave tile: 64 x 64 here, same MFMA and K order as 128 x 64) and the same split-K, so every output element is summed in
// the order the mode's convs sum it (with zero offsets the two are bit-identical), on a plan tuned for these kernels.  The caller planned for
// gemm_f32_kernel and sized the scratch for that plan's slices: never more slices than those (the partial layout does not depend on the tile).
static int deform_split_plan(const GemmParams& p, int caller_slices, int& splitk) {
    const GemmPlan pp = plan_gemm(p.M, p.N, p.K, p.planes);
    splitk = pp.splitk < caller_slices ? pp.splitk : caller_slices;
    if (splitk < 1) splitk = 1;
    return gemm_split_is_ws(pp.cfg) ? 0 : 2;
}

hipError_t launch_gemm(const GemmParams& p_in, const GemmPlan& pl, float* ws, hipStream_t s) {
    if (p_in.M <= 0 || p_in.N <= 0 || p_in.K <= 0 || (p_in.K % BK) != 0) return hipErrorInvalidValue;
    if ((p_in.mode == GEMM_CONV_NHWC || p_in.mode == GEMM_DEFORM_NHWC) && (p_in.Cin % BK) != 0) return hipErrorInvalidValue;
    GemmParams p = p_in;
    p.splitk = pl.splitk < 1 ? 1 : pl.splitk;
    p.part = ws;
    if (p.splitk > 1 && !ws) return hipErrorInvalidValue;
    if (p.a_bf16 && p.mode != GEMM_DEFORM_NHWC) return hipErrorInvalidValue;       // only the deformable loader reads bf16 maps here
    if (p.c_bf16 && (p.splitk > 1 || p.R || (p.planes > 0 && p.Wp && p.mode != GEMM_DEFORM_NHWC && p.mode != GEMM_GATHER_NCHW))) return hipErrorInvalidValue;
    const bool deform_split = deform_on_split(p);
    int deform_cfg = 0;
    if (deform_split) deform_cfg = deform_split_plan(p, p.splitk, p.splitk);
    if (p.h2 && !(p.planes == 2 && p.Wp && (p.mode == GEMM_DENSE || p.mode == GEMM_CONV_NHWC || deform_split))) p.h2 = 0;     // (the fp32-MFMA kernel reads W itself: nothing is scaled)
    if (p.h2 && !(p.a_scale > 0.f && p.out_scale > 0.f)) return hipErrorInvalidValue;
    if (pl.raw && (p.splitk < 2 || p.c_planes || p.c_bf16)) return hipErrorInvalidValue;   // raw slices: fp32 partial sums of a real split only
    if (p.a_planes || p.c_planes) {         // P2 layouts: 2-plane split mode, dense, on the warp-specialised kernel only
        if (!(p.planes == 2 || p.planes == 3) || !p.Wp || p.mode != GEMM_DENSE || !gemm_split_is_ws(pl.cfg)) return hipErrorInvalidValue;
        if (p.a_planes && (p.a_planes != p.planes || p.lda % 16 || p.a_coff)) return hipErrorInvalidValue;
        if (p.c_planes && (p.c_planes != p.planes || p.splitk > 1 || p.R || p.N % 32 || p.ldc % 16 || p.c_coff % 32)) return hipErrorInvalidValue;
    }
    hipError_t e;
    if (p.planes > 0 && p.Wp && (p.mode == GEMM_DENSE || p.mode == GEMM_CONV_NHWC)) e = launch_gemm_split(p, pl.cfg, s);   // split-bf16 path: tile choice by the same plan
    else if (deform_split) e = launch_gemm_split(p, deform_cfg, s);
    else if (pl.cfg == 0) e = launch_cfg<128, 128, 2, 2>(p, s);
    else if (pl.cfg == 1) e = launch_cfg<128, 64, 2, 2>(p, s);
    else if (pl.cfg == 3) e = launch_cfg<128, 128, 2, 4>(p, s);
    else if (pl.cfg == 4) e = launch_cfg<256, 128, 4, 2>(p, s);
    else if (pl.cfg == 5) e = launch_cfg<128, 128, 4, 2>(p, s);
    else e = launch_cfg<64, 64, 2, 2>(p, s);
    if (e != hipSuccess || p.splitk == 1 || pl.raw) return e;      // raw: the slices stay in ws for the LayerNorm that sums them
    long total = (long)p.M * p.N;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace brn
