// gemm_split.hip — the contraction of gemm_f32.hip on the bf16 / fp16 matrix cores with fp32-class accuracy (compute modes f32_split3,
// f32_split2, f32_half2; one plane = mode bf16_operands, diag build only): gemm_split_kernel (4-wave 64x64 / 128x64 tiles) and the
// warp-specialised gemm_split_ws_kernel (128x128), and their launcher.  What the kernels are made of — plane products, operand staging, the
// deformable loader, the warp-specialised kernel's layout and roles — is gemm_split_stages.h.  launch_gemm (gemm_f32.hip) validates, plans
// split-K and calls launch_gemm_split; split-K partial sums are reduced by gemm_f32.hip's splitk_reduce_kernel.
#include "../brn_kernels.h"
#include "gemm_common.h"
#include "gemm_split_stages.h"
#include "gemm_conv_halo.h"

namespace brn {

// =====================================================================================================================
// gemm_split_kernel — the same contraction on the bf16 matrix cores with fp32-class accuracy.
// Every fp32 operand x is split error-free into NP bf16 planes (x = x_h + x_m + x_l up to 2^-25 |x|: each plane is the
// round-to-nearest bf16 of what the previous planes left over), the product is the sum of the plane products whose
// magnitude is >= 2^-24 of the full product (NP = 3: hh, hm, mh, hl, lh, mm — 6 x v_mfma_f32_32x32x16_bf16), each exact in
// the MFMA's fp32 accumulator.  6 bf16 MFMAs replace 8 fp32 MFMAs (k = 16 vs 2) at 16x the per-instruction rate: 2.67x the
// fp32-MFMA peak.  A is split while it is staged (fp32 in HBM, no second copy); W is pre-split at load time ([NP][Npad][K]).
// NP = 2 keeps hh, hm, mh (~2^-16 relative); NP = 1 is plain bf16 x bf16 -> fp32 (the bf16 throughput mode).
// LDS: per plane [rows][40 bf16] (80-byte rows: conflict-free for the ds_read_b128 lane groups).
// =====================================================================================================================
constexpr int SPLIT_LD = 40;   // bf16 elements per LDS row of gemm_split_kernel

template <int BM, int BN, int WM, int WN, int MODE, int NP, bool H = false>   // H: the two planes are fp16 (mode f32_half2)
__global__ void __launch_bounds__(WM* WN * 64) gemm_split_kernel(const GemmParams p) {
    static_assert(!H || NP == 2, "fp16 planes come in pairs");
    constexpr int SLD = SPLIT_LD;
    constexpr int NT = WM * WN * 64;
    constexpr int RPP = NT / 8;           // A rows per pass (8 float4 per 32-float row)
    constexpr int PA = BM / RPP;
    constexpr int WRPP = NT / 4;          // W rows per pass (4 x 16-byte chunks per 32-bf16 row)
    constexpr int PB = BN / WRPP;
    constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 32, TN = WTN / 32;
    static_assert(PA >= 1 && PB >= 1 && TM >= 1 && TN >= 1, "tile too small for the thread count");

    constexpr int SMEM_MAIN = NP * (BM + BN) * SLD * 2, SMEM_EPI = WM * WN * EPI_WAVE_FLOATS * 4;   // bytes
    __shared__ __attribute__((aligned(16))) char smem_raw[SMEM_MAIN > SMEM_EPI ? SMEM_MAIN : SMEM_EPI];
    __bf16* smem = reinterpret_cast<__bf16*>(smem_raw);
    __bf16* As = smem;                       // [NP][BM][SLD]
    __bf16* Bs = smem + NP * BM * SLD;       // [NP][BN][SLD]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const TileSlice ts = tile_slice<BM, BN>(p, BK);
    const int slice = ts.slice, m0 = ts.m0, n0 = ts.n0, kt0 = ts.kt0, nk = ts.nk;

    const int kq = tid & 7, lrow = tid >> 3;
    long a_base[PA];
    int a_iy[PA], a_ix[PA];
    bool a_ok[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) gather_row_init<MODE>(p, m0 + lrow + i * RPP, a_ok[i], a_base[i], a_iy[i], a_ix[i]);
    const int wc = tid & 3, wrow = tid >> 2;
    // W planes are interleaved per 32-deep K tile: [row][K/32][plane][32] bf16, so the NP x 64 bytes a (row, K tile) needs
    // are contiguous (NP = 2: exactly one 128-byte line; separate planes fetched every line twice: measured 2x L2->L1 traffic)
    const long wrow_stride = (long)p.K * NP;
    const __bf16* wsrc = reinterpret_cast<const __bf16*>(p.Wp) + (long)(n0 + wrow) * wrow_stride + wc * 8;

    // two staging register sets: tile kt+2 is already in flight while tile kt is multiplied (bytes in flight per CU, not
    // bandwidth, bound this kernel: a bf16-rate K tile lasts a few hundred cycles, an L2/HBM round trip ~1-2 thousand)
    f32x4 ra[2][PA];
    bf16x8 rb[2][NP][PB];
    unsigned am[2][PA];
    // The deformable loader (DeformLoader above): a staged row is its four corner float4s, blended at the LDS store.  Two sets of those
    // would cost the workgroups per CU that hide this kernel's latencies, so there is one (rc, for K tile rk), loaded one tile ahead.
    constexpr bool DEFORM = MODE == GEMM_DEFORM_NHWC;
    f32x4 rc[DEFORM ? PA : 1][4];
    int rk = 0;
    DeformLoader<PA, 8> dl;
    if constexpr (DEFORM) dl.init(p, m0, lrow, RPP, kq, lane);

    auto gload = [&](int kt, f32x4 (&qa)[PA], bf16x8 (&qb)[NP][PB], unsigned (&qm)[PA]) {
        const int k0 = kt * BK;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int i = 0; i < PB; ++i)
                qb[pl][i] = *reinterpret_cast<const bf16x8*>(wsrc + (long)i * WRPP * wrow_stride + (long)kt * (NP * 32) + pl * 32);
        if constexpr (DEFORM) {
            rk = k0;
            dl.template issue<0, PA>(p, k0, rc);
        } else {
            gather_rows_load<MODE>(&p, k0, kq, a_ok, a_base, a_iy, a_ix, qa, qm);
        }
    };
    auto lds_store = [&](const f32x4 (&qa)[PA], const bf16x8 (&qb)[NP][PB], const unsigned (&qm)[PA]) {
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            auto at = [&](int pl) { return As + (pl * BM + lrow + i * RPP) * SLD + kq * 4; };
            if constexpr (DEFORM) stage_a_row<NP, H>(dl.finish(p, rk, i, rc[i]), 0xffffffffu, false, p.a_scale, at);
            else stage_a_row<NP, H>(qa[i], qm[i], true, p.a_scale, at);
        }
        stage_w_planes<NP, PB>(qb, [&](int pl, int i) { return Bs + (pl * BN + wrow + i * WRPP) * SLD + wc * 8; });
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // MFMA 32x32x16 bf16 operand map: lane l holds row (l & 31), k = 8 * (l >> 5) + j, j = 0..7
    const __bf16* a_frag = As + (wm * WTM + (lane & 31)) * SLD + (lane >> 5) * 8;
    const __bf16* b_frag = Bs + (wn * WTN + (lane & 31)) * SLD + (lane >> 5) * 8;

    auto compute = [&]() {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[NP][TM], bf[NP][TN];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[pl][i] = *reinterpret_cast<const bf16x8*>(a_frag + (pl * BM + i * 32) * SLD + ks * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[pl][j] = *reinterpret_cast<const bf16x8*>(b_frag + (pl * BN + j * 32) * SLD + ks * 16);
            }
            plane_products<NP, H, false>(af, bf, acc);
        }
    };

    if constexpr (DEFORM) {
        if (kt0 < nk) {
            gload(kt0, ra[0], rb[0], am[0]);
            lds_store(ra[0], rb[0], am[0]);
        }
        __syncthreads();
        for (int kt = kt0; kt < nk; ++kt) {
            if (kt + 1 < nk) gload(kt + 1, ra[0], rb[0], am[0]);
            compute();
            __syncthreads();
            if (kt + 1 < nk) {
                lds_store(ra[0], rb[0], am[0]);
                __syncthreads();
            }
        }
    } else {
    if (kt0 < nk) {
        gload(kt0, ra[0], rb[0], am[0]);
        if (kt0 + 1 < nk) gload(kt0 + 1, ra[1], rb[1], am[1]);
        lds_store(ra[0], rb[0], am[0]);
    }
    __syncthreads();
    // body for one K tile whose successor sits in register set NXT; the set just consumed (CUR) is refilled 2 tiles ahead.  (A macro: CUR and
    // NXT have to be compile-time indices, and a generic lambda taking them as integral_constants compiled to other code with other register
    // counts, profiles/isa_parity_gemm_split.md.)
#define BRN_SPLIT_STEP(KT, CUR, NXT)                                  \
    {                                                                 \
        if ((KT) + 2 < nk) gload((KT) + 2, ra[CUR], rb[CUR], am[CUR]);         \
        compute();                                                    \
        __syncthreads();                                              \
        if ((KT) + 1 < nk) {                                          \
            lds_store(ra[NXT], rb[NXT], am[NXT]);            \
            __syncthreads();                                          \
        }                                                             \
    }
    for (int kt = kt0; kt < nk; kt += 2) {
        BRN_SPLIT_STEP(kt, 0, 1)
        if (kt + 1 < nk) BRN_SPLIT_STEP(kt + 1, 1, 0)
    }
#undef BRN_SPLIT_STEP
    }
    gemm_epilogue<TM, TN, WTM, WTN>(p, acc, m0, n0, wm, wn, lane, slice, reinterpret_cast<float*>(smem_raw) + wave * EPI_WAVE_FLOATS);
}

// ---------------------------------------------------------------------------------------------------------------------
// gemm_split_ws_kernel — warp-specialised form of gemm_split_kernel for the 128x128 tile: 8 waves, two per SIMD.  LDS layout and the
// producers' thread map: WsLayout (gemm_split_stages.h).  Top to bottom: the tile slice; the producers (waves 4-7), register-staged or
// deformable; the consumers (waves 0-3), 16x16x32 or 32x32x16 MFMAs; one barrier; the epilogue on all eight waves.
// Producers stage: global loads into two register sets, three K tiles ahead of the consumers, operand split, LDS writes into the ring of two
// K-tile buffers, one tile ahead.  Consumers own the 2x2 grid of 64x64 sub-tiles: fragment reads + MFMA only.  ONE workgroup barrier per
// K tile.  Tile t + 1 is complete only after step t's barrier, so a consumer reads its first fragments right after it and double-buffers
// fragments in registers: at bf16 MFMA rates an exposed LDS read (~250 cycles) per 32-deep K tile (768 MFMA cycles) was a third of the
// loop (measured by ablation: staging and MFMA phases added up, then the fragment-read stall did).
//   APL:  A arrives in the P layout (its producer already split it): the staging waves only copy
//   H:    the two planes are fp16 planes of the scaled operands (mode f32_half2; split4h / the f16 MFMAs), same bytes and layouts
//   DIAG: ablation switches (p.abl) + per-K-tile cycle stamps (WsTrace; brn_gemm_microbench only; costs registers)
//   KS:   k elements per LDS stage (32, or 16 to halve the stage when 3 planes must fit twice per CU)
// (the deformable producers hold four corners per staged row: the 2-plane form is told to stay within the 128 VGPRs of two workgroups per CU)
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE, int NP, int KS, bool DIAG, bool APL, bool H = false>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(MODE == GEMM_DEFORM_NHWC && NP == 2 ? 4 : 1)))
gemm_split_ws_kernel(const GemmParams p) {
    using L = WsLayout<NP, KS, APL>;
    constexpr int BM = L::BM, BN = L::BN, WTM = L::WTM, WTN = L::WTN, TM = 2, TN = 2;
    static_assert(!APL || ((NP == 2 || NP == 3) && MODE == GEMM_DENSE), "the P input layout is the NP-plane split of a dense A");
    static_assert(!H || NP == 2, "fp16 planes come in pairs");
    static_assert(L::NBUF == 2, "the producers stage one tile ahead of the consumers; a tile's first fragments are read after the step's barrier");
    constexpr int SLD = L::ROW, KSTEPS = L::KSTEPS, NBUF = L::NBUF, AQ = L::AQ, RPP = L::RPP, PA = L::PA, WQ = L::WQ, WRPP = L::WRPP, PB = L::PB;
    constexpr int APAD = L::APAD, AREG = L::AREG, BUF = L::BUF, EP_LD = L::EP_LD;
    __shared__ __attribute__((aligned(16))) char smem_raw[L::SMEM];
    __bf16* smem = reinterpret_cast<__bf16*>(smem_raw);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int abl = DIAG ? p.abl : 0;
    const bool producer = wave >= 4;
    const TileSlice ts = tile_slice<BM, BN>(p, KS);
    const int slice = ts.slice, m0 = ts.m0, n0 = ts.n0, kt0 = ts.kt0, nk = ts.nk;
    const int nt = nk > kt0 ? nk - kt0 : 0;         // K tiles of this slice; local tile index t = kt - kt0

    const WsTrace<DIAG> tr(p);
    tr.start(tid);
    f32x16 acc[TM][TN];
    if (producer) {
        const int pt = tid - 256;
        const int kq = pt % AQ, lrow = pt / AQ;
        long a_base[PA];        // (a_base, a_iy, a_ix, a_ok: the implicit-GEMM form only; dense rows are bounded by their buffer resource)
        int a_iy[PA], a_ix[PA];
        bool a_ok[PA];
        int p_lds[PA];          // P-layout input: LDS element offset of this thread's i-th chunk (plane, row, 8-element column)
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            p_lds[i] = 0;
            if (APL) {
                const int q = i * 256 + pt, row = q / (4 * NP), c = q - row * (4 * NP);   // chunk c of the row: plane c / 4, k = 8 (c % 4)
                p_lds[i] = ((c >> 2) * BM + row) * SLD + (c >> 2) * APAD + ((c & 3) ^ L::swz_key(row)) * 8;
            }
            gather_row_init<MODE>(p, m0 + lrow + i * RPP, a_ok[i], a_base[i], a_iy[i], a_ix[i]);
        }
        const int wc = pt % WQ, wrow = pt / WQ;
        // element offsets inside an LDS row of this thread's pieces (RPP and WRPP are multiples of 32 rows: the key is that of lrow / wrow)
        const int a_sw = ((kq >> 1) ^ L::swz_key(lrow)) * 8 + (kq & 1) * 4;
        const int w_sw = (wc ^ L::swz_key(wrow)) * 8;
        const long wrow_stride = (long)p.K * NP;         // W planes interleaved per K tile: [row][K/32][plane][32] bf16
        // Dense operands are buffer-addressed: a resource per tile (A: based at row m0, num_records = the tile's valid rows, so rows
        // >= M come back as zeros without a mask; W planes: based at row n0), a 32-bit lane offset fixed for the tile, the K tile in the
        // instruction's SGPR offset.  The producers share their SIMDs with the MFMA waves: the 64-bit per-lane address arithmetic and
        // the row mask were ~5 VALU per load, a quarter of the producers' vector work per K tile.
        // The implicit-GEMM form: the resource is based at the first image of the tile, a lane's pixel offset is fixed for the tile, the
        // K tile's (tap, channel) offset is uniform (Cin % KS == 0: a K tile lies inside one tap) and is added to it; a tap outside the
        // image gets an offset past num_records, which the buffer unit answers with zeros.  The P-layout form (APL) is the dense one
        // with 16 NP floats per K tile.
        constexpr bool BUFA = MODE == GEMM_DENSE;                       // dense (plain or P-layout rows): valid-row num_records, no mask
        constexpr bool BUFC = MODE == GEMM_CONV_NHWC;
        const int conv_b0 = BUFC ? min(m0, p.M - 1) / (p.Hout * p.Wout) : 0;
        // (32-bit byte offsets span the two images a tile can touch: larger maps keep the general 64-bit addresses below)
        const bool bufc_ok = BUFC && (double)p.Hin * p.Win * p.lda * 8.0 < 2147483648.0;
        __amdgpu_buffer_rsrc_t rsrc_a = BUFC
            ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A + (long)conv_b0 * p.Hin * p.Win * p.lda + p.a_coff), 0, 0x7fffffff, 0x00020000)
            : __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A + (long)m0 * p.lda), 0, (int)min((long)(p.M - m0) * p.lda * 4, 0x7fffffffL), 0x00020000);
        int conv_pix[PA];
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            conv_pix[i] = 0;
            if (BUFC) {
                const int m = m0 + lrow + i * RPP, hw = p.Hout * p.Wout;
                const int bq = a_ok[i] ? m / hw - conv_b0 : 0;
                conv_pix[i] = (((bq * p.Hin + a_iy[i]) * p.Win + a_ix[i]) * p.lda + kq * 4) * 4;   // bytes; negative inside the padding
            }
        }
        __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(reinterpret_cast<const __bf16*>(p.Wp) + (long)n0 * wrow_stride), 0,
                                                                          0x7fffffff, 0x00020000);
        unsigned voff_a[PA], voff_w[PB];
#pragma unroll
        for (int i = 0; i < PA; ++i) {
            if (APL) { const int q = i * 256 + pt, row = q / (4 * NP), c = q - row * (4 * NP); voff_a[i] = (unsigned)((row * p.lda + c * 4) * 4); }
            else voff_a[i] = (unsigned)(((lrow + i * RPP) * p.lda + kq * 4) * 4);
        }
#pragma unroll
        for (int i = 0; i < PB; ++i) voff_w[i] = (unsigned)(((long)(wrow + i * WRPP) * wrow_stride + wc * 8) * 2);
        f32x4 ra[2][PA];
        bf16x8 rb[2][NP][PB];
        unsigned am[2][PA];
        // the NP W planes of K tile kt (a 16-deep stage takes one half of the 32-deep tile's 64 bytes per plane)
        auto wload = [&](int kt, bf16x8 (&qb)[NP][PB]) {
            const int wk = (KS == 32 ? kt * (NP * 32) : (kt >> 1) * (NP * 32) + (kt & 1) * 16) * 2;   // bytes, uniform
#pragma unroll
            for (int pl = 0; pl < NP; ++pl)
#pragma unroll
                for (int i = 0; i < PB; ++i)
                    qb[pl][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, voff_w[i], wk + pl * 64, 0));
        };
        auto gload = [&](int t, f32x4 (&qa)[PA], bf16x8 (&qb)[NP][PB], unsigned (&qm)[PA]) {
            const int k0 = (kt0 + t) * KS;
            wload(kt0 + t, qb);
            if (BUFA) {
#pragma unroll
                for (int i = 0; i < PA; ++i) {
                    qa[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, voff_a[i], APL ? (kt0 + t) * (64 * NP) : k0 * 4, 0));
                    qm[i] = 0xffffffffu;
                }
                return;
            }
            const ConvTap tp = conv_tap(p, k0);
            const int dy = tp.ky * p.dil, dx = tp.kx * p.dil;
            if (bufc_ok) {
                const int tap_off = ((dy * p.Win + dx) * p.lda + tp.ci0) * 4;        // uniform
#pragma unroll
                for (int i = 0; i < PA; ++i) {
                    const int iy = a_iy[i] + dy, ix = a_ix[i] + dx;
                    const bool ok = a_ok[i] && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
                    qa[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, ok ? (unsigned)(conv_pix[i] + tap_off) : 0x80000000u, 0, 0));
                    qm[i] = 0xffffffffu;
                }
                return;
            }
            // maps too large for 32-bit offsets: 64-bit addresses, clamped + masked, as gather_rows_load does it (written out here: that helper
            // inside this lambda changes the code of the buffer-addressed paths as well, profiles/isa_parity_gemm_split.md)
#pragma unroll
            for (int i = 0; i < PA; ++i) {
                const int iy = a_iy[i] + dy, ix = a_ix[i] + dx;
                const bool ok = a_ok[i] && (unsigned)iy < (unsigned)p.Hin && (unsigned)ix < (unsigned)p.Win;
                const long off = ok ? a_base[i] + ((long)iy * p.Win + ix) * p.lda + tp.ci0 : (long)p.a_coff;
                qa[i] = load4_masked(p.A + off + kq * 4, ok, qm[i]);
            }
        };
        auto w_store = [&](int t, const bf16x8 (&qb)[NP][PB]) {
            __bf16* Bs = smem + (t % NBUF) * BUF + AREG;
            stage_w_planes<NP, PB>(qb, [&](int pl, int i) { return Bs + (pl * BN + wrow + i * WRPP) * SLD + w_sw; });
        };
        auto lds_store = [&](int t, const f32x4 (&qa)[PA], const bf16x8 (&qb)[NP][PB], const unsigned (&qm)[PA]) {
            __bf16* As = smem + (t % NBUF) * BUF;
            if (APL) {
                // 16 bytes = 8 bf16 of plane kq >> 2 at k = 8 (kq & 3): one ds_write_b128, no arithmetic (rows beyond M were
                // loaded from row 0 and are zeroed by an integer AND with the row's 0 / ~0 mask)
#pragma unroll
                for (int i = 0; i < PA; ++i) {
                    const u32x4 bits = __builtin_bit_cast(u32x4, qa[i]) & qm[i];
                    *reinterpret_cast<u32x4*>(As + p_lds[i]) = bits;
                }
            } else {
#pragma unroll
                for (int i = 0; i < PA; ++i)
                    stage_a_row<NP, H>(qa[i], qm[i], !(BUFA || (BUFC && bufc_ok)), p.a_scale, [&](int pl) { return As + (pl * BM + lrow + i * RPP) * SLD + a_sw; });
            }
            w_store(t, qb);
        };
        if constexpr (MODE == GEMM_DEFORM_NHWC) {
        // The deformable loader (DeformLoader above).  A staged row is four corner float4s: two register sets of those are more than the
        // 128 VGPRs of two workgroups per CU hold, so there is one, and a tile's rows go in two halves: blend, split and store half h of tile
        // u, then issue half h of tile u + 1.  The corner loads of the next tile are then in flight across the other half's split and LDS
        // stores, the barrier and the consumers' K tile.  W has one register set as well, loaded one tile ahead.
        static_assert(!APL && !DIAG && NBUF == 2 && PA % 2 == 0, "the deformable producer: plain A, the 2-deep ring, rows in two halves");
        constexpr int HR = PA / 2;
        DeformLoader<PA, AQ> dl;
        dl.init(p, m0, lrow, RPP, kq, lane);
        f32x4 rc[PA][4];
        auto a_store = [&](int t, int i, const f32x4 v) {
            __bf16* As = smem + (t % NBUF) * BUF;
            stage_a_row<NP, H>(v, 0xffffffffu, false, p.a_scale, [&](int pl) { return As + (pl * BM + lrow + i * RPP) * SLD + a_sw; });
            __builtin_amdgcn_sched_barrier(0);      // one row at a time: interleaved rows' temporaries do not fit beside the corners in flight
        };
        // prologue: LDS tile 0 stored, the corners and the W planes of tile 1 in flight
        if (nt > 0) { wload(kt0, rb[0]); dl.template issue<0, PA>(p, kt0 * KS, rc); }
        if (nt > 0) {
#pragma unroll
            for (int i = 0; i < PA; ++i) a_store(0, i, dl.finish(p, kt0 * KS, i, rc[i]));
            w_store(0, rb[0]);
        }
        if (nt > 1) { dl.template issue<0, PA>(p, (kt0 + 1) * KS, rc); wload(kt0 + 1, rb[0]); }
        __syncthreads();
        // step t (the consumers multiply tile t): stage tile u = t + 1
        for (int t = 0; t < nt; ++t) {
            const int u = t + 1;
            if (u < nt) {
                const int k0 = (kt0 + u) * KS;
#pragma unroll
                for (int i = 0; i < HR; ++i) a_store(u, i, dl.finish(p, k0, i, rc[i]));
                if (u + 1 < nt) dl.template issue<0, HR>(p, k0 + KS, rc);
#pragma unroll
                for (int i = HR; i < PA; ++i) a_store(u, i, dl.finish(p, k0, i, rc[i]));
                if (u + 1 < nt) dl.template issue<HR, PA>(p, k0 + KS, rc);
                w_store(u, rb[0]);
                if (u + 1 < nt) wload(kt0 + u + 1, rb[0]);
            }
            __syncthreads();
        }
        } else {
        // prologue: LDS tile 0 stored, the register sets hold tiles 1 and 2
        if (nt > 0) gload(0, ra[0], rb[0], am[0]);
        if (nt > 1) gload(1, ra[1], rb[1], am[1]);
        if (nt > 0 && !(abl & 2)) lds_store(0, ra[0], rb[0], am[0]);
        if (nt > 2) gload(2, ra[0], rb[0], am[0]);
        tr.cycles(tid == 256, 8 + 3);
        __syncthreads();
        // step T (the consumers multiply tile T): store tile T + 1 from register set SET, refill that set with tile T + 3.  (A macro, like
        // BRN_SPLIT_STEP above: SET has to be a compile-time index, and a generic lambda taking it as an integral_constant compiled to other
        // code with other register counts, profiles/isa_parity_gemm_split.md.)
#define BRN_PROD_STEP(T, SET)                                                                      \
        {                                                                                          \
            tr.cycles(tid == 256 && (T) < 24, 16 + (T) * 4 + 0);                                   \
            tr.drain_loads();                                                                      \
            tr.cycles(tid == 256 && (T) < 24, 16 + (T) * 4 + 3);                                   \
            if ((T) + 1 < nt) {                                                                \
                if (!(abl & 2)) lds_store((T) + 1, ra[SET], rb[SET], am[SET]);                 \
                tr.cycles(tid == 256 && (T) < 24, 16 + (T) * 4 + 1);                               \
                if ((T) + 3 < nt && !(abl & 1)) gload((T) + 3, ra[SET], rb[SET], am[SET]); \
            }                                                                                      \
            tr.cycles(tid == 256 && (T) < 24, 16 + (T) * 4 + 2);                                   \
            if (!(abl & 16)) __syncthreads();                                                      \
        }
        for (int t = 0; t < nt; t += 2) {
            BRN_PROD_STEP(t, 1)
            if (t + 1 < nt) BRN_PROD_STEP(t + 1, 0)
        }
#undef BRN_PROD_STEP
        }   // (the register-staged producers)
        tr.cycles(tid == 256, 8 + 4);
        tr.wall(tid == 256, 8 + 5);
    } else if constexpr (KS == 32 && NP == 2 && !DIAG) {
    // ---- consumers, 16 x 16 x 32 MFMAs: the same cycles per flop as 32 x 32 x 16, but the chip holds a higher clock under the smaller
    // shape (MI355X_MICROARCH.md, DVFS; gemm_bf16.hip measured + 5 ... 13 % on its LDS-fed tiles).  One MFMA k = the whole 32-deep stage; a wave's
    // 64 x 64 is 4 x 4 blocks, multiplied as four 2 x 2 quadrants.  Fragment of a 16-row block: lane l reads row l & 15, 16-byte k chunk l >> 4 (XOR the row's key).
    f32x4 acc4[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc4[i][j] = zero4();
    const int wm = wave >> 1, wn = wave & 1;
    const int r16 = lane & 15, kc = lane >> 4;
    const int fch = (kc ^ L::swz_key(r16)) * 8;           // (the key of a row depends on its bits 2, 3: the same in every 16-row block)
    const int a_row = (wm * WTM + r16) * SLD + fch, b_row = AREG + (wn * WTN + r16) * SLD + fch;
    auto read_a = [&](int t, int half, bf16x8 (&af)[NP][2]) {
        const __bf16* buf = smem + (t % NBUF) * BUF;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int i = 0; i < 2; ++i) af[pl][i] = *reinterpret_cast<const bf16x8*>(buf + a_row + (pl * BM + (half * 2 + i) * 16) * SLD + pl * APAD);
    };
    auto read_b = [&](int t, int half, bf16x8 (&bf)[NP][2]) {
        const __bf16* buf = smem + (t % NBUF) * BUF;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[pl][j] = *reinterpret_cast<const bf16x8*>(buf + b_row + (pl * BN + (half * 2 + j) * 16) * SLD);
    };
    // per stage: the first quadrant's fragments (A blocks 0, 1; W blocks 0, 1: 8 reads) are fetched right after the barrier, the other 8 reads ride
    // under the first quadrant's 12 MFMAs
    bf16x8 fa0[NP][2], fa1[NP][2], fb0[NP][2], fb1[NP][2];
    __syncthreads();   // prologue barrier: LDS tile 0 is complete
    if (nt > 0) { read_a(0, 0, fa0); read_b(0, 0, fb0); }
    for (int t = 0; t < nt; ++t) {
        read_a(t, 1, fa1);
        read_b(t, 1, fb1);
        plane_products<NP, H, true>(fa0, fb0, acc4, 0, 0);
        plane_products<NP, H, true>(fa1, fb0, acc4, 2, 0);
        plane_products<NP, H, true>(fa0, fb1, acc4, 0, 2);
        plane_products<NP, H, true>(fa1, fb1, acc4, 2, 2);
        __syncthreads();
        if (t + 1 < nt) { read_a(t + 1, 0, fa0); read_b(t + 1, 0, fb0); }
    }
    // the C tile image (see the 32 x 32 form below): row = the lane's row of the block, columns 4 (lane >> 4) .. + 3
    float* ctile = reinterpret_cast<float*>(smem_raw);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<f32x4*>(ctile + (wm * WTM + i * 16 + r16) * EP_LD + wn * WTN + j * 16 + 4 * kc) = acc4[i][j];
    } else {
    // ---- consumers ----
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int wm = wave >> 1, wn = wave & 1;
    // (the swizzle key of a fragment row depends on its low five bits only: every block offset below is a multiple of 32 rows)
    const int fkey = L::swz_key(lane & 31);
    const int a_row = (wm * WTM + (lane & 31)) * SLD, b_row = AREG + (wn * WTN + (lane & 31)) * SLD;
    int f_chunk[KSTEPS];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) f_chunk[ks] = (((lane >> 5) + 2 * ks) ^ fkey) * 8;
    auto read_frags = [&](int t, int ks, bf16x8 (&af)[NP][TM], bf16x8 (&bf)[NP][TN]) {
        const __bf16* buf = smem + (t % NBUF) * BUF;
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
            for (int i = 0; i < TM; ++i) af[pl][i] = *reinterpret_cast<const bf16x8*>(buf + a_row + (pl * BM + i * 32) * SLD + pl * APAD + f_chunk[ks]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[pl][j] = *reinterpret_cast<const bf16x8*>(buf + b_row + (pl * BN + j * 32) * SLD + f_chunk[ks]);
        }
    };
    bf16x8 fa0[NP][TM], fb0[NP][TN], fa1[NP][TM], fb1[NP][TN];
    __syncthreads();   // prologue barrier: LDS tile 0 is complete
    tr.cycles(tid == 0, 3);
    if (nt > 0 && !(abl & 4)) read_frags(0, 0, fa0, fb0);
    for (int t = 0; t < nt; ++t) {
        tr.cycles(tid == 0 && t < 24, 128 + t * 4 + 0);
        if (!(abl & 4)) {
            if (KSTEPS == 2) {
                read_frags(t, 1, fa1, fb1);
                plane_products<NP, H, true>(fa0, fb0, acc);
                plane_products<NP, H, true>(fa1, fb1, acc);
            } else {
                plane_products<NP, H, true>(fa0, fb0, acc);
            }
        }
        tr.cycles(tid == 0 && t < 24, 128 + t * 4 + 1);
        if (!(abl & 16)) __syncthreads();
        if (t + 1 < nt && !(abl & 4)) read_frags(t + 1, 0, fa0, fb0);
    }
    tr.cycles(tid == 0, 4);
    // the staging LDS is dead (every fragment read retired at the last barrier): the consumers lay their accumulators down as a
    // row-major image of the C tile
    float* ctile = reinterpret_cast<float*>(smem_raw);
    {
        // the product was formed transposed (W fragment = the MFMA's first operand): a lane holds ONE row (lane & 31) of a 32 x 32 block and
        // columns 8g + 4h + {0..3} in registers 4g .. 4g+3 (h = lane >> 5) — 16 ds_write_b128 per lane instead of 64 ds_write_b32
        // (rows are 528 bytes apart: 8 consecutive lanes hit 8 x 4 different banks)
        const int row = lane & 31, h4 = (lane >> 5) * 4;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                    *reinterpret_cast<f32x4*>(ctile + (wm * WTM + i * 32 + row) * EP_LD + wn * WTN + j * 32 + 8 * g + h4) = v;
                }
    }
    }   // consumers
    // ---- epilogue, all eight waves: the producers have nothing left to do, and a 4-wave epilogue was 5-11 us of store-issue
    // latency per tile.  Each pass moves 16 rows x 512 B: one wave = two full rows, float4 per lane ----
    __syncthreads();
    gemm_epilogue_tile<BM, BN, EP_LD>(p, reinterpret_cast<const float*>(smem_raw), m0, n0, tid, slice);
    tr.cycles(tid == 0, 5);
    tr.wall(tid == 0, 6);
}

// ---- launcher ----
// The warp-specialised kernel for NP planes (H: the fp16 pair) and KS-deep stages, by A mode and A layout.
template <int NP, int KS, bool H>
static hipError_t launch_split_ws_ks(const GemmParams& p, dim3 grid, hipStream_t s) {
    const dim3 block(512);
    if (p.a_planes) {
        if constexpr (NP == 2 && KS == 32) {   // (the 3-plane form works too, but was 2 % slower per forward: rows 1.5x as long)
            if (p.mode != GEMM_DENSE || p.a_planes != NP) return hipErrorInvalidValue;
#ifdef BRN_DIAG_BUILD
            if constexpr (!H)
                if (p.abl || p.trace) { hipLaunchKernelGGL((gemm_split_ws_kernel<GEMM_DENSE, 2, 32, true, true>), grid, block, 0, s, p); return hipGetLastError(); }
#endif
            hipLaunchKernelGGL((gemm_split_ws_kernel<GEMM_DENSE, 2, 32, false, true, H>), grid, block, 0, s, p);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
#ifdef BRN_DIAG_BUILD
    if constexpr (!H)
        if (p.mode == GEMM_DENSE && KS == 32 && (p.abl || p.trace)) { hipLaunchKernelGGL((gemm_split_ws_kernel<GEMM_DENSE, NP, 32, true, false>), grid, block, 0, s, p); return hipGetLastError(); }
#endif
    if (p.mode == GEMM_DENSE) hipLaunchKernelGGL((gemm_split_ws_kernel<GEMM_DENSE, NP, KS, false, false, H>), grid, block, 0, s, p);
    else if (p.mode == GEMM_CONV_NHWC) hipLaunchKernelGGL((gemm_split_ws_kernel<GEMM_CONV_NHWC, NP, KS, false, false, H>), grid, block, 0, s, p);
    else if (p.mode == GEMM_DEFORM_NHWC) {
        if constexpr (NP >= 2 && KS == 32) hipLaunchKernelGGL((gemm_split_ws_kernel<GEMM_DEFORM_NHWC, NP, 32, false, false, H>), grid, block, 0, s, p);
        else return hipErrorInvalidValue;
    }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
template <int NP>
static hipError_t launch_split_ws(const GemmParams& p, hipStream_t s) {
    const int tiles = ((p.M + 127) / 128) * ((p.N + 127) / 128) * p.splitk;
    const dim3 grid(tiles);
    if (p.h2) {                           // mode f32_half2: two fp16 planes, 32-deep stages
        if constexpr (NP == 2) return launch_split_ws_ks<2, 32, true>(p, grid, s);
        else return hipErrorInvalidValue;
    }
    // 3 planes: 32-deep stages need 120 KB of LDS (one workgroup per CU); 16-deep stages (2 x 36 KB) let two share a CU like the
    // 2-plane kernel's do, at twice the barriers per K: worth it as soon as there is more than one workgroup per CU to place
    // (the deformable loader is built for 32-deep stages only)
    if constexpr (NP == 3)
        if (tiles > 256 && !(p.abl || p.trace) && p.mode != GEMM_DEFORM_NHWC) return launch_split_ws_ks<3, 16, false>(p, grid, s);
    return launch_split_ws_ks<NP, 32, false>(p, grid, s);
}

template <int BM, int BN, int WM, int WN, int NP, bool H>
static hipError_t launch_split_cfg(const GemmParams& p, hipStream_t s) {
    const int tiles = ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN) * p.splitk;
    dim3 grid(tiles), block(WM * WN * 64);
    if (p.mode == GEMM_DENSE) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, WM, WN, GEMM_DENSE, NP, H>), grid, block, 0, s, p);
    else if (p.mode == GEMM_CONV_NHWC) hipLaunchKernelGGL((gemm_split_kernel<BM, BN, WM, WN, GEMM_CONV_NHWC, NP, H>), grid, block, 0, s, p);
    else if (p.mode == GEMM_DEFORM_NHWC) {
        if constexpr (NP >= 2 && BM == 64 && BN == 64) hipLaunchKernelGGL((gemm_split_kernel<64, 64, WM, WN, GEMM_DEFORM_NHWC, NP, H>), grid, block, 0, s, p);   // (launch_gemm's deformable tiles: this one and the warp-specialised kernel)
        else return hipErrorInvalidValue;
    }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
// the 4-wave tiles: 128x64 for cfg 1, 64x64 for every other plan that is not warp-specialised (as launch_gemm's fp32 ladder treats an unknown cfg)
template <int NP, bool H>
static hipError_t launch_split_tile(const GemmParams& p, int cfg, hipStream_t s) {
    if (cfg == 1) return launch_split_cfg<128, 64, 2, 2, NP, H>(p, s);
    return launch_split_cfg<64, 64, 2, 2, NP, H>(p, s);
}

template <int NP>
static hipError_t launch_split_np(const GemmParams& p, int cfg, hipStream_t s) {
    if (gemm_split_is_ws(cfg)) return launch_split_ws<NP>(p, s);
    if constexpr (NP == 2)      // a 4-wave plan of a 3x3 conv: the halo-staged kernel (gemm_conv_halo.h), whatever the plan's tile
        if (conv_halo_eligible(p)) return p.h2 ? launch_conv_halo<true>(p, s) : launch_conv_halo<false>(p, s);
    if (p.h2) {
        if constexpr (NP == 2) return launch_split_tile<2, true>(p, cfg, s);
        else return hipErrorInvalidValue;
    }
    return launch_split_tile<NP, false>(p, cfg, s);
}
hipError_t launch_gemm_split(const GemmParams& p, int cfg, hipStream_t s) {
    if (p.planes == 3) return launch_split_np<3>(p, cfg, s);
    if (p.planes == 2) return launch_split_np<2>(p, cfg, s);
#ifdef BRN_DIAG_BUILD                   // one bf16 plane (mode bf16_operands, superseded by the bf16-storage mode): diag build only
    return launch_split_np<1>(p, cfg, s);
#else
    return hipErrorInvalidValue;
#endif
}

}  // namespace brn
