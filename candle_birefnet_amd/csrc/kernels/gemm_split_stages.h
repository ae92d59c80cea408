// gemm_split_stages.h — what gemm_split.hip's two kernels are made of.  Shared by both: the plane products (plane_products), the operand
// staging (stage_a_row, stage_w_planes) and the deformable A loader (DeformLoader).  The warp-specialised kernel alone: its LDS layout and
// thread map (WsLayout) and its diag-build cycle stamps (WsTrace).
#pragma once
#include "../brn_kernels.h"
#include "gemm_common.h"

namespace brn {

// ---- plane products ----
// one MFMA over 8 k values per lane of two 16-bit planes (H: fp16, else bf16); its shape follows the accumulator: 32x32x16 or 16x16x32
template <bool H>
__device__ __forceinline__ void mfma_planes(const bf16x8 a, const bf16x8 b, f32x16& c) {
    if constexpr (H) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool H>
__device__ __forceinline__ void mfma_planes(const bf16x8 a, const bf16x8 b, f32x4& c) {
    if constexpr (H) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// acc[i0 + i][j0 + j] += the kept plane products (pa + pb < NP) of A fragments af[pa][i] and W fragments bf[pb][j], smallest plane products
// first.  WFIRST: the W fragment is the MFMA's first operand (the product is formed transposed: a lane then holds consecutive columns of one row).
template <int NP, bool H, bool WFIRST, int TM, int TN, typename ACC, int AM, int AN>
__device__ __forceinline__ void plane_products(const bf16x8 (&af)[NP][TM], const bf16x8 (&bf)[NP][TN], ACC (&acc)[AM][AN], const int i0 = 0, const int j0 = 0) {
#pragma unroll
    for (int sum = NP - 1; sum >= 0; --sum)
#pragma unroll
        for (int pa = 0; pa < NP; ++pa) {
            const int pb = sum - pa;
            if (pb < 0 || pb >= NP) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    if constexpr (WFIRST) mfma_planes<H>(bf[pb][j], af[pa][i], acc[i0 + i][j0 + j]);
                    else mfma_planes<H>(af[pa][i], bf[pb][j], acc[i0 + i][j0 + j]);
        }
}

// ---- operand staging ----
// Split four fp32 A values into their NP planes (H: the fp16 pair of a_scale x v) and store plane pl at at(pl): where is the caller's layout.
// masked: AND the values with `keep` first (load4_masked); else `keep` is not looked at.
template <int NP, bool H, typename AT>
__device__ __forceinline__ void stage_a_row(const f32x4 v, const unsigned keep, const bool masked, const float a_scale, AT at) {
    bf16x4 sp[NP];
    if constexpr (H) { if (!masked) split4h<false>(v, keep, a_scale, sp); else split4h<true>(v, keep, a_scale, sp); }
    else if (!masked) split4<NP, false>(v, keep, sp); else split4<NP>(v, keep, sp);
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) *reinterpret_cast<bf16x4*>(at(pl)) = sp[pl];
}
// store a thread's 16-byte chunks of the NP W planes: chunk i of plane pl at at(pl, i)
template <int NP, int PB, typename AT>
__device__ __forceinline__ void stage_w_planes(const bf16x8 (&qb)[NP][PB], AT at) {
#pragma unroll
    for (int pl = 0; pl < NP; ++pl)
#pragma unroll
        for (int i = 0; i < PB; ++i) *reinterpret_cast<bf16x8*>(at(pl, i)) = qb[pl][i];
}

// ---------------------------------------------------------------------------------------------------------------------
// DeformLoader — the modulated-deformable A loader of both split kernels (MODE == GEMM_DEFORM_NHWC): the bilinear gather x modulator of
// gemm_f32_kernel's loader (torchvision deform_conv2d, one offset group; a sample counts when y > -1 && y < Hin && x > -1 && x < Win, every
// corner is tested on its own, rows >= M are zero), computed in fp32 while A is staged and handed to split4 / split4h like any other A value.
// A staging thread holds one float4 (4 channels) of PA tile rows; the LPR lanes of a row are neighbours in the wave.
//   * Sampling parameters are computed ONCE per (pixel, tap): lane q of a row's lane group owns (tile row q % PA, tap TPB blk + q / PA) of the
//     current block of TPB = LPR / PA taps — offsets and modulator loaded one block ahead, floor / clamp / validity / four weights x modulator
//     worked out once per block — and keeps ONE packed corner word and four weights.  Whoever stages a K tile of that (row, tap) fetches them
//     with ds_bpermute (lanes of its own wave: no LDS bytes, no barrier), for each of the tap's Cin / KS K tiles.
//   * Corners are clamped into the map and carry a zero weight when they are not real corners: no exec branch around a load (see
//     load4_masked), so the corner loads of a later K tile stay in flight while an earlier one is blended, split and stored.  All four are
//     buffer loads off one resource (the whole batch of maps: launch_gemm checks it spans < 2 GiB); the K tile's channel offset is uniform.
//     The packed word is the byte offset of corner (yl, xl) — a multiple of 16 — with bit 0 / bit 1 saying whether the x / y neighbour is
//     one pixel / one map row further or (clamped at a border) the same pixel.
//   * The blend happens when the registers are consumed (finish), with the weights of the tile's tap: those live in two buffers by block
//     parity, because the tile being blended may belong to the block before the one whose corners are being issued.
// (A clamped corner's value is multiplied by a zero weight, not masked: a non-finite value there gives NaN, never a wrong finite number.
// A NaN offset poisons its sample where gemm_f32_kernel's loader drops it: see param_compute.)
// ---------------------------------------------------------------------------------------------------------------------
template <int PA, int LPR>
struct DeformLoader {
    static constexpr int TPB = LPR / PA;
    static_assert(TPB >= 1 && TPB * PA == LPR, "a row's lanes share out (tile row, tap) pairs evenly");
    __amdgpu_buffer_rsrc_t rsrc;
    int kq16, grp4;               // this lane's 16 bytes inside a K tile; 4 x the first lane of the row's lane group (ds_bpermute addresses bytes)
    int pixb, rowb, ntaps;
    // owner role (kept small: the staging waves of the warp-specialised kernel live within 128 VGPRs)
    int o_yx;                     // the row's window origin, (iy << 16) | (ix & 0xffff)
    unsigned o_img, o_om;         // byte offset of its image; element offset of its offsets / modulator row
    float om_y, om_x, om_m;       // offsets / modulator of the owner's tap in the next block
    unsigned own_off;
    float own_w[2][4];
    int cur_blk;

    __device__ __forceinline__ void init(const GemmParams& p, int m0, int lrow, int rpp, int kq, int lane) {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A + p.a_coff), 0, 0x7fffffff, 0x00020000);
        kq16 = kq * 16;
        grp4 = (lane & ~(LPR - 1)) * 4;
        pixb = p.lda * 4;
        rowb = p.Win * pixb;
        ntaps = p.kh * p.kw;
        const int m = m0 + lrow + (kq % PA) * rpp;
        const int mm = min(m, p.M - 1);
        const int hw = p.Hout * p.Wout;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / p.Wout, ox = rem - oy * p.Wout;
        // a row >= M reads row M - 1's offsets from an origin far above the map: never inside, so it is staged as zeros (launch_gemm bounds the geometry)
        const int iy = m < p.M ? oy * p.stride - p.pad : -32768, ix = ox * p.stride - p.pad;
        o_yx = (int)(((unsigned)iy << 16) | ((unsigned)ix & 0xffffu));
        o_img = (unsigned)b * (unsigned)(p.Hin * rowb);
        o_om = (unsigned)mm * (unsigned)p.om_ld;
        om_y = om_x = om_m = 0.f;
        own_off = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) own_w[0][c] = own_w[1][c] = 0.f;
        cur_blk = -1;
    }
    __device__ __forceinline__ void param_load(const GemmParams& p, int blk) {
        const int tap = min(blk * TPB + (kq16 >> 4) / PA, ntaps - 1);
        const float* om = p.om + o_om;
        om_y = om[2 * tap]; om_x = om[2 * tap + 1]; om_m = om[p.om_mask_off + tap];
    }
    __device__ __forceinline__ void param_compute(const GemmParams& p, int blk) {
        const ConvTap t = conv_tap_at(p, min(blk * TPB + (kq16 >> 4) / PA, ntaps - 1), 0);
        const float y = (float)((o_yx >> 16) + t.ky * p.dil) + om_y;
        const float x = (float)((short)o_yx + t.kx * p.dil) + om_x;
        const bool inside = y > -1.f && y < (float)p.Hin && x > -1.f && x < (float)p.Win;
        const float yf = floorf(y), xf = floorf(x);
        const float ly = y - yf, lx = x - xf, hy = 1.f - ly, hx = 1.f - lx;
        // (an inside sample has yl in [-1, Hin - 1]; the clamps tame NaN and huge offsets: such a sample is not inside, every weight is zero)
        const int yl = (int)fminf(fmaxf(yf, -1.f), (float)(p.Hin - 1)), xl = (int)fminf(fmaxf(xf, -1.f), (float)(p.Win - 1));
        const bool yl_ok = yl >= 0, yh_ok = yl + 1 <= p.Hin - 1, xl_ok = xl >= 0, xh_ok = xl + 1 <= p.Win - 1;
        // (selects, not a multiply by 0: ly / lx of a sample that is not inside may be NaN.)  A NaN position is not "outside": the offsets come
        // from a conv of the same mode, and beyond f32_half2's range that conv answers NaN — the sample is poisoned, not dropped, so that the
        // result stays non-finite instead of silently losing a tap.
        const float out = (y != y || x != x) ? __builtin_nanf("") : 0.f;
        const float w0 = (inside && yl_ok && xl_ok) ? om_m * (hy * hx) : out;
        const float w1 = (inside && yl_ok && xh_ok) ? om_m * (hy * lx) : out;
        const float w2 = (inside && yh_ok && xl_ok) ? om_m * (ly * hx) : out;
        const float w3 = (inside && yh_ok && xh_ok) ? om_m * (ly * lx) : out;
        const bool odd = blk & 1;
        own_w[0][0] = odd ? own_w[0][0] : w0; own_w[1][0] = odd ? w0 : own_w[1][0];
        own_w[0][1] = odd ? own_w[0][1] : w1; own_w[1][1] = odd ? w1 : own_w[1][1];
        own_w[0][2] = odd ? own_w[0][2] : w2; own_w[1][2] = odd ? w2 : own_w[1][2];
        own_w[0][3] = odd ? own_w[0][3] : w3; own_w[1][3] = odd ? w3 : own_w[1][3];
        const int ylc = max(yl, 0), xlc = max(xl, 0);
        // x / y neighbour distinct from the clamped low corner: only when both are real pixels
        own_off = (o_img + (unsigned)(ylc * p.Win + xlc) * (unsigned)pixb) | ((xl_ok && xh_ok) ? 1u : 0u) | ((yl_ok && yh_ok) ? 2u : 0u);
    }
    // the four corner loads of K tile [k0, k0 + KS) for tile rows [I0, I1) of this thread; called with ascending k0
    template <int I0, int I1>
    __device__ __forceinline__ void issue(const GemmParams& p, int k0, f32x4 (&qc)[PA][4]) {
        const ConvTap t = conv_tap(p, k0);
        const int tap = t.tap, ci0 = t.ci0, blk = tap / TPB;
        if (blk != cur_blk) {                       // uniform: a new block of taps
            if (cur_blk < 0) param_load(p, blk);    // (the first tile of a split-K slice)
            param_compute(p, blk);
            cur_blk = blk;
            if ((blk + 1) * TPB < ntaps) param_load(p, blk + 1);
        }
        const int src = grp4 + (tap - blk * TPB) * (PA * 4);
#pragma unroll
        for (int i = I0; i < I1; ++i) {
            const unsigned v = (unsigned)__builtin_amdgcn_ds_bpermute(src + i * 4, (int)own_off);
            const unsigned o = (v & ~3u) + (unsigned)kq16;
            const unsigned sx = (v & 1u) ? (unsigned)pixb : 0u, sy = (v & 2u) ? (unsigned)rowb : 0u;
            qc[i][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, ci0 * 4, 0));
            qc[i][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + sx, ci0 * 4, 0));
            qc[i][2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + sy, ci0 * 4, 0));
            qc[i][3] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o + sx + sy, ci0 * 4, 0));
        }
    }
    // modulator x bilinear blend of row i of the K tile that starts at k0 (its corners: qc)
    __device__ __forceinline__ f32x4 finish(const GemmParams& p, int k0, int i, const f32x4 (&qc)[4]) const {
        const int tap = conv_tap(p, k0).tap, blk = tap / TPB;
        const int src = grp4 + (tap - blk * TPB) * (PA * 4) + i * 4;
        const bool odd = blk & 1;
        float w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            w[c] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, odd ? own_w[1][c] : own_w[0][c])));
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = fmaf(w[3], qc[3][e], fmaf(w[2], qc[2][e], fmaf(w[1], qc[1][e], w[0] * qc[0][e])));
        return r;
    }
};

// =====================================================================================================================
// The warp-specialised kernel (gemm_split_ws_kernel): 128x128 tile, 8 waves.  Waves 0-3 consume, waves 4-7 produce.
// =====================================================================================================================
// LDS layout and the producers' thread map.  KS = k elements per stage; APL: A arrives in the P layout.
// Rows are UNPADDED KS-element rows with the 16-byte chunks of a row XOR-permuted by the row — key (row >> 3) & 1 for the 32-byte rows of a
// 16-deep stage (8 rows per 256-byte bank row), (row >> 2) & 3 for 64-byte rows (4 per bank row).  A ds_read_b128 lane group (16 consecutive
// rows, one logical chunk) then touches 16 different 16-byte slots, AND a producer store instruction (8-byte pieces: 4 or 8 lanes per row,
// 32 lanes = 8 or 4 whole rows) covers one bank row exactly once.  Padded rows (KS + 8 elements) were conflict-free for the reads only: the
// producers' ds_write_b64 halves wrapped onto banks of the first rows — the 4 % SQ_LDS_BANK_CONFLICT of profiles/r03_pmc_sq_c2_f32_split3.csv,
// paid by the staging waves, which are this kernel's critical path.
// The ring is 2 deep (2 x NP x 20 KB: two workgroups per CU at NP <= 2).  3 deep was slower: one workgroup per CU exposes each tile's
// prologue and epilogue.
template <int NP, int KS, bool APL>
struct WsLayout {
    static_assert(KS == 32 || KS == 16, "the interleaved W plane layout is per 32-deep K tile; a 16-deep stage takes one half of it");
    static_assert(!APL || KS == 32, "P-layout input is staged in whole 32-deep K tiles");
    static constexpr int BM = 128, BN = 128, WTM = 64, WTN = 64;
    static constexpr int NBUF = 2;
    static constexpr int ROW = KS;                                 // bf16 per LDS row
    static constexpr int KSTEPS = KS / 16;                         // 32x32x16 MFMA k-steps per stage
    static constexpr int AQ = KS / 4, RPP = 256 / AQ;              // producers: 256 threads, AQ float4 per KS-float row
    static constexpr int PA = APL ? 2 * NP : BM / RPP;             // P-layout input: 4 NP 16-byte chunks per (row, K tile), 128 rows / 256 threads
    static constexpr int WQ = KS / 8, WRPP = 256 / WQ, PB = BN / WRPP;   // WQ 16-byte chunks per KS-bf16 row
    // P-layout input: ONE ds_write_b128 instruction covers both planes of a row (lanes c = 0..3 plane 0, 4..7 plane 1), and BM x ROW x 2 bytes is
    // a multiple of the 256-byte bank row: the two planes of a row would sit on the same banks (2-way conflict on every staging write: 2.5 % of
    // wave cycles in profiles/r04_pmc_sq_c2_f32_half2.csv).  Plane p of A is therefore shifted by p x 128 bytes: rows r, r + 1 of both planes
    // then cover the four 64-byte quarters of a bank row.  (The fragment reads stay conflict-free: a constant shift per plane.)
    static constexpr int APAD = APL ? 64 : 0;                      // elements
    static constexpr int AREG = NP * BM * ROW + (NP - 1) * APAD;   // A region of a buffer
    static constexpr int BUF = AREG + NP * BN * ROW;               // bf16 elements per LDS buffer
    static constexpr int EP_LD = BN + 4;                           // floats per row of the epilogue's LDS image of the C tile
    static constexpr int SMEM_MAIN = NBUF * BUF * 2, SMEM_EPI = BM * EP_LD * 4, SMEM = SMEM_MAIN > SMEM_EPI ? SMEM_MAIN : SMEM_EPI;   // bytes
    static __device__ __forceinline__ int swz_key(int row) { return KS == 16 ? (row >> 3) & 1 : (row >> 2) & 3; }
    static __device__ __forceinline__ __bf16* buffer(__bf16* smem, int t) { return smem + (t % NBUF) * BUF; }     // the ring buffer of K tile t
};

// Cycle stamps of the diag library (brn_gemm_microbench; tools/gemm_trace.py reads the slots): 256 words per workgroup.  Thread 0 speaks for
// the consumers, thread 256 for the producers.  Every method is empty when !DIAG.
//   [0..2] / [8..10] start: clock, wall clock, (XCC id << 32) | HW id      [3] / [11] the prologue barrier      [4] / [12], [13] loop end (+ wall)
//   [5], [6] kernel end (+ wall)      [16 + 4 t ..] producer step t < 24: start, LDS stores done, step end, loads drained      [128 + 4 t ..] consumer step: start, MFMAs issued
template <bool DIAG>
struct WsTrace {
    unsigned long long* trc;
    __device__ __forceinline__ explicit WsTrace(const GemmParams& p) : trc((DIAG && p.trace) ? p.trace + (long)blockIdx.x * 256 : nullptr) {}
    __device__ __forceinline__ void start(int tid) const {
        if constexpr (DIAG) {
            if (trc && (tid == 0 || tid == 256)) {
                unsigned hwid, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                trc[(tid >> 8) * 8 + 0] = clock64();
                trc[(tid >> 8) * 8 + 1] = wall_clock64();
                trc[(tid >> 8) * 8 + 2] = ((unsigned long long)xcc << 32) | hwid;
            }
        }
    }
    __device__ __forceinline__ void cycles(bool who, int slot) const { if constexpr (DIAG) { if (trc && who) trc[slot] = clock64(); } }
    __device__ __forceinline__ void wall(bool who, int slot) const { if constexpr (DIAG) { if (trc && who) trc[slot] = wall_clock64(); } }
    __device__ __forceinline__ void drain_loads() const { if constexpr (DIAG) { if (trc) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } }
};

}  // namespace brn
