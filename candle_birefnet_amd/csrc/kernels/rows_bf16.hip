// rows_bf16.hip — the whole-row kernels of compute modes BRN_BF16 / BRN_F16 (compiled twice, s16_common.h): dense GEMMs whose workgroups own
// complete rows of C, on v_mfma_f32_16x16x32 with fp32 accumulation.
//   gemm_wstat_bf16_kernel     short K (192 / 384), the weights resident in registers, bias + activation, 16-bit out
//   gemm_wstat_ln_bf16_kernel  the same core at N = K = 192 with + fp32 residual and the block's LayerNorm in the epilogue
//   gemm_rowln_bf16_kernel     the same epilogue for N = 768 / 384 and any K, W streamed through LDS
// One copy each of what they share, as per-lane state + __forceinline__ functions (no callbacks: the kernels keep their own loops, which is
// what leaves their register allocation alone): WstatLane / wstat_init / wstat_issue / wstat_tile (the weight-stationary core) and
// LnHalf / ln_half_prefetch / ln_half_finish (the residual + LayerNorm epilogue).  The tiled kernel that serves every other shape is in
// gemm_bf16.hip.
#include "../brn_kernels.h"
#include "s16_common.h"

BRN_S16_BEGIN

// =====================================================================================================================
// gemm_wstat_bf16_kernel — dense C = act(A W^T + b) for SHORT K (K = 64 KS: 192, or 384 with 32-row tiles) and wide A (M >> N): the stage-0 /
// stage-1 qkv and fc1 GEMMs of the Swin backbone at batch >= 4 (swin.rs:98,130; M = 655 360, K = 192, N = 576 / 768 at batch 8).  With three K steps per tile the
// persistent 256 x 256 kernel of gemm_bf16.hip is prologue / epilogue all the way (2.0 - 2.6 TB/s of algorithmic traffic); here the weights never
// move: a wave keeps its 48 columns of W (K x 48 bf16 = 72 VGPRs, loaded once, stored in MFMA fragment order by attach_dense_frags) for
// the whole launch and the workgroup streams 64-row tiles of A through a two-buffer LDS ring (LDS-DMA, XOR-swizzled 128-byte rows:
// swz_slot); what is left per tile is 24 KB in, 96 MFMAs per wave, 24 KB out.  A workgroup = 4 waves = 192 columns; the N / 192 column
// groups of a row tile are neighbouring workgroups of one XCD walking the same tiles (the A tile is read from HBM once, then from L2).
// The C tile goes back through the A buffer it came from (two 32-row halves, 512-byte rows, XOR-ed chunks) and leaves as 384-byte
// row segments.
// =====================================================================================================================
constexpr int WSTAT_WG_PER_CU = 2;      // 2: <= 256 VGPRs, no spill (forced to 168 for three per CU the kernel spills 30-40 registers)

// the row tiles [t_lo, t_hi) of BM rows that the workgroups of this XCD (same blockIdx % 8) walk: XCD x owns a contiguous run
template <int BM> __device__ __forceinline__ void xcd_tile_run(const GemmParams& p, int& t_lo, int& t_hi) {
    const int T = (p.M + BM - 1) / BM, xcd = blockIdx.x & 7;
    t_lo = (int)((long)T * xcd / 8); t_hi = (int)((long)T * (xcd + 1) / 8);
}

// The weight-stationary core.  Wave `wave` of a 4-wave workgroup keeps the K x 48 slice of W that starts at column n0 (and its bias) in
// registers (wstat_init); the workgroup walks row tiles t, t + nw, ... < t_hi of its XCD and streams them through the two-buffer ring
// `smem`: wstat_issue(first tile) once, then per tile wstat_tile — issue of the next tile, counted wait, the whole K loop — which leaves
// acc[i][j] = rows 16 i + (lane & 15) of the tile x columns n0 + 16 j + 4 (lane >> 4) + {0..3} and returns the tile's A buffer behind a
// workgroup barrier: the buffer is the kernel's epilogue's to reuse, and the epilogue ends with a barrier of its own.
// WBM = rows per A tile: 64 at K = 192 (two 24-KB buffers), 32 at K = 384 (the W slice is 144 VGPRs there; two 24-KB buffers again,
// so two workgroups still share a CU and one's epilogue overlaps the other's MFMAs)
template <int KS, int WBM>
struct WstatLane {
    static constexpr int SUB = WBM * 128;                                // bytes of one K step's sub-tile
    static constexpr int K32 = KS * 2, ABUF = KS * SUB;
    static constexpr int NJ = WBM / 32, RF = WBM / 16;                   // LDS-DMA instructions per wave and K step, 16-row fragments per tile
    static_assert(WBM == 64 || WBM == 32, "tile rows");
    s16x8 wfr[3][K32];                                                   // W fragments, resident for the whole launch
    f32x4 bias[3];
    unsigned a_voff[NJ];                                                 // this lane's share of an A tile: LDS-DMA instruction ii = wave + 4 j (j < NJ) of every
    int a_row[NJ];                                                       // sub-tile fills bank rows 4 ii .. 4 ii + 3
    int a_foff[RF][2];
};
template <int KS, int WBM>
__device__ __forceinline__ void wstat_init(const GemmParams& p, WstatLane<KS, WBM>& ws, int lane, int wave, int n0) {
    using L = WstatLane<KS, WBM>;
    constexpr int K32 = L::K32, NJ = L::NJ, RF = L::RF;
    {
        const char* wf = reinterpret_cast<const char*>(p.Wp) + ((long)(n0 >> 4) * K32 * 64 + lane) * 16;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int ks = 0; ks < K32; ++ks) ws.wfr[j][ks] = *reinterpret_cast<const s16x8*>(wf + (long)(j * K32 + ks) * 1024);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) ws.bias[j] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n0 + 16 * j + 4 * (lane >> 4)) : zero4();
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int pr = 4 * (wave + 4 * j) + (lane >> 4), qs = (lane & 15) ^ (pr & 15);
        ws.a_row[j] = 2 * pr + (qs >> 3);
        ws.a_voff[j] = (unsigned)((qs & 7) * 16);                       // byte offset inside the 128-byte K-step piece of the row
    }
#pragma unroll
    for (int i = 0; i < RF; ++i)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) ws.a_foff[i][s2] = swz_slot(16 * i + (lane & 15), 4 * s2 + (lane >> 4));
}
template <int KS, int WBM>
__device__ __forceinline__ void wstat_issue(const GemmParams& p, const WstatLane<KS, WBM>& ws, int wave, int t, char* buf) {
    const s16_t* Ab = reinterpret_cast<const s16_t*>(p.A);
    const int m0 = t * WBM;
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<s16_t*>(Ab + (long)m0 * p.lda + p.a_coff), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int j = 0; j < WstatLane<KS, WBM>::NJ; ++j) {
        const unsigned ro = (unsigned)((min(m0 + ws.a_row[j], p.M - 1) - m0) * p.lda * 2) + ws.a_voff[j];   // rows >= M re-read row M - 1 (never stored)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) blds16(rs, ro, ks * 128, buf + ks * WstatLane<KS, WBM>::SUB + (wave + 4 * j) * 1024);
    }
}
// tile t (the it-th of this workgroup, the next one being t + nw if < t_hi): returns its buffer, acc = the product
template <int KS, int WBM>
__device__ __forceinline__ char* wstat_tile(const GemmParams& p, const WstatLane<KS, WBM>& ws, char* smem, int wave, int it, int t, int nw, int t_hi,
                                            f32x4 (&acc)[WBM / 16][3]) {
    using L = WstatLane<KS, WBM>;
    constexpr int K32 = L::K32, NJ = L::NJ, RF = L::RF, ABUF = L::ABUF, SUB = L::SUB;
    char* buf = smem + (it & 1) * ABUF;
    const bool more = t + nw < t_hi;
    if (more) { wstat_issue(p, ws, wave, t + nw, smem + ((it + 1) & 1) * ABUF); wait_vmcnt<NJ * KS>(); }   // this tile (and the previous tile's stores) landed; the next one may be in flight
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < RF; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = zero4();
#pragma unroll
    for (int ks = 0; ks < K32; ++ks) {
        s16x8 af[RF];
#pragma unroll
        for (int i = 0; i < RF; ++i) af[i] = *reinterpret_cast<const s16x8*>(buf + (ks >> 1) * SUB + ws.a_foff[i][ks & 1]);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int i = 0; i < RF; ++i) acc[i][j] = BRN_MFMA_16X16X32(ws.wfr[j][ks], af[i], acc[i][j]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                       // every wave has read its fragments: the buffer now takes the C tile
    return buf;
}

template <int KS, int ACT, int WBM = 64>
__global__ void __launch_bounds__(256, 2) gemm_wstat_bf16_kernel(const GemmParams p) {
    constexpr int WBN = 192, ABUF = KS * WBM * 128;                      // columns per workgroup, bytes of an A buffer
    static_assert(ABUF >= 32 * 512, "a 32-row half of the C tile (512-byte rows) must fit the A buffer it replaces");
    __shared__ __attribute__((aligned(1024))) char smem[2 * ABUF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = p.N / WBN;
    // workgroups of one XCD (same blockIdx % 8): local index li -> column group li % G, walker li / G of nw
    const int li = blockIdx.x >> 3, nw = ((int)gridDim.x >> 3) / G;
    const int grp = li % G, wk = li / G;
    int t_lo, t_hi;
    xcd_tile_run<WBM>(p, t_lo, t_hi);
    if (wk >= nw) return;
    WstatLane<KS, WBM> ws;
    wstat_init(p, ws, lane, wave, grp * WBN + wave * 48);
    int t = t_lo + wk;
    if (t < t_hi) wstat_issue(p, ws, wave, t, smem);
    for (int it = 0; t < t_hi; ++it, t += nw) {
        f32x4 acc[WBM / 16][3];
        char* buf = wstat_tile(p, ws, smem, wave, it, t, nw, t_hi, acc);
        const int m0 = t * WBM;
        s16_t* Cb = reinterpret_cast<s16_t*>(p.C);
#pragma unroll
        for (int half = 0; half < WBM / 32; ++half) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = 2 * half + ii, row = 16 * ii + (lane & 15);          // row within the 32-row half
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    f32x4 v = acc[i][j] + ws.bias[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (ACT == ACT_GELU_ERF) v[e] = gelu_erf_bf16out(v[e]);
                        else if (ACT == ACT_RELU) v[e] = fmaxf(v[e], 0.f);
                    }
                    const int col = wave * 48 + 16 * j + 4 * (lane >> 4);           // column within the workgroup's 192
                    const u32x2 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
                    *reinterpret_cast<u32x2*>(buf + row * 512 + (((col >> 3) ^ (row & 31)) << 4) + (col & 4) * 2) = o;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int q = 0; q < 3; ++q) {                                // 32 rows x 24 chunks of 16 bytes over 256 threads
                const int idx = tid + 256 * q, row = idx / 24, ch = idx - row * 24;
                const u32x4 v = *reinterpret_cast<const u32x4*>(buf + row * 512 + ((ch ^ (row & 31)) << 4));
                const int m = m0 + half * 32 + row;
                if (m < p.M) *reinterpret_cast<u32x4*>(Cb + (long)m * p.ldc + p.c_coff + grp * WBN + ch * 8) = v;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                               // the half (and, after the second one, the buffer) is free again
        }
    }
}

// =====================================================================================================================
// The residual + LayerNorm epilogue of a 64-row tile of NC columns whose fp32 accumulators sit in the registers of the workgroup
// (32 LPR threads): x = acc + bias + residual (fp32, p.C, in place or not) and y = LayerNorm(x) gamma + beta (16-bit, Y).  Per 32-row
// half: ln_half_prefetch requests the residual rows, the kernel puts acc + bias of the half into cbuf as fp32 rows of NC * 4 bytes with
// 16-byte chunk ch of row r at byte ln_chunk<LPR>(r, ch) (how the accumulators are indexed differs between the kernels), and
// ln_half_finish takes the rows back with LPR lanes per row (chunks ec + LPR k): + residual, store of x, two-pass mean / biased variance
// over the LPR lanes — the arithmetic of layernorm_kernel; the order of the sums is part of the result's bits — gamma / beta (global or
// LDS), store of y.  It ends with a barrier: cbuf is free again.
// =====================================================================================================================
// byte offset of 16-byte chunk ch within row `row` of the fp32 C half: chunks XOR-ed with the row inside groups of LPR (768-byte rows = 48 chunks: 8, not 16)
template <int LPR> __device__ __forceinline__ int ln_chunk(int row, int ch) { return ((ch & ~(LPR - 1)) | ((ch ^ row) & (LPR - 1))) << 4; }
template <int NC, int LPR /* lanes per row */>
struct LnHalf {                                                          // a lane's share of one 32-row half
    static constexpr int CPL = NC / 4 / LPR;                             // 16-byte chunks per lane
    int er, ec, m;                                                       // row of the half, first chunk (then + LPR k), row of C
    f32x4 rr[CPL];                                                       // the residual
};
template <int NC, int LPR>
__device__ __forceinline__ LnHalf<NC, LPR> ln_half_prefetch(const GemmParams& p, int m_half, int tid) {
    static_assert(LPR == 8 || LPR == 16, "lanes per row");
    LnHalf<NC, LPR> h;
    h.er = tid >> (LPR == 16 ? 4 : 3); h.ec = tid & (LPR - 1);
    h.m = m_half + h.er;
    const int mc = min(h.m, p.M - 1);
    const float* Rf = reinterpret_cast<const float*>(p.R);
#pragma unroll
    for (int k = 0; k < LnHalf<NC, LPR>::CPL; ++k) h.rr[k] = *reinterpret_cast<const f32x4*>(Rf + (long)mc * p.ldr + p.r_coff + (h.ec + LPR * k) * 4);
    return h;
}
template <int NC, int LPR>
__device__ __forceinline__ void ln_half_finish(const GemmParams& p, const LnHalf<NC, LPR>& h, const char* cbuf, const float* gamma, const float* beta,
                                               float eps, s16_t* Y, int ldy) {
    constexpr int CPL = NC / 4 / LPR;
    const int er = h.er, ec = h.ec, m = h.m;
    float* Cf = reinterpret_cast<float*>(p.C);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    f32x4 xv[CPL];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        // ln_chunk<LPR>(er, ch), spelled out per LPR: through the function (or the one general form) the read-back offsets are no longer the
        // parent's (rowln<768>: one XOR + constants became 12 address computations, + 25 VGPRs; wstat_ln: 10 VGPRs fewer, other counts)
        const int ch = ec + LPR * k;
        if constexpr (LPR == 16) xv[k] =*reinterpret_cast<const f32x4*>(cbuf + er * (NC * 4) + (((ch & ~15) | ((ch ^ er) & 15)) << 4)) + h.rr[k];
        else xv[k] = *reinterpret_cast<const f32x4*>(cbuf + er * (NC * 4) + ((ch ^ (er & 7)) << 4)) + h.rr[k];
        sum += (xv[k][0] + xv[k][1]) + (xv[k][2] + xv[k][3]);
    }
    if (m < p.M) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) *reinterpret_cast<f32x4*>(Cf + (long)m * p.ldc + p.c_coff + (ec + LPR * k) * 4) = xv[k];
    }
#pragma unroll
    for (int d = 1; d < LPR; d *= 2) sum += __shfl_xor(sum, d);
    const float mean = sum / (float)NC;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        xv[k] = xv[k] - mean;
        sq += (xv[k][0] * xv[k][0] + xv[k][1] * xv[k][1]) + (xv[k][2] * xv[k][2] + xv[k][3] * xv[k][3]);
    }
#pragma unroll
    for (int d = 1; d < LPR; d *= 2) sq += __shfl_xor(sq, d);
    const float rstd = 1.0f / sqrtf(sq / (float)NC + eps);
    if (m < p.M) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c0 = (ec + LPR * k) * 4;
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c0), bt = *reinterpret_cast<const f32x4*>(beta + c0);
            const f32x4 o = xv[k] * rstd * gm + bt;
            const u32x2 ob = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
            *reinterpret_cast<u32x2*>(Y + (long)m * ldy + c0) = ob;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                       // the half is free again
}

// =====================================================================================================================
// gemm_wstat_ln_bf16_kernel — the attention output projection of a C = 192 stage with the block's second LayerNorm in its epilogue
// (swin.rs:310,406,407): x = A Wᵀ + bias + x (fp32 residual stream, in place) and y = LayerNorm(x) γ + β (bf16, the fc1 operand).
// N = K = 192: a workgroup of the weight-stationary kernel above owns WHOLE rows (4 waves x 48 columns), so the row statistics are
// local.  The C tile goes through the A buffer as fp32 (32 rows x 768 B = the 24-KB buffer, 16-byte chunks XOR-ed with the row); on the
// way back 8 lanes share a row (6 chunks each): ln_half_finish with γ / β from LDS.  What it saves is the stand-alone LayerNorm's read of x.
// =====================================================================================================================
__global__ void __launch_bounds__(256, 2) gemm_wstat_ln_bf16_kernel(const GemmParams p, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                     const float eps, s16_t* __restrict__ Y, const int ldy) {
    constexpr int KS = 3, WBM = 64, WBN = 192, ABUF = KS * WBM * 128;
    static_assert(ABUF == 32 * WBN * 4, "a 32-row half of the fp32 C tile is exactly one A buffer");
    __shared__ __attribute__((aligned(1024))) char smem[2 * ABUF];
    __shared__ __attribute__((aligned(16))) float gb_s[2 * WBN];         // gamma | beta
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t_lo, t_hi;
    xcd_tile_run<WBM>(p, t_lo, t_hi);
    if (tid < WBN) { gb_s[tid] = gamma[tid]; gb_s[WBN + tid] = beta[tid]; }
    const int wk = blockIdx.x >> 3, nw = (int)gridDim.x >> 3;
    WstatLane<KS, WBM> ws;
    wstat_init(p, ws, lane, wave, wave * 48);
    int t = t_lo + wk;
    if (t < t_hi) wstat_issue(p, ws, wave, t, smem);
    for (int it = 0; t < t_hi; ++it, t += nw) {
        f32x4 acc[4][3];
        char* buf = wstat_tile(p, ws, smem, wave, it, t, nw, t_hi, acc);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const auto h = ln_half_prefetch<WBN, 8>(p, t * WBM + half * 32, tid);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = 2 * half + ii, row = 16 * ii + (lane & 15);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int ch = (wave * 48 + 16 * j + 4 * (lane >> 4)) >> 2;      // 16-byte chunk of the 768-byte row
                    *reinterpret_cast<f32x4*>(buf + row * 768 + ln_chunk<8>(row, ch)) = acc[i][j] + ws.bias[j];
                }
            }
            ln_half_finish(p, h, buf, gb_s, gb_s + WBN, eps, Y, ldy);
        }
    }
}

// =====================================================================================================================
// gemm_rowln_bf16_kernel<NC> (round 4) — the row-owning projection for the WIDE stages (NC = 768: stage 2, 18 of the 24 blocks; NC = 384:
// stage 1): x = A W^T + bias + x on the fp32 residual stream (in place) AND y = LayerNorm(x) gamma + beta as the bf16 operand of the next
// GEMM, in one launch (swin.rs:310,406,407) — the stand-alone LayerNorm launch and its fp32 re-read of x are gone.
// A workgroup of 8 waves owns 64 WHOLE rows (64 x NC fp32 accumulators = 96 / 48 VGPRs per lane; wave w = columns [w NC/8, (w+1) NC/8)),
// so the row statistics are local.  W does not fit anything but L2, so it streams through LDS: K step 32 (64-byte tile rows, four per
// 256-byte bank row, 16-byte chunks XOR-ed with the bank row as in gemm_bf16_kernel<BBK = 32>), three ring slots of (64 + NC) x 64 B, the
// pieces of K step t + 2 issued right after the barrier of step t (counted vmcnt; waves 0-3 carry the A pieces).  Per 64 rows the
// workgroup takes in the whole W (1.18 MB at NC = 768): the K loop is bound by the CU's L2 -> LDS intake, not by the matrix pipe, and the
// launch as a whole by HBM (A once, x read + written once, y once) — which is the point: 378 MB per stage-2 launch instead of the 504 MB of
// projection + LayerNorm.  Epilogue: ln_half_prefetch / ln_half_finish through the ring (two 32-row fp32 halves, 16-byte chunks XOR-ed with the row) with 16
// lanes per row (whole 256-byte segments) and γ / β from global memory.  The next tile's first K step is already in flight (slot 2) during
// the epilogue.
// =====================================================================================================================
template <int NC>
__global__ void __launch_bounds__(512) gemm_rowln_bf16_kernel(const GemmParams p, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float eps, s16_t* __restrict__ Y, const int ldy) {
    constexpr int RBM = 64, RBK = 32, ROWB = RBK * 2;                    // 64-byte tile rows
    constexpr int WCOL = NC / 8;                                         // columns per wave: 96 / 48
    constexpr int FN = WCOL / 16, FM = RBM / 16;                         // 16 x 16 blocks of a wave tile
    constexpr int A_BYTES = RBM * ROWB, SLOT = (RBM + NC) * ROWB;        // 4 KB + 48 / 24 KB
    constexpr int LW = NC / 16 / 8;                                      // W pieces (1 KiB = 16 tile rows) per wave and K step: 6 / 3
    constexpr int HALF_BYTES = 32 * NC * 4;                              // a 32-row half of the fp32 C tile
    static_assert(3 * SLOT <= 160 * 1024 && HALF_BYTES <= 2 * SLOT - 0 && NC % 128 == 0, "ring / epilogue geometry");
    __shared__ __attribute__((aligned(1024))) char smem[3 * SLOT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = blockIdx.x >> 3, nw = (int)gridDim.x >> 3;
    int t_lo, t_hi;
    xcd_tile_run<RBM>(p, t_lo, t_hi);
    const int nk = p.K / RBK;
    const s16_t* Ab = reinterpret_cast<const s16_t*>(p.A);
    const s16_t* Wb = reinterpret_cast<const s16_t*>(p.Wp);

    // ---- LDS-DMA: instruction ii fills bank rows 4 ii .. 4 ii + 3 (16 tile rows); lane -> (tile row, k chunk) through the swizzle ----
    const int pr_l = lane >> 4;
    // (bank row pr = 4 ii + pr_l, key pr & 3 = pr_l: the lane's logical slot and hence its (row in the 16-row piece, chunk) are the same for every piece)
    const int qs = (lane & 15) ^ pr_l;
    const int row16 = 4 * pr_l + (qs >> 2);                              // row within a 16-row piece
    const unsigned kch_b = (unsigned)((qs & 3) * 16);                    // byte offset of the lane's k chunk within the 64-byte K step
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<s16_t*>(Wb), 0, 0x7fffffff, 0x00020000);
    unsigned w_voff[LW];
#pragma unroll
    for (int j = 0; j < LW; ++j) w_voff[j] = (unsigned)((16 * (wave * LW + j) + row16) * p.wp_ld * 2) + kch_b;
    auto issue = [&](int m0, int kt, int slot) {                         // K step kt of the row tile at m0 into ring slot `slot`
        char* sb = smem + slot * SLOT;
        if (wave < 4) {
            const int r = 16 * wave + row16;
            const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<s16_t*>(Ab + (long)m0 * p.lda + p.a_coff), 0, 0x7fffffff, 0x00020000);
            const unsigned vo = (unsigned)((min(m0 + r, p.M - 1) - m0) * p.lda * 2) + kch_b;     // rows >= M re-read row M - 1 (never stored)
            blds16(a_rsrc, vo, kt * ROWB, sb + wave * 1024);
        }
#pragma unroll
        for (int j = 0; j < LW; ++j) blds16(w_rsrc, w_voff[j], kt * ROWB, sb + A_BYTES + (wave * LW + j) * 1024);
    };
    // fragment offsets within a slot: 16x16x32: lane reads row (lane & 15) of a 16-row block (4 bank rows), chunk lane >> 4 (all of a K step)
    const int f_off = ((lane & 15) >> 2) * 256 + (((((lane & 15) & 3) << 2) | (lane >> 4)) ^ (((lane & 15) >> 2) & 3)) * 16;

    int t = t_lo + wk;
    if (t < t_hi) issue(t * RBM, 0, 2);                                  // K step kt lives in slot (kt + 2) % 3
    for (; t < t_hi; t += nw) {
        const int m0 = t * RBM;
        f32x4 acc[FM][FN];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = zero4();
        if (nk > 1) issue(m0, 1, 0);
        for (int kt = 0; kt < nk; ++kt) {
            // this wave's pieces of step kt have landed when at most those of step kt + 1 are outstanding
            if (kt + 1 < nk) { if (wave < 4) wait_vmcnt<LW + 1>(); else wait_vmcnt<LW>(); }
            else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();                                // everybody's pieces landed; everybody is done reading step kt - 1
            if (kt + 2 < nk) issue(m0, kt + 2, (kt + 4) % 3);            // into the slot step kt - 1 just left
            const char* sb = smem + ((kt + 2) % 3) * SLOT;
            s16x8 af[FM], bfr[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const s16x8*>(sb + i * 1024 + f_off);
#pragma unroll
            for (int j = 0; j < FN; ++j) bfr[j] = *reinterpret_cast<const s16x8*>(sb + A_BYTES + (wave * FN + j) * 1024 + f_off);
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
                for (int i = 0; i < FM; ++i) acc[i][j] = BRN_MFMA_16X16X32(bfr[j], af[i], acc[i][j]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                    // every fragment read of the tile is done: the ring is free
        const bool more = t + nw < t_hi;
        if (more) issue((t + nw) * RBM, 0, 2);                           // the next tile's first K step flies during the epilogue (slot 2 is not touched by it)
        // ---- epilogue: two 32-row halves through smem[0, HALF_BYTES); after the second one the K loop's slots 0 / 1 are free again ----
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const auto h = ln_half_prefetch<NC, 16>(p, m0 + half * 32, tid);
#pragma unroll
            for (int ii = 0; ii < 2; ++ii) {
                const int i = 2 * half + ii, row = 16 * ii + (lane & 15);
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    const int col = wave * WCOL + 16 * j + 4 * (lane >> 4);
                    f32x4 bias4 = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : zero4();
                    *reinterpret_cast<f32x4*>(smem + row * (NC * 4) + ln_chunk<16>(row, col >> 2)) = acc[i][j] + bias4;
                }
            }
            ln_half_finish(p, h, smem, gamma, beta, eps, Y, ldy);
        }
    }
}
bool gemm_rowln_eligible(const GemmParams& p) {
    return p.mode == GEMM_DENSE && p.Wp && (p.N == 768 || p.N == 384) && p.K >= 64 && (p.K % 32) == 0 && p.c_f32 && p.R && p.r_f32 && !p.scale && !p.bbias &&
           p.act == ACT_NONE && ((p.lda | p.a_coff) & 7) == 0 && ((p.ldc | p.c_coff | p.ldr | p.r_coff) & 3) == 0 && p.M >= 8192 && p.wp_rows >= p.N &&
           p.wp_ld >= p.K && (p.wp_ld & 7) == 0 && (double)p.wp_ld * 2.0 * p.N < 2147483648.0 && (double)p.lda * 2.0 * 64 < 2147483648.0;
}
hipError_t launch_gemm_rowln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y_bf16, int ldy, hipStream_t s) {
    if (!BRN_S16_SELF(gemm_rowln_eligible)(p) || !gamma || !beta || !y_bf16 || (ldy & 3)) return hipErrorInvalidValue;
    const int tiles = (p.M + 63) / 64;
    int g = launch_cus();
    if (g > tiles) g = (tiles + 7) / 8 * 8;
    dim3 grid(g), block(512);
    if (p.N == 768) hipLaunchKernelGGL(gemm_rowln_bf16_kernel<768>, grid, block, 0, s, p, gamma, beta, eps, reinterpret_cast<s16_t*>(y_bf16), ldy);
    else hipLaunchKernelGGL(gemm_rowln_bf16_kernel<384>, grid, block, 0, s, p, gamma, beta, eps, reinterpret_cast<s16_t*>(y_bf16), ldy);
    return hipGetLastError();
}

bool gemm_wstat_ln_eligible(const GemmParams& p) {
    return p.mode == GEMM_DENSE && p.Wp && p.K == 192 && p.N == 192 && p.c_f32 && p.R && p.r_f32 && !p.scale && !p.bbias && p.act == ACT_NONE &&
           ((p.lda | p.a_coff) & 7) == 0 && ((p.ldc | p.c_coff | p.ldr | p.r_coff) & 3) == 0 && p.M >= 32768 && (long)p.lda * 2 * 64 < 0x7fffffffL;
}
hipError_t launch_gemm_wstat_ln(const GemmParams& p, const float* gamma, const float* beta, float eps, void* y_bf16, int ldy, hipStream_t s) {
    if (!BRN_S16_SELF(gemm_wstat_ln_eligible)(p) || !gamma || !beta || !y_bf16 || (ldy & 3)) return hipErrorInvalidValue;
    dim3 grid(8 * (launch_cus() * 2 / 8)), block(256);
    hipLaunchKernelGGL(gemm_wstat_ln_bf16_kernel, grid, block, 0, s, p, gamma, beta, eps, reinterpret_cast<s16_t*>(y_bf16), ldy);
    return hipGetLastError();
}

bool gemm_wstat_eligible(const GemmParams& p) {
    // (N / 192 column groups share the chip's workgroup slots: beyond that many groups there is no walker left per group, and the
    // tiled kernel serves the shape)
    return p.mode == GEMM_DENSE && p.Wp && (p.K == 192 || p.K == 384) && p.N >= 192 && (p.N % 192) == 0 && p.N / 192 <= launch_cus() * WSTAT_WG_PER_CU / 8 &&
           !p.c_f32 && !p.R && !p.scale && !p.bbias &&
           ((p.lda | p.a_coff | p.ldc | p.c_coff) & 7) == 0 && p.M >= 32768 && (long)p.lda * 2 * 64 < 0x7fffffffL;
}
hipError_t launch_gemm_wstat(const GemmParams& p, hipStream_t s) {
    if (!BRN_S16_SELF(gemm_wstat_eligible)(p)) return hipErrorInvalidValue;
    const int G = p.N / 192;
    const int nw = (launch_cus() * WSTAT_WG_PER_CU / 8) / G;
    if (nw < 1) return hipErrorInvalidValue;
    dim3 grid(8 * G * nw), block(256);
    if (p.K == 384) {
        if (p.act == ACT_GELU_ERF) hipLaunchKernelGGL((gemm_wstat_bf16_kernel<6, ACT_GELU_ERF, 32>), grid, block, 0, s, p);
        else if (p.act == ACT_RELU) hipLaunchKernelGGL((gemm_wstat_bf16_kernel<6, ACT_RELU, 32>), grid, block, 0, s, p);
        else hipLaunchKernelGGL((gemm_wstat_bf16_kernel<6, ACT_NONE, 32>), grid, block, 0, s, p);
        return hipGetLastError();
    }
    if (p.act == ACT_GELU_ERF) hipLaunchKernelGGL((gemm_wstat_bf16_kernel<3, ACT_GELU_ERF>), grid, block, 0, s, p);
    else if (p.act == ACT_RELU) hipLaunchKernelGGL((gemm_wstat_bf16_kernel<3, ACT_RELU>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((gemm_wstat_bf16_kernel<3, ACT_NONE>), grid, block, 0, s, p);
    return hipGetLastError();
}

BRN_S16_END
