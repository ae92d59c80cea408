// gemm_conv_halo.h — conv_halo_kernel, the halo-staged implicit GEMM of the two-plane modes (f32_half2, f32_split2) for 3x3 / stride 1 /
// dilation 1 / pad 1 convs over channels-last fp32 maps (which launches: conv_halo_eligible, conv_halo_geometry.h; routed by
// launch_gemm_split for the plans of the 4-wave tiles).
// gemm_split_kernel orders K as (tap, channel) and stages a fresh A tile per K step: every input element is fetched and split nine times, once
// per tap.  Here the K loop is chunk-major: per 32-channel chunk the (TH + 2) x (TW + 2) halo of the workgroup's TH x TW pixel block is loaded
// and split ONCE into LDS, and the nine taps read their A fragments from it at the shifted pixel (ty + ky) (TW + 2) + tx + kx.  W needs no
// repacking: K tile tap (Cin / 32) + chunk of the [row][K / 32][plane][32] layout, fetched by each wave for itself straight into registers (16 rows x 64 bytes
// per plane and block, put into MFMA fragment order by ds_bpermute: no LDS bytes, no barrier per tap), two taps ahead.  The next chunk's halo is in flight in
// registers while the current chunk's nine taps multiply, and is split and stored into the other LDS buffer behind them: one barrier per chunk.
// Per output element the sum runs over chunks ascending, taps ascending inside a chunk, the plane products smallest first (plane_products),
// then over the split-K slices in splitk_reduce_kernel: the same order for every pixel of every image, no atomics.
#pragma once
#include <type_traits>
#include "../brn_kernels.h"
#include "conv_halo_geometry.h"
#include "gemm_common.h"
#include "gemm_split_stages.h"

namespace brn {

// LDS image of one halo: per plane four arrays, one per 8-channel group (the 16 bytes a lane of a 16x16x32 MFMA holds), of NPIX 16-byte
// pixel slots.  A fragment read (ds_read_b128: lane l reads pixel base + (l & 15), group l >> 4) starts at an arbitrary pixel, so no XOR key
// of the row can serve; but a ds_read_b128 lane group is 8 pixels of one channel group + the OTHER 8 pixels of the next one, and with arrays a
// multiple of 256 bytes apart (NPIX % 16 == 0) those are 16 consecutive 16-byte slots modulo the 64 banks whatever the base: conflict-free.
// The staging stores (ds_write_b64, 16 lanes = 2 pixels x 8 float4) would put all four groups of a pixel pair on the same banks; the pad
// between the group pairs {0, 1} and {2, 3}, which no read's lane group straddles, halves that to two-way.
struct HaloLayout {
    static constexpr int NPIX = 192;                            // HALO_PIXELS rounded up to 16 (the slots behind the halo hold zeros, never read)
    static constexpr int GROUP = NPIX * 16, PAIR_PAD = 64;      // bytes
    static constexpr int PLANE = 4 * GROUP + PAIR_PAD, BUF = 2 * PLANE;
    static constexpr int EP_LD = HALO_BN + 4;                   // floats per row of the epilogue's LDS image of the C tile
    static constexpr int SMEM_MAIN = 2 * BUF, SMEM_EPI = HALO_BM * EP_LD * 4, SMEM = SMEM_MAIN > SMEM_EPI ? SMEM_MAIN : SMEM_EPI;
    static_assert(NPIX >= HALO_PIXELS && NPIX % 16 == 0 && PLANE % 16 == 0, "fragment reads are 16-byte aligned and conflict-free");
    static __device__ __forceinline__ int group_off(int g) { return g * GROUP + (g >> 1) * PAIR_PAD; }
};

template <bool H>   // H: the two planes are fp16 (mode f32_half2), else bf16 (f32_split2)
__global__ void __launch_bounds__(256) conv_halo_kernel(const GemmParams p) {
    using L = HaloLayout;
    constexpr int NP = 2, PA = (HALO_PIXELS * 8 + 255) / 256;   // float4 pieces of a halo chunk per thread
    static_assert(HALO_TW == 16 && HALO_TH == 8 && HALO_BN == 64, "2 x 2 waves of 4 x 2 blocks of 16 x 16");
    static_assert((256 / 8) * PA <= L::NPIX, "every staged piece has a pixel slot");
    __shared__ __attribute__((aligned(16))) char smem[L::SMEM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int r16 = lane & 15, kc = lane >> 4;

    // work item: (slice, pixel block, N tile), N fastest: the N tiles of a block share its halo in L2
    const int Hm = p.Hout, Wm = p.Wout;
    const int tiles_n = (p.N + HALO_BN - 1) / HALO_BN;
    const int ntiles = conv_halo_tiles(p.M / (Hm * Wm), Hm, Wm) * tiles_n;
    const int swz = xcd_remap();
    const int slice = swz / ntiles, t = swz - slice * ntiles;
    const int tile_m = t / tiles_n, n0 = (t - tile_m * tiles_n) * HALO_BN;
    const ConvHaloTile tl = conv_halo_tile(Hm, Wm, tile_m);
    const int nch = p.Cin / 32, per = conv_halo_chunks_per_slice(p.Cin, p.splitk);
    const int c0 = slice * per, c1 = min(nch, c0 + per);

    // A: one buffer resource per image; a lane's pixel offset is fixed for the tile, the chunk's channel offset is uniform.  A halo pixel
    // outside the image (and a piece behind the halo) gets an offset past num_records, which the buffer unit answers with zeros.
    const __amdgpu_buffer_rsrc_t rsrc_a =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A + (long)tl.b * p.Hin * p.Win * p.lda + p.a_coff), 0, 0x7fffffff, 0x00020000);
    const int kq = tid & 7;
    unsigned voff_a[PA];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int hp = (tid >> 3) + 32 * i, hy = hp / HALO_W, hx = hp - hy * HALO_W;
        const int y = tl.y0 - 1 + hy, x = tl.x0 - 1 + hx;
        const bool ok = hp < HALO_PIXELS && (unsigned)y < (unsigned)p.Hin && (unsigned)x < (unsigned)p.Win;
        voff_a[i] = ok ? (unsigned)(((y * p.Win + x) * p.lda + kq * 4) * 4) : 0x80000000u;
    }
    const int a_st = L::group_off(kq >> 1) + (tid >> 3) * 16 + (kq & 1) * 8;       // piece i: + 512 i
    // W planes: a resource based at the N tile's first row (rows are padded to 128: a 64-row tile may over-read), lane = (row, 8-k group)
    const long wrow_stride = (long)p.K * NP;
    const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<__bf16*>(reinterpret_cast<const __bf16*>(p.Wp) + (long)n0 * wrow_stride), 0, 0x7fffffff, 0x00020000);
    // A load instruction covers 16 rows x 64 bytes of one plane with lane l on (row l >> 2, 8-k group l & 3): four neighbouring lanes read one row's
    // 64 contiguous bytes.  (Loaded in fragment order — lane l on row l & 15 — every lane of an instruction is a request to another cache line:
    // measured, the texture unit then bounds the kernel at 4 x the time of these.)  ds_bpermute puts them in fragment order, lane l <- 4 (l & 15) + (l >> 4).
    unsigned voff_w[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) voff_w[j] = (unsigned)(((long)(wn * 32 + j * 16 + (lane >> 2)) * wrow_stride + (lane & 3) * 8) * 2);
    const int w_src = (r16 * 4 + kc) * 4;          // ds_bpermute addresses bytes
    // A fragments: block i of the wave is output row wm 4 + i, 16 consecutive x; tap (ky, kx) reads halo pixel (wm 4 + i + ky) HALO_W + r16 + kx
    const int a_rd = L::group_off(kc) + (wm * 4 * HALO_W + r16) * 16;

    f32x4 ra[PA];
    u32x4 wraw[NP][2];             // the W loads in flight, two taps ahead
    bf16x8 wb[2][NP][2];           // W fragments of the current and the next tap
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = zero4();

    auto aload = [&](int c) {
#pragma unroll
        for (int i = 0; i < PA; ++i) ra[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, voff_a[i], c * 128, 0));
    };
    auto astore = [&](int buf) {
        char* dst = smem + buf * L::BUF + a_st;
#pragma unroll
        for (int i = 0; i < PA; ++i) stage_a_row<NP, H>(ra[i], 0xffffffffu, false, p.a_scale, [&](int pl) { return dst + pl * L::PLANE + i * 512; });
    };
    // W of step `tap` of chunk c (tap >= 9: of chunk c + 1, if the slice has one): K tile tap (Cin / 32) + c
    auto wload = [&](int c, int tap) {
        if (tap >= 9) { tap -= 9; ++c; }
        if (c >= c1) return;
        const int wk = (tap * nch + c) * (NP * 64);                  // bytes, uniform
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int j = 0; j < 2; ++j) wraw[pl][j] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_w, voff_w[j], wk + pl * 64, 0));
    };
    auto wpermute = [&](bf16x8 (&q)[NP][2]) {
#pragma unroll
        for (int pl = 0; pl < NP; ++pl)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                u32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (unsigned)__builtin_amdgcn_ds_bpermute(w_src, (int)wraw[pl][j][e]);
                q[pl][j] = __builtin_bit_cast(bf16x8, v);
            }
    };
    // one chunk: its halo sits in LDS buffer `buf`, the W fragments of its tap 0 in register set PAR, the loads of its tap 1 in flight
    auto chunk = [&](int c, int buf, auto par) {
        constexpr int PAR = decltype(par)::value;
        const bool more = c + 1 < c1;
        if (more) aload(c + 1);
        const char* src = smem + buf * L::BUF + a_rd;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int cur = (tap + PAR) & 1, ky = tap / 3, kx = tap - ky * 3;
            if (tap < 8 || more) wpermute(wb[cur ^ 1]);      // the next step's W, loaded a step ago
            wload(c, tap + 2);
            // (left alone, the scheduler sinks these loads to their first use, to save registers: every tap then waits a whole L2 round trip)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                bf16x8 af[NP][2];
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        af[pl][i] = *reinterpret_cast<const bf16x8*>(src + pl * L::PLANE + ((half * 2 + i + ky) * HALO_W + kx) * 16);
                plane_products<NP, H, true>(af, wb[cur], acc, half * 2, 0);
            }
        }
        if (more) astore(buf ^ 1);
        __syncthreads();
    };

    if (c0 < c1) {
        aload(c0);
        wload(c0, 0);
        astore(0);
        wpermute(wb[0]);
        wload(c0, 1);
        __syncthreads();
    }
    for (int c = c0; c < c1; c += 2) {
        chunk(c, 0, std::integral_constant<int, 0>{});
        if (c + 1 < c1) chunk(c + 1, 1, std::integral_constant<int, 1>{});
    }

    // every fragment read retired at the last barrier: the accumulators are laid down as a row-major image of the C tile (the product was
    // formed transposed: a lane holds row r16 of a block and columns 4 kc .. + 3), then written by all four waves through the fp32 epilogue
    float* ctile = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            *reinterpret_cast<f32x4*>(ctile + (wm * 64 + i * 16 + r16) * L::EP_LD + wn * 32 + j * 16 + 4 * kc) = acc[i][j];
    __syncthreads();
    const int c4 = (tid & 15) * 4, n = n0 + c4;
    if (n >= p.N) return;
    const EpiCols cols = epilogue_cols(p, slice, n);
#pragma unroll 2
    for (int ps = 0; ps < HALO_BM / 16; ++ps) {
        const int row = ps * 16 + (tid >> 4);
        const int m = conv_halo_row(Hm, Wm, tl, row);
        if (m < 0) continue;
        epilogue_row<false, false>(p, cols, m, n, *reinterpret_cast<const f32x4*>(ctile + row * L::EP_LD + c4));
    }
}

template <bool H>
static hipError_t launch_conv_halo(const GemmParams& p, hipStream_t s) {
    static_assert(HALO_CONV_MODE == GEMM_CONV_NHWC, "conv_halo_geometry.h names the mode by value");
    const int tiles = conv_halo_tiles(p.M / (p.Hout * p.Wout), p.Hout, p.Wout) * ((p.N + HALO_BN - 1) / HALO_BN) * p.splitk;
    hipLaunchKernelGGL((conv_halo_kernel<H>), dim3(tiles), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace brn
