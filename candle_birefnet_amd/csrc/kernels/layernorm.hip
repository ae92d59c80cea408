// layernorm.hip — candle_nn::layer_norm forward (swin.rs:333,335,486,680,754), one wave64 per row, the row kept
// in registers (two-pass mean / biased variance, eps inside the sqrt), float4 loads and stores.  HBM-bound.
// mode 1 fuses PatchMerging's 2x2 strided gather + concat (swin.rs:505-522) into the load.
#include "layernorm_row.h"

namespace brn {

template <int SRC, int NV>
__global__ void __launch_bounds__(LN_WAVES * 64) layernorm_kernel(const LayerNormParams p) {
    const int lane = threadIdx.x & 63;
    const long nwaves = (long)gridDim.x * LN_WAVES;
    // each wave walks rows with a grid stride (few, fat workgroups: the kernel is launch/latency bound otherwise)
    for (long row = (long)blockIdx.x * LN_WAVES + (threadIdx.x >> 6); row < p.rows; row += nwaves) layernorm_row<SRC, NV>(p, row, lane);
}

hipError_t launch_layernorm(const LayerNormParams& p, hipStream_t s) {
    if (!layernorm_params_ok(p)) return hipErrorInvalidValue;
    long blocks = (p.rows + LN_WAVES - 1) / LN_WAVES;
    if (blocks > LN_MAX_BLOCKS) blocks = LN_MAX_BLOCKS;
    dim3 grid((unsigned)blocks), block(LN_WAVES * 64);
    const int nv = layernorm_nv(p);
#define BRN_LN(SRC_, NV_) hipLaunchKernelGGL((layernorm_kernel<SRC_, NV_>), grid, block, 0, s, p)
#define BRN_LN_NV(SRC_)                                                                        \
    if (nv == 1) BRN_LN(SRC_, 1); else if (nv == 2) BRN_LN(SRC_, 2); else if (nv == 3) BRN_LN(SRC_, 3); \
    else if (nv == 6) BRN_LN(SRC_, 6); else BRN_LN(SRC_, 12)
    if (p.part) { BRN_LN_NV(LN_SRC_SLICES); } else if (p.mode == 0) { BRN_LN_NV(LN_SRC_ROWS); } else { BRN_LN_NV(LN_SRC_MERGE); }
#undef BRN_LN_NV
#undef BRN_LN
    return hipGetLastError();
}

}  // namespace brn
