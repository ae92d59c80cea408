// brn_gemm_ln.cpp — a route of the Swin graph that lives outside the graph files and registers itself when the library is loaded
// (g_gemm_ln_route in brn_graph.h; the graph files reference no symbol outside their own launches): a split-mode dense GEMM followed by a
// LayerNorm as a GEMM that leaves its raw split-K slices + a LayerNorm that sums them.  The reduce pass of a split-K GEMM is "sum the slices,
// add bias and residual, write x", and the LayerNorm behind it reads that x back at once: the LayerNorm does the sum itself, in the reduce
// pass's operand order, so x keeps its bits under the same plan.  With the reduce pass gone a cut costs little, and plan_gemm_ln cuts where
// plan_gemm does not.
#include "brn_graph.h"

namespace brn {
namespace {

bool gemm_ln_route(Ctx& c, const GemmW& w, const GemmIO& io, const LNW& ln, const LnOut& out) {
    const int sw = switches().gemm_ln;
    if (!sw || c.bf16 || !w.wp || !(w.planes == 2 || w.planes == 3) || w.mode != GEMM_DENSE || w.act != ACT_NONE || w.scale || io.bbias || io.c_planes ||
        out.y_s16 || ln.C != w.N || !ln.g || !ln.b || (w.N & 3) || ((io.ldc | io.c_coff) & 3) || (io.R && ((io.ldr | io.r_coff) & 3)))
        return false;
    const int M = io.M;
    GemmPlan pl = plan_gemm_ln(M, w.N, w.K, w.planes);
    if (sw == 2) {          // every eligible pair, two slices (tests, A/B): the tile plan_gemm would run, cut in two
        pl = plan_gemm(M, w.N, w.K, w.planes);
        pl.splitk = w.K / 32 >= 2 ? 2 : 1;
        pl.ws_floats = (size_t)pl.splitk * M * w.N;
        pl.raw = 1;
    }
    if (pl.splitk < 2) return false;
    if (io.a_planes) pl.cfg = 0;              // P operands exist only on the warp-specialised kernel (run_gemm)
    // the slices live until the LayerNorm has been enqueued (in-order stream), then they are dead
    const size_t mk = c.arena->mark();
    float* ws = c.arena->alloc(pl.ws_floats);
    c.arena->release(mk);
    if (c.dry) return true;
    GemmParams p = dense_params(w, io);
    p.bbias_rows = 1;
    fill_weights_f32(p, w);
    p.a_planes = io.a_planes;
    {
        const double mn = (double)M * w.N;
        Bracket b(c, FAM_GEMM_DENSE, 2.0 * mn * w.K, 4.0 * ((double)M * w.K + (double)w.N * w.K + pl.splitk * mn), M, w.N, w.K);
        BRN_LAUNCH(launch_gemm(p, pl, ws, c.stream));
    }
    LayerNormParams q{};
    q.y = out.y; q.rows = M; q.C = ln.C; q.gamma = ln.g; q.beta = ln.b; q.eps = 1e-5f;
    q.ldy = out.ldy; q.y_coff = out.y_coff; q.y_planes = out.y_planes;
    q.y_h2 = out.y_planes == 2 ? c.h2_scale : 0.f;
    q.part = ws; q.slices = pl.splitk; q.bias = w.bias;
    q.R = io.R; q.ldr = io.ldr; q.r_coff = io.r_coff;
    q.x_out = io.C; q.ldxo = io.ldc; q.xo_coff = io.c_coff;
    Bracket b(c, FAM_LAYERNORM, 0.0, 4.0 * (pl.splitk + (io.R ? 3.0 : 2.0)) * M * (double)ln.C, M, ln.C, pl.splitk);
    BRN_LAUNCH(launch_layernorm(q, c.stream));
    return true;
}

struct Registrar { Registrar() { g_gemm_ln_route = &gemm_ln_route; } } registrar;     // runs when the library is loaded

}  // namespace
}  // namespace brn
