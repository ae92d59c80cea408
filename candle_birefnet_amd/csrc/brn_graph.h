// brn_graph.h — what the three files of the forward graph share (brn_graph.cpp: arena and the run_* primitives; brn_graph_swin.cpp: the
// backbone pass; brn_graph_model.cpp: decoder blocks, ASPP, decoder, the whole forward): the launch bracket and the graph branches.
#pragma once
#include "brn_host.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>

namespace brn {

// ---- launch bracket -----------------------------------------------------------------------------------------------
struct Cost { double flop, bytes; };
struct Bracket {
    Ctx& c; bool on;
    Bracket(Ctx& c_, int fam, double flop, double bytes, int M = 0, int N = 0, int K = 0) : c(c_), on(c_.profile && !c_.dry) {
        if (!on) return;
        auto next = [&]() -> hipEvent_t {
            if (*c.event_next >= c.event_pool->size()) { hipEvent_t e; BRN_HIP(hipEventCreate(&e)); c.event_pool->push_back(e); }
            return (*c.event_pool)[(*c.event_next)++];
        };
        LaunchRecord r; r.fam = fam; r.flop = flop; r.bytes = bytes; r.e0 = next(); r.e1 = next(); r.M = M; r.N = N; r.K = K; r.region = c.region;
        BRN_HIP(hipEventRecord(r.e0, c.stream));
        c.records->push_back(r);
    }
    Bracket(Ctx& c_, int fam, Cost cost, int M, int N, int K) : Bracket(c_, fam, cost.flop, cost.bytes, M, N, K) {}
    ~Bracket() { if (on) (void)hipEventRecord(c.records->back().e1, c.stream); }
};
#define BRN_LAUNCH(expr)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) fail(BRN_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));        \
    } while (0)
// compute mode BRN_F16 (c.bf16 == 2): the 16-bit kernels of namespace brn::hf (fp16 storage / MFMA operands)
#define S16F(C_, FN_) ((C_).bf16 == 2 ? hf::FN_ : FN_)

// ---- graph branches on auxiliary streams --------------------------------------------------------------------------------
// While a Branch is alive, launches go to aux stream k, ordered after everything enqueued on the main stream so far; join_branches
// makes the main stream wait for every branch enqueued since the last join.  Same kernels, same arguments, same results: only
// the order in which independent launches may run changes.  Buffers a branch writes must stay allocated until the join (Arena::hold).
struct Branch {
    Ctx& c; hipStream_t main; int k; bool on;
    Branch(Ctx& c_, int k_) : c(c_), main(c_.stream), k(k_), on(c_.br && !c_.dry && !c_.profile && k_ >= 0 && k_ < BRN_AUX_STREAMS && ((c_.br_mask >> k_) & 1u)) {
        if (!on) return;
        BRN_HIP(hipEventRecord(c.br->fork_ev[k], main));
        BRN_HIP(hipStreamWaitEvent(c.br->stream[k], c.br->fork_ev[k], 0));
        c.stream = c.br->stream[k];
    }
    ~Branch() {
        if (!on) return;
        (void)hipEventRecord(c.br->join_ev[k], c.stream);
        c.stream = main;
        c.pending |= 1u << k;
    }
};
inline void join_branches(Ctx& c, unsigned mask) {
    for (int k = 0; k < BRN_AUX_STREAMS; ++k)
        if (c.pending & mask & (1u << k)) BRN_HIP(hipStreamWaitEvent(c.stream, c.br->join_ev[k], 0));
    c.pending &= ~mask;
}
// ---- the generic window route (brn_window_generic.cpp) ---------------------------------------------------------------------
// The attention of one map for a window side other than 12 and 7, between the qkv GEMM and the projection: qkv [B, H, W, 3C] -> att
// [B, H, W, C] (both in the mode's storage type) as pack, bias build, flash attention with bias, scatter.  It lives outside the graph
// files, which link against nothing but the launches of their own (tests/test_graph_trace_cpu.py), and registers itself here when the
// library is loaded; null = not linked in.  Allocates from c.arena and releases to its own mark; in a dry run it only allocates.
using WindowGenericRoute = void (*)(Ctx& c, const SwinBlockW& blk, const float* qkv, float* att, int B, int H, int W, int C, int window, int shift);
extern WindowGenericRoute g_window_generic_route;      // defined in brn_graph_swin.cpp

// ---- GEMM -> LayerNorm with the split-K slices summed by the LayerNorm (brn_gemm_ln.cpp) ---------------------------------------------
// x_out = io.A w^T + bias + io.R (io.C, which may be io.R: the residual stream in place) and y = LayerNorm(x_out) into `out`, as a GEMM that
// leaves its raw slices (GemmPlan::raw) and a LayerNorm that sums them (LayerNormParams::part): no splitk_reduce_kernel, and x is not read
// back.  false = nothing enqueued or allocated (one slice planned, not a split mode, an activation ...): the caller launches the pair.
// Registered like the generic window route; null = today's launches.  Allocates the slice scratch identically in a dry run.
using GemmLnRoute = bool (*)(Ctx& c, const GemmW& w, const GemmIO& io, const LNW& ln, const LnOut& out);
extern GemmLnRoute g_gemm_ln_route;                    // defined in brn_graph_swin.cpp
// the dense descriptor of run_gemm and its fp32-class weights (brn_graph.cpp)
GemmParams dense_params(const GemmW& w, const GemmIO& io);
void fill_weights_f32(GemmParams& p, const GemmW& w);

constexpr int AUX_IPT = 3, AUX_LAT = 4;
constexpr unsigned AUX_ASPP_MASK = 7u;
struct ArenaHold { Arena& a; explicit ArenaHold(Arena& a_) : a(a_) { ++a.hold; } ~ArenaHold() { --a.hold; } };

}  // namespace brn
