// brn_window_generic.cpp — the generic window route: the attention of a Swin block for every window side the fused kernels
// (kernels/window_attention.hip: 12 and 7) do not cover, as
//   pack -> bias build -> flash attention with bias (1 or 2 launches) -> scatter
// between the block's qkv GEMM and its projection (swin_attention_multi, brn_graph_swin.cpp, which reaches this file through
// g_window_generic_route: the graph files reference no symbol outside their own launches).  DESIGN.md 3.2e.
//
// Slots (kernels/window_generic_geometry.h): the interior windows of all images, then [image][border window].  An unshifted block has no
// mask (swin.rs:383-384, even on a padded canvas): one launch over all slots, n_bias = 1.  A shifted block runs the interior slots with
// the plain relative-position pattern (n_bias = 1) and the border slots with n_bias = nwh + nww - 1 patterns, slot % n_bias = the border
// window — the launch's batch is [image][border window], so the flash kernel's b % n_bias is the window's pattern.
// q, k, v and y are fp32 in every mode (the flash kernel's interface); in the 16-bit modes the kernel rounds q, k, v and the softmax
// numerators to the 16-bit type itself (s16), and they already hold 16-bit values: the qkv GEMM's rounded output.
#include "brn_graph.h"
#include "kernels/window_generic_geometry.h"

namespace brn {
namespace {

void window_generic_route(Ctx& c, const SwinBlockW& blk, const float* qkv, float* att, int B, int H, int W, int C, int window, int shift) {
    if (window < WGEN_MIN_WS || window > WGEN_MAX_WS || !(shift == 0 || shift == window / 2) || blk.heads < 1 || C != blk.heads * 32)
        fail(BRN_ERR_INVALID_ARG, "generic window route: window_size %d (%d .. %d), shift %d (0 or window_size / 2), head_dim %d (32)", window, WGEN_MIN_WS,
             WGEN_MAX_WS, shift, blk.heads > 0 ? C / blk.heads : 0);
    const WgenGeom g = wgen_geom(B, H, W, window, shift);
    const int N = wgen_tokens(g), heads = blk.heads, slots = wgen_slots(g), n_pat = wgen_bias_patterns(g);
    const size_t per_slot = (size_t)heads * N * 32, nqkv = (size_t)slots * per_slot, slab = (size_t)heads * N * N;
    // everything from the arena, sized by the arguments alone, before anything is launched: a dry run plans exactly this
    const size_t mk = c.arena->mark();
    float* q = c.arena->alloc(nqkv);
    float* k = c.arena->alloc(nqkv);
    float* v = c.arena->alloc(nqkv);
    float* y = c.arena->alloc(nqkv);
    float* bias = c.arena->alloc((size_t)n_pat * slab);
    if (!c.dry) {
        WindowGenericParams p{};
        p.B = B; p.H = H; p.W = W; p.C = C; p.heads = heads; p.ws = window; p.shift = shift; p.s16 = c.bf16;
        p.qkv = qkv; p.qkv_bias = blk.qkv.bias; p.q = q; p.k = k; p.v = v;
        p.rel_table = blk.rel_table; p.bias = bias; p.scale = 1.0f / sqrtf(32.0f);          // head_dim^-0.5 (swin.rs:134)
        p.y = y; p.att = att; p.ld_att = C;
        const double tok_bytes = (double)slots * N * C;
        {
            Bracket b(c, FAM_ELEMENTWISE, 0.0, (double)c.esz() * 3.0 * B * H * W * C + 4.0 * 3.0 * tok_bytes, slots * N, 3 * C, shift);
            BRN_LAUNCH(launch_window_pack(p, c.stream));
        }
        {
            Bracket b(c, FAM_ELEMENTWISE, 0.0, 4.0 * (double)n_pat * slab, n_pat * heads * N, N, shift);
            BRN_LAUNCH(launch_window_bias_build(p, c.stream));
        }
        FlashAttentionParams f{};
        f.heads = heads; f.kv_heads = heads; f.seq_q = N; f.seq_kv = N; f.head_dim = 32;
        f.q_ss = 32; f.q_sh = (long)N * 32; f.q_sb = (long)heads * f.q_sh;                    // BHSD
        f.kv_ss = f.q_ss; f.kv_sh = f.q_sh; f.kv_sb = f.q_sb;
        f.scale = p.scale; f.s16 = c.bf16;
        f.b_sh = (long)N * N; f.b_sp = (long)heads * f.b_sh;
        auto flash = [&](int first_slot, int nslots, const float* patterns, int n_bias) {
            if (nslots < 1) return;
            const size_t o = (size_t)first_slot * per_slot;
            f.q = q + o; f.k = k + o; f.v = v + o; f.y = y + o; f.batch = nslots; f.bias = patterns; f.n_bias = n_bias;
            Bracket b(c, FAM_ATTENTION, (double)nslots * heads * 2.0 * 2.0 * N * (double)N * 32, 4.0 * (4.0 * nslots * (double)per_slot + (double)n_bias * slab), nslots * N, C, shift);
            BRN_LAUNCH(launch_flash_attention(f, c.stream));
        };
        if (shift == 0) flash(0, slots, bias, 1);
        else {
            const int first_border = wgen_first_border_slot(g);
            flash(0, first_border, bias, 1);
            flash(first_border, slots - first_border, bias + (size_t)wgen_plain_patterns(g) * slab, g.n_border);
        }
        {
            Bracket b(c, FAM_ELEMENTWISE, 0.0, (4.0 + (double)c.esz()) * B * H * W * C, B * H * W, C, shift);
            BRN_LAUNCH(launch_window_scatter(p, c.stream));
        }
    }
    c.arena->release(mk);
}

struct Registrar { Registrar() { g_window_generic_route = &window_generic_route; } } registrar;     // runs when the library is loaded

}  // namespace
}  // namespace brn
