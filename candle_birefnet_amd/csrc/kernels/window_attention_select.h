// window_attention_select.h — which window attention kernel a launch runs, with which grid and block, or that the parameters are invalid.
// Plain host arithmetic on the fields of WindowAttnParams (brn_kernels.h), no HIP header needed: the launcher (kernels/window_attention.hip)
// switches over the result, and a stand-alone CPU check (tests/test_attention_select_cpu.py) compares it with the nested form it replaced.
// P = WindowAttnParams, or any struct with the same fields.
#pragma once

namespace brn {

constexpr int ATT_THREADS = 192;   // 3 waves, 3 query tiles each

enum AttKernel {
    ATT_INVALID = 0,
    ATT_F32_W7, ATT_F32_W7_BF16, ATT_F32_W7_F16,          // window_attention_f32_kernel<7, 3, 0 / 1 / 2>
    ATT_F32_W12_9, ATT_F32_W12_3,                         // window_attention_f32_kernel<12, 9 / 3>
    ATT_SPLIT2, ATT_SPLIT2_H, ATT_SPLIT1,                 // window_attention_split_kernel<2>, <2, true>, <1> (diag build)
    ATT_BF16_1, ATT_BF16_2, ATT_F16_1, ATT_F16_2          // window_attention_bf16_kernel<heads per workgroup, fp16 storage>
};
struct AttLaunch {
    AttKernel kernel;
    int grid_x, grid_y, block;     // grid_x = windows of both maps, grid_y = heads or head pairs
    int nblk0;                     // windows of the first map
};

template <class P>
inline bool att_geometry_ok(const P& p, int ws) {
    const bool whole_heads = p.C == p.heads * 32;
    const bool canvas_is_whole_windows = p.Hp % ws == 0 && p.Wp % ws == 0;
    const bool canvas_covers_map = p.Hp >= p.H && p.Wp >= p.W;
    const bool shift_is_none_or_half = p.shift == 0 || p.shift == ws / 2;
    const bool window7_is_fp32_only = ws == 12 || !(p.planes || p.out_planes);     // Swin-T / S: the fp32-MFMA kernel (fp32 or 16-bit matrices in / out)
    return whole_heads && canvas_is_whole_windows && canvas_covers_map && shift_is_none_or_half && window7_is_fp32_only;
}

// hpw, f32_waves: the values of BRN_ATT_HPW (default 2) and BRN_ATT_F32_WAVES (default 9); p2: the second map of the launch, or null
template <class P>
inline AttLaunch select_window_attention(const P& p, const P* p2, int hpw, int f32_waves, bool diag) {
    const AttLaunch invalid = {ATT_INVALID, 0, 0, 0, 0};
    const int ws = p.ws ? p.ws : 12;
    const P& q = p2 ? *p2 : p;
    const bool window_is_12_or_7 = ws == 12 || ws == 7;
    if (!window_is_12_or_7 || !att_geometry_ok(p, ws)) return invalid;
    const bool same_window = (q.ws ? q.ws : 12) == ws;
    if (!same_window || !att_geometry_ok(q, ws)) return invalid;
    const bool maps_agree = !p2 || (q.C == p.C && q.heads == p.heads && q.planes == p.planes && q.out_planes == p.out_planes && q.io_bf16 == p.io_bf16
                                    && q.out_h2 == p.out_h2 && q.h2 == p.h2);
    const bool out_planes_match_split_kernel = p.out_planes == 2 && p.planes == 2 && (p.out_h2 > 0.f) == (p.h2 != 0);
    const bool out_three_planes_from_fp32_kernel = p.out_planes == 3 && p.planes == 0;
    const bool out_fp16_planes_from_fp32_kernel = p.out_planes == 2 && p.planes == 0 && p.out_h2 > 0.f && !p.io_bf16;
    const bool out_form_has_a_kernel = !p.out_planes || out_planes_match_split_kernel || out_three_planes_from_fp32_kernel || out_fp16_planes_from_fp32_kernel;
    const bool fp16_planes_need_two_plane_kernel_and_fp32_matrices = !p.h2 || (p.planes == 2 && !p.io_bf16);
    if (!maps_agree || !out_form_has_a_kernel || !fp16_planes_need_two_plane_kernel_and_fp32_matrices) return invalid;

    const int n0 = p.B * (p.Hp / ws) * (p.Wp / ws), n1 = p2 ? q.B * (q.Hp / ws) * (q.Wp / ws) : 0;
    AttLaunch l = {ATT_INVALID, n0 + n1, p.heads, ATT_THREADS, n0};
    if (p.io_bf16) {                                       // 16-bit matrices in and out: 1 = bf16, 2 = fp16
        const bool fp16 = p.io_bf16 == 2;
        const bool rows_are_whole_vectors = (p.C & (ws == 7 ? 3 : 7)) == 0;
        if (p.out_planes || !rows_are_whole_vectors) return invalid;
        if (ws == 7) l.kernel = fp16 ? ATT_F32_W7_F16 : ATT_F32_W7_BF16;
        else if (hpw != 1 && !(p.heads & 1)) {             // two heads per workgroup: whole 128-byte lines of K and V
            l.kernel = fp16 ? ATT_F16_2 : ATT_BF16_2;
            l.grid_y = p.heads / 2;
            l.block = 2 * ATT_THREADS;
        } else l.kernel = fp16 ? ATT_F16_1 : ATT_BF16_1;
    } else if (p.planes == 2) l.kernel = p.h2 ? ATT_SPLIT2_H : ATT_SPLIT2;
    else if (p.planes == 1) l.kernel = diag ? ATT_SPLIT1 : ATT_INVALID;      // mode bf16_operands: diag build only
    else if (ws == 7) l.kernel = ATT_F32_W7;
    else if (f32_waves == 9) { l.kernel = ATT_F32_W12_9; l.block = 9 * 64; }
    else l.kernel = ATT_F32_W12_3;
    return l;
}

}  // namespace brn
