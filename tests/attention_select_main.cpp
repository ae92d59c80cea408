// Stand-alone check of csrc/kernels/window_attention_select.h (built and run by tests/test_attention_select_cpu.py under ASan / UBSan):
// select_window_attention against the nested launcher decision it replaced, restated here as it stood, over a full product of parameters.
#include <cstdio>
#include <initializer_list>

#include "kernels/window_attention_select.h"

using namespace brn;

// the fields of WindowAttnParams (brn_kernels.h) that the decision reads
struct Params {
    int B, H, W, C, heads, Hp, Wp, shift, planes, out_planes, h2;
    float out_h2;
    int ws, io_bf16;
};
struct Decision {
    bool valid;
    AttKernel kernel;
    int gx, gy, block, n0;
};
struct dim3 { int x, y; dim3(int x_, int y_ = 1) : x(x_), y(y_) {} };

// ---- the launcher as it was (kernels/window_attention.hip before the selector): hipLaunchKernelGGL replaced by LAUNCH, which records ----
enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1 };
constexpr int WS = 12, HD = 32;
#define LAUNCH(kernel_id, grid_, block_) (d.valid = true, d.kernel = kernel_id, d.gx = (grid_).x, d.gy = (grid_).y, d.block = (block_).x, d.n0 = n0)

static hipError_t check_attention(const Params& p) {
    const int ws = p.ws ? p.ws : WS;
    if (!(ws == 12 || ws == 7)) return hipErrorInvalidValue;
    if (p.C != p.heads * HD || p.Hp % ws || p.Wp % ws || p.Hp < p.H || p.Wp < p.W) return hipErrorInvalidValue;
    if (!(p.shift == 0 || p.shift == ws / 2)) return hipErrorInvalidValue;
    if (ws != WS && (p.planes || p.out_planes)) return hipErrorInvalidValue;
    return hipSuccess;
}
static hipError_t old_launch(const Params& p, const Params* p2, bool two_heads, int f32_waves, bool diag_build, Decision& d) {
    d = Decision{false, ATT_INVALID, 0, 0, 0, 0};
    if (check_attention(p) != hipSuccess) return hipErrorInvalidValue;
    const int ws = p.ws ? p.ws : WS;
    const int n0 = p.B * (p.Hp / ws) * (p.Wp / ws);
    int n1 = 0;
    if (p2) {
        if ((p2->ws ? p2->ws : WS) != ws) return hipErrorInvalidValue;
        if (check_attention(*p2) != hipSuccess || p2->C != p.C || p2->heads != p.heads || p2->planes != p.planes || p2->out_planes != p.out_planes || p2->io_bf16 != p.io_bf16) return hipErrorInvalidValue;
        n1 = p2->B * (p2->Hp / ws) * (p2->Wp / ws);
    }
    if (p.out_planes && !((p.out_planes == 2 && p.planes == 2 && (p.out_h2 > 0.f) == (p.h2 != 0)) || (p.out_planes == 3 && p.planes == 0) || (p.out_planes == 2 && p.planes == 0 && p.out_h2 > 0.f && !p.io_bf16)))
        return hipErrorInvalidValue;
    if (p.h2 && (p.planes != 2 || p.io_bf16)) return hipErrorInvalidValue;
    if (p2 && (p2->out_h2 != p.out_h2 || p2->h2 != p.h2)) return hipErrorInvalidValue;
    dim3 grid(n0 + n1, p.heads), block(ATT_THREADS);
    if (p.io_bf16 && ws == 7) {
        if (p.out_planes || (p.C & 3)) return hipErrorInvalidValue;
        if (p.io_bf16 == 2) LAUNCH(ATT_F32_W7_F16, grid, block);
        else LAUNCH(ATT_F32_W7_BF16, grid, block);
    } else if (p.io_bf16) {
        if (p.out_planes || (p.C & 7)) return hipErrorInvalidValue;
        if (p.io_bf16 == 2) {
            if (two_heads && !(p.heads & 1)) LAUNCH(ATT_F16_2, dim3(n0 + n1, p.heads / 2), dim3(2 * ATT_THREADS));
            else LAUNCH(ATT_F16_1, grid, block);
        } else if (two_heads && !(p.heads & 1)) LAUNCH(ATT_BF16_2, dim3(n0 + n1, p.heads / 2), dim3(2 * ATT_THREADS));
        else LAUNCH(ATT_BF16_1, grid, block);
    } else if (p.planes == 2 && p.h2) LAUNCH(ATT_SPLIT2_H, grid, block);
    else if (p.planes == 2) LAUNCH(ATT_SPLIT2, grid, block);
    else if (p.planes == 1 && diag_build) LAUNCH(ATT_SPLIT1, grid, block);        // (was #ifdef BRN_DIAG_BUILD)
    else if (p.planes == 1) return hipErrorInvalidValue;
    else if (ws == 7) LAUNCH(ATT_F32_W7, grid, block);
    else {
        if (f32_waves == 9) LAUNCH(ATT_F32_W12_9, grid, dim3(9 * 64));
        else LAUNCH(ATT_F32_W12_3, grid, block);
    }
    return hipSuccess;
}

static long n_valid = 0, n_invalid = 0, fails = 0;

static void compare(const Params& p, const Params* p2, int hpw, int f32_waves, bool diag) {
    Decision d;
    const hipError_t e = old_launch(p, p2, hpw != 1, f32_waves, diag, d);
    const AttLaunch l = select_window_attention(p, p2, hpw, f32_waves, diag);
    const bool same = d.valid ? (e == hipSuccess && l.kernel == d.kernel && l.grid_x == d.gx && l.grid_y == d.gy && l.block == d.block && l.nblk0 == d.n0)
                              : (e == hipErrorInvalidValue && l.kernel == ATT_INVALID);
    if (d.valid) ++n_valid; else ++n_invalid;
    if (!same && ++fails <= 20)
        std::printf("FAIL ws %d planes %d out_planes %d h2 %d out_h2 %g io %d C %d heads %d shift %d second %d hpw %d waves %d diag %d: old %d kernel %d (%d, %d) x %d n0 %d, new kernel %d (%d, %d) x %d n0 %d\n",
                    p.ws, p.planes, p.out_planes, p.h2, (double)p.out_h2, p.io_bf16, p.C, p.heads, p.shift, p2 ? 1 : 0, hpw, f32_waves, (int)diag,
                    (int)d.valid, (int)d.kernel, d.gx, d.gy, d.block, d.n0, (int)l.kernel, l.grid_x, l.grid_y, l.block, l.nblk0);
}

int main() {
    const int C_heads[][2] = {{64, 2}, {68, 2}, {60, 1}, {64, 3}, {96, 3}, {32, 1}};      // C / 32 heads, one inconsistent pair, odd and even head counts
    for (int ws : {0, 7, 12, 8})
    for (int planes : {0, 1, 2})
    for (int out_planes : {0, 2, 3})
    for (int h2 : {0, 1})
    for (float out_h2 : {0.f, 256.f})
    for (int io : {0, 1, 2})
    for (const auto& ch : C_heads)
    for (int si = 0; si < 3; ++si)
    for (int hpw : {1, 2})
    for (int waves : {3, 9})
    for (int diag = 0; diag < 2; ++diag) {
        const int wse = ws ? ws : 12;
        Params p = {1, 18, 18, ch[0], ch[1], (18 + wse - 1) / wse * wse, (18 + wse - 1) / wse * wse, si == 0 ? 0 : si == 1 ? wse / 2 : 1, planes, out_planes, h2, out_h2, ws, io};
        compare(p, nullptr, hpw, waves, diag != 0);
        Params q = p;                                      // the half-scale map of the same stage
        q.B = 2; q.H = q.W = 9; q.Hp = q.Wp = wse;
        compare(p, &q, hpw, waves, diag != 0);
        compare(p, &p, hpw, waves, diag != 0);
        for (int f = 0; f < 9; ++f) {                       // the second map differs in one field that the launcher compares or checks
            Params r = q;
            switch (f) {
            case 0: r.ws = wse == 12 ? 7 : 12; break;
            case 1: r.C += 32; r.heads += 1; break;
            case 2: r.heads += 1; break;
            case 3: r.planes = (r.planes + 1) % 3; break;
            case 4: r.out_planes = r.out_planes == 2 ? 3 : 2; break;
            case 5: r.io_bf16 = (r.io_bf16 + 1) % 3; break;
            case 6: r.out_h2 = r.out_h2 > 0.f ? 0.f : 256.f; break;
            case 7: r.h2 = !r.h2; break;
            default: r.Hp += 1; break;                     // its own geometry check
            }
            compare(p, &r, hpw, waves, diag != 0);
        }
    }
    std::printf("valid %ld invalid %ld\n", n_valid, n_invalid);
    if (fails) std::printf("FAILED %ld\n", fails);
    else std::printf("ok\n");
    return fails ? 1 : 0;
}
