// Stand-alone check of csrc/kernels/window_generic_geometry.h (built and run by tests/test_window_generic_cpu.py under ASan / UBSan): the
// slot order, the interior / border split, the region mask of every window and the token round trip of the generic window route, each
// against a brute-force restatement of the reference's tensors (swin.rs:359-401, 603-655).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "kernels/window_generic_geometry.h"

using namespace brn;

static int fails = 0;
static long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { if (++fails <= 20) { std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// create_attention_mask's region image (swin.rs:612-632) on the padded canvas: three slices per axis, painted in order
static std::vector<int> region_image(int Hp, int Wp, int ws, int shift) {
    std::vector<int> img((size_t)Hp * Wp, 0);
    const int hs[3][2] = {{0, Hp - ws}, {Hp - ws, Hp - shift}, {Hp - shift, Hp}};
    const int wsl[3][2] = {{0, Wp - ws}, {Wp - ws, Wp - shift}, {Wp - shift, Wp}};
    int cnt = 0;
    for (auto& a : hs)
        for (auto& b : wsl) {
            for (int i = a[0]; i < a[1]; ++i) for (int j = b[0]; j < b[1]; ++j) img[(size_t)i * Wp + j] = cnt;
            ++cnt;
        }
    return img;
}

static void check_case(int B, int H, int W, int ws, int shift) {
    const WgenGeom g = wgen_geom(B, H, W, ws, shift);
    const int N = ws * ws, slots = wgen_slots(g);
#define WHERE "B %d H %d W %d ws %d shift %d", B, H, W, ws, shift
    CHECK(g.Hp % ws == 0 && g.Wp % ws == 0 && g.Hp >= H && g.Hp - H < ws && g.Wp >= W && g.Wp - W < ws && g.Hp >= ws && g.Wp >= ws, WHERE);
    CHECK(g.nwh == g.Hp / ws && g.nww == g.Wp / ws && g.n_int + g.n_border == g.nwh * g.nww && wgen_tokens(g) == N, WHERE);
    // (a) slot <-> (image, wy, wx) is a bijection and its inverse agrees; (b) interior slots first, border = last window row or column
    std::vector<int> seen((size_t)slots, 0);
    const int first_border = wgen_first_border_slot(g);
    for (int b = 0; b < B; ++b)
        for (int wy = 0; wy < g.nwh; ++wy)
            for (int wx = 0; wx < g.nww; ++wx) {
                const int s = wgen_slot(g, b, wy, wx);
                CHECK(s >= 0 && s < slots, WHERE);
                if (s < 0 || s >= slots) continue;
                ++seen[(size_t)s];
                const WgenWindow w = wgen_slot_window(g, s);
                CHECK(w.b == b && w.wy == wy && w.wx == wx, WHERE);
                const bool border = wy == g.nwh - 1 || wx == g.nww - 1;
                CHECK(wgen_is_border(g, wy, wx) == border && (s >= first_border) == border, WHERE);
                if (border) {
                    const int j = wgen_border_index(g, wy, wx);
                    const WgenWindow bw = wgen_border_window(g, j);
                    CHECK(j >= 0 && j < g.n_border && bw.wy == wy && bw.wx == wx, WHERE);
                    // the flash kernel's pattern of this slot: (slot - first border slot) mod n_border
                    CHECK((s - first_border) % g.n_border == j && (s - first_border) / g.n_border == b, WHERE);
                }
            }
    for (int s = 0; s < slots; ++s) CHECK(seen[(size_t)s] == 1, WHERE);
    CHECK(first_border == B * g.n_int && slots - first_border == B * g.n_border, WHERE);
    CHECK(wgen_plain_patterns(g) == ((shift == 0 || g.n_int > 0) ? 1 : 0) && wgen_bias_patterns(g) == wgen_plain_patterns(g) + (shift ? g.n_border : 0), WHERE);
    // (c) the mask of every window against the region image: interior windows all zero, border patterns equal
    // (the mask is a function of the canvas alone: Hp, Wp, ws, shift — compared once per canvas, not once per B, H, W that pad to it)
    static std::set<std::tuple<int, int, int, int>> canvases;
    if (shift > 0 && canvases.insert(std::make_tuple(g.Hp, g.Wp, ws, shift)).second) {
        const std::vector<int> img = region_image(g.Hp, g.Wp, ws, shift);
        for (int wy = 0; wy < g.nwh; ++wy)
            for (int wx = 0; wx < g.nww; ++wx) {
                const bool border = wgen_is_border(g, wy, wx);
                // the window's cut of the image (window_partition) and the header's region ids, then mask[q][k] = ids differ, both ways
                std::vector<int> cut((size_t)N), ids((size_t)N);
                for (int t = 0; t < N; ++t) {
                    cut[(size_t)t] = img[(size_t)(wy * ws + t / ws) * g.Wp + wx * ws + t % ws];
                    ids[(size_t)t] = wgen_region(g, wy, wx, t / ws, t % ws);
                }
                bool any = false, agree = true;
                for (int qt = 0; qt < N; ++qt)
                    for (int kt = 0; kt < N; ++kt) {
                        const bool brute = cut[(size_t)qt] != cut[(size_t)kt];
                        any = any || brute;
                        if (border) agree = agree && brute == (ids[(size_t)qt] != ids[(size_t)kt]);
                    }
                CHECK(border || !any, WHERE);
                CHECK(agree, WHERE);
            }
    }
    // (d) source (roll + pad) and destination (un-roll + crop) indices: every real token is read by exactly one window position, and
    // its output is taken from that very position; every other position is a pad token
    std::vector<int> reads((size_t)B * H * W, 0);
    long pads = 0;
    for (int s = 0; s < slots; ++s) {
        const WgenWindow w = wgen_slot_window(g, s);
        for (int t = 0; t < N; ++t) {
            const int src = wgen_src_token(g, w.b, w.wy, w.wx, t / ws, t % ws);
            CHECK(src >= -1 && src < B * H * W, WHERE);
            if (src < 0) { ++pads; continue; }
            if (src >= B * H * W) continue;
            ++reads[(size_t)src];
            // brute force: the padded canvas rolled by -shift holds padded[(r + shift) mod Hp]
            const int r = (w.wy * ws + t / ws + shift) % g.Hp, cc = (w.wx * ws + t % ws + shift) % g.Wp;
            CHECK(r < H && cc < W && src == (w.b * H + r) * W + cc, WHERE);
            const WgenPlace p = wgen_dst_place(g, w.b, r, cc);
            CHECK(p.slot == s && p.t == t, WHERE);
        }
    }
    for (size_t i = 0; i < reads.size(); ++i) CHECK(reads[i] == 1, WHERE);
    CHECK(pads == (long)B * (g.Hp * g.Wp - H * W), WHERE);
#undef WHERE
}

int main() {
    const int sides[] = {2, 3, 5, 8, 16, 24, 32};
    const int images[] = {1, 3};
    int cases = 0;
    for (int ws : sides)
        for (int sh = 0; sh < 2; ++sh)
            for (int nwh = 1; nwh <= 4; ++nwh)
                for (int nww = 1; nww <= 5; ++nww)
                    for (int B : images) {
                        // ragged maps of nwh x nww windows: full, one short, one past the previous window, and (one window) a single row / column
                        const int hs[] = {nwh * ws, nwh * ws - 1, (nwh - 1) * ws + 1}, wsz[] = {nww * ws, nww * ws - (ws > 2 ? 2 : 1), (nww - 1) * ws + 1};
                        for (int H : hs)
                            for (int W : wsz) { check_case(B, H, W, ws, sh ? ws / 2 : 0); ++cases; }
                    }
    std::printf("cases %d checks %ld\n", cases, checks);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
