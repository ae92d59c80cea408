// Stand-alone check of csrc/kernels/window_geometry.h (built and run by tests/test_attention_geometry_cpu.py under ASan / UBSan): the
// packed query slots of a window against a brute-force restatement of the kernels' tok_src, and the dispatch order of a launch.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "kernels/window_geometry.h"

using namespace brn;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails <= 20) { std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int roundup12(int x) { return (x + 11) / 12 * 12; }

// window_attention.hip, tok_src: source row of window token t (roll + partition), -1 = pad token
static int tok_src(int b, int wr, int wc, int t, int shift, int H, int W, int Hp, int Wp) {
    const int ti = t / 12, tj = t - ti * 12;
    int sh = wr * 12 + ti + shift, sw = wc * 12 + tj + shift;
    if (sh >= Hp) sh -= Hp;
    if (sw >= Wp) sw -= Wp;
    return (sh < H && sw < W) ? (b * H + sh) * W + sw : -1;
}

// every window of one geometry: slots <-> real tokens; returns the packed tile total of one image
static int check_windows(int H, int W, int shift) {
    const int Hp = roundup12(H), Wp = roundup12(W);
    int tiles = 0;
    for (int wr = 0; wr < Hp / 12; ++wr)
        for (int wc = 0; wc < Wp / 12; ++wc) {
            std::set<int> real;
            for (int t = 0; t < 144; ++t) if (tok_src(0, wr, wc, t, shift, H, W, Hp, Wp) >= 0) real.insert(t);
            const WindowReal g = window_real(wr, wc, shift, H, W, Hp, Wp, true);
            CHECK(g.nq == (int)real.size() && g.nq >= 1, "H %d W %d shift %d window (%d, %d): nq %d, brute force %zu", H, W, shift, wr, wc, g.nq, real.size());
            std::set<int> got;
            int prev = -1;
            for (int s = 0; s < g.nq; ++s) {
                const int t = slot_token(g, s);
                CHECK(t >= 0 && t < 144 && real.count(t) == 1, "H %d W %d shift %d window (%d, %d): slot %d -> token %d is not real", H, W, shift, wr, wc, s, t);
                CHECK(t > prev, "H %d W %d shift %d window (%d, %d): slot %d -> token %d not row-major", H, W, shift, wr, wc, s, t);
                prev = t;
                got.insert(t);
            }
            CHECK(got == real, "H %d W %d shift %d window (%d, %d): slots are not a bijection onto the real tokens", H, W, shift, wr, wc);
            tiles += window_tiles(g);
            // unpacked: slot == token, all nine tiles
            const WindowReal u = window_real(wr, wc, shift, H, W, Hp, Wp, false);
            CHECK(u.nq == 144 && window_tiles(u) == 9, "unpacked nq %d", u.nq);
            for (int s = 0; s < 144; ++s) CHECK(slot_token(u, s) == s, "unpacked slot %d -> %d", s, slot_token(u, s));
        }
    return tiles;
}

// the order of a launch over ngeom geometries: a permutation of all windows, tile counts non-increasing (identity when nothing is padded)
static void check_order(const WindowGeom* g, int ngeom, bool reorder) {
    WindowOrder o;
    build_window_order(g, ngeom, true, reorder, o);
    bool padded = false;
    int total = 0;
    for (int k = 0; k < ngeom; ++k) { padded = padded || g[k].Hp != g[k].H || g[k].Wp != g[k].W; total += g[k].B * (g[k].Hp / 12) * (g[k].Wp / 12); }
    CHECK(o.pack == (padded ? 1 : 0) && o.heads_inner == (padded && reorder ? 1 : 0), "pack %d heads_inner %d padded %d", o.pack, o.heads_inner, (int)padded);
    CHECK(o.ncls >= 1 && o.ncls <= WG_MAX_CLS && o.start[0] == 0, "ncls %d", o.ncls);
    std::set<std::tuple<int, int, int, int>> seen;
    int prev_tiles = 1 << 30;
    for (int flat = 0; flat < total; ++flat) {
        const WindowId id = order_window(o, flat);
        CHECK(id.geom >= 0 && id.geom < ngeom, "geom %d", id.geom);
        if (id.geom < 0 || id.geom >= ngeom) continue;
        const WindowGeom& q = g[id.geom];
        CHECK(id.b >= 0 && id.b < q.B && id.wr >= 0 && id.wr < q.Hp / 12 && id.wc >= 0 && id.wc < q.Wp / 12, "flat %d -> (%d, %d, %d, %d) outside the launch", flat, id.geom, id.b, id.wr, id.wc);
        CHECK(seen.insert(std::make_tuple(id.geom, id.b, id.wr, id.wc)).second, "flat %d -> (%d, %d, %d, %d) twice", flat, id.geom, id.b, id.wr, id.wc);
        if (o.heads_inner) {
            const int tiles = window_tiles(window_real(id.wr, id.wc, q.shift, q.H, q.W, q.Hp, q.Wp, true));
            CHECK(tiles <= prev_tiles, "H %d W %d shift %d flat %d: %d tiles after %d", g[0].H, g[0].W, g[0].shift, flat, tiles, prev_tiles);
            prev_tiles = tiles;
        } else {
            // the order before: geometry 0's windows (b, wr, wc) row-major, then geometry 1's
            const int n0 = g[0].B * (g[0].Hp / 12) * (g[0].Wp / 12);
            const int k = flat >= n0 ? 1 : 0, bw = flat - k * n0, nWw = g[k].Wp / 12, nW = (g[k].Hp / 12) * nWw;
            CHECK(id.geom == k && id.b == bw / nW && id.wr == (bw % nW) / nWw && id.wc == (bw % nW) % nWw, "identity order: flat %d -> (%d, %d, %d, %d)", flat, id.geom, id.b, id.wr, id.wc);
        }
    }
    CHECK((int)seen.size() == total, "%zu windows of %d", seen.size(), total);
    // pack off: identity, all positions
    WindowOrder z;
    build_window_order(g, ngeom, false, true, z);
    CHECK(z.pack == 0 && z.heads_inner == 0 && z.ncls == ngeom, "pack off: pack %d heads_inner %d ncls %d", z.pack, z.heads_inner, z.ncls);
}

int main() {
    for (int shift = 0; shift <= 6; shift += 6)
        for (int H = 1; H <= 40; ++H)
            for (int W = 1; W <= 40; ++W) {
                check_windows(H, W, shift);
                // one geometry, and with its half-scale map in the same launch (two images each)
                const WindowGeom g[2] = {{2, H, W, roundup12(H), roundup12(W), shift}, {2, (H + 1) / 2, (W + 1) / 2, roundup12((H + 1) / 2), roundup12((W + 1) / 2), shift}};
                check_order(g, 1, true);
                check_order(g, 2, true);
                check_order(g, 2, false);
            }
    // the four stage geometries of a 1024 x 1024 image and its half-scale pass (token maps 256, 128, 64, 32 and half of each)
    for (int st = 0; st < 4; ++st)
        for (int shift = 0; shift <= 6; shift += 6) {
            const int a = 256 >> st, b = 128 >> st;
            const WindowGeom g[2] = {{1, a, a, roundup12(a), roundup12(a), shift}, {1, b, b, roundup12(b), roundup12(b), shift}};
            check_order(g, 2, true);
            const int nwin = (g[0].Hp / 12) * (g[0].Wp / 12) + (g[1].Hp / 12) * (g[1].Wp / 12);
            std::printf("stage %d shift %d windows %d tiles_all %d tiles_packed %d\n", st, shift, nwin, nwin * 9, check_windows(a, a, shift) + check_windows(b, b, shift));
        }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
