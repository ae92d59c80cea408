// window_geometry.h — which tokens of a 12 x 12 (shifted) window are real, and the order in which a launch visits its windows.  Shared by
// the attention kernels (kernels/window_attention.hip), their host launcher and a stand-alone CPU check (tests/test_attention_geometry_cpu.py):
// plain integer arithmetic, no HIP header needed.
//
// The reference pads the map to multiples of the window (swin.rs:359-366), rolls it by -shift (swin.rs:371-377), partitions it, and crops
// the pad rows again after the window reverse: a pad token is a KEY of its window (its k / v is the qkv bias) but its QUERY row never
// reaches the output.  The real tokens of a window are a product set (rows) x (columns); per axis the window covers the canvas
// positions s .. s + 11, s = 12 w + shift < Lp, taken mod Lp, and position x is real when x mod Lp < L.  Lp - L < 12, so the real ones are
//   [s, min(s + 12, L))  and  [max(s, Lp), min(s + 12, Lp + L))        (either may be empty, never both)
// i.e. in window coordinates [0, split) and [split + gap, n + gap): the k-th real coordinate is k + (k >= split ? gap : 0).
#pragma once
#include <climits>

#if defined(__HIPCC__)
#define BRN_WG_HD __host__ __device__ __forceinline__
#else
#define BRN_WG_HD inline
#endif

namespace brn {

constexpr int WG_WS = 12;                       // window side of the kernels that use this header (Swin-B / L)
constexpr int WG_NTOK = WG_WS * WG_WS;

BRN_WG_HD int wg_min(int a, int b) { return a < b ? a : b; }
BRN_WG_HD int wg_max(int a, int b) { return a > b ? a : b; }

struct AxisReal { int n, split, gap; };         // n real coordinates of 12: [0, split) and [split + gap, n + gap)

// window w of an axis of L real positions on a canvas of Lp (a multiple of 12, Lp - L < 12), rolled by shift (0 .. 11)
BRN_WG_HD AxisReal axis_real(int w, int shift, int L, int Lp) {
    const int s = w * WG_WS + shift;
    const int n1 = wg_max(0, wg_min(s + WG_WS, L) - s);
    const int lo2 = wg_max(s, Lp);
    const int n2 = wg_max(0, wg_min(s + WG_WS, Lp + L) - lo2);
    AxisReal a;
    a.n = n1 + n2; a.split = n1; a.gap = n2 > 0 ? lo2 - s - n1 : 0;
    return a;
}
BRN_WG_HD int axis_coord(const AxisReal& a, int k) { return k + (k >= a.split ? a.gap : 0); }

// the real tokens of one window, numbered row-major over (real rows) x (real columns): query slots 0 .. nq - 1
struct WindowReal {
    AxisReal r, c;
    int nq;          // 1 .. 144
    int cdiv;        // ceil(2^16 / c.n): slot / c.n == (slot * cdiv) >> 16 for slot < 144
};
// pack = false: every position of the window is a slot (slot == token, nq == 144): the order before queries were packed
BRN_WG_HD WindowReal window_real(int wr, int wc, int shift, int H, int W, int Hp, int Wp, bool pack) {
    WindowReal g;
    if (pack) { g.r = axis_real(wr, shift, H, Hp); g.c = axis_real(wc, shift, W, Wp); }
    else { g.r.n = WG_WS; g.r.split = WG_WS; g.r.gap = 0; g.c = g.r; }
    g.nq = g.r.n * g.c.n;
    g.cdiv = (65536 + g.c.n - 1) / g.c.n;
    return g;
}
BRN_WG_HD int window_tiles(const WindowReal& g) { return (g.nq + 15) >> 4; }      // 16-query tiles
// window token (ti * 12 + tj) of query slot 0 <= slot < nq
BRN_WG_HD int slot_token(const WindowReal& g, int slot) {
    const int q = (slot * g.cdiv) >> 16, r = slot - q * g.c.n;
    return axis_coord(g.r, q) * WG_WS + axis_coord(g.c, r);
}

// ---- dispatch order of a launch over one or two geometries: windows with more query tiles first, so that the workgroups which do not
// fit the first round of CU slots are the short ones.  Along an axis, windows with the same real count are consecutive (interior
// windows, then at most two border ones), so the windows of a launch fall into a few CLASSES = (geometry, run of window rows, run of
// window columns, all images), every window of a class with the same tile count.  The host sorts the classes by tile count and hands
// the kernel their first flat index; the kernel finds its class by comparison and its window by two divisions — no table in memory.
constexpr int WG_MAX_CLS = 18;                  // 2 geometries x 3 row runs x 3 column runs
struct WindowClass { int geom, wr0, nwr, wc0, nwc, tiles; };
struct WindowOrder {
    int pack;                                   // 1: the kernels run over the real queries of a window only (window_real); 0: over all 144 positions
    int heads_inner;                           // 1: the workgroups of one window (its heads) are adjacent in dispatch order; 0: grid.y = head
    int ncls;
    int start[WG_MAX_CLS];                      // first flat window of class i (in dispatch order); INT_MAX beyond ncls
    WindowClass cls[WG_MAX_CLS];
};
struct WindowId { int geom, b, wr, wc; };
BRN_WG_HD WindowId order_window(const WindowOrder& o, int flat) {
    int ci = 0;
    for (int i = 1; i < WG_MAX_CLS; ++i) ci += (int)((unsigned)(o.start[i] - flat - 1) >> 31);   // flat >= start[i] (0 <= flat, start: no overflow)
    const WindowClass& k = o.cls[ci];
    const int l = flat - o.start[ci], per = k.nwr * k.nwc;
    WindowId id;
    id.geom = k.geom;
    id.b = l / per;
    const int r = l - id.b * per, rr = r / k.nwc;
    id.wr = k.wr0 + rr;
    id.wc = k.wc0 + (r - rr * k.nwc);
    return id;
}

struct WindowGeom { int B, H, W, Hp, Wp, shift; };
// identity: geometry 0's windows (b, wr, wc) row-major, then geometry 1's — one class per geometry
inline void identity_window_order(const WindowGeom* g, int ngeom, WindowOrder& o) {
    o.pack = 0; o.heads_inner = 0; o.ncls = ngeom;
    int at = 0;
    for (int i = 0; i < WG_MAX_CLS; ++i) {
        o.start[i] = INT_MAX;
        o.cls[i] = WindowClass{0, 0, 1, 0, 1, 0};
        if (i < ngeom) {
            o.start[i] = at;
            o.cls[i] = WindowClass{i, 0, g[i].Hp / WG_WS, 0, g[i].Wp / WG_WS, WG_NTOK / 16};
            at += g[i].B * (g[i].Hp / WG_WS) * (g[i].Wp / WG_WS);
        }
    }
}
// pack = false, or no pad token in any geometry: the identity order, all positions; reorder = false: real queries only, identity order
inline void build_window_order(const WindowGeom* g, int ngeom, bool pack, bool reorder, WindowOrder& o) {
    identity_window_order(g, ngeom, o);
    bool padded = false;
    for (int k = 0; k < ngeom; ++k) padded = padded || g[k].Hp != g[k].H || g[k].Wp != g[k].W;
    if (!pack || !padded) return;
    o.pack = 1;
    if (!reorder) return;
    WindowClass cls[WG_MAX_CLS];
    int ncls = 0;
    for (int k = 0; k < ngeom; ++k) {
        const int nWh = g[k].Hp / WG_WS, nWw = g[k].Wp / WG_WS, shift = g[k].shift;
        for (int r0 = 0; r0 < nWh;) {
            const int nr = axis_real(r0, shift, g[k].H, g[k].Hp).n;
            int r1 = r0 + 1;
            while (r1 < nWh && axis_real(r1, shift, g[k].H, g[k].Hp).n == nr) ++r1;
            for (int c0 = 0; c0 < nWw;) {
                const int nc = axis_real(c0, shift, g[k].W, g[k].Wp).n;
                int c1 = c0 + 1;
                while (c1 < nWw && axis_real(c1, shift, g[k].W, g[k].Wp).n == nc) ++c1;
                if (ncls == WG_MAX_CLS) return;               // (cannot happen with Lp - L < 12: at most three runs per axis) identity
                cls[ncls++] = WindowClass{k, r0, r1 - r0, c0, c1 - c0, (nr * nc + 15) >> 4};
                c0 = c1;
            }
            r0 = r1;
        }
    }
    for (int i = 1; i < ncls; ++i) {                          // stable: equal tile counts keep geometry / row-major order
        const WindowClass c = cls[i];
        int j = i;
        for (; j > 0 && cls[j - 1].tiles < c.tiles; --j) cls[j] = cls[j - 1];
        cls[j] = c;
    }
    o.heads_inner = 1; o.ncls = ncls;
    int at = 0;
    for (int i = 0; i < ncls; ++i) {
        o.start[i] = at;
        o.cls[i] = cls[i];
        at += g[cls[i].geom].B * cls[i].nwr * cls[i].nwc;
    }
}

}  // namespace brn
