// window_generic_geometry.h — the index math of the generic window route (any window side 2 .. 32; kernels/window_generic.hip, its host
// path brn_window_generic.cpp and a stand-alone CPU check, tests/test_window_generic_cpu.py): plain integer arithmetic, no HIP header needed.
//
// The reference pads the [H, W] map with zeros to multiples of the window AFTER norm1 (swin.rs:359-366), rolls the padded canvas by
// -shift (swin.rs:371-377), partitions it into nwh x nww windows of N = ws * ws positions (swin.rs:446-459), and undoes all three after
// the attention (swin.rs:387-401).  Position (i, j) of window (wy, wx) is the canvas position (wy ws + i, wx ws + j) of the ROLLED
// canvas, which holds the padded map's position ((wy ws + i + shift) mod Hp, (wx ws + j + shift) mod Wp): a real token when that is
// inside [0, H) x [0, W), a pad token (q / k / v = the qkv bias, a key like any other) otherwise.
//
// The region mask of a shifted block (swin.rs:603-655) paints the rolled canvas with 3 x 3 regions, slices [0, Lp - ws), [Lp - ws, Lp - shift),
// [Lp - shift, Lp) per axis, and adds -100 to the score of (query, key) whose regions differ.  Only the last window row and the last
// window column reach past Lp - ws: every other window is all region 0 and its mask is zero.  So the windows are numbered ("slots") with
// the INTERIOR windows of all images first, then the BORDER windows as [image][border window]: the interior ones share one bias pattern
// (the relative-position bias), and border slot s reads pattern s mod (nwh + nww - 1) — the bias memory does not grow with the window count.
#pragma once

#if defined(__HIPCC__)
#define BRN_WGEN_HD __host__ __device__ __forceinline__
#else
#define BRN_WGEN_HD inline
#endif

namespace brn {

constexpr int WGEN_MIN_WS = 2, WGEN_MAX_WS = 32;      // window sides of the generic route
constexpr float WGEN_MASK = -100.0f;                  // swin.rs:645 (not -inf: a masked key keeps the weight exp(-100))

struct WgenGeom {
    int B, H, W;          // images, real rows and columns of the token map
    int ws, shift;        // window side; 0 or ws / 2
    int Hp, Wp;           // padded canvas (multiples of ws; never smaller than one window)
    int nwh, nww;         // windows per column / row of the canvas
    int n_int, n_border;  // interior / border windows of ONE image: (nwh - 1)(nww - 1) and nwh + nww - 1
};

BRN_WGEN_HD WgenGeom wgen_geom(int B, int H, int W, int ws, int shift) {
    WgenGeom g;
    g.B = B; g.H = H; g.W = W; g.ws = ws; g.shift = shift;
    g.nwh = (H + ws - 1) / ws; g.nww = (W + ws - 1) / ws;
    g.Hp = g.nwh * ws; g.Wp = g.nww * ws;
    g.n_int = (g.nwh - 1) * (g.nww - 1);
    g.n_border = g.nwh + g.nww - 1;
    return g;
}
BRN_WGEN_HD int wgen_tokens(const WgenGeom& g) { return g.ws * g.ws; }                       // N
BRN_WGEN_HD int wgen_slots(const WgenGeom& g) { return g.B * g.nwh * g.nww; }
BRN_WGEN_HD int wgen_first_border_slot(const WgenGeom& g) { return g.B * g.n_int; }

// border = last window row or last window column; numbered row-major: (wy, nww - 1) for wy < nwh - 1, then the last row's nww windows
BRN_WGEN_HD bool wgen_is_border(const WgenGeom& g, int wy, int wx) { return wy == g.nwh - 1 || wx == g.nww - 1; }
BRN_WGEN_HD int wgen_border_index(const WgenGeom& g, int wy, int wx) { return wy < g.nwh - 1 ? wy : g.nwh - 1 + wx; }
struct WgenWindow { int b, wy, wx; };
BRN_WGEN_HD WgenWindow wgen_border_window(const WgenGeom& g, int j) {
    WgenWindow w; w.b = 0;
    if (j < g.nwh - 1) { w.wy = j; w.wx = g.nww - 1; } else { w.wy = g.nwh - 1; w.wx = j - (g.nwh - 1); }
    return w;
}

// slot <-> (image, wy, wx)
BRN_WGEN_HD int wgen_slot(const WgenGeom& g, int b, int wy, int wx) {
    if (wgen_is_border(g, wy, wx)) return g.B * g.n_int + b * g.n_border + wgen_border_index(g, wy, wx);
    return b * g.n_int + wy * (g.nww - 1) + wx;
}
BRN_WGEN_HD WgenWindow wgen_slot_window(const WgenGeom& g, int slot) {
    const int first = g.B * g.n_int;
    WgenWindow w;
    if (slot >= first) {
        const int l = slot - first, b = l / g.n_border;
        w = wgen_border_window(g, l - b * g.n_border);
        w.b = b;
    } else {
        const int b = slot / g.n_int, r = slot - b * g.n_int;
        w.b = b; w.wy = r / (g.nww - 1); w.wx = r - w.wy * (g.nww - 1);
    }
    return w;
}

// roll(-shift) + pad: the row of the [B, H, W] token matrix that position (i, j) of window (b, wy, wx) holds, -1 = a pad token
BRN_WGEN_HD int wgen_src_token(const WgenGeom& g, int b, int wy, int wx, int i, int j) {
    int sh = wy * g.ws + i + g.shift, sw = wx * g.ws + j + g.shift;
    if (sh >= g.Hp) sh -= g.Hp;
    if (sw >= g.Wp) sw -= g.Wp;
    return (sh < g.H && sw < g.W) ? (b * g.H + sh) * g.W + sw : -1;
}
// window reverse + roll(+shift) + crop: where real token (b, h, w) is computed — its slot and its position t = i ws + j in the window
struct WgenPlace { int slot, t; };
BRN_WGEN_HD WgenPlace wgen_dst_place(const WgenGeom& g, int b, int h, int w) {
    int r = h - g.shift, c = w - g.shift;
    if (r < 0) r += g.Hp;
    if (c < 0) c += g.Wp;
    const int wy = r / g.ws, wx = c / g.ws;
    WgenPlace p;
    p.slot = wgen_slot(g, b, wy, wx);
    p.t = (r - wy * g.ws) * g.ws + (c - wx * g.ws);
    return p;
}

// region id (0 .. 8) of position (i, j) of window (wy, wx) on the rolled canvas (swin.rs:612-632); shift > 0
BRN_WGEN_HD int wgen_axis_region(int x, int Lp, int ws, int shift) { return x < Lp - ws ? 0 : x < Lp - shift ? 1 : 2; }
BRN_WGEN_HD int wgen_region(const WgenGeom& g, int wy, int wx, int i, int j) {
    return wgen_axis_region(wy * g.ws + i, g.Hp, g.ws, g.shift) * 3 + wgen_axis_region(wx * g.ws + j, g.Wp, g.ws, g.shift);
}

// the bias patterns one block builds: the relative-position bias alone (pattern 0; every window of an unshifted block, the interior
// windows of a shifted one) and, for a shifted block, one per border window with its region mask
BRN_WGEN_HD int wgen_plain_patterns(const WgenGeom& g) { return (g.shift == 0 || g.n_int > 0) ? 1 : 0; }
BRN_WGEN_HD int wgen_bias_patterns(const WgenGeom& g) { return wgen_plain_patterns(g) + (g.shift > 0 ? g.n_border : 0); }

}  // namespace brn
