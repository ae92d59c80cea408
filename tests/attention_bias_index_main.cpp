// Stand-alone check of csrc/kernels/window_attention_index.h (built and run by tests/test_attention_bias_index_cpu.py): the reversed-table
// index the split and bf16 window attention kernels form — one address per 16-key tile, four words from it — against the relative
// position index written out per (query, key) pair, for every pair of a 12 x 12 window; and, with csrc/kernels/window_geometry.h, that
// every query slot a workgroup can form on a padded map (slots past the last real query are clamped to it) stays inside the table.
#include <cstdio>

#include "kernels/window_attention_index.h"
#include "kernels/window_geometry.h"

using namespace brn;

constexpr int WS = 12, NTOK = WS * WS, TABN = (2 * WS - 1) * (2 * WS - 1);

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the index of (query token, key) the kernel reads: lane group g = (key % 16) / 4 of key tile kt = key / 16, register r = key % 4
static int kernel_index(int qtok, int key) {
    const int kt = key / 16, g = (key % 16) / 4, r = key % 4;
    return att_qrev(qtok / WS, qtok % WS) + att_koff(att_key0(kt, g)) + r;
}

int main() {
    static_assert(WS % 4 == 0 && NTOK % 16 == 0, "the four keys of a lane's tile chunk lie in one window row");
    // ---- every (query, key) pair of the window ----
    long pairs = 0;
    int lo = TABN, hi = -1;
    for (int q = 0; q < NTOK; ++q) {
        for (int key = 0; key < NTOK; ++key) {
            const int idx = kernel_index(q, key);
            CHECK(idx >= 0 && idx <= TABN - 1, "q %d key %d index %d", q, key, idx);
            // the plain table index, by att_qbase and spelled out from the token coordinates (swin.rs:182-184)
            const int plain = att_qbase(q / WS, q % WS) - key - (WS - 1) * (key / WS);
            const int spelled = (q / WS - key / WS + WS - 1) * (2 * WS - 1) + (q % WS - key % WS + WS - 1);
            CHECK(plain == spelled, "q %d key %d att_qbase form %d, spelled out %d", q, key, plain, spelled);
            CHECK(idx == TABN - 1 - plain, "q %d key %d index %d, expected %d", q, key, idx, TABN - 1 - plain);
            // the four keys of a chunk lie in one window row
            if (key % 4 == 0) CHECK(key / WS == (key + 3) / WS, "keys %d .. %d span two window rows", key, key + 3);
            lo = idx < lo ? idx : lo;
            hi = idx > hi ? idx : hi;
            ++pairs;
        }
    }
    CHECK(lo == 0 && hi == TABN - 1, "index range %d .. %d", lo, hi);
    std::printf("pairs %ld range %d %d\n", pairs, lo, hi);

    // ---- padded maps: every slot of every tile a workgroup runs, as the kernels form it (slot_token(wg, min(slot, nq - 1))), with
    // packed queries and without, on every map up to 40 x 40 at shift 0 and 6 ----
    long slots = 0, past = 0;
    for (int H = 1; H <= 40; ++H) {
        for (int W = 1; W <= 40; ++W) {
            const int Hp = (H + WS - 1) / WS * WS, Wp = (W + WS - 1) / WS * WS;
            for (int shift = 0; shift <= 6; shift += 6) {
                for (int pack = 0; pack < 2; ++pack) {
                    for (int wr = 0; wr < Hp / WS; ++wr) {
                        for (int wc = 0; wc < Wp / WS; ++wc) {
                            const WindowReal wg = window_real(wr, wc, shift, H, W, Hp, Wp, pack != 0);
                            CHECK(wg.nq >= 1 && wg.nq <= NTOK, "%dx%d shift %d window (%d, %d): nq %d", H, W, shift, wr, wc, wg.nq);
                            const int ntile = window_tiles(wg);
                            // waves 0 .. 2 start at tile = wave whether or not they have one, and fetch one tile ahead: slots up to 16 (ntile + 3) - 1
                            for (int slot = 0; slot < (ntile + 3) * 16; ++slot) {
                                const int qtok = slot_token(wg, wg_min(slot, wg.nq - 1));
                                CHECK(qtok >= 0 && qtok < NTOK, "%dx%d shift %d window (%d, %d) slot %d: token %d", H, W, shift, wr, wc, slot, qtok);
                                const int qrev = att_qrev(qtok / WS, qtok % WS);
                                for (int kt = 0; kt < 9; ++kt) {
                                    for (int g = 0; g < 4; ++g) {
                                        const int first = qrev + att_koff(att_key0(kt, g));
                                        CHECK(first >= 0 && first + 3 <= TABN - 1, "%dx%d shift %d window (%d, %d) slot %d tile %d group %d: words %d .. %d",
                                              H, W, shift, wr, wc, slot, kt, g, first, first + 3);
                                    }
                                }
                                ++slots;
                                past += slot >= wg.nq;
                            }
                        }
                    }
                }
            }
        }
    }
    std::printf("slots %ld past_nq %ld\n", slots, past);
    if (fails) { std::printf("%ld checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
