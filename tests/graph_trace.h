// graph_trace.h — what graph_trace_stubs.cpp and graph_trace_main.cpp share: the fake address ranges pointers are printed from, and the
// controls of the log.  Nothing here is ever dereferenced.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace trace {

// every fake pointer lives in one of these ranges and is printed as <name>+<byte offset> (or w<id> for weights)
constexpr uintptr_t ARENA_BASE = 0x100000000000ull;    // the workspace arena: arena+<offset>
constexpr size_t ARENA_CAP = (size_t)1 << 40;
constexpr uintptr_t W_BASE = 0x200000000000ull;        // weights: w<id>, one id per tensor and kind, W_STRIDE bytes apart
constexpr uintptr_t W_STRIDE = 4096;
constexpr uintptr_t IMG_BASE = 0x300000000000ull;      // the input image: img
constexpr uintptr_t OUT_BASE = 0x310000000000ull;      // the logits: out
constexpr uintptr_t STREAM_BASE = 0x400000000000ull;   // streams: s<ordinal> (0 = the forward's own, 1 + k = auxiliary stream k)
constexpr uintptr_t FORK_BASE = 0x500000000000ull;     // events: fork<k>, join<k>, stage<i>; hipEventCreate hands out ev<n>
constexpr uintptr_t JOIN_BASE = 0x510000000000ull;
constexpr uintptr_t STAGE_BASE = 0x520000000000ull;
constexpr uintptr_t EV_BASE = 0x530000000000ull;

inline hipStream_t stream(int ordinal) { return reinterpret_cast<hipStream_t>(STREAM_BASE + 16 * (uintptr_t)ordinal); }
inline hipEvent_t event(uintptr_t base, int i) { return reinterpret_cast<hipEvent_t>(base + 16 * (uintptr_t)i); }

void set_quiet(bool q);       // true: the stubs print nothing (dry and profiled runs)
void reset_events();          // the next hipEventCreate hands out ev0 again

}  // namespace trace
