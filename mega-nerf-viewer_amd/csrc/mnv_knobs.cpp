// mnv_knobs.cpp -- see mnv_knobs.h.  Compiled twice: plain for libmnv.so (no getenv, no names), with MNV_TEST_HOOKS for testhooks/libmnv.so.
#include "mnv_knobs.h"

#ifdef MNV_TEST_HOOKS
#include <atomic>
#include <cstdint>
#include <cstdlib>
#endif

namespace mnv {

#ifdef MNV_TEST_HOOKS
static const char *const kKnobNames[KNOB_COUNT] = {
    "MNV_TILE_WLOG",      "MNV_QUEUES",           "MNV_LDS_LEVEL",      "MNV_BLOCKS_PER_CU",   "MNV_REFILL_MIN",     "MNV_ABLATE",
    "MNV_STATS",          "MNV_TIMELINE",         "MNV_GRID2_LEVEL",    "MNV_BRICK_LEVELS",    "MNV_F2_BLOCKS_PER_CU", "MNV_F2_SWITCH_MIN",
    "MNV_FUSED_BATCH_MIN", "MNV_VOTE_WIDE_KEYS",  "MNV_VOTE_FULL_SORT", "MNV_ASSEMBLE_NARROW", "MNV_REFRESH_DEBUG",  "MNV_SYNTH_TIMING",
    "MNV_FOOTPRINT",      "MNV_SHADOW",           "MNV_MARCH_SHAPE",
};
const char *knob_str(Knob k) { return k >= 0 && k < KNOB_COUNT ? std::getenv(kKnobNames[k]) : nullptr; }
int knob_int(Knob k, int dflt) {
    const char *v = knob_str(k);
    return v ? std::atoi(v) : dflt;
}
bool knob_set(Knob k) { return knob_str(k) != nullptr; }
static std::atomic<long long> g_ref_table_min_rays{1 << 16};
long long ref_table_min_rays() { return g_ref_table_min_rays.load(std::memory_order_relaxed); }
// bits 0..7: BASIS + 1 (RGBA rows are BASIS -1), 8..15: MODE, 16: BRICK, 17: RAYS, 31: set once a launch was noted
static std::atomic<uint32_t> g_last_march_variant{0};
void note_march_variant(int basis, int mode, bool brick, bool rays) {
    g_last_march_variant.store(0x80000000u | (uint32_t)((basis + 1) & 0xff) | (uint32_t)(mode & 0xff) << 8 | (uint32_t)brick << 16 | (uint32_t)rays << 17,
                               std::memory_order_relaxed);
}
static std::atomic<int> g_last_march_shape{-1};
void note_march_shape(int shape) { g_last_march_shape.store(shape, std::memory_order_relaxed); }
#else
long long ref_table_min_rays() { return 1 << 16; }
const char *knob_str(Knob) { return nullptr; }
int knob_int(Knob, int dflt) { return dflt; }
bool knob_set(Knob) { return false; }
void note_march_variant(int, int, bool, bool) {}
void note_march_shape(int) {}
#endif

}  // namespace mnv

#ifdef MNV_TEST_HOOKS
extern "C" void mnv_hook_set_ref_table_min_rays(long long min_rays) { mnv::g_ref_table_min_rays.store(min_rays, std::memory_order_relaxed); }
extern "C" void mnv_hook_last_march_variant(int32_t out4[4]) {
    const uint32_t w = mnv::g_last_march_variant.load(std::memory_order_relaxed);
    const bool any = (w >> 31) != 0;
    out4[0] = any ? (int32_t)(w & 0xff) - 1 : -2;
    out4[1] = any ? (int32_t)(w >> 8 & 0xff) : -1;
    out4[2] = any ? (int32_t)(w >> 16 & 1) : -1;
    out4[3] = any ? (int32_t)(w >> 17 & 1) : -1;
}
extern "C" int32_t mnv_hook_last_march_shape() { return (int32_t)mnv::g_last_march_shape.load(std::memory_order_relaxed); }
#endif
