// mnv_march_diag.h -- the measurement instruments of march_accel_kernel (mnv_march_accel_kernel.h), device half: MarchProbe, one object
// per thread whose methods are empty in every instantiation but the diagnostics one (MODE 1), and the shadow loads of the
// -DMNV_SHADOW_MASK variants.  The host half -- knobs, buffers, reports -- is mnv_accel_diag.hip.
#pragma once

#include "mnv_accel_launch.h"

namespace mnv {

// Attribution of the L2 misses by array (tools/traffic_by_array.sh builds variants of the library with -DMNV_SHADOW_MASK=<bits>): every load
// of the chosen array is repeated at the same index of a copy at other addresses -- results stay right, the miss counters grow by about
// that array's share.  8 grid2 (its shadow is grid2_vox), 16 nodes, 32 rows, 64 brick records.  0 in every shipped build.
#ifndef MNV_SHADOW_MASK
#define MNV_SHADOW_MASK 0
#endif
constexpr int kShadow = MNV_SHADOW_MASK;

// a shadow load (behind `if constexpr ((kShadow & bit) != 0)`: the shipped kernels do not even form the address): one dword at p
// (rows: one more line fill), kept alive without a use
__device__ __forceinline__ void shadow_load(const uint32_t *p) {
    const uint32_t w2 = *p;
    asm volatile("" ::"v"(w2));
}
__device__ __forceinline__ void shadow_load(const uint2 *p) {
    const uint2 e2 = *p;
    asm volatile("" ::"v"(e2.x));
}

// counters of MNV_STATS (slot of the wave-level count in K.diag.stats; the lane-level count follows it) and the report's names for them
// (kCountExpUniform / kCountExpGeneral: dense iterations of the per-lane SH block whose four exponentials ran as one block behind the
// wavefront's range test / through exact_expf because a dense lane held an argument of |x| >= 88; the report's "[mnv exp paths]" line)
enum MarchCount {
    kCountOuterIter = 0, kCountRefill = 2, kCountMarchStep = 4, kCountNodeLoad = 6, kCountDense = 8, kCountColourPass = 10,
    kCountExpUniform = 12, kCountExpGeneral = 14
};
// regions of the MNV_FOOTPRINT bitmap (K.diag.line_base)
enum MarchRegion { kLinesGrid2 = 0, kLinesRecs = 1, kLinesNodes = 2, kLinesRows = 3, kLinesGrid2Vox = 4, kLinesGridVox = 5 };
// phases of a wavefront's step (MNV_STATS=2)
enum MarchPhase { kPhaseLookup, kPhaseStep, kPhaseRow, kPhaseColour };

template <int MODE, bool RAYS, int BLOCK>
struct MarchProbe {
    const LaunchBlock<RAYS> &K;
    const int lane;
    // MNV_TIMELINE: when each tile was grabbed and finished and by which wavefront (tools/timeline.py)
    uint32_t tl_rec = ~0u, tl_iters = 0;
    // MNV_STATS=2: where the cycles of a wavefront's step go.  Every stamp waits for all outstanding memory operations first, so the
    // phases do not overlap as they may in the product kernel: this is the DEPENDENT chain, what bounds a launch that drains.
    // stats[16..]: lookup (LDS grid -> grid2 -> node words), step arithmetic + opacity, row wait, colour arithmetic, the wavefront's
    // whole time, wave-steps (tools/step_phases.py; LAB_NOTEBOOK.md round 3).
    unsigned long long ph_lookup = 0, ph_step = 0, ph_row = 0, ph_colour = 0, ph_steps = 0, ph_mark = 0, ph_begin = 0;

    __device__ __forceinline__ MarchProbe(const LaunchBlock<RAYS> &launch, int lane_of_wave) : K(launch), lane(lane_of_wave) {}

    __device__ __forceinline__ static uint32_t wave_id() { return blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); }

    // diagnostics only (breaks results): 1 no colour, 2 no dense samples, 4 cached rows
    __device__ __forceinline__ bool ablate(int bit) const {
        if constexpr (MODE == 1) return (K.ablate & bit) != 0;
        else return false;
    }

    // one wave-level and popcount(pred) lane-level events
    __device__ __forceinline__ void count(MarchCount slot, bool pred) const {
        if constexpr (MODE == 1) {
            if (!K.diag.count_stats) return;
            const uint64_t m = __ballot(pred);
            if (m && lane == (int)__builtin_ctzll(m)) {
                atomicAdd(&K.diag.stats[slot], 1ull);
                atomicAdd(&K.diag.stats[slot + 1], (unsigned long long)__popcll(m));
            }
        }
    }

    // MNV_FOOTPRINT: the 128-byte line a load touches, by array (region) and byte offset into it
    __device__ __forceinline__ void touch(MarchRegion region, uint64_t byte_off) const {
        if constexpr (MODE == 1) {
            if (K.diag.line_bits) {
                const uint32_t line = K.diag.line_base[region] + (uint32_t)(byte_off >> 7);
                atomicOr(&K.diag.line_bits[line >> 5], 1u << (line & 31u));
            }
        }
    }

    __device__ __forceinline__ unsigned long long phase_clock() const {
        if constexpr (MODE == 1) {
            if (K.diag.count_stats == 2) {
                __builtin_amdgcn_s_waitcnt(0);
                return (unsigned long long)__builtin_readcyclecounter();
            }
        }
        return 0ull;
    }

    __device__ __forceinline__ void wave_begin() {
        if constexpr (MODE == 1) {
            if (K.diag.timeline && lane == 0) K.diag.timeline[(size_t)K.diag.timeline_tiles * 4 + (size_t)wave_id() * 2] = wall_clock64();
            ph_begin = phase_clock();
        }
    }
    // the flush of the phase sums and the wavefront's exit stamp
    __device__ __forceinline__ void wave_end() const {
        if constexpr (MODE == 1) {
            if (K.diag.count_stats == 2 && lane == 0) {
                atomicAdd(&K.diag.stats[16], ph_lookup);
                atomicAdd(&K.diag.stats[17], ph_step);
                atomicAdd(&K.diag.stats[18], ph_row);
                atomicAdd(&K.diag.stats[19], ph_colour);
                atomicAdd(&K.diag.stats[20], phase_clock() - ph_begin);
                atomicAdd(&K.diag.stats[21], ph_steps);
            }
            if (K.diag.timeline && lane == 0) K.diag.timeline[(size_t)K.diag.timeline_tiles * 4 + (size_t)wave_id() * 2 + 1] = wall_clock64();
        }
    }

    __device__ __forceinline__ void iteration() {
        if constexpr (MODE == 1) ++tl_iters;
    }
    __device__ __forceinline__ void tile_close(unsigned long long now) const {
        if constexpr (MODE == 1) {
            if (K.diag.timeline && tl_rec != ~0u && lane == 0) {
                K.diag.timeline[(size_t)tl_rec * 4 + 1] = now;
                K.diag.timeline[(size_t)tl_rec * 4 + 3] = tl_iters;
            }
        }
    }
    // the wavefront took the tile of rays [base, base + 64) of frame f (closes the record of the tile it held)
    __device__ __forceinline__ void tile_grabbed(uint32_t f, uint32_t base) {
        if constexpr (MODE == 1) {
            if (K.diag.timeline) {
                const unsigned long long now = wall_clock64();
                tile_close(now);
                tl_rec = f * K.n_tiles + (base >> 6);
                tl_iters = 0;
                if (lane == 0) {
                    K.diag.timeline[(size_t)tl_rec * 4 + 0] = now;
                    K.diag.timeline[(size_t)tl_rec * 4 + 2] = wave_id();
                }
            }
        }
    }
    // no lane of the wavefront is alive: the tile is done; what follows is queue polling
    __device__ __forceinline__ void tile_done() {
        if constexpr (MODE == 1) {
            if (K.diag.timeline && tl_rec != ~0u) {
                tile_close(wall_clock64());
                tl_rec = ~0u;
            }
        }
    }

    // a step begins / phase PH of it has ended (the step phase counts the wave-step; the colour phase is the step's last)
    __device__ __forceinline__ void step_begin() {
        if constexpr (MODE == 1) ph_mark = phase_clock();
    }
    template <MarchPhase PH>
    __device__ __forceinline__ void phase_end() {
        if constexpr (MODE == 1) {
            if (K.diag.count_stats == 2) {
                const unsigned long long now = phase_clock();
                (PH == kPhaseLookup ? ph_lookup : PH == kPhaseStep ? ph_step : PH == kPhaseRow ? ph_row : ph_colour) += now - ph_mark;
                if constexpr (PH != kPhaseColour) ph_mark = now;  // (step_begin sets the next step's)
                if constexpr (PH == kPhaseStep) ++ph_steps;
            }
        }
    }
};

}  // namespace mnv
