// mnv_accel_diag.hip -- the host half of the march's measurement instruments (device half: mnv_march_diag.h): which of them a launch
// carries (the knobs of the DESIGN.md section 5.2 table; the shipped library reads none, mnv_knobs.cpp), their buffers (mnv_accel::diag)
// and the reports written when the accel is destroyed.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "mnv_accel_launch.h"
#include "mnv_knobs.h"

namespace mnv {

// The diagnostics of a launch (knobs read once): counters, ablations, the tile / wavefront timeline, the footprint bitmap and the shadow
// copies.  The caller holds the launch lock; the buffers belong to the accel.
int attach_diagnostics(mnv_accel *a, AccelLaunch &K, bool rays, bool fused, int n_blocks, hipStream_t stream) {
    AccelDiag &d = a->diag;
    static const int env_ablate = knob_int(KNOB_ABLATE, 0);
    K.ablate = env_ablate;
    static const bool env_stats = knob_set(KNOB_STATS);
    static const char *env_timeline = knob_str(KNOB_TIMELINE);
    static const char *env_footprint = knob_str(KNOB_FOOTPRINT);
    if ((env_stats || env_ablate || env_timeline || env_footprint) && !rays) {  // all four run on the diagnostics instantiation (camera frames only)
        if (!d.stats) {
            if (d.stats.alloc(32) != hipSuccess) return (int)hipErrorOutOfMemory;
            (void)hipMemsetAsync(d.stats.get(), 0, d.stats.bytes(), stream);
        }
        K.diag.stats = d.stats.get();
    }
    static const int env_stats_level = env_stats ? std::max(1, knob_int(KNOB_STATS, 1)) : 0;
    K.diag.count_stats = env_stats ? env_stats_level : 0;
    if (env_footprint && !fused) {
        // one bit per 128-byte line of every array the march loads from; the bits of all launches accumulate until mnv_accel_destroy counts them
        if (!d.line_bits) {
            const uint64_t cells2 = a->view.grid2_level > 0 ? (uint64_t)1 << (3 * a->view.grid2_level) : 0, cells1 = (uint64_t)1 << (3 * a->view.grid_level);
            const uint64_t nvox = (uint64_t)a->reserved * 8;
            const uint64_t bytes[6] = {cells2 * 4, (uint64_t)a->reserved * kRecWords * 4, nvox * 4, nvox * (uint64_t)a->view.row_bytes, cells2 * 4, cells1 * 4};
            uint64_t at = 0;
            for (int i = 0; i < 6; ++i) {
                d.line_base[i] = (uint32_t)at;
                at += (bytes[i] + 127) / 128 + 1;
            }
            d.line_base[6] = (uint32_t)at;
            const size_t words = (size_t)(at + 31) / 32;
            if (d.line_bits.alloc(words) != hipSuccess) return (int)hipErrorOutOfMemory;
            (void)hipMemsetAsync(d.line_bits.get(), 0, words * 4, stream);
        }
        K.diag.line_bits = d.line_bits.get();
        for (int i = 0; i < 6; ++i) K.diag.line_base[i] = d.line_base[i];
    }
    static const int env_shadow = knob_int(KNOB_SHADOW, 0);
    if (env_shadow & (16 | 32 | 64)) {
        // shadow loads (test-hook build + a -DMNV_SHADOW_MASK variant of the march): copies of the arrays at other addresses, made once
        const size_t nvox = (size_t)a->reserved * 8;
        auto shadow = [&](Buffer<uint8_t> &dst, const void *src, size_t bytes) -> int {
            if (dst || !src) return 0;
            hipError_t es = dst.alloc(bytes);
            if (es == hipSuccess) es = hipMemcpyAsync(dst.get(), src, bytes, hipMemcpyDeviceToDevice, stream);
            return (int)es;
        };
        int es = 0;
        if (env_shadow & 16) es = shadow(d.shadow_nodes, a->nodes.get(), nvox * 4);
        if (!es && (env_shadow & 32)) es = shadow(d.shadow_rows, a->rows.get(), nvox * (size_t)a->view.row_bytes);
        if (!es && (env_shadow & 64) && a->recs) es = shadow(d.shadow_nodes, a->recs.get(), (size_t)a->reserved * kRecWords * 4);  // (bits 16 and 64 are not combined)
        if (es) return es;
        K.shadow_nodes = reinterpret_cast<const uint32_t *>(d.shadow_nodes.get());
        K.shadow_rows = d.shadow_rows.get();
        K.shadow_recs = reinterpret_cast<const uint2 *>(d.shadow_nodes.get());
    }
    if (env_timeline && K.diag.stats) {
        // (re)allocate the record buffer of this launch; mnv_accel_destroy writes the last launch's records to the file
        const size_t tiles = (size_t)K.n_tiles * (size_t)K.n_frames, waves = (size_t)n_blocks * 4;
        const size_t bytes = (tiles * 4 + waves * 2) * 8;
        if (grow(d.timeline, bytes / 8, bytes / 8, stream, false) != hipSuccess) return (int)hipErrorOutOfMemory;
        (void)hipMemsetAsync(d.timeline.get(), 0, bytes, stream);
        d.timeline_tiles = tiles;
        d.timeline_waves = waves;
        d.timeline_tiles_per_frame = K.n_tiles;
        K.diag.timeline = d.timeline.get();
        K.diag.timeline_tiles = (uint32_t)tiles;
    }
    return 0;
}

// What the instruments gathered over the accel's life: counters and phase shares on stderr, the last launch's timeline and the
// footprint into the files their knobs name.
void report_diagnostics(const mnv_accel *a) {
    const AccelDiag &d = a->diag;
    if (d.stats && knob_set(KNOB_STATS)) {
        unsigned long long h[16];
        if (hipMemcpy(h, d.stats.get(), sizeof(h), hipMemcpyDeviceToHost) == hipSuccess) {
            unsigned long long ph[8] = {};
            if (hipMemcpy(ph, d.stats.get() + 16, sizeof(ph), hipMemcpyDeviceToHost) == hipSuccess && ph[4] > 0)
                fprintf(stderr, "[mnv phases] share of the wavefronts' time (serialised by the stamps): lookup %.3f, step arithmetic + opacity %.3f, row wait %.3f, "
                                "colour arithmetic %.3f, other (refill, ray set-up, flush, loop) %.3f; wave-steps %llu\n",
                        (double)ph[0] / ph[4], (double)ph[1] / ph[4], (double)ph[2] / ph[4], (double)ph[3] / ph[4], 1.0 - (double)(ph[0] + ph[1] + ph[2] + ph[3]) / ph[4], ph[5]);
            const char *names[] = {"outer_iter", "refill", "march_step", "node_load", "dense", "colour_pass"};
            for (int i = 0; i < 6; ++i)
                fprintf(stderr, "[mnv stats] %-13s wave-level %llu lane-level %llu (%.1f lanes)\n", names[i], h[2 * i], h[2 * i + 1],
                        h[2 * i] ? (double)h[2 * i + 1] / (double)h[2 * i] : 0.0);
            // the colour block's two exponential paths (kCountExpUniform, kCountExpGeneral), a line of their own
            fprintf(stderr, "[mnv exp paths] uniform wave-level %llu lane-level %llu, general wave-level %llu lane-level %llu\n", h[12], h[13], h[14], h[15]);
        }
    }
    if (d.timeline && knob_str(KNOB_TIMELINE)) {
        const size_t words = d.timeline_tiles * 4 + d.timeline_waves * 2;
        std::vector<unsigned long long> h(words + 3);
        h[0] = d.timeline_tiles;
        h[1] = d.timeline_waves;
        h[2] = d.timeline_tiles_per_frame;
        if (hipMemcpy(h.data() + 3, d.timeline.get(), words * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *f = fopen(knob_str(KNOB_TIMELINE), "wb")) {
                fwrite(h.data(), 8, h.size(), f);
                fclose(f);
            }
        }
    }
    if (d.line_bits && knob_str(KNOB_FOOTPRINT)) {
        // unique 128-byte lines per array, as JSON (tools/footprint.py reads it)
        const size_t words = ((size_t)d.line_base[6] + 31) / 32;
        std::vector<uint32_t> h(words);
        if (hipMemcpy(h.data(), d.line_bits.get(), words * 4, hipMemcpyDeviceToHost) == hipSuccess) {
            static const char *names[6] = {"grid2", "records", "nodes", "rows", "grid2_vox", "grid_vox"};
            unsigned long long lines[6] = {};
            for (int r = 0; r < 6; ++r)
                for (uint32_t l = d.line_base[r]; l < d.line_base[r + 1]; ++l) lines[r] += (h[l >> 5] >> (l & 31u)) & 1u;
            if (FILE *f = fopen(knob_str(KNOB_FOOTPRINT), "w")) {
                fprintf(f, "{");
                for (int r = 0; r < 6; ++r) fprintf(f, "\"%s_lines\": %llu, ", names[r], lines[r]);
                fprintf(f, "\"line_bytes\": 128}\n");
                fclose(f);
            }
        }
    }
}

}  // namespace mnv
