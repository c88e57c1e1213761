/*
 * abnn_debug.h -- diagnostics exported by libabnn_hip.so beside the C-ABI of
 * abnn.h.  NOT part of the stable boundary: their layouts follow the kernels
 * (abnn_amd/csrc/engine.h) and change without an ABI version bump.  Used by
 * tools/ (wave_clock.py, apply_clock.py, pass_stats.py) and the GPU tests.
 * Every call is synchronous (waits for the device) and copies at most n words.
 */
#ifndef ABNN_ABNN_DEBUG_H
#define ABNN_ABNN_DEBUG_H

#include "abnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Record the per-wave gate timeline of the following passes (on != 0) or not
 * (the default: the timeline's stores cost ~1.2 us per fused pass). */
abnn_status abnn_debug_set_wave_clock(abnn_brain* b, int on);
/* The last pass's per-wave gate timeline: 12 u64 per range (100-MHz ticks:
 * start, stream done, tail done, entry, look-back done, walk done, ...),
 * recorded while abnn_debug_set_wave_clock is on. */
abnn_status abnn_debug_wave_clock(abnn_brain* b, uint64_t* out, uint64_t n);
/* The same for pass p of the fused single-GPU pass, slot = p % 8 (the last
 * eight fused passes are kept). */
abnn_status abnn_debug_wave_clock_slot(abnn_brain* b, uint32_t slot, uint64_t* out, uint64_t n);
/* The last two-kernel pass's per-workgroup k_apply timeline, 8 u64 each. */
abnn_status abnn_debug_apply_clock(abnn_brain* b, uint64_t* out, uint64_t n);
/* The recent-spike bitmap the last pass read (bit i: neuron i recent at its
 * start), and whether the next pass's was built in-pass (1) or will be
 * rebuilt from lastFired (0). */
abnn_status abnn_debug_bitmap(abnn_brain* b, uint32_t* out, uint64_t n, int* incremental_next);
/* The current sweep partition: n_ranges + 1 iteration bounds. */
abnn_status abnn_debug_range_bounds(abnn_brain* b, uint32_t* out, uint64_t n);
/* The pinned slice of the sweep's record stream in use: iterations whose index
 * mod 16 is below *pin_k are read with ordinary loads (ABNN_STREAM_PIN_MB). */
abnn_status abnn_debug_stream_pin(abnn_brain* b, uint32_t* pin_k);

/* Buffer-index launcher (abnn_launch_traversal): the last pass's pre-gated
 * and refractory-surviving events {g1, g2} from its workspace (synchronises
 * `stream`); HIP events around every k_raw_gate launch while enabled (enable
 * also clears them), their summed milliseconds and count. */
abnn_status abnn_debug_raw_stats(const void* workspace, uint64_t* out2, void* stream);
abnn_status abnn_debug_raw_gate_timing(int enable);
abnn_status abnn_debug_raw_gate_time(double* total_ms, uint32_t* launches);
/* The buffer-index pass in one launch after the filter (k_raw_pass) or the
 * five-launch pass of round 4: mode 1 / 0, or -1 = the ABNN_RAW_FUSED
 * environment variable (default: the fused pass when its 256 workgroups fit
 * the device at once). */
abnn_status abnn_debug_raw_fused(int mode);
/* 1 when the next abnn_launch_traversal runs the fused pass, else 0. */
int abnn_debug_raw_fused_active(void);
/* The last fused buffer-index pass's per-range timeline from its workspace:
 * 8 u64 per range (100-MHz ticks: entry, stream start, stream done, look-back
 * done, walk done, end; then iterations, survivors). */
abnn_status abnn_debug_raw_wave_clock(const void* workspace, uint64_t workspace_bytes, uint32_t n_syn,
                                      uint32_t events, uint64_t* out, uint64_t n, void* stream);

/* The sharded pass's exchange alone: `count` in-place all-gathers of
 * `bytes` per rank on the library's RCCL communicator (enqueued on `stream`;
 * buf holds world x bytes, this rank's record at rank x bytes). */
abnn_status abnn_debug_comm_allgather(abnn_comm* c, void* buf, uint64_t bytes, uint32_t count, void* stream);

/* Device allocations the library made (for its handles: brains, snapshots,
 * engines, communicators, and inside its calls) and has not freed yet, in the
 * whole process.  Every destroy brings it back to what it was before the
 * create; a caller's workspace (abnn_launch_traversal) is not the library's and
 * is not counted.  Not synchronous, touches no device. */
uint64_t abnn_debug_live_allocations(void);

/* The forward instance of the handle's following propagations (abnn_propagate_*):
 * 0 = chosen on the device from the non-zero count of x (the default), 1 = the
 * sparse one, 2 = the dense one.  The result's words do not depend on it.
 * Not synchronous. */
abnn_status abnn_debug_set_propagate_path(abnn_brain* b, int path);

/* The LINK step of the handle's following component searches (abnn_components_*):
 * 0 = the settled map when the handle holds enough records per neuron for it
 * to pay (the default), 1 = never (every followed record walks the plane), 2 =
 * always.  The result's words do not depend on it.  Not synchronous. */
abnn_status abnn_debug_set_components_path(abnn_brain* b, int path);

/* The kernel path of the handle's following connectivity matrices
 * (abnn_matrix_*): how a record's cell is added -- run aggregation along the
 * wave (a wave in one cell adds once), or one LDS atomic per record -- and where
 * a LABELS scan reads a population: the handle's packed byte plane or the
 * caller's u32 plane.  0 = the default (runs, packed), 1 = runs + packed, 2 =
 * runs + direct, 3 = atomics + packed, 4 = atomics + direct.  The result's
 * words do not depend on it.  Not synchronous. */
abnn_status abnn_debug_set_matrix_path(abnn_brain* b, int path);

/* The indexed fused pass: out = {index built (0/1), its entries,
 * its largest degree, the last pass was indexed (0/1), indexed passes so far,
 * consecutive eligible passes since the records last changed, ABNN_INDEXED in
 * force, the sweep's visited events E}; *build_ms (may be null): the last
 * build's time.  Not synchronous. */
#define ABNN_DEBUG_INDEX_WORDS 8
abnn_status abnn_debug_index_state(abnn_brain* b, uint64_t out[ABNN_DEBUG_INDEX_WORDS], double* build_ms);
/* The 32-bit words of the event mask that differ from what the next indexed
 * pass expects: bit e set iff src(e) is in the marked set, the bitmap of the
 * last indexed pass (all-zero after a build).  The expected mask is made by the
 * mark kernel itself from the marked set.  0 at every kernel boundary, 0
 * without an index.  Synchronous. */
abnn_status abnn_debug_index_mask_dirty(abnn_brain* b, uint64_t* words);
/* The event mask's first n_words 32-bit words (bit e of the mask: event e) and
 * the marked set's first n_marked_words (bit n: neuron n) to the host; a count
 * above a buffer's length copies all of it (the mask's padding included) and
 * leaves the rest of the caller's words as they are, as abnn_debug_bitmap.
 * Synchronous; an error without an index. */
abnn_status abnn_debug_index_mask_copy(abnn_brain* b, uint32_t* mask_words_out, uint64_t n_words, uint32_t* marked_out,
                                       uint64_t n_marked_words);
/* The last mark launch: out = {neurons that entered the marked set, neurons
 * that left it, mask bits set, mask bits cleared}.  Zeros before the first
 * indexed pass since the build.  Synchronous. */
abnn_status abnn_debug_index_delta(abnn_brain* b, uint64_t out[4]);
/* ABNN_INDEXED for this handle's following passes: 0 never indexed, 1 the
 * default rule, 2 whenever the index is valid.  Not synchronous. */
abnn_status abnn_debug_set_indexed(abnn_brain* b, int mode);
/* ABNN_FUSED for this handle's following single-GPU passes: 1 = the fused
 * launch where the gate shape has one (the default), 0 = the two-kernel pass
 * (k_gate + k_apply).  Results do not depend on it.  Not synchronous. */
abnn_status abnn_debug_set_fused(abnn_brain* b, int on);
/* The built index's row[0, n_row) (n_row <= N_NRN + 1) and off[0, n_off)
 * (n_off <= entries) to the host.  Synchronous; an error without an index. */
abnn_status abnn_debug_index_copy(abnn_brain* b, uint32_t* row, uint64_t n_row, uint32_t* off, uint64_t n_off);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* ABNN_ABNN_DEBUG_H */
