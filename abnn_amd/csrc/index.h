// index.h -- the src index of the swept records and the per-pass event mask
// of the indexed fused pass (index.hip; DESIGN.md §5 "Indexed pass").
// Internal, like engine.h.
//
// The index groups the events [0, E) of a sweep by the src of their record:
// row[n] .. row[n + 1] are neuron n's entries of off[], each the offset of one
// record whose decoded src (code_src) is n, whatever its dst (a tombstone dst
// still counts as pre-gated).  Tombstone src stays out.  Order inside a list
// is whatever the scatter's atomics made it.  It is valid while the src of
// records [0, E) and E itself do not change (capi.hip index_invalidate).
//
// The mask holds one bit per event, and the index keeps a marked set beside
// it, a bitmap over neurons.  The invariant, at every kernel boundary: mask
// bit e is set iff src(e) is in the marked set.  Both start all-zero when the
// index is built and go with it (index_invalidate); k_index_mark is their only
// writer, so passes of other flavours in between leave them alone.
// k_index_mark, launched in front of an indexed pass, is a delta mark: it
// compares the marked set with this pass's exact recent-spike bitmap, ORs the
// lists of the neurons that enter into the mask, AND-NOTs the lists of those
// that leave out of it, and leaves marked set = bitmap.  Afterwards bit e is
// set iff bitmap[src(e)] is, which is the pre-spike gate itself
// (brain.metal:73-77), no false positives and no false negatives.  k_gate's
// mask flavour (kernels.hip) streams the mask where the stream flavour streams
// the 3-B src codes, and only reads it.
//
// The marked set has two buffers: a launch reads the one and writes the other
// (a heavy chunk's workgroup reads its neuron's old bit from a word that a
// light wave of the same launch rewrites), and the host swaps them after an
// indexed pass, as it rotates the partition's bounds.
#pragma once

#include "engine.h"

namespace abnn {

// The mask flavour reads a wave's mask bytes in rounds of kMaskRoundBytes,
// whole, so the last round of the sweep's last range reads up to one round
// past the sweep: the mask is padded by two (zero, never written).
constexpr uint32_t kMaskRoundBytes = 4096;
inline uint64_t index_mask_words(uint64_t iters, uint64_t iter_events)
{
    return iters * iter_events / 32 + 2 * kMaskRoundBytes / 4;
}

// The exclusive scan's tiles: kIndexTile neurons per workgroup.
constexpr uint32_t kIndexTile = 4096;
inline uint64_t index_tiles(uint64_t n_nrn) { return (n_nrn + kIndexTile - 1) / kIndexTile; }

// Builds row[n_nrn + 1] and off[] (room for `events` entries) from records
// [0, events), all on `s`: count (cursor, zeroed here), scan, scatter.
// cursor[n_nrn + 1] and part[index_tiles + 1] are scratch; info[4]: info[0] =
// the largest degree, info[1] = the entries, info[2] = the heavy list's chunks.
hipError_t launch_index_build(const SynArrays& syn, uint64_t events, uint64_t n_nrn, uint32_t* row, uint32_t* cursor,
                              uint32_t* part, uint32_t* off, uint32_t* info, uint32_t cus, hipStream_t s);
// The heavy list, after the build and its read-back of info: the lists above
// kHeavyLen entries as `chunks` = info[2] chunks {neuron, first entry, entries,
// 0} of heavy[chunks] (info[3]: the fill's cursor).
hipError_t launch_index_heavy(const uint32_t* row, uint64_t n_nrn, uint4* heavy, uint32_t chunks, uint32_t* info,
                              hipStream_t s);
// The delta mark.  mask |= the events of every neuron of bitmap & ~marked,
// mask &= ~ the events of every neuron of marked & ~bitmap, marked_next =
// bitmap (all three of n_words; bitmap: this pass's exact one): one launch, the
// short lists by the waves that hold their neurons' bitmap words, every chunk
// of the heavy list by a workgroup of its own.  delta (may be null): the
// launch adds {neurons entered, neurons left, entries set, entries cleared} to
// the kDeltaSlots slots of four words (a wave's slot by its number: the sum
// over the slots is the launch's); delta_next (may be null), as long, is zeroed
// for the next launch.
constexpr uint32_t kDeltaSlots = 1024;
hipError_t launch_index_mark(const uint32_t* bitmap, const uint32_t* marked, uint32_t* marked_next, uint32_t n_words,
                             uint64_t n_nrn, const uint32_t* row, const uint32_t* off, uint32_t* mask, uint64_t events,
                             const uint4* heavy, uint32_t chunks, uint32_t* delta, uint32_t* delta_next, hipStream_t s);
// *out (zeroed here) = the words of mask[words] that differ from want[words] (abnn_debug_index_mask_dirty).
hipError_t launch_index_dirty(const uint32_t* mask, const uint32_t* want, uint64_t words, unsigned long long* out,
                              hipStream_t s);

}  // namespace abnn
