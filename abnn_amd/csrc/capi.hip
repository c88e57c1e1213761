// capi.hip -- implementation of the C-ABI (include/abnn/abnn.h) over the HIP
// kernels of kernels.hip.  Replaces the Metal host class Brain
// (abnn/src/core/brain/brain.{h,cpp}); each function cites what it replaces.
#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>  // types only: the entry points are resolved at run time (rccl_api)

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "census.h"
#include "degree.h"
#include "select.h"
#include "edit.h"
#include "snapshot.h"
#include "graph.h"
#include "hops.h"
#include "components.h"
#include "matrix.h"
#include "engine.h"
#include "learn.h"
#include "spikes.h"
#include "corr.h"
#include "reorder.h"
#include "propagate.h"
#include "index.h"
#include "pool.h"
#include "../../include/abnn/abnn_debug.h"

using namespace abnn;

static thread_local std::string g_err;

void abnn::set_err(const std::string& m) { g_err = m; }

namespace {

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t _e = (expr);                                                        \
        if (_e != hipSuccess) {                                                        \
            set_err(std::string(#expr) + ": " + hipGetErrorString(_e));                \
            return ABNN_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)

#define REQUIRE(cond, msg)                                                             \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            set_err(msg);                                                              \
            return ABNN_ERR_INVALID;                                                   \
        }                                                                              \
    } while (0)

uint64_t visited_events(const abnn_dims& d, uint32_t mode)
{
    if (mode == ABNN_MODE_RANDOM) return d.n_syn ? d.events_per_pass : 0;  // README §4: EVENTS picks
    uint64_t grid = (d.events_per_pass + 255u) / 256u * 256u;  // brain.cpp:116-118
    return grid < d.n_syn ? grid : d.n_syn;                     // brain.metal:61
}

struct EventPair {
    hipEvent_t a, b;
};

// The indexed fused pass (index.h): the src index of records
// [0, E), the per-pass event mask, and the bookkeeping of when they hold.
struct IndexState {
    uint32_t *row = nullptr, *off = nullptr, *mask = nullptr, *info = nullptr;
    uint4* heavy = nullptr;        // the lists above index.hip's kHeavyLen entries, in chunks (launch_index_heavy)
    // the marked set the mask stands for (index.h), N_NRN bits, and the buffer the next mark launch writes it to
    // (run_fused swaps them); delta: two blocks of launch_index_mark's counters (4 * kDeltaSlots words each),
    // delta_at the last launch's
    uint32_t *marked = nullptr, *marked_next = nullptr, *delta = nullptr;
    uint32_t delta_at = 0;
    uint32_t heavy_chunks = 0;
    uint64_t mask_words = 0;
    bool built = false;            // row / off describe the records as they are (index_invalidate clears it)
    uint64_t entries = 0;          // records of [0, E) with a live src
    uint32_t max_degree = 0;       // the longest list
    float build_ms = 0.0f;         // the last build, a HIP event pair around its launches
    uint64_t eligible = 0;         // consecutive eligible passes since the records last changed
    bool last_indexed = false;     // the last pass ran the mask flavour
    uint64_t indexed_passes = 0;
    int flavour = -1;              // the last fused pass's (0 stream, 1 mask): the partition's cost history is per flavour
    int mode = 1;                  // ABNN_INDEXED: 0 never, 1 the rule (index_pass_rule), 2 whenever the index is valid
    uint32_t after = 4;            // ABNN_INDEX_AFTER: eligible passes before the build
    uint64_t max_mb = 4096;        // ABNN_INDEX_MAX_MB: no index above it
};

}  // namespace

struct abnn_brain {
    abnn_dims dims{};
    abnn_params params{};
    KernelParams kp{};
    int device = 0;
    hipStream_t stream = nullptr;  // default stream of state accessors (the null stream)
    uint64_t n_nrn = 0;
    DevicePool pool;               // owns every device buffer below and in d, select, spikes, corr, reorder (pool.h)
    DeviceState d{};
    void* scalar_block = nullptr;  // clock | reward | rbar
    uint64_t clock_host = 0;       // mirror, for the renormalisation decision (brain.cpp:127)
    uint64_t rng = 0;              // host RNG of inject_inputs
    uint64_t stim_first = 0, stim_count = 0;
    // steady-state bitmap build by k_apply (build_next_ok): consecutive
    // single-GPU passes whose spike lists are in fired_ring with no clock
    // discontinuity, the highest lastFired value the host wrote (creation's
    // zeros included), the stimulus of the last kFiredRing passes, whether
    // the next pass's bitmap was built (and for which stimulus), borrowed
    // state pointers handed out.  Bitmap and images are triple-buffered by
    // pass % 3: read by pass p, built by pass p - 1, zeroed by pass p - 2.
    uint64_t clean_passes = 0, max_host_stamp = 0;
    uint64_t stim_ring[kFiredRing][2] = {};
    bool next_built = false;
    uint64_t built_stim[2] = {};
    bool ext_ptrs = false, force_full_bitmap = false;
    uint32_t* bitmap_buf[3] = {};
    uint32_t* filter_buf[3] = {};
    // fused single-GPU sweep passes (ABNN_FUSED=0: gate + apply launches):
    // whether the previous pass was fused (its gate costs are in cost_buf[cost
    // parity ^ 1] and its prologue adapts the partition), the look-back words
    bool use_fused = true, last_pass_fused = false;
    uint32_t* cost_buf[2] = {};
    uint32_t cost_parity = 0;
    bool pending_renorm = false;   // shard protocol: decided at gate time
    int timing = 0;                // time every timing-th gate launch (0: off)
    uint64_t timing_count = 0;
    std::vector<EventPair> events;
    size_t events_used = 0;
    uint32_t* idx_scratch = nullptr;
    uint64_t idx_cap = 0;
    uint64_t* u64_scratch = nullptr;
    uint64_t* census_out = nullptr;  // abnn_census's device result (allocated by its first call)
    uint64_t* degree_out = nullptr;  // abnn_degree's device result, grown to the largest one asked
    uint64_t degree_cap = 0;
    SelectScratch select;            // abnn_select_*: per-tile counts and offsets for syn_capacity (its first call)
    uint32_t* hops_bitmap = nullptr; // abnn_hops_*: the frontier bitmap, N_NRN bits (its first call)
    uint64_t* hops_out = nullptr;    // abnn_hops's device result, grown to the largest one asked
    uint64_t hops_cap = 0;
    CompScratch comp;                // abnn_components_*: the size counters, the settled map, the sample's word (its first call)
    uint32_t comp_path = 0;          // ... LINK: 0 the record count chooses, 1 never the settled map, 2 always (abnn_debug_set_components_path)
    uint64_t* comp_out = nullptr;    // abnn_components's device result, grown to the largest one asked
    uint64_t comp_cap = 0;
    uint8_t* mat_pack = nullptr;     // abnn_matrix_*: the label plane packed to one byte per neuron (its first LABELS call)
    uint32_t mat_path = 0;           // ... 0 auto, 1..4 runs / atomics x packed / direct (abnn_debug_set_matrix_path)
    uint64_t* mat_out = nullptr;     // abnn_matrix's device result, grown to the largest one asked
    uint64_t mat_cap = 0;
    uint32_t graph_blocks = 0;       // abnn_build_graph: the most workgroups of its launch (64 per CU; ABNN_GRAPH_BLOCKS)
    bool graph_nt = false;           // ... with non-temporal stores (ABNN_GRAPH_NT=1)
    uint32_t select_blocks = 0;      // ... the most workgroups of its count and emit launches (4 per CU; ABNN_SELECT_BLOCKS)
    uint32_t edit_blocks = 0;        // abnn_edit_*: the most workgroups of its launch (4 per CU; ABNN_EDIT_BLOCKS)
    bool edit_nt = true;             // ... with non-temporal stores (ABNN_EDIT_NT=0: plain)
    float* edit_plane = nullptr;     // abnn_edit's staged plane, grown to the largest one asked
    uint64_t edit_plane_cap = 0;
    uint64_t* edit_out = nullptr;    // abnn_edit's device result (allocated by its first call)
    uint64_t* diff_out = nullptr;    // abnn_snapshot_diff's device result (allocated by its first call)
    SpikeRecorder spikes;            // abnn_spikes_*: on between start and stop (run_commit enqueues its launch)
    CorrScratch corr;                // abnn_corr_*: the map, the planes, the row lists and the tallies (its first call)
    uint64_t* corr_out = nullptr;    // abnn_corr's device result, grown to the largest one asked
    uint64_t corr_cap = 0;
    ReorderScratch reorder;          // abnn_reorder_*: the pair buffers and the records' packed copy for syn_capacity (its first call)
    uint32_t reorder_blocks = 0;     // ... the most workgroups of its launches (4 per CU; ABNN_REORDER_BLOCKS)
    bool reorder_skip = true;        // ... leaving out the radix passes of a constant digit (ABNN_REORDER_SKIP=0: all four)
    PropScratch prop;                // abnn_propagate_*: the non-zero map and the rescale's words (its first call)
    uint32_t prop_path = 0;          // ... the forward instance: 0 the device chooses, 1 sparse, 2 dense (abnn_debug_set_propagate_path)
    int32_t* prop_x = nullptr;       // abnn_propagate's staged x plane, N_NRN int32 (its first call)
    uint64_t* prop_out = nullptr;    // abnn_propagate's device result, grown to the largest one asked
    uint64_t prop_cap = 0;
    int cus = 256, per_cu = 1;     // gate partition inputs (configure)
    uint64_t pass_host = 0;        // mirror of pass_index (structural-update schedule)
    uint64_t rot = 0;              // passes run by this handle: the bitmap buffers' rotation (never reset)
    // structural updates (compact_every > 0, in place: kernels.hip
    // launch_structural_update): the hole blocks' ranks (k_swap_scan2), the
    // scan's per-slice sums, the tail blocks' live prefix (k_swap_tail)
    uint64_t* compact_offsets = nullptr;
    uint64_t* swap_part = nullptr;
    uint64_t* swap_toff = nullptr;
    unsigned long long* span_words = nullptr;  // the update's device words (kernels.hip k_span_init)
    uint32_t* grown_cnt = nullptr;             // used grown slots per 1024-slot block (k_grown_counts)
    uint64_t structural_updates = 0;  // run so far (abnn_structural_updates)
    uint64_t last_pass = ~0ull;       // pass_index of the last pass (its spike list: abnn_get_budget)
    // host-mapped error word: a fused pass whose look-back wait gave up sets it
    // (kernels.hip wg_poll); abnn_traverse sees it without synchronising
    uint32_t* err_host = nullptr;
    // a sharded pass on the fused path: its first launch (k_gate in shard
    // mode) ran, k_shard_walk follows the exchange (abnn_shard_apply)
    bool pending_walk = false;
    // the sharded lastVisited merge: a track_visits shard marks
    // the neurons it visits (d.visit_mark); marks_dirty = a pass ran since the
    // last merge or host write of lastVisited
    bool marks_dirty = false;
    uint64_t renorms = 0;  // renormalisations run (abnn_renormalisations)
    // a structural update that failed part-way left the records invalid (the
    // compaction works in place): every pass is refused until they are
    // reloaded (abnn_load_bnn / abnn_load_flat / abnn_generate_synapses / an
    // upload of every record)
    bool records_invalid = false;
    IndexState ix;  // the indexed fused pass: src index, event mask, policy (index_* below)

    // On the handle's device.  The device memory goes with the pool; the rest
    // is the timing events and the error word.
    ~abnn_brain()
    {
        pool.release_all();
        for (auto& e : events) {
            (void)hipEventDestroy(e.a);
            (void)hipEventDestroy(e.b);
        }
        if (err_host) (void)hipHostFree(err_host);
    }
};

namespace {

// Pass functions run on the caller's stream (NULL = the default stream).
hipStream_t pick(abnn_brain*, void* s) { return static_cast<hipStream_t>(s); }

// A fused pass whose look-back wait gave up (never expected: every gate
// workgroup is resident, checked at create) reports it once, here, instead of
// hanging the GPU; the word is re-armed, so only that failure is reported.
abnn_status pass_error(abnn_brain* b)
{
    if (!b->err_host || __atomic_load_n(b->err_host, __ATOMIC_ACQUIRE) == 0) return ABNN_OK;
    __atomic_store_n(b->err_host, 0u, __ATOMIC_RELEASE);
    set_err("fused pass: a look-back wait timed out; the state after that pass is invalid "
            "(reload it: abnn_load_bnn / abnn_load_flat)");
    return ABNN_ERR_HIP;
}

// State accessors are synchronous: they wait for all work on the handle's
// device (whatever stream it was enqueued on), then copy on the default stream.
abnn_status sync_all(abnn_brain* b)
{
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());
    return pass_error(b);
}

void reorder_free(abnn_brain* b)
{
    ReorderScratch& r = b->reorder;
    b->pool.release(&r.pairs[0], &r.pairs[1], &r.rec, &r.counts, &r.seg_tomb, &r.state);
    r = ReorderScratch{};
}

#define ST_TRY(expr)                        \
    do {                                    \
        abnn_status _s = (expr);            \
        if (_s != ABNN_OK) return _s;       \
    } while (0)

// The tail of a synchronous call: `words` u64 of its device result to the host
// on the handle's stream, then the wait for them.
abnn_status read_words(abnn_brain* b, const uint64_t* dev, uint64_t* out_host, uint64_t words)
{
    HIP_TRY(hipMemcpyAsync(out_host, dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return ABNN_OK;
}

abnn_status ensure_idx_scratch(abnn_brain* b, uint64_t n) { return b->pool.grow(&b->idx_scratch, &b->idx_cap, n); }

// a src / dst range of a config: not set (count 0), or inside [0, n_nrn)
inline bool range_ok(uint32_t first, uint32_t count, uint64_t n_nrn) { return !count || (uint64_t)first + count <= n_nrn; }

// Device records are the packed src streams, dst and w (SynArrays, engine.h);
// abnn_synapse is the host interchange format.  Capacity `count` records.
abnn_status alloc_syn(DevicePool& pool, SynArrays* a, uint64_t count, bool random_mode)
{
    ST_TRY(pool.alloc(zeroed(&a->lo, count)));
    ST_TRY(pool.alloc(zeroed(&a->hi, hi_bytes(count))));
    if (random_mode) ST_TRY(pool.alloc(zeroed(&a->src32, count)));
    return pool.alloc(zeroed(&a->dw, count));
}

// Chunked copies between device arrays [first, first + n) and host records.
constexpr uint64_t kXferRecs = 1u << 22;

abnn_status records_d2h(const SynArrays& a, uint64_t first, uint64_t n, abnn_synapse* out)
{
    std::vector<uint32_t> s;
    std::vector<uint2> dw;
    DeviceTemp<uint32_t> st;  // the chunk's src values as u32, for the pack / unpack kernels
    if (n) ST_TRY(st.alloc(std::min<uint64_t>(kXferRecs, n)));
    for (uint64_t i = 0; i < n; i += kXferRecs) {
        const uint64_t m = std::min<uint64_t>(kXferRecs, n - i);
        s.resize(m);
        dw.resize(m);
        HIP_TRY(launch_unpack_src(a, st.dev, first + i, m, nullptr));
        HIP_TRY(hipMemcpy(s.data(), st.dev, m * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dw.data(), a.dw + first + i, m * 8, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < m; ++k) {
            float w;
            std::memcpy(&w, &dw[k].y, 4);
            out[i + k] = {s[k], dw[k].x, w, 0.0f};
        }
    }
    return ABNN_OK;
}

abnn_status records_h2d(const SynArrays& a, uint64_t first, uint64_t n, const abnn_synapse* in)
{
    std::vector<uint32_t> s;
    std::vector<uint2> dw;
    DeviceTemp<uint32_t> st;  // the chunk's src values as u32, for the pack / unpack kernels
    if (n) ST_TRY(st.alloc(std::min<uint64_t>(kXferRecs, n)));
    for (uint64_t i = 0; i < n; i += kXferRecs) {
        const uint64_t m = std::min<uint64_t>(kXferRecs, n - i);
        s.resize(m);
        dw.resize(m);
        for (uint64_t k = 0; k < m; ++k) {
            s[k] = in[i + k].src;
            dw[k].x = in[i + k].dst;
            std::memcpy(&dw[k].y, &in[i + k].w, 4);
        }
        HIP_TRY(hipMemcpy(st.dev, s.data(), m * 4, hipMemcpyHostToDevice));
        HIP_TRY(launch_pack_src(a, st.dev, first + i, m, nullptr));
        HIP_TRY(hipDeviceSynchronize());  // the staging buffer is reused
        HIP_TRY(hipMemcpy(a.dw + first + i, dw.data(), m * 8, hipMemcpyHostToDevice));
    }
    return ABNN_OK;
}

// Every record names two neurons, or is the pruning tombstone {src = dst =
// 0xFFFFFFFF} that downloads, .bnn and flat saves of a pruned brain hold
// between structural updates (abnn.h; k_pack_src maps it to kSrcNone).
abnn_status validate_records(const abnn_brain* b, const abnn_synapse* s, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i)
        if ((s[i].src >= b->n_nrn || s[i].dst >= b->n_nrn) &&
            !(s[i].src == 0xFFFFFFFFu && s[i].dst == 0xFFFFFFFFu)) {
            set_err("synapse " + std::to_string(i) + " has src/dst >= N_NRN (" +
                    std::to_string(b->n_nrn) + ")");
            return ABNN_ERR_INVALID;
        }
    return ABNN_OK;
}

// Host-written records may hold tombstones (a saved pruned brain): recount the
// structural update's per-block tally over them (structural updates on only:
// d.dead exists when compact_every > 0).
void index_invalidate(abnn_brain* b);

abnn_status retally(abnn_brain* b, uint64_t first, uint64_t n)
{
    index_invalidate(b);  // the records were written: their src may have changed
    if (!b->d.dead || n == 0) return ABNN_OK;
    HIP_TRY(launch_tally_dead(b->d.syn, b->dims.n_syn, b->d.dead, first, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    return ABNN_OK;
}

uint64_t tick_events(const abnn_brain* b)
{
    return b->dims.global_events ? b->dims.global_events : b->d.events;
}

// renormalise_if_needed (brain.cpp:127-128) on the pass-start clock: the
// reference's clock is a u32, so the test is on its low 32 bits
bool renorm_due(const abnn_brain* b) { return (uint64_t)(uint32_t)b->clock_host > b->params.renorm_thresh; }

constexpr const char* kRecordsInvalid =
    "a failed structural update left the records invalid: reload them (abnn_load_bnn / abnn_load_flat / "
    "abnn_generate_synapses / abnn_upload_synapses of every record) before the next pass";

// A shard that tracks visits keeps per-neuron visit marks for the lastVisited
// merge; allocated at creation when global_events is set, else
// by the first sharded pass (zeros: nothing visited yet).
abnn_status ensure_visit_marks(abnn_brain* b)
{
    if (!b->params.track_visits || b->d.visit_mark) return ABNN_OK;
    return b->pool.alloc(zeroed(&b->d.visit_mark, b->n_nrn));
}

void host_tick(abnn_brain* b)
{
    if (tick_events(b) > 0) b->clock_host += b->params.clock_inc;  // brain.metal:129
}

abnn_status time_begin(abnn_brain* b, hipStream_t s, EventPair** out)
{
    *out = nullptr;
    if (b->timing <= 0) return ABNN_OK;
    // sampling every n-th launch starts at the second one: the first launch
    // after enable_timing is the one most likely to carry a transient
    const uint64_t n = (uint64_t)b->timing, c = b->timing_count++;
    if (c % n != (n > 1 ? 1u : 0u)) return ABNN_OK;
    if (b->events_used == b->events.size()) {
        EventPair p;
        HIP_TRY(hipEventCreate(&p.a));
        HIP_TRY(hipEventCreate(&p.b));
        b->events.push_back(p);
    }
    *out = &b->events[b->events_used++];
    HIP_TRY(hipEventRecord((*out)->a, s));
    return ABNN_OK;
}

// Bytes of the sweep's record stream kept in the Infinity Cache from pass to
// pass (ABNN_STREAM_PIN_MB, MiB; 0 = none: every stream load non-temporal).
// profiles/ab_stream_pin.txt has the sweep over it.
constexpr uint64_t kStreamPinMiB = 160;  // config 3: 5 of 16, the best of the sweep
uint64_t stream_pin_bytes()
{
    uint64_t mib = kStreamPinMiB;
    if (const char* env = std::getenv("ABNN_STREAM_PIN_MB")) mib = (uint64_t)std::min(4096, std::max(0, std::atoi(env)));
    return mib << 20;
}

// The src index (index.h) holds only while the src of records [0, E) and E
// itself are what it was built from.  Every writer of a record's src, of a
// tombstone or of the record count calls this: upload, generate, the graph
// builder and the file loads (through retally), the edit's KILL, the reorder,
// a snapshot roll-back, the structural update, and configure when E changes.
// The buffers are freed; the index is built again after ABNN_INDEX_AFTER
// eligible passes.  (hipFree waits for the device: no pass still reads them.)
void index_invalidate(abnn_brain* b)
{
    IndexState& x = b->ix;
    if (x.row || x.off || x.mask || x.info || x.heavy || x.marked || x.marked_next || x.delta) {
        (void)hipSetDevice(b->device);
        b->pool.release(&x.row, &x.off, &x.mask, &x.info, &x.heavy, &x.marked, &x.marked_next, &x.delta);
    }
    x.delta_at = 0;
    x.heavy_chunks = 0;
    x.built = false;
    x.entries = 0;
    x.max_degree = 0;
    x.mask_words = 0;
    x.eligible = 0;
}

// Sweep partition for the current record count: visited events, wave
// iterations and the persistent gate grid (one range per wave).  Run at
// creation and after every structural update.
void configure(abnn_brain* b)
{
    DeviceState& d = b->d;
    d.n_syn = b->dims.n_syn;
    const uint64_t ev = visited_events(b->dims, b->params.mode);
    if (ev != d.events) index_invalidate(b);
    d.events = ev;
    const uint64_t iters = (d.events + d.iter_events - 1) / d.iter_events;
    d.iters = (uint32_t)iters;
    uint64_t G = std::min<uint64_t>(iters, std::min<uint64_t>((uint64_t)b->cus * b->per_cu, kMaxGateBlocks));
    // ranges are per wave; the last workgroup may own fewer than one iteration each
    const uint64_t waves = d.gate_block / 64;
    G = std::min<uint64_t>(G, (iters + waves - 1) / waves);
    if (G == 0 && iters > 0) G = 1;
    d.gate_blocks = (uint32_t)G;
    d.n_ranges = (uint32_t)(G * waves);  // <= kMaxGateBlocks * 16 = kMaxRanges
    // the slice of the 3 B/event record stream that fits the budget, in
    // sixteenths of the sweep (engine.h pin_k): config 3's 450 MB get 5 of 16
    // at 160 MiB, the full sweep's 3 GB none
    const uint64_t budget = stream_pin_bytes();
    d.pin_k = 0;
    if (d.events > 0 && b->params.mode == ABNN_MODE_SWEEP && !b->params.track_visits)
        d.pin_k = (uint32_t)std::min<uint64_t>(16, 16 * budget / (3 * d.events));
}

// Uniform sweep partition: range r starts at iteration floor(r * iters / NR)
// (k_apply then adapts it pass by pass, partition_bounds).
abnn_status reset_ranges(abnn_brain* b)
{
    const DeviceState& d = b->d;
    std::vector<uint32_t> rb(d.n_ranges + 1);
    for (uint32_t r = 0; r <= d.n_ranges; ++r) rb[r] = (uint32_t)((uint64_t)r * d.iters / std::max(1u, d.n_ranges));
    HIP_TRY(hipMemcpy(d.range_bounds, rb.data(), rb.size() * 4, hipMemcpyHostToDevice));
    return ABNN_OK;
}

// build_buffers, brain.cpp:52-69: allocate and zero every buffer of a new
// handle (its pool frees what a failure leaves), then the uniform partition.
// `slots`: the most events a pass visits, in whole wave iterations.
abnn_status brain_buffers(abnn_brain* b, uint64_t slots, uint64_t max_ranges, bool genesis)
{
    DeviceState& d = b->d;
    DevicePool& pool = b->pool;
    const abnn_params& p = b->params;
    const uint64_t n_nrn = b->n_nrn, cap = b->dims.syn_capacity;
    // padded: the gate's last iteration reads up to one iteration past the sweep
    ST_TRY(alloc_syn(pool, &d.syn, cap + kDummyRecords, p.mode == ABNN_MODE_RANDOM));
    ST_TRY(pool.alloc_all({zeroed(&d.last_fired, n_nrn), zeroed(&d.last_visited, n_nrn)}));
    // a shard (global_events set) that tracks visits marks them for the merge
    if (p.track_visits && b->dims.global_events) ST_TRY(pool.alloc(zeroed(&d.visit_mark, n_nrn)));
    uint64_t* sb = nullptr;
    ST_TRY(pool.alloc(zeroed(&sb, 3)));  // {clock, reward|rbar, pass_index}
    b->scalar_block = sb;
    d.clock = sb;
    d.reward = reinterpret_cast<float*>(sb + 1);
    d.rbar = d.reward + 1;
    d.pass_index = sb + 2;
    for (int i = 0; i < 3; ++i)
        ST_TRY(pool.alloc_all({zeroed(&b->bitmap_buf[i], d.n_bitmap_words + 2ull), zeroed(&b->filter_buf[i], 2 * kMaxFilterWords)}));
    d.bitmap = b->bitmap_buf[0];
    d.filter = b->filter_buf[0];
    uint32_t* dummy = nullptr;
    // g2x: per-range regions of refractory survivors (16 B per event: every
    // event of a range may pass in the warm-up passes)
    ST_TRY(pool.alloc_all({zeroed(&b->cost_buf[0], max_ranges), zeroed(&b->cost_buf[1], max_ranges),
                           zeroed(&d.lb_status, kMaxGateBlocks), zeroed(&d.cand_list, (uint64_t)kFusedMaxRanges * kCandCap),
                           zeroed(&d.range_info, max_ranges), zeroed(&d.range_g1, max_ranges), zeroed(&d.g2x, slots),
                           zeroed(&d.chunk_cnt, slots / kChunkSlotDiv + 8), zeroed(&dummy, 2 * kDummyRecords),
                           zeroed(&d.wg_stats, kWalkBlocks)}));
    d.dummy = dummy;
    if (p.mode == ABNN_MODE_RANDOM) ST_TRY(pool.alloc(zeroed(&d.claim, cap)));
    if (p.compact_every > 0) {
        // structural updates (in place): the span's offsets (<= nb used, + slack), the scan's sums, the tail blocks'
        // prefix (+ 1 <= nb + 2), the device words; the tombstone tally: pruning's, and an upload's (a saved pruned brain)
        const uint64_t nb = (cap + kCompactChunk - 1) / kCompactChunk;
        ST_TRY(pool.alloc_all({zeroed(&b->compact_offsets, nb + 4), zeroed(&b->swap_part, (nb + kScanThreads - 1) / kScanThreads + 1),
                               zeroed(&b->swap_toff, nb + 4), zeroed(&b->span_words, 8), zeroed(&d.dead, nb)}));
    }
    if (genesis) {
        const uint64_t grown = (uint64_t)p.compact_every * p.max_spikes;
        ST_TRY(pool.alloc_all({zeroed(&d.g2src, slots), zeroed(&d.grown, grown),
                               zeroed(&b->grown_cnt, (grown + kScanThreads - 1) / kScanThreads + 1)}));
    }
    ST_TRY(pool.alloc(zeroed(&d.work, 1)));
    if (hipHostMalloc(reinterpret_cast<void**>(&b->err_host), 4, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void**>(&d.err_word), b->err_host, 0) != hipSuccess) {
        set_err("hipHostMalloc (error word) failed");
        return ABNN_ERR_OOM;
    }
    *b->err_host = 0;
    ST_TRY(pool.alloc_all({zeroed(&b->u64_scratch, 4), zeroed(&d.wave_clock, (uint64_t)kWaveClockPasses * kWaveClock * kMaxRanges + 32),
                           zeroed(&d.apply_clock, 8 * (uint64_t)kWalkBlocks),
                           zeroed(&d.fired_ring, (uint64_t)kFiredRing * std::max(1u, p.max_spikes)),
                           zeroed(&d.n_fired_ring, kFiredRing), zeroed(&d.range_bounds, max_ranges + 1),
                           zeroed(&d.range_bounds_next, max_ranges + 1), zeroed(&d.range_bounds_prev, max_ranges + 1)}));
    return reset_ranges(b);
}

// The sweep partition after dims.n_syn changed (a structural update, a
// snapshot restore): configure, then the ranges.  The device is idle.
abnn_status repartition(abnn_brain* b)
{
    DeviceState& d = b->d;
    const uint32_t old_iters = d.iters, old_ranges = d.n_ranges;
    configure(b);
    if (d.n_ranges == old_ranges && old_iters > 0) {
        // the same ranges over (nearly) the same records: keep the adapted
        // partition -- rescaled if the sweep's length changed -- and the
        // measured costs, instead of restarting from a uniform partition
        // (a uniform one costs ~3 passes at several times the pass time)
        if (d.iters != old_iters) {
            std::vector<uint32_t> rb(d.n_ranges + 1);
            for (uint32_t* buf : {d.range_bounds, d.range_bounds_prev}) {
                HIP_TRY(hipMemcpy(rb.data(), buf, rb.size() * 4, hipMemcpyDeviceToHost));
                for (auto& v : rb) v = (uint32_t)((uint64_t)v * d.iters / old_iters);
                rb[d.n_ranges] = d.iters;
                HIP_TRY(hipMemcpy(buf, rb.data(), rb.size() * 4, hipMemcpyHostToDevice));
            }
        }
        return ABNN_OK;
    }
    b->last_pass_fused = false;  // new ranges: the measured costs do not apply
    return reset_ranges(b);
}

// README §5 structural update (contract in abnn.h): the tombstones' span
// [a, z) closes up in order and the hole at its end takes the array's last D
// records (or the tail shifts down), then the grown records are appended in
// (pass, slot) order while capacity lasts.  Synchronous; runs between passes.
// Only the span and D records move: the tally's bounds give the span's blocks,
// whose live records move down to their final places in place (one pass over
// the span, no spare buffer), so a sweep's update costs O(events), not
// O(n_syn), and the records take their own size in HBM, not twice it.
abnn_status structural_update(abnn_brain* b)
{
    DeviceState& d = b->d;
    const uint64_t n = b->dims.n_syn, cap = b->dims.syn_capacity;
    ST_TRY(sync_all(b));
    const uint64_t nb = (n + kCompactChunk - 1) / kCompactChunk;
    const uint64_t slots = d.grown ? (uint64_t)b->params.compact_every * b->params.max_spikes : 0;
    // the whole update on the device (kernels.hip launch_structural_update):
    // the tally's span, its offsets, the in-place compaction, the hole, the
    // grown records; one synchronisation reads D and the records appended
    *b->err_host = 0;
    unsigned long long* sp = b->span_words;
    hipError_t e = launch_structural_update(d.syn, n, cap, d.dead, nb, b->compact_offsets, b->swap_part, b->swap_toff,
                                            sp, d.err_word, (uint32_t)b->cus, d.grown, slots, b->grown_cnt,
                                            reinterpret_cast<unsigned long long*>(&d.work->stats.grown), nullptr);
    unsigned long long w[5] = {0, 0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(w, sp, sizeof(w), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        b->records_invalid = true;  // the update may have stopped part-way through its in-place moves
        set_err(std::string("structural update: ") + hipGetErrorString(e) +
                "; the records are not valid, reload them (abnn_load_bnn / abnn_load_flat)");
        return ABNN_ERR_HIP;
    }
    if (const uint32_t err = *b->err_host) {
        // the compaction moves records in place, so a part-done update cannot
        // be rolled back: passes are refused until the records are reloaded
        *b->err_host = 0;
        b->records_invalid = true;
        set_err("structural update: the tombstone tally and the records disagree; "
                "the records are not valid, reload them (abnn_load_bnn / abnn_load_flat)");
        return ABNN_ERR_HIP;
    }
    b->dims.n_syn = n - w[2] + w[4];
    b->structural_updates += 1;
    // (an update that found no tombstone and appended nothing moved no record: the index holds;
    // when E changes, configure drops it as well)
    if (w[2] != 0 || w[4] != 0) index_invalidate(b);
    return repartition(b);
}

// A host write to lastFired (or a clock change) up to `stamp`: the recent-spike
// bitmap is rebuilt from all of lastFired (k_bitmap) until k_apply's build is
// exact again.
void state_written(abnn_brain* b, uint64_t stamp)
{
    b->clean_passes = 0;
    b->max_host_stamp = std::max(b->max_host_stamp, stamp);
    b->next_built = false;
}

// k_apply of pass p may build pass p+1's bitmap from the spike lists
// (kernels.hip, build_next_lists) iff: the clock advances by one per pass; the
// last window_pre - 1 passes were single-GPU passes after the last
// discontinuity, so their spike lists are in fired_ring; and no value the
// host wrote is recent at pass p+1 (clock >= max_host_stamp + window_pre).
bool build_next_ok(const abnn_brain* b)
{
    const uint64_t W = b->params.window_pre;
    return !b->ext_ptrs && !b->force_full_bitmap && b->params.clock_inc == 1 && W >= 1 && W < kFiredRing &&
           b->clean_passes + 1 >= W && b->clock_host >= b->max_host_stamp + W &&
           b->clock_host + W < (1ull << 32);  // ages are u32 (age32): the stamp order above holds below 2^32
}

// This pass's recent-spike buffers (triple-buffered by pass % 3) and, unless
// the previous pass built them, the bitmap from lastFired (k_bitmap).
abnn_status pass_buffers(abnn_brain* b, hipStream_t s, bool* was_prebuilt = nullptr)
{
    DeviceState& d = b->d;
    const uint64_t p = b->rot;  // not pass_host: set_scalars may move that
    d.bitmap = b->bitmap_buf[p % 3];
    d.filter = b->filter_buf[p % 3];
    d.bitmap_next = b->bitmap_buf[(p + 1) % 3];
    d.filter_next = b->filter_buf[(p + 1) % 3];
    d.bitmap_clear = b->bitmap_buf[(p + 2) % 3];
    d.filter_clear = b->filter_buf[(p + 2) % 3];
    d.stim_first = b->stim_first;
    d.stim_count = b->stim_count;
    const bool prebuilt = b->next_built && b->built_stim[0] == b->stim_first &&
                          b->built_stim[1] == b->stim_count;
    b->next_built = false;
    if (was_prebuilt) *was_prebuilt = prebuilt;
    if (!prebuilt) HIP_TRY(launch_bitmap(d, b->kp, b->stim_first, b->stim_count, s));
    b->stim_ring[b->pass_host % kFiredRing][0] = b->stim_first;
    b->stim_ring[b->pass_host % kFiredRing][1] = b->stim_count;
    return ABNN_OK;
}

// Whether this pass builds the next one's bitmap, and from which stimulus ranges.
void plan_build(abnn_brain* b)
{
    DeviceState& d = b->d;
    d.build_next = build_next_ok(b) ? 1u : 0u;
    d.n_next_stim = 0;
    if (d.build_next) {  // distinct stimulus ranges of passes p+1-W .. p+1 (p+1: the current one)
        const uint64_t W = b->params.window_pre, p = b->pass_host;
        auto add = [&](uint64_t f, uint64_t c) {
            if (c == 0) return;
            for (uint32_t r = 0; r < d.n_next_stim; ++r)
                if (d.next_stim[r][0] == f && d.next_stim[r][1] == c) return;
            d.next_stim[d.n_next_stim][0] = f;
            d.next_stim[d.n_next_stim++][1] = c;
        };
        for (uint64_t q = p + 1 - W; q <= p; ++q) add(b->stim_ring[q % kFiredRing][0], b->stim_ring[q % kFiredRing][1]);
        add(b->stim_first, b->stim_count);
    }
}

// Handles that may run indexed passes: sweep mode, single GPU, none of
// track_visits, pruning, synaptogenesis; the lean fused instance; record
// arrays never handed out; E below 2^32 (off[] holds u32 offsets) and the
// index within ABNN_INDEX_MAX_MB.
uint64_t index_bytes(const abnn_brain* b)
{
    // off, row, the mask, the marked set's two buffers, the mark's two counter blocks and info.  The heavy list is
    // not in it: its length is known only after the build (16 B per 1024 entries of a list above kHeavyLen).
    return 4 * b->d.events + 4 * (b->n_nrn + 1) + 4 * index_mask_words(b->d.iters, b->d.iter_events) +
           2 * 4 * (uint64_t)b->d.n_bitmap_words + 2 * 4 * 4 * (uint64_t)kDeltaSlots + 4 * 4;
}

bool index_eligible(const abnn_brain* b)
{
    const DeviceState& d = b->d;
    const abnn_params& p = b->params;
    const bool plastic = p.w_prune > 0.0f || (d.grown != nullptr && p.p_new > 0.0f);
    return b->ix.mode != 0 && p.mode == ABNN_MODE_SWEEP && !p.track_visits && !plastic && d.lean && !d.g2src &&
           !b->ext_ptrs && b->dims.global_events == 0 && d.events > 0 && d.events < (1ull << 32) &&
           index_bytes(b) <= (b->ix.max_mb << 20);
}

// The default rule (ABNN_INDEXED=1).  When this pass's bitmap was built from
// the spike lists (build_next_ok held when the previous pass built it), the
// recent set holds at most window_pre x (max_spikes + stimulus count) neurons
// (the largest stimulus of the window's passes): the pass is indexed iff that
// bound times the index's largest degree is at most E / 8.  A bitmap from
// k_bitmap (the first passes, where lastFired = 0 makes every neuron recent;
// host writes) has no such bound: the pass streams.
bool index_pass_rule(const abnn_brain* b, bool prebuilt)
{
    if (!prebuilt) return false;
    const uint64_t W = b->params.window_pre, p = b->pass_host;
    uint64_t stim = b->stim_count;
    for (uint64_t q = p >= W ? p - W : 0; q <= p; ++q) stim = std::max(stim, b->stim_ring[q % kFiredRing][1]);
    const uint64_t bound = W * ((uint64_t)b->params.max_spikes + stim);
    return bound * b->ix.max_degree <= b->d.events / 8;
}

// Builds the index on the pass's stream, with one read-back (the largest
// degree and the entry count) and a HIP event pair around its launches.  No
// memory for it: the handle goes on streaming (ABNN_INDEXED=0 from here on).
abnn_status index_build(abnn_brain* b, hipStream_t s)
{
    IndexState& x = b->ix;
    const DeviceState& d = b->d;
    index_invalidate(b);
    DeviceTemp<uint32_t> cursor, part;
    x.mask_words = index_mask_words(d.iters, d.iter_events);
    abnn_status st = b->pool.alloc_all({raw(&x.row, b->n_nrn + 1), raw(&x.off, d.events), zeroed(&x.mask, x.mask_words),
                                        zeroed(&x.info, 4), zeroed(&x.marked, d.n_bitmap_words),
                                        zeroed(&x.marked_next, d.n_bitmap_words), zeroed(&x.delta, 2 * 4 * kDeltaSlots)});
    if (st == ABNN_OK) st = cursor.alloc(b->n_nrn + 1, false);
    if (st == ABNN_OK) st = part.alloc(index_tiles(b->n_nrn) + 1, false);
    if (st != ABNN_OK) {
        index_invalidate(b);
        x.mode = 0;
        return st == ABNN_ERR_OOM ? ABNN_OK : st;
    }
    hipEvent_t ea = nullptr, eb = nullptr;
    HIP_TRY(hipEventCreate(&ea));
    hipError_t e = hipEventCreate(&eb);
    uint32_t info[4] = {0, 0, 0, 0};
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventRecord(ea, s);
    if (e == hipSuccess) e = launch_index_build(d.syn, d.events, b->n_nrn, x.row, cursor.dev, part.dev, x.off, x.info, (uint32_t)b->cus, s);
    if (e == hipSuccess) e = hipEventRecord(eb, s);
    if (e == hipSuccess) e = hipMemcpyAsync(info, x.info, sizeof(info), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ea, eb);
    (void)hipEventDestroy(ea);
    if (eb) (void)hipEventDestroy(eb);
    HIP_TRY(e);
    x.max_degree = info[0];
    x.entries = info[1];
    x.build_ms = ms;
    if (info[2]) {  // the heavy list (the build's time leaves this one small launch out)
        st = b->pool.alloc(raw(&x.heavy, info[2]));
        if (st != ABNN_OK) {
            index_invalidate(b);
            x.mode = 0;
            return st == ABNN_ERR_OOM ? ABNN_OK : st;
        }
        HIP_TRY(launch_index_heavy(x.row, b->n_nrn, x.heavy, info[2], x.info, s));
    }
    x.heavy_chunks = info[2];
    x.built = true;
    return ABNN_OK;
}

// A sharded pass takes the fused path (two launches around the exchange:
// k_gate in shard mode, k_shard_walk) where a single-GPU pass would.
bool shard_fused(const abnn_brain* b)
{
    return b->use_fused && fused_pass_supported(b->d) && b->d.gate_block == 1024;
}

abnn_status run_shard_fused_gate(abnn_brain* b, int32_t* xchg, hipStream_t s);

// bitmap + streaming gate (with the refractory stage) [+ the exchange record
// of a sharded pass]: the first half of every pass.
abnn_status run_gate(abnn_brain* b, int32_t* xchg_out, hipStream_t s)
{
    if (xchg_out && shard_fused(b)) return run_shard_fused_gate(b, xchg_out, s);
    ST_TRY(pass_buffers(b, s));
    b->last_pass_fused = false;
    b->ix.eligible = 0;  // not an eligible pass (index_eligible): the count is of consecutive ones
    b->ix.last_indexed = false;
    b->ix.flavour = 0;
    EventPair* ev = nullptr;
    ST_TRY(time_begin(b, s, &ev));
    HIP_TRY(launch_gate(b->d, b->kp, s));
    if (ev) HIP_TRY(hipEventRecord(ev->b, s));
    if (xchg_out) HIP_TRY(launch_scan(b->d, b->kp, xchg_out, s));
    return ABNN_OK;
}

// After a pass: the partition it computed for the next one becomes current
// (kernel arguments are captured at launch), its own becomes the previous one.
void rotate_bounds(abnn_brain* b)
{
    DeviceState& d = b->d;
    uint32_t* prev = d.range_bounds_prev;
    d.range_bounds_prev = d.range_bounds;
    d.range_bounds = d.range_bounds_next;
    d.range_bounds_next = prev;
}

// budget walk, weight update, stamps, pass end; k_apply writes the next
// pass's partition into range_bounds_next (rotate_bounds)
abnn_status run_apply(abnn_brain* b, const int32_t* gathered, uint32_t world, uint32_t rank, hipStream_t s)
{
    DeviceState& d = b->d;
    if (b->pending_walk) {  // the sharded fused pass's second launch
        b->pending_walk = false;
        HIP_TRY(launch_shard_walk(d, b->kp, gathered, world, rank, s));
        b->next_built = d.build_next != 0;
        b->built_stim[0] = b->stim_first;
        b->built_stim[1] = b->stim_count;
        rotate_bounds(b);
        return ABNN_OK;
    }
    plan_build(b);
    HIP_TRY(launch_apply(d, b->kp, gathered, world, rank, s));
    b->next_built = d.build_next != 0;
    b->built_stim[0] = b->stim_first;
    b->built_stim[1] = b->stim_count;
    rotate_bounds(b);
    return ABNN_OK;
}

// The whole single-GPU sweep pass in one launch (kernels.hip, k_gate<...,
// kFused>): gate, look-back budget walk, weight update, stamps, pass end.  Its
// prologue computes the next pass's partition (range_bounds_next) from the
// previous fused pass's gate costs.
//
// The pass is indexed (DESIGN.md §5 "Indexed pass": k_index_mark, then the
// mask flavour of the same launch) iff the handle is eligible, the index is
// valid and the rule admits it; otherwise it streams.  Results never depend on
// the choice.  The host decides from what it knows without reading the device.
abnn_status run_fused(abnn_brain* b, hipStream_t s)
{
    DeviceState& d = b->d;
    IndexState& x = b->ix;
    const bool eligible = index_eligible(b);
    if (eligible && !x.built && x.eligible >= x.after) ST_TRY(index_build(b, s));
    bool prebuilt = false;
    ST_TRY(pass_buffers(b, s, &prebuilt));
    plan_build(b);
    const bool indexed = eligible && x.built && (x.mode == 2 || index_pass_rule(b, prebuilt));
    // the partition adapts on the costs of its own flavour: after a change of
    // flavour the bounds stay for one pass (fused_next_bounds copies them)
    d.prologue_adapt = b->last_pass_fused && x.flavour == (indexed ? 1 : 0) && d.adapt_ranges ? 1u : 0u;
    d.cost_in = b->cost_buf[b->cost_parity ^ 1u];
    d.cost_out = b->cost_buf[b->cost_parity];
    d.indexed = indexed ? 1u : 0u;
    d.ev_mask = x.mask;
    EventPair* ev = nullptr;
    ST_TRY(time_begin(b, s, &ev));
    hipError_t e = hipSuccess;
    if (indexed) {
        // the delta mark: the mask moves from the marked set to this pass's bitmap, which is the marked set from here on
        // (a launch that failed moved nothing: the buffers and the counter blocks stay as they are)
        const uint32_t at = x.delta_at ^ 4u * kDeltaSlots;
        e = launch_index_mark(d.bitmap, x.marked, x.marked_next, d.n_bitmap_words, d.n_nrn, x.row, x.off, x.mask, d.events,
                              x.heavy, x.heavy_chunks, x.delta + at, x.delta + x.delta_at, s);
        if (e == hipSuccess) {
            std::swap(x.marked, x.marked_next);
            x.delta_at = at;
        }
    }
    if (e == hipSuccess) e = launch_fused_pass(d, b->kp, s);
    d.indexed = 0u;
    HIP_TRY(e);
    if (ev) HIP_TRY(hipEventRecord(ev->b, s));
    x.flavour = indexed ? 1 : 0;
    x.last_indexed = indexed;
    x.indexed_passes += indexed ? 1u : 0u;
    x.eligible = eligible ? x.eligible + 1 : 0;
    b->next_built = d.build_next != 0;
    b->built_stim[0] = b->stim_first;
    b->built_stim[1] = b->stim_count;
    rotate_bounds(b);
    b->cost_parity ^= 1u;
    b->last_pass_fused = true;
    return ABNN_OK;
}

// The first launch of a sharded pass on the fused path: gate, refractory
// stage, look-back over this shard's workgroups with local budget positions,
// this shard's exchange record (kernels.hip fused_end, shard mode).  Like
// run_fused, but the walk, the stamps and the pass end wait for the exchange.
abnn_status run_shard_fused_gate(abnn_brain* b, int32_t* xchg, hipStream_t s)
{
    DeviceState& d = b->d;
    ST_TRY(pass_buffers(b, s));
    plan_build(b);
    d.prologue_adapt = b->last_pass_fused && d.adapt_ranges ? 1u : 0u;
    d.cost_in = b->cost_buf[b->cost_parity ^ 1u];
    d.cost_out = b->cost_buf[b->cost_parity];
    d.shard_mode = 1;
    d.xchg = xchg;
    b->ix.eligible = 0;  // a sharded pass streams; its costs are the stream flavour's
    b->ix.last_indexed = false;
    b->ix.flavour = 0;
    EventPair* ev = nullptr;
    ST_TRY(time_begin(b, s, &ev));
    const hipError_t e = launch_fused_pass(d, b->kp, s);
    d.shard_mode = 0;
    d.xchg = nullptr;
    HIP_TRY(e);
    if (ev) HIP_TRY(hipEventRecord(ev->b, s));
    b->cost_parity ^= 1u;
    b->last_pass_fused = true;
    b->pending_walk = true;
    return ABNN_OK;
}

abnn_status run_commit(abnn_brain* b, const int32_t* gathered, uint32_t world, bool renorm,
                       hipStream_t s)
{
    // the spike recorder: this pass's list, with the mirrors' values before the tick, the +1 and the renormalisation
    if (b->spikes.on) {
        const uint64_t slot = b->pass_host & (kFiredRing - 1);
        HIP_TRY(launch_spike_record(b->spikes, b->d.fired_ring + slot * (uint64_t)b->params.max_spikes,
                                    b->d.n_fired_ring + slot, b->params.max_spikes, b->pass_host, b->clock_host,
                                    (uint32_t)b->renorms, s));
    }
    host_tick(b);
    // sharded passes write the merged spike list into fired_ring too
    b->clean_passes += 1;
    if (renorm) {  // renormalise_if_needed, brain.cpp:125-141; kernel brain.metal:135-145
        HIP_TRY(launch_renorm(b->d, b->clock_host, s));
        b->renorms += 1;
        const uint64_t base = b->clock_host;
        b->max_host_stamp = b->max_host_stamp > base ? b->max_host_stamp - base : 0;
        b->clean_passes = 0;  // the clock jumps back
        b->next_built = false;
        b->clock_host = 0;
    }
    b->last_pass = b->pass_host;
    b->pass_host += 1;
    b->rot += 1;
    const uint32_t ce = b->params.compact_every;
    if (ce != 0 && b->pass_host % ce == 0) ST_TRY(structural_update(b));  // README §5
    return ABNN_OK;
}

// One whole single-GPU pass (abnn_traverse's loop body, abnn_engine_run
// between its boundary launches): the fused launch where the shape has one,
// else gate + apply; then the commit.
abnn_status run_pass(abnn_brain* b, hipStream_t s)
{
    // the host reads the clock at encode time, before the pass (brain.cpp:127-128)
    const bool renorm = renorm_due(b);
    if (b->use_fused && fused_pass_supported(b->d)) {
        ST_TRY(run_fused(b, s));
    } else {
        ST_TRY(run_gate(b, nullptr, s));
        ST_TRY(run_apply(b, nullptr, 1, 0, s));
    }
    return run_commit(b, nullptr, 1, renorm, s);
}

// RCCL entry points, resolved once: the librccl already loaded in the process
// (torch's, when the caller imported it: one RCCL per process), else the
// system's librccl.so.1.
struct RcclApi {
    ncclResult_t (*get_unique_id)(ncclUniqueId*);
    ncclResult_t (*comm_init_rank)(ncclComm_t*, int, ncclUniqueId, int);
    ncclResult_t (*comm_destroy)(ncclComm_t);
    ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
    ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    const char* (*error_string)(ncclResult_t);
    bool ok;
};

int find_loaded_rccl(struct dl_phdr_info* info, size_t, void* out)
{
    if (info->dlpi_name && std::strstr(info->dlpi_name, "librccl.so")) {
        *static_cast<std::string*>(out) = info->dlpi_name;
        return 1;
    }
    return 0;
}

const RcclApi& rccl_api()
{
    static RcclApi api = [] {
        RcclApi a{};
        std::string loaded;
        dl_iterate_phdr(find_loaded_rccl, &loaded);
        void* h = loaded.empty() ? nullptr : dlopen(loaded.c_str(), RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return a;
        a.get_unique_id = reinterpret_cast<decltype(a.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
        a.comm_init_rank = reinterpret_cast<decltype(a.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
        a.comm_destroy = reinterpret_cast<decltype(a.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        a.all_gather = reinterpret_cast<decltype(a.all_gather)>(dlsym(h, "ncclAllGather"));
        a.all_reduce = reinterpret_cast<decltype(a.all_reduce)>(dlsym(h, "ncclAllReduce"));
        a.error_string = reinterpret_cast<decltype(a.error_string)>(dlsym(h, "ncclGetErrorString"));
        a.ok = a.get_unique_id && a.comm_init_rank && a.comm_destroy && a.all_gather && a.all_reduce && a.error_string;
        return a;
    }();
    return api;
}

#define RCCL_TRY(expr)                                                                 \
    do {                                                                               \
        ncclResult_t _r = (expr);                                                      \
        if (_r != ncclSuccess) {                                                       \
            set_err(std::string(#expr) + ": " + rccl_api().error_string(_r));          \
            return ABNN_ERR_HIP;                                                       \
        }                                                                              \
    } while (0)

// Chunked host<->device copies for the file formats.
constexpr uint64_t kIoRecs = 1u << 22;  // 4M records (64 MiB) per piece

}  // namespace

extern "C" {

int abnn_abi_version(void) { return ABNN_ABI_VERSION; }

const char* abnn_status_string(abnn_status s)
{
    switch (s) {
        case ABNN_OK: return "ok";
        case ABNN_ERR_INVALID: return "invalid argument";
        case ABNN_ERR_HIP: return "HIP runtime error";
        case ABNN_ERR_OOM: return "out of memory";
        case ABNN_ERR_SIZE_MISMATCH: return "size mismatch";
        case ABNN_ERR_IO: return "I/O error";
        case ABNN_ERR_NO_DEVICE: return "no HIP device";
    }
    return "unknown status";
}

const char* abnn_last_error(void) { return g_err.c_str(); }

void abnn_default_params(abnn_params* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->base_scale = 0.8f;         // brain.metal:22
    p->refractory = 2u;           // brain.metal:23
    p->window_pre = 5u;           // brain.metal:24
    p->clock_inc = 1u;            // brain.metal:26
    p->target_rate_hz = 1000.0f;  // brain.metal:28
    p->eta_home = 1.0e-6f;        // brain.metal:29
    p->eta_reward = 1.0e-3f;      // brain.metal:30
    p->alpha_rbar = 0.001f;       // brain.metal:31
    p->a_ltp = 0.04f;             // constants.h:16
    p->a_ltd = 0.02f;             // constants.h:17
    p->w_min = 0.001f;            // constants.h:18
    p->w_max = 1.0f;              // constants.h:19
    p->max_spikes = 2560u;        // brain.h:18
    p->tick_ns = 1000u;           // brain.h:17
    p->tau_vis = 50000u;          // brain.cpp:102
    p->tau_pre = 50000u;          // brain.cpp:102
    p->renorm_thresh = 4000000u;  // brain.h:19
    p->track_visits = 0u;
    p->seed = 1u;
}

int abnn_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

abnn_status abnn_brain_create(const abnn_dims* dims, const abnn_params* params, int device,
                              abnn_brain** out)
{
    REQUIRE(dims && out, "null argument");
    *out = nullptr;
    REQUIRE(dims->n_input > 0 || dims->n_output > 0 || dims->n_hidden > 0, "no neurons");
    const uint64_t n_nrn = (uint64_t)dims->n_input + dims->n_output + dims->n_hidden;
    REQUIRE(n_nrn < kMaxNeurons, "N_NRN must be below 2^24 - 1 (src is held in 24 bits on the device, DESIGN.md 4)");
    abnn_params p;
    if (params) p = *params;
    else abnn_default_params(&p);
    REQUIRE(p.max_spikes < (1u << 30), "max_spikes too large");
    REQUIRE(p.mode == ABNN_MODE_SWEEP || p.mode == ABNN_MODE_RANDOM, "unknown mode");
    const uint64_t cap = std::max<uint64_t>(dims->syn_capacity, dims->n_syn);  // 0 = creation size
    abnn_dims dmax = *dims;
    dmax.n_syn = cap;
    const uint64_t E = visited_events(dmax, p.mode);  // the most events a pass can visit
    REQUIRE(p.mode != ABNN_MODE_RANDOM || E < 0xFFFFFFFFull, "random mode: events per pass must fit u32");
    const bool genesis = p.p_new > 0.0f && p.compact_every > 0;
    // Gate kernel shape: threads per workgroup x events per lane x KiB per LDS
    // filter image (ABNN_GATE="1024x16f32"; tuning knob, the default is the measured best:
    // profiles/r01s_shape_sweep.txt).
    uint32_t gate_block = 1024, gate_k = 8, filter_kib = 32;  // profiles/r03l_ab_k8.txt: 1024x8 -1.7 us against 1024x16
    if (const char* env = std::getenv("ABNN_GATE")) {
        unsigned gb = 0, gk = 0, fk = 0;
        const int got = std::sscanf(env, "%ux%uf%u", &gb, &gk, &fk);
        if (got >= 2) {
            gate_block = gb;
            gate_k = gk;
            if (got == 3) filter_kib = fk;
        }
    }
    const uint32_t filter_words = filter_kib * 256;
    REQUIRE(gate_shape_supported(gate_block, gate_k, filter_words), "unsupported ABNN_GATE shape");
    const uint64_t iter_events = 64ull * gate_k;  // one wave iteration
    const uint64_t iters = (E + iter_events - 1) / iter_events;
    REQUIRE(iters < 0x7FFFFFFFull, "too many events for one handle");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_err("no HIP device visible");
        return ABNN_ERR_NO_DEVICE;
    }
    REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");

    HIP_TRY(hipSetDevice(device));
    abnn_brain* b = new (std::nothrow) abnn_brain();
    if (!b) return ABNN_ERR_OOM;
    b->dims = *dims;
    b->dims.syn_capacity = cap;
    b->params = p;
    b->kp = to_kernel_params(p);
    b->device = device;
    b->n_nrn = n_nrn;
    b->rng = p.seed;
    DeviceState& d = b->d;
    d.n_nrn = n_nrn;
    d.n_input = dims->n_input;
    d.syn_offset = dims->syn_offset;
    d.seed = p.seed;
    d.mode = p.mode;
    d.gate_block = gate_block;
    d.gate_k = gate_k;
    d.iter_events = (uint32_t)iter_events;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    // one wave of persistent workgroups: as many as are resident (each keeps the
    // 64 KiB filter in LDS, so at most two per CU)
    int per_cu = gate_blocks_per_cu(gate_block, gate_k, filter_words, p.track_visits != 0,
                                    p.mode == ABNN_MODE_RANDOM);
    if (per_cu <= 0) per_cu = 1;
    if (per_cu > 4) per_cu = 4;
    // at most kFusedMaxRanges ranges (the fused pass's partition prefix in LDS)
    per_cu = std::min<int>(per_cu, std::max<int>(1, (int)(kFusedMaxRanges / ((uint32_t)cus * (gate_block / 64)))));
    b->cus = cus;
    b->per_cu = per_cu;
    // partition A-B knobs: wave -> range map, adaptation gain
    if (const char* env = std::getenv("ABNN_RANGE_MAP")) d.range_map = std::atoi(env) ? 1u : 0u;
    d.adapt_gain = 1;  // profiles/r03g_*: 1 with tail priority 0 is -1 us against 2 with the rank kept
    if (const char* env = std::getenv("ABNN_ADAPT_GAIN")) d.adapt_gain = (uint32_t)std::min(4, std::max(1, std::atoi(env)));
    d.chunk_penalty = 600;  // 24 us per full chunk: the dense input->output stretch spread over more
                            // ranges (ABNN_CHUNK_PENALTY: 25 -> 350 measured -6 us per pass in round 2;
                            // 600 with the 1024x8 gate, profiles/r03l_ab_k8.txt)
    d.apply_blocks = kWalkBlocks;
    if (const char* env = std::getenv("ABNN_APPLY_BLOCKS"))
        d.apply_blocks = (uint32_t)std::min<int>(kWalkBlocks, std::max(1, std::atoi(env)));
    if (const char* env = std::getenv("ABNN_CHUNK_PENALTY")) d.chunk_penalty = (uint32_t)std::max(0, std::atoi(env));
    d.fused_max_blocks = (uint32_t)std::max(0, fused_blocks_per_cu(gate_block, gate_k, filter_words, p.track_visits != 0)) *
                         (uint32_t)cus;
    configure(b);  // sweep partition for the creation size
    const uint64_t max_ranges = (uint64_t)std::min<int>(kMaxGateBlocks, cus * per_cu) * (gate_block / 64);
    d.n_bitmap_words = (uint32_t)(2 * ((n_nrn + 63) / 64));
    d.filter_words = filter_words;
    d.filter_log2 = (uint32_t)__builtin_ctz(filter_words);
    if (const char* env = std::getenv("ABNN_FUSED")) b->use_fused = std::atoi(env) != 0;
    d.spec_mode = 1;
    d.spec_margin = -1;
    if (const char* env = std::getenv("ABNN_SPEC_MARGIN")) d.spec_margin = std::atoi(env);
    d.flush_at = kChunk;
    if (const char* env = std::getenv("ABNN_FLUSH_AT"))
        d.flush_at = (uint32_t)std::min<int>((int)kChunk, std::max(64, std::atoi(env)));
    d.lean = 1;
    if (const char* env = std::getenv("ABNN_LEAN")) d.lean = std::atoi(env) != 0;
    if (const char* env = std::getenv("ABNN_SPEC")) d.spec_mode = (uint32_t)std::min(2, std::max(0, std::atoi(env)));
    b->force_full_bitmap = std::getenv("ABNN_FULL_BITMAP") != nullptr;
    // the indexed pass: 0 never, 1 the rule (default), 2 whenever the index is valid
    if (const char* env = std::getenv("ABNN_INDEXED")) b->ix.mode = std::min(2, std::max(0, std::atoi(env)));
    if (const char* env = std::getenv("ABNN_INDEX_AFTER")) b->ix.after = (uint32_t)std::max(0, std::atoi(env));
    if (const char* env = std::getenv("ABNN_INDEX_MAX_MB")) b->ix.max_mb = (uint64_t)std::max(0, std::atoi(env));
    d.adapt_ranges = std::getenv("ABNN_STATIC_RANGES") ? 0u : 1u;
    b->select_blocks = 4u * (uint32_t)std::max(1, b->cus);  // 32 waves per CU, as the census
    if (const char* env = std::getenv("ABNN_SELECT_BLOCKS")) b->select_blocks = (uint32_t)std::max(1, std::atoi(env));
    b->edit_blocks = 4u * (uint32_t)std::max(1, b->cus);  // as the select
    if (const char* env = std::getenv("ABNN_EDIT_BLOCKS")) b->edit_blocks = (uint32_t)std::max(1, std::atoi(env));
    if (const char* env = std::getenv("ABNN_EDIT_NT")) b->edit_nt = std::atoi(env) != 0;
    b->reorder_blocks = 4u * (uint32_t)std::max(1, b->cus);  // as the select
    if (const char* env = std::getenv("ABNN_REORDER_BLOCKS")) b->reorder_blocks = (uint32_t)std::max(1, std::atoi(env));
    if (const char* env = std::getenv("ABNN_REORDER_SKIP")) b->reorder_skip = std::atoi(env) != 0;
    b->graph_blocks = 64u * (uint32_t)std::max(1, b->cus);  // measured: the finer grid evens the tail out
    if (const char* env = std::getenv("ABNN_GRAPH_BLOCKS")) b->graph_blocks = (uint32_t)std::max(1, std::atoi(env));
    if (const char* env = std::getenv("ABNN_GRAPH_NT")) b->graph_nt = std::atoi(env) != 0;
    const abnn_status s = brain_buffers(b, iters * iter_events, max_ranges, genesis);
    if (s != ABNN_OK) {
        delete b;
        return s;
    }
    *out = b;
    return ABNN_OK;
}

abnn_status abnn_brain_destroy(abnn_brain* b)
{
    if (!b) return ABNN_OK;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();
    delete b;
    return ABNN_OK;
}

abnn_status abnn_get_dims(const abnn_brain* b, abnn_dims* out)
{
    REQUIRE(b && out, "null argument");
    *out = b->dims;
    return ABNN_OK;
}

abnn_status abnn_get_params(const abnn_brain* b, abnn_params* out)
{
    REQUIRE(b && out, "null argument");
    *out = b->params;
    return ABNN_OK;
}

abnn_status abnn_state_ptrs(abnn_brain* b, abnn_state* out)
{
    REQUIRE(b && out, "null argument");
    // the caller may write lastFired or the clock behind the handle's back:
    // rebuild the recent-spike bitmap from lastFired every pass from now on
    b->ext_ptrs = true;
    index_invalidate(b);  // never used again (index_eligible): its memory goes now
    out->synapses = b->d.syn.lo;  // opaque (abnn_synapse_layout describes the arrays)
    out->last_fired = b->d.last_fired;
    out->last_visited = b->d.last_visited;
    out->clock = b->d.clock;
    out->reward = b->d.reward;
    out->rbar = b->d.rbar;
    return ABNN_OK;
}

// The device record layout (layout 3): the 24-bit src as its
// filter code in two streams (lo u16 in record order, hi u8 permuted within
// every 256-record group) and the {dst, w} pairs; random mode adds the u32 src
// mirror.  Each array holds capacity + padding entries.
abnn_status abnn_synapse_layout(abnn_brain* b, abnn_layout* out)
{
    REQUIRE(b && out, "null argument");
    std::memset(out, 0, sizeof(*out));
    b->ext_ptrs = true;  // as abnn_state_ptrs: the caller may write behind the handle's back
    index_invalidate(b);  // never used again (index_eligible): its memory goes now
    const uint64_t n = b->dims.syn_capacity + kDummyRecords;
    auto put = [&](void* p, uint64_t bytes, uint32_t eb, const char* name) {
        abnn_array_desc& a = out->arrays[out->n_arrays++];
        a.ptr = p;
        a.bytes = bytes;
        a.elem_bytes = eb;
        std::strncpy(a.name, name, sizeof(a.name) - 1);
    };
    out->version = ABNN_LAYOUT_VERSION;
    put(b->d.syn.lo, n * 2, 2, "src_code_lo");
    put(b->d.syn.hi, hi_bytes(n), 1, "src_code_hi");
    put(b->d.syn.dw, n * 8, 8, "dst_w");
    if (b->d.syn.src32) put(b->d.syn.src32, n * 4, 4, "src32");
    return ABNN_OK;
}

uint64_t abnn_n_neuron(const abnn_brain* b) { return b ? b->n_nrn : 0; }

abnn_status abnn_get_budget(abnn_brain* b, uint32_t* remaining)
{
    REQUIRE(b && remaining, "null argument");
    ST_TRY(sync_all(b));
    uint32_t used = 0;
    if (b->last_pass != ~0ull)  // spikes of the last pass (its spike list's length, in fired_ring)
        HIP_TRY(hipMemcpy(&used, b->d.n_fired_ring + (b->last_pass & (kFiredRing - 1)), 4, hipMemcpyDeviceToHost));
    *remaining = b->params.max_spikes - std::min(used, b->params.max_spikes);
    return ABNN_OK;
}

uint64_t abnn_structural_updates(const abnn_brain* b) { return b ? b->structural_updates : 0; }

uint64_t abnn_renormalisations(const abnn_brain* b) { return b ? b->renorms : 0; }

abnn_status abnn_upload_synapses(abnn_brain* b, uint64_t first, const abnn_synapse* src, uint64_t n)
{
    REQUIRE(b && (src || n == 0), "null argument");
    REQUIRE(first <= b->dims.n_syn && n <= b->dims.n_syn - first, "range out of bounds");
    ST_TRY(validate_records(b, src, n));
    ST_TRY(sync_all(b));
    ST_TRY(records_h2d(b->d.syn, first, n, src));
    if (first == 0 && n == b->dims.n_syn) b->records_invalid = false;  // every record rewritten
    return retally(b, first, n);
}

abnn_status abnn_download_synapses(abnn_brain* b, uint64_t first, abnn_synapse* dst, uint64_t n)
{
    REQUIRE(b && (dst || n == 0), "null argument");
    REQUIRE(first <= b->dims.n_syn && n <= b->dims.n_syn - first, "range out of bounds");
    ST_TRY(sync_all(b));
    return records_d2h(b->d.syn, first, n, dst);
}

abnn_status abnn_generate_synapses(abnn_brain* b, uint64_t seed)
{
    REQUIRE(b, "null argument");
    const uint64_t n_io = (uint64_t)b->dims.n_input * b->dims.n_output;
    REQUIRE(b->dims.syn_offset + b->dims.n_syn <= n_io || b->dims.n_hidden > 0,
            "sparse hidden synapses need n_hidden > 0 (brain-engine.cpp:46-47)");
    REQUIRE(b->dims.n_output > 0 || b->dims.syn_offset + b->dims.n_syn <= n_io,
            "dense block needs n_output > 0");
    ST_TRY(sync_all(b));
    HIP_TRY(launch_generate(b->d, b->dims.n_input, b->dims.n_output, seed, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->records_invalid = false;
    return retally(b, 0, b->dims.n_syn);
}

abnn_status abnn_checksum_synapses(abnn_brain* b, uint64_t* out)
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(launch_checksum(b->d, b->u64_scratch, b->stream));
    HIP_TRY(hipMemcpyAsync(out, b->u64_scratch, sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return ABNN_OK;
}

/* ---- graph builder (graph.hip) ------------------------------ */

uint64_t abnn_graph_records(const abnn_graph_spec* spec) { return graph_records(spec); }

namespace {
const char* const kGraphInvalid =
    "graph: n_blocks must be 1..16, reserved words and the blocks past n_blocks 0; per block count 1..2^59-1, "
    "non-empty populations below 2^32, a known topology (k and p_rewire only with RING: one population, 1 <= k < n, "
    "p_rewire in [0, 1]) and weight law (beta_a, beta_b only with BETA: >= 1, a + b - 1 <= 15), finite w_lo <= w_hi";
}

abnn_status abnn_graph_fill_host(const abnn_graph_spec* spec, uint64_t first, uint64_t n, abnn_synapse* out_host)
{
    REQUIRE(spec && (out_host || n == 0), "null argument");
    const uint64_t total = graph_records(spec);
    REQUIRE(total != 0, kGraphInvalid);
    REQUIRE(first <= total && n <= total - first, "abnn_graph_fill_host: the range ends past abnn_graph_records(spec)");
    graph_fill(graph_table(*spec), first, n, out_host);
    return ABNN_OK;
}

abnn_status abnn_build_graph(abnn_brain* b, const abnn_graph_spec* spec)
{
    REQUIRE(b && spec, "null argument");
    const uint64_t total = graph_records(spec);
    REQUIRE(total != 0, kGraphInvalid);
    REQUIRE(b->dims.syn_offset <= total && b->dims.n_syn <= total - b->dims.syn_offset,
            "abnn_build_graph: syn_offset + n_syn exceeds abnn_graph_records(spec)");
    for (uint32_t j = 0; j < spec->n_blocks; ++j) {
        const abnn_graph_block& k = spec->blocks[j];
        REQUIRE((uint64_t)k.src_first + k.src_count <= b->n_nrn && (uint64_t)k.dst_first + k.dst_count <= b->n_nrn,
                "abnn_build_graph: a population ends above N_NRN");
    }
    ST_TRY(sync_all(b));
    HIP_TRY(launch_build_graph(b->d.syn, b->dims.n_syn, b->dims.syn_offset, graph_table(*spec), b->graph_blocks,
                               b->graph_nt, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->records_invalid = false;
    return retally(b, 0, b->dims.n_syn);
}

/* ---- synapse census (census.hip) --------------------------- */

uint64_t abnn_census_words(const abnn_census_config* cfg)
{
    return census_config_ok(cfg, nullptr) ? ABNN_CENSUS_HEADER_WORDS + (uint64_t)cfg->bins : 0;
}

namespace {

// The checks of a census on handle b that need no device; *scale for the launch.
abnn_status census_check(const abnn_brain* b, const abnn_census_config* cfg, float* scale)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(census_config_ok(cfg, scale),
            "census: bins must be 1..4096, lo < hi both finite with a finite bins / (hi - lo), reserved 0");
    REQUIRE(range_ok(cfg->src_first, cfg->src_count, b->n_nrn), "census: src range ends above N_NRN");
    REQUIRE(range_ok(cfg->dst_first, cfg->dst_count, b->n_nrn), "census: dst range ends above N_NRN");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_census_enqueue(abnn_brain* b, const abnn_census_config* cfg, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    float scale = 0.0f;
    ST_TRY(census_check(b, cfg, &scale));
    HIP_TRY(hipSetDevice(b->device));
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_census(b->d.syn, b->dims.n_syn, *cfg, scale, out_dev, (uint32_t)b->cus, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_census(abnn_brain* b, const abnn_census_config* cfg, uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    float scale = 0.0f;
    ST_TRY(census_check(b, cfg, &scale));
    REQUIRE(words == abnn_census_words(cfg), "abnn_census: words must equal abnn_census_words(cfg)");
    ST_TRY(sync_all(b));
    if (!b->census_out) ST_TRY(b->pool.alloc(zeroed(&b->census_out, ABNN_CENSUS_HEADER_WORDS + ABNN_CENSUS_MAX_BINS)));
    HIP_TRY(launch_census(b->d.syn, b->dims.n_syn, *cfg, scale, b->census_out, (uint32_t)b->cus, b->stream));
    return read_words(b, b->census_out, out_host, words);
}

/* ---- neuron degree census (degree.hip) ---------------------- */

uint64_t abnn_degree_words(const abnn_degree_config* cfg, uint64_t n_nrn) { return degree_words(cfg, n_nrn); }

namespace {

abnn_status degree_check(const abnn_brain* b, const abnn_degree_config* cfg)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(degree_config_ok(cfg, b->n_nrn, nullptr),
            "degree: what must be a non-empty subset of the four planes, reserved 0, count 0 only with first 0, "
            "first + count <= N_NRN");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_degree_enqueue(abnn_brain* b, const abnn_degree_config* cfg, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(degree_check(b, cfg));
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(launch_degree(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, out_dev, (uint32_t)b->cus, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_degree(abnn_brain* b, const abnn_degree_config* cfg, uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(degree_check(b, cfg));
    REQUIRE(words == degree_words(cfg, b->n_nrn), "abnn_degree: words must equal abnn_degree_words(cfg, N_NRN)");
    ST_TRY(sync_all(b));
    ST_TRY(b->pool.grow(&b->degree_out, &b->degree_cap, words));
    HIP_TRY(launch_degree(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, b->degree_out, (uint32_t)b->cus, b->stream));
    return read_words(b, b->degree_out, out_host, words);
}

/* ---- synapse select (select.hip) ---------------------------- */

uint64_t abnn_select_words(const abnn_select_config* cfg, uint64_t capacity) { return select_words(cfg, capacity); }

namespace {

// The checks of a select on handle b, then its scratch (the first call
// allocates it: that one may synchronise the device).
abnn_status select_check(abnn_brain* b, const abnn_select_config* cfg, uint64_t capacity)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(select_words(cfg, capacity) != 0,
            "select: unknown flags, reserved != 0, w_lo / w_hi without WEIGHT, a NaN bound or w_lo >= w_hi, "
            "ANY with no range set, or a range that wraps u32");
    REQUIRE(range_ok(cfg->src_first, cfg->src_count, b->n_nrn), "select: src range ends above N_NRN");
    REQUIRE(range_ok(cfg->dst_first, cfg->dst_count, b->n_nrn), "select: dst range ends above N_NRN");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    if (b->select.counts) return ABNN_OK;
    // no memset: a select zeroes the counts it reads and writes the offsets it reads
    return b->pool.alloc_all(
        {raw(&b->select.counts, std::max<uint64_t>(4, select_count_words(b->dims.syn_capacity))),
         raw(&b->select.offsets, select_tiles(b->dims.syn_capacity))});
}

}  // namespace

abnn_status abnn_select_enqueue(abnn_brain* b, const abnn_select_config* cfg, uint64_t capacity, uint64_t* out_dev,
                                void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(select_check(b, cfg, capacity));
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_select(b->d.syn, b->dims.n_syn, b->dims.syn_offset, *cfg, capacity, b->select, out_dev,
                          b->select_blocks, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_select(abnn_brain* b, const abnn_select_config* cfg, uint64_t capacity, uint64_t* out_host,
                        uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(select_check(b, cfg, capacity));
    REQUIRE(words == select_words(cfg, capacity), "abnn_select: words must equal abnn_select_words(cfg, capacity)");
    ST_TRY(sync_all(b));
    // the device result lives for this call only: a capacity of every record is 24 B per record
    DeviceTemp<uint64_t> res;
    ST_TRY(res.alloc(words, false));  // no memset: launch_select zeroes the header, the rest is read up to `written`
    uint64_t* dev = res.dev;
    HIP_TRY(launch_select(b->d.syn, b->dims.n_syn, b->dims.syn_offset, *cfg, capacity, b->select, dev, b->select_blocks,
                          b->stream));
    const uint64_t h = ABNN_SELECT_HEADER_WORDS;
    ST_TRY(read_words(b, dev, out_host, h));
    const uint64_t written = out_host[3];
    if (written) {  // the header, then only the entries that were written
        HIP_TRY(hipMemcpyAsync(out_host + h, dev + h, written * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipMemcpyAsync(out_host + h + capacity, dev + h + capacity, written * sizeof(abnn_synapse),
                               hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    return ABNN_OK;
}

/* ---- synapse edit (edit.hip) -------------------------------- */

uint64_t abnn_edit_words(const abnn_edit_config* cfg) { return edit_words(cfg); }

namespace {

constexpr const char* kEditInvalid =
    "edit: an unknown op or flag, reserved != 0, a parameter set that the op and flags do not read, a NaN in one that "
    "is read, c_lo > c_hi, DRAW with a > b or a bound that is not finite, CLAMP with KILL, ANY with a SCALE op, or "
    "what abnn_select_words refuses for the ranges and the weight bounds";

// The checks of an edit over a brain of n_nrn neurons that need no device.
abnn_status edit_check(const abnn_edit_config* cfg, uint64_t n_nrn, bool has_plane)
{
    REQUIRE(edit_words(cfg) != 0, kEditInvalid);
    REQUIRE(range_ok(cfg->src_first, cfg->src_count, n_nrn), "edit: src range ends above N_NRN");
    REQUIRE(range_ok(cfg->dst_first, cfg->dst_count, n_nrn), "edit: dst range ends above N_NRN");
    REQUIRE(n_nrn <= kMaxNeurons, "edit: N_NRN above the library's limit");
    REQUIRE(edit_is_scale(cfg->op) == has_plane, "edit: a SCALE op needs a plane, every other op none");
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_edit_enqueue(abnn_brain* b, const abnn_edit_config* cfg, const float* plane_dev, uint64_t* out_dev,
                              void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(edit_check(cfg, b->n_nrn, plane_dev != nullptr));
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    if (cfg->op == ABNN_EDIT_KILL) index_invalidate(b);  // tombstones: their src leaves the index
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_edit(b->d.syn, b->dims.n_syn, edit_rule(*cfg, b->n_nrn, b->dims.syn_offset), plane_dev, b->d.dead,
                        out_dev, b->edit_blocks, b->edit_nt, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_edit(abnn_brain* b, const abnn_edit_config* cfg, const float* plane_host, uint64_t plane_count,
                      uint64_t out_host[ABNN_EDIT_HEADER_WORDS])
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(edit_check(cfg, b->n_nrn, plane_host != nullptr));
    REQUIRE(plane_count == edit_plane_count(*cfg, b->n_nrn),
            "abnn_edit: plane_count must equal the neurons of the SCALE op's range (N_NRN when it is not set), 0 otherwise");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    ST_TRY(sync_all(b));
    if (cfg->op == ABNN_EDIT_KILL) index_invalidate(b);  // tombstones: their src leaves the index
    if (!b->edit_out) ST_TRY(b->pool.alloc(zeroed(&b->edit_out, ABNN_EDIT_HEADER_WORDS)));
    ST_TRY(b->pool.grow(&b->edit_plane, &b->edit_plane_cap, plane_count));
    if (plane_count)
        HIP_TRY(hipMemcpyAsync(b->edit_plane, plane_host, plane_count * sizeof(float), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(launch_edit(b->d.syn, b->dims.n_syn, edit_rule(*cfg, b->n_nrn, b->dims.syn_offset),
                        plane_count ? b->edit_plane : nullptr, b->d.dead, b->edit_out, b->edit_blocks, b->edit_nt,
                        b->stream));
    return read_words(b, b->edit_out, out_host, ABNN_EDIT_HEADER_WORDS);
}

abnn_status abnn_edit_host(const abnn_edit_config* cfg, uint64_t n_nrn, uint64_t syn_offset, abnn_synapse* records,
                           uint64_t n, const float* plane, uint64_t out[ABNN_EDIT_HEADER_WORDS])
{
    REQUIRE(cfg && out && (records || n == 0), "null argument");
    ST_TRY(edit_check(cfg, n_nrn, plane != nullptr));
    edit_host(*cfg, n_nrn, syn_offset, records, n, plane, out);
    return ABNN_OK;
}

abnn_status abnn_edit_factors_enqueue(abnn_brain* b, const uint64_t* strength_dev, uint64_t count, float target,
                                      float f_lo, float f_hi, float* plane_dev, void* stream)
{
    REQUIRE(b && ((strength_dev && plane_dev) || count == 0), "null argument");
    REQUIRE(edit_factors_ok(target, f_lo, f_hi), "edit factors: target > 0 finite and 0 < f_lo <= f_hi finite");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(launch_edit_factors(strength_dev, count, target, f_lo, f_hi, plane_dev, b->edit_blocks, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_edit_factors_host(const uint64_t* strength, uint64_t count, float target, float f_lo, float f_hi,
                                   float* plane)
{
    REQUIRE((strength && plane) || count == 0, "null argument");
    REQUIRE(edit_factors_ok(target, f_lo, f_hi), "edit factors: target > 0 finite and 0 < f_lo <= f_hi finite");
    edit_factors_host(strength, count, target, f_lo, f_hi, plane);
    return ABNN_OK;
}

/* ---- record reorder (reorder.hip) ---------------------------- */

uint64_t abnn_reorder_words(const abnn_reorder_config* cfg, uint64_t n_syn) { return reorder_words(cfg, n_syn); }

namespace {

constexpr const char* kReorderInvalid =
    "reorder: an unknown key or flag, DESCENDING with NONE, RANDOM or PERM, a reserved word or an unread seed that is "
    "not 0, or more than 2^32 records";

// The checks of a reorder on handle b, then its scratch (the first call
// allocates it: that one may synchronise the device).
abnn_status reorder_check(abnn_brain* b, const abnn_reorder_config* cfg, bool has_perm)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(reorder_words(cfg, b->dims.n_syn) != 0, kReorderInvalid);
    REQUIRE((cfg->key == ABNN_REORDER_PERM) == has_perm, "reorder: PERM needs a perm, every other key none");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    REQUIRE(!b->pending_walk, "reorder: a sharded pass is half done (abnn_shard_apply)");
    HIP_TRY(hipSetDevice(b->device));
    ReorderScratch& r = b->reorder;
    if (r.capacity < b->dims.syn_capacity || !r.state) {
        ST_TRY(sync_all(b));
        reorder_free(b);
        // no memset: a reorder writes every word it reads; whole 16-B pairs
        const uint64_t cap = std::max<uint64_t>(b->dims.syn_capacity, 1) + 2;
        ST_TRY(b->pool.alloc_all({raw(&r.pairs[0], cap), raw(&r.pairs[1], cap), raw(&r.rec, cap * 3),
                                  raw(&r.counts, (uint64_t)kReorderDigits * kReorderMaxSegments),
                                  raw(&r.seg_tomb, kReorderMaxSegments + 1), raw(&r.state, kReorderStateWords)}));
        r.capacity = b->dims.syn_capacity;
    }
    return ABNN_OK;
}

// The reorder and its bookkeeping on stream s (what a records-only snapshot
// restore redoes when n_syn is unchanged): the random-mode src mirror, the
// pruning tally zeroed and recounted over [0, n).
abnn_status reorder_launch(abnn_brain* b, const abnn_reorder_config* cfg, const uint32_t* perm_dev, uint64_t* out_dev,
                           hipStream_t s)
{
    const uint64_t n = b->dims.n_syn;  // the host knows n_syn: structural updates synchronise
    index_invalidate(b);  // records move
    HIP_TRY(launch_reorder(b->d.syn, n, b->dims.syn_offset, *cfg, perm_dev, b->reorder, out_dev, b->reorder_blocks,
                           b->reorder_skip, s));
    HIP_TRY(launch_src32_sync(b->d.syn, n, s));
    if (b->d.dead) {
        const uint64_t nb = (b->dims.syn_capacity + kCompactChunk - 1) / kCompactChunk;
        HIP_TRY(hipMemsetAsync(b->d.dead, 0, nb * sizeof(uint32_t), s));
        HIP_TRY(launch_tally_dead(b->d.syn, n, b->d.dead, 0, n, s));
    }
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_reorder_enqueue(abnn_brain* b, const abnn_reorder_config* cfg, const uint32_t* perm_dev,
                                 uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(reorder_check(b, cfg, perm_dev != nullptr));
    return reorder_launch(b, cfg, perm_dev, out_dev, pick(b, stream));
}

abnn_status abnn_reorder(abnn_brain* b, const abnn_reorder_config* cfg, const uint32_t* perm_host, uint64_t* out_host,
                         uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(reorder_check(b, cfg, perm_host != nullptr));
    REQUIRE(words == reorder_words(cfg, b->dims.n_syn), "abnn_reorder: words must equal abnn_reorder_words(cfg, n_syn)");
    ST_TRY(sync_all(b));
    // the device result and the staged perm live for this call only
    DeviceTemp<uint64_t> res;
    DeviceTemp<uint32_t> perm;
    ST_TRY(res.alloc(words, false));  // no memset: launch_reorder fills the result
    const uint64_t n = b->dims.n_syn;
    if (perm_host) ST_TRY(perm.alloc(n, false));
    const abnn_status st = [&]() -> abnn_status {  // the perm in, the reorder, the result out
        if (perm_host && n) HIP_TRY(hipMemcpyAsync(perm.dev, perm_host, n * 4, hipMemcpyHostToDevice, b->stream));
        ST_TRY(reorder_launch(b, cfg, perm.dev, res.dev, b->stream));
        HIP_TRY(hipMemcpyAsync(out_host, res.dev, words * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream));
        return ABNN_OK;
    }();
    const hipError_t e = hipStreamSynchronize(b->stream);  // before the two are freed, also after a failure
    ST_TRY(st);
    HIP_TRY(e);
    return ABNN_OK;
}

abnn_status abnn_reorder_release(abnn_brain* b)
{
    REQUIRE(b, "null argument");
    ST_TRY(sync_all(b));
    reorder_free(b);
    return ABNN_OK;
}

abnn_status abnn_reorder_host(const abnn_reorder_config* cfg, uint64_t syn_offset, abnn_synapse* records, uint64_t n,
                              const uint32_t* perm, uint64_t* out)
{
    REQUIRE(cfg && out && (records || n == 0), "null argument");
    REQUIRE(reorder_words(cfg, n) != 0, kReorderInvalid);
    REQUIRE((cfg->key == ABNN_REORDER_PERM) == (perm != nullptr), "reorder: PERM needs a perm, every other key none");
    reorder_host(*cfg, syn_offset, records, n, perm, out);
    return ABNN_OK;
}

/* ---- device-side snapshots (snapshot.hip) -------------------- */

// A copy of a handle's state in device memory, sized for its syn_capacity and
// N_NRN, and the host mirrors as they were when the last capture was enqueued.
struct abnn_snapshot {
    abnn_brain* b = nullptr;
    DevicePool pool;                 // owns the buffers below
    SynArrays syn{};                 // lo, hi, dw of [0, n_syn); no src32 (restore rebuilds the mirror)
    uint64_t* last_fired = nullptr;  // [n_nrn]
    uint64_t* last_visited = nullptr;
    uint64_t* scalars = nullptr;     // the scalar block: {clock, reward | rbar, pass_index}
    uint4* grown = nullptr;          // genesis on: [grown_slots]
    uint64_t grown_slots = 0;
    uint64_t captures = 0, n_syn = 0, bytes = 0;
    uint64_t clock_host = 0, pass_host = 0, rng = 0, max_host_stamp = 0;
};

namespace {

abnn_status snapshot_alloc(abnn_snapshot* s)
{
    const abnn_brain* b = s->b;
    const uint64_t cap = b->dims.syn_capacity + 2;  // whole 16-B pairs
    std::vector<Slot> bufs = {zeroed(&s->syn.lo, cap),           zeroed(&s->syn.hi, cap),
                              zeroed(&s->syn.dw, cap),           zeroed(&s->last_fired, b->n_nrn),
                              zeroed(&s->last_visited, b->n_nrn), zeroed(&s->scalars, 3)};
    if (b->d.grown) {
        s->grown_slots = (uint64_t)b->params.compact_every * b->params.max_spikes;
        bufs.push_back(zeroed(&s->grown, s->grown_slots));
    }
    ST_TRY(s->pool.alloc_all(bufs));
    HIP_TRY(hipDeviceSynchronize());  // the buffers' zeros
    s->bytes = cap * 11 + b->n_nrn * 16 + 24 + s->grown_slots * 16;
    return ABNN_OK;
}

constexpr const char* kDiffInvalid =
    "snapshot diff: bins must be 1..4096, lo < hi both finite with a finite bins / (hi - lo), reserved 0";

// The checks of a diff over a brain of n_nrn neurons that need no device; *scale for the launch.
abnn_status diff_check(const abnn_diff_config* cfg, uint64_t n_nrn, float* scale)
{
    REQUIRE(diff_config_ok(cfg, scale), kDiffInvalid);
    REQUIRE(range_ok(cfg->src_first, cfg->src_count, n_nrn), "snapshot diff: src range ends above N_NRN");
    REQUIRE(range_ok(cfg->dst_first, cfg->dst_count, n_nrn), "snapshot diff: dst range ends above N_NRN");
    return ABNN_OK;
}

// ... and of its two sides on handle b.
abnn_status diff_sides_check(const abnn_brain* b, const abnn_snapshot* then, const abnn_snapshot* now)
{
    REQUIRE(then->b == b && (!now || now->b == b), "snapshot diff: a snapshot of another brain");
    REQUIRE(then->captures > 0 && (!now || now->captures > 0), "snapshot diff: nothing was captured yet");
    REQUIRE(now || !b->records_invalid, kRecordsInvalid);
    return ABNN_OK;
}

hipError_t diff_launch(abnn_brain* b, const abnn_snapshot* then, const abnn_snapshot* now, const abnn_diff_config& cfg,
                       float scale, uint64_t* out_dev, hipStream_t s)
{
    // the host knows the handle's n_syn: structural updates synchronise
    return launch_diff(then->syn, then->n_syn, now ? now->syn : b->d.syn, now ? now->n_syn : b->dims.n_syn,
                       diff_rule(cfg, scale), out_dev, (uint32_t)b->cus, s);
}

}  // namespace

abnn_status abnn_snapshot_create(abnn_brain* b, abnn_snapshot** out)
{
    REQUIRE(b && out, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(b->device));
    abnn_snapshot* s = new (std::nothrow) abnn_snapshot();
    if (!s) return ABNN_ERR_OOM;
    s->b = b;
    const abnn_status st = snapshot_alloc(s);
    if (st != ABNN_OK) {
        delete s;  // nothing half made: its pool frees the buffers
        return st;
    }
    *out = s;
    return ABNN_OK;
}

abnn_status abnn_snapshot_destroy(abnn_snapshot* s)
{
    if (!s) return ABNN_OK;
    (void)hipSetDevice(s->b->device);
    (void)hipDeviceSynchronize();  // an enqueued capture or diff may still use the buffers
    delete s;  // its pool frees the buffers
    return ABNN_OK;
}

abnn_status abnn_snapshot_get_info(const abnn_snapshot* s, abnn_snapshot_info* out)
{
    REQUIRE(s && out, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->captures = s->captures;
    out->n_syn = s->n_syn;
    out->scalars.clock = s->clock_host;
    out->scalars.pass_index = s->pass_host;
    out->bytes = s->bytes;
    return ABNN_OK;
}

abnn_status abnn_snapshot_capture_enqueue(abnn_brain* b, abnn_snapshot* s, void* stream)
{
    REQUIRE(b && s, "null argument");
    REQUIRE(s->b == b, "abnn_snapshot_capture_enqueue: a snapshot of another brain");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t q = pick(b, stream);
    const DeviceState& d = b->d;
    // the host knows n_syn: structural updates synchronise
    const uint64_t n = b->dims.n_syn;
    if (n) {
        HIP_TRY(hipMemcpyAsync(s->syn.lo, d.syn.lo, n * 2, hipMemcpyDeviceToDevice, q));
        HIP_TRY(hipMemcpyAsync(s->syn.hi, d.syn.hi, n, hipMemcpyDeviceToDevice, q));
        HIP_TRY(hipMemcpyAsync(s->syn.dw, d.syn.dw, n * 8, hipMemcpyDeviceToDevice, q));
    }
    HIP_TRY(hipMemcpyAsync(s->last_fired, d.last_fired, b->n_nrn * 8, hipMemcpyDeviceToDevice, q));
    HIP_TRY(hipMemcpyAsync(s->last_visited, d.last_visited, b->n_nrn * 8, hipMemcpyDeviceToDevice, q));
    HIP_TRY(hipMemcpyAsync(s->scalars, b->scalar_block, 24, hipMemcpyDeviceToDevice, q));
    if (s->grown) HIP_TRY(hipMemcpyAsync(s->grown, d.grown, s->grown_slots * 16, hipMemcpyDeviceToDevice, q));
    // the mirrors as they are now: the passes enqueued so far have advanced them
    s->n_syn = n;
    s->clock_host = b->clock_host;
    s->pass_host = b->pass_host;
    s->rng = b->rng;
    s->max_host_stamp = b->max_host_stamp;
    s->captures += 1;
    return ABNN_OK;
}

abnn_status abnn_snapshot_restore(abnn_brain* b, const abnn_snapshot* s, uint32_t what)
{
    REQUIRE(b && s, "null argument");
    REQUIRE(s->b == b, "abnn_snapshot_restore: a snapshot of another brain");
    REQUIRE(what != 0 && !(what & ~(ABNN_SNAP_RECORDS | ABNN_SNAP_STATE)),
            "abnn_snapshot_restore: what must be ABNN_SNAP_RECORDS, ABNN_SNAP_STATE or both");
    REQUIRE(s->captures > 0, "abnn_snapshot_restore: nothing was captured yet");
    REQUIRE(!b->pending_walk, "abnn_snapshot_restore: a sharded pass is half done (abnn_shard_apply)");
    ST_TRY(sync_all(b));
    DeviceState& d = b->d;
    if (what & ABNN_SNAP_RECORDS) {
        // [0, n) come back; what lies at and past n stays (as after a shrinking
        // structural update: a pass masks the events past its last one)
        const uint64_t n = s->n_syn;
        index_invalidate(b);  // the records come back as they were captured
        if (n) {
            HIP_TRY(hipMemcpyAsync(d.syn.lo, s->syn.lo, n * 2, hipMemcpyDeviceToDevice, b->stream));
            HIP_TRY(hipMemcpyAsync(d.syn.hi, s->syn.hi, n, hipMemcpyDeviceToDevice, b->stream));
            HIP_TRY(hipMemcpyAsync(d.syn.dw, s->syn.dw, n * 8, hipMemcpyDeviceToDevice, b->stream));
            HIP_TRY(launch_src32_sync(d.syn, n, b->stream));
        }
        HIP_TRY(hipDeviceSynchronize());
        if (n != b->dims.n_syn) {
            b->dims.n_syn = n;
            ST_TRY(repartition(b));
        }
        if (d.dead) {  // no tally is left past the records: appended records land there
            const uint64_t nb = (b->dims.syn_capacity + kCompactChunk - 1) / kCompactChunk;
            HIP_TRY(hipMemset(d.dead, 0, nb * sizeof(uint32_t)));
            ST_TRY(retally(b, 0, n));
        }
        b->records_invalid = false;  // a restore is a reload
    }
    if (what & ABNN_SNAP_STATE) {
        HIP_TRY(hipMemcpyAsync(d.last_fired, s->last_fired, b->n_nrn * 8, hipMemcpyDeviceToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(d.last_visited, s->last_visited, b->n_nrn * 8, hipMemcpyDeviceToDevice, b->stream));
        HIP_TRY(hipMemcpyAsync(b->scalar_block, s->scalars, 24, hipMemcpyDeviceToDevice, b->stream));
        if (s->grown) HIP_TRY(hipMemcpyAsync(d.grown, s->grown, s->grown_slots * 16, hipMemcpyDeviceToDevice, b->stream));
        if (d.visit_mark) HIP_TRY(hipMemsetAsync(d.visit_mark, 0, b->n_nrn, b->stream));
        HIP_TRY(hipDeviceSynchronize());
        b->marks_dirty = false;
        b->clock_host = s->clock_host;
        b->pass_host = s->pass_host;
        b->rng = s->rng;
        // the bitmap is rebuilt from lastFired; every restored stamp is at most
        // the larger of the captured clock and what the host had written by
        // then, so the steady-state build resumes once the clock has passed it
        // (the handle's own value may lie ahead of a clock that moved back)
        state_written(b, 0);
        b->max_host_stamp = std::max(s->max_host_stamp, s->clock_host);
        b->last_pass = ~0ull;  // no pass since: abnn_get_budget answers max_spikes
    }
    return ABNN_OK;
}

uint64_t abnn_snapshot_diff_words(const abnn_diff_config* cfg) { return diff_words(cfg); }

abnn_status abnn_snapshot_diff_enqueue(abnn_brain* b, const abnn_snapshot* then, const abnn_snapshot* now,
                                       const abnn_diff_config* cfg, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && then && cfg && out_dev, "null argument");
    float scale = 0.0f;
    ST_TRY(diff_check(cfg, b->n_nrn, &scale));
    ST_TRY(diff_sides_check(b, then, now));
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(diff_launch(b, then, now, *cfg, scale, out_dev, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_snapshot_diff(abnn_brain* b, const abnn_snapshot* then, const abnn_snapshot* now,
                               const abnn_diff_config* cfg, uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && then && cfg && out_host, "null argument");
    float scale = 0.0f;
    ST_TRY(diff_check(cfg, b->n_nrn, &scale));
    ST_TRY(diff_sides_check(b, then, now));
    REQUIRE(words == diff_words(cfg), "abnn_snapshot_diff: words must equal abnn_snapshot_diff_words(cfg)");
    ST_TRY(sync_all(b));
    if (!b->diff_out) ST_TRY(b->pool.alloc(zeroed(&b->diff_out, ABNN_DIFF_HEADER_WORDS + ABNN_DIFF_MAX_BINS)));
    HIP_TRY(diff_launch(b, then, now, *cfg, scale, b->diff_out, b->stream));
    return read_words(b, b->diff_out, out_host, words);
}

abnn_status abnn_snapshot_diff_host(const abnn_diff_config* cfg, uint64_t n_nrn, const abnn_synapse* then,
                                    uint64_t n_then, const abnn_synapse* now, uint64_t n_now, uint64_t* out)
{
    REQUIRE(cfg && out && (then || n_then == 0) && (now || n_now == 0), "null argument");
    float scale = 0.0f;
    ST_TRY(diff_check(cfg, n_nrn, &scale));
    diff_host(*cfg, scale, then, n_then, now, n_now, out);
    return ABNN_OK;
}

/* ---- reachability (hops.hip) --------------------------------- */

uint64_t abnn_hops_words(const abnn_hops_config* cfg, uint64_t n_nrn) { return hops_words(cfg, n_nrn); }

namespace {

// The checks of a search on handle b, then its scratch (the first call
// allocates it: that one may synchronise the device).
abnn_status hops_check(abnn_brain* b, const abnn_hops_config* cfg)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(hops_config_ok(cfg, b->n_nrn),
            "hops: seed_count >= 1 and the seed range inside N_NRN, max_hops in 1..1024, no unknown flags, reserved 0, "
            "w_lo / w_hi +0 without WEIGHT, with it no NaN bound and w_lo < w_hi");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    // no memset: every step writes every word of the bitmap before it reads it
    if (!b->hops_bitmap) ST_TRY(b->pool.alloc(raw(&b->hops_bitmap, hops_bitmap_words(b->n_nrn))));
    return ABNN_OK;
}

abnn_status hops_steps(abnn_brain* b, const abnn_hops_config* cfg, uint64_t* out_dev, hipStream_t s)
{
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_hops_step(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, ABNN_HOPS_BEGIN, out_dev, b->hops_bitmap,
                             (uint32_t)b->cus, s));
    for (uint32_t h = 0; h <= cfg->max_hops; ++h)
        HIP_TRY(launch_hops_step(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, h, out_dev, b->hops_bitmap, (uint32_t)b->cus, s));
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_hops_enqueue(abnn_brain* b, const abnn_hops_config* cfg, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 7u) == 0, "hops: out_dev must be 8-byte aligned");
    ST_TRY(hops_check(b, cfg));
    return hops_steps(b, cfg, out_dev, pick(b, stream));
}

abnn_status abnn_hops_step_enqueue(abnn_brain* b, const abnn_hops_config* cfg, uint32_t step, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 7u) == 0, "hops: out_dev must be 8-byte aligned");
    ST_TRY(hops_check(b, cfg));
    REQUIRE(step == ABNN_HOPS_BEGIN || step <= cfg->max_hops, "hops: a step is ABNN_HOPS_BEGIN or 0 .. max_hops");
    HIP_TRY(launch_hops_step(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, step, out_dev, b->hops_bitmap, (uint32_t)b->cus,
                             pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_hops(abnn_brain* b, const abnn_hops_config* cfg, uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(hops_check(b, cfg));
    REQUIRE(words == hops_words(cfg, b->n_nrn), "abnn_hops: words must equal abnn_hops_words(cfg, N_NRN)");
    ST_TRY(sync_all(b));
    ST_TRY(b->pool.grow(&b->hops_out, &b->hops_cap, words));
    ST_TRY(hops_steps(b, cfg, b->hops_out, b->stream));
    return read_words(b, b->hops_out, out_host, words);
}

/* ---- connected components (components.hip) --------------------- */

uint64_t abnn_components_words(const abnn_components_config* cfg, uint64_t n_nrn) { return components_words(cfg, n_nrn); }

namespace {

constexpr const char* kCompConfig =
    "components: count >= 1 and the range inside N_NRN, no unknown flags, reserved 0, "
    "w_lo / w_hi +0 without WEIGHT, with it no NaN bound and w_lo < w_hi";

// The checks of a search on handle b, then its scratch (the first call
// allocates it, all or nothing: that one may synchronise the device).
abnn_status components_check(abnn_brain* b, const abnn_components_config* cfg, const uint64_t* out_dev)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 7u) == 0, "components: out_dev must be 8-byte aligned");
    REQUIRE(components_config_ok(cfg, b->n_nrn), kCompConfig);
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    // no memset: CLOSE zeroes the counters, LINK writes every word of the map and the sample's words before it reads them
    if (!b->comp.counts)
        ST_TRY(b->pool.alloc_all({raw(&b->comp.counts, 2 * components_plane_words(b->n_nrn)),
                                  raw(&b->comp.settled, comp_settled_words(b->n_nrn)), raw(&b->comp.major, 2)}));
    return ABNN_OK;
}

abnn_status components_step(abnn_brain* b, const abnn_components_config* cfg, uint32_t step, uint64_t* out_dev, hipStream_t s)
{
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_components_step(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, step, out_dev, b->comp, b->comp_path,
                                   (uint32_t)b->cus, s));
    return ABNN_OK;
}

abnn_status components_steps(abnn_brain* b, const abnn_components_config* cfg, uint64_t* out_dev, hipStream_t s)
{
    for (uint32_t step : {ABNN_COMP_BEGIN, ABNN_COMP_LINK, ABNN_COMP_FLATTEN, ABNN_COMP_CLOSE})
        ST_TRY(components_step(b, cfg, step, out_dev, s));
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_components_enqueue(abnn_brain* b, const abnn_components_config* cfg, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(components_check(b, cfg, out_dev));
    return components_steps(b, cfg, out_dev, pick(b, stream));
}

abnn_status abnn_components_step_enqueue(abnn_brain* b, const abnn_components_config* cfg, uint32_t step, uint64_t* out_dev,
                                         void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(components_check(b, cfg, out_dev));
    REQUIRE(step <= ABNN_COMP_CLOSE, "components: a step is ABNN_COMP_BEGIN, LINK, FLATTEN or CLOSE");
    return components_step(b, cfg, step, out_dev, pick(b, stream));
}

abnn_status abnn_components_merge_enqueue(abnn_brain* b, const abnn_components_config* cfg, const uint32_t* planes_dev,
                                          uint32_t n_planes, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev && planes_dev, "null argument");
    REQUIRE(n_planes >= 1, "components: a merge takes at least one plane");
    REQUIRE((reinterpret_cast<uintptr_t>(planes_dev) & 3u) == 0, "components: planes_dev must be 4-byte aligned");
    ST_TRY(components_check(b, cfg, out_dev));
    HIP_TRY(launch_components_merge(*cfg, b->n_nrn, planes_dev, n_planes, out_dev, (uint32_t)b->cus, pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_components(abnn_brain* b, const abnn_components_config* cfg, uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(components_check(b, cfg, nullptr));
    REQUIRE(words == components_words(cfg, b->n_nrn), "abnn_components: words must equal abnn_components_words(cfg, N_NRN)");
    ST_TRY(sync_all(b));
    ST_TRY(b->pool.grow(&b->comp_out, &b->comp_cap, words, false));
    ST_TRY(components_steps(b, cfg, b->comp_out, b->stream));
    ST_TRY(read_words(b, b->comp_out, out_host, words));
    if (out_host[7] != 0) {
        set_err("abnn_components: a bounded loop gave up, code " + std::to_string(out_host[7]) +
                " (1 the walk to a root, 2 the hook): the result is invalid");
        return ABNN_ERR_HIP;
    }
    return ABNN_OK;
}

abnn_status abnn_components_host(const abnn_synapse* records, uint64_t n, const abnn_components_config* cfg, uint64_t n_nrn,
                                 uint64_t* out, uint64_t words)
{
    REQUIRE(cfg && out && (records || n == 0), "null argument");
    REQUIRE(components_config_ok(cfg, n_nrn), kCompConfig);
    REQUIRE(words == components_words(cfg, n_nrn), "abnn_components_host: words must equal abnn_components_words(cfg, n_nrn)");
    components_host(*cfg, n_nrn, records, n, out);
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): pin the LINK step of the handle's component searches.
abnn_status abnn_debug_set_components_path(abnn_brain* b, int path)
{
    REQUIRE(b, "null argument");
    REQUIRE(path >= 0 && path <= 2, "abnn_debug_set_components_path: 0 auto, 1 never the settled map, 2 always");
    b->comp_path = (uint32_t)path;
    return ABNN_OK;
}

/* ---- population connectivity matrix (matrix.hip) ---------------- */

uint64_t abnn_matrix_words(const abnn_matrix_config* cfg) { return matrix_words(cfg); }

namespace {

constexpr const char* kMatConfig =
    "matrix: pops in 1..64, what a non-empty subset of COUNT | W | P, no unknown flags, reserved 0, "
    "w_lo / w_hi +0 without WEIGHT, with it no NaN bound and w_lo < w_hi";
constexpr const char* kMatPartition =
    "matrix: exactly one of bounds / labels is set, the one the LABELS flag names";
constexpr const char* kMatBounds = "matrix: bounds[0] <= bounds[1] <= ... <= bounds[P] <= N_NRN";

// the checks that need no handle
abnn_status matrix_args_check(const abnn_matrix_config* cfg, const uint32_t* bounds, const uint32_t* labels, uint64_t n_nrn)
{
    REQUIRE(cfg, "null argument");
    REQUIRE(matrix_config_ok(cfg), kMatConfig);
    const bool lab = cfg->flags & ABNN_MAT_LABELS;
    REQUIRE(lab ? (labels && !bounds) : (bounds && !labels), kMatPartition);
    REQUIRE(lab || matrix_bounds_ok(bounds, cfg->pops, n_nrn), kMatBounds);
    return ABNN_OK;
}

// The checks of a matrix on handle b, then its scratch (the first LABELS call
// allocates it: that one may synchronise the device).
abnn_status matrix_check(abnn_brain* b, const abnn_matrix_config* cfg, const uint32_t* bounds, const uint32_t* labels_dev,
                         const uint64_t* out_dev)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 7u) == 0, "matrix: out_dev must be 8-byte aligned");
    REQUIRE((reinterpret_cast<uintptr_t>(labels_dev) & 3u) == 0, "matrix: labels_dev must be 4-byte aligned");
    ST_TRY(matrix_args_check(cfg, bounds, labels_dev, b->n_nrn));
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    // no memset: k_matrix_pack writes every byte before the scan reads it
    if ((cfg->flags & ABNN_MAT_LABELS) && !b->mat_pack) ST_TRY(b->pool.alloc_all({raw(&b->mat_pack, b->n_nrn)}));
    return ABNN_OK;
}

abnn_status matrix_launch(abnn_brain* b, const abnn_matrix_config* cfg, const uint32_t* bounds, const uint32_t* labels_dev,
                          uint64_t* out_dev, hipStream_t s)
{
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_matrix(b->d.syn, b->dims.n_syn, *cfg, bounds, labels_dev, b->n_nrn, b->kp.base_scale, b->mat_pack,
                          b->mat_path, out_dev, (uint32_t)b->cus, s));
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_matrix_enqueue(abnn_brain* b, const abnn_matrix_config* cfg, const uint32_t* bounds_host,
                                const uint32_t* labels_dev, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    ST_TRY(matrix_check(b, cfg, bounds_host, labels_dev, out_dev));
    return matrix_launch(b, cfg, bounds_host, labels_dev, out_dev, pick(b, stream));
}

abnn_status abnn_matrix(abnn_brain* b, const abnn_matrix_config* cfg, const uint32_t* bounds_host, const uint32_t* labels_dev,
                        uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    // every refusal comes before the scratch: a refused call allocates nothing and synchronises nothing
    ST_TRY(matrix_args_check(cfg, bounds_host, labels_dev, b->n_nrn));
    REQUIRE(words == matrix_words(cfg), "abnn_matrix: words must equal abnn_matrix_words(cfg)");
    ST_TRY(matrix_check(b, cfg, bounds_host, labels_dev, nullptr));
    ST_TRY(sync_all(b));
    ST_TRY(b->pool.grow(&b->mat_out, &b->mat_cap, words, false));
    ST_TRY(matrix_launch(b, cfg, bounds_host, labels_dev, b->mat_out, b->stream));
    return read_words(b, b->mat_out, out_host, words);
}

abnn_status abnn_matrix_host(const abnn_synapse* records, uint64_t n, const abnn_matrix_config* cfg, const uint32_t* bounds,
                             const uint32_t* labels, uint64_t n_nrn, float base_scale, uint64_t* out, uint64_t words)
{
    REQUIRE(cfg && out && (records || n == 0), "null argument");
    REQUIRE(n_nrn >= 1 && n_nrn < (1ull << 32), "matrix: n_nrn in 1 .. 2^32 - 1");
    ST_TRY(matrix_args_check(cfg, bounds, labels, n_nrn));
    REQUIRE(words == matrix_words(cfg), "abnn_matrix_host: words must equal abnn_matrix_words(cfg)");
    matrix_host(*cfg, bounds, labels, n_nrn, base_scale, records, n, out);
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): pin the kernel path of the handle's matrices.
abnn_status abnn_debug_set_matrix_path(abnn_brain* b, int path)
{
    REQUIRE(b, "null argument");
    REQUIRE(path >= 0 && path <= 4,
            "abnn_debug_set_matrix_path: 0 auto, 1 runs + packed, 2 runs + direct, 3 atomics + packed, 4 atomics + direct");
    b->mat_path = (uint32_t)path;
    return ABNN_OK;
}

/* ---- signal propagation (propagate.hip) ----------------------- */

uint64_t abnn_propagate_words(const abnn_propagate_config* cfg, uint64_t n_nrn) { return propagate_words(cfg, n_nrn); }

namespace {

constexpr const char* kPropConfig =
    "propagate: no unknown flags, reserved 0, a count of 0 only with first 0, both ranges inside N_NRN, "
    "w_lo / w_hi +0 without WEIGHT, with it no NaN bound and w_lo < w_hi";

// The checks of a propagation on handle b, then its scratch (the first call
// allocates it: that one may synchronise the device).
abnn_status propagate_check(abnn_brain* b, const abnn_propagate_config* cfg)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(propagate_config_ok(cfg, b->n_nrn, nullptr), kPropConfig);
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    // no memset: k_prop_map writes every word of the map, the rescale zeroes its words in stream order
    if (!b->prop.map)
        ST_TRY(b->pool.alloc_all({raw(&b->prop.map, (b->n_nrn + 31) / 32), raw(&b->prop.red, 2)}));
    return ABNN_OK;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

abnn_status propagate_launch(abnn_brain* b, const abnn_propagate_config* cfg, const int32_t* x_dev, uint64_t* out_dev,
                             hipStream_t s)
{
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_propagate(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, b->kp.base_scale, x_dev, out_dev, b->prop, b->prop_path,
                             (uint32_t)b->cus, s));
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_propagate_enqueue(abnn_brain* b, const abnn_propagate_config* cfg, const int32_t* x_dev, uint64_t* out_dev,
                                   void* stream)
{
    REQUIRE(b && cfg && x_dev && out_dev, "null argument");
    REQUIRE(aligned(x_dev, 16) && aligned(out_dev, 8), "propagate: x_dev must be 16-byte and out_dev 8-byte aligned");
    ST_TRY(propagate_check(b, cfg));
    return propagate_launch(b, cfg, x_dev, out_dev, pick(b, stream));
}

abnn_status abnn_propagate(abnn_brain* b, const abnn_propagate_config* cfg, const int32_t* x_host, uint64_t* out_host,
                           uint64_t words)
{
    REQUIRE(b && cfg && x_host && out_host, "null argument");
    ST_TRY(propagate_check(b, cfg));
    REQUIRE(words == propagate_words(cfg, b->n_nrn), "abnn_propagate: words must equal abnn_propagate_words(cfg, N_NRN)");
    ST_TRY(sync_all(b));
    if (!b->prop_x) ST_TRY(b->pool.alloc(raw(&b->prop_x, b->n_nrn)));
    ST_TRY(b->pool.grow(&b->prop_out, &b->prop_cap, words, false));
    HIP_TRY(hipMemcpyAsync(b->prop_x, x_host, b->n_nrn * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    ST_TRY(propagate_launch(b, cfg, b->prop_x, b->prop_out, b->stream));
    return read_words(b, b->prop_out, out_host, words);
}

abnn_status abnn_propagate_rescale_enqueue(abnn_brain* b, const abnn_propagate_config* cfg, const uint64_t* out_dev,
                                           int32_t* x_dev, uint64_t* trace_row_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev && x_dev, "null argument");
    REQUIRE(aligned(x_dev, 16) && aligned(out_dev, 8) && aligned(trace_row_dev, 8),
            "propagate: x_dev must be 16-byte, out_dev and trace_row_dev 8-byte aligned");
    ST_TRY(propagate_check(b, cfg));
    HIP_TRY(launch_propagate_rescale(*cfg, b->n_nrn, out_dev, x_dev, trace_row_dev, b->prop, (uint32_t)b->cus,
                                     pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_propagate_iterate_enqueue(abnn_brain* b, const abnn_propagate_config* cfg, uint32_t steps, int32_t* x_dev,
                                           uint64_t* work_dev, uint64_t* trace_dev, void* stream)
{
    REQUIRE(b && cfg && x_dev && work_dev && trace_dev, "null argument");
    REQUIRE(aligned(x_dev, 16) && aligned(work_dev, 8) && aligned(trace_dev, 8),
            "propagate: x_dev must be 16-byte, work_dev and trace_dev 8-byte aligned");
    ST_TRY(propagate_check(b, cfg));
    REQUIRE(steps >= 1 && steps <= kPropMaxSteps, "propagate: steps must be 1 .. 4096");
    REQUIRE(propagate_ranges_equal(*cfg), "propagate: iterate needs the in-range and the out-range to be the same");
    hipStream_t s = pick(b, stream);
    for (uint32_t k = 0; k < steps; ++k) {
        ST_TRY(propagate_launch(b, cfg, x_dev, work_dev, s));
        HIP_TRY(launch_propagate_rescale(*cfg, b->n_nrn, work_dev, x_dev, trace_dev + (uint64_t)k * ABNN_PROP_TRACE_WORDS,
                                         b->prop, (uint32_t)b->cus, s));
    }
    return ABNN_OK;
}

abnn_status abnn_propagate_host(const abnn_propagate_config* cfg, uint64_t n_nrn, float base_scale, const abnn_synapse* syn,
                                uint64_t n_syn, const int32_t* x, uint64_t* out)
{
    REQUIRE(cfg && x && out && (syn || n_syn == 0), "null argument");
    REQUIRE(propagate_config_ok(cfg, n_nrn, nullptr), kPropConfig);
    propagate_host(*cfg, n_nrn, base_scale, syn, n_syn, x, out);
    return ABNN_OK;
}

abnn_status abnn_propagate_rescale_host(const abnn_propagate_config* cfg, uint64_t n_nrn, const uint64_t* out, int32_t* x,
                                        uint64_t* trace_row)
{
    REQUIRE(cfg && out && x, "null argument");
    REQUIRE(propagate_config_ok(cfg, n_nrn, nullptr), kPropConfig);
    propagate_rescale_host(*cfg, n_nrn, out, x, trace_row);
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): pin the forward instance of the handle's propagations.
abnn_status abnn_debug_set_propagate_path(abnn_brain* b, int path)
{
    REQUIRE(b, "null argument");
    REQUIRE(path >= 0 && path <= 2, "abnn_debug_set_propagate_path: 0 auto, 1 sparse, 2 dense");
    b->prop_path = (uint32_t)path;
    return ABNN_OK;
}

/* ---- spike recorder (spikes.hip) --------------------------- */

namespace {

void spikes_free(abnn_brain* b)
{
    SpikeRecorder& r = b->spikes;
    b->pool.release(&r.words, &r.passes, &r.raster, &r.counts);
    r = SpikeRecorder{};
}

constexpr const char* kNoRecorder = "abnn_spikes: the handle has no recorder (abnn_spikes_start)";

}  // namespace

abnn_status abnn_spikes_start(abnn_brain* b, const abnn_spikes_config* cfg)
{
    REQUIRE(b && cfg, "null argument");
    ST_TRY(sync_all(b));  // launches of a running recorder write its buffers
    spikes_free(b);
    REQUIRE(cfg->reserved[0] == 0 && cfg->reserved[1] == 0 && cfg->counts <= 1,
            "abnn_spikes_start: reserved must be 0, counts 0 or 1");
    REQUIRE(cfg->pass_capacity >= 1, "abnn_spikes_start: pass_capacity must be at least 1");
    REQUIRE(!cfg->count || (uint64_t)cfg->first + cfg->count <= b->n_nrn, "abnn_spikes_start: the range ends above N_NRN");
    SpikeRecorder& r = b->spikes;
    r.cfg = *cfg;
    r.first = cfg->count ? cfg->first : 0u;
    r.n_counts = cfg->counts ? (cfg->count ? (uint64_t)cfg->count : b->n_nrn) : 0;
    std::vector<Slot> bufs = {zeroed(&r.words, kSpikeWords), zeroed(&r.passes, cfg->pass_capacity)};
    if (cfg->raster_capacity) bufs.push_back(zeroed(&r.raster, cfg->raster_capacity));
    if (r.n_counts) bufs.push_back(zeroed(&r.counts, r.n_counts));
    ST_TRY(b->pool.alloc_all(bufs));
    HIP_TRY(hipDeviceSynchronize());  // the buffers' zeros
    r.on = true;
    return ABNN_OK;
}

abnn_status abnn_spikes_stop(abnn_brain* b)
{
    REQUIRE(b, "null argument");
    REQUIRE(b->spikes.on, kNoRecorder);
    ST_TRY(sync_all(b));
    spikes_free(b);
    return ABNN_OK;
}

abnn_status abnn_spikes_clear(abnn_brain* b, int keep_counts)
{
    REQUIRE(b, "null argument");
    REQUIRE(b->spikes.on, kNoRecorder);
    ST_TRY(sync_all(b));
    SpikeRecorder& r = b->spikes;
    HIP_TRY(hipMemset(r.words + 3, 0, (kSpikeWords - 3) * sizeof(uint64_t)));  // recorded, dropped, the flag
    if (!keep_counts && r.counts) HIP_TRY(hipMemset(r.counts, 0, r.n_counts * sizeof(uint32_t)));
    HIP_TRY(hipDeviceSynchronize());
    return ABNN_OK;
}

abnn_status abnn_spikes_get_info(abnn_brain* b, abnn_spikes_info* out)
{
    REQUIRE(b && out, "null argument");
    REQUIRE(b->spikes.on, kNoRecorder);
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, b->spikes.words, sizeof(*out), hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_spikes_read_passes(abnn_brain* b, uint64_t first, uint64_t n, abnn_spike_pass* out)
{
    REQUIRE(b && (out || n == 0), "null argument");
    REQUIRE(b->spikes.on, kNoRecorder);
    abnn_spikes_info info{};
    ST_TRY(abnn_spikes_get_info(b, &info));
    REQUIRE(first <= info.passes_recorded && n <= info.passes_recorded - first,
            "abnn_spikes_read_passes: beyond the recorded passes");
    if (n) HIP_TRY(hipMemcpy(out, b->spikes.passes + first, n * sizeof(*out), hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_spikes_read_raster(abnn_brain* b, uint64_t first, uint64_t n, uint32_t* out)
{
    REQUIRE(b && (out || n == 0), "null argument");
    REQUIRE(b->spikes.on, kNoRecorder);
    abnn_spikes_info info{};
    ST_TRY(abnn_spikes_get_info(b, &info));
    const uint64_t have = b->spikes.raster ? info.spikes_recorded : 0;
    REQUIRE(first <= have && n <= have - first, "abnn_spikes_read_raster: beyond the recorded spikes");
    if (n) HIP_TRY(hipMemcpy(out, b->spikes.raster + first, n * sizeof(*out), hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_spikes_read_counts(abnn_brain* b, uint64_t first_neuron, uint64_t n, uint32_t* out)
{
    REQUIRE(b && (out || n == 0), "null argument");
    const SpikeRecorder& r = b->spikes;
    REQUIRE(r.on, kNoRecorder);
    REQUIRE(r.counts, "abnn_spikes_read_counts: the recorder keeps no counts");
    REQUIRE(first_neuron >= r.first && first_neuron - r.first <= r.n_counts && n <= r.n_counts - (first_neuron - r.first),
            "abnn_spikes_read_counts: neurons outside the selected range");
    ST_TRY(sync_all(b));
    if (n) HIP_TRY(hipMemcpy(out, r.counts + (first_neuron - r.first), n * sizeof(*out), hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_spikes_load(abnn_brain* b, const abnn_spike_pass* passes, uint64_t n_passes, const uint32_t* raster,
                             uint64_t n_raster)
{
    REQUIRE(b && (passes || n_passes == 0) && (raster || n_raster == 0), "null argument");
    const SpikeRecorder& r = b->spikes;
    REQUIRE(r.on, kNoRecorder);
    REQUIRE(r.raster, "abnn_spikes_load: the recorder keeps no raster");
    REQUIRE(n_passes <= r.cfg.pass_capacity && n_raster <= r.cfg.raster_capacity,
            "abnn_spikes_load: more passes or spikes than the recorder holds");
    uint64_t at = 0;
    for (uint64_t k = 0; k < n_passes; ++k) {
        REQUIRE(passes[k].offset == at && passes[k].count <= n_raster - at,
                "abnn_spikes_load: the offsets must be 0, count_0, count_0 + count_1, ... inside the raster");
        at += passes[k].count;
    }
    REQUIRE(at == n_raster, "abnn_spikes_load: the counts must sum to n_raster");
    for (uint64_t i = 0; i < n_raster; ++i) {
        REQUIRE(raster[i] < b->n_nrn, "abnn_spikes_load: an id at or above N_NRN");
        REQUIRE(!r.cfg.count || raster[i] - r.cfg.first < r.cfg.count, "abnn_spikes_load: an id outside the recorder's range");
    }
    ST_TRY(sync_all(b));
    if (n_passes) HIP_TRY(hipMemcpy(r.passes, passes, n_passes * sizeof(*passes), hipMemcpyHostToDevice));
    if (n_raster) HIP_TRY(hipMemcpy(r.raster, raster, n_raster * sizeof(*raster), hipMemcpyHostToDevice));
    const uint64_t tail[kSpikeWords - 3] = {n_passes, n_raster, 0, 0, 0};  // recorded, dropped, the flag
    HIP_TRY(hipMemcpy(r.words + 3, tail, sizeof(tail), hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    return ABNN_OK;
}

/* ---- spike correlograms (corr.hip) --------------------------- */

uint64_t abnn_corr_words(const abnn_corr_config* cfg) { return corr_words(cfg); }

namespace {

constexpr const char* kCorrConfig =
    "corr: mode POP / PAIRS / SYNAPSES, no unknown flags, max_lag <= 256, ranges inside N_NRN, PAIRS with both counts "
    ">= 1 and at most 2^24 plane words, reserved 0, w_lo / w_hi +0 without WEIGHT, with it no NaN bound and w_lo < w_hi";

// The checks of a correlogram on handle b, then its scratch (the first call,
// and the first after the recorder was restarted larger, allocates it: that
// one may synchronise the device).
abnn_status corr_check(abnn_brain* b, const abnn_corr_config* cfg)
{
    REQUIRE(b && cfg, "null argument");
    REQUIRE(corr_config_ok(cfg, nullptr) && corr_ranges_ok(*cfg, b->n_nrn), kCorrConfig);
    REQUIRE(b->spikes.on, kNoRecorder);
    REQUIRE(b->spikes.raster, "corr: the recorder keeps no raster");
    REQUIRE(cfg->mode != ABNN_CORR_SYNAPSES || !b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    CorrScratch& c = b->corr;
    // no memset: every word is written before it is read (launch_corr)
    if (!c.map)
        ST_TRY(b->pool.alloc_all({raw(&c.map, corr_map_words(b->n_nrn)), raw(&c.cnt, b->n_nrn),
                                  raw(&c.off, b->n_nrn), raw(&c.cur, b->n_nrn), raw(&c.cursor, 2)}));
    ST_TRY(b->pool.grow(&c.rows, &c.raster_cap, b->spikes.cfg.raster_capacity, false));
    ST_TRY(b->pool.grow(&c.tally, &c.pass_cap, b->spikes.cfg.pass_capacity, false));
    return ABNN_OK;
}

}  // namespace

abnn_status abnn_corr_enqueue(abnn_brain* b, const abnn_corr_config* cfg, uint64_t* out_dev, void* stream)
{
    REQUIRE(b && cfg && out_dev, "null argument");
    REQUIRE((reinterpret_cast<uintptr_t>(out_dev) & 7u) == 0, "corr: out_dev must be 8-byte aligned");
    ST_TRY(corr_check(b, cfg));
    // the host knows n_syn: structural updates synchronise
    HIP_TRY(launch_corr(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, b->spikes, b->corr, out_dev, (uint32_t)b->cus,
                        pick(b, stream)));
    return ABNN_OK;
}

abnn_status abnn_corr(abnn_brain* b, const abnn_corr_config* cfg, uint64_t* out_host, uint64_t words)
{
    REQUIRE(b && cfg && out_host, "null argument");
    ST_TRY(corr_check(b, cfg));
    REQUIRE(words == corr_words(cfg), "abnn_corr: words must equal abnn_corr_words(cfg)");
    ST_TRY(sync_all(b));
    ST_TRY(b->pool.grow(&b->corr_out, &b->corr_cap, words));
    HIP_TRY(launch_corr(b->d.syn, b->dims.n_syn, *cfg, b->n_nrn, b->spikes, b->corr, b->corr_out, (uint32_t)b->cus,
                        b->stream));
    return read_words(b, b->corr_out, out_host, words);
}

abnn_status abnn_corr_host(const abnn_corr_config* cfg, uint64_t n_nrn, const abnn_spike_pass* passes, uint64_t n_passes,
                           const uint32_t* raster, uint64_t n_raster, const abnn_synapse* records, uint64_t n_records,
                           uint64_t* out)
{
    REQUIRE(cfg && out && (passes || n_passes == 0) && (raster || n_raster == 0) && (records || n_records == 0),
            "null argument");
    REQUIRE(n_nrn < (1ull << 32) && corr_config_ok(cfg, nullptr) && corr_ranges_ok(*cfg, n_nrn), kCorrConfig);
    corr_host(*cfg, n_nrn, passes, n_passes, raster, n_raster, records, n_records, out);
    return ABNN_OK;
}

abnn_status abnn_get_last_fired(abnn_brain* b, uint64_t first, uint64_t* out, uint64_t n)
{
    REQUIRE(b && (out || n == 0), "null argument");
    REQUIRE(first <= b->n_nrn && n <= b->n_nrn - first, "range out of bounds");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, b->d.last_fired + first, n * 8, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_set_last_fired(abnn_brain* b, uint64_t first, const uint64_t* src, uint64_t n)
{
    REQUIRE(b && (src || n == 0), "null argument");
    REQUIRE(first <= b->n_nrn && n <= b->n_nrn - first, "range out of bounds");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(b->d.last_fired + first, src, n * 8, hipMemcpyHostToDevice));
    state_written(b, n ? *std::max_element(src, src + n) : 0);
    return ABNN_OK;
}

abnn_status abnn_get_last_visited(abnn_brain* b, uint64_t first, uint64_t* out, uint64_t n)
{
    REQUIRE(b && (out || n == 0), "null argument");
    REQUIRE(first <= b->n_nrn && n <= b->n_nrn - first, "range out of bounds");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, b->d.last_visited + first, n * 8, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_set_last_visited(abnn_brain* b, uint64_t first, const uint64_t* src, uint64_t n)
{
    REQUIRE(b && (src || n == 0), "null argument");
    REQUIRE(first <= b->n_nrn && n <= b->n_nrn - first, "range out of bounds");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(b->d.last_visited + first, src, n * 8, hipMemcpyHostToDevice));
    // a host write is replicated on every shard (the neuron state is): it
    // replaces whatever this shard visited before it
    if (b->d.visit_mark && n) HIP_TRY(hipMemset(b->d.visit_mark + first, 0, n));
    // a write of the whole array leaves no unmerged mark (as abnn_load_flat):
    // a single-rank restore may then move the clock back (abnn_set_scalars)
    if (first == 0 && n == b->n_nrn) b->marks_dirty = false;
    return ABNN_OK;
}

abnn_status abnn_set_timestamps(abnn_brain* b, const uint32_t* idx, uint64_t n, uint64_t value)
{
    REQUIRE(b && (idx || n == 0), "null argument");
    for (uint64_t i = 0; i < n; ++i) REQUIRE(idx[i] < b->n_nrn, "neuron index out of range");
    ST_TRY(sync_all(b));
    ST_TRY(ensure_idx_scratch(b, n));
    HIP_TRY(hipMemcpy(b->idx_scratch, idx, n * 4, hipMemcpyHostToDevice));
    HIP_TRY(launch_stamp_list(b->d, b->idx_scratch, n, nullptr, value, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    state_written(b, value);
    return ABNN_OK;
}

abnn_status abnn_get_scalars(abnn_brain* b, abnn_scalars* out)
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    uint64_t blk[3];
    HIP_TRY(hipMemcpy(blk, b->scalar_block, sizeof(blk), hipMemcpyDeviceToHost));
    out->clock = blk[0];
    std::memcpy(&out->reward, reinterpret_cast<char*>(blk) + 8, 4);
    std::memcpy(&out->rbar, reinterpret_cast<char*>(blk) + 12, 4);
    out->pass_index = blk[2];
    return ABNN_OK;
}

abnn_status abnn_set_scalars(abnn_brain* b, const abnn_scalars* in)
{
    REQUIRE(b && in, "null argument");
    // the merge takes the largest value among the shards that visited a
    // neuron: the clock must not move back over unmerged visits
    REQUIRE(!(b->marks_dirty && in->clock < b->clock_host),
            "the clock moves back over unmerged lastVisited stamps: merge them first "
            "(abnn_comm_sync_visits, or abnn_shard_visits_delta / _merge) on every rank");
    ST_TRY(sync_all(b));
    uint64_t blk[3];
    blk[0] = in->clock;
    std::memcpy(reinterpret_cast<char*>(blk) + 8, &in->reward, 4);
    std::memcpy(reinterpret_cast<char*>(blk) + 12, &in->rbar, 4);
    blk[2] = in->pass_index;
    HIP_TRY(hipMemcpy(b->scalar_block, blk, sizeof(blk), hipMemcpyHostToDevice));
    state_written(b, b->clock_host);  // every stamp so far is <= the old clock
    b->clock_host = in->clock;
    b->pass_host = in->pass_index;
    return ABNN_OK;
}

abnn_status abnn_set_reward(abnn_brain* b, float r)
{
    REQUIRE(b, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(b->d.reward, &r, 4, hipMemcpyHostToDevice));
    return ABNN_OK;
}

abnn_status abnn_inject_inputs(abnn_brain* b, const float* v, uint32_t n, float hz)
{
    REQUIRE(b && (v || n == 0), "null argument");
    REQUIRE(n == b->dims.n_input, "inject_inputs: size must equal n_input (brain.cpp:75)");
    // pTick = hz * kTickNS * NSEC_PER_SEC, all in float (brain.cpp:76)
    float p_tick = hz * (float)b->params.tick_ns;
    p_tick = p_tick * (float)1000000000ull;
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < n; ++i) {
        b->rng += 0x9E3779B97F4A7C15ull;  // SplitMix64 step
        uint64_t z = b->rng;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        const float uni = (float)(z >> 40) * (1.0f / 16777216.0f);
        if (uni < p_tick * v[i]) idx.push_back(i);  // brain.cpp:82
    }
    ST_TRY(sync_all(b));
    if (idx.empty()) return ABNN_OK;
    ST_TRY(ensure_idx_scratch(b, idx.size()));
    HIP_TRY(hipMemcpy(b->idx_scratch, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
    // lastFired[i] = clock, read on the device
    HIP_TRY(launch_stamp_list(b->d, b->idx_scratch, idx.size(), b->d.clock, 0, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    state_written(b, b->clock_host);
    return ABNN_OK;
}

abnn_status abnn_read_outputs(abnn_brain* b, uint8_t* out, uint32_t n)
{
    REQUIRE(b && (out || n == 0), "null argument");
    REQUIRE(n == b->dims.n_output, "read_outputs: size must equal n_output");
    ST_TRY(sync_all(b));
    std::vector<uint64_t> lf(n);
    uint64_t clk = 0;
    if (n) HIP_TRY(hipMemcpy(lf.data(), b->d.last_fired + b->dims.n_input, n * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&clk, b->d.clock, 8, hipMemcpyDeviceToHost));
    // u32 timestamps, as the reference's (brain.cpp:149-153): the low 32 bits
    const uint32_t now = (uint32_t)clk, start = now > 1 ? now - 1 : 0;  // brain.cpp:151
    for (uint32_t o = 0; o < n; ++o) {
        const uint32_t ts = (uint32_t)lf[o];
        out[o] = (ts != 0 && ts >= start && ts < now) ? 1 : 0;  // brain.cpp:153-154
    }
    return ABNN_OK;
}

abnn_status abnn_set_auto_stimulus(abnn_brain* b, uint64_t first, uint64_t count)
{
    REQUIRE(b, "null argument");
    REQUIRE(count == 0 || (first < b->n_nrn && count <= b->n_nrn - first), "range out of bounds");
    b->stim_first = count ? first : 0;
    b->stim_count = count;
    return ABNN_OK;
}

abnn_status abnn_traverse(abnn_brain* b, uint32_t passes, void* stream)
{
    REQUIRE(b, "null argument");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    ST_TRY(pass_error(b));  // a pass already completed failed: enqueue nothing more
    if (b->d.visit_mark && passes) b->marks_dirty = true;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = pick(b, stream);
    for (uint32_t i = 0; i < passes; ++i) ST_TRY(run_pass(b, s));
    return ABNN_OK;
}

abnn_status abnn_synchronize(abnn_brain* b, void* stream)
{
    REQUIRE(b, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    return sync_all(b);
}

uint64_t abnn_exchange_bytes(const abnn_brain* b)
{
    return b ? 4ull * xchg_words(b->params.max_spikes) : 0;
}

abnn_status abnn_set_global_events(abnn_brain* b, uint64_t global_events)
{
    REQUIRE(b, "null argument");
    b->dims.global_events = global_events;
    return ABNN_OK;
}

abnn_status abnn_shard_gate(abnn_brain* b, void* xchg_dev, void* stream)
{
    REQUIRE(b && xchg_dev, "null argument");
    REQUIRE(((uintptr_t)xchg_dev & 7u) == 0, "exchange record must be 8-B aligned");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    HIP_TRY(hipSetDevice(b->device));
    ST_TRY(ensure_visit_marks(b));
    if (b->d.visit_mark) b->marks_dirty = true;
    hipStream_t s = pick(b, stream);
    b->pending_renorm = renorm_due(b);
    return run_gate(b, static_cast<int32_t*>(xchg_dev), s);
}

abnn_status abnn_shard_apply(abnn_brain* b, const void* gathered_dev, uint32_t world, uint32_t rank,
                             void* stream)
{
    REQUIRE(b && gathered_dev, "null argument");
    REQUIRE(world >= 1 && rank < world, "bad world/rank");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = pick(b, stream);
    return run_apply(b, static_cast<const int32_t*>(gathered_dev), world, rank, s);
}

abnn_status abnn_shard_commit(abnn_brain* b, const void* gathered_dev, uint32_t world, void* stream)
{
    REQUIRE(b && gathered_dev, "null argument");
    REQUIRE(world >= 1, "bad world");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = pick(b, stream);
    const bool renorm = b->pending_renorm;
    b->pending_renorm = false;
    return run_commit(b, static_cast<const int32_t*>(gathered_dev), world, renorm, s);
}

// The lastVisited merge over a caller's exchange (abnn.h): this shard's deltas,
// then the all-reduced ones applied.
abnn_status abnn_shard_visits_delta(abnn_brain* b, void* delta_dev, void* stream)
{
    REQUIRE(b && delta_dev, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = pick(b, stream);
    uint64_t* delta = static_cast<uint64_t*>(delta_dev);
    if (!b->params.track_visits) {  // lastVisited is never written: nothing to merge
        HIP_TRY(hipMemsetAsync(delta, 0, b->n_nrn * 8, s));
        return ABNN_OK;
    }
    ST_TRY(ensure_visit_marks(b));
    HIP_TRY(launch_visits_delta(b->d.last_visited, b->d.visit_mark, delta, b->n_nrn, s));
    return ABNN_OK;
}

abnn_status abnn_shard_visits_merge(abnn_brain* b, const void* reduced_dev, void* stream)
{
    REQUIRE(b && reduced_dev, "null argument");
    HIP_TRY(hipSetDevice(b->device));
    if (!b->params.track_visits) return ABNN_OK;
    ST_TRY(ensure_visit_marks(b));
    HIP_TRY(launch_visits_merge(b->d.last_visited, b->d.visit_mark, static_cast<const uint64_t*>(reduced_dev), b->n_nrn,
                                pick(b, stream)));
    b->marks_dirty = false;
    return ABNN_OK;
}

// ---- sharded passes over RCCL ------------------------------------------------

struct abnn_comm {
    ncclComm_t comm = nullptr;
    abnn_comm_group* local = nullptr;  // in-process group (abnn_comm_create_local): no RCCL
    uint32_t world = 1, rank = 0;
    int device = 0;
    DevicePool pool;            // owns the device buffers below
    char* gathered = nullptr;   // world exchange records, rank order
    uint64_t rec_bytes = 0;
    uint64_t* scratch = nullptr;  // visited-events all-reduce
    uint64_t* visits = nullptr;   // the lastVisited merge's deltas (n_nrn words, sized on first use)
    uint64_t visits_n = 0;
    bool broken = false;          // an earlier pass failed on this rank (abnn.h: abort on every rank)
    // in-process group: this rank's events (its stream reached the collective /
    // its reads of the peers' buffers are enqueued) and the all-reduce's
    // accumulator and peer staging buffer (sized on first use)
    hipEvent_t ev_ready = nullptr, ev_done = nullptr;
    uint64_t* red_acc = nullptr;
    uint64_t* red_in = nullptr;
    uint64_t red_n = 0;
};

// ---- in-process communicator group (abnn.h abnn_comm_group) -----------------
// `world` ranks in ONE process, one host thread per rank (SURVEY §4 item 4's
// fake communicator behind the same comm interface): the collectives
// abnn_shard_traverse / abnn_comm_sync_visits need -- the in-place all-gather
// of the exchange records and the all-reduce(MAX / SUM) of u64 words -- are
// device copies and a reduction kernel on each rank's own stream, between two
// host barriers:
//   1. every rank records ev_ready on its stream (its inputs are enqueued),
//      barrier;
//   2. every rank's stream waits for the peers' ev_ready, copies / reduces the
//      peers' buffers into its own (rank order), records ev_done, barrier;
//   3. every rank's stream waits for the peers' ev_done (no rank overwrites a
//      buffer a peer still reads).
// No GPU work ever waits for the host, so a rank blocked in a host
// synchronisation never holds up a peer.  Ranks on one device must pass one
// stream (a pass keeps one workgroup per CU resident for its look-back: two
// passes must not run at once); ranks on different devices copy over
// xGMI/PCIe (hipMemcpyDefault).  A barrier that waits longer than
// kGroupTimeout, or a rank that fails (abnn_shard_traverse error), breaks the
// group: every later collective on it fails at once.
struct abnn_comm_group {
    uint32_t world = 0;
    std::mutex m;
    std::condition_variable cv;
    uint64_t gen = 0;       // barrier generation
    uint32_t arrived = 0;
    bool broken = false;
    std::string why;
    std::vector<abnn_comm*> ranks;     // registered communicators (null: free slot)
    std::vector<const char*> buf;      // this collective's buffer of every rank
    std::vector<hipStream_t> streams;  // ... and its stream
};

namespace {

constexpr auto kGroupTimeout = std::chrono::seconds(300);

void group_break(abnn_comm_group* g, const std::string& why)
{
    std::lock_guard<std::mutex> lk(g->m);
    if (!g->broken) g->why = why;
    g->broken = true;
    g->cv.notify_all();
}

abnn_status group_barrier(abnn_comm_group* g)
{
    std::unique_lock<std::mutex> lk(g->m);
    if (g->broken) {
        set_err("local communicator group is broken: " + g->why);
        return ABNN_ERR_INVALID;
    }
    const uint64_t my = g->gen;
    if (++g->arrived == g->world) {
        g->arrived = 0;
        ++g->gen;
        g->cv.notify_all();
        return ABNN_OK;
    }
    if (!g->cv.wait_for(lk, kGroupTimeout, [&] { return g->gen != my || g->broken; })) {
        g->broken = true;
        g->why = "a rank did not reach a collective within 300 s";
        g->cv.notify_all();
    }
    if (g->broken) {
        set_err("local communicator group is broken: " + g->why);
        return ABNN_ERR_INVALID;
    }
    return ABNN_OK;
}

// Steps 1-2 of a collective: publish (buf, s), wait for every rank, check the
// stream rule, and make s wait for every peer's inputs.
abnn_status group_enter(abnn_comm* c, const void* buf, hipStream_t s)
{
    abnn_comm_group* g = c->local;
    g->buf[c->rank] = static_cast<const char*>(buf);
    g->streams[c->rank] = s;
    HIP_TRY(hipEventRecord(c->ev_ready, s));
    ST_TRY(group_barrier(g));
    for (uint32_t j = 0; j < g->world; ++j) {
        if (j == c->rank) continue;
        if (g->ranks[j]->device == c->device && g->streams[j] != s) {
            // every rank sees the same mismatch and fails the same way
            set_err("local communicator: ranks on one device must pass the same stream (their passes must not "
                    "run at once)");
            return ABNN_ERR_INVALID;
        }
        HIP_TRY(hipStreamWaitEvent(s, g->ranks[j]->ev_ready, 0));
    }
    return ABNN_OK;
}

// Step 3: the peers' reads of this rank's buffer are enqueued before s goes on.
abnn_status group_leave(abnn_comm* c, hipStream_t s)
{
    abnn_comm_group* g = c->local;
    HIP_TRY(hipEventRecord(c->ev_done, s));
    ST_TRY(group_barrier(g));
    for (uint32_t j = 0; j < g->world; ++j)
        if (j != c->rank) HIP_TRY(hipStreamWaitEvent(s, g->ranks[j]->ev_done, 0));
    return ABNN_OK;
}

abnn_status local_all_gather(abnn_comm* c, char* recv, uint64_t bytes, hipStream_t s)
{
    abnn_comm_group* g = c->local;
    ST_TRY(group_enter(c, recv, s));
    for (uint32_t j = 0; j < g->world; ++j)  // slot j of every rank's buffer = rank j's record
        if (j != c->rank)
            HIP_TRY(hipMemcpyAsync(recv + bytes * j, g->buf[j] + bytes * j, bytes, hipMemcpyDefault, s));
    return group_leave(c, s);
}

abnn_status local_all_reduce_u64(abnn_comm* c, uint64_t* buf, uint64_t n, bool max, hipStream_t s)
{
    abnn_comm_group* g = c->local;
    if (c->red_n < n) {  // before the barrier: a failed allocation must not leave peers waiting in step 2
        c->pool.release(&c->red_acc, &c->red_in);
        c->red_n = 0;
        if (c->pool.alloc_all({zeroed(&c->red_acc, n), zeroed(&c->red_in, n)}) != ABNN_OK) {
            group_break(g, "rank " + std::to_string(c->rank) + " could not allocate the all-reduce buffers");
            return ABNN_ERR_OOM;
        }
        c->red_n = n;
    }
    ST_TRY(group_enter(c, buf, s));
    HIP_TRY(hipMemcpyAsync(c->red_acc, buf, n * 8, hipMemcpyDefault, s));
    for (uint32_t j = 0; j < g->world; ++j) {
        if (j == c->rank) continue;
        HIP_TRY(hipMemcpyAsync(c->red_in, g->buf[j], n * 8, hipMemcpyDefault, s));
        HIP_TRY(launch_reduce_u64(c->red_acc, c->red_in, n, max, s));
    }
    ST_TRY(group_leave(c, s));
    HIP_TRY(hipMemcpyAsync(buf, c->red_acc, n * 8, hipMemcpyDefault, s));
    return ABNN_OK;
}

}  // namespace

// The collectives of the sharded pass, over RCCL or the in-process group.
static abnn_status comm_all_gather(abnn_comm* c, char* recv, uint64_t bytes, hipStream_t s)
{
    if (c->local) return local_all_gather(c, recv, bytes, s);
    RCCL_TRY(rccl_api().all_gather(recv + bytes * c->rank, recv, bytes, ncclInt8, c->comm, s));  // in place
    return ABNN_OK;
}

static abnn_status comm_all_reduce_u64(abnn_comm* c, uint64_t* buf, uint64_t n, bool max, hipStream_t s)
{
    if (c->local) return local_all_reduce_u64(c, buf, n, max, s);
    RCCL_TRY(rccl_api().all_reduce(buf, buf, n, ncclUint64, max ? ncclMax : ncclSum, c->comm, s));
    return ABNN_OK;
}

// The lastVisited merge on the stream: every rank's deltas
// (k_visits_delta), one all-reduce(MAX) of n_nrn words in place, the merge.
static abnn_status merge_visits(abnn_brain* b, abnn_comm* c, hipStream_t s)
{
    if (!b->params.track_visits) return ABNN_OK;  // lastVisited is never written
    ST_TRY(ensure_visit_marks(b));
    if (c->visits_n != b->n_nrn) {
        c->pool.release(&c->visits);
        c->visits_n = 0;
        ST_TRY(c->pool.alloc(zeroed(&c->visits, b->n_nrn)));
        c->visits_n = b->n_nrn;
    }
    HIP_TRY(launch_visits_delta(b->d.last_visited, b->d.visit_mark, c->visits, b->n_nrn, s));
    ST_TRY(comm_all_reduce_u64(c, c->visits, b->n_nrn, true, s));
    HIP_TRY(launch_visits_merge(b->d.last_visited, b->d.visit_mark, c->visits, b->n_nrn, s));
    b->marks_dirty = false;
    return ABNN_OK;
}

abnn_status abnn_comm_unique_id(void* id_out)
{
    REQUIRE(id_out, "null argument");
    const RcclApi& r = rccl_api();
    if (!r.ok) {
        set_err("RCCL (librccl) not found");
        return ABNN_ERR_NO_DEVICE;
    }
    ncclUniqueId id;
    RCCL_TRY(r.get_unique_id(&id));
    std::memcpy(id_out, &id, sizeof(id));
    return ABNN_OK;
}

abnn_status abnn_comm_create(const void* id, uint32_t world, uint32_t rank, int device, abnn_comm** out)
{
    REQUIRE(id && out && world >= 1 && rank < world, "bad argument");
    static_assert(sizeof(ncclUniqueId) == ABNN_COMM_ID_BYTES, "unique id size");
    *out = nullptr;
    const RcclApi& r = rccl_api();
    if (!r.ok) {
        set_err("RCCL (librccl) not found");
        return ABNN_ERR_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    abnn_comm* c = new (std::nothrow) abnn_comm();
    if (!c) return ABNN_ERR_OOM;
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    const ncclResult_t e = r.comm_init_rank(&c->comm, (int)world, uid, (int)rank);
    if (e != ncclSuccess) {
        set_err(std::string("ncclCommInitRank: ") + r.error_string(e));
        delete c;
        return ABNN_ERR_HIP;
    }
    c->world = world;
    c->rank = rank;
    c->device = device;
    if (c->pool.alloc(zeroed(&c->scratch, 1)) != ABNN_OK) {
        abnn_comm_destroy(c);
        return ABNN_ERR_OOM;
    }
    *out = c;
    return ABNN_OK;
}

abnn_status abnn_comm_destroy(abnn_comm* c)
{
    if (!c) return ABNN_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->comm) rccl_api().comm_destroy(c->comm);
    if (c->local) {
        std::lock_guard<std::mutex> lk(c->local->m);
        c->local->ranks[c->rank] = nullptr;
    }
    c->pool.release_all();
    if (c->ev_ready) (void)hipEventDestroy(c->ev_ready);
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    delete c;
    return ABNN_OK;
}

abnn_status abnn_comm_group_create(uint32_t world, abnn_comm_group** out)
{
    REQUIRE(out && world >= 1 && world <= 4096, "bad argument");
    abnn_comm_group* g = new (std::nothrow) abnn_comm_group();
    if (!g) return ABNN_ERR_OOM;
    g->world = world;
    g->ranks.assign(world, nullptr);
    g->buf.assign(world, nullptr);
    g->streams.assign(world, nullptr);
    *out = g;
    return ABNN_OK;
}

abnn_status abnn_comm_group_destroy(abnn_comm_group* g)
{
    if (!g) return ABNN_OK;
    {
        std::lock_guard<std::mutex> lk(g->m);
        for (abnn_comm* c : g->ranks)
            REQUIRE(c == nullptr, "abnn_comm_group_destroy: destroy every rank's communicator first");
    }
    delete g;
    return ABNN_OK;
}

abnn_status abnn_comm_create_local(abnn_comm_group* g, uint32_t rank, int device, abnn_comm** out)
{
    REQUIRE(g && out, "null argument");
    REQUIRE(rank < g->world, "rank out of range");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    abnn_comm* c = new (std::nothrow) abnn_comm();
    if (!c) return ABNN_ERR_OOM;
    c->local = g;
    c->world = g->world;
    c->rank = rank;
    c->device = device;
    if (hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming) != hipSuccess ||
        c->pool.alloc(zeroed(&c->scratch, 1)) != ABNN_OK) {
        c->local = nullptr;
        abnn_comm_destroy(c);
        set_err("abnn_comm_create_local: event or buffer allocation failed");
        return ABNN_ERR_OOM;
    }
    {
        std::lock_guard<std::mutex> lk(g->m);
        if (g->ranks[rank] != nullptr) {
            c->local = nullptr;
            abnn_comm_destroy(c);
            set_err("abnn_comm_create_local: rank already has a communicator in this group");
            return ABNN_ERR_INVALID;
        }
        g->ranks[rank] = c;
    }
    *out = c;
    return ABNN_OK;
}

// One sharded pass per iteration.  An error part-way through a pass leaves
// the other ranks inside (or about to enter) the pass's collectives, so the
// communicator is marked broken: every later call on it fails at once, and
// the caller must abort / destroy it on every rank (abnn.h).  The handle's
// half-done pass is dropped (no walk of a gate whose exchange never came).
static abnn_status shard_traverse_passes(abnn_brain* b, abnn_comm* c, uint32_t passes, hipStream_t s)
{
    const uint64_t rec = abnn_exchange_bytes(b);
    if (rec != c->rec_bytes) {  // the records' size follows the budget: sized on first use
        c->pool.release(&c->gathered);
        ST_TRY(c->pool.alloc(zeroed(&c->gathered, rec * c->world)));
        c->rec_bytes = rec;
    }
    char* mine = c->gathered + rec * c->rank;
    for (uint32_t i = 0; i < passes; ++i) {
        ST_TRY(abnn_shard_gate(b, mine, s));
        ST_TRY(comm_all_gather(c, c->gathered, rec, s));  // in place, rank order
        ST_TRY(abnn_shard_apply(b, c->gathered, c->world, c->rank, s));
        const uint64_t updates = b->structural_updates, renorms = b->renorms;
        ST_TRY(abnn_shard_commit(b, c->gathered, c->world, s));
        // the clock went back: merge lastVisited before the next pass stamps
        // smaller values than this epoch's
        if (b->renorms != renorms && b->params.track_visits) ST_TRY(merge_visits(b, c, s));
        if (b->structural_updates != updates) {
            // every shard's record count changed (all ranks update after the
            // same pass): re-sum the visited events for the clock-tick rule
            uint64_t mine_ev = visited_events(b->dims, b->params.mode), tot = 0;
            HIP_TRY(hipMemcpyAsync(c->scratch, &mine_ev, 8, hipMemcpyHostToDevice, s));
            ST_TRY(comm_all_reduce_u64(c, c->scratch, 1, false, s));
            HIP_TRY(hipMemcpyAsync(&tot, c->scratch, 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            b->dims.global_events = tot;
        }
    }
    return ABNN_OK;
}

static abnn_status shard_traverse_checked(abnn_brain* b, abnn_comm* c, uint32_t passes, void* stream)
{
    REQUIRE(b, "null argument");
    REQUIRE(c->device == b->device, "communicator and handle are on different devices");
    REQUIRE(!c->broken, "communicator unusable after an earlier error on this rank: abort / destroy it on every rank");
    HIP_TRY(hipSetDevice(b->device));
    ST_TRY(pass_error(b));
    return shard_traverse_passes(b, c, passes, pick(b, stream));
}

abnn_status abnn_shard_traverse(abnn_brain* b, abnn_comm* c, uint32_t passes, void* stream)
{
    REQUIRE(c, "null argument");
    const abnn_status st = shard_traverse_checked(b, c, passes, stream);
    if (st != ABNN_OK) {
        c->broken = true;
        if (b) b->pending_walk = false;
        // the peers are in (or about to enter) this pass's collectives: an
        // in-process group lets them fail at once (RCCL ranks abort)
        if (c->local) group_break(c->local, "rank " + std::to_string(c->rank) + ": " + g_err);
    }
    return st;
}

// Diagnostics (abnn_debug.h): `count` in-place all-gathers of `bytes` per
// rank from `buf` (rank order, world x bytes), the sharded pass's exchange
// alone (tools/allgather_time.py).
abnn_status abnn_debug_comm_allgather(abnn_comm* c, void* buf, uint64_t bytes, uint32_t count, void* stream)
{
    REQUIRE(c && buf, "null argument");
    REQUIRE(!c->broken, "communicator unusable after an earlier error on this rank: abort / destroy it on every rank");
    HIP_TRY(hipSetDevice(c->device));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(buf);
    for (uint32_t i = 0; i < count; ++i) ST_TRY(comm_all_gather(c, base, bytes, s));
    return ABNN_OK;
}

abnn_status abnn_comm_sync_visits(abnn_brain* b, abnn_comm* c, void* stream)
{
    REQUIRE(b && c, "null argument");
    REQUIRE(c->device == b->device, "communicator and handle are on different devices");
    REQUIRE(!c->broken, "communicator unusable after an earlier error on this rank: abort / destroy it on every rank");
    ST_TRY(sync_all(b));
    hipStream_t s = pick(b, stream);
    abnn_status st = merge_visits(b, c, s);
    if (st == ABNN_OK && hipStreamSynchronize(s) != hipSuccess) {
        set_err("hipStreamSynchronize failed after the lastVisited merge");
        st = ABNN_ERR_HIP;
    }
    if (st != ABNN_OK) {
        c->broken = true;
        if (c->local) group_break(c->local, "rank " + std::to_string(c->rank) + ": " + g_err);
    }
    return st;
}

// Diagnostics (not part of abnn.h): record the per-wave gate times of the
// following passes (on) or not (off, the default).
abnn_status abnn_debug_set_wave_clock(abnn_brain* b, int on)
{
    REQUIRE(b, "null argument");
    b->d.wave_clock_on = on ? 1u : 0u;
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): the last pass's per-wave gate times,
// kWaveClock u64 per range (engine.h, DeviceState::wave_clock), 100 MHz ticks.
abnn_status abnn_debug_wave_clock_slot(abnn_brain* b, uint32_t slot, uint64_t* out, uint64_t n)
{
    REQUIRE(b && out, "null argument");
    REQUIRE(slot < kWaveClockPasses, "slot out of range");
    ST_TRY(sync_all(b));
    const uint64_t per = (uint64_t)kWaveClock * kMaxRanges;
    HIP_TRY(hipMemcpy(out, b->d.wave_clock + slot * per, std::min<uint64_t>(n, per) * 8, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_debug_wave_clock(abnn_brain* b, uint64_t* out, uint64_t n)
{
    REQUIRE(b, "null argument");
    // a fused pass p writes slot p % kWaveClockPasses, the two-kernel gate slot 0
    const uint32_t slot = b->last_pass_fused && b->pass_host ? (uint32_t)((b->pass_host - 1) % kWaveClockPasses) : 0u;
    return abnn_debug_wave_clock_slot(b, slot, out, n);
}

// Diagnostics (not part of abnn.h): the last k_apply's per-workgroup timeline,
// 8 u64 per workgroup (see k_apply), 100 MHz ticks.
abnn_status abnn_debug_apply_clock(abnn_brain* b, uint64_t* out, uint64_t n)
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, b->d.apply_clock, std::min<uint64_t>(n, 8ull * kWalkBlocks) * 8, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): the recent-spike bitmap of the last pass
// (n_bitmap_words u32; bit i = neuron i was recent at that pass's start) and
// whether k_apply built the next pass's (no k_bitmap launch).
abnn_status abnn_debug_bitmap(abnn_brain* b, uint32_t* out, uint64_t n, int* incremental_next)
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, b->d.bitmap, std::min<uint64_t>(n, b->d.n_bitmap_words) * 4, hipMemcpyDeviceToHost));
    if (incremental_next) *incremental_next = b->next_built ? 1 : 0;
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): the current sweep partition, n_ranges + 1
// iteration bounds.
abnn_status abnn_debug_range_bounds(abnn_brain* b, uint32_t* out, uint64_t n)
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, b->d.range_bounds, std::min<uint64_t>(n, b->d.n_ranges + 1ull) * 4, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

// Diagnostics (not part of abnn.h): the stream's pinned slice in use, in
// sixteenths of the sweep (engine.h pin_k).
abnn_status abnn_debug_stream_pin(abnn_brain* b, uint32_t* pin_k)
{
    REQUIRE(b && pin_k, "null argument");
    *pin_k = b->d.pin_k;
    return ABNN_OK;
}

// The indexed pass (index.h).  out: {index built, its entries, its largest
// degree, the last pass was indexed, indexed passes so far, consecutive
// eligible passes, ABNN_INDEXED, E}; *build_ms: the last build.
abnn_status abnn_debug_index_state(abnn_brain* b, uint64_t out[ABNN_DEBUG_INDEX_WORDS], double* build_ms)
{
    REQUIRE(b && out, "null argument");
    const IndexState& x = b->ix;
    out[0] = x.built ? 1 : 0;
    out[1] = x.entries;
    out[2] = x.max_degree;
    out[3] = x.last_indexed ? 1 : 0;
    out[4] = x.indexed_passes;
    out[5] = x.eligible;
    out[6] = (uint64_t)x.mode;
    out[7] = b->d.events;
    if (build_ms) *build_ms = x.build_ms;
    return ABNN_OK;
}

// The event mask's words that differ from what the next indexed pass expects
// (index.h's invariant; 0 without an index): the expected mask is the current
// marked set marked by k_index_mark itself from an all-zero one into a zeroed
// scratch mask.  Synchronous.
abnn_status abnn_debug_index_mask_dirty(abnn_brain* b, uint64_t* words)
{
    REQUIRE(b && words, "null argument");
    *words = 0;
    ST_TRY(sync_all(b));
    const IndexState& x = b->ix;
    if (!x.mask) return ABNN_OK;
    const DeviceState& d = b->d;
    DeviceTemp<uint32_t> want, none, next;
    ST_TRY(want.alloc(x.mask_words));
    ST_TRY(none.alloc(d.n_bitmap_words));
    ST_TRY(next.alloc(d.n_bitmap_words, false));
    if (x.built)  // (never otherwise: the mask goes with the index)
        HIP_TRY(launch_index_mark(x.marked, none.dev, next.dev, d.n_bitmap_words, d.n_nrn, x.row, x.off, want.dev, d.events,
                                  x.heavy, x.heavy_chunks, nullptr, nullptr, b->stream));
    HIP_TRY(launch_index_dirty(x.mask, want.dev, x.mask_words, reinterpret_cast<unsigned long long*>(b->u64_scratch), b->stream));
    return read_words(b, b->u64_scratch, words, 1);
}

// The event mask's first n_words words (all of it, padding included, when
// n_words is at least its length; what lies past it in the caller's buffer
// stays) and likewise the marked set's first n_marked_words, as
// abnn_debug_bitmap.  Synchronous; an error without an index.
abnn_status abnn_debug_index_mask_copy(abnn_brain* b, uint32_t* mask_words_out, uint64_t n_words, uint32_t* marked_out,
                                       uint64_t n_marked_words)
{
    REQUIRE(b && (mask_words_out || n_words == 0) && (marked_out || n_marked_words == 0), "null argument");
    ST_TRY(sync_all(b));
    REQUIRE(b->ix.built, "abnn_debug_index_mask_copy: no index is built");
    n_words = std::min<uint64_t>(n_words, b->ix.mask_words);
    n_marked_words = std::min<uint64_t>(n_marked_words, b->d.n_bitmap_words);
    if (n_words) HIP_TRY(hipMemcpy(mask_words_out, b->ix.mask, n_words * 4, hipMemcpyDeviceToHost));
    if (n_marked_words) HIP_TRY(hipMemcpy(marked_out, b->ix.marked, n_marked_words * 4, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

// The last mark launch's {neurons entered, neurons left, entries set, entries
// cleared} (zeros without an index or before its first indexed pass).  Synchronous.
abnn_status abnn_debug_index_delta(abnn_brain* b, uint64_t out[4])
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    std::vector<uint32_t> v(4 * kDeltaSlots, 0u);
    if (b->ix.delta) HIP_TRY(hipMemcpy(v.data(), b->ix.delta + b->ix.delta_at, v.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = 0;
    for (size_t i = 0; i < v.size(); ++i) out[i & 3] += v[i];
    return ABNN_OK;
}

// ABNN_INDEXED for this handle from now on (0 never, 1 the rule, 2 whenever the index is valid).
abnn_status abnn_debug_set_indexed(abnn_brain* b, int mode)
{
    REQUIRE(b && mode >= 0 && mode <= 2, "abnn_debug_set_indexed: mode must be 0, 1 or 2");
    b->ix.mode = mode;
    return ABNN_OK;
}

// ABNN_FUSED for this handle's following single-GPU passes: 1 the fused launch where the shape has one, 0 gate + apply.
abnn_status abnn_debug_set_fused(abnn_brain* b, int on)
{
    REQUIRE(b, "null argument");
    REQUIRE(!b->pending_walk, "abnn_debug_set_fused: a sharded pass is half done (abnn_shard_apply)");
    b->use_fused = on != 0;
    return ABNN_OK;
}

// row[0, n_row) and off[0, n_off) of a built index (n_row <= N_NRN + 1, n_off <= entries).  Synchronous.
abnn_status abnn_debug_index_copy(abnn_brain* b, uint32_t* row, uint64_t n_row, uint32_t* off, uint64_t n_off)
{
    REQUIRE(b && (row || n_row == 0) && (off || n_off == 0), "null argument");
    ST_TRY(sync_all(b));
    REQUIRE(b->ix.built, "abnn_debug_index_copy: no index is built");
    REQUIRE(n_row <= b->n_nrn + 1 && n_off <= b->ix.entries, "abnn_debug_index_copy: range out of bounds");
    if (n_row) HIP_TRY(hipMemcpy(row, b->ix.row, n_row * 4, hipMemcpyDeviceToHost));
    if (n_off) HIP_TRY(hipMemcpy(off, b->ix.off, n_off * 4, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

// ... and the device allocations of pool.h that are live in this process.
uint64_t abnn_debug_live_allocations(void) { return g_live_allocations.load(std::memory_order_relaxed); }

abnn_status abnn_get_stats(abnn_brain* b, abnn_stats* out)
{
    REQUIRE(b && out, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemcpy(out, &b->d.work->stats, sizeof(abnn_stats), hipMemcpyDeviceToHost));
    std::vector<abnn_stats> wg(kWalkBlocks);
    HIP_TRY(hipMemcpy(wg.data(), b->d.wg_stats, kWalkBlocks * sizeof(abnn_stats), hipMemcpyDeviceToHost));
    for (const abnn_stats& x : wg) {
        out->passes += x.passes;
        out->events += x.events;
        out->pre_gated += x.pre_gated;
        out->post_gated += x.post_gated;
        out->updated += x.updated;
        out->fired += x.fired;
        out->pruned += x.pruned;
        out->grown += x.grown;
    }
    return ABNN_OK;
}

abnn_status abnn_reset_stats(abnn_brain* b)
{
    REQUIRE(b, "null argument");
    ST_TRY(sync_all(b));
    HIP_TRY(hipMemset(&b->d.work->stats, 0, sizeof(abnn_stats)));
    HIP_TRY(hipMemset(b->d.wg_stats, 0, kWalkBlocks * sizeof(abnn_stats)));
    return ABNN_OK;
}

abnn_status abnn_enable_timing(abnn_brain* b, int every)
{
    REQUIRE(b && every >= 0, "bad argument");
    ST_TRY(sync_all(b));
    b->timing = every;
    b->timing_count = 0;
    b->events_used = 0;
    return ABNN_OK;
}

abnn_status abnn_get_kernel_time(abnn_brain* b, double* ms_total, uint64_t* launches)
{
    REQUIRE(b && ms_total && launches, "null argument");
    ST_TRY(sync_all(b));
    double tot = 0;
    for (size_t i = 0; i < b->events_used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, b->events[i].a, b->events[i].b));
        tot += ms;
    }
    *ms_total = tot;
    *launches = b->events_used;
    b->events_used = 0;
    return ABNN_OK;
}

abnn_status abnn_get_kernel_times(abnn_brain* b, float* out_ms, uint64_t cap, uint64_t* launches)
{
    REQUIRE(b && launches && (out_ms || cap == 0), "null argument");
    ST_TRY(sync_all(b));
    for (size_t i = 0; i < b->events_used && i < cap; ++i)
        HIP_TRY(hipEventElapsedTime(&out_ms[i], b->events[i].a, b->events[i].b));
    *launches = b->events_used;
    b->events_used = 0;
    return ABNN_OK;
}

// ---- persistence -----------------------------------------------------------

abnn_status abnn_save_bnn(abnn_brain* b, const char* path)
{
    REQUIRE(b && path, "null argument");
    REQUIRE(b->dims.n_syn <= 0xFFFFFFFFull && b->n_nrn <= 0xFFFFFFFFull,
            ".bnn header holds u32 sizes (brain.cpp:163-164)");
    ST_TRY(sync_all(b));
    FILE* f = std::fopen(path, "wb");
    if (!f) {
        set_err(std::string("cannot open ") + path);
        return ABNN_ERR_IO;
    }
    const uint32_t hdr[2] = {(uint32_t)b->dims.n_syn, (uint32_t)b->n_nrn};  // brain.cpp:163-164
    bool ok = std::fwrite(hdr, 4, 2, f) == 2;
    std::vector<abnn_synapse> buf;
    for (uint64_t i = 0; ok && i < b->dims.n_syn; i += kIoRecs) {
        const uint64_t n = std::min<uint64_t>(kIoRecs, b->dims.n_syn - i);
        buf.resize(n);
        if (records_d2h(b->d.syn, i, n, buf.data()) != ABNN_OK) {
            std::fclose(f);
            return ABNN_ERR_HIP;
        }
        ok = std::fwrite(buf.data(), 16, n, f) == n;  // brain.cpp:165-166
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) {
        set_err(std::string("write failed: ") + path);
        return ABNN_ERR_IO;
    }
    return ABNN_OK;
}

abnn_status abnn_load_bnn(abnn_brain* b, const char* path)
{
    REQUIRE(b && path, "null argument");
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        set_err(std::string("cannot open ") + path);
        return ABNN_ERR_IO;
    }
    uint32_t hdr[2] = {0, 0};
    if (std::fread(hdr, 4, 2, f) != 2) {
        std::fclose(f);
        set_err("short .bnn header");
        return ABNN_ERR_IO;
    }
    if (!(hdr[0] == b->dims.n_syn && hdr[1] == b->n_nrn)) {  // brain.cpp:174
        std::fclose(f);
        set_err(".bnn header does not match this brain");
        return ABNN_ERR_SIZE_MISMATCH;
    }
    abnn_status st = sync_all(b);
    if (st != ABNN_OK) {
        std::fclose(f);
        return st;
    }
    std::vector<abnn_synapse> buf;
    for (uint64_t i = 0; i < b->dims.n_syn; i += kIoRecs) {
        const uint64_t n = std::min<uint64_t>(kIoRecs, b->dims.n_syn - i);
        buf.resize(n);
        if (std::fread(buf.data(), 16, n, f) != n) {
            std::fclose(f);
            set_err("short .bnn body");
            return ABNN_ERR_IO;
        }
        st = validate_records(b, buf.data(), n);
        if (st == ABNN_OK) st = records_h2d(b->d.syn, i, n, buf.data());
        if (st != ABNN_OK) {
            std::fclose(f);
            return st;
        }
    }
    std::fclose(f);
    b->records_invalid = false;
    return retally(b, 0, b->dims.n_syn);
}

abnn_status abnn_save_flat(abnn_brain* b, const char* path)
{
    REQUIRE(b && path, "null argument");
    REQUIRE(b->dims.n_syn <= 0xFFFFFFFFull && b->n_nrn <= 0xFFFFFFFFull,
            "flat header holds u32 sizes (README §2.1)");
    ST_TRY(sync_all(b));
    FILE* f = std::fopen(path, "wb");
    if (!f) {
        set_err(std::string("cannot open ") + path);
        return ABNN_ERR_IO;
    }
    uint32_t hdr[4] = {(uint32_t)b->dims.n_syn, (uint32_t)b->n_nrn, 0, 0};
    bool ok = std::fwrite(hdr, 4, 4, f) == 4;
    std::vector<abnn_synapse> buf;
    std::vector<uint32_t> pairs;
    std::vector<float> ws;
    // synapses (src, dst) pairs, then weights: two sweeps
    for (int sweep = 0; ok && sweep < 2; ++sweep) {
        for (uint64_t i = 0; ok && i < b->dims.n_syn; i += kIoRecs) {
            const uint64_t n = std::min<uint64_t>(kIoRecs, b->dims.n_syn - i);
            buf.resize(n);
            if (records_d2h(b->d.syn, i, n, buf.data()) != ABNN_OK) {
                ok = false;
                break;
            }
            if (sweep == 0) {
                pairs.resize(2 * n);
                for (uint64_t k = 0; k < n; ++k) {
                    pairs[2 * k] = buf[k].src;
                    pairs[2 * k + 1] = buf[k].dst;
                }
                ok = std::fwrite(pairs.data(), 8, n, f) == n;
            } else {
                ws.resize(n);
                for (uint64_t k = 0; k < n; ++k) ws[k] = buf[k].w;
                ok = std::fwrite(ws.data(), 4, n, f) == n;
            }
        }
    }
    std::vector<uint64_t> ts(b->n_nrn);
    for (int arr = 0; ok && arr < 2; ++arr) {
        uint64_t* src = arr == 0 ? b->d.last_fired : b->d.last_visited;
        if (b->n_nrn && hipMemcpy(ts.data(), src, b->n_nrn * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            ok = false;
            break;
        }
        ok = std::fwrite(ts.data(), 8, b->n_nrn, f) == b->n_nrn;
    }
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) {
        set_err(std::string("flat save failed: ") + path);
        return ABNN_ERR_IO;
    }
    return ABNN_OK;
}

abnn_status abnn_load_flat(abnn_brain* b, const char* path)
{
    REQUIRE(b && path, "null argument");
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        set_err(std::string("cannot open ") + path);
        return ABNN_ERR_IO;
    }
    uint32_t hdr[4] = {0, 0, 0, 0};
    if (std::fread(hdr, 4, 4, f) != 4) {
        std::fclose(f);
        set_err("short flat header");
        return ABNN_ERR_IO;
    }
    if (!(hdr[0] == b->dims.n_syn && hdr[1] == b->n_nrn)) {
        std::fclose(f);
        set_err("flat header does not match this brain");
        return ABNN_ERR_SIZE_MISMATCH;
    }
    abnn_status st = sync_all(b);
    if (st != ABNN_OK) {
        std::fclose(f);
        return st;
    }
    const uint64_t N = b->dims.n_syn;
    const long pairs_at = 16, weights_at = 16 + (long)(8 * N);
    std::vector<abnn_synapse> buf;
    std::vector<uint32_t> pairs;
    std::vector<float> ws;
    bool ok = true;
    for (uint64_t i = 0; ok && i < N; i += kIoRecs) {
        const uint64_t n = std::min<uint64_t>(kIoRecs, N - i);
        pairs.resize(2 * n);
        ws.resize(n);
        buf.resize(n);
        ok = std::fseek(f, pairs_at + (long)(8 * i), SEEK_SET) == 0 &&
             std::fread(pairs.data(), 8, n, f) == n &&
             std::fseek(f, weights_at + (long)(4 * i), SEEK_SET) == 0 &&
             std::fread(ws.data(), 4, n, f) == n;
        if (!ok) break;
        for (uint64_t k = 0; k < n; ++k) buf[k] = {pairs[2 * k], pairs[2 * k + 1], ws[k], 0.0f};
        st = validate_records(b, buf.data(), n);
        if (st != ABNN_OK) {
            std::fclose(f);
            return st;
        }
        ok = records_h2d(b->d.syn, i, n, buf.data()) == ABNN_OK;
    }
    std::vector<uint64_t> ts(b->n_nrn);
    if (ok) ok = std::fseek(f, weights_at + (long)(4 * N), SEEK_SET) == 0;
    for (int arr = 0; ok && arr < 2; ++arr) {
        ok = std::fread(ts.data(), 8, b->n_nrn, f) == b->n_nrn;
        uint64_t* dst = arr == 0 ? b->d.last_fired : b->d.last_visited;
        if (ok && b->n_nrn)
            ok = hipMemcpy(dst, ts.data(), b->n_nrn * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (ok && arr == 0) state_written(b, b->n_nrn ? *std::max_element(ts.begin(), ts.end()) : 0);
    }
    std::fclose(f);
    if (!ok) {
        set_err(std::string("flat load failed: ") + path);
        return ABNN_ERR_IO;
    }
    b->records_invalid = false;
    if (b->d.visit_mark) {  // lastVisited replaced on every shard (replicated state)
        HIP_TRY(hipMemset(b->d.visit_mark, 0, b->n_nrn));
        b->marks_dirty = false;
    }
    return retally(b, 0, N);
}

/* ---- device-resident learning loop (learn.hip) ------------- */

// The driver's state lives on the device (LearnState); the host keeps what it
// needs to enqueue without reading it back: the two RNG states (counter-based
// draws: a pass's draws are a function of the state before it), the steps
// enqueued, and two frame buffers (pinned staging + device) used alternately,
// each guarded by an event recorded after the last launch of the call that
// read it -- so a call never waits for the call just before it.
struct abnn_engine {
    abnn_brain* b = nullptr;
    abnn_engine_config cfg{};
    DevicePool pool;  // owns st's buffers, frames_dev and census_ring
    LearnState st{};
    float* frames_dev[2] = {};
    float* frames_host[2] = {};
    hipEvent_t done[2] = {};
    bool used[2] = {};
    uint32_t parity = 0;
    uint64_t teacher_rng = 0;
    uint64_t step_host = 0;  // steps enqueued so far
    // the census hook (abnn_engine_set_census): a device ring of census_cap
    // results of census_words u64 each; snapshot k is at slot k % census_cap
    // and census_steps[k % census_cap] is the step count it was enqueued at
    bool census_on = false;
    abnn_census_config census_cfg{};
    float census_scale = 0.0f;
    uint32_t census_every = 0, census_cap = 0;
    uint64_t census_words = 0, census_taken = 0;
    uint64_t* census_ring = nullptr;
    std::vector<uint64_t> census_steps;

    ~abnn_engine()  // on the brain's device; the pool frees the device buffers
    {
        for (int k = 0; k < 2; ++k) {
            if (frames_host[k]) (void)hipHostFree(frames_host[k]);
            if (done[k]) (void)hipEventDestroy(done[k]);
        }
    }
};

namespace {

constexpr uint64_t kSplitMixGamma = 0x9E3779B97F4A7C15ull;

abnn_status engine_alloc(abnn_engine* e)
{
    LearnState& st = e->st;
    const uint64_t no = st.n_out, tp = st.trace_passes;
    const uint64_t frame_floats = tp * ((uint64_t)st.n_in + no);
    ST_TRY(e->pool.alloc_all(
        {zeroed(&st.sc, 1), zeroed(&st.rate, no), zeroed(&st.filt, no), zeroed(&st.smooth, no),
         zeroed(&st.fir, st.use_fir ? (uint64_t)st.fir_size * no : 0), zeroed(&st.spike_window, no),
         zeroed(&st.trace_out, tp * no), zeroed(&st.trace_smooth, tp * no),
         zeroed(&e->frames_dev[0], frame_floats), zeroed(&e->frames_dev[1], frame_floats)}));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->frames_host[k]), std::max<uint64_t>(frame_floats, 1) * 4,
                              hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&e->done[k], hipEventDisableTiming));
    }
    LearnScalars sc{};
    sc.last_loss = e->cfg.last_loss;
    sc.max_observed = e->cfg.max_observed;
    HIP_TRY(hipMemcpy(st.sc, &sc, sizeof(sc), hipMemcpyHostToDevice));
    return ABNN_OK;
}

}  // namespace

void abnn_default_engine_config(abnn_engine_config* c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->input_rate_hz = 1000.0f;  // INPUT_RATE_HZ, constants.h:9
    c->peak_decay = 0.999f;      // PEAK_DECAY, constants.h:10
    c->rate_alpha = 0.5f;        // ENG:146
    c->max_observed = 0.5f;      // brain-engine.h:54
    c->filter_tau = 0.02;        // FILTER_TAU, constants.h:12
    c->dt_sec = 0.0009;          // dT_SEC, constants.h:14
    c->last_loss = 0.25;         // brain-engine.h:83
    c->use_fir = 1u;             // USE_FIR, constants.h:13
    c->fir_size = 20u;           // rate-filter.h:14
    c->win_size = 1000u;         // WIN_SIZE_, brain-engine.h:81
    c->trace_passes = 4096u;
    c->teacher_seed = 1u;
}

abnn_status abnn_engine_create(abnn_brain* b, const abnn_engine_config* cfg, abnn_engine** out)
{
    REQUIRE(b && cfg && out, "null argument");
    *out = nullptr;
    REQUIRE(b->dims.global_events == 0, "abnn_engine_create: a sharded handle has no device-resident loop");
    REQUIRE(cfg->trace_passes >= 1, "abnn_engine_create: trace_passes must be at least 1");
    REQUIRE(!cfg->use_fir || cfg->fir_size >= 1, "abnn_engine_create: use_fir needs fir_size >= 1");
    HIP_TRY(hipSetDevice(b->device));
    abnn_engine* e = new (std::nothrow) abnn_engine();
    if (!e) {
        set_err("host allocation failed");
        return ABNN_ERR_OOM;
    }
    e->b = b;
    e->cfg = *cfg;
    e->teacher_rng = cfg->teacher_seed;
    LearnState& st = e->st;
    st.last_fired = b->d.last_fired;
    st.clock = b->d.clock;
    st.reward = b->d.reward;
    st.n_in = b->dims.n_input;
    st.n_out = b->dims.n_output;
    st.use_fir = cfg->use_fir ? 1u : 0u;
    st.fir_size = cfg->fir_size;
    st.win_size = cfg->win_size;
    st.trace_passes = cfg->trace_passes;
    // pTick = hz * kTickNS * NSEC_PER_SEC, all in float (brain.cpp:76), as abnn_inject_inputs
    float p_tick = cfg->input_rate_hz * (float)b->params.tick_ns;
    p_tick = p_tick * (float)1000000000ull;
    st.p_tick = p_tick;
    st.rate_alpha = cfg->rate_alpha;
    st.peak_decay = cfg->peak_decay;
    st.filt_a = cfg->dt_sec / (cfg->filter_tau + cfg->dt_sec);  // rate-filter.h:30
    const abnn_status s = engine_alloc(e);
    if (s != ABNN_OK) {
        delete e;
        return s;
    }
    *out = e;
    return ABNN_OK;
}

abnn_status abnn_engine_destroy(abnn_engine* e)
{
    REQUIRE(e, "null argument");
    (void)hipSetDevice(e->b->device);
    (void)hipDeviceSynchronize();
    delete e;
    return ABNN_OK;
}

abnn_status abnn_engine_run(abnn_engine* e, const float* in_frames, const float* expected_frames,
                            uint32_t passes, void* stream)
{
    REQUIRE(e && in_frames && expected_frames, "null argument");
    abnn_brain* b = e->b;
    REQUIRE(passes <= e->cfg.trace_passes, "abnn_engine_run: more passes than trace_passes in one call");
    REQUIRE(b->dims.global_events == 0, "abnn_engine_run: the handle became a shard");
    REQUIRE(!b->records_invalid, kRecordsInvalid);
    ST_TRY(pass_error(b));
    if (passes == 0) return ABNN_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = pick(b, stream);
    const LearnState& st = e->st;
    const uint64_t n_in = st.n_in, n_out = st.n_out;

    // this call's frames: staged in the buffer the call before the last one used
    const uint32_t k = e->parity;
    if (e->used[k]) HIP_TRY(hipEventSynchronize(e->done[k]));
    float* hin = e->frames_host[k];
    float* hex = hin + passes * n_in;
    std::memcpy(hin, in_frames, passes * n_in * 4);
    std::memcpy(hex, expected_frames, passes * n_out * 4);
    if (passes * (n_in + n_out))
        HIP_TRY(hipMemcpyAsync(e->frames_dev[k], hin, passes * (n_in + n_out) * 4, hipMemcpyHostToDevice, s));
    const float* din = e->frames_dev[k];
    const float* dex = din + passes * n_in;

    for (uint32_t p = 0; p <= passes; ++p) {
        LearnStep sp{};
        if (p > 0) sp.post_expected = dex + (uint64_t)(p - 1) * n_out;
        if (p < passes) {
            sp.pre_in = din + (uint64_t)p * n_in;
            sp.pre_expected = dex + (uint64_t)p * n_out;
            sp.inject_state = b->rng;
            sp.teacher_state = e->teacher_rng;
        }
        HIP_TRY(launch_learn_boundary(st, sp, s));
        if (e->census_on && p > 0 && e->step_host % e->census_every == 0) {
            // the boundary launch above closed step step_host: the weights after its pass
            const uint64_t slot = e->census_taken % e->census_cap;
            HIP_TRY(launch_census(b->d.syn, b->dims.n_syn, e->census_cfg, e->census_scale,
                                  e->census_ring + slot * e->census_words, (uint32_t)b->cus, s));
            e->census_steps[slot] = e->step_host;
            e->census_taken += 1;
        }
        if (p == passes) break;
        // the draws this pass consumed: the handle's stream stays the all-host driver's
        b->rng += n_in * kSplitMixGamma;
        e->teacher_rng += n_out * kSplitMixGamma;
        state_written(b, b->clock_host);  // the pre half may stamp `now`, as abnn_inject_inputs
        ST_TRY(run_pass(b, s));
        e->step_host += 1;
    }
    HIP_TRY(hipEventRecord(e->done[k], s));
    e->used[k] = true;
    e->parity ^= 1u;
    return ABNN_OK;
}

abnn_status abnn_engine_get_state(abnn_engine* e, abnn_engine_state* out)
{
    REQUIRE(e && out, "null argument");
    ST_TRY(sync_all(e->b));
    LearnScalars sc{};
    HIP_TRY(hipMemcpy(&sc, e->st.sc, sizeof(sc), hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof(*out));
    out->step = sc.step;
    out->windows = sc.windows;
    out->win_pos = sc.win_pos;
    out->teach = sc.teach;
    out->max_observed = sc.max_observed;
    out->last_reward = sc.last_reward;
    out->last_loss = sc.last_loss;
    return ABNN_OK;
}

abnn_status abnn_engine_get_rates(abnn_engine* e, float* rate, float* smooth, uint32_t* spike_window,
                                  uint32_t n_output)
{
    REQUIRE(e, "null argument");
    REQUIRE(n_output == e->st.n_out, "abnn_engine_get_rates: size must equal n_output");
    ST_TRY(sync_all(e->b));
    const size_t bytes = (size_t)n_output * 4;
    if (rate && bytes) HIP_TRY(hipMemcpy(rate, e->st.rate, bytes, hipMemcpyDeviceToHost));
    if (smooth && bytes) HIP_TRY(hipMemcpy(smooth, e->st.smooth, bytes, hipMemcpyDeviceToHost));
    if (spike_window && bytes) HIP_TRY(hipMemcpy(spike_window, e->st.spike_window, bytes, hipMemcpyDeviceToHost));
    return ABNN_OK;
}

abnn_status abnn_engine_read_trace(abnn_engine* e, uint64_t first_step, uint32_t n, uint8_t* out, float* smooth)
{
    REQUIRE(e, "null argument");
    const uint64_t have = e->step_host, cap = e->st.trace_passes, no = e->st.n_out;
    REQUIRE(first_step <= have && n <= have - first_step, "abnn_engine_read_trace: a step that has not run");
    REQUIRE(have - first_step <= cap, "abnn_engine_read_trace: a step no longer held (trace_passes)");
    ST_TRY(sync_all(e->b));
    // the ring: step s is at slot s % trace_passes, so the range is at most two pieces
    for (uint64_t done = 0; done < n && no;) {
        const uint64_t slot = (first_step + done) % cap, run = std::min<uint64_t>(n - done, cap - slot);
        if (out)
            HIP_TRY(hipMemcpy(out + done * no, e->st.trace_out + slot * no, run * no, hipMemcpyDeviceToHost));
        if (smooth)
            HIP_TRY(hipMemcpy(smooth + done * no, e->st.trace_smooth + slot * no, run * no * 4,
                              hipMemcpyDeviceToHost));
        done += run;
    }
    return ABNN_OK;
}

abnn_status abnn_engine_set_census(abnn_engine* e, const abnn_census_config* cfg, uint32_t every, uint32_t capacity)
{
    REQUIRE(e, "null argument");
    float scale = 0.0f;
    if (cfg) {
        ST_TRY(census_check(e->b, cfg, &scale));
        REQUIRE(every >= 1 && capacity >= 1, "abnn_engine_set_census: every and capacity must be at least 1");
    }
    ST_TRY(sync_all(e->b));  // censuses already enqueued write the ring
    e->pool.release(&e->census_ring);
    e->census_on = false;
    e->census_taken = 0;
    e->census_steps.clear();
    if (!cfg) return ABNN_OK;
    const uint64_t words = abnn_census_words(cfg);
    ST_TRY(e->pool.alloc(zeroed(&e->census_ring, words * capacity)));
    e->census_steps.assign(capacity, 0);
    e->census_cfg = *cfg;
    e->census_scale = scale;
    e->census_every = every;
    e->census_cap = capacity;
    e->census_words = words;
    e->census_on = true;
    return ABNN_OK;
}

uint64_t abnn_engine_census_count(const abnn_engine* e) { return e ? e->census_taken : 0; }

abnn_status abnn_engine_read_census(abnn_engine* e, uint64_t first, uint32_t n, uint64_t* out, uint64_t* steps)
{
    REQUIRE(e, "null argument");
    REQUIRE(e->census_on, "abnn_engine_read_census: no census is set");
    const uint64_t have = e->census_taken, cap = e->census_cap, words = e->census_words;
    REQUIRE(first <= have && n <= have - first, "abnn_engine_read_census: a snapshot that has not been taken");
    REQUIRE(n == 0 || have - first <= cap, "abnn_engine_read_census: a snapshot no longer held (capacity)");
    ST_TRY(sync_all(e->b));
    // the ring: snapshot k is at slot k % capacity, so the range is at most two pieces
    for (uint64_t done = 0; done < n;) {
        const uint64_t slot = (first + done) % cap, run = std::min<uint64_t>(n - done, cap - slot);
        if (out)
            HIP_TRY(hipMemcpy(out + done * words, e->census_ring + slot * words, run * words * sizeof(uint64_t),
                              hipMemcpyDeviceToHost));
        if (steps) std::copy_n(e->census_steps.begin() + slot, run, steps + done);
        done += run;
    }
    return ABNN_OK;
}

}  // extern "C"
