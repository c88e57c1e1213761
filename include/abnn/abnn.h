/*
 * abnn.h -- C-ABI of the MI355X-native Monte-Carlo synapse traversal engine.
 *
 * This is the drop-in boundary for the reference's hot path:
 *   - the host class `Brain`            (abnn/src/core/brain/brain.h:24-83,
 *                                        abnn/src/core/brain/brain.cpp:21-178)
 *   - the kernel buffer-index ABI of    `monte_carlo_traversal`
 *                                       (abnn/src/core/kernels/brain.metal:41-58)
 *     and `renormalise_clock_and_times` (brain.metal:135-145)
 * Paths are relative to the reference root.  Every entry point below names the
 * reference interface it replaces.
 *
 * Rules of the boundary:
 *   - plain C types only (no torch, no HIP types: streams are `void*` that hold
 *     a hipStream_t, NULL = the default stream).  Pass functions
 *     (abnn_traverse, abnn_shard_*) only enqueue on that stream; every other
 *     function is synchronous and first waits for all work on the device;
 *   - every function returns an abnn_status; no exception crosses the ABI
 *     (the reference threw a *pointer* `new std::exception()` from Brain::load,
 *     brain.cpp:174 -- here that case is ABNN_ERR_SIZE_MISMATCH);
 *   - device pointers returned by abnn_state_ptrs are BORROWED (the handle
 *     owns them), exactly like the unretained MTL::Buffer getters of
 *     brain.h:54-58;
 *   - a handle is not thread-safe: the caller serialises (the reference drove
 *     one Brain from one worker thread, brain-engine.cpp:193-201).
 *
 * Semantics: every pass executes the deterministic legal schedule "C1" of the
 * reference kernel: events in increasing tid order, an
 * ordered global spike budget, all reads of lastFired/clock/rBar observe the
 * pass-start values, stores become visible at pass end.  Timestamps are
 * stored as u64 (README lastFiredNS) and every decision on them is the
 * reference's u32 arithmetic on their low 32 bits (brain.metal:43-45 declare
 * them `uint`): ages `now - ts` wrap at 2^32 (brain.metal:74,80,116),
 * read_outputs and the renormalisation test compare u32 values
 * (brain.cpp:127-128,149-154).
 */
#ifndef ABNN_ABNN_H
#define ABNN_ABNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ABNN_ABI_VERSION 10

typedef enum abnn_status {
    ABNN_OK = 0,
    ABNN_ERR_INVALID = 1,        /* bad argument / shape                          */
    ABNN_ERR_HIP = 2,            /* a HIP runtime call failed (see abnn_last_error) */
    ABNN_ERR_OOM = 3,            /* device or host allocation failed              */
    ABNN_ERR_SIZE_MISMATCH = 4,  /* .bnn header does not match (brain.cpp:174)    */
    ABNN_ERR_IO = 5,             /* file open/read/write failed                   */
    ABNN_ERR_NO_DEVICE = 6       /* no HIP device / bad ordinal                   */
} abnn_status;

/* SynapsePacked -- brain.metal:11, brain.h:21, README §2.2.  16 bytes, AoS.
 * This is the INTERCHANGE format (upload/download, .bnn, the C++ wrapper).
 * On the device the records are held as arrays (abnn_state):
 * the sweep's gate needs only `src`, held in 24 bits, so it streams 3 B per
 * event instead of 16.  `pad` is not stored; downloads return 0 (the
 * reference never writes or reads it: brain.metal:11, brain-engine.cpp:31-53).
 * N_NRN = n_input + n_output + n_hidden must be below 2^24 - 1 (16,777,215;
 * the reference's configurations reach 5,000,512): abnn_brain_create returns
 * ABNN_ERR_INVALID above. */
typedef struct abnn_synapse {
    uint32_t src;
    uint32_t dst;
    float w;
    float pad; /* always 0, never read (brain.metal:11) */
} abnn_synapse;

/* Sizes fixed at construction: Brain(nInput, nOutput, nHidden, nSynapses,
 * eventsPerPass), brain.h:27-31.  N_NRN = n_input + n_output + n_hidden
 * (brain.cpp:24).  64-bit where the reference used uint32_t (4B synapses). */
typedef struct abnn_dims {
    uint32_t n_input;            /* 256 (constants.h:2)                         */
    uint32_t n_output;           /* 256 (constants.h:3)                         */
    uint64_t n_hidden;           /* 5'000'000 (constants.h:4)                   */
    uint64_t n_syn;              /* synapses held by THIS handle (its shard)    */
    uint64_t events_per_pass;    /* EVENTS_PER_PASS (constants.h:11); visited
                                    events per pass are
                                    min(roundup(events,256), n_syn) (brain.cpp:117,
                                    brain.metal:61) in sweep mode and exactly
                                    events_per_pass in random mode              */
    uint64_t syn_offset;         /* global id of local synapse 0 (sharding; 0)   */
    uint64_t global_events;      /* sum over shards of visited events per pass;
                                    0 = this handle alone (used for the clock
                                    tick rule, brain.metal:61,129)             */
    uint64_t syn_capacity;       /* records this handle may grow to by
                                    synaptogenesis; 0 = n_syn (no growth)     */
} abnn_dims;

/* Every knob of the path with the reference default (abnn_default_params). */
typedef struct abnn_params {
    float base_scale;        /* 0.8f    BASE_SCALE      brain.metal:22 */
    uint32_t refractory;     /* 2       REFRACTORY      brain.metal:23 */
    uint32_t window_pre;     /* 5       WINDOW_PRE      brain.metal:24 */
    uint32_t clock_inc;      /* 1       CLOCK_INC       brain.metal:26 */
    float target_rate_hz;    /* 1000    TARGET_RATE_HZ  brain.metal:28 */
    float eta_home;          /* 1e-6    ETA_HOME        brain.metal:29 */
    float eta_reward;        /* 1e-3    ETA_REWARD      brain.metal:30 */
    float alpha_rbar;        /* 1e-3    ALPHA_RBAR      brain.metal:31 */
    float a_ltp;             /* 0.04f   _aLTP           constants.h:16 */
    float a_ltd;             /* 0.02f   _aLTD           constants.h:17 */
    float w_min;             /* 0.001f  _wMin           constants.h:18 */
    float w_max;             /* 1.0f    _wMax           constants.h:19 */
    uint32_t max_spikes;     /* 2560    kMaxSpikes      brain.h:18     */
    uint32_t tick_ns;        /* 1000    kTickNS         brain.h:17     */
    uint32_t tau_vis;        /* 50000   brain.cpp:102 (bound, unused: brain.metal:47) */
    uint32_t tau_pre;        /* 50000   brain.cpp:102 (bound, unused: brain.metal:48) */
    uint64_t renorm_thresh;  /* 4000000 kRenormThresh   brain.h:19     */
    uint32_t track_visits;   /* 0: lastVisited untouched (reference code,
                                brain.metal:44); 1: lastVisited[dst] = now for
                                every visited event (README §4)        */
    uint32_t mode;           /* ABNN_MODE_SWEEP (the reference code: event t
                                visits synapse t) or ABNN_MODE_RANDOM (README
                                §4, SURVEY §8(a) A14: event t visits a uniform
                                random synapse, below)                 */
    uint64_t seed;           /* seed of the handle's host RNG (inject_inputs)
                                and of the random-mode picks           */
    /* structural plasticity (README §5; build-defined, below) */
    float w_prune;           /* 0: off; updated weight < w_prune removes the synapse */
    float p_new;             /* 0: off; probability that a spike grows a synapse     */
    float w_init;            /* weight of a grown synapse                            */
    uint32_t compact_every;  /* structural update after every N-th pass; 0 = never   */
} abnn_params;

/* Structural plasticity (README §5 "Plasticity & Rewiring"; no reference code,
 * so the build defines it; the CPU oracle restates it):
 *   pruning: an event that reached the weight update and whose stored weight
 *     (random mode: the winning store) is < w_prune removes its synapse: the
 *     record becomes the tombstone {src = dst = 0xFFFFFFFF, w, 0}, which never
 *     passes the pre-spike gate but still counts as a visited event;
 *   synaptogenesis: the spike in global budget slot k of pass p grows a
 *     synapse iff unit24(x) < p_new, x = splitmix64_at(seed ^ ABNN_GENESIS_KEY,
 *     (p << 32) | k) (the generator's SplitMix64, unit24 = top 24 bits / 2^24):
 *     record {src of the firing synapse, n_input + ((x & 0xFFFFFFFF) *
 *     (N_NRN - n_input) >> 32), w_init, 0};
 *   structural update, after every pass whose ticked pass_index is a multiple
 *     of compact_every: the D tombstones are removed -- the array ends at
 *     m = n_syn - D, and the tombstones below m, in index order, take the
 *     live records of the tail [m, n_syn), in index order (only the filled
 *     holes' records move: O(D); ABI 10 -- until ABI 9 the tombstones' span
 *     closed up in order, O(span)); then the synapses grown since the
 *     previous update are appended in (pass, slot) order while n_syn <
 *     syn_capacity.  n_syn and
 *     the visited events change here; the records are compacted in place (no
 *     second buffer), so the borrowed synapse pointer (abnn_state_ptrs) stays
 *     valid.  Sweep-mode event ids stay syn_offset + local index (syn_offset
 *     is fixed). */
#define ABNN_GENESIS_KEY 0xA24BAED4963EE407ull

/* Random-edge mode (README §4 "pick a random synapse"; no reference code, so
 * the build defines it):
 *   E = events_per_pass events per pass; event t (local index) visits record
 *   e(t) = mulhi64(x, n_syn), x = (out[1] << 32) | out[0] of
 *   Philox4x32-10(counter = {t_lo, t_hi, pass_lo, pass_hi},
 *                 key = {seed_lo ^ off_lo, seed_hi ^ off_hi}),
 *   pass = abnn_scalars.pass_index, off = abnn_dims.syn_offset (a shard picks
 *   within its own records, with its own stream).
 *   Gates, budget, candidate test (rand01((u32)(syn_offset + t) ^ now)) and
 *   stamps follow schedule C1 with t as the event id.  Every event reads the
 *   pass-start record; when several events that reached the update picked
 *   the same synapse, the weight stored is the one computed by the highest
 *   event index (a legal serialisation of the racy kernel: all reads before
 *   all writes, writes in event order).                                      */
#define ABNN_MODE_SWEEP 0u
#define ABNN_MODE_RANDOM 1u

/* Scalar state (brain.cpp:57-60): clock, reward, running-average reward,
 * plus the pass counter that keys the random-mode picks. */
typedef struct abnn_scalars {
    uint64_t clock;          /* u64 storage; decisions use its low 32 bits (the
                                reference's u32 clock, brain.cpp:57)          */
    float reward;
    float rbar;
    uint64_t pass_index;     /* passes run by this handle (+1 per pass; not
                                reset by renormalisation or reset_stats)    */
} abnn_scalars;

/* Cumulative per-handle pass statistics (for the roofline byte count). */
typedef struct abnn_stats {
    uint64_t passes;
    uint64_t events;         /* E: visited events                        */
    uint64_t pre_gated;      /* G1: passed the pre-spike gate (brain.metal:73-77) */
    uint64_t post_gated;     /* passed the refractory gate (brain.metal:79-83)   */
    uint64_t updated;        /* G2: reached the weight update (budget > 0)       */
    uint64_t fired;          /* F: spikes emitted (lastFired stamps)             */
    uint64_t pruned;         /* synapses removed (tombstoned)                    */
    uint64_t grown;          /* synapses appended by structural updates          */
} abnn_stats;

/* Borrowed device pointers (brain.h:54-58 buffer getters).  The neuron state
 * and the scalars are plain arrays (u64 timestamps, README lastFiredNS; every
 * decision takes their low 32 bits, as the reference's `uint` arithmetic,
 * brain.metal:43-45,74,80,116).  The synapse records (bufSyn_) are held in a
 * kernel-specific device layout: `synapses` is opaque.  Read and write
 * records through abnn_upload_synapses / abnn_download_synapses (the
 * SynapsePacked interchange format), or describe the layout with
 * abnn_synapse_layout (versioned separately from the ABI: a layout change
 * does not change this header).  Taking the pointers makes every later pass
 * rebuild the recent-spike bitmap from lastFired (the caller may write it
 * behind the handle's back). */
typedef struct abnn_state {
    void* synapses;          /* opaque: the device record arrays (abnn_synapse_layout) */
    uint64_t* last_fired;    /* N_NRN (bufLastFire_)                     */
    uint64_t* last_visited;  /* N_NRN (bufLastVisit_)                    */
    uint64_t* clock;         /* 1 (bufClock_)                            */
    float* reward;           /* 1 (bufReward_)                           */
    float* rbar;             /* 1 (bufRBar_)                             */
} abnn_state;

/* The device record layout behind abnn_state.synapses, for tools that must
 * address it directly (profilers, debuggers, custom kernels).  `version`
 * names the layout (DESIGN.md §4 documents each; ABNN_LAYOUT_VERSION is the
 * one this library writes); arrays[i] = {device pointer, bytes, element
 * bytes, name}.  A caller that does not know `version` must not touch them. */
#define ABNN_LAYOUT_VERSION 4
#define ABNN_LAYOUT_MAX_ARRAYS 4
typedef struct abnn_array_desc {
    void* ptr;
    uint64_t bytes;
    uint32_t elem_bytes;
    char name[20];
} abnn_array_desc;
typedef struct abnn_layout {
    uint32_t version;
    uint32_t n_arrays;
    abnn_array_desc arrays[ABNN_LAYOUT_MAX_ARRAYS];
} abnn_layout;

typedef struct abnn_brain abnn_brain;

/* ---- library ------------------------------------------------------------ */
int abnn_abi_version(void);
const char* abnn_status_string(abnn_status s);
/* Last error message of the calling thread (empty string if none). */
const char* abnn_last_error(void);
/* Reference defaults for every knob (brain.metal:22-31, constants.h:16-19,
 * brain.h:17-19, brain.cpp:102). */
void abnn_default_params(abnn_params* out);
/* Number of HIP devices visible (0 without a GPU; never fails). */
int abnn_device_count(void);

/* ---- lifetime: Brain::Brain + build_pipeline + build_buffers -------------
 * brain.cpp:21-26 (ctor), brain.cpp:38-48 (build_pipeline: kernels are
 * compiled in, nothing to build), brain.cpp:52-69 (build_buffers: allocate
 * and zero; budget = kMaxSpikes; reward = rBar = 0; clock = 0).            */
abnn_status abnn_brain_create(const abnn_dims* dims, const abnn_params* params,
                              int device, abnn_brain** out);
/* ~Brain / release_all, brain.cpp:27-34. */
abnn_status abnn_brain_destroy(abnn_brain* b);
abnn_status abnn_get_dims(const abnn_brain* b, abnn_dims* out);
abnn_status abnn_get_params(const abnn_brain* b, abnn_params* out);
abnn_status abnn_state_ptrs(abnn_brain* b, abnn_state* out);
abnn_status abnn_synapse_layout(abnn_brain* b, abnn_layout* out);
/* n_neuron() = n_input + n_output + n_hidden (brain.h:51). */
uint64_t abnn_n_neuron(const abnn_brain* b);

/* ---- synapses ------------------------------------------------------------ */
/* Host -> device copy of records [first, first+n) (the reference wrote the
 * Managed buffer directly, brain-engine.cpp:37-52). */
abnn_status abnn_upload_synapses(abnn_brain* b, uint64_t first,
                                 const abnn_synapse* src, uint64_t n);
abnn_status abnn_download_synapses(abnn_brain* b, uint64_t first,
                                   abnn_synapse* dst, uint64_t n);
/* Synthetic graph with the recipe of build_random_graph (brain-engine.cpp:31-53)
 * and this library's portable counter-based RNG: global record
 * i < n_input*n_output is the dense block {i/n_out, n_in + i%n_out,
 * w~U(0.4,0.8)}; the rest {src,dst ~ U[n_in+n_out, N_NRN-1], w~U(0.1,0.2)}.
 * Generated on the device, shard-aware (uses syn_offset).                   */
abnn_status abnn_generate_synapses(abnn_brain* b, uint64_t seed);
/* Order-sensitive 64-bit checksum of the local synapse array (device-side). */
abnn_status abnn_checksum_synapses(abnn_brain* b, uint64_t* out);

/* ---- graph builder -------------------------------------------
 * The reference's specification asks for more graphs than its code builds
 * (README §6: "Generate connectivity (Erdős–Rényi or small-world)", "Initialize
 * weights ~ Beta(2,8)").  A graph is described as up to ABNN_GRAPH_MAX_BLOCKS
 * BLOCKS laid end to end in global record order: block j holds count_j records,
 * and global record start_j + r (start_j = the sum of the earlier counts) is
 * record r of block j.  A block names a source population [src_first, src_first
 * + S), a target population [dst_first, dst_first + D), a topology and a weight
 * law.  Every record is a closed-form function of (spec.seed, j, r): the result
 * does not depend on the grid, a shard generates exactly its slice [syn_offset,
 * syn_offset + n_syn), and a block's records depend on its number and the
 * seed alone, not on the counts or contents of the blocks before it (abnn_amd/
 * graph.py restates the rule in numpy).
 * The draws.  X(c) = splitmix64_at(seed ^ (ABNN_GRAPH_KEY * (j + 1)), (r << 5)
 * | c) for c < 32, in u64 arithmetic, where
 *   splitmix64_at(s, k): z = s + (k + 1) * 0x9E3779B97F4A7C15;
 *     z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) *
 *     0x94D049BB133111EB; return z ^ z >> 31.
 *   u(c) = (float)(X(c) >> 40) * 2^-24 (unit24: 24 bits, exact, in [0, 1)).
 *   pick(c, n) = (uint32_t)(((X(c) >> 32) * n) >> 32).
 * Topologies give (src, dst):
 *   DENSE:  src = src_first + (r / D) % S,  dst = dst_first + r % D.
 *   RANDOM: src = src_first + pick(0, S),   dst = dst_first + pick(1, D).
 *   RING:   one population (src_first == dst_first, S == D == n) and 1 <= k < n.
 *           i = (r / k) % n, q = r % k, o = (q >> 1) + 1; the lattice target is
 *           t = (i + ((q & 1) ? n - o : o)) % n: i+1, i-1, i+2, i-2, ... -- k
 *           distinct neighbours, none of them i.  If u(0) < p_rewire (one fp32
 *           compare) the edge is rewired: t = (i + 1 + pick(1, n - 1)) % n,
 *           uniform over the other n - 1 nodes, never a self-loop.
 *           src = src_first + i, dst = src_first + t.
 * Weight.  w = w_lo + v * (w_hi - w_lo) as three separate fp32 operations (the
 * subtraction, the product, the addition; no fused multiply-add), with
 *   UNIFORM: v = u(2);
 *   BETA:    v = the beta_a-th smallest of u(2) ... u(2 + m - 1), m = beta_a +
 *            beta_b - 1: exactly Beta(a, b) for integer parameters, by
 *            comparisons alone (Beta(2,8): the second smallest of nine draws).
 * pad = 0.  With a count above S * D (DENSE) or n * k (RING) the pattern
 * repeats, with fresh weights.                                               */
#define ABNN_GRAPH_MAX_BLOCKS 16
#define ABNN_GRAPH_KEY 0xD1B54A32D192ED03ull
#define ABNN_TOPO_DENSE  0u   /* all-to-all, row-major                                  */
#define ABNN_TOPO_RANDOM 1u   /* src, dst uniform and independent (Erdős–Rényi G(n,M) with
                                 replacement: multi-edges and self-loops allowed, as
                                 brain-engine.cpp:46-47)                                 */
#define ABNN_TOPO_RING   2u   /* directed Watts–Strogatz: ring lattice of out-degree k,
                                 each edge rewired with probability p_rewire            */
#define ABNN_W_UNIFORM 0u
#define ABNN_W_BETA    1u     /* Beta(a, b), integer a, b: an order statistic of uniforms */
typedef struct abnn_graph_block {        /* 64 bytes */
    uint64_t count;                      /* 1 .. 2^59 - 1 */
    uint32_t src_first, src_count;       /* S = src_count >= 1 */
    uint32_t dst_first, dst_count;       /* D = dst_count >= 1 */
    uint32_t topology, k;                /* k: RING only, else 0 */
    float    p_rewire;                   /* RING only (0..1), else +0.0f */
    uint32_t weight_law;
    float    w_lo, w_hi;                 /* finite, w_lo <= w_hi */
    uint32_t beta_a, beta_b;             /* BETA only: >= 1, a + b - 1 <= 15; else 0 */
    uint32_t reserved[2];                /* 0 */
} abnn_graph_block;
typedef struct abnn_graph_spec {         /* 1040 bytes */
    uint64_t seed;
    uint32_t n_blocks, reserved;         /* 1 .. 16; 0 */
    abnn_graph_block blocks[ABNN_GRAPH_MAX_BLOCKS];   /* entries past n_blocks all zero */
} abnn_graph_spec;
/* The sum of the counts, or 0 for an invalid spec (whatever can be checked
 * without a handle): null; n_blocks outside 1..16; a reserved word that is not
 * 0 or a non-zero byte in a block past n_blocks; a count of 0 or >= 2^59; S or
 * D of 0, or first + count above 2^32; an unknown topology or weight law; k or
 * p_rewire (any bits but +0.0f) set on a block that is not RING; a RING block
 * with different populations, k == 0, k >= n, or p_rewire outside [0, 1] or
 * NaN; beta_a or beta_b set on a block that is not BETA; a BETA block with a
 * zero parameter or a + b - 1 > 15; a bound that is not finite, w_lo > w_hi.   */
uint64_t    abnn_graph_records(const abnn_graph_spec* spec);
/* The rule on the host, without a device or a handle: global records [first,
 * first + n) of the spec into out_host.  ABNN_ERR_INVALID: a null spec (or a
 * null out_host with n > 0), an invalid spec, first + n above its total.       */
abnn_status abnn_graph_fill_host(const abnn_graph_spec* spec, uint64_t first, uint64_t n, abnn_synapse* out_host);
/* Synchronous, as abnn_generate_synapses: waits for the device, fills the
 * handle's local records k < n_syn with global record syn_offset + k of the
 * spec, waits again; the records are valid afterwards and the pruning tally is
 * recounted.  The neuron state and the scalars are untouched; nothing at or
 * past n_syn is written.  ABNN_ERR_INVALID (the records stay as they were): a
 * null argument, an invalid spec, syn_offset + n_syn > abnn_graph_records(spec),
 * a population that ends above N_NRN.  n_syn == 0 is valid.                   */
abnn_status abnn_build_graph(abnn_brain* b, const abnn_graph_spec* spec);

/* ---- synapse census ----------------------------------------
 * One streaming pass over the handle's local records [0, n_syn): live and
 * tombstone counts and a histogram of the selected weights, without moving the
 * records to the host.  Records past n_syn (the capacity's headroom, the
 * padding) are never read.
 * A tombstone is a record with dst == 0xFFFFFFFF.  A record is SELECTED when
 * it is live and passes both ranges.  A selected record with weight w counts,
 * in this order: w != w -> NaN; w < lo -> under; w >= hi -> over; otherwise
 * bin min((uint32_t)((w - lo) * scale), bins - 1), scale = (float)bins /
 * (hi - lo), every operation a single IEEE fp32 operation.  hi - lo and scale
 * must be finite.  Min and max are taken over the selected non-NaN weights in
 * the total order of the sign-flip integer key (-0.0 < +0.0); with none, min
 * is +inf and max is -inf.  selected == under + over + nan + sum of the bins.
 * Every word is an integer, so the result is the same for any grid and order
 * (abnn_amd/census.py restates it in numpy).
 * Result: ABNN_CENSUS_HEADER_WORDS + bins u64 words:
 *   0 records scanned (= n_syn)   1 tombstones among them   2 selected
 *   3 under   4 over   5 NaN
 *   6 / 7 f32 bits of the minimum / maximum, in the low 32 bits
 *   8... the bins                                                            */
#define ABNN_CENSUS_MAX_BINS 4096
#define ABNN_CENSUS_HEADER_WORDS 8
typedef struct abnn_census_config {
    float lo, hi;            /* bins cover [lo, hi); finite, lo < hi                   */
    uint32_t bins;           /* 1 .. ABNN_CENSUS_MAX_BINS                              */
    uint32_t src_first, src_count;   /* count 0 = any src; else src in [first, first+count) */
    uint32_t dst_first, dst_count;   /* likewise for dst                                */
    uint32_t reserved;       /* 0 */
} abnn_census_config;         /* 32 bytes */
/* ABNN_CENSUS_HEADER_WORDS + bins, or 0 for an invalid config (whatever can be
 * checked without a handle: a range's end is checked against N_NRN below).  */
uint64_t abnn_census_words(const abnn_census_config* cfg);
/* Enqueue only: zeroes and fills out_dev (DEVICE memory, abnn_census_words(cfg)
 * u64) in stream order on `stream`; no synchronise, so it can sit between
 * passes.  A shard handle censuses its own records.  ABNN_ERR_INVALID: a null
 * argument, an invalid config, a range that ends above N_NRN, a handle whose
 * records are invalid (a failed structural update).  n_syn == 0 is valid.    */
abnn_status abnn_census_enqueue(abnn_brain* b, const abnn_census_config* cfg, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_census_words(cfg)). */
abnn_status abnn_census(abnn_brain* b, const abnn_census_config* cfg, uint64_t* out_host, uint64_t words);

/* ---- neuron degree census -----------------------------------
 * One streaming pass over the handle's local records [0, n_syn): per neuron of
 * a range R = [first, first + M) (M = count, or N_NRN when count == 0), the
 * number of live records that leave it (src == n) and that enter it (dst == n)
 * and the fixed-point sums of their weights, without moving the records to the
 * host.  A tombstone (dst == 0xFFFFFFFF) counts in no plane; records past n_syn
 * are never read.
 * Strength.  A weight is SUMMABLE iff fabsf(w) < 128.0f (false for NaN and
 * +-inf); its term is q = (int32_t)(w * 16777216.0f): one fp32 multiply (exact)
 * and a truncation toward zero (denormals give 0).  A strength plane holds the
 * two's-complement 64-bit sum of the terms modulo 2^64: strength = (int64_t)word
 * / 2^24.  A record that is not summable adds nothing to the strength plane, 1
 * to the skipped word and 1 to the degree plane.
 * Every word is an integer sum, so the result is the same for any grid and
 * order (abnn_amd/degree.py restates it in numpy).
 * Result: ABNN_DEGREE_HEADER_WORDS + P * M u64 words, P = the bits set in what:
 *   0 records scanned (= n_syn)   1 tombstones among them
 *   2 live records with src in R (0 unless OUT or OUT_W is asked)
 *   3 live records with dst in R (0 unless IN or IN_W is asked)
 *   4 records of word 2 that are not summable (0 unless OUT_W is asked)
 *   5 likewise for word 3 (0 unless IN_W is asked)          6, 7 zero
 *   8... one plane of M words per bit asked, in increasing bit order; word j
 *        of a plane belongs to neuron first + j.
 * Word 2 is the sum of the OUT plane and word 3 of the IN plane, when asked.  */
#define ABNN_DEG_OUT   1u   /* plane: live records with src == n (fan-out)            */
#define ABNN_DEG_IN    2u   /* plane: live records with dst == n (fan-in)             */
#define ABNN_DEG_OUT_W 4u   /* plane: fixed-point sum of w over records with src == n */
#define ABNN_DEG_IN_W  8u   /* plane: ... with dst == n                               */
#define ABNN_DEGREE_HEADER_WORDS 8
typedef struct abnn_degree_config {
    uint32_t first, count;   /* neurons [first, first+count); count 0 = every neuron (first must be 0) */
    uint32_t what;           /* non-empty subset of the four bits above */
    uint32_t reserved[5];    /* 0 */
} abnn_degree_config;         /* 32 bytes */
/* The result's words for a brain of n_nrn neurons, or 0 for an invalid config:
 * null, what == 0 or a bit above 15, a reserved word that is not 0, count == 0
 * with first != 0, first + count > n_nrn, n_nrn == 0.                          */
uint64_t abnn_degree_words(const abnn_degree_config* cfg, uint64_t n_nrn);
/* Enqueue only: zeroes and fills out_dev (DEVICE memory, abnn_degree_words(cfg,
 * N_NRN) u64) in stream order on `stream`; no synchronise, so it can sit
 * between passes.  A shard handle counts its own records.  ABNN_ERR_INVALID: a
 * null argument, a config that is invalid for the handle's N_NRN, a handle
 * whose records are invalid.  n_syn == 0 is valid: all-zero planes.           */
abnn_status abnn_degree_enqueue(abnn_brain* b, const abnn_degree_config* cfg, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_degree_words(cfg,
 * N_NRN)).  Its device scratch stays with the handle until abnn_brain_destroy. */
abnn_status abnn_degree(abnn_brain* b, const abnn_degree_config* cfg, uint64_t* out_host, uint64_t words);

/* ---- synapse select ------------------------------------------
 * An ordered stream compaction of the handle's local records [0, n_syn): the
 * records that MATCH, in increasing record order and with their indices, into a
 * caller-sized buffer, without moving the other records to the host.  Records
 * past n_syn are never read.
 * Matching rule (every comparison one u32 or IEEE fp32 operation; abnn_amd/
 * select.py restates it in numpy).  A tombstone (dst == 0xFFFFFFFF) never
 * matches.  S is src - src_first < src_count and D is dst - dst_first <
 * dst_count, in u32.  Without ABNN_SELECT_ANY a range that is not set (count 0)
 * is true and the range test is S && D; with it a range that is not set is
 * false and the test is S || D (ANY with neither range set is invalid).  With
 * ABNN_SELECT_WEIGHT the record must also satisfy w >= w_lo && w < w_hi: NaN
 * never matches; the bounds are not NaN, w_lo < w_hi, +-inf are allowed.
 * Result, as u64 words (abnn_select_words = 8 + 3 * capacity):
 *   0 records scanned (= n_syn)   1 tombstones among them
 *   2 matched: every matching record, whatever the capacity
 *   3 written = min(matched, capacity)   4 the handle's syn_offset   5..7 zero
 *   8 ...             the index plane: capacity u64; entry k = syn_offset +
 *                     the local index of the k-th match in index order
 *   8 + capacity ...  the record plane: capacity abnn_synapse (16 B each);
 *                     entry k is that record {src, dst, w, pad = 0}, the bits
 *                     of w unchanged
 * The first `capacity` matches in index order are written.  Plane entries at
 * and past `written` are NOT written (only the header is zeroed), so a large
 * buffer costs no memset.  capacity == 0 is a pure count (8 words).  The result
 * does not depend on the grid or on timing.                                   */
#define ABNN_SELECT_ANY     1u  /* a record matches when EITHER set range holds (neighbourhood); default: every set range holds */
#define ABNN_SELECT_WEIGHT  2u  /* also require w_lo <= w && w < w_hi */
#define ABNN_SELECT_HEADER_WORDS 8
typedef struct abnn_select_config {      /* 32 bytes */
    uint32_t src_first, src_count;       /* count 0 = range not set */
    uint32_t dst_first, dst_count;
    float    w_lo, w_hi;                 /* read only with ABNN_SELECT_WEIGHT; else both must be +0.0f */
    uint32_t flags;
    uint32_t reserved;                   /* 0 */
} abnn_select_config;
/* 8 + 3 * capacity, or 0 for an invalid config (whatever can be checked without
 * a handle): null, unknown flag bits, reserved != 0, a non-zero w_lo or w_hi
 * without WEIGHT, a NaN bound or w_lo >= w_hi with it, ANY with neither range
 * set, a range whose first + count exceeds 2^32.                               */
uint64_t    abnn_select_words(const abnn_select_config* cfg, uint64_t capacity);
/* Enqueue only: three launches in stream order on `stream` (count per tile of
 * records, prefix over the tiles, emit) that fill out_dev (DEVICE memory,
 * abnn_select_words(cfg, capacity) u64); no workgroup waits for another and
 * nothing synchronises, so it can sit between passes.  A shard handle selects
 * its own records; its indices are global through syn_offset.
 * The handle owns the select's scratch (per-tile counts and offsets, sized for
 * syn_capacity): the FIRST select call on a handle allocates it and may
 * synchronise the device; abnn_brain_destroy frees it.  Because the scratch is
 * per handle, two selects of one handle enqueued on different streams must be
 * ordered by the caller (an event, or one stream).
 * ABNN_ERR_INVALID: a null argument, an invalid config, a range that ends above
 * N_NRN, a handle whose records are invalid.  n_syn == 0 is valid.            */
abnn_status abnn_select_enqueue(abnn_brain* b, const abnn_select_config* cfg, uint64_t capacity, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_select_words(cfg,
 * capacity)); the header and only the first `written` entries of each plane are
 * copied, the rest of out_host is left untouched.                             */
abnn_status abnn_select(abnn_brain* b, const abnn_select_config* cfg, uint64_t capacity, uint64_t* out_host, uint64_t words);

/* ---- synapse edit --------------------------------------------
 * One streaming read-modify-write pass over the handle's local records [0,
 * n_syn), on the device: lesion a population, re-draw a projection's weights,
 * clamp or rescale a weight band, scale each neuron's inputs -- without moving
 * the records to the host.  Records at or past n_syn are never read or written.
 * A record MATCHES by abnn_select's rule, bit for bit (the tombstone never
 * matches; S / D are the u32 range tests; ABNN_EDIT_ANY / ABNN_EDIT_WEIGHT have
 * the values and the meaning of ABNN_SELECT_ANY / ABNN_SELECT_WEIGHT; NaN never
 * matches a weight interval).  A matched record with weight w gets the value v,
 * every operation a single IEEE fp32 operation (no fused multiply-add):
 *   ABNN_EDIT_SET        v = b
 *   ABNN_EDIT_AFFINE     t = w * a;  v = t + b
 *   ABNN_EDIT_SCALE_DST  v = w * plane[key - first], key = the record's dst
 *   ABNN_EDIT_SCALE_SRC  ... key = the record's src.  (first, M) is the dst /
 *                        src range of the config, or (0, N_NRN) when that range
 *                        is not set; plane is M f32.  A matched record whose
 *                        key lies outside the plane (no valid record has one)
 *                        is left as it is.
 *   ABNN_EDIT_DRAW       d = b - a;  t = u * d;  v = a + t  (three operations,
 *                        as abnn_graph_block's weight), u = unit24(
 *                        splitmix64_at(seed ^ ABNN_EDIT_KEY, syn_offset + the
 *                        local index)), the graph builder's functions: a shard
 *                        draws what the unsharded brain draws.
 *   ABNN_EDIT_KILL       the record becomes the pruning tombstone {src = dst =
 *                        0xFFFFFFFF, w unchanged, 0}.
 * With ABNN_EDIT_CLAMP (any op but KILL) two comparisons follow, so a NaN stays
 * a NaN:  if (v < c_lo) v = c_lo;  if (v > c_hi) v = c_hi;
 * The bits of v replace the bits of w; a v that is a NaN is stored as the quiet
 * NaN 0x7FC00000 (IEEE leaves a NaN's sign and payload to the platform; so the
 * host rule and the device agree on inf * 0 too).  A record is CHANGED when the stored
 * bits differ from the old ones (-0.0 and +0.0 differ); only changed records
 * are written.  KILL changes every record it matches.
 * Result: ABNN_EDIT_HEADER_WORDS u64 words, all integers (the result depends on
 * neither the grid nor the timing; abnn_amd/edit.py restates the rule in numpy):
 *   0 records scanned (= n_syn)   1 tombstones among them before the edit
 *   2 matched   3 changed   4 killed
 *   5 matched records whose stored v is NaN or +-inf (non-zero: the edit
 *     poisoned the traversal; KILL stores no v: 0)     6, 7 zero
 * KILL's bookkeeping is the pruning path's: the tombstone src code in the src
 * streams, the kills added to the structural update's tally (compact_every >
 * 0), n_syn unchanged -- the next structural update removes the tombstones as
 * it removes pruned ones; with compact_every == 0 they stay (a saved pruned
 * brain).  abnn_stats.pruned is a pass statistic and is not touched.         */
#define ABNN_EDIT_ANY     1u   /* = ABNN_SELECT_ANY */
#define ABNN_EDIT_WEIGHT  2u   /* = ABNN_SELECT_WEIGHT */
#define ABNN_EDIT_CLAMP   4u   /* clamp v to [c_lo, c_hi] after the op */
#define ABNN_EDIT_SET       0u
#define ABNN_EDIT_AFFINE    1u
#define ABNN_EDIT_SCALE_DST 2u
#define ABNN_EDIT_SCALE_SRC 3u
#define ABNN_EDIT_DRAW      4u
#define ABNN_EDIT_KILL      5u
#define ABNN_EDIT_HEADER_WORDS 8
#define ABNN_EDIT_KEY 0x8CB92BA72F3D8DD7ull
typedef struct abnn_edit_config {        /* 64 bytes */
    uint32_t src_first, src_count;       /* as abnn_select_config */
    uint32_t dst_first, dst_count;
    float    w_lo, w_hi;                 /* read only with ABNN_EDIT_WEIGHT; else both +0.0f */
    uint32_t flags, op;
    float    a, b;                       /* SET reads b; AFFINE and DRAW read a and b */
    float    c_lo, c_hi;                 /* read only with ABNN_EDIT_CLAMP */
    uint64_t seed;                       /* DRAW only */
    uint32_t reserved[2];                /* 0 */
} abnn_edit_config;
/* ABNN_EDIT_HEADER_WORDS, or 0 for a config that can be refused without a
 * handle: everything abnn_select_words refuses for the shared fields; an unknown
 * op or flag bit; reserved != 0; any of a, b, c_lo, c_hi, seed that the op and
 * the flags do not read and whose bits are not all zero; a NaN in a parameter
 * that is read; c_lo > c_hi; DRAW with a > b or a bound that is not finite;
 * CLAMP with KILL; ANY with a SCALE op (the key could fall outside the plane). */
uint64_t    abnn_edit_words(const abnn_edit_config* cfg);
/* Enqueue only: zeroes and fills out_dev (DEVICE memory, 8 u64) and edits the
 * records in stream order on `stream`; no synchronise and no workgroup waits for
 * another, so it can sit between passes and between abnn_engine_run calls.
 * plane_dev: the M f32 factors of a SCALE op in DEVICE memory, NULL otherwise.
 * A shard handle edits its own records.  ABNN_ERR_INVALID: a null argument, an
 * invalid config, a range that ends above N_NRN, plane_dev null with a SCALE op
 * or non-null without one, a handle whose records are invalid.  n_syn == 0 is
 * valid.                                                                       */
abnn_status abnn_edit_enqueue(abnn_brain* b, const abnn_edit_config* cfg, const float* plane_dev, uint64_t* out_dev, void* stream);
/* Synchronous convenience: plane_host (plane_count == M f32; NULL and 0 without
 * a SCALE op) is staged in scratch the handle owns (freed by abnn_brain_destroy). */
abnn_status abnn_edit(abnn_brain* b, const abnn_edit_config* cfg, const float* plane_host, uint64_t plane_count, uint64_t out_host[8]);
/* The rule on the host, without a device or a handle, on n interchange records
 * in place (local record k has global index syn_offset + k; plane: M f32 for a
 * SCALE op, else NULL).  ABNN_ERR_INVALID as abnn_edit_enqueue, for a brain of
 * n_nrn neurons.                                                               */
abnn_status abnn_edit_host(const abnn_edit_config* cfg, uint64_t n_nrn, uint64_t syn_offset, abnn_synapse* records, uint64_t n, const float* plane, uint64_t out[8]);
/* Factors from a degree-census strength plane (the int64 fixed-point words of
 * ABNN_DEG_IN_W / ABNN_DEG_OUT_W), `count` of them:
 *   S = (float)(int64_t)word * 2^-24   (one conversion, round to nearest even,
 *                                       then one exact product)
 *   f = S > 0 ? target / S : 1.0f      (one correctly rounded fp32 division)
 *   if (f < f_lo) f = f_lo;  if (f > f_hi) f = f_hi;
 * target > 0 finite and 0 < f_lo <= f_hi finite, else ABNN_ERR_INVALID.  With
 * it abnn_degree_enqueue -> abnn_edit_factors_enqueue -> abnn_edit_enqueue(
 * SCALE_DST) is synaptic scaling with nothing returning to the host.  Enqueue
 * only, on `stream`; strength_dev and plane_dev are DEVICE memory.            */
abnn_status abnn_edit_factors_enqueue(abnn_brain* b, const uint64_t* strength_dev, uint64_t count, float target, float f_lo, float f_hi, float* plane_dev, void* stream);
abnn_status abnn_edit_factors_host(const uint64_t* strength, uint64_t count, float target, float f_lo, float f_hi, float* plane);

/* ---- record reorder: sort, shuffle, permute -------------------
 * One operation over the handle's local records [0, n), n = n_syn, on the
 * device.  It produces a permutation origin[0..n) of the local indices;
 * afterwards the record at k is the old record origin[k]: src, dst and the bits
 * of w unchanged, pad 0.  Records at and past n_syn are neither read nor
 * written.  n_syn, the neuron state, the scalars, the statistics, the spike
 * recorder and an engine's driver state are untouched.
 * origin is the STABLE ascending order of the 33-bit key (tomb << 32) | k32:
 * records with equal keys keep their old relative order.
 *   tomb = (dst == 0xFFFFFFFF); a tombstone's k32 is 0 under every key and
 *   direction, so the tombstones always end up last, in their old relative
 *   order.
 *   With ABNN_REORDER_DESCENDING a live record's k32 is replaced by ~k32 (ties
 *   still keep their old order).
 *   k32 of a live record by cfg.key:
 *     ABNN_REORDER_SRC / _DST  the interchange value of src / dst
 *     ABNN_REORDER_W       the census's order key of the bits b of w: b ^ ((b >>
 *                          31) ? 0xFFFFFFFF : 0x80000000) -- a total order with
 *                          -0.0 < +0.0; NaNs sort by their bits, at the two ends
 *     ABNN_REORDER_RANDOM  (a seeded shuffle) (uint32_t)(splitmix64_at(seed ^
 *                          ABNN_REORDER_KEY, syn_offset + k) >> 32), the graph
 *                          builder's splitmix64_at, k the local index: a shard
 *                          draws what the unsharded brain draws for the same
 *                          global index
 *     ABNN_REORDER_NONE    0: only the tombstones move, to the end (an
 *                          order-preserving compaction)
 *     ABNN_REORDER_PERM    no key: origin is the caller's perm (n u32).  It is
 *                          valid only if it is a permutation of [0, n), which
 *                          is checked on the device; an invalid one leaves the
 *                          records exactly as they were and reports how many
 *                          entries were out of range or repeated an earlier
 *                          value.  Tombstones are not treated specially: PERM
 *                          with the inverse of a returned origin undoes a
 *                          reorder.
 * Result, as u64 words (abnn_reorder_words = 8 + (ORIGIN ? (n_syn + 1) / 2 : 0)):
 *   0 records (= n_syn)
 *   1 tombstones; after the call they are exactly the records [n - T, n)
 *     (except for PERM)
 *   2 moved: the k with origin[k] != k
 *   3 invalid perm entries (PERM only; non-zero: nothing moved and word 2 is 0)
 *   4 the handle's syn_offset     5..7 zero
 *   8 ...  with ABNN_REORDER_ORIGIN: origin as packed u32, two per word, the low
 *          half first (the high half of the last word of an odd n is 0; after an
 *          invalid perm it is the identity: nothing moved)
 * Bookkeeping, in stream order after the move (what a records-only snapshot
 * restore redoes): the random-mode src mirror is rebuilt and the pruning tally
 * is zeroed and recounted over [0, n), so the next structural update removes the
 * tombstones now at the end.  n_syn does not change, so the partition stays.
 * Two consequences: a snapshot diff across a reorder pairs records by index and
 * therefore reports them as rewired (the origin plane is how a caller maps
 * back); and a shard reorders its own slice only -- there is no global sort
 * across shards.
 * Scratch: two 8-byte (key, index) buffers and a 12-byte packed copy of the
 * records (one gather per record, not one per stream), 28 bytes per record of
 * syn_capacity, plus about 1 MiB.                                              */
#define ABNN_REORDER_SRC    0u
#define ABNN_REORDER_DST    1u
#define ABNN_REORDER_W      2u
#define ABNN_REORDER_RANDOM 3u
#define ABNN_REORDER_NONE   4u
#define ABNN_REORDER_PERM   5u
#define ABNN_REORDER_DESCENDING 1u  /* SRC, DST, W only */
#define ABNN_REORDER_ORIGIN     2u  /* also return origin */
#define ABNN_REORDER_HEADER_WORDS 8
#define ABNN_REORDER_SCRATCH_BYTES_PER_RECORD 28
#define ABNN_REORDER_KEY 0xC2B2AE3D27D4EB4Full
typedef struct abnn_reorder_config {     /* 32 bytes */
    uint32_t key, flags;
    uint64_t seed;                       /* RANDOM only; else 0 */
    uint32_t reserved[4];                /* 0 */
} abnn_reorder_config;
/* 8 + (ORIGIN ? (n_syn + 1) / 2 : 0), or 0 for what can be refused without a
 * handle: null, an unknown key or flag bit, DESCENDING with NONE, RANDOM or
 * PERM, a reserved word or an unread seed that is not 0, n_syn > 2^32 (local
 * indices are u32).                                                            */
uint64_t    abnn_reorder_words(const abnn_reorder_config* cfg, uint64_t n_syn);
/* Enqueue only: everything runs in stream order on `stream`; no workgroup waits
 * for another and nothing synchronises, so it can sit between passes and
 * between abnn_engine_run calls.  perm_dev: PERM's n u32 in DEVICE memory, NULL
 * otherwise.  out_dev: DEVICE memory of abnn_reorder_words(cfg, n_syn) u64.
 * The handle owns the scratch, sized for syn_capacity: the FIRST reorder call
 * on a handle allocates it and may synchronise the device; abnn_brain_destroy
 * and abnn_reorder_release free it.  Two reorders of one handle enqueued on
 * different streams must be ordered by the caller.
 * ABNN_ERR_INVALID: a null argument, what abnn_reorder_words refuses, perm_dev
 * null with PERM or non-null without it, a handle whose records are invalid, a
 * sharded pass half done.  ABNN_ERR_OOM for the scratch leaves the records
 * untouched.  n_syn == 0 is valid.                                             */
abnn_status abnn_reorder_enqueue(abnn_brain* b, const abnn_reorder_config* cfg, const uint32_t* perm_dev, uint64_t* out_dev, void* stream);
/* Synchronous convenience: perm_host is PERM's n u32 on the host (else NULL),
 * out_host holds `words` u64 (== abnn_reorder_words(cfg, n_syn)).              */
abnn_status abnn_reorder(abnn_brain* b, const abnn_reorder_config* cfg, const uint32_t* perm_host, uint64_t* out_host, uint64_t words);
/* Frees the reorder's scratch early (synchronises the device first); the next
 * reorder allocates it again.                                                  */
abnn_status abnn_reorder_release(abnn_brain* b);
/* The rule on the host, without a device or a handle, over n interchange
 * records in place (local record k has global index syn_offset + k; perm: PERM's
 * n u32, else NULL); out holds abnn_reorder_words(cfg, n) u64.  A std::stable_sort. */
abnn_status abnn_reorder_host(const abnn_reorder_config* cfg, uint64_t syn_offset, abnn_synapse* records, uint64_t n, const uint32_t* perm, uint64_t* out);

/* ---- device-side snapshots: capture, roll back, diff ----------
 * A snapshot keeps a copy of a handle's state in device memory: the records
 * [0, n_syn) (11 B each: the two src streams and {dst, w}), the two timestamp
 * planes, the scalar block and, with synaptogenesis on, the grown records that
 * wait for the next structural update.  Capture is device-to-device copies in
 * stream order; restore puts the copy back and redoes the handle's bookkeeping;
 * the diff is one streaming pass over two record arrays.  Nothing moves to the
 * host.
 *
 * Restore (synchronous: it waits for the device, as a structural update does).
 * ABNN_SNAP_RECORDS: the records and n_syn are the captured ones; the sweep is
 * partitioned for the restored n_syn as after a structural update, the records
 * at and past n_syn are whatever was there (nothing reads them: a pass masks
 * the events past its last one, exactly as after a shrinking structural
 * update), the tombstone tally is recounted, a random-mode handle's src mirror
 * rebuilt, and a handle whose records were invalid (a failed structural
 * update) is usable again: a restore is a reload.  A shard handle's caller
 * re-sums global_events afterwards (abnn_set_global_events), as after a
 * structural update.
 * ABNN_SNAP_STATE: lastFired, lastVisited, clock, reward, rbar, pass_index, the
 * abnn_inject_inputs RNG and the grown records are the captured ones; the clock
 * may move back; a shard's visit marks are cleared; abnn_get_budget answers
 * max_spikes, as before a first pass.
 * With both: capture after any passes, run any passes and structural updates,
 * restore, run P passes -- the records, lastFired, lastVisited and the scalars
 * are bit for bit what the same P passes gave when run straight after the
 * capture.
 * Not restored: the cumulative counters (abnn_get_stats, abnn_renormalisations,
 * abnn_structural_updates), the spike recorder (passes after a restore append
 * as usual), and an abnn_engine's own driver state (its rates, filters,
 * windows and teacher RNG go on from where they are).                          */
typedef struct abnn_snapshot abnn_snapshot;
#define ABNN_SNAP_RECORDS 1u   /* the records [0, n_syn) and n_syn itself */
#define ABNN_SNAP_STATE   2u   /* lastFired, lastVisited, clock, reward, rbar, pass_index,
                                  the inject_inputs RNG, the grown records waiting for the
                                  next structural update */
typedef struct abnn_snapshot_info {   /* host view, no synchronise */
    uint64_t captures;        /* 0: nothing captured yet */
    uint64_t n_syn;           /* the handle's n_syn at the last capture */
    abnn_scalars scalars;     /* clock and pass_index from the host mirrors at capture;
                                 reward and rbar are 0 here (they live on the device) */
    uint64_t bytes;           /* device memory the snapshot holds */
} abnn_snapshot_info;
/* Allocates for the handle's syn_capacity and N_NRN on the handle's device (may
 * synchronise).  ABNN_ERR_OOM leaves nothing allocated.  Destroy a snapshot
 * before its brain.                                                            */
abnn_status abnn_snapshot_create(abnn_brain* b, abnn_snapshot** out);
abnn_status abnn_snapshot_destroy(abnn_snapshot* s);
abnn_status abnn_snapshot_get_info(const abnn_snapshot* s, abnn_snapshot_info* out);
/* Enqueue only: device-to-device copies in stream order on `stream`, and the
 * host mirrors (n_syn, clock, pass_index, the RNG) as they are at the call --
 * passes and abnn_engine_run advance those when they enqueue, so a capture sits
 * between them without a synchronise.  A second capture overwrites the first.
 * ABNN_ERR_INVALID: a null argument, a snapshot of another brain, a handle
 * whose records are invalid.                                                   */
abnn_status abnn_snapshot_capture_enqueue(abnn_brain* b, abnn_snapshot* s, void* stream);
/* what: ABNN_SNAP_RECORDS | ABNN_SNAP_STATE, at least one.  ABNN_ERR_INVALID:
 * what is 0 or has unknown bits, nothing was captured yet, the snapshot belongs
 * to another brain, or a sharded pass is half done (between abnn_shard_gate and
 * abnn_shard_apply).                                                           */
abnn_status abnn_snapshot_restore(abnn_brain* b, const abnn_snapshot* s, uint32_t what);

/* The diff of two record arrays, `then` (a snapshot) and `now` (another
 * snapshot of the same brain, or NULL = the handle's records).  A = record k of
 * then, B = record k of now, for k < c = min(n_then, n_now); a tombstone is
 * dst == 0xFFFFFFFF; every comparison is one u32 or one IEEE fp32 operation.
 * Classes, in this order: both tombstones -> dead_both; A live, B a tombstone
 * -> killed; A a tombstone, B live -> revived; both live with a different src
 * or dst -> rewired; otherwise paired.  A paired record is SELECTED when it
 * passes both ranges (x - first < count; count 0 passes anything).  A selected
 * record with equal weight bits is same, else changed; for a changed record
 * d = w_B - w_A (one subtraction): d != d -> nan; d > 0 -> up; d < 0 -> down;
 * otherwise zero (a +0 / -0 pair).  A changed record with a non-NaN d counts,
 * by the census's rule on d: d < lo -> under; d >= hi -> over; otherwise bin
 * min((uint32_t)((d - lo) * scale), bins - 1), scale = (float)bins / (hi - lo);
 * and it raises the maximum of the bits of |d| taken as a u32 (+inf allowed).
 * With q(w) = (int32_t)(w * 16777216.0f), a weight summable iff |w| < 128: a
 * changed record with both weights summable adds q_B - q_A to net (int64
 * modulo 2^64) and |q_B - q_A| to abs, any other changed record 1 to
 * not_summable.
 * Result: ABNN_DIFF_HEADER_WORDS + bins u64 words:
 *    0 n_now   1 n_then   2 compared = c   3 born = n_now - c   4 gone = n_then - c
 *    5 dead_both   6 killed   7 revived   8 rewired   9 paired
 *   10 selected   11 same   12 changed   13 up   14 down   15 zero   16 nan
 *   17 under   18 over   19 net   20 abs   21 not_summable
 *   22 bits of the largest |d| in the low 32 bits (0 with none)   23 zero
 *   24... the bins
 * compared = 5+6+7+8+9; selected = same + changed; changed = up + down + zero +
 * nan; up + down + zero = under + over + sum of the bins.  Every word is an
 * integer sum or maximum: the result depends on neither the grid nor the order
 * (abnn_amd/snapshot.py restates it in numpy).  Shards diff their own records;
 * a merge adds every word except 22, which takes the maximum.                  */
#define ABNN_DIFF_MAX_BINS 4096
#define ABNN_DIFF_HEADER_WORDS 24
typedef struct abnn_diff_config {      /* 32 bytes; the fields and checks of abnn_census_config */
    float lo, hi; uint32_t bins;       /* bins over d = w_now - w_then, [lo, hi) */
    uint32_t src_first, src_count, dst_first, dst_count;   /* count 0 = any */
    uint32_t reserved;
} abnn_diff_config;
/* ABNN_DIFF_HEADER_WORDS + bins, or 0 for an invalid config (the refusals of
 * abnn_census_words).                                                          */
uint64_t abnn_snapshot_diff_words(const abnn_diff_config* cfg);
/* Enqueue only: zeroes and fills out_dev (DEVICE memory, abnn_snapshot_diff_words
 * (cfg) u64) in stream order on `stream`.  ABNN_ERR_INVALID: a null b, then, cfg
 * or out_dev, an invalid config, a range that ends above N_NRN, a snapshot with
 * nothing captured or of another brain, now == NULL on a handle whose records
 * are invalid.  n_syn == 0 on either side is valid.                            */
abnn_status abnn_snapshot_diff_enqueue(abnn_brain* b, const abnn_snapshot* then, const abnn_snapshot* now, const abnn_diff_config* cfg, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_snapshot_diff_words(cfg)).
 * Its device result buffer belongs to the handle (as abnn_census's): the
 * snapshots are only read.                                                     */
abnn_status abnn_snapshot_diff(abnn_brain* b, const abnn_snapshot* then, const abnn_snapshot* now, const abnn_diff_config* cfg, uint64_t* out_host, uint64_t words);
/* The rule on the host, without a device or a handle, over interchange records
 * of a brain of n_nrn neurons; out holds abnn_snapshot_diff_words(cfg) u64.    */
abnn_status abnn_snapshot_diff_host(const abnn_diff_config* cfg, uint64_t n_nrn, const abnn_synapse* then, uint64_t n_then, const abnn_synapse* now, uint64_t n_now, uint64_t* out);

/* ---- reachability: hop distances from a seed set -------------
 * A breadth-first search over the handle's local records [0, n_syn), on the
 * device: the hop distance of every neuron from a seed set S = [seed_first,
 * seed_first + seed_count), at most H = max_hops hops, without moving the
 * records to the host.  One hop is one streaming pass over the records against
 * a one-bit-per-neuron frontier map.
 * Followed records.  Record k < n_syn is FOLLOWED when it is live (dst !=
 * 0xFFFFFFFF), src < N_NRN and dst < N_NRN (records written through
 * abnn_state_ptrs are not validated: nothing outside the planes is indexed) and,
 * with ABNN_HOPS_WEIGHT, w >= w_lo && w < w_hi as single fp32 comparisons (NaN
 * is never followed; the bounds rules are abnn_select's).  A followed record is
 * the edge u -> v = src -> dst, with ABNN_HOPS_REVERSE dst -> src (who can reach
 * the seeds).  Records at or past n_syn are never read.
 * Result: 8 + (H + 1) + (N_NRN + 1) / 2 u64 words:
 *   0 the handle's n_syn   1 N_NRN   2 reached = the sum of the levels
 *   3 depth: the largest h with levels[h] > 0
 *   4 complete: 1 iff levels[H] == 0 (the search ran out of frontier: every
 *     reachable neuron is in the plane)                           5..7 zero
 *   8 ...          levels[0..H], one word each: the neurons at distance h
 *   8 + H + 1 ...  the distance plane: N_NRN little-endian u32 (an odd N_NRN is
 *                  padded with one zero entry); entry n is the hop distance of
 *                  neuron n from S: 0 for a seed, ABNN_HOPS_UNREACHED when it is
 *                  not reached within H hops
 * Steps.  abnn_hops_enqueue is exactly the steps BEGIN, 0, 1, ..., H in order:
 *   BEGIN     zero the header and the levels; plane = 0 on S, UNREACHED elsewhere
 *   h < H     if h > 0 and levels[h-1] == 0: nothing.  Else levels[h] = #{n :
 *             plane[n] == h}; then plane[v] = min(plane[v], h + 1) for every
 *             followed local record u -> v with plane[u] == h
 *   H         levels[H] likewise (same early-out), then words 0..4
 * The early-out is read on the device: the host enqueues every step and learns
 * nothing in between; a dead step's kernels read one word and return.
 * Distances are breadth-first levels, so the result depends on neither the
 * grid nor the order nor the timing, and every word is an integer (abnn_amd/
 * hops.py restates it in numpy).
 * Shards.  A shard holds some of the edges.  A sharded caller runs the steps
 * itself (abnn_hops_step_enqueue) and, between two steps, replaces every rank's
 * plane with the element-wise minimum over the ranks; levels[h] is recounted
 * from the plane at step h, so every rank ends with the same result: words 1..4
 * describe the whole graph, word 0 is the rank's own n_syn.
 * Scratch.  The frontier bitmap (N_NRN bits) stays with the handle: the FIRST
 * hops call on a handle allocates it and may synchronise the device;
 * abnn_brain_destroy frees it.  Two searches of one handle enqueued on
 * different streams must be ordered by the caller.                            */
#define ABNN_HOPS_MAX        1024u
#define ABNN_HOPS_REVERSE    1u   /* follow dst -> src: who can reach the seeds */
#define ABNN_HOPS_WEIGHT     2u   /* follow a record only if w_lo <= w && w < w_hi */
#define ABNN_HOPS_HEADER_WORDS 8
#define ABNN_HOPS_UNREACHED  0xFFFFFFFFu
#define ABNN_HOPS_BEGIN      0xFFFFFFFFu   /* step value: initialise */
typedef struct abnn_hops_config {   /* 32 bytes */
    uint32_t seed_first, seed_count; /* the seed set [first, first+count), count >= 1 */
    uint32_t max_hops;               /* H: 1 .. ABNN_HOPS_MAX */
    uint32_t flags;
    float    w_lo, w_hi;             /* as abnn_select_config: +0.0f unless WEIGHT */
    uint32_t reserved[2];            /* 0 */
} abnn_hops_config;
/* The result's words for a brain of n_nrn neurons, or 0 for an invalid config:
 * null, seed_count == 0, a seed range that ends above n_nrn, max_hops outside
 * 1..ABNN_HOPS_MAX, unknown flag bits, a reserved word that is not 0, a
 * non-zero w_lo or w_hi without WEIGHT, a NaN bound or w_lo >= w_hi with it,
 * n_nrn == 0.                                                                 */
uint64_t    abnn_hops_words(const abnn_hops_config* cfg, uint64_t n_nrn);
/* Enqueue only: every step in order, in stream order on `stream`, into out_dev
 * (DEVICE memory, 8-byte aligned, abnn_hops_words(cfg, N_NRN) u64); nothing
 * synchronises after the handle's first hops call, so it can sit between
 * passes.  ABNN_ERR_INVALID: a null argument, a config that is invalid for the
 * handle's N_NRN, a handle whose records are invalid.  n_syn == 0 is valid and
 * gives the seeds only.                                                       */
abnn_status abnn_hops_enqueue(abnn_brain* b, const abnn_hops_config* cfg, uint64_t* out_dev, void* stream);
/* One step (ABNN_HOPS_BEGIN, or 0 .. max_hops) of the search in out_dev; also
 * ABNN_ERR_INVALID for any other step value.  The caller runs BEGIN first and
 * the steps in increasing order.                                              */
abnn_status abnn_hops_step_enqueue(abnn_brain* b, const abnn_hops_config* cfg, uint32_t step, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_hops_words(cfg,
 * N_NRN)).  Its device result stays with the handle until abnn_brain_destroy. */
abnn_status abnn_hops(abnn_brain* b, const abnn_hops_config* cfg, uint64_t* out_host, uint64_t words);

/* ---- connected components: is it still one network -----------
 * The weakly connected components of the handle's local records [0, n_syn) over
 * a neuron range R = [first, first + count), on the device, without moving the
 * records to the host: one streaming pass over the records with a lock-free
 * union-find in a one-u32-per-neuron label plane.
 * Followed records.  Record k < n_syn is FOLLOWED when it is live (dst !=
 * 0xFFFFFFFF), src and dst are both in R (R lies inside [0, N_NRN), so nothing
 * outside the plane is ever indexed, also for records written through
 * abnn_state_ptrs that were never validated) and, with ABNN_COMP_WEIGHT, w >=
 * w_lo && w < w_hi as single fp32 comparisons (NaN is never followed; the bounds
 * rules are abnn_select's).  A followed record joins src and dst; the direction
 * is ignored and a self-loop joins nothing.  Records at or past n_syn are never
 * read.
 * Result: 8 + 32 + (N_NRN + 1) / 2 u64 words, with ABNN_COMP_SIZES (N_NRN + 1) /
 * 2 more:
 *   0 the handle's n_syn   1 N_NRN   2 followed records (this handle's)
 *   3 components: the distinct labels in R (a neuron that no followed record
 *     touches is a component of size 1)
 *   4 the size of the largest component   5 its label (the smallest label
 *     among equally large ones)           6 components of size 1
 *   7 give-up code: 0 in every correct run (see "Bounded loops")
 *   8..39   bins[j]: the components whose size s has floor(log2 s) == j
 *   40 ...  the label plane: N_NRN little-endian u32 (an odd N_NRN is padded with
 *           one zero entry); entry n is the smallest neuron id of n's
 *           component, ABNN_COMP_NONE for n outside R
 *   then, with ABNN_COMP_SIZES, the size plane, laid out likewise: entry n is
 *           the size of n's component, 0 outside R
 * Steps.  abnn_components_enqueue is exactly BEGIN, LINK, FLATTEN, CLOSE:
 *   BEGIN    zero words 0..39; plane[n] = n on R, ABNN_COMP_NONE elsewhere
 *   LINK     unite the ends of every followed local record; add them to word 2
 *   FLATTEN  replace every entry in R by the root of its tree
 *   CLOSE    count the sizes; fill words 0, 1, 3..6, the bins and the size plane
 * Any sequence BEGIN, (LINK | MERGE)*, FLATTEN, CLOSE is valid: a flattened
 * plane is again a valid forest, so LINK and MERGE may follow a FLATTEN.  The
 * plane keeps plane[x] <= x with plane[x] an ancestor of x; the root of a
 * finished component is its smallest id, so the result is canonical: it depends
 * on neither the grid nor the order nor the timing, and every word is an integer
 * (abnn_amd/components.py restates it in numpy).
 * Bounded loops.  No kernel waits for another workgroup.  A walk to a root
 * strictly decreases the id, a failed hook returns a strictly smaller id; both
 * loops also carry a hard cap (`count` steps, 2 x `count` retries).  A lane
 * that reaches it stores a non-zero code in word 7 (1 the walk, 2 the hook) and
 * stops; abnn_components then returns ABNN_ERR_HIP with the code in
 * abnn_last_error.
 * Shards.  A shard holds some of the edges.  A sharded caller runs BEGIN, LINK,
 * FLATTEN on every rank, all-gathers the label planes, and runs
 * abnn_components_merge_enqueue of all of them on every rank, then FLATTEN,
 * CLOSE.  One exchange suffices: a rank's label plane is a spanning forest of
 * that rank's connectivity.  Every rank then holds the whole graph's words 1,
 * 3..7, bins and planes; words 0 and 2 are the rank's own.
 * Scratch.  The size counters (used when SIZES is off) and the settled map (a
 * bit per neuron that LINK keeps for the neurons already in the majority tree,
 * so that a record between two of them is skipped without a walk) stay with the
 * handle: the FIRST components call on a handle allocates them, all or nothing
 * (ABNN_ERR_OOM), and may synchronise the device; abnn_brain_destroy frees them.
 * Two calls on one handle enqueued on different streams must be ordered by the
 * caller.  The calls write no record, no neuron state, no mark and no bitmap of
 * the passes.
 * Strongly connected components are out of scope; the strong component of ONE
 * seed is the intersection of a forward and a reverse abnn_hops from it.      */
#define ABNN_COMP_WEIGHT   1u   /* follow a record only if w_lo <= w && w < w_hi */
#define ABNN_COMP_SIZES    2u   /* also return the per-neuron component-size plane */
#define ABNN_COMP_HEADER_WORDS 8
#define ABNN_COMP_SIZE_BINS    32
#define ABNN_COMP_NONE     0xFFFFFFFFu
/* step values */
#define ABNN_COMP_BEGIN 0u
#define ABNN_COMP_LINK 1u
#define ABNN_COMP_FLATTEN 2u
#define ABNN_COMP_CLOSE 3u
typedef struct abnn_components_config {   /* 32 bytes */
    uint32_t first, count;   /* the neuron range R = [first, first+count), count >= 1 */
    uint32_t flags;
    float    w_lo, w_hi;     /* as abnn_hops_config: +0.0f unless WEIGHT */
    uint32_t reserved[3];    /* 0 */
} abnn_components_config;
/* The result's words for a brain of n_nrn neurons, or 0 for an invalid config:
 * null, count == 0, a range that ends above n_nrn, unknown flag bits, a
 * reserved word that is not 0, a non-zero w_lo or w_hi without WEIGHT, a NaN
 * bound or w_lo >= w_hi with it, n_nrn == 0 or >= 2^32.                        */
uint64_t    abnn_components_words(const abnn_components_config* cfg, uint64_t n_nrn);
/* Enqueue only: BEGIN, LINK, FLATTEN, CLOSE in stream order on `stream`, into
 * out_dev (DEVICE memory, 8-byte aligned, abnn_components_words(cfg, N_NRN)
 * u64); nothing synchronises after the handle's first components call, so it
 * can sit between passes and between abnn_engine_run calls.  ABNN_ERR_INVALID:
 * a null argument, a misaligned out_dev, a config that is invalid for the
 * handle's N_NRN, a handle whose records are invalid.  n_syn == 0 is valid:
 * every neuron of R is a component of its own.                                */
abnn_status abnn_components_enqueue(abnn_brain* b, const abnn_components_config* cfg, uint64_t* out_dev, void* stream);
/* One step (ABNN_COMP_BEGIN / LINK / FLATTEN / CLOSE) in out_dev; also
 * ABNN_ERR_INVALID for any other step value.                                  */
abnn_status abnn_components_step_enqueue(abnn_brain* b, const abnn_components_config* cfg, uint32_t step, uint64_t* out_dev, void* stream);
/* The shard merge, enqueue only: unites n with planes[p][n] for every n in R
 * and every p < n_planes in out_dev's plane.  planes_dev is DEVICE memory:
 * n_planes label planes one after the other, each as a result holds it (2 *
 * ((N_NRN + 1) / 2) u32, the pad entry included) -- what an all-gather of the
 * ranks' planes leaves.  An entry that is ABNN_COMP_NONE or not in R is skipped:
 * nothing is indexed from it.  Also ABNN_ERR_INVALID for a null planes_dev and
 * for n_planes == 0.                                                          */
abnn_status abnn_components_merge_enqueue(abnn_brain* b, const abnn_components_config* cfg, const uint32_t* planes_dev, uint32_t n_planes, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (==
 * abnn_components_words(cfg, N_NRN)).  Its device result stays with the handle
 * until abnn_brain_destroy.  ABNN_ERR_HIP when word 7 is not 0.               */
abnn_status abnn_components(abnn_brain* b, const abnn_components_config* cfg, uint64_t* out_host, uint64_t words);
/* The rule on the host, without a device or a handle, over interchange records
 * of a brain of n_nrn neurons; out holds `words` u64 (==
 * abnn_components_words(cfg, n_nrn)).                                          */
abnn_status abnn_components_host(const abnn_synapse* records, uint64_t n, const abnn_components_config* cfg, uint64_t n_nrn, uint64_t* out, uint64_t words);

/* ---- population connectivity matrix: who talks to whom --------
 * For a partition of the neurons into P populations, the count and the summed
 * weight of the records from population a to population b, for every pair, in
 * ONE streaming pass over the handle's local records [0, n_syn), on the device.
 * Records at or past n_syn are never read.
 * Partition.  A partition maps a neuron id to a population 0 .. P - 1 or to
 * none, 1 <= P <= ABNN_MATRIX_MAX_POPS.
 *   BOUNDS (default): P + 1 HOST u32 values bounds[0] <= bounds[1] <= ... <=
 *     bounds[P] <= N_NRN; pop(n) = j iff bounds[j] <= n < bounds[j + 1]; n <
 *     bounds[0] or n >= bounds[P] is none.  Empty populations (equal
 *     neighbours) are legal.  The values are read during the call.
 *   LABELS (ABNN_MAT_LABELS): a DEVICE plane of N_NRN little-endian u32 -- the
 *     layout of the abnn_hops distance plane and of the abnn_components label
 *     plane, so a pointer into either result is a valid argument.  pop(n) =
 *     labels[n] when n < N_NRN and labels[n] < P, otherwise none
 *     (ABNN_HOPS_UNREACHED, ABNN_COMP_NONE and any value >= P are none).  An id
 *     >= N_NRN on a live record (such records reach a handle through
 *     abnn_state_ptrs) is never used as an index.
 * Each record is classified in this order:
 *   1. dst == 0xFFFFFFFF: a tombstone (word 1).
 *   2. with ABNN_MAT_WEIGHT, a record that fails w >= w_lo && w < w_hi (single
 *      fp32 comparisons; NaN never passes; the bounds rules are abnn_select's)
 *      is out of band (word 6).
 *   3. otherwise a = pop(src), b = pop(dst): both set: COUNTED (word 2), cell
 *      a * P + b; only b set: word 3; only a set: word 4; neither: word 5.
 * Planes: one u64 per cell, row-major, one plane per bit of `what` in increasing
 * bit order.
 *   ABNN_MAT_COUNT  the counted records of the cell
 *   ABNN_MAT_W      the two's-complement sum modulo 2^64 of the degree census's
 *                   term: a record with fabsf(w) < 128 is summable, its term is
 *                   q = (int32_t)(w * 16777216.0f); a counted record that is
 *                   not summable adds nothing and is counted in word 7
 *   ABNN_MAT_P      the same with c = (w * w) * base_scale in place of w (two
 *                   fp32 operations: abnn_propagate's coefficient with FIRE_P
 *                   and its summability test): the expected spikes per visit,
 *                   the coupling the traversal sees; not summable: word 8
 * Result: ABNN_MATRIX_HEADER_WORDS + P + planes * P * P u64:
 *   0 scanned (n_syn)   1 tombstones   2 counted   3 src unassigned
 *   4 dst unassigned    5 both unassigned   6 out of band
 *   7 / 8 counted records not summable for W / P (0 unless the plane is asked)
 *   9 P   10 N_NRN   11 assigned neurons   12..15 zero
 *   16 .. 16 + P - 1   sizes[j]: the neurons of population j (BOUNDS: bounds[j +
 *                      1] - bounds[j]; LABELS: counted on the device)
 *   then the planes.
 * Words 1 + 2 + 3 + 4 + 5 + 6 == word 0, the COUNT plane sums to word 2, the
 * sizes sum to word 11.  Every word is an integer sum: the result depends on
 * neither the grid nor the order nor the timing (abnn_amd/matrix.py restates it
 * in numpy).
 * Shards.  Words 0..8 and the planes of the shards' results add up to the whole
 * graph's; words 9..11 and the sizes are the same on every rank.
 * Scratch.  A LABELS call packs the plane into one byte per neuron (N_NRN bytes)
 * that stay with the handle: the FIRST LABELS call on a handle allocates them
 * (ABNN_ERR_OOM) and may synchronise the device; abnn_brain_destroy frees them.
 * Two LABELS calls on one handle enqueued on different streams must be ordered
 * by the caller.  The calls write no record, no neuron state and no bitmap of
 * the passes, and no workgroup waits for another.                             */
#define ABNN_MAT_COUNT   1u   /* `what`: the planes */
#define ABNN_MAT_W       2u
#define ABNN_MAT_P       4u
#define ABNN_MAT_LABELS  1u   /* `flags`: the partition is a device label plane */
#define ABNN_MAT_WEIGHT  2u   /* count a record only if w_lo <= w && w < w_hi */
#define ABNN_MATRIX_MAX_POPS     64
#define ABNN_MATRIX_HEADER_WORDS 16
typedef struct abnn_matrix_config {   /* 32 bytes */
    uint32_t pops;           /* P */
    uint32_t what;           /* a non-empty subset of COUNT | W | P */
    uint32_t flags;          /* ABNN_MAT_LABELS, ABNN_MAT_WEIGHT */
    float    w_lo, w_hi;     /* as abnn_hops_config: +0.0f unless WEIGHT */
    uint32_t reserved[3];    /* 0 */
} abnn_matrix_config;
/* The result's words, or 0 for an invalid config: null, pops outside 1..64,
 * `what` empty or with unknown bits, unknown flag bits, a reserved word that is
 * not 0, a non-zero w_lo or w_hi without WEIGHT, a NaN bound or w_lo >= w_hi
 * with it.                                                                    */
uint64_t    abnn_matrix_words(const abnn_matrix_config* cfg);
/* Enqueue only, in stream order on `stream`, into out_dev (DEVICE memory, 8-byte
 * aligned, abnn_matrix_words(cfg) u64); nothing synchronises after the handle's
 * first LABELS call, so it can sit between passes and between abnn_engine_run
 * calls.  Exactly one of bounds_host / labels_dev is non-null, the one the
 * LABELS flag names.  ABNN_ERR_INVALID: a null argument, a misaligned out_dev or
 * labels_dev (4 bytes), an invalid config, a partition argument that contradicts
 * the flag, decreasing bounds, bounds[P] > N_NRN, a handle whose records are
 * invalid.  n_syn == 0 is valid: the sizes only.                              */
abnn_status abnn_matrix_enqueue(abnn_brain* b, const abnn_matrix_config* cfg, const uint32_t* bounds_host, const uint32_t* labels_dev, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_matrix_words(cfg)).
 * Its device result stays with the handle until abnn_brain_destroy.           */
abnn_status abnn_matrix(abnn_brain* b, const abnn_matrix_config* cfg, const uint32_t* bounds_host, const uint32_t* labels_dev, uint64_t* out_host, uint64_t words);
/* The rule on the host, without a device or a handle, over interchange records
 * of a brain of n_nrn neurons (1 <= n_nrn < 2^32); `labels` is a HOST plane of
 * n_nrn u32 here; base_scale is abnn_params.base_scale (the P plane's).       */
abnn_status abnn_matrix_host(const abnn_synapse* records, uint64_t n, const abnn_matrix_config* cfg, const uint32_t* bounds, const uint32_t* labels, uint64_t n_nrn, float base_scale, uint64_t* out, uint64_t words);

/* ---- signal propagation: W.x and the branching ratio ----------
 * The handle's local records [0, n_syn) used as the sparse matrix they are: one
 * streaming pass y[kout] += c(w) * x[kin] on the device, in integers, without
 * moving the records to the host.  x is a plane of N_NRN int32: a fixed-point
 * activity whose scale is the caller's (abnn_amd/propagate.py uses 1 << 30).
 * For a record (src, dst, w): kin = src, kout = dst; with ABNN_PROP_REVERSE kin =
 * dst, kout = src (the transpose).  In = [in_first, in_first + in_count), Out =
 * [out_first, out_first + M) likewise (a count of 0: every neuron).
 * Followed records.  Record k < n_syn is FOLLOWED when it is live (dst !=
 * 0xFFFFFFFF), kin - in_first < in_count and kout - out_first < M as u32
 * comparisons, with ABNN_PROP_WEIGHT w >= w_lo && w < w_hi (abnn_select's rule:
 * NaN never matches), and x[kin] != 0.  Records at or past n_syn are never read.
 * Term.  c = w, with ABNN_PROP_FIRE_P c = (w*w)*base_scale (the handle's
 * base_scale; two fp32 operations in this order): the probability that an event
 * on the record fires.  c is SUMMABLE iff fabsf(c) < 128.0f; then q =
 * (int32_t)(c * 16777216.0f) (the degree census's term), term = ((int64_t)q *
 * (int64_t)x[kin]) >> 16 (arithmetic: a floor) and y[kout - out_first] += term
 * modulo 2^64.  y carries 8 fractional bits more than x: its value is
 * (int64_t)y / 256 in x's units.  A followed record that is not summable adds
 * nothing and counts in word 3.
 * Result: ABNN_PROP_HEADER_WORDS + M u64 words:
 *   0 records scanned (= n_syn)   1 tombstones among them
 *   2 records followed            3 followed records that are not summable
 *   4 non-zero x in In            5 the sum of |x| over In           6, 7 zero
 *   8... y, word j belongs to neuron out_first + j.
 * Every word is an integer sum, so the result is the same for any grid, order
 * and path (abnn_amd/propagate.py restates it in numpy).  A tombstone carries
 * src = dst = 0xFFFFFFFF (every writer of records keeps the two together): the
 * sparse forward path counts word 1 from the src stream.
 * Rescale.  A result's y into the next x over Out: Mx = max |y_j| as u64
 * (INT64_MIN counts as 2^63), L = the bit length of Mx, e = 30 - L, x[out_first
 * + j] = (int32_t)(e >= 0 ? y_j << e : y_j >> -e) (arithmetic), so that 2^29 <=
 * max |x| <= 2^30; Mx == 0 gives x = 0 and e = 0.  x outside Out is not touched.
 * Its trace row, 8 u64: {word 4, word 5, the sum of |y| mod 2^64, Mx,
 * (uint64_t)(int64_t)e, word 2, word 3, 0}.  (sum |y| / 256) / word 5 estimates
 * the step's eigenvalue: for non-negative c and x it converges, iterated, to the
 * spectral radius of the operator restricted to Out x Out -- with FIRE_P the
 * branching ratio.
 * Iterate.  `steps` (1 .. ABNN_PROP_MAX_STEPS) times propagate x -> work, rescale
 * work -> x, one trace row per step; In and Out must be the same range.
 * Shards.  A shard propagates its own records; the sum of the shards' results,
 * word by word except words 4 and 5 (every shard reads the same x), is the
 * unsharded result, and the rescale follows the sum.
 * Scratch.  The non-zero map (N_NRN bits) and the rescale's two words stay with
 * the handle: the FIRST propagate call on a handle allocates them and may
 * synchronise the device; abnn_brain_destroy frees them.  Two propagations of
 * one handle enqueued on different streams must be ordered by the caller.      */
#define ABNN_PROP_REVERSE   1u   /* the transpose: kin = dst, kout = src */
#define ABNN_PROP_FIRE_P    2u   /* c = (w*w)*base_scale, not w */
#define ABNN_PROP_WEIGHT    4u   /* follow a record only if w_lo <= w && w < w_hi */
#define ABNN_PROP_HEADER_WORDS 8
#define ABNN_PROP_TRACE_WORDS  8
#define ABNN_PROP_MAX_STEPS 4096u
typedef struct abnn_propagate_config {   /* 48 bytes */
    uint32_t in_first, in_count;     /* In; count 0 = every neuron (first must be 0) */
    uint32_t out_first, out_count;   /* Out, likewise */
    uint32_t flags;
    float    w_lo, w_hi;             /* as abnn_select_config: +0.0f unless WEIGHT */
    uint32_t reserved[5];            /* 0 */
} abnn_propagate_config;
/* The result's words for a brain of n_nrn neurons, or 0 for an invalid config:
 * null, unknown flag bits, a reserved word that is not 0, a count of 0 with a
 * first that is not, a range that ends above n_nrn, a non-zero w_lo or w_hi
 * without WEIGHT, a NaN bound or w_lo >= w_hi with it, n_nrn == 0 or >= 2^32.  */
uint64_t    abnn_propagate_words(const abnn_propagate_config* cfg, uint64_t n_nrn);
/* Enqueue only: zeroes and fills out_dev (DEVICE memory, 8-byte aligned,
 * abnn_propagate_words(cfg, N_NRN) u64) from x_dev (DEVICE memory, 16-byte
 * aligned, N_NRN int32) in stream order on `stream`; nothing synchronises after
 * the handle's first propagate call, so it can sit between passes and between
 * abnn_engine_run calls.  ABNN_ERR_INVALID: a null argument, a misaligned
 * plane, a config that is invalid for the handle's N_NRN, a handle whose
 * records are invalid.  n_syn == 0 is valid: y is zero.                        */
abnn_status abnn_propagate_enqueue(abnn_brain* b, const abnn_propagate_config* cfg, const int32_t* x_dev, uint64_t* out_dev, void* stream);
/* Synchronous convenience with host planes: x_host holds N_NRN int32, out_host
 * `words` u64 (== abnn_propagate_words(cfg, N_NRN)).  Its device planes stay
 * with the handle until abnn_brain_destroy.                                    */
abnn_status abnn_propagate(abnn_brain* b, const abnn_propagate_config* cfg, const int32_t* x_host, uint64_t* out_host, uint64_t words);
/* Enqueue only: the rescale of the result out_dev into x_dev over Out and, when
 * trace_row_dev is not null, its trace row (DEVICE memory, 8 u64).             */
abnn_status abnn_propagate_rescale_enqueue(abnn_brain* b, const abnn_propagate_config* cfg, const uint64_t* out_dev, int32_t* x_dev, uint64_t* trace_row_dev, void* stream);
/* Enqueue only: `steps` times propagate and rescale; x_dev ends as the last
 * rescaled plane, work_dev (abnn_propagate_words u64) as the last result,
 * trace_dev (steps x 8 u64) holds one row per step.  Also ABNN_ERR_INVALID for
 * steps outside 1..ABNN_PROP_MAX_STEPS and for In != Out.                      */
abnn_status abnn_propagate_iterate_enqueue(abnn_brain* b, const abnn_propagate_config* cfg, uint32_t steps, int32_t* x_dev, uint64_t* work_dev, uint64_t* trace_dev, void* stream);
/* The rule on the host, without a device or a handle, over interchange records
 * of a brain of n_nrn neurons with the given base_scale; x holds n_nrn int32,
 * out abnn_propagate_words(cfg, n_nrn) u64.                                    */
abnn_status abnn_propagate_host(const abnn_propagate_config* cfg, uint64_t n_nrn, float base_scale, const abnn_synapse* syn, uint64_t n_syn, const int32_t* x, uint64_t* out);
/* The rescale on the host: `out` is a result, x (n_nrn int32) is rewritten over
 * Out, trace_row (8 u64) may be null.                                          */
abnn_status abnn_propagate_rescale_host(const abnn_propagate_config* cfg, uint64_t n_nrn, const uint64_t* out, int32_t* x, uint64_t* trace_row);

/* ---- spike recorder -----------------------------------------
 * A recorder attached to a handle.  While it is on, every pass the handle
 * completes (abnn_traverse, the passes inside abnn_engine_run, abnn_shard_commit
 * / abnn_shard_traverse) enqueues one small launch, in stream order after the
 * pass's kernels, that appends the pass's spikes to device buffers.  Nothing
 * synchronises and nothing returns to the host; with the recorder off a pass
 * enqueues exactly what it enqueued before.
 * For one pass, L is its spike list: the dst of every spike the traversal
 * emitted, in global budget order -- exactly the sequence of lastFired[dst] =
 * now stamps of schedule C1.  |L| is the pass's increment of abnn_stats.fired;
 * a dst may occur many times.  Stamps written by the host or by the learning
 * loop's boundary kernel (abnn_inject_inputs, teacher forcing,
 * abnn_set_timestamps / abnn_set_last_fired, the auto-stimulus) are not spikes
 * of the traversal and are not in L.  S is the subsequence of L whose dst lies
 * in [first, first + count), or all of L when count == 0, in the same order.
 * Per pass:
 *   - passes_seen += 1, spikes_seen += |L|, selected_seen += |S|;
 *   - with counts: counts[d - first] += 1 (u32) for every entry d of S -- over
 *     every pass since the start, dropped ones included;
 *   - the pass is RECORDED iff no earlier pass was dropped since the start or
 *     the last clear, the pass table has a free entry, and raster_capacity == 0
 *     or spikes_recorded + |S| <= raster_capacity.  A recorded pass appends its
 *     abnn_spike_pass entry (offset = spikes_recorded before it), with a raster
 *     also S as u32 dst, and adds 1 / |S| to passes_recorded / spikes_recorded;
 *   - otherwise it is DROPPED whole (passes_dropped += 1, spikes_dropped +=
 *     |S|), and so is every later pass until a clear: the recorded passes are
 *     always the first K consecutive ones and the raster never holds part of a
 *     pass.
 * Every word is an integer, so the result does not depend on the launch shape
 * (abnn_amd/spikes.py restates the rule in numpy).  A shard handle is accepted:
 * every rank's spike list is the merged global one, so any rank's recorder
 * holds the whole network's spikes.                                           */
typedef struct abnn_spikes_config {      /* 32 bytes */
    uint64_t raster_capacity;   /* spikes the raster holds; 0 = keep no raster (pass table and counts only) */
    uint32_t pass_capacity;     /* pass entries held, >= 1 */
    uint32_t first, count;      /* count 0 = every neuron; else only dst in [first, first + count) */
    uint32_t counts;            /* 1: keep per-neuron spike counts over the selected neurons */
    uint32_t reserved[2];       /* 0 */
} abnn_spikes_config;
typedef struct abnn_spike_pass {         /* 32 bytes, one per recorded pass */
    uint64_t pass_index;        /* abnn_scalars.pass_index the pass ran as (before its +1) */
    uint64_t now;               /* the pass-start clock = the value its stamps wrote */
    uint64_t offset;            /* its first raster entry */
    uint32_t count;             /* |S| */
    uint32_t epoch;             /* abnn_renormalisations before the pass (low 32 bits) */
} abnn_spike_pass;
typedef struct abnn_spikes_info {        /* u64 words; host view after a synchronise */
    uint64_t passes_seen, spikes_seen, selected_seen;   /* since start: passes, sum |L|, sum |S| */
    uint64_t passes_recorded, spikes_recorded;           /* since start or the last clear */
    uint64_t passes_dropped, spikes_dropped;             /* since start or the last clear; spikes = sum |S| of dropped passes */
} abnn_spikes_info;
/* Allocates and zeroes the recorder's buffers and synchronises; a second call
 * restarts (the old recorder is freed first).  ABNN_ERR_INVALID: a null
 * argument, reserved != 0, counts > 1, pass_capacity == 0, a range that ends
 * above N_NRN.  ABNN_ERR_OOM: an allocation failed.  A failed start leaves no
 * recorder (one that was running is stopped) and the handle usable.          */
abnn_status abnn_spikes_start(abnn_brain* b, const abnn_spikes_config* cfg);
/* Synchronises and frees.  abnn_brain_destroy frees too.  Every function below
 * (and this one) returns ABNN_ERR_INVALID when the handle has no recorder.    */
abnn_status abnn_spikes_stop(abnn_brain* b);
/* Synchronises, empties the pass table and the raster and re-arms recording:
 * the *_recorded and *_dropped words restart at 0, the *_seen words go on.
 * keep_counts == 0 also zeroes the per-neuron counts.                         */
abnn_status abnn_spikes_clear(abnn_brain* b, int keep_counts);
/* The readers synchronise first, like every state accessor.  A read beyond
 * what is recorded is ABNN_ERR_INVALID: passes [first, first + n) within
 * passes_recorded; raster entries within spikes_recorded (any n > 0 without a
 * raster); counts for the ABSOLUTE neuron ids [first_neuron, first_neuron + n)
 * inside the selected range (every neuron when count == 0), counts on.        */
abnn_status abnn_spikes_get_info(abnn_brain* b, abnn_spikes_info* out);
abnn_status abnn_spikes_read_passes(abnn_brain* b, uint64_t first, uint64_t n, abnn_spike_pass* out);
abnn_status abnn_spikes_read_raster(abnn_brain* b, uint64_t first, uint64_t n, uint32_t* out);
abnn_status abnn_spikes_read_counts(abnn_brain* b, uint64_t first_neuron, uint64_t n, uint32_t* out);
/* Synchronises and replaces the recorded passes and the raster with the host's:
 * the state afterwards is as after a clear followed by n_passes recorded
 * passes.  passes_recorded = n_passes, spikes_recorded = n_raster, the *_dropped
 * words and the sticky flag zero; the *_seen words and the per-neuron counts are
 * left as they are.  Refused with ABNN_ERR_INVALID, before anything is written:
 * no recorder or no raster, a null array that is not empty, n_passes >
 * pass_capacity, n_raster > raster_capacity, offsets that are not 0, count_0,
 * count_0 + count_1, ... summing to n_raster, an id at or above N_NRN, an id
 * outside the recorder's range.                                               */
abnn_status abnn_spikes_load(abnn_brain* b, const abnn_spike_pass* passes, uint64_t n_passes, const uint32_t* raster, uint64_t n_raster);

/* ---- spike correlograms --------------------------------------
 * A correlogram of the recorder's raster, computed on the device without moving
 * the raster or the records to the host.
 * Rows.  The recorded passes are rows 0 .. K-1 of the pass table; K is
 * passes_recorded (at most pass_capacity) as it stands in stream order when the
 * kernels run: it is read on the device.  The window is [row_first, row_first +
 * row_count) ∩ [0, K); row_count == 0 means "through row K-1".  Row r holds the
 * entries raster[offset_r + i], i < count_r (offset + count clamped to
 * raster_capacity); an entry is a neuron id and may repeat within a row.
 * Lag.  The lag of an ordered pair of entries (e in row p, f in row q) is q - p,
 * a difference of TABLE ROWS: consecutive rows are consecutive passes (one clock
 * tick each) unless an abnn_spikes_clear, an abnn_spikes_load or a state restore
 * came between them; that is not detected.  Pairs with |q - p| <= L = max_lag
 * count, 0 <= L <= ABNN_CORR_MAX_LAG; both rows lie inside the window.
 * Populations.  A (the reference, "pre") and B (the target, "post") are ranges
 * with the u32 test x - first < count; count == 0 means every neuron.  An id at
 * or above N_NRN (the recorder writes none, abnn_spikes_load refuses them) is
 * in neither.
 * Modes.
 *   ABNN_CORR_POP       H[l + L] = the pairs (e, f) with id(e) in A, id(f) in B
 *                       and lag l.  Nothing is excluded: at l = 0 an entry whose
 *                       id is in both ranges pairs with itself.  2L + 1 words.
 *   ABNN_CORR_PAIRS     the same count split by the two ids: M[((x - a_first) *
 *                       b_count + (y - b_first)) * (2L + 1) + l + L]; both
 *                       counts >= 1 and a_count * b_count * (2L + 1) <=
 *                       ABNN_CORR_MAX_PAIR_WORDS.
 *   ABNN_CORR_SYNAPSES  H[l + L] = the sum, over the FOLLOWED local records k <
 *                       n_syn, of the pairs (e, f) with id(e) == src_k, id(f) ==
 *                       dst_k and lag l: a positive lag is post after pre.  A
 *                       record is followed when it is live (dst != 0xFFFFFFFF),
 *                       src < N_NRN and dst < N_NRN, src is in A and dst is in B
 *                       and, with ABNN_CORR_WEIGHT, w >= w_lo && w < w_hi
 *                       (abnn_select's rule: NaN never matches).  A followed
 *                       record is COUPLED when it adds at least one pair.
 *                       Records at or past n_syn are never read.  The mode
 *                       equals the sum of M_all[src_k][dst_k][.] over the
 *                       followed records.
 * Result: abnn_corr_words(cfg) u64 words, a header of 8 and the plane:
 *   0 rows used   1 entries in the window   2 entries with id in A   3 ... in B
 *   4 the sum of the plane   5 followed records   6 coupled records (5, 6:
 *   SYNAPSES, else 0)   7 K
 * Every word is an integer sum, so the result depends on neither the grid nor
 * the order nor the timing (abnn_amd/corr.py restates it in numpy).  Shards: a
 * rank follows its own records, so a sharded caller adds words 4..6 and the
 * plane of SYNAPSES over the ranks; every rank's recorder holds the whole
 * network's spikes, so POP and PAIRS are the same on every rank.  The recorder's
 * own neuron range applies upstream: a neuron it did not keep has no entries.
 * Scratch.  The per-row tallies, the one-bit-per-neuron map, three u32 planes of
 * N_NRN and the row lists (one u32 per raster entry) stay with the handle: the
 * FIRST correlogram of a handle, and the first after its recorder was restarted
 * larger, allocates them and may synchronise the device; abnn_brain_destroy
 * frees them.  Two correlograms of one handle enqueued on different streams
 * must be ordered by the caller.                                              */
#define ABNN_CORR_MAX_LAG        256u
#define ABNN_CORR_MAX_PAIR_WORDS (1ull << 24)
#define ABNN_CORR_POP       0u
#define ABNN_CORR_PAIRS     1u
#define ABNN_CORR_SYNAPSES  2u
#define ABNN_CORR_WEIGHT    1u   /* flag, SYNAPSES: follow a record only if w_lo <= w && w < w_hi */
#define ABNN_CORR_HEADER_WORDS 8
typedef struct abnn_corr_config {        /* 64 bytes */
    uint32_t a_first, a_count;           /* population A ("pre"); count 0 = every neuron */
    uint32_t b_first, b_count;           /* population B ("post") */
    uint64_t row_first, row_count;       /* the window of table rows; count 0 = through row K-1 */
    uint32_t max_lag;                    /* L: 0 .. ABNN_CORR_MAX_LAG */
    uint32_t mode;                       /* ABNN_CORR_POP / PAIRS / SYNAPSES */
    uint32_t flags;                      /* ABNN_CORR_WEIGHT */
    float    w_lo, w_hi;                 /* as abnn_select_config: +0.0f unless WEIGHT */
    uint32_t reserved[3];                /* 0 */
} abnn_corr_config;
/* The result's words, or 0 for an invalid config (whatever can be checked
 * without a handle): null, an unknown mode or flag bit, max_lag above the cap,
 * a range whose first + count exceeds 2^32, PAIRS with a zero count or more
 * than ABNN_CORR_MAX_PAIR_WORDS plane words, a non-zero w_lo or w_hi without
 * WEIGHT, a NaN bound or w_lo >= w_hi with it, a reserved word that is not 0. */
uint64_t    abnn_corr_words(const abnn_corr_config* cfg);
/* Enqueue only: zeroes and fills out_dev (DEVICE memory, 8-byte aligned,
 * abnn_corr_words(cfg) u64) in stream order on `stream`; nothing synchronises
 * after the handle's first call, so it can sit between passes and between
 * abnn_engine_run calls.  ABNN_ERR_INVALID: a null argument, an invalid config,
 * a range that ends above N_NRN, no recorder, a recorder without a raster,
 * SYNAPSES on a handle whose records are invalid.  n_syn == 0 and K == 0 are
 * valid and give zero planes.                                                 */
abnn_status abnn_corr_enqueue(abnn_brain* b, const abnn_corr_config* cfg, uint64_t* out_dev, void* stream);
/* Synchronous convenience: out_host holds `words` u64 (== abnn_corr_words(cfg)).
 * Its device result stays with the handle until abnn_brain_destroy.           */
abnn_status abnn_corr(abnn_brain* b, const abnn_corr_config* cfg, uint64_t* out_host, uint64_t words);
/* The rule on the host, without a device or a handle, over a pass table and a
 * raster of a brain of n_nrn neurons (K = n_passes, raster_capacity = n_raster)
 * and, for SYNAPSES, interchange records (else NULL / 0); out holds
 * abnn_corr_words(cfg) u64.  ABNN_ERR_INVALID as abnn_corr_enqueue.           */
abnn_status abnn_corr_host(const abnn_corr_config* cfg, uint64_t n_nrn, const abnn_spike_pass* passes, uint64_t n_passes, const uint32_t* raster, uint64_t n_raster, const abnn_synapse* records, uint64_t n_records, uint64_t* out);

/* ---- neuron timestamps / scalars ----------------------------------------- */
abnn_status abnn_get_last_fired(abnn_brain* b, uint64_t first, uint64_t* out, uint64_t n);
abnn_status abnn_set_last_fired(abnn_brain* b, uint64_t first, const uint64_t* src, uint64_t n);
abnn_status abnn_get_last_visited(abnn_brain* b, uint64_t first, uint64_t* out, uint64_t n);
abnn_status abnn_set_last_visited(abnn_brain* b, uint64_t first, const uint64_t* src, uint64_t n);
/* (A shard's abnn_set_last_visited clears the visit marks of what it writes,
 * and a write of [0, N_NRN) leaves none unmerged.  Writes through the
 * abnn_state_ptrs pointers bypass the marks and the host's bookkeeping: use
 * the setters on sharded brains.) */
/* lastFired[idx[i]] = value for i < n (teacher / input spikes written by the
 * host, brain.cpp:82, brain-engine.cpp:131). */
abnn_status abnn_set_timestamps(abnn_brain* b, const uint32_t* idx, uint64_t n, uint64_t value);
abnn_status abnn_get_scalars(abnn_brain* b, abnn_scalars* out);
abnn_status abnn_set_scalars(abnn_brain* b, const abnn_scalars* in);
/* *reward = r (brain-engine.cpp:180-182). */
abnn_status abnn_set_reward(abnn_brain* b, float r);

/* ---- pass-boundary hooks --------------------------------------------------
 * Brain::inject_inputs(vals, hz), brain.cpp:73-83: for every input i,
 * lastFired[i] = clock when uni() < hz*kTickNS*NSEC_PER_SEC * v[i]; uni() is
 * the handle's seeded host RNG (params.seed) instead of a random_device mt19937.
 * n must equal n_input (the reference asserts it, brain.cpp:75).            */
abnn_status abnn_inject_inputs(abnn_brain* b, const float* v, uint32_t n, float hz);
/* Brain::read_outputs(), brain.cpp:145-157: out[o] = 1 iff
 * ts = lastFired[n_input+o] != 0 && start <= ts < now, start = now>1 ? now-1 : 0.
 * n must equal n_output.                                                     */
abnn_status abnn_read_outputs(abnn_brain* b, uint8_t* out, uint32_t n);
/* Stamp lastFired[first, first+count) = clock at the start of EVERY pass
 * (fused into the pass; the bench stimulus of SURVEY §8d).  count = 0 = off. */
abnn_status abnn_set_auto_stimulus(abnn_brain* b, uint64_t first, uint64_t count);

/* ---- passes: Brain::encode_traversal + commit/wait ------------------------
 * brain.cpp:87-141 + brain-engine.cpp:136-141.  Enqueues `passes` whole C1
 * passes (traversal + clock tick + renormalisation when the pass-start clock
 * exceeds renorm_thresh) on `stream` (NULL = the default stream).  Returns
 * without waiting; abnn_synchronize waits for `stream` and the device.       */
abnn_status abnn_traverse(abnn_brain* b, uint32_t passes, void* stream);
abnn_status abnn_synchronize(abnn_brain* b, void* stream);

/* ---- device-resident learning loop -------------------------
 * BrainEngine::run_one_pass (brain-engine.cpp:108-190, restated in
 * include/abnn/engine.hpp) with the driver's state on the device: one
 * abnn_engine_run enqueues `passes` whole learning passes -- input injection,
 * teacher forcing, the traversal, the output read, the rate filter and the
 * windowed loss -> reward -- and nothing synchronises until the caller asks
 * for results.  The results are bit-identical to abnn::BrainEngine<Brain>::
 * run_one_pass called `passes` times with the same brain, config and frames.
 * Input draws continue the handle's RNG (abnn_inject_inputs' stream); teacher
 * draws use the engine's own stream (teacher_seed).  One engine per brain; a
 * sharded handle is refused.  Destroy the engine before its brain.           */
typedef struct abnn_engine_config {   /* defaults = abnn::EngineConfig's */
    float input_rate_hz, peak_decay, rate_alpha, max_observed;
    double filter_tau, dt_sec, last_loss;
    uint32_t use_fir, fir_size, win_size;
    uint32_t trace_passes;            /* capacity of the per-pass record, default 4096 */
    uint64_t teacher_seed;
} abnn_engine_config;
typedef struct abnn_engine_state {    /* host view after a synchronise */
    uint64_t step, windows, win_pos;
    uint32_t teach;                   /* the reference's `even` */
    float max_observed, last_reward;
    double last_loss;
} abnn_engine_state;
typedef struct abnn_engine abnn_engine;

void abnn_default_engine_config(abnn_engine_config* cfg);
abnn_status abnn_engine_create(abnn_brain* b, const abnn_engine_config* cfg, abnn_engine** out);
abnn_status abnn_engine_destroy(abnn_engine* e);
/* in_frames: passes x n_input floats, expected_frames: passes x n_output
 * floats (HOST memory; frame p = what nextInput() / nextExpected() returned
 * for pass p; copied before the call returns).  Enqueues only: it does not
 * wait for the passes of an earlier call.  passes <= trace_passes.           */
abnn_status abnn_engine_run(abnn_engine* e, const float* in_frames, const float* expected_frames,
                            uint32_t passes, void* stream);
/* The three below synchronise first (the device, as every state accessor). */
abnn_status abnn_engine_get_state(abnn_engine* e, abnn_engine_state* out);
/* rate = the output-spike EWMA, smooth = the last pass's normalised rates;
 * any of the three may be NULL.  n_output must equal the brain's.           */
abnn_status abnn_engine_get_rates(abnn_engine* e, float* rate, float* smooth,
                                  uint32_t* spike_window, uint32_t n_output);
/* Per-pass record of steps [first_step, first_step + n): out = n x n_output u8
 * output spikes, smooth = n x n_output normalised rates (either may be NULL).
 * Held for the last trace_passes steps; an older (or future) step is
 * ABNN_ERR_INVALID.                                                          */
abnn_status abnn_engine_read_trace(abnn_engine* e, uint64_t first_step, uint32_t n,
                                   uint8_t* out, float* smooth);
/* A synapse census (above) every `every` steps inside the loop.  cfg NULL =
 * off.  From now on a census is enqueued right after the boundary launch that
 * closes every step whose step count is a multiple of `every` (>= 1), into a
 * device ring of `capacity` (>= 1) results; restarts the ring (and waits for
 * the device).  The census sees the weights after that step's pass.
 * abnn_engine_run stays enqueue-only; with the census off it enqueues exactly
 * what it enqueues without this call.                                        */
abnn_status abnn_engine_set_census(abnn_engine* e, const abnn_census_config* cfg, uint32_t every, uint32_t capacity);
/* Censuses taken since abnn_engine_set_census (host-side count, no synchronisation). */
uint64_t abnn_engine_census_count(const abnn_engine* e);
/* Snapshots [first, first + n) since abnn_engine_set_census: out = n x
 * abnn_census_words(cfg) u64, steps = n u64 (the step count each was taken
 * at); either may be NULL.  Synchronises.  An evicted or not yet taken
 * snapshot is ABNN_ERR_INVALID.                                              */
abnn_status abnn_engine_read_census(abnn_engine* e, uint64_t first, uint32_t n, uint64_t* out, uint64_t* steps);

/* ---- sharded passes (synapse-shard data parallelism) --------
 * One pass on rank r of W = three calls around ONE exchange:
 *   abnn_shard_gate   -> writes this shard's exchange record to `xchg_dev`
 *                        (abnn_exchange_bytes(b) bytes): ABNN_SUMMARY_WORDS
 *                        int64 {spike candidates capped at the budget, global
 *                        event 0 reached the update, visited events, passed the
 *                        refractory gate}, then the shard's spikes (dst, int32)
 *                        in local budget order, max_spikes slots (padded to 8 B);
 *   [all-gather the W records, rank order, into `gathered_dev`]
 *   abnn_shard_apply  -> weight updates of this shard's events that fall inside
 *                        the global budget (offset = capped sum of lower ranks);
 *   abnn_shard_commit -> stamps every shard's spikes in rank order (= global
 *                        budget order, the first max_spikes), updates rBar,
 *                        ticks the clock, renormalises if due.
 * All pointers are device pointers; the exchange is the caller's (RCCL via
 * torch.distributed in abnn_amd/shard.py).  W = 1 with the local record is
 * exactly abnn_traverse.                                                     */
#define ABNN_SUMMARY_WORDS 4
uint64_t abnn_exchange_bytes(const abnn_brain* b);
/* abnn_dims.global_events after the shards' record counts changed (structural
 * updates): the visited events of all shards per pass (the clock-tick rule,
 * brain.metal:61,129).  The caller sums the shards' visited events (an
 * all-reduce) and sets it on every rank.                                    */
abnn_status abnn_set_global_events(abnn_brain* b, uint64_t global_events);
abnn_status abnn_shard_gate(abnn_brain* b, void* xchg_dev, void* stream);
abnn_status abnn_shard_apply(abnn_brain* b, const void* gathered_dev, uint32_t world,
                             uint32_t rank, void* stream);
abnn_status abnn_shard_commit(abnn_brain* b, const void* gathered_dev, uint32_t world,
                              void* stream);

/* The lastVisited merge of a sharded brain with track_visits.
 * Unsharded, lastVisited[n] holds the last value written: the clock of the
 * last pass that visited n, or what the host wrote after it.  Each shard
 * marks the neurons its passes visit; between merges the clock only moves
 * forward (abnn_set_scalars refuses to move it back over unmerged visits, and
 * abnn_shard_traverse merges after every renormalisation), so the shard that
 * visited n last wrote the largest value:
 *   abnn_shard_visits_delta -> delta_dev[i] = visited since the last merge ?
 *                              lastVisited[i] + 1 : 0   (u64 x N_NRN, device)
 *   [all-reduce(MAX) of the deltas over the shards]
 *   abnn_shard_visits_merge -> lastVisited[i] = reduced[i] - 1 where reduced[i]
 *                              != 0; every mark clears.
 * A caller driving the shard phases itself merges whenever
 * abnn_renormalisations changed after a pass, and before reading lastVisited
 * (abnn_comm_sync_visits does all three steps over RCCL).  Host writes
 * (abnn_set_last_visited, abnn_load_flat) must be the same on every shard;
 * they clear the marks of what they write.  Without track_visits both calls
 * are no-ops (delta = 0).                                                    */
abnn_status abnn_shard_visits_delta(abnn_brain* b, void* delta_dev, void* stream);
abnn_status abnn_shard_visits_merge(abnn_brain* b, const void* reduced_dev, void* stream);
/* Renormalisations run by this handle (host-side count, no synchronisation). */
uint64_t abnn_renormalisations(const abnn_brain* b);

/* Spike budget left by the last pass: max_spikes minus the spikes it emitted
 * (the reference's bufBudget_ after a pass, brain.h:58; the host resets it to
 * kMaxSpikes before every pass, brain.cpp:90, here the max_spikes knob; C1 never
 * lets it wrap).  max_spikes before the first pass (brain.cpp:66). */
abnn_status abnn_get_budget(abnn_brain* b, uint32_t* remaining);
/* Structural updates run by this handle (host-side count, no synchronisation):
 * a sharded caller re-sums abnn_dims.global_events when it changes. */
uint64_t abnn_structural_updates(const abnn_brain* b);

/* ---- buffer-index launcher (the reference's kernel ABI) ---------------------
 * monte_carlo_traversal's 14 buffers (brain.metal:42-58, bound by
 * Brain::encode_traversal at brain.cpp:93-118) as CALLER-OWNED device memory
 * in the reference's own layouts: 16-B SynapsePacked records and u32
 * lastF / clock / budget (brain.cpp:54-60).  One call enqueues one pass of
 * schedule C1 over the first min(roundup(events,256), n_syn) records on
 * `stream`: gates, ordered budget (the first *budget spike candidates fire;
 * *budget is left at the remainder), STDP + reward + homeostasis, write-back
 * (the whole 16-B record, brain.metal:122), deferred stamps, rBar and one
 * clock tick.  The knobs the reference compiles in (#define BASE_SCALE ...,
 * brain.metal:22-31) come from `knobs` (NULL = the reference defaults; only
 * the #define fields are read -- aLTP..wMax are the buffer arguments).
 * Scratch: `workspace` of device memory (any contents on first use; reused
 * every pass: it carries the pass's adaptive partition and look-back epoch),
 * 16-B aligned: abnn_traversal_workspace_bytes(n_syn, events) is the
 * recommended size (~61 MB at config 3: a bounded pool of refractory
 * survivors, 1/64 of the visited events, plus per-1024-event counters),
 * abnn_traversal_workspace_min_bytes the least accepted (no pool).  Survivors
 * that do not fit the pool are recomputed from the records (slower, same
 * results).  The spikes are stamped after the pass's last lastF read from a
 * list of min(events, 65536) entries; a pass with more spikes than that
 * stamps the rest directly, which may land before another workgroup's lastF
 * reads (the fused pass), or (the five-launch pass) before a recomputed
 * group's when survivors also overflowed the pool -- such a pass is reported
 * by abnn_traversal_workspace_error (1); the host's kMaxSpikes = 2560,
 * brain.cpp:90, never comes near it.  This is the reference's memory
 * layout, so it streams 16 B per visited event; the pre-spike test is
 * answered from an LDS filter of lastF, which is gathered only for the ~1 %
 * of events the filter passes (the handle API's layout moves
 * 3 B per event).
 * The single-launch pass after the filter keeps one workgroup per CU resident
 * for the whole pass (its look-back waits on every other workgroup): run it
 * with the device to itself -- not beside another stream's persistent kernels
 * (a second handle's pass, RCCL) -- or select the five-launch pass
 * (ABNN_RAW_FUSED=0), and check abnn_traversal_workspace_error now and then:
 * a starved pass is not hung but reported there (2).
 * renormalise_clock_and_times (brain.metal:135-145) on the same buffers:
 * lastF[i] -= *clock for i < n_nrn, then *clock = 0 (the host decides when,
 * brain.cpp:127-128).                                                         */
typedef struct abnn_traversal_args {
    abnn_synapse* syn;          /* buffer(0)  SynapsePacked[n_syn]           rw */
    uint32_t* last_fired;       /* buffer(1)  atomic_uint lastF[n_nrn]       rw */
    uint32_t* last_visited;     /* buffer(2)  unused (brain.metal:44)           */
    uint32_t* clock;            /* buffer(3)  atomic_uint                    rw */
    uint32_t n_syn;             /* buffer(4)                                    */
    uint32_t tau_vis, tau_pre;  /* buffer(5,6) unused (brain.metal:47-48)       */
    float a_ltp, a_ltd;         /* buffer(7,8)                                  */
    float w_min, w_max;         /* buffer(9,10)                                 */
    uint32_t* budget;           /* buffer(11) atomic_uint                    rw */
    const float* reward;        /* buffer(12)                                   */
    float* rbar;                /* buffer(13) atomic_float                   rw */
    uint32_t n_nrn;             /* lastF length (src/dst >= n_nrn never pass)    */
    uint32_t events;            /* EVENTS_PER_PASS: grid roundup(events,256)    */
    const abnn_params* knobs;   /* #define knobs, NULL = reference defaults     */
    void* workspace;            /* device scratch                               */
    uint64_t workspace_bytes;
} abnn_traversal_args;
uint64_t abnn_traversal_workspace_bytes(uint32_t n_syn, uint32_t events);
uint64_t abnn_traversal_workspace_min_bytes(uint32_t n_syn, uint32_t events);
/* synchronises `stream`: 1 if any pass on this workspace since the last call
 * (or since its first launch) stamped directly where that may race (see
 * above), 2 if a pass's look-back wait gave up (never expected:
 * every workgroup of the pass is resident), else 0; the flag is sticky until
 * this call reads and clears it, so one check after many passes sees every
 * pass */
abnn_status abnn_traversal_workspace_error(const void* workspace, uint32_t* err, void* stream);
abnn_status abnn_launch_traversal(const abnn_traversal_args* a, void* stream);
abnn_status abnn_launch_renormalise(uint32_t* last_fired, uint32_t* last_visited, uint32_t* clock,
                                    uint32_t n_nrn, void* stream);

/* ---- sharded passes driven from C over RCCL ---------------------------------
 * One process per GPU (xGMI), one communicator per shard handle.  The
 * library's own RCCL communicator (RCCL = NCCL on ROCm; the one already
 * loaded in the process, e.g. by torch, else librccl.so.1): one rank calls
 * abnn_comm_unique_id, every rank gets those ABNN_COMM_ID_BYTES bytes (any
 * channel: torch.distributed broadcast, a file, MPI) and calls
 * abnn_comm_create.  abnn_shard_traverse then enqueues `passes` whole sharded
 * passes on `stream` -- per pass: abnn_shard_gate, ONE ncclAllGather of the
 * exchange records (in place, on the stream), abnn_shard_apply,
 * abnn_shard_commit -- with no host round trip except after a structural
 * update (an all-reduce of the shards' visited events for the clock-tick
 * rule, then abnn_set_global_events) and, with track_visits, the lastVisited
 * merge after every renormalisation (above).  abnn_comm_sync_visits is that
 * merge on demand (lastVisited is never read by a decision, brain.metal:44;
 * merge before reading or saving it).
 * An error on any rank (a failed launch or collective, a pass error flag)
 * leaves the other ranks inside the pass's collectives: the communicator is
 * then marked unusable (every later abnn_shard_traverse on it returns
 * ABNN_ERR_INVALID) and the caller must abort / destroy it on every rank, as
 * after any NCCL error. */
#define ABNN_COMM_ID_BYTES 128
typedef struct abnn_comm abnn_comm;
abnn_status abnn_comm_unique_id(void* id_out);
abnn_status abnn_comm_create(const void* id, uint32_t world, uint32_t rank, int device, abnn_comm** out);
abnn_status abnn_comm_destroy(abnn_comm* c);
abnn_status abnn_shard_traverse(abnn_brain* b, abnn_comm* c, uint32_t passes, void* stream);
abnn_status abnn_comm_sync_visits(abnn_brain* b, abnn_comm* c, void* stream);

/* In-process communicator group: `world` ranks in ONE process, one host
 * thread per rank, each calling abnn_shard_traverse / abnn_comm_sync_visits
 * on its own shard handle with the communicator of abnn_comm_create_local
 * (the same calls, in the same order, on every rank -- as with RCCL).  The
 * collectives are device copies and a reduction kernel on each rank's stream
 * between host barriers (no RCCL): the sharded pass at world > 1 on ONE GPU
 * (k handles share the device), or over several GPUs of one process.  Ranks
 * on one device must pass the same stream (a pass keeps one workgroup per CU
 * resident: two must not run at once); a rank that fails, or one that does
 * not reach a collective within 300 s, breaks the group and every rank's
 * next collective fails (ABNN_ERR_INVALID).  Destroy every rank's
 * communicator before the group.                                             */
typedef struct abnn_comm_group abnn_comm_group;
abnn_status abnn_comm_group_create(uint32_t world, abnn_comm_group** out);
abnn_status abnn_comm_group_destroy(abnn_comm_group* g);
abnn_status abnn_comm_create_local(abnn_comm_group* g, uint32_t rank, int device, abnn_comm** out);

/* ---- statistics / timing ---------------------------------------------------- */
abnn_status abnn_get_stats(abnn_brain* b, abnn_stats* out);   /* synchronises */
abnn_status abnn_reset_stats(abnn_brain* b);
/* every > 0: HIP events around the gate (streaming) kernel, on the stream it
 * is launched on, for every launch (every = 1) or every `every`-th launch
 * starting with the second after this call (an event pair costs stream time,
 * so sampling keeps it out of the rate; the first launch is skipped because
 * it is the one most likely to carry a transient); 0: off.
 * abnn_get_kernel_time returns the summed milliseconds and the count of timed
 * launches since the last call; abnn_get_kernel_times the same launches one by
 * one (up to `cap` of them into out_ms; *launches = how many were timed).
 * Either call resets the record.                                            */
abnn_status abnn_enable_timing(abnn_brain* b, int every);
abnn_status abnn_get_kernel_time(abnn_brain* b, double* ms_total, uint64_t* launches);
abnn_status abnn_get_kernel_times(abnn_brain* b, float* out_ms, uint64_t cap, uint64_t* launches);

/* ---- persistence ------------------------------------------------------------
 * .bnn = u32 N_SYN, u32 N_NRN, N_SYN x 16-B SynapsePacked (Brain::save/load,
 * brain.cpp:161-178).  Load of a mismatched header -> ABNN_ERR_SIZE_MISMATCH.  */
abnn_status abnn_save_bnn(abnn_brain* b, const char* path);
abnn_status abnn_load_bnn(abnn_brain* b, const char* path);
/* README §2 flat buffer: 16-B header {u32 N_SYN, u32 N_NRN, 8 B pad},
 * synapses (u32 src, u32 dst) x N_SYN, weights f32 x N_SYN,
 * lastFiredNS u64 x N_NRN, lastVisitedNS u64 x N_NRN.                         */
abnn_status abnn_save_flat(abnn_brain* b, const char* path);
abnn_status abnn_load_flat(abnn_brain* b, const char* path);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* ABNN_ABNN_H */
