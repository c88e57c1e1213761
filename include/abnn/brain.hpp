// brain.hpp -- header-only C++ `Brain` over the C-ABI (abnn.h).
//
// Mirrors the reference host class abnn/src/core/brain/brain.h:24-83 so that a
// BrainEngine-style caller changes only what Metal forced on it (see
// INTEGRATION.md):
//   Brain(nInput, nOutput, nHidden, nSynapses, eventsPerPass)   brain.h:27-31
//   build_pipeline / build_buffers                               brain.h:35-36
//   encode_traversal                                             brain.h:39
//   inject_inputs / read_outputs                                 brain.h:40-41
//   save(ostream&) / load(istream&)                              brain.h:44-45
//   n_input() ... n_syn()                                        brain.h:48-52
//   synapse_buffer() ... budget_buffer()  (MTL::Buffer-like views) brain.h:54-58
// Errors throw std::runtime_error (the reference threw a pointer,
// brain.cpp:174); a .bnn size mismatch throws abnn::size_mismatch.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <istream>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "abnn.h"

namespace abnn {

using SynapsePacked = abnn_synapse;  // {u32 src, u32 dst, f32 w, f32 pad}, brain.h:21

static constexpr uint32_t kTickNS = 1000;             // brain.h:17
static constexpr uint32_t kMaxSpikes = 2560;          // brain.h:18
static constexpr uint32_t kRenormThresh = 4'000'000;  // brain.h:19

// NS::Range(location, length) of the reference's didModifyRange calls (ENG:52,181).
struct Range {
    uint64_t location, length;
    Range(uint64_t loc, uint64_t len) : location(loc), length(len) {}
};

struct size_mismatch : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline void check(abnn_status s, const char* what)
{
    if (s == ABNN_OK) return;
    std::string m = std::string(what) + ": " + abnn_status_string(s) + " (" + abnn_last_error() + ")";
    if (s == ABNN_ERR_SIZE_MISMATCH) throw size_mismatch(m);
    throw std::runtime_error(m);
}

// A census result (abnn.h abnn_census: ABNN_CENSUS_HEADER_WORDS + bins words).
struct Census {
    uint64_t records = 0, tombstones = 0, selected = 0, under = 0, over = 0, nan = 0;
    float min = 0.0f, max = 0.0f;  // +inf / -inf when no selected weight is a number
    std::vector<uint64_t> counts;  // the bins
    uint64_t live() const { return records - tombstones; }
    static Census from_words(const uint64_t* w, uint32_t bins)
    {
        Census c;
        c.records = w[0], c.tombstones = w[1], c.selected = w[2], c.under = w[3], c.over = w[4], c.nan = w[5];
        const uint32_t lo = (uint32_t)w[6], hi = (uint32_t)w[7];
        std::memcpy(&c.min, &lo, 4);
        std::memcpy(&c.max, &hi, 4);
        c.counts.assign(w + ABNN_CENSUS_HEADER_WORDS, w + ABNN_CENSUS_HEADER_WORDS + bins);
        return c;
    }
};

// A view of a degree census result (abnn.h abnn_degree: the header and one
// plane of `count` words per bit of `what`); it does not own the words.
struct DegreeView {
    const uint64_t* words = nullptr;
    uint32_t what = 0;
    uint64_t count = 0;  // neurons of the range
    DegreeView(const uint64_t* w, const abnn_degree_config& cfg, uint64_t n_nrn)
        : words(w), what(cfg.what), count(cfg.count ? cfg.count : n_nrn)
    {
    }
    uint64_t records() const { return words[0]; }
    uint64_t tombstones() const { return words[1]; }
    uint64_t out_total() const { return words[2]; }
    uint64_t in_total() const { return words[3]; }
    uint64_t out_skipped() const { return words[4]; }
    uint64_t in_skipped() const { return words[5]; }
    // the plane of one bit (ABNN_DEG_*): `count` words, or nullptr when it was not asked
    const uint64_t* plane(uint32_t bit) const
    {
        if (!(what & bit)) return nullptr;
        uint64_t before = 0;
        for (uint32_t b = 1; b < bit; b <<= 1) before += (what & b) ? 1 : 0;
        return words + ABNN_DEGREE_HEADER_WORDS + before * count;
    }
    const uint64_t* out() const { return plane(ABNN_DEG_OUT); }
    const uint64_t* in() const { return plane(ABNN_DEG_IN); }
    // the strength planes as two's-complement sums: strength = value / 2^24
    const int64_t* out_w() const { return reinterpret_cast<const int64_t*>(plane(ABNN_DEG_OUT_W)); }
    const int64_t* in_w() const { return reinterpret_cast<const int64_t*>(plane(ABNN_DEG_IN_W)); }
};

// A view of a select result (abnn.h abnn_select: the header, the index plane
// and the record plane of `capacity` entries each, the first written() of them
// valid); it does not own the words.
struct SelectView {
    const uint64_t* words = nullptr;
    uint64_t capacity = 0;
    SelectView(const uint64_t* w, uint64_t cap) : words(w), capacity(cap) {}
    uint64_t records() const { return words[0]; }
    uint64_t tombstones() const { return words[1]; }
    uint64_t matched() const { return words[2]; }
    uint64_t written() const { return words[3]; }
    uint64_t syn_offset() const { return words[4]; }
    // entry k < written(): the global index of the k-th match, and the record
    const uint64_t* index() const { return words + ABNN_SELECT_HEADER_WORDS; }
    const abnn_synapse* syn() const
    {
        return reinterpret_cast<const abnn_synapse*>(words + ABNN_SELECT_HEADER_WORDS + capacity);
    }
};

// A view of an edit result (abnn.h abnn_edit: ABNN_EDIT_HEADER_WORDS words);
// it does not own the words.
struct EditView {
    const uint64_t* words = nullptr;
    explicit EditView(const uint64_t* w) : words(w) {}
    uint64_t records() const { return words[0]; }
    uint64_t tombstones() const { return words[1]; }  // before the edit
    uint64_t matched() const { return words[2]; }
    uint64_t changed() const { return words[3]; }
    uint64_t killed() const { return words[4]; }
    uint64_t nonfinite() const { return words[5]; }  // non-zero: the edit stored a NaN or an inf
};

// A view of a reorder result (abnn.h abnn_reorder: the header and, with
// ABNN_REORDER_ORIGIN, the permutation as packed u32); it does not own the words.
struct ReorderView {
    const uint64_t* words = nullptr;
    explicit ReorderView(const uint64_t* w) : words(w) {}
    uint64_t records() const { return words[0]; }
    uint64_t tombstones() const { return words[1]; }  // afterwards the last ones, except under PERM
    uint64_t moved() const { return words[2]; }
    uint64_t invalid() const { return words[3]; }  // PERM: entries out of range or repeated; non-zero: nothing moved
    uint64_t syn_offset() const { return words[4]; }
    // with ABNN_REORDER_ORIGIN: the record at k is the old record origin()[k]
    const uint32_t* origin() const { return reinterpret_cast<const uint32_t*>(words + ABNN_REORDER_HEADER_WORDS); }
};

// A view of a reachability result (abnn.h abnn_hops: the header, the levels
// and the distance plane); it does not own the words.
struct HopsView {
    const uint64_t* words = nullptr;
    uint32_t max_hops = 0;
    HopsView(const uint64_t* w, const abnn_hops_config& cfg) : words(w), max_hops(cfg.max_hops) {}
    uint64_t records() const { return words[0]; }
    uint64_t neurons() const { return words[1]; }
    uint64_t reached() const { return words[2]; }
    uint64_t depth() const { return words[3]; }
    bool complete() const { return words[4] != 0; }
    // levels()[h], h = 0 .. max_hops: the neurons at distance h
    const uint64_t* levels() const { return words + ABNN_HOPS_HEADER_WORDS; }
    // dist()[n], n < neurons(): the hop distance of neuron n, ABNN_HOPS_UNREACHED = not within max_hops
    const uint32_t* dist() const
    {
        return reinterpret_cast<const uint32_t*>(words + ABNN_HOPS_HEADER_WORDS + max_hops + 1);
    }
};

// A view of a connected-components result (abnn.h abnn_components: the header,
// the bins, the label plane and, with ABNN_COMP_SIZES, the size plane); it does
// not own the words.
struct ComponentsView {
    const uint64_t* words = nullptr;
    bool has_sizes = false;
    ComponentsView(const uint64_t* w, const abnn_components_config& cfg) : words(w), has_sizes(cfg.flags & ABNN_COMP_SIZES) {}
    uint64_t records() const { return words[0]; }
    uint64_t neurons() const { return words[1]; }
    uint64_t followed() const { return words[2]; }
    uint64_t components() const { return words[3]; }
    uint64_t largest() const { return words[4]; }
    uint64_t largest_label() const { return words[5]; }
    uint64_t singletons() const { return words[6]; }
    uint64_t gave_up() const { return words[7]; }
    // bins()[j], j < ABNN_COMP_SIZE_BINS: the components whose size s has floor(log2 s) == j
    const uint64_t* bins() const { return words + ABNN_COMP_HEADER_WORDS; }
    // labels()[n], n < neurons(): the smallest neuron id of n's component, ABNN_COMP_NONE outside the range
    const uint32_t* labels() const
    {
        return reinterpret_cast<const uint32_t*>(words + ABNN_COMP_HEADER_WORDS + ABNN_COMP_SIZE_BINS);
    }
    // sizes()[n]: the size of n's component, 0 outside the range; null without ABNN_COMP_SIZES
    const uint32_t* sizes() const
    {
        return has_sizes ? labels() + 2 * ((neurons() + 1) / 2) : nullptr;
    }
};

// A view of a connectivity-matrix result (abnn.h abnn_matrix: the header, the
// sizes and one P x P plane per bit of `what`); it does not own the words.
struct MatrixView {
    const uint64_t* words = nullptr;
    uint32_t what = 0;
    MatrixView(const uint64_t* w, const abnn_matrix_config& cfg) : words(w), what(cfg.what) {}
    uint64_t records() const { return words[0]; }
    uint64_t tombstones() const { return words[1]; }
    uint64_t counted() const { return words[2]; }
    uint64_t src_unassigned() const { return words[3]; }
    uint64_t dst_unassigned() const { return words[4]; }
    uint64_t unassigned() const { return words[5]; }
    uint64_t out_of_band() const { return words[6]; }
    uint64_t skipped_w() const { return words[7]; }
    uint64_t skipped_p() const { return words[8]; }
    uint64_t pops() const { return words[9]; }
    uint64_t neurons() const { return words[10]; }
    uint64_t assigned() const { return words[11]; }
    // the neurons of population j
    uint64_t size(uint64_t j) const { return words[ABNN_MATRIX_HEADER_WORDS + j]; }
    // the plane of `bit` (one of ABNN_MAT_COUNT / W / P), P x P row-major; null when it was not asked
    const uint64_t* plane(uint32_t bit) const
    {
        if (!(what & bit)) return nullptr;
        uint64_t before = 0;
        for (uint32_t b = 1; b < bit; b <<= 1) before += (what & b) ? 1 : 0;
        return words + ABNN_MATRIX_HEADER_WORDS + pops() + before * pops() * pops();
    }
    // the records from population a to population b
    uint64_t count(uint64_t a, uint64_t b) const { return plane(ABNN_MAT_COUNT)[a * pops() + b]; }
    // their summed weight / fire probability, in 2^-24 fixed point
    int64_t weight(uint64_t a, uint64_t b) const { return (int64_t)plane(ABNN_MAT_W)[a * pops() + b]; }
    int64_t fire_p(uint64_t a, uint64_t b) const { return (int64_t)plane(ABNN_MAT_P)[a * pops() + b]; }
};

// A view of a propagation result (abnn.h abnn_propagate: the header and y); it
// does not own the words.
struct PropagateView {
    const uint64_t* words = nullptr;
    uint64_t count = 0;  // the neurons of the out-range
    PropagateView(const uint64_t* w, const abnn_propagate_config& cfg, uint64_t n_nrn)
        : words(w), count(cfg.out_count ? cfg.out_count : n_nrn) {}
    uint64_t records() const { return words[0]; }
    uint64_t tombstones() const { return words[1]; }
    uint64_t followed() const { return words[2]; }
    uint64_t skipped() const { return words[3]; }  // followed records whose coefficient is not summable
    uint64_t nonzero() const { return words[4]; }  // non-zero x in the in-range
    uint64_t sum_abs_x() const { return words[5]; }
    // y()[j], j < count: the sum for neuron out_first + j, 8 fractional bits more than x
    const int64_t* y() const { return reinterpret_cast<const int64_t*>(words + ABNN_PROP_HEADER_WORDS); }
};

// The outcome of Brain::branching: the trace (steps rows of ABNN_PROP_TRACE_WORDS
// u64, abnn.h) and the last rescaled plane.
struct Branching {
    std::vector<uint64_t> trace;
    std::vector<int32_t> x;
    size_t steps() const { return trace.size() / ABNN_PROP_TRACE_WORDS; }
    // step k's eigenvalue estimate (sum |y| / 256) / sum |x|, 0 when x was zero
    double estimate(size_t k) const
    {
        const uint64_t* r = trace.data() + k * ABNN_PROP_TRACE_WORDS;
        return r[1] ? (static_cast<double>(r[2]) / 256.0) / static_cast<double>(r[1]) : 0.0;
    }
    double ratio() const { return steps() ? estimate(steps() - 1) : 0.0; }
};

// A view of a correlogram (abnn.h abnn_corr: the header and the plane); it does
// not own the words.
struct CorrView {
    const uint64_t* words = nullptr;
    abnn_corr_config cfg{};
    CorrView(const uint64_t* w, const abnn_corr_config& c) : words(w), cfg(c) {}
    uint64_t rows() const { return words[0]; }
    uint64_t entries() const { return words[1]; }
    uint64_t in_a() const { return words[2]; }
    uint64_t in_b() const { return words[3]; }
    uint64_t total() const { return words[4]; }     // the sum of the plane
    uint64_t followed() const { return words[5]; }  // SYNAPSES
    uint64_t coupled() const { return words[6]; }
    uint64_t recorded() const { return words[7]; }  // K
    uint32_t bins() const { return 2 * cfg.max_lag + 1; }
    // POP / SYNAPSES: the pairs at lag l, -max_lag <= l <= max_lag
    uint64_t at(int64_t lag) const { return words[ABNN_CORR_HEADER_WORDS + (uint64_t)(lag + (int64_t)cfg.max_lag)]; }
    // PAIRS: the pairs (x in A, y in B) at lag l; x and y are neuron ids
    uint64_t at(uint32_t x, uint32_t y, int64_t lag) const
    {
        return words[ABNN_CORR_HEADER_WORDS + ((uint64_t)(x - cfg.a_first) * cfg.b_count + (y - cfg.b_first)) * bins() +
                     (uint64_t)(lag + (int64_t)cfg.max_lag)];
    }
};

// A view of a snapshot diff result (abnn.h abnn_snapshot_diff: the header and
// the bins over d = w_now - w_then); it does not own the words.
struct DiffView {
    const uint64_t* words = nullptr;
    uint32_t n_bins = 0;
    DiffView(const uint64_t* w, const abnn_diff_config& cfg) : words(w), n_bins(cfg.bins) {}
    uint64_t n_now() const { return words[0]; }
    uint64_t n_then() const { return words[1]; }
    uint64_t compared() const { return words[2]; }
    uint64_t born() const { return words[3]; }
    uint64_t gone() const { return words[4]; }
    uint64_t dead_both() const { return words[5]; }
    uint64_t killed() const { return words[6]; }
    uint64_t revived() const { return words[7]; }
    uint64_t rewired() const { return words[8]; }
    uint64_t paired() const { return words[9]; }
    uint64_t selected() const { return words[10]; }
    uint64_t same() const { return words[11]; }
    uint64_t changed() const { return words[12]; }
    uint64_t up() const { return words[13]; }
    uint64_t down() const { return words[14]; }
    uint64_t zero() const { return words[15]; }
    uint64_t nan() const { return words[16]; }
    uint64_t under() const { return words[17]; }
    uint64_t over() const { return words[18]; }
    int64_t net() const { return (int64_t)words[19]; }  // 2^-24 fixed point
    uint64_t abs() const { return words[20]; }
    uint64_t not_summable() const { return words[21]; }
    float max_abs() const  // the largest |d|
    {
        const uint32_t u = (uint32_t)words[22];
        float x;
        std::memcpy(&x, &u, 4);
        return x;
    }
    const uint64_t* bins() const { return words + ABNN_DIFF_HEADER_WORDS; }
};

class Brain;

// A device-side snapshot of one Brain (abnn.h abnn_snapshot_*): made by
// Brain::snapshot, destroyed before its Brain.
class Snapshot {
public:
    Snapshot(Snapshot&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Snapshot& operator=(Snapshot&& o) noexcept
    {
        if (this != &o) {
            abnn_snapshot_destroy(h_);
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    Snapshot(const Snapshot&) = delete;
    Snapshot& operator=(const Snapshot&) = delete;
    ~Snapshot() { abnn_snapshot_destroy(h_); }
    abnn_snapshot_info info() const
    {
        abnn_snapshot_info i{};
        check(abnn_snapshot_get_info(h_, &i), "abnn_snapshot_get_info");
        return i;
    }
    abnn_snapshot* handle() const { return h_; }

private:
    friend class Brain;
    explicit Snapshot(abnn_snapshot* h) : h_(h) {}
    abnn_snapshot* h_ = nullptr;
};

class Brain {
public:
    Brain(uint32_t nInput, uint32_t nOutput, uint32_t nHidden, uint32_t nSynapses,
          uint32_t eventsPerPass, int device = 0, const abnn_params* params = nullptr,
          uint64_t synCapacity = 0)  // records the handle may grow to (abnn_dims.syn_capacity; 0 = nSynapses)
    {
        abnn_dims d{};
        d.n_input = nInput;
        d.n_output = nOutput;
        d.n_hidden = nHidden;
        d.n_syn = nSynapses;
        d.events_per_pass = eventsPerPass;
        d.syn_capacity = synCapacity;
        check(abnn_brain_create(&d, params, device, &h_), "abnn_brain_create");
    }
    ~Brain() { abnn_brain_destroy(h_); }
    Brain(const Brain&) = delete;
    Brain& operator=(const Brain&) = delete;

    // brain.h:35-36.  Kernels are compiled into the library and buffers are
    // allocated (zeroed) by the constructor; build_buffers re-zeroes the state.
    void build_pipeline() {}
    void build_buffers()
    {
        touch();
        std::vector<uint64_t> z(n_neuron(), 0);
        check(abnn_set_last_fired(h_, 0, z.data(), z.size()), "abnn_set_last_fired");
        check(abnn_set_last_visited(h_, 0, z.data(), z.size()), "abnn_set_last_visited");
        abnn_scalars s{0, 0.0f, 0.0f};
        check(abnn_set_scalars(h_, &s), "abnn_set_scalars");
    }

    // One C1 pass: traversal + clock tick + renormalisation when due
    // (brain.cpp:87-141).  Enqueued on `stream` (a hipStream_t, NULL =
    // default); synchronize() is the reference's waitUntilCompleted.
    void encode_traversal(void* stream = nullptr, uint32_t passes = 1)
    {
        touch();
        check(abnn_traverse(h_, passes, stream), "abnn_traverse");
    }
    void synchronize(void* stream = nullptr) { check(abnn_synchronize(h_, stream), "abnn_synchronize"); }

    void inject_inputs(const std::vector<float>& vals, float hz)  // brain.cpp:73-83
    {
        touch();
        check(abnn_inject_inputs(h_, vals.data(), (uint32_t)vals.size(), hz), "abnn_inject_inputs");
    }
    std::vector<bool> read_outputs() const  // brain.cpp:145-157
    {
        flush_shared();
        std::vector<uint8_t> o(n_output());
        check(abnn_read_outputs(h_, o.data(), (uint32_t)o.size()), "abnn_read_outputs");
        return std::vector<bool>(o.begin(), o.end());
    }

    // .bnn persistence, byte-compatible with brain.cpp:161-178.
    void save(std::ostream& os) const
    {
        flush_shared();
        const uint32_t hdr[2] = {n_syn(), n_neuron()};
        os.write(reinterpret_cast<const char*>(hdr), sizeof(hdr));
        std::vector<SynapsePacked> buf;
        for (uint64_t i = 0; i < n_syn(); i += kPiece) {
            const uint64_t n = std::min<uint64_t>(kPiece, n_syn() - i);
            buf.resize(n);
            check(abnn_download_synapses(h_, i, buf.data(), n), "abnn_download_synapses");
            os.write(reinterpret_cast<const char*>(buf.data()), (std::streamsize)(n * sizeof(SynapsePacked)));
        }
    }
    void load(std::istream& is)
    {
        touch();
        uint32_t s = 0, n = 0;
        is.read(reinterpret_cast<char*>(&s), 4);
        is.read(reinterpret_cast<char*>(&n), 4);
        if (!(s == n_syn() && n == n_neuron())) throw size_mismatch(".bnn header does not match");
        std::vector<SynapsePacked> buf;
        for (uint64_t i = 0; i < n_syn(); i += kPiece) {
            const uint64_t k = std::min<uint64_t>(kPiece, n_syn() - i);
            buf.resize(k);
            is.read(reinterpret_cast<char*>(buf.data()), (std::streamsize)(k * sizeof(SynapsePacked)));
            if (!is) throw std::runtime_error("short .bnn body");
            check(abnn_upload_synapses(h_, i, buf.data(), k), "abnn_upload_synapses");
        }
    }

    uint32_t n_input() const { return dims().n_input; }
    uint32_t n_output() const { return dims().n_output; }
    uint32_t n_hidden() const { return (uint32_t)dims().n_hidden; }
    uint32_t n_neuron() const { return (uint32_t)abnn_n_neuron(h_); }
    uint32_t n_syn() const { return (uint32_t)dims().n_syn; }

    // The buffer getters (brain.h:54-58): host views standing in for the
    // MTL::Buffer objects, so the reference's callers keep their code:
    //   auto* syn = (SynapsePacked*)b.synapse_buffer()->contents();   ENG:37
    //   ... syn[idx++] = {...};  b.synapse_buffer()->didModifyRange(Range(0, n*16));  ENG:52
    //   uint32_t* lf = (uint32_t*)b.last_fired_buffer()->contents();  ENG:123
    //   uint32_t now = *(uint32_t*)b.clock_buffer()->contents();      ENG:124
    //   lf[nIn + o] = now;                                            ENG:131
    //   float* r = (float*)b.reward_buffer()->contents(); *r = x; didModifyRange   ENG:180-182
    // contents() is a host copy, downloaded when the device state changed
    // since it was taken.  Managed buffers (synapses, reward, budget;
    // brain.cpp:54,58-59) send host writes with didModifyRange.  Shared ones
    // (lastFired, clock; brain.cpp:55-57) need no call: the writes are sent
    // before the next device operation of this Brain (encode_traversal, ...).
    // lastFired and the clock are presented as the reference's u32 (the low
    // 32 bits of the u64 state, on which every decision is taken).  The
    // budget view reads the budget left by the last pass (writing it is an
    // error: the reference's host resets it to kMaxSpikes every pass,
    // brain.cpp:90; the knob is abnn_params.max_spikes).
    class Buffer {
    public:
        void* contents()
        {
            if (!mapped_ || version_ != owner_->version_) refresh();
            return host_.data();
        }
        uint64_t length() const { return bytes(); }
        void didModifyRange(Range r)  // Managed: upload [location, location + length)
        {
            if (!mapped_) return;
            const uint64_t es = elem_bytes(), i0 = r.location / es, i1 = (r.location + r.length + es - 1) / es;
            upload(i0, std::min<uint64_t>(i1, count()));
        }

    private:
        friend class Brain;
        enum Kind { kSynapses, kLastFired, kClock, kReward, kBudget };
        Buffer(Brain* owner, Kind k) : owner_(owner), kind_(k) {}
        uint64_t count() const
        {
            switch (kind_) {
                case kSynapses: return owner_->n_syn();
                case kLastFired: return owner_->n_neuron();
                default: return 1;
            }
        }
        uint64_t elem_bytes() const { return kind_ == kSynapses ? sizeof(SynapsePacked) : 4; }
        uint64_t bytes() const { return count() * elem_bytes(); }
        bool shared() const { return kind_ == kLastFired || kind_ == kClock; }
        void refresh()
        {
            owner_->flush_shared();
            host_.assign(bytes(), 0);
            abnn_brain* h = owner_->h_;
            switch (kind_) {
                case kSynapses:
                    for (uint64_t i = 0; i < count(); i += kPiece)
                        check(abnn_download_synapses(h, i, reinterpret_cast<SynapsePacked*>(host_.data()) + i,
                                                     std::min<uint64_t>(kPiece, count() - i)),
                              "abnn_download_synapses");
                    break;
                case kLastFired: {
                    const std::vector<uint64_t> v = owner_->last_fired();
                    uint32_t* o = reinterpret_cast<uint32_t*>(host_.data());
                    for (uint64_t i = 0; i < v.size(); ++i) o[i] = (uint32_t)v[i];
                    break;
                }
                case kClock: {
                    const uint32_t c = (uint32_t)owner_->scalars().clock;
                    std::memcpy(host_.data(), &c, 4);
                    break;
                }
                case kReward: {
                    const float r = owner_->scalars().reward;
                    std::memcpy(host_.data(), &r, 4);
                    break;
                }
                case kBudget: {
                    uint32_t left = 0;
                    check(abnn_get_budget(h, &left), "abnn_get_budget");
                    std::memcpy(host_.data(), &left, 4);
                    break;
                }
            }
            pristine_ = host_;
            mapped_ = true;
            version_ = owner_->version_;
        }
        void upload(uint64_t i0, uint64_t i1)  // elements [i0, i1) host -> device
        {
            if (i1 <= i0) return;
            abnn_brain* h = owner_->h_;
            switch (kind_) {
                case kSynapses:
                    for (uint64_t i = i0; i < i1; i += kPiece)
                        check(abnn_upload_synapses(h, i, reinterpret_cast<const SynapsePacked*>(host_.data()) + i,
                                                   std::min<uint64_t>(kPiece, i1 - i)),
                              "abnn_upload_synapses");
                    break;
                case kLastFired: {  // changed entries, grouped by value (the teacher writes one value)
                    const uint32_t* v = reinterpret_cast<const uint32_t*>(host_.data());
                    const uint32_t* p = reinterpret_cast<const uint32_t*>(pristine_.data());
                    std::vector<std::pair<uint32_t, uint32_t>> ch;
                    for (uint64_t i = i0; i < i1; ++i)
                        if (v[i] != p[i]) ch.push_back({v[i], (uint32_t)i});
                    std::sort(ch.begin(), ch.end());
                    for (size_t a = 0; a < ch.size();) {
                        size_t e = a;
                        std::vector<uint32_t> idx;
                        while (e < ch.size() && ch[e].first == ch[a].first) idx.push_back(ch[e++].second);
                        check(abnn_set_timestamps(h, idx.data(), idx.size(), ch[a].first), "abnn_set_timestamps");
                        a = e;
                    }
                    break;
                }
                case kClock: {
                    abnn_scalars sc{};
                    check(abnn_get_scalars(h, &sc), "abnn_get_scalars");
                    uint32_t c;
                    std::memcpy(&c, host_.data(), 4);
                    sc.clock = c;
                    check(abnn_set_scalars(h, &sc), "abnn_set_scalars");
                    break;
                }
                case kReward: {
                    float r;
                    std::memcpy(&r, host_.data(), 4);
                    check(abnn_set_reward(h, r), "abnn_set_reward");
                    break;
                }
                case kBudget:
                    if (std::memcmp(host_.data(), pristine_.data(), 4) != 0)
                        throw std::logic_error("budget_buffer() is read-only: the budget resets to max_spikes every "
                                               "pass (brain.cpp:90)");
                    break;
            }
            std::copy(host_.begin() + i0 * elem_bytes(), host_.begin() + i1 * elem_bytes(),
                      pristine_.begin() + i0 * elem_bytes());
            ++owner_->version_;  // the device changed: other views refresh
            version_ = owner_->version_;
        }
        Brain* owner_;
        Kind kind_;
        bool mapped_ = false;
        uint64_t version_ = 0;
        std::vector<uint8_t> host_, pristine_;
    };

    Buffer* synapse_buffer() const { return view(Buffer::kSynapses); }
    Buffer* last_fired_buffer() const { return view(Buffer::kLastFired); }
    Buffer* clock_buffer() const { return view(Buffer::kClock); }
    Buffer* reward_buffer() const { return view(Buffer::kReward); }
    Buffer* budget_buffer() const { return view(Buffer::kBudget); }

    // Borrowed device pointers (abnn_state; the synapse records are opaque).
    abnn_state device_state() const { return state(); }

    // Additions used by the engine-side driver.
    void build_random_graph(uint64_t seed = 1)  // brain-engine.cpp:31-53 recipe
    {
        touch();
        check(abnn_generate_synapses(h_, seed), "abnn_generate_synapses");
    }
    // Fill the records from a graph spec on the device (abnn_build_graph; the rule is in abnn.h).
    void build_graph(const abnn_graph_spec& spec)
    {
        touch();
        check(abnn_build_graph(h_, &spec), "abnn_build_graph");
    }
    void set_auto_stimulus(uint64_t first, uint64_t count)
    {
        check(abnn_set_auto_stimulus(h_, first, count), "abnn_set_auto_stimulus");
    }
    void set_reward(float r)
    {
        touch();
        check(abnn_set_reward(h_, r), "abnn_set_reward");
    }
    void set_timestamps(const std::vector<uint32_t>& idx, uint64_t value)
    {
        touch();
        check(abnn_set_timestamps(h_, idx.data(), idx.size(), value), "abnn_set_timestamps");
    }
    abnn_scalars scalars() const
    {
        flush_shared();
        abnn_scalars s{};
        check(abnn_get_scalars(h_, &s), "abnn_get_scalars");
        return s;
    }
    std::vector<uint64_t> last_fired() const { return last_fired(0, n_neuron()); }
    std::vector<uint64_t> last_fired(uint64_t first, uint64_t n) const
    {
        flush_shared();
        std::vector<uint64_t> v(n);
        check(abnn_get_last_fired(h_, first, v.data(), n), "abnn_get_last_fired");
        return v;
    }
    uint64_t checksum() const
    {
        uint64_t c = 0;
        check(abnn_checksum_synapses(h_, &c), "abnn_checksum_synapses");
        return c;
    }
    // Synapse census on the device (abnn_census; the definition is in abnn.h).
    Census census(const abnn_census_config& cfg) const
    {
        std::vector<uint64_t> w(abnn_census_words(&cfg) ? abnn_census_words(&cfg) : 1);
        check(abnn_census(h_, &cfg, w.data(), abnn_census_words(&cfg)), "abnn_census");
        return Census::from_words(w.data(), cfg.bins);
    }
    // Neuron degree census on the device (abnn_degree; the definition is in
    // abnn.h): the result's words, to be read through a DegreeView.
    std::vector<uint64_t> degrees(const abnn_degree_config& cfg) const
    {
        const uint64_t words = abnn_degree_words(&cfg, n_neuron());
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_degree(h_, &cfg, w.data(), words), "abnn_degree");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_degree_words(&cfg, n_neuron()) u64.
    void degrees_enqueue(const abnn_degree_config& cfg, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_degree_enqueue(h_, &cfg, out_dev, stream), "abnn_degree_enqueue");
    }
    // Synapse select on the device (abnn_select; the rule is in abnn.h): the
    // result's words for at most `capacity` matches, to be read through a
    // SelectView.  The plane entries at and past written() stay zero.
    std::vector<uint64_t> select(const abnn_select_config& cfg, uint64_t capacity) const
    {
        const uint64_t words = abnn_select_words(&cfg, capacity);
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_select(h_, &cfg, capacity, w.data(), words), "abnn_select");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_select_words(&cfg, capacity) u64.
    void select_enqueue(const abnn_select_config& cfg, uint64_t capacity, uint64_t* out_dev,
                        void* stream = nullptr) const
    {
        check(abnn_select_enqueue(h_, &cfg, capacity, out_dev, stream), "abnn_select_enqueue");
    }
    // Synapse edit on the device (abnn_edit; the rule is in abnn.h): the
    // matching records get a new weight or become tombstones; the result's 8
    // words, to be read through an EditView.  plane: the factors of a SCALE op
    // (one per neuron of its range), empty otherwise.
    std::vector<uint64_t> edit(const abnn_edit_config& cfg, const std::vector<float>& plane = {})
    {
        std::vector<uint64_t> w(ABNN_EDIT_HEADER_WORDS);
        check(abnn_edit(h_, &cfg, plane.empty() ? nullptr : plane.data(), plane.size(), w.data()), "abnn_edit");
        return w;
    }
    // Enqueue only: plane_dev (a SCALE op's factors, else null) and out_dev (8 u64) are device memory.
    void edit_enqueue(const abnn_edit_config& cfg, const float* plane_dev, uint64_t* out_dev, void* stream = nullptr)
    {
        check(abnn_edit_enqueue(h_, &cfg, plane_dev, out_dev, stream), "abnn_edit_enqueue");
    }
    // Record reorder on the device (abnn_reorder; the rule is in abnn.h): the
    // records in the stable order of cfg's key, shuffled, compacted or (perm:
    // n_syn u32) permuted; the result's words, to be read through a ReorderView.
    std::vector<uint64_t> reorder(const abnn_reorder_config& cfg, const std::vector<uint32_t>& perm = {})
    {
        abnn_dims d{};
        check(abnn_get_dims(h_, &d), "abnn_get_dims");
        const uint64_t words = abnn_reorder_words(&cfg, d.n_syn);
        std::vector<uint64_t> w(words ? words : 1);
        const bool has_perm = cfg.key == ABNN_REORDER_PERM;
        check(abnn_reorder(h_, &cfg, has_perm ? perm.data() : nullptr, w.data(), words), "abnn_reorder");
        return w;
    }
    // Enqueue only: perm_dev (PERM's n_syn u32, else null) and out_dev
    // (abnn_reorder_words(&cfg, n_syn) u64) are device memory.
    void reorder_enqueue(const abnn_reorder_config& cfg, const uint32_t* perm_dev, uint64_t* out_dev,
                         void* stream = nullptr)
    {
        check(abnn_reorder_enqueue(h_, &cfg, perm_dev, out_dev, stream), "abnn_reorder_enqueue");
    }
    // Enqueue only: `count` strength words of a degree census (device memory) into factors target / strength
    // clamped to [f_lo, f_hi] at plane_dev.
    void edit_factors_enqueue(const uint64_t* strength_dev, uint64_t count, float target, float f_lo, float f_hi,
                              float* plane_dev, void* stream = nullptr) const
    {
        check(abnn_edit_factors_enqueue(h_, strength_dev, count, target, f_lo, f_hi, plane_dev, stream),
              "abnn_edit_factors_enqueue");
    }
    // Device-side snapshots (abnn_snapshot_*; the contract is in abnn.h).
    // snapshot(): create, capture and synchronise; capture(): enqueue only.
    Snapshot snapshot(void* stream = nullptr)
    {
        flush_shared();
        abnn_snapshot* s = nullptr;
        check(abnn_snapshot_create(h_, &s), "abnn_snapshot_create");
        Snapshot snap(s);
        capture(snap, stream);
        synchronize(stream);
        return snap;
    }
    void capture(Snapshot& s, void* stream = nullptr)
    {
        flush_shared();
        check(abnn_snapshot_capture_enqueue(h_, s.handle(), stream), "abnn_snapshot_capture_enqueue");
    }
    // Roll back to the snapshot (synchronous): what = ABNN_SNAP_RECORDS | ABNN_SNAP_STATE.
    void restore(const Snapshot& s, uint32_t what = ABNN_SNAP_RECORDS | ABNN_SNAP_STATE)
    {
        touch();
        check(abnn_snapshot_restore(h_, s.handle(), what), "abnn_snapshot_restore");
    }
    // What changed since `then`: against another snapshot, or (now == nullptr)
    // this Brain's records; the result's words, to be read through a DiffView.
    std::vector<uint64_t> diff(const Snapshot& then, const abnn_diff_config& cfg, const Snapshot* now = nullptr) const
    {
        const uint64_t words = abnn_snapshot_diff_words(&cfg);
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_snapshot_diff(h_, then.handle(), now ? now->handle() : nullptr, &cfg, w.data(), words),
              "abnn_snapshot_diff");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_snapshot_diff_words(&cfg) u64.
    void diff_enqueue(const Snapshot& then, const abnn_diff_config& cfg, uint64_t* out_dev, void* stream = nullptr,
                      const Snapshot* now = nullptr) const
    {
        check(abnn_snapshot_diff_enqueue(h_, then.handle(), now ? now->handle() : nullptr, &cfg, out_dev, stream),
              "abnn_snapshot_diff_enqueue");
    }
    // Connected components on the device (abnn_components; the rule is in
    // abnn.h): the result's words, to be read through a ComponentsView.
    std::vector<uint64_t> components(const abnn_components_config& cfg) const
    {
        const uint64_t words = abnn_components_words(&cfg, n_neuron());
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_components(h_, &cfg, w.data(), words), "abnn_components");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_components_words(&cfg, n_neuron()) u64.
    void components_enqueue(const abnn_components_config& cfg, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_components_enqueue(h_, &cfg, out_dev, stream), "abnn_components_enqueue");
    }
    // One step (ABNN_COMP_BEGIN / LINK / FLATTEN / CLOSE): the sharded caller's path.
    void components_step_enqueue(const abnn_components_config& cfg, uint32_t step, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_components_step_enqueue(h_, &cfg, step, out_dev, stream), "abnn_components_step_enqueue");
    }
    // The shard merge: planes_dev holds n_planes label planes one after the other (device memory).
    void components_merge_enqueue(const abnn_components_config& cfg, const uint32_t* planes_dev, uint32_t n_planes,
                                  uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_components_merge_enqueue(h_, &cfg, planes_dev, n_planes, out_dev, stream), "abnn_components_merge_enqueue");
    }
    // Population connectivity matrix on the device (abnn_matrix; the rule is in
    // abnn.h): the result's words, to be read through a MatrixView.  bounds_host
    // (P + 1 values) or labels_dev (device memory, N_NRN u32), whichever the
    // config's LABELS flag names; the other is null.
    std::vector<uint64_t> matrix(const abnn_matrix_config& cfg, const uint32_t* bounds_host,
                                 const uint32_t* labels_dev = nullptr) const
    {
        const uint64_t words = abnn_matrix_words(&cfg);
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_matrix(h_, &cfg, bounds_host, labels_dev, w.data(), words), "abnn_matrix");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_matrix_words(&cfg) u64.
    void matrix_enqueue(const abnn_matrix_config& cfg, const uint32_t* bounds_host, const uint32_t* labels_dev,
                        uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_matrix_enqueue(h_, &cfg, bounds_host, labels_dev, out_dev, stream), "abnn_matrix_enqueue");
    }
    // Reachability on the device (abnn_hops; the rule is in abnn.h): the
    // result's words, to be read through a HopsView.
    std::vector<uint64_t> hops(const abnn_hops_config& cfg) const
    {
        const uint64_t words = abnn_hops_words(&cfg, n_neuron());
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_hops(h_, &cfg, w.data(), words), "abnn_hops");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_hops_words(&cfg, n_neuron()) u64.
    void hops_enqueue(const abnn_hops_config& cfg, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_hops_enqueue(h_, &cfg, out_dev, stream), "abnn_hops_enqueue");
    }
    // One step (ABNN_HOPS_BEGIN, or 0 .. max_hops): the sharded caller's path.
    void hops_step_enqueue(const abnn_hops_config& cfg, uint32_t step, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_hops_step_enqueue(h_, &cfg, step, out_dev, stream), "abnn_hops_step_enqueue");
    }
    // Signal propagation on the device (abnn_propagate; the rule is in abnn.h):
    // x holds n_neuron() int32; the result's words, to be read through a PropagateView.
    std::vector<uint64_t> propagate(const abnn_propagate_config& cfg, const std::vector<int32_t>& x) const
    {
        if (x.size() != n_neuron()) throw std::runtime_error("Brain::propagate: x must hold n_neuron() entries");
        const uint64_t words = abnn_propagate_words(&cfg, n_neuron());
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_propagate(h_, &cfg, x.data(), w.data(), words), "abnn_propagate");
        return w;
    }
    // Enqueue only: x_dev is device memory of n_neuron() int32 (16-byte aligned), out_dev of
    // abnn_propagate_words(&cfg, n_neuron()) u64.
    void propagate_enqueue(const abnn_propagate_config& cfg, const int32_t* x_dev, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_propagate_enqueue(h_, &cfg, x_dev, out_dev, stream), "abnn_propagate_enqueue");
    }
    // Enqueue only: the rescale of out_dev into x_dev and its trace row (8 u64 of device memory, or null).
    void propagate_rescale_enqueue(const abnn_propagate_config& cfg, const uint64_t* out_dev, int32_t* x_dev,
                                   uint64_t* trace_row_dev = nullptr, void* stream = nullptr) const
    {
        check(abnn_propagate_rescale_enqueue(h_, &cfg, out_dev, x_dev, trace_row_dev, stream),
              "abnn_propagate_rescale_enqueue");
    }
    // Enqueue only: `steps` times propagate and rescale with nothing returning to the host; trace_dev holds
    // steps x ABNN_PROP_TRACE_WORDS u64.
    void propagate_iterate_enqueue(const abnn_propagate_config& cfg, uint32_t steps, int32_t* x_dev, uint64_t* work_dev,
                                   uint64_t* trace_dev, void* stream = nullptr) const
    {
        check(abnn_propagate_iterate_enqueue(h_, &cfg, steps, x_dev, work_dev, trace_dev, stream),
              "abnn_propagate_iterate_enqueue");
    }
    // The branching ratio: `steps` power iterations of cfg (its in-range and out-range the same) from x.
    // This convenience owns no device memory: every step is the synchronous propagation and the host's
    // rescale (abnn_propagate_rescale_host: the same words as the device's); a caller with device planes
    // enqueues propagate_iterate_enqueue instead.
    Branching branching(const abnn_propagate_config& cfg, uint32_t steps, std::vector<int32_t> x) const
    {
        if (steps < 1 || steps > ABNN_PROP_MAX_STEPS || cfg.in_first != cfg.out_first || cfg.in_count != cfg.out_count)
            throw std::runtime_error("Brain::branching: steps in 1..ABNN_PROP_MAX_STEPS, in-range == out-range");
        Branching b;
        b.trace.assign(static_cast<size_t>(steps) * ABNN_PROP_TRACE_WORDS, 0);
        for (uint32_t k = 0; k < steps; ++k) {
            const std::vector<uint64_t> w = propagate(cfg, x);
            check(abnn_propagate_rescale_host(&cfg, n_neuron(), w.data(), x.data(), b.trace.data() + k * ABNN_PROP_TRACE_WORDS),
                  "abnn_propagate_rescale_host");
        }
        b.x = std::move(x);
        return b;
    }
    // The spike recorder (abnn_spikes_*; the contract is in abnn.h): from
    // record_spikes on, every pass appends its spike list to device buffers.
    void record_spikes(const abnn_spikes_config& cfg) { check(abnn_spikes_start(h_, &cfg), "abnn_spikes_start"); }
    abnn_spikes_info spikes_info() const
    {
        abnn_spikes_info i{};
        check(abnn_spikes_get_info(h_, &i), "abnn_spikes_get_info");
        return i;
    }
    // every recorded pass / the whole raster / the counts of the selected neurons
    std::vector<abnn_spike_pass> read_spike_passes() const
    {
        std::vector<abnn_spike_pass> p(spikes_info().passes_recorded);
        check(abnn_spikes_read_passes(h_, 0, p.size(), p.data()), "abnn_spikes_read_passes");
        return p;
    }
    std::vector<uint32_t> read_spike_raster(uint64_t first, uint64_t n) const
    {
        std::vector<uint32_t> r(n);
        check(abnn_spikes_read_raster(h_, first, n, r.data()), "abnn_spikes_read_raster");
        return r;
    }
    std::vector<uint32_t> read_spike_counts(uint64_t first_neuron, uint64_t n) const
    {
        std::vector<uint32_t> c(n);
        check(abnn_spikes_read_counts(h_, first_neuron, n, c.data()), "abnn_spikes_read_counts");
        return c;
    }
    void clear_spikes(bool keep_counts = false) { check(abnn_spikes_clear(h_, keep_counts ? 1 : 0), "abnn_spikes_clear"); }
    void stop_spikes() { check(abnn_spikes_stop(h_), "abnn_spikes_stop"); }
    // Replace what the recorder holds with a host pass table and its raster (abnn_spikes_load).
    void load_spikes(const std::vector<abnn_spike_pass>& passes, const std::vector<uint32_t>& raster)
    {
        check(abnn_spikes_load(h_, passes.data(), passes.size(), raster.data(), raster.size()), "abnn_spikes_load");
    }
    // A correlogram of the recorded spikes on the device (abnn_corr; the rule is
    // in abnn.h): the result's words, to be read through a CorrView.
    std::vector<uint64_t> correlate(const abnn_corr_config& cfg) const
    {
        const uint64_t words = abnn_corr_words(&cfg);
        std::vector<uint64_t> w(words ? words : 1);
        check(abnn_corr(h_, &cfg, w.data(), words), "abnn_corr");
        return w;
    }
    // Enqueue only: out_dev is device memory of abnn_corr_words(&cfg) u64.
    void correlate_enqueue(const abnn_corr_config& cfg, uint64_t* out_dev, void* stream = nullptr) const
    {
        check(abnn_corr_enqueue(h_, &cfg, out_dev, stream), "abnn_corr_enqueue");
    }
    abnn_brain* handle() const { return h_; }
    // Before a caller changes the device state through handle() (the
    // device-resident learning loop, engine.hpp): pending Shared-view writes
    // are sent first and every host view refreshes on its next contents().
    void device_state_changes() { touch(); }

private:
    static constexpr uint64_t kPiece = 1u << 20;
    abnn_dims dims() const
    {
        abnn_dims d{};
        abnn_get_dims(h_, &d);
        return d;
    }
    abnn_state state() const
    {
        abnn_state s{};
        abnn_state_ptrs(h_, &s);
        return s;
    }
    Buffer* view(int k) const
    {
        if (!views_[k]) views_[k].reset(new Buffer(const_cast<Brain*>(this), (Buffer::Kind)k));
        return views_[k].get();
    }
    // Host writes into the current Shared views (lastFired, clock) go to the
    // device before any other operation of this Brain (brain.cpp:55-57 are
    // StorageModeShared: the reference's host writes are seen by the next pass).
    // The dirty views are collected against the version seen on entry: an
    // upload bumps the version, so checking inside the loop would skip (and a
    // later contents() would overwrite) the second view's write.  After the
    // uploads every flushed view equals the device again.
    void flush_shared() const
    {
        Buffer* dirty[2];
        int n = 0;
        for (int k : {(int)Buffer::kLastFired, (int)Buffer::kClock}) {
            Buffer* v = views_[k].get();
            if (v && v->mapped_ && v->version_ == version_ && v->host_ != v->pristine_) dirty[n++] = v;
        }
        for (int i = 0; i < n; ++i) dirty[i]->upload(0, dirty[i]->count());
        for (int i = 0; i < n; ++i) dirty[i]->version_ = version_;
    }
    void touch() const  // before an operation that changes device state
    {
        flush_shared();
        ++version_;
    }
    abnn_brain* h_ = nullptr;
    mutable uint64_t version_ = 1;
    mutable std::unique_ptr<Buffer> views_[5];
};

}  // namespace abnn
