"""ctypes binding of the C-ABI in include/abnn/abnn.h (libabnn_hip.so).

The library is built in-tree by ``abnn_amd.build.build_hip()`` (hipcc,
--offload-arch=gfx950).  There is no fallback: if the shared object is missing
or does not export the ABI, importing the product fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ABNN_LIB: another build of the same ABI (A/B timing of kernel variants,
# tools/ab_variants.sh); the default is the in-tree product library
LIB_PATH = os.environ.get("ABNN_LIB") or os.path.join(_HERE, "libabnn_hip.so")

SUMMARY_WORDS = 4
COMM_ID_BYTES = 128


class Dims(C.Structure):
    """abnn_dims -- Brain(nInput, nOutput, nHidden, nSynapses, eventsPerPass), brain.h:27-31."""

    _fields_ = [
        ("n_input", C.c_uint32),
        ("n_output", C.c_uint32),
        ("n_hidden", C.c_uint64),
        ("n_syn", C.c_uint64),
        ("events_per_pass", C.c_uint64),
        ("syn_offset", C.c_uint64),
        ("global_events", C.c_uint64),
        ("syn_capacity", C.c_uint64),
    ]


class Params(C.Structure):
    """abnn_params -- every knob of brain.metal:22-31, constants.h:16-19, brain.h:17-19."""

    _fields_ = [
        ("base_scale", C.c_float),
        ("refractory", C.c_uint32),
        ("window_pre", C.c_uint32),
        ("clock_inc", C.c_uint32),
        ("target_rate_hz", C.c_float),
        ("eta_home", C.c_float),
        ("eta_reward", C.c_float),
        ("alpha_rbar", C.c_float),
        ("a_ltp", C.c_float),
        ("a_ltd", C.c_float),
        ("w_min", C.c_float),
        ("w_max", C.c_float),
        ("max_spikes", C.c_uint32),
        ("tick_ns", C.c_uint32),
        ("tau_vis", C.c_uint32),
        ("tau_pre", C.c_uint32),
        ("renorm_thresh", C.c_uint64),
        ("track_visits", C.c_uint32),
        ("mode", C.c_uint32),
        ("seed", C.c_uint64),
        ("w_prune", C.c_float),
        ("p_new", C.c_float),
        ("w_init", C.c_float),
        ("compact_every", C.c_uint32),
    ]


class Scalars(C.Structure):
    _fields_ = [("clock", C.c_uint64), ("reward", C.c_float), ("rbar", C.c_float),
                ("pass_index", C.c_uint64)]


MODE_SWEEP, MODE_RANDOM = 0, 1  # abnn_params.mode (include/abnn/abnn.h)
ABI_VERSION = 10
LAYOUT_VERSION = 4


class Stats(C.Structure):
    _fields_ = [
        ("passes", C.c_uint64),
        ("events", C.c_uint64),
        ("pre_gated", C.c_uint64),
        ("post_gated", C.c_uint64),
        ("updated", C.c_uint64),
        ("fired", C.c_uint64),
        ("pruned", C.c_uint64),
        ("grown", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class State(C.Structure):
    _fields_ = [
        ("synapses", C.c_void_p),  # opaque device records (abnn_synapse_layout)
        ("last_fired", C.c_void_p),
        ("last_visited", C.c_void_p),
        ("clock", C.c_void_p),
        ("reward", C.c_void_p),
        ("rbar", C.c_void_p),
    ]


class EngineConfig(C.Structure):
    """abnn_engine_config -- abnn::EngineConfig (include/abnn/engine.hpp) plus the trace capacity."""

    _fields_ = [
        ("input_rate_hz", C.c_float), ("peak_decay", C.c_float), ("rate_alpha", C.c_float),
        ("max_observed", C.c_float),
        ("filter_tau", C.c_double), ("dt_sec", C.c_double), ("last_loss", C.c_double),
        ("use_fir", C.c_uint32), ("fir_size", C.c_uint32), ("win_size", C.c_uint32),
        ("trace_passes", C.c_uint32),
        ("teacher_seed", C.c_uint64),
    ]


class EngineState(C.Structure):
    """abnn_engine_state -- the learning driver's scalars, read back after a synchronise."""

    _fields_ = [
        ("step", C.c_uint64), ("windows", C.c_uint64), ("win_pos", C.c_uint64),
        ("teach", C.c_uint32),
        ("max_observed", C.c_float), ("last_reward", C.c_float),
        ("last_loss", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


CENSUS_MAX_BINS = 4096
CENSUS_HEADER_WORDS = 8


class CensusConfig(C.Structure):
    """abnn_census_config -- the bins and the src / dst ranges of a synapse census (count 0 = any)."""

    _fields_ = [
        ("lo", C.c_float), ("hi", C.c_float), ("bins", C.c_uint32),
        ("src_first", C.c_uint32), ("src_count", C.c_uint32),
        ("dst_first", C.c_uint32), ("dst_count", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


DEG_OUT, DEG_IN, DEG_OUT_W, DEG_IN_W = 1, 2, 4, 8
DEGREE_HEADER_WORDS = 8


class DegreeConfig(C.Structure):
    """abnn_degree_config -- the neuron range (count 0 = every neuron) and the planes of a degree census."""

    _fields_ = [
        ("first", C.c_uint32), ("count", C.c_uint32), ("what", C.c_uint32),
        ("reserved", C.c_uint32 * 5),
    ]


SELECT_ANY, SELECT_WEIGHT = 1, 2
SELECT_HEADER_WORDS = 8


class SelectConfig(C.Structure):
    """abnn_select_config -- the src / dst ranges (count 0 = not set), the weight bounds and the flags of a select."""

    _fields_ = [
        ("src_first", C.c_uint32), ("src_count", C.c_uint32),
        ("dst_first", C.c_uint32), ("dst_count", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("flags", C.c_uint32), ("reserved", C.c_uint32),
    ]


EDIT_ANY, EDIT_WEIGHT, EDIT_CLAMP = 1, 2, 4
EDIT_SET, EDIT_AFFINE, EDIT_SCALE_DST, EDIT_SCALE_SRC, EDIT_DRAW, EDIT_KILL = 0, 1, 2, 3, 4, 5
EDIT_HEADER_WORDS = 8
EDIT_KEY = 0x8CB92BA72F3D8DD7


class EditConfig(C.Structure):
    """abnn_edit_config -- a select's match fields, the op, its parameters, the clamp bounds and the DRAW seed."""

    _fields_ = [
        ("src_first", C.c_uint32), ("src_count", C.c_uint32),
        ("dst_first", C.c_uint32), ("dst_count", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("flags", C.c_uint32), ("op", C.c_uint32),
        ("a", C.c_float), ("b", C.c_float), ("c_lo", C.c_float), ("c_hi", C.c_float),
        ("seed", C.c_uint64),
        ("reserved", C.c_uint32 * 2),
    ]


REORDER_SRC, REORDER_DST, REORDER_W, REORDER_RANDOM, REORDER_NONE, REORDER_PERM = 0, 1, 2, 3, 4, 5
REORDER_DESCENDING, REORDER_ORIGIN = 1, 2
REORDER_HEADER_WORDS = 8
REORDER_SCRATCH_BYTES_PER_RECORD = 28
REORDER_KEY = 0xC2B2AE3D27D4EB4F


class ReorderConfig(C.Structure):
    """abnn_reorder_config -- the key, the flags and the RANDOM seed of a record reorder."""

    _fields_ = [
        ("key", C.c_uint32), ("flags", C.c_uint32), ("seed", C.c_uint64),
        ("reserved", C.c_uint32 * 4),
    ]


SNAP_RECORDS, SNAP_STATE = 1, 2
DIFF_MAX_BINS = 4096
DIFF_HEADER_WORDS = 24


class DiffConfig(C.Structure):
    """abnn_diff_config -- the bins over d = w_now - w_then and the src / dst ranges of a snapshot diff (count 0 = any)."""

    _fields_ = [
        ("lo", C.c_float), ("hi", C.c_float), ("bins", C.c_uint32),
        ("src_first", C.c_uint32), ("src_count", C.c_uint32),
        ("dst_first", C.c_uint32), ("dst_count", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SnapshotInfo(C.Structure):
    """abnn_snapshot_info -- a snapshot's host view: captures, n_syn and the mirrors at the last capture, its bytes."""

    _fields_ = [("captures", C.c_uint64), ("n_syn", C.c_uint64), ("scalars", Scalars), ("bytes", C.c_uint64)]


COMP_WEIGHT, COMP_SIZES = 1, 2
COMP_HEADER_WORDS = 8
COMP_SIZE_BINS = 32
COMP_NONE = 0xFFFFFFFF
COMP_BEGIN, COMP_LINK, COMP_FLATTEN, COMP_CLOSE = 0, 1, 2, 3


class ComponentsConfig(C.Structure):
    """abnn_components_config -- the neuron range, the flags and the weight bounds of a connected-components labelling."""

    _fields_ = [
        ("first", C.c_uint32), ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("reserved", C.c_uint32 * 3),
    ]


MAT_COUNT, MAT_W, MAT_P = 1, 2, 4
MAT_LABELS, MAT_WEIGHT = 1, 2
MATRIX_MAX_POPS = 64
MATRIX_HEADER_WORDS = 16


class MatrixConfig(C.Structure):
    """abnn_matrix_config -- the populations, the planes, the flags and the weight bounds of a connectivity matrix."""

    _fields_ = [
        ("pops", C.c_uint32), ("what", C.c_uint32),
        ("flags", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("reserved", C.c_uint32 * 3),
    ]


HOPS_MAX = 1024
HOPS_REVERSE, HOPS_WEIGHT = 1, 2
HOPS_HEADER_WORDS = 8
HOPS_UNREACHED = 0xFFFFFFFF
HOPS_BEGIN = 0xFFFFFFFF


class HopsConfig(C.Structure):
    """abnn_hops_config -- the seed range, the hop limit, the flags and the weight bounds of a reachability search."""

    _fields_ = [
        ("seed_first", C.c_uint32), ("seed_count", C.c_uint32),
        ("max_hops", C.c_uint32), ("flags", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("reserved", C.c_uint32 * 2),
    ]


PROP_REVERSE, PROP_FIRE_P, PROP_WEIGHT = 1, 2, 4
PROP_HEADER_WORDS = 8
PROP_TRACE_WORDS = 8
PROP_MAX_STEPS = 4096


class PropagateConfig(C.Structure):
    """abnn_propagate_config -- the in- and out-range (count 0 = every neuron), the flags and the weight bounds of a
    propagation."""

    _fields_ = [
        ("in_first", C.c_uint32), ("in_count", C.c_uint32),
        ("out_first", C.c_uint32), ("out_count", C.c_uint32),
        ("flags", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("reserved", C.c_uint32 * 5),
    ]


GRAPH_MAX_BLOCKS = 16
GRAPH_KEY = 0xD1B54A32D192ED03
TOPO_DENSE, TOPO_RANDOM, TOPO_RING = 0, 1, 2
W_UNIFORM, W_BETA = 0, 1


class GraphBlock(C.Structure):
    """abnn_graph_block -- one block of a graph spec: count, the two populations, the topology and the weight law."""

    _fields_ = [
        ("count", C.c_uint64),
        ("src_first", C.c_uint32), ("src_count", C.c_uint32),
        ("dst_first", C.c_uint32), ("dst_count", C.c_uint32),
        ("topology", C.c_uint32), ("k", C.c_uint32), ("p_rewire", C.c_float),
        ("weight_law", C.c_uint32), ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("beta_a", C.c_uint32), ("beta_b", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class GraphSpec(C.Structure):
    """abnn_graph_spec -- the seed and up to GRAPH_MAX_BLOCKS blocks laid end to end (entries past n_blocks zero)."""

    _fields_ = [
        ("seed", C.c_uint64), ("n_blocks", C.c_uint32), ("reserved", C.c_uint32),
        ("blocks", GraphBlock * GRAPH_MAX_BLOCKS),
    ]


class SpikesConfig(C.Structure):
    """abnn_spikes_config -- the spike recorder's capacities, neuron range (count 0 = every neuron) and counts switch."""

    _fields_ = [
        ("raster_capacity", C.c_uint64), ("pass_capacity", C.c_uint32),
        ("first", C.c_uint32), ("count", C.c_uint32), ("counts", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class SpikePass(C.Structure):
    """abnn_spike_pass -- one recorded pass (spikes.SPIKE_PASS_DTYPE is its numpy view)."""

    _fields_ = [
        ("pass_index", C.c_uint64), ("now", C.c_uint64), ("offset", C.c_uint64),
        ("count", C.c_uint32), ("epoch", C.c_uint32),
    ]


class SpikesInfo(C.Structure):
    """abnn_spikes_info -- the recorder's seven u64 words."""

    _fields_ = [(k, C.c_uint64) for k in ("passes_seen", "spikes_seen", "selected_seen", "passes_recorded",
                                          "spikes_recorded", "passes_dropped", "spikes_dropped")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


CORR_MAX_LAG = 256
CORR_MAX_PAIR_WORDS = 1 << 24
CORR_POP, CORR_PAIRS, CORR_SYNAPSES = 0, 1, 2
CORR_WEIGHT = 1
CORR_HEADER_WORDS = 8


class CorrConfig(C.Structure):
    """abnn_corr_config -- the two populations, the row window, the largest lag, the mode and the weight bounds."""

    _fields_ = [
        ("a_first", C.c_uint32), ("a_count", C.c_uint32), ("b_first", C.c_uint32), ("b_count", C.c_uint32),
        ("row_first", C.c_uint64), ("row_count", C.c_uint64),
        ("max_lag", C.c_uint32), ("mode", C.c_uint32), ("flags", C.c_uint32),
        ("w_lo", C.c_float), ("w_hi", C.c_float),
        ("reserved", C.c_uint32 * 3),
    ]


LAYOUT_MAX_ARRAYS = 4


class ArrayDesc(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_uint64), ("elem_bytes", C.c_uint32), ("name", C.c_char * 20)]


class Layout(C.Structure):
    """abnn_layout -- the device record layout behind abnn_state.synapses (versioned apart from the ABI)."""

    _fields_ = [("version", C.c_uint32), ("n_arrays", C.c_uint32), ("arrays", ArrayDesc * LAYOUT_MAX_ARRAYS)]


class TraversalArgs(C.Structure):
    """abnn_traversal_args -- monte_carlo_traversal's 14 buffers (brain.metal:42-58), caller-owned."""

    _fields_ = [
        ("syn", C.c_void_p), ("last_fired", C.c_void_p), ("last_visited", C.c_void_p), ("clock", C.c_void_p),
        ("n_syn", C.c_uint32), ("tau_vis", C.c_uint32), ("tau_pre", C.c_uint32),
        ("a_ltp", C.c_float), ("a_ltd", C.c_float), ("w_min", C.c_float), ("w_max", C.c_float),
        ("budget", C.c_void_p), ("reward", C.c_void_p), ("rbar", C.c_void_p),
        ("n_nrn", C.c_uint32), ("events", C.c_uint32), ("knobs", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64),
    ]


class AbnnError(RuntimeError):
    def __init__(self, fn: str, status: int, msg: str):
        super().__init__(f"{fn} failed: status {status} ({msg})")
        self.status = status


# Every symbol include/abnn/abnn.h declares: (name, restype, argtypes).
_VP, _U32, _U64, _I32, _F = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
_PU64, _PU32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SIGNATURES = [
    ("abnn_abi_version", C.c_int, []),
    ("abnn_status_string", C.c_char_p, [C.c_int]),
    ("abnn_last_error", C.c_char_p, []),
    ("abnn_default_params", None, [C.POINTER(Params)]),
    ("abnn_device_count", C.c_int, []),
    ("abnn_brain_create", C.c_int, [C.POINTER(Dims), C.POINTER(Params), C.c_int, C.POINTER(_VP)]),
    ("abnn_brain_destroy", C.c_int, [_VP]),
    ("abnn_get_dims", C.c_int, [_VP, C.POINTER(Dims)]),
    ("abnn_get_params", C.c_int, [_VP, C.POINTER(Params)]),
    ("abnn_state_ptrs", C.c_int, [_VP, C.POINTER(State)]),
    ("abnn_synapse_layout", C.c_int, [_VP, C.POINTER(Layout)]),
    ("abnn_n_neuron", C.c_uint64, [_VP]),
    ("abnn_upload_synapses", C.c_int, [_VP, _U64, _VP, _U64]),
    ("abnn_download_synapses", C.c_int, [_VP, _U64, _VP, _U64]),
    ("abnn_generate_synapses", C.c_int, [_VP, _U64]),
    ("abnn_checksum_synapses", C.c_int, [_VP, _PU64]),
    ("abnn_graph_records", C.c_uint64, [C.POINTER(GraphSpec)]),
    ("abnn_graph_fill_host", C.c_int, [C.POINTER(GraphSpec), _U64, _U64, _VP]),
    ("abnn_build_graph", C.c_int, [_VP, C.POINTER(GraphSpec)]),
    ("abnn_census_words", C.c_uint64, [C.POINTER(CensusConfig)]),
    ("abnn_census_enqueue", C.c_int, [_VP, C.POINTER(CensusConfig), _VP, _VP]),
    ("abnn_census", C.c_int, [_VP, C.POINTER(CensusConfig), _VP, _U64]),
    ("abnn_degree_words", C.c_uint64, [C.POINTER(DegreeConfig), _U64]),
    ("abnn_degree_enqueue", C.c_int, [_VP, C.POINTER(DegreeConfig), _VP, _VP]),
    ("abnn_degree", C.c_int, [_VP, C.POINTER(DegreeConfig), _VP, _U64]),
    ("abnn_select_words", C.c_uint64, [C.POINTER(SelectConfig), _U64]),
    ("abnn_select_enqueue", C.c_int, [_VP, C.POINTER(SelectConfig), _U64, _VP, _VP]),
    ("abnn_select", C.c_int, [_VP, C.POINTER(SelectConfig), _U64, _VP, _U64]),
    ("abnn_edit_words", C.c_uint64, [C.POINTER(EditConfig)]),
    ("abnn_edit_enqueue", C.c_int, [_VP, C.POINTER(EditConfig), _VP, _VP, _VP]),
    ("abnn_edit", C.c_int, [_VP, C.POINTER(EditConfig), _VP, _U64, _VP]),
    ("abnn_edit_host", C.c_int, [C.POINTER(EditConfig), _U64, _U64, _VP, _U64, _VP, _VP]),
    ("abnn_edit_factors_enqueue", C.c_int, [_VP, _VP, _U64, _F, _F, _F, _VP, _VP]),
    ("abnn_edit_factors_host", C.c_int, [_VP, _U64, _F, _F, _F, _VP]),
    ("abnn_reorder_words", C.c_uint64, [C.POINTER(ReorderConfig), _U64]),
    ("abnn_reorder_enqueue", C.c_int, [_VP, C.POINTER(ReorderConfig), _VP, _VP, _VP]),
    ("abnn_reorder", C.c_int, [_VP, C.POINTER(ReorderConfig), _VP, _VP, _U64]),
    ("abnn_reorder_release", C.c_int, [_VP]),
    ("abnn_reorder_host", C.c_int, [C.POINTER(ReorderConfig), _U64, _VP, _U64, _VP, _VP]),
    ("abnn_snapshot_create", C.c_int, [_VP, C.POINTER(_VP)]),
    ("abnn_snapshot_destroy", C.c_int, [_VP]),
    ("abnn_snapshot_get_info", C.c_int, [_VP, C.POINTER(SnapshotInfo)]),
    ("abnn_snapshot_capture_enqueue", C.c_int, [_VP, _VP, _VP]),
    ("abnn_snapshot_restore", C.c_int, [_VP, _VP, _U32]),
    ("abnn_snapshot_diff_words", C.c_uint64, [C.POINTER(DiffConfig)]),
    ("abnn_snapshot_diff_enqueue", C.c_int, [_VP, _VP, _VP, C.POINTER(DiffConfig), _VP, _VP]),
    ("abnn_snapshot_diff", C.c_int, [_VP, _VP, _VP, C.POINTER(DiffConfig), _VP, _U64]),
    ("abnn_snapshot_diff_host", C.c_int, [C.POINTER(DiffConfig), _U64, _VP, _U64, _VP, _U64, _VP]),
    ("abnn_hops_words", C.c_uint64, [C.POINTER(HopsConfig), _U64]),
    ("abnn_hops_enqueue", C.c_int, [_VP, C.POINTER(HopsConfig), _VP, _VP]),
    ("abnn_hops_step_enqueue", C.c_int, [_VP, C.POINTER(HopsConfig), C.c_uint32, _VP, _VP]),
    ("abnn_hops", C.c_int, [_VP, C.POINTER(HopsConfig), _VP, _U64]),
    ("abnn_components_words", C.c_uint64, [C.POINTER(ComponentsConfig), _U64]),
    ("abnn_components_enqueue", C.c_int, [_VP, C.POINTER(ComponentsConfig), _VP, _VP]),
    ("abnn_components_step_enqueue", C.c_int, [_VP, C.POINTER(ComponentsConfig), C.c_uint32, _VP, _VP]),
    ("abnn_components_merge_enqueue", C.c_int, [_VP, C.POINTER(ComponentsConfig), _VP, C.c_uint32, _VP, _VP]),
    ("abnn_components", C.c_int, [_VP, C.POINTER(ComponentsConfig), _VP, _U64]),
    ("abnn_components_host", C.c_int, [_VP, _U64, C.POINTER(ComponentsConfig), _U64, _VP, _U64]),
    ("abnn_matrix_words", C.c_uint64, [C.POINTER(MatrixConfig)]),
    ("abnn_matrix_enqueue", C.c_int, [_VP, C.POINTER(MatrixConfig), _VP, _VP, _VP, _VP]),
    ("abnn_matrix", C.c_int, [_VP, C.POINTER(MatrixConfig), _VP, _VP, _VP, _U64]),
    ("abnn_matrix_host", C.c_int, [_VP, _U64, C.POINTER(MatrixConfig), _VP, _VP, _U64, C.c_float, _VP, _U64]),
    ("abnn_propagate_words", C.c_uint64, [C.POINTER(PropagateConfig), _U64]),
    ("abnn_propagate_enqueue", C.c_int, [_VP, C.POINTER(PropagateConfig), _VP, _VP, _VP]),
    ("abnn_propagate", C.c_int, [_VP, C.POINTER(PropagateConfig), _VP, _VP, _U64]),
    ("abnn_propagate_rescale_enqueue", C.c_int, [_VP, C.POINTER(PropagateConfig), _VP, _VP, _VP, _VP]),
    ("abnn_propagate_iterate_enqueue", C.c_int, [_VP, C.POINTER(PropagateConfig), _U32, _VP, _VP, _VP, _VP]),
    ("abnn_propagate_host", C.c_int, [C.POINTER(PropagateConfig), _U64, _F, _VP, _U64, _VP, _VP]),
    ("abnn_propagate_rescale_host", C.c_int, [C.POINTER(PropagateConfig), _U64, _VP, _VP, _VP]),
    ("abnn_spikes_start", C.c_int, [_VP, C.POINTER(SpikesConfig)]),
    ("abnn_spikes_stop", C.c_int, [_VP]),
    ("abnn_spikes_clear", C.c_int, [_VP, C.c_int]),
    ("abnn_spikes_get_info", C.c_int, [_VP, C.POINTER(SpikesInfo)]),
    ("abnn_spikes_read_passes", C.c_int, [_VP, _U64, _U64, _VP]),
    ("abnn_spikes_read_raster", C.c_int, [_VP, _U64, _U64, _VP]),
    ("abnn_spikes_read_counts", C.c_int, [_VP, _U64, _U64, _VP]),
    ("abnn_spikes_load", C.c_int, [_VP, _VP, _U64, _VP, _U64]),
    ("abnn_corr_words", C.c_uint64, [C.POINTER(CorrConfig)]),
    ("abnn_corr_enqueue", C.c_int, [_VP, C.POINTER(CorrConfig), _VP, _VP]),
    ("abnn_corr", C.c_int, [_VP, C.POINTER(CorrConfig), _VP, _U64]),
    ("abnn_corr_host", C.c_int, [C.POINTER(CorrConfig), _U64, _VP, _U64, _VP, _U64, _VP, _U64, _VP]),
    ("abnn_get_last_fired", C.c_int, [_VP, _U64, _VP, _U64]),
    ("abnn_set_last_fired", C.c_int, [_VP, _U64, _VP, _U64]),
    ("abnn_get_last_visited", C.c_int, [_VP, _U64, _VP, _U64]),
    ("abnn_set_last_visited", C.c_int, [_VP, _U64, _VP, _U64]),
    ("abnn_set_timestamps", C.c_int, [_VP, _VP, _U64, _U64]),
    ("abnn_get_scalars", C.c_int, [_VP, C.POINTER(Scalars)]),
    ("abnn_set_scalars", C.c_int, [_VP, C.POINTER(Scalars)]),
    ("abnn_set_reward", C.c_int, [_VP, _F]),
    ("abnn_inject_inputs", C.c_int, [_VP, _VP, _U32, _F]),
    ("abnn_read_outputs", C.c_int, [_VP, _VP, _U32]),
    ("abnn_set_auto_stimulus", C.c_int, [_VP, _U64, _U64]),
    ("abnn_traverse", C.c_int, [_VP, _U32, _VP]),
    ("abnn_synchronize", C.c_int, [_VP, _VP]),
    ("abnn_default_engine_config", None, [C.POINTER(EngineConfig)]),
    ("abnn_engine_create", C.c_int, [_VP, C.POINTER(EngineConfig), C.POINTER(_VP)]),
    ("abnn_engine_destroy", C.c_int, [_VP]),
    ("abnn_engine_run", C.c_int, [_VP, _VP, _VP, _U32, _VP]),
    ("abnn_engine_get_state", C.c_int, [_VP, C.POINTER(EngineState)]),
    ("abnn_engine_get_rates", C.c_int, [_VP, _VP, _VP, _VP, _U32]),
    ("abnn_engine_read_trace", C.c_int, [_VP, _U64, _U32, _VP, _VP]),
    ("abnn_engine_set_census", C.c_int, [_VP, C.POINTER(CensusConfig), _U32, _U32]),
    ("abnn_engine_census_count", C.c_uint64, [_VP]),
    ("abnn_engine_read_census", C.c_int, [_VP, _U64, _U32, _VP, _VP]),
    ("abnn_exchange_bytes", C.c_uint64, [_VP]),
    ("abnn_set_global_events", C.c_int, [_VP, _U64]),
    ("abnn_shard_gate", C.c_int, [_VP, _VP, _VP]),
    ("abnn_shard_apply", C.c_int, [_VP, _VP, _U32, _U32, _VP]),
    ("abnn_shard_commit", C.c_int, [_VP, _VP, _U32, _VP]),
    ("abnn_get_budget", C.c_int, [_VP, _PU32]),
    ("abnn_structural_updates", C.c_uint64, [_VP]),
    ("abnn_shard_visits_delta", C.c_int, [_VP, _VP, _VP]),
    ("abnn_shard_visits_merge", C.c_int, [_VP, _VP, _VP]),
    ("abnn_renormalisations", C.c_uint64, [_VP]),
    ("abnn_traversal_workspace_bytes", C.c_uint64, [_U32, _U32]),
    ("abnn_traversal_workspace_min_bytes", C.c_uint64, [_U32, _U32]),
    ("abnn_traversal_workspace_error", C.c_int, [_VP, _PU32, _VP]),
    ("abnn_launch_traversal", C.c_int, [C.POINTER(TraversalArgs), _VP]),
    ("abnn_launch_renormalise", C.c_int, [_VP, _VP, _VP, _U32, _VP]),
    ("abnn_comm_unique_id", C.c_int, [_VP]),
    ("abnn_comm_create", C.c_int, [_VP, _U32, _U32, C.c_int, C.POINTER(_VP)]),
    ("abnn_comm_destroy", C.c_int, [_VP]),
    ("abnn_shard_traverse", C.c_int, [_VP, _VP, _U32, _VP]),
    ("abnn_comm_sync_visits", C.c_int, [_VP, _VP, _VP]),
    ("abnn_comm_group_create", C.c_int, [_U32, C.POINTER(_VP)]),
    ("abnn_comm_group_destroy", C.c_int, [_VP]),
    ("abnn_comm_create_local", C.c_int, [_VP, _U32, C.c_int, C.POINTER(_VP)]),
    ("abnn_get_stats", C.c_int, [_VP, C.POINTER(Stats)]),
    ("abnn_reset_stats", C.c_int, [_VP]),
    ("abnn_enable_timing", C.c_int, [_VP, C.c_int]),
    ("abnn_get_kernel_time", C.c_int, [_VP, C.POINTER(C.c_double), _PU64]),
    ("abnn_get_kernel_times", C.c_int, [_VP, _VP, _U64, _PU64]),
    ("abnn_save_bnn", C.c_int, [_VP, C.c_char_p]),
    ("abnn_load_bnn", C.c_int, [_VP, C.c_char_p]),
    ("abnn_save_flat", C.c_int, [_VP, C.c_char_p]),
    ("abnn_load_flat", C.c_int, [_VP, C.c_char_p]),
]

# entry points new in ABI 10: an older A/B variant build (ABNN_LIB, timing only) may lack them
ABI10_ADDITIONS = ("abnn_comm_group_create", "abnn_comm_group_destroy", "abnn_comm_create_local",
                   "abnn_default_engine_config", "abnn_engine_create", "abnn_engine_destroy", "abnn_engine_run",
                   "abnn_engine_get_state", "abnn_engine_get_rates", "abnn_engine_read_trace",
                   "abnn_census_words", "abnn_census_enqueue", "abnn_census", "abnn_engine_set_census",
                   "abnn_engine_census_count", "abnn_engine_read_census",
                   "abnn_spikes_start", "abnn_spikes_stop", "abnn_spikes_clear", "abnn_spikes_get_info",
                   "abnn_spikes_read_passes", "abnn_spikes_read_raster", "abnn_spikes_read_counts",
                   "abnn_degree_words", "abnn_degree_enqueue", "abnn_degree",
                   "abnn_select_words", "abnn_select_enqueue", "abnn_select",
                   "abnn_graph_records", "abnn_graph_fill_host", "abnn_build_graph",
                   "abnn_hops_words", "abnn_hops_enqueue", "abnn_hops_step_enqueue", "abnn_hops",
                   "abnn_edit_words", "abnn_edit_enqueue", "abnn_edit", "abnn_edit_host",
                   "abnn_edit_factors_enqueue", "abnn_edit_factors_host",
                   "abnn_snapshot_create", "abnn_snapshot_destroy", "abnn_snapshot_get_info",
                   "abnn_snapshot_capture_enqueue", "abnn_snapshot_restore", "abnn_snapshot_diff_words",
                   "abnn_snapshot_diff_enqueue", "abnn_snapshot_diff", "abnn_snapshot_diff_host",
                   "abnn_spikes_load", "abnn_corr_words", "abnn_corr_enqueue", "abnn_corr", "abnn_corr_host",
                   "abnn_reorder_words", "abnn_reorder_enqueue", "abnn_reorder", "abnn_reorder_release",
                   "abnn_reorder_host",
                   "abnn_propagate_words", "abnn_propagate_enqueue", "abnn_propagate", "abnn_propagate_rescale_enqueue",
                   "abnn_propagate_iterate_enqueue", "abnn_propagate_host", "abnn_propagate_rescale_host",
                   "abnn_components_words", "abnn_components_enqueue", "abnn_components_step_enqueue",
                   "abnn_components_merge_enqueue", "abnn_components", "abnn_components_host",
                   "abnn_matrix_words", "abnn_matrix_enqueue", "abnn_matrix", "abnn_matrix_host")

_lib = None


def _share_hip_runtime_with_torch() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  If
    this library pulled in /opt/rocm's copy first, a later `import torch` would
    load a second HIP runtime into the process and fail to see the GPU.  When
    torch is installed, preload its runtime (by path, without importing torch)
    so both resolve libamdhip64.so.7 to the same object whatever the import
    order; without torch the system ROCm runtime is used."""
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)


# diagnostics (include/abnn/abnn_debug.h, outside the stable boundary)
DEBUG_SIGNATURES = [
    ("abnn_debug_set_wave_clock", C.c_int, [_VP, C.c_int]),
    ("abnn_debug_raw_stats", C.c_int, [_VP, C.POINTER(C.c_uint64), _VP]),
    ("abnn_debug_raw_gate_timing", C.c_int, [C.c_int]),
    ("abnn_debug_raw_gate_time", C.c_int, [C.POINTER(C.c_double), _PU32]),
    ("abnn_debug_raw_fused", C.c_int, [C.c_int]),
    ("abnn_debug_raw_fused_active", C.c_int, []),
    ("abnn_debug_raw_wave_clock", C.c_int, [_VP, C.c_uint64, _U32, _U32, C.POINTER(C.c_uint64), C.c_uint64, _VP]),
    ("abnn_debug_live_allocations", C.c_uint64, []),
    ("abnn_debug_set_propagate_path", C.c_int, [_VP, C.c_int]),
    ("abnn_debug_set_components_path", C.c_int, [_VP, C.c_int]),
    ("abnn_debug_set_matrix_path", C.c_int, [_VP, C.c_int]),
    ("abnn_debug_index_state", C.c_int, [_VP, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("abnn_debug_index_mask_dirty", C.c_int, [_VP, C.POINTER(C.c_uint64)]),
    ("abnn_debug_set_indexed", C.c_int, [_VP, C.c_int]),
    ("abnn_debug_set_fused", C.c_int, [_VP, C.c_int]),
    ("abnn_debug_index_copy", C.c_int, [_VP, _PU32, C.c_uint64, _PU32, C.c_uint64]),
    ("abnn_debug_index_mask_copy", C.c_int, [_VP, _PU32, C.c_uint64, _PU32, C.c_uint64]),
    ("abnn_debug_index_delta", C.c_int, [_VP, C.POINTER(C.c_uint64)]),
]


def load() -> C.CDLL:
    """Load libabnn_hip.so (built in-tree); raise if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the traversal engine)")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SIGNATURES + DEBUG_SIGNATURES:
        if not hasattr(lib, name) and ((name, res, args) in DEBUG_SIGNATURES or
                                       (os.environ.get("ABNN_LIB") and name in ABI10_ADDITIONS)):
            continue  # an older variant build (A/B timing) without this diagnostic / entry point
        fn = getattr(lib, name)  # AttributeError = the ABI is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.abnn_abi_version()
    if got != ABI_VERSION:
        # an A/B timing build of another ABI version only with an explicit
        # opt-in: its state layout and record encoding may differ
        if not os.environ.get("ABNN_LIB_ANY_ABI"):
            raise ImportError(f"{LIB_PATH}: ABI version {got}, this binding is {ABI_VERSION} "
                              "(ABNN_LIB_ANY_ABI=1 accepts it for pass timing only)")
        import warnings

        warnings.warn(f"{LIB_PATH}: ABI version {got} != {ABI_VERSION}; use pass/timing entry points only")
    _lib = lib
    return lib


def check(fn_name: str, status: int) -> None:
    if status != 0:
        lib = load()
        msg = lib.abnn_last_error().decode(errors="replace")
        raise AbnnError(fn_name, status, msg)


def call(fn_name: str, *args) -> None:
    lib = load()
    check(fn_name, getattr(lib, fn_name)(*args))


def default_params(**overrides) -> Params:
    p = Params()
    load().abnn_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def device_count() -> int:
    return int(load().abnn_device_count())
