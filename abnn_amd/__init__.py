"""abnn_amd -- MI355X-native Monte-Carlo synapse traversal engine.

The product is the HIP library ``libabnn_hip.so`` (C-ABI: include/abnn/abnn.h);
this package is its Python host mirror:

* :class:`Brain` -- the reference ``Brain`` (abnn/src/core/brain/brain.h:24-83);
* :class:`LearnEngine` -- the device-resident learning loop (``abnn_engine_*``);
* :mod:`abnn_amd.census` -- the synapse census: config, numpy reference, merge of shard results;
* :mod:`abnn_amd.degree` -- the neuron degree census: config, numpy reference, merge of shard results;
* :mod:`abnn_amd.select` -- the synapse select: config, numpy reference, merge of shard results;
* :mod:`abnn_amd.edit` -- the synapse edit: config, numpy reference, scaling factors, sum of shard headers;
* :mod:`abnn_amd.reorder` -- the record reorder: config, keys, numpy reference, the inverse of an origin;
* :mod:`abnn_amd.snapshot` -- device-side snapshots: the Snapshot object, the diff's config, numpy reference and merge;
* :mod:`abnn_amd.hops` -- reachability: config, numpy reference, the merge of shard planes between steps;
* :mod:`abnn_amd.components` -- connected components: config, numpy reference, decode, the merge of shard planes;
* :mod:`abnn_amd.matrix` -- the population connectivity matrix: config, built-in bounds, numpy reference, decode, merge of shard results;
* :mod:`abnn_amd.propagate` -- signal propagation: config, numpy reference, rescale, merge of shard results, branching ratio;
* :mod:`abnn_amd.graph` -- the graph builder: blocks, weight laws, spec, validator, numpy reference;
* :mod:`abnn_amd.spikes` -- the spike recorder: config, pass dtype, numpy reference, raster split;
* :mod:`abnn_amd.corr` -- spike correlograms: config, decode, numpy reference, merge of shard results;
* :mod:`abnn_amd.shard` -- synapse-shard data parallelism over torch.distributed;
* :mod:`abnn_amd.configs` -- the BASELINE.json workloads.
"""
from . import census, components, corr, degree, edit, graph, hops, matrix, propagate, reorder, select, snapshot, spikes
from ._lib import (AbnnError, CensusConfig, ComponentsConfig, CorrConfig, DegreeConfig, DiffConfig, EditConfig, GraphBlock, GraphSpec, HopsConfig, MatrixConfig, PropagateConfig, ReorderConfig, SelectConfig, SpikesConfig,
                   default_params, device_count,
                   load as load_library)
from .brain import SYN_DTYPE, Brain, visited_events
from .configs import CONFIGS, Workload
from .learn import LearnEngine, default_engine_config
from .snapshot import Snapshot
from .spikes import SPIKE_PASS_DTYPE

__all__ = [
    "AbnnError", "Brain", "CONFIGS", "CensusConfig", "ComponentsConfig", "CorrConfig", "DegreeConfig", "DiffConfig", "EditConfig", "GraphBlock", "GraphSpec", "HopsConfig", "LearnEngine", "MatrixConfig", "PropagateConfig", "ReorderConfig", "SPIKE_PASS_DTYPE", "SYN_DTYPE",
    "SelectConfig", "Snapshot", "SpikesConfig", "Workload", "default_engine_config", "census", "components", "corr", "default_params", "degree",
    "device_count", "edit", "graph", "hops", "load_library", "matrix", "propagate", "reorder", "select", "snapshot", "spikes", "visited_events",
]
