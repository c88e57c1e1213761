"""The graph builder's C++ mirror (abnn::Brain::build_graph, brain.hpp) on the
GPU: tests/cpp/graph_test.cpp builds a mixed spec on the device and compares
the download with abnn_graph_fill_host."""
import json
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_cpp_build_graph(gpu):
    from abnn_amd.build import build_graph_test

    prog = build_graph_test()
    r = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-2000:])
    res = json.loads(lines[-1])
    assert r.returncode == 0 and res["ok"], (res, r.stderr[-2000:])
    assert res["records"] == 129 + 1 + 40_001 + 30_000 + 5
