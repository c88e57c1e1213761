#!/usr/bin/env python3
"""Generate tests/golden/ref_case*.json and tests/golden/ref_driver.json from
the reference's own program text, compiled in place on the host
(oracle/ref_recipe/ -> oracle/_ref/, abnn_amd/build.py: build_reference).
Never from the oracle: these fixtures are what the oracle, and through it the
GPU passes, are pinned to.

* ref_case*.json: the cases of tests/ref_kernel_helpers.py run through
  `ref_pass` / `ref_renormalise`, in make_golden.py's per-pass format in the
  reference's layouts: SHA-256 of the 16-B records and of u32 lastF, the clock,
  the budget left, rBar's bits, a sparse sample of weight bits.
* ref_driver.json: what oracle/_ref/ref_driver prints (the reference's
  RateFilter and FunctionalDataset over the grid of tests/cpp/driver_grid.hpp).

Needs the reference checkout (ABNN_REFERENCE_DIR).

    python tests/golden/make_ref_golden.py        # rewrites the fixtures
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

DRIVER_FIXTURE = os.path.join(HERE, "ref_driver.json")


def driver_text() -> str:
    from abnn_amd.build import build_reference

    built = build_reference()
    assert built is not None, "no reference checkout (ABNN_REFERENCE_DIR) and no oracle/_ref/"
    return subprocess.run([built[1]], capture_output=True, text=True, check=True).stdout


def main():
    import ref_kernel_helpers as R
    from abnn_amd.build import build_oracle, reference_dir

    assert reference_dir() is not None, "the fixtures are made from the reference checkout (ABNN_REFERENCE_DIR)"
    build_oracle()  # the graph generator only
    for name in R.CASES:
        data = R.case_fixture(R.RefRunner, name)
        with open(R.fixture_path(name), "w") as f:
            f.write(R.fixture_text(data))
        print("wrote", name, [len(r["passes"]) for r in data["runs"]], "passes",
              [sum(r["max_spikes"] - p["budget_left"] for p in r["passes"]) for r in data["runs"]], "spikes")
    with open(DRIVER_FIXTURE, "w") as f:
        f.write(driver_text())
    print("wrote ref_driver")


if __name__ == "__main__":
    main()
