"""Record tests/golden/edge_phase_parent.json on an MI355X: the cases of
tests/test_gpu_edge_phase_fixture.py run with the library that ADMM_TOMO_LIB names (a build of the
commit to compare against, e.g. under variants/).

    ADMM_TOMO_LIB=variants/lib_parent.so python tests/golden/make_edge_phase_golden.py COMMIT [OUT.json]
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "distributed-inverse-problem-admm_amd"), ROOT, os.path.dirname(HERE)]

import torch  # noqa: E402

import test_gpu_edge_phase_fixture as t  # noqa: E402


def write(doc, out):
    """One case per line."""
    head = {k: v for k, v in doc.items() if k != "cases"}
    with open(out, "w") as fh:
        fh.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        fh.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in doc["cases"]))
        fh.write("\n ]\n}\n")


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else t.FIXTURE
    lib = os.environ.get("ADMM_TOMO_LIB")
    if not lib:
        raise SystemExit("set ADMM_TOMO_LIB to the library to record from")
    dev = torch.device("cuda", 0)
    doc = dict(
        recorded_from=dict(commit=commit, device=torch.cuda.get_device_name(0)),
        inputs="seeded: test_gpu_bounds._kernel_case, test_gpu_relax._edge_case, metrics_ref.phantom "
               "(test_gpu_edge_phase_fixture.run_case)",
        sums="float64 bit patterns, big-endian hex, row-major",
        cases=[dict(case=c, **t.run_case(c, dev)) for c in t.CASES])
    write(doc, out)
    print("wrote", out, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
