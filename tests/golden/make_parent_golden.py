"""Record a bitwise fixture of a parent commit on an MI355X: the cases of the named fixture test
module (test_gpu_edge_phase_fixture -> edge_phase_parent.json, test_gpu_x_update_fixture ->
x_update_parent.json) run with the library that ADMM_TOMO_LIB names (a build of the commit to
compare against, e.g. under variants/).  The module gives CASES, run_case(case, device), FIXTURE
(the file to write) and FIXTURE_NOTES (what the inputs and the stored values are).

    ADMM_TOMO_LIB=variants/lib_parent.so python tests/golden/make_parent_golden.py MODULE COMMIT [OUT.json]
"""
from __future__ import annotations

import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "distributed-inverse-problem-admm_amd"), ROOT, os.path.dirname(HERE)]

import torch  # noqa: E402


def write(doc, out):
    """One case per line."""
    head = {k: v for k, v in doc.items() if k != "cases"}
    with open(out, "w") as fh:
        fh.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        fh.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in doc["cases"]))
        fh.write("\n ]\n}\n")


def main():
    t = importlib.import_module(sys.argv[1])
    commit = sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else t.FIXTURE
    lib = os.environ.get("ADMM_TOMO_LIB")
    if not lib:
        raise SystemExit("set ADMM_TOMO_LIB to the library to record from")
    dev = torch.device("cuda", 0)
    doc = dict(
        recorded_from=dict(commit=commit, device=torch.cuda.get_device_name(0)),
        **t.FIXTURE_NOTES,
        cases=[dict(case=c, **t.run_case(c, dev)) for c in t.CASES])
    write(doc, out)
    print("wrote", out, len(doc["cases"]), "cases")


if __name__ == "__main__":
    main()
