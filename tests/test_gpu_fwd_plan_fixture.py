"""GPU: the bound batches of tests/golden/fwd_plans_parent.json (recorded from the library before
the planner left admm_tomo.hip) bind to the same plans, the same active plan, the same node-
interleave width and the same mirror flag.  Zero sinograms, no solve: binding takes
milliseconds.  The planner's tables themselves are checked on the CPU (test_fwd_plan_cpu.py).
"""
import json
import os

import networkx as nx
import pytest
import torch

from admm_hip.geometry import ParallelBeamGeometry
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_plans_parent.json")) as _fh:
    BATCHES = json.load(_fh)["batches"]


@pytest.mark.parametrize("row", BATCHES, ids=[f"N{b['N']}-a{b['angles']}-{b['dtype']}-V{b['V']}" for b in BATCHES])
def test_bound_batch_matches_fixture(cuda, monkeypatch, row):
    for k in ("ADMM_FWD_PLAN", "ADMM_FWD_CPB", "ADMM_FWD_MIRROR", "ADMM_FWD_MIRROR_XCD", "ADMM_FWD_NATURAL_ORDER"):
        monkeypatch.delenv(k, raising=False)
    geom = ParallelBeamGeometry(row["N"], row["angles"], row["det_width_factor"])
    V, dtype = row["V"], row["dtype"]
    plan = make_plan(nx.empty_graph(V), V)
    sdt = torch.float64 if dtype == "float64" else torch.float32
    sinos = {g: torch.zeros(geom.m, dtype=sdt) for g in plan.local_nodes}
    nb = NodeBatch(geom, dtype, plan, sinos, None, 2.0, 0.02, 0.2, 2, 2, "iso", None, 0)
    got = [dict(plan=p["plan"], groups=p["groups"], blocks=p["blocks"], staged_px=p["staged_px"], active=p["active"])
           for p in nb.fwd_plans()]
    want = [dict(plan=p["plan"], groups=p["groups"], blocks=p["blocks"], staged_px=float(p["staged_px"]),
                 active=p["active"]) for p in row["plans"]]
    assert got == want
    assert (nb.ctx_vb, nb.mirror) == (row["vb"], row["mirror"])
