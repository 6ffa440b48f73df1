"""run_admm's host path -- the declared node-table layout (admm_hip/table.py) and the one recorder
(admm._Recorder, admm._flush_pipelined) -- against the histories of the commit that still had one
hand-written peeler per feature (tests/golden/history_parent.json, written by
tests/golden/make_history_golden.py from that commit): every history key, bit for bit, through the live
call and through the pipelined flush, for all 16 feature combinations with and without a phantom.
No GPU: the tables are seeded synthetic ones, the same the fixture was recorded from.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from admm_hip import admm
from admm_hip.bounds import BOUND_KEYS
from admm_hip.fuse import FUSE_KEYS
from admm_hip.penalty import NORM_KEYS, incidences
from admm_hip.table import NodeColumns
from history_hex import digest_history, encode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_history_golden", os.path.join(GOLDEN, "make_history_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)  # (its ``cases`` / ``tables`` import nothing of the package)

CASES = gen.cases()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "history_parent.json")) as f:
        return json.load(f)


def layout(m, b, n, f):
    """A layout declared as RankGroups declares it for these features, restated here with literal widths and no
    sources: RankGroups needs a device, so its own declarations are held by the GPU tests (node_stat_width in
    test_gpu_bounds / test_gpu_fuse, test_every_table_block_at_once)."""
    cols = NodeColumns()
    names = gen.METRICS if m else ()
    if b:
        cols.add("bounds", 3, None, BOUND_KEYS)
    if n:
        cols.add("norms", 3, None, NORM_KEYS)
    if f:  # (enable_fuse after enable_metrics, as run_admm calls them; the layout keeps its order regardless)
        cols.add("fuse", 2 + len(names), None, FUSE_KEYS + tuple(f"fused_{x}" for x in names))
    if m:
        cols.add("metrics", len(names), None, tuple(k for x in names for k in (f"{x}_per_node", f"{x}_mean")))
    return cols


def recorder(m, b, n, f, p):
    hist = {}
    ninc = incidences(gen.EDGES, gen.V_TOTAL, b) if n else None
    rec = admm._Recorder(hist, layout(m, b, n, f), gen.EDGES, gen.V_TOTAL, gen.LAM_TV, p, gen.METRICS if m else None,
                         ninc, gen.TOL if n else None, gen.N_PIXELS)
    return hist, rec


def test_the_fixture_holds_every_case(golden):
    assert golden["parent"] == "9521003"
    assert len(CASES) == 32 and set(golden["cases"]) == {c[0] for c in CASES}
    assert sum("pipelined" in c for c in golden["cases"].values()) == 16


@pytest.mark.parametrize("index", range(32), ids=[c[0] for c in CASES])
def test_histories_equal_the_parent_bitwise(golden, index):
    name, m, b, n, f, p = CASES[index]
    gold = golden["cases"][name]
    rows = gen.tables(index, m, b, n, f)
    hist, rec = recorder(m, b, n, f, p)
    returned = []
    for k, (ns, es, rho_k, eps_used, n_upd) in enumerate(rows):
        before = ns.copy()
        pn, dn, bres, eps = rec(k, ns, es, rho_k, eps_used, n_upd)
        returned.append([pn, dn, bres, None if eps is None else tuple(eps)])
        assert np.array_equal(ns, before)  # the recorder reads the table, it never writes it
    live = digest_history(hist)
    assert set(live) == set(gold["live"])
    for key in live:
        assert live[key] == gold["live"][key], key
    assert encode(returned) == gold["returned"]
    assert (bres is not None) == b and (eps is not None) == n
    assert ("pipelined" in gold) == (not n)
    if n:
        return
    # the pipelined flush: the same rows as one device-history block, the loop's two columns absent
    hist2, rec2 = recorder(m, b, n, f, p)
    flat = torch.from_numpy(np.stack([np.concatenate([ns.ravel(), es.ravel()]) for ns, es, *_ in rows]))
    assert admm._flush_pipelined(rec2, flat, 0, gen.ITERS, gen.RHO, False) == gen.ITERS
    piped = digest_history(hist2)
    want = gold["live"] if gold["pipelined"] == "live" else gold["pipelined"]  # ("live": the parent's were equal)
    assert set(piped) == set(want)
    for key in piped:
        assert piped[key] == want[key], key
    assert set(hist) == set(hist2)
    for key in hist:  # live == pipelined (array_equal over the stacked histories: NaN equals NaN)
        assert np.array_equal(np.asarray(hist[key]), np.asarray(hist2[key]), equal_nan=True), key
    assert all(np.isnan(e).all() for e in hist2["eps_used_history"])


@pytest.mark.parametrize("index", range(0, 32, 2), ids=[c[0][:-9] for c in CASES[::2]])
def test_layout_widths_and_views(index):
    _, m, b, n, f, _ = CASES[index]
    cols = layout(m, b, n, f)
    # RankGroups.node_stat_width before the layout was declared: 6 core columns, one per metric, 3 sums of
    # the projection, 3 norms, and the fusion's dev2 + |xbar - phantom|^2 + one per metric
    k = 2 if m else 0
    assert cols.width == 6 + k + (3 if b else 0) + (3 if n else 0) + ((1 + 1 + k) if f else 0) == gen.width(m, b, n, f)
    assert [blk.name for blk in cols.blocks] == [x for x, on in (("core", True), ("metrics", m), ("bounds", b),
                                                                 ("norms", n), ("fuse", f)) if on]
    assert cols.width_of("fuse") == ((2 + k) if f else 0)
    table = np.arange(5.0 * cols.width).reshape(5, cols.width)
    views = cols.split(table)
    assert list(views) == [blk.name for blk in cols.blocks]
    c = 0
    for blk in cols.blocks:
        v = views[blk.name]
        assert v.shape == (5, blk.width) and np.shares_memory(v, table)
        assert np.array_equal(v, table[:, c:c + blk.width])
        c += blk.width
    assert c == cols.width
    with pytest.raises(ValueError, match="columns"):
        cols.split(table[:, :-1])
    with pytest.raises(ValueError, match="columns"):
        cols.split(np.zeros((5, cols.width + 2)))


def test_core_block_alone_adds_no_device_work():
    """With no feature on a batch's rows ARE its node_stats tensor: one source, nothing to concatenate."""
    cols = NodeColumns()
    nb = type("Batch", (), {"node_stats": object()})()
    assert cols.sources(nb) == [nb.node_stats] and cols.width == 6
    assert set(cols.blocks[0].keys) == set(admm.HISTORY_KEYS + admm.EXTRA_KEYS)
