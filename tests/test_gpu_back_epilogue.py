"""GPU: the mirror back projector's H epilogue reads its p stencil from an LDS tile
(kernels.hpp ptile_stage / PTile; ADMM_BK_EPI=lds, the default) or by per-pixel global loads
(ADMM_BK_EPI=global), and rho D is scaled once when the batch is bound.

Only where an operand is read from differs, so the two forms agree bit for bit: checked on the
state of a node batch after one x-update and after three ADMM iterations of a ring, with one
lane block per block (ADMM_BK_STAGING=dma1, k_back_mirror) and two (dma2, k_back_mirror_2), at
the smallest shapes where the staging can go wrong (test_epilogue_forms_bitwise).  The default
build against the float64 oracle, and the re-bind that re-packs rho D (set_precisions).
"""
import networkx as nx
import numpy as np
import pytest
import torch

from admm_hip.data import make_precisions, make_sinograms, shepp_logan
from admm_hip.plan import make_plan
from admm_hip.solver import NodeBatch, make_operators
from block_6_admm_loop_ver2 import decentralized_admm
from oracle import admm as oadmm
from oracle.geometry import Geometry, joseph_matrix

pytestmark = pytest.mark.gpu

A_PER = 24  # angles per node (even: mirror mode)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _batch(N, V, Q=None, seed=7):
    """A V-ring's node batch on one GPU, 2 split-Bregman rounds x 5 CG steps per x-update."""
    ops = make_operators(N, V, A_PER * V, dtype="float32", device=0)
    ph = shepp_logan(N)
    plan = make_plan(nx.cycle_graph(V), V)
    sinos = dict(zip(plan.local_nodes, make_sinograms(ops, ph, 0.005, seed=seed)))
    if Q is None:
        _, Q = make_precisions(ops)
    nb = NodeBatch(ops[0].geom, "float32", plan, sinos, Q, 2.0, 0.02, 0.2, 2, 5, "iso", ph, 0)
    assert nb.mirror
    return nb


def _state(nb):
    torch.cuda.synchronize()
    return {k: getattr(nb, k).detach().cpu().numpy().copy()
            for k in ("x_ext", "d", "e", "y", "node_stats", "edge_stats")}


def _trajectory(N, V):
    """State after one x-update and after three ADMM iterations (x-update + consensus)."""
    nb = _batch(N, V)
    nb.node_update()
    first = _state(nb)
    nb.consensus()
    for _ in range(2):
        nb.node_update()
        nb.consensus()
    return first, _state(nb)


@pytest.mark.parametrize("staging", ["dma1", "dma2"])
@pytest.mark.parametrize("V", [4, 5, 8])
@pytest.mark.parametrize("N", [47, 64, 50, 96])
def test_epilogue_forms_bitwise(cuda, monkeypatch, N, V, staging):
    """N = 47: odd (the middle row pairs with itself), partial tiles both ways, the halo off the
    image on every side; 64: exact tiles; 50: a partial last tile, segments ending in short
    chunks; 96: a tile interior with all four neighbours in other tiles and a mirrored half not
    adjacent to the upper one.  V = 5: a one-node lane block; V = 8: two full lane blocks (dma2:
    k_back_mirror_2)."""
    monkeypatch.setenv("ADMM_FWD_MIRROR", "1")
    monkeypatch.setenv("ADMM_BK_STAGING", staging)
    out = {}
    for epi in ("lds", "global"):
        monkeypatch.setenv("ADMM_BK_EPI", epi)
        out[epi] = _trajectory(N, V)
    for when, a, b in zip(("one x-update", "three iterations"), out["lds"], out["global"]):
        assert np.all(np.isfinite(a["x_ext"])) and np.any(a["x_ext"] != 0.0), when
        for k in a:
            assert np.array_equal(a[k], b[k]), (when, k, float(np.max(np.abs(a[k] - b[k]))))


def test_default_epilogue_matches_oracle(cuda, monkeypatch):
    """The default build (LDS epilogue) against the float64 oracle at N = 47, a 4-ring: images
    and residual trajectories within 1e-5 (the bar of test_gpu_admm's C1 test)."""
    for k in ("ADMM_BK_EPI", "ADMM_BK_STAGING", "ADMM_FWD_MIRROR"):
        monkeypatch.delenv(k, raising=False)
    N, V, iters, tol = 47, 4, 4, 1e-5
    ops = make_operators(N, V, A_PER * V, dtype="float32", device=0)
    ph = shepp_logan(N)
    sinos = make_sinograms(ops, ph, 0.005, seed=1000)
    Wi, Q = make_precisions(ops)
    G = nx.cycle_graph(V)
    x, h = decentralized_admm(ops, sinos, G, Wi, Q, N, lam_tv=0.02, rho=2.0, max_iters=iters, eps_pri=0.0,
                              eps_dual=0.0, verbose=False, phantom_true=ph.numpy(), write_params=False)
    A = joseph_matrix(Geometry(N, A_PER))
    xo, ho = oadmm.decentralized_admm([A] * V, [s.double().cpu().numpy() for s in sinos], G, Q, N, lam_tv=0.02,
                                      rho=2.0, max_iters=iters, eps_pri=0.0, eps_dual=0.0,
                                      phantom_true=ph.numpy())
    errs = {"x": rel(np.stack(x), np.stack(xo)), "primal": rel(h["primal"], ho["primal"]),
            "dual": rel(h["dual"], ho["dual"])}
    print({k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < tol for v in errs.values()), errs


def _q_fn(N, V, seed):
    """Per-edge, per-pixel distinct q_ij, one q slot per incidence (what set_precisions needs)."""
    rng = np.random.default_rng(seed)
    W = [np.exp(0.5 * rng.standard_normal(N * N)) for _ in range(V)]
    fn = lambda i, j: 0.5 * (W[i] + W[j])  # noqa: E731
    fn.qslot_key = lambda i, j: ("inc", i, j)
    return fn


def test_set_precisions_rebinds_scaled_d(cuda, monkeypatch):
    """rho D is packed when a batch is bound: new q on a bound batch (set_precisions re-binds)
    must give bitwise the x-update of a batch built with that q."""
    for k in ("ADMM_BK_EPI", "ADMM_BK_STAGING", "ADMM_FWD_MIRROR"):
        monkeypatch.delenv(k, raising=False)
    N, V = 47, 4
    q1, q2 = _q_fn(N, V, 1), _q_fn(N, V, 2)
    nb = _batch(N, V, q1)
    nb.node_update()
    old = _state(nb)
    plan = nb.plan
    qs = [q2(plan.local_nodes[k], plan.inc_nbr[s]) for k in range(V)
          for s in range(plan.inc_off[k], plan.inc_off[k + 1])]
    nb.set_precisions(qs)
    nb.x_ext.zero_()
    nb.start_edges()
    nb.node_update()
    got = _state(nb)
    fresh = _batch(N, V, q2)
    fresh.node_update()
    want = _state(fresh)
    assert not np.array_equal(old["x_ext"], want["x_ext"])  # q matters
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, float(np.max(np.abs(got[k] - want[k]))))
