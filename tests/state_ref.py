"""Random warm ADMM states and float64 references for single kernels' worth of work.

The solver tests start every node batch from the all-zero state on one smooth phantom and judge
whole-image norms.  The helpers here start one x-update, or one consensus, from a random
non-smooth state with a distinct precision vector per incidence, so that a wrong sign, slot, row,
border or tile seam shows at the pixel it touches:

* ``host_state`` / ``random_state``: reproducible random x_ext, d, e, y, y_b, z / x_prev;
* ``precisions``: q_ij = (W_i + W_j) / 2 with random per-node, per-pixel W, one q slot per incidence;
* ``oracle_update``: oracle.node_solver.node_update of every local node of a plan from such a
  state (float64, or the float32 emulation that is the float32 yardstick);
* ``consensus_ref``: the edge update in the kernels' operation order, statistics by math.fsum;
* ``field_err`` / ``stat_cols`` / ``yardstick``: the per-pixel and per-statistic measures and the
  float32 rounding yardstick (float64 oracle against its own float32 emulation);
* ``UPDATE_CASES`` / ``REUSE_CASES``: the x-update cases of test_gpu_state_update.py, kept here so
  that test_state_ref_cpu.py checks their conditions on the oracle without a GPU.
"""
from __future__ import annotations

import math
from collections import namedtuple

import networkx as nx
import numpy as np

import free_geom
from oracle import node_solver as ons
from oracle import tv as otv
from oracle.geometry import Geometry, joseph_matrix, shepp_logan

STAT_NAMES = ("MSE_SINO", "sqrt(G2)", "TV", "QUAD", "IMG", "sqrt(SBRES2)")  # node_stats column order
F64_BAR = 1e-9      # float64 samples against the float64 oracle
F32_FACTOR = 4.0    # float32 samples: device error <= 4 x the emulation's (the yardstick)
RHO, LAM, MU = 2.0, 0.5, 0.5  # tau = lam / mu = 1: shrink is active on about half of the random pixels


# --------------------------------------------------------------------------------------
# problems and states
# --------------------------------------------------------------------------------------
def graph_of(kind: str, V: int):
    """ring: both incidence signs at every node; star: node 0 with V - 1 incidences; path: end
    nodes with one; none: no edges (a one-node ring would be a self loop)."""
    if kind == "ring":
        return nx.cycle_graph(V)
    if kind == "star":
        return nx.star_graph(V - 1)
    if kind == "path":
        return nx.path_graph(V)
    if kind == "none":
        return nx.empty_graph(V)
    if kind == "complete":
        return nx.complete_graph(V)
    raise ValueError(kind)


def precisions(n: int, n_nodes: int, seed: int):
    """(W, q_fn): W[g] random per node and pixel, q_fn(i, j) = (W_i + W_j) / 2 with a qslot_key
    that gives every incidence its own slot."""
    rng = np.random.default_rng([seed, 77])
    W = [np.exp(0.5 * rng.standard_normal(n)) for _ in range(n_nodes)]
    fn = lambda i, j: 0.5 * (W[i] + W[j])  # noqa: E731
    fn.qslot_key = lambda i, j: ("inc", i, j)
    return W, fn


def sinograms(A, N: int, nodes, seed: int, dtype: str):
    """{g: b_g}: noisy projections of the phantom (rounded to float32 for float32 samples, so the
    device and the oracle read the same numbers), and the phantom."""
    rng = np.random.default_rng([seed, 99])
    ph = shepp_logan(N).reshape(-1).astype(np.float64)
    clean = A @ ph
    out = {}
    for g in nodes:
        b = clean + 0.05 * rng.standard_normal(clean.shape)
        out[g] = b.astype(np.float32).astype(np.float64) if dtype == "float32" else b
    return out, ph


def host_state(plan, n: int, seed: int, fusion: str = "midpoint", derive_z: bool = False, x_ext=None):
    """Random state of a batch on ``plan`` as float64 arrays (shapes as NodeBatch's tensors).
    ``x_ext``: keep these images (the ADMM_BATCH_KEEP_X contract) and randomise the rest."""
    rng = np.random.default_rng([seed, 11])
    E = max(len(plan.stored_edges), 1)
    st = {}
    x = rng.standard_normal((plan.n_xext, n))
    st["x_ext"] = x if x_ext is None else np.array(x_ext, dtype=np.float64)
    st["d"] = 0.3 * rng.standard_normal((plan.V, 2, n))
    st["e"] = 0.3 * rng.standard_normal((plan.V, 2, n))
    # Where a forward difference is identically zero (gx on the last row, gy on the last column)
    # u = e for ever: a large e there would be clamped to +-tau by the first round and sit on the
    # shrink threshold from the second on.  Real runs keep it 0; here it stays small (d stays
    # random: no kernel may read it there).
    N = int(round(math.sqrt(n)))
    ev = st["e"].reshape(plan.V, 2, N, N)
    ev[:, 0, N - 1, :] *= 1.0 / 3.0
    ev[:, 1, :, N - 1] *= 1.0 / 3.0
    st["y"] = 0.5 * rng.standard_normal((E, n))
    st["y_b"] = 0.5 * rng.standard_normal((E, n)) if fusion == "weighted" else None
    st["z"] = None if derive_z else rng.standard_normal((E, n))  # not the midpoint of anything
    st["x_prev"] = rng.standard_normal((plan.n_xext, n)) if derive_z else None
    return st


def random_state(nb, seed: int, keep_x: bool = False):
    """Fill the bound NodeBatch ``nb`` in place with ``host_state`` (halo rows included);
    ``keep_x``: every field but x_ext.  Returns the host float64 copies."""
    import torch
    torch.cuda.synchronize()
    x = nb.x_ext.detach().cpu().numpy() if keep_x else None
    st = host_state(nb.plan, nb.geom.n, seed, nb.fusion, nb.derive_z, x_ext=x)
    for k, v in st.items():
        t = getattr(nb, k)
        assert (t is None) == (v is None), k
        if v is not None and not (keep_x and k == "x_ext"):
            assert tuple(t.shape) == v.shape, (k, tuple(t.shape), v.shape)
            t.copy_(torch.from_numpy(v))
    torch.cuda.synchronize()
    return st


def z_of(st, plan, k: int):
    """z of stored edge slot k: the stored vector or the midpoint of the x_prev rows."""
    if st["z"] is not None:
        return st["z"][k]
    return (st["x_prev"][plan.edge_a_row[k]] + st["x_prev"][plan.edge_b_row[k]]) * 0.5


# --------------------------------------------------------------------------------------
# x-update
# --------------------------------------------------------------------------------------
def oracle_update(host_state, plan, A, b, q_fn, params, fusion, dtype=np.float64, phantom=None):
    """One oracle x-update of every local node from ``host_state`` (not modified).
    v_ij = z_ij - y_ij,i with y_ij,i = y at the lower endpoint and -y (midpoint) or y_b (weighted)
    at the higher.  Returns {x (V, n), d, e (V, 2, n), stats (V, 6)} in float64, the statistics in
    node_stats' column order (G2 and SBRES2 squared, IMG = |x - phantom|^2)."""
    st = host_state
    n = st["x_ext"].shape[1]
    N = int(round(math.sqrt(n)))
    V = plan.V
    AT = A.T.tocsr()
    out = {"x": np.zeros((V, n)), "d": np.zeros((V, 2, n)), "e": np.zeros((V, 2, n)),
           "stats": np.zeros((V, 6))}
    for k, g in enumerate(plan.local_nodes):
        qv = []
        for s in range(plan.inc_off[k], plan.inc_off[k + 1]):
            e = plan.inc_edge[s]
            if plan.inc_sign[s] > 0:
                yi = st["y"][e]
            else:
                yi = st["y_b"][e] if fusion == "weighted" else -st["y"][e]
            qv.append((np.asarray(q_fn(g, plan.inc_nbr[s]), dtype=np.float64), z_of(st, plan, e) - yi))
        D, c = ons.assemble(qv, n)
        cast = lambda v: np.array(v, dtype=dtype)  # noqa: E731
        ns = ons.NodeState(cast(st["x_ext"][k]), cast(st["d"][k, 0]), cast(st["d"][k, 1]),
                           cast(st["e"][k, 0]), cast(st["e"][k, 1]))
        bg = np.asarray(b[g], dtype=np.float64).reshape(-1)
        dg = ons.node_update(A, AT @ bg, bg, D, c, qv, ns, N, params, dtype=dtype, AT=AT)
        x = ns.x.astype(np.float64)
        out["x"][k] = x
        out["d"][k, 0], out["d"][k, 1] = ns.dx, ns.dy
        out["e"][k, 0], out["e"][k, 1] = ns.ex, ns.ey
        img = float(np.sum((x - phantom) ** 2)) if phantom is not None else np.nan
        out["stats"][k] = (dg.mse_sino, dg.g_norm ** 2, dg.tv, dg.quad, img, dg.sb_res ** 2)
    return out


def as_f32_matrix(A):
    """The Joseph matrix with its stored values rounded to float32 (products with float32
    vectors then accumulate in float32): the operator of the float32 emulation."""
    return A.astype(np.float32)


def continue_state(st, upd, **new):
    """The state after an oracle update ``upd`` of ``st``: its x, d, e with the rest of ``st``,
    overridden by ``new``."""
    out = dict(st)
    x = np.array(st["x_ext"])
    x[: upd["x"].shape[0]] = upd["x"]
    out.update(x_ext=x, d=upd["d"], e=upd["e"])
    out.update(new)
    return out


def rerandomised(plan, n: int, case):
    """The second random draw of a start-reuse case: every field but x_ext (what
    ``random_state(nb, case.seed + 1000, keep_x=True)`` writes)."""
    st = host_state(plan, n, case.seed + 1000, case.fusion, case.derive_z)
    del st["x_ext"]
    return st


def field_err(got, want):
    """(max |got - want| / max |want|, index of the worst entry) of one field."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    at = np.unravel_index(int(np.argmax(diff)), diff.shape)
    return float(diff[at] / max(float(np.max(np.abs(want))), 1e-300)), tuple(int(i) for i in at)


def stat_cols(stats):
    """(V, 6) node_stats -> the compared quantities STAT_NAMES: G2 and SBRES2 as norms."""
    s = np.array(stats, dtype=np.float64)
    s[:, 1] = np.sqrt(s[:, 1])
    s[:, 5] = np.sqrt(s[:, 5])
    return s


def stat_err(got, want):
    """(V, 6) relative errors of the statistics, each on its own."""
    g, w = stat_cols(got), stat_cols(want)
    return np.abs(g - w) / np.maximum(np.abs(w), 1e-300)


def yardstick(ref, emu):
    """The float32 rounding yardstick of one case: how far the float64 oracle ``ref`` lies from
    its own float32 emulation ``emu`` -- per field relative to the field's max-abs, per statistic
    column the largest relative error over the nodes."""
    y = {k: field_err(emu[k], ref[k])[0] for k in ("x", "d", "e")}
    y["stats"] = stat_err(emu["stats"], ref["stats"]).max(axis=0)
    return y


def conditions(upd, N: int, tv_kind: str, tau: float):
    """(gmin, umargin) of an oracle update: the smallest |Kx| (iso; aniso: the smallest |gx| or
    |gy|) where the forward differences exist, and the smallest distance of the final
    u = Kx + e_old = d' + e' from the shrink threshold (iso: ||u| - tau|; aniso: ||u_c| - tau|)."""
    gmin, um = np.inf, np.inf
    for k in range(upd["x"].shape[0]):
        gx, gy = otv.grad(upd["x"][k], N)
        gx, gy = gx.reshape(N, N)[:-1, :-1], gy.reshape(N, N)[:-1, :-1]
        ux, uy = upd["d"][k, 0] + upd["e"][k, 0], upd["d"][k, 1] + upd["e"][k, 1]
        if tv_kind == "iso":
            gmin = min(gmin, float(np.min(np.sqrt(gx * gx + gy * gy))))
            um = min(um, float(np.min(np.abs(np.sqrt(ux * ux + uy * uy) - tau))))
        else:
            gmin = min(gmin, float(np.min(np.abs(gx))), float(np.min(np.abs(gy))))
            um = min(um, float(np.min(np.abs(np.abs(ux) - tau))), float(np.min(np.abs(np.abs(uy) - tau))))
    return gmin, um


# --------------------------------------------------------------------------------------
# consensus
# --------------------------------------------------------------------------------------
def consensus_ref(x, y, y_b, z_old, w, edges, fusion):
    """One edge update in float64 in the kernels' operation order.  ``edges``: (row_a, row_b) of
    x per edge slot; ``fusion``: "midpoint" (stored z: z' = ((x_a + y) + (x_b - y)) * 0.5),
    "derived" (z' = (x_a + x_b) * 0.5; ``z_old``: the midpoints of the old x_prev rows) or
    "weighted" (z' = (W_a (x_a + y) + W_b (x_b + y_b)) / (W_a + W_b), y_b' = y_b + x_b - z').
    y' = y + x_a - z'.  Returns z', y', y_b' (or None) and the (E, 3) statistics
    |x_a - z'|^2, |x_b - z'|^2, |z' - z_old|^2 summed with math.fsum."""
    E = len(edges)
    zn, yn = np.zeros((E, x.shape[1])), np.zeros((E, x.shape[1]))
    ybn = np.zeros_like(zn) if fusion == "weighted" else None
    stats = np.zeros((E, 3))
    for k, (a, b) in enumerate(edges):
        xa, xb = x[a], x[b]
        if fusion == "midpoint":
            z = ((xa + y[k]) + (xb - y[k])) * 0.5
        elif fusion == "derived":
            z = (xa + xb) * 0.5
        elif fusion == "weighted":
            z = (w[a] * (xa + y[k]) + w[b] * (xb + y_b[k])) / (w[a] + w[b])
            ybn[k] = y_b[k] + xb - z
        else:
            raise ValueError(fusion)
        zn[k] = z
        yn[k] = y[k] + xa - z
        for c, v in enumerate((xa - z, xb - z, z - z_old[k])):
            stats[k, c] = math.fsum(v * v)
    return zn, yn, ybn, stats


def ulps(got, want):
    """|got - want| in units of the spacing of ``want``, elementwise."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


# --------------------------------------------------------------------------------------
# the x-update cases
# --------------------------------------------------------------------------------------
# geom: None (the standard geometry of N and a_per) or the id of a free geometry (free_geom.BY_ID)
Case = namedtuple("Case", "N V graph tv_iters cg_iters tv_kind a_per mirror fusion derive_z seed geom",
                  defaults=(None,))


def _c(N, V, graph, iters, kind, a_per, mirror, edge, seed=1):
    fusion = "weighted" if edge == "weighted" else "midpoint"
    return Case(N, V, graph, iters[0], iters[1], kind, a_per, mirror, fusion, edge == "derived", seed)


def _f(geom, V, graph, iters, mirror, edge, seed=1):
    """A case on the free geometry ``geom`` (isotropic TV)."""
    g = free_geom.BY_ID[geom]
    return _c(g.N, V, graph, iters, "iso", g.n_angles, mirror, edge, seed)._replace(geom=geom)


# mirror: ADMM_FWD_MIRROR ("1" / "0"; None: an odd angle count, which cannot mirror).
# Every N, V, graph, (tv_iters, cg_iters), tv_kind, angle form and edge state appears, and each
# case runs with float32 and float64 samples.  The seeds are those at which the conditions of
# ``conditions`` hold (test_state_ref_cpu.py).  The anisotropic cases are few, small and of one
# round: min(|gx|, |gy|) >= 1e-3 over every pixel of every node holds at about one seed in a
# hundred after one round of up to five CG steps, and at none of 3000 seeds tried after two rounds,
# which smooth x (the anisotropic shrink of the later rounds is covered by the exact-shrink test's
# arithmetic and by the isotropic cases' round sequencing).
UPDATE_CASES = [
    _c(33, 1, "none", (1, 1), "iso", 12, "1", "stored"),
    _c(33, 3, "path", (1, 5), "aniso", 12, "1", "stored", seed=131),
    _c(33, 3, "ring", (1, 1), "aniso", 9, None, "weighted", seed=582),
    _c(33, 5, "star", (3, 2), "iso", 24, "0", "derived"),
    _c(33, 8, "ring", (4, 3), "iso", 12, "1", "weighted"),
    _c(33, 11, "ring", (2, 9), "iso", 12, "0", "stored"),
    _c(47, 1, "none", (2, 9), "iso", 24, "1", "stored"),
    _c(47, 3, "ring", (3, 2), "iso", 9, None, "derived"),
    _c(47, 4, "ring", (1, 1), "iso", 24, "1", "derived"),
    _c(47, 5, "star", (1, 5), "iso", 12, "0", "weighted"),
    _c(47, 8, "ring", (2, 3), "iso", 24, "1", "stored"),
    _c(47, 11, "ring", (4, 3), "iso", 12, "1", "derived"),
    _c(64, 3, "path", (3, 2), "iso", 24, "1", "derived"),
    _c(64, 4, "ring", (2, 3), "iso", 24, "0", "stored"),
    _c(64, 5, "ring", (4, 3), "iso", 12, "1", "weighted"),
    _c(64, 8, "ring", (1, 1), "iso", 9, None, "stored"),
    _c(65, 3, "ring", (1, 5), "iso", 24, "1", "stored"),
    _c(65, 4, "ring", (2, 9), "iso", 12, "0", "derived"),
    _c(65, 5, "star", (2, 3), "iso", 24, "1", "stored"),
    _c(65, 8, "ring", (4, 3), "iso", 24, "1", "derived"),
    _c(65, 11, "ring", (3, 2), "iso", 9, None, "weighted"),
]
# the start-reuse cases (ADMM_BATCH_KEEP_X): two x-updates, the second from k_start_reuse
REUSE_CASES = [
    _c(33, 3, "ring", (2, 3), "iso", 12, "1", "stored"),
    _c(33, 8, "ring", (2, 3), "iso", 24, "0", "derived"),
    _c(65, 3, "path", (2, 3), "iso", 9, None, "weighted"),
    _c(65, 8, "ring", (2, 3), "iso", 24, "1", "stored"),
]
# a batch with halo rows: rank 0 of 2 of an 8-ring (nodes 0-3, halo images of nodes 4 and 7)
HALO_CASE = _c(33, 4, "ring", (2, 3), "iso", 12, "1", "derived", seed=2)
GMIN, UMARGIN = 1e-3, 1e-6  # the conditions' bars
# x-updates on the free geometries (tests/free_geom.py; test_gpu_free_geom_update.py): n_det != N
# with mirror mode on and off, an asymmetric detector, the full circle, odd counts, more than one
# tile and ray chunk, and the geometry the grouped forward kernel does not fit (k_fwd; 1 x 2 inner
# iterations keep its 256^2 oracle short).  mirror None: the mode the library picks (none of
# those geometries is mirror-eligible or has a grouped plan).
FREE_UPDATE_CASES = [
    _f("wide", 5, "ring", (2, 3), "1", "derived"),
    _f("wide", 5, "ring", (2, 3), "0", "derived"),
    _f("coarse", 2, "path", (3, 2), "1", "stored"),
    _f("shifted", 3, "ring", (2, 3), None, "weighted"),
    _f("circle", 4, "ring", (1, 5), None, "stored"),
    _f("odd", 3, "ring", (4, 3), None, "derived"),
    _f("tiles", 2, "path", (2, 3), None, "stored"),
    _f("nofit", 2, "path", (1, 2), None, "stored"),
    _f("nofit", 5, "ring", (1, 2), None, "weighted"),
]
# the detector that misses the image (A = 0) under every forced forward plan (test_gpu_free_geom.py)
MISSED_CASE = _f("missed", 3, "ring", (2, 3), None, "stored")


def case_id(c: Case) -> str:
    edge = "weighted" if c.fusion == "weighted" else ("derived" if c.derive_z else "stored")
    return ((c.geom + "-") if c.geom else "") + \
        f"N{c.N}-V{c.V}-{c.graph}-{c.tv_iters}x{c.cg_iters}-{c.tv_kind}-a{c.a_per}m{c.mirror}-{edge}"


def case_matrix(c: Case):
    """The float64 Joseph matrix of a case's geometry."""
    return joseph_matrix(free_geom.BY_ID[c.geom].oracle() if c.geom else Geometry(c.N, c.a_per))


def case_problem(c: Case, dtype: str):
    """Everything of a case that needs no GPU: plan, matrix, sinograms, phantom, W, q_fn, params."""
    from admm_hip.plan import make_plan
    n = c.N * c.N
    plan = make_plan(graph_of(c.graph, c.V), c.V)
    A = case_matrix(c)
    b, ph = sinograms(A, c.N, plan.local_nodes, c.seed, dtype)
    W, q_fn = precisions(n, c.V, c.seed)
    prm = ons.NodeParams(rho=RHO, lam=LAM, mu=MU, tv_iters=c.tv_iters, cg_iters=c.cg_iters, tv_kind=c.tv_kind)
    return dict(plan=plan, A=A, b=b, ph=ph, W=W, q_fn=q_fn, prm=prm, n=n)


def halo_problem(dtype: str):
    """HALO_CASE's problem on the plan of rank 0 of 2 of an 8-ring."""
    from admm_hip.plan import make_plan
    P = case_problem(HALO_CASE, dtype)
    P["plan"] = make_plan(nx.cycle_graph(8), 8, world=2, rank=0)
    P["W"], P["q_fn"] = precisions(P["n"], 8, HALO_CASE.seed)
    return P
