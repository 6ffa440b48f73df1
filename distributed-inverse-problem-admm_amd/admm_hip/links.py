"""Unreliable links: per-iteration edge activation (scope row f14).

At iteration k every graph edge is up or down.  An up edge performs its z / y update as ever (relaxed,
weighted: whatever the run does); a down edge keeps y, z (and y_b) bit for bit, and both its endpoints go
on with the last (z, y) they hold.  Its statistics are the disagreement with that z: RA2 = |x_a - z|^2,
RB2 = |x_b - z|^2, DZ2 = 0.  Updating a random subset of the edge blocks per iteration is the randomized
ADMM of Iutzeler, Bianchi, Ciblat and Hachem (CDC 2013): the edge phase is a fixed-point iteration of an
averaged operator on (y_e, z_e), and it converges almost surely to the same fixed point when every edge is
up with positive probability (stated for exact node solves and i.i.d. activation).

Host side of ``admm_consensus_gated`` (csrc/links.hip):

* ``check_links`` / ``check_links_run``: the argument checks, which need no device;
* ``edge_list`` / ``schedule``: the run's global edge order and the bool table (iterations x edges) a
  ``links`` value stands for -- pinned, so that every rank, a reference and a user form the same one;
* ``links_up`` / ``link_age_max``: the two history keys, host arithmetic on the table;
* ``Gate``: one NodeBatch's table on the device in slot order, the kernel's scratch and the current row.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib
from .plan import canonical_edges, derived_z_requested

LINK_KEYS = ("links_up", "link_age_max")
SEED_TAG = 0x4C4E4B53  # second word of the generator's seed: [seed, SEED_TAG]
_DICT_KEYS = ("p", "seed", "max_age", "outages")


def _check_p(p):
    if isinstance(p, bool) or not isinstance(p, numbers.Real):
        raise ValueError(f"links: p must be a real number in (0, 1], got {p!r}")
    v = float(p)
    if math.isnan(v) or not (0.0 < v <= 1.0):
        raise ValueError(f"links: p must lie in (0, 1], got {p!r}")
    return v


def _check_int(v, name, lo):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) < lo:
        raise ValueError(f"links: {name} must be an int >= {lo}, got {v!r}")
    return int(v)


def check_links(links):
    """``links`` as None (every edge up in every iteration: the run without the keyword), a dict with all
    of ``p``, ``seed``, ``max_age``, ``outages`` (a tuple of (a, b, k0, k1), a < b, k1 None = for good), or
    a 2-D bool array (used as it is; its shape is checked against the run by ``schedule``).  Raises
    ValueError for a bool, NaN, p <= 0 or p > 1, unknown keys, max_age < 1, a malformed outage or one with
    k1 <= k0, and anything else.  Host work only."""
    if links is None:
        return None
    if isinstance(links, bool):
        raise ValueError(f"links must be None, a probability in (0, 1], a dict or a bool array, got {links!r}")
    if isinstance(links, numbers.Real):
        p = _check_p(links)
        return None if p == 1.0 else dict(p=p, seed=0, max_age=None, outages=())
    if isinstance(links, dict):
        unknown = sorted(set(links) - set(_DICT_KEYS), key=str)
        if unknown:
            raise ValueError(f"links: unknown keys {unknown}; known: {list(_DICT_KEYS)}")
        p = _check_p(links.get("p", 1.0))
        seed = _check_int(links.get("seed", 0), "seed", 0)
        max_age = links.get("max_age")
        if max_age is not None:
            max_age = _check_int(max_age, "max_age", 1)
        outages = []
        raw = links.get("outages") or ()
        if isinstance(raw, (str, bytes)) or not hasattr(raw, "__iter__"):
            raise ValueError(f"links: outages must be a list of (a, b, k0, k1), got {raw!r}")
        for o in raw:
            if isinstance(o, (str, bytes)) or not hasattr(o, "__len__") or len(o) != 4:
                raise ValueError(f"links: an outage is (a, b, k0, k1), got {o!r}")
            a, b = _check_int(o[0], "an outage's node", 0), _check_int(o[1], "an outage's node", 0)
            k0 = _check_int(o[2], "an outage's k0", 0)
            k1 = None if o[3] is None else _check_int(o[3], "an outage's k1", 0)
            if k1 is not None and k1 <= k0:
                raise ValueError(f"links: outage {tuple(o)!r} has k1 <= k0")
            outages.append((min(a, b), max(a, b), k0, k1))
        if p == 1.0 and not outages:  # (max_age alone forces nothing: no edge is ever down)
            return None
        return dict(p=p, seed=seed, max_age=max_age, outages=tuple(outages))
    if isinstance(links, np.ndarray) or type(links).__module__.startswith("torch"):
        arr = np.asarray(links.detach().cpu().numpy() if hasattr(links, "detach") else links)
        if arr.dtype != np.bool_ or arr.ndim != 2:
            raise ValueError(f"links: an array must be 2-D bool (iterations, edges), got {arr.dtype} {arr.shape}")
        return np.ascontiguousarray(arr)
    raise ValueError(f"links must be None, a probability in (0, 1], a dict or a bool array, got {links!r}")


def check_links_run(links, edge_state, env_edge_state: str = ""):
    """The combination a run with ``links`` (checked) does not support, as ValueError (host work only): a
    derived z is the midpoint of the last images, so it has no per-edge age."""
    if links is None:
        return
    if derived_z_requested(edge_state, env_edge_state):
        raise ValueError("links need stored z (edge_state='stored'): a derived z is the midpoint of the last "
                         "images of both endpoints, so a down edge cannot keep the z it last agreed on")


def edge_list(G):
    """The run's global edge order: ``G.edges()`` as (min, max) pairs -- the columns of ``schedule``, the
    rows of the edge table."""
    return canonical_edges(G, G.number_of_nodes())


def schedule(G, max_iters: int, links):
    """The (max_iters, E) bool table of ``links`` on graph ``G``: entry [k, e] says that edge e of
    ``edge_list(G)`` is up in iteration k.  None (and what normalises to it): all True.  A probability p /
    a dict: ``np.random.default_rng([seed, 0x4C4E4B53]).random((max_iters, E)) < p``, then an edge that has
    been down ``max_age`` iterations in a row is forced up, then the outages take their edges down (an
    outage wins: it is physical).  An array: its first max_iters rows; ValueError if it has fewer rows or
    not E columns.  An outage that names a non-edge raises ValueError."""
    cfg = check_links(links)
    edges = edge_list(G)
    E, K = len(edges), int(max_iters)
    if cfg is None:
        return np.ones((K, E), dtype=bool)
    if isinstance(cfg, np.ndarray):
        if cfg.shape[1] != E:
            raise ValueError(f"links: the table has {cfg.shape[1]} columns, the graph has {E} edges")
        if cfg.shape[0] < K:
            raise ValueError(f"links: the table has {cfg.shape[0]} rows, the run may take {K} iterations")
        return cfg[:K].copy()
    up = np.random.default_rng([cfg["seed"], SEED_TAG]).random((K, E)) < cfg["p"]
    if cfg["max_age"] is not None:
        down = np.zeros(E, dtype=np.int64)  # iterations in a row each edge has been down
        for k in range(K):
            up[k] |= down >= cfg["max_age"]
            down = np.where(up[k], 0, down + 1)
    col = {e: c for c, e in enumerate(edges)}
    for a, b, k0, k1 in cfg["outages"]:
        if (a, b) not in col:
            raise ValueError(f"links: outage names ({a}, {b}), which is no edge of the graph")
        up[k0:(K if k1 is None else k1), col[(a, b)]] = False
    return up


def links_up(table) -> np.ndarray:
    """Up edges per iteration."""
    return np.asarray(table, dtype=bool).sum(axis=1).astype(np.int64)


def link_age_max(table) -> np.ndarray:
    """After each iteration, the largest number of iterations since an edge's last update (0: every edge
    was updated in this one; an edge never updated counts from the start of the run)."""
    t = np.asarray(table, dtype=bool)
    age = np.zeros(t.shape[1], dtype=np.int64)
    out = np.zeros(t.shape[0], dtype=np.int64)
    for k in range(t.shape[0]):
        age = np.where(t[k], 0, age + 1)
        out[k] = age.max() if age.size else 0
    return out


def describe(cfg, table) -> str:
    """One line for admm_internal_params.txt."""
    frac = float(np.mean(table)) if table.size else 1.0
    if isinstance(cfg, np.ndarray):
        return f"Unreliable links: explicit table {table.shape[0]} x {table.shape[1]}, up fraction = {frac:.4f}"
    return (f"Unreliable links: p = {cfg['p']}, seed = {cfg['seed']}, max_age = {cfg['max_age']}, outages = "
            f"{list(cfg['outages'])}, up fraction = {frac:.4f}")


class Gate:
    """The gated edge updates of one NodeBatch with ``n_edges`` real edge slots of ``n`` pixels on
    ``device``: ``table`` (iterations x global edges, bool) mapped through ``stored_edges`` (the global
    edge of every slot) into a uint8 device table in slot order -- an edge stored by two batches or two
    ranks reads the same column --, alpha (None: 1.0), the kernel's scratch and the current row."""

    def __init__(self, table, stored_edges, n: int, device, alpha=None):
        import torch
        self.lib = _lib.load()
        t = np.asarray(table, dtype=bool)
        self.n = int(n)
        self.n_edges = len(stored_edges)
        self.alpha = 1.0 if alpha is None else float(alpha)
        cols = np.asarray(list(stored_edges), dtype=np.int64)
        if cols.size and (cols.min() < 0 or cols.max() >= t.shape[1]):
            raise ValueError(f"stored edges reach column {int(cols.max())} of a table with {t.shape[1]} columns")
        host = np.ascontiguousarray(t[:, cols].astype(np.uint8)) if cols.size else np.zeros((t.shape[0], 1), np.uint8)
        self.up = torch.from_numpy(host).to(device)
        self.rows = int(t.shape[0])
        self.row = 0
        self.work = _lib.work_buffer("admm_consensus_gated_work", self.n, self.n_edges, device=device)

    def set_row(self, k: int) -> None:
        """The iteration whose gates the next ``run_edges`` reads (host arithmetic on a pointer)."""
        if not (0 <= int(k) < self.rows):
            raise ValueError(f"iteration {k} outside the link table's [0, {self.rows})")
        self.row = int(k)

    def run_edges(self, nb, e0: int, e1: int, stream: int) -> None:
        """y, z (weighted fusion: y_b too) and ``edge_stats`` of ``nb``'s edge slots [e0, e1) <- the gated
        update around its x_ext under the current row, in place, on ``stream``."""
        if not (0 <= e0 <= e1 <= self.n_edges):
            raise ValueError(f"edge slots [{e0}, {e1}) outside the batch's [0, {self.n_edges})")
        p = _lib.ptr
        _lib.check(self.lib.admm_consensus_gated(p(nb.x_ext), self.n, nb.x_ext.shape[0], p(nb.y), p(nb.y_b), p(nb.z),
                                                 p(nb.w), p(nb.edge_a), p(nb.edge_b), int(e0), int(e1), self.alpha,
                                                 C.c_void_p(self.up[self.row].data_ptr()), p(self.work),
                                                 p(nb.edge_stats), C.c_void_p(stream)),
                   "admm_consensus_gated")
