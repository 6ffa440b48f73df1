"""Device-resident node batch: the per-GPU state of the decentralized ADMM hot path.

Holds, in HBM, everything one GPU needs for its graph nodes (layout: DESIGN.md
"Data layout in HBM") and drives the C-ABI entry points:

* ``node_update()``  -- x-update of every local node (admm_node_update; replaces
  block_6_admm_loop_ver2.py:81-197: neighbour gather, CVXPY/SCS solve, g check);
* ``consensus()``    -- z / y / residual partials of every stored edge
  (admm_consensus; replaces block_6_admm_loop_ver2.py:210-253).

Both are stream-ordered on the current torch stream and replay hipGraphs
recorded at bind time.  ``keep_x=True`` promises that nothing but ``node_update``
writes the local rows of ``x_ext``; each update then starts from the previous
update's A^T(Ax - b) instead of projecting x again (ADMM_BATCH_KEEP_X).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math
import numbers

import numpy as np
import torch

from . import _lib
from .bounds import BoundProjector, check_bound_run, check_bound_weight, check_bounds
from .geometry import (CSR_WEIGHTS_MSG, ParallelBeamGeometry, RayTransform, current_stream_handle,
                       ray_weights_host, _Ctx)
from .links import Gate
from .penalty import NodeNorms
from .plan import ShardPlan, need_stored_z, z_is_stored
from .relax import Relaxer, check_relaxation, check_relaxed_run


def _as_f64_tensor(v, n: int, dev) -> torch.Tensor:
    t = torch.as_tensor(v) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    t = t.reshape(-1)
    if t.numel() != n:
        raise ValueError(f"vector has {t.numel()} entries, expected {n}")
    return t.to(device=dev, dtype=torch.float64)


def _vec_key(t: torch.Tensor):
    h = hashlib.blake2b(t.detach().to("cpu").numpy().tobytes(), digest_size=16).hexdigest()
    return ("hash", h)


def node_ray_weights(ray_weights, nodes, m: int):
    """``ray_weights`` (None, one array broadcast to every node, or a per-global-node sequence
    whose entries are None or an (m,) / (angles, det) array or tensor) as checked float64 host
    arrays {g: (m,)} for ``nodes`` (None entries left out), or None when no node of ``nodes`` has
    weights.  Raises ValueError on a wrong length or a negative / non-finite weight."""
    if ray_weights is None:
        return None
    if isinstance(ray_weights, (list, tuple)):
        get = lambda g: ray_weights[g] if g < len(ray_weights) else None  # noqa: E731
        out = {g: ray_weights_host(get(g), m, f"ray_weights[{g}]") for g in nodes if get(g) is not None}
        return out or None
    w = ray_weights_host(ray_weights, m)
    return {g: w for g in nodes}


class NodeBatch:
    def __init__(self, geom: ParallelBeamGeometry, dtype: str, plan: ShardPlan, sinograms,
                 Qij_diag_fn, rho: float, lam: float, mu: float, tv_iters: int = 10,
                 cg_iters: int = 5, tv_kind: str = "iso", phantom=None, device: int = 0,
                 fusion: str = "midpoint", Wi_list=None, keep_x: bool = False, derive_z: bool | None = None,
                 links=None, relaxation=None, bounds=None, bound_weight=None, ray_weights=None):
        """``links``: None or a bool table (iterations, global edges) (links.schedule): the edge updates of
        ``consensus`` and ``consensus_range`` go through the gate (links.Gate, admm_consensus_gated), which reads
        row ``gate.row`` of the table on the device: an up edge is updated as ever (relaxed if ``relaxation``
        is set, either fusion), a down edge keeps y, z (and y_b) bit for bit.  The bound projection stays as it
        is.  Needs stored z.  None: nothing changes, no buffer.

        ``relaxation``: None or alpha in (0, 2) (relax.check_relaxation; 1.0 is None): the edge
        updates and the constraint's projection run over-relaxed, around alpha x + (1 - alpha) z_old
        (admm_consensus_relaxed / admm_bound_project_relaxed through ``consensus``, ``consensus_range``
        and ``bound_project``; either fusion).  Needs stored z.  None: nothing changes, no buffer.

        ``bounds``: None or (lo, hi) (bounds.check_bounds): the box lo <= x <= hi on every local
        image through the splitting x_k = w_k, w_k in the box.  The plan stays as it is; local node k
        gets one more incidence after its real ones -- edge slot E + k (``z[E + k]`` = w_k,
        ``y[E + k]`` = the scaled dual f_k, sign +1, edge_a = edge_b = k) with the q slot
        ``n_qslots + k`` holding q_c,k = ``bound_weight`` * Wi_list[g] (kappa, default 1) -- so the
        unchanged x-update reads it like an edge term, D includes q_c, the QUAD statistic includes
        the constraint's quadratic term (it is part of the node's subproblem), and the batch is bound
        with n_edges = E + V.  ``consensus`` then updates the real edges (admm_consensus_range) and
        projects (admm_bound_project -> ``bound_stats``); admm_consensus never sees the extra slots.
        Needs stored z and midpoint fusion.  None: nothing changes.

        ``ray_weights``: per-ray weights omega of the data term 1/2 sum_r omega_r (A x - b)_r^2
        (node_ray_weights: None, one array for every node, or a per-global-node sequence; finite,
        >= 0, checked once here on the host; a node without an entry has omega = 1).  None leaves
        the unweighted path untouched.

        ``derive_z``: z_ij is not stored but derived from the endpoint images of the last
        consensus (``x_prev``, one row per x_ext row; ABI 7; midpoint fusion only).  None: the
        edge-state rule (plan.z_is_stored) on this batch alone -- stored z, the faster form,
        unless its rows would exceed the rule's share of HBM; RankGroups passes the run's one
        global decision instead.  block_5's drop-in, which injects arbitrary targets v_ij through
        z, keeps it stored (``derive_z=False``)."""
        self.lib = _lib.load()
        self.geom = geom
        self.plan = plan
        self.dtype = dtype
        self.device = device
        dev = torch.device("cuda", device)
        self.dev = dev
        n, m = geom.n, geom.m
        V = plan.V
        if V < 1:
            raise ValueError("rank owns no graph nodes")
        # bound constraints: checked on the host before any device work
        self.bounds = check_bounds(bounds, geom.N)
        kappa = check_bound_weight(bound_weight, self.bounds)
        alpha = check_relaxation(relaxation)
        check_relaxed_run(alpha, "derived" if derive_z else None)
        if links is not None and derive_z:
            raise ValueError("links need stored z: a derived z has no per-edge age")
        check_bound_run(self.bounds, fusion, "derived" if derive_z else None)
        if self.bounds is not None and Wi_list is None:
            raise ValueError("bounds need Wi_list: q_c,i = bound_weight * Wi_list[i]")
        wts = node_ray_weights(ray_weights, plan.local_nodes, m)
        if wts is not None and hasattr(geom, "create_ctx"):
            raise ValueError(CSR_WEIGHTS_MSG)
        sdt = torch.float64 if dtype == "float64" else torch.float32
        self.ctx = _Ctx(geom, dtype, device, max_images=max(1, V))
        self.x_ext = torch.zeros((plan.n_xext, n), dtype=torch.float64, device=dev)
        self.d = torch.zeros((V, 2, n), dtype=torch.float64, device=dev)
        self.e = torch.zeros((V, 2, n), dtype=torch.float64, device=dev)
        self.atb = torch.zeros((V, n), dtype=torch.float64, device=dev)
        self.b = torch.empty((V, m), dtype=sdt, device=dev)
        for k, g in enumerate(plan.local_nodes):
            s = sinograms[g]
            st = s if isinstance(s, torch.Tensor) else torch.as_tensor(np.asarray(s))
            st = st.reshape(-1)
            if st.numel() != m:
                raise ValueError(f"sinogram of node {g} has {st.numel()} entries, expected {m}")
            self.b[k].copy_(st.to(device=dev, dtype=sdt))
        self.phantom = None
        if phantom is not None:
            self.phantom = _as_f64_tensor(phantom, n, dev)
        # precision vectors q_ij, deduplicated into slots
        E = len(plan.stored_edges)
        NB = V if self.bounds is not None else 0  # constraint slots: edge slots E .. E + V - 1
        self.n_real_edges = E
        keyfn = getattr(Qij_diag_fn, "qslot_key", None)
        slots, qvecs, inc_qslot = {}, [], []
        for k, g in enumerate(plan.local_nodes):
            for q in range(plan.inc_off[k], plan.inc_off[k + 1]):
                j = plan.inc_nbr[q]
                key = keyfn(g, j) if keyfn is not None else None
                if key is not None and key in slots:
                    inc_qslot.append(slots[key])
                    continue
                vec = _as_f64_tensor(Qij_diag_fn(g, j), n, dev)
                if key is None:
                    key = _vec_key(vec)
                if key not in slots:
                    slots[key] = len(qvecs)
                    qvecs.append(vec)
                inc_qslot.append(slots[key])
        self.n_qslots = len(qvecs)  # the real incidences' slots; q_c,k follows in slot n_qslots + k
        self.inc_qslot_host = list(inc_qslot)
        if NB:
            qvecs = qvecs + [kappa * _as_f64_tensor(Wi_list[g], n, dev) for g in plan.local_nodes]
        self.q = torch.stack(qvecs) if qvecs else torch.zeros((1, n), dtype=torch.float64, device=dev)
        ii = lambda a: torch.tensor(a if len(a) else [0], dtype=torch.int32, device=dev)  # noqa: E731
        if NB:
            # node k's incidences: the plan's, then the constraint's (so c = sum q v adds it last)
            off, edge, sign, qslot = [0], [], [], []
            for k in range(V):
                lo_, hi_ = plan.inc_off[k], plan.inc_off[k + 1]
                edge += list(plan.inc_edge[lo_:hi_]) + [E + k]
                sign += list(plan.inc_sign[lo_:hi_]) + [1]
                qslot += inc_qslot[lo_:hi_] + [self.n_qslots + k]
                off.append(len(edge))
            self.inc_off, self.inc_edge, self.inc_sign, self.inc_qslot = ii(off), ii(edge), ii(sign), ii(qslot)
            self.edge_a = ii(list(plan.edge_a_row) + list(range(V)))
            self.edge_b = ii(list(plan.edge_b_row) + list(range(V)))
        else:
            self.inc_off = ii(plan.inc_off)
            self.inc_edge = ii(plan.inc_edge)
            self.inc_sign = ii(plan.inc_sign)
            self.inc_qslot = ii(inc_qslot)
            self.edge_a = ii(plan.edge_a_row)
            self.edge_b = ii(plan.edge_b_row)
        ES = E + NB  # edge slots the batch is bound with
        self.y = torch.zeros((max(ES, 1), n), dtype=torch.float64, device=dev)
        # weighted edge fusion: both endpoint duals + W of every x_ext row
        if fusion not in ("midpoint", "weighted"):
            raise ValueError("fusion must be 'midpoint' or 'weighted'")
        if derive_z is None:
            hbm = int(torch.cuda.get_device_properties(dev).total_memory)
            derive_z = not z_is_stored([ES], n, hbm, fusion)
            need_stored_z(derive_z, bool(NB), alpha is not None, "batch", links=links is not None)
        if derive_z and fusion != "midpoint":
            raise ValueError("derived z needs midpoint fusion")
        self.derive_z = bool(derive_z)
        # derived: x_ext at the last consensus (x = 0 before the first: z = 0); stored: z per edge
        self.z = None if self.derive_z else torch.zeros((max(ES, 1), n), dtype=torch.float64, device=dev)
        self.x_prev = torch.zeros((plan.n_xext, n), dtype=torch.float64, device=dev) if self.derive_z else None
        self.fusion = fusion
        self.y_b = None
        self.w = None
        if fusion == "weighted":
            if Wi_list is None:
                raise ValueError("weighted fusion needs Wi_list")
            self.y_b = torch.zeros((max(E, 1), n), dtype=torch.float64, device=dev)
            self.w = torch.stack([_as_f64_tensor(Wi_list[g], n, dev)
                                  for g in plan.local_nodes + plan.halo_nodes])
        # D_i = sum_j q_ij  (constant across iterations; setup)
        self.dsum = torch.zeros((V, n), dtype=torch.float64, device=dev)
        self._sum_precisions()
        self.node_stats = torch.zeros((V, _lib.NODE_STATS), dtype=torch.float64, device=dev)
        self.edge_stats = torch.zeros((max(ES, 1), _lib.EDGE_STATS), dtype=torch.float64, device=dev)
        # the projection's scratch and its per-node sums (|x - w|^2, |w - w_old|^2, |x - clip(x)|^2)
        self.projector = BoundProjector(self.bounds, n, dev, V) if NB else None
        self.bound_stats = self.projector.sums if NB else None  # (V, BOUND_STATS), written by the kernel
        # over-relaxation: alpha and the relaxed edge kernel's scratch (None: the plain updates)
        self.relaxer = Relaxer(alpha, n, E, dev) if alpha is not None else None
        # unreliable links: the gate table in slot order, alpha and the gated kernel's scratch (None: every edge up)
        self.gate = Gate(links, plan.stored_edges, n, dev, alpha) if links is not None else None
        # the stop test's three norms per node (node_norms): scratch and sums made at the first call
        self.norms = None
        self.norm_stats = None
        self.params = dict(rho=float(rho), lam=float(lam), mu=float(mu), tv_iters=int(tv_iters),
                           cg_iters=int(cg_iters), tv_kind=tv_kind)
        p = _lib.ptr
        self.cb = _lib.Batch(
            V, plan.n_xext, ES, int(tv_iters), int(cg_iters),
            _lib.ADMM_TV_ANISO if tv_kind == "aniso" else _lib.ADMM_TV_ISO,
            float(rho), float(lam), float(mu),
            p(self.x_ext), p(self.d), p(self.e), p(self.atb), p(self.dsum), p(self.b), p(self.phantom),
            p(self.y), p(self.z), p(self.q), p(self.edge_a), p(self.edge_b), p(self.inc_off),
            p(self.inc_edge), p(self.inc_qslot), p(self.inc_sign), p(self.node_stats),
            p(self.edge_stats),
            _lib.ADMM_FUSE_WEIGHTED if fusion == "weighted" else _lib.ADMM_FUSE_MIDPOINT,
            _lib.ADMM_BATCH_KEEP_X if keep_x else 0,
            p(self.y_b), p(self.w), p(self.x_prev))
        # per-ray weights [V][m] in the sample dtype (None: the unweighted batch, no buffer, no call)
        self.ray_weights = self._weights_tensor(wts)
        torch.cuda.synchronize(dev)
        _lib.check(self.lib.admm_batch_bind(self.ctx.h, C.byref(self.cb)), "admm_batch_bind")
        self._apply_ray_weights()
        _lib.check(self.lib.admm_batch_atb(self.ctx.h, p(self.atb), C.c_void_p(self._s())),
                   "admm_batch_atb")

    def _sum_precisions(self) -> None:
        """dsum[k] = D_k = sum_j q_kj in incidence order, then q_c,k when the batch has bounds."""
        plan = self.plan
        self.dsum.zero_()
        for k in range(plan.V):
            for s in range(plan.inc_off[k], plan.inc_off[k + 1]):
                self.dsum[k] += self.q[self.inc_qslot_host[s]]
            if self.bounds is not None:
                self.dsum[k] += self.q[self.n_qslots + k]

    def _weights_tensor(self, wts):
        """{g: (m,)} host weights -> the batch's [V][m] device tensor (1 where a node has none)."""
        if wts is None:
            return None
        t = torch.ones_like(self.b)
        for k, g in enumerate(self.plan.local_nodes):
            if g in wts:
                t[k].copy_(torch.as_tensor(wts[g]).to(device=self.dev, dtype=t.dtype))
        return t

    def _apply_ray_weights(self) -> None:
        """After every bind (which drops them): the batch's weights, if it has any."""
        if self.ray_weights is not None:
            _lib.check(self.lib.admm_batch_set_ray_weights(self.ctx.h, C.c_void_p(self.ray_weights.data_ptr()),
                                                           C.c_void_p(self._s())), "admm_batch_set_ray_weights")

    def set_ray_weights(self, ray_weights) -> None:
        """New per-ray weights for the bound batch (as at construction; None clears them): the
        library re-records its sequences and A^T (omega b) is formed again."""
        wts = node_ray_weights(ray_weights, self.plan.local_nodes, self.geom.m)
        if wts is not None and hasattr(self.geom, "create_ctx"):
            raise ValueError(CSR_WEIGHTS_MSG)
        if wts is None and self.ray_weights is None:
            return
        self.ray_weights = self._weights_tensor(wts)
        torch.cuda.synchronize(self.dev)
        if wts is None:
            _lib.check(self.lib.admm_batch_set_ray_weights(self.ctx.h, C.c_void_p(0), C.c_void_p(self._s())),
                       "admm_batch_set_ray_weights")
        else:
            self._apply_ray_weights()
        _lib.check(self.lib.admm_batch_atb(self.ctx.h, C.c_void_p(self.atb.data_ptr()), C.c_void_p(self._s())),
                   "admm_batch_atb")

    def update_ray_weights(self, t) -> None:
        """New values for the weights of a batch that has some, from the device tensor ``t`` ([V][m] in
        the sample dtype, contiguous), on the current stream: the library repacks them into its own
        buffer (admm_batch_update_ray_weights: no host copy, no synchronisation, nothing re-recorded)
        and A^T (omega b) is formed again.  The next update is bitwise that of a batch given ``t`` by
        ``set_ray_weights``.  ``ray_weights`` -- what a re-bind applies again -- stays the caller's."""
        if self.ray_weights is None:
            raise ValueError("update_ray_weights needs a batch with ray weights (set_ray_weights first)")
        if not isinstance(t, torch.Tensor) or t.device != self.b.device or t.dtype != self.b.dtype or \
                tuple(t.shape) != tuple(self.b.shape) or not t.is_contiguous():
            raise ValueError(f"weights must be a contiguous {self.b.dtype} {tuple(self.b.shape)} tensor on "
                             f"{self.b.device}")
        s = C.c_void_p(self._s())
        _lib.check(self.lib.admm_batch_update_ray_weights(self.ctx.h, C.c_void_p(t.data_ptr()), s),
                   "admm_batch_update_ray_weights")
        _lib.check(self.lib.admm_batch_atb(self.ctx.h, C.c_void_p(self.atb.data_ptr()), s), "admm_batch_atb")

    def refresh_kept_start(self) -> None:
        """After ``update_ray_weights`` on a ``keep_x`` batch that had completed an update: the kept
        A^T omega (A x - b) formed again under the new weights (admm_batch_refresh_kept, on the current
        stream), so that the next update starts from it -- as every update of a run with fixed weights
        does -- instead of projecting x again."""
        _lib.check(self.lib.admm_batch_refresh_kept(self.ctx.h, C.c_void_p(self._s())), "admm_batch_refresh_kept")

    def project_samples(self, xs, out) -> None:
        """``out`` ([V][m]) <- A ``xs`` ([V][n]), both contiguous in the sample dtype, with the batch's
        own operator context on the current stream (admm_project_fwd: the operator scratch, not the
        bound batch's)."""
        _lib.check(self.lib.admm_project_fwd(self.ctx.h, C.c_void_p(xs.data_ptr()), C.c_void_p(out.data_ptr()),
                                             self.V, C.c_void_p(self._s())), "admm_project_fwd")

    def set_precisions(self, qs) -> None:
        """New q_ij for a batch bound with one q slot per incidence (in incidence order): the
        slots are rewritten (q_c of a batch with bounds is not one of them and stays), D = sum_j q_ij
        (+ q_c) is recomputed as at construction (same order) and the
        batch re-bound (its interleaved D samples and recorded sequences are bind-time data).
        Used by the block_5 drop-in's batch cache."""
        if len(qs) != len(self.inc_qslot_host) or sorted(self.inc_qslot_host) != list(range(len(qs))):
            raise ValueError("set_precisions needs one q slot per incidence")
        for s, q in enumerate(qs):
            self.q[self.inc_qslot_host[s]].copy_(_as_f64_tensor(q, self.geom.n, self.dev))
        self._sum_precisions()
        torch.cuda.synchronize(self.dev)
        _lib.check(self.lib.admm_batch_bind(self.ctx.h, C.byref(self.cb)), "admm_batch_bind")
        self._apply_ray_weights()

    def set_rho(self, rho) -> None:
        """The batch's penalty rho <- ``rho`` (finite, > 0) between two iterations.  The scaled duals
        stand for the unscaled rho y, so y -- the constraint rows f included -- and y_b are multiplied
        by rho_old / rho_new (exact for a power of two); z, d, e, atb and mu are untouched.  The
        library packs rho D again and re-records its sequences (admm_batch_set_rho: weights, forward
        plan and scratch stay); the next update is bitwise a freshly bound batch's with this rho."""
        if isinstance(rho, bool) or not isinstance(rho, numbers.Real) or not (math.isfinite(rho) and rho > 0):
            raise ValueError(f"rho must be a finite real number > 0, got {rho!r}")
        new, old = float(rho), self.params["rho"]
        if new == old:
            return
        c = old / new
        self.y.mul_(c)
        if self.y_b is not None:
            self.y_b.mul_(c)
        _lib.check(self.lib.admm_batch_set_rho(self.ctx.h, new, C.c_void_p(self._s())), "admm_batch_set_rho")
        self.params["rho"] = new
        self.cb.rho = new

    def node_norms(self) -> torch.Tensor:
        """``norm_stats`` (V, 3) <- X2 = |x_k|^2, Z2 = sum of |z_e|^2 and U2 = |sum of the scaled duals|^2
        over node k's incidences (the constraint slot of a batch with bounds included), on the current
        stream (admm_node_norms; penalty.thresholds turns them into the stop thresholds).  Needs
        stored z.  The scratch is made at the first call."""
        if self.z is None:
            raise ValueError("node_norms needs stored z")
        if self.norms is None:
            self.norms = NodeNorms(self.geom.n, self.V, self.dev)
            self.norm_stats = self.norms.sums
        n_edges = self.cb.n_edges
        return self.norms.run(self.x_local, self.y, self.y_b, self.z, self.inc_off,
                              self.inc_edge if n_edges else None, self.inc_sign if n_edges else None, n_edges,
                              self._s())

    def set_local_images(self, images) -> None:
        """Local rows of x_ext <- ``images[g]`` (float64 (n,) device tensors by global node)."""
        for r, g in enumerate(self.plan.local_nodes):
            self.x_ext[r].copy_(images[g])

    def start_edges(self) -> None:
        """A fresh ADMM state around the current x_ext (halo rows included): zero duals and
        split-Bregman variables, z_e = (x_a + x_b) / 2 (weighted fusion: (W_a x_a + W_b x_b) /
        (W_a + W_b)); derived z: x_prev = x_ext.  Elementwise torch expressions of the endpoint
        rows, so every batch and rank that stores an edge forms the same z bitwise.  The library
        projects x again in the first update after a bind, so keep_x batches start correctly."""
        self.d.zero_()
        self.e.zero_()
        self.y.zero_()
        if self.y_b is not None:
            self.y_b.zero_()
        if self.x_prev is not None:
            self.x_prev.copy_(self.x_ext)
        if self.z is None:
            return
        x, w = self.x_ext, self.w
        if self.bounds is not None:  # constraint slots: w = clip(x), f = 0 (y is zero already)
            E = self.n_real_edges
            self.z[E:E + self.V] = self.projector.clip(self.x_local)
        for k in range(len(self.plan.stored_edges)):  # one edge at a time: no [E][n] temporaries
            a, b = self.plan.edge_a_row[k], self.plan.edge_b_row[k]
            if self.fusion == "weighted":
                self.z[k] = (w[a] * x[a] + w[b] * x[b]) / (w[a] + w[b])
            else:
                self.z[k] = (x[a] + x[b]) * 0.5

    def z_of(self, k: int) -> torch.Tensor:
        """z of stored edge slot k: the stored vector, or (derived) the midpoint of its endpoint
        rows of x_prev -- the value every kernel forms."""
        if self.z is not None:
            return self.z[k]
        return (self.x_prev[self.plan.edge_a_row[k]] + self.x_prev[self.plan.edge_b_row[k]]) * 0.5

    def _s(self) -> int:
        return current_stream_handle(self.dev)

    @property
    def V(self) -> int:
        return self.plan.V

    def _info(self) -> tuple[int, bool]:
        vb, mm = C.c_int(), C.c_int()
        _lib.check(self.lib.admm_batch_info(self.ctx.h, C.byref(vb), C.byref(mm)), "admm_batch_info")
        return vb.value, bool(mm.value)

    @property
    def ctx_vb(self) -> int:
        """Node-interleave width the library chose for this batch (admm_batch_info, ABI 8):
        vb_for(V) in admm_tomo.hip, capped at 16-byte vectors in mirror mode."""
        return self._info()[0]

    @property
    def mirror(self) -> bool:
        """The bound batch's projectors run in mirror mode (admm_batch_info, ABI 8)."""
        return self._info()[1]

    @property
    def x_local(self) -> torch.Tensor:
        return self.x_ext[: self.plan.V]

    def node_update(self, rounds: int | None = None) -> None:
        """One x-update of every local node; ``rounds`` overrides the bound split-Bregman
        round count (chunked solves, admm_node_update_rounds)."""
        if rounds is None:
            _lib.check(self.lib.admm_node_update(self.ctx.h, C.c_void_p(self._s())), "admm_node_update")
        else:
            _lib.check(self.lib.admm_node_update_rounds(self.ctx.h, int(rounds), C.c_void_p(self._s())),
                       "admm_node_update_rounds")

    def node_update_masked(self, active) -> None:
        """x-update of the nodes where ``active`` (bool, length V) is set; the others keep
        their x, d, e and statistics bitwise (saved before, restored after the batched
        update).  Needs keep_x=False: a restored node's x no longer matches the kept
        A^T(Ax - b) of the reuse start."""
        act = torch.as_tensor(np.asarray(active, dtype=bool))
        if bool(act.all()):
            self.node_update()
            return
        if not bool(act.any()):
            return
        if self.cb.flags & _lib.ADMM_BATCH_KEEP_X:
            raise RuntimeError("node_update_masked needs a batch bound with keep_x=False")
        idx = torch.nonzero(~act).reshape(-1).to(self.dev)
        saved = [(t, t.index_select(0, idx)) for t in (self.x_local, self.d, self.e, self.node_stats)]
        self.node_update()
        for t, s in saved:
            t.index_copy_(0, idx, s)

    def consensus(self) -> None:
        if self.gate is not None:  # every real edge under the current row's gates, then the constraint slots
            self.gate.run_edges(self, 0, self.n_real_edges, self._s())
            if self.bounds is not None:
                self.bound_project()
        elif self.relaxer is not None:  # every real edge (either fusion), then the constraint slots
            self.relaxer.run_edges(self, 0, self.n_real_edges, self._s())
            if self.bounds is not None:
                self.bound_project()
        elif self.bounds is not None:  # the real edges only, then the projection of the constraint slots
            self.consensus_range(0, self.n_real_edges, self.plan.n_xext)
            self.bound_project()
        elif self.plan.stored_edges:
            _lib.check(self.lib.admm_consensus(self.ctx.h, C.c_void_p(self._s())), "admm_consensus")

    @property
    def w_bound(self) -> torch.Tensor:
        """w_k of every local node (rows E .. E + V - 1 of z): inside the box exactly."""
        return self.z[self.n_real_edges:self.n_real_edges + self.V]

    @property
    def f_bound(self) -> torch.Tensor:
        """The constraint's scaled dual f_k of every local node (rows E .. E + V - 1 of y)."""
        return self.y[self.n_real_edges:self.n_real_edges + self.V]

    def bound_project(self) -> None:
        """w' = clip(x + f), f' = f + x - w' of every local node (admm_bound_project on the current
        stream; needs no halo row) and ``bound_stats`` <- its three sums per node.  A relaxed batch
        projects around alpha x + (1 - alpha) w (admm_bound_project_relaxed)."""
        if self.relaxer is not None:
            self.relaxer.run_bounds(self.projector, self.x_local, self.w_bound, self.f_bound, self._s())
        else:
            self.projector.run(self.x_local, self.w_bound, self.f_bound, self._s())

    def consensus_range(self, e0: int, e1: int, rows: int) -> None:
        """Edge updates of stored slots [e0, e1) only, whose endpoints lie in x_ext rows [0, rows)
        (stored z, midpoint fusion; admm_consensus_range, ABI 9): the same per-edge results and
        statistics as ``consensus``.  The endpoint rows are checked here against ``rows`` (the
        library reads only rows below it while the halo rows may still be landing)."""
        if e1 > e0:
            top = max(max(self.plan.edge_a_row[e0:e1]), max(self.plan.edge_b_row[e0:e1]))
            if top >= rows:
                raise ValueError(f"edge slots [{e0}, {e1}) reach x_ext row {top} >= rows={rows}")
            if self.gate is not None or self.relaxer is not None:
                if self.fusion != "midpoint":
                    raise ValueError("consensus_range needs midpoint fusion")
                (self.gate or self.relaxer).run_edges(self, e0, e1, self._s())
                return
            _lib.check(self.lib.admm_consensus_range(self.ctx.h, int(e0), int(e1), int(rows), C.c_void_p(self._s())),
                       "admm_consensus_range")

    def marker(self) -> None:
        """One k_tv_grad launch (never part of an x-update or consensus): delimits the
        bench's timed steps in rocprofv3 PMC traces (scripts/traffic_summary.py)."""
        if getattr(self, "_mk", None) is None:
            self._mk = torch.empty((2, self.geom.n), dtype=torch.float64, device=self.dev)
        _lib.check(self.lib.admm_tv_grad(self.ctx.h, C.c_void_p(self.x_ext.data_ptr()),
                                         C.c_void_p(self._mk[0].data_ptr()),
                                         C.c_void_p(self._mk[1].data_ptr()), 1, C.c_void_p(self._s())),
                   "admm_tv_grad")

    def time_forward(self, reps: int = 20, in_solve: bool = False) -> float:
        """Average k_fwdg launch (ms): ``reps`` back-to-back, or ``in_solve`` -- every CG-step
        forward of one directly enqueued x-update (the batch's state advances by it)."""
        ms = C.c_double()
        _lib.check(self.lib.admm_time_forward(self.ctx.h, reps, int(in_solve), C.c_void_p(self._s()), C.byref(ms)),
                   "admm_time_forward")
        return ms.value

    def time_back(self) -> float:
        """Average in-solve back projector launch (ms; k_back / k_back_mirror in H mode): every
        CG step of one directly enqueued x-update (admm_time_back, ABI 9; the state advances)."""
        ms = C.c_double()
        _lib.check(self.lib.admm_time_back(self.ctx.h, C.c_void_p(self._s()), C.byref(ms)), "admm_time_back")
        return ms.value

    def fwd_plans(self) -> list[dict]:
        """The grouped forward projector's plans for this batch's geometry (admm_fwd_plan_info):
        per plan 0-5 its angle groups, blocks per node chunk, staged row pixels (host model)
        and whether it is the bound one; plans the geometry does not have are omitted."""
        out = []
        for pl in range(6):
            g, b, a, st = C.c_int(), C.c_int(), C.c_int(), C.c_double()
            _lib.check(self.lib.admm_fwd_plan_info(self.ctx.h, pl, C.byref(g), C.byref(b), C.byref(st),
                                                   C.byref(a)), "admm_fwd_plan_info")
            if g.value:
                out.append(dict(plan=pl, groups=g.value, blocks=b.value, staged_px=st.value,
                                active=bool(a.value)))
        return out


def make_operators(N: int, num_nodes: int, angles_total: int | None = None, dtype: str = "float32",
                   device: int | None = None, det_width_factor: float = 1.0) -> list[RayTransform]:
    """Per-node ray transforms of block_2_load_odl_data.py:16-65 (all nodes span [0, pi)),
    on ``device`` (default: the current device, see geometry.default_device)."""
    from .geometry import default_device, split_angles
    if device is None:
        device = default_device()
    if angles_total is None:
        angles_total = max(180, 3 * N)
    per = split_angles(angles_total, num_nodes)
    return [RayTransform(ParallelBeamGeometry(N, a, det_width_factor), dtype, device) for a in per]
