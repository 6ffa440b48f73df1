"""One rank's graph nodes as device batches, one batch per distinct operator.

The batched kernels project every node of a batch with one angle table (or one CSR
matrix): node-interleaved samples put the same pixel of VB nodes in one vector, so
those nodes must share A.  The reference does not guarantee that: ``load_odl_data``
splits ``max(180, 3N)`` angles over the nodes with the remainder going to the first
ones (/root/reference/block_2_load_odl_data.py:31-38) -- its own defaults give
77/77/77/77/76 angles at N=128 and 39/39/38/38/38 at N=64 with 5 nodes
(block_7_main_ver3.py:334-335) -- and a saved ``A_dense_list`` may hold any matrices.

``RankGroups`` therefore splits the rank's nodes by operator key (geometry or matrix
digest, sample dtype, device) into node batches (``NodeBatch``, each with a subset plan,
plan.make_subset_plan).  A group larger than one batch may hold (max_batch_nodes: 56 nodes
at 2048^2) is split into several batches the same way (C5's 64 nodes on one GPU: 56 + 8).  With one batch -- every BASELINE
config at its GPU count -- the batch IS the rank:
its ``x_ext`` is exchanged in place and nothing else runs.  With several, an edge between
two groups is stored by both and updated bitwise identically at both (the single-y /
two-dual edge math is elementwise and deterministic), and each group's halo rows (other
groups' nodes, remote nodes) are filled from one rank-level image table after the
inter-rank exchange: local rows in, ``HaloExchange.run``, halo rows out -- device copies
of the same bytes, so the run is bitwise the one a single batch would do if the
operators were equal.
"""
from __future__ import annotations

import os
import warnings

import torch

from .exchange import HaloExchange, all_reduce, assemble_stats_device, assemble_stats_parts, gather_images_parts
import torch.distributed as dist

from .plan import STORED_Z_HBM_FRACTION, ShardPlan, make_plan, make_subset_plan, need_stored_z, z_is_stored
from .bounds import BOUND_KEYS, BOUND_STATS, check_bound_run, check_bound_weight, check_bounds
from .fuse import FUSE_KEYS, FUSE_SCALARS, TERM_W, TERM_WD2, TERM_WX, FixedSum, Fuser, check_fuse
from .penalty import NORM_KEYS, NORM_STATS, check_tolerance_run
from .links import check_links_run
from .relax import check_relaxation, check_relaxed_run
from .solver import NodeBatch
from .table import NodeColumns
from ._lib import ADMM_BATCH_KEEP_X


def operator_key(A):
    """Nodes with equal keys share one batch (one projector context)."""
    return (A.geom, A.dtype, A.device)


# smallest batch a concurrent split makes: a full node-interleave vector (8 float32 / 4 float64
# nodes; admm_tomo.hip vb_for) -- narrower batches pay the per-tap address VALU per fewer nodes
SPLIT_MIN = {"float32": 8, "float64": 4}


def max_batch_nodes(geom) -> int:
    """Most nodes one device batch may hold: the library addresses a batch's node-interleaved
    sample buffers with 32-bit offsets (admm_batch_bind: V x max(n, m) x 8 bytes < 2^31), so
    at 2048^2 (n = 4.2 M) that is 63 nodes, rounded down to whole 8-node chunks (the widest
    interleave): 56."""
    cap = ((1 << 31) - 1) // (8 * max(geom.n, geom.m))
    return cap - cap % 8 if cap >= 8 else max(1, cap)


def rank_batches(A_list, plan: ShardPlan, streams: int = 1):
    """The device batches of one rank: [(batch key, its global nodes)] in batch order.  Nodes
    are grouped by operator key; a group larger than one batch may hold is split into
    consecutive cap-sized chunks -- not near-equal: every edge between two batches is stored
    (and updated) by both, and for a dense graph the cross edges |A| x |B| are fewest for the
    most unequal split (C5 on one GPU as 56 + 8 stores 2464 edges, as 32 + 32 it would store
    3040: +36 GB of float64 edge state); at 2048^2 an 8-node batch is two 4-node chunks of 1816
    forward blocks each, so the small batch does not idle the GPU.  ``streams`` > 1: every group
    of at least 2 x SPLIT_MIN nodes is further split into up to that many near-equal
    consecutive parts of >= SPLIT_MIN nodes (RankGroups' concurrent batches)."""
    keys, members = [], {}
    for g in plan.local_nodes:
        k = operator_key(A_list[g])
        if k not in members:
            keys.append(k)
            members[k] = []
        members[k].append(g)
    split = []
    for k in keys:
        cap = max_batch_nodes(k[0])
        nodes = members.pop(k)
        for c0 in range(0, len(nodes), cap):
            split.append((k, c0))
            members[(k, c0)] = nodes[c0:c0 + cap]
    keys = split
    if streams > 1:
        split = []
        for k in keys:
            nodes = members.pop(k)
            parts = max(1, min(streams, len(nodes) // SPLIT_MIN[k[0][1]]))
            c0 = 0
            for q in range(parts):
                sz = len(nodes) // parts + (1 if q < len(nodes) % parts else 0)
                split.append((k[0], (k[1], q)))  # (operator key, batch tag)
                members[(k[0], (k[1], q))] = nodes[c0:c0 + sz]
                c0 += sz
        keys = split
    return [(k, members[k]) for k in keys]


def stored_edges_per_rank(A_list, G, V_total: int, world: int, streams: int = 1, bound_slots: bool = False) -> list[int]:
    """Stored edge slots of every rank of a ``world``-rank run, summed over each rank's device
    batches (rank_batches) -- what the stored-z rule (plan.z_is_stored) weighs.  ``bound_slots``:
    a run with bound constraints stores one more (w, f) row pair per local node."""
    out = []
    for r in range(world):
        pr = make_plan(G, V_total, world, r)
        if not pr.local_nodes:
            out.append(0)
            continue
        extra = len(pr.local_nodes) if bound_slots else 0
        bs = rank_batches(A_list, pr, streams)
        if len(bs) == 1:
            out.append(len(pr.stored_edges) + extra)
        else:
            out.append(sum(len(make_subset_plan(G, V_total, nodes, world, r, pr.ranges, pr.edges).stored_edges)
                           for _, nodes in bs) + extra)
    return out


def min_over_ranks(value: int, world: int, group=None, device=None) -> int:
    """``value`` reduced to its minimum over the ranks of a distributed run (one all-reduce;
    gloo reduces a host tensor, RCCL a tensor on ``device``); the value itself otherwise."""
    if world > 1 and dist.is_available() and dist.is_initialized():
        gloo = dist.get_backend(group) == "gloo"
        t = torch.tensor([int(value)], dtype=torch.int64,
                         device="cpu" if gloo or device is None else torch.device("cuda", device))
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
        return int(t.item())
    return int(value)


def run_hbm_bytes(device, world: int, group=None, collective: bool = True) -> int:
    """HBM of the run's devices: this device's total memory, the minimum over ranks when the run
    is distributed (one all-reduce at setup), so a rule weighed against it is identical on
    every rank even if the devices differ."""
    hbm = int(torch.cuda.get_device_properties(device).total_memory)
    return min_over_ranks(hbm, world, group, device) if collective else hbm


class RankGroups:
    def __init__(self, A_list, G, V_total: int, world: int, rank: int, sinograms, Qij_diag_fn,
                 rho, lam, mu, tv_iters, cg_iters, tv_kind, phantom, fusion="midpoint", Wi_list=None,
                 keep_x=False, group=None, halo=True, streams=1, derive_z=None,
                 stop_norms=False, links=None, relaxation=None, bounds=None, bound_weight=None, ray_weights=None):
        """``links``: None or the run's bool table (iterations, global edges) (links.schedule): every batch gets
        a gate (links.Gate) holding its stored edges' columns, so an edge stored by two batches or two ranks is
        gated alike; ``set_link_row(k)`` before ``exchange_consensus`` picks the iteration.  It needs stored z:
        derived z -- forced, or chosen by the HBM rule -- raises ValueError on every rank alike.
        ``stop_norms``: the run takes the three norms of the scale-free stop test after every
        iteration (``node_norms``; run_admm's eps_abs / eps_rel): three more node columns, and stored z
        -- derived z, forced or chosen by the HBM rule, raises ValueError on every rank alike.
        ``relaxation``: None or alpha in (0, 2): every batch's edge updates and projection run
        over-relaxed (NodeBatch; relax.check_relaxation).  It needs stored z: derived z -- forced, or
        chosen by the HBM rule -- raises ValueError, from run-global facts and so on every rank alike.
        ``bounds`` / ``bound_weight``: the box lo <= x <= hi on every image and kappa of
        q_c,i = kappa * Wi_list[i] (NodeBatch; bounds.check_bounds).  They need stored z and midpoint
        fusion: derived z -- forced, or chosen by the HBM rule, which counts the V extra rows -- and
        weighted fusion raise ValueError, from run-global facts and so on every rank alike.
        ``ray_weights``: per-ray weights of the data term by global node (solver.node_ray_weights);
        every batch takes its own nodes' entries.  ``halo=False``: no inter-rank exchange (bench.py's per-rank proxy: one rank's share
        of a ``world``-rank run on one GPU, its halo rows held fixed).  ``streams`` > 1: every
        operator group of at least 2 x SPLIT_MIN nodes is split into up to that many near-equal
        batches whose x-updates (and edge updates) run concurrently on their own HIP streams,
        so one batch's kernels fill the other's dependent-launch gaps and kernel tails; each
        batch keeps a full node-interleave width (SPLIT_MIN nodes), and the run is bitwise the
        one-batch run (the batch split never changes a node's arithmetic).
        ``derive_z`` None: the run's one edge-state rule (plan.z_is_stored over every rank's
        stored edges) unless ADMM_EDGE_STATE=stored|derived forces it; True / False force
        derived / stored z."""
        self.plan: ShardPlan = make_plan(G, V_total, world, rank)
        self.bounds = check_bounds(bounds, A_list[0].geom.N) if bounds is not None else None
        check_bound_weight(bound_weight, self.bounds)
        forced = os.environ.get("ADMM_EDGE_STATE", "")
        edge_state = {None: None, True: "derived", False: "stored"}[derive_z]
        check_bound_run(self.bounds, fusion, edge_state, forced)
        self.relaxation = check_relaxation(relaxation)
        check_relaxed_run(self.relaxation, edge_state, forced)
        check_links_run(links, edge_state, forced)
        if links is not None and tuple(links.shape[1:]) != (len(self.plan.edges),):
            raise ValueError(f"links: the table has shape {tuple(links.shape)}, the graph has "
                             f"{len(self.plan.edges)} edges")
        self.stop_norms = bool(stop_norms)
        check_tolerance_run(True if self.stop_norms else None, edge_state, forced)
        if not self.plan.local_nodes:
            raise ValueError(f"rank {rank} owns no graph nodes ({V_total} nodes over {world} ranks)")
        self.world = world
        self.group = group
        dev0 = A_list[self.plan.local_nodes[0]].device
        n0 = A_list[self.plan.local_nodes[0]].geom.n
        hbm = run_hbm_bytes(dev0, world, group, collective=halo)
        if streams > 1:
            # a stream split stores every cross-batch edge twice (y, and z when stored): the
            # split is dropped -- on every rank alike, from the busiest rank's extra slots -- when
            # that extra edge state would exceed the stored-z rule's HBM fraction
            extra = max(a - b for a, b in zip(stored_edges_per_rank(A_list, G, V_total, world, streams),
                                              stored_edges_per_rank(A_list, G, V_total, world, 1)))
            if extra * n0 * 16 > STORED_Z_HBM_FRACTION * hbm:
                warnings.warn(f"streams={streams} would store {extra} more edge slots on the busiest rank "
                              f"({extra * n0 * 16 / 2**30:.1f} GiB of float64 edge state): running one batch "
                              f"stream", RuntimeWarning)
                streams = 1
        self.streams_requested = streams
        self.metric_names = ()  # enable_metrics
        self.fuse_mode = None  # enable_fuse
        self.robust = None  # enable_robust
        # the node table's columns (table.py); enable_metrics, enable_robust and enable_fuse widen it
        self.columns = NodeColumns()
        if self.bounds is not None:
            self.columns.add("bounds", BOUND_STATS, lambda nb: [nb.bound_stats], BOUND_KEYS)
        if self.stop_norms:
            self.columns.add("norms", NORM_STATS, lambda nb: [nb.norm_stats], NORM_KEYS)
        bs = rank_batches(A_list, self.plan, streams)
        keys = [k for k, _ in bs]
        members = dict(bs)
        self.fusion = fusion
        if derive_z is None and forced in ("stored", "derived"):
            derive_z = forced == "derived"
        if derive_z is None and fusion == "midpoint":
            derive_z = not z_is_stored(stored_edges_per_rank(A_list, G, V_total, world, streams,
                                                             bound_slots=self.bounds is not None), n0, hbm, fusion)
            need_stored_z(derive_z, self.bounds is not None, self.relaxation is not None, "run", self.stop_norms,
                          links=links is not None)
        self.derive_z = bool(derive_z) if derive_z is not None else False
        devices = {k[0][2] for k in keys}
        if len(devices) > 1:
            raise ValueError("a rank's operators must all live on one device (got "
                             f"{sorted(devices)}): one process per GPU")
        if len(keys) == 1:
            plans = [self.plan]
        else:
            plans = [make_subset_plan(G, V_total, members[k], world, rank, self.plan.ranges, self.plan.edges)
                     for k in keys]
        self.batches = []
        for k, gp in zip(keys, plans):
            geom, dtype, device = k[0]
            self.batches.append(NodeBatch(geom, dtype, gp, sinograms, Qij_diag_fn, rho, lam, mu, tv_iters,
                                          cg_iters, tv_kind, phantom, device, fusion=fusion, Wi_list=Wi_list,
                                          keep_x=keep_x, derive_z=self.derive_z, ray_weights=ray_weights,
                                          bounds=self.bounds, bound_weight=bound_weight,
                                          relaxation=self.relaxation, links=links))
        self.device = self.batches[0].dev
        if len(self.batches) == 1:
            self.x_rank = self.batches[0].x_ext
            self.moves = []
        else:
            n = self.batches[0].x_ext.shape[1]
            self.x_rank = torch.zeros((self.plan.n_xext, n), dtype=torch.float64, device=self.device)
            row = self.plan.xrow
            lt = lambda v: torch.tensor(v, dtype=torch.long, device=self.device)  # noqa: E731
            # (batch, its local rows' slots in x_rank, x_rank slots of its halo rows)
            self.moves = [(nb, lt([row[g] for g in nb.plan.local_nodes]), lt([row[g] for g in nb.plan.halo_nodes]))
                          for nb in self.batches]
        self.halo = HaloExchange(self.plan, self.x_rank, group) if halo else None
        # one stream per batch when several run concurrently (streams > 1)
        self.streams = ([torch.cuda.Stream(device=self.device) for _ in self.batches]
                        if streams > 1 and len(self.batches) > 1 else None)

    def _concurrent(self, fn) -> None:
        """fn(nb) for every batch: in order on the current stream, or (streams > 1) each on its
        own stream, forked from and joined back into the current one."""
        if self.streams is None:
            for nb in self.batches:
                fn(nb)
            return
        cur = torch.cuda.current_stream(self.device)
        fork = cur.record_event()
        for nb, s in zip(self.batches, self.streams):
            s.wait_event(fork)
            with torch.cuda.stream(s):
                fn(nb)
        for s in self.streams:
            cur.wait_stream(s)

    @property
    def single(self) -> bool:
        return len(self.batches) == 1

    @property
    def V(self) -> int:
        return self.plan.V

    def node_update(self, rounds: int | None = None) -> None:
        self._concurrent(lambda nb: nb.node_update(rounds))

    def exchange(self) -> None:
        """Every batch's halo rows <- the current images of their nodes (other batches of
        this rank, other ranks)."""
        for nb, loc, _ in self.moves:
            self.x_rank.index_copy_(0, loc, nb.x_local)
        if self.halo is not None:
            self.halo.run()
        for nb, _, hal in self.moves:
            if hal.numel():
                torch.index_select(self.x_rank, 0, hal, out=nb.x_ext[nb.V:])

    def start_from(self, images) -> None:
        """Start the run from the images ``images[g]`` (float64 (n,) device tensors; at least this
        rank's nodes) instead of x = 0: a fresh ADMM around a consistent (x, z) with zero duals
        (NodeBatch.start_edges).  The local rows are written, every halo and cross-batch row is
        filled by ``exchange()`` -- bitwise its owner's image on every rank -- and each batch then
        forms z (or x_prev) from its x_ext rows.  Collective over the ranks of a distributed run."""
        for nb in self.batches:
            nb.set_local_images(images)
        self.exchange()
        for nb in self.batches:
            nb.start_edges()

    def consensus(self) -> None:
        self._concurrent(lambda nb: nb.consensus())

    def set_link_row(self, k: int) -> None:
        """Iteration ``k``'s gates for every batch's next edge updates (a run with ``links``; host arithmetic
        on a pointer, no device work).  Call before ``exchange_consensus``."""
        for nb in self.batches:
            if nb.gate is not None:
                nb.gate.set_row(k)

    def set_rho(self, rho: float) -> None:
        """Every batch's penalty <- ``rho`` (NodeBatch.set_rho: the scaled duals rescaled, the library's
        sequences recorded again).  Every rank computes the same rho from the same all-reduced
        table, so this needs no collective; an edge stored by two batches is rescaled bitwise alike
        by both."""
        for nb in self.batches:
            nb.set_rho(rho)

    def node_norms(self) -> None:
        """Each batch's ``norm_stats`` <- X2, Z2, U2 of its local nodes after this iteration's edge
        updates and projection, on the batch's stream (a ``stop_norms`` run)."""
        self._concurrent(lambda nb: nb.node_norms())

    @property
    def overlaps_exchange(self) -> bool:
        """exchange_consensus can run the rank-internal edge updates under the halo exchange:
        one batch, stored z, midpoint fusion, an inter-rank exchange, and internal edges (or the
        bound projection, which needs no halo row either)."""
        if self.halo is None or not self.halo.active or not self.single:
            return False
        nb = self.batches[0]
        return nb.z is not None and nb.fusion == "midpoint" and (nb.plan.n_internal > 0 or nb.bounds is not None)

    def exchange_consensus(self) -> None:
        """``exchange()`` then ``consensus()``, with the edges whose endpoints are both local
        (stored slots [0, n_internal), x_ext rows < V) updated while the halo images are in
        flight: the exchange is issued asynchronously (RCCL on its own stream), those edges run
        on the current stream, then the halo rows land and the remaining edges run.  The same
        per-edge kernels and statistics as the serial order, bitwise (a relaxed run's range calls go
        to admm_consensus_relaxed)."""
        if not self.overlaps_exchange or os.environ.get("ADMM_EXCHANGE_OVERLAP", "1") == "0":
            self.exchange()
            self.consensus()
            return
        nb = self.batches[0]
        h = self.halo.start()
        nb.consensus_range(0, nb.plan.n_internal, nb.V)
        if nb.bounds is not None:
            nb.bound_project()  # rank-local: with the internal edges, under the exchange
        self.halo.finish(h)
        nb.consensus_range(nb.plan.n_internal, len(nb.plan.stored_edges), nb.plan.n_xext)

    def enable_metrics(self, names, data_range=None, mask=None) -> None:
        """Score every batch's images against its phantom from now on (metrics.Scorer, one per
        batch: each owns its kernel scratch, so concurrent batches do not share any).  Every rank
        and batch derives the same L and pixel counts from the same phantom and mask."""
        from .metrics import Scorer
        self.metric_names = tuple(names)
        self._metric_mask = mask
        self.columns.remove("metrics")
        if self.metric_names:  # (no name: no column, nothing to concatenate)
            self.columns.add("metrics", len(self.metric_names), lambda nb: [nb.metric_cols],
                             tuple(k for m in self.metric_names for k in (f"{m}_per_node", f"{m}_mean")))
        for nb in self.batches:
            nb.scorer = Scorer(nb.phantom, data_range, mask, device=nb.device, max_images=nb.V)
            nb.metric_cols = None

    def score_images(self) -> None:
        """Each batch's ``metric_cols`` <- the requested metrics of its current local images,
        (V, k) on the device, on the batch's stream."""
        def score(nb):
            nb.metric_cols = nb.scorer.columns(nb.x_local, self.metric_names)
        self._concurrent(score)

    def enable_robust(self, cfg) -> None:
        """The Huber data term by reweighted rays from now on (robust.check_robust's configuration;
        ``reweight``).  Every batch gets weights here, at setup -- the caller's, or all-ones, which are
        bitwise the unweighted batch -- so the weighted launches are recorded once and every later
        refresh is NodeBatch.update_ray_weights.  Each batch gets the kernel's scratch (robust.HuberWeights)
        and its projection buffers (one warm-up projection: the operator's scratch is allocated here,
        not in the loop); the node table gains the block ``robust``: the weighted Huber value and the
        outlier count per node.  The scale form (``scale`` in the configuration) also gives each batch a
        robust.RayQuantile, and the block a third column: the threshold in force, read from the quantile's
        output without a launch.  Explicit-matrix operators raise ValueError before any device work."""
        from .robust import (ROBUST_KEYS, ROBUST_MATRIX_MSG, ROBUST_SCALE_KEYS, ROBUST_SCALE_STATS, ROBUST_STATS,
                             HuberWeights, RayQuantile, check_robust, scale_factor)
        self.robust = check_robust(cfg)
        self.columns.remove("robust")
        if self.robust is None:
            return
        if any(hasattr(nb.geom, "create_ctx") for nb in self.batches):
            raise ValueError(ROBUST_MATRIX_MSG)
        scaled = "scale" in self.robust
        if scaled:
            self.robust_c = scale_factor(self.robust)  # formed once
            self.columns.add("robust", ROBUST_SCALE_STATS, lambda nb: [nb.huber.sums, nb.quant.out[:, 0:1]],
                             ROBUST_SCALE_KEYS)
        else:
            self.columns.add("robust", ROBUST_STATS, lambda nb: [nb.huber.sums], ROBUST_KEYS)
        for nb in self.batches:
            nb.robust_base = nb.ray_weights  # omega: the caller's weights, None for 1
            if nb.ray_weights is None:
                nb.set_ray_weights(torch.ones(nb.geom.m, dtype=torch.float64))
            nb.huber = HuberWeights(nb.geom.m, nb.V, nb.b.dtype, nb.dev)
            if scaled:
                nb.quant = RayQuantile(nb.geom.m, nb.V, nb.b.dtype, nb.dev)
            nb.robust_xs = torch.zeros((nb.V, nb.geom.n), dtype=nb.b.dtype, device=nb.dev)
            nb.robust_ax = torch.empty((nb.V, nb.geom.m), dtype=nb.b.dtype, device=nb.dev)
            nb.project_samples(nb.robust_xs, nb.robust_ax)
        torch.cuda.synchronize(self.device)

    def reweight(self, apply: bool, estimate: bool = True) -> None:
        """Per batch, on its stream: the sample-rounded local images projected with the batch's
        operator, the Huber weights and sums of that residual (``nb.huber.sums``, the block ``robust``),
        and -- ``apply`` -- omega^eff = omega h pushed into the batch for the next x-update
        (NodeBatch.update_ray_weights), after which a keep_x batch forms its kept A^T omega (A x - b) again
        under the new weights (NodeBatch.refresh_kept_start), so that the next update starts as every
        update of a run with fixed weights does.  The scale form: between the projection and the Huber
        kernel -- ``estimate`` (robust.estimates) -- each node's threshold is formed again from this residual
        (admm_ray_quantile; masked are the caller's zeros, never the moving weights), and the Huber kernel
        reads the thresholds in place from the device (admm_huber_weights_dev); without ``estimate`` they
        stay at their last values.  Call where ``score_images`` is called: x is final for the iteration.
        No host synchronisation."""
        cfg = self.robust
        scaled = "scale" in cfg

        def one(nb):
            nb.robust_xs.copy_(nb.x_local)
            nb.project_samples(nb.robust_xs, nb.robust_ax)
            if scaled:
                if estimate:
                    nb.quant.run(nb.robust_ax, nb.b, nb.robust_base, cfg["quantile"], self.robust_c, cfg["delta_min"],
                                 nb._s())
                nb.huber.run(nb.robust_ax, nb.b, nb.robust_base, nb.quant.delta, nb._s())
            else:
                nb.huber.run(nb.robust_ax, nb.b, nb.robust_base, cfg["delta"], nb._s())
            if apply:
                nb.update_ray_weights(nb.huber.w_out)
                if nb.cb.flags & ADMM_BATCH_KEEP_X:  # the next update starts as the plain run's does
                    nb.refresh_kept_start()
        self._concurrent(one)

    def enable_fuse(self, mode, Wi_list=None) -> None:
        """Fuse the network's images from now on (fuse.check_fuse modes; ``fuse_images``): every batch gets
        a fuse.Fuser and, for "precision", its local nodes' rows of ``Wi_list`` as a [V][n] device tensor
        (weighted fusion's ``nb.w`` covers x_ext rows and exists only there); the rank gets the int64
        accumulators, the fused image and -- with a phantom -- the scratch of |xbar - phantom|^2 and of the
        fused image's metrics (a Scorer of its own: the batches' run on their streams).  Dn = fixed_sum(W)
        is static and formed here, once.  Collective over the ranks of a distributed run."""
        from .solver import _as_f64_tensor
        self.fuse_mode = check_fuse(mode)
        self.columns.remove("fuse")
        if self.fuse_mode is None:
            return
        if self.fuse_mode == "precision" and Wi_list is None:
            raise ValueError("fuse='precision' needs Wi_list")
        n = self.batches[0].x_ext.shape[1]
        dev = self.batches[0].dev
        self.columns.add("fuse", 1 + FUSE_SCALARS + len(self.metric_names),
                         lambda nb: [nb.fuser.dev2.view(-1, 1), nb.fuse_scalars],
                         FUSE_KEYS + tuple(f"fused_{m}" for m in self.metric_names))
        for nb in self.batches:
            nb.fuser = Fuser(n, nb.V, dev)
            nb.fuse_w = (torch.stack([_as_f64_tensor(Wi_list[g], n, dev) for g in nb.plan.local_nodes])
                         if self.fuse_mode == "precision" else None)
            # the rank-replicated scalars ride in the row of global node 0 and are zero elsewhere
            nb.fuse_scalars = torch.zeros((nb.V, FUSE_SCALARS + len(self.metric_names)), dtype=torch.float64,
                                          device=dev)
        self._fuse_owner = next(((nb, nb.plan.local_nodes.index(0)) for nb in self.batches
                                 if 0 in nb.plan.local_nodes), None)
        self._fuse_one = Fuser(n, 1, dev)  # one-image launches: finish, |xbar - phantom|^2
        self._fuse_num = FixedSum(n, dev)
        self._fuse_var = None  # the spread's sum, made when asked for
        self.fused = torch.zeros(n, dtype=torch.float64, device=dev)
        self._fuse_se = torch.zeros(1, dtype=torch.float64, device=dev)
        self._fuse_scorer = None
        if self.metric_names:
            from .metrics import Scorer
            nb0 = self.batches[0]
            self._fuse_scorer = Scorer(nb0.phantom, nb0.scorer.data_range, self._metric_mask, device=nb0.device,
                                       max_images=1)
        self._fuse_den = None
        if self.fuse_mode == "precision":
            self._fuse_den = FixedSum(n, dev)
            self._fixed_sum(self._fuse_den, TERM_W, [(nb, None) for nb in self.batches], None)

    def _fixed_sum(self, fs, mode, parts, mean) -> None:
        """``fs`` <- fixed_sum of the terms ``mode`` over ALL graph nodes, ``parts`` = [(batch, its image
        rows)] being this rank's: every batch's absmax, the MAX over ranks, every batch's accumulate into the
        rank's one accumulator, the int64 SUM over ranks.  All on the current stream, one batch after the
        other -- the accumulator has one writer at a time, and the integer sum is exact in any order."""
        fs.zero_()
        for nb, x in parts:
            nb.fuser.absmax(x, nb.fuse_w, mean, mode, fs)
        if self.world > 1 and self.halo is not None:
            all_reduce(fs.bmax, dist.ReduceOp.MAX, self.group)
        for nb, x in parts:
            nb.fuser.accumulate(x, nb.fuse_w, mean, mode, fs, self.plan.V_total)
        if self.world > 1 and self.halo is not None:
            all_reduce(fs.acc, dist.ReduceOp.SUM, self.group)

    def _fuse(self, rows, out) -> None:
        self._fixed_sum(self._fuse_num, TERM_WX, [(nb, rows(nb)) for nb in self.batches], None)
        self._fuse_one.finish(self._fuse_num, self._fuse_den, self.plan.V_total, out)

    def fuse_images(self) -> None:
        """``fused`` <- the fusion of every node's current image, bitwise the same on every rank and for every
        batch split; each batch's ``fuser.dev2`` <- |x_i - xbar|^2 of its local nodes, and the row of global
        node 0 of ``fuse_scalars`` <- |xbar - phantom|^2 and the fused image's metrics.  Call where
        ``score_images`` is called: x is final for the iteration.  No host synchronisation (RCCL; gloo
        stages through the host).  Collective over the ranks of a distributed run."""
        self._fuse(lambda nb: nb.x_local, self.fused)
        for nb in self.batches:
            nb.fuser.deviation(nb.x_local, self.fused)
        nb0 = self.batches[0]
        if nb0.phantom is None or self._fuse_owner is None:
            return
        own, r = self._fuse_owner
        self._fuse_one.deviation(self.fused.view(1, -1), nb0.phantom, out=self._fuse_se)
        own.fuse_scalars[r, 0:1].copy_(self._fuse_se)
        if self._fuse_scorer is not None:
            own.fuse_scalars[r, 1:].copy_(self._fuse_scorer.columns(self.fused.view(1, -1), self.metric_names)[0])

    def fused_image(self, feasible: bool = False, spread: bool = False):
        """(xbar, spread or None) of the current images -- ``feasible`` (a run with bounds): of the constraint
        copies w_i, a convex combination of box-feasible images, clipped to the box so that a last-ulp
        rounding of the quotient cannot leave it -- as fresh (n,) device tensors."""
        if feasible and self.bounds is None:
            raise ValueError("feasible images need bounds")
        rows = (lambda nb: nb.w_bound) if feasible else (lambda nb: nb.x_local)
        mean = torch.empty_like(self.fused)
        self._fuse(rows, mean)
        if feasible:
            # Nn and Dn are rounded independently, so where every w_i sits on a bound their quotient may
            # leave the box by an ulp: the promise "inside the box exactly" is kept by the box's own clip
            mean = self.batches[0].projector.clip(mean.view(1, -1)).reshape(-1).contiguous()
        if not spread:
            return mean, None
        if self._fuse_var is None:
            self._fuse_var = FixedSum(mean.numel(), mean.device)
        self._fixed_sum(self._fuse_var, TERM_WD2, [(nb, rows(nb)) for nb in self.batches], mean)
        sp = self._fuse_one.finish(self._fuse_var, self._fuse_den, self.plan.V_total, torch.empty_like(mean), root=True)
        return mean, sp

    def _node_stats(self, nb):
        """The batch's rows of the node table: its ``columns`` side by side (table.py states the order);
        ``nb.node_stats`` itself, no device work, when no feature widens the table."""
        cols = self.columns.sources(nb)
        return torch.cat(cols, 1) if len(cols) > 1 else nb.node_stats

    @property
    def fuse_width(self) -> int:
        """The fusion's node-table columns: dev2, |xbar - phantom|^2 and one per metric; 0 when off."""
        return self.columns.width_of("fuse")

    @property
    def node_stat_width(self) -> int:
        """Columns of the node table ``stats_device`` assembles."""
        return self.columns.width

    def stats(self, extra=None):
        """Global node / edge statistics; ``extra`` (rank-local [V, k] numpy, rows in
        plan.local_nodes order) is appended to the node statistics."""
        parts = []
        for nb in self.batches:
            ns = self._node_stats(nb)
            if extra is not None:
                rows = [self.plan.local_nodes.index(g) for g in nb.plan.local_nodes]
                ex = torch.as_tensor(extra[rows], dtype=torch.float64, device=ns.device)
                ns = torch.cat([ns, ex], dim=1)
            parts.append((nb.plan, ns, nb.edge_stats[: len(nb.plan.stored_edges)]))
        return assemble_stats_parts(self.plan.V_total, len(self.plan.edges), self.world, parts, self.group)

    def stats_device(self) -> torch.Tensor:
        """The global statistics table on the device (exchange.assemble_stats_device): no
        host synchronisation."""
        parts = [(nb.plan, self._node_stats(nb), nb.edge_stats[: len(nb.plan.stored_edges)]) for nb in self.batches]
        return assemble_stats_device(self.plan.V_total, len(self.plan.edges), self.world, parts, self.group)

    def local_images(self):
        """[(global node, image row tensor)] of this rank's nodes, ascending."""
        out = []
        for nb in self.batches:
            out.extend((g, nb.x_local[r]) for r, g in enumerate(nb.plan.local_nodes))
        return sorted(out, key=lambda t: t[0])

    def images(self, feasible: bool = False) -> torch.Tensor:
        """Every node's image x_i; ``feasible`` (a run with bounds): its constraint copy w_i, which
        lies in the box exactly."""
        if feasible and self.bounds is None:
            raise ValueError("feasible images need bounds")
        return gather_images_parts(self.plan.V_total, self.world,
                                   [(nb.plan, nb.w_bound if feasible else nb.x_local) for nb in self.batches],
                                   self.group)
