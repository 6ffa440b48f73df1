"""Decentralized edge-split ADMM loop on MI355X (the reference's block_6 hot path).

``run_admm`` implements /root/reference/block_6_admm_loop_ver2.py:15-326 with
the node solves and edge updates on the GPU:

  for k in range(max_iters):                         (:69)
      x-update of every local node   -> NodeBatch.node_update   (:81-187)
      halo exchange of x_j           -> HaloExchange.run (RCCL)
      z/y update + residual partials -> NodeBatch.consensus     (:210-253)
      statistics -> history, stop test                          (:189-206,255-289)

Histories carry the reference's keys (:310-326), plus ``sb_res_history`` (the
split-Bregman stationarity residual ||A^T(Ax-b) + rho(Dx-c) + mu K^T e|| of each
accepted x) and ``inner_updates_history`` (x-updates spent per node).

Inner-solve control (row a5).  Default (``inner_tol=None``): one fixed-count x-update
(tv_iters x cg_iters) per node per iteration, deterministic; ``eps_used_history`` is NaN
because no tolerance is applied.  ``inner_tol="reference"``: the accept / tighten loop of
:100-176 -- the node is solved to eps_try = min(1e-2, eps_target(k)) (repeated warm
x-updates until its split-Bregman residual <= eps_try, at most ``max_inner_updates`` per
solve, standing in for SCS's tolerance), accepted if the reference's ||g|| <= eps_target,
else eps_try /= 5 and re-solved, at most twice, then force-accepted; eps_used is the
eps_try of the accepted iterate.  Other nodes' state is untouched while one node
re-solves (masked batch updates).  Nodes may have different operators (the reference's
own angle split gives unequal counts, block_2_load_odl_data.py:31-38; matrix lists may
hold any matrices): each distinct operator is one device batch (groups.RankGroups).
One process per GPU: when
``torch.distributed`` is initialised with world size > 1 the graph nodes are
sharded (plan.py) and every rank returns the same ``(x_list, history)``.
"""
from __future__ import annotations

import math
import os
from datetime import datetime

import numpy as np
import torch
import torch.distributed as dist

from .bounds import BOUND_STATS, check_bound_run, check_bound_weight, check_bounds
from .exchange import split_stats
from .fuse import FUSE_SCALARS, check_fuse
from .fbp import FILTERS, fbp
from .geometry import CSR_WEIGHTS_MSG, RayTransform
from .groups import RankGroups
from .solver import node_ray_weights
from ._lib import EDGE_STATS
from .matrix import MatrixOperator, as_operators
from .links import check_links, check_links_run, describe, link_age_max, links_up, schedule
from .relax import check_relaxation, check_relaxed_run
from .robust import ROBUST_MATRIX_MSG, applies, check_robust, estimates
from .penalty import (NORM_KEYS, balance, check_adapt_rho, check_stop_tolerances, check_tolerance_run,
                      incidences, thresholds)
from .table import DZ2, G2, IMG, MSE_SINO, QUAD, RA2, RB2, SBRES2, TV
from .table import EXTRA_KEYS, HISTORY_KEYS  # noqa: F401  (the core block's keys; importers find them here)
from .metrics import check_data_range, check_metrics, check_side, _check_mask_shape

DEFAULT_MU_FACTOR = 10.0  # split-Bregman penalty mu = 10 * lam_tv
EPS_CAP, CALIB_ALPHA, MAX_TIGHTEN = 1e-2, 1.0, 2  # block_6_admm_loop_ver2.py:106-113
PIPELINE_BLOCK = 64  # iterations of statistics held on the device in the pipelined mode


def eps_target(k: int) -> float:
    """block_6_admm_loop_ver2.py:101-103."""
    return 2.0 / ((k + 1) ** 1.005)


def _check_operators(A_list, N):
    """Every entry an admm_hip operator on an N x N image.  Nodes may have different
    operators (unequal angle counts, different matrices): RankGroups batches equal ones."""
    for A in A_list:
        if not isinstance(A, (RayTransform, MatrixOperator)):
            raise TypeError(
                "A_dense_list entries must be admm_hip operators (RayTransform, MatrixOperator) "
                f"or matrices; got {type(A).__name__}")
        if A._adjoint:
            raise ValueError("A_dense_list entry is an adjoint view")
        if A.geom.N != N:
            raise ValueError(f"N={N} does not match an operator's N={A.geom.N}")


def _dist_info(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def run_admm(A_dense_list, sinograms, G, Wi_list, Qij_diag_fn, N, lam_tv=0.01, rho=1.0,
             max_iters=10, eps_pri=1e-1, eps_dual=1e-1, verbose=True, snapshot_dir=None,
             snapshot_every=None, snapshot_div=10, phantom_true=None, mu=None, tv_iters=10,
             cg_iters=5, tv_kind="iso", group=None, return_tensors=False, timing=None,
             write_params=True, fusion="midpoint", inner_tol=None, max_inner_updates=10,
             inner_chunks=None, chunk_snapshot_dir=None, chunk_save_every=1, inspect=None,
             pipeline=None, streams=1, edge_state=None, x_init=None, fuse=None, fuse_out=None, robust=None,
             links=None, metrics=None, data_range=None,
             metrics_mask=None, adapt_rho=None, eps_abs=None, eps_rel=None, relaxation=None, bounds=None,
             bound_weight=None, return_feasible=False, ray_weights=None):
    """``links``: None (default: every edge of G updates in every iteration), a real p in (0, 1], a dict or a
    bool array: unreliable links (admm_hip/links.py, csrc/links.hip).  At iteration k every
    edge is up or down.  An up edge performs exactly today's z / y update (relaxed with ``relaxation``, the
    weighted form with fusion="weighted"); a down edge keeps its y, z (and y_b) bit for bit, both endpoints
    go on with the last (z, y) they hold, and its three sums are |x_a - z|^2, |x_b - z|^2 -- the true
    disagreement with the last agreed z -- and 0.  Every node runs its x-update every iteration; the
    constraint slot of a run with ``bounds`` is node-local and always updated; ``primal``, ``dual``, the
    per-node arrays, the stop tests, ``adapt_rho`` and the stop norms keep their definitions and read the same
    tables; a change of rho rescales the scaled duals of down edges too.  p: every edge is up independently
    with probability p in every iteration (seed 0; 1.0 is None).  A dict with any of ``p`` (1.0), ``seed``
    (0), ``max_age`` (None or an int >= 1: an edge that has been down that many iterations in a row is forced
    up, the bounded-delay model) and ``outages`` (a list of (a, b, k0, k1): edge {a, b} is down for
    k0 <= k < k1, k1=None for good), applied in that order -- an outage wins --; a dict that leaves every
    edge up in every iteration is None.  A bool array (rows >= max_iters, E) is used as it is, columns in the
    run's edge order (``admm_hip.links.edge_list(G)``).  The random table is
    ``np.random.default_rng([seed, 0x4C4E4B53]).random((max_iters, E)) < p`` (``admm_hip.links.schedule``
    returns the table of any value), the same on every rank.  The gates live on the device (one byte per
    edge and iteration, uploaded once), so the pipelined mode stays available.  The history gains
    ``links_up`` (up edges per iteration) and ``link_age_max`` (after each iteration, the largest number of
    iterations since an edge's last update), host arithmetic on the table.  Randomised edge activation
    converges almost surely to the same fixed point if every edge is up with positive probability (Iutzeler et
    al., CDC 2013; stated for exact node solves); expect about 1 / p times the iterations.  A bool, NaN,
    p <= 0 or p > 1, unknown keys, max_age < 1, an outage that names a non-edge or has k1 <= k0, and an array
    of the wrong width or with too few rows raise ValueError on the host, on every rank alike.  Needs stored
    z (ValueError with derived z, forced or chosen by the HBM rule: a derived z has no per-edge age).  With
    links=None nothing changes: no launch, no buffer, no history key.
    ``robust``: None (default), a real delta > 0 (inf allowed) or a dict with ``delta`` (required),
    ``every`` (1: reweight every this many iterations) and ``until`` (None; else after that many iterations
    the weights stay as they are): the data term of every node becomes the Huber loss
    sum_r omega_r psi_delta((A x - b)_r), psi_delta(a) = a^2 / 2 for |a| <= delta and delta |a| - delta^2 / 2
    beyond, minimised by iteratively reweighted rays (admm_hip/robust.py, csrc/robust.hip).
    After every iteration's last x-update (``inner_tol`` / ``inner_chunks`` solves included) the residual
    r = A x_i - b_i of every node gives h_r = 1 where |r_r| <= delta, else delta / |r_r|, and -- when
    (k + 1) % every == 0 and k + 1 <= until -- the next iteration's x-update runs with omega h (omega: the
    caller's ``ray_weights``, or 1; iteration 0 runs with omega, plain least squares; the precisions W_i,
    Q_ij stay those of the caller's weights).  Every iteration records ``robust_loss_per_node`` /
    ``robust_loss_total`` (the weighted Huber value of the iteration's images) and
    ``robust_outliers_per_node`` / ``robust_outliers_total`` (unmasked rays beyond delta).  ``mse_sino_*``
    keeps its definition -- the weighted sum under the weights the update ran with -- so ``obj_*`` is the
    value of the quadratic surrogate, not of the Huber objective.  The values ride in node-table columns
    and the weights are refreshed on the device, so the pipelined mode stays available.  Geometry
    operators only; a bool, NaN, delta <= 0, unknown keys and ``every`` < 1 raise ValueError on the host,
    on every rank alike.  With robust=None nothing changes: no launch, no buffer, no column, no history key.
    The self-scaling form: a dict with ``scale`` (a finite real > 0; no default) in place of
    ``delta``, and optionally ``quantile`` (0.5), ``delta_min`` (0.0) and ``consistency`` (1.4826): every
    iteration each node's threshold is delta_i = max(scale * consistency * a_k, delta_min), a_k the
    floor(quantile (cnt - 1))-th smallest |A x_i - b_i| among the cnt rays the caller's ``ray_weights`` do not
    mask (the lower median) -- an exact order statistic found on the device (csrc/scale.hip) and read by the
    Huber kernel from device memory, no host synchronisation; a zero or non-finite estimate gives
    delta_i = inf (least squares), never 0.  The estimate is refreshed while k + 1 <= until (always at
    k = 0), then kept; until it is frozen a moving delta gives up the fixed-delta descent guarantee of
    majorise-minimise.  The history gains ``robust_delta_per_node`` (the thresholds formed from the
    iteration's images); loss and outliers are reported at the threshold in force.
    ``fuse``: None (default), "uniform" or "precision": after every iteration's x-update the network's
    images are fused on the GPU into xbar = (sum_i W_i x_i) / (sum_i W_i) per pixel over all graph nodes
    (W = Wi_list; "uniform": W = 1, the plain mean) and the history gains ``consensus_err`` =
    sqrt(sum_i |x_i - xbar|^2) -- unlike ``primal`` independent of the graph and its edge count --,
    ``consensus_err_per_node`` (|x_i - xbar|, one V_total array per iteration), ``fused_img_mse`` =
    |xbar - phantom|^2 (a sum like ``img_mse_*``; NaN without a phantom) and, with ``metrics``,
    ``fused_psnr`` / ``fused_ssim`` of xbar (same data_range and mask).  The sums over nodes are fixed-point
    (admm_hip/fuse.py, csrc/fuse.hip): exact, so every value is bitwise the same for any rank count, batch
    split and ``streams``; their resolution is 2 V^2 B 2^-61 with B the largest |W_i x_i| of the network.
    The values ride in node-table columns, so the pipelined mode keeps its freedom from host
    synchronisation.  ``fuse_out``: a dict that receives ``"image"`` (the fusion of the returned images: of
    w_i with ``return_feasible``) and ``"spread"`` (their per-pixel weighted standard deviation across
    nodes) as (N, N) arrays, or device tensors with ``return_tensors``; bitwise
    ``admm_hip.fuse_images(x_list, Wi_list, spread=True)``.  Works with every other keyword (the feature
    only reads images).  Anything else raises ValueError on the host.  With fuse=None nothing changes: no
    launch, no buffer, no column, no history key, no collective.
    ``adapt_rho``: None / False (default: one fixed rho), True, or a dict with any of ``ratio`` (10, > 1),
    ``factor`` (2, > 1), ``every`` (1), ``until`` (None: always; else no change after that many
    iterations), ``rho_min`` / ``rho_max`` (rho / 1024, rho * 1024): residual balancing (Boyd et al.
    3.4.1).  After iteration k (when (k + 1) % every == 0 and k + 1 <= until) rho is multiplied by factor
    where r > ratio * s and divided by it where s > ratio * r, clamped to [rho_min, rho_max]; r, s are
    ``primal``, ``dual`` (with bounds sqrt(primal^2 + bound_primal^2), sqrt(dual^2 + bound_dual^2)); a
    residual that is not finite changes nothing.  A change rescales the scaled duals by rho_old /
    rho_new (exact for factor 2) and re-records the batches' launch sequences (RankGroups.set_rho,
    admm_batch_set_rho); every rank derives the same rho from the same table.  ``dual``, ``bound_dual``
    and ``dual_per_node`` use the rho the iteration ran with; the history gains ``rho_history`` (that
    rho, one per iteration).  From rho_0 a factor 400 off it needs fewer iterations than the hand-tuned
    rho.  Works with either edge state.  Bad values raise ValueError on the host.
    ``eps_abs`` / ``eps_rel``: None (default: the absolute test ``eps_pri`` / ``eps_dual``) or finite reals
    >= 0, not both 0: the scale-free stop test of Boyd et al. (3.12) replaces the absolute one
    (``eps_pri`` / ``eps_dual`` are then not consulted): stop when r < eps_pri_k and s < eps_dual_k, r and s
    as above, eps_pri_k = sqrt(n sum_i ninc_i) eps_abs + eps_rel max(||Ax||, ||Bz||), eps_dual_k =
    sqrt(n V_total) eps_abs + eps_rel ||A^T y||, ninc_i = node i's incidences (degree, + 1 with bounds),
    the norms those of the stacked constraint after the iteration's edge updates and projection
    (admm_node_norms, three more columns of the node table; penalty.thresholds).  The history gains
    ``eps_pri_history``, ``eps_dual_history``, ``ax_norm``, ``bz_norm``, ``aty_norm`` (the unscaled dual's:
    rho_k ||A^T u||).  Needs stored z (ValueError with derived z, forced or chosen by the HBM rule).
    Either keyword forces the per-iteration read-back (no pipelined mode).  With all three None
    nothing changes: no launch, no buffer, no history key.
    ``relaxation``: None (default) or alpha in the open interval (0, 2): over-relaxation of the
    consensus step (Eckstein-Bertsekas; Boyd et al. 3.4.3).  In the z- and y-updates of every edge
    (and in the projection of a run with ``bounds``) x_i is replaced by alpha x_i + (1 - alpha) z_old
    (admm_consensus_relaxed, admm_bound_project_relaxed; either fusion).  The
    residuals keep the true x_i, so ``primal``, ``dual``, the per-node arrays and the stop test keep
    their definitions, and the run reaches the same fixed point.  Recommended: 1.5 - 1.8 (with the
    fixed-count x-update 1.6 needs about 0.63 x, 1.8 about 0.56 x the iterations of alpha = 1 to a
    given residual; values near 2 oscillate with the inexact inner solve); alpha < 1
    under-relaxes.  A bool, NaN, alpha <= 0 and alpha >= 2 raise ValueError on the host, on every rank
    alike.  Needs stored z: with edge_state="derived", ADMM_EDGE_STATE=derived, or where the HBM
    rule picks derived z the run is refused with ValueError (a relaxed z is not the midpoint of the
    endpoint images).  None and 1.0 change nothing: no launch, no buffer, no history key, bitwise
    the same results.
    ``bounds``: None or (lo, hi): the box lo <= x_i <= hi on every node's image; each of lo, hi is
    None (that side off), a scalar, or an (N, N) / (n,) array shared by all nodes (a support mask is
    hi = 0 outside the support); NaN and lo > hi anywhere raise ValueError on the host.  Node i gets
    the splitting x_i = w_i, w_i in the box: one more quadratic term (rho / 2) ||x_i - (w_i - f_i)||^2
    weighted by q_c,i = ``bound_weight`` * Wi_list[i] (kappa, default 1, > 0) in its x-update, and after
    the edge updates w_i = clip(x_i + f_i), f_i += x_i - w_i (admm_bound_project; exact in the limit,
    rank-local).  The history gains ``bound_primal`` = sqrt(sum_i |x_i - w_i|^2), ``bound_dual`` =
    rho sqrt(sum_i |w_i - w_i_old|^2), ``bound_violation`` = sqrt(sum_i |x_i - clip(x_i)|^2) and the
    per-node arrays ``bound_pri_per_node`` / ``bound_violation_per_node`` (the sums, not their roots);
    ``primal`` and ``dual`` keep the reference's edge-only definition; the stop test additionally
    requires bound_primal < eps_pri and bound_dual < eps_dual; ``obj_per_node`` / ``obj_total`` then
    include the constraint's quadratic term (ADMM_NODE_STAT_QUAD: it is part of the node's
    subproblem).  Needs stored z and fusion="midpoint" (ValueError otherwise, on every rank alike).
    ``return_feasible=True`` returns w_i, inside the box exactly, instead of x_i.  With bounds=None
    nothing changes: no slot, no launch, no table column, no history key.
    ``ray_weights``: per-ray weights omega of the data term, 1/2 sum_r omega_r (A x - b)_r^2
    (weighted least squares; omega = 0 masks a ray): None, one (m,) / (angles, det) array for every
    node, or one entry (array, tensor or None) per graph node; finite and >= 0, checked on the host
    before any device work; geometry operators only.  ``sino_mse`` then records the weighted sum.
    With None nothing changes: no call, no buffer, identical histories.
    ``metrics``: None, or a subset of ("psnr", "ssim"): after every iteration's x-update each
    node's image is scored against ``phantom_true`` (required then) on the GPU (admm_hip.metrics,
    admm_image_metrics on the batch's stream) and the history gains ``psnr_per_node`` / ``psnr_mean``
    and / or ``ssim_per_node`` / ``ssim_mean`` (one V_total array / its mean per iteration); the
    values ride in extra columns of the node-statistics table, so the pipelined mode stays free of
    host synchronisation.  ``data_range``: L of both (default phantom.max() - phantom.min(), > 0);
    ``metrics_mask``: (N, N) or (n,), nonzero = pixel counted (default all).  With ``metrics=None``
    nothing changes: no launch, no table column, no history key.
    ``x_init``: where the run starts.  None: x = 0, z = 0 (the reference, _ver2:35-43).
    "fbp" or "fbp:<filter>" (admm_hip.fbp.FILTERS): node g starts from the filtered back
    projection of its own sinogram, ``A_g.fbp(sinograms[g], filter)``.  A list, array or tensor of
    one image per graph node, (N, N) or (n,): node g starts from entry g (converted to float64).
    Either way the run is a fresh ADMM around those images: y = 0, d = e = 0 and
    z_e = (x_a + x_b) / 2 (weighted fusion: the W-weighted mean) -- groups.RankGroups.start_from.
    ``edge_state``: "stored" / "derived" z (None: the run's rule, plan.z_is_stored --
    stored wherever it fits; ADMM_EDGE_STATE in the environment forces it too).
``inner_chunks``: split each x-update into warm-started solves of these round counts
    (block_6_admm_loop.py:14-69 chunked SCS); ``chunk_snapshot_dir`` then receives that
    file's per-chunk snapshots (``_chunk_snapshot``) every ``chunk_save_every`` chunks.
    ``inspect(rg)``: called with the rank's device state (groups.RankGroups) after the loop
    (tests check the edge invariants on the device arrays).  ``pipeline``: read the
    statistics back once after the loop instead of every iteration (default: whenever the
    stop test cannot fire and no per-iteration host output is requested; False forces the
    per-iteration read-back).  ``streams``: concurrent node batches per rank (groups.RankGroups;
    bitwise the same run).  In the pipelined mode the device keeps the statistics of at most
    ``PIPELINE_BLOCK`` iterations (V_total x 8 + E x 3 float64 each) and flushes them to the host
    every ``PIPELINE_BLOCK`` iterations, so the verbose progress lines of those iterations are
    printed at each flush (and at the end), not as each iteration finishes."""
    if inner_tol not in (None, "reference"):
        raise ValueError("inner_tol must be None (fixed counts) or 'reference'")
    if inner_chunks is not None:
        inner_chunks = [int(r) for r in inner_chunks]
        if not inner_chunks or min(inner_chunks) < 1:
            raise ValueError("inner_chunks must be a non-empty list of positive round counts")
        if inner_tol is not None:
            raise ValueError("inner_chunks and inner_tol are exclusive")
        tv_iters = inner_chunks[0]
    # argument errors on every rank alike, before any operator is built on the device
    metrics = _check_metric_args(metrics, data_range, metrics_mask, phantom_true, N)
    bounds = check_bounds(bounds, N)
    bound_weight = check_bound_weight(bound_weight, bounds)
    forced = os.environ.get("ADMM_EDGE_STATE", "")
    check_bound_run(bounds, fusion, edge_state, forced)
    if return_feasible and bounds is None:
        raise ValueError("return_feasible needs bounds=(lo, hi)")
    relaxation = check_relaxation(relaxation)
    check_relaxed_run(relaxation, edge_state, forced)
    links = check_links(links)
    link_table = None
    if links is not None:
        link_table = schedule(G, max_iters, links)  # (the outages' edges and an array's shape are checked here)
        if not isinstance(links, np.ndarray) and bool(link_table.all()):
            links = link_table = None  # every edge up in every iteration: the run without the keyword
    check_links_run(links, edge_state, forced)
    adapt = check_adapt_rho(adapt_rho, rho)
    tol = check_stop_tolerances(eps_abs, eps_rel)
    check_tolerance_run(tol, edge_state, forced)
    fuse = check_fuse(fuse)
    robust = check_robust(robust)
    if fuse is None and fuse_out is not None:
        raise ValueError("fuse_out needs fuse='uniform' or 'precision'")
    if fuse_out is not None and not isinstance(fuse_out, dict):
        raise ValueError("fuse_out must be a dict (it is filled like timing)")
    if fuse == "precision" and Wi_list is None:
        raise ValueError("fuse='precision' needs Wi_list")
    V_total = len(A_dense_list)
    # matrices (the reference's dense A_dense_list; dense numpy / torch, scipy.sparse)
    # become explicit-matrix operators (matrix.py); operators pass through
    A_dense_list = as_operators(A_dense_list, N=N)
    _check_operators(A_dense_list, N)
    if sorted(G.nodes()) != list(range(V_total)):
        raise ValueError("graph nodes must be 0..num_nodes-1")
    mu = DEFAULT_MU_FACTOR * lam_tv if mu is None else float(mu)
    if not mu > 0:
        raise ValueError("mu must be > 0 (set lam_tv > 0 or pass mu explicitly)")
    start = _parse_x_init(x_init, A_dense_list, V_total, N)  # argument errors on every rank alike
    if ray_weights is not None:
        for g, A in enumerate(A_dense_list):
            if node_ray_weights(ray_weights, [g], A.geom.m) is not None and hasattr(A.geom, "create_ctx"):
                raise ValueError(CSR_WEIGHTS_MSG)
    if robust is not None and any(hasattr(A.geom, "create_ctx") for A in A_dense_list):
        raise ValueError(ROBUST_MATRIX_MSG)
    world, rank = _dist_info(group)
    torch.cuda.set_device(A_dense_list[0].device)
    if snapshot_dir is not None:
        os.makedirs(snapshot_dir, exist_ok=True)
    if snapshot_every is None:
        snapshot_every = max(1, max_iters // snapshot_div)  # _ver2:31-32
    rg = RankGroups(A_dense_list, G, V_total, world, rank, sinograms, Qij_diag_fn, rho, lam_tv, mu,
                    tv_iters, cg_iters, tv_kind, phantom_true, fusion=fusion, Wi_list=Wi_list,
                    keep_x=inner_tol is None, group=group, streams=streams,  # this loop never writes x itself
                    derive_z=None if edge_state is None else {"stored": False, "derived": True}[edge_state],
                    ray_weights=ray_weights, bounds=bounds, bound_weight=bound_weight if bounds is not None else None,
                    relaxation=relaxation, stop_norms=tol is not None, links=link_table)
    # (masked re-solves of the tolerance mode restore x rows, so that mode re-projects x)
    plan = rg.plan
    if start is not None:
        rg.start_from(_initial_images(start, A_dense_list, sinograms, plan.local_nodes, rg.device))
    if metrics:
        rg.enable_metrics(metrics, data_range, metrics_mask)
    if robust is not None:
        rg.enable_robust(robust)
    if fuse is not None:
        rg.enable_fuse(fuse, Wi_list)  # (after the metrics: the fused image is scored like the nodes')
    if world > 1:
        dist.barrier(group=group)
    hist = {}
    record = _Recorder(hist, rg.columns, plan.edges, V_total, lam_tv, phantom_true is not None, metrics,
                       incidences(plan.edges, V_total, bounds is not None) if tol is not None else None, tol, N * N)
    if adapt is not None:
        hist["rho_history"] = []  # (the loop's own key, after the blocks': the dict's order is no promise)
    rho_k = rho  # the rho the next iteration runs with (adapt_rho moves it)
    rho_changes = 0
    if verbose and rank == 0:
        print(f"Max ADMM Iteration in Block-6 B4 Loop = {max_iters}")
    torch.cuda.synchronize()
    t_loop = None
    if timing is not None:
        import time
        t_loop = time.perf_counter()
    iters_done = 0
    # Pipelined statistics: when the stop test cannot fire (eps_pri <= 0 or eps_dual <= 0:
    # primal / dual are norms) and nothing else needs host values per iteration, each
    # iteration's statistics table is assembled on the device (RCCL all-reduce at N > 1) into
    # a row of a device history and read back once after the loop -- no host synchronisation
    # per iteration, so the next iteration's launches queue behind the current one.  The
    # histories are computed from the same values by the same host code (bitwise equal).
    pipelined = ((eps_pri <= 0 or eps_dual <= 0) and inner_tol is None and snapshot_dir is None
                 and chunk_snapshot_dir is None and pipeline is not False and adapt is None and tol is None)
    dev_hist = None
    flushed = 0  # iterations of the pipelined statistics already recorded on the host
    for k in range(max_iters):
        et = eps_target(k)
        if inner_chunks is None:
            rg.node_update()
        else:
            for cid, rounds in enumerate(inner_chunks):
                rg.node_update(rounds=rounds)
                if chunk_snapshot_dir is not None and cid % int(chunk_save_every) == 0:
                    _chunk_snapshot(chunk_snapshot_dir, k, cid, rg, N)
        eps_used = np.full(plan.V, np.nan)
        n_upd = np.ones(plan.V)
        if inner_tol == "reference":
            for nb in rg.batches:
                rows = [plan.local_nodes.index(g) for g in nb.plan.local_nodes]
                eps_used[rows], n_upd[rows] = _solve_to_reference_tolerance(nb, et, max_inner_updates)
        if metrics:
            rg.score_images()  # x is final for this iteration: the consensus writes z and y only
        if fuse is not None:
            rg.fuse_images()
        if robust is not None:  # the Huber sums of this iteration's images; the next update's weights
            rg.reweight(applies(robust, k), estimates(robust, k))
        if link_table is not None:
            rg.set_link_row(k)  # this iteration's gates: a row of the device table, no host synchronisation
        rg.exchange_consensus()  # (rank-internal edges under the halo exchange)
        if tol is not None:
            rg.node_norms()  # z, y (w, f) are final for this iteration
        iters_done = k + 1
        if pipelined:
            flat = rg.stats_device()
            if dev_hist is None:
                dev_hist = torch.empty((min(max_iters, PIPELINE_BLOCK), flat.numel()), dtype=torch.float64,
                                       device=flat.device)
            dev_hist[k - flushed].copy_(flat)
            if k + 1 - flushed == dev_hist.shape[0]:  # block full: flush to the host
                flushed = _flush_pipelined(record, dev_hist, flushed, k + 1, rho, verbose and rank == 0)
            continue
        ns, es = rg.stats(np.stack([eps_used, n_upd], axis=1))  # (the loop's two columns, gathered with the table)
        ns, w = ns.numpy(), rg.columns.width
        pn, dn, bres, eps = record(k, ns[:, :w], es.numpy(), rho_k, ns[:, w], ns[:, w + 1])
        if snapshot_dir is not None and ((k + 1) % snapshot_every == 0):
            _snapshot(snapshot_dir, k, rg, N)
        if verbose and rank == 0 and k % 10 == 0:
            print(f"iter {k}, primal {pn:.3e}, dual {dn:.3e}")
        if adapt is not None or tol is not None:  # the stacked residuals: the constraint's rows included
            r_k = pn if bres is None else math.sqrt(pn * pn + bres[0] * bres[0])
            s_k = dn if bres is None else math.sqrt(dn * dn + bres[1] * bres[1])
        if adapt is not None:
            hist["rho_history"].append(float(rho_k))
        if tol is not None:
            stop = r_k < eps[0] and s_k < eps[1]
        else:
            stop = pn < eps_pri and dn < eps_dual and (bres is None or (bres[0] < eps_pri and bres[1] < eps_dual))
        if stop:
            if verbose and rank == 0:
                print(f"stopped at iter {k}, primal {pn:.3e}, dual {dn:.3e}")
            break
        if adapt is not None and k + 1 < max_iters:  # (after the last iteration no update follows)
            rho_new = balance(rho_k, r_k, s_k, adapt, k)
            if rho_new != rho_k:
                rg.set_rho(rho_new)
                rho_k = rho_new
                rho_changes += 1
    if pipelined and dev_hist is not None and iters_done > flushed:
        flushed = _flush_pipelined(record, dev_hist, flushed, iters_done, rho, verbose and rank == 0)
    torch.cuda.synchronize()
    if link_table is not None:  # host arithmetic on the table, trimmed to the iterations run
        hist["links_up"] = [int(v) for v in links_up(link_table[:iters_done])]
        hist["link_age_max"] = [int(v) for v in link_age_max(link_table[:iters_done])]
    if timing is not None:
        import time
        timing["loop_s"] = time.perf_counter() - t_loop
        timing["iters"] = iters_done
        timing["V_total"] = V_total
    if write_params and rank == 0:
        _write_params(snapshot_dir, rho_k, lam_tv, V_total, mu, tv_iters, cg_iters, relaxation,
                      (rho, adapt, rho_changes) if adapt is not None else None, fuse, robust,
                      describe(links, link_table[:iters_done]) if link_table is not None else None)
    if inspect is not None:
        inspect(rg)
    if fuse is not None and fuse_out is not None:  # the returned images' fusion and spread: after the loop's clock
        xbar, sp = rg.fused_image(feasible=bool(return_feasible), spread=True)
        for key, t in (("image", xbar), ("spread", sp)):
            fuse_out[key] = t.view(N, N) if return_tensors else t.to("cpu").numpy().reshape(N, N)
    X = rg.images(feasible=bool(return_feasible))
    if return_tensors:
        return [X[i] for i in range(V_total)], hist
    Xh = X.to("cpu").numpy()
    return [Xh[i].copy() for i in range(V_total)], hist


def _parse_x_init(x_init, A_list, V_total, N):
    """Validate ``x_init`` (run_admm) without device work: None, ("fbp", filter) or
    ("images", [V_total entries])."""
    if x_init is None:
        return None
    if isinstance(x_init, str):
        kind, _, filt = x_init.partition(":")
        filt = filt or "ram-lak"
        if kind != "fbp" or filt not in FILTERS:
            raise ValueError(f"x_init must be None, 'fbp', 'fbp:<filter>' with a filter of {FILTERS}, "
                             f"or one image per node; got {x_init!r}")
        for g, A in enumerate(A_list):
            if not isinstance(A, RayTransform):
                raise ValueError(f"x_init='fbp': node {g} has an explicit-matrix operator, which has no "
                                 "detector axis to filter along")
        return ("fbp", filt)
    if isinstance(x_init, (torch.Tensor, np.ndarray)):
        if x_init.ndim < 2:
            raise ValueError(f"x_init needs one image per graph node ({V_total}), got shape {tuple(x_init.shape)}")
    imgs = list(x_init)
    if len(imgs) != V_total:
        raise ValueError(f"x_init has {len(imgs)} images, the graph has {V_total} nodes")
    for g, im in enumerate(imgs):
        size = im.numel() if isinstance(im, torch.Tensor) else np.asarray(im).size
        if size != N * N:
            raise ValueError(f"x_init image of node {g} has {size} entries, expected {N} x {N} = {N * N}")
    return ("images", imgs)


def _initial_images(start, A_list, sinograms, local_nodes, dev):
    """{g: float64 (n,) device tensor} for this rank's nodes from a parsed ``x_init``."""
    kind, arg = start
    out = {}
    for g in local_nodes:
        if kind == "fbp":
            A = A_list[g]
            s = sinograms[g]
            s = s if isinstance(s, torch.Tensor) else torch.as_tensor(np.asarray(s))
            im = fbp(A, s.reshape(-1), arg)
        else:
            im = arg[g]
            im = im if isinstance(im, torch.Tensor) else torch.as_tensor(np.asarray(im))
        out[g] = im.reshape(-1).to(device=dev, dtype=torch.float64)
    return out


def _check_metric_args(metrics, data_range, metrics_mask, phantom_true, N):
    """Validate run_admm's metric keywords without device work; the requested names or None."""
    metrics = check_metrics(metrics)
    if metrics is None:
        if data_range is not None or metrics_mask is not None:
            raise ValueError("data_range / metrics_mask need metrics=('psnr', 'ssim') or a subset")
        return None
    if phantom_true is None:
        raise ValueError(f"metrics={metrics!r} needs phantom_true: PSNR and SSIM are taken against it")
    check_side(N)
    check_data_range(data_range)
    if metrics_mask is not None:
        _check_mask_shape(metrics_mask, N)
    return metrics


class _Recorder:
    """One run's histories: made once with what is constant over the run, then called once per iteration
    with the global statistics tables -- by the live loop and by the pipelined flush alike.  The node
    table's blocks are read through the run's layout (table.NodeColumns), which also names the history
    keys of every block.  ``ninc`` / ``tol`` / ``n_pixels``: the stop test's incidences (penalty.incidences),
    (eps_abs, eps_rel) and pixels per image -- a layout with the ``norms`` block needs them."""

    def __init__(self, hist, cols, edges, V_total, lam_tv, have_ph, metrics, ninc=None, tol=None, n_pixels=None):
        self.hist, self.cols, self.edges, self.V_total = hist, cols, edges, V_total
        self.lam_tv, self.have_ph, self.metrics = lam_tv, have_ph, tuple(metrics or ())
        self.ninc, self.tol, self.n_pixels = ninc, tol, n_pixels
        for block in cols.blocks:
            hist.update({k: [] for k in block.keys})

    def __call__(self, k, ns, es, rho, eps_used=None, n_upd=None):
        """Append iteration ``k``'s histories from the global tables ``ns`` (V_total x the layout's width)
        and ``es`` (edges x EDGE_STATS), ``rho`` being the rho the iteration ran with.  ``eps_used`` /
        ``n_upd``: the loop's own two per-node columns; None (the pipelined mode, which applies no
        tolerance) records NaN and 1.  Returns (primal, dual, (bound_primal, bound_dual) or None,
        (eps_pri_k, eps_dual_k) or None)."""
        hist, V_total = self.hist, self.V_total
        v = self.cols.split(ns)
        bres = eps = None
        if "metrics" in v:
            for j, name in enumerate(self.metrics):
                col = v["metrics"][:, j].copy()
                hist[f"{name}_per_node"].append(col)
                hist[f"{name}_mean"].append(float(np.mean(col)))
        if "bounds" in v:  # the projection's three sums
            r2, dw2, viol = (v["bounds"][:, j].copy() for j in range(BOUND_STATS))
            bres = (math.sqrt(float(np.sum(r2))), rho * math.sqrt(float(np.sum(dw2))))  # the form of ``dual``
            hist["bound_primal"].append(bres[0])
            hist["bound_dual"].append(bres[1])
            hist["bound_violation"].append(math.sqrt(float(np.sum(viol))))
            hist["bound_pri_per_node"].append(r2)
            hist["bound_violation_per_node"].append(viol)
        if "norms" in v:  # X2, Z2, U2 -> the stop thresholds
            vals = thresholds(self.tol[0], self.tol[1], self.n_pixels, self.ninc, v["norms"].copy(), rho)
            for key, val in zip(NORM_KEYS, vals):
                hist[key].append(val)
            eps = vals[:2]
        if "robust" in v:  # the weighted Huber value and the outlier count per node
            loss, cnt = v["robust"][:, 0].copy(), v["robust"][:, 1].copy()
            hist["robust_loss_per_node"].append(loss)
            hist["robust_loss_total"].append(float(np.sum(loss)))
            hist["robust_outliers_per_node"].append(cnt)
            hist["robust_outliers_total"].append(float(np.sum(cnt)))
            if v["robust"].shape[1] > 2:  # the scale form: the threshold formed from this iteration's images
                hist["robust_delta_per_node"].append(v["robust"][:, 2].copy())
        if "fuse" in v:  # |x_i - xbar|^2 per node, then -- in the row of global node 0 only -- the scalars
            dev2 = v["fuse"][:, 0].copy()
            hist["consensus_err"].append(math.sqrt(float(np.sum(dev2))))
            hist["consensus_err_per_node"].append(np.sqrt(dev2))
            hist["fused_img_mse"].append(float(v["fuse"][0, 1]) if self.have_ph else float("nan"))
            for j, name in enumerate(self.metrics):
                hist[f"fused_{name}"].append(float(v["fuse"][0, 1 + FUSE_SCALARS + j]))
        # --- node diagnostics (_ver2:145-206) ---
        core = v["core"]
        mse = core[:, MSE_SINO].copy()
        obj = 0.5 * core[:, MSE_SINO] + self.lam_tv * core[:, TV] + core[:, QUAD]
        hist["g_norm_history"].append(np.sqrt(core[:, G2]))
        hist["eps_used_history"].append(np.full(V_total, np.nan) if eps_used is None else eps_used.copy())
        hist["eps_target_history"].append(np.full(V_total, eps_target(k)))
        hist["sb_res_history"].append(np.sqrt(core[:, SBRES2]))
        hist["inner_updates_history"].append((np.ones(V_total) if n_upd is None else n_upd).astype(np.int64))
        hist["mse_sino_per_node"].append(mse)
        hist["mse_sino_total"].append(float(np.sum(mse)))
        img = core[:, IMG].copy() if self.have_ph else np.full(V_total, np.nan)
        hist["img_mse_per_node"].append(img)
        hist["img_mse_total"].append(float(np.sum(img)))
        # --- residuals in G.edges() order (_ver2:232-258) ---
        r2 = 0.0
        s2 = 0.0
        pri = np.zeros(V_total)
        dua = np.zeros(V_total)
        for ge, (a, b) in enumerate(self.edges):
            ra2, rb2, dz2 = float(es[ge, RA2]), float(es[ge, RB2]), float(es[ge, DZ2])
            r2 += ra2 + rb2
            pri[a] += ra2
            pri[b] += rb2
            s2 += rho * rho * dz2
            dua[a] += rho * rho * dz2
            dua[b] += rho * rho * dz2
        pn, dn = math.sqrt(r2), math.sqrt(s2)
        hist["primal"].append(pn)
        hist["dual"].append(dn)
        hist["obj_per_node"].append(obj)
        hist["obj_total"].append(float(np.sum(obj)))
        hist["pri_per_node"].append(np.sqrt(pri))
        hist["dual_per_node"].append(np.sqrt(dua))
        return pn, dn, bres, eps


def _flush_pipelined(record, dev_hist, k0, k1, rho, verbose):
    """Record iterations k0 .. k1-1 of the pipelined statistics (rows 0 .. k1-k0-1 of
    ``dev_hist``) on the host; returns k1."""
    host = dev_hist[: k1 - k0].to("cpu")
    for k in range(k0, k1):
        ns, es = split_stats(host[k - k0], record.V_total, record.cols.width, len(record.edges), EDGE_STATS)
        pn, dn, _, _ = record(k, ns.numpy(), es.numpy(), rho)
        if verbose and k % 10 == 0:
            print(f"iter {k}, primal {pn:.3e}, dual {dn:.3e}")
    return k1


def _solve_to_reference_tolerance(nb, et, max_inner_updates):
    """block_6_admm_loop_ver2.py:105-176 for every local node (after its first x-update):
    solve to eps_try, accept if ||g|| <= eps_target, else tighten eps_try /= 5 (<= 2 times)."""
    V = nb.V
    eps_try = np.full(V, min(EPS_CAP, CALIB_ALPHA * et))
    tries = np.zeros(V, dtype=np.int64)
    n_upd = np.ones(V)
    active = np.ones(V, dtype=bool)
    st = nb.node_stats.to("cpu").numpy()
    while True:
        g, sb = np.sqrt(st[:, 1]), np.sqrt(st[:, 5])
        need = active & (sb > eps_try) & (n_upd < (tries + 1) * max_inner_updates)
        if need.any():  # keep solving the nodes not yet at their eps_try
            nb.node_update_masked(need)
            n_upd += need
            st = nb.node_stats.to("cpu").numpy()
            continue
        done = active & ((g <= et) | (tries >= MAX_TIGHTEN))  # accepted or forced (:155-172)
        active &= ~done
        if not active.any():
            return eps_try, n_upd
        tries[active] += 1
        eps_try[active] /= 5.0  # :174-176


def _chunk_snapshot(out_dir, k, cid, rg, N):
    """block_6_admm_loop.py:55-66: {out_dir}/node_{i}/node_{i}_outer_{k}_chunk_{c}.npy holding
    x.reshape(N, N, order="F") (the skeleton's Fortran-order image), + .png."""
    plt = _pyplot()
    for g, xr in rg.local_images():
        d = os.path.join(out_dir, f"node_{g}")
        os.makedirs(d, exist_ok=True)
        tag = f"node_{g}_outer_{k}"
        img = xr.to("cpu").numpy().reshape(N, N, order="F")
        np.save(os.path.join(d, f"{tag}_chunk_{cid}.npy"), img)
        if plt is not None:
            plt.figure(figsize=(5, 5))
            plt.imshow(img, cmap="gray")
            plt.title(f"{tag} after chunk {cid}")
            plt.axis("off")
            plt.tight_layout()
            plt.savefig(os.path.join(d, f"{tag}_chunk_{cid}.png"), dpi=220)
            plt.close()


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt
    except Exception:  # pragma: no cover
        return None


def _snapshot(snapshot_dir, k, rg, N):
    """_ver2:269-281: iter_XXXX_node_i.npy (C-order reshape) + .png."""
    it_tag = f"iter_{k + 1:04d}"
    plt = _pyplot()
    for g, xr in rg.local_images():
        img = xr.to("cpu").numpy().reshape(N, N)
        np.save(os.path.join(snapshot_dir, f"{it_tag}_node_{g}.npy"), img)
        if plt is not None:
            plt.figure(figsize=(5, 5))
            plt.imshow(img, cmap="gray")
            plt.title(f"{it_tag}  node {g}")
            plt.axis("off")
            plt.tight_layout()
            plt.savefig(os.path.join(snapshot_dir, f"{it_tag}_node_{g}.png"), dpi=220)
            plt.close()


def _write_params(snapshot_dir, rho, lam_tv, V, mu, tv_iters, cg_iters, relaxation=None, balancing=None, fuse=None,
                  robust=None, links=None):
    """_ver2:291-306 admm_internal_params.txt (``links``: the schedule's line, links.describe; a relaxed run adds its alpha; a run with residual
    balancing passes the rho its last iteration ran with and ``balancing`` = (rho_0, the checked
    adapt_rho configuration, the number of changes), which becomes one more line)."""
    try:
        log_dir = snapshot_dir if snapshot_dir is not None else os.getcwd()
        os.makedirs(log_dir, exist_ok=True)
        with open(os.path.join(log_dir, "admm_internal_params.txt"), "w") as f:
            f.write("===== ADMM Internal Parameters =====\n")
            f.write(f"rho = {rho}\n")
            f.write(f"lambda_tv = {lam_tv}\n")
            f.write(f"Number of nodes = {V}\n")
            f.write("Calib alpha = 1.0\n")
            f.write("Eps cap = 0.01\n")
            f.write(f"Split-Bregman mu = {mu}\n")
            f.write(f"Inner iterations (tv x cg) = {tv_iters} x {cg_iters}\n")
            if relaxation is not None:
                f.write(f"Over-relaxation alpha = {relaxation}\n")
            if balancing is not None:
                rho0, cfg, changes = balancing
                f.write(f"Residual balancing: rho_0 = {rho0}, ratio = {cfg['ratio']}, factor = {cfg['factor']}, "
                        f"every = {cfg['every']}, until = {cfg['until']}, rho in [{cfg['rho_min']}, "
                        f"{cfg['rho_max']}], changes = {changes}\n")
            if fuse is not None:
                f.write(f"Fused image = {fuse} mean over the nodes\n")
            if robust is not None and "scale" in robust:
                f.write(f"Huber data term: delta = scale x consistency x quantile of |A x - b| per node, scale = "
                        f"{robust['scale']}, consistency = {robust['consistency']}, quantile = "
                        f"{robust['quantile']}, delta_min = {robust['delta_min']}, reweighted every = "
                        f"{robust['every']}, until = {robust['until']}\n")
            elif robust is not None:
                f.write(f"Huber data term: delta = {robust['delta']}, reweighted every = {robust['every']}, "
                        f"until = {robust['until']}\n")
            if links is not None:
                f.write(links + "\n")
            f.write(f"Date-Time: {datetime.now().strftime('%Y-%m-%d %H:%M:%S')}\n")
    except Exception as e:  # pragma: no cover
        print(f"[WARN] Could not save internal params: {e}")
