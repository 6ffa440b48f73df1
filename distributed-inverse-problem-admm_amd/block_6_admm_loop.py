"""Drop-in for /root/reference/block_6_admm_loop.py (the module block_7_main.py:11 imports).

Accepts that file's keyword surface (:72-84) and runs the full consensus ADMM of
block_6_admm_loop_ver2.py (the skeleton's empty neighbour lists and missing z/y
updates, :119-154, are a reference defect not reproduced).  The returned history has
the ``_ver2`` keys plus this file's ``primal_res`` / ``dual_res`` / ``obj`` (:101-105).

SCS controls map onto the split-Bregman inner solve (CG steps play SCS's iterations,
as block_5_node_problem's ``max_iters`` does):

* ``scs_total_iters`` -> ceil(scs_total_iters / cg_iters) rounds per x-update (unless
  ``tv_iters`` is given explicitly).  The exchange rate is one CG step (one A^T A p) per
  SCS iteration (one KKT matvec in SCS's indirect mode): a modelling choice, not an
  equivalence.  At this file's default (100) that is 20 rounds x 5 CG steps, twice the
  inner work of the ``_ver2`` drop-in's fixed 10 x 5;
* ``scs_chunk_iters`` -> the x-update runs as warm-started chunks of
  ceil(scs_chunk_iters / cg_iters) rounds (:127-146, _scs_solve_in_chunks :14-69);
* ``scs_snapshot_dir`` / ``scs_save_every_chunks`` -> after chunk c (c % every == 0)
  ``{dir}/node_{i}/node_{i}_outer_{k}_chunk_{c}.npy`` with the Fortran-order reshape of
  :58 (+ .png), only for chunked solves, as in the reference (:137-146);
* ``scs_eps`` / ``scs_use_indirect`` / ``scs_alpha`` / ``scs_acceleration`` /
  ``scs_lookback`` / ``scs_scale``: SCS-only, accepted and ignored.

Beyond the reference's surface:

* ``bounds``    None (default) or (lo, hi): the box lo <= x_i <= hi on every node's image; each is
                None, a scalar or an (N, N) / (n,) array shared by all nodes (a support mask is
                hi = 0 outside the support).  Adds the history keys bound_primal, bound_dual,
                bound_violation, bound_pri_per_node, bound_violation_per_node; needs
                fusion="midpoint" and stored z (admm_hip/admm.py, admm_hip/bounds.py)
* ``bound_weight``  kappa > 0 of the constraint's weight q_c,i = kappa * Wi_list[i] (default 1)
* ``return_feasible``  True: return the constraint copies w_i, inside the box exactly, not x_i
* ``adapt_rho``   None (default), True or a dict (ratio, factor, every, until, rho_min, rho_max): residual
                balancing of rho (Boyd et al. 3.4.1: rho * factor where primal > ratio * dual, rho /
                factor where dual > ratio * primal, the scaled duals rescaled); adds the history key
                rho_history (admm_hip/admm.py, admm_hip/penalty.py)
* ``eps_abs``, ``eps_rel``  None (default) or the tolerances of the scale-free stop test (Boyd et al.
                3.12), which then replaces eps_pri / eps_dual; adds the history keys eps_pri_history,
                eps_dual_history, ax_norm, bz_norm, aty_norm; needs stored z
* ``relaxation``  None (default) or alpha in (0, 2): over-relaxation of the edge updates (x_i replaced
                by alpha x_i + (1 - alpha) z_old in the z- and y-updates; the projection of ``bounds``
                too).  1.5 - 1.8 cuts the iterations to a given residual to about 0.6 x; values
                near 2 oscillate with the inexact x-update.  Needs stored z; None and 1.0 change
                nothing (admm_hip/admm.py, admm_hip/relax.py)
* ``fuse``      None (default), "uniform" or "precision": the network's fused image xbar = (sum_i W_i
                x_i) / (sum_i W_i) over all nodes (W = Wi_list, or 1) after every iteration, on the GPU with
                exact fixed-point sums (bitwise the same for any rank count and batch split); adds the
                history keys consensus_err, consensus_err_per_node, fused_img_mse and, with metrics,
                fused_psnr / fused_ssim (admm_hip/admm.py, admm_hip/fuse.py)
* ``fuse_out``  a dict that receives "image" (the fusion of the returned images) and "spread" (their
                per-pixel weighted standard deviation across nodes) as (N, N) arrays
* ``robust``    None (default), a Huber threshold delta > 0 or a dict (delta or scale, every, until; scale:
                delta_i = scale * 1.4826 * median|A x_i - b_i| per node, found on the GPU): the data term
                becomes the Huber loss, minimised by reweighting the rays from each iteration's residual
                (h = min(1, delta / |A x - b|) times ``ray_weights``); adds the history keys
                robust_loss_per_node / robust_loss_total, robust_outliers_per_node /
                robust_outliers_total; geometry operators only (admm_hip/admm.py, admm_hip/robust.py)
* ``links``     None (default), a probability p in (0, 1], a dict (p, seed, max_age, outages) or a bool array
                (iterations, edges): unreliable links.  In every iteration each edge of G is up -- its z / y
                update runs as ever -- or down: it keeps y and z, and both endpoints go on with the last
                values they hold.  Converges to the same fixed point in about 1 / p times the iterations;
                adds the history keys links_up and link_age_max; needs stored z (admm_hip/admm.py,
                admm_hip/links.py)
"""
from __future__ import annotations

import math

from admm_hip.admm import run_admm


def _rounds(iters, cg):
    return max(1, math.ceil(int(iters) / cg))


def decentralized_admm(A_dense_list, sinograms, G, Wi_list, Qij_diag_fn,
                       N, lam_tv=0.01, rho=1.0,
                       max_iters=200,
                       eps_pri=1e-3, eps_dual=1e-3,
                       verbose=True,
                       scs_total_iters=100,
                       scs_chunk_iters=None,
                       scs_snapshot_dir=None,
                       scs_use_indirect=True,
                       scs_eps=3e-3, scs_alpha=1.5,
                       scs_acceleration=1, scs_lookback=10, scs_scale=1e-1,
                       scs_save_every_chunks=1,
                       mu=None, tv_iters=None, cg_iters=5, tv_kind="iso", group=None,
                       phantom_true=None, write_params=True, fuse=None, fuse_out=None, robust=None,
                       links=None, adapt_rho=None, eps_abs=None, eps_rel=None, relaxation=None, bounds=None,
                       bound_weight=None, return_feasible=False, ray_weights=None):
    del scs_use_indirect, scs_eps, scs_alpha, scs_acceleration, scs_lookback, scs_scale
    cg = int(cg_iters)
    total = int(tv_iters) if tv_iters is not None else _rounds(scs_total_iters, cg)
    chunks = None
    if scs_chunk_iters is not None:
        per = _rounds(scs_chunk_iters, cg)
        chunks = [per] * (total // per) + ([total % per] if total % per else [])
    x, hist = run_admm(A_dense_list, sinograms, G, Wi_list, Qij_diag_fn, N, lam_tv=lam_tv,
                       rho=rho, max_iters=max_iters, eps_pri=eps_pri, eps_dual=eps_dual,
                       verbose=verbose, phantom_true=phantom_true, mu=mu, tv_iters=total,
                       cg_iters=cg, tv_kind=tv_kind, group=group, write_params=write_params,
                       inner_chunks=chunks,
                       chunk_snapshot_dir=scs_snapshot_dir if chunks is not None else None,
                       chunk_save_every=scs_save_every_chunks, ray_weights=ray_weights, bounds=bounds,
                       bound_weight=bound_weight, return_feasible=return_feasible, relaxation=relaxation,
                       adapt_rho=adapt_rho, eps_abs=eps_abs, eps_rel=eps_rel, fuse=fuse, fuse_out=fuse_out,
                       robust=robust, links=links)
    hist["primal_res"] = hist["primal"]
    hist["dual_res"] = hist["dual"]
    hist["obj"] = hist["obj_total"]
    return x, hist
