"""Drop-in for /root/reference/block_6_admm_loop_ver2.py (the canonical ADMM loop).

Same signature (:15-20) and history keys (:310-326); the node solves and edge
updates run on MI355X (admm_hip.admm.run_admm).  Extra keyword arguments:

* ``mu``        split-Bregman penalty (default 10 * lam_tv)
* ``tv_iters``  split-Bregman rounds per x-update (default 10)
* ``cg_iters``  CG steps per round (default 5)
* ``tv_kind``   "iso" (default) or "aniso"
* ``group``     torch.distributed process group (default: WORLD if initialised)
* ``fusion``    "midpoint" (default; z = (a_i + a_j)/2 as the reference runs, :220-223)
                or "weighted" (z = (W_i a_i + W_j a_j)/(W_i + W_j) with W = Wi_list, the
                form commented out at :221-222 and ADMM_Algo.pdf eq.(2))

* ``inner_tol``  None (default: fixed tv_iters x cg_iters per x-update, deterministic) or
                "reference" (the accept / tighten loop of :100-176: solve to
                eps_try = min(1e-2, eps_target), accept if ||g|| <= eps_target, else
                eps_try /= 5, at most twice; see admm_hip/admm.py)
* ``max_inner_updates``  x-updates per tolerance solve in "reference" mode (default 10)
* ``x_init``    None (default: x = 0, z = 0 as the reference starts, :35-43), "fbp" /
                "fbp:<filter>" (node g starts from the filtered back projection of its own
                sinogram, admm_hip/fbp.py) or one image per graph node ((N, N) or (n,)); the
                run is then a fresh ADMM around those images (y = 0, z = edge means)
* ``metrics``   None (default) or a subset of ("psnr", "ssim"): per-node image quality against
                ``phantom_true`` after every iteration, computed on the GPU (admm_hip/metrics.py);
                adds the history keys psnr_per_node / psnr_mean, ssim_per_node / ssim_mean
* ``data_range``    L of PSNR and SSIM (default phantom_true.max() - phantom_true.min())
* ``metrics_mask``  (N, N) or (n,) mask of the pixels the metrics count (default: all)

* ``ray_weights``   per-ray weights of the data term, 1/2 sum_r w_r (A x - b)_r^2: None, one
                (angles, det) / (m,) array for every node, or one entry (array or None) per node;
                finite and >= 0, 0 masks a ray (geometry operators only)

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
* ``relaxation``  None (default) or alpha in (0, 2): over-relaxation of the edge updates (:210-230
                with x_i replaced by alpha x_i + (1 - alpha) z_old; the projection of ``bounds``
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
                update of :210-230 runs as ever -- or down: it keeps y and z, and both endpoints go on with
                the last values they hold.  Converges to the same fixed point in about 1 / p times the
                iterations; adds the history keys links_up and link_age_max; needs stored z
                (admm_hip/admm.py, admm_hip/links.py)

``max_inner_iters`` is accepted and, as in the reference, unused.
"""
from __future__ import annotations

from admm_hip.admm import run_admm


def decentralized_admm(A_dense_list, sinograms, G, Wi_list, Qij_diag_fn,
                       N, lam_tv=0.01, rho=1.0,
                       max_iters=10, max_inner_iters=100,
                       eps_pri=1e-1, eps_dual=1e-1,
                       verbose=True, snapshot_dir=None,
                       snapshot_every=None, snapshot_div=10, phantom_true=None,
                       mu=None, tv_iters=10, cg_iters=5, tv_kind="iso", group=None,
                       write_params=True, fusion="midpoint", inner_tol=None,
                       max_inner_updates=10, x_init=None, fuse=None, fuse_out=None, robust=None,
                       links=None, metrics=None, data_range=None, metrics_mask=None,
                       adapt_rho=None, eps_abs=None, eps_rel=None, relaxation=None,
                       bounds=None, bound_weight=None,
                       return_feasible=False, ray_weights=None):
    """Returns (x_list, history) like block_6_admm_loop_ver2.py:310-326."""
    del max_inner_iters  # accepted but unused, as in the reference (_ver2:17)
    return run_admm(A_dense_list, sinograms, G, Wi_list, Qij_diag_fn, N, lam_tv=lam_tv, rho=rho,
                    max_iters=max_iters, eps_pri=eps_pri, eps_dual=eps_dual, verbose=verbose,
                    snapshot_dir=snapshot_dir, snapshot_every=snapshot_every,
                    snapshot_div=snapshot_div, phantom_true=phantom_true, mu=mu,
                    tv_iters=tv_iters, cg_iters=cg_iters, tv_kind=tv_kind, group=group,
                    write_params=write_params, fusion=fusion, inner_tol=inner_tol,
                    max_inner_updates=max_inner_updates, x_init=x_init, metrics=metrics,
                    data_range=data_range, metrics_mask=metrics_mask, ray_weights=ray_weights,
                    bounds=bounds, bound_weight=bound_weight, return_feasible=return_feasible,
                    relaxation=relaxation, adapt_rho=adapt_rho, eps_abs=eps_abs, eps_rel=eps_rel,
                    fuse=fuse, fuse_out=fuse_out, robust=robust, links=links)
