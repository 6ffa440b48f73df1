"""Over-relaxation of the edge and constraint updates (scope row f9).

Host side of ``admm_consensus_relaxed`` (csrc/relax.hip; the relaxed projection of a bounded run is
``admm_bound_project_relaxed``, csrc/bounds.hip, reached through bounds.BoundProjector): the
argument checks, which need no device (``check_relaxation``, ``check_relaxed_run``), and ``Relaxer``,
which owns the edge kernel's scratch and enqueues the relaxed updates of a NodeBatch

    xh_i = alpha x_i + (1 - alpha) z_old   in place of x_i in the z- and y-updates, 0 < alpha < 2

(Eckstein-Bertsekas; Boyd et al. 3.4.3).  The residual statistics keep the true x_i, so ``primal``,
``dual`` and the stop test keep their definitions.  alpha in 1.5 - 1.8 is the useful range: on this
solver's inexact fixed-count x-update 1.6 needs about 0.63 x and 1.8 about 0.56 x the iterations of
alpha = 1, and values near 2 oscillate.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib
from .plan import derived_z_requested


def check_relaxation(relaxation) -> float | None:
    """``relaxation`` = None or a real number in the open interval (0, 2), as the alpha of a relaxed
    run or None for the plain one (None and 1.0: today's path exactly).  Raises ValueError for a
    bool, anything that is not a real number, NaN and values <= 0 or >= 2.  Host work only."""
    if relaxation is None:
        return None
    if isinstance(relaxation, bool) or not isinstance(relaxation, numbers.Real):
        raise ValueError(f"relaxation must be None or a real number in (0, 2), got {relaxation!r}")
    a = float(relaxation)
    if math.isnan(a) or not (0.0 < a < 2.0):
        raise ValueError(f"relaxation must lie in the open interval (0, 2), got {relaxation!r}")
    return None if a == 1.0 else a


def check_relaxed_run(alpha, edge_state, env_edge_state: str = ""):
    """The combination a relaxed run does not support, as ValueError (host work only): derived z is
    the midpoint of the endpoint images of the last consensus, which a relaxed z' is not."""
    if alpha is None:
        return
    if derived_z_requested(edge_state, env_edge_state):
        raise ValueError("relaxation needs stored z (edge_state='stored'): a relaxed z is not the midpoint of "
                         "the endpoint images, so it cannot be derived from them")


class Relaxer:
    """The relaxed updates of one NodeBatch with ``n_edges`` real edge slots of ``n`` pixels on
    ``device``: alpha and the edge kernel's scratch."""

    def __init__(self, alpha: float, n: int, n_edges: int, device):
        self.lib = _lib.load()
        self.alpha = float(alpha)
        self.n = int(n)
        self.n_edges = int(n_edges)
        self.work = _lib.work_buffer("admm_consensus_relaxed_work", self.n, self.n_edges, device=device)

    def run_edges(self, nb, e0: int, e1: int, stream: int) -> None:
        """y, z (weighted fusion: y_b too) and ``edge_stats`` of ``nb``'s edge slots [e0, e1) <- the
        relaxed update around its x_ext, in place, on ``stream``."""
        if not (0 <= e0 <= e1 <= self.n_edges):
            raise ValueError(f"edge slots [{e0}, {e1}) outside the batch's [0, {self.n_edges})")
        p = _lib.ptr
        _lib.check(self.lib.admm_consensus_relaxed(p(nb.x_ext), self.n, nb.x_ext.shape[0], p(nb.y), p(nb.y_b),
                                                   p(nb.z), p(nb.w), p(nb.edge_a), p(nb.edge_b), int(e0), int(e1),
                                                   self.alpha, p(self.work), p(nb.edge_stats), C.c_void_p(stream)),
                   "admm_consensus_relaxed")

    def run_bounds(self, projector, x, w, f, stream: int) -> torch.Tensor:
        """``projector.run`` (bounds.BoundProjector: its checks, scratch, maps and sums) around the
        relaxed images alpha x + (1 - alpha) w."""
        return projector.run(x, w, f, stream, alpha=self.alpha)
