"""The layout of the per-iteration node-statistics table, declared once (host only, no device work).

Every iteration each rank assembles one (V_total, width) float64 table of per-node values, all-reduced
over the ranks in one collective (exchange.assemble_stats_*) and turned into histories on the host
(admm._Recorder).  Its columns are blocks in one fixed order, present only when their feature is on:

    core     the library's NODE_STATS columns (include/admm_tomo.h ADMM_NODE_STAT_*)
    metrics  one column per requested image metric                    (RankGroups.enable_metrics)
    bounds   the projection's BOUND_STATS sums                        (a run with bounds)
    norms    the stop test's NORM_STATS sums X2, Z2, U2               (RankGroups(stop_norms=True))
    robust   the Huber value and the outlier count of the ROBUST_STATS sums   (RankGroups.enable_robust);
             the scale form adds the threshold in force (ROBUST_SCALE_STATS columns)
    fuse     |x_i - xbar|^2, then -- in the row of global node 0 only, zero elsewhere -- the
             FUSE_SCALARS scalars and one column per metric of the fused image (RankGroups.enable_fuse)

``NodeColumns`` is that list: RankGroups builds it and widens it where a feature is enabled; the device
side reads ``sources`` (what a batch concatenates), the host side ``split`` (named views of the table)
and each block's ``keys`` (the history keys its columns feed).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

from ._lib import EDGE_STATS, NODE_STATS

# the core block's columns and the edge table's, named as in include/admm_tomo.h
MSE_SINO, G2, TV, QUAD, IMG, SBRES2 = range(NODE_STATS)
RA2, RB2, DZ2 = range(EDGE_STATS)

ORDER = ("core", "metrics", "bounds", "norms", "robust", "fuse")

HISTORY_KEYS = (
    "primal", "dual", "pri_per_node", "dual_per_node", "obj_per_node", "obj_total",
    "mse_sino_per_node", "mse_sino_total", "img_mse_per_node", "img_mse_total",
    "g_norm_history", "eps_used_history", "eps_target_history",
)
EXTRA_KEYS = ("sb_res_history", "inner_updates_history")


@dataclass(frozen=True)
class Block:
    name: str
    width: int
    source: Callable  # batch -> the (V, k) device tensors that fill the block, left to right
    keys: tuple  # history keys recorded from the block


class NodeColumns:
    def __init__(self):
        self.blocks = [Block("core", NODE_STATS, lambda nb: [nb.node_stats], HISTORY_KEYS + EXTRA_KEYS)]

    def remove(self, name: str) -> None:
        """The feature is off: no block ``name``."""
        self.blocks = [b for b in self.blocks if b.name != name]

    def add(self, name: str, width: int, source: Callable, keys: tuple) -> None:
        """Add the block ``name`` at its place in ``ORDER`` (enabled again: in place of the earlier one)."""
        self.remove(name)
        self.blocks = sorted(self.blocks + [Block(name, int(width), source, tuple(keys))],
                             key=lambda b: ORDER.index(b.name))

    @property
    def width(self) -> int:
        return sum(b.width for b in self.blocks)

    def width_of(self, name: str) -> int:
        """Columns of the block ``name``; 0 when it is off."""
        return sum(b.width for b in self.blocks if b.name == name)

    def sources(self, nb) -> list:
        """The device tensors whose concatenation along dim 1 is the batch's rows of the table."""
        return [t for b in self.blocks for t in b.source(nb)]

    def split(self, table) -> dict:
        """{block name: its columns} as views of the (rows, width) array ``table``: nothing is copied."""
        if table.ndim != 2 or table.shape[1] != self.width:
            raise ValueError(f"node table of shape {tuple(table.shape)}, the layout has {self.width} columns")
        out, c = {}, 0
        for b in self.blocks:
            out[b.name] = table[:, c:c + b.width]
            c += b.width
        return out
