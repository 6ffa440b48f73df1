"""Free geometries: detectors with n_det != N or not symmetric about 0, and angle ranges other
than [0, pi] -- the general case of admm_geom (include/admm_tomo.h) that ParallelBeamGeometry
does not expose.

One list, ``GEOMS``, shared by the oracle pins (test_oracle.py), the host planner's cases
(test_fwd_plan_cpu.py) and the GPU tests (test_gpu_free_geom*.py).  N is small on purpose: these
are the smallest shapes at which each path can still go wrong.  A ``FreeGeometry`` passes as a
geometry wherever the product reads only ``n``, ``m``, ``N`` and ``to_c()`` (RayTransform, _Ctx,
NodeBatch); it is hashable, so get_ctx caches its contexts.  Every entry passes check_geom: the
detector spacing is at least the pixel size.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

from oracle.geometry import Geometry

PI = math.pi


@dataclass(frozen=True)
class FreeGeometry:
    id: str
    N: int
    n_angles: int
    n_det: int
    angle_min: float
    angle_max: float
    det_min: float
    det_max: float

    @property
    def n(self) -> int:
        return self.N * self.N

    @property
    def m(self) -> int:
        return self.n_angles * self.n_det

    def to_c(self):
        from admm_hip import _lib
        return _lib.Geom(self.N, self.n_angles, self.n_det, 0, float(self.angle_min), float(self.angle_max),
                         float(self.det_min), float(self.det_max))

    def oracle(self) -> Geometry:
        return Geometry(self.N, self.n_angles, n_det=self.n_det, det_min=self.det_min, det_max=self.det_max,
                        angle_min=self.angle_min, angle_max=self.angle_max)


GEOMS = [
    # n_det > N, mirror-eligible in float32
    FreeGeometry("wide", 48, 24, 70, 0.0, PI, -1.5, 1.5),
    # n_det < N, mirror-eligible, one ragged 64-ray chunk
    FreeGeometry("coarse", 48, 24, 31, 0.0, PI, -1.0, 1.0),
    # asymmetric: not mirror-eligible, part of the image unseen
    FreeGeometry("shifted", 48, 24, 48, 0.0, PI, -0.6, 1.4),
    # detector inside the image: k_f out of range for most pixels
    FreeGeometry("inner", 48, 24, 20, 0.0, PI, 0.1, 0.95),
    # the full circle: negative cos (case A) / sin (case B) as the interpolation axis
    FreeGeometry("circle", 48, 24, 48, 0.0, 2.0 * PI, -1.0, 1.0),
    # limited angle, negative start
    FreeGeometry("limited", 48, 24, 48, -0.3, 0.9, -1.0, 1.0),
    # all of the above at once, odd counts
    FreeGeometry("odd", 48, 25, 61, 0.4, 0.4 + 2.0 * PI, -1.7, 1.2),
    # more than one 64-pixel tile and 64-ray chunk both ways
    FreeGeometry("tiles", 130, 40, 200, -1.0, 5.0, -1.6, 1.5),
    # a single bin
    FreeGeometry("one", 47, 7, 1, 0.0, PI, -0.02, 0.03),
    # no ray meets the image: the clipped forward plans have groups and no blocks
    FreeGeometry("missed", 64, 16, 64, 0.0, PI, 3.0, 5.0),
    # fits = false: no grouped forward plan, the ungrouped k_fwd
    FreeGeometry("nofit", 256, 24, 64, 0.0, PI, -1.0, 1.0),
]
BY_ID = {g.id: g for g in GEOMS}
IDS = [g.id for g in GEOMS]
