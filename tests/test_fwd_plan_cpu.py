"""CPU: the host planner (csrc/fwd_plan.hpp, csrc/tables.hpp) without a GPU.

tests/host/plan_dump.cpp is built with g++ and with ROCm's clang++, both under the address and
undefined-behaviour sanitizers, and run for every geometry of tests/golden/fwd_plans_parent.json
(recorded from the library before the planner left admm_tomo.hip; mirror-mode rows are the half
geometry's, as admm_batch_bind halves it).  Checked: the plan rows equal the fixture exactly;
the dumped tables are well formed under every plan; fwd_block_order returns permutations that
deal the XCDs round-robin; the plan choice; and both compilers' programs print the same bytes
with nothing on stderr.

The free geometries of tests/free_geom.py (n_det != N, detectors not symmetric about 0, other
angle ranges, one the grouped kernel does not fit) run through the same programs and table
checks without fixture rows, and a plan without blocks is never chosen or accepted as forced.
"""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import free_geom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "plan_dump.cpp")
FLAGS = ["-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
COMPILERS = {"gcc": "g++", "clang": "/opt/rocm/llvm/bin/clang++"}

with open(os.path.join(ROOT, "tests", "golden", "fwd_plans_parent.json")) as _fh:
    FIXTURE = json.load(_fh)


def _cases():
    """(id, N, angles, angle_max, det half width, dtype code, fixture plan rows, dump orders)."""
    out = []
    for b in FIXTURE["batches"]:
        half = b["mirror"]
        out.append((f"N{b['N']}-a{b['angles']}-{b['dtype']}-V{b['V']}" + ("-half" if half else ""), b["N"],
                    b["angles"] // 2 if half else b["angles"], 0.0 + 0.5 * (math.pi - 0.0) if half else math.pi,
                    b["det_width_factor"], int(b["dtype"] == "float64"), b["plans"], True))
    for r in FIXTURE["plan_rows"]:
        half = r["half"]
        out.append((f"N{r['N']}-a{r['angles']}-{r['dtype']}" + ("-half" if half else ""), r["N"],
                    r["angles"] // 2 if half else r["angles"], 0.0 + 0.5 * (math.pi - 0.0) if half else math.pi, 1.0,
                    int(r["dtype"] == "float64"), r["plans"], False))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_dump")
    exes = {}
    for name, cxx in COMPILERS.items():
        exe = d / f"plan_dump_{name}"
        subprocess.run([cxx, *FLAGS, "-o", str(exe), SRC], check=True)
        exes[name] = str(exe)
    return exes


def _dump(programs, N, angles, amax, dwf, dtype, what):
    return _dump_geom(programs, N, angles, N, 0.0, amax, -dwf, dwf, dtype, what)


def _dump_geom(programs, N, angles, n_det, amin, amax, dmin, dmax, dtype, what):
    args = [str(N), str(angles), str(n_det), float(amin).hex(), float(amax).hex(), float(dmin).hex(),
            float(dmax).hex(), str(dtype), what]
    outs = {}
    for name, exe in programs.items():
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        outs[name] = r.stdout
    assert outs["gcc"] == outs["clang"]
    return json.loads(outs["gcc"])


def _check_tables(d, N, n_det, n_angles):
    kG, kSeg = d["kFgG"], d["kFgSeg"]
    fa = d["fa"]
    assert len(fa) == n_angles
    A0, A1, dl = (np.array([a[i] for a in fa]) for i in range(3))
    cover = {}  # plan -> bool [segment][angle][ray]
    for p in d["plans"]:
        pl, groups, ranges, blocks = p["plan"], p["groups"], p["ranges"], p["blocks"]
        # groups: consecutive, single-case, G <= kFgG
        t = 0
        for t0, G, caseA in groups:
            assert t0 == t and 1 <= G <= kG, (pl, t0, G)
            assert {fa[t0 + q][3] for q in range(G)} == {caseA}, (pl, t0, G)
            t += G
        assert t == n_angles
        # blocks: one per range, in range order; {range, group, segment, G}
        assert [b[0] for b in blocks] == list(range(len(ranges)))
        cov = np.zeros((kSeg, n_angles, n_det), dtype=bool)
        last = {}  # (group, segment, angle) -> end of its previous range
        for x, gi, s, w in blocks:
            t0, G, _ = groups[gi]
            assert 0 <= s < kSeg and w == G, (pl, x)
            k0, nk = ranges[x]
            assert len(k0) == kG and len(nk) == kG
            assert all(n == 0 for n in nk[G:]), (pl, x)
            assert any(n > 0 for n in nk[:G]), (pl, x)  # (empty blocks are not emitted)
            for q in range(G):
                assert 0 <= nk[q] <= 64, (pl, x, q)
                if nk[q] == 0:  # no ray (the 64-ray plans leave such a k0 at n_det)
                    continue
                assert 0 <= k0[q] and k0[q] + nk[q] <= n_det, (pl, x, q)  # rays k0 .. k0+nk-1 in [0, n_det)
                assert k0[q] >= last.get((gi, s, q), 0), (pl, x, q)  # disjoint and ascending
                last[(gi, s, q)] = k0[q] + nk[q]
                assert not cov[s, t0 + q, k0[q]:k0[q] + nk[q]].any()
                cov[s, t0 + q, k0[q]:k0[q] + nk[q]] = True
        cover[pl] = cov
        if pl < 3:
            assert cov.all(), pl  # the unclipped plans cover [0, n_det) of every (segment, angle)
    k = np.arange(n_det, dtype=np.float64)
    for pl, cov in cover.items():
        if pl < 3:
            continue
        assert pl - 3 in cover and not (cov & ~cover[pl - 3]).any()
        # a dropped ray misses [-2, N + 1] at every row of the segment: its position
        # l = A0 + k A1 + m dl is linear in the row m, and |dl| <= 1 cannot step over the image
        for s in range(kSeg):
            mlo, mhi = s * N // kSeg, (s + 1) * N // kSeg
            la = A0[:, None] + k[None, :] * A1[:, None] + mlo * dl[:, None]
            lb = A0[:, None] + k[None, :] * A1[:, None] + (mhi - 1) * dl[:, None]
            out = (np.maximum(la, lb) < -2.0) | (np.minimum(la, lb) > N + 1.0)
            assert np.abs(dl).max() <= 1.0
            assert out[~cov[s]].all(), (pl, s)


def _check_orders(d):
    kSeg, kX = d["kFgSeg"], d["kXcds"]
    for p in d["plans"]:
        caseA = [g[2] for g in p["groups"]]
        seen = set()
        for o in p["orders"]:
            nch, cus, paired, table = o["nch"], o["cus"], o["paired"], o["table"]
            seen.add((nch, cus, paired))
            want = sorted([x, y, z + kSeg * c, 0] for c in range(nch) for x, y, z, _ in p["blocks"])
            assert sorted(table) == want, (p["plan"], nch, cus, paired)
            if cus == 0:
                assert table == [[x, y, z + kSeg * c, 0] for c in range(nch) for x, y, z, _ in p["blocks"]]
            if cus != 256:
                continue

            def xcd(b):
                sg = b[2] % kSeg
                return (2 * min(sg, kSeg - 1 - sg) + caseA[b[1]]) % kX if paired else sg % kX
            left = [0] * kX
            for b in table:
                left[xcd(b)] += 1
            for pos, b in enumerate(table):
                if left[pos % kX] > 0:  # this XCD's list lasts: launch position pos runs one of its blocks
                    assert xcd(b) == pos % kX, (p["plan"], nch, paired, pos)
                left[xcd(b)] -= 1
        assert seen == {(n, c, q) for n in (1, 2, 3) for c in (0, 256, 250) for q in (0, 1)}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_planner_matches_fixture_and_is_well_formed(programs, case):
    _, N, angles, amax, dwf, dtype, rows, orders = case
    d = _dump(programs, N, angles, amax, dwf, dtype, "orders" if orders else "tables")
    assert d["error"] is None
    got = [dict(plan=p["plan"], groups=len(p["groups"]), blocks=len(p["blocks"]), staged_px=p["staged_px"])
           for p in d["plans"]]
    want = [dict(plan=r["plan"], groups=r["groups"], blocks=r["blocks"], staged_px=float(r["staged_px"]))
            for r in rows]
    assert got == want  # (staged_px: doubles compared with ==)
    assert d["fits"] == bool(rows)
    _check_tables(d, N, N, angles)
    if orders:
        _check_orders(d)
    have = {p["plan"] for p in d["plans"]}
    ch = d["choice"]
    if have:
        assert ch["one_round"] == 0  # every plan in one round: the 64-ray plan
        assert all(c in have for c in ch["slots512"])
        free = ch["forced"][0]
        for f in range(6):
            assert ch["forced"][1 + f] == (f if f in have else free), f  # a forced plan the geometry has
        assert ch["forced"][7] == free


def test_planner_reports_the_geometry_errors(programs):
    """The two messages of admm_ctx_create that come from the tables: a detector finer than the
    pixels, and (float32 samples) a detector so far off the image that kf_split's range breaks."""
    d = _dump(programs, 64, 12, math.pi, 0.5, 0, "tables")
    assert "detector spacing finer than the pixel size" in d["error"]
    args = ["64", "12", "64", (0.0).hex(), math.pi.hex(), (-4.0e4).hex(), (-4.0e4 + 2.0).hex(), "0", "tables"]
    for exe in programs.values():
        r = subprocess.run([exe, *args], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == ""
        assert "kf_split" in json.loads(r.stdout)["error"]


# ----------------------------------------------------------------------------
# free geometries (tests/free_geom.py): n_det != N, detectors not symmetric about 0, angle
# ranges other than [0, pi].  No fixture rows: well-formed tables, identical bytes from both
# compilers and an empty stderr (sanitizers) are the assertions.
# ----------------------------------------------------------------------------
def _blocks(d):
    return {p["plan"]: len(p["blocks"]) for p in d["plans"]}


def _check_choice_has_blocks(d):
    """Every plan choice -- free, by rounds, forced -- names a plan with blocks; a forced plan
    the geometry does not have, or has without blocks, falls back to the free choice."""
    nb = _blocks(d)
    ch = d["choice"]
    assert nb.get(ch["one_round"], 0) > 0
    assert all(nb.get(c, 0) > 0 for c in ch["slots512"])
    free = ch["forced"][0]
    assert nb.get(free, 0) > 0 and ch["forced"][7] == free
    for f in range(6):
        assert ch["forced"][1 + f] == (f if nb.get(f, 0) > 0 else free), f


@pytest.mark.parametrize("dtype", [0, 1], ids=["float32", "float64"])
@pytest.mark.parametrize("g", free_geom.GEOMS, ids=free_geom.IDS)
def test_planner_on_free_geometries_is_well_formed(programs, g, dtype):
    d = _dump_geom(programs, g.N, g.n_angles, g.n_det, g.angle_min, g.angle_max, g.det_min, g.det_max, dtype,
                   "orders" if g.id in ("wide", "odd") else "tables")
    assert d["error"] is None
    _check_tables(d, g.N, g.n_det, g.n_angles)
    if g.id == "nofit":  # no grouped kernel: the ungrouped k_fwd projects this geometry
        assert d["fits"] is False and d["plans"] == []
        return
    assert d["fits"] is True
    assert {0, 1} <= set(_blocks(d))  # the mandatory plans
    if "orders" in d["plans"][0]:
        _check_orders(d)
    _check_choice_has_blocks(d)
    A1 = np.array([a[1] for a in d["fa"]])
    if g.id in ("circle", "odd", "tiles"):  # past pi/2 .. 3pi/2: descending rays
        assert (A1 < 0).any() and (A1 > 0).any()
    if g.id in ("wide", "coarse"):  # mirror-eligible: the half geometry admm_batch_bind plans
        h = _dump_geom(programs, g.N, g.n_angles // 2, g.n_det, g.angle_min,
                       g.angle_min + 0.5 * (g.angle_max - g.angle_min), g.det_min, g.det_max, dtype, "tables")
        assert h["error"] is None and h["fits"] is True
        _check_tables(h, g.N, g.n_det, g.n_angles // 2)
        _check_choice_has_blocks(h)
        assert h["fa"] == d["fa"][: g.n_angles // 2]  # bitwise the full geometry's first half


def test_a_plan_without_blocks_is_never_chosen(programs):
    """A detector that misses the image: the clipped plans 3-5 keep their groups and have no
    block.  They count as plans the geometry does not have (a launch of 0 blocks is an error):
    never the free choice, and forced they fall back like a missing plan."""
    g = free_geom.BY_ID["missed"]
    for dtype in (0, 1):
        d = _dump_geom(programs, g.N, g.n_angles, g.n_det, g.angle_min, g.angle_max, g.det_min, g.det_max, dtype,
                       "tables")
        nb = _blocks(d)
        assert all(len(p["groups"]) > 0 for p in d["plans"])
        assert [nb[p] for p in (3, 4, 5)] == [0, 0, 0] and all(nb[p] > 0 for p in (0, 1, 2))
        _check_choice_has_blocks(d)
        ch = d["choice"]
        assert ch["forced"][4:7] == [ch["forced"][0]] * 3


def test_a_detector_that_misses_some_segments(programs):
    """Detector [1.1, 3.1] at N = 64: its rays meet the image only near the corners, so a clipped
    plan has fewer blocks than segments x groups and still some; every choice has blocks."""
    d = _dump_geom(programs, 64, 16, 64, 0.0, math.pi, 1.1, 3.1, 0, "tables")
    assert d["error"] is None and d["fits"] is True
    _check_tables(d, 64, 64, 16)
    p3 = next(p for p in d["plans"] if p["plan"] == 3)
    assert 0 < len(p3["blocks"]) < d["kFgSeg"] * len(p3["groups"])
    _check_choice_has_blocks(d)
