"""Exact clearance of the ego rectangle to the occupied cells of the map (cilqr_map_clearance*, include/cilqr.h): the map counterpart of
CILQR_FP_CLEARANCE.

Expected values never come from the HIP path: `clearance_restate` is a numpy restatement of the header's definition over ALL in-map
seeds (no window), checked here against densely sampled rectangle boundaries.  Tolerances are those tests/test_footprint.py applies to
CILQR_FP_CLEARANCE: 1e-9 absolute on clearances (ABS_TOL), infinite values and every count and index exact.  An index is decided only
where the two smallest values differ by more than that tolerance; `test_conditions` asserts on the restatement alone that every scene is
decided everywhere — no two seeds within ABS_TOL at a step's minimum, no seed within ABS_TOL of `reach`, no step within ABS_TOL of
min_clearance or of 0 — so the GPU tests compare every index and count exactly.

Scenes (map GEOM_A, 160 x 80 cells of 0.1 m; a wall of seeds across the path at x = 5 m, 2 % random seeds behind it up to x = 10 m, 3 % NaN
cells from x = 4.4 m on; rows drive along x from in front of the wall to beyond the map's far edge at 14 m):
  S3    N 8,  B 1, S 3: one shared map, three rows of one solve
  R5    N 8,  B 5, S 1: a layer and a pose per solve
  T40   N 40, B 6, S 1: one shared map
  P40   N 40, B 3, S 2: a layer and a pose per solve, two rows each
Every scene holds steps of each kind: positive finite clearance, <= 0, +HUGE_VAL (no seed within reach), a window that leaves the map,
and lost (a state that is not finite).
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import ABS_TOL, _bits
from test_footprint import LENGTH, WIDTH, boundary
from test_map_distance import rect_clearance, seeds_of
from test_risk_map import GEOM_A, POSE_A, _c_poses, _Map, _params

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_map_clearance", "cilqr_map_clearance_device")
FIELDS = ("CLEARANCE", "STEP", "CELL", "BELOW_STEPS", "FIRST_BELOW", "TOUCH_STEPS", "OFF_MAP_STEPS", "LOST_STEPS")
CLEARANCE, STEP, CELL, BELOW_STEPS, FIRST_BELOW, TOUCH_STEPS, OFF_MAP_STEPS, LOST_STEPS = range(8)
THRESHOLD, REACH, MIN_CLEARANCE, MARGIN = 50.0, 1.0, 0.25, 0.1
_dp = C.POINTER(C.c_double)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _row_restate(g, pose, layer, X, N, hl, hw, threshold, reach, unknown_seeds):
    """One row.  Returns per step: clearance, cell, gap (second smallest - smallest among the seeds within reach; inf), edge (distance of
    the seed nearest to `reach` from it), off (the window leaves the map), lost."""
    rows, cols, res = int(g.rows), int(g.cols), float(g.res)
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    inv_res = 1.0 / res
    cp, sp = math.cos(pose[2]), math.sin(pose[2])
    si, sj = np.nonzero(seeds_of(layer, threshold, 1 if unknown_seeds else 0))
    cell = si + sj * rows
    order = np.argsort(cell)
    si, sj, cell = si[order], sj[order], cell[order]
    mx, my = x_first - si * res, y_first - sj * res
    clr, at, gap, edge = np.full(N, np.inf), np.full(N, -1.0), np.full(N, np.inf), np.full(N, np.inf)
    off, lost = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    for t in range(N):
        x, y, th = X[t, 0], X[t, 1], X[t, 3]
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(th)):
            clr[t], lost[t] = -np.inf, True
            continue
        ct, st = math.cos(th), math.sin(th)
        dx, dy = x - pose[0], y - pose[1]
        cx, cy = cp * dx + sp * dy, cp * dy - sp * dx
        cm, sm = ct * cp + st * sp, st * cp - ct * sp
        # the window: the corners of the rectangle grown by reach, in the map frame, one cell wider on every side
        qx, qy = [], []
        for a, b in ((hl + reach, hw + reach), (hl + reach, -hw - reach), (-hl - reach, -hw - reach), (-hl - reach, hw + reach)):
            Px, Py = x + (a * ct - b * st), y + (a * st + b * ct)
            ex, ey = Px - pose[0], Py - pose[1]
            qx.append(cp * ex + sp * ey)
            qy.append(cp * ey - sp * ex)
        i_lo, i_hi = math.floor((x_first - max(qx)) * inv_res) - 1, math.ceil((x_first - min(qx)) * inv_res) + 1
        j_lo, j_hi = math.floor((y_first - max(qy)) * inv_res) - 1, math.ceil((y_first - min(qy)) * inv_res) + 1
        off[t] = i_lo < 0 or j_lo < 0 or i_hi > rows - 1 or j_hi > cols - 1
        da, db = mx - cx, my - cy
        a, b = da * cm + db * sm, db * cm - da * sm
        ua, ub = np.abs(a) - hl, np.abs(b) - hw
        s = np.where((ua > 0.0) | (ub > 0.0), np.hypot(np.maximum(ua, 0.0), np.maximum(ub, 0.0)), np.maximum(ua, ub))
        if s.size:
            edge[t] = float(np.abs(s - reach).min())
        near = s <= reach
        if near.any():
            v, c = s[near], cell[near]
            k = int(np.argmin(v))  # the first of equal values: the lowest cell
            clr[t], at[t] = v[k], c[k]
            if v.size > 1:
                gap[t] = float(np.partition(v, 1)[1] - v[k])
    return clr, at, gap, edge, off, lost


def clearance_restate(p, g, layers, poses, X, N, S, margin, threshold, reach, min_clearance, unknown_seeds, base=None):
    """X (R, 4(N+1)); layers / poses one shared or lists per solve.  Returns dict(mc (R, 8), step_clearance (R, N), total, and the
    decidedness measures gap / edge / step_gap per row)."""
    R = X.shape[0]
    hl, hw = 0.5 * p.length + margin, 0.5 * p.width + margin
    per_solve = isinstance(layers, list)
    mc, sc = np.zeros((R, 8)), np.zeros((R, N))
    gaps, edges, step_gap, cells = np.zeros((R, N)), np.zeros((R, N)), np.full(R, np.inf), np.zeros((R, N))
    for r in range(R):
        b = r // S
        clr, at, gap, edge, off, lost = _row_restate(g, poses[b] if per_solve else poses, layers[b] if per_solve else layers,
                                                     X[r].reshape(N + 1, 4), N, hl, hw, threshold, reach, unknown_seeds)
        sc[r], gaps[r], edges[r], cells[r] = clr, gap, edge, at
        has = clr < np.inf
        f = mc[r]
        f[CLEARANCE], f[STEP], f[CELL] = np.inf, -1.0, -1.0
        if has.any():
            k = int(np.argmin(np.where(has, clr, np.inf)))  # the lowest t on equal values
            f[CLEARANCE], f[STEP], f[CELL] = clr[k], k, at[k]
            rest = np.delete(np.where(has, clr, np.inf), k)
            if rest.size and np.isfinite(clr[k]):
                step_gap[r] = float(rest.min() - clr[k])
        below = clr < min_clearance
        f[BELOW_STEPS], f[FIRST_BELOW] = below.sum(), (int(np.argmax(below)) if below.any() else -1)
        f[TOUCH_STEPS], f[OFF_MAP_STEPS], f[LOST_STEPS] = (clr <= 0.0).sum(), off.sum(), lost.sum()
    total = None
    if base is not None:
        ok = np.isfinite(base) & (mc[:, LOST_STEPS] == 0) & (mc[:, CLEARANCE] >= min_clearance)
        total = np.where(ok, base, np.nan)
    return dict(mc=mc, step_clearance=sc, total=total, gap=gaps, edge=edges, step_gap=step_gap, cells=cells)


# ---- scenes --------------------------------------------------------------------------------------------------------------------
def seed_layer(g, pose, seed):
    """(rows, cols) float32: a wall of seeds (100) across the path at world x in [5, 5.1), 2 % random seeds up to x = 10, 40 (below the
    threshold) on a tenth of the cells, 3 % NaN cells from x = 4.4 on."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, cols = int(g.rows), int(g.cols)
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    mx = (x_first - np.arange(rows) * g.res)[:, None]
    my = (y_first - np.arange(cols) * g.res)[None, :]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    wx, wy = pose[0] + c * mx - s * my, pose[1] + s * mx + c * my
    layer = np.where(rng.random((rows, cols)) < 0.1, 40.0, 0.0).astype(np.float32)
    layer[(wx >= 5.0) & (wx < 5.1) & (np.abs(wy) < 3.0)] = 100.0
    layer[(wx >= 5.1) & (wx < 10.0) & (rng.random((rows, cols)) < 0.02)] = 100.0
    layer[(wx >= 4.4) & (rng.random((rows, cols)) < 0.03)] = np.nan
    return layer


def _rows(N, R, reach_x):
    """R rows along x: row r starts at x = 0.2 + 0.15 r, so that the first steps lie farther than `reach` in front of the wall, a later one
    within it, the middle ones over seeds and the last ones beyond x = reach_x; a gentle turn; one lost step per scene."""
    X = np.zeros((R, N + 1, 4))
    for r in range(R):
        x0, y0 = 0.2 + 0.15 * r, -1.0 + 0.45 * r
        step = (reach_x - x0) / (N - 1)
        # the first quarter of the steps approaches the wall slowly, the rest covers the map
        t = np.arange(N + 1)
        slow = max(2, N // 4)
        x = np.where(t < slow, x0 + 1.6 * t / slow, x0 + 1.6 + (t - slow) * (reach_x - x0 - 1.6) / max(1, N - 1 - slow))
        if r % 3 == 1:  # this row stops in front of the wall: a row that is clear, or clear but for min_clearance
            x = x0 + 1.6 * np.minimum(t, slow) / slow
        X[r, :, 0], X[r, :, 1], X[r, :, 2] = x, y0 + 0.02 * t * step, 4.0
        X[r, :, 3] = 0.002 + 0.031 * (r - 1) + 0.0037 * t  # (never a map's own heading: aligned, a line of wall cells ties)
    X[R - 1, N // 2, 1] = np.nan   # a lost step
    X[0, N, 0] = np.inf            # x_N is not visited
    return X.reshape(R, -1)


def _scene(O, name, N, B, S, per_solve):
    p = O.default_params(N)
    g = O.map_geom(*GEOM_A)
    if per_solve:
        poses = _c_poses(B)
        layers = [seed_layer(g, poses[b], 10 + b) for b in range(B)]
    else:
        poses, layers = POSE_A, seed_layer(g, POSE_A, 3)
    X = _rows(N, B * S, 15.5)
    s = dict(name=name, p=p, N=N, B=B, S=S, R=B * S, X=X, geom=GEOM_A, g=g, layers=layers, poses=poses, probes=(3, 3),
             base=10.0 + np.arange(B * S)[::-1].astype(np.float64))
    for unknown in (False, True):
        s[unknown] = clearance_restate(p, g, layers, poses, X, N, S, MARGIN, THRESHOLD, REACH, MIN_CLEARANCE, unknown, s["base"])
    return s


SCENES = ["S3", "R5", "T40", "P40"]


@pytest.fixture(scope="module")
def scenes(oracle):
    """Every scene's inputs and restatement (both flags).  Computed once; never modified."""
    O = oracle
    return {"S3": _scene(O, "S3", 8, 1, 3, False), "R5": _scene(O, "R5", 8, 5, 1, True), "T40": _scene(O, "T40", 40, 6, 1, False),
            "P40": _scene(O, "P40", 40, 3, 2, True)}


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_call(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_MAP_CLEARANCE_FIELDS\s+8\b", h) and re.search(r"#define\s+CILQR_MAP_CLEARANCE_UNKNOWN_SEEDS\s+1u", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_MC_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "MC_" + name) == i
    assert cilqr.MAP_CLEARANCE_FIELDS == 8 and cilqr.MAP_CLEARANCE_UNKNOWN_SEEDS == 1
    assert callable(cilqr.Solver.map_clearance) and callable(cilqr.Solver.map_clearance_device)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_map_clearance\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_map_clearance.hip" in mk and len(re.findall(r"build/cilqr_map_clearance\.o", mk)) == 2  # `check` and its resource list
    text = re.sub(r"\s*\n \*\s*", " ", full)
    for phrase in ("minus the penetration depth", "Seeds with s > reach never count", "it may differ from Polygon::isInside",
                   "on DIFFERENT streams of one handle must not overlap"):
        assert phrase in text, phrase


def test_the_facade_exports_the_setter():
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_map_clearance_check\s*\(\s*double\s+min_clearance\s*,\s*double\s+reach\s*,\s*double\s+occ_threshold\s*,\s*double\s+margin\s*=\s*0\.0\s*,"
                     r"\s*bool\s+unknown_seeds\s*=\s*false\s*,\s*bool\s+on\s*=\s*true\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_map_clearance\s*,\s*last_map_step_clearance\s*;", f)
    lay = open(os.path.join(PKG, "host", "candidate_layout.h")).read()
    assert re.search(r"bool\s+map_clearance\s*=\s*false\s*;", lay) and re.search(r"bool\s+map_clearance_check\s*\(\s*\)\s*const", lay)


def _build(tmp_path, source, *includes, lib=False):
    exe = str(tmp_path / source.replace(".cpp", ""))
    link = ["-L" + os.path.join(PKG, "lib"), "-lcilqr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib")] if lib else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall"] + ["-I" + d for d in includes] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", source)] + link, check=True)
    return exe


def test_the_layout_with_the_map_clearance_flag(tmp_path):
    """tests/cpp/candidate_layout_map_clearance_dump.cpp beside the two existing dumps: with the flag off every record — predicates,
    every offset and `end` — is what the footprint dump gives (and so, with that flag off too, what the first dump gives); with it on
    the stage's three arrays are reserved in front of the footprint check's, nothing before them moves, and the stage runs only while a
    map is set."""
    inc = os.path.join(PKG, "host"), os.path.join(ROOT, "include")
    first, old, new = (_build(tmp_path, n, *inc) for n in ("candidate_layout_dump.cpp", "candidate_layout_footprint_dump.cpp", "candidate_layout_map_clearance_dump.cpp"))

    def names(exe):
        d = dict(line.split(":") for line in subprocess.run([exe, "names"], check=True, capture_output=True, text=True).stdout.splitlines())
        return d["flags"].split(), d["predicates"].split(), d["arrays"].split()
    (f0, p0, a0), (f1, p1, a1) = names(old), names(new)
    assert f1 == f0 + ["map_clearance"] and p1 == p0 + ["map_clearance_check"]  # one flag, one predicate
    assert a1 == a0 and a1[-7:] == ["mcrow", "mcstep", "mctotal", "fprow", "fpstep", "fptotal", "end"]
    rng = np.random.default_rng(6)
    n = 600
    rec = np.zeros((n, 8), dtype=np.uint64)
    rec[:, 0] = rng.integers(0, 2 ** len(f0), n)
    rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = rng.integers(1, 7, n), rng.integers(1, 51, n), rng.integers(0, 5, n), rng.integers(0, 300, n)
    rec[:, 5], rec[:, 6], rec[:, 7] = rng.integers(0, 3, n), rng.integers(0, 3, n), rng.integers(0, 28, n)

    def run(exe, records):
        out = subprocess.run([exe], input=records.tobytes(), capture_output=True, check=True).stdout
        return np.frombuffer(out, dtype=np.uint64).reshape(len(records), -1)
    off_old, off_new = run(old, rec), run(new, rec)
    assert np.array_equal(off_old, off_new)  # flag off: every predicate, every offset and `end`
    no_fp = rec.copy()
    no_fp[:, 0] &= np.uint64(2 ** (len(f0) - 1) - 1)
    assert np.array_equal(run(first, no_fp)[:, 1:], run(new, no_fp)[:, 1:])
    k = {name: 1 + i for i, name in enumerate(a1)}
    on = rec.copy()
    on[:, 0] |= np.uint64(1 << len(f0))
    got = run(new, on).astype(np.int64)
    B, N = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    even = lambda v: (v + 1) // 2 * 2  # noqa: E731
    for name in a0[:-7] + ["mcrow"]:
        assert np.array_equal(got[:, k[name]], off_old[:, k[name]].astype(np.int64)), name  # flag on: nothing before the new arrays moves
    assert np.array_equal(got[:, k["mcstep"]] - got[:, k["mcrow"]], even(B * 8))
    assert np.array_equal(got[:, k["mctotal"]] - got[:, k["mcstep"]], even(B * N))
    assert np.array_equal(got[:, k["fprow"]] - got[:, k["mctotal"]], even(B))
    grown = even(B * 8) + even(B * N) + even(B)
    for name in ("fprow", "fpstep", "fptotal", "end"):
        assert np.array_equal(got[:, k[name]], off_old[:, k[name]].astype(np.int64) + grown), name
    bit = {name: i for i, name in enumerate(p1)}
    fbit = {name: i for i, name in enumerate(f1)}
    map_set = (on[:, 0] >> np.uint64(fbit["map_set"])) & np.uint64(1)
    runs = (got[:, 0] >> bit["map_clearance_check"]) & 1
    assert np.array_equal(runs, map_set.astype(np.int64)) and 0 < runs.sum() < n
    assert np.all(((got[:, 0] >> bit["in_block"]) & 1)[runs == 1])


# the six-candidate scene of tests/cpp/candidates_map_clearance.cpp: the blob scene of tests/test_tighten_map.py, seeds above 80
SIX_THRESHOLD, SIX_REACH, SIX_BETWEEN, SIX_PICK_CHEAPEST, SIX_PICK_CLEAR = 80.0, 1.0, 0.25, 3, 4


@pytest.fixture(scope="module")
def six(oracle):
    from test_tighten_map import _round_scene
    O = oracle
    s = _round_scene(O)
    um, keep = O.uncertainty_map(s["layers"], s["g"], s["poses"], s["probes"])
    r = O.solve_batch_unc(s["p"], s["N"], 0, s["x0"], s["U0"].copy(), s["poly"], s["fl"], None, None, None, um, threads=min(8, O.max_threads()))
    want = clearance_restate(s["p"], s["g"], s["layers"], s["poses"], r["X"], s["N"], 1, 0.0, SIX_THRESHOLD, SIX_REACH, SIX_BETWEEN, False, r["J"])
    return dict(s=s, solve=r, want=want)


def test_the_six_candidate_table(six):
    """The constants of tests/cpp/candidates_map_clearance.cpp, from the oracle's solves and the restatement alone: the cheapest candidate
    by J is 3 and passes 0.18 m from the seeds; min_clearance 0.25 lies between the clearances of candidates 3 and 4, decided by more
    than 5 cm either way, and the cheapest candidate at least that clear is 4; at 0 candidates 0 and 1 are rejected; nobody is 0.5 m clear."""
    J, c = six["solve"]["J"], six["want"]["mc"][:, CLEARANCE]
    print("J %s; clearance %s" % (np.round(J, 4).tolist(), np.round(c, 4).tolist()))
    assert int(np.argmin(J)) == SIX_PICK_CHEAPEST and 0.0 < c[SIX_PICK_CHEAPEST] < SIX_BETWEEN - 0.05
    clear = c >= SIX_BETWEEN
    assert clear.tolist() == [False, False, False, False, True, True] and c[4] > SIX_BETWEEN + 0.03
    assert int(np.argmin(np.where(clear, J, np.inf))) == SIX_PICK_CLEAR
    assert (c >= 0.0).tolist() == [False, False, True, True, True, True] and np.abs(c).min() > 0.02 and c.max() < 0.45
    assert np.diff(np.sort(J)).min() > 1e-3
    # the whole-field restatement of tests/test_map_distance.py agrees where every seed is within reach
    assert np.allclose(c, rect_clearance(six["s"]["p"], six["s"]["g"], six["s"]["poses"], six["s"]["layers"], six["solve"]["X"], six["s"]["N"], SIX_THRESHOLD), atol=1e-12)


def test_argument_errors_need_no_device(cilqr):
    """Decided before the handle is looked at (there is none here); valid arguments reach the handle check."""
    L = cilqr.lib()
    R, N = 2, 4
    X, base, mc, total = np.zeros((R, 4 * (N + 1))), np.zeros(R), np.zeros((R, 8)), np.zeros(R)
    no_handle = C.c_void_p()
    d = C.c_double
    nan, inf = float("nan"), float("inf")

    def call(dev, S=1, margin=0.0, thr=THRESHOLD, reach=REACH, min_clearance=0.0, flags=0, **nulls):
        a = dict(X=X, base=base, mc=mc, total=total)
        a.update(nulls)
        f = L.cilqr_map_clearance_device if dev else L.cilqr_map_clearance
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, R, N, S, _p(a["X"]), d(margin), d(thr), d(reach), d(min_clearance), C.c_uint32(flags), _p(a["base"]), _p(a["mc"]), None,
                 _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "mc"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert call(dev, S=0) == ERR_ARG and b"S = 0" in L.cilqr_last_error()
        for bad in (-1e-3, nan, inf, -inf):
            assert call(dev, margin=bad) == ERR_ARG and b"margin is negative or not finite" in L.cilqr_last_error(), bad
            assert call(dev, reach=bad) == ERR_ARG and b"reach is negative or not finite" in L.cilqr_last_error(), bad
        assert call(dev, thr=nan) == ERR_ARG and b"is NaN" in L.cilqr_last_error()
        assert call(dev, min_clearance=nan) == ERR_ARG and b"is NaN" in L.cilqr_last_error()
        assert call(dev, flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, reach=0.0, thr=inf, min_clearance=-inf, flags=1, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()


def test_the_closed_form_clearance_against_sampled_boundaries(scenes):
    """Outside the rectangle never above the distance to a densely sampled boundary and at most one sample spacing below it; inside, minus
    the penetration depth is that distance within one spacing."""
    from scipy.spatial import cKDTree
    spacing = 0.004
    s = scenes["T40"]
    g, pose, N = s["g"], s["poses"], s["N"]
    hl, hw = 0.5 * LENGTH + MARGIN, 0.5 * WIDTH + MARGIN
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    c, sn = math.cos(pose[2]), math.sin(pose[2])
    n_out = n_in = 0
    want = s[False]
    for r in range(0, s["R"], 2):
        X = s["X"][r].reshape(N + 1, 4)
        for t in range(0, N, 3):
            cell = int(want["cells"][r, t])
            if cell < 0:
                continue
            i, j = cell % g.rows, cell // g.rows
            mx, my = x_first - i * g.res, y_first - j * g.res
            w = np.array([[pose[0] + c * mx - sn * my, pose[1] + sn * mx + c * my]])
            sampled = float(cKDTree(boundary(X[t, 0], X[t, 1], X[t, 3], hl, hw, spacing)).query(w)[0][0])
            v = want["step_clearance"][r, t]
            if v > 0.0:
                assert v <= sampled + 1e-12 and sampled - v <= spacing, (r, t, v, sampled)
                n_out += 1
            else:
                assert -v <= sampled + 1e-12 and sampled + v <= spacing, (r, t, v, sampled)
                n_in += 1
    print("%d steps outside, %d inside" % (n_out, n_in))
    assert n_out >= 3 and n_in >= 10


def test_the_two_hand_cases(oracle):
    """One seed, map frame = planning frame, heading 0: in front of the bumper, s = the gap; under the body, s = minus the depth."""
    O = oracle
    p = O.default_params(1)
    g = O.map_geom(8.0, 4.0, 0.5, 0.0, 0.0)  # 16 x 8 cells; centres at x = 3.75 - 0.5 i, y = 1.75 - 0.5 j
    layer = np.zeros((16, 8), dtype=np.float32)
    layer[1, 3] = 100.0                      # centre (3.25, 0.25)
    hl, hw = 0.5 * p.length, 0.5 * p.width
    X = np.zeros((2, 8))
    X[0, 0], X[1, 0] = 0.0, 2.0
    w = clearance_restate(p, g, layer, (0.0, 0.0, 0.0), X, 1, 1, 0.0, 50.0, 5.0, 0.0, False)
    assert abs(w["mc"][0, CLEARANCE] - (3.25 - hl)) < 1e-15 and w["mc"][0, CELL] == 1 + 3 * 16
    assert abs(w["mc"][1, CLEARANCE] + min(hl - 1.25, hw - 0.25)) < 1e-15 and w["mc"][1, TOUCH_STEPS] == 1
    far = clearance_restate(p, g, layer, (0.0, 0.0, 0.0), X, 1, 1, 0.0, 50.0, 0.5, 0.0, False)
    assert far["mc"][0, CLEARANCE] == np.inf and far["mc"][0, STEP] == -1 and far["mc"][1, CLEARANCE] < 0


@pytest.mark.parametrize("name", SCENES)
def test_conditions(scenes, name):
    """On the restatement alone: every scene holds a step of each kind, and every value the device is compared on is decided."""
    s = scenes[name]
    for unknown in (False, True):
        w = s[unknown]
        sc, mc = w["step_clearance"], w["mc"]
        kinds = dict(positive=((sc > 0.0) & np.isfinite(sc)).sum(), touching=((sc <= 0.0) & np.isfinite(sc)).sum(), none=(sc == np.inf).sum(),
                     off_map=int(mc[:, OFF_MAP_STEPS].sum()), lost=(sc == -np.inf).sum())
        print("scene %s, unknown seeds %s: %s; clearance %s" % (name, unknown, kinds, np.round(mc[:, CLEARANCE], 4).tolist()))
        assert all(v >= 1 for v in kinds.values()), kinds
        assert mc[:, LOST_STEPS].sum() == 1
        finite = np.isfinite(sc)
        assert w["gap"][finite].min() > 1e-7 and w["edge"].min() > 1e-7        # a step's cell and the reach are decided
        assert w["step_gap"].min() > 1e-7                                           # a row's step is decided
        assert np.abs(sc[finite] - MIN_CLEARANCE).min() > 1e-7 and np.abs(sc[finite]).min() > 1e-7
        total = w["total"]
        assert np.isnan(total).any() and (np.isfinite(total).any() or unknown)
    a, b = s[False]["step_clearance"], s[True]["step_clearance"]
    assert not np.array_equal(a, b) and np.all(b <= a)  # the NaN cells matter, and more seeds never raise a clearance
    if isinstance(s["layers"], list):
        alt = clearance_restate(s["p"], s["g"], s["layers"][0], s["poses"][0], s["X"], s["N"], s["S"], MARGIN, THRESHOLD, REACH, MIN_CLEARANCE, False)
        assert not np.array_equal(alt["step_clearance"][-1], a[-1])  # the last solve's own layer and pose matter


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(_params(cilqr), max_batch=16, max_horizon=50, max_obstacles=0, device=0)
    yield s
    s.close()


def _host(cilqr, solver, s, unknown, rows=None, steps=True, base=True, min_clearance=MIN_CLEARANCE, reach=REACH):
    """The host form for the rows `rows` (whole solves, in that order) of the scene."""
    S = s["S"]
    idx = list(range(s["R"])) if rows is None else list(rows)
    solves = [idx[k] // S for k in range(0, len(idx), S)]
    with _Map(cilqr, solver, s, sel=solves if isinstance(s["layers"], list) else None):
        return solver.map_clearance(s["N"], s["X"][idx], reach, S=S, margin=MARGIN, occ_threshold=THRESHOLD, min_clearance=min_clearance,
                                    base=s["base"][idx] if base else None, unknown_seeds=unknown, steps=steps)


def _device(cilqr, solver, s, unknown, rows=None, pick=False):
    import torch
    S = s["S"]
    idx = list(range(s["R"])) if rows is None else list(rows)
    solves = [idx[k] // S for k in range(0, len(idx), S)]
    R, N = len(idx), s["N"]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    X, base = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (s["X"][idx], s["base"][idx]))
    mc, sc, total = (torch.full(shape, -7.0, dtype=torch.float64, device=dev) for shape in ((R, 8), (R, N), (R,)))
    pair = torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    with _Map(cilqr, solver, s, sel=solves if isinstance(s["layers"], list) else None):
        solver.map_clearance_device(st, R // S, N, S, X.data_ptr(), mc.data_ptr(), REACH, margin=MARGIN, occ_threshold=THRESHOLD,
                                    min_clearance=MIN_CLEARANCE, flags=1 if unknown else 0, base=base.data_ptr(), step_clearance=sc.data_ptr(),
                                    total=total.data_ptr())
        if pick:
            solver.argmin_device(st, R, total.data_ptr(), pair.data_ptr())
        torch.cuda.synchronize(dev)
    return dict(mc=mc.cpu().numpy(), step_clearance=sc.cpu().numpy(), total=total.cpu().numpy(), pair=pair.cpu().numpy())


def _close(a, b):
    inf = np.isinf(b)
    return np.array_equal(a[inf], b[inf]) and bool(np.all(np.abs(a[~inf] - b[~inf]) <= ABS_TOL))


def _check_against(got, want, what, rows=slice(None)):
    mc, w = got["mc"], want["mc"][rows]
    print("%s: clearance %s (want %s), step %s, cell %s, below %s, touching %s, off the map %s, lost %s" % (
        what, mc[:, CLEARANCE].tolist(), w[:, CLEARANCE].tolist(), mc[:, STEP].tolist(), mc[:, CELL].tolist(), mc[:, BELOW_STEPS].tolist(),
        mc[:, TOUCH_STEPS].tolist(), mc[:, OFF_MAP_STEPS].tolist(), mc[:, LOST_STEPS].tolist()))
    assert _close(mc[:, CLEARANCE], w[:, CLEARANCE]), what
    for f in range(1, 8):
        assert np.array_equal(mc[:, f], w[:, f]), (what, FIELDS[f], mc[:, f].tolist(), w[:, f].tolist())
    if got["step_clearance"] is not None:
        assert _close(got["step_clearance"], want["step_clearance"][rows]), what
    if got["total"] is not None:
        assert np.array_equal(_bits(got["total"]), _bits(want["total"][rows])), (what, got["total"], want["total"][rows])


def _same_bits(a, b, rows_b=slice(None)):
    return all(np.array_equal(_bits(a[k]), _bits(b[k][rows_b])) for k in ("mc", "step_clearance", "total"))


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_fields_against_the_restatement(cilqr, solver, scenes, name):
    """Both settings of UNKNOWN_SEEDS; the host form and the device form agree bit for bit."""
    s = scenes[name]
    for unknown in (False, True):
        host = _host(cilqr, solver, s, unknown)
        _check_against(host, s[unknown], "scene %s, unknown seeds %s, host form" % (name, unknown))
        dev = _device(cilqr, solver, s, unknown)
        _check_against(dev, s[unknown], "scene %s, unknown seeds %s, device form" % (name, unknown))
        assert _same_bits(host, dev)


@gpu
def test_a_rows_bits_do_not_depend_on_its_place(cilqr, solver, scenes):
    s = scenes["T40"]
    whole = _host(cilqr, solver, s, False)
    for order in ([4, 0, 5, 2], [3], [5, 4, 3, 2, 1, 0]):
        assert _same_bits(_host(cilqr, solver, s, False, rows=order), whole, rows_b=order), order
    p = scenes["P40"]  # rows travel with their solve's layer and pose: solves 2, 0 are rows 4, 5, 0, 1
    whole = _host(cilqr, solver, p, True)
    order = [4, 5, 0, 1]
    assert _same_bits(_host(cilqr, solver, p, True, rows=order), whole, rows_b=order)
    small = cilqr.Solver(_params(cilqr), max_batch=6, max_horizon=40, max_obstacles=0, device=0)
    try:
        assert _same_bits(_host(cilqr, small, s, False), _host(cilqr, solver, s, False))
    finally:
        small.close()


@gpu
def test_every_optional_output_left_out(cilqr, solver, scenes):
    s = scenes["R5"]
    full = _host(cilqr, solver, s, False)
    bare = _host(cilqr, solver, s, False, steps=False, base=False)
    assert bare["step_clearance"] is None and bare["total"] is None and np.array_equal(_bits(bare["mc"]), _bits(full["mc"]))
    no_steps = _host(cilqr, solver, s, False, steps=False)
    assert np.array_equal(_bits(no_steps["total"]), _bits(full["total"])) and np.array_equal(_bits(no_steps["mc"]), _bits(full["mc"]))


@gpu
def test_total_thresholds_and_the_pick(cilqr, solver, scenes):
    """total = base where the row has no lost step and its clearance is >= min_clearance, at thresholds on either side of every row's
    clearance; cilqr_argmin_device picks the cheapest row that is clear."""
    s = scenes["T40"]
    want = s[False]
    c = want["mc"][:, CLEARANCE]
    for thr in [-np.inf, np.inf] + [float(v) for v in np.sort(c[np.isfinite(c)])[[0, -1]]]:
        for eps in (-1e-6, 1e-6):
            got = _host(cilqr, solver, s, False, min_clearance=thr + eps if np.isfinite(thr) else thr)
            ok = (want["mc"][:, LOST_STEPS] == 0) & (c >= (thr + eps if np.isfinite(thr) else thr))
            assert np.array_equal(np.isfinite(got["total"]), ok), (thr, eps, got["total"], c)
            assert np.array_equal(got["total"][ok], s["base"][ok])
    # a reach that finds nothing: every row without a lost step is clear, whatever min_clearance is
    got = _host(cilqr, solver, s, False, reach=0.0, min_clearance=1e300)
    inside = want["mc"][:, TOUCH_STEPS] - want["mc"][:, LOST_STEPS] > 0
    assert np.array_equal(np.isfinite(got["total"]), ~inside & (want["mc"][:, LOST_STEPS] == 0)) and np.isfinite(got["total"]).any()
    dev = _device(cilqr, solver, s, False, pick=True)
    masked = np.where(np.isfinite(want["total"]), want["total"], np.inf)
    assert np.isfinite(masked).any() and int(np.argmin(masked)) != int(np.argmin(s["base"]))  # the cheapest row is not clear
    assert dev["pair"][1] == float(np.argmin(masked)) and dev["pair"][0] == masked.min()


@gpu
def test_limits(cilqr, scenes):
    """No map set: CILQR_ERR_ARG, saying so.  B*S or N beyond the handle's: CILQR_ERR_ARG.  A reach whose window spans more than 1024
    cells: CILQR_ERR_UNSUPPORTED; the largest one that does not runs."""
    s = scenes["S3"]
    sv = cilqr.Solver(_params(cilqr), max_batch=3, max_horizon=s["N"], max_obstacles=0, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*no uncertainty map" % ERR_ARG):
            sv.map_clearance(s["N"], s["X"], REACH, S=3)
        with _Map(cilqr, sv, s):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*B\\*S = 4 outside" % ERR_ARG):
                sv.map_clearance(s["N"], np.concatenate([s["X"], s["X"][:1]]), REACH, S=1)
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: N=%d outside" % (ERR_ARG, s["N"] + 1)):
                sv.map_clearance(s["N"] + 1, np.zeros((3, 4 * (s["N"] + 2))), REACH)
            hl, hw = 0.5 * LENGTH + MARGIN, 0.5 * WIDTH + MARGIN
            edge = 0.5 * 0.1 * 1022 - math.hypot(hl, hw)  # ceil(2 (hypot + reach) / res) + 2 = 1024 exactly
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*more than 1024 cells" % ERR_UNSUPPORTED):
                sv.map_clearance(s["N"], s["X"], edge + 0.06, S=3, margin=MARGIN)
            got = sv.map_clearance(s["N"], s["X"], edge - 0.01, S=3, margin=MARGIN, occ_threshold=THRESHOLD, min_clearance=MIN_CLEARANCE, base=s["base"])
        want = clearance_restate(s["p"], s["g"], s["layers"], s["poses"], s["X"], s["N"], 3, MARGIN, THRESHOLD, edge - 0.01, MIN_CLEARANCE, False, s["base"])
        assert _close(got["step_clearance"], want["step_clearance"]) and np.array_equal(got["mc"][:, [BELOW_STEPS, TOUCH_STEPS, OFF_MAP_STEPS, LOST_STEPS]],
                                                                                        want["mc"][:, [BELOW_STEPS, TOUCH_STEPS, OFF_MAP_STEPS, LOST_STEPS]])
        assert want["mc"][:, OFF_MAP_STEPS].tolist() == [s["N"] - (1 if r == 2 else 0) for r in range(3)]  # every window leaves the map; one step is lost
    finally:
        sv.close()


@gpu
def test_cpp_facade_map_clearance_checked_candidates(six, tmp_path):
    """tests/cpp/candidates_map_clearance.cpp: run_candidates under iLQR::set_map_clearance_check against the C-ABI sequence called by hand,
    bit for bit (inside the program), and its clearances against the restatement on the oracle's solves (here)."""
    exe = _build(tmp_path, "candidates_map_clearance.cpp", os.path.join(ROOT, "include"), os.path.join(PKG, "host"), lib=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map clearance pick ok" in r.stdout
    got = np.array([float(v) for v in re.search(r"clearances:(.*)", r.stdout).group(1).split()])
    J = np.array([float(v) for v in re.search(r"J:(.*)", r.stdout).group(1).split()])
    # (the program's plans are the device's, 1e-9 from the oracle's, and its layer is libm's where the scene's is numpy's)
    assert np.max(np.abs(got - six["want"]["mc"][:, CLEARANCE])) <= 1e-6 and np.max(np.abs(J - six["solve"]["J"])) <= 1e-6
