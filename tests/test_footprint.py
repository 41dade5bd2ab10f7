"""Exact footprint check (cilqr_footprint_check*, include/cilqr.h): the vehicle's rectangle against obstacle rectangles (separating
axes, and the exact distance where separated) and against the cells of the map set on the handle (Polygon::isInside of every centre).

Expected values never come from the HIP path.  They come from `restate` below: plain float64, math.sin / math.cos, and the crossing
test of tests/test_polygon_raster.py (`inside_mask`) on cell centres taken as that file takes them.  No reference binary can pin it
(the reference's Experiment.cpp includes a header it does not ship), so the restatement itself is checked on the CPU against
independent forms: the reference's isCollision restated literally, densely sampled boundaries, matplotlib's point-in-path, two cases
worked by hand, and the six-candidate table of DESIGN §4.8o from the oracle's solves.

Tolerances are the suite's own: 1e-9 absolute on FP_CLEARANCE and step_clearance (ABS_TOL of tests/test_candidate_score.py), equality
on every index, count and map field, step_occ as bit patterns.  What makes the exact comparisons meaningful is asserted on the
restatement, for every GPU scene, in test_conditions: no |clearance| below 1e-6, the two smallest clearances of a row more than 1e-6
apart, no cell centre within 1e-9 of a footprint edge (crossing abscissa and straddle test), no occupancy within 1e-6 of the threshold;
equal occupancies are resolved by the index rule on both sides (float equality is exact).

Scenes (rows are synthetic arcs at 5 m/s: the call judges any row, solved or not):
  T1, T5, T50   N = 1, 5, 50: one step, a partial group of four, the workload's horizon; (B, S) = (1, 1), (3, 1), (2, 3);
                M = 1, 3, 70 dense; the 150 x 100 map at 0.1 m, shared, pose (0.3, -0.2, 0.05); margin 0 and 0.137
  SH, ST        T50's rows against obstacles shared (0, N, 1) and static (0, 1, 0): bit-equal to their dense expansion
  P             per-solve layers and poses (device form), the 12 x 9 map at 1 m: a bounding box under 64 cells
  E             M = 0 and no map: the empty values
"""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import ABS_TOL, MARGIN, MAX_C, COLLISION, _bits, _circle_values, _expected, _one_circle_params, _totals
from test_polygon_raster import inside_mask

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_footprint_check", "cilqr_footprint_check_device")
FIELDS = ("CLEARANCE", "CLEARANCE_ENTRY", "HIT_STEPS", "FIRST_HIT", "MAP_OCC", "MAP_OCC_STEP", "MAP_OCC_CELL", "MAP_HIT_STEPS",
          "MAP_FIRST_HIT", "MAP_HIT_CELLS", "MAP_UNKNOWN_STEPS", "MAP_CELLS")
(CLEARANCE, CLEARANCE_ENTRY, HIT_STEPS, FIRST_HIT, MAP_OCC, MAP_OCC_STEP, MAP_OCC_CELL, MAP_HIT_STEPS, MAP_FIRST_HIT, MAP_HIT_CELLS,
 MAP_UNKNOWN_STEPS, MAP_CELLS) = range(12)
UNKNOWN_HITS, SKIP_MAP = 1, 2
EDGE = 1e-9
LENGTH, WIDTH = 4.79, 2.16  # Parameters::length / width (cilqr_params_default)
GEOM_BIG, GEOM_SMALL = (15.0, 10.0, 0.1, 7.5, 0.0), (12.0, 9.0, 1.0, 6.0, 0.5)
POSE_SHARED = (0.3, -0.2, 0.05)
THRESHOLD = 97.5  # the layers hold whole numbers: no occupancy is within 1e-6 of it; only the patches' peaks are above
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _frame(th):
    c, s = math.cos(th), math.sin(th)
    return (c, s), (-s, c)


def clearance(ex, ey, eth, hl, hw, ox, oy, oth, ol, ow):
    """Signed clearance of two rectangles by the header's statements: the four gaps, then the eight vertex distances where separated."""
    E = (ex, ey, _frame(eth), hl, hw)
    O = (ox, oy, _frame(oth), ol, ow)

    def radius(R, u):
        (a, b), l, w = R[2], R[3], R[4]
        return l * abs(u[0] * a[0] + u[1] * a[1]) + w * abs(u[0] * b[0] + u[1] * b[1])
    d = (ox - ex, oy - ey)
    g = max(abs(u[0] * d[0] + u[1] * d[1]) - (radius(E, u) + radius(O, u)) for u in E[2] + O[2])
    if not g > 0.0:
        return g

    def vertices(R):
        (a, b), l, w = R[2], R[3], R[4]
        return [(R[0] + sa * l * a[0] + sb * w * b[0], R[1] + sa * l * a[1] + sb * w * b[1]) for sa in (1, -1) for sb in (1, -1)]

    def to_box(P, R):
        (a, b), l, w = R[2], R[3], R[4]
        px, py = P[0] - R[0], P[1] - R[1]
        return math.hypot(max(abs(px * a[0] + py * a[1]) - l, 0.0), max(abs(px * b[0] + py * b[1]) - w, 0.0))
    return min([to_box(P, O) for P in vertices(E)] + [to_box(P, E) for P in vertices(O)])


def corners_world(x, y, th, hl, hw):
    """bondingBoxHandle's order: (hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw)."""
    ct, st = math.cos(th), math.sin(th)
    return [(x + (a * ct - b * st), y + (a * st + b * ct)) for a, b in ((hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw))]


def corners_map(x, y, th, hl, hw, pose):
    px, py, pth = pose
    cp, sp = math.cos(pth), math.sin(pth)
    out = []
    for Px, Py in corners_world(x, y, th, hl, hw):
        dx, dy = Px - px, Py - py
        out.append((cp * dx + sp * dy, cp * dy - sp * dx))
    return out


def first_cell(g):
    return g.pos_x + (0.5 * g.len_x - 0.5 * g.res), g.pos_y + (0.5 * g.len_y - 0.5 * g.res)


def covered_cells(g, quad):
    """(i, j) arrays of the VIRTUAL cells whose centre passes the crossing test for the 4-gon, lowest i + j*rows first, and the
    smallest distance of any centre of the window to a crossing abscissa / of any vertex ordinate to a row of centres."""
    xf, yf = first_cell(g)
    xs, ys = [q[0] for q in quad], [q[1] for q in quad]
    i = np.arange(math.floor((xf - max(xs)) / g.res) - 2, math.ceil((xf - min(xs)) / g.res) + 3)
    j = np.arange(math.floor((yf - max(ys)) / g.res) - 2, math.ceil((yf - min(ys)) / g.res) + 3)
    cx, cy = xf + g.res * (-i).astype(np.float64), yf + g.res * (-j).astype(np.float64)
    mask = inside_mask(cx, cy, [quad])
    edge = np.inf
    for k in range(4):
        (xi, yi), (xj, yj) = quad[k], quad[k - 1]
        straddle = (yi > cy) != (yj > cy)
        edge = min(edge, float(np.min(np.abs(cy - yi))))
        if straddle.any():
            at = (xj - xi) * (cy[straddle] - yi) / (yj - yi) + xi
            edge = min(edge, float(np.min(np.abs(cx[:, None] - at[None, :]))))
    ii, jj = np.nonzero(mask)
    order = np.lexsort((ii, jj))  # j slowest: ascending i + j*rows for the cells inside the map
    return i[ii[order]], j[jj[order]], edge


def restate(p, N, X, S=1, pose=None, dim=None, margin=0.0, min_clearance=0.0, threshold=math.inf, unknown_hits=False, skip_map=False,
            umap=None, base=None):
    """X (R, 4(N+1)); pose (B, M, 4N) / dim (B, M, 2N) dense or None; umap None or dict(g, layers: one (rows, cols) float32 or a list
    of B, poses: one or a list of B).  Returns dict(fp (R, 12), step_clearance, step_occ, total, entry (R, M, N) clearances with NaN
    where an entry has none, cells: per (row, step) the covered (i, j), edge: the smallest centre-to-edge distance met)."""
    R = X.shape[0]
    B = R // S
    M = 0 if pose is None else pose.shape[1]
    hl, hw = 0.5 * p.length + margin, 0.5 * p.width + margin
    st = X.reshape(R, N + 1, 4)
    fp = np.zeros((R, 12))
    sc, so = np.full((R, N), np.inf), np.full((R, N), np.nan, dtype=np.float32)
    entry = np.full((R, M, N), np.nan)
    map_on = umap is not None and not skip_map
    cells, edge = {}, np.inf
    for r in range(R):
        b = r // S
        lost = ~np.isfinite(st[r, :N][:, [0, 1, 3]]).all(axis=1)
        hit = lost.copy()
        for t in range(N):
            if lost[t]:
                sc[r, t] = -np.inf
                continue
            x, y, th = st[r, t, 0], st[r, t, 1], st[r, t, 3]
            for m in range(M):
                o, d = pose[b, m, 4 * t:4 * t + 4], dim[b, m, 2 * t:2 * t + 2]
                if not (np.isfinite(o[[0, 1, 3]]).all() and np.isfinite(d).all() and d[0] >= 0 and d[1] >= 0):
                    hit[t] = True
                    continue
                c = clearance(x, y, th, hl, hw, o[0], o[1], o[3], 0.5 * d[0], 0.5 * d[1])
                entry[r, m, t] = c
                sc[r, t] = min(sc[r, t], c)
                hit[t] |= c <= 0.0
        flat = entry[r].reshape(-1)
        if np.isfinite(flat).any():
            e = int(np.nanargmin(flat))  # the lowest index of the minimum
            fp[r, CLEARANCE], fp[r, CLEARANCE_ENTRY] = flat[e], e
        else:
            fp[r, CLEARANCE], fp[r, CLEARANCE_ENTRY] = np.inf, -1
        fp[r, HIT_STEPS], fp[r, FIRST_HIT] = hit.sum(), (int(np.argmax(hit)) if hit.any() else -1)
        fp[r, MAP_OCC], fp[r, MAP_OCC_STEP], fp[r, MAP_OCC_CELL], fp[r, MAP_FIRST_HIT] = -np.inf, -1, -1, -1
        if not map_on:
            continue
        g = umap["g"]
        layer = umap["layers"][b] if isinstance(umap["layers"], list) else umap["layers"]
        mpose = umap["poses"][b] if isinstance(umap["poses"], list) else umap["poses"]
        for t in range(N):
            if lost[t]:
                mhit, unknown, n_cells, n_above, best = True, True, 0, 0, None
            else:
                quad = corners_map(st[r, t, 0], st[r, t, 1], st[r, t, 3], hl, hw, mpose)
                ci, cj, e = covered_cells(g, quad)
                edge = min(edge, e)
                cells[(r, t)] = (ci, cj)
                inm = (ci >= 0) & (ci < g.rows) & (cj >= 0) & (cj < g.cols)
                v = layer[ci[inm], cj[inm]]
                unknown = bool((~inm).any() or np.isnan(v).any())
                n_cells, n_above = ci.size, int((v.astype(np.float64) > threshold).sum())  # (NaN compares false)
                fin = np.isfinite(v)
                best = None
                if fin.any():
                    k = int(np.argmax(np.where(fin, v, -np.inf)))  # first of the maximum: the lowest cell
                    best = (v[k], int(ci[inm][k] + cj[inm][k] * g.rows))
                mhit = n_above > 0 or (unknown_hits and unknown)
            if best is not None:
                so[r, t] = best[0]
                if best[0] > fp[r, MAP_OCC]:
                    fp[r, MAP_OCC], fp[r, MAP_OCC_STEP], fp[r, MAP_OCC_CELL] = best[0], t, best[1]
            if mhit:
                fp[r, MAP_HIT_STEPS] += 1
                if fp[r, MAP_FIRST_HIT] < 0:
                    fp[r, MAP_FIRST_HIT] = t
            fp[r, MAP_HIT_CELLS] = max(fp[r, MAP_HIT_CELLS], n_above)
            fp[r, MAP_UNKNOWN_STEPS] += unknown
            fp[r, MAP_CELLS] += n_cells
    total = None
    if base is not None:
        ok = np.isfinite(base) & (fp[:, HIT_STEPS] == 0) & (fp[:, CLEARANCE] >= min_clearance) & (fp[:, MAP_HIT_STEPS] == 0)
        total = np.where(ok, base, np.nan)
    return dict(fp=fp, step_clearance=sc, step_occ=so, total=total, entry=entry, cells=cells, edge=edge)


# ---- independent forms the restatement is checked against ------------------------------------------------------------------------
def sat_literal(v1, v2):
    """The reference's collision test of two vehicles (x, y, yaw, length, width), restated: corners from (-l/2, -w/2) counter-clockwise,
    four axes as the atan2 of the edges 0->1 and 0->3 of each, min / max corner projections, separated when max1 < min2 or
    max2 < min1 (strict: touching collides)."""
    def corners(v):
        x, y, yaw, length, width = v
        hl, hw = length / 2.0, width / 2.0
        return [(x + (a * math.cos(yaw) - b * math.sin(yaw)), y + (a * math.sin(yaw) + b * math.cos(yaw)))
                for a, b in ((-hl, -hw), (hl, -hw), (hl, hw), (-hl, hw))]
    c1, c2 = corners(v1), corners(v2)
    axes = [math.atan2(c[k][1] - c[0][1], c[k][0] - c[0][0]) for c in (c1, c2) for k in (1, 3)]
    for axis in axes:
        p1 = [q[0] * math.cos(axis) + q[1] * math.sin(axis) for q in c1]
        p2 = [q[0] * math.cos(axis) + q[1] * math.sin(axis) for q in c2]
        if max(p1) < min(p2) or max(p2) < min(p1):
            return False
    return True


def boundary(x, y, th, hl, hw, spacing):
    """Points along the rectangle's boundary, at most `spacing` apart."""
    q = corners_world(x, y, th, hl, hw)
    pts = []
    for k in range(4):
        (x0, y0), (x1, y1) = q[k - 1], q[k]
        n = int(math.ceil(math.hypot(x1 - x0, y1 - y0) / spacing)) + 1
        s = np.linspace(0.0, 1.0, n)
        pts.append(np.stack([x0 + s * (x1 - x0), y0 + s * (y1 - y0)], axis=1))
    return np.concatenate(pts)


# ---- scenes --------------------------------------------------------------------------------------------------------------------
HEADINGS = (0.0, math.pi / 2, -2.2, 7.0)


def arcs(R, N, seed, start=(2.0, 0.0)):
    """R rows [4(N+1)]: arcs at 5 m/s from near `start`, headings 0, pi/2, -2.2, 7.0 in turn, a yaw rate of a few degrees per step."""
    rng = np.random.default_rng(seed)
    X = np.zeros((R, N + 1, 4))
    for r in range(R):
        x, y = start[0] + rng.uniform(-0.5, 0.5), start[1] + rng.uniform(-0.5, 0.5)
        th, w = HEADINGS[r % 4] + rng.uniform(-0.01, 0.01), rng.uniform(-0.05, 0.05)
        for t in range(N + 1):
            X[r, t] = (x, y, 5.0, th)
            x, y, th = x + 0.5 * math.cos(th), y + 0.5 * math.sin(th), th + w
    return X.reshape(R, 4 * (N + 1))


def boxes(B, M, N, seed, X, S):
    """Dense (B, M, 4N) / (B, M, 2N): boxes of 0.4 ... 5 m drifting near the rows of their solve; about a third overlap a row."""
    rng = np.random.default_rng(seed)
    pose, dim = np.zeros((B, M, N, 4)), np.zeros((B, M, N, 2))
    st = X.reshape(-1, N + 1, 4)
    for b in range(B):
        for m in range(M):
            t0 = int(rng.integers(0, N))
            cx, cy = st[b * S, t0, 0] + rng.normal(0.0, 4.0), st[b * S, t0, 1] + rng.normal(0.0, 4.0)
            th, vx, vy = rng.uniform(-math.pi, math.pi), rng.normal(0.0, 0.1), rng.normal(0.0, 0.1)
            l, w = rng.uniform(0.4, 5.0), rng.uniform(0.4, 2.5)
            for t in range(N):
                pose[b, m, t] = (cx + vx * t, cy + vy * t, 1.0, th + 0.01 * t)
                dim[b, m, t] = (l, w)
    return pose.reshape(B, M, 4 * N), dim.reshape(B, M, 2 * N)


def whole_layer(rows, cols, seed, nan_share=0.0003):
    """Whole numbers 0 ... 100 in smooth patches (many equal neighbours: the index rule decides), a few NaN cells."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = 50.0 + 50.0 * np.sin(0.13 * i + rng.uniform(0, 6)) * np.cos(0.11 * j + rng.uniform(0, 6))
    layer = np.round(z).astype(np.float32)
    layer[rng.random((rows, cols)) < nan_share] = np.nan
    return layer


def _scene(O, name, B, S, N, M, margin, seed, geom=None, per_solve=False):
    p = O.default_params(N)
    R = B * S
    X = arcs(R, N, seed)
    pose, dim = boxes(B, M, N, seed + 1, X, S) if M else (None, None)
    umap = None
    if geom is not None:
        g = O.map_geom(*geom)
        if per_solve:
            umap = dict(g=g, geom=geom, layers=[whole_layer(g.rows, g.cols, seed + 10 + b) for b in range(B)],
                        poses=[(0.2 * b, -0.1 * b, 0.3 * b - 0.2) for b in range(B)])
        else:
            umap = dict(g=g, geom=geom, layers=whole_layer(g.rows, g.cols, seed + 10), poses=POSE_SHARED)
    base = np.linspace(5.0, 4.0, R)
    s = dict(name=name, p=p, B=B, S=S, N=N, M=M, R=R, X=X, pose=pose, dim=dim, margin=margin, umap=umap, base=base, threshold=THRESHOLD)
    for flag in (False, True):
        s[flag] = restate(p, N, X, S, pose, dim, margin, 0.0, THRESHOLD, flag, False, umap, base)
    return s


@pytest.fixture(scope="module")
def scenes(oracle):
    """Computed once, shared, never modified."""
    O = oracle
    out = {}
    out["T1"] = _scene(O, "T1", 1, 1, 1, 1, 0.0, 100, GEOM_BIG)
    out["T5"] = _scene(O, "T5", 3, 1, 5, 3, 0.137, 200, GEOM_BIG)
    out["T50"] = _scene(O, "T50", 2, 3, 50, 70, 0.0, 300, GEOM_BIG)
    out["P"] = _scene(O, "P", 3, 1, 5, 3, 0.137, 400, GEOM_SMALL, per_solve=True)
    out["E"] = _scene(O, "E", 2, 1, 5, 0, 0.0, 500)
    return out


GPU_SCENES = ["T1", "T5", "T50", "P", "E"]


# ---- the six-candidate scene ----------------------------------------------------------------------------------------
SIX_N, SIX_B = 40, 6
SIX_POST = (8.0, 1.2, 0.5, 0.5)
SIX_TABLE = [(21.77, 0.082, 1.013), (21.30, 0.070, 1.054), (22.15, 0.056, 1.096), (24.32, 0.039, 1.126), (27.83, 0.021, 1.154),
             (32.69, 0.001, 1.182)]  # J, max c, exact clearance
# what tests/cpp/candidates_footprint.cpp asserts, first asserted here from the oracle's solves
SIX_MIN_CLEARANCE_LOW, SIX_MIN_CLEARANCE_BETWEEN = 0.5, 1.11


@pytest.fixture(scope="module")
def six(oracle):
    O = oracle
    N, B = SIX_N, SIX_B
    p = O.default_params(N)
    path = np.stack([np.arange(200.0), np.zeros(200)], axis=1)
    x0 = np.array([[0.0, -0.3 * b, 5.0, 0.0] for b in range(B)])
    plans = [O.local_plan(p, path, x0[b]) for b in range(B)]
    poly, fl = np.array([c for c, _ in plans]), np.array([[ref[0, 0], ref[-1, 0]] for _, ref in plans])
    U = np.tile(O.default_control_seq(N), (B, 1))
    pose = np.tile(np.array([SIX_POST[0], SIX_POST[1], 0.0, 0.0]), (B, 1, N)).reshape(B, 1, 4 * N)
    dim = np.tile(np.array(SIX_POST[2:]), (B, 1, N)).reshape(B, 1, 2 * N)
    r = O.solve_batch(p, N, 1, x0, U, poly, fl, pose, dim, None, threads=min(6, O.max_threads()))
    rows, _ = _expected(O, p, N, r["X"], r["U"], poly, fl, pose, dim)
    w = restate(p, N, r["X"], 1, pose, dim)
    return dict(p=p, N=N, B=B, x0=x0, U0=U, poly=poly, fl=fl, pose=pose, dim=dim, X=r["X"], U=r["U"], J=r["J"], rows=rows, total=_totals(rows), fp=w["fp"], w=w)


# ---- CPU: declarations ---------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_call(cilqr):
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cilqr.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_FOOTPRINT_FIELDS\s+12\b", h)
    assert re.search(r"#define\s+CILQR_FOOTPRINT_UNKNOWN_HITS\s+1u", h) and re.search(r"#define\s+CILQR_FOOTPRINT_SKIP_MAP\s+2u", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_FP_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "FP_" + name) == i
    assert cilqr.FOOTPRINT_FIELDS == 12 and (cilqr.FOOTPRINT_UNKNOWN_HITS, cilqr.FOOTPRINT_SKIP_MAP) == (1, 2)
    assert callable(cilqr.Solver.footprint_check) and callable(cilqr.Solver.footprint_check_device)
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    assert "a row's bits depend on that row's inputs alone" in full  # the determinism statement
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_footprint_check\s*\(\s*double\s+min_clearance\s*,\s*double\s+occ_threshold\s*,\s*double\s+margin\s*=\s*0\.0\s*,"
                     r"\s*bool\s+unknown_hits\s*=\s*false\s*,\s*bool\s+on\s*=\s*true\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_footprint\b", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_footprint\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_footprint.hip" in mk and re.search(r"check_kernel_resources\.py --map .*build/cilqr_footprint\.o", mk)


def test_argument_errors_need_no_device(cilqr):
    """NULL X or fp, obs NULL with M > 0, total without base, S < 1, a negative stride, a margin that is negative or not finite, a NaN
    min_clearance or occ_threshold, unknown flag bits: CILQR_ERR_ARG, decided before the handle is looked at (there is none here)."""
    L = cilqr.lib()
    B, N, M = 2, 4, 1
    X, fp, base, total = np.zeros((B, 4 * (N + 1))), np.zeros((B, 12)), np.zeros(B), np.zeros(B)
    pose, dim = np.zeros((M, 4)), np.ones((M, 2))
    no_handle, d, nan = C.c_void_p(), C.c_double, float("nan")

    def call(dev, M_=M, S=1, stride=0, margin=0.0, mc=0.0, thr=50.0, flags=0, obs=True, **nulls):
        a = dict(X=X, fp=fp, base=base, total=total)
        a.update(nulls)
        o = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, 0, 1, stride, 0)
        f = L.cilqr_footprint_check_device if dev else L.cilqr_footprint_check
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, M_, S, _p(a["X"]), C.byref(o) if obs else None, d(margin), d(mc), d(thr), C.c_uint32(flags), _p(a["base"]),
                 _p(a["fp"]), None, None, _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "fp"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, obs=False) == ERR_ARG and b"is null" in L.cilqr_last_error()
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert call(dev, S=0) == ERR_ARG and b"at least 1" in L.cilqr_last_error()
        assert call(dev, stride=-1) == ERR_ARG and b"negative stride" in L.cilqr_last_error()
        for margin in (-0.1, nan, float("inf")):
            assert call(dev, margin=margin) == ERR_ARG and b"margin" in L.cilqr_last_error(), margin
        for kw in ("mc", "thr"):
            assert call(dev, **{kw: nan}) == ERR_ARG and b"NaN" in L.cilqr_last_error(), kw
        assert call(dev, flags=4) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev, flags=3, mc=-math.inf, thr=math.inf) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid, no handle
        assert call(dev, M_=0, obs=False, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()


# ---- CPU: the restatement against independent forms -------------------------------------------------------------------------------
def _all_entries(s):
    """(ego state, obstacle pose, dims, clearance) of every entry of a scene that has a clearance value."""
    st = s["X"].reshape(s["R"], s["N"] + 1, 4)
    for r, m, t in zip(*np.nonzero(np.isfinite(s[False]["entry"]))):
        b = r // s["S"]
        yield st[r, t], s["pose"][b, m, 4 * t:4 * t + 4], s["dim"][b, m, 2 * t:2 * t + 2], s[False]["entry"][r, m, t]


def test_the_hit_flag_is_the_references_collision_test(scenes, six):
    """isCollision's own statements, restated literally, give the restatement's hit flag (clearance <= 0) on every entry of every
    scene used below."""
    n = hits = 0
    six_scene = dict(six, name="six", R=six["B"], S=1, margin=0.0)
    six_scene[False] = six["w"]
    for s in list(scenes.values()) + [six_scene]:
        if s["pose"] is None:
            continue
        hl, hw = 0.5 * LENGTH + s["margin"], 0.5 * WIDTH + s["margin"]
        for e, o, d, c in _all_entries(s):
            want = sat_literal((e[0], e[1], e[3], 2 * hl, 2 * hw), (o[0], o[1], o[3], d[0], d[1]))
            assert want == (c <= 0.0), (s.get("name"), e, o, d, c)
            n += 1
            hits += want
    print("%d entries, %d of them collisions" % (n, hits))
    assert n > 5000 and 50 < hits < n - 50


def test_the_closed_form_clearance_against_sampled_boundaries(scenes):
    """Never above the distance between densely sampled boundaries, and at most one sample spacing below it (separated pairs; for
    overlapping ones the sampled distance of the boundaries is not the overlap)."""
    from scipy.spatial import cKDTree
    spacing, n = 0.004, 0
    s = scenes["T50"]
    hl, hw = 0.5 * LENGTH + s["margin"], 0.5 * WIDTH + s["margin"]
    for k, (e, o, d, c) in enumerate(_all_entries(s)):
        if k % 17 or not 0.0 < c < 6.0:
            continue
        a, b = boundary(e[0], e[1], e[3], hl, hw, spacing), boundary(o[0], o[1], o[3], 0.5 * d[0], 0.5 * d[1], spacing)
        sampled = float(cKDTree(a).query(b)[0].min())
        assert c <= sampled + 1e-12 and sampled - c <= spacing, (e, o, d, c, sampled)
        n += 1
    print("%d separated pairs" % n)
    assert n > 150


def test_the_crossing_test_against_matplotlib(scenes):
    """matplotlib.path.Path.contains_points agrees with the crossing test on every cell centre farther than 1e-6 from an edge."""
    from matplotlib.path import Path
    n = 0
    for name in ("T5", "P"):
        s = scenes[name]
        g = s["umap"]["g"]
        xf, yf = first_cell(g)
        st = s["X"].reshape(s["R"], s["N"] + 1, 4)
        hl, hw = 0.5 * LENGTH + s["margin"], 0.5 * WIDTH + s["margin"]
        for (r, t), (ci, cj) in s[False]["cells"].items():
            mpose = s["umap"]["poses"][r // s["S"]] if isinstance(s["umap"]["poses"], list) else s["umap"]["poses"]
            quad = np.array(corners_map(st[r, t, 0], st[r, t, 1], st[r, t, 3], hl, hw, mpose))
            i = np.arange(ci.min() - 3, ci.max() + 4) if ci.size else np.arange(0, 1)
            j = np.arange(cj.min() - 3, cj.max() + 4) if cj.size else np.arange(0, 1)
            I, J = np.meshgrid(i, j, indexing="ij")
            pts = np.stack([xf + g.res * (-I.ravel()).astype(float), yf + g.res * (-J.ravel()).astype(float)], axis=1)
            mine = np.zeros(I.shape, dtype=bool)
            mine[np.searchsorted(i, ci), np.searchsorted(j, cj)] = True
            # distance of every point to the quad's edges
            dist = np.full(len(pts), np.inf)
            for k in range(4):
                a, b = quad[k - 1], quad[k]
                ab = b - a
                u = np.clip(((pts - a) @ ab) / (ab @ ab), 0.0, 1.0)
                dist = np.minimum(dist, np.linalg.norm(pts - (a + u[:, None] * ab), axis=1))
            far = dist > 1e-6
            theirs = Path(quad).contains_points(pts)
            assert np.array_equal(theirs[far], mine.ravel()[far]), (name, r, t)
            n += int(far.sum())
    print("%d cell centres" % n)
    assert n > 2000


def test_the_two_hand_cases(oracle):
    """The flank post: 0.5 m square centred 1.2 m beside the ego centre overlaps the 2.16 m wide body by 0.13 m, yet c = -1.4536 on both
    circles.  Two 4.79 x 2.16 cars side by side 2.5 m apart: 0.34 m of air between them, yet c = +0.060."""
    O = oracle
    p = O.default_params(40)
    one = _one_circle_params(p)

    def c_of(pose, dim, state):
        vf, vr = _circle_values(O, one, np.array(pose), np.array(dim), np.array(state))
        return math.log(vf / p.q1_front) / p.q2_front, math.log(vr / p.q1_rear) / p.q2_rear
    ego = [0.0, 0.0, 5.0, 0.0]
    c = clearance(0.0, 0.0, 0.0, LENGTH / 2, WIDTH / 2, 0.0, 1.2, 0.0, 0.25, 0.25)
    assert abs(c - (-0.13)) <= 1e-12
    cf, cr = c_of([0.0, 1.2, 0.0, 0.0], [0.5, 0.5], ego)
    # (figures quoted to so many decimals: within one unit of the last one, whether they were rounded or cut)
    assert abs(cf - (-1.4536)) <= 1e-4 and abs(cr - (-1.4536)) <= 1e-4, (cf, cr)
    c = clearance(0.0, 0.0, 0.0, LENGTH / 2, WIDTH / 2, 0.0, 2.5, 0.0, LENGTH / 2, WIDTH / 2)
    assert abs(c - 0.34) <= 1e-12
    cf, cr = c_of([0.0, 2.5, 0.0, 0.0], [LENGTH, WIDTH], ego)
    assert abs(max(cf, cr) - 0.060) <= 1e-3, (cf, cr)


def test_the_six_candidate_table(six):
    """The table of DESIGN §4.8o from the oracle's solves: J, max c and the exact clearance of the six candidates; all six count as collisions
    for the surrogate while every plan passes the post with more than a metre to spare.  And the constants of
    tests/cpp/candidates_footprint.cpp: the cheapest plan by total, and the cheapest among those at least 1.11 m clear."""
    for b, (J, c, clr) in enumerate(SIX_TABLE):
        print("candidate %d: J %.4f total %.4f max c %+.4f clearance %.4f" % (b, six["J"][b], six["total"][b], six["rows"][b, MAX_C], six["fp"][b, CLEARANCE]))
        assert abs(six["J"][b] - J) <= 0.006 and abs(six["rows"][b, MAX_C] - c) <= 0.0006 and abs(six["fp"][b, CLEARANCE] - clr) <= 0.0006
    assert np.all(six["rows"][:, COLLISION] == 1.0) and np.all(six["fp"][:, HIT_STEPS] == 0) and np.all(six["fp"][:, CLEARANCE] > 1.0)
    clr, total = six["fp"][:, CLEARANCE], six["total"]
    assert np.all(np.diff(clr) > 0.01) and clr[2] + 0.005 < SIX_MIN_CLEARANCE_BETWEEN < clr[3] - 0.005
    low, left = int(np.argmin(total)), 3 + int(np.argmin(total[3:]))
    order = np.sort(total)
    assert order[1] - order[0] > 1e-3 and np.sort(total[3:])[1] - total[left] > 1e-3  # the picks are decided
    assert (low, left) == (SIX_PICK_LOW, SIX_PICK_BETWEEN), (low, left)


SIX_PICK_LOW, SIX_PICK_BETWEEN = 2, 3  # (kPickLow, kPickBetween of the program)


@pytest.mark.parametrize("name", GPU_SCENES)
def test_conditions(scenes, name):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the restatement's numbers alone."""
    s = scenes[name]
    w = s[False]
    e = w["entry"]
    fin = e[np.isfinite(e)]
    if fin.size:
        assert np.min(np.abs(fin)) > MARGIN, np.min(np.abs(fin))
        for r in range(s["R"]):
            v = np.sort(e[r][np.isfinite(e[r])])
            assert v.size < 2 or v[1] - v[0] > MARGIN, (r, v[:2])
    if s["umap"] is not None:
        assert w["edge"] > EDGE, w["edge"]
        layers = s["umap"]["layers"] if isinstance(s["umap"]["layers"], list) else [s["umap"]["layers"]]
        for layer in layers:
            known = layer[np.isfinite(layer)]
            assert np.min(np.abs(known.astype(np.float64) - s["threshold"])) > MARGIN
    print("scene %s: R %d N %d M %d; hit steps %s; clearance %s; map hit steps %s unknown %s cells %s; edge %.3g" % (
        name, s["R"], s["N"], s["M"], w["fp"][:, HIT_STEPS].tolist(), np.round(w["fp"][:, CLEARANCE], 3).tolist(),
        w["fp"][:, MAP_HIT_STEPS].tolist(), w["fp"][:, MAP_UNKNOWN_STEPS].tolist(), w["fp"][:, MAP_CELLS].tolist(), w["edge"]))


def test_the_scenes_exercise_what_they_are_for(scenes):
    t = scenes["T50"][False]["fp"]
    assert (t[:, HIT_STEPS] > 0).any() and (t[:, MAP_UNKNOWN_STEPS] > 0).all() and (t[:, MAP_HIT_STEPS] > 0).any()
    assert scenes["T50"][False]["fp"][:, MAP_CELLS].min() > 64 * 50  # many wavefront passes per step
    small = scenes["P"][False]["cells"]
    assert max(ci.size for ci, _ in small.values()) < 64  # a bounding box under 64 cells
    assert not np.array_equal(scenes["T50"][False]["fp"][:, MAP_HIT_STEPS], scenes["T50"][True]["fp"][:, MAP_HIT_STEPS])  # UNKNOWN_HITS matters
    e = scenes["E"][False]
    assert np.all(e["fp"][:, CLEARANCE] == np.inf) and np.all(e["fp"][:, CLEARANCE_ENTRY] == -1) and np.all(e["fp"][:, MAP_OCC] == -np.inf)


# ---- CPU: plan_footprint, the index range, the layout -----------------------------------------------------------------------------
def _build(tmp_path, src, *include):
    exe = str(tmp_path / os.path.splitext(src)[0])
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall"] + ["-I" + i for i in include] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", src)],
                   check=True)
    return exe


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_footprint.cpp: plan_footprint laid out without an arena against host_arena_bytes at every shape
    include/cilqr.h says fits; host_arena_bytes is still what tests/golden/host_arena_cap.json recorded; one layout in full."""
    exe = _build(tmp_path, "host_plan_footprint.cpp", os.path.join(ROOT, "include"), os.path.join(PKG, "csrc"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "8 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20
    R, N, M, span = 6, 5, 3, 2 * 3 * 5
    r = subprocess.run([exe, "layout", str(R), str(N), str(M), str(span), "1"], capture_output=True, text=True, check=True)
    entries = [[int(v) for v in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("entry ")]
    sizes = [R * 4 * (N + 1) * 8, span * 32, span * 16, R * 8, R * 12 * 8, R * N * 8, R * N * 4, R * 8]  # X, pose, dim, base | fp, clearances, occ, total
    at = 0
    for (off, nbytes, src, dst), want in zip(entries, sizes):
        assert (off, nbytes) == (at, want)
        at = (off + nbytes + 15) // 16 * 16
    assert len(entries) == 8 and [e[2] for e in entries] == [1, 1, 1, 1, 0, 0, 0, 0] and [e[3] for e in entries] == [0, 0, 0, 0, 1, 1, 1, 1]
    tail = dict(zip(r.stdout.splitlines()[-1].split()[1::2], (int(v) for v in r.stdout.splitlines()[-1].split()[2::2])))
    assert tail["ok"] == 1 and tail["in_end"] == tail["out_begin"] == entries[4][0] and tail["end"] == at


def test_the_index_range_on_the_cpu(tmp_path, oracle):
    """csrc/cilqr_footprint_range.h through tests/cpp/footprint_range_dump.cpp, before it ever runs on a device: states at +-1e6,
    +-1e300, +-inf and NaN, resolutions 0.01 ... 10.  Every returned range fits int32 (in fact +-2^30), is empty and flagged for a
    state that is not finite or out of range, and otherwise contains the restatement's covered cells."""
    exe = _build(tmp_path, "footprint_range_dump.cpp", os.path.join(PKG, "csrc"))
    hl, hw = 0.5 * LENGTH + 0.137, 0.5 * WIDTH + 0.137
    inf, nan = math.inf, math.nan
    cases = []
    for res in (0.01, 0.1, 1.0, 10.0):
        for pose in ((0.0, 0.0, 0.0), (0.3, -0.2, 0.05), (5.0, 7.0, -2.0)):
            for th in HEADINGS:
                for xy in ((1.0, 2.0), (-3.3, 0.4), (1e6, 0.0), (-1e6, 3.0), (0.0, 1e6), (2.0, -1e6), (1e300, 0.0), (0.0, -1e300), (inf, 0.0),
                           (0.0, -inf), (nan, 0.0), (0.0, nan), (1e10, 1e10)):
                    cases.append((xy[0], xy[1], th, hl, hw) + pose + (7.45, 4.95, res))
            cases.append((1.0, 2.0, nan, hl, hw) + pose + (7.45, 4.95, res))
            cases.append((1.0, 2.0, inf, hl, hw) + pose + (7.45, 4.95, res))
    text = "\n".join(" ".join(repr(float(v)) for v in c) for c in cases) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60)
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    n_ok = n_flagged = 0
    for c, line in zip(cases, lines):
        v = line.split()
        ok, ilo, ihi, jlo, jhi = (int(x) for x in v[:5])
        assert all(abs(k) <= 2 ** 30 for k in (ilo, ihi, jlo, jhi)), (c, line)
        x, y, th, _, _, px, py, pth, xf, yf, res = c
        finite = all(math.isfinite(q) for q in (x, y, th))
        if not finite:
            assert ok == 0, (c, line)
        if not ok:
            assert (ilo, ihi, jlo, jhi) == (0, -1, 0, -1), (c, line)
            n_flagged += 1
            assert not finite or max(abs(x), abs(y)) / res > 2 ** 29, (c, line)  # flagged only where the indices really are large
            continue
        n_ok += 1
        quad = corners_map(x, y, th, hl, hw, (px, py, pth))
        assert np.allclose(np.array(quad).ravel(), [float(q) for q in v[5:]], rtol=0, atol=1e-9 * max(1.0, abs(x), abs(y)))
        g = type("G", (), dict(res=res, rows=1, cols=1, pos_x=xf, pos_y=yf, len_x=res, len_y=res))  # first_cell(g) = (xf, yf)
        if max(abs(x), abs(y)) < 1e7:  # (beyond, the crossing test's window is too large to enumerate here)
            ci, cj, _ = covered_cells(g, quad)
            if ci.size:
                assert ilo <= ci.min() and ci.max() <= ihi and jlo <= cj.min() and cj.max() <= jhi, (c, line)
            assert (ihi - ilo + 1) <= math.ceil(2 * math.hypot(hl, hw) / res) + 5 and (jhi - jlo + 1) <= math.ceil(2 * math.hypot(hl, hw) / res) + 5
    print("%d ranges, %d flagged" % (n_ok, n_flagged))
    assert n_ok > 250 and n_flagged > 100


def test_the_layout_with_the_footprint_flag(tmp_path):
    """tests/cpp/candidate_layout_footprint_dump.cpp beside tests/cpp/candidate_layout_dump.cpp: with the flag off every existing
    array's offset and `end` equal the existing dump's; with it on the stage's three arrays are reserved behind everything else."""
    inc = os.path.join(PKG, "host"), os.path.join(ROOT, "include")
    old, new = _build(tmp_path, "candidate_layout_dump.cpp", *inc), _build(tmp_path, "candidate_layout_footprint_dump.cpp", *inc)

    def names(exe):
        d = dict(line.split(":") for line in subprocess.run([exe, "names"], check=True, capture_output=True, text=True).stdout.splitlines())
        return d["flags"].split(), d["predicates"].split(), d["arrays"].split()
    (f0, p0, a0), (f1, p1, a1) = names(old), names(new)
    assert f1 == f0 + ["footprint"] and p1 == p0 + ["footprint_check"]
    assert a1 == a0 and a1[-4:] == ["fprow", "fpstep", "fptotal", "end"]  # (the existing dump reads the same header: at the END)
    rng = np.random.default_rng(5)
    rec = np.zeros((400, 8), dtype=np.uint64)
    rec[:, 0] = rng.integers(0, 2 ** len(f0), 400)
    rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = rng.integers(1, 7, 400), rng.integers(1, 51, 400), rng.integers(0, 5, 400), rng.integers(0, 300, 400)
    rec[:, 5], rec[:, 6], rec[:, 7] = rng.integers(0, 3, 400), rng.integers(0, 3, 400), rng.integers(0, 28, 400)

    def run(exe, records):
        out = subprocess.run([exe], input=records.tobytes(), capture_output=True, check=True).stdout
        return np.frombuffer(out, dtype=np.uint64).reshape(len(records), -1)
    off_old, off_new = run(old, rec), run(new, rec)
    k = {n: 1 + i for i, n in enumerate(a1)}
    assert np.array_equal(off_old[:, 1:], off_new[:, 1:])  # flag off: every offset and `end`
    assert np.array_equal(off_new[:, k["fprow"]], off_new[:, k["end"]]) and np.array_equal(off_old[:, 0], off_new[:, 0] & np.uint64(2 ** len(p0) - 1))
    on = rec.copy()
    on[:, 0] |= np.uint64(1 << len(f0))
    got = run(new, on)
    B, N = rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64)
    even = lambda v: (v + 1) // 2 * 2  # noqa: E731
    for n in a0[:-4]:
        assert np.array_equal(got[:, k[n]], off_old[:, k[n]]), n  # flag on: nothing before the new arrays moves
    assert np.array_equal(got[:, k["fprow"]].astype(np.int64), off_old[:, k["end"]].astype(np.int64))
    assert np.array_equal(got[:, k["fpstep"]].astype(np.int64) - got[:, k["fprow"]].astype(np.int64), even(B * 12))
    assert np.array_equal(got[:, k["fptotal"]].astype(np.int64) - got[:, k["fpstep"]].astype(np.int64), even(B * N))
    assert np.array_equal(got[:, k["end"]].astype(np.int64) - got[:, k["fptotal"]].astype(np.int64), even(B))
    bit = {n: i for i, n in enumerate(p1)}
    assert np.all((got[:, 0] >> np.uint64(bit["footprint_check"])) & np.uint64(1)) and np.all((got[:, 0] >> np.uint64(bit["in_block"])) & np.uint64(1))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(50), max_batch=8, max_horizon=50, max_obstacles=70, device=0)
    yield s
    s.close()


class _Map:
    """The scene's map on the solver: the host form for a shared layer, the device form (torch buffers kept here) for per-solve ones."""

    def __init__(self, cilqr, solver, umap, sel=None):
        self.solver, self.on = solver, umap is not None
        if not self.on:
            return
        g = cilqr.map_geom(*umap["geom"])
        if isinstance(umap["layers"], list):
            import torch
            idx = range(len(umap["layers"])) if sel is None else sel
            flat = np.stack([np.asfortranarray(umap["layers"][b]).flatten(order="F") for b in idx])
            self.layers = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0")
            self.poses = torch.from_numpy(np.ascontiguousarray([umap["poses"][b] for b in idx], dtype=np.float64)).to("cuda:0")
            torch.cuda.synchronize()
            solver.set_uncertainty_map_device(self.layers.data_ptr(), g, (0.0, 0.0, 0.0), (3, 3), layer_stride=flat.shape[1], poses_ptr=self.poses.data_ptr())
        else:
            solver.set_uncertainty_map(umap["layers"], g, umap["poses"], (3, 3))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.on:
            self.solver.clear_uncertainty_map()


def _host(solver, s, rows=slice(None), solves=slice(None), pose=None, dim=None, **kw):
    a = dict(S=s["S"], margin=s["margin"], min_clearance=0.0, occ_threshold=s["threshold"], base=s["base"][rows])
    a.update(kw)
    pose, dim = (s["pose"], s["dim"]) if pose is None else (pose, dim)
    return solver.footprint_check(s["N"], s["X"][rows], None if pose is None else (pose[solves] if pose.ndim == 3 else pose),
                                  None if dim is None else (dim[solves] if dim.ndim == 3 else dim), **a)


def _device(solver, s, flags=0, min_clearance=0.0, steps=True, with_total=True):
    """The device form on torch buffers, dense obstacles."""
    import torch
    B, N, M, S, R = s["B"], s["N"], s["M"], s["S"], s["R"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    X, base = up(s["X"]), up(s["base"])
    pose, dim = (up(s["pose"]), up(s["dim"])) if M else (None, None)
    z = lambda *shape, dt=torch.float64: torch.full(shape, 7.0, dtype=dt, device=dev)  # noqa: E731
    fp, sc, so, total = z(R, 12), z(R, N), z(R, N, dt=torch.float32), z(R)
    torch.cuda.synchronize(dev)
    solver.footprint_check_device(stream, B, N, M, S, X.data_ptr(), pose.data_ptr() if M else 0, dim.data_ptr() if M else 0, (M * N, N, 1, 0),
                                  fp.data_ptr(), margin=s["margin"], min_clearance=min_clearance, occ_threshold=s["threshold"], flags=flags,
                                  base=base.data_ptr() if with_total else 0, step_clearance=sc.data_ptr() if steps else 0,
                                  step_occ=so.data_ptr() if steps else 0, total=total.data_ptr() if with_total else 0)
    torch.cuda.synchronize(dev)
    return dict(fp=fp.cpu().numpy(), step_clearance=sc.cpu().numpy(), step_occ=so.cpu().numpy(), total=total.cpu().numpy())


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ("fp", "step_clearance", "step_occ", "total"))


def _check_against(got, want, what):
    fp, w = got["fp"], want["fp"]
    print("%s: clearance %s (want %s), hit steps %s, map occ %s, map hit steps %s, unknown %s, cells %s" % (
        what, fp[:, CLEARANCE].tolist(), w[:, CLEARANCE].tolist(), fp[:, HIT_STEPS].tolist(), fp[:, MAP_OCC].tolist(), fp[:, MAP_HIT_STEPS].tolist(),
        fp[:, MAP_UNKNOWN_STEPS].tolist(), fp[:, MAP_CELLS].tolist()))
    inf = np.isinf(w[:, CLEARANCE])
    assert np.array_equal(fp[inf, CLEARANCE], w[inf, CLEARANCE]) and np.all(np.abs(fp[~inf, CLEARANCE] - w[~inf, CLEARANCE]) <= ABS_TOL), what
    for f in range(1, 12):
        assert np.array_equal(fp[:, f], w[:, f]), (what, FIELDS[f], fp[:, f].tolist(), w[:, f].tolist())
    if got["step_clearance"] is not None:
        a, b = got["step_clearance"], want["step_clearance"]
        inf = np.isinf(b)
        assert np.array_equal(a[inf], b[inf]) and np.all(np.abs(a[~inf] - b[~inf]) <= ABS_TOL), what
        assert np.array_equal(got["step_occ"].view(np.uint32), want["step_occ"].view(np.uint32)), what
    if want["total"] is not None and got["total"] is not None:
        assert np.array_equal(_bits(got["total"]), _bits(want["total"])), (what, got["total"], want["total"])


@gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_fields_against_the_restatement(cilqr, solver, scenes, name):
    """Both settings of UNKNOWN_HITS; the host form and the device form agree bit for bit; SKIP_MAP is the call without a map."""
    s = scenes[name]
    with _Map(cilqr, solver, s["umap"]):
        for flag in (False, True):
            host = _host(solver, s, unknown_hits=flag)
            _check_against(host, s[flag], "%s, unknown_hits %s" % (name, flag))
            assert _same_bits(host, _device(solver, s, flags=UNKNOWN_HITS if flag else 0)), (name, flag)
        skipped = _host(solver, s, skip_map=True)
    no_map = restate(s["p"], s["N"], s["X"], s["S"], s["pose"], s["dim"], s["margin"], 0.0, s["threshold"], base=s["base"])
    _check_against(skipped, no_map, name + ", SKIP_MAP")
    assert _same_bits(skipped, _host(solver, s))  # ... and with no map set


@gpu
def test_shared_and_static_obstacles_equal_their_dense_expansion(cilqr, solver, scenes):
    s = scenes["T50"]
    B, M, N = s["B"], s["M"], s["N"]
    moving = (s["pose"][0], s["dim"][0])                                                       # (M, 4N): (0, N, 1)
    static = (np.ascontiguousarray(s["pose"][0][:, :4]), np.ascontiguousarray(s["dim"][0][:, :2]))  # (M, 4): (0, 1, 0)
    with _Map(cilqr, solver, s["umap"]):
        for what, (pose, dim) in (("shared", moving), ("static", static)):
            dense = (np.ascontiguousarray(np.broadcast_to(np.tile(pose, (1, 4 * N // pose.shape[1])), (B, M, 4 * N))),
                     np.ascontiguousarray(np.broadcast_to(np.tile(dim, (1, 2 * N // dim.shape[1])), (B, M, 2 * N))))
            a, b = _host(solver, s, pose=pose, dim=dim), _host(solver, s, pose=dense[0], dim=dense[1])
            assert _same_bits(a, b), what
            want = restate(s["p"], N, s["X"], s["S"], dense[0], dense[1], s["margin"], 0.0, s["threshold"], umap=s["umap"], base=s["base"])
            _check_against(a, want, what)


@gpu
def test_a_rows_bits_do_not_depend_on_its_place(cilqr, solver, scenes):
    """Rows of solve 1 of T50 alone (B = 1, S = 3) against the same rows inside the batch; a row of T5 moved from solve 2 to solve 0."""
    s = scenes["T50"]
    S = s["S"]
    with _Map(cilqr, solver, s["umap"]):
        full = _host(solver, s)
        alone = _host(solver, s, rows=slice(S, 2 * S), solves=slice(1, 2))
    for k in ("fp", "step_clearance", "step_occ", "total"):
        assert np.array_equal(full[k][S:2 * S].view(np.uint8), alone[k].view(np.uint8)), k
    p = scenes["P"]  # per-solve layers and poses: solve 2 alone, with its own layer and pose
    with _Map(cilqr, solver, p["umap"]):
        full = _host(solver, p)
    with _Map(cilqr, solver, p["umap"], sel=[2]):
        alone = _host(solver, p, rows=slice(2, 3), solves=slice(2, 3))
    for k in ("fp", "step_clearance", "step_occ", "total"):
        assert np.array_equal(full[k][2:3].view(np.uint8), alone[k].view(np.uint8)), k


@gpu
def test_every_optional_output_left_out(cilqr, solver, scenes):
    s = scenes["T5"]
    with _Map(cilqr, solver, s["umap"]):
        full = _device(solver, s)
        lean = _device(solver, s, steps=False, with_total=False)
        host = _host(solver, s, steps=False, base=None)
    assert np.array_equal(full["fp"].view(np.uint8), lean["fp"].view(np.uint8)) and np.array_equal(full["fp"].view(np.uint8), host["fp"].view(np.uint8))
    assert np.all(lean["step_clearance"] == 7.0) and np.all(lean["step_occ"] == 7.0) and np.all(lean["total"] == 7.0)  # untouched
    assert host["step_clearance"] is None and host["total"] is None


@gpu
def test_states_and_entries_that_are_not_finite(cilqr, solver, scenes):
    """A NaN x at one step, an infinite theta at another: obstacle hit, map hit and unknown at those steps, -HUGE_VAL in
    step_clearance, no cell covered, nothing else changed.  A NaN obstacle pose and a negative dimension: hits with no clearance value."""
    s = scenes["T5"]
    N = s["N"]
    X = s["X"].copy()
    X[0, 4 * 1] = np.nan
    X[1, 4 * 3 + 3] = np.inf
    pose, dim = s["pose"].copy(), s["dim"].copy()
    pose[2, 1, 4 * 2 + 1] = np.nan
    dim[2, 0, 2 * 4] = -1.0
    want = restate(s["p"], N, X, s["S"], pose, dim, s["margin"], 0.0, s["threshold"], umap=s["umap"], base=s["base"])
    assert want["step_clearance"][0, 1] == -np.inf and want["fp"][0, HIT_STEPS] >= 1 and want["fp"][2, HIT_STEPS] >= 2 and np.isnan(want["total"][:3]).all()
    s2 = dict(s, X=X, pose=pose, dim=dim)
    with _Map(cilqr, solver, s["umap"]):
        _check_against(_host(solver, s2), want, "not finite")
    no_obs = restate(s["p"], N, X, s["S"], None, None, s["margin"], 0.0, s["threshold"], base=s["base"])
    assert no_obs["fp"][0, HIT_STEPS] == 1 and no_obs["fp"][0, FIRST_HIT] == 1
    _check_against(solver.footprint_check(N, X, margin=s["margin"], occ_threshold=s["threshold"], base=s["base"]), no_obs, "not finite, M = 0, no map")


@gpu
def test_map_edge_cases(cilqr, solver, oracle):
    """A footprint half off the map, wholly off it, an ego 1e6 m away, a NaN cell under the body, and one cell at 100 under the flank
    where the 3 x 3 probes of the map cost read nothing."""
    O = oracle
    N = 5
    p = O.default_params(N)
    g = O.map_geom(*GEOM_BIG)
    layer = np.zeros((g.rows, g.cols), dtype=np.float32)
    xf, yf = first_cell(g)
    i_flank, j_flank = int(round((xf - 5.03) / g.res)), int(round((yf - 0.93) / g.res))  # body frame (0.03, 0.93) of a state at (5, 0)
    layer[i_flank, j_flank] = 100.0
    layer[int(round((xf - 9.03) / g.res)), int(round((yf + 0.52) / g.res))] = np.nan
    X = np.zeros((5, N + 1, 4))
    X[..., 2] = 5.0
    X[0, :, 0], X[0, :, 1] = 5.0, 0.0                      # over the cell at 100
    X[1, :, 0], X[1, :, 1] = 9.0, 0.011                    # over the NaN cell
    X[2, :, 0], X[2, :, 1], X[2, :, 3] = 14.93, 0.013, 0.3  # half off the map
    X[3, :, 0], X[3, :, 1] = 40.0, 0.0                     # wholly off it
    X[4, :, 0], X[4, :, 1], X[4, :, 3] = 1.0e6, -1.0e6, 1.0  # far away
    X = X.reshape(5, -1)
    umap = dict(g=g, geom=GEOM_BIG, layers=layer, poses=(0.0, 0.0, 0.0))
    base = np.ones(5)
    sv = cilqr.Solver(cilqr.default_params(N), max_batch=5, max_horizon=N, max_obstacles=0, device=0)
    try:
        with _Map(cilqr, sv, umap):
            for flag in (False, True):
                want = restate(p, N, X, 1, None, None, 0.0, 0.0, THRESHOLD, flag, False, umap, base)
                assert want["edge"] > EDGE
                got = sv.footprint_check(N, X, occ_threshold=THRESHOLD, base=base, unknown_hits=flag)
                _check_against(got, want, "edge cases, unknown_hits %s" % flag)
            w = want["fp"]
            assert w[0, MAP_OCC] == 100.0 and w[0, MAP_OCC_CELL] == i_flank + j_flank * g.rows and w[0, MAP_HIT_STEPS] == N and w[0, MAP_HIT_CELLS] == 1
            assert w[1, MAP_UNKNOWN_STEPS] == N and w[2, MAP_UNKNOWN_STEPS] == N and w[3, MAP_OCC] == -np.inf and w[3, MAP_CELLS] > 0
            assert w[4, MAP_UNKNOWN_STEPS] == N and w[4, MAP_CELLS] > 0 and w[4, MAP_OCC_STEP] == -1
            # the surrogate sees nothing of the cell at 100: the map cost at that state is the cost on an all-zero map
            cost = sv.debug_uncertainty_cost(X[0, :4])[0]
            sv.set_uncertainty_map(np.zeros_like(layer), cilqr.map_geom(*GEOM_BIG), (0.0, 0.0, 0.0), (3, 3))
            assert np.array_equal(_bits(cost), _bits(sv.debug_uncertainty_cost(X[0, :4])[0]))
    finally:
        sv.close()


@gpu
def test_the_covered_cells_are_the_rasterisers(cilqr, solver, scenes):
    """Secondary: the cells cilqr_rasterize_polygons marks for the restatement's vertices are the restatement's covered in-map cells."""
    s = scenes["T5"]
    g = cilqr.map_geom(*GEOM_BIG)
    st = s["X"].reshape(s["R"], s["N"] + 1, 4)
    hl, hw = 0.5 * LENGTH + s["margin"], 0.5 * WIDTH + s["margin"]
    for (r, t), (ci, cj) in list(s[False]["cells"].items())[::4]:
        quad = corners_map(st[r, t, 0], st[r, t, 1], st[r, t, 3], hl, hw, POSE_SHARED)
        marked = solver.rasterize_polygons(g, [quad]) == 100.0
        inm = (ci >= 0) & (ci < g.rows) & (cj >= 0) & (cj < g.cols)
        mine = np.zeros_like(marked)
        mine[ci[inm], cj[inm]] = True
        assert np.array_equal(marked, mine), (r, t)


@gpu
def test_total_thresholds_and_the_pick(cilqr, solver, scenes):
    """min_clearance 1e-6 either side of each row's clearance; occ_threshold either side of a row's largest occupancy; a NaN base
    stays NaN; the total feeds cilqr_argmin_device."""
    from test_risk_map import _device_pick
    from test_rollout_risk import _pick
    s = scenes["T5"]
    w = s[False]
    with _Map(cilqr, solver, s["umap"]):
        free = _host(solver, s, occ_threshold=math.inf, min_clearance=-math.inf)  # only obstacle hits reject
        assert np.array_equal(np.isnan(free["total"]), w["fp"][:, HIT_STEPS] > 0)
        for r in range(s["R"]):
            c = w["fp"][r, CLEARANCE]
            for mc, passes in ((c - 1e-6, True), (c + 1e-6, False)):
                got = _host(solver, s, occ_threshold=math.inf, min_clearance=mc)["total"][r]
                assert np.isnan(got) == (not passes or w["fp"][r, HIT_STEPS] > 0), (r, mc, got)
            o = float(w["fp"][r, MAP_OCC])
            for thr, passes in ((o + 1e-6, True), (o - 1e-6, False)):
                got = _host(solver, s, occ_threshold=thr, min_clearance=-math.inf)["total"][r]
                assert np.isnan(got) == (not passes or w["fp"][r, HIT_STEPS] > 0), (r, thr, got)
        base = s["base"].copy()
        base[0] = np.nan
        got = _host(solver, s, occ_threshold=math.inf, min_clearance=-math.inf, base=base)["total"]
        want = np.where(np.isnan(free["total"]), np.nan, base)
        assert np.isnan(got[0]) and np.array_equal(_bits(got), _bits(want))
        assert _device_pick(solver, got) == _pick(want)
        assert _device_pick(solver, np.full(3, np.nan)) == -1


@gpu
def test_limits(cilqr, scenes):
    """B*S above max_batch, M above max_obstacles: CILQR_ERR_ARG, and the handle stays usable.  A margin that makes the footprint wider
    than 1024 cells: CILQR_ERR_UNSUPPORTED, only where a map test would run."""
    s = scenes["T5"]
    sv = cilqr.Solver(cilqr.default_params(s["N"]), max_batch=3, max_horizon=s["N"], max_obstacles=3, device=0)
    try:
        X4 = np.concatenate([s["X"], s["X"][:1]])
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*B\\*S" % ERR_ARG):
            sv.footprint_check(s["N"], X4)
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d" % ERR_ARG):
            sv.footprint_check(s["N"], s["X"], np.zeros((4, 4)), np.ones((4, 2)))
        with _Map(cilqr, sv, s["umap"]):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*1024 cells" % ERR_UNSUPPORTED):
                sv.footprint_check(s["N"], s["X"], margin=40.0)
            wide = sv.footprint_check(s["N"], s["X"], margin=40.0, skip_map=True)
            assert np.all(wide["fp"][:, MAP_CELLS] == 0)
            _check_against(_host(sv, s), s[False], "after the refused calls")
    finally:
        sv.close()


@gpu
def test_pipeline_on_device_buffers(cilqr, six):
    """Solve the six-candidate scene -> footprint check (base = J) -> argmin, all on device buffers of one stream: the pick is the
    candidate of least J among those the restatement lets through at min_clearance between candidates 2 and 3."""
    import torch
    N, B = six["N"], six["B"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    x0, U, poly, fl = up(six["x0"]), up(six["U0"]), up(six["poly"]), up(six["fl"])
    pose, dim = up(np.array([SIX_POST[0], SIX_POST[1], 0.0, 0.0])), up(np.array(SIX_POST[2:]))
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    X, J, it, status, fp, total, pair = z(B, 4 * (N + 1)), z(B), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, 12), z(B), z(2)
    sv = cilqr.Solver(cilqr.default_params(N), max_batch=B, max_horizon=N, max_obstacles=1, device=0)
    try:
        torch.cuda.synchronize(dev)
        obs = cilqr.Obstacles(pose.data_ptr(), dim.data_ptr(), None, 0, 1, 0, 0)
        rc = cilqr.lib().cilqr_solve_batch_obstacles_device(sv._h, C.c_void_p(stream), B, N, 1, C.c_void_p(x0.data_ptr()), C.c_void_p(U.data_ptr()),
                                                            C.c_void_p(poly.data_ptr()), C.c_void_p(fl.data_ptr()), C.byref(obs), C.c_void_p(X.data_ptr()),
                                                            C.c_void_p(J.data_ptr()), C.c_void_p(it.data_ptr()), C.c_void_p(status.data_ptr()), C.c_uint32(0))
        assert rc == 0, cilqr.lib().cilqr_last_error()
        sv.footprint_check_device(stream, B, N, 1, 1, X.data_ptr(), pose.data_ptr(), dim.data_ptr(), (0, 1, 0, 0), fp.data_ptr(),
                                  min_clearance=SIX_MIN_CLEARANCE_BETWEEN, base=J.data_ptr(), total=total.data_ptr())
        sv.argmin_device(stream, B, total.data_ptr(), pair.data_ptr())
        torch.cuda.synchronize(dev)
    finally:
        sv.close()
    got, Jd = fp.cpu().numpy(), J.cpu().numpy()
    print("J %s clearance %s total %s pair %s" % (Jd.tolist(), got[:, CLEARANCE].tolist(), total.cpu().numpy().tolist(), pair.cpu().numpy().tolist()))
    assert np.all(np.abs(got[:, CLEARANCE] - six["fp"][:, CLEARANCE]) <= 1e-5)  # (the device's own solves: within the solve's 1e-6 on U)
    assert np.array_equal(np.isnan(total.cpu().numpy()), six["fp"][:, CLEARANCE] < SIX_MIN_CLEARANCE_BETWEEN)
    assert int(pair.cpu().numpy()[1]) == 3 + int(np.argmin(six["J"][3:]))


@gpu
def test_cpp_facade_footprint_checked_candidates(six, tmp_path):
    """tests/cpp/candidates_footprint.cpp on the six-candidate scene; its constants are asserted from the oracle's solves in
    test_the_six_candidate_table."""
    exe = str(tmp_path / "candidates_footprint")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_footprint.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "footprint pick ok" in r.stdout
    clr = [float(v) for v in re.search(r"clearances:(.*)", r.stdout).group(1).split()]
    assert len(clr) == 6 and np.all(np.abs(np.array(clr) - six["fp"][:, CLEARANCE]) <= 1e-5)
