"""Obstacles from the map (cilqr_map_obstacles*, include/cilqr.h): the connected components of the linked cells of L distance
fields per call, their integer moments, and the principal-axis box of each as a row of the obstacle channel.

Expected values never come from the HIP path.  `flood_labels` forms the labels by flood fill (and is checked against
scipy.ndimage.label on every test layer); `components_restate` and `rows_restate` are the header's formulas in numpy doubles, one
operation at a time.  The device is compared with them integer for integer; boxes, poses, dims and FILL within 1e-9 (metres, radians;
relative for FILL): the only difference is the device's atan2 and sincos against libm on exact integer inputs.  The solves carry the
suite's bar: max|dU| <= 1e-9, equal iterations and exits.

Shapes: 1x1, 1x7, 7x1; 65x3, 3x65; 64x64; 130x129 (past two seams of the 64 x 16 tiles in either direction); 150x100 (the node's).
Layers per shape (`seed_layers`): 2 % and 50 % random seeds; none; every cell; one corner cell; a checkerboard (one component under
8-connectivity, every seed alone under FOUR: more than K, the truncation path); a serpentine of single-cell width through the whole
layer; a comb whose teeth join only at the far edge; two blobs two cells apart (two components at gap2 = 0, one at gap2 = 1).

The scene that shows what the call is for (`test_the_box_does_what_it_is_for`): the blob scene of tests/test_tighten_map.py — six
candidates side by side, the blob at (6, -1.4), seeds above 50, no ellipse.  From the oracle and the restatements alone:
  the blob is one component of 266 seeds; its box is 1.8 m x 1.8 m at (5.978, -1.403), yaw 1.621 (FILL 0.821);
  exact clearance of the six plans to the ORIGINAL map     map only    [-0.6525, -0.5389, -0.4242, -0.3279, -0.2278, -0.1332]
                                                            map + box   [ 0.0777, -0.0009,  0.0673,  0.2623,  0.4894,  0.6655]
  CILQR_FP_CLEARANCE                                        map only    +inf (M = 0: nothing to measure against)
  the same rectangle test of the map-only plans against the box       [-0.7844, -0.6320, -0.4815, -0.4132, -0.3407, -0.2730]
  CILQR_FP_CLEARANCE                                        map + box   [-0.0990, -0.1027, -0.0034,  0.2034,  0.4322,  0.5890]
  iterations [15, 16, 7, 8, 9, 18] -> [7, 7, 7, 7, 7, 13]
With the map alone all six plans cut through the occupied cells.  With the box every plan moves away, by 0.49 m to 0.80 m; the plan
deepest in contact (0.65 m inside) ends 0.08 m clear, the second still touches (-0.0009 m).  The barrier is the ellipse of
Obstacle.cpp, a soft term: three plans still overlap the BOX by up to 0.10 m, which CILQR_FP_CLEARANCE now reports and can reject.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_footprint import restate as footprint_restate
from test_map_distance import rect_clearance, seeds_of
from test_polygon_raster import boxes_to_polygons_restated, inside_mask
from test_tighten_map import ROUND_BLOB, _round_params, _round_scene

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_INTERNAL = -1, -4, -6
NONE = 2 ** 31 - 1
FOUR = 1
FAR = 1.0e6
FIELDS = ("LABEL", "CELLS", "LINKED", "I_MIN", "I_MAX", "J_MIN", "J_MAX", "SUM_I", "SUM_J", "SUM_II", "SUM_IJ", "SUM_JJ", "FILL")
(LABEL, CELLS, LINKED, I_MIN, I_MAX, J_MIN, J_MAX, SUM_I, SUM_J, SUM_II, SUM_IJ, SUM_JJ, FILL) = range(13)
ENTRY_POINTS = ("cilqr_map_obstacles", "cilqr_map_obstacles_device")
SHAPES = [(1, 1), (1, 7), (7, 1), (65, 3), (3, 65), (64, 64), (130, 129), (150, 100)]
LAYER_NAMES = ("sparse", "dense", "none", "every", "corner", "checker", "serpentine", "comb", "two_blobs")
GAPS = (0, 1, 4)
THRESHOLD = 50.0
RES = 0.1
GEOM_POS = (1.5, -0.25)  # pos_x, pos_y of the test geometry
PAD = 0.05
MAX_SIZE = 1.234  # metres: no restated size lies within 1e-9 of it (asserted), so the filter's decision is not a matter of rounding
TOL = 1e-9
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- the layers ---------------------------------------------------------------------------------------------------------------------
def seed_layers(rows, cols):
    """The nine seed masks (rows, cols) of a shape, in the order of LAYER_NAMES."""
    rng = np.random.Generator(np.random.PCG64(7000 * rows + cols))
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    corner = np.zeros((rows, cols), dtype=bool)
    corner[rows - 1, 0] = True
    serpentine = (j % 2 == 0) | ((j % 4 == 1) & (i == rows - 1)) | ((j % 4 == 3) & (i == 0))
    comb = (j % 2 == 0) | (i == rows - 1)
    two = np.zeros((rows, cols), dtype=bool)
    if rows >= cols:  # two blobs along i, two free cells between them
        n, w = max(1, min(5, (rows - 2) // 2)), max(1, min(4, cols))
        two[0:n, 0:w] = True
        two[n + 2:2 * n + 2, 0:w] = True
    else:
        n, w = max(1, min(5, (cols - 2) // 2)), max(1, min(4, rows))
        two[0:w, 0:n] = True
        two[0:w, n + 2:2 * n + 2] = True
    return [rng.random((rows, cols)) < 0.02, rng.random((rows, cols)) < 0.5, np.zeros((rows, cols), dtype=bool),
            np.ones((rows, cols), dtype=bool), corner, (i + j) % 2 == 0, serpentine, comb, two]


def d2_of(seed):
    """The field cilqr_map_distance gives for the seeds (tests/test_map_distance.py pins that call against this transform)."""
    from scipy.ndimage import distance_transform_edt
    if not seed.any():
        return np.full(seed.shape, NONE, dtype=np.int32)
    return np.rint(distance_transform_edt(~seed) ** 2).astype(np.int32)


# ---- expected values: the definitions, restated -------------------------------------------------------------------------------------
def flood_labels(linked, four):
    """Flood fill over the linked cells, visited in ascending i + j*rows: the first cell of a component met is its lowest, and its index
    is the component's label.  (rows, cols) int32, -1 where not linked."""
    rows, cols = linked.shape
    R = rows + 2
    pad = np.zeros((cols + 2, R), dtype=bool)  # [j + 1][i + 1]: one free ring, so that no neighbour needs a bounds test
    pad[1:-1, 1:-1] = linked.T
    flat = pad.reshape(-1).tolist()
    steps = [1, -1, R, -R] + ([] if four else [R + 1, R - 1, -R + 1, -R - 1])
    lab = [-1] * len(flat)
    for s in np.flatnonzero(pad.reshape(-1)).tolist():  # ascending (j, i)
        if lab[s] >= 0:
            continue
        label = (s % R - 1) + (s // R - 1) * rows
        lab[s] = label
        stack = [s]
        while stack:
            c = stack.pop()
            for o in steps:
                n = c + o
                if flat[n] and lab[n] < 0:
                    lab[n] = label
                    stack.append(n)
    return np.array(lab, dtype=np.int32).reshape(cols + 2, R)[1:-1, 1:-1].T.copy()


def components_restate(d2, lab, res, x_first, y_first, pose, pad):
    """Every component of a labelled layer, in ascending label order: comp (n, 13) and boxes (n, 5) by the header's formulas, and the
    axes and extents in index coordinates (with the seeds and their component) for the containment test."""
    linked, seed = lab >= 0, d2 == 0
    roots = np.unique(lab[linked])
    n = roots.size
    comp, boxes = np.zeros((n, 13)), np.zeros((n, 5))
    if n == 0:
        return comp, boxes, None
    n_linked = np.bincount(np.searchsorted(roots, lab[linked]), minlength=n)
    si, sj = np.nonzero(seed)
    ks = np.searchsorted(roots, lab[seed])  # (boolean indexing and nonzero visit the cells in the same order)
    si, sj = si.astype(np.int64), sj.astype(np.int64)

    def total(v):
        out = np.zeros(n, dtype=np.int64)
        np.add.at(out, ks, v)
        return out

    def extreme(v, fn, start):
        out = np.full(n, start, dtype=v.dtype)
        fn.at(out, ks, v)
        return out
    c, Si, Sj, Sii, Sij, Sjj = total(np.ones_like(si)), total(si), total(sj), total(si * si), total(si * sj), total(sj * sj)
    assert (c >= 1).all()  # every component holds a seed
    a, b, d = c * Sii - Si * Si, c * Sij - Si * Sj, c * Sjj - Sj * Sj
    phi = 0.5 * np.arctan2(2.0 * b.astype(np.float64), a.astype(np.float64) - d.astype(np.float64))
    co, so = np.cos(phi), np.sin(phi)
    mi, mj = Si.astype(np.float64) / c.astype(np.float64), Sj.astype(np.float64) / c.astype(np.float64)
    di, dj = si.astype(np.float64) - mi[ks], sj.astype(np.float64) - mj[ks]
    p, q = di * co[ks] + dj * so[ks], dj * co[ks] - di * so[ks]
    h = 0.5 * (np.abs(co) + np.abs(so))
    p0, p1 = extreme(p, np.minimum, np.inf) - h, extreme(p, np.maximum, -np.inf) + h
    q0, q1 = extreme(q, np.minimum, np.inf) - h, extreme(q, np.maximum, -np.inf) + h
    pc, qc = 0.5 * (p0 + p1), 0.5 * (q0 + q1)
    ci, cj = mi + pc * co - qc * so, mj + pc * so + qc * co
    mx, my = x_first - ci * res, y_first - cj * res
    cs, sn = math.cos(pose[2]), math.sin(pose[2])
    boxes[:, 0], boxes[:, 1] = pose[0] + (cs * mx - sn * my), pose[1] + (sn * mx + cs * my)
    boxes[:, 2] = phi + pose[2]
    boxes[:, 3], boxes[:, 4] = (p1 - p0) * res + 2.0 * pad, (q1 - q0) * res + 2.0 * pad
    comp[:, LABEL], comp[:, CELLS], comp[:, LINKED] = roots, c, n_linked
    comp[:, I_MIN], comp[:, I_MAX] = extreme(si, np.minimum, 1 << 30), extreme(si, np.maximum, -1)
    comp[:, J_MIN], comp[:, J_MAX] = extreme(sj, np.minimum, 1 << 30), extreme(sj, np.maximum, -1)
    comp[:, SUM_I], comp[:, SUM_J], comp[:, SUM_II], comp[:, SUM_IJ], comp[:, SUM_JJ] = Si, Sj, Sii, Sij, Sjj
    comp[:, FILL] = c.astype(np.float64) / ((p1 - p0) * (q1 - q0))
    return comp, boxes, dict(co=co, so=so, mi=mi, mj=mj, p0=p0, p1=p1, q0=q0, q1=q1, ks=ks, si=si, sj=sj)


def rows_restate(comp, boxes, seeds, K, min_cells, max_size):
    """Which rows are written: n (4,), comp (K, 13), boxes (K, 5), pose (K, 4), dim (K, 2), filler included; and `slots`, the indices
    of the components that got a slot."""
    passed = np.flatnonzero(comp[:, CELLS] >= min_cells)
    slots = passed[:K]
    kept = slots[~(np.maximum(boxes[slots, 3], boxes[slots, 4]) > max_size)]
    w = kept.size
    out_c, out_b = np.full((K, 13), -1.0), np.zeros((K, 5))
    out_b[:, 0], out_b[:, 1] = FAR, FAR
    out_c[:w], out_b[:w] = comp[kept], boxes[kept]
    pose, dim = np.zeros((K, 4)), out_b[:, 3:5].copy()
    pose[:, 0], pose[:, 1], pose[:, 3] = out_b[:, 0], out_b[:, 1], out_b[:, 2]
    return dict(n=np.array([comp.shape[0], passed.size, w, seeds], dtype=np.int32), comp=out_c, boxes=out_b, pose=pose, dim=dim, slots=slots,
                kept=kept)


def _x_first(g):
    return g.pos_x + (0.5 * g.len_x - 0.5 * g.res), g.pos_y + (0.5 * g.len_y - 0.5 * g.res)


def _geom(cilqr, rows, cols, res=RES, pos=GEOM_POS):
    g = cilqr.MapGeom()
    g.rows, g.cols, g.res, g.len_x, g.len_y, g.pos_x, g.pos_y = rows, cols, res, rows * res, cols * res, pos[0], pos[1]
    return g


def _poses(n):
    """One pose per layer of a shape: the identity first, then turned and shifted ones."""
    return np.array([[0.0, 0.0, 0.0]] + [[0.7 * l - 2.0, 1.1 - 0.4 * l, 0.35 * l - 1.0] for l in range(1, n)])


class _G:  # the geometry without the library, for the CPU restatements
    def __init__(self, rows, cols):
        self.rows, self.cols, self.res, self.len_x, self.len_y, self.pos_x, self.pos_y = rows, cols, RES, rows * RES, cols * RES, GEOM_POS[0], GEOM_POS[1]


@pytest.fixture(scope="module")
def cases():
    """Per shape: seeds, d2 and poses of the nine layers; per (four, gap2) the flood-fill labels and, per layer, every component with
    its box.  Computed once; never modified."""
    out = {}
    for rows, cols in SHAPES:
        seeds = seed_layers(rows, cols)
        d2 = [d2_of(s) for s in seeds]
        poses = _poses(len(seeds))
        xf, yf = _x_first(_G(rows, cols))
        per = {}
        for four in (0, 1):
            for gap2 in GAPS:
                labs = [flood_labels((d != NONE) & (d <= gap2), four) for d in d2]
                per[(four, gap2)] = dict(label=labs, comps=[components_restate(d, lab, RES, xf, yf, poses[l], PAD) for l, (d, lab) in enumerate(zip(d2, labs))])
        out[(rows, cols)] = dict(seeds=seeds, d2=d2, poses=poses, per=per)
    return out


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_MAP_OBSTACLE_FIELDS\s+13\b", h) and re.search(r"#define\s+CILQR_MAP_OBSTACLES_FOUR\s+1u", h)
    assert re.search(r"#define\s+CILQR_MAP_OBSTACLES_FAR\s+1\.0e6\b", h) and re.search(r"CILQR_ERR_INTERNAL\s*=\s*-6\b", h)
    for k, name in enumerate(FIELDS):
        assert re.search(r"CILQR_MO_%s\s*=\s*%d\b" % (name, k), h), name
        assert getattr(cilqr, "MO_" + name) == k
    assert (cilqr.MAP_OBSTACLE_FIELDS, cilqr.MAP_OBSTACLES_FOUR, cilqr.MAP_OBSTACLES_FAR, cilqr.ERR_INTERNAL) == (13, FOUR, FAR, ERR_INTERNAL)
    assert re.search(r"#define\s+CILQR_MAX_POLYGONS\s+%d\b" % cilqr.MAX_POLYGONS, h)
    for m in ("map_obstacles", "map_obstacles_device"):
        assert callable(getattr(cilqr.Solver, m)), m
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_map_obstacles\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/costmap_components.hip" in mk and len(re.findall(r"build/costmap_components\.o", mk)) == 2  # `check` and its resource list
    text = re.sub(r"\s*\n \*\s*", " ", full)
    for phrase in ("K CAPS THE SLOTS BEFORE THE SIZE FILTER", "NOT the minimum-area box", "is never linked", "bounded by rows*cols"):
        assert phrase in text, phrase


def test_the_facade_and_the_replay_tool_export_the_setter():
    """iLQR::set_map_obstacles with its fields; candidate_layout.h knows nothing of it (the rows live among the obstacles: with the
    setter off the layout and its dumps are what they were); cilqr_replay takes --map-obstacles."""
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_map_obstacles\s*\(\s*double\s+occ_threshold\s*,\s*double\s+gap\s*,\s*int\s+min_cells\s*,\s*double\s+max_size\s*,"
                     r"\s*double\s+pad\s*,\s*int\s+K\s*,\s*bool\s+on\s*=\s*true\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_map_obstacles\s*;", f) and "last_map_obstacle_counts[4]" in f
    assert "map_obstacles" not in open(os.path.join(PKG, "host", "candidate_layout.h")).read()
    r = open(os.path.join(PKG, "host", "replay_main.cpp")).read()
    assert "--map-obstacles" in r and "set_map_obstacles" in r


def test_argument_errors_need_no_device(cilqr):
    """Everything the header lists is decided before the handle is looked at (there is none here); valid arguments reach the handle."""
    L = cilqr.lib()
    rows, cols, K = 5, 4, 3
    d2, work, label = (np.zeros(2 * rows * cols, dtype=np.int32) for _ in range(3))
    n_out, comp, pose = np.zeros(8, dtype=np.int32), np.zeros(2 * K * 13), np.zeros(6)
    nan, inf = float("nan"), float("inf")
    no_handle = C.c_void_p()

    def call(dev, n=2, g=None, gap2=0, flags=0, pose_stride=3, K=K, min_cells=1, max_size=inf, pad=0.0, **nulls):
        a = dict(d2=d2, work=work, label=label, n_out=n_out, comp=comp)
        a.update(nulls)
        g = _geom(cilqr, rows, cols) if g is None else g
        f = L.cilqr_map_obstacles_device if dev else L.cilqr_map_obstacles
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, n, _p(a["d2"], _ip), C.byref(g) if g != 0 else None, gap2, C.c_uint32(flags), _p(pose), pose_stride, K, min_cells,
                 C.c_double(max_size), C.c_double(pad), _p(a["work"], _ip), _p(a["label"], _ip), _p(a["n_out"], _ip), _p(a["comp"]), None, None, None)

    for dev in (False, True):
        for name in ("d2", "work", "label", "n_out", "comp"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null" in L.cilqr_last_error(), name
        assert call(dev, g=0) == ERR_ARG and b"null" in L.cilqr_last_error()
        for n in (0, -1):
            assert call(dev, n=n) == ERR_ARG and b"must be at least 1" in L.cilqr_last_error()
        for bad in (_geom(cilqr, 0, 4), _geom(cilqr, 4, 0), _geom(cilqr, 4, 4, 0.0), _geom(cilqr, 4, 4, -0.1), _geom(cilqr, 4, 4, nan), _geom(cilqr, 4, 4, inf)):
            assert call(dev, g=bad) == ERR_ARG and b"bad geometry" in L.cilqr_last_error()
        for big in (_geom(cilqr, 1025, 2), _geom(cilqr, 2, 1025), _geom(cilqr, 8193, 2)):
            assert call(dev, g=big) == ERR_UNSUPPORTED and b"more than 1024 along a side" in L.cilqr_last_error()
        assert call(dev, gap2=-1) == ERR_ARG and b"gap2" in L.cilqr_last_error()
        assert call(dev, flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        for stride in (-3, 1, 2, 4):
            assert call(dev, pose_stride=stride) == ERR_ARG and b"pose_stride" in L.cilqr_last_error(), stride
        for k in (0, -1, 1025):
            assert call(dev, K=k) == ERR_ARG and b"K = " in L.cilqr_last_error(), k
        for m in (0, -2):
            assert call(dev, min_cells=m) == ERR_ARG and b"min_cells" in L.cilqr_last_error()
        for v in (0.0, -1.0, nan):
            assert call(dev, max_size=v) == ERR_ARG and b"max_size" in L.cilqr_last_error(), v
        for v in (-0.1, nan, inf):
            assert call(dev, pad=v) == ERR_ARG and b"pad" in L.cilqr_last_error(), v
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, g=_geom(cilqr, 1024, 1024), K=1024, flags=FOUR, gap2=7, pose_stride=0, max_size=0.5, pad=3.0) == ERR_ARG and b"null handle" in L.cilqr_last_error()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_flood_fill_against_scipy(cases, shape):
    """The restated labels equal scipy.ndimage.label with both structures, relabelled to the lowest column-major index; the component
    counts are equal too; and the layers are what they are there for."""
    from scipy import ndimage
    c = cases[shape]
    rows, cols = shape
    index = np.arange(rows)[:, None] + np.arange(cols)[None, :] * rows
    for (four, gap2), per in c["per"].items():
        structure = ndimage.generate_binary_structure(2, 1 if four else 2)
        for d2, lab in zip(c["d2"], per["label"]):
            linked = (d2 != NONE) & (d2 <= gap2)
            theirs, n = ndimage.label(linked, structure=structure)
            want = np.full(shape, -1, dtype=np.int64)
            if n:
                lowest = ndimage.minimum(index, theirs, np.arange(1, n + 1))
                want[linked] = np.asarray(lowest, dtype=np.int64)[theirs[linked] - 1]
            assert np.array_equal(lab, want), (four, gap2)
            assert np.unique(lab[linked]).size == n
    count = lambda four, gap2, name: c["per"][(four, gap2)]["comps"][LAYER_NAMES.index(name)][0].shape[0]  # noqa: E731
    seeds = dict(zip(LAYER_NAMES, c["seeds"]))
    assert count(0, 0, "none") == 0 and count(0, 0, "every") == 1 and count(0, 0, "corner") == 1 and seeds["corner"][-1, 0]
    assert count(0, 0, "serpentine") == 1 and count(1, 0, "serpentine") == 1 and count(0, 0, "comb") == 1 and count(1, 0, "comb") == 1
    assert count(1, 0, "checker") == seeds["checker"].sum()  # under FOUR every seed stands alone
    if min(rows, cols) >= 2:
        assert count(0, 0, "checker") == 1  # diagonals join them
    if rows * cols >= 6:
        assert count(0, 0, "two_blobs") == 2 and count(1, 0, "two_blobs") == 2 and count(0, 1, "two_blobs") == 1 and count(1, 1, "two_blobs") == 1
    if shape == (150, 100):
        assert count(1, 0, "checker") > 1024  # more components than any K: the truncation path
        chain = c["per"][(1, 0)]["comps"][LAYER_NAMES.index("serpentine")][0]
        assert chain[0, CELLS] > 7000  # a chain through the whole layer


def test_the_union_find_header_under_the_sanitizers(cases, tmp_path):
    """tests/cpp/components_emulation.cpp: union and find of csrc/costmap_components.hpp driven through a sequential emulation of the tile
    and seam launches, compiled with -fsanitize=address,undefined, over every test layer, connectivity and gap: the flood fill's labels,
    no loop bound reached, no sanitizer report."""
    exe = str(tmp_path / "components_emulation")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: it needs nothing loaded in front of it)
                    "-I" + os.path.join(PKG, "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "components_emulation.cpp")], check=True)
    records, want = [], []
    for (rows, cols), c in cases.items():
        for (four, gap2), per in c["per"].items():
            for d2, lab in zip(c["d2"], per["label"]):
                records.append(np.array([rows, cols, gap2, four], dtype=np.int32))
                records.append(np.ascontiguousarray(d2.T).reshape(-1))
                want.append(np.ascontiguousarray(lab.T).reshape(-1))
                want.append(np.zeros(1, dtype=np.int32))  # the overrun flag
    src, dst = tmp_path / "cases.bin", tmp_path / "labels.bin"
    np.concatenate(records).tofile(str(src))
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.split()[0] == str(len(want) // 2)
    assert np.array_equal(np.fromfile(str(dst), dtype=np.int32), np.concatenate(want))


def _corners(box):
    x, y, yaw, sx, sy = box
    c, s = math.cos(yaw), math.sin(yaw)
    return [(x + (a * c - b * s), y + (a * s + b * c)) for a, b in ((sx / 2, sy / 2), (sx / 2, -sy / 2), (-sx / 2, -sy / 2), (-sx / 2, sy / 2))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_seed_square_lies_inside_its_box(cases, shape):
    """In index coordinates: the four corners of every seed's unit square lie within [p0, p1] x [q0, q1] of their component to 1e-9
    cells; FILL is in (0, 1]; no restated size is within 1e-9 of MAX_SIZE."""
    c = cases[shape]
    worst = 0.0
    for (four, gap2), per in c["per"].items():
        for l in range(len(LAYER_NAMES)):
            comp, boxes, a = per["comps"][l]
            if comp.shape[0] == 0:
                continue
            for ei in (-0.5, 0.5):
                for ej in (-0.5, 0.5):
                    di, dj = a["si"] + ei - a["mi"][a["ks"]], a["sj"] + ej - a["mj"][a["ks"]]
                    p, q = di * a["co"][a["ks"]] + dj * a["so"][a["ks"]], dj * a["co"][a["ks"]] - di * a["so"][a["ks"]]
                    out = np.maximum.reduce([a["p0"][a["ks"]] - p, p - a["p1"][a["ks"]], a["q0"][a["ks"]] - q, q - a["q1"][a["ks"]]])
                    worst = max(worst, float(out.max()))
            assert (comp[:, FILL] > 0.0).all() and (comp[:, FILL] <= 1.0 + 1e-12).all()
            assert np.abs(boxes[:, 3:5] - MAX_SIZE).min() > TOL
    assert worst <= 1e-9


@pytest.mark.parametrize("shape", [(7, 1), (65, 3), (64, 64), (150, 100)], ids=lambda s: "%dx%d" % s)
def test_the_restated_boxes_mark_their_seeds(cilqr, cases, shape):
    """The restated boxes through cilqr_boxes_to_polygons (own pose = the layer's pose, inflate 0) and then the restated
    Polygon::isInside of tests/test_polygon_raster.py: every seed of a component is marked by its component's box."""
    c = cases[shape]
    g = _G(*shape)
    xf, yf = _x_first(g)
    cx, cy = xf - np.arange(g.rows) * RES, yf - np.arange(g.cols) * RES
    for key in ((0, 0), (1, 1)):
        per = c["per"][key]
        for l, name in enumerate(LAYER_NAMES):
            comp, boxes, _ = per["comps"][l]
            if name in ("dense", "checker") or comp.shape[0] == 0 or comp.shape[0] > 64:
                continue
            pose = c["poses"][l]
            polys = cilqr.boxes_to_polygons(boxes, pose[0], pose[1], pose[2], inflate=0.0, max_distance=1e9)
            assert polys.shape[0] == boxes.shape[0]
            assert np.max(np.abs(polys - boxes_to_polygons_restated(boxes, pose[0], pose[1], pose[2], 0.0, 1e9))) < 1e-12
            for k in range(comp.shape[0]):
                mask = inside_mask(cx, cy, [polys[k]])
                mine = (per["label"][l] == int(comp[k, LABEL])) & (c["d2"][l] == 0)
                assert mask[mine].all(), (key, name, k)


def _filler_scene(O, N=40):
    """One candidate on a straight path and one obstacle beside it (dense tables, constant over the horizon)."""
    p = O.default_params(N)
    path = np.stack([np.arange(200.0), np.zeros(200)], 1)
    x0 = np.array([[0.0, 0.2, 4.0, 0.0]])
    coeffs, ref = O.local_plan(p, path, x0[0])
    U0 = np.zeros((1, N, 2))
    O.lib().oracle_default_control_seq(N, _p(U0[0]))
    return dict(p=p, N=N, x0=x0, poly=coeffs[None], fl=np.array([[ref[0, 0], ref[-1, 0]]]), U0=U0.reshape(1, -1),
                pose=np.array([8.0, 1.0, 0.0, 0.3]), dim=np.array([2.0, 1.0]))


def _dense(pose_rows, dim_rows, B, N):
    """(M, 4) / (M, 2) rows -> the dense (B, M, 4N) / (B, M, 2N) tables of a static set shared by the batch."""
    M = pose_rows.shape[0]
    return np.tile(pose_rows[None, :, None, :], (B, 1, N, 1)).reshape(B, M, 4 * N), np.tile(dim_rows[None, :, None, :], (B, 1, N, 1)).reshape(B, M, 2 * N)


def test_filler_rows_change_no_bit_of_a_solve(oracle):
    """The oracle's solve at N = 40 with one real obstacle and three filler rows at 1e4, 1e6 (CILQR_MAP_OBSTACLES_FAR), 1e9 and 1e150
    equals the solve with the one row alone: U, J, iterations and status bit for bit.  The filler's barrier term underflows to 0."""
    O = oracle
    s = _filler_scene(O)
    N = s["N"]
    pose1, dim1 = _dense(s["pose"][None], s["dim"][None], 1, N)
    alone = O.solve_batch(s["p"], N, 1, s["x0"], s["U0"], s["poly"], s["fl"], pose1, dim1)
    bare = O.solve_batch(s["p"], N, 0, s["x0"], s["U0"], s["poly"], s["fl"])
    assert not np.array_equal(alone["U"], bare["U"])  # the real obstacle matters
    for far in (1e4, FAR, 1e9, 1e150):
        rows = np.array([s["pose"]] + [[far, far, 0.0, 0.0]] * 3)
        dims = np.array([s["dim"]] + [[0.0, 0.0]] * 3)
        pose4, dim4 = _dense(rows, dims, 1, N)
        got = O.solve_batch(s["p"], N, 4, s["x0"], s["U0"], s["poly"], s["fl"], pose4, dim4)
        for k in ("U", "J", "X"):
            assert np.array_equal(got[k].view(np.uint64), alone[k].view(np.uint64)), (far, k)
        assert np.array_equal(got["iters"], alone["iters"]) and np.array_equal(got["status"], alone["status"]), far


# ---- the scene that shows what the call is for -------------------------------------------------------------------------------------------
SCENE_K, SCENE_MIN_CELLS = 4, 3


@pytest.fixture(scope="module")
def scene(oracle):
    """The blob scene of tests/test_tighten_map.py, from the oracle and the restatements alone: the component of the blob and its box;
    the solve with the map only and with the map plus the K rows (filler included); exact clearances to the ORIGINAL map and
    CILQR_FP_CLEARANCE of both."""
    O = oracle
    s = _round_scene(O)
    g, pose, N, B = s["g"], s["poses"], s["N"], s["B"]
    d2 = d2_of(seeds_of(s["layers"], THRESHOLD))
    lab = flood_labels(d2 == 0, 0)
    xf, yf = _x_first(g)
    comp, boxes, _ = components_restate(d2, lab, g.res, xf, yf, pose, 0.0)
    rows = rows_restate(comp, boxes, int((d2 == 0).sum()), SCENE_K, SCENE_MIN_CELLS, math.inf)
    th = min(8, O.max_threads())
    um, keep = O.uncertainty_map(s["layers"], g, pose, s["probes"])
    before = O.solve_batch_unc(s["p"], N, 0, s["x0"], s["U0"].copy(), s["poly"], s["fl"], None, None, None, um, threads=th)
    obs_pose, obs_dim = _dense(rows["pose"], rows["dim"], B, N)
    after = O.solve_batch_unc(s["p"], N, SCENE_K, s["x0"], s["U0"].copy(), s["poly"], s["fl"], obs_pose, obs_dim, None, um, threads=th)
    clr = [rect_clearance(s["p"], g, pose, s["layers"], r["X"], N, THRESHOLD) for r in (before, after)]
    w = int(rows["n"][2])
    fp = [footprint_restate(s["p"], N, r["X"], pose=obs_pose[:, :w], dim=obs_dim[:, :w])["fp"][:, 0] for r in (before, after)]
    fp_none = footprint_restate(s["p"], N, before["X"])["fp"][:, 0]
    return dict(s=s, d2=d2, label=lab, comp=comp, boxes=boxes, rows=rows, before=before, after=after, clr_before=clr[0], clr_after=clr[1],
                fp_before=fp[0], fp_after=fp[1], fp_none=fp_none, obs_pose=obs_pose, obs_dim=obs_dim)


def test_the_box_does_what_it_is_for(scene):
    """From the oracle's solves on the CPU (the figures are in the module docstring, the README and DESIGN §4.8r): the blob is one
    component; with M = 0 CILQR_FP_CLEARANCE has nothing to act on (+inf); with the box in the obstacle channel the plan deepest in
    contact with the occupied cells ends clear of them, and every plan is at least 0.4 m farther from the ORIGINAL map than before."""
    a = scene
    r = a["rows"]
    print("components %s, box %s, FILL %.4f" % (r["n"].tolist(), np.round(r["boxes"][0], 4).tolist(), r["comp"][0, FILL]))
    print("clearance to the original map  map only  %s\n                               map + box %s" % (
        np.round(a["clr_before"], 4).tolist(), np.round(a["clr_after"], 4).tolist()))
    print("FP_CLEARANCE to the box        map only  %s\n                               map + box %s\niterations %s -> %s" % (
        np.round(a["fp_before"], 4).tolist(), np.round(a["fp_after"], 4).tolist(), a["before"]["iters"].tolist(), a["after"]["iters"].tolist()))
    assert ROUND_BLOB[:2] == (6.0, -1.4) and a["s"]["B"] == 6
    assert r["n"].tolist() == [1, 1, 1, 266] and r["comp"][0, CELLS] == 266
    assert np.allclose(r["boxes"][0, :2], (5.978, -1.403), atol=1e-3) and np.allclose(r["boxes"][0, 3:], (1.8, 1.8), atol=1e-3)
    assert abs(r["comp"][0, FILL] - 0.821) < 1e-3
    assert np.all(np.isposinf(a["fp_none"]))  # M = 0: nothing to measure against
    k = int(np.argmin(a["clr_before"]))
    assert k == 0 and a["clr_before"][k] < 0.0 < a["clr_after"][k]  # the plan deepest in contact ends clear
    assert np.all(a["clr_after"] > a["clr_before"] + 0.4) and np.all(a["fp_after"] > a["fp_before"] + 0.4) and np.all(np.isfinite(a["fp_after"]))
    assert np.allclose(a["clr_before"], [-0.6525, -0.5389, -0.4242, -0.3279, -0.2278, -0.1332], atol=5e-4)
    assert np.allclose(a["clr_after"], [0.0777, -0.0009, 0.0673, 0.2623, 0.4894, 0.6655], atol=5e-4)
    assert np.allclose(a["fp_before"], [-0.7844, -0.6320, -0.4815, -0.4132, -0.3407, -0.2730], atol=5e-4)
    assert np.allclose(a["fp_after"], [-0.0990, -0.1027, -0.0034, 0.2034, 0.4322, 0.5890], atol=5e-4)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


SENTINEL_I, SENTINEL_F = -7, -7.5  # what the output buffers hold before a call


def _device(cilqr, solver, d2s, g, K, gap2=0, flags=0, poses=None, pose_stride=3, min_cells=1, max_size=math.inf, pad=PAD, tables=True):
    """The device form on torch buffers.  d2s: a list of (rows, cols) int32.  Returns dict(label (L, rows, cols), n, comp, boxes, pose,
    dim)."""
    import torch
    dev = torch.device("cuda", 0)
    rows, cols, n = int(g.rows), int(g.cols), len(d2s)
    cells = rows * cols
    d2 = torch.from_numpy(np.stack([np.ascontiguousarray(d.T).reshape(-1) for d in d2s]).astype(np.int32)).to(dev)
    work = torch.full((n, cells), SENTINEL_I, dtype=torch.int32, device=dev)
    label = torch.full((n, cells), SENTINEL_I, dtype=torch.int32, device=dev)
    counts = torch.full((n, 4), SENTINEL_I, dtype=torch.int32, device=dev)
    comp = torch.full((n, K, 13), SENTINEL_F, dtype=torch.float64, device=dev)
    boxes, pose_out, dim_out = (torch.full((n, K, w), SENTINEL_F, dtype=torch.float64, device=dev) if tables else None for w in (5, 4, 2))
    pose = None if poses is None else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).to(dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)
    solver.map_obstacles_device(st, n, d2.data_ptr(), g, K, work.data_ptr(), label.data_ptr(), counts.data_ptr(), comp.data_ptr(), ptr(boxes),
                                ptr(pose_out), ptr(dim_out), gap2=gap2, flags=flags, pose=ptr(pose), pose_stride=pose_stride if poses is not None else 0,
                                min_cells=min_cells, max_size=max_size, pad=pad)
    torch.cuda.synchronize(dev)
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(label=label.cpu().numpy().reshape(n, cols, rows).transpose(0, 2, 1), n=host(counts), comp=host(comp), boxes=host(boxes),
                pose=host(pose_out), dim=host(dim_out))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


INTEGER_FIELDS = [f for f in range(13) if f != FILL]


def _check_layer(got, l, want_label, want, what):
    """One layer of a device result against the restated label array and rows."""
    assert np.array_equal(got["label"][l], want_label), what
    assert np.array_equal(got["n"][l], want["n"]), (what, got["n"][l].tolist(), want["n"].tolist())
    assert np.array_equal(got["comp"][l][:, INTEGER_FIELDS], want["comp"][:, INTEGER_FIELDS]), what
    w = int(want["n"][2])
    fill_got, fill_want = got["comp"][l][:, FILL], want["comp"][:, FILL]
    assert np.all(np.abs(fill_got[:w] - fill_want[:w]) <= TOL * fill_want[:w]) and np.array_equal(fill_got[w:], fill_want[w:]), what
    for k in ("boxes", "pose", "dim"):
        assert np.max(np.abs(got[k][l] - want[k]), initial=0.0) <= TOL, (what, k)
        assert np.array_equal(_bits(got[k][l][w:]), _bits(want[k][w:])), (what, k)  # the filler rows, bit for bit


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_labels_counts_moments_and_boxes_against_the_restatement(cilqr, solver, cases, shape):
    """Every layer of the shape in one batch (L = 9, one pose per layer), for 8 and FOUR, gap2 in {0, 1, 4}, min_cells in {1, 3},
    K in {1, 4, 1024} and max_size infinite and finite: label_out, n_out and every integer field exactly, boxes, poses, dims and FILL
    within 1e-9, the filler rows bit for bit.  Truncation, the size filter and filler rows all occur, and n_out shows each."""
    c = cases[shape]
    g = _geom(cilqr, *shape)
    seen = dict(truncated=0, dropped=0, filler=0, full=0)
    for (four, gap2), per in c["per"].items():
        for min_cells in (1, 3):
            for K in (1, 4, 1024):
                for max_size in (math.inf, MAX_SIZE):
                    got = _device(cilqr, solver, c["d2"], g, K, gap2=gap2, flags=FOUR if four else 0, poses=c["poses"], min_cells=min_cells,
                                  max_size=max_size)
                    for l, name in enumerate(LAYER_NAMES):
                        comp, boxes, _ = per["comps"][l]
                        want = rows_restate(comp, boxes, int(c["seeds"][l].sum()), K, min_cells, max_size)
                        _check_layer(got, l, per["label"][l], want, (four, gap2, min_cells, K, max_size, name))
                        n = want["n"]
                        seen["truncated"] += n[1] > K
                        seen["dropped"] += n[2] < min(n[1], K)
                        seen["filler"] += n[2] < K
                        seen["full"] += n[2] == K
    assert seen["filler"] > 0 and seen["full"] > 0
    if shape[0] * shape[1] >= 64 * 64:
        assert seen["truncated"] > 0 and seen["dropped"] > 0, seen


@gpu
def test_a_layers_bits_depend_on_that_layer_alone(cilqr, solver, cases):
    """layer -> cilqr_map_distance_device -> cilqr_map_obstacles_device with L = 3: the layer in the middle of a batch of different
    layers (dense), and one shared layer (layer_stride 0) three times: every output of the layer is bit-identical to its L = 1 run."""
    import torch
    dev = torch.device("cuda", 0)
    for shape in ((65, 3), (130, 129), (150, 100)):
        c = cases[shape]
        g = _geom(cilqr, *shape)
        rows, cols = shape
        cells = rows * cols
        seeds = dict(zip(LAYER_NAMES, c["seeds"]))
        layer = lambda name: np.ascontiguousarray((100.0 * seeds[name]).astype(np.float32).T).reshape(-1)  # noqa: E731
        st = torch.cuda.current_stream(dev).cuda_stream

        def run(names, stride, pose):
            n = len(names) if stride else 3
            lay = torch.from_numpy(np.concatenate([layer(nm) for nm in names])).to(dev)
            d2 = torch.zeros((n, cells), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            solver.map_distance_device(st, n, lay.data_ptr(), stride, g, THRESHOLD, d2.data_ptr())
            torch.cuda.synchronize(dev)
            d2s = [a.reshape(cols, rows).T for a in d2.cpu().numpy()]
            return _device(cilqr, solver, d2s, g, 16, gap2=1, poses=pose, pose_stride=3 if np.ndim(pose) == 2 else 0, max_size=MAX_SIZE)
        pose = np.array([0.4, -0.3, 0.2])
        alone = run(["sparse"], cells, pose[None])
        assert alone["n"][0, 3] == seeds["sparse"].sum() and (cells < 10000 or alone["n"][0, 2] > 8)
        batch = run(["dense", "sparse", "comb"], cells, np.stack([pose + 1.0, pose, pose - 1.0]))
        shared = run(["sparse"], 0, pose)
        for k in ("n", "comp", "boxes", "pose", "dim", "label"):
            same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))  # noqa: E731
            assert same(batch[k][1], alone[k][0]), (shape, k)
            for l in range(3):
                assert same(shared[k][l], alone[k][0]), (shape, k, l)


@gpu
def test_the_host_form_optional_outputs_and_a_null_pose(cilqr, solver, cases):
    """The host form gives the device form's bits, with the optional outputs and without them; pose NULL is pose (0, 0, 0)."""
    for shape in ((7, 1), (64, 64), (150, 100)):
        c = cases[shape]
        g = _geom(cilqr, *shape)
        d2s = c["d2"][:3] if shape == (150, 100) else c["d2"]  # (three of the node's layers fit the arena of this handle)
        poses = c["poses"][:len(d2s)]
        kw = dict(gap2=1, min_cells=2, max_size=MAX_SIZE)
        dev = _device(cilqr, solver, d2s, g, 8, poses=poses, **kw)
        host = solver.map_obstacles(np.stack(d2s), g, 8, pose=poses, pad=PAD, **kw)
        bare_dev = _device(cilqr, solver, d2s, g, 8, poses=poses, tables=False, **kw)
        bare_host = solver.map_obstacles(np.stack(d2s), g, 8, pose=poses, pad=PAD, tables=False, **kw)
        for k in ("label", "n", "comp", "boxes", "pose", "dim"):
            assert np.array_equal(np.ascontiguousarray(host[k]).view(np.uint8), np.ascontiguousarray(dev[k]).view(np.uint8)), (shape, k)
        for k in ("label", "n", "comp"):
            assert np.array_equal(np.ascontiguousarray(bare_dev[k]).view(np.uint8), np.ascontiguousarray(dev[k]).view(np.uint8)), (shape, k)
            assert np.array_equal(np.ascontiguousarray(bare_host[k]).view(np.uint8), np.ascontiguousarray(dev[k]).view(np.uint8)), (shape, k)
        assert bare_dev["boxes"] is None and bare_host["boxes"] is None and bare_host["pose"] is None and bare_host["dim"] is None
        null = _device(cilqr, solver, d2s, g, 8, poses=None, **kw)
        zero = _device(cilqr, solver, d2s, g, 8, poses=np.zeros(3), pose_stride=0, **kw)
        per_layer = _device(cilqr, solver, d2s, g, 8, poses=np.zeros((len(d2s), 3)), **kw)
        for k in ("label", "n", "comp", "boxes", "pose", "dim"):
            for other in (zero, per_layer):
                assert np.array_equal(np.ascontiguousarray(null[k]).view(np.uint8), np.ascontiguousarray(other[k]).view(np.uint8)), (shape, k)
        assert dev["n"][:, 2].max() > 0
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers" % ERR_ARG):
        solver.map_obstacles(np.stack(cases[(150, 100)]["d2"] + cases[(150, 100)]["d2"]), _geom(cilqr, 150, 100), 8)
    assert solver.map_obstacles(cases[(7, 1)]["d2"][3], _geom(cilqr, 7, 1), 2)["n"][0].tolist() == [1, 1, 1, 7]  # the handle stays usable


@gpu
def test_round_trip_boxes_to_polygons_to_the_rasteriser(cilqr, solver, cases):
    """On the device: boxes -> cilqr_boxes_to_polygons (own pose = the layer's pose, inflate 0) -> cilqr_rasterize_polygons_device marks
    every seed of the components that got a row."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    for shape in ((65, 3), (64, 64), (150, 100)):
        c = cases[shape]
        g = _geom(cilqr, *shape)
        rows, cols = shape
        names = ("sparse", "corner", "comb", "two_blobs", "every")
        pick = [LAYER_NAMES.index(nm) for nm in names]
        got = _device(cilqr, solver, [c["d2"][l] for l in pick], g, 64, poses=c["poses"][pick], pad=0.0)
        for k, l in enumerate(pick):
            w = int(got["n"][k, 2])
            assert w == min(int(got["n"][k, 1]), 64) and w > 0
            pose = c["poses"][l]
            polys = cilqr.boxes_to_polygons(got["boxes"][k][:w], pose[0], pose[1], pose[2], inflate=0.0, max_distance=1e9)
            assert polys.shape[0] == w
            layer = torch.zeros(rows * cols, dtype=torch.float32, device=dev)
            torch.cuda.synchronize(dev)
            solver.rasterize_polygons_device(st, g, polys, layer.data_ptr(), value=100.0, clear=True)
            torch.cuda.synchronize(dev)
            marked = layer.cpu().numpy().reshape(cols, rows).T == 100.0
            mine = np.isin(got["label"][k], got["comp"][k][:w, LABEL].astype(np.int64)) & (c["d2"][l] == 0)
            assert mine.any() and marked[mine].all(), (shape, names[k])


@gpu
def test_pipeline_layer_to_distance_to_obstacles_to_solve(cilqr, scene):
    """layer -> cilqr_map_distance_device -> cilqr_map_obstacles_device -> cilqr_solve_batch_obstacles_device with strides (0, 1, 0) and
    M = K, on device buffers as one sequence on one stream, against the oracle's solve on the restated rows, filler included:
    max|dU| <= 1e-9, equal iterations and exits; the rows within 1e-9 of the restatement; the clearances of the module docstring."""
    import torch
    a = scene
    s = a["s"]
    B, N, g, K = s["B"], s["N"], s["g"], SCENE_K
    cells = int(g.rows) * int(g.cols)
    geom = cilqr.map_geom(*s["geom"])
    solver = cilqr.Solver(_round_params(cilqr, N), max_batch=B, max_horizon=N, max_obstacles=K, device=0)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
        x0, U, poly, fl, pose = (up(v) for v in (s["x0"], s["U0"], s["poly"], s["fl"], np.array(s["poses"])))
        layer = torch.from_numpy(np.ascontiguousarray(s["layers"].T).reshape(-1)).to(dev)
        d2, work, label = (torch.zeros(cells, dtype=torch.int32, device=dev) for _ in range(3))
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        comp, boxes, pose_out, dim_out = (torch.zeros((K, w), dtype=torch.float64, device=dev) for w in (13, 5, 4, 2))
        X, J = torch.zeros((B, 4 * (N + 1)), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
        it, ex = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        solver.set_uncertainty_map_device(layer.data_ptr(), geom, s["poses"], s["probes"])
        solver.map_distance_device(st, 1, layer.data_ptr(), 0, geom, THRESHOLD, d2.data_ptr())
        solver.map_obstacles_device(st, 1, d2.data_ptr(), geom, K, work.data_ptr(), label.data_ptr(), counts.data_ptr(), comp.data_ptr(),
                                    boxes.data_ptr(), pose_out.data_ptr(), dim_out.data_ptr(), pose=pose.data_ptr(), min_cells=SCENE_MIN_CELLS, pad=0.0)
        solver.solve_batch_obstacles_device(st, B, N, K, x0.data_ptr(), U.data_ptr(), poly.data_ptr(), fl.data_ptr(), pose_out.data_ptr(),
                                            dim_out.data_ptr(), 0, (0, 1, 0, 0), X.data_ptr(), J.data_ptr(), it.data_ptr(), ex.data_ptr())
        torch.cuda.synchronize(dev)
        solver.clear_uncertainty_map()
    finally:
        solver.close()
    want = a["rows"]
    assert np.array_equal(d2.cpu().numpy().reshape(int(g.cols), int(g.rows)).T, a["d2"])
    assert np.array_equal(label.cpu().numpy().reshape(int(g.cols), int(g.rows)).T, a["label"])
    assert np.array_equal(counts.cpu().numpy(), want["n"])
    assert np.max(np.abs(pose_out.cpu().numpy() - want["pose"])) <= TOL and np.max(np.abs(dim_out.cpu().numpy() - want["dim"])) <= TOL
    assert np.max(np.abs(boxes.cpu().numpy() - want["boxes"])) <= TOL
    dU = float(np.max(np.abs(U.cpu().numpy() - a["after"]["U"])))
    print("max|dU| %.3g, iterations %s (oracle %s)" % (dU, it.cpu().numpy().tolist(), a["after"]["iters"].tolist()))
    assert np.array_equal(it.cpu().numpy(), a["after"]["iters"]) and np.array_equal(ex.cpu().numpy(), a["after"]["status"])
    assert dU <= 1e-9
    got_clr = rect_clearance(s["p"], g, s["poses"], s["layers"], X.cpu().numpy(), N, THRESHOLD)
    k = int(np.argmin(a["clr_before"]))
    assert got_clr[k] > 0.0 > a["clr_before"][k] and np.all(got_clr > a["clr_before"] + 0.4)
    assert np.allclose(got_clr, a["clr_after"], atol=1e-6)


def _build(tmp_path, source, *includes, lib=False):
    exe = str(tmp_path / source.replace(".cpp", ""))
    link = ["-L" + os.path.join(PKG, "lib"), "-lcilqr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib")] if lib else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall"] + ["-I" + d for d in includes] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", source)] + link, check=True)
    return exe


@gpu
def test_cpp_facade_map_obstacles(scene, tmp_path):
    """tests/cpp/candidates_map_obstacles.cpp: run_candidates under iLQR::set_map_obstacles against the C-ABI sequence called by hand, bit
    for bit, last_map_obstacles against that call's rows, and the setter off against the solve without the row (inside the program); its
    row and costs against the restatement and the oracle's solves (here)."""
    exe = _build(tmp_path, "candidates_map_obstacles.cpp", os.path.join(ROOT, "include"), os.path.join(PKG, "host"), lib=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map obstacles ok" in r.stdout
    row = np.array([float(v) for v in re.search(r"rows:(.*)", r.stdout).group(1).split()])
    J = np.array([float(v) for v in re.search(r"J:(.*)", r.stdout).group(1).split()])
    J0 = np.array([float(v) for v in re.search(r"J0:(.*)", r.stdout).group(1).split()])
    # (the program's plans are the device's, 1e-9 from the oracle's, and its layer is libm's where the scene's is numpy's)
    assert np.max(np.abs(row - scene["rows"]["boxes"][0])) <= 1e-6
    assert np.max(np.abs(J - scene["after"]["J"])) <= 1e-6 and np.max(np.abs(J0 - scene["before"]["J"])) <= 1e-6


@gpu
def test_replay_tool_reports_the_boxes(tmp_path):
    """cilqr_replay --map-obstacles: a tick with a map of two blobs reports two boxes of two components, a tick without a map none, and
    without the option the line is what it was."""
    exe = os.path.join(PKG, "bin", "cilqr_replay")
    cells = ["%d %d 100" % (i, j) for i in range(20, 24) for j in range(10, 13)] + ["%d %d 100" % (i, j) for i in range(60, 63) for j in range(30, 34)]
    cells.append("90 5 100")  # a single return: below min_cells
    log = tmp_path / "two_ticks.log"
    log.write_text("cilqr-replay 1\nhorizon 10\npath 3\n0 0\n50 0\n100 0\ntick\nego 0 0 1 0\nobstacles 0\n"
                   "map 10.0 5.0 0.1 20.0 8.0 0.0 0.0 0.0 %d\n%s\ntick\nego 0 0 1 0\nobstacles 0\n" % (len(cells), "\n".join(cells)))
    r = subprocess.run([exe, str(log), "--map-obstacles", "50,0,2,3.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and lines[0].endswith(" map_obstacles 2 3") and lines[1].endswith(" map_obstacles 0 0")
    plain = subprocess.run([exe, str(log)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and all("map_obstacles" not in line for line in plain.stdout.splitlines())
