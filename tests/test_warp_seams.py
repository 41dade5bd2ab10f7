"""The estimate/exact seam of csrc/costmap_warp.hip, and the source lengths its kernels rely on.

The warp kernels decide the first cell of a lane's run the reference's way (cell_exact: IEEE division, a `len` test and an index
test) and the cells after it from an estimate (cell_estimated), which falls back to cell_exact only when a quotient lies within
estimate_guard of an integer.  Generic poses never come near an integer, so these inputs are built to: grids whose cell centres
land ON source-cell boundaries (aligned, same-resolution, the map's own edges at 0 and `rows`), the same far from the origin
(where one ulp of a coordinate is 2e-9 cells), and non-finite poses.  The CPU tests prove, with the oracle's index arithmetic in
numpy and nothing of the kernel's, that the inputs do reach the seam; the -m gpu tests hold every kernel form to oracle.warp bit
for bit (np.array_equal(..., equal_nan=True), the out-of-range count with ==).  The oracle is pinned to the reference's
grid_map_core by tests/test_oracle.py.

Every source layer identifies its cells, src[i, j] = float32(j * rows + i) (exact below 2^24), so a read from a wrong neighbour
always shows; NaN holes go on top where a case needs NaN destination cells.

Which of the eight instantiations a call reaches follows from the launchers' predicates (launch_warp, launch_warp_batch,
launch_warp_polygons in costmap_warp.hip), with r = destination rows and K = frames of the call:
    r % 4 != 0:  single frame -> warp_kernel<false,false>;  K >= 2 -> warp_kernel<false,true>;  polygons -> warp_kernel<true,false>
    r % 4 == 0:  CILQR_WARP_LDS=1 (and the staged box fits 48 KiB: _tile_fits) -> warp_tile_kernel, any K
                 else r % 8 == 0 and CILQR_WARP_ROWS=8 -> warp_batch_kernel<8,true,false>, any K
                 else K >= 4 -> warp_batch_kernel<4,true,false>;  K < 4 (a single frame is K = 1) -> warp_batch_kernel<4,false,false>
                 polygons -> warp_batch_kernel<4,false,true>
so destination maps of 68 rows (in fours, not eights), 72 rows (in eights) and 66 rows (not in fours) with K = 1, 2, 3, 5 and the
two switches reach all eight (_forms).

The second half is the rule that a warp's SOURCE geometry carries len == (double)size * res (cilqr_map_geom_set's bits): the
estimate tests 0 < q < size only, the exact path t < len as well, and the two disagree inside one lane's run when len is shorter
(test_shrunk_source_lengths_make_the_two_in_map_tests_disagree records it on the oracle).  Every warp and frame entry point
rejects such a geometry with CILQR_ERR_ARG before anything is enqueued.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import load_golden

# ------------------------------------------------------------------------------------------------------------ the inputs
SRC_NEAR = (60.0, 52.0, 0.2, 3.0, -2.0)             # 300 x 260
SRC_FAR = (60.0, 52.0, 0.2, 500003.0, 4000002.0)    # the same map 4e6 m from the origin
SRC_SAME_RES = (12.0, 10.0, 0.2, 0.0, 0.0)          # 60 x 50
SRC_EDGE = (4.0, 4.0, 0.5, 0.5, -0.5)               # 8 x 8: most of every destination map lies outside it

# destination geometries by row class: rows in fours but not eights / in eights / not in fours
DST_01 = {68: (6.8, 3.3, 0.1, 1.0, 0.0), 72: (7.2, 3.3, 0.1, 1.0, 0.0), 66: (6.6, 3.3, 0.1, 1.0, 0.0)}
DST_SAME_RES = {36: (7.2, 3.4, 0.2, 1.0, 0.0), 32: (6.4, 3.4, 0.2, 1.0, 0.0), 33: (6.6, 3.4, 0.2, 1.1, 0.0)}  # (33 rows: centre moved half a cell to stay aligned)
DST_EDGE = {44: (22.0, 12.0, 0.5, 1.0, 1.0), 40: (20.0, 12.0, 0.5, 1.0, 1.0), 42: (21.0, 12.0, 0.5, 1.0, 1.0)}

THETAS = (0.0, math.pi / 2, math.pi, -math.pi / 2)
SIGNS = ((1, 1), (-1, 1), (1, -1), (-1, -1))
ALIGNED = [(sx * 0.05, sy * 0.05, th) for (sx, sy), th in zip(SIGNS, THETAS)]
CONTROL = (0.05, 0.05, 0.3)
# far from the origin BOTH quotients are near integers (test_inputs_reach_the_seam): there the exact arithmetic of a cell is off an
# integer by the rounding of its own rotated centre (1e-9 cells) and an estimate by that of the run's first cell, so the two can
# truncate apart only along the direction in which the near-integer quotient CHANGES — down the rows for the kernels whose runs
# follow rows, across the columns for warp_kernel, whose runs follow columns.  With one axis aligned, one of the two never sees it.
FAR_ALIGNED = [(500000.05, 4000000.0, THETAS[0]), (500000.0, 4000000.05, THETAS[1]), (499999.95, 4000000.1, THETAS[2]), (500000.0, 3999999.95, THETAS[3])]
FAR_GENERIC = [(500000.37, 3999999.21, 0.3), (499998.9, 4000001.3, -2.1), (500001.234, 4000000.777, 1.234)]
SAME_RES_POSES = [(0.1, 0.1, th) for th in THETAS]
EDGE_POSES = [(0.25, 0.25, 0.0), (0.5, 0.5, 0.0)]
NAN, INF = float("nan"), float("inf")
NONFINITE = [(NAN, 0.05, 0.0), (0.05, INF, 0.0), (0.05, 0.05, NAN)]
# finite and non-finite frames interleaved: every batch window of _windows holds both
NONFINITE_MIX = [ALIGNED[0], NONFINITE[0], ALIGNED[1], NONFINITE[1], CONTROL, NONFINITE[2], ALIGNED[2]]


class Case:
    """One source map, one destination map, a list of poses; the layers the runs share are made once."""

    def __init__(self, name, sgeo, dgeo, poses):
        self.name, self.sgeo, self.dgeo, self.poses = name, sgeo, dgeo, [tuple(p) for p in poses]
        self._made = {}

    def geoms(self, mod):
        return mod.map_geom(*self.sgeo), mod.map_geom(*self.dgeo)

    def layer(self, which, oracle):
        """'ident': the cell-identifying source.  'holed': the same with 2 % NaN holes.  'bbox': 3 % of the destination cells at
        100, one at exactly 90.0 (not above 90: the warped value stays) and one at 95 on a cell that is NaN in the first frame."""
        if which in self._made:
            return self._made[which]
        osg, odg = self.geoms(oracle)
        if which == "ident":
            out = ident_source(osg.rows, osg.cols)
        elif which == "holed":
            out = self.layer("ident", oracle).copy(order="F")
            out[np.random.default_rng(11).random(out.shape) < 0.02] = np.nan
        else:
            rng = np.random.default_rng(5)
            out = np.zeros((odg.rows, odg.cols), dtype=np.float32, order="F")
            out[rng.random(out.shape) < 0.03] = 100.0
            first = next(p for p in self.poses if all(map(math.isfinite, p)))
            w0, _ = oracle.warp(self.layer("holed", oracle), osg, odg, *first)
            fin, nan = np.argwhere(~np.isnan(w0) & (out == 0.0)), np.argwhere(np.isnan(w0) & (out == 0.0))
            assert len(fin) and len(nan), self.name  # a condition on the inputs: the case has both kinds of destination cell
            out[tuple(fin[len(fin) // 2])] = 90.0
            out[tuple(nan[len(nan) // 2])] = 95.0
        self._made[which] = out
        return out


def ident_source(rows, cols):
    assert rows * cols < 2 ** 24
    return np.arange(rows * cols, dtype=np.float32).reshape((rows, cols), order="F")  # src[i, j] = j * rows + i


def _cases():
    out = []
    for rows, dgeo in DST_01.items():
        out.append(Case("aligned_%d" % rows, SRC_NEAR, dgeo, ALIGNED + [CONTROL]))
        out.append(Case("far_%d" % rows, SRC_FAR, dgeo, FAR_ALIGNED + FAR_GENERIC))
    for rows, dgeo in DST_SAME_RES.items():
        out.append(Case("same_res_%d" % rows, SRC_SAME_RES, dgeo, SAME_RES_POSES))
    for rows, dgeo in DST_EDGE.items():
        out.append(Case("edge_%d" % rows, SRC_EDGE, dgeo, EDGE_POSES))
    return out


CASES = _cases()
NONFINITE_CASES = [Case("nonfinite_%d" % rows, SRC_NEAR, dgeo, NONFINITE_MIX) for rows, dgeo in DST_01.items()]
_WANT = {}  # (case, layer, bbox?, pose) -> the oracle's (dst, n_oob): computed once, shared by every form, never written to


def want(oracle, case, pose, which, with_bbox):
    key = (case.name, which, with_bbox, repr(pose))
    if key not in _WANT:
        osg, odg = case.geoms(oracle)
        dst, oob = oracle.warp(case.layer(which, oracle), osg, odg, *pose, bbox=case.layer("bbox", oracle) if with_bbox else None)
        dst.setflags(write=False)
        _WANT[key] = (dst, oob)
    return _WANT[key]


def quotients(sg, dg, pose):
    """The oracle's index arithmetic (warp_oracle.c: oracle_map_get_position, the rotation, oracle_map_get_index) over the whole
    destination map: the quotients whose truncation is the source index, and the rotated centres."""
    vx, vy, th = pose
    s, c = math.sin(th), math.cos(th)
    i = np.arange(dg.rows, dtype=np.float64)[:, None]
    j = np.arange(dg.cols, dtype=np.float64)[None, :]
    Cx = (dg.pos_x + (0.5 * dg.len_x - 0.5 * dg.res)) + dg.res * (-i)
    Cy = (dg.pos_y + (0.5 * dg.len_y - 0.5 * dg.res)) + dg.res * (-j)
    x_og = (Cx * c - Cy * s) + vx
    y_og = (Cx * s + Cy * c) + vy
    qx = -(((x_og - 0.5 * sg.len_x) - sg.pos_x) / sg.res)
    qy = -(((y_og - 0.5 * sg.len_y) - sg.pos_y) / sg.res)
    return qx, qy, x_og, y_og


def boundary_share(sg, dg, pose, tol):
    qx, qy, _, _ = quotients(sg, dg, pose)
    return float(np.mean((np.abs(qx - np.rint(qx)) < tol) | (np.abs(qy - np.rint(qy)) < tol)))


def _tile_fits(sg, dg):
    """launch_warp_batch's own condition for the LDS-tiled kernel (64 x 32 destination tiles), beside CILQR_WARP_LDS=1."""
    side = math.ceil(math.sqrt(64.0 * 64.0 + 32.0 * 32.0) * (dg.res / sg.res)) + 6.0
    return side * side * 4 <= 48.0 * 1024.0


def _forms(rows):
    """(name, frames per call, environment) for a destination map of `rows` rows, and the instantiation it reaches."""
    if rows % 4:
        return [("single", 1, {}, "warp_kernel<false,false>"), ("frames_K3", 3, {}, "warp_kernel<false,true>")]
    forms = [("single", 1, {}, "warp_batch_kernel<4,false,false>"), ("batch_K2", 2, {}, "warp_batch_kernel<4,false,false>"),
             ("batch_K5", 5, {}, "warp_batch_kernel<4,true,false>"),
             ("tile_single", 1, {"CILQR_WARP_LDS": "1"}, "warp_tile_kernel"), ("tile_K5", 5, {"CILQR_WARP_LDS": "1"}, "warp_tile_kernel")]
    if rows % 8 == 0:
        forms += [("rows8_single", 1, {"CILQR_WARP_ROWS": "8"}, "warp_batch_kernel<8,true,false>"),
                  ("rows8_K5", 5, {"CILQR_WARP_ROWS": "8"}, "warp_batch_kernel<8,true,false>")]
    return forms


def _windows(n, K):
    """Index windows of K frames that together visit every pose: consecutive, the last one wrapping round."""
    return [[(a + t) % n for t in range(K)] for a in range(0, n, K)]


def _polygons(dg):
    """Two quadrilaterals in the destination frame: one turned, inside the map; one across the far edge (row 0, x = pos + len/2)."""
    def quad(cx, cy, hx, hy, a):
        p = np.array([(hx, hy), (hx, -hy), (-hx, -hy), (-hx, hy)])
        return np.stack([cx + math.cos(a) * p[:, 0] - math.sin(a) * p[:, 1], cy + math.sin(a) * p[:, 0] + math.cos(a) * p[:, 1]], 1)
    return np.stack([quad(dg.pos_x - 0.2 * dg.len_x, dg.pos_y + 0.1 * dg.len_y, 0.12 * dg.len_x, 0.2 * dg.len_y, 0.4),
                     quad(dg.pos_x + 0.5 * dg.len_x, dg.pos_y - 0.2 * dg.len_y, 0.08 * dg.len_x, 0.15 * dg.len_y, 0.0)])


# ------------------------------------------------------------------------------------------------------------ without a GPU
def test_row_classes_and_forms_reach_all_eight_instantiations(oracle):
    """The destination maps have the row counts the launchers branch on, the tiled kernel's size condition holds for every case,
    and the forms of the three row classes name all eight instantiations."""
    for table, want_rows in ((DST_01, (68, 72, 66)), (DST_SAME_RES, (36, 32, 33)), (DST_EDGE, (44, 40, 42))):
        got = [oracle.map_geom(*g).rows for g in table.values()]
        assert tuple(got) == want_rows == tuple(table)
        assert [(r % 4 == 0, r % 8 == 0) for r in got] == [(True, False), (True, True), (False, False)]
    reached = set()
    for case in CASES + NONFINITE_CASES:
        sg, dg = case.geoms(oracle)
        assert _tile_fits(sg, dg), case.name
        assert 500 <= dg.rows * dg.cols <= 5000, case.name  # a few thousand cells at the most
        reached |= {f[3] for f in _forms(dg.rows)}
        reached.add("warp_kernel<true,false>" if dg.rows % 4 else "warp_batch_kernel<4,false,true>")
        for _, K, _, _ in _forms(dg.rows):
            assert sorted({k for w in _windows(len(case.poses), K) for k in w}) == list(range(len(case.poses)))
    assert reached == {"warp_kernel<false,false>", "warp_kernel<false,true>", "warp_kernel<true,false>", "warp_batch_kernel<4,false,false>",
                       "warp_batch_kernel<4,true,false>", "warp_batch_kernel<4,false,true>", "warp_batch_kernel<8,true,false>", "warp_tile_kernel"}


def test_inputs_reach_the_seam(oracle):
    """Conditions on the INPUTS, from the oracle's arithmetic alone: the share of destination cells whose source quotient lies
    within tol of an integer in x or y.  Aligned: >= 0.4 at 1e-12 (0.50 measured).  Far: >= 0.4 at 1e-7 (one ulp at 4e6 m is
    2e-9 cells), and >= 0.4 in x and in y separately (0.48 ... 0.52 measured).  Same resolution: every cell (>= 0.99 held).  The generic control pose: none at 1e-9."""
    for case in CASES:
        sg, dg = case.geoms(oracle)
        kind = case.name.rsplit("_", 1)[0]
        for pose in case.poses:
            share = boundary_share(sg, dg, pose, 1e-7 if kind == "far" else 1e-12)
            print("%s %r: share %.3f" % (case.name, pose, share))
            if kind == "aligned" and pose != CONTROL:
                assert share >= 0.4, (case.name, pose, share)
            if kind == "far" and pose in FAR_ALIGNED:
                assert share >= 0.4, (case.name, pose, share)
                qx, qy, _, _ = quotients(sg, dg, pose)  # and in each axis on its own (see FAR_ALIGNED)
                each = [float(np.mean(np.abs(q - np.rint(q)) < 1e-7)) for q in (qx, qy)]
                assert min(each) >= 0.4, (case.name, pose, each)
            if kind == "same_res":
                assert share >= 0.99, (case.name, pose, share)
        if kind == "aligned":
            assert boundary_share(sg, dg, CONTROL, 1e-9) == 0.0
        if kind == "edge":  # the map's own edges are boundary integers: cells sit exactly on quotient 0 and on quotient rows
            qx, qy, _, _ = quotients(sg, dg, EDGE_POSES[0])
            assert (qx == 0.0).any() and (qx == float(sg.rows)).any() and (qy == 0.0).any() and (qy == float(sg.cols)).any()
            w, oob = oracle.warp(case.layer("ident", oracle), sg, dg, *EDGE_POSES[0])
            assert 0 < oob < dg.rows * dg.cols and int(np.isnan(w).sum()) == oob
    # a batch mixes aligned and generic frames: every window of every batched form of the aligned and far cases holds both kinds
    for poses, generic in ((ALIGNED + [CONTROL], {CONTROL}), (FAR_ALIGNED + FAR_GENERIC, set(FAR_GENERIC))):
        for K in (2, 3, 5):
            kinds = [{poses[k] in generic for k in w} for w in _windows(len(poses), K)]
            assert any(k == {True, False} for k in kinds), (K, kinds)


def test_oracle_on_non_finite_poses(oracle):
    """What the GPU forms are held to for vx = NaN, vy = +inf, theta = NaN: every cell NaN except the bbox overrides, every cell
    counted out of range."""
    for case in NONFINITE_CASES:
        dg = case.geoms(oracle)[1]
        bbox = case.layer("bbox", oracle)
        for pose in NONFINITE:
            for with_bbox in (False, True):
                dst, oob = want(oracle, case, pose, "holed", with_bbox)
                assert oob == dg.rows * dg.cols
                over = (bbox > 90.0) if with_bbox else np.zeros(bbox.shape, dtype=bool)
                assert np.isnan(dst[~over]).all() and np.array_equal(dst[over], bbox[over]) and (over.sum() > 0) == with_bbox


SHRUNK_SRC = (12.0, 10.0, 0.5, 0.5, -0.5)  # 24 x 20 cells; len_x then set to 21 cells' worth and len_y to 18
SHRUNK_DST = {40: (20.0, 12.0, 0.5, 1.0, 1.0), 42: (21.0, 12.0, 0.5, 1.0, 1.0)}
SHRUNK_POSES = [(0.5, 0.5, 0.7), (0.3, -0.2, 0.0), (0.3, -0.2, 2.0)]


def shrunk(mod, x=True, y=True):
    g = mod.map_geom(*SHRUNK_SRC)
    assert (g.rows, g.cols) == (24, 20)
    if x:
        g.len_x = 21 * g.res
    if y:
        g.len_y = 18 * g.res
    return g


def test_shrunk_source_lengths_make_the_two_in_map_tests_disagree(oracle):
    """Why equality is required.  On a source geometry with len < size * res the reference's two tests part: cells exist whose
    index is inside the map (0 <= trunc(q) < size, all the estimate looks at) while t >= len, which the reference — and the
    oracle, and the kernels' exact path — call out of range.  With len == size * res there is no such cell."""
    for dgeo in SHRUNK_DST.values():
        dg = oracle.map_geom(*dgeo)
        for pose in SHRUNK_POSES:
            for sg, expect_some in ((shrunk(oracle), True), (oracle.map_geom(*SHRUNK_SRC), False)):
                qx, qy, x_og, y_og = quotients(sg, dg, pose)
                tx = -1.0 * ((x_og - sg.pos_x) - 0.5 * sg.len_x)
                ty = -1.0 * ((y_og - sg.pos_y) - 0.5 * sg.len_y)
                by_index = (qx > -1.0) & (qy > -1.0) & (np.trunc(qx) < sg.rows) & (np.trunc(qy) < sg.cols) & (tx >= 0.0) & (ty >= 0.0)
                part = by_index & ((tx >= sg.len_x) | (ty >= sg.len_y))
                dst, oob = oracle.warp(ident_source(sg.rows, sg.cols), sg, dg, *pose)
                print("%s %r shrunk=%s: %d of %d cells inside by index, outside by length" % (dgeo, pose, expect_some, part.sum(), part.size))
                assert np.isnan(dst[part]).all()  # the oracle sides with the length test
                assert (part.sum() > 0) == expect_some
                assert oob == int(np.isnan(dst).sum())


class _NoDevice:
    """Stands in for a Solver in calls that must fail on an argument: the handle is never dereferenced."""
    _h = C.c_void_p(8)


def _entry_points(cilqr, s, stream, src, sg, dst, dg, unc, oob=0):
    """Every entry that hands a source geometry to a warp launcher, as closures over device addresses (or a host array for the
    host form)."""
    S, pose, poses, sig = cilqr.Solver, (0.5, 0.5, 0.7), np.array([[0.5, 0.5, 0.7], [0.3, -0.2, 0.0]]), (0.16, 0.16, 0.017)
    polys = _polygons(dg)
    return {
        "cilqr_warp_costmap_device": lambda: S.warp_costmap_device(s, stream, src, sg, dst, dg, *pose, n_oob=oob),
        "cilqr_warp_costmap_batch_device": lambda: S.warp_costmap_batch_device(s, stream, src, sg, dst, dg, poses, n_oob=oob),
        "cilqr_warp_costmap_batch_device K=1": lambda: S.warp_costmap_batch_device(s, stream, src, sg, dst, dg, poses[:1], n_oob=oob),
        "cilqr_warp_costmap_polygons_device": lambda: S.warp_costmap_polygons_device(s, stream, src, sg, dst, dg, *pose, polys, n_oob=oob),
        "cilqr_costmap_frame_device": lambda: S.costmap_frame_device(s, stream, src, sg, dg, *pose, *sig, dst, unc, n_oob=oob),
        "cilqr_costmap_frame_batch_device": lambda: S.costmap_frame_batch_device(s, stream, src, sg, dg, poses, *sig, dst, unc, n_oob=oob),
        "cilqr_costmap_frame_batch_device K=1": lambda: S.costmap_frame_batch_device(s, stream, src, sg, dg, poses[:1], *sig, dst, unc, n_oob=oob),
        "cilqr_costmap_frame_polygons_device": lambda: S.costmap_frame_polygons_device(s, stream, src, sg, dg, *pose, polys, *sig, dst, unc, n_oob=oob),
    }


def test_source_lengths_are_checked_before_the_handle_is_touched(cilqr):
    """Every entry point returns CILQR_ERR_ARG for a source geometry whose len is not (double)size * res — shorter, longer or NaN,
    in x or in y, the message naming the field — with a handle that cannot be dereferenced and addresses that are no memory:
    nothing is enqueued, nothing read."""
    fake = _NoDevice()
    bad = {"len_x": [shrunk(cilqr, y=False)], "len_y": [shrunk(cilqr, x=False)]}
    for field in ("len_x", "len_y"):
        for value in (lambda g: getattr(g, field) + g.res, lambda g: NAN, lambda g: float(np.nextafter(getattr(g, field), 0.0))):
            g = cilqr.map_geom(*SHRUNK_SRC)
            setattr(g, field, value(g))
            bad[field].append(g)
    both = shrunk(cilqr)
    for dgeo in SHRUNK_DST.values():
        dg = cilqr.map_geom(*dgeo)
        for field, geoms in list(bad.items()) + [("len_x", [both])]:
            for sg in geoms:
                calls = _entry_points(cilqr, fake, 16, 32, sg, 48, dg, 64)
                calls["cilqr_warp_costmap"] = lambda: cilqr.Solver.warp_costmap(fake, np.zeros((sg.rows, sg.cols), dtype=np.float32), sg, dg, 0.5, 0.5, 0.7)
                for name, call in calls.items():
                    with pytest.raises(cilqr.CilqrError) as e:
                        call()
                    msg = str(e.value)
                    assert "cilqr error -1:" in msg and field in msg and "source geometry" in msg, (name, msg)


EXTRA_SET_GEOMETRIES = [[10.05, 10.05, 0.1, 0.0, 0.0], [6.6, 6.6, 0.1, 2.0, -1.0], [204.8, 204.8, 0.2, 3.0, -2.0], [10.05, 6.6, 0.1, -4.0, 9.0]]


def test_set_geometries_satisfy_the_rule(cilqr):
    """cilqr_map_geom_set writes the very bits the rule asks for — the golden geometries of the reference's setGeometry and lengths
    that are no multiple of the resolution."""
    args = [c["args"] for c in load_golden("ref_gridmap.json")["geometry"]] + EXTRA_SET_GEOMETRIES
    for a in args + [SRC_NEAR, SRC_FAR, SRC_SAME_RES, SRC_EDGE, SHRUNK_SRC]:
        g = cilqr.map_geom(*a)
        assert g.len_x == float(g.rows) * g.res and g.len_y == float(g.cols) * g.res, a



# ------------------------------------------------------------------------------------------------------------ with a GPU
SENTINEL = -7.0
PAD = 64  # floats behind the last frame that no call may write


@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=1, max_horizon=1, max_obstacles=0, device=0)
    yield s
    s.close()


def _flat(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, order="F"))


class _Device:
    """One case's layers on the device and the two warp calls on them."""

    def __init__(self, cilqr, oracle, solver, case):
        import torch
        self.torch, self.solver, self.case = torch, solver, case
        self.dev = torch.device("cuda", 0)
        self.sg, self.dg = case.geoms(cilqr)
        self.cells = self.dg.rows * self.dg.cols
        self.src = {w: torch.from_numpy(_flat(case.layer(w, oracle))).to(self.dev) for w in ("ident", "holed")}
        self.bbox = torch.from_numpy(_flat(case.layer("bbox", oracle))).to(self.dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def buffers(self, K):
        t = self.torch
        return t.full((K * self.cells + PAD,), SENTINEL, dtype=t.float32, device=self.dev), t.full((K + 1,), -1, dtype=t.int64, device=self.dev)

    def frames(self, d_dst, d_oob, K):
        """The K frames as (K, rows, cols) float32 and their counters; nothing behind them was written."""
        self.torch.cuda.synchronize()
        out, oob = d_dst.cpu().numpy(), d_oob.cpu().numpy()
        assert (out[K * self.cells:] == SENTINEL).all() and oob[K] == -1
        return out[:K * self.cells].reshape(K, self.dg.cols, self.dg.rows).transpose(0, 2, 1), oob[:K]

    def warp(self, poses, which, with_bbox):
        """len(poses) == 1: cilqr_warp_costmap_device; more: cilqr_warp_costmap_batch_device."""
        K = len(poses)
        d_dst, d_oob = self.buffers(K)
        bb = self.bbox.data_ptr() if with_bbox else 0
        if K == 1:
            self.solver.warp_costmap_device(self.stream, self.src[which].data_ptr(), self.sg, d_dst.data_ptr(), self.dg, *poses[0], bbox=bb, n_oob=d_oob.data_ptr())
        else:
            self.solver.warp_costmap_batch_device(self.stream, self.src[which].data_ptr(), self.sg, d_dst.data_ptr(), self.dg, np.array(poses), bbox=bb,
                                                  n_oob=d_oob.data_ptr())
        return self.frames(d_dst, d_oob, K)

    def warp_polygons(self, pose, which, polys):
        d_dst, d_oob = self.buffers(1)
        self.solver.warp_costmap_polygons_device(self.stream, self.src[which].data_ptr(), self.sg, d_dst.data_ptr(), self.dg, *pose, polys, n_oob=d_oob.data_ptr())
        return self.frames(d_dst, d_oob, 1)


def _run_every_form(cilqr, oracle, solver, monkeypatch, case):
    """Every pose of the case through every form of its row class, without a bbox layer on the cell-identifying source and with
    one on the holed source: each frame equal to the oracle's and to the single-frame call's, counters included."""
    d = _Device(cilqr, oracle, solver, case)
    poses, n = case.poses, len(case.poses)
    for which, with_bbox in (("ident", False), ("holed", True)):
        singles = {}
        for name, K, env, _ in _forms(d.dg.rows):
            print("%s: %s, %s source, bbox %s" % (case.name, name, which, with_bbox), flush=True)
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                for window in _windows(n, K):
                    got, oob = d.warp([poses[k] for k in window], which, with_bbox)
                    for f, k in enumerate(window):
                        w_dst, w_oob = want(oracle, case, poses[k], which, with_bbox)
                        if not np.array_equal(got[f], w_dst, equal_nan=True):
                            differ = int((~((got[f] == w_dst) | (np.isnan(got[f]) & np.isnan(w_dst)))).sum())
                            raise AssertionError("%s %s %s %r: %d cells differ from the oracle" % (case.name, name, which, poses[k], differ))
                        assert int(oob[f]) == w_oob, (case.name, name, which, poses[k], int(oob[f]), w_oob)
                        if name == "single":
                            singles[k] = got[f].copy()
                        assert np.array_equal(got[f].view(np.int32), singles[k].view(np.int32)), (case.name, name, which, poses[k])
        assert sorted(singles) == list(range(n))
    # the polygon forms against the layer forms given the rasterised layer, and against the oracle given it
    polys = _polygons(d.dg)
    layer = solver.rasterize_polygons(d.dg, polys)
    assert (layer[0, :] == 100.0).any() and (layer[d.dg.rows // 2:, :] == 100.0).any() and np.isnan(layer).any()  # across the far edge; inside; not everywhere
    d.bbox = d.torch.from_numpy(_flat(layer)).to(d.dev)
    osg, odg = case.geoms(oracle)
    for pose in poses:
        got, oob = d.warp_polygons(pose, "ident", polys)
        by_layer, oob_layer = d.warp([pose], "ident", True)
        w_dst, w_oob = oracle.warp(case.layer("ident", oracle), osg, odg, *pose, bbox=layer)
        assert np.array_equal(got[0], w_dst, equal_nan=True) and int(oob[0]) == w_oob, (case.name, "polygons", pose)
        assert np.array_equal(got[0].view(np.int32), by_layer[0].view(np.int32)) and int(oob[0]) == int(oob_layer[0]), (case.name, "polygons", pose)
        assert (got[0][layer == 100.0] == 100.0).all()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_seam_cases_on_every_kernel_form(cilqr, oracle, solver, monkeypatch, case):
    """Aligned, far, same-resolution and map-edge inputs at 68/72/66-row class destinations through all eight instantiations
    (module docstring), bit for bit against oracle.warp."""
    _run_every_form(cilqr, oracle, solver, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", NONFINITE_CASES, ids=[c.name for c in NONFINITE_CASES])
def test_non_finite_poses_on_every_kernel_form(cilqr, oracle, solver, monkeypatch, case):
    """vx = NaN, vy = +inf, theta = NaN as single frames and as frames among finite ones, in every form: all cells NaN except the
    bbox overrides and n_oob the cell count (test_oracle_on_non_finite_poses holds the oracle to that), the finite frames beside
    them what they are alone.  (warp_tile_kernel's staging box once passed a NaN pose for finite and read the source out of bounds:
    profiles/r20_warp_seams.txt.)"""
    d = _run_every_form(cilqr, oracle, solver, monkeypatch, case)
    got, oob = d.warp([NONFINITE[2]], "ident", False)  # once more in the open, not through the oracle
    assert np.isnan(got[0]).all() and int(oob[0]) == d.cells


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def _ulp32(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aligned_68", "far_66", "aligned_72", "far_68"])
def test_frame_entry_points_on_seam_inputs(cilqr, oracle, solver, name):
    """cilqr_costmap_frame_device and cilqr_costmap_frame_batch_device on aligned and far inputs (holed source, bbox layer): the
    vehicle layer of every frame is the oracle's warp bit for bit and n_oob its count; batch and single frames agree bit for bit
    in all outputs; blur and OccupancyGrid of frame 0 under the bounds of test_frame_batch.test_frame_batch_equals_single_frames
    (NaN masks equal, at most 1 float32 ulp, at least 99.9 % bit-equal, the grid that of the layer)."""
    import torch
    case = next(c for c in CASES if c.name == name)
    d = _Device(cilqr, oracle, solver, case)
    poses, K, cells, sig = np.array(case.poses), len(case.poses), d.cells, (0.16, 0.16, 0.017)
    assert K >= 4

    def buffers():
        return (torch.full((K * cells + PAD,), SENTINEL, dtype=torch.float32, device=d.dev), torch.full((K * cells + PAD,), SENTINEL, dtype=torch.float32, device=d.dev),
                torch.full((K * cells + PAD,), -100, dtype=torch.int8, device=d.dev), torch.full((K + 1,), -1, dtype=torch.int64, device=d.dev))

    b_veh, b_unc, b_occ, b_oob = buffers()
    s_veh, s_unc, s_occ, s_oob = buffers()
    src = d.src["holed"].data_ptr()
    solver.costmap_frame_batch_device(d.stream, src, d.sg, d.dg, poses, *sig, b_veh.data_ptr(), b_unc.data_ptr(), b_occ.data_ptr(), bbox=d.bbox.data_ptr(),
                                      n_oob=b_oob.data_ptr())
    for k in range(K):
        solver.costmap_frame_device(d.stream, src, d.sg, d.dg, *poses[k], *sig, s_veh.data_ptr() + 4 * k * cells, s_unc.data_ptr() + 4 * k * cells,
                                    s_occ.data_ptr() + k * cells, bbox=d.bbox.data_ptr(), n_oob=s_oob.data_ptr() + 8 * k)
    torch.cuda.synchronize()
    for what, b, s in (("vehicle", b_veh, s_veh), ("uncertainty", b_unc, s_unc), ("occupancy", b_occ, s_occ), ("n_oob", b_oob, s_oob)):
        assert np.array_equal(_bits(b), _bits(s)), (name, what)  # batch against single frames, pads included
    veh, unc, occ, oob = b_veh.cpu().numpy(), b_unc.cpu().numpy(), b_occ.cpu().numpy(), b_oob.cpu().numpy()
    assert (veh[K * cells:] == SENTINEL).all() and (unc[K * cells:] == SENTINEL).all() and (occ[K * cells:] == -100).all() and oob[K] == -1
    osg, odg = case.geoms(oracle)
    for k in range(K):
        w_dst, w_oob = want(oracle, case, case.poses[k], "holed", True)
        assert np.array_equal(veh[k * cells:(k + 1) * cells], w_dst.reshape(-1, order="F"), equal_nan=True), (name, k)
        assert int(oob[k]) == w_oob, (name, k)
    th = case.poses[0][2]
    w_veh, _ = want(oracle, case, case.poses[0], "holed", True)
    w_unc, _, _ = oracle.blur(w_veh, odg, np.sin(th), np.cos(th), *sig, threads=min(16, oracle.max_threads()))
    w_unc, f_unc = w_unc.reshape(-1, order="F"), unc[:cells]
    fin = ~np.isnan(w_unc)
    assert np.array_equal(np.isnan(f_unc), ~fin)
    ulp = _ulp32(f_unc[fin], w_unc[fin])
    print("%s frame 0 blur against the oracle: max ulp %d, bit-equal %.5f" % (name, ulp.max(), (ulp == 0).mean()))
    assert ulp.max() <= 1 and (ulp == 0).mean() >= 0.999
    assert np.array_equal(occ[:cells], oracle.layer_to_occupancy(f_unc, 0.0, 100.0))
    same = np.ones(cells, dtype=bool)
    same[fin] = ulp == 0
    assert np.array_equal(occ[:cells][::-1][same], oracle.layer_to_occupancy(w_unc, 0.0, 100.0)[::-1][same])


@pytest.mark.gpu
def test_shrunk_source_geometry_is_rejected_and_the_handle_stays_usable(cilqr, oracle, solver):
    """With a live handle: every entry point refuses the shrunk source geometry, the sentinel-filled destination, second layer and
    counters are untouched, and a valid warp on the same handle afterwards is the oracle's."""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    good, osg = cilqr.map_geom(*SHRUNK_SRC), oracle.map_geom(*SHRUNK_SRC)
    src_h = ident_source(good.rows, good.cols)
    d_src = torch.from_numpy(_flat(src_h)).to(dev)
    for dgeo in SHRUNK_DST.values():
        dg, odg = cilqr.map_geom(*dgeo), oracle.map_geom(*dgeo)
        cells = dg.rows * dg.cols
        d_dst = torch.full((2 * cells,), SENTINEL, dtype=torch.float32, device=dev)
        d_unc = torch.full((2 * cells,), SENTINEL, dtype=torch.float32, device=dev)
        d_oob = torch.full((2,), -1, dtype=torch.int64, device=dev)
        for sg, field in ((shrunk(cilqr), "len_x"), (shrunk(cilqr, x=False), "len_y")):
            calls = _entry_points(cilqr, solver, stream, d_src.data_ptr(), sg, d_dst.data_ptr(), dg, d_unc.data_ptr(), d_oob.data_ptr())
            calls["cilqr_warp_costmap"] = lambda: solver.warp_costmap(src_h, sg, dg, 0.5, 0.5, 0.7)
            for name, call in calls.items():
                with pytest.raises(cilqr.CilqrError) as e:
                    call()
                assert "cilqr error -1:" in str(e.value) and field in str(e.value), (name, str(e.value))
        torch.cuda.synchronize()
        assert (d_dst == SENTINEL).all().item() and (d_unc == SENTINEL).all().item() and (d_oob == -1).all().item()
        for pose in SHRUNK_POSES:
            w_dst, w_oob = oracle.warp(src_h, osg, odg, *pose)
            got, oob = solver.warp_costmap(src_h, good, dg, *pose)
            assert np.array_equal(got, w_dst, equal_nan=True) and oob == w_oob and 0 < oob < cells, (dgeo, pose)
            solver.warp_costmap_device(stream, d_src.data_ptr(), good, d_dst.data_ptr(), dg, *pose, n_oob=d_oob.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(d_dst.cpu().numpy()[:cells].reshape(dg.cols, dg.rows).T, w_dst, equal_nan=True) and int(d_oob[0].item()) == w_oob
            d_dst.fill_(SENTINEL)


@pytest.mark.gpu
def test_set_geometries_are_accepted_as_sources(cilqr, oracle, solver):
    """A geometry from cilqr_map_geom_set is never rejected: the golden geometries and lengths that are no multiple of the
    resolution as sources of a small warp, which is the oracle's."""
    args = [c["args"] for c in load_golden("ref_gridmap.json")["geometry"]] + EXTRA_SET_GEOMETRIES
    for a in args:
        sg, osg = cilqr.map_geom(*a), oracle.map_geom(*a)
        res = a[2]
        dgeo = (16 * res, 12 * res, res / 2, a[3] + 0.3 * res, a[4])
        dg, odg = cilqr.map_geom(*dgeo), oracle.map_geom(*dgeo)
        src = ident_source(sg.rows, sg.cols)
        pose = (0.1 * res, -0.2 * res, 0.0)
        got, oob = solver.warp_costmap(src, sg, dg, *pose)
        w_dst, w_oob = oracle.warp(src, osg, odg, *pose)
        assert np.array_equal(got, w_dst, equal_nan=True) and oob == w_oob and not np.isnan(got).all(), a
