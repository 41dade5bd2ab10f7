"""Obstacle bounding boxes on the device: cilqr_boxes_to_polygons (host), cilqr_rasterize_polygons(_device) and the warp / frame
calls that take the polygons in place of a bbox layer.

Reference: LocalCostmap::bondingBoxHandle (M/src/local_costmap.cpp:860-922) over grid_map's PolygonIterator, whose cells are
those of the polygon's bounding submap with Polygon::isInside(centre) (G/grid_map_core/src/Polygon.cpp:32-44).  Every comparison
here is exact: float32 layers as bit patterns, doubles with ==.
"""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import load_golden

NAN_BITS = np.float32("nan").view(np.uint32)
ERR_ARG = -1


# ---------------------------------------------------------------------------------------------- restatements of the reference
def boxes_to_polygons_restated(boxes, own_x, own_y, own_yaw, inflate, max_distance):
    """bondingBoxHandle's corner arithmetic (M/src/local_costmap.cpp:866-913) in plain Python floats and math.sin / math.cos."""
    out = []
    for x, y, yaw, size_x, size_y in boxes:
        distance = math.sqrt((x - own_x) * (x - own_x) + (y - own_y) * (y - own_y))
        if not distance <= max_distance:
            continue
        hx, hy = (size_x + inflate) / 2.0, (size_y + inflate) / 2.0
        poly = []
        for cx, cy in ((hx, hy), (hx, -hy), (-hx, -hy), (-hx, hy)):
            gx = math.cos(yaw) * cx - math.sin(yaw) * cy + x
            gy = math.sin(yaw) * cx + math.cos(yaw) * cy + y
            lx = math.cos(own_yaw) * (gx - own_x) + math.sin(own_yaw) * (gy - own_y)
            ly = -math.sin(own_yaw) * (gx - own_x) + math.cos(own_yaw) * (gy - own_y)
            poly.append((lx, ly))
        out.append(poly)
    return np.array(out, dtype=np.float64).reshape(-1, 4, 2)


def inside_mask(cx, cy, polygons):
    """Polygon::isInside (Polygon.cpp:32-44) of EVERY cell centre (cx[i], cy[j]) for every polygon, brute force: no bounding box,
    no early exit.  numpy's elementwise double arithmetic is IEEE and unfused, in the reference's order."""
    mask = np.zeros((cx.size, cy.size), dtype=bool)
    px = cx[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        for poly in polygons:
            cross = np.zeros((cx.size, cy.size), dtype=np.int32)
            V = len(poly)
            j = V - 1
            for i in range(V):
                xi, yi = float(poly[i][0]), float(poly[i][1])
                xj, yj = float(poly[j][0]), float(poly[j][1])
                straddle = (yi > cy) != (yj > cy)
                at = (xj - xi) * (cy - yi) / (yj - yi) + xi
                cross += straddle[None, :] & (px < at[None, :])
                j = i
            mask |= (cross % 2).astype(bool)
    return mask


def cell_centres(oracle, args):
    """Centres of the rows (x) and columns (y) of the map setGeometry(Length(args[0], args[1]), args[2], Position(args[3], args[4]))
    gives: from the live reference where it was built (getPosition is separable: rows + cols calls), else from the formula
    ref_gridmap.json pins (test_oracle.test_gridmap_vs_reference)."""
    g = oracle.map_geom(*args)
    fx = np.array([(g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) + g.res * float(-i) for i in range(g.rows)])
    fy = np.array([(g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) + g.res * float(-j) for j in range(g.cols)])
    L = oracle.ref_lib("gridmap")
    if L is None:
        return fx, fy
    x, y = C.c_double(), C.c_double()
    a = [C.c_double(v) for v in args]
    lx = np.zeros(g.rows)
    ly = np.zeros(g.cols)
    for i in range(g.rows):
        assert L.ref_get_position(*a, i, 0, C.byref(x), C.byref(y)) == 1
        lx[i] = x.value
    for j in range(g.cols):
        assert L.ref_get_position(*a, 0, j, C.byref(x), C.byref(y)) == 1
        ly[j] = y.value
    assert np.array_equal(lx, fx) and np.array_equal(ly, fy)
    return lx, ly


def expected_layer(mask, value=100.0, background=None):
    out = np.full(mask.shape, np.nan, dtype=np.float32) if background is None else np.array(background, dtype=np.float32)
    out = np.asfortranarray(out)
    out[mask] = np.float32(value)
    return out


def same_bits(a, b):
    a, b = np.asfortranarray(a, dtype=np.float32), np.asfortranarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- scenes
GEOMETRIES = {
    "1024x1024": (102.4, 102.4, 0.1, 10.0, 0.0),
    "300x200": (60.0, 40.0, 0.2, 25.0, -7.5),
    "513x207": (51.3, 20.7, 0.1, 15.0, 0.0),
    "8x5": (8.0, 5.0, 1.0, 0.0, 0.0),
}
SHAPES = {"1024x1024": (1024, 1024), "300x200": (300, 200), "513x207": (513, 207), "8x5": (8, 5)}


def scene_boxes(args, seed, n=70):
    """n boxes (x, y, yaw, size_x, size_y) in the planning frame around a map of the vehicle at OWN (heading 0).  Every seventh box
    is axis-aligned with centre and half sizes on the map's 0.1 m lattice, so that its edges run through cell centres; two more
    boxes lie across the map's edge and wholly outside it."""
    len_x, len_y, res, pos_x, pos_y = args
    rng = np.random.default_rng(seed)
    big = res >= 1.0
    boxes = []
    for k in range(n):
        x = OWN[0] + pos_x + rng.uniform(-0.5 * len_x - 2.0, 0.5 * len_x + 2.0)
        y = OWN[1] + pos_y + rng.uniform(-0.5 * len_y - 2.0, 0.5 * len_y + 2.0)
        if k % 7 == 0:  # aligned: the inflated half sizes (size + 0.2) / 2 are odd multiples of 0.05, the centre a multiple of 0.1
            sx = 0.1 * (2 * int(rng.integers(5, 25)) + 1) - 0.2
            sy = 0.1 * (2 * int(rng.integers(3, 12)) + 1) - 0.2
            boxes.append((round(x, 1), round(y, 1), 0.0, sx, sy))
        else:
            boxes.append((x, y, rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 3.0) if big else rng.uniform(1.5, 6.0),
                          rng.uniform(0.4, 2.0) if big else rng.uniform(0.8, 2.5)))
    boxes.append((OWN[0] + pos_x + 0.5 * len_x, OWN[1] + pos_y + 0.1 * len_y, 0.4, 4.0, 2.0))        # across the far edge
    boxes.append((OWN[0] + pos_x + 0.5 * len_x + 6.0, OWN[1] + pos_y, -0.3, 4.5, 1.9))               # wholly outside
    return np.array(boxes, dtype=np.float64)


OWN = (123.4, -56.7)


def scene_polygons(cilqr, args, seed):
    polys = cilqr.boxes_to_polygons(scene_boxes(args, seed), OWN[0], OWN[1], 0.0)
    assert polys.shape[0] >= 60
    return polys


def outside_counts(args, polys):
    """(polygons partly outside the map's rectangle, polygons wholly outside it)"""
    len_x, len_y, _, pos_x, pos_y = args
    x0, x1, y0, y1 = pos_x - 0.5 * len_x, pos_x + 0.5 * len_x, pos_y - 0.5 * len_y, pos_y + 0.5 * len_y
    partly = wholly = 0
    for p in polys:
        inside = (p[:, 0] > x0) & (p[:, 0] < x1) & (p[:, 1] > y0) & (p[:, 1] < y1)
        disjoint = p[:, 0].max() < x0 or p[:, 0].min() > x1 or p[:, 1].max() < y0 or p[:, 1].min() > y1
        wholly += bool(disjoint)
        partly += bool(inside.any() and not inside.all())
    return partly, wholly


# ---------------------------------------------------------------------------------------------- without a GPU
def test_boxes_to_polygons_matches_restatement(cilqr):
    rng = np.random.default_rng(20240607)
    own_x, own_y = 12.5, -3.25
    n = 240
    boxes = np.zeros((n, 5))
    r = rng.uniform(0.0, 130.0, n)  # about a quarter lie beyond 100 m
    phi = rng.uniform(-math.pi, math.pi, n)
    boxes[:, 0] = own_x + r * np.cos(phi)
    boxes[:, 1] = own_y + r * np.sin(phi)
    boxes[:, 2] = rng.uniform(-math.pi, math.pi, n)  # negative yaws among them
    boxes[:, 3] = rng.uniform(0.5, 12.0, n)
    boxes[:, 4] = rng.uniform(0.3, 3.0, n)
    boxes[0, :3] = (own_x + 60.0, own_y + 80.0, -0.75)  # exactly at max_distance: 60^2 + 80^2 = 100^2, all exact in binary
    boxes[1, :3] = (own_x + 60.0, np.nextafter(own_y + 80.0, np.inf), 0.3)  # the next double beyond it
    boxes[2, :3] = (own_x, own_y, -3.0)
    assert (boxes[:, 2] < 0).sum() > 50 and (r > 100.0).sum() > 20
    for own_yaw in (0.0, -0.7, 2.1, -3.1):
        want = boxes_to_polygons_restated(boxes, own_x, own_y, own_yaw, 0.2, 100.0)
        got = cilqr.boxes_to_polygons(boxes, own_x, own_y, own_yaw)
        assert 100 < want.shape[0] < n  # some kept, some dropped
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the box at exactly max_distance is kept, the next double is not
    assert cilqr.boxes_to_polygons(boxes[:2], own_x, own_y, 0.0).shape[0] == 1
    assert cilqr.boxes_to_polygons(boxes[1:2], own_x, own_y, 0.0).shape[0] == 0
    # other inflations and distances go through the same expressions
    want = boxes_to_polygons_restated(boxes, own_x, own_y, 0.4, 0.35, 42.0)
    got = cilqr.boxes_to_polygons(boxes, own_x, own_y, 0.4, inflate=0.35, max_distance=42.0)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert cilqr.boxes_to_polygons(np.zeros((0, 5)), 0.0, 0.0, 0.0).shape == (0, 4, 2)


def test_polygon_argument_errors_do_not_need_a_device(cilqr):
    L = cilqr.lib()
    dp = C.POINTER(C.c_double)
    g = cilqr.map_geom(8.0, 5.0, 1.0, 0.0, 0.0)
    d = C.c_double
    square = np.array([[-1.0, 1.5], [1.0, 1.5], [1.0, -1.5], [-1.0, -1.5]])
    many = np.zeros((1025, 4, 2))
    no_handle = C.c_void_p()
    layer = np.zeros(40, dtype=np.float32).ctypes.data_as(C.c_void_p)

    # cilqr_boxes_to_polygons
    kept = C.c_int32(7)
    box = np.array([1.0, 2.0, 0.1, 4.0, 2.0])
    out = np.zeros(8)
    assert L.cilqr_boxes_to_polygons(-1, box.ctypes.data_as(dp), d(0), d(0), d(0), d(0.2), d(100), out.ctypes.data_as(dp), C.byref(kept)) == ERR_ARG
    assert L.cilqr_boxes_to_polygons(1, box.ctypes.data_as(dp), d(0), d(0), d(0), d(0.2), d(100), out.ctypes.data_as(dp), None) == ERR_ARG
    assert L.cilqr_boxes_to_polygons(1, None, d(0), d(0), d(0), d(0.2), d(100), out.ctypes.data_as(dp), C.byref(kept)) == ERR_ARG
    assert L.cilqr_boxes_to_polygons(1, box.ctypes.data_as(dp), d(0), d(0), d(0), d(0.2), d(100), None, C.byref(kept)) == ERR_ARG
    assert L.cilqr_boxes_to_polygons(1, box.ctypes.data_as(dp), d(0), d(0), d(0), d(0.2), d(100), out.ctypes.data_as(dp), C.byref(kept)) == 0
    assert kept.value == 1

    def raster_dev(n, V, v, geom=g):
        return L.cilqr_rasterize_polygons_device(no_handle, None, C.byref(geom) if geom is not None else None, n, V,
                                                 v.ctypes.data_as(dp) if v is not None else None, C.c_float(100.0), 1, layer)

    def raster_host(n, V, v, geom=g):
        return L.cilqr_rasterize_polygons(no_handle, C.byref(geom) if geom is not None else None, n, V,
                                          v.ctypes.data_as(dp) if v is not None else None, C.c_float(100.0), 1, layer)

    def warp(n, V, v, geom=g):
        return L.cilqr_warp_costmap_polygons_device(no_handle, None, layer, C.byref(g), layer, C.byref(geom) if geom is not None else None,
                                                    d(0), d(0), d(0), n, V, v.ctypes.data_as(dp) if v is not None else None, None)

    def frame(n, V, v, geom=g):
        return L.cilqr_costmap_frame_polygons_device(no_handle, None, layer, C.byref(g), C.byref(geom) if geom is not None else None, d(0),
                                                     d(0), d(0), n, V, v.ctypes.data_as(dp) if v is not None else None, d(0.1), d(0.1),
                                                     d(0.01), layer, layer, None, None)

    bad_geom = cilqr.map_geom(8.0, 5.0, 1.0, 0.0, 0.0)
    bad_geom.rows = 0
    for call in (raster_dev, raster_host, warp, frame):
        for bad_value in (float("nan"), float("inf"), float("-inf")):
            v = square.copy()
            v[2, 1] = bad_value
            assert call(1, 4, v) == ERR_ARG
            assert b"not finite" in L.cilqr_last_error()
        assert call(-1, 4, square) == ERR_ARG and b"n_polygons" in L.cilqr_last_error()
        assert call(1025, 4, many) == ERR_ARG and b"n_polygons" in L.cilqr_last_error()
        assert call(1, 2, square) == ERR_ARG and b"n_vertices" in L.cilqr_last_error()
        assert call(1, 17, np.zeros((1, 17, 2))) == ERR_ARG and b"n_vertices" in L.cilqr_last_error()
        assert call(1, 4, None) == ERR_ARG and b"null vertices" in L.cilqr_last_error()
        assert call(1, 4, square, None) == ERR_ARG and b"null geometry" in L.cilqr_last_error()
        assert call(1, 4, square, bad_geom) == ERR_ARG and b"bad geometry" in L.cilqr_last_error()
        assert call(1, 4, square) == ERR_ARG and b"null argument" in L.cilqr_last_error()  # valid polygons, no handle
        assert call(0, 4, None) == ERR_ARG and b"null argument" in L.cilqr_last_error()


def test_polygon_gtest_fixture_is_consistent(oracle):
    """The stored expectations of the reference's PolygonIteratorTest.cpp agree with brute-force isInside over the 8x5 map."""
    gold = load_golden("ref_polygon_gtest.json")
    cx, cy = cell_centres(oracle, gold["geometry"])
    assert (cx.size, cy.size) == (gold["rows"], gold["cols"]) == (8, 5)
    for c in gold["cases"]:
        mask = inside_mask(cx, cy, [c["vertices"]])
        cells = {tuple(ij) for ij in c["cells"]}
        got = {(int(i), int(j)) for i, j in zip(*np.nonzero(mask))}
        assert (got == cells) if c["complete"] else (cells <= got), c["name"]


# ---------------------------------------------------------------------------------------------- with a GPU
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=4, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


def _device_raster(solver, g, polys, value=100.0, clear=True, start=None):
    import torch
    dev = torch.device("cuda", 0)
    if start is None:
        d = torch.full((g.rows * g.cols,), 7.0, dtype=torch.float32, device=dev)  # every cell must be overwritten when clear
    else:
        d = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(start, dtype=np.float32).reshape(-1, order="F")).view(np.int32)).to(dev)
        d = d.view(torch.float32)
    solver.rasterize_polygons_device(torch.cuda.current_stream().cuda_stream, g, polys, d.data_ptr(), value=value, clear=clear)
    torch.cuda.synchronize()
    return d.view(torch.int32).cpu().numpy().view(np.float32).reshape((g.rows, g.cols), order="F"), d


@pytest.mark.gpu
def test_reference_gtest_cases_on_device(cilqr, oracle, solver):
    gold = load_golden("ref_polygon_gtest.json")
    g = cilqr.map_geom(*gold["geometry"])
    assert (g.rows, g.cols) == (8, 5)
    for c in gold["cases"]:
        layer, _ = _device_raster(solver, g, np.array([c["vertices"]]))
        got = {(int(i), int(j)) for i, j in zip(*np.nonzero(layer == 100.0))}
        cells = {tuple(ij) for ij in c["cells"]}
        if c["complete"]:
            assert got == cells, c["name"]
        else:
            assert cells <= got, c["name"]
        assert np.all(np.isnan(layer[layer != 100.0])), c["name"]
    full = next(c for c in gold["cases"] if c["name"] == "FullCover")
    assert len(full["cells"]) == 40


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_random_scenes_match_brute_force(cilqr, oracle, solver, name):
    args = GEOMETRIES[name]
    g = cilqr.map_geom(*args)
    assert (g.rows, g.cols) == SHAPES[name]
    polys = scene_polygons(cilqr, args, seed=sum(map(ord, name)))
    partly, wholly = outside_counts(args, polys)
    assert partly >= 1 and wholly >= 1
    cx, cy = cell_centres(oracle, args)
    mask = inside_mask(cx, cy, polys)
    print("%s: %d polygons, %d cells marked, %d partly / %d wholly outside" % (name, polys.shape[0], int(mask.sum()), partly, wholly))
    if name != "8x5":
        assert mask.sum() >= 1000
    want = expected_layer(mask)
    got, _ = _device_raster(solver, g, polys)
    assert same_bits(got, want)  # value inside, the NaN of a cleared layer elsewhere
    assert np.array_equal(np.isnan(got), ~mask)
    # the host form is the device form
    assert same_bits(solver.rasterize_polygons(g, polys), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1024x1024", "513x207"])
def test_accumulation_leaves_other_cells_untouched(cilqr, oracle, solver, name):
    args = GEOMETRIES[name]
    g = cilqr.map_geom(*args)
    polys = scene_polygons(cilqr, args, seed=11)
    first, second = polys[:30], polys[30:]
    cx, cy = cell_centres(oracle, args)
    m1, m2 = inside_mask(cx, cy, first), inside_mask(cx, cy, second)
    # arbitrary bit patterns underneath (NaNs with payloads among them): clear = 0 must not read-modify-write them
    start = np.random.default_rng(5).integers(0, 2 ** 32, size=(g.rows, g.cols), dtype=np.uint64).astype(np.uint32).view(np.float32)
    start = np.asfortranarray(start)
    got1, _ = _device_raster(solver, g, first, value=55.0, clear=False, start=start)
    want1 = expected_layer(m1, 55.0, background=start)
    assert same_bits(got1, want1)
    got2, _ = _device_raster(solver, g, second, value=100.0, clear=False, start=got1)
    want2 = np.asfortranarray(want1.copy())
    want2[m2] = np.float32(100.0)
    assert same_bits(got2, want2)
    # host form, accumulating
    assert same_bits(solver.rasterize_polygons(g, second, value=100.0, layer=got1), want2)
    # clear = 1 over the same start: NaN elsewhere
    got3, _ = _device_raster(solver, g, polys, clear=True, start=start)
    assert same_bits(got3, expected_layer(m1 | m2))
    # no polygons: all NaN with clear, nothing touched without
    got4, _ = _device_raster(solver, g, np.zeros((0, 4, 2)), clear=True, start=start)
    assert np.all(got4.view(np.uint32) == NAN_BITS)
    got5, _ = _device_raster(solver, g, np.zeros((0, 4, 2)), clear=False, start=start)
    assert same_bits(got5, start)


@pytest.mark.gpu
def test_nonconvex_and_closing_vertex(cilqr, oracle, solver):
    args = GEOMETRIES["300x200"]
    g = cilqr.map_geom(*args)
    cx, cy = cell_centres(oracle, args)
    # an L-shaped hexagon and an arrowhead (both non-convex, six vertices), rotated off the axes
    def rot(p, a, ox, oy):
        p = np.array(p, dtype=np.float64)
        return np.stack([math.cos(a) * p[:, 0] - math.sin(a) * p[:, 1] + ox, math.sin(a) * p[:, 0] + math.cos(a) * p[:, 1] + oy], 1)
    ell = rot([(0, 0), (12, 0), (12, 3), (4, 3), (4, 9), (0, 9)], 0.37, 18.0, -12.0)
    arrow = rot([(0, 0), (8, 5), (0, 10), (3, 5), (0, 5.5), (2.5, 4.5)], -1.1, 40.0, 2.0)
    hexes = np.stack([ell, arrow])
    mask = inside_mask(cx, cy, hexes)
    assert mask.sum() >= 1000
    got, _ = _device_raster(solver, g, hexes)
    assert same_bits(got, expected_layer(mask))
    # a notch of the L is really outside: the polygon is not filled as its hull
    hull_only = inside_mask(cx, cy, [rot([(0, 0), (12, 0), (12, 3), (0, 9)], 0.37, 18.0, -12.0)]) & ~inside_mask(cx, cy, [ell])
    assert hull_only.sum() > 100 and np.all(np.isnan(got[hull_only & ~inside_mask(cx, cy, [arrow])]))
    # with the closing vertex the reference adds (seven vertices) nothing changes
    closed = np.concatenate([hexes, hexes[:, :1]], axis=1)
    assert closed.shape == (2, 7, 2)
    assert np.array_equal(inside_mask(cx, cy, closed), mask)
    got_closed, _ = _device_raster(solver, g, closed)
    assert same_bits(got_closed, got)
    # and so for boxes: four corners against five
    boxes = scene_polygons(cilqr, args, seed=3)
    a, _ = _device_raster(solver, g, boxes)
    b, _ = _device_raster(solver, g, np.concatenate([boxes, boxes[:, :1]], axis=1))
    assert same_bits(a, b)
    # sixteen vertices, the most a polygon may have: a star
    ang = np.linspace(0.0, 2.0 * math.pi, 16, endpoint=False)
    rad = np.where(np.arange(16) % 2 == 0, 9.0, 3.5)
    star = np.stack([25.0 + rad * np.cos(ang), -7.0 + rad * np.sin(ang)], 1)[None]
    got_star, _ = _device_raster(solver, g, star)
    assert same_bits(got_star, expected_layer(inside_mask(cx, cy, star)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1024x1024", "513x207"])
def test_warp_and_frame_with_polygons_equal_the_layer_calls(cilqr, oracle, solver, name):
    import torch
    dev = torch.device("cuda", 0)
    args = GEOMETRIES[name]
    dg = cilqr.map_geom(*args)
    sg = cilqr.map_geom(70.0, 36.0, 0.2, 12.0, -3.0)  # smaller than the 1024^2 frame and turned: part of every frame is out of range
    vx, vy, vth = 2.0, -1.5, 0.7
    rng = np.random.default_rng(17)
    src = rng.integers(0, 101, (sg.rows, sg.cols)).astype(np.float32)
    src[rng.random(src.shape) < 0.05] = np.nan
    d_src = torch.from_numpy(np.ascontiguousarray(src.reshape(-1, order="F"))).to(dev)
    polys = scene_polygons(cilqr, args, seed=29)
    nd = dg.rows * dg.cols
    stream = torch.cuda.current_stream().cuda_stream
    bbox, d_bbox = _device_raster(solver, dg, polys)
    assert (bbox == 100.0).sum() >= 1000

    f32 = lambda: torch.full((nd,), -3.0, dtype=torch.float32, device=dev)  # noqa: E731
    oob_a, oob_b = torch.full((1,), -1, dtype=torch.int64, device=dev), torch.full((1,), -1, dtype=torch.int64, device=dev)
    bits = lambda t: t.view(torch.int32).cpu().numpy()  # noqa: E731

    # warp
    dst_a, dst_b = f32(), f32()
    solver.warp_costmap_device(stream, d_src.data_ptr(), sg, dst_a.data_ptr(), dg, vx, vy, vth, bbox=d_bbox.data_ptr(), n_oob=oob_a.data_ptr())
    solver.warp_costmap_polygons_device(stream, d_src.data_ptr(), sg, dst_b.data_ptr(), dg, vx, vy, vth, polys, n_oob=oob_b.data_ptr())
    torch.cuda.synchronize()
    assert int(oob_a.item()) == int(oob_b.item()) > 0
    assert int(oob_a.item()) < nd  # part of the frame is inside the source
    assert np.array_equal(bits(dst_a), bits(dst_b))
    host = dst_b.cpu().numpy().reshape((dg.rows, dg.cols), order="F")
    assert np.all(host[bbox == 100.0] == 100.0)
    assert np.isnan(host).sum() > 0  # out-of-range cells outside the polygons stay NaN
    # no polygons: the warp without a bbox layer
    solver.warp_costmap_device(stream, d_src.data_ptr(), sg, dst_a.data_ptr(), dg, vx, vy, vth, n_oob=oob_a.data_ptr())
    solver.warp_costmap_polygons_device(stream, d_src.data_ptr(), sg, dst_b.data_ptr(), dg, vx, vy, vth, np.zeros((0, 4, 2)), n_oob=oob_b.data_ptr())
    torch.cuda.synchronize()
    assert int(oob_a.item()) == int(oob_b.item()) and np.array_equal(bits(dst_a), bits(dst_b))

    # frame
    sig = (0.16, 0.16, 0.017)
    veh_a, veh_b, unc_a, unc_b = f32(), f32(), f32(), f32()
    occ_a, occ_b = torch.full((nd,), 77, dtype=torch.int8, device=dev), torch.full((nd,), 78, dtype=torch.int8, device=dev)
    oob_a.fill_(-1)
    oob_b.fill_(-1)
    solver.costmap_frame_device(stream, d_src.data_ptr(), sg, dg, vx, vy, vth, *sig, veh_a.data_ptr(), unc_a.data_ptr(),
                                occupancy_out=occ_a.data_ptr(), bbox=d_bbox.data_ptr(), n_oob=oob_a.data_ptr())
    solver.costmap_frame_polygons_device(stream, d_src.data_ptr(), sg, dg, vx, vy, vth, polys, *sig, veh_b.data_ptr(), unc_b.data_ptr(),
                                         occupancy_out=occ_b.data_ptr(), n_oob=oob_b.data_ptr())
    torch.cuda.synchronize()
    assert int(oob_a.item()) == int(oob_b.item()) > 0
    assert np.array_equal(bits(veh_a), bits(veh_b))
    assert np.array_equal(bits(unc_a), bits(unc_b))
    assert np.array_equal(occ_a.cpu().numpy(), occ_b.cpu().numpy())
    # the frame's vehicle layer is the warp with the rasterised layer
    solver.warp_costmap_device(stream, d_src.data_ptr(), sg, dst_a.data_ptr(), dg, vx, vy, vth, bbox=d_bbox.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(bits(veh_b), bits(dst_a))
