"""Distance to the occupied cells of a layer (cilqr_map_distance*, cilqr_inflate_map*, include/cilqr.h): the exact squared Euclidean
distance transform of L layers per call, in cells, and the layers inflated from that field, which the unchanged solve kernels read.

Expected values never come from the HIP path.  `d2_brute` is the definition itself — the minimum over ALL seeds of (i - i')^2 +
(j - j')^2 in integers — and is checked against scipy.ndimage.distance_transform_edt on every test shape; `dist_restate` and
`inflate_restate` are the header's formulas in numpy doubles, one operation at a time.  The device is compared with them integer for
integer and bit for bit: there is no tolerance in this file except the solve's (max|dU| <= 1e-9, equal iterations, the suite's bar).

Shapes: 1x1, 1x7, 7x1 (degenerate lines); 65x3, 3x65 (one past a wavefront in either direction); 64x64, 130x129, 150x100 (the node's).
Layers per shape (`_layers`): 2 % random seeds with NaN cells; one corner cell; every second cell with NaN cells; none; every cell.
Inflation constants of the pipeline test: inscribed 0.3 m, radius 1.5 m, peak 100.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_tighten_map import ROUND_BLOB, _round_params, _round_scene

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
NONE = 2 ** 31 - 1
UNKNOWN_SEEDS, TO_FREE = 1, 2
ENTRY_POINTS = ("cilqr_map_distance", "cilqr_map_distance_device", "cilqr_inflate_map", "cilqr_inflate_map_device")
SHAPES = [(1, 1), (1, 7), (7, 1), (65, 3), (3, 65), (64, 64), (130, 129), (150, 100)]
THRESHOLD = 50.0
RES = 0.1
INFLATE = dict(inscribed=0.3, radius=1.5, peak=100.0)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


# ---- expected values: the definition, restated --------------------------------------------------------------------------------------
def seeds_of(layer, threshold, flags=0):
    """The header's seed predicate on a (rows, cols) float32 layer."""
    with np.errstate(invalid="ignore"):
        seed = np.isfinite(layer) & (layer.astype(np.float64) > threshold)
    if flags & UNKNOWN_SEEDS:
        seed = seed | np.isnan(layer)
    return ~seed if flags & TO_FREE else seed


def d2_brute(seed):
    """min over all seeds of (i - i')^2 + (j - j')^2, int32; NONE without a seed."""
    rows, cols = seed.shape
    si, sj = np.nonzero(seed)
    if si.size == 0:
        return np.full((rows, cols), NONE, dtype=np.int32)
    i, j = (a.reshape(-1).astype(np.int64) for a in np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij"))
    out = np.empty(rows * cols, dtype=np.int64)
    step = max(1, (1 << 22) // si.size)
    for a in range(0, rows * cols, step):
        di, dj = i[a:a + step, None] - si[None, :], j[a:a + step, None] - sj[None, :]
        out[a:a + step] = (di * di + dj * dj).min(axis=1)
    return out.reshape(rows, cols).astype(np.int32)


def dist_restate(d2, res):
    """(float)(res * sqrt((double)d2)); +inf where the layer has no seed."""
    with np.errstate(over="ignore"):
        return np.where(d2 == NONE, np.float32(np.inf), (res * np.sqrt(d2.astype(np.float64))).astype(np.float32))


def inflate_restate(layer, d2, res, inscribed, radius, peak):
    d = res * np.sqrt(d2.astype(np.float64))
    ramp = peak * (radius - d) / (radius - inscribed)
    v = np.where(d2 == NONE, 0.0, np.where(d <= inscribed, peak, np.where(d >= radius, 0.0, ramp)))
    f = v.astype(np.float32)
    with np.errstate(invalid="ignore"):
        known = np.where(layer > f, layer, f)
    return np.where(np.isnan(layer), np.where(v > 0.0, f, np.float32(np.nan)), known).astype(np.float32)


def _layers(rows, cols):
    """Five (rows, cols) float32 layers: sparse with NaN, one corner, dense with NaN, none, every cell."""
    rng = np.random.Generator(np.random.PCG64(1000 * rows + cols))
    cells = rows * cols

    reserved = [0, (rows // 2) + (cols // 2) * rows] if cells > 4 else []
    free = np.setdiff1d(np.arange(cells), reserved)

    def field(density):
        a = rng.uniform(0.0, THRESHOLD, (rows, cols)).astype(np.float32)
        pick = rng.choice(free, max(1, int(round(density * free.size))), replace=False)
        a[pick % rows, pick // rows] = rng.uniform(THRESHOLD + 1.0, 100.0, pick.size).astype(np.float32)
        nan = rng.choice(free, max(1, cells // 50), replace=False)
        a[nan % rows, nan // rows] = np.nan
        if reserved:
            a[0, 0] = np.float32(THRESHOLD)    # AT the threshold: strict > makes no seed of it
            a[rows // 2, cols // 2] = np.inf   # not finite: no seed
        return a

    sparse, dense = field(0.02), field(0.5)
    corner = np.zeros((rows, cols), dtype=np.float32)
    corner[rows - 1, 0] = 100.0
    return [sparse, corner, dense, np.zeros((rows, cols), dtype=np.float32), np.full((rows, cols), 100.0, dtype=np.float32)]


@pytest.fixture(scope="module")
def cases():
    """Per shape: the layers and, per flags value, the brute-force d2 of each.  Computed once; never modified."""
    out = {}
    for rows, cols in SHAPES:
        layers = _layers(rows, cols)
        out[(rows, cols)] = dict(layers=layers, d2={f: [d2_brute(seeds_of(a, THRESHOLD, f)) for a in layers] for f in range(4)})
    return out


def _geom(cilqr, rows, cols, res=RES):
    g = cilqr.MapGeom()
    g.rows, g.cols, g.res, g.len_x, g.len_y = rows, cols, res, rows * res, cols * res
    return g


def _flat(a):
    return np.ascontiguousarray(np.asarray(a).T).reshape(-1)


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_MAP_DISTANCE_UNKNOWN_SEEDS\s+1u", h) and re.search(r"#define\s+CILQR_MAP_DISTANCE_TO_FREE\s+2u", h)
    assert (cilqr.MAP_DISTANCE_UNKNOWN_SEEDS, cilqr.MAP_DISTANCE_TO_FREE, cilqr.MAP_DISTANCE_NONE) == (1, 2, NONE)
    for m in ("map_distance", "map_distance_device", "inflate_map", "inflate_map_device"):
        assert callable(getattr(cilqr.Solver, m)), m
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_map_distance\s*\(", plan) and re.search(r"inline\s+void\s+plan_inflate_map\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/costmap_distance.hip" in mk and len(re.findall(r"build/costmap_distance\.o", mk)) == 2  # `check` and its resource list
    text = re.sub(r"\s*\n \*\s*", " ", full)
    for phrase in ("INT32_MAX when the layer has no seed", "is complemented", "unknown stays unknown", "judge the final plan against the ORIGINAL map"):
        assert phrase in text, phrase


def test_argument_errors_need_no_device(cilqr):
    """Everything the header lists is decided before the handle is looked at (there is none here); valid arguments reach the handle."""
    L = cilqr.lib()
    rows, cols = 5, 4
    layer, d2, dist, out = (np.zeros(3 * rows * cols, dtype=t) for t in (np.float32, np.int32, np.float32, np.float32))
    nan, inf = float("nan"), float("inf")
    no_handle = C.c_void_p()

    def distance(dev, n=3, stride=rows * cols, g=None, thr=THRESHOLD, flags=0, **nulls):
        a = dict(layer=layer, d2=d2)
        a.update(nulls)
        g = _geom(cilqr, rows, cols) if g is None else g
        f = L.cilqr_map_distance_device if dev else L.cilqr_map_distance
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, n, _p(a["layer"], _fp), C.c_int64(stride), C.byref(g) if g != 0 else None, C.c_double(thr), C.c_uint32(flags),
                 _p(a["d2"], _ip), _p(dist, _fp))

    def inflate(dev, n=3, stride=rows * cols, g=None, inscribed=0.3, radius=1.5, peak=100.0, **nulls):
        a = dict(layer=layer, d2=d2, out=out)
        a.update(nulls)
        g = _geom(cilqr, rows, cols) if g is None else g
        f = L.cilqr_inflate_map_device if dev else L.cilqr_inflate_map
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, n, _p(a["layer"], _fp), C.c_int64(stride), C.byref(g) if g != 0 else None, _p(a["d2"], _ip), C.c_double(inscribed),
                 C.c_double(radius), C.c_double(peak), _p(a["out"], _fp))

    for dev in (False, True):
        for call, names in ((distance, ("layer", "d2")), (inflate, ("layer", "d2", "out"))):
            for name in names:
                assert call(dev, **{name: None}) == ERR_ARG and b"null" in L.cilqr_last_error(), name
            assert call(dev, g=0) == ERR_ARG and b"null layer or geometry" in L.cilqr_last_error()
            for n in (0, -1):
                assert call(dev, n=n) == ERR_ARG and b"must be at least 1" in L.cilqr_last_error()
            for stride in (-1, 1, rows * cols - 1):
                assert call(dev, stride=stride) == ERR_ARG and b"layer_stride" in L.cilqr_last_error(), stride
            for bad in (_geom(cilqr, 0, 4), _geom(cilqr, 4, 0), _geom(cilqr, 4, 4, 0.0), _geom(cilqr, 4, 4, -0.1), _geom(cilqr, 4, 4, nan), _geom(cilqr, 4, 4, inf)):
                assert call(dev, stride=0, g=bad) == ERR_ARG and b"bad geometry" in L.cilqr_last_error()
            for big in (_geom(cilqr, 8193, 2), _geom(cilqr, 2, 8193)):
                assert call(dev, stride=0, g=big) == ERR_UNSUPPORTED and b"more than 8192 along a side" in L.cilqr_last_error()
            assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()            # valid arguments, no handle
            assert call(dev, stride=0) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # one shared layer is allowed
            assert call(dev, stride=0, g=_geom(cilqr, 8192, 8192)) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # the largest map
        assert distance(dev, thr=nan) == ERR_ARG and b"occ_threshold is NaN" in L.cilqr_last_error()
        assert distance(dev, flags=4) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert distance(dev, thr=inf, flags=3) == ERR_ARG and b"null handle" in L.cilqr_last_error()
        for kw in (dict(inscribed=-0.1), dict(inscribed=nan), dict(radius=nan), dict(radius=inf), dict(inscribed=1.5), dict(inscribed=2.0)):
            assert inflate(dev, **kw) == ERR_ARG and b"0 <= inscribed < radius" in L.cilqr_last_error(), kw
        for peak in (0.0, -1.0, nan, inf):
            assert inflate(dev, peak=peak) == ERR_ARG and b"peak" in L.cilqr_last_error(), peak
        assert inflate(dev, inscribed=0.0) == ERR_ARG and b"null handle" in L.cilqr_last_error()


def _build(tmp_path, source, *includes):
    exe = str(tmp_path / source.replace(".cpp", ""))
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + ["-I" + d for d in includes] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", source)],
                   check=True)
    return exe


def test_the_host_forms_fit_the_unchanged_arena_or_return_its_error(tmp_path):
    """tests/cpp/host_plan_map_distance.cpp: host_arena_bytes is still what tests/golden/host_arena_cap.json recorded; the distance and
    inflate plans are three arrays of 4 bytes a cell, inputs in front of outputs; the node's 150 x 100 map fits the arena of a
    (64, 50, 4) handle with L = 6 and not with L = 8, where the transport returns its error (test_limits runs that on the device)."""
    import json
    exe = _build(tmp_path, "host_plan_map_distance.cpp", os.path.join(ROOT, "include"), os.path.join(PKG, "csrc"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every clearance shape fits" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20
    cap = dict(((b, n, m), c) for b, n, m, c in golden)[(64, 50, 4)]
    cells = 150 * 100
    for L, stride, fits in ((1, 0, True), (6, cells, True), (8, cells, False), (16, 0, False)):
        span = (L - 1) * stride + cells
        r = subprocess.run([exe, "layers", str(L), str(cells), str(span), "1"], capture_output=True, text=True, check=True)
        for name, third_in in (("distance", 0), ("inflate", 1)):
            lines = [line.split()[1:] for line in r.stdout.splitlines() if line.startswith(name + " ")]
            entries = [[int(v) for v in line[1:]] for line in lines if line[0] == "entry"]
            sizes, at = [4 * span, 4 * L * cells, 4 * L * cells], 0
            for (off, nbytes, src, dst), want in zip(entries, sizes):
                assert (off, nbytes) == (at, want)
                at = (off + nbytes + 15) // 16 * 16
            assert [e[2] for e in entries] == ([1, 1, 0] if third_in else [1, 0, 0]) and [e[3] for e in entries] == ([0, 0, 1] if third_in else [0, 1, 1])
            tail = [line for line in lines if line[0] == "plan"][0]
            tail = dict(zip(tail[1::2], (int(v) for v in tail[2::2])))
            assert tail["ok"] == 1 and tail["end"] == at and (at <= cap) == fits, (name, L, stride, at, cap)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_brute_force_against_scipy(cases, shape):
    """The definition — the minimum over all seeds — equals rint(distance_transform_edt(~seed)**2) wherever there is a seed, for every
    layer and every flags value; and the layers are what they are there for."""
    from scipy.ndimage import distance_transform_edt
    c = cases[shape]
    n = 0
    for flags in range(4):
        for layer, d2 in zip(c["layers"], c["d2"][flags]):
            seed = seeds_of(layer, THRESHOLD, flags)
            if seed.any():
                assert np.array_equal(d2, np.rint(distance_transform_edt(~seed) ** 2).astype(np.int32))
                assert np.array_equal(d2 == 0, seed)
                n += 1
            else:
                assert np.all(d2 == NONE)
    sparse, corner, dense, none, every = (seeds_of(a, THRESHOLD) for a in c["layers"])
    assert n >= 8 and not none.any() and every.all() and corner.sum() == 1 and corner[-1, 0]
    assert np.isnan(c["layers"][0]).any() and np.isnan(c["layers"][2]).any()
    if shape[0] * shape[1] > 4:
        assert c["layers"][0][0, 0] == np.float32(THRESHOLD) and not sparse[0, 0]  # AT the threshold: strict > makes no seed of it
        assert not np.array_equal(c["d2"][0][0], c["d2"][UNKNOWN_SEEDS][0])  # the NaN cells matter
        assert np.isinf(c["layers"][0]).any() and not sparse[np.isinf(c["layers"][0])].any()


def test_the_inflation_restated():
    """The ramp on a hand case: one seed, res 0.5: peak within inscribed, linear between, zero from radius on; NaN cells take v > 0 only."""
    layer = np.zeros((1, 9), dtype=np.float32)
    layer[0, 0], layer[0, 2], layer[0, 7], layer[0, 3] = 100.0, np.nan, np.nan, 60.0
    d2 = d2_brute(seeds_of(layer, THRESHOLD))
    assert d2[0].tolist() == [0, 1, 1, 0, 1, 4, 9, 16, 25]
    got = inflate_restate(layer, d2, 0.5, 0.5, 2.0, 90.0)
    assert got[0, :7].tolist() == [100.0, 90.0, 90.0, 90.0, 90.0, 60.0, 30.0] and np.isnan(got[0, 7]) and got[0, 8] == 0.0
    assert np.array_equal(inflate_restate(layer, np.full((1, 9), NONE, dtype=np.int32), 0.5, 0.5, 2.0, 90.0).view(np.uint32), layer.view(np.uint32))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


FILL_I, FILL_F = -7, -7.0  # what the output buffers hold before a call


def _device(cilqr, solver, layers, g, flags, n=None, pad=0, want_dist=True, inflate=None, in_place=False):
    """The device forms on torch buffers.  layers: a list (layer stride cells + pad) or one layer with n given (stride 0).  Returns
    dict(d2, dist, out) as (L, rows, cols) arrays."""
    import torch
    dev = torch.device("cuda", 0)
    rows, cols = int(g.rows), int(g.cols)
    cells = rows * cols
    if n is None:
        n, stride = len(layers), cells + pad
        buf = np.full(n * stride, np.float32(100.0))  # (padding that would be a seed if it were read as a cell)
        for l, a in enumerate(layers):
            buf[l * stride:l * stride + cells] = _flat(a)
    else:
        stride, buf = 0, _flat(layers)
    lay = torch.from_numpy(buf).to(dev)
    d2 = torch.full((n, cells), FILL_I, dtype=torch.int32, device=dev)
    dist = torch.full((n, cells), FILL_F, dtype=torch.float32, device=dev) if want_dist else None
    st = torch.cuda.current_stream(dev).cuda_stream
    torch.cuda.synchronize(dev)
    solver.map_distance_device(st, n, lay.data_ptr(), stride, g, THRESHOLD, d2.data_ptr(), dist.data_ptr() if want_dist else 0, flags)
    out = None
    if inflate is not None:
        out = lay if in_place else torch.full((n, cells), FILL_F, dtype=torch.float32, device=dev)
        solver.inflate_map_device(st, n, lay.data_ptr(), stride, g, d2.data_ptr(), inflate["inscribed"], inflate["radius"], inflate["peak"], out.data_ptr())
    torch.cuda.synchronize(dev)
    shape = lambda t: None if t is None else t.cpu().numpy().reshape(n, cols, rows).transpose(0, 2, 1)  # noqa: E731
    return dict(d2=shape(d2), dist=shape(dist), out=shape(out))


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_distance_and_inflation_against_the_restatement(cilqr, solver, cases, shape):
    """Every flags value; L = 5 with its own (padded) stride, every layer alone at L = 1, and L = 3 of one shared layer: d2 integer for
    integer, dist_out and layer_out bit for bit; a layer's result inside the batch is its result alone."""
    c = cases[shape]
    g = _geom(cilqr, *shape)
    for flags in range(4):
        want = c["d2"][flags]
        got = _device(cilqr, solver, c["layers"], g, flags, pad=5, inflate=INFLATE)
        for l, layer in enumerate(c["layers"]):
            assert np.array_equal(got["d2"][l], want[l]), (flags, l)
            assert np.array_equal(_bits32(got["dist"][l]), _bits32(dist_restate(want[l], RES))), (flags, l)
            assert np.array_equal(_bits32(got["out"][l]), _bits32(inflate_restate(layer, want[l], RES, **INFLATE))), (flags, l)
            alone = _device(cilqr, solver, [layer], g, flags, inflate=INFLATE)
            for k in ("d2", "dist", "out"):
                assert np.array_equal(alone[k][0].view(np.uint32), got[k][l].view(np.uint32)), (flags, l, k)
        three = _device(cilqr, solver, c["layers"][:3], g, flags, pad=3, inflate=INFLATE)  # L = 3 with its own stride
        for k in ("d2", "dist", "out"):
            assert np.array_equal(three[k].view(np.uint32), got[k][:3].view(np.uint32)), (flags, k)
        shared = _device(cilqr, solver, c["layers"][0], g, flags, n=3, inflate=INFLATE)
        for l in range(3):
            for k in ("d2", "dist", "out"):
                assert np.array_equal(shared[k][l].view(np.uint32), got[k][0].view(np.uint32)), (flags, l, k)
    assert np.all(got["d2"][3] == 0) and np.all(np.isinf(got["dist"][4])) and np.all(got["d2"][4] == NONE)  # flags 3: none <-> every cell


@gpu
def test_optional_outputs_the_host_forms_and_in_place(cilqr, solver, cases):
    """dist_out left out; the host forms give the device forms' bits; layer_out may be the layers themselves."""
    for shape in ((65, 3), (150, 100)):
        c = cases[shape]
        g = _geom(cilqr, *shape)
        full = _device(cilqr, solver, c["layers"][:3], g, 0, inflate=INFLATE)
        bare = _device(cilqr, solver, c["layers"][:3], g, 0, want_dist=False)
        assert bare["dist"] is None and np.array_equal(bare["d2"], full["d2"])
        host = solver.map_distance(np.stack(c["layers"][:3]), g, THRESHOLD)
        assert np.array_equal(host["d2"], full["d2"]) and np.array_equal(_bits32(host["dist"]), _bits32(full["dist"]))
        assert solver.map_distance(c["layers"][0], g, THRESHOLD, want_dist=False)["dist"] is None
        shared = solver.map_distance(c["layers"][0], g, THRESHOLD, L=2, unknown_seeds=True, to_free=True)
        assert np.array_equal(shared["d2"][1], c["d2"][3][0]) and np.array_equal(shared["d2"][0], shared["d2"][1])
        out = solver.inflate_map(np.stack(c["layers"][:3]), g, host["d2"], **INFLATE)
        assert np.array_equal(_bits32(out), _bits32(full["out"]))
        same = _device(cilqr, solver, c["layers"][:3], g, 0, inflate=INFLATE, in_place=True)
        assert np.array_equal(_bits32(same["out"]), _bits32(full["out"]))


@gpu
def test_limits(cilqr, solver, cases):
    """A host call beyond the arena returns the transport's error and the handle stays usable; an output that overlaps the layers
    without being them is refused; a map beyond 8192 cells along a side is unsupported."""
    import torch
    c = cases[(150, 100)]
    g = _geom(cilqr, 150, 100)
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers" % ERR_ARG):
        solver.map_distance(np.stack([c["layers"][0]] * 16), g, THRESHOLD)
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers" % ERR_ARG):
        solver.inflate_map(np.stack([c["layers"][0]] * 16), g, np.zeros((16, 150, 100), dtype=np.int32), **INFLATE)
    assert np.array_equal(solver.map_distance(c["layers"][0], g, THRESHOLD)["d2"][0], c["d2"][0][0])
    dev = torch.device("cuda", 0)
    cells = 150 * 100
    lay = torch.zeros(3 * cells + 8, dtype=torch.float32, device=dev)
    d2 = torch.zeros(3 * cells, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    for stride, off in ((cells, 1), (cells, cells), (0, 0), (cells + 4, 0)):
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*overlaps layer" % ERR_ARG):
            solver.inflate_map_device(0, 3, lay.data_ptr(), stride, g, d2.data_ptr(), 0.3, 1.5, 100.0, lay.data_ptr() + 4 * off)
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*more than 8192" % ERR_UNSUPPORTED):
        solver.map_distance_device(0, 1, lay.data_ptr(), 0, _geom(cilqr, 8193, 1), THRESHOLD, d2.data_ptr())


# ---- distance -> inflate -> set map -> solve, judged against the ORIGINAL map ------------------------------------------------------------
def rect_clearance(p, g, pose, layer, X, N, threshold, margin=0.0):
    """The definition of cilqr_map_clearance restated without a reach (tests/test_map_clearance.py holds the full restatement and checks
    it against sampled boundaries): per plan the minimum over t < N and over the seeds of the signed clearance of the cell's centre
    to the rectangle."""
    hl, hw = 0.5 * p.length + margin, 0.5 * p.width + margin
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    si, sj = np.nonzero(seeds_of(layer, threshold))
    mx, my = x_first - si * g.res, y_first - sj * g.res
    c, s = math.cos(pose[2]), math.sin(pose[2])
    wx, wy = pose[0] + c * mx - s * my, pose[1] + s * mx + c * my  # the seeds' centres in the planning frame
    out = []
    for Xb in X.reshape(X.shape[0], N + 1, 4):
        best = np.inf
        for t in range(N):
            x, y, th = Xb[t, 0], Xb[t, 1], Xb[t, 3]
            a = (wx - x) * math.cos(th) + (wy - y) * math.sin(th)
            b = (wy - y) * math.cos(th) - (wx - x) * math.sin(th)
            ua, ub = np.abs(a) - hl, np.abs(b) - hw
            sgn = np.where((ua > 0) | (ub > 0), np.hypot(np.maximum(ua, 0), np.maximum(ub, 0)), np.maximum(ua, ub))
            best = min(best, float(sgn.min()))
        out.append(best)
    return np.array(out)


@pytest.fixture(scope="module")
def blob(oracle):
    """The blob scene of tests/test_tighten_map.py — six candidates beside a straight path, the blob at (6, -1.4), w_uncertainty 5 —
    solved by the oracle on the original layer and on the numpy-inflated one; the restated clearance of both plans to the ORIGINAL map."""
    O = oracle
    s = _round_scene(O)
    th = min(8, O.max_threads())
    d2 = d2_brute(seeds_of(s["layers"], THRESHOLD))
    inflated = inflate_restate(s["layers"], d2, s["g"].res, **INFLATE)
    solves = []
    for layer in (s["layers"], inflated):
        um, keep = O.uncertainty_map(layer, s["g"], s["poses"], s["probes"])
        solves.append(O.solve_batch_unc(s["p"], s["N"], 0, s["x0"], s["U0"].copy(), s["poly"], s["fl"], None, None, None, um, threads=th))
    clr = [rect_clearance(s["p"], s["g"], s["poses"], s["layers"], r["X"], s["N"], THRESHOLD) for r in solves]
    return dict(s=s, d2=d2, inflated=inflated, before=solves[0], after=solves[1], clr_before=clr[0], clr_after=clr[1])


def test_the_inflated_layer_does_what_it_is_for(blob):
    """From the oracle's solves on the CPU: against the ORIGINAL map, the candidate nearest the blob is strictly farther from the occupied
    cells after solving on the inflated layer than before (the six before/after values are in DESIGN §4.8p)."""
    a = blob
    print("clearance to the original map before %s\n                                  after  %s\niterations %s -> %s" % (
        np.round(a["clr_before"], 4).tolist(), np.round(a["clr_after"], 4).tolist(), a["before"]["iters"].tolist(), a["after"]["iters"].tolist()))
    assert ROUND_BLOB[:2] == (6.0, -1.4) and a["s"]["p"].w_uncertainty == 5.0 and a["s"]["B"] == 6
    k = int(np.argmin(a["clr_before"]))
    assert np.isfinite(a["clr_before"]).all() and a["clr_after"][k] > a["clr_before"][k]
    raised = (a["inflated"] > a["s"]["layers"]).sum()
    assert raised > 100 and np.all(a["inflated"] >= a["s"]["layers"])


@gpu
def test_pipeline_distance_inflate_set_solve(cilqr, blob):
    """distance -> inflate -> set map -> solve, every call in its device form on one stream, against numpy inflation and the oracle's
    solve with the map set: the layer bit for bit, max|dU| <= 1e-9, equal iterations and exits."""
    import torch
    a = blob
    s = a["s"]
    B, N, g = s["B"], s["N"], s["g"]
    k = int(np.argmin(a["clr_before"]))
    assert a["clr_after"][k] > a["clr_before"][k]  # what the feature is for, from the oracle's solves alone
    cells = int(g.rows) * int(g.cols)
    geom = cilqr.map_geom(*s["geom"])
    solver = cilqr.Solver(_round_params(cilqr, N), max_batch=B, max_horizon=N, max_obstacles=0, device=0)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
        x0, U, poly, fl = (up(v) for v in (s["x0"], s["U0"], s["poly"], s["fl"]))
        layer = torch.from_numpy(_flat(s["layers"])).to(dev)
        d2 = torch.zeros(cells, dtype=torch.int32, device=dev)
        soft = torch.zeros(cells, dtype=torch.float32, device=dev)
        X, J = torch.zeros((B, 4 * (N + 1)), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
        it, ex = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        solver.map_distance_device(st, 1, layer.data_ptr(), 0, geom, THRESHOLD, d2.data_ptr())
        solver.inflate_map_device(st, 1, layer.data_ptr(), 0, geom, d2.data_ptr(), INFLATE["inscribed"], INFLATE["radius"], INFLATE["peak"], soft.data_ptr())
        solver.set_uncertainty_map_device(soft.data_ptr(), geom, s["poses"], s["probes"])
        solver.solve_batch_device(st, B, N, 0, x0.data_ptr(), U.data_ptr(), poly.data_ptr(), fl.data_ptr(), 0, 0, 0, X.data_ptr(), J.data_ptr(),
                                  it.data_ptr(), ex.data_ptr())
        torch.cuda.synchronize(dev)
        solver.clear_uncertainty_map()
    finally:
        solver.close()
    got_layer = soft.cpu().numpy().reshape(int(g.cols), int(g.rows)).T
    dU = float(np.max(np.abs(U.cpu().numpy() - a["after"]["U"])))
    print("max|dU| %.3g, iterations %s (oracle %s)" % (dU, it.cpu().numpy().tolist(), a["after"]["iters"].tolist()))
    assert np.array_equal(d2.cpu().numpy().reshape(int(g.cols), int(g.rows)).T, a["d2"])
    assert np.array_equal(_bits32(got_layer), _bits32(a["inflated"]))
    assert np.array_equal(it.cpu().numpy(), a["after"]["iters"]) and np.array_equal(ex.cpu().numpy(), a["after"]["status"])
    assert dU <= 1e-9
    got_clr = rect_clearance(s["p"], g, s["poses"], s["layers"], X.cpu().numpy(), N, THRESHOLD)
    k = int(np.argmin(a["clr_before"]))
    assert got_clr[k] > a["clr_before"][k]
