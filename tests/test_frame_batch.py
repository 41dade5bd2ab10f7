"""K costmap frames per launch: cilqr_blur_costmap_batch_device and cilqr_costmap_frame_batch_device.

The batched kernels are the single-frame kernels with a frame dimension (blockIdx.y), so the -m gpu tests hold every frame to the
single-frame HIP path BIT FOR BIT (the existing suite pins that path to the oracle), and hold the first and last frame of every
case to the oracle directly under the bounds of test_gpu_parity.test_blur_kernel_vs_oracle /
test_costmap_frame_equals_its_three_steps: ellipse membership counts equal, outputs within 1 float32 ulp, at least 99.9 % of
them bit-equal.  The solve at the end of the candidate sequence is held to the suite's enforced TIGHT = 1e-9.
"""
import ctypes as C

import numpy as np
import pytest

ERR_ARG = -1


# ---------------------------------------------------------------------------------------------- without a GPU
def test_frame_batch_argument_errors_do_not_need_a_device(cilqr):
    """Every rejection include/cilqr.h lists for the two entry points comes back as CILQR_ERR_ARG with no handle and no device, and
    cilqr_last_error() names the function."""
    L = cilqr.lib()
    d, dp = C.c_double, C.POINTER(C.c_double)
    g = cilqr.map_geom(30.0, 20.0, 0.2, 15.0, 0.0)
    gg = cilqr.map_geom(120.0, 120.0, 0.2, 3.0, -2.0)
    cells = g.rows * g.cols
    no_handle = C.c_void_p()
    fake_handle = C.c_void_p(8)  # never dereferenced: each call below fails on an argument first
    layer = np.zeros(cells, dtype=np.float32).ctypes.data_as(C.c_void_p)  # (a host buffer: never read either)
    thetas = np.zeros(1025)
    poses = np.zeros((1025, 3))
    assert L.cilqr_abi_version() == 2

    def blur(h=fake_handle, src=layer, stride=0, geom=g, index=0, K=4, th=thetas, out=layer):
        return L.cilqr_blur_costmap_batch_device(h, None, src, C.c_int64(stride), C.byref(geom) if geom is not None else None, index, K,
                                                 th.ctypes.data_as(dp) if th is not None else None, d(0.16), d(0.16), d(0.017), out, None)

    def frame(h=fake_handle, glob=layer, ggeom=gg, vgeom=g, K=4, po=poses, veh=layer, unc=layer):
        return L.cilqr_costmap_frame_batch_device(h, None, glob, C.byref(ggeom) if ggeom is not None else None,
                                                  C.byref(vgeom) if vgeom is not None else None, K, po.ctypes.data_as(dp) if po is not None else None,
                                                  None, d(0.16), d(0.16), d(0.017), veh, unc, None, None)

    def rejected(rc, who, what):
        msg = L.cilqr_last_error()
        return rc == ERR_ARG and who in msg and what in msg

    def bad(**kw):
        b = cilqr.map_geom(30.0, 20.0, 0.2, 15.0, 0.0)
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    who = b"cilqr_blur_costmap_batch"
    assert rejected(blur(h=no_handle), who, b"null argument")
    assert rejected(blur(src=None), who, b"null argument")
    assert rejected(blur(geom=None), who, b"null argument")
    assert rejected(blur(th=None), who, b"null argument")
    assert rejected(blur(out=None), who, b"null argument")
    for K in (0, -3, 1025):
        assert rejected(blur(K=K), who, b"K=")
    for geom in (bad(rows=0), bad(cols=-1), bad(res=0.0), bad(res=float("nan"))):
        assert rejected(blur(geom=geom), who, b"bad geometry")
    assert rejected(blur(index=-1), who, b"bad geometry")
    for stride in (-1, -cells, 1, cells - 1):
        assert rejected(blur(stride=stride), who, b"src_stride")
    # the null handle is what stops an otherwise valid call (strides 0, rows*cols and above are accepted)
    for stride in (0, cells, cells + 64):
        assert rejected(blur(h=no_handle, stride=stride, K=1024), who, b"null argument")

    who = b"cilqr_costmap_frame_batch"
    assert rejected(frame(h=no_handle), who, b"null argument")
    assert rejected(frame(glob=None), who, b"null argument")
    assert rejected(frame(ggeom=None), who, b"null argument")
    assert rejected(frame(vgeom=None), who, b"null argument")
    assert rejected(frame(po=None), who, b"null argument")
    assert rejected(frame(veh=None), who, b"null argument")
    assert rejected(frame(unc=None), who, b"null argument")
    for K in (0, -1, 1025):
        assert rejected(frame(K=K), who, b"K=")
    for geom in (bad(rows=0), bad(cols=0), bad(res=-0.2)):
        assert rejected(frame(vgeom=geom), who, b"bad geometry")
        assert rejected(frame(ggeom=geom), who, b"bad geometry")
    assert rejected(frame(h=no_handle, K=1), who, b"null argument")


def test_binding_has_the_two_batch_methods(cilqr):
    assert {"cilqr_blur_costmap_batch_device", "cilqr_costmap_frame_batch_device"} <= set(cilqr.ABI_SYMBOLS)
    assert callable(cilqr.Solver.blur_costmap_batch_device) and callable(cilqr.Solver.costmap_frame_batch_device)


# ---------------------------------------------------------------------------------------------- with a GPU
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=1, max_horizon=1, max_obstacles=0, device=0)
    yield s
    s.close()


def _flat(a):
    """(rows, cols) host layer -> its column-major cells."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, order="F"))


def _bits(t):
    return t.cpu().numpy().view(np.int32)


def _blur_vs_oracle(what, out, cnt, want, wcnt, index):
    """The bounds of test_blur_kernel_vs_oracle on one frame; the figures are printed before they are held."""
    from test_gpu_parity import _ulp32_diff
    d = _ulp32_diff(np.ascontiguousarray(out), _flat(want))
    print("%s: counts equal %s, max ulp %d, bit-equal %.5f" % (what, np.array_equal(cnt[index:], wcnt[index:]), d.max(), (d == 0).mean()))
    assert np.array_equal(cnt[index:], wcnt[index:]), what
    assert d.max() <= 1, (what, d.max())
    assert (d == 0).mean() >= 0.999, what
    assert np.isnan(out[:index]).all(), what


# (geometry, sigma, first and last heading, index): rows of test_blur_kernel_vs_oracle, whose source generator gives the first
# and last frame their source too — those two frames are frames that test holds to the oracle.  The headings in between
# include a negative one and one above pi.  The last case is this file's own.
_BLUR_CASES = [
    # 150 x 100: 8 lanes per cell; one source per frame
    ("node", (30.0, 20.0, 0.2, 15.0, 0.0), (0.16, 0.16, 0.017), 0, [-1.2, 3.6, 0.0, -2.9, 0.7, -1.2], "per_frame"),
    # 150 x 100 again, index > 0, one source under K headings
    ("node_index", (30.0, 20.0, 0.2, 15.0, 0.0), (0.005, 0.005, 0.0125), 40, [0.3, -0.7, 4.0, 0.3], "shared"),
    # 400 x 300: 4 lanes per cell; sources further apart than one layer
    ("400x300", (40.0, 30.0, 0.1, 12.0, 1.5), (0.16, 0.16, 0.017), 7, [0.9, 3.3, -2.1, 0.9], "padded"),
    # 1024 x 1024, K = 2: 1 lane per cell
    ("1024x1024", (102.4, 102.4, 0.1, 5.0, -3.0), (0.16, 0.16, 0.017), 0, [0.3, 0.3], "per_frame"),
    # 65 x 17: neither side a multiple of anything the kernel deals in; the last workgroup of a frame is mostly empty
    ("65x17", (13.0, 3.4, 0.2, 2.0, -1.0), (0.16, 0.16, 0.017), 3, [0.5, -2.0, 3.9, 1.1], "shared"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,geom,sigma,index,thetas,layout", _BLUR_CASES, ids=[c[0] for c in _BLUR_CASES])
def test_blur_batch_equals_single_frames(cilqr, oracle, solver, name, geom, sigma, index, thetas, layout):
    """cilqr_blur_costmap_batch_device against K cilqr_blur_costmap_device calls: out (as int32, NaN bits included) and count_out
    of every frame equal, at all three lanes-per-cell instantiations; first and last frame against the oracle."""
    import torch
    rng = np.random.default_rng(31)
    g, og = cilqr.map_geom(*geom), oracle.map_geom(*geom)
    cells, K = g.rows * g.cols, len(thetas)
    assert (g.rows, g.cols) == {"node": (150, 100), "node_index": (150, 100), "400x300": (400, 300), "1024x1024": (1024, 1024), "65x17": (65, 17)}[name]

    def draw():
        src = rng.integers(0, 101, (g.rows, g.cols)).astype(np.float32)
        src[rng.random(src.shape) < 0.01] = np.nan
        return src

    first = draw()  # test_blur_kernel_vs_oracle's source for this geometry
    if layout == "shared":
        srcs, stride = [first] * K, 0
    else:
        srcs = [first] + [draw() for _ in range(K - 2)] + [first]
        stride = cells if layout == "per_frame" else cells + 192
    dev = torch.device("cuda", 0)
    if stride == 0:
        d_src = torch.from_numpy(_flat(first)).to(dev)
    else:
        h_src = np.full(K * stride, -5.0, dtype=np.float32)
        for k in range(K):
            h_src[k * stride:k * stride + cells] = _flat(srcs[k])
        d_src = torch.from_numpy(h_src).to(dev)
    d_out = torch.full((K * cells,), 7.0, dtype=torch.float32, device=dev)
    d_cnt = torch.full((K * cells,), -7, dtype=torch.int32, device=dev)
    s_out = torch.full((K * cells,), 7.0, dtype=torch.float32, device=dev)
    s_cnt = torch.full((K * cells,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    solver.blur_costmap_batch_device(stream, d_src.data_ptr(), g, thetas, *sigma, d_out.data_ptr(), index=index, count_out=d_cnt.data_ptr(),
                                     src_stride=stride)
    for k in range(K):
        solver.blur_costmap_device(stream, d_src.data_ptr() + 4 * k * stride, g, thetas[k], *sigma, s_out.data_ptr() + 4 * k * cells, index=index,
                                   count_out=s_cnt.data_ptr() + 4 * k * cells)
    torch.cuda.synchronize()
    out, cnt, want, wcnt = _bits(d_out).reshape(K, cells), d_cnt.cpu().numpy().reshape(K, cells), _bits(s_out).reshape(K, cells), s_cnt.cpu().numpy().reshape(K, cells)
    for k in range(K):
        assert np.array_equal(out[k], want[k]), (name, k, int((out[k] != want[k]).sum()))
        assert np.array_equal(cnt[k], wcnt[k]), (name, k)
    assert not np.array_equal(want[0, index:], np.full(cells - index, 7.0, dtype=np.float32).view(np.int32))  # the single-frame leg did run
    if K > 2:
        assert not np.array_equal(out[0], out[1])  # the frames are not one frame K times
    # the batch without count_out writes the same layers
    d_out2 = torch.full((K * cells,), 7.0, dtype=torch.float32, device=dev)
    solver.blur_costmap_batch_device(stream, d_src.data_ptr(), g, thetas, *sigma, d_out2.data_ptr(), index=index, src_stride=stride)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(d_out2), _bits(d_out))
    fout = d_out.cpu().numpy().reshape(K, cells)
    oracle_frames = {}  # (the first and the last frame can be one and the same input: the oracle then runs once)
    for k in sorted({0, K - 1}):
        key = (id(srcs[k]), thetas[k])
        if key not in oracle_frames:
            oracle_frames[key] = oracle.blur(srcs[k], og, np.sin(thetas[k]), np.cos(thetas[k]), *sigma, index=index, threads=min(16, oracle.max_threads()))
        _blur_vs_oracle("%s frame %d" % (name, k), fout[k], cnt[k], oracle_frames[key][0], oracle_frames[key][1], index)


def _blob_map(rng, g, n_blobs=60, nan_frac=0.02):
    """The global layer of test_costmap_frame_equals_its_three_steps."""
    src = np.zeros((g.rows, g.cols), dtype=np.float32, order="F")
    for _ in range(n_blobs):
        i, j = rng.integers(0, g.rows - 30), rng.integers(0, g.cols - 30)
        src[i:i + rng.integers(3, 30), j:j + rng.integers(3, 30)] = 100.0
    src[rng.random(src.shape) < nan_frac] = np.nan
    return src


# the global map spans x in [-57, 63], y in [-62, 58]: frames 3 and 6 reach over its edge
_FRAME_POSES = np.array([[7.5, -4.25, 0.83], [0.0, 0.0, 0.0], [-12.0, 9.5, -1.3], [55.0, 0.0, 0.4], [3.0, 3.0, 3.5], [20.0, -30.0, -2.7],
                         [0.0, -61.0, 2.0], [7.6, -4.2, 0.84], [-30.0, 25.0, 1.57]])


@pytest.mark.gpu
@pytest.mark.parametrize("vgeo", [(30.0, 20.0, 0.2, 10.0 - 5, 0.0), (16.0, 10.0, 0.1, 8.0, 0.0)], ids=["node_150_rows", "res_0.1_160_rows"])
def test_frame_batch_equals_single_frames(cilqr, oracle, solver, vgeo):
    """cilqr_costmap_frame_batch_device against K cilqr_costmap_frame_device calls, all four outputs of every frame bit for bit:
    the node's 150-row vehicle map (the cell-by-cell warp with a frame dimension) and a 0.1 m map with rows in fours (the
    16-byte-store warp), with and without the bbox layer and the OccupancyGrid.  Frame 0 against the oracle's three steps as
    test_costmap_frame_equals_its_three_steps holds them (whose inputs frame 0 of the node geometry has)."""
    import torch
    rng = np.random.default_rng(77)
    sgeo = (120.0, 120.0, 0.2, 3.0, -2.0)
    sg, vg, osg, ovg = cilqr.map_geom(*sgeo), cilqr.map_geom(*vgeo), oracle.map_geom(*sgeo), oracle.map_geom(*vgeo)
    assert vg.rows == (150 if vgeo[2] == 0.2 else 160) and (vg.rows % 4 == 0) == (vgeo[2] == 0.1)
    src = _blob_map(rng, sg)
    bbox = np.zeros((vg.rows, vg.cols), dtype=np.float32, order="F")
    bbox[40:60, 30:45] = 100.0
    poses, K, cells = _FRAME_POSES, len(_FRAME_POSES), vg.rows * vg.cols
    sx, sy, st = 0.16, 0.16, 0.017
    dev = torch.device("cuda", 0)
    d_src, d_bbox = torch.from_numpy(_flat(src)).to(dev), torch.from_numpy(_flat(bbox)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def buffers():
        return (torch.full((K * cells,), 7.0, dtype=torch.float32, device=dev), torch.full((K * cells,), 7.0, dtype=torch.float32, device=dev),
                torch.full((K * cells,), -100, dtype=torch.int8, device=dev), torch.full((K,), -1, dtype=torch.int64, device=dev))

    for with_bbox, with_occ in ((True, True), (False, False), (True, False), (False, True)):
        what = "%s bbox=%s occ=%s" % (vgeo, with_bbox, with_occ)
        b_veh, b_unc, b_occ, b_oob = buffers()
        s_veh, s_unc, s_occ, s_oob = buffers()
        bb = d_bbox.data_ptr() if with_bbox else 0
        solver.costmap_frame_batch_device(stream, d_src.data_ptr(), sg, vg, poses, sx, sy, st, b_veh.data_ptr(), b_unc.data_ptr(),
                                          b_occ.data_ptr() if with_occ else 0, bbox=bb, n_oob=b_oob.data_ptr())
        for k in range(K):
            solver.costmap_frame_device(stream, d_src.data_ptr(), sg, vg, *poses[k], sx, sy, st, s_veh.data_ptr() + 4 * k * cells,
                                        s_unc.data_ptr() + 4 * k * cells, s_occ.data_ptr() + k * cells if with_occ else 0, bbox=bb,
                                        n_oob=s_oob.data_ptr() + 8 * k)
        torch.cuda.synchronize()
        oob = b_oob.cpu().numpy()
        assert np.array_equal(oob, s_oob.cpu().numpy()), what
        assert (oob >= 0).all() and (oob[[3, 6]] > 0).all() and oob[0] == 0, (what, oob)
        veh, unc, occ = _bits(b_veh).reshape(K, cells), _bits(b_unc).reshape(K, cells), b_occ.cpu().numpy().reshape(K, cells)
        wveh, wunc, wocc = _bits(s_veh).reshape(K, cells), _bits(s_unc).reshape(K, cells), s_occ.cpu().numpy().reshape(K, cells)
        for k in range(K):
            assert np.array_equal(veh[k], wveh[k]), (what, k)
            assert np.array_equal(unc[k], wunc[k]), (what, k, int((unc[k] != wunc[k]).sum()))
            assert np.array_equal(occ[k], wocc[k]), (what, k)
        assert (occ >= -1).all() if with_occ else (occ == -100).all(), what  # (-100 is no OccupancyGrid value)
        assert not np.array_equal(unc[0], unc[1])
        # the batch without the counters writes the same layers
        c_veh, c_unc, c_occ, _ = buffers()
        solver.costmap_frame_batch_device(stream, d_src.data_ptr(), sg, vg, poses, sx, sy, st, c_veh.data_ptr(), c_unc.data_ptr(),
                                          c_occ.data_ptr() if with_occ else 0, bbox=bb)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(c_veh), _bits(b_veh)) and np.array_equal(_bits(c_unc), _bits(b_unc)) and torch.equal(c_occ, b_occ), what
        if not (with_bbox and with_occ):
            continue
        # frame 0 against the oracle's warp -> blur -> OccupancyGrid
        vx, vy, th = poses[0]
        w_veh, n_oob = oracle.warp(src, osg, ovg, vx, vy, th, bbox=bbox)
        assert int(oob[0]) == n_oob == 0
        f_veh = b_veh.cpu().numpy()[:cells]
        w_flat = w_veh.reshape(-1, order="F")
        assert np.array_equal(np.isnan(f_veh), np.isnan(w_flat))
        assert np.array_equal(f_veh[~np.isnan(f_veh)], w_flat[~np.isnan(f_veh)])
        w_unc, _, _ = oracle.blur(w_veh, ovg, np.sin(th), np.cos(th), sx, sy, st, threads=min(16, oracle.max_threads()))
        f_unc = b_unc.cpu().numpy()[:cells]
        w_unc = w_unc.reshape(-1, order="F")
        fin = ~np.isnan(w_unc)
        assert np.array_equal(np.isnan(f_unc), ~fin)
        ulp = np.abs(f_unc[fin].view(np.int32).astype(np.int64) - w_unc[fin].view(np.int32).astype(np.int64))
        print("%s frame 0 against the oracle: max ulp %d, bit-equal %.5f" % (what, ulp.max(), (ulp == 0).mean()))
        assert ulp.max() <= 1 and (ulp == 0).mean() >= 0.999
        assert np.array_equal(occ[0], oracle.layer_to_occupancy(f_unc, 0.0, 100.0))
        same = np.ones(cells, dtype=bool)
        same[fin] = ulp == 0
        assert np.array_equal(occ[0][::-1][same], oracle.layer_to_occupancy(w_unc, 0.0, 100.0)[::-1][same])


@pytest.mark.gpu
def test_frame_batch_then_per_solve_maps_on_one_stream(cilqr, oracle):
    """The candidate sequence on ONE side stream with nothing synchronised in between: K pose-noise frames in one
    cilqr_costmap_frame_batch_device call -> their K uncertainty layers and poses set as the per-solve maps -> batched solve ->
    cilqr_argmin_device.  Scene and parameters of test_frame_then_solve_on_one_stream.  The oracle is given the K layers the
    device produced (the frames' own parity is test_frame_batch_equals_single_frames); iterations and exits equal, U, X, J within
    TIGHT = 1e-9 (_compare), the picked index np.argmin of the oracle's J."""
    import torch
    from cilqr_amd import scenes
    from test_gpu_parity import TIGHT, _compare, _unc_params
    N, M, B = 50, 2, 64
    K = B
    p, po = _unc_params(cilqr, N), _unc_params(oracle, N)
    sc = scenes.make_static(B, N, M, p, 977)
    sgeo, vgeo = (120.0, 120.0, 0.2, 10.0, 0.0), (30.0, 20.0, 0.2, 15.0, 0.0)
    sg, vg, ovg = cilqr.map_geom(*sgeo), cilqr.map_geom(*vgeo), oracle.map_geom(*vgeo)
    cells = vg.rows * vg.cols
    glob = scenes.make_occupancy(sg.rows, sg.cols, 5, n_blobs=250, nan_frac=0.0)
    poses = np.array([0.5, -0.3, 0.08]) + np.random.default_rng(113).normal(0.0, 1.0, (K, 3)) * np.array([0.16, 0.16, 0.017])
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    d_glob = torch.from_numpy(np.ascontiguousarray(glob.T)).to(dev)
    d_poses = torch.from_numpy(np.ascontiguousarray(poses)).to(dev)
    veh = torch.zeros(K * cells, dtype=torch.float32, device=dev)
    unc = torch.zeros_like(veh)
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in ("x0", "U", "poly", "xplan_fl", "obs_pose", "obs_dim")}
    X = torch.zeros(B, 4 * (N + 1), dtype=torch.float64, device=dev)
    J = torch.zeros(B, dtype=torch.float64, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    st = torch.zeros(B, dtype=torch.int32, device=dev)
    pick = torch.full((2,), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    s = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        s.costmap_frame_batch_device(side.cuda_stream, d_glob.data_ptr(), sg, vg, poses, 0.16, 0.16, 0.017, veh.data_ptr(), unc.data_ptr())
        s.set_uncertainty_map_device(unc.data_ptr(), vg, (0.0, 0.0, 0.0), (3, 3), layer_stride=cells, poses_ptr=d_poses.data_ptr())
        s.solve_batch_device(side.cuda_stream, B, N, M, t["x0"].data_ptr(), t["U"].data_ptr(), t["poly"].data_ptr(), t["xplan_fl"].data_ptr(),
                             t["obs_pose"].data_ptr(), t["obs_dim"].data_ptr(), 0, X.data_ptr(), J.data_ptr(), it.data_ptr(), st.data_ptr())
        s.argmin_device(side.cuda_stream, B, J.data_ptr(), pick.data_ptr())
        side.synchronize()
    finally:
        s.close()
    layers = unc.cpu().numpy().reshape(K, vg.cols, vg.rows).transpose(0, 2, 1)
    assert all(np.nanmax(layer) > 50 for layer in layers)  # every frame did put obstacles under the planner
    assert sum(not np.array_equal(layers[k], layers[0], equal_nan=True) for k in range(1, K)) >= 1  # at least two frames differ
    um, keep = oracle.uncertainty_map(layers, ovg, (0.0, 0.0, 0.0), (3, 3), poses=poses, batched=True)
    want = oracle.solve_batch_unc(po, N, M, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], sc["obs_pose"], sc["obs_dim"], None, um,
                                  threads=min(16, oracle.max_threads()))
    got = dict(U=t["U"].cpu().numpy(), X=X.cpu().numpy(), J=J.cpu().numpy(), iters=it.cpu().numpy(), status=st.cpu().numpy())
    worst = _compare(got, want, TIGHT, "frame batch -> per-solve maps -> solve")
    print("frame batch -> solve: max|dU| = %.3e" % worst)
    j_min, index = pick.cpu().numpy()
    assert int(index) == int(np.argmin(want["J"])) and j_min == got["J"][int(index)]
