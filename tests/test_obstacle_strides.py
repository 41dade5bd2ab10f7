"""Obstacles given by strides (cilqr_solve_batch_obstacles / _device, include/cilqr.h): one obstacle set shared by the batch,
obstacles constant over the horizon, or both.

The contract checked on the GPU: for any strides the results equal, bit for bit, what cilqr_solve_batch returns on the dense
expansion of the same inputs (np.broadcast_to) — U, X, J, iteration counts and exit reasons — on every kernel family, with and
without an uncertainty map, in the reference-loop mode and on the GENERAL kernels.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT

gpu = pytest.mark.gpu


# ---- CPU: declarations, struct layout, shapes → strides ----------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "cilqr.h")).read()


def test_header_declares_strided_entry_points_and_struct(cilqr):
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("cilqr_solve_batch_obstacles", "cilqr_solve_batch_obstacles_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
        assert name in cilqr.ABI_SYMBOLS
        assert hasattr(cilqr.lib(), name), name
    assert re.search(r"typedef\s+struct\s+cilqr_obstacles\s*\{", h)


def test_obstacles_struct_mirrors_header(cilqr):
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+cilqr_obstacles\s*\{(.*?)\}\s*cilqr_obstacles\s*;", h, re.S).group(1)
    declared = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            declared += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert declared == ["pose", "dim", "weight", "batch_stride", "obstacle_stride", "step_stride", "weight_batch_stride"]
    assert [f for f, _ in cilqr.Obstacles._fields_] == declared
    assert [C.sizeof(t) for _, t in cilqr.Obstacles._fields_] == [8] * 7
    assert C.sizeof(cilqr.Obstacles) == 7 * 8  # three pointers and four int64, no padding


def test_obstacle_strides_shape_forms(cilqr):
    B, N, M = 7, 11, 3
    s = cilqr.obstacle_strides
    assert s((M, 4), (M, 2), None, B, N) == (M, 0, 1, 0, 0)                    # one static set for the batch
    assert s((B, M, 4), (B, M, 2), None, B, N) == (M, M, 1, 0, 0)              # static, one set per solve
    assert s((M, 4 * N), (M, 2 * N), None, B, N) == (M, 0, N, 1, 0)            # one moving set for the batch
    assert s((B, M, 4 * N), (B, M, 2 * N), None, B, N) == (M, M * N, N, 1, 0)  # dense: cilqr_solve_batch's layout
    assert s((M, 4), (M, 2), (M,), B, N)[4] == 0
    assert s((B, M, 4 * N), (B, M, 2 * N), (B, M), B, N)[4] == M


@pytest.mark.parametrize("pose,dim,weight", [
    ((3, 5), (3, 2), None),              # neither 4 nor 4N columns
    ((3, 4), (3, 2 * 11), None),         # pose static, dim per step
    ((3, 4), (2, 2), None),              # obstacle counts differ
    ((6, 3, 4), (6, 3, 2), None),        # batch dimension is not B
    ((3, 4), (3, 2), (7, 2)),            # weights for another M
    ((3, 4), (3, 2), (3, 1)),            # weights neither (M,) nor (B, M)
    ((4,), (2,), None),                  # no obstacle axis
    ((1, 7, 3, 4), (1, 7, 3, 2), None),  # too many axes
])
def test_obstacle_strides_rejects_other_shapes(cilqr, pose, dim, weight):
    with pytest.raises(cilqr.CilqrError):
        cilqr.obstacle_strides(pose, dim, weight, 7, 11)


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------
def _dense(pose, dim, weight, B, N):
    """The dense [B][M][4N] / [2N] / [B][M] expansion of any shape form (what cilqr_solve_batch takes)."""
    M = pose.shape[-2]
    if pose.shape[-1] == 4:
        pose = np.repeat(pose[..., None, :], N, axis=-2).reshape(pose.shape[:-1] + (4 * N,))
        dim = np.repeat(dim[..., None, :], N, axis=-2).reshape(dim.shape[:-1] + (2 * N,))
    pose = np.ascontiguousarray(np.broadcast_to(pose, (B, M, 4 * N)))
    dim = np.ascontiguousarray(np.broadcast_to(dim, (B, M, 2 * N)))
    w = None if weight is None else np.ascontiguousarray(np.broadcast_to(weight, (B, M)))
    return pose, dim, w


def _same(got, want, what):
    for k in ("U", "X", "J", "iters", "status"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs (%d of %d solves)" % (
            what, k, int((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1).sum()), len(got[k]))


def _check_against_dense(solver, sc, pose, dim, weight=None, flags=0, what=""):
    N, B = sc["N"], sc["x0"].shape[0]
    got = solver.solve_batch_obstacles(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], pose, dim, weight, flags=flags)
    dp, dd, dw = _dense(pose, dim, weight, B, N)
    want = solver.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], dp, dd, dw, flags=flags)
    _same(got, want, what)
    return got


def _forms(sc, moving=None):
    """{name: (pose, dim)}: shared static (M,4), static per solve (B,M,4) and, given (M,4N) moving tables, shared moving."""
    B, M, N = sc["x0"].shape[0], sc["M"], sc["N"]
    pose = sc["obs_pose"].reshape(B, M, N, 4)
    dim = sc["obs_dim"].reshape(B, M, N, 2)
    out = {"shared static": (pose[0, :, 0].copy(), dim[0, :, 0].copy()),
           "static per solve": (pose[:, :, 0].copy(), dim[:, :, 0].copy())}
    if moving is not None:
        out["shared moving"] = moving
    return out


def _moving(M, N, dt, seed):
    from cilqr_amd import scenes
    rng = np.random.default_rng(seed)
    curve = (np.array([1.5]), np.array([0.05]), np.array([0.3]))
    pose, dim = scenes._obstacles(rng, curve, 1, M, N, dt, 4.0)
    return pose[0].reshape(M, 4 * N), dim[0].reshape(M, 2 * N)


# ---- GPU: config 2, one scene for many candidates, the grouped family, the table in the workspace --------------------------
@gpu
def test_config2_static_per_solve(cilqr, oracle):
    """Config 2 as static per solve (B, M, 4): bit-identical to the dense call on the share kernel, and within 1e-9 of the
    oracle on a 64-solve sample."""
    from cilqr_amd import scenes
    N, M, B = 50, 4, 1024
    p = cilqr.default_params(N)
    sc = scenes.make_c2(B, p)
    pose = sc["obs_pose"].reshape(B, M, N, 4)
    dim = sc["obs_dim"].reshape(B, M, N, 2)
    assert np.array_equal(pose, np.broadcast_to(pose[:, :, :1], pose.shape))  # config 2's obstacles do not move
    assert np.array_equal(dim, np.broadcast_to(dim[:, :, :1], dim.shape))
    s = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        assert s.solve_wavefronts(B, N, M) > 1
        got = _check_against_dense(s, sc, pose[:, :, 0].copy(), dim[:, :, 0].copy(), what="config 2 static per solve")
    finally:
        s.close()
    k = 64
    sub = {key: sc[key][:k] for key in ("x0", "U", "poly", "xplan_fl", "obs_pose", "obs_dim")}
    want = oracle.solve_batch(oracle.default_params(N), N, M, sub["x0"], sub["U"], sub["poly"], sub["xplan_fl"], sub["obs_pose"],
                              sub["obs_dim"], None, threads=min(16, oracle.max_threads()))
    assert np.max(np.abs(got["U"][:k] - want["U"])) <= 1e-9
    assert np.array_equal(got["iters"][:k], want["iters"])


def _candidates(cilqr, solver, B, N, seed):
    """B candidates around one ego pose on one path (the node's pose noise): the device pre-step on the shared path."""
    rng = np.random.default_rng(seed)
    x = np.arange(0.0, 200.0, 1.0)
    path = np.stack([x, 1.5 * np.sin(0.05 * x + 0.3)], axis=1)
    ego = np.array([20.0, 1.5 * np.sin(1.3), 4.0, 0.05])
    egos = ego + rng.normal(0.0, 1.0, (B, 4)) * np.array([0.3, 0.3, 0.2, 0.03])
    plan = solver.local_plan_batch(path, egos)
    U = np.tile(cilqr.default_control_seq(N), (B, 1))
    return dict(N=N, x0=egos, U=U, poly=plan["poly"], xplan_fl=plan["xplan_fl"])


@gpu
def test_one_scene_for_many_candidates(cilqr):
    """B = 256 candidates, one obstacle set: moving (M, 4N) and static (M, 4); plain, with a map, reference-loop mode, GENERAL."""
    from cilqr_amd import scenes
    N, M, B = 50, 4, 256
    p = cilqr.default_params(N)
    s = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        sc = _candidates(cilqr, s, B, N, 5)
        mp, md = _moving(M, N, p.timestep, 6)
        forms = {"shared moving": (mp, md),
                 "shared static": (mp.reshape(M, N, 4)[:, 0].copy(), md.reshape(M, N, 2)[:, 0].copy())}
        geom = cilqr.map_geom(60.0, 20.0, 0.2, 30.0, 0.0)
        layer = np.nan_to_num(scenes.make_occupancy(geom.rows, geom.cols, 3), nan=0.0)
        for mode, flags in (("plain", 0), ("map", 0), ("faithful", cilqr.FLAG_FAITHFUL_ITERS), ("general", cilqr.FLAG_GENERAL_ONLY)):
            if mode == "map":
                s.set_uncertainty_map(layer, geom, (-20.0, 0.0, 0.0), (3, 3))
            for name, (pose, dim) in forms.items():
                _check_against_dense(s, sc, pose, dim, flags=flags, what="%s, %s" % (name, mode))
            if mode == "map":
                s.clear_uncertainty_map()
    finally:
        s.close()


@pytest.fixture(scope="module")
def big_solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=8192, max_horizon=80, max_obstacles=16, device=0)
    yield s
    s.close()


@gpu
@pytest.mark.parametrize("N,M", [(50, 4), (80, 16)])
def test_grouped_family(cilqr, big_solver, N, M):
    """B = 8192 on the grouped family: shared static, shared moving and static per solve; the shared forms read one table built
    in front of the kernels.  Then every solve through the GENERAL kernel (FLAG_GENERAL_ONLY), reading that shared table."""
    from cilqr_amd import scenes
    B = 8192
    p = cilqr.default_params(N)
    assert big_solver.solve_family(B, N, M) < 64
    sc = scenes.make_static(B, N, M, p, 4242 + N)
    forms = _forms(sc, _moving(M, N, p.timestep, 7 + N))
    for name, (pose, dim) in forms.items():
        _check_against_dense(big_solver, sc, pose, dim, what="grouped %s N=%d M=%d" % (name, N, M))
    for name in ("shared static", "shared moving"):
        pose, dim = forms[name]
        _check_against_dense(big_solver, sc, pose, dim, flags=cilqr.FLAG_GENERAL_ONLY, what="grouped GENERAL %s N=%d" % (name, N))


@gpu
def test_wave_family_table_in_workspace(cilqr):
    """B = 1024, N = 50, M = 40: one wavefront per solve with the 96 000-byte table past the LDS budget (TAB = 0 kernels); one
    shared scene, then the same through the GENERAL kernel."""
    from cilqr_amd import scenes
    N, M, B = 50, 40, 1024
    p = cilqr.default_params(N)
    s = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        assert s.solve_family(B, N, M) == 64 and s.solve_wavefronts(B, N, M) == 1
        sc = scenes.make_static(B, N, M, p, 777)
        mp, md = _moving(M, N, p.timestep, 8)
        for flags in (0, cilqr.FLAG_GENERAL_ONLY):
            _check_against_dense(s, sc, mp, md, flags=flags, what="wave TAB=0 shared moving, flags %d" % flags)
            _check_against_dense(s, sc, *_forms(sc)["shared static"], flags=flags, what="wave TAB=0 shared static, flags %d" % flags)
    finally:
        s.close()


@gpu
def test_weights(cilqr, big_solver):
    """Weights shared (M,), per solve (B, M) and NULL, on the share kernel (config 2) and on the grouped family's shared table."""
    from cilqr_amd import scenes
    N, M = 50, 4
    p = cilqr.default_params(N)
    rng = np.random.default_rng(9)
    for B in (1024, 8192):
        sc = scenes.make_static(B, N, M, p, 99 + B)
        for name, (pose, dim) in _forms(sc).items():
            for wname, w in (("shared", rng.uniform(0.5, 2.0, M)), ("per solve", rng.uniform(0.5, 2.0, (B, M))), ("none", None)):
                _check_against_dense(big_solver, sc, pose, dim, w, what="B=%d %s, weights %s" % (B, name, wname))


@gpu
def test_device_entry_and_pinned_memory(cilqr):
    """The device entry point with torch tensors on a side stream equals the host entry point; pinned buffers equal pageable."""
    import torch
    from cilqr_amd import scenes
    N, M, B = 50, 4, 512
    p = cilqr.default_params(N)
    s = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        sc = scenes.make_static(B, N, M, p, 31)
        w = np.random.default_rng(2).uniform(0.5, 2.0, M)
        for name, (pose, dim) in _forms(sc, _moving(M, N, p.timestep, 3)).items():
            host = s.solve_batch_obstacles(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], pose, dim, w)
            pin = {k: cilqr.pinned_copy(v) for k, v in (("x0", sc["x0"]), ("poly", sc["poly"]), ("xplan_fl", sc["xplan_fl"]),
                                                         ("pose", pose), ("dim", dim), ("w", w))}
            out = {"U": cilqr.pinned_copy(sc["U"]), "X": cilqr.pinned_empty((B, 4 * (N + 1))), "J": cilqr.pinned_empty((B,)),
                   "iters": cilqr.pinned_empty((B,), np.int32), "status": cilqr.pinned_empty((B,), np.int32)}
            pinned = s.solve_batch_obstacles(N, pin["x0"], None, pin["poly"], pin["xplan_fl"], pin["pose"], pin["dim"], pin["w"], out=out)
            _same(pinned, host, "pinned %s" % name)

            dev = torch.device("cuda", 0)
            t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in (("x0", sc["x0"]), ("U", sc["U"]), ("poly", sc["poly"]),
                                                                                  ("fl", sc["xplan_fl"]), ("pose", pose), ("dim", dim), ("w", w))}
            X = torch.zeros((B, 4 * (N + 1)), dtype=torch.float64, device=dev)
            J = torch.zeros(B, dtype=torch.float64, device=dev)
            it = torch.zeros(B, dtype=torch.int32, device=dev)
            st = torch.zeros(B, dtype=torch.int32, device=dev)
            _, bs, ms, ts, wbs = cilqr.obstacle_strides(pose.shape, dim.shape, w.shape, B, N)
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                s.solve_batch_obstacles_device(side.cuda_stream, B, N, M, t["x0"].data_ptr(), t["U"].data_ptr(), t["poly"].data_ptr(),
                                               t["fl"].data_ptr(), t["pose"].data_ptr(), t["dim"].data_ptr(), t["w"].data_ptr(),
                                               (bs, ms, ts, wbs), X.data_ptr(), J.data_ptr(), it.data_ptr(), st.data_ptr())
            side.synchronize()
            _same(dict(U=t["U"].cpu().numpy(), X=X.cpu().numpy(), J=J.cpu().numpy(), iters=it.cpu().numpy(), status=st.cpu().numpy()),
                  host, "device entry %s" % name)
    finally:
        s.close()


@gpu
def test_errors_leave_the_handle_usable(cilqr):
    """Negative stride, NULL obs with M > 0, M > max_obstacles: -1 (CILQR_ERR_ARG); the handle solves correctly after each."""
    from cilqr_amd import scenes
    N, M, B = 30, 3, 64
    p = cilqr.default_params(N)
    s = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        sc = scenes.make_static(B, N, M, p, 12)
        pose, dim = _forms(sc)["shared static"]
        want = s.solve_batch(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], *_dense(pose, dim, None, B, N))
        L = cilqr.lib()
        dp = C.POINTER(C.c_double)
        x0, poly, fl = (np.ascontiguousarray(sc[k]) for k in ("x0", "poly", "xplan_fl"))
        U = np.ascontiguousarray(sc["U"]).copy()
        X, J = np.zeros((B, 4 * (N + 1))), np.zeros(B)
        it, st = np.zeros(B, np.int32), np.zeros(B, np.int32)

        def call(m, obs):
            return L.cilqr_solve_batch_obstacles(s._h, B, N, m, x0.ctypes.data_as(dp), U.ctypes.data_as(dp), poly.ctypes.data_as(dp),
                                                 fl.ctypes.data_as(dp), None if obs is None else C.byref(obs), X.ctypes.data_as(dp),
                                                 J.ctypes.data_as(dp), it.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 st.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(0))

        for bad in ("negative", "null", "too many"):
            if bad == "negative":
                rc = call(M, cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, 0, -1, 0, 0))
            elif bad == "null":
                rc = call(M, None)
            else:
                rc = call(M + 1, cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, 0, 1, 0, 0))
            assert rc == -1, bad
            got = s.solve_batch_obstacles(N, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], pose, dim)
            _same(got, want, "after %s" % bad)
    finally:
        s.close()


@gpu
def test_cpp_facade_candidates_share_one_obstacle_set(tmp_path):
    """tests/cpp/candidates_shared_obstacles.cpp: iLQR::run_candidates (one obstacle set for every candidate) against a
    hand-written dense cilqr_solve_batch and the strict-< minimum pick, bit for bit, with static and with moving obstacles."""
    import subprocess
    exe = str(tmp_path / "candidates_shared_obstacles")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_shared_obstacles.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bit-identical" in r.stdout, r.stdout
