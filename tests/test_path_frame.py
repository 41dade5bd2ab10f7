"""The path-aligned planning frame on the CPU: the oracle's solves on inputs the numpy restatement (tests/path_frame_ref.py) took
into the frame.  What is checked here is the DEFINITION of include/cilqr.h — that planning in the frame makes the plan independent
of where the road lies and which way it points — and what the unframed pre-step does instead.  The kernels are held to the same
restatement bit for bit in tests/test_path_frame_gpu.py.

N = 30, default parameters, fresh warm start throughout.  Each test prints its figures before it asserts.
"""
import functools
import math

import numpy as np

import path_frame_ref as R

N = 30
DIM = np.array([[4.79, 2.16]] * 2)
OBS = np.array([[15.0, 0.8, 0.0, 0.0], [27.0, -1.0, 0.0, 0.1]])  # two static obstacles
EGO = np.array([0.0, 0.1, 3.0, 0.02])


def _east():
    i = np.arange(200.0)
    return np.stack([i, np.zeros(200)], axis=1)


def _known_answer_path():
    i = np.arange(200.0)
    return np.stack([i, 0.5 * np.sin(0.05 * i)], axis=1)


def _unframed(O, p, path, ego, obs):
    c, ref = O.local_plan(p, path, ego)
    M = len(obs)
    pose = np.broadcast_to(obs[:, None, :], (M, N, 4)).reshape(M, 4 * N)
    dim = np.broadcast_to(DIM[:, None, :], (M, N, 2)).reshape(M, 2 * N)
    r = O.solve(p, N, ego, O.default_control_seq(N), c, ref[0, 0], ref[-1, 0], pose, dim)
    r["poly"], r["xplan_fl"] = c, (ref[0, 0], ref[-1, 0])
    return r


@functools.lru_cache(maxsize=None)
def _base(kind):
    """The framed solve of the unmoved scene, computed once."""
    from oracle import oracle as O
    p = O.default_params(N)
    path = _east() if kind == "east" else _known_answer_path()
    return R.framed_solve(O, p, N, path, EGO, O.default_control_seq(N), OBS, DIM)


def test_east_road_the_frame_changes_nothing(oracle):
    """A road along x from the origin: the frame is the map frame and the framed solve is the unframed one."""
    p = oracle.default_params(N)
    u = _unframed(oracle, p, _east(), EGO, OBS)
    f = _base("east")
    dX = np.abs(f["X_map"].ravel() - u["X"]).max()
    print("path_frame east: unframed J=%.17g iters=%d | framed J=%.17g iters=%d | max|dX|=%.3g" % (u["J"], u["iters"], f["J"], f["iters"], dX))
    assert f["plan"]["info"] == 0 and f["plan"]["frame"].tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert abs(u["J"] - 124.583165733) <= 1e-6 and u["iters"] == 16  # the figures README.md quotes
    assert f["iters"] == u["iters"] and f["status"] == u["status"] and abs(f["J"] - u["J"]) <= 1e-12 * abs(u["J"]) and dX <= 1e-12


def test_north_road_unframed_plan_is_degenerate_framed_plan_is_the_east_plan(oracle):
    """The same road and obstacles turned to head north (x = 3 everywhere).  Unframed, the slice's abscissae coincide: x_local_plan's
    first and last element are equal, the fit is a constant, the solve still reports a healthy status and its cost is several times
    the east road's.  Framed, the solve is the east road's: J, iterations, and U within 1e-12; X comes back as the east plan turned."""
    p = oracle.default_params(N)
    path, ego, obs = R.move_scene(math.pi / 2, (3.0, 0.0), _east(), EGO, OBS)
    assert np.all(path[:, 0] == 3.0)
    u = _unframed(oracle, p, path, ego, obs)
    e = _base("east")
    f = R.framed_solve(oracle, p, N, path, ego, oracle.default_control_seq(N), obs, DIM)
    dU = np.abs(f["U"] - e["U"]).max()
    ex, ey = e["X_map"][:, 0], e["X_map"][:, 1]
    dX = max(np.abs(f["X_map"][:, 0] - (3.0 - ey)).max(), np.abs(f["X_map"][:, 1] - ex).max())
    print("path_frame north: unframed xplan_fl=%r poly=%r J=%.6g iters=%d status=%d | framed J=%.17g iters=%d max|dU|=%.3g max|dX|=%.3g"
          % (u["xplan_fl"], u["poly"].tolist(), u["J"], u["iters"], u["status"], f["J"], f["iters"], dU, dX))
    assert u["xplan_fl"][0] == u["xplan_fl"][1]
    assert abs(u["J"] - 660.349) <= 1e-2 and u["iters"] == 13 and abs(u["poly"][5] - 0.039) <= 1e-3  # the figures README.md quotes
    assert np.all(u["poly"][:5] == 0.0) and u["status"] == e["status"] and u["J"] > 3.0 * e["J"]
    assert f["plan"]["info"] == 0
    assert f["iters"] == e["iters"] and f["status"] == e["status"] and abs(f["J"] - e["J"]) <= 1e-12 * abs(e["J"]) and dU <= 1e-12
    assert dX <= 1e-12


def test_slice_that_doubles_back_in_x(oracle):
    """(i, 0.5 sin 0.05 i) turned by a quarter turn, ego at waypoint 25: the slice's map abscissae double back, the unframed fit has
    coefficients of order 1e7 and a cost several times the framed one; in the frame the abscissae increase and nothing is flagged."""
    p = oracle.default_params(N)
    ego = np.array([25.0, 0.5 * math.sin(1.25), 3.0, 0.02])
    path, ego, obs = R.move_scene(math.pi / 2, (0.0, 0.0), _known_answer_path(), ego, OBS)
    u = _unframed(oracle, p, path, ego, obs)
    f = R.framed_solve(oracle, p, N, path, ego, oracle.default_control_seq(N), obs, DIM)
    x = path[25:45, 0]
    print("path_frame doubled back: unframed max|poly|=%.3g J=%.6g | framed J=%.6g info=%d" % (np.abs(u["poly"]).max(), u["J"], f["J"], f["plan"]["info"]))
    assert not np.all(x[1:] > x[:-1]) and not np.all(x[1:] < x[:-1])
    assert np.abs(u["poly"]).max() > 1e6 and u["J"] > 2.0 * f["J"]
    assert abs(u["J"] - 487.49) <= 1e-1 and abs(f["J"] - 123.67) <= 1e-2  # the figures README.md quotes (the unframed fit is ill-conditioned)
    assert f["plan"]["info"] == 0 and f["plan"]["first"] == 25


ROTATIONS = (0.5, math.pi / 2, 2.4, math.pi, -math.pi / 2)
OFFSETS = ((0.0, 0.0), (300.0, -200.0), (1e5, 5e5))


def test_framed_pipeline_is_invariant_under_rotation_and_translation(oracle):
    """The known-answer scene turned by {0.5, pi/2, 2.4, pi, -pi/2} and moved by up to (1e5, 5e5): U of the framed pipeline stays
    within 1e-9 of the unmoved scene's (the project's bar for parity), iterations and status equal.  Unframed, turning the scene by
    0.5 rad alone moves U[0] by 1e-4."""
    p = oracle.default_params(N)
    path, base = _known_answer_path(), _base("known")
    worst = 0.0
    for a in ROTATIONS:
        for t in OFFSETS:
            pp, ee, oo = R.move_scene(a, t, path, EGO, OBS)
            r = R.framed_solve(oracle, p, N, pp, ee, oracle.default_control_seq(N), oo, DIM)
            dU = np.abs(r["U"] - base["U"]).max()
            print("path_frame invariance: turn %.4f offset %r: max|dU|=%.3g iters=%d" % (a, t, dU, r["iters"]))
            assert r["iters"] == base["iters"] and r["status"] == base["status"] and r["plan"]["info"] == 0
            assert dU <= 1e-9
            worst = max(worst, dU)
    u0 = _unframed(oracle, p, path, EGO, OBS)
    pp, ee, oo = R.move_scene(0.5, (0.0, 0.0), path, EGO, OBS)
    u1 = _unframed(oracle, p, pp, ee, oo)
    print("path_frame invariance: framed worst max|dU|=%.3g; unframed, turned by 0.5: max|dU|=%.3g" % (worst, np.abs(u1["U"] - u0["U"]).max()))
    assert np.abs(u1["U"] - u0["U"]).max() > 1e3 * max(worst, 1e-12)


def test_global_inflation_restores_the_map_frames_semi_axes(oracle):
    """With CILQR_FRAME_GLOBAL_INFLATION the semi-axes the reference's formula (I/Obstacle.cpp:41-43) gives on the compensated frame
    rows equal those on the map rows within 1e-12, for v in {0, 3, 8} and ten headings; without it a moving obstacle's differ."""
    p = oracle.default_params(N)
    frame, _ = R.make_frame((2.0, -1.0), (2.0 + math.cos(0.9), -1.0 + math.sin(0.9)), 2)

    def axes(pose, dim):
        a = dim[..., 0] / 2.0 + np.abs(pose[..., 2] * np.cos(pose[..., 3])) * p.t_safe + p.s_safe_a + p.ego_rad
        b = dim[..., 1] / 2.0 + np.abs(pose[..., 2] * np.sin(pose[..., 3])) * p.t_safe + p.s_safe_b + p.ego_rad + 1
        return a, b

    th = np.linspace(-3.0, 3.0, 10)
    worst = plain = 0.0
    for v in (0.0, 3.0, 8.0):
        pose = np.stack([np.full(10, 20.0), np.full(10, 1.0), np.full(10, v), th], axis=1).reshape(1, 1, 10, 4)
        dim = np.broadcast_to(np.array([4.79, 2.16]), (1, 1, 10, 2))
        want = axes(pose, dim)
        on = R.frame_obstacles(frame[None], pose, dim, t_safe=p.t_safe, flags=R.GLOBAL_INFLATION)
        off = R.frame_obstacles(frame[None], pose, dim, t_safe=p.t_safe, flags=0)
        got, raw = axes(on["pose"], on["dim"]), axes(off["pose"], off["dim"])
        d = max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())
        dr = max(np.abs(raw[0] - want[0]).max(), np.abs(raw[1] - want[1]).max())
        print("path_frame inflation: v=%g compensated max|d semi-axis|=%.3g, uncompensated %.3g" % (v, d, dr))
        assert d <= 1e-12
        assert np.array_equal(off["dim"], dim)
        if v == 0.0:
            assert np.array_equal(on["dim"], dim) and dr <= 1e-12
        else:
            plain = max(plain, dr)
        worst = max(worst, d)
    assert plain > 0.1  # the quirk is real: metres, not rounding
