"""The path-aligned planning frame on the device: cilqr_local_plan_frames, cilqr_frame_obstacles, cilqr_frame_states and
cilqr_frame_poses against the numpy restatement of include/cilqr.h (tests/path_frame_ref.py).

Positions, dimensions, covariances, first, n, the info word, (ox, oy, c, s) and the fit are compared BIT FOR BIT.  Two things are
not: phi = atan2(s, c), where the device's atan2 and the host's libm may round differently, and the ego heading theta - phi that
inherits it.  HEADING_ULPS below is twice the largest difference measured over the pre-step cases of this file and 10 000 seeded
chords, a quarter of them packed around the axes and diagonals: 1.000 ulp (profiles/r32_path_frame.txt, written by
tools/path_frame_ab.py; each case here prints its figure before the assertion).  The factor two is because the seeded set is a
sample.  The unit is the ulp of PHI — the spacing of doubles at max(|phi|, |value|)
— not the ulp of the ego heading, which is finer where |theta - phi| is small; the ego heading is ALSO held, bit for bit, to
theta - phi on the device's own phi.  The transforms take frames as INPUT, so their headings are exact again.

With CILQR_FRAME_GLOBAL_INFLATION the kernel takes sines and cosines from the kernels' own sincos (tests/test_device_math.py holds
it to 2 ulp); the restatement is handed the same routine through Solver.debug_math, so that every other operation is still held
to bits.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import path_frame_ref as R

pytestmark = pytest.mark.gpu

HEADING_ULPS = 2.0  # twice the measured 1.000 (profiles/r32_path_frame.txt)
W0 = 20
ERR_ARG = -1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same_bits_or_nan(a, b):
    """Bits where the restatement is a number; where it is NaN (a NaN ego) a NaN, whatever its sign and payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def heading_ulps(got, want, phi):
    """|got - want| in spacings of doubles at max(|phi|, |want|)."""
    got, want, phi = np.asarray(got), np.asarray(want), np.asarray(phi)
    unit = np.spacing(np.maximum(np.abs(phi), np.abs(want)))
    return float(np.max(np.abs(got - want) / unit)) if got.size else 0.0


@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(30), max_batch=64, max_horizon=65, max_obstacles=3, device=0)
    yield s
    s.close()


# ---------------------------------------------------------------------------------------------------------------- the pre-step
def _compare_prestep(label, got, want, egos):
    """Bits everywhere but phi and the ego heading; returns the largest heading difference in ulps."""
    worst = 0.0
    for b, w in enumerate(want):
        n = w["n"]
        at = (label, b)
        assert int(got["first"][b]) == w["first"] and int(got["n"][b]) == n and int(got["info"][b]) == w["info"], at
        assert _same_bits(got["frames"][b, :4], w["frame"][:4]), at
        assert _same_bits_or_nan(got["ego"][b, :3], w["ego"][:3]), at
        assert _same_bits(got["xplan_fl"][b], w["xplan_fl"]), at
        assert _same_bits(got["ref_traj"][b, :n, 0], w["ref"][:, 0]), at
        assert _same_bits(got["poly"][b], w["poly"]), (at, got["poly"][b], w["poly"])
        assert _same_bits(got["ref_traj"][b, :n, 1], w["ref"][:, 1]), at
        phi, phi_w = got["frames"][b, 4], w["frame"][4]
        worst = max(worst, heading_ulps(phi, phi_w, phi_w))
        if not np.isnan(egos[b, 3]):
            worst = max(worst, heading_ulps(got["ego"][b, 3], w["ego"][3], phi_w))
            assert _same_bits(got["ego"][b, 3], egos[b, 3] - phi), at  # theta - phi on the device's own phi: exact
        else:
            assert np.isnan(got["ego"][b, 3])
    return worst


def test_prestep_against_the_restatement(cilqr, oracle, solver):
    infos, worst = set(), 0.0
    for label, paths, egos in R.prestep_cases():
        want = R.restated(oracle, paths, egos)
        got = solver.local_plan_frames(paths, egos)
        w = _compare_prestep(label, got, want, egos)
        print("path_frame prestep %-14s B=%-2d first=%s n=%s info=%s heading ulps=%.2f"
              % (label, egos.shape[0], sorted({x["first"] for x in want}), sorted({x["n"] for x in want}), sorted({x["info"] for x in want}), w))
        infos |= {x["info"] for x in want}
        worst = max(worst, w)
    assert infos >= {0, R.DEGENERATE, R.NOT_MONOTONE, R.DEGENERATE | R.NOT_MONOTONE}
    assert worst <= HEADING_ULPS, worst


def test_prestep_device_form_and_strided_paths(cilqr, oracle, solver):
    """The device form on windows over one long path (path_stride = one waypoint) and without the optional outputs."""
    import torch
    B, P = 33, 25
    rng = np.random.default_rng(3202)
    L = B - 1 + P
    t = 0.8 * np.arange(L)
    long_path = np.stack([50.0 + t * math.cos(2.0) + 0.6 * np.sin(0.3 * t), -20.0 + t * math.sin(2.0)], axis=1)
    win = np.stack([long_path[b:b + P] for b in range(B)])
    k = rng.integers(0, P, B)
    egos = np.stack([win[np.arange(B), k, 0] + 0.1, win[np.arange(B), k, 1] - 0.1, np.full(B, 3.0), rng.uniform(-3, 3, B)], axis=1)
    want = R.restated(oracle, win, egos)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
    dp, de = d(long_path), d(egos)
    fr, info, eo, poly, fl, ref = z(B, 5), z(B, dt=torch.int32), z(B, 4), z(B, 6), z(B, 2), z(B, W0, 2)
    n, first = z(B, dt=torch.int32), z(B, dt=torch.int32)
    fr2, info2, eo2, poly2, fl2 = z(B, 5), z(B, dt=torch.int32), z(B, 4), z(B, 6), z(B, 2)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    solver.local_plan_frames_device(st, B, P, dp.data_ptr(), 2, de.data_ptr(), fr.data_ptr(), info.data_ptr(), eo.data_ptr(), poly.data_ptr(),
                                    fl.data_ptr(), ref.data_ptr(), n.data_ptr(), first.data_ptr())
    solver.local_plan_frames_device(st, B, P, dp.data_ptr(), 2, de.data_ptr(), fr2.data_ptr(), info2.data_ptr(), eo2.data_ptr(),
                                    poly2.data_ptr(), fl2.data_ptr())
    torch.cuda.synchronize()
    got = dict(frames=fr.cpu().numpy(), info=info.cpu().numpy(), ego=eo.cpu().numpy(), poly=poly.cpu().numpy(), xplan_fl=fl.cpu().numpy(),
               ref_traj=ref.cpu().numpy(), n=n.cpu().numpy(), first=first.cpu().numpy())
    worst = _compare_prestep("windows", got, want, egos)
    print("path_frame prestep windows: B=%d heading ulps=%.2f" % (B, worst))
    assert worst <= HEADING_ULPS
    assert len({w["first"] for w in want}) > 5
    for a, b in ((fr, fr2), (eo, eo2), (poly, poly2), (fl, fl2)):
        assert _same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert np.array_equal(info.cpu().numpy(), info2.cpu().numpy())
    host = solver.local_plan_frames(win, egos)  # host form = device form
    for key in ("frames", "ego", "poly", "xplan_fl", "ref_traj"):
        assert _same_bits(host[key], got[key]), key
    for key in ("info", "n", "first"):
        assert np.array_equal(host[key], got[key]), key


# ---------------------------------------------------------------------------------------------------------------- the transforms
def _frames(rng, B):
    """Frame records as the pre-step would write them, one of them degenerate."""
    out = []
    for b in range(B):
        o = rng.uniform(-500, 500, 2)
        a = rng.uniform(-math.pi, math.pi)
        f, _ = R.make_frame(o, o + rng.uniform(5, 30) * np.array([math.cos(a), math.sin(a)]), 2 if b != 1 else 1)
        out.append(f)
    return np.array(out)


def _device_sincos(cilqr, solver):
    def sincos(th):
        r = solver.debug_math(cilqr.MATH_SINCOS_FAST, np.ascontiguousarray(th).reshape(-1))
        return r[:, 0].reshape(np.shape(th)), r[:, 1].reshape(np.shape(th))
    return sincos


@pytest.mark.parametrize("N", (1, 64, 65))
@pytest.mark.parametrize("M", (1, 3))
def test_frame_obstacles_bits(cilqr, solver, N, M):
    """Dense, (0, N, 1) and (0, 1, 0) strides; frame_stride 0 and 5; with and without covariances; both flag values."""
    rng = np.random.default_rng(3210 + 10 * N + M)
    B = 5
    frames = _frames(rng, B)
    t_safe = solver.params.t_safe
    sincos = _device_sincos(cilqr, solver)

    def draw(*lead):
        pose = np.concatenate([rng.uniform(-400, 400, lead + (2,)), rng.choice([0.0, 3.0, 8.0], lead + (1,)), rng.uniform(-3.1, 3.1, lead + (1,))], axis=-1)
        dim = rng.uniform(1.0, 5.0, lead + (2,))
        a, b = rng.uniform(0.05, 0.6, lead), rng.uniform(0.05, 0.6, lead)
        rho = rng.uniform(-0.9, 0.9, lead)
        return pose, dim, np.stack([a * a, rho * a * b, b * b], axis=-1)

    layouts = {"dense": draw(B, M, N), "shared moving": draw(M, N), "shared static": draw(M)}
    for name, (pose, dim, cov) in layouts.items():
        if name == "dense":
            args = (pose.reshape(B, M, 4 * N), dim.reshape(B, M, 2 * N), cov.reshape(B, M, 3 * N))
            full = (pose, dim, cov)
        elif name == "shared moving":
            args = (pose.reshape(M, 4 * N), dim.reshape(M, 2 * N), cov.reshape(M, 3 * N))
            full = tuple(np.broadcast_to(a[None], (B,) + a.shape) for a in (pose, dim, cov))
        else:
            args = (pose, dim, cov)
            full = tuple(np.broadcast_to(a[None, :, None, :], (B, M, N, a.shape[-1])) for a in (pose, dim, cov))
        for fr, fr_full in ((frames, frames), (frames[3], np.broadcast_to(frames[3], (B, 5)))):
            for flag in (False, True):
                for with_cov in (False, True):
                    got = solver.frame_obstacles(B, N, fr, args[0], args[1], args[2] if with_cov else None, global_inflation=flag)
                    want = R.frame_obstacles(fr_full, full[0], full[1], full[2] if with_cov else None, t_safe=t_safe,
                                             flags=R.GLOBAL_INFLATION if flag else 0, sincos=sincos)
                    at = (name, fr.shape, flag, with_cov)
                    assert _same_bits(got["pose"].reshape(B, M, N, 4), want["pose"]), at
                    assert _same_bits(got["dim"].reshape(B, M, N, 2), want["dim"]), at
                    if with_cov:
                        assert _same_bits(got["cov"].reshape(B, M, N, 3), want["cov"]), at
                    else:
                        assert got["cov"] is None
                    if flag:  # static entries keep their dimensions, moving ones do not
                        still = np.broadcast_to(full[0][..., 2] == 0.0, (B, M, N))
                        assert _same_bits(got["dim"].reshape(B, M, N, 2)[still], np.broadcast_to(full[1], (B, M, N, 2))[still])
                        assert still.all() or not _same_bits(got["dim"].reshape(B, M, N, 2), np.broadcast_to(full[1], (B, M, N, 2)))


def test_frame_obstacles_host_form_at_the_handles_sizes(cilqr, solver):
    """B = max_batch, M = max_obstacles, N = max_horizon, dense rows and covariances: 18 M N doubles per solve, three times what the
    arena of the other host forms reserves for one.  The host form takes it (its table travels through scratch of its own)."""
    rng = np.random.default_rng(3260)
    B, M, N = 64, 3, 65
    frames = _frames(rng, B)
    pose = np.concatenate([rng.uniform(-400, 400, (B, M, N, 2)), rng.uniform(0, 8, (B, M, N, 1)), rng.uniform(-3, 3, (B, M, N, 1))], axis=-1)
    dim, cov = rng.uniform(1, 5, (B, M, N, 2)), rng.uniform(0.05, 0.3, (B, M, N, 3))
    got = solver.frame_obstacles(B, N, frames, pose.reshape(B, M, 4 * N), dim.reshape(B, M, 2 * N), cov.reshape(B, M, 3 * N))
    want = R.frame_obstacles(frames, pose, dim, cov)
    assert _same_bits(got["pose"].reshape(B, M, N, 4), want["pose"]) and _same_bits(got["dim"].reshape(B, M, N, 2), want["dim"])
    assert _same_bits(got["cov"].reshape(B, M, N, 3), want["cov"])


def test_frame_obstacles_without_obstacles(cilqr, solver):
    """M = 0: nothing to write, nothing launched, no error."""
    rc = cilqr.lib().cilqr_frame_obstacles(solver._h, 4, 10, 0, np.zeros(5).ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(0), None, None,
                                           C.c_uint32(0), None, None, None)
    assert rc == 0


@pytest.mark.parametrize("N", (1, 64, 65))
@pytest.mark.parametrize("S", (1, 3))
def test_frame_states_bits(cilqr, solver, N, S):
    """Both directions, out of place (host form) and in place (device form), frame_stride 5 and 0."""
    import torch
    rng = np.random.default_rng(3230 + 10 * N + S)
    B = 7
    frames = _frames(rng, B)
    X = np.concatenate([rng.uniform(-600, 600, (B * S, N + 1, 2)), rng.uniform(0, 9, (B * S, N + 1, 1)), rng.uniform(-7, 7, (B * S, N + 1, 1))], axis=-1)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    for direction in (R.TO, R.FROM):
        for fr, fr_full, fs in ((frames, frames, 5), (frames[2], np.broadcast_to(frames[2], (B, 5)), 0)):
            want = R.frame_states(fr_full, X, direction, S)
            got = solver.frame_states(N, fr, X, direction, S).reshape(B * S, N + 1, 4)
            assert _same_bits(got, want), (direction, fs)
            dX, dF = torch.from_numpy(X.copy()).to(dev), torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
            torch.cuda.synchronize()
            solver.frame_states_device(st, B, S, N, dF.data_ptr(), fs, direction, dX.data_ptr(), dX.data_ptr())
            torch.cuda.synchronize()
            assert _same_bits(dX.cpu().numpy(), want), (direction, fs, "in place")
    back = solver.frame_states(N, frames, solver.frame_states(N, frames, X, R.TO, S), R.FROM, S).reshape(X.shape)
    assert np.abs(back - X).max() <= 1e-12 * 1200  # a round trip returns the states to rounding


@pytest.mark.parametrize("K", (1, 2))
def test_frame_poses_bits(cilqr, solver, K):
    """One pose set for the batch (pose_stride 0) and one per solve (3K); host form = device form."""
    import torch
    rng = np.random.default_rng(3240 + K)
    B = 9
    frames = _frames(rng, B)
    per = np.concatenate([rng.uniform(-300, 300, (B, K, 2)), rng.uniform(-3, 3, (B, K, 1))], axis=-1)
    for poses, full in ((per, per), (per[4], np.broadcast_to(per[4], (B, K, 3)))):
        for fr, fr_full, fs in ((frames, frames, 5), (frames[0], np.broadcast_to(frames[0], (B, 5)), 0)):
            want = R.frame_poses(fr_full, full)
            got = solver.frame_poses(B, fr, poses)
            assert _same_bits(got, want), (poses.shape, fs)
            dev = torch.device("cuda", 0)
            dP, dF = torch.from_numpy(np.ascontiguousarray(poses)).to(dev), torch.from_numpy(np.ascontiguousarray(fr)).to(dev)
            out = torch.zeros(B, K, 3, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            solver.frame_poses_device(torch.cuda.current_stream().cuda_stream, B, K, dF.data_ptr(), fs, dP.data_ptr(), 3 * K if poses.ndim == 3 else 0,
                                      out.data_ptr())
            torch.cuda.synchronize()
            assert _same_bits(out.cpu().numpy(), want)


def test_frame_obstacles_device_form_is_the_host_form(cilqr, solver):
    import torch
    rng = np.random.default_rng(3250)
    B, N, M = 6, 30, 2
    frames = _frames(rng, B)
    pose = np.concatenate([rng.uniform(-50, 50, (M, N, 2)), rng.uniform(0, 8, (M, N, 1)), rng.uniform(-3, 3, (M, N, 1))], axis=-1)
    dim, cov = rng.uniform(1, 5, (M, N, 2)), rng.uniform(0.1, 0.3, (M, N, 3))
    host = solver.frame_obstacles(B, N, frames, pose.reshape(M, 4 * N), dim.reshape(M, 2 * N), cov.reshape(M, 3 * N), global_inflation=True)
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    dF, dP, dD, dC = d(frames), d(pose), d(dim), d(cov)
    oP, oD, oC = (torch.zeros(B, M, N * k, dtype=torch.float64, device=dev) for k in (4, 2, 3))
    torch.cuda.synchronize()
    solver.frame_obstacles_device(torch.cuda.current_stream().cuda_stream, B, N, M, dF.data_ptr(), 5, dP.data_ptr(), dD.data_ptr(), (0, N, 1),
                                  oP.data_ptr(), oD.data_ptr(), dC.data_ptr(), oC.data_ptr(), flags=cilqr.FRAME_GLOBAL_INFLATION)
    torch.cuda.synchronize()
    assert _same_bits(oP.cpu().numpy(), host["pose"]) and _same_bits(oD.cpu().numpy(), host["dim"]) and _same_bits(oC.cpu().numpy(), host["cov"])


# ---------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_name_the_field_and_launch_nothing(cilqr, solver):
    """Every refusal leaves the outputs as they were (host forms: nothing travels; the message names the argument)."""
    B, N, M = 4, 10, 2
    frames = np.zeros((B, 5))
    frames[:, 2] = 1.0
    pose, dim = np.ones((M, 4)), np.ones((M, 2))
    X = np.ones((B, 4 * (N + 1)))

    def refused(match, fn):
        with pytest.raises(cilqr.CilqrError, match=match):
            fn()

    dp = C.POINTER(C.c_double)
    L = cilqr.lib()
    out = np.full((B, M, 4 * N), 7.5)
    dout = np.full((B, M, 2 * N), 7.5)
    obs = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, 0, 1, 0, 0)
    for fs in (1, 4, 6, -5):
        rc = L.cilqr_frame_obstacles(solver._h, B, N, M, frames.ctypes.data_as(dp), C.c_int64(fs), C.byref(obs), None, C.c_uint32(0),
                                     out.ctypes.data_as(dp), dout.ctypes.data_as(dp), None)
        assert rc == ERR_ARG and b"frame_stride" in L.cilqr_last_error()
        rc = L.cilqr_frame_states(solver._h, B, 1, N, frames.ctypes.data_as(dp), C.c_int64(fs), 1, X.ctypes.data_as(dp), out.ctypes.data_as(dp))
        assert rc == ERR_ARG and b"frame_stride" in L.cilqr_last_error()
        rc = L.cilqr_frame_poses(solver._h, B, 1, frames.ctypes.data_as(dp), C.c_int64(fs), X.ctypes.data_as(dp), C.c_int64(0), out.ctypes.data_as(dp))
        assert rc == ERR_ARG and b"frame_stride" in L.cilqr_last_error()
    bad = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, 0, -1, 0, 0)
    rc = L.cilqr_frame_obstacles(solver._h, B, N, M, frames.ctypes.data_as(dp), C.c_int64(5), C.byref(bad), None, C.c_uint32(0),
                                 out.ctypes.data_as(dp), dout.ctypes.data_as(dp), None)
    assert rc == ERR_ARG and b"negative stride" in L.cilqr_last_error()
    rc = L.cilqr_frame_obstacles(solver._h, B, N, M, frames.ctypes.data_as(dp), C.c_int64(5), C.byref(obs), None, C.c_uint32(2),
                                 out.ctypes.data_as(dp), dout.ctypes.data_as(dp), None)
    assert rc == ERR_ARG and b"flag" in L.cilqr_last_error()
    assert (out == 7.5).all() and (dout == 7.5).all()
    refused("B=65 outside", lambda: solver.frame_obstacles(65, N, np.zeros((65, 5)), pose, dim))
    refused("N=66 outside", lambda: solver.frame_obstacles(B, 66, frames, pose, dim))
    refused("M=4 outside", lambda: solver.frame_obstacles(B, N, frames, np.ones((4, 4)), np.ones((4, 2))))
    refused("N=66 outside", lambda: solver.frame_states(66, frames, np.ones((B, 4 * 67))))
    refused("B\\*S", lambda: solver.frame_states(N, np.zeros((33, 5)), np.ones((66, 4 * (N + 1))), S=2))
    refused("direction=2", lambda: solver.frame_states(N, frames, X, direction=2))
    refused("B=65 outside", lambda: solver.frame_poses(65, np.zeros((65, 5)), np.zeros((1, 3))))
    rc = L.cilqr_frame_poses(solver._h, B, 2, frames.ctypes.data_as(dp), C.c_int64(5), X.ctypes.data_as(dp), C.c_int64(3), out.ctypes.data_as(dp))
    assert rc == ERR_ARG and b"pose_stride" in L.cilqr_last_error()
    path, ego = np.zeros((5, 2)), np.zeros((65, 4))
    refused("B=65 outside", lambda: solver.local_plan_frames(path, ego))
    rc = L.cilqr_local_plan_frames(solver._h, 1, 5, path.ctypes.data_as(dp), C.c_int64(-1), ego.ctypes.data_as(dp), frames.ctypes.data_as(dp),
                                   np.zeros(1, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32)), X.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                   dout.ctypes.data_as(dp), None, None, None)
    assert rc == ERR_ARG and b"path_stride" in L.cilqr_last_error()
    assert (out == 7.5).all() and (dout == 7.5).all()


# ---------------------------------------------------------------------------------------------------------------- composition
COMP_N, COMP_M = 30, 2
COMP_OBS = np.array([[15.0, 0.8, 0.0, 0.0], [27.0, -1.0, 0.0, 0.1]])
COMP_DIM = np.array([[4.79, 2.16]] * 2)
COMP_EGO = np.array([0.0, 0.1, 3.0, 0.02])
MAP_GEOM = (24.0, 12.0, 0.2, 0.0, 0.0)
MAP_POSE = np.array([9.0, 0.0, 0.0])  # the map's centre 9 m ahead of the unturned ego, its x axis along the road
BLOB = (6.0, -0.9, 0.7)               # world x, y of the blob's centre in the unturned scene and its width


@functools.lru_cache(maxsize=None)
def comp_scene():
    """Six solves: the east road, the same road heading north and west, the known-answer scene as it is, turned by 0.5 and turned
    by 2.4 at (300, -200).  Solves 1 and 2 are solve 0 moved; solves 4 and 5 are solve 3 moved."""
    i = np.arange(200.0)
    east = np.stack([i, np.zeros(200)], axis=1)
    known = np.stack([i, 0.5 * np.sin(0.05 * i)], axis=1)
    moves = ((east, 0.0, (0.0, 0.0)), (east, math.pi / 2, (3.0, 0.0)), (east, math.pi, (-40.0, 6.5)), (known, 0.0, (0.0, 0.0)),
             (known, 0.5, (0.0, 0.0)), (known, 2.4, (300.0, -200.0)))
    paths, egos, obs, poses = [], [], [], []
    for path, a, t in moves:
        pp, ee, oo = R.move_scene(a, t, path, COMP_EGO, COMP_OBS)
        _, mp, _ = R.move_scene(a, t, path, np.array([MAP_POSE[0], MAP_POSE[1], 0.0, MAP_POSE[2]]))
        paths.append(pp), egos.append(ee), obs.append(oo), poses.append([mp[0], mp[1], mp[3]])
    return np.array(paths), np.array(egos), np.array(obs), np.array(poses)


def _blob_layer(g):
    """(rows, cols) float32 in the map's own frame (grid_map order: cell (0, 0) at the largest x and y), as tests/test_tighten_map.py
    builds it, for the map at MAP_POSE."""
    mx = (g.pos_x + (0.5 * g.len_x - 0.5 * g.res) - np.arange(g.rows) * g.res)[:, None]
    my = (g.pos_y + (0.5 * g.len_y - 0.5 * g.res) - np.arange(g.cols) * g.res)[None, :]
    c, s = math.cos(MAP_POSE[2]), math.sin(MAP_POSE[2])
    wx, wy = MAP_POSE[0] + c * mx - s * my, MAP_POSE[1] + s * mx + c * my
    r2 = (wx - BLOB[0]) ** 2 + (wy - BLOB[1]) ** 2
    return (100.0 * np.tanh(1.3 * np.exp(-0.5 * r2 / BLOB[2] ** 2))).astype(np.float32)


def test_composition_on_device_buffers(cilqr, oracle, solver):
    """Framed pre-step -> frame_obstacles -> cilqr_solve_batch_obstacles_device -> frame_states back, all on device buffers.  U
    within 1e-9 of the oracle's solve on the restated frame inputs, iterations and status equal; the north and west roads' U within
    1e-9 of the east road's.  Then, with the blob layer set through frame_poses, the footprint check on the framed X of the turned
    scenes returns the map counts and cells of the unturned ones, bit for bit."""
    import torch
    B, N, M, P = 6, COMP_N, COMP_M, 200
    paths, egos, obs, map_poses = comp_scene()
    po = oracle.default_params(N)
    U0 = oracle.default_control_seq(N)
    want = [R.framed_solve(oracle, po, N, paths[b], egos[b], U0, obs[b], COMP_DIM) for b in range(B)]
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
    dPath, dEgo, dObs, dDim = d(paths), d(egos), d(obs), d(np.broadcast_to(COMP_DIM, (B, M, 2)))
    fr, info, x0, poly, fl = z(B, 5), z(B, dt=torch.int32), z(B, 4), z(B, 6), z(B, 2)
    oP, oD = z(B, M, 4 * N), z(B, M, 2 * N)
    U, X, J, it, status = d(np.tile(U0, (B, 1))), z(B, 4 * (N + 1)), z(B), z(B, dt=torch.int32), z(B, dt=torch.int32)
    Xmap = z(B, 4 * (N + 1))
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    solver.local_plan_frames_device(st, B, P, dPath.data_ptr(), 2 * P, dEgo.data_ptr(), fr.data_ptr(), info.data_ptr(), x0.data_ptr(),
                                    poly.data_ptr(), fl.data_ptr())
    solver.frame_obstacles_device(st, B, N, M, fr.data_ptr(), 5, dObs.data_ptr(), dDim.data_ptr(), (M, 1, 0), oP.data_ptr(), oD.data_ptr())
    solver.solve_batch_obstacles_device(st, B, N, M, x0.data_ptr(), U.data_ptr(), poly.data_ptr(), fl.data_ptr(), oP.data_ptr(), oD.data_ptr(),
                                        0, (M * N, N, 1, 0), X.data_ptr(), J.data_ptr(), it.data_ptr(), status.data_ptr())
    solver.frame_states_device(st, B, 1, N, fr.data_ptr(), 5, R.FROM, X.data_ptr(), Xmap.data_ptr())
    torch.cuda.synchronize()
    gU, gX, gXm, gfr = U.cpu().numpy(), X.cpu().numpy(), Xmap.cpu().numpy().reshape(B, N + 1, 4), fr.cpu().numpy()
    assert not info.cpu().numpy().any()
    for b in range(B):
        dU = np.abs(gU[b] - want[b]["U"]).max()
        dXm = np.abs(gXm[b][:, :2] - want[b]["X_map"][:, :2]).max()
        print("path_frame composition solve %d: max|dU|=%.3g vs oracle, iters %d/%d, max|dX_map|=%.3g" % (b, dU, int(it[b]), want[b]["iters"], dXm))
        assert dU <= 1e-9 and int(it[b]) == want[b]["iters"] and int(status[b]) == want[b]["status"]
        assert dXm <= 1e-9 * max(1.0, np.abs(want[b]["X_map"][:, :2]).max())
        assert _same_bits(gXm[b], R.frame_states(gfr[b][None], gX[b].reshape(1, N + 1, 4), R.FROM)[0])
    for b, base in ((1, 0), (2, 0), (4, 3), (5, 3)):
        dU = np.abs(gU[b] - gU[base]).max()
        print("path_frame composition: solve %d against solve %d: max|dU|=%.3g" % (b, base, dU))
        assert dU <= 1e-9 and int(it[b]) == int(it[base])
    # the map: one layer in its own frame, its pose moved with each scene, taken into each solve's frame
    g = cilqr.map_geom(*MAP_GEOM)
    layer = _blob_layer(g)
    dLayer = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(layer).flatten(order="F"))).to(dev)
    dMapPose, fPose = d(map_poses.reshape(B, 1, 3)), z(B, 1, 3)
    fp = z(B, cilqr.FOOTPRINT_FIELDS)
    solver.frame_poses_device(st, B, 1, fr.data_ptr(), 5, dMapPose.data_ptr(), 3, fPose.data_ptr())
    torch.cuda.synchronize()
    assert _same_bits(fPose.cpu().numpy(), R.frame_poses(gfr, map_poses.reshape(B, 1, 3)))
    solver.set_uncertainty_map_device(dLayer.data_ptr(), g, probes=(3, 3), layer_stride=0, poses_ptr=fPose.data_ptr())
    try:
        solver.footprint_check_device(st, B, N, M, 1, X.data_ptr(), oP.data_ptr(), oD.data_ptr(), (M * N, N, 1, 0), fp.data_ptr(), occ_threshold=50.0)
        torch.cuda.synchronize()
    finally:
        solver.clear_uncertainty_map()
    gfp = fp.cpu().numpy()
    cols = [cilqr.FP_HIT_STEPS, cilqr.FP_FIRST_HIT, cilqr.FP_MAP_OCC, cilqr.FP_MAP_OCC_STEP, cilqr.FP_MAP_OCC_CELL, cilqr.FP_MAP_HIT_STEPS,
            cilqr.FP_MAP_FIRST_HIT, cilqr.FP_MAP_HIT_CELLS, cilqr.FP_MAP_UNKNOWN_STEPS, cilqr.FP_MAP_CELLS]
    print("path_frame composition footprint rows:\n%s" % gfp[:, cols])
    assert gfp[0, cilqr.FP_MAP_CELLS] > 100 and gfp[0, cilqr.FP_MAP_OCC] > 1.0  # the plans do run over the map and near the blob
    for b, base in ((1, 0), (2, 0), (4, 3), (5, 3)):
        assert _same_bits(gfp[b, cols], gfp[base, cols]), (b, base)


# ---------------------------------------------------------------------------------------------------------------- the facade
def test_facade_set_path_frame(cilqr, tmp_path):
    """tests/cpp/candidates_path_frame.cpp: setter off bit for bit what it was, the north road under the setter returns the east
    road's plan turned (1e-9), through run_candidates, MinTotalCost and run_step; an in-block mode with the setter throws."""
    import os
    import subprocess
    from conftest import PKG, ROOT
    exe = str(tmp_path / "candidates_path_frame")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_path_frame.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "path frame ok" in r.stdout, r.stdout
