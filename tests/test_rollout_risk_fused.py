"""Fused rollout risk (cilqr_rollout_risk*, include/cilqr.h): the collision share per solve, the worst constraint with its row and entry,
and the hits per step of S closed-loop rollouts, with no rollout stored.

Expected values come from the CPU oracle's exported pieces alone, through the helpers of the suite: o_gains, o_rollout and the scenes of
tests/test_rollout_risk.py, `_expected` of tests/test_candidate_score.py.  From its c (rows, M, N, 2) numpy forms the hits (a row hits at
step t when max(c_front, c_rear) > 0 for some m), the per-step counts, the first step, the worst row and its worst entry m*N + t.
Counts, steps, rows and entries are compared exactly, WORST_C within the suite's own 1e-9 absolute.  What makes the exact comparisons
meaningful is asserted on the oracle's numbers in CPU tests: every finite c more than 1e-6 from 0, the worst-row gap and the worst-entry
gap within the worst row above 1e-6.

  case A  scene R (B 8, N 12, M 3), S = 70,  pose_offsets(70, 0.16, 0.16, 0.017, 5),  k_scale 0: one wavefront and a 6-row tail
  case B  scene R,                  S = 300, pose_offsets(300, 0.16, 0.16, 0.017, 5), k_scale 0: two workgroups per solve (256 + 44 rows)
  case C  scene L (B 6, N 50, M 4), S = 64,  the scene's own offsets,                 k_scale 1: the workload's horizon
(Scene L at k_scale 0 has margins of 1.3e-6 and 3.2e-6, too close to the condition.)
"""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import MAX_C, MAX_C_ENTRY, _bits, _expected, _totals
from test_rollout_risk import _pick, _scene_l, _scene_r, o_gains, o_rollout

gpu = pytest.mark.gpu

ABS_TOL, MARGIN = 1e-9, 1e-6
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_rollout_risk", "cilqr_rollout_risk_device")
RR_COLLISION, RR_WORST_C, RR_WORST_ROW, RR_WORST_ENTRY, RR_FIRST_STEP, RR_STEP_SHARE = range(6)
R_COLLISION, R_WORST_C, R_WORST_ROW = range(3)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- expected values from the oracle ------------------------------------------------------------------------------------------
def _reduce(c, extra_hit=None):
    """c (B, S, M, N, 2) of `_expected` -> dict of what the call returns, by numpy.  extra_hit (B, S, N) bool: rows that hit at a step
    for a reason other than c (a state that is not finite); such rows must carry c = -inf."""
    B, S, M, N = c.shape[:4]
    per_entry = c.max(axis=4)                                   # (B, S, M, N): max(c_front, c_rear)
    hit = (per_entry > 0).any(axis=2)                           # (B, S, N)
    if extra_hit is not None:
        hit = hit | extra_hit
    step_hits = hit.sum(axis=1).astype(np.int32)                # (B, N)
    risk = np.zeros((B, 6))
    risk[:, RR_COLLISION] = hit.any(axis=2).sum(axis=1) / S
    any_step = step_hits > 0
    risk[:, RR_FIRST_STEP] = np.where(any_step.any(axis=1), any_step.argmax(axis=1), -1)
    risk[:, RR_STEP_SHARE] = step_hits.max(axis=1) / S
    flat = per_entry.reshape(B, S, M * N)                       # entry index m*N + t
    if M:
        row_max = flat.max(axis=2)
        rows = row_max.argmax(axis=1)
        risk[:, RR_WORST_C] = row_max.max(axis=1)
        risk[:, RR_WORST_ROW] = rows
        risk[:, RR_WORST_ENTRY] = [int(flat[b, rows[b]].argmax()) for b in range(B)]
    else:
        risk[:, RR_WORST_C], risk[:, RR_WORST_ROW], risk[:, RR_WORST_ENTRY] = -np.inf, -1, -1
    return dict(risk=risk, step_hits=step_hits, hit_rows=hit.any(axis=2).sum(axis=1))


def _case(O, s, S, delta, k_scale, N=None):
    """One case on scene `s` (gains already there): the oracle's rollouts from `delta` (S, 4) and their c."""
    B, M = s["B"], s["M"]
    p = s["p"]
    X, U, k, K, pose, dim = s["X"], s["U"], s["k"], s["K"], s["pose"], s["dim"]
    if N is None:
        N = s["N"]
    else:  # the first N steps of the same trajectories, gains and obstacles
        p = copy.copy(p)
        p.horizon = N
        X, U = np.ascontiguousarray(X[:, :4 * (N + 1)]), np.ascontiguousarray(U[:, :2 * N])
        k, K = np.ascontiguousarray(k[:, :2 * N]), np.ascontiguousarray(K[:, :8 * N])
        pose = np.ascontiguousarray(pose.reshape(B, M, s["N"], 4)[:, :, :N].reshape(B, M, 4 * N))
        dim = np.ascontiguousarray(dim.reshape(B, M, s["N"], 2)[:, :, :N].reshape(B, M, 2 * N))
    d = np.ascontiguousarray(np.broadcast_to(delta, (B, S, 4)))
    Xr, Ur = o_rollout(O, p, N, X, U, k, K, d, k_scale)
    rep = lambda a: np.ascontiguousarray(np.repeat(a, S, axis=0))  # noqa: E731  (row r belongs to solve r // S)
    _, c = _expected(O, p, N, Xr.reshape(B * S, -1), Ur.reshape(B * S, -1), rep(s["poly"]), rep(s["fl"]), rep(pose), rep(dim))
    c = c.reshape(B, S, M, N, 2)
    out = dict(B=B, N=N, M=M, S=S, X=X, U=U, k=k, K=K, pose=pose, dim=dim, poly=s["poly"], fl=s["fl"], delta=np.ascontiguousarray(delta),
               k_scale=k_scale, c=c, p=p)
    out.update(_reduce(c))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """Cases A, B, C, the N = 2 edge of scene R and scene R's nominal totals, from the oracle.  Computed once; never modified."""
    from cilqr_amd import scenes
    O = oracle
    r, l = _scene_r(O), _scene_l(O)
    for s in (r, l):
        s["k"], s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
        assert np.all(ok == 1)
    out = {"A": _case(O, r, 70, r["delta"], 0.0), "B": _case(O, r, 300, scenes.pose_offsets(300, 0.16, 0.16, 0.017, seed=5), 0.0),
           "C": _case(O, l, 64, l["delta"], 1.0), "N2": _case(O, r, 70, r["delta"], 0.0, N=2)}
    nominal, _ = _expected(O, r["p"], r["N"], r["X"], r["U"], r["poly"], r["fl"], r["pose"], r["dim"])
    out["A"]["base"] = _totals(nominal)
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    import re
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cilqr.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_ROLLOUT_RISK_FIELDS\s+6\b", h)
    for i, name in enumerate(("COLLISION", "WORST_C", "WORST_ROW", "WORST_ENTRY", "FIRST_STEP", "STEP_SHARE")):
        assert re.search(r"\bCILQR_RR_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "RR_" + name) == i
    assert cilqr.ROLLOUT_RISK_FIELDS == 6
    assert callable(cilqr.Solver.rollout_risk) and callable(cilqr.Solver.rollout_risk_device)
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_pose_noise_check_fused\s*\(\s*const\s+std::vector<double>&\s+offsets\s*,\s*double\s+max_risk\s*,\s*double\s+lamb\s*=\s*1\.0\s*\)", f)
    assert re.search(r"std::vector<int32_t>\s+last_step_hits\s*;", f)


def test_argument_errors_need_no_device(cilqr):
    """NULL required pointers, total without base, S < 1, a negative stride, a NaN k_scale or max_risk: CILQR_ERR_ARG, decided before the
    handle is looked at (there is none here)."""
    L = cilqr.lib()
    B, N, M, S = 2, 4, 1, 3
    X, U, k, K = np.zeros((B, 4 * (N + 1))), np.zeros((B, 2 * N)), np.zeros((B, 2 * N)), np.zeros((B, 8 * N))
    pose, dim, delta = np.zeros((B, M, 4 * N)), np.ones((B, M, 2 * N)), np.zeros((S, 4))
    risk, hits, total, base = np.zeros((B, 6)), np.zeros((B, N), dtype=np.int32), np.zeros(B), np.zeros(B)
    good = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, M * N, N, 1, 0)
    bad = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, M * N, -1, 1, 0)
    no_handle = C.c_void_p()
    d = C.c_double

    def call(dev, S_=S, stride=0, obs=good, ks=0.0, mr=1.0, **nulls):
        a = dict(X=X, U=U, k=k, K=K, delta=delta, risk=risk, base=base, total=total)
        a.update(nulls)
        f = L.cilqr_rollout_risk_device if dev else L.cilqr_rollout_risk
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, M, S_, _p(a["X"]), _p(a["U"]), _p(a["k"]), _p(a["K"]), _p(a["delta"]), C.c_int64(stride), d(ks), C.byref(obs),
                 d(mr), _p(a["base"]), _p(a["risk"]), _p(hits, _ip), _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "U", "k", "K", "delta", "risk"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert call(dev, S_=0) == ERR_ARG and b"S >= 1" in L.cilqr_last_error()
        assert call(dev, stride=-1) == ERR_ARG and b"negative stride" in L.cilqr_last_error()
        assert call(dev, obs=bad) == ERR_ARG and b"negative stride" in L.cilqr_last_error()
        assert call(dev, ks=float("nan")) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert call(dev, mr=float("nan")) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # neither: valid too


@pytest.mark.parametrize("name", ["A", "B", "C", "N2"])
def test_conditions(cases, name):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the oracle's numbers alone."""
    s = cases[name]
    c, B, S, M, N = s["c"], s["B"], s["S"], s["M"], s["N"]
    assert not np.isnan(c).any()
    finite = c[np.isfinite(c)]
    print("case %s: min|c| %.3g, hits per solve %s, first steps %s" % (name, np.min(np.abs(finite)), s["hit_rows"].tolist(),
                                                                     s["risk"][:, RR_FIRST_STEP].astype(int).tolist()))
    assert np.min(np.abs(finite)) > MARGIN                      # every c that decides a hit
    flat = c.max(axis=4).reshape(B, S, M * N)
    row_max = np.sort(flat.max(axis=2), axis=1)
    print("  worst rows %s, smallest row gap %.3g" % (s["risk"][:, RR_WORST_ROW].astype(int).tolist(), np.min(row_max[:, -1] - row_max[:, -2])))
    assert np.min(row_max[:, -1] - row_max[:, -2]) > MARGIN      # the worst row of every solve is decided
    ent = np.sort(np.stack([flat[b, int(s["risk"][b, RR_WORST_ROW])] for b in range(B)]), axis=1)
    print("  worst entries %s, smallest entry gap %.3g" % (s["risk"][:, RR_WORST_ENTRY].astype(int).tolist(), np.min(ent[:, -1] - ent[:, -2])))
    assert np.min(ent[:, -1] - ent[:, -2]) > MARGIN              # and the worst entry within it
    if name == "A":
        assert s["hit_rows"].tolist() == [5, 30, 5, 4, 0, 0, 0, 0]
        assert s["risk"][:, RR_FIRST_STEP].tolist() == [9, 5, 5, 7, -1, -1, -1, -1]
        assert not np.any(np.abs(s["risk"][:, RR_COLLISION] - 0.06) < 1e-3)
    if name == "B":
        assert s["hit_rows"].tolist() == [27, 152, 25, 14, 1, 0, 0, 0]
    if name == "C":
        assert s["hit_rows"].tolist() == [64, 64, 64, 0, 64, 64]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


def _host(solver, s, sel=slice(None), delta=None, pose="scene", dim=None, k_scale=None, max_risk=1.0, base=None):
    if isinstance(pose, str):
        pose, dim = s["pose"][sel], s["dim"][sel]
    return solver.rollout_risk(s["N"], s["X"][sel], s["U"][sel], s["k"][sel], s["K"][sel], s["delta"] if delta is None else delta, pose, dim,
                               None, k_scale=s["k_scale"] if k_scale is None else k_scale, max_risk=max_risk, base=base)


def _device(cilqr, solver, s, base=None, max_risk=1.0, three_call=False):
    """The device form on torch buffers: (risk, step_hits, total); three_call: also cilqr_rollout_batch_device -> cilqr_score_rollouts_device
    on the same buffers -> (rows (B, S, 8), risk (B, 4))."""
    import torch
    B, N, M, S = s["B"], s["N"], s["M"], s["S"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = {n: torch.from_numpy(np.ascontiguousarray(s[n])).to(dev) for n in ("X", "U", "k", "K", "delta", "pose", "dim", "poly", "fl")}
    strides = cilqr.obstacle_strides(s["pose"].shape, s["dim"].shape, None, B, N)[1:]
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    risk, hits, total = z(B, 6), z(B, N, dt=torch.int32), z(B)
    tb = None if base is None else torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    solver.rollout_risk_device(stream, B, N, M, S, t["X"].data_ptr(), t["U"].data_ptr(), t["k"].data_ptr(), t["K"].data_ptr(),
                               t["delta"].data_ptr(), 0, t["pose"].data_ptr(), t["dim"].data_ptr(), strides, risk.data_ptr(), hits.data_ptr(),
                               total.data_ptr() if tb is not None else 0, tb.data_ptr() if tb is not None else 0, k_scale=s["k_scale"],
                               max_risk=max_risk)
    out = [risk, hits, total]
    if three_call:
        Xr, Ur, rows, risk3 = z(B, S, 4 * (N + 1)), z(B, S, 2 * N), z(B, S, 8), z(B, 4)
        solver.rollout_batch_device(stream, B, N, S, t["X"].data_ptr(), t["U"].data_ptr(), t["k"].data_ptr(), t["K"].data_ptr(),
                                    t["delta"].data_ptr(), 0, Xr.data_ptr(), Ur.data_ptr(), k_scale=s["k_scale"])
        solver.score_rollouts_device(stream, B, N, M, S, Xr.data_ptr(), Ur.data_ptr(), t["poly"].data_ptr(), t["fl"].data_ptr(),
                                     t["pose"].data_ptr(), t["dim"].data_ptr(), 0, strides, rows.data_ptr(), risk3.data_ptr(), max_risk=1.0)
        out += [rows, risk3]
    torch.cuda.synchronize(dev)
    out = [a.cpu().numpy() for a in out]
    if tb is None:
        out[2] = None
    return out


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def _check_against(got_risk, got_hits, want, what):
    risk, hits = want["risk"], want["step_hits"]
    print("%s: hits per solve %s, |WORST_C - oracle| max %.3g" % (what, np.rint(got_risk[:, RR_COLLISION] * want["S"]).astype(int).tolist(),
                                                                  np.max(np.abs(got_risk[:, RR_WORST_C] - risk[:, RR_WORST_C]))))
    assert np.array_equal(got_hits, hits), what
    for f in (RR_COLLISION, RR_FIRST_STEP, RR_STEP_SHARE, RR_WORST_ROW, RR_WORST_ENTRY):
        assert np.array_equal(got_risk[:, f], risk[:, f]), (what, f, got_risk[:, f], risk[:, f])
    assert np.max(np.abs(got_risk[:, RR_WORST_C] - risk[:, RR_WORST_C])) <= ABS_TOL, what


@gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_fields_against_the_oracle(cilqr, solver, cases, name):
    """Fed the oracle's gains: shares, step counts, first steps, step shares, worst rows and entries exact, WORST_C within 1e-9; the
    host form and the device form give the same bits."""
    s = cases[name]
    risk, hits, total = _host(solver, s)
    assert total is None and hits.dtype == np.int32
    _check_against(risk, hits, s, "case %s, host form" % name)
    drisk, dhits, _ = _device(cilqr, solver, s)
    _check_against(drisk, dhits, s, "case %s, device form" % name)
    assert _same((risk, hits), (drisk, dhits))


@gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_against_the_stored_rows_path(cilqr, solver, cases, name):
    """cilqr_rollout_batch_device -> cilqr_score_rollouts_device on the same device buffers: the share, the worst row, that row's worst
    entry, and WORST_C bit for bit."""
    s = cases[name]
    risk, hits, _, rows, risk3 = _device(cilqr, solver, s, three_call=True)
    B = s["B"]
    assert np.array_equal(risk[:, RR_COLLISION], risk3[:, R_COLLISION])
    assert np.array_equal(risk[:, RR_WORST_ROW], risk3[:, R_WORST_ROW])
    worst = risk3[:, R_WORST_ROW].astype(int)
    assert np.array_equal(risk[:, RR_WORST_ENTRY], rows[np.arange(B), worst, MAX_C_ENTRY])
    print("case %s: WORST_C fused %s\n          stored rows %s" % (name, risk[:, RR_WORST_C].tolist(), risk3[:, R_WORST_C].tolist()))
    assert np.array_equal(_bits(risk[:, RR_WORST_C]), _bits(risk3[:, R_WORST_C]))
    # every row's own maximum, through the hits: a row hits exactly when its stored-row MAX_C is positive
    assert np.array_equal(hits.sum(axis=1) > 0, (rows[:, :, MAX_C] > 0).any(axis=1))


@gpu
def test_a_result_depends_on_its_own_solve_alone(solver, cases):
    """A solve alone, in another batch position, with a per-solve copy of the shared offsets, and through strides that address the same
    obstacle values: the same bits.  S = 300: two workgroups per solve and the finish kernel."""
    s = cases["B"]
    B, N, M, S = s["B"], s["N"], s["M"], s["S"]
    risk, hits, _ = _host(solver, s)
    for b in (1, B - 1):  # alone
        r1, h1, _ = _host(solver, s, sel=slice(b, b + 1))
        assert _same((r1[0], h1[0]), (risk[b], hits[b])), b
    order = np.array([5, 1, 7, 0, 2])  # another batch, other positions
    t = dict(s)
    for n in ("X", "U", "k", "K", "pose", "dim"):
        t[n] = np.ascontiguousarray(s[n][order])
    r2, h2, _ = _host(solver, t)
    assert _same((r2, h2), (risk[order], hits[order]))
    r3, h3, _ = _host(solver, s, delta=np.ascontiguousarray(np.broadcast_to(s["delta"], (B, S, 4))))  # delta_batch_stride 1
    assert _same((r3, h3), (risk, hits))
    # one obstacle set shared by the batch, constant over the horizon: (M, 4) / (M, 2) against its dense expansion
    sp = np.ascontiguousarray(s["pose"].reshape(B, M, N, 4)[1, :, 0])
    sd = np.ascontiguousarray(s["dim"].reshape(B, M, N, 2)[1, :, 0])
    dp = np.ascontiguousarray(np.broadcast_to(np.repeat(sp[:, None, :], N, axis=1).reshape(1, M, 4 * N), (B, M, 4 * N)))
    dd = np.ascontiguousarray(np.broadcast_to(np.repeat(sd[:, None, :], N, axis=1).reshape(1, M, 2 * N), (B, M, 2 * N)))
    shared, dense = _host(solver, s, pose=sp, dim=sd), _host(solver, s, pose=dp, dim=dd)
    assert _same(shared[:2], dense[:2])
    assert shared[1].any()  # (the shared set still produces hits: the comparison is not one of zeros)


@gpu
def test_no_obstacles_and_two_steps(solver, cases):
    a = cases["A"]
    risk, hits, _ = _host(solver, a, pose=None)
    B = a["B"]
    assert np.all(np.isneginf(risk[:, RR_WORST_C]))
    for f, v in ((RR_COLLISION, 0.0), (RR_WORST_ROW, -1.0), (RR_WORST_ENTRY, -1.0), (RR_FIRST_STEP, -1.0), (RR_STEP_SHARE, 0.0)):
        assert np.array_equal(risk[:, f], np.full(B, v)), f
    assert not hits.any()
    s = cases["N2"]
    risk, hits, _ = _host(solver, s)
    _check_against(risk, hits, s, "N = 2")


@gpu
def test_one_row_on_the_nominal_trajectory_is_the_score_call(solver, cases):
    """S = 1, a zero offset, k_scale 0 on a trajectory the device's own dynamics produced (the zero-offset rollout of scene R): every
    state of the row is the nominal state bit for bit, so WORST_C and WORST_ENTRY equal cilqr_score_batch's MAX_C and MAX_C_ENTRY of that
    trajectory bit for bit."""
    s = cases["A"]
    N = s["N"]
    roll = solver.rollout_batch(N, s["X"], s["U"], s["k"], s["K"], np.zeros((1, 4)), k_scale=0.0)
    X, U = np.ascontiguousarray(roll["X"][:, 0]), np.ascontiguousarray(roll["U"][:, 0])
    again = solver.rollout_batch(N, X, U, s["k"], s["K"], np.zeros((1, 4)), k_scale=0.0)
    assert np.array_equal(_bits(again["X"][:, 0]), _bits(X))  # the trajectory reproduces itself
    score = solver.score_batch(N, X, U, s["poly"], s["fl"], s["pose"], s["dim"])["score"]
    risk, hits, _ = solver.rollout_risk(N, X, U, s["k"], s["K"], np.zeros((1, 4)), s["pose"], s["dim"], k_scale=0.0)
    assert np.array_equal(_bits(risk[:, RR_WORST_C]), _bits(score[:, MAX_C]))
    assert np.array_equal(risk[:, RR_WORST_ENTRY], score[:, MAX_C_ENTRY])
    assert np.array_equal(risk[:, RR_WORST_ROW], np.zeros(s["B"]))
    assert np.array_equal(risk[:, RR_COLLISION], (score[:, MAX_C] > 0).astype(float))


@gpu
def test_a_nan_offset_row_hits_from_step_0_and_never_wins(solver, cases):
    s = cases["A"]
    B, S, N = s["B"], s["S"], s["N"]
    row = 7
    assert not np.any(s["risk"][:, RR_WORST_ROW] == row)
    delta = s["delta"].copy()
    delta[row] = np.nan
    c = s["c"].copy()
    c[:, row] = -np.inf
    extra = np.zeros((B, S, N), dtype=bool)
    extra[:, row] = True
    want = dict(_reduce(c, extra), S=S)
    assert np.all(want["risk"][:, RR_FIRST_STEP] == 0) and np.all(want["step_hits"] >= 1)
    risk, hits, _ = _host(solver, s, delta=delta)
    _check_against(risk, hits, want, "one NaN offset row")
    clean = _host(solver, s)
    assert np.array_equal(_bits(risk[:, RR_WORST_C]), _bits(clean[0][:, RR_WORST_C]))


def _device_pick(solver, values):
    import torch
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    solver.argmin_device(torch.cuda.current_stream(dev).cuda_stream, len(values), v.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)
    return int(out.cpu().numpy()[1])


@gpu
def test_total_and_the_pick(cilqr, solver, cases):
    """total is base where the share is at most max_risk and base is finite, NaN elsewhere; the pick through cilqr_argmin_device is numpy's,
    -1 included."""
    s = cases["A"]
    share = s["risk"][:, RR_COLLISION]
    base = s["base"].copy()
    picks = []
    for max_risk in (0.06, 0.0, -1.0, 1.0):
        want = np.where(share > max_risk, np.nan, base)
        for form in ("host", "device"):
            total = _host(solver, s, max_risk=max_risk, base=base)[2] if form == "host" else _device(cilqr, solver, s, base=base, max_risk=max_risk)[2]
            assert np.array_equal(np.isnan(total), np.isnan(want)), (max_risk, form)
            assert np.array_equal(_bits(total[~np.isnan(want)]), _bits(base[~np.isnan(want)])), (max_risk, form)
            assert _device_pick(solver, total) == _pick(want), (max_risk, form)
        picks.append(_pick(want))
    assert picks[2] == -1 and picks[0] >= 3 and picks[3] == _pick(base)  # all rejected; solves 0-2 rejected at 0.06; none at 1
    base[6] = np.inf  # a base that is not finite is rejected whatever its share
    total = _host(solver, s, max_risk=1.0, base=base)[2]
    assert np.isnan(total[6]) and not np.isnan(np.delete(total, 6)).any()


@gpu
def test_limits(cilqr, cases):
    """B * ceil(S/256) above max_batch: CILQR_ERR_ARG, and the handle stays usable.  A shape beyond the LDS bound (N 80, M 16: 70 864
    bytes): CILQR_ERR_UNSUPPORTED."""
    s = cases["B"]
    sv = cilqr.Solver(cilqr.default_params(), max_batch=15, max_horizon=s["N"], max_obstacles=3, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="above max_batch"):
            _host(sv, s)  # 8 solves x 2 partial records
        k = slice(0, 7)
        risk, hits, _ = _host(sv, s, sel=k)  # 14 records
        _check_against(risk, hits, dict(risk=s["risk"][k], step_hits=s["step_hits"][k], S=s["S"]), "7 solves on a handle of 15")
    finally:
        sv.close()
    B, N, M, S = 2, 80, 16, 64
    sv = cilqr.Solver(cilqr.default_params(N), max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*LDS" % ERR_UNSUPPORTED):
            sv.rollout_risk(N, np.zeros((B, 4 * (N + 1))), np.zeros((B, 2 * N)), np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros((S, 4)),
                            np.zeros((B, M, 4 * N)), np.ones((B, M, 2 * N)))
    finally:
        sv.close()


def _oracle_pick_of_the_dump(O, cilqr, path):
    """What tests/cpp/candidates_risk_fused.cpp wrote -> the oracle-derived shares, step counts and pick for the candidates it solved:
    oracle gains at the solved trajectories, oracle rollouts from its offsets, `_expected`'s c, numpy."""
    v = open(path).read().split()
    B, N, M, S = (int(x) for x in v[:4])
    max_risk, best = float(v[4]), int(v[5])
    a = np.array([float(x) for x in v[6:]])
    take = lambda n, at=[0]: (a[at[0]:at[0] + n], at.__setitem__(0, at[0] + n))[0]  # noqa: E731
    poly, fl = take(B * 6).reshape(B, 6), take(B * 2).reshape(B, 2)
    X, U, base = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1), take(B)
    delta, risk, hits = take(S * 4).reshape(S, 4), take(B * 6).reshape(B, 6), take(B * N).reshape(B, N).astype(np.int32)
    p = O.default_params(N)
    pose = np.ascontiguousarray(np.broadcast_to(np.tile([12.0, -1.0, 0.0, 0.0], N), (B, M, 4 * N)))
    dim = np.ascontiguousarray(np.broadcast_to(np.tile([4.79, 2.16], N), (B, M, 2 * N)))
    s = dict(p=p, B=B, N=N, M=M, X=X, U=U, poly=poly, fl=fl, pose=pose, dim=dim)
    s["k"], s["K"], ok = o_gains(O, p, N, X, U, poly, fl, pose, dim, None, 1.0)
    want = _case(O, s, S, delta, 0.0)
    nominal, _ = _expected(O, p, N, X, U, poly, fl, pose, dim)
    return dict(best=best, max_risk=max_risk, base=base, risk=risk, hits=hits, want=want, o_base=_totals(nominal))


@gpu
def test_cpp_facade_fused_risk_checked_candidates(oracle, cilqr, tmp_path):
    """tests/cpp/candidates_risk_fused.cpp: iLQR::run_candidates with set_pose_noise_check_fused against the C-ABI sequence called by hand
    (inside the program) and against the oracle-derived pick for the candidates it solved (here).  The façade takes one obstacle set for
    all candidates, so its scene is the program's own (that of candidates_risk.cpp), not scene R; the conditions on c are asserted for it."""
    exe, dump = str(tmp_path / "candidates_risk_fused"), str(tmp_path / "dump.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_risk_fused.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fused risk pick ok" in r.stdout, r.stdout
    d = _oracle_pick_of_the_dump(oracle, cilqr, dump)
    want = d["want"]
    finite = want["c"][np.isfinite(want["c"])]
    print("min|c| %.3g, oracle hits per candidate %s" % (np.min(np.abs(finite)), want["hit_rows"].tolist()))
    assert np.min(np.abs(finite)) > MARGIN
    assert np.min(np.abs(want["risk"][:, RR_COLLISION] - d["max_risk"])) > 1e-3
    assert np.array_equal(d["risk"][:, RR_COLLISION], want["risk"][:, RR_COLLISION])
    assert np.array_equal(d["hits"], want["step_hits"])
    assert np.array_equal(d["risk"][:, RR_FIRST_STEP], want["risk"][:, RR_FIRST_STEP])
    assert np.array_equal(d["risk"][:, RR_STEP_SHARE], want["risk"][:, RR_STEP_SHARE])
    assert np.max(np.abs(d["risk"][:, RR_WORST_C] - want["risk"][:, RR_WORST_C])) <= ABS_TOL
    assert np.allclose(d["base"], d["o_base"], rtol=1e-9, atol=0.0)
    ranked = np.sort(d["o_base"])
    assert np.min(np.diff(ranked)) > MARGIN * abs(ranked[0])  # the cheapest is decided
    assert d["best"] == _pick(np.where(want["risk"][:, RR_COLLISION] > d["max_risk"], np.nan, d["o_base"]))
