"""Stop plans (cilqr_stop_plans*, include/cilqr.h): the geometry of a solved plan under a braking speed profile, the fallback for a
tick whose candidates were all rejected.

Expected values never come from the HIP path: `stop_restate` is the numpy restatement of the header's definitions, checked here on
the CPU against the oracle's model (its nominal trajectory over U_stop reproduces X_stop), against physics (a stopped row has
travelled v0^2/(2d)) and against a brute-force distance to the densely sampled path.  The device is compared with it at ABS_TOL =
1e-9, the bar of tests/test_candidate_score.py, on X_stop, U_stop, SP_DISTANCE, SP_END_SPEED, SP_DEVIATION and cost; counts, indices
and the placement of NaN are exact.  That is sound because `test_conditions` asserts on the restatement alone that every scene is
DECIDED: no comparison the definitions make (the stopping comparison, the least advance that still steers, the yaw clamp, the end of
the path, max_deviation, the branch cut of the turn) is within 1e-7 of flipping.

Scenes (plans are the oracle's model run over chosen controls, the oracle's solves, or hand-made polylines):
  A1    N 1,  B 1, D 1, hold 0
  A8    N 8,  B 5, D 3, hold 2: a plan that itself stops and then steps backwards (segments of length 0), a lost plan between two good
        ones, a tight corner at low speed (the yaw clamp acts), a heading that crosses pi, a plan at rest (v0 = 0); the middle level
        stops at step N-1 and the gentlest at step N or later
  D65   N 8,  B 3, D 65, hold 0: more levels than a wavefront has lanes
  C40   N 40, B 6, D 5, hold 1: the oracle's solves of a curved scene, the last plan replaced by one that brakes at -4 m/s^2 (followed
        more gently it is overrun); a level that never stops; max_deviation rejects rows
  H8    the plans of A8 with hold >= N: the rows are the plans
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import ABS_TOL, _bits

gpu = pytest.mark.gpu

ERR_ARG = -1
ENTRY_POINTS = ("cilqr_stop_plans", "cilqr_stop_plans_device")
FIELDS = ("STOP_STEP", "DISTANCE", "END_SPEED", "DEVIATION", "DEVIATION_STEP", "CLAMPED_STEPS", "OVERRUN_STEPS", "LOST")
STOP_STEP, DISTANCE, END_SPEED, DEVIATION, DEVIATION_STEP, CLAMPED_STEPS, OVERRUN_STEPS, LOST = range(8)
VALUES, EXACT = (DISTANCE, END_SPEED, DEVIATION), (STOP_STEP, DEVIATION_STEP, CLAMPED_STEPS, OVERRUN_STEPS, LOST)
MIN_ADVANCE = 1.0e-3
DECIDED = 1e-7
_dp = C.POINTER(C.c_double)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def path_of(X, N):
    """The plan's monotone polyline: V (N+1, 2), s (N+1,), dirs (N+1, 2)."""
    st = X.reshape(N + 1, 4)
    dirs = np.stack([np.cos(st[:, 3]), np.sin(st[:, 3])], axis=1)
    adv = np.maximum(np.sum((st[1:, :2] - st[:-1, :2]) * dirs[:-1], axis=1), 0.0)
    s = np.concatenate([[0.0], np.cumsum(adv)])
    V = st[0, :2] + np.concatenate([np.zeros((1, 2)), np.cumsum(adv[:, None] * dirs[:-1], axis=0)])
    return V, s, dirs


def path_point(V, s, dirs, N, sigma):
    """Q(sigma): on the polyline, or on the ray behind its end."""
    if sigma >= s[N]:
        return V[N] + (sigma - s[N]) * dirs[N]
    t = int(np.searchsorted(s[:N], sigma, side="right")) - 1  # max{t <= N-1 : s_t <= sigma}
    return V[t] + (sigma - s[t]) * dirs[t]


def _brake(v, d, dt):
    if v == 0.0:
        return 0.0, False, math.inf
    q = v / dt
    return (-q, True, abs(q - d)) if d >= q else (-d, False, abs(q - d))


def _row_restate(p, N, X, U, d, hold):
    """One row.  Returns X_stop (N+1, 4), U_stop (N, 2), the sp row and `margin`: the least distance of any comparison from flipping."""
    dt = p.timestep
    yaw_hi, yaw_lo = math.tan(p.steer_angle_max) / p.wheelbase, math.tan(p.steer_angle_min) / p.wheelbase
    V, s, dirs = path_of(X, N)
    plan_u = U.reshape(N, 2)
    x, y, v, th = X.reshape(N + 1, 4)[0]
    Xs, Us = np.zeros((N + 1, 4)), np.zeros((N, 2))
    sigma, dev, dev_step, stop_step, clamped, overrun = 0.0, -1.0, -1, -1, 0, 0
    margin, errs = math.inf, []
    acc_b, stops, m = _brake(v, d, dt)
    for j in range(N + 1):
        Xs[j] = x, y, v, th
        if v == 0.0 and stop_step < 0:
            stop_step = j
        q = path_point(V, s, dirs, N, sigma)
        e = math.hypot(x - q[0], y - q[1])
        errs.append(e)
        if e > dev:
            dev, dev_step = e, j
        if j == N:
            break
        held = j < hold
        if held:
            u0, u1 = plan_u[j]
        else:
            u0, u1 = acc_b, 0.0
            margin = min(margin, m)
        acc = max(min(u0, p.acc_max), p.acc_min)
        adv = v * dt + acc * dt * dt / 2.0
        xn, yn = x + math.cos(th) * adv, y + math.sin(th) * adv
        vn = 0.0 if (not held and stops) else min(max(v + acc * dt, 0.0), p.speed_max)
        sigma += max(adv, 0.0)
        acc_b, stops, m = _brake(vn, d, dt)
        if not held and j < N - 1:
            adv_n = vn * dt + acc_b * dt * dt / 2.0
            if vn != 0.0:
                margin = min(margin, abs(adv_n - MIN_ADVANCE))
            if adv_n >= MIN_ADVANCE:
                target = sigma + adv_n
                margin = min(margin, abs(target - s[N]))
                if target >= s[N]:
                    overrun += 1
                q = path_point(V, s, dirs, N, target)
                turn = math.atan2(q[1] - yn, q[0] - xn) - th
                k = math.ceil((turn - math.pi) / (2.0 * math.pi))
                wrapped = turn - 2.0 * math.pi * k
                margin = min(margin, math.pi - abs(wrapped))  # the branch cut of the turn
                u1 = wrapped / dt
        w = max(min(u1, v * yaw_hi), v * yaw_lo)
        if not held:
            if u1 != 0.0 or v != 0.0:
                margin = min(margin, abs(u1 - v * yaw_hi), abs(u1 - v * yaw_lo))
            if w != u1:
                clamped += 1
            u1 = w
        Us[j] = u0, u1
        x, y, v, th = xn, yn, vn, th + w * dt
    sp = np.array([stop_step, sigma, v, dev, dev_step, clamped, overrun, 0.0])
    # by how much the largest deviation leads the next; the copies a held state makes of it are the same bits anywhere and do not count
    rest = [e for j, e in enumerate(errs) if j != dev_step and not (0 <= stop_step <= j and e == dev)]
    return Xs, Us, sp, margin, (dev - max(rest) if rest else math.inf), np.array(errs)


def stop_restate(p, N, X, U, decel, hold, max_deviation=math.inf, plan_cost=None, decel_weight=0.0, allow_moving=False):
    """X (B, 4(N+1)), U (B, 2N), decel (D,).  Returns dict(X (B*D, 4(N+1)), U (B*D, 2N), sp (B*D, 8), cost (B*D,), margin (B*D,): how far
    the row's nearest comparison is from flipping, dev_gap (B*D,): by how much the largest deviation leads the next, errs (B*D, N+1): the
    deviation at every step)."""
    X, U, decel = np.asarray(X, dtype=np.float64), np.asarray(U, dtype=np.float64), np.asarray(decel, dtype=np.float64).reshape(-1)
    B, D = X.shape[0], decel.size
    R = B * D
    Xs, Us, sp, cost = np.full((R, 4 * (N + 1)), np.nan), np.full((R, 2 * N), np.nan), np.zeros((R, 8)), np.full(R, np.nan)
    margin, dev_gap, errs = np.full(R, math.inf), np.full(R, math.inf), np.full((R, N + 1), np.nan)
    for r in range(R):
        b, l = divmod(r, D)
        d = float(decel[l])
        if not (np.isfinite(X[b]).all() and np.isfinite(U[b]).all()) or not (0.0 < d <= -p.acc_min):
            sp[r] = -1.0, np.nan, np.nan, np.nan, -1.0, 0.0, 0.0, 1.0
            continue
        x, u, sp[r], margin[r], dev_gap[r], errs[r] = _row_restate(p, N, X[b], U[b], d, hold)
        Xs[r], Us[r] = x.reshape(-1), u.reshape(-1)
        at_rest = 0 <= sp[r, STOP_STEP] <= N - 1
        if sp[r, DEVIATION] <= max_deviation and (at_rest or allow_moving):
            cost[r] = decel_weight * d + (0.0 if plan_cost is None else plan_cost[b])
    return dict(X=Xs, U=Us, sp=sp, cost=cost, margin=margin, dev_gap=dev_gap, errs=errs)


# ---- plans and scenes ---------------------------------------------------------------------------------------------------------------
def nominal(O, p, N, x0, U):
    """The oracle's nominal trajectory over U from x0: (4(N+1),)."""
    x0, U = np.ascontiguousarray(x0, dtype=np.float64), np.ascontiguousarray(U, dtype=np.float64).reshape(-1)
    X = np.zeros(4 * (N + 1))
    O.lib().oracle_nominal_trajectory(C.byref(p), C.c_int(N), _p(x0), _p(U), _p(X))
    return X


def model_plan(O, p, N, x0, acc, yaw):
    U = np.stack([np.broadcast_to(acc, (N,)), np.broadcast_to(yaw, (N,))], axis=1).astype(np.float64).reshape(-1)
    return nominal(O, p, N, x0, U), U


def level_that_stops_after(v, dt, k):
    """A level at which a row of speed v comes to rest exactly k steps later, decided by half a step: v/(d dt) = k - 0.5."""
    return v / (dt * (k - 0.5))


def plans_a8(O, p, N=8):
    dt = p.timestep
    plans = [model_plan(O, p, N, [0.0, 0.0, 0.93, 0.1], -4.0, 0.02),        # stops within three steps, then steps backwards by a dt^2/2
             model_plan(O, p, N, [1.0, 2.0, 3.07, -0.4], 0.2, 0.05),          # (made lost below)
             None,                                                           # a corner no steering angle follows
             model_plan(O, p, N, [5.0, -1.0, 2.11, 3.1], 0.1, 0.35),          # the heading grows past pi
             model_plan(O, p, N, [-2.0, 0.5, 0.0, 0.7], 0.0, 0.0)]            # at rest
    t = np.arange(N + 1)
    th = 0.3 + 0.45 * np.maximum(t - 2, 0)  # 0.45 rad a step at 1.1 m/s: four times what the clamp allows
    X = np.zeros((N + 1, 4))
    X[:, 2], X[:, 3] = 1.13, th
    X[1:, 0] = np.cumsum(1.13 * dt * np.cos(th[:-1]))
    X[1:, 1] = np.cumsum(1.13 * dt * np.sin(th[:-1]))
    plans[2] = (X.reshape(-1), np.stack([np.zeros(N), np.diff(th) / dt], axis=1).reshape(-1))
    X, U = np.array([x for x, _ in plans]), np.array([u for _, u in plans])
    good = X.copy()
    X[1, 4 * 3 + 1] = np.nan
    return X, U, good


def _curved(O, N=40, B=6):
    p = O.default_params(N)
    i = np.arange(200.0)
    path = np.stack([i, 6.0 * np.sin(0.06 * i)], axis=1)
    x0 = np.array([[0.0, 0.25 * b - 0.5, 8.03 - 0.4 * b, 0.33] for b in range(B)])
    plans = [O.local_plan(p, path, x0[b]) for b in range(B)]
    poly, fl = np.array([c for c, _ in plans]), np.array([[ref[0, 0], ref[-1, 0]] for _, ref in plans])
    U = np.tile(O.default_control_seq(N), (B, 1))
    r = O.solve_batch(p, N, 0, x0, U, poly, fl, None, None, None, threads=min(6, O.max_threads()))
    return p, r["X"].reshape(B, -1).copy(), r["U"].reshape(B, -1).copy(), r["J"].copy()


def _finish(name, p, N, X, U, decel, hold, max_deviation=math.inf, plan_cost=None, decel_weight=0.0):
    s = dict(name=name, p=p, N=N, B=X.shape[0], D=len(decel), X=X, U=U, decel=np.asarray(decel, dtype=np.float64), hold=hold,
             max_deviation=max_deviation, plan_cost=plan_cost, decel_weight=decel_weight)
    for moving in (False, True):
        s[moving] = stop_restate(p, N, X, U, s["decel"], hold, max_deviation, plan_cost, decel_weight, moving)
    return s


@pytest.fixture(scope="module")
def scenes(oracle):
    """Every scene's inputs and restatement (both settings of ALLOW_MOVING).  Computed once; never modified."""
    O = oracle
    out = {}
    p1 = O.default_params(1)
    X, U = model_plan(O, p1, 1, [0.3, -0.2, 3.07, 0.4], 0.3, 0.1)
    out["A1"] = _finish("A1", p1, 1, X[None], U[None], [2.03], 0)
    p8 = O.default_params(8)
    X, U, _ = plans_a8(O, p8)
    v2 = float(nominal(O, p8, 8, X[3, :4], U[3]).reshape(9, 4)[2, 2])  # plan 3's speed when braking starts (hold 2)
    levels = [level_that_stops_after(v2, p8.timestep, 6), level_that_stops_after(v2, p8.timestep, 5), 5.2]  # at rest at step 8 = N, 7 = N-1, earlier
    out["A8"] = _finish("A8", p8, 8, X, U, levels, 2, plan_cost=np.array([3.0, 1.0, 4.0, 1.5, 9.0]), decel_weight=10.0)
    out["H8"] = _finish("H8", p8, 8, X, U, levels, 8)
    out["D65"] = _finish("D65", p8, 8, X[[0, 3, 2]], U[[0, 3, 2]], np.linspace(0.52, 5.5, 65), 0, decel_weight=1.0)
    p40, X, U, J = _curved(O)
    X[5], U[5] = model_plan(O, p40, 40, [0.0, 1.0, 8.03, 0.2], -4.0, 0.08)  # brakes harder than most levels: overrun
    free = stop_restate(p40, 40, X, U, [1.03, 2.03, 3.07, 4.1, 5.5], 1)
    rest = (free["sp"][:, STOP_STEP] >= 0) & (free["sp"][:, STOP_STEP] <= 39)
    dv, at_rest = np.sort(free["sp"][:, DEVIATION]), free["sp"][rest, DEVIATION]
    gaps = np.where((dv[:-1] >= at_rest.min()) & (dv[1:] <= at_rest.max()), np.diff(dv), 0.0)
    k = int(np.argmax(gaps))  # the widest gap among all deviations that has rows that come to rest on either side of it
    out["C40"] = _finish("C40", p40, 40, X, U, [1.03, 2.03, 3.07, 4.1, 5.5], 1, max_deviation=0.5 * (dv[k] + dv[k + 1]), plan_cost=J, decel_weight=1e6)
    return out


GPU_SCENES = ["A1", "A8", "H8", "D65", "C40"]


# ---- CPU: declarations ---------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_call(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_STOP_FIELDS\s+8\b", h) and re.search(r"#define\s+CILQR_STOP_ALLOW_MOVING\s+1u", h)
    assert float(re.search(r"#define\s+CILQR_STOP_MIN_ADVANCE\s+(\S+)", h).group(1)) == MIN_ADVANCE == cilqr.STOP_MIN_ADVANCE
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_SP_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "SP_" + name) == i
    assert cilqr.STOP_FIELDS == 8 and cilqr.STOP_ALLOW_MOVING == 1
    assert callable(cilqr.Solver.stop_plans) and callable(cilqr.Solver.stop_plans_device)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_stop_plans\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_stop.hip" in mk and len(re.findall(r"build/cilqr_stop\.o(?!:)", mk)) == 2  # `check` and its resource list
    text = re.sub(r"\s*\n \*\s*", " ", full)
    for phrase in ("a row's bits depend on plan b, level l, hold and the parameters alone", "A row is as safe as those checks say, no more",
                   "a stopping vehicle stops and does not reverse", "a stop it never sees finished is not a verified stop"):
        assert phrase in text, phrase


def test_argument_errors_need_no_device(cilqr):
    """Decided before the handle is looked at (there is none here); valid arguments reach the handle check.  The host-buffer form reads
    its levels; the device form cannot (there a bad level loses its rows: test_a_bad_level_on_the_device)."""
    L = cilqr.lib()
    B, N, D = 2, 4, 3
    R = B * D
    arrays = dict(X=np.zeros((B, 4 * (N + 1))), U=np.zeros((B, 2 * N)), decel=np.array([1.0, 2.0, 3.0]), X_stop=np.zeros((R, 4 * (N + 1))),
                  U_stop=np.zeros((R, 2 * N)), sp=np.zeros((R, 8)))
    cost, plan_cost = np.zeros(R), np.zeros(B)
    no_handle = C.c_void_p()
    d = C.c_double
    nan, inf = float("nan"), float("inf")

    def call(dev, D=D, hold=1, max_deviation=0.5, weight=1.0, flags=0, levels=None, **nulls):
        a = dict(arrays)
        a.update(nulls)
        if levels is not None:
            a["decel"] = np.asarray(levels, dtype=np.float64)
        f = L.cilqr_stop_plans_device if dev else L.cilqr_stop_plans
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, D, _p(a["X"]), _p(a["U"]), _p(a["decel"]), hold, d(max_deviation), _p(plan_cost), d(weight), C.c_uint32(flags),
                 _p(a["X_stop"]), _p(a["U_stop"]), _p(a["sp"]), _p(cost))

    for dev in (False, True):
        for name in arrays:
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, D=0) == ERR_ARG and b"D = 0" in L.cilqr_last_error()
        assert call(dev, hold=-1) == ERR_ARG and b"hold = -1" in L.cilqr_last_error()
        for bad in (-1e-3, nan, -inf):
            assert call(dev, max_deviation=bad) == ERR_ARG and b"max_deviation is negative or NaN" in L.cilqr_last_error(), bad
        for bad in (nan, inf, -inf):
            assert call(dev, weight=bad) == ERR_ARG and b"decel_weight is not finite" in L.cilqr_last_error(), bad
        assert call(dev, flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, hold=0, max_deviation=inf, weight=0.0, flags=1) == ERR_ARG and b"null handle" in L.cilqr_last_error()
    for bad in (0.0, -1.0, nan, inf):
        assert call(False, levels=[1.0, bad, 3.0]) == ERR_ARG and b"decel[1] is not finite or not positive" in L.cilqr_last_error(), bad


def _build(tmp_path, source, *includes, lib=False):
    exe = str(tmp_path / source.replace(".cpp", ""))
    link = ["-L" + os.path.join(PKG, "lib"), "-lcilqr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib")] if lib else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall"] + ["-I" + d for d in includes] + ["-o", exe, os.path.join(ROOT, "tests", "cpp", source)] + link, check=True)
    return exe


def test_the_facade_exports_the_setter():
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_stop_fallback\s*\(\s*const\s+std::vector<double>&\s+decels\s*,\s*int\s+hold\s*=\s*1\s*,\s*double\s+max_deviation\s*=\s*0\.5\s*,"
                     r"\s*bool\s+on\s*=\s*true\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_stop\s*,\s*last_stop_footprint\s*;", f)
    assert re.search(r"int\s+last_stop_pick\s*=\s*-1\s*,\s*last_stop_level\s*=\s*-1\s*;", f)
    lay = open(os.path.join(PKG, "host", "candidate_layout.h")).read()
    assert re.search(r"bool\s+stop_fallback\s*=\s*false\s*;", lay) and re.search(r"bool\s+stop_fallback_check\s*\(\s*\)\s*const", lay)
    replay = open(os.path.join(PKG, "host", "replay_main.cpp")).read()
    assert "--stop-fallback" in replay and "set_stop_fallback" in replay


def test_the_layout_with_the_stop_fallback_flag(tmp_path):
    """tests/cpp/candidate_layout_stop_dump.cpp beside the map clearance dump: with the flag off every record — predicates, every offset
    and `end` — is what that dump gives, whatever D is; with it on the stage's arrays lie behind every earlier array, none of which
    moves, and the stage runs only under set_footprint_check."""
    inc = os.path.join(PKG, "host"), os.path.join(ROOT, "include")
    old, new = (_build(tmp_path, n, *inc) for n in ("candidate_layout_map_clearance_dump.cpp", "candidate_layout_stop_dump.cpp"))

    def names(exe):
        return {k: v.split() for k, v in (line.split(":") for line in subprocess.run([exe, "names"], check=True, capture_output=True, text=True).stdout.splitlines())}
    n0, n1 = names(old), names(new)
    assert n1["flags"] == n0["flags"] + ["stop_fallback"] and n1["predicates"] == n0["predicates"] + ["stop_fallback_check"]  # one flag, one predicate
    assert n1["arrays"] == n0["arrays"][:-1] and n0["arrays"][-1] == "end"  # every earlier array, in its order
    stop = n1["stop"]
    assert stop == ["stlv", "stX", "stU", "stsp", "stcost", "stfp", "stfptotal", "stmc", "stmctotal", "stpair", "end"]
    rng = np.random.default_rng(7)
    n = 600
    rec = np.zeros((n, 9), dtype=np.uint64)
    rec[:, 0] = rng.integers(0, 2 ** len(n0["flags"]), n)
    rec[:, 1], rec[:, 2], rec[:, 3], rec[:, 4] = rng.integers(1, 13, n), rng.integers(1, 51, n), rng.integers(0, 5, n), rng.integers(0, 300, n)
    rec[:, 5], rec[:, 6], rec[:, 7], rec[:, 8] = rng.integers(0, 3, n), rng.integers(0, 3, n), rng.integers(0, 28, n), rng.integers(1, 9, n)

    def run(exe, records):
        out = subprocess.run([exe], input=np.ascontiguousarray(records).tobytes(), capture_output=True, check=True).stdout
        return np.frombuffer(out, dtype=np.uint64).reshape(len(records), -1).astype(np.int64)
    off_old, off_new = run(old, rec[:, :8]), run(new, rec)
    na = len(n1["arrays"])
    assert np.array_equal(off_new[:, :1 + na], off_old[:, :1 + na])              # flag off: every predicate (the new one is 0) and offset
    assert np.array_equal(off_new[:, -1], off_old[:, -1])                        # ... and `end`
    assert np.all(off_new[:, 1 + na:-1] == off_old[:, -1:])                      # ... the stop arrays empty, at the old end
    on = rec.copy()
    on[:, 0] |= np.uint64(1 << len(n0["flags"]))
    got = run(new, on)
    assert np.array_equal(got[:, 1:1 + na], off_old[:, 1:1 + na])                # flag on: nothing before the new arrays moves
    k = {name: 1 + na + i for i, name in enumerate(stop)}
    B, N, D = (rec[:, c].astype(np.int64) for c in (1, 2, 8))
    even = lambda v: (v + 1) // 2 * 2  # noqa: E731
    assert np.array_equal(got[:, k["stlv"]], off_old[:, -1])                     # the first of them starts at the old end
    sizes = [D, B * 4 * (N + 1), B * 2 * N, B * 8, B, B * 12, B, B * 8, B, np.full(n, 2)]
    for (a, b), size in zip(zip(stop[:-1], stop[1:]), sizes):
        assert np.array_equal(got[:, k[b]] - got[:, k[a]], even(size)), (a, b)
    bit = {name: i for i, name in enumerate(n1["predicates"])}
    fbit = {name: i for i, name in enumerate(n1["flags"])}
    footprint = ((on[:, 0] >> np.uint64(fbit["footprint"])) & np.uint64(1)).astype(np.int64)
    runs = (got[:, 0] >> bit["stop_fallback_check"]) & 1
    assert np.array_equal(runs, footprint) and 0 < runs.sum() < n
    assert np.all(((got[:, 0] >> bit["in_block"]) & 1)[runs == 1])
    assert np.array_equal(got[:, 0] & ((1 << bit["stop_fallback_check"]) - 1), off_old[:, 0])  # no earlier predicate changes


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_stop.cpp: plan_stop_plans laid out without an arena against host_arena_bytes at the shapes include/cilqr.h says
    fit (B*D = max_batch rows in every split, N up to the largest horizon); host_arena_bytes is still what
    tests/golden/host_arena_cap.json recorded; one layout in full."""
    import json
    exe = _build(tmp_path, "host_plan_stop.cpp", os.path.join(ROOT, "include"), os.path.join(PKG, "csrc"))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "8 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20
    B, N, D = 3, 5, 4
    R = B * D
    r = subprocess.run([exe, "layout", str(B), str(N), str(D), "1"], capture_output=True, text=True, check=True)
    entries = [[int(v) for v in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("entry ")]
    sizes = [B * 4 * (N + 1) * 8, B * 2 * N * 8, D * 8, B * 8, R * 4 * (N + 1) * 8, R * 2 * N * 8, R * 8 * 8, R * 8]  # X, U, decel, plan_cost | X_stop, U_stop, sp, cost
    at = 0
    for (off, nbytes, src, dst), want in zip(entries, sizes):
        assert (off, nbytes) == (at, want)
        at = (off + nbytes + 15) // 16 * 16
    assert len(entries) == 8 and [e[2] for e in entries] == [1, 1, 1, 1, 0, 0, 0, 0] and [e[3] for e in entries] == [0, 0, 0, 0, 1, 1, 1, 1]
    tail = dict(zip(r.stdout.splitlines()[-1].split()[1::2], (int(v) for v in r.stdout.splitlines()[-1].split()[2::2])))
    assert tail["ok"] == 1 and tail["in_end"] == tail["out_begin"] == entries[4][0] and tail["end"] == at


# ---- CPU: the restatement against the oracle's model, physics and brute force ------------------------------------------------------------
@pytest.fixture(scope="module")
def curved(oracle):
    p, X, U, J = _curved(oracle)
    return dict(p=p, N=40, X=X, U=U, J=J)


def test_the_restatement_is_the_models_chain(oracle, curved):
    """On the oracle's solves of the curved scene: the oracle's nominal trajectory over U_stop reproduces X_stop to 1e-12 (the speed of
    the stopping step is 0 by definition where the model's own arithmetic may leave a rounding); hold >= N returns the plan's U bit for
    bit."""
    p, N, X, U = curved["p"], curved["N"], curved["X"], curved["U"]
    B = X.shape[0]
    decel = np.array([1.03, 2.03, 3.07, 4.1, 5.5])
    for hold in (0, 1, 7):
        w = stop_restate(p, N, X, U, decel, hold)
        for r in range(B * len(decel)):
            b = r // len(decel)
            again = nominal(oracle, p, N, X[b, :4], w["U"][r])
            assert np.max(np.abs(again - w["X"][r])) <= 1e-12, (hold, r)
            assert np.array_equal(w["X"][r, :4], X[b, :4])
            assert np.array_equal(w["U"][r, :2 * hold], U[b, :2 * hold])
    w = stop_restate(p, N, X, U, decel, N)
    assert np.array_equal(_bits(w["U"]), _bits(np.repeat(U, len(decel), axis=0)))
    assert np.max(np.abs(w["X"] - np.repeat(X, len(decel), axis=0))) <= 1e-12 and np.max(w["sp"][:, DEVIATION]) <= 1e-12
    assert np.array_equal(_bits(stop_restate(p, N, X, U, decel, N + 3)["U"]), _bits(w["U"]))


def test_a_stopped_row_has_travelled_v0_squared_over_2d(curved):
    p, N, X, U = curved["p"], curved["N"], curved["X"], curved["U"]
    decel = np.array([1.03, 2.03, 3.07, 4.1, 5.5])
    w = stop_restate(p, N, X, U, decel, 0)
    st = w["X"].reshape(-1, N + 1, 4)
    n_stopped = 0
    for r in range(st.shape[0]):
        b, l = divmod(r, len(decel))
        v0, d = X[b, 2], decel[l]
        k = int(w["sp"][r, STOP_STEP])
        if k < 0:
            assert v0 - d * p.timestep * N > 0.0 and w["sp"][r, END_SPEED] > 0.0  # too gentle for the horizon
            continue
        n_stopped += 1
        assert abs(w["sp"][r, DISTANCE] - v0 * v0 / (2.0 * d)) <= v0 * p.timestep  # within one step's advance
        assert np.all(st[r, k:, 2] == 0.0) and np.all(st[r, k:] == st[r, k]) and np.all(w["U"][r].reshape(N, 2)[k:] == 0.0)  # held
        assert np.all(np.diff(st[r, :, 2]) <= 0.0) and w["sp"][r, END_SPEED] == 0.0
        assert np.all(w["U"][r].reshape(N, 2)[:k, 0] >= -d - 1e-15)
    assert n_stopped >= 4 * X.shape[0] - 2 and (w["sp"][:, STOP_STEP] < 0).any()


def test_the_deviation_against_a_densely_sampled_path(curved):
    """SP_DEVIATION is measured against Q(sigma_j), a point of the path, so it is never below the distance to the path itself; on these
    plans the lag along the path is small, and the brute-force distance to the sampled polyline and ray is within the sampling pitch of
    it or below it."""
    from scipy.spatial import cKDTree
    p, N, X, U = curved["p"], curved["N"], curved["X"], curved["U"]
    pitch = 1e-3
    decel = np.array([2.03, 4.1])
    w = stop_restate(p, N, X, U, decel, 1)
    for b in range(X.shape[0]):
        V, s, dirs = path_of(X[b], N)
        sig = np.arange(0.0, s[N] + 30.0, pitch)
        tree = cKDTree(np.array([path_point(V, s, dirs, N, v) for v in sig]))
        for l in range(len(decel)):
            r = b * len(decel) + l
            st = w["X"][r].reshape(N + 1, 4)
            brute = tree.query(st[:, :2])[0]
            assert brute.max() <= w["sp"][r, DEVIATION] + pitch
            j = int(w["sp"][r, DEVIATION_STEP])
            assert w["sp"][r, DEVIATION] - brute[j] <= 0.05 * w["sp"][r, DEVIATION] + pitch  # pursuit keeps the row beside its own arc length
    print("deviation %s" % np.round(w["sp"][:, DEVIATION], 5).tolist())
    assert w["sp"][:, DEVIATION].max() < 0.05


@pytest.mark.parametrize("name", GPU_SCENES)
def test_conditions(scenes, name):
    """On the restatement alone: every scene is decided, and between them the scenes hold every case the device tests rely on."""
    s = scenes[name]
    w = s[False]
    live = w["sp"][:, LOST] == 0
    few = slice(None, 30)
    print("scene %s: stop %s clamped %s overrun %s deviation %s margin %.3g" % (
        name, w["sp"][few, STOP_STEP].tolist(), w["sp"][few, CLAMPED_STEPS].tolist(), w["sp"][few, OVERRUN_STEPS].tolist(),
        np.round(w["sp"][few, DEVIATION], 5).tolist(), w["margin"][live].min()))
    assert w["margin"][live].min() > DECIDED, w["margin"]
    # the STEP of the largest deviation is an index among values: it is compared exactly where it leads by more than DECIDED, and
    # elsewhere (a row that creeps, a row on its path) the device's step must be one whose deviation is the largest within ABS_TOL
    decided = w["dev_gap"][live] > DECIDED
    print("  deviation step decided in %d of %d rows" % (decided.sum(), decided.size))
    assert name in ("A1", "H8") or decided.sum() >= decided.size // 3  # (A1 and H8: rows on their paths)
    if math.isfinite(s["max_deviation"]):
        assert np.abs(w["sp"][live, DEVIATION] - s["max_deviation"]).min() > DECIDED


def test_the_scenes_hold_every_case(scenes):
    a, N = scenes["A8"], 8
    sp = a[False]["sp"].reshape(5, 3, 8)
    assert np.all(sp[1, :, LOST] == 1) and np.all(sp[[0, 2, 3, 4], :, LOST] == 0)              # a lost plan between two good ones
    assert np.isnan(a[False]["X"].reshape(5, 3, -1)[1]).all() and np.all(sp[1, :, STOP_STEP] == -1)
    assert sp[3, :, STOP_STEP].tolist()[:2] == [N, N - 1]                                     # at rest at step N, at step N - 1
    cost, cost_moving = a[False]["cost"].reshape(5, 3), a[True]["cost"].reshape(5, 3)
    assert np.isnan(cost[3, 0]) and np.isfinite(cost_moving[3, 0]) and np.isfinite(cost[3, 1])
    assert cost[3, 1] == 10.0 * a["decel"][1] + 1.5
    assert np.all(sp[4, :, STOP_STEP] == 0) and np.all(sp[4, :, DISTANCE] == 0.0)               # v0 = 0
    V, s_arc, _ = path_of(a["X"][0], N)
    assert (np.diff(s_arc) == 0.0).sum() >= 3                                                 # the plan itself stopped: segments of length 0
    assert sp[2, :, CLAMPED_STEPS].min() >= 2                                                  # the corner no steering angle follows
    th = a[False]["X"].reshape(5, 3, N + 1, 4)[3, :, :, 3]
    assert th.min() < math.pi < th.max()                                                      # a heading that crosses pi
    # a row held after its stop repeats its last deviation bit for bit: where that is the largest, "lowest on equal values" decides the step,
    # and the device tests compare such a row's step exactly (stop_restate leaves the held copies out of dev_gap)
    w8 = a[False]
    held = [r for r in range(15) if w8["sp"][r, LOST] == 0 and 0 < w8["sp"][r, STOP_STEP] <= w8["sp"][r, DEVIATION_STEP] < N
            and w8["errs"][r, N] == w8["sp"][r, DEVIATION] and w8["dev_gap"][r] > DECIDED]
    assert held, "no row whose largest deviation is repeated by the held state"
    h = scenes["H8"][False]
    assert np.array_equal(_bits(h["U"].reshape(5, 3, -1)[[0, 2, 3, 4]]), _bits(np.repeat(a["U"][[0, 2, 3, 4], None], 3, axis=1)))
    c = scenes["C40"]
    sp = c[False]["sp"].reshape(6, 5, 8)
    assert np.all(sp[:5, 0, STOP_STEP] == -1) and np.isnan(c[False]["cost"].reshape(6, 5)[:5, 0]).all()  # a level that never stops
    assert sp[5, 1, OVERRUN_STEPS] >= 10 and np.all(sp[:5, 1:, OVERRUN_STEPS] == 0)          # the plan brakes harder than the level
    rejected = (sp[:, :, DEVIATION] > c["max_deviation"]) & (sp[:, :, STOP_STEP] >= 0) & (sp[:, :, STOP_STEP] <= 39)
    assert rejected.any() and np.isnan(c[False]["cost"].reshape(6, 5)[rejected]).all() and np.isfinite(c[False]["cost"]).any()
    assert scenes["D65"]["D"] == 65 and scenes["A1"]["N"] == 1 and {scenes[k]["hold"] for k in GPU_SCENES} >= {0, 2, 8}


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(40), max_batch=195, max_horizon=40, max_obstacles=1, device=0)
    yield s
    s.close()


def _host(solver, s, moving=False, plans=None, levels=None, cost=True):
    b = list(range(s["B"])) if plans is None else list(plans)
    decel = s["decel"] if levels is None else s["decel"][list(levels)]
    return solver.stop_plans(s["N"], s["X"][b], s["U"][b], decel, hold=s["hold"], max_deviation=s["max_deviation"],
                             plan_cost=None if s["plan_cost"] is None else s["plan_cost"][b], decel_weight=s["decel_weight"],
                             allow_moving=moving, want_cost=cost)


def _device(cilqr, solver, s, moving=False, decel=None):
    import torch
    B, N = s["B"], s["N"]
    decel = s["decel"] if decel is None else np.asarray(decel, dtype=np.float64)
    R = B * len(decel)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    X, U, lv = up(s["X"]), up(s["U"]), up(decel)
    pc = None if s["plan_cost"] is None else up(s["plan_cost"])
    Xs, Us, sp, cost = (torch.full(shape, -7.0, dtype=torch.float64, device=dev) for shape in ((R, 4 * (N + 1)), (R, 2 * N), (R, 8), (R,)))
    torch.cuda.synchronize(dev)
    solver.stop_plans_device(st, B, N, len(decel), X.data_ptr(), U.data_ptr(), lv.data_ptr(), Xs.data_ptr(), Us.data_ptr(), sp.data_ptr(),
                             hold=s["hold"], max_deviation=s["max_deviation"], plan_cost=0 if pc is None else pc.data_ptr(),
                             decel_weight=s["decel_weight"], flags=cilqr.STOP_ALLOW_MOVING if moving else 0, cost=cost.data_ptr())
    torch.cuda.synchronize(dev)
    return dict(X=Xs.cpu().numpy(), U=Us.cpu().numpy(), sp=sp.cpu().numpy(), cost=cost.cpu().numpy())


def _close(a, b):
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and bool(np.all(np.abs(a[~nan] - b[~nan]) <= ABS_TOL))


def _check_against(got, want, what, rows=slice(None)):
    sp, w = got["sp"], want["sp"][rows]
    few = slice(None, 30)
    print("%s: stop %s distance %s deviation %s clamped %s overrun %s; largest |dX| %.3g |dU| %.3g" % (
        what, sp[few, STOP_STEP].tolist(), np.round(sp[few, DISTANCE], 6).tolist(), np.round(sp[few, DEVIATION], 6).tolist(), sp[few, CLAMPED_STEPS].tolist(),
        sp[few, OVERRUN_STEPS].tolist(), np.nanmax(np.abs(got["X"] - want["X"][rows]), initial=0.0), np.nanmax(np.abs(got["U"] - want["U"][rows]), initial=0.0)))
    assert _close(got["X"], want["X"][rows]) and _close(got["U"], want["U"][rows]), what
    for f in VALUES:
        assert _close(sp[:, f], w[:, f]), (what, FIELDS[f], sp[:, f].tolist(), w[:, f].tolist())
    for f in EXACT:
        decided = want["dev_gap"][rows] > DECIDED if f == DEVIATION_STEP else np.ones(len(w), dtype=bool)
        assert np.array_equal(sp[decided, f], w[decided, f]), (what, FIELDS[f], sp[:, f].tolist(), w[:, f].tolist())
    errs = want["errs"][rows]
    for r in np.nonzero(w[:, LOST] == 0)[0]:  # wherever it is not decided: a step whose deviation is the largest within the tolerance
        k = int(sp[r, DEVIATION_STEP])
        assert 0 <= k <= errs.shape[1] - 1 and errs[r, k] >= w[r, DEVIATION] - ABS_TOL, (what, r, k)
    if got["cost"] is not None:
        assert _close(got["cost"], want["cost"][rows]), (what, got["cost"], want["cost"][rows])


def _same_bits(a, b, rows_b=slice(None)):
    return all(np.array_equal(_bits(a[k]), _bits(b[k][rows_b])) for k in ("X", "U", "sp", "cost"))


@gpu
@pytest.mark.parametrize("name", GPU_SCENES)
def test_rows_against_the_restatement(cilqr, solver, scenes, name):
    """Both settings of ALLOW_MOVING; the host form and the device form agree bit for bit."""
    s = scenes[name]
    for moving in (False, True):
        host = _host(solver, s, moving)
        _check_against(host, s[moving], "scene %s, allow moving %s, host form" % (name, moving))
        dev = _device(cilqr, solver, s, moving)
        _check_against(dev, s[moving], "scene %s, allow moving %s, device form" % (name, moving))
        assert _same_bits(host, dev)


@gpu
def test_a_rows_bits_do_not_depend_on_its_place(cilqr, solver, scenes):
    """Plan b alone (B = 1) and inside the batch, level l alone (D = 1) and among the others, a batch in another order: the same bits in
    every output."""
    for name in ("A8", "C40"):
        s = scenes[name]
        B, D = s["B"], s["D"]
        whole = _host(solver, s)
        for b in range(B):
            assert _same_bits(_host(solver, s, plans=[b]), whole, rows_b=slice(b * D, (b + 1) * D)), (name, b)
        for l in range(D):
            assert _same_bits(_host(solver, s, levels=[l]), whole, rows_b=slice(l, None, D)), (name, l)
        order = list(range(B))[::-1]
        rows = [b * D + l for b in order for l in range(D)]
        assert _same_bits(_host(solver, s, plans=order), whole, rows_b=rows), name
    s = scenes["D65"]  # a level's bits in a chunk of 64 and alone
    whole = _host(solver, s)
    for l in (0, 63, 64):
        assert _same_bits(_host(solver, s, levels=[l]), whole, rows_b=slice(l, None, 65)), l


@gpu
def test_cost_left_out_and_a_bad_level_on_the_device(cilqr, solver, scenes):
    s = scenes["A8"]
    full, bare = _host(solver, s), _host(solver, s, cost=False)
    assert bare["cost"] is None and all(np.array_equal(_bits(bare[k]), _bits(full[k])) for k in ("X", "U", "sp"))
    # the device form cannot read its levels on the host: rows of a level outside (0, -acc_min] are lost, the others are what they were
    bad = _device(cilqr, solver, s, decel=[s["decel"][0], 5.6, s["decel"][2]])
    sp = bad["sp"].reshape(5, 3, 8)
    assert np.all(sp[:, 1, LOST] == 1) and np.isnan(bad["X"].reshape(5, 3, -1)[:, 1]).all() and np.isnan(bad["cost"].reshape(5, 3)[:, 1]).all()
    good = _device(cilqr, solver, s)
    for k in ("X", "U", "sp", "cost"):
        a, b = bad[k].reshape(5, 3, -1)[:, [0, 2]], good[k].reshape(5, 3, -1)[:, [0, 2]]
        assert np.array_equal(_bits(a), _bits(b)), k
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*above -acc_min" % ERR_ARG):
        solver.stop_plans(s["N"], s["X"], s["U"], [1.0, 5.6])


@gpu
def test_limits(cilqr, scenes):
    s = scenes["A8"]
    sv = cilqr.Solver(cilqr.default_params(8), max_batch=15, max_horizon=8, max_obstacles=0, device=0)
    try:
        _check_against(sv.stop_plans(8, s["X"], s["U"], s["decel"], hold=2, plan_cost=s["plan_cost"], decel_weight=10.0), s[False], "B*D = max_batch")
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*B\\*D = 20 outside" % ERR_ARG):
            sv.stop_plans(8, s["X"], s["U"], [1.0, 2.0, 3.0, 4.0])
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: N=9 outside" % ERR_ARG):
            sv.stop_plans(9, np.zeros((1, 40)), np.zeros((1, 18)), [1.0])
    finally:
        sv.close()


# ---- scene W: every solved candidate is rejected, a middle braking level is clear ------------------------------------------------------
W_N, W_B, W_LEVELS, W_HOLD, W_WALL_X, W_THRESHOLD, W_WEIGHT = 40, 4, (1.5, 3.0, 5.0), 1, 9.0, 50.0, 1e6
W_GEOM, W_MAP_POSE = (24.0, 8.0, 0.2, 11.0, 0.0), (0.1, -0.05, 0.03)
W_BOX = (W_WALL_X + 0.25, 0.0, 0.5, 8.0)  # the second variant: an obstacle rectangle across the road (x, y, length, width), heading 0


@pytest.fixture(scope="module")
def scene_w(oracle):
    """A straight path, four candidates 0 ... 0.9 m beside it at about 5 m/s, the oracle's solves; a wall of occupied cells (variant `map`)
    or an obstacle rectangle (variant `box`) across the whole road 9 m ahead.  Everything the device tests use is restated here."""
    from test_footprint import restate
    O = oracle
    N, B, D = W_N, W_B, len(W_LEVELS)
    p = O.default_params(N)
    path = np.stack([np.arange(200.0), np.zeros(200)], axis=1)
    x0 = np.array([[0.0, 0.3 * b, 5.03, 0.0] for b in range(B)])
    plans = [O.local_plan(p, path, x0[b]) for b in range(B)]
    poly, fl = np.array([c for c, _ in plans]), np.array([[ref[0, 0], ref[-1, 0]] for _, ref in plans])
    r = O.solve_batch(p, N, 0, x0, np.tile(O.default_control_seq(N), (B, 1)), poly, fl, None, None, None, threads=min(4, O.max_threads()))
    X, U, J = r["X"].reshape(B, -1), r["U"].reshape(B, -1), r["J"]
    stop = stop_restate(p, N, X, U, W_LEVELS, W_HOLD, 0.5, J, W_WEIGHT)
    g = O.map_geom(*W_GEOM)
    x_first, y_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    mx, my = (x_first - np.arange(g.rows) * g.res)[:, None], (y_first - np.arange(g.cols) * g.res)[None, :]
    c, s = math.cos(W_MAP_POSE[2]), math.sin(W_MAP_POSE[2])
    wx = W_MAP_POSE[0] + c * mx - s * my
    layer = np.where((wx >= W_WALL_X) & (wx < W_WALL_X + 0.5), 100.0, 0.0).astype(np.float32)
    umap = dict(g=g, geom=W_GEOM, layers=layer, poses=W_MAP_POSE)
    pose = np.tile(np.array([W_BOX[0], W_BOX[1], 0.0, 0.0]), (B, 1, N)).reshape(B, 1, 4 * N)
    dim = np.tile(np.array(W_BOX[2:]), (B, 1, N)).reshape(B, 1, 2 * N)
    out = dict(p=p, N=N, B=B, D=D, X=X, U=U, J=J, stop=stop, umap=umap, pose=pose, dim=dim)
    for variant in ("map", "box"):
        kw = dict(threshold=W_THRESHOLD, umap=umap) if variant == "map" else dict(pose=pose, dim=dim)
        out[variant] = dict(solved=restate(p, N, X, 1, base=J, **kw), rows=restate(p, N, stop["X"], D, base=stop["cost"], **kw))
    return out


@pytest.mark.parametrize("variant", ["map", "box"])
def test_scene_w_on_the_restatements(scene_w, variant):
    """Asserted on the restatements alone before any device test uses them: every solved candidate is rejected; the gentlest level
    reaches the wall; the middle level stops clear of it and so does the hardest; the pick is the cheapest candidate's middle level."""
    w, D = scene_w, scene_w["D"]
    v = w[variant]
    assert np.isnan(v["solved"]["total"]).all()                                     # no solved candidate passes
    sp, cost = w["stop"]["sp"].reshape(w["B"], D, 8), w["stop"]["cost"].reshape(w["B"], D)
    assert np.all(sp[:, :, LOST] == 0) and np.all(sp[:, :, STOP_STEP] >= 0) and np.all(sp[:, :, STOP_STEP] <= w["N"] - 1) and np.isfinite(cost).all()
    assert w["stop"]["margin"].min() > DECIDED and sp[:, :, DEVIATION].max() < 0.01
    total = v["rows"]["total"].reshape(w["B"], D)
    print("variant %s: stopping distances %s; totals %s" % (variant, np.round(sp[:, :, DISTANCE], 3).tolist(), total.tolist()))
    assert np.isnan(total[:, 0]).all() and np.isfinite(total[:, 1]).all() and np.isfinite(total[:, 2]).all()
    fp = v["rows"]["fp"].reshape(w["B"], D, 12)
    if variant == "box":
        assert np.all(fp[:, 0, 0] <= -0.5) and np.all(fp[:, 1:, 0] >= 0.5)          # CLEARANCE: decided by half a metre either way
    else:
        assert v["rows"]["edge"] > 1e-9 and v["solved"]["edge"] > 1e-9             # no cell centre on a footprint's edge
        assert np.all(fp[:, 0, 7] >= 3) and np.all(fp[:, 1:, 7] == 0)               # MAP_HIT_STEPS
    masked = np.where(np.isfinite(total), total, np.inf).reshape(-1)
    pick = int(np.argmin(masked))
    assert pick == int(np.argmin(w["J"])) * D + 1 and np.diff(np.sort(masked[np.isfinite(masked)])).min() > 1e-3


@gpu
@pytest.mark.parametrize("variant", ["map", "box"])
def test_composition_on_device_buffers(cilqr, scene_w, variant):
    """cilqr_stop_plans_device -> cilqr_footprint_check_device (S = D, base = cost) -> cilqr_argmin_device on one stream, nothing coming
    back in between: the pick is the pick of the restatements (stop_restate, and the footprint restatement of tests/test_footprint.py)."""
    import torch
    from test_footprint import _Map
    w = scene_w
    N, B, D = w["N"], w["B"], w["D"]
    R = B * D
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    X, U, J, lv, pose, dim = up(w["X"]), up(w["U"]), up(w["J"]), up(np.array(W_LEVELS)), up(w["pose"]), up(w["dim"])
    z = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)  # noqa: E731
    Xs, Us, sp, cost, fp, total, pair = z(R, 4 * (N + 1)), z(R, 2 * N), z(R, 8), z(R), z(R, 12), z(R), z(2)
    sv = cilqr.Solver(cilqr.default_params(N), max_batch=R, max_horizon=N, max_obstacles=1, device=0)
    try:
        torch.cuda.synchronize(dev)
        with _Map(cilqr, sv, w["umap"] if variant == "map" else None):
            sv.stop_plans_device(st, B, N, D, X.data_ptr(), U.data_ptr(), lv.data_ptr(), Xs.data_ptr(), Us.data_ptr(), sp.data_ptr(), hold=W_HOLD,
                                 max_deviation=0.5, plan_cost=J.data_ptr(), decel_weight=W_WEIGHT, cost=cost.data_ptr())
            M = 0 if variant == "map" else 1
            sv.footprint_check_device(st, B, N, M, D, Xs.data_ptr(), pose.data_ptr() if M else 0, dim.data_ptr() if M else 0, (N, N, 1, 0),
                                      fp.data_ptr(), occ_threshold=W_THRESHOLD, base=cost.data_ptr(), total=total.data_ptr())
            sv.argmin_device(st, R, total.data_ptr(), pair.data_ptr())
            torch.cuda.synchronize(dev)
    finally:
        sv.close()
    want = w[variant]["rows"]["total"]
    got, pair = total.cpu().numpy(), pair.cpu().numpy()
    print("totals %s (want %s), pair %s" % (got.tolist(), want.tolist(), pair.tolist()))
    assert _close(got, want)  # (a total is its row's cost: decel_weight * d + J, one rounding near 5e6 at most apart, 9.3e-10)
    masked = np.where(np.isfinite(want), want, np.inf)
    assert int(pair[1]) == int(np.argmin(masked)) and abs(pair[0] - masked.min()) <= ABS_TOL
    assert int(pair[1]) // D == int(np.argmin(w["J"])) and int(pair[1]) % D == 1  # the cheapest candidate, braked at the middle level
    assert _close(Xs.cpu().numpy(), w["stop"]["X"]) and _close(cost.cpu().numpy(), w["stop"]["cost"])


# ---- the facade ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_cpp_facade_stop_fallback(scene_w, tmp_path):
    """tests/cpp/candidates_stop.cpp: run_candidates under iLQR::set_stop_fallback against the C-ABI sequence called by hand, bit for bit
    (inside the program); its pick is the one the restatements give on the oracle's solves without the obstacle in the solve (here: the
    candidate and the level, which the wall decides by metres)."""
    exe = _build(tmp_path, "candidates_stop.cpp", os.path.join(ROOT, "include"), os.path.join(PKG, "host"), lib=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stop fallback ok" in r.stdout
    cand, level = (int(v) for v in re.search(r"stop pick: candidate (\d+) level (\d+)", r.stdout).groups())
    want = int(np.argmin(np.where(np.isfinite(scene_w["box"]["rows"]["total"]), scene_w["box"]["rows"]["total"], np.inf)))
    assert (cand, level) == divmod(want, scene_w["D"])


@gpu
def test_replay_under_the_stop_fallback(tmp_path):
    """bin/cilqr_replay --stop-fallback: a tick with the road blocked 9 m ahead publishes a stop plan at the middle level and ends at rest;
    a tick on a free road publishes the solved plan."""
    exe = os.path.join(PKG, "bin", "cilqr_replay")
    log = tmp_path / "two_ticks.log"
    path = "".join("%d 0\n" % i for i in range(60))
    log.write_text("cilqr-replay 1\nhorizon 40\npath 60\n" + path + "tick\nego 0 0 5 0\nobstacles 1\n%g 0 0 0 0.5 8\ntick\nego 0 0 5 0\nobstacles 0\n" % W_BOX[0])
    r = subprocess.run([exe, str(log), "--stop-fallback", "1.5,3,5:1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2
    first, second = (line.split() for line in lines)
    assert first[-4:] == ["stop", "1", "1", "1"] and second[-4:] == ["stop", "0", "-1", second[-1]]
    X = np.array([float(v) for v in first[first.index("X") + 1:first.index("U")]])
    assert X.size == 4 * 41
    plain = subprocess.run([exe, str(log)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and all("stop" not in line.split() for line in plain.stdout.splitlines())
