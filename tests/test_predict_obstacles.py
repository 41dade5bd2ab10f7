"""Tracked obstacles predicted with covariance (cilqr_predict_obstacles*, include/cilqr.h) and the chance risk that reads it
(cilqr_chance_risk_cov*).

Expected values never come from the HIP path: `predict_restate` below is a numpy restatement of the header's recurrences, and
`restate_cov` is tests/test_chance_risk.py's `restate` (imported: the chain, the lost steps) with the header's covariance term added
to every entry's quadratic form.  Tolerances are the suite's: poses 1e-9 absolute (coordinates within +-100 m), every P_t 1e-9 of its
largest entry, entry_p 1e-9 absolute and 1e-9 relative where the expected p >= 1e-150, step_risk and the probability fields 1e-9; steps,
entries and picks exact where test_chance_risk._decided decides them; everything the header calls a bit copy is compared by bits.
test_conditions asserts, on the restatement alone, what keeps those comparisons from hiding a failure.

  scene T   ego N = 30 at 5 m/s along x, candidates at y = 0, -0.8, -1.6, -2.4, the constant gain of test_chance_risk._straight,
            Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2), no W; ONE oncoming track (30, 4.2, 5, pi, 0, 0), 4 x 2 m,
            P_0 = diag(0.3^2, 0.3^2, 0.5^2, 0.05^2), Q = diag(1e-4, 1e-4, 4e-4, 1e-6).
            CR_STEP_RISK with the predicted covariance 0.1566, 0.0362, 0.0068, 0.00093; without it below 1e-60 for all four.
  scene R   tests/test_rollout_risk.py's (B 8, N 12, M 3) with the oracle's gains: the bit equalities and the further cases.

  scene F   the facade's (tests/cpp/candidates_tracked.cpp): a straight path, candidates at y = 0, 0.3, 0.6, 0.9 m and 5 m/s, one oncoming
            track (30, 3.4, 5, pi, 0, 0) with scene T's P_0 and Q; solved here by the oracle, judged by the restatement: the cheapest
            candidate is the riskiest, and max_risk 0.155 separates it from the next with margins printed by _scene_f.
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import _bits
from test_chance_risk import (MARGIN, MAX_ENTRY, MAX_P, SIGMA0, STEP_RISK, SUM_RISK, TOL, W_DIAG, WORST_STEP, _check_against, _decided,
                              _device_pick, _sym, _total, restate)
from test_rollout_risk import _pick, _scene_r, o_gains

gpu = pytest.mark.gpu

ERR_ARG = -1
ENTRY_POINTS = ("cilqr_predict_obstacles", "cilqr_predict_obstacles_device", "cilqr_chance_risk_cov", "cilqr_chance_risk_cov_device")
_dp = C.POINTER(C.c_double)
P0_T = np.diag([0.3 ** 2, 0.3 ** 2, 0.5 ** 2, 0.05 ** 2])
BRAKING = (0.0, 0.0, 1.0, 0.3, -4.0, 0.2)
HORIZONS = (1, 2, 30, 64, 65)
SETS = ((1, 1), (1, 3), (13, 5))  # (T, M): 1, 3 and 65 tracks


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _cm(m):
    """(4, 4) [r][c] -> (16,) column-major."""
    return np.ascontiguousarray(np.asarray(m, dtype=np.float64).T.reshape(16))


# ---- expected values: numpy restatements of the header's definitions --------------------------------------------------------------
def predict_restate(dt, N, track, cov, Q, T=np.float64):
    """track (..., 6), cov (..., 16) or None, Q (16,) or None -> dict(pose (..., N, 4), sigma (..., N, 4, 4), stop (..., N) bool),
    float64 whatever T.  stop[t]: step t -> t+1 stopped the vehicle."""
    track = np.asarray(track, dtype=np.float64)
    lead = track.shape[:-1]
    tr = track.reshape(-1, 6)
    n = tr.shape[0]
    cv = None if cov is None else np.asarray(cov, dtype=np.float64).reshape(n, 16)
    Qm = np.zeros((4, 4), dtype=T) if Q is None else _sym(Q, T)
    dt = T(dt)
    pose, sig, stops = np.zeros((n, N, 4)), np.zeros((n, N, 4, 4)), np.zeros((n, N), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(n):
            x, y, v, th, a, w = (T(val) for val in tr[k])
            P = np.zeros((4, 4), dtype=T) if cv is None else _sym(cv[k], T)
            for t in range(N):
                pose[k, t] = [x, y, v, th]
                sig[k, t] = P
                stop = bool(v + a * dt < 0)
                stops[k, t] = stop
                at = -v / dt if stop else a
                adv = v * dt + at * dt * dt / 2
                A = np.eye(4, dtype=T)
                A[0, 2], A[1, 2], A[0, 3], A[1, 3] = dt * np.cos(th), dt * np.sin(th), -np.sin(th) * adv, np.cos(th) * adv
                x, y = x + np.cos(th) * adv, y + np.sin(th) * adv
                v = T(0) if stop else v + a * dt
                th = th + w * dt
                P2 = A @ P @ A.T + Qm
                P = np.triu(P2) + np.triu(P2, 1).T
    return dict(pose=pose.reshape(lead + (N, 4)), sigma=sig.reshape(lead + (N, 4, 4)), stop=stops.reshape(lead + (N,)))


def restate_cov(p, N, X, U, K, sigma0, W, pose, dim, cov, T=np.float64):
    """test_chance_risk.restate with the obstacle's covariance: cov (B, M, N, 3) = (xx, xy, yy) or None.  restate supplies the chain and
    the lost steps; the entries are formed again from its Sigma_t with q' = g'Sigma g + gx^2 Cxx + 2 gx gy Cxy + gy^2 Cyy; an entry whose
    covariance is not finite has p = 1.  Without cov the entries must reproduce restate's (asserted)."""
    import math
    base = restate(p, N, X, U, K, sigma0, W, pose, dim, T)
    B, M = base["B"], base["M"]
    if M == 0:
        return base
    Xs = X.reshape(B, N + 1, 4).astype(T)
    # Sigma_t in the working precision: restate returns it rounded to float64, so the longdouble run forms it again
    sig = base["sigma"].reshape(B, N + 1, 16).reshape(B, N + 1, 4, 4).swapaxes(-1, -2) if T is np.float64 else _sigma_chain(p, N, X, U, K, sigma0, W, T)
    pp = np.zeros((B, M, N, 2))
    root2 = np.sqrt(T(2))
    cv = np.zeros((B, M, N, 3), dtype=T) if cov is None else np.asarray(cov).reshape(B, M, N, 3).astype(T)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            x, y, th = Xs[b, :N, 0], Xs[b, :N, 1], Xs[b, :N, 3]
            S = sig[b, :N]
            for m in range(M):
                po, di = pose[b, m].reshape(N, 4).astype(T), dim[b, m].reshape(N, 2).astype(T)
                co, so = np.cos(po[:, 3]), np.sin(po[:, 3])
                ea = di[:, 0] / 2 + np.abs(po[:, 2] * co) * T(p.t_safe) + T(p.s_safe_a) + T(p.ego_rad)
                eb = di[:, 1] / 2 + np.abs(po[:, 2] * so) * T(p.t_safe) + T(p.s_safe_b) + T(p.ego_rad) + 1
                for side, lever in ((0, T(p.ego_front)), (1, -T(p.ego_rear))):
                    ex, ey = x + lever * np.cos(th) - po[:, 0], y + lever * np.sin(th) - po[:, 1]
                    d0, d1 = co * ex + so * ey, co * ey - so * ex
                    c = 1 - (d0 * d0 / ea / ea + d1 * d1 / eb / eb)
                    p0, p1 = d0 / ea / ea, d1 / eb / eb
                    gx, gy = -2 * (co * p0 - so * p1), -2 * (so * p0 + co * p1)
                    gt = gx * (-lever * np.sin(th)) + gy * (lever * np.cos(th))
                    q = (gx * gx * S[:, 0, 0] + gy * gy * S[:, 1, 1] + gt * gt * S[:, 3, 3]
                         + 2 * (gx * gy * S[:, 0, 1] + gx * gt * S[:, 0, 3] + gy * gt * S[:, 1, 3]))
                    q = q + (gx * gx * cv[b, m, :, 0] + 2 * gx * gy * cv[b, m, :, 1] + gy * gy * cv[b, m, :, 2])
                    s = np.sqrt(np.fmax(q, 0))
                    for t in range(N):
                        if not np.all(np.isfinite(cv[b, m, t].astype(np.float64))):
                            pp[b, m, t, side] = 1.0
                        elif s[t] > 0:
                            z = float(-c[t] / (s[t] * root2))
                            pp[b, m, t, side] = z if math.isnan(z) else 0.5 * math.erfc(z)
                        else:
                            pp[b, m, t, side] = 1.0 if c[t] > 0 else 0.0
        entry_p = np.fmax(pp[..., 0], pp[..., 1]).reshape(B, M * N)
        if cov is None and T is np.float64:
            assert np.array_equal(_bits(entry_p), _bits(base["entry_p"]))  # the same statements as restate's
        lost = ~(np.isfinite(X.reshape(B, N + 1, 4)[:, :N]).all(axis=2) & np.isfinite(U.reshape(B, N, 2)).all(axis=2)
                 & np.isfinite(K.reshape(B, N, 8)).all(axis=2) & np.isfinite(base["sigma"].reshape(B, N + 1, 16)[:, :N]).all(axis=2))
        step_risk = np.where(lost, 1.0, np.fmin(1.0, entry_p.reshape(B, M, N).sum(axis=1)))
        out = dict(base)
        risk = base["risk"].copy()
        risk[:, STEP_RISK] = step_risk.max(axis=1)
        risk[:, WORST_STEP] = step_risk.argmax(axis=1)
        risk[:, SUM_RISK] = np.minimum(1.0, step_risk.sum(axis=1))
        e = np.where(np.isnan(entry_p), -np.inf, entry_p)
        risk[:, MAX_P], risk[:, MAX_ENTRY] = e.max(axis=1), e.argmax(axis=1)
        out.update(entry_p=entry_p, step_risk=step_risk, risk=risk)
    return out


def _sigma_chain(p, N, X, U, K, sigma0, W, T):
    """restate's covariance chain in precision T (restate returns it rounded to float64)."""
    B = X.shape[0]
    Xs, Us, Ks = X.reshape(B, N + 1, 4).astype(T), U.reshape(B, N, 2).astype(T), K.reshape(B, N, 4, 2).astype(T)
    dt = T(p.timestep)
    s0 = np.broadcast_to(np.asarray(sigma0).reshape(-1, 16), (B, 16))
    Wm = np.zeros((4, 4), dtype=T) if W is None else _sym(W, T)
    sig = np.zeros((B, N + 1, 4, 4), dtype=T)
    for b in range(B):
        S = _sym(s0[b], T)
        sig[b, 0] = S
        for t in range(N):
            v, th, a = Xs[b, t, 2], Xs[b, t, 3], Us[b, t, 0]
            adv = v * dt + a * dt * dt / 2
            A, Bm = np.eye(4, dtype=T), np.zeros((4, 2), dtype=T)
            A[0, 2], A[1, 2], A[0, 3], A[1, 3] = dt * np.cos(th), dt * np.sin(th), -np.sin(th) * adv, np.cos(th) * adv
            Bm[0, 0], Bm[1, 0], Bm[2, 0], Bm[3, 1] = dt * dt * np.cos(th) / 2, dt * dt * np.sin(th) / 2, dt, dt
            F = A + Bm @ Ks[b, t].T
            S2 = F @ S @ F.T + Wm
            S = np.triu(S2) + np.triu(S2, 1).T
            sig[b, t + 1] = S
    return sig


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _tracks(T, M, seed):
    """T x M tracks within +-100 m over 65 steps: speeds 0 ... 12 m/s, accelerations -3 ... 2 (some brake to a stop), yaw rates
    +-0.3; a full P_0 per track (a random factor times its transpose) with NaN below the diagonal; dimensions 3 ... 6 x 1.5 ... 2.5."""
    rng = np.random.Generator(np.random.PCG64(seed))
    tr = np.zeros((T, M, 6))
    tr[..., 0], tr[..., 1] = rng.uniform(-20, 20, (T, M)), rng.uniform(-20, 20, (T, M))
    tr[..., 2], tr[..., 3] = rng.uniform(0, 12, (T, M)), rng.uniform(-3.1, 3.1, (T, M))
    tr[..., 4], tr[..., 5] = rng.uniform(-3, 2, (T, M)), rng.uniform(-0.3, 0.3, (T, M))
    dim = np.stack([rng.uniform(3, 6, (T, M)), rng.uniform(1.5, 2.5, (T, M))], axis=-1)
    cov = np.zeros((T, M, 16))
    for t in range(T):
        for m in range(M):
            L = rng.normal(size=(4, 4)) * [0.3, 0.3, 0.5, 0.05]
            P = L.T @ L
            P[np.tril_indices(4, -1)] = np.nan
            cov[t, m] = _cm(P)
    return tr, dim, cov


def _noise(nan_below=True):
    Q = W_DIAG.copy()
    Q[0, 1] = 2e-5
    if nan_below:
        Q[np.tril_indices(4, -1)] = np.nan
    return _cm(Q)


def _scene_t(p):
    """The plans, the gain and the track of scene T; p = the oracle's parameters at N = 30."""
    N, ys = 30, (0.0, -0.8, -1.6, -2.4)
    B = len(ys)
    X, U, K = np.zeros((B, N + 1, 4)), np.zeros((B, N, 2)), np.zeros((B, N, 4, 2))
    X[:, :, 0], X[:, :, 2] = 5.0 * p.timestep * np.arange(N + 1), 5.0
    for b, y in enumerate(ys):
        X[b, :, 1] = y
    K[:, :, 2, 0] = -1.0
    K[:, :, 1, 1], K[:, :, 3, 1] = -0.5, -1.5
    track = np.array([[30.0, 4.2, 5.0, np.pi, 0.0, 0.0]])
    return dict(p=p, B=B, N=N, M=1, X=X.reshape(B, -1), U=U.reshape(B, -1), K=K.reshape(B, -1), track=track, track_dim=np.array([[4.0, 2.0]]),
                track_cov=_cm(P0_T)[None], Q=_cm(W_DIAG), sigma0=_cm(SIGMA0), base=np.array([1.0, 2.0, 3.0, 4.0]))


def _scene_t_want(s, T=np.float64):
    """Scene T's expected values: the restated prediction, then the restated judge with and without its covariance."""
    B, N = s["B"], s["N"]
    pr = predict_restate(s["p"].timestep, N, s["track"], s["track_cov"], s["Q"], T)
    pose = np.ascontiguousarray(np.broadcast_to(pr["pose"].reshape(1, 1, 4 * N), (B, 1, 4 * N)))
    dim = np.ascontiguousarray(np.broadcast_to(np.tile(s["track_dim"], N).reshape(1, 1, 2 * N), (B, 1, 2 * N)))
    c3 = np.stack([pr["sigma"][0, :, 0, 0], pr["sigma"][0, :, 0, 1], pr["sigma"][0, :, 1, 1]], axis=-1)
    cov = np.ascontiguousarray(np.broadcast_to(c3[None, None], (B, 1, N, 3)))
    with_cov = restate_cov(s["p"], N, s["X"], s["U"], s["K"], s["sigma0"], None, pose, dim, cov, T)
    without = restate_cov(s["p"], N, s["X"], s["U"], s["K"], s["sigma0"], None, pose, dim, None, T)
    return dict(pred=pr, pose=pose, dim=dim, cov=cov, with_cov=with_cov, without=without)


@pytest.fixture(scope="module")
def cases(oracle):
    """Scene T and scene R with every expected value.  Computed once; never modified."""
    O = oracle
    t = _scene_t(O.default_params(30))
    r = _scene_r(O)
    r["pose"], r["dim"] = np.ascontiguousarray(r["pose"]).reshape(r["B"], r["M"], -1), np.ascontiguousarray(r["dim"]).reshape(r["B"], r["M"], -1)
    _, r["K"], ok = o_gains(O, r["p"], r["N"], r["X"], r["U"], r["poly"], r["fl"], r["pose"], r["dim"], None, 1.0)
    assert np.all(ok == 1)
    rng = np.random.Generator(np.random.PCG64(11))
    B, M, N = r["B"], r["M"], r["N"]
    rcov = np.zeros((B, M, N, 3))
    grow = 1.0 + 0.2 * np.arange(N)
    rcov[..., 0] = rng.uniform(0.02, 0.1, (B, M, 1)) * grow
    rcov[..., 2] = rng.uniform(0.02, 0.1, (B, M, 1)) * grow
    rcov[..., 1] = 0.4 * np.sqrt(rcov[..., 0] * rcov[..., 2])
    s0 = _cm(SIGMA0)
    out = {"T": t, "T_want": _scene_t_want(t), "R": r, "R_cov": rcov, "sigma0": s0,
           "R_want": restate_cov(r["p"], N, r["X"], r["U"], r["K"], s0, _cm(W_DIAG), r["pose"], r["dim"], rcov)}
    return out


F_MAX_RISK, F_MARGIN = 0.155, 1e-3  # scene F: the bound, and how far every candidate's CR_STEP_RISK must stay from it


def _scene_f(O):
    """Scene F on the CPU: the oracle's local plans, solves and gains, the restated prediction and judge.  Returns dict(J, with_cov,
    without (CR_STEP_RISK per candidate), pick_off, pick_on)."""
    N, B = 30, 4
    p = O.default_params(N)
    path = np.stack([np.arange(200.0), np.zeros(200)], 1)
    x0 = np.array([[0.0, 0.3 * b, 5.0, 0.0] for b in range(B)])
    poly, fl = np.zeros((B, 6)), np.zeros((B, 2))
    for b in range(B):
        poly[b], ref = O.local_plan(p, path, x0[b])
        fl[b] = (ref[0, 0], ref[-1, 0])
    track, Q = np.array([[30.0, 3.4, 5.0, np.pi, 0.0, 0.0]]), _cm(W_DIAG)
    pr = predict_restate(p.timestep, N, track, _cm(P0_T)[None], Q)
    pose = np.ascontiguousarray(np.broadcast_to(pr["pose"].reshape(1, 1, 4 * N), (B, 1, 4 * N)))
    dim = np.ascontiguousarray(np.broadcast_to(np.tile([4.0, 2.0], N).reshape(1, 1, 2 * N), (B, 1, 2 * N)))
    c3 = np.stack([pr["sigma"][0, :, 0, 0], pr["sigma"][0, :, 0, 1], pr["sigma"][0, :, 1, 1]], axis=-1)
    cov = np.ascontiguousarray(np.broadcast_to(c3[None, None], (B, 1, N, 3)))
    r = O.solve_batch(p, N, 1, x0, np.tile(O.default_control_seq(N), (B, 1)), poly, fl, pose, dim)
    _, K, ok = o_gains(O, p, N, r["X"], r["U"], poly, fl, pose, dim, None, 1.0)
    assert np.all(ok == 1)
    s0 = _cm(SIGMA0)
    a = restate_cov(p, N, r["X"], r["U"], K, s0, Q, pose, dim, cov)
    bare = restate_cov(p, N, r["X"], r["U"], K, s0, Q, pose, dim, None)
    out = dict(J=r["J"], with_cov=a["risk"][:, STEP_RISK], without=bare["risk"][:, STEP_RISK],
               pick_on=_pick(_total(a["risk"], r["J"], F_MAX_RISK)), pick_off=_pick(_total(bare["risk"], r["J"], F_MAX_RISK)))
    print("scene F (oracle solves, restated judge): J %s\n  CR_STEP_RISK with the covariance %s, margins to %g: %s\n  without %s; picks off %d, on %d"
          % (out["J"].tolist(), out["with_cov"].tolist(), F_MAX_RISK, (out["with_cov"] - F_MAX_RISK).tolist(), out["without"].tolist(),
             out["pick_off"], out["pick_on"]))
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_the_facade_scene_separates_its_candidates(oracle):
    """Scene F on the CPU alone: the cheapest candidate is the one the covariance rejects, every CR_STEP_RISK is at least 1e-3 from the
    bound (the device's solves agree with the oracle's to 1e-6 in U: a thousandth of that margin), and the pick moves."""
    f = _scene_f(oracle)
    assert int(np.argmin(f["J"])) == 0 and np.min(np.diff(np.sort(f["J"]))) > F_MARGIN
    assert np.min(np.abs(f["with_cov"] - F_MAX_RISK)) > F_MARGIN and np.all(f["without"] < 1e-30)
    assert f["with_cov"][0] > F_MAX_RISK > f["with_cov"][1]
    assert (f["pick_off"], f["pick_on"]) == (0, 1)
    header = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_tracked_obstacles\s*\(", header) and re.search(r"void\s+set_obstacle_covariance_check\s*\(\s*bool\s+on\s*\)", header)


def test_header_library_and_binding_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    for name in ("predict_obstacles", "predict_obstacles_device", "chance_risk_cov", "chance_risk_cov_device"):
        assert callable(getattr(cilqr.Solver, name)), name
    assert "8*18*N bytes" in full  # the LDS formula is stated
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_predict_obstacles\s*\(", plan) and re.search(r"inline\s+void\s+plan_chance_risk_cov\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_predict.hip" in mk and re.search(r"^check:.*build/cilqr_predict\.o", mk, flags=re.M)


def test_argument_errors_need_no_device(cilqr):
    """NULL track, track_dim, pose_out or dim_out and T, N or M < 1: CILQR_ERR_ARG before the handle is looked at (there is none
    here); valid arguments then meet the null handle.  cilqr_chance_risk_cov: the errors of cilqr_chance_risk."""
    L = cilqr.lib()
    T, N, M = 2, 4, 3
    tr, dm, cv, Q = np.zeros((T, M, 6)), np.ones((T, M, 2)), np.zeros((T, M, 16)), np.zeros(16)
    pose, dim, cov, sig = np.zeros((T, M, 4 * N)), np.zeros((T, M, 2 * N)), np.zeros((T, M, N, 3)), np.zeros((T, M, N, 16))
    no_handle = C.c_void_p()

    def call(dev, T_=T, N_=N, M_=M, **nulls):
        a = dict(track=tr, track_dim=dm, pose_out=pose, dim_out=dim)
        a.update(nulls)
        f = L.cilqr_predict_obstacles_device if dev else L.cilqr_predict_obstacles
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, T_, N_, M_, _p(a["track"]), _p(a["track_dim"]), _p(cv), _p(Q), _p(a["pose_out"]), _p(a["dim_out"]), _p(cov), _p(sig))

    for dev in (False, True):
        for name in ("track", "track_dim", "pose_out", "dim_out"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        for kw in (dict(T_=0), dict(N_=0), dict(M_=0), dict(T_=-1)):
            assert call(dev, **kw) == ERR_ARG and b"at least 1" in L.cilqr_last_error(), kw
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
    B = 2
    X, U, K, s0 = np.zeros((B, 4 * (N + 1))), np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros(16)
    opose, odim, ocov = np.zeros((B, 1, 4 * N)), np.ones((B, 1, 2 * N)), np.zeros((B, 1, N, 3))
    risk = np.zeros((B, 6))
    o = cilqr.Obstacles(opose.ctypes.data, odim.ctypes.data, None, N, N, 1, 0)
    for dev in (False, True):
        f = L.cilqr_chance_risk_cov_device if dev else L.cilqr_chance_risk_cov
        head = (no_handle, None) if dev else (no_handle,)

        def judge(X_=X, obs=o, mr=1.0, flags=0):
            return f(*head, B, N, 1, _p(X_), _p(U), _p(K), _p(s0), C.c_int64(0), None, C.byref(obs) if obs else None, _p(ocov),
                     C.c_uint32(flags), C.c_double(mr), None, _p(risk), None, None, None, None)

        assert judge(X_=None) == ERR_ARG and b"null required pointer" in L.cilqr_last_error()
        assert judge(obs=None) == ERR_ARG and b"obs is null" in L.cilqr_last_error()
        assert judge(mr=float("nan")) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert judge(flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert judge() == ERR_ARG and b"null handle" in L.cilqr_last_error()


def _agree(a, b, what):
    dp = float(np.max(np.abs(a["entry_p"] - b["entry_p"])))
    big = b["entry_p"] >= 1e-150
    drel = float(np.max(np.abs(a["entry_p"] - b["entry_p"])[big] / b["entry_p"][big])) if big.any() else 0.0
    dr = float(np.max(np.abs(a["step_risk"] - b["step_risk"])))
    f = [STEP_RISK, SUM_RISK, MAX_P]
    df = float(np.max(np.abs(a["risk"][:, f] - b["risk"][:, f])))
    print("%s, float64 vs longdouble: entry_p %.3g abs %.3g rel, step_risk %.3g, fields %.3g" % (what, dp, drel, dr, df))
    assert max(dp, drel, dr, df) <= 1e-11, what


def test_conditions(oracle, cases):
    """What keeps the GPU comparisons from hiding a failure, on the restatements' numbers alone."""
    assert np.longdouble(1) + np.finfo(np.longdouble).eps != 1 and np.finfo(np.longdouble).eps < 1e-18  # longdouble is wider here
    p = cases["T"]["p"]
    dt = p.timestep
    # the prediction: float64 against longdouble, in the measures of the GPU comparisons, on every case used below
    Q = _noise()
    for T, M in SETS:
        tr, _, cov = _tracks(T, M, 100 + T * M)
        for N in HORIZONS:
            a, b = predict_restate(dt, N, tr, cov, Q), predict_restate(dt, N, tr, cov, Q, np.longdouble)
            dpose = float(np.max(np.abs(a["pose"] - b["pose"])))
            scale = np.max(np.abs(b["sigma"]), axis=(-1, -2), keepdims=True)
            dsig = float(np.max(np.abs(a["sigma"] - b["sigma"]) / scale))
            assert dpose <= 1e-11 and dsig <= 1e-11, (T, M, N, dpose, dsig)
            assert np.max(np.abs(b["pose"][..., :2])) < 100.0 and np.array_equal(a["stop"], b["stop"])
            if N == 65 and T * M == 65:
                print("65 tracks, N 65: float64 vs longdouble pose %.3g, P_t %.3g (scaled); %d tracks stop" % (dpose, dsig, int(a["stop"].any(axis=-1).sum())))
                assert a["stop"].any() and not a["stop"].any(axis=-1).all()
                # every stop decision is decided: v_t + a*dt is at least MARGIN from 0 wherever it is taken
                v, acc = b["pose"][..., 2], tr[..., 4][..., None]
                assert np.min(np.abs(v + acc * dt)[v > 0]) > MARGIN
    # the braking case really reaches `stop`, with its decisions decided
    br = predict_restate(dt, 8, np.array(BRAKING), None, None)
    assert br["stop"].tolist() == [False, False, True] + [True] * 5  # (a stopped vehicle with a < 0 "stops" again: v stays 0)
    assert np.allclose(br["pose"][:4, 2], [1.0, 0.6, 0.2, 0.0], atol=1e-15) and np.all(br["pose"][3:, 2] == 0.0)
    assert np.min(np.abs(br["pose"][:, 2] + BRAKING[4] * dt)) > MARGIN
    assert np.array_equal(br["pose"][3:, :2], np.broadcast_to(br["pose"][3, :2], (5, 2))) and np.all(np.diff(br["pose"][:, 3]) > 0.019)
    # scene T: the figures of the issue, float64 against longdouble, thresholds and the pick
    s, w = cases["T"], cases["T_want"]
    wl = _scene_t_want(s, np.longdouble)
    _agree(w["with_cov"], wl["with_cov"], "scene T with the predicted covariance")
    _agree(w["without"], wl["without"], "scene T without it")
    step, bare = w["with_cov"]["risk"][:, STEP_RISK], w["without"]["risk"][:, STEP_RISK]
    print("scene T: CR_STEP_RISK with the predicted covariance %s, without %s" % (step.tolist(), bare.tolist()))
    assert np.all(np.abs(step - [0.1566, 0.0362, 0.0068, 0.00093]) <= [5e-5, 5e-5, 5e-5, 5e-6]) and np.all(bare < 1e-60)
    assert np.min(np.abs(step - 0.05)) > MARGIN
    assert _pick(_total(w["with_cov"]["risk"], s["base"], 0.05)) == 1 and _pick(_total(w["without"]["risk"], s["base"], 0.05)) == 0
    gs, ge = _decided(w["with_cov"])
    assert gs.min() > MARGIN and ge.min() > MARGIN
    # scene R with a covariance: it matters, float64 against longdouble, every solve decided
    r = cases["R"]
    rw = cases["R_want"]
    rl = restate_cov(r["p"], r["N"], r["X"], r["U"], r["K"], cases["sigma0"], _cm(W_DIAG), r["pose"], r["dim"], cases["R_cov"], np.longdouble)
    _agree(rw, rl, "scene R with a covariance")
    bare = restate_cov(r["p"], r["N"], r["X"], r["U"], r["K"], cases["sigma0"], _cm(W_DIAG), r["pose"], r["dim"], None)
    assert np.min(np.abs(rw["risk"][:, STEP_RISK] - bare["risk"][:, STEP_RISK])) > MARGIN
    gs, ge = _decided(rw)
    print("scene R with a covariance: smallest r_t gap %.3g, smallest entry_p gap %.3g; STEP_RISK %s" % (gs.min(), ge.min(), np.round(rw["risk"][:, STEP_RISK], 5).tolist()))
    assert gs.min() > MARGIN and ge.min() > MARGIN


def test_the_host_forms_fit_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_predict.cpp: plan_predict_obstacles and plan_chance_risk_cov laid out without an arena against
    host_arena_bytes at the shapes include/cilqr.h says always fit; host_arena_bytes is still what tests/golden/host_arena_cap.json
    recorded."""
    exe = str(tmp_path / "host_plan_predict")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_predict.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1200:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "14 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


# ---- GPU: predict ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=104, max_horizon=80, max_obstacles=5, device=0)
    yield s
    s.close()


PRED_OUT = ("pose", "dim", "cov", "sigma")


def _predict(solver, N, track, dim, cov=None, Q=None, skip=(), keep=False):
    """The device form on torch buffers.  track (T, M, 6).  Returns dict(pose (T, M, N, 4), dim (T, M, N, 2), cov (T, M, N, 3), sigma
    (T, M, N, 16)), None where skipped; with keep=True the device tensors instead."""
    import torch
    T, M = track.shape[:2]
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    ttr, tdm, tcv, tq = up(track), up(dim), up(cov), up(Q)
    z = lambda *shape: torch.full(shape, -123.456, dtype=torch.float64, device=dev)  # noqa: E731
    out = dict(pose=z(T, M, N, 4), dim=z(T, M, N, 2), cov=z(T, M, N, 3), sigma=z(T, M, N, 16))
    for n in skip:
        out[n] = None
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    torch.cuda.synchronize(dev)
    solver.predict_obstacles_device(torch.cuda.current_stream(dev).cuda_stream, T, N, M, ttr.data_ptr(), tdm.data_ptr(), out["pose"].data_ptr(),
                                    out["dim"].data_ptr(), track_cov=ptr(tcv), track_noise=ptr(tq), cov_out=ptr(out["cov"]),
                                    sigma_out=ptr(out["sigma"]))
    torch.cuda.synchronize(dev)
    if keep:
        return out
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _same(a, b, sel_a=slice(None), sel_b=slice(None), names=PRED_OUT):
    return all(np.array_equal(_bits(a[n][sel_a]), _bits(b[n][sel_b])) for n in names)


def _check_prediction(got, want, track, dim, cov, what):
    pose, sig = got["pose"], got["sigma"].reshape(got["sigma"].shape[:3] + (4, 4)).swapaxes(-1, -2)  # column-major -> [r][c]
    assert all(np.all(got[n] != -123.456) for n in PRED_OUT), what  # everything was written
    dpose = float(np.max(np.abs(pose - want["pose"])))
    scale = np.max(np.abs(want["sigma"]), axis=(-1, -2), keepdims=True)
    dsig = float(np.max(np.abs(sig - want["sigma"]) / np.where(scale > 0, scale, 1.0)))
    print("%s: pose max |d| %.3g, P_t %.3g of its largest entry" % (what, dpose, dsig))
    assert dpose <= TOL and dsig <= TOL, what
    assert np.array_equal(_bits(sig), _bits(sig.swapaxes(-1, -2))), what  # exactly symmetric
    assert np.array_equal(_bits(got["cov"]), _bits(got["sigma"][..., [0, 4, 5]])), what  # (0,0), (0,1), (1,1)
    assert np.array_equal(_bits(got["dim"]), _bits(np.broadcast_to(dim[:, :, None, :], got["dim"].shape))), what
    assert np.array_equal(_bits(pose[:, :, 0]), _bits(track[..., :4])), what  # entry 0: the tracked state
    p0 = np.zeros(track.shape[:2] + (4, 4)) if cov is None else np.stack([np.stack([_sym(c, np.float64) for c in row]) for row in cov])
    assert np.array_equal(_bits(sig[:, :, 0]), _bits(p0)), what  # P_0 mirrored from its upper triangle


@gpu
@pytest.mark.parametrize("N", HORIZONS)
def test_predicted_values(cilqr, solver, cases, N):
    """1, 3 and 65 tracks at every horizon: poses, every P_t, symmetry, the bit copies; a set alone (T = 1) has the bits it has among 13."""
    dt = cases["T"]["p"].timestep
    Q = _noise()
    for T, M in SETS:
        tr, dim, cov = _tracks(T, M, 100 + T * M)
        got = _predict(solver, N, tr, dim, cov, Q)
        _check_prediction(got, predict_restate(dt, N, tr, cov, Q), tr, dim, cov, "T %d, M %d, N %d" % (T, M, N))
        if T > 1:
            for t in (0, T - 1):
                one = _predict(solver, N, tr[t:t + 1], dim[t:t + 1], cov[t:t + 1], Q)
                assert _same(one, got, sel_b=slice(t, t + 1)), t


@gpu
def test_optional_arguments_and_constant_velocity(cilqr, solver, cases):
    """NULL track_cov and NULL track_noise are zeros; only row <= column of either is read; each optional output left out leaves the
    others' bits; a = omega = 0 keeps v and theta bit-constant."""
    dt, N = cases["T"]["p"].timestep, 30
    tr, dim, cov = _tracks(1, 3, 5)
    full = _predict(solver, N, tr, dim, cov, _noise())
    clean_cov = np.stack([[_cm(_sym(c, np.float64)) for c in row] for row in cov])
    assert np.isnan(cov).any() and np.isnan(_noise()).any() and not np.isnan(clean_cov).any()
    assert _same(_predict(solver, N, tr, dim, clean_cov, _noise(nan_below=False)), full)
    none = _predict(solver, N, tr, dim, None, None)
    _check_prediction(none, predict_restate(dt, N, tr, None, None), tr, dim, None, "no covariance, no noise")
    assert not none["sigma"].any() and _same(_predict(solver, N, tr, dim, np.zeros((1, 3, 16)), np.zeros(16)), none)
    _check_prediction(_predict(solver, N, tr, dim, None, _noise()), predict_restate(dt, N, tr, None, _noise()), tr, dim, None, "noise alone")
    _check_prediction(_predict(solver, N, tr, dim, cov, None), predict_restate(dt, N, tr, cov, None), tr, dim, cov, "covariance alone")
    for n in ("cov", "sigma"):
        part = _predict(solver, N, tr, dim, cov, _noise(), skip=(n,))
        assert part[n] is None and _same(part, full, names=[m for m in PRED_OUT if m != n]), n
    part = _predict(solver, N, tr, dim, cov, _noise(), skip=("cov", "sigma"))
    assert _same(part, full, names=("pose", "dim"))
    steady = tr.copy()
    steady[..., 4:] = 0.0
    got = _predict(solver, 65, steady, dim, cov, _noise())
    assert np.array_equal(_bits(got["pose"][..., 2:]), _bits(np.broadcast_to(steady[:, :, None, 2:4], got["pose"][..., 2:].shape)))
    _check_prediction(got, predict_restate(dt, 65, steady, cov, _noise()), steady, dim, cov, "constant velocity")


@gpu
def test_a_braking_vehicle_stops(cilqr, solver, cases):
    """(0, 0, 1.0, 0.3, -4.0, 0.2): v goes 1, 0.6, 0.2, 0, 0, ...; the position stands still from step 3; theta keeps turning; the
    covariance keeps growing after the stop."""
    dt, N = cases["T"]["p"].timestep, 8
    tr, dim = np.array(BRAKING).reshape(1, 1, 6), np.array([[[4.0, 2.0]]])
    cov = _cm(P0_T).reshape(1, 1, 16)
    got = _predict(solver, N, tr, dim, cov, _noise())
    _check_prediction(got, predict_restate(dt, N, tr, cov, _noise()), tr, dim, cov, "braking")
    pose = got["pose"][0, 0]
    assert np.all(np.abs(pose[:4, 2] - [1.0, 0.6, 0.2, 0.0]) <= 1e-15) and np.all(pose[3:, 2] == 0.0)
    assert np.array_equal(_bits(pose[3:, :2]), _bits(np.broadcast_to(pose[3, :2], (5, 2)))) and np.hypot(*pose[3, :2]) > 0.1
    assert np.all(np.abs(np.diff(pose[:, 3]) - 0.2 * dt) <= 1e-15)
    assert np.all(np.diff(got["cov"][0, 0, :, 0]) > 0) and np.all(np.diff(got["cov"][0, 0, :, 2]) > 0)


@gpu
def test_a_track_depends_on_itself_alone(cilqr, solver, cases):
    """A NaN in one track changes no bit of the others; each track alone and the batch reversed give the batch's bits; the host form
    equals the device form bit for bit, through ctypes and through the binding."""
    N = 30
    T, M = 13, 5
    tr, dim, cov = _tracks(T, M, 165)
    Q = _noise()
    whole = _predict(solver, N, tr, dim, cov, Q)
    flat = lambda a: a.reshape((T * M, 1) + a.shape[2:])  # noqa: E731
    single = _predict(solver, N, flat(tr), flat(dim), flat(cov), Q)  # 65 sets of one track
    assert all(np.array_equal(_bits(single[n].reshape(whole[n].shape)), _bits(whole[n])) for n in PRED_OUT)
    for k in (0, 37, 64):
        one = _predict(solver, N, flat(tr)[k:k + 1], flat(dim)[k:k + 1], flat(cov)[k:k + 1], Q)
        assert all(np.array_equal(_bits(one[n][0, 0]), _bits(whole[n].reshape((T * M,) + whole[n].shape[2:])[k])) for n in PRED_OUT), k
    rev = _predict(solver, N, tr[::-1, ::-1], dim[::-1, ::-1], cov[::-1, ::-1], Q)
    assert _same(rev, whole, sel_b=(slice(None, None, -1), slice(None, None, -1)))
    for col, what in ((1, "y"), (4, "a")):
        bad = tr.copy()
        bad[6, 2, col] = np.nan
        got = _predict(solver, N, bad, dim, cov, Q)
        keep = np.ones((T, M), dtype=bool)
        keep[6, 2] = False
        assert all(np.array_equal(_bits(got[n][keep]), _bits(whole[n][keep])) for n in PRED_OUT), what
        assert np.isnan(got["pose"][6, 2, 1:]).any(), what
    badcov = cov.copy()
    badcov[3, 1, 0] = np.nan
    got = _predict(solver, N, tr, dim, badcov, Q)
    keep = np.ones((T, M), dtype=bool)
    keep[3, 1] = False
    assert all(np.array_equal(_bits(got[n][keep]), _bits(whole[n][keep])) for n in PRED_OUT)
    assert np.isnan(got["sigma"][3, 1]).any() and np.array_equal(_bits(got["pose"][3, 1]), _bits(whole["pose"][3, 1]))
    # host forms
    host = dict(pose=np.full((T, M, N, 4), -1.5), dim=np.full((T, M, N, 2), -1.5), cov=np.full((T, M, N, 3), -1.5), sigma=np.full((T, M, N, 16), -1.5))
    cilqr._check(cilqr.lib().cilqr_predict_obstacles(solver._h, T, N, M, _p(tr), _p(dim), _p(cov), _p(Q), _p(host["pose"]), _p(host["dim"]),
                                                     _p(host["cov"]), _p(host["sigma"])))
    assert _same(host, whole)
    via = solver.predict_obstacles(N, tr, dim, cov, Q)
    assert via["pose"].shape == (T, M, 4 * N) and via["cov"].shape == (T, M, 3 * N) and via["sigma"].shape == (T, M, N, 16)
    assert all(np.array_equal(_bits(via[n].reshape(whole[n].shape)), _bits(whole[n])) for n in PRED_OUT)
    lean = solver.predict_obstacles(N, tr[0], dim[0], want_cov=False, want_sigma=False)
    assert lean["pose"].shape == (M, 4 * N) and lean["cov"] is None and lean["sigma"] is None
    assert np.array_equal(_bits(lean["pose"].reshape(M, N, 4)), _bits(_predict(solver, N, tr[:1], dim[:1])["pose"][0]))


@gpu
def test_limits(cilqr, solver):
    """T, N, M beyond the create limits and a host call beyond the arena are CILQR_ERR_ARG; the handle stays usable."""
    tr, dim, cov = _tracks(1, 2, 3)
    ok = solver.predict_obstacles(4, tr[0], dim[0], cov[0])
    for T, N, M, what in ((105, 4, 1, "T="), (1, 81, 1, "N="), (1, 4, 6, "M=")):
        t, d, _ = _tracks(T, M, 1)
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: %s" % (ERR_ARG, what)):
            solver.predict_obstacles(N, t, d)
    t, d, c = _tracks(104, 5, 1)
    with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers reserved at create" % ERR_ARG):
        solver.predict_obstacles(80, t, d, c)  # T = max_batch with every output: beyond the arena
    small = solver.predict_obstacles(80, t[:13], d[:13], c[:13])  # T = max_batch / 8: fits
    assert np.all(np.isfinite(small["pose"]))
    again = solver.predict_obstacles(4, tr[0], dim[0], cov[0])
    assert all(np.array_equal(_bits(again[n]), _bits(ok[n])) for n in PRED_OUT)


# ---- GPU: judge --------------------------------------------------------------------------------------------------------------
JUDGE_OUT = ("risk", "step_risk", "entry_p", "sigma", "total")


def _judge(cilqr, solver, s, sigma0, W=None, cov="none", sel=slice(None), obstacles="dense", max_risk=1.0, base=None, plain=False):
    """The host forms through ctypes: cilqr_chance_risk_cov, or with plain=True cilqr_chance_risk.  cov: "none" (NULL) or an array in
    the obstacles' layout.  obstacles: "dense", None, or (pose, dim, M, strides)."""
    N = s["N"]
    X, U, K = (np.ascontiguousarray(s[n][sel]) for n in ("X", "U", "K"))
    B = X.shape[0]
    if obstacles == "dense":
        pose, dim, M = np.ascontiguousarray(s["pose"][sel]), np.ascontiguousarray(s["dim"][sel]), s["M"]
        st = (M * N, N, 1)
    elif obstacles is None:
        pose = dim = None
        M, st = 0, (0, 0, 0)
    else:
        pose, dim, M, st = obstacles
    o = None if M == 0 else cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, st[0], st[1], st[2], 0)
    cv = None if isinstance(cov, str) else np.ascontiguousarray(cov, dtype=np.float64)
    Wf = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
    base = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
    out = dict(risk=np.full((B, 6), -123.456), step_risk=np.full((B, N), -123.456), entry_p=np.full((B, M * N), -123.456),
               sigma=np.full((B, N + 1, 16), -123.456), total=None if base is None else np.full(B, -123.456))
    L = cilqr.lib()
    head = (solver._h, B, N, M, _p(X), _p(U), _p(K), _p(np.ascontiguousarray(sigma0)), C.c_int64(0), _p(Wf), None if o is None else C.byref(o))
    tail = (C.c_uint32(0), C.c_double(max_risk), _p(base), _p(out["risk"]), _p(out["step_risk"]), _p(out["entry_p"]), _p(out["sigma"]), _p(out["total"]))
    cilqr._check(L.cilqr_chance_risk(*head, *tail) if plain else L.cilqr_chance_risk_cov(*head, _p(cv), *tail))
    return out


def _same_judge(a, b, sel_a=slice(None), sel_b=slice(None)):
    for n in JUDGE_OUT:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
            continue
        if not np.array_equal(_bits(a[n][sel_a]), _bits(b[n][sel_b])):
            return False
    return True


@gpu
def test_null_and_zero_covariance_are_the_plain_call(cilqr, solver, cases):
    """Scene R: NULL and all-zero obs_cov give cilqr_chance_risk's bits in every output."""
    s, s0, W = cases["R"], cases["sigma0"], _cm(W_DIAG)
    base = np.linspace(1.0, 2.0, s["B"])
    kw = dict(W=W, max_risk=0.05, base=base)
    plain = _judge(cilqr, solver, s, s0, plain=True, **kw)
    assert np.isnan(plain["total"]).any() and not np.isnan(plain["total"]).all()
    assert _same_judge(_judge(cilqr, solver, s, s0, **kw), plain)
    assert _same_judge(_judge(cilqr, solver, s, s0, cov=np.zeros_like(cases["R_cov"]), **kw), plain)
    via = solver.chance_risk_cov(s["N"], s["X"], s["U"], s["K"], s0, W, s["pose"], s["dim"], obs_cov=None, max_risk=0.05, base=base)
    assert _same_judge(via, plain)


@gpu
def test_scene_r_with_a_covariance(cilqr, solver, cases):
    """Scene R with a covariance per entry against the restatement; strides shared against dense; a non-finite entry; batch
    independence; N = 1; M = 0; the binding."""
    s, s0, W, cov, want = cases["R"], cases["sigma0"], _cm(W_DIAG), cases["R_cov"], cases["R_want"]
    B, N, M = s["B"], s["N"], s["M"]
    base = np.linspace(1.0, 2.0, B)
    kw = dict(W=W, max_risk=0.05, base=base)
    got = _judge(cilqr, solver, s, s0, cov=cov, **kw)
    ks, ke = _check_against(got, want, "scene R with a covariance")
    assert ks.all() and ke.all()
    expect = _total(want["risk"], base, 0.05)
    assert np.array_equal(np.isnan(got["total"]), np.isnan(expect)) and _device_pick(solver, got["total"]) == _pick(expect)
    via = solver.chance_risk_cov(N, s["X"], s["U"], s["K"], s0, W, s["pose"], s["dim"], obs_cov=cov.reshape(B, M, 3 * N), max_risk=0.05, base=base)
    assert _same_judge(via, got)
    # each solve alone and the batch reversed
    for b in (0, 5):
        one = _judge(cilqr, solver, s, s0, W=W, cov=cov[b:b + 1], sel=slice(b, b + 1), max_risk=0.05, base=base[b:b + 1])
        assert _same_judge(one, got, sel_b=slice(b, b + 1)), b
    rev = _judge(cilqr, solver, s, s0, W=W, cov=cov[::-1], sel=slice(None, None, -1), max_risk=0.05, base=base[::-1])
    assert _same_judge(rev, got, sel_b=slice(None, None, -1))
    # one obstacle set (solve 3's) shared by the batch, strides (0, N, 1), against its dense expansion
    pose1, dim1, cov1 = np.ascontiguousarray(s["pose"][3]), np.ascontiguousarray(s["dim"][3]), np.ascontiguousarray(cov[3])
    dense = (np.ascontiguousarray(np.broadcast_to(pose1[None], (B, M, 4 * N))), np.ascontiguousarray(np.broadcast_to(dim1[None], (B, M, 2 * N))), M, (M * N, N, 1))
    d = _judge(cilqr, solver, s, s0, cov=np.ascontiguousarray(np.broadcast_to(cov1[None], (B, M, N, 3))), obstacles=dense, **kw)
    sh = _judge(cilqr, solver, s, s0, cov=cov1, obstacles=(pose1, dim1, M, (0, N, 1)), **kw)
    assert _same_judge(sh, d)
    _check_against(d, restate_cov(s["p"], N, s["X"], s["U"], s["K"], s0, W, dense[0], dense[1], np.broadcast_to(cov1[None], (B, M, N, 3))), "solve 3's obstacles for every solve")
    # a non-finite covariance entry: entry_p = 1 there, no other solve changes
    for comp, val in ((0, np.nan), (1, np.nan), (2, np.nan), (0, np.inf), (1, -np.inf), (2, np.inf)):  # xx, xy, yy: each alone decides
        bad = cov.copy()
        bad[2, 1, 4, comp] = val
        g = _judge(cilqr, solver, s, s0, cov=bad, **kw)
        assert g["entry_p"][2, 1 * N + 4] == 1.0 and g["step_risk"][2, 4] == 1.0 and g["risk"][2, STEP_RISK] == 1.0 and np.isnan(g["total"][2])
        others = np.setdiff1d(np.arange(B), [2])
        assert _same_judge(g, got, sel_a=others, sel_b=others)
        w = restate_cov(s["p"], N, s["X"], s["U"], s["K"], s0, W, s["pose"], s["dim"], bad)
        assert np.all(np.abs(g["entry_p"] - w["entry_p"]) <= TOL) and np.all(np.abs(g["step_risk"] - w["step_risk"]) <= TOL)
    # N = 1
    cut = dict(s)
    cut.update(N=1, X=np.ascontiguousarray(s["X"][:, :8]), U=np.ascontiguousarray(s["U"][:, :2]), K=np.ascontiguousarray(s["K"][:, :8]),
               pose=np.ascontiguousarray(s["pose"].reshape(B, M, N, 4)[:, :, :1].reshape(B, M, 4)),
               dim=np.ascontiguousarray(s["dim"].reshape(B, M, N, 2)[:, :, :1].reshape(B, M, 2)))
    g = _judge(cilqr, solver, cut, s0, W=W, cov=cov[:, :, :1])
    _check_against(g, restate_cov(s["p"], 1, cut["X"], cut["U"], cut["K"], s0, W, cut["pose"], cut["dim"], cov[:, :, :1]), "N = 1")
    # M = 0: obs_cov is not read
    g = _judge(cilqr, solver, s, s0, W=W, cov=np.full(3, np.nan), obstacles=None)
    assert _same_judge(g, _judge(cilqr, solver, s, s0, W=W, obstacles=None, plain=True))
    assert np.all(g["risk"][:, [STEP_RISK, SUM_RISK, MAX_P]] == 0.0) and np.all(g["risk"][:, [WORST_STEP, MAX_ENTRY]] == -1.0)


@gpu
def test_scene_t_the_predicted_covariance_moves_the_pick(cilqr, solver, cases):
    """Tracks -> cilqr_predict_obstacles_device -> cilqr_chance_risk_cov_device on the buffers it wrote, strides (0, N, 1) -> argmin:
    CR_STEP_RISK 0.1566, 0.0362, 0.0068, 0.00093 against below 1e-60 without the covariance; with max_risk 0.05 and the cheapest
    candidate at y = 0 the pick moves from candidate 0 to candidate 1."""
    import torch
    s, w = cases["T"], cases["T_want"]
    B, N, M = s["B"], s["N"], 1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    pred = _predict(solver, N, s["track"][None], s["track_dim"][None], s["track_cov"][None], s["Q"], keep=True)
    host = {k: v.cpu().numpy() for k, v in pred.items()}
    _check_prediction(host, dict(pose=w["pred"]["pose"][None], sigma=w["pred"]["sigma"][None]), s["track"][None], s["track_dim"][None], s["track_cov"][None], "scene T's track")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    t = {n: up(s[n]) for n in ("X", "U", "K", "sigma0", "base")}
    z = lambda *shape: torch.full(shape, -123.456, dtype=torch.float64, device=dev)  # noqa: E731
    picks = {}
    for name, cov_ptr in (("with_cov", pred["cov"].data_ptr()), ("without", 0)):
        out = dict(risk=z(B, 6), step_risk=z(B, N), entry_p=z(B, M * N), sigma=z(B, N + 1, 16), total=z(B))
        pair = torch.zeros(2, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        solver.chance_risk_cov_device(stream, B, N, M, t["X"].data_ptr(), t["U"].data_ptr(), t["K"].data_ptr(), t["sigma0"].data_ptr(), 0, 0,
                                      pred["pose"].data_ptr(), pred["dim"].data_ptr(), (0, N, 1, 0), cov_ptr, out["risk"].data_ptr(),
                                      out["step_risk"].data_ptr(), out["entry_p"].data_ptr(), out["sigma"].data_ptr(), out["total"].data_ptr(),
                                      t["base"].data_ptr(), max_risk=0.05)
        solver.argmin_device(stream, B, out["total"].data_ptr(), pair.data_ptr())
        torch.cuda.synchronize(dev)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        ks, ke = _check_against(got, w[name], "scene T, " + name)
        if name == "with_cov":
            assert ks.all() and ke.all()
        expect = _total(w[name]["risk"], s["base"], 0.05)
        assert np.array_equal(np.isnan(got["total"]), np.isnan(expect)) and np.array_equal(got["total"][~np.isnan(expect)], expect[~np.isnan(expect)])
        picks[name] = int(pair.cpu().numpy()[1])
        assert picks[name] == _pick(expect), name
        print("scene T, %s: CR_STEP_RISK %s, pick %d" % (name, got["risk"][:, STEP_RISK].tolist(), picks[name]))
    assert picks == {"with_cov": 1, "without": 0}


@gpu
def test_cpp_facade_tracked_candidates(tmp_path, oracle):
    """tests/cpp/candidates_tracked.cpp on scene F: set_tracked_obstacles equals the hand-built set_Obstacle + set_obstacle_covariance in
    picks and plans, bit for bit; with the check off run_candidates gives the results of a planner that knows neither call; with
    set_obstacle_covariance_check(true) the pick is the one the CPU figures give (0 -> 1) and the device's CR_STEP_RISK agrees with them
    to the scene's margin; a horizon change predicts again; clear_Obstacle removes everything."""
    f = _scene_f(oracle)
    exe = str(tmp_path / "candidates_tracked")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_tracked.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, repr(F_MAX_RISK), str(f["pick_off"]), str(f["pick_on"])], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("tracked equals hand-built ok", "check off is the parent ok", "check changes the pick ok", "horizon change and clear ok"):
        assert line in r.stdout, line
    got = np.array([float(m) for m in re.findall(r"CR_STEP_RISK with the covariance (\S+) ", r.stdout)])
    assert got.shape == (4,)
    d = np.abs(got - f["with_cov"])
    print("device CR_STEP_RISK against the CPU figures: max |d| %.3g (margin %g)" % (d.max(), F_MARGIN))
    assert np.all(d < F_MARGIN)
