"""Analytic pose-noise risk (cilqr_chance_risk*, include/cilqr.h): the closed-loop covariance chain Sigma_0 -> Sigma_N of a solved plan
under u = U_t + K_t (x - X_t), and from Sigma_t the Gaussian chance value of every (obstacle, step, ego circle).

Expected values never come from the HIP path: the oracle's trajectories and gains (_scene_r, _scene_l, o_gains of
tests/test_rollout_risk.py, lamb = 1) and `restate` below, a numpy restatement of the header's definitions with math.erfc for the normal
distribution.  Its cbar is additionally asserted equal, to 1e-12, to the c that test_candidate_score._expected derives from the oracle's
obstacle cost.  Tolerances are the suite's own: Sigma entries |d| <= 1e-9 * max(1, max|Sigma| of that solve) (_close); entry_p, step_risk
and the three probability fields 1e-9 absolute, entry_p also 1e-9 relative where the expected p >= 1e-150; MAX_POS_SIGMA 1e-9; steps,
entries and picks exact; total bit-equal to base, or NaN.

What makes the exact comparisons meaningful is asserted on the restatement's numbers in test_conditions: float64 and numpy.longdouble
runs agree to 1e-11; for every solve of scene R the largest and second-largest r_t, and the two largest entry_p, are more than 1e-6
apart; thresholds are more than 1e-6 from every value they separate.  Where a case has solves that do not meet the gap (scene L: p
saturates at 1 or underflows; the one- and two-step cuts of scene R), steps and entries are compared for the solves that do, the test
prints which, and values are compared for all.

  R0   scene R (B 8, N 12, M 3), Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2) shared, W none
  RS   the same with W = diag(1e-4, 1e-4, 4e-4, 1e-6)   (conditions only)
  RW   scene R, that W, Sigma_0 per solve: solve b scaled by 1 + 0.1 b, x-y correlation 0.3, NaN below the diagonal (never read)
  L0   scene L (B 6, N 50, M 4), the shared Sigma_0, W none;   LZ  scene L with Sigma_0 = 0: s = 0 everywhere, p in {0, 1}

The kernel's LDS, 8*(33*N + M*N + 16) bytes, exceeds 64 KiB above N = 247 without obstacles and above N = 220 with M = 4, inside
CILQR_MAX_HORIZON = 384: test_limits runs the largest horizons that fit and asserts CILQR_ERR_UNSUPPORTED one step beyond.
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import _bits, _expected
from test_rollout_risk import _close, _pick, _scene_l, _scene_r, o_gains

gpu = pytest.mark.gpu

TOL, MARGIN = 1e-9, 1e-6
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_chance_risk", "cilqr_chance_risk_device")
FIELDS = ("STEP_RISK", "WORST_STEP", "SUM_RISK", "MAX_P", "MAX_ENTRY", "MAX_POS_SIGMA")
STEP_RISK, WORST_STEP, SUM_RISK, MAX_P, MAX_ENTRY, MAX_POS_SIGMA = range(6)
BOUND_SUM = 1
SIGMA0 = np.diag([0.16 ** 2, 0.16 ** 2, 0.0, 0.017 ** 2])
W_DIAG = np.diag([1e-4, 1e-4, 4e-4, 1e-6])
_dp = C.POINTER(C.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


# ---- expected values: a numpy restatement of the header's definitions ------------------------------------------------------------
def _sym(a, T):
    """(16,) column-major, only row <= column read -> symmetric (4, 4) [r][c]."""
    m = np.asarray(a, dtype=T).reshape(4, 4).T  # entry (r, c) at [r + 4*c]
    u = np.triu(m)
    return u + np.triu(m, 1).T


def restate(p, N, X, U, K, sigma0, W, pose, dim, T=np.float64):
    """X (B, 4(N+1)), U (B, 2N), K (B, 8N); sigma0 (16,) shared or (B, 16); W (16,) or None; pose (B, M, 4N), dim (B, M, 2N) dense or
    None.  Returns dict(sigma (B, N+1, 16), cbar (B, M, N, 2), entry_p (B, M*N), step_risk (B, N), risk (B, 6)), float64 whatever T."""
    B = X.shape[0]
    M = 0 if pose is None else pose.shape[1]
    Xs, Us, Ks = X.reshape(B, N + 1, 4).astype(T), U.reshape(B, N, 2).astype(T), K.reshape(B, N, 4, 2).astype(T)  # K[t, c, r]
    dt = T(p.timestep)
    s0 = np.broadcast_to(np.asarray(sigma0).reshape(-1, 16), (B, 16))
    Wm = np.zeros((4, 4), dtype=T) if W is None else _sym(W, T)
    sig = np.zeros((B, N + 1, 4, 4), dtype=T)
    with np.errstate(invalid="ignore", over="ignore"):
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
        cbar, pp = np.zeros((B, M, N, 2)), np.zeros((B, M, N, 2))
        root2 = np.sqrt(T(2))
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
                    s = np.sqrt(np.fmax(q, 0))
                    cbar[b, m, :, side] = c.astype(np.float64)
                    for t in range(N):
                        if s[t] > 0:
                            z = float(-c[t] / (s[t] * root2))
                            pp[b, m, t, side] = z if math.isnan(z) else 0.5 * math.erfc(z)
                        else:
                            pp[b, m, t, side] = 1.0 if c[t] > 0 else 0.0
        entry_p = np.fmax(pp[..., 0], pp[..., 1]).reshape(B, M * N)  # a NaN never wins
        sig64 = sig.astype(np.float64)
        lost = ~(np.isfinite(Xs[:, :N]).all(axis=2) & np.isfinite(Us).all(axis=2) & np.isfinite(Ks).all(axis=(2, 3))
                 & np.isfinite(sig64[:, :N]).all(axis=(2, 3)))
        step_risk = np.where(lost, 1.0, np.fmin(1.0, entry_p.reshape(B, M, N).sum(axis=1)))
        risk = np.zeros((B, 6))
        risk[:, STEP_RISK] = step_risk.max(axis=1)
        risk[:, WORST_STEP] = step_risk.argmax(axis=1) if M else -1
        risk[:, SUM_RISK] = np.minimum(1.0, step_risk.sum(axis=1))
        if M:
            e = np.where(np.isnan(entry_p), -np.inf, entry_p)
            risk[:, MAX_P], risk[:, MAX_ENTRY] = e.max(axis=1), e.argmax(axis=1)
        else:
            risk[:, MAX_P], risk[:, MAX_ENTRY] = 0.0, -1
        a, d, bb = sig64[:, :, 0, 0], sig64[:, :, 1, 1], sig64[:, :, 0, 1]
        lam = 0.5 * (a + d) + np.sqrt((0.5 * (a - d)) ** 2 + bb * bb)
        risk[:, MAX_POS_SIGMA] = np.sqrt(np.fmax.reduce(np.fmax(lam, 0.0), axis=1))
    return dict(sigma=sig64.reshape(B, N + 1, 16), cbar=cbar, entry_p=entry_p, step_risk=step_risk, risk=risk, B=B, N=N, M=M)


def _total(risk, base, max_risk, sum_bound=False):
    field = risk[:, SUM_RISK if sum_bound else STEP_RISK]
    return np.where((field > max_risk) | ~np.isfinite(base), np.nan, base)


def _decided(want):
    """Per solve: is WORST_STEP decided (largest and second-largest r_t more than 1e-6 apart), is MAX_ENTRY (the two largest entry_p)?"""
    def gap(v):
        if v.shape[1] < 2:
            return np.full(v.shape[0], np.inf)
        s = np.sort(np.where(np.isnan(v), -np.inf, v), axis=1)
        return s[:, -1] - s[:, -2]
    return gap(want["step_risk"]), gap(want["entry_p"])


def _per_solve_sigma0(B):
    """(B, 16): solve b's Sigma_0 = (1 + 0.1 b) * [the shared one with an x-y correlation of 0.3]; NaN below the diagonal."""
    out = np.zeros((B, 16))
    for b in range(B):
        S = SIGMA0.copy()
        S[0, 1] = S[1, 0] = 0.3 * 0.16 * 0.16
        S = (1.0 + 0.1 * b) * S
        S[np.tril_indices(4, -1)] = np.nan
        out[b] = S.T.reshape(16)  # column-major
    return out


def _cut(s, N):
    """The first N steps of scene `s`."""
    B, M, N0 = s["B"], s["M"], s["N"]
    out = dict(s)
    out.update(N=N, X=np.ascontiguousarray(s["X"][:, :4 * (N + 1)]), U=np.ascontiguousarray(s["U"][:, :2 * N]),
               K=np.ascontiguousarray(s["K"][:, :8 * N]),
               pose=np.ascontiguousarray(s["pose"].reshape(B, M, N0, 4)[:, :, :N].reshape(B, M, 4 * N)),
               dim=np.ascontiguousarray(s["dim"].reshape(B, M, N0, 2)[:, :, :N].reshape(B, M, 2 * N)))
    return out


def _want(s, sigma0, W, T=np.float64, obstacles=True):
    return restate(s["p"], s["N"], s["X"], s["U"], s["K"], sigma0, None if W is None else W.T.reshape(16),
                   s["pose"] if obstacles else None, s["dim"] if obstacles else None, T)


@pytest.fixture(scope="module")
def cases(oracle):
    """Scenes R and L with the oracle's gains (lamb = 1) and the restatement's numbers for every case.  Computed once; never modified."""
    O = oracle
    r, l = _scene_r(O), _scene_l(O)
    for s in (r, l):
        s["pose"], s["dim"] = np.ascontiguousarray(s["pose"]).reshape(s["B"], s["M"], -1), np.ascontiguousarray(s["dim"]).reshape(s["B"], s["M"], -1)
        _, s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
        assert np.all(ok == 1)
    s0 = SIGMA0.T.reshape(16)
    rw0 = _per_solve_sigma0(r["B"])
    out = {"R": r, "L": l, "rw_sigma0": rw0, "sigma0": s0,
           "R0": _want(r, s0, None), "RS": _want(r, s0, W_DIAG), "RW": _want(r, rw0, W_DIAG),
           "L0": _want(l, s0, None), "LZ": _want(l, np.zeros(16), None),
           "R_N1": _want(_cut(r, 1), s0, None), "R_N2": _want(_cut(r, 2), s0, None), "R_M0": _want(r, s0, None, obstacles=False)}
    return out


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_CHANCE_FIELDS\s+6\b", h)
    assert re.search(r"#define\s+CILQR_CHANCE_BOUND_SUM\s+1u\b", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_CR_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "CR_" + name) == i
    assert cilqr.CHANCE_FIELDS == 6 and cilqr.CHANCE_BOUND_SUM == 1
    assert callable(cilqr.Solver.chance_risk) and callable(cilqr.Solver.chance_risk_device)
    assert "8*(33*N + M*N + 16)" in full  # the LDS formula is stated
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_pose_covariance_check\s*\(\s*const\s+double\s+Sigma0\[16\]\s*,\s*const\s+double\*\s+W\s*,\s*double\s+max_risk\s*,"
                     r"\s*double\s+lamb\s*=\s*1\.0\s*,\s*bool\s+sum_bound\s*=\s*false\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_chance_risk\s*,\s*last_step_risk\s*;", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_chance_risk\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_chance.hip" in mk and re.search(r"^check:.*build/cilqr_chance\.o", mk, flags=re.M)


def test_argument_errors_need_no_device(cilqr):
    """NULL X, U, K, sigma0 or risk, total without base, obs NULL with M > 0, a negative stride, sigma0_batch_stride outside {0, 1}, a NaN
    max_risk, unknown flag bits: CILQR_ERR_ARG, decided before the handle is looked at (there is none here).  The limits of a handle and
    the arena's are in test_limits."""
    L = cilqr.lib()
    B, N, M = 2, 4, 1
    X, U, K, s0, W = np.zeros((B, 4 * (N + 1))), np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros(16), np.zeros(16)
    pose, dim = np.zeros((B, M, 4 * N)), np.ones((B, M, 2 * N))
    risk, step, ep, so, total, base = np.zeros((B, 6)), np.zeros((B, N)), np.zeros((B, M * N)), np.zeros((B, N + 1, 16)), np.zeros(B), np.zeros(B)
    no_handle = C.c_void_p()
    nan = float("nan")

    def call(dev, stride=0, flags=0, mr=1.0, M_=M, obs="dense", obs_strides=(M * N, N, 1, 0), **nulls):
        a = dict(X=X, U=U, K=K, sigma0=s0, risk=risk, base=base, total=total)
        a.update(nulls)
        o = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, *obs_strides)
        f = L.cilqr_chance_risk_device if dev else L.cilqr_chance_risk
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, M_, _p(a["X"]), _p(a["U"]), _p(a["K"]), _p(a["sigma0"]), C.c_int64(stride), _p(W),
                 C.byref(o) if obs else None, C.c_uint32(flags), C.c_double(mr), _p(a["base"]), _p(a["risk"]), _p(step), _p(ep), _p(so),
                 _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "U", "K", "sigma0", "risk"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert call(dev, obs=None) == ERR_ARG and b"obs is null" in L.cilqr_last_error()
        for k in range(3):
            st = [M * N, N, 1, 0]
            st[k] = -1
            assert call(dev, obs_strides=tuple(st)) == ERR_ARG and b"negative stride" in L.cilqr_last_error(), k
        assert call(dev, stride=-1) == ERR_ARG and b"negative stride" in L.cilqr_last_error()
        assert call(dev, stride=2) == ERR_ARG and b"sigma0_batch_stride" in L.cilqr_last_error()
        assert call(dev, mr=nan) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert call(dev, flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev, flags=1, stride=1) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, base=None, total=None, M_=0, obs=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid too


def _agree(a, b, what):
    """float64 against longdouble, in the measures of the GPU comparisons: a hundredth of their tolerance."""
    B = a["B"]
    scale = np.maximum(1.0, np.max(np.abs(a["sigma"].reshape(B, -1)), axis=1))
    ds = float(np.max(np.max(np.abs(a["sigma"] - b["sigma"]).reshape(B, -1), axis=1) / scale))
    dp = float(np.max(np.abs(a["entry_p"] - b["entry_p"]))) if a["M"] else 0.0
    big = b["entry_p"] >= 1e-150
    drel = float(np.max(np.abs(a["entry_p"] - b["entry_p"])[big] / b["entry_p"][big])) if big.any() else 0.0
    dr = float(np.max(np.abs(a["step_risk"] - b["step_risk"])))
    df = float(np.max(np.abs(a["risk"][:, [STEP_RISK, SUM_RISK, MAX_P, MAX_POS_SIGMA]] - b["risk"][:, [STEP_RISK, SUM_RISK, MAX_P, MAX_POS_SIGMA]])))
    print("%s, float64 vs longdouble: Sigma %.3g (scaled), entry_p %.3g abs %.3g rel, step_risk %.3g, fields %.3g" % (what, ds, dp, drel, dr, df))
    assert max(ds, dp, drel, dr, df) <= 1e-11, what


def test_conditions(oracle, cases):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the restatement's numbers alone."""
    r, l = cases["R"], cases["L"]
    s0 = cases["sigma0"]
    # cbar is the oracle's c (through test_candidate_score._expected: the logarithm of its barrier value, where that has not underflowed)
    for s, name in ((r, "R0"), (l, "L0")):
        _, c = _expected(oracle, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"])
        fin = np.isfinite(c)
        d = float(np.max(np.abs(cases[name]["cbar"] - c)[fin]))
        print("scene %s: cbar vs the oracle's c, %d of %d entries finite, max |d| %.3g" % (name[0], int(fin.sum()), fin.size, d))
        assert fin.any() and d <= 1e-12
    assert np.longdouble(1) + np.finfo(np.longdouble).eps != 1 and np.finfo(np.longdouble).eps < 1e-18  # longdouble is wider here
    for name, s, sig, W in (("R0", r, s0, None), ("RS", r, s0, W_DIAG), ("RW", r, cases["rw_sigma0"], W_DIAG), ("L0", l, s0, None)):
        _agree(cases[name], _want(s, sig, W, np.longdouble), name)
    # every solve of scene R is decided, with and without process noise, shared and per-solve Sigma_0
    for name in ("R0", "RS", "RW"):
        gs, ge = _decided(cases[name])
        print("%s: smallest r_t gap %.3g, smallest entry_p gap %.3g; STEP_RISK %s; SUM_RISK %s" % (
            name, gs.min(), ge.min(), np.round(cases[name]["risk"][:, STEP_RISK], 5).tolist(), np.round(cases[name]["risk"][:, SUM_RISK], 5).tolist()))
        assert gs.min() > MARGIN and ge.min() > MARGIN, name
    for name in ("L0", "LZ", "R_N1", "R_N2"):
        gs, ge = _decided(cases[name])
        print("%s: WORST_STEP decided for solves %s, MAX_ENTRY for %s" % (name, np.nonzero(gs > MARGIN)[0].tolist(), np.nonzero(ge > MARGIN)[0].tolist()))
    # the thresholds of the picks: 0.05 on STEP_RISK rejects candidates 0-3 of R0 alone, on SUM_RISK candidate 4 as well
    step, total = cases["R0"]["risk"][:, STEP_RISK], cases["R0"]["risk"][:, SUM_RISK]
    assert np.min(np.abs(step - 0.05)) > MARGIN and np.min(np.abs(total - 0.05)) > MARGIN and step.min() > MARGIN
    assert (step > 0.05).tolist() == [True] * 4 + [False] * 4 and (total > 0.05).tolist() == [True] * 5 + [False] * 3
    # the analytic figures order the four candidates the rollouts call 0/70
    assert len(set(np.round(step[4:], 6).tolist())) == 4
    # Sigma_0 = 0: every cbar of scene L is decided in sign, and some are contacts
    c = cases["LZ"]["cbar"]
    assert np.min(np.abs(c)) > MARGIN and (c > 0).any() and (c < 0).any()
    assert set(np.unique(cases["LZ"]["entry_p"]).tolist()) == {0.0, 1.0} and not cases["LZ"]["sigma"].any()
    # per-solve Sigma_0 matters: the shared one would give other numbers
    assert np.min(np.abs(cases["RW"]["risk"][1:, STEP_RISK] - cases["RS"]["risk"][1:, STEP_RISK])) > 1e-6


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_chance.cpp: plan_chance_risk laid out without an arena against host_arena_bytes at the shapes include/cilqr.h
    says always fit; and host_arena_bytes is still what tests/golden/host_arena_cap.json recorded before this call existed."""
    import json
    exe = str(tmp_path / "host_plan_chance")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_chance.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1200:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "13 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


OUTPUTS = ("step_risk", "entry_p", "sigma", "total")


def _host(cilqr, solver, s, sigma0, W=None, sel=slice(None), obstacles="dense", max_risk=1.0, base=None, flags=0, skip=()):
    """The host form through ctypes (every optional output can be left out: `skip`).  obstacles: "dense", None, or (pose, dim, M,
    (batch, obstacle, step) strides).  Returns dict(risk, step_risk, entry_p, sigma, total), None where not asked for."""
    N = s["N"]
    X, U, K = (np.ascontiguousarray(s[n][sel]) for n in ("X", "U", "K"))
    B = X.shape[0]
    sigma0 = np.ascontiguousarray(sigma0)
    stride = 0 if sigma0.size == 16 else 1
    if stride:
        sigma0 = np.ascontiguousarray(sigma0.reshape(-1, 16)[sel])
    if obstacles == "dense":
        pose, dim, M = np.ascontiguousarray(s["pose"][sel]), np.ascontiguousarray(s["dim"][sel]), s["M"]
        st = (M * N, N, 1)
    elif obstacles is None:
        pose = dim = None
        M, st = 0, (0, 0, 0)
    else:
        pose, dim, M, st = obstacles
    o = None if M == 0 else cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, st[0], st[1], st[2], 0)
    Wf = None if W is None else np.ascontiguousarray(W.T.reshape(16))
    base = None if base is None else np.ascontiguousarray(base, dtype=np.float64)
    out = dict(risk=np.full((B, 6), -123.456), step_risk=np.full((B, N), -123.456), entry_p=np.full((B, M * N), -123.456), sigma=np.full((B, N + 1, 16), -123.456),
               total=None if base is None else np.full(B, -123.456))
    for n in skip:
        out[n] = None
    cilqr._check(cilqr.lib().cilqr_chance_risk(solver._h, B, N, M, _p(X), _p(U), _p(K), _p(sigma0), C.c_int64(stride), _p(Wf),
                                               None if o is None else C.byref(o), C.c_uint32(flags), C.c_double(max_risk), _p(base),
                                               _p(out["risk"]), _p(out["step_risk"]), _p(out["entry_p"]), _p(out["sigma"]), _p(out["total"])))
    return out


def _device(solver, s, sigma0, W=None, max_risk=1.0, base=None, flags=0):
    """The device form on torch buffers, dense obstacles."""
    import torch
    B, N, M = s["B"], s["N"], s["M"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    t = {n: up(s[n]) for n in ("X", "U", "K", "pose", "dim")}
    ts0, tW = up(sigma0), None if W is None else up(W.T.reshape(16))
    tb = None if base is None else up(base)
    z = lambda *shape: torch.full(shape, -123.456, dtype=torch.float64, device=dev)  # noqa: E731
    risk, step, ep, so, total = z(B, 6), z(B, N), z(B, M * N), z(B, N + 1, 16), z(B)
    torch.cuda.synchronize(dev)
    solver.chance_risk_device(stream, B, N, M, t["X"].data_ptr(), t["U"].data_ptr(), t["K"].data_ptr(), ts0.data_ptr(),
                              0 if np.asarray(sigma0).size == 16 else 1, 0 if tW is None else tW.data_ptr(), t["pose"].data_ptr(),
                              t["dim"].data_ptr(), (M * N, N, 1, 0), risk.data_ptr(), step.data_ptr(), ep.data_ptr(), so.data_ptr(),
                              total.data_ptr() if tb is not None else 0, tb.data_ptr() if tb is not None else 0, max_risk=max_risk, flags=flags)
    torch.cuda.synchronize(dev)
    out = dict(risk=risk, step_risk=step, entry_p=ep, sigma=so, total=total)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    if tb is None:
        out["total"] = None
    return out


def _same(a, b, sel_a=slice(None), sel_b=slice(None), names=("risk",) + OUTPUTS):
    for n in names:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
            continue
        if not np.array_equal(_bits(a[n][sel_a]), _bits(b[n][sel_b])):
            return False
    return True


def _check_against(got, want, what, sel=slice(None)):
    """Values to tolerance for every solve; WORST_STEP and MAX_ENTRY exact for the solves whose maxima are decided (printed)."""
    w = {n: want[n][sel] for n in ("sigma", "entry_p", "step_risk", "risk")}
    B, M = w["risk"].shape[0], want["M"]
    assert all(np.all(got[n] != -123.456) for n in ("risk", "step_risk", "sigma")), what  # everything was written
    _close(got["sigma"].reshape(B, -1), w["sigma"].reshape(B, -1), what + ": Sigma")
    assert np.array_equal(got["sigma"].reshape(B, -1, 4, 4), got["sigma"].reshape(B, -1, 4, 4).transpose(0, 1, 3, 2)), what  # exactly symmetric
    dp = np.abs(got["entry_p"] - w["entry_p"])
    big = w["entry_p"] >= 1e-150
    rel = float(np.max(dp[big] / w["entry_p"][big])) if big.any() else 0.0
    fields = [STEP_RISK, SUM_RISK, MAX_P, MAX_POS_SIGMA]
    df = np.abs(got["risk"][:, fields] - w["risk"][:, fields])
    print("%s: entry_p max |d| %.3g abs, %.3g rel over %d entries >= 1e-150; step_risk %.3g; STEP, SUM, MAX_P, MAX_POS_SIGMA %s" % (
        what, float(dp.max()) if dp.size else 0.0, rel, int(big.sum()), float(np.max(np.abs(got["step_risk"] - w["step_risk"]))),
        df.max(axis=0).tolist()))
    if M:
        assert np.all(dp <= TOL) and rel <= TOL, what
    assert np.all(np.abs(got["step_risk"] - w["step_risk"]) <= TOL), what
    assert np.all(df <= TOL), what
    gs, ge = _decided(w)
    ks, ke = gs > MARGIN, ge > MARGIN
    print("  WORST_STEP compared for solves %s, MAX_ENTRY for %s" % (np.nonzero(ks)[0].tolist(), np.nonzero(ke)[0].tolist()))
    assert np.array_equal(got["risk"][ks, WORST_STEP], w["risk"][ks, WORST_STEP]), (what, got["risk"][:, WORST_STEP], w["risk"][:, WORST_STEP])
    assert np.array_equal(got["risk"][ke, MAX_ENTRY], w["risk"][ke, MAX_ENTRY]), (what, got["risk"][:, MAX_ENTRY], w["risk"][:, MAX_ENTRY])
    return ks, ke


def _device_pick(solver, values):
    import torch
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    solver.argmin_device(torch.cuda.current_stream(dev).cuda_stream, len(values), v.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)
    return int(out.cpu().numpy()[1])


def _check_total(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(_bits(got[~np.isnan(want)]), _bits(want[~np.isnan(want)])), what


@gpu
def test_scene_r_against_the_restatement(cilqr, solver, cases):
    """R0: every output, all 8 solves compared exactly in steps and entries; the risk-bounded picks."""
    s, want = cases["R"], cases["R0"]
    B = s["B"]
    got = _host(cilqr, solver, s, cases["sigma0"])
    ks, ke = _check_against(got, want, "R0")
    assert ks.all() and ke.all()
    base = np.linspace(3.0, 2.0, B)
    base[1] = 1.0  # the cheapest candidate is the riskiest: the bound changes the pick
    picks = []
    for max_risk, flags in ((0.05, 0), (0.05, BOUND_SUM), (0.0, 0), (1.0, 0)):
        t = _host(cilqr, solver, s, cases["sigma0"], max_risk=max_risk, base=base, flags=flags)
        expect = _total(want["risk"], base, max_risk, bool(flags))
        _check_total(t["total"], expect, (max_risk, flags))
        assert _same(t, got, names=("risk", "step_risk", "entry_p", "sigma"))
        assert _device_pick(solver, t["total"]) == _pick(expect), (max_risk, flags)
        picks.append((_pick(expect), np.isnan(expect).tolist()))
    assert picks[0][1] == [True] * 4 + [False] * 4 and picks[1][1] == [True] * 5 + [False] * 3
    assert picks[2] == (-1, [True] * B) and picks[3][0] == 1 and picks[0][0] != 1
    nan_base = base.copy()
    nan_base[6] = np.nan  # a base that is already rejected stays rejected
    t = _host(cilqr, solver, s, cases["sigma0"], max_risk=1.0, base=nan_base)
    _check_total(t["total"], _total(want["risk"], nan_base, 1.0), "a NaN base")


@gpu
def test_process_noise_and_per_solve_sigma0(cilqr, solver, cases):
    """RW: W = diag(1e-4, 1e-4, 4e-4, 1e-6), Sigma_0 per solve (stride 1) with an x-y correlation, NaN below the diagonal of every
    Sigma_0 and of W: only row <= column is read."""
    s, want = cases["R"], cases["RW"]
    W = W_DIAG.copy()
    W[np.tril_indices(4, -1)] = np.nan
    got = _host(cilqr, solver, s, cases["rw_sigma0"], W=W)
    ks, ke = _check_against(got, want, "RW")
    assert ks.all() and ke.all()
    assert np.all(np.abs(got["sigma"][:, 0].reshape(-1, 4, 4)[:, 0, 1] - 0.3 * 0.16 * 0.16 * (1 + 0.1 * np.arange(s["B"]))) < 1e-15)


@gpu
def test_a_result_depends_on_its_own_solve_alone(cilqr, solver, cases):
    """Each solve of scene R alone (B = 1) and the batch reversed give the batch's bits in every output (RW: per-solve Sigma_0)."""
    s = cases["R"]
    B = s["B"]
    base = np.linspace(1.0, 2.0, B)
    kw = dict(W=W_DIAG, max_risk=0.05, base=base)
    whole = _host(cilqr, solver, s, cases["rw_sigma0"], **kw)
    assert np.isnan(whole["total"]).any() and not np.isnan(whole["total"]).all()
    for b in range(B):
        one = _host(cilqr, solver, s, cases["rw_sigma0"], sel=slice(b, b + 1), W=W_DIAG, max_risk=0.05, base=base[b:b + 1])
        assert _same(one, whole, sel_b=slice(b, b + 1)), b
    rev = _host(cilqr, solver, s, cases["rw_sigma0"], sel=slice(None, None, -1), W=W_DIAG, max_risk=0.05, base=base[::-1])
    assert _same(rev, whole, sel_b=slice(None, None, -1))


@gpu
def test_strides_and_optional_outputs(cilqr, solver, cases):
    """One obstacle set shared by the batch (batch_stride 0) and constant over the horizon (step_stride 0) equals its dense expansion bit
    for bit; every optional output left out, one at a time, leaves the others unchanged bit for bit."""
    s = cases["R"]
    B, N, M = s["B"], s["N"], s["M"]
    pose1 = np.ascontiguousarray(s["pose"].reshape(B, M, N, 4)[3, :, 0])  # (M, 4): solve 3's obstacles at step 0
    dim1 = np.ascontiguousarray(s["dim"].reshape(B, M, N, 2)[3, :, 0])
    dense_pose = np.ascontiguousarray(np.broadcast_to(pose1[None, :, None, :], (B, M, N, 4))).reshape(B, M, 4 * N)
    dense_dim = np.ascontiguousarray(np.broadcast_to(dim1[None, :, None, :], (B, M, N, 2))).reshape(B, M, 2 * N)
    base = np.linspace(1.0, 2.0, B)
    kw = dict(W=W_DIAG, max_risk=0.05, base=base)
    dense = _host(cilqr, solver, s, cases["sigma0"], obstacles=(dense_pose, dense_dim, M, (M * N, N, 1)), **kw)
    shared = _host(cilqr, solver, s, cases["sigma0"], obstacles=(pose1, dim1, M, (0, 1, 0)), **kw)
    assert _same(shared, dense)
    per_solve_static = np.ascontiguousarray(np.broadcast_to(pose1[None], (B, M, 4))), np.ascontiguousarray(np.broadcast_to(dim1[None], (B, M, 2)))
    assert _same(_host(cilqr, solver, s, cases["sigma0"], obstacles=per_solve_static + (M, (M, 1, 0)), **kw), dense)
    want = restate(s["p"], N, s["X"], s["U"], s["K"], cases["sigma0"], W_DIAG.T.reshape(16), dense_pose, dense_dim)
    _check_against(dense, want, "solve 3's obstacles for every solve")
    full = _host(cilqr, solver, s, cases["sigma0"], **kw)
    for n in OUTPUTS:
        part = _host(cilqr, solver, s, cases["sigma0"], skip=(n,), **({**kw, "base": None} if n == "total" else kw))
        assert part[n] is None
        assert _same(part, full, names=[m for m in ("risk",) + OUTPUTS if m != n]), n
    none = _host(cilqr, solver, s, cases["sigma0"], W=W_DIAG, skip=OUTPUTS)
    assert np.array_equal(_bits(none["risk"]), _bits(full["risk"]))


@gpu
def test_edges(cilqr, solver, cases):
    """N = 1 and N = 2; M = 0; Sigma_0 = 0 on scene L (nominal contacts: p is 1 or 0 by the sign of cbar); a NaN in K."""
    r, l = cases["R"], cases["L"]
    s0 = cases["sigma0"]
    for N in (1, 2):
        _check_against(_host(cilqr, solver, _cut(r, N), s0), cases["R_N%d" % N], "scene R cut to N = %d" % N)
    got = _host(cilqr, solver, r, s0, obstacles=None)
    _check_against(got, cases["R_M0"], "M = 0")
    assert np.all(got["risk"][:, [STEP_RISK, SUM_RISK, MAX_P]] == 0.0) and np.all(got["risk"][:, [WORST_STEP, MAX_ENTRY]] == -1.0)
    assert got["entry_p"].shape == (r["B"], 0) and not got["step_risk"].any()
    assert np.array_equal(_bits(got["sigma"]), _bits(_host(cilqr, solver, r, s0)["sigma"]))  # the chain does not depend on the obstacles
    got = _host(cilqr, solver, l, np.zeros(16))
    want = cases["LZ"]
    _check_against(got, want, "Sigma_0 = 0 on scene L")
    assert not got["sigma"].any() and np.array_equal(got["entry_p"], want["entry_p"]) and np.array_equal(got["step_risk"], want["step_risk"])
    assert set(np.unique(got["entry_p"]).tolist()) == {0.0, 1.0} and got["risk"][:, MAX_POS_SIGMA].tolist() == [0.0] * l["B"]
    # a NaN in K at step 5 of solve 2: r_t = 1 from there on, and the other solves keep their bits
    bad = dict(r)
    bad["K"] = r["K"].copy()
    bad["K"][2, 8 * 5 + 3] = np.nan
    base = np.linspace(1.0, 2.0, r["B"])
    clean = _host(cilqr, solver, r, s0, max_risk=0.5, base=base)
    got = _host(cilqr, solver, bad, s0, max_risk=0.5, base=base)
    want = _want(bad, s0, None)
    assert np.all(want["step_risk"][2, 5:] == 1.0) and np.all(want["step_risk"][2, :5] < 0.5 - MARGIN)
    assert np.all(got["step_risk"][2, 5:] == 1.0) and np.all(np.abs(got["step_risk"][2, :5] - want["step_risk"][2, :5]) <= TOL)
    assert got["risk"][2, STEP_RISK] == 1.0 and got["risk"][2, WORST_STEP] == 5.0 and got["risk"][2, SUM_RISK] == 1.0
    assert np.isnan(got["total"][2]) and not np.isnan(clean["total"]).any()
    assert np.isnan(got["sigma"][2, 6:]).any() and np.all(np.isfinite(got["sigma"][2, :6]))
    others = np.setdiff1d(np.arange(r["B"]), [2])
    assert _same(got, clean, sel_a=others, sel_b=others)
    assert _device_pick(solver, got["total"]) == _pick(_total(want["risk"], base, 0.5)) != 2


@gpu
def test_scene_l_the_workloads_horizon(cilqr, solver, cases):
    """L0 (B 6, N 50, M 4): values to tolerance for every solve; steps and entries for the solves whose maxima are decided."""
    got = _host(cilqr, solver, cases["L"], cases["sigma0"])
    _check_against(got, cases["L0"], "L0")
    withW = _host(cilqr, solver, cases["L"], cases["sigma0"], W=W_DIAG)
    _check_against(withW, _want(cases["L"], cases["sigma0"], W_DIAG), "scene L with process noise")


def _straight(N, B, M, seed):
    """A synthetic plan of any horizon: a gentle arc at 2 m/s, a stabilising constant gain, obstacles well to the side."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X, U, K = np.zeros((B, N + 1, 4)), np.zeros((B, N, 2)), np.zeros((B, N, 4, 2))
    for b in range(B):
        th = 0.002 * (b + 1) * np.arange(N + 1)
        X[b, :, 2], X[b, :, 3] = 2.0, th
        X[b, 1:, 0], X[b, 1:, 1] = np.cumsum(0.2 * np.cos(th[:-1])), np.cumsum(0.2 * np.sin(th[:-1]))
        U[b, :, 1] = 0.002 * (b + 1) / 0.1
    K[:, :, 2, 0] = -1.0                    # acceleration against the speed error
    K[:, :, 1, 1], K[:, :, 3, 1] = -0.5, -1.5  # yaw rate against the lateral and heading errors
    pose = np.zeros((B, M, N, 4))
    dim = np.ones((B, M, N, 2)) * [4.0, 2.0]
    for m in range(M):
        pose[:, m, :, 0] = X[:, :N, 0] + rng.uniform(-3, 3)
        pose[:, m, :, 1] = X[:, :N, 1] + rng.uniform(5.0, 7.0) * (1 if m % 2 else -1)
    return dict(B=B, N=N, M=M, X=X.reshape(B, -1), U=U.reshape(B, -1), K=K.reshape(B, -1), pose=pose.reshape(B, M, 4 * N), dim=dim.reshape(B, M, 2 * N))


@gpu
def test_limits(cilqr, oracle, cases):
    """The header's LDS formula decides CILQR_ERR_UNSUPPORTED exactly where it says: the largest horizon that fits runs and is right,
    one step more is refused.  B, N, M beyond the create limits and a host call beyond the arena are CILQR_ERR_ARG, and the handle
    stays usable."""
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    Nmax = int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1))
    lds = lambda N, M: 8 * (33 * N + M * N + 16)  # noqa: E731
    s0 = cases["sigma0"]
    for M, N in ((0, 247), (4, 220)):
        assert lds(N, M) <= 64 * 1024 < lds(N + 1, M) and N + 1 <= Nmax
        p = oracle.default_params(N)
        sv = cilqr.Solver(cilqr.default_params(N), max_batch=2, max_horizon=Nmax, max_obstacles=4, device=0)
        try:
            s = _straight(N, 1, M, 3)
            s["p"] = p
            got = _host(cilqr, sv, s, s0, W=W_DIAG, obstacles="dense" if M else None)
            _check_against(got, _want(s, s0, W_DIAG, obstacles=bool(M)), "N = %d, M = %d" % (N, M))
            big = _straight(N + 1, 1, M, 3)
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit 64 KiB of LDS" % ERR_UNSUPPORTED):
                _host(cilqr, sv, big, s0, obstacles="dense" if M else None)
            again = _host(cilqr, sv, s, s0, W=W_DIAG, obstacles="dense" if M else None)
            assert _same(again, got)
        finally:
            sv.close()
    r = cases["R"]
    sv = cilqr.Solver(cilqr.default_params(12), max_batch=8, max_horizon=12, max_obstacles=3, device=0)
    try:
        whole = _host(cilqr, sv, r, s0, skip=("entry_p", "sigma"))  # B = max_batch without the two large outputs: fits
        half = _host(cilqr, sv, r, s0, sel=slice(0, 4))            # B = max_batch / 2 with every output: fits
        assert np.array_equal(_bits(whole["risk"][:4]), _bits(half["risk"]))
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers reserved at create" % ERR_ARG):
            _host(cilqr, sv, r, s0)                                 # B = max_batch with every output: beyond the arena
        assert _same(_host(cilqr, sv, r, s0, sel=slice(0, 4)), half)
    finally:
        sv.close()
    sv = cilqr.Solver(cilqr.default_params(11), max_batch=7, max_horizon=11, max_obstacles=2, device=0)
    try:
        for sel, cut, obstacles, what in ((slice(None), 11, None, "B="), (slice(0, 4), 12, None, "N="), (slice(0, 4), 11, "dense", "M=")):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: %s" % (ERR_ARG, what)):
                _host(cilqr, sv, _cut(r, cut), s0, sel=sel, obstacles=obstacles)
    finally:
        sv.close()


@gpu
def test_host_form_equals_device_form(cilqr, solver, cases):
    """Scene R, both configurations: the same bits from both forms in every output."""
    s = cases["R"]
    base = np.linspace(1.0, 2.0, s["B"])
    for sigma0, W, flags in ((cases["sigma0"], None, 0), (cases["rw_sigma0"], W_DIAG, BOUND_SUM)):
        host = _host(cilqr, solver, s, sigma0, W=W, max_risk=0.05, base=base, flags=flags)
        dev = _device(solver, s, sigma0, W=W, max_risk=0.05, base=base, flags=flags)
        assert _same(host, dev)
        via_binding = solver.chance_risk(s["N"], s["X"], s["U"], s["K"], sigma0, None if W is None else W.T.reshape(16), s["pose"], s["dim"],
                                         max_risk=0.05, base=base, sum_bound=bool(flags))
        assert _same(host, via_binding)
    dev = _device(solver, s, cases["sigma0"])
    assert dev["total"] is None


@gpu
def test_cpp_facade_chance_checked_candidates(tmp_path):
    """tests/cpp/candidates_chance.cpp: under iLQR::set_pose_covariance_check the index run_candidates picks equals the pick computed from
    the C-ABI calls made by hand (solve, gains, chance risk, argmin) on the same candidates, last_chance_risk and last_step_risk are
    that call's bits, set_map_risk_check composes after it, and the two conflicting setters throw."""
    exe = str(tmp_path / "candidates_chance")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_chance.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "chance pick ok" in r.stdout and "conflicts throw ok" in r.stdout, r.stdout
