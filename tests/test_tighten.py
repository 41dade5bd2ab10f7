"""Chance-constraint tightening (cilqr_tighten_obstacles*, cilqr_chance_kappa, include/cilqr.h): every obstacle entry grown by kappa
standard deviations of the relative position along the ellipse's axes, from the Sigma_t of cilqr_chance_risk, and the round
solve -> gains -> chance risk -> tighten -> warm re-solve built from it.

Expected values never come from the HIP path: the oracle's solves and gains (_scene_r, _scene_l, o_gains of tests/test_rollout_risk.py,
lamb = 1), `restate` of tests/test_chance_risk.py for Sigma_t, `tighten_restate` below — a numpy restatement of the header's definition —
and math.erfc for kappa.  Tolerances are the suite's own: dim_out and the two delta fields |d| <= 1e-9 * max(1, max|value| of that
solve) (_close); pose_out bit-equal to the addressed poses; TG_MAX_ENTRY and TG_CAPPED exact.

What makes the exact comparisons meaningful is asserted on the restatement's numbers in test_conditions: float64 and numpy.longdouble
runs agree to 1e-11; per solve the two largest max(da, db) are more than 1e-6 apart; every uncapped kappa*sqrt(v) is more than 1e-6
from the cap; the capped case has capped and uncapped entries in every solve.  Scene L's two largest values come as close as 2e-5, which
still decides its entries.

  R0   scene R (B 8, N 12, M 3), Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2) shared, kappa = chance_kappa(0.05), no cap in reach
  RC   the same with max_inflate 0.32: some entries of every solve capped, some not
  RO   R0 with obs_cov[b, m, t] = ((0.05 (t+1))^2, 0.3 * 0.05 * 0.03 (t+1)^2, (0.03 (t+1))^2)
  RW   scene R with W = diag(1e-4, 1e-4, 4e-4, 1e-6) and Sigma_0 per solve (scaled by 1 + 0.1 b, x-y correlation 0.3)
  L0   scene L (B 6, N 50, M 4), the shared Sigma_0
  A    B 8, N 30, one static obstacle 12 m ahead of each ego and 1.0 + 0.4 b m to the side: the round itself (test_pipeline_scene_a)

The facade and the replay tool are checked against the C-ABI (the binding's) calls made by hand, bit for bit: tests/cpp/candidates_tightened.cpp
(run_candidates alone, under MinTotalCost, two rounds with obs_cov, composed with set_pose_covariance_check; run_step; the off switches; the
conflict with set_obstacle_samples) and test_replay_tool_tighten_option.

The kernel's LDS, 8*(6*N + 20) bytes, stays below 64 KiB up to N = 1362, beyond CILQR_MAX_HORIZON = 384: no horizon a handle accepts is
refused, so "the largest N that fits and CILQR_ERR_UNSUPPORTED one beyond" has no shape to run at; test_edges runs the largest horizon
a handle accepts and asserts from the formula that it fits.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import _bits, _expected
from test_chance_risk import SIGMA0, STEP_RISK, W_DIAG, _per_solve_sigma0, _straight, restate
from test_rollout_risk import _close, _scene_l, _scene_r, o_gains

gpu = pytest.mark.gpu

MARGIN = 1e-6
ERR_ARG = -1
ENTRY_POINTS = ("cilqr_tighten_obstacles", "cilqr_tighten_obstacles_device")
FIELDS = ("MAX_DA", "MAX_DB", "MAX_ENTRY", "CAPPED")
MAX_DA, MAX_DB, MAX_ENTRY, CAPPED = range(4)
NO_CAP, CAP = 2.0, 0.32
EPS = 0.05
_dp = C.POINTER(C.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def kappa_of(eps):
    """erfc(kappa / sqrt 2) / 2 = eps by bisection on math.erfc: the CPU side's own kappa."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(mid / math.sqrt(2.0)) > eps:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


KAPPA = kappa_of(EPS)


# ---- expected values: a numpy restatement of the header's definition ---------------------------------------------------------------
def tighten_restate(p, N, X, sigma, pose, dim, obs_cov, kappa, cap, T=np.float64):
    """X (B, 4(N+1)), sigma (B, N+1, 16) column-major, pose (B, M, 4N), dim (B, M, 2N) dense, obs_cov (B, M, N, 3) or None.
    Returns dict(dim (B, M, 2N), da, db (B, M, N) after the cap, raw_a, raw_b before it, capped (B, M, N) bool, tighten (B, 4)),
    float64 whatever T."""
    B, M = pose.shape[0], pose.shape[1]
    th = X.reshape(B, N + 1, 4)[:, :N, 3].astype(T)
    S = sigma.reshape(B, N + 1, 4, 4).transpose(0, 1, 3, 2)[:, :N].astype(T)  # [r][c] from entry (r, c) at [r + 4c]; r <= c read
    po, di = pose.reshape(B, M, N, 4).astype(T), dim.reshape(B, M, N, 2).astype(T)
    co, so = np.cos(po[..., 3]), np.sin(po[..., 3])
    oc = np.zeros((B, M, N, 3), dtype=T) if obs_cov is None else np.asarray(obs_cov).reshape(B, M, N, 3).astype(T)
    va, vb = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for lever in (T(p.ego_front), -T(p.ego_rear)):
            jx, jy = -lever * np.sin(th), lever * np.cos(th)
            cxx = S[:, :, 0, 0] + 2 * jx * S[:, :, 0, 3] + jx * jx * S[:, :, 3, 3]
            cyy = S[:, :, 1, 1] + 2 * jy * S[:, :, 1, 3] + jy * jy * S[:, :, 3, 3]
            cxy = S[:, :, 0, 1] + jx * S[:, :, 1, 3] + jy * S[:, :, 0, 3] + jx * jy * S[:, :, 3, 3]
            cxx, cyy, cxy = cxx[:, None] + oc[..., 0], cyy[:, None] + oc[..., 2], cxy[:, None] + oc[..., 1]
            va.append(co * co * cxx + 2 * co * so * cxy + so * so * cyy)
            vb.append(so * so * cxx - 2 * co * so * cxy + co * co * cyy)
        out = {}
        for name, (f, r) in (("a", va), ("b", vb)):
            v = np.fmax(f, r)  # a NaN loses to a number
            v = np.where(v < 0, T(0), v)  # (a NaN stays)
            raw = (T(kappa) * np.sqrt(v)).astype(np.float64)
            hit = ~np.isfinite(raw) | (raw > cap)
            out["raw_" + name], out["cap_" + name], out["d" + name] = raw, hit, np.where(hit, cap, raw)
    capped = out["cap_a"] | out["cap_b"]
    d = np.zeros((B, M, N, 2))
    d[..., 0], d[..., 1] = di[..., 0].astype(np.float64) + 2 * out["da"], di[..., 1].astype(np.float64) + 2 * out["db"]
    tg = np.zeros((B, 4))
    if M:
        big = np.maximum(out["da"], out["db"]).reshape(B, M * N)
        tg[:, MAX_DA], tg[:, MAX_DB] = out["da"].reshape(B, -1).max(axis=1), out["db"].reshape(B, -1).max(axis=1)
        tg[:, MAX_ENTRY], tg[:, CAPPED] = big.argmax(axis=1), capped.reshape(B, -1).sum(axis=1)  # argmax: the lowest index
    else:
        tg[:, MAX_ENTRY] = -1
    return dict(dim=d.reshape(B, M, 2 * N), da=out["da"], db=out["db"], raw_a=out["raw_a"], raw_b=out["raw_b"], capped=capped, tighten=tg,
                B=B, M=M, N=N)


def _obs_cov(B, M, N):
    t = np.arange(1, N + 1, dtype=np.float64)
    oc = np.zeros((B, M, N, 3))
    oc[..., 0], oc[..., 1], oc[..., 2] = (0.05 * t) ** 2, 0.3 * 0.05 * 0.03 * t * t, (0.03 * t) ** 2
    return oc


def _scene_a(O):
    """Scene A of the issue: the tightening has room to act."""
    from cilqr_amd import scenes
    B, N, M = 8, 30, 1
    p = O.default_params(N)
    sc = scenes.make_static(B, N, M, p, 7, local_plan=O.local_plan)
    pose, dim = sc["obs_pose"].reshape(B, M, N, 4).copy(), np.ascontiguousarray(sc["obs_dim"].reshape(B, M, 2 * N))
    for b in range(B):
        x, y, _, th = sc["x0"][b]
        lat = 1.0 + 0.4 * b
        pose[b, 0, :, :] = [x + 12.0 * np.cos(th) - lat * np.sin(th), y + 12.0 * np.sin(th) + lat * np.cos(th), 0.0, th]
    return dict(p=p, B=B, N=N, M=M, x0=sc["x0"], U0=sc["U"], poly=sc["poly"], fl=sc["xplan_fl"], pose=pose.reshape(B, M, 4 * N), dim=dim)


def _sigma(s, sigma0, W=None, T=np.float64):
    """Sigma_t of the scene's plan by the chance-risk restatement (obstacles play no part in the chain)."""
    return restate(s["p"], s["N"], s["X"], s["U"], s["K"], sigma0, None if W is None else W.T.reshape(16), None, None, T)["sigma"]


def _sigma_ld(s, sigma0, W=None):
    """The same chain carried in longdouble to its end (restate returns float64: the chain is repeated here at full width)."""
    T = np.longdouble
    B, N, p = s["B"], s["N"], s["p"]
    Xs, Us, Ks = s["X"].reshape(B, N + 1, 4).astype(T), s["U"].reshape(B, N, 2).astype(T), s["K"].reshape(B, N, 4, 2).astype(T)
    s0 = np.broadcast_to(np.asarray(sigma0).reshape(-1, 16), (B, 16))
    dt = T(p.timestep)
    out = np.zeros((B, N + 1, 16), dtype=T)
    sym = lambda a: np.triu(np.asarray(a, dtype=T).reshape(4, 4).T) + np.triu(np.asarray(a, dtype=T).reshape(4, 4).T, 1).T  # noqa: E731
    Wm = np.zeros((4, 4), dtype=T) if W is None else sym(W.T.reshape(16))
    for b in range(B):
        S = sym(s0[b])
        out[b, 0] = S.T.reshape(16)
        for t in range(N):
            v, th, a = Xs[b, t, 2], Xs[b, t, 3], Us[b, t, 0]
            adv = v * dt + a * dt * dt / 2
            A, Bm = np.eye(4, dtype=T), np.zeros((4, 2), dtype=T)
            A[0, 2], A[1, 2], A[0, 3], A[1, 3] = dt * np.cos(th), dt * np.sin(th), -np.sin(th) * adv, np.cos(th) * adv
            Bm[0, 0], Bm[1, 0], Bm[2, 0], Bm[3, 1] = dt * dt * np.cos(th) / 2, dt * dt * np.sin(th) / 2, dt, dt
            F = A + Bm @ Ks[b, t].T
            S2 = F @ S @ F.T + Wm
            S = np.triu(S2) + np.triu(S2, 1).T
            out[b, t + 1] = S.T.reshape(16)
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """Scenes R and L with the oracle's gains, the restated Sigma_t and the tightening's expected values.  Computed once; never modified."""
    O = oracle
    r, l = _scene_r(O), _scene_l(O)
    for s in (r, l):
        s["pose"], s["dim"] = np.ascontiguousarray(s["pose"]).reshape(s["B"], s["M"], -1), np.ascontiguousarray(s["dim"]).reshape(s["B"], s["M"], -1)
        _, s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
        assert np.all(ok == 1)
    s0 = SIGMA0.T.reshape(16)
    rw0 = np.nan_to_num(_per_solve_sigma0(r["B"]), nan=0.0)
    r["sigma"], r["sigma_w"], l["sigma"] = _sigma(r, s0), _sigma(r, rw0, W_DIAG), _sigma(l, s0)
    r["cov"] = _obs_cov(r["B"], r["M"], r["N"])
    want = lambda s, sig, cov, cap: tighten_restate(s["p"], s["N"], s["X"], sig, s["pose"], s["dim"], cov, KAPPA, cap)  # noqa: E731
    return {"R": r, "L": l, "sigma0": s0, "rw_sigma0": rw0,
            "R0": want(r, r["sigma"], None, NO_CAP), "RC": want(r, r["sigma"], None, CAP), "RO": want(r, r["sigma"], r["cov"], NO_CAP),
            "RW": want(r, r["sigma_w"], None, NO_CAP), "L0": want(l, l["sigma"], None, NO_CAP)}


def _max_c(O, s, X, U):
    """max over entries and circles of the oracle's constraint c against the scene's ORIGINAL obstacles, per solve."""
    _, c = _expected(O, s["p"], s["N"], X, U, s["poly"], s["fl"], s["pose"], s["dim"])
    return c.reshape(s["B"], -1).max(axis=1)


def _step_risk(O, s, X, U):
    """CR_STEP_RISK of a plan against the scene's original obstacles: the oracle's gains, the chance-risk restatement."""
    _, K, ok = o_gains(O, s["p"], s["N"], X, U, s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
    assert np.all(ok == 1)
    w = restate(s["p"], s["N"], X, U, K, SIGMA0.T.reshape(16), None, s["pose"], s["dim"])
    return w["risk"][:, STEP_RISK], K, w["sigma"]


@pytest.fixture(scope="module")
def round_a(oracle):
    """One tightening round on scene A, CPU side: oracle solve -> oracle gains -> restated Sigma_t -> restated tightening -> oracle
    re-solve from the first solve's U on the tightened table."""
    O = oracle
    s = _scene_a(O)
    th = min(8, O.max_threads())
    first = O.solve_batch(s["p"], s["N"], s["M"], s["x0"], s["U0"], s["poly"], s["fl"], s["pose"], s["dim"], None, threads=th)
    risk0, K, sigma = _step_risk(O, s, first["X"], first["U"])
    tg = tighten_restate(s["p"], s["N"], first["X"], sigma, s["pose"], s["dim"], None, KAPPA, NO_CAP)
    second = O.solve_batch(s["p"], s["N"], s["M"], s["x0"], first["U"], s["poly"], s["fl"], s["pose"], tg["dim"], None, threads=th)
    risk1, _, _ = _step_risk(O, s, second["X"], second["U"])
    return dict(s=s, first=first, K=K, sigma=sigma, tighten=tg, second=second, risk0=risk0, risk1=risk1,
                c0=_max_c(O, s, first["X"], first["U"]), c1=_max_c(O, s, second["X"], second["U"]))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert "cilqr_chance_kappa" in cilqr.ABI_SYMBOLS and hasattr(cilqr.lib(), "cilqr_chance_kappa")
    assert re.search(r"\bdouble\s+cilqr_chance_kappa\s*\(\s*double\s+eps\s*\)", h)
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_TIGHTEN_FIELDS\s+4\b", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_TG_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "TG_" + name) == i
    assert cilqr.TIGHTEN_FIELDS == 4
    assert callable(cilqr.Solver.tighten_obstacles) and callable(cilqr.Solver.tighten_obstacles_device) and callable(cilqr.chance_kappa)
    assert "8*(6*N + 20)" in full  # the LDS formula is stated
    assert "first order only" in full and "does not help" in full  # what the tightening is, and where it fails
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_chance_tightening\s*\(\s*const\s+double\s+Sigma0\[16\]\s*,\s*const\s+double\*\s+W\s*,\s*double\s+eps\s*,"
                     r"\s*int\s+rounds\s*=\s*1\s*,\s*double\s+max_inflate\s*=\s*2\.0\s*,\s*double\s+lamb\s*=\s*1\.0\s*\)", f)
    assert re.search(r"void\s+set_obstacle_covariance\s*\(\s*const\s+std::vector<double>&", f)
    assert re.search(r"std::vector<double>\s+last_tighten\s*,\s*last_tighten_risk_before\s*;", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_tighten_obstacles\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_tighten.hip" in mk and re.search(r"^check:.*build/cilqr_tighten\.o", mk, flags=re.M)


def test_argument_errors_need_no_device(cilqr):
    """NULL X, sigma, dim_out or tighten, obs NULL with M > 0, a negative stride, a kappa or max_inflate that is negative or not finite:
    CILQR_ERR_ARG, decided before the handle is looked at (there is none here)."""
    L = cilqr.lib()
    B, N, M = 2, 4, 1
    X, sig = np.zeros((B, 4 * (N + 1))), np.zeros((B, N + 1, 16))
    pose, dim, cov = np.zeros((B, M, 4 * N)), np.ones((B, M, 2 * N)), np.zeros((B, M, N, 3))
    po, do, tg = np.zeros((B, M, 4 * N)), np.zeros((B, M, 2 * N)), np.zeros((B, 4))
    no_handle = C.c_void_p()
    nan, inf = float("nan"), float("inf")

    def call(dev, kappa=1.0, cap=2.0, M_=M, obs="dense", obs_strides=(M * N, N, 1, 0), **nulls):
        a = dict(X=X, sigma=sig, dim_out=do, tighten=tg)
        a.update(nulls)
        o = cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, *obs_strides)
        f = L.cilqr_tighten_obstacles_device if dev else L.cilqr_tighten_obstacles
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, M_, _p(a["X"]), _p(a["sigma"]), C.byref(o) if obs else None, _p(cov), C.c_double(kappa), C.c_double(cap),
                 _p(po), _p(a["dim_out"]), _p(a["tighten"]))

    for dev in (False, True):
        for name in ("X", "sigma", "dim_out", "tighten"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, obs=None) == ERR_ARG and b"obs is null" in L.cilqr_last_error()
        for k in range(4):
            st = [M * N, N, 1, 0]
            st[k] = -1
            assert call(dev, obs_strides=tuple(st)) == ERR_ARG and b"negative stride" in L.cilqr_last_error(), k
        for bad in (-1.0, nan, inf, -inf):
            assert call(dev, kappa=bad) == ERR_ARG and b"kappa" in L.cilqr_last_error(), bad
            assert call(dev, cap=bad) == ERR_ARG and b"max_inflate" in L.cilqr_last_error(), bad
        assert call(dev, kappa=0.0, cap=0.0) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, M_=0, obs=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid too


def test_chance_kappa(cilqr):
    """erfc(kappa / sqrt 2) / 2 agrees with eps to 1e-13 relative; NaN outside (0, 0.5]; exactly 0 at 0.5; the same bits every time."""
    for eps in (0.5, 0.1, 0.05, 1e-3, 1e-9):
        k = cilqr.chance_kappa(eps)
        back = 0.5 * math.erfc(k / math.sqrt(2.0))
        print("eps %g: kappa %.17g, erfc(kappa / sqrt 2) / 2 = %.17g, relative error %.3g; bisection %.17g" % (
            eps, k, back, abs(back - eps) / eps, kappa_of(eps)))
        assert abs(back - eps) <= 1e-13 * eps, eps
        assert abs(k - kappa_of(eps)) <= 1e-12 * max(1.0, k)
        assert cilqr.chance_kappa(eps) == k
    assert cilqr.chance_kappa(0.5) == 0.0 and math.copysign(1.0, cilqr.chance_kappa(0.5)) == 1.0
    for bad in (0.0, -0.1, 0.5000001, 1.0, float("nan"), float("inf")):
        assert math.isnan(cilqr.chance_kappa(bad)), bad
    ks = [cilqr.chance_kappa(e) for e in (0.4, 0.2, 0.05, 1e-4, 1e-12, 1e-100)]
    assert all(a < b for a, b in zip(ks, ks[1:]))  # smaller eps, larger kappa
    assert abs(cilqr.chance_kappa(EPS) - KAPPA) <= 1e-12


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_tighten.cpp: plan_tighten_obstacles laid out without an arena against host_arena_bytes at the shapes
    include/cilqr.h says always fit; and host_arena_bytes is still what tests/golden/host_arena_cap.json recorded."""
    exe = str(tmp_path / "host_plan_tighten")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_tighten.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1200:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "8 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


def _top_gap(w):
    """Per solve: the distance between the two largest max(da, db)."""
    big = np.sort(np.maximum(w["da"], w["db"]).reshape(w["B"], -1), axis=1)
    return big[:, -1] - big[:, -2]


def test_conditions(cases):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the restatement's numbers alone."""
    r, l = cases["R"], cases["L"]
    assert np.longdouble(1) + np.finfo(np.longdouble).eps != 1 and np.finfo(np.longdouble).eps < 1e-18  # longdouble is wider here
    LD = np.longdouble
    runs = (("R0", r, cases["sigma0"], None, None, NO_CAP), ("RC", r, cases["sigma0"], None, None, CAP),
            ("RO", r, cases["sigma0"], None, r["cov"], NO_CAP), ("RW", r, cases["rw_sigma0"], W_DIAG, None, NO_CAP),
            ("L0", l, cases["sigma0"], None, None, NO_CAP))
    for name, s, sigma0, W, cov, cap in runs:
        a = cases[name]
        b = tighten_restate(s["p"], s["N"], s["X"], _sigma_ld(s, sigma0, W), s["pose"], s["dim"], cov, kappa_of(EPS), cap, LD)
        d = max(float(np.max(np.abs(a[n] - b[n]))) for n in ("dim", "da", "db", "raw_a", "raw_b"))
        gap = _top_gap(a)
        raw = np.concatenate([a["raw_a"].ravel(), a["raw_b"].ravel()])
        miss = float(np.min(np.abs(raw - cap)))
        print("%s: float64 vs longdouble %.3g; da %.4g-%.4g, db %.4g-%.4g; smallest top gap %.3g; capped per solve %s; nearest to the cap %.3g"
              % (name, d, a["da"].min(), a["da"].max(), a["db"].min(), a["db"].max(), gap.min(), a["tighten"][:, CAPPED].astype(int).tolist(), miss))
        assert d <= 1e-11, name
        assert np.array_equal(a["capped"], b["capped"]) and np.array_equal(a["tighten"][:, MAX_ENTRY], b["tighten"][:, MAX_ENTRY]), name
        assert miss > MARGIN, name
        if name == "RC":
            n = a["capped"].reshape(a["B"], -1).sum(axis=1)
            assert np.all(n > 0) and np.all(n < a["M"] * a["N"])  # capped and uncapped entries in every solve
            assert np.all(a["tighten"][:, [MAX_DA, MAX_DB]].max(axis=1) == CAP)
        else:
            assert gap.min() > MARGIN, name  # MAX_ENTRY is decided in every solve
            assert not a["capped"].any()
    # the cases differ from one another by more than the tolerance: obs_cov, W and the per-solve Sigma_0 are seen
    for name in ("RO", "RW"):
        assert np.min(np.abs(cases[name]["dim"] - cases["R0"]["dim"]).reshape(r["B"], -1).max(axis=1)[1:]) > 1e-3, name
    # kappa = 0 and Sigma = 0 leave the dimensions as they are
    for kappa, sig in ((0.0, r["sigma"]), (KAPPA, np.zeros_like(r["sigma"]))):
        w = tighten_restate(r["p"], r["N"], r["X"], sig, r["pose"], r["dim"], None, kappa, NO_CAP)
        assert np.array_equal(_bits(w["dim"]), _bits(r["dim"])) and not w["tighten"][:, [MAX_DA, MAX_DB, CAPPED]].any()


def test_scene_a_one_round_removes_the_contact(round_a):
    """The behaviour the loop exists for, on the oracle side alone (figures printed): before the round one candidate is in contact with
    CR_STEP_RISK > 0.05; after it every candidate has max c < -1e-3 and CR_STEP_RISK < 0.05 against the ORIGINAL obstacles; every
    such value is more than 1e-6 from its threshold."""
    a = round_a
    print("scene A before: max c %s\n  CR_STEP_RISK %s\nafter one round (kappa %.6f): max c %s\n  CR_STEP_RISK %s\n  iterations %s -> %s; da up to %.4f, db up to %.4f"
          % (np.round(a["c0"], 4).tolist(), a["risk0"].tolist(), KAPPA, np.round(a["c1"], 4).tolist(), a["risk1"].tolist(),
             a["first"]["iters"].tolist(), a["second"]["iters"].tolist(), a["tighten"]["tighten"][:, MAX_DA].max(), a["tighten"]["tighten"][:, MAX_DB].max()))
    hit = a["c0"] > 0
    assert hit.sum() >= 1 and np.all(a["risk0"][hit] > 0.05)
    assert np.all(a["c1"] < -1e-3) and np.all(a["risk1"] < 0.05)
    assert np.min(np.abs(a["c0"])) > MARGIN and np.min(np.abs(a["risk0"] - 0.05)) > MARGIN
    assert np.min(np.abs(a["c1"] + 1e-3)) > MARGIN and np.min(np.abs(a["risk1"] - 0.05)) > MARGIN
    assert not a["tighten"]["capped"].any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


FILL = -123.456


def _host(cilqr, solver, s, sigma, kappa=KAPPA, cap=NO_CAP, cov=None, sel=slice(None), obstacles="dense", want_pose=True):
    """The host form through ctypes.  obstacles: "dense", None, or (pose, dim, cov or None, M, (batch, obstacle, step) strides).
    Returns dict(dim, pose or None, tighten)."""
    N = s["N"]
    X, sigma = np.ascontiguousarray(s["X"][sel]), np.ascontiguousarray(sigma[sel])
    B = X.shape[0]
    if obstacles == "dense":
        pose, dim, M = np.ascontiguousarray(s["pose"][sel]), np.ascontiguousarray(s["dim"][sel]), s["M"]
        cov = None if cov is None else np.ascontiguousarray(cov[sel])
        st = (M * N, N, 1)
    elif obstacles is None:
        pose = dim = cov = None
        M, st = 0, (0, 0, 0)
    else:
        pose, dim, cov, M, st = obstacles
    o = None if M == 0 else cilqr.Obstacles(pose.ctypes.data, dim.ctypes.data, None, st[0], st[1], st[2], 0)
    out = dict(dim=np.full((B, M, 2 * N), FILL), pose=np.full((B, M, 4 * N), FILL) if want_pose else None, tighten=np.full((B, 4), FILL))
    cilqr._check(cilqr.lib().cilqr_tighten_obstacles(solver._h, B, N, M, _p(X), _p(sigma), None if o is None else C.byref(o), _p(cov),
                                                     C.c_double(kappa), C.c_double(cap), _p(out["pose"]), _p(out["dim"]), _p(out["tighten"])))
    return out


def _device(solver, s, sigma, kappa=KAPPA, cap=NO_CAP, cov=None):
    """The device form on torch buffers, dense obstacles."""
    import torch
    B, N, M = s["B"], s["N"], s["M"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    t = {n: up(s[n]) for n in ("X", "pose", "dim")}
    tsig, tcov = up(sigma), None if cov is None else up(cov)
    z = lambda *shape: torch.full(shape, FILL, dtype=torch.float64, device=dev)  # noqa: E731
    dim, pose, tg = z(B, M, 2 * N), z(B, M, 4 * N), z(B, 4)
    torch.cuda.synchronize(dev)
    solver.tighten_obstacles_device(stream, B, N, M, t["X"].data_ptr(), tsig.data_ptr(), t["pose"].data_ptr(), t["dim"].data_ptr(),
                                    (M * N, N, 1, 0), dim.data_ptr(), tg.data_ptr(), pose_out=pose.data_ptr(),
                                    obs_cov=0 if tcov is None else tcov.data_ptr(), kappa=kappa, max_inflate=cap)
    torch.cuda.synchronize(dev)
    return dict(dim=dim.cpu().numpy(), pose=pose.cpu().numpy(), tighten=tg.cpu().numpy())


def _same(a, b, sel_a=slice(None), sel_b=slice(None), names=("dim", "pose", "tighten")):
    for n in names:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
            continue
        if not np.array_equal(_bits(a[n][sel_a]), _bits(b[n][sel_b])):
            return False
    return True


def _check_against(got, want, pose, what, sel=slice(None)):
    B = want["tighten"][sel].shape[0]
    assert np.all(got["dim"] != FILL) and np.all(got["tighten"] != FILL), what  # everything was written
    _close(got["dim"].reshape(B, -1), want["dim"][sel].reshape(B, -1), what + ": dim_out")
    _close(got["tighten"][:, [MAX_DA, MAX_DB]], want["tighten"][sel][:, [MAX_DA, MAX_DB]], what + ": MAX_DA, MAX_DB")
    print("  MAX_ENTRY %s, CAPPED %s" % (got["tighten"][:, MAX_ENTRY].astype(int).tolist(), got["tighten"][:, CAPPED].astype(int).tolist()))
    assert np.array_equal(got["tighten"][:, [MAX_ENTRY, CAPPED]], want["tighten"][sel][:, [MAX_ENTRY, CAPPED]]), what
    if got["pose"] is not None:
        assert np.array_equal(_bits(got["pose"]), _bits(np.ascontiguousarray(pose[sel]))), what


@gpu
def test_scene_r_against_the_restatement(cilqr, solver, cases):
    """R0, RC, RO, RW: dim_out and the delta fields to tolerance, the entry and the count exactly, pose_out the bits of the poses."""
    r = cases["R"]
    assert abs(cilqr.chance_kappa(EPS) - KAPPA) <= 1e-12
    k = cilqr.chance_kappa(EPS)
    _check_against(_host(cilqr, solver, r, r["sigma"], kappa=k), cases["R0"], r["pose"], "R0")
    _check_against(_host(cilqr, solver, r, r["sigma"], kappa=k, cap=CAP), cases["RC"], r["pose"], "RC (cap 0.32)")
    _check_against(_host(cilqr, solver, r, r["sigma"], kappa=k, cov=r["cov"]), cases["RO"], r["pose"], "RO (obs_cov)")
    _check_against(_host(cilqr, solver, r, r["sigma_w"], kappa=k), cases["RW"], r["pose"], "RW (W, per-solve Sigma_0)")
    # sigma below the diagonal is never read
    low = r["sigma"].reshape(r["B"], r["N"] + 1, 4, 4).copy()  # [.., c, r]: entry (r, c) at [r + 4c]
    low[:, :, np.triu_indices(4, 1)[0], np.triu_indices(4, 1)[1]] = np.nan  # c < r: below the diagonal
    assert _same(_host(cilqr, solver, r, low.reshape(r["B"], r["N"] + 1, 16), kappa=k), _host(cilqr, solver, r, r["sigma"], kappa=k))


@gpu
def test_scene_l_the_workloads_horizon(cilqr, solver, cases):
    l = cases["L"]
    _check_against(_host(cilqr, solver, l, l["sigma"]), cases["L0"], l["pose"], "L0")


@gpu
def test_a_result_depends_on_its_own_solve_alone(cilqr, solver, cases):
    """Each solve of scene R alone (B = 1), a sub-batch and the batch reversed give the batch's bits in every output (cap and obs_cov on)."""
    r = cases["R"]
    B = r["B"]
    kw = dict(cap=CAP, cov=r["cov"])
    whole = _host(cilqr, solver, r, r["sigma_w"], **kw)
    assert 0 < whole["tighten"][:, CAPPED].min()
    for b in range(B):
        assert _same(_host(cilqr, solver, r, r["sigma_w"], sel=slice(b, b + 1), **kw), whole, sel_b=slice(b, b + 1)), b
    assert _same(_host(cilqr, solver, r, r["sigma_w"], sel=slice(2, 7), **kw), whole, sel_b=slice(2, 7))
    assert _same(_host(cilqr, solver, r, r["sigma_w"], sel=slice(None, None, -1), **kw), whole, sel_b=slice(None, None, -1))
    perm = np.array([5, 0, 7, 2, 1, 6, 3, 4])
    assert _same(_host(cilqr, solver, r, r["sigma_w"], sel=perm, **kw), whole, sel_b=perm)


@gpu
def test_strides_and_optional_outputs(cilqr, solver, cases):
    """One obstacle set shared by the batch (batch_stride 0), constant over the horizon (step_stride 0), and both, equal their dense
    expansion bit for bit, obs_cov addressed by the same entry index; pose_out NULL is accepted and changes nothing else."""
    r = cases["R"]
    B, N, M = r["B"], r["N"], r["M"]
    P, D, Cv = r["pose"].reshape(B, M, N, 4), r["dim"].reshape(B, M, N, 2), r["cov"]
    dense = lambda a, w: np.ascontiguousarray(np.broadcast_to(a, (B, M, N, w)))  # noqa: E731
    shapes = {
        "static, shared": (P[3, :, 0], D[3, :, 0], Cv[3, :, 0], (0, 1, 0), lambda a: a[None, :, None, :]),
        "static, per solve": (P[:, :, 0], D[:, :, 0], Cv[:, :, 0], (M, 1, 0), lambda a: a[:, :, None, :]),
        "moving, shared": (P[3], D[3], Cv[3], (0, N, 1), lambda a: a[None]),
    }
    for what, (pose, dim, cov, st, expand) in shapes.items():
        pose, dim, cov = (np.ascontiguousarray(a) for a in (pose, dim, cov))
        got = _host(cilqr, solver, r, r["sigma"], cap=CAP, obstacles=(pose, dim, cov, M, st))
        dp, dd, dc = dense(expand(pose), 4), dense(expand(dim), 2), dense(expand(cov), 3)
        full = _host(cilqr, solver, r, r["sigma"], cap=CAP, obstacles=(dp.reshape(B, M, -1), dd.reshape(B, M, -1), dc, M, (M * N, N, 1)))
        assert _same(got, full), what
        assert np.array_equal(_bits(got["pose"]), _bits(dp.reshape(B, M, -1))), what  # the dense table the re-solve needs
        want = tighten_restate(r["p"], N, r["X"], r["sigma"], dp.reshape(B, M, -1), dd.reshape(B, M, -1), dc, KAPPA, CAP)
        _check_against(got, want, dp.reshape(B, M, -1), what)
        no_cov = _host(cilqr, solver, r, r["sigma"], cap=CAP, obstacles=(pose, dim, None, M, st), want_pose=False)
        assert no_cov["pose"] is None
        assert _same(no_cov, _host(cilqr, solver, r, r["sigma"], cap=CAP, obstacles=(pose, dim, None, M, st)), names=("dim", "tighten")), what
    via_binding = solver.tighten_obstacles(N, r["X"], r["sigma"], P[3, :, 0], D[3, :, 0], Cv[3, :, 0], kappa=KAPPA, max_inflate=CAP)
    pose, dim, cov = (np.ascontiguousarray(a) for a in shapes["static, shared"][:3])
    assert _same(via_binding, _host(cilqr, solver, r, r["sigma"], cap=CAP, obstacles=(pose, dim, cov, M, (0, 1, 0))))


@gpu
def test_host_form_equals_device_form(cilqr, solver, cases):
    r = cases["R"]
    for sigma, cap, cov in ((r["sigma"], NO_CAP, None), (r["sigma_w"], CAP, r["cov"])):
        host = _host(cilqr, solver, r, sigma, cap=cap, cov=cov)
        assert _same(host, _device(solver, r, sigma, cap=cap, cov=cov))
        assert _same(host, solver.tighten_obstacles(r["N"], r["X"], sigma, r["pose"], r["dim"], cov, kappa=KAPPA, max_inflate=cap))


def _cut(s, sigma, N):
    """The first N steps of scene `s` and of its Sigma_t."""
    B, M, N0 = s["B"], s["M"], s["N"]
    out = dict(s)
    out.update(N=N, X=np.ascontiguousarray(s["X"][:, :4 * (N + 1)]),
               pose=np.ascontiguousarray(s["pose"].reshape(B, M, N0, 4)[:, :, :N].reshape(B, M, 4 * N)),
               dim=np.ascontiguousarray(s["dim"].reshape(B, M, N0, 2)[:, :, :N].reshape(B, M, 2 * N)))
    return out, np.ascontiguousarray(sigma[:, :N + 1])


@gpu
def test_edges(cilqr, oracle, solver, cases):
    """kappa = 0; Sigma = 0; a NaN in one Sigma_t; N = 1; M = 0; the largest horizon a handle accepts."""
    r = cases["R"]
    B, N, M = r["B"], r["N"], r["M"]
    for what, kappa, sigma in (("kappa = 0", 0.0, r["sigma"]), ("Sigma = 0", KAPPA, np.zeros_like(r["sigma"]))):
        got = _host(cilqr, solver, r, sigma, kappa=kappa, cap=CAP)
        assert np.array_equal(_bits(got["dim"]), _bits(r["dim"])), what
        assert np.array_equal(_bits(got["pose"]), _bits(r["pose"])), what
        assert not got["tighten"][:, [MAX_DA, MAX_DB, CAPPED]].any() and np.all(got["tighten"][:, MAX_ENTRY] == 0.0), what
    # a NaN in Sigma_5 of solve 2 caps the M entries of step 5 of that solve; the other solves keep their bits
    bad = r["sigma"].copy()
    bad[2, 5, 0] = np.nan
    clean, got = _host(cilqr, solver, r, r["sigma"]), _host(cilqr, solver, r, bad)
    want = tighten_restate(r["p"], N, r["X"], bad, r["pose"], r["dim"], None, KAPPA, NO_CAP)
    assert want["capped"][2, :, 5].all() and want["capped"].sum() == M and want["tighten"][2].tolist() == [NO_CAP, NO_CAP, 5.0, float(M)]
    _check_against(got, want, r["pose"], "a NaN in Sigma_5 of solve 2")
    others = np.setdiff1d(np.arange(B), [2])
    assert _same(got, clean, sel_a=others, sel_b=others)
    step5 = np.zeros((M, N, 2), dtype=bool)
    step5[:, 5] = True
    assert np.array_equal(_bits(got["dim"][2].reshape(M, N, 2)[~step5]), _bits(clean["dim"][2].reshape(M, N, 2)[~step5]))
    assert np.array_equal(got["dim"][2].reshape(M, N, 2)[:, 5], r["dim"][2].reshape(M, N, 2)[:, 5] + 2 * NO_CAP)
    zero = _host(cilqr, solver, r, bad, kappa=0.0)  # kappa = 0 does not hide it
    assert zero["tighten"][2].tolist() == [NO_CAP, NO_CAP, 5.0, float(M)] and not zero["tighten"][others].any()
    # N = 1
    one, sig1 = _cut(r, r["sigma"], 1)
    _check_against(_host(cilqr, solver, one, sig1), tighten_restate(r["p"], 1, one["X"], sig1, one["pose"], one["dim"], None, KAPPA, NO_CAP),
                   one["pose"], "scene R cut to N = 1")
    # M = 0: the fields alone
    got = _host(cilqr, solver, r, r["sigma"], obstacles=None)
    assert got["tighten"].tolist() == [[0.0, 0.0, -1.0, 0.0]] * B and got["dim"].shape == (B, 0, 2 * N)
    # the largest horizon a handle accepts: its LDS fits by the header's formula, as does every horizon up to 1362
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    Nmax = int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1))
    lds = lambda n: 8 * (6 * n + 20)  # noqa: E731
    assert lds(Nmax) <= lds(1362) <= 64 * 1024 < lds(1363)
    sv = cilqr.Solver(cilqr.default_params(Nmax), max_batch=2, max_horizon=Nmax, max_obstacles=4, device=0)
    try:
        s = _straight(Nmax, 2, 4, 3)
        s["p"] = oracle.default_params(Nmax)
        P = s["pose"].reshape(2, 4, Nmax, 4).copy()
        P[..., 3] = 0.3 * np.arange(1, 5)[None, :, None]  # one heading per obstacle: the largest inflation belongs to one of them
        s["pose"] = P.reshape(2, 4, 4 * Nmax)
        sig = restate(s["p"], Nmax, s["X"], s["U"], s["K"], cases["sigma0"], W_DIAG.T.reshape(16), None, None)["sigma"]
        got = _host(cilqr, sv, s, sig, sel=slice(0, 1), want_pose=False)
        want = tighten_restate(s["p"], Nmax, s["X"], sig, s["pose"], s["dim"], None, KAPPA, NO_CAP)
        assert _top_gap(want)[0] > MARGIN and not want["capped"].any()
        _check_against(got, want, s["pose"], "N = %d, M = 4" % Nmax, sel=slice(0, 1))
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers reserved at create" % ERR_ARG):
            _host(cilqr, sv, s, sig)  # B = max_batch with pose_out: beyond the arena; the handle stays usable
        assert _same(_host(cilqr, sv, s, sig, sel=slice(0, 1), want_pose=False), got)
    finally:
        sv.close()
    for sel, cut, obstacles, what in ((slice(None), 11, None, "B="), (slice(0, 4), 12, None, "N="), (slice(0, 4), 11, "dense", "M=")):
        sv = cilqr.Solver(cilqr.default_params(11), max_batch=7, max_horizon=11, max_obstacles=2, device=0)
        try:
            c, sig = _cut(r, r["sigma"], cut)
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: %s" % (ERR_ARG, what)):
                _host(cilqr, sv, c, sig, sel=sel, obstacles=obstacles)
        finally:
            sv.close()


@gpu
def test_pipeline_scene_a(cilqr, solver, round_a):
    """One round, every call in its device form on one stream: solve -> gains -> chance risk (sigma_out) -> tighten -> re-solve from the
    first solve's U on (pose_out, dim_out).  Against the same sequence on the oracle and the restatements: iteration counts and exits
    equal, max|dU| <= 1e-8 after the warm-started second solve (the bar of test_warm_start_second_tick)."""
    import torch
    a = round_a
    s = a["s"]
    B, N, M = s["B"], s["N"], s["M"]
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    zi = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
    x0, U, poly, fl, pose, dim, s0 = (up(v) for v in (s["x0"], s["U0"], s["poly"], s["fl"], s["pose"], s["dim"], SIGMA0.T.reshape(16)))
    X, J, it, ex = z(B, 4 * (N + 1)), z(B), zi(B), zi(B)
    k, K, ok = z(B, 2 * N), z(B, 8 * N), zi(B)
    risk, sig, tpose, tdim, tg = z(B, 6), z(B, N + 1, 16), z(B, M, 4 * N), z(B, M, 2 * N), z(B, 4)
    X2, J2, it2, ex2 = z(B, 4 * (N + 1)), z(B), zi(B), zi(B)
    strides = (M * N, N, 1, 0)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    torch.cuda.synchronize(dev)
    solver.solve_batch_obstacles_device(st, B, N, M, ptr(x0), ptr(U), ptr(poly), ptr(fl), ptr(pose), ptr(dim), 0, strides, ptr(X), ptr(J), ptr(it), ptr(ex))
    U1 = U.clone()
    solver.gains_batch_device(st, B, N, M, ptr(X), ptr(U), ptr(poly), ptr(fl), ptr(pose), ptr(dim), 0, strides, ptr(k), ptr(K), ptr(ok))
    solver.chance_risk_device(st, B, N, M, ptr(X), ptr(U), ptr(K), ptr(s0), 0, 0, ptr(pose), ptr(dim), strides, ptr(risk), sigma_out=ptr(sig))
    solver.tighten_obstacles_device(st, B, N, M, ptr(X), ptr(sig), ptr(pose), ptr(dim), strides, ptr(tdim), ptr(tg), pose_out=ptr(tpose),
                                    kappa=cilqr.chance_kappa(EPS), max_inflate=NO_CAP)
    solver.solve_batch_obstacles_device(st, B, N, M, ptr(x0), ptr(U), ptr(poly), ptr(fl), ptr(tpose), ptr(tdim), 0, strides, ptr(X2), ptr(J2), ptr(it2), ptr(ex2))
    torch.cuda.synchronize(dev)
    n = lambda t: t.cpu().numpy()  # noqa: E731
    d1, d2 = float(np.max(np.abs(n(U1) - a["first"]["U"]))), float(np.max(np.abs(n(U) - a["second"]["U"])))
    print("first solve max|dU| %.3g, iterations %s; after the round max|dU| %.3g, iterations %s (oracle %s); CR_STEP_RISK before %s"
          % (d1, n(it).tolist(), d2, n(it2).tolist(), a["second"]["iters"].tolist(), n(risk)[:, STEP_RISK].tolist()))
    assert np.array_equal(n(it), a["first"]["iters"]) and np.array_equal(n(ex), a["first"]["status"])
    assert np.all(n(ok) == 1)
    _close(n(sig).reshape(B, -1), a["sigma"].reshape(B, -1), "Sigma_t of the first plan")
    _close(n(tdim).reshape(B, -1), a["tighten"]["dim"].reshape(B, -1), "tightened dimensions")
    assert np.array_equal(_bits(n(tpose)), _bits(s["pose"]))
    _close(n(tg)[:, [MAX_DA, MAX_DB]], a["tighten"]["tighten"][:, [MAX_DA, MAX_DB]], "MAX_DA, MAX_DB")
    assert np.all(n(tg)[:, CAPPED] == 0.0)
    assert np.all(np.abs(n(risk)[:, STEP_RISK] - a["risk0"]) <= 1e-9)
    assert np.array_equal(n(it2), a["second"]["iters"]) and np.array_equal(n(ex2), a["second"]["status"])
    assert d2 <= 1e-8


@gpu
def test_cpp_facade_tightened_candidates(tmp_path):
    """tests/cpp/candidates_tightened.cpp: run_candidates under iLQR::set_chance_tightening returns the index, X_result, U_result,
    last_cost and last_tighten of the C-ABI sequence called by hand, bit for bit, alone and composed with set_pose_covariance_check;
    run_step likewise; rounds = 0 and a null Sigma0 switch it off; the conflict with set_obstacle_samples throws."""
    exe = str(tmp_path / "candidates_tightened")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_tightened.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("tightened pick ok", "composed pick ok", "run_step ok", "off switches ok", "conflicts throw ok"):
        assert line in r.stdout, r.stdout


@gpu
def test_replay_tool_tighten_option(cilqr, tmp_path):
    """bin/cilqr_replay --tighten eps,rounds: a tick with an obstacle ends with the tightening's fields and carries the plan of the
    binding's calls made by hand (solve, then twice gains -> chance risk -> tighten -> re-solve), bit for bit; a tick without
    obstacles has no such fields and starts from that plan's U."""
    exe = os.path.join(PKG, "bin", "cilqr_replay")
    assert os.path.exists(exe), "bin/cilqr_replay not built (make -C %s)" % PKG
    N, P, rounds = 30, 200, 2
    p = cilqr.default_params(N)
    path = np.stack([np.arange(float(P)), np.zeros(P)], axis=1)
    ego = np.array([0.0, 0.5, 5.0, 0.0])
    ob = (12.0, -1.0, 0.0, 0.0, 4.79, 2.16)
    lines = ["cilqr-replay 1", "horizon %d" % N, "path %d" % P] + ["%r %r" % (float(a), float(b)) for a, b in path]
    lines += ["tick", "ego " + " ".join(repr(float(v)) for v in ego), "obstacles 1", " ".join(repr(float(v)) for v in ob)]
    lines += ["tick", "ego " + " ".join(repr(float(v)) for v in ego), "obstacles 0"]
    log = tmp_path / "ticks.log"
    log.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(log), "--tighten", "%r,%d" % (EPS, rounds)], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()
    assert len(out) == 2
    sv = cilqr.Solver(p, max_batch=3, max_horizon=N, max_obstacles=1, device=0)
    try:
        coeffs, ref = cilqr.local_plan(p, path, ego)
        fl = np.array([ref[0, 0], ref[-1, 0]])
        pose, dim = np.array([ob[:4]]), np.array([ob[4:]])
        r = sv.solve_batch_obstacles(N, ego, cilqr.default_control_seq(N), coeffs, fl, pose, dim)
        first_U = r["U"].copy()
        for _ in range(rounds):
            g = sv.gains_batch(N, r["X"], r["U"], coeffs, fl, pose, dim, lamb=1.0)
            c = sv.chance_risk(N, r["X"], r["U"], g["K"], SIGMA0.T.reshape(16), None, pose, dim, want_entry_p=False)
            t = sv.tighten_obstacles(N, r["X"], c["sigma"], pose, dim, None, kappa=cilqr.chance_kappa(EPS), max_inflate=2.0)
            r = sv.solve_batch(N, ego, r["U"], coeffs, fl, t["pose"], t["dim"])
        second = sv.solve_batch(N, ego, r["U"], coeffs, fl)
    finally:
        sv.close()
    w = out[0].split()
    at = 11 + 4 * (N + 1) + 2 * N
    assert w[at] == "tighten" and len(w) == at + 6
    assert int(w[6]) == r["iters"][0] and int(w[7]) == r["status"][0] and float(w[8]) == r["J"][0]
    assert np.array_equal(np.array(w[10:10 + 4 * (N + 1)], dtype=float), r["X"][0])
    assert np.array_equal(np.array(w[11 + 4 * (N + 1):at], dtype=float), r["U"][0])
    assert not np.array_equal(r["U"], first_U)  # the rounds moved the plan
    assert [float(v) for v in w[at + 1:at + 5]] == t["tighten"][0].tolist() and float(w[at + 5]) == c["risk"][0, STEP_RISK]
    w = out[1].split()
    assert len(w) == at and "tighten" not in w
    assert np.array_equal(np.array(w[11 + 4 * (N + 1):], dtype=float), second["U"][0])
