"""Analytic chance risk against sampled obstacles in compact form (cilqr_chance_risk_sampled*, include/cilqr.h): per entry the chance
value of cilqr_chance_risk on the materialised sample, per (obstacle, step) the mean over the obstacle's samples, per step the sum
over the obstacles, and the eight fields.

Expected values never come from the HIP path: `restate` of tests/test_chance_risk.py applied to the MATERIALISED obstacles
(scenes.materialise_samples) on the oracle's trajectories and gains (`_scene` of tests/test_risk_sampled.py, lamb = 1), Sigma_0 =
diag(0.16^2, 0.16^2, 0, 0.017^2), no W; then q = mean over j, r_t, the nominal share from the sign of the restatement's cbar, and the
fields by numpy (`_fields`).  The Sigma handed to the call is the restatement's own, except where a test says otherwise.
Tolerances are those of tests/test_chance_risk.py: entry_p, pair_p, step_risk and the four probability fields 1e-9 absolute, entry_p
also 1e-9 relative where the expected p >= 1e-150; steps, pairs and entries exact for the solves whose two largest values are more
than 1e-6 apart (printed); CRS_NOMINAL_SHARE exact; total bit-equal to base, or NaN.

  S, T, V   the scenes of tests/test_risk_sampled.py: B 6, 2 x 8;  B 3, 3 x 32;  B 2, 3 x 5 (N = 12).  Only obstacle 0 is near.
  S_N1, S_N10, S_1x2   cuts of scene S: one step (a single wavefront), ten steps (a partial last workgroup), one obstacle with two
            samples (the smallest n_obs and n_samples)
  X         scene S with obstacle 1 mirrored to the ego's other side, re-solved by the oracle: two obstacles each add more than 1e-3
            to r_t at the worst step (asserted), so the sum over the obstacles is exercised
  C3        the config-3 shape: scenes.make_c3, B 2, 8 x 32, N = 50 (256 materialised obstacles: cilqr_chance_risk cannot run it)
  W         synthetic plans, 3 x 70 and 1 x 2048 samples, N = 2: more than 64 samples per obstacle (a lane adds several), and the
            largest scene the kernel's LDS, 32*n_obs*n_samples bytes, admits; 1 x 2049 is CILQR_ERR_UNSUPPORTED.

Index products beyond 2^31 - 1 (n_obs*n_samples*N, B*ceil(N/4)) cannot be reached below CILQR_MAX_HORIZON = 384 and the 2^20 entries
a sampled call accepts: those two checks are not exercised.
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
from test_chance_risk import SIGMA0, restate
from test_risk_sampled import SCENES, _scene
from test_rollout_risk import _pick, o_gains

gpu = pytest.mark.gpu

TOL, MARGIN = 1e-9, 1e-6
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_chance_risk_sampled", "cilqr_chance_risk_sampled_device")
FIELDS = ("STEP_RISK", "WORST_STEP", "SUM_RISK", "MAX_PAIR_P", "MAX_PAIR", "MAX_ENTRY_P", "MAX_ENTRY", "NOMINAL_SHARE")
STEP_RISK, WORST_STEP, SUM_RISK, MAX_PAIR_P, MAX_PAIR, MAX_ENTRY_P, MAX_ENTRY, NOMINAL_SHARE = range(8)
PROB = [STEP_RISK, SUM_RISK, MAX_PAIR_P, MAX_ENTRY_P]
BOUND_SUM = 1
S0 = SIGMA0.T.reshape(16)
SIX = [0, 4, 12, 5, 13, 15]  # (0,0), (0,1), (0,3), (1,1), (1,3), (3,3) at [r + 4c]
_dp = C.POINTER(C.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


# ---- expected values --------------------------------------------------------------------------------------------------------------
def _fields(entry_p, hit, n_obs, ns, lost):
    """entry_p (B, M, N) and hit (B, M, N) bool, m = o*ns + j; lost (B, N) bool -> pair_p, step_risk, nominal counts and risk by numpy."""
    B, M, N = entry_p.shape
    with np.errstate(invalid="ignore"):
        q = entry_p.reshape(B, n_obs, ns, N).mean(axis=2)
        r = np.where(lost, 1.0, np.fmin(1.0, q.sum(axis=1)))
    k = hit.reshape(B, n_obs, ns, N).sum(axis=2)
    risk = np.zeros((B, 8))
    risk[:, STEP_RISK], risk[:, WORST_STEP] = r.max(axis=1), r.argmax(axis=1)
    risk[:, SUM_RISK] = np.minimum(1.0, r.sum(axis=1))
    for v, fv, fi in ((q.reshape(B, -1), MAX_PAIR_P, MAX_PAIR), (entry_p.reshape(B, -1), MAX_ENTRY_P, MAX_ENTRY)):
        e = np.where(np.isnan(v), -np.inf, v)  # a NaN never wins
        risk[:, fv], risk[:, fi] = e.max(axis=1), e.argmax(axis=1)
    risk[:, NOMINAL_SHARE] = k.max(axis=(1, 2)) / ns
    return dict(entry_p=entry_p, pair_p=q, step_risk=r, k=k, risk=risk)


def _want(s, sigma0=S0, T=np.float64):
    """The restatement on scene `s` (a dict with p, N, X, U, K, the materialised pose / dim, n_obs, ns)."""
    B, N, n_obs, ns = s["X"].shape[0], s["N"], s["n_obs"], s["ns"]
    w = restate(s["p"], N, s["X"], s["U"], s["K"], sigma0, None, s["pose"], s["dim"], T)
    X = s["X"].reshape(B, N + 1, 4)
    lost = ~(np.isfinite(X[:, :N][:, :, [0, 1, 3]]).all(axis=2) & np.isfinite(w["sigma"][:, :N][:, :, SIX]).all(axis=2))
    with np.errstate(invalid="ignore"):
        hit = w["cbar"].max(axis=3) > 0
    out = _fields(w["entry_p"].reshape(B, n_obs * ns, N), hit, n_obs, ns, lost)
    out.update(sigma=w["sigma"], cbar=w["cbar"], B=B)
    return out


def _gaps(want):
    """Per solve: the gap between the two largest r_t, q and p (inf where there is only one)."""
    def gap(v):
        v = v.reshape(v.shape[0], -1)
        if v.shape[1] < 2:
            return np.full(v.shape[0], np.inf)
        s = np.sort(np.where(np.isnan(v), -np.inf, v), axis=1)
        return s[:, -1] - s[:, -2]
    return gap(want["step_risk"]), gap(want["pair_p"]), gap(want["entry_p"])


def _total(risk, base, max_risk, sum_bound=False):
    field = risk[:, SUM_RISK if sum_bound else STEP_RISK]
    return np.where((field > max_risk) | ~np.isfinite(base), np.nan, base)


def _cut(s, N=None, n_obs=None, ns=None):
    """The first N steps, the first n_obs obstacles and the first ns samples of each of scene `s`."""
    B, N0, o0, j0 = s["X"].shape[0], s["N"], s["n_obs"], s["ns"]
    N, n_obs, ns = N or N0, n_obs or o0, ns or j0
    out = dict(s)
    out.update(N=N, n_obs=n_obs, ns=ns, X=np.ascontiguousarray(s["X"][:, :4 * (N + 1)]), U=np.ascontiguousarray(s["U"][:, :2 * N]),
               K=np.ascontiguousarray(s["K"][:, :8 * N]),
               nom_pose=np.ascontiguousarray(s["nom_pose"].reshape(B, o0, N0, 4)[:, :n_obs, :N].reshape(B, n_obs, 4 * N)),
               nom_dim=np.ascontiguousarray(s["nom_dim"].reshape(B, o0, N0, 2)[:, :n_obs, :N].reshape(B, n_obs, 2 * N)),
               off=np.ascontiguousarray(s["off"][:, :n_obs, :ns]),
               pose=np.ascontiguousarray(s["pose"].reshape(B, o0, j0, N0, 4)[:, :n_obs, :ns, :N].reshape(B, n_obs * ns, 4 * N)),
               dim=np.ascontiguousarray(s["dim"].reshape(B, o0, j0, N0, 2)[:, :n_obs, :ns, :N].reshape(B, n_obs * ns, 2 * N)))
    return out


def _solved(O, p, N, sc, nom_pose, nom_dim, off):
    """A compact scene solved by the oracle on its materialised obstacles, with the oracle's gains at lamb 1."""
    from cilqr_amd import scenes
    B, n_obs, ns = off.shape[:3]
    pose, dim, w = scenes.materialise_samples(nom_pose, nom_dim, off, N)
    pose, dim = np.ascontiguousarray(pose), np.ascontiguousarray(dim)
    r = O.solve_batch(p, N, n_obs * ns, sc["x0"], sc["U"], sc["poly"], sc["xplan_fl"], pose, dim, w, threads=min(8, O.max_threads()))
    _, K, ok = o_gains(O, p, N, r["X"], r["U"], sc["poly"], sc["xplan_fl"], pose, dim, w, 1.0)
    assert np.all(ok == 1)
    return dict(p=p, N=N, n_obs=n_obs, ns=ns, X=r["X"], U=r["U"], K=K, poly=sc["poly"], fl=sc["xplan_fl"], pose=pose, dim=dim,
                nom_pose=np.ascontiguousarray(nom_pose), nom_dim=np.ascontiguousarray(nom_dim), off=np.ascontiguousarray(off), weight=1.0 / ns)


def _scene_x(O):
    """Scene S with obstacle 1 mirrored to the other side: the construction of tests/test_risk_sampled.py's `_scene`, obstacle 1 on
    the ego's right at the lateral distance obstacle 0 has on its left."""
    from cilqr_amd import scenes
    B, n_obs, ns, _, lat0, oseed, _ = SCENES["S"]
    N = 12
    p = O.default_params(N)
    sc = scenes.make_static(B, N, n_obs, p, 7, local_plan=O.local_plan)
    nom = sc["obs_pose"].reshape(B, n_obs, N, 4).copy()
    t = np.arange(N) * p.timestep
    for b in range(B):
        x, y, _, th = sc["x0"][b]
        for o, side in ((0, 1.0), (1, -1.0)):
            lat = side * (lat0 + 0.1 * b)
            nom[b, o, :, 0] = x + 1.0 * np.cos(th) - lat * np.sin(th) + (1.5 * np.cos(th)) * t
            nom[b, o, :, 1] = y + 1.0 * np.sin(th) + lat * np.cos(th) + (1.5 * np.sin(th)) * t
            nom[b, o, :, 2], nom[b, o, :, 3] = 1.5, th
    off = np.random.Generator(np.random.PCG64(oseed)).normal(0.0, 1.0, (B, n_obs, ns, 3)) * scenes.POSE_SIGMA
    return _solved(O, p, N, sc, nom.reshape(B, n_obs, 4 * N), sc["obs_dim"].reshape(B, n_obs, 2 * N), off)


def _scene_c3(O):
    from cilqr_amd import scenes
    p = O.default_params(50)
    sc = scenes.make_c3(B=2, params=p, local_plan=O.local_plan)
    return _solved(O, p, 50, sc, sc["nom_pose"], sc["nom_dim"], sc["offsets"])


def _scene_w(O, n_obs, ns, seed, B=2, N=2):
    """Synthetic: B plans of N steps along x at 2 m/s, zero gains; obstacles beside the plan, their samples spread by 0.3 m."""
    from cilqr_amd import scenes
    rng = np.random.Generator(np.random.PCG64(seed))
    X = np.zeros((B, N + 1, 4))
    X[:, :, 0], X[:, :, 2], X[:, :, 3] = 0.2 * np.arange(N + 1), 2.0, (0.01 * (1 + np.arange(B)) * np.where(np.arange(B) % 2, -1.0, 1.0))[:, None]
    nom_pose = np.zeros((B, n_obs, N, 4))
    nom_pose[..., 0] = rng.uniform(0.0, 3.0, (B, n_obs, 1))
    nom_pose[..., 1] = rng.uniform(3.2, 3.8, (B, n_obs, 1)) * np.where(np.arange(n_obs) % 2, -1.0, 1.0)[None, :, None]
    nom_pose[..., 2], nom_pose[..., 3] = 1.0, rng.uniform(-0.3, 0.3, (B, n_obs, 1))
    nom_dim = np.ones((B, n_obs, N, 2)) * [4.0, 2.0]
    off = rng.normal(0.0, 1.0, (B, n_obs, ns, 3)) * [0.3, 0.3, 0.05]
    nom_pose, nom_dim = nom_pose.reshape(B, n_obs, 4 * N), nom_dim.reshape(B, n_obs, 2 * N)
    pose, dim, _ = scenes.materialise_samples(nom_pose, nom_dim, off, N)
    return dict(p=O.default_params(N), N=N, n_obs=n_obs, ns=ns, X=X.reshape(B, -1), U=np.zeros((B, 2 * N)), K=np.zeros((B, 8 * N)),
                pose=np.ascontiguousarray(pose), dim=np.ascontiguousarray(dim), nom_pose=nom_pose, nom_dim=nom_dim, off=off)


@pytest.fixture(scope="module")
def cases(oracle):
    """Every scene with the restatement's numbers.  Computed once; never modified."""
    sc = {name: _scene(oracle, name) for name in SCENES}
    sc["X"] = _scene_x(oracle)
    sc["C3"] = _scene_c3(oracle)
    sc["S_N1"], sc["S_N10"], sc["S_1x2"] = _cut(sc["S"], N=1), _cut(sc["S"], N=10), _cut(sc["S"], n_obs=1, ns=2)
    sc["W70"], sc["W2048"] = _scene_w(oracle, 3, 70, 21), _scene_w(oracle, 1, 2048, 22)
    want = {name: _want(s) for name, s in sc.items()}
    want["S_zero"] = _want(sc["S"], np.zeros(16))
    return dict(scenes=sc, want=want)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_CRS_FIELDS\s+8\b", h)
    assert re.search(r"#define\s+CILQR_CHANCE_SAMPLED_BOUND_SUM\s+1u\b", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_CRS_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "CRS_" + name) == i
    assert cilqr.CRS_FIELDS == 8 and cilqr.CHANCE_SAMPLED_BOUND_SUM == 1
    assert callable(cilqr.Solver.chance_risk_sampled) and callable(cilqr.Solver.chance_risk_sampled_device)
    assert "32*n_obs*n_samples bytes" in full  # the LDS formula is stated
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_sample_covariance_check\s*\(\s*const\s+double\s+Sigma0\[16\]\s*,\s*const\s+double\*\s+W\s*,\s*double\s+max_risk\s*,"
                     r"\s*double\s+lamb\s*=\s*1\.0\s*,\s*bool\s+sum_bound\s*=\s*false\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_chance_risk_sampled\s*;", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_chance_sampled\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_chance_sampled.hip" in mk and re.search(r"^check:.*build/cilqr_chance_sampled\.o", mk, flags=re.M)
    assert re.search(r"check_kernel_resources\.py --map.*build/cilqr_chance_sampled\.o", mk)


def test_argument_errors_need_no_device(cilqr):
    """NULL X, sigma, nominal table, sample offset or risk, total without base, n_obs < 1, n_samples < 2, a NaN max_risk, unknown flag
    bits: CILQR_ERR_ARG, decided before the handle is looked at (there is none here)."""
    L = cilqr.lib()
    B, N, n_obs, ns = 2, 4, 2, 3
    a0 = dict(X=np.zeros((B, 4 * (N + 1))), sigma=np.zeros((B, N + 1, 16)), nom_pose=np.zeros((B, n_obs, 4 * N)),
              nom_dim=np.ones((B, n_obs, 2 * N)), off=np.zeros((B, n_obs, ns, 3)), risk=np.zeros((B, 8)), base=np.zeros(B), total=np.zeros(B))
    step, pair, ep = np.zeros((B, N)), np.zeros((B, n_obs, N)), np.zeros((B, n_obs * ns, N))
    no_handle = C.c_void_p()

    def call(dev, flags=0, mr=1.0, n_obs_=n_obs, ns_=ns, **nulls):
        a = dict(a0)
        a.update(nulls)
        f = L.cilqr_chance_risk_sampled_device if dev else L.cilqr_chance_risk_sampled
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, n_obs_, ns_, _p(a["X"]), _p(a["sigma"]), _p(a["nom_pose"]), _p(a["nom_dim"]), _p(a["off"]), C.c_uint32(flags),
                 C.c_double(mr), _p(a["base"]), _p(a["risk"]), _p(step), _p(pair), _p(ep), _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "sigma", "nom_pose", "nom_dim", "off", "risk"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert call(dev, n_obs_=0) == ERR_ARG and b"n_obs >= 1 and n_samples >= 2" in L.cilqr_last_error()
        assert call(dev, ns_=1) == ERR_ARG and b"n_obs >= 1 and n_samples >= 2" in L.cilqr_last_error()
        assert call(dev, mr=float("nan")) == ERR_ARG and b"NaN" in L.cilqr_last_error()
        assert call(dev, flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev, flags=1) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid too


def test_conditions(oracle, cases):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the restatement's numbers alone."""
    sc, want = cases["scenes"], cases["want"]
    assert np.longdouble(1) + np.finfo(np.longdouble).eps != 1 and np.finfo(np.longdouble).eps < 1e-18  # longdouble is wider here
    for name in ("S", "T", "V", "X"):
        a, b = want[name], _want(sc[name], S0, np.longdouble)
        d = [float(np.max(np.abs(a[n] - b[n]))) for n in ("entry_p", "pair_p", "step_risk")] + [float(np.max(np.abs(a["risk"][:, PROB] - b["risk"][:, PROB])))]
        print("%s, float64 vs longdouble: entry_p %.3g, pair_p %.3g, step_risk %.3g, fields %.3g" % ((name,) + tuple(d)))
        assert max(d) <= 1e-11 and np.array_equal(a["k"], b["k"]), name
    for name, w in want.items():
        gr, gq, gp = _gaps(w)
        print("%s: max_t r_t %s; worst steps %s; smallest top-two gaps r_t %.3g, q %.3g, p %.3g; excluded from WORST_STEP %s, MAX_PAIR %s, MAX_ENTRY %s" % (
            name, np.round(w["risk"][:, STEP_RISK], 5).tolist(), w["risk"][:, WORST_STEP].astype(int).tolist(), gr.min(), gq.min(), gp.min(),
            np.nonzero(~(gr > MARGIN))[0].tolist(), np.nonzero(~(gq > MARGIN))[0].tolist(), np.nonzero(~(gp > MARGIN))[0].tolist()))
        if name in ("S", "T", "V"):
            assert gr.min() > MARGIN, name  # none is excluded on r_t
    # the figures the scenes were chosen by
    assert np.round(want["S"]["risk"][:, STEP_RISK], 5).tolist() == [0.45549, 0.06325, 0.24824, 0.05187, 0.00084, 0.04759]
    assert want["S"]["risk"][:, WORST_STEP].tolist() == [0, 8, 8, 7, 8, 9]
    assert np.round(want["T"]["risk"][:, STEP_RISK], 5).tolist() == [0.42357, 0.16345, 0.15123] and want["T"]["risk"][:, WORST_STEP].tolist() == [0, 8, 8]
    assert np.round(want["V"]["risk"][:, STEP_RISK], 5).tolist() == [0.17647, 0.07376] and want["V"]["risk"][:, WORST_STEP].tolist() == [7, 8]
    # thresholds: each candidate's value -/+ 1e-6 (decided by the 1e-9 the values agree to) is more than 1e-6 from every OTHER
    # candidate's value; 0.1 on STEP_RISK and on SUM_RISK is more than 1e-6 from every value and separates the candidates
    for name in ("S", "X"):
        r, total = want[name]["risk"][:, STEP_RISK], want[name]["risk"][:, SUM_RISK]
        d = np.abs(r[:, None] - r[None, :]) + np.eye(len(r))
        assert d.min() > 2 * MARGIN and r.min() > 2 * MARGIN, name
        assert np.min(np.abs(r - 0.1)) > MARGIN and np.min(np.abs(total - 0.1)) > MARGIN
    r, total = want["S"]["risk"][:, STEP_RISK], want["S"]["risk"][:, SUM_RISK]
    assert 0 < (r > 0.1).sum() < len(r) and (total > 0.1).sum() > (r > 0.1).sum()
    # scene X: two obstacles each add more than 1e-3 to r_t at the worst step
    w = want["X"]
    at = w["risk"][:, WORST_STEP].astype(int)
    both = np.array([w["pair_p"][b, :, at[b]] for b in range(w["B"])])
    print("scene X: q(o, worst step) per solve %s" % np.round(both, 5).tolist())
    assert both.shape[1] == 2 and (both > 1e-3).all(axis=1).any(), both
    x_two = np.nonzero((both > 1e-3).all(axis=1))[0]
    assert len(x_two) >= 2, both
    # in S only obstacle 0 is near
    assert want["S"]["pair_p"][:, 1].max() < 1e-3
    # Sigma_0 = 0: every cbar is decided in sign by more than 1e-6, some samples are in contact, and q is the integer share exactly
    z = want["S_zero"]
    assert np.min(np.abs(z["cbar"])) > MARGIN and z["k"].max() > 0 and not z["sigma"].any()
    assert np.array_equal(z["pair_p"], z["k"] / sc["S"]["ns"])


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_chance_sampled.cpp: plan_chance_sampled's arrays, offsets and contiguous in / out ranges over a grid of small
    shapes; the header's "always fits" bounds against host_arena_bytes, which is still what tests/golden/host_arena_cap.json recorded."""
    exe = str(tmp_path / "host_plan_chance_sampled")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_chance_sampled.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "layout ok" in r.stdout and "every shape fits" in r.stdout and "11 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=16, max_horizon=50, max_obstacles=256, device=0)
    yield s
    s.close()


OUTPUTS = ("step_risk", "pair_p", "entry_p", "total")


def _host(solver, s, sigma, sel=slice(None), max_risk=1.0, base=None, sum_bound=False, skip=()):
    """The host form through the binding; `skip`: optional outputs left out."""
    g = lambda a: np.ascontiguousarray(a[sel])  # noqa: E731
    return solver.chance_risk_sampled(s["N"], g(s["X"]), g(sigma), g(s["nom_pose"]), g(s["nom_dim"]), g(s["off"]), max_risk=max_risk,
                                      base=None if base is None else g(np.asarray(base, dtype=np.float64)), sum_bound=sum_bound,
                                      want_steps="step_risk" not in skip, want_pair_p="pair_p" not in skip, want_entry_p="entry_p" not in skip)


def _device(solver, s, sigma, max_risk=1.0, base=None, flags=0):
    """The device form on torch buffers."""
    import torch
    B, N, n_obs, ns = s["X"].shape[0], s["N"], s["n_obs"], s["ns"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
    t = {n: up(s[n]) for n in ("X", "nom_pose", "nom_dim", "off")}
    ts, tb = up(sigma), None if base is None else up(base)
    z = lambda *shape: torch.full(shape, -123.456, dtype=torch.float64, device=dev)  # noqa: E731
    risk, step, pair, ep, total = z(B, 8), z(B, N), z(B, n_obs, N), z(B, n_obs * ns, N), z(B)
    torch.cuda.synchronize(dev)
    solver.chance_risk_sampled_device(stream, B, N, n_obs, ns, t["X"].data_ptr(), ts.data_ptr(), t["nom_pose"].data_ptr(),
                                      t["nom_dim"].data_ptr(), t["off"].data_ptr(), risk.data_ptr(), step.data_ptr(), pair.data_ptr(),
                                      ep.data_ptr(), total.data_ptr() if tb is not None else 0, tb.data_ptr() if tb is not None else 0,
                                      max_risk=max_risk, flags=flags)
    torch.cuda.synchronize(dev)
    out = {k: v.cpu().numpy() for k, v in dict(risk=risk, step_risk=step, pair_p=pair, entry_p=ep, total=total).items()}
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
    """Values to tolerance for every solve; steps, pairs and entries exact for the solves whose maxima are decided (printed)."""
    w = {n: want[n][sel] for n in ("entry_p", "pair_p", "step_risk", "risk")}
    dp, dq, dr = (np.abs(got[n] - w[n]) for n in ("entry_p", "pair_p", "step_risk"))
    big = w["entry_p"] >= 1e-150
    rel = float(np.max(dp[big] / w["entry_p"][big])) if big.any() else 0.0
    df = np.abs(got["risk"][:, PROB] - w["risk"][:, PROB])
    print("%s: entry_p max |d| %.3g abs, %.3g rel over %d entries >= 1e-150; pair_p %.3g; step_risk %.3g; STEP, SUM, MAX_PAIR_P, MAX_ENTRY_P %s" % (
        what, float(np.nanmax(dp)), rel, int(big.sum()), float(np.nanmax(dq)), float(dr.max()), df.max(axis=0).tolist()))
    assert np.array_equal(np.isnan(got["entry_p"]), np.isnan(w["entry_p"])) and np.array_equal(np.isnan(got["pair_p"]), np.isnan(w["pair_p"])), what
    assert np.all(dp[~np.isnan(dp)] <= TOL) and rel <= TOL and np.all(dq[~np.isnan(dq)] <= TOL) and np.all(dr <= TOL) and np.all(df <= TOL), what
    assert np.array_equal(got["risk"][:, NOMINAL_SHARE], w["risk"][:, NOMINAL_SHARE]), what
    gr, gq, gp = (g > MARGIN for g in _gaps(w))
    print("  WORST_STEP compared for solves %s, MAX_PAIR for %s, MAX_ENTRY for %s" % tuple(np.nonzero(g)[0].tolist() for g in (gr, gq, gp)))
    for keep, f in ((gr, WORST_STEP), (gq, MAX_PAIR), (gp, MAX_ENTRY)):
        assert np.array_equal(got["risk"][keep, f], w["risk"][keep, f]), (what, FIELDS[f], got["risk"][:, f], w["risk"][:, f])
    return gr, gq, gp


def _check_total(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(_bits(got[~np.isnan(want)]), _bits(want[~np.isnan(want)])), what


@gpu
@pytest.mark.parametrize("name", ["S", "T", "V", "X", "S_N1", "S_N10", "S_1x2", "C3", "W70"])
def test_values_against_the_restatement(solver, cases, name):
    """Every output against the restatement; total bit-equal to base, or NaN."""
    s, want = cases["scenes"][name], cases["want"][name]
    B = want["B"]
    base = np.linspace(3.0, 2.0, B)
    got = _host(solver, s, want["sigma"], max_risk=0.1, base=base)
    gr, _, _ = _check_against(got, want, name)
    if name in ("S", "T", "V"):
        assert gr.all()
    _check_total(got["total"], _total(want["risk"], base, 0.1), name)


@gpu
@pytest.mark.parametrize("name", ["S", "V"])
def test_entry_p_is_the_materialised_calls_bit_for_bit(solver, cases, name):
    """cilqr_chance_risk on the materialised obstacles and this call on the compact form, both under that call's sigma_out — which the
    M = 0 call reproduces bit for bit: the chain reads no obstacle — give the same entry_p bits."""
    s = cases["scenes"][name]
    B, N, M = s["X"].shape[0], s["N"], s["n_obs"] * s["ns"]
    mat = solver.chance_risk(N, s["X"], s["U"], s["K"], S0, None, s["pose"], s["dim"])
    m0 = solver.chance_risk(N, s["X"], s["U"], s["K"], S0)
    assert np.array_equal(_bits(mat["sigma"]), _bits(m0["sigma"]))
    got = _host(solver, s, m0["sigma"])
    assert got["entry_p"].shape == (B, M, N) and np.any(got["entry_p"] > 0) and np.any(got["entry_p"] < 1)
    assert np.array_equal(_bits(got["entry_p"].reshape(B, M * N)), _bits(mat["entry_p"]))


@gpu
def test_sigma_zero_gives_the_nominal_share(solver, cases):
    """Sigma = 0: p is 1 or 0 by the sign of cbar, pair_p is the integer share k/n_samples exactly, and CRS_MAX_PAIR_P ==
    CRS_NOMINAL_SHARE == CILQR_SCORE_COLLISION of cilqr_score_batch_sampled on the same plan."""
    import cilqr_amd
    s, want = cases["scenes"]["S"], cases["want"]["S_zero"]
    got = _host(solver, s, np.zeros_like(want["sigma"]))
    assert set(np.unique(got["entry_p"]).tolist()) == {0.0, 1.0}
    assert np.array_equal(got["pair_p"], want["k"] / s["ns"]) and np.array_equal(got["entry_p"], want["entry_p"])
    score = solver.score_batch_sampled(s["N"], s["X"], s["U"], s["poly"], s["fl"], s["nom_pose"], s["nom_dim"], s["off"], s["weight"])["score"]
    assert np.array_equal(got["risk"][:, MAX_PAIR_P], got["risk"][:, NOMINAL_SHARE])
    assert np.array_equal(got["risk"][:, NOMINAL_SHARE], score[:, cilqr_amd.SCORE_COLLISION]) and got["risk"][:, NOMINAL_SHARE].max() > 0
    # under the scenes' Sigma the nominal share is the same count
    noisy = _host(solver, s, cases["want"]["S"]["sigma"])
    assert np.array_equal(noisy["risk"][:, NOMINAL_SHARE], score[:, cilqr_amd.SCORE_COLLISION])


@gpu
def test_a_result_depends_on_its_own_solve_alone(solver, cases):
    """Each solve of scene X alone (B = 1), the batch reversed, and the batch embedded in a larger one give the batch's bits."""
    s, sigma = cases["scenes"]["X"], cases["want"]["X"]["sigma"]
    B = s["X"].shape[0]
    base = np.linspace(1.0, 2.0, B)
    whole = _host(solver, s, sigma, max_risk=0.1, base=base)
    assert np.isnan(whole["total"]).any() and not np.isnan(whole["total"]).all()
    for b in range(B):
        assert _same(_host(solver, s, sigma, sel=slice(b, b + 1), max_risk=0.1, base=base), whole, sel_b=slice(b, b + 1)), b
    assert _same(_host(solver, s, sigma, sel=slice(None, None, -1), max_risk=0.1, base=base), whole, sel_b=slice(None, None, -1))
    idx = np.array([3, 0, 1, 2, 3, 4, 5, 5, 2, 0, 1, 4, 3, 2, 1, 0])  # 16 solves: the batch at places 1..6 of a larger one
    big = _host(solver, s, sigma, sel=idx, max_risk=0.1, base=base)
    assert _same(big, whole, sel_a=slice(1, 7)) and _same(big, whole, sel_a=slice(13, 16), sel_b=slice(2, None, -1))


@gpu
def test_call_forms_and_composition(cilqr, solver, cases):
    """Host form == device form; optional outputs left out change nothing else; CILQR_CHANCE_SAMPLED_BOUND_SUM; max_risk 1e-6 either side
    of each candidate's value; a NaN base stays NaN; the total feeds cilqr_argmin_device."""
    import torch
    s, want = cases["scenes"]["S"], cases["want"]["S"]
    B = want["B"]
    sigma = want["sigma"]
    base = np.linspace(3.0, 2.0, B)
    for max_risk, flags in ((0.1, 0), (0.1, BOUND_SUM)):
        host = _host(solver, s, sigma, max_risk=max_risk, base=base, sum_bound=bool(flags))
        assert _same(host, _device(solver, s, sigma, max_risk=max_risk, base=base, flags=flags))
        expect = _total(want["risk"], base, max_risk, bool(flags))
        _check_total(host["total"], expect, (max_risk, flags))
        dev = torch.device("cuda", 0)
        v, out = torch.from_numpy(host["total"]).to(dev), torch.zeros(2, dtype=torch.float64, device=dev)
        solver.argmin_device(torch.cuda.current_stream(dev).cuda_stream, B, v.data_ptr(), out.data_ptr())
        torch.cuda.synchronize(dev)
        assert int(out.cpu().numpy()[1]) == _pick(expect)
    assert np.isnan(_total(want["risk"], base, 0.1, True)).sum() > np.isnan(_total(want["risk"], base, 0.1)).sum() > 0
    assert _device(solver, s, sigma)["total"] is None
    full = _host(solver, s, sigma, max_risk=0.1, base=base)
    for n in OUTPUTS:
        part = _host(solver, s, sigma, max_risk=0.1, base=None if n == "total" else base, skip=(n,))
        assert part[n] is None and _same(part, full, names=[m for m in ("risk",) + OUTPUTS if m != n]), n
    none = _host(solver, s, sigma, skip=OUTPUTS)
    assert np.array_equal(_bits(none["risk"]), _bits(full["risk"]))
    for b in range(B):
        r = want["risk"][b, STEP_RISK]
        below, above = (_host(solver, s, sigma, max_risk=r + d, base=base, skip=("entry_p",))["total"] for d in (-MARGIN, MARGIN))
        assert np.isnan(below[b]) and above[b] == base[b], b
        _check_total(below, _total(want["risk"], base, r - MARGIN), b)
        _check_total(above, _total(want["risk"], base, r + MARGIN), b)
    nan_base = base.copy()
    nan_base[4] = np.nan  # a base that is already rejected stays rejected
    _check_total(_host(solver, s, sigma, max_risk=1.0, base=nan_base)["total"], _total(want["risk"], nan_base, 1.0), "a NaN base")


@gpu
def test_lost_steps(solver, cases):
    """A NaN in X_t (solve 1, step 3) and in one of the six Sigma_t entries (solve 2, step 5): r_t = 1 there and nowhere else.  The
    entries keep the header's definitions: a quadratic form that is NaN counts as 0, so s = 0 and p is 1 or 0 by the sign of cbar — 0
    where cbar itself is NaN; no maximum is NaN.  Every other step and solve keeps its bits."""
    s, want = cases["scenes"]["S"], cases["want"]["S"]
    B, N, n_obs, ns = want["B"], s["N"], s["n_obs"], s["ns"]
    clean = _host(solver, s, want["sigma"])
    bad, sigma = dict(s), want["sigma"].copy()
    bad["X"] = s["X"].copy()
    bad["X"][1, 4 * 3 + 1] = np.nan
    sigma[2, 5, 12] = np.nan
    got = _host(solver, bad, sigma)
    ep = want["entry_p"].copy()
    ep[1, :, 3] = 0.0
    with np.errstate(invalid="ignore"):
        hit = want["cbar"].max(axis=3) > 0
    ep[2, :, 5] = hit[2, :, 5]
    hit[1, :, 3] = False
    lost = np.zeros((B, N), dtype=bool)
    lost[1, 3] = lost[2, 5] = True
    expect = _fields(ep, hit, n_obs, ns, lost)
    _check_against(got, expect, "lost steps")
    assert got["step_risk"][1, 3] == 1.0 and got["step_risk"][2, 5] == 1.0
    keep = ~lost
    assert np.array_equal(_bits(got["step_risk"][keep]), _bits(clean["step_risk"][keep]))
    assert not got["entry_p"][1, :, 3].any() and not got["pair_p"][1, :, 3].any()
    assert not np.isnan(got["risk"]).any() and set(np.unique(got["entry_p"][2, :, 5]).tolist()) <= {0.0, 1.0}
    assert np.array_equal(got["risk"][[1, 2], STEP_RISK], [1.0, 1.0]) and got["risk"][[1, 2], WORST_STEP].tolist() == [3.0, 5.0]
    others = np.array([0, 3, 4, 5])
    assert _same(got, clean, sel_a=others, sel_b=others, names=("risk", "step_risk", "pair_p", "entry_p"))


@gpu
def test_errors_and_limits(cilqr, oracle, cases):
    """B, N and n_obs*n_samples beyond the create limits and a host call beyond the arena are CILQR_ERR_ARG; the largest scene the LDS
    formula of the header admits (32*n_obs*n_samples = 64 KiB) runs and is right, one sample more is CILQR_ERR_UNSUPPORTED; the
    handle stays usable."""
    s, want = cases["scenes"]["S"], cases["want"]["S"]
    sv = cilqr.Solver(cilqr.default_params(12), max_batch=4, max_horizon=10, max_obstacles=15, device=0)
    try:
        for sc, sel, what in ((_cut(s, N=10), slice(0, 5), "B="), (s, slice(0, 2), "N="), (_cut(s, N=10), slice(0, 2), "M=")):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: %s" % (ERR_ARG, what)):
                _host(sv, sc, want["sigma"][:, :sc["N"] + 1], sel=sel)
        small = _cut(s, N=10, ns=7)
        ok = _host(sv, small, want["sigma"][:, :11], sel=slice(0, 4))
        assert np.all(np.abs(ok["step_risk"] - _want(small)["step_risk"][:4]) <= TOL)
    finally:
        sv.close()
    # max_horizon 1, 7 x 2 samples, B = max_batch = 128: with entry_p only B <= max_batch / 2 is promised, and here the whole batch
    # is beyond the arena — 159744 bytes against the 158208 that host_arena_bytes(128, 1, 14) reserves
    one = _scene_w(oracle, 7, 2, 24, B=128, N=1)
    w1 = _want(one)
    sv = cilqr.Solver(cilqr.default_params(12), max_batch=128, max_horizon=1, max_obstacles=14, device=0)
    try:
        lean = _host(sv, one, w1["sigma"], skip=("entry_p",))
        assert np.all(np.abs(lean["pair_p"] - w1["pair_p"]) <= TOL) and np.all(np.abs(lean["step_risk"] - w1["step_risk"]) <= TOL)
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers reserved at create" % ERR_ARG):
            _host(sv, one, w1["sigma"], base=np.zeros(128))  # (every array of the call: base and total included)
        half = _host(sv, one, w1["sigma"], sel=slice(0, 64))
        assert _same(half, lean, sel_b=slice(0, 64), names=("risk", "step_risk", "pair_p"))
        _check_against(half, w1, "7 x 2 samples, N = 1", sel=slice(0, 64))
    finally:
        sv.close()
    w = cases["scenes"]["W2048"]
    assert 32 * 1 * 2048 == 64 * 1024
    sv = cilqr.Solver(cilqr.default_params(12), max_batch=2, max_horizon=2, max_obstacles=2049, device=0)
    try:
        got = _host(sv, w, cases["want"]["W2048"]["sigma"])
        _check_against(got, cases["want"]["W2048"], "1 x 2048 samples")
        more = _scene_w(oracle, 1, 2049, 23)
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*do not fit 64 KiB of LDS" % ERR_UNSUPPORTED):
            _host(sv, more, cases["want"]["W2048"]["sigma"])
        assert _same(_host(sv, w, cases["want"]["W2048"]["sigma"]), got)
    finally:
        sv.close()


@gpu
def test_cpp_facade_sample_covariance_checked_candidates(tmp_path):
    """tests/cpp/candidates_chance_sampled.cpp: with samples set, the index run_candidates picks under iLQR::set_sample_covariance_check
    equals the pick computed from the C-ABI calls in the documented order on the same candidates; a max_risk that rejects all gives
    -1; the conflicts with the noise setters and with "no samples set" throw, naming the other setter; set_pose_covariance_check with
    samples still throws."""
    exe = str(tmp_path / "candidates_chance_sampled")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_chance_sampled.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sample chance pick ok" in r.stdout and "rejects all ok" in r.stdout and "conflicts throw ok" in r.stdout, r.stdout
