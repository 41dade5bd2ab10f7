"""Analytic map risk (cilqr_chance_risk_map*, cilqr_pose_quadrature, include/cilqr.h): per step the pose marginal of Sigma_t is factored,
Q weighted standard-normal nodes are placed through the factor, the footprint is looked up in the uncertainty map under every node, and the
weighted mass of nodes that hit, of nodes that are unknown and the weighted mean of the nodes' largest occupancy are reported.

Expected values never come from the HIP path: the oracle's scenes, trajectories and gains (tests/test_rollout_risk.py), `restate` of
tests/test_chance_risk.py for Sigma_t, probe_positions / np_lookup / smooth_layer of tests/test_risk_map.py, and `restate_map` below, a
numpy restatement of the header's definitions.  r_t, u_t and the fields made of them within 1e-9 absolute, e_t and the occupancies
within 1e-7 (the suite's OCC_TOL), steps and picks exact, total bit-equal to base or NaN.  What makes the exact comparisons meaningful
is asserted on the restatement in test_conditions.

  R1 ... R405   scene R (B 8, N 12) on case A's map of test_risk_map (160 x 80 at 0.1 m, probes 3 x 3, threshold 50), Gauss-Hermite rules
                1x1x1, 5x3x3, 4x4x4, 5x5x3, 7x7x3, 9x9x5: Q = 1 (the nominal footprint), 45 (a partial wavefront), 64, 75 (64 + 11),
                147 (three chunks), 405 (seven)
  N2            the first two steps of R, Q = 75: a workgroup with two idle wavefronts
  L             scene L (B 6, N 50) on case L's map, Q = 75: 13 workgroups per solve, the last with two steps
  C1, C23       R, Q = 75, per-solve layers (seeds 1..8) and poses through set_uncertainty_map_device, probes 1 x 1 and 2 x 3
  D             R, Q = 75, the map that ends inside the horizon (GEOM_D), threshold 100: u_t > 0, both settings of UNKNOWN_HITS
  Z             R, Q = 75, Sigma = 0: every node on the mean
"""
import copy
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
from test_risk_map import (GEOM_A, GEOM_D, GEOM_L, OCC_TOL, POSE_A, POSE_L, SAFE, _c_poses, _case, _Map, _params, np_lookup,
                           probe_positions, smooth_layer)
from test_rollout_risk import _pick, _scene_l, _scene_r, o_gains

gpu = pytest.mark.gpu

TOL, MARGIN = 1e-9, 1e-6
ERR_ARG = -1
ENTRY_POINTS = ("cilqr_chance_risk_map", "cilqr_chance_risk_map_device", "cilqr_pose_quadrature")
FIELDS = ("STEP_RISK", "WORST_STEP", "SUM_RISK", "FIRST_STEP", "MEAN_OCC", "MEAN_OCC_STEP", "WORST_OCC", "UNKNOWN")
STEP_RISK, WORST_STEP, SUM_RISK, FIRST_STEP, MEAN_OCC, MEAN_OCC_STEP, WORST_OCC, UNKNOWN = range(8)
UNKNOWN_HITS, BOUND_SUM = 1, 2
SIX = (0, 4, 5, 12, 13, 15)  # (0,0), (0,1), (1,1), (0,3), (1,3), (3,3) at [r + 4c]
ROLLOUT_S, ROLLOUT_SEED = 1000, 9
# max over solves and steps of |r_t - the rollouts' share at step t| with the rollouts' own draws as equal-weight nodes, measured with
# the restatement on the CPU at S = 1000, seed 9: 0.007 (seven rows of a thousand).  The tests assert twice that.
ROLLOUT_MEASURED = 0.007
_dp = C.POINTER(C.c_double)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


# ---- expected values: numpy's Gauss-Hermite rule and a numpy restatement of the header's definitions -------------------------------
def np_quadrature(nx, ny, nth):
    """The tensor product of numpy's probabilists' Gauss-Hermite rules, weights normalised per axis; z_theta fastest, z_x slowest."""
    from numpy.polynomial.hermite_e import hermegauss
    ax = [hermegauss(n) for n in (nx, ny, nth)]
    ax = [(z, w / np.sqrt(2.0 * np.pi)) for z, w in ax]
    zx, zy, zt = np.meshgrid(ax[0][0], ax[1][0], ax[2][0], indexing="ij")
    wx, wy, wt = np.meshgrid(ax[0][1], ax[1][1], ax[2][1], indexing="ij")
    return np.stack([zx.ravel(), zy.ravel(), zt.ravel()], axis=1), (wx * wy * wt).ravel()


def factor(sigma, T=np.float64):
    """sigma (..., 16) -> (l00, l10, l11, l20, l21, l22) (..., 6) by the header's statements, evaluated in T."""
    c00, c10, c11, c20, c21, c22 = (np.asarray(sigma[..., i], dtype=T) for i in SIX)
    zero = T(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        l00 = np.sqrt(np.fmax(c00, zero))
        l10, l20 = np.where(l00 > 0, c10 / l00, zero), np.where(l00 > 0, c20 / l00, zero)
        l11 = np.sqrt(np.fmax(c11 - l10 * l10, zero))
        l21 = np.where(l11 > 0, (c21 - l20 * l10) / l11, zero)
        l22 = np.sqrt(np.fmax(c22 - l20 * l20 - l21 * l21, zero))
    return np.stack([l00, l10, l11, l20, l21, l22], axis=-1)


def reduce_steps(r, u, e, step_worst):
    """(B, N) per-step values -> risk (B, 8)."""
    B = r.shape[0]
    risk = np.zeros((B, 8))
    risk[:, STEP_RISK], risk[:, WORST_STEP] = r.max(axis=1), r.argmax(axis=1)
    risk[:, SUM_RISK] = np.minimum(1.0, r.sum(axis=1))
    risk[:, FIRST_STEP] = np.where((r > 0).any(axis=1), (r > 0).argmax(axis=1), -1)
    risk[:, MEAN_OCC], risk[:, MEAN_OCC_STEP] = e.max(axis=1), e.argmax(axis=1)
    risk[:, WORST_OCC] = step_worst.max(axis=1)
    risk[:, UNKNOWN] = u.max(axis=1)
    return risk


def restate_map(p, probes, N, X, sigma, nodes, weights, g, layers, poses, threshold):
    """X (B, 4(N+1)), sigma (B, N+1, 16), nodes (Q, 3), weights (Q,); layers / poses one shared or lists of B.  Returns the node
    poses' probes and occupancies and, under [False] / [True] (UNKNOWN_HITS), dict(step_risk, step_occ, step_unknown, risk, hit)."""
    B, Q = X.shape[0], weights.shape[0]
    Xs, S = X.reshape(B, N + 1, 4)[:, :N], sigma.reshape(B, N + 1, 16)[:, :N]
    L = factor(S)
    zx, zy, zt = nodes[:, 0], nodes[:, 1], nodes[:, 2]
    states = np.zeros((B, N, Q, 4))
    with np.errstate(invalid="ignore"):
        states[..., 0] = Xs[..., 0:1] + L[..., 0:1] * zx
        states[..., 1] = Xs[..., 1:2] + (L[..., 1:2] * zx + L[..., 2:3] * zy)
        states[..., 3] = Xs[..., 3:4] + (L[..., 3:4] * zx + L[..., 4:5] * zy + L[..., 5:6] * zt)
    lost = ~(np.isfinite(Xs[..., [0, 1, 3]]).all(axis=2) & np.isfinite(S[..., list(SIX)]).all(axis=2))   # (B, N)
    per_solve = isinstance(layers, list)
    P = probes[0] * probes[1]
    occ, ok = np.zeros((B, N, Q, P)), np.zeros((B, N, Q, P), dtype=bool)
    qx, qy = np.zeros((B, N, Q, P)), np.zeros((B, N, Q, P))
    with np.errstate(invalid="ignore"):
        for b in range(B):
            qx[b], qy[b] = probe_positions(p, probes, states[b], poses[b] if per_solve else poses)
            occ[b], ok[b] = np_lookup(layers[b] if per_solve else layers, g, qx[b], qy[b])
    unknown = (~ok).any(axis=3)
    has = ok.any(axis=3)
    m = np.where(ok, occ, -np.inf).max(axis=3)
    e = np.where(lost, 0.0, (weights * np.where(has, m, 0.0)).sum(axis=2))
    u = np.where(lost, 1.0, np.minimum(1.0, (weights * unknown).sum(axis=2)))
    step_worst = np.where(lost, -np.inf, m.max(axis=2))
    out = dict(B=B, N=N, Q=Q, occ=occ, ok=ok, qx=qx, qy=qy, lost=lost, L=L, unknown=unknown)
    for flag in (False, True):
        hit = (ok & (occ > threshold)).any(axis=3)
        if flag:
            hit = hit | unknown
        r = np.where(lost, 1.0, np.minimum(1.0, (weights * hit).sum(axis=2)))
        out[flag] = dict(step_risk=r, step_occ=e, step_unknown=u, risk=reduce_steps(r, u, e, step_worst), hit=hit)
    return out


def _total(risk, base, max_risk, sum_bound=False):
    field = risk[:, SUM_RISK if sum_bound else STEP_RISK]
    return np.where((field > max_risk) | ~np.isfinite(base), np.nan, base)


def _decided(w):
    """Per solve: is WORST_STEP decided — every step within 1e-6 of the largest r_t has the hit set of the winner, so the same bits
    and the lowest index wins on both sides — and is MEAN_OCC_STEP (the two largest e_t more than 1e-6 apart)?"""
    r, e, hit = w["step_risk"], w["step_occ"], w["hit"]
    B = r.shape[0]
    worst = np.ones(B, dtype=bool)
    for b in range(B):
        t0 = int(r[b].argmax())
        for t in np.nonzero(np.abs(r[b] - r[b, t0]) <= MARGIN)[0]:
            worst[b] &= bool(np.array_equal(hit[b, t], hit[b, t0]))
    s = np.sort(e, axis=1)
    occ = (s[:, -1] - s[:, -2] > MARGIN) if e.shape[1] > 1 else np.ones(B, dtype=bool)
    return worst, occ


RULES = {"R1": (1, 1, 1), "R45": (5, 3, 3), "R64": (4, 4, 4), "R75": (5, 5, 3), "R147": (7, 7, 3), "R405": (9, 9, 5)}


def _mk(s, N, sigma, rule, geom, probes, threshold, layers, poses, O):
    p = copy.copy(s["p"])
    p.safe_length, p.safe_width = SAFE
    X = np.ascontiguousarray(s["X"][:, :4 * (N + 1)])
    sigma = np.ascontiguousarray(sigma[:, :N + 1])
    nodes, weights = np_quadrature(*rule) if len(rule) == 3 else rule
    g = O.map_geom(*geom)
    out = restate_map(p, probes, N, X, sigma, nodes, weights, g, layers, poses, threshold)
    out.update(p=p, X=X, sigma=sigma, nodes=np.ascontiguousarray(nodes), weights=np.ascontiguousarray(weights), geom=geom, g=g,
               probes=probes, threshold=threshold, layers=layers, poses=poses)
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """Every case's restatement (both flags).  Computed once; never modified."""
    from cilqr_amd import scenes
    O = oracle
    r, l = _scene_r(O), _scene_l(O)
    for s in (r, l):
        pose, dim = np.ascontiguousarray(s["pose"]).reshape(s["B"], s["M"], -1), np.ascontiguousarray(s["dim"]).reshape(s["B"], s["M"], -1)
        s["k"], s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], pose, dim, None, 1.0)
        assert np.all(ok == 1)
        s["sigma"] = restate(s["p"], s["N"], s["X"], s["U"], s["K"], SIGMA0.T.reshape(16), None, None, None)["sigma"]
    la, ld, ll = smooth_layer(160, 80, 3), smooth_layer(30, 80, 3), smooth_layer(300, 100, 3)
    lc = [smooth_layer(160, 80, seed) for seed in range(1, r["B"] + 1)]
    out = {name: _mk(r, r["N"], r["sigma"], rule, GEOM_A, (3, 3), 50.0, la, POSE_A, O) for name, rule in RULES.items()}
    q75 = RULES["R75"]
    out["N2"] = _mk(r, 2, r["sigma"], q75, GEOM_A, (3, 3), 50.0, la, POSE_A, O)
    out["L"] = _mk(l, l["N"], l["sigma"], q75, GEOM_L, (3, 3), 50.0, ll, POSE_L, O)
    out["C1"] = _mk(r, r["N"], r["sigma"], q75, GEOM_A, (1, 1), 50.0, lc, _c_poses(r["B"]), O)
    out["C23"] = _mk(r, r["N"], r["sigma"], q75, GEOM_A, (2, 3), 50.0, lc, _c_poses(r["B"]), O)
    out["D"] = _mk(r, r["N"], r["sigma"], q75, GEOM_D, (3, 3), 100.0, ld, POSE_A, O)
    out["Z"] = _mk(r, r["N"], np.zeros_like(r["sigma"]), q75, GEOM_A, (3, 3), 50.0, la, POSE_A, O)
    # the oracle's rollouts from S seeded offsets, k_scale 0, and the same draws divided by their sigmas as equal-weight nodes
    delta = scenes.pose_offsets(ROLLOUT_S, 0.16, 0.16, 0.017, seed=ROLLOUT_SEED)
    roll = _case(O, r, ROLLOUT_S, delta, 0.0, GEOM_A, (3, 3), 50.0, la, POSE_A)
    draws = (np.ascontiguousarray(delta[:, [0, 1, 3]] / np.array([0.16, 0.16, 0.017])), np.full(ROLLOUT_S, 1.0 / ROLLOUT_S))
    out["S"] = _mk(r, r["N"], r["sigma"], draws, GEOM_A, (3, 3), 50.0, la, POSE_A, O)
    out["S"]["share"] = roll[False]["step_hits"] / float(ROLLOUT_S)
    out["scene_r"], out["scene_l"] = r, l
    return out


CASES = list(RULES) + ["N2", "L", "C1", "C23", "D", "Z", "S"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_CHANCE_MAP_FIELDS\s+8\b", h) and re.search(r"#define\s+CILQR_MAX_QUAD_NODES\s+1024\b", h)
    assert re.search(r"#define\s+CILQR_CHANCE_MAP_UNKNOWN_HITS\s+1u", h) and re.search(r"#define\s+CILQR_CHANCE_MAP_BOUND_SUM\s+2u", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_CM_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "CM_" + name) == i
    assert cilqr.CHANCE_MAP_FIELDS == 8 and cilqr.CHANCE_MAP_UNKNOWN_HITS == 1 and cilqr.CHANCE_MAP_BOUND_SUM == 2
    assert cilqr.MAX_QUAD_NODES == 1024
    assert callable(cilqr.Solver.chance_risk_map) and callable(cilqr.Solver.chance_risk_map_device) and callable(cilqr.pose_quadrature)
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_map_covariance_check\s*\(\s*double\s+occ_threshold\s*,\s*double\s+max_risk\s*,\s*int\s+nx\s*=\s*5\s*,"
                     r"\s*int\s+ny\s*=\s*5\s*,\s*int\s+nth\s*=\s*3\s*,\s*bool\s+sum_bound\s*=\s*false\s*,\s*bool\s+unknown_hits\s*=\s*false\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_chance_map_risk\s*,\s*last_map_step_risk\s*;", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_chance_risk_map\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_chance_map.hip" in mk and re.search(r"^check:.*build/cilqr_chance_map\.o", mk, flags=re.M)


def test_argument_errors_need_no_device(cilqr):
    """NULL X, sigma, nodes, weights or risk, total without base, Q outside 1 ... 1024, a NaN occ_threshold or max_risk, unknown flag bits,
    and in the host form a weight that is negative or not finite: CILQR_ERR_ARG, decided before the handle is looked at (there is none
    here).  cilqr_pose_quadrature: NULL pointers and node counts outside 1 ... 9."""
    L = cilqr.lib()
    B, N, Q = 2, 4, 3
    X, sigma, nodes, weights = np.zeros((B, 4 * (N + 1))), np.zeros((B, N + 1, 16)), np.zeros((Q, 3)), np.full(Q, 1.0 / Q)
    risk, sr, so, su, total, base = np.zeros((B, 8)), np.zeros((B, N)), np.zeros((B, N)), np.zeros((B, N)), np.zeros(B), np.zeros(B)
    no_handle = C.c_void_p()
    d = C.c_double
    nan = float("nan")

    def call(dev, Q_=Q, thr=50.0, flags=0, mr=1.0, **nulls):
        a = dict(X=X, sigma=sigma, nodes=nodes, weights=weights, risk=risk, base=base, total=total)
        a.update(nulls)
        f = L.cilqr_chance_risk_map_device if dev else L.cilqr_chance_risk_map
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, Q_, _p(a["X"]), _p(a["sigma"]), _p(a["nodes"]), _p(a["weights"]), d(thr), C.c_uint32(flags), d(mr),
                 _p(a["base"]), _p(a["risk"]), _p(sr), _p(so), _p(su), _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "sigma", "nodes", "weights", "risk"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        for q in (0, -1, 1025):
            assert call(dev, Q_=q) == ERR_ARG and b"outside [1, 1024]" in L.cilqr_last_error(), q
        for kw in ("thr", "mr"):
            assert call(dev, **{kw: nan}) == ERR_ARG and b"NaN" in L.cilqr_last_error(), kw
        assert call(dev, flags=4) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev, flags=3) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # neither: valid too
    for bad in (-1e-3, nan, float("inf")):
        w = weights.copy()
        w[1] = bad
        assert call(False, weights=w) == ERR_ARG and b"weight 1 is negative or not finite" in L.cilqr_last_error(), bad
        assert call(True, weights=w) == ERR_ARG and b"null handle" in L.cilqr_last_error(), bad  # device memory is not read on the host
    out_n, out_w = np.zeros((9 * 9 * 9, 3)), np.zeros(9 * 9 * 9)
    assert L.cilqr_pose_quadrature(3, 3, 3, None, _p(out_w)) == ERR_ARG and L.cilqr_pose_quadrature(3, 3, 3, _p(out_n), None) == ERR_ARG
    for bad in ((0, 3, 3), (3, 10, 3), (3, 3, -1)):
        assert L.cilqr_pose_quadrature(*bad, _p(out_n), _p(out_w)) == ERR_ARG and b"1 ... 9" in L.cilqr_last_error(), bad


def test_pose_quadrature_is_numpys_gauss_hermite(cilqr):
    """Every n in 1 ... 9 per axis against numpy.polynomial.hermite_e.hermegauss to 1e-13; z_theta fastest, z_x slowest, each axis
    ascending; the weights sum to 1 within 1e-14; the same arguments give the same bits."""
    worst = 0.0
    for n in range(1, 10):
        for rule in ((n, 1, 1), (1, n, 1), (1, 1, n), (n, 10 - n, (n + 3) % 9 + 1)):
            nodes, weights = cilqr.pose_quadrature(*rule)
            zn, wn = np_quadrature(*rule)
            assert nodes.shape == zn.shape and weights.shape == wn.shape
            worst = max(worst, float(np.max(np.abs(nodes - zn))), float(np.max(np.abs(weights - wn))))
            assert abs(weights.sum() - 1.0) <= 1e-14 and np.all(weights > 0)
    print("max |node or weight - numpy's| %.3g" % worst)
    assert worst <= 1e-13
    nodes, weights = cilqr.pose_quadrature(3, 2, 4)
    assert np.all(np.diff(nodes[:4, 2]) > 0) and np.all(nodes[:4, :2] == nodes[0, :2])   # z_theta fastest, ascending
    assert nodes[4, 1] > nodes[0, 1] and nodes[8, 0] > nodes[0, 0] and nodes[7, 0] == nodes[0, 0]  # then z_y, then z_x
    assert np.array_equal(nodes[:, 0], -nodes[::-1, 0])  # mirrored about 0 exactly
    again = cilqr.pose_quadrature(3, 2, 4)
    assert np.array_equal(_bits(again[0]), _bits(nodes)) and np.array_equal(_bits(again[1]), _bits(weights))
    big = cilqr.pose_quadrature(9, 9, 9)
    assert big[1].shape == (729,) and abs(big[1].sum() - 1.0) <= 1e-14


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_chance_map.cpp: plan_chance_risk_map laid out without an arena against host_arena_bytes at the shapes
    include/cilqr.h says always fit; and host_arena_bytes is still what tests/golden/host_arena_cap.json recorded."""
    exe = str(tmp_path / "host_plan_chance_map")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_chance_map.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1200:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "10 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


@pytest.mark.parametrize("name", CASES)
def test_conditions(cases, name):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the restatement's numbers alone: every valid probe's
    occupancy more than 1e-6 from the threshold, every probe's validity unchanged at the four points displaced by 1e-6 m, the factors in
    float64 and longdouble within 1e-11; which solves' WORST_STEP and MEAN_OCC_STEP are decided is printed (the others are compared on
    values only)."""
    s = cases[name]
    occ, ok = s["occ"], s["ok"]
    w = s[False]
    gap = float(np.min(np.abs(occ[ok] - s["threshold"])))
    worst, mean = _decided(w)
    print("case %s: Q %d, min|occ - thr| %.3g; STEP_RISK %s; MEAN_OCC %s; WORST_STEP decided for %s, MEAN_OCC_STEP for %s" % (
        name, s["Q"], gap, np.round(w["risk"][:, STEP_RISK], 5).tolist(), np.round(w["risk"][:, MEAN_OCC], 3).tolist(),
        np.nonzero(worst)[0].tolist(), np.nonzero(mean)[0].tolist()))
    assert not s["lost"].any()
    assert gap > MARGIN
    per_solve = isinstance(s["layers"], list)
    for dx, dy in ((MARGIN, 0.0), (-MARGIN, 0.0), (0.0, MARGIN), (0.0, -MARGIN)):
        for b in range(s["B"]):
            _, okd = np_lookup(s["layers"][b] if per_solve else s["layers"], s["g"], s["qx"][b] + dx, s["qy"][b] + dy)
            assert np.array_equal(okd, ok[b]), (b, dx, dy)
    assert np.longdouble(1) + np.finfo(np.longdouble).eps != 1 and np.finfo(np.longdouble).eps < 1e-18  # longdouble is wider here
    dl = float(np.max(np.abs(s["L"] - factor(s["sigma"][:, :s["N"]], np.longdouble).astype(np.float64))))
    print("  factors, float64 vs longdouble: %.3g" % dl)
    assert dl <= 1e-11
    assert np.all(np.isfinite(w["risk"][:, WORST_OCC]))
    r = w["step_risk"]
    if name == "R1":  # the nominal footprint: every r_t is 0 or 1
        assert set(np.unique(r).tolist()) <= {0.0, 1.0} and (r == 1.0).any() and (r == 0.0).any()
    if name in ("R75", "R147", "R405", "S"):
        assert np.any((r > 0) & (r < 1))
    if name == "Z":  # Sigma = 0: every node on the mean, and R1's verdicts
        assert not s["L"].any() and np.array_equal(r, np.where(cases["R1"][False]["step_risk"] > 0.5, np.minimum(1.0, s["weights"].sum()), 0.0))
    if name == "D":  # the map ends inside the horizon: u_t rises to 1, nothing hits without the flag, the flag makes hits
        u = w["step_unknown"]
        assert np.all(u[:, -1] > 0.99) and np.any((u > 1e-3) & (u < 1 - 1e-3)) and not r.any()
        assert np.array_equal(s[True]["step_risk"], u)
    if name in ("C1", "C23"):  # solve b's own layer and pose matter
        alt = restate_map(s["p"], s["probes"], s["N"], s["X"], s["sigma"], s["nodes"], s["weights"], s["g"], s["layers"][0], s["poses"][0],
                          s["threshold"])[False]
        assert np.all(np.max(np.abs(alt["step_occ"][1:] - w["step_occ"][1:]), axis=1) > 1e-3)


def test_the_restatement_reproduces_the_rollouts_marginals(cases):
    """Scene R on case A's map, k_scale 0: the oracle's S = 1000 rollouts from seeded offsets against r_t of the restatement with the
    same draws, divided by their sigmas, as equal-weight nodes through the factor of the restated Sigma_t.  The linear covariance chain
    reproduces the rollouts' per-step marginals: max |r_t - share_t| was 0.007 on the CPU at S = 1000, seed 9 (ROLLOUT_MEASURED); twice
    that is asserted."""
    s = cases["S"]
    d = np.abs(s[False]["step_risk"] - s["share"])
    print("max |r_t - rollouts' share| %.4g at (solve, step) %s; largest shares %s" % (
        d.max(), np.unravel_index(int(d.argmax()), d.shape), np.round(s["share"].max(axis=1), 4).tolist()))
    assert np.any((s["share"] > 0) & (s["share"] < 1))
    assert d.max() <= 2 * ROLLOUT_MEASURED


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(_params(cilqr), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


OUT = ("risk", "step_risk", "step_occ", "step_unknown", "total")


def _host(solver, s, sel=slice(None), flags=0, max_risk=1.0, base=None, X=None, sigma=None, want_steps=True):
    return solver.chance_risk_map(s["N"], (s["X"] if X is None else X)[sel], (s["sigma"] if sigma is None else sigma)[sel], s["nodes"],
                                  s["weights"], s["threshold"], max_risk=max_risk, base=base, sum_bound=bool(flags & BOUND_SUM),
                                  unknown_hits=bool(flags & UNKNOWN_HITS), want_steps=want_steps)


def _device(solver, s, flags=0, max_risk=1.0, base=None, steps=True):
    """The device form on torch buffers."""
    import torch
    B, N, Q = s["B"], s["N"], s["Q"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = {n: torch.from_numpy(np.ascontiguousarray(s[n])).to(dev) for n in ("X", "sigma", "nodes", "weights")}
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    risk, sr, so, su, total = z(B, 8), z(B, N), z(B, N), z(B, N), z(B)
    tb = None if base is None else torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    torch.cuda.synchronize(dev)
    solver.chance_risk_map_device(stream, B, N, Q, t["X"].data_ptr(), t["sigma"].data_ptr(), t["nodes"].data_ptr(), t["weights"].data_ptr(),
                                  s["threshold"], risk.data_ptr(), sr.data_ptr() if steps else 0, so.data_ptr() if steps else 0,
                                  su.data_ptr() if steps else 0, total.data_ptr() if tb is not None else 0,
                                  tb.data_ptr() if tb is not None else 0, max_risk=max_risk, flags=flags)
    torch.cuda.synchronize(dev)
    out = dict(risk=risk.cpu().numpy(), step_risk=sr.cpu().numpy(), step_occ=so.cpu().numpy(), step_unknown=su.cpu().numpy(),
               total=None if tb is None else total.cpu().numpy())
    return out


def _same(a, b, sel_a=slice(None), sel_b=slice(None), names=OUT):
    return all((a[n] is None and b[n] is None) or np.array_equal(_bits(a[n][sel_a]), _bits(b[n][sel_b])) for n in names)


def _check_against(got, want, what, sel=slice(None)):
    risk, wr = got["risk"], want["risk"][sel]
    worst, mean = (d[sel] for d in _decided(want))
    d = {n: float(np.max(np.abs(got[n] - want[n][sel]))) for n in ("step_risk", "step_unknown", "step_occ")}
    df = {FIELDS[f]: float(np.max(np.abs(risk[:, f] - wr[:, f]))) for f in (STEP_RISK, SUM_RISK, UNKNOWN, MEAN_OCC, WORST_OCC)}
    print("%s: %s %s; undecided WORST_STEP %s, MEAN_OCC_STEP %s" % (what, d, df, np.nonzero(~worst)[0].tolist(), np.nonzero(~mean)[0].tolist()))
    assert d["step_risk"] <= TOL and d["step_unknown"] <= TOL and d["step_occ"] <= OCC_TOL, what
    for f in (STEP_RISK, SUM_RISK, UNKNOWN):
        assert df[FIELDS[f]] <= TOL, (what, FIELDS[f])
    for f in (MEAN_OCC, WORST_OCC):
        assert df[FIELDS[f]] <= OCC_TOL, (what, FIELDS[f])
    assert np.array_equal(risk[:, FIRST_STEP], wr[:, FIRST_STEP]), (what, risk[:, FIRST_STEP], wr[:, FIRST_STEP])
    assert np.array_equal(risk[worst, WORST_STEP], wr[worst, WORST_STEP]), (what, risk[:, WORST_STEP], wr[:, WORST_STEP])
    assert np.array_equal(risk[mean, MEAN_OCC_STEP], wr[mean, MEAN_OCC_STEP]), (what, risk[:, MEAN_OCC_STEP], wr[:, MEAN_OCC_STEP])
    # where the step is not decided it still names a step whose value is the maximum
    rows = np.arange(risk.shape[0])
    assert np.all(np.abs(got["step_risk"][rows, risk[:, WORST_STEP].astype(int)] - risk[:, STEP_RISK]) == 0), what
    assert np.all(np.abs(got["step_occ"][rows, risk[:, MEAN_OCC_STEP].astype(int)] - risk[:, MEAN_OCC]) == 0), what


def _check_total(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(_bits(got[~np.isnan(want)]), _bits(want[~np.isnan(want)])), what


@gpu
@pytest.mark.parametrize("name", list(RULES) + ["N2", "L", "D", "Z"])
def test_fields_against_the_restatement(cilqr, solver, cases, name):
    """A shared map, the host and the device form, both settings of UNKNOWN_HITS: per-step values and fields within the tolerances, steps
    exact where decided; the two forms give the same bits; without per-step outputs the fields are the same bits."""
    s = cases[name]
    with _Map(cilqr, solver, s):
        for flag in (False, True):
            host = _host(solver, s, flags=UNKNOWN_HITS if flag else 0)
            assert host["total"] is None
            _check_against(host, s[flag], "case %s, host form, unknown_hits %s" % (name, flag))
            dev = _device(solver, s, flags=UNKNOWN_HITS if flag else 0)
            _check_against(dev, s[flag], "case %s, device form, unknown_hits %s" % (name, flag))
            assert _same(host, dev)
            lean = _host(solver, s, flags=UNKNOWN_HITS if flag else 0, want_steps=False)
            assert lean["step_risk"] is None and _same(lean, host, names=("risk",))
            lean = _device(solver, s, flags=UNKNOWN_HITS if flag else 0, steps=False)
            assert not lean["step_risk"].any() and _same(lean, host, names=("risk",))
        if name == "R1":
            assert set(np.unique(host["step_risk"]).tolist()) <= {0.0, 1.0}
        if name == "D":
            assert np.array_equal(_bits(host["step_risk"]), _bits(host["step_unknown"])) and not dev["step_risk"].all()


@gpu
@pytest.mark.parametrize("name", ["C1", "C23"])
def test_per_solve_layers_and_poses(cilqr, solver, cases, name):
    """set_uncertainty_map_device with layer_stride = rows*cols and poses [B][3]: solve b reads layer b with pose b — also when it sits
    elsewhere in a batch whose layers and poses travel with it."""
    s = cases[name]
    with _Map(cilqr, solver, s):
        for flag in (False, True):
            _check_against(_device(solver, s, flags=UNKNOWN_HITS if flag else 0), s[flag], "case %s, unknown_hits %s" % (name, flag))
        whole = _host(solver, s)
        _check_against(whole, s[False], "case %s, host form" % name)
    order = [5, 1, 7, 0, 2]
    with _Map(cilqr, solver, s, sel=order):
        moved = _host(solver, s, X=s["X"][order], sigma=s["sigma"][order])
    assert _same(moved, whole, sel_b=order)


@gpu
def test_a_result_depends_on_its_own_solve_alone(cilqr, solver, cases):
    """One solve alone, the batch reversed and the whole batch of 8; a shared layer and one equal copy of it per solve: identical bits per
    solve in every output.  Q = 147 (three chunks) and Q = 45 (a partial wavefront)."""
    import torch
    for name in ("R147", "R45"):
        s = cases[name]
        B = s["B"]
        base = np.linspace(1.0, 2.0, B)
        v = np.unique(s[False]["risk"][:, STEP_RISK])
        cut = 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])  # between two candidates' values
        with _Map(cilqr, solver, s):
            whole = _host(solver, s, base=base, max_risk=cut)
            for b in (2, B - 1):
                one = _host(solver, s, sel=slice(b, b + 1), base=base[b:b + 1], max_risk=cut)
                assert _same(one, whole, sel_b=slice(b, b + 1)), (name, b)
            rev = _host(solver, s, sel=slice(None, None, -1), base=base[::-1], max_risk=cut)
            assert _same(rev, whole, sel_b=slice(None, None, -1)), name
        assert np.isnan(whole["total"]).any() and not np.isnan(whole["total"]).all(), name
        flat = np.stack([np.asfortranarray(s["layers"]).flatten(order="F")] * B)
        layers = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0")
        torch.cuda.synchronize()
        # one equal copy of the layer per solve; the pose stays the shared one (a per-solve pose's cos and sin are the device's)
        solver.set_uncertainty_map_device(layers.data_ptr(), cilqr.map_geom(*s["geom"]), s["poses"], s["probes"], layer_stride=flat.shape[1])
        try:
            per_solve = _host(solver, s, base=base, max_risk=cut)
        finally:
            solver.clear_uncertainty_map()
        assert _same(per_solve, whole), name


@gpu
def test_lost_steps(cilqr, solver, cases):
    """A NaN in x of one X_t and in one of the six entries of one Sigma_t — and one in an entry that is NOT read: the two steps are lost
    (r_t = 1, u_t = 1, e_t = 0, nothing for WORST_OCC), every other step and solve keeps its bits."""
    s = cases["R75"]
    B, N = s["B"], s["N"]
    X, sigma = s["X"].copy(), s["sigma"].copy()
    X[2, 4 * 3 + 0] = np.nan          # solve 2, step 3: x
    sigma[5, 7, 13] = np.inf          # solve 5, step 7: entry (1, 3)
    sigma[1, 4, 10] = np.nan          # solve 1, step 4: the speed's variance, not read
    X[3, 4 * 6 + 2] = np.nan          # solve 3, step 6: the speed, not read
    sigma[6, N, 0] = np.nan           # Sigma_N is not visited
    want = restate_map(s["p"], s["probes"], N, X, sigma, s["nodes"], s["weights"], s["g"], s["layers"], s["poses"], s["threshold"])
    lost = np.zeros((B, N), dtype=bool)
    lost[2, 3] = lost[5, 7] = True
    assert np.array_equal(want["lost"], lost)
    with _Map(cilqr, solver, s):
        got = _host(solver, s, X=X, sigma=sigma)
        clean = _host(solver, s)
    for n, v in (("step_risk", 1.0), ("step_unknown", 1.0), ("step_occ", 0.0)):
        assert np.all(got[n][lost] == v), n
        assert np.array_equal(_bits(got[n][~lost]), _bits(clean[n][~lost])), n
    others = [0, 1, 3, 4, 6, 7]
    assert _same(got, clean, sel_a=others, sel_b=others, names=OUT[:4])
    assert np.all(got["risk"][[2, 5], STEP_RISK] == 1.0) and np.all(got["risk"][[2, 5], UNKNOWN] == 1.0)
    d = np.abs(got["risk"] - want[False]["risk"])
    assert np.max(d[:, [STEP_RISK, SUM_RISK, UNKNOWN]]) <= TOL and np.max(d[:, [MEAN_OCC, WORST_OCC]]) <= OCC_TOL
    assert np.array_equal(got["risk"][:, FIRST_STEP], want[False]["risk"][:, FIRST_STEP])


def _device_pick(solver, values):
    import torch
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(np.ascontiguousarray(values)).to(dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    solver.argmin_device(torch.cuda.current_stream(dev).cuda_stream, len(values), v.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)
    return int(out.cpu().numpy()[1])


@gpu
def test_max_risk_bound_sum_and_the_pick(cilqr, solver, cases):
    """max_risk placed between the candidates' values (1e-6 below each distinct value, and midway), on CM_STEP_RISK and under BOUND_SUM on
    CM_SUM_RISK; a base with a NaN and an infinity: total is base or NaN bit for bit, and cilqr_argmin_device returns numpy's pick."""
    s = cases["R75"]
    B = s["B"]
    want = s[False]["risk"]
    base = np.linspace(3.0, 2.0, B)
    base[int(np.argmax(want[:, STEP_RISK]))] = 1.0  # cheapest where the risk is largest: the bound changes the pick
    base[0], base[1] = np.nan, np.inf
    picks = set()
    with _Map(cilqr, solver, s):
        for sum_bound in (False, True):
            v = np.unique(want[:, SUM_RISK if sum_bound else STEP_RISK])
            assert len(v) >= 3 and np.min(np.diff(v)) > 4e-6
            cuts = sorted(set((v - 1e-6).tolist() + (v + 1e-6).tolist() + (0.5 * (v[1:] + v[:-1])).tolist() + [-1.0, 1.0]))
            for cut in cuts:
                w = _total(want, base, cut, sum_bound)
                for form in ("host", "device"):
                    f = _host if form == "host" else _device
                    got = f(solver, s, flags=BOUND_SUM if sum_bound else 0, max_risk=cut, base=base)["total"]
                    _check_total(got, w, (sum_bound, cut, form))
                    assert _device_pick(solver, got) == _pick(w), (sum_bound, cut, form)
                picks.add(_pick(w))
    assert -1 in picks and len(picks) >= 3
    assert np.any(want[:, SUM_RISK] > want[:, STEP_RISK] + 1e-3)  # the two bounds differ on this scene


@gpu
def test_the_kernel_reproduces_the_rollouts_marginals(cilqr, solver, cases):
    """The kernel itself, without the restatement: scene R on case A's map with the S = 1000 draws as equal-weight nodes against the
    oracle's rollouts' per-step share, at the bound of test_the_restatement_reproduces_the_rollouts_marginals (twice the 0.007 measured on
    the CPU).  Q = 1000: sixteen chunks, the last partial."""
    s = cases["S"]
    with _Map(cilqr, solver, s):
        got = _host(solver, s)
    d = np.abs(got["step_risk"] - s["share"])
    print("max |r_t - rollouts' share| %.4g; kernel vs restatement %.3g" % (d.max(), np.max(np.abs(got["step_risk"] - s[False]["step_risk"]))))
    assert d.max() <= 2 * ROLLOUT_MEASURED
    _check_against(got, s[False], "case S")


@gpu
def test_limits(cilqr, cases):
    """No map set: CILQR_ERR_ARG, saying so.  B or N beyond the handle's: CILQR_ERR_ARG.  A host call beyond the arena: CILQR_ERR_ARG, and
    the handle stays usable.  The largest horizon a handle takes runs: LDS does not grow with N."""
    s = cases["R75"]
    sv = cilqr.Solver(_params(cilqr), max_batch=4, max_horizon=s["N"], max_obstacles=0, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*no uncertainty map" % ERR_ARG):
            _host(sv, s, sel=slice(0, 4))
        with _Map(cilqr, sv, s):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: B=8 outside" % ERR_ARG):
                _host(sv, s)
            big = dict(s)
            big["nodes"], big["weights"] = np.zeros((1024, 3)), np.full(1024, 1.0 / 1024)
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers" % ERR_ARG):
                _host(sv, big, sel=slice(0, 4))  # 4*(23*12 + 30) + 4096 doubles against 4*(22*12 + 34)
            got = _host(sv, s, sel=slice(0, 3))
            _check_against(got, s[False], "3 solves on a handle of 4", sel=slice(0, 3))
    finally:
        sv.close()
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    N = int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1))
    B = 2  # (with the per-step outputs the host form fits for B <= 7*max_batch/8)
    sv = cilqr.Solver(_params(cilqr, N), max_batch=B + 1, max_horizon=N, max_obstacles=0, device=0)
    try:
        with _Map(cilqr, sv, s):
            X = np.zeros((B, 4 * (N + 1)))
            X[:, 0::4] = np.linspace(0.0, 10.0, N + 1)
            sigma = np.zeros((B, N + 1, 16))
            sigma[:, :, [0, 5]], sigma[:, :, 15] = 0.16 ** 2, 0.017 ** 2
            got = sv.chance_risk_map(N, X, sigma, s["nodes"], s["weights"], 50.0)
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: N=%d outside" % (ERR_ARG, N + 1)):
                sv.chance_risk_map(N + 1, np.zeros((B, 4 * (N + 2))), np.zeros((B, N + 2, 16)), s["nodes"], s["weights"], 50.0)
        assert got["step_risk"].shape == (B, N) and np.all(np.isfinite(got["risk"][:, WORST_OCC]))
        assert np.array_equal(_bits(got["step_occ"][0]), _bits(got["step_occ"][1]))
    finally:
        sv.close()


def _restated_pick_of_the_dump(O, path):
    """What tests/cpp/candidates_chance_map.cpp wrote -> the restated map risk and pick for the candidates it solved: Sigma_t by `restate`
    from the dumped plans and gains, then restate_map on the dumped layer with the dumped nodes."""
    v = open(path).read().split()
    B, N, Q, rows, cols = (int(x) for x in v[:5])
    a = np.array([float(x) for x in v[5:]])
    take = lambda n, at=[0]: (a[at[0]:at[0] + n], at.__setitem__(0, at[0] + n))[0]  # noqa: E731
    threshold, max_risk, best = take(1)[0], take(1)[0], int(take(1)[0])
    geom, pose = tuple(take(5)), tuple(take(3))
    X, U, K = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1), take(B * 8 * N).reshape(B, -1)
    base, sigma0 = take(B), take(16)
    nodes, weights = take(Q * 3).reshape(Q, 3), take(Q)
    risk, step = take(B * 8).reshape(B, 8), take(B * N).reshape(B, N)
    layer = take(rows * cols).astype(np.float32).reshape(cols, rows).T  # written column-major
    p = O.default_params(N)
    sigma = restate(p, N, X, U, K, sigma0, None, None, None)["sigma"]
    s = _mk(dict(p=p, X=X), N, sigma, (nodes, weights), geom, (3, 3), threshold, layer, pose, O)
    s.update(best=best, max_risk=max_risk, base=base, got=dict(risk=risk, step_risk=step))
    return s


@gpu
def test_cpp_facade_map_covariance_checked_candidates(cilqr, oracle, tmp_path):
    """tests/cpp/candidates_chance_map.cpp: iLQR::run_candidates under set_pose_covariance_check + set_uncertainty_map +
    set_map_covariance_check against the C-ABI sequence called by hand (inside the program: picks, last_chance_map_risk bit for bit, no
    map, check off, all rejected, composition with set_map_risk_check) and against the restated map risk and pick for the candidates it
    solved (here), with the conditions on the occupancies asserted for its scene.  The nodes it built are numpy's."""
    exe, dump = str(tmp_path / "candidates_chance_map"), str(tmp_path / "dump.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_chance_map.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map covariance pick ok" in r.stdout, r.stdout
    s = _restated_pick_of_the_dump(oracle, dump)
    want = s[False]
    zn, wn = np_quadrature(5, 5, 3)
    assert np.max(np.abs(s["nodes"] - zn)) <= 1e-13 and np.max(np.abs(s["weights"] - wn)) <= 1e-13
    gap = float(np.min(np.abs(s["occ"][s["ok"]] - s["threshold"])))
    print("min|occ - thr| %.3g, restated STEP_RISK %s" % (gap, np.round(want["risk"][:, STEP_RISK], 6).tolist()))
    assert gap > MARGIN
    for dx, dy in ((MARGIN, 0.0), (-MARGIN, 0.0), (0.0, MARGIN), (0.0, -MARGIN)):
        assert np.array_equal(np_lookup(s["layers"], s["g"], s["qx"] + dx, s["qy"] + dy)[1], s["ok"])
    assert np.min(np.abs(want["risk"][:, STEP_RISK] - s["max_risk"])) > MARGIN
    got = s["got"]
    assert np.max(np.abs(got["step_risk"] - want["step_risk"])) <= TOL
    d = np.abs(got["risk"] - want["risk"])
    assert np.max(d[:, [STEP_RISK, SUM_RISK, UNKNOWN]]) <= TOL and np.max(d[:, [MEAN_OCC, WORST_OCC]]) <= OCC_TOL
    assert np.array_equal(got["risk"][:, FIRST_STEP], want["risk"][:, FIRST_STEP])
    worst, _ = _decided(want)
    assert np.array_equal(got["risk"][worst, WORST_STEP], want["risk"][worst, WORST_STEP])
    total = _total(want["risk"], s["base"], s["max_risk"])
    assert np.isnan(total).any() and not np.isnan(total).all()
    assert s["best"] == _pick(total)
