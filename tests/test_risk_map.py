"""Map rollout risk (cilqr_rollout_risk_map*, include/cilqr.h): the share of S closed-loop rollouts per solve whose footprint probes
enter cells of the uncertainty map above an occupancy threshold, the worst occupancy touched with its row and entry, the hits per step
and the rollouts that leave the known map.

Expected values come from the CPU oracle's exported pieces plus numpy, never from the HIP path: o_gains, o_rollout and the scenes of
tests/test_rollout_risk.py; the probe positions restated in numpy from the header's definition (body offsets a_k, b_l on safe_length x
safe_width = 1.1 x 0.9 turned by the state's heading, a rigid transform into the map frame); the lookup by a vectorised numpy restatement of
oracle.layer_bilinear, asserted equal to it on every probe of case A.  Counts, steps, rows, entries, shares and picks are compared
exactly; MR_WORST_OCC within 1e-7 absolute (the suite's 1e-9 on c, and here c = occupancy/100 - 1).  What makes the exact comparisons
meaningful is asserted on the oracle's numbers in CPU tests: every valid probe's |occupancy - threshold| > 1e-6, the worst-row gap and
the worst-entry gap within the worst row > 1e-6, every probe's validity unchanged at the four points displaced by 1e-6 m in x and y.

Layers are smooth and seeded (five Gaussian bumps through 100*tanh(z/100), 12 NaN cells): no plateaus, so no ties.

  case A   scene R (B 8, N 12), S = 70, the scene's offsets, k_scale 0; map 160 x 80 at 0.1 m centred (6, 0), pose (0, 0, 0.05), probes
           3 x 3, threshold 50: one wavefront and a 6-row tail
  case B   the same, S = 300: two workgroups per solve (256 + 44 rows) and the finish kernel
  case C1, C23  scene R, S = 70, per-solve layers (seeds 1..8) and poses through set_uncertainty_map_device; probes 1 x 1 and 2 x 3
  case D   scene R, S = 70, a map that ends inside the horizon (30 x 80 cells centred (1, 0)), threshold 100 (no cell reaches it)
  case N2  the first two steps of case A
  case L   scene L (B 6, N 50), S = 64, k_scale 1; map 300 x 100 at 0.2 m centred (30, 0), pose (-20, 0.3, 0.05): the workload's horizon

The kernel's LDS, 8*(14*N + 4) + 4*N + 160 bytes, stays below 64 KiB up to N = 563, and a handle takes N <= CILQR_MAX_HORIZON = 384: no
accepted horizon reaches CILQR_ERR_UNSUPPORTED.  test_limits asserts the formula's verdict at the largest horizon a handle takes.
"""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import _bits
from test_rollout_risk import _pick, _scene_l, _scene_r, o_gains, o_rollout

gpu = pytest.mark.gpu

OCC_TOL, MARGIN = 1e-7, 1e-6
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_rollout_risk_map", "cilqr_rollout_risk_map_device")
FIELDS = ("COLLISION", "WORST_OCC", "WORST_ROW", "WORST_ENTRY", "FIRST_STEP", "STEP_SHARE", "UNKNOWN")
MR_COLLISION, MR_WORST_OCC, MR_WORST_ROW, MR_WORST_ENTRY, MR_FIRST_STEP, MR_STEP_SHARE, MR_UNKNOWN = range(7)
SAFE = (1.1, 0.9)  # safe_length, safe_width: the launch file's values (ilqr/launch/Experiment.launch:7-8)
GEOM_A, POSE_A = (16.0, 8.0, 0.1, 6.0, 0.0), (0.0, 0.0, 0.05)
GEOM_D = (3.0, 8.0, 0.1, 1.0, 0.0)
GEOM_L, POSE_L = (60.0, 20.0, 0.2, 30.0, 0.0), (-20.0, 0.3, 0.05)
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


# ---- expected values: the oracle's rollouts, numpy probes, a numpy lookup checked against the oracle's --------------------------
def smooth_layer(rows, cols, seed):
    """(rows, cols) float32: five Gaussian bumps through 100*tanh(z/100), then 12 NaN cells."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = np.zeros((rows, cols))
    for _ in range(5):
        ci, cj = rng.uniform(0, rows), rng.uniform(0, cols)
        si, sj = rng.uniform(rows / 16, rows / 6), rng.uniform(cols / 10, cols / 4)
        amp = rng.uniform(40, 100)
        z += amp * np.exp(-0.5 * (((i - ci) / si) ** 2 + ((j - cj) / sj) ** 2))
    layer = (100.0 * np.tanh(z / 100.0)).astype(np.float32)
    ni = rng.integers(0, rows, 12)
    nj = rng.integers(0, cols, 12)
    layer[ni, nj] = np.nan
    return layer


def probe_positions(p, probes, states, pose):
    """The header's footprint at states (..., 4) -> map-frame positions qx, qy (..., P), probe q = k*probes_w + l."""
    nl, nw = probes
    a = np.array([-0.5 * p.safe_length + k * (p.safe_length / (nl - 1)) if nl > 1 else 0.0 for k in range(nl)])
    b = np.array([-0.5 * p.safe_width + l * (p.safe_width / (nw - 1)) if nw > 1 else 0.0 for l in range(nw)])
    a, b = np.repeat(a, nw), np.tile(b, nl)
    x, y, th = states[..., 0:1], states[..., 1:2], states[..., 3:4]
    ct, st = np.cos(th), np.sin(th)
    Px, Py = x + (a * ct - b * st), y + (a * st + b * ct)
    dx, dy = Px - pose[0], Py - pose[1]
    cp, sp = np.cos(pose[2]), np.sin(pose[2])
    return cp * dx + sp * dy, cp * dy - sp * dx


def np_lookup(layer, g, qx, qy):
    """oracle_layer_bilinear restated on arrays: (occupancy, ok); the occupancy of a probe that is not ok is NaN."""
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    inv_res = 1.0 / g.res
    with np.errstate(invalid="ignore"):
        fi, fj = (x_first - qx) * inv_res, (y_first - qy) * inv_res
        inside = (fi >= 0.0) & (fj >= 0.0) & (fi < float(g.rows - 1)) & (fj < float(g.cols - 1))
    i0, j0 = np.where(inside, fi, 0.0).astype(np.int64), np.where(inside, fj, 0.0).astype(np.int64)
    ti, tj = fi - i0, fj - j0
    lay = np.asarray(layer, dtype=np.float32).astype(np.float64)
    f00, f10, f01, f11 = lay[i0, j0], lay[i0 + 1, j0], lay[i0, j0 + 1], lay[i0 + 1, j0 + 1]
    ok = inside & np.isfinite(f00) & np.isfinite(f10) & np.isfinite(f01) & np.isfinite(f11)
    with np.errstate(invalid="ignore"):
        a0, a1 = f00 + ti * (f10 - f00), f01 + ti * (f11 - f01)
        occ = a0 + tj * (a1 - a0)
    return np.where(ok, occ, np.nan), ok


def reduce_map(occ, ok, lost, S, threshold, unknown_hits):
    """occ, ok (B, S, N, P), lost (B, S, N) -> what the call returns, by numpy."""
    B, _, N, P = occ.shape
    unknown = (~ok).any(axis=3)                                      # (B, S, N)
    hit = (ok & (occ > threshold)).any(axis=3) | lost
    if unknown_hits:
        hit = hit | unknown
    step_hits, unknown_steps = hit.sum(axis=1).astype(np.int32), unknown.sum(axis=1).astype(np.int32)
    risk = np.zeros((B, 7))
    risk[:, MR_COLLISION] = hit.any(axis=2).sum(axis=1) / S
    risk[:, MR_UNKNOWN] = unknown.any(axis=2).sum(axis=1) / S
    any_step = step_hits > 0
    risk[:, MR_FIRST_STEP] = np.where(any_step.any(axis=1), any_step.argmax(axis=1), -1)
    risk[:, MR_STEP_SHARE] = step_hits.max(axis=1) / S
    flat = np.where(ok, occ, -np.inf).transpose(0, 1, 3, 2).reshape(B, S, P * N)   # entry index q*N + t
    row_max = flat.max(axis=2)
    rows = row_max.argmax(axis=1)                                    # the lowest row on equal values
    none = ~ok.reshape(B, -1).any(axis=1)
    risk[:, MR_WORST_OCC] = row_max.max(axis=1)
    risk[:, MR_WORST_ROW] = np.where(none, -1, rows)
    risk[:, MR_WORST_ENTRY] = np.where(none, -1, [int(flat[b, rows[b]].argmax()) for b in range(B)])
    return dict(risk=risk, step_hits=step_hits, unknown_steps=unknown_steps, hit_rows=hit.any(axis=2).sum(axis=1),
                unknown_rows=unknown.any(axis=2).sum(axis=1), flat=flat)


def _case(O, s, S, delta, k_scale, geom, probes, threshold, layers, poses, N=None):
    """One case on scene `s` (gains already there): the oracle's rollouts from `delta` (S, 4), the probes of every visited state and
    their occupancies.  layers / poses: one (rows, cols) layer and one pose shared by the solves, or lists of B of each."""
    B, p = s["B"], copy.copy(s["p"])
    p.safe_length, p.safe_width = SAFE  # (read by the probes alone)
    X, U, k, K = s["X"], s["U"], s["k"], s["K"]
    if N is None:
        N = s["N"]
    else:  # the first N steps of the same trajectories and gains
        X, U = np.ascontiguousarray(X[:, :4 * (N + 1)]), np.ascontiguousarray(U[:, :2 * N])
        k, K = np.ascontiguousarray(k[:, :2 * N]), np.ascontiguousarray(K[:, :8 * N])
    d = np.ascontiguousarray(np.broadcast_to(delta, (B, S, 4)))
    Xr, Ur = o_rollout(O, p, N, X, U, k, K, d, k_scale)
    states = Xr.reshape(B, S, N + 1, 4)[:, :, :N]
    lost = ~(np.isfinite(states).all(axis=3) & np.isfinite(Ur.reshape(B, S, N, 2)).all(axis=3))
    g = O.map_geom(*geom)
    per_solve = isinstance(layers, list)
    P = probes[0] * probes[1]
    occ, ok = np.zeros((B, S, N, P)), np.zeros((B, S, N, P), dtype=bool)
    qx, qy = np.zeros((B, S, N, P)), np.zeros((B, S, N, P))
    for b in range(B):
        qx[b], qy[b] = probe_positions(p, probes, states[b], poses[b] if per_solve else poses)
        occ[b], ok[b] = np_lookup(layers[b] if per_solve else layers, g, qx[b], qy[b])
    ok &= np.isfinite(states).all(axis=3)[..., None]  # a state that is not finite has no valid probe
    out = dict(B=B, N=N, S=S, X=X, U=U, k=k, K=K, delta=np.ascontiguousarray(delta), k_scale=k_scale, geom=geom, probes=probes,
               threshold=threshold, layers=layers, poses=poses, p=p, states=states, occ=occ, ok=ok, lost=lost, qx=qx, qy=qy, g=g)
    out[False] = reduce_map(occ, ok, lost, S, threshold, False)
    out[True] = reduce_map(occ, ok, lost, S, threshold, True)
    return out


def _c_poses(B):
    return [(0.05 * b, -0.03 * b, 0.05 - 0.01 * b) for b in range(B)]


@pytest.fixture(scope="module")
def cases(oracle):
    """Every case's oracle rollouts, probes, occupancies and reductions (both flags).  Computed once; never modified."""
    from cilqr_amd import scenes
    O = oracle
    r, l = _scene_r(O), _scene_l(O)
    for s in (r, l):
        s["k"], s["K"], ok = o_gains(O, s["p"], s["N"], s["X"], s["U"], s["poly"], s["fl"], s["pose"], s["dim"], None, 1.0)
        assert np.all(ok == 1)
    la, ld, ll = smooth_layer(160, 80, 3), smooth_layer(30, 80, 3), smooth_layer(300, 100, 3)
    lc = [smooth_layer(160, 80, seed) for seed in range(1, r["B"] + 1)]
    out = {"A": _case(O, r, 70, r["delta"], 0.0, GEOM_A, (3, 3), 50.0, la, POSE_A),
           "B": _case(O, r, 300, scenes.pose_offsets(300, 0.16, 0.16, 0.017, seed=5), 0.0, GEOM_A, (3, 3), 50.0, la, POSE_A),
           "C1": _case(O, r, 70, r["delta"], 0.0, GEOM_A, (1, 1), 50.0, lc, _c_poses(r["B"])),
           "C23": _case(O, r, 70, r["delta"], 0.0, GEOM_A, (2, 3), 50.0, lc, _c_poses(r["B"])),
           "D": _case(O, r, 70, r["delta"], 0.0, GEOM_D, (3, 3), 100.0, ld, POSE_A),
           "N2": _case(O, r, 70, r["delta"], 0.0, GEOM_A, (3, 3), 50.0, la, POSE_A, N=2),
           "L": _case(O, l, 64, l["delta"], 1.0, GEOM_L, (3, 3), 50.0, ll, POSE_L)}
    out["scene_r"] = r
    return out


CASES = ["A", "B", "C1", "C23", "D", "N2", "L"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cilqr.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_MAP_RISK_FIELDS\s+7\b", h)
    assert re.search(r"#define\s+CILQR_MAP_RISK_UNKNOWN_HITS\s+1u\b", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_MR_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "MR_" + name) == i
    assert cilqr.MAP_RISK_FIELDS == 7 and cilqr.MAP_RISK_UNKNOWN_HITS == 1
    assert callable(cilqr.Solver.rollout_risk_map) and callable(cilqr.Solver.rollout_risk_map_device)
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_map_risk_check\s*\(\s*double\s+occ_threshold\s*,\s*double\s+max_risk\s*,\s*bool\s+unknown_hits\s*=\s*false\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_map_risk\s*;", f)
    assert re.search(r"std::vector<int32_t>\s+last_map_step_hits\s*,\s*last_map_unknown_hits\s*;", f)
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    assert "8*(14*N + 4) + 4*N + 160" in full  # the LDS formula is stated
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_rollout_risk_map\s*\(", plan)


def test_argument_errors_need_no_device(cilqr):
    """NULL required pointers, total without base, S < 1, a negative stride, a NaN k_scale, occ_threshold or max_risk, unknown flag
    bits: CILQR_ERR_ARG, decided before the handle is looked at (there is none here)."""
    L = cilqr.lib()
    B, N, S = 2, 4, 3
    X, U, k, K = np.zeros((B, 4 * (N + 1))), np.zeros((B, 2 * N)), np.zeros((B, 2 * N)), np.zeros((B, 8 * N))
    delta = np.zeros((S, 4))
    risk, hits, unk = np.zeros((B, 7)), np.zeros((B, N), dtype=np.int32), np.zeros((B, N), dtype=np.int32)
    total, base = np.zeros(B), np.zeros(B)
    no_handle = C.c_void_p()
    d = C.c_double
    nan = float("nan")

    def call(dev, S_=S, stride=0, ks=0.0, thr=50.0, flags=0, mr=1.0, **nulls):
        a = dict(X=X, U=U, k=k, K=K, delta=delta, risk=risk, base=base, total=total)
        a.update(nulls)
        f = L.cilqr_rollout_risk_map_device if dev else L.cilqr_rollout_risk_map
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, S_, _p(a["X"]), _p(a["U"]), _p(a["k"]), _p(a["K"]), _p(a["delta"]), C.c_int64(stride), d(ks), d(thr),
                 C.c_uint32(flags), d(mr), _p(a["base"]), _p(a["risk"]), _p(hits, _ip), _p(unk, _ip), _p(a["total"]))

    for dev in (False, True):
        for name in ("X", "U", "k", "K", "delta", "risk"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, base=None) == ERR_ARG and b"total needs base" in L.cilqr_last_error()
        assert call(dev, S_=0) == ERR_ARG and b"S >= 1" in L.cilqr_last_error()
        assert call(dev, stride=-1) == ERR_ARG and b"negative stride" in L.cilqr_last_error()
        for kw in ("ks", "thr", "mr"):
            assert call(dev, **{kw: nan}) == ERR_ARG and b"NaN" in L.cilqr_last_error(), kw
        assert call(dev, flags=2) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        assert call(dev, flags=1) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, base=None, total=None) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # neither: valid too


def test_the_numpy_lookup_is_the_oracles(oracle, cases):
    """np_lookup against oracle.layer_bilinear on every probe of case A (8 x 70 x 12 x 9), and at positions around the map's edges and
    its NaN cells: the same validity, the same bits."""
    s = cases["A"]
    qx, qy = s["qx"].ravel(), s["qy"].ravel()
    g = s["g"]
    edge = np.array([-2.0, -1.95, -1.9499999, 13.9, 13.94999, 13.95, 14.0, np.nan, np.inf])
    qx, qy = np.concatenate([qx, edge, np.full(edge.size, 3.0)]), np.concatenate([qy, np.full(edge.size, 0.3), edge / 3.5])
    v, _, _, ok = oracle.layer_bilinear(s["layers"], g, qx, qy)
    occ, ok2 = np_lookup(s["layers"], g, qx, qy)
    assert np.array_equal(ok, ok2) and ok.any() and not ok.all()
    assert np.array_equal(_bits(v[ok]), _bits(occ[ok]))


def test_the_host_form_fits_the_arena_at_the_promised_shapes(tmp_path):
    """tests/cpp/host_plan_risk_map.cpp: plan_rollout_risk_map laid out without an arena against host_arena_bytes, at B = max_batch,
    N = max_horizon and (delta_batch_stride ? B : 1)*S = max_batch*max_horizon, shared and per-solve offsets, with every output asked
    for — the shapes include/cilqr.h says always fit."""
    exe = str(tmp_path / "host_plan_risk_map")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_risk_map.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout


@pytest.mark.parametrize("name", CASES)
def test_conditions(cases, name):
    """What keeps the exact comparisons of the GPU tests from hiding a failure, on the oracle's numbers alone."""
    s = cases[name]
    B, S, N = s["B"], s["S"], s["N"]
    occ, ok = s["occ"], s["ok"]
    r = s[False]
    print("case %s: hit rows %s, unknown rows %s, min|occ - thr| %.3g" % (name, r["hit_rows"].tolist(), r["unknown_rows"].tolist(),
                                                                        np.min(np.abs(occ[ok] - s["threshold"]))))
    assert not s["lost"].any()
    assert np.min(np.abs(occ[ok] - s["threshold"])) > MARGIN          # every occupancy that decides a hit
    flat = r["flat"]
    row_max = np.sort(flat.max(axis=2), axis=1)
    assert np.all(np.isfinite(row_max[:, -1]))                        # every solve has a valid probe
    gap = row_max[:, -1] - row_max[:, -2]
    ent = np.sort(np.stack([flat[b, int(r["risk"][b, MR_WORST_ROW])] for b in range(B)]), axis=1)
    egap = ent[:, -1] - ent[:, -2] if ent.shape[1] > 1 else np.full(B, np.inf)
    print("  smallest worst-row gap %.3g, smallest entry gap %.3g" % (np.min(gap), np.min(egap)))
    assert np.min(gap) > MARGIN and np.min(egap) > MARGIN
    per_solve = isinstance(s["layers"], list)
    for dx, dy in ((MARGIN, 0.0), (-MARGIN, 0.0), (0.0, MARGIN), (0.0, -MARGIN)):   # validity is decided
        for b in range(B):
            _, okd = np_lookup(s["layers"][b] if per_solve else s["layers"], s["g"], s["qx"][b] + dx, s["qy"][b] + dy)
            assert np.array_equal(okd, ok[b]), (b, dx, dy)
    share, unknown = r["risk"][:, MR_COLLISION], r["risk"][:, MR_UNKNOWN]
    if name in ("A", "B"):
        assert np.any((share > 0) & (share < 1)) and np.any((unknown > 0) & (unknown < 1))
    if name == "D":  # the map ends inside the horizon: unknown counts rise, nothing hits without the flag, the flag makes hits
        assert np.all(r["unknown_steps"][:, -1] == S) and np.all(r["unknown_steps"].min(axis=1) < S // 2)
        assert np.all(r["unknown_steps"].argmin(axis=1) < N - 1)
        assert not r["step_hits"].any() and np.array_equal(s[True]["step_hits"], r["unknown_steps"])
    if name in ("C1", "C23"):  # solve b's own layer and pose matter: with layer 0 and pose 0 every other solve would count otherwise
        for b in range(1, B):
            occ0, ok0 = np_lookup(s["layers"][0], s["g"], *probe_positions(s["p"], s["probes"], s["states"][b], s["poses"][0]))
            alt = reduce_map(occ0[None], ok0[None], s["lost"][b:b + 1], S, s["threshold"], False)
            assert not (np.array_equal(alt["step_hits"][0], r["step_hits"][b]) and np.array_equal(alt["unknown_steps"][0], r["unknown_steps"][b])
                        and alt["risk"][0, MR_WORST_OCC] == r["risk"][b, MR_WORST_OCC]), b
    assert np.all(r["risk"][:, MR_WORST_ENTRY] < s["probes"][0] * s["probes"][1] * N)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _params(cilqr, horizon=None):
    p = cilqr.default_params(horizon)
    p.safe_length, p.safe_width = SAFE
    return p


@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(_params(cilqr), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    yield s
    s.close()


class _Map:
    """The case's map set on the solver: the host form for a shared layer, the device form (torch buffers kept here) for per-solve ones."""

    def __init__(self, cilqr, solver, s, sel=None):
        self.solver = solver
        g = cilqr.map_geom(*s["geom"])
        if isinstance(s["layers"], list):
            import torch
            idx = range(s["B"]) if sel is None else sel
            flat = np.stack([np.asfortranarray(s["layers"][b]).flatten(order="F") for b in idx])
            self.layers = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0")
            self.poses = torch.from_numpy(np.ascontiguousarray([s["poses"][b] for b in idx], dtype=np.float64)).to("cuda:0")
            torch.cuda.synchronize()
            solver.set_uncertainty_map_device(self.layers.data_ptr(), g, (0.0, 0.0, 0.0), s["probes"], layer_stride=flat.shape[1],
                                              poses_ptr=self.poses.data_ptr())
        else:
            solver.set_uncertainty_map(s["layers"], g, s["poses"], s["probes"])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.solver.clear_uncertainty_map()


def _host(solver, s, sel=slice(None), delta=None, unknown_hits=False, max_risk=1.0, base=None, X=None):
    return solver.rollout_risk_map(s["N"], (s["X"] if X is None else X)[sel], s["U"][sel], s["k"][sel], s["K"][sel],
                                   s["delta"] if delta is None else delta, s["threshold"], k_scale=s["k_scale"], max_risk=max_risk, base=base,
                                   unknown_hits=unknown_hits)


def _device(solver, s, unknown_hits=False, max_risk=1.0, base=None):
    """The device form on torch buffers: (risk, step_hits, unknown_hits, total)."""
    import torch
    B, N, S = s["B"], s["N"], s["S"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    t = {n: torch.from_numpy(np.ascontiguousarray(s[n])).to(dev) for n in ("X", "U", "k", "K", "delta")}
    z = lambda *shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    risk, hits, unk, total = z(B, 7), z(B, N, dt=torch.int32), z(B, N, dt=torch.int32), z(B)
    tb = None if base is None else torch.from_numpy(np.ascontiguousarray(base)).to(dev)
    torch.cuda.synchronize(dev)
    solver.rollout_risk_map_device(stream, B, N, S, t["X"].data_ptr(), t["U"].data_ptr(), t["k"].data_ptr(), t["K"].data_ptr(),
                                   t["delta"].data_ptr(), 0, s["threshold"], risk.data_ptr(), hits.data_ptr(), unk.data_ptr(),
                                   total.data_ptr() if tb is not None else 0, tb.data_ptr() if tb is not None else 0, k_scale=s["k_scale"],
                                   max_risk=max_risk, flags=1 if unknown_hits else 0)
    torch.cuda.synchronize(dev)
    out = [a.cpu().numpy() for a in (risk, hits, unk, total)]
    if tb is None:
        out[3] = None
    return out


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


def _check_against(got, want, S, what):
    risk, hits, unk = got[:3]
    print("%s: hit rows %s, unknown rows %s, |WORST_OCC - oracle| max %.3g" % (
        what, np.rint(risk[:, MR_COLLISION] * S).astype(int).tolist(), np.rint(risk[:, MR_UNKNOWN] * S).astype(int).tolist(),
        np.max(np.abs(risk[:, MR_WORST_OCC] - want["risk"][:, MR_WORST_OCC]))))
    assert hits.dtype == np.int32 and unk.dtype == np.int32
    assert np.array_equal(hits, want["step_hits"]), what
    assert np.array_equal(unk, want["unknown_steps"]), what
    for f in (MR_COLLISION, MR_UNKNOWN, MR_FIRST_STEP, MR_STEP_SHARE, MR_WORST_ROW, MR_WORST_ENTRY):
        assert np.array_equal(risk[:, f], want["risk"][:, f]), (what, FIELDS[f], risk[:, f], want["risk"][:, f])
    assert np.max(np.abs(risk[:, MR_WORST_OCC] - want["risk"][:, MR_WORST_OCC])) <= OCC_TOL, what


@gpu
@pytest.mark.parametrize("name", ["A", "B", "D", "N2", "L"])
def test_fields_against_the_oracle(cilqr, solver, cases, name):
    """A shared map, host and device forms, both flags: counts, steps, shares, rows and entries exact, WORST_OCC within 1e-7; the two
    forms give the same bits."""
    s = cases[name]
    with _Map(cilqr, solver, s):
        for flag in (False, True):
            host = _host(solver, s, unknown_hits=flag)
            assert host[3] is None
            _check_against(host, s[flag], s["S"], "case %s, host form, unknown_hits %s" % (name, flag))
            dev = _device(solver, s, unknown_hits=flag)
            _check_against(dev, s[flag], s["S"], "case %s, device form, unknown_hits %s" % (name, flag))
            assert _same(host[:3], dev[:3])
            if name == "D":  # no cell reaches the threshold: nothing hits without the flag, every unknown row hits with it
                assert np.array_equal(host[1], host[2] if flag else np.zeros_like(host[1])) and host[2][:, -1].all()


@gpu
@pytest.mark.parametrize("name", ["C1", "C23"])
def test_per_solve_layers_and_poses(cilqr, solver, cases, name):
    """set_uncertainty_map_device with layer_stride = rows*cols and poses [B][3]: solve b reads layer b with pose b — also when it sits
    elsewhere in a batch whose layers and poses travel with it."""
    s = cases[name]
    with _Map(cilqr, solver, s):
        for flag in (False, True):
            _check_against(_device(solver, s, unknown_hits=flag), s[flag], s["S"], "case %s, unknown_hits %s" % (name, flag))
        whole = _host(solver, s)  # (the host form of the CALL on a map set through the device form)
        _check_against(whole, s[False], s["S"], "case %s, host form" % name)
    counts = s[False]["step_hits"].sum(axis=1) + s[False]["unknown_steps"].sum(axis=1)
    assert len(set(counts.tolist())) > 1  # the solves differ: one layer and pose for all would not pass
    order = [5, 1, 7, 0, 2]
    t = dict(s)
    for n in ("X", "U", "k", "K"):
        t[n] = np.ascontiguousarray(s[n][order])
    t["B"] = len(order)
    with _Map(cilqr, solver, s, sel=order):
        moved = _host(solver, t)
    assert _same(moved[:3], [a[order] for a in whole[:3]])


@gpu
def test_a_result_depends_on_its_own_solve_alone(cilqr, solver, cases):
    """One solve alone, the batch reversed, the whole batch, and a per-solve copy of the shared offsets: identical bits per solve in
    every output.  S = 300: two workgroups per solve and the finish kernel; S = 70: the one-workgroup path."""
    for name in ("B", "A"):
        s = cases[name]
        B, S = s["B"], s["S"]
        with _Map(cilqr, solver, s):
            base = np.linspace(1.0, 2.0, B)
            whole = _host(solver, s, base=base, max_risk=0.5)
            for b in (2, B - 1):
                one = _host(solver, s, sel=slice(b, b + 1), base=base[b:b + 1], max_risk=0.5)
                assert _same([a[0] for a in one], [a[b] for a in whole]), (name, b)
            rev = _host(solver, s, sel=slice(None, None, -1), base=base[::-1], max_risk=0.5)
            assert _same([a[::-1] for a in rev], whole), name
            dense = _host(solver, s, delta=np.ascontiguousarray(np.broadcast_to(s["delta"], (B, S, 4))), base=base, max_risk=0.5)
            assert _same(dense, whole), name
        assert np.isnan(whole[3]).any() and not np.isnan(whole[3]).all()


@gpu
def test_a_nan_solve_hits_everywhere_is_unknown_and_never_wins(cilqr, solver, cases):
    """A solve whose X holds a NaN — x of its first state in one solve, the SPEED of its first state in another (its probes at step 0
    could be looked up, and are not: a state that is not finite has no valid probe): every row hits from that step on, its probes
    there count as unknown, it has no worst occupancy, and the other solves' bits are untouched."""
    s = cases["A"]
    B, S, N = s["B"], s["S"], s["N"]
    bad = [2, 4]
    X = s["X"].copy()
    X[2, 0] = np.nan
    X[4, 2] = np.nan
    occ, ok, lost = s["occ"].copy(), s["ok"].copy(), s["lost"].copy()
    ok[bad], lost[bad] = False, True
    want = reduce_map(occ, ok, lost, S, s["threshold"], False)
    assert np.all(want["step_hits"][bad] == S) and np.all(want["unknown_steps"][bad] == S)
    assert np.all(np.isneginf(want["risk"][bad, MR_WORST_OCC])) and np.all(want["risk"][bad][:, [MR_WORST_ROW, MR_WORST_ENTRY]] == -1)
    with _Map(cilqr, solver, s):
        got = _host(solver, s, X=X)
        clean = _host(solver, s)
    others = np.setdiff1d(np.arange(B), bad)
    assert np.all(np.isneginf(got[0][bad, MR_WORST_OCC]))
    assert np.array_equal(np.delete(got[0], MR_WORST_OCC, axis=1)[bad], np.delete(want["risk"], MR_WORST_OCC, axis=1)[bad])
    assert np.array_equal(got[1][bad], want["step_hits"][bad]) and np.array_equal(got[2][bad], want["unknown_steps"][bad])
    assert _same([a[others] for a in got[:3]], [a[others] for a in clean[:3]])
    _check_against([a[others] for a in got[:3]], {k: v[others] for k, v in want.items() if k in ("risk", "step_hits", "unknown_steps")}, S,
                   "the other solves")


@gpu
def test_worst_occupancy_is_the_map_costs_own_lookup(cilqr, solver, cases):
    """Probes 1 x 1, S = 1, a zero offset, k_scale 0 on trajectories the device's own dynamics produced (the zero-offset rollout of scene
    R reproduces itself): every visited state is the nominal state bit for bit, so q1*exp(q2*(MR_WORST_OCC/100 - 1)) is the maximum
    over t < N of cilqr_debug_uncertainty_cost at the nominal states within 1e-9 relative, and MR_WORST_ENTRY's step is that argmax."""
    s = cases["A"]
    B, N = s["B"], s["N"]
    zero = np.zeros((1, 4))
    roll = solver.rollout_batch(N, s["X"], s["U"], s["k"], s["K"], zero, k_scale=0.0)
    X, U = np.ascontiguousarray(roll["X"][:, 0]), np.ascontiguousarray(roll["U"][:, 0])
    again = solver.rollout_batch(N, X, U, s["k"], s["K"], zero, k_scale=0.0)
    assert np.array_equal(_bits(again["X"][:, 0]), _bits(X))  # the trajectory reproduces itself
    solver.set_uncertainty_map(s["layers"], cilqr.map_geom(*s["geom"]), s["poses"], (1, 1))
    try:
        risk, hits, unk, _ = solver.rollout_risk_map(N, X, U, s["k"], s["K"], zero, s["threshold"], k_scale=0.0)
        cost, _, _ = solver.debug_uncertainty_cost(X.reshape(B, N + 1, 4)[:, :N].reshape(B * N, 4))
    finally:
        solver.clear_uncertainty_map()
    cost = cost.reshape(B, N)
    q1, q2 = solver.params.q1_uncertainty, solver.params.q2_uncertainty
    assert np.array_equal(cost > 0, unk == 0) and np.all((cost > 0).any(axis=1))  # (an invalid probe costs 0 and makes its one row unknown)
    assert np.min(np.diff(np.sort(cost, axis=1), axis=1)[:, -1] / cost.max(axis=1)) > 1e-6  # the argmax is decided
    mine = q1 * np.exp(q2 * (risk[:, MR_WORST_OCC] / 100.0 - 1.0))
    print("barrier of WORST_OCC %s\nmax debug cost      %s" % (mine.tolist(), cost.max(axis=1).tolist()))
    assert np.max(np.abs(mine - cost.max(axis=1)) / cost.max(axis=1)) <= 1e-9
    assert np.array_equal(risk[:, MR_WORST_ENTRY], cost.argmax(axis=1).astype(float))  # probes 1 x 1: entry = t
    assert np.array_equal(risk[:, MR_WORST_ROW], np.zeros(B))


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
def test_composition_with_the_obstacle_risk_and_the_pick(cilqr, solver, cases):
    """base = the total of cilqr_rollout_risk on the same scene (NaN where the obstacles already rejected): those NaNs stay, the map
    rejects on top, and cilqr_argmin_device returns numpy's pick of the numpy-derived total, -1 when all are rejected."""
    s, r = cases["A"], cases["scene_r"]
    B = s["B"]
    share = s[False]["risk"][:, MR_COLLISION]
    assert not np.any(np.abs(share - 0.06) < 1e-3)
    cost = np.linspace(3.0, 2.0, B)  # a per-solve cost to rank by ...
    cost[int(np.argmax(share))] = 1.0  # ... cheapest where the map share is largest: the map's say changes the pick
    assert share.max() > 0.06
    _, _, obstacle_total = solver.rollout_risk(s["N"], s["X"], s["U"], s["k"], s["K"], s["delta"], r["pose"], r["dim"], None, k_scale=0.0,
                                               max_risk=0.06, base=cost)
    assert np.isnan(obstacle_total).any() and not np.isnan(obstacle_total).all()
    picks = []
    with _Map(cilqr, solver, s):
        for max_risk in (0.06, 0.0, -1.0, 1.0):
            want = np.where((share > max_risk) | np.isnan(obstacle_total), np.nan, obstacle_total)
            for form in ("host", "device"):
                f = _host if form == "host" else _device
                total = f(solver, s, max_risk=max_risk, base=obstacle_total)[3]
                assert np.array_equal(np.isnan(total), np.isnan(want)), (max_risk, form)
                assert np.array_equal(_bits(total[~np.isnan(want)]), _bits(want[~np.isnan(want)])), (max_risk, form)
                assert _device_pick(solver, total) == _pick(want), (max_risk, form)
            picks.append(_pick(want))
    assert picks[2] == -1 and picks[3] == _pick(obstacle_total) and picks[0] != picks[3]


@gpu
def test_limits(cilqr, cases):
    """B * ceil(S/256) above max_batch: CILQR_ERR_ARG, and the handle stays usable.  No map set: CILQR_ERR_ARG, saying so.  The LDS
    formula allows every horizon a handle takes: the largest one runs."""
    s = cases["B"]
    sv = cilqr.Solver(_params(cilqr), max_batch=15, max_horizon=s["N"], max_obstacles=0, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*no uncertainty map" % ERR_ARG):
            _host(sv, s, sel=slice(0, 7))
        with _Map(cilqr, sv, s):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*above max_batch" % ERR_ARG):
                _host(sv, s)  # 8 solves x 2 partial records
            k = slice(0, 7)
            got = _host(sv, s, sel=k)  # 14 records
            _check_against(got, {n: s[False][n][k] for n in ("risk", "step_hits", "unknown_steps")}, s["S"], "7 solves on a handle of 15")
    finally:
        sv.close()
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    N = int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1))
    lds = 8 * (14 * N + 4) + 4 * N + 160
    assert lds <= 64 * 1024  # so CILQR_ERR_UNSUPPORTED is out of reach, and this horizon must run
    B, S = 2, 64
    sv = cilqr.Solver(_params(cilqr, N), max_batch=B, max_horizon=N, max_obstacles=0, device=0)
    try:
        a = cases["A"]
        with _Map(cilqr, sv, a):
            X = np.zeros((B, 4 * (N + 1)))
            X[:, 2::4] = 1.0
            risk, hits, unk, _ = sv.rollout_risk_map(N, X, np.zeros((B, 2 * N)), np.zeros((B, 2 * N)), np.zeros((B, 8 * N)), np.zeros((S, 4)), 50.0)
        assert hits.shape == (B, N) and np.all(np.isfinite(risk[:, MR_WORST_OCC]))
    finally:
        sv.close()


def _oracle_pick_of_the_dump(O, path):
    """What tests/cpp/candidates_risk_map.cpp wrote -> the numpy-derived map risk and pick for the candidates it solved: oracle rollouts
    with the dumped gains from its offsets, the probes and the lookup of this file on the dumped layer."""
    v = open(path).read().split()
    B, N, S, rows, cols = (int(x) for x in v[:5])
    a = np.array([float(x) for x in v[5:]])
    take = lambda n, at=[0]: (a[at[0]:at[0] + n], at.__setitem__(0, at[0] + n))[0]  # noqa: E731
    threshold, max_risk, best = take(1)[0], take(1)[0], int(take(1)[0])
    geom, pose = tuple(take(5)), tuple(take(3))
    X, U = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1)
    k, K, base = take(B * 2 * N).reshape(B, -1), take(B * 8 * N).reshape(B, -1), take(B)
    delta = take(S * 4).reshape(S, 4)
    risk = take(B * 7).reshape(B, 7)
    hits, unk = take(B * N).reshape(B, N).astype(np.int32), take(B * N).reshape(B, N).astype(np.int32)
    layer = take(rows * cols).astype(np.float32).reshape(cols, rows).T  # written column-major
    p = O.default_params(N)
    s = dict(p=p, B=B, N=N, X=X, U=U, k=k, K=K)
    want = _case(O, s, S, delta, 0.0, geom, (3, 3), threshold, layer, pose)
    return dict(best=best, max_risk=max_risk, base=base, risk=risk, hits=hits, unk=unk, want=want)


@gpu
def test_cpp_facade_map_risk_checked_candidates(oracle, tmp_path):
    """tests/cpp/candidates_risk_map.cpp: iLQR::run_candidates under set_pose_noise_check_fused + set_uncertainty_map +
    set_map_risk_check against the C-ABI sequence called by hand (inside the program) and against the numpy-derived map risk and pick for
    the candidates it solved (here).  The conditions on the occupancies are asserted for its scene."""
    exe, dump = str(tmp_path / "candidates_risk_map"), str(tmp_path / "dump.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_risk_map.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map risk pick ok" in r.stdout, r.stdout
    d = _oracle_pick_of_the_dump(oracle, dump)
    s = d["want"]
    want = s[False]
    print("min|occ - thr| %.3g, oracle hit rows %s, unknown rows %s" % (np.min(np.abs(s["occ"][s["ok"]] - s["threshold"])),
                                                                      want["hit_rows"].tolist(), want["unknown_rows"].tolist()))
    assert np.min(np.abs(s["occ"][s["ok"]] - s["threshold"])) > MARGIN
    for dx, dy in ((MARGIN, 0.0), (-MARGIN, 0.0), (0.0, MARGIN), (0.0, -MARGIN)):
        assert np.array_equal(np_lookup(s["layers"], s["g"], s["qx"] + dx, s["qy"] + dy)[1], s["ok"])
    assert np.min(np.abs(want["risk"][:, MR_COLLISION] - d["max_risk"])) > 1e-3
    _check_against((d["risk"], d["hits"], d["unk"]), want, s["S"], "the façade's last_map_risk")
    total = np.where((want["risk"][:, MR_COLLISION] > d["max_risk"]) | np.isnan(d["base"]), np.nan, d["base"])
    assert np.isnan(total).any() and not np.isnan(total).all()
    assert d["best"] == _pick(total)
