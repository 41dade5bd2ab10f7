"""Map tightening (cilqr_tighten_map*, include/cilqr.h): the uncertainty-map layer set on the handle dilated, per cell, by kappa standard
deviations of where the footprint point over that cell may be, from the Sigma_t of the plan's nearest step; the dense per-solve layers a
warm-started re-solve reads.

Expected values never come from the HIP path: `tighten_map_restate` below is a numpy restatement of the header's definition, written from
the header; Sigma_t comes from `restate` of tests/test_chance_risk.py, the lookup, geometries, `_Map` and layers from tests/test_risk_map.py,
the map risk from `restate_map` of tests/test_chance_risk_map.py.  Every output value is a bit copy of an input value, so layers are compared
bit for bit on every cell that is not BORDERLINE: the two smallest step distances within 1e-9 relative, or an in-box neighbour whose
ellipse test lies within 1e-9 relative of its bound.  Counts and indices exactly, TM_MAX_RAISE bit-equal, TM_MAX_REACH within 4 ulp.
Case C's poses are per solve, so their cosine and sine are the device's where the restatement has the host's; it is held to the same
bounds as every other case (measured on the MI355X: TM_MAX_REACH 0 ulp from the restatement in every case, C included).

  A    GEOM_A (160 x 80 at 0.1 m), N 20, B 3, shared layer and POSE_A, kappa 1.645, max_inflate 1.0: a curved plan, Sigma_t growing along it
       with non-zero cross terms; 50 workgroups per solve
  D    GEOM_D (30 x 80), N 2, max_inflate 0.3: every cell capped
  O    37 x 53 cells, N 5: no tile size divides it; 8 workgroups, the last partial
  W    240 x 90 cells, N 20: 85 tiles of 256 cells on the 64 workgroups a solve has at most, so workgroups take a second tile
  C    A's geometry, one layer (1 % NaN cells) and one pose per solve, a plan that leaves the map
  Z    A with kappa 0: the identity.   Z1: A with max_inflate 0: the identity, every cell with a reach capped
  L    A with one step lost through X, one through Sigma_t, and a solve with every step lost
"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_candidate_score import _bits
from test_chance_risk import SIGMA0, W_DIAG, restate
from test_chance_risk_map import STEP_RISK as CM_STEP_RISK
from test_chance_risk_map import TOL as CM_TOL
from test_chance_risk_map import np_quadrature, restate_map
from test_risk_map import GEOM_A, GEOM_D, POSE_A, SAFE, _c_poses, _Map, _params, smooth_layer
from test_rollout_risk import _close, o_gains

gpu = pytest.mark.gpu

ERR_ARG = -1
ENTRY_POINTS = ("cilqr_tighten_map", "cilqr_tighten_map_device")
FIELDS = ("RAISED", "MAX_RAISE", "MAX_CELL", "MAX_REACH", "CAPPED", "LOST")
RAISED, MAX_RAISE, MAX_CELL, MAX_REACH, CAPPED, LOST = range(6)
SIX = (0, 4, 5, 12, 13, 15)  # (0,0), (0,1), (1,1), (0,3), (1,3), (3,3) at [r + 4c]
KAPPA = 1.645
BORDER = 1e-9
GEOM_O = (3.7, 5.3, 0.1, 1.5, 0.2)
GEOM_W = (24.0, 9.0, 0.1, 10.0, 0.0)
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- expected values: a numpy restatement of the header's definition ----------------------------------------------------------------
def _solve_restate(p, N, X, S, g, layer, pose, kappa, cap):
    """One solve.  X (N+1, 4), S (N+1, 16), layer (rows, cols) float32, pose (x, y, theta).  Every
    formula as include/cilqr.h writes it, evaluated left to right."""
    rows, cols, res = int(g.rows), int(g.cols), float(g.res)
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    r_fp = 0.5 * math.sqrt(p.safe_length * p.safe_length + p.safe_width * p.safe_width)
    c, s = math.cos(pose[2]), math.sin(pose[2])
    Xs, S = X[:N], S[:N]
    S00, S01, S11, S03, S13, S33 = (S[:, i] for i in SIX)
    live = np.isfinite(Xs[:, [0, 1, 3]]).all(axis=1) & np.isfinite(S[:, list(SIX)]).all(axis=1)
    layer = np.asarray(layer, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy = Xs[:, 0] - pose[0], Xs[:, 1] - pose[1]
        px, py = c * dx + s * dy, c * dy - s * dx
        cc, ss, cs_ = c * c, s * s, c * s
        Pxx = cc * S00 + 2.0 * cs_ * S01 + ss * S11
        Pxy = cs_ * (S11 - S00) + (cc - ss) * S01
        Pyy = ss * S00 - 2.0 * cs_ * S01 + cc * S11
        cx, cy, Stt = c * S03 + s * S13, c * S13 - s * S03, S33
        mx = (x_first - np.arange(rows, dtype=np.float64) * res)[:, None, None]
        my = (y_first - np.arange(cols, dtype=np.float64) * res)[None, :, None]
        ex, ey = mx - px, my - py
        d2 = ex * ex + ey * ey                                      # (rows, cols, N)
        d2 = np.where(live & np.isfinite(d2), d2, np.inf)
        ts = d2.argmin(axis=2)                                      # the lowest t on equal values
        has = np.isfinite(d2.min(axis=2))
        two = np.sort(d2, axis=2)[:, :, :2] if N > 1 else np.stack([d2[:, :, 0], np.full((rows, cols), np.inf)], axis=2)
        border = has & np.isfinite(two[:, :, 1]) & (two[:, :, 1] - two[:, :, 0] <= BORDER * two[:, :, 1])
        ddx, ddy = mx[:, :, 0] - px[ts], my[:, :, 0] - py[ts]
        length = np.sqrt(ddx * ddx + ddy * ddy)
        f = r_fp / length
        longer = length > r_fp
        ddx, ddy = np.where(longer, ddx * f, ddx), np.where(longer, ddy * f, ddy)
        jx, jy = -ddy, ddx
        Cxx = Pxx[ts] + 2.0 * jx * cx[ts] + jx * jx * Stt[ts]
        Cyy = Pyy[ts] + 2.0 * jy * cy[ts] + jy * jy * Stt[ts]
        Cxy = Pxy[ts] + jx * cy[ts] + jy * cx[ts] + jx * jy * Stt[ts]
        hx, hy = kappa * np.sqrt(np.where(Cxx < 0.0, 0.0, Cxx)), kappa * np.sqrt(np.where(Cyy < 0.0, 0.0, Cyy))
        reach_raw = has & ((hx > 0.0) | (hy > 0.0) | ~np.isfinite(hx) | ~np.isfinite(hy))
        capx, capy = ~np.isfinite(hx) | (hx > cap), ~np.isfinite(hy) | (hy > cap)
        hx, hy = np.where(capx, cap, hx), np.where(capy, cap, hy)
        ni = np.minimum(np.floor(hx / res), rows - 1).astype(np.int64)
        nj = np.minimum(np.floor(hy / res), cols - 1).astype(np.int64)
        det = Cxx * Cyy - Cxy * Cxy
        lim = kappa * kappa * det
    own = layer
    act = has & np.isfinite(own)
    best = own.copy()
    ii, jj = np.arange(rows)[:, None], np.arange(cols)[None, :]
    clipped = act & ((ni > ii) | (ni > rows - 1 - ii) | (nj > jj) | (nj > cols - 1 - jj))
    max_ni, max_nj = (int(ni[act].max()), int(nj[act].max())) if act.any() else (0, 0)
    for bb in range(-max_nj, max_nj + 1):
        ey1 = -float(bb) * res
        for aa in range(-max_ni, max_ni + 1):
            ex1 = -float(aa) * res
            inside = (ii + aa >= 0) & (ii + aa < rows) & (jj + bb >= 0) & (jj + bb < cols)
            v = np.full((rows, cols), np.nan, dtype=np.float32)
            i0, i1, j0, j1 = max(0, -aa), min(rows, rows - aa), max(0, -bb), min(cols, cols - bb)
            v[i0:i1, j0:j1] = layer[i0 + aa:i1 + aa, j0 + bb:j1 + bb]
            with np.errstate(invalid="ignore", over="ignore"):
                q = Cyy * (ex1 * ex1) - 2.0 * Cxy * ex1 * ey1 + Cxx * (ey1 * ey1)
                box = act & inside & (abs(aa) <= ni) & (abs(bb) <= nj)
                ok = box & (~(det > 0.0) | (q <= lim)) & np.isfinite(v)
                if aa or bb:  # (the cell itself is no neighbour: its q is 0)
                    border |= box & (det > 0.0) & (np.abs(q - lim) <= BORDER * lim)
                best = np.where(ok & (v > best), v, best)
    with np.errstate(invalid="ignore"):
        raise_ = best.astype(np.float64) - own.astype(np.float64)
    up = raise_ > 0.0
    fields = np.zeros(6)
    fields[RAISED] = up.sum()
    fields[MAX_CELL] = -1.0
    if up.any():
        flat = np.where(up, raise_, -np.inf).flatten(order="F")  # index i + rows*j; argmax: the lowest on equal values
        fields[MAX_RAISE], fields[MAX_CELL] = flat.max(), int(flat.argmax())
    fields[MAX_REACH] = float(np.maximum(hx, hy)[has].max()) if has.any() else 0.0
    fields[CAPPED] = ((capx | capy) & has).sum()
    fields[LOST] = N - int(live.sum())
    return dict(layer=best, fields=fields, border=border, clipped=clipped, reach_raw=reach_raw, capped=(capx | capy) & has, ni=ni, nj=nj,
                act=act, ts=ts, has=has)


def tighten_map_restate(p, N, X, sigma, g, layers, poses, kappa, cap):
    """X (B, 4(N+1)), sigma (B, N+1, 16); layers / poses one shared or lists of B.  Returns dict(layer (B, rows, cols) float32, fields
    (B, 6), border / clipped / reach_raw / capped (B, rows, cols) bool, ni, nj)."""
    B = X.shape[0]
    per_solve = isinstance(layers, list)
    each = [_solve_restate(p, N, X[b].reshape(N + 1, 4), sigma[b].reshape(N + 1, 16), g, layers[b] if per_solve else layers,
                           poses[b] if per_solve else poses, kappa, cap) for b in range(B)]
    return {k: np.stack([e[k] for e in each]) for k in each[0]}


def _plan(N, B, step, turn, y0=-0.6):
    """A synthetic plan of any horizon: arcs of `step` metres per step that start side by side, a stabilising constant gain."""
    X, U, K = np.zeros((B, N + 1, 4)), np.zeros((B, N, 2)), np.zeros((B, N, 4, 2))
    for b in range(B):
        th = 0.15 * b - 0.2 + turn * (b + 1) * np.arange(N + 1)
        X[b, :, 2], X[b, :, 3] = step / 0.1, th
        X[b, 0, 0], X[b, 0, 1] = 0.3 + 0.07 * b, y0 + 0.45 * b
        X[b, 1:, 0], X[b, 1:, 1] = X[b, 0, 0] + np.cumsum(step * np.cos(th[:-1])), X[b, 0, 1] + np.cumsum(step * np.sin(th[:-1]))
        U[b, :, 1] = turn * (b + 1) / 0.1
    K[:, :, 2, 0] = -1.0                       # acceleration against the speed error
    K[:, :, 1, 1], K[:, :, 3, 1] = -0.5, -1.5  # yaw rate against the lateral and heading errors
    return X.reshape(B, -1), U.reshape(B, -1), K.reshape(B, -1)


SIGMA0_M = np.diag([0.12 ** 2, 0.1 ** 2, 0.2 ** 2, 0.05 ** 2])
SIGMA0_M[0, 1] = SIGMA0_M[1, 0] = 0.3 * 0.12 * 0.1
SIGMA0_M[1, 3] = SIGMA0_M[3, 1] = 0.4 * 0.1 * 0.05


def _mk(O, N, B, step, turn, geom, layers, poses, kappa, cap, sigma0=SIGMA0_M, edit=None):
    p = O.default_params(N)
    p.safe_length, p.safe_width = SAFE
    X, U, K = _plan(N, B, step, turn)
    sigma = restate(p, N, X, U, K, sigma0.T.reshape(16), (25.0 * W_DIAG).T.reshape(16), None, None)["sigma"]
    if edit is not None:
        X, sigma = X.copy(), sigma.copy()
        edit(X, sigma)
    g = O.map_geom(*geom)
    s = dict(p=p, N=N, B=B, X=np.ascontiguousarray(X), sigma=np.ascontiguousarray(sigma), geom=geom, g=g, layers=layers, poses=poses,
             probes=(3, 3), kappa=kappa, cap=cap)
    s["want"] = tighten_map_restate(p, N, s["X"], s["sigma"], g, layers, poses, kappa, cap)
    return s


def _nan_layer(rows, cols, seed):
    """smooth_layer with 1 % of its cells unknown."""
    layer = smooth_layer(rows, cols, seed)
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    flat = rng.choice(rows * cols, rows * cols // 100, replace=False)
    layer[flat % rows, flat // rows] = np.nan
    return layer


def _lose(X, sigma):
    N = sigma.shape[1] - 1
    X[0, 4 * 3 + 0] = np.nan    # solve 0, step 3: x
    sigma[1, 7, 13] = np.nan    # solve 1, step 7: entry (1, 3)
    sigma[1, 4, 10] = np.nan    # the speed's variance is not read
    sigma[0, N, 0] = np.nan     # Sigma_N is not visited
    X[2, 0::4] = np.inf         # solve 2: every step


@pytest.fixture(scope="module")
def cases(oracle):
    """Every case's inputs and restatement.  Computed once; never modified."""
    O = oracle
    la = smooth_layer(160, 80, 3)
    out = {"A": _mk(O, 20, 3, 0.3, 0.03, GEOM_A, la, POSE_A, KAPPA, 1.0),
           "D": _mk(O, 2, 3, 0.3, 0.03, GEOM_D, smooth_layer(30, 80, 3), POSE_A, KAPPA, 0.3, sigma0=4.0 * SIGMA0_M),
           "O": _mk(O, 5, 3, 0.3, 0.03, GEOM_O, smooth_layer(37, 53, 5), (0.1, -0.05, 0.05), KAPPA, 1.0),
           "W": _mk(O, 20, 3, 0.3, 0.03, GEOM_W, smooth_layer(240, 90, 7), POSE_A, KAPPA, 1.0),
           "C": _mk(O, 20, 3, 0.9, 0.012, GEOM_A, [_nan_layer(160, 80, seed) for seed in (1, 2, 3)], _c_poses(3), KAPPA, 1.0),
           "Z": _mk(O, 20, 3, 0.3, 0.03, GEOM_A, la, POSE_A, 0.0, 1.0),
           "Z1": _mk(O, 20, 3, 0.3, 0.03, GEOM_A, la, POSE_A, KAPPA, 0.0),
           "L": _mk(O, 20, 3, 0.3, 0.03, GEOM_A, la, POSE_A, KAPPA, 1.0, edit=_lose)}
    return out


CASES = ["A", "D", "O", "W", "C", "Z", "Z1", "L"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_TIGHTEN_MAP_FIELDS\s+6\b", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_TM_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "TM_" + name) == i
    assert cilqr.TIGHTEN_MAP_FIELDS == 6
    assert callable(cilqr.Solver.tighten_map) and callable(cilqr.Solver.tighten_map_device)
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_map_tightening\s*\(\s*const\s+double\s+Sigma0\s*\[\s*16\s*\]\s*,\s*const\s+double\s*\*\s*W\s*,\s*double\s+eps\s*,"
                     r"\s*int\s+rounds\s*=\s*1\s*,\s*double\s+max_inflate\s*=\s*1\.0\s*,\s*double\s+lamb\s*=\s*1\.0\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_tighten_map\s*,\s*last_tighten_map_risk_before\s*;", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_tighten_map\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_tighten_map.hip" in mk and len(re.findall(r"build/cilqr_tighten_map\.o", mk)) == 2  # `check` and its resource list
    # the definition stands in the header, and says what the nearest-step rule leaves out
    for phrase in ("nearest step", "strict <, lowest t on equal", "copied through: unknown stays unknown", "the LOWEST such step wins",
                   "Judge the final plan against the ORIGINAL map"):
        assert phrase in full, phrase


def test_argument_errors_need_no_device(cilqr):
    """NULL X, sigma, layer_out or tighten, a kappa or max_inflate that is negative or not finite: CILQR_ERR_ARG, decided before the handle
    is looked at (there is none here); valid arguments reach the handle check."""
    L = cilqr.lib()
    B, N = 2, 4
    X, sigma, layer, tg = np.zeros((B, 4 * (N + 1))), np.zeros((B, N + 1, 16)), np.zeros((B, 12), dtype=np.float32), np.zeros((B, 6))
    no_handle = C.c_void_p()
    d = C.c_double
    nan, inf = float("nan"), float("inf")

    def call(dev, kappa=KAPPA, cap=1.0, **nulls):
        a = dict(X=X, sigma=sigma, layer=layer, tg=tg)
        a.update(nulls)
        f = L.cilqr_tighten_map_device if dev else L.cilqr_tighten_map
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, _p(a["X"]), _p(a["sigma"]), d(kappa), d(cap), _p(a["layer"], _fp), _p(a["tg"]))

    for dev in (False, True):
        for name in ("X", "sigma", "layer", "tg"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        for bad in (-1e-3, nan, inf, -inf):
            assert call(dev, kappa=bad) == ERR_ARG and b"kappa is negative or not finite" in L.cilqr_last_error(), bad
            assert call(dev, cap=bad) == ERR_ARG and b"max_inflate is negative or not finite" in L.cilqr_last_error(), bad
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, kappa=0.0, cap=0.0) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # zero is valid


@pytest.mark.parametrize("name", CASES)
def test_conditions(cases, name):
    """On the restatement alone: how many cells are BORDERLINE (at most 1 % of a case's cells; A and D must have none, their fields are
    compared), and that each case exercises what it is there for."""
    s = cases[name]
    w = s["want"]
    cells = w["layer"][0].size
    share = w["border"].sum() / float(w["border"].size)
    own = np.stack(s["layers"]) if isinstance(s["layers"], list) else np.broadcast_to(s["layers"], w["layer"].shape)
    print("case %s: %d cells, borderline %d (share %.3g); fields %s; reach up to %d x %d cells" % (
        name, cells, w["border"].sum(), share, w["fields"].tolist(), w["ni"][w["act"]].max() if w["act"].any() else 0,
        w["nj"][w["act"]].max() if w["act"].any() else 0))
    assert share <= 0.01
    # every output value is an input value of the same layer; an unknown cell stays unknown
    for b in range(s["B"]):
        assert np.isin(_bits32(w["layer"][b][np.isfinite(w["layer"][b])]), _bits32(own[b][np.isfinite(own[b])])).all()
    assert np.array_equal(np.isnan(w["layer"]), np.isnan(own))
    with np.errstate(invalid="ignore"):
        assert not np.any(w["layer"] < own)
    if name in ("A", "D"):
        assert share == 0.0
    if name == "A":
        assert np.all(w["fields"][:, RAISED] > 1000) and np.all(w["fields"][:, LOST] == 0)
        assert w["ni"][w["act"]].max() >= 3 and w["nj"][w["act"]].max() >= 4 and np.all(w["fields"][:, CAPPED] == 0)
        ts = w["ts"]
        assert all(len(np.unique(ts[b])) == s["N"] for b in range(s["B"]))  # every step is some cell's nearest
        S = s["sigma"][:, :s["N"]]
        assert np.all(S[:, -1, 0] > 2.0 * S[:, 0, 0]) and np.all(np.abs(S[:, 1:, 4]) > 1e-5) and np.all(np.abs(S[:, 1:, 12]) > 1e-5)
    if name == "D":
        assert np.all(w["fields"][:, CAPPED] == cells) and np.all(w["fields"][:, MAX_REACH] == 0.3)
    if name == "O":
        assert cells == 37 * 53 and np.all(w["fields"][:, RAISED] > 0)
    if name == "W":  # more tiles than a solve has workgroups, and the plan's neighbourhood lies in first and in second tiles
        assert (cells + 255) // 256 > 64 and np.all(w["fields"][:, RAISED] > 1000)
    if name == "C":
        assert np.all(w["clipped"].reshape(s["B"], -1).sum(axis=1) > 0)
        assert np.isnan(own).reshape(s["B"], -1).sum(axis=1).min() >= cells // 100
        X = s["X"].reshape(s["B"], s["N"] + 1, 4)
        assert np.all(X[:, s["N"] - 1, 0] > 14.5)  # the plan leaves the map (x up to 14 m)
        alt = _solve_restate(s["p"], s["N"], X[1], s["sigma"][1], s["g"], s["layers"][0], s["poses"][0], s["kappa"], s["cap"])
        assert not np.array_equal(_bits32(alt["layer"]), _bits32(w["layer"][1]))  # solve 1's own layer and pose matter
    if name == "Z":
        assert np.array_equal(_bits32(w["layer"]), _bits32(own)) and not w["fields"][:, [RAISED, MAX_RAISE, MAX_REACH, CAPPED]].any()
        assert np.all(w["fields"][:, MAX_CELL] == -1)
    if name == "Z1":
        assert np.array_equal(_bits32(w["layer"]), _bits32(own)) and not w["fields"][:, [RAISED, MAX_RAISE, MAX_REACH]].any()
        assert np.array_equal(w["fields"][:, CAPPED], w["reach_raw"].reshape(s["B"], -1).sum(axis=1)) and np.all(w["fields"][:, CAPPED] == cells)
    if name == "L":
        assert w["fields"][:, LOST].tolist() == [1.0, 1.0, float(s["N"])]
        assert np.array_equal(_bits32(w["layer"][2]), _bits32(own[2])) and w["fields"][2].tolist() == [0.0, 0.0, -1.0, 0.0, 0.0, float(s["N"])]
        a = cases["A"]["want"]
        assert not (w["ts"][0] == 3).any() and (a["ts"][0] == 3).any() and not (w["ts"][1] == 7).any()
        assert np.all(w["fields"][:2, RAISED] > 1000)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    # (the host form stages the layers through the arena: 3*(20*20 + 26 + 10800) doubles of case W against 32*(22*50 + 34))
    s = cilqr.Solver(_params(cilqr), max_batch=32, max_horizon=50, max_obstacles=0, device=0)
    yield s
    s.close()


FILL = -7.0  # what the output buffers hold before a call: no input layer holds it


def _layers_of(flat, g):
    return flat.reshape(flat.shape[0], int(g.cols), int(g.rows)).transpose(0, 2, 1)


def _device(cilqr, solver, s, sel=None, copies=False, keep=None):
    """The device form on torch buffers, for the solves `sel` of the case in that order.  copies: a shared layer given as one equal copy
    per solve (the shared pose stays).  keep: a dict that receives the device buffers (the layers feed the map cost)."""
    import torch
    idx = list(range(s["B"])) if sel is None else list(sel)
    B, N, g = len(idx), s["N"], s["g"]
    cells = int(g.rows) * int(g.cols)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    X, sigma = (torch.from_numpy(np.ascontiguousarray(s[n][idx])).to(dev) for n in ("X", "sigma"))
    out = torch.full((B, cells), FILL, dtype=torch.float32, device=dev)
    tg = torch.full((B, 6), FILL, dtype=torch.float64, device=dev)
    per_solve = isinstance(s["layers"], list)
    if copies:
        assert not per_solve
        flat = np.stack([np.asfortranarray(s["layers"]).flatten(order="F")] * B)
        lay = torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    torch.cuda.synchronize(dev)
    if copies:
        solver.set_uncertainty_map_device(lay.data_ptr(), cilqr.map_geom(*s["geom"]), s["poses"], s["probes"], layer_stride=cells)
        m = None
    else:
        m = _Map(cilqr, solver, s, sel=idx if per_solve else None)
    try:
        solver.tighten_map_device(stream, B, N, X.data_ptr(), sigma.data_ptr(), out.data_ptr(), tg.data_ptr(), kappa=s["kappa"], max_inflate=s["cap"])
        torch.cuda.synchronize(dev)
    finally:
        solver.clear_uncertainty_map()
    if keep is not None:
        keep.update(out=out, map=m)
    return dict(layer=_layers_of(out.cpu().numpy(), g), fields=tg.cpu().numpy())


def _host(cilqr, solver, s, sel=None):
    idx = list(range(s["B"])) if sel is None else list(sel)
    per_solve = isinstance(s["layers"], list)
    with _Map(cilqr, solver, s, sel=idx if per_solve else None):
        got = solver.tighten_map(s["N"], s["X"][idx], s["sigma"][idx], (s["g"].rows, s["g"].cols), kappa=s["kappa"], max_inflate=s["cap"])
    return dict(layer=np.ascontiguousarray(got["layer"]), fields=got["tighten"])


def _same(a, b, sel_a=slice(None), sel_b=slice(None)):
    return np.array_equal(_bits32(a["layer"][sel_a]), _bits32(b["layer"][sel_b])) and np.array_equal(_bits(a["fields"][sel_a]), _bits(b["fields"][sel_b]))


def _ulps(a, b):
    return np.abs(_bits(np.asarray(a, dtype=np.float64)).astype(np.int64) - _bits(np.asarray(b, dtype=np.float64)).astype(np.int64))


def _check_against(got, s, what, sel=None):
    idx = list(range(s["B"])) if sel is None else list(sel)
    w = s["want"]
    wl, wf, border = w["layer"][idx], w["fields"][idx], w["border"][idx]
    differ = _bits32(got["layer"]) != _bits32(wl)
    print("%s: %d cells differ, %d of them borderline (%d borderline in all); fields %s" % (
        what, differ.sum(), (differ & border).sum(), border.sum(), got["fields"].tolist()))
    assert not (differ & ~border).any(), what
    assert not (got["layer"] == FILL).any(), what
    assert np.array_equal(got["fields"][:, LOST], wf[:, LOST]), what
    for k, b in enumerate(idx):
        if border[k].any():  # fields are compared for solves without a borderline cell
            continue
        f = got["fields"][k]
        assert np.array_equal(f[[RAISED, MAX_CELL, CAPPED]], wf[k][[RAISED, MAX_CELL, CAPPED]]), (what, b, f, wf[k])
        assert _bits(f[MAX_RAISE:MAX_RAISE + 1])[0] == _bits(wf[k][MAX_RAISE:MAX_RAISE + 1])[0], (what, b)
        d = int(_ulps(f[MAX_REACH:MAX_REACH + 1], wf[k][MAX_REACH:MAX_REACH + 1])[0])
        print("%s, solve %d: TM_MAX_REACH %d ulp from the restatement (bound: 4)" % (what, b, d))
        assert d <= 4, (what, b, f[MAX_REACH], wf[k][MAX_REACH])


@gpu
@pytest.mark.parametrize("name", CASES)
def test_layers_and_fields_against_the_restatement(cilqr, solver, cases, name):
    """The device form and the host form: layers bit for bit on every cell that is not borderline, counts and indices exact, TM_MAX_RAISE
    bit-equal, TM_MAX_REACH within 4 ulp; the two forms give the same bits."""
    s = cases[name]
    dev = _device(cilqr, solver, s)
    _check_against(dev, s, "case %s, device form" % name)
    host = _host(cilqr, solver, s)
    _check_against(host, s, "case %s, host form" % name)
    assert _same(host, dev)
    if name in ("A", "D"):
        assert not s["want"]["border"].any()
    if name in ("Z", "Z1"):
        own = np.broadcast_to(s["layers"], dev["layer"].shape)
        assert np.array_equal(_bits32(dev["layer"]), _bits32(own)) and not dev["fields"][:, RAISED].any()
    if name == "L":
        assert np.array_equal(_bits32(dev["layer"][2]), _bits32(s["layers"])) and dev["fields"][2].tolist() == [0.0, 0.0, -1.0, 0.0, 0.0, 20.0]


@gpu
def test_a_result_depends_on_its_own_solve_alone(cilqr, solver, cases):
    """A solve's layer and fields are the same bits at B = 1 and at B = 3 in any position, with a shared layer and with one equal copy
    per solve, and on a handle of other create sizes; per-solve layers and poses travel with their solve."""
    wholes = {}
    for name in ("A", "W"):
        s = cases[name]
        whole = wholes[name] = _device(cilqr, solver, s)
        for b in range(s["B"]):
            assert _same(_device(cilqr, solver, s, sel=[b]), whole, sel_b=slice(b, b + 1)), (name, b)
        for order in ([2, 0, 1], [1, 2, 0]):
            assert _same(_device(cilqr, solver, s, sel=order), whole, sel_b=order), (name, order)
        assert _same(_device(cilqr, solver, s, copies=True), whole), name
    s = cases["A"]
    small = cilqr.Solver(_params(cilqr), max_batch=3, max_horizon=s["N"], max_obstacles=0, device=0)
    try:
        assert _same(_device(cilqr, small, s), wholes["A"])
    finally:
        small.close()
    c = cases["C"]
    whole = _device(cilqr, solver, c)
    order = [2, 0, 1]
    assert _same(_device(cilqr, solver, c, sel=order), whole, sel_b=order)
    assert _same(_device(cilqr, solver, c, sel=[1]), whole, sel_b=slice(1, 2))


@gpu
def test_the_output_feeds_the_map_cost(cilqr, oracle, solver, cases):
    """The tightened layers set through cilqr_set_uncertainty_map_device with layer_stride = rows*cols: cilqr_debug_uncertainty_cost
    (which reads solve 0's layer, so each solve's layer is set in turn) equals the oracle's uncertainty_cost on the restated layer at the
    plan's states and at random ones, within the bounds of test_uncertainty_cost_kernel_vs_oracle (1e-11 relative)."""
    O = oracle
    rng = np.random.default_rng(17)
    for name in ("A", "C"):
        s = cases[name]
        keep = {}
        _device(cilqr, solver, s, keep=keep)
        g, cells = s["g"], int(s["g"].rows) * int(s["g"].cols)
        per_solve = isinstance(s["layers"], list)
        for b in range(s["B"]):
            pose = s["poses"][b] if per_solve else s["poses"]
            st = np.concatenate([s["X"][b].reshape(-1, 4)[:s["N"]],
                                 np.stack([rng.uniform(-2, 14, 256), rng.uniform(-4, 4, 256), rng.uniform(0, 8, 256), rng.uniform(-3.2, 3.2, 256)], 1)])
            solver.set_uncertainty_map_device(keep["out"].data_ptr() + 4 * cells * b, cilqr.map_geom(*s["geom"]), pose, s["probes"], layer_stride=cells)
            try:
                cost, vx, mx = solver.debug_uncertainty_cost(st)
            finally:
                solver.clear_uncertainty_map()
            assert not s["want"]["border"][b].any()  # the restated layer is the device's, cell for cell
            um, alive = O.uncertainty_map(s["want"]["layer"][b], g, pose, s["probes"])
            wc, wv, wm = O.uncertainty_cost(s["p"], um, st)
            um0, alive0 = O.uncertainty_map(s["layers"][b] if per_solve else s["layers"], g, pose, s["probes"])
            w0, _, _ = O.uncertainty_cost(s["p"], um0, st)
            print("case %s solve %d: max cost %.4g on the tightened layer, %.4g on the original" % (name, b, wc.max(), w0.max()))
            assert (wc > 0).mean() > 0.5 and np.all(wc >= w0 * (1.0 - 1e-12)) and np.any(wc > w0 * 1.01)  # the dilation raises the cost and never lowers it
            assert np.allclose(cost, wc, rtol=1e-11, atol=1e-14)
            assert np.allclose(vx, wv[:, :2], rtol=1e-11, atol=1e-12)
            assert np.allclose(mx, np.stack([wm[:, 0, 0], wm[:, 0, 1], wm[:, 1, 1]], 1), rtol=1e-11, atol=1e-12)


@gpu
def test_limits(cilqr, solver, cases):
    """No map set: CILQR_ERR_ARG, saying so.  B or N beyond the handle's: CILQR_ERR_ARG.  layer_out inside the set layer: CILQR_ERR_ARG.  A
    host call beyond the arena: CILQR_ERR_ARG, and the handle stays usable.  The largest horizon a handle takes runs."""
    import torch
    s = cases["O"]
    rows, cols = int(s["g"].rows), int(s["g"].cols)
    sv = cilqr.Solver(_params(cilqr), max_batch=2, max_horizon=s["N"], max_obstacles=0, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*no uncertainty map" % ERR_ARG):
            sv.tighten_map(s["N"], s["X"][:2], s["sigma"][:2], (rows, cols), kappa=KAPPA)
        with _Map(cilqr, sv, s):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: B=3 outside" % ERR_ARG):
                sv.tighten_map(s["N"], s["X"], s["sigma"], (rows, cols), kappa=KAPPA)
            # 2*(20*5 + 26 + 1961/2) doubles against the 2*(22*5 + 34) the arena holds at least
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers" % ERR_ARG):
                sv.tighten_map(s["N"], s["X"][:2], s["sigma"][:2], (rows, cols), kappa=KAPPA)
        got = _device(cilqr, sv, s, sel=[0, 1])
        _check_against(got, s, "2 solves on a handle of 2", sel=[0, 1])
        dev = torch.device("cuda", 0)
        lay = torch.zeros(3 * rows * cols, dtype=torch.float32, device=dev)
        X, sigma, tg = (torch.zeros(n, dtype=torch.float64, device=dev) for n in (2 * 4 * (s["N"] + 1), 2 * 16 * (s["N"] + 1), 12))
        torch.cuda.synchronize(dev)
        sv.set_uncertainty_map_device(lay.data_ptr(), cilqr.map_geom(*s["geom"]), s["poses"], s["probes"], layer_stride=rows * cols)
        try:
            for off in (0, rows * cols - 1, 2 * rows * cols - 1):  # any cell of the two layers read
                with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*overlaps the layer set" % ERR_ARG):
                    sv.tighten_map_device(0, 2, s["N"], X.data_ptr(), sigma.data_ptr(), lay.data_ptr() + 4 * off, tg.data_ptr(), kappa=KAPPA)
        finally:
            sv.clear_uncertainty_map()
    finally:
        sv.close()
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    N = int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1))
    big = dict(cases["O"])
    X = np.zeros((2, N + 1, 4))
    X[:, :, 0], X[:, :, 1] = np.linspace(0.2, 3.0, N + 1), 0.3
    sigma = np.zeros((2, N + 1, 16))
    sigma[:, :, [0, 5]], sigma[:, :, 15] = 0.16 ** 2, 0.017 ** 2
    big.update(N=N, B=2, X=X.reshape(2, -1), sigma=sigma)
    big["want"] = tighten_map_restate(big["p"], N, big["X"], sigma, big["g"], big["layers"], big["poses"], KAPPA, 1.0)
    sv = cilqr.Solver(_params(cilqr, N), max_batch=2, max_horizon=N, max_obstacles=0, device=0)
    try:
        got = _device(cilqr, sv, big)
        _check_against(got, big, "N = %d" % N)
        assert np.array_equal(_bits32(got["layer"][0]), _bits32(got["layer"][1]))
        with _Map(cilqr, sv, big):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: N=%d outside" % (ERR_ARG, N + 1)):
                sv.tighten_map(N + 1, np.zeros((2, 4 * (N + 2))), np.zeros((2, N + 2, 16)), (rows, cols), kappa=KAPPA)
    finally:
        sv.close()


# ---- one round: solve -> gains -> Sigma_t -> tightened layers -> re-solve, judged against the ORIGINAL map ---------------------------------
ROUND_B, ROUND_N, ROUND_EPS, ROUND_THRESHOLD = 6, 25, 0.05, 50.0
ROUND_W_UNCERTAINTY = 5.0  # Parameters::w_uncertainty of the scene: at the default 1 the map term is too weak to move a plan off the blob
ROUND_BLOB = (6.0, -1.4, 0.7)  # a blob beside the straight path y = 0: world x, y of its centre and its width


def blob_layer(g, pose, blob=ROUND_BLOB):
    """(rows, cols) float32: 100*tanh(1.3*exp(-r^2 / (2 w^2))) around the blob's centre, on the cell centres of the map at `pose`."""
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    mx = (x_first - np.arange(g.rows) * g.res)[:, None]
    my = (y_first - np.arange(g.cols) * g.res)[None, :]
    c, s = math.cos(pose[2]), math.sin(pose[2])
    wx, wy = pose[0] + c * mx - s * my, pose[1] + s * mx + c * my
    r2 = (wx - blob[0]) ** 2 + (wy - blob[1]) ** 2
    return (100.0 * np.tanh(1.3 * np.exp(-0.5 * r2 / blob[2] ** 2))).astype(np.float32)


def _round_scene(O):
    """B candidates side by side on a straight path, no obstacle: the map is all the planner knows."""
    B, N = ROUND_B, ROUND_N
    p = O.default_params(N)
    p.safe_length, p.safe_width = SAFE
    p.w_uncertainty = ROUND_W_UNCERTAINTY
    path = np.stack([np.arange(200.0), np.zeros(200)], 1)
    x0 = np.zeros((B, 4))
    x0[:, 1], x0[:, 2] = -1.0 + 0.4 * np.arange(B), 4.0
    poly, fl = np.zeros((B, 6)), np.zeros((B, 2))
    for b in range(B):
        c, ref = O.local_plan(p, path, x0[b])
        poly[b], fl[b] = c, (ref[0, 0], ref[-1, 0])
    U0 = np.zeros((B, N, 2))
    O.lib().oracle_default_control_seq(N, _p(U0[0]))
    U0[:] = U0[0]
    g = O.map_geom(*GEOM_A)
    return dict(p=p, B=B, N=N, x0=x0, U0=U0.reshape(B, -1), poly=poly, fl=fl, geom=GEOM_A, g=g, layers=blob_layer(g, POSE_A), poses=POSE_A,
                probes=(3, 3), kappa=kappa_of(ROUND_EPS), cap=1.0, sigma0=SIGMA0.T.reshape(16), W=W_DIAG.T.reshape(16))


def kappa_of(eps):
    """The kappa with erfc(kappa / sqrt 2) / 2 = eps, by bisection on math.erfc."""
    lo, hi = 0.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if 0.5 * math.erfc(mid / math.sqrt(2.0)) > eps else (lo, mid)
    return 0.5 * (lo + hi)


def _map_risk(s, X, sigma):
    nodes, weights = np_quadrature(5, 5, 3)
    return restate_map(s["p"], s["probes"], s["N"], X, sigma, nodes, weights, s["g"], s["layers"], s["poses"], ROUND_THRESHOLD)[False]


def _round_after(O, s, X1, U1, K1):
    """From a first plan and its gains: the restated Sigma_t, the restated tightened layers, the oracle's re-solve on them from U1, and
    CM_STEP_RISK of both plans against the ORIGINAL map (the second plan's own gains from the oracle, without a map term)."""
    B, N, p = s["B"], s["N"], s["p"]
    th = min(8, O.max_threads())
    sigma1 = restate(p, N, X1, U1, K1, s["sigma0"], s["W"], None, None)["sigma"]
    tm = tighten_map_restate(p, N, X1, sigma1, s["g"], s["layers"], s["poses"], s["kappa"], s["cap"])
    um, keep = O.uncertainty_map(tm["layer"], s["g"], s["poses"], s["probes"], batched=True)
    second = O.solve_batch_unc(p, N, 0, s["x0"], U1, s["poly"], s["fl"], None, None, None, um, threads=th)
    _, K2, ok = o_gains(O, p, N, second["X"], second["U"], s["poly"], s["fl"])
    assert np.all(ok == 1)
    sigma2 = restate(p, N, second["X"], second["U"], K2, s["sigma0"], s["W"], None, None)["sigma"]
    return dict(sigma1=sigma1, tm=tm, second=second, K2=K2, sigma2=sigma2, risk0=_map_risk(s, X1, sigma1), risk1=_map_risk(s, second["X"], sigma2))


@pytest.fixture(scope="module")
def round_m(oracle):
    """One round on the CPU, from the reference pipeline alone: oracle.solve_batch_unc -> oracle gains -> `restate` (Sigma_t) -> this
    restatement -> solve_batch_unc on the tightened layers -> `restate_map` against the ORIGINAL map."""
    O = oracle
    s = _round_scene(O)
    um, keep = O.uncertainty_map(s["layers"], s["g"], s["poses"], s["probes"])
    first = O.solve_batch_unc(s["p"], s["N"], 0, s["x0"], s["U0"], s["poly"], s["fl"], None, None, None, um, threads=min(8, O.max_threads()))
    _, K1, ok = o_gains(O, s["p"], s["N"], first["X"], first["U"], s["poly"], s["fl"])
    assert np.all(ok == 1)
    out = _round_after(O, s, first["X"], first["U"], K1)
    out.update(s=s, first=first, K1=K1)
    return out


def test_one_round_on_the_cpu_does_what_it_is_for(round_m):
    """A condition on the scene, not a measurement of the kernel: under the original map one candidate's footprint is in contact
    (CM_STEP_RISK above one half), and one round of the reference pipeline at least halves its CM_STEP_RISK against the ORIGINAL map."""
    a = round_m
    r0, r1 = a["risk0"]["risk"][:, CM_STEP_RISK], a["risk1"]["risk"][:, CM_STEP_RISK]
    print("CM_STEP_RISK before %s\n             after  %s\nraised cells %s, iterations %s -> %s" % (
        np.round(r0, 6).tolist(), np.round(r1, 6).tolist(), a["tm"]["fields"][:, RAISED].tolist(), a["first"]["iters"].tolist(),
        a["second"]["iters"].tolist()))
    k = int(np.argmax(r0))
    assert r0[k] > 0.5 and r1[k] <= 0.5 * r0[k]
    assert np.all(r1 <= r0 + 1e-12) and np.all(a["tm"]["fields"][:, RAISED] > 0)
    assert not a["tm"]["border"].any()


def _round_params(cilqr, N):
    p = _params(cilqr, N)
    p.w_uncertainty = ROUND_W_UNCERTAINTY
    return p


@gpu
def test_pipeline_one_round(cilqr, round_m):
    """One round, every call in its device form on one stream: solve with the map set -> gains (the map cleared for this call alone: the
    oracle's backward pass has no map term) -> chance risk with M = 0 (sigma_out) -> tighten_map -> the tightened per-solve layers set ->
    re-solve from the first solve's U; then the map risk of both plans against the ORIGINAL map.  Against the same sequence on the oracle
    and the restatements: iterations and exits equal, max|dU| <= 1e-8 after the warm-started second solve (the bar of
    test_warm_start_second_tick), the layers bit for bit, CM_STEP_RISK before and after within 1e-9, and the same strict decrease."""
    import torch
    a = round_m
    s = a["s"]
    B, N, g = s["B"], s["N"], s["g"]
    cells = int(g.rows) * int(g.cols)
    geom = cilqr.map_geom(*s["geom"])
    nodes, weights = np_quadrature(5, 5, 3)
    Q = weights.shape[0]
    solver = cilqr.Solver(_round_params(cilqr, N), max_batch=B, max_horizon=N, max_obstacles=0, device=0)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
        zi = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        ptr = lambda t: t.data_ptr()  # noqa: E731
        x0, U, poly, fl, s0, W, qn, qw = (up(v) for v in (s["x0"], s["U0"], s["poly"], s["fl"], s["sigma0"], s["W"], nodes, weights))
        layer = torch.from_numpy(np.ascontiguousarray(np.asfortranarray(s["layers"]).flatten(order="F"))).to(dev)
        tight = torch.zeros((B, cells), dtype=torch.float32, device=dev)
        X, J, it, ex = z(B, 4 * (N + 1)), z(B), zi(B), zi(B)
        X2, J2, it2, ex2 = z(B, 4 * (N + 1)), z(B), zi(B), zi(B)
        k, K, ok, k2, K2, ok2 = z(B, 2 * N), z(B, 8 * N), zi(B), z(B, 2 * N), z(B, 8 * N), zi(B)
        risk, sig, sig2, tm, mrisk, mrisk2 = z(B, 6), z(B, N + 1, 16), z(B, N + 1, 16), z(B, 6), z(B, 8), z(B, 8)
        none = (0, 0, 0, 0)
        original = lambda: solver.set_uncertainty_map_device(ptr(layer), geom, s["poses"], s["probes"])  # noqa: E731
        torch.cuda.synchronize(dev)
        original()
        solver.solve_batch_device(st, B, N, 0, ptr(x0), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, ptr(X), ptr(J), ptr(it), ptr(ex))
        U1 = U.clone()
        solver.clear_uncertainty_map()
        solver.gains_batch_device(st, B, N, 0, ptr(X), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, none, ptr(k), ptr(K), ptr(ok))
        original()
        solver.chance_risk_device(st, B, N, 0, ptr(X), ptr(U), ptr(K), ptr(s0), 0, ptr(W), 0, 0, none, ptr(risk), sigma_out=ptr(sig))
        solver.chance_risk_map_device(st, B, N, Q, ptr(X), ptr(sig), ptr(qn), ptr(qw), ROUND_THRESHOLD, ptr(mrisk))
        solver.tighten_map_device(st, B, N, ptr(X), ptr(sig), ptr(tight), ptr(tm), kappa=cilqr.chance_kappa(ROUND_EPS), max_inflate=s["cap"])
        solver.set_uncertainty_map_device(ptr(tight), geom, s["poses"], s["probes"], layer_stride=cells)
        solver.solve_batch_device(st, B, N, 0, ptr(x0), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, ptr(X2), ptr(J2), ptr(it2), ptr(ex2))
        solver.clear_uncertainty_map()
        solver.gains_batch_device(st, B, N, 0, ptr(X2), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, none, ptr(k2), ptr(K2), ptr(ok2))
        original()
        solver.chance_risk_device(st, B, N, 0, ptr(X2), ptr(U), ptr(K2), ptr(s0), 0, ptr(W), 0, 0, none, ptr(risk), sigma_out=ptr(sig2))
        solver.chance_risk_map_device(st, B, N, Q, ptr(X2), ptr(sig2), ptr(qn), ptr(qw), ROUND_THRESHOLD, ptr(mrisk2))
        torch.cuda.synchronize(dev)
        solver.clear_uncertainty_map()
    finally:
        solver.close()
    n = lambda t: t.cpu().numpy()  # noqa: E731
    assert abs(cilqr.chance_kappa(ROUND_EPS) - s["kappa"]) <= 1e-12
    d1, d2 = float(np.max(np.abs(n(U1) - a["first"]["U"]))), float(np.max(np.abs(n(U) - a["second"]["U"])))
    r0, r1 = n(mrisk)[:, CM_STEP_RISK], n(mrisk2)[:, CM_STEP_RISK]
    w0, w1 = a["risk0"]["risk"][:, CM_STEP_RISK], a["risk1"]["risk"][:, CM_STEP_RISK]
    got_layers = _layers_of(n(tight), g)
    differ = _bits32(got_layers) != _bits32(a["tm"]["layer"])
    print("first solve max|dU| %.3g, iterations %s; after the round max|dU| %.3g, iterations %s (oracle %s); %d tightened cells differ\n"
          "CM_STEP_RISK before %s (CPU %s)\n             after  %s (CPU %s)" % (d1, n(it).tolist(), d2, n(it2).tolist(), a["second"]["iters"].tolist(),
                                                                               differ.sum(), r0.tolist(), w0.tolist(), r1.tolist(), w1.tolist()))
    assert np.array_equal(n(it), a["first"]["iters"]) and np.array_equal(n(ex), a["first"]["status"]) and np.all(n(ok) == 1)
    _close(n(sig).reshape(B, -1), a["sigma1"].reshape(B, -1), "Sigma_t of the first plan")
    # (the kernel's Sigma_t is the device's, 1e-9 from the restated one: a cell may differ where the restatement is borderline at THAT width)
    assert differ.sum() <= 0.001 * differ.size
    assert np.array_equal(n(tm)[:, [CAPPED, LOST]], a["tm"]["fields"][:, [CAPPED, LOST]])
    assert np.array_equal(n(it2), a["second"]["iters"]) and np.array_equal(n(ex2), a["second"]["status"])
    assert d2 <= 1e-8
    assert np.max(np.abs(r0 - w0)) <= CM_TOL and np.max(np.abs(r1 - w1)) <= CM_TOL
    kk = int(np.argmax(w0))
    assert r0[kk] > 0.5 and r1[kk] < r0[kk] and r1[kk] <= 0.5 * r0[kk]


def _restated_pipeline_of_the_dump(O, path):
    """What tests/cpp/candidates_map_tightened.cpp wrote -> the restated pipeline from the first plans and gains it solved: Sigma_t by
    `restate`, the tightened layers by this restatement, the oracle's re-solve on them."""
    v = open(path).read().split()
    B, N, rows, cols, best = (int(x) for x in v[:5])
    a = np.array([float(x) for x in v[5:]])
    take = lambda n, at=[0]: (a[at[0]:at[0] + n], at.__setitem__(0, at[0] + n))[0]  # noqa: E731
    kappa, cap, w_unc = take(3)
    geom, pose = tuple(take(5)), tuple(take(3))
    x0, poly, fl = take(B * 4).reshape(B, 4), take(B * 6).reshape(B, 6), take(B * 2).reshape(B, 2)
    X1, U1, K1 = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1), take(B * 8 * N).reshape(B, -1)
    sigma0, W = take(16), take(16)
    X2, U2, J2, tm = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1), take(B), take(B * 6).reshape(B, 6)
    iters = take(B).astype(np.int32)
    layer = take(rows * cols).astype(np.float32).reshape(cols, rows).T  # written column-major
    tight = take(B * rows * cols).astype(np.float32).reshape(B, cols, rows).transpose(0, 2, 1)
    p = O.default_params(N)
    p.safe_length, p.safe_width = SAFE
    p.w_uncertainty = w_unc
    g = O.map_geom(*geom)
    assert (g.rows, g.cols) == (rows, cols)
    s = dict(p=p, B=B, N=N, x0=x0, poly=poly, fl=fl, geom=geom, g=g, layers=layer, poses=pose, probes=(3, 3), kappa=kappa, cap=cap, sigma0=sigma0, W=W)
    out = _round_after(O, s, np.ascontiguousarray(X1), np.ascontiguousarray(U1), np.ascontiguousarray(K1))
    out.update(s=s, best=best, got=dict(X=X2, U=U2, J=J2, tm=tm, iters=iters, tight=tight))
    return out


@gpu
def test_cpp_facade_map_tightened_candidates(oracle, tmp_path):
    """tests/cpp/candidates_map_tightened.cpp: run_candidates and run_step under iLQR::set_map_tightening against the C-ABI sequence called
    by hand, bit for bit (inside the program: picks, last_tighten_map, the map on the handle before and after, the off switches, the
    conflicts, the composition with set_chance_tightening), and against the restated pipeline for the candidates it solved (here): the
    tightened layers, the re-solved plans within 1e-8, the iteration counts, the pick."""
    exe, dump = str(tmp_path / "candidates_map_tightened"), str(tmp_path / "dump.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_map_tightened.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("map tightened pick ok", "map restored ok", "run_step ok", "off switches ok", "conflicts throw ok", "chance off beside map ok", "composed ok"):
        assert line in r.stdout, r.stdout
    a = _restated_pipeline_of_the_dump(oracle, dump)
    got, want = a["got"], a["second"]
    differ = _bits32(got["tight"]) != _bits32(a["tm"]["layer"])
    dU = float(np.max(np.abs(got["U"] - want["U"])))
    print("tightened cells that differ %d of %d; max|dU| %.3g; iterations %s (oracle %s); J %s" % (
        differ.sum(), differ.size, dU, got["iters"].tolist(), want["iters"].tolist(), got["J"].tolist()))
    assert differ.sum() <= 0.001 * differ.size
    assert np.array_equal(got["tm"][:, [CAPPED, LOST]], a["tm"]["fields"][:, [CAPPED, LOST]])
    assert np.max(np.abs(got["tm"][:, RAISED] - a["tm"]["fields"][:, RAISED])) <= 0.001 * differ[0].size
    assert np.array_equal(got["iters"], want["iters"]) and dU <= 1e-8
    gaps = np.diff(np.sort(want["J"]))
    assert gaps.min() > 1e-6 and a["best"] == int(np.argmin(want["J"]))  # the pick is decided, and it is the restated pipeline's
    assert np.max(np.abs(got["X"] - want["X"])) <= 1e-7
