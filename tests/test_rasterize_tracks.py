"""Predicted tracks rasterised into the costmap along each plan (cilqr_rasterize_tracks*, include/cilqr.h): per solve a copy of the layer
set on the handle in which every cell is raised to 100 x the probability that a predicted vehicle covers it, at the steps when that
solve's plan is near the cell (or over the whole horizon, swept mode).

Expected values never come from the HIP path: `tracks_restate` below is a numpy restatement of the header's definition, written from the
header, with torch.erf in float64 (math.erf where torch is missing) and, once, in np.longdouble with a series of positive terms for erf.
The values v = (float)(100 p) are compared within 1 float32 ulp on every cell that is not BORDERLINE: within 1e-9 relative of a reach
test (which is the indicator's edge where su = 0), or with its two smallest step distances within 1e-9 relative.  Bit-copied cells by
bits.  Counts exactly where a solve has no borderline cell and no cell whose v sits within 1 ulp of its input; TKM_MAX_CELL and
TKM_MAX_ENTRY exactly where the runner-up is more than 1 ulp away.

The issue's 257-cell map does not exist: 257 is prime and cilqr_set_uncertainty_map needs two rows and two columns.  6 x 43 = 258 cells,
the smallest map above one tile of 256, stands in for it (a second workgroup with two cells), beside 15 x 17 = 255 and 16 x 16 = 256.
The records kernel forms 256 entries per workgroup: M*N = 255, 256 and 257 are cases e255, e256 and e257 (N = 1).

  case     map        N   M    window  mode    form     tracks  map
  tiny     3 x 5      2   1    0       along   product  shared  shared
  t256     16 x 16    64  3    1       along   MIN      dense   per solve
  t258     6 x 43     65  3    2       along   product  dense   shared
  t255     15 x 17    65  1    70      along   MIN      shared  per solve
  s256     16 x 16    64  3    -       swept   product  shared  shared
  s258     6 x 43     2   3    -       swept   MIN      dense   per solve
  e255     16 x 16    1   255  0       along   product  shared  shared
  e256     16 x 16    1   256  -       swept   product  dense   shared
  e257     3 x 5      1   257  1       along   MIN      shared  shared
  node     150 x 100  64  3    2       along   product  shared  shared
  nodes    150 x 100  2   3    -       swept   product  shared  shared
Every case has B = 3, a layer with NaN cells, NaN entries, one lost plan step in solve 0 and every step lost in solve 2 (along mode).

Exact probability (scipy): over 60 random entries and cells with correlations up to 0.9 in the vehicle's frame the product form is up to
0.0547 away from the exact rectangle probability at |rho| <= 0.6, the scenes' correlations, and 0.107 up to 0.9
(measured by test_exact_probability, printed there); the MIN form was never below the exact value by more than 1.4e-17.

Purpose (test_one_round_on_the_cpu_does_what_it_is_for, measured on the CPU, oracle solves): see that test's docstring.
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
from test_chance_risk import SIGMA0, STEP_RISK, W_DIAG
from test_polygon_raster import inside_mask
from test_predict_obstacles import P0_T, _cm, predict_restate, restate_cov
from test_risk_map import SAFE, _params
from test_rollout_risk import o_gains

try:
    import torch
except ImportError:  # the restatement then takes math.erf
    torch = None

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
ENTRY_POINTS = ("cilqr_rasterize_tracks", "cilqr_rasterize_tracks_device")
FIELDS = ("RAISED", "MAX_VALUE", "MAX_CELL", "MAX_ENTRY", "LOST_ENTRIES", "LOST_STEPS")
RAISED, MAX_VALUE, MAX_CELL, MAX_ENTRY, LOST_ENTRIES, LOST_STEPS = range(6)
BORDER = 1e-9
SIGMA_MIN = 1e-150
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- expected values: a numpy restatement of the header's definition ----------------------------------------------------------------
def _erf(x, T):
    """erf elementwise.  float64: torch.erf (math.erf without torch).  longdouble: 2/sqrt(pi) exp(-x^2) sum 2^n x^(2n+1)/(2n+1)!!, every
    term positive, |x| cut at 6.5 (erf = 1 to 4e-20 there)."""
    x = np.asarray(x, dtype=T)
    if T is np.float64:
        if torch is not None:
            return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()
        return np.array([math.erf(v) for v in x.reshape(-1)]).reshape(x.shape)
    sign, ax = np.sign(x), np.minimum(np.abs(x), T(6.5))
    total = np.zeros(ax.shape, dtype=T)
    for lo, hi, terms in ((-1.0, 1.5, 45), (1.5, 3.5, 90), (3.5, 7.0, 170)):  # (the terms fall below 1e-22 of the sum within these counts)
        pick = (ax > lo) & (ax <= hi)
        if not pick.any():
            continue
        a = ax[pick]
        term, acc = a.copy(), a.copy()
        for n in range(terms):
            term = term * (2 * a * a) / T(2 * n + 3)
            acc = acc + term
        total[pick] = acc
    return sign * (T(2) / np.sqrt(np.arccos(T(-1)))) * np.exp(-ax * ax) * total


def entry_records(N, pose, dim, cov, inflate, z_max, T=np.float64):
    """pose (M, N, 4), dim (M, N, 2), cov (M, N, 3) or None -> dict of (M, N) arrays: the entry records of the header, in precision T."""
    pose, dim = np.asarray(pose, dtype=np.float64), np.asarray(dim, dtype=np.float64)
    M = pose.shape[0]
    cv = np.zeros((M, N, 3)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(M, N, 3)
    live = np.isfinite(pose[..., [0, 1, 3]]).all(axis=-1) & np.isfinite(dim).all(axis=-1) & np.isfinite(cv).all(axis=-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x, y, th = pose[..., 0].astype(T), pose[..., 1].astype(T), pose[..., 3].astype(T)
        co, so = np.cos(th), np.sin(th)
        hl, hw = (dim[..., 0].astype(T) + T(inflate)) / 2, (dim[..., 1].astype(T) + T(inflate)) / 2
        cxx, cxy, cyy = (cv[..., k].astype(T) for k in range(3))
        cc, ss, cs = co * co, so * so, co * so
        su2 = cc * cxx + 2 * cs * cxy + ss * cyy
        sw2 = ss * cxx - 2 * cs * cxy + cc * cyy
        su, sw = np.sqrt(np.where(su2 < 0, 0, su2)), np.sqrt(np.where(sw2 < 0, 0, sw2))
        root2 = np.sqrt(T(2))
        ku = np.where(su >= SIGMA_MIN, 1 / np.where(su >= SIGMA_MIN, su * root2, 1), 0)
        kw = np.where(sw >= SIGMA_MIN, 1 / np.where(sw >= SIGMA_MIN, sw * root2, 1), 0)
        ru, rw = hl + T(z_max) * su, hw + T(z_max) * sw
    return dict(x=x, y=y, co=co, so=so, hl=hl, hw=hw, ku=ku, kw=kw, ru=ru, rw=rw, live=live)


def entry_prob(r, m, t, wx, wy, bound_min, T=np.float64, part=True):
    """Entry (m, t) of `r` at the points (wx, wy): (p, reach mask, borderline mask).  p is 0 outside the reach, and outside `part` (the
    points whose window holds t)."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = wx - r["x"][m, t], wy - r["y"][m, t]
        du, dw = r["co"][m, t] * dx + r["so"][m, t] * dy, r["co"][m, t] * dy - r["so"][m, t] * dx
        hl, hw, ku, kw, ru, rw = (r[k][m, t] for k in ("hl", "hw", "ku", "kw", "ru", "rw"))
        au, aw = np.abs(du), np.abs(dw)
        reach = bool(r["live"][m, t]) & (au <= ru) & (aw <= rw) & part
        border = bool(r["live"][m, t]) & (((np.abs(au - ru) <= BORDER * ru) & (aw <= rw * (1 + BORDER)))
                                          | ((np.abs(aw - rw) <= BORDER * rw) & (au <= ru * (1 + BORDER))))
        p = np.zeros(np.shape(wx), dtype=T)
        if np.any(reach):
            u, w = du[reach], dw[reach]
            pu = 0.5 * (_erf((u + hl) * ku, T) - _erf((u - hl) * ku, T)) if ku > 0 else (np.abs(u) <= hl).astype(T)
            pw = 0.5 * (_erf((w + hw) * kw, T) - _erf((w - hw) * kw, T)) if kw > 0 else (np.abs(w) <= hw).astype(T)
            p[reach] = np.minimum(pu, pw) if bound_min else pu * pw
    return p, reach, border


def _solve_restate(g, layer, mpose, N, X, r, window, bound_min, T=np.float64):
    """One solve.  layer (rows, cols) float32, mpose (x, y, theta) of the map, X (N+1, 4) or None (swept), r = entry_records."""
    rows, cols, res = int(g.rows), int(g.cols), float(g.res)
    x_first = g.pos_x + (0.5 * g.len_x - 0.5 * g.res)
    y_first = g.pos_y + (0.5 * g.len_y - 0.5 * g.res)
    M = r["x"].shape[0]
    c, s = (math.cos(mpose[2]), math.sin(mpose[2])) if T is np.float64 else (np.cos(T(mpose[2])), np.sin(T(mpose[2])))
    c, s, px0, py0 = T(c), T(s), T(mpose[0]), T(mpose[1])
    mx = (T(x_first) - np.arange(rows).astype(T) * T(res))[:, None] + np.zeros((1, cols), dtype=T)
    my = (T(y_first) - np.arange(cols).astype(T) * T(res))[None, :] + np.zeros((rows, 1), dtype=T)
    border = np.zeros((rows, cols), dtype=bool)
    lost_steps = 0
    t_lo, t_hi = np.zeros((rows, cols), dtype=np.int64), np.full((rows, cols), N - 1, dtype=np.int64)
    if X is not None:
        Xs = np.asarray(X, dtype=np.float64).reshape(N + 1, 4)[:N]
        live = np.isfinite(Xs[:, :2]).all(axis=1)
        lost_steps = N - int(live.sum())
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = Xs[:, 0].astype(T) - px0, Xs[:, 1].astype(T) - py0
            ptx, pty = c * dx + s * dy, c * dy - s * dx
            ex, ey = mx[:, :, None] - ptx, my[:, :, None] - pty
            d2 = ex * ex + ey * ey
            d2 = np.where(live & np.isfinite(d2.astype(np.float64)), d2, np.inf)
        ts = d2.argmin(axis=2)  # the lowest t on equal values
        has = np.isfinite(d2.min(axis=2).astype(np.float64))
        if N > 1 and T is np.float64:  # (ties are looked for in float64, the precision the kernel decides them in)
            two = np.sort(np.partition(d2, 1, axis=2)[:, :, :2], axis=2)
            with np.errstate(invalid="ignore"):
                border |= has & np.isfinite(two[:, :, 1].astype(np.float64)) & (two[:, :, 1] - two[:, :, 0] <= BORDER * two[:, :, 1])
        t_lo = np.where(has, np.maximum(0, ts - window), 0)
        t_hi = np.where(has, np.minimum(N - 1, ts + window), -1)
    wx, wy = px0 + (c * mx - s * my), py0 + (s * mx + c * my)
    best_p, best_e = np.zeros((rows, cols), dtype=T), np.full((rows, cols), -1, dtype=np.int64)
    second = np.zeros((rows, cols), dtype=T)  # the largest p of another entry: decides whether TKM_MAX_ENTRY is pinned
    for m in range(M):
        for t in range(N):
            if not r["live"][m, t]:
                continue
            part = (t_lo <= t) & (t <= t_hi)
            if not part.any():
                continue
            p, reach, bd = entry_prob(r, m, t, wx, wy, bound_min, T, part)
            border |= bd & part
            up = p > best_p
            second = np.where(up, best_p, np.maximum(second, p))
            best_e = np.where(up, m * N + t, best_e)
            best_p = np.where(up, p, best_p)
    own = np.asarray(layer, dtype=np.float32)
    v = (100 * best_p).astype(np.float64).astype(np.float32)
    with np.errstate(invalid="ignore"):
        take = (v > 0) & (np.isnan(own) | (own < v))
    out = np.where(take, v, own).astype(np.float32)
    fields = np.zeros(6)
    fields[RAISED] = take.sum()
    fields[MAX_CELL] = fields[MAX_ENTRY] = -1.0
    if (v > 0).any():
        flat = v.flatten(order="F")  # index i + rows*j; argmax: the lowest on equal values
        k = int(flat.argmax())
        fields[MAX_VALUE], fields[MAX_CELL], fields[MAX_ENTRY] = float(flat[k]), k, float(best_e.flatten(order="F")[k])
    fields[LOST_ENTRIES] = (~r["live"]).sum()
    fields[LOST_STEPS] = lost_steps
    return dict(layer=out, v=v, p=best_p.astype(np.float64) if T is np.float64 else best_p, e=best_e, second=second.astype(np.float64),
                take=take, fields=fields, border=border)


def tracks_restate(g, layers, mposes, N, X, pose, dim, cov, inflate, z_max, window, bound_min, B=None, T=np.float64):
    """layers / mposes one shared or lists of B; X (B, 4(N+1)) or None with B given (swept); pose (M, 4N) shared or (B, M, 4N), dim and cov
    (3N columns or None) alike.  Returns dict(layer (B, rows, cols) float32, v, p, e, second, take, fields (B, 6), border)."""
    B = X.shape[0] if X is not None else B
    pose = np.asarray(pose, dtype=np.float64)
    shared = pose.ndim == 2
    per_map = isinstance(layers, list)
    rec_shared = entry_records(N, pose.reshape(pose.shape[0], N, 4), np.asarray(dim).reshape(pose.shape[0], N, 2),
                               None if cov is None else np.asarray(cov).reshape(pose.shape[0], N, 3), inflate, z_max, T) if shared else None
    each = []
    for b in range(B):
        r = rec_shared if shared else entry_records(N, pose[b].reshape(-1, N, 4), np.asarray(dim)[b].reshape(-1, N, 2),
                                                    None if cov is None else np.asarray(cov)[b].reshape(-1, N, 3), inflate, z_max, T)
        each.append(_solve_restate(g, layers[b] if per_map else layers, mposes[b] if per_map else mposes, N,
                                   None if X is None else X[b], r, window, bound_min, T))
    return {k: np.stack([e[k] for e in each]) for k in each[0]}


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _geom_of(rows, cols, res):
    """A map of rows x cols cells ahead of its pose: x in [0, rows*res], y centred."""
    return (rows * res, cols * res, res, 0.5 * rows * res, 0.0)


def _layer(rows, cols, seed):
    """(rows, cols) float32 in 0 ... 60 with cells at 0 and at 100 and one cell in twenty (at least two) unknown."""
    rng = np.random.Generator(np.random.PCG64(seed))
    layer = rng.uniform(0.0, 60.0, (rows, cols)).astype(np.float32)
    flat = rng.choice(rows * cols, max(4, rows * cols // 8), replace=False)
    q = len(flat) // 4
    layer[flat[:q] % rows, flat[:q] // rows] = 0.0
    layer[flat[q:2 * q] % rows, flat[q:2 * q] // rows] = 100.0
    n_nan = max(2, rows * cols // 20)
    layer[flat[2 * q:2 * q + n_nan] % rows, flat[2 * q:2 * q + n_nan] // rows] = np.nan
    return layer


def _mk_tracks(rng, sets, M, N, Lx, Ly, scale):
    """sets x M tracks that cross a map of Lx x Ly metres in N steps: pose (sets, M, 4N), dim (sets, M, 2N), cov (sets, M, 3N).  The
    covariance grows along the horizon, its correlation is up to 0.6 either way; each track's first entry has none (the indicator)."""
    pose, dim, cov = np.zeros((sets, M, N, 4)), np.zeros((sets, M, N, 2)), np.zeros((sets, M, N, 3))
    t = np.arange(N)
    for k in range(sets):
        for m in range(M):
            x0, y0 = rng.uniform(0.1, 0.9) * Lx, rng.uniform(-0.4, 0.4) * Ly
            th, w = rng.uniform(-3.1, 3.1), rng.uniform(-0.02, 0.02)
            step = rng.uniform(0.2, 0.6) * min(Lx, Ly) / max(N, 4)
            heading = th + w * t
            pose[k, m, :, 0] = x0 + np.cumsum(step * np.cos(heading)) - step * np.cos(heading[0])
            pose[k, m, :, 1] = y0 + np.cumsum(step * np.sin(heading)) - step * np.sin(heading[0])
            pose[k, m, :, 2], pose[k, m, :, 3] = step / 0.1, heading
            dim[k, m, :, 0], dim[k, m, :, 1] = rng.uniform(3.0, 5.0) * scale, rng.uniform(1.5, 2.2) * scale
            sx, sy = rng.uniform(0.1, 0.4) * scale * (1 + 0.05 * t), rng.uniform(0.1, 0.4) * scale * (1 + 0.05 * t)
            rho = rng.uniform(-0.6, 0.6)
            cov[k, m, :, 0], cov[k, m, :, 1], cov[k, m, :, 2] = sx * sx, rho * sx * sy, sy * sy
            cov[k, m, 0] = 0.0
    return pose.reshape(sets, M, 4 * N), dim.reshape(sets, M, 2 * N), cov.reshape(sets, M, 3 * N)


def _mk(O, seed, rows, cols, res, N, M, window, along, bound_min, dense, per_map, B=3, inflate=0.2, z_max=3.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    geom = _geom_of(rows, cols, res)
    g = O.map_geom(*geom)
    assert (int(g.rows), int(g.cols)) == (rows, cols)
    Lx, Ly = rows * res, cols * res
    scale = min(1.0, min(Lx, Ly) / 4.0)
    pose, dim, cov = _mk_tracks(rng, B if dense else 1, M, N, Lx, Ly, scale)
    if not dense:
        pose, dim, cov = pose[0], dim[0], cov[0]
    # NaN entries: a pose, a dimension and a covariance entry (the speed, pose[2], is not read)
    fp, fd, fc = pose.reshape(-1, N, 4), dim.reshape(-1, N, 2), cov.reshape(-1, N, 3)
    fp[0, N - 1, 0] = np.nan
    fp[-1, 0, 2] = np.nan
    if fp.shape[0] * N > 2:
        fd[-1, N // 2, 1] = np.inf
        fc[fp.shape[0] // 2, N - 1, 1] = np.nan
    if per_map:
        layers = [_layer(rows, cols, seed * 10 + b) for b in range(B)]
        mposes = [(0.03 * Lx * b, -0.02 * Ly * b, 0.04 * (b + 1)) for b in range(B)]
    else:
        layers, mposes = _layer(rows, cols, seed * 10), (0.02 * Lx, -0.03 * Ly, 0.05)
    X = None
    if along:
        X = np.zeros((B, N + 1, 4))
        tt = np.arange(N + 1) / float(max(N, 1))
        for b in range(B):
            X[b, :, 0] = 0.05 * Lx + 0.9 * Lx * tt
            X[b, :, 1] = (-0.25 + 0.2 * b) * Ly + 0.2 * Ly * np.sin(2.0 * tt + 0.3 * b)
            X[b, :, 2], X[b, :, 3] = 5.0, 0.1 * b
        if N > 1:
            X[0, N // 2, 1] = np.nan   # solve 0: one lost step
        X[0, N, 0] = np.nan            # x_N is not visited
        X[0, 0, 3] = np.nan            # the heading is not read
        if B > 2:
            X[2, :, 0] = np.inf        # solve 2: every step lost
        X = X.reshape(B, -1)
    s = dict(geom=geom, g=g, rows=rows, cols=cols, N=N, M=M, B=B, window=window, along=along, bound_min=bound_min, dense=dense,
             per_map=per_map, layers=layers, poses=mposes, probes=(3, 3), X=X, pose=np.ascontiguousarray(pose), dim=np.ascontiguousarray(dim),
             cov=np.ascontiguousarray(cov), inflate=inflate, z_max=z_max)
    s["want"] = tracks_restate(g, layers, mposes, N, X, s["pose"], s["dim"], s["cov"], inflate, z_max, window, bound_min, B=B)
    return s


#            seed rows cols res   N   M    window along bound_min dense per_map
CASE_ARGS = {"tiny": (1, 3, 5, 1.0, 2, 1, 0, True, False, False, False),
             "t256": (2, 16, 16, 0.5, 64, 3, 1, True, True, True, True),
             "t258": (3, 6, 43, 0.5, 65, 3, 2, True, False, True, False),
             "t255": (4, 15, 17, 0.5, 65, 1, 70, True, True, False, True),
             "s256": (5, 16, 16, 0.5, 64, 3, 0, False, False, False, False),
             "s258": (6, 6, 43, 0.5, 2, 3, 0, False, True, True, True),
             "e255": (7, 16, 16, 0.5, 1, 255, 0, True, False, False, False),
             "e256": (8, 16, 16, 0.5, 1, 256, 0, False, False, True, False),
             "e257": (9, 3, 5, 1.0, 1, 257, 1, True, True, False, False),
             "node": (10, 150, 100, 0.1, 64, 3, 2, True, False, False, False),
             "nodes": (11, 150, 100, 0.1, 2, 3, 0, False, False, False, False)}
CASES = list(CASE_ARGS)


@pytest.fixture(scope="module")
def cases(oracle):
    """Every case's inputs and restatement.  Computed once; never modified."""
    return {name: _mk(oracle, *args) for name, args in CASE_ARGS.items()}


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_facade_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    assert re.search(r"#define\s+CILQR_TRACK_MAP_FIELDS\s+6\b", h) and re.search(r"#define\s+CILQR_TRACK_MAP_BOUND_MIN\s+1u\b", h)
    for i, name in enumerate(FIELDS):
        assert re.search(r"\bCILQR_TKM_%s\s*=\s*%d\b" % (name, i), h), name
        assert getattr(cilqr, "TKM_" + name) == i
    assert cilqr.TRACK_MAP_FIELDS == 6 and cilqr.TRACK_MAP_BOUND_MIN == 1
    assert callable(cilqr.Solver.rasterize_tracks) and callable(cilqr.Solver.rasterize_tracks_device)
    f = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_track_map\s*\(\s*double\s+inflate\s*,\s*double\s+z_max\s*,\s*int\s+window\s*,\s*int\s+rounds\s*=\s*1\s*,"
                     r"\s*bool\s+ellipses\s*=\s*true\s*\)", f)
    assert re.search(r"std::vector<double>\s+last_track_map\s*;", f)
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_rasterize_tracks\s*\(", plan)
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_track_map.hip" in mk and len(re.findall(r"build/cilqr_track_map\.o", mk)) == 2  # `check` and its resource list
    # the definition stands in the header, and says what it is and what it leaves out
    for phrase in ("soft, first-order, time-windowed occupancy", "It guarantees nothing", "LEFT OUT: the uncertainty of the track's heading",
                   "unknown\n *              stays unknown", "and the ORIGINAL map, always", "strict <, lowest t on"):
        assert phrase in full, phrase


def test_argument_errors_need_no_device(cilqr):
    """Every CILQR_ERR_ARG the header lists as decided before the handle is looked at (there is none here); valid arguments reach the
    handle check."""
    L = cilqr.lib()
    B, N, M = 2, 4, 3
    pose, dim, cov = np.zeros((M, 4 * N)), np.ones((M, 2 * N)), np.zeros((M, 3 * N))
    X, layer, fields = np.zeros((B, 4 * (N + 1))), np.zeros((B, 12), dtype=np.float32), np.zeros((B, 6))
    no_handle = C.c_void_p()
    d = C.c_double
    nan, inf = float("nan"), float("inf")

    def call(dev, B=B, N=N, M=M, inflate=0.2, z_max=3.0, window=2, flags=0, strides=(0, N, 1, 0), obs=True, **nulls):
        a = dict(pose=pose, dim=dim, layer=layer, fields=fields)
        a.update(nulls)
        o = cilqr.Obstacles(None if a["pose"] is None else a["pose"].ctypes.data, None if a["dim"] is None else a["dim"].ctypes.data, None,
                            *strides)
        f = L.cilqr_rasterize_tracks_device if dev else L.cilqr_rasterize_tracks
        head = (no_handle, None) if dev else (no_handle,)
        return f(*head, B, N, M, _p(X), C.byref(o) if obs else None, _p(cov), d(inflate), d(z_max), window, C.c_uint32(flags),
                 _p(a["layer"], _fp), _p(a["fields"]))

    for dev in (False, True):
        assert call(dev, obs=False) == ERR_ARG and b"null required pointer" in L.cilqr_last_error()
        for name in ("pose", "dim", "layer", "fields"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        for kw in (dict(B=0), dict(N=0), dict(M=0), dict(B=-1)):
            assert call(dev, **kw) == ERR_ARG and b"each must be at least 1" in L.cilqr_last_error(), kw
        for bad in (-1e-3, nan, inf, -inf):
            assert call(dev, inflate=bad) == ERR_ARG and b"inflate is negative or not finite" in L.cilqr_last_error(), bad
            assert call(dev, z_max=bad) == ERR_ARG and b"z_max is negative or not finite" in L.cilqr_last_error(), bad
        assert call(dev, window=-1) == ERR_ARG and b"window is negative" in L.cilqr_last_error()
        for k in range(3):
            st = [0, N, 1, 0]
            st[k] = -1
            assert call(dev, strides=tuple(st)) == ERR_ARG and b"negative stride" in L.cilqr_last_error(), k
        for flags in (2, 3, 0x80000000):
            assert call(dev, flags=flags) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error(), flags
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle
        assert call(dev, inflate=0.0, z_max=0.0, window=0, flags=1) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # zero is valid


@pytest.fixture(scope="module")
def cases_ld(cases):
    """The longdouble restatement of every case: its p per cell."""
    out = {}
    for name, s in cases.items():
        out[name] = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], s["X"], s["pose"], s["dim"], s["cov"], s["inflate"], s["z_max"],
                                   s["window"], s["bound_min"], B=s["B"], T=np.longdouble)
    return out


@pytest.mark.parametrize("name", CASES)
def test_conditions(cases, cases_ld, name):
    """On the restatement alone.  Precision: the float64 and longdouble restatements agree to 1e-9 relative on every non-zero p that is
    not borderline: the erf differences lose nothing at these shapes.  Borderline cells: at most 1 % of a case's cells.  And each case
    exercises what it is there for."""
    s, w, ld = cases[name], cases[name]["want"], cases_ld[name]
    cells = s["rows"] * s["cols"]
    ok = ~w["border"] & ~ld["border"]
    p64, pld = w["p"][ok], ld["p"][ok].astype(np.longdouble)
    both = (p64 > 0) | (pld > 0)
    rel = float(np.max(np.abs(p64[both] - pld[both]) / pld[both])) if both.any() else 0.0
    share = w["border"].sum() / float(w["border"].size)
    print("case %s: %d cells, borderline %d (share %.3g); non-zero p %d, smallest %.3g, float64 against longdouble %.3g relative; fields %s"
          % (name, cells, w["border"].sum(), share, both.sum(), p64[both].min() if both.any() else 0.0, rel, w["fields"].tolist()))
    assert rel <= 1e-9
    assert share <= 0.01
    own = np.stack(s["layers"]) if s["per_map"] else np.broadcast_to(s["layers"], w["layer"].shape)
    assert np.isnan(own).reshape(s["B"], -1).sum(axis=1).min() >= 2
    # unknown stays unknown where nothing reaches; a raised unknown cell takes v; no cell is lowered
    assert np.array_equal(_bits32(w["layer"][~w["take"]]), _bits32(own[~w["take"]]))
    assert np.array_equal(_bits32(w["layer"][w["take"]]), _bits32(w["v"][w["take"]]))
    if name in ("node", "nodes", "t258"):
        assert (np.isnan(own) & w["take"]).any()  # an unknown cell a vehicle reaches takes v
    with np.errstate(invalid="ignore"):
        assert not np.any(w["layer"] < own)
    assert np.all(w["fields"][:, LOST_ENTRIES] >= 1)
    live = [b for b in range(s["B"]) if not (s["along"] and b == 2)]
    assert np.all(w["fields"][live, RAISED] > 0) and np.all(w["fields"][live, MAX_VALUE] > 1.0)
    if s["along"]:
        assert w["fields"][:, LOST_STEPS].tolist() == [1.0 if s["N"] > 1 else 0.0, 0.0, float(s["N"])]
        assert np.array_equal(_bits32(w["layer"][2]), _bits32(own[2]))
        assert w["fields"][2].tolist()[:4] == [0.0, 0.0, -1.0, -1.0]
    else:
        assert not w["fields"][:, LOST_STEPS].any()
    if s["along"] and s["window"] < s["N"] and s["N"] > 2:
        # the window matters: the swept layer of the same inputs raises more
        sw = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], None, s["pose"], s["dim"], s["cov"], s["inflate"], s["z_max"], 0,
                            s["bound_min"], B=s["B"])
        assert np.all(sw["fields"][:2, RAISED] > w["fields"][:2, RAISED])
    if name == "t258":
        assert cells == 258
    if name in ("e255", "e256", "e257"):
        assert s["M"] * s["N"] == int(name[1:])
    if s["per_map"]:
        r = entry_records(s["N"], (s["pose"][1] if s["dense"] else s["pose"]).reshape(-1, s["N"], 4),
                          (s["dim"][1] if s["dense"] else s["dim"]).reshape(-1, s["N"], 2),
                          (s["cov"][1] if s["dense"] else s["cov"]).reshape(-1, s["N"], 3), s["inflate"], s["z_max"])
        alt = _solve_restate(s["g"], s["layers"][0], s["poses"][0], s["N"], None if s["X"] is None else s["X"][1], r, s["window"], s["bound_min"])
        assert not np.array_equal(_bits32(alt["layer"]), _bits32(w["layer"][1]))  # solve 1's own layer and pose matter


def _boxes_in_map_frame(pose, dim, mpose, N):
    """Corners of every (track, step) rectangle, inflate 0, in the map frame: (M*N, 4, 2)."""
    po, di = pose.reshape(-1, N, 4), dim.reshape(-1, N, 2)
    c, s = math.cos(mpose[2]), math.sin(mpose[2])
    out = []
    for m in range(po.shape[0]):
        for t in range(N):
            x, y, th = po[m, t, 0], po[m, t, 1], po[m, t, 3]
            hl, hw = di[m, t, 0] / 2, di[m, t, 1] / 2
            poly = []
            for a, b in ((hl, hw), (hl, -hw), (-hl, -hw), (-hl, hw)):
                wx, wy = x + math.cos(th) * a - math.sin(th) * b, y + math.sin(th) * a + math.cos(th) * b
                dx, dy = wx - mpose[0], wy - mpose[1]
                poly.append((c * dx + s * dy, c * dy - s * dx))
            out.append(poly)
    return np.array(out)


def _zero_cov_scene(O):
    rng = np.random.Generator(np.random.PCG64(41))
    rows, cols, res, N, M = 40, 30, 0.25, 12, 3
    geom = _geom_of(rows, cols, res)
    g = O.map_geom(*geom)
    pose, dim, _ = _mk_tracks(rng, 1, M, N, rows * res, cols * res, 0.6)
    return dict(geom=geom, g=g, rows=rows, cols=cols, N=N, M=M, B=1, pose=pose[0], dim=dim[0], poses=(0.4, -0.3, 0.07),
                layers=np.zeros((rows, cols), dtype=np.float32), probes=(3, 3))


def _zero_cov_want(s):
    g = s["g"]
    cx = (g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) - np.arange(s["rows"], dtype=np.float64) * g.res
    cy = (g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) - np.arange(s["cols"], dtype=np.float64) * g.res
    return inside_mask(cx, cy, _boxes_in_map_frame(s["pose"], s["dim"], s["poses"], s["N"]))


def test_zero_covariance_limit_is_the_polygon_rasteriser(oracle):
    """Swept, obs_cov NULL, inflate 0, a NaN-free zero layer: the cells at 100 are exactly the cells that test_polygon_raster's isInside
    marks for the union of the rectangles over all tracks and steps; every other cell keeps its 0.  No centre lies within 1e-9 relative
    (2e-9 m and more) of an edge."""
    s = _zero_cov_scene(oracle)
    w = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], None, s["pose"], s["dim"], None, 0.0, 3.0, 0, False, B=1)
    mask = _zero_cov_want(s)
    assert not w["border"].any()
    assert 50 < mask.sum() < mask.size - 50
    assert np.array_equal(w["layer"][0] == 100.0, mask) and np.all(w["layer"][0][~mask] == 0.0)
    assert w["fields"][0].tolist()[:2] == [float(mask.sum()), 100.0]


def test_exact_probability():
    """Against scipy.stats.multivariate_normal rectangle probabilities (abseps 1e-8) of the vehicle's centre in its own frame: the product
    form within 1e-7 where the body-frame covariance is diagonal; the MIN form >= exact - 1e-7 for correlated covariances (60 random
    entries and cells each, correlation up to 0.9).  The largest product-versus-exact gap at correlations up to 0.6, the scenes', is
    printed: 0.0547 when this was written (measured, not a bound), 0.107 up to 0.9."""
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.Generator(np.random.PCG64(5))

    def exact(du, dw, hl, hw, cb):
        f = lambda a, b: float(stats.multivariate_normal.cdf(np.array([a, b]), mean=[du, dw], cov=cb, allow_singular=True,  # noqa: E731
                                                             maxpts=4000000, abseps=1e-8, releps=1e-8))
        return f(hl, hw) - f(-hl, hw) - f(hl, -hw) + f(-hl, -hw)

    worst_diag, worst_min, gap, gap_scene = 0.0, 0.0, 0.0, 0.0
    for k in range(120):
        th = rng.uniform(-3.1, 3.1)
        su, sw = rng.uniform(0.1, 1.2), rng.uniform(0.1, 1.2)
        rho = 0.0 if k < 60 else rng.uniform(-0.9, 0.9)
        cb = np.array([[su * su, rho * su * sw], [rho * su * sw, sw * sw]])
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        cw = R @ cb @ R.T  # the planning frame's (xx, xy, yy)
        pose = np.array([[[rng.uniform(-3, 3), rng.uniform(-3, 3), 5.0, th]]])
        dim = np.array([[[rng.uniform(3, 5), rng.uniform(1.5, 2.2)]]])
        cov = np.array([[[cw[0, 0], cw[0, 1], cw[1, 1]]]])
        r = entry_records(1, pose, dim, cov, 0.2, 40.0)
        wx, wy = pose[0, 0, 0] + rng.uniform(-4, 4, 1), pose[0, 0, 1] + rng.uniform(-4, 4, 1)
        dx, dy = wx[0] - pose[0, 0, 0], wy[0] - pose[0, 0, 1]
        du, dw = math.cos(th) * dx + math.sin(th) * dy, math.cos(th) * dy - math.sin(th) * dx
        # (the records' own variances are the body frame's within rounding: su, sw)
        assert abs(1 / (r["ku"][0, 0] * math.sqrt(2)) - su) < 1e-9 and abs(1 / (r["kw"][0, 0] * math.sqrt(2)) - sw) < 1e-9
        want = exact(du, dw, float(r["hl"][0, 0]), float(r["hw"][0, 0]), cb)
        prod = float(entry_prob(r, 0, 0, wx, wy, False)[0][0])
        pmin = float(entry_prob(r, 0, 0, wx, wy, True)[0][0])
        if k < 60:
            worst_diag = max(worst_diag, abs(prod - want))
        else:
            worst_min = max(worst_min, want - pmin)
            gap = max(gap, abs(prod - want))
            if abs(rho) <= 0.6:
                gap_scene = max(gap_scene, abs(prod - want))
    print("diagonal: product against exact %.3g; correlated: exact - MIN at most %.3g; product against exact up to %.3g (|rho| <= 0.6: %.3g)"
          % (worst_diag, worst_min, gap, gap_scene))
    assert worst_diag <= 1e-7
    assert worst_min <= 1e-7


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_track_map.cpp: the plan of the host form at the shapes the header promises, against the arena of the earlier
    calls (tests/golden/host_arena_cap.json: it has not grown)."""
    import json
    exe = str(tmp_path / "host_plan_track_map")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_track_map.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "6 arrays at most of 16" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20
    assert "B 128 of max_batch 1024, max_horizon 50, max_obstacles 8, X and obs_cov" in r.stdout
    assert "(CILQR_ERR_ARG)" in r.stdout  # the whole batch does not fit: the header promises max_batch/8


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(_params(cilqr), max_batch=4, max_horizon=65, max_obstacles=257, device=0)
    yield s
    s.close()


FILL = -7.0  # what the output buffers hold before a call: no input layer holds it


def _layers_of(flat, rows, cols):
    return flat.reshape(flat.shape[0], cols, rows).transpose(0, 2, 1)


class _SetMap:
    """The case's map set on the solver for the solves `idx` (device buffers kept here); copies: a shared layer given as one equal copy
    per solve (the shared pose stays)."""

    def __init__(self, cilqr, solver, s, idx, copies=False):
        self.solver = solver
        g = cilqr.map_geom(*s["geom"])
        cells = s["rows"] * s["cols"]
        if s["per_map"]:
            flat = np.stack([np.asfortranarray(s["layers"][b]).flatten(order="F") for b in idx])
            self.layers = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0")
            self.poses = torch.from_numpy(np.ascontiguousarray([s["poses"][b] for b in idx], dtype=np.float64)).to("cuda:0")
            torch.cuda.synchronize()
            solver.set_uncertainty_map_device(self.layers.data_ptr(), g, (0.0, 0.0, 0.0), s["probes"], layer_stride=cells,
                                              poses_ptr=self.poses.data_ptr())
        elif copies:  # one equal copy of the shared layer per solve; the shared pose stays
            flat = np.stack([np.asfortranarray(s["layers"]).flatten(order="F")] * len(idx))
            self.layers = torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0")
            torch.cuda.synchronize()
            solver.set_uncertainty_map_device(self.layers.data_ptr(), g, s["poses"], s["probes"], layer_stride=cells)
        else:
            solver.set_uncertainty_map(s["layers"], g, s["poses"], s["probes"])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.solver.clear_uncertainty_map()


def _tracks_for(s, idx, repeat=False):
    """(pose, dim, cov, strides) for the solves idx; repeat: shared tracks given as one equal copy per solve (dense strides)."""
    N, M = s["N"], s["M"]
    if s["dense"]:
        return s["pose"][idx], s["dim"][idx], s["cov"][idx], (M * N, N, 1, 0)
    if repeat:
        rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[None], (len(idx),) + a.shape))  # noqa: E731
        return rep(s["pose"]), rep(s["dim"]), rep(s["cov"]), (M * N, N, 1, 0)
    return s["pose"], s["dim"], s["cov"], (0, N, 1, 0)


def _device(cilqr, solver, s, sel=None, cov="given", copies=False, repeat=False, along=None, keep=None):
    """The device form on torch buffers, for the solves `sel` of the case in that order."""
    idx = list(range(s["B"])) if sel is None else list(sel)
    B, N, M = len(idx), s["N"], s["M"]
    cells = s["rows"] * s["cols"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
    pose, dim, cv, strides = _tracks_for(s, idx, repeat)
    d_pose, d_dim = up(pose), up(dim)
    d_cov = None if cov == "null" else up(np.zeros_like(cv) if cov == "zero" else cv)
    along = s["along"] if along is None else along
    d_X = up(s["X"][idx]) if along else None
    out = torch.full((B, cells), FILL, dtype=torch.float32, device=dev)
    fields = torch.full((B, 6), FILL, dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    with _SetMap(cilqr, solver, s, idx, copies=copies):
        solver.rasterize_tracks_device(stream, B, N, M, d_X.data_ptr() if along else 0, d_pose.data_ptr(), d_dim.data_ptr(), strides,
                                       out.data_ptr(), fields.data_ptr(), obs_cov=0 if d_cov is None else d_cov.data_ptr(),
                                       inflate=s["inflate"], z_max=s["z_max"], window=s["window"],
                                       flags=cilqr.TRACK_MAP_BOUND_MIN if s["bound_min"] else 0)
        torch.cuda.synchronize(dev)
    if keep is not None:
        keep.update(out=out)
    return dict(layer=_layers_of(out.cpu().numpy(), s["rows"], s["cols"]), fields=fields.cpu().numpy())


def _host(cilqr, solver, s, sel=None):
    idx = list(range(s["B"])) if sel is None else list(sel)
    pose, dim, cv, _ = _tracks_for(s, idx)
    with _SetMap(cilqr, solver, s, idx):
        got = solver.rasterize_tracks(s["N"], (s["rows"], s["cols"]), pose, dim, obs_cov=cv, X=s["X"][idx] if s["along"] else None, B=len(idx),
                                      inflate=s["inflate"], z_max=s["z_max"], window=s["window"], bound_min=s["bound_min"])
    return dict(layer=np.ascontiguousarray(got["layer"]), fields=got["fields"])


def _same(a, b, sel_a=slice(None), sel_b=slice(None)):
    return np.array_equal(_bits32(a["layer"][sel_a]), _bits32(b["layer"][sel_b])) and np.array_equal(_bits(a["fields"][sel_a]), _bits(b["fields"][sel_b]))


def _ulp32(a, b):
    """Distance in float32 ulps between positive finite floats."""
    return np.abs(_bits32(a).astype(np.int64) - _bits32(b).astype(np.int64))


def _check_against(got, s, what, sel=None, w=None):
    idx = list(range(s["B"])) if sel is None else list(sel)
    w = s["want"] if w is None else w
    own = np.stack([s["layers"][b] for b in idx]) if s["per_map"] else np.broadcast_to(s["layers"], got["layer"].shape)
    wl, wv, take, border, wf = w["layer"][idx], w["v"][idx], w["take"][idx], w["border"][idx], w["fields"][idx]
    gl = got["layer"]
    assert not (gl == FILL).any(), what
    copied = _bits32(gl) == _bits32(own)
    # a cell the restatement copies is copied (by bits) unless v sits within 1 ulp of the input; a cell it raises holds v within 1 ulp
    near_own = np.zeros(wl.shape, dtype=bool)
    fin = np.isfinite(own) & (wv > 0) & (own > 0)
    near_own[fin] = _ulp32(wv[fin], own[fin]) <= 1
    d = np.zeros(wl.shape, dtype=np.int64)
    pos = take & (gl > 0) & np.isfinite(gl)
    d[pos] = _ulp32(gl[pos], wv[pos])
    bad_raise = take & ~border & ~((gl > 0) & np.isfinite(gl) & (d <= 1)) & ~(near_own & copied)
    bad_copy = ~take & ~border & ~copied & ~near_own
    # (a v of 0 in the restatement whose device value rounds above 0: p below 1e-47, out of reach of these shapes)
    print("%s: raised %d cells, %d of them 1 ulp from the restatement, none further; %d borderline cells; fields %s" % (
        what, take.sum(), (d == 1).sum(), border.sum(), got["fields"].tolist()))
    assert not bad_raise.any() and not bad_copy.any(), (what, np.argwhere(bad_raise)[:5], np.argwhere(bad_copy)[:5])
    assert np.array_equal(got["fields"][:, [LOST_ENTRIES, LOST_STEPS]], wf[:, [LOST_ENTRIES, LOST_STEPS]]), what
    for k, b in enumerate(idx):
        f, n_loose = got["fields"][k], int(border[k].sum() + near_own[k].sum())
        assert abs(f[RAISED] - wf[k][RAISED]) <= n_loose, (what, b, f, wf[k])
        if wf[k][MAX_VALUE] == 0.0:
            assert f[:4].tolist() == [0.0, 0.0, -1.0, -1.0], (what, b)
            continue
        top = np.float32(wf[k][MAX_VALUE])
        assert _ulp32(np.float32(f[MAX_VALUE]), top) <= 1 or border[k].any(), (what, b, f[MAX_VALUE], top)
        flat_v, flat_e = wv[k].flatten(order="F"), w["e"][idx][k].flatten(order="F")
        flat_p, flat_2 = w["p"][idx][k].flatten(order="F"), w["second"][idx][k].flatten(order="F")
        rivals = (flat_v < top) & (flat_v > 0) & (_ulp32(np.where(flat_v > 0, flat_v, top), top) <= 1)
        if not rivals.any() and not border[k].any():  # the runner-up is more than 1 ulp away: the cell is pinned
            assert f[MAX_CELL] == wf[k][MAX_CELL], (what, b, f, wf[k])
            cell = int(wf[k][MAX_CELL])
            if flat_2[cell] < flat_p[cell] * (1.0 - 2.0 ** -22):  # and so is the entry that gave it
                assert f[MAX_ENTRY] == float(flat_e[cell]), (what, b, f, wf[k])
        else:
            assert 0 <= f[MAX_CELL] < flat_v.size and _ulp32(flat_v[int(f[MAX_CELL])], top) <= 1 or border[k].any(), (what, b)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_layers_and_fields_against_the_restatement(cilqr, solver, cases, name):
    """The device form and the host form against the restatement; the two forms give the same bits; obs_cov NULL and all zeros give the
    same bits, and those are the restatement's without a covariance."""
    s = cases[name]
    dev = _device(cilqr, solver, s)
    _check_against(dev, s, "case %s, device form" % name)
    host = _host(cilqr, solver, s)
    assert _same(host, dev)
    null, zero = _device(cilqr, solver, s, cov="null"), _device(cilqr, solver, s, cov="zero")
    assert _same(null, zero)
    w0 = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], s["X"], s["pose"], s["dim"], None, s["inflate"], s["z_max"], s["window"],
                        s["bound_min"], B=s["B"])
    assert w0["border"].sum() <= 0.01 * w0["border"].size
    _check_against(null, s, "case %s, no covariance" % name, w=w0)
    if s["along"]:
        own = s["layers"][2] if s["per_map"] else s["layers"]
        assert np.array_equal(_bits32(dev["layer"][2]), _bits32(own)) and dev["fields"][2].tolist()[:4] == [0.0, 0.0, -1.0, -1.0]


@gpu
def test_a_result_depends_on_its_own_solve_alone(cilqr, solver, cases):
    """A solve's layer and fields are the same bits alone, in a batch, at another place in the batch, with shared inputs and with
    repeated inputs (layer and pose, tracks), and on a handle of other create sizes."""
    for name in ("t258", "s256", "node", "t256"):
        s = cases[name]
        whole = _device(cilqr, solver, s)
        for b in range(s["B"]):
            assert _same(_device(cilqr, solver, s, sel=[b]), whole, sel_b=slice(b, b + 1)), (name, b)
        for order in ([2, 0, 1], [1, 2, 0]):
            assert _same(_device(cilqr, solver, s, sel=order), whole, sel_b=order), (name, order)
        if not s["dense"]:
            assert _same(_device(cilqr, solver, s, repeat=True), whole), name
        if not s["per_map"]:
            assert _same(_device(cilqr, solver, s, copies=True), whole), name  # the layer shared, and one equal copy per solve
            if not s["dense"]:
                assert _same(_device(cilqr, solver, s, copies=True, repeat=True), whole), name
    s = cases["t258"]
    small = cilqr.Solver(_params(cilqr), max_batch=3, max_horizon=s["N"], max_obstacles=s["M"], device=0)
    try:
        assert _same(_device(cilqr, small, s), _device(cilqr, solver, s))
    finally:
        small.close()


@gpu
def test_zero_covariance_limit_on_the_device(cilqr, oracle, solver):
    """test_zero_covariance_limit_is_the_polygon_rasteriser on the device, and against cilqr_rasterize_polygons itself."""
    s = dict(_zero_cov_scene(oracle), per_map=False, dense=False, along=False, window=0, bound_min=False, inflate=0.0, z_max=3.0, X=None)
    s["cov"] = np.zeros((s["M"], 3 * s["N"]))
    got = _device(cilqr, solver, s, cov="null")
    mask = _zero_cov_want(s)
    assert np.array_equal(got["layer"][0] == 100.0, mask) and np.all(got["layer"][0][~mask] == 0.0)
    assert got["fields"][0].tolist() == [float(mask.sum()), 100.0, float(np.flatnonzero(mask.flatten(order="F"))[0]),
                                         got["fields"][0][MAX_ENTRY], 0.0, 0.0]
    polys = _boxes_in_map_frame(s["pose"], s["dim"], s["poses"], s["N"])
    layer = solver.rasterize_polygons(cilqr.map_geom(*s["geom"]), polys)
    assert np.array_equal(layer == 100.0, mask)


@gpu
def test_limits(cilqr, oracle, solver, cases):
    """No map set: CILQR_ERR_ARG, saying so.  B, N or M beyond the handle's: CILQR_ERR_ARG.  layer_out inside the set layer: CILQR_ERR_ARG.
    A host call beyond the arena: CILQR_ERR_ARG, and the handle stays usable.  The largest (N, M) a small handle accepts runs: the
    header's LDS formula, 8*(2*N + 20) bytes, stays below 64 KiB for every horizon up to CILQR_MAX_HORIZON, so CILQR_ERR_UNSUPPORTED is
    out of reach."""
    s = cases["t258"]
    rows, cols, N, M = s["rows"], s["cols"], s["N"], s["M"]
    sv = cilqr.Solver(_params(cilqr), max_batch=2, max_horizon=N, max_obstacles=M, device=0)
    try:
        with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*no uncertainty map" % ERR_ARG):
            sv.rasterize_tracks(N, (rows, cols), s["pose"][:2], s["dim"][:2], X=s["X"][:2])
        with _SetMap(cilqr, sv, s, [0, 1]):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: B=3 outside" % ERR_ARG):
                sv.rasterize_tracks(N, (rows, cols), s["pose"], s["dim"], X=s["X"])
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: M=%d outside" % (ERR_ARG, M + 1)):
                sv.rasterize_tracks(N, (rows, cols), np.zeros((M + 1, 4 * N)), np.ones((M + 1, 2 * N)), X=s["X"][:2])
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: N=%d outside" % (ERR_ARG, N + 1)):
                sv.rasterize_tracks(N + 1, (rows, cols), np.zeros((M, 4 * (N + 1))), np.ones((M, 2 * (N + 1))), B=2)
        got = _device(cilqr, sv, s, sel=[0, 1])
        _check_against(got, s, "2 solves on a handle of 2", sel=[0, 1])
        dev = torch.device("cuda", 0)
        lay = torch.zeros(3 * rows * cols, dtype=torch.float32, device=dev)
        z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
        X, pose, dim, fields = z(2 * 4 * (N + 1)), z(M * 4 * N), z(M * 2 * N), z(12)
        torch.cuda.synchronize(dev)
        sv.set_uncertainty_map_device(lay.data_ptr(), cilqr.map_geom(*s["geom"]), s["poses"], s["probes"], layer_stride=rows * cols)
        try:
            for off in (0, rows * cols - 1, 2 * rows * cols - 1):  # any cell of the two layers read
                with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*overlaps the layer set" % ERR_ARG):
                    sv.rasterize_tracks_device(0, 2, N, M, X.data_ptr(), pose.data_ptr(), dim.data_ptr(), (0, N, 1, 0),
                                               lay.data_ptr() + 4 * off, fields.data_ptr())
        finally:
            sv.clear_uncertainty_map()
    finally:
        sv.close()
    # a host call beyond the arena: the node's map on a handle whose arena holds 4 solves of N = 2 without obstacles' worth
    n = cases["node"]
    sv = cilqr.Solver(_params(cilqr), max_batch=4, max_horizon=n["N"], max_obstacles=n["M"], device=0)
    try:
        with _SetMap(cilqr, sv, n, [0, 1, 2]):
            with pytest.raises(cilqr.CilqrError, match="cilqr error %d: .*does not fit the device buffers" % ERR_ARG):
                sv.rasterize_tracks(n["N"], (n["rows"], n["cols"]), n["pose"], n["dim"], obs_cov=n["cov"], X=n["X"])
        _check_against(_device(cilqr, sv, n), n, "the node's map on a handle of its own sizes")
    finally:
        sv.close()
    h = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    NMAX = int(re.search(r"#define\s+CILQR_MAX_HORIZON\s+(\d+)", h).group(1))
    assert 8 * (2 * NMAX + 20) <= 64 * 1024 and "8*(2*N + 20) bytes" in h
    Mbig = 5
    big = _mk(oracle, 21, 6, 43, 0.5, NMAX, Mbig, 3, True, False, False, False, B=2)
    sv = cilqr.Solver(_params(cilqr, NMAX), max_batch=2, max_horizon=NMAX, max_obstacles=Mbig, device=0)
    try:
        _check_against(_device(cilqr, sv, big), big, "N = %d, M = %d: the largest a handle of these sizes accepts" % (NMAX, Mbig))
    finally:
        sv.close()


# ---- what it is for: one round on the CPU, from the reference pipeline alone ---------------------------------------------------------
PURPOSE_N, PURPOSE_W_UNCERTAINTY = 40, 5.0  # Parameters::w_uncertainty as in test_tighten_map's round scene
PURPOSE_GEOM, PURPOSE_POSE = (30.0, 12.0, 0.2, 15.0, 0.0), (0.0, 0.0, 0.0)
PURPOSE_INFLATE, PURPOSE_Z, PURPOSE_WINDOW = 0.2, 2.0, 2  # (z_max 2: at 3 the tail of A's last entries reaches the footprint)
TRACK_A = (20.0, -10.0, 5.0, math.pi / 2, 0.0, 0.0)  # crosses y = 0 at x = 20 after 2 s: two seconds before the ego gets there
# crosses 0.4 s after the ego arrives.  MOVED from y = -20 (crossing as the ego arrives): there CR_STEP_RISK is 1.0 before and after the
# round — min(1, .) saturates — and no direction can show; the scan of the start is in the test's docstring
TRACK_B = (20.0, -22.0, 5.0, math.pi / 2, 0.0, 0.0)


def _purpose_scene(O):
    """The ego at 5 m/s along x, two candidates side by side, no ellipse (M = 0: the live node's configuration), a zero map."""
    N, B = PURPOSE_N, 2
    p = O.default_params(N)
    p.safe_length, p.safe_width = SAFE
    p.w_uncertainty = PURPOSE_W_UNCERTAINTY
    path = np.stack([np.arange(200.0), np.zeros(200)], 1)
    x0 = np.array([[0.0, 0.0, 5.0, 0.0], [0.0, -0.4, 5.0, 0.0]])
    poly, fl = np.zeros((B, 6)), np.zeros((B, 2))
    for b in range(B):
        c, ref = O.local_plan(p, path, x0[b])
        poly[b], fl[b] = c, (ref[0, 0], ref[-1, 0])
    U0 = np.tile(O.default_control_seq(N), (B, 1))
    g = O.map_geom(*PURPOSE_GEOM)
    track = np.array([TRACK_A, TRACK_B])
    pr = predict_restate(p.timestep, N, track, np.stack([_cm(P0_T)] * 2), _cm(W_DIAG))
    pose = np.ascontiguousarray(pr["pose"].reshape(2, 4 * N))
    dim = np.ascontiguousarray(np.tile([4.0, 2.0], (2, N)))
    cov = np.ascontiguousarray(np.stack([pr["sigma"][:, :, 0, 0], pr["sigma"][:, :, 0, 1], pr["sigma"][:, :, 1, 1]], axis=-1).reshape(2, 3 * N))
    return dict(p=p, N=N, B=B, x0=x0, poly=poly, fl=fl, U0=U0, geom=PURPOSE_GEOM, g=g, poses=PURPOSE_POSE, probes=(3, 3),
                layers=np.zeros((int(g.rows), int(g.cols)), dtype=np.float32), track=track, pose=pose, dim=dim, cov=cov,
                sigma0=_cm(SIGMA0), W=_cm(W_DIAG))


def _footprint(s, X):
    """(B, rows, cols) bool: the cells whose centre lies within half the footprint's diagonal and one cell of a plan position."""
    g, N = s["g"], s["N"]
    mx = (g.pos_x + (0.5 * g.len_x - 0.5 * g.res)) - np.arange(int(g.rows)) * g.res
    my = (g.pos_y + (0.5 * g.len_y - 0.5 * g.res)) - np.arange(int(g.cols)) * g.res
    r = 0.5 * math.hypot(*SAFE) + g.res
    Xs = X.reshape(X.shape[0], N + 1, 4)[:, :N]
    d2 = (mx[None, :, None, None] - Xs[:, None, None, :, 0]) ** 2 + (my[None, None, :, None] - Xs[:, None, None, :, 1]) ** 2
    return d2.min(axis=3) <= r * r


def _judge(O, s, X, U):
    """CR_STEP_RISK of the restated cilqr_chance_risk_cov against both tracks, with the oracle's gains at the plan (no map term)."""
    B, N = s["B"], s["N"]
    _, K, ok = o_gains(O, s["p"], N, X, U, s["poly"], s["fl"])
    assert np.all(ok == 1)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[None], (B,) + a.shape))  # noqa: E731
    out = restate_cov(s["p"], N, X, U, K, s["sigma0"], s["W"], rep(s["pose"]), rep(s["dim"]), rep(s["cov"].reshape(2, N, 3)))
    return out["risk"][:, STEP_RISK], K


def _resolve(O, s, layers, U):
    um, keep = O.uncertainty_map(layers, s["g"], s["poses"], s["probes"], batched=layers.ndim == 3)
    return O.solve_batch_unc(s["p"], s["N"], 0, s["x0"], U, s["poly"], s["fl"], None, None, None, um, threads=min(8, O.max_threads()))


@pytest.fixture(scope="module")
def purpose(oracle):
    O = oracle
    s = _purpose_scene(O)
    first = _resolve(O, s, s["layers"], s["U0"])
    args = (s["inflate"] if "inflate" in s else PURPOSE_INFLATE, PURPOSE_Z)
    one = lambda m: (s["pose"][m:m + 1], s["dim"][m:m + 1], s["cov"][m:m + 1])  # noqa: E731
    along_a = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], first["X"], *one(0), *args, PURPOSE_WINDOW, False)
    swept_a = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], None, *one(0), *args, 0, False, B=s["B"])
    both = tracks_restate(s["g"], s["layers"], s["poses"], s["N"], first["X"], s["pose"], s["dim"], s["cov"], *args, PURPOSE_WINDOW, False)
    control = _resolve(O, s, s["layers"], first["U"])
    second_a = _resolve(O, s, along_a["layer"], first["U"])
    second = _resolve(O, s, both["layer"], first["U"])
    risk0, K1 = _judge(O, s, first["X"], first["U"])
    risk1, K2 = _judge(O, s, second["X"], second["U"])
    return dict(s=s, first=first, along_a=along_a, swept_a=swept_a, both=both, control=control, second_a=second_a, second=second,
                risk0=risk0, risk1=risk1, K1=K1, K2=K2)


def test_one_round_on_the_cpu_does_what_it_is_for(purpose):
    """A condition on the scene, not a measurement of the kernel: the oracle's solves plus the restatement.  The ego runs at 5 m/s along x
    (two candidates, y = 0 and -0.4), N = 40, no ellipse; tracks A and B cross x = 20 heading +y at 5 m/s, P_0 and Q of scene T.
      track A alone, along the plan, window 2: no cell under the plan's footprint is raised, and the re-solve from the plan's U equals the
      re-solve on the original map (the control) to 1e-9 and stays within the solver's tolerance of the first plan (sqrt(tolerance / w)
      per state): the planner is not disturbed by a vehicle that is gone when it gets there.  The
      swept layer of A raises cells under the footprint: the time-collapsed stripe would block the road.
      tracks A and B: B raises cells on the plan, and CR_STEP_RISK of the restated cilqr_chance_risk_cov against the tracks is lower
      after one round than before.
    Figures measured here (the direction alone is asserted), z_max 2, window 2: track A alone raises 579 cells per candidate, none under the
    footprint, and the re-solve equals the control bit for bit; its swept layer raises 131 and 129 footprint cells, up to 91.99.  With both
    tracks 1860 cells are raised, 142 and 141 under the footprint; CR_STEP_RISK 0.6099, 0.6059 before and 0.5626, 0.5595 after one round
    (7 iterations each; the plan's last x from 19.92 to 19.85: at w_uncertainty 5 the map term slows the plan a little, it does not stop
    it).  Track B's start was moved from y = -20 to -22: at -20 CR_STEP_RISK is 1.0 before and after (saturated); at -24 it is 0.2786 ->
    0.2691, at -26 0.1183 -> 0.1189 (the map there is raised to 2.6 at most and the risk is track A's), at -28 nothing is raised."""
    a = purpose
    s = a["s"]
    foot = _footprint(s, a["first"]["X"])
    own = np.broadcast_to(s["layers"], a["along_a"]["layer"].shape)
    raised_a = _bits32(a["along_a"]["layer"]) != _bits32(own)
    raised_s = _bits32(a["swept_a"]["layer"]) != _bits32(own)
    raised_b = _bits32(a["both"]["layer"]) != _bits32(own)
    dX = float(np.max(np.abs(a["second_a"]["X"] - a["control"]["X"])))
    move = float(np.max(np.abs(a["control"]["X"] - a["first"]["X"])))
    xN = lambda r: r["X"].reshape(s["B"], s["N"] + 1, 4)[:, -1, 0].tolist()  # noqa: E731
    print("track A along the plan: %s cells raised, %s under the footprint; swept: %s under the footprint, up to %.4g\n"
          "re-solve on A's layers against the control %.3g (the control moved %.3g from the first plan)\n"
          "A and B: %s cells raised, %s under the footprint; CR_STEP_RISK before %s after %s; iterations %s -> %s; x_N %s -> %s" % (
              raised_a.reshape(s["B"], -1).sum(1).tolist(), (raised_a & foot).reshape(s["B"], -1).sum(1).tolist(),
              (raised_s & foot).reshape(s["B"], -1).sum(1).tolist(), float(a["swept_a"]["layer"][foot].max()), dX, move,
              raised_b.reshape(s["B"], -1).sum(1).tolist(), (raised_b & foot).reshape(s["B"], -1).sum(1).tolist(), a["risk0"].tolist(),
              a["risk1"].tolist(), a["first"]["iters"].tolist(), a["second"]["iters"].tolist(), xN(a["first"]), xN(a["second"])))
    assert not a["along_a"]["border"].any() and not a["both"]["border"].any()
    assert np.all(raised_a.reshape(s["B"], -1).sum(1) > 0) and not (raised_a & foot).any()
    assert dX <= 1e-9
    # ... and within the solver's tolerance of the first plan.  The solver stops when an iteration changes J by less than
    # Parameters::tolerance; a state that is off by delta costs w*delta^2 or more in J, so the solver does not resolve a position below
    # sqrt(tolerance / w_pos) or a speed below sqrt(tolerance / w_vel): 0.0124 m and 0.0058 m/s at the defaults (the heading carries no
    # weight of its own).  Measured: 0.00917 m and 0.0040 m/s, the control's own distance from the first plan.
    p = s["p"]
    gone = np.abs(a["second_a"]["X"] - a["first"]["X"]).reshape(s["B"], s["N"] + 1, 4)
    print("re-solve on A's layers against the first plan: position %.3g (bound %.3g), speed %.3g (bound %.3g)" % (
        gone[:, :, :2].max(), math.sqrt(p.tolerance / p.w_pos), gone[:, :, 2].max(), math.sqrt(p.tolerance / p.w_vel)))
    assert gone[:, :, :2].max() <= math.sqrt(p.tolerance / p.w_pos) and gone[:, :, 2].max() <= math.sqrt(p.tolerance / p.w_vel)
    assert np.all((raised_s & foot).reshape(s["B"], -1).sum(1) > 0) and float(a["swept_a"]["layer"][foot].max()) > 50.0
    assert np.all((raised_b & foot).reshape(s["B"], -1).sum(1) > 0)
    assert np.all(a["risk0"] > 0.01) and np.all(a["risk1"] < a["risk0"])


@gpu
def test_pipeline_on_device_buffers(cilqr, purpose):
    """predict -> solve with the map set -> rasterise along the plans -> the per-solve layers set -> re-solve from the plan's U ->
    cilqr_chance_risk_cov against the tracks, every call in its device form on one stream (the gains with the map cleared for that call
    alone: the oracle's backward pass has no map term).  Against the purpose test's CPU figures at the suite's tolerances: iterations
    and exits equal, max|dU| <= 1e-8 after the warm-started second solve, CR_STEP_RISK before and after within 1e-9, the same strict
    decrease; the rasterised layers within 1 ulp of the restated ones (the plan they follow is the device's, 1e-9 from the oracle's)."""
    a = purpose
    s = a["s"]
    B, N, M, g = s["B"], s["N"], 2, s["g"]
    rows, cols = int(g.rows), int(g.cols)
    cells = rows * cols
    geom = cilqr.map_geom(*s["geom"])
    p = _params(cilqr, N)
    p.w_uncertainty = PURPOSE_W_UNCERTAINTY
    solver = cilqr.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
        zi = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        ptr = lambda t: t.data_ptr()  # noqa: E731
        x0, U, poly, fl, s0, W = (up(v) for v in (s["x0"], s["U0"], s["poly"], s["fl"], s["sigma0"], s["W"]))
        track, tdim, tcov = up(s["track"]), up(np.tile([4.0, 2.0], (M, 1))), up(np.stack([_cm(P0_T)] * M))
        pose, dim, cov = z(M, 4 * N), z(M, 2 * N), z(M, 3 * N)
        layer = torch.zeros(cells, dtype=torch.float32, device=dev)
        raster = torch.zeros((B, cells), dtype=torch.float32, device=dev)
        X, J, it, ex = z(B, 4 * (N + 1)), z(B), zi(B), zi(B)
        X2, J2, it2, ex2 = z(B, 4 * (N + 1)), z(B), zi(B), zi(B)
        k, K, ok, k2, K2, ok2 = z(B, 2 * N), z(B, 8 * N), zi(B), z(B, 2 * N), z(B, 8 * N), zi(B)
        risk, risk2, fields = z(B, 6), z(B, 6), z(B, 6)
        none, shared = (0, 0, 0, 0), (0, N, 1, 0)
        original = lambda: solver.set_uncertainty_map_device(ptr(layer), geom, s["poses"], s["probes"])  # noqa: E731
        torch.cuda.synchronize(dev)
        solver.predict_obstacles_device(st, 1, N, M, ptr(track), ptr(tdim), ptr(pose), ptr(dim), track_cov=ptr(tcov), track_noise=ptr(W),
                                        cov_out=ptr(cov))
        original()
        solver.solve_batch_device(st, B, N, 0, ptr(x0), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, ptr(X), ptr(J), ptr(it), ptr(ex))
        U1 = U.clone()
        solver.clear_uncertainty_map()
        solver.gains_batch_device(st, B, N, 0, ptr(X), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, none, ptr(k), ptr(K), ptr(ok))
        solver.chance_risk_cov_device(st, B, N, M, ptr(X), ptr(U), ptr(K), ptr(s0), 0, ptr(W), ptr(pose), ptr(dim), shared, ptr(cov), ptr(risk))
        original()
        solver.rasterize_tracks_device(st, B, N, M, ptr(X), ptr(pose), ptr(dim), shared, ptr(raster), ptr(fields), obs_cov=ptr(cov),
                                       inflate=PURPOSE_INFLATE, z_max=PURPOSE_Z, window=PURPOSE_WINDOW)
        solver.set_uncertainty_map_device(ptr(raster), geom, s["poses"], s["probes"], layer_stride=cells)
        solver.solve_batch_device(st, B, N, 0, ptr(x0), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, ptr(X2), ptr(J2), ptr(it2), ptr(ex2))
        solver.clear_uncertainty_map()
        solver.gains_batch_device(st, B, N, 0, ptr(X2), ptr(U), ptr(poly), ptr(fl), 0, 0, 0, none, ptr(k2), ptr(K2), ptr(ok2))
        solver.chance_risk_cov_device(st, B, N, M, ptr(X2), ptr(U), ptr(K2), ptr(s0), 0, ptr(W), ptr(pose), ptr(dim), shared, ptr(cov), ptr(risk2))
        torch.cuda.synchronize(dev)
    finally:
        solver.close()
    n = lambda t: t.cpu().numpy()  # noqa: E731
    d1, d2 = float(np.max(np.abs(n(U1) - a["first"]["U"]))), float(np.max(np.abs(n(U) - a["second"]["U"])))
    r0, r1 = n(risk)[:, STEP_RISK], n(risk2)[:, STEP_RISK]
    got = _layers_of(n(raster), rows, cols)
    want = a["both"]
    both_up = (got > 0) & (want["layer"] > 0)
    far = np.zeros(got.shape, dtype=bool)
    far[both_up] = _ulp32(got[both_up], want["layer"][both_up]) > 1
    differ = far | ((got > 0) != (want["layer"] > 0))
    print("first solve max|dU| %.3g, iterations %s; after the round max|dU| %.3g, iterations %s (oracle %s); %d of %d rasterised cells more "
          "than 1 ulp from the restated ones\nCR_STEP_RISK before %s (CPU %s)\n             after  %s (CPU %s); fields %s" % (
              d1, n(it).tolist(), d2, n(it2).tolist(), a["second"]["iters"].tolist(), differ.sum(), differ.size, r0.tolist(), a["risk0"].tolist(),
              r1.tolist(), a["risk1"].tolist(), n(fields).tolist()))
    assert np.max(np.abs(n(pose).reshape(M, N, 4) - predict_restate(s["p"].timestep, N, s["track"], np.stack([_cm(P0_T)] * M), s["W"])["pose"])) <= 1e-9
    assert np.array_equal(n(it), a["first"]["iters"]) and np.array_equal(n(ex), a["first"]["status"]) and np.all(n(ok) == 1)
    # (the plan the device rasterises along is 1e-9 from the oracle's: a cell may differ where the restatement is borderline at THAT width)
    assert differ.sum() <= 0.001 * differ.size
    assert np.array_equal(n(fields)[:, [LOST_ENTRIES, LOST_STEPS]], want["fields"][:, [LOST_ENTRIES, LOST_STEPS]])
    assert np.max(np.abs(n(fields)[:, RAISED] - want["fields"][:, RAISED])) <= 0.001 * cells
    assert np.array_equal(n(it2), a["second"]["iters"]) and np.array_equal(n(ex2), a["second"]["status"]) and np.all(n(ok2) == 1)
    assert d2 <= 1e-8
    assert np.max(np.abs(r0 - a["risk0"])) <= 1e-9 and np.max(np.abs(r1 - a["risk1"])) <= 1e-9
    assert np.all(r1 < r0)


@gpu
def test_cpp_facade_track_map_candidates(oracle, purpose, tmp_path):
    """tests/cpp/candidates_track_map.cpp: run_candidates and run_step under iLQR::set_track_map against the C-ABI sequence called by hand,
    bit for bit, with the ellipses off and on (inside the program: picks, last_track_map, the map on the handle afterwards, the off
    switches, the round composed with set_map_tightening, the covariance check behind the map-only plan, the conflicts), and against the restated pipeline for the candidates it solved with the ellipses off (here): the
    rasterised layers, the re-solved plans within 1e-8, the iteration counts, the pick."""
    O = oracle
    exe, dump = str(tmp_path / "candidates_track_map"), str(tmp_path / "dump.txt")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_track_map.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe, dump], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("ellipses off ok", "ellipses on ok", "map restored ok", "run_step ok", "off switches ok", "composed with map tightening ok",
                 "judged behind the map ok", "conflicts throw ok"):
        assert line in r.stdout, r.stdout
    v = open(dump).read().split()
    B, N, rows, cols, best = (int(x) for x in v[:5])
    a = np.array([float(x) for x in v[5:]])
    take = lambda n, at=[0]: (a[at[0]:at[0] + n], at.__setitem__(0, at[0] + n))[0]  # noqa: E731
    X1, U1 = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1)
    X2, U2, J2, fields = take(B * 4 * (N + 1)).reshape(B, -1), take(B * 2 * N).reshape(B, -1), take(B), take(B * 6).reshape(B, 6)
    iters = take(B).astype(np.int32)
    layers = take(B * rows * cols).astype(np.float32).reshape(B, cols, rows).transpose(0, 2, 1)
    s = purpose["s"]
    assert (B, N, rows, cols) == (s["B"], s["N"], int(s["g"].rows), int(s["g"].cols))
    # the restated pipeline from the first plans the program solved
    want = tracks_restate(s["g"], s["layers"], s["poses"], N, np.ascontiguousarray(X1), s["pose"], s["dim"], s["cov"], PURPOSE_INFLATE, PURPOSE_Z,
                          PURPOSE_WINDOW, False)
    second = _resolve(O, s, want["layer"], np.ascontiguousarray(U1))
    both_up = (layers > 0) & (want["layer"] > 0)
    far = np.zeros(layers.shape, dtype=bool)
    far[both_up] = _ulp32(layers[both_up], want["layer"][both_up]) > 1
    differ = far | ((layers > 0) != (want["layer"] > 0))
    dU = float(np.max(np.abs(U2 - second["U"])))
    print("rasterised cells more than 1 ulp from the restated ones %d of %d; max|dU| %.3g; iterations %s (oracle %s); J %s (oracle %s)" % (
        differ.sum(), differ.size, dU, iters.tolist(), second["iters"].tolist(), J2.tolist(), second["J"].tolist()))
    # (the tracks the program rasterises are the device's prediction, 1e-9 from the restated one)
    assert differ.sum() <= 0.001 * differ.size
    assert np.array_equal(fields[:, [LOST_ENTRIES, LOST_STEPS]], want["fields"][:, [LOST_ENTRIES, LOST_STEPS]])
    assert np.max(np.abs(fields[:, RAISED] - want["fields"][:, RAISED])) <= 0.001 * rows * cols
    assert np.array_equal(iters, second["iters"]) and dU <= 1e-8
    gaps = np.diff(np.sort(second["J"]))
    assert gaps.min() > 1e-6 and best == int(np.argmin(second["J"]))  # the pick is decided, and it is the restated pipeline's
