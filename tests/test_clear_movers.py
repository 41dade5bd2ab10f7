"""cilqr_clear_movers(_device): the static layer — the cells of tracked movers taken out of the map (csrc/costmap_movers.hip).

Expected values never come from the HIP path.  `owners_brute` below is the definition of include/cilqr.h by brute force over all
linked cells: per cell the lexicographic minimum of (squared distance, label) over the window.  `restate` puts the mover test, the
fill rule and the eight fields on top of it.  test_conditions checks the restatement on the CPU against the separable evaluation
(best (|di|, label) per column, then (di^2 + dj^2, label) over the columns) and, where no two labels tie, against
scipy.ndimage.distance_transform_edt(return_indices=True).

No tolerance exists in this feature: layers compare as uint32 views, owner_out and the fields exactly.  The one real-valued decision,
hypot(VX, VY) >= v_clear, is drawn with a margin of MARGIN = 1e-6 (asserted), nineteen orders above hypot's rounding.

The crossing scene (test_scene_conditions, test_device_chain_*): a 150 x 100 map at 0.1 m centred at (12, 0); a standing 8 x 8-cell
block at [2:10, 1:9]; a 9 x 20-cell block at [90:99, 15 + 5k : 35 + 5k] for the ticks k = 0 ... 5 with a two-cell ring of value 30
around it; seeds above 50, make_filter() defaults of tests/test_track_update.py.  After tick 5 the crossing block is row 1, label
6090, slot 1, 6 hits, 5.0025 m/s at (10.05, 0.0004).  With halo2 = 9 the rule clears 312 cells (180 linked + 132 ring), with
halo2 = 0 the 180 (190 halo cells are owned at halo2 = 9; the 58 beyond the ring hold 0 and do not change).  Four straight candidates at 5 m/s on y = 0, -0.8, -1.6, -2.4 (N = 30, base costs 1 ... 4): on the ORIGINAL layer
cilqr_footprint_check rejects candidates 0, 1 and 2 and the pick is 3; on the cleared layer with the predicted track table as the
check's obstacles every candidate passes and the pick is 0.  That is the scene of the issue, unmoved: the footprint restatement of
tests/test_footprint.py decides both picks with its EDGE margin (test_scene_conditions).
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
from test_map_obstacles import NONE, components_restate, d2_of, flood_labels, rows_restate
from test_track_update import (CHAIN_COLS, CHAIN_K, CHAIN_N, CHAIN_POS, CHAIN_RES, CHAIN_ROWS, CHAIN_TICKS, CHAIN_YS, DET, HITS, ID, MARGIN, STATE,
                               VX, VY, WORLD_FIELDS, _margins, c_filter, check_world, free_table, make_filter, new_diag, tick_restate)

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
FIELDS = 8
MOVERS, CLEARED, OWNED_LINKED, OWNED_HALO, MAX_VALUE, MAX_CELL, CONTESTED, KEPT_UNKNOWN = range(FIELDS)
MAX_HALO2 = 1024
MO_FIELDS, MO_LABEL = 13, 0
ENTRY_POINTS = ("cilqr_clear_movers", "cilqr_clear_movers_device")
SHAPES = [(1, 1), (1, 7), (7, 1), (65, 17), (150, 100)]
HALOS = [0, 2, 9, 13, 1024]  # r = 0, 1, 3, 3 (a halo2 that is no square), 32
SENTINEL = -123.25

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def isqrt(h):
    return int(math.isqrt(int(h)))


# ---- the definition, restated -------------------------------------------------------------------------------------------------------
BIG = 1 << 40


def owners_brute(label, halo2, only=None):
    """label (rows, cols) int32.  Every linked cell (of the labels in `only`, if given) offers (d2, label) to the cells of its window;
    the lexicographic minimum stays.  Returns (owner (rows, cols) int64: -1 where none or beyond halo2; d2 (rows, cols): BIG where
    none; tie (rows, cols) bool: another label stood at the winning distance)."""
    rows, cols = label.shape
    r = isqrt(halo2)
    best_d = np.full((rows, cols), BIG, dtype=np.int64)
    best_l = np.full((rows, cols), BIG, dtype=np.int64)
    tie = np.zeros((rows, cols), dtype=bool)
    ii, jj = np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64)
    linked = label >= 0
    if only is not None:
        linked = linked & np.isin(label, np.asarray(sorted(only), dtype=np.int64))
    for qi, qj in zip(*np.nonzero(linked)):
        i0, i1, j0, j1 = max(0, qi - r), min(rows, qi + r + 1), max(0, qj - r), min(cols, qj + r + 1)
        d = ((ii[i0:i1] - qi) ** 2)[:, None] + ((jj[j0:j1] - qj) ** 2)[None, :]
        lb = int(label[qi, qj])
        wd, wl, wt = best_d[i0:i1, j0:j1], best_l[i0:i1, j0:j1], tie[i0:i1, j0:j1]
        closer = d < wd
        same = (d == wd) & (wl != lb)
        wt[closer] = False
        wt[same] = True
        take = closer | ((d == wd) & (lb < wl))
        wd[take] = d[take]
        wl[take] = lb
    owner = np.where(best_d <= halo2, best_l, -1)
    return owner, best_d, tie


def owners_separable(label, halo2):
    """The same owner by the two passes the header allows: per (i, column) the best (|di|, label), then over the columns."""
    rows, cols = label.shape
    r = isqrt(halo2)
    NO = 1 << 30
    adi = np.full((rows, cols), NO, dtype=np.int64)
    lab = np.full((rows, cols), NO, dtype=np.int64)
    L = np.where(label >= 0, label.astype(np.int64), NO)
    for di in range(-r, r + 1):
        sh = np.full((rows, cols), NO, dtype=np.int64)
        lo, hi = max(0, -di), min(rows, rows - di)
        if lo < hi:
            sh[lo:hi] = L[lo + di:hi + di]
        a = np.where(sh < NO, abs(di), NO)
        take = (a < adi) | ((a == adi) & (sh < lab))
        adi, lab = np.where(take, a, adi), np.where(take, sh, lab)
    best_d = np.full((rows, cols), BIG, dtype=np.int64)
    best_l = np.full((rows, cols), BIG, dtype=np.int64)
    for dj in range(-r, r + 1):
        a, l2 = np.full((rows, cols), NO, dtype=np.int64), np.full((rows, cols), NO, dtype=np.int64)
        lo, hi = max(0, -dj), min(cols, cols - dj)
        if lo < hi:
            a[:, lo:hi], l2[:, lo:hi] = adi[:, lo + dj:hi + dj], lab[:, lo + dj:hi + dj]
        d = np.where(a < NO, a * a + dj * dj, BIG)
        take = (d < best_d) | ((d == best_d) & (d < BIG) & (l2 < best_l))
        best_d, best_l = np.where(take, d, best_d), np.where(take, l2, best_l)
    return np.where(best_d <= halo2, best_l, -1)


def tracker_movers(comp_label, assign, state, min_hits, v_clear, margins=None):
    """The tracker form's rule for one layer: comp_label (K,), assign (K,), state (M, 32) -> (K,) bool."""
    K, M = comp_label.shape[0], state.shape[0]
    out = np.zeros(K, dtype=bool)
    for k in range(K):
        m = int(assign[k])
        if not (comp_label[k] >= 0) or m < 0 or m >= M:
            continue
        s = state[m]
        if not (s[ID] >= 0) or s[DET] != k or not (s[HITS] >= min_hits):
            continue
        v = math.hypot(s[VX], s[VY])
        if margins is not None and v == v:
            margins.append(abs(v - v_clear))
        out[k] = v >= v_clear
    return out


def restate(layer, label, comp_label, movers, halo2, fill):
    """One layer.  layer (rows, cols) float32, label (rows, cols) int32, comp_label (K,) doubles, movers (K,) bool.  Returns
    dict(layer, owner (int32), fields (8,))."""
    rows, cols = label.shape
    mover_labels = sorted({int(comp_label[k]) for k in range(len(comp_label)) if movers[k] and comp_label[k] >= 0})
    owner, _, _ = owners_brute(label, halo2)
    _, mover_d2, _ = owners_brute(label, halo2, only=mover_labels)
    linked = label >= 0
    owned = (owner >= 0) & np.isin(owner, np.asarray(mover_labels, dtype=np.int64))
    nan = np.isnan(layer)
    out = layer.copy()
    out[owned & ~nan] = np.float32(fill)
    f = np.zeros(FIELDS)
    f[MOVERS] = int(np.count_nonzero(np.asarray(movers) & (np.asarray(comp_label) >= 0)))
    f[CLEARED] = int(np.count_nonzero(_u32(out) != _u32(layer)))
    f[OWNED_LINKED], f[OWNED_HALO] = int((owned & linked).sum()), int((owned & ~linked).sum())
    f[CONTESTED] = int((~linked & (mover_d2 <= halo2) & ~owned).sum())
    f[KEPT_UNKNOWN] = int((owned & nan).sum())
    f[MAX_VALUE], f[MAX_CELL] = -1.0, -1.0
    fin = owned & np.isfinite(layer)
    if fin.any():
        top = float(layer[fin].max())
        ci, cj = np.nonzero(fin & (layer == np.float32(top)))
        f[MAX_VALUE], f[MAX_CELL] = top + 0.0, int(np.min(ci + cj * rows))
    return dict(layer=out, owner=owner.astype(np.int32), fields=f)


# ---- random layers --------------------------------------------------------------------------------------------------------------------
def blob_layer(rows, cols, seed, K, drop_share=0.25):
    """Seeded blobs labelled by flood_labels; values 0 ... 100 with a few NaN, -0, +inf and negative cells; comp rows for the first
    K components that are not dropped (a dropped one keeps its label in the layer and gets no row), filler behind; a random mask."""
    rng = np.random.Generator(np.random.PCG64(seed))
    linked = np.zeros((rows, cols), dtype=bool)
    n_blobs = max(1, rows * cols // 40)
    for _ in range(n_blobs):
        ci, cj, a, b = rng.integers(0, rows), rng.integers(0, cols), rng.integers(1, 5), rng.integers(1, 5)
        linked[max(0, ci - a // 2):ci + a, max(0, cj - b // 2):cj + b] = True
    linked &= rng.random((rows, cols)) < 0.9
    if rows * cols == 1:
        linked[:] = True
    label = flood_labels(linked, 0)
    layer = np.where(linked, 100.0, np.rint(rng.random((rows, cols)) * 60.0)).astype(np.float32)
    layer[rng.random((rows, cols)) < 0.05] = np.nan
    layer[rng.random((rows, cols)) < 0.02] = -0.0
    layer[rng.random((rows, cols)) < 0.01] = np.inf
    layer[rng.random((rows, cols)) < 0.01] = -3.5
    roots = np.unique(label[label >= 0])
    kept = roots[rng.random(roots.size) >= drop_share][:K]
    comp = np.full((K, MO_FIELDS), -1.0)
    comp[:kept.size, MO_LABEL] = kept
    comp[:kept.size, 1:] = 7.0  # (not read)
    mask = (rng.random(K) < 0.5).astype(np.int32) * rng.integers(1, 1 << 20, K).astype(np.int32)
    return dict(layer=layer, label=label, comp=comp, mask=mask, rng=rng)


V_CLEAR = 1.5


def tracker_rows(comp, M, min_hits, rng):
    """assign (K,) and state (M, 32) with every edge of the tracker form among the rows: assign -1, -2 and beyond M, a free slot, DET
    of another row, HITS one below and at min_hits, speeds MARGIN below and above V_CLEAR, a NaN VX."""
    K = comp.shape[0]
    assign = np.full(K, -2, dtype=np.int32)
    state = free_table(M)
    slots = rng.permutation(M)
    for n, k in enumerate(rng.permutation(K)):
        if n >= M:
            assign[k] = [-1, -2, M, M + 5][n % 4]
            continue
        m = int(slots[n])
        kind = n % 9
        assign[k] = m
        th = rng.random() * 6.0
        v = V_CLEAR + [MARGIN, -MARGIN, 2.0, -1.0, 0.5, 3.0, 1.0, 0.25, 2.5][kind]
        state[m, VX], state[m, VY] = v * math.cos(th), v * math.sin(th)
        state[m, ID], state[m, DET], state[m, HITS] = float(n), float(k), float(min_hits)
        if kind == 4:
            state[m, HITS] = float(min_hits - 1)
        if kind == 5:
            state[m, DET] = float((k + 1) % max(K, 2))
        if kind == 6:
            state[m, ID] = -1.0
        if kind == 7:
            state[m, VX] = np.nan
        if kind == 8:
            assign[k] = -1
    return assign, state


def make_case(rows, cols, halo2, L, K, M, form, seed, fill=0.0, min_hits=2):
    layers = [blob_layer(rows, cols, seed + 17 * l, K) for l in range(L)]
    case = dict(rows=rows, cols=cols, halo2=halo2, L=L, K=K, M=M, form=form, fill=fill, min_hits=min_hits,
                layer=np.stack([b["layer"] for b in layers]), label=np.stack([b["label"] for b in layers]),
                comp=np.stack([b["comp"] for b in layers]), margins=[])
    if form == "mask":
        case["mask"] = np.stack([b["mask"] for b in layers])
        movers = [case["mask"][l] != 0 for l in range(L)]
    else:
        pairs = [tracker_rows(b["comp"], M, min_hits, b["rng"]) for b in layers]
        case["assign"], case["state"] = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        movers = [tracker_movers(case["comp"][l][:, MO_LABEL], case["assign"][l], case["state"][l], min_hits, V_CLEAR, case["margins"]) for l in range(L)]
    case["movers"] = movers
    case["want"] = [restate(case["layer"][l], case["label"][l], case["comp"][l][:, MO_LABEL], movers[l], halo2, fill) for l in range(L)]
    return case


def shape_case(shape, halo2):
    """The case of a (shape, halo2) pair: L, K, M and the form walk through their values with the pair's index."""
    n = SHAPES.index(shape) * len(HALOS) + HALOS.index(halo2)
    K, M, L = (1, 8, 64)[n % 3], (1, 64)[(n // 3) % 2], (1, 3)[n % 2]
    return make_case(shape[0], shape[1], halo2, L, K, M, ("tracker", "mask")[(n // 2) % 2], 9000 + n)


@pytest.fixture(scope="module")
def cases():
    """Every (shape, halo2) case with its restated results, computed once and left unchanged."""
    return {(s, h): shape_case(s, h) for s in SHAPES for h in HALOS}


# ---- the crossing scene -----------------------------------------------------------------------------------------------------------------
SCENE_V_CLEAR, SCENE_HALO2 = 1.0, 9
SCENE_BASE = np.array([1.0, 2.0, 3.0, 4.0])
SCENE_THRESHOLD = 50.0


def scene_layers():
    layers = np.zeros((CHAIN_TICKS, CHAIN_ROWS, CHAIN_COLS), dtype=np.float32)
    for k in range(CHAIN_TICKS):
        layers[k, 88:101, 13 + 5 * k:37 + 5 * k] = 30.0
        layers[k, 90:99, 15 + 5 * k:35 + 5 * k] = 100.0
        layers[k, 2:10, 1:9] = 100.0
    return layers


class _Geom:
    def __init__(self):
        self.rows, self.cols, self.res = CHAIN_ROWS, CHAIN_COLS, CHAIN_RES
        self.len_x, self.len_y, self.pos_x, self.pos_y = CHAIN_ROWS * CHAIN_RES, CHAIN_COLS * CHAIN_RES, CHAIN_POS[0], CHAIN_POS[1]


def scene_restate(p):
    """Map -> distance -> obstacles -> tracker -> clear_movers per tick on the restatements, as chain_restate of
    tests/test_track_update.py runs the first three; then the footprint check of the four candidates on the original layer without
    obstacles and on the cleared layer with the predicted track table."""
    from test_footprint import restate as footprint_restate
    from test_predict_obstacles import predict_restate
    from test_rollout_risk import _pick
    N, B, K = CHAIN_N, len(CHAIN_YS), CHAIN_K
    layers = scene_layers()
    x_first, y_first = CHAIN_POS[0] + (0.5 * CHAIN_ROWS * CHAIN_RES - 0.5 * CHAIN_RES), CHAIN_POS[1] + (0.5 * CHAIN_COLS * CHAIN_RES - 0.5 * CHAIN_RES)
    f = make_filter()
    state, world, ticks, rows, cleared = free_table(K), np.zeros(WORLD_FIELDS), [], [], []
    diag, margins = new_diag(), []
    for k in range(CHAIN_TICKS):
        seed = layers[k] > SCENE_THRESHOLD
        d2 = d2_of(seed)
        lab = flood_labels((d2 != NONE) & (d2 <= 0), 0)
        comp, boxes, _ = components_restate(d2, lab, CHAIN_RES, x_first, y_first, (0.0, 0.0, 0.0), 0.0)
        r = rows_restate(comp, boxes, int(seed.sum()), K, 1, math.inf)
        rows.append(dict(r, d2=d2, label=lab))
        t = tick_restate(f, state, world, r["boxes"], n=int(r["n"][2]), reset=(k == 0), diag=diag)
        state, world = t["state"], t["world"]
        ticks.append(t)
        mv = tracker_movers(r["comp"][:, MO_LABEL], t["assign"], t["state"], f["min_hits"], SCENE_V_CLEAR, margins)
        cleared.append({h: restate(layers[k], lab, r["comp"][:, MO_LABEL], mv, h, 0.0) for h in (SCENE_HALO2, 0)})
        cleared[-1]["movers"] = mv
    last = ticks[-1]
    X = np.zeros((B, N + 1, 4))
    X[:, :, 0], X[:, :, 2] = 5.0 * p.timestep * np.arange(N + 1), 5.0
    for b, y in enumerate(CHAIN_YS):
        X[b, :, 1] = y
    X = X.reshape(B, -1)
    cov16 = np.stack([c.T.reshape(16) for c in last["cov"]])
    pr = predict_restate(p.timestep, N, last["track"][None], cov16[None], None)
    pose = np.ascontiguousarray(np.broadcast_to(pr["pose"].reshape(1, K, 4 * N), (B, K, 4 * N)))
    dim = np.ascontiguousarray(np.broadcast_to(np.repeat(last["dim"][:, None, :], N, axis=1).reshape(1, K, 2 * N), (B, K, 2 * N)))
    g = _Geom()
    judge = {}
    for name, layer, po, dm in (("original", layers[-1], None, None), ("cleared", cleared[-1][SCENE_HALO2]["layer"], pose, dim)):
        judge[name] = footprint_restate(p, N, X, pose=po, dim=dm, threshold=SCENE_THRESHOLD, umap=dict(g=g, layers=layer, poses=(0.0, 0.0, 0.0)),
                                        base=SCENE_BASE)
    picks = {n: _pick(j["total"]) for n, j in judge.items()}
    return dict(p=p, layers=layers, f=f, rows=rows, ticks=ticks, diag=diag, margins=margins, cleared=cleared, X=X, pred=pr, pose=pose, dim=dim,
                judge=judge, picks=picks)


@pytest.fixture(scope="module")
def scene(cilqr):
    return scene_restate(cilqr.default_params(CHAIN_N))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    for name in ("clear_movers", "clear_movers_device"):
        assert callable(getattr(cilqr.Solver, name)), name
    block = re.search(r"typedef enum cilqr_clear_movers_field \{(.*?)\}", h, flags=re.S).group(1)  # (the chance-map fields share the prefix)
    enum = {k: int(v) for k, v in re.findall(r"\bCILQR_(CM_[A-Z_]+)\s*=\s*(\d+)", block)}
    mine = dict(CM_MOVERS=MOVERS, CM_CLEARED=CLEARED, CM_OWNED_LINKED=OWNED_LINKED, CM_OWNED_HALO=OWNED_HALO, CM_MAX_VALUE=MAX_VALUE,
                CM_MAX_CELL=MAX_CELL, CM_CONTESTED=CONTESTED, CM_KEPT_UNKNOWN=KEPT_UNKNOWN)
    assert enum == mine
    for k, v in mine.items():
        assert getattr(cilqr, k) == v, k
    defs = dict(re.findall(r"#define\s+CILQR_(CLEAR_MOVERS_[A-Z0-9_]+)\s+(\w+)", h))
    assert defs == dict(CLEAR_MOVERS_MAX_HALO2="1024", CLEAR_MOVERS_FIELDS="8")
    assert (cilqr.CLEAR_MOVERS_FIELDS, cilqr.CLEAR_MOVERS_MAX_HALO2) == (FIELDS, MAX_HALO2)
    # the header says what the call leaves out
    for phrase in ("merged with a wall", "beyond halo2 stays", "must come back through the tracks"):
        assert phrase in full, phrase
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_clear_movers\s*\(", plan)
    assert "plan_clear_movers(" in open(os.path.join(PKG, "csrc", "cilqr_api.cpp")).read()
    assert "launch_clear_movers" in open(os.path.join(PKG, "csrc", "cilqr_internal.h")).read()
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/costmap_movers.hip" in mk and re.search(r"^check:.*build/costmap_movers\.o", mk, flags=re.M)
    assert re.search(r"check_kernel_resources\.py --map .*build/costmap_movers\.o", mk)
    assert os.path.exists(os.path.join(PKG, "csrc", "costmap_movers.hpp"))


def test_argument_errors_need_no_device(cilqr):
    """Every argument error of the header without a handle; valid arguments then meet the null handle."""
    Lb = cilqr.lib()
    L, rows, cols, K, M = 2, 5, 4, 3, 2
    cells = rows * cols
    layer, out = np.zeros((L, cells), dtype=np.float32), np.zeros((L, cells), dtype=np.float32)
    label, owner = np.zeros((L, cells), dtype=np.int32), np.zeros((L, cells), dtype=np.int32)
    comp, fields = np.zeros((L, K, MO_FIELDS)), np.zeros((L, FIELDS))
    assign, mask, state = np.zeros((L, K), dtype=np.int32), np.zeros((L, K), dtype=np.int32), np.zeros((L, M, STATE))
    no_handle = C.c_void_p()

    def geom(r=rows, c=cols, res=0.1):
        g = cilqr.MapGeom()
        g.rows, g.cols, g.res, g.len_x, g.len_y, g.pos_x, g.pos_y = r, c, res, r * res, c * res, 0.0, 0.0
        return g

    def call(dev, L_=L, K_=K, M_=M, g=True, stride=cells, min_hits=1, v_clear=0.0, halo2=9, fill=0.0, form="tracker", out_=None, **nulls):
        a = dict(layer=layer, label=label, comp=comp, layer_out=out if out_ is None else out_, fields=fields,
                 assign=assign if form in ("tracker", "both", "assign") else None, state=state if form in ("tracker", "both", "state") else None,
                 mask=mask if form in ("mask", "both") else None)
        a.update(nulls)
        gg = (geom() if g is True else g)
        fn = Lb.cilqr_clear_movers_device if dev else Lb.cilqr_clear_movers
        head = (no_handle, None) if dev else (no_handle,)
        return fn(*head, L_, _p(a["layer"], _fp), C.c_int64(stride), C.byref(gg) if gg is not None else None, _p(a["label"], _ip), K_, _p(a["comp"]),
                  M_, _p(a["assign"], _ip), _p(a["state"]), min_hits, C.c_double(v_clear), _p(a["mask"], _ip), halo2, C.c_float(fill),
                  _p(a["layer_out"], _fp), _p(owner, _ip), _p(a["fields"]))

    nan, inf = float("nan"), float("inf")
    for dev in (False, True):
        err = Lb.cilqr_last_error
        for name in ("layer", "label", "comp", "layer_out", "fields"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null" in err(), name
        assert call(dev, g=None) == ERR_ARG and b"null" in err()
        for kw in (dict(L_=0), dict(L_=-2), dict(g=geom(0, 4)), dict(g=geom(5, 0)), dict(g=geom(res=0.0)), dict(g=geom(res=nan)),
                   dict(stride=-1), dict(stride=cells - 1), dict(stride=(1 << 40) + 1)):
            assert call(dev, **kw) == ERR_ARG and b"cilqr_clear_movers" in err(), kw
        for k in (0, -1, 1025):
            assert call(dev, K_=k) == ERR_ARG and b"K = " in err(), k
        for form in ("both", "neither", "assign", "state"):
            assert call(dev, form=form) == ERR_ARG and b"exactly one" in err(), form
        for m in (0, -1, 65):
            assert call(dev, M_=m) == ERR_ARG and b"M = " in err(), m
        assert call(dev, M_=0, form="mask") == ERR_ARG and b"null handle" in err()  # the mask form reads no M
        assert call(dev, min_hits=0) == ERR_ARG and b"min_hits" in err()
        assert call(dev, min_hits=0, v_clear=-1.0, form="mask") == ERR_ARG and b"null handle" in err()
        for v in (-1e-9, nan):
            assert call(dev, v_clear=v) == ERR_ARG and b"v_clear" in err(), v
        for h2 in (-1, 1025):
            assert call(dev, halo2=h2) == ERR_ARG and b"halo2" in err(), h2
        for f in (inf, -inf):
            assert call(dev, fill=f) == ERR_ARG and b"fill is infinite" in err(), f
        for kw in (dict(fill=nan), dict(halo2=0), dict(halo2=1024), dict(K_=1024, form="mask", comp=np.zeros((L, 1024, MO_FIELDS)),
                                                                             mask=np.zeros((L, 1024), dtype=np.int32)),
                   dict(M_=64, state=np.zeros((L, 64, STATE))), dict(v_clear=inf), dict(stride=0), dict(form="mask")):
            assert call(dev, **kw) == ERR_ARG and b"null handle" in err(), kw
        assert call(dev, g=geom(1025, 4), layer=np.zeros((L, 1025 * 4), dtype=np.float32), stride=1025 * 4) == ERR_UNSUPPORTED and b"1024" in err()
        assert call(dev, g=geom(4, 1025), layer=np.zeros((L, 1025 * 4), dtype=np.float32), stride=1025 * 4) == ERR_UNSUPPORTED
        assert call(dev) == ERR_ARG and b"null handle" in err()  # valid arguments, no handle
    # the overlap rule of cilqr_inflate_map, device form: the same layers in place are fine, anything else that overlaps is not
    big = np.zeros(4 * cells, dtype=np.float32)
    err = Lb.cilqr_last_error
    assert call(True, layer=big, out_=big) == ERR_ARG and b"null handle" in err()  # dense, in place
    assert call(True, layer=big, out_=big, stride=0) == ERR_ARG and b"overlaps" in err()  # one shared layer, two outputs over it
    assert call(True, L_=1, layer=big, out_=big, stride=0) == ERR_ARG and b"null handle" in err()
    assert call(True, layer=big, out_=big[1:]) == ERR_ARG and b"overlaps" in err()
    assert call(True, layer=big, out_=big[cells:]) == ERR_ARG and b"overlaps" in err()
    assert call(True, layer=big, out_=big[2 * cells:]) == ERR_ARG and b"null handle" in err()


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_clear_movers.cpp: plan_clear_movers laid out without an arena; at the node's shape (one 150 x 100 layer,
    K = 8 rows, M = 8 slots, owner_out included) it fits the arena of a max_batch 1024, max_horizon 50, max_obstacles 4 handle;
    host_arena_bytes is still what tests/golden/host_arena_cap.json recorded."""
    exe = str(tmp_path / "host_plan_clear_movers")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_clear_movers.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "8 arrays at most of 16" in r.stdout and "the node's shape fits" in r.stdout
    # layer, label, comp, assign, state in; layer_out, owner_out, fields out: 4 x 60000 bytes of cells, 832 + 32 + 2048 + 64 of rows
    assert "layout tracker: 8 arrays, in_end 122912, out_begin 122912, end 242976" in r.stdout
    assert "layout mask, no owner: 6 arrays, in_end 120864, out_begin 120864, end 180928" in r.stdout
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


def test_conditions(cases):
    """The restatement against the separable evaluation everywhere, and against scipy's exact Euclidean transform where no two labels
    tie; the tracker form's speeds keep their margin; the cases exercise what they are for."""
    from scipy.ndimage import distance_transform_edt
    seen = dict(contested=0, kept_unknown=0, tie=0, no_row=0, movers=0, cleared=0)
    for (shape, halo2), c in cases.items():
        assert not c["margins"] or min(c["margins"]) >= MARGIN * (1.0 - 1e-6), (shape, halo2, min(c["margins"]))
        for l in range(c["L"]):
            label = c["label"][l]
            owner, d2, tie = owners_brute(label, halo2)
            assert np.array_equal(owner, owners_separable(label, halo2)), (shape, halo2, l)
            assert np.array_equal(owner.astype(np.int32), c["want"][l]["owner"])
            linked = label >= 0
            assert np.array_equal(owner[linked], label[linked])  # a linked cell owns itself
            if linked.any():
                dist, (ni, nj) = distance_transform_edt(~linked, return_indices=True)
                e2 = np.rint(dist ** 2).astype(np.int64)
                assert np.array_equal(e2 <= halo2, owner >= 0)
                assert np.array_equal(e2[owner >= 0], d2[owner >= 0])
                sure = (owner >= 0) & ~tie
                assert np.array_equal(label[ni[sure], nj[sure]], owner[sure])
            else:
                assert (owner == -1).all()
            f = c["want"][l]["fields"]
            seen["contested"] += f[CONTESTED]
            seen["kept_unknown"] += f[KEPT_UNKNOWN]
            seen["tie"] += int((tie & (owner >= 0)).sum())
            seen["movers"] += f[MOVERS]
            seen["cleared"] += f[CLEARED]
            roots = set(np.unique(label[linked]).tolist())
            seen["no_row"] += len(roots - set(c["comp"][l][:, MO_LABEL].astype(np.int64).tolist()))
    print(seen)
    assert all(v > 0 for v in seen.values()), seen
    forms = {(c["form"], c["K"], c["M"], c["L"]) for c in cases.values()}
    assert {f[0] for f in forms} == {"tracker", "mask"} and {f[1] for f in forms} == {1, 8, 64} and {f[3] for f in forms} == {1, 3}
    assert {f[2] for f in forms if f[0] == "tracker"} == {1, 64}


def test_the_rule_header_under_the_sanitizers(cases, tmp_path):
    """tests/cpp/movers_emulation.cpp: the functions of csrc/costmap_movers.hpp driven tile after tile as the kernel drives them,
    compiled with -fsanitize=address,undefined, over the small shapes at every halo2: the brute-force owners, the nearest-mover
    distances and the mover flags, and no sanitizer report."""
    exe = str(tmp_path / "movers_emulation")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: it needs nothing loaded in front of it)
                    "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "movers_emulation.cpp")], check=True)
    records, want = [], []
    for (shape, halo2), c in cases.items():
        if shape == (150, 100) and halo2 == 1024:
            continue  # (the small shapes; the large one at the smaller halos)
        for l in range(c["L"]):
            labels = sorted({int(v) for v, m in zip(c["comp"][l][:, MO_LABEL], c["movers"][l]) if m and v >= 0})
            _, mover_d2, _ = owners_brute(c["label"][l], halo2, only=labels)
            records.append(np.array([shape[0], shape[1], halo2, len(labels)] + labels, dtype=np.int32))
            records.append(np.ascontiguousarray(c["label"][l].T).reshape(-1))
            want.append(np.ascontiguousarray(c["want"][l]["owner"].T).reshape(-1))
            want.append(np.ascontiguousarray(np.where(mover_d2 <= halo2, mover_d2, -1).astype(np.int32).T).reshape(-1))
    src, dst = tmp_path / "cases.bin", tmp_path / "owners.bin"
    np.concatenate(records).tofile(str(src))
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout.split()[0] == str(len(want) // 2)
    assert np.array_equal(np.fromfile(str(dst), dtype=np.int32), np.concatenate(want))


def test_scene_conditions(scene):
    """On the restatements alone: the figures of the crossing scene, and both picks decided."""
    from test_footprint import EDGE, HIT_STEPS, MAP_HIT_STEPS
    mg = _margins(scene["diag"])
    assert min(mg.values()) > MARGIN, mg
    assert min(scene["margins"]) > MARGIN
    last, rows, cl = scene["ticks"][-1], scene["rows"][-1], scene["cleared"][-1]
    assert rows["comp"][:2, MO_LABEL].tolist() == [152.0, 6090.0] and rows["n"][2] == 2
    assert cl["movers"].tolist() == [False, True] + [False] * (CHAIN_K - 2)
    m = int(last["assign"][1])
    v = math.hypot(last["state"][m, VX], last["state"][m, VY])
    print("crossing block: slot %d, hits %g, speed %.4f, at (%.4f, %.4f); smallest tracker margin %.2e" %
          (m, last["state"][m, HITS], v, last["state"][m, 0], last["state"][m, 1], min(mg.values())))
    assert m == 1 and last["state"][m, HITS] == 6 and abs(v - 5.0025) < 1e-3
    assert abs(last["state"][m, 0] - 10.05) < 1e-3 and abs(last["state"][m, 1] - 0.0004) < 1e-3
    assert math.hypot(last["state"][int(last["assign"][0]), VX], last["state"][int(last["assign"][0]), VY]) == 0.0
    f9, f0 = cl[SCENE_HALO2]["fields"], cl[0]["fields"]
    # (190 cells of halo are owned; the 132 of the ring change, the other 58 hold 0 already: CLEARED counts bits)
    assert f9.tolist() == [1, 312, 180, 190, 100.0, 6090, 0, 0] and f0.tolist() == [1, 180, 180, 0, 100.0, 6090, 0, 0]
    after = cl[SCENE_HALO2]["layer"]
    assert (after[2:10, 1:9] == 100.0).all() and (after[80:110, :] == 0.0).all() and (cl[0]["layer"][88:101, 38:62] == 30.0).sum() == 132
    # ticks before the track is confirmed as moving clear nothing
    cleared_per_tick = [c[SCENE_HALO2]["fields"][CLEARED] for c in scene["cleared"]]
    print("cleared per tick:", cleared_per_tick)
    assert cleared_per_tick[0] == 0 and cleared_per_tick[-1] == 312
    orig, clr = scene["judge"]["original"], scene["judge"]["cleared"]
    print("original: map hit steps %s, total %s; cleared: box hit steps %s, map hit steps %s, clearance %s, total %s; picks %s" % (
        orig["fp"][:, MAP_HIT_STEPS].tolist(), orig["total"].tolist(), clr["fp"][:, HIT_STEPS].tolist(), clr["fp"][:, MAP_HIT_STEPS].tolist(),
        clr["fp"][:, 0].tolist(), clr["total"].tolist(), scene["picks"]))
    assert orig["edge"] > EDGE and clr["edge"] > EDGE  # no cell centre within rounding of a rectangle's edge
    assert (orig["fp"][:3, MAP_HIT_STEPS] > 0).all() and orig["fp"][3, MAP_HIT_STEPS] == 0
    assert (clr["fp"][:, MAP_HIT_STEPS] == 0).all() and (clr["fp"][:, HIT_STEPS] == 0).all() and clr["fp"][:, 0].min() > 0.5
    assert scene["picks"] == dict(original=3, cleared=0)


def test_the_facade_and_the_replay_tool_export_the_setter():
    header = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_mover_clearing\s*\(\s*double\s+v_clear,\s*double\s+halo,\s*float\s+fill\s*=\s*0\.0f,\s*bool\s+on\s*=\s*true\s*\)", header)
    assert "last_mover_clearing" in header
    assert "--clear-movers" in open(os.path.join(PKG, "host", "replay_main.cpp")).read()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=8, max_horizon=50, max_obstacles=64, device=0)
    yield s
    s.close()


def _flat(a):
    """(L, rows, cols) -> (L, rows*cols) column-major per layer."""
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 1)).reshape(a.shape[0], -1)


def _device(cilqr, solver, c, layers=None, shared=False, in_place=False, want_owner=True, L=None, sel=None):
    """The device form on torch buffers.  c: a case; sel: the layers of the case to send (default all); shared: ONE layer with
    layer_stride 0 (sel must then name one layer, sent L times for the rows).  Returns dict(layer (L, rows, cols), owner, fields)."""
    import torch
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    sel = list(range(c["L"])) if sel is None else sel
    n = len(sel)
    rows, cols, K = c["rows"], c["cols"], c["K"]
    cells = rows * cols
    g = cilqr.map_geom(rows * 0.1, cols * 0.1, 0.1, 0.0, 0.0)
    g.rows, g.cols = rows, cols
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)  # noqa: E731
    src = c["layer"] if layers is None else layers
    lay = up(_flat(src[sel[:1]] if shared else src[sel]), np.float32)
    label, comp = up(_flat(c["label"][sel]), np.int32), up(c["comp"][sel], np.float64)
    out = lay if in_place else torch.full((n, cells), SENTINEL, dtype=torch.float32, device=dev)
    owner = torch.full((n, cells), -77, dtype=torch.int32, device=dev)
    fields = torch.full((n, FIELDS), SENTINEL, dtype=torch.float64, device=dev)
    kw = dict(halo2=c["halo2"], fill=c["fill"], owner_out=owner.data_ptr() if want_owner else 0)
    keep = []
    if c["form"] == "mask":
        keep.append(up(c["mask"][sel], np.int32))
        kw.update(mask=keep[0].data_ptr())
    else:
        keep += [up(c["assign"][sel], np.int32), up(c["state"][sel], np.float64)]
        kw.update(M=c["M"], assign=keep[0].data_ptr(), state=keep[1].data_ptr(), min_hits=c["min_hits"], v_clear=V_CLEAR)
    torch.cuda.synchronize(dev)
    solver.clear_movers_device(st, n, lay.data_ptr(), 0 if shared else cells, g, label.data_ptr(), K, comp.data_ptr(), out.data_ptr(),
                               fields.data_ptr(), **kw)
    torch.cuda.synchronize(dev)
    shape = lambda t: t.cpu().numpy().reshape(n, cols, rows).transpose(0, 2, 1)  # noqa: E731
    return dict(layer=shape(out), owner=shape(owner), fields=fields.cpu().numpy())


def _check(got, want, l, what, owner=True):
    w = want
    print("%s: fields %s (want %s)" % (what, got["fields"][l].tolist(), w["fields"].tolist()))
    assert np.array_equal(got["fields"][l], w["fields"]), what
    assert np.array_equal(_u32(got["layer"][l]), _u32(w["layer"])), what
    if owner:
        assert np.array_equal(got["owner"][l], w["owner"]), what


@gpu
@pytest.mark.parametrize("halo2", HALOS, ids=lambda h: "halo2_%d" % h)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_layers_owners_and_fields_against_the_restatement(cilqr, solver, cases, shape, halo2):
    c = cases[(shape, halo2)]
    got = _device(cilqr, solver, c)
    for l in range(c["L"]):
        _check(got, c["want"][l], l, "%dx%d halo2 %d %s K %d M %d layer %d" % (shape + (halo2, c["form"], c["K"], c["M"], l)))


@gpu
def test_the_host_form_and_the_binding(cilqr, solver, cases):
    """The host-buffer form through the arena, both mover forms, with and without owner_out."""
    for key in (((65, 17), 9), ((65, 17), 13), ((7, 1), 2), ((1, 7), 0)):
        c = cases[key]
        g = cilqr.map_geom(c["rows"] * 0.1, c["cols"] * 0.1, 0.1, 0.0, 0.0)
        g.rows, g.cols = c["rows"], c["cols"]
        kw = dict(mask=c["mask"]) if c["form"] == "mask" else dict(assign=c["assign"], state=c["state"], min_hits=c["min_hits"], v_clear=V_CLEAR)
        for want_owner in (True, False):
            got = solver.clear_movers(c["layer"], g, c["label"], c["comp"], halo2=c["halo2"], fill=c["fill"], want_owner=want_owner, **kw)
            assert (got["owner"] is None) == (not want_owner)
            for l in range(c["L"]):
                _check(got, c["want"][l], l, "host form %s layer %d" % (key, l), owner=want_owner)


def _hand_case(label, layer, mover_labels, halo2, fill=0.0, rowless=()):
    """A mask-form case of one layer from a label image: a row per label in ascending order but the `rowless` ones."""
    roots = [int(v) for v in np.unique(label[label >= 0]) if int(v) not in rowless]
    K = max(1, len(roots))
    comp = np.full((1, K, MO_FIELDS), -1.0)
    comp[0, :len(roots), MO_LABEL] = roots
    mask = np.zeros((1, K), dtype=np.int32)
    for k, v in enumerate(roots):
        mask[0, k] = 1 if v in mover_labels else 0
    c = dict(rows=label.shape[0], cols=label.shape[1], halo2=halo2, L=1, K=K, M=0, form="mask", fill=fill, min_hits=1, layer=layer[None].astype(np.float32),
             label=label[None].astype(np.int32), comp=comp, mask=mask, movers=[mask[0] != 0])
    c["want"] = [restate(c["layer"][0], c["label"][0], comp[0][:, MO_LABEL], c["movers"][0], halo2, fill)]
    return c


def _labels_of(linked):
    return flood_labels(linked, 0)


@gpu
def test_ownership_edges(cilqr, solver):
    """Two components equidistant from a cell; a mover against the border; a mover one cell from a component without a row; a halo
    window over three tiles; no linked cell; every row a mover."""
    # equidistant: cells (2, 1) and (2, 5); column 3 is 2 away from both, the lower label owns it whichever of the two moves
    linked = np.zeros((5, 7), dtype=bool)
    linked[2, 1] = linked[2, 5] = True
    lab = _labels_of(linked)
    lo, hi = int(lab[2, 1]), int(lab[2, 5])
    assert lo < hi
    layer = np.full((5, 7), 40.0, dtype=np.float32)
    for movers, cleared_mid in (({lo}, True), ({hi}, False)):
        c = _hand_case(lab, layer, movers, 4)
        assert c["want"][0]["owner"][2, 3] == lo and (c["want"][0]["layer"][2, 3] == 0.0) == cleared_mid
        assert c["want"][0]["fields"][CONTESTED] == (0 if cleared_mid else 1)  # kept: within reach of the mover, owned by the other
        _check(_device(cilqr, solver, c), c["want"][0], 0, "equidistant, mover %s" % movers)
    # a mover in the corners and along the borders of a map with tile seams in both directions
    linked = np.zeros((130, 35), dtype=bool)
    linked[0:3, 0:2] = linked[127:130, 33:35] = linked[63:66, 15:18] = linked[0:2, 30:35] = True
    lab = _labels_of(linked)
    layer = np.full((130, 35), 25.0, dtype=np.float32)
    c = _hand_case(lab, layer, set(np.unique(lab[lab >= 0]).tolist()), 25)
    assert c["want"][0]["fields"][MOVERS] == 4 and c["want"][0]["fields"][CONTESTED] == 0  # every row a mover: nothing contested
    _check(_device(cilqr, solver, c), c["want"][0], 0, "borders, every row a mover")
    # a mover one cell from a wall that got no row (max_size dropped it): the wall keeps its halo, the cells between go to the nearer
    linked = np.zeros((40, 20), dtype=bool)
    linked[5:35, 4] = True        # the wall
    linked[18:21, 6:9] = True     # the mover, one free column (5) between
    lab = _labels_of(linked)
    wall, mover = int(lab[5, 4]), int(lab[18, 6])
    layer = np.where(linked, 100.0, 30.0).astype(np.float32)
    c = _hand_case(lab, layer, {mover}, 9, rowless={wall})
    w = c["want"][0]
    assert wall < mover and (w["owner"][18:21, 5] == wall).all() and (w["layer"][18:21, 5] == 30.0).all()  # equal distance: the lower label
    assert (w["layer"][5:35, 4] == 100.0).all() and (w["layer"][5:35, 3] == 30.0).all() and w["fields"][CONTESTED] > 0
    assert (w["layer"][18:21, 9:12] == 0.0).all()
    _check(_device(cilqr, solver, c), w, 0, "a wall without a row")
    # one linked cell whose halo of r = 32 spans three tiles along j and two along i
    linked = np.zeros((100, 60), dtype=bool)
    linked[50, 24] = True
    lab = _labels_of(linked)
    c = _hand_case(lab, np.full((100, 60), 10.0, dtype=np.float32), {int(lab[50, 24])}, 1024)
    assert c["want"][0]["fields"][OWNED_HALO] > 2500 and c["want"][0]["owner"][50, 56] >= 0 and c["want"][0]["owner"][50, 57] == -1
    _check(_device(cilqr, solver, c), c["want"][0], 0, "three tiles")
    # no linked cell
    lab = np.full((65, 17), -1, dtype=np.int32)
    c = _hand_case(lab, np.full((65, 17), 10.0, dtype=np.float32), set(), 1024)
    assert c["want"][0]["fields"].tolist() == [0, 0, 0, 0, -1, -1, 0, 0]
    _check(_device(cilqr, solver, c), c["want"][0], 0, "no linked cell")


@gpu
def test_values(cilqr, solver):
    """NaN cells inside a mover and in its halo are kept and counted; fill NaN; fill equal to the input: CLEARED counts bit
    differences only; -0 and infinite inputs."""
    linked = np.zeros((20, 20), dtype=bool)
    linked[8:12, 8:12] = True
    lab = _labels_of(linked)
    mover = int(lab[8, 8])
    layer = np.where(linked, 100.0, 30.0).astype(np.float32)
    layer[9, 9] = layer[7, 8] = layer[0, 0] = np.nan
    layer[10, 10], layer[6, 10], layer[11, 11], layer[12, 12] = np.inf, -np.inf, -0.0, 0.0
    for fill in (0.0, np.nan, 30.0, 100.0, -0.0):
        c = _hand_case(lab, layer, {mover}, 4, fill=fill)
        w = c["want"][0]
        assert w["fields"][KEPT_UNKNOWN] == 2 and np.isnan(w["layer"][9, 9]) and np.isnan(w["layer"][7, 8])
        assert w["fields"][MAX_VALUE] == 100.0 and w["fields"][MAX_CELL] == 8 + 8 * 20
        owned = w["fields"][OWNED_LINKED] + w["fields"][OWNED_HALO]
        same = dict([(0.0, 1), (30.0, 0), (100.0, 0), (-0.0, 1)]).get(fill, 0)  # (12, 12) holds +0, (11, 11) holds -0
        if fill == 30.0:
            same = int(((w["owner"] == mover) & (layer == 30.0)).sum())
        if fill == 100.0:
            same = int(((w["owner"] == mover) & (layer == 100.0)).sum())
        assert w["fields"][CLEARED] == owned - 2 - same, (fill, w["fields"].tolist(), same)
        _check(_device(cilqr, solver, c), w, 0, "fill %r" % fill)
    # the largest value is negative; the same largest value twice: the lowest cell
    layer2 = np.full((20, 20), -7.5, dtype=np.float32)
    layer2[9, 8] = layer2[8, 9] = -2.0
    c = _hand_case(lab, layer2, {mover}, 0)
    assert c["want"][0]["fields"][MAX_VALUE] == -2.0 and c["want"][0]["fields"][MAX_CELL] == 9 + 8 * 20
    _check(_device(cilqr, solver, c), c["want"][0], 0, "negative values")


@gpu
def test_bit_properties(cilqr, solver, cases):
    """A layer's outputs are the same bits alone and as layer 2 of 3, and with a shared against a repeated layer; an in-place
    layer_out equals the out-of-place one; owner_out NULL changes nothing else."""
    for key in (((65, 17), 13), ((150, 100), 9), ((65, 17), 1024)):
        c = cases[key] if cases[key]["L"] == 3 else make_case(key[0][0], key[0][1], key[1], 3, 8, 8, "tracker", 4242)
        base = _device(cilqr, solver, c)
        for l in range(3):
            _check(base, c["want"][l], l, "%s layer %d" % (key, l))
        alone = _device(cilqr, solver, c, sel=[2])
        assert np.array_equal(_u32(alone["layer"][0]), _u32(base["layer"][2])) and np.array_equal(alone["owner"][0], base["owner"][2]), key
        assert np.array_equal(alone["fields"][0].view(np.uint64), base["fields"][2].view(np.uint64)), key
        # one shared layer (layer_stride 0) under the three layers' labels and rows, against that layer repeated
        rep = np.stack([c["layer"][1]] * 3)
        dense, shared = _device(cilqr, solver, c, layers=rep), _device(cilqr, solver, c, layers=rep, shared=True)
        assert np.array_equal(_u32(dense["layer"]), _u32(shared["layer"])) and np.array_equal(dense["owner"], shared["owner"])
        assert np.array_equal(dense["fields"].view(np.uint64), shared["fields"].view(np.uint64))
        for l in range(3):
            _check(dense, restate(rep[l], c["label"][l], c["comp"][l][:, MO_LABEL], c["movers"][l], c["halo2"], c["fill"]), l, "repeated layer %d" % l)
        in_place, no_owner = _device(cilqr, solver, c, in_place=True), _device(cilqr, solver, c, want_owner=False)
        for other in (in_place, no_owner):
            assert np.array_equal(_u32(base["layer"]), _u32(other["layer"])) and np.array_equal(base["fields"].view(np.uint64), other["fields"].view(np.uint64))
        assert np.array_equal(in_place["owner"], base["owner"]) and (no_owner["owner"] == -77).all()


@gpu
def test_limits(cilqr, solver):
    """K = 1024 rows in the mask form with r = 32: the largest LDS block; and a 1024 x 1024 layer with labels up to 2^20 - 1."""
    rng = np.random.Generator(np.random.PCG64(5))
    linked = rng.random((150, 100)) < 0.04
    lab = _labels_of(linked)
    roots = np.unique(lab[lab >= 0])
    assert 300 < roots.size <= 1024
    movers = set(roots[rng.random(roots.size) < 0.3].tolist())
    c = _hand_case(lab, np.rint(rng.random((150, 100)) * 90.0).astype(np.float32), movers, 1024)
    comp, mask = np.full((1, 1024, MO_FIELDS), -1.0), np.zeros((1, 1024), dtype=np.int32)
    order = rng.permutation(c["K"])  # rows in any order: the call sorts the mover labels itself
    comp[0, :c["K"]], mask[0, :c["K"]] = c["comp"][0][order], c["mask"][0][order]
    mask[0, c["K"]:] = 1  # filler rows under a set mask are no movers
    c.update(K=1024, comp=comp, mask=mask)
    _check(_device(cilqr, solver, c), c["want"][0], 0, "K 1024, r 32")
    big = np.full((1024, 1024), -1, dtype=np.int32)
    big[1020:1024, 1020:1024] = 1020 + 1020 * 1024
    big[1023, 1023] = (1 << 20) - 1  # (a label of its own: the largest there is)
    big[0:2, 0:2] = 0
    layer = np.full((1024, 1024), 5.0, dtype=np.float32)
    c = _hand_case(big, layer, {(1 << 20) - 1, 0}, 2)
    w = c["want"][0]
    assert w["owner"][1023, 1023] == (1 << 20) - 1 and w["fields"][OWNED_LINKED] == 5
    _check(_device(cilqr, solver, c), w, 0, "1024 x 1024")


@gpu
def test_device_chain_clears_the_crossing_block(cilqr, scene):
    """Per tick cilqr_map_distance_device -> cilqr_map_obstacles_device (K = 8) -> cilqr_track_update_device -> cilqr_clear_movers_device
    (tracker form, v_clear 1.0, fill 0; halo2 9 and, beside it, 0) on one stream, copies taken only for the comparison afterwards.
    Then the consequence: on the ORIGINAL layer cilqr_footprint_check rejects every candidate whose rectangle covers the block and
    cilqr_argmin_device picks another; on the cleared layer with the predicted track table as the check's obstacles candidate 0
    passes and is picked."""
    import torch
    from test_rollout_risk import _pick
    N, B, K = CHAIN_N, len(CHAIN_YS), CHAIN_K
    cells = CHAIN_ROWS * CHAIN_COLS
    geom = cilqr.map_geom(CHAIN_ROWS * CHAIN_RES, CHAIN_COLS * CHAIN_RES, CHAIN_RES, CHAIN_POS[0], CHAIN_POS[1])
    assert (geom.rows, geom.cols) == (CHAIN_ROWS, CHAIN_COLS)
    cf = c_filter(cilqr, scene["f"])
    solver = cilqr.Solver(scene["p"], max_batch=B, max_horizon=N, max_obstacles=K, device=0)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
        z = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=dev)  # noqa: E731
        layers = torch.from_numpy(np.ascontiguousarray(scene["layers"].transpose(0, 2, 1)).reshape(CHAIN_TICKS, cells)).to(dev)
        d2, work, label, owner = (torch.zeros(cells, dtype=torch.int32, device=dev) for _ in range(4))
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        comp, boxes = (torch.zeros((K, w), dtype=torch.float64, device=dev) for w in (13, 5))
        state, world, track, tdim, tcov = z(1, K, STATE), z(1, WORLD_FIELDS), z(1, K, 6), z(1, K, 2), z(1, K, 16)
        assign = torch.full((1, K), -77, dtype=torch.int32, device=dev)
        static9, static0 = (torch.full((cells,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2))
        f9, f0 = z(1, FIELDS), z(1, FIELDS)
        X, base = up(scene["X"]), up(SCENE_BASE)
        ppose, pdim = z(1, K, 4 * N), z(1, K, 2 * N)
        out = {n: dict(fp=z(B, 12), total=z(B), pair=z(2)) for n in ("original", "cleared")}
        kept = []
        torch.cuda.synchronize(dev)
        for k in range(CHAIN_TICKS):
            solver.map_distance_device(st, 1, layers[k].data_ptr(), 0, geom, SCENE_THRESHOLD, d2.data_ptr())
            solver.map_obstacles_device(st, 1, d2.data_ptr(), geom, K, work.data_ptr(), label.data_ptr(), counts.data_ptr(), comp.data_ptr(),
                                        boxes.data_ptr(), pad=0.0)
            solver.track_update_device(st, 1, K, K, boxes.data_ptr(), cf, state.data_ptr(), state.data_ptr(), world.data_ptr(), track.data_ptr(),
                                       tdim.data_ptr(), tcov.data_ptr(), n_det=counts.data_ptr() + 8, n_det_stride=4, assign=assign.data_ptr(),
                                       flags=1 if k == 0 else 0)
            for h2, dst, fl in ((SCENE_HALO2, static9, f9), (0, static0, f0)):
                solver.clear_movers_device(st, 1, layers[k].data_ptr(), 0, geom, label.data_ptr(), K, comp.data_ptr(), dst.data_ptr(), fl.data_ptr(),
                                           halo2=h2, fill=0.0, M=K, assign=assign.data_ptr(), state=state.data_ptr(), min_hits=scene["f"]["min_hits"],
                                           v_clear=SCENE_V_CLEAR, owner_out=owner.data_ptr() if h2 else 0)
            kept.append({n: t.clone() for n, t in dict(state=state, world=world, assign=assign, track=track, dim=tdim, cov=tcov, static9=static9,
                                                       static0=static0, f9=f9, f0=f0, owner=owner).items()})
        solver.predict_obstacles_device(st, 1, N, K, track.data_ptr(), tdim.data_ptr(), ppose.data_ptr(), pdim.data_ptr(), track_cov=tcov.data_ptr())
        for name, layer_ptr, M_, pose_ptr, dim_ptr in (("original", layers[CHAIN_TICKS - 1].data_ptr(), 0, 0, 0),
                                                      ("cleared", static9.data_ptr(), K, ppose.data_ptr(), pdim.data_ptr())):
            o = out[name]
            solver.set_uncertainty_map_device(layer_ptr, geom, (0.0, 0.0, 0.0), (3, 3))
            solver.footprint_check_device(st, B, N, M_, 1, X.data_ptr(), pose_ptr, dim_ptr, (0, N, 1, 0), o["fp"].data_ptr(),
                                          occ_threshold=SCENE_THRESHOLD, base=base.data_ptr(), total=o["total"].data_ptr())
            solver.argmin_device(st, B, o["total"].data_ptr(), o["pair"].data_ptr())
        torch.cuda.synchronize(dev)
    finally:
        solver.close()
    shape = lambda t: t.cpu().numpy().reshape(CHAIN_COLS, CHAIN_ROWS).T  # noqa: E731
    for k in range(CHAIN_TICKS):
        g = {n: t.cpu().numpy() for n, t in kept[k].items()}
        check_world({n: g[n][0] for n in ("state", "world", "assign", "track", "dim", "cov")}, scene["ticks"][k], "scene tick %d" % k)
        for h2, lay, fl in ((SCENE_HALO2, "static9", "f9"), (0, "static0", "f0")):
            want = scene["cleared"][k][h2]
            assert np.array_equal(g[fl][0], want["fields"]), (k, h2, g[fl][0].tolist(), want["fields"].tolist())
            assert np.array_equal(_u32(shape(kept[k][lay])), _u32(want["layer"])), (k, h2)
        assert np.array_equal(shape(kept[k]["owner"]), scene["cleared"][k][SCENE_HALO2]["owner"]), k
    last = {n: t.cpu().numpy() for n, t in kept[-1].items()}
    print("tick 5: fields at halo2 9 %s, at halo2 0 %s" % (last["f9"][0].tolist(), last["f0"][0].tolist()))
    assert last["f9"][0][MOVERS] == 1 and last["f9"][0][CLEARED] == 312 and last["f9"][0][OWNED_LINKED] == 180 and last["f9"][0][OWNED_HALO] == 190
    assert last["f0"][0][CLEARED] == 180 and last["f9"][0][MAX_CELL] == 6090
    assert (shape(kept[-1]["static9"])[2:10, 1:9] == 100.0).all()  # the standing block's 64 cells are kept
    picks = {}
    for name in ("original", "cleared"):
        got = {n: t.cpu().numpy() for n, t in out[name].items()}
        want = scene["judge"][name]
        assert np.array_equal(np.isnan(got["total"]), np.isnan(want["total"])), name
        assert np.array_equal(got["fp"][:, 2:4], want["fp"][:, 2:4]) and np.array_equal(got["fp"][:, 7:10], want["fp"][:, 7:10]), name
        picks[name] = int(got["pair"][1])
        assert picks[name] == _pick(want["total"]), name
        print("scene, %s: total %s, pick %d" % (name, got["total"].tolist(), picks[name]))
    assert picks == scene["picks"] == dict(original=3, cleared=0)


def _build(tmp_path, source):
    exe = str(tmp_path / os.path.splitext(os.path.basename(source))[0])
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", source), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib")],
                   check=True)
    return exe


@gpu
def test_cpp_facade_mover_clearing(scene, tmp_path):
    """tests/cpp/candidates_clear_movers.cpp: iLQR with set_map_obstacles + set_map_tracker + set_footprint_check over the six ticks of
    the crossing scene.  Off, run_candidates returns the original-map pick; on, candidate 0; the run with it on equals the C-ABI
    sequence called by hand bit for bit, last_mover_clearing equals that sequence's fields (both inside the program) and the
    restatement's (here); without set_map_tracker the setter throws."""
    r = subprocess.run([_build(tmp_path, "candidates_clear_movers.cpp")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mover clearing ok" in r.stdout and "setter without a tracker throws" in r.stdout
    fields = [[float(v) for v in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("fields:")]
    assert fields == [c[SCENE_HALO2]["fields"].tolist() for c in scene["cleared"]]
    picks = {m.group(1): int(m.group(2)) for m in re.finditer(r"pick (off|on): (-?\d+)", r.stdout)}
    assert picks["on"] == 0 and picks["off"] not in (0,), picks


@gpu
def test_replay_tool_reports_the_fields(tmp_path):
    """cilqr_replay --map-obstacles --map-tracker --clear-movers: the six ticks of the crossing scene report the eight fields per
    tick; without the option the lines are what they were; without --map-tracker the option is refused."""
    exe = os.path.join(PKG, "bin", "cilqr_replay")
    layers = scene_layers()
    ticks = []
    for k in range(CHAIN_TICKS):
        ii, jj = np.nonzero(layers[k])
        cells = ["%d %d %g" % (i, j, layers[k][i, j]) for i, j in zip(ii.tolist(), jj.tolist())]
        ticks.append("tick\nego 0 0 5 0\nobstacles 0\nmap 15.0 10.0 0.1 12.0 0.0 0.0 0.0 0.0 %d\n%s\n" % (len(cells), "\n".join(cells)))
    log = tmp_path / "crossing_block.log"
    log.write_text("cilqr-replay 1\nhorizon 10\npath 3\n0 0\n50 0\n100 0\n" + "".join(ticks))
    common = [exe, str(log), "--map-obstacles", "50,0,2,3.0", "--map-tracker", "0.1,0.5,0.05,9.21,2,3"]
    r = subprocess.run(common + ["--clear-movers", "1.0,0.31"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == CHAIN_TICKS
    tails = [[float(v) for v in line.split(" clear_movers ")[1].split()] for line in lines]
    print(tails)
    assert all(len(t) == FIELDS for t in tails)
    assert tails[-1][:4] == [1.0, 312.0, 180.0, 190.0] and tails[0][:2] == [0.0, 0.0]
    plain = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and all(" clear_movers " not in line for line in plain.stdout.splitlines())
    assert [line.split(" clear_movers ")[0].split(" tracks ")[0].split()[0] for line in lines] == [line.split()[0] for line in plain.stdout.splitlines()]
    alone = subprocess.run([exe, str(log), "--map-obstacles", "50,0,2,3.0", "--clear-movers", "1.0,0.31"], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 1 and "--map-tracker" in alone.stderr
