"""cilqr_track_update(_device): map obstacles tracked across ticks — association and Kalman update (csrc/cilqr_track.hip).

Expected values never come from the HIP path: `tick_restate` below restates the seven steps of include/cilqr.h in numpy, matrix
form, one world and one tick at a time.  The restatement itself is checked on the CPU (test_conditions) against a Kalman update
written in information form and against scipy.optimize.linear_sum_assignment on every tick of every scene: there the greedy
assignment must have the optimal gated cost and as many matches.  That is a condition on the scenes, not a property of the call.

Tolerances are the suite's: positions and velocities 1e-9 absolute (coordinates within +-100 m), every covariance 1e-9 of its
largest entry; integers, IDs, assign, DET, counts and everything the header calls a bit copy are exact or compared by bits.
test_conditions asserts, on the restatement alone, that every decision has a margin of 1e-6, so that 1e-9 cannot flip it:
|d2 - gate2| of every pair, the gap between winner and runner-up of every greedy round, |v - v_min| and ||cos| - |sin|| of the swap
rule.  The random worlds of the shape tests are drawn with a seed that is advanced until those margins hold (the seed is part of
the case, the margins are asserted).
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

gpu = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -4
TOL = 1e-9
MARGIN = 1e-6
FAR = 1.0e6
STATE, WORLD_FIELDS = 32, 9
X, Y, VX, VY, P0 = 0, 1, 2, 3, 4
SIZE_X, SIZE_Y, YAW, ID, HITS, MISSES, AGE, DET = range(20, 28)
NEXT_ID, TICKS, LIVE, CONFIRMED, MATCHED, BORN, DIED, DROPPED, INVALID = range(9)
ENTRY_POINTS = ("cilqr_track_update", "cilqr_track_update_device")
SHAPES = [(1, 1, 0), (1, 1, 1), (1, 2, 3), (3, 63, 64), (2, 64, 64), (5, 64, 1), (1, 64, 0)]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the filter ---------------------------------------------------------------------------------------------------------------
def white_q(q, dt):
    Q = np.zeros((4, 4))
    for a in (0, 1):
        Q[a, a], Q[a, a + 2], Q[a + 2, a], Q[a + 2, a + 2] = q * dt ** 3 / 3, q * dt ** 2 / 2, q * dt ** 2 / 2, q * dt
    return Q


def make_filter(dt=0.1, q=0.5, r=0.05, p_birth=(0.05 ** 2, 0.05 ** 2, 16.0, 16.0), gate2=9.21, min_hits=2, max_misses=3, v_min=1.0,
                theta_var_slow=0.25, Q=None, R=None, P_birth=None):
    return dict(dt=dt, Q=white_q(q, dt) if Q is None else np.array(Q, dtype=float), R=np.eye(2) * r * r if R is None else np.array(R, dtype=float),
                P_birth=np.diag(p_birth) if P_birth is None else np.array(P_birth, dtype=float), gate2=gate2, min_hits=min_hits,
                max_misses=max_misses, v_min=v_min, theta_var_slow=theta_var_slow)


def c_filter(cilqr, f):
    return cilqr.track_filter(f["dt"], f["Q"], f["R"], f["P_birth"], gate2=f["gate2"], min_hits=f["min_hits"], max_misses=f["max_misses"],
                              v_min=f["v_min"], theta_var_slow=f["theta_var_slow"])


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _sym_upper(A):
    """Entries with row <= column, mirrored."""
    U = np.triu(np.asarray(A, dtype=float))
    return U + np.triu(U, 1).T


def _cm(row16):
    """[r + 4c] -> [r][c]"""
    return np.asarray(row16, dtype=float).reshape(4, 4).T


def free_table(M):
    st = np.zeros((M, STATE))
    st[:, ID] = -1.0
    return st


H = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0]])


def tick_restate(f, state, world, det, n=None, reset=False, diag=None):
    """One tick of one world.  state (M, 32), world (9,), det (D, 5).  Returns dict(state, world, assign, track, dim, cov (M, 4, 4)
    as [r][c]).  `diag`, a dict of lists, collects the margins of the decisions taken and what the CPU checks need."""
    M, D = state.shape[0], det.shape[0]
    n = D if n is None else min(max(int(n), 0), D)
    dt, Q, R = f["dt"], _sym_upper(f["Q"]), _sym_upper(f["R"])
    st = free_table(M)
    next_id = ticks = 0.0
    if not reset:
        next_id, ticks = float(world[NEXT_ID]), float(world[TICKS])
        for m in range(M):
            if state[m, ID] >= 0.0:
                st[m] = state[m]
                st[m, 28:] = 0.0
    live = st[:, ID] >= 0.0
    F = np.eye(4)
    F[0, 2] = F[1, 3] = dt
    P = np.zeros((M, 4, 4))
    # 1 predict
    for m in np.nonzero(live)[0]:
        st[m, X] = st[m, X] + dt * st[m, VX]
        st[m, Y] = st[m, Y] + dt * st[m, VY]
        P[m] = _sym_upper(F @ _sym_upper(_cm(st[m, P0:P0 + 16])) @ F.T + Q)
        st[m, AGE] += 1.0
    # 2 gate
    valid = np.array([d < n and bool(np.isfinite(det[d, 0]) and np.isfinite(det[d, 1])) for d in range(D)], dtype=bool)
    d2 = np.full((M, D), np.nan)
    adm = np.zeros((M, D), dtype=bool)
    for m in np.nonzero(live)[0]:
        S = P[m][:2, :2] + R
        dS = S[0, 0] * S[1, 1] - S[0, 1] * S[0, 1]
        if not dS > 0.0:
            continue
        for d in np.nonzero(valid)[0]:
            nx, ny = det[d, 0] - st[m, X], det[d, 1] - st[m, Y]
            q = (S[1, 1] * nx * nx - 2.0 * S[0, 1] * nx * ny + S[0, 0] * ny * ny) / dS
            d2[m, d] = q
            adm[m, d] = bool(q <= f["gate2"])
            if diag is not None and np.isfinite(q) and np.isfinite(f["gate2"]):
                diag["gate"].append(abs(q - f["gate2"]))
    # 3 associate
    slot_of, det_of = np.full(D, -1), np.full(M, -1)
    while True:
        pairs = sorted((d2[m, d], m, d) for m in range(M) for d in range(D) if adm[m, d] and det_of[m] < 0 and slot_of[d] < 0)
        if not pairs:
            break
        if diag is not None and len(pairs) > 1:
            diag["greedy"].append(pairs[1][0] - pairs[0][0])
        _, m, d = pairs[0]
        det_of[m], slot_of[d] = d, m
    if diag is not None:
        diag["d2"].append(d2)
        diag["adm"].append(adm)
        diag["det_of"].append(det_of.copy())
    # 4 update, 5 miss and death
    died = np.zeros(M, dtype=bool)
    for m in np.nonzero(live)[0]:
        d = det_of[m]
        if d >= 0:
            S = H @ P[m] @ H.T + R
            K = P[m] @ H.T @ np.linalg.inv(S)
            nu = det[d, :2] - st[m, :2]
            if diag is not None:
                diag["update"].append((st[m, :4].copy(), P[m].copy(), det[d, :2].copy(), R))
            st[m, :4] = st[m, :4] + K @ nu
            A = np.eye(4) - K @ H
            P[m] = _sym_upper(A @ P[m] @ A.T + K @ R @ K.T)
            if diag is not None:
                diag["updated"].append((st[m, :4].copy(), P[m].copy()))
            st[m, SIZE_X], st[m, SIZE_Y], st[m, YAW] = det[d, 3], det[d, 4], det[d, 2]
            st[m, HITS] += 1.0
            st[m, MISSES] = 0.0
            st[m, DET] = float(d)
        else:
            st[m, MISSES] += 1.0
            st[m, DET] = -1.0
            if st[m, MISSES] > f["max_misses"]:
                died[m] = True
    for m in np.nonzero(died)[0]:
        st[m] = 0.0
        st[m, ID] = -1.0
        P[m] = 0.0
    # 6 birth
    waiting = [d for d in range(D) if valid[d] and slot_of[d] < 0]
    room = [m for m in range(M) if not live[m]]
    born = min(len(waiting), len(room))
    for r in range(born):
        m, d = room[r], waiting[r]
        st[m] = 0.0
        st[m, X], st[m, Y] = det[d, 0], det[d, 1]
        P[m] = _sym_upper(f["P_birth"])
        st[m, SIZE_X], st[m, SIZE_Y], st[m, YAW] = det[d, 3], det[d, 4], det[d, 2]
        st[m, ID] = next_id + r
        st[m, HITS] = 1.0
        st[m, DET] = float(d)
        slot_of[d] = m
    for m in range(M):
        st[m, P0:P0 + 16] = P[m].T.reshape(16)
    assign = np.where(valid, slot_of, -2).astype(np.int32)
    live_now = st[:, ID] >= 0.0
    conf = live_now & (st[:, HITS] >= f["min_hits"])
    wo = np.zeros(WORLD_FIELDS)
    wo[NEXT_ID], wo[TICKS] = next_id + born, ticks + 1.0
    wo[LIVE], wo[CONFIRMED], wo[MATCHED], wo[BORN] = live_now.sum(), conf.sum(), (det_of >= 0).sum(), born
    wo[DIED], wo[DROPPED], wo[INVALID] = died.sum(), len(waiting) - born, sum(1 for d in range(n) if not valid[d])
    # 7 output
    track, dim, cov = np.zeros((M, 6)), np.zeros((M, 2)), np.zeros((M, 4, 4))
    track[:, 0] = track[:, 1] = FAR
    for m in np.nonzero(conf)[0]:
        vx, vy = st[m, VX], st[m, VY]
        v = math.hypot(vx, vy)
        if diag is not None:
            diag["speed"].append(abs(v - f["v_min"]))
        track[m, 0], track[m, 1] = st[m, X], st[m, Y]
        if v >= f["v_min"]:
            th = math.atan2(vy, vx)
            track[m, 2], track[m, 3] = v, th
            J = np.eye(4)
            J[2:, 2:] = [[vx / v, vy / v], [-vy / (v * v), vx / (v * v)]]
            cov[m] = _sym_upper(J @ P[m] @ J.T)
            c, s = abs(math.cos(th - st[m, YAW])), abs(math.sin(th - st[m, YAW]))
            if diag is not None:
                diag["swap"].append(abs(c - s))
            dim[m] = (st[m, SIZE_X], st[m, SIZE_Y]) if c >= s else (st[m, SIZE_Y], st[m, SIZE_X])
        else:
            track[m, 3] = st[m, YAW]
            cov[m][:2, :2] = P[m][:2, :2]
            cov[m][2, 2] = P[m][2, 2] + P[m][3, 3]
            cov[m][3, 3] = f["theta_var_slow"]
            dim[m] = (st[m, SIZE_X], st[m, SIZE_Y])
    return dict(state=st, world=wo, assign=assign, track=track, dim=dim, cov=cov)


def new_diag():
    return dict(gate=[], greedy=[], speed=[], swap=[], d2=[], adm=[], det_of=[], update=[], updated=[])


def run_restate(f, M, ticks, diag=None):
    """ticks: list of (det (D, 5), n).  Returns the list of per-tick results, the state carried."""
    state, world, out = free_table(M), np.zeros(WORLD_FIELDS), []
    for k, (det, n) in enumerate(ticks):
        r = tick_restate(f, state, world, det, n, reset=(k == 0), diag=diag)
        state, world = r["state"], r["world"]
        out.append(r)
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _pack(rows, D):
    """Detections of one tick in ascending (y, x), the stand-in for the label order of the map; padded to D rows with NaN (beyond n)."""
    rows = sorted(rows, key=lambda r: (r[1], r[0]))
    det = np.full((D, 5), np.nan)
    for i, r in enumerate(rows):
        det[i] = r
    return det, len(rows)


def scene_c():
    """The issue's scene C.  Objects: A crossing, post C, B oncoming, post D from tick 6, a fifth from tick 10."""
    rng = np.random.default_rng(7)
    dt, ticks, who = 0.1, [], []
    for k in range(16):
        t = k * dt
        objs = {"A": (20.0, -6.0 + 5.0 * t, math.pi / 2 + 0.03, 4.5, 1.9), "C": (12.0, -3.0, 0.3, 0.5, 0.3),
                "B": (35.0 - 4.0 * t, 3.4, 0.02, 4.4, 1.8)}
        if k in (7, 8):
            del objs["A"]
        if k >= 6:
            objs["D"] = (28.0, -4.0, -0.4, 0.5, 0.3)
        if k >= 10:
            objs["E"] = (5.0, 6.0, 0.1, 0.6, 0.6)
        rows = []
        for name in sorted(objs):
            o = objs[name]
            e = rng.normal(0.0, 0.03, 2)
            rows.append((o[0] + e[0], o[1] + e[1], o[2], o[3], o[4], name))
        rows.sort(key=lambda r: (r[1], r[0]))
        who.append([r[5] for r in rows])
        ticks.append(_pack([r[:5] for r in rows], 6))
    return dict(name="C", f=make_filter(), M=4, ticks=ticks, who=who)


def scene_death():
    """Death and slot reuse.  P at (10, 0) is seen at ticks 0-2 and lost from tick 3: with max_misses = 2 it is freed at tick 5.  Z at
    (20, -5) is seen throughout.  N at (30, 5) appears at tick 5: the slot freed that tick takes no birth (DROPPED), tick 6 gives it
    the slot with a new ID."""
    rng = np.random.default_rng(11)
    ticks = []
    for k in range(9):
        rows = [(20.0, -5.0, 0.0, 1.0, 1.0)]
        if k <= 2:
            rows.append((10.0, 0.0, 0.2, 2.0, 1.0))
        if k >= 5:
            rows.append((30.0, 5.0, 0.4, 3.0, 1.5))
        rows = [(r[0] + e[0], r[1] + e[1]) + r[2:] for r, e in ((r, rng.normal(0.0, 0.02, 2)) for r in rows)]
        ticks.append(_pack(rows, 3))
    return dict(name="death", f=make_filter(max_misses=2), M=2, ticks=ticks)


def scene_standing_and_swap():
    """A standing track (a creeping object at 0.2 m/s under v_min = 1), a vehicle heading along +y whose box yaw is 0.05 (sizes swap)
    and one heading along +x with the same yaw (sizes stay)."""
    rng = np.random.default_rng(13)
    ticks = []
    for k in range(8):
        t = 0.1 * k
        rows = [(-10.0 + 0.2 * t, 4.0, 0.7, 1.2, 0.8), (0.0, -8.0 + 6.0 * t, 0.05, 4.6, 2.0), (8.0 + 6.0 * t, 9.0, 0.05, 4.2, 1.7)]
        rows = [(r[0] + e[0], r[1] + e[1]) + r[2:] for r, e in ((r, rng.normal(0.0, 0.01, 2)) for r in rows)]
        ticks.append(_pack(rows, 4))
    return dict(name="standing_swap", f=make_filter(), M=5, ticks=ticks)


def scene_contested():
    """Two tracks gate the same detection and the nearer wins: posts at (0, 0) and (1, 0) seen twice, then one return at (0.4, 0.02);
    R = 0.3^2 keeps both inside the gate.  The other track coasts; both are seen again afterwards."""
    ticks = [_pack([(0.0, 0.0, 0.0, 0.3, 0.3), (1.0, 0.01, 0.0, 0.3, 0.3)], 2), _pack([(0.02, -0.01, 0.0, 0.3, 0.3), (0.97, 0.0, 0.0, 0.3, 0.3)], 2),
             _pack([(0.4, 0.02, 0.0, 0.3, 0.3)], 2), _pack([(0.01, 0.01, 0.0, 0.3, 0.3), (1.02, -0.02, 0.0, 0.3, 0.3)], 2)]
    return dict(name="contested", f=make_filter(r=0.3, p_birth=(0.09, 0.09, 1.0, 1.0)), M=3, ticks=ticks)


SCENES = (scene_c, scene_death, scene_standing_and_swap, scene_contested)


# ---- random worlds for the shape tests -----------------------------------------------------------------------------------------
def random_world(M, D, seed):
    """One tick from a mid-life table: live and free slots on a 4 m grid, detections near some predicted positions, clutter on free grid
    points (births; more of them than free slots where D allows), misses at the limit."""
    rng = np.random.default_rng(seed)
    f = make_filter(gate2=13.8, max_misses=2)
    grid = [(-30.0 + 4.0 * (i % 16), -14.0 + 4.0 * (i // 16)) for i in range(128)]
    order = rng.permutation(128)
    state, used = free_table(M), []
    live = rng.random(M) < 0.7
    if M >= 2:
        live[0], live[M - 1] = True, False
    for m in np.nonzero(live)[0]:
        g = grid[order[m]]
        sp, th = rng.choice([0.0, 0.3, 3.0, 6.0]), rng.uniform(-math.pi, math.pi)
        L = rng.normal(0.0, 1.0, (4, 4)) * np.array([0.05, 0.05, 0.6, 0.6])[:, None]
        Pm = L @ L.T + np.diag([1e-3, 1e-3, 0.05, 0.05])
        state[m, :4] = (g[0], g[1], sp * math.cos(th), sp * math.sin(th))
        state[m, P0:P0 + 16] = Pm.T.reshape(16)
        state[m, SIZE_X:YAW + 1] = (rng.uniform(0.5, 5.0), rng.uniform(0.5, 2.0), rng.uniform(-math.pi, math.pi))
        state[m, ID], state[m, HITS], state[m, MISSES], state[m, AGE] = 100 + m, rng.integers(1, 4), rng.integers(0, 3), rng.integers(1, 9)
        state[m, DET] = -1.0 if state[m, MISSES] else 0.0
        used.append(m)
    world = np.zeros(WORLD_FIELDS)
    world[NEXT_ID], world[TICKS] = 200.0, 17.0
    rows = []
    for m in used:
        if rng.random() < 0.7:
            pred = state[m, :2] + f["dt"] * state[m, 2:4]
            rows.append((pred[0] + rng.normal(0, 0.04), pred[1] + rng.normal(0, 0.04), rng.uniform(-3, 3), rng.uniform(0.5, 5), rng.uniform(0.5, 2)))
    k = M
    while len(rows) < D:
        g = grid[order[k % 128]]
        k += 1
        rows.append((g[0] + rng.normal(0, 0.04), g[1] + rng.normal(0, 0.04), rng.uniform(-3, 3), rng.uniform(0.5, 5), rng.uniform(0.5, 2)))
    rows = rows[:D]
    det = np.array(rows, dtype=float).reshape(-1, 5)[rng.permutation(len(rows))] if rows else np.zeros((0, 5))
    return dict(f=f, state=state, world=world, det=det.reshape(D, 5))


def _margins(diag):
    return {k: (min(diag[k]) if diag[k] else math.inf) for k in ("gate", "greedy", "speed", "swap")}


def decided_world(M, D, seed):
    """random_world at the first seed, counted up from `seed`, whose decisions all have ten times the margin test_conditions asserts."""
    for s in range(seed, seed + 50):
        wd = random_world(M, D, s)
        diag = new_diag()
        tick_restate(wd["f"], wd["state"], wd["world"], wd["det"], diag=diag)
        if min(_margins(diag).values()) > 10 * MARGIN:
            wd["seed"] = s
            return wd
    raise AssertionError("no decided world for M %d D %d from seed %d" % (M, D, seed))


@pytest.fixture(scope="module")
def cases():
    """Every scene and every random world with its restated results, computed once and left unchanged."""
    out = dict(scenes={}, worlds={})
    for make in SCENES:
        sc = make()
        sc["diag"] = new_diag()
        sc["want"] = run_restate(sc["f"], sc["M"], sc["ticks"], sc["diag"])
        out["scenes"][sc["name"]] = sc
    for (W, M, D) in SHAPES:
        worlds = [decided_world(M, D, 1000 * M + 10 * D + 100 * w) for w in range(W)]
        for wd in worlds:
            wd["diag"] = new_diag()
            wd["want"] = tick_restate(wd["f"], wd["state"], wd["world"], wd["det"], diag=wd["diag"])
        out["worlds"][(W, M, D)] = worlds
    return out


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_export_the_calls(cilqr):
    full = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    h = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in ENTRY_POINTS:
        assert name in cilqr.ABI_SYMBOLS, name
        assert hasattr(cilqr.lib(), name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    assert cilqr.lib().cilqr_abi_version() == 2  # additive: the ABI number stays
    for name in ("track_update", "track_update_device"):
        assert callable(getattr(cilqr.Solver, name)), name
    # the enums and sizes of the header against the binding's constants and this file's
    enum = {k: int(v) for k, v in re.findall(r"\bCILQR_(T[SW]_[A-Z_]+)\s*=\s*(\d+)", h)}
    mine = dict(TS_X=X, TS_Y=Y, TS_VX=VX, TS_VY=VY, TS_P=P0, TS_SIZE_X=SIZE_X, TS_SIZE_Y=SIZE_Y, TS_YAW=YAW, TS_ID=ID, TS_HITS=HITS,
                TS_MISSES=MISSES, TS_AGE=AGE, TS_DET=DET, TW_NEXT_ID=NEXT_ID, TW_TICKS=TICKS, TW_LIVE=LIVE, TW_CONFIRMED=CONFIRMED,
                TW_MATCHED=MATCHED, TW_BORN=BORN, TW_DIED=DIED, TW_DROPPED=DROPPED, TW_INVALID=INVALID)
    assert enum == mine
    for k, v in mine.items():
        assert getattr(cilqr, k) == v, k
    defs = {k: v for k, v in re.findall(r"#define\s+CILQR_(TRACK_(?!MAP_)[A-Z_]+)\s+(\w+)", h)}
    assert defs == dict(TRACK_MAX_SLOTS="64", TRACK_MAX_DETECTIONS="64", TRACK_STATE="32", TRACK_WORLD_FIELDS="9", TRACK_RESET="1u")
    assert (cilqr.TRACK_STATE, cilqr.TRACK_WORLD_FIELDS, cilqr.TRACK_RESET, cilqr.TRACK_MAX_SLOTS) == (STATE, WORLD_FIELDS, 1, 64)
    assert C.sizeof(cilqr.TrackFilter) == 8 * (1 + 16 + 4 + 16 + 3) + 2 * 4
    assert "NOT the optimal" in full and "constant velocity" in full  # the header says what greedy and the model leave out
    plan = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert re.search(r"inline\s+void\s+plan_track_update\s*\(", plan)
    api = open(os.path.join(PKG, "csrc", "cilqr_api.cpp")).read()
    assert "plan_track_update(" in api and "launch_track_update" in open(os.path.join(PKG, "csrc", "cilqr_internal.h")).read()
    mk = open(os.path.join(PKG, "Makefile")).read()
    assert "csrc/cilqr_track.hip" in mk and re.search(r"^check:.*build/cilqr_track\.o", mk, flags=re.M)
    assert re.search(r"check_kernel_resources\.py --map .*build/cilqr_track\.o", mk)


def test_argument_errors_need_no_device(cilqr):
    """Every argument error of the header without a handle; valid arguments then meet the null handle."""
    L = cilqr.lib()
    W, M, D = 2, 3, 4
    det, st, wo = np.zeros((W, D, 5)), np.zeros((W, M, STATE)), np.zeros((W, WORLD_FIELDS))
    tr, dm, cv, asg, cnt = np.zeros((W, M, 6)), np.zeros((W, M, 2)), np.zeros((W, M, 16)), np.zeros((W, D), dtype=np.int32), np.zeros(W, dtype=np.int32)
    no_handle = C.c_void_p()
    good = make_filter()

    def call(dev, W_=W, M_=M, D_=D, flags=0, stride=1, filt=good, **nulls):
        a = dict(det=det, f=True, state_in=st, state_out=st, world=wo, track_out=tr, dim_out=dm, cov_out=cv)
        a.update(nulls)
        cf = c_filter(cilqr, filt)
        fn = L.cilqr_track_update_device if dev else L.cilqr_track_update
        head = (no_handle, None) if dev else (no_handle,)
        return fn(*head, W_, M_, D_, _p(a["det"]), _p(cnt, _ip), C.c_int64(stride), C.byref(cf) if a["f"] else None, _p(a["state_in"]),
                  _p(a["state_out"]), _p(a["world"]), C.c_uint32(flags), _p(asg, _ip), _p(a["track_out"]), _p(a["dim_out"]), _p(a["cov_out"]))

    for dev in (False, True):
        for name in ("f", "state_out", "world", "track_out", "dim_out", "cov_out"):
            assert call(dev, **{name: None}) == ERR_ARG and b"null required pointer" in L.cilqr_last_error(), name
        assert call(dev, state_in=None) == ERR_ARG and b"state_in" in L.cilqr_last_error()
        assert call(dev, state_in=None, flags=1) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # RESET needs no state_in
        assert call(dev, det=None) == ERR_ARG and b"det is null" in L.cilqr_last_error()
        assert call(dev, det=None, D_=0) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # D = 0 needs no det
        for kw in (dict(W_=0), dict(M_=0), dict(D_=-1), dict(W_=-3)):
            assert call(dev, **kw) == ERR_ARG and b"at least" in L.cilqr_last_error(), kw
        assert call(dev, stride=-1) == ERR_ARG and b"n_det_stride" in L.cilqr_last_error()
        for flags in (2, 3, 0x80000000):
            assert call(dev, flags=flags) == ERR_ARG and b"unknown flag bits" in L.cilqr_last_error()
        nan, inf = float("nan"), float("inf")
        for key, values in (("dt", (0.0, -0.1, nan, inf)), ("gate2", (-1.0, nan)), ("v_min", (-0.5, nan)), ("theta_var_slow", (-1e-9, nan)),
                            ("min_hits", (0, -1)), ("max_misses", (-1,))):
            for v in values:
                bad = dict(good)
                bad[key] = v
                assert call(dev, filt=bad) == ERR_ARG and key.encode() in L.cilqr_last_error(), (key, v)
        for key, v in (("gate2", inf), ("gate2", 0.0), ("v_min", 0.0), ("theta_var_slow", 0.0), ("max_misses", 0), ("min_hits", 1)):
            ok = dict(good)
            ok[key] = v
            assert call(dev, filt=ok) == ERR_ARG and b"null handle" in L.cilqr_last_error(), (key, v)
        assert call(dev, M_=65) == ERR_UNSUPPORTED and b"at most 64" in L.cilqr_last_error()
        assert call(dev, D_=65) == ERR_UNSUPPORTED and b"at most 64" in L.cilqr_last_error()
        assert call(dev, M_=64, D_=64) == ERR_ARG and b"null handle" in L.cilqr_last_error()
        assert call(dev) == ERR_ARG and b"null handle" in L.cilqr_last_error()  # valid arguments, no handle


def _information_form(x, P, z, R):
    """The Kalman update by the inverse covariances."""
    Pi, Ri = np.linalg.inv(P), np.linalg.inv(R)
    Pn = np.linalg.inv(Pi + H.T @ Ri @ H)
    return Pn @ (Pi @ x + H.T @ Ri @ z), Pn


def _optimal(d2, adm):
    """(matches, cost) of the best gated assignment: most matches first, then the smallest summed d2."""
    from scipy.optimize import linear_sum_assignment
    if not adm.any():
        return 0, 0.0
    big = 1.0e6  # above every gated sum: a pair outside the gate is never worth taking
    cost = np.where(adm, d2, big)
    r, c = linear_sum_assignment(cost)
    take = adm[r, c]
    return int(take.sum()), float(cost[r, c][take].sum())


def test_conditions(cases):
    """What keeps the GPU comparisons from hiding a failure, on the restatement's numbers alone."""
    # every decision of every scene and every random world has its margin
    for name, sc in cases["scenes"].items():
        mg = _margins(sc["diag"])
        print("scene %s: margins gate %.3g greedy %.3g speed %.3g swap %.3g" % (name, mg["gate"], mg["greedy"], mg["speed"], mg["swap"]))
        assert min(mg.values()) > MARGIN, (name, mg)
    for shape, worlds in cases["worlds"].items():
        for wd in worlds:
            mg = _margins(wd["diag"])
            assert min(mg.values()) > MARGIN, (shape, wd["seed"], mg)
            assert np.max(np.abs(wd["want"]["state"][:, :2])) < 100.0
    # the Kalman update against the information form, on every update of every scene
    worst_x = worst_p = 0.0
    n_updates = 0
    for sc in cases["scenes"].values():
        for (x, P, z, R), (xn, Pn) in zip(sc["diag"]["update"], sc["diag"]["updated"]):
            xi, Pi = _information_form(x, P, z, R)
            worst_x = max(worst_x, float(np.max(np.abs(xi - xn))))
            worst_p = max(worst_p, float(np.max(np.abs(Pi - Pn)) / np.max(np.abs(Pn))))
            n_updates += 1
    print("Joseph form against the information form over %d updates: state %.3g, P %.3g of its largest entry" % (n_updates, worst_x, worst_p))
    assert n_updates > 40 and worst_x <= 1e-9 and worst_p <= 1e-9
    # greedy equals the optimal gated assignment on every tick of every scene
    for name, sc in cases["scenes"].items():
        for k, (d2, adm, det_of) in enumerate(zip(sc["diag"]["d2"], sc["diag"]["adm"], sc["diag"]["det_of"])):
            got = [(m, d) for m, d in enumerate(det_of) if d >= 0]
            n_opt, c_opt = _optimal(d2, adm)
            c_got = sum(d2[m, d] for m, d in got)
            assert len(got) == n_opt and abs(c_got - c_opt) <= 1e-9 * max(1.0, c_opt), (name, k, got, n_opt, c_opt)
    # scene C: what the issue describes
    c = cases["scenes"]["C"]
    want, who = c["want"], c["who"]
    worlds = np.array([r["world"] for r in want])
    assert worlds[0, BORN] == 3 and worlds[6, BORN] == 1 and worlds[:, BORN].sum() == 4
    assert np.all(worlds[10:, DROPPED] == 1) and np.all(worlds[:10, DROPPED] == 0)
    assert want[6]["state"][3, ID] == 3 and np.all(want[5]["state"][3, ID] == -1)  # the post at tick 6 takes the last slot
    slot_a = int(want[0]["assign"][who[0].index("A")])
    id_a = want[0]["state"][slot_a, ID]
    assert [r["state"][slot_a, DET] for r in want[7:9]] == [-1.0, -1.0] and [r["state"][slot_a, MISSES] for r in want[7:10]] == [1.0, 2.0, 0.0]
    assert all(r["state"][slot_a, ID] == id_a for r in want)  # A coasts two ticks and is re-acquired with its ID
    assert want[9]["assign"][who[9].index("A")] == slot_a
    slot_b = int(want[0]["assign"][who[0].index("B")])
    va = [r["track"][slot_a, 2] for r in want[10:]]
    vb = [r["track"][slot_b, 2] for r in want[10:]]
    print("scene C: speeds of A %.3f ... %.3f, of B %.3f ... %.3f; IDs %s" % (min(va), max(va), min(vb), max(vb), want[-1]["state"][:, ID].tolist()))
    assert 4.8 < min(va) and max(va) < 5.2 and 3.8 < min(vb) and max(vb) < 4.2
    assert len({w.index("B") for w in who[6:10]}) > 1 and who[5].index("A") != who[9].index("A")  # the detection order changes
    for r in want:
        assert np.all(r["world"][[LIVE, MATCHED, BORN]] >= 0) and r["world"][LIVE] <= 4
    # death and slot reuse
    d = cases["scenes"]["death"]["want"]
    ids = [r["state"][:, ID].tolist() for r in d]
    slot_p = int(d[0]["assign"][1])  # P is the second detection of tick 0 in (y, x) order
    assert abs(d[0]["state"][slot_p, X] - 10.0) < 0.1
    assert ids[4][slot_p] >= 0 and ids[5][slot_p] == -1 and d[5]["world"][DIED] == 1 and d[5]["world"][DROPPED] == 1 and d[5]["world"][BORN] == 0
    assert d[6]["world"][BORN] == 1 and ids[6][slot_p] == 2.0 and ids[6][slot_p] not in ids[0]  # a NEW id in the freed slot
    assert np.all(d[5]["state"][slot_p, [c for c in range(STATE) if c != ID]] == 0.0)
    # standing track, size swap
    s = cases["scenes"]["standing_swap"]["want"][-1]
    rows = {int(s["assign"][i]): i for i in range(3)}
    by_x = sorted(rows, key=lambda m: s["state"][m, X])  # the creeping object, the one along +y, the one along +x
    st, up, along = by_x
    assert s["track"][st, 2] == 0.0 and s["track"][st, 3] == s["state"][st, YAW] and s["cov"][st][3, 3] == 0.25 and s["cov"][st][0, 2] == 0.0
    assert abs(s["track"][up, 3] - math.pi / 2) < 0.05 and s["dim"][up].tolist() == [s["state"][up, SIZE_Y], s["state"][up, SIZE_X]]
    assert abs(s["track"][along, 3]) < 0.05 and s["dim"][along].tolist() == [s["state"][along, SIZE_X], s["state"][along, SIZE_Y]]
    # contested detection: both tracks gate it, the nearer one takes it
    q = cases["scenes"]["contested"]
    adm2, d22, det2 = q["diag"]["adm"][2], q["diag"]["d2"][2], q["diag"]["det_of"][2]
    assert adm2[:2, 0].all() and d22[0, 0] < d22[1, 0] and det2[0] == 0 and det2[1] == -1 and q["want"][2]["state"][1, MISSES] == 1
    # the random worlds reach what the shapes are for
    w = cases["worlds"]
    assert all(x["want"]["world"][DROPPED] > 0 for x in w[(2, 64, 64)]) and all(x["want"]["world"][MATCHED] > 5 for x in w[(3, 63, 64)])
    assert any(x["want"]["world"][DIED] > 0 for x in w[(2, 64, 64)] + w[(3, 63, 64)] + w[(5, 64, 1)])
    assert all(x["want"]["world"][BORN] > 0 for x in w[(3, 63, 64)])


def test_the_host_form_fits_the_unchanged_arena(tmp_path):
    """tests/cpp/host_plan_track_update.cpp: plan_track_update laid out without an arena against host_arena_bytes at the shapes
    include/cilqr.h says always fit; host_arena_bytes is still what tests/golden/host_arena_cap.json recorded."""
    exe = str(tmp_path / "host_plan_track_update")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_track_update.cpp")], check=True)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))["cases"]
    r = subprocess.run([exe] + [str(v) for case in golden for v in case[:3]], capture_output=True, text=True, timeout=60)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every shape fits" in r.stdout and "9 arrays at most of 16" in r.stdout
    assert "layout in place: 8 arrays, in_end 2448, out_begin 256, end 4016" in r.stdout  # det and counts in, state and world both ways
    assert "layout reset, D 0: 5 arrays, in_end 0, out_begin 0" in r.stdout  # a first tick sends nothing up
    got = [[int(v) for v in re.findall(r"\d+", line)] for line in r.stdout.splitlines() if line.startswith("arena ")]
    assert got == golden and len(got) > 20


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver(cilqr):
    s = cilqr.Solver(cilqr.default_params(), max_batch=8, max_horizon=50, max_obstacles=64, device=0)
    yield s
    s.close()


SENTINEL = -123.456


class DeviceWorlds:
    """W worlds on the device: the table, the world records and the output rows, updated by the device form."""

    def __init__(self, solver, cf, W, M, D, state=None, world=None):
        import torch
        self.torch, self.solver, self.cf, self.W, self.M, self.D = torch, solver, cf, W, M, D
        self.dev = torch.device("cuda", 0)
        z = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=self.dev)  # noqa: E731
        self.state = z(W, M, STATE) if state is None else self.up(state)
        self.world = z(W, WORLD_FIELDS) if world is None else self.up(world)
        self.track, self.dim, self.cov = z(W, M, 6), z(W, M, 2), z(W, M, 16)
        self.assign = torch.full((W, max(D, 1)), -77, dtype=torch.int32, device=self.dev)

    def up(self, a, dtype=np.float64):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def tick(self, det, n_det=None, stride=1, reset=False, state_out=None, n_det_ptr=None):
        """det (W, D, 5).  n_det: None, or an int32 array read with `stride`.  Returns the numpy results."""
        torch = self.torch
        tdet = self.up(det) if self.D else None
        tn = None if n_det is None else self.up(n_det, np.int32)
        out_state = self.state if state_out is None else state_out
        torch.cuda.synchronize(self.dev)
        self.solver.track_update_device(torch.cuda.current_stream(self.dev).cuda_stream, self.W, self.M, self.D,
                                        tdet.data_ptr() if self.D else 0, self.cf, self.state.data_ptr(), out_state.data_ptr(),
                                        self.world.data_ptr(), self.track.data_ptr(), self.dim.data_ptr(), self.cov.data_ptr(),
                                        n_det=n_det_ptr if n_det_ptr is not None else (0 if tn is None else tn.data_ptr()),
                                        n_det_stride=stride, assign=self.assign.data_ptr() if self.D else 0, flags=1 if reset else 0)
        torch.cuda.synchronize(self.dev)
        return self.results(out_state)

    def results(self, out_state=None):
        out_state = self.state if out_state is None else out_state
        return dict(state=out_state.cpu().numpy(), world=self.world.cpu().numpy(), assign=self.assign.cpu().numpy()[:, :self.D],
                    track=self.track.cpu().numpy(), dim=self.dim.cpu().numpy(), cov=self.cov.cpu().numpy())


def _world_of(res, w):
    return {k: v[w] for k, v in res.items()}


def check_world(got, want, what):
    """One world's results against the restatement's: tolerances and exactness as the module docstring lists them."""
    gs, ws = got["state"], want["state"]
    M = gs.shape[0]
    assert not np.any(gs == SENTINEL) and not np.any(got["track"] == SENTINEL) and not np.any(got["cov"] == SENTINEL), what
    assert not np.any(got["dim"] == SENTINEL) and not np.any(got["world"] == SENTINEL), what
    exact = [ID, HITS, MISSES, AGE, DET, 28, 29, 30, 31]
    assert np.array_equal(gs[:, exact], ws[:, exact]), (what, gs[:, exact], ws[:, exact])
    assert np.array_equal(_bits(gs[:, SIZE_X:YAW + 1]), _bits(ws[:, SIZE_X:YAW + 1])), what  # bit copies of the detection
    assert np.array_equal(got["world"], want["world"]), (what, got["world"], want["world"])
    assert np.array_equal(got["assign"], want["assign"]), (what, got["assign"], want["assign"])
    dx = float(np.max(np.abs(gs[:, :4] - ws[:, :4])))
    gP, wP = gs[:, P0:P0 + 16].reshape(M, 4, 4).swapaxes(1, 2), ws[:, P0:P0 + 16].reshape(M, 4, 4).swapaxes(1, 2)
    scale = np.max(np.abs(wP), axis=(1, 2), keepdims=True)
    dP = float(np.max(np.abs(gP - wP) / np.where(scale > 0, scale, 1.0)))
    assert np.array_equal(_bits(gP), _bits(gP.swapaxes(1, 2))), what  # exactly symmetric
    free = ws[:, ID] < 0
    assert np.all(gs[free][:, [c for c in range(STATE) if c != ID]] == 0.0), what  # a free slot: ID -1, everything else 0
    # the rows cilqr_predict_obstacles reads
    gt, wt = got["track"], want["track"]
    dt_ = float(np.max(np.abs(gt[:, :4] - wt[:, :4])))
    assert np.all(gt[:, 4:] == 0.0), what  # constant velocity: a and omega are 0
    assert np.array_equal(_bits(got["dim"]), _bits(want["dim"])), (what, got["dim"], want["dim"])
    gC, wC = got["cov"].reshape(M, 4, 4).swapaxes(1, 2), want["cov"]
    cs = np.max(np.abs(wC), axis=(1, 2), keepdims=True)
    dC = float(np.max(np.abs(gC - wC) / np.where(cs > 0, cs, 1.0)))
    assert np.array_equal(_bits(gC), _bits(gC.swapaxes(1, 2))), what
    filler = wt[:, 0] == FAR
    assert np.all(gt[filler] == [FAR, FAR, 0, 0, 0, 0]) and np.all(got["dim"][filler] == 0.0) and np.all(gC[filler] == 0.0), what
    standing = ~filler & (wt[:, 2] == 0.0)
    assert np.array_equal(_bits(gC[standing][:, :2, :2]), _bits(gP[standing][:, :2, :2])), what  # the position block is bit-copied
    assert np.all(gC[standing][:, :2, 2:] == 0.0) and np.all(gC[standing][:, 2, 3] == 0.0), what  # every cross term is 0
    assert np.array_equal(_bits(gt[standing][:, 3]), _bits(gs[standing][:, YAW])), what
    print("%s: state %.3g, P %.3g, track %.3g, cov %.3g" % (what, dx, dP, dt_, dC))
    assert dx <= TOL and dP <= TOL and dt_ <= TOL and dC <= TOL, what


def _stack(worlds, key):
    return np.stack([wd[key] for wd in worlds])


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "W%d_M%d_D%d" % s)
def test_one_tick_of_random_worlds(cilqr, solver, cases, shape):
    """The wavefront's edges: an empty detection list, a full wave, one lane short of full, more detections than slots, more births than
    free slots.  Every world against the restatement; in place."""
    W, M, D = shape
    worlds = cases["worlds"][shape]
    dw = DeviceWorlds(solver, c_filter(cilqr, worlds[0]["f"]), W, M, D, _stack(worlds, "state"), _stack(worlds, "world"))
    got = dw.tick(_stack(worlds, "det"))
    for w, wd in enumerate(worlds):
        check_world(_world_of(got, w), wd["want"], "W %d M %d D %d world %d (seed %d)" % (W, M, D, w, wd["seed"]))
        print("  world %d: %s" % (w, wd["want"]["world"].tolist()))


@gpu
@pytest.mark.parametrize("name", ["C", "death", "standing_swap", "contested"])
def test_scenes_over_all_their_ticks(cilqr, solver, cases, name):
    """Scene C and the further scenes: the device form with the state carried on the device, in place, and the host form with the
    state carried by the caller; both against the restatement at every tick, and equal to each other by bits."""
    sc = cases["scenes"][name]
    M, D = sc["M"], sc["ticks"][0][0].shape[0]
    cf = c_filter(cilqr, sc["f"])
    dw = DeviceWorlds(solver, cf, 1, M, D)
    host = None
    for k, (det, n) in enumerate(sc["ticks"]):
        got = dw.tick(det[None], n_det=np.array([n], dtype=np.int32), reset=(k == 0))
        check_world(_world_of(got, 0), sc["want"][k], "scene %s tick %d, device form" % (name, k))
        if k == 0:
            host = solver.track_update(det, cf, n_det=[n], reset=True, M=M)
        else:
            host = solver.track_update(det, cf, state=host["state"], world=host["world"], n_det=[n])
        for key in ("state", "world", "track", "dim", "cov"):
            assert np.array_equal(_bits(host[key]), _bits(got[key][0]), ), (name, k, key)
        assert np.array_equal(host["assign"], got["assign"][0])
    print("scene %s: last world record %s" % (name, sc["want"][-1]["world"].tolist()))


@gpu
def test_bit_properties(cilqr, solver, cases):
    """A world alone against the same world at positions 0, 2 and 4 of five; in place against a separate state_out; CILQR_TRACK_RESET
    against a hand-initialised all-free table; n_det NULL against counts equal to D; n_det read with stride 4 from a (W, 4) array."""
    five = cases["worlds"][(3, 63, 64)] + cases["worlds"][(3, 63, 64)][:2]
    M, D = 63, 64
    cf = c_filter(cilqr, five[0]["f"])
    together = DeviceWorlds(solver, cf, 5, M, D, _stack(five, "state"), _stack(five, "world")).tick(_stack(five, "det"))
    for w in (0, 2, 4):
        alone = DeviceWorlds(solver, cf, 1, M, D, five[w]["state"][None], five[w]["world"][None]).tick(five[w]["det"][None])
        for key in alone:
            assert np.array_equal(_bits(alone[key][0]) if alone[key].dtype == np.float64 else alone[key][0],
                                  _bits(together[key][w]) if together[key].dtype == np.float64 else together[key][w]), (w, key)
    # in place against a separate state_out (whose input table is left as it was)
    dw = DeviceWorlds(solver, cf, 5, M, D, _stack(five, "state"), _stack(five, "world"))
    sep = dw.torch.full((5, M, STATE), SENTINEL, dtype=dw.torch.float64, device=dw.dev)
    apart = dw.tick(_stack(five, "det"), state_out=sep)
    assert np.array_equal(_bits(dw.state.cpu().numpy()), _bits(_stack(five, "state")))
    for key in apart:
        assert np.array_equal(apart[key].view(np.uint8), together[key].view(np.uint8)), key
    # RESET against an all-free table with NEXT_ID = 0; garbage in state and world must not be read under RESET
    M2, D2 = 64, 64
    two = cases["worlds"][(2, 64, 64)]
    cf2 = c_filter(cilqr, two[0]["f"])
    by_reset = DeviceWorlds(solver, cf2, 2, M2, D2).tick(_stack(two, "det"), reset=True)  # sentinel state and world: not read
    by_hand = DeviceWorlds(solver, cf2, 2, M2, D2, np.stack([free_table(M2)] * 2), np.zeros((2, WORLD_FIELDS))).tick(_stack(two, "det"))
    for key in by_reset:
        assert np.array_equal(by_reset[key].view(np.uint8), by_hand[key].view(np.uint8)), key
    assert by_reset["world"][0].tolist() == [64.0, 1.0, 64.0, 0.0, 0.0, 64.0, 0.0, 0.0, 0.0]  # (min_hits 2: none confirmed yet)
    # n_det NULL against counts equal to D, and counts read with stride 4 from a (W, 4) array (the n_out of cilqr_map_obstacles)
    st, wo, det = _stack(two, "state"), _stack(two, "world"), _stack(two, "det")
    null = DeviceWorlds(solver, cf2, 2, M2, D2, st, wo).tick(det)
    full = DeviceWorlds(solver, cf2, 2, M2, D2, st, wo).tick(det, n_det=np.array([D2, D2], dtype=np.int32))
    n_out = np.array([[7, 7, 40, 9], [3, 3, 64, 1]], dtype=np.int32)
    strided = DeviceWorlds(solver, cf2, 2, M2, D2, st, wo)
    tn = strided.up(n_out, np.int32)
    by4 = strided.tick(det, n_det_ptr=tn.data_ptr() + 8, stride=4)
    for key in null:
        assert np.array_equal(null[key].view(np.uint8), full[key].view(np.uint8)), key
    for w, n in enumerate((40, 64)):
        want = tick_restate(two[w]["f"], two[w]["state"], two[w]["world"], two[w]["det"], n=n)
        assert np.array_equal(by4["assign"][w], want["assign"]) and np.array_equal(by4["world"][w], want["world"]), w
        assert np.all(by4["assign"][w][n:] == -2)
    assert not np.array_equal(by4["world"][0], null["world"][0])
    # counts outside [0, D] are clamped
    clamp = DeviceWorlds(solver, cf2, 2, M2, D2, st, wo).tick(det, n_det=np.array([D2 + 1000, -5], dtype=np.int32))
    assert np.array_equal(clamp["world"][0], null["world"][0]) and np.all(clamp["assign"][1] == -2) and clamp["world"][1][MATCHED] == 0


@gpu
def test_nan_containment(cilqr, solver, cases):
    """A detection with x = NaN is INVALID, gets assign -2 and changes no other bit of the world; a NaN in one slot's state leaves every
    other slot's bits as they are."""
    wd = cases["worlds"][(2, 64, 64)][0]
    M, D = 64, 64
    cf = c_filter(cilqr, wd["f"])
    # a table without a free slot, so that a detection far from everything is DROPPED: the finite twin of the invalid one
    st = wd["state"].copy()
    for m in np.nonzero(st[:, ID] < 0)[0]:
        st[m] = st[0]
        st[m, :2] = (90.0 - 0.5 * m, -90.0)
        st[m, ID] = 300 + m
    j = 5
    far, bad = wd["det"].copy(), wd["det"].copy()
    far[j, :2] = (-95.0, 95.0)
    bad[j, 0] = np.nan
    a = DeviceWorlds(solver, cf, 1, M, D, st[None], wd["world"][None]).tick(far[None])
    b = DeviceWorlds(solver, cf, 1, M, D, st[None], wd["world"][None]).tick(bad[None])
    want = tick_restate(wd["f"], st, wd["world"], bad)
    check_world(_world_of(b, 0), want, "a detection with x = NaN")
    assert b["assign"][0][j] == -2 and a["assign"][0][j] == -1 and b["world"][0][INVALID] == 1 and a["world"][0][DROPPED] == b["world"][0][DROPPED] + 1
    for key in ("state", "track", "dim", "cov"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), key
    others = [d for d in range(D) if d != j]
    assert np.array_equal(a["assign"][0][others], b["assign"][0][others])
    keep = [c for c in range(WORLD_FIELDS) if c not in (DROPPED, INVALID)]
    assert np.array_equal(a["world"][0][keep], b["world"][0][keep])
    # a NaN in the state of a slot that matches nothing either way
    k = int(np.nonzero(wd["state"][:, ID] < 0)[0][0])
    assert np.all(a["state"][0][k, DET] == -1)  # the healthy twin at (90, -90) misses
    for col in (X, P0, VX):
        sick = st.copy()
        sick[k, col] = np.nan
        c = DeviceWorlds(solver, cf, 1, M, D, sick[None], wd["world"][None]).tick(far[None])
        rest = [m for m in range(M) if m != k]
        for key in ("state", "track", "dim", "cov"):
            assert np.array_equal(_bits(a[key][0][rest]), _bits(c[key][0][rest])), (col, key)
        assert np.array_equal(a["assign"], c["assign"]) and np.array_equal(a["world"], c["world"]), col
        assert np.isnan(c["state"][0][k]).any() and c["state"][0][k, MISSES] == a["state"][0][k, MISSES]


# ---- the device chain: map -> distance -> obstacles -> tracker -> prediction -> judge -> pick ------------------------------------
CHAIN_ROWS, CHAIN_COLS, CHAIN_RES, CHAIN_POS = 150, 100, 0.1, (12.0, 0.0)
CHAIN_K, CHAIN_TICKS, CHAIN_N = 8, 6, 30
CHAIN_MAX_RISK = 0.02
CHAIN_YS = (0.0, -0.8, -1.6, -2.4)


def chain_layers():
    """Six 150 x 100 layers at 0.1 m: an 8 x 8-cell block that stands and a 20 x 9-cell block that moves 5 cells per tick towards
    larger i, that is towards smaller x: an oncoming vehicle at 5 m/s for a tracker with dt = 0.1."""
    layers = np.zeros((CHAIN_TICKS, CHAIN_ROWS, CHAIN_COLS), dtype=np.float32)
    for k in range(CHAIN_TICKS):
        layers[k, 2:10, 1:9] = 100.0
        layers[k, 20 + 5 * k:40 + 5 * k, 8:17] = 100.0
    return layers


def chain_restate(p):
    """The whole chain on the restatements: tests/test_map_obstacles.py's for the boxes, this file's for the tracks, predict_restate and
    restate_cov of tests/test_predict_obstacles.py for the prediction and the judge.  p: the parameters at N = CHAIN_N."""
    from test_chance_risk import SIGMA0, _total
    from test_map_obstacles import NONE, components_restate, d2_of, flood_labels, rows_restate
    from test_predict_obstacles import _cm as cm16, predict_restate, restate_cov
    from test_rollout_risk import _pick
    N, B, K = CHAIN_N, len(CHAIN_YS), CHAIN_K
    layers = chain_layers()
    x_first, y_first = CHAIN_POS[0] + (0.5 * CHAIN_ROWS * CHAIN_RES - 0.5 * CHAIN_RES), CHAIN_POS[1] + (0.5 * CHAIN_COLS * CHAIN_RES - 0.5 * CHAIN_RES)
    f = make_filter()
    state, world, ticks, rows = free_table(K), np.zeros(WORLD_FIELDS), [], []
    diag = new_diag()
    for k in range(CHAIN_TICKS):
        seed = layers[k] > 50.0
        d2 = d2_of(seed)
        lab = flood_labels((d2 != NONE) & (d2 <= 0), 0)
        comp, boxes, _ = components_restate(d2, lab, CHAIN_RES, x_first, y_first, (0.0, 0.0, 0.0), 0.0)
        r = rows_restate(comp, boxes, int(seed.sum()), K, 1, math.inf)
        rows.append(dict(r, d2=d2, label=lab))
        t = tick_restate(f, state, world, r["boxes"], n=int(r["n"][2]), reset=(k == 0), diag=diag)
        state, world = t["state"], t["world"]
        ticks.append(t)
    last = ticks[-1]
    X, U, Kg = np.zeros((B, N + 1, 4)), np.zeros((B, N, 2)), np.zeros((B, N, 4, 2))
    X[:, :, 0], X[:, :, 2] = 5.0 * p.timestep * np.arange(N + 1), 5.0
    for b, y in enumerate(CHAIN_YS):
        X[b, :, 1] = y
    Kg[:, :, 2, 0] = -1.0  # the constant gain of tests/test_chance_risk.py
    Kg[:, :, 1, 1], Kg[:, :, 3, 1] = -0.5, -1.5
    X, U, Kg = X.reshape(B, -1), U.reshape(B, -1), Kg.reshape(B, -1)
    sigma0, base = cm16(SIGMA0), np.array([1.0, 2.0, 3.0, 4.0])
    cov16 = np.stack([c.T.reshape(16) for c in last["cov"]])
    pr = predict_restate(p.timestep, N, last["track"][None], cov16[None], None)
    pose = np.ascontiguousarray(np.broadcast_to(pr["pose"].reshape(1, K, 4 * N), (B, K, 4 * N)))
    dim = np.ascontiguousarray(np.broadcast_to(np.repeat(last["dim"][:, None, :], N, axis=1).reshape(1, K, 2 * N), (B, K, 2 * N)))
    c3 = np.stack([pr["sigma"][0, :, :, 0, 0], pr["sigma"][0, :, :, 0, 1], pr["sigma"][0, :, :, 1, 1]], axis=-1)
    cov = np.ascontiguousarray(np.broadcast_to(c3[None], (B, K, N, 3)))
    tracked = restate_cov(p, N, X, U, Kg, sigma0, None, pose, dim, cov)
    # the same boxes taken as standing: this tick's rows of cilqr_map_obstacles, constant over the horizon, no covariance
    spose = np.ascontiguousarray(np.broadcast_to(np.repeat(rows[-1]["pose"][:, None, :], N, axis=1).reshape(1, K, 4 * N), (B, K, 4 * N)))
    sdim = np.ascontiguousarray(np.broadcast_to(np.repeat(rows[-1]["dim"][:, None, :], N, axis=1).reshape(1, K, 2 * N), (B, K, 2 * N)))
    standing = restate_cov(p, N, X, U, Kg, sigma0, None, spose, sdim, None)
    picks = dict(tracked=_pick(_total(tracked["risk"], base, CHAIN_MAX_RISK)), standing=_pick(_total(standing["risk"], base, CHAIN_MAX_RISK)))
    return dict(p=p, layers=layers, f=f, rows=rows, ticks=ticks, diag=diag, X=X, U=U, K=Kg, sigma0=sigma0, base=base, pred=pr, tracked=tracked,
                standing=standing, picks=picks)


@pytest.fixture(scope="module")
def chain(cilqr):
    return chain_restate(cilqr.default_params(CHAIN_N))


def test_chain_conditions(chain):
    """On the restatements alone: the moving block's track has its speed, the tracked pick differs from the pick with the same boxes
    taken as standing, and every decision on the way is decided."""
    from test_chance_risk import MARGIN as RISK_MARGIN, STEP_RISK, _decided
    mg = _margins(chain["diag"])
    assert min(mg.values()) > MARGIN, mg
    last = chain["ticks"][-1]
    moving = [m for m in range(CHAIN_K) if last["track"][m, 2] > 0.0]
    assert len(moving) == 1 and last["world"][CONFIRMED] == 2 and last["world"][LIVE] == 2
    m = moving[0]
    v, th = last["track"][m, 2], last["track"][m, 3]
    ids = [t["state"][m, ID] for t in chain["ticks"]]
    step, bare = chain["tracked"]["risk"][:, STEP_RISK], chain["standing"]["risk"][:, STEP_RISK]
    print("chain: moving track in slot %d, id %s, speed %.4f m/s, heading %.4f rad, dims %s" % (m, ids, v, th, last["dim"][m].tolist()))
    print("chain: CR_STEP_RISK tracked %s, standing %s; max_risk %g; picks %s" % (step.tolist(), bare.tolist(), CHAIN_MAX_RISK, chain["picks"]))
    assert abs(v - 5.0) < 0.25 and abs(abs(th) - math.pi) < 0.05 and len(set(ids)) == 1
    assert last["dim"][m].tolist() == [2.0, 0.9] or np.allclose(last["dim"][m], [2.0, 0.9], atol=1e-12)
    assert chain["picks"]["tracked"] != chain["picks"]["standing"], chain["picks"]
    assert np.min(np.abs(step - CHAIN_MAX_RISK)) > RISK_MARGIN and np.min(np.abs(bare - CHAIN_MAX_RISK)) > RISK_MARGIN
    gs, ge = _decided(chain["tracked"])
    assert gs.min() > RISK_MARGIN and ge.min() > RISK_MARGIN


@gpu
def test_device_chain_from_the_map_to_the_pick(cilqr, chain):
    """Per tick cilqr_map_distance_device -> cilqr_map_obstacles_device (K = 8) -> cilqr_track_update_device reading n_out + 2 with stride 4;
    after the last tick cilqr_predict_obstacles_device -> cilqr_chance_risk_cov_device on four straight candidates -> cilqr_argmin_device:
    one stream, device buffers, nothing read back between the calls (the per-tick copies below are taken for the comparison after the
    last call has been enqueued).  Every stage against its restatement; the pick differs from the one with this tick's boxes taken as
    standing."""
    import torch
    from test_chance_risk import STEP_RISK, _check_against, _total
    from test_rollout_risk import _pick
    N, B, K = CHAIN_N, len(CHAIN_YS), CHAIN_K
    cells = CHAIN_ROWS * CHAIN_COLS
    geom = cilqr.map_geom(CHAIN_ROWS * CHAIN_RES, CHAIN_COLS * CHAIN_RES, CHAIN_RES, CHAIN_POS[0], CHAIN_POS[1])
    assert (geom.rows, geom.cols) == (CHAIN_ROWS, CHAIN_COLS)
    cf = c_filter(cilqr, chain["f"])
    solver = cilqr.Solver(chain["p"], max_batch=B, max_horizon=N, max_obstacles=K, device=0)
    try:
        dev = torch.device("cuda", 0)
        st = torch.cuda.current_stream(dev).cuda_stream
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
        z = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float64, device=dev)  # noqa: E731
        layers = torch.from_numpy(np.ascontiguousarray(chain["layers"].transpose(0, 2, 1)).reshape(CHAIN_TICKS, cells)).to(dev)
        d2, work, label = (torch.zeros(cells, dtype=torch.int32, device=dev) for _ in range(3))
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        comp, boxes, pose_out, dim_out = (torch.zeros((K, w), dtype=torch.float64, device=dev) for w in (13, 5, 4, 2))
        state, world, track, tdim, tcov = z(1, K, STATE), z(1, WORLD_FIELDS), z(1, K, 6), z(1, K, 2), z(1, K, 16)
        assign = torch.full((1, K), -77, dtype=torch.int32, device=dev)
        X, U, Kg, s0, base = (up(chain[n]) for n in ("X", "U", "K", "sigma0", "base"))
        ppose, pdim, pcov = z(1, K, 4 * N), z(1, K, 2 * N), z(1, K, 3 * N)
        out = {n: dict(risk=z(B, 6), step_risk=z(B, N), entry_p=z(B, K * N), sigma=z(B, N + 1, 16), total=z(B), pair=z(2)) for n in ("tracked", "standing")}
        kept = []
        torch.cuda.synchronize(dev)
        for k in range(CHAIN_TICKS):
            solver.map_distance_device(st, 1, layers[k].data_ptr(), 0, geom, 50.0, d2.data_ptr())
            solver.map_obstacles_device(st, 1, d2.data_ptr(), geom, K, work.data_ptr(), label.data_ptr(), counts.data_ptr(), comp.data_ptr(),
                                        boxes.data_ptr(), pose_out.data_ptr(), dim_out.data_ptr(), pad=0.0)
            solver.track_update_device(st, 1, K, K, boxes.data_ptr(), cf, state.data_ptr(), state.data_ptr(), world.data_ptr(), track.data_ptr(),
                                       tdim.data_ptr(), tcov.data_ptr(), n_det=counts.data_ptr() + 8, n_det_stride=4, assign=assign.data_ptr(),
                                       flags=1 if k == 0 else 0)
            kept.append({n: t.clone() for n, t in dict(boxes=boxes, counts=counts, state=state, world=world, assign=assign, track=track, dim=tdim, cov=tcov).items()})
        solver.predict_obstacles_device(st, 1, N, K, track.data_ptr(), tdim.data_ptr(), ppose.data_ptr(), pdim.data_ptr(), track_cov=tcov.data_ptr(),
                                        cov_out=pcov.data_ptr())
        for name, pose_ptr, dim_ptr, strides, cov_ptr in (("tracked", ppose.data_ptr(), pdim.data_ptr(), (0, N, 1, 0), pcov.data_ptr()),
                                                          ("standing", pose_out.data_ptr(), dim_out.data_ptr(), (0, 1, 0, 0), 0)):
            o = out[name]
            solver.chance_risk_cov_device(st, B, N, K, X.data_ptr(), U.data_ptr(), Kg.data_ptr(), s0.data_ptr(), 0, 0, pose_ptr, dim_ptr, strides,
                                          cov_ptr, o["risk"].data_ptr(), o["step_risk"].data_ptr(), o["entry_p"].data_ptr(), o["sigma"].data_ptr(),
                                          o["total"].data_ptr(), base.data_ptr(), max_risk=CHAIN_MAX_RISK)
            solver.argmin_device(st, B, o["total"].data_ptr(), o["pair"].data_ptr())
        torch.cuda.synchronize(dev)
    finally:
        solver.close()
    for k in range(CHAIN_TICKS):
        g = {n: t.cpu().numpy() for n, t in kept[k].items()}
        rows = chain["rows"][k]
        assert np.array_equal(g["counts"], rows["n"]) and np.max(np.abs(g["boxes"] - rows["boxes"])) <= TOL, k
        check_world({n: g[n][0] for n in ("state", "world", "assign", "track", "dim", "cov")}, chain["ticks"][k], "chain tick %d" % k)
    want = chain["pred"]
    assert np.max(np.abs(ppose.cpu().numpy().reshape(K, N, 4) - want["pose"][0])) <= TOL
    picks = {}
    for name in ("tracked", "standing"):
        got = {n: t.cpu().numpy() for n, t in out[name].items()}
        _check_against(got, chain[name], "chain, " + name)
        expect = _total(chain[name]["risk"], chain["base"], CHAIN_MAX_RISK)
        assert np.array_equal(np.isnan(got["total"]), np.isnan(expect))
        picks[name] = int(got["pair"][1])
        assert picks[name] == _pick(expect), name
        print("chain, %s: CR_STEP_RISK %s, pick %d" % (name, got["risk"][:, STEP_RISK].tolist(), picks[name]))
    assert picks == chain["picks"] and picks["tracked"] != picks["standing"]


# ---- the facade and the replay tool ---------------------------------------------------------------------------------------------
def test_the_facade_and_the_replay_tool_export_the_tracker():
    header = open(os.path.join(PKG, "host", "ilqr_adapter.h")).read()
    assert re.search(r"void\s+set_map_tracker\s*\(\s*const\s+cilqr_track_filter&\s*f,\s*int\s+slots,\s*bool\s+on\s*=\s*true\s*\)", header)
    assert "last_tracks" in header and "last_track_counts" in header
    assert "--map-tracker" in open(os.path.join(PKG, "host", "replay_main.cpp")).read()
    # the tracker runs at set_uncertainty_map, outside the candidate pipeline: its layout header knows nothing of it
    assert "track_update" not in open(os.path.join(PKG, "host", "candidate_layout.h")).read()


@gpu
def test_cpp_facade_map_tracker(tmp_path):
    """tests/cpp/candidates_map_tracker.cpp: four set_uncertainty_map calls with a moving block under set_map_obstacles + set_map_tracker
    against the C-ABI sequence called by hand, bit for bit (inside the program); the moving track against this file's restatement of
    the same scene (here)."""
    from test_map_obstacles import NONE, components_restate, d2_of, flood_labels, rows_restate
    exe = str(tmp_path / "candidates_map_tracker")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "host"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidates_map_tracker.cpp"), "-L" + os.path.join(PKG, "lib"), "-lcilqr_hip",
                    "-Wl,-rpath," + os.path.join(PKG, "lib")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "map tracker ok" in r.stdout
    got = [[float(v) for v in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("track:")]
    # the restatement of the program's four maps (the first four layers of the chain scene)
    layers = chain_layers()[:4]
    x_first, y_first = CHAIN_POS[0] + (0.5 * CHAIN_ROWS * CHAIN_RES - 0.5 * CHAIN_RES), CHAIN_POS[1] + (0.5 * CHAIN_COLS * CHAIN_RES - 0.5 * CHAIN_RES)
    f, state, world, want = make_filter(), free_table(8), np.zeros(WORLD_FIELDS), []
    for k in range(4):
        d2 = d2_of(layers[k] > 50.0)
        lab = flood_labels((d2 != NONE) & (d2 <= 0), 0)
        comp, boxes, _ = components_restate(d2, lab, CHAIN_RES, x_first, y_first, (0.0, 0.0, 0.0), 0.0)
        rows = rows_restate(comp, boxes, int((layers[k] > 50.0).sum()), 8, 1, math.inf)
        t = tick_restate(f, state, world, rows["boxes"], n=int(rows["n"][2]), reset=(k == 0))
        state, world = t["state"], t["world"]
        for m in range(8):
            if t["track"][m, 2] > 0.0:
                want.append([k, t["state"][m, ID]] + t["track"][m, :4].tolist())
    assert len(got) == len(want) == 3
    assert np.max(np.abs(np.array(got) - np.array(want))) <= TOL, (got, want)
    assert abs(got[-1][4] - 5.0) < 0.25
    tracked = [float(v) for v in re.search(r"risk tracked:(.*)", r.stdout).group(1).split()]
    standing = [float(v) for v in re.search(r"risk standing:(.*)", r.stdout).group(1).split()]
    assert tracked[0] > 0.01 > standing[0]


@gpu
def test_replay_tool_reports_the_tracks(tmp_path):
    """cilqr_replay --map-obstacles --map-tracker: four ticks whose maps hold a block that moves 5 cells of 0.1 m per tick report, from
    the second tick on, one confirmed track with a stable ID, heading along -x, at the block's speed; without the option the lines are
    what they were."""
    exe = os.path.join(PKG, "bin", "cilqr_replay")
    ticks = []
    for k in range(4):
        cells = ["%d %d 100" % (i, j) for i in range(20 + 5 * k, 40 + 5 * k) for j in range(8, 17)]
        ticks.append("tick\nego 0 0 5 0\nobstacles 0\nmap 15.0 10.0 0.1 12.0 0.0 0.0 0.0 0.0 %d\n%s\n" % (len(cells), "\n".join(cells)))
    log = tmp_path / "moving_block.log"
    log.write_text("cilqr-replay 1\nhorizon 10\npath 3\n0 0\n50 0\n100 0\n" + "".join(ticks))
    r = subprocess.run([exe, str(log), "--map-obstacles", "50,0,2,3.0", "--map-tracker", "0.1,0.5,0.05,9.21,2,3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 4
    tails = [line.split(" tracks ")[1].split() for line in lines]
    print(tails)
    assert tails[0] == ["0"] and all(t[0] == "1" and t[1] == "0" for t in tails[1:])
    speeds, headings, xs = [float(t[4]) for t in tails[1:]], [float(t[5]) for t in tails[1:]], [float(t[2]) for t in tails[1:]]
    assert abs(speeds[-1] - 5.0) < 0.25 and all(abs(abs(h) - math.pi) < 0.05 for h in headings) and xs[0] > xs[1] > xs[2]
    plain = subprocess.run([exe, str(log), "--map-obstacles", "50,0,2,3.0"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and all(" tracks " not in line and line.endswith(" map_obstacles 1 1") for line in plain.stdout.splitlines())
    alone = subprocess.run([exe, str(log), "--map-tracker", "0.1,0.5,0.05,9.21,2,3"], capture_output=True, text=True, timeout=120)
    assert alone.returncode == 1 and "--map-obstacles" in alone.stderr
