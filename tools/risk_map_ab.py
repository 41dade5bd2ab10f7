#!/usr/bin/env python3
"""The map rollout-risk launch (cilqr_rollout_risk_map_device) beside the solve launch and the obstacle risk launch (cilqr_rollout_risk_device)
of the same batch, in one process, alternated round by round so that all see the same clocks and neighbours:

  config-2 scenes   B = 1024, N = 50, M = 4 static obstacles, S = 64 start offsets shared by the batch (65 536 rollout rows), the node's
                    150 x 100 map at 0.2 m: one layer and pose shared by the batch, and one layer and pose per solve; footprint probes
                    3 x 3, and 1 x 1 (one lookup per state: what is left is the rollout itself)
  planner's shape   B = 16 of the same scenes with S = 1024

The map is set while the solve runs (the node's situation), so the solve launch is the map-cost instantiation.  Before anything is
timed, the counts, shares, worst rows and entries of the new launch are asserted equal to a numpy reduction of the STORED rollouts
(cilqr_rollout_batch_device) of the first --check solves — the probes and the bilinear lookup restated in numpy — and the worst occupancy
within 1e-9.  Times are device events; the launches are short, so a window holds --reps launches back to back and is divided by their
number.  Nothing is promised in advance: the file reports the medians.

    python tools/risk_map_ab.py [--rounds R] [--reps K] [--out profiles/r12_risk_map.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402

GEOM, POSE, THRESHOLD = (30.0, 20.0, 0.2, 15.0, 0.0), (-1.0, 0.4, 0.05), 50.0
SAFE = (1.1, 0.9)  # safe_length, safe_width of the launch file


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


def smooth_layer(rows, cols, seed):
    """Five Gaussian bumps through 100*tanh(z/100), then 12 unknown cells: occupied regions with soft edges, as a blurred costmap has."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    z = np.zeros((rows, cols))
    for _ in range(5):
        ci, cj = rng.uniform(0, rows), rng.uniform(0, cols)
        si, sj = rng.uniform(rows / 16, rows / 6), rng.uniform(cols / 10, cols / 4)
        z += rng.uniform(40, 100) * np.exp(-0.5 * (((i - ci) / si) ** 2 + ((j - cj) / sj) ** 2))
    layer = (100.0 * np.tanh(z / 100.0)).astype(np.float32)
    layer[rng.integers(0, rows, 12), rng.integers(0, cols, 12)] = np.nan
    return layer


def numpy_map_risk(g, layers, poses, probes, states, S):
    """The header's definition on stored rollout states (B, S, N, 4): step_hits, unknown_hits (B, N), and per solve the share, the
    unknown share, the worst occupancy, its row and its entry."""
    B, _, N, _ = states.shape
    nl, nw = probes
    a = np.array([-0.5 * SAFE[0] + k * (SAFE[0] / (nl - 1)) if nl > 1 else 0.0 for k in range(nl)])
    b = np.array([-0.5 * SAFE[1] + l * (SAFE[1] / (nw - 1)) if nw > 1 else 0.0 for l in range(nw)])
    a, b = np.repeat(a, nw), np.tile(b, nl)
    x_first, y_first, inv = g.pos_x + (0.5 * g.len_x - 0.5 * g.res), g.pos_y + (0.5 * g.len_y - 0.5 * g.res), 1.0 / g.res
    hits, unk, out = np.zeros((B, N), dtype=np.int32), np.zeros((B, N), dtype=np.int32), np.zeros((B, 5))
    for s in range(B):
        x, y, th = states[s, :, :, 0:1], states[s, :, :, 1:2], states[s, :, :, 3:4]
        ct, st = np.cos(th), np.sin(th)
        dx, dy = x + (a * ct - b * st) - poses[s][0], y + (a * st + b * ct) - poses[s][1]
        cp, sp = np.cos(poses[s][2]), np.sin(poses[s][2])
        fi, fj = (x_first - (cp * dx + sp * dy)) * inv, (y_first - (cp * dy - sp * dx)) * inv
        inside = (fi >= 0.0) & (fj >= 0.0) & (fi < g.rows - 1.0) & (fj < g.cols - 1.0)
        i0, j0 = np.where(inside, fi, 0.0).astype(np.int64), np.where(inside, fj, 0.0).astype(np.int64)
        ti, tj = fi - i0, fj - j0
        lay = layers[s].astype(np.float64)
        f00, f10, f01, f11 = lay[i0, j0], lay[i0 + 1, j0], lay[i0, j0 + 1], lay[i0 + 1, j0 + 1]
        ok = inside & np.isfinite(f00) & np.isfinite(f10) & np.isfinite(f01) & np.isfinite(f11)
        with np.errstate(invalid="ignore"):
            a0, a1 = f00 + ti * (f10 - f00), f01 + ti * (f11 - f01)
            occ = np.where(ok, a0 + tj * (a1 - a0), -np.inf)          # (S, N, P)
        hit, unknown = (occ > THRESHOLD).any(axis=2), (~ok).any(axis=2)
        hits[s], unk[s] = hit.sum(axis=0), unknown.sum(axis=0)
        flat = occ.transpose(0, 2, 1).reshape(S, -1)                   # entry q*N + t
        row = int(flat.max(axis=1).argmax())
        out[s] = (hit.any(axis=1).sum() / S, unknown.any(axis=1).sum() / S, flat[row].max(), row, int(flat[row].argmax()))
    return hits, unk, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--check", type=int, default=32, help="solves whose stored rollouts numpy reduces before timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, S, N, M = args.batch, args.samples, 50, 4
    Bp, Sp = 16, 1024  # the planner's shape
    Bc = min(args.check, B)
    p = cilqr_amd.default_params(N)
    p.safe_length, p.safe_width = SAFE
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=max(B, Bp * (Sp // 256)), max_horizon=N, max_obstacles=M, device=0)
    g = cilqr_amd.map_geom(*GEOM)
    kinds = [smooth_layer(g.rows, g.cols, seed) for seed in range(1, 9)]  # per solve: layer b % 8, pose shifted with b % 8
    layers = [kinds[b % 8] for b in range(B)]
    poses = np.array([(POSE[0] + 0.05 * (b % 8), POSE[1] - 0.03 * (b % 8), POSE[2] + 0.004 * (b % 8)) for b in range(B)])
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    flat = lambda a: np.asfortranarray(a).flatten(order="F")  # noqa: E731  (column-major: i is contiguous)
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
             delta=dv(scenes.pose_offsets(S, 0.16, 0.16, 0.017, seed=5)), deltap=dv(scenes.pose_offsets(Sp, 0.16, 0.16, 0.017, seed=5)),
             shared=dv(flat(kinds[0])), layers=dv(np.stack([flat(a) for a in layers])), poses=dv(poses))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32), Xr=zeros(Bc * S, 4 * (N + 1)), Ur=zeros(Bc * S, 2 * N),
             frisk=zeros(B, cilqr_amd.ROLLOUT_RISK_FIELDS), fhits=zeros(B, N, dtype=torch.int32), ftotal=zeros(B),
             mrisk=zeros(B, cilqr_amd.MAP_RISK_FIELDS), mhits=zeros(B, N, dtype=torch.int32), munk=zeros(B, N, dtype=torch.int32), mtotal=zeros(B))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)

    def set_map(per_solve, probes=(3, 3)):
        if per_solve:
            s.set_uncertainty_map_device(ptr["layers"], g, (0.0, 0.0, 0.0), probes, layer_stride=g.rows * g.cols, poses_ptr=ptr["poses"])
        else:
            s.set_uncertainty_map_device(ptr["shared"], g, POSE, probes)

    def solve():
        s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"],
                             ptr["it"], ptr["st"])

    def gains():
        s.gains_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"],
                             ptr["K"], ptr["ok"], lamb=1.0)

    def obstacle_risk(b=B, n_s=S, delta="delta"):
        s.rollout_risk_device(stream, b, N, M, n_s, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr[delta], 0, ptr["pose"], ptr["dim"], strides,
                              ptr["frisk"], ptr["fhits"], ptr["ftotal"], ptr["J"], k_scale=0.0, max_risk=0.05)

    def map_risk(b=B, n_s=S, delta="delta"):
        s.rollout_risk_map_device(stream, b, N, n_s, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr[delta], 0, THRESHOLD, ptr["mrisk"],
                                  ptr["mhits"], ptr["munk"], ptr["mtotal"], ptr["ftotal"], k_scale=0.0, max_risk=0.05)

    # (name, per-solve map, probes, launch)
    steps = [("obstacle rollout_risk", None, None, obstacle_risk),
             ("map risk, shared map, 3x3", False, (3, 3), map_risk),
             ("map risk, per-solve, 3x3", True, (3, 3), map_risk),
             ("map risk, shared map, 1x1", False, (1, 1), map_risk),
             ("obstacle risk, B=%d S=%d" % (Bp, Sp), None, None, lambda: obstacle_risk(Bp, Sp, "deltap")),
             ("map risk 3x3, B=%d S=%d" % (Bp, Sp), False, (3, 3), lambda: map_risk(Bp, Sp, "deltap"))]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    set_map(False)
    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        t["U"].copy_(t["U0"])
        solve()
        gains()
        for _, per_solve, probes, f in steps:
            if probes:
                set_map(per_solve, probes)
            f()
        set_map(False)
    torch.cuda.synchronize()
    # ---- agreement with a numpy reduction of the stored rollouts of the first Bc solves, before anything is timed
    s.rollout_batch_device(stream, Bc, N, S, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta"], 0, ptr["Xr"], ptr["Ur"], k_scale=0.0)
    torch.cuda.synchronize()
    states = t["Xr"].cpu().numpy().reshape(Bc, S, N + 1, 4)[:, :, :N]
    assert np.isfinite(states).all() and np.isfinite(t["Ur"].cpu().numpy()).all()
    shares = {}
    for per_solve in (False, True):
        set_map(per_solve)
        map_risk()
        torch.cuda.synchronize()
        r, h, u = t["mrisk"].cpu().numpy(), t["mhits"].cpu().numpy(), t["munk"].cpu().numpy()
        wh, wu, w = numpy_map_risk(g, layers if per_solve else [kinds[0]] * Bc, poses if per_solve else [POSE] * Bc, (3, 3), states, S)
        what = "per-solve maps" if per_solve else "shared map"
        assert np.array_equal(h[:Bc], wh) and np.array_equal(u[:Bc], wu), "step counts differ from the stored rollouts' (%s)" % what
        assert np.array_equal(r[:Bc, cilqr_amd.MR_COLLISION], w[:, 0]) and np.array_equal(r[:Bc, cilqr_amd.MR_UNKNOWN], w[:, 1]), what
        assert np.max(np.abs(r[:Bc, cilqr_amd.MR_WORST_OCC] - w[:, 2])) <= 1e-9, "worst occupancy differs (%s)" % what
        assert np.array_equal(r[:Bc, cilqr_amd.MR_WORST_ROW], w[:, 3]) and np.array_equal(r[:Bc, cilqr_amd.MR_WORST_ENTRY], w[:, 4]), what
        shares[per_solve] = (r[:, cilqr_amd.MR_COLLISION].copy(), r[:, cilqr_amd.MR_UNKNOWN].copy(), int(np.isnan(t["mtotal"].cpu().numpy()).sum()))
    set_map(False)
    first = None
    times = {name: [] for name in ("solve",) + tuple(st[0] for st in steps)}
    same = True
    for _ in range(args.rounds):
        t["U"].copy_(t["U0"])
        torch.cuda.synchronize()
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        times["solve"].append(e0.elapsed_time(e1))
        gains()
        for name, per_solve, probes, f in steps:
            if probes:
                set_map(per_solve, probes)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.reps)
            if name == steps[1][0]:
                if first is None:
                    first = t["mrisk"].clone()
                same = same and torch.equal(t["mrisk"].view(torch.int64), first.view(torch.int64))
        set_map(False)
    ok = t["ok"].cpu().numpy()
    lines = ["map rollout-risk launch beside the solve launch and the obstacle rollout-risk launch of the same batch: device events, %d "
             "alternated rounds, one process" % args.rounds,
             "config-2 scenes: B=%d, N=%d, M=%d static obstacles (dense tables), S=%d start offsets shared by the batch (%d rows); map %d x %d "
             "cells of %.1f m, threshold %g; solve with the shared map set, on %d lanes per solve, %d wavefront(s)"
             % (B, N, M, S, B * S, g.rows, g.cols, g.res, THRESHOLD, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M)),
             "counts, shares, worst rows and entries equal to a numpy reduction of the stored rollouts of the first %d solves (shared and "
             "per-solve maps), worst occupancy within 1e-9: asserted before timing" % Bc,
             "   solve launch, ms                                  %s" % spread(times["solve"])]
    ms, ob = median(times["solve"]), median(times[steps[0][0]])
    for name, _, _, _ in steps[:4]:
        lines.append("   %-26s ms (%2d per window)     %s   = %.3f of the solve launch, %.2f x the obstacle risk launch"
                     % (name + ",", args.reps, spread(times[name]), median(times[name]) / ms, median(times[name]) / ob))
    obp = median(times[steps[4][0]])
    for name, _, _, _ in steps[4:]:
        lines.append("   %-26s ms (%2d per window)     %s   = %.2f x the obstacle risk launch of that shape"
                     % (name + ",", args.reps, spread(times[name]), median(times[name]) / obp))
    lines.append("   map risk rows bit-identical over the rounds: %s; gains ok on %d of %d solves" % (same, int(ok.sum()), B))
    for per_solve in (False, True):
        sh, un, rej = shares[per_solve]
        lines.append("   %s: solves with share 0: %d, with 0 < share < 1: %d, with share 1: %d; with unknown rows: %d; NaN totals at "
                     "max_risk 0.05 (the obstacles' included): %d of %d" % ("per-solve maps" if per_solve else "shared map    ", int((sh == 0).sum()),
                                                                         int(((sh > 0) & (sh < 1)).sum()), int((sh == 1).sum()), int((un > 0).sum()), rej, B))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
