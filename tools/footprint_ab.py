#!/usr/bin/env python3
"""The footprint check (cilqr_footprint_check_device: two or three launches) beside the solve, the score launch
(cilqr_score_batch_device) and the map rollout-risk launch at S = 1 (cilqr_rollout_risk_map_device) of the same batch, in one process,
alternated round by round so that all see the same clocks and neighbours:

  config-2 scenes at N = 50, B = 16 (the planner's shape) and B = 1024; M = 4 static obstacles, and M = 30 (the four of the scene
  and 26 more boxes scattered along the road, read by the checks only: the solve keeps its four); the node's 150 x 100 map at
  0.1 m, one layer and pose shared by the batch.

The map is set while the solve runs (the node's situation), so the solve launch is the map-cost instantiation.  Before anything is
timed, the footprint rows of the first --check solves are asserted against the numpy restatement of tests/test_footprint.py
(clearance within 1e-9, every index, count and map field equal).  Times are device events; the launches are short, so a window
holds --reps calls back to back and is divided by their number; the footprint call is timed TWICE per round (an A/A pair: what
the difference of two equal things looks like here).  Nothing is promised in advance: the file reports the medians.

    python tools/footprint_ab.py [--rounds R] [--reps K] [--out profiles/r22_footprint.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402

GEOM, POSE, THRESHOLD = (15.0, 10.0, 0.1, 7.5, 0.0), (-1.0, 0.4, 0.05), 50.5
SAFE = (1.1, 0.9)  # safe_length, safe_width of the launch file


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


def whole_layer(rows, cols, seed):
    """Whole numbers 0 ... 100 in smooth patches and a few unknown cells (no occupancy within 1e-6 of the threshold)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    layer = np.round(50.0 + 50.0 * np.sin(0.13 * i + 1.0) * np.cos(0.11 * j + 2.0)).astype(np.float32)
    layer[rng.integers(0, rows, 12), rng.integers(0, cols, 12)] = np.nan
    return layer


def more_boxes(sc, B, N, M_more, seed):
    """The scene's dense tables (B, 4, 4N) / (B, 4, 2N) with M_more standing boxes behind them, scattered 5 ... 60 m ahead."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pose = np.zeros((B, M_more, N, 4))
    dim = np.zeros((B, M_more, N, 2))
    pose[..., 0] = rng.uniform(5.0, 60.0, (B, M_more, 1))
    pose[..., 1] = rng.uniform(-12.0, 12.0, (B, M_more, 1))
    pose[..., 3] = rng.uniform(-3.0, 3.0, (B, M_more, 1))
    dim[..., 0] = rng.uniform(0.5, 5.0, (B, M_more, 1))
    dim[..., 1] = rng.uniform(0.5, 2.5, (B, M_more, 1))
    return (np.concatenate([sc["obs_pose"], pose.reshape(B, M_more, 4 * N)], axis=1),
            np.concatenate([sc["obs_dim"], dim.reshape(B, M_more, 2 * N)], axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=4, help="solves whose rows the numpy restatement judges before timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, M, M_big = 50, 4, 30
    p = cilqr_amd.default_params(N)
    p.safe_length, p.safe_width = SAFE
    g = cilqr_amd.map_geom(*GEOM)
    layer = whole_layer(g.rows, g.cols, 3)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    d_layer = dv(np.asfortranarray(layer).flatten(order="F"))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = ["footprint check beside the solve, the score launch and the map rollout-risk launch (S = 1) of the same batch: device events, "
             "%d alternated rounds of %d calls per window, one process" % (args.rounds, args.reps),
             "config-2 scenes, N=%d; map %d x %d cells of %.1f m shared by the batch, threshold %g; the footprint call is three launches "
             "(boxes, map, merge) and is timed twice per round (A/A)" % (N, g.rows, g.cols, g.res, THRESHOLD)]
    for B in (16, 1024):
        sc = scenes.make_c2(B, p)
        big_pose, big_dim = more_boxes(sc, B, N, M_big - M, 11)
        s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M_big, device=0)
        t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
                 pose_big=dv(big_pose), dim_big=dv(big_dim), delta=zeros(1, 4))
        t["U"] = t["U0"].clone()
        t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32), k=zeros(B, 2 * N),
                 K=zeros(B, 8 * N), score=zeros(B, cilqr_amd.SCORE_FIELDS), stotal=zeros(B), mrisk=zeros(B, cilqr_amd.MAP_RISK_FIELDS),
                 mtotal=zeros(B), fp=zeros(B, cilqr_amd.FOOTPRINT_FIELDS), fclr=zeros(B, N), focc=zeros(B, N, dtype=torch.float32), ftotal=zeros(B))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        ptr = {k: v.data_ptr() for k, v in t.items()}
        s.set_uncertainty_map_device(d_layer.data_ptr(), g, POSE, (3, 3))

        def solve():
            s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"],
                                 ptr["it"], ptr["st"])

        def score(m=M, pose="pose", dim="dim"):
            s.score_batch_device(stream, B, N, m, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr[pose], ptr[dim], 0, (m * N, N, 1, 0), ptr["score"],
                                 ptr["stotal"], max_collision=1.0)

        def map_risk():
            s.rollout_risk_map_device(stream, B, N, 1, ptr["X"], ptr["U"], ptr["k"], ptr["K"], ptr["delta"], 0, THRESHOLD, ptr["mrisk"], 0, 0,
                                      ptr["mtotal"], ptr["stotal"], k_scale=0.0, max_risk=0.0)

        def footprint(m=M, pose="pose", dim="dim", flags=0):
            s.footprint_check_device(stream, B, N, m, 1, ptr["X"], ptr[pose], ptr[dim], (m * N, N, 1, 0), ptr["fp"], min_clearance=0.0,
                                     occ_threshold=THRESHOLD, flags=flags, base=ptr["stotal"], step_clearance=ptr["fclr"], step_occ=ptr["focc"],
                                     total=ptr["ftotal"])

        big = dict(m=M_big, pose="pose_big", dim="dim_big")
        steps = [("score launch, M=%d" % M, score), ("score launch, M=%d" % M_big, lambda: score(**big)), ("map risk 3x3, S=1", map_risk),
                 ("footprint, M=%d" % M, footprint), ("footprint, M=%d (A/A)" % M, footprint), ("footprint, M=%d" % M_big, lambda: footprint(**big)),
                 ("footprint, M=%d, no map" % M, lambda: footprint(flags=cilqr_amd.FOOTPRINT_SKIP_MAP))]
        for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
            t["U"].copy_(t["U0"])
            solve()
            for _, f in steps:
                f()
        torch.cuda.synchronize()
        # ---- agreement with the numpy restatement on the first solves, before anything is timed
        from test_footprint import CLEARANCE, restate  # noqa: E402  (tests/: the restatement the suite checks on the CPU)
        Bc = min(args.check, B)
        footprint(**big)
        torch.cuda.synchronize()
        got = t["fp"].cpu().numpy()[:Bc]
        umap = dict(g=g, layers=layer, poses=POSE)
        want = restate(p, N, t["X"].cpu().numpy()[:Bc], 1, big_pose[:Bc], big_dim[:Bc], 0.0, 0.0, THRESHOLD, False, False, umap)["fp"]
        fin = np.isfinite(want[:, CLEARANCE])
        assert np.array_equal(got[~fin, CLEARANCE], want[~fin, CLEARANCE]) and np.max(np.abs(got[fin, CLEARANCE] - want[fin, CLEARANCE]), initial=0.0) <= 1e-9
        assert np.array_equal(got[:, 1:], want[:, 1:]), "footprint rows differ from the numpy restatement"
        first, same = None, True
        times = {name: [] for name in ("solve",) + tuple(st[0] for st in steps)}
        for _ in range(args.rounds):
            t["U"].copy_(t["U0"])
            torch.cuda.synchronize()
            e0.record()
            solve()
            e1.record()
            torch.cuda.synchronize()
            times["solve"].append(e0.elapsed_time(e1))
            for name, f in steps:
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.reps)
                if name == steps[3][0]:
                    if first is None:
                        first = t["fp"].clone()
                    same = same and torch.equal(t["fp"].view(torch.int64), first.view(torch.int64))
        footprint()
        torch.cuda.synchronize()
        rows, sc_rows = t["fp"].cpu().numpy(), t["score"].cpu().numpy()
        ms = median(times["solve"])
        lines.append("B=%d, M=%d static obstacles (dense tables); solve with the map set, on %d lanes per solve, %d wavefront(s); rows of the "
                     "first %d solves equal to the numpy restatement at M=%d: asserted before timing" % (B, M, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M), Bc, M_big))
        lines.append("   solve launch, ms                                   %s" % spread(times["solve"]))
        for name, _ in steps:
            lines.append("   %-28s ms (%2d per window)    %s   = %.3f of the solve launch" % (name + ",", args.reps, spread(times[name]), median(times[name]) / ms))
        lines.append("   footprint rows bit-identical over the rounds: %s; plans the score call counts as collisions: %d of %d; with an exact obstacle "
                     "hit: %d; with a map hit: %d; with unknown cells: %d" % (same, int((sc_rows[:, cilqr_amd.SCORE_COLLISION] > 0).sum()), B,
                                                                           int((rows[:, cilqr_amd.FP_HIT_STEPS] > 0).sum()), int((rows[:, cilqr_amd.FP_MAP_HIT_STEPS] > 0).sum()),
                                                                           int((rows[:, cilqr_amd.FP_MAP_UNKNOWN_STEPS] > 0).sum())))
        s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
