#!/usr/bin/env python3
"""The stop-plan launch (cilqr_stop_plans_device) and the fallback sequence it feeds — stop plans, the footprint check with S = D on
the retimed rows, the argmin over the B*D totals — beside the solve launch and the S = 1 footprint check of the same batch, in one
process, alternated round by round so that all see the same clocks and neighbours:

  config-2 scenes at N = 50; B = 16 with D = 4 and D = 8 braking levels (the planner's shape) and B = 128 with D = 8; M = 4 static
  obstacles; the node's 150 x 100 map at 0.1 m, one layer and pose shared by the batch.

The map is set while the solve runs (the node's situation), so the solve launch is the map-cost instantiation.  Before anything is
timed the rows of the first --check plans are compared with the numpy restatement of tests/test_stop_plans.py, which is why tests/ is on
the path: a sanity check that the launch being timed computes stop plans, not a test of them (that is the suite's).  It looks only at rows
none of whose comparisons the restatement finds within 1e-7 of flipping, asks for at least half of the rows to be such, and leaves the
step of the largest deviation out.  Times are device events; the launches are short, so a window holds --reps calls back to back and is
divided by their number; the stop launch is timed TWICE per round (an A/A pair: what the difference of two equal things looks like
here).  Nothing is promised in advance: the file reports the medians.

    python tools/stop_plans_ab.py [--rounds R] [--reps K] [--out profiles/r24_stop_plans.txt]
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
HOLD, MAX_DEVIATION, WEIGHT = 1, 0.5, 1e6


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=4, help="plans whose rows the numpy restatement judges before timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, M = 50, 4
    p = cilqr_amd.default_params(N)
    p.safe_length, p.safe_width = SAFE
    g = cilqr_amd.map_geom(*GEOM)
    layer = whole_layer(g.rows, g.cols, 3)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    d_layer = dv(np.asfortranarray(layer).flatten(order="F"))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    lines = ["stop plans beside the solve launch and the S = 1 footprint check of the same batch: device events, %d alternated rounds of %d "
             "calls per window, one process" % (args.rounds, args.reps),
             "config-2 scenes, N=%d, M=%d; map %d x %d cells of %.1f m shared by the batch, threshold %g; hold %d; the sequence is the stop "
             "launch, the footprint check with S = D (three launches) and the argmin over B*D totals; the stop launch is timed twice per round (A/A)"
             % (N, M, g.rows, g.cols, g.res, THRESHOLD, HOLD)]
    for B, D in ((16, 4), (16, 8), (128, 8)):
        R = B * D
        levels = np.linspace(1.03, 5.5, D)
        sc = scenes.make_c2(B, p)
        s = cilqr_amd.Solver(p, max_batch=R, max_horizon=N, max_obstacles=M, device=0)
        t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]), lv=dv(levels))
        t["U"] = t["U0"].clone()
        t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
                 fp=zeros(B, cilqr_amd.FOOTPRINT_FIELDS), ftotal=zeros(B), Xs=zeros(R, 4 * (N + 1)), Us=zeros(R, 2 * N), sp=zeros(R, cilqr_amd.STOP_FIELDS),
                 cost=zeros(R), fps=zeros(R, cilqr_amd.FOOTPRINT_FIELDS), stotal=zeros(R), pair=zeros(2))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        ptr = {k: v.data_ptr() for k, v in t.items()}
        s.set_uncertainty_map_device(d_layer.data_ptr(), g, POSE, (3, 3))

        def solve():
            s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"],
                                 ptr["it"], ptr["st"])

        def footprint():
            s.footprint_check_device(stream, B, N, M, 1, ptr["X"], ptr["pose"], ptr["dim"], (M * N, N, 1, 0), ptr["fp"], occ_threshold=THRESHOLD,
                                     base=ptr["J"], total=ptr["ftotal"])

        def stop():
            s.stop_plans_device(stream, B, N, D, ptr["X"], ptr["U"], ptr["lv"], ptr["Xs"], ptr["Us"], ptr["sp"], hold=HOLD, max_deviation=MAX_DEVIATION,
                                plan_cost=ptr["J"], decel_weight=WEIGHT, cost=ptr["cost"])

        def sequence():
            stop()
            s.footprint_check_device(stream, B, N, M, D, ptr["Xs"], ptr["pose"], ptr["dim"], (M * N, N, 1, 0), ptr["fps"], occ_threshold=THRESHOLD,
                                     base=ptr["cost"], total=ptr["stotal"])
            s.argmin_device(stream, R, ptr["stotal"], ptr["pair"])

        steps = [("footprint, S=1", footprint), ("stop plans", stop), ("stop plans (A/A)", stop), ("stop + footprint S=D + argmin", sequence)]
        for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
            t["U"].copy_(t["U0"])
            solve()
            for _, f in steps:
                f()
        torch.cuda.synchronize()
        # ---- agreement with the numpy restatement on the first plans, before anything is timed
        from test_stop_plans import EXACT, VALUES, stop_restate  # noqa: E402  (tests/: the restatement the suite checks on the CPU)
        Bc = min(args.check, B)
        X, U, J = (t[k].cpu().numpy() for k in ("X", "U", "J"))
        want = stop_restate(p, N, X[:Bc], U[:Bc], levels, HOLD, MAX_DEVIATION, J[:Bc], WEIGHT)
        got = dict(X=t["Xs"].cpu().numpy()[:Bc * D], U=t["Us"].cpu().numpy()[:Bc * D], sp=t["sp"].cpu().numpy()[:Bc * D])
        ok = want["margin"] > 1e-7  # rows none of whose comparisons is within 1e-7 of flipping (a lost row has none)
        assert ok.sum() * 2 >= ok.size, "fewer than half of the checked rows are decided on these plans"
        for k in ("X", "U"):
            assert np.nanmax(np.abs(got[k][ok] - want[k][ok]), initial=0.0) <= 1e-9, k
        assert np.nanmax(np.abs(got["sp"][ok][:, VALUES] - want["sp"][ok][:, VALUES]), initial=0.0) <= 1e-9
        exact = [f for f in EXACT if f != cilqr_amd.SP_DEVIATION_STEP]  # (that index is decided only where one deviation leads: the suite's test)
        assert np.array_equal(got["sp"][ok][:, exact], want["sp"][ok][:, exact]), "stop rows differ from the numpy restatement"
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
                if name == steps[1][0]:
                    if first is None:
                        first = t["Xs"].clone()
                    same = same and torch.equal(t["Xs"].view(torch.int64), first.view(torch.int64))
        sequence()
        torch.cuda.synchronize()
        sp, total, pair = t["sp"].cpu().numpy(), t["stotal"].cpu().numpy(), t["pair"].cpu().numpy()
        ms = median(times["solve"])
        lines.append("B=%d plans, D=%d levels %.2f ... %.2f m/s^2 (%d rows); solve with the map set, on %d lanes per solve, %d wavefront(s); rows of "
                     "the first %d plans equal to the numpy restatement: asserted before timing" % (B, D, levels[0], levels[-1], R, s.solve_family(B, N, M),
                                                                                                s.solve_wavefronts(B, N, M), Bc))
        lines.append("   solve launch, ms                                       %s" % spread(times["solve"]))
        for name, _ in steps:
            lines.append("   %-32s ms (%2d per window)    %s   = %.3f of the solve launch" % (name + ",", args.reps, spread(times[name]), median(times[name]) / ms))
        lines.append("   stop rows bit-identical over the rounds: %s; rows at rest by step N-1: %d of %d; rows the S = D check lets through: %d; "
                     "pick: row %d (plan %d, level %d)" % (same, int(((sp[:, cilqr_amd.SP_STOP_STEP] >= 0) & (sp[:, cilqr_amd.SP_STOP_STEP] <= N - 1)).sum()), R,
                                                         int(np.isfinite(total).sum()), int(pair[1]), int(pair[1]) // D if pair[1] >= 0 else -1,
                                                         int(pair[1]) % D if pair[1] >= 0 else -1))
        s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
