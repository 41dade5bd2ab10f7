#!/usr/bin/env python3
"""The score launch (cilqr_score_batch*_device) beside the solve launch of the same batch, in one process, alternated round by
round so that both see the same clocks and the same neighbours:

  config 2   B = 1024, N = 50, M = 4 static obstacles         cilqr_solve_batch_device, then cilqr_score_batch_device
  config 3   B = 4096, N = 50, 8 obstacles x 32 pose samples   cilqr_solve_batch_sampled_device, then cilqr_score_batch_sampled_device

Times are device events.  A solve launch is timed alone (its warm start is restored outside the window); the score launch is a few
tens of microseconds, so a window holds --score-reps launches back to back and is divided by their number.  The expectation this is
read against: the score evaluates every obstacle entry once where the launch-deciding solve evaluates it in up to 20 linearisations
beside its backward and forward passes, so it should take at most a tenth of the solve launch.

    python tools/score_ab.py [--rounds R] [--score-reps K] [--out profiles/r08_score.txt]
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


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def median(ts):
    return sorted(ts)[len(ts) // 2]


def setup(config):
    N = 50
    p = cilqr_amd.default_params(N)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    if config == 2:
        B, M = 1024, 4
        sc = scenes.make_c2(B, p)
        t = dict(pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]))
    else:
        B, n_obs, S = 4096, 8, 32
        M = n_obs * S
        sc = scenes.make_c3(B, p, n_dyn=n_obs, n_samples=S)
        t = dict(pose=dv(sc["nom_pose"]), dim=dv(sc["nom_dim"]), off=dv(sc["offsets"]))
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    t.update(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]))
    t["U"] = t["U0"].clone()
    t["X"] = torch.zeros(B, 4 * (N + 1), dtype=torch.float64, device="cuda")
    t["J"] = torch.zeros(B, dtype=torch.float64, device="cuda")
    t["it"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    t["st"] = torch.zeros(B, dtype=torch.int32, device="cuda")
    t["score"] = torch.zeros(B, cilqr_amd.SCORE_FIELDS, dtype=torch.float64, device="cuda")
    t["total"] = torch.zeros(B, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}

    if config == 2:
        def solve():
            s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"],
                                 ptr["J"], ptr["it"], ptr["st"])

        def score():
            s.score_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, (M * N, N, 1, 0),
                                 ptr["score"], ptr["total"], max_collision=0.0)
        what = "config 2: B=%d, N=%d, M=%d static obstacles (dense tables); solve on %d lanes per solve, %d wavefront(s)" % (
            B, N, M, s.solve_family(B, N, M), s.solve_wavefronts(B, N, M))
    else:
        def solve():
            s.solve_batch_sampled_device(stream, B, N, n_obs, S, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"],
                                         ptr["off"], sc["sample_weight"], ptr["X"], ptr["J"], ptr["it"], ptr["st"])

        def score():
            s.score_batch_sampled_device(stream, B, N, n_obs, S, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"],
                                         ptr["off"], sc["sample_weight"], ptr["score"], ptr["total"], max_collision=0.3)
        what = "config 3: B=%d, N=%d, %d obstacles x %d pose samples (compact form); solve on %d wavefront(s) per solve" % (
            B, N, n_obs, S, s.solve_sampled_wavefronts(B, N, n_obs))
    return s, t, solve, score, what


def run(config, rounds, reps, lines):
    s, t, solve, score, what = setup(config)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):  # warm-up of both launches: code objects loaded, the solve's schedule hint built
        t["U"].copy_(t["U0"])
        solve()
        score()
    torch.cuda.synchronize()
    first = (t["score"].clone(), t["total"].clone())
    t_solve, t_score = [], []
    same = True
    for _ in range(rounds):
        t["U"].copy_(t["U0"])
        torch.cuda.synchronize()
        e0.record()
        solve()
        e1.record()
        torch.cuda.synchronize()
        t_solve.append(e0.elapsed_time(e1))
        e0.record()
        for _ in range(reps):
            score()
        e1.record()
        torch.cuda.synchronize()
        t_score.append(e0.elapsed_time(e1) / reps)
        same = same and torch.equal(t["score"].view(torch.int64), first[0].view(torch.int64))
    total = t["total"].cpu().numpy()
    sc = t["score"].cpu().numpy()
    lines.append(what)
    lines.append("   solve launch, ms                 %s" % spread(t_solve))
    lines.append("   score launch, ms (%2d per window) %s" % (reps, spread(t_score)))
    lines.append("   score / solve (medians)          %.4f   (expectation: at most 0.1)" % (median(t_score) / median(t_solve)))
    lines.append("   scores bit-identical over the rounds: %s; candidates rejected: %d of %d; largest collision share %.4f"
                 % (same, int(np.isnan(total).sum()), len(total), float(sc[:, cilqr_amd.SCORE_COLLISION].max())))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--score-reps", type=int, default=20)
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["score launch beside the solve launch of the same batch: device events, %d alternated rounds, one process" % args.rounds]
    for c in args.configs.split(","):
        run(int(c), args.rounds, args.score_reps, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
