#!/usr/bin/env python3
"""The map tightening launch (cilqr_tighten_map_device) beside the chance-risk launch that feeds it and beside the solve with the map
set, and one full round of the loop beside the first solve — in one process, alternated round by round so that all see the same clocks
and neighbours:

  config-2 scenes   N = 50, M = 4 static obstacles, the node's 150 x 100 map (15 m x 10 m at 0.1 m, probes 3 x 3) shared by the batch,
                    Sigma_0 = diag(0.16^2, 0.16^2, 0, 0.017^2), no process noise, kappa = 1.645, max_inflate = 1.0, at B = 1024 and at
                    the planner's B = 16:
                    the tighten-map launch  |  the chance launch (sigma_out)  |  the solve with the map set
                    round = gains + chance risk (sigma_out) + tighten_map + the per-solve layers set + re-solve from the first solve's
                    U + the shared map set again, beside the first solve

Times are device events; the short launches are timed --reps back to back and divided by their number, solves and rounds one per window
(each from the cold warm start).  Nothing is promised in advance: the file reports the medians.

    python tools/tighten_map_ab.py [--rounds R] [--reps K] [--out profiles/r17_tighten_map.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from cilqr_amd import scenes  # noqa: E402
from risk_map_ab import SAFE, median, smooth_layer, spread  # noqa: E402

SIGMA0 = np.diag([0.16 ** 2, 0.16 ** 2, 0.0, 0.017 ** 2]).reshape(16)
KAPPA, CAP = 1.645, 1.0
GEOM, POSE = (15.0, 10.0, 0.1, 7.5, 0.0), (-1.0, 0.4, 0.05)  # the node's local map: 150 x 100 cells ahead of the vehicle

dv = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731


def timed(f, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, M, Bp = args.batch, 50, 4, 16
    p = cilqr_amd.default_params(N)
    p.safe_length, p.safe_width = SAFE
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    g = cilqr_amd.map_geom(*GEOM)
    cells = g.rows * g.cols
    layer = smooth_layer(g.rows, g.cols, 1)
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]), s0=dv(SIGMA0),
             layer=torch.from_numpy(np.ascontiguousarray(np.asfortranarray(layer).flatten(order="F"))).cuda())
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32), crisk=zeros(B, cilqr_amd.CHANCE_FIELDS),
             csig=zeros(B, N + 1, 16), tight=zeros(B, cells, dtype=torch.float32), tm=zeros(B, cilqr_amd.TIGHTEN_MAP_FIELDS),
             it1=zeros(B, dtype=torch.int32))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)

    def shared_map():
        s.set_uncertainty_map_device(ptr["layer"], g, POSE, (3, 3))

    def solve(b=B):
        s.solve_batch_device(stream, b, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"], ptr["it"],
                             ptr["st"])

    def gains(b=B):
        s.gains_batch_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"], ptr["K"],
                             ptr["ok"], lamb=1.0)

    def chance(b=B):
        s.chance_risk_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, 0, ptr["pose"], ptr["dim"], strides, ptr["crisk"],
                             sigma_out=ptr["csig"])

    def tighten(b=B):
        s.tighten_map_device(stream, b, N, ptr["X"], ptr["csig"], ptr["tight"], ptr["tm"], kappa=KAPPA, max_inflate=CAP)

    def one_round(b=B):
        gains(b)
        chance(b)
        tighten(b)
        s.set_uncertainty_map_device(ptr["tight"], g, POSE, (3, 3), layer_stride=cells)
        solve(b)
        shared_map()

    shared_map()
    launches = [("tighten_map", tighten), ("chance_risk, sigma_out", chance), ("gains", gains),
                ("tighten_map, B=%d" % Bp, lambda: tighten(Bp)), ("chance_risk, B=%d, sigma_out" % Bp, lambda: chance(Bp)),
                ("gains, B=%d" % Bp, lambda: gains(Bp))]
    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        for b in (B, Bp):
            t["U"].copy_(t["U0"])
            solve(b)
            one_round(b)
    torch.cuda.synchronize()
    names = ["solve", "round", "solve, B=%d" % Bp, "round, B=%d" % Bp] + [n for n, _ in launches]
    times = {n: [] for n in names}
    first, same = None, True
    iters = {}
    for _ in range(args.rounds):
        for b, tag in ((B, ""), (Bp, ", B=%d" % Bp)):
            t["U"].copy_(t["U0"])
            times["solve" + tag].append(timed(lambda: solve(b)))
            t["it1"].copy_(t["it"])
            times["round" + tag].append(timed(lambda: one_round(b)))
            iters[b] = (t["it1"][:b].cpu().numpy().copy(), t["it"][:b].cpu().numpy().copy())
        # the short launches, on the plan of a fresh first solve
        t["U"].copy_(t["U0"])
        solve()
        gains()
        chance()
        for name, f in launches:
            times[name].append(timed(f, args.reps))
        tighten()
        torch.cuda.synchronize()
        if first is None:
            first = (t["tm"].clone(), t["tight"].clone())
        same = same and torch.equal(t["tm"].view(torch.int64), first[0].view(torch.int64)) and torch.equal(t["tight"].view(torch.int32), first[1].view(torch.int32))
    tm = t["tm"].cpu().numpy()
    lines = ["map tightening (cilqr_tighten_map_device) beside the chance-risk and gains launches and the solve of the same batch with the map set: "
             "device events, %d alternated rounds, one process" % args.rounds,
             "config-2 scenes: N=%d, M=%d static obstacles; map %d x %d at %.1f m shared by the batch, probes 3 x 3; one shared Sigma_0, no process "
             "noise, kappa %.3f, max_inflate %.1f; %d workgroups per solve" % (N, M, g.rows, g.cols, g.res, KAPPA, CAP, min((cells + 255) // 256, 64))]
    for b, tag in ((B, ", B=%d" % B), (Bp, ", B=%d" % Bp)):
        key = "" if b == B else tag
        ms, mr = median(times["solve" + key]), median(times["round" + key])
        lines.append("   %-36s ms (1 per window)      %s" % ("first solve" + tag + ",", spread(times["solve" + key])))
        lines.append("   %-36s ms (1 per window)      %s   = %.3f of the first solve; iterations: first solve mean %.2f max %d, re-solve mean %.2f max %d"
                     % ("round" + tag + ",", spread(times["round" + key]), mr / ms, iters[b][0].mean(), iters[b][0].max(), iters[b][1].mean(), iters[b][1].max()))
    for i, (name, _) in enumerate(launches):
        ms = median(times["solve" if i < 3 else "solve, B=%d" % Bp])
        lines.append("   %-36s ms (%2d per window)     %s   = %.4f of the first solve of that batch" % (name + ",", args.reps, spread(times[name]), median(times[name]) / ms))
    lines.append("   tighten rows and layers bit-identical over the rounds: %s; B=%d: cells raised %d .. %d of %d, MAX_REACH %.3f .. %.3f m, capped cells %d, "
                 "lost steps %d" % (same, B, int(tm[:, 0].min()), int(tm[:, 0].max()), cells, tm[:, 3].min(), tm[:, 3].max(), int(tm[:, 4].sum()), int(tm[:, 5].sum())))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
