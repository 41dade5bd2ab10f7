#!/usr/bin/env python3
"""The distance field, the inflation and the map clearance (cilqr_map_distance_device, cilqr_inflate_map_device,
cilqr_map_clearance_device) beside the map products and checks they stand next to — the cilqr_tighten_map launch, the footprint check
and the solve with the map set — in one process, alternated round by round so that all see the same clocks and neighbours:

  config-2 scenes   N = 50, M = 4 static obstacles, the node's 150 x 100 map (15 m x 10 m at 0.1 m, probes 3 x 3) shared by the batch,
                    seeds above 50;
                    the distance call at L = 1, 16 and 1024 layers of that map and at L = 1 on a 1024 x 1024 map  |  the inflate launch
                    (inscribed 0.3 m, radius 1.5 m, peak 100) at L = 1 and 1024  |  the clearance call at B = 16 and 1024 (reach 1 m)
                    |  the tighten-map launch (kappa 1.645, max_inflate 1.0)  |  the footprint check (M = 4 and the map)  |  the solve

Times are device events.  Every launch is timed TWICE per round, as an A/A pair ("a" and "b" below) at different places of the round:
the difference of the two medians is what this method cannot tell apart.  The short launches are timed --reps back to back and divided
by their number, the solve one per window from the cold warm start.  Nothing is promised in advance: the file reports the medians.

    python tools/map_distance_ab.py [--rounds R] [--reps K] [--out profiles/r23_map_distance.txt]
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
from tighten_map_ab import CAP, GEOM, KAPPA, POSE, SIGMA0, dv, timed, zeros  # noqa: E402

THRESHOLD, REACH, INSCRIBED, RADIUS, PEAK = 50.0, 1.0, 0.3, 1.5, 100.0


def flat(layer):
    return torch.from_numpy(np.ascontiguousarray(np.asfortranarray(layer).flatten(order="F"))).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, M, Bp, Lm = 1024, 50, 4, 16, 16
    p = cilqr_amd.default_params(N)
    p.safe_length, p.safe_width = SAFE
    sc = scenes.make_c2(B, p)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=M, device=0)
    g = cilqr_amd.map_geom(*GEOM)
    cells = g.rows * g.cols
    big = cilqr_amd.map_geom(102.4, 102.4, 0.1, 0.0, 0.0)
    big_cells = big.rows * big.cols
    layer, big_layer = smooth_layer(g.rows, g.cols, 1), smooth_layer(big.rows, big.cols, 2)
    t = dict(x0=dv(sc["x0"]), U0=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]), s0=dv(SIGMA0),
             layer=flat(layer), layers=flat(layer).repeat(B), big=flat(big_layer))
    t["U"] = t["U0"].clone()
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32),
             k=zeros(B, 2 * N), K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32), crisk=zeros(B, cilqr_amd.CHANCE_FIELDS),
             csig=zeros(B, N + 1, 16), tight=zeros(B, cells, dtype=torch.float32), tm=zeros(B, cilqr_amd.TIGHTEN_MAP_FIELDS),
             d2=zeros(B, cells, dtype=torch.int32), dist=zeros(B, cells, dtype=torch.float32), soft=zeros(B, cells, dtype=torch.float32),
             big_d2=zeros(big_cells, dtype=torch.int32), big_dist=zeros(big_cells, dtype=torch.float32),
             mc=zeros(B, cilqr_amd.MAP_CLEARANCE_FIELDS), mstep=zeros(B, N), fp=zeros(B, cilqr_amd.FOOTPRINT_FIELDS), fstep=zeros(B, N))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)

    def solve(b=B):
        s.solve_batch_device(stream, b, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"], ptr["it"],
                             ptr["st"])

    def distance(L):
        s.map_distance_device(stream, L, ptr["layers"], cells, g, THRESHOLD, ptr["d2"], ptr["dist"])

    def distance_big():
        s.map_distance_device(stream, 1, ptr["big"], 0, big, THRESHOLD, ptr["big_d2"], ptr["big_dist"])

    def inflate(L):
        s.inflate_map_device(stream, L, ptr["layers"], cells, g, ptr["d2"], INSCRIBED, RADIUS, PEAK, ptr["soft"])

    def clearance(b):
        s.map_clearance_device(stream, b, N, 1, ptr["X"], ptr["mc"], REACH, occ_threshold=THRESHOLD, step_clearance=ptr["mstep"])

    def footprint(b):
        s.footprint_check_device(stream, b, N, M, 1, ptr["X"], ptr["pose"], ptr["dim"], strides, ptr["fp"], occ_threshold=THRESHOLD, step_clearance=ptr["fstep"])

    def tighten(b):
        s.tighten_map_device(stream, b, N, ptr["X"], ptr["csig"], ptr["tight"], ptr["tm"], kappa=KAPPA, max_inflate=CAP)

    s.set_uncertainty_map_device(ptr["layer"], g, POSE, (3, 3))
    launches = [("map_distance, L=1", lambda: distance(1)), ("map_distance, L=%d" % Lm, lambda: distance(Lm)), ("map_distance, L=%d" % B, lambda: distance(B)),
                ("map_distance, L=1, %d x %d" % (big.rows, big.cols), distance_big),
                ("inflate_map, L=1", lambda: inflate(1)), ("inflate_map, L=%d" % B, lambda: inflate(B)),
                ("map_clearance, B=%d" % Bp, lambda: clearance(Bp)), ("map_clearance, B=%d" % B, lambda: clearance(B)),
                ("footprint_check, B=%d" % Bp, lambda: footprint(Bp)), ("footprint_check, B=%d" % B, lambda: footprint(B)),
                ("tighten_map, B=%d" % Bp, lambda: tighten(Bp)), ("tighten_map, B=%d" % B, lambda: tighten(B))]

    def prepare():  # the plan of a fresh first solve, its gains and Sigma_t
        t["U"].copy_(t["U0"])
        solve()
        s.gains_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"], ptr["K"], ptr["ok"], lamb=1.0)
        s.chance_risk_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, 0, ptr["pose"], ptr["dim"], strides, ptr["crisk"], sigma_out=ptr["csig"])

    for _ in range(3):  # warm-up of every launch: code objects loaded, the solve's schedule hint built
        prepare()
        for _, f in launches:
            f()
    torch.cuda.synchronize()
    times = {(n, ab): [] for n, _ in launches + [("solve, B=%d" % B, None)] for ab in "ab"}
    first, same = None, True
    for _ in range(args.rounds):
        for ab, order in (("a", launches), ("b", launches[::-1])):
            t["U"].copy_(t["U0"])
            times[("solve, B=%d" % B, ab)].append(timed(solve))
            prepare()
            for name, f in order:
                times[(name, ab)].append(timed(f, args.reps))
        distance(Lm)
        clearance(B)
        torch.cuda.synchronize()
        now = (t["d2"][:Lm].clone(), t["mc"].clone())
        first = now if first is None else first
        same = same and torch.equal(now[0], first[0]) and torch.equal(now[1].view(torch.int64), first[1].view(torch.int64))
    d2, mc = t["d2"][0].cpu().numpy(), t["mc"].cpu().numpy()
    seeds = int((d2 == 0).sum())
    lines = ["distance field, inflation and map clearance beside the tighten-map launch, the footprint check and the solve with the map set: device "
             "events, %d alternated rounds, one process; every launch timed twice per round (a, b): an A/A pair" % args.rounds,
             "config-2 scenes: N=%d, M=%d static obstacles; map %d x %d at %.1f m shared by the batch, probes 3 x 3; seeds above %.0f: %d of %d cells "
             "(%d of %d on the %d x %d map); reach %.1f m; inscribed %.1f m, radius %.1f m, peak %.0f"
             % (N, M, g.rows, g.cols, g.res, THRESHOLD, seeds, cells, int((t["big_d2"] == 0).sum()), big_cells, big.rows, big.cols, REACH, INSCRIBED, RADIUS, PEAK)]
    ms = median(times[("solve, B=%d" % B, "a")] + times[("solve, B=%d" % B, "b")])
    for name in ["solve, B=%d" % B] + [n for n, _ in launches]:
        reps = 1 if name.startswith("solve") else args.reps
        a, b = times[(name, "a")], times[(name, "b")]
        lines.append("   %-34s ms (%2d per window)   a: %s   b: %s   a/b medians differ by %.1f %%   = %.4f of the solve"
                     % (name + ",", reps, spread(a), spread(b), 100.0 * abs(median(a) - median(b)) / max(median(a), median(b)), median(a + b) / ms))
    fin = mc[:, 0][np.isfinite(mc[:, 0])]
    lines.append("   d2 of the %d layers and the clearance rows bit-identical over the rounds: %s; largest d2 %d cells^2; B=%d: clearance %.3f .. %.3f m over %d "
                 "rows with a seed within reach, %d rows without" % (Lm, same, int(d2[d2 < 2 ** 31 - 1].max()), B, fin.min() if fin.size else float("nan"),
                                                                      fin.max() if fin.size else float("nan"), fin.size, int(np.isposinf(mc[:, 0]).sum())))
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
