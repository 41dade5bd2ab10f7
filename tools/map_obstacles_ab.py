#!/usr/bin/env python3
"""The component labelling (cilqr_map_obstacles_device) beside the call that precedes it (cilqr_map_distance_device) and beside what it
replaces on the way to the solve — the page-locked upload of K host-made obstacle rows — in one process, alternated round by round so
that all see the same clocks and neighbours:

  the node's 150 x 100 map (15 m x 10 m at 0.1 m), five soft bumps, seeds above 50, gap2 = 1, min_cells 3, K = 16, no size limit:
  the obstacles call at L = 1, 16 and 1024 layers of that map and at L = 1 on a 1024 x 1024 map  |  the distance call at the same four
  sizes  |  the upload of K rows (pose and dim tables, 6 doubles a row) from page-locked memory

Times are device events.  Every launch is timed TWICE per round, as an A/A pair ("a" and "b" below) at different places of the round:
the difference of the two medians is what this method cannot tell apart.  Each is timed --reps back to back and divided by their number.
Nothing is promised in advance: the file reports the medians, and the distance call of the same run is the yardstick.

    python tools/map_obstacles_ab.py [--rounds R] [--reps K] [--out profiles/r25_map_obstacles.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from map_distance_ab import THRESHOLD, flat  # noqa: E402
from risk_map_ab import median, smooth_layer, spread  # noqa: E402
from tighten_map_ab import GEOM, POSE, timed, zeros  # noqa: E402

GAP2, MIN_CELLS, K = 1, 3, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, Lm = 1024, 16
    s = cilqr_amd.Solver(cilqr_amd.default_params(50), max_batch=64, max_horizon=50, max_obstacles=4, device=0)
    g = cilqr_amd.map_geom(*GEOM)
    cells = g.rows * g.cols
    big = cilqr_amd.map_geom(102.4, 102.4, 0.1, 0.0, 0.0)
    big_cells = big.rows * big.cols
    layer, big_layer = smooth_layer(g.rows, g.cols, 1), smooth_layer(big.rows, big.cols, 2)
    i32 = dict(dtype=torch.int32)
    t = dict(layers=flat(layer).repeat(B), big=flat(big_layer), pose=torch.tensor(POSE, dtype=torch.float64).cuda(),
             d2=zeros(B, cells, **i32), work=zeros(B, cells, **i32), label=zeros(B, cells, **i32), n=zeros(B, 4, **i32),
             comp=zeros(B, K, cilqr_amd.MAP_OBSTACLE_FIELDS), boxes=zeros(B, K, 5), opose=zeros(B, K, 4), odim=zeros(B, K, 2),
             big_d2=zeros(big_cells, **i32), big_work=zeros(big_cells, **i32), big_label=zeros(big_cells, **i32), rows=zeros(K, 6))
    host_rows = cilqr_amd.pinned_empty((K, 6))
    host_rows[...] = 1.0
    pinned = torch.from_numpy(host_rows)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}

    def distance(L):
        s.map_distance_device(stream, L, ptr["layers"], cells, g, THRESHOLD, ptr["d2"])

    def distance_big():
        s.map_distance_device(stream, 1, ptr["big"], 0, big, THRESHOLD, ptr["big_d2"])

    def obstacles(L):
        s.map_obstacles_device(stream, L, ptr["d2"], g, K, ptr["work"], ptr["label"], ptr["n"], ptr["comp"], ptr["boxes"], ptr["opose"], ptr["odim"],
                               gap2=GAP2, pose=ptr["pose"], pose_stride=0, min_cells=MIN_CELLS)

    def obstacles_big():
        s.map_obstacles_device(stream, 1, ptr["big_d2"], big, K, ptr["big_work"], ptr["big_label"], ptr["n"], ptr["comp"], ptr["boxes"], ptr["opose"],
                               ptr["odim"], gap2=GAP2, min_cells=MIN_CELLS)

    def upload():
        t["rows"].copy_(pinned, non_blocking=True)

    launches = [("map_obstacles, L=1", lambda: obstacles(1)), ("map_obstacles, L=%d" % Lm, lambda: obstacles(Lm)), ("map_obstacles, L=%d" % B, lambda: obstacles(B)),
                ("map_obstacles, L=1, %d x %d" % (big.rows, big.cols), obstacles_big),
                ("map_distance, L=1", lambda: distance(1)), ("map_distance, L=%d" % Lm, lambda: distance(Lm)), ("map_distance, L=%d" % B, lambda: distance(B)),
                ("map_distance, L=1, %d x %d" % (big.rows, big.cols), distance_big),
                ("upload of %d rows, page-locked" % K, upload)]
    distance(B)
    distance_big()
    for _ in range(3):  # warm-up of every launch: code objects loaded
        for _, f in launches:
            f()
    torch.cuda.synchronize()
    times = {(n, ab): [] for n, _ in launches for ab in "ab"}
    first, same = None, True
    for _ in range(args.rounds):
        for ab, order in (("a", launches), ("b", launches[::-1])):
            for name, f in order:
                times[(name, ab)].append(timed(f, args.reps))
        obstacles(Lm)
        torch.cuda.synchronize()
        now = (t["label"][:Lm].clone(), t["n"][:Lm].clone(), t["comp"][:Lm].clone(), t["boxes"][:Lm].clone())
        first = now if first is None else first
        same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, first))
    n = t["n"][0].cpu().numpy()
    obstacles_big()
    torch.cuda.synchronize()
    n_big = t["n"][0].cpu().numpy()
    lines = ["component labelling beside the distance call in front of it and the upload of K host-made rows: device events, %d alternated rounds, one "
             "process; every launch timed twice per round (a, b): an A/A pair" % args.rounds,
             "map %d x %d at %.1f m, seeds above %.0f, gap2 %d, min_cells %d, K %d, no size limit: %d components, %d of min_cells, %d rows, %d seeds "
             "(%d x %d: %d components, %d of min_cells, %d rows, %d seeds)"
             % (g.rows, g.cols, g.res, THRESHOLD, GAP2, MIN_CELLS, K, n[0], n[1], n[2], n[3], big.rows, big.cols, n_big[0], n_big[1], n_big[2], n_big[3])]
    yard = {}
    for name in [nm for nm, _ in launches]:
        a, b = times[(name, "a")], times[(name, "b")]
        key = name.split(", ", 1)[1] if ", " in name else None
        if name.startswith("map_distance"):
            yard[key] = median(a + b)
        lines.append("   %-36s ms (%2d per window)   a: %s   b: %s   a/b medians differ by %.1f %%"
                     % (name + ",", args.reps, spread(a), spread(b), 100.0 * abs(median(a) - median(b)) / max(median(a), median(b))))
    for name in [nm for nm, _ in launches if nm.startswith("map_obstacles")]:
        key = name.split(", ", 1)[1]
        m = median(times[(name, "a")] + times[(name, "b")])
        lines.append("   %-36s %.4f ms = %.2f of the distance call of the same size (%.4f ms)" % (name + ":", m, m / yard[key], yard[key]))
    lines.append("   labels, n_out, comp and boxes of the %d layers bit-identical over the rounds: %s" % (Lm, same))
    lines.append("   where the time goes inside the call's seven launches was not measured")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
