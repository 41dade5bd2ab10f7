#!/usr/bin/env python3
"""The mover clearing (cilqr_clear_movers_device) beside a launch of the same lane = cell shape (cilqr_inflate_map_device), beside the
tracker tick in front of it (cilqr_track_update_device) and beside what a node without it would do — clear the layer on the host and
upload it from page-locked memory — in one process, alternated round by round so that all see the same clocks and neighbours:

  the node's 150 x 100 map (15 m x 10 m at 0.1 m), five soft bumps, seeds above 50, gap2 = 1, min_cells 3, K = 16, no size limit; every
  second row a mover (mask form: the tracker form differs by the prologue's K loads of a table row), fill 0, owner_out written:
  the clearing at L = 1, 16 and 1024 layers of that map and at L = 1 on a 1024 x 1024 map, each at halo2 = 0, 9 and 1024  |  the
  inflation at the same four sizes  |  one tracker tick, W = 1, M = 16, D = 16  |  the upload of one 150 x 100 layer

Times are device events.  Every launch is timed TWICE per round, as an A/A pair ("a" and "b" below) at different places of the round:
the difference of the two medians is what this method cannot tell apart.  Each is timed --reps back to back and divided by their number.
Nothing is promised in advance: the file reports the medians, and the inflation of the same run is the yardstick.

    python tools/clear_movers_ab.py [--rounds R] [--reps K] [--out profiles/r27_clear_movers.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402
from map_distance_ab import INSCRIBED, PEAK, RADIUS, THRESHOLD, flat  # noqa: E402
from risk_map_ab import median, smooth_layer, spread  # noqa: E402
from tighten_map_ab import GEOM, POSE, dv, timed, zeros  # noqa: E402
from track_update_ab import DT, detections  # noqa: E402

GAP2, MIN_CELLS, K = 1, 3, 16
HALOS = (0, 9, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, Lm = 1024, 16
    s = cilqr_amd.Solver(cilqr_amd.default_params(50), max_batch=64, max_horizon=50, max_obstacles=16, device=0)
    g = cilqr_amd.map_geom(*GEOM)
    cells = g.rows * g.cols
    big = cilqr_amd.map_geom(102.4, 102.4, 0.1, 0.0, 0.0)
    big_cells = big.rows * big.cols
    layer, big_layer = smooth_layer(g.rows, g.cols, 1), smooth_layer(big.rows, big.cols, 2)
    i32, f32 = dict(dtype=torch.int32), dict(dtype=torch.float32)
    mask = torch.tensor([k % 2 for k in range(K)] * B, dtype=torch.int32).cuda()
    t = dict(layers=flat(layer).repeat(B), big=flat(big_layer), pose=torch.tensor(POSE, dtype=torch.float64).cuda(), mask=mask,
             d2=zeros(B, cells, **i32), work=zeros(B, cells, **i32), label=zeros(B, cells, **i32), n=zeros(B, 4, **i32),
             comp=zeros(B, K, cilqr_amd.MAP_OBSTACLE_FIELDS), big_comp=zeros(K, cilqr_amd.MAP_OBSTACLE_FIELDS), out=zeros(B, cells, **f32),
             owner=zeros(B, cells, **i32), fields=zeros(B, cilqr_amd.CLEAR_MOVERS_FIELDS), big_d2=zeros(big_cells, **i32),
             big_work=zeros(big_cells, **i32), big_label=zeros(big_cells, **i32), big_out=zeros(big_cells, **f32), big_owner=zeros(big_cells, **i32),
             one=zeros(cells, **f32))
    host_layer = cilqr_amd.pinned_empty((cells,), np.float32)
    host_layer[...] = 1.0
    pinned = torch.from_numpy(host_layer)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    ptr = {k: v.data_ptr() for k, v in t.items()}
    # what stands in front of the call: the field, the labels and the rows, once
    s.map_distance_device(stream, B, ptr["layers"], cells, g, THRESHOLD, ptr["d2"])
    s.map_obstacles_device(stream, B, ptr["d2"], g, K, ptr["work"], ptr["label"], ptr["n"], ptr["comp"], gap2=GAP2, pose=ptr["pose"], pose_stride=0,
                           min_cells=MIN_CELLS)
    s.map_distance_device(stream, 1, ptr["big"], 0, big, THRESHOLD, ptr["big_d2"])
    s.map_obstacles_device(stream, 1, ptr["big_d2"], big, K, ptr["big_work"], ptr["big_label"], ptr["n"], ptr["big_comp"], gap2=GAP2, min_cells=MIN_CELLS)
    s.map_obstacles_device(stream, B, ptr["d2"], g, K, ptr["work"], ptr["label"], ptr["n"], ptr["comp"], gap2=GAP2, pose=ptr["pose"], pose_stride=0,
                           min_cells=MIN_CELLS)
    torch.cuda.synchronize()

    def clear(L, halo2):
        s.clear_movers_device(stream, L, ptr["layers"], cells, g, ptr["label"], K, ptr["comp"], ptr["out"], ptr["fields"], halo2=halo2, mask=ptr["mask"],
                              owner_out=ptr["owner"])

    def clear_big(halo2):
        s.clear_movers_device(stream, 1, ptr["big"], 0, big, ptr["big_label"], K, ptr["big_comp"], ptr["big_out"], ptr["fields"], halo2=halo2,
                              mask=ptr["mask"], owner_out=ptr["big_owner"])

    def inflate(L):
        s.inflate_map_device(stream, L, ptr["layers"], cells, g, ptr["d2"], INSCRIBED, RADIUS, PEAK, ptr["out"])

    def inflate_big():
        s.inflate_map_device(stream, 1, ptr["big"], 0, big, ptr["big_d2"], INSCRIBED, RADIUS, PEAK, ptr["big_out"])

    filt = cilqr_amd.track_filter(DT, cilqr_amd.white_acceleration_noise(0.5, DT), np.eye(2) * 0.05 ** 2, np.diag([0.05 ** 2, 0.05 ** 2, 16.0, 16.0]),
                                  gate2=9.21, min_hits=2, max_misses=3, v_min=0.5, theta_var_slow=1.0)
    M = D = 16
    k = dict(state=zeros(1, M, cilqr_amd.TRACK_STATE), out=zeros(1, M, cilqr_amd.TRACK_STATE), world=zeros(1, cilqr_amd.TRACK_WORLD_FIELDS),
             track=zeros(1, M, 6), dim=zeros(1, M, 2), cov=zeros(1, M, 16), assign=zeros(1, D, **i32))
    for tick in range(4):
        det = dv(detections(M, D, tick, D)[None])
        s.track_update_device(stream, 1, M, D, det.data_ptr(), filt, k["state"].data_ptr(), k["state"].data_ptr(), k["world"].data_ptr(),
                              k["track"].data_ptr(), k["dim"].data_ptr(), k["cov"].data_ptr(), assign=k["assign"].data_ptr(),
                              flags=cilqr_amd.TRACK_RESET if tick == 0 else 0)
    torch.cuda.synchronize()
    k["det"] = dv(detections(M, D, 4, 3 * D // 4)[None])

    def tick_once():
        s.track_update_device(stream, 1, M, D, k["det"].data_ptr(), filt, k["state"].data_ptr(), k["out"].data_ptr(), k["world"].data_ptr(),
                              k["track"].data_ptr(), k["dim"].data_ptr(), k["cov"].data_ptr(), assign=k["assign"].data_ptr())

    def upload():
        t["one"].copy_(pinned, non_blocking=True)

    sizes = [("L=1", lambda h: clear(1, h), lambda: inflate(1)), ("L=%d" % Lm, lambda h: clear(Lm, h), lambda: inflate(Lm)),
             ("L=%d" % B, lambda h: clear(B, h), lambda: inflate(B)), ("L=1, %d x %d" % (big.rows, big.cols), clear_big, inflate_big)]
    launches = []
    for name, c, _ in sizes:
        for h in HALOS:
            launches.append(("clear_movers, %s, halo2 %d" % (name, h), (lambda c=c, h=h: c(h))))
    launches += [("inflate_map, %s" % name, f) for name, _, f in sizes]
    launches += [("track_update, W=1, M=16, D=16", tick_once), ("upload of one %d x %d layer, page-locked" % (g.rows, g.cols), upload)]
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
        clear(Lm, 9)
        torch.cuda.synchronize()
        now = (t["out"][:Lm].clone(), t["owner"][:Lm].clone(), t["fields"][:Lm].clone())
        first = now if first is None else first
        same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, first))
    fields = t["fields"][0].cpu().numpy()
    n = t["n"][0].cpu().numpy()
    lines = ["mover clearing beside the inflation (the same lane = cell shape), the tracker tick and the upload of one layer: device events, %d "
             "alternated rounds, one process; every launch timed twice per round (a, b): an A/A pair" % args.rounds,
             "map %d x %d at %.1f m, seeds above %.0f, gap2 %d, min_cells %d, K %d: %d rows, every second one a mover (mask form), fill 0, owner_out "
             "written; at halo2 9 the fields of a layer are %s" % (g.rows, g.cols, g.res, THRESHOLD, GAP2, MIN_CELLS, K, n[2], fields.tolist())]
    yard = {}
    for name in [nm for nm, _ in launches]:
        a, b = times[(name, "a")], times[(name, "b")]
        if name.startswith("inflate_map"):
            yard[name.split(", ", 1)[1]] = median(a + b)
        lines.append("   %-44s ms (%2d per window)   a: %s   b: %s   a/b medians differ by %.1f %%"
                     % (name + ",", args.reps, spread(a), spread(b), 100.0 * abs(median(a) - median(b)) / max(median(a), median(b))))
    for name in [nm for nm, _ in launches if nm.startswith("clear_movers")]:
        key = name.split(", ", 1)[1].rsplit(", halo2", 1)[0]
        m = median(times[(name, "a")] + times[(name, "b")])
        lines.append("   %-44s %.4f ms = %.2f of the inflation of the same size (%.4f ms)" % (name + ":", m, m / yard[key], yard[key]))
    lines.append("   layers, owners and fields of the %d layers at halo2 9 bit-identical over the rounds: %s" % (Lm, same))
    lines.append("   where the time goes inside the call (the clear of the fields, the tile launch, the finish launch) was not measured")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
