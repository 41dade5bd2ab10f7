#!/usr/bin/env python3
"""The tracker tick (cilqr_track_update_device) beside the call in front of it (cilqr_map_obstacles_device), the launch behind it
(cilqr_predict_obstacles_device) and what it replaces on the way from the map's boxes to the prediction — the page-locked read-back of D
boxes plus the upload of M tracks of 24 doubles — in one process, alternated round by round so that all see the same clocks and
neighbours:

  the tick at W = 1 with (M, D) = (16, 16) and (64, 64), and at W = 1024 with (16, 16): a mid-life table (a grid of vehicles 6 m apart
  at 5 m/s, four ticks old, three quarters of them seen again this tick, the rest of the detections new) read from one buffer and
  written to another, so that every launch does the same work  |  map_obstacles at L = 1 on the node's 150 x 100 map, K = 16  |
  predict_obstacles at T = 1, N = 50, M = 16  |  the copy of 16 boxes to page-locked memory and of 16 x 24 doubles from it

Times are device events.  Every launch is timed TWICE per round, as an A/A pair ("a" and "b" below) at different places of the round: the
difference of the two medians is what this method cannot tell apart.  Each is timed --reps back to back and divided by their number.
The host loop a caller would run between the read-back and the upload (association and filter on the CPU) is NOT in the replaced
figure.  Nothing is promised in advance: at W = 1 the tick is one wavefront's chain.

    python tools/track_update_ab.py [--rounds R] [--reps K] [--out profiles/r26_track_update.txt]
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
from tighten_map_ab import GEOM, POSE, dv, timed, zeros  # noqa: E402

DT, N_PLAN, K_MAP = 0.1, 50, 16


def detections(M, D, tick, seen):
    """Vehicle m of a grid 6 m apart, at 5 m/s along +x, as a box row at `tick`; the first `seen` vehicles, then new ones elsewhere."""
    rows = np.zeros((D, 5))
    for d in range(D):
        m = d if d < seen else M + d
        rows[d] = (-45.0 + 6.0 * (m % 16) + 5.0 * DT * tick, -45.0 + 6.0 * (m // 16), 0.0, 4.5, 1.9)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Wb = 1024
    s = cilqr_amd.Solver(cilqr_amd.default_params(N_PLAN), max_batch=Wb, max_horizon=N_PLAN, max_obstacles=64, device=0)
    filt = cilqr_amd.track_filter(DT, cilqr_amd.white_acceleration_noise(0.5, DT), np.eye(2) * 0.05 ** 2, np.diag([0.05 ** 2, 0.05 ** 2, 16.0, 16.0]),
                                  gate2=9.21, min_hits=2, max_misses=3, v_min=0.5, theta_var_slow=1.0)
    stream = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32)
    cases, records = {}, {}
    for name, W, M, D in (("W=1, M=16, D=16", 1, 16, 16), ("W=1, M=64, D=64", 1, 64, 64), ("W=%d, M=16, D=16" % Wb, Wb, 16, 16)):
        t = dict(state=zeros(W, M, cilqr_amd.TRACK_STATE), out=zeros(W, M, cilqr_amd.TRACK_STATE), world=zeros(W, cilqr_amd.TRACK_WORLD_FIELDS),
                 track=zeros(W, M, 6), dim=zeros(W, M, 2), cov=zeros(W, M, 16), assign=zeros(W, D, **i32))
        for tick in range(4):  # the table's first four ticks, in place: every vehicle seen
            det = dv(np.broadcast_to(detections(M, D, tick, D), (W, D, 5)))
            s.track_update_device(stream, W, M, D, det.data_ptr(), filt, t["state"].data_ptr(), t["state"].data_ptr(), t["world"].data_ptr(),
                                  t["track"].data_ptr(), t["dim"].data_ptr(), t["cov"].data_ptr(), assign=t["assign"].data_ptr(),
                                  flags=cilqr_amd.TRACK_RESET if tick == 0 else 0)
        torch.cuda.synchronize()
        t["det"] = dv(np.broadcast_to(detections(M, D, 4, 3 * D // 4), (W, D, 5)))
        cases[name] = (W, M, D, t)

    def tick_of(name):
        W, M, D, t = cases[name]

        def f():
            s.track_update_device(stream, W, M, D, t["det"].data_ptr(), filt, t["state"].data_ptr(), t["out"].data_ptr(), t["world"].data_ptr(),
                                  t["track"].data_ptr(), t["dim"].data_ptr(), t["cov"].data_ptr(), assign=t["assign"].data_ptr())
        return f

    g = cilqr_amd.map_geom(*GEOM)
    cells = g.rows * g.cols
    m = dict(layer=flat(smooth_layer(g.rows, g.cols, 1)), pose=torch.tensor(POSE, dtype=torch.float64).cuda(), d2=zeros(cells, **i32),
             work=zeros(cells, **i32), label=zeros(cells, **i32), n=zeros(4, **i32), comp=zeros(K_MAP, cilqr_amd.MAP_OBSTACLE_FIELDS),
             boxes=zeros(K_MAP, 5))
    s.map_distance_device(stream, 1, m["layer"].data_ptr(), 0, g, THRESHOLD, m["d2"].data_ptr())

    def obstacles():
        s.map_obstacles_device(stream, 1, m["d2"].data_ptr(), g, K_MAP, m["work"].data_ptr(), m["label"].data_ptr(), m["n"].data_ptr(),
                               m["comp"].data_ptr(), m["boxes"].data_ptr(), gap2=1, pose=m["pose"].data_ptr(), pose_stride=0, min_cells=3)

    _, Mp, _, tp = cases["W=1, M=16, D=16"]
    p = dict(pose=zeros(Mp, 4 * N_PLAN), dim=zeros(Mp, 2 * N_PLAN), cov=zeros(Mp, 3 * N_PLAN))

    def predict():
        s.predict_obstacles_device(stream, 1, N_PLAN, Mp, tp["track"].data_ptr(), tp["dim"].data_ptr(), p["pose"].data_ptr(), p["dim"].data_ptr(),
                                   track_cov=tp["cov"].data_ptr(), cov_out=p["cov"].data_ptr())

    host_boxes, host_tracks = torch.from_numpy(cilqr_amd.pinned_empty((16, 5))), torch.from_numpy(cilqr_amd.pinned_empty((16, 24)))
    host_tracks[...] = 1.0
    dev_tracks = zeros(16, 24)

    def replaced():
        host_boxes.copy_(m["boxes"], non_blocking=True)
        dev_tracks.copy_(host_tracks, non_blocking=True)

    launches = [("track_update, " + name, tick_of(name)) for name in cases] + [
        ("map_obstacles, L=1, K=%d (in front)" % K_MAP, obstacles), ("predict_obstacles, T=1, N=%d, M=%d (behind)" % (N_PLAN, Mp), predict),
        ("16 boxes down + 16 x 24 doubles up, page-locked", replaced)]
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
        now = [cases[n][3][k].clone() for n in cases for k in ("out", "track", "dim", "cov", "assign")]
        first = now if first is None else first
        same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, first))
    for name in cases:
        records[name] = cases[name][3]["world"][0].cpu().numpy().astype(int).tolist()
    lines = ["tracker tick beside the map's boxes in front of it, the prediction behind it and the two page-locked copies it replaces: device events, "
             "%d alternated rounds, one process; every launch timed twice per round (a, b): an A/A pair" % args.rounds,
             "world record of the timed tick (next_id ticks live confirmed matched born died dropped invalid; next_id and ticks count the timed "
             "launches): " + "; ".join("%s: %s" % (n, records[n]) for n in cases)]
    for name in [nm for nm, _ in launches]:
        a, b = times[(name, "a")], times[(name, "b")]
        lines.append("   %-50s ms (%2d per window)   a: %s   b: %s   a/b medians differ by %.1f %%"
                     % (name + ",", args.reps, spread(a), spread(b), 100.0 * abs(median(a) - median(b)) / max(median(a), median(b))))
    med = {name: median(times[(name, "a")] + times[(name, "b")]) for name, _ in launches}
    node = "track_update, W=1, M=16, D=16"
    lines.append("   %s: %.4f ms = %.2f of map_obstacles in front of it (%.4f ms), %.2f of predict_obstacles behind it (%.4f ms), %.2f of the two "
                 "copies it replaces (%.4f ms; the host loop between them is not in that figure)"
                 % (node, med[node], med[node] / med[launches[3][0]], med[launches[3][0]], med[node] / med[launches[4][0]], med[launches[4][0]],
                    med[node] / med[launches[5][0]], med[launches[5][0]]))
    big = "track_update, W=%d, M=16, D=16" % Wb
    lines.append("   %s: %.4f ms = %.2f of the tick of one world" % (big, med[big], med[big] / med[node]))
    lines.append("   state, track, dim, cov and assign of the three cases bit-identical over the rounds: %s" % same)
    lines.append("   where the time goes inside the tick's one launch was not measured")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
