#!/usr/bin/env python3
"""K costmap frames (warp -> blur -> OccupancyGrid), one frame per call against one call for all, alternated in one process so that
both see the same clocks:

  a  K cilqr_costmap_frame_device calls enqueued back to back (2K launches): what a caller with K candidate poses had to do;
  b  one cilqr_costmap_frame_batch_device call (2 launches, one pose-table upload).

and the same two legs for the blur alone at the node's size (cilqr_blur_costmap_device K times / cilqr_blur_costmap_batch_device).
Device events around every call sequence on an idle stream, LAUNCHES of each after warm-up; all outputs of the two legs are
compared bit for bit first.  Each figure is the event time of one sequence: host enqueue cost that the device has to wait for is
inside it, as it is for a caller.

Leg a uses only entry points that were there before the batch calls, so the script also runs against an older checkout's package
and library (--tree DIR: leg b is skipped when that package has no batch call): the two leg-a medians show whether the single-frame
path has moved.

    python tools/frame_batch_ab.py [--launches 40] [--tree OLDER_CHECKOUT] [--out profiles/r07_frame_batch.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch  # (before the library: torch's HIP runtime first, tests/conftest.py)

PKG_NAME = "uncertainty-aware-cilqr-for-trajectory-optimization_amd"


def spread(ts, K):
    ts = sorted(ts)
    lo, med, hi = ts[0], ts[len(ts) // 2], ts[-1]
    return "min %8.1f  median %8.1f  max %8.1f   per frame: median %7.2f  (min-max spread %.2f)" % (lo, med, hi, med / K, (hi - lo) / K)


def node_source(rng):
    """bench.py --workload frame: the node's 1506 x 1506 global map at 0.2 m"""
    src = np.zeros((1506, 1506), dtype=np.float32)
    for _ in range(400):
        i, j = rng.integers(0, 1450, 2)
        src[i:i + rng.integers(3, 50), j:j + rng.integers(3, 50)] = 100.0
    src[rng.random(src.shape) < 0.02] = np.nan
    return src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package and built library are measured")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.launches >= 30
    sys.path[:0] = [args.tree, os.path.join(args.tree, PKG_NAME)]
    import cilqr_amd
    from cilqr_amd import scenes
    have_batch = hasattr(cilqr_amd.Solver, "costmap_frame_batch_device")

    dev = torch.device("cuda", 0)
    s = cilqr_amd.Solver(cilqr_amd.default_params(), max_batch=1, max_horizon=1, max_obstacles=0, device=0)
    stream = torch.cuda.current_stream().cuda_stream
    sig = (0.16, 0.16, 0.017)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rng = np.random.default_rng(61)
    circle = [(60 * np.cos(a), 60 * np.sin(a), a + np.pi / 2) for a in np.linspace(0, 2 * np.pi, 300, endpoint=False)]
    c4 = scenes.make_c4()
    node_src = node_source(rng)
    shapes = [
        ("node sizes (bench.py --workload frame)", node_src, (301.2, 301.2, 0.2, 0.0, 0.0), (30.0, 20.0, 0.2, 10.0 - 5, 0.0), circle, (1, 4, 16, 64)),
        ("400x300 vehicle map at 0.1 m", node_src, (301.2, 301.2, 0.2, 0.0, 0.0), (40.0, 30.0, 0.1, 10.0, 0.0), circle, (1, 4, 16)),
        ("1024x1024 -> 1024x1024 (config 4)", c4["src"], c4["src_geom"], c4["dst_geom"], [tuple(p) for p in c4["poses"]], (1, 4)),
    ]
    lines = ["K costmap frames (warp -> blur -> OccupancyGrid): microseconds per call sequence by device events on an idle stream,",
             "%d launches of each after %d of warm-up, the legs alternated; device: %s" % (args.launches, args.warmup, torch.cuda.get_device_name(0)),
             "  a = K cilqr_costmap_frame_device calls back to back   b = one cilqr_costmap_frame_batch_device call",
             "  (blur alone: a = K cilqr_blur_costmap_device calls, b = one cilqr_blur_costmap_batch_device call)",
             "library: %s%s" % (os.path.relpath(cilqr_amd.LIB_PATH, args.tree), "" if have_batch else "   (no batch entry points: leg a only)"), ""]

    def measure(legs, K):
        res = {k: [] for k in legs}
        for it in range(args.warmup + args.launches):
            for name, fn in legs.items():
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    res[name].append(1e3 * e0.elapsed_time(e1))
        for name in legs:
            lines.append("   %s  %s" % (name, spread(res[name], K)))

    for title, src_h, sgeo, dgeo, pose_list, Ks in shapes:
        sg, dg = cilqr_amd.map_geom(*sgeo), cilqr_amd.map_geom(*dgeo)
        cells = dg.rows * dg.cols
        d_src = torch.from_numpy(np.ascontiguousarray(np.asarray(src_h).T)).to(dev)
        lines.append("%s: %dx%d source at %.1f m -> %dx%d vehicle map at %.1f m" % (title, sg.rows, sg.cols, sg.res, dg.rows, dg.cols, dg.res))
        for K in Ks:
            poses = np.array([pose_list[(7 * k) % len(pose_list)] for k in range(K)], dtype=np.float64)
            out = {leg: (torch.zeros(K * cells, dtype=torch.float32, device=dev), torch.zeros(K * cells, dtype=torch.float32, device=dev),
                         torch.zeros(K * cells, dtype=torch.int8, device=dev), torch.zeros(K, dtype=torch.int64, device=dev)) for leg in "ab"}

            def leg_a(o=out["a"]):
                for k in range(K):
                    s.costmap_frame_device(stream, d_src.data_ptr(), sg, dg, *poses[k], *sig, o[0].data_ptr() + 4 * k * cells, o[1].data_ptr() + 4 * k * cells,
                                           occupancy_out=o[2].data_ptr() + k * cells, n_oob=o[3].data_ptr() + 8 * k)

            def leg_b(o=out["b"]):
                s.costmap_frame_batch_device(stream, d_src.data_ptr(), sg, dg, poses, *sig, o[0].data_ptr(), o[1].data_ptr(), occupancy_out=o[2].data_ptr(),
                                             n_oob=o[3].data_ptr())

            legs = {"frame a": leg_a}
            same = "-"
            if have_batch:
                legs["frame b"] = leg_b
                leg_a()
                leg_b()
                torch.cuda.synchronize()
                same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                           for x, y in zip(out["a"], out["b"]))
            lines.append(" K = %d; all outputs of a and b bit-identical: %s" % (K, same))
            measure(legs, K)
            del out
        lines.append("")

    # the blur alone at the node's size, each frame blurring its own layer
    g = cilqr_amd.map_geom(30.0, 20.0, 0.2, 10.0 - 5, 0.0)
    cells = g.rows * g.cols
    lines.append("blur alone, %dx%d at %.1f m, one source layer per frame" % (g.rows, g.cols, g.res))
    for K in (1, 4, 16, 64):
        layers = rng.integers(0, 101, K * cells).astype(np.float32)
        layers[rng.random(K * cells) < 0.01] = np.nan
        d_layers = torch.from_numpy(layers).to(dev)
        thetas = np.array([circle[(7 * k) % len(circle)][2] for k in range(K)])
        out = {leg: torch.zeros(K * cells, dtype=torch.float32, device=dev) for leg in "ab"}

        def blur_a(o=out["a"]):
            for k in range(K):
                s.blur_costmap_device(stream, d_layers.data_ptr() + 4 * k * cells, g, thetas[k], *sig, o.data_ptr() + 4 * k * cells)

        def blur_b(o=out["b"]):
            s.blur_costmap_batch_device(stream, d_layers.data_ptr(), g, thetas, *sig, o.data_ptr(), src_stride=cells)

        legs = {"blur  a": blur_a}
        same = "-"
        if have_batch:
            legs["blur  b"] = blur_b
            blur_a()
            blur_b()
            torch.cuda.synchronize()
            same = torch.equal(out["a"].view(torch.int32), out["b"].view(torch.int32))
        lines.append(" K = %d; outputs of a and b bit-identical: %s" % (K, same))
        measure(legs, K)
    lines.append("")
    s.close()
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
