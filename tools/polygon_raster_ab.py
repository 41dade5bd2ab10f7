#!/usr/bin/env python3
"""The bounding-box override of one 1024^2 map frame, three ways, alternated in one process so that all see the same clocks:

  a  what a caller had to do before there were polygon entry points: a page-locked 4 MiB bbox layer (rasterised on the host,
     which is NOT timed here) uploaded on the stream, then cilqr_warp_costmap_device / cilqr_costmap_frame_device with it;
  b  cilqr_rasterize_polygons_device into a device layer, then the same warp;
  c  cilqr_warp_costmap_polygons_device / cilqr_costmap_frame_polygons_device: no layer at all.

Device events around every call sequence, LAUNCHES of each after warm-up, for 16, 64 and 256 boxes; the outputs of the three are
compared bit for bit first.  Each figure is the event time of one sequence enqueued on an idle stream: host enqueue cost that the
device has to wait for is inside it, as it is for a caller.

    python tools/polygon_raster_ab.py [--launches 60] [--out profiles/r06_polygon_raster.txt]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uncertainty-aware-cilqr-for-trajectory-optimization_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library: torch's HIP runtime first, tests/conftest.py)

import cilqr_amd  # noqa: E402


def spread(ts):
    ts = sorted(ts)
    return "min %7.1f  median %7.1f  max %7.1f" % (ts[0], ts[len(ts) // 2], ts[-1])


def boxes(n, dg_args, seed):
    """n vehicle-sized boxes over the map, every seventh axis-aligned, in the vehicle frame of a vehicle at the origin."""
    len_x, len_y, _, pos_x, pos_y = dg_args
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 5))
    b[:, 0] = pos_x + rng.uniform(-0.5 * len_x, 0.5 * len_x, n)
    b[:, 1] = pos_y + rng.uniform(-0.5 * len_y, 0.5 * len_y, n)
    b[:, 2] = rng.uniform(-math.pi, math.pi, n)
    b[::7, 2] = 0.0
    b[:, 3] = rng.uniform(3.5, 5.5, n)
    b[:, 4] = rng.uniform(1.6, 2.2, n)
    return cilqr_amd.boxes_to_polygons(b, 0.0, 0.0, 0.0)


def equal(a, b, kind):
    """warp: destination layer and out-of-range counter; frame: both layers, the occupancy grid and the counter"""
    return all(torch.equal(a[i], b[i]) if isinstance(a[i], torch.Tensor) else a[i] == b[i] for i in ((0, 3) if kind == "warp" else (0, 1, 2, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.launches >= 50

    dev = torch.device("cuda", 0)
    s = cilqr_amd.Solver(cilqr_amd.default_params(), max_batch=4, max_horizon=50, max_obstacles=4, device=0)
    dg_args = (102.4, 102.4, 0.1, 10.0, 0.0)
    dg = cilqr_amd.map_geom(*dg_args)
    sg = cilqr_amd.map_geom(301.2, 301.2, 0.2, 20.0, -10.0)  # the reference's global map size (M/src/local_costmap.cpp:119)
    pose = (2.0, -1.5, 0.7)
    sig = (0.16, 0.16, 0.017)
    rng = np.random.default_rng(0)
    d_src = torch.from_numpy(rng.integers(0, 101, sg.rows * sg.cols).astype(np.float32)).to(dev)
    nd = dg.rows * dg.cols
    stream = torch.cuda.current_stream().cuda_stream
    new = lambda dt=torch.float32: torch.zeros(nd, dtype=dt, device=dev)  # noqa: E731
    d_bbox, d_dst, d_veh, d_unc, d_occ = new(), new(), new(), new(), new(torch.int8)
    d_oob = torch.zeros(1, dtype=torch.int64, device=dev)
    pinned = torch.empty(nd, dtype=torch.float32).pin_memory()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    lines = ["bounding-box override of one %dx%d frame at %.1f m (source %dx%d at %.1f m), microseconds per call sequence by device events,"
             % (dg.rows, dg.cols, dg.res, sg.rows, sg.cols, sg.res),
             "%d launches of each after %d of warm-up, the variants alternated; device: %s" % (args.launches, args.warmup, torch.cuda.get_device_name(0)),
             "  a = page-locked 4 MiB bbox upload + call with the layer   b = cilqr_rasterize_polygons_device + call with the layer",
             "  c = the call with the polygons (no layer)", ""]
    for n in (16, 64, 256):
        polys = boxes(n, dg_args, seed=n)

        def warp_layer():
            s.warp_costmap_device(stream, d_src.data_ptr(), sg, d_dst.data_ptr(), dg, *pose, bbox=d_bbox.data_ptr(), n_oob=d_oob.data_ptr())

        def frame_layer():
            s.costmap_frame_device(stream, d_src.data_ptr(), sg, dg, *pose, *sig, d_veh.data_ptr(), d_unc.data_ptr(),
                                   occupancy_out=d_occ.data_ptr(), bbox=d_bbox.data_ptr(), n_oob=d_oob.data_ptr())

        def upload():
            d_bbox.copy_(pinned, non_blocking=True)

        def raster():
            s.rasterize_polygons_device(stream, dg, polys, d_bbox.data_ptr())

        variants = {
            "warp  a": lambda: (upload(), warp_layer()),
            "warp  b": lambda: (raster(), warp_layer()),
            "warp  c": lambda: s.warp_costmap_polygons_device(stream, d_src.data_ptr(), sg, d_dst.data_ptr(), dg, *pose, polys, n_oob=d_oob.data_ptr()),
            "frame a": lambda: (upload(), frame_layer()),
            "frame b": lambda: (raster(), frame_layer()),
            "frame c": lambda: s.costmap_frame_polygons_device(stream, d_src.data_ptr(), sg, dg, *pose, polys, *sig, d_veh.data_ptr(),
                                                               d_unc.data_ptr(), occupancy_out=d_occ.data_ptr(), n_oob=d_oob.data_ptr()),
            "raster ": raster,
        }
        # the layer of variant a is variant b's, fetched once; outputs of the three, bit for bit
        raster()
        torch.cuda.synchronize()
        pinned.copy_(d_bbox)
        marked = int((pinned == 100.0).sum())
        outs = {}
        for name in ("warp  a", "warp  b", "warp  c", "frame a", "frame b", "frame c"):
            d_bbox.fill_(-1.0)
            variants[name]()
            torch.cuda.synchronize()
            first = d_dst if name.startswith("warp") else d_veh
            outs[name] = (first.view(torch.int32).clone(), d_unc.view(torch.int32).clone(), d_occ.clone(), int(d_oob.item()))
        same = all(equal(outs["%-5s a" % k], outs["%-5s %s" % (k, o)], k) for k in ("warp", "frame") for o in "bc")
        res = {k: [] for k in variants}
        for it in range(args.warmup + args.launches):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    res[name].append(1e3 * e0.elapsed_time(e1))
        lines.append("%d boxes (%d cells marked); outputs of a, b and c bit-identical: %s" % (n, marked, same))
        for name in variants:
            lines.append("   %s  %s" % (name, spread(res[name])))
        lines.append("")
    s.close()
    text = "\n".join(lines)
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
