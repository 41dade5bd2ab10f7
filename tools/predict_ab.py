#!/usr/bin/env python3
"""The two launches of the tracked-obstacle path, each beside the launch it is set against, in one process, alternated round by round so
that all see the same clocks and neighbours:

  predict      cilqr_predict_obstacles_device (every output) at T = 1 with M = 8 and M = 30 and at T = 1024 with M = 4, N = 50,
               beside the page-locked upload of the same host-built table (pose, dim, cov: 9*M*N doubles per set), which it replaces
  chance cov   cilqr_chance_risk_cov_device on config-2 scenes at B = 16 and B = 1024 (N = 50, M = 4, one covariance per entry),
               beside cilqr_chance_risk_device in the same run, every optional output asked for

Times are device events; the launches are short, so a window holds --reps of them back to back and is divided by their number.  Every
step is measured TWICE per round, as series A and series A' of the same code: the difference of their medians is the run's A/A spread,
and a difference between two steps counts only beyond it.  Nothing is promised in advance: the file reports the medians, and where a
new launch is slower than its neighbour by more than the A/A spread the line says SLOWER (README.md says what is known and what is
only supposed about where that time goes: this file holds nothing written by hand).  The last lines give the new kernels' register
counts, read from the built objects' metadata (tools/check_kernel_resources.py).

    python tools/predict_ab.py [--rounds R] [--reps K] [--out profiles/r18_predict.txt]
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

SIGMA0 = np.diag([0.16 ** 2, 0.16 ** 2, 0.0, 0.017 ** 2]).reshape(16)
W = np.diag([1e-4, 1e-4, 4e-4, 1e-6]).reshape(16)
P0 = np.diag([0.3 ** 2, 0.3 ** 2, 0.5 ** 2, 0.05 ** 2]).reshape(16)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def spread(ts):
    ts = sorted(ts)
    return "min %.4f  median %.4f  max %.4f" % (ts[0], ts[len(ts) // 2], ts[-1])


def tracks(T, M, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    tr = np.zeros((T, M, 6))
    tr[..., 0], tr[..., 1] = rng.uniform(-20, 20, (T, M)), rng.uniform(-20, 20, (T, M))
    tr[..., 2], tr[..., 3] = rng.uniform(0, 12, (T, M)), rng.uniform(-3.1, 3.1, (T, M))
    tr[..., 4], tr[..., 5] = rng.uniform(-3, 2, (T, M)), rng.uniform(-0.3, 0.3, (T, M))
    dim = np.stack([rng.uniform(3, 6, (T, M)), rng.uniform(1.5, 2.5, (T, M))], axis=-1)
    return tr, dim, np.ascontiguousarray(np.broadcast_to(P0, (T, M, 16)))


def register_lines():
    """Vector registers, spills and scratch of the predict and chance-risk kernels, from the metadata of every gfx950 code object inside
    the built library (the notes tools/check_kernel_resources.py reads from one object file)."""
    import re
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    out = []
    try:
        with tempfile.TemporaryDirectory() as d:
            tmp = os.path.join(d, "lib.so")
            with open(cilqr_amd.LIB_PATH, "rb") as f, open(tmp, "wb") as g:
                g.write(f.read())
            subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", tmp], cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            for n in sorted(os.listdir(d)):
                if "amdgcn" not in n:
                    continue
                text = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(d, n)], check=True, capture_output=True, text=True).stdout
                for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
                    blk = m.group(0)
                    name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                    if "cilqr_predict_obstacles_kernel" not in name and "cilqr_chance_risk_kernel" not in name:
                        continue
                    g = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))  # noqa: E731
                    out.append("registers: %-100s %3d VGPR, %d AGPR, %d spilled, %d bytes of scratch" % (
                        name, g("vgpr_count"), g("agpr_count"), g("vgpr_spill_count") + g("sgpr_spill_count"), g("private_segment_fixed_size")))
    except (OSError, subprocess.CalledProcessError) as e:
        out.append("registers: not read (%s)" % e)
    return sorted(out) or ["registers: no such kernel found in the library"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, M, B = 50, 4, 1024
    p = cilqr_amd.default_params(N)
    s = cilqr_amd.Solver(p, max_batch=B, max_horizon=N, max_obstacles=30, device=0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device="cuda")  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    steps = []  # (name, callable, name of the step it is set beside or None)

    # ---- predict beside the upload it replaces
    keep = []
    for T, Mp in ((1, 8), (1, 30), (1024, 4)):
        tr, dim, cov = tracks(T, Mp, 3)
        d = dict(tr=dv(tr), dim=dv(dim), cov=dv(cov), Q=dv(W), pose=zeros(T, Mp, 4 * N), dout=zeros(T, Mp, 2 * N), cout=zeros(T, Mp, 3 * N),
                 sig=zeros(T, Mp, N, 16))
        table = torch.from_numpy(np.random.default_rng(1).normal(size=(T, Mp, 9 * N))).pin_memory()  # the host-built pose, dim, cov
        dst = zeros(T, Mp, 9 * N)
        keep.append((d, table, dst))
        tag = "T=%d M=%d" % (T, Mp)

        def predict(d=d, T=T, Mp=Mp, full=True):
            s.predict_obstacles_device(stream, T, N, Mp, d["tr"].data_ptr(), d["dim"].data_ptr(), d["pose"].data_ptr(), d["dout"].data_ptr(),
                                       track_cov=d["cov"].data_ptr(), track_noise=d["Q"].data_ptr(), cov_out=d["cout"].data_ptr(),
                                       sigma_out=d["sig"].data_ptr() if full else 0)

        def upload(table=table, dst=dst):
            dst.copy_(table, non_blocking=True)

        steps.append(("upload of the table, %s" % tag, upload, None))
        steps.append(("predict, pose + dim + cov, %s" % tag, lambda f=predict: f(full=False), "upload of the table, %s" % tag))
        steps.append(("predict, every output, %s" % tag, predict, "upload of the table, %s" % tag))

    # ---- the judge with and without the obstacle covariance
    sc = scenes.make_c2(B, p)
    t = dict(x0=dv(sc["x0"]), U=dv(sc["U"]), poly=dv(sc["poly"]), fl=dv(sc["xplan_fl"]), pose=dv(sc["obs_pose"]), dim=dv(sc["obs_dim"]),
             s0=dv(SIGMA0), W=dv(W), ocov=dv(np.broadcast_to(np.array([0.09, 0.01, 0.09]), (B, M, N, 3))))
    t.update(X=zeros(B, 4 * (N + 1)), J=zeros(B), it=zeros(B, dtype=torch.int32), st=zeros(B, dtype=torch.int32), k=zeros(B, 2 * N),
             K=zeros(B, 8 * N), ok=zeros(B, dtype=torch.int32), crisk=zeros(B, cilqr_amd.CHANCE_FIELDS), cstep=zeros(B, N), cep=zeros(B, M * N),
             csig=zeros(B, N + 1, 16), ctotal=zeros(B))
    ptr = {k: v.data_ptr() for k, v in t.items()}
    strides = (M * N, N, 1, 0)
    torch.cuda.synchronize()
    s.solve_batch_device(stream, B, N, M, ptr["x0"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, ptr["X"], ptr["J"], ptr["it"], ptr["st"])
    s.gains_batch_device(stream, B, N, M, ptr["X"], ptr["U"], ptr["poly"], ptr["fl"], ptr["pose"], ptr["dim"], 0, strides, ptr["k"], ptr["K"], ptr["ok"], lamb=1.0)
    torch.cuda.synchronize()

    def chance(b, cov):
        s.chance_risk_cov_device(stream, b, N, M, ptr["X"], ptr["U"], ptr["K"], ptr["s0"], 0, ptr["W"], ptr["pose"], ptr["dim"], strides,
                                 ptr["ocov"] if cov else 0, ptr["crisk"], ptr["cstep"], ptr["cep"], ptr["csig"], ptr["ctotal"], ptr["J"], max_risk=0.05)

    for b in (16, B):
        steps.append(("chance_risk, B=%d" % b, lambda b=b: chance(b, False), None))
        steps.append(("chance_risk_cov, B=%d" % b, lambda b=b: chance(b, True), "chance_risk, B=%d" % b))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        for _, f, _ in steps:
            f()
    torch.cuda.synchronize()
    times = {(name, series): [] for name, _, _ in steps for series in "AB"}
    for _ in range(args.rounds):
        for series in "AB":
            for name, f, _ in steps:
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[(name, series)].append(e0.elapsed_time(e1) / args.reps * 1e3)
    s.close()
    lines = ["tracked-obstacle path: device events, %d alternated rounds of two series (A, A') per step, %d launches per window, one process; "
             "microseconds per launch" % (args.rounds, args.reps),
             "N=%d; predict: one wavefront per track, T*M workgroups; upload: 9*M*N doubles per set from page-locked memory in one copy" % N]
    med = {}
    for name, _, beside in steps:
        a, b = median(times[(name, "A")]), median(times[(name, "B")])
        med[name] = (0.5 * (a + b), abs(a - b))
        line = "   %-44s A: %s   A': median %.4f   A/A %.4f us (%.1f %%)" % (name + ",", spread(times[(name, "A")]), b, abs(a - b), 100 * abs(a - b) / a)
        if beside:
            ref, ref_aa = med[beside]
            d = med[name][0] - ref
            noise = max(ref_aa, med[name][1])
            verdict = "within the A/A spread" if abs(d) <= noise else ("faster" if d < 0 else "SLOWER")
            line += "   = %.2f x %s (%+.3f us: %s)" % (med[name][0] / ref, beside, d, verdict)
        lines.append(line)
    lines += register_lines()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
