"""The facade's device block (host/candidate_layout.h): where the arrays of iLQR::run_candidates lie and which stages a run enqueues are
decided by one plain struct, on the host.  Checked here without a GPU through tests/cpp/candidate_layout_dump.cpp, over the full product
of the mode flags at small sizes:
  * every offset is even (int32 arrays share double slots), no two arrays overlap, `end` is the sum of the rounded sizes;
  * every array a stage of that mode reads or writes has its full size reserved (NEEDS below: what each C-ABI call takes, from
    include/cilqr.h, stated here and not read from the header under test);
  * for the modes that existed before the block was laid out there — everything but the sample covariance check — every offset and
    `end` equal those of the adapter's earlier reserve function, whose rules `earlier_layout` restates independently.
Sizes: B in {1, 3}, N in {1, 2, 7}, M in {0, 1, 3}, S in {1, 2, 257} (0 with no offsets set), n_samples in {0, 2} (n_samples > 0 IS the
`sampled` flag), Q in {0, 1, 27} (Q > 0 IS set_map_covariance_check being on)."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

SCORE, RISK, RRISK, RRS, MAPR, CHANCE, TIGHTEN, TMAP, TRACK, CMAP, CRS, POLY = 8, 4, 6, 8, 7, 6, 4, 6, 6, 8, 8, 6  # include/cilqr.h


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("candidate_layout") / "candidate_layout_dump")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "host"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "candidate_layout_dump.cpp")], check=True)
    names = dict(line.split(":") for line in subprocess.run([exe, "names"], check=True, capture_output=True, text=True).stdout.splitlines())
    flags, preds, arrays = (names[k].split() for k in ("flags", "predicates", "arrays"))

    def run(f, z):
        """f: {flag: bool array}, z: {size: int array} -> ({predicate: bool array}, {array: offsets}, reserved {array: doubles})"""
        n = len(z["B"])
        rec = np.zeros((n, 8), dtype=np.uint64)
        for i, name in enumerate(flags):
            rec[:, 0] |= f[name].astype(np.uint64) << np.uint64(i)
        for i, name in enumerate(("B", "N", "M", "S", "n_obs", "n_samples", "Q")):
            rec[:, 1 + i] = z[name]
        out = subprocess.run([exe], input=rec.tobytes(), check=True, capture_output=True).stdout
        out = np.frombuffer(out, dtype=np.uint64).reshape(n, 1 + len(arrays)).astype(np.int64)
        p = {name: (out[:, 0] >> i) & 1 == 1 for i, name in enumerate(preds)}
        off = {name: out[:, 1 + i] for i, name in enumerate(arrays)}
        reserved = {name: out[:, 2 + i] - out[:, 1 + i] for i, name in enumerate(arrays[:-1])}
        return p, off, reserved
    run.flags, run.arrays = flags, arrays
    return run


def _product(flag_names):
    """Every combination of `flag_names` x the sizes of the module docstring."""
    rows = list(itertools.product(*([(False, True)] * len(flag_names)), (1, 3), (1, 2, 7), (0, 1, 3), (0, 1, 2, 257), (0, 2), (0, 1, 27)))
    a = np.array(rows, dtype=np.int64)
    k = len(flag_names)
    f = {name: a[:, i] == 1 for i, name in enumerate(flag_names)}
    z = dict(B=a[:, k], N=a[:, k + 1], M=a[:, k + 2], S=a[:, k + 3], n_samples=a[:, k + 4], Q=a[:, k + 5])
    f["noise"], f["sampled"], f["cmap"] = z["S"] > 0, z["n_samples"] > 0, z["Q"] > 0
    z["n_obs"] = np.where(f["sampled"], 2, 0)
    return f, z


LAYOUT_FLAGS = ["fused", "cov", "scov", "cov_judge", "tighten", "map_tighten", "track_map"]  # with noise, sampled, cmap: all the layout reads
RUN_FLAGS = ["map", "min_total", "map_set", "obstacles", "tracks"]


@pytest.fixture(scope="module")
def layouts(dump):
    f, z = _product(LAYOUT_FLAGS)
    for name in RUN_FLAGS:
        f[name] = np.zeros(len(z["B"]), dtype=bool)
    return (f, z) + dump(f, z)


def test_header_is_plain_cpp():
    text = open(os.path.join(PKG, "host", "candidate_layout.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text


def test_layout_does_not_read_the_scene(dump):
    """No setter reserves by the pick, the map, the obstacles or the tracks that are set at the time of a run: the offsets ignore them."""
    f, z = _product(LAYOUT_FLAGS[:3] + RUN_FLAGS)
    for name in LAYOUT_FLAGS[3:]:
        f[name] = np.ones(len(z["B"]), dtype=bool)
    _, off, _ = dump(f, z)
    g = dict(f)
    for name in RUN_FLAGS:
        g[name] = np.zeros(len(z["B"]), dtype=bool)
    _, off0, _ = dump(g, z)
    for name in dump.arrays:
        assert np.array_equal(off[name], off0[name]), name


def test_offsets_even_disjoint_and_end_is_the_sum(layouts, dump):
    f, z, _, off, reserved = layouts
    assert dump.arrays[-1] == "end" and np.all(off[dump.arrays[0]] == 0)
    total = np.zeros(len(z["B"]), dtype=np.int64)
    for name in dump.arrays[:-1]:  # (the arrays lie in this order: reserved = the next offset minus this one)
        assert np.all(off[name] % 2 == 0), name
        assert np.all(reserved[name] >= 0), name
        assert np.all(off[name] == total), name
        total += reserved[name]
    assert np.array_equal(off["end"], total) and np.all(off["end"] % 2 == 0)


def earlier_layout(f, z):
    """The rules of the adapter's reserve function before the layout moved into the header, array by array in its order."""
    B, N, M, ns, n_obs, Q = z["B"], z["N"], z["M"], z["n_samples"], z["n_obs"], z["Q"]
    cov, tg, mt, trk = (f[k].astype(np.int64) for k in ("cov", "tighten", "map_tighten", "track_map"))
    fused = (f["fused"] | f["cov"] | ~f["noise"]).astype(np.int64)
    S = np.where(f["cov"], 1, z["S"])
    R = (1 - fused) * B * S
    sam = ns > 0
    samples = n_obs * ns * 3
    cm = cov * f["cmap"]
    chain = np.maximum(tg, mt)
    sizes = [
        ("x0", B * 4), ("U", B * 2 * N), ("poly", B * POLY), ("fl", B * 2),
        ("pose", np.where(sam, B * n_obs * 4 * N, M * 4 * N)), ("dim", np.where(sam, B * n_obs * 2 * N, M * 2 * N)), ("soff", B * samples),
        ("X", B * 4 * (N + 1)), ("J", B), ("iters", B), ("status", B), ("k", B * 2 * N), ("K", B * 8 * N), ("ok", B), ("delta", S * 4),
        ("Xr", R * 4 * (N + 1)), ("Ur", R * 2 * N), ("rows", R * SCORE),
        ("risk", B * np.where(sam, RRS, np.where(fused == 1, RRISK, RISK))), ("total", B), ("pair", 2 + 0 * B),
        ("score", fused * B * SCORE), ("base", fused * B), ("hits", fused * ((B * N + 1) // 2)),
        ("mrisk", fused * B * MAPR), ("mtotal", fused * B), ("mhits", fused * ((B * N + 1) // 2)), ("munk", fused * ((B * N + 1) // 2)),
        ("s0", cov * 16), ("W", cov * 16), ("crisk", cov * B * CHANCE), ("cstep", cov * B * N), ("ccov", cov * f["cov_judge"] * M * N * 3),
        ("csig", cm * B * (N + 1) * 16), ("qn", cm * Q * 3), ("qw", cm * Q), ("cmrisk", cm * B * CMAP), ("cmstep", cm * B * N), ("cmtotal", cm * B),
        ("ts0", chain * 16), ("tW", chain * 16), ("tsig", chain * B * (N + 1) * 16), ("trisk", chain * B * CHANCE),
        ("tpose", tg * B * M * 4 * N), ("tdim", tg * B * M * 2 * N), ("tg", tg * B * TIGHTEN), ("tcov", tg * M * N * 3),
        ("tmg", mt * B * TMAP), ("tkcov", trk * M * N * 3), ("tkf", trk * B * TRACK),
    ]
    off, o = {}, np.zeros(len(B), dtype=np.int64)
    for name, doubles in sizes:
        off[name] = o.copy()
        o += (doubles + 1) & ~1
    off["end"] = o
    return off


def test_existing_modes_keep_every_offset(layouts):
    """Without the sample covariance check, which had a block of its own, the block neither grows nor reorders."""
    f, z, _, off, _ = layouts
    was = ~f["scov"]
    want = earlier_layout(f, z)
    assert was.sum() * 2 == len(was)
    for name, at in want.items():
        assert np.array_equal(off[name][was], at[was]), name
    for name in set(off) - set(want):  # what the sample covariance check added lies behind everything else, and is empty without it
        assert np.all(off[name][was] == want["end"][was]), name


def _legal(f, p):
    """The combinations a run does not refuse with std::logic_error (ilqr_adapter.h names each conflict), and that run in the block."""
    bad = (f["cov"] & f["noise"]) | (f["cov"] & f["sampled"]) | (f["scov"] & f["noise"]) | (f["scov"] & ~f["sampled"])
    bad |= (f["tighten"] | f["map_tighten"]) & f["sampled"]
    bad |= f["sampled"] & ~f["scov"] & ~f["fused"]  # the stored-rows check has no sampled form
    bad |= f["track_map"] & f["tracks"] & f["map_set"] & f["sampled"]
    return p["in_block"] & ~bad


def _needs(f, z, p):
    """[(stage runs, {array: doubles it reads or writes})] for a run of B = max_candidates candidates, from the C-ABI's signatures."""
    B, N, M, Q, n_obs, ns = z["B"], z["N"], z["M"], z["Q"], z["n_obs"], z["n_samples"]
    S = np.where(f["cov"], 1, z["S"])  # the covariance check rolls out ONE zero offset for the map risk call
    yes, ints, steps = np.ones(len(B), dtype=bool), (B + 1) // 2, (B * N + 1) // 2
    sam, nominal = f["sampled"], ~f["sampled"]
    gains = dict(X=B * 4 * (N + 1), U=B * 2 * N, poly=B * POLY, fl=B * 2, k=B * 2 * N, K=B * 8 * N, ok=ints)
    chain = p["obstacle_rounds"] | p["map_rounds"]
    sigma = B * (N + 1) * 16
    chance = dict(s0=16 + 0 * B, W=16 + 0 * B, crisk=B * CHANCE, total=B, K=B * 8 * N)
    return [
        (yes, dict(x0=B * 4, U=B * 2 * N, poly=B * POLY, fl=B * 2, X=B * 4 * (N + 1), J=B, iters=ints, status=ints, pair=2 + 0 * B)),
        (sam, dict(pose=B * n_obs * 4 * N, dim=B * n_obs * 2 * N, soff=B * n_obs * ns * 3)),
        (nominal, dict(pose=M * 4 * N, dim=M * 2 * N)),
        (chain, dict(gains, ts0=16 + 0 * B, tW=16 + 0 * B, tsig=sigma, trisk=B * CHANCE)),
        (p["obstacle_rounds"], dict(tsig=sigma, tpose=B * M * 4 * N, tdim=B * M * 2 * N, tg=B * TIGHTEN, tcov=M * N * 3)),
        (p["map_rounds"], dict(tsig=sigma, tmg=B * TMAP)),
        (p["track_rounds"], dict(tkcov=M * N * 3, tkf=B * TRACK)),
        (p["scored"] & p["plain"], dict(score=B * SCORE, total=B)),
        (p["scored"] & ~p["plain"], dict(score=B * SCORE, base=B)),
        (p["gains"], gains),
        (p["stored_rows_risk"], dict(delta=S * 4, Xr=B * S * 4 * (N + 1), Ur=B * S * 2 * N, rows=B * S * SCORE, risk=B * RISK, total=B)),
        (p["fused_risk"], dict(delta=S * 4, base=B, risk=B * RRISK, hits=steps, total=B)),
        (p["fused_sampled_risk"], dict(delta=S * 4, base=B, risk=B * RRS, hits=steps, total=B)),
        (p["chance"], chance),
        (p["chance"] & f["cov"], dict(cstep=B * N)),
        (p["chance"] & f["cov"] & f["cov_judge"] & f["obstacles"], dict(ccov=M * N * 3)),
        (p["chance"] & (f["scov"] | p["map_covariance"]), dict(csig=sigma)),
        (p["chance_sampled"], dict(csig=sigma, srisk=B * CRS, stotal=B)),
        (p["map_covariance"], dict(csig=sigma, qn=Q * 3, qw=Q, cmrisk=B * CMAP, cmtotal=B)),
        (p["map_covariance"] & f["cov"], dict(cmstep=B * N)),
        (p["map_rollout_risk"], dict(delta=S * 4, k=B * 2 * N, K=B * 8 * N, mrisk=B * MAPR, mhits=steps, munk=steps, mtotal=B)),
    ]


def test_every_stage_finds_its_arrays_reserved(layouts, dump):
    """For every scene a run may meet (pick, map set, obstacles set, tracks set) the stages that CandidateModes says run find the full
    size of every array they touch; and each check's base is a total that a stage before it wrote."""
    f, z, _, _, reserved = layouts
    ran = {}
    for scene in itertools.product((False, True), repeat=len(RUN_FLAGS)):
        g = dict(f)
        for name, on in zip(RUN_FLAGS, scene):
            g[name] = np.full(len(z["B"]), on)
        p, _, reserved_now = dump(g, z)
        legal = _legal(g, p)
        for i, (runs, arrays) in enumerate(_needs(g, z, p)):
            rows = runs & legal
            ran[i] = ran.get(i, 0) + int(rows.sum())
            for name, doubles in arrays.items():
                short = rows & (reserved_now[name] < doubles)
                assert not short.any(), (i, name, {k: int(v[short][0]) for k, v in {**g, **z}.items()})
        # the order of the chain: a score before a check that takes a base, the chance call before what reads its Sigma_t
        assert not (legal & (p["fused_risk"] | p["fused_sampled_risk"] | p["chance_sampled"]) & ~p["scored"]).any()
        assert not (legal & (p["chance_sampled"] | p["map_covariance"]) & ~p["chance"]).any()
        assert not (legal & ~p["plain"] & ~p["gains"]).any()
    assert all(n > 0 for n in ran.values()), ran  # every stage ran in some legal combination: none of the rows above is vacuous
