"""Where a host-buffer call's arrays lie in the handle's device arena (csrc/cilqr_host_plan.h) is plain integer arithmetic on the
host: checked here without a GPU through tests/cpp/host_plan_dump.cpp, for every host form over a grid of small shapes, together
with the arena cilqr_create reserves (tests/golden/host_arena_cap.json: the values of the commit before the single transport)."""
import itertools
import json
import os
import subprocess

import pytest

from conftest import PKG, ROOT

POLY, SCORE, RISK, RR = 6, 8, 4, 6  # CILQR_POLY_COEFFS, CILQR_SCORE_FIELDS, CILQR_RISK_FIELDS, CILQR_ROLLOUT_RISK_FIELDS (include/cilqr.h)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "host_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "host_plan_dump.cpp")], check=True)

    def run(shapes):
        args = [",".join("%s=%s" % kv for kv in s.items()) for s in shapes]
        r = subprocess.run([exe] + args, check=True, capture_output=True, text=True)
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


def span_of(B, N, M, strides):
    """Entries and weights the strides address (cilqr_solve_batch_obstacles, include/cilqr.h)."""
    bs, ms, ts, wbs = strides
    if M == 0:
        return 0, 0
    b1 = max(B - 1, 0)
    return b1 * bs + (M - 1) * ms + (N - 1) * ts + 1, b1 * wbs + M


def grid():
    """(shape given to the dump, {array: bytes expected} for inputs, in/out arrays, outputs) for the nine host forms.  The handle is
    the smallest that takes the call: max_batch = B (B*S rows for the forms that move rows), max_horizon = N, max_obstacles = M."""
    cases = []
    for B, N, M, opt, weights in itertools.product([0, 1, 3, 64], [1, 5, 50], [0, 1, 4], [0, 1], [0, 1]):
        X, U, path = B * 4 * (N + 1) * 8, B * 2 * N * 8, {"poly": B * POLY * 8, "xplan_fl": B * 2 * 8}
        solve_out = {"X_out": X, "J_out": B * 8, "iters_out": B * 4, "status_out": B * 4}  # J, iters, status: reserved even when null
        score_out = {"score": B * SCORE * 8, "total": B * 8 if opt else 0}
        for dense in (1, 0):  # dense [B][M][N] tables, or one static scene for the batch: strides (0, 1, 0), one weight vector
            span, w_span = span_of(B, N, M, (M * N, N, 1, M) if dense else (0, 1, 0, 0))
            w_span = w_span if weights else 0
            obs = {"obs_weight": w_span * 8, "obs_pose": span * 32, "obs_dim": span * 16}
            common = dict(B=B, N=N, M=M, span=span, w_span=w_span, weights=weights, opt=opt, max_B=max(B, 1), max_N=N, max_M=M)
            cases.append((dict(form="solve_batch" if dense else "solve_batch_obstacles", **common), dict(x0=B * 32, **path, **obs), {"U": U}, solve_out))
            if not dense or not weights:  # (cilqr_score_batch takes strides only; one dense case stands for (M*N, N, 1))
                cases.append((dict(form="score_batch", **common), dict(X=X, U=U, **path, **obs), {}, score_out))
            cases.append((dict(form="gains_batch", **common), dict(X=X, U=U, **path, **obs), {},
                          {"k_out": U, "K_out": B * 8 * N * 8, "ok_out": B * 4 if opt else 0}))
            for S in (1, 3):
                rows = dict(common, S=S, max_B=max(B * S, 1))
                cases.append((dict(form="score_rollouts", **rows), dict(X_roll=S * X, U_roll=S * U, **path, **obs), {},
                              {"row_score": B * S * SCORE * 8, "risk": B * RISK * 8, "total": B * 8 if opt else 0}))
                for delta_sets in (1, B):
                    gains = {"X": X, "U": U, "k": U, "K": B * 8 * N * 8, "delta": delta_sets * S * 32}
                    no_w = dict(obs, obs_weight=0)  # (the risk kernel reads no weights: they do not travel)
                    cases.append((dict(form="rollout_risk", delta_sets=delta_sets, **dict(common, S=S)), dict(gains, base=B * 8 if opt else 0, **no_w), {},
                                  {"risk": B * RR * 8, "step_hits": B * N * 4 if opt else 0, "total": B * 8 if opt else 0}))
                    if dense and not weights and M == 0:
                        cases.append((dict(form="rollout_batch", delta_sets=delta_sets, **rows), gains, {}, {"X_roll": S * X, "U_roll": S * U}))
        if M > 0 and not weights:  # the sampled forms: n_obs = 2 nominal obstacles, M stands for nothing here
            for n_samples in (2, 3):
                span = B * 2 * N
                common = dict(B=B, N=N, M=2, n_samples=n_samples, span=span, opt=opt, max_B=max(B, 1), max_N=N, max_M=2 * n_samples)
                samp = {"samp_off": B * 2 * n_samples * 24, "obs_pose": span * 32, "obs_dim": span * 16, "obs_weight": 0}
                cases.append((dict(form="solve_batch_sampled", **common), dict(x0=B * 32, **path, **samp), {"U": U}, solve_out))
                cases.append((dict(form="score_batch_sampled", **common), dict(X=X, U=U, **path, **samp), {}, score_out))
    return cases


def test_header_is_plain_cpp():
    """The plan header compiles without HIP (its only include beyond the C library is include/cilqr.h)."""
    text = open(os.path.join(PKG, "csrc", "cilqr_host_plan.h")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text and "hipMemcpy" not in text


def test_field_counts_match_the_header():
    import re
    text = open(os.path.join(ROOT, "include", "cilqr.h")).read()
    for name, want in [("POLY_COEFFS", POLY), ("SCORE_FIELDS", SCORE), ("RISK_FIELDS", RISK), ("ROLLOUT_RISK_FIELDS", RR)]:
        assert int(re.search(r"#define\s+CILQR_%s\s+(\d+)" % name, text).group(1)) == want


def test_every_host_form_over_the_grid(dump):
    cases = grid()
    assert {c[0]["form"] for c in cases} == {"solve_batch", "solve_batch_obstacles", "solve_batch_sampled", "score_batch", "score_batch_sampled",
                                             "gains_batch", "rollout_batch", "score_rollouts", "rollout_risk"}
    plans = dump([c[0] for c in cases])
    assert len(plans) == len(cases)
    for (shape, ins, inouts, outs), p in zip(cases, plans):
        assert p["ok"] == 1, shape
        entries = p["entries"]
        # 16-byte alignment, no overlap, declared back to back
        at = 0
        for off, nbytes, _, _ in entries:
            assert off % 16 == 0 and off == at and nbytes > 0, (shape, entries)
            at = (off + nbytes + 15) // 16 * 16
        assert p["end"] == at and p["end"] % 16 == 0, shape
        # inputs + in/out arrays are exactly the prefix [0, in_end), in/out arrays + outputs exactly the suffix [out_begin, end):
        # one copy each way moves a packed call
        travels_in = [(off, nbytes) for off, nbytes, i, _ in entries if i]
        reserved_out = [(off, nbytes) for off, nbytes, i, o in entries if o or not i]
        assert all(off + nbytes <= p["in_end"] for off, nbytes in travels_in) and all(off >= p["out_begin"] for off, _ in reserved_out), shape
        assert all(i for off, _, i, _ in entries if off < p["out_begin"]) and all(o or not i for off, _, i, o in entries if off >= p["in_end"]), shape
        assert p["in_end"] == (max(off + nbytes for off, nbytes in travels_in) + 15) // 16 * 16 if travels_in else p["in_end"] == 0, shape
        assert p["out_begin"] == (min(off for off, _ in reserved_out) if reserved_out else p["end"]), shape
        # every array has the size the call's documentation gives it; what is null or empty takes no place and stays null
        by_off = {off: (nbytes, i, o) for off, nbytes, i, o in entries}
        want = [(n, b, 1, 0) for n, b in ins.items()] + [(n, b, 1, 1) for n, b in inouts.items()] + [(n, b, 0, None) for n, b in outs.items()]
        assert len([w for w in want if w[1]]) == len(entries), (shape, entries)
        for name, nbytes, i, o in want:
            off = p["at"][name]
            if nbytes == 0:
                assert off == -1, (shape, name)
            else:
                assert by_off[off][0] == nbytes and by_off[off][1] == i and (o is None or by_off[off][2] == o), (shape, name, by_off[off])
        if not shape["opt"]:  # null J_out / iters_out / status_out keep their places (no copy back); other null outputs have none
            kept = {"J_out", "iters_out", "status_out"} & set(outs)
            assert all(by_off[p["at"][n]][2] == 0 for n in kept if outs[n]) and all(by_off[p["at"][n]][2] == 1 for n in outs if outs[n] and n not in kept)
        # the call fits the arena of the smallest handle that takes it
        assert p["end"] <= p["cap"], (shape, p["end"], p["cap"])


def test_a_malformed_plan_is_marked(dump):
    """Arrays declared out of order, or more of them than a plan holds: `ok` is false (the executor then refuses the call) and
    nothing is placed beyond the plan's capacity."""
    bad, full, over = dump([dict(form="declared_out_of_order"), dict(form="too_many_arrays", B=16), dict(form="too_many_arrays", B=17)])
    assert bad["ok"] == 0 and len(bad["entries"]) == 1
    assert full["ok"] == 1 and len(full["entries"]) == 16 and over["ok"] == 0 and len(over["entries"]) == 16 and over["end"] == full["end"]


def test_rollout_risk_offsets_promise(dump):
    """include/cilqr.h, cilqr_rollout_risk: "(delta_batch_stride ? B : 1)*S <= max_batch*max_horizon always fits"."""
    shapes = []
    for max_B, max_N, max_M in [(4, 5, 0), (4, 5, 2), (1, 1, 0), (1, 50, 4), (64, 50, 4), (3, 7, 1)]:
        S = max_B * max_N
        for M in {0, max_M}:
            lim = dict(N=max_N, M=M, opt=1, max_B=max_B, max_N=max_N, max_M=max_M)
            shapes.append(dict(form="rollout_risk", B=1, S=S, delta_sets=1, span=M * max_N, **lim))            # one shared set of S offsets
            shapes.append(dict(form="rollout_risk", B=max_B, S=S, delta_sets=1, span=max_B * M * max_N, **lim))  # the same, full batch
            shapes.append(dict(form="rollout_risk", B=max_B, S=max_N, delta_sets=max_B, span=max_B * M * max_N, **lim))  # dense: B*S offsets
    for s, p in zip(shapes, dump(shapes)):
        assert p["ok"] == 1 and p["end"] <= p["cap"], (s, p["end"], p["cap"])
        delta = [e for e in p["entries"] if e[0] == p["at"]["delta"]][0]
        assert delta[1] == s["delta_sets"] * s["S"] * 4 * 8


def test_arena_bytes_are_those_of_the_previous_layouts(dump):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "host_arena_cap.json")))
    cases = golden["cases"]
    assert len(cases) >= 20 and all(t in [c[:3] for c in cases] for t in ([1, 1, 0], [1, 40, 0], [64, 50, 4], [4096, 50, 4], [3, 5, 2]))
    got = dump([dict(max_B=b, max_N=n, max_M=m) for b, n, m, _ in cases])
    assert [p["cap"] for p in got] == [c[3] for c in cases]
