"""GPU box: host-to-host time of the two-view initialiser's two device calls against the host evaluator, per size:
  ransac   N = 100 / 300 / 1000 matches, H = 200 hypotheses
    device    ccm_twoview_ransac_eval, host to host through the Python wrapper
    host_1    the same arguments through twoview_math.h compiled for the host, one thread
    host_2    H and F on two threads, as the reference runs FindHomography / FindFundamental: the BASELINE
  check_rt N = 300 / 1000 matches under 4 and 8 motion hypotheses
    device    ccm_twoview_check_rt
    host_1    the host evaluator on one thread, as the reference runs CheckRT: the BASELINE
Each figure is the median of 15 repetitions; the candidates of a row are interleaved within every repetition.  The whole table is measured three times
(`runs`); margin_us = max - min of the baseline's three medians is what counts as a difference in that row.  Compare only figures of one invocation.
Prints one JSON line; --out FILE also writes it there (profiles/twoview_profile.json).
Device time: `rocprofv3 --kernel-trace --stats -d DIR -o tv -- python scripts/twoview_profile.py --device-only`, then
`python scripts/twoview_profile.py --from-trace DIR/tv_results.db --out B.json`: the medians of the three kernels per row, split by the launch counts
of the --device-only run (3 warm-up + 15 timed calls per row, in the order of the table)."""
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import twoview as tv
from ccm_slam_amd._lib import Context

REPS = 15
WARM = 3
RANSAC = [(100, 200), (300, 200), (1000, 200)]
CHECK_RT = [(300, 4), (300, 8), (1000, 4), (1000, 8)]


def _interleaved(fs):
    """medians (us) of the callables of `fs`, each called once per repetition, in turn"""
    for _ in range(WARM):
        for f in fs.values():
            f()
    ts = {k: [] for k in fs}
    for _ in range(REPS):
        for k, f in fs.items():
            t = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t)
    return {k: round(1e6 * float(np.median(v)), 1) for k, v in ts.items()}


def _two_threads(a, sets):
    def f():
        th = [threading.Thread(target=tv.ransac_eval_host, args=(*a, 1.0, sets, m)) for m in (1, 2)]   # ctypes releases the GIL for the call
        for t in th:
            t.start()
        for t in th:
            t.join()
    return f


def ransac_case(N, H):
    sc = tv.make_scene("general", N, seed=900 + N, unmatched=N // 4, outliers=0.1)
    return tv.ransac_inputs(sc), tv.random_sets(N, H, N)


def check_rt_case(N, Q):
    sc = tv.make_scene("general", N, seed=900 + N, unmatched=N // 4, outliers=0.1)
    Rs, ts = tv.motion_hypotheses(sc, Q)
    rec = np.stack([tv.prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(Q)])
    return rec, sc["K"], sc["xy1"], sc["xy2"], np.ones(N, bool), 4.0


def one_run(ctx):
    rows = []
    for N, H in RANSAC:
        a, sets = ransac_case(N, H)
        r = _interleaved(dict(device_us=lambda: tv.ransac_eval(ctx, *a, 1.0, sets), host_1_us=lambda: tv.ransac_eval_host(*a, 1.0, sets),
                              host_2_us=_two_threads(a, sets)))
        rows.append(dict(call="ransac", N=N, H=H, baseline="host_2_us", **r))
    for N, Q in CHECK_RT:
        c = check_rt_case(N, Q)
        r = _interleaved(dict(device_us=lambda: tv.check_rt(ctx, *c), host_1_us=lambda: tv.check_rt_host(*c)))
        rows.append(dict(call="check_rt", N=N, n_hyp=Q, baseline="host_1_us", **r))
    return rows


def device_only():
    ctx = Context(0)
    for N, H in RANSAC:
        a, sets = ransac_case(N, H)
        for _ in range(WARM + REPS):
            tv.ransac_eval(ctx, *a, 1.0, sets)
    for N, Q in CHECK_RT:
        c = check_rt_case(N, Q)
        for _ in range(WARM + REPS):
            tv.check_rt(ctx, *c)
    ctx.close()


def from_trace(db_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, duration from kernels order by start"))
    pick = lambda key: [d for n, d in rows if key in n]
    solve, score, rt = pick("twoview_solve_kernel"), pick("twoview_score_kernel"), pick("twoview_check_rt_kernel")
    per = WARM + REPS
    if len(solve) != per * len(RANSAC) or len(score) != len(solve) or len(rt) != per * len(CHECK_RT):
        raise SystemExit(f"trace holds {len(solve)} / {len(score)} / {len(rt)} launches, expected {per * len(RANSAC)} / {per * len(RANSAC)} / {per * len(CHECK_RT)}")
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    out = []
    for i, (N, H) in enumerate(RANSAC):
        s = slice(i * per + WARM, (i + 1) * per)
        out.append(dict(call="ransac", N=N, H=H, solve_kernel_us=med(solve[s]), score_kernel_us=med(score[s])))
    for i, (N, Q) in enumerate(CHECK_RT):
        out.append(dict(call="check_rt", N=N, n_hyp=Q, check_rt_kernel_us=med(rt[i * per + WARM:(i + 1) * per])))
    line = json.dumps(dict(kernel_source="rocprofv3 --kernel-trace --stats of scripts/twoview_profile.py --device-only, medians of 15", rows=out))
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def main():
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    if "--device-only" in sys.argv:
        return device_only()
    if "--from-trace" in sys.argv:
        return from_trace(arg("--from-trace"), arg("--out"))
    runs = []
    for _ in range(3):
        ctx = Context(0)
        runs.append(one_run(ctx))
        ctx.close()
    table = []
    for i, row in enumerate(runs[0]):
        base = [r[i][row["baseline"]] for r in runs]
        keys = [k for k in row if k.endswith("_us")]
        table.append(dict({k: v for k, v in row.items() if not k.endswith("_us")}, **{k: [r[i][k] for r in runs] for k in keys},
                          margin_us=round(max(base) - min(base), 1)))
    line = json.dumps(dict(reps=REPS, runs=3, rows=table))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
