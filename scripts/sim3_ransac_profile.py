"""GPU box: host-to-host time of the Sim3 RANSAC (ccm_sim3_ransac_eval, cslam::Sim3RansacBatch) for K candidates of N correspondences,
K in {1, 4, 8, 16}, N in {50, 200, 1000}, median of repeated runs:
  pass     one ccm_sim3_ransac_eval of 300 hypotheses per candidate (the whole schedule of a ComputeSim3 in which no candidate succeeds)
  compute  a whole ComputeSim3 through Sim3RansacBatch in which every candidate fails: create + next() until every candidate is discarded
           (300 x K hypotheses, mSolverIterations = 5)
  iterate5 one Sim3Solver::iterate(5) of the drop-in shim/Sim3Solver_hip.cpp path (ccmh_sim3_solver_iterate: one launch of 5 hypotheses) on a
           candidate that never succeeds
Prints one JSON line; --out FILE also writes it there.  Each run records how many sim3_ransac_kernel launches it made, in order.
Device time per configuration: run the script under `rocprofv3 --kernel-trace -d DIR -o sim3 -- python scripts/sim3_ransac_profile.py --out A.json`,
then `python scripts/sim3_ransac_profile.py --from-trace DIR/sim3_results.db --runs A.json --out B.json --stats-csv C.csv`: the trace's
sim3_ransac_kernel dispatches are split by those counts, B.json is A.json with the median kernel time of each phase added (pass_kernel_us,
compute_pass_kernel_us, iterate5_kernel_us), and C.csv is the trace's per-kernel summary in rocprofv3's --stats layout."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import sim3, synth
from ccm_slam_amd._lib import Context, check, lib

REPS = 30


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run(ctx, K, N, rng):
    cands = [sim3.Sim3Candidate(**d) for d in synth.make_sim3_candidates(K * 1000 + N, 0, K, N, 1.0)]
    pt_off, X1, X2, K1, K2, t1, t2, _, _ = sim3.pack(cands)
    H = 300 * K
    hc = np.repeat(np.arange(K, dtype=np.int32), 300)
    hi = np.stack([rng.choice(N, 3, replace=False) for _ in range(H)]).astype(np.int32)
    n_inl = np.zeros(H, np.int32); rts = np.zeros(13 * H, np.float32); mask_off = np.zeros(H + 1, np.int32)
    mask = np.zeros(H * ((N + 31) // 32), np.uint32)
    args = (ctx.handle, K, _p(pt_off), _p(X1), _p(X2), _p(K1), _p(K2), _p(t1), _p(t2), H, _p(hc), _p(hi), 0, _p(n_inl), _p(rts), _p(mask_off), _p(mask))
    f = lib().ccm_sim3_ransac_eval
    for _ in range(3):
        check(f(*args), ctx.handle)
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        check(f(*args), ctx.handle)
        ts.append(time.perf_counter() - t)
    t_pass = float(np.median(ts))
    draws = rng.integers(0, 2 ** 31, 3 * H + 16).astype(np.int32)
    tc, hyps = [], 0
    for r in range(REPS // 3 + 2):   # every failing ComputeSim3 is one pass: one launch each
        sim3.clear_draws()
        t = time.perf_counter()
        b = sim3.Sim3Ransac(cands, draws=draws)
        while b.next() is not None:
            pass
        dt = time.perf_counter() - t
        hyps = b.stats()[1]
        b.close()
        if r >= 2:
            tc.append(dt)
    sim3.clear_draws()
    n_compute = REPS // 3 + 2
    # the drop-in path: iterate(5) on the first (failing) candidate; a fresh solver when it runs out of iterations
    ti, n_iter = [], 0
    solver = sim3.Sim3Solver(cands[0])
    for r in range(REPS + 3):
        t = time.perf_counter()
        ok, no_more, _, _ = solver.iterate(5)
        dt = time.perf_counter() - t
        n_iter += 1
        if r >= 3:
            ti.append(dt)
        if no_more:
            solver = sim3.Sim3Solver(cands[0])
    sim3.clear_draws()
    return dict(K=K, N=N, hypotheses=H, pass_us=round(1e6 * t_pass, 1), compute_us=round(1e6 * float(np.median(tc)), 1), compute_hypotheses=int(hyps),
                iterate5_us=round(1e6 * float(np.median(ti)), 1),
                launches=dict(pass_warm=3, pass_timed=REPS, compute_warm=2, compute_timed=n_compute - 2, iterate5_warm=3, iterate5_timed=REPS))


def from_trace(db_path, runs_path, out_path, csv_path):
    """split the trace's sim3_ransac_kernel dispatches (in start order) by the launch counts each run recorded; add the median of each phase"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, duration from kernels order by start"))
    res = json.load(open(runs_path))
    k = [d for n, d in rows if "sim3_ransac_kernel" in n]
    need = sum(sum(r["launches"].values()) for r in res["runs"])
    if len(k) != need:
        raise SystemExit(f"trace holds {len(k)} sim3_ransac_kernel launches, the runs recorded {need}")
    o = 0
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    for r in res["runs"]:
        L = r["launches"]
        seg = {}
        for phase in ("pass", "compute", "iterate5"):
            o += L[phase + "_warm"]
            seg[phase] = k[o:o + L[phase + "_timed"]]
            o += L[phase + "_timed"]
        r["pass_kernel_us"], r["compute_pass_kernel_us"], r["iterate5_kernel_us"] = med(seg["pass"]), med(seg["compute"]), med(seg["iterate5"])
    res["kernel_source"] = "rocprofv3 --kernel-trace of the same script, medians per phase (scripts/sim3_ransac_profile.py --from-trace)"
    line = json.dumps(res)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    if csv_path:
        by = {}
        for n, d in rows:
            by.setdefault(n, []).append(d)
        tot = sum(sum(v) for v in by.values())
        with open(csv_path, "w") as f:
            f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n')
            for n, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
                v = np.array(v, float)
                f.write('"%s",%d,%d,%f,%.2f,%d,%d,%f\n' % (n, len(v), v.sum(), v.mean(), 100 * v.sum() / tot, v.min(), v.max(), v.std()))


def main():
    if "--from-trace" in sys.argv:
        arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
        from_trace(arg("--from-trace"), arg("--runs"), arg("--out"), arg("--stats-csv"))
        return
    rng = np.random.default_rng(0)
    ctx = Context(0)
    runs = [run(ctx, K, N, rng) for K in (1, 4, 8, 16) for N in (50, 200, 1000)]
    ctx.close()
    line = json.dumps(dict(reps=REPS, runs=runs))
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
