"""GPU box: time of the keyframe culling walk (ccm_kfcull_walk) at the two sizes of ccm_slam_amd.culling.SIZES on a redundant-rich neighbourhood with thres = 0.98,
median of interleaved repetitions (device call, host evaluator, map-copy model, device call, ... on one box):
  call_us    ccm_kfcull_walk host to host: checks, packing, one H2D copy, two launches, one D2H copy, unpacking
  host_us    the same arguments through kfcull_math.h compiled for the host, on one thread (ccmh_kfcull_walk_host)
  model_us   the same walk on std::map observations that are copied for every checked slot of every candidate, as the reference's GetObservations() does
             (ccmh_kfcull_walk_mapcopy_model): a MODEL of the reference's containers without its mutexes, shared_ptr counts and graph updates, not the reference
All go through the same ctypes binding, whose cost (array checks, output allocation) is in every figure.  Compare only rows of one run.
Prints one JSON line; --out FILE also writes it there (profiles/kfcull_profile.json).
Device time, in a run of its own: `rocprofv3 --kernel-trace --stats -d DIR -o kc -- python scripts/kfcull_profile.py --out A.json`, then
`python scripts/kfcull_profile.py --from-trace DIR/kc_results.db --runs A.json --out B.json`: the trace's launches are split by the call counts each size recorded
(two launches per call); B.json is A.json with the median per call of each kernel."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import culling as K
from ccm_slam_amd._lib import Context

REPS = 15
WARM = 2
THRES = 0.98
PER_CALL = ("kfcull_eval_kernel", "kfcull_walk_kernel")


def run(ctx, size):
    sc = K.profile_scene(size)
    dev, host, model = [], [], []
    for i in range(WARM + REPS):
        t = time.perf_counter(); d = K.walk(ctx, sc, thres=THRES); a = time.perf_counter() - t
        t = time.perf_counter(); h = K.walk_host(sc, thres=THRES); b = time.perf_counter() - t
        t = time.perf_counter(); m = K.walk_mapcopy_model(sc, thres=THRES); c = time.perf_counter() - t
        assert all(np.array_equal(d[k], h[k]) for k in ("verdict", "n_mps", "n_red", "pt_gone", "pt_nobs_out")) and d["n_reeval"] == h["n_reeval"]
        assert np.array_equal(m, h["verdict"])
        if i >= WARM:
            dev.append(a); host.append(b); model.append(c)
    call, hst, mdl = (1e6 * float(np.median(v)) for v in (dev, host, model))
    return dict(size=size, candidates=int(sc["n_cand"]), keyframes_all=int(sc["n_all"]), slots=int(sc["list_pt"].size), points=int(sc["n_pt"]),
                observations=int(sc["obs_kf"].size), thres=THRES, culled=int((d["verdict"] == K.CULLED).sum()), reevaluated=d["n_reeval"],
                points_gone=int(d["pt_gone"].sum() - np.asarray(sc["pt_bad"]).sum()), call_us=round(call, 1), host_us=round(hst, 1), model_us=round(mdl, 1),
                host_over_call=round(hst / call, 2), model_over_call=round(mdl / call, 2), calls=dict(untimed=WARM, timed=REPS))


def from_trace(db_path, runs_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = [(n, d) for n, d in db.execute("select name, duration from kernels order by start") if "kfcull_" in n]
    res = json.load(open(runs_path))
    n_call = len(PER_CALL)
    if len(rows) % n_call or any(PER_CALL[k % n_call] not in rows[k][0] for k in range(len(rows))):
        raise SystemExit("the trace's kfcull launches are not whole calls of two")
    calls = [rows[k:k + n_call] for k in range(0, len(rows), n_call)]
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    o = 0
    for r in res["runs"]:
        o += r["calls"]["untimed"]
        mine = calls[o:o + r["calls"]["timed"]]; o += r["calls"]["timed"]
        r["eval_kernel_us"] = med([c[0][1] for c in mine])
        r["walk_kernel_us"] = med([c[1][1] for c in mine])
        r["kernels_us"] = med([c[0][1] + c[1][1] for c in mine])
    if o > len(calls):
        raise SystemExit(f"trace holds {len(calls)} calls, the runs recorded {o}")
    res["kernel_source"] = "rocprofv3 --kernel-trace of the same script, medians per size (scripts/kfcull_profile.py --from-trace)"
    line = json.dumps(res)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def main():
    if "--from-trace" in sys.argv:
        arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
        from_trace(arg("--from-trace"), arg("--runs"), arg("--out"))
        return
    ctx = Context(0)
    runs = [run(ctx, s) for s in ("local", "wide")]
    ctx.close()
    line = json.dumps(dict(reps=REPS, runs=runs))
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
