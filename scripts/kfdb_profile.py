"""GPU box: per-query time of the device keyframe database (ccm_kfdb_query) at 2 000 and 10 000 keyframes of 800 words over a 10^6-word
vocabulary, host to host (wall clock around the call, median of many queries), without a filter and with DetectLoopCandidates' filter (the
query itself, the whole map as allow list, 10 connected keyframes).  Device-only time: run it under
`rocprofv3 --kernel-trace --stats -- python scripts/kfdb_profile.py` and add the kfdb_count / kfdb_select / kfdb_score rows per query.
Prints one JSON line; --out FILE also writes it there."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd._lib import Context
from ccm_slam_amd.kfdb import KeyFrameDatabase

N_WORDS, WORDS_PER_KF, N_QUERIES = 1_000_000, 800, 200


def make_kf(rng, base):
    b = base[int(rng.integers(0, len(base)))]
    w = np.unique(np.concatenate([b[rng.random(b.size) < 0.8], rng.choice(N_WORDS, WORDS_PER_KF // 5)]))[:WORDS_PER_KF].astype(np.int32)
    v = rng.uniform(0.05, 1.0, w.size)
    return w, v / v.sum()


def run(ctx, n_kf, rng):
    base = [rng.choice(N_WORDS, WORDS_PER_KF, replace=False) for _ in range(max(n_kf // 20, 1))]
    db = KeyFrameDatabase(ctx, N_WORDS)
    keys = []
    t0 = time.perf_counter()
    for i in range(n_kf):
        db.add(i << 8 | (i % 4), i % 4, *make_kf(rng, base))
        keys.append(i << 8 | (i % 4))
    t_add = (time.perf_counter() - t0) / n_kf
    queries = [make_kf(rng, base) for _ in range(N_QUERIES)]
    out = {}
    keys = np.asarray(keys, np.int64)
    for name, kw in (("plain", {}), ("loop_filter", dict(self_key=int(keys[0]), allow=keys, exclude=keys[1:11]))):
        for q in queries[:10]:
            db.query(*q, **kw)
        ts, rows = [], []
        for q in queries:
            t = time.perf_counter()
            r = db.query(*q, **kw)
            ts.append(time.perf_counter() - t)
            rows.append(r["key"].size)
        out[name] = dict(median_us=round(1e6 * float(np.median(ts)), 1), p90_us=round(1e6 * float(np.percentile(ts, 90)), 1),
                         mean_rows=round(float(np.mean(rows)), 1))
    db.close()
    return dict(n_kf=n_kf, add_us=round(1e6 * t_add, 1), **out)


def main():
    rng = np.random.default_rng(0)
    ctx = Context(0)
    res = dict(words_per_kf=WORDS_PER_KF, n_words=N_WORDS, queries=N_QUERIES, runs=[run(ctx, n, rng) for n in (2000, 10000)])
    ctx.close()
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
