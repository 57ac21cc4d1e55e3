"""GPU box: host-to-host time of bringing the keyframes of a message onto the device on a synthetic vocabulary of ORBvoc's shape (k = 10, L = 6,
levelsup = 4), per workload: 1 x 1 000 features, 40 x 1 000 (a full message), 40 x 2 000 (initialisation keyframes: the keyframe kernel's 128 KB form), 500 x 1 000
(a loaded map).  Routes, interleaved within every repetition, each
reported as median and the 10th .. 90th percentile, all through the Python wrappers with the profiler off; every route starts from an empty store:
    ingest_us       KeyFrameStore.ingest: ccm_kfstore_ingest, one upload, three launches, one download
    today_us        today's route: per keyframe matcher.Vocabulary.transform (ccm_bow_transform and the wrapper's host accumulation), then one batched add and one
                    set_featvec per key
    today_calls_us  the device calls of today's route alone (ccm_bow_transform per keyframe, add, set_featvec per key) on vectors prepared beforehand: what today's
                    route costs at the least, whatever accumulates on the host
    host_1_us       the host evaluator on one thread (csrc/kfingest_math.h) on a host-only store
REPS = 200 after WARM = 10 for every device route of every workload; the host evaluator alone runs in the first 20 repetitions only (after one of the warm-up) on
the loaded map, where one call of it takes over half a second (its count is in the JSON as host_reps).  The routes must
return the same vectors: asserted.  Also per workload the bytes each device route uploads.  Prints one JSON line; --out FILE also writes it there.

Kernel time: `rocprofv3 --kernel-trace --stats -d DIR -o kfi -- python scripts/kfingest_profile.py --device-only`, then
`python scripts/kfingest_profile.py --from-trace DIR/kfi_results.db --out profiles/kfingest_profile_traced.json`: the median per workload of the three kernels of the
ingest and of bow_descend_kernel (per launch, one keyframe) over the timed calls of the --device-only mode.  Compare only figures of one invocation on one box."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import fuse_sim3 as fs, kfstore as ks, matcher, synth
from ccm_slam_amd._lib import Context, _p, check, lib

REPS, WARM = 200, 10
SIZES = {"1x1000": (1, 1000, REPS), "40x1000": (40, 1000, REPS), "40x2000": (40, 2000, REPS), "500x1000": (500, 1000, 20)}   # keyframes, features, host_1_us repetitions
LEVELSUP = 4
REC = fs.kf_record(np.array(synth.EUROC_K, np.float32), fs.BOUNDS)


def orbvoc_shape(k=10, L=6, seed=0, stop_frac=0.02):
    """synth.make_vocabulary's tree at ORBvoc's size, its descriptors drawn level by level in slices (the one-piece form needs gigabytes at a million leaves)"""
    rng = np.random.default_rng(seed)
    n_nodes = (k ** (L + 1) - 1) // (k - 1)
    n_inner = (k ** L - 1) // (k - 1)
    child_off = np.zeros(n_nodes + 1, np.int32)
    child_off[1:n_inner + 1] = np.arange(1, n_inner + 1) * k
    child_off[n_inner + 1:] = n_inner * k
    desc = np.zeros((n_nodes, 32), np.uint8)
    desc[0] = rng.integers(0, 256, 32, dtype=np.uint8)
    start = 1
    for lvl in range(1, L + 1):
        for a in range(start, start + k ** lvl, 50000):
            ids = np.arange(a, min(a + 50000, start + k ** lvl))
            bits = np.unpackbits(desc[(ids - 1) // k], axis=1)
            desc[ids] = np.packbits(bits ^ (rng.random(bits.shape) < 0.12), axis=1)
        start += k ** lvl
    word_id = -np.ones(n_nodes, np.int32)
    word_id[n_inner:] = np.arange(n_nodes - n_inner)
    weight = np.zeros(n_nodes)
    weight[n_inner:] = rng.uniform(0.5, 6.0, n_nodes - n_inner)
    weight[n_inner:][rng.random(n_nodes - n_inner) < stop_frac] = 0.0
    return dict(n_nodes=n_nodes, L=L, child_off=child_off, child_id=np.arange(1, n_inner * k + 1, dtype=np.int32), node_desc=desc, word_id=word_id, weight=weight)


def workload(v, M, n, seed=1):
    """M keyframes of n features: descriptors of random nodes with 5 % of the bits flipped"""
    rng = np.random.default_rng(seed)
    F = M * n
    desc = np.zeros((F, 32), np.uint8)
    for a in range(0, F, 50000):
        bits = np.unpackbits(v["node_desc"][rng.integers(1, v["n_nodes"], min(50000, F - a))], axis=1)
        desc[a:a + 50000] = np.packbits(bits ^ (rng.random(bits.shape) < 0.05), axis=1)
    xy = np.stack([rng.uniform(0, 752, F), rng.uniform(0, 480, F)], 1).astype(np.float32)
    return dict(M=M, n=n, keys=np.arange(1, M + 1, dtype=np.int64), rec=np.tile(REC, M), off=(np.arange(M + 1) * n).astype(np.int32), xy=xy,
                oct=rng.integers(0, 8, F).astype(np.uint8), desc=desc)


def _ingest(store, voc, w):
    store.clear()
    return store.ingest(voc, w["keys"], w["rec"], w["off"], w["xy"], w["oct"], w["desc"], levelsup=LEVELSUP)


def _today(store, voc, w):
    store.clear()
    out = []
    for m in range(w["M"]):
        _, _, _, ids, vals, fv = voc.transform(w["desc"][m * w["n"]:(m + 1) * w["n"]], LEVELSUP)
        out.append(dict(bow_word=ids, bow_value=vals, fv_node=fv[0], fv_off=fv[1], fv_idx=fv[2]))
    store.add(w["keys"], w["rec"], w["off"], w["xy"], w["oct"], w["desc"])
    for m in range(w["M"]):
        store.set_featvec(int(w["keys"][m]), (out[m]["fv_node"], out[m]["fv_off"], out[m]["fv_idx"]))
    return out


def _today_calls(store, voc, w, vectors, scratch):
    store.clear()
    word, wt, node = scratch
    for m in range(w["M"]):
        check(lib().ccm_bow_transform(voc._h, _p(w["desc"][m * w["n"]:(m + 1) * w["n"]]), w["n"], LEVELSUP, _p(word), _p(wt), _p(node)), voc.ctx.handle)
    store.add(w["keys"], w["rec"], w["off"], w["xy"], w["oct"], w["desc"])
    for m in range(w["M"]):
        store.set_featvec(int(w["keys"][m]), (vectors[m]["fv_node"], vectors[m]["fv_off"], vectors[m]["fv_idx"]))


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[f], y[f]) for x, y in zip(a, b) for f in ("bow_word", "fv_node", "fv_off", "fv_idx")) and \
        all(np.array_equal(np.asarray(x["bow_value"], np.float64).view(np.uint64), np.asarray(y["bow_value"], np.float64).view(np.uint64)) for x, y in zip(a, b))


def _interleaved(fns, reps_of):
    """every route in every repetition it has a share in: route k runs in the first reps_of[k] repetitions (and in as large a share of the warm-up)"""
    for i in range(WARM):
        for k, f in fns.items():
            if i * REPS < reps_of[k] * WARM:
                f()
    t_ = {k: [] for k in fns}
    for i in range(REPS):
        for k, f in fns.items():
            if i >= reps_of[k]:
                continue
            t = time.perf_counter()
            f()
            t_[k].append(time.perf_counter() - t)
    us = lambda x, q: round(1e6 * float(np.percentile(x, q)), 1)
    return {k: dict(median=us(x, 50), p10=us(x, 10), p90=us(x, 90)) for k, x in t_.items()}


def routes(ctx, v, voc, name):
    M, n, host_reps = SIZES[name]
    w = workload(v, M, n)
    F = M * n
    stores = [ks.KeyFrameStore(ctx, M, n) for _ in range(3)] + [ks.KeyFrameStore(None, M, n)]
    info = {}
    info["host"] = _ingest(stores[3], v, w)
    scratch = (np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32))

    def new():
        info["dev"] = _ingest(stores[0], voc, w)

    def old():
        info["today"] = _today(stores[1], voc, w)

    def calls():
        _today_calls(stores[2], voc, w, info["host"], scratch)

    def on_host():
        info["host"] = _ingest(stores[3], v, w)
    r = _interleaved(dict(ingest_us=new, today_us=old, today_calls_us=calls, host_1_us=on_host),
                     dict(ingest_us=REPS, today_us=REPS, today_calls_us=REPS, host_1_us=host_reps))
    agree = _same(info["dev"], info["host"]) and _same(info["dev"], info["today"])
    assert agree, f"{name}: the routes do not return the same vectors"
    for s in stores:
        s.close()
    nn = sum(int(x["fv_node"].size) for x in info["host"]); kept = sum(int(x["fv_off"][-1]) for x in info["host"])
    common = 32 * F + 8 * F + F + 40 * M + 4 * (M + 1)      # descriptors, xy, octaves, records, offsets
    return dict(size=name, keyframes=M, features=F, reps=REPS, warm=WARM, host_reps=host_reps, words=sum(int(x["bow_word"].size) for x in info["host"]), nodes=nn, kept=kept,
                routes_agree=bool(agree), up_bytes_ingest=common + 4 * M, up_bytes_today=common + 4 * M + 32 * F + 4 * nn + 4 * (nn + M) + 2 * kept, **r)


KERNELS = ("kfstore_add_kernel", "kfi_descend_kernel", "kfi_vectors_kernel", "bow_descend_kernel")


def device_only():
    ctx = Context(0)
    v = orbvoc_shape()
    voc = matcher.Vocabulary(ctx, v)
    for name, (M, n, _) in SIZES.items():
        reps, warm = REPS, WARM
        w = workload(v, M, n)
        a, b = ks.KeyFrameStore(ctx, M, n), ks.KeyFrameStore(ctx, M, n)
        vectors = _ingest(a, voc, w)
        scratch = (np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32))
        for _ in range(warm + reps - 1):
            _ingest(a, voc, w)
        for _ in range(warm + reps):
            _today_calls(b, voc, w, vectors, scratch)
        a.close(); b.close()
    voc.close(); ctx.close()


def from_trace(db_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    launches = list(db.execute("select name, duration from kernels order by start"))
    seq = {k: [x for n, x in launches if k in n] for k in KERNELS}
    pos = {k: 0 for k in KERNELS}
    med = lambda x: dict(median=round(float(np.median(x)) / 1e3, 1), p10=round(float(np.percentile(x, 10)) / 1e3, 1), p90=round(float(np.percentile(x, 90)) / 1e3, 1))

    def take(k, count, skip):
        d = seq[k][pos[k]:pos[k] + count]
        if len(d) != count:
            raise SystemExit(f"trace holds too few launches of {k}")
        pos[k] += count
        return med(np.array(d[skip:]))
    rows = []
    for name, (M, n, _) in SIZES.items():
        reps, warm = REPS, WARM
        per = warm + reps
        row = dict(size=name)
        row["ingest_add_us"] = take("kfstore_add_kernel", per, warm)
        row["ingest_descend_us"] = take("kfi_descend_kernel", per, warm)
        row["ingest_vectors_us"] = take("kfi_vectors_kernel", per, warm)
        row["today_add_us"] = take("kfstore_add_kernel", per, warm)
        row["today_descend_per_keyframe_us"] = take("bow_descend_kernel", per * M, warm * M)
        rows.append(row)
    line = json.dumps(dict(kernel_source="rocprofv3 --kernel-trace --stats of scripts/kfingest_profile.py --device-only", rows=rows))
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
    ctx = Context(0)
    v = orbvoc_shape()
    voc = matcher.Vocabulary(ctx, v)
    only = arg("--only")
    rows = [routes(ctx, v, voc, name) for name in SIZES if only in (None, name)]
    voc.close(); ctx.close()
    line = json.dumps(dict(vocabulary="synthetic, k = 10, L = 6, levelsup = 4", rows=rows))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
