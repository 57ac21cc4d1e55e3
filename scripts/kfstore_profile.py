"""GPU box: host-to-host time of the resident Fuse calls (ccm_fuse_sim3_eval_resident, ccm_fuse_pose_eval_resident on a keyframe store) against
the stateless calls (ccm_fuse_sim3_eval, ccm_fuse_pose_eval) built from the same tree, through the Python wrappers, profiler off, at the three sizes of
scripts/fuse_sim3_profile.py (keyframes x points) and the three of scripts/fuse_pose_profile.py (calls x the current keyframe's points + candidates), about 1 000
features per keyframe:
    resident_us    the resident call; the keyframes were added to the store before the clock starts
    stateless_us   the existing call, which uploads every keyframe's static data again: the BASELINE
Each figure is the median of 15 repetitions; the two calls of a row are interleaved within every repetition.  The whole table is measured three times (`runs`);
margin_us = max - min of the baseline's three medians is what counts as a difference in that row, and `verdict` says on which side of it the resident call lies
(by the medians of the three medians).  Compare only figures of one invocation.
Per row also the library's three host phases of the resident call (packing; upload + kernel + download; unpacking) and its upload in bytes, from its CCM_DBG=fuse
lines: medians of a child process that makes 3 + 15 resident calls per size with that variable set.
`add`: the one-off cost of ccm_kfstore_add, which is what residency has to pay back: medians of 15 adds of M = 1 and of M = 500 keyframes (1 000 features each, grid
built on the device) through the C ABI, and through cslam::KeyFrameStore, which also builds the host shadow; per keyframe, and `calls_to_pay`: that cost over the gain
per call and keyframe of the merge_1_agent row.
Prints one JSON line; --out FILE also writes it there (profiles/kfstore_profile.json)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, kfstore as ks
from ccm_slam_amd._lib import Context, _p, check, lib

REPS = 15
WARM = 3
ROWS = [("sim3", n) for n in fs.PROFILE_SIZES] + [("pose", n) for n in fp.PROFILE_SIZES]
MAX_KF, MAX_FEAT = 1024, 1000


def _interleaved(fns):
    """medians (us) of the callables of `fns`, each called once per repetition, in turn"""
    for _ in range(WARM):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            t = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t)
    return {k: round(1e6 * float(np.median(v)), 1) for k, v in ts.items()}


def scene_of(form, name):
    return fs.profile_scene(name) if form == "sim3" else fp.profile_scene(name)


def calls_of(ctx, store, form, sc):
    """(the resident call, the stateless call) on the scene's keyframes, added to the (cleared) store under the keys 0 .. K - 1"""
    store.clear()
    store.add_scene(range(sc.K), sc)
    keys = np.arange(sc.K, dtype=np.int64)
    if form == "sim3":
        return (lambda: ks.fuse_sim3_eval_resident(ctx, store, keys, sc)), (lambda: fs.fuse_sim3_eval(ctx, sc))
    return (lambda: ks.fuse_pose_eval_resident(ctx, store, keys, sc)), (lambda: fp.fuse_pose_eval(ctx, sc))


def one_run(scenes):
    ctx = Context(0)
    store = ks.KeyFrameStore(ctx, MAX_KF, MAX_FEAT)
    rows = []
    for form, name in ROWS:
        sc = scenes[form, name]
        res, stl = calls_of(ctx, store, form, sc)
        a, b = res(), stl()
        if not (np.array_equal(a["table"], b["table"]) and np.array_equal(a["n_hit"], b["n_hit"])):
            raise SystemExit(f"{form} {name}: the resident call and the stateless call disagree")
        r = _interleaved(dict(resident_us=res, stateless_us=stl))
        rows.append(dict(form=form, size=name, K=sc.K, P=sc.P, pairs=int(a["table"].size), baseline="stateless_us", **r))
    store.close()
    ctx.close()
    return rows


def phases_child():
    """the child of phases(): WARM + REPS resident calls per row, the library printing its phase clocks"""
    ctx = Context(0)
    store = ks.KeyFrameStore(ctx, MAX_KF, MAX_FEAT)
    for form, name in ROWS:
        res, _ = calls_of(ctx, store, form, scene_of(form, name))
        for _ in range(WARM + REPS):
            res()
    store.close()
    ctx.close()


def phases():
    env = dict(os.environ, CCM_DBG="fuse")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--phases-child"], env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit("the phase run failed:\n" + r.stderr[-2000:])
    pat = re.compile(r"\[fuse(?:_pose)?_resident\] .*?pack_us=([\d.]+) device_us=([\d.]+) unpack_us=([\d.]+) up_bytes=(\d+) down_bytes=(\d+)")
    got = [tuple(float(x) for x in m.groups()) for m in map(pat.search, r.stderr.splitlines()) if m]
    per = WARM + REPS
    if len(got) != per * len(ROWS):
        raise SystemExit(f"the phase run printed {len(got)} lines, expected {per * len(ROWS)}")
    out = []
    for i in range(len(ROWS)):
        p = np.array(got[i * per + WARM:(i + 1) * per])
        out.append(dict(pack_us=round(float(np.median(p[:, 0])), 1), device_phase_us=round(float(np.median(p[:, 1])), 1), unpack_us=round(float(np.median(p[:, 2])), 1),
                        up_bytes=int(p[0, 3]), down_bytes=int(p[0, 4])))
    return out


def add_costs():
    """medians (us) of ccm_kfstore_add for M = 1 and M = 500, through the C ABI and through the mirror"""
    sc = fs.profile_scene("merge_1_agent")
    l = lib()
    V = C.c_void_p
    l.ccm_kfstore_destroy.restype = None
    l.ccm_kfstore_add.argtypes = [V, V, C.c_int] + [V] * 8
    ctx = Context(0)
    raw = V()
    check(l.ccm_kfstore_create(ctx.handle, MAX_KF, MAX_FEAT, C.byref(raw)), ctx.handle)
    mirror = ks.KeyFrameStore(ctx, MAX_KF, MAX_FEAT)
    out = {}
    for M in (1, 500):
        sub = sc.subset(range(M))
        keys = np.arange(M, dtype=np.int64)

        def add_raw():
            check(l.ccm_kfstore_add(raw, ctx.handle, M, _p(keys), _p(sub.rec), _p(sub.feat_off), _p(sub.feat_xy), _p(sub.feat_octave), _p(sub.feat_desc), None, None), ctx.handle)
        ts = {"c_abi_us": [], "mirror_us": []}
        for rep in range(WARM + REPS):
            t = time.perf_counter(); add_raw(); a = time.perf_counter() - t
            check(l.ccm_kfstore_clear(raw, ctx.handle), ctx.handle)
            t = time.perf_counter(); mirror.add(keys, sub.rec, sub.feat_off, sub.feat_xy, sub.feat_octave, sub.feat_desc); b = time.perf_counter() - t
            mirror.clear()
            if rep >= WARM:
                ts["c_abi_us"].append(a); ts["mirror_us"].append(b)
        out[f"M={M}"] = {k: round(1e6 * float(np.median(v)), 1) for k, v in ts.items()}
        out[f"M={M}"].update({k.replace("_us", "_us_per_kf"): round(1e6 * float(np.median(v)) / M, 1) for k, v in ts.items()})
    l.ccm_kfstore_destroy(raw)
    mirror.close()
    ctx.close()
    return out


def main():
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    if "--phases-child" in sys.argv:
        return phases_child()
    scenes = {(form, name): scene_of(form, name) for form, name in ROWS}
    runs = [one_run(scenes) for _ in range(3)]
    ph = phases()
    table = []
    for i, row in enumerate(runs[0]):
        res = [r[i]["resident_us"] for r in runs]; stl = [r[i]["stateless_us"] for r in runs]
        margin = round(max(stl) - min(stl), 1)
        gain = round(float(np.median(stl)) - float(np.median(res)), 1)
        verdict = "faster" if gain > margin else "slower" if -gain > margin else "within the margin"
        table.append(dict({k: v for k, v in row.items() if not k.endswith("_us")}, resident_us=res, stateless_us=stl, margin_us=margin, gain_us=gain, verdict=verdict,
                          resident_phases=ph[i]))
    add = add_costs()
    m1 = next(r for r in table if r["size"] == "merge_1_agent")
    per_kf_gain = m1["gain_us"] / m1["K"]
    add["calls_to_pay"] = {k: (round(add["M=500"][k + "_us_per_kf"] / per_kf_gain, 2) if per_kf_gain > 0 else None) for k in ("c_abi", "mirror")}
    line = json.dumps(dict(reps=REPS, runs=3, rows=table, add=add))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
