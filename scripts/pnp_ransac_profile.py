"""GPU box: host-to-host time of the PnP RANSAC evaluation (ccm_pnp_ransac_eval) against the host evaluator (csrc/pnp_math.h on ONE thread,
ccmh_pnp_ransac_eval_host) for K candidates of N correspondences and 300 hypotheses each: the whole schedule of a relocalisation in which no candidate succeeds.

Medians of 200 repetitions; device and host calls alternate, so that both see the same machine state.  Shapes: 1 x 300 x 50, 5 x 300 x 100, 10 x 300 x 200.
Both evaluators must return the same counts and masks before anything is timed.  Prints one JSON line; --out FILE also writes it there
(profiles/pnp_ransac_profile.json is the copy DESIGN.md §27 and the README quote)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import pnp
from ccm_slam_amd._lib import Context, check, lib

REPS = 200
SHAPES = ((1, 50), (5, 100), (10, 200))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def make_candidate(seed, N):
    """N correspondences of a random pose, 60 % exact and 40 % displaced by tens of pixels (the generator of tests/pnp_cases.py, restated: scripts do not import tests)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.3, 0.3, 3); th = np.linalg.norm(a); k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.5]
    cam = (500.0, 510.0, 320.0, 240.0)
    X = (rng.uniform(-1.5, 1.5, (N, 3)) + [0, 0, 5]).astype(np.float32)
    Xc = X.astype(np.float64) @ R.T + t
    uv = np.stack([cam[2] + cam[0] * Xc[:, 0] / Xc[:, 2], cam[3] + cam[1] * Xc[:, 1] / Xc[:, 2]], 1)
    n_out = (2 * N) // 5
    ang = rng.uniform(0, 2 * np.pi, n_out); r = rng.uniform(30, 80, n_out)
    uv[N - n_out:] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    return pnp.PnPCandidate(P3Dw=X, P2D=uv.astype(np.float32), sigma2=np.ones(N, np.float32), cam=cam)


def run(ctx, K, N, rng):
    cands = [make_candidate(1000 * K + c, N) for c in range(K)]
    pt_off, P3, P2, s2, cam, _, _ = pnp.pack(cands)
    me = np.ascontiguousarray(pnp.max_errors(s2))
    H = 300 * K
    hc = np.repeat(np.arange(K, dtype=np.int32), 300)
    hi = np.stack([rng.choice(N, 4, replace=False) for _ in range(H)]).astype(np.int32)
    words = H * ((N + 31) // 32)
    out = [(np.zeros(H, np.int32), np.zeros(12 * H), np.zeros(H + 1, np.int32), np.zeros(words, np.uint32)) for _ in range(2)]
    tail = lambda o: (K, _p(pt_off), _p(P3), _p(P2), _p(me), _p(cam), H, _p(hc), _p(hi), _p(o[0]), _p(o[1]), _p(o[2]), _p(o[3]))
    dev = lambda: check(lib().ccm_pnp_ransac_eval(ctx.handle, *tail(out[0])), ctx.handle)
    fh = pnp._host().ccmh_pnp_ransac_eval_host

    def host():
        assert fh(*tail(out[1])) == 0

    for _ in range(3):
        dev(); host()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][3], out[1][3]), "device and host evaluator disagree"
    td, th_ = [], []
    for _ in range(REPS):
        t = time.perf_counter(); dev(); td.append(time.perf_counter() - t)
        t = time.perf_counter(); host(); th_.append(time.perf_counter() - t)
    d, h = float(np.median(td)), float(np.median(th_))
    return dict(K=K, N=N, hypotheses=H, device_us=round(1e6 * d, 1), host_1thread_us=round(1e6 * h, 1), host_over_device=round(h / d, 2),
                best_inliers=int(out[0][0].max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = Context(0)
    rng = np.random.default_rng(0)
    res = dict(what="ccm_pnp_ransac_eval against ccmh_pnp_ransac_eval_host (one thread), host to host, medians of %d interleaved repetitions" % REPS,
               runs=[run(ctx, K, N, rng) for K, N in SHAPES])
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
