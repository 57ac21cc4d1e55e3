"""CPU side of the triangulation of new map points (LocalMapping::CreateNewMapPoints, cslam/src/Mapping.cpp:353-448): a numpy-f32 checker that restates
OpenCV 4.2's 4x4 JacobiSVD (`jacobi_svd4`) and the whole per-match arithmetic (`ref_pairs`) independently of csrc/triangulate_math.h, known answers for
it, numpy.linalg.svd in f64 as the yardstick of the restated SVD, the header compiled for the host against the checker (bit-identical), and
cslam::NewMapPointBatch through its host evaluator against the literal per-neighbour sequence.

`python -m tests.test_triangulate_cpu` prints the measured constant c of the SVD bound.

The checker is vectorised over matches: every f32 operation is one numpy float32 ufunc call (IEEE single, nothing fused), every f64 one on float64.
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f32, f64 = np.float32, np.float64
FLT_EPSILON = f32(2.0 ** -23)

# c of the bound |v - v_ref| <= c * 2^-24 * sigma1 / sigma3 (and the same, times |x_ref|, for the dehomogenised point), measured over
# the seeded sweep of measure_c() on the CPU (13 035 matrices of twelve scenes): the maxima were 7.573 for the singular vector and 24.358 for the
# point.  Asserted at 4 x the maximum: the margin covers other seeds and another summation order.
C_VECTOR = 7.573
C_POINT = 24.358
C_MARGIN = 4.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def cv_hypot64(a, b):
    """hypot of lapack.cpp in double, element-wise: the scaled form"""
    a = np.abs(a); b = np.abs(b)
    with np.errstate(all="ignore"):
        r1 = b / a
        g1 = a * np.sqrt(1 + r1 * r1)
        r2 = a / b
        g2 = b * np.sqrt(1 + r2 * r2)
    return np.where(a > b, g1, np.where(b > 0, g2, 0.0))


def _sumsq64(rows):
    """double sum of squares of f32 rows (..., 4), left to right"""
    r = rows.astype(f64)
    s = np.zeros(r.shape[:-1], f64)
    for k in range(r.shape[-1]):
        s = s + r[..., k] * r[..., k]
    return s


def jacobi_svd4(A):
    """cv::SVD::compute on (N, 4, 4) f32 matrices as JacobiSVDImpl_<float> runs it (m = n = 4, eps = 2 FLT_EPSILON, at most 30 sweeps):
    returns (w (N, 4) f64 descending, vt (N, 4, 4) f32).  U is not produced."""
    A = np.asarray(A, f32)
    if A.ndim == 2:
        w, vt = jacobi_svd4(A[None])
        return w[0], vt[0]
    N = A.shape[0]
    At = np.ascontiguousarray(np.swapaxes(A, 1, 2)).copy()          # rows of At = columns of A
    Vt = np.tile(np.eye(4, dtype=f32), (N, 1, 1))
    W = _sumsq64(At)
    eps = f64(f32(2) * FLT_EPSILON)
    with np.errstate(all="ignore"):
        for _ in range(30):
            changed = np.zeros(N, bool)
            for i in range(3):
                for j in range(i + 1, 4):
                    a, b = W[:, i], W[:, j]
                    p = np.zeros(N, f64)
                    for k in range(4):
                        p = p + At[:, i, k].astype(f64) * At[:, j, k].astype(f64)
                    rot = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not rot.any():
                        continue
                    p = p * 2
                    beta = a - b
                    gamma = cv_hypot64(p, beta)
                    neg = beta < 0
                    s_n = np.sqrt((gamma - beta) * 0.5 / gamma).astype(f32)
                    c_n = (p / (gamma * s_n.astype(f64) * 2)).astype(f32)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2)).astype(f32)
                    s_p = (p / (gamma * c_p.astype(f64) * 2)).astype(f32)
                    c = np.where(neg, c_n, c_p)[:, None]
                    s = np.where(neg, s_n, s_p)[:, None]
                    for M in (At, Vt):
                        x, y = M[:, i, :].copy(), M[:, j, :].copy()
                        t0 = (c * x) + (s * y)
                        t1 = ((-s) * x) + (c * y)
                        M[:, i, :] = np.where(rot[:, None], t0, x)
                        M[:, j, :] = np.where(rot[:, None], t1, y)
                    W[:, i] = np.where(rot, _sumsq64(At[:, i, :]), a)
                    W[:, j] = np.where(rot, _sumsq64(At[:, j, :]), b)
                    changed |= rot
            if not changed.any():
                break
            # a matrix whose sweep changed nothing stops; its later sweeps would change nothing either (every pair is skipped again), so going on is the same
        W = np.sqrt(_sumsq64(At))
    ar = np.arange(N)
    for i in range(3):                                              # selection sort, descending, strict <
        j = np.full(N, i)
        for k in range(i + 1, 4):
            j = np.where(W[ar, j] < W[:, k], k, j)
        wi, wj = W[:, i].copy(), W[ar, j].copy()
        W[:, i] = wj; W[ar, j] = wi
        vi, vj = Vt[:, i, :].copy(), Vt[ar, j, :].copy()
        Vt[:, i, :] = vj; Vt[ar, j, :] = vi
    return W, Vt


def _rowdot(R3, t, X):
    """Rcw.row(r).dot(x3Dt) + tcw(r): double dot, double add, the float"""
    d = np.zeros(X.shape[0], f64)
    for k in range(3):
        d = d + R3[:, k].astype(f64) * X[:, k].astype(f64)
    return (d + t.astype(f64)).astype(f32)


def _norm3(D):
    s = np.zeros(D.shape[0], f64)
    for k in range(3):
        s = s + D[:, k].astype(f64) * D[:, k].astype(f64)
    return np.sqrt(s)


def _cams(cam):
    cam = np.asarray(cam, f32).reshape(-1, 21)
    return dict(R=cam[:, :9].reshape(-1, 3, 3), t=cam[:, 9:12], O=cam[:, 12:15], fx=cam[:, 15], fy=cam[:, 16], cx=cam[:, 17], cy=cam[:, 18], ifx=cam[:, 19], ify=cam[:, 20])


def ref_pairs(cam1, cam2, pair_off, xy, oct_, sigma2_1, sf_1, sigma2_2, sf_2, ratio, details=False):
    """The reference's loop body for every match: (status (P,) u8, x3d (P, 3) f32).  details: also a dict of intermediate values."""
    pair_off = np.asarray(pair_off)
    P = int(pair_off[-1])
    xy = np.asarray(xy, f32).reshape(-1, 4); oct_ = np.asarray(oct_).reshape(-1, 2)
    grp = np.repeat(np.arange(pair_off.size - 1), np.diff(pair_off))
    c1 = _cams(np.tile(np.asarray(cam1, f32).reshape(1, 21), (P, 1)))
    c2 = _cams(np.asarray(cam2, f32).reshape(-1, 21)[grp])
    ratio = f32(ratio)
    with np.errstate(all="ignore"):
        xn, ray = [], []
        for c, x, y in ((c1, xy[:, 0], xy[:, 1]), (c2, xy[:, 2], xy[:, 3])):
            a = (x - c["cx"]) * c["ifx"]; b = (y - c["cy"]) * c["ify"]
            xn.append((a, b))
            R = c["R"]                                              # Rwc = Rcw.t(): Rwc[r][k] = Rcw[k][r]; small gemm, f32 accumulator left to right
            ray.append(np.stack([((R[:, 0, r] * a) + (R[:, 1, r] * b)) + (R[:, 2, r] * f32(1)) for r in range(3)], 1))
        r1, r2 = ray[0].astype(f64), ray[1].astype(f64)
        dot = np.zeros(P, f64); n1 = np.zeros(P, f64); n2 = np.zeros(P, f64)
        for k in range(3):
            dot = dot + r1[:, k] * r2[:, k]; n1 = n1 + r1[:, k] * r1[:, k]; n2 = n2 + r2[:, k] * r2[:, k]
        cos = (dot / (np.sqrt(n1) * np.sqrt(n2))).astype(f32)
        par_ok = (cos < (cos + f32(1))) & (cos > 0) & (cos.astype(f64) < 0.9998)
        A = np.zeros((P, 4, 4), f32)
        for row, (c, s, k) in enumerate(((c1, xn[0][0], 0), (c1, xn[0][1], 1), (c2, xn[1][0], 0), (c2, xn[1][1], 1))):
            T2 = np.concatenate([c["R"][:, 2, :], c["t"][:, 2:3]], 1)
            Tk = np.concatenate([c["R"][:, k, :], c["t"][:, k:k + 1]], 1)
            A[:, row, :] = (s[:, None] * T2) - Tk
        _, Vt = jacobi_svd4(A)
        v = Vt[:, 3, :]
        w_zero = v[:, 3] == 0
        inv = (1.0 / v[:, 3].astype(f64)).astype(f32)
        X = (v[:, :3] * inv[:, None]) + f32(0)
        z1 = _rowdot(c1["R"][:, 2, :], c1["t"][:, 2], X)
        z2 = _rowdot(c2["R"][:, 2, :], c2["t"][:, 2], X)
        e2, fail = [], []
        for c, z, kx, ky, sig in ((c1, z1, xy[:, 0], xy[:, 1], np.asarray(sigma2_1, f32)[oct_[:, 0]]), (c2, z2, xy[:, 2], xy[:, 3], np.asarray(sigma2_2, f32)[oct_[:, 1]])):
            x = _rowdot(c["R"][:, 0, :], c["t"][:, 0], X)
            y = _rowdot(c["R"][:, 1, :], c["t"][:, 1], X)
            invz = (1.0 / z.astype(f64)).astype(f32)
            u = ((c["fx"] * x) * invz) + c["cx"]
            vv = ((c["fy"] * y) * invz) + c["cy"]
            ex = u - kx; ey = vv - ky
            e = (ex * ex) + (ey * ey)
            e2.append(e)
            fail.append(e.astype(f64) > 5.991 * sig.astype(f64))
        d1 = _norm3(X - c1["O"]).astype(f32); d2 = _norm3(X - c2["O"]).astype(f32)
        rd = d2 / d1
        ro = np.asarray(sf_1, f32)[oct_[:, 0]] / np.asarray(sf_2, f32)[oct_[:, 1]]
        scale_fail = ((rd * ratio) < ro) | (rd > (ro * ratio))
    conds = [~par_ok, w_zero, z1 <= 0, z2 <= 0, fail[0], fail[1], (d1 == 0) | (d2 == 0), scale_fail]
    status = np.select(conds, list(range(1, 9)), 0).astype(np.uint8)
    x3d = X.copy()
    x3d[status == 2] = v[status == 2, :3]
    x3d[status == 1] = np.nan
    if details:
        return status, x3d, dict(cos=cos, A=A, v=v, z1=z1, z2=z2, e2_1=e2[0], e2_2=e2[1], d1=d1, d2=d2)
    return status, x3d


def same_bits(a, b):
    """bit-identical floats; NaNs must sit in the same places (their payloads are not compared)"""
    a = np.asarray(a, f32); b = np.asarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_diagonal_and_permuted_diagonal_matrices():
    w, vt = jacobi_svd4(np.diag([1.0, 3.0, 2.0, 4.0]).astype(f32))
    assert list(w) == [4, 3, 2, 1]
    assert list(np.argmax(np.abs(vt), 1)) == [3, 1, 2, 0] and np.array_equal(np.abs(vt).sum(1), np.ones(4))
    # a tie keeps the first index first: columns 1 and 3 both have norm 3
    w, vt = jacobi_svd4(np.diag([1.0, 3.0, 2.0, 3.0]).astype(f32))
    assert list(w) == [3, 3, 2, 1] and list(np.argmax(np.abs(vt), 1)) == [1, 3, 2, 0]
    # permuted diagonal: column j holds d[j] in row perm[j]; the singular vectors are still unit vectors of the column index
    P = np.zeros((4, 4), f32)
    for j, (r, d) in enumerate(zip([2, 0, 3, 1], [5.0, 0.5, 7.0, 5.0])):
        P[r, j] = d
    w, vt = jacobi_svd4(P)
    assert list(w) == [7, 5, 5, 0.5] and list(np.argmax(np.abs(vt), 1)) == [2, 0, 3, 1]
    # batched = one by one
    rng = np.random.default_rng(0)
    B = rng.normal(size=(7, 4, 4)).astype(f32)
    wb, vb = jacobi_svd4(B)
    for i in range(7):
        w1, v1 = jacobi_svd4(B[i])
        assert np.array_equal(w1, wb[i]) and np.array_equal(v1, vb[i])


def test_rank_three_matrix_with_a_known_null_vector():
    # rows orthogonal to n = (1, 2, -2, 4) / 5
    n = np.array([1.0, 2.0, -2.0, 4.0]) / 5
    B = np.array([[2, -1, 0, 0], [2, 0, 1, 0], [4, 0, 0, -1], [0, 2, 2, 0]], f64)
    assert np.abs(B @ n).max() == 0
    w, vt = jacobi_svd4(B.astype(f32))
    assert w[3] < 1e-6 * w[0] and np.all(np.diff(w) <= 0)
    v = vt[3].astype(f64)
    assert min(np.abs(v - n).max(), np.abs(v + n).max()) < 5e-7
    assert np.abs(vt.astype(f64) @ vt.astype(f64).T - np.eye(4)).max() < 1e-6


def test_noise_free_two_view_scene_recovers_the_planted_points():
    from ccm_slam_amd import triangulate as T
    sc = T.make_pair_scene(seed=3, S=3, n_pairs=150, noise_px=0.0, mismatch=0.0, behind=0.0, tiny_baseline=0.0, wild_octave=0.0)
    status, x3d = ref_pairs(*T.flat(sc))
    ok = status == 0
    assert ok.mean() > 0.9, np.bincount(status, minlength=9)
    err = np.linalg.norm(x3d[ok].astype(f64) - sc["X"][ok], axis=1) / np.linalg.norm(sc["X"][ok], axis=1)
    assert err.max() < 2e-3, err.max()            # f32 keypoints (2^-24 * 752 px) over a baseline of 0.15 .. 0.6 at depth <= 9
    assert np.median(err) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the restated SVD against numpy.linalg.svd in f64
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _sweep_matrices(seeds=range(100, 112)):
    from ccm_slam_amd import triangulate as T
    As = []
    for seed in seeds:
        sc = T.make_pair_scene(seed=seed, S=5, n_pairs=250)
        st, _, d = ref_pairs(*T.flat(sc), details=True)
        As.append(d["A"][st != 1])
    return np.concatenate(As)


def measure_c(A=None):
    """max over the sweep of err / (2^-24 * sigma1 / sigma3 [* |x_ref|]) for the last right singular vector (up to sign) and the dehomogenised point"""
    A = _sweep_matrices() if A is None else A
    _, Vt = jacobi_svd4(A)
    U, S, Vh = np.linalg.svd(A.astype(f64))
    vr = Vh[:, 3, :]
    v = Vt[:, 3, :].astype(f64)
    sign = np.where(np.sum(v * vr, 1) < 0, -1.0, 1.0)[:, None]
    unit = 2.0 ** -24 * S[:, 0] / S[:, 2]
    cv = np.linalg.norm(v - sign * vr, axis=1) / unit
    x = v[:, :3] / v[:, 3:4]; xr = vr[:, :3] / vr[:, 3:4]
    cx = np.linalg.norm(x - xr, axis=1) / (unit * np.linalg.norm(xr, axis=1))
    return A.shape[0], float(cv.max()), float(cx.max())


def test_restated_svd_against_numpy_f64():
    n, cv, cx = measure_c()
    print(f"SVD sweep: {n} matrices, c(vector) = {cv:.3f}, c(point) = {cx:.3f}")
    assert n >= 10000
    assert cv <= C_MARGIN * C_VECTOR and cx <= C_MARGIN * C_POINT, (cv, cx)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the header compiled for the host against the checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def build_host_check(tmp_path):
    exe = tmp_path / "triangulate_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe),
                    os.path.join(HERE, "host", "triangulate_check.cpp"), "-lm"], check=True)
    return exe


def run_host_check(exe, tmp_path, cam1, cam2, pair_off, xy, oct_, s1, f1, s2, f2, ratio):
    c = lambda a, dt: np.ascontiguousarray(a, dt).tobytes()
    P = int(pair_off[-1])
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(pair_off) - 1, P, len(s1)], np.int32).tobytes() + np.array([ratio], f32).tobytes())
        f.write(c(cam1, f32) + c(cam2, f32) + c(pair_off, np.int32) + c(xy, f32) + c(oct_, np.int32) + c(s1, f32) + c(f1, f32) + c(s2, f32) + c(f2, f32))
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    raw = (tmp_path / "out.bin").read_bytes()
    return np.frombuffer(raw, np.uint8, P), np.frombuffer(raw, f32, 3 * P, P).reshape(P, 3)


def planted_scenes():
    """Every planted case as (name, flat arguments): the parallax threshold, z = 0, w = 0, a zero distance, the reprojection thresholds of both keyframes."""
    from ccm_slam_amd import triangulate as T
    s2, sf = T.level_tables()
    ratio = T.ratio_factor()
    one = lambda cam1, cam2, xy, oct_, t1=None, t2=None: (cam1, cam2.reshape(1, 21), np.array([0, len(xy)], np.int32), xy, np.asarray(oct_, np.int32),
                                                          s2 if t1 is None else t1, sf if t1 is None else np.ones(8, f32), s2 if t2 is None else t2,
                                                          sf if t1 is None else np.ones(8, f32), ratio)
    out = []
    cam1, cam2, xy, cos = T.plant_parallax_threshold()
    out.append(("parallax", one(cam1, cam2, xy, np.zeros((3, 2)))))
    cam1, cam2, xy = T.plant_depth_zero()
    out.append(("z = 0", one(cam1, cam2, xy, [[0, 0]])))
    cam1, cam2, xy = T.plant_w_zero()
    out.append(("w = 0", one(cam1, cam2, xy, [[0, 0]])))
    # a zero distance: the record's Ow set to the triangulated point of an accepted match
    sc = T.make_pair_scene(seed=8, S=1, n_pairs=40, mismatch=0, behind=0, tiny_baseline=0, wild_octave=0)
    st, x3d = ref_pairs(*T.flat(sc))
    i = int(np.nonzero(st == 0)[0][0])
    for which in (1, 2):
        cam1, cam2 = sc["cam1"].copy(), sc["cam2"][0].copy()
        (cam1 if which == 1 else cam2)[12:15] = x3d[i]
        out.append((f"dist{which} = 0", one(cam1, cam2, sc["xy"][i:i + 1], sc["oct"][i:i + 1])))
    # reprojection: the sigma2 table brackets the match's own squared error, octaves 0 / 1 / 2 = one ulp below, nearest, one ulp above
    _, _, d = ref_pairs(*T.flat(sc), details=True)
    big = np.full(8, 1e6, f32)
    xy3 = np.repeat(sc["xy"][i:i + 1], 3, 0)
    out.append(("reprojection 1", one(sc["cam1"], sc["cam2"][0], xy3, [[0, 0], [1, 0], [2, 0]], T.sigma2_bracket(d["e2_1"][i]), big)))
    out.append(("reprojection 2", one(sc["cam1"], sc["cam2"][0], xy3, [[0, 0], [0, 1], [0, 2]], big, T.sigma2_bracket(d["e2_2"][i]))))
    return out


def test_planted_cases_on_the_checker():
    from ccm_slam_amd import triangulate as T
    got = {name: ref_pairs(*args, details=True) for name, args in planted_scenes()}
    st, _, d = got["parallax"]
    assert list(d["cos"]) == [np.nextafter(f32(0.9998), f32(0)), f32(0.9998), np.nextafter(f32(0.9998), f32(2))]
    # 0.9998f = 0.99980002641677856 > 0.9998: the float on the threshold is already rejected, the float below passes the gate
    assert st[0] != 1 and st[1] == 1 and st[2] == 1
    st, x, d = got["z = 0"]
    assert list(st) == [3] and d["z1"][0] == 0 and np.array_equal(x[0], np.zeros(3, f32))
    st, x, d = got["w = 0"]
    assert list(st) == [2] and d["v"][0, 3] == 0 and d["cos"][0] < 0.99 and np.array_equal(np.abs(x[0]), [0, 0, 1])
    assert list(got["dist1 = 0"][0]) == [7] and got["dist1 = 0"][2]["d1"][0] == 0
    assert list(got["dist2 = 0"][0]) == [7] and got["dist2 = 0"][2]["d2"][0] == 0
    st = got["reprojection 1"][0]
    assert st[0] == 5 and st[2] == 0 and st[1] in (0, 5), st
    st = got["reprojection 2"][0]
    assert st[0] == 6 and st[2] == 0 and st[1] in (0, 6), st


def test_header_on_the_host_matches_the_checker(tmp_path):
    """triangulate_math.h compiled with g++ against ref_pairs on more than 20 000 matches: equal status, bit-identical x3D."""
    from ccm_slam_amd import triangulate as T
    exe = build_host_check(tmp_path)
    total = 0
    hist = np.zeros(9, np.int64)
    cases = [(f"scene {seed}", T.flat(T.make_pair_scene(seed=seed, S=20, n_pairs=[(37 * (seed + s)) % 130 + 40 for s in range(20)], empty=(3, 11)))) for seed in range(10)]
    sc = T.make_pair_scene(seed=77, S=2, n_pairs=30)
    sc["cam2"][1, 9] = np.nan                                        # a NaN translation passes the parallax gate and runs through the SVD
    sc["xy"][3, 0] = np.nan                                          # a NaN keypoint stops at it
    cases.append(("nan", T.flat(sc)))
    for name, args in cases + planted_scenes():
        st, x3d = run_host_check(exe, tmp_path, *args)
        rst, rx = ref_pairs(*args)
        assert np.array_equal(st, rst), (name, np.nonzero(st != rst)[0][:10], st[st != rst][:10], rst[st != rst][:10])
        assert same_bits(x3d, rx), name
        total += st.size
        hist += np.bincount(st, minlength=9)
    assert total >= 20000, total
    assert (hist > 0).all(), hist                                    # every gate of the reference is reached


# ---------------------------------------------------------------------------------------------------------------------------------------------
# NewMapPointBatch through its host evaluator against the literal per-neighbour sequence
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sequential_reference(sc, has1=None):
    """The reference's loop over the neighbours: resolve with the flags as they are, triangulate every match, an accepted match gives idx1 a map point."""
    from ccm_slam_amd import triangulate as T
    has1 = np.zeros(sc["keys1"][0].size, np.uint8) if has1 is None else has1.copy()
    out = []
    for j in range(len(sc["keys2"])):
        pairs = T.resolve_candidates(sc["cands"][j], has1)
        xy, oct_ = T.pairs_to_flat(sc, j, pairs)
        st, x3d = ref_pairs(sc["cam1"], sc["cam2"][j:j + 1], [0, len(pairs)], xy, oct_, sc["sigma2"], sc["sf"], sc["sigma2"], sc["sf"], sc["ratio"])
        out.append((pairs, st, x3d))
        has1[pairs[st == 0, 0]] = 1
    return out


def run_batch(sc, device):
    """The same loop through NewMapPoints: the prediction with the flags of the build, then points(j, pairs as they are now)."""
    from ccm_slam_amd import triangulate as T
    has1 = np.zeros(sc["keys1"][0].size, np.uint8)
    pred = [T.resolve_candidates(c, has1) for c in sc["cands"]]
    b = T.NewMapPoints(device, sc["cam1"], sc["keys1"], sc["cam2"], sc["keys2"], pred, sc["sigma2"], sc["sf"], sc["sigma2"], sc["sf"], sc["ratio"])
    out = []
    for j in range(len(sc["keys2"])):
        pairs = T.resolve_candidates(sc["cands"][j], has1)
        st, x3d, n_ok = b.points(j, pairs)
        assert n_ok == int((st == 0).sum())
        out.append((pairs, st, x3d))
        has1[pairs[st == 0, 0]] = 1
    stats = b.stats()
    b.close()
    return out, stats, sum(len(p) for p in pred)


def check_batch(sc, device):
    got, (predicted, hits, misses), n_pred = run_batch(sc, device)
    want = sequential_reference(sc)
    for j, ((p, st, x), (rp, rst, rx)) in enumerate(zip(got, want)):
        assert np.array_equal(p, rp) and np.array_equal(st, rst) and same_bits(x, rx), j
    assert predicted == n_pred and hits + misses == sum(len(p) for p, _, _ in got)
    return predicted, hits, misses, sum(int((st == 0).sum()) for _, st, _ in got)


def test_batch_equals_the_per_neighbour_sequence_on_the_host():
    from ccm_slam_amd import triangulate as T
    seen_miss = False
    for seed in (0, 1, 2):
        predicted, hits, misses, accepted = check_batch(T.make_keyframe_scene(seed=seed, S=8, n_feat=300), None)
        assert accepted > 100 and hits > 100
        seen_miss |= misses > 0
    assert seen_miss                                                 # accepted points changed a later neighbour's matches
    predicted, hits, misses, accepted = check_batch(T.make_keyframe_scene(seed=5, S=8, n_feat=300, disjoint=True), None)
    assert misses == 0 and hits == predicted and accepted > 100


if __name__ == "__main__":
    n, cv, cx = measure_c()
    print(f"restated JacobiSVD against numpy.linalg.svd (f64) over {n} matrices: c(vector) = {cv:.3f}, c(point) = {cx:.3f}")
