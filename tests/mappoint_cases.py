"""The planted cases of ccm_mappoint_refresh_resident, shared by tests/test_mappoint_refresh_cpu.py and tests/test_mappoint_refresh_gpu.py, and an
independent replay of MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) in numpy: a literal sort
for the median, np.argmin for the first minimum, np.float32 scalars and Python doubles as oracle.update_normal_and_depth restates the reference.  It shares nothing
with csrc/mappoint_math.h.

One store of 8 keyframes (keys 100 .. 107) of at most 300 features holds every case; a case is a list of points, a point a list of (keyframe, feature)
observations, so every case can run alone and all of them in one call on the same keys and centres."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from ccm_slam_amd import fuse_sim3 as fs

K = 8
KEYS = np.arange(100, 100 + K, dtype=np.int64)
MAX_FEAT = 300
NLEVELS = 8
SF = (np.float32(1.2) ** np.arange(NLEVELS)).astype(np.float32)
K4 = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
REC = fs.kf_record(K4, fs.BOUNDS)
# every boundary of the kernel's size classes (8, 16, 32 lanes per point; above that a workgroup, whose lanes hold one more column from 65, 129 and 193 on) minus
# one, at it and plus one, and the cap
SIZES = (1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256)


@dataclass
class Point:
    obs: List[Tuple[int, int]]                  # (keyframe, feature) in list order
    pos: np.ndarray
    ref: Optional[Tuple[int, int]]              # (keyframe, feature) or None: ref_kf = -1
    seed: np.ndarray = field(default_factory=lambda: np.zeros(5, np.float32))   # normal (3), min_dist, max_dist before the call


@dataclass
class Case:
    name: str
    points: List[Point]


class Cases:
    def __init__(self):
        self.desc = [[] for _ in range(K)]
        self.oct = [[] for _ in range(K)]
        self.cases: List[Case] = []
        self.rng = np.random.default_rng(25)
        r = np.random.default_rng(7)
        self.centres = np.stack([r.uniform(-2, 2, K), r.uniform(-1, 1, K), r.uniform(-0.5, 0.5, K)], 1).astype(np.float32)
        self._n_seed = 0

    # ---- building ----
    def feat(self, kf: int, desc, octave: int = 0) -> Tuple[int, int]:
        assert len(self.desc[kf]) < MAX_FEAT
        self.desc[kf].append(np.asarray(desc, np.uint8).reshape(32)); self.oct[kf].append(octave)
        return kf, len(self.desc[kf]) - 1

    def emptiest(self) -> int:
        return int(np.argmin([len(d) for d in self.desc]))

    def rand_desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, d, bits):
        """d with the listed bit positions flipped"""
        b = np.unpackbits(np.asarray(d, np.uint8))
        b[np.asarray(bits, int)] ^= 1
        return np.packbits(b)

    def seed(self):
        self._n_seed += 1
        s = np.float32(self._n_seed)
        return np.array([s + 0.25, -s, s * 0.5, s + 100, s + 200], np.float32)

    def pos(self):
        return np.array([self.rng.uniform(-3, 3), self.rng.uniform(-2, 2), self.rng.uniform(2, 8)], np.float32)

    def point(self, descs, kfs=None, octs=None, ref="first", pos=None) -> Point:
        """a point whose observation i is a new feature with descs[i] in keyframe kfs[i] (default: the emptiest keyframe at that moment)"""
        obs = [self.feat(self.emptiest() if kfs is None else kfs[i], d, 0 if octs is None else octs[i]) for i, d in enumerate(descs)]
        return Point(obs, self.pos() if pos is None else np.asarray(pos, np.float32), obs[0] if ref == "first" and obs else (None if ref == "first" else ref), self.seed())

    def add(self, name, *points):
        self.cases.append(Case(name, list(points)))

    def finish(self):
        self.kfs = []
        for k in range(K):
            n = len(self.desc[k])
            r = np.random.default_rng(k)
            self.kfs.append(dict(desc=np.stack(self.desc[k]), oct=np.array(self.oct[k], np.uint8), xy=np.stack([r.uniform(20, 700, n), r.uniform(20, 450, n)], 1).astype(np.float32)))
        return self

    def by_name(self, name) -> Case:
        return next(c for c in self.cases if c.name == name)

    def all_points(self) -> List[Point]:
        return [p for c in self.cases for p in c.points]


def install(store, cs: Cases, keys=KEYS):
    for key, kf in zip(keys, cs.kfs):
        store.add([int(key)], REC, [0, kf["oct"].size], kf["xy"], kf["oct"], kf["desc"])


def planted() -> Cases:
    cs = Cases()
    rng = cs.rng
    # the sizes: noisy copies of one descriptor (8 % of the bits), so that the medians differ and sometimes tie; the first observer is the reference
    for n in SIZES:
        base = cs.rand_desc()
        bits = np.unpackbits(base)
        descs = [np.packbits(bits ^ (rng.random(256) < 0.08)) for _ in range(n)]
        cs.add(f"N={n}", cs.point(descs))
    a, b = cs.rand_desc(), cs.rand_desc()
    cs.add("N=2 of unrelated descriptors: the rank is 0, index 0 wins", cs.point([a, b]), cs.point([b, a]))
    cs.add("equal least medians, the earlier wins", cs.point([b, a, a]), cs.point([a, b, b, a]))
    c = cs.rand_desc()
    spokes = [cs.flipped(c, range(40 * i, 40 * i + 40)) for i in range(4)]          # 40 from the hub, 80 from each other
    cs.add("the least median at the last index", cs.point(spokes + [c]))
    cs.add("identical descriptors", cs.point([a] * 5))
    cs.add("complementary descriptors: a distance of 256", cs.point([a, ~a]), cs.point([a, ~a, ~a]), cs.point([~a, a, ~a, a, a]))
    # two points that share observations, and one keyframe twice (and one feature twice) in a list
    shared = cs.point([cs.rand_desc() for _ in range(6)])
    other = Point(shared.obs[2:] + [cs.feat(3, cs.rand_desc())], cs.pos(), shared.obs[3], cs.seed())
    cs.add("two points sharing observations", shared, other)
    twice = cs.point([cs.rand_desc() for _ in range(4)], kfs=[5, 5, 2, 5])
    twice.obs.append(twice.obs[1])
    cs.add("one keyframe twice in a list", twice)
    cs.add("an empty list", Point([], cs.pos(), (0, 0), cs.seed()), Point([], cs.pos(), None, cs.seed()))
    # normal / depth
    cs.add("an observer exactly at the point", cs.point([cs.rand_desc() for _ in range(3)], kfs=[1, 4, 6], pos=cs.centres[4]),
           cs.point([cs.rand_desc() for _ in range(2)], kfs=[2, 3], pos=cs.centres[2]))          # the second one's observer is its reference too: distance 0
    cs.add("ref_kf = -1", cs.point([cs.rand_desc() for _ in range(4)], ref=None), cs.point([cs.rand_desc() for _ in range(40)], ref=None))
    far = cs.feat(7, cs.rand_desc(), 3)
    cs.add("a reference keyframe that is no observer", cs.point([cs.rand_desc() for _ in range(3)], kfs=[0, 1, 2], ref=far))
    cs.add("the reference octave nlevels - 1", cs.point([cs.rand_desc() for _ in range(3)], octs=[NLEVELS - 1, 0, 0]),
           cs.point([cs.rand_desc() for _ in range(50)], octs=[NLEVELS - 1] + [0] * 49))
    cs.add("a reference octave beyond the tables", cs.point([cs.rand_desc() for _ in range(3)], octs=[NLEVELS, 0, 0]), cs.point([cs.rand_desc() for _ in range(3)], octs=[255, 1, 1]),
           cs.point([cs.rand_desc() for _ in range(35)], octs=[NLEVELS + 1] + [0] * 34))
    # a list whose f32 sum depends on its order (test_the_order_of_the_list_matters asserts it for the replay)
    cs.add("the sum runs in list order", cs.point([cs.rand_desc() for _ in range(7)], kfs=[0, 1, 2, 3, 4, 5, 6]), cs.point([cs.rand_desc() for _ in range(40)], kfs=[k % K for k in range(40)]))
    # the last feature of a keyframe: allocated last
    last = cs.point([cs.rand_desc() for _ in range(2)], kfs=[0, 0])
    cs.add("feature index n - 1", last)
    cs.finish()
    assert last.obs[1][1] == cs.kfs[0]["oct"].size - 1 and max(kf["oct"].size for kf in cs.kfs) <= MAX_FEAT
    return cs


def flatten(cs: Cases, points: List[Point]) -> dict:
    """the call's arrays for a list of points"""
    P = len(points)
    off = np.zeros(P + 1, np.int32); off[1:] = np.cumsum([len(p.obs) for p in points])
    obs = [o for p in points for o in p.obs]
    seed = np.stack([p.seed for p in points]) if P else np.zeros((0, 5), np.float32)
    return dict(keys=KEYS, kf_center=cs.centres, obs_off=off, obs_kf=np.array([o[0] for o in obs], np.int32), obs_feat=np.array([o[1] for o in obs], np.int32),
                pos=np.stack([p.pos for p in points]).astype(np.float32) if P else np.zeros((0, 3), np.float32),
                ref_kf=np.array([-1 if p.ref is None else p.ref[0] for p in points], np.int32), ref_feat=np.array([0 if p.ref is None else p.ref[1] for p in points], np.int32),
                scale_factors=SF, normal=seed[:, :3].copy(), min_dist=seed[:, 3].copy(), max_dist=seed[:, 4].copy())


ARG_NAMES = ("keys", "kf_center", "obs_off", "obs_kf", "obs_feat", "pos", "ref_kf", "ref_feat", "scale_factors")


def call(fn, first, f: dict, want_desc=True) -> dict:
    """fn = mappoint.refresh_resident (first = (ctx, store)) or mappoint.refresh_host (first = (store,)) on flatten's dictionary"""
    return fn(*first, *[f[k] for k in ARG_NAMES], normal=f["normal"], min_dist=f["min_dist"], max_dist=f["max_dist"], want_desc=want_desc)


# ---- the replay -------------------------------------------------------------------------------------------------------------------------------
def replay_best(desc: np.ndarray) -> int:
    """ComputeDistinctiveDescriptors on the rows of desc (N, 32): the distance matrix, a literal sort per row, the first least median"""
    N = desc.shape[0]
    if N == 0:
        return -1
    bits = np.unpackbits(desc, axis=1).astype(np.int32)
    D = (bits[:, None, :] != bits[None, :, :]).sum(2)
    med = np.array([np.sort(D[i])[int(0.5 * (N - 1))] for i in range(N)])
    return int(np.argmin(med))


def replay_normal_depth(pos, centres, ref_centre, level, sf):
    """UpdateNormalAndDepth for one point with a non-empty list of observer centres, in list order: (normal[3], min_dist, max_dist)"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        n = [f32(0), f32(0), f32(0)]
        for O in centres:
            d = [f32(pos[i]) - f32(O[i]) for i in range(3)]
            s = 0.0
            for x in d:
                s += float(x) * float(x)
            a = f32(np.float64(1.0) / np.sqrt(np.float64(s)))
            n = [f32(n[i] + f32(d[i] * a)) for i in range(3)]
        c = [f32(pos[i]) - f32(ref_centre[i]) for i in range(3)]
        s = 0.0
        for x in c:
            s += float(x) * float(x)
        dist = f32(np.sqrt(np.float64(s)))
        dmax = f32(dist * f32(sf[level]))
        dmin = f32(dmax / f32(sf[len(sf) - 1]))
        an = f32(1.0 / float(len(centres)))
        return np.array([f32(x * an) for x in n], np.float32), dmin, dmax


def replay(cs: Cases, points: List[Point]) -> dict:
    P = len(points)
    out = dict(best_obs=np.full(P, -1, np.int32), best_desc=np.zeros((P, 32), np.uint8), normal=np.zeros((P, 3), np.float32), min_dist=np.zeros(P, np.float32),
               max_dist=np.zeros(P, np.float32), status=np.zeros(P, np.uint8))
    for i, p in enumerate(points):
        out["normal"][i], out["min_dist"][i], out["max_dist"][i] = p.seed[:3], p.seed[3], p.seed[4]
        if not p.obs:
            continue
        desc = np.stack([cs.kfs[k]["desc"][f] for k, f in p.obs])
        b = replay_best(desc)
        out["best_obs"][i] = b; out["best_desc"][i] = desc[b]; out["status"][i] = 1
        if p.ref is None:
            continue
        level = int(cs.kfs[p.ref[0]]["oct"][p.ref[1]])
        if level >= NLEVELS:
            out["status"][i] |= 4
            continue
        out["normal"][i], out["min_dist"][i], out["max_dist"][i] = replay_normal_depth(p.pos, [cs.centres[k] for k, _ in p.obs], cs.centres[p.ref[0]], level, SF)
        out["status"][i] |= 2
    return out


def same_f32(a, b) -> bool:
    """bit patterns; a NaN matches a NaN"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1); b = np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same(got: dict, want: dict, tag, desc=True):
    """every point, every output, exactly"""
    assert np.array_equal(got["best_obs"], want["best_obs"]), (tag, "best_obs", np.flatnonzero(got["best_obs"] != want["best_obs"])[:8])
    assert np.array_equal(got["status"], want["status"]), (tag, "status")
    if desc:
        have = want["best_obs"] >= 0
        assert np.array_equal(got["best_desc"][have], want["best_desc"][have]), (tag, "best_desc")
    for k in ("normal", "min_dist", "max_dist"):
        assert same_f32(got[k], want[k]), (tag, k)


def todays_inputs(cs: Cases, f: dict) -> dict:
    """what today's route takes for the same points: the gathered descriptor rows and ref_level read on the host.  The reference of a point that has none, and a
    level beyond the tables, are replaced by entries the old call accepts; the caller compares only the points whose status has the normal / depth bit"""
    M = f["obs_kf"].size
    desc = np.stack([cs.kfs[k]["desc"][i] for k, i in zip(f["obs_kf"], f["obs_feat"])]) if M else np.zeros((0, 32), np.uint8)
    level = np.array([0 if k < 0 else int(cs.kfs[k]["oct"][i]) for k, i in zip(f["ref_kf"], f["ref_feat"])], np.int32)
    ok = (f["ref_kf"] >= 0) & (level < NLEVELS)
    return dict(desc=desc, ref_kf=np.where(ok, f["ref_kf"], 0).astype(np.int32), ref_level=np.where(ok, level, 0).astype(np.int32), ok=ok)
