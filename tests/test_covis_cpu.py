"""CPU: the covisibility update (csrc/covis_math.h through the host evaluator and cslam::CovisibilityBatch) against

  * a literal sequential replay of KeyFrame::UpdateConnections, AddConnection and UpdateBestCovisibles (KeyFrame.cpp:629-711, :392-426) written here with dicts
    keyed by keyframe, independent of the header: it mutates every keyframe's map and ordered vectors along the walk, starting from empty ones;
  * known answers.
Every comparison is exact integer equality.
"""
import numpy as np
import pytest

EMPTY, FALLBACK, CHANGED = 1, 2, 4
KEYS = ("flags", "row_off", "col", "count", "fw_off", "fw_col", "fw_w", "ord_off", "ord_kf", "ord_w")


@pytest.fixture(scope="module")
def V():
    from ccm_slam_amd import covis
    return covis


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Replay:
    """weights[k]: mConnectedKeyFrameWeights, ord_kf[k] / ord_w[k]: mvpOrderedConnectedKeyFrames / mvOrderedWeights of every keyframe, the outside ones included"""

    def __init__(self, sc, th=15):
        self.sc, self.th = sc, th
        self.n_kf, self.n_all = int(sc["n_kf"]), int(sc["n_all"])
        self.key = [int(k) for k in sc["order_key"]]
        self.weights = [dict() for _ in range(self.n_all)]
        self.ord_kf = [[] for _ in range(self.n_all)]
        self.ord_w = [[] for _ in range(self.n_all)]
        self.counter = [dict() for _ in range(self.n_kf)]
        self.flags = [0] * self.n_kf
        self.rebuilt = [False] * self.n_all
        self.outside = []
        for i in range(self.n_kf):
            self.update_connections(i)

    def update_best_covisibles(self, k):
        pairs = sorted((w, self.key[j], j) for j, w in self.weights[k].items())       # sort(vPairs): by weight, then by pointer
        lk, lw = [], []
        for w, _, j in pairs:
            lk.insert(0, j); lw.insert(0, w)                                             # push_front
        self.ord_kf[k], self.ord_w[k] = lk, lw
        self.rebuilt[k] = True

    def add_connection(self, k, src, w):
        if k >= self.n_kf:
            self.outside.append((k, src, w))
        if src not in self.weights[k]:
            self.weights[k][src] = w
        elif self.weights[k][src] != w:
            self.weights[k][src] = w
        else:
            return
        self.update_best_covisibles(k)

    def update_connections(self, i):
        sc = self.sc
        counter = {}
        for e in range(int(sc["list_off"][i]), int(sc["list_off"][i + 1])):
            p = int(sc["list_pt"][e])
            if p < 0:
                continue
            if sc["list_skip"][e]:
                continue
            for o in range(int(sc["obs_off"][p]), int(sc["obs_off"][p + 1])):
                j = int(sc["obs_kf"][o])
                if j == i:
                    continue
                counter[j] = counter.get(j, 0) + 1
        self.counter[i] = dict(counter)
        if not counter:
            self.flags[i] |= EMPTY
            return
        nmax, kmax, pairs = 0, None, []
        for j in sorted(counter, key=lambda j: self.key[j]):                             # the std::map is walked in pointer order
            if counter[j] > nmax:
                nmax, kmax = counter[j], j
            if counter[j] >= self.th:
                pairs.append((counter[j], self.key[j], j))
                self.add_connection(j, i, counter[j])
        if not pairs:
            self.flags[i] |= FALLBACK
            pairs.append((nmax, self.key[kmax], kmax))
            self.add_connection(kmax, i, nmax)
        pairs.sort()
        lk, lw = [], []
        for w, _, j in pairs:
            lk.insert(0, j); lw.insert(0, w)
        self.weights[i] = dict(counter)
        self.ord_kf[i], self.ord_w[i] = lk, lw
        self.rebuilt[i] = False

    def arrays(self):
        """the layout of covis.update / update_host"""
        def csr(rows):
            off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
            flat = [x for r in rows for x in r]
            return off, np.array([x[0] for x in flat], np.int32).reshape(-1), np.array([x[1] for x in flat], np.int32).reshape(-1)
        o = {}
        o["row_off"], o["col"], o["count"] = csr([sorted(c.items()) for c in self.counter])
        o["fw_off"], o["fw_col"], o["fw_w"] = csr([sorted(self.weights[i].items()) for i in range(self.n_kf)])
        o["ord_off"], o["ord_kf"], o["ord_w"] = csr([list(zip(self.ord_kf[i], self.ord_w[i])) for i in range(self.n_kf)])
        o["flags"] = np.array([f | (CHANGED if self.rebuilt[i] else 0) for i, f in enumerate(self.flags)], np.int32)
        o["outside"] = np.array(self.outside, np.int32).reshape(-1, 3)
        return o


_REPLAYS = {}


def replay_arrays(sc, th=15, tag=None):
    """the replay's arrays; computed once per `tag` (scenes are never modified)"""
    if tag is None:
        return Replay(sc, th).arrays()
    if (tag, th) not in _REPLAYS:
        _REPLAYS[(tag, th)] = Replay(sc, th).arrays()
    return _REPLAYS[(tag, th)]


def assert_same(got, exp, what=""):
    for k in KEYS:
        a, b = np.asarray(got[k]), np.asarray(exp[k])
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), (what, k, a[:20], b[:20])


def hand_scene(n_kf, n_all, points, order_key=None, lists=None, bad=()):
    """points: the observers of each point; keyframe i of the set lists the points that see it, in point order, unless `lists` gives its list"""
    obs_off = np.concatenate([[0], np.cumsum([len(p) for p in points])]).astype(np.int32)
    obs_kf = np.array([k for p in points for k in p], np.int32)
    if lists is None:
        lists = [[p for p, obs in enumerate(points) if i in obs] for i in range(n_kf)]
    list_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    list_pt = np.array([p for l in lists for p in l], np.int32)
    list_skip = np.array([1 if p in bad else 0 for p in list_pt], np.uint8)
    key = np.arange(n_all, dtype=np.int32) if order_key is None else np.asarray(order_key, np.int32)
    return dict(n_kf=n_kf, n_all=n_all, n_pt=len(points), order_key=key, list_off=list_off, list_pt=list_pt, list_skip=list_skip, obs_off=obs_off, obs_kf=obs_kf)


def mixed_scene(V):
    """every kind of entry: null, repeated, stale, bad; counts on both sides of 15"""
    return V.make_scene(seed=5, n_kf=20, n_out=6, n_pt=420, window=12, mean_obs=5.0, null_frac=0.05, dup_frac=0.03, bad_frac=0.04, stale_frac=0.06)


def sparse_scene(V):
    return V.make_scene(seed=8, n_kf=20, n_out=6, n_pt=60, window=12, mean_obs=3.0, null_frac=0.05, dup_frac=0.03, bad_frac=0.04, stale_frac=0.3)


def walks(n_kf, n=6, seed=3):
    rng = np.random.default_rng(seed)
    return [np.arange(n_kf), np.arange(n_kf)[::-1]] + [rng.permutation(n_kf) for _ in range(n - 2)]


def state_by_old_index(sc, o):
    """per keyframe of the ORIGINAL scene: (weights as {old index: w}, ordered old indices, ordered weights)"""
    old = np.asarray(sc["old_of_new"]) if "old_of_new" in sc else np.arange(sc["n_all"])
    out = {}
    for i in range(sc["n_kf"]):
        f = slice(o["fw_off"][i], o["fw_off"][i + 1]); r = slice(o["ord_off"][i], o["ord_off"][i + 1])
        out[int(old[i])] = (dict(zip(old[o["fw_col"][f]].tolist(), o["fw_w"][f].tolist())), old[o["ord_kf"][r]].tolist(), o["ord_w"][r].tolist())
    return out


def bad_arguments(sc):
    """(what, scene) for every CCM_E_ARG case that depends on the arrays"""
    def mod(**kw):
        d = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
        d.update(kw)
        return d
    loff = np.array(sc["list_off"], copy=True); loff[1], loff[2] = loff[2] + 1, loff[1]
    yield "list_off decreases", mod(list_off=loff)
    ooff = np.array(sc["obs_off"], copy=True); ooff[3] = ooff[4] + 1
    yield "obs_off decreases", mod(obs_off=ooff)
    okf = np.array(sc["obs_kf"], copy=True); okf[5] = sc["n_all"]
    yield "observer >= n_all", mod(obs_kf=okf)
    okf = np.array(sc["obs_kf"], copy=True); okf[5] = -1
    yield "observer < 0", mod(obs_kf=okf)
    lpt = np.array(sc["list_pt"], copy=True); lpt[0] = sc["n_pt"]
    yield "point >= n_pt", mod(list_pt=lpt)
    key = np.array(sc["order_key"], copy=True); key[-1] = key[0]
    yield "duplicate order_key", mod(order_key=key)
    yield "n_kf < 1", mod(n_kf=0)
    yield "n_all < n_kf", mod(n_all=sc["n_kf"] - 1)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# host evaluator against the replay
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_host_equals_replay_for_six_walk_orders(V):
    sc = mixed_scene(V)
    lp = np.asarray(sc["list_pt"])
    assert (lp < 0).any() and np.asarray(sc["list_skip"]).any()
    per_kf = [lp[sc["list_off"][i]:sc["list_off"][i + 1]] for i in range(sc["n_kf"])]
    assert any(len(set(l[l >= 0].tolist())) < (l >= 0).sum() for l in per_kf)          # a repeated entry
    seen = dict(changed=0, fallback=0, extra=0, below=0)
    for w, walk in enumerate(walks(sc["n_kf"])):
        s = V.reorder(sc, walk)
        exp = replay_arrays(s, tag=("mixed", w))
        got = V.update_host(s)
        assert_same(got, exp, f"walk {w}")
        seen["changed"] += int((got["flags"] & CHANGED != 0).sum()); seen["fallback"] += int((got["flags"] & FALLBACK != 0).sum())
        seen["below"] += int((got["ord_w"] < 15).sum())
        # a sparse map, a third of its entries stale: pairs whose only shared point is listed on one side, so the other side's fallback adds an entry the row lacks
        t = V.reorder(sparse_scene(V), walk)
        got = V.update_host(t)
        assert_same(got, replay_arrays(t, tag=("sparse", w)), f"sparse, walk {w}")
        seen["extra"] += int(got["fw_col"].size - got["col"].size); seen["fallback"] += int((got["flags"] & FALLBACK != 0).sum())
        assert_same(V.update_host(t, th=1), replay_arrays(t, th=1, tag=("sparse", w)), f"sparse, walk {w}, th = 1")
    assert seen["changed"] > 0 and seen["extra"] > 0 and seen["below"] > 0 and seen["fallback"] > 0, seen
    # every keyframe below the threshold: the fallback everywhere
    s = V.reorder(sc, walks(sc["n_kf"])[3])
    got = V.update_host(s, th=10**6)
    assert_same(got, replay_arrays(s, th=10**6), "th above every count")
    assert ((got["flags"] & (FALLBACK | EMPTY)) != 0).all()


def test_replay_depends_on_the_walk_order_only_with_asymmetric_entries(V):
    sc = mixed_scene(V)
    states = [state_by_old_index(s, replay_arrays(s, tag=("mixed", w))) for w, s in ((w, V.reorder(sc, walk)) for w, walk in enumerate(walks(sc["n_kf"])))]
    assert any(states[0] != st for st in states[1:])
    clean = V.make_scene(seed=6, n_kf=20, n_out=6, n_pt=420, window=12, mean_obs=5.0, null_frac=0.05, dup_frac=0.0, bad_frac=0.0, stale_frac=0.0)
    ref = None
    for walk in walks(clean["n_kf"]):
        s = V.reorder(clean, walk)
        o = Replay(s).arrays()
        assert not (o["flags"] & CHANGED).any()
        st = state_by_old_index(s, o)
        ref = st if ref is None else ref
        assert st == ref
        assert_same(V.update_host(s), o, "clean")


def test_small_capacity_reports_what_is_needed(V):
    sc = mixed_scene(V)
    full = V.update_host(sc)
    rc, _, needed = V.call(V._host().ccmh_covis_update_host, (), sc, 15, 8)
    assert rc == 0 and needed.tolist() == [full["col"].size, full["fw_col"].size, full["ord_kf"].size]
    again = V.update_host(sc, cap=8)
    assert again["calls"] == 2
    assert_same(again, full)


def test_bad_arguments_host(V):
    sc = mixed_scene(V)
    for what, bad in bad_arguments(sc):
        rc, _, _ = V.call(V._host().ccmh_covis_update_host, (), bad, 15, 4096)
        assert rc == -1, what
    for th, cap in ((0, 4096), (15, -1)):
        assert V.call(V._host().ccmh_covis_update_host, (), sc, th, cap)[0] == -1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------------------------------
def rows(o, i, which):
    off, a, b = {"row": ("row_off", "col", "count"), "fw": ("fw_off", "fw_col", "fw_w"), "ord": ("ord_off", "ord_kf", "ord_w")}[which]
    s = slice(o[off][i], o[off][i + 1])
    return o[a][s].tolist(), o[b][s].tolist()


@pytest.mark.parametrize("shared", [14, 15])
def test_two_keyframes_at_the_threshold(V, shared):
    o = V.update_host(hand_scene(2, 2, [[0, 1]] * shared + [[0]] * 3))
    for i in (0, 1):
        assert rows(o, i, "row") == ([1 - i], [shared]) and rows(o, i, "fw") == ([1 - i], [shared]) and rows(o, i, "ord") == ([1 - i], [shared])
    assert o["flags"].tolist() == ([FALLBACK, FALLBACK] if shared == 14 else [0, 0])


def test_fallback_tie_goes_to_the_smallest_order_key(V):
    # keyframe 0 shares 3 points with each of the outside keyframes 1, 2, 3; keys 50, 7, 20
    sc = hand_scene(1, 4, [[0, 1]] * 3 + [[0, 2]] * 3 + [[0, 3]] * 3, order_key=[0, 50, 7, 20])
    o = V.update_host(sc)
    assert o["flags"].tolist() == [FALLBACK] and rows(o, 0, "ord") == ([2], [3]) and rows(o, 0, "fw") == ([1, 2, 3], [3, 3, 3])
    b = V.CovisibilityBatch(sc)
    assert b.results()["outside"].tolist() == [[2, 0, 3]]
    assert_same(o, replay_arrays(sc))


def test_equal_weights_are_ordered_by_order_key_descending(V):
    sc = hand_scene(1, 5, [[0, 1]] * 15 + [[0, 2]] * 15 + [[0, 3]] * 15 + [[0, 4]] * 16, order_key=[9, -4, 30, 2, -100])
    o = V.update_host(sc)
    assert rows(o, 0, "ord") == ([4, 2, 3, 1], [16, 15, 15, 15]) and o["flags"].tolist() == [0]
    assert_same(o, replay_arrays(sc))


def test_a_keyframe_whose_points_are_all_bad_is_empty(V):
    pts = [[0, 1]] * 20
    sc = hand_scene(2, 2, pts, bad=set(range(20)))
    o = V.update_host(sc)
    assert o["flags"].tolist() == [EMPTY, EMPTY] and o["col"].size == o["fw_col"].size == o["ord_kf"].size == 0
    # keyframe 1 lists nothing, keyframe 0 still sees it: 1 is EMPTY and receives 0's call on top of whatever it had
    sc = hand_scene(2, 2, pts, lists=[list(range(20)), []])
    o = V.update_host(sc)
    assert o["flags"].tolist() == [0, EMPTY | CHANGED] and rows(o, 1, "fw") == ([0], [20]) and rows(o, 1, "ord") == ([0], [20]) and rows(o, 1, "row") == ([], [])
    assert_same(o, replay_arrays(sc))


def test_a_repeated_entry_counts_twice(V):
    # keyframe 0 lists point 0 twice: C_0[1] = 16, C_1[0] = 15; walked first, 0 then takes 1's weight and rebuilds its list
    sc = hand_scene(2, 2, [[0, 1]] * 15, lists=[[0] + list(range(15)), list(range(15))])
    o = V.update_host(sc)
    assert rows(o, 0, "row") == ([1], [16]) and rows(o, 1, "row") == ([0], [15])
    assert rows(o, 0, "fw") == ([1], [15]) and rows(o, 0, "ord") == ([1], [15]) and rows(o, 1, "fw") == ([0], [15])
    assert o["flags"].tolist() == [CHANGED, 0]
    assert_same(o, replay_arrays(sc))


def test_outside_keyframes_receive_their_calls_in_reference_order(V):
    # set = {0, 1}, outside = {2, 3, 4}; keys put 4 before 2 before 3
    pts = [[0, 2]] * 15 + [[0, 3]] * 20 + [[0, 4]] * 16 + [[1, 3]] * 2 + [[1, 4]] * 2 + [[0, 1]] * 1
    sc = hand_scene(2, 5, pts, order_key=[100, 101, 5, 9, 1])
    b = V.CovisibilityBatch(sc)
    r = b.results()
    assert r["outside"].tolist() == [[4, 0, 16], [2, 0, 15], [3, 0, 20], [4, 1, 2]]
    exp = replay_arrays(sc)
    assert np.array_equal(r["outside"], exp["outside"])
    assert_same(r, exp)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_mirror_views(V):
    sc = V.reorder(mixed_scene(V), walks(20)[2])
    exp = replay_arrays(sc, tag=("mixed", 2))
    b = V.CovisibilityBatch(sc)
    r = b.results()
    assert_same(r, exp)
    assert np.array_equal(r["outside"], exp["outside"]) and r["outside"].shape[0] > 0
    for i in range(sc["n_kf"]):
        kf, w = rows(exp, i, "ord")
        assert b.best_covisibles(i, 10).tolist() == kf[:10] and b.best_covisibles(i, 1000).tolist() == kf
        for t in (1, 15, 30, 100):
            n = sum(x >= t for x in w)                     # upper_bound with weightComp; `it == end` returns nothing (KeyFrame.cpp:461)
            assert b.covisibles_by_weight(i, t).tolist() == ([] if n == len(w) else kf[:n]), (i, t)
    with pytest.raises(V.CcmError):
        V.CovisibilityBatch(dict(sc, order_key=np.zeros(sc["n_all"], np.int32)))
    b.close()
