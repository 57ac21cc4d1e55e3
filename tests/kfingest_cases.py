"""Cases shared by tests/test_kfingest_cpu.py and tests/test_kfingest_gpu.py (no test lives here): vocabularies, planted keyframes and the Python replay of
DBoW2's TemplatedVocabulary::transform with BowVector::addWeight / normalize and FeatureVector::addFeature that ccm_kfstore_ingest is held to.

The replay descends the tree with numpy (np.argmin: the first minimum in child order) and builds the two vectors with a dict filled in feature order and sorted();
it shares nothing with csrc/kfingest_math.h.  Every comparison is exact: integers as integers, doubles as bit patterns.

Vocabularies (name -> vocabulary dictionary, levelsup):
  k10L4     synth.make_vocabulary(10, 4), levelsup 2, with planted weights: 0.1 on the word six identical descriptors fall on (their sequential sum is not 6 * 0.1),
            one negative and one NaN weight;
  k7L5      (7, 5), levelsup 4;
  k10L3     (10, 3), levelsup 4: the recorded level is below the root's, every node is 0;
  permuted  k10L4's tree with the word ids permuted, so that word order is not leaf order;
  cut       (6, 3), levelsup 1, with two first-level nodes made leaves: a leaf above the recorded level, node 0 for its features.
"""
import functools

import numpy as np

from ccm_slam_amd import kfstore as ks, synth
from kfstore_cases import REC, rec_with

f32 = np.float32
MAXF = ks.KFI_MAX_FEAT
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 2000, MAXF)   # 1024 | 1025: the switch between the two sizes of the keyframe kernel


# ---- the replay -------------------------------------------------------------------------------------------------------------------------------------------
def replay_descent(v, desc, levelsup):
    """(leaf, node at level L - levelsup) per descriptor"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    N = desc.shape[0]
    co, ci, nd = np.asarray(v["child_off"], np.int64), np.asarray(v["child_id"], np.int64), np.asarray(v["node_desc"], np.uint8)
    node = np.zeros(N, np.int64); nid = np.zeros(N, np.int64)
    nid_level = int(v["L"]) - int(levelsup)
    lvl = 0
    while True:
        act = np.flatnonzero(co[node + 1] > co[node])
        if act.size == 0:
            break
        lvl += 1        # every feature starts at the root and takes one step per round
        order = act[np.argsort(node[act], kind="stable")]
        us, starts = np.unique(node[order], return_index=True)
        for u, a, b in zip(us.tolist(), starts.tolist(), starts.tolist()[1:] + [order.size]):
            f = order[a:b]
            ch = ci[co[u]:co[u + 1]]
            d = np.unpackbits(desc[f][:, None, :] ^ nd[ch][None, :, :], axis=2).sum(2)
            node[f] = ch[d.argmin(1)]      # the first minimum in child order
        if lvl == nid_level:
            nid[act] = node[act]
    return node.astype(np.int32), nid.astype(np.int32)


def replay_vectors(v, leaf, nid):
    """one keyframe's vectors from its features' leaves and nodes: addWeight in feature order, normalize in ascending word id, addFeature"""
    wid, wt = np.asarray(v["word_id"]), np.asarray(v["weight"], np.float64)
    acc, fv = {}, {}
    for i, (l, nd) in enumerate(zip(leaf.tolist(), nid.tolist())):
        w = float(wt[l])
        if w > 0:                      # TemplatedVocabulary.h:1157; false for a NaN
            k = int(wid[l])
            if k in acc:
                acc[k] += w
            else:
                acc[k] = w
            fv.setdefault(nd, []).append(i)
    ids = sorted(acc)
    vals = [acc[k] for k in ids]
    norm = 0.0
    for x in vals:
        norm += abs(x)
    if norm > 0.0:
        vals = [x / norm for x in vals]
    nodes = sorted(fv)
    off = np.zeros(len(nodes) + 1, np.int32)
    off[1:] = np.cumsum([len(fv[k]) for k in nodes])
    idx = [i for k in nodes for i in fv[k]]
    return dict(bow_word=np.array(ids, np.int32), bow_value=np.array(vals, np.float64), fv_node=np.array(nodes, np.int32), fv_off=off, fv_idx=np.array(idx, np.int32),
                feat_word=wid[leaf].astype(np.int32), feat_node=nid, norm=norm, raw=[acc[k] for k in ids])


# ---- vocabularies -----------------------------------------------------------------------------------------------------------------------------------------
def _noisy(v, rng, n, flip=0.05):
    """n descriptors: those of random nodes with a few bits flipped"""
    nd = np.asarray(v["node_desc"], np.uint8)
    bits = np.unpackbits(nd[rng.integers(1, nd.shape[0], n)], axis=1)
    return np.packbits(bits ^ (rng.random(bits.shape) < flip), axis=1) if n else np.zeros((0, 32), np.uint8)


@functools.lru_cache(maxsize=None)
def vocabularies():
    out = {}
    v = synth.make_vocabulary(10, 4, seed=1)
    v["weight"] = v["weight"].copy()
    # planted weights: the words three descriptors fall on
    rng = np.random.default_rng(100)
    plant = _noisy(v, rng, 3)
    leaf, _ = replay_descent(v, plant, 2)
    assert len(set(leaf.tolist())) == 3
    v["weight"][leaf[0]] = 0.1
    v["weight"][leaf[1]] = -1.5
    v["weight"][leaf[2]] = np.nan
    v["_plant"] = plant
    out["k10L4"] = (v, 2)
    out["k7L5"] = (synth.make_vocabulary(7, 5, seed=2), 4)
    out["k10L3"] = (synth.make_vocabulary(10, 3, seed=3), 4)
    p = dict(v)
    p["word_id"] = v["word_id"].copy()
    leaves = np.flatnonzero(np.diff(v["child_off"]) == 0)
    p["word_id"][leaves] = np.random.default_rng(101).permutation(leaves.size).astype(np.int32)
    out["permuted"] = (p, 2)
    c = synth.make_vocabulary(6, 3, seed=4)
    cnt = np.diff(c["child_off"]).copy()
    keep = np.ones(c["child_id"].size, bool)
    c["word_id"] = c["word_id"].copy(); c["weight"] = c["weight"].copy()
    for j, u in enumerate((2, 5)):      # two children of the root become leaves; their subtrees stay in the arrays, unreachable
        keep[c["child_off"][u]:c["child_off"][u + 1]] = False
        cnt[u] = 0
        c["word_id"][u] = c["word_id"].max() + 1 + j
        c["weight"][u] = 2.5 + j
    c["child_id"] = np.ascontiguousarray(c["child_id"][keep])
    c["child_off"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    out["cut"] = (c, 1)
    return out


# ---- keyframes ----------------------------------------------------------------------------------------------------------------------------------------------
def _kf(name, voc, desc, seed, xy=None, rec=REC):
    rng = np.random.default_rng(seed)
    n = len(desc)
    if xy is None:
        xy = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], 1).astype(f32)
    return dict(name=name, voc=voc, n=n, xy=np.ascontiguousarray(xy, f32).reshape(-1, 2), oct=rng.integers(0, 8, n).astype(np.uint8),
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), rec=np.asarray(rec, f32), angle=rng.uniform(0, 360, n).astype(f32))


@functools.lru_cache(maxsize=None)
def keyframes():
    """every planted keyframe, in a fixed order; the names are unique"""
    V = vocabularies()
    v = V["k10L4"][0]
    plant = v["_plant"]
    rng = np.random.default_rng(7)
    out = [_kf(f"n = {n}", "k10L4", _noisy(v, rng, n), 10 + i) for i, n in enumerate(SIZES)]
    # six identical descriptors on the word of weight 0.1 among others
    d = _noisy(v, rng, 300); d[[3, 50, 51, 120, 121, 299]] = plant[0]
    out.append(_kf("six on one word", "k10L4", d, 40))
    out.append(_kf("all on one word", "k10L4", np.repeat(_noisy(v, rng, 1), 100, axis=0), 41))
    # every word stopped: descriptors that fall on words of weight 0
    pool = _noisy(v, rng, 20000, flip=0.02)
    leaf, _ = replay_descent(v, pool, 2)
    stopped = pool[v["weight"][leaf] == 0][:70]
    assert len(stopped) >= 40
    out.append(_kf("every word stopped", "k10L4", stopped, 42))
    d = _noisy(v, rng, 400); d[5::7] = stopped[:len(d[5::7])]
    out.append(_kf("stopped among kept", "k10L4", d, 43))
    d = _noisy(v, rng, 130); d[[0, 64, 129]] = plant[1]; d[[1, 63, 65]] = plant[2]; d[2] = stopped[0]
    out.append(_kf("a negative and a NaN weight", "k10L4", d, 44))
    r2 = np.random.default_rng(45)
    xy = np.stack([r2.uniform(-200, 950, 500), r2.uniform(-150, 630, 500)], 1).astype(f32)
    xy[[0, 7, 499]] = [[np.nan, 10], [np.inf, -np.inf], [3e38, 5]]
    out.append(_kf("keypoints outside the grid", "k10L4", _noisy(v, rng, 500), 46, xy=xy, rec=rec_with(-17, -9, f32(75) / f32(769), f32(48) / f32(489))))
    for j, name in enumerate(("k7L5", "k10L3", "permuted", "cut")):
        vv = V[name][0]
        for n in (64, 257, 1000):
            out.append(_kf(f"{name}, n = {n}", name, _noisy(vv, rng, n), 50 + 3 * j + n % 3))
    assert len({k["name"] for k in out}) == len(out)
    return out


def by_vocabulary():
    """{vocabulary name: its keyframes}"""
    out = {}
    for k in keyframes():
        out.setdefault(k["voc"], []).append(k)
    return out


@functools.lru_cache(maxsize=None)
def message():
    """40 keyframes of 1 000 features on k10L4: a full message"""
    v = vocabularies()["k10L4"][0]
    rng = np.random.default_rng(8)
    return [_kf(f"message {m}", "k10L4", _noisy(v, rng, 1000), 200 + m) for m in range(40)]


_expected = {}


def expected(kf):
    """the replay's vectors of one keyframe, computed once"""
    if kf["name"] not in _expected:
        v, levelsup = vocabularies()[kf["voc"]]
        leaf, nid = replay_descent(v, kf["desc"], levelsup)
        _expected[kf["name"]] = replay_vectors(v, leaf, nid)
    return _expected[kf["name"]]


def call_arrays(kfs, first_key=1):
    """(keys, rec, feat_off, feat_xy, feat_octave, feat_desc, angle) of one call"""
    M = len(kfs)
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum([k["n"] for k in kfs])
    cat = lambda f, w, dt: np.concatenate([k[f].reshape(-1, w) for k in kfs]).astype(dt) if M else np.zeros((0, w), dt)
    return (np.arange(first_key, first_key + M, dtype=np.int64), np.concatenate([k["rec"] for k in kfs]).astype(f32) if M else np.zeros(0, f32), off, cat("xy", 2, f32),
            cat("oct", 1, np.uint8), cat("desc", 32, np.uint8), cat("angle", 1, f32))


VEC = ("bow_word", "bow_value", "fv_node", "fv_off", "fv_idx")


def same_vectors(got, want, tag, fields=VEC):
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, f, a.shape, b.shape)
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b), (tag, f)


def planted_properties():
    """what the planted keyframes are planted for, asserted on the replay itself, so that a product, a tree reduction or a reciprocal cannot pass"""
    kfs = {k["name"]: k for k in keyframes()}
    v = vocabularies()["k10L4"][0]
    e = expected(kfs["six on one word"])
    leaf, _ = replay_descent(v, v["_plant"], 2)
    w6 = int(v["word_id"][leaf[0]])
    r = e["raw"][e["bow_word"].tolist().index(w6)]
    assert r == 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1 and r != 6 * 0.1
    e = expected(kfs["n = 1000"])
    assert e["norm"] != float(np.sum(np.abs(np.array(e["raw"])))) and e["bow_word"].size > 128      # np.sum adds pairwise
    raw = np.array(e["raw"])
    assert not np.array_equal(raw / e["norm"], raw * (1.0 / e["norm"]))                              # a reciprocal and a product differ somewhere
    e = expected(kfs["all on one word"])
    assert e["bow_word"].size == 1 and e["fv_node"].size == 1 and e["fv_off"][-1] == 100
    e = expected(kfs["every word stopped"])
    assert e["bow_word"].size == 0 and e["fv_node"].size == 0 and np.array_equal(e["fv_off"], [0])
    e = expected(kfs["stopped among kept"])
    assert 0 < e["fv_off"][-1] < kfs["stopped among kept"]["n"]
    e = expected(kfs["a negative and a NaN weight"])
    assert 0 < e["fv_off"][-1] <= 130 - 7 and not ({0, 64, 129, 1, 63, 65, 2} & set(e["fv_idx"].tolist()))
    e = expected(kfs["k10L3, n = 257"])
    assert np.array_equal(e["fv_node"], [0])
    e = expected(kfs["cut, n = 1000"])
    cut = vocabularies()["cut"][0]
    assert e["fv_node"][0] == 0 and e["fv_node"].size > 1 and {int(cut["word_id"][2]), int(cut["word_id"][5])} <= set(e["bow_word"].tolist())
    p = expected(kfs["permuted, n = 1000"])
    assert np.all(np.diff(p["bow_word"]) > 0)
