"""The device keyframe database (ccm_kfdb_*, ccm_slam_amd/kfdb.py) against the reference's KeyFrameDatabase (cslam/src/Database.cpp).

The checker is written here: RefKeyFrameDatabase restates Database.cpp line by line (one Python list per word in insertion order, erase of the
first occurrence, per-keyframe scratch, float32 through numpy) with fresh scratch per query, the contract of the device version
(include/ccm_hip.h); l1_score restates L1Scoring::score (thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-66) and is itself pinned to the
reference's compiled DBoW2 (oracle/_ref/libmatcher_ref.so: ref_bow_score).  phase1_vectorised is the numpy form used at 10 000 keyframes;
tests/test_kfdb_cpu.py checks it against the literal one.
"""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

from ccm_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libmatcher_ref.so")
F32 = np.float32


# ---- the checker ------------------------------------------------------------------------------------------------------------
def l1_score(qw, qv, kw, kv):
    """L1Scoring::score(q, kf): sum of fabs(v-w) - fabs(v) - fabs(w) over the common words in ascending word order, f64, then -score/2.0."""
    score = 0.0
    i = j = 0
    while i < len(qw) and j < len(kw):
        if qw[i] == kw[j]:
            vi, wi = float(qv[i]), float(kv[j])
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif qw[i] < kw[j]:
            i += 1
        else:
            j += 1
    return -score / 2.0


class RefKeyFrameDatabase:
    """Database.cpp with Python lists.  Keyframes are keys with a client id and a BowVector."""

    def __init__(self):
        self.inv = {}        # mvInvertedFile: word -> list of keys in insertion order
        self.bow = {}        # key -> (words, values)
        self.client = {}

    def add(self, key, client, words, values):                       # Database.cpp:37-43
        self.bow[key] = (list(int(w) for w in words), list(float(v) for v in values))
        self.client[key] = client
        for w in self.bow[key][0]:
            self.inv.setdefault(w, []).append(key)

    def erase(self, key):                                             # :45-64
        if key not in self.bow:
            return
        for w in self.bow[key][0]:
            lst = self.inv.get(w, [])
            if key in lst:
                lst.remove(key)                                       # the first occurrence

    def clear(self):                                                  # :66-70
        self.inv = {}

    def phase1(self, qw, qv, excluded):
        """:74-146 on fresh scratch: (listed keys in lKFsSharingWords order, count per key, maxCommonWords, minCommonWords, rows) where rows =
        [(key, count, si f32, score f64)] for count > minCommonWords in list order."""
        listed, count = [], {}
        for w in qw:
            for k in self.inv.get(int(w), []):
                if excluded(k):
                    continue
                if k not in count:
                    count[k] = 0
                    listed.append(k)
                count[k] += 1
        if not listed:
            return listed, count, 0, 0, []
        max_common = max(count[k] for k in listed)
        min_common = int(F32(max_common) * F32(0.8))
        rows = []
        for k in listed:
            if count[k] > min_common:
                s = l1_score(qw, qv, *self.bow[k])
                rows.append((k, count[k], F32(s), s))
        return listed, count, max_common, min_common, rows


def resolve(rows, min_score, neighbours):
    """Phase 2 (:148-201) in float32: accumulate by covisibility, retain > 0.75 * best, first occurrence of pBestKF wins."""
    scored = {k: si for k, _, si, _ in rows}
    min_score = F32(min_score)
    score_and_match = [(si, k) for k, _, si, _ in rows if si >= min_score]
    acc_and_match = []
    best_acc = min_score
    for si, k in score_and_match:
        best, acc, best_kf = si, si, k
        for k2 in list(neighbours.get(k, []))[:10]:
            if k2 in scored:
                acc = F32(acc + scored[k2])
                if scored[k2] > best:
                    best_kf, best = k2, scored[k2]
        acc_and_match.append((acc, best_kf))
        if acc > best_acc:
            best_acc = acc
    retain = F32(F32(0.75) * best_acc)
    out, seen = [], set()
    for acc, k in acc_and_match:
        if acc > retain and k not in seen:
            out.append(k)
            seen.add(k)
    return out, acc_and_match


def loop_excluded(ref, self_key, map_keys, connected):
    mk = None if map_keys is None else set(map_keys)
    cn = set(connected)
    return lambda k: k == self_key or (mk is not None and k not in mk) or k in cn


def group_excluded(ref, clients):
    cl = set(clients)
    return lambda k: ref.client[k] in cl


def phase1_vectorised(kf_keys, kf_words, kf_values, qw, qv, excluded_mask):
    """numpy form of RefKeyFrameDatabase.phase1 for a database built by adds only (list order = add order): kf_words / kf_values lists of arrays in
    add order, excluded_mask[i] for keyframe i.  Returns (n_sharing, max_common, rows)."""
    n = len(kf_words)
    lens = np.array([len(w) for w in kf_words])
    allw = np.concatenate(kf_words) if n else np.zeros(0, np.int64)
    owner = np.repeat(np.arange(n), lens)
    lut_w = np.asarray(qw, np.int64)
    pos = np.searchsorted(lut_w, allw)
    pos_c = np.minimum(pos, max(len(lut_w) - 1, 0))
    hit = (pos < len(lut_w)) & (lut_w[pos_c] == allw) if len(lut_w) else np.zeros(allw.size, bool)
    cnt = np.bincount(owner[hit], minlength=n)
    first = np.full(n, 1 << 30)
    np.minimum.at(first, owner[hit], pos_c[hit])
    cnt[excluded_mask] = 0
    listed = np.flatnonzero(cnt > 0)
    if listed.size == 0:
        return 0, 0, []
    order = listed[np.lexsort((listed, first[listed]))]
    max_common = int(cnt.max())
    min_common = int(F32(max_common) * F32(0.8))
    rows = []
    for i in order:
        if cnt[i] > min_common:
            s = l1_score(qw, qv, kf_words[i], kf_values[i])
            rows.append((kf_keys[i], int(cnt[i]), F32(s), s))
    return int(listed.size), max_common, rows


# ---- synthetic maps ---------------------------------------------------------------------------------------------------------
def bow(rng, words):
    w = np.unique(np.asarray(words, np.int64)).astype(np.int32)
    v = rng.uniform(0.05, 1.0, w.size)
    return w, v / v.sum()


def place_map(rng, n_words, n_places, base_words, keep=0.7, extra=10):
    base = [rng.choice(n_words, base_words, replace=False) for _ in range(n_places)]

    def kf_at(p):
        b = base[p % n_places]
        w = np.concatenate([b[rng.random(b.size) < keep], rng.choice(n_words, extra), base[(p + 1) % n_places][:base_words // 8]])
        return bow(rng, w)
    return kf_at


def revisit_map(seed=0, n_words=3000):
    """Four agents (client ids 0..3) walking 24 places, three keyframes per place, with revisits; keys = id << 8 | client; covisibility = the
    agent's keyframes within +-4 along its trajectory, nearest first."""
    rng = np.random.default_rng(seed)
    kf_at = place_map(rng, n_words, 24, 120)
    kfs, nb = [], {}
    for a in range(4):
        path = [(a * 5 + t // 3) % 24 for t in range(60)] + [(a * 5 + t // 3) % 24 for t in range(18)]   # three keyframes per place; a second lap revisits
        keys = [(t << 8) | a for t in range(len(path))]
        for t, p in enumerate(path):
            w, v = kf_at(p)
            kfs.append((keys[t], a, w, v))
        for t in range(len(path)):
            order = sorted([u for u in range(max(0, t - 4), min(len(path), t + 5)) if u != t], key=lambda u: (abs(u - t), u))
            nb[keys[t]] = [keys[u] for u in order][:10]
    return kfs, nb, kf_at


def _rows_equal(got, rows):
    assert list(got["key"]) == [r[0] for r in rows]
    assert list(got["count"]) == [r[1] for r in rows]
    assert np.array_equal(got["score"], np.array([r[2] for r in rows], np.float32))
    assert np.array_equal(got["score64"].view(np.uint64), np.array([r[3] for r in rows], np.float64).view(np.uint64))


# ---- tests ------------------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kfdb_mod():
    from ccm_slam_amd import kfdb
    return kfdb


def _write_orbvoc_txt(path, vocab, k):
    """ORBvoc.txt text format (TemplatedVocabulary::loadFromTextFile): header 'k L scoring weighting', then per non-root node: parent, is-leaf,
    the 32 descriptor bytes, the weight"""
    n = vocab["n_nodes"]
    with open(path, "w") as f:
        f.write(f"{k} {vocab['L']} 0 0\n")
        lines = []
        for i in range(1, n):
            leaf = int(vocab["child_off"][i + 1] == vocab["child_off"][i])
            lines.append(f"{(i - 1) // k} {leaf} " + " ".join(str(int(b)) for b in vocab["node_desc"][i]) + f" {float(vocab['weight'][i])!r}")
        f.write("\n".join(lines))


@pytest.mark.skipif(not os.path.exists(REF_LIB) and not os.path.isdir("/root/reference/cslam"), reason="oracle/_ref not built")
def test_score_bits_against_the_references_dbow2(ctx, kfdb_mod, tmp_path):
    """ccm_kfdb_score vs ref_bow_score (the reference's DBoW2 L1Scoring, compiled verbatim) bit for bit in f64, on BowVectors that the
    reference's own TemplatedVocabulary::transform produced: identical, disjoint (-0.0), one common word, 1 vs ~1000 words, random pairs."""
    if not os.path.exists(REF_LIB):
        import oracle.ref as ref
        ref.build()
    rlib = C.CDLL(REF_LIB)
    rlib.ref_vocab_load_text.restype = C.c_void_p
    rlib.ref_bow_score.restype = C.c_double
    k, L = 10, 4
    vocab = synth.make_vocabulary(k, L, seed=3)
    path = str(tmp_path / "voc.txt")
    _write_orbvoc_txt(path, vocab, k)
    h = rlib.ref_vocab_load_text(path.encode())
    assert h
    rng = np.random.default_rng(11)
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def ref_bow(N):
        desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
        ids = np.zeros(N, np.int32); vals = np.zeros(N, np.float64); nfv = np.zeros(1, np.int32)
        fvn = np.zeros(N, np.int32); fvo = np.zeros(N + 1, np.int32); fvf = np.zeros(N, np.int32)
        n = rlib.ref_bow_transform(C.c_void_p(h), P(desc), N, 4, P(ids), P(vals), P(nfv), P(fvn), P(fvo), P(fvf))
        return ids[:n].copy(), vals[:n].copy()

    def ref_score(a, b):
        return rlib.ref_bow_score(C.c_void_p(h), P(a[0]), P(a[1]), a[0].size, P(b[0]), P(b[1]), b[0].size)

    try:
        db = kfdb_mod.KeyFrameDatabase(ctx, k ** L)
        q = ref_bow(1500)
        assert q[0].size > 900
        other = ref_bow(1500)
        disjoint = tuple(x[~np.isin(other[0], q[0])] for x in other)
        one = (np.sort(np.concatenate([disjoint[0][:50], q[0][7:8]])), None)
        one = (one[0], np.concatenate([disjoint[1][:50], [0.013]])[np.argsort(np.concatenate([disjoint[0][:50], q[0][7:8]]))])
        single = (q[0][100:101].copy(), np.array([1.0]))
        cases = {1: q, 2: disjoint, 3: one, 4: other}
        for i in range(5, 25):
            cases[i] = ref_bow(int(rng.integers(50, 1500)))
        for key, (w, v) in cases.items():
            db.add(key, 0, w, v)
        for qq in (q, single, other):
            keys = list(cases)
            got = db.score(qq[0], qq[1], keys)
            exp = np.array([ref_score(qq, cases[kk]) for kk in keys])
            assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
        got = db.score(q[0], q[1], [1, 2, 3])
        assert got[0] == ref_score(q, q) and got[0] > 0.999                       # identical
        assert got[1] == 0.0 and np.signbit(got[1])                               # disjoint: -0.0
        assert np.signbit(ref_score(q, disjoint))
        assert got[2] > 0                                                          # one common word
        assert l1_score(q[0], q[1], one[0], one[1]) == got[2]                     # the restatement agrees with the reference's bits
        db.close()
    finally:
        rlib.ref_vocab_free(C.c_void_p(h))


def _check_all_filters(db, ref, rng, kf_at, live_keys, clients=4):
    live = sorted(live_keys)
    for trial in range(3):
        qw, qv = kf_at(int(rng.integers(0, 1000)))
        self_key = live[int(rng.integers(0, len(live)))] if live else -1
        map_keys = [k for k in live if rng.random() < 0.7]
        connected = [k for k in live if rng.random() < 0.15]
        groups = [c for c in range(clients) if rng.random() < 0.4]
        for excl, kw in ((lambda k: False, {}),
                         (loop_excluded(ref, self_key, None, connected), dict(self_key=self_key, exclude=connected)),
                         (loop_excluded(ref, self_key, map_keys, connected), dict(self_key=self_key, allow=map_keys, exclude=connected)),
                         (lambda k: ref.client[k] in groups, dict(exclude_groups=sum(1 << c for c in groups)))):
            listed, count, max_common, _, rows = ref.phase1(qw, qv, excl)
            got = db.query(qw, qv, **kw)
            assert got["n_sharing"] == len(listed) and got["max_common"] == max_common
            _rows_equal(got, rows)


def test_phase1_tables_through_add_erase_clear_and_rebuilds(ctx, kfdb_mod):
    """Random interleavings of add / erase (also of unknown keys) / clear / re-add with log_capacity 3, so the device file is rebuilt and compacted many
    times: every phase-1 table (keys in lKFsSharingWords order, counts, f32 and f64 scores, n_sharing, max_common) equals the restatement, under
    every filter kind (none, self + connected, map membership, client ids)."""
    rng = np.random.default_rng(1)
    n_words = 2000
    kf_at = place_map(rng, n_words, 12, 60)
    db = kfdb_mod.KeyFrameDatabase(ctx, n_words, log_capacity=3)
    ref = RefKeyFrameDatabase()
    live, next_key, checks, rebuilt = set(), 0, 0, 0
    for step in range(260):
        u = rng.random()
        if u < 0.6 or not live:
            key = next_key if rng.random() < 0.8 or not ref.bow else int(rng.choice([k for k in ref.bow if k not in live] or [next_key]))
            if key == next_key:
                next_key += 1
            w, v = kf_at(int(rng.integers(0, 40)))
            c = int(rng.integers(0, 4))
            db.add(key, c, w, v)
            ref.add(key, c, w, v)
            live.add(key)
        elif u < 0.9:
            key = int(rng.choice(sorted(live))) if rng.random() < 0.9 else 10 ** 6 + step
            db.erase(key)
            if key in live:
                ref.erase(key)
                live.discard(key)
        elif u < 0.93:
            db.clear()
            ref.clear()
            live.clear()
        if step % 7 == 0:
            _check_all_filters(db, ref, rng, kf_at, live)
            checks += 1
        rebuilt += 1
    assert checks > 30
    # no shared word / empty query: an empty table
    got = db.query(np.array([n_words - 1], np.int32), np.array([1.0]))
    if not ref.inv.get(n_words - 1):
        assert got["key"].size == 0 and got["n_sharing"] == 0
    db.clear()
    got = db.query(*kf_at(3))
    assert got["key"].size == 0 and got["n_sharing"] == 0 and got["max_common"] == 0
    db.close()


def test_candidates_of_a_four_agent_revisit_map(ctx, kfdb_mod):
    """DetectLoopCandidates / DetectMapMatchCandidates / DetectRelocalizationCandidates through the host mirror equal the restatement, order included, on a
    map where candidates come out, covisibility accumulation changes scores and several matches share one pBestKF."""
    kfs, nb, kf_at = revisit_map()
    db = kfdb_mod.KeyFrameDatabase(ctx, 3000, log_capacity=16)
    ref = RefKeyFrameDatabase()
    for key, c, w, v in kfs:
        db.add(key, c, w, v)
        ref.add(key, c, w, v)
    n_cand = n_acc = n_repeat = 0
    for key, c, w, v in kfs[::3]:
        map_keys = [k for k, cc, _, _ in kfs if cc in (c, (c + 1) % 4)]
        connected = nb[key][:6]
        for min_score in (0.0, 0.02):
            _, _, _, _, rows = ref.phase1(w, v, loop_excluded(ref, key, map_keys, connected))
            exp, acc = resolve(rows, min_score, nb)
            got = db.detect_loop_candidates(key, w, v, min_score, map_keys, connected, nb)
            assert got == exp
            n_cand += len(exp)
            n_acc += sum(1 for a, (k, _, si, _) in zip(acc, [r for r in rows if r[2] >= F32(min_score)]) if a[0] != si)
            n_repeat += len(acc) - len({k for _, k in acc})
        clients = [c]
        _, _, _, _, rows = ref.phase1(w, v, group_excluded(ref, clients))
        exp, _ = resolve(rows, 0.01, nb)
        assert db.detect_map_match_candidates(w, v, 0.01, clients, nb) == exp
        n_cand += len(exp)
        _, _, _, _, rows = ref.phase1(w, v, lambda k: False)
        exp, _ = resolve(rows, 0.0, nb)
        assert db.detect_relocalization_candidates(w, v, nb) == exp
    assert n_cand > 50 and n_acc > 20 and n_repeat > 5, (n_cand, n_acc, n_repeat)
    db.close()


def test_scale_10000_keyframes(ctx, kfdb_mod):
    """10 000 keyframes of ~800 words over a 10^6-word vocabulary (default log capacity): a few queries against the vectorised restatement."""
    rng = np.random.default_rng(7)
    n_words = 1_000_000
    kf_at = place_map(rng, n_words, 500, 850, keep=0.8, extra=60)
    db = kfdb_mod.KeyFrameDatabase(ctx, n_words)
    keys, words, values = [], [], []
    for i in range(10_000):
        w, v = kf_at(int(rng.integers(0, 500)))
        key = (i << 8) | (i % 4)
        db.add(key, i % 4, w, v)
        keys.append(key); words.append(w); values.append(v)
    assert 700 < np.mean([w.size for w in words]) < 900
    for t in range(4):
        qw, qv = kf_at(int(rng.integers(0, 500)))
        excl = np.zeros(len(keys), bool)
        if t % 2:
            excl[rng.random(len(keys)) < 0.2] = True
        n_sharing, max_common, rows = phase1_vectorised(keys, words, values, qw, qv, excl)
        got = db.query(qw, qv, allow=[k for k, e in zip(keys, excl) if not e] if t % 2 else None)
        assert got["n_sharing"] == n_sharing and got["max_common"] == max_common
        assert len(rows) > 5
        _rows_equal(got, rows)
    db.close()


def test_concurrent_queries_and_a_writer(kfdb_mod):
    """Four threads with their own contexts query one database at once: every result equals the solo run.  Then one thread adds while three query: each
    result equals the restatement at the generation the query saw."""
    from ccm_slam_amd._lib import Context
    rng = np.random.default_rng(3)
    n_words = 4000
    kf_at = place_map(rng, n_words, 20, 100)
    main = Context(0)
    db = kfdb_mod.KeyFrameDatabase(main, n_words, log_capacity=8)
    ref = RefKeyFrameDatabase()
    for key in range(300):
        w, v = kf_at(key % 40)
        db.add(key, key % 4, w, v)
        ref.add(key, key % 4, w, v)
    queries = [kf_at(int(p)) for p in rng.integers(0, 40, 12)]
    solo = [db.query(*q) for q in queries]
    errors = []

    def reader(tid, out, rounds, start=None, writing=None):
        ctx = Context(0)
        try:
            if start is not None:
                start.wait()
            r = 0
            while r < rounds or (writing is not None and writing.is_set()):
                for qi, q in enumerate(queries):
                    out.append((qi, db.query(*q, ctx=ctx)))
                r += 1
        except Exception as e:   # noqa: BLE001
            errors.append(e)
        finally:
            ctx.close()

    outs = [[] for _ in range(4)]
    th = [threading.Thread(target=reader, args=(i, outs[i], 3)) for i in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    for out in outs:
        assert len(out) == 36
        for qi, got in out:
            for f in ("key", "count", "score"):
                assert np.array_equal(got[f], solo[qi][f])
            assert np.array_equal(got["score64"].view(np.uint64), solo[qi]["score64"].view(np.uint64))
    # one writer, three readers
    gen0 = solo[0]["generation"]
    new = [(300 + i, kf_at(int(rng.integers(0, 40)))) for i in range(40)]
    expected = {}
    snap = RefKeyFrameDatabase()
    snap.inv = {w: list(l) for w, l in ref.inv.items()}; snap.bow = dict(ref.bow); snap.client = dict(ref.client)
    for g in range(len(new) + 1):
        if g:
            key, (w, v) = new[g - 1]
            snap.add(key, key % 4, w, v)
        expected[gen0 + g] = [snap.phase1(q[0], q[1], lambda k: False) for q in queries[:4]]

    start, writing = threading.Barrier(4), threading.Event()
    writing.set()

    def writer():
        ctx = Context(0)
        try:
            start.wait()
            for key, (w, v) in new:
                db.add(key, key % 4, w, v, ctx=ctx)
                time.sleep(0.002)
        except Exception as e:   # noqa: BLE001
            errors.append(e)
        finally:
            writing.clear()
            ctx.close()

    queries_all = queries
    queries = queries_all[:4]
    outs = [[] for _ in range(3)]
    th = [threading.Thread(target=writer)] + [threading.Thread(target=reader, args=(i, outs[i], 2, start, writing)) for i in range(3)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    gens = set()
    for out in outs:
        for qi, got in out:
            listed, _, max_common, _, rows = expected[got["generation"]][qi]
            gens.add(got["generation"])
            assert got["n_sharing"] == len(listed) and got["max_common"] == max_common
            _rows_equal(got, rows)
    assert len(gens) >= 5, sorted(gens)                                    # the queries saw the database grow
    db.close()
    main.close()


def test_error_paths(ctx, kfdb_mod):
    from ccm_slam_amd._lib import CcmError, lib
    db = kfdb_mod.KeyFrameDatabase(ctx, 100)
    # empty database: an empty table
    got = db.query(np.array([1, 2], np.int32), np.array([0.5, 0.5]))
    assert got["key"].size == 0 and got["n_sharing"] == 0 and got["generation"] == 0
    for w in ([3, 2], [2, 2], [5, 100], [-1, 4]):
        with pytest.raises(CcmError, match="-1"):
            db.add(1, 0, np.array(w, np.int32), np.array([0.5, 0.5]))
        with pytest.raises(CcmError, match="-1"):
            db.query(np.array(w, np.int32), np.array([0.5, 0.5]))
    db.add(1, 0, np.array([2, 3], np.int32), np.array([0.5, 0.5]))
    with pytest.raises(CcmError, match="-6"):
        db.add(1, 0, np.array([4], np.int32), np.array([1.0]))
    db.erase(12345)                                                           # unknown key: no-op
    assert db.query(np.array([3], np.int32), np.array([1.0]))["generation"] == 1
    got = db.query(np.array([7], np.int32), np.array([1.0]))                 # no shared word
    assert got["key"].size == 0 and got["n_sharing"] == 0
    with pytest.raises(CcmError, match="-1"):
        db.score(np.array([3], np.int32), np.array([1.0]), [99])
    db.erase(1)
    db.add(1, 0, np.array([4], np.int32), np.array([1.0]))                   # re-adding an erased key is fine
    with pytest.raises(CcmError):
        kfdb_mod.KeyFrameDatabase(ctx, 0)
    if lib().ccm_device_count() > 1:                                          # a context on another device
        from ccm_slam_amd._lib import Context
        other = Context(1)
        with pytest.raises(CcmError, match="-1"):
            db.add(2, 0, np.array([4], np.int32), np.array([1.0]), ctx=other)
        other.close()
    db.close()
