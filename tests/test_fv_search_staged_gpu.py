"""GPU: ccm_bow_pair_eval_resident and ccm_tri_search_eval_resident are one stage function on two blocks (fv_pair_stage of csrc/fv_pair.h over BowPairResidentBlock
and TriSearchResidentBlock).  Here they alternate through ONE context's scratch and ONE store, at sizes that grow and then shrink: one job, every
planted case of tri_search_cases.planted_cases() in one call (keyframes of at most 200 features), one job again, so that each form finds the buffers as the other
form of another size left them: 64-bit words where 32-bit words were, two counters where three were, no level tables and job floats where there were some.  Every
table and counter equals its host evaluator's (exact)."""
import numpy as np
import pytest

from tri_search_cases import S2, SF, install, planted_cases


def _same(got, want, tag):
    assert np.array_equal(got["table"], want["table"]), tag
    for k in want:
        if k.startswith("n_"):
            assert np.array_equal(got[k], want[k]), (tag, k)


@pytest.mark.gpu
def test_the_two_searches_alternate_through_one_scratch_at_growing_and_shrinking_sizes():
    from ccm_slam_amd import bow_search as bs, kfstore as ks, tri_search as ts
    from ccm_slam_amd._lib import Context
    cases = planted_cases()
    assert max(max(c.kf1.n, c.kf2.n) for c in cases) <= 200
    ctx = Context(0)
    store = ks.KeyFrameStore(ctx, 2 * len(cases), 200)
    try:
        for i, c in enumerate(cases):
            install(store, 2 * i, 2 * i + 1, c)
        tri_all = [c.job(2 * i, 2 * i + 1) for i, c in enumerate(cases)]
        bow_all = [(2 * i, 2 * i + 1, 1 - c.kf1.has, 1 - c.kf2.has) for i, c in enumerate(cases)]   # SearchByBoW on the features the other search takes
        mid = len(cases) // 2
        rounds = [("one job", slice(0, 1)), ("all planted cases", slice(None)), ("one job again", slice(mid, mid + 1))]
        want = {tag: dict(bow=bs.pair_eval_host(store, bow_all[sl]), tri=ts.pair_eval_host(store, tri_all[sl], SF, S2)) for tag, sl in rounds}
        big = want["all planted cases"]
        assert big["bow"]["n_query"].sum() > 100 and big["tri"]["n_query"].sum() > 100 and big["tri"]["n_match"].sum() > 10 and big["bow"]["n_dist"].sum() > 1000
        assert big["bow"]["table"].size == big["tri"]["table"].size > 10 * want["one job"]["tri"]["table"].size
        for tag, sl in rounds:
            calls = dict(bow=lambda: bs.pair_eval_resident(ctx, store, bow_all[sl]), tri=lambda: ts.pair_eval_resident(ctx, store, tri_all[sl], SF, S2))
            for n, form in enumerate(("bow", "tri", "tri", "bow", "tri", "bow")):   # each form behind itself and behind the other
                _same(calls[form](), want[tag][form], (tag, n, form))
    finally:
        store.close()
        ctx.close()
