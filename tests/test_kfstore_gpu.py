"""GPU: the keyframe feature store (ccm_kfstore_*).  The grid kernel — KeyFrame::AssignFeaturesToGrid for every keyframe of an add in one launch —
read back through ccm_kfstore_get against the host store (csrc/kfstore_math.h under g++) and kfstore.build_grid_keyframe, the literal replay: every grid case of the
CPU file, adds of 1, 2, 3 and 40 keyframes of mixed sizes with a featureless one among them, a keyframe that fills its slot, the slot-reuse sequence, clear, and
every refusal.  Every comparison is exact."""
import numpy as np
import pytest

from ccm_slam_amd import kfstore as ks
from kfstore_cases import REC, add_one, bookkeeping_sequence, feats, grid_cases, refusals, same_grid

pytestmark = pytest.mark.gpu
f32 = np.float32


def test_device_grid_of_every_case_equals_the_host_store_and_the_replay(ctx):
    cases = grid_cases()
    dev = ks.KeyFrameStore(ctx, len(cases), 1008)
    host = ks.KeyFrameStore(None, len(cases), 1008)
    try:
        for key, (name, xy, rec) in enumerate(cases):
            add_one(dev, key, xy, rec); add_one(host, key, xy, rec)
        for key, (name, xy, rec) in enumerate(cases):
            got, want = dev.get(key), host.get(key)
            same_grid(got, xy, rec, name)
            assert (got["n"], got["n_in"]) == (want["n"], want["n_in"]) and np.array_equal(got["cell_off"], want["cell_off"]) and np.array_equal(got["cell_idx"], want["cell_idx"]), name
            sh = dev.get(key, shadow=True)
            assert np.array_equal(sh["cell_off"], got["cell_off"]) and np.array_equal(sh["cell_idx"], got["cell_idx"]), name
    finally:
        dev.close(); host.close()


@pytest.mark.parametrize("M", [1, 2, 3, 40])
def test_one_add_of_many_keyframes_of_mixed_sizes(ctx, M):
    rng = np.random.default_rng(30 + M)
    sizes = [int(rng.integers(1, 700)) for _ in range(M)]
    if M > 1:
        sizes[M // 2] = 0            # a keyframe without features among them
    if M > 2:
        sizes[0] = 700               # n == max_feat (the stride is 704)
    xys = [np.stack([rng.uniform(-20, 770, n), rng.uniform(-20, 500, n)], 1).astype(f32) for n in sizes]      # some keypoints outside the grid
    off = np.concatenate([[0], np.cumsum(sizes)])
    cat = lambda v, dt, w: np.concatenate([np.asarray(a, dt).reshape(-1, w) for a in v]).reshape(-1) if off[-1] else np.zeros(0, dt)
    oc = [feats(x, i)[0] for i, x in enumerate(xys)]; de = [feats(x, i)[1] for i, x in enumerate(xys)]
    dev = ks.KeyFrameStore(ctx, M + 1, 700)
    try:
        dev.add(range(1000, 1000 + M), np.tile(REC, M), off, cat(xys, f32, 2), cat(oc, np.uint8, 1), cat(de, np.uint8, 32))
        assert dev.count() == (M, 1)
        seen_out = 0
        for m in range(M):
            g = dev.get(1000 + m)
            same_grid(g, xys[m], REC, (M, m))
            seen_out += g["n"] - g["n_in"]
        assert M == 1 or seen_out > 0
    finally:
        dev.close()


def test_a_keyframe_that_fills_a_slot_of_65535_features(ctx):
    """the largest keyframe the store takes: every wave's quarter is 256 chunks long, and 16-bit indices reach 65 534"""
    rng = np.random.default_rng(3)
    n = 65535
    xy = np.stack([rng.uniform(-5, 760, n), rng.uniform(-5, 485, n)], 1).astype(f32)
    dev = ks.KeyFrameStore(ctx, 1, n)
    try:
        oc = np.zeros(n, np.uint8); de = np.zeros((n, 32), np.uint8)
        dev.add([1], REC, [0, n], xy, oc, de)
        g = dev.get(1)
        host = ks.KeyFrameStore(None, 1, n)
        host.add([1], REC, [0, n], xy, oc, de)
        want = host.get(1)
        assert g["n"] == n and 0 < g["n_in"] == want["n_in"] < n and np.array_equal(g["cell_off"], want["cell_off"]) and np.array_equal(g["cell_idx"], want["cell_idx"])
        assert all((np.diff(g["cell_idx"][a:b]) > 0).all() for a, b in zip(g["cell_off"][:-1:97], g["cell_off"][1::97]))      # ascending inside a cell
    finally:
        dev.close()


def test_slot_reuse_clear_and_every_refusal_on_the_device(ctx):
    dev = ks.KeyFrameStore(ctx, 4, 256)
    try:
        bookkeeping_sequence(dev)
        refusals(dev)
        dev.clear()
        assert dev.count() == (0, 4)
        with pytest.raises(ks.StoreError):
            dev.get(1)
        bookkeeping_sequence(dev)      # the cleared store takes the same keys again, into slots that held other keyframes
    finally:
        dev.close()
    for bad in ((0, 10), (1, 0), (1, 65536), (40000, 65535)):
        with pytest.raises(ks.CcmError):
            ks.KeyFrameStore(ctx, *bad)
