"""The per-frame kernels (csrc/frame.hip: grid, window count / fill, scan, frustum; csrc/hamming.hip: bow_descend_kernel) at the sizes where their launch shape
changes and on values planted on their thresholds.  Everything is integer or bit-identical f32 work: no assertion here has a tolerance.  The expected result is
tests/frame_reference.py (a NumPy restatement, pinned to the oracle by tests/test_frame_reference_cpu.py); the oracle is compared too wherever the input lies in
the source's defined domain.  The cases are tests/frame_edge_cases.py.

36 tests, 1.1 s on an MI355X; the shapes, the measured counts and the mutations that fail this file are in DESIGN.md §4.4.1."""
import ctypes as C
import os

import numpy as np
import pytest

import frame_edge_cases as fc
import frame_reference as fr
from ccm_slam_amd import matcher
from ccm_slam_amd.frame import FrameGrid, is_in_frustum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_FORMS = {"dist_zeros4": np.zeros(4, np.float32), "n_dist_0": np.zeros(0, np.float32)}     # both are "no distortion": positions reach the grid as written


@pytest.fixture(scope="module", params=list(DIST_FORMS))
def grid(ctx, request):
    fg = FrameGrid(ctx, fc.EUROC_K, DIST_FORMS[request.param], fc.W, fc.H)
    assert np.array_equal(fg.bounds, np.array(fc.BOUNDS))
    yield fg
    fg.close()


@pytest.fixture(scope="module")
def grid0(ctx):
    fg = FrameGrid(ctx, fc.EUROC_K, np.zeros(0, np.float32), fc.W, fc.H)
    yield fg
    fg.close()


def _check_grid(fg, kps, desc, oracle_lib=None):
    fg.set_keypoints(kps, desc)
    xy, off, idx = fg.get()
    assert np.array_equal(xy.view(np.uint32), np.stack([kps["x"], kps["y"]], 1).view(np.uint32))     # bits: -0.0 and NaN travel as they are
    eoff, eidx = fr.build_grid(fc.BOUNDS, kps["x"], kps["y"])
    assert np.array_equal(off, eoff) and np.array_equal(idx, eidx)
    if oracle_lib is not None:
        ooff, oidx = oracle_lib.build_grid(kps["x"], kps["y"], fc.BOUNDS)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    return off, idx


def test_grid_sizes_growth_and_reuse_on_one_handle(grid, oracle_lib):
    """N = 1, 1023, 1024, 1025 (the stride loops' second trip), 2048, 2049, 3100 (frame_reserve grows past its first capacity) and then 5 on the same handle"""
    for n in fc.GRID_SIZES:
        off, _ = _check_grid(grid, *fc.grid_size_kps(n), oracle_lib)
    assert fc.GRID_SIZES[-1] == 5 and off[-1] == 5


def test_crowded_cells_come_out_in_ascending_order(grid, oracle_lib):
    (kps, desc), cells = fc.crowded_case()
    off, idx = _check_grid(grid, kps, desc, oracle_lib)
    for c in np.unique(cells):
        lst = idx[off[c]:off[c + 1]]
        assert lst.size == 500 and (np.diff(lst) > 0).all()
    assert off[-1] == 1500 and all((np.diff(idx[off[c]:off[c + 1]]) > 0).all() for c in range(fr.N_CELLS))


def test_keypoints_outside_and_on_the_rim(grid, oracle_lib):
    kps, desc = fc.rim_case()
    off, _ = _check_grid(grid, kps, desc, oracle_lib)
    assert len(kps) - off[-1] == (fr.cell_of(fc.BOUNDS, kps["x"], kps["y"]) < 0).sum() > 0           # the dropped count
    kps, desc = fc.rim_case(wild=True)                                                                # NaN, Inf, 3e38: in no cell (reference only)
    off, _ = _check_grid(grid, kps, desc)
    assert len(kps) - off[-1] == (fr.cell_of(fc.BOUNDS, kps["x"], kps["y"]) < 0).sum()


def test_half_cell_ties_go_to_the_upper_cell(grid, oracle_lib):
    (kps, desc), exp, tx, ty = fc.tie_case()
    off, idx = _check_grid(grid, kps, desc, oracle_lib)
    got = np.full(len(kps), -1, np.int64)
    got[idx] = np.repeat(np.arange(fr.N_CELLS), np.diff(off))
    assert np.array_equal(got, exp) and len(tx) >= 40 and len(ty) >= 20


def _search(fg, q):
    return fg.window_search(q["u"], q["v"], q["r"], q["minl"], q["maxl"], q["qdesc"])


def _check_windows(fg, kps, desc, q, oracle_lib=None, expected=None):
    off, idx, dist = _search(fg, q)
    eoff, eidx = expected if expected is not None else fr.window_candidates(fc.BOUNDS, kps["x"], kps["y"], kps["octave"], q["u"], q["v"], q["r"], q["minl"], q["maxl"])
    assert np.array_equal(off, eoff) and np.array_equal(idx, eidx)
    assert np.array_equal(dist, fr.hamming(np.repeat(q["qdesc"], np.diff(off), axis=0), desc[idx]))
    if oracle_lib is not None:
        ooff, oidx = oracle_lib.grid_candidates(kps["x"], kps["y"], kps["octave"], fc.BOUNDS, q["u"], q["v"], q["r"], q["minl"], q["maxl"])
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    return off, idx


@pytest.fixture(scope="module")
def count_case():
    kps, desc, q = fc.query_count_case()
    return kps, desc, q, fr.window_candidates(fc.BOUNDS, kps["x"], kps["y"], kps["octave"], q["u"], q["v"], q["r"], q["minl"], q["maxl"])


@pytest.mark.parametrize("Q", fc.QUERY_COUNTS)
def test_query_counts_around_the_block_and_the_scan_steps(grid0, oracle_lib, count_case, Q):
    """8 queries per block (Q = 7, 8, 9) and the scan's ceil(Q / 1024) (Q = 1023, 1024, 1025, 2049)"""
    kps, desc, q, (eoff, eidx) = count_case
    grid0.set_keypoints(kps, desc)
    _check_windows(grid0, kps, desc, fc.take(q, slice(0, Q)), oracle_lib, expected=(eoff[:Q + 1], eidx[:eoff[Q]]))


def test_window_shapes(grid, oracle_lib):
    kps, desc, q, row = fc.window_shape_case()
    grid.set_keypoints(kps, desc)
    off, idx = _check_windows(grid, kps, desc, q, oracle_lib)
    lst = lambda name: idx[off[row[name]]:off[row[name] + 1]]
    assert lst("r0_on_keypoint").size == 0
    assert fc.B_IDX not in lst("dx_equals_r") and fc.B_IDX in lst("dx_below_next_r")
    assert lst("cells_16")[-1] == fc.C_IDX and lst("cells_17")[-1] == fc.D_IDX                 # the candidate of the 16th cell, and of the 17th: the second trip
    assert np.array_equal(lst("whole_grid"), grid.get()[2])                                # 225 trips: the grid's own list, whatever a reference says
    for name in ("left_of", "right_of", "above", "below"):
        assert lst(name).size == 0
    for name in ("cells_16", "cells_17", "corner_00", "corner_w0", "corner_0h", "corner_wh", "straddle_left", "straddle_right", "straddle_top", "straddle_bottom"):
        assert lst(name).size > 0, name


def test_level_windows(grid0, oracle_lib):
    kps, desc, q = fc.level_case()
    grid0.set_keypoints(kps, desc)
    off, idx = _check_windows(grid0, kps, desc, q, oracle_lib)
    lists = {p: idx[off[i]:off[i + 1]] for i, p in enumerate(fc.LEVEL_PAIRS)}
    assert lists[(5, 2)].size == 0
    # (0, -1) checks no level: everything the window holds, counted here over the keypoints that are in the grid
    inside = (fr.cell_of(fc.BOUNDS, kps["x"], kps["y"]) >= 0) & (np.abs(kps["x"] - q["u"][0]) < q["r"][0]) & (np.abs(kps["y"] - q["v"][0]) < q["r"][0])
    assert np.array_equal(lists[(0, -1)], lists[(-1, -1)]) and np.array_equal(np.sort(lists[(0, -1)]), np.nonzero(inside)[0])
    assert (kps["octave"][lists[(7, 7)]] == 7).all() and set(kps["octave"][lists[(2, 5)]].tolist()) == {2, 3, 4, 5} and (kps["octave"][lists[(3, -1)]] >= 3).all()


def test_capacity_equal_to_one_short_of_and_zero(grid0):
    from ccm_slam_amd._lib import lib
    kps, desc, q = fc.query_count_case()
    grid0.set_keypoints(kps, desc)
    Q = 40
    q = fc.take(q, slice(0, Q))
    eoff, eidx, edist = _search(grid0, q)
    total = int(eoff[-1])
    assert total > 100
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pad = 64

    def call(cap):
        off = np.full(Q + 1, -3, np.int32); idx = np.full(total + pad, -7, np.int32); dist = np.full(total + pad, 9999, np.uint16); n = C.c_int64(-1)
        rc = lib().ccm_frame_window_search(grid0._h, Q, p(q["u"]), p(q["v"]), p(q["r"]), p(q["minl"]), p(q["maxl"]), p(q["qdesc"]), p(off), p(idx) if cap else None,
                                           p(dist) if cap else None, C.c_int64(cap), C.byref(n))
        return rc, off, idx, dist, n.value
    rc, off, idx, dist, n = call(total)                                 # exactly enough
    assert rc == 0 and n == total and np.array_equal(off, eoff) and np.array_equal(idx[:total], eidx) and np.array_equal(dist[:total], edist)
    assert (idx[total:] == -7).all() and (dist[total:] == 9999).all()
    rc, off, idx, dist, n = call(total - 1)                             # one short: refused, the size reported, nothing written
    assert rc != 0 and n == total and np.array_equal(off, eoff) and (idx == -7).all() and (dist == 9999).all()
    rc, off, idx, dist, n = call(0)                                     # sizing call: offsets only
    assert rc == 0 and n == total and np.array_equal(off, eoff) and (idx == -7).all() and (dist == 9999).all()


@pytest.fixture(scope="module")
def hostlib():
    return C.CDLL(os.path.join(ROOT, "ccm_slam_amd", "libccm_host.so"))


def test_the_cell_range_is_total(grid0, hostlib, oracle_lib):
    """u, v in {NaN, +-inf} and r in {NaN, -1, -100, -240 (whose unchecked range is inverted), +inf, 1e12, 3e38} between ordinary queries of the same 8-query
    blocks.  Expected: the reference alone (the source's conversion is undefined there).  The ordinary neighbours keep their lists, and the host evaluator, which
    compiles the same frame_cell_range, gives what the device gives."""
    kps, desc, q, ordinary = fc.total_range_case()
    grid0.set_keypoints(kps, desc)
    off, idx = _check_windows(grid0, kps, desc, q)
    whole = grid0.get()[2]
    for i in np.nonzero(~ordinary)[0]:
        u, v, r = q["u"][i], q["v"][i], q["r"][i]
        empty = np.isnan(u) or np.isnan(v) or np.isnan(r) or r < 0 or np.isinf(u) or np.isinf(v)
        assert (off[i + 1] == off[i]) if empty else np.array_equal(idx[off[i]:off[i + 1]], whole), (u, v, r)
    ooff, oidx = _check_windows(grid0, kps, desc, fc.take(q, ordinary), oracle_lib)                   # the ordinary queries alone: the same lists
    n = np.diff(off)
    assert np.array_equal(np.diff(ooff), n[ordinary]) and np.array_equal(oidx, idx[np.repeat(ordinary, n)])
    # host evaluator and its device-grid form: r = th * mvScaleFactors[level] with th = 1, so the table carries each special radius to the window as it is
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    kx, ky, oc = (np.ascontiguousarray(kps[f]) for f in ("x", "y", "octave"))
    N, n_pts = len(kps), q["u"].size
    level = np.full(n_pts, 3, np.int32); valid = np.ones(n_pts, np.uint8); is2 = np.ones(8, np.float32)
    for r in (fc.F(25.0),) + fc.BAD_R:
        sf = np.ones(8, np.float32); sf[3] = r
        eoff, eidx = fr.window_candidates(fc.BOUNDS, kx, ky, oc, q["u"], q["v"], np.full(n_pts, r, np.float32), level - 1, level)
        ebi = np.full(n_pts, -1, np.int32); ebd = np.full(n_pts, np.iinfo(np.int32).max, np.int32)
        for i in range(n_pts):
            cand = eidx[eoff[i]:eoff[i + 1]]
            if cand.size:
                d = fr.hamming(q["qdesc"][i], desc[cand])
                ebi[i], ebd[i] = cand[np.argmin(d)], d.min()
        for dev in (False, True):
            bi = np.zeros(n_pts, np.int32); bd = np.zeros(n_pts, np.int32)
            b4 = [C.c_float(752.0), C.c_float(480.0)] if dev else [C.c_float(b) for b in fc.BOUNDS]
            fn = hostlib.ccmh_projected_window_search_dev if dev else hostlib.ccmh_projected_window_search
            got = fn(0, p(kx), p(ky), p(oc), p(desc), N, *b4, p(sf), p(is2), n_pts, p(valid), p(q["u"]), p(q["v"]), p(level), p(q["qdesc"]), C.c_float(1.0), 0, 256, None, 0,
                     None, p(bi), p(bd))
            assert got == (ebi >= 0).sum() and np.array_equal(bi, ebi) and np.array_equal(bd, ebd), (r, dev)


# ---- frustum --------------------------------------------------------------------------------------------------------------------------------------------
def _frustum_equals_oracle(ctx, oracle_lib, frame, P, Pn, dmin, dmax):
    got = is_in_frustum(ctx, frame, fc.N_LEVELS, P, Pn, dmin, dmax, 0.5)
    exp = oracle_lib.is_in_frustum(frame, fc.N_LEVELS, P, Pn, dmin, dmax, 0.5)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[3], exp[3])
    for g, e in ((got[1], exp[1]), (got[2], exp[2]), (got[4], exp[4])):
        assert ((g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))).all()          # bit for bit; a NaN (0 * inf at Pc.z == 0) equals a NaN
    return got


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_frustum_counts_around_the_block(ctx, oracle_lib, n):
    frame, P, Pn, dmin, dmax = fc.frustum_random_case(257, 3)
    got = _frustum_equals_oracle(ctx, oracle_lib, frame, P[:n], Pn[:n], dmin[:n], dmax[:n])
    assert n < 255 or 0.02 < got[0].mean() < 0.6


def test_frustum_equality_table(ctx, oracle_lib):
    """one row ON each comparison's equality: u == minX / maxX, v == minY / maxY, Pc.z == +-0 and the least negative float, dist == 1.2f dmax, dist == 0.8f dmin,
    viewCos == 0.5, level quotients that are exact integers (and their next floats), a ratio below 1 and one that clamps"""
    rows = fc.frustum_table()
    fc.check_frustum_table(rows)
    got = _frustum_equals_oracle(ctx, oracle_lib, fc.TABLE_FRAME, *fc.table_arrays(rows))
    for i, r in enumerate(rows):
        assert got[0][i] == r[5] and (r[6] is None or got[3][i] == r[6]), r[0]


@pytest.mark.parametrize("test", fc.PLANT_TESTS)
def test_frustum_adjacent_floats_across_every_rejection(ctx, oracle_lib, test):
    """two adjacent f32 values of one input on which the oracle's flag differs, for 64 base points: the device gives the oracle's five outputs on both"""
    (P, Pn, dmin, dmax), near = fc.plant_adjacent(oracle_lib.is_in_frustum, test)
    assert near.sum() >= 58
    keep = np.concatenate([near, near])
    got = _frustum_equals_oracle(ctx, oracle_lib, fc.PLANT_FRAME, P[keep], Pn[keep], dmin[keep], dmax[keep])
    n = int(near.sum())
    assert got[0][:n].all() and not got[0][n:].any()


# ---- vocabulary descent ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["wide", "ragged"])
def test_bow_descent_on_wide_and_ragged_trees(ctx, oracle_lib, tree):
    """nodes with 1, 2, 63, 64, 65 and 130 children (one, two and three trips of 64), leaves at depths 1..L, N around the 4 features per block, every levelsup
    from the leaves to above the root"""
    vocab, _ = fc.wide_vocabulary() if tree == "wide" else fc.ragged_vocabulary()
    L = vocab["L"]
    desc = fc.bow_queries(vocab, 1023, 70 + L)
    if tree == "wide":
        desc[:2] = vocab["node_desc"][[fc.TIE_FIRST, fc.SECOND_TRIP_NODE]]       # the tie across two trips; a query equal to a child of the second trip
    V = matcher.Vocabulary(ctx, vocab)
    for levelsup in (0, L - 1, L, L + 2):
        leaf, enode = fr.bow_descend(vocab, desc, levelsup)
        oword, ow, onode, _, _ = oracle_lib.bow_transform(vocab, desc, levelsup)
        for N in (1, 2, 3, 4, 5, 1023):
            word, w, node, *_ = V.transform(desc[:N], levelsup)
            assert np.array_equal(word, vocab["word_id"][leaf[:N]]) and np.array_equal(w, vocab["weight"][leaf[:N]]) and np.array_equal(node, enode[:N])
            assert np.array_equal(word, oword[:N]) and np.array_equal(w, ow[:N]) and np.array_equal(node, onode[:N])
        if tree == "wide" and levelsup == L - 1:
            assert node[:2].tolist() == [fc.TIE_FIRST, fc.SECOND_TRIP_NODE]      # child 3 wins over child 70
    V.close()
