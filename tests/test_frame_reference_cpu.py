"""CPU: tests/frame_reference.py, the NumPy restatement that tests/test_frame_edges_gpu.py holds the per-frame kernels to, is itself held to the oracle on every
case of tests/frame_edge_cases.py that lies in the source's defined domain (finite input, r >= 0), and the cases are held to what they claim: ties are ties, the
16- and 17-cell windows have 16 and 17 cells, the frustum table's rows stand on their equalities, the planted pairs are adjacent floats that straddle one
comparison.  The last test compiles csrc/frame_math.h for the host, as the host mirror does, under the undefined-behaviour sanitizer and compares its cell,
cell-range and frustum functions with the reference and the oracle, the inputs outside the defined domain included."""
import os
import subprocess

import numpy as np
import pytest

import frame_edge_cases as fc
import frame_reference as fr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _grid_both(oracle_lib, kps):
    off, idx = fr.build_grid(fc.BOUNDS, kps["x"], kps["y"])
    off_o, idx_o = oracle_lib.build_grid(kps["x"], kps["y"], fc.BOUNDS)
    assert np.array_equal(off, off_o) and np.array_equal(idx, idx_o)
    return off, idx


def test_grid_reference_matches_the_oracle_on_every_grid_case(oracle_lib):
    for n in fc.GRID_SIZES:
        kps, _ = fc.grid_size_kps(n)
        off, _ = _grid_both(oracle_lib, kps)
        assert off[-1] < n if n >= 1000 else off[-1] == n            # the margin drops some; the single one and the last five are all placed
    (kps, _), cells = fc.crowded_case()
    off, idx = _grid_both(oracle_lib, kps)
    assert np.array_equal(fr.cell_of(fc.BOUNDS, kps["x"], kps["y"]), cells)
    for c in (0, 37 * 48 + 23, 74 * 48 + 47):
        lst = idx[off[c]:off[c + 1]]
        assert lst.size == 500 and (np.diff(lst) > 0).all()
    kps, _ = fc.rim_case()
    off, _ = _grid_both(oracle_lib, kps)
    c = fr.cell_of(fc.BOUNDS, kps["x"], kps["y"])
    assert 0 < off[-1] < len(kps) and len(kps) - off[-1] == (c < 0).sum()
    # x == maxX and its lower neighbour round to column 75: outside; x == 0 and -0 are column 0
    assert (c[kps["x"] >= np.nextafter(fc.F(fc.W), fc.F(0))] == -1).all() and (c[(kps["x"] == 0) & (kps["y"] == 5.0)] == 1).all()
    kps, _ = fc.rim_case(wild=True)
    c = fr.cell_of(fc.BOUNDS, kps["x"], kps["y"])
    assert (c[~np.isfinite(kps["x"]) | ~np.isfinite(kps["y"]) | (np.abs(kps["x"]) > 1e30) | (np.abs(kps["y"]) > 1e30)] == -1).all()


def test_half_cell_ties_exist_and_round_away_from_zero(oracle_lib):
    (kps, _), exp, tx, ty = fc.tie_case()
    wInv, hInv = fr.grid_inverses(fc.BOUNDS)
    for ties, inv, need in ((tx, wInv, 20), (ty, hInv, 10)):
        assert all(fc.F(c * inv) == fc.F(k + 0.5) for k, c in ties)
        even, odd = sum(1 for k, _ in ties if k % 2 == 0), sum(1 for k, _ in ties if k % 2 == 1)
        assert even >= need and odd >= need, (even, odd)              # rint() would send the even ones down
    assert np.array_equal(fr.cell_of(fc.BOUNDS, kps["x"], kps["y"]), exp)
    _grid_both(oracle_lib, kps)


def _windows_both(oracle_lib, kps, q):
    off, idx = fr.window_candidates(fc.BOUNDS, kps["x"], kps["y"], kps["octave"], q["u"], q["v"], q["r"], q["minl"], q["maxl"])
    off_o, idx_o = oracle_lib.grid_candidates(kps["x"], kps["y"], kps["octave"], fc.BOUNDS, q["u"], q["v"], q["r"], q["minl"], q["maxl"])
    assert np.array_equal(off, off_o) and np.array_equal(idx, idx_o)
    return off, idx


def test_window_reference_matches_the_oracle_and_the_shapes_are_what_they_claim(oracle_lib):
    kps, _, q = fc.query_count_case()
    off, idx = _windows_both(oracle_lib, kps, q)
    assert idx.size > 20000 and (np.diff(off) == 0).sum() > 100
    for Q in fc.QUERY_COUNTS:                                          # a prefix of the queries has the prefix of the lists
        o, i = fr.window_candidates(fc.BOUNDS, kps["x"], kps["y"], kps["octave"], *(q[k][:Q] for k in ("u", "v", "r", "minl", "maxl")))
        assert np.array_equal(o, off[:Q + 1]) and np.array_equal(i, idx[:off[Q]])

    kps, _, q, row = fc.window_shape_case()
    off, idx = _windows_both(oracle_lib, kps, q)
    lst = lambda name: idx[off[row[name]]:off[row[name] + 1]]
    cells = lambda name: (lambda g: (g[1] - g[0] + 1) * (g[3] - g[2] + 1))(fr.cell_range(fc.BOUNDS, q["u"][row[name]], q["v"][row[name]], q["r"][row[name]]))
    assert kps["x"][fc.A_IDX] == q["u"][row["r0_on_keypoint"]] and kps["y"][fc.A_IDX] == q["v"][row["r0_on_keypoint"]] and lst("r0_on_keypoint").size == 0
    i = row["dx_equals_r"]
    assert np.abs(kps["x"][fc.B_IDX] - q["u"][i]) == q["r"][i] and kps["y"][fc.B_IDX] == q["v"][i]
    assert fc.B_IDX not in lst("dx_equals_r") and fc.B_IDX in lst("dx_below_next_r") and q["r"][i + 1] == np.nextafter(q["r"][i], fc.INF)
    assert cells("cells_16") == 16 and cells("cells_17") == 17 and cells("whole_grid") == fr.N_CELLS
    assert lst("cells_16")[-1] == fc.C_IDX and lst("cells_17")[-1] == fc.D_IDX                    # a candidate in the 16th and in the 17th cell (the second trip)
    assert np.array_equal(lst("whole_grid"), fr.build_grid(fc.BOUNDS, kps["x"], kps["y"])[1])
    for name in ("left_of", "right_of", "above", "below"):
        assert fr.cell_range(fc.BOUNDS, q["u"][row[name]], q["v"][row[name]], q["r"][row[name]]) is None
    for name in ("cells_16", "cells_17", "corner_00", "corner_w0", "corner_0h", "corner_wh", "straddle_left", "straddle_right", "straddle_top", "straddle_bottom"):
        assert lst(name).size > 0, name

    kps, _, q = fc.level_case()
    off, idx = _windows_both(oracle_lib, kps, q)
    lists = [idx[off[i]:off[i + 1]] for i in range(len(fc.LEVEL_PAIRS))]
    assert np.array_equal(lists[0], lists[1]) and lists[5].size == 0 and lists[0].size > 50
    assert 0 < lists[2].size < lists[3].size < lists[0].size and 0 < lists[6].size and 0 < lists[4].size

    kps, _, q, ordinary = fc.total_range_case()
    _windows_both(oracle_lib, kps, fc.take(q, ordinary))                # the oracle sees the defined domain only
    off, idx = fr.window_candidates(fc.BOUNDS, kps["x"], kps["y"], kps["octave"], q["u"], q["v"], q["r"], q["minl"], q["maxl"])
    whole = fr.build_grid(fc.BOUNDS, kps["x"], kps["y"])[1]
    seen = set()
    for i in np.nonzero(~ordinary)[0]:
        u, v, r = q["u"][i], q["v"][i], q["r"][i]
        empty = np.isnan(u) or np.isnan(v) or np.isnan(r) or r < 0 or np.isinf(u) or np.isinf(v)
        assert (off[i + 1] - off[i] == 0) if empty else np.array_equal(idx[off[i]:off[i + 1]], whole), (u, v, r)
        seen.add((str(u), str(v), str(r)))
    assert len(seen) == 16 and (np.diff(off)[ordinary] > 0).all()


def test_bow_reference_matches_the_oracle_on_the_hand_built_trees(oracle_lib):
    from ccm_slam_amd import synth
    wide, depth_w = fc.wide_vocabulary()
    ragged, depth_r = fc.ragged_vocabulary()
    fan = set(np.diff(wide["child_off"]).tolist()) | set(np.diff(ragged["child_off"]).tolist())
    assert {1, 2, 63, 64, 65, 130} <= fan and wide["L"] == 3 and ragged["L"] == 5
    for vocab in (wide, ragged, synth.make_vocabulary(7, 3, seed=3)):
        L = vocab["L"]
        desc = fc.bow_queries(vocab, 1023, 70 + L)
        for levelsup in (0, L - 1, L, L + 2):
            leaf, node = fr.bow_descend(vocab, desc, levelsup)
            word, w, onode, _, _ = oracle_lib.bow_transform(vocab, desc, levelsup)
            assert np.array_equal(vocab["word_id"][leaf], word) and np.array_equal(vocab["weight"][leaf], w) and np.array_equal(node, onode)
            assert (node == 0).all() if levelsup >= L else (node > 0).any()
        assert len(np.unique(leaf)) > 20
    # the tie: the root's children 3 and 70 are both at distance 0; the first wins.  A query equal to a child of the second trip reaches it.
    d = wide["node_desc"]
    assert np.array_equal(d[fc.TIE_FIRST], d[fc.TIE_SECOND]) and wide["child_id"][3] == fc.TIE_FIRST and wide["child_id"][70] == fc.TIE_SECOND
    _, node = fr.bow_descend(wide, d[[fc.TIE_FIRST, fc.SECOND_TRIP_NODE]], wide["L"] - 1)
    assert node.tolist() == [fc.TIE_FIRST, fc.SECOND_TRIP_NODE] and 64 <= wide["child_id"].tolist().index(fc.SECOND_TRIP_NODE) < 128


def test_frustum_table_stands_on_its_equalities_and_the_planting_succeeds(oracle_lib):
    rows = fc.frustum_table()
    fc.check_frustum_table(rows)
    P, Pn, dmin, dmax = fc.table_arrays(rows)
    inv, u, v, lvl, cs = oracle_lib.is_in_frustum(fc.TABLE_FRAME, fc.N_LEVELS, P, Pn, dmin, dmax, 0.5)
    for i, r in enumerate(rows):
        assert inv[i] == r[5], r[0]
        assert r[6] is None or lvl[i] == r[6], (r[0], lvl[i])
    planted = {}
    for test in fc.PLANT_TESTS:
        (P, Pn, dmin, dmax), near = fc.plant_adjacent(oracle_lib.is_in_frustum, test)
        n = fc.N_PLANT
        moved = [a for a in (P[:, 0], P[:, 1], P[:, 2], Pn[:, 0], dmin, dmax) if not np.array_equal(a[:n], a[n:])]
        assert len(moved) == 1                                                                       # ONE input differs between the two sides ...
        assert (np.abs(fc._ordered(moved[0][:n]) - fc._ordered(moved[0][n:])) == 1).all()            # ... by one float
        planted[test] = int(near.sum())
    assert all(c >= 58 for c in planted.values()), planted


def _same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def test_frame_math_compiled_for_the_host_equals_the_reference_on_every_input(oracle_lib, tmp_path):
    exe = tmp_path / "frame_math_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "frame_math_check.cpp")], check=True)

    def run(mode, head, body):
        fin, fout = tmp_path / (mode + ".in"), tmp_path / (mode + ".out")
        np.concatenate([np.asarray(head, np.float32).ravel(), np.asarray(body, np.float32).ravel()]).tofile(fin)
        r = subprocess.run([str(exe), mode, str(fin), str(fout)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        return np.fromfile(fout, np.int32)
    bounds6 = [*fc.BOUNDS, *fr.grid_inverses(fc.BOUNDS)]
    # cells: every grid case, the wild rim included
    sets = [fc.uniform_kps(3100, 4100)[0], fc.crowded_case()[0][0], fc.rim_case(wild=True)[0], fc.tie_case()[0][0]]
    x = np.concatenate([k["x"] for k in sets]); y = np.concatenate([k["y"] for k in sets])
    assert np.array_equal(run("cell", bounds6, np.stack([x, y], 1)), fr.cell_of(fc.BOUNDS, x, y))
    # cell ranges: every query of every window case, and every pairing of special values
    qs = [fc.query_count_case()[2], fc.window_shape_case()[2], fc.total_range_case()[2]]
    sp = np.array([np.nan, np.inf, -np.inf, -100.0, -1.0, -0.0, 0.0, 25.0, 240.0, 800.0, 1e12, 3e38], np.float32)
    g = np.stack(np.meshgrid(sp, sp, sp, indexing="ij"), -1).reshape(-1, 3)
    uvr = np.concatenate([np.stack([q["u"], q["v"], q["r"]], 1) for q in qs] + [g])
    got = run("range", bounds6, uvr).reshape(-1, 5)
    for (u, v, r), row in zip(uvr, got):
        exp = fr.cell_range(fc.BOUNDS, u, v, r)
        assert (row[0] == 0) if exp is None else (row.tolist() == [1, *exp]), (u, v, r, row, exp)
    # frustum: the table, the planted pairs and random points, bit for bit with the oracle (a NaN equals a NaN)
    def frustum(frame, P, Pn, dmin, dmax):
        got = run("frustum", np.concatenate([frame, [fc.N_LEVELS, 0.5]]), np.concatenate([P, Pn, dmin[:, None], dmax[:, None]], 1)).reshape(-1, 5)
        exp = oracle_lib.is_in_frustum(frame, fc.N_LEVELS, P, Pn, dmin, dmax, 0.5)
        assert np.array_equal(got[:, 0], exp[0]) and np.array_equal(got[:, 3], exp[3])
        for col, e in ((1, exp[1]), (2, exp[2]), (4, exp[4])):
            assert _same_f32(got[:, col].copy().view(np.float32), e)
    frustum(fc.TABLE_FRAME, *fc.table_arrays(fc.frustum_table()))
    for test in fc.PLANT_TESTS:
        frustum(fc.PLANT_FRAME, *fc.plant_adjacent(oracle_lib.is_in_frustum, test)[0])
    frustum(*fc.frustum_random_case(2000, 5))
