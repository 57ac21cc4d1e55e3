"""A plain NumPy restatement of the per-frame glue, written from the definitions the kernels cite and from nothing of this project's C++:
Frame::AssignFeaturesToGrid / PosInGrid (cslam/src/Frame.cpp:103-118, 254-265), Frame::GetFeaturesInArea (:200-253) and
TemplatedVocabulary::transform (DBoW2/TemplatedVocabulary.h:1218-1260).  Everything is integer work or f32 arithmetic done by NumPy on float32 arrays,
one rounding per operation, so device results are compared with it for equality.

bounds is (mnMinX, mnMinY, mnMaxX, mnMaxY); the grid has 75 x 48 cells, cell = ix * 48 + iy (mGrid[x][y]: x-major)."""
import numpy as np

GRID_COLS, GRID_ROWS = 75, 48
N_CELLS = GRID_COLS * GRID_ROWS
_F = np.float32


def grid_inverses(bounds):
    """mfGridElementWidthInv / HeightInv (Frame.cpp:87-88): f32 quotients of f32 values"""
    minX, minY, maxX, maxY = (_F(b) for b in bounds)
    return _F(GRID_COLS) / _F(maxX - minX), _F(GRID_ROWS) / _F(maxY - minY)


def _round_half_away(t32):
    """round() of an f32 value, in f64: floor(|t| + 0.5) with the sign restored.  |t| + 0.5 is exact in f64 for every f32 t below 2^28 (the same sum in f32 is
    rounded: 0.5 - 2^-25 would round up to 1)."""
    t = np.asarray(t32, np.float32).astype(np.float64)
    return np.copysign(np.floor(np.abs(t) + 0.5), t)


def cell_of(bounds, x, y):
    """PosInGrid for arrays of keypoint positions: the cell ix * 48 + iy, or -1 outside the grid"""
    minX, minY = _F(bounds[0]), _F(bounds[1])
    wInv, hInv = grid_inverses(bounds)
    x, y = np.atleast_1d(np.asarray(x, np.float32)), np.atleast_1d(np.asarray(y, np.float32))
    with np.errstate(all="ignore"):
        px = _round_half_away((x - minX) * wInv)
        py = _round_half_away((y - minY) * hInv)
        ok = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)      # a NaN is in no cell
        return np.where(ok, px * GRID_ROWS + py, -1.0).astype(np.int64)


def build_grid(bounds, x, y):
    """AssignFeaturesToGrid: (cell_off[3601], cell_idx); the features of a cell in push_back order, which is ascending index"""
    c = cell_of(bounds, x, y)
    keep = np.nonzero(c >= 0)[0]
    order = keep[np.argsort(c[keep], kind="stable")]
    cell_off = np.zeros(N_CELLS + 1, np.int32)
    cell_off[1:] = np.cumsum(np.bincount(c[keep], minlength=N_CELLS))
    return cell_off, order.astype(np.int32)


def cell_range(bounds, u, v, r):
    """The cell range of GetFeaturesInArea as (x0, x1, y0, y1), or None for a window without cells.  Total: None for a NaN among u, v, r and for r < 0, and also
    for a window edge that is itself NaN (inf - inf; with u, v, r free of NaN there is no other way to one).  Otherwise the four f32 products are clamped to
    [-1, 76] before the conversion to an integer: both ends lie outside the grid on both axes, so the range of every window whose products an int holds is the
    source's own."""
    u, v, r = _F(u), _F(v), _F(r)
    if np.isnan(u) or np.isnan(v) or np.isnan(r) or r < 0:
        return None
    minX, minY = _F(bounds[0]), _F(bounds[1])
    wInv, hInv = grid_inverses(bounds)
    with np.errstate(all="ignore"):
        t = [_F(_F(_F(u - minX) - r) * wInv), _F(_F(_F(u - minX) + r) * wInv), _F(_F(_F(v - minY) - r) * hInv), _F(_F(_F(v - minY) + r) * hInv)]
    if any(np.isnan(a) for a in t):
        return None
    t = [float(min(max(a, _F(-1)), _F(76))) for a in t]
    x0 = max(0, int(np.floor(t[0])))
    if x0 >= GRID_COLS:
        return None
    x1 = min(GRID_COLS - 1, int(np.ceil(t[1])))
    if x1 < 0:
        return None
    y0 = max(0, int(np.floor(t[2])))
    if y0 >= GRID_ROWS:
        return None
    y1 = min(GRID_ROWS - 1, int(np.ceil(t[3])))
    if y1 < 0:
        return None
    return x0, x1, y0, y1


def window_candidates(bounds, kx, ky, octave, u, v, r, min_level, max_level, grid=None):
    """GetFeaturesInArea for a batch of queries: (off[Q + 1], idx) with every list in the source's order: ix ascending, then iy, then the cell's own order.
    Level rule: bCheckLevels = minLevel > 0 or maxLevel >= 0; then octave < minLevel is skipped, and octave > maxLevel where maxLevel >= 0.
    Distance rule: |kx - u| < r and |ky - v| < r, strict, on f32 differences."""
    kx, ky = np.asarray(kx, np.float32), np.asarray(ky, np.float32)
    octave = np.asarray(octave, np.int64)
    u, v, r = (np.atleast_1d(np.asarray(a, np.float32)) for a in (u, v, r))
    min_level, max_level = np.atleast_1d(np.asarray(min_level, np.int64)), np.atleast_1d(np.asarray(max_level, np.int64))
    cell_off, cell_idx = grid if grid is not None else build_grid(bounds, kx, ky)
    off, out = [0], []
    for q in range(u.size):
        rng = cell_range(bounds, u[q], v[q], r[q])
        n = 0
        if rng is not None:
            x0, x1, y0, y1 = rng
            # the cells (ix, y0 .. y1) are neighbours in cell_off: one slice per column holds them in iy order
            k = np.concatenate([cell_idx[cell_off[ix * GRID_ROWS + y0]:cell_off[ix * GRID_ROWS + y1 + 1]] for ix in range(x0, x1 + 1)])
            keep = np.ones(k.size, bool)
            if min_level[q] > 0 or max_level[q] >= 0:
                keep &= octave[k] >= min_level[q]
                if max_level[q] >= 0:
                    keep &= octave[k] <= max_level[q]
            with np.errstate(all="ignore"):
                keep &= (np.abs(kx[k] - u[q]) < r[q]) & (np.abs(ky[k] - v[q]) < r[q])
            k = k[keep]
            out.append(k)
            n = k.size
        off.append(off[-1] + n)
    idx = np.concatenate(out).astype(np.int32) if out else np.zeros(0, np.int32)
    return np.array(off, np.int32), idx


_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b):
    """FORB::distance / ORBmatcher::DescriptorDistance: differing bits of 32-byte descriptors; a: (32,) or (n, 32), b: (n, 32)"""
    return _POPCOUNT[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum(axis=-1)


def bow_descend(vocab, desc, levelsup):
    """TemplatedVocabulary::transform's descent for every descriptor: (leaf node, node at level L - levelsup; 0 when that level is <= 0 or is never reached).
    At every node the child with the least distance wins, the first one in child order among equals (np.argmin returns the first minimum)."""
    child_off, child_id, node_desc = vocab["child_off"], vocab["child_id"], vocab["node_desc"]
    nid_level = int(vocab["L"]) - int(levelsup)
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    leaf, node = np.zeros(desc.shape[0], np.int32), np.zeros(desc.shape[0], np.int32)
    for f in range(desc.shape[0]):
        cur, level, nid = 0, 0, 0
        while child_off[cur + 1] > child_off[cur]:
            level += 1
            ch = child_id[child_off[cur]:child_off[cur + 1]]
            cur = int(ch[np.argmin(hamming(desc[f], node_desc[ch]))])
            if level == nid_level:
                nid = cur
        leaf[f], node[f] = cur, nid
    return leaf, node
