"""The launch list of the dense inverse's fused chain (ccm_dense_chol_inverse_dev in dense_chol.hip), restated at tile level in numpy: every launch is a list of
workgroups, every workgroup names the tiles it reads and the tiles it writes.  Launches are stream-ordered and no workgroup waits on another inside a launch, so
  * no workgroup may read or write a tile that ANOTHER workgroup of the same launch writes,
  * an operand that must be final (everything except a workgroup's own running sum) must have had its last write in an EARLIER launch,
and the tiles that come out must be the inverse.  Storage: A[r][c] (lower triangle: the matrix, then L_jj on the diagonal; upper slot (j, i): L_ij for the L^-1
steps), Li[j] (inverse of L_jj, d_linv), X[i][j] (L^-1 below the diagonal; its diagonal tiles are Li), Ainv.  A "workgroup" here is everything that works on one
output tile: the kernels split it further (four quadrants of an update tile, four column strips of an L^-1 or X^T X tile), each part with the tile's reads and a
disjoint part of its writes."""
import numpy as np
import pytest

B = 8   # tile edge of the restatement (the kernels use 64; the launch list does not depend on it)


def launch_list(T):
    """[(name, [workgroup, ...])], workgroup = dict(kind=..., reads=[final operands], rmw=[own running sums], writes=[...], args)"""
    def diag(j):
        return ("diag%d" % j, [dict(kind="diag", j=j, reads=[], rmw=[("A", j, j)], writes=[("A", j, j), ("Li", j)])])

    def tri_wgs(k):   # L^-1 step k: X_ij += L_ik X_kj for i > k >= j, rows i = k + 1 are finished with Li_ii
        wgs = []
        for i in range(k + 1, T):
            for j in range(k + 1):
                reads = [("A", k, i), ("Li", k) if j == k else ("X", k, j)]
                if i == k + 1: reads.append(("Li", i))
                wgs.append(dict(kind="tri", i=i, j=j, k=k, reads=reads, rmw=[] if j == k else [("X", i, j)], writes=[("X", i, j)]))
        return wgs

    out = [diag(0)]
    for j in range(T - 1):
        wgs = []
        for i in range(j + 1, T):
            for k in range(j + 1, i + 1):
                w = dict(kind="upd", i=i, k=k, j=j, reads=[("A", i, j), ("A", k, j), ("Li", j)], rmw=[("A", i, k)], writes=[("A", i, k)])
                if k == j + 1: w["writes"].append(("A", j, i))
                wgs.append(w)
        if j > 0: wgs += tri_wgs(j - 1)
        out.append(("step%d" % j, wgs))
        out.append(diag(j + 1))
    if T > 1: out.append(("tri%d" % (T - 2), tri_wgs(T - 2)))
    xtx = []
    for p in range(T):
        for q in range(p + 1):
            reads = []
            for k in range(p, T):
                reads += [("Li", k) if k == p else ("X", k, p), ("Li", k) if k == q else ("X", k, q)]
            xtx.append(dict(kind="xtx", p=p, q=q, reads=reads, rmw=[], writes=[("Ainv", p, q)] + ([("Ainv", q, p)] if p != q else [])))
    out.append(("xtx", xtx))
    return out


def run(T, M):
    """executes the list on the T x T tiles of M; returns (Ainv, violations)"""
    mem = {("A", r, c): M[B * r:B * r + B, B * c:B * c + B].copy() for r in range(T) for c in range(r + 1)}
    launches = launch_list(T)
    last_write = {}
    for li, (_, wgs) in enumerate(launches):
        for w in wgs:
            for t in w["writes"]: last_write[t] = li
    bad = []
    for li, (name, wgs) in enumerate(launches):
        written_by = {}
        for wi, w in enumerate(wgs):
            for t in w["writes"]:
                if t in written_by: bad.append((name, "two writers", t))
                written_by[t] = wi
        staged = []
        for wi, w in enumerate(wgs):
            for t in w["reads"] + w["rmw"]:
                if t not in mem: bad.append((name, "read before any write", t))
                if written_by.get(t, wi) != wi: bad.append((name, "reads a tile another workgroup of the launch writes", t))
            for t in w["reads"]:
                if last_write.get(t, -1) >= li: bad.append((name, "operand not final", t))
            g = lambda t: mem[t]
            if w["kind"] == "diag":
                L = np.linalg.cholesky(g(("A", w["j"], w["j"])))
                staged += [(("A", w["j"], w["j"]), L), (("Li", w["j"]), np.linalg.inv(L))]
            elif w["kind"] == "upd":
                i, k, j = w["i"], w["k"], w["j"]
                Lij, Lkj = g(("A", i, j)) @ g(("Li", j)).T, g(("A", k, j)) @ g(("Li", j)).T
                staged.append((("A", i, k), g(("A", i, k)) - Lij @ Lkj.T))
                if k == j + 1: staged.append((("A", j, i), Lij))
            elif w["kind"] == "tri":
                i, j, k = w["i"], w["j"], w["k"]
                s = g(("A", k, i)) @ (g(("Li", k)) if j == k else g(("X", k, j)))
                if j != k: s = g(("X", i, j)) + s
                staged.append((("X", i, j), -g(("Li", i)) @ s if i == k + 1 else s))
            else:
                p, q = w["p"], w["q"]
                s = sum((g(("Li", k)) if k == p else g(("X", k, p))).T @ (g(("Li", k)) if k == q else g(("X", k, q))) for k in range(p, T))
                staged.append((("Ainv", p, q), s))
                if p != q: staged.append((("Ainv", q, p), s.T))
        for t, v in staged: mem[t] = v     # a launch's writes land after all of its reads: the checks above make the order inside a launch irrelevant
    Ainv = np.block([[mem[("Ainv", p, q)] for q in range(T)] for p in range(T)])
    return Ainv, bad


@pytest.mark.parametrize("T", [1, 2, 3, 4, 12])
def test_fused_chain_launch_list(T):
    rng = np.random.default_rng(T)
    n = B * T
    G = rng.normal(size=(n, n))
    M = G @ G.T + n * np.eye(n)
    Ainv, bad = run(T, M)
    assert not bad, bad[:5]
    assert np.abs(Ainv - np.linalg.inv(M)).max() <= 1e-10
    # the chain: T diagonal tiles, T - 1 step launches, one L^-1 launch after the last diagonal tile, X^T X
    assert len(launch_list(T)) == T + (T - 1) + (1 if T > 1 else 0) + 1
    steps = [w for name, w in launch_list(T) if name.startswith("step")]
    for j, w in enumerate(steps):   # the grid the host code launches: (T - j - 1)(T - j) / 2 update pairs (x 4 quadrants) + (T - j) j products of L^-1 step j - 1 (x 4 strips)
        assert sum(x["kind"] == "upd" for x in w) == (T - j - 1) * (T - j) // 2 and sum(x["kind"] == "tri" for x in w) == (T - j) * j
    if T == 12:   # the flagship: at most 66 pairs and at most 36 products in a launch
        assert max(sum(x["kind"] == "upd" for x in w) for w in steps) == 66 and max(sum(x["kind"] == "tri" for x in w) for w in steps) == 36


def test_the_checks_see_an_in_place_panel():
    """the same list with L_ij stored over A_ij (what a fused launch must NOT do) is flagged: other pairs of the launch still read the raw A_ij"""
    T = 3
    launches = launch_list(T)
    name, wgs = launches[1]
    clash = [w for w in wgs if w["kind"] == "upd" and w["k"] == w["j"] + 1]
    readers = {t for w in wgs for t in w["reads"]}
    assert all(("A", w["i"], w["j"]) in readers for w in clash)          # the slot an in-place store would hit is an input of the launch
    assert all(("A", w["j"], w["i"]) not in readers for w in clash)      # the upper slot is not
