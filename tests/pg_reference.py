"""Plain-numpy reference of the pose graph's two PCG solve paths (posegraph.hip): the spanning forest, its matrix T and an exact solve with T,
the block-Jacobi preconditioner, the block mat-vec and a PCG with the kernels' stop rules.  The forest and preconditioner functions take `dtype`
(np.float64 or np.longdouble); the distance between the two runs is the yardstick for the device (tests/test_posegraph_pcg_gpu.py).

Conventions: free vertices get slots 0 .. F-1 in vertex order; J[e, side, k, d] = d err_k / d update_d of edge e (indexed like pg["e_i"]), side 0 = the
vertex e_i, side 1 = e_j, zero for a fixed side; H either dense [7F, 7F] or only its diagonal blocks [F, 7, 7]."""
import numpy as np


def slots(pg):
    fixed = np.asarray(pg["fixed"]) != 0
    slot = -np.ones(fixed.size, np.int64)
    slot[~fixed] = np.arange(int((~fixed).sum()))
    return slot


def active_edges(pg):
    fixed = np.asarray(pg["fixed"]) != 0
    return np.flatnonzero(~(fixed[pg["e_i"]] & fixed[pg["e_j"]]))


def forest(pg):
    """Kruskal over the active edges, stable by |e_i - e_j|, all fixed vertices contracted into one root.
    Returns (tree, roots): tree = sorted edge indices of the forest, roots = the lowest free slot of every component without a fixed vertex."""
    slot = slots(pg)
    F = int((slot >= 0).sum())
    act = active_edges(pg)
    ei, ej = np.asarray(pg["e_i"], np.int64), np.asarray(pg["e_j"], np.int64)
    order = act[np.argsort(np.abs(ei[act] - ej[act]), kind="stable")]
    uf = list(range(F + 1))

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x
    tree = []
    for e in order:
        a = slot[ei[e]] if slot[ei[e]] >= 0 else F
        b = slot[ej[e]] if slot[ej[e]] >= 0 else F
        ra, rb = find(a), find(b)
        if ra != rb:
            uf[ra] = rb
            tree.append(int(e))
    anchored = find(F)
    seen, roots = set(), []
    for a in range(F):
        c = find(a)
        if c != anchored and c not in seen:
            seen.add(c)
            roots.append(a)
    return sorted(tree), roots


def _diag_block(H, a):
    H = np.asarray(H)
    return H[7 * a:7 * a + 7, 7 * a:7 * a + 7] if H.ndim == 2 else H[a]


def _tree_jacobians(pg, J, e, dtype):
    """(Ji, Jj) of a forest edge as the preconditioner sees them: with fix_scale the scale row and column are replaced by the unit entries +1 / -1."""
    Ji, Jj = np.array(J[e, 0], dtype), np.array(J[e, 1], dtype)
    if pg["fix_scale"]:
        for M, v in ((Ji, 1.0), (Jj, -1.0)):
            M[6, :] = 0
            M[:, 6] = 0
            M[6, 6] = v
    return Ji, Jj


def forest_matrix(pg, H, J, lam, dtype=np.float64):
    """Dense T = sum over forest edges of [Ji Jj]^T [Ji Jj] restricted to the free vertices, plus H_aa + (lam + 1e-12) I on the diagonal block of every
    floating root.  For small F."""
    slot = slots(pg)
    F = int((slot >= 0).sum())
    tree, roots = forest(pg)
    T = np.zeros((7 * F, 7 * F), dtype)
    for e in tree:
        Jm = _tree_jacobians(pg, J, e, dtype)
        s = (slot[pg["e_i"][e]], slot[pg["e_j"][e]])
        for x in range(2):
            for y in range(2):
                if s[x] >= 0 and s[y] >= 0:
                    T[7 * s[x]:7 * s[x] + 7, 7 * s[y]:7 * s[y] + 7] += Jm[x].T @ Jm[y]
    for a in roots:
        T[7 * a:7 * a + 7, 7 * a:7 * a + 7] += np.array(_diag_block(H, a), dtype) + dtype(lam + 1e-12) * np.eye(7, dtype=dtype)
    return T


def inv_batch(A, dtype=np.float64):
    """Inverses of a stack of small matrices [n, m, m] by Gauss-Jordan with partial pivoting in `dtype` (numpy.linalg has no long double)."""
    A = np.array(A, dtype)
    n, m, _ = A.shape
    W = np.concatenate([A, np.broadcast_to(np.eye(m, dtype=dtype), (n, m, m))], axis=2)
    idx = np.arange(n)
    for c in range(m):
        piv = c + np.argmax(np.abs(W[:, c:, c]), axis=1)
        rows_c, rows_p = W[idx, c].copy(), W[idx, piv].copy()
        W[idx, c], W[idx, piv] = rows_p, rows_c
        W[:, c] /= W[:, c, c][:, None]
        f = W[:, :, c].copy()
        f[:, c] = 0
        W -= f[:, :, None] * W[:, c][:, None, :]
    return W[:, :, m:]


def forest_solve(pg, H, J, lam, dtype=np.longdouble):
    """Exact solve with T by block elimination on the forest: Schur complements from the leaves to the roots, substitution back.  O(F).
    Returns apply(r) -> T^-1 r for r of shape [7F] or [7F, m]."""
    slot = slots(pg)
    F = int((slot >= 0).sum())
    tree, roots = forest(pg)
    ei, ej = np.asarray(pg["e_i"]), np.asarray(pg["e_j"])
    D = np.zeros((F, 7, 7), dtype)          # diagonal blocks of T
    adj = [[] for _ in range(F)]            # (neighbour, T_{self, neighbour})
    start = list(roots)
    for e in tree:
        Ji, Jj = _tree_jacobians(pg, J, e, dtype)
        a, b = slot[ei[e]], slot[ej[e]]
        if a >= 0:
            D[a] += Ji.T @ Ji
        if b >= 0:
            D[b] += Jj.T @ Jj
        if a >= 0 and b >= 0:
            adj[a].append((b, Ji.T @ Jj))
            adj[b].append((a, Jj.T @ Ji))
        else:
            start.append(int(a if a >= 0 else b))   # hangs off a fixed vertex: a root of the eliminated forest
    for a in roots:
        D[a] += np.array(_diag_block(H, a), dtype) + dtype(lam + 1e-12) * np.eye(7, dtype=dtype)
    # any parents-first order from the roots
    parent = -np.ones(F, np.int64)
    Tkp = np.zeros((F, 7, 7), dtype)        # T_{k, parent(k)}
    order, seen = [], np.zeros(F, bool)
    for r0 in start:
        seen[r0] = True
        stack = [r0]
        while stack:
            u = stack.pop()
            order.append(u)
            for v, Tuv in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    parent[v] = u
                    Tkp[v] = Tuv.T
                    stack.append(v)
    assert len(order) == F and seen.all()
    S = D                                    # becomes the Schur complements
    Sinv = np.zeros_like(S)
    U = np.zeros_like(S)                     # U_k = T_{parent, k} S_k^-1
    for k in reversed(order):
        Sinv[k] = inv_batch(S[k][None], dtype)[0]
        p = parent[k]
        if p >= 0:
            U[k] = Tkp[k].T @ Sinv[k]
            S[p] -= U[k] @ Tkp[k]

    def apply(r):
        g = np.array(r, dtype).reshape(F, 7, -1).copy()
        for k in reversed(order):
            if parent[k] >= 0:
                g[parent[k]] -= U[k] @ g[k]
        z = np.zeros_like(g)
        for k in order:
            z[k] = Sinv[k] @ g[k]
            if parent[k] >= 0:
                z[k] -= U[k].T @ z[parent[k]]
        return z.reshape(np.shape(r))
    return apply


def block_jacobi(H, lam, dtype=np.float64):
    """apply(r) -> blockdiag(H_aa + lam I)^-1 r"""
    H = np.asarray(H)
    F = H.shape[0] // 7 if H.ndim == 2 else H.shape[0]
    B = np.stack([np.array(_diag_block(H, a), dtype) for a in range(F)]) + dtype(lam) * np.eye(7, dtype=dtype)
    Binv = inv_batch(B, dtype)

    def apply(r):
        return np.einsum("aij,aj->ai", Binv, np.array(r, dtype).reshape(F, 7)).reshape(np.shape(r))
    return apply


def matvec(blocks, keys, lam, x):
    """(H + lam I) x from the upper-triangle blocks[k] = H[a, b], keys[k] = (a, b), a <= b; in the dtype of x"""
    dtype = x.dtype.type
    B = np.asarray(blocks, dtype)
    a, b = np.asarray(keys)[:, 0], np.asarray(keys)[:, 1]
    X = x.reshape(-1, 7)
    Y = dtype(lam) * X
    np.add.at(Y, a, np.einsum("kij,kj->ki", B, X[b]))
    off = a != b
    np.add.at(Y, b[off], np.einsum("kji,kj->ki", B[off], X[a[off]]))
    return Y.ravel()


def blocks_of_dense(H):
    """(blocks, keys) of the non-zero upper-triangle 7x7 blocks of a dense H"""
    F = H.shape[0] // 7
    blocks, keys = [], []
    for a in range(F):
        for b in range(a, F):
            Bk = H[7 * a:7 * a + 7, 7 * b:7 * b + 7]
            if a == b or np.any(Bk != 0):
                blocks.append(Bk)
                keys.append((a, b))
    return np.stack(blocks), np.array(keys)


def pcg(Av, b, M, rel_tol, max_it, stall):
    """Preconditioned CG with the stop rules of the kernels: before iteration k it ends when r.z <= rel_tol^2 r0.z0 or !(r.z > 0); a step with
    !(p.q > 0) ends it as a failure; with `stall` it ends after an iteration when r.z has not improved by 10 % for more than 40 iterations.
    Runs in the precision of b (float64 like the device, unless b is long double).
    Returns (x, iterations, flags) with flags = [done, iterations, fail, stalled] as the device reports them."""
    b = np.array(b)
    dtype = b.dtype.type
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = np.zeros_like(b)
    rz = r @ z
    rz0, rz_prev = rz, rz
    best, best_k = rz, 0
    tol2 = dtype(rel_tol) * dtype(rel_tol)
    k = 0
    done = fail = stalled = 0
    while k < max_it:
        if rz <= tol2 * rz0 or not (rz > 0):
            done = 1
            fail = int(rz != rz)
            break
        beta = dtype(0) if k == 0 else rz / rz_prev
        p = z + beta * p
        q = Av(p)
        pq = p @ q
        if not (pq > 0):
            done = fail = 1
            break
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = M(r)
        rz_prev, rz = rz, r @ z
        k += 1
        if stall:
            if rz < dtype(0.9) * best:
                best, best_k = rz, k
            elif k - best_k > 40:
                done = stalled = 1
                break
    return x, k, np.array([done, k, fail, stalled])
