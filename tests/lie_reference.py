"""Running-error reference of the SE3 / Sim3 math every optimiser shares (ccm_slam_amd/csrc/ba_math.h, sim3_math.h).  Plain numpy; no GPU, no library call.

A TRACKED number (class T) holds a numpy.longdouble value and a first-order absolute bound on the error of a float64 evaluation of the same expression:

    +, -        e_a + e_b + u |z|                                         u = 2^-53 (charged as 2^-53 (1 + 2^-10): the long-double run's own rounding)
    *           |a| e_b + |b| e_a + e_a e_b + u |z|
    /           (e_a + |z| e_b) / (|b| - e_b) + u |z|                     (the divisor taken at its smallest magnitude)
    sqrt        the image of [a - e_a, a + e_a], + u |z|
    fma         |a| e_b + |b| e_a + e_a e_b + e_c + u |z|
    sin, cos    e_a min(1, |f'(a)| + e_a) + LIBM_ULP[f] 2^-52 |z|
    exp         z expm1(e_a) + LIBM_ULP 2^-52 |z|;     log, acos: the image of [a - e_a, a + e_a] + LIBM_ULP 2^-52 |z|

Exact inputs carry e = 0; adding an exact zero and multiplying by an exact power of two are exact (they are in binary arithmetic).  A comparison whose two
sides' bounds overlap raises Ambiguous with the case's name, unless the case carries that branch explicitly (`forced`); two exact sides compare exactly.

The formulas below are written from the two headers and the g2o / Eigen lines those cite, operation by operation in the header's order — g2o's
B = ((0.5 sigma^2 - sigma + 1) s) / sigma^3 included (sim3.h:116,199 lack a -1 there; parity with the reference is the contract, tests/test_ref_g2o.py pins
it, and log(exp(u)) is therefore off by O(1) in upsilon for 1e-5 <= theta < 4.47e-3 with |sigma| >= 1e-5: FACT1 below).  They take a context `c` and run
unchanged in two arithmetics: "tracked" (the truth and its bound) and "f64" (numpy float64: the restatement tests/test_lie_reference_cpu.py plants defects in).
Evaluation is vectorised over cases; a comparison that comes out differently within a batch splits the batch.

LIBM_ULP: one charge per libm function = max(1, 2 x the error measured on the MI355X over the case tables' own arguments, rounded up to an integer);
tests/test_lie_math_gpu.py measures and asserts measured <= charge / 2, tests/test_lie_math_cpu.py the same for glibc.  sqrt, division and fma are charged
0.5 ulp (u) as correctly rounded, and the raw-op tests assert 0 mismatches against the exactly rounded result.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

LD = np.longdouble
HAVE_EXTENDED = np.finfo(LD).nmant >= 63
U = LD(2.0) ** -53 * (1 + LD(2.0) ** -10)     # 2^-53 for the float64 rounding, and 2^-63 for the long-double evaluation's own (2^-64 per operation)
ULP = LD(2.0) ** -52
EPS = 0.00001
N_IN, N_OUT, FLAG = 48, 40, 39

# largest error measured on the MI355X, in ulp of the double result against long double, over raw_cases() (tests/test_lie_math_gpu.py prints them)
LIBM_MEASURED = {"sin": 0.677, "cos": 0.672, "sincos": 0.576, "exp": 0.680, "log": 0.574, "acos": 0.649}     # 2 x each, rounded up: 2
LIBM_ULP = {"sin": 2, "cos": 2, "sincos": 2, "exp": 2, "log": 2, "acos": 2}

_RECORD = None       # raw_cases() sets a dict here: the f64 arithmetic then records every argument it feeds a libm function


class Ambiguous(Exception):
    pass


class PlantedBranchWrong(Exception):
    pass


class _Split(Exception):
    def __init__(self, mask):
        self.mask = mask


def _pow2(v):
    m, _ = np.frexp(v)
    return np.abs(m) == 0.5


class T:
    """tracked number(s): value v (long double) and absolute error bound e of a float64 evaluation"""
    __slots__ = ("v", "e")
    __array_ufunc__ = None

    def __init__(self, v, e=None):
        self.v = np.asarray(v, LD)
        self.e = np.zeros(self.v.shape, LD) if e is None else np.asarray(e, LD)

    def __neg__(self):
        return T(-self.v, self.e)

    def __abs__(self):
        return T(np.abs(self.v), self.e)

    def __add__(a, b):
        b = _t(b)
        z = a.v + b.v
        e = a.e + b.e + U * np.abs(z)
        e = np.where((b.v == 0) & (b.e == 0), a.e, np.where((a.v == 0) & (a.e == 0), b.e, e))
        return T(z, e)

    __radd__ = __add__

    def __sub__(a, b):
        return a + (-_t(b))

    def __rsub__(a, b):
        return _t(b) + (-a)

    def __mul__(a, b):
        b = _t(b)
        z = a.v * b.v
        av, bv = np.abs(a.v), np.abs(b.v)
        e = av * b.e + bv * a.e + a.e * b.e + U * np.abs(z)
        e = np.where((b.e == 0) & _pow2(b.v), bv * a.e, np.where((a.e == 0) & _pow2(a.v), av * b.e, e))
        return T(z, e)

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = _t(b)
        z = a.v / b.v
        m = np.abs(b.v) - b.e
        e = np.where(m > 0, (a.e + np.abs(z) * b.e) / np.where(m > 0, m, 1) + U * np.abs(z), np.where(np.isnan(m), LD(np.nan), LD(np.inf)))
        return T(z, e)

    def __rtruediv__(a, b):
        return _t(b) / a


def _t(x):
    return x if isinstance(x, T) else T(x.astype(LD) if isinstance(x, np.ndarray) else LD(x))


class Ctx:
    """one batch of cases in one arithmetic: mode "tracked" or "f64"; defect: one of the planted defects of test_lie_reference_cpu.py (f64 only)"""

    def __init__(self, mode, names, forced, defect=None):
        self.mode, self.names, self.forced, self.defect = mode, names, forced, defect
        self.labels = {}

    def inp(self, col):
        col = np.asarray(col, np.float64)
        return T(col.astype(LD)) if self.mode == "tracked" else col.copy()

    def _n(self, x, name=None):
        if self.mode == "tracked":
            return _t(x)
        x = np.asarray(x, np.float64)
        if _RECORD is not None and name:
            _RECORD.setdefault(name, []).append(np.broadcast_to(x, (len(self.names),)).copy())
        return x

    # -- comparisons ---------------------------------------------------------------------------------------------------
    def cmp(self, a, op, b, label):
        n = len(self.names)
        if self.mode == "tracked":
            a, b = _t(a), _t(b)
            av, bv = np.broadcast_to(a.v, (n,)), np.broadcast_to(b.v, (n,))
            tol = np.broadcast_to(a.e + b.e, (n,))
        else:
            av, bv = np.broadcast_to(np.asarray(a, np.float64), (n,)), np.broadcast_to(np.asarray(b, np.float64), (n,))
            tol = np.zeros(n)
        with np.errstate(invalid="ignore"):
            res = np.array({"<": av < bv, ">": av > bv, "<=": av <= bv, ">=": av >= bv}[op])
            amb = (tol > 0) & (np.abs(av - bv) <= tol)
        if self.mode == "tracked":
            for k in range(n):
                f = self.forced[k].get(label)
                if f is not None:
                    if amb[k]:
                        res[k] = f
                    elif bool(res[k]) != bool(f):
                        raise PlantedBranchWrong(f"{self.names[k]}: {label} is {bool(res[k])} beyond doubt, planted {f}")
                elif amb[k]:
                    raise Ambiguous(f"{self.names[k]}: {label}: |{av[k]!r} - {bv[k]!r}| <= {tol[k]!r}")
        if res.any() and not res.all():
            raise _Split(res)
        self.labels[label] = bool(res[0])
        return bool(res[0])

    def note(self, label, value):
        self.labels[label] = value

    # -- functions -----------------------------------------------------------------------------------------------------
    def sqrt(self, x):
        x = self._n(x)
        with np.errstate(invalid="ignore"):
            if self.mode != "tracked":
                return np.sqrt(x)
            z = np.sqrt(x.v)
            lo, hi = np.sqrt(np.maximum(x.v - x.e, 0)), np.sqrt(x.v + x.e)
            return T(z, np.maximum(z - lo, hi - z) + U * z)

    def _trig(self, f, df, x, name):
        x = self._n(x, name)
        if self.mode != "tracked":
            return f(x)
        z = f(x.v)
        return T(z, x.e * np.minimum(1, np.abs(df(x.v)) + x.e) + LIBM_ULP[name] * ULP * np.abs(z))

    def sin(self, x, name="sin"):
        return self._trig(np.sin, np.cos, x, name)

    def cos(self, x, name="cos"):
        return self._trig(np.cos, np.sin, x, name)

    def sincos(self, x):
        s = self.sin(x, "sincos")
        if _RECORD is not None and self.mode != "tracked":
            _RECORD["sincos"].pop()                     # (recorded once, not twice)
        return s, self.cos(x, "sincos")

    def exp(self, x):
        x = self._n(x, "exp")
        if self.mode != "tracked":
            return np.exp(x)
        z = np.exp(x.v)
        return T(z, z * np.expm1(x.e) + LIBM_ULP["exp"] * ULP * z)

    def log(self, x):
        x = self._n(x, "log")
        with np.errstate(invalid="ignore", divide="ignore"):
            if self.mode != "tracked":
                return np.log(x)
            z = np.log(x.v)
            return T(z, np.where(x.e > 0, -np.log1p(-x.e / x.v), 0) + LIBM_ULP["log"] * ULP * np.abs(z))

    def acos(self, x):
        x = self._n(x, "acos")
        with np.errstate(invalid="ignore"):
            if self.mode != "tracked":
                r = np.arccos(x)
                return r * (1 + 64 * 2.0 ** -52) if self.defect == "g" else r     # (g): an acos with 64 ulp of error
            z = np.arccos(x.v)
            lo, hi = np.arccos(np.clip(x.v + x.e, -1, 1)), np.arccos(np.clip(x.v - x.e, -1, 1))
            return T(z, np.maximum(z - lo, hi - z) + LIBM_ULP["acos"] * ULP * np.abs(z))

    def fma(self, a, b, c):
        if self.mode != "tracked":
            a, b, c = (np.asarray(v, np.float64).astype(LD) for v in (a, b, c))
            return (a * b + c).astype(np.float64)            # (long double holds the product to 64 bits: a fused multiply-add to within 2^-11 ulp)
        a, b, c = _t(a), _t(b), _t(c)
        z = a.v * b.v + c.v
        return T(z, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e + U * np.abs(z))

    def f32_square(self, x):
        """(double)(float)(x * x) of an EXACT input: one correctly rounded product and one conversion, both reproduced here bit for bit"""
        if self.mode == "tracked":
            assert not x.e.any()
            v = x.v.astype(np.float64)
        else:
            v = x
        with np.errstate(over="ignore"):
            r = (v * v).astype(np.float32).astype(np.float64)
        return T(r.astype(LD)) if self.mode == "tracked" else r


# ---- ba_math.h -------------------------------------------------------------------------------------------------------------------------------------------
def normalize_rotation(c, q):
    """ba_normalize_rotation of (qx, qy, qz, qw): one reciprocal, four products"""
    if c.cmp(q[3], "<", 0.0, "norm.qw<0"):
        q = [-x for x in q]
    inv = 1.0 / c.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [x * inv for x in q]


def qrot(c, q, v):
    uv0, uv1, uv2 = q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]
    uv0, uv1, uv2 = uv0 + uv0, uv1 + uv1, uv2 + uv2
    return [v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1), v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2), v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0)]


def pose_map(c, T7, X):
    r = qrot(c, T7[:4], X)
    return [r[0] + T7[4], r[1] + T7[5], r[2] + T7[6]]


def q_to_R(c, q):
    qx, qy, qz, qw = q
    tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def R_to_q(c, m):
    """Eigen's Quaterniond(R): (qx, qy, qz, qw)"""
    t = m[0] + m[4] + m[8]
    if c.cmp(t, ">", 0.0, "R2q.trace>0"):
        c.note("R2q.branch", "trace")
        t = c.sqrt(t + 1.0)
        qw = 0.5 * t
        t = 0.5 / t
        return [(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, qw]
    gt = ">=" if c.defect == "b" else ">"                                  # (b): the tie rule
    i = 0
    if c.cmp(m[4], gt, m[0], "R2q.m11>m00"):
        i = 1
    if c.cmp(m[8], gt, m[0] if i == 0 else m[4], "R2q.m22>max"):
        i = 2
    c.note("R2q.branch", i)
    if i == 0:
        t = c.sqrt(m[0] - m[4] - m[8] + 1.0)
        qx = 0.5 * t; t = 0.5 / t
        return [qx, (m[3] + m[1]) * t, (m[6] + m[2]) * t, (m[7] - m[5]) * t]
    if i == 1:
        t = c.sqrt(m[4] - m[8] - m[0] + 1.0)
        qy = 0.5 * t; t = 0.5 / t
        qw = (m[6] - m[2]) * t if c.defect == "a" else (m[2] - m[6]) * t    # (a): j and k swapped: m(k, j) - m(j, k) changes sign, the two sums do not
        return [(m[1] + m[3]) * t, qy, (m[7] + m[5]) * t, qw]
    t = c.sqrt(m[8] - m[0] - m[4] + 1.0)
    qz = 0.5 * t; t = 0.5 / t
    return [(m[2] + m[6]) * t, (m[5] + m[7]) * t, qz, (m[3] - m[1]) * t]


def _skew(o):
    return [0.0, -o[2], o[1], o[2], 0.0, -o[0], -o[1], o[0], 0.0]


def _sq3(Om):
    out = []
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s = s + Om[i * 3 + k] * Om[k * 3 + j]
            out.append(s)
    return out


def _eye(i):
    return 1.0 if i % 4 == 0 else 0.0


def _qmul_norm(c, E, Et, T7):
    """E * T and the final normalisation, shared by ba_oplus and ba_oplus_fast"""
    rt = qrot(c, E, T7[4:7])
    t = [Et[0] + rt[0], Et[1] + rt[1], Et[2] + rt[2]]
    ex, ey, ez, ew = E
    tx, ty, tz, tw = T7[:4]
    qw = ew * tw - ex * tx - ey * ty - ez * tz
    qx = ew * tx + ex * tw + ey * tz - ez * ty
    qy = ew * ty + ey * tw + ez * tx - ex * tz
    qz = ew * tz + ez * tw + ex * ty - ey * tx
    return normalize_rotation(c, [qx, qy, qz, qw]) + t


def oplus(c, u, T7):
    o = u[:3]
    theta = c.sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2])
    Om = _skew(o)
    Om2 = _sq3(Om)
    if c.cmp(theta, "<", EPS, "theta<eps"):
        R = [_eye(i) + Om[i] + Om2[i] for i in range(9)]
        V = R
    else:
        st, ct = c.sincos(theta)
        it = 1.0 / theta
        it2 = it * it
        a, b, cc = st * it, (1.0 - ct) * it2, (theta - st) * it2 * it
        R = [_eye(i) + a * Om[i] + b * Om2[i] for i in range(9)]
        V = [_eye(i) + b * Om[i] + cc * Om2[i] for i in range(9)]
    E = R_to_q(c, R)
    Et = [V[0] * u[3] + V[1] * u[4] + V[2] * u[5], V[3] * u[3] + V[4] * u[4] + V[5] * u[5], V[6] * u[3] + V[7] * u[4] + V[8] * u[5]]
    E = normalize_rotation(c, E)
    return _qmul_norm(c, E, Et, T7)


def _horner(c, x, coef):
    """fma(x, fma(x, ... fma(x, coef[0], coef[1]) ..., coef[-2]), coef[-1])"""
    acc = c.fma(x, coef[0], coef[1])
    for k in coef[2:]:
        acc = c.fma(x, acc, k)
    return acc


# the header's constants: quotients of doubles, rounded once by the compiler as Python rounds them here
SH = [1.0 / 6227020800.0, -1.0 / 39916800, 1.0 / 362880, -1.0 / 5040, 1.0 / 120, -1.0 / 6, 1.0]
CW = [-1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800, 1.0 / 40320, -1.0 / 720, 1.0 / 24, -1.0 / 2, 1.0]
CB = [-1.0 / 20922789888000.0, 1.0 / 87178291200.0, -1.0 / 479001600.0, 1.0 / 3628800, -1.0 / 40320, 1.0 / 720, -1.0 / 24, 1.0 / 2]
CC = [-1.0 / 355687428096000.0, 1.0 / 1307674368000.0, -1.0 / 6227020800.0, 1.0 / 39916800, -1.0 / 362880, 1.0 / 5040, -1.0 / 120, 1.0 / 6]


def oplus_fast(c, u, T7):
    """ba_oplus_fast with its own series"""
    o0, o1, o2 = u[:3]
    x = o0 * o0 + o1 * o1 + o2 * o2
    lo = ">" if c.defect == "h" else ">="                                    # (h): the tie rule at theta^2 == 1e-10
    if not (c.cmp(x, lo, 1e-10, "fast.x>=1e-10") and c.cmp(x, "<", 0.25, "fast.x<0.25")):
        c.note("fast.series", False)
        return oplus(c, u, T7)
    c.note("fast.series", True)
    y = 0.25 * x
    sh_coef = list(SH)
    if c.defect == "e":
        sh_coef[5] = sh_coef[5] * (1 + 1e-12)                                # (e): one Horner coefficient off by 1e-12 relative
    sh = _horner(c, y, sh_coef)
    cw = _horner(c, y, CW)
    b = _horner(c, x, CB)
    cc = _horner(c, x, CC)
    hs = 0.5 * sh
    E = [hs * o0, hs * o1, hs * o2, cw]
    w0, w1, w2 = o1 * u[5] - o2 * u[4], o2 * u[3] - o0 * u[5], o0 * u[4] - o1 * u[3]
    z0, z1, z2 = o1 * w2 - o2 * w1, o2 * w0 - o0 * w2, o0 * w1 - o1 * w0
    Et = [u[3] + b * w0 + cc * z0, u[4] + b * w1 + cc * z1, u[5] + b * w2 + cc * z2]
    return _qmul_norm(c, E, Et, T7)


def huber(c, e2, delta):
    dsqr = c.f32_square(delta)
    if c.cmp(delta, "<=", 0.0, "huber.delta<=0") or c.cmp(e2, "<=", dsqr, "huber.inlier"):
        return [e2, 1.0]
    s = c.sqrt(e2)
    return [2.0 * s * delta - dsqr, delta / s]


def sym3_inv(c, a):
    c00 = a[3] * a[5] - a[4] * a[4]
    c01 = a[4] * a[2] - a[1] * a[5]
    c02 = a[1] * a[4] - a[3] * a[2]
    det = c00 * a[0] + c01 * a[1] + c02 * a[2]
    idet = 1.0 / det
    return [c00 * idet, c01 * idet, c02 * idet, (a[0] * a[5] - a[2] * a[2]) * idet, (a[2] * a[1] - a[0] * a[4]) * idet, (a[0] * a[3] - a[1] * a[1]) * idet]


def spd6_inv(c, A):
    """None: not positive definite (ba_spd6_inv returned false and left Inv untouched)"""
    L = [0.0] * 36
    for j in range(6):
        d = A[j * 6 + j]
        for k in range(j):
            d = d - L[j * 6 + k] * L[j * 6 + k]
        if not c.cmp(d, ">", 0.0, f"spd6.pivot{j}>0"):
            return None
        d = c.sqrt(d)
        L[j * 6 + j] = d
        for i in range(j + 1, 6):
            s = A[i * 6 + j]
            for k in range(j):
                s = s - L[i * 6 + k] * L[j * 6 + k]
            L[i * 6 + j] = s / d
    Li = [0.0] * 36
    for cc in range(6):
        Li[cc * 6 + cc] = 1.0 / L[cc * 6 + cc]
        for r in range(cc + 1, 6):
            s = 0.0
            for k in range(cc, r):
                s = s - L[r * 6 + k] * Li[k * 6 + cc]
            Li[r * 6 + cc] = s / L[r * 6 + r]
    Inv = [0.0] * 36
    for r in range(6):
        for cc in range(r + 1):
            s = 0.0
            for k in range(r, 6):
                s = s + Li[k * 6 + r] * Li[k * 6 + cc]
            Inv[r * 6 + cc] = s
            Inv[cc * 6 + r] = s
    return Inv


# ---- sim3_math.h -----------------------------------------------------------------------------------------------------------------------------------------
def _next_up(x):
    return float(np.nextafter(np.float64(x), np.inf))


def _abc(c, theta, sigma, s, small, label):
    """A, B, C of Sim3(Vector7d) and Sim3::log: the four (theta, sigma) branches; `small` is the theta branch already taken"""
    if c.defect == "c":
        sig_small = False                                                    # (c): the |sigma| < eps test dropped
    elif c.defect == "d":
        sig_small = c.cmp(abs(sigma), "<=", _next_up(EPS), label)            # (d): C = 1 also for |sigma| just above eps
    else:
        sig_small = c.cmp(abs(sigma), "<", EPS, label)
    c.note(label, sig_small)
    if sig_small:
        C = 1.0
        if small:
            A, B = 1. / 2., 1. / 6.
        else:
            theta2 = theta * theta
            A = (1.0 - c.cos(theta)) / theta2
            B = (theta - c.sin(theta)) / (theta2 * theta)
    else:
        C = (s - 1.0) / sigma
        if small:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
        else:
            a, b = s * c.sin(theta), s * c.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            cc = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * cc)
            B = (C - ((b - 1.0) * sigma + a * theta) / cc) * 1.0 / theta2
    return A, B, C


def sim3_exp(c, u):
    sigma = u[6]
    theta = c.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    Om = _skew(u[:3])
    Om2 = _sq3(Om)
    s = c.exp(sigma)
    small = c.cmp(theta, "<", EPS, "theta<eps")
    if small:
        R = [_eye(i) + Om[i] + Om2[i] for i in range(9)]
    else:
        a, b = c.sin(theta) / theta, (1.0 - c.cos(theta)) / (theta * theta)
        R = [_eye(i) + a * Om[i] + b * Om2[i] for i in range(9)]
    A, B, C = _abc(c, theta, sigma, s, small, "|sigma|<eps")
    q = R_to_q(c, R)
    t = []
    for i in range(3):
        acc = 0.0
        for k in range(3):
            W = A * Om[i * 3 + k] + B * Om2[i * 3 + k] + C * (1.0 if i == k else 0.0)
            acc = acc + W * u[3 + k]
        t.append(acc)
    return q + t + [s]


def sim3_mul(c, a, b):
    qw = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]
    qx = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1]
    qy = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]
    qz = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0]
    rt = qrot(c, a[:4], b[4:7])
    return [qx, qy, qz, qw, a[7] * rt[0] + a[4], a[7] * rt[1] + a[5], a[7] * rt[2] + a[6], a[7] * b[7]]


def sim3_inv(c, a):
    q = [-a[0], -a[1], -a[2], a[3]]
    k = -1.0 / a[7]
    t = qrot(c, q, [k * a[4], k * a[5], k * a[6]])
    return q + t + [1.0 / a[7]]


def sim3_map(c, S, X):
    r = qrot(c, S[:4], X)
    return [S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]]


def lu3_solve(c, W, t):
    """Eigen's PartialPivLU<Matrix3d>: the first maximum of the column wins"""
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = W
    y0, y1, y2 = t
    best, bv = 0, abs(a00)
    if c.cmp(abs(a10), ">", bv, "lu3.col0.row1"):
        bv, best = abs(a10), 1
    if c.cmp(abs(a20), ">", bv, "lu3.col0.row2"):
        best = 2
    if best == 1:
        a00, a10, a01, a11, a02, a12, y0, y1 = a10, a00, a11, a01, a12, a02, y1, y0
    elif best == 2:
        a00, a20, a01, a21, a02, a22, y0, y2 = a20, a00, a21, a01, a22, a02, y2, y0
    a10 = a10 / a00; a20 = a20 / a00
    a11 = a11 - a10 * a01; a12 = a12 - a10 * a02
    a21 = a21 - a20 * a01; a22 = a22 - a20 * a02
    second = False if c.defect == "f" else c.cmp(abs(a21), ">", abs(a11), "lu3.col1.row2")      # (f): the second pivot not taken
    c.note("lu3.order", (best, int(second)))
    if second:
        a10, a20, a11, a21, a12, a22, y1, y2 = a20, a10, a21, a11, a22, a12, y2, y1
    a21 = a21 / a11
    a22 = a22 - a21 * a12
    y1 = y1 - a10 * y0
    y2 = y2 - a20 * y0; y2 = y2 - a21 * y1
    x2 = y2 / a22
    x1 = (y1 - a12 * x2) / a11
    x0 = (y0 - a01 * x1 - a02 * x2) / a00
    return [x0, x1, x2]


def sim3_log(c, S):
    sigma = c.log(S[7])
    R = q_to_R(c, S[:4])
    d = 0.5 * (R[0] + R[4] + R[8] - 1.0)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    small = c.cmp(d, ">", 1 - EPS, "d>1-eps")
    theta = 0.0
    if small:
        omega = [0.5 * x for x in dR]
    else:
        theta = c.acos(d)
        k = theta / (2.0 * c.sqrt(1.0 - d * d))
        omega = [k * x for x in dR]
    A, B, C = _abc(c, theta, sigma, S[7], small, "|sigma|<eps")
    Om = _skew(omega)
    W = []
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + Om[i * 3 + k] * Om[k * 3 + j]
            W.append(A * Om[i * 3 + j] + B * acc + C * (1.0 if i == j else 0.0))
    ups = lu3_solve(c, W, S[4:7])
    return omega + ups + [sigma]


def pg_edge_error(c, x):
    """EdgeSim3::computeError as posegraph.hip composes it: log(C * Si * Sj^-1); x = C (8) | Si (8) | Sj (8)"""
    return sim3_log(c, sim3_mul(c, sim3_mul(c, x[:8], x[8:16]), sim3_inv(c, x[16:24])))


# ---- the ops: name -> (LieOp number of csrc/test_lie_ops.h or None, inputs, outputs, function of (c, list of inputs)) ------------------------------------
OPS = {
    "normalize": (0, 7, 7, lambda c, x: normalize_rotation(c, x[:4]) + x[4:7]),
    "qrot": (1, 7, 3, lambda c, x: qrot(c, x[:4], x[4:7])),
    "map": (2, 10, 3, lambda c, x: pose_map(c, x[:7], x[7:10])),
    "q_to_R": (3, 7, 9, lambda c, x: q_to_R(c, x[:4])),
    "R_to_q": (4, 9, 4, lambda c, x: R_to_q(c, x)),
    "oplus": (5, 13, 7, lambda c, x: oplus(c, x[:6], x[6:13])),
    "oplus_fast": (6, 13, 7, lambda c, x: oplus_fast(c, x[:6], x[6:13])),
    "huber": (7, 2, 2, lambda c, x: huber(c, x[0], x[1])),
    "sym3_inv": (8, 6, 6, lambda c, x: sym3_inv(c, x)),
    "spd6_inv": (9, 36, 36, lambda c, x: spd6_inv(c, x)),
    "sim3_exp": (10, 7, 8, lambda c, x: sim3_exp(c, x)),
    "sim3_log": (11, 8, 7, lambda c, x: sim3_log(c, x)),
    "sim3_mul": (12, 16, 8, lambda c, x: sim3_mul(c, x[:8], x[8:16])),
    "sim3_inv": (13, 8, 8, lambda c, x: sim3_inv(c, x)),
    "sim3_map": (14, 11, 3, lambda c, x: sim3_map(c, x[:8], x[8:11])),
    "lu3": (15, 12, 3, lambda c, x: lu3_solve(c, x[:9], x[9:12])),
    "pg_err": (None, 24, 7, pg_edge_error),
    # compositions for the group identities of tests/test_lie_reference_cpu.py
    "log_exp": (None, 7, 7, lambda c, x: sim3_log(c, sim3_exp(c, x))),
    "mul_inv": (None, 8, 8, lambda c, x: sim3_mul(c, x, sim3_inv(c, x))),
    "R_round_trip": (None, 4, 18, lambda c, x: (lambda R: R + q_to_R(c, R_to_q(c, R)))(q_to_R(c, x))),
}
RAW_OPS = {"sin": 16, "cos": 17, "sincos": 18, "exp": 19, "log": 20, "acos": 21, "sqrt": 22, "rcp": 23, "div": 24, "fma": 25}
DEVICE_OPS = [k for k, v in OPS.items() if v[0] is not None]


class Cases:
    """a case table of one op: names, x[n, 48] (float64), forced[n] (dict label -> bool)"""

    def __init__(self, op):
        self.op, self.names, self.rows, self.forced = op, [], [], []

    def add(self, name, x, forced=None):
        x = np.asarray(x, np.float64).ravel()
        assert x.size == OPS[self.op][1], (self.op, name, x.size)
        self.names.append(f"{self.op}/{name}")
        self.rows.append(np.concatenate([x, np.zeros(N_IN - x.size)]))
        self.forced.append(dict(forced or {}))

    @property
    def x(self):
        return np.stack(self.rows)

    def index(self, name):
        return self.names.index(f"{self.op}/{name}")

    def __len__(self):
        return len(self.names)


def evaluate(op, x, names=None, forced=None, mode="tracked", defect=None):
    """The op over the cases x[n, >= inputs].  Returns dict(val[n, m], bnd[n, m], ok[n] (False: ba_spd6_inv's false return), labels[n]); in f64 mode val is
    float64 and bnd is absent."""
    _, n_in, n_out, fn = OPS[op]
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    names = names or [f"{op}/#{k}" for k in range(n)]
    forced = forced or [{}] * n
    dt = LD if mode == "tracked" else np.float64
    val, bnd = np.full((n, n_out), np.nan, dt), np.full((n, n_out), np.nan, LD)
    ok, labels = np.ones(n, bool), [None] * n

    def rec(idx):
        c = Ctx(mode, [names[k] for k in idx], [forced[k] for k in idx], defect)
        try:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
                out = fn(c, [c.inp(x[idx, j]) for j in range(n_in)])
        except _Split as s:
            rec(idx[s.mask]); rec(idx[~s.mask])
            return
        for k in idx:
            labels[k] = c.labels
        if out is None:
            ok[idx] = False
            return
        for j, o in enumerate(out):
            if isinstance(o, T):
                val[idx, j], bnd[idx, j] = np.broadcast_to(o.v, idx.shape), np.broadcast_to(o.e, idx.shape)
            else:
                val[idx, j], bnd[idx, j] = np.broadcast_to(np.asarray(o, dt), idx.shape), 0
    rec(np.arange(n))
    r = dict(val=val, ok=ok, labels=labels)
    if mode == "tracked":
        r["bnd"] = bnd
    return r


def failures(ref, names, got, factor=1.0):
    """(name, output, error, bound) of every output of `got` (float64 [n, >= m]) farther than factor x bound from the tracked value; a zero bound asks for equality"""
    m = ref["val"].shape[1]
    g = np.asarray(got, np.float64)[:, :m].astype(LD)
    with np.errstate(invalid="ignore"):
        err = np.abs(g - ref["val"])
        bad = ~(err <= factor * ref["bnd"]) & ref["ok"][:, None]
    return [(names[i], int(j), float(err[i, j]), float(ref["bnd"][i, j])) for i, j in zip(*np.nonzero(bad))]


def worst_ratio(ref, got):
    """largest error / bound over the outputs with a positive bound"""
    m = ref["val"].shape[1]
    g = np.asarray(got, np.float64)[:, :m].astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = (ref["bnd"] > 0) & ref["ok"][:, None] & np.isfinite(ref["bnd"])
        r = np.where(pos, np.abs(g - ref["val"]) / np.where(pos, ref["bnd"], 1), 0)
    return float(r.max()) if r.size else 0.0


# ---- case tables ---------------------------------------------------------------------------------------------------------------------------------------------
TWO_PI_3 = float(2 * np.pi / 3)
TH_LOG = float(np.arccos(np.float64(1 - 1e-5)))          # theta at which Sim3::log leaves its small branch (d = 1 - 1e-5)
THETAS_EDGE = {"0": 0.0, "1e-12": 1e-12, "eps-": float(np.nextafter(EPS, 0)), "eps": EPS, "eps+": float(np.nextafter(EPS, 1)), "0.5-": float(np.nextafter(0.5, 0)),
               "0.5": 0.5}                                   # planted on an axis: theta = |omega_x| exactly, the branch carried
THETAS = {"3e-5": 3e-5, "1e-3": 1e-3, "thlog-": TH_LOG * (1 - 1e-9), "thlog+": TH_LOG * (1 + 1e-9), "0.1": 0.1, "1": 1.0, "2": 2.0,
          "2pi/3-": TWO_PI_3 * (1 - 1e-9), "2pi/3+": TWO_PI_3 * (1 + 1e-9), "2.5": 2.5, "3": 3.0, "pi-1e-3": float(np.pi - 1e-3), "pi-1e-4": float(np.pi - 1e-4)}
SIGMAS = {"0": 0.0, "+eps-": float(np.nextafter(EPS, 0)), "+eps": EPS, "+eps+": float(np.nextafter(EPS, 1)), "-eps-": -float(np.nextafter(EPS, 0)), "-eps": -EPS,
          "-eps+": -float(np.nextafter(EPS, 1)), "1e-3": 1e-3, "-1e-3": -1e-3, "-0.7": -0.7, "2": 2.0}
UPS = {"0": 0.0, "1": 1.0, "1e3": 1e3}


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _omega_cases(seed):
    """(name, omega, forced): every theta of the tables; the edge ones on an axis (cycling x, y, z and the sign), the others on a random and on each coordinate axis"""
    rng = np.random.default_rng(seed)
    out = []
    for k, (nm, th) in enumerate(THETAS_EDGE.items()):
        o = np.zeros(3); o[k % 3] = th if k % 2 == 0 else -th
        out.append((f"theta={nm}", o, {"theta<eps": th < EPS}))
    for nm, th in THETAS.items():
        out.append((f"theta={nm}", th * _unit(rng), {}))
        for ax in range(3):
            o = np.zeros(3); o[ax] = th
            # on the z axis m00 == m11 in exact arithmetic and bit for bit in every float64 evaluation: the later m22 > max(.) decides alone
            out.append((f"theta={nm},axis{'xyz'[ax]}", o, {"R2q.m11>m00": False} if ax == 2 else {}))
    return out


def exp_cases():
    """sim3_exp: every theta x every sigma (all four branch combinations, the thresholds from both sides) x upsilon 0 / O(1) / 1e3, then 600 random ones"""
    cs, rng = Cases("sim3_exp"), np.random.default_rng(11)
    for tn, o, f in _omega_cases(1):
        for sn, sg in SIGMAS.items():
            for un, up in UPS.items():
                cs.add(f"{tn},sigma={sn},ups={un}", np.concatenate([o, up * rng.normal(size=3), [sg]]), f)
    for k in range(600):
        th = [rng.uniform(2e-5, 2.0), rng.uniform(2.2, 3.1), rng.uniform(0, 5e-6)][k % 3]
        cs.add(f"random{k}", np.concatenate([th * _unit(rng), rng.normal(size=3) * 10.0 ** rng.uniform(-2, 2), [rng.uniform(-1, 1) * 10.0 ** rng.uniform(-4, 0)]]))
    return cs


def _quat(o):
    """float64 unit quaternion (x, y, z, w) of the rotation vector o"""
    th = np.linalg.norm(o)
    if th == 0:
        return np.array([0.0, 0, 0, 1])
    return np.concatenate([np.sin(th / 2) * o / th, [np.cos(th / 2)]])


def _random_sim3(rng, th_max=3.1, unit=True):
    q = _quat(rng.uniform(0, th_max) * _unit(rng))
    if not unit:
        q = q * rng.choice([0.5, 2.0])
    return np.concatenate([q, rng.normal(size=3) * 10.0 ** rng.uniform(-1, 2), [np.exp(rng.uniform(-0.7, 0.7))]])


def log_cases():
    """sim3_log: quaternions of every theta (d = cos theta: 1 - 1e-5 from both sides) x scales exp(sigma) (|log s| = 1e-5 (1 -+ 1e-9): the exact threshold cannot be
    planted through log) x translations 0 / O(1) / 1e3, all four branch combinations, then 600 random ones"""
    cs, rng = Cases("sim3_log"), np.random.default_rng(12)
    sig = {k: v for k, v in SIGMAS.items() if "eps" not in k}
    sig.update({"+eps(1-1e-9)": EPS * (1 - 1e-9), "+eps(1+1e-9)": EPS * (1 + 1e-9), "-eps(1-1e-9)": -EPS * (1 - 1e-9), "-eps(1+1e-9)": -EPS * (1 + 1e-9)})
    for tn, o, _ in _omega_cases(2):
        for sn, sg in sig.items():
            for un, up in UPS.items():
                cs.add(f"{tn},sigma={sn},t={un}", np.concatenate([_quat(o), up * rng.normal(size=3), [np.exp(sg)]]))
    for k in range(600):
        cs.add(f"random{k}", _random_sim3(rng))
    return cs


FACT1 = (1e-5, 4.47e-3)      # log(exp(u)) != u for theta in this range with |sigma| >= 1e-5 (g2o's B)


def group_cases(op):
    """sim3_mul / sim3_inv / sim3_map / qrot / map / q_to_R / normalize: random transforms, unit quaternions and quaternions of norm 0.5 and 2 (the headers do not
    normalise), translations 0.1 ... 100; normalize also with qw < 0, qw = -0.0 and qw = 0"""
    cs, rng = Cases(op), np.random.default_rng(20 + len(op))
    for k in range(400):
        a, b = _random_sim3(rng, unit=k % 3 != 0), _random_sim3(rng, unit=k % 5 != 0)
        X = rng.normal(size=3) * 10.0 ** rng.uniform(-1, 2)
        nm = f"random{k}" + (",norm!=1" if k % 3 == 0 else "")
        if op == "sim3_mul":
            cs.add(nm, np.concatenate([a, b]))
        elif op == "sim3_inv":
            cs.add(nm, a)
        elif op == "sim3_map":
            cs.add(nm, np.concatenate([a, X]))
        elif op == "qrot":
            cs.add(nm, np.concatenate([a[:4], X]))
        elif op == "map":
            cs.add(nm, np.concatenate([a[:7], X]))
        elif op == "q_to_R":
            cs.add(nm, a[:7])
        elif op == "normalize":
            q = a[:7].copy()
            if k % 2:
                q[:4] = -q[:4]
            cs.add(nm + (",qw<0" if q[3] < 0 else ""), q)
    if op == "normalize":
        cs.add("qw=-0.0", [0.6, 0.0, 0.8, -0.0, 1, 2, 3])
        cs.add("qw=0", [0.6, 0.0, 0.8, 0.0, 1, 2, 3])
        cs.add("norm=0.5,qw<0", [0.1, -0.2, 0.4, -0.2, 1, 2, 3])
        cs.add("norm=2", [1.0, 1.0, 1.0, 1.0, 0, 0, 0])
    return cs


def _R64(o):
    x, y, z, w = _quat(np.asarray(o, float))
    return np.array([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])


def _R_pi(n):
    """rotation by pi about the INTEGER direction n of squared length 2: n n^T - I, exact"""
    n = np.asarray(n, float)
    return (2 * np.outer(n, n) / (n @ n) - np.eye(3)).ravel()


S2 = float(np.sqrt(0.5))
# known answers: name -> (matrix, quaternion, branch, exact); exact False: 0.5 sqrt(2) and 2 (0.5 / sqrt(2)) are each within an ulp of sqrt(1/2), the zeros are exact
R_TO_Q_KNOWN = {
    "diag(1,-1,-1)": (np.diag([1., -1, -1]).ravel(), [1, 0, 0, 0], 0, True),
    "diag(-1,1,-1)": (np.diag([-1., 1, -1]).ravel(), [0, 1, 0, 0], 1, True),
    "diag(-1,-1,1)": (np.diag([-1., -1, 1]).ravel(), [0, 0, 1, 0], 2, True),
    "identity": (np.eye(3).ravel(), [0, 0, 0, 1], "trace", True),
    "cyclic permutation": (np.array([0., 0, 1, 1, 0, 0, 0, 1, 0]), [.5, .5, .5, .5], 0, True),          # trace == 0 takes the else-branch, three-way tie: i = 0
    "pi about (1,1,0)": (_R_pi([1, 1, 0]), [S2, S2, 0, 0], 0, False),                                  # m00 == m11 > m22: the strict > keeps i = 0
    "pi about (1,-1,0)": (_R_pi([1, -1, 0]), [S2, -S2, 0, 0], 0, False),                               # the same tie; with >= the answer changes sign
    "pi about (0,1,-1)": (_R_pi([0, 1, -1]), [0, S2, -S2, 0], 1, False),                               # m11 == m22 > m00: i = 1
    "pi about (1,0,-1)": (_R_pi([1, 0, -1]), [S2, 0, -S2, 0], 0, False),                               # m00 == m22 > m11: i = 0
}


def r_to_q_cases():
    """ba_R_to_q: the known answers (ties exact), then rotations of 100 ... 179.9 degrees about axes near x, y and z (branches 0, 1, 2 with generic off-diagonal
    entries), 150 random rotations of every angle (trace branch and the others), the trace on either side of 0"""
    cs, rng = Cases("R_to_q"), np.random.default_rng(13)
    for nm, (m, _, _, _) in R_TO_Q_KNOWN.items():
        cs.add(nm, m)
    for ax in range(3):
        for deg in (100, 125, 150, 170, 175, 179, 179.9):
            n = np.eye(3)[ax] + 0.25 * rng.normal(size=3)
            cs.add(f"i{ax} generic {deg}deg", _R64(np.deg2rad(deg) * n / np.linalg.norm(n)))
    for k in range(150):
        cs.add(f"random{k}", _R64(rng.uniform(0, 3.1) * _unit(rng)))
    for sgn in (-1, 1):
        cs.add(f"trace {'+' if sgn > 0 else '-'}1e-9", _R64(TWO_PI_3 * (1 - sgn * 1e-9) * _unit(rng)))
    return cs


def _theta2_cases():
    """omega with theta^2 = fl(omega . omega) at the doubles below / at / above 1e-10 and 0.25.  On an axis the squares of doubles are sparse: 0.25 is one (0.5^2),
    its neighbours below and above are the nearest representable squares; no double squares to 1e-10 (fl(1e-5^2) is one ulp above it), so "at 1e-10" takes the
    "below" value on x and a second component on y, found by a short search, with fl(fl(o0^2) + fl(o1^2)) == 1e-10 exactly.  Every case carries its branches."""
    out = []
    for tn, target in (("1e-10", 1e-10), ("0.25", 0.25)):
        cand = [np.float64(np.sqrt(target))]
        for _ in range(6):
            cand = [np.nextafter(cand[0], 0)] + cand + [np.nextafter(cand[-1], 1)]
        sq = np.array([float(v * v) for v in cand])
        below, above = max(k for k in range(len(cand)) if sq[k] < target), min(k for k in range(len(cand)) if sq[k] > target)
        picks = {"below": np.array([cand[below], 0, 0]), "above": np.array([0, cand[above], 0])}
        at = [k for k in range(len(cand)) if sq[k] == target]
        if at:
            picks["at"] = np.array([0, 0, cand[at[0]]])
        else:
            o1 = np.float64(np.sqrt(np.float64(target) - sq[below]))
            for _ in range(64):
                if float(np.float64(sq[below]) + o1 * o1) == target:
                    picks["at"] = np.array([cand[below], o1, 0])
                    break
                o1 = np.nextafter(o1, 1 if float(np.float64(sq[below]) + o1 * o1) < target else 0)
        assert set(picks) == {"below", "at", "above"}, (tn, sorted(picks))
        for nm, o in picks.items():
            x = np.float64(o[0]) * o[0] + np.float64(o[1]) * o[1] + np.float64(o[2]) * o[2]          # the header's order
            assert (x < target, x == target, x > target)[("below", "at", "above").index(nm)], (tn, nm, x)
            f = {"fast.x>=1e-10": bool(x >= 1e-10), "fast.x<0.25": bool(x < 0.25), "theta<eps": bool(np.sqrt(x) < EPS)}
            if o[2] != 0:
                f["R2q.m11>m00"] = False
            out.append((f"theta2 {nm} {tn}", o, f))
    return out


def oplus_cases(op):
    """ba_oplus / ba_oplus_fast: every theta of the tables (theta^2 at the doubles below / at / above 1e-10 and 0.25: _theta2_cases) x upsilon 0 / O(1) /
    1e3 x poses with unit quaternions of either sign of qw, then 600 random updates, three quarters of them in the series' range"""
    cs, rng = Cases(op), np.random.default_rng(14)
    for tn, o, f in _omega_cases(3) + _theta2_cases():
        for un, up in UPS.items():
            T7 = _random_sim3(rng)[:7]
            if len(cs) % 2:
                T7[:4] = -T7[:4]
            cs.add(f"{tn},ups={un}", np.concatenate([o, up * rng.normal(size=3), T7]), f)
    for k in range(600):
        th = 10.0 ** rng.uniform(-4.9, -0.31) if k % 4 else rng.uniform(0.51, 3.0)
        cs.add(f"random{k}", np.concatenate([th * _unit(rng), rng.normal(size=3) * 10.0 ** rng.uniform(-3, 1), _random_sim3(rng)[:7]]))
    return cs


def huber_cases():
    """ba_huber: e2 at the f32-rounded delta^2, the doubles next to it, far inside and outside, e2 = 0, delta <= 0"""
    cs = Cases("huber")
    for dn, delta in (("sqrt5.991", float(np.float32(np.sqrt(5.991)))), ("sqrt7.815", float(np.float32(np.sqrt(7.815)))), ("1", 1.0), ("0.1", 0.1)):
        d2 = float(np.float32(np.float64(delta) * np.float64(delta)))
        for en, e2 in (("=dsqr", d2), ("=next above dsqr", float(np.nextafter(d2, np.inf))), ("=next below dsqr", float(np.nextafter(d2, 0))), ("=0", 0.0),
                       ("=0.3 dsqr", 0.3 * d2), ("=50 dsqr", 50 * d2), ("=1e8", 1e8)):
            cs.add(f"delta={dn},e2{en}", [e2, delta])
    for delta in (0.0, -1.0):
        for e2 in (0.0, 3.0, 1e6):
            cs.add(f"delta={delta},e2={e2}", [e2, delta])
    return cs


def _spd(rng, n, cond):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.geomspace(1, 1 / cond, n)) @ Q.T
    return (A + A.T) / 2


def sym3_cases():
    """ba_sym3_inv: SPD matrices with cond 1 ... 1e10, scaled by 1e-6, 1 and 1e6; the identity and a diagonal one"""
    cs, rng = Cases("sym3_inv"), np.random.default_rng(15)
    iu = [0, 1, 2, 4, 5, 8]
    cs.add("identity", np.eye(3).ravel()[iu])
    cs.add("diag(1,2,4)", np.diag([1., 2, 4]).ravel()[iu])
    for ce in range(0, 11, 2):
        for k in range(20):
            cs.add(f"cond=1e{ce},#{k}", (_spd(rng, 3, 10.0 ** ce) * 10.0 ** rng.choice([-6, 0, 6])).ravel()[iu])
    return cs


SPD6_FALSE = ("zero pivot 0", "zero pivot 3", "negative pivot 4", "NaN on the diagonal")


def spd6_cases():
    """ba_spd6_inv: SPD matrices with cond 1 ... 1e10; then a zero first pivot, a zero pivot in row 3 of a matrix whose factorisation is exact, a negative pivot
    and a NaN entry on the diagonal: these four return false"""
    cs, rng = Cases("spd6_inv"), np.random.default_rng(16)
    cs.add("identity", np.eye(6).ravel())
    for ce in range(0, 11, 2):
        for k in range(12):
            cs.add(f"cond=1e{ce},#{k}", _spd(rng, 6, 10.0 ** ce).ravel())
    A = np.eye(6); A[0, 0] = 0
    cs.add("zero pivot 0", A.ravel())
    L = np.tril(np.ones((6, 6))); L[3, 3] = 0                                  # L L^T in small integers: every step of the factorisation is exact
    cs.add("zero pivot 3", (L @ L.T).ravel(), {"spd6.pivot3>0": False})
    A = np.eye(6) * 2; A[4, 4] = -1
    cs.add("negative pivot 4", A.ravel())
    A = _spd(rng, 6, 10.0); A[2, 2] = np.nan
    cs.add("NaN on the diagonal", A.ravel())
    return cs


LU3_ORDERS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
# the planted ties in whole numbers and the (column 0 row, column 1 swap) that Eigen's first-maximum rule gives them
LU3_TIES = {"tie col0 rows 0,1": ([2, 1, 0, -2, 1, 1, 1, 0, 3], (0, 0)), "tie col0 rows 1,2": ([1, 1, 0, -2, 1, 1, 2, 0, 3], (1, 0)),
            "tie col0 all": ([2, 1, 0, 2, 3, 1, -2, 0, 5], (0, 0)), "tie col1": ([4, 0, 1, 0, 2, 1, 0, -2, 3], (0, 0)),
            "zero second pivot": ([1, 1, 0, 1, 1, 1, 0, 1, 1], (0, 1))}


def lu3_cases():
    """sim3_lu3_solve: each of the 3 x 2 pivot orders x cond 1 ... 1e12, ties in column 0 (first maximum wins) and in column 1 (no swap), a second pivot that is
    exactly zero unless the rows are swapped"""
    cs, rng = Cases("lu3"), np.random.default_rng(17)
    for (p0, p1) in LU3_ORDERS:
        for ce in (0, 3, 6, 9, 12):
            for k in range(6):
                # rows of L U with |L| <= 0.8, permuted so that the pivot order is (p0, p1) beyond doubt
                Lm = np.eye(3); Lm[1, 0], Lm[2, 0], Lm[2, 1] = rng.uniform(-0.8, 0.8, 3)
                Um = np.triu(rng.normal(size=(3, 3))); Um[np.diag_indices(3)] = np.geomspace(1, 10.0 ** -ce, 3) * rng.choice([-1, 1], 3)
                Um[0, 1:] *= 0.5; Um[1, 2] *= 10.0 ** (-ce / 2)
                rows = [0, 1, 2]
                if p1:
                    rows[1], rows[2] = rows[2], rows[1]
                if p0:
                    rows[0], rows[p0] = rows[p0], rows[0]
                cs.add(f"order=({p0},{p1}),cond~1e{ce},#{k}", np.concatenate([(Lm @ Um)[rows].ravel(), rng.normal(size=3)]))
    for nm, (W, _) in LU3_TIES.items():
        cs.add(nm, W + [1, 2, 3])
    return cs


def out_of_domain_cases():
    """op -> Cases without a reference value: theta = pi exactly in log (d = -1 divides by zero), s <= 0, the zero quaternion, NaN / inf entries, singular systems"""
    out = {}
    cs = Cases("sim3_log")
    cs.add("theta=pi about z", [0, 0, 1, 0, 1, 2, 3, 1.5])
    cs.add("theta=pi about x", [1, 0, 0, 0, 1, 2, 3, 1.0])
    cs.add("s=0", [0, 0, 0, 1, 1, 2, 3, 0.0])
    cs.add("s<0", [0.1, 0.2, 0.3, 0.9, 1, 2, 3, -2.0])
    cs.add("zero quaternion", [0, 0, 0, 0, 1, 2, 3, 1.0])
    cs.add("norm 2", [1, 1, 1, 1, 1, 2, 3, 1.0])
    out["sim3_log"] = cs
    cs = Cases("sim3_inv"); cs.add("s=0", [0, 0, 0, 1, 1, 2, 3, 0.0]); out["sim3_inv"] = cs
    cs = Cases("normalize"); cs.add("zero quaternion", [0, 0, 0, 0, 1, 2, 3]); cs.add("NaN", [np.nan, 0, 0, 1, 1, 2, 3]); out["normalize"] = cs
    for op in ("oplus", "oplus_fast"):
        cs = Cases(op)
        cs.add("NaN omega", [np.nan, 0.1, 0.2, 1, 2, 3, 0, 0, 0, 1, 1, 2, 3])
        cs.add("inf omega", [np.inf, 0.1, 0.2, 1, 2, 3, 0, 0, 0, 1, 1, 2, 3])
        cs.add("zero pose quaternion", [0.1, 0.1, 0.2, 1, 2, 3, 0, 0, 0, 0, 1, 2, 3])
        out[op] = cs
    cs = Cases("sim3_exp"); cs.add("NaN sigma", [0.1, 0.2, 0.3, 1, 2, 3, np.nan]); cs.add("sigma=800", [0.1, 0.2, 0.3, 1, 2, 3, 800.0]); out["sim3_exp"] = cs
    cs = Cases("sym3_inv"); cs.add("singular", [1, 1, 1, 1, 1, 1]); out["sym3_inv"] = cs
    cs = Cases("lu3"); cs.add("zero matrix", np.zeros(12)); out["lu3"] = cs
    cs = Cases("R_to_q"); cs.add("NaN entry", [np.nan, 0, 0, 0, 1, 0, 0, 0, 1]); out["R_to_q"] = cs
    return out


_TABLES, _REFS = {}, {}


def cases(op):
    """the in-domain case table of a device op, built once"""
    if op not in _TABLES:
        make = {"sim3_exp": exp_cases, "sim3_log": log_cases, "R_to_q": r_to_q_cases, "huber": huber_cases, "sym3_inv": sym3_cases, "spd6_inv": spd6_cases,
                "lu3": lu3_cases}
        _TABLES[op] = make[op]() if op in make else oplus_cases(op) if op.startswith("oplus") else group_cases(op)
    return _TABLES[op]


def reference(op):
    """the tracked evaluation of cases(op), computed once and shared (callers leave it unchanged)"""
    if op not in _REFS:
        cs = cases(op)
        _REFS[op] = evaluate(op, cs.x, cs.names, cs.forced)
    return _REFS[op]


# ---- the raw libm calls and operations ---------------------------------------------------------------------------------------------------------------------------
_RAW = None


def raw_cases():
    """f -> arguments [n, k].  libm functions: EVERY argument the case tables feed them, recorded while the float64 arithmetic runs over all tables.  sqrt, 1/x, x/y
    and fma: 3000 arguments over twenty decades, fma's with a sum that cancels to 1e-9 of the product."""
    global _RECORD, _RAW
    if _RAW is None:
        _RECORD = {}
        try:
            for op in DEVICE_OPS:
                evaluate(op, cases(op).x, mode="f64")
        finally:
            rec, _RECORD = _RECORD, None
        _RAW = {f: np.unique(np.concatenate(v))[:, None] for f, v in rec.items()}
        _RAW = {f: v[np.isfinite(v[:, 0])] for f, v in _RAW.items()}
        rng = np.random.default_rng(18)
        pos = 10.0 ** rng.uniform(-12, 8, 3000)
        a, b, cc = rng.normal(size=3000) * pos, rng.normal(size=3000), rng.normal(size=3000)
        _RAW.update({"sqrt": pos[:, None], "rcp": a[:, None], "div": np.stack([a, b + np.sign(b)], 1), "fma": np.stack([a, b, -(a * b) + cc * 1e-9 * np.abs(a)], 1)})
    return _RAW


def raw_truth(f, x):
    """long-double value(s) of the libm function f at float64 arguments x[n, 1]: [n, outputs]"""
    a = np.asarray(x, np.float64).astype(LD)[:, 0]
    if f == "sincos":
        return np.stack([np.sin(a), np.cos(a)], 1)
    return {"sin": np.sin, "cos": np.cos, "exp": np.exp, "log": np.log, "acos": np.arccos}[f](a)[:, None]


def ulp_error(got, truth):
    """|got - truth| in units of the spacing of doubles at truth"""
    got, truth = np.asarray(got, np.float64).astype(LD), np.asarray(truth, LD)
    return np.abs(got - truth) / np.spacing(np.abs(truth).astype(np.float64)).astype(LD)


def correctly_rounded_mismatches(f, x, got):
    """how many results of sqrt / rcp / div / fma are NOT the exactly rounded ones (rational arithmetic; no double rounding through long double)"""
    bad = 0
    for row, g in zip(np.asarray(x, np.float64), np.asarray(got, np.float64)):
        g = float(g)
        if f == "sqrt":
            lo, hi = (Fraction(g) + Fraction(float(np.nextafter(g, 0)))) / 2, (Fraction(g) + Fraction(float(np.nextafter(g, np.inf)))) / 2
            bad += not (lo * lo <= Fraction(float(row[0])) <= hi * hi)
        else:
            r = [Fraction(float(v)) for v in row]
            want = 1 / r[0] if f == "rcp" else r[0] / r[1] if f == "div" else r[0] * r[1] + r[2]
            bad += float(want) != g                      # float(Fraction) rounds to nearest even, once
    return bad


# ---- pose graphs for the composition log(C Si Sj^-1) -----------------------------------------------------------------------------------------------------------
def _normalized(v):
    return v / np.linalg.norm(v)


def _sim3_64(o, t, s):
    return np.concatenate([_quat(np.asarray(o, float)), t, [s]])


def _val64(op, x):
    return evaluate(op, np.asarray(x)[None])["val"][0].astype(np.float64)


def four_vertex_graph(kind):
    """Two graphs of four keyframes, vertex 0 fixed, six edges (every pair).
    "wide": rotations of 152 degrees about (nearly) x, y and z next to a small one and scales 1, 1.6, 0.8, 1.25, measurements near the identity: the error
    transform C Si Sj^-1 of every edge turns by 150 - 175 degrees with a scale ratio in 0.5 ... 2.
    "consistent": each measurement is the float64 rounding of the long-double Sj Si^-1, so err is about 0 and its bound is absolute."""
    rng = np.random.default_rng(31 if kind == "wide" else 32)
    if kind == "wide":
        rots = [np.deg2rad(0.5) * _unit(rng)] + [np.deg2rad(152) * _normalized(np.eye(3)[k] + 0.01 * rng.normal(size=3)) for k in range(3)]
        S = [_sim3_64(o, rng.normal(size=3) * 3, s) for o, s in zip(rots, (1.0, 1.6, 0.8, 1.25))]
    else:
        S = [_random_sim3(rng, 2.0) for _ in range(4)]
    S = np.stack(S)
    e_i, e_j, meas = [], [], []
    for i in range(4):
        for j in range(i):
            if kind == "wide":
                m = _sim3_64(np.deg2rad(0.5) * _unit(rng), 0.05 * rng.normal(size=3), float(np.exp(0.03 * rng.normal())))
            else:
                m = _val64("sim3_mul", np.concatenate([S[j], _val64("sim3_inv", S[i])]))
            e_i.append(i); e_j.append(j); meas.append(m)
    fixed = np.zeros(4, np.uint8); fixed[0] = 1
    return dict(sim3=S, fixed=fixed, fix_scale=False, e_i=np.array(e_i, np.int32), e_j=np.array(e_j, np.int32), meas=np.stack(meas), n_vert=4, n_edge=len(e_i))


def pg_errors(pg):
    """tracked log(C Si Sj^-1) of every edge of a pose graph"""
    x = np.concatenate([pg["meas"], pg["sim3"][pg["e_i"]], pg["sim3"][pg["e_j"]]], 1)
    return evaluate("pg_err", x, [f"pg_err/edge{k}({i},{j})" for k, (i, j) in enumerate(zip(pg["e_i"], pg["e_j"]))])
