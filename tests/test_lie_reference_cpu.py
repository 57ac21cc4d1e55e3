"""CPU: the tracked long-double reference tests/lie_reference.py checked on its own — known answers, one truth with tests/lm_reference.py, group identities within
the tracked bound, the series against the closed form, no ambiguous case, and the checker's power: the float64 restatement of the formulas passes as written
and fails, on a NAMED case, with each of the seven planted defects the tests were asked to reject and an eighth, the tie rule of ba_oplus_fast's range."""
import numpy as np
import pytest

from tests import lie_reference as lr
from tests import lm_reference as lmr

LD = np.longdouble
pytestmark = pytest.mark.skipif(not lr.HAVE_EXTENDED, reason="numpy.longdouble is not an extended format here")


def test_r_to_q_known_answers_are_exact():
    cs, ref = lr.cases("R_to_q"), lr.reference("R_to_q")
    for nm, (_, q, branch, exact) in lr.R_TO_Q_KNOWN.items():
        k = cs.index(nm)
        v, q = ref["val"][k], np.array(q, np.float64)
        assert ref["labels"][k]["R2q.branch"] == branch, nm
        if exact:
            assert np.array_equal(v, q.astype(LD)) and not ref["bnd"][k][q == 0].any() and (ref["bnd"][k] < 4 * 2.0 ** -53).all(), nm
        else:   # sqrt(1/2): in long double to its own rounding, the zeros exact and their bound zero
            assert np.array_equal(v[q == 0], q[q == 0].astype(LD)) and not ref["bnd"][k][q == 0].any(), nm
            assert (np.abs(v - np.sign(q) * np.sqrt(LD(0.5)))[q != 0] <= 2 * np.finfo(LD).eps).all() and (ref["bnd"][k][q != 0] < 4 * 2.0 ** -53).all(), nm


def test_one_truth_with_lm_reference():
    """In long double the tracked values ARE tests/lm_reference.py's sim3_exp / sim3_mul / sim3_inv / sim3_map / rot wherever both are defined: lm_reference's exp
    knows the trace branch only, and in the branch theta < eps, |sigma| < eps the header's B is the DOUBLE 1 / 6 while lm_reference divides in long double."""
    cs, ref = lr.cases("sim3_exp"), lr.reference("sim3_exp")
    n = 0
    for k, l in enumerate(ref["labels"]):
        if l["R2q.branch"] != "trace" or (l["theta<eps"] and l["|sigma|<eps"]):
            continue
        assert np.array_equal(lmr.sim3_exp(cs.x[k, :7], LD), ref["val"][k]), cs.names[k]
        n += 1
    assert n > 1200
    for op, f in (("sim3_mul", lambda x: lmr.sim3_mul(x[:8], x[8:16], LD)), ("sim3_inv", lambda x: lmr.sim3_inv(x[:8], LD)),
                  ("sim3_map", lambda x: lmr.sim3_map(x[:8], x[None, 8:11], LD)[0])):
        cs, ref = lr.cases(op), lr.reference(op)
        for k in range(len(cs)):
            assert np.array_equal(f(cs.x[k].astype(LD)), ref["val"][k]), cs.names[k]
    # rot normalises by division first; q_to_R does not normalise: fed the same normalised quaternion the nine entries are equal
    q = lr.cases("q_to_R").x[:, :4].astype(LD)
    qn = q / np.sqrt((q * q).sum(1))[:, None]
    c = lr.Ctx("tracked", list(lr.cases("q_to_R").names), [{}] * len(q))
    R = np.stack([np.broadcast_to(r.v, (len(q),)) for r in lr.q_to_R(c, [lr.T(qn[:, j]) for j in range(4)])], 1)
    for k in range(len(q)):
        assert np.array_equal(lmr.rot(q[k], LD).ravel(), R[k]), k


def _unit_defect(q):
    q = np.asarray(q, np.float64).astype(LD)
    return np.abs((q * q).sum(1) - 1)


def test_group_identities_within_the_tracked_bound():
    """S S^-1 = 1, q_to_R(R_to_q(R)) = R and log(exp(u)) = u for the LONG-DOUBLE values, within the bound the composition carries.  A float64 quaternion is unit
    only to rounding; with delta = |q|^2 - 1 the first two identities hold up to terms worked out from the formulas: q q* = (0, 0, 0, |q|^2), the translation of
    S S^-1 is -4 delta [u]x^2 t, and q_to_R(q) = I + 2 w [u]x + 2 [u]x^2 gives m_ii - m_jj - m_kk + 1 = 4 u_i^2 whatever the norm (the three non-trace branches
    return +-q exactly) and trace + 1 = 4 (w^2 - delta) (the trace branch, w > 1/2: q moves by at most 2 |delta|, R by 4 x that)."""
    rng = np.random.default_rng(5)
    S = np.stack([lr._random_sim3(rng) for _ in range(300)])
    r = lr.evaluate("mul_inv", S)
    d = _unit_defect(S[:, :4])[:, None]
    tn = np.abs(S[:, 4:7]).sum(1).astype(LD)[:, None]
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1], LD)
    slack = np.concatenate([np.zeros((300, 3), LD), d, 4 * d * tn * np.ones((1, 3), LD), np.zeros((300, 1), LD)], 1)
    assert (np.abs(r["val"] - ident) <= r["bnd"] + slack).all()
    assert (r["bnd"][:, :4] < 1e-15).all()                                       # (the bound itself stays a rounding-size number)
    # rotations in every branch of ba_R_to_q
    q = np.stack([lr._quat(th * lr._unit(rng)) for th in np.concatenate([rng.uniform(0, 3.1, 200), rng.uniform(2.2, 3.14, 200)])])
    r = lr.evaluate("R_round_trip", q)
    branches = {l["R2q.branch"] for l in r["labels"]}
    assert branches == {"trace", 0, 1, 2}
    d = _unit_defect(q)[:, None]
    assert (np.abs(r["val"][:, 9:] - r["val"][:, :9]) <= r["bnd"][:, 9:] + 8 * d).all()
    # log(exp(u)) = u where both maps use their closed forms: theta beyond log's small-angle branch (this leaves FACT1's region out: there the small-theta B of
    # g2o is not the exponential's), theta < pi, and sigma = 0 (C = 1 exactly) or |sigma| >= 1e-5
    u = np.stack([np.concatenate([rng.uniform(1.01 * lr.TH_LOG, 3.1) * lr._unit(rng), rng.normal(size=3) * 10.0 ** rng.uniform(-2, 2),
                                  [0.0 if k % 4 == 0 else rng.choice([-1, 1]) * 10.0 ** rng.uniform(-4.9, 0)]]) for k in range(400)])
    assert lr.FACT1[1] <= 1.01 * lr.TH_LOG
    r = lr.evaluate("log_exp", u)
    assert np.isfinite(r["bnd"]).all() and (np.abs(r["val"] - u.astype(LD)) <= r["bnd"]).all()
    assert not any(l["d>1-eps"] or l["theta<eps"] for l in r["labels"])
    # and inside FACT1's region with |sigma| >= 1e-5 the round trip is NOT the identity (parity with the reference's g2o, tests/test_ref_g2o.py)
    u = np.array([[1e-3, 2e-3, -1e-3, 1.0, 2.0, 3.0, 1e-3]])
    r = lr.evaluate("log_exp", u)
    dev = np.abs(r["val"][0, 3:6] - u[0, 3:6].astype(LD)).max()
    assert dev > 0.1 and dev > 1000 * r["bnd"][0, 3:6].max() and r["labels"][0]["d>1-eps"] and not r["labels"][0]["theta<eps"]


def test_series_reference_agrees_with_the_closed_form_reference():
    """ba_oplus_fast's series reference against ba_oplus's closed-form reference over the series' range, within the closed form's bound (the series' truncation,
    < 1e-17 relative, and both long-double evaluations' roundings are far below it)"""
    a, b = lr.reference("oplus"), lr.reference("oplus_fast")
    inside = np.array([l["fast.series"] for l in b["labels"]])
    assert inside.sum() > 400
    assert (np.abs(a["val"][inside] - b["val"][inside]) <= a["bnd"][inside]).all()
    assert np.array_equal(a["val"][~inside], b["val"][~inside]) and np.array_equal(a["bnd"][~inside], b["bnd"][~inside])


@pytest.mark.parametrize("op", lr.DEVICE_OPS)
def test_every_case_is_unambiguous_or_carries_its_branch(op):
    ref = lr.reference(op)                                                         # raises Ambiguous / PlantedBranchWrong with the case's name otherwise
    assert np.isfinite(ref["bnd"][ref["ok"]]).all() and all(l is not None for l in ref["labels"])
    for cs in [c for o, c in lr.out_of_domain_cases().items() if o == op]:
        assert len(cs) and not set(cs.names) & set(lr.cases(op).names)             # listed separately, no reference value


def test_a_threshold_case_without_its_branch_is_refused():
    cs = lr.cases("sim3_exp")
    k = cs.index("theta=eps,sigma=0,ups=1")
    with pytest.raises(lr.Ambiguous, match="theta=eps,sigma=0,ups=1: theta<eps"):
        lr.evaluate("sim3_exp", cs.x[k:k + 1], [cs.names[k]])
    k = cs.index("theta=1,sigma=0,ups=1")
    with pytest.raises(lr.PlantedBranchWrong):
        lr.evaluate("sim3_exp", cs.x[k:k + 1], [cs.names[k]], [{"theta<eps": True}])
    cs = lr.cases("spd6_inv")
    k = cs.index("zero pivot 3")
    with pytest.raises(lr.Ambiguous):
        lr.evaluate("spd6_inv", cs.x[k:k + 1], [cs.names[k]])


# (defect, op, the case that must fail)
DEFECTS = [("a", "R_to_q", "i1 generic 150deg"),             # j and k swapped in the i == 1 case: qw changes sign
           ("b", "R_to_q", "pi about (1,-1,0)"),             # the tie rule >= instead of >: i = 1, the quaternion changes sign
           ("c", "sim3_exp", "theta=1,sigma=0,ups=1"),       # the |sigma| < eps test dropped: 0 / 0
           ("d", "sim3_exp", "theta=1,sigma=+eps+,ups=1"),   # C = 1 used just above eps: 5e-6 relative in the translation
           ("e", "oplus_fast", "theta2 below 0.25,ups=1"),   # one Horner coefficient off by 1e-12 relative
           ("f", "lu3", "zero second pivot"),                # the second pivot not taken: a division by zero
           ("g", "sim3_log", "theta=2,sigma=0,t=1"),         # acos with 64 ulp of error
           ("h", "oplus_fast", "theta2 at 1e-10,ups=1e3")]   # > instead of >= at theta^2 == 1e-10: the closed form's cancellation, 1e-11 relative in the translation


@pytest.mark.parametrize("op", lr.DEVICE_OPS)
def test_float64_restatement_passes_as_written(op):
    cs, ref = lr.cases(op), lr.reference(op)
    got = lr.evaluate(op, cs.x, cs.names, mode="f64")
    assert np.array_equal(got["ok"], ref["ok"]) and not lr.failures(ref, cs.names, got["val"])
    for k in range(len(cs)):                                                       # through the same branches, every case
        assert got["labels"][k] == ref["labels"][k], cs.names[k]


@pytest.mark.parametrize("defect,op,name", DEFECTS)
def test_checker_rejects_the_planted_defect_on_its_named_case(defect, op, name):
    cs, ref = lr.cases(op), lr.reference(op)
    got = lr.evaluate(op, cs.x, cs.names, mode="f64", defect=defect)
    failed = {f[0] for f in lr.failures(ref, cs.names, got["val"])}
    assert f"{op}/{name}" in failed, sorted(failed)[:10]
    if defect == "a":
        assert ref["labels"][cs.index(name)]["R2q.branch"] == 1
