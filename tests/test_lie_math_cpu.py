"""CPU: ccm_slam_amd/csrc/test_lie_ops.h (one entry to every function of ba_math.h / sim3_math.h) compiled with g++ -O2 -ffp-contract=off, against the tracked
long-double reference tests/lie_reference.py: every output of every in-domain case within 1.0 x its running error bound, the exact cases exact, ba_spd6_inv's flag
and untouched output, ba_oplus_fast's bits outside its range, glibc's libm under the charges of LIBM_ULP, and tests/host/lie_check.cpp under the address and
undefined-behaviour sanitizers as a stand-alone program.  The check_* functions take the evaluator, so that tests/test_lie_math_gpu.py asserts the same of the
device's outputs.

    python -m tests.test_lie_math_cpu        prints the largest error / bound per op and glibc's ulp errors (DESIGN.md records them)
"""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import lie_reference as lr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = r'''
#include "%s/ccm_slam_amd/csrc/test_lie_ops.h"
extern "C" int lie_eval_host(int op, int n, const double* in, double* out) {
  for (int i = 0; i < n; i++) if (!lie_eval(op, in + (long)kLieIn * i, out + (long)kLieOut * i)) return 1;
  return 0;
}
''' % ROOT
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def _lib():
    d = tempfile.mkdtemp()
    src, so = os.path.join(d, "lie.cpp"), os.path.join(d, "lie.so")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so, "-lm"])
    return C.CDLL(so)


def host_eval(op, x, out_init=None):
    """lie_eval of the g++ build over x[n, 48] -> out[n, 40]"""
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros((x.shape[0], lr.N_OUT)) if out_init is None else np.ascontiguousarray(out_init, np.float64).copy()
    assert x.shape[1] == lr.N_IN and _lib().lie_eval_host(int(op), int(x.shape[0]), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
    return out


# ---- the assertions, shared with the GPU test ----------------------------------------------------------------------------------------------------------------
def check_bounds(ev, op):
    """every output of every in-domain case within 1.0 x the tracked bound (a zero bound: equal); every output slot beyond the op's own and the flag untouched.
    Returns the largest error / bound."""
    cs, ref = lr.cases(op), lr.reference(op)
    m = lr.OPS[op][2]
    got = ev(lr.OPS[op][0], cs.x, np.full((len(cs), lr.N_OUT), SENTINEL))
    assert np.isfinite(ref["bnd"][ref["ok"]]).all() and np.isfinite(ref["val"][ref["ok"]].astype(np.float64)).all()
    bad = lr.failures(ref, cs.names, got)
    ratio = lr.worst_ratio(ref, got)
    print(f"{op}: {len(cs)} cases, largest error / bound {ratio:.3f}")
    assert not bad, bad[:10]
    assert (got[:, m:lr.FLAG] == SENTINEL).all()
    assert np.array_equal(got[:, lr.FLAG], ref["ok"].astype(np.float64))
    return ratio


def check_exact(ev):
    """ba_R_to_q's known answers: the representable ones bit for bit, sqrt(1/2) within an ulp with exact zeros; ba_huber's inliers untouched"""
    cs = lr.cases("R_to_q")
    got = ev(lr.OPS["R_to_q"][0], cs.x)
    for nm, (_, q, _, exact) in lr.R_TO_Q_KNOWN.items():
        g, q = got[cs.index(nm), :4], np.array(q, np.float64)
        if exact:
            assert np.array_equal(g, q), (nm, g)
        else:
            assert np.array_equal(g[q == 0], q[q == 0]) and np.array_equal(np.sign(g), np.sign(q)) and (np.abs(g - q) <= np.spacing(np.abs(q))).all(), (nm, g)
    cs, ref = lr.cases("huber"), lr.reference("huber")
    got = ev(lr.OPS["huber"][0], cs.x)
    inl = np.array([bool(l.get("huber.delta<=0")) or bool(l.get("huber.inlier")) for l in ref["labels"]])
    assert inl.sum() >= 20 and np.array_equal(got[inl, 0], cs.x[inl, 0]) and (got[inl, 1] == 1).all()
    assert not inl[cs.index("delta=sqrt5.991,e2=next above dsqr")] and inl[cs.index("delta=sqrt5.991,e2=dsqr")]
    cs = lr.cases("normalize")
    got = ev(lr.OPS["normalize"][0], cs.x)
    k = cs.index("qw=-0.0")
    assert got[k, 3] == 0 and np.signbit(got[k, 3]) and got[k, 0] > 0            # -0.0 < 0 is false: nothing is negated
    assert np.array_equal(got[:, 4:7], cs.x[:, 4:7])                                # the translation passes through
    # the header's claim: one reciprocal and four products differ from Eigen's four divisions by at most 1 ulp per component
    q = np.where(cs.x[:, 3:4] < 0, -cs.x[:, :4], cs.x[:, :4])
    eig = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    assert (np.abs(got[:, :4] - eig) <= np.spacing(np.abs(eig))).all()


def check_spd6(ev):
    cs, ref = lr.cases("spd6_inv"), lr.reference("spd6_inv")
    got = ev(lr.OPS["spd6_inv"][0], cs.x, np.full((len(cs), lr.N_OUT), SENTINEL))
    false = [cs.index(n) for n in lr.SPD6_FALSE]
    assert sorted(np.flatnonzero(got[:, lr.FLAG] == 0)) == sorted(false) == sorted(np.flatnonzero(~ref["ok"]))
    assert (got[false, :36] == SENTINEL).all()                                      # Inv untouched on a false return
    ok = ref["ok"]
    assert np.array_equal(got[ok, :36].reshape(-1, 6, 6), got[ok, :36].reshape(-1, 6, 6).transpose(0, 2, 1))


def fast_outside(ref):
    return np.array([not l["fast.series"] for l in ref["labels"]])


def check_fast_bits(ev):
    """outside [1e-10, 0.25) ba_oplus_fast IS ba_oplus: the same bits (the planted squares next to both ends, a NaN and an infinite omega included); theta^2 == 1e-10
    exactly takes the series (the header's >=) and 0.25 exactly does not"""
    cs, ref = lr.cases("oplus_fast"), lr.reference("oplus_fast")
    assert np.array_equal(cs.x, lr.cases("oplus").x)
    out = fast_outside(ref)
    for nm, series in (("theta2 below 1e-10", False), ("theta2 at 1e-10", True), ("theta2 above 1e-10", True), ("theta2 below 0.25", True), ("theta2 at 0.25", False), ("theta2 above 0.25", False),
                       ("theta=0.5-", True), ("theta=0.5", False), ("theta=eps", True), ("theta=eps-", False), ("theta=0", False)):
        assert out[cs.index(nm + ",ups=1")] == (not series), nm
    a, b = ev(lr.OPS["oplus"][0], cs.x[out]), ev(lr.OPS["oplus_fast"][0], cs.x[out])
    assert out.sum() > 200 and (~out).sum() > 400 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # a NaN or infinite omega fails both range tests: the same call, so the same bits, NaN payloads included
    ood = lr.out_of_domain_cases()
    assert np.array_equal(ood["oplus"].x, ood["oplus_fast"].x, equal_nan=True)
    k = [ood["oplus"].index("NaN omega"), ood["oplus"].index("inf omega")]
    a, b = ev(lr.OPS["oplus"][0], ood["oplus"].x[k]), ev(lr.OPS["oplus_fast"][0], ood["oplus"].x[k])
    assert np.isnan(a[:, :7]).all() and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    return out


def nonfinite_positions(ev):
    """op -> bool[n, 40]: where the outputs of the out-of-domain cases are not finite"""
    return {op: ~np.isfinite(ev(lr.OPS[op][0], cs.x)) for op, cs in lr.out_of_domain_cases().items()}


def check_raw(ev, what):
    """libm: the largest ulp error over every argument the case tables feed each function, asserted <= LIBM_ULP / 2; sqrt, 1/x, x/y, fma: exactly rounded"""
    raw, worst = lr.raw_cases(), {}
    for f, op in lr.RAW_OPS.items():
        x = np.zeros((raw[f].shape[0], lr.N_IN)); x[:, :raw[f].shape[1]] = raw[f]
        got = ev(op, x)
        if f in lr.LIBM_ULP:
            k = 2 if f == "sincos" else 1
            worst[f] = float(lr.ulp_error(got[:, :k], lr.raw_truth(f, raw[f])).max())
            print(f"{what} {f}: {raw[f].shape[0]} arguments in [{raw[f].min():.3g}, {raw[f].max():.3g}], largest error {worst[f]:.3f} ulp (charge {lr.LIBM_ULP[f]})")
        else:
            worst[f] = lr.correctly_rounded_mismatches(f, raw[f], got[:, 0])
            print(f"{what} {f}: {raw[f].shape[0]} arguments, {worst[f]} not exactly rounded")
    for f, w in worst.items():
        assert w <= lr.LIBM_ULP[f] / 2 if f in lr.LIBM_ULP else w == 0, (f, w)
    return worst


def planted_label_mismatches():
    """the reference's branch labels against what the tables plant: a list of (case, label, got)"""
    bad = []

    def want(op, name, label, value):
        l = lr.reference(op)["labels"][lr.cases(op).index(name)]
        if l.get(label) != value:
            bad.append((f"{op}/{name}", label, l.get(label)))
    for op in ("sim3_exp", "oplus"):
        tail = ",sigma=0,ups=1" if op == "sim3_exp" else ",ups=1"
        for nm, th in lr.THETAS_EDGE.items():
            want(op, f"theta={nm}{tail}", "theta<eps", th < lr.EPS)
        want(op, f"theta=2pi/3-{tail}", "R2q.branch", "trace")
        for ax in range(3):
            want(op, f"theta=2pi/3+,axis{'xyz'[ax]}{tail}", "R2q.branch", ax)
            want(op, f"theta=pi-1e-4,axis{'xyz'[ax]}{tail}", "R2q.branch", ax)
    for sn, sg in lr.SIGMAS.items():
        for tn in ("eps-", "eps", "1"):
            want("sim3_exp", f"theta={tn},sigma={sn},ups=1", "|sigma|<eps", abs(sg) < lr.EPS)
    for tn, small in (("thlog-", True), ("thlog+", False), ("1e-3", True), ("0.1", False)):
        for sn, ss in (("+eps(1-1e-9)", True), ("+eps(1+1e-9)", False), ("-eps(1-1e-9)", True), ("-eps(1+1e-9)", False), ("0", True), ("2", False)):
            want("sim3_log", f"theta={tn},sigma={sn},t=1", "d>1-eps", small)
            want("sim3_log", f"theta={tn},sigma={sn},t=1", "|sigma|<eps", ss)
    for nm, (_, _, br, _) in lr.R_TO_Q_KNOWN.items():
        want("R_to_q", nm, "R2q.branch", br)
    for p in lr.LU3_ORDERS:
        for ce in (0, 3, 6, 9, 12):
            for k in range(6):
                want("lu3", f"order=({p[0]},{p[1]}),cond~1e{ce},#{k}", "lu3.order", p)
    for nm, (_, order) in lr.LU3_TIES.items():
        want("lu3", nm, "lu3.order", order)
    return bad


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------------------------
pytestmark = pytest.mark.skipif(not lr.HAVE_EXTENDED, reason="numpy.longdouble is not an extended format here")


@pytest.mark.parametrize("op", lr.DEVICE_OPS)
def test_every_output_within_its_tracked_bound(op):
    check_bounds(host_eval, op)


def test_branch_labels_are_as_planted():
    assert planted_label_mismatches() == []


def test_exact_cases_match_exactly():
    check_exact(host_eval)


def test_spd6_flag_and_untouched_output():
    check_spd6(host_eval)


def test_oplus_fast_is_oplus_bit_for_bit_outside_its_range():
    check_fast_bits(host_eval)


def test_out_of_domain_inputs_give_non_finite_outputs_where_expected():
    """no reference value here: only WHERE the g++ build's outputs are not finite is recorded (the GPU test compares the device's positions with these)"""
    nf = nonfinite_positions(host_eval)
    ood = lr.out_of_domain_cases()
    log = ood["sim3_log"]
    assert nf["sim3_log"][log.index("theta=pi about z"), :3].all()                 # acos(-1) / (2 sqrt(0)) times a zero difference
    assert nf["sim3_log"][log.index("s=0"), 6] and nf["sim3_log"][log.index("s<0"), 6]
    assert nf["normalize"][0, :4].all() and not nf["normalize"][0, 4:7].any()
    assert nf["oplus_fast"][0, :7].all() and np.array_equal(nf["oplus"], nf["oplus_fast"])
    assert all(v[:, lr.FLAG].sum() == 0 for v in nf.values())


def test_glibc_stays_below_the_libm_charges():
    check_raw(host_eval, "glibc")


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/host/lie_check.cpp over every case, the out-of-domain ones included, each item in heap blocks of exactly 48 and 40 doubles"""
    blocks = [(lr.OPS[op][0], lr.OPS[op][2], lr.cases(op).x) for op in lr.DEVICE_OPS] + [(lr.OPS[op][0], lr.OPS[op][2], cs.x) for op, cs in lr.out_of_domain_cases().items()]
    raw = lr.raw_cases()
    for f, op in lr.RAW_OPS.items():
        x = np.zeros((raw[f].shape[0], lr.N_IN)); x[:, :raw[f].shape[1]] = raw[f]
        blocks.append((op, 2 if f == "sincos" else 1, x))
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([len(blocks)], np.int32).tobytes())
        for op, n_out, x in blocks:
            fh.write(np.array([op, n_out, x.shape[0]], np.int32).tobytes()); fh.write(np.ascontiguousarray(x, np.float64).tobytes())
    exe = tmp_path / "lie_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                    "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "lie_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    m = re.search(r"lie ops ok: (\d+) blocks, (\d+) items", r.stdout)
    assert r.returncode == 0 and m and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    assert int(m.group(1)) == len(blocks) and int(m.group(2)) == sum(b[2].shape[0] for b in blocks)


if __name__ == "__main__":
    for op_ in lr.DEVICE_OPS:
        check_bounds(host_eval, op_)
    check_raw(host_eval, "glibc")
