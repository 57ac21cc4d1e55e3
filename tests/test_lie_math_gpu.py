"""GPU: ba_math.h / sim3_math.h on the device, one lane per item through the test hook ccm_debug_lie_eval (csrc/test_lie_ops.h), against the tracked long-double
reference tests/lie_reference.py — the assertions of tests/test_lie_math_cpu.py on the device's outputs (every output within 1.0 x its running error bound, exact
cases exact, flags), ba_oplus_fast's two claims, the out-of-domain inputs' non-finite positions against the g++ build's, the device's libm measured in ulp,
position independence, and the pose graph's edge errors and initial chi2 through the existing hooks.  DESIGN.md records the printed figures."""
import functools

import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from tests import lie_reference as lr
from tests import test_lie_math_cpu as host
from tests.test_posegraph_gpu import _hub_graph

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53


def _dev(ctx):
    return lambda op, x, out_init=None: optimizer.debug_lie_eval(ctx, op, x, out_init)


@pytest.mark.parametrize("op", lr.DEVICE_OPS)
def test_every_output_within_its_tracked_bound(ctx, op):
    host.check_bounds(_dev(ctx), op)


def test_exact_cases_match_exactly(ctx):
    host.check_exact(_dev(ctx))


def test_spd6_flag_and_untouched_output(ctx):
    host.check_spd6(_dev(ctx))


def test_oplus_fast_bits_outside_and_claims_inside_its_range(ctx):
    """Outside [1e-10, 0.25) the bits of ba_oplus.  Inside (within the series reference's bound: test_every_output_within_its_tracked_bound[oplus_fast]) the two
    claims of the header's comment, measured as tests/host/oplus_check.cpp measures them and held to the bars of tests/test_ba_math_host.py: the largest
    quaternion component difference to ba_oplus < 1e-15, the largest translation difference / (1 + |t|_inf) < 1e-10."""
    ev = _dev(ctx)
    out = host.check_fast_bits(ev)
    cs = lr.cases("oplus_fast")
    a, b = ev(lr.OPS["oplus"][0], cs.x[~out]), ev(lr.OPS["oplus_fast"][0], cs.x[~out])
    dq = np.abs(a[:, :4] - b[:, :4]).max()
    dt = (np.abs(a[:, 4:7] - b[:, 4:7]).max(1) / (1 + np.abs(a[:, 4:7]).max(1))).max()
    print(f"ba_oplus_fast vs ba_oplus on the device, {(~out).sum()} updates in range: quaternion component difference {dq:.3e} ({dq / 2.0 ** -52:.2f} ulp of 1), "
          f"relative translation difference {dt:.3e}")
    assert dq < 1e-15 and dt < 1e-10


def test_out_of_domain_non_finite_positions_equal_the_host_builds(ctx):
    """theta = pi in log, s <= 0, the zero quaternion, NaN / inf entries, singular systems: no reference value; the outputs are non-finite where the g++ build's
    are (NaN signs and payloads differ between the two, positions do not)"""
    dev, cpu = host.nonfinite_positions(_dev(ctx)), host.nonfinite_positions(host.host_eval)
    for op in cpu:
        assert np.array_equal(dev[op], cpu[op]), (op, np.argwhere(dev[op] != cpu[op])[:5])


def test_device_libm_in_ulp_and_exactly_rounded_operations(ctx):
    host.check_raw(_dev(ctx), "device")


@pytest.mark.parametrize("op", ["sim3_log", "sim3_exp", "oplus_fast", "spd6_inv"])
def test_position_independence(ctx, op):
    """the same 65 items alone (n = 1 each), as a batch of 65, and at offsets 191 ... 255 and 256 ... 320 of a batch of 321 (across a workgroup's end): the same bits"""
    ev, cs = _dev(ctx), lr.cases(op)
    x = cs.x[np.linspace(0, len(cs) - 1, 65).astype(int)]
    batch = ev(lr.OPS[op][0], x)
    alone = np.concatenate([ev(lr.OPS[op][0], x[k:k + 1]) for k in range(65)])
    filler = cs.x[np.arange(321) % len(cs)]
    big = []
    for off in (191, 256):
        y = filler.copy(); y[off:off + 65] = x
        big.append(ev(lr.OPS[op][0], y)[off:off + 65])
    for other in [alone] + big:
        assert np.array_equal(batch.view(np.uint64), other.view(np.uint64))


# ---- the pose graph's errors: log(C Si Sj^-1) through ccm_debug_pg_solve, chi2 through ccm_pose_graph_optimize ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pg(name):
    if name == "chain7":
        return synth.make_pose_graph(8, 1, n_loop=1)
    return _hub_graph() if name == "hub" else lr.four_vertex_graph(name)


@pytest.mark.parametrize("name", ["chain7", "hub", "wide", "consistent"])
def test_pose_graph_errors_and_initial_chi2(ctx, name):
    """h["err"] of the hook (max_it = 0: one linearisation) against the tracked composition log(mul(mul(C, Si), inv(Sj))), every component within its bound (for the
    consistent graph err is about 0 and the bound absolute); chi2_initial of the product call against the long-double sum of the hook's err^2 within gamma_{7E+2}
    times that sum (the gamma rule of tests/test_posegraph_pcg_gpu.py: a sum of 7E squares in any order, + 2 for the squares and the reference's own rounding)."""
    pg = _pg(name)
    E = int(pg["e_i"].size)
    h = optimizer.debug_pg_solve(ctx, pg, 1e-16, "jacobi", 1e-10, 0)
    assert np.array_equal(h["active"], np.arange(E))                              # every edge has a free end
    ref = lr.pg_errors(pg)
    assert np.isfinite(ref["bnd"]).all()
    bad = lr.failures(ref, [f"{name}/{k}" for k in range(E)], h["err"])
    print(f"{name}: {E} edges, |err| up to {np.abs(h['err']).max():.3e}, largest error / bound {lr.worst_ratio(ref, h['err']):.3f}")
    assert not bad, bad[:10]
    lab = ref["labels"]
    if name == "wide":
        th = np.linalg.norm(h["err"][:, :3], axis=1)
        assert (th > np.deg2rad(150)).all() and (th < np.deg2rad(175)).all() and (np.abs(h["err"][:, 6]) < np.log(2)).all() and not any(l["d>1-eps"] for l in lab)
    if name == "consistent":
        assert np.abs(h["err"]).max() < 1e-12 and all(l["d>1-eps"] and l["|sigma|<eps"] for l in lab)
    _, st = optimizer.pose_graph_optimization(ctx, pg, max_iters=1)
    want = (h["err"].astype(LD) ** 2).sum()
    n = 7 * E + 2
    assert abs(LD(st.chi2_initial) - want) <= (n * U / (1 - n * U)) * want, (st.chi2_initial, float(want))
