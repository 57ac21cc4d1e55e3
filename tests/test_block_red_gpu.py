"""ccm_slam_amd/csrc/block_red.h and the two untested pieces of lane_xor.h (from_partner_c, wave_min_u32), on their own.

The single-workgroup LM kernels (poseopt.hip, sim3opt.hip) take every decision from sums that BlockRedT hands to all 256 threads; a thread that ended with other
bits would leave a workgroup-uniform branch, and a dropped or mispaired term would only bend the path of an iteration that corrects itself.  The probe
(ccm_debug_block_red) runs in ONE launch, on ONE BlockRedT<4> object with the LDS layout of poseopt_kernel<true>,

    sum1, sum28_lds, sum28_lds, sum1, sum27, sum27, sum64<35>, sum64<35>, sum1

so that the ping-pong phase and the transpose block are reused back to back as in a kernel, and returns what EVERY thread ended with.

  exact data   integers in +-2^30 held in doubles, distinct per (thread, slot): every f64 sum of them is exact in any order (256 terms < 2^38), so each result must
               equal the integer sum bit for bit in all 256 threads.
  order data   standard_normal x 10^(-15 .. 15) with a signed zero, a denormal and a cancelling pair (the choice of tests/test_lane_xor_gpu.py): all threads
               identical, and equal to the numpy transliteration below of the association order block_red.h documents.  The transliteration is checked on the
               CPU, on the exact data, before it is trusted.
"""
import numpy as np
import pytest

from ccm_slam_amd import optimizer

CALLS = optimizer.BLOCK_RED_CALLS
SLOTS = optimizer.BLOCK_RED_SLOTS
N_DATA = {"sum1": 1, "sum28_lds": 28, "sum27": 28, "sum64": 35}   # slots that carry data; the rest of a call's input is zero (sum27, sum64) or garbage (sum28_lds)


# ---- the association order of block_red.h, in numpy (x: [slots, 256], thread t = 64 wave + lane) -------------------------------------------------------------

def _wave_butterfly(x):
    """[..., 64] -> [...]: the xor butterfly 32, 16, 8, 4, 2, 1 (lanex::wave_sum, and what the halving butterflies of sum27 / sum64 compute per value: the lane
    that keeps a value adds its own and its partner's, and f64 addition is commutative, so both lanes of a pair hold the same bits)."""
    for half in (32, 16, 8, 4, 2, 1):
        x = x[..., :half] + x[..., half:2 * half]
    return x[..., 0]


def _waves_in_turn(p):
    """[..., 4] per-wave partials -> ((p0 + p1) + p2) + p3, the loop over the LDS buffer"""
    s = p[..., 0]
    for w in range(1, 4):
        s = s + p[..., w]
    return s


def ref_butterfly(x, n_out):
    """sum1 (one row), sum27 (28 results) and sum64<35> (35): per value the wave butterfly, then the four waves in turn"""
    x = np.asarray(x, np.float64)[:n_out]
    return _waves_in_turn(_wave_butterfly(x.reshape(n_out, 4, 64)))


def ref_sum28_lds(x):
    """sum28_lds: thread 8 v + p adds the columns p, p + 8, ... of value v in four running sums (column 8 i + p goes to sum i mod 4, each started from +0),
    joins them as (s0 + s1) + (s2 + s3), and the 8 parts meet by the xor butterfly 1, 2, 4."""
    x = np.asarray(x, np.float64)[:28]
    cols = x.reshape(28, 32, 8)                       # [value, i, part]: column 8 i + part
    s = np.zeros((4, 28, 8))
    for i in range(32):
        s[i % 4] = s[i % 4] + cols[:, i, :]
    part = (s[0] + s[1]) + (s[2] + s[3])              # [value, part]
    idx = np.arange(8)
    for m in (1, 2, 4):
        part = part + part[:, idx ^ m]
    assert all(np.array_equal(part[:, 0].view(np.uint64), part[:, p].view(np.uint64)) for p in range(8))
    return part[:, 0]


def reference(inputs):
    out = []
    for name, x in zip(CALLS, inputs):
        out.append(ref_sum28_lds(x) if name == "sum28_lds" else ref_butterfly(x, SLOTS[name][1]))
    return out


# ---- data ----------------------------------------------------------------------------------------------------------------------------------------------------

def _pad(name, data, rng):
    """data [N_DATA, 256] -> the call's input [slots, 256]: zeros behind the data (sum27's 28..31, sum64's 35..63), garbage — NaN, infinities, large values —
    in the slots 28..31 that sum28_lds never reads"""
    slots = SLOTS[name][0]
    x = np.zeros((slots, 256))
    x[:data.shape[0]] = data
    if name == "sum28_lds":
        g = rng.standard_normal((4, 256)) * 1e300
        g[0, ::3] = np.nan; g[1, ::5] = np.inf; g[2, ::7] = -np.inf
        x[28:32] = g
    return x


def exact_inputs(seed):
    rng = np.random.default_rng(seed)
    ins, sums = [], []
    for name in CALLS:
        k = N_DATA[name]
        v = np.unique(rng.integers(-2 ** 30, 2 ** 30 + 1, 2 * k * 256))                                 # distinct per (thread, slot)
        v = rng.permutation(v)[:k * 256].reshape(k, 256)
        assert v.size == k * 256
        ins.append(_pad(name, v.astype(np.float64), rng))
        full = np.zeros(SLOTS[name][1])
        full[:k] = v.sum(1).astype(np.float64)        # int64 sums, exact
        sums.append(full)
    return ins, sums


def order_inputs(seed):
    rng = np.random.default_rng(seed)
    ins = []
    for name in CALLS:
        k = N_DATA[name]
        v = rng.standard_normal((k, 256)) * 10.0 ** rng.integers(-15, 15, (k, 256))
        v[:, 3] = 0.0; v[:, 35] = -0.0; v[:, 17] = 5e-324; v[:, 60] = -v[:, 28]; v[:, 200] = -v[:, 71]   # (a pair inside one wave, a pair across waves)
        ins.append(_pad(name, v, rng))
    return ins


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- CPU: the transliteration on the exact data ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_the_transliteration_sums_the_exact_data_exactly(seed):
    ins, sums = exact_inputs(seed)
    for c, (name, got, want) in enumerate(zip(CALLS, reference(ins), sums)):
        assert np.array_equal(_bits(got), _bits(want)), (c, name)
    # and it is order-sensitive: on the order data it differs from a plain numpy sum somewhere (otherwise the order test below would pin nothing)
    ins = order_inputs(seed)
    ref = reference(ins)
    assert any(not np.array_equal(_bits(r), _bits(x[:r.size].sum(1))) for r, x in zip(ref, ins))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_exact_data_every_thread_holds_the_integer_sum(ctx, seed):
    ins, sums = exact_inputs(seed)
    out = optimizer.debug_block_red(ctx, ins)
    for c, (name, got, want) in enumerate(zip(CALLS, out, sums)):
        assert got.shape == (SLOTS[name][1], 256)
        wrong = np.argwhere(_bits(got) != _bits(want)[:, None])
        assert wrong.size == 0, (c, name, "first (value, thread) that differs", wrong[0].tolist(), got[tuple(wrong[0])], want[wrong[0][0]])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_order_data_all_threads_identical_and_in_the_documented_order(ctx, seed):
    ins = order_inputs(seed)
    out = optimizer.debug_block_red(ctx, ins)
    again = optimizer.debug_block_red(ctx, ins)
    for c, (name, got, rep, want) in enumerate(zip(CALLS, out, again, reference(ins))):
        same = _bits(got) == _bits(got)[:, :1]
        assert same.all(), (c, name, "a thread ended with other bits: (value, thread)", np.argwhere(~same)[0].tolist())
        assert np.array_equal(_bits(got[:, 0]), _bits(want)), (c, name, np.flatnonzero(_bits(got[:, 0]) != _bits(want)).tolist())
        assert np.array_equal(_bits(got), _bits(rep)), (c, name, "the repeated launch gave other bits")
        assert np.isfinite(got).all()    # the garbage of sum28_lds' slots 28..31 reached no result


@pytest.mark.gpu
def test_from_partner_c_hands_over_the_partners_bits(ctx):
    rng = np.random.default_rng(3)
    v = rng.standard_normal(64) * 10.0 ** rng.integers(-15, 15, 64)
    v[3] = 0.0; v[35] = -0.0; v[17] = 5e-324; v[60] = -v[28]
    partner, _ = optimizer.debug_lane_ops(ctx, v, np.zeros(64, np.uint32))
    lanes = np.arange(64)
    for k, off in enumerate((1, 2, 4, 8, 16, 32)):
        assert np.array_equal(_bits(partner[k]), _bits(v[lanes ^ off])), f"from_partner_c(v, {off})"


@pytest.mark.gpu
def test_wave_min_u32_is_the_minimum_in_every_lane(ctx):
    rng = np.random.default_rng(4)
    v = np.zeros(64)
    cases = []
    for k in range(64):                                # the unique minimum at lane k
        key = rng.integers(1000, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32)
        key[k] = rng.integers(0, 1000)
        cases.append(key)
    cases.append(np.full(64, 7, np.uint32))            # all lanes equal
    cases.append(np.zeros(64, np.uint32))
    cases.append(np.full(64, 0xFFFFFFFF, np.uint32))
    for lane in (0, 31, 32, 63):                       # the extreme keys against each other
        key = np.full(64, 0xFFFFFFFF, np.uint32); key[lane] = 0
        cases.append(key)
        key = np.full(64, 0xFFFFFFFF, np.uint32); key[lane] = 0xFFFFFFFE
        cases.append(key)
    for i, key in enumerate(cases):
        _, kmin = optimizer.debug_lane_ops(ctx, v, key)
        assert np.array_equal(kmin, np.full(64, key.min(), np.uint32)), (i, key.tolist(), kmin.tolist())
