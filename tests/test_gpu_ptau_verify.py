"""zkmi_ptau_section_check on the device (csrc/ptau_verify.hip; snarkjs_amd/powersoftau_verify.py) against the CPU oracle's literal restatement of
processSection and verifyLagrangeEvaluations (tests/ptau_verify_vectors.py): both curves and both groups, sections of 1, 2, 3, 127 and 128 points, ladders of
top 0, 1 and 7 with and without the zeroed last term, pages that split a point, a point at infinity inside the section, one wrong Lagrange point per power,
guard bytes behind every output, the refusal of top > Fr.s and of a call while a pipeline slot holds work; and the driver, powersoftau_verify.verify, on every
case of tests/golden/ptau_verify_golden.json with the reference's verdict and lines."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
import ptau_verify_vectors as P
from snarkjs_amd import powersoftau_verify as tv
from snarkjs_amd import zkmi

pytestmark = pytest.mark.gpu
GUARD = 64                                         # bytes behind every output, which must come back untouched
# (top, zero_last, n_tau): every top with both rules, and sections longer than the ladder needs
LADDERS = [(0, False, 1), (0, True, 1), (1, False, 2), (1, True, 1), (1, False, 3), (7, False, 128), (7, True, 127), (7, True, 128)]


def raw_call(cv, group, tau_pages, n_tau, lag_pages, top, zero_last, u_split=None, expect=0):
    """the entry point itself, every output with guard bytes behind it and u_out in two pages when u_split is given -> (u, r1 jac, r2 jac, ladder int8)"""
    sg, jac = P.point_size(cv, group), 3 * group * cv["n8q"]
    nb = n_tau * sg
    cuts = [nb] if u_split is None else [u_split, nb - u_split]
    u_bufs = [np.full(k + GUARD, 0xAB, np.uint8) for k in cuts]
    r1, r2, lad = (np.full(k + GUARD, 0xAB, np.uint8) for k in (jac, jac, top + 1))
    pt = zkmi.pages_of(tau_pages)
    pl = zkmi.pages_of(lag_pages) if lag_pages is not None else None
    u_ptr, u_len = (C.c_void_p * len(cuts))(*[b.ctypes.data for b in u_bufs]), (C.c_size_t * len(cuts))(*cuts)
    rc = zkmi.lib().zkmi_ptau_section_check(cv["id"], group, pt.pages, n_tau, C.byref(pl.pages) if pl else None, top, int(zero_last), tv._seed(P.PAIR_SEED), tv._seed(P.LADDER_SEED),
                                            u_ptr, u_len, len(cuts), zkmi.ptr(r1), zkmi.ptr(r2), zkmi.ptr(lad))
    assert rc == expect, zkmi.lib().zkmi_last_error()
    for b, k in zip(u_bufs + [r1, r2, lad], cuts + [jac, jac, top + 1]):
        assert (b[k:] == 0xAB).all(), "wrote behind an output"
    if rc:
        for b in u_bufs + [r1, r2, lad]:
            assert (b == 0xAB).all(), "a refused call wrote to an output"
        return None
    return b"".join(b[:k].tobytes() for b, k in zip(u_bufs, cuts)), r1[:jac], r2[:jac], lad[:top + 1].view(np.int8)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_sections_without_lagrange_points(curve, group):
    zkmi.init()
    cv = P.curve_record(curve)
    sg, dev, ref = P.point_size(cv, group), tv.Device(), P.OracleDevice()
    for n in (1, 2, 3, 127, 128):
        tau = P.tau_points(cv, group, n, inf_at=3)
        want = ref.section_check(cv, group, tau, n, None, 0, False, P.PAIR_SEED, P.LADDER_SEED)
        assert dev.section_check(cv, group, tau, n, None, 0, False, P.PAIR_SEED, P.LADDER_SEED) == want, n
        assert want[3] is None and (n > 1) == any(want[1]) == any(want[2])
        # pages that split a point on the way in and on the way out, more bytes than n points, guard bytes behind every output
        cut = 5 * sg + 7 if n > 5 else 9
        u, r1, r2, lad = raw_call(cv, group, [tau[:cut], tau[cut:] + bytes(30)], n, None, 0, False, u_split=min(n * sg - 1, 3 * sg + 11))
        assert (u, orc.to_affine(cv["id"], group, r1).tobytes(), orc.to_affine(cv["id"], group, r2).tobytes()) == want[:3], n
        assert (lad.view(np.uint8) == 0xAB).all(), "no ladder was asked for"
    u, r1, r2, _ = raw_call(cv, group, b"", 0, None, 0, False)
    assert u == b"" and not r1.any() and not r2.any(), "an empty section: both sums are infinity"
    raw_call(cv, group, tau[:-1], 128, None, 0, False, expect=2)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_ladders(curve, group):
    zkmi.init()
    cv = P.curve_record(curve)
    sg, dev, ref = P.point_size(cv, group), tv.Device(), P.OracleDevice()
    for top, zero_last, n in LADDERS:
        tau = P.tau_points(cv, group, n, inf_at=3)
        lag = P.lagrange_of(cv, group, tau, top, zero_last)
        want = ref.section_check(cv, group, tau, n, lag, top, zero_last, P.PAIR_SEED, P.LADDER_SEED)
        assert want[3] == [True] * (top + 1)
        cut = len(lag) // 2 + 5
        assert dev.section_check(cv, group, tau, n, [lag[:cut], lag[cut:]], top, zero_last, P.PAIR_SEED, P.LADDER_SEED) == want, (top, zero_last, n)
    u, r1, r2, lad = raw_call(cv, group, tau, n, lag, top, zero_last, u_split=sg + 1)
    assert u == want[0] and lad.tolist() == [1] * (top + 1)
    # too few points for the ladder, in either section
    raw_call(cv, group, tau, 126, lag, 7, True, expect=2)
    raw_call(cv, group, tau, n, lag[:-1], 7, True, expect=2)


@pytest.mark.parametrize("zero_last", [False, True])
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_one_wrong_lagrange_point_fails_exactly_its_power(curve, group, zero_last):
    zkmi.init()
    cv = P.curve_record(curve)
    sg, top, dev = P.point_size(cv, group), 7, tv.Device()
    n = 128 - (1 if zero_last else 0)
    tau = P.tau_points(cv, group, n)
    lag = P.lagrange_of(cv, group, tau, top, zero_last)
    other = tau[5 * sg:6 * sg]
    for p, i in ((0, 0), (3, 6), (top, 127), (top, 0)):
        at = ((1 << p) - 1 + i) * sg
        bad = lag[:at] + other + lag[at + sg:]
        assert bad != lag and len(bad) == len(lag)
        want = [q != p for q in range(top + 1)]
        assert P.OracleDevice().section_check(cv, group, tau, n, bad, top, zero_last, P.PAIR_SEED, P.LADDER_SEED)[3] == want, (p, i)
        assert dev.section_check(cv, group, tau, n, bad, top, zero_last, P.PAIR_SEED, P.LADDER_SEED)[3] == want, (p, i)


def test_top_beyond_the_two_adicity_is_refused_without_touching_the_device():
    zkmi.init()
    for curve in P.CURVES:
        cv = P.curve_record(curve)
        tau = P.tau_points(cv, 1, 2)
        # a Lagrange section far too short for 2^(s + 2) - 1 points: the refusal comes before any length is looked at, and nothing is allocated or written
        raw_call(cv, 1, tau, 2, tau, cv["s"] + 1, True, expect=4)
        assert b"top > Fr.s" in zkmi.lib().zkmi_last_error()
        raw_call(cv, 1, tau, 2, None, cv["s"] + 1, True, expect=4)
        raw_call(cv, 3, tau, 2, None, 1, False, expect=2)


def test_a_busy_pipeline_slot_refuses_the_call_and_keeps_its_work():
    zkmi.init()
    L, c, n = zkmi.lib(), orc.BN128, 64
    cv = P.curve_record("bn128")
    pts = orc.geom_bases(c, 1, n)
    sc = np.frombuffer(b"".join(((i * 0x9e3779b97f4a7c15 + 5) % (1 << 250)).to_bytes(32, "little") for i in range(n)), np.uint8).copy()
    d_pts, d_sc = zkmi.DeviceBuffer.from_host(pts), zkmi.DeviceBuffer.from_host(sc)
    tab = C.c_uint64()
    zkmi.check(L.zkmi_msm_table_build(c, 1, d_pts.ptr, n, C.byref(tab)))
    tau = P.tau_points(cv, 1, 2)
    lag = P.lagrange_of(cv, 1, tau, 1, False)
    try:
        zkmi.check(L.zkmi_pipeline_select(0))
        zkmi.check(L.zkmi_msm_table_multi_enqueue_dev(tab.value, (C.c_void_p * 1)(d_sc.ptr), (C.c_size_t * 1)(n), 1, 32))
        with pytest.raises(zkmi.ZkmiError, match="ptau_section_check: a pipeline slot holds work in flight"):
            tv.Device().section_check(cv, 1, tau, 2, lag, 1, False, P.PAIR_SEED, P.LADDER_SEED)
        raw_call(cv, 1, tau, 2, lag, 1, False, expect=2)
        out = np.zeros(3 * 32, np.uint8)
        zkmi.check(L.zkmi_msm_table_multi_collect(tab.value, 1, zkmi.ptr(out)))
        assert orc.to_affine(c, 1, out).tobytes() == orc.to_affine(c, 1, orc.msm(c, 1, pts, sc, n)).tobytes(), "the pending MSM was disturbed"
        assert tv.Device().section_check(cv, 1, tau, 2, lag, 1, False, P.PAIR_SEED, P.LADDER_SEED)[3] == [True, True]
    finally:
        L.zkmi_msm_table_release(tab.value)
        d_pts.free(); d_sc.free()


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_the_driver_on_every_golden_case(case):
    """the reference's verdict or refusal and its lines (tests/test_ptau_verify_host.py pins the same for the CPU driver), through the kernels"""
    log, raw = P.Log(), P.case_file(case)
    if "throws" in case:
        with pytest.raises(tv.PtauError, match=r"^ptau: Invalid File format$"):
            tv.verify(raw, log, P.RANDOM32)
        return
    assert tv.verify(raw, log, P.RANDOM32) is case["verdict"]
    assert log.lines == P.case_lines(case)


@pytest.mark.parametrize("curve", P.CURVES)
def test_the_driver_from_a_path_with_fresh_randomness_and_no_logger(curve):
    import os
    assert tv.verify(os.path.join(P.GOLDEN, f"ptau_{curve}_p6_c3b.ptau")) is True
    swapped = next(c for c in P.CASES if c["curve"] == curve and "section 12" in c["label"])
    assert tv.verify(P.case_file(swapped)) is False
