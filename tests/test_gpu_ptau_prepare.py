"""zkmi_ptau_lagrange_section / _dev on the device (csrc/ptau_lagrange.cuh; snarkjs_amd/powersoftau_prepare.py) against the CPU oracle's G.ifft power by power
(ptau_verify_vectors.lagrange_of): both curves and both groups, ladders of top 0, 1, 2, 5, 6 and 7 (the slots per twiddle pass the width of a wave only at 6
and 7) with and without the zeroed last point, whole (first = 0) and the top block alone (first = top), top = 8 as the first grid of more than one block per
stage; infinity at the front, in the middle and everywhere, and one point repeated (the doubling and the cancelling case of the butterfly's addition); pages
that split a point, guard bytes, the resident form, each block against zkmi_group_fft_dev of its prefix; the refusals; and the drivers prepare_phase2 and
convert on the committed files, byte for byte (tests/test_ptau_prepare_host.py pins the same with the oracle in place of the device)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as orc
import ptau_verify_vectors as P
from snarkjs_amd import powersoftau_prepare as tp
from snarkjs_amd import powersoftau_verify as tv
from snarkjs_amd import zkmi
from test_ptau_prepare_host import check_truncation_case, without_top_block

pytestmark = pytest.mark.gpu
GUARD = 64                                         # bytes behind every output page, which must come back untouched
TOPS = (0, 1, 2, 5, 6, 7)
_want = {}


def want_of(cv, group, tau, top, zero_last, first=0):
    """the oracle's ladder, computed once per input and shared by the tests"""
    k = (cv["name"], group, tau, top, zero_last)
    if k not in _want:
        _want[k] = P.lagrange_of(cv, group, tau, top, zero_last)
    return _want[k][((1 << first) - 1) * P.point_size(cv, group):]


def n_out(first, top):
    return (2 << top) - (1 << first)


def raw_call(cv, group, tau_pages, n_tau, first, top, zero_last, out_cuts=None, expect=0):
    """the paged entry point itself, guard bytes behind every output page -> the output bytes (None when refused)"""
    nb = n_out(first, top) * P.point_size(cv, group) if first <= top and top < 20 else 64
    cuts = [nb] if out_cuts is None else list(out_cuts) + [nb - sum(out_cuts)]
    bufs = [np.full(k + GUARD, 0xAB, np.uint8) for k in cuts]
    pt = zkmi.pages_of(tau_pages)
    o_ptr, o_len = (C.c_void_p * len(cuts))(*[b.ctypes.data for b in bufs]), (C.c_size_t * len(cuts))(*cuts)
    rc = zkmi.lib().zkmi_ptau_lagrange_section(cv["id"], group, pt.pages, n_tau, first, top, int(zero_last), o_ptr, o_len, len(cuts))
    assert rc == expect, zkmi.lib().zkmi_last_error()
    for b, k in zip(bufs, cuts):
        assert (b[k:] == 0xAB).all(), "wrote behind an output page"
    if rc:
        for b in bufs:
            assert (b == 0xAB).all(), "a refused call wrote to an output"
        return None
    return b"".join(b[:k].tobytes() for b, k in zip(bufs, cuts))


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_ladders_against_the_oracle(curve, group):
    zkmi.init()
    cv, dev = P.curve_record(curve), tp.Device()
    for top in TOPS:
        for zero_last in (False, True):
            n = (1 << top) - (1 if zero_last else 0)
            tau = P.tau_points(cv, group, n)
            for first in sorted({0, top}):
                assert dev.lagrange_section(cv, group, tau, n, first, top, zero_last) == want_of(cv, group, tau, top, zero_last, first), (top, zero_last, first)


def test_more_than_one_block_of_lanes_per_stage():
    zkmi.init()
    cv = P.curve_record("bn128")
    tau = orc.geom_bases(orc.BN128, 1, 256).tobytes()
    got = tp.Device().lagrange_section(cv, 1, tau, 256, 0, 8, False)
    assert got == want_of(cv, 1, tau, 8, False)
    assert tp.Device().lagrange_section(cv, 1, tau[:255 * 64], 255, 8, 8, True) == want_of(cv, 1, tau[:255 * 64], 8, True, 8)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_points_at_infinity_and_one_point_repeated(curve, group):
    zkmi.init()
    cv, dev, top, n = P.curve_record(curve), tp.Device(), 5, 32
    sg = P.point_size(cv, group)
    for label, tau in (("infinity at index 0", P.tau_points(cv, group, n, inf_at=0)), ("infinity in the middle", P.tau_points(cv, group, n, inf_at=13)),
                       ("all points at infinity", bytes(n * sg))):
        for zero_last in (False, True):
            m = n - (1 if zero_last else 0)
            assert dev.lagrange_section(cv, group, tau[:m * sg], m, 0, top, zero_last) == want_of(cv, group, tau[:m * sg], top, zero_last), (label, zero_last)
    assert dev.lagrange_section(cv, group, bytes(n * sg), n, 0, top, False) == bytes(63 * sg)
    # the same point 32 times: every butterfly of the first stage adds a point to itself and to its negative; the transform of a constant is the constant, then zeros
    one = P.tau_points(cv, group, 2)[sg:]
    got = dev.lagrange_section(cv, group, one * n, n, 0, top, False)
    assert got == b"".join(one + bytes(((1 << p) - 1) * sg) for p in range(top + 1))
    assert got == want_of(cv, group, one * n, top, False)


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_pages_guards_the_resident_form_and_the_single_transforms(curve, group):
    zkmi.init()
    L, cv, top = zkmi.lib(), P.curve_record(curve), 7
    sg = P.point_size(cv, group)
    for zero_last, first in ((True, 0), (False, 0), (True, top)):
        n = 128 - (1 if zero_last else 0)
        tau = P.tau_points(cv, group, n, inf_at=3)
        want = want_of(cv, group, tau, top, zero_last, first)
        # pages that split a point on the way in and on the way out, more bytes than n points in
        cut = 5 * sg + 7
        assert raw_call(cv, group, [tau[:cut], tau[cut:] + bytes(30)], n, first, top, zero_last, out_cuts=[3 * sg + 11, sg - 1]) == want
        d_tau, d_out = zkmi.DeviceBuffer.from_host(np.frombuffer(tau, np.uint8)), zkmi.DeviceBuffer(len(want) + GUARD)
        try:
            zkmi.check(L.zkmi_memset_dev(d_out.ptr, 0xAB, len(want) + GUARD))
            zkmi.check(L.zkmi_ptau_lagrange_dev(cv["id"], group, d_tau.ptr, n, d_out.ptr, first, top, int(zero_last)))
            back = d_out.to_host()
            assert back[:len(want)].tobytes() == want and (back[len(want):] == 0xAB).all()
        finally:
            d_tau.free(); d_out.free()
    # each block is the library's own single transform of its prefix
    tau = P.tau_points(cv, group, 128, inf_at=3)
    ladder = want_of(cv, group, tau, top, False)
    d_tau, d_one = zkmi.DeviceBuffer.from_host(np.frombuffer(tau, np.uint8)), zkmi.DeviceBuffer(128 * sg)
    try:
        for p in range(top + 1):
            zkmi.check(L.zkmi_group_fft_dev(cv["id"], group, d_tau.ptr, d_one.ptr, p, 1))
            assert d_one.to_host((1 << p) * sg).tobytes() == ladder[((1 << p) - 1) * sg:((2 << p) - 1) * sg], p
    finally:
        d_tau.free(); d_one.free()


def test_refusals():
    zkmi.init()
    cv = P.curve_record("bn128")
    tau = P.tau_points(cv, 1, 4)
    # top = 29 on BN254 (Fr.s = 28): refused before any length is looked at, nothing allocated or written
    raw_call(cv, 1, tau, (1 << 29) - 1, 0, 29, True, expect=4)
    assert b"top > Fr.s" in zkmi.lib().zkmi_last_error()
    bls = P.curve_record("bls12381")
    raw_call(bls, 1, P.tau_points(bls, 1, 4), 1 << 29, 0, 29, False, expect=4)        # within Fr.s = 32, beyond the 2^28 points of the top block
    for n in (3, 5):
        raw_call(cv, 1, tau + tau, n, 0, 2, False, expect=2)
    raw_call(cv, 1, tau, 4, 0, 2, True, expect=2)
    raw_call(cv, 1, tau, 4, 3, 2, False, expect=2)
    assert b"first > top" in zkmi.lib().zkmi_last_error()
    raw_call(cv, 3, tau, 4, 0, 2, False, expect=2)
    raw_call(cv, 1, tau[:-1], 4, 0, 2, False, expect=2)
    raw_call(cv, 1, tau, 4, 0, 2, False, out_cuts=[64, 64], expect=0)
    nb = 7 * 64
    short = np.full(nb - 1 + GUARD, 0xAB, np.uint8)
    rc = zkmi.lib().zkmi_ptau_lagrange_section(cv["id"], 1, zkmi.pages_of(tau).pages, 4, 0, 2, 0, (C.c_void_p * 1)(short.ctypes.data), (C.c_size_t * 1)(nb - 1), 1)
    assert rc == 2 and (short == 0xAB).all()
    assert zkmi.lib().zkmi_ptau_lagrange_dev(cv["id"], 1, None, 4, None, 0, 2, 0) == 2


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
    try:
        zkmi.check(L.zkmi_pipeline_select(0))
        zkmi.check(L.zkmi_msm_table_multi_enqueue_dev(tab.value, (C.c_void_p * 1)(d_sc.ptr), (C.c_size_t * 1)(n), 1, 32))
        with pytest.raises(zkmi.ZkmiError, match="ptau_lagrange_section: a pipeline slot holds work in flight"):
            tp.Device().lagrange_section(cv, 1, tau, 2, 0, 1, False)
        raw_call(cv, 1, tau, 2, 0, 1, False, expect=2)
        assert L.zkmi_ptau_lagrange_dev(cv["id"], 1, d_pts.ptr, 2, d_sc.ptr, 0, 1, 0) == 2
        out = np.zeros(3 * 32, np.uint8)
        zkmi.check(L.zkmi_msm_table_multi_collect(tab.value, 1, zkmi.ptr(out)))
        assert orc.to_affine(c, 1, out).tobytes() == orc.to_affine(c, 1, orc.msm(c, 1, pts, sc, n)).tobytes(), "the pending MSM was disturbed"
        assert tp.Device().lagrange_section(cv, 1, tau, 2, 0, 1, False) == want_of(cv, 1, tau, 1, False)
    finally:
        L.zkmi_msm_table_release(tab.value)
        d_pts.free(); d_sc.free()


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", P.CURVES)
def test_prepare_phase2_of_the_raw_p6_file_is_the_prepared_file_and_verifies(curve, tmp_path):
    raw, prepared = P.gold(f"ptau_{curve}_p6_c3b_raw.ptau"), P.gold(f"ptau_{curve}_p6_c3b.ptau")
    dst = tmp_path / "new.ptau"
    assert tp.prepare_phase2(os.path.join(P.GOLDEN, f"ptau_{curve}_p6_c3b_raw.ptau"), str(dst)) == prepared == dst.read_bytes()
    assert tp.prepare_phase2(raw) == prepared
    assert tv.verify(str(dst)) is True


@pytest.mark.parametrize("curve", P.CURVES)
def test_prepare_phase2_of_the_p8_setup_file_is_that_file(curve):
    """top = 9 with the zeroed last point for section 12"""
    p8 = P.gold(f"setup_{curve}_p8.ptau")
    assert tp.prepare_phase2(p8) == p8


@pytest.mark.parametrize("curve", P.CURVES)
def test_prepare_phase2_of_a_power_4_cut(curve):
    check_truncation_case(tp.prepare_phase2, curve)


@pytest.mark.parametrize("curve", P.CURVES)
def test_convert_appends_the_top_block_whether_it_is_there_or_not(curve):
    cv = P.curve_record(curve)
    prepared, p8 = P.gold(f"ptau_{curve}_p6_c3b.ptau"), P.gold(f"setup_{curve}_p8.ptau")
    assert tp.convert(without_top_block(prepared, cv, 6)) == prepared
    twice = tp.convert(p8)
    top_block = dict(P.split(p8))[12][-512 * 2 * cv["n8q"]:]
    assert twice != p8 and twice == P.join(p8, [(t, b + top_block if t == 12 else b) for t, b in P.split(p8)])
