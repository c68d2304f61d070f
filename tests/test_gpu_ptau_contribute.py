"""A phase-1 contribution on the device: the per-lane-scalar G1 kernel (csrc/ptau_contribute.cuh through zkmi_diag_group_mul_each_dev) against the CPU oracle,
the section call zkmi_ptau_contribute_section against the library's general kernel (zkmi_group_batch_apply_key), its conversions (zkmi_group_convert) and the
oracle, and the drivers of snarkjs_amd/powersoftau_contribute.py on the golden chains of tools/gen_ptau_contribute_golden.js, both curves."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import oracle_lib as orc
import ptau_verify_vectors as P
from ptau_contribute_vectors import R, edge_scalars, expected_each, mont, normal
from snarkjs_amd import powersoftau_contribute as tc
from snarkjs_amd import powersoftau_prepare as tp
from snarkjs_amd import powersoftau_verify as tv
from snarkjs_amd import zkmi
from test_ptau_contribute_host import GOLD, STEPS, run_step

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12381"]
SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1021]
GUARD = 64


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------------------------
_ref = {}


def kernel_reference(curve):
    """1021 points of the (7 * 11^i) G table, lane i with edge scalar i mod 116 — the first wave holds 0, 1, r - 1, even and odd ones — and the oracle's
    products, computed once; a smaller size takes the prefix"""
    if curve not in _ref:
        c = orc.CURVE_ID[curve]
        ks = edge_scalars(curve)
        assert {0, 1, R[curve] - 1} <= set(ks[:64]) and any(k % 2 for k in ks[:64]) and any(k % 2 == 0 and k for k in ks[:64])
        ks = [ks[i % len(ks)] for i in range(1021)]
        pts = orc.geom_bases(c, 1, 1021)
        _ref[curve] = (ks, pts, expected_each(curve, pts, ks))
    return _ref[curve]


def planted(n):
    """where the point at infinity goes: the first and the last lane and, inside an inversion group, lane 6 and all of lanes 8 .. 11"""
    return sorted({0, n - 1} | {i for i in (6, 8, 9, 10, 11) if i < n}) if n >= 3 else []


def mul_each(curve, pts, ks):
    zkmi.init()
    c, L = orc.CURVE_ID[curve], zkmi.lib()
    n = len(ks)
    d_in, d_k = zkmi.DeviceBuffer.from_host(pts), zkmi.DeviceBuffer.from_host(np.frombuffer(normal(ks), np.uint8))
    d_out = zkmi.DeviceBuffer.from_host(np.full(pts.size + GUARD, 0xA5, np.uint8))
    try:
        zkmi.check(L.zkmi_diag_group_mul_each_dev(c, 1, d_in.ptr, d_k.ptr, d_out.ptr, n))
        out = d_out.to_host()
        assert d_in.to_host().tobytes() == pts.tobytes(), "the source was written"
    finally:
        d_in.free(); d_k.free(); d_out.free()
    assert (out[pts.size:] == 0xA5).all(), "bytes after the last point were written"
    return out[:pts.size].tobytes()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("curve", CURVES)
def test_kernel_against_the_oracle(curve, n):
    ks, pts, want = kernel_reference(curve)
    sz = pts.size // 1021
    for holes in ([], planted(n)) if planted(n) else ([],):
        p, w = pts[:n * sz].copy().reshape(n, sz), np.frombuffer(want[:n * sz], np.uint8).copy().reshape(n, sz)
        for i in holes:
            p[i] = 0
            w[i] = 0
        got = mul_each(curve, p.reshape(-1), ks[:n])
        for i in range(n):
            assert got[i * sz:(i + 1) * sz] == w[i].tobytes(), (n, i, hex(ks[i]), bool(holes))


def test_kernel_entry_refusals():
    zkmi.init()
    L = zkmi.lib()
    d = zkmi.DeviceBuffer.from_host(np.zeros(256, np.uint8))
    try:
        assert L.zkmi_diag_group_mul_each_dev(0, 2, d.ptr, d.ptr, d.ptr, 1) == 4, "ZKMI_ERR_UNSUPPORTED"
        assert L.zkmi_diag_group_mul_each_dev(7, 1, d.ptr, d.ptr, d.ptr, 1) != 0 and b"unknown curve or group" in L.zkmi_last_error()
        assert L.zkmi_diag_group_mul_each_dev(0, 1, None, d.ptr, d.ptr, 1) != 0 and b"null buffer" in L.zkmi_last_error()
        assert L.zkmi_diag_group_mul_each_dev(0, 1, None, None, None, 0) == 0
    finally:
        d.free()


# ---- the section call -------------------------------------------------------------------------------------------------------------------------------------
_pts = {}


def points(cv, group, n, inf_at=None):
    """n points of the (7 * 11^i) G table of the group, optionally with infinity at one index"""
    k = (cv["name"], group)
    if k not in _pts:
        _pts[k] = orc.geom_bases(cv["id"], group, 300).tobytes()
    sg = 2 * group * cv["n8q"]
    b = bytearray(_pts[k][:n * sg])
    if inf_at is not None and inf_at < n:
        b[inf_at * sg:(inf_at + 1) * sg] = bytes(sg)
    return bytes(b)


def cut(total, sizes):
    """page lengths that add up to total: the given sizes in turn, the last page short"""
    out, i = [], 0
    while total:
        k = min(total, sizes[i % len(sizes)])
        out.append(k)
        total -= k
        i += 1
    return out or [0]


def section_call(cv, group, body, n, first, inc, in_page=None, out_pages=(1000, 777, 333), expect=0):
    """zkmi_ptau_contribute_section with pages that split a point going in and coming out and guard bytes behind every output page -> (lem, c, u)"""
    zkmi.init()
    sg = 2 * group * cv["n8q"]
    body = np.frombuffer(bytes(body), np.uint8)
    pg = zkmi.pages_of([body[o:o + in_page] for o in range(0, body.size, in_page)] if in_page and body.size else body)
    f, i = np.frombuffer(bytes(first), np.uint8).copy(), np.frombuffer(bytes(inc), np.uint8).copy()
    bufs, args = [], []
    for total, page in zip((n * sg, n * sg // 2, n * sg), out_pages):
        pages = [np.full(k + GUARD, 0xA5, np.uint8) for k in cut(total, [page, page + 1])]
        lens = cut(total, [page, page + 1])
        bufs.append((pages, lens))
        args += [(C.c_void_p * len(pages))(*[p.ctypes.data for p in pages]), (C.c_size_t * len(pages))(*lens), len(pages)]
    rc = zkmi.lib().zkmi_ptau_contribute_section(cv["id"], group, pg.pages, n, zkmi.ptr(f), zkmi.ptr(i), *args)
    assert rc == expect, zkmi.lib().zkmi_last_error()
    for pages, lens in bufs:
        assert all((p[k:] == 0xA5).all() for p, k in zip(pages, lens)), "guard bytes were written"
    if expect:
        assert all((p == 0xA5).all() for pages, _ in bufs for p in pages), "a refused call wrote its outputs"
        return None
    return tuple(b"".join(p[:k].tobytes() for p, k in zip(pages, lens)) for pages, lens in bufs)


def parent_kernel(cv, group, body, n, first, inc):
    """what the parent commit computes: zkmi_group_batch_apply_key, and zkmi_group_convert of its output"""
    zkmi.init()
    L, c = zkmi.lib(), cv["id"]
    body = np.frombuffer(bytes(body), np.uint8)
    f, i = np.frombuffer(bytes(first), np.uint8).copy(), np.frombuffer(bytes(inc), np.uint8).copy()
    lem = np.zeros(body.size, np.uint8)
    zkmi.check(L.zkmi_group_batch_apply_key(c, group, zkmi.pages_of(body).pages, (C.c_void_p * 1)(lem.ctypes.data), (C.c_size_t * 1)(lem.size), 1, n, zkmi.ptr(f), zkmi.ptr(i)))
    out = [lem.tobytes()]
    for kind, size in ((zkmi.CONV_LEM_TO_C, body.size // 2), (zkmi.CONV_LEM_TO_U, body.size)):
        o = np.zeros(size, np.uint8)
        zkmi.check(L.zkmi_group_convert(c, group, kind, zkmi.pages_of(lem).pages, (C.c_void_p * 1)(o.ctypes.data), (C.c_size_t * 1)(o.size), 1, n))
        out.append(o.tobytes())
    return tuple(out)


def oracle_section(cv, group, body, first, inc):
    c = cv["id"]
    lem = orc.group_apply_key(c, group, np.frombuffer(bytes(body), np.uint8).copy(), np.frombuffer(bytes(first), np.uint8), np.frombuffer(bytes(inc), np.uint8))
    return lem.tobytes(), orc.group_convert(c, group, "LEMtoC", lem).tobytes(), orc.group_convert(c, group, "LEMtoU", lem).tobytes()


def section_scalars(curve):
    """first in {0, 1, random} x inc in {1, random, a primitive 2^8-th root: the powers wrap at n = 300}, Montgomery bytes"""
    c = orc.CURVE_ID[curve]
    rnd = random.Random(20261020)
    firsts = [("0", bytes(32)), ("1", orc.fr_one(c).tobytes()), ("random", mont(curve, rnd.randrange(R[curve])).tobytes())]
    incs = [("1", orc.fr_one(c).tobytes()), ("random", mont(curve, rnd.randrange(R[curve])).tobytes()), ("w8", orc.fr_w(c, 8).tobytes())]
    return [(a + "," + b, f, i) for a, f in firsts for b, i in incs]


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", CURVES)
def test_section_call_against_the_parents_kernel_and_the_oracle(curve, group):
    cv = P.curve_record(curve)
    L = zkmi.lib()
    for n in (1, 2, 3, 127, 300):
        body = points(cv, group, n, inf_at=(n // 2 if n > 2 else None))
        combos = section_scalars(curve)
        for label, first, inc in combos:
            if n == 300:
                zkmi.check(L.zkmi_diag_set_ptau_slice(128))        # two slice edges and a tail of 44 points
            try:
                got = section_call(cv, group, body, n, first, inc, in_page=1000)
            finally:
                zkmi.check(L.zkmi_diag_set_ptau_slice(0))
            want = parent_kernel(cv, group, body, n, first, inc)
            for name, g, w, o in zip(("LEM", "C", "U"), got, want, oracle_section(cv, group, body, first, inc)):
                assert g == w, (n, label, name, "against zkmi_group_batch_apply_key / zkmi_group_convert")
                assert g == o, (n, label, name, "against the oracle")


def test_section_call_slices_do_not_change_the_result():
    cv = P.curve_record("bn128")
    L = zkmi.lib()
    _, first, inc = section_scalars("bn128")[4]
    body = points(cv, 1, 300)
    whole = section_call(cv, 1, body, 300, first, inc)
    for s in (1, 64, 299, 300, 301):
        zkmi.check(L.zkmi_diag_set_ptau_slice(s))
        try:
            assert section_call(cv, 1, body, 300, first, inc) == whole, s
        finally:
            zkmi.check(L.zkmi_diag_set_ptau_slice(0))


def test_section_call_refusals():
    zkmi.init()
    cv, L = P.curve_record("bn128"), zkmi.lib()
    one = orc.fr_one(0).tobytes()
    body = P.tau_points(cv, 1, 4)
    bad = dict(cv, id=7)
    section_call(bad, 1, body, 4, one, one, expect=2)
    assert b"ptau_contribute_section: unknown curve or group" in L.zkmi_last_error()
    section_call(cv, 3, body, 4, one, one, expect=2)
    section_call(cv, 1, body, 5, one, one, expect=2)
    assert b"input pages do not hold n points" in L.zkmi_last_error()
    section_call(cv, 1, body + bytes(1), 4, one, one, expect=2)
    # an output list one byte short, each in turn
    for k in range(3):
        lens = [256, 128, 256]
        lens[k] -= 1
        outs = [np.full(256, 0xA5, np.uint8) for _ in range(3)]
        args = []
        for o, ln in zip(outs, lens):
            args += [(C.c_void_p * 1)(o.ctypes.data), (C.c_size_t * 1)(ln), 1]
        f = np.frombuffer(one, np.uint8).copy()
        assert L.zkmi_ptau_contribute_section(0, 1, zkmi.pages_of(body).pages, 4, zkmi.ptr(f), zkmi.ptr(f), *args) == 2
        assert b"output pages do not hold n points" in L.zkmi_last_error() and all((o == 0xA5).all() for o in outs)
    f = np.frombuffer(one, np.uint8).copy()
    nul = [None, None, 0] * 3
    assert L.zkmi_ptau_contribute_section(0, 1, zkmi.pages_of(body).pages, 4, None, zkmi.ptr(f), *nul) == 2 and b"null argument" in L.zkmi_last_error()
    assert L.zkmi_ptau_contribute_section(0, 1, zkmi.pages_of(body).pages, 4, zkmi.ptr(f), zkmi.ptr(f), *nul) == 2 and b"null argument" in L.zkmi_last_error()
    # n == 0 touches nothing
    assert L.zkmi_ptau_contribute_section(0, 1, zkmi.pages_of(b"").pages, 0, zkmi.ptr(f), zkmi.ptr(f), *nul) == 0


def test_a_busy_pipeline_slot_refuses_the_call_and_keeps_its_work():
    zkmi.init()
    L, c, n = zkmi.lib(), orc.BN128, 64
    cv = P.curve_record("bn128")
    pts = orc.geom_bases(c, 1, n)
    sc = np.frombuffer(b"".join(((i * 0x9e3779b97f4a7c15 + 5) % (1 << 250)).to_bytes(32, "little") for i in range(n)), np.uint8).copy()
    d_pts, d_sc = zkmi.DeviceBuffer.from_host(pts), zkmi.DeviceBuffer.from_host(sc)
    tab = C.c_uint64()
    zkmi.check(L.zkmi_msm_table_build(c, 1, d_pts.ptr, n, C.byref(tab)))
    one = orc.fr_one(c).tobytes()
    body = P.tau_points(cv, 1, 4)
    try:
        zkmi.check(L.zkmi_pipeline_select(0))
        zkmi.check(L.zkmi_msm_table_multi_enqueue_dev(tab.value, (C.c_void_p * 1)(d_sc.ptr), (C.c_size_t * 1)(n), 1, 32))
        with pytest.raises(zkmi.ZkmiError, match="ptau_contribute_section: a pipeline slot holds work in flight"):
            tc.Device().contribute_section(cv, 1, body, 4, one, one)
        section_call(cv, 1, body, 4, one, one, expect=2)
        assert L.zkmi_diag_group_mul_each_dev(c, 1, d_pts.ptr, d_sc.ptr, d_pts.ptr, 2) == 2
        out = np.zeros(3 * 32, np.uint8)
        zkmi.check(L.zkmi_msm_table_multi_collect(tab.value, 1, zkmi.ptr(out)))
        assert orc.to_affine(c, 1, out).tobytes() == orc.to_affine(c, 1, orc.msm(c, 1, pts, sc, n)).tobytes(), "the pending MSM was disturbed"
        assert tc.Device().contribute_section(cv, 1, body, 4, one, one) == oracle_section(cv, 1, body, one, one)
    finally:
        L.zkmi_msm_table_release(tab.value)
        d_pts.free(); d_sc.free()


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STEPS)
def test_each_golden_step_on_the_device(name):
    rec = GOLD["steps"][name]
    (raw, response), lines = run_step(rec, tc.Device())
    assert response.hex() == rec["returned"] and raw == P.gold(name)
    assert [list(x) for x in lines] == rec["lines"]


@pytest.mark.parametrize("power", [1, 5])
@pytest.mark.parametrize("curve", CURVES)
def test_a_ceremony_end_to_end_on_the_device(curve, power, tmp_path):
    """new_accumulator -> C1 -> C2 -> B3 through the public functions and paths, then verify, and prepare_phase2 where the reference's bytes are at hand"""
    path = [str(tmp_path / f"{i}.ptau") for i in range(4)]
    raw, first = tc.new_accumulator(curve, power, path[0])
    assert first.hex() == GOLD["fresh"][f"{curve}_p{power}"]["firstChallengeHash"]
    for i, tag in enumerate(("c1", "c2", "b3")):
        rec = GOLD["steps"][f"ptau_{curve}_p{power}_{tag}.ptau"]
        if rec["op"] == "contribute":
            raw, h = tc.contribute(path[i], rec["name"], rec["entropy"], path[i + 1], None, bytes.fromhex(rec["random64"]))
        else:
            raw, h = tc.beacon(path[i], rec["name"], rec["beaconHash"], rec["numIterationsExp"], path[i + 1])
        assert h.hex() == rec["returned"]
    assert raw == P.gold(f"ptau_{curve}_p{power}_b3.ptau") == open(path[3], "rb").read()
    assert tv.verify(raw) is True
    prepared = tp.prepare_phase2(raw)
    assert tv.verify(prepared) is True


@pytest.mark.parametrize("curve", CURVES)
def test_contributions_on_top_of_the_references_power_6_ceremony(curve):
    """the golden raw file of tools/gen_ptau_golden.js prepares to the reference's prepared file (the one chain with prepared bytes at hand: the random64 of its
    contributions was not recorded, so it cannot be made again here); a contribution and a beacon on top of it prepare and verify"""
    raw6 = P.gold(f"ptau_{curve}_p6_c3b_raw.ptau")
    assert tp.prepare_phase2(raw6) == P.gold(f"ptau_{curve}_p6_c3b.ptau")
    out, _ = tc.contribute(raw6, "C4", "Entropy4", None, None, bytes(range(64)))
    assert tv.verify(tp.prepare_phase2(out)) is True
    res = tc.beacon(out, "B5", "0a0b0c", 10)
    assert res is not False and tv.verify(res[0]) is True


def test_the_power_14_contribution_on_the_device():
    rec = GOLD["p14"]
    raw = tc.new_accumulator("bn128", 14)[0]
    assert hashlib.sha256(raw).hexdigest() == rec["freshSha256"]
    out, response = tc.contribute(raw, rec["name"], rec["entropy"], None, None, bytes.fromhex(rec["random64"]))
    assert dict(P.split(out))[7].hex() == rec["section7"]
    assert response.hex() == rec["returned"] and hashlib.sha256(out).hexdigest() == rec["sha256"]


def test_the_refusals_on_the_device():
    c1 = P.gold("ptau_bn128_p5_c1.ptau")
    cv = P.curve_record("bn128")
    reduced = P.join(c1, [(t, b) for t, b in P.split(P.truncate4(c1, cv["n8q"])) if t < 12])
    log = P.Log()
    with pytest.raises(tc.PtauError, match="^This file has been reduced"):
        tc.contribute(reduced, "X", "e", None, log)
    assert tc.beacon(reduced, "X", "0102", 10, None, log) is False
    assert tc.beacon(c1, "X", "012", 10, None, log) is False and tc.beacon(c1, "X", "0102", 9, None, log) is False and tc.beacon(c1, "X", "0102", 64, None, log) is False
    assert [lv for lv, _ in log.lines] == ["error"] * 5
