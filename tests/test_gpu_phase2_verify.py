"""zKey.verifyFromInit / verifyFromR1cs on the device (snarkjs_amd/groth16_phase2_verify.py; csrc/chacha.cuh, csrc/phase2_verify.hip): the generator kernels
against the sequential generator on the host, the same-ratio kernel against the Python pairing, the two sums of the L and of the H check against the CPU
oracle's, and the driver on the eight golden keys and the tamper table with the lines tests/test_phase2_verify_host.py pins for the CPU driver."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import oracle_lib as orc
import phase2_verify_vectors as V
from snarkjs_amd import groth16_phase2 as p2
from snarkjs_amd import groth16_phase2_verify as pv
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi

pytestmark = pytest.mark.gpu
GUARD = 64                                         # bytes behind every device output, which must come back untouched
TOP = 16 * ((1 << 32) - 1) - 3                     # three words before the block whose counter carries from word 12 into word 13


def rejecting_seed(curve):
    return next(x["seed"] for x in V.INDEX["vectors"][curve]["fromRng"] if x["frDraws"] > 4)


def guarded(nbytes):
    return zkmi.DeviceBuffer.from_host(np.full(nbytes + GUARD, 0xAB, np.uint8))


def take(buf, nbytes):
    got = buf.to_host()
    buf.free()
    assert (got[nbytes:] == 0xAB).all(), "wrote behind its output"
    return got[:nbytes]


@pytest.mark.parametrize("first_word", [0, 5, TOP])
def test_chacha_words(first_word):
    zkmi.init()
    seed = rejecting_seed("bn128")
    for n in (0, 1, 15, 16, 17, 1000):
        d = guarded(4 * n)
        zkmi.check(zkmi.lib().zkmi_chacha_words_dev((C.c_uint32 * 8)(*seed), first_word, d.ptr, n))
        assert np.array_equal(take(d, 4 * n).view(np.uint32), V.host_words(seed, first_word, n)), n


@pytest.mark.parametrize("curve", V.CURVES)
def test_chacha_fr(curve):
    zkmi.init()
    L, c, seed = zkmi.lib(), orc.CURVE_ID[curve], rejecting_seed(curve)
    cs = (C.c_uint32 * 8)(*seed)
    want_all, _ = V.host_fr(c, seed, 4097)
    try:
        for blocks in (0, 7):                     # by the keep rate; in rounds of 7 blocks: the places do not depend on the cut
            zkmi.check(L.zkmi_chacha_set_round_blocks(blocks))
            for n in (0, 1, 63, 64, 65, 1000, 4097):
                d, w = guarded(32 * n), C.c_uint64(99)
                zkmi.check(L.zkmi_chacha_fr_dev(c, cs, d.ptr, n, C.byref(w)))
                assert np.array_equal(take(d, 32 * n), want_all[:32 * n]), (blocks, n)
                assert w.value == V.host_fr(c, seed, n)[1], (blocks, n)
    finally:
        L.zkmi_chacha_set_round_blocks(0)
    d = guarded(32)
    assert L.zkmi_chacha_fr_dev(c, cs, d.ptr + 4, 1, None) != 0 and b"16-byte aligned" in L.zkmi_last_error()
    d.free()


def _mont(k, r):
    return np.frombuffer(((k << 256) % r).to_bytes(32, "little"), np.uint8)


@pytest.mark.parametrize("curve", V.CURVES)
def test_same_ratio_batch(curve):
    zkmi.init()
    cv = V.curve_record(curve)
    c, s1, s2 = cv["id"], 2 * cv["n8q"], 4 * cv["n8q"]
    one = orc.fr_one(c)
    P, Q = orc.geom_bases(c, 1, 3), orc.geom_bases(c, 2, 3)
    mul = lambda g, pts, i, k: orc.group_apply_key(c, g, pts[i * (s1 if g == 1 else s2):(i + 1) * (s1 if g == 1 else s2)], _mont(k, cv["r"]), one).tobytes()
    p = lambda i: P[i * s1:(i + 1) * s1].tobytes()
    q = lambda i: Q[i * s2:(i + 1) * s2].tobytes()
    k1, k2 = 0x1234567890abcdef1234567890abcdef, cv["r"] - 5
    pool = [(p(0), mul(1, P, 0, k1), q(1), mul(2, Q, 1, k1)), (p(2), mul(1, P, 2, k2), q(0), mul(2, Q, 0, k2)),              # (P, kP, Q, kQ)
            (p(0), mul(1, P, 0, k1), q(1), mul(2, Q, 1, k1 + 1)), (p(1), mul(1, P, 1, k2), q(2), mul(2, Q, 2, k1)),          # (P, kP, Q, k'Q)
            (p(1), p(1), q(1), q(1))]                                                                                        # k = 1
    good = pool[0]
    pool += [tuple(bytes(len(x)) if j == i else x for j, x in enumerate(good)) for i in range(4)]                            # each point at infinity in turn
    want_of = {t: V.oracle_same_ratio(cv, *t) for t in pool}
    assert [want_of[t] for t in pool] == [True, True, False, False, True, False, False, False, False]
    dev = pv.Device()
    assert dev.same_ratio_batch(cv, []) == []
    out = np.full(4, 7, np.int8)
    zkmi.check(zkmi.lib().zkmi_same_ratio_batch(c, None, None, None, None, 0, zkmi.ptr(out)))
    assert (out == 7).all()
    for n in (1, 65):
        checks = [pool[(5 * i + i // 9) % len(pool)] for i in range(n)]
        assert dev.same_ratio_batch(cv, checks) == [want_of[t] for t in checks], n
    assert dev.same_ratio_batch(cv, pool) == [want_of[t] for t in pool]


@pytest.mark.parametrize("curve", V.CURVES)
def test_section_ratio(curve):
    zkmi.init()
    cv = V.curve_record(curve)
    c, s1 = cv["id"], 2 * cv["n8q"]
    A = bytearray(V.gold(f"{curve}_n1024_g1_bases.bin")[:1000 * s1])
    A[3 * s1:4 * s1] = bytes(s1)                                    # a point at infinity, in both inputs after the scaling
    A = bytes(A)
    B = p2.scale_section(cv, A, _mont(0xfeedface12345, cv["r"]).tobytes())
    assert B[3 * s1:4 * s1] == bytes(s1) and B != A
    dev, ref = pv.Device(), V.OracleDevice()
    seed = V.RANDOM64[:32]
    for n in (1, 1000):
        want = ref.section_ratio(cv, A[:n * s1], B[:n * s1], n, seed)
        assert dev.section_ratio(cv, A[:n * s1], B[:n * s1], n, seed) == want, n
        # pages that split a point, and more bytes than n points
        cut = 5 * s1 + 7 if n > 5 else 9
        assert dev.section_ratio(cv, [A[:cut], A[cut:]], [B[:cut + 30], B[cut + 30:]], n, seed) == want, n
    assert want[0] != want[1]
    r = np.full(2 * 3 * cv["n8q"], 9, np.uint8)
    empty = zkmi.pages_of(b"")
    zkmi.check(zkmi.lib().zkmi_phase2_section_ratio(c, empty.pages, empty.pages, 0, V.seed_words(seed), zkmi.ptr(r), zkmi.ptr(r[3 * cv["n8q"]:])))
    assert not r.any(), "n = 0: both sums are infinity"
    short = zkmi.pages_of(A[:s1 - 1])
    assert zkmi.lib().zkmi_phase2_section_ratio(c, short.pages, short.pages, 1, V.seed_words(seed), zkmi.ptr(r), zkmi.ptr(r)) != 0


@pytest.mark.parametrize("name", ["phase2_bn128_full_c3.zkey", "phase2_bn128_edge_c1.zkey", "phase2_bls12381_full_c3.zkey", "phase2_bls12381_edge_c1.zkey"])
def test_h_ratio(name):
    """the full keys have the ptau's own power: tauG1 holds exactly 2 domainSize - 1 points; for the edge keys the slice is cut to as many"""
    zkmi.init()
    curve = V.curve_of_file(name)
    cv = V.curve_record(curve)
    s1 = 2 * cv["n8q"]
    h = V.section(V.gold(name), 9)
    dom = len(h) // s1
    power = dom.bit_length() - 1
    ptau = gs._Source(V.gold(f"setup_{curve}_p8.ptau"))
    off, ln = gs.read_sections(ptau, b"ptau", 1)[2][0]
    assert ln >= (2 * dom - 1) * s1 and (("full" in name) == (ln == (2 * dom - 1) * s1))
    tau = ptau.read(off, (2 * dom - 1) * s1)
    seed = V.RANDOM64[32:]
    got = pv.Device().h_ratio(cv, tau, h, power, seed)
    assert got == V.OracleDevice().h_ratio(cv, tau, h, power, seed)
    assert any(got[0]) and any(got[1])
    r = np.zeros(3 * cv["n8q"], np.uint8)
    pt, ph = zkmi.pages_of(tau[:-1]), zkmi.pages_of(h)
    assert zkmi.lib().zkmi_phase2_h_ratio(cv["id"], pt.pages, ph.pages, power, V.seed_words(seed), zkmi.ptr(r), zkmi.ptr(r)) != 0
    assert b"2 domainSize - 1 points" in zkmi.lib().zkmi_last_error()
    assert zkmi.lib().zkmi_phase2_h_ratio(cv["id"], pt.pages, ph.pages, cv["s"], V.seed_words(seed), zkmi.ptr(r), zkmi.ptr(r)) == 4      # ZKMI_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", V.STEPS)
def test_the_golden_keys_verify(name):
    curve = V.curve_of_file(name)
    log = V.Log()
    # from paths for the edge keys, from bytes for the others
    src = (lambda f: os.path.join(V.GOLDEN, f)) if "edge" in name else V.gold
    assert pv.verify_from_init(src(V.init_of(name)), src(f"setup_{curve}_p8.ptau"), src(name), log, V.RANDOM64) is True
    assert log.lines == V.expected_success_lines(name)
    assert pv.verify_from_init(V.gold(V.init_of(name)), V.gold(f"setup_{curve}_p8.ptau"), V.gold(name)) is True, "fresh randomness, no logger"


@pytest.mark.parametrize("curve", V.CURVES)
def test_the_tamper_table(curve):
    ptau = V.gold(f"setup_{curve}_p8.ptau")
    rows = V.tamper_table(curve)
    assert len(rows) == 11
    for label, init, key, level, line in rows:
        log = V.Log()
        assert pv.verify_from_init(init, ptau, key, log, V.RANDOM64) is False, label
        assert log.verdict_lines() == [(level, line)], label


def test_keys_of_another_protocol_are_refused_in_the_references_words():
    plonk, init, ptau = V.gold("plonk_bn128_small.zkey"), V.gold("setup_bn128_full.zkey"), V.gold("setup_bn128_p8.ptau")
    with pytest.raises(p2.Phase2Error, match=r"^zkey file is not groth16$"):
        pv.verify_from_init(init, ptau, plonk)
    with pytest.raises(p2.Phase2Error, match=r"^zkeyinit file is not groth16$"):
        pv.verify_from_init(plonk, ptau, V.gold("phase2_bn128_full_c1.zkey"))


@pytest.mark.parametrize("curve", V.CURVES)
def test_new_zkey_contribute_verify_from_r1cs(curve):
    r1cs, ptau = V.gold(f"setup_{curve}_edge.r1cs"), V.gold(f"setup_{curve}_p8.ptau")
    init, _cs = gs.new_zkey(r1cs, ptau)
    key, _h = p2.contribute(init, "first", "some entropy", bytes(64))
    key, h2 = p2.beacon(key, "last", "0102030405", 10)
    log = V.Log()
    assert pv.verify_from_r1cs(r1cs, ptau, key, log, V.RANDOM64) is True
    assert log.lines[-1] == ("info", "ZKey Ok!") and ("info", V.format_hash(h2, "contribution #2 last:")) in log.lines
    assert pv.verify_from_r1cs(V.gold(f"setup_{curve}_full.r1cs"), ptau, key, log, V.RANDOM64) is False
    assert log.lines[-1] == ("error", "INVALID:  Different circuit parameters")


def test_a_busy_pipeline_slot_refuses_the_call_and_keeps_its_work():
    zkmi.init()
    L, c, n = zkmi.lib(), orc.BN128, 64
    args = (V.gold("setup_bn128_edge.zkey"), V.gold("setup_bn128_p8.ptau"), V.gold("phase2_bn128_edge_c1.zkey"))
    pts = orc.geom_bases(c, 1, n)
    sc = np.frombuffer(b"".join(((i * 0x9e3779b97f4a7c15 + 5) % (1 << 250)).to_bytes(32, "little") for i in range(n)), np.uint8).copy()
    d_pts, d_sc = zkmi.DeviceBuffer.from_host(pts), zkmi.DeviceBuffer.from_host(sc)
    tab = C.c_uint64()
    zkmi.check(L.zkmi_msm_table_build(c, 1, d_pts.ptr, n, C.byref(tab)))
    try:
        zkmi.check(L.zkmi_pipeline_select(0))
        zkmi.check(L.zkmi_msm_table_multi_enqueue_dev(tab.value, (C.c_void_p * 1)(d_sc.ptr), (C.c_size_t * 1)(n), 1, 32))
        with pytest.raises(zkmi.ZkmiError, match="phase2_section_ratio: a pipeline slot holds work in flight"):
            pv.verify_from_init(*args, random64=V.RANDOM64)
        cv = V.curve_record("bn128")
        with pytest.raises(zkmi.ZkmiError, match="phase2_h_ratio: a pipeline slot holds work in flight"):
            pv.Device().h_ratio(cv, bytes(255 * 64), bytes(128 * 64), 7, V.RANDOM64[32:])
        out = np.zeros(3 * 32, np.uint8)
        zkmi.check(L.zkmi_msm_table_multi_collect(tab.value, 1, zkmi.ptr(out)))
        assert orc.to_affine(c, 1, out).tobytes() == orc.to_affine(c, 1, orc.msm(c, 1, pts, sc, n)).tobytes(), "the pending MSM was disturbed"
        assert pv.verify_from_init(*args, random64=V.RANDOM64) is True
    finally:
        L.zkmi_msm_table_release(tab.value)
        d_pts.free(); d_sc.free()
