"""The Bellman phase-2 round trip on the device: zkmi_bellman_h_section (csrc/bellman.cuh) in both directions against the CPU oracle's composition of the
reference's steps (group FFT, batchApplyKey, conversion) at sizes below a wave, of one wave, across waves, of one block, across blocks and of many blocks, and
the three drivers of snarkjs_amd/groth16_bellman.py against the reference's files (tests/golden/bellman_*)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bellman_vectors as bv
import oracle_lib as orc
from snarkjs_amd import groth16_bellman as gb
from snarkjs_amd import groth16_phase2_verify as pv
from snarkjs_amd import zkmi

pytestmark = pytest.mark.gpu

LOGS = (1, 2, 5, 6, 7, 8, 9, 12)
CASES = [(c, k) for c in bv.CURVES for k in bv.CIRCUITS]


def holes(n):
    """places of the points at infinity among n: the first, the middle, the last, and a whole inversion group; below eight points the first alone, and none
    where that would leave no point"""
    if n < 8:
        return (0,) if n >= 3 else ()
    return tuple(sorted({0, n // 2, n - 1} | ({4, 5, 6, 7} if n >= 16 else set())))


def lem_to_u(curve, lem):
    return orc.group_convert(orc.CURVE_ID[curve], 1, "LEMtoU", lem).tobytes()


@functools.lru_cache(maxsize=None)
def export_case(curve, log_n):
    """(section 9 as the call takes it, the reference's H points)"""
    n = 1 << log_n
    lem = bv.subgroup_points(curve, n, holes(n))
    return lem, bv.h_export(curve, lem, log_n)


@functools.lru_cache(maxsize=None)
def import_case(curve, log_n):
    """(H points as the call takes them, the reference's section 9)"""
    m = (1 << log_n) - 1
    s = 2 * bv.curve_record(curve)["n8q"]
    u = lem_to_u(curve, bv.subgroup_points(curve, 1 << log_n, holes(m))[:m * s])
    return u, bv.h_import(curve, u, log_n)


def h_section(curve, body, log_n, direction):
    return gb.Device().h_section(bv.curve_record(curve), body, log_n, direction)


@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("curve", bv.CURVES)
def test_export_direction_against_the_oracle(curve, log_n):
    lem, want = export_case(curve, log_n)
    got = h_section(curve, lem, log_n, 0)
    s = 2 * bv.curve_record(curve)["n8q"]
    assert len(got) == len(want) == ((1 << log_n) - 1) * s
    bad = [i for i in range(len(want) // s) if got[i * s:(i + 1) * s] != want[i * s:(i + 1) * s]]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("log_n", LOGS)
@pytest.mark.parametrize("curve", bv.CURVES)
def test_import_direction_against_the_oracle(curve, log_n):
    u, want = import_case(curve, log_n)
    got = h_section(curve, u, log_n, 1)
    s = 2 * bv.curve_record(curve)["n8q"]
    assert len(got) == len(want) == (1 << log_n) * s
    bad = [i for i in range(len(want) // s) if got[i * s:(i + 1) * s] != want[i * s:(i + 1) * s]]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("curve", bv.CURVES)
def test_the_exports_store_meets_infinity_at_every_place_and_in_a_whole_group(curve):
    """the store sees what the FFT leaves, so the section is chosen backwards: the inverse of the reference's composition on H points with infinities"""
    log_n = 5
    u, lem = import_case(curve, log_n)
    s = 2 * bv.curve_record(curve)["n8q"]
    assert all(u[i * s:(i + 1) * s] == bytes(s) for i in holes(31))
    got = h_section(curve, lem, log_n, 0)
    assert got == bv.h_export(curve, lem, log_n) == u


@pytest.mark.parametrize("log_n", (1, 5, 9))
@pytest.mark.parametrize("curve", bv.CURVES)
def test_import_of_an_export_restores_all_but_the_dropped_coefficient(curve, log_n):
    """export drops coefficient n - 1 and import puts zero there: the section that comes back is the reference's for these H points, differs from the one that
    went out, and exports to the same H points again"""
    lem, u = export_case(curve, log_n)
    back = h_section(curve, u, log_n, 1)
    assert back == bv.h_import(curve, u, log_n) and back != lem
    assert h_section(curve, back, log_n, 0) == u


def test_sizes_outside_the_domain_of_the_roots_are_refused():
    L = zkmi.lib()
    zkmi.init()
    for curve, s in (("bn128", 28), ("bls12381", 32)):
        cv = bv.curve_record(curve)
        one = np.zeros(2 * cv["n8q"], np.uint8)
        out = np.zeros(4 * cv["n8q"], np.uint8)
        op, ol = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(out.size)
        for log_n in (0, s, s + 1):
            for direction in (0, 1):
                assert L.zkmi_bellman_h_section(cv["id"], zkmi.pages_of(one).pages, log_n, direction, op, ol, 1) == 4, (curve, log_n)      # ZKMI_ERR_UNSUPPORTED
                assert L.zkmi_bellman_h_section_dev(cv["id"], None, None, log_n, direction) == 4
        assert L.zkmi_bellman_h_section(cv["id"], zkmi.pages_of(one).pages, 1, 2, op, ol, 1) == 2                                          # ZKMI_ERR_INVALID
        assert L.zkmi_bellman_h_section(cv["id"], zkmi.pages_of(one).pages, 2, 1, op, ol, 1) == 2, "page totals"
    assert L.zkmi_bellman_h_section(7, zkmi.pages_of(one).pages, 1, 0, op, ol, 1) == 2


def test_the_resident_twin_gives_the_same_bytes():
    curve, log_n = "bn128", 7
    lem, want = export_case(curve, log_n)
    d_in, d_out = zkmi.DeviceBuffer(len(lem)), zkmi.DeviceBuffer(len(lem))
    try:
        host = np.frombuffer(lem, np.uint8).copy()
        zkmi.check(zkmi.lib().zkmi_memcpy_h2d(d_in.ptr, zkmi.ptr(host), host.size))
        zkmi.check(zkmi.lib().zkmi_bellman_h_section_dev(0, d_in.ptr, d_out.ptr, log_n, 0))
        got = np.zeros(len(want), np.uint8)
        zkmi.check(zkmi.lib().zkmi_memcpy_d2h(zkmi.ptr(got), d_out.ptr, got.size))
        assert got.tobytes() == want
        zkmi.check(zkmi.lib().zkmi_bellman_h_section_dev(0, d_out.ptr, d_in.ptr, log_n, 1))
        back = np.zeros(len(lem), np.uint8)
        zkmi.check(zkmi.lib().zkmi_memcpy_d2h(zkmi.ptr(back), d_in.ptr, back.size))
        assert back.tobytes() == bv.h_import(curve, want, log_n)
    finally:
        d_in.free(); d_out.free()


@pytest.mark.parametrize("curve,circuit", CASES)
def test_the_three_drivers_hold_the_golden_bytes_and_the_imported_key_verifies(curve, circuit):
    key = bv.gold(f"phase2_{curve}_{circuit}_c1.zkey")
    ch = gb.export_bellman(key)
    assert ch == bv.gold(f"bellman_{curve}_{circuit}_challenge.params")
    rec = bv.INDEX["files"][f"bellman_{curve}_{circuit}_response.params"]
    rs, h = gb.bellman_contribute(curve, ch, rec["entropy"], bytes.fromhex(rec["random64"]))
    assert h.hex() == rec["contributionHash"] and rs == bv.gold(f"bellman_{curve}_{circuit}_response.params")
    imp = bv.INDEX["imported"][f"{curve}_{circuit}"]
    new = gb.import_bellman(key, rs, imp["name"])
    assert [(t, bv.sha(b)) for t, b in bv.sections_of(new)] == [(s["type"], s["sha256"]) for s in imp["sections"]] and bv.sha(new) == imp["sha256"]
    assert pv.verify_from_init(bv.gold(f"setup_{curve}_{circuit}.zkey"), bv.gold(f"setup_{curve}_p8.ptau"), new) is imp["verifyFromInit"] is True
