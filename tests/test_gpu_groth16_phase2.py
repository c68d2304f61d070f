"""Groth16 phase 2 on the device (snarkjs_amd/groth16_phase2.py, csrc/group_scale.cuh): every step of tests/golden/phase2_golden.json from its golden
predecessor, bytes and contribution hash against the reference's (tools/gen_phase2_golden.js), the three-step chain end to end, and the refusals: a PLONK key,
and a call while a pipeline slot holds work, which must leave that work as it was."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_phase2 as p2
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX = json.load(open(os.path.join(GOLDEN, "phase2_golden.json")))["files"]
CURVES = ["bn128", "bls12381"]


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def run(rec, zkey):
    if rec["op"] == "contribute":
        return p2.contribute(zkey, rec["name"], rec["entropy"], bytes.fromhex(rec["random64"]))
    return p2.beacon(zkey, rec["name"], rec["beaconHash"], rec["numIterationsExp"])


def differing_sections(got, want):
    src = gs._Source(want)
    tab = gs.read_sections(src, b"zkey", 2)
    return [t for t, v in sorted(tab.items()) if got[v[0][0]:v[0][0] + v[0][1]] != want[v[0][0]:v[0][0] + v[0][1]]]


@pytest.mark.parametrize("name", sorted(INDEX))
def test_each_step_from_its_golden_predecessor(name):
    rec = INDEX[name]
    # from a path for the edge keys (sections read by offset), from bytes for the others
    zkey, h = run(rec, os.path.join(GOLDEN, rec["from"]) if "edge" in name else gold(rec["from"]))
    assert h.hex() == rec["contributionHash"]
    if zkey != gold(name):
        pytest.fail(f"sections that differ from the reference's key: {differing_sections(zkey, gold(name))}")


@pytest.mark.parametrize("curve", CURVES)
def test_the_three_step_chain_end_to_end(curve):
    zkey = gold(f"setup_{curve}_full.zkey")
    for step in ("c1", "b2", "c3"):
        rec = INDEX[f"phase2_{curve}_full_{step}.zkey"]
        zkey, h = run(rec, zkey)
        assert h.hex() == rec["contributionHash"], step
    assert zkey == gold(f"phase2_{curve}_full_c3.zkey")


def test_a_plonk_key_is_refused_in_the_references_words():
    with pytest.raises(p2.Phase2Error, match=r"^zkey file is not groth16$"):
        p2.contribute(gold("plonk_bn128_small.zkey"), "c", "e", bytes(64))
    with pytest.raises(p2.Phase2Error, match=r"^zkey file is not groth16$"):
        p2.beacon(gold("plonk_bn128_small.zkey"), "c", "0102", 10)


def test_a_busy_pipeline_slot_refuses_the_call_and_keeps_its_work():
    zkmi.init()
    L, c, n = zkmi.lib(), orc.BN128, 64
    rec = INDEX["phase2_bn128_edge_c1.zkey"]
    pts = orc.geom_bases(c, 1, n)
    sc = np.frombuffer(b"".join(((i * 0x9e3779b97f4a7c15 + 5) % (1 << 250)).to_bytes(32, "little") for i in range(n)), np.uint8).copy()
    d_pts, d_sc = zkmi.DeviceBuffer.from_host(pts), zkmi.DeviceBuffer.from_host(sc)
    tab = C.c_uint64()
    zkmi.check(L.zkmi_msm_table_build(c, 1, d_pts.ptr, n, C.byref(tab)))
    try:
        zkmi.check(L.zkmi_pipeline_select(0))
        zkmi.check(L.zkmi_msm_table_multi_enqueue_dev(tab.value, (C.c_void_p * 1)(d_sc.ptr), (C.c_size_t * 1)(n), 1, 32))
        with pytest.raises(zkmi.ZkmiError, match="group scale: a pipeline slot holds work in flight"):
            run(rec, gold(rec["from"]))
        out = np.zeros(3 * 32, np.uint8)
        zkmi.check(L.zkmi_msm_table_multi_collect(tab.value, 1, zkmi.ptr(out)))
        assert orc.to_affine(c, 1, out).tobytes() == orc.to_affine(c, 1, orc.msm(c, 1, pts, sc, n)).tobytes(), "the pending MSM was disturbed"
        zkey, _h = run(rec, gold(rec["from"]))
        assert zkey == gold("phase2_bn128_edge_c1.zkey")
    finally:
        L.zkmi_msm_table_release(tab.value)
        d_pts.free(); d_sc.free()
