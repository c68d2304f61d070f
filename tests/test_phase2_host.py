"""Groth16 phase 2 (snarkjs_amd/groth16_phase2.py), the parts that need no device: the library's restatement of the reference's ChaCha generator, fromRng and
hashToG2 against vectors the reference produced (tests/golden/phase2_golden.json, tools/gen_phase2_golden.js), the beacon seed, section 10 of the eight golden
keys read and written back, their transcripts and contribution hashes recomputed, the digit recoding the scaling kernel is handed, what contribute and beacon
refuse and in which words, and the whole driver with the CPU oracle standing in for the one device call."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_phase2 as p2
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi
from test_group_scale_host import R, scalars

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX = json.load(open(os.path.join(GOLDEN, "phase2_golden.json")))
STEPS = sorted(INDEX["files"])
CURVES = ("bn128", "bls12381")


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def curve_record(curve):
    return next(c for c in gs.CURVES.values() if c["name"] == curve)


def sections_of(raw):
    src = gs._Source(raw)
    return {t: src.read(*v[0]) for t, v in gs.read_sections(src, b"zkey", 2).items()}


def run_step(name, scale=None):
    rec = INDEX["files"][name]
    kw = {} if scale is None else {"scale": scale}
    if rec["op"] == "contribute":
        return p2._apply(gold(rec["from"]), rec["name"], p2.seed_from_entropy(bytes.fromhex(rec["random64"]), rec["entropy"]), dict(type=0), **kw)
    return p2._apply(gold(rec["from"]), rec["name"], p2.seed_from_beacon(bytes.fromhex(rec["beaconHash"]), rec["numIterationsExp"]),
                     dict(type=1, numIterationsExp=rec["numIterationsExp"], beaconHash=bytes.fromhex(rec["beaconHash"])), **kw)


def test_the_golden_files_are_the_recorded_ones():
    assert len(STEPS) == 8
    for name, rec in INDEX["files"].items():
        assert hashlib.sha256(gold(name)).hexdigest() == rec["sha256"], name
        assert (rec["random64"] is not None) == (rec["op"] == "contribute")


@pytest.mark.parametrize("curve", CURVES)
def test_from_rng_and_hash_to_g2_against_the_references_vectors(curve):
    cv, v = curve_record(curve), INDEX["vectors"][curve]
    assert len(v["fromRng"]) >= 16 and len(v["hashToG2"]) >= 16
    # the vectors cover a rejection in F.fromRng and a second pass of G.fromRng's x loop, on both groups
    assert any(x["frDraws"] > 4 for x in v["fromRng"]) and any(x["xPasses"] > 1 for x in v["fromRng"]) and any(x["xPasses"] > 1 for x in v["hashToG2"])
    for x in v["fromRng"]:
        prv, g1_s, g1_sx = p2.key_from_seed(cv, x["seed"])
        assert prv.hex() == x["fr"] and g1_s.hex() == x["g1"], x["seed"]
        # g1_sx = prvKey * g1_s: the oracle's scalar multiplication of the same point
        want = orc.group_apply_key(cv["id"], 1, np.frombuffer(g1_s, np.uint8), np.frombuffer(prv, np.uint8), orc.fr_one(cv["id"])).tobytes()
        assert g1_sx == want
    for x in v["hashToG2"]:
        assert p2.hash_to_g2(cv, bytes.fromhex(x["transcript"])).hex() == x["g2"], x["transcript"]


@pytest.mark.parametrize("curve", CURVES)
def test_point_mul_against_the_oracle(curve):
    cv = curve_record(curve)
    c = cv["id"]
    for group in (1, 2):
        pt = orc.geom_bases(c, group, 3)[2 * (2 * group * cv["n8q"]):]
        for k in scalars(curve)[:12]:
            km = ((k << 256) % R[curve]).to_bytes(32, "little")
            assert p2.point_mul(cv, group, pt.tobytes(), km) == orc.group_apply_key(c, group, pt, np.frombuffer(km, np.uint8), orc.fr_one(c)).tobytes(), (group, hex(k))
        assert p2.point_mul(cv, group, bytes(pt.size), (1 << 200).to_bytes(32, "little")) == bytes(pt.size)


@pytest.mark.parametrize("curve", CURVES)
def test_beacon_seed(curve):
    b = INDEX["vectors"][curve]["beaconSeed"]
    assert p2.seed_from_beacon(bytes.fromhex(b["beaconHash"]), b["numIterationsExp"]) == b["seed"]
    rec = INDEX["files"][f"phase2_{curve}_full_c1.zkey"]
    assert p2.seed_from_entropy(bytes.fromhex(rec["random64"]), rec["entropy"]) == rec["seed"]


@pytest.mark.parametrize("name", STEPS)
def test_section_10_round_trip_transcript_and_contribution_hash(name):
    rec = INDEX["files"][name]
    z = sections_of(gold(name))
    cv, _sec2, _d1, _d2 = p2.read_header(gs._Source(gold(name)), gs.read_sections(gs._Source(gold(name)), b"zkey", 2))
    cs_hash, cons = p2.parse_mpc_params(z[10], cv)
    assert p2.serialise_mpc_params(cs_hash, cons) == z[10]
    assert cs_hash == sections_of(gold(rec["from"]))[10][:64]
    last = cons[-1]
    assert last.get("name") == rec["name"] and last["type"] == (1 if rec["op"] == "beacon" else 0)
    if rec["op"] == "beacon":
        assert last["beaconHash"].hex() == rec["beaconHash"] and last["numIterationsExp"] == rec["numIterationsExp"]
    # the three kinds of parameter block are all among the eight keys: none, a name, a name with the beacon's parameters
    h = hashlib.blake2b(digest_size=64)
    h.update(cs_hash)
    for c in cons[:-1]:
        p2.hash_pub_key(h, cv, c)
    h.update(gs.lem_to_u_host(cv, last["g1_s"], 1)); h.update(gs.lem_to_u_host(cv, last["g1_sx"], 1))
    assert h.digest() == last["transcript"]
    assert p2.contribution_hash(cv, last).hex() == rec["contributionHash"]
    # deltaAfter is the key's new delta1
    _cv, sec2, at_d1, _ = p2.read_header(gs._Source(gold(name)), gs.read_sections(gs._Source(gold(name)), b"zkey", 2))
    assert sec2[at_d1:at_d1 + 2 * cv["n8q"]] == last["deltaAfter"]


def test_parameter_blocks_cover_no_name_a_name_and_a_beacon():
    kinds = set()
    for name in STEPS:
        cv = curve_record("bn128" if "bn128" in name else "bls12381")
        for c in p2.parse_mpc_params(sections_of(gold(name))[10], cv)[1]:
            kinds.add(("name" in c, c["type"]))
    assert kinds == {(False, 0), (True, 0), (True, 1)}


@pytest.mark.parametrize("curve", CURVES)
def test_digit_recoding_reconstructs_the_scalar(curve):
    L = zkmi.lib()
    for k in scalars(curve):
        km = np.frombuffer(((k << 256) % R[curve]).to_bytes(32, "little"), np.uint8)
        digits, n = np.full(256, 9, np.int8), C.c_int(-1)
        assert L.zkmi_group_scale_recode(orc.CURVE_ID[curve], zkmi.ptr(km), zkmi.ptr(digits), C.byref(n)) == 0
        d = digits[:n.value].tolist()
        assert 0 <= n.value <= 256 and set(d) <= {-1, 0, 1}
        v = 0
        for x in d:
            v = 2 * v + x
        assert v == k, hex(k)
        assert (not d or d[0] == 1) and all(a == 0 or b == 0 for a, b in zip(d, d[1:])), "a non-adjacent form, most significant digit first"
        assert n.value <= max(k.bit_length() + 1, 0)


@pytest.mark.parametrize("name", STEPS)
def test_the_whole_driver_with_the_oracle_in_place_of_the_device_call(name):
    """every byte of the key except what zkmi_group_scale computes is host work; with G1.batchApplyKey(k, 1) from the CPU oracle for sections 8 and 9 the file
    is the reference's (tests/test_gpu_groth16_phase2.py runs the same steps through the kernel)"""
    def scale(cv, body, k_mont):
        c = cv["id"]
        return orc.group_apply_key(c, 1, np.frombuffer(body, np.uint8), np.frombuffer(k_mont, np.uint8), orc.fr_one(c)).tobytes() if body else b""
    raw, h = run_step(name, scale)
    assert h.hex() == INDEX["files"][name]["contributionHash"]
    assert raw == gold(name)


def test_refusals_in_the_references_words():
    key = gold("setup_bn128_edge.zkey")
    with pytest.raises(p2.Phase2Error, match=r"^zkey file is not groth16$"):
        p2.contribute(gold("plonk_bn128_small.zkey"), "x", "e", bytes(64))
    with pytest.raises(p2.Phase2Error, match=r"^zkey file is not groth16$"):
        p2.beacon(gold("plonk_bn128_small.zkey"), "x", "0102", 10)
    for bad in ("", "0", "012", "zz", "01 2", "0x0102"):
        with pytest.raises(p2.Phase2Error) as e:
            p2.beacon(key, "x", bad, 10)
        assert str(e.value) == "Invalid Beacon Hash. (It must be a valid hexadecimal sequence)", bad
    with pytest.raises(p2.Phase2Error) as e:
        p2.beacon(key, "x", "ab" * 256, 10)
    assert str(e.value) == "Maximum length of beacon hash is 255 bytes"
    for bad in (9, 64, 0):
        with pytest.raises(p2.Phase2Error) as e:
            p2.beacon(key, "x", "0102", bad)
        assert str(e.value) == "Invalid numIterationsExp. (Must be between 10 and 63)"
    with pytest.raises(p2.Phase2Error):
        p2.contribute(key, "x", "e", bytes(63))
    with pytest.raises(p2.Phase2Error, match="Invalid File format"):
        p2.contribute(gold("setup_bn128_edge.r1cs"), "x", "e", bytes(64))


def test_names_are_cut_like_the_references():
    """name.substring(0, 64) counts UTF-16 code units; TextEncoder writes a surrogate cut off from its partner as U+FFFD"""
    assert p2._js_name("a" * 70) == b"a" * 64
    assert p2._js_name("€" * 70) == "€".encode() * 64
    assert p2._js_name("a" * 63 + "\U0001f600") == b"a" * 63 + b"\xef\xbf\xbd"
    assert p2._js_name("a" * 62 + "\U0001f600") == b"a" * 62 + "\U0001f600".encode()
    cons = [dict(deltaAfter=b"", g1_s=b"", g1_sx=b"", g2_spx=b"", transcript=b"", type=0, name="n" * 300)]
    assert p2.serialise_mpc_params(b"", cons).endswith(bytes([1, 64]) + b"n" * 64)


def test_contribute_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(zkmi.ZkmiError) as e:
        p2.contribute(gold("setup_bn128_edge.zkey"), "c1", "Entropy1", bytes(64))
    assert e.value.code == zkmi.ERR_NO_DEVICE
