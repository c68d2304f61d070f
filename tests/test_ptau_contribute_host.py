"""powersOfTau.newAccumulator / contribute / beacon (snarkjs_amd/powersoftau_contribute.py; csrc/ptau_contribute.hip), the parts that need no device: the hasher
state a contribution keeps (zkmi_blake2b512_partial) against the reference's own hasher, and the whole driver with the CPU oracle's G.batchApplyKey and
conversions in place of the device, held to the files, hashes and logger lines tools/gen_ptau_contribute_golden.js recorded from the reference: each step of the
power-1 and power-5 chains from its golden predecessor (tests/test_gpu_ptau_contribute.py holds the device to the same)."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as orc
import ptau_verify_vectors as P
from snarkjs_amd import powersoftau_contribute as tc
from snarkjs_amd import powersoftau_verify as tv
from snarkjs_amd import zkmi

GOLD = json.load(open(os.path.join(P.GOLDEN, "ptau_contribute_golden.json")))
STEPS = sorted(GOLD["steps"])


class OracleDevice:
    """powersoftau_contribute.Device on the CPU: orc_group_apply_key and the oracle's conversions"""

    def __init__(self):
        self.calls = []

    def contribute_section(self, cv, group, body, n, first, inc):
        c = cv["id"]
        assert len(body) == n * 2 * group * cv["n8q"]
        lem = orc.group_apply_key(c, group, np.frombuffer(bytes(body), np.uint8).copy(), np.frombuffer(first, np.uint8), np.frombuffer(inc, np.uint8))
        self.calls.append((group, n))
        return lem.tobytes(), orc.group_convert(c, group, "LEMtoC", lem).tobytes(), orc.group_convert(c, group, "LEMtoU", lem).tobytes()


def pattern(n, at=0):
    return bytes((7 * (at + i) + 3) & 255 for i in range(n))


def run_step(rec, dev, old=None):
    """the recorded call on its golden predecessor (or `old`) -> (result, lines)"""
    log = P.Log()
    if old is None:
        old = P.gold(rec["from"]) if rec["from"] else tc.new_accumulator(rec["curve"], rec["power"])[0]
    if rec["op"] == "contribute":
        return tc._contribute(old, rec["name"], rec["entropy"], None, log, bytes.fromhex(rec["random64"]), dev), log.lines
    return tc._beacon(old, rec["name"], rec["beaconHash"], rec["numIterationsExp"], None, log, dev), log.lines


# ---- the hasher state ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vec", GOLD["blake2bPartial"]["vectors"], ids=lambda v: "-".join(map(str, v["lens"])) or "none")
def test_partial_state_after_the_references_update_calls(vec):
    """the 216 bytes of misc.toPartialHash, stale buffer bytes included, and the digest resumed from them"""
    assert GOLD["blake2bPartial"]["pattern"] == "(7 * i + 3) & 255"
    chunks, at = [], 0
    for n in vec["lens"]:
        chunks.append(pattern(n, at))
        at += n
    partial = tc.blake2b_partial(chunks)
    assert partial.hex() == vec["partial"]
    whole, tail = b"".join(chunks), pattern(300, at)
    assert tv.blake2b_resume(partial, b"") == hashlib.blake2b(whole, digest_size=64).digest() == bytes.fromhex(vec["digest"])
    assert tv.blake2b_resume(partial, tail) == hashlib.blake2b(whole + tail, digest_size=64).digest()
    words = np.frombuffer(partial[128:], np.uint32)
    assert words[17] == 0 and words[19] == 0 and int(words[16]) + int(words[18]) == len(whole) % (1 << 32)


def test_the_cut_into_update_calls_shows_in_the_buffer_only():
    lens = [v["lens"] for v in GOLD["blake2bPartial"]["vectors"]]
    assert [525352] in lens and [64, 525288] in lens and [64, 524288, 1000] in lens
    by = {tuple(v["lens"]): bytes.fromhex(v["partial"]) for v in GOLD["blake2bPartial"]["vectors"]}
    a, b = by[(525352,)], by[(64, 524288, 1000)]
    assert a[128:] == b[128:] and a[:128] != b[:128], "same state and position, different stale bytes"
    pos = int(np.frombuffer(a[128:], np.uint32)[18])
    assert a[:pos] == b[:pos]


def test_partial_refuses_null_arguments():
    L = zkmi.lib()
    assert L.zkmi_blake2b512_partial(None, None, 1, zkmi.ptr(np.zeros(216, np.uint8))) != 0
    assert L.zkmi_blake2b512_partial(None, None, 0, None) != 0
    assert b"null argument" in L.zkmi_last_error()


# ---- the driver, the oracle in place of the device ----------------------------------------------------------------------------------------------------
def test_the_golden_files_are_the_recorded_ones():
    assert len(STEPS) == 12
    for name in STEPS:
        raw = P.gold(name)
        assert hashlib.sha256(raw).hexdigest() == GOLD["steps"][name]["sha256"] and len(raw) == GOLD["steps"][name]["bytes"] < 120 * 1024, name


@pytest.mark.parametrize("key", sorted(GOLD["fresh"]) + ["bn128_p14"])
def test_new_accumulator_by_sha256(key):
    rec = GOLD["fresh"].get(key) or dict(curve="bn128", power=14, sha256=GOLD["p14"]["freshSha256"])
    log = P.Log()
    raw, first = tc.new_accumulator(rec["curve"], rec["power"], None, log)
    assert hashlib.sha256(raw).hexdigest() == rec["sha256"]
    if "lines" in rec:
        assert first.hex() == rec["firstChallengeHash"] and len(raw) == rec["bytes"]
        assert log.lines == [tuple(x) for x in rec["lines"]] or [list(x) for x in log.lines] == rec["lines"]
    assert tv._verify(raw, None, P.RANDOM32, P.OracleDevice()) is False, "no contribution yet"


@pytest.mark.parametrize("name", STEPS)
def test_each_step_from_its_golden_predecessor(name):
    """the file byte for byte, the returned response hash, the two info lines"""
    rec, dev = GOLD["steps"][name], OracleDevice()
    (raw, response), lines = run_step(rec, dev)
    assert response.hex() == rec["returned"]
    assert hashlib.sha256(raw).hexdigest() == rec["sha256"] and raw == P.gold(name)
    assert [list(x) for x in lines] == rec["lines"] and [x[1].split("\n")[0] for x in lines] == ["Contribution Response Hash imported: ", "Next Challenge Hash: "]
    n = 1 << rec["power"]
    assert dev.calls == [(1, 2 * n - 1), (2, n), (1, n), (1, n)], "one call per section"


@pytest.mark.parametrize("curve", P.CURVES)
def test_a_chain_made_here_end_to_end_passes_verify(curve):
    """new_accumulator -> C1 -> C2 -> B3 with nothing of the reference in between: the golden b3 file, which this project's verify (CPU stand-in) accepts"""
    raw = tc.new_accumulator(curve, 5)[0]
    for tag in ("c1", "c2", "b3"):
        (raw, _), _ = run_step(GOLD["steps"][f"ptau_{curve}_p5_{tag}.ptau"], OracleDevice(), old=raw)
    assert raw == P.gold(f"ptau_{curve}_p5_b3.ptau")
    log = P.Log()
    assert tv._verify(raw, log, P.RANDOM32, P.OracleDevice()) is True
    assert log.lines[-1][1] == "Powers of Tau Ok!"


def test_the_power_14_contribution_two_chunks_of_the_response_hasher():
    """tauG1 at power 14 is 2^15 - 1 points: one chunk of 2^14 points and one of 2^14 - 1 in the reference's response hasher, which section 7 remembers"""
    rec = GOLD["p14"]
    raw = tc.new_accumulator("bn128", 14)[0]
    out, response = tc._contribute(raw, rec["name"], rec["entropy"], None, None, bytes.fromhex(rec["random64"]), OracleDevice())
    assert dict(P.split(out))[7].hex() == rec["section7"]
    assert response.hex() == rec["returned"] and len(out) == rec["bytes"] and hashlib.sha256(out).hexdigest() == rec["sha256"]


@pytest.mark.parametrize("case", GOLD["refused"], ids=lambda c: c["curve"] + "-" + c["label"].replace(" ", "_"))
def test_what_the_reference_refuses(case):
    cv = P.curve_record(case["curve"])
    old = P.gold(case["from"])
    if case["rule"] == "truncate4":
        old = P.join(old, [(t, b) for t, b in P.split(P.truncate4(old, cv["n8q"])) if t < 12])
    log, dev = P.Log(), OracleDevice()
    if case["op"] == "contribute":
        with pytest.raises(tc.PtauError) as e:
            tc._contribute(old, case["name"], case["entropy"], None, log, bytes(64), dev)
        assert str(e.value) == case["throws"]
    elif "throws" in case:                                            # the reference fails inside hex2ByteArray: nothing to reproduce but the refusal
        with pytest.raises(tc.PtauError):
            tc._beacon(old, case["name"], case["beaconHash"], case["numIterationsExp"], None, log, dev)
    else:
        assert case["returns"] is False
        assert tc._beacon(old, case["name"], case["beaconHash"], case["numIterationsExp"], None, log, dev) is False
    assert [list(x) for x in log.lines] == case["lines"] and dev.calls == []


def test_more_refusals_and_the_phase2_warning():
    cv = P.curve_record("bn128")
    c1 = P.gold("ptau_bn128_p5_c1.ptau")
    assert all("throws" in GOLD["power0"][c]["contribute"] and "throws" in GOLD["power0"][c]["beacon"] for c in P.CURVES), "the reference fails at power 0"
    raw0 = tc.new_accumulator("bn128", 0)[0]
    assert hashlib.sha256(raw0).hexdigest() == GOLD["power0"]["bn128"]["sha256"]
    with pytest.raises(tc.PtauError, match="^power 0"):
        tc._contribute(raw0, "C1", "Entropy1", None, None, bytes(64), OracleDevice())
    with pytest.raises(tc.PtauError, match="^power 0"):
        tc._beacon(raw0, "B1", "0102", 10, None, None, OracleDevice())
    with pytest.raises(tc.PtauError, match="entropy"):
        tc._contribute(c1, "C", "", None, None, None, OracleDevice())
    with pytest.raises(tc.PtauError, match="^Curve not supported"):
        tc.new_accumulator("secp256k1", 3)
    # a "0x" in front counts towards the length the reference compares: refused with the line
    log = P.Log()
    assert tc._beacon(c1, "B", "0x0102", 10, None, log, OracleDevice()) is False and log.lines[0][1].startswith("Invalid Beacon Hash")
    # a contribution whose bytes do not come back from the reader and writer: a parameter block with the name after the beacon parameters is refused by the reader;
    # a name of zero length is read but never written
    secs = P.split(c1)
    s7 = bytearray(dict(secs)[7])
    at = s7.rindex(b"\x01\x02C1")
    bad = bytes(s7[:at - 4]) + (2).to_bytes(4, "little") + b"\x01\x00"
    with pytest.raises(tc.PtauError, match="serialise back"):
        tc._contribute(P.join(c1, [(t, bad if t == 7 else b) for t, b in secs]), "C", "e", None, None, bytes(64), OracleDevice())
    # section 12 present: the warning, in each function's own words, and the contribution goes through
    prepared = P.gold("ptau_bn128_p6_c3b.ptau")
    log = P.Log()
    out, _ = tc._contribute(prepared, "C4", "e", None, log, bytes(64), OracleDevice())
    assert log.lines[0] == ("warn", "WARNING: Contributing into a file that has phase2 calculated. You will have to prepare phase2 again.")
    assert [t for t, _ in P.split(out)] == [1, 2, 3, 4, 5, 6, 7]
    log = P.Log()
    tc._beacon(prepared, "B4", "0102", 10, None, log, OracleDevice())
    assert log.lines[0] == ("warn", "Contributing into a file that has phase2 calculated. You will have to prepare phase2 again.")


def test_the_driver_writes_the_file_when_given_a_path(tmp_path, monkeypatch):
    monkeypatch.setattr(tc, "Device", OracleDevice)
    rec = GOLD["steps"]["ptau_bn128_p1_c1.ptau"]
    fresh, dst = tmp_path / "fresh.ptau", tmp_path / "c1.ptau"
    raw, _ = tc.new_accumulator("bn128", 1, str(fresh))
    assert fresh.read_bytes() == raw
    out, _ = tc.contribute(str(fresh), rec["name"], rec["entropy"], str(dst), None, bytes.fromhex(rec["random64"]))
    assert out == dst.read_bytes() == P.gold("ptau_bn128_p1_c1.ptau")


def test_the_section_call_without_a_device_fails_loudly():
    import torch
    L = zkmi.lib()
    assert L.zkmi_ptau_contribute_section and L.zkmi_diag_group_mul_each_dev and L.zkmi_diag_set_ptau_slice
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    cv = P.curve_record("bn128")
    one = ((1 << 256) % cv["r"]).to_bytes(32, "little")
    with pytest.raises(zkmi.ZkmiError) as e:
        tc.Device().contribute_section(cv, 1, P.tau_points(cv, 1, 2), 2, one, one)
    assert e.value.code == zkmi.ERR_NO_DEVICE
