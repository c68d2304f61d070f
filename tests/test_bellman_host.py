"""The Bellman phase-2 round trip (snarkjs_amd/groth16_bellman.py), everything that needs no device: the three drivers with the CPU oracle in the place of
their device steps against the files the reference wrote (tests/golden/bellman_*, tools/gen_bellman_golden.js), every refusal in the recorded words, and what
a round trip does to a key."""
import hashlib
import struct

import pytest

import bellman_vectors as bv
from snarkjs_amd import groth16_bellman as gb
from snarkjs_amd import zkmi

DEV = bv.OracleDevice()
CASES = [(c, k) for c in bv.CURVES for k in bv.CIRCUITS]


def key_of(curve, circuit):
    return f"phase2_{curve}_{circuit}_c1.zkey"


def test_the_golden_files_are_the_recorded_ones():
    assert len(bv.INDEX["files"]) == 8 and len(bv.INDEX["imported"]) == 4
    for name, rec in bv.INDEX["files"].items():
        assert bv.sha(bv.gold(name)) == rec["sha256"], name
    for rec in bv.INDEX["imported"].values():
        assert rec["verifyFromInit"] is True and [s["type"] for s in rec["sections"]] == [1, 2, 3, 4, 9, 8, 5, 6, 7, 10]


@pytest.mark.parametrize("curve,circuit", CASES)
def test_export_writes_the_references_challenge(curve, circuit):
    assert gb._export(bv.gold(key_of(curve, circuit)), DEV) == bv.gold(f"bellman_{curve}_{circuit}_challenge.params")


@pytest.mark.parametrize("curve,circuit", CASES)
def test_contribute_writes_the_references_response_and_hash(curve, circuit):
    name = f"bellman_{curve}_{circuit}_response.params"
    rec = bv.INDEX["files"][name]
    raw, h = gb._contribute(curve, bv.gold(rec["from"]), rec["entropy"], bytes.fromhex(rec["random64"]), DEV)
    assert h.hex() == rec["contributionHash"]
    assert raw == bv.gold(name)


@pytest.mark.parametrize("curve,circuit", CASES)
def test_import_writes_the_references_key_section_by_section(curve, circuit):
    rec = bv.INDEX["imported"][f"{curve}_{circuit}"]
    raw = gb._import(bv.gold(rec["old"]), bv.gold(rec["params"]), rec["name"], DEV)
    got = bv.sections_of(raw)
    assert [(t, len(b), bv.sha(b)) for t, b in got] == [(s["type"], s["size"], s["sha256"]) for s in rec["sections"]]
    assert len(raw) == rec["bytes"] and bv.sha(raw) == rec["sha256"]
    # sections 3 - 7 are the old key's, new contributions carry the name, old ones keep theirs
    old = dict(bv.sections_of(bv.gold(rec["old"])))
    new = dict(got)
    assert all(new[t] == old[t] for t in (3, 4, 5, 6, 7))
    cv = bv.curve_record(curve)
    cons = gb.parse_mpc_params(new[10], cv)[1]
    assert [c.get("name") for c in cons] == ["c1", "imp"] and [c["type"] for c in cons] == [0, 0]


@pytest.mark.parametrize("curve,circuit", CASES)
def test_export_then_import_changes_section_9_alone(curve, circuit):
    """export drops the last coefficient of H and import puts zero in its place: every other section, header included, comes back as it was, section 9 comes
    back as the reference's composition gives it, and a second round trip changes nothing more"""
    key = bv.gold(key_of(curve, circuit))
    back = gb._import(key, gb._export(key, DEV), None, DEV)
    old, new = dict(bv.sections_of(key)), dict(bv.sections_of(back))
    assert [t for t, _ in bv.sections_of(back)] == [1, 2, 3, 4, 9, 8, 5, 6, 7, 10]
    assert all(new[t] == old[t] for t in (1, 2, 3, 4, 5, 6, 7, 8, 10))
    power = (len(old[9]) // (2 * bv.curve_record(curve)["n8q"])).bit_length() - 1
    assert new[9] != old[9] and new[9] == bv.h_import(curve, bv.h_export(curve, old[9], power), power)
    assert gb._import(back, gb._export(back, DEV), None, DEV) == back


def test_refusals_carry_the_recorded_words():
    for curve in bv.CURVES:
        ref = bv.INDEX["refusals"][curve]
        key, rs = bv.gold(key_of(curve, "full")), bv.gold(f"bellman_{curve}_full_response.params")
        plonk = bv.gold("plonk_bn128_small.zkey")
        assert ref["plonk_export"]["threw"] == ref["plonk_import"]["threw"] == "zkey file is not groth16"
        with pytest.raises(gb.BellmanError, match=r"^zkey file is not groth16$"):
            gb._export(plonk, DEV)
        with pytest.raises(gb.BellmanError, match=r"^zkey file is not groth16$"):
            gb._import(plonk, rs, "x", DEV)

        def line(case):
            assert ref[case]["returned"] is False and len(ref[case]["lines"]) == 1 and ref[case]["lines"][0][0] == "error"
            return ref[case]["lines"][0][1]
        with pytest.raises(gb.BellmanError) as e:
            gb._import(bv.gold(ref["fewer_contributions"]["old"]), rs, "x", DEV)
        assert str(e.value) == line("fewer_contributions") == "The impoerted file does not include new contributions"
        flipped = bytearray(rs)
        flipped[ref["flipped_transcript"]["at"]] ^= 1
        with pytest.raises(gb.BellmanError) as e:
            gb._import(key, bytes(flipped), "x", DEV)
        assert str(e.value) == line("flipped_transcript") == "Previous contribution 0 does not match"
        wrong = bytearray(rs)
        struct.pack_into(">I", wrong, ref["wrong_h_count"]["at"], ref["wrong_h_count"]["value"])
        with pytest.raises(gb.BellmanError) as e:
            gb._import(key, bytes(wrong), "x", DEV)
        assert str(e.value) == line("wrong_h_count") == "Invalid number of points in H"
        assert ref["cut_by_10"]["threw"] == "Reading out of bounds"
        with pytest.raises(gb.BellmanError, match="too short"):
            gb._import(key, rs[:-10], "x", DEV)
        with pytest.raises(gb.BellmanError, match="too short"):
            gb._contribute(curve, rs[:-10], "e", bytes(64), DEV)


def test_the_other_counts_and_the_circuit_hash_are_checked_in_the_references_order():
    curve = "bn128"
    cv = bv.curve_record(curve)
    key, rs = bv.gold(key_of(curve, "edge")), bv.gold("bellman_bn128_edge_response.params")
    _cv, _sec2, _d1, _d2, n_vars, n_public, domain, _body = gb._open_key(key)
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    at, places = 3 * s1 + 3 * s2, {}
    for what, size, n in (("IC", s1, n_public + 1), ("H", s1, domain - 1), ("L", s1, n_vars - n_public - 1), ("A", s1, n_vars), ("B1", s1, n_vars), ("B2", s2, n_vars)):
        assert struct.unpack_from(">I", rs, at)[0] == n, what
        places[what] = at
        at += 4 + n * size
    for what, where in places.items():
        bad = bytearray(rs)
        struct.pack_into(">I", bad, where, struct.unpack_from(">I", rs, where)[0] + 1)
        with pytest.raises(gb.BellmanError) as e:
            gb._import(key, bytes(bad), None, DEV)
        assert str(e.value) == f"Invalid number of points in {what}"
    bad = bytearray(rs)
    bad[at] ^= 1                                                              # csHash; the count of IC is wrong too, and the hash is looked at first
    struct.pack_into(">I", bad, places["IC"], 0)
    with pytest.raises(gb.BellmanError) as e:
        gb._import(key, bytes(bad), None, DEV)
    assert str(e.value) == "Hash of the original circuit does not match with the MPC one"


def test_entropy_and_random_bytes_are_refused_as_in_phase_2():
    ch = bv.gold("bellman_bn128_edge_challenge.params")
    with pytest.raises(gb.BellmanError, match="entropy must not be empty"):
        gb._contribute("bn128", ch, "", bytes(64), DEV)
    with pytest.raises(gb.BellmanError, match="random64 must be 64 bytes"):
        gb._contribute("bn128", ch, "e", bytes(63), DEV)
    with pytest.raises(gb.BellmanError, match="Curve not supported"):
        gb._contribute("secp256k1", ch, "e", bytes(64), DEV)


def test_fresh_randomness_gives_a_response_that_imports(tmp_path):
    """no recorded bytes: the response of os.urandom still appends one contribution whose hash is hashPubKey of it, and paths work as bytes do"""
    key = bv.gold(key_of("bn128", "edge"))
    ch = tmp_path / "challenge.params"
    ch.write_bytes(bv.gold("bellman_bn128_edge_challenge.params"))
    raw, h = gb._contribute("bn128", str(ch), "some entropy", None, DEV)
    assert raw != bv.gold("bellman_bn128_edge_response.params") and len(raw) == len(bv.gold("bellman_bn128_edge_response.params"))
    cv = bv.curve_record("bn128")
    cons = gb.parse_mpc_params(dict(bv.sections_of(gb._import(key, raw, None, DEV)))[10], cv)[1]
    assert len(cons) == 2 and "name" not in cons[1] and gb.contribution_hash(cv, cons[1]) == h


def test_the_drivers_without_a_device_fail_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(zkmi.ZkmiError) as e:
        gb.export_bellman(bv.gold(key_of("bn128", "edge")))
    assert e.value.code == zkmi.ERR_NO_DEVICE
