"""Groth16 setup (snarkjs_amd/groth16_setup.py), the parts that need no device: what newZKey refuses and in which words, the chunk ranges of
hashHPoints, sections 1, 2, 4 and 9 against the reference's keys under tests/golden/setup_* (tools/gen_setup_golden.js), and the circuit hash
recomputed from a golden key's own sections with the H differences taken from the CPU oracle."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi
from snarkjs_amd.workloads import synth_r1cs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(c, k) for c in ("bn128", "bls12381") for k in ("edge", "full")]


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def sections_of(data, magic):
    src = gs._Source(data)
    return {t: data[v[0][0]:v[0][0] + v[0][1]] for t, v in gs.read_sections(src, magic).items()}


def ptau_with(power, curve="bn128", prepared=True, tau_points=None):
    """a ptau container whose sections have the right lengths and hold zeros: enough for everything newZKey checks before it computes"""
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    q = next(k for k, c in gs.CURVES.items() if c is cv)
    s1 = 2 * cv["n8q"]
    secs = [(1, struct.pack("<I", cv["n8q"]) + q.to_bytes(cv["n8q"], "little") + struct.pack("<II", power, power)),
            (2, bytes(((2 << power) - 1 if tau_points is None else tau_points) * s1)), (4, bytes(s1)), (5, bytes(s1)), (6, bytes(2 * s1))]
    if prepared:
        secs.append((12, b""))
    out = bytearray(b"ptau" + struct.pack("<II", 1, len(secs)))
    for typ, body in secs:
        out += struct.pack("<IQ", typ, len(body)) + body
    return bytes(out)


def r1cs_with(curve, n_constraints, n_vars=4, n_public=1):
    """an r1cs whose HEADER announces n_constraints (the constraint section stays empty: the refusals come first)"""
    data = bytearray(synth_r1cs.write_r1cs(curve, n_vars, 1, n_public - 1, []))
    src = gs._Source(bytes(data))
    off = gs.read_sections(src, b"r1cs")[1][0][0]
    struct.pack_into("<I", data, off + 4 + 32 + 24, n_constraints)
    return bytes(data)


def test_refusals_in_the_references_words():
    ptau8 = gold("setup_bn128_p8.ptau")
    with pytest.raises(gs.SetupError, match="r1cs curve does not match powers of tau ceremony curve"):
        gs.open_inputs(gold("setup_bls12381_edge.r1cs"), ptau8)
    with pytest.raises(gs.SetupError, match=r"circuit too big for this power of tau ceremony\. 300\*2 > 2\*\*8"):
        gs.open_inputs(r1cs_with("bn128", 300), ptau8)
    with pytest.raises(gs.SetupError, match=r"Powers of tau is not prepared\."):
        gs.open_inputs(gold("setup_bn128_edge.r1cs"), ptau_with(8, prepared=False, tau_points=0))
    with pytest.raises(gs.SetupError, match="Circuit too big for this curve"):
        gs.open_inputs(r1cs_with("bn128", 1 << 28), ptau_with(30, tau_points=0))
    with pytest.raises(gs.SetupError, match="Invalid File format"):
        gs.open_inputs(gold("setup_bn128_edge.r1cs"), gold("setup_bn128_edge.r1cs"))
    # accepted: the same checks pass for the fixtures
    ptau, _sp, cv, power, r1, _sr, hdr, cir_power = gs.open_inputs(gold("setup_bn128_edge.r1cs"), ptau8)
    ptau.close(); r1.close()
    assert (cv["name"], power, cir_power, hdr["nConstraints"], hdr["nOutputs"] + hdr["nPubInputs"]) == ("bn128", 8, 7, 110, 2)


def test_domain_2p15_at_the_ceremony_power_is_refused_with_the_reason():
    """the one case of the hashHPoints quirk that is not imitated: the extra point lies past the end of the tauG1 section"""
    with pytest.raises(gs.SetupError, match="one point past"):
        gs.new_zkey(r1cs_with("bn128", 20000), ptau_with(15))
    # one power more in the ceremony and the same circuit passes the check (it then fails later, on the empty constraint section, in the library or for want of a device)
    with pytest.raises(Exception) as e:
        gs.new_zkey(r1cs_with("bn128", 20000), ptau_with(16))
    assert "one point past" not in str(e.value)


def literal_hash_h_ranges(domain_size):
    """hashHPoints of src/zkey_new.js:504-514, restated word for word"""
    CHUNK_SIZE = 1 << 14
    out = []
    i = 0
    while i < domain_size - 1:
        n = min(domain_size - 1, CHUNK_SIZE)
        out.append((i, n))
        i += CHUNK_SIZE
    return out


@pytest.mark.parametrize("power", list(range(1, 21)))
def test_hash_h_chunks_against_the_literal_loop(power):
    d = 1 << power
    assert gs.hash_h_chunks(d) == literal_hash_h_ranges(d)
    covered = [p for off, n in gs.hash_h_chunks(d) for p in range(off, off + n)] if power <= 16 else None
    want = d - 1 if power < 15 else d                         # the quirk: one point more from 2^15 on
    assert gs.hashed_h_points(d) == want
    if covered is not None:
        assert covered == list(range(want))


@pytest.mark.parametrize("curve,kind", CASES)
def test_sections_1_2_9_against_the_golden(curve, kind):
    z = sections_of(gold(f"setup_{curve}_{kind}.zkey"), b"zkey")
    ptau, sp, cv, _power, r1, _sr, hdr, cir_power = gs.open_inputs(gold(f"setup_{curve}_{kind}.r1cs"), gold(f"setup_{curve}_p8.ptau"))
    try:
        d, s1 = 1 << cir_power, 2 * cv["n8q"]
        assert cir_power == (7 if kind == "edge" else 8)
        sec1, sec2, _hdr_u = gs.header_sections(cv, hdr, d, ptau.read(sp[4][0][0], s1), ptau.read(sp[5][0][0], s1), ptau.read(sp[6][0][0], 2 * s1))
        assert sec1 == z[1] and sec2 == z[2]
        assert gs.read_h_section(ptau, sp, cv, cir_power, d) == z[9]
    finally:
        ptau.close(); r1.close()


@pytest.mark.parametrize("curve,kind", CASES)
def test_section_4_against_the_golden(curve, kind):
    """the library's one-pass parser (host side, no device): records in constraint order, A before B, the binding rows, values times R^2"""
    z = sections_of(gold(f"setup_{curve}_{kind}.zkey"), b"zkey")
    r1 = gold(f"setup_{curve}_{kind}.r1cs")
    src = gs._Source(r1)
    sr = gs.read_sections(src, b"r1cs")
    hdr = gs.read_r1cs_header(src, sr)
    cons = src.read(*sr[2][0])
    n_public = hdr["nOutputs"] + hdr["nPubInputs"]
    L = zkmi.lib()
    # the constraint section in three pages cut at odd places: records straddle them
    for pages in ([cons], [cons[:5], cons[5:1001], cons[1001:]]):
        pg = zkmi.pages_of(pages)
        n = C.c_size_t()
        assert L.zkmi_groth16_setup_coeffs_len(pg.pages, hdr["nConstraints"], n_public, C.byref(n)) == 0
        assert n.value == len(z[4])
        out = np.zeros(n.value, np.uint8)
        assert L.zkmi_groth16_setup_coeffs(zkmi.CURVE_ID[curve], pg.pages, hdr["nConstraints"], hdr["nVars"], n_public, zkmi.ptr(out), out.size) == 0
        assert out.tobytes() == z[4]
    # a truncated section and a signal beyond nVars are refused, not read past
    pg = zkmi.pages_of(cons[:-7])
    assert L.zkmi_groth16_setup_coeffs_len(pg.pages, hdr["nConstraints"], n_public, C.byref(n)) == 2 and b"ends inside a constraint" in L.zkmi_last_error()
    pg = zkmi.pages_of(cons)
    assert L.zkmi_groth16_setup_coeffs(zkmi.CURVE_ID[curve], pg.pages, hdr["nConstraints"], 3, n_public, zkmi.ptr(out), out.size) == 2
    assert b"beyond nVars" in L.zkmi_last_error()


def test_setup_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(zkmi.ZkmiError) as e:
        gs.new_zkey(gold("setup_bn128_edge.r1cs"), gold("setup_bn128_p8.ptau"))
    assert e.value.code == zkmi.ERR_NO_DEVICE


@pytest.mark.parametrize("curve,kind", CASES)
def test_circuit_hash_from_the_goldens_own_sections(curve, kind):
    """csHash fed in the reference's order reproduces section 10 of the reference's key; the H differences come from the CPU oracle"""
    cid = orc.CURVE_ID[curve]
    z = sections_of(gold(f"setup_{curve}_{kind}.zkey"), b"zkey")
    ptau, sp, cv, _power, r1, _sr, hdr, cir_power = gs.open_inputs(gold(f"setup_{curve}_{kind}.r1cs"), gold(f"setup_{curve}_p8.ptau"))
    try:
        d, s1 = 1 << cir_power, 2 * cv["n8q"]
        n_h = gs.hashed_h_points(d)
        assert n_h == d - 1
        tau = ptau.read(sp[2][0][0], (d + n_h) * s1)
        _s1, _s2, hdr_u = gs.header_sections(cv, hdr, d, ptau.read(sp[4][0][0], s1), ptau.read(sp[5][0][0], s1), ptau.read(sp[6][0][0], 2 * s1))
    finally:
        ptau.close(); r1.close()
    one_minus = (1).to_bytes(32, "little") + (cv["r"] - 1).to_bytes(32, "little")
    diffs = b"".join(orc.to_affine(cid, 1, orc.msm(cid, 1, tau[(i + d) * s1:(i + d + 1) * s1] + tau[i * s1:(i + 1) * s1], one_minus, 2)).tobytes() for i in range(n_h))
    u = lambda g, b: orc.group_convert(cid, g, "LEMtoU", b).tobytes()
    n_public = hdr["nOutputs"] + hdr["nPubInputs"]
    want = gs.circuit_hash(hdr_u, n_public, u(1, z[3]), d, u(1, diffs), u(1, z[8]), u(1, z[5]), u(1, z[6]), u(2, z[7]), s1)
    assert want == z[10][:64] and z[10][64:] == struct.pack("<I", 0)
    assert want.hex() == json.load(open(os.path.join(GOLDEN, "setup_golden.json")))[f"setup_{curve}_{kind}.zkey"]["csHash"]
    # the header points' host conversion agrees with the oracle's batchLEMtoU
    pts = z[2][-(2 + 2 + 4 + 4 + 2 + 4) * cv["n8q"]:]
    o, conv = 0, b""
    for g in (1, 1, 2, 2, 1, 2):
        conv += u(g, pts[o:o + 2 * g * cv["n8q"]]); o += 2 * g * cv["n8q"]
    assert conv == hdr_u
