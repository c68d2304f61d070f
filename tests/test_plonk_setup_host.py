"""PLONK setup (snarkjs_amd/plonk_setup.py), the parts that need no device: the library's gate lowering against sections 3 - 6 and the header
counts of the reference's keys under tests/golden/plonk_setup_* (tools/gen_plonk_setup_golden.js), the selector columns and the predecessor map
against those keys' own coefficient and sigma sections (through the CPU oracle's transforms), sections 1, 2 and 14, and what plonk.setup refuses
and in which words."""
import json
import os
import struct

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import plonk_setup as ps
from snarkjs_amd import zkmi
from test_groth16_setup_host import gold, ptau_with, sections_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(c, k) for c in ("bn128", "bls12381") for k in ("edge", "mix", "tiny")]
# PLONK constraints and domainSize the reference reported for every fixture (its log line "Plonk constraints: N")
ROWS = {("bn128", "edge"): 178, ("bls12381", "edge"): 178, ("bn128", "mix"): 92, ("bls12381", "mix"): 134, ("bn128", "tiny"): 3, ("bls12381", "tiny"): 3}


def r1cs_of(curve, kind):
    return gold(f"setup_{curve}_edge.r1cs" if kind == "edge" else f"plonk_setup_{curve}_{kind}.r1cs")


def plonk_header(sec2, cv):
    o = 4 + cv["n8q"] + 4 + 32
    names = ("nVars", "nPublic", "domainSize", "nAdditions", "nConstraints")
    h = dict(zip(names, struct.unpack_from("<IIIII", sec2, o)))
    o += 20
    h["k1"], h["k2"] = sec2[o:o + 32], sec2[o + 32:o + 64]
    o += 64
    s1 = 2 * cv["n8q"]
    h["commitments"] = sec2[o:o + 8 * s1]
    h["X_2"] = sec2[o + 8 * s1:]
    return h


def lowered(curve, kind):
    ptau, sp, cv, power, r1, sr, hdr = ps.open_inputs(r1cs_of(curve, kind), gold(f"setup_{curve}_p8.ptau"))
    try:
        return cv, hdr, ps.lower_checked(ptau, sp, cv, power, r1, sr, hdr)
    finally:
        ptau.close(); r1.close()


def test_the_golden_files_are_the_recorded_ones():
    import hashlib
    index = json.load(open(os.path.join(GOLDEN, "plonk_setup_golden.json")))
    for name, rec in index.items():
        if "sha256" in rec:
            assert hashlib.sha256(gold(name)).hexdigest() == rec["sha256"], name
    for curve, kind in CASES:
        assert index[f"plonk_setup_{curve}_{kind}.zkey"]["log"] == [f"Plonk constraints: {ROWS[curve, kind]}"]
    assert len(gold("plonk_setup_bn128_edge.zkey")) == 434236 and len(gold("plonk_setup_bls12381_edge.zkey")) == 442956


@pytest.mark.parametrize("curve,kind", CASES)
def test_lowering_against_sections_3_to_6_and_the_header_counts(curve, kind):
    z = sections_of(gold(f"plonk_setup_{curve}_{kind}.zkey"), b"zkey")
    cv, hdr, low = lowered(curve, kind)
    h = plonk_header(z[2], cv)
    assert (low["plonk_n_vars"], low["n_additions"], low["n_constraints"], low["domain_size"]) == (h["nVars"], h["nAdditions"], h["nConstraints"], h["domainSize"])
    assert low["n_constraints"] == ROWS[curve, kind] and h["nPublic"] == hdr["nOutputs"] + hdr["nPubInputs"]
    assert low["domain_size"] == 1 << max(3, (ROWS[curve, kind] - 1).bit_length())
    assert low["additions"].tobytes() == z[3]
    assert low["map_a"].tobytes() == z[4] and low["map_b"].tobytes() == z[5] and low["map_c"].tobytes() == z[6]


@pytest.mark.parametrize("curve,kind", CASES)
def test_selector_columns_are_the_transform_of_the_goldens_coefficients(curve, kind):
    """Q = fft(coefficients of sections 7 - 11), zero beyond the PLONK constraints"""
    cid = orc.CURVE_ID[curve]
    z = sections_of(gold(f"plonk_setup_{curve}_{kind}.zkey"), b"zkey")
    _cv, _hdr, low = lowered(curve, kind)
    d, n_c = low["domain_size"], low["n_constraints"]
    sel = low["selectors"].reshape(5, n_c * 32)
    for i in range(5):
        col = orc.ntt(cid, np.frombuffer(z[7 + i][:d * 32], np.uint8)).tobytes()
        assert col[:n_c * 32] == sel[i].tobytes() and col[n_c * 32:] == bytes((d - n_c) * 32), f"section {7 + i}"


@pytest.mark.parametrize("curve,kind", CASES)
def test_predecessor_map_gives_the_goldens_sigma(curve, kind):
    """sigma[p] = ident[pred[p]] with ident[col * n + i] = w^i {1, 2, 3}[col] is the transform of section 12's coefficients"""
    cid = orc.CURVE_ID[curve]
    z = sections_of(gold(f"plonk_setup_{curve}_{kind}.zkey"), b"zkey")
    cv, _hdr, low = lowered(curve, kind)
    d, r = low["domain_size"], cv["r"]
    assert low["pred"].size == 3 * d and int(low["pred"].max()) < 3 * d
    assert sorted(low["pred"].tolist()) == list(range(3 * d)), "the predecessor map is a permutation of the positions"
    w = int.from_bytes(orc.from_mont(cid, orc.fr_w(cid, d.bit_length() - 1)).tobytes(), "little")
    ident, x = [], 1
    for _ in range(d):
        ident.append(x); x = x * w % r
    ident = ident + [2 * v % r for v in ident] + [3 * v % r for v in ident]
    for col in range(3):
        want = orc.from_mont(cid, orc.ntt(cid, np.frombuffer(z[12][col * 5 * d * 32:(col * 5 + 1) * d * 32], np.uint8))).tobytes()
        got = b"".join(ident[p].to_bytes(32, "little") for p in low["pred"][col * d:(col + 1) * d])
        assert got == want, f"S{col + 1}"


@pytest.mark.parametrize("curve,kind", CASES)
def test_sections_1_2_14_against_the_golden(curve, kind):
    z = sections_of(gold(f"plonk_setup_{curve}_{kind}.zkey"), b"zkey")
    ptau, sp, cv, power, r1, sr, hdr = ps.open_inputs(r1cs_of(curve, kind), gold(f"setup_{curve}_p8.ptau"))
    try:
        low = ps.lower_checked(ptau, sp, cv, power, r1, sr, hdr)
        sec14, x_2 = ps.sections_14_and_x2(ptau, sp, cv, low["domain_size"])
    finally:
        ptau.close(); r1.close()
    h = plonk_header(z[2], cv)
    assert sec14 == z[14] and x_2 == h["X_2"]
    assert h["k1"] == ((2 << 256) % cv["r"]).to_bytes(32, "little") and h["k2"] == ((3 << 256) % cv["r"]).to_bytes(32, "little")
    # the header is rebuilt from the lowering's counts; the eight commitments are the device's part (tests/test_gpu_plonk_setup.py)
    sec1, sec2 = ps.header_sections(cv, hdr["nOutputs"] + hdr["nPubInputs"], low, h["commitments"], x_2)
    assert sec1 == z[1] == struct.pack("<I", 2) and sec2 == z[2]
    # the section table: 3 .. 14 first, the two headers last
    raw = gold(f"plonk_setup_{curve}_{kind}.zkey")
    assert raw[:12] == b"zkey" + struct.pack("<II", 1, 14)
    order, off = [], 12
    while off < len(raw):
        typ, ln = struct.unpack_from("<IQ", raw, off)
        order.append(typ); off += 12 + ln
    assert order == list(range(3, 15)) + [1, 2]
    assert ps.assemble_plonk([(t, z[t]) for t in order]) == raw


def test_lowering_refuses_what_it_cannot_read():
    cv, hdr, _low = lowered("bn128", "mix")
    src = gs._Source(r1cs_of("bn128", "mix"))
    cons = src.read(*gs.read_sections(src, b"r1cs")[2][0])
    with pytest.raises(zkmi.ZkmiError, match="ends inside a constraint"):
        ps.lower(cv, hdr, cons[:-7])
    with pytest.raises(zkmi.ZkmiError, match="beyond nVars"):
        ps.lower(cv, dict(hdr, nVars=3), cons)
    # the constraint section in three pages cut at odd places: records straddle them
    a, b = ps.lower(cv, hdr, cons), ps.lower(cv, hdr, [cons[:5], cons[5:1001], cons[1001:]])
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_deviations_from_the_reader_and_coefficients_of_r_or_more():
    """The reference's reader takes any 32 bytes (F.fromRprLE = toMontgomery of the raw value, which keeps c mod r); it does not compare nVars
    with nPublic, which the lowering refuses on purpose (csrc/gate_setup.hpp: lower)"""
    from snarkjs_amd.workloads import synth_r1cs
    for curve in ("bn128", "bls12381"):
        cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
        r, top = cv["r"], (1 << 256) - 1

        def low(coefs):
            a, b, c, d = coefs
            cons = [([(1, a), (2, b)], [(0, c), (3, 1)], [(2, d), (4, 1), (1, a)]), ([(0, d)], [(2, b), (3, 1)], [(4, c)])]
            data = synth_r1cs.write_r1cs(curve, 5, 1, 0, cons)
            src = gs._Source(data)
            sr = gs.read_sections(src, b"r1cs")
            return ps.lower(cv, gs.read_r1cs_header(src, sr), src.read(*sr[2][0]))
        raw, reduced = low((r + 5, top, r, 4 * r + 1 if 4 * r + 1 <= top else 2 * r + 1)), low((5, top % r, 0, 1))
        assert all(np.array_equal(raw[k], reduced[k]) for k in raw)
        assert int.from_bytes(raw["selectors"][-32:].tobytes(), "little") < r
    cv, hdr, _low = lowered("bn128", "tiny")
    src = gs._Source(r1cs_of("bn128", "tiny"))
    cons = src.read(*gs.read_sections(src, b"r1cs")[2][0])
    with pytest.raises(zkmi.ZkmiError, match="nVars must exceed nPublic"):
        ps.lower(cv, dict(hdr, nOutputs=hdr["nVars"]), cons)


def test_the_committed_r1cs_fixtures_are_what_the_generators_build():
    """tools/gen_plonk_setup_golden.js regenerates them through tools/gen_plonk_setup_r1cs.py; a generator edited without regenerating shows here"""
    from snarkjs_amd.workloads import synth_r1cs
    for curve in ("bn128", "bls12381"):
        for kind, make in (("mix", synth_r1cs.plonk_mix_circuit), ("tiny", synth_r1cs.plonk_tiny_circuit)):
            assert synth_r1cs.write_r1cs(curve, *make(curve)) == gold(f"plonk_setup_{curve}_{kind}.r1cs"), (curve, kind)


def test_refusals_in_the_references_words():
    index = json.load(open(os.path.join(GOLDEN, "plonk_setup_golden.json")))
    with pytest.raises(gs.SetupError, match="r1cs curve does not match powers of tau ceremony curve"):
        ps.setup(gold("setup_bls12381_edge.r1cs"), gold("setup_bn128_p8.ptau"))
    for curve, rows in (("bn128", 1268), ("bls12381", 1283)):
        text = f"circuit too big for this power of tau ceremony. {rows} > 2**8"
        assert index[f"setup_{curve}_full.r1cs"]["refused"] == text
        with pytest.raises(gs.SetupError) as e:
            ps.setup(gold(f"setup_{curve}_full.r1cs"), gold(f"setup_{curve}_p8.ptau"))
        assert str(e.value) == text
    with pytest.raises(gs.SetupError, match=r"^Powers of tau is not prepared\.$"):
        ps.setup(gold("setup_bn128_edge.r1cs"), ptau_with(8, prepared=False, tau_points=0))
    with pytest.raises(gs.SetupError, match="Invalid File format"):
        ps.setup(gold("setup_bn128_edge.r1cs"), gold("setup_bn128_edge.r1cs"))


def test_setup_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(zkmi.ZkmiError) as e:
        ps.setup(gold("setup_bn128_edge.r1cs"), gold("setup_bn128_p8.ptau"))
    assert e.value.code == zkmi.ERR_NO_DEVICE
