"""FFLONK setup (snarkjs_amd/fflonk_setup.py), the parts that need no device: the library's gate lowering against sections 3 - 6 and the header
counts of the reference's keys under tests/golden/fflonk_setup_* (tools/gen_fflonk_setup_golden.js), the selector columns and the predecessor map
against those keys' own coefficient sections (through the CPU oracle's transforms), sections 1, 2, 16 and 17, and what fflonk.setup refuses, in
which words and in which order."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import fflonk_setup as fs
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi
from test_groth16_setup_host import gold, sections_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P8, P12S = "setup_bn128_p8.ptau", "fflonk_setup_bn128_p12s.ptau"
# kind -> r1cs, ptau, rows, additions, domain (the reference's "Constraints:" and "Additions:" log lines)
FIXTURES = {
    "tiny": ("plonk_setup_bn128_tiny.r1cs", P8, 3, 0, 8),
    "quirks": ("fflonk_setup_bn128_quirks.r1cs", P8, 14, 9, 16),
    "rows30": ("fflonk_setup_bn128_rows30.r1cs", P8, 30, 0, 32),
    "mix": ("plonk_setup_bn128_mix.r1cs", P12S, 82, 39, 128),
    "edge": ("setup_bn128_edge.r1cs", P12S, 176, 64, 256),
}
KINDS = list(FIXTURES)
SIZES = {"tiny": 20060, "mix": 296456, "edge": 631160}
TOO_SMALL = "Powers of Tau is not big enough for this circuit size. Section 2 too small."
BN = gs.CURVES[next(k for k, c in gs.CURVES.items() if c["name"] == "bn128")]
R = BN["r"]


def key_of(kind):
    return gold(f"fflonk_setup_bn128_{kind}.zkey")


def fflonk_header(sec2):
    o = 4 + 32 + 4 + 32
    h = dict(zip(("nVars", "nPublic", "domainSize", "nAdditions", "nConstraints"), struct.unpack_from("<IIIII", sec2, o)))
    o += 20
    for name in ("k1", "k2", "w3", "w4", "w8", "wr"):
        h[name] = sec2[o:o + 32]
        o += 32
    h["X_2"], h["C0"] = sec2[o:o + 128], sec2[o + 128:]
    assert len(h["C0"]) == 64
    return h


def lowered(kind):
    r1cs, ptau = FIXTURES[kind][:2]
    ptau_f, sp, cv, r1, sr, hdr = fs.open_inputs(gold(r1cs), gold(ptau))
    try:
        return cv, hdr, fs.lower_checked(sp, cv, r1, sr, hdr)
    finally:
        ptau_f.close(); r1.close()


def from_mont_int(b):
    return int.from_bytes(b, "little") * pow(1 << 256, -1, R) % R


def test_the_golden_files_are_the_recorded_ones():
    index = json.load(open(os.path.join(GOLDEN, "fflonk_setup_golden.json")))
    for name, rec in index.items():
        if isinstance(rec, dict) and "sha256" in rec:
            assert hashlib.sha256(gold(name)).hexdigest() == rec["sha256"], name
    for kind, (r1cs, ptau, rows, adds, _dom) in FIXTURES.items():
        rec = index[f"fflonk_setup_bn128_{kind}.zkey"]
        assert (rec["r1cs"], rec["ptau"]) == (r1cs, ptau)
        assert rec["log"] == [f"Constraints:   {rows}", f"Additions:     {adds}"]
    for kind, size in SIZES.items():
        assert len(key_of(kind)) == size
    assert len(gold(P12S)) == 148968
    want = [("fflonk_setup_bn128_rows31.r1cs", P8), ("plonk_setup_bn128_mix.r1cs", P8), ("setup_bn128_edge.r1cs", P8), ("setup_bn128_full.r1cs", P8), ("setup_bn128_full.r1cs", P12S)]
    assert [(r["r1cs"], r["ptau"], r["message"]) for r in index["refused"]] == [(a, b, TOO_SMALL) for a, b in want]


def test_the_trimmed_ptau_holds_what_the_setup_reads_at_domain_256():
    src = gs._Source(gold(P12S))
    sp = gs.read_sections(src, b"ptau")
    assert sorted(sp) == [1, 2, 3, 12]
    assert gs.read_ptau_header(src, sp)[1] == 12
    assert (sp[2][0][1], sp[3][0][1], sp[12][0][1]) == ((9 * 256 + 18) * 64, 2 * 128, 0)


@pytest.mark.parametrize("kind", KINDS)
def test_lowering_against_sections_3_to_6_and_the_header_counts(kind):
    z = sections_of(key_of(kind), b"zkey")
    _r1cs, _ptau, rows, adds, dom = FIXTURES[kind]
    _cv, hdr, low = lowered(kind)
    h = fflonk_header(z[2])
    assert (low["plonk_n_vars"], low["n_additions"], low["n_constraints"], low["domain_size"]) == (h["nVars"], h["nAdditions"], h["nConstraints"], h["domainSize"])
    assert (low["n_constraints"], low["n_additions"], low["domain_size"]) == (rows, adds, dom) and h["nPublic"] == hdr["nOutputs"] + hdr["nPubInputs"]
    assert h["nVars"] == hdr["nVars"] + adds, "nVars of the header is the count after the lowering"
    assert low["additions"].tobytes() == z[3]
    assert low["map_a"].tobytes() == z[4] and low["map_b"].tobytes() == z[5] and low["map_c"].tobytes() == z[6]


def test_the_domain_keeps_two_rows_free():
    assert [fs.circuit_power(n) for n in (1, 6, 7, 14, 15, 30, 31, 62, 63)] == [3, 3, 4, 4, 5, 5, 6, 6, 7]


@pytest.mark.parametrize("kind", KINDS)
def test_selector_columns_are_the_transform_of_the_goldens_coefficients(kind):
    """Q = fft(coefficients of sections 7 - 11: QL QR QM QO QC), zero beyond the rows"""
    z = sections_of(key_of(kind), b"zkey")
    _cv, _hdr, low = lowered(kind)
    d, n_c = low["domain_size"], low["n_constraints"]
    sel = low["selectors"].reshape(5, n_c * 32)
    for i in range(5):
        assert len(z[7 + i]) == 5 * d * 32
        col = orc.ntt(0, np.frombuffer(z[7 + i][:d * 32], np.uint8)).tobytes()
        assert col[:n_c * 32] == sel[i].tobytes() and col[n_c * 32:] == bytes((d - n_c) * 32), f"section {7 + i}"


@pytest.mark.parametrize("kind", KINDS)
def test_predecessor_map_gives_the_goldens_sigma(kind):
    """sigma[p] = ident[pred[p]] with ident[col * n + i] = w^i {1, 2, 3}[col] is the transform of the coefficients of sections 12 - 14; the last two
    rows keep the identity, the rows between the constraints and them hold signal 0"""
    z = sections_of(key_of(kind), b"zkey")
    _cv, _hdr, low = lowered(kind)
    d, n_c, pred = low["domain_size"], low["n_constraints"], low["pred"]
    assert pred.size == 3 * d and sorted(pred.tolist()) == list(range(3 * d)), "the predecessor map is a permutation of the positions"
    for col in range(3):
        for i in (d - 2, d - 1):
            assert pred[col * d + i] == col * d + i
    filler = [col * d + i for i in range(n_c, d - 2) for col in range(3)]
    if kind == "rows30":
        assert not filler
    zero_cycle = {p for p in filler} | {col * d + i for col, m in enumerate(("map_a", "map_b", "map_c")) for i in range(n_c) if low[m][i] == 0}
    assert all(int(pred[p]) in zero_cycle for p in filler)
    w = int.from_bytes(orc.from_mont(0, orc.fr_w(0, d.bit_length() - 1)).tobytes(), "little")
    ident, x = [], 1
    for _ in range(d):
        ident.append(x); x = x * w % R
    ident = ident + [2 * v % R for v in ident] + [3 * v % R for v in ident]
    for col in range(3):
        assert len(z[12 + col]) == 5 * d * 32
        want = orc.from_mont(0, orc.ntt(0, np.frombuffer(z[12 + col][:d * 32], np.uint8))).tobytes()
        got = b"".join(ident[p].to_bytes(32, "little") for p in pred[col * d:(col + 1) * d])
        assert got == want, f"S{col + 1}"


def table_order(raw):
    order, off = [], 12
    while off < len(raw):
        typ, ln = struct.unpack_from("<IQ", raw, off)
        order.append(typ); off += 12 + ln
    return order


@pytest.mark.parametrize("kind", KINDS)
def test_sections_1_2_16_and_the_roots_against_the_golden(kind):
    raw = key_of(kind)
    z = sections_of(raw, b"zkey")
    r1cs, ptau = FIXTURES[kind][:2]
    ptau_f, sp, cv, r1, sr, hdr = fs.open_inputs(gold(r1cs), gold(ptau))
    try:
        low = fs.lower_checked(sp, cv, r1, sr, hdr)
        sec16, x_2 = fs.section_16_and_x2(ptau_f, sp, cv, low["domain_size"])
    finally:
        ptau_f.close(); r1.close()
    h = fflonk_header(z[2])
    d = low["domain_size"]
    power = d.bit_length() - 1
    assert sec16 == z[16] and len(sec16) == (9 * d + 18) * 64 and x_2 == h["X_2"]
    assert h["k1"] == ((2 << 256) % R).to_bytes(32, "little") and h["k2"] == ((3 << 256) % R).to_bytes(32, "little")
    w3, w4, w8, wr = (from_mont_int(h[k]) for k in ("w3", "w4", "w8", "wr"))
    assert (w3, w4, w8, wr) == fs.roots(power)
    assert pow(w3, 3, R) == 1 and w3 != 1
    assert pow(w4, 4, R) == 1 and pow(w4, 2, R) != 1
    assert pow(w8, 8, R) == 1 and pow(w8, 4, R) != 1
    fr_w = int.from_bytes(orc.from_mont(0, orc.fr_w(0, power)).tobytes(), "little")
    assert pow(wr, 3, R) == fr_w == fs.fr_root(power)
    # the headers are rebuilt from the lowering's counts around the golden's own commitment: that one is the device's part (tests/test_gpu_fflonk_setup.py)
    sec1, sec2 = fs.header_sections(cv, hdr["nOutputs"] + hdr["nPubInputs"], low, h["C0"], x_2)
    assert sec1 == z[1] == struct.pack("<I", 10) and sec2 == z[2]
    # the section table: the zkey header first, 3 .. 17, the FFLONK header last
    assert raw[:12] == b"zkey" + struct.pack("<II", 1, 17)
    order = table_order(raw)
    assert order == [1] + list(range(3, 18)) + [2]
    assert fs.assemble_fflonk([(t, z[t]) for t in order]) == raw


@pytest.mark.parametrize("kind", KINDS)
def test_section_17_interleaves_the_goldens_coefficients_with_qo_before_qm(kind):
    """C0[8 i + j] = coefficient i of (QL, QR, QO, QM, QC, S1, S2, S3)[j]: sections 7, 8, 10, 9, 11, 12, 13, 14"""
    z = sections_of(key_of(kind), b"zkey")
    d = fflonk_header(z[2])["domainSize"]
    assert len(z[17]) == 8 * d * 32
    c0 = np.frombuffer(z[17], np.uint8).reshape(d, 8, 32)
    for j, sec in enumerate((7, 8, 10, 9, 11, 12, 13, 14)):
        assert c0[:, j, :].tobytes() == z[sec][:d * 32], f"polynomial {j} is not section {sec}"
    assert z[9][:d * 32] != z[10][:d * 32], "QM and QO must differ for the order to show"


def ptau_of(sections):
    out = bytearray(b"ptau" + struct.pack("<II", 1, len(sections)))
    for typ, body in sections:
        out += struct.pack("<IQ", typ, len(body)) + body
    return bytes(out)


def ptau_header(curve="bn128", power=8):
    cv = next(c for c in gs.CURVES.values() if c["name"] == curve)
    q = next(k for k, c in gs.CURVES.items() if c is cv)
    return struct.pack("<I", cv["n8q"]) + q.to_bytes(cv["n8q"], "little") + struct.pack("<II", power, power)


def test_refusals_in_the_references_words_and_order():
    tiny, p8 = gold("plonk_setup_bn128_tiny.r1cs"), gold(P8)
    sp8 = sections_of(p8, b"ptau")
    # 1: section 12 comes before everything, the curves included
    with pytest.raises(gs.SetupError, match=r"^Powers of Tau is not well prepared\. Section 12 missing\.$"):
        fs.setup(gold("setup_bls12381_edge.r1cs"), ptau_of([(1, sp8[1]), (2, sp8[2]), (3, sp8[3])]))
    # 2: the curves, once the r1cs header is read, before the lowering (an r1cs that would not fit is refused for its curve)
    with pytest.raises(gs.SetupError, match=r"^r1cs curve does not match powers of tau ceremony curve$"):
        fs.setup(gold("setup_bls12381_full.r1cs"), p8)
    with pytest.raises(gs.SetupError, match=r"^r1cs curve does not match powers of tau ceremony curve$"):
        fs.setup(tiny, gold("setup_bls12381_p8.ptau"))
    # 3 and 4 after the lowering; section 2 before section 3
    short3 = [(1, sp8[1]), (2, sp8[2]), (3, sp8[3][:127]), (12, b"")]
    for r1cs, ptau in (("fflonk_setup_bn128_rows31.r1cs", p8), ("plonk_setup_bn128_mix.r1cs", p8), ("setup_bn128_edge.r1cs", p8), ("setup_bn128_full.r1cs", p8),
                       ("setup_bn128_full.r1cs", gold(P12S)), ("fflonk_setup_bn128_rows31.r1cs", ptau_of(short3))):
        with pytest.raises(gs.SetupError) as e:
            fs.setup(gold(r1cs), ptau)
        assert str(e.value) == TOO_SMALL, r1cs
    with pytest.raises(gs.SetupError, match=r"^Powers of Tau is not well prepared\. Section 3 too small\.$"):
        fs.setup(tiny, ptau_of(short3))
    with pytest.raises(gs.SetupError, match="Invalid File format"):
        fs.setup(tiny, tiny)


def test_rows30_fits_the_power_8_ceremony_and_one_row_more_does_not():
    """9 * 32 + 18 = 306 <= 511 < 9 * 64 + 18: the same circuit plus one row moves to domain 64"""
    from snarkjs_amd.workloads import synth_r1cs
    a, b = synth_r1cs.fflonk_rows_circuit("bn128", 30), synth_r1cs.fflonk_rows_circuit("bn128", 31)
    assert b[3][:-1] == a[3] and len(b[3]) == len(a[3]) + 1
    src = gs._Source(gold("fflonk_setup_bn128_rows31.r1cs"))
    sr = gs.read_sections(src, b"r1cs")
    low = fs.lower(BN, gs.read_r1cs_header(src, sr), src.read(*sr[2][0]))
    assert (low["n_constraints"], low["domain_size"]) == (31, 64)
    assert len(sections_of(gold(P8), b"ptau")[2]) == 511 * 64


def test_bls12381_is_refused_before_any_device_call():
    """right after the curve-mismatch check, by the driver and by every C entry (no device is initialised in this test)"""
    bls_r1cs, bls_ptau = gold("setup_bls12381_edge.r1cs"), gold("setup_bls12381_p8.ptau")
    with pytest.raises(gs.SetupError, match="not supported on BLS12-381"):
        fs.setup(bls_r1cs, bls_ptau)
    with pytest.raises(gs.SetupError, match="curve does not match"):
        fs.setup(gold("setup_bn128_edge.r1cs"), bls_ptau)
    L = zkmi.lib()
    src = gs._Source(bls_r1cs)
    sr = gs.read_sections(src, b"r1cs")
    hdr = gs.read_r1cs_header(src, sr)
    pg = zkmi.pages_of(src.read(*sr[2][0]))
    cnt = (zkmi.C.c_uint32 * 4)()
    unsupported = 4                                                     # ZKMI_ERR_UNSUPPORTED
    assert L.zkmi_fflonk_setup_lower_len(1, pg.pages, hdr["nConstraints"], hdr["nVars"], 2, cnt) == unsupported
    assert b"BN254 only" in L.zkmi_last_error()
    assert L.zkmi_fflonk_setup_lower(1, pg.pages, hdr["nConstraints"], hdr["nVars"], 2, zkmi.C.byref(zkmi.PlonkLowered())) == unsupported
    din = zkmi.FflonkSetupIn(1, 1, 3, 8, None, None, pg.pages)
    assert L.zkmi_fflonk_setup(zkmi.C.byref(din), zkmi.C.byref(zkmi.FflonkSetupOut())) == unsupported
    din.curve, din.domain_size, din.n_constraints = 0, 1 << 27, 1 << 26
    assert L.zkmi_fflonk_setup(zkmi.C.byref(din), zkmi.C.byref(zkmi.FflonkSetupOut())) == unsupported
    assert b"2^26" in L.zkmi_last_error()


def test_lowering_refuses_what_it_cannot_read_and_reads_odd_pages():
    _cv, hdr, low = lowered("mix")
    src = gs._Source(gold("plonk_setup_bn128_mix.r1cs"))
    cons = src.read(*gs.read_sections(src, b"r1cs")[2][0])
    with pytest.raises(zkmi.ZkmiError, match="fflonk_setup: the r1cs constraint section ends inside a constraint"):
        fs.lower(BN, hdr, cons[:-7])
    with pytest.raises(zkmi.ZkmiError, match="beyond nVars"):
        fs.lower(BN, dict(hdr, nVars=3), cons)
    with pytest.raises(zkmi.ZkmiError, match="nVars must exceed nPublic"):
        fs.lower(BN, dict(hdr, nOutputs=hdr["nVars"]), cons)
    # the constraint section in three pages cut at odd places: records straddle them
    paged = fs.lower(BN, hdr, [cons[:5], cons[5:1001], cons[1001:]])
    assert all(np.array_equal(low[k], paged[k]) for k in low)


def test_the_committed_r1cs_fixtures_are_what_the_generators_build():
    """tools/gen_fflonk_setup_golden.js regenerates them through tools/gen_fflonk_setup_r1cs.py; a generator edited without regenerating shows here"""
    from snarkjs_amd.workloads import synth_r1cs
    makes = (("quirks", synth_r1cs.fflonk_quirks_circuit("bn128")), ("rows30", synth_r1cs.fflonk_rows_circuit("bn128", 30)), ("rows31", synth_r1cs.fflonk_rows_circuit("bn128", 31)))
    for kind, circuit in makes:
        assert synth_r1cs.write_r1cs("bn128", *circuit) == gold(f"fflonk_setup_bn128_{kind}.r1cs"), kind


def test_setup_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(zkmi.ZkmiError) as e:
        fs.setup(gold("plonk_setup_bn128_tiny.r1cs"), gold(P8))
    assert e.value.code == zkmi.ERR_NO_DEVICE
