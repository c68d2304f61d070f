"""FFLONK setup on the device: snarkjs.fflonk.setup (src/fflonk_setup.js), byte for byte, on BN254.

    zkey_bytes = setup(r1cs, ptau)          # each argument: bytes or a path

The gate lowering (sections 3 - 6, the selector columns, the permutation's predecessor map) is one host pass of the library
(include/zkmi.h: zkmi_fflonk_setup_lower); sections 7 - 15, the C0 polynomial of section 17 and its commitment come from ONE device call
(zkmi_fflonk_setup; kernels in csrc/plonk_setup.cuh and csrc/fflonk_setup.cuh). This module reads the slices of the two files that the reference
reads (by offset: a large ptau is never loaded whole), writes the header sections 1 and 2 and the tauG1 copy of section 16, and puts the 17
sections in the order the reference writes them: 1, 3 - 17, 2.

BLS12-381 is refused: the reference writes BN254's w3 and wr into such a key (tests/test_fflonk_bls_unsupported.py), so no proof exists under it.
"""
import struct

from . import _gate_setup as gate
from . import zkmi
from .groth16_setup import SetupError, _Source, log2, read_ptau_header, read_r1cs_header, read_sections

PROTOCOL_ID = 10
K1, K2 = gate.K1, gate.K2
BN128_R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
# computeW3 (:534-542) and getOmegaCubicRoot (:552-557), both hard-coded for BN254
W3_GENERATOR = 31624
W3_EXPONENT = 3648040478639879203707734290876212514758060733402672390616367364429301415936 // 3    # its "order(r - 1)" is (r - 1) / 6
WR_FIRST_ROOT = 467799165886069610036046866799264026481344299079011762026774533774345988080


def fr_root(i):
    """Fr.w[i] of ffjavascript on BN254: the 2^i-th root of unity that descends from 5^((r - 1) / 2^28)"""
    return pow(pow(5, (BN128_R - 1) >> 28, BN128_R), 1 << (28 - i), BN128_R)


def roots(power):
    """w3, w4, w8, wr of the header as integers (:139-148)"""
    return pow(W3_GENERATOR, W3_EXPONENT, BN128_R), fr_root(2), fr_root(3), pow(WR_FIRST_ROOT, 1 << (28 - power), BN128_R)


def circuit_power(n_rows):
    """cirPower of src/fflonk_setup.js:112"""
    return max(3, log2(n_rows + 1) + 1)


def lower(cv, hdr, constraints):
    """zkmi_fflonk_setup_lower (host only, needs no device): the record of _gate_setup.lower, selectors QL QR QM QO QC"""
    L = zkmi.lib()
    return gate.lower(cv, hdr, constraints, L.zkmi_fflonk_setup_lower_len, L.zkmi_fflonk_setup_lower)


def device_sections(cv, n_public, low, tau_g1):
    """zkmi_fflonk_setup: dict q (five arrays: sections 7 - 11), sigma (sections 12 - 14, one after the other), lagrange (15), c0 (17),
    commitment (one G1 point) as numpy uint8. tau_g1: the first 8 * domain_size points of ptau section 2."""
    return gate.device_sections(cv, n_public, low, tau_g1, zkmi.FflonkSetupIn, zkmi.FflonkSetupOut, zkmi.lib().zkmi_fflonk_setup,
                                [("c0", 8 * low["domain_size"] * 32), ("commitment", 2 * cv["n8q"])])


def header_sections(cv, n_public, low, commitment, x_2):
    """sections 1 and 2 (writeZkeyHeader :279-283, writeFFlonkHeader :466-503)"""
    sec2 = gate.section2_head(cv, n_public, low) + b"".join(gate.fr_mont(BN128_R, w) for w in roots(log2(low["domain_size"]))) + x_2 + bytes(commitment)
    return struct.pack("<I", PROTOCOL_ID), sec2


def open_inputs(r1cs_src, ptau_src):
    """What fflonk.setup reads before it computes, with its first two refusals and the one of this module, in the reference's order (:66-83):
    (ptau, ptau sections, curve, r1cs, r1cs sections, r1cs header)"""
    ptau = _Source(ptau_src)
    r1 = _Source(r1cs_src)
    try:
        sp = read_sections(ptau, b"ptau")
        if 12 not in sp:
            raise SetupError("Powers of Tau is not well prepared. Section 12 missing.")
        cv, _power = read_ptau_header(ptau, sp)
        sr = read_sections(r1, b"r1cs")
        hdr = read_r1cs_header(r1, sr)
        if hdr["prime"] != cv["r"]:
            raise SetupError("r1cs curve does not match powers of tau ceremony curve")
        if cv["r"] != BN128_R:
            raise SetupError("fflonk.setup is not supported on BLS12-381: the reference writes BN254's w3 and wr into the key, so no proof under it verifies")
        return ptau, sp, cv, r1, sr, hdr
    except Exception:
        ptau.close(); r1.close()
        raise


def lower_checked(sp, cv, r1, sr, hdr):
    """The lowering and the two refusals that follow it (:112-120)"""
    low = lower(cv, hdr, r1.read(*sr[2][0]))
    assert low["domain_size"] == 1 << circuit_power(low["n_constraints"])
    if sp[2][0][1] < (low["domain_size"] * 9 + 18) * 2 * cv["n8q"]:
        raise SetupError("Powers of Tau is not big enough for this circuit size. Section 2 too small.")
    if sp[3][0][1] < 4 * cv["n8q"]:
        raise SetupError("Powers of Tau is not well prepared. Section 3 too small.")
    return low


def section_16_and_x2(ptau, sp, cv, domain_size):
    return ptau.read(sp[2][0][0], (domain_size * 9 + 18) * 2 * cv["n8q"]), gate.read_x2(ptau, sp, cv)


def setup(r1cs, ptau):
    """snarkjs.fflonk.setup(r1cs, ptau) -> zkey bytes. Raises SetupError, with the reference's words, where the reference throws."""
    ptau_f, sp, cv, r1_f, sr, hdr = open_inputs(r1cs, ptau)
    try:
        low = lower_checked(sp, cv, r1_f, sr, hdr)
        n_public = hdr["nOutputs"] + hdr["nPubInputs"]
        dom, s_g1 = low["domain_size"], 2 * cv["n8q"]
        sec16, x_2 = section_16_and_x2(ptau_f, sp, cv, dom)
        dev = device_sections(cv, n_public, low, memoryview(sec16)[:8 * dom * s_g1])
        sec1, sec2 = header_sections(cv, n_public, low, dev["commitment"].tobytes(), x_2)
        rec = 5 * dom * 32
        body = [(1, sec1), (3, low["additions"].tobytes()), (4, low["map_a"].tobytes()), (5, low["map_b"].tobytes()), (6, low["map_c"].tobytes())] + \
            [(7 + i, dev["q"][i].tobytes()) for i in range(5)] + [(12 + i, dev["sigma"][i * rec:(i + 1) * rec].tobytes()) for i in range(3)] + \
            [(15, dev["lagrange"].tobytes()), (16, sec16), (17, dev["c0"].tobytes()), (2, sec2)]
        return assemble_fflonk(body)
    finally:
        ptau_f.close(); r1_f.close()


# createBinFile("zkey", 1, 17) with the sections in the order fflonk.setup writes them: 1, 3 - 17, then the FFLONK header
assemble_fflonk = gate.assemble_gate_zkey
