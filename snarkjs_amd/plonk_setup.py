"""PLONK setup on the device: snarkjs.plonk.setup (src/plonk_setup.js), byte for byte.

    zkey_bytes = setup(r1cs, ptau)          # each argument: bytes or a path

The gate lowering (sections 3 - 6, the selector columns, the permutation's predecessor map) is one host pass of the library
(include/zkmi.h: zkmi_plonk_setup_lower); sections 7 - 13 and the eight commitments of the header come from ONE device call (zkmi_plonk_setup;
kernels in csrc/plonk_setup.cuh). This module reads the slices of the two files that the reference reads (by offset: a large ptau is never loaded
whole), writes the header sections 1 and 2 and the tauG1 copy of section 14, and puts the 14 sections in the order the reference writes them.
"""
import struct

from . import _gate_setup as gate
from . import zkmi
from .groth16_setup import SetupError, _Source, log2, read_ptau_header, read_r1cs_header, read_sections

PROTOCOL_ID = 2
K1, K2 = gate.K1, gate.K2


def circuit_power(n_plonk_constraints):
    """cirPower of src/plonk_setup.js:74-75"""
    return max(3, log2(n_plonk_constraints - 1) + 1)


def lower(cv, hdr, constraints):
    """zkmi_plonk_setup_lower (host only, needs no device): the record of _gate_setup.lower, selectors Qm Ql Qr Qo Qc"""
    L = zkmi.lib()
    return gate.lower(cv, hdr, constraints, L.zkmi_plonk_setup_lower_len, L.zkmi_plonk_setup_lower)


def device_sections(cv, n_public, low, lagrange_g1):
    """zkmi_plonk_setup: dict q (five arrays: sections 7 - 11), sigma (12), lagrange (13), commitments (8 G1 points) as numpy uint8"""
    return gate.device_sections(cv, n_public, low, lagrange_g1, zkmi.PlonkSetupIn, zkmi.PlonkSetupOut, zkmi.lib().zkmi_plonk_setup, [("commitments", 8 * 2 * cv["n8q"])])


def header_sections(cv, n_public, low, commitments, x_2):
    """sections 1 and 2 (writeHeaders, src/plonk_setup.js:436-482)"""
    return struct.pack("<I", PROTOCOL_ID), gate.section2_head(cv, n_public, low) + bytes(commitments) + x_2


def open_inputs(r1cs_src, ptau_src):
    """What plonk.setup reads before it computes: (ptau, ptau sections, curve, power, r1cs, r1cs sections, r1cs header)"""
    ptau = _Source(ptau_src)
    r1 = _Source(r1cs_src)
    try:
        sp = read_sections(ptau, b"ptau")
        cv, power = read_ptau_header(ptau, sp)
        sr = read_sections(r1, b"r1cs")
        return ptau, sp, cv, power, r1, sr, read_r1cs_header(r1, sr)
    except Exception:
        ptau.close(); r1.close()
        raise


def lower_checked(ptau, sp, cv, power, r1, sr, hdr):
    """The lowering and the three refusals, in the reference's order (:62-87: it lowers the constraints before it compares the curves)"""
    if hdr["n8"] != 32:
        raise SetupError("r1cs curve does not match powers of tau ceremony curve")      # a field of another width: the lowering could not read it
    low = lower(cv, hdr, r1.read(*sr[2][0]))
    if hdr["prime"] != cv["r"]:
        raise SetupError("r1cs curve does not match powers of tau ceremony curve")
    cir_power = circuit_power(low["n_constraints"])
    assert low["domain_size"] == 1 << cir_power
    if cir_power > power:
        raise SetupError(f"circuit too big for this power of tau ceremony. {low['n_constraints']} > 2**{power}")
    if 12 not in sp:
        raise SetupError("Powers of tau is not prepared.")
    return low


def sections_14_and_x2(ptau, sp, cv, domain_size):
    return ptau.read(sp[2][0][0], (domain_size + 6) * 2 * cv["n8q"]), gate.read_x2(ptau, sp, cv)


def setup(r1cs, ptau):
    """snarkjs.plonk.setup(r1cs, ptau) -> zkey bytes. Raises SetupError, with the reference's log text, where the reference returns -1."""
    ptau_f, sp, cv, power, r1_f, sr, hdr = open_inputs(r1cs, ptau)
    try:
        low = lower_checked(ptau_f, sp, cv, power, r1_f, sr, hdr)
        n_public = hdr["nOutputs"] + hdr["nPubInputs"]
        dom, s_g1 = low["domain_size"], 2 * cv["n8q"]
        dev = device_sections(cv, n_public, low, ptau_f.read(sp[12][0][0] + (dom - 1) * s_g1, dom * s_g1))
        sec14, x_2 = sections_14_and_x2(ptau_f, sp, cv, dom)
        sec1, sec2 = header_sections(cv, n_public, low, dev["commitments"].tobytes(), x_2)
        body = [(3, low["additions"].tobytes()), (4, low["map_a"].tobytes()), (5, low["map_b"].tobytes()), (6, low["map_c"].tobytes())] + \
            [(7 + i, dev["q"][i].tobytes()) for i in range(5)] + [(12, dev["sigma"].tobytes()), (13, dev["lagrange"].tobytes()), (14, sec14), (1, sec1), (2, sec2)]
        return assemble_plonk(body)
    finally:
        ptau_f.close(); r1_f.close()


# createBinFile("zkey", 1, 14) with the sections in the order plonk.setup writes them: 3 - 14, then the two headers
assemble_plonk = gate.assemble_gate_zkey
