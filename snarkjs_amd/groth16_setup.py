"""Groth16 setup on the device: snarkjs.zKey.newZKey (src/zkey_new.js), byte for byte.

    zkey_bytes, cs_hash = new_zkey(r1cs, ptau)          # each argument: bytes or a path

The point sections 3, 5, 6, 7, 8, the coefficient section 4 and the H points of the circuit hash come from ONE library call
(include/zkmi.h: zkmi_groth16_setup; kernels in csrc/groth16_setup.cuh); this module reads the slices of the two files that
newZKey reads (by offset: a large ptau is never loaded whole), writes the header sections 1, 2, the H section 9 (a copy of ptau
points) and the contribution section 10, and feeds the circuit hash in the reference's order. Nothing here computes on curve points
except the six header points' change of format (O(1), Python integers).
"""
import ctypes as C
import hashlib
import os
import struct

import numpy as np

from . import zkmi

CURVES = {
    21888242871839275222246405745257275088696311157297823662689037894645226208583: dict(
        name="bn128", id=0, n8q=32, s=28,
        r=21888242871839275222246405745257275088548364400416034343698204186575808495617,
        g1=(1, 2),
        g2=((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
            (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))),
    0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab: dict(
        name="bls12381", id=1, n8q=48, s=32,
        r=52435875175126190479447740508185965837690552500527637822603658699938581184513,
        g1=(0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
            0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1),
        g2=((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
             0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
            (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
             0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be))),
}
HASH_CHUNK = 1 << 14          # CHUNK_SIZE of hashHPoints (src/zkey_new.js:505)


class SetupError(ValueError):
    """newZKey refused the inputs (the reference logs the message and returns -1, or throws)"""


class _Source:
    """bytes or a file, read by offset"""

    def __init__(self, src):
        self.data = None if isinstance(src, (str, os.PathLike)) else memoryview(bytes(src) if not isinstance(src, (bytes, bytearray, memoryview)) else src)
        self.f = open(src, "rb") if self.data is None else None
        self.size = os.fstat(self.f.fileno()).st_size if self.f else len(self.data)

    def read(self, off, n):
        if off < 0 or n < 0 or off + n > self.size:
            raise SetupError("read beyond the end of the file")
        if self.f is None:
            return bytes(self.data[off:off + n])
        self.f.seek(off)
        return self.f.read(n)

    def close(self):
        if self.f:
            self.f.close()


def read_sections(src, magic, max_version=1):
    """@iden3/binfileutils readBinFile: section type -> [(offset, length)], from the section headers alone"""
    head = src.read(0, 12) if src.size >= 12 else b""
    if len(head) < 12 or head[:4] != magic:
        raise SetupError(f"{magic.decode()}: Invalid File format")
    version, n_sections = struct.unpack_from("<II", head, 4)
    if version > max_version:
        raise SetupError("Version not supported")
    sections, off = {}, 12
    for _ in range(n_sections):
        typ, ln = struct.unpack("<IQ", src.read(off, 12))
        off += 12
        sections.setdefault(typ, []).append((off, ln))
        off += ln
    if off > src.size:
        raise SetupError("read beyond the end of the file")
    return sections


def read_ptau_header(src, sections):
    """src/powersoftau_utils.js readPTauHeader: (curve record, power)"""
    if 1 not in sections:
        raise SetupError(f"{src}: File has no  header")
    off, ln = sections[1][0]
    n8 = struct.unpack("<I", src.read(off, 4))[0]
    q = int.from_bytes(src.read(off + 4, n8), "little")
    if q not in CURVES:
        raise SetupError(f"Curve not supported: {q}")
    cv = CURVES[q]
    if cv["n8q"] != n8:
        raise SetupError("Invalid size")
    power, _ceremony_power = struct.unpack("<II", src.read(off + 4 + n8, 8))
    return cv, power


def read_r1cs_header(src, sections):
    """r1csfile readR1csHeader"""
    off, _ln = sections[1][0]
    n8 = struct.unpack("<I", src.read(off, 4))[0]
    prime = int.from_bytes(src.read(off + 4, n8), "little")
    n_vars, n_outputs, n_pub, n_prv, n_labels, n_constraints = struct.unpack("<IIIIQI", src.read(off + 4 + n8, 28))
    return dict(n8=n8, prime=prime, nVars=n_vars, nOutputs=n_outputs, nPubInputs=n_pub, nPrvInputs=n_prv, nLabels=n_labels, nConstraints=n_constraints)


def log2(v):
    """src/misc.js log2 (position of the top bit of a 32-bit value)"""
    return v.bit_length() - 1 if v > 0 else 0


def circuit_power(r1cs):
    return log2(r1cs["nConstraints"] + r1cs["nPubInputs"] + r1cs["nOutputs"] + 1 - 1) + 1


def hash_h_chunks(domain_size):
    """The (offset, count) ranges hashHPoints feeds to the circuit hash (src/zkey_new.js:504-514). The reference takes
    n = min(domainSize - 1, CHUNK_SIZE) for EVERY chunk, not for the last one what is left: from domainSize = 2^15 on the last chunk ends at
    point domainSize - 1, one past the domainSize - 1 points announced."""
    n = min(domain_size - 1, HASH_CHUNK)
    return [(i, n) for i in range(0, domain_size - 1, HASH_CHUNK)]


def hashed_h_points(domain_size):
    ch = hash_h_chunks(domain_size)
    return ch[-1][0] + ch[-1][1] if ch else 0


def _fq_lem(cv, v):
    q = next(k for k, c in CURVES.items() if c is cv)
    return ((v << (8 * cv["n8q"])) % q).to_bytes(cv["n8q"], "little")


def generators_lem(cv):
    """curve.G1.g, curve.G2.g as toRprLEM writes them"""
    g1 = b"".join(_fq_lem(cv, v) for v in cv["g1"])
    g2 = b"".join(_fq_lem(cv, v) for xy in cv["g2"] for v in xy)
    return g1, g2


def lem_to_u_host(cv, buf, group):
    """batchLEMtoU for a handful of header points (Python integers): big-endian normal form, an Fq2 coordinate as c1 || c0"""
    q = next(k for k, c in CURVES.items() if c is cv)
    n8 = cv["n8q"]
    rinv = pow(1 << (8 * n8), -1, q)
    el = [(int.from_bytes(buf[i:i + n8], "little") * rinv % q).to_bytes(n8, "big") for i in range(0, len(buf), n8)]
    if group == 2:
        el = [el[i ^ 1] for i in range(len(el))]
    return b"".join(el)


def _u32be(v):
    return struct.pack(">I", v)


def circuit_hash(header_u, n_public, ic_u, domain_size, h_u, c_u, a_u, b1_u, b2_u, s_g1):
    """csHash of newZKey from the uncompressed forms, in the reference's order; h_u holds hashed_h_points(domain_size) points"""
    h = hashlib.blake2b(digest_size=64)
    h.update(header_u)
    h.update(_u32be(n_public + 1)); h.update(ic_u)
    h.update(_u32be(domain_size - 1))
    hv = memoryview(h_u)
    for off, n in hash_h_chunks(domain_size):
        h.update(hv[off * s_g1:(off + n) * s_g1])
    for sec, sz in ((c_u, s_g1), (a_u, s_g1), (b1_u, s_g1), (b2_u, 2 * s_g1)):
        h.update(_u32be(len(sec) // sz)); h.update(sec)
    return h.digest()


def header_sections(cv, r1cs, domain_size, alpha1, beta1, beta2):
    """sections 1 and 2 of the new key and the uncompressed header points that open the circuit hash"""
    q = next(k for k, c in CURVES.items() if c is cv)
    n_public = r1cs["nOutputs"] + r1cs["nPubInputs"]
    g1, g2 = generators_lem(cv)
    sec2 = struct.pack("<I", cv["n8q"]) + q.to_bytes(cv["n8q"], "little") + struct.pack("<I", 32) + cv["r"].to_bytes(32, "little") + \
        struct.pack("<III", r1cs["nVars"], n_public, domain_size) + alpha1 + beta1 + beta2 + g2 + g1 + g2
    hdr_u = lem_to_u_host(cv, alpha1, 1) + lem_to_u_host(cv, beta1, 1) + lem_to_u_host(cv, beta2, 2) + lem_to_u_host(cv, g2, 2) + lem_to_u_host(cv, g1, 1) + \
        lem_to_u_host(cv, g2, 2)
    return struct.pack("<I", 1), sec2, hdr_u


def read_h_section(ptau, sections, cv, cir_power, domain_size):
    """writeHs (src/zkey_new.js:182-201): the odd-indexed points of the 2 * domainSize Lagrange basis"""
    s_g1 = 2 * cv["n8q"]
    base = sections[12][0][0]
    if cir_power < cv["s"]:
        buf = np.frombuffer(ptau.read(base + (domain_size * 2 - 1) * s_g1, domain_size * 2 * s_g1), np.uint8).reshape(domain_size, 2, s_g1)
        return buf[:, 1, :].tobytes()
    if cir_power == cv["s"]:
        return ptau.read(base + ((1 << (cir_power + 1)) - 1) * s_g1 + domain_size * s_g1, domain_size * s_g1)
    raise SetupError("Circuit too big for this curve")


def open_inputs(r1cs_src, ptau_src):
    """Everything newZKey checks before it computes: (ptau, ptau sections, curve, power, r1cs, r1cs sections, header, cirPower). Raises SetupError
    with the reference's message where the reference logs it and returns -1."""
    ptau = _Source(ptau_src)
    r1 = _Source(r1cs_src)
    try:
        sp = read_sections(ptau, b"ptau")
        cv, power = read_ptau_header(ptau, sp)
        sr = read_sections(r1, b"r1cs")
        hdr = read_r1cs_header(r1, sr)
        if hdr["prime"] != cv["r"]:
            raise SetupError("r1cs curve does not match powers of tau ceremony curve")
        cir_power = circuit_power(hdr)
        if cir_power > power:
            raise SetupError(f"circuit too big for this power of tau ceremony. {hdr['nConstraints']}*2 > 2**{power}")
        if 12 not in sp:
            raise SetupError("Powers of tau is not prepared.")
        if cir_power > cv["s"]:
            raise SetupError("Circuit too big for this curve")
        return ptau, sp, cv, power, r1, sr, hdr, cir_power
    except Exception:
        ptau.close(); r1.close()
        raise


def assemble(sections):
    """createBinFile("zkey", 1, 10) with the sections in the order newZKey writes them"""
    out = [b"zkey", struct.pack("<II", 1, 10)]
    for typ, body in sections:
        out.append(struct.pack("<IQ", typ, len(body)))
        out.append(body)
    return b"".join(out)


def device_sections(cv, hdr, domain_size, n_h, constraints, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, tau_powers):
    """zkmi_groth16_setup: dict ic, coeffs, a, b1, b2, c, h (numpy uint8)"""
    zkmi.init()
    L = zkmi.lib()
    n_public = hdr["nOutputs"] + hdr["nPubInputs"]
    s_g1 = 2 * cv["n8q"]
    hold = [zkmi.pages_of(b) for b in (constraints, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, tau_powers)]
    din = zkmi.Groth16SetupIn(cv["id"], hdr["nConstraints"], hdr["nVars"], n_public, domain_size, n_h, *[h.pages for h in hold])
    n4 = C.c_size_t()
    zkmi.check(L.zkmi_groth16_setup_coeffs_len(hold[0].pages, hdr["nConstraints"], n_public, C.byref(n4)))
    lens = dict(ic=(n_public + 1) * s_g1, coeffs=n4.value, a=hdr["nVars"] * s_g1, b1=hdr["nVars"] * s_g1, b2=hdr["nVars"] * 2 * s_g1,
                c=(hdr["nVars"] - n_public - 1) * s_g1, h=n_h * s_g1)
    bufs = {k: np.zeros(max(v, 1), np.uint8) for k, v in lens.items()}
    dout = zkmi.Groth16SetupOut(*[bufs[k].ctypes.data for k in ("ic", "coeffs", "a", "b1", "b2", "c", "h")], *[lens[k] for k in ("ic", "coeffs", "a", "b1", "b2", "c", "h")])
    zkmi.check(L.zkmi_groth16_setup(C.byref(din), C.byref(dout)))
    return {k: bufs[k][:lens[k]] for k in lens}


def _to_u(cv, group, buf):
    n = len(buf) // (2 * group * cv["n8q"])
    if n == 0:
        return b""
    pg = zkmi.pages_of(buf)
    out = np.empty(len(buf), np.uint8)
    op, ol = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(out.size)
    zkmi.check(zkmi.lib().zkmi_group_convert(cv["id"], group, zkmi.CONV_LEM_TO_U, pg.pages, op, ol, 1, n))
    return out.tobytes()


def new_zkey(r1cs, ptau):
    """snarkjs.zKey.newZKey(r1cs, ptau) -> (zkey bytes, csHash). Raises SetupError where the reference refuses."""
    ptau_f, sp, cv, power, r1_f, sr, hdr, cir_power = open_inputs(r1cs, ptau)
    try:
        domain_size = 1 << cir_power
        n_public = hdr["nOutputs"] + hdr["nPubInputs"]
        s_g1, s_g2 = 2 * cv["n8q"], 4 * cv["n8q"]
        n_h = hashed_h_points(domain_size)
        tau_points = sp[2][0][1] // s_g1
        if domain_size + n_h > tau_points:
            raise SetupError(f"domainSize 2^{cir_power} equals the ceremony's power: from 2^15 on the reference's circuit hash takes H point {domain_size - 1}, which lies one point past "
                             "the end of the ptau's tauG1 section (it hashes bytes of the next section's header); refused rather than imitated")
        alpha1 = ptau_f.read(sp[4][0][0], s_g1)
        beta1 = ptau_f.read(sp[5][0][0], s_g1)
        beta2 = ptau_f.read(sp[6][0][0], s_g2)
        sec1, sec2, hdr_u = header_sections(cv, hdr, domain_size, alpha1, beta1, beta2)
        constraints = r1_f.read(*sr[2][0])

        def lagrange(typ, sz):
            return ptau_f.read(sp[typ][0][0] + (domain_size - 1) * sz, domain_size * sz)
        dev = device_sections(cv, hdr, domain_size, n_h, constraints, lagrange(12, s_g1), lagrange(13, s_g2), lagrange(14, s_g1), lagrange(15, s_g1),
                              ptau_f.read(sp[2][0][0], (domain_size + n_h) * s_g1))
        sec9 = read_h_section(ptau_f, sp, cv, cir_power, domain_size)
        cs_hash = circuit_hash(hdr_u, n_public, _to_u(cv, 1, dev["ic"]), domain_size, dev["h"].tobytes(), _to_u(cv, 1, dev["c"]), _to_u(cv, 1, dev["a"]),
                               _to_u(cv, 1, dev["b1"]), _to_u(cv, 2, dev["b2"]), s_g1)
        zkey = assemble([(1, sec1), (2, sec2), (4, dev["coeffs"].tobytes()), (3, dev["ic"].tobytes()), (9, sec9), (8, dev["c"].tobytes()), (5, dev["a"].tobytes()),
                         (6, dev["b1"].tobytes()), (7, dev["b2"].tobytes()), (10, cs_hash + struct.pack("<I", 0))])
        return zkey, cs_hash
    finally:
        ptau_f.close(); r1_f.close()
