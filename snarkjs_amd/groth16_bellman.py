"""A Groth16 phase-2 key to a ceremony run with Bellman-format tooling and back, on the device: snarkjs.zKey.exportBellman (src/zkey_export_bellman.js),
zKey.bellmanContribute (src/zkey_bellman_contribute.js) and zKey.importBellman (src/zkey_import_bellman.js), byte for byte.

    params = export_bellman(zkey)                                                        # zkey, params: bytes or a path
    response, contribution_hash = bellman_contribute(curve_name, challenge, entropy, random64=None)
    new_zkey = import_bellman(zkey_old, mpc_params, name=None)

A parameter file is alpha1, beta1, beta2, gamma2, delta1, delta2, then IC, H, L, A, B1, B2 each as a big-endian count and its points, then csHash, a big-endian
count and per contribution deltaAfter, g1_s, g1_sx, g2_spx and the transcript; every point uncompressed, big-endian, normal form. H is not section 9 of the key
but its image under a group FFT and a per-point twist (domainSize - 1 points): ONE library call each way (include/zkmi.h: zkmi_bellman_h_section; kernels in
csrc/bellman.cuh). The other sections go through zkmi_group_convert, the 1 / delta of a contribution over H and L through
zkmi_ptau_challenge_section (U in, U out). The key pair, hashToG2 and the few header points are the host calls of groth16_phase2. Export followed by import is not
the identity on section 9: the coefficient export drops comes back as zero (the reference's behaviour). importBellman does not verify the contributions, and
neither does this: groth16_phase2_verify does. random64 (default os.urandom(64)) is what the reference draws from getRandomValues."""
import ctypes as C
import hashlib
import os
import struct

import numpy as np

from . import zkmi
from .groth16_phase2 import (Phase2Error, contribution_hash, fr_inverse_mont, hash_pub_key, hash_to_g2, key_from_seed, parse_mpc_params, point_mul, read_header,
                             seed_from_entropy, serialise_mpc_params)
from .groth16_setup import SetupError, _Source, lem_to_u_host, read_sections
from .powersoftau_challenge import _bytes_of, _curve, _u_to_lem_host
from .powersoftau_verify import PtauError


class BellmanError(Phase2Error):
    """exportBellman / bellmanContribute / importBellman refused the inputs (the reference throws, or logs the message and returns false)"""


def _out(n_bytes):
    o = np.zeros(max(n_bytes, 1), np.uint8)
    return o, [(C.c_void_p * 1)(o.ctypes.data), (C.c_size_t * 1)(n_bytes), 1]


class Device:
    """the three steps that need the device; tests/test_bellman_host.py puts the CPU oracle in their place"""

    def convert(self, cv, group, kind, body):
        """zkmi_group_convert over a whole section: kind = zkmi.CONV_LEM_TO_U or zkmi.CONV_U_TO_LEM"""
        s_g = 2 * group * cv["n8q"]
        n = len(body) // s_g
        if not n:
            return b""
        zkmi.init()
        o, arg = _out(n * s_g)
        zkmi.check(zkmi.lib().zkmi_group_convert(cv["id"], group, kind, zkmi.pages_of(body).pages, *arg, n))
        return o[:n * s_g].tobytes()

    def h_section(self, cv, body, power, direction):
        """zkmi_bellman_h_section: direction 0 takes the 2^power LEM points of section 9 to 2^power - 1 U points, direction 1 takes them back"""
        zkmi.init()
        n = (1 << power) - (0 if direction else 1)
        o, arg = _out(n * 2 * cv["n8q"])
        zkmi.check(zkmi.lib().zkmi_bellman_h_section(cv["id"], zkmi.pages_of(body).pages, power, direction, *arg))
        return o[:n * 2 * cv["n8q"]].tobytes()

    def scale_u(self, cv, body_u, k_mont):
        """k P for every point of a G1 section in U form, U out: zkmi_ptau_challenge_section with first = k, inc = 1"""
        n = len(body_u) // (2 * cv["n8q"])
        if not n:
            return b""
        zkmi.init()
        k, one = np.frombuffer(bytes(k_mont), np.uint8), np.frombuffer(((1 << 256) % cv["r"]).to_bytes(32, "little"), np.uint8)
        o, arg = _out(len(body_u))
        zkmi.check(zkmi.lib().zkmi_ptau_challenge_section(cv["id"], 1, zkmi.pages_of(body_u).pages, n, zkmi.ptr(k), zkmi.ptr(one), *arg, 1))
        return o[:len(body_u)].tobytes()


def _open_key(zkey):
    """the header and the bodies of sections 3 - 10 of a Groth16 key -> (cv, sec2, at_delta1, at_delta2, n_vars, n_public, domain_size, body)"""
    src = _Source(zkey)
    try:
        try:
            sections = read_sections(src, b"zkey", 2)
            cv, sec2, at_d1, at_d2 = read_header(src, sections)
        except SetupError as e:
            raise BellmanError(str(e)) from None
        except Phase2Error as e:
            raise BellmanError(str(e)) from None
        body = {t: src.read(*sections[t][0]) for t in range(3, 11)}
    finally:
        src.close()
    n_vars, n_public, domain_size = struct.unpack_from("<III", sec2, at_d1 - 6 * 2 * cv["n8q"] - 12)
    return cv, sec2, at_d1, at_d2, n_vars, n_public, domain_size, body


def _power(domain_size):
    if domain_size < 1 or domain_size & (domain_size - 1):
        raise BellmanError("the key's domainSize is not a power of two")
    return domain_size.bit_length() - 1


def _contributions_u(cv, contributions):
    """the contribution records of a parameter file"""
    return b"".join(lem_to_u_host(cv, c["deltaAfter"], 1) + lem_to_u_host(cv, c["g1_s"], 1) + lem_to_u_host(cv, c["g1_sx"], 1) + lem_to_u_host(cv, c["g2_spx"], 2) + c["transcript"]
                    for c in contributions)


class _Reader:
    """a parameter file read front to back; a read past its end is the reference's `Reading out of bounds`"""

    def __init__(self, data):
        self.data, self.pos = data, 0

    def read(self, n):
        if n < 0 or self.pos + n > len(self.data):
            raise BellmanError("the parameter file is too short for the sizes it declares (the reference: Reading out of bounds)")
        self.pos += n
        return self.data[self.pos - n:self.pos]

    def u32be(self):
        return struct.unpack(">I", self.read(4))[0]

    def contributions(self, cv):
        """csHash, the count and the records -> (csHash, contributions with LEM points as parse_mpc_params gives them)"""
        s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
        cs_hash, out = self.read(64), []
        for _ in range(self.u32be()):
            c = {k: _u_to_lem_host(cv, self.read(s1 * g), g) for k, g in (("deltaAfter", 1), ("g1_s", 1), ("g1_sx", 1), ("g2_spx", 2))}
            c["transcript"] = self.read(64)
            out.append(c)
        return cs_hash, out


def _export(zkey, dev):
    cv, sec2, at_d1, _at_d2, _n_vars, _n_public, domain_size, body = _open_key(zkey)
    s1 = 2 * cv["n8q"]
    at = at_d1 - 6 * s1                                                       # alpha1, beta1, beta2, gamma2, delta1, delta2: 3 G1 and 3 G2 points
    out = []
    for group in (1, 1, 2, 2, 1, 2):
        out.append(lem_to_u_host(cv, sec2[at:at + s1 * group], group))
        at += s1 * group
    cs_hash, contributions = parse_mpc_params(body[10], cv)

    def points(group, u):
        out.extend([struct.pack(">I", len(u) // (s1 * group)), u])
    points(1, dev.convert(cv, 1, zkmi.CONV_LEM_TO_U, body[3]))
    if len(body[9]) != domain_size * s1:
        raise BellmanError("section 9 does not hold domainSize points")
    points(1, dev.h_section(cv, body[9], _power(domain_size), 0))
    for t, group in ((8, 1), (5, 1), (6, 1), (7, 2)):
        points(group, dev.convert(cv, group, zkmi.CONV_LEM_TO_U, body[t]))
    out += [cs_hash, struct.pack(">I", len(contributions)), _contributions_u(cv, contributions)]
    return b"".join(out)


def _contribute(curve_name, challenge, entropy, random64, dev):
    try:
        cv = _curve(curve_name)
    except PtauError as e:
        raise BellmanError(str(e)) from None
    if not entropy:
        raise BellmanError("entropy must not be empty (the reference asks for it until it is)")
    random64 = os.urandom(64) if random64 is None else bytes(random64)
    if len(random64) != 64:
        raise BellmanError("random64 must be 64 bytes")
    rd = _Reader(_bytes_of(challenge))
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    prv, g1_s, g1_sx = key_from_seed(cv, seed_from_entropy(random64, entropy))
    inv_delta = fr_inverse_mont(cv, prv)
    out = [rd.read(s1 + s1 + s2 + s2)]                                        # alpha1, beta1, beta2, gamma2
    delta1 = point_mul(cv, 1, _u_to_lem_host(cv, rd.read(s1), 1), prv)
    delta2 = point_mul(cv, 2, _u_to_lem_host(cv, rd.read(s2), 2), prv)
    out += [lem_to_u_host(cv, delta1, 1), lem_to_u_host(cv, delta2, 2)]
    for what, size in (("IC", s1), ("H", s1), ("L", s1), ("A", s1), ("B1", s1), ("B2", s2)):
        n = rd.u32be()
        pts = rd.read(n * size)
        out += [struct.pack(">I", n), dev.scale_u(cv, pts, inv_delta) if what in ("H", "L") else pts]
    cs_hash, contributions = rd.contributions(cv)
    transcript = hashlib.blake2b(digest_size=64)
    transcript.update(cs_hash)
    for c in contributions:
        hash_pub_key(transcript, cv, c)
    transcript.update(lem_to_u_host(cv, g1_s, 1))
    transcript.update(lem_to_u_host(cv, g1_sx, 1))
    cur = dict(deltaAfter=delta1, g1_s=g1_s, g1_sx=g1_sx, transcript=transcript.digest(), type=0)
    cur["g2_spx"] = point_mul(cv, 2, hash_to_g2(cv, cur["transcript"]), prv)
    contributions.append(cur)
    out += [cs_hash, struct.pack(">I", len(contributions)), _contributions_u(cv, contributions)]
    return b"".join(out), contribution_hash(cv, cur)


def _import(zkey_old, mpc_params, name, dev):
    cv, sec2, at_d1, _at_d2, n_vars, n_public, domain_size, body = _open_key(zkey_old)
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    old_hash, old = parse_mpc_params(body[10], cv)
    data = _bytes_of(mpc_params)
    # the reference reads the contributions first, at the place the KEY's sizes put them, then the sections front to back
    rd = _Reader(data)
    rd.read(3 * s1 + 3 * s2 + 8 + s1 * n_vars + 4 + s1 * (domain_size - 1) + 4 + s1 * n_vars + 4 + s1 * n_vars + 4 + s2 * n_vars)
    new_hash, new = rd.contributions(cv)
    if new_hash != old_hash:
        raise BellmanError("Hash of the original circuit does not match with the MPC one")
    if len(old) > len(new):
        raise BellmanError("The impoerted file does not include new contributions")
    for i, (a, b) in enumerate(zip(old, new)):
        if any(a[k] != b[k] for k in ("deltaAfter", "g1_s", "g1_sx", "g2_spx", "transcript")):
            raise BellmanError(f"Previous contribution {i} does not match")
        b["type"] = a["type"]
        for k in ("beaconHash", "numIterationsExp", "name"):
            if k in a:
                b[k] = a[k]
    if name:
        for c in new[len(old):]:
            c["name"] = name
    sec10 = serialise_mpc_params(new_hash, new)
    rd = _Reader(data)
    rd.read(s1 + s1 + s2 + s2)                                                # alpha1, beta1, beta2, gamma2: the key keeps its own
    delta1, delta2 = _u_to_lem_host(cv, rd.read(s1), 1), _u_to_lem_host(cv, rd.read(s2), 2)
    taken = {}
    for what, size, want in (("IC", s1, n_public + 1), ("H", s1, domain_size - 1), ("L", s1, n_vars - n_public - 1), ("A", s1, n_vars), ("B1", s1, n_vars), ("B2", s2, n_vars)):
        if rd.u32be() != want:
            raise BellmanError(f"Invalid number of points in {what}")
        taken[what] = rd.read(want * size)
    h = dev.h_section(cv, taken["H"], _power(domain_size), 1)
    ell = dev.convert(cv, 1, zkmi.CONV_U_TO_LEM, taken["L"])
    out = [(1, struct.pack("<I", 1)), (2, sec2[:at_d1] + delta1 + delta2), (3, body[3]), (4, body[4]), (9, h), (8, ell), (5, body[5]), (6, body[6]), (7, body[7]), (10, sec10)]
    raw = [b"zkey", struct.pack("<II", 1, 10)]
    for typ, b in out:
        raw += [struct.pack("<IQ", typ, len(b)), b]
    return b"".join(raw)


def _finish(raw, path):
    if path is not None:
        with open(path, "wb") as f:
            f.write(raw)
    return raw


def export_bellman(zkey, mpc_params=None):
    """snarkjs.zKey.exportBellman(zkey, mpcparams) -> the parameter file's bytes (also written to mpc_params when it is a path)"""
    return _finish(_export(zkey, Device()), mpc_params)


def bellman_contribute(curve_name, challenge, entropy, random64=None, response=None):
    """snarkjs.zKey.bellmanContribute(curve, challenge, response, entropy) -> (response bytes, contribution hash)"""
    raw, h = _contribute(curve_name, challenge, entropy, random64, Device())
    return _finish(raw, response), h


def import_bellman(zkey_old, mpc_params, name=None, zkey_new=None):
    """snarkjs.zKey.importBellman(zkeyOld, mpcparams, zkeyNew, name) -> the new key's bytes; where the reference logs an error and returns false, BellmanError
    carries that line"""
    return _finish(_import(zkey_old, mpc_params, name, Device()), zkey_new)
