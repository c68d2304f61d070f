"""Phase 2 of a Groth16 ceremony on the device: snarkjs.zKey.contribute (src/zkey_contribute.js) and zKey.beacon (src/zkey_beacon.js), byte for byte.

    new_zkey, contribution_hash = contribute(zkey, name, entropy)                          # zkey: bytes or a path
    new_zkey, contribution_hash = beacon(zkey, name, beacon_hash_hex, num_iterations_exp)

The two point sections a contribution rewrites, L (8) and H (9) times 1 / delta, come from ONE library call each (include/zkmi.h: zkmi_group_scale; kernel in
csrc/group_scale.cuh). The key pair, hashToG2 and the four header and public-key points are O(1) host work in the library (zkmi_phase2_key_from_seed,
zkmi_phase2_hash_to_g2, zkmi_point_mul: the reference's ChaCha generator and its fromRng, restated). This module hashes, reads and writes: the transcript in
the reference's order, the header, the copied sections 3 - 7 and the MPC parameters of section 10.
"""
import ctypes as C
import hashlib
import os
import struct

import numpy as np

from . import zkmi
from .groth16_setup import CURVES, SetupError, _Source, lem_to_u_host, read_sections


class Phase2Error(ValueError):
    """zKey.contribute / zKey.beacon refused the inputs (the reference throws, or logs the message and returns false)"""


def _curve_of(q):
    if q not in CURVES:
        raise Phase2Error(f"Curve not supported: {q}")
    return CURVES[q]


def read_header(src, sections):
    """zkey_utils.readHeader for a Groth16 key: the curve record, the raw bytes of section 2 and the offsets of delta1 / delta2 in them"""
    off, ln = sections[1][0]
    if struct.unpack("<I", src.read(off, 4))[0] != 1:
        raise Phase2Error("zkey file is not groth16")
    off, ln = sections[2][0]
    sec2 = src.read(off, ln)
    n8q = struct.unpack_from("<I", sec2, 0)[0]
    cv = _curve_of(int.from_bytes(sec2[4:4 + n8q], "little"))
    o = 4 + n8q + 4 + struct.unpack_from("<I", sec2, 4 + n8q)[0] + 12
    s1, s2 = 2 * n8q, 4 * n8q
    at_delta1 = o + s1 + s1 + s2 + s2               # alpha1, beta1, beta2, gamma2
    if len(sec2) != at_delta1 + s1 + s2:
        raise Phase2Error("zkey header has an unexpected length")
    return cv, sec2, at_delta1, at_delta1 + s1


def _js_name(name):
    """c.name.substring(0, 64) as TextEncoder writes it: 64 UTF-16 code units, a surrogate cut off from its partner becomes U+FFFD"""
    units = name.encode("utf-16-le", "surrogatepass")[:128]
    return units.decode("utf-16-le", "replace").encode("utf-8")


def parse_mpc_params(sec10, cv):
    """zkey_utils.readMPCParams: (csHash, contributions); points as the affine Montgomery bytes of the file"""
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    cs_hash, n = sec10[:64], struct.unpack_from("<I", sec10, 64)[0]
    o, out = 68, []
    for _ in range(n):
        c = dict(deltaAfter=sec10[o:o + s1], g1_s=sec10[o + s1:o + 2 * s1], g1_sx=sec10[o + 2 * s1:o + 3 * s1], g2_spx=sec10[o + 3 * s1:o + 3 * s1 + s2])
        o += 3 * s1 + s2
        c["transcript"] = sec10[o:o + 64]
        c["type"], plen = struct.unpack_from("<II", sec10, o + 64)
        o += 72
        end, last = o + plen, 0
        while o < end:
            typ = sec10[o]
            if typ <= last:
                raise Phase2Error("Parameters in the contribution must be sorted")
            last = typ
            if typ == 1:
                c["name"] = sec10[o + 2:o + 2 + sec10[o + 1]].decode("utf-8", "replace")
                o += 2 + sec10[o + 1]
            elif typ == 2:
                c["numIterationsExp"] = sec10[o + 1]
                o += 2
            elif typ == 3:
                c["beaconHash"] = sec10[o + 2:o + 2 + sec10[o + 1]]
                o += 2 + sec10[o + 1]
            else:
                raise Phase2Error("Parameter not recognized")
        if o != end:
            raise Phase2Error("Parameters do not match")
        out.append(c)
    if o != len(sec10):
        raise Phase2Error("MPC parameter section has bytes left over")
    return cs_hash, out


def serialise_mpc_params(cs_hash, contributions):
    """zkey_utils.writeMPCParams"""
    out = [cs_hash, struct.pack("<I", len(contributions))]
    for c in contributions:
        out += [c["deltaAfter"], c["g1_s"], c["g1_sx"], c["g2_spx"], c["transcript"], struct.pack("<I", c.get("type") or 0)]
        params = b""
        if c.get("name"):
            name = _js_name(c["name"])
            if len(name) > 255:
                raise Phase2Error("the name's UTF-8 encoding exceeds the 255 bytes its one-byte length field can state")
            params += bytes([1, len(name)]) + name
        if c.get("type") == 1:
            params += bytes([2, c["numIterationsExp"], 3, len(c["beaconHash"])]) + bytes(c["beaconHash"])
        out += [struct.pack("<I", len(params)), params]
    return b"".join(out)


def hash_pub_key(hasher, cv, c):
    """zkey_utils.hashPubKey: the four public points in uncompressed form, then the transcript"""
    for k, group in (("deltaAfter", 1), ("g1_s", 1), ("g1_sx", 1), ("g2_spx", 2)):
        hasher.update(lem_to_u_host(cv, c[k], group))
    hasher.update(c["transcript"])


def contribution_hash(cv, c):
    h = hashlib.blake2b(digest_size=64)
    hash_pub_key(h, cv, c)
    return h.digest()


def seed_from_entropy(random64, entropy):
    """misc.getRandomRng: Blake2b-512 over the 64 random bytes and the UTF-8 entropy; the seed is its first eight big-endian words"""
    h = hashlib.blake2b(bytes(random64) + entropy.encode("utf-8"), digest_size=64).digest()
    return list(struct.unpack(">8I", h[:32]))


def seed_from_beacon(beacon_hash, num_iterations_exp):
    """misc.rngFromBeaconParams: 2^numIterationsExp nested SHA-256"""
    cur = bytes(beacon_hash)
    for _ in range(1 << num_iterations_exp):
        cur = hashlib.sha256(cur).digest()
    return list(struct.unpack(">8I", cur))


def _arr(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def key_from_seed(cv, seed):
    """(prvKey, g1_s, g1_sx): Fr.fromRng, G1.fromRng and their product from ChaCha(seed)"""
    s1 = 2 * cv["n8q"]
    prv, g1_s, g1_sx = np.zeros(32, np.uint8), np.zeros(s1, np.uint8), np.zeros(s1, np.uint8)
    zkmi.check(zkmi.lib().zkmi_phase2_key_from_seed(cv["id"], (C.c_uint32 * 8)(*seed), zkmi.ptr(prv), zkmi.ptr(g1_s), zkmi.ptr(g1_sx)))
    return prv.tobytes(), g1_s.tobytes(), g1_sx.tobytes()


def hash_to_g2(cv, transcript):
    out, t = np.zeros(4 * cv["n8q"], np.uint8), _arr(transcript)
    zkmi.check(zkmi.lib().zkmi_phase2_hash_to_g2(cv["id"], zkmi.ptr(t), zkmi.ptr(out)))
    return out.tobytes()


def point_mul(cv, group, point, k_mont):
    p, k, out = _arr(point), _arr(k_mont), np.zeros(2 * group * cv["n8q"], np.uint8)
    zkmi.check(zkmi.lib().zkmi_point_mul(cv["id"], group, zkmi.ptr(p), zkmi.ptr(k), zkmi.ptr(out)))
    return out.tobytes()


def fr_inverse_mont(cv, k_mont):
    """Fr.inv on a Montgomery element"""
    r = cv["r"]
    k = int.from_bytes(k_mont, "little") * pow(1 << 256, -1, r) % r
    return (pow(k, -1, r) * (1 << 256) % r).to_bytes(32, "little")


def scale_section(cv, body, k_mont):
    """(k P) for every point of a G1 section: zkmi_group_scale, the whole section in one call"""
    n = len(body) // (2 * cv["n8q"])
    if n == 0:
        return b""
    zkmi.init()
    pg, k = zkmi.pages_of(body), _arr(k_mont)
    out = np.empty(len(body), np.uint8)
    op, ol = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(out.size)
    zkmi.check(zkmi.lib().zkmi_group_scale(cv["id"], 1, pg.pages, op, ol, 1, n, zkmi.ptr(k)))
    return out.tobytes()


def _apply(zkey, name, seed, extra, scale=scale_section):
    """One contribution from ChaCha(seed): (new key bytes, contribution hash). extra: the type and, for a beacon, its parameters. scale is the one step that needs
    the device; tests/test_phase2_host.py passes the CPU oracle's batchApplyKey(k, 1) there to hold every other byte to the reference without a device."""
    src = _Source(zkey)
    try:
        try:
            sections = read_sections(src, b"zkey", 2)
        except SetupError as e:
            raise Phase2Error(str(e)) from None
        cv, sec2, at_d1, at_d2 = read_header(src, sections)
        body = {t: src.read(*sections[t][0]) for t in range(3, 11)}
    finally:
        src.close()
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    cs_hash, contributions = parse_mpc_params(body[10], cv)
    transcript = hashlib.blake2b(digest_size=64)
    transcript.update(cs_hash)
    for c in contributions:
        hash_pub_key(transcript, cv, c)
    prv, g1_s, g1_sx = key_from_seed(cv, seed)
    transcript.update(lem_to_u_host(cv, g1_s, 1))
    transcript.update(lem_to_u_host(cv, g1_sx, 1))
    cur = dict(g1_s=g1_s, g1_sx=g1_sx, transcript=transcript.digest())
    cur["g2_spx"] = point_mul(cv, 2, hash_to_g2(cv, cur["transcript"]), prv)
    delta1 = point_mul(cv, 1, sec2[at_d1:at_d1 + s1], prv)
    delta2 = point_mul(cv, 2, sec2[at_d2:at_d2 + s2], prv)
    cur["deltaAfter"] = delta1
    cur.update(extra)
    if name:
        cur["name"] = name
    contributions.append(cur)
    sec10 = serialise_mpc_params(cs_hash, contributions)                       # before the device work: an over-long name is refused first
    inv_delta = fr_inverse_mont(cv, prv)
    out = [(1, struct.pack("<I", 1)), (2, sec2[:at_d1] + delta1 + delta2)] + [(t, body[t]) for t in range(3, 8)]
    out += [(8, scale(cv, body[8], inv_delta)), (9, scale(cv, body[9], inv_delta)), (10, sec10)]
    raw = [b"zkey", struct.pack("<II", 1, 10)]
    for typ, b in out:
        raw += [struct.pack("<IQ", typ, len(b)), b]
    return b"".join(raw), contribution_hash(cv, cur)


def contribute(zkey, name, entropy, random64=None):
    """snarkjs.zKey.contribute(zkey, new, name, entropy) -> (new zkey bytes, contribution hash). random64: the 64 bytes the reference draws from
    getRandomValues (default os.urandom(64)); passing them reproduces a run."""
    if not entropy:
        raise Phase2Error("entropy must not be empty (the reference asks for it until it is)")
    random64 = os.urandom(64) if random64 is None else bytes(random64)
    if len(random64) != 64:
        raise Phase2Error("random64 must be 64 bytes")
    return _apply(zkey, name, seed_from_entropy(random64, entropy), dict(type=0))


def beacon(zkey, name, beacon_hash_hex, num_iterations_exp):
    """snarkjs.zKey.beacon(zkey, new, name, beaconHash, numIterationsExp) -> (new zkey bytes, contribution hash)"""
    text = beacon_hash_hex[2:] if beacon_hash_hex[:2] in ("0x", "0X") else beacon_hash_hex
    try:
        beacon_hash = bytes.fromhex(text) if text.isalnum() else b""
    except ValueError:
        beacon_hash = b""
    if not beacon_hash or 2 * len(beacon_hash) != len(beacon_hash_hex):
        raise Phase2Error("Invalid Beacon Hash. (It must be a valid hexadecimal sequence)")
    if len(beacon_hash) >= 256:
        raise Phase2Error("Maximum length of beacon hash is 255 bytes")
    num_iterations_exp = int(num_iterations_exp)
    if num_iterations_exp < 10 or num_iterations_exp > 63:
        raise Phase2Error("Invalid numIterationsExp. (Must be between 10 and 63)")
    return _apply(zkey, name, seed_from_beacon(beacon_hash, num_iterations_exp), dict(type=1, numIterationsExp=num_iterations_exp, beaconHash=beacon_hash))
