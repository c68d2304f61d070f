"""Phase 1 of a ceremony on the device: powersOfTau.newAccumulator (src/powersoftau_new.js), powersOfTau.contribute (src/powersoftau_contribute.js) and
powersOfTau.beacon (src/powersoftau_beacon.js), byte for byte.

    raw, first_challenge_hash = new_accumulator(curve_name, power, new_ptau=None, logger=None)
    raw, response_hash = contribute(old_ptau, name, entropy, new_ptau=None, logger=None, random64=None)          # old_ptau: bytes or a path
    raw, response_hash = beacon(old_ptau, name, beacon_hash_hex, num_iterations_exp, new_ptau=None, logger=None)  # or False where the reference returns false

Each returns the new file's bytes and also writes them when a path is given. A contribution multiplies point i of sections 2 - 5 by first * inc^i, with
(first, inc) = (1, tau), (1, tau), (alpha, tau), (beta, tau), and the one point of section 6 by beta. Everything on the points of a section is ONE library call
(include/zkmi.h: zkmi_ptau_contribute_section): from one upload the new points as the file holds them (LEM), in C form (the bytes of the response
hash) and in U form (the bytes of the next challenge hash). The key pair, hashToG2, the point of section 6 and the public key are O(1) host work in the library
(zkmi_ptau_key_from_seed, zkmi_phase2_hash_to_g2, zkmi_point_mul). This module hashes, reads and writes. The 216 bytes a contribution keeps of its response
hasher (misc.toPartialHash) hold the hasher's block buffer, whose stale bytes depend on how the data was cut into `update` calls: zkmi_blake2b512_partial takes
the reference's cuts, the challenge hash and then chunks of floor(2^20 / sG) points of C form, section by section. logger(level, text) receives the reference's
info, warn and error lines (its debug progress lines are not reproduced; new_accumulator logs its debug and info lines). random64 (default os.urandom(64)) is
what the reference draws from getRandomValues; passing it reproduces a run. At power 0 section 2 holds a single point and the reference fails on the second
one it wants for the contribution record (a TypeError on an undefined point): PtauError here.
"""
import ctypes as C
import hashlib
import os
import re
import struct

import numpy as np

from . import zkmi
from .groth16_phase2 import _js_name, point_mul, seed_from_beacon, seed_from_entropy
from .groth16_phase2_verify import format_hash
from .groth16_setup import CURVES, _Source, generators_lem, lem_to_u_host
from .powersoftau_prepare import _file, _finish, _header, _open
from .powersoftau_verify import PtauError, _g2sp, _read_contributions, first_challenge_hash

_REDUCED = "This file has been reduced. You cannot contribute into a reduced file."


class Device:
    """the one call that needs the device; tests/test_ptau_contribute_host.py puts the CPU oracle in its place"""

    def contribute_section(self, cv, group, body, n, first, inc):
        """body: the n affine LEM points of a section; first, inc: Montgomery Fr bytes -> (LEM, C, U) bytes of (first * inc^i) P_i"""
        zkmi.init()
        s_g = 2 * group * cv["n8q"]
        pg = zkmi.pages_of(body)
        f, i = np.frombuffer(bytes(first), np.uint8), np.frombuffer(bytes(inc), np.uint8)
        outs = [np.zeros(max(sz, 1), np.uint8) for sz in (n * s_g, n * s_g // 2, n * s_g)]
        args = []
        for o, sz in zip(outs, (n * s_g, n * s_g // 2, n * s_g)):
            args += [(C.c_void_p * 1)(o.ctypes.data), (C.c_size_t * 1)(sz), 1]
        zkmi.check(zkmi.lib().zkmi_ptau_contribute_section(cv["id"], group, pg.pages, n, zkmi.ptr(f), zkmi.ptr(i), *args))
        return tuple(o[:sz].tobytes() for o, sz in zip(outs, (n * s_g, n * s_g // 2, n * s_g)))


def blake2b_partial(chunks):
    """misc.toPartialHash of a fresh Blake2b-512 hasher after one update per chunk: 216 bytes"""
    arrs = [np.frombuffer(bytes(c), np.uint8) if not isinstance(c, np.ndarray) else c for c in chunks]
    n = len(arrs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    out = np.zeros(216, np.uint8)
    zkmi.check(zkmi.lib().zkmi_blake2b512_partial(ptrs, lens, n, zkmi.ptr(out)))
    return out.tobytes()


def _lem_to_c_host(cv, point, group):
    """G.toRprCompressed of one affine LEM point (Python integers): x big-endian in normal form, an Fq2 coordinate as c1 || c0; bit 7 of the first byte when y is
    the larger of the two roots (an Fq2 y: by c1, by c0 when c1 is zero), bit 6 for the point at infinity"""
    q = next(k for k, c in CURVES.items() if c is cv)
    n8 = cv["n8q"]
    if not any(point):
        return bytes([0x40]) + bytes(group * n8 - 1)
    rinv = pow(1 << (8 * n8), -1, q)
    el = [int.from_bytes(point[i:i + n8], "little") * rinv % q for i in range(0, len(point), n8)]
    x, y = el[:group], el[group:]
    sign = y[-1] if (group == 1 or y[1]) else y[0]
    out = bytearray(b"".join(v.to_bytes(n8, "big") for v in reversed(x)))
    if sign > (q - 1) // 2:
        out[0] |= 0x80
    return bytes(out)


def _write_contributions(cv, contributions):
    """powersoftau_utils.writeContributions: the body of section 7"""
    out = [struct.pack("<I", len(contributions))]
    for c in contributions:
        k = c["key"]
        out += [c["tauG1"], c["tauG2"], c["alphaG1"], c["betaG1"], c["betaG2"]]
        out += [k[n] for n in ("tau.g1_s", "tau.g1_sx", "alpha.g1_s", "alpha.g1_sx", "beta.g1_s", "beta.g1_sx", "tau.g2_spx", "alpha.g2_spx", "beta.g2_spx")]
        out += [c["partialHash"], c["nextChallenge"], struct.pack("<I", c.get("type") or 0)]
        params = b""
        if c.get("name"):
            name = _js_name(c["name"])
            if len(name) > 255:
                raise PtauError("the name's UTF-8 encoding exceeds the 255 bytes its one-byte length field can state")
            params += bytes([1, len(name)]) + name
        if c.get("type") == 1:
            params += bytes([2, c["numIterationsExp"], 3, len(c["beaconHash"])]) + bytes(c["beaconHash"])
        out += [struct.pack("<I", len(params)), params]
    return b"".join(bytes(x) for x in out)


def _key(cv, seed, challenge):
    """keypair.createPTauKey from ChaCha(seed): (prvKeys tau / alpha / beta, the public key as the fields of a contribution)"""
    s1 = 2 * cv["n8q"]
    prv, g1_s, g1_sx = np.zeros(96, np.uint8), np.zeros(3 * s1, np.uint8), np.zeros(3 * s1, np.uint8)
    zkmi.check(zkmi.lib().zkmi_ptau_key_from_seed(cv["id"], (C.c_uint32 * 8)(*seed), zkmi.ptr(prv), zkmi.ptr(g1_s), zkmi.ptr(g1_sx)))
    prvs, key = [], {}
    for i, k in enumerate(("tau", "alpha", "beta")):
        s, sx, p = g1_s[i * s1:(i + 1) * s1].tobytes(), g1_sx[i * s1:(i + 1) * s1].tobytes(), prv[32 * i:32 * i + 32].tobytes()
        prvs.append(p)
        key[k + ".g1_s"], key[k + ".g1_sx"] = s, sx
        key[k + ".g2_spx"] = point_mul(cv, 2, _g2sp(cv, i, challenge, s, sx), p)
    return prvs, key


def _apply(old_ptau, new_ptau, log, dev, extra, seed_of, reduced):
    """One contribution: (new file bytes, response hash). seed_of() -> the ChaCha seed, called once the file has been accepted; reduced(): what a reduced file
    comes to (raises, or returns the value to hand back)"""
    src = _Source(old_ptau)
    try:
        sections, cv, power = _open(src)
        head = src.read(*sections[1][0])
        ceremony_power = struct.unpack_from("<I", head, 4 + cv["n8q"] + 4)[0]
        if power != ceremony_power:
            log("error", _REDUCED)
            return reduced()
        if 12 in sections:
            log("warn", ("WARNING: " if extra["type"] == 0 else "") + "Contributing into a file that has phase2 calculated. You will have to prepare phase2 again.")
        if power == 0:
            raise PtauError("power 0: the tauG1 section holds one point and a contribution records the second (the reference fails on the undefined point)")
        old7 = src.read(*sections[7][0])
        contributions = _read_contributions(cv, old7)
        if _write_contributions(cv, contributions) != old7:
            raise PtauError("the contributions of the old file do not serialise back to its section 7")
        body = {t: src.read(*sections[t][0]) for t in range(2, 7)}
    finally:
        src.close()
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    challenge = contributions[-1]["nextChallenge"] if contributions else first_challenge_hash(cv, power)
    (tau, alpha, beta), key = _key(cv, seed_of(), challenge)
    one = ((1 << 256) % cv["r"]).to_bytes(32, "little")
    cur = dict(extra, key=key)
    chunks, us, secs = [challenge], [], [(1, _header(cv, power))]
    for t, group, n, first, field, at in ((2, 1, (2 << power) - 1, one, "tauG1", 1), (3, 2, 1 << power, one, "tauG2", 1), (4, 1, 1 << power, alpha, "alphaG1", 0),
                                          (5, 1, 1 << power, beta, "betaG1", 0)):
        sg = 2 * group * cv["n8q"]
        lem, c, u = dev.contribute_section(cv, group, body[t], n, first, tau)
        cur[field] = lem[at * sg:(at + 1) * sg]
        step = ((1 << 20) // sg) * (sg // 2)                                   # the reference's chunk of floor(2^20 / sG) points, in C form
        cm = np.frombuffer(c, np.uint8)
        chunks += [cm[o:o + step] for o in range(0, len(c), step)]
        us.append(u)
        secs.append((t, lem))
    cur["betaG2"] = point_mul(cv, 2, body[6], beta)
    chunks.append(_lem_to_c_host(cv, cur["betaG2"], 2))
    us.append(lem_to_u_host(cv, cur["betaG2"], 2))
    secs.append((6, cur["betaG2"]))
    cur["partialHash"] = blake2b_partial(chunks)
    pub = b"".join(lem_to_u_host(cv, key[k], 1) for k in ("tau.g1_s", "tau.g1_sx", "alpha.g1_s", "alpha.g1_sx", "beta.g1_s", "beta.g1_sx"))
    pub += b"".join(lem_to_u_host(cv, key[k], 2) for k in ("tau.g2_spx", "alpha.g2_spx", "beta.g2_spx"))
    hasher = hashlib.blake2b(digest_size=64)
    for ch in chunks:
        hasher.update(ch)
    hasher.update(pub)
    response = hasher.digest()
    log("info", format_hash(response, "Contribution Response Hash imported: "))
    hasher = hashlib.blake2b(response, digest_size=64)
    for u in us:
        hasher.update(u)
    cur["nextChallenge"] = hasher.digest()
    log("info", format_hash(cur["nextChallenge"], "Next Challenge Hash: "))
    secs.append((7, _write_contributions(cv, contributions + [cur])))
    return _finish(_file(secs), new_ptau), response


def _logger(logger):
    return logger if logger else (lambda level, text: None)


def _contribute(old_ptau, name, entropy, new_ptau, logger, random64, dev):
    if not entropy:
        raise PtauError("entropy must not be empty (the reference asks for it until it is)")
    random64 = os.urandom(64) if random64 is None else bytes(random64)
    if len(random64) != 64:
        raise PtauError("random64 must be 64 bytes")

    def reduced():
        raise PtauError(_REDUCED)
    return _apply(old_ptau, new_ptau, _logger(logger), dev, dict(name=name, type=0), lambda: seed_from_entropy(random64, entropy), reduced)


def _beacon(old_ptau, name, beacon_hash_hex, num_iterations_exp, new_ptau, logger, dev):
    log = _logger(logger)
    # misc.hex2ByteArray: an "0x" in front is dropped, then every pair of hex digits it finds; the length is compared with the string as given
    pairs = re.findall(r"[0-9a-fA-F]{2}", beacon_hash_hex[2:] if beacon_hash_hex[:2] == "0x" else beacon_hash_hex)
    if not pairs:
        raise PtauError("the beacon hash holds no pair of hexadecimal digits (the reference fails on it)")
    beacon_hash = bytes.fromhex("".join(pairs))
    if 2 * len(beacon_hash) != len(beacon_hash_hex):
        log("error", "Invalid Beacon Hash. (It must be a valid hexadecimal sequence)")
        return False
    if len(beacon_hash) >= 256:
        log("error", "Maximum length of beacon hash is 255 bytes")
        return False
    num_iterations_exp = int(num_iterations_exp)
    if num_iterations_exp < 10 or num_iterations_exp > 63:
        log("error", "Invalid numIterationsExp. (Must be between 10 and 63)")
        return False
    return _apply(old_ptau, new_ptau, log, dev, dict(name=name, type=1, numIterationsExp=num_iterations_exp, beaconHash=beacon_hash),
                  lambda: seed_from_beacon(beacon_hash, num_iterations_exp), lambda: False)


def new_accumulator(curve_name, power, new_ptau=None, logger=None):
    """snarkjs.powersOfTau.newAccumulator(curve, power, fileName, logger) -> (the file's bytes, the first challenge hash)"""
    log = _logger(logger)
    names = {"bn128": "bn128", "bn254": "bn128", "altbn128": "bn128", "bls12381": "bls12381"}
    key = names.get(re.sub(r"[^0-9a-z]", "", str(curve_name).lower()))
    cv = next((c for c in CURVES.values() if c["name"] == key), None)
    if cv is None:
        raise PtauError(f"Curve not supported: {curve_name}")
    power = int(power)
    if power < 0 or power + 1 > cv["s"]:
        raise PtauError(f"power {power}: beyond what this curve's Fr.s = {cv['s']} allows a ceremony to be prepared for")
    g1, g2 = generators_lem(cv)
    n = 1 << power
    secs = [(1, _header(cv, power)), (2, g1 * (2 * n - 1)), (3, g2 * n), (4, g1 * n), (5, g1 * n), (6, g2), (7, struct.pack("<I", 0))]
    for label, count in (("tauG1", 2 * n - 1), ("tauG2", n), ("alphaTauG1", n), ("betaTauG1", n)):
        for i in range(100000, count, 100000):
            log("log", f"{label}: {i}")
    raw = _finish(_file(secs), new_ptau)
    log("debug", "Calculating First Challenge Hash")
    for i, (label, count) in enumerate((("tauG1", 2 * n - 1), ("tauG2", n), ("alphaTauG1", n), ("betaTauG1", n))):
        log("debug", f"Calculate Initial Hash: {label}")
        for b in range(count // 341000):
            log("debug", f"Initial hash: {b * 341000}")
    first = first_challenge_hash(cv, power)
    log("debug", format_hash(hashlib.blake2b(digest_size=64).digest(), "Blank Contribution Hash:"))
    log("info", format_hash(first, "First Contribution Hash:"))
    return raw, first


def contribute(old_ptau, name, entropy, new_ptau=None, logger=None, random64=None):
    """snarkjs.powersOfTau.contribute(oldPtau, newPtau, name, entropy, logger) -> (the new file's bytes, the response hash)"""
    return _contribute(old_ptau, name, entropy, new_ptau, logger, random64, Device())


def beacon(old_ptau, name, beacon_hash_hex, num_iterations_exp, new_ptau=None, logger=None):
    """snarkjs.powersOfTau.beacon(oldPtau, newPtau, name, beaconHash, numIterationsExp, logger) -> (the new file's bytes, the response hash), or False"""
    return _beacon(old_ptau, name, beacon_hash_hex, num_iterations_exp, new_ptau, logger, Device())
