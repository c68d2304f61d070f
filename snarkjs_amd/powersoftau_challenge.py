"""The challenge / response round trip of phase 1 on the device: powersOfTau.exportChallenge (src/powersoftau_export_challenge.js), powersOfTau.challengeContribute
(src/powersoftau_challenge_contribute.js with applyKeyToChallengeSection of src/mpc_applykey.js) and powersOfTau.importResponse (src/powersoftau_import.js).

    challenge, challenge_hash = export_challenge(ptau, challenge=None, logger=None)                                   # ptau: bytes or a path
    response, response_hash = challenge_contribute(curve_name, challenge, response=None, entropy=..., logger=None, random64=None)
    raw, next_challenge = import_response(old_ptau, response, new_ptau=None, name=None, import_points=True, logger=None)

Each returns the new file's bytes and also writes them when a path is given. A challenge file is the last response hash and the five point sections in U form; a
response is the challenge's hash, the five sections multiplied by the key in C form, and the public key in U form. Everything on the points of a section is ONE
library call (include/zkmi.h): zkmi_group_convert(LEM_TO_U) for the export, zkmi_ptau_challenge_section (U in, C out) for the response,
zkmi_ptau_import_section (C in, LEM and U out) for the import; an import without points takes its four recorded points through zkmi_group_convert(C_TO_LEM).
The key pair, hashToG2 and the public key are O(1) host work in the library, as in powersoftau_contribute. This module hashes, reads and writes.
importResponse does not verify the contribution, and neither does this: powersoftau_verify.verify does. logger(level, text) receives the reference's info and
error lines (its debug progress lines are not reproduced). random64 (default os.urandom(64)) is what the reference draws from getRandomValues.
The 216 bytes a contribution keeps of its response hasher hold the hasher's block buffer, whose stale bytes depend on how the data was cut into `update` calls:
response_cuts() is the reference's cut list, floor(2^24 / sG) points a call when the points are imported and floor(2^24 / scG) when they are not.
At power 0 section 2 holds a single point and the reference's import fails, after its info lines, on the second one it wants for the contribution record:
PtauError here, after the same lines. A missing section is named as the reference names it: the path in front, `undefined` for a file given as bytes.
"""
import ctypes as C
import hashlib
import os
import re
import struct

import numpy as np

from . import zkmi
from .groth16_phase2 import seed_from_entropy
from .groth16_phase2_verify import format_hash
from .groth16_setup import CURVES, SetupError, _Source, lem_to_u_host, read_sections
from .powersoftau_contribute import _key, _write_contributions, blake2b_partial
from .powersoftau_prepare import _file, _finish, _header
from .powersoftau_verify import PtauError, _read_contributions, first_challenge_hash

NO_HASH = bytes([0xFF]) * 64
_CORRUPTED = "PTau file is corrupted. Calculated new challenge hash does not match with the eclared one"


def _out(n_bytes):
    o = np.zeros(max(n_bytes, 1), np.uint8)
    return o, [(C.c_void_p * 1)(o.ctypes.data), (C.c_size_t * 1)(n_bytes), 1]


class Device:
    """the calls that need the device; tests/test_ptau_challenge_host.py puts the CPU oracle in their place"""

    def convert(self, cv, group, kind, body, n):
        """zkmi_group_convert: kind = zkmi.CONV_LEM_TO_U or zkmi.CONV_C_TO_LEM"""
        zkmi.init()
        s_g = 2 * group * cv["n8q"]
        o, arg = _out(n * s_g)
        zkmi.check(zkmi.lib().zkmi_group_convert(cv["id"], group, kind, zkmi.pages_of(body).pages, *arg, n))
        return o[:n * s_g].tobytes()

    def challenge_section(self, cv, group, body_u, n, first, inc):
        """body_u: n affine points in U form; first, inc: Montgomery Fr bytes -> the C bytes of (first * inc^i) P_i"""
        zkmi.init()
        s_g = 2 * group * cv["n8q"]
        f, i = np.frombuffer(bytes(first), np.uint8), np.frombuffer(bytes(inc), np.uint8)
        o, arg = _out(n * s_g // 2)
        zkmi.check(zkmi.lib().zkmi_ptau_challenge_section(cv["id"], group, zkmi.pages_of(body_u).pages, n, zkmi.ptr(f), zkmi.ptr(i), *arg, 0))
        return o[:n * s_g // 2].tobytes()

    def import_section(self, cv, group, body_c, n):
        """body_c: n points in C form -> (LEM, U) bytes"""
        zkmi.init()
        s_g = 2 * group * cv["n8q"]
        lem, a1 = _out(n * s_g)
        u, a2 = _out(n * s_g)
        zkmi.check(zkmi.lib().zkmi_ptau_import_section(cv["id"], group, zkmi.pages_of(body_c).pages, n, *a1, *a2))
        return lem[:n * s_g].tobytes(), u[:n * s_g].tobytes()


def _logger(logger):
    return logger if logger else (lambda level, text: None)


def _shapes(power):
    """(section, group, points) of the five point sections"""
    return ((2, 1, (2 << power) - 1), (3, 2, 1 << power), (4, 1, 1 << power), (5, 1, 1 << power), (6, 2, 1))


def response_cuts(cv, power, import_points):
    """the byte lengths of the `update` calls importResponse makes on its response hasher before it takes the partial hash: the 64-byte previous hash, then each
    section of C-form points in calls of floor(2^24 / sG) points when the points are imported (processSectionImportPoints) and of floor(2^24 / scG) points when
    they are not (processSectionNoImportPoints)"""
    cuts = [64]
    for _, group, n in _shapes(power):
        sc = group * cv["n8q"]
        per = (1 << 24) // (2 * sc if import_points else sc)
        cuts += [min(per, n - i) * sc for i in range(0, n, per)]
    return cuts


def _open_header(src):
    """readBinFile + readPTauHeader, for a file that may hold sections 1 and 7 alone -> (sections, cv, power)"""
    try:
        sections = read_sections(src, b"ptau", 1)
    except (SetupError, struct.error) as e:
        raise PtauError(str(e)) from None
    for t in (1, 7):
        if t not in sections:
            raise PtauError(f"ptau: Missing section {t}")
        if len(sections[t]) > 1:
            raise PtauError(f"ptau: Section Duplicated {t}")
    head = src.read(*sections[1][0])
    n8 = struct.unpack_from("<I", head, 0)[0] if len(head) >= 4 else -1
    if len(head) != 4 + n8 + 8:
        raise PtauError("Invalid PTau header size")
    q = int.from_bytes(head[4:4 + n8], "little")
    if q not in CURVES:
        raise PtauError(f"Curve not supported: {q}")
    cv = CURVES[q]
    return sections, cv, struct.unpack_from("<I", head, 4 + n8)[0]


def _curve(curve_name):
    names = {"bn128": "bn128", "bn254": "bn128", "altbn128": "bn128", "bls12381": "bls12381"}
    key = names.get(re.sub(r"[^0-9a-z]", "", str(curve_name).lower()))
    cv = next((c for c in CURVES.values() if c["name"] == key), None)
    if cv is None:
        raise PtauError(f"Curve not supported: {curve_name}")
    return cv


def _bytes_of(x):
    if isinstance(x, (bytes, bytearray, memoryview, np.ndarray)):
        return bytes(x)
    with open(x, "rb") as f:
        return f.read()


def _u_to_lem_host(cv, buf, group):
    """batchUtoLEM for the nine points of a public key (Python integers): the inverse of lem_to_u_host"""
    q = next(k for k, c in CURVES.items() if c is cv)
    n8 = cv["n8q"]
    el = [(int.from_bytes(buf[i:i + n8], "big") << (8 * n8)) % q for i in range(0, len(buf), n8)]
    if group == 2:
        el = [el[i ^ 1] for i in range(len(el))]
    return b"".join(v.to_bytes(n8, "little") for v in el)


_KEY_FIELDS = (("tau.g1_s", 1), ("tau.g1_sx", 1), ("alpha.g1_s", 1), ("alpha.g1_sx", 1), ("beta.g1_s", 1), ("beta.g1_sx", 1), ("tau.g2_spx", 2), ("alpha.g2_spx", 2),
               ("beta.g2_spx", 2))


def _export_challenge(ptau, challenge, logger, dev):
    log = _logger(logger)
    src = _Source(ptau)
    try:
        sections, cv, power = _open_header(src)
        contributions = _read_contributions(cv, src.read(*sections[7][0]))
        if contributions:
            last_response, declared = contributions[-1]["responseHash"], contributions[-1]["nextChallenge"]
        else:
            last_response, declared = hashlib.blake2b(digest_size=64).digest(), first_challenge_hash(cv, power)
        log("info", format_hash(last_response, "Last Response Hash: "))
        log("info", format_hash(declared, "New Challenge Hash: "))
        out = [last_response]
        for t, group, n in _shapes(power):
            if t not in sections:                                   # a file imported without points: startReadUniqueSection throws, the file's name in front
                raise PtauError(f"{os.fspath(ptau) if isinstance(ptau, (str, os.PathLike)) else 'undefined'}: Missing section {t}")
            if len(sections[t]) > 1:
                raise PtauError(f"ptau: Section Duplicated {t}")
            if sections[t][0][1] < n * 2 * group * cv["n8q"]:
                raise PtauError("Invalid section size reading")
            body = src.read(sections[t][0][0], n * 2 * group * cv["n8q"])
            out.append(dev.convert(cv, group, zkmi.CONV_LEM_TO_U, body, n))
    finally:
        src.close()
    raw = _finish(b"".join(out), challenge)                         # the reference has written the file before it compares the hashes
    calc = hashlib.blake2b(raw, digest_size=64).digest()
    if calc != declared:
        log("info", format_hash(calc, "Calc Curret Challenge Hash: "))
        log("error", _CORRUPTED)
        raise PtauError(_CORRUPTED)
    return raw, declared


def _challenge_contribute(curve_name, challenge, response, entropy, logger, random64, dev):
    log = _logger(logger)
    cv = _curve(curve_name)
    data = _bytes_of(challenge)
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    num, den = len(data) + s1 - 64 - s2, 4 * s1 + s2
    domain = num // den
    if num % den or domain < 1 or domain & (domain - 1):
        raise PtauError("Invalid file size")
    power = domain.bit_length() - 1
    if not entropy:
        raise PtauError("entropy must not be empty (the reference asks for it until it is)")
    random64 = os.urandom(64) if random64 is None else bytes(random64)
    if len(random64) != 64:
        raise PtauError("random64 must be 64 bytes")
    seed = seed_from_entropy(random64, entropy)
    log("info", format_hash(data[:64], "Claimed Previous Response Hash: "))
    challenge_hash = hashlib.blake2b(data, digest_size=64).digest()
    log("info", format_hash(challenge_hash, "Current Challenge Hash: "))
    (tau, alpha, beta), key = _key(cv, seed, challenge_hash)
    one = ((1 << 256) % cv["r"]).to_bytes(32, "little")
    out, at = [challenge_hash], 64
    for (_, group, n), first in zip(_shapes(power), (one, one, alpha, beta, beta)):
        size = n * 2 * group * cv["n8q"]
        out.append(dev.challenge_section(cv, group, data[at:at + size], n, first, tau))
        at += size
    out.append(b"".join(lem_to_u_host(cv, key[k], g) for k, g in _KEY_FIELDS))        # toPtauPubKeyRpr(..., false): normal-form U bytes
    raw = b"".join(out)
    response_hash = hashlib.blake2b(raw, digest_size=64).digest()
    log("info", format_hash(response_hash, "Contribution Response Hash: "))
    return _finish(raw, response), response_hash


def _import_response(old_ptau, response, new_ptau, name, import_points, logger, dev):
    log = _logger(logger)
    src = _Source(old_ptau)
    try:
        sections, cv, power = _open_header(src)
        contributions = _read_contributions(cv, src.read(*sections[7][0]))
    finally:
        src.close()
    data = _bytes_of(response)
    n8 = cv["n8q"]
    s1, s2 = 2 * n8, 4 * n8
    shapes = _shapes(power)
    if len(data) != 64 + sum(n * group * n8 for _, group, n in shapes) + 6 * s1 + 3 * s2:
        raise PtauError("Size of the contribution is invalid")
    last = contributions[-1]["nextChallenge"] if contributions else first_challenge_hash(cv, power)
    previous = data[:64]
    if last == NO_HASH:
        if not contributions:
            raise PtauError("the old file has no contribution whose next challenge the response could supply (the reference fails on the undefined record)")
        last = previous
        contributions[-1]["nextChallenge"] = last
    if previous != last:
        raise PtauError("Wrong contribution. This contribution is not based on the previous hash")
    cur = {}
    if name:
        cur["name"] = name
    secs, us, at = [(1, _header(cv, power))], [], 64
    for (t, group, n), field, sp in zip(shapes, ("tauG1", "tauG2", "alphaG1", "betaG1", "betaG2"), (1, 1, 0, 0, 0)):
        sc, sg = group * n8, 2 * group * n8
        body = data[at:at + n * sc]
        at += n * sc
        if import_points:
            lem, u = dev.import_section(cv, group, body, n)
            secs.append((t, lem))
            us.append(u)
            cur[field] = lem[sp * sg:(sp + 1) * sg]
        elif sp < n:
            cur[field] = dev.convert(cv, group, zkmi.CONV_C_TO_LEM, body[sp * sc:(sp + 1) * sc], 1)
    body = np.frombuffer(data, np.uint8)
    chunks, o = [], 0
    for ln in response_cuts(cv, power, import_points):
        chunks.append(body[o:o + ln])
        o += ln
    cur["partialHash"] = blake2b_partial(chunks)
    pub = data[at:]
    cur["key"], o = {}, 0
    for k, g in _KEY_FIELDS:
        cur["key"][k] = _u_to_lem_host(cv, pub[o:o + 2 * g * n8], g)
        o += 2 * g * n8
    response_hash = hashlib.blake2b(data, digest_size=64).digest()
    log("info", format_hash(response_hash, "Contribution Response Hash imported: "))
    if import_points:
        hasher = hashlib.blake2b(response_hash, digest_size=64)
        for u in us:
            hasher.update(u)
        cur["nextChallenge"] = hasher.digest()
        log("info", format_hash(cur["nextChallenge"], "Next Challenge Hash: "))
    else:
        cur["nextChallenge"] = NO_HASH
    if power == 0:                                                  # the reference has logged its lines when writeContributions meets the undefined point
        raise PtauError("power 0: the tauG1 section holds one point and a contribution records the second (the reference fails on the undefined point)")
    secs.append((7, _write_contributions(cv, contributions + [cur])))
    return _finish(_file(secs), new_ptau), cur["nextChallenge"]


def export_challenge(ptau, challenge=None, logger=None):
    """snarkjs.powersOfTau.exportChallenge(pTauFilename, challengeFilename, logger) -> (the challenge file's bytes, the challenge hash)"""
    return _export_challenge(ptau, challenge, logger, Device())


def challenge_contribute(curve_name, challenge, response=None, entropy=None, logger=None, random64=None):
    """snarkjs.powersOfTau.challengeContribute(curve, challengeFilename, responseFileName, entropy, logger) -> (the response file's bytes, the response hash)"""
    return _challenge_contribute(curve_name, challenge, response, entropy, logger, random64, Device())


def import_response(old_ptau, response, new_ptau=None, name=None, import_points=True, logger=None):
    """snarkjs.powersOfTau.importResponse(oldPtau, response, newPtau, name, importPoints, logger) -> (the new file's bytes, the next challenge hash)"""
    return _import_response(old_ptau, response, new_ptau, name, import_points, logger, Device())
