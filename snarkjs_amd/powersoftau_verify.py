"""powersOfTau.verify on the device (src/powersoftau_verify.js): the check a ceremony's coordinator runs on every .ptau it receives.

    ok = verify(ptau, logger=None, random32=None)                                    # ptau: bytes or a path

The checks run in the reference's order and stop at the first that fails; logger(level, text) receives the reference's info, warn and error lines in its order,
spellings included (its debug progress lines are not reproduced). Everything on curve points is one of two library calls (include/zkmi.h):
    zkmi_ptau_section_check     once per section 2 - 5, from one upload: the section in U form (the bytes the reference hashes), the two sums of processSection
                                and one verdict per power of verifyLagrangeEvaluations (None when the file has no Lagrange sections)
    zkmi_same_ratio_batch       misc.sameRatio for all 8 c + 4 checks of a file with c contributions in ONE launch (verifyContribution makes eight)
The host work of all contributions (beacon keys, hashToG2, the hashes) is done first. random32 (default os.urandom(32)) is the randomness of a run: seed j is
the first 32 bytes of blake2b(random32 || byte j) read as eight big-endian words, j = 2 .. 5 the pair seeds of the sections and j = 12 .. 15 their ladder seeds
(the reference draws both from the system generator). blake2b_resume is misc.fromPartialHash(partial).update(data).digest(): Python's hashlib cannot restore
a state, so this one hash is the library's; it needs no device. The first challenge hash of a ceremony is about 2^(ceremonyPower + 8) bytes of Blake2b on one
host core (96 GB for a file cut from a 2^28 ceremony); it is computed only when contribution 1 is reached.
"""
import ctypes as C
import hashlib
import os
import struct

import numpy as np

from . import zkmi
from .groth16_phase2 import hash_to_g2, point_mul, seed_from_beacon
from .groth16_phase2_verify import Device as _RatioDevice, format_hash
from .groth16_setup import CURVES, SetupError, _Source, generators_lem, lem_to_u_host, read_sections


class PtauError(ValueError):
    """powersOfTau.verify refused the file (the reference throws)"""


def _seed(b32):
    return (C.c_uint32 * 8)(*struct.unpack(">8I", bytes(b32)))


def blake2b_resume(partial216, data):
    """Blake2b-512 continued from the 216-byte partial state a contribution keeps of its response hash"""
    partial216, data = bytes(partial216), bytes(data)
    if len(partial216) != 216:
        raise ValueError("a partial hash is 216 bytes")
    p, d, out = np.frombuffer(partial216, np.uint8), np.frombuffer(data, np.uint8), np.zeros(64, np.uint8)
    zkmi.check(zkmi.lib().zkmi_blake2b512_resume(zkmi.ptr(p), zkmi.ptr(d) if len(data) else None, len(data), zkmi.ptr(out)))
    return out.tobytes()


def to_affine(cv, group, jac):
    j, out = np.frombuffer(bytes(jac), np.uint8).copy(), np.zeros(2 * group * cv["n8q"], np.uint8)
    zkmi.check(zkmi.lib().zkmi_to_affine(cv["id"], group, zkmi.ptr(j), zkmi.ptr(out)))
    return out.tobytes()


class Device(_RatioDevice):
    """the two calls that need the device (same_ratio_batch is groth16_phase2_verify.Device's); tests/test_ptau_verify_host.py puts the CPU oracle in their place"""

    def section_check(self, cv, group, tau, n_tau, lagrange, top, zero_last, pair_seed32, ladder_seed32):
        """tau, lagrange: bytes or a list of pages (lagrange None: absent) -> (U bytes, r1 affine, r2 affine, [bool] * (top + 1) | None)"""
        zkmi.init()
        s_g, jac = 2 * group * cv["n8q"], 3 * group * cv["n8q"]
        pt = zkmi.pages_of(tau)
        pl = zkmi.pages_of(lagrange) if lagrange is not None else None
        u = np.zeros(max(n_tau * s_g, 1), np.uint8)
        r1, r2, ladder = np.zeros(jac, np.uint8), np.zeros(jac, np.uint8), np.zeros(top + 1, np.int8)
        u_ptr, u_len = (C.c_void_p * 1)(u.ctypes.data), (C.c_size_t * 1)(n_tau * s_g)
        zkmi.check(zkmi.lib().zkmi_ptau_section_check(cv["id"], group, pt.pages, n_tau, C.byref(pl.pages) if pl else None, top, 1 if zero_last else 0, _seed(pair_seed32),
                                                      _seed(ladder_seed32), u_ptr, u_len, 1, zkmi.ptr(r1), zkmi.ptr(r2), zkmi.ptr(ladder)))
        return u[:n_tau * s_g].tobytes(), to_affine(cv, group, r1), to_affine(cv, group, r2), ([bool(v == 1) for v in ladder] if pl else None)


# ---- the file ---------------------------------------------------------------------------------------------------------------------------------------------
def _read_contributions(cv, body):
    """powersoftau_utils.readContributions on the bytes of section 7"""
    s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
    n, o, out = struct.unpack_from("<I", body, 0)[0], 4, []
    for i in range(n):
        c = dict(id=i + 1)
        for k, sz in (("tauG1", s1), ("tauG2", s2), ("alphaG1", s1), ("betaG1", s1), ("betaG2", s2)):
            c[k] = body[o:o + sz]
            o += sz
        key = {}
        for k in ("tau.g1_s", "tau.g1_sx", "alpha.g1_s", "alpha.g1_sx", "beta.g1_s", "beta.g1_sx"):
            key[k] = body[o:o + s1]
            o += s1
        for k in ("tau.g2_spx", "alpha.g2_spx", "beta.g2_spx"):
            key[k] = body[o:o + s2]
            o += s2
        c["key"] = key
        c["partialHash"], c["nextChallenge"] = body[o:o + 216], body[o + 216:o + 280]
        if o + 288 > len(body):
            raise PtauError("Invalid contribution section size")
        c["type"], plen = struct.unpack_from("<II", body, o + 280)
        o += 288
        end, last = o + plen, 0
        while o < end:
            typ = body[o]
            if typ <= last:
                raise PtauError("Parameters in the contribution must be sorted")
            last = typ
            if typ == 1:
                c["name"] = body[o + 2:o + 2 + body[o + 1]].decode("utf-8", "replace")
                o += 2 + body[o + 1]
            elif typ == 2:
                c["numIterationsExp"] = body[o + 1]
                o += 2
            elif typ == 3:
                c["beaconHash"] = body[o + 2:o + 2 + body[o + 1]]
                o += 2 + body[o + 1]
            else:
                raise PtauError("Parameter not recognized")
        if o != end:
            raise PtauError("Parameters do not match")
        pub = b"".join(lem_to_u_host(cv, key[k], 1) for k in ("tau.g1_s", "tau.g1_sx", "alpha.g1_s", "alpha.g1_sx", "beta.g1_s", "beta.g1_sx"))
        pub += b"".join(lem_to_u_host(cv, key[k], 2) for k in ("tau.g2_spx", "alpha.g2_spx", "beta.g2_spx"))
        c["responseHash"] = blake2b_resume(c["partialHash"], pub)
        out.append(c)
    if o != len(body):
        raise PtauError("Invalid contribution section size")
    return out


def first_challenge_hash(cv, ceremony_power):
    """powersoftau_utils.calculateFirstChallengeHash: the generators repeated, fed from one buffer"""
    g1, g2 = generators_lem(cv)
    u1, u2 = lem_to_u_host(cv, g1, 1), lem_to_u_host(cv, g2, 2)
    h = hashlib.blake2b(hashlib.blake2b(digest_size=64).digest(), digest_size=64)

    def block(u, n):
        big = u * min(n, 1 << 14)
        for _ in range(n // (1 << 14)):
            h.update(big)
        h.update(u * (n % (1 << 14)))
    n = 1 << ceremony_power
    block(u1, 2 * n - 1)
    block(u2, n)
    block(u1, n)
    block(u1, n)
    h.update(u2)
    return h.digest()


def _g2sp(cv, personalization, challenge, g1_s, g1_sx):
    """keypair.getG2sp"""
    h = hashlib.blake2b(bytes([personalization]) + challenge + lem_to_u_host(cv, g1_s, 1) + lem_to_u_host(cv, g1_sx, 1), digest_size=64).digest()
    return hash_to_g2(cv, h)


def _beacon_failure(cv, cur, prev):
    """the first of the nine comparisons of a beacon contribution's key that fails, as the reference names it (None: all hold)"""
    s1 = 2 * cv["n8q"]
    if "beaconHash" not in cur or "numIterationsExp" not in cur:
        raise PtauError(f"beacon contribution #{cur['id']} has no beaconHash or numIterationsExp parameter")
    prv, g1_s, g1_sx = np.zeros(96, np.uint8), np.zeros(3 * s1, np.uint8), np.zeros(3 * s1, np.uint8)
    seed = (C.c_uint32 * 8)(*seed_from_beacon(cur["beaconHash"], cur["numIterationsExp"]))
    zkmi.check(zkmi.lib().zkmi_ptau_key_from_seed(cv["id"], seed, zkmi.ptr(prv), zkmi.ptr(g1_s), zkmi.ptr(g1_sx)))
    for i, k in enumerate(("tau", "alpha", "beta")):
        s, sx = g1_s[i * s1:(i + 1) * s1].tobytes(), g1_sx[i * s1:(i + 1) * s1].tobytes()
        if cur["key"][k + ".g1_s"] != s:
            return f"{k}G1_s"
        if cur["key"][k + ".g1_sx"] != sx:
            return f"{k}G1_sx"
        if cur["key"][k + ".g2_spx"] != point_mul(cv, 2, _g2sp(cv, i, prev["nextChallenge"], s, sx), prv[32 * i:32 * i + 32].tobytes()):
            return f"{k}G2_spx"
    return None


_RATIO_LINES = ("INVALID key (tau) in challenge #{id}", "INVALID key (alpha) in challenge #{id}", "INVALID key (beta) in challenge #{id}",
                "INVALID tau*G1. challenge #{id} It does not follow the previous contribution", "INVALID tau*G2. challenge #{id} It does not follow the previous contribution",
                "INVALID alpha*G1. challenge #{id} It does not follow the previous contribution", "INVALID beta*G1. challenge #{id} It does not follow the previous contribution",
                "INVALID beta*G2. challenge #{id}It does not follow the previous contribution")


def _contribution_checks(cv, cur, prev):
    """the eight sameRatio calls of verifyContribution, in its order"""
    k = cur["key"]
    sp = [_g2sp(cv, i, prev["nextChallenge"], k[n + ".g1_s"], k[n + ".g1_sx"]) for i, n in enumerate(("tau", "alpha", "beta"))]
    return [(k["tau.g1_s"], k["tau.g1_sx"], sp[0], k["tau.g2_spx"]), (k["alpha.g1_s"], k["alpha.g1_sx"], sp[1], k["alpha.g2_spx"]),
            (k["beta.g1_s"], k["beta.g1_sx"], sp[2], k["beta.g2_spx"]), (prev["tauG1"], cur["tauG1"], sp[0], k["tau.g2_spx"]),
            (k["tau.g1_s"], k["tau.g1_sx"], prev["tauG2"], cur["tauG2"]), (prev["alphaG1"], cur["alphaG1"], sp[1], k["alpha.g2_spx"]),
            (prev["betaG1"], cur["betaG1"], sp[2], k["beta.g2_spx"]), (k["beta.g1_s"], k["beta.g1_sx"], prev["betaG2"], cur["betaG2"])]


def _verify(ptau, logger, random32, dev):
    log = logger if logger else (lambda level, text: None)
    random32 = os.urandom(32) if random32 is None else bytes(random32)
    if len(random32) != 32:
        raise PtauError("random32 must be 32 bytes")
    seed_of = lambda j: hashlib.blake2b(random32 + bytes([j]), digest_size=64).digest()[:32]
    src = _Source(ptau)
    try:
        try:
            sections = read_sections(src, b"ptau", 1)
        except SetupError as e:
            raise PtauError(str(e)) from None
        if 1 not in sections:
            raise PtauError("File has no  header")
        if len(sections[1]) > 1:
            raise PtauError("File has more than one header")
        head = src.read(*sections[1][0])
        n8 = struct.unpack_from("<I", head, 0)[0]
        if len(head) != 4 + n8 + 8:
            raise PtauError("Invalid PTau header size")
        q = int.from_bytes(head[4:4 + n8], "little")
        if q not in CURVES:
            raise PtauError(f"Curve not supported: {q}")
        cv = CURVES[q]
        if cv["n8q"] != n8:
            raise PtauError("Invalid size")
        power, ceremony_power = struct.unpack_from("<II", head, 4 + n8)
        if 7 not in sections:
            raise PtauError("File has no  contributions")
        contrs = _read_contributions(cv, src.read(*sections[7][0]))
        if power + 1 > cv["s"]:
            raise PtauError(f"power {power}: the tauG1 ladder needs a transform of 2^{power + 1} elements, beyond the limit of 2^{cv['s']} (Fr.s) of this curve")
        if not contrs:
            log("error", "This file has no contribution! It cannot be used in production")
            return False
        s1, s2 = 2 * cv["n8q"], 4 * cv["n8q"]
        g1, g2 = generators_lem(cv)
        # ---- the host work of all contributions, last to first as they are reported
        initial = dict(tauG1=g1, tauG2=g2, alphaG1=g1, betaG1=g1, betaG2=g2)
        checks, beacon_bad = [], {}
        for i in range(len(contrs) - 1, -1, -1):
            cur = contrs[i]
            if i == 0:
                initial["nextChallenge"] = first_challenge_hash(cv, ceremony_power)
            prev = contrs[i - 1] if i else initial
            if cur["type"] == 1:
                bad = _beacon_failure(cv, cur, prev)
                if bad:
                    beacon_bad[i] = bad
                    break                         # nothing after this failure is reported
            checks += _contribution_checks(cv, cur, prev)
        # ---- the four sections: one call each
        last = contrs[-1]
        lagrange_there = all(t in sections for t in (12, 13, 14, 15))
        hasher = hashlib.blake2b(last["responseHash"], digest_size=64)
        sec, sec_throw = {}, {}                   # what the reference throws at a section is raised where it would reach that section, after the lines before it
        for t, group, n_tau, top in ((2, 1, 2 * (1 << power) - 1, power + 1), (3, 2, 1 << power, power), (4, 1, 1 << power, power), (5, 1, 1 << power, power)):
            sg = 2 * group * cv["n8q"]
            if t not in sections:
                sec_throw[t] = f"ptau: Missing section {t}"
            elif len(sections[t]) > 1:
                sec_throw[t] = f"ptau: Section Duplicated {t}"
            elif sections[t][0][1] != n_tau * sg:
                sec_throw[t] = "Invalid section size reading"
            if t in sec_throw:
                break                             # the reference goes no further: no device work for this section or those after it
            tau = src.read(*sections[t][0])
            lag, lag_throw = None, None
            if lagrange_there:
                if len(sections[t + 10]) > 1:
                    lag_throw = f"ptau: Section Duplicated {t + 10}"
                elif sections[t + 10][0][1] < ((2 << top) - 1) * sg:
                    lag_throw = "Invalid section size reading"
                else:
                    lag = src.read(sections[t + 10][0][0], ((2 << top) - 1) * sg)
            u, r1, r2, ladder = dev.section_check(cv, group, tau, n_tau, lag, top, t == 2, seed_of(t), seed_of(t + 10))
            hasher.update(u)
            sec[t] = dict(first=tau[:sg], second=tau[sg:2 * sg], r1=r1, r2=r2, ladder=ladder, lag_throw=lag_throw)
        beta_g2 = src.read(sections[6][0][0], s2) if 6 in sections and len(sections[6]) == 1 else None
    finally:
        src.close()
    at_sec = {}
    for t, quad in ((2, lambda x: (x["r1"], x["r2"], g2, last["tauG2"])), (3, lambda x: (g1, last["tauG1"], x["r1"], x["r2"])),
                    (4, lambda x: (x["r1"], x["r2"], g2, last["tauG2"])), (5, lambda x: (x["r1"], x["r2"], g2, last["tauG2"]))):
        if t in sec:
            at_sec[t] = len(checks)
            checks.append(quad(sec[t]))
    verdicts = dev.same_ratio_batch(cv, checks)

    # ---- the lines, in the reference's order
    def contribution_ok(i):
        cur = contrs[i]
        if i in beacon_bad:
            log("error", f"BEACON key ({beacon_bad[i]}) is not generated correctly in challenge #{cur['id']}  {cur.get('name') or ''}")
            return False
        at = 8 * (len(contrs) - 1 - i)
        for j, line in enumerate(_RATIO_LINES):
            if not verdicts[at + j]:
                log("error", line.format(id=cur["id"]))
                return False
        log("info", "Powers Of tau file OK!")
        return True

    def print_contribution(i):
        cur, prev = contrs[i], (contrs[i - 1] if i else initial)
        log("info", "-----------------------------------------------------")
        log("info", f"Contribution #{cur['id']}: {cur.get('name') or ''}")
        log("info", format_hash(cur["nextChallenge"], "Next Challenge: "))
        log("info", format_hash(cur["responseHash"], "Response Hash:"))
        log("info", format_hash(prev["nextChallenge"], "Response Hash:"))
        if cur["type"] == 1:
            log("info", f"Beacon generator: {bytes(cur['beaconHash']).hex()}")
            log("info", f"Beacon iterations Exp: {cur['numIterationsExp']}")

    if not contribution_ok(len(contrs) - 1):
        return False
    for t, name, firsts in ((2, "tauG1", ((g1, "First element of tau*G1 section must be the generator"),
                                          (last["tauG1"], "Second element of tau*G1 section does not match the one in the contribution section"))),
                            (3, "tauG2", ((g2, "First element of tau*G2 section must be the generator"),
                                          (last["tauG2"], "Second element of tau*G2 section does not match the one in the contribution section"))),
                            (4, "alphaTauG1", ((last["alphaG1"], "First element of alpha*tau*G1 section (alpha*G1) does not match the one in the contribution section"),)),
                            (5, "betaTauG1", ((last["betaG1"], "First element of beta*tau*G1 section (beta*G1) does not match the one in the contribution section"),))):
        if t in sec_throw:
            raise PtauError(sec_throw[t])
        if not verdicts[at_sec[t]]:
            log("error", f"{name} section. Powers do not match")
            return False
        for (want, line), got in zip(firsts, (sec[t]["first"], sec[t]["second"])):
            if got != want:
                log("error", line)
                return False
    if beta_g2 is None:
        log("error", "File has no BetaG2 section")
        raise PtauError("File has no BetaG2 section" if 6 not in sections else "File has more than one GetaG2 section")
    hasher.update(lem_to_u_host(cv, beta_g2, 2))
    if beta_g2 != last["betaG2"]:
        log("error", "betaG2 element in betaG2 section does not match the one in the contribution section")
        return False
    next_hash = hasher.digest()
    if power == ceremony_power and next_hash != last["nextChallenge"]:
        log("error", "Hash of the values does not match the next challenge of the last contributor in the contributions section")
        return False
    log("info", format_hash(next_hash, "Next challenge hash: "))
    print_contribution(len(contrs) - 1)
    for i in range(len(contrs) - 2, -1, -1):
        if not contribution_ok(i):
            return False
        print_contribution(i)
    log("info", "-----------------------------------------------------")
    if not lagrange_there:
        log("warn", "this file does not contain phase2 precalculated values. Please run: \n" +
            "   snarkjs \"powersoftau preparephase2\" to prepare this file to be used in the phase2 ceremony.")
    else:
        for t in (2, 3, 4, 5):
            if sec[t]["lag_throw"]:
                raise PtauError(sec[t]["lag_throw"])
            if not all(sec[t]["ladder"]):
                log("error", "Phase2 caclutation does not match with powers of tau")
                return False
    log("info", "Powers of Tau Ok!")
    return True


def verify(ptau, logger=None, random32=None):
    """snarkjs.powersOfTau.verify(ptau, logger) -> bool"""
    return _verify(ptau, logger, random32, Device())
