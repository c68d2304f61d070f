"""Verification of a Groth16 phase-2 key on the device: snarkjs.zKey.verifyFromInit (src/zkey_verify_frominit.js) and zKey.verifyFromR1cs
(src/zkey_verify_fromr1cs.js), the command a ceremony's coordinator runs after every contribution.

    ok = verify_from_init(init_zkey, ptau, zkey, logger=None, random64=None)        # each file: bytes or a path
    ok = verify_from_r1cs(r1cs, ptau, zkey, logger=None, random64=None)             # groth16_setup.new_zkey in memory, then verify_from_init

The checks run in the reference's order and stop at the first that fails; logger(level, text) receives the reference's lines, levels ("log" for what it
prints with console.log, else "error" / "debug" / "info") and order, spellings and double spaces included. Everything on curve points is one of three
library calls (include/zkmi.h):
    zkmi_same_ratio_batch       misc.sameRatio for the 2c + 1 checks of a key with c contributions in ONE launch, then one launch for L and H together
    zkmi_phase2_section_ratio   the two sums of the L check, scalars from ChaCha(L seed) made on the device
    zkmi_phase2_h_ratio         the two sums of the H check: Fr.fromRng draws, batchSubtract, batchApplyKey + fft, all on the device
random64 (default os.urandom(64)) is the randomness of a run: bytes 0 - 31 are the L seed and bytes 32 - 63 the H seed, each as eight big-endian words, the way
the reference builds its H seed. The reference draws its L scalars from the system generator directly; here they are the keystream of the L seed.
"""
import ctypes as C
import hashlib
import os
import struct

import numpy as np

from . import zkmi
from .groth16_phase2 import Phase2Error, hash_pub_key, hash_to_g2, key_from_seed, parse_mpc_params, read_header, seed_from_beacon
from .groth16_setup import SetupError, _Source, generators_lem, lem_to_u_host, new_zkey, read_sections

CHUNK = 1 << 20               # MAX_CHUNK_SIZE of the reference's loops: one debug line per chunk


def format_hash(b, title):
    """misc.formatHash"""
    w = struct.unpack(f">{len(b) // 4}I", b)
    s = "\n".join("\t\t" + " ".join(f"{w[4 * i + j]:08x}" for j in range(4)) for i in range(4))
    return title + "\n" + s if title else s


def _to_affine(cv, jac):
    j, out = np.frombuffer(bytes(jac), np.uint8).copy(), np.zeros(2 * cv["n8q"], np.uint8)
    zkmi.check(zkmi.lib().zkmi_to_affine(cv["id"], 1, zkmi.ptr(j), zkmi.ptr(out)))
    return out.tobytes()


def _seed(b32):
    return (C.c_uint32 * 8)(*struct.unpack(">8I", b32))


class Device:
    """the three calls that need the device; tests/test_phase2_verify_host.py puts the CPU oracle in their place"""

    def same_ratio_batch(self, cv, checks):
        """checks: (g1s, g1sx, g2s, g2sx) affine Montgomery bytes -> list of bool"""
        if not checks:
            return []
        zkmi.init()
        cols = [np.frombuffer(b"".join(c[k] for c in checks), np.uint8).copy() for k in range(4)]
        out = np.zeros(len(checks), np.int8)
        zkmi.check(zkmi.lib().zkmi_same_ratio_batch(cv["id"], *[zkmi.ptr(c) for c in cols], len(checks), zkmi.ptr(out)))
        return [bool(v == 1) for v in out]

    def section_ratio(self, cv, a, b, n, seed32):
        """(sum s_i A_i, sum s_i B_i), affine"""
        zkmi.init()
        pa, pb = zkmi.pages_of(a), zkmi.pages_of(b)
        ra, rb = np.zeros(3 * cv["n8q"], np.uint8), np.zeros(3 * cv["n8q"], np.uint8)
        zkmi.check(zkmi.lib().zkmi_phase2_section_ratio(cv["id"], pa.pages, pb.pages, n, _seed(seed32), zkmi.ptr(ra), zkmi.ptr(rb)))
        return _to_affine(cv, ra), _to_affine(cv, rb)

    def h_ratio(self, cv, tau_g1, h, power, seed32):
        """(R1, R2) of sameRatioH, affine"""
        zkmi.init()
        pt, ph = zkmi.pages_of(tau_g1), zkmi.pages_of(h)
        r1, r2 = np.zeros(3 * cv["n8q"], np.uint8), np.zeros(3 * cv["n8q"], np.uint8)
        zkmi.check(zkmi.lib().zkmi_phase2_h_ratio(cv["id"], pt.pages, ph.pages, power, _seed(seed32), zkmi.ptr(r1), zkmi.ptr(r2)))
        return _to_affine(cv, r1), _to_affine(cv, r2)


def _open_key(src, not_groth16):
    """sections, curve record, section 2 and the offsets of its fields; Phase2Error(not_groth16) for another protocol"""
    try:
        sections = read_sections(src, b"zkey", 2)
    except SetupError as e:
        raise Phase2Error(str(e)) from None
    try:
        cv, sec2, at_d1, at_d2 = read_header(src, sections)
    except Phase2Error as e:
        raise Phase2Error(not_groth16 if str(e) == "zkey file is not groth16" else str(e)) from None
    n8q = cv["n8q"]
    n8r = struct.unpack_from("<I", sec2, 4 + n8q)[0]
    o = 4 + n8q + 4 + n8r
    s1, s2 = 2 * n8q, 4 * n8q
    hdr = dict(n8q=n8q, q=sec2[4:4 + n8q], n8r=n8r, r=sec2[8 + n8q:8 + n8q + n8r])
    hdr["nVars"], hdr["nPublic"], hdr["domainSize"] = struct.unpack_from("<III", sec2, o)
    o += 12
    for k, sz in (("alpha1", s1), ("beta1", s1), ("beta2", s2), ("gamma2", s2), ("delta1", s1), ("delta2", s2)):
        hdr[k] = sec2[o:o + sz]
        o += sz
    return sections, cv, hdr


def _section(src, sections, typ):
    if typ not in sections:
        raise Phase2Error(f"zkey: Missing section {typ}")
    if len(sections[typ]) > 1:
        raise Phase2Error(f"zkey: Section Duplicated {typ}")
    return src.read(*sections[typ][0])


def _verify(init_zkey, ptau, zkey, logger, random64, dev):
    log = logger if logger else (lambda level, text: None)
    random64 = os.urandom(64) if random64 is None else bytes(random64)
    if len(random64) != 64:
        raise Phase2Error("random64 must be 64 bytes")
    src = _Source(zkey)
    src_init = src_ptau = None
    try:
        sections, cv, key = _open_key(src, "zkey file is not groth16")
        s1 = 2 * cv["n8q"]
        cs_hash, contributions = parse_mpc_params(_section(src, sections, 10), cv)
        g1_gen, g2_gen = generators_lem(cv)

        # ---- the contributions: everything but the pairings is host work, so the 2c + 1 same-ratio checks of the key go to the device together. A check
        # that an earlier failure makes moot is left out of the launch.
        steps, checks = [], []                    # steps: (message, verdict | index into checks), in the reference's order
        acc = hashlib.blake2b(digest_size=64)
        acc.update(cs_hash)
        cur_delta = g1_gen
        for i, c in enumerate(contributions):
            ours = acc.copy()
            ours.update(lem_to_u_host(cv, c["g1_s"], 1))
            ours.update(lem_to_u_host(cv, c["g1_sx"], 1))
            steps.append((f"INVALID({i}): Inconsistent transcript ", ours.digest() == c["transcript"]))
            if not steps[-1][1]:
                break
            g2_sp = hash_to_g2(cv, c["transcript"])
            steps.append((f"INVALID({i}): public key G1 and G2 do not have the same ration ", len(checks)))
            checks.append((c["g1_s"], c["g1_sx"], g2_sp, c["g2_spx"]))
            steps.append((f"INVALID({i}): deltaAfter does not fillow the public key ", len(checks)))
            checks.append((cur_delta, c["deltaAfter"], g2_sp, c["g2_spx"]))
            if c["type"] == 1:
                _prv, g1_s, g1_sx = key_from_seed(cv, seed_from_beacon(c["beaconHash"], c["numIterationsExp"]))
                steps.append((f"INVALID({i}): Key of the beacon does not match. g1_s ", g1_s == c["g1_s"]))
                steps.append((f"INVALID({i}): Key of the beacon does not match. g1_sx ", g1_sx == c["g1_sx"]))
                if not (steps[-2][1] and steps[-1][1]):
                    break
            hash_pub_key(acc, cv, c)
            h = hashlib.blake2b(digest_size=64)
            hash_pub_key(h, cv, c)
            c["contributionHash"] = h.digest()
            cur_delta = c["deltaAfter"]
        host_ok = all(v is not False for _m, v in steps)
        at_delta2 = None
        if host_ok:                               # delta2 needs nothing of the init key: it rides along
            at_delta2 = len(checks)
            checks.append((g1_gen, cur_delta, g2_gen, key["delta2"]))
        verdicts = dev.same_ratio_batch(cv, checks)
        for msg, v in steps:
            if not (verdicts[v] if type(v) is int else v):
                log("log", msg)
                return False

        # ---- against the init key
        src_init = _Source(init_zkey)
        sections_init, _cv_init, init = _open_key(src_init, "zkeyinit file is not groth16")
        if any(init[k] != key[k] for k in ("q", "r", "n8q", "n8r")):
            log("error", "INVALID:  Different curves")
            return False
        if any(init[k] != key[k] for k in ("nVars", "nPublic", "domainSize")):
            log("error", "INVALID:  Different circuit parameters")
            return False
        for k, name in (("alpha1", "alpha1"), ("beta1", "beta1"), ("beta2", "beta2"), ("gamma2", "gamma2")):
            if key[k] != init[k]:
                log("error", f"INVALID:  Invalid {name}")
                return False
        if key["delta1"] != cur_delta:
            log("error", "INVALID:  Invalid delta1")
            return False
        if not verdicts[at_delta2]:
            log("error", "INVALID:  Invalid delta2")
            return False
        cs_hash_init, _ = parse_mpc_params(_section(src_init, sections_init, 10), cv)
        if cs_hash != cs_hash_init:
            log("error", "INVALID:  Circuit does not match")
            return False
        n_l, domain = key["nVars"] - key["nPublic"] - 1, key["domainSize"]
        if sections[8][0][1] != s1 * n_l:
            log("error", "INVALID:  Invalid L section size")
            return False
        if sections[9][0][1] != s1 * domain:
            log("error", "INVALID:  Invalid H section size")
            return False
        for typ, msg in ((3, "INVALID:  IC section is not identical"), (4, "Coeffs section is not identical"), (5, "A section is not identical"),
                         (6, "B1 section is not identical"), (7, "B2 section is not identical")):
            if _section(src, sections, typ) != _section(src_init, sections_init, typ):
                log("error", msg)
                return False

        # ---- L and H. One lane's pairing is the time of a whole same-ratio launch, so the two checks share one: the sums of H are computed before the verdict on L
        # is known. The lines, and whatever the H side raises, still come in the reference's order: nothing of H is reported unless L has passed.
        l_init = _section(src_init, sections_init, 8)
        n_points = len(l_init) // s1
        pending = []
        if n_points:
            r1, r2 = dev.section_ratio(cv, l_init, _section(src, sections, 8), n_points, random64[:32])
            pending.append((r1, r2, key["delta2"], init["delta2"]))
        h_error = None
        try:
            power = domain.bit_length() - 1
            if domain != 1 << power:
                raise Phase2Error("domainSize is not a power of two")
            src_ptau = _Source(ptau)
            try:
                sp = read_sections(src_ptau, b"ptau", 1)
            except SetupError as e:
                raise Phase2Error(str(e)) from None
            if 2 not in sp or sp[2][0][1] < (2 * domain - 1) * s1:
                raise Phase2Error("the ptau's tauG1 section holds fewer than 2 domainSize - 1 points")
            r1, r2 = dev.h_ratio(cv, src_ptau.read(sp[2][0][0], (2 * domain - 1) * s1), _section(src, sections, 9), power, random64[32:])
            pending.append((r1, r2, key["delta2"], init["delta2"]))
        except Exception as e:                    # reported only once L has passed
            h_error = e
        verdicts = dev.same_ratio_batch(cv, pending)
        for i in range(0, n_points, CHUNK):
            log("debug", f"Same ratio check L section:  {i}/{n_points}")
        if n_points and not verdicts[0]:
            log("error", "L section does not match")
            return False
        if h_error is not None:
            raise h_error
        for name in ("tau", "lagrange"):
            for i in range(0, domain, CHUNK):
                log("debug", f"H Verification({name}):  {i}/{domain}")
        if not verdicts[-1]:
            log("error", "H section does not match")
            return False

        log("info", format_hash(cs_hash, "Circuit Hash: "))
        for i in range(len(contributions) - 1, -1, -1):
            c = contributions[i]
            log("info", "-------------------------")
            log("info", format_hash(c["contributionHash"], f"contribution #{i + 1} {c.get('name') or ''}:"))
            if c["type"] == 1:
                log("info", f"Beacon generator: {bytes(c['beaconHash']).hex()}")
                log("info", f"Beacon iterations Exp: {c['numIterationsExp']}")
        log("info", "-------------------------")
        log("info", "ZKey Ok!")
        return True
    finally:
        for s in (src, src_init, src_ptau):
            if s is not None:
                s.close()


def verify_from_init(init_zkey, ptau, zkey, logger=None, random64=None):
    """snarkjs.zKey.verifyFromInit(initFileName, pTauFileName, zkeyFileName, logger) -> bool"""
    return _verify(init_zkey, ptau, zkey, logger, random64, Device())


def verify_from_r1cs(r1cs, ptau, zkey, logger=None, random64=None):
    """snarkjs.zKey.verifyFromR1cs(r1csFileName, pTauFileName, zkeyFileName, logger) -> bool: the init key is built in memory by the device newZKey"""
    init, _cs_hash = new_zkey(r1cs, ptau)
    return _verify(init, ptau, zkey, logger, random64, Device())
