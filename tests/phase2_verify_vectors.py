"""Shared by tests/test_phase2_verify_host.py and tests/test_gpu_phase2_verify.py: the golden phase-2 chain, the tamper table of zKey.verifyFromInit built in
memory from it, and the three device calls of snarkjs_amd/groth16_phase2_verify.py restated on the CPU oracle (its MSM, its transform and the Python pairing
of oracle/groth16_verify_oracle.py, with the sequential generator struct of the library for the scalars)."""
import ctypes as C
import json
import os
import struct

import numpy as np

import groth16_verify_oracle as GO
import oracle_lib as orc
from snarkjs_amd import groth16_phase2 as p2
from snarkjs_amd import groth16_setup as gs
from snarkjs_amd import zkmi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX = json.load(open(os.path.join(GOLDEN, "phase2_golden.json")))
STEPS = sorted(INDEX["files"])
CURVES = ("bn128", "bls12381")
RANDOM64 = bytes(range(64))


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def curve_record(curve):
    return next(c for c in gs.CURVES.values() if c["name"] == curve)


def curve_of_file(name):
    return "bn128" if "bn128" in name else "bls12381"


def init_of(name):
    """the setup key a golden phase-2 key descends from"""
    while name in INDEX["files"]:
        name = INDEX["files"][name]["from"]
    return name


def chain_hashes(name):
    """contribution hashes of the key, first contribution first"""
    out = []
    while name in INDEX["files"]:
        out.append(INDEX["files"][name]["contributionHash"])
        name = INDEX["files"][name]["from"]
    return out[::-1]


def seed_words(b32):
    return (C.c_uint32 * 8)(*struct.unpack(">8I", b32))


# ---- host references of the generator ---------------------------------------------------------------------------------------------------------------------
def host_words(seed, first_word, n):
    """keystream words from the sequential generator struct (phase2::ChaCha)"""
    out = np.zeros(max(n, 1), np.uint32)
    assert zkmi.lib().zkmi_chacha_struct_words_host((C.c_uint32 * 8)(*seed), first_word, zkmi.ptr(out), n) == 0
    return out[:n]


def host_fr(curve_id, seed, n, compact=False):
    """(n x 32 bytes, words consumed) of sequential Fr.fromRng draws; compact: by the kernels' rule on the host instead"""
    out, w = np.zeros(max(32 * n, 1), np.uint8), C.c_uint64(0)
    fn = zkmi.lib().zkmi_chacha_fr_compact_host if compact else zkmi.lib().zkmi_chacha_fr_host
    assert fn(curve_id, (C.c_uint32 * 8)(*seed), zkmi.ptr(out), n, C.byref(w)) == 0
    return out[:32 * n], w.value


# ---- the CPU oracle in place of the device ------------------------------------------------------------------------------------------------------------
def _q(cv):
    return next(k for k, c in gs.CURVES.items() if c is cv)


def _ints(cv, buf):
    q, n8 = _q(cv), cv["n8q"]
    rinv = pow(1 << (8 * n8), -1, q)
    return [int.from_bytes(buf[i:i + n8], "little") * rinv % q for i in range(0, len(buf), n8)]


def g1_of(cv, buf):
    return None if not any(buf) else tuple(_ints(cv, buf))


def g2_of(cv, buf):
    if not any(buf):
        return None
    v = _ints(cv, buf)
    return ((v[0], v[1]), (v[2], v[3]))


def oracle_same_ratio(cv, g1s, g1sx, g2s, g2sx):
    """misc.sameRatio on the Python pairing"""
    E = GO.CURVES[cv["name"]]
    a, ax, b, bx = g1_of(cv, g1s), g1_of(cv, g1sx), g2_of(cv, g2s), g2_of(cv, g2sx)
    if a is None or ax is None or b is None or bx is None:
        return False
    return bool(E.pairing_product_is_one([(a, bx), (E.g1_neg(ax), b)]))


class OracleDevice:
    """groth16_phase2_verify.Device on the CPU. Verdicts are memoised over the module: the keys of a chain share their contributions' checks."""
    memo = {}

    def __init__(self):
        self.ratios = {}                          # "L" / "H" -> (R1, R2) of the last call

    def same_ratio_batch(self, cv, checks):
        out = []
        for c in checks:
            k = (cv["name"],) + tuple(bytes(x) for x in c)
            if k not in self.memo:
                self.memo[k] = oracle_same_ratio(cv, *c)
            out.append(self.memo[k])
        return out

    def section_ratio(self, cv, a, b, n, seed32):
        c = cv["id"]
        s = host_words(struct.unpack(">8I", seed32), 0, n).view(np.uint8)
        r = tuple(orc.to_affine(c, 1, orc.msm(c, 1, np.frombuffer(x, np.uint8), s, n, 4)).tobytes() for x in (a, b))
        self.ratios["L"] = r
        return r

    def h_ratio(self, cv, tau_g1, h, power, seed32):
        c, r, dom, s1 = cv["id"], cv["r"], 1 << power, 2 * cv["n8q"]
        raw = np.zeros(32 * dom, np.uint8)
        raw[:32 * (dom - 1)] = host_fr(c, struct.unpack(">8I", seed32), dom - 1)[0]
        e = orc.from_mont(c, raw)
        # sum e_i (tau[dom + i] - tau[i]) = sum e_i tau[dom + i] + sum (r - e_i) tau[i] over i < dom - 1: one MSM, no subtraction of points
        neg = b"".join(((r - int.from_bytes(e[32 * i:32 * i + 32], "little")) % r).to_bytes(32, "little") for i in range(dom - 1))
        tau = np.frombuffer(tau_g1, np.uint8)
        bases = np.concatenate([tau[dom * s1:(2 * dom - 1) * s1], tau[:(dom - 1) * s1]])
        scalars = np.concatenate([e[:32 * (dom - 1)], np.frombuffer(neg, np.uint8)])
        r1 = orc.to_affine(c, 1, orc.msm(c, 1, bases, scalars, 2 * (dom - 1))).tobytes()
        two = int.from_bytes(orc.fr_e(c, 2).tobytes(), "little")
        first = np.frombuffer(((r - two) % r).to_bytes(32, "little"), np.uint8)
        t = orc.from_mont(c, orc.ntt(c, orc.apply_key(c, raw, first, orc.fr_w(c, power + 1))))
        r2 = orc.to_affine(c, 1, orc.msm(c, 1, np.frombuffer(h, np.uint8), t, dom)).tobytes()
        self.ratios["H"] = (r1, r2)
        return r1, r2


# ---- keys taken apart and put together again ----------------------------------------------------------------------------------------------------------
def split(raw):
    """[(type, body)] in file order"""
    n, out, off = struct.unpack_from("<I", raw, 8)[0], [], 12
    for _ in range(n):
        typ, ln = struct.unpack_from("<IQ", raw, off)
        out.append((typ, raw[off + 12:off + 12 + ln]))
        off += 12 + ln
    return out


def join(raw, secs):
    out = [raw[:8], struct.pack("<I", len(secs))]
    for typ, body in secs:
        out += [struct.pack("<IQ", typ, len(body)), body]
    return b"".join(out)


def with_section(raw, typ, fn):
    return join(raw, [(t, fn(b) if t == typ else b) for t, b in split(raw)])


def section(raw, typ):
    return next(b for t, b in split(raw) if t == typ)


def header_fields(cv, sec2):
    """name -> (offset, size) of the six points of section 2"""
    n8q = cv["n8q"]
    o = 4 + n8q + 4 + struct.unpack_from("<I", sec2, 4 + n8q)[0] + 12
    out = {}
    for k, sz in (("alpha1", 2 * n8q), ("beta1", 2 * n8q), ("beta2", 4 * n8q), ("gamma2", 4 * n8q), ("delta1", 2 * n8q), ("delta2", 4 * n8q)):
        out[k] = (o, sz)
        o += sz
    return out


def _header(cv, raw, edits):
    """section 2 with field <- bytes for every (field, source field | bytes) of edits, sources read before any write"""
    def fn(sec2):
        f = header_fields(cv, sec2)
        val = {k: (sec2[f[v][0]:f[v][0] + f[v][1]] if isinstance(v, str) else v) for k, v in edits.items()}
        b = bytearray(sec2)
        for k, v in val.items():
            assert len(v) == f[k][1]
            b[f[k][0]:f[k][0] + f[k][1]] = v
        return bytes(b)
    return with_section(raw, 2, fn)


def _contribution(cv, raw, i, edit):
    def fn(sec10):
        cs_hash, cons = p2.parse_mpc_params(sec10, cv)
        edit(cons[i])
        return p2.serialise_mpc_params(cs_hash, cons)
    return with_section(raw, 10, fn)


def swap_points(body, size, pick):
    """the section with the first two distinct points that satisfy pick swapped, and their indices"""
    pts = [body[i:i + size] for i in range(0, len(body), size)]
    i = next(k for k, p in enumerate(pts) if pick(p))
    j = next(k for k in range(i + 1, len(pts)) if pick(pts[k]) and pts[k] != pts[i])
    pts[i], pts[j] = pts[j], pts[i]
    return b"".join(pts), (i, j)


def tamper_table(curve):
    """[(label, init key, key, level, expected line)]: every row of the issue's table, from the golden keys, with valid curve points only"""
    cv = curve_record(curve)
    s1 = 2 * cv["n8q"]
    init, edge = gold(f"setup_{curve}_full.zkey"), gold(f"setup_{curve}_edge.zkey")
    key = gold(f"phase2_{curve}_full_c3.zkey")                          # c1, the beacon b2, c3
    sec2 = section(key, 2)
    f = header_fields(cv, sec2)
    pt = lambda k: sec2[f[k][0]:f[k][0] + f[k][1]]

    def flip(c):
        c["transcript"] = bytes([c["transcript"][0] ^ 1]) + c["transcript"][1:]
    rows = [
        ("transcript byte", init, _contribution(cv, key, 1, flip), "log", "INVALID(1): Inconsistent transcript "),
        ("g2_spx <- beta2", init, _contribution(cv, key, 2, lambda c: c.update(g2_spx=pt("beta2"))), "log", "INVALID(2): public key G1 and G2 do not have the same ration "),
        ("deltaAfter <- alpha1", init, _contribution(cv, key, 2, lambda c: c.update(deltaAfter=pt("alpha1"))), "log", "INVALID(2): deltaAfter does not fillow the public key "),
        ("beacon iterations 10 -> 11", init, _contribution(cv, key, 1, lambda c: c.update(numIterationsExp=11)), "log", "INVALID(1): Key of the beacon does not match. g1_s "),
        ("alpha1 <-> beta1", init, _header(cv, key, dict(alpha1="beta1", beta1="alpha1")), "error", "INVALID:  Invalid alpha1"),
        ("delta1 <- alpha1", init, _header(cv, key, dict(delta1="alpha1")), "error", "INVALID:  Invalid delta1"),
        ("delta2 <- gamma2", init, _header(cv, key, dict(delta2="gamma2")), "error", "INVALID:  Invalid delta2"),
        ("full key, edge init", edge, key, "error", "INVALID:  Different circuit parameters"),
        ("A point <- its neighbour", init, with_section(key, 5, lambda b: b[:s1] + b[2 * s1:3 * s1] + b[2 * s1:]), "error", "A section is not identical"),
        ("two L points swapped", init, with_section(key, 8, lambda b: swap_points(b, s1, any)[0]), "error", "L section does not match"),
        ("two H points swapped", init, with_section(key, 9, lambda b: swap_points(b, s1, lambda p: True)[0]), "error", "H section does not match"),
    ]
    assert section(key, 5)[s1:2 * s1] != section(key, 5)[2 * s1:3 * s1]
    return rows


def format_hash(b, title):
    """misc.formatHash, restated here apart from the driver's"""
    rows = ["\t\t" + " ".join(b[16 * i + 4 * j:16 * i + 4 * j + 4].hex() for j in range(4)) for i in range(4)]
    return title + "\n" + "\n".join(rows)


def expected_success_lines(name):
    """every line a successful verification of the golden key logs, debug lines included, from the recorded hashes"""
    curve = curve_of_file(name)
    cv = curve_record(curve)
    raw = gold(name)
    sec10, sec2 = section(raw, 10), section(raw, 2)
    cons = p2.parse_mpc_params(sec10, cv)[1]
    hashes = chain_hashes(name)
    assert len(cons) == len(hashes)
    n_vars, n_public, dom = struct.unpack_from("<III", sec2, 4 + cv["n8q"] + 4 + 32)
    out = [("debug", f"Same ratio check L section:  0/{n_vars - n_public - 1}"), ("debug", f"H Verification(tau):  0/{dom}"), ("debug", f"H Verification(lagrange):  0/{dom}"),
           ("info", format_hash(sec10[:64], "Circuit Hash: "))]
    for i in range(len(hashes) - 1, -1, -1):
        out.append(("info", "-------------------------"))
        out.append(("info", format_hash(bytes.fromhex(hashes[i]), f"contribution #{i + 1} {cons[i].get('name') or ''}:")))
        if cons[i]["type"] == 1:
            out += [("info", "Beacon generator: " + INDEX["files"][f"phase2_{curve}_full_b2.zkey"]["beaconHash"]), ("info", "Beacon iterations Exp: 10")]
    return out + [("info", "-------------------------"), ("info", "ZKey Ok!")]


class Log:
    def __init__(self):
        self.lines = []

    def __call__(self, level, text):
        self.lines.append((level, text))

    def verdict_lines(self):
        return [x for x in self.lines if x[0] != "debug"]
