"""What the Bellman round-trip tests share: the golden index (tests/golden/bellman_golden.json, tools/gen_bellman_golden.js), the CPU oracle standing in for the
three device steps of snarkjs_amd/groth16_bellman.py, and the oracle's statement of the H basis change (group FFT + apply-key + conversion, as the reference
composes it)."""
import functools
import hashlib
import json
import os

import numpy as np

import oracle_lib as orc
from snarkjs_amd import groth16_setup as gs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX = json.load(open(os.path.join(GOLDEN, "bellman_golden.json")))
CURVES = ("bn128", "bls12381")
CIRCUITS = ("full", "edge")
R = {c["name"]: c["r"] for c in gs.CURVES.values()}


def gold(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def curve_record(curve):
    return next(c for c in gs.CURVES.values() if c["name"] == curve)


def sections_of(raw):
    """[(type, body)] in file order"""
    src = gs._Source(raw)
    found = [(off, t, ln) for t, v in gs.read_sections(src, b"zkey", 2).items() for off, ln in v]
    return [(t, src.read(off, ln)) for off, t, ln in sorted(found)]


def mont(curve, v):
    r = R[curve]
    return np.frombuffer((((v % r) << 256) % r).to_bytes(32, "little"), np.uint8)


def root(curve, i):
    """Fr.w[i] as an integer"""
    r = R[curve]
    return int.from_bytes(orc.fr_w(orc.CURVE_ID[curve], i).tobytes(), "little") * pow(1 << 256, -1, r) % r


def h_export(curve, lem, power):
    """src/zkey_export_bellman.js:43-52 by the oracle: fft, batchApplyKey(-2, Fr.w[power + 1]), the last point dropped, batchLEMtoU"""
    c = orc.CURVE_ID[curve]
    t = orc.group_apply_key(c, 1, orc.group_fft(c, 1, lem), mont(curve, -2), mont(curve, root(curve, power + 1)))
    return orc.group_convert(c, 1, "LEMtoU", t[:t.size - 2 * orc.n8q(c)]).tobytes()


def h_import(curve, u, power):
    """src/zkey_import_bellman.js:133-142 by the oracle: batchUtoLEM, a zero last point, batchApplyKey(-(1/2), 1 / Fr.w[power + 1]), ifft"""
    c, r = orc.CURVE_ID[curve], R[curve]
    lem = np.concatenate([orc.group_convert(c, 1, "UtoLEM", u), np.zeros(2 * orc.n8q(c), np.uint8)])
    t = orc.group_apply_key(c, 1, lem, mont(curve, -pow(2, -1, r)), mont(curve, pow(root(curve, power + 1), -1, r)))
    return orc.group_fft(c, 1, t, inverse=True).tobytes()


class OracleDevice:
    """the CPU oracle in the place of groth16_bellman.Device"""

    def convert(self, cv, group, kind, body):
        return orc.group_convert(cv["id"], group, {0: "LEMtoU", 1: "UtoLEM"}[kind], body).tobytes() if body else b""

    def h_section(self, cv, body, power, direction):
        return h_import(cv["name"], body, power) if direction else h_export(cv["name"], body, power)

    def scale_u(self, cv, body_u, k_mont):
        if not body_u:
            return b""
        c = cv["id"]
        t = orc.group_apply_key(c, 1, orc.group_convert(c, 1, "UtoLEM", body_u), np.frombuffer(bytes(k_mont), np.uint8), orc.fr_one(c))
        return orc.group_convert(c, 1, "LEMtoU", t).tobytes()


def sha(b):
    return hashlib.sha256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def subgroup_points(curve, n, holes=()):
    """n G1 points of the r-torsion as LEM bytes (k_i G for k_i from a seeded generator), infinity at the places `holes`"""
    c = orc.CURVE_ID[curve]
    s = 2 * orc.n8q(c)
    rng = np.random.default_rng(0xBE11 + n + c)
    ks = [int.from_bytes(rng.bytes(32), "little") % R[curve] for _ in range(n)]
    pts = np.concatenate([orc.to_affine(c, 1, orc.generator_mul(c, 1, k)) for k in ks])
    for h in holes:
        pts[h * s:(h + 1) * s] = 0
    return pts.tobytes()
