"""Shared inputs of the PLONK verifier tests: the golden (vk, publicSignals, proof) triples the reference accepted, their tampered variants,
and the CPU expectation every device verdict is held to. Pure Python, nothing of the code under test.

The expectation is composed from two pinned pieces: oracle/plonk_verify_oracle.py::verifier_values (pinned to the reference verifier's own
trace) for A1 and B1, and oracle/groth16_verify_oracle.py's pairing (pinned to the reference's Groth16 verdicts) for
e(-A1, X_2) e(B1, [1]_2) == 1, preceded by the reference's input checks in the reference's order (src/plonk_verify.js:44-62).
The pure-Python pairing takes about half a second: callers compute each distinct expectation once."""
import copy
import json
import os
import random

import groth16_verify_oracle as GO
import plonk_verify_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_FILES = ["plonk_bn128_small.json", "plonk_bn128_n2048.json", "plonk_bls12381_small.json"]
POINTS = ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw")
EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")
MESSAGES = {1: ("info", "OK!"), 0: ("warn", "Invalid Proof"), -1: ("error", "Public inputs are not valid."), -2: ("error", "Proof commitments are not valid."),
            -3: ("error", "Invalid number of public inputs")}
# the generators of G2 (ffjavascript's curve.G2.g: the standard ones of both curves), ((x.c0, x.c1), (y.c0, y.c1))
G2_GEN = {
    "bn128": ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
              (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531)),
    "bls12381": ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
                  0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
                 (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
                  0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be)),
}


def golden(name):
    d = json.load(open(os.path.join(GOLDEN, name)))
    assert d["verified"] is True
    return d["vk"], d["publicSignals"], d["proof"]


def curve_of(vk):
    return GO.CURVES[vk.get("curve", "bn128")]


def affine(E, o):
    """G1.fromObject: (x, y, z) with z = 0 infinity (None), z = 1 affine, otherwise Jacobian; coordinates reduced modulo q"""
    x, y, z = (int(v) % E.P for v in (o[0], o[1], o[2] if len(o) > 2 else 1))
    if z == 0:
        return None
    zi = pow(z, -1, E.P)
    return (x * zi * zi % E.P, y * zi * zi * zi % E.P)


def obj(p):
    return ["0", "1", "0"] if p is None else [str(p[0]), str(p[1]), "1"]


def values(vk, pubs, proof):
    """verifier_values on a proof whose points may be Jacobian: the oracle reads affine objects, so they are normalised first"""
    E = curve_of(vk)
    pr = dict(proof)
    for k in POINTS:
        pr[k] = obj(affine(E, proof[k]))
    return PO.verifier_values(vk, [int(x) for x in pubs], pr)


def pairing_ok(vk, val):
    E = curve_of(vk)
    return E.pairing_product_is_one([(E.g1_neg(val["A1"]), GO._g2(vk["X_2"])), (val["B1"], G2_GEN[vk.get("curve", "bn128")])])


def expected_code(vk, pubs, proof):
    """the reference's verdict as a code: 1 OK, 0 invalid proof, -1 public inputs not valid, -2 commitments not valid, -3 wrong signal count"""
    E = curve_of(vk)
    if not all(E.g1_on_curve(affine(E, proof[k])) for k in POINTS):
        return -2
    if len(pubs) != int(vk["nPublic"]):
        return -3
    if any(not (0 <= int(x) < E.R) for x in pubs):
        return -1
    return 1 if pairing_ok(vk, values(vk, pubs, proof)) else 0


def other_point(E, proof, k):
    """a valid curve point that is not proof[k]: twice it (or another commitment when proof[k] is infinity)"""
    p = affine(E, proof[k])
    return E.g1_add(p, p) if p is not None else affine(E, proof["A" if k != "A" else "B"])


def jacobian(E, p, z):
    return [str(p[0] * z * z % E.P), str(p[1] * z * z * z % E.P), str(z)]


def with_(proof, **kw):
    p = copy.deepcopy(proof)
    p.update(kw)
    return p


def tampers(vk, pubs, proof, full=True):
    """(label, publicSignals, proof, expected code or None = ask expected_code) for one valid triple. Codes written here follow from the
    reference's input checks alone; a 0 or 1 always comes from expected_code (None)."""
    E = curve_of(vk)
    out = []
    pts = POINTS if full else ("A", "Z", "Wxiw")
    for k in pts:
        out.append((k + "_other_point", pubs, with_(proof, **{k: obj(other_point(E, proof, k))}), None))
        bad = copy.deepcopy(proof[k])
        bad[0] = str((int(bad[0]) + 1) % E.P)
        out.append((k + "_off_curve", pubs, with_(proof, **{k: bad}), -2))
        out.append((k + "_infinity", pubs, with_(proof, **{k: ["0", "1", "0"]}), None))
        out.append((k + "_jacobian", pubs, with_(proof, **{k: jacobian(E, affine(E, proof[k]), 7 + len(k))}), None))
    for k in (EVALS if full else ("eval_a", "eval_zw")):
        v = int(proof[k])
        out.append((k + "_plus_1", pubs, with_(proof, **{k: str((v + 1) % E.R)}), None))
        out.append((k + "_minus_1", pubs, with_(proof, **{k: str((v - 1) % E.R)}), None))
    out.append(("eval_a_plus_r", pubs, with_(proof, eval_a=str(int(proof["eval_a"]) + E.R)), None))
    for j in range(len(pubs)):
        for d in (1, -1):
            pu = list(pubs)
            pu[j] = str((int(pubs[j]) + d) % E.R)
            out.append((f"public{j}_{'plus' if d > 0 else 'minus'}_1", pu, proof, None))
        pu = list(pubs)
        pu[j] = str(E.R)
        out.append((f"public{j}_eq_r", pu, proof, -1))
    bad = copy.deepcopy(proof["C"])
    bad[1] = str((int(bad[1]) + 1) % E.P)
    if pubs:
        out.append(("bad_point_and_bad_public", [str(E.R)] + list(pubs[1:]), with_(proof, C=bad), -2))
    out.append(("one_signal_more", list(pubs) + ["1"], proof, -3))
    if pubs:
        out.append(("one_signal_less", list(pubs[:-1]), proof, -3))
    out.append(("bad_point_and_wrong_count", list(pubs) + ["1"], with_(proof, C=bad), -2))
    return out


def with_n_public(vk, n, seed):
    """the key with nPublic set to n and n seeded public signals: a golden proof is invalid under it, yet every intermediate value and the
    verdict are defined"""
    E = curve_of(vk)
    rnd = random.Random(seed)
    v = dict(vk)
    v["nPublic"] = n
    return v, [str(rnd.randrange(E.R)) for _ in range(n)]
