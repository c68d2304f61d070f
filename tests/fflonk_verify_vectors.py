"""Shared inputs of the FFLONK verifier tests: the golden (vk, publicSignals, proof) triples the reference accepted, their tampered variants,
and the CPU expectation every device verdict is held to. Pure Python, nothing of the code under test.

The expectation is composed from two pinned pieces: oracle/fflonk_verify_oracle.py::verifier_values (pinned to the reference verifier's own
trace, tests/test_plonk_oracle.py::test_fflonk_verifier_trace) for A1 and B1 = W2, and oracle/groth16_verify_oracle.py's pairing (pinned to
the reference's Groth16 verdicts) for e(-A1, [1]_2) e(W2, X_2) == 1, preceded by the reference's input checks in the reference's order
(src/fflonk_verify.js:45-67): the number of public signals FIRST, then the commitments and the key's C0, then the public signals.
The pure-Python pairing takes about half a second: callers compute each distinct expectation once."""
import copy
import json
import os
import random

import fflonk_verify_oracle as FO
import groth16_verify_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_FILES = ["fflonk_bn128_small.json", "fflonk_bn128_n256.json"]
POINTS = ("C1", "C2", "W1", "W2")
EVALS = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3", "a", "b", "c", "z", "zw", "t1w", "t2w")
STARTED, FINISHED = ("info", "FFLONK VERIFIER STARTED"), ("info", "FFLONK VERIFIER FINISHED")
MESSAGES = {1: ("info", "PROOF VERIFIED SUCCESSFULLY"), 0: ("warn", "Invalid Proof"), -1: ("error", "Public inputs are not valid."),
            -2: ("error", "Proof commitments are not valid"), -3: ("error", "Number of public signals does not match with vk")}
E = GO.CURVES["bn128"]
# the generator of G2 (ffjavascript's curve.G2.g), ((x.c0, x.c1), (y.c0, y.c1))
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531))


def golden(name):
    d = json.load(open(os.path.join(GOLDEN, name)))
    assert d["verified"] is True
    return d["vk"], d["publicSignals"], d["proof"]


def affine(o):
    """G1.fromObject: (x, y, z) with z = 0 infinity (None), z = 1 affine, otherwise Jacobian; coordinates reduced modulo q"""
    x, y, z = (int(v) % E.P for v in (o[0], o[1], o[2] if len(o) > 2 else 1))
    if z == 0:
        return None
    zi = pow(z, -1, E.P)
    return (x * zi * zi % E.P, y * zi * zi * zi % E.P)


def obj(p):
    return ["0", "1", "0"] if p is None else [str(p[0]), str(p[1]), "1"]


def values(vk, pubs, proof):
    """verifier_values on a proof (and a key) whose points may be Jacobian or at infinity: the oracle reads affine objects, so they are
    normalised first. The oracle's transcript has no case for the point at infinity; it is handed over as (0, 0), which the oracle writes
    as the zero bytes G1.toRprUncompressed writes for it and its MSM reads as the point at infinity, and comes back as None."""
    def norm(o):
        p = affine(o)
        return ["0", "0", "1"] if p is None else obj(p)
    pr = {"polynomials": {k: norm(proof["polynomials"][k]) for k in POINTS}, "evaluations": proof["evaluations"]}
    val = FO.verifier_values(dict(vk, C0=norm(vk["C0"])), [int(x) for x in pubs], pr)
    if val["B1"] == (0, 0):
        val["B1"] = None
    return val


def pairing_ok(vk, val):
    return E.pairing_product_is_one([(E.g1_neg(val["A1"]), G2_GEN), (val["B1"], GO._g2(vk["X_2"]))])


def expected_code(vk, pubs, proof):
    """the reference's verdict as a code: 1 valid, 0 invalid proof, -1 public inputs not valid, -2 commitments not valid, -3 wrong signal count"""
    if len(pubs) != int(vk["nPublic"]):
        return -3
    if not all(E.g1_on_curve(affine(o)) for o in [proof["polynomials"][k] for k in POINTS] + [vk["C0"]]):
        return -2
    if any(not (0 <= int(x) < E.R) for x in pubs):
        return -1
    return 1 if pairing_ok(vk, values(vk, pubs, proof)) else 0


def other_point(proof, k):
    """a valid curve point that is not the commitment k: twice it"""
    p = affine(proof["polynomials"][k])
    return E.g1_add(p, p)


def jacobian(p, z):
    return [str(p[0] * z * z % E.P), str(p[1] * z * z * z % E.P), str(z)]


def with_point(proof, k, o):
    p = copy.deepcopy(proof)
    p["polynomials"][k] = o
    return p


def with_eval(proof, k, v):
    p = copy.deepcopy(proof)
    p["evaluations"][k] = str(v)
    return p


def off_curve(o):
    bad = list(copy.deepcopy(o))
    bad[0] = str((int(bad[0]) + 1) % E.P)
    return bad


def tampers(vk, pubs, proof, full=True):
    """(label, publicSignals, proof, expected code or None = ask expected_code) for one valid triple, all under the golden key. Codes
    written here follow from the reference's input checks alone; a 0 or 1 always comes from expected_code (None)."""
    out = []
    po, ev = proof["polynomials"], proof["evaluations"]
    for k in (POINTS if full else ("C1", "W2")):
        out.append((k + "_other_point", pubs, with_point(proof, k, obj(other_point(proof, k))), None))
        out.append((k + "_off_curve", pubs, with_point(proof, k, off_curve(po[k])), -2))
        out.append((k + "_infinity", pubs, with_point(proof, k, ["0", "1", "0"]), None))
        out.append((k + "_jacobian", pubs, with_point(proof, k, jacobian(affine(po[k]), 7 + len(k) + POINTS.index(k))), None))
    for k in (EVALS if full else ("ql", "t2w")):
        v = int(ev[k])
        out.append((k + "_plus_1", pubs, with_eval(proof, k, (v + 1) % E.R), None))
        out.append((k + "_minus_1", pubs, with_eval(proof, k, (v - 1) % E.R), None))
    out.append(("a_plus_r", pubs, with_eval(proof, "a", int(ev["a"]) + E.R), None))
    out.append(("inv_changed", pubs, with_eval(proof, "inv", (int(ev["inv"]) + 1) % E.R), None))
    for j in range(len(pubs)):
        for d in (1, -1):
            pu = list(pubs)
            pu[j] = str((int(pubs[j]) + d) % E.R)
            out.append((f"public{j}_{'plus' if d > 0 else 'minus'}_1", pu, proof, None))
        pu = list(pubs)
        pu[j] = str(E.R)
        out.append((f"public{j}_eq_r", pu, proof, -1))
    bad = with_point(proof, "C2", off_curve(po["C2"]))
    if pubs:
        out.append(("bad_point_and_bad_public", [str(E.R)] + list(pubs[1:]), bad, -2))
    out.append(("one_signal_more", list(pubs) + ["1"], proof, -3))
    if pubs:
        out.append(("one_signal_less", list(pubs[:-1]), proof, -3))
    out.append(("bad_point_and_wrong_count", list(pubs) + ["1"], bad, -3))          # the count is tested first: the opposite of PLONK
    return out


def with_c0_off_curve(vk):
    """the key with C0 moved off the curve: the reference loads it and answers -2 for every proof"""
    return dict(vk, C0=off_curve(vk["C0"]))


def with_n_public(vk, n, seed):
    """the key with nPublic set to n and n seeded public signals: a golden proof is invalid under it, yet every intermediate value and the
    verdict are defined"""
    rnd = random.Random(seed)
    v = dict(vk)
    v["nPublic"] = n
    return v, [str(rnd.randrange(E.R)) for _ in range(n)]


N_PUBLIC_CASES = (0, 1, 9, 17)          # 9 and 17 cross the chunk-of-eight boundary of the Lagrange terms
