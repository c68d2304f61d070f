"""Shared inputs of the Groth16 verifier tests: the golden (vk, proof, publicSignals) triples the reference accepted, and the tampered
variants of item 2 of the verifier's test plan. Pure Python; the expected verdicts come from oracle/groth16_verify_oracle.py."""
import copy
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_FILES = ["groth16_bn128_n1024.json", "groth16_bls12381_n1024.json", "groth16_valid_synth_n64.json"]


def golden(name):
    d = json.load(open(os.path.join(GOLDEN, name)))
    assert d["verified"] is True
    return d["vk"], d["publicSignals"], d["proof"]


def tampers(E, vk, pubs, proof):
    """(label, publicSignals, proof, expected code or None = the oracle's verdict) for one valid triple on curve E (oracle Pairing)"""
    out = []
    p = copy.deepcopy(proof)
    p["pi_a"], p["pi_c"] = proof["pi_c"], proof["pi_a"]
    out.append(("swap_a_c", pubs, p, 0))
    if pubs:
        out.append(("public_plus_1", [str((int(pubs[0]) + 1) % E.R)] + pubs[1:], proof, 0))
        out.append(("public_eq_r", [str(E.R)] + pubs[1:], proof, -1))
    p = copy.deepcopy(proof)
    p["pi_a"][0] = str(int(p["pi_a"][0]) + 1)
    out.append(("a_off_curve", pubs, p, -2))
    p = copy.deepcopy(proof)
    p["pi_b"][1][0] = str(int(p["pi_b"][1][0]) + 1)
    out.append(("b_off_curve", pubs, p, -2))
    for k in ("pi_a", "pi_c"):
        p = copy.deepcopy(proof)
        p[k] = ["0", "1", "0"]
        out.append((k + "_infinity", pubs, p, None))
    p = copy.deepcopy(proof)
    p["pi_b"] = [["0", "0"], ["1", "0"], ["0", "0"]]
    out.append(("pi_b_infinity", pubs, p, None))
    out.append(("jacobian", pubs, jacobian(E, proof, 7, 11), 1))
    q = off_subgroup_g2(E)
    if q is not None:
        p = copy.deepcopy(proof)
        p["pi_b"] = [[str(q[0][0]), str(q[0][1])], [str(q[1][0]), str(q[1][1])], ["1", "0"]]
        out.append(("pi_b_off_subgroup", pubs, p, None))
    return out


def jacobian(E, proof, za, zb):
    """the same proof with pi_a, pi_c written with Jacobian z = za and pi_b with z = (zb, 1)"""
    P = E.P
    p = copy.deepcopy(proof)
    for k in ("pi_a", "pi_c"):
        x, y = int(proof[k][0]), int(proof[k][1])
        p[k] = [str(x * za * za % P), str(y * za * za * za % P), str(za)]
    z = (zb, 1)
    z2 = E.f2_mul(z, z)
    z3 = E.f2_mul(z2, z)
    x = (int(proof["pi_b"][0][0]), int(proof["pi_b"][0][1]))
    y = (int(proof["pi_b"][1][0]), int(proof["pi_b"][1][1]))
    X, Y = E.f2_mul(x, z2), E.f2_mul(y, z3)
    p["pi_b"] = [[str(X[0]), str(X[1])], [str(Y[0]), str(Y[1])], [str(z[0]), str(z[1])]]
    return p


def off_subgroup_g2(E, start=1):
    """a point on the twist that is not in G2 (the twist's cofactor is large on both curves): the first x = (k, 1) with a square rhs"""
    P = E.P
    for k in range(start, start + 200):
        x = (k, 1)
        rhs = E.f2_add(E.f2_mul(E.f2_mul(x, x), x), E.TWIST_B)
        y = f2_sqrt(E, rhs)
        if y is not None:
            return (x, y)
    return None


def f2_sqrt(E, a):
    """square root in Fp2 = Fp[u]/(u^2+1) for p = 3 mod 4 (both curves), None if a is not a square"""
    P = E.P
    a0, a1 = a
    n = (a0 * a0 + a1 * a1) % P
    s = pow(n, (P + 1) // 4, P)
    if s * s % P != n:
        return None
    for t in (s, (-s) % P):
        x2 = (a0 + t) * pow(2, -1, P) % P
        x = pow(x2, (P + 1) // 4, P)
        if x * x % P != x2:
            continue
        if x == 0:
            continue
        y = a1 * pow(2 * x, -1, P) % P
        if E.f2_mul((x, y), (x, y)) == (a0 % P, a1 % P):
            return (x, y)
    if a1 % P == 0:                                                     # a in Fp: sqrt(a0) or u sqrt(-a0)
        for c, u in ((a0, False), ((-a0) % P, True)):
            r = pow(c, (P + 1) // 4, P)
            if r * r % P == c:
                return (0, r) if u else (r, 0)
    return None


def oracle_verdict(E, vk, pubs, proof):
    """code the reference's verifier gives: 1 OK, 0 invalid proof, -1 public inputs not valid, -2 commitments not valid"""
    import groth16_verify_oracle as O
    vals = [int(s) for s in pubs]
    if any(not (0 <= v < E.R) for v in vals):
        return -1
    pa, pb, pc = _affine1(E, proof["pi_a"]), _affine2(E, proof["pi_b"]), _affine1(E, proof["pi_c"])
    if not (E.g1_on_curve(pa) and E.g2_on_curve(pb) and E.g1_on_curve(pc)):
        return -2
    v = dict(vk)
    v["IC"] = vk["IC"][:len(vals) + 1]
    pr = {"pi_a": _obj1(pa), "pi_b": _obj2(pb), "pi_c": _obj1(pc)}
    return 1 if E.groth16_verify(v, pubs, pr) else 0


def _affine1(E, o):
    x, y, z = (int(v) % E.P for v in o[:3])
    if z == 0:
        return None
    zi = pow(z, -1, E.P)
    return (x * zi * zi % E.P, y * zi * zi * zi % E.P)


def _affine2(E, o):
    x, y, z = ((int(v[0]) % E.P, int(v[1]) % E.P) for v in o[:3])
    if z == (0, 0):
        return None
    zi = E.f2_inv(z)
    zi2 = E.f2_mul(zi, zi)
    return (E.f2_mul(x, zi2), E.f2_mul(y, E.f2_mul(zi2, zi)))


def _obj1(p):
    return ["0", "1", "0"] if p is None else [str(p[0]), str(p[1]), "1"]


def _obj2(p):
    return [["0", "0"], ["1", "0"], ["0", "0"]] if p is None else [[str(p[0][0]), str(p[0][1])], [str(p[1][0]), str(p[1][1])], ["1", "0"]]
