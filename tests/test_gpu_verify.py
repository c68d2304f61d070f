"""Batch Groth16 verification on the device (csrc/groth16_verify.hip) against the reference's verdicts: the golden proofs the reference
accepted, the tampers of tests/verify_vectors.py (expected codes, else the oracle's verdict), mixed batches of several sizes with exact
verdict arrays, keys with nPublic 0 / 2 / 40, the diagnostic pairing against the oracle, and a prover left untouched by a verify batch."""
import copy
import os
import random

import numpy as np
import pytest

import groth16_verify_oracle as O
import verify_vectors as V

pytestmark = pytest.mark.gpu
CURVE = {"bn128": O.BN254, "bls12381": O.BLS12381}


@pytest.fixture(scope="module")
def gv():
    from snarkjs_amd import groth16_verify
    return groth16_verify


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
def test_golden_and_tampers(gv, f):
    vk, pubs, proof = V.golden(f)
    E = CURVE[vk["curve"]]
    key = gv.VerifyingKey(vk)
    cases = [("golden", pubs, proof, 1)] + V.tampers(E, vk, pubs, proof)
    got = key.verify_codes([c[1] for c in cases], [c[2] for c in cases])
    for (label, pu, p, want), g in zip(cases, got):
        if want is None:
            want = V.oracle_verdict(E, vk, pu, p)
        assert g == want, label
    assert gv.verify(vk, pubs, proof) is True
    key.release()


def _trapdoor_key(E, base_vk, n_public, seed):
    """a verifying key with nPublic = n_public and a valid proof for random publics: IC_i = k_i alpha_1, delta = gamma, A = alpha_1,
    B = beta_2, C = -vk_x (then e(-A, B) e(alpha, beta) = 1 and e(vk_x, gamma) e(C, gamma) = 1)"""
    rnd = random.Random(seed)
    al = O._g1(base_vk["vk_alpha_1"])
    ic = [E.g1_mul(al, rnd.randrange(1, E.R)) for _ in range(n_public + 1)]
    vk = dict(base_vk)
    vk["nPublic"] = n_public
    vk["vk_delta_2"] = base_vk["vk_gamma_2"]
    vk["IC"] = [[str(p[0]), str(p[1]), "1"] for p in ic]
    pubs = [str(rnd.randrange(E.R)) for _ in range(n_public)]
    vx = ic[0]
    for v, p in zip(pubs, ic[1:]):
        vx = E.g1_add(vx, E.g1_mul(p, int(v)))
    c = E.g1_neg(vx)
    proof = {"pi_a": base_vk["vk_alpha_1"], "pi_b": base_vk["vk_beta_2"], "pi_c": ["0", "1", "0"] if c is None else [str(c[0]), str(c[1]), "1"]}
    return vk, pubs, proof


@pytest.mark.parametrize("f", ["groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"])
@pytest.mark.parametrize("n_public", [0, 2, 40])
def test_public_counts(gv, f, n_public):
    base, _, _ = V.golden(f)
    E = CURVE[base["curve"]]
    vk, pubs, proof = _trapdoor_key(E, base, n_public, 0x77 + n_public)
    key = gv.VerifyingKey(vk)
    lists, proofs, want = [pubs], [proof], [1]
    if n_public:
        lists.append([str((int(pubs[-1]) + 1) % E.R)] + pubs[:-1] if n_public == 1 else pubs[:-1] + [str((int(pubs[-1]) + 1) % E.R)])
        proofs.append(proof)
        want.append(0)
    assert key.verify_codes(lists, proofs) == want
    key.release()


@pytest.mark.parametrize("f,n", [("groth16_bn128_n1024.json", 1), ("groth16_bn128_n1024.json", 63), ("groth16_bn128_n1024.json", 65),
                                 ("groth16_bn128_n1024.json", 4097), ("groth16_bls12381_n1024.json", 1024)])
def test_batch_exact(gv, f, n):
    """mixed batch: the golden proof in affine and in Jacobian forms (a distinct z per entry, so every lane decodes different bytes), one in eight
    tampered at seeded positions; 32 sampled verdicts against the oracle"""
    vk, pubs, proof = V.golden(f)
    E = CURVE[vk["curve"]]
    rnd = random.Random(n)
    swapped = copy.deepcopy(proof)
    swapped["pi_a"], swapped["pi_c"] = proof["pi_c"], proof["pi_a"]
    bad_pub = [str((int(pubs[0]) + 1) % E.R)] + pubs[1:]
    lists, proofs, want = [], [], []
    for i in range(n):
        r = rnd.randrange(8)
        if r == 0:
            lists.append(bad_pub if rnd.randrange(2) else pubs)
            proofs.append(swapped if lists[-1] is pubs else proof)
            want.append(0)
        else:
            lists.append(pubs)
            proofs.append(proof if r == 1 else V.jacobian(E, proof, 2 + i, 3 + i))          # distinct encodings: distinct lane inputs
            want.append(1)
    key = gv.VerifyingKey(vk)
    got = key.verify_codes(lists, proofs)
    assert got == want
    for i in random.Random(1).sample(range(n), min(n, 32)):
        assert got[i] == V.oracle_verdict(E, vk, lists[i], proofs[i])
    key.release()


@pytest.mark.parametrize("f", ["groth16_bn128_n1024.json", "groth16_bls12381_n1024.json"])
def test_pairing_dev_matches_oracle(gv, f):
    vk, _, _ = V.golden(f)
    E = CURVE[vk["curve"]]
    n8 = 32 if vk["curve"] == "bn128" else 48
    al = O._g1(vk["vk_alpha_1"])
    pts = [E.g1_mul(al, k) for k in (3, 1 << 40)]
    qs = [vk["vk_beta_2"], vk["vk_gamma_2"]]
    g1 = b"".join(x.to_bytes(n8, "little") for p in pts for x in (p[0], p[1], 1))
    g2 = b"".join(int(c).to_bytes(n8, "little") for q in qs for pair in q[:3] for c in pair)
    got = gv.pairing(vk["curve"], np.frombuffer(g1, np.uint8), np.frombuffer(g2, np.uint8))
    for p, q, g in zip(pts, qs, got):
        assert g == E.final_exp(E.miller_loop(O._g2(q), p))


def test_prover_in_flight_unaffected(gv):
    """a proof submitted to a pipeline slot BEFORE a verify batch and collected AFTER it equals the same proof with no verify in between"""
    import oracle_lib as OL
    from snarkjs_amd import groth16, binfile, zkmi
    gd = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    zkey, wtns = open(os.path.join(gd, "groth16_bn128_n1024.zkey"), "rb").read(), open(os.path.join(gd, "groth16_bn128_n1024.wtns"), "rb").read()
    w = zkmi.u8(binfile.read_wtns(wtns)["witness"])
    r_m, s_m = OL.fr_e(OL.BN128, 3), OL.fr_e(OL.BN128, 5)
    L = zkmi.lib()
    d = zkmi.C.c_void_p(0)
    zkmi.check(L.zkmi_dev_alloc(w.size, zkmi.C.byref(d)))
    zkmi.check(L.zkmi_memcpy_h2d(d, zkmi.ptr(w), w.size))
    pk = groth16.ProvingKey(zkey)
    vk, pubs, proof = V.golden("groth16_bn128_n1024.json")
    key = gv.VerifyingKey(vk)
    try:
        pk.submit(d.value, 0)
        ref = [bytes(x) for x in pk.collect(0, r_m, s_m)]          # no verify in between
        for slot in (0, 1):
            pk.submit(d.value, slot)
            assert key.verify_many([pubs] * 4097, [proof] * 4097) == [True] * 4097
            got = [bytes(x) for x in pk.collect(slot, r_m, s_m)]
            assert got == ref, slot
    finally:
        key.release()
        pk.release()
        L.zkmi_dev_free(d)


def test_fewer_signals_than_public(gv):
    """n_signals < nPublic uses the first n_signals IC points (the reference builds vk_x from publicSignals.length); more is an error"""
    base, _, _ = V.golden("groth16_bn128_n1024.json")
    E = O.BN254
    vk, pubs, proof = _trapdoor_key(E, base, 5, 0x5)
    # a proof valid for the first 3 publics under the 5-public key: C = -(IC0 + sum_{j<3} pub_j IC_{j+1})
    vx = O._g1(vk["IC"][0])
    for v, p in zip(pubs[:3], vk["IC"][1:4]):
        vx = E.g1_add(vx, E.g1_mul(O._g1(p), int(v)))
    c = E.g1_neg(vx)
    proof3 = dict(proof, pi_c=[str(c[0]), str(c[1]), "1"])
    key = gv.VerifyingKey(vk)
    assert key.verify_codes([pubs[:3], pubs[:3]], [proof3, proof]) == [1, V.oracle_verdict(E, vk, pubs[:3], proof)]
    with pytest.raises(ValueError):
        key.verify_codes([pubs + ["1"]], [proof])
    key.release()
