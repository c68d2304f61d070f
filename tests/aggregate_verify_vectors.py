"""The aggregated PLONK / FFLONK check restated in Python for the tests: the challenges r_i, the sums S_P = sum r_i P_i and S_Q = sum r_i Q_i and the
verdict, from pieces that are pinned elsewhere and nothing of the code under test: each proof's pair from oracle/plonk_verify_oracle.py /
oracle/fflonk_verify_oracle.py (through plonk_verify_vectors.values / fflonk_verify_vectors.values), the G1 arithmetic and the pairing of
oracle/groth16_verify_oracle.py, and Keccak-256 by the library's host-side zkmi_keccak256 (pinned to the reference's transcript hash by the
prover tests).

    r_i = the first 16 bytes, little-endian, of Keccak-256(seed | LE64(i)), with bit 127 set
    PLONK:  (P, Q) = (A1, B1), e(-S_P, X_2) e(S_Q, [1]_2) == 1;      FFLONK: (P, Q) = (A1, W2), e(-S_P, [1]_2) e(S_Q, X_2) == 1
A proof that fails the input checks keeps its code (-2 / -1, in its protocol's order) and stays out of the sums; one that passes has code 1."""
import ctypes
import random

import fflonk_verify_vectors as FV
import groth16_verify_oracle as GO
import plonk_verify_vectors as PV

# what final_exp_chain returns is final_exp(f)^K: K = 2x(6x^2 + 3x + 1) on BN254 (x from the loop scalar 6x + 2), 3 on BLS12-381
X_BN = (GO.BN254.loop - 2) // 6
CHAIN_K = {"bn128": 2 * X_BN * (6 * X_BN * X_BN + 3 * X_BN + 1), "bls12381": 3}


def keccak256(data):
    from snarkjs_amd import zkmi
    out = ctypes.create_string_buffer(32)
    assert zkmi.lib().zkmi_keccak256(bytes(data), len(data), out) == 0
    return out.raw


def challenge(seed, i):
    assert len(seed) == 32
    return int.from_bytes(keccak256(bytes(seed) + int(i).to_bytes(8, "little"))[:16], "little") | (1 << 127)


def seed_of(tag):
    """a fixed 32-byte seed per tag"""
    rnd = random.Random(tag)
    return bytes(rnd.randrange(256) for _ in range(32))


def structural_code(proto, vk, pubs, proof):
    """the input checks of one proof, in its protocol's order, without the pairing: -3 / -2 / -1, or 1 = enters the sums"""
    if proto == "plonk":
        E = PV.curve_of(vk)
        if not all(E.g1_on_curve(PV.affine(E, proof[k])) for k in PV.POINTS):
            return -2
        if len(pubs) != int(vk["nPublic"]):
            return -3
    else:
        E = FV.E
        if len(pubs) != int(vk["nPublic"]):
            return -3
        if not all(E.g1_on_curve(FV.affine(o)) for o in [proof["polynomials"][k] for k in FV.POINTS] + [vk["C0"]]):
            return -2
    if any(not (0 <= int(x) < E.R) for x in pubs):
        return -1
    return 1


def pair_of(proto, vk, pubs, proof):
    val = (PV if proto == "plonk" else FV).values(vk, pubs, proof)
    return val["A1"], val["B1"]


def restate(proto, vk, batch, seed):
    """(ok, codes, S_P, S_Q) of a batch [(publicSignals, proof), ...] under vk; a sum is (x, y) or None"""
    E = PV.curve_of(vk) if proto == "plonk" else FV.E
    codes, sp, sq = [], None, None
    for i, (pubs, proof) in enumerate(batch):
        c = structural_code(proto, vk, pubs, proof)
        codes.append(c)
        if c == 1:
            r = challenge(seed, i)
            p, q = pair_of(proto, vk, pubs, proof)
            sp = E.g1_add(sp, E.g1_mul(p, r))
            sq = E.g1_add(sq, E.g1_mul(q, r))
    if proto == "plonk":
        pairs = [(E.g1_neg(sp), GO._g2(vk["X_2"])), (sq, PV.G2_GEN[vk.get("curve", "bn128")])]
    else:
        pairs = [(E.g1_neg(sp), FV.G2_GEN), (sq, GO._g2(vk["X_2"]))]
    ok = all(c == 1 for c in codes) and E.pairing_product_is_one(pairs)
    return ok, codes, sp, sq


def sums_from_bytes(b, n8):
    """S_P, S_Q of a *_aggregate_trace_dev report: 4 x n8 bytes, zero = infinity"""
    v = [int.from_bytes(bytes(b[i * n8:(i + 1) * n8]), "little") for i in range(4)]
    return (None if (v[0], v[1]) == (0, 0) else (v[0], v[1])), (None if (v[2], v[3]) == (0, 0) else (v[2], v[3]))
