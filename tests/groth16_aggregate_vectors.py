"""The aggregated Groth16 check restated in Python for the tests, from pieces that are pinned elsewhere and nothing of the code under test: the G1
arithmetic, miller_loop, final_exp and pairing_product_is_one of oracle/groth16_verify_oracle.py and the challenge of
aggregate_verify_vectors.challenge (Keccak-256 by the library's host-side zkmi_keccak256).

    r_i = the first 16 bytes, little-endian, of Keccak-256(seed | LE64(i)), with bit 127 set
    E   = the proofs that pass the input checks, in the per-proof order: a public >= r -> -1, then pi_a / pi_b / pi_c on the curve -> -2
    F   = prod_E miller(-r_i A_i, B_i),  S_X = sum_E r_i vk_x_i,  S_C = sum_E r_i C_i,  s = sum_E r_i
    ok  = every code is 1  and  final_exp(F miller(S_X, gamma) miller(S_C, delta) miller(alpha, beta)^s) == 1
A pair with a point at infinity contributes 1. vk_x uses the first len(pubs) + 1 points of IC (fewer signals than nPublic are accepted)."""
import copy

import aggregate_verify_vectors as AV
import groth16_verify_oracle as GO
import verify_vectors as GV

seed_of = AV.seed_of
challenge = AV.challenge


def curve_of(vk):
    return GO.CURVES[vk.get("curve", "bn128")]


def structural_code(E, pubs, proof):
    if any(not (0 <= int(x) < E.R) for x in pubs):
        return -1
    pa, pb, pc = GV._affine1(E, proof["pi_a"]), GV._affine2(E, proof["pi_b"]), GV._affine1(E, proof["pi_c"])
    if not (E.g1_on_curve(pa) and E.g2_on_curve(pb) and E.g1_on_curve(pc)):
        return -2
    return 1


def vk_x(E, vk, pubs):
    ic = [GV._affine1(E, o) for o in vk["IC"]]
    acc = ic[0]
    for v, pt in zip(pubs, ic[1:]):
        acc = E.g1_add(acc, E.g1_mul(pt, int(v)))
    return acc


def restate(vk, batch, seed, pairing=True):
    """(ok, codes, S_X, S_C, s, GT) of a batch [(publicSignals, proof), ...] under vk; a sum is (x, y) or None, GT = final_exp(F) as the
    oracle's 12 coefficients. Without pairing no Miller loop is run and ok, GT are None."""
    E = curve_of(vk)
    codes, sx, sc, s, F = [], None, None, 0, E.F12_ONE
    for i, (pubs, proof) in enumerate(batch):
        c = structural_code(E, pubs, proof)
        codes.append(c)
        if c != 1:
            continue
        r = challenge(seed, i)
        a, b, cc = GV._affine1(E, proof["pi_a"]), GV._affine2(E, proof["pi_b"]), GV._affine1(E, proof["pi_c"])
        s += r
        sx = E.g1_add(sx, E.g1_mul(vk_x(E, vk, pubs), r))
        sc = E.g1_add(sc, E.g1_mul(cc, r))
        ra = E.g1_neg(E.g1_mul(a, r))
        if pairing and ra is not None and b is not None:
            F = E.f12_mul(F, E.miller_loop(b, ra))
    if not pairing:
        return None, codes, sx, sc, s, None
    f = F
    for g1, g2 in ((sx, GV._affine2(E, vk["vk_gamma_2"])), (sc, GV._affine2(E, vk["vk_delta_2"]))):
        if g1 is not None and g2 is not None:
            f = E.f12_mul(f, E.miller_loop(g2, g1))
    al, be = GV._affine1(E, vk["vk_alpha_1"]), GV._affine2(E, vk["vk_beta_2"])
    if al is not None and be is not None:
        f = E.f12_mul(f, E.f12_pow(E.miller_loop(be, al), s))
    ok = all(c == 1 for c in codes) and E.final_exp(f) == E.F12_ONE
    return ok, codes, sx, sc, s, E.final_exp(F)


def with_c_plus(E, proof, T, sign=1):
    """the proof with pi_c replaced by pi_c + sign * T (T a G1 point (x, y)): per-proof code 0"""
    p = copy.deepcopy(proof)
    p["pi_c"] = GV._obj1(E.g1_add(GV._affine1(E, proof["pi_c"]), T if sign > 0 else E.g1_neg(T)))
    return p


def alpha_of(E, vk):
    return GV._affine1(E, vk["vk_alpha_1"])
