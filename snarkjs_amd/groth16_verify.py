"""Batch Groth16 verification on the device: snarkjs.groth16.verify (src/groth16_verify.js:26-87) for many proofs against one key.

One verdict per proof with the reference's per-proof semantics (not a probabilistic batch check). Codes: 1 valid ("OK!"), 0 pairing check
failed ("Invalid proof"), -1 a public input not in [0, r) ("Public inputs are not valid."), -2 a proof point not on the curve ("Proof
commitments are not valid."). The kernels are csrc/groth16_verify.hip; there is no CPU path.
"""
import numpy as np

from . import zkmi

VALID, INVALID, BAD_PUBLIC, BAD_POINT = 1, 0, -1, -2
MESSAGES = {VALID: "OK!", INVALID: "Invalid proof", BAD_PUBLIC: "Public inputs are not valid.", BAD_POINT: "Proof commitments are not valid."}
_FQ = {"bn128": (zkmi.BN128, 32, 21888242871839275222246405745257275088696311157297823662689037894645226208583,
                 21888242871839275222246405745257275088548364400416034343698204186575808495617),
       "bls12381": (zkmi.BLS12381, 48, 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
                    0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001)}


def _int(v):
    """unstringifyBigInts of one value: decimal string (or "0x" hex) or int"""
    if isinstance(v, int):
        return v
    if isinstance(v, str):
        return int(v, 16) if v.startswith("0x") else int(v)
    raise TypeError(f"not a field element: {v!r}")


def _fq(v, p, n8):
    return (_int(v) % p).to_bytes(n8, "little")           # F.fromObject reduces modulo p


def _g1(o, p, n8):
    z = o[2] if len(o) > 2 else 1
    return _fq(o[0], p, n8) + _fq(o[1], p, n8) + _fq(z, p, n8)


def _g2(o, p, n8):
    z = o[2] if len(o) > 2 else [1, 0]
    return b"".join(_fq(c[0], p, n8) + _fq(c[1], p, n8) for c in (o[0], o[1], z))


class VerifyingKey:
    """A verifying key resident on the device (the object zKey.exportVerificationKey writes)."""

    def __init__(self, vk):
        name = vk.get("curve", "bn128")
        if name not in _FQ:
            raise ValueError(f"unsupported curve {name!r}")
        if vk.get("protocol", "groth16") != "groth16":
            raise ValueError("not a Groth16 verifying key")
        self.curve, self.n8, self.p, self.r = _FQ[name]
        self.n_public = len(vk["IC"]) - 1
        p, n8 = self.p, self.n8
        a = np.frombuffer(_g1(vk["vk_alpha_1"], p, n8), np.uint8).copy()
        b, g, d = (np.frombuffer(_g2(vk[k], p, n8), np.uint8).copy() for k in ("vk_beta_2", "vk_gamma_2", "vk_delta_2"))
        ic = np.frombuffer(b"".join(_g1(x, p, n8) for x in vk["IC"]), np.uint8).copy()
        h = zkmi.C.c_uint64(0)
        zkmi.check(zkmi.lib().zkmi_groth16_vk_load(self.curve, zkmi.ptr(a), zkmi.ptr(b), zkmi.ptr(g), zkmi.ptr(d), zkmi.ptr(ic), self.n_public, zkmi.C.byref(h)))
        self.handle = h.value

    def pack(self, public_signals_list, proofs):
        """(proofs_u8, publics_u8, n_signals, pre): packed records; pre[i] = -1 where a public is outside [0, r) (checked here, since
        negative values have no 32-byte form), else None"""
        n = len(proofs)
        if len(public_signals_list) != n:
            raise ValueError("one publicSignals list per proof")
        n_sig = len(public_signals_list[0]) if n else 0
        if n_sig > self.n_public:
            raise ValueError(f"{n_sig} public signals for a key with nPublic = {self.n_public}")
        p, n8, r = self.p, self.n8, self.r
        recs, pubs, pre = [], [], [None] * n
        for i, (sig, pr) in enumerate(zip(public_signals_list, proofs)):
            if len(sig) != n_sig:
                raise ValueError("every proof of a batch needs the same number of public signals")
            vals = [_int(s) for s in sig]
            if any(v < 0 or v >= r for v in vals):
                pre[i] = BAD_PUBLIC
                vals = [0] * n_sig
            pubs.append(b"".join(v.to_bytes(32, "little") for v in vals))
            recs.append(_g1(pr["pi_a"], p, n8) + _g2(pr["pi_b"], p, n8) + _g1(pr["pi_c"], p, n8))
        return np.frombuffer(b"".join(recs), np.uint8).copy(), np.frombuffer(b"".join(pubs), np.uint8).copy(), n_sig, pre

    def verify_raw(self, proofs_u8, publics_u8, n_signals=None, n=None):
        """verdict codes (int8 array) of packed records: proofs_u8 n x 12 n8q bytes (pi_a | pi_b | pi_c as (x, y, z), standard form, LE),
        publics_u8 n x n_signals x 32 bytes (LE)"""
        proofs_u8, publics_u8 = zkmi.u8(proofs_u8), zkmi.u8(publics_u8)
        rec = 12 * self.n8
        if n is None:
            n = proofs_u8.size // rec
        if n_signals is None:
            n_signals = publics_u8.size // (32 * n) if n else 0
        if proofs_u8.size != n * rec or publics_u8.size != n * n_signals * 32:
            raise ValueError("packed arrays do not match n and n_signals")
        out = np.zeros(max(n, 1), np.int8)
        pub = publics_u8 if publics_u8.size else np.zeros(1, np.uint8)
        zkmi.check(zkmi.lib().zkmi_groth16_verify_batch(self.handle, zkmi.ptr(proofs_u8), zkmi.ptr(pub), n_signals, n, zkmi.ptr(out)))
        return out[:n]

    def verify_codes(self, public_signals_list, proofs):
        recs, pubs, n_sig, pre = self.pack(public_signals_list, proofs)
        codes = self.verify_raw(recs, pubs, n_sig, len(proofs)) if proofs else np.zeros(0, np.int8)
        return [pre[i] if pre[i] is not None else int(c) for i, c in enumerate(codes)]

    def verify_many(self, public_signals_list, proofs):
        return [c == VALID for c in self.verify_codes(public_signals_list, proofs)]

    def release(self):
        if self.handle:
            zkmi.check(zkmi.lib().zkmi_groth16_vk_release(self.handle))
            self.handle = 0


_resident = {}                      # verify(): keys resident per vk content (a key load builds three line tables and a Miller value on one lane)


def verify(vk, public_signals, proof, logger=None):
    """groth16.verify(vk, publicSignals, proof, logger) with the reference's return value and logger messages. The key stays resident per vk
    content (release_all() frees them). One proof alone is latency-bound (one lane does the whole check): verify_many is the fast path."""
    import json
    kid = json.dumps(vk, sort_keys=True, default=str)
    key = _resident.get(kid)
    if key is None:
        key = _resident[kid] = VerifyingKey(vk)
    code = key.verify_codes([public_signals], [proof])[0]
    if logger is not None:
        (logger.info if code == VALID else logger.error)(MESSAGES[code])
    return code == VALID


def release_all():
    """free the keys verify() keeps resident"""
    for k in _resident.values():
        k.release()
    _resident.clear()


def pairing(curve, g1_xyz, g2_xyz):
    """reduced pairings e(P_i, Q_i) (zkmi_pairing_dev): 12 Fq coefficients per pair in the oracle's w-basis, as Python ints"""
    cid, n8, _, _ = _FQ[curve]
    g1, g2 = zkmi.u8(g1_xyz), zkmi.u8(g2_xyz)
    n = g1.size // (3 * n8)
    out = np.zeros(max(n, 1) * 12 * n8, np.uint8)
    zkmi.check(zkmi.lib().zkmi_pairing_dev(cid, zkmi.ptr(g1), zkmi.ptr(g2), n, zkmi.ptr(out)))
    b = out.tobytes()
    return [[int.from_bytes(b[(12 * i + k) * n8:(12 * i + k + 1) * n8], "little") for k in range(12)] for i in range(n)]
