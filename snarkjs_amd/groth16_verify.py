"""Batch Groth16 verification on the device: snarkjs.groth16.verify (src/groth16_verify.js:26-87) for many proofs against one key.

One verdict per proof with the reference's per-proof semantics; verify_all / verify_many_fast add the probabilistic check of a whole batch by
one final exponentiation. Codes: 1 valid ("OK!"), 0 pairing check
failed ("Invalid proof"), -1 a public input not in [0, r) ("Public inputs are not valid."), -2 a proof point not on the curve ("Proof
commitments are not valid."). The kernels are csrc/groth16_verify.hip; there is no CPU path.
"""
import numpy as np

from . import _verify_common as _vc
from . import zkmi
from ._verify_common import _FQ, _fq, _g1, _g2, _int

VALID, INVALID, BAD_PUBLIC, BAD_POINT = 1, 0, -1, -2
MESSAGES = {VALID: "OK!", INVALID: "Invalid proof", BAD_PUBLIC: "Public inputs are not valid.", BAD_POINT: "Proof commitments are not valid."}


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
        p, n8 = self.p, self.n8
        return _vc.pack(self, public_signals_list, proofs, lambda pr: _g1(pr["pi_a"], p, n8) + _g2(pr["pi_b"], p, n8) + _g1(pr["pi_c"], p, n8), 0, fewer=True)

    def verify_raw(self, proofs_u8, publics_u8, n_signals=None, n=None):
        """verdict codes (int8 array) of packed records: proofs_u8 n x 12 n8q bytes (pi_a | pi_b | pi_c as (x, y, z), standard form, LE),
        publics_u8 n x n_signals x 32 bytes (LE)"""
        return _vc.verify_raw(self, zkmi.lib().zkmi_groth16_verify_batch, 12 * self.n8, proofs_u8, publics_u8, n_signals, n, 0)

    def verify_codes(self, public_signals_list, proofs):
        recs, pubs, n_sig, pre = self.pack(public_signals_list, proofs)
        codes = self.verify_raw(recs, pubs, n_sig, len(proofs)) if proofs else np.zeros(0, np.int8)
        return [pre[i] if pre[i] is not None else int(c) for i, c in enumerate(codes)]

    def verify_many(self, public_signals_list, proofs):
        return [c == VALID for c in self.verify_codes(public_signals_list, proofs)]

    @property
    def record_bytes(self):
        return 12 * self.n8

    def verify_all_raw(self, proofs_u8, publics_u8, n_signals=None, n=None, seed=None):
        """(ok, codes) of packed records (the layouts of verify_raw) by the aggregated check: one Miller loop per proof, ONE final exponentiation
        for the batch. ok is True when every proof is valid, and False when one is not except with probability about 2^-127 over the 32-byte
        seed (drawn from the OS unless given; whoever made the proofs must not know it). codes[i]: proof i's input-check code (-1 / -2), or 1:
        it entered the check."""
        return _vc.verify_all_raw(self, zkmi.lib().zkmi_groth16_verify_aggregate, self.record_bytes, proofs_u8, publics_u8, n_signals, n, 0, seed)

    def verify_all(self, public_signals_list, proofs, seed=None):
        """are all of these valid? One final exponentiation for the whole batch (verify_all_raw); an empty batch is. Equals
        all(verify_many(...)) except with probability about 2^-127 over the seed."""
        return _vc.verify_all(self, public_signals_list, proofs, seed, None)

    def verify_many_fast(self, public_signals_list, proofs, seed=None):
        """verify_many for mostly honest traffic: [True, ...] when the aggregated check passes, else the answer of verify_many"""
        return _vc.verify_many_fast(self, public_signals_list, proofs, seed, None)

    def aggregate_trace(self, public_signals_list, proofs, seed):
        """zkmi_groth16_aggregate_trace_dev: (ok, codes, S_X, S_C, s, GT) — a sum as (x, y) or None, s = sum r_i, GT = final_exp of the
        product of the lanes' Miller values as 12 Fq coefficients in the oracle's w-basis"""
        n8 = self.n8
        ok, codes, sx, sc, more = _vc.aggregate_trace(self, zkmi.lib().zkmi_groth16_aggregate_trace_dev, public_signals_list, proofs, seed, 24 + 12 * n8)
        return ok, codes, sx, sc, int.from_bytes(more[:24], "little"), [int.from_bytes(more[24 + k * n8:24 + (k + 1) * n8], "little") for k in range(12)]

    def release(self):
        _vc.release(self, zkmi.lib().zkmi_groth16_vk_release)


_resident = {}                      # verify(): keys resident per vk content (a key load builds three line tables and a Miller value on one lane)


def verify(vk, public_signals, proof, logger=None):
    """groth16.verify(vk, publicSignals, proof, logger) with the reference's return value and logger messages. The key stays resident per vk
    content (release_all() frees them). One proof alone is latency-bound (one lane does the whole check): verify_many is the fast path."""
    code = _vc.resident(_resident, VerifyingKey, vk).verify_codes([public_signals], [proof])[0]
    if logger is not None:
        (logger.info if code == VALID else logger.error)(MESSAGES[code])
    return code == VALID


def release_all():
    """free the keys verify() keeps resident"""
    _vc.release_all(_resident)


def pairing(curve, g1_xyz, g2_xyz):
    """reduced pairings e(P_i, Q_i) (zkmi_pairing_dev): 12 Fq coefficients per pair in the oracle's w-basis, as Python ints"""
    cid, n8, _, _ = _FQ[curve]
    g1, g2 = zkmi.u8(g1_xyz), zkmi.u8(g2_xyz)
    n = g1.size // (3 * n8)
    out = np.zeros(max(n, 1) * 12 * n8, np.uint8)
    zkmi.check(zkmi.lib().zkmi_pairing_dev(cid, zkmi.ptr(g1), zkmi.ptr(g2), n, zkmi.ptr(out)))
    b = out.tobytes()
    return [[int.from_bytes(b[(12 * i + k) * n8:(12 * i + k + 1) * n8], "little") for k in range(12)] for i in range(n)]
