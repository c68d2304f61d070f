"""Batch PLONK verification on the device: snarkjs.plonk.verify (src/plonk_verify.js:29-123) for many proofs against one key.

One verdict per proof with the reference's per-proof semantics; verify_all / verify_many_fast add the probabilistic check of a whole batch by
one pairing. Codes, in the order the reference tests:
-2 a commitment not on the curve ("Proof commitments are not valid."), -3 a wrong number of public signals ("Invalid number of public
inputs"), -1 a public input not in [0, r) ("Public inputs are not valid."), 0 pairing check failed ("Invalid Proof", logged with warn),
1 valid ("OK!"). -4 ("Proof evaluations are not valid") is reserved: the reference's test reads already reduced values and cannot fire.
The kernels are csrc/plonk_verify.hip; there is no CPU path.
"""
import numpy as np

from . import zkmi
from . import _verify_common as _vc
from ._verify_common import _FQ, _fr, _g1, _g2, _int, _root

VALID, INVALID, BAD_PUBLIC, BAD_POINT, BAD_COUNT = 1, 0, -1, -2, -3
MESSAGES = {VALID: "OK!", INVALID: "Invalid Proof", BAD_PUBLIC: "Public inputs are not valid.", BAD_POINT: "Proof commitments are not valid.",
            BAD_COUNT: "Invalid number of public inputs"}
KEY_POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")
PROOF_POINTS = ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw")
PROOF_EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")
TRACE_FR = ("beta", "gamma", "alpha", "xi", "v1", "u", "L1", "pi", "r0")


class VerifyingKey:
    """A PLONK verifying key resident on the device (the object zKey.exportVerificationKey writes, with X_2)."""

    def __init__(self, vk):
        name = vk.get("curve", "bn128")
        if name not in _FQ:
            raise ValueError(f"unsupported curve {name!r}")
        if vk.get("protocol") != "plonk":
            raise ValueError("not a PLONK verifying key")
        self.curve, self.n8, self.p, self.r = _FQ[name]
        self.n_public, self.power = int(vk["nPublic"]), int(vk["power"])
        p, n8 = self.p, self.n8
        g1 = np.frombuffer(b"".join(_g1(vk[k], p, n8) for k in KEY_POINTS), np.uint8).copy()
        x2 = np.frombuffer(_g2(vk["X_2"], p, n8), np.uint8).copy()
        k1, k2 = (np.frombuffer((_int(vk[k]) % self.r).to_bytes(32, "little"), np.uint8).copy() for k in ("k1", "k2"))
        h = zkmi.C.c_uint64(0)
        zkmi.check(zkmi.lib().zkmi_plonk_vk_load(self.curve, zkmi.ptr(g1), zkmi.ptr(x2), zkmi.ptr(k1), zkmi.ptr(k2), self.power, self.n_public, zkmi.C.byref(h)))
        self.handle = h.value

    @property
    def record_bytes(self):
        return 27 * self.n8 + 192

    def pack(self, public_signals_list, proofs):
        """(proofs_u8, publics_u8, n_signals, pre): packed records; pre[i] = -1 where a public is outside [0, r) (checked here, since
        such values may have no 32-byte form; a bad commitment still wins: verify_codes), else None. Every proof of a batch carries the
        same number of signals; a number other than the key's nPublic is packed as given and refused by the device call."""
        p, n8, r = self.p, self.n8, self.r
        return _vc.pack(self, public_signals_list, proofs, lambda pr: b"".join(_g1(pr[k], p, n8) for k in PROOF_POINTS) + b"".join(_fr(pr[k], r) for k in PROOF_EVALS), self.n_public)

    def verify_raw(self, proofs_u8, publics_u8, n_signals=None, n=None):
        """verdict codes (int8 array) of packed records: proofs_u8 n x (27 n8q + 192) bytes (nine commitments as (x, y, z), six evaluations,
        standard form, LE), publics_u8 n x n_signals x 32 bytes (LE). Raises ZkmiError "Invalid number of public inputs" when n_signals is
        not the key's nPublic."""
        return _vc.verify_raw(self, zkmi.lib().zkmi_plonk_verify_batch, self.record_bytes, proofs_u8, publics_u8, n_signals, n, self.n_public)

    def _on_curve(self, o):
        """G1.isValid of a point in object form, on the host: only used to keep the reference's order (commitments before the signal count)
        for a call the device refuses as a whole"""
        p = self.p
        x, y, z = (_int(v) % p for v in (o[0], o[1], o[2] if len(o) > 2 else 1))
        if z == 0:
            return True
        b = 3 if self.n8 == 32 else 4
        z2 = z * z % p
        return (y * y - x * x * x - b * z2 * z2 * z2) % p == 0

    def verify_codes(self, public_signals_list, proofs):
        if not proofs:
            return []
        recs, pubs, n_sig, pre = self.pack(public_signals_list, proofs)
        if n_sig != self.n_public:
            _vc.refused_count(self, recs, pubs, n_sig, len(proofs), MESSAGES[BAD_COUNT])
            return [BAD_COUNT if all(self._on_curve(pr[k]) for k in PROOF_POINTS) else BAD_POINT for pr in proofs]
        codes = self.verify_raw(recs, pubs, n_sig, len(proofs))
        return [int(c) if pre[i] is None or int(c) == BAD_POINT else pre[i] for i, c in enumerate(codes)]

    def verify_many(self, public_signals_list, proofs):
        return [c == VALID for c in self.verify_codes(public_signals_list, proofs)]

    def verify_all_raw(self, proofs_u8, publics_u8, n_signals=None, n=None, seed=None):
        """(ok, codes) of packed records (the layouts of verify_raw) by the aggregated check: ONE pairing check for the batch. ok is True when
        every proof is valid, and False when one is not except with probability about 2^-127 over the 32-byte seed (drawn from the OS unless
        given; whoever made the proofs must not know it). codes[i]: proof i's input-check code (-2 / -1), or 1: it entered the check."""
        return _vc.verify_all_raw(self, zkmi.lib().zkmi_plonk_verify_aggregate, self.record_bytes, proofs_u8, publics_u8, n_signals, n, self.n_public, seed)

    def verify_all(self, public_signals_list, proofs, seed=None):
        """are all of these valid? One pairing check for the whole batch (verify_all_raw); an empty batch is. Equals all(verify_many(...))
        except with probability about 2^-127 over the seed."""
        return _vc.verify_all(self, public_signals_list, proofs, seed, MESSAGES[BAD_COUNT])

    def verify_many_fast(self, public_signals_list, proofs, seed=None):
        """verify_many for mostly honest traffic: [True, ...] when the aggregated check passes, else the answer of verify_many"""
        return _vc.verify_many_fast(self, public_signals_list, proofs, seed, MESSAGES[BAD_COUNT])

    def aggregate_trace(self, public_signals_list, proofs, seed):
        """zkmi_plonk_aggregate_trace_dev: (ok, codes, S_P, S_Q), a sum as (x, y) or None"""
        return _vc.aggregate_trace(self, zkmi.lib().zkmi_plonk_aggregate_trace_dev, public_signals_list, proofs, seed)

    def trace(self, public_signals, proof):
        """zkmi_plonk_verify_trace_dev for one proof: dict of beta gamma alpha xi v1 u L1 pi r0 (ints) and A1, B1 ((x, y) or None)"""
        return _vc.trace(self, zkmi.lib().zkmi_plonk_verify_trace_dev, TRACE_FR, public_signals, proof)

    def release(self):
        _vc.release(self, zkmi.lib().zkmi_plonk_vk_release)


_resident = {}                      # verify(): keys resident per vk content (a key load builds two line tables on one lane)


def verify(vk, public_signals, proof, logger=None):
    """plonk.verify(vk, publicSignals, proof, logger) with the reference's return value and logger messages ("PLONK VERIFIER STARTED" first;
    "Invalid Proof" goes to logger.warn). Where the reference throws — a bad commitment without a logger — this returns False. The key stays
    resident per vk content (release_all() frees them). One proof alone is latency-bound: verify_many is the fast path."""
    key = _vc.resident(_resident, VerifyingKey, vk)
    if logger is not None:
        logger.info("PLONK VERIFIER STARTED")
    code = key.verify_codes([public_signals], [proof])[0]
    if logger is not None:
        (logger.info if code == VALID else logger.warn if code == INVALID else logger.error)(MESSAGES[code])
    return code == VALID


def release_all():
    """free the keys verify() keeps resident"""
    _vc.release_all(_resident)


def vk_from_zkey(zkey_bytes):
    """zKey.exportVerificationKey for a PLONK key (plonkVk, src/zkey_export_verificationkey.js:92-121), X_2 and w included. Needs no device."""
    z = _vc.ZkeyHeader(zkey_bytes, 2, "plonk")
    if z.name is None:
        raise ValueError("unsupported curve")
    vk = {"protocol": "plonk", "curve": z.name, "nPublic": z.n_public, "power": z.power}
    for k in ("k1", "k2"):
        vk[k] = str(z.fr())
    for k in KEY_POINTS:
        vk[k] = z.g1()
    vk["X_2"] = z.g2()
    vk["w"] = str(_root(z.cid, z.power, z.r))
    return vk
