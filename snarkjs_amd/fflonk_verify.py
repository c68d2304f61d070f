"""Batch FFLONK verification on the device: snarkjs.fflonk.verify (src/fflonk_verify.js:28-137) for many proofs against one key. BN254 only:
the reference's fflonk.setup / fflonk.prove do not work on BLS12-381, so a BLS12-381 key is refused.

One verdict per proof with the reference's per-proof semantics; verify_all / verify_many_fast add the probabilistic check of a whole batch by
one pairing. Codes, in the order the reference tests
(which differs from PLONK's: the count comes first): -3 a wrong number of public signals ("Number of public signals does not match with vk"),
-2 a commitment or the key's C0 not on the curve ("Proof commitments are not valid"), -1 a public input not in [0, r) ("Public inputs are not
valid."), 0 pairing check failed ("Invalid Proof", logged with warn), 1 valid ("PROOF VERIFIED SUCCESSFULLY"). -4 ("Proof evaluations are not
valid.") is reserved: the reference's test reads already reduced values and cannot fire. The proof's evaluations.inv is not read.
The kernels are csrc/fflonk_verify.hip; there is no CPU path.
"""
import numpy as np

from . import zkmi
from . import _verify_common as _vc
from ._verify_common import _FQ, _fr, _g1, _g2, _int, _root

VALID, INVALID, BAD_PUBLIC, BAD_POINT, BAD_COUNT = 1, 0, -1, -2, -3
MESSAGES = {VALID: "PROOF VERIFIED SUCCESSFULLY", INVALID: "Invalid Proof", BAD_PUBLIC: "Public inputs are not valid.", BAD_POINT: "Proof commitments are not valid",
            BAD_COUNT: "Number of public signals does not match with vk"}
KEY_CONSTS = ("k1", "k2", "w3", "w4", "w8", "wr")
PROOF_POINTS = ("C1", "C2", "W1", "W2")
PROOF_EVALS = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3", "a", "b", "c", "z", "zw", "t1w", "t2w")
TRACE_FR = ("beta", "gamma", "xi", "alpha", "y", "r0", "r1", "r2")


class VerifyingKey:
    """An FFLONK verifying key resident on the device (the object zKey.exportVerificationKey writes, with X_2 and C0). A key whose C0 is
    not on the curve loads, and every proof under it gets -2, as the reference has it; an X_2 off its curve is refused. w3 w4 w8 wr are
    taken as given (the reference does not check them). The reference reads vk.w in one place and Fr.w[power] in another; one value is used
    here, so a vk.w that is present and differs from Fr.w[power] is refused."""

    def __init__(self, vk):
        name = vk.get("curve", "bn128")
        if name not in _FQ:
            raise ValueError(f"unsupported curve {name!r}")
        if vk.get("protocol") != "fflonk":
            raise ValueError("not an FFLONK verifying key")
        if name != "bn128":
            raise ValueError(f"FFLONK verification serves bn128 only, not curve {name!r}: the reference has no FFLONK on it")
        self.curve, self.n8, self.p, self.r = _FQ[name]
        self.n_public, self.power = int(vk["nPublic"]), int(vk["power"])
        if "w" in vk and _int(vk["w"]) % self.r != _root(self.curve, self.power, self.r):
            raise ValueError("vk.w is not Fr.w[power]")
        p, n8 = self.p, self.n8
        c0 = np.frombuffer(_g1(vk["C0"], p, n8), np.uint8).copy()
        x2 = np.frombuffer(_g2(vk["X_2"], p, n8), np.uint8).copy()
        consts = np.frombuffer(b"".join((_int(vk[k]) % self.r).to_bytes(32, "little") for k in KEY_CONSTS), np.uint8).copy()
        h = zkmi.C.c_uint64(0)
        zkmi.check(zkmi.lib().zkmi_fflonk_vk_load(self.curve, zkmi.ptr(c0), zkmi.ptr(x2), zkmi.ptr(consts), self.power, self.n_public, zkmi.C.byref(h)))
        self.handle = h.value

    @property
    def record_bytes(self):
        return 12 * self.n8 + 480

    def pack(self, public_signals_list, proofs):
        """(proofs_u8, publics_u8, n_signals, pre): packed records; pre[i] = -1 where a public is outside [0, r) (checked here, since
        such values may have no 32-byte form; a bad commitment still wins: verify_codes), else None. Every proof of a batch carries the
        same number of signals; a number other than the key's nPublic is packed as given and refused by the device call."""
        p, n8, r = self.p, self.n8, self.r
        return _vc.pack(self, public_signals_list, proofs, lambda pr: b"".join(_g1(pr["polynomials"][k], p, n8) for k in PROOF_POINTS) + b"".join(_fr(pr["evaluations"][k], r) for k in PROOF_EVALS), self.n_public)

    def verify_raw(self, proofs_u8, publics_u8, n_signals=None, n=None):
        """verdict codes (int8 array) of packed records: proofs_u8 n x (12 n8q + 480) bytes (C1 C2 W1 W2 as (x, y, z), fifteen evaluations
        ql qr qm qo qc s1 s2 s3 a b c z zw t1w t2w, standard form, LE), publics_u8 n x n_signals x 32 bytes (LE). Raises ZkmiError "Number of
        public signals does not match with vk" when n_signals is not the key's nPublic."""
        return _vc.verify_raw(self, zkmi.lib().zkmi_fflonk_verify_batch, self.record_bytes, proofs_u8, publics_u8, n_signals, n, self.n_public)

    def verify_codes(self, public_signals_list, proofs):
        if not proofs:
            return []
        recs, pubs, n_sig, pre = self.pack(public_signals_list, proofs)
        if n_sig != self.n_public:                 # the reference tests the count first: -3 whatever the commitments are
            _vc.refused_count(self, recs, pubs, n_sig, len(proofs), MESSAGES[BAD_COUNT])
            return [BAD_COUNT] * len(proofs)
        codes = self.verify_raw(recs, pubs, n_sig, len(proofs))
        return [int(c) if pre[i] is None or int(c) == BAD_POINT else pre[i] for i, c in enumerate(codes)]

    def verify_many(self, public_signals_list, proofs):
        return [c == VALID for c in self.verify_codes(public_signals_list, proofs)]

    def verify_all_raw(self, proofs_u8, publics_u8, n_signals=None, n=None, seed=None):
        """(ok, codes) of packed records (the layouts of verify_raw) by the aggregated check: ONE pairing check for the batch. ok is True when
        every proof is valid, and False when one is not except with probability about 2^-127 over the 32-byte seed (drawn from the OS unless
        given; whoever made the proofs must not know it). codes[i]: proof i's input-check code (-2 / -1), or 1: it entered the check."""
        return _vc.verify_all_raw(self, zkmi.lib().zkmi_fflonk_verify_aggregate, self.record_bytes, proofs_u8, publics_u8, n_signals, n, self.n_public, seed)

    def verify_all(self, public_signals_list, proofs, seed=None):
        """are all of these valid? One pairing check for the whole batch (verify_all_raw); an empty batch is. Equals all(verify_many(...))
        except with probability about 2^-127 over the seed."""
        return _vc.verify_all(self, public_signals_list, proofs, seed, MESSAGES[BAD_COUNT])

    def verify_many_fast(self, public_signals_list, proofs, seed=None):
        """verify_many for mostly honest traffic: [True, ...] when the aggregated check passes, else the answer of verify_many"""
        return _vc.verify_many_fast(self, public_signals_list, proofs, seed, MESSAGES[BAD_COUNT])

    def aggregate_trace(self, public_signals_list, proofs, seed):
        """zkmi_fflonk_aggregate_trace_dev: (ok, codes, S_P, S_Q), a sum as (x, y) or None"""
        return _vc.aggregate_trace(self, zkmi.lib().zkmi_fflonk_aggregate_trace_dev, public_signals_list, proofs, seed)

    def trace(self, public_signals, proof):
        """zkmi_fflonk_verify_trace_dev for one proof: dict of beta gamma xi alpha y r0 r1 r2 (ints) and A1, B1 ((x, y) or None)"""
        return _vc.trace(self, zkmi.lib().zkmi_fflonk_verify_trace_dev, TRACE_FR, public_signals, proof)

    def release(self):
        _vc.release(self, zkmi.lib().zkmi_fflonk_vk_release)


_resident = {}                      # verify(): keys resident per vk content (a key load builds two line tables on one lane)


def verify(vk, public_signals, proof, logger=None):
    """fflonk.verify(vk, publicSignals, proof, logger) with the reference's return value and its verdict messages: "FFLONK VERIFIER STARTED"
    first, then one of MESSAGES ("Invalid Proof" goes to logger.warn, the errors to logger.error), and "FFLONK VERIFIER FINISHED" after a
    pairing verdict (0 / 1) only, as the reference returns early on the input checks. The reference's progress lines (the settings block,
    "> Computing ...", the challenge values) are not reproduced. Where the reference throws — a wrong number of signals without a logger,
    its logger.error is unguarded — this returns False. The key stays resident per vk content (release_all() frees them). One proof alone
    is latency-bound: verify_many is the fast path."""
    key = _vc.resident(_resident, VerifyingKey, vk)
    if logger is not None:
        logger.info("FFLONK VERIFIER STARTED")
    code = key.verify_codes([public_signals], [proof])[0]
    if logger is not None:
        (logger.info if code == VALID else logger.warn if code == INVALID else logger.error)(MESSAGES[code])
        if code in (VALID, INVALID):
            logger.info("FFLONK VERIFIER FINISHED")
    return code == VALID


def release_all():
    """free the keys verify() keeps resident"""
    _vc.release_all(_resident)


def vk_from_zkey(zkey_bytes):
    """zKey.exportVerificationKey for an FFLONK key (fflonkVk, src/zkey_export_verificationkey.js; header: src/zkey_utils.js
    readHeaderFFlonk), X_2, C0 and w included. Needs no device."""
    z = _vc.ZkeyHeader(zkey_bytes, 10, "fflonk")
    if z.name != "bn128":
        raise ValueError("unsupported curve: FFLONK verification serves bn128 only")
    vk = {"protocol": "fflonk", "curve": z.name, "nPublic": z.n_public, "power": z.power}
    consts = {k: str(z.fr()) for k in KEY_CONSTS}
    vk["k1"], vk["k2"] = consts["k1"], consts["k2"]
    vk["w"] = str(_root(z.cid, z.power, z.r))
    for k in ("w3", "w4", "w8", "wr"):
        vk[k] = consts[k]
    vk["X_2"] = z.g2()
    vk["C0"] = z.g1()
    return vk
