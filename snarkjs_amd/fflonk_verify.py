"""Batch FFLONK verification on the device: snarkjs.fflonk.verify (src/fflonk_verify.js:28-137) for many proofs against one key. BN254 only:
the reference's fflonk.setup / fflonk.prove do not work on BLS12-381, so a BLS12-381 key is refused.

One verdict per proof with the reference's per-proof semantics (not a probabilistic batch check). Codes, in the order the reference tests
(which differs from PLONK's: the count comes first): -3 a wrong number of public signals ("Number of public signals does not match with vk"),
-2 a commitment or the key's C0 not on the curve ("Proof commitments are not valid"), -1 a public input not in [0, r) ("Public inputs are not
valid."), 0 pairing check failed ("Invalid Proof", logged with warn), 1 valid ("PROOF VERIFIED SUCCESSFULLY"). -4 ("Proof evaluations are not
valid.") is reserved: the reference's test reads already reduced values and cannot fire. The proof's evaluations.inv is not read.
The kernels are csrc/fflonk_verify.hip; there is no CPU path.
"""
import struct

import numpy as np

from . import zkmi
from .groth16_verify import _FQ, _g1, _g2, _int
from .plonk_verify import _fr

VALID, INVALID, BAD_PUBLIC, BAD_POINT, BAD_COUNT = 1, 0, -1, -2, -3
MESSAGES = {VALID: "PROOF VERIFIED SUCCESSFULLY", INVALID: "Invalid Proof", BAD_PUBLIC: "Public inputs are not valid.", BAD_POINT: "Proof commitments are not valid",
            BAD_COUNT: "Number of public signals does not match with vk"}
KEY_CONSTS = ("k1", "k2", "w3", "w4", "w8", "wr")
PROOF_POINTS = ("C1", "C2", "W1", "W2")
PROOF_EVALS = ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3", "a", "b", "c", "z", "zw", "t1w", "t2w")
TRACE_FR = ("beta", "gamma", "xi", "alpha", "y", "r0", "r1", "r2")


def _root(cid, power, r):
    """Fr.w[power] in standard form"""
    w = np.zeros(32, np.uint8)
    zkmi.check(zkmi.lib().zkmi_fr_root(cid, power, zkmi.ptr(w)))
    return int.from_bytes(w.tobytes(), "little") * pow(pow(2, 256, r), -1, r) % r


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
        n = len(proofs)
        if len(public_signals_list) != n:
            raise ValueError("one publicSignals list per proof")
        n_sig = len(public_signals_list[0]) if n else self.n_public
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
            po, ev = pr["polynomials"], pr["evaluations"]
            recs.append(b"".join(_g1(po[k], p, n8) for k in PROOF_POINTS) + b"".join(_fr(ev[k], r) for k in PROOF_EVALS))
        return np.frombuffer(b"".join(recs), np.uint8).copy(), np.frombuffer(b"".join(pubs), np.uint8).copy(), n_sig, pre

    def verify_raw(self, proofs_u8, publics_u8, n_signals=None, n=None):
        """verdict codes (int8 array) of packed records: proofs_u8 n x (12 n8q + 480) bytes (C1 C2 W1 W2 as (x, y, z), fifteen evaluations
        ql qr qm qo qc s1 s2 s3 a b c z zw t1w t2w, standard form, LE), publics_u8 n x n_signals x 32 bytes (LE). Raises ZkmiError "Number of
        public signals does not match with vk" when n_signals is not the key's nPublic."""
        proofs_u8, publics_u8 = zkmi.u8(proofs_u8), zkmi.u8(publics_u8)
        rec = self.record_bytes
        if n is None:
            n = proofs_u8.size // rec
        if n_signals is None:
            n_signals = publics_u8.size // (32 * n) if n else self.n_public
        if proofs_u8.size != n * rec or publics_u8.size != n * n_signals * 32:
            raise ValueError("packed arrays do not match n and n_signals")
        out = np.zeros(max(n, 1), np.int8)
        pub = publics_u8 if publics_u8.size else np.zeros(1, np.uint8)
        zkmi.check(zkmi.lib().zkmi_fflonk_verify_batch(self.handle, zkmi.ptr(proofs_u8), zkmi.ptr(pub), n_signals, n, zkmi.ptr(out)))
        return out[:n]

    def verify_codes(self, public_signals_list, proofs):
        if not proofs:
            return []
        recs, pubs, n_sig, pre = self.pack(public_signals_list, proofs)
        if n_sig != self.n_public:                 # the reference tests the count first: -3 whatever the commitments are
            try:
                self.verify_raw(recs, pubs, n_sig, len(proofs))
            except zkmi.ZkmiError as e:
                if MESSAGES[BAD_COUNT] not in str(e):
                    raise
            else:
                raise RuntimeError("a wrong number of public signals was not refused")
            return [BAD_COUNT] * len(proofs)
        codes = self.verify_raw(recs, pubs, n_sig, len(proofs))
        return [int(c) if pre[i] is None or int(c) == BAD_POINT else pre[i] for i, c in enumerate(codes)]

    def verify_many(self, public_signals_list, proofs):
        return [c == VALID for c in self.verify_codes(public_signals_list, proofs)]

    def trace(self, public_signals, proof):
        """zkmi_fflonk_verify_trace_dev for one proof: dict of beta gamma xi alpha y r0 r1 r2 (ints) and A1, B1 ((x, y) or None)"""
        recs, pubs, n_sig, pre = self.pack([public_signals], [proof])
        if pre[0] is not None:
            raise ValueError("a public signal is outside [0, r)")
        n8 = self.n8
        out = np.zeros(256 + 4 * n8, np.uint8)
        pub = pubs if pubs.size else np.zeros(1, np.uint8)
        zkmi.check(zkmi.lib().zkmi_fflonk_verify_trace_dev(self.handle, zkmi.ptr(recs), zkmi.ptr(pub), n_sig, zkmi.ptr(out)))
        b = out.tobytes()
        res = {k: int.from_bytes(b[32 * i:32 * i + 32], "little") for i, k in enumerate(TRACE_FR)}
        for i, k in enumerate(("A1", "B1")):
            x, y = (int.from_bytes(b[256 + (2 * i + j) * n8:256 + (2 * i + j + 1) * n8], "little") for j in (0, 1))
            res[k] = None if (x, y) == (0, 0) else (x, y)
        return res

    def release(self):
        if self.handle:
            zkmi.check(zkmi.lib().zkmi_fflonk_vk_release(self.handle))
            self.handle = 0


_resident = {}                      # verify(): keys resident per vk content (a key load builds two line tables on one lane)


def verify(vk, public_signals, proof, logger=None):
    """fflonk.verify(vk, publicSignals, proof, logger) with the reference's return value and its verdict messages: "FFLONK VERIFIER STARTED"
    first, then one of MESSAGES ("Invalid Proof" goes to logger.warn, the errors to logger.error), and "FFLONK VERIFIER FINISHED" after a
    pairing verdict (0 / 1) only, as the reference returns early on the input checks. The reference's progress lines (the settings block,
    "> Computing ...", the challenge values) are not reproduced. Where the reference throws — a wrong number of signals without a logger,
    its logger.error is unguarded — this returns False. The key stays resident per vk content (release_all() frees them). One proof alone
    is latency-bound: verify_many is the fast path."""
    import json
    kid = json.dumps(vk, sort_keys=True, default=str)
    key = _resident.get(kid)
    if key is None:
        key = _resident[kid] = VerifyingKey(vk)
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
    for k in _resident.values():
        k.release()
    _resident.clear()


def vk_from_zkey(zkey_bytes):
    """zKey.exportVerificationKey for an FFLONK key (fflonkVk, src/zkey_export_verificationkey.js; header: src/zkey_utils.js
    readHeaderFFlonk), X_2, C0 and w included. Needs no device."""
    data = bytes(zkey_bytes)
    nsec = struct.unpack_from("<I", data, 8)[0]
    off, sec = 12, {}
    for _ in range(nsec):
        t, ln = struct.unpack_from("<IQ", data, off)
        off += 12
        sec[t] = off
        off += ln
    if struct.unpack_from("<I", data, sec[1])[0] != 10:
        raise ValueError("zkey file is not fflonk")
    off = sec[2]
    n8q = struct.unpack_from("<I", data, off)[0]
    q = int.from_bytes(data[off + 4:off + 4 + n8q], "little"); off += 4 + n8q
    n8r = struct.unpack_from("<I", data, off)[0]; off += 4 + n8r
    name = next((k for k, v in _FQ.items() if v[2] == q), None)
    if name != "bn128":
        raise ValueError("unsupported curve: FFLONK verification serves bn128 only")
    cid, _, _, r = _FQ[name]
    _, n_public, domain, _, _ = struct.unpack_from("<IIIII", data, off); off += 20
    power = domain.bit_length() - 1
    rri, rqi = pow(pow(2, 256, r), -1, r), pow(pow(2, 8 * n8q, q), -1, q)

    def fq():
        nonlocal off
        v = int.from_bytes(data[off:off + n8q], "little") * rqi % q
        off += n8q
        return v
    vk = {"protocol": "fflonk", "curve": name, "nPublic": n_public, "power": power}
    consts = {}
    for k in KEY_CONSTS:
        consts[k] = str(int.from_bytes(data[off:off + 32], "little") * rri % r); off += 32
    vk["k1"], vk["k2"] = consts["k1"], consts["k2"]
    vk["w"] = str(_root(cid, power, r))
    for k in ("w3", "w4", "w8", "wr"):
        vk[k] = consts[k]
    c = [fq() for _ in range(4)]
    vk["X_2"] = [["0", "0"], ["1", "0"], ["0", "0"]] if not any(c) else [[str(c[0]), str(c[1])], [str(c[2]), str(c[3])], ["1", "0"]]
    x, y = fq(), fq()
    vk["C0"] = ["0", "1", "0"] if (x, y) == (0, 0) else [str(x), str(y), "1"]           # G1.toObject of the point at infinity
    return vk
