"""Batch PLONK verification on the device: snarkjs.plonk.verify (src/plonk_verify.js:29-123) for many proofs against one key.

One verdict per proof with the reference's per-proof semantics (not a probabilistic batch check). Codes, in the order the reference tests:
-2 a commitment not on the curve ("Proof commitments are not valid."), -3 a wrong number of public signals ("Invalid number of public
inputs"), -1 a public input not in [0, r) ("Public inputs are not valid."), 0 pairing check failed ("Invalid Proof", logged with warn),
1 valid ("OK!"). -4 ("Proof evaluations are not valid") is reserved: the reference's test reads already reduced values and cannot fire.
The kernels are csrc/plonk_verify.hip; there is no CPU path.
"""
import struct

import numpy as np

from . import zkmi
from .groth16_verify import _FQ, _g1, _g2, _int

VALID, INVALID, BAD_PUBLIC, BAD_POINT, BAD_COUNT = 1, 0, -1, -2, -3
MESSAGES = {VALID: "OK!", INVALID: "Invalid Proof", BAD_PUBLIC: "Public inputs are not valid.", BAD_POINT: "Proof commitments are not valid.",
            BAD_COUNT: "Invalid number of public inputs"}
KEY_POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")
PROOF_POINTS = ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw")
PROOF_EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw")
TRACE_FR = ("beta", "gamma", "alpha", "xi", "v1", "u", "L1", "pi", "r0")


def _fr(v, r):
    """an evaluation as the device reads it: 32 bytes; the device reduces modulo r (Fr.fromObject), the host only what does not fit"""
    v = _int(v)
    return (v if 0 <= v < (1 << 256) else v % r).to_bytes(32, "little")


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
            recs.append(b"".join(_g1(pr[k], p, n8) for k in PROOF_POINTS) + b"".join(_fr(pr[k], r) for k in PROOF_EVALS))
        return np.frombuffer(b"".join(recs), np.uint8).copy(), np.frombuffer(b"".join(pubs), np.uint8).copy(), n_sig, pre

    def verify_raw(self, proofs_u8, publics_u8, n_signals=None, n=None):
        """verdict codes (int8 array) of packed records: proofs_u8 n x (27 n8q + 192) bytes (nine commitments as (x, y, z), six evaluations,
        standard form, LE), publics_u8 n x n_signals x 32 bytes (LE). Raises ZkmiError "Invalid number of public inputs" when n_signals is
        not the key's nPublic."""
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
        zkmi.check(zkmi.lib().zkmi_plonk_verify_batch(self.handle, zkmi.ptr(proofs_u8), zkmi.ptr(pub), n_signals, n, zkmi.ptr(out)))
        return out[:n]

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
            try:
                self.verify_raw(recs, pubs, n_sig, len(proofs))
            except zkmi.ZkmiError as e:
                if MESSAGES[BAD_COUNT] not in str(e):
                    raise
            else:
                raise RuntimeError("a wrong number of public signals was not refused")
            return [BAD_COUNT if all(self._on_curve(pr[k]) for k in PROOF_POINTS) else BAD_POINT for pr in proofs]
        codes = self.verify_raw(recs, pubs, n_sig, len(proofs))
        return [int(c) if pre[i] is None or int(c) == BAD_POINT else pre[i] for i, c in enumerate(codes)]

    def verify_many(self, public_signals_list, proofs):
        return [c == VALID for c in self.verify_codes(public_signals_list, proofs)]

    def trace(self, public_signals, proof):
        """zkmi_plonk_verify_trace_dev for one proof: dict of beta gamma alpha xi v1 u L1 pi r0 (ints) and A1, B1 ((x, y) or None)"""
        recs, pubs, n_sig, pre = self.pack([public_signals], [proof])
        if pre[0] is not None:
            raise ValueError("a public signal is outside [0, r)")
        n8 = self.n8
        out = np.zeros(288 + 4 * n8, np.uint8)
        pub = pubs if pubs.size else np.zeros(1, np.uint8)
        zkmi.check(zkmi.lib().zkmi_plonk_verify_trace_dev(self.handle, zkmi.ptr(recs), zkmi.ptr(pub), n_sig, zkmi.ptr(out)))
        b = out.tobytes()
        res = {k: int.from_bytes(b[32 * i:32 * i + 32], "little") for i, k in enumerate(TRACE_FR)}
        for i, k in enumerate(("A1", "B1")):
            x, y = (int.from_bytes(b[288 + (2 * i + j) * n8:288 + (2 * i + j + 1) * n8], "little") for j in (0, 1))
            res[k] = None if (x, y) == (0, 0) else (x, y)
        return res

    def release(self):
        if self.handle:
            zkmi.check(zkmi.lib().zkmi_plonk_vk_release(self.handle))
            self.handle = 0


_resident = {}                      # verify(): keys resident per vk content (a key load builds two line tables on one lane)


def verify(vk, public_signals, proof, logger=None):
    """plonk.verify(vk, publicSignals, proof, logger) with the reference's return value and logger messages ("PLONK VERIFIER STARTED" first;
    "Invalid Proof" goes to logger.warn). Where the reference throws — a bad commitment without a logger — this returns False. The key stays
    resident per vk content (release_all() frees them). One proof alone is latency-bound: verify_many is the fast path."""
    import json
    kid = json.dumps(vk, sort_keys=True, default=str)
    key = _resident.get(kid)
    if key is None:
        key = _resident[kid] = VerifyingKey(vk)
    if logger is not None:
        logger.info("PLONK VERIFIER STARTED")
    code = key.verify_codes([public_signals], [proof])[0]
    if logger is not None:
        (logger.info if code == VALID else logger.warn if code == INVALID else logger.error)(MESSAGES[code])
    return code == VALID


def release_all():
    """free the keys verify() keeps resident"""
    for k in _resident.values():
        k.release()
    _resident.clear()


def vk_from_zkey(zkey_bytes):
    """zKey.exportVerificationKey for a PLONK key (plonkVk, src/zkey_export_verificationkey.js:92-121), X_2 and w included. Needs no device."""
    data = bytes(zkey_bytes)
    nsec = struct.unpack_from("<I", data, 8)[0]
    off, sec = 12, {}
    for _ in range(nsec):
        t, ln = struct.unpack_from("<IQ", data, off)
        off += 12
        sec[t] = off
        off += ln
    if struct.unpack_from("<I", data, sec[1])[0] != 2:
        raise ValueError("zkey file is not plonk")
    off = sec[2]
    n8q = struct.unpack_from("<I", data, off)[0]
    q = int.from_bytes(data[off + 4:off + 4 + n8q], "little"); off += 4 + n8q
    n8r = struct.unpack_from("<I", data, off)[0]; off += 4 + n8r
    name = next((k for k, v in _FQ.items() if v[2] == q), None)
    if name is None:
        raise ValueError("unsupported curve")
    cid, _, _, r = _FQ[name]
    _, n_public, domain, _, _ = struct.unpack_from("<IIIII", data, off); off += 20
    power = domain.bit_length() - 1
    rri, rqi = pow(pow(2, 256, r), -1, r), pow(pow(2, 8 * n8q, q), -1, q)

    def fq():
        nonlocal off
        v = int.from_bytes(data[off:off + n8q], "little") * rqi % q
        off += n8q
        return v
    vk = {"protocol": "plonk", "curve": name, "nPublic": n_public, "power": power}
    for k in ("k1", "k2"):
        vk[k] = str(int.from_bytes(data[off:off + 32], "little") * rri % r); off += 32
    for k in KEY_POINTS:
        x, y = fq(), fq()
        vk[k] = ["0", "1", "0"] if (x, y) == (0, 0) else [str(x), str(y), "1"]           # G1.toObject of the point at infinity
    c = [fq() for _ in range(4)]
    vk["X_2"] = [["0", "0"], ["1", "0"], ["0", "0"]] if not any(c) else [[str(c[0]), str(c[1])], [str(c[2]), str(c[3])], ["1", "0"]]
    w = np.zeros(32, np.uint8)
    zkmi.check(zkmi.lib().zkmi_fr_root(cid, power, zkmi.ptr(w)))
    vk["w"] = str(int.from_bytes(w.tobytes(), "little") * rri % r)
    return vk
