"""What the three batch verifiers (groth16_verify, plonk_verify, fflonk_verify) share on the host: field-element and point encoding, the
public-signal half of a packed batch, the size checks around a *_verify_batch call, the trace decoder, the aggregated check
(verify_all / verify_all_raw / verify_many_fast), the cache behind verify() /
release_all() (each module passes its own dict) and the zkey header reader of the two vk_from_zkey. Needs no device except root()."""
import json
import os
import struct

import numpy as np

from . import zkmi

BAD_PUBLIC = -1
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


def _fr(v, r):
    """an evaluation as the device reads it: 32 bytes; the device reduces modulo r (Fr.fromObject), the host only what does not fit"""
    v = _int(v)
    return (v if 0 <= v < (1 << 256) else v % r).to_bytes(32, "little")


def _root(cid, power, r):
    """Fr.w[power] in standard form"""
    w = np.zeros(32, np.uint8)
    zkmi.check(zkmi.lib().zkmi_fr_root(cid, power, zkmi.ptr(w)))
    return int.from_bytes(w.tobytes(), "little") * pow(pow(2, 256, r), -1, r) % r


def pack(key, public_signals_list, proofs, record, n_sig_empty, fewer=False):
    """(proofs_u8, publics_u8, n_signals, pre) of a batch: record(proof) gives a proof's packed bytes; pre[i] = -1 where a public is outside
    [0, r) (checked here, since such values may have no 32-byte form), else None. Every proof of a batch carries the same number of signals
    (n_sig_empty for an empty batch); with fewer (Groth16) any number up to the key's nPublic is packed and more raise, without it the number is
    packed as given and a wrong one is left to the device call to refuse. Reads only r and n_public of key."""
    n = len(proofs)
    if len(public_signals_list) != n:
        raise ValueError("one publicSignals list per proof")
    n_sig = len(public_signals_list[0]) if n else n_sig_empty
    if fewer and n_sig > key.n_public:
        raise ValueError(f"{n_sig} public signals for a key with nPublic = {key.n_public}")
    recs, pubs, pre = [], [], [None] * n
    for i, (sig, pr) in enumerate(zip(public_signals_list, proofs)):
        if len(sig) != n_sig:
            raise ValueError("every proof of a batch needs the same number of public signals")
        vals = [_int(s) for s in sig]
        if any(v < 0 or v >= key.r for v in vals):
            pre[i] = BAD_PUBLIC
            vals = [0] * n_sig
        pubs.append(b"".join(v.to_bytes(32, "little") for v in vals))
        recs.append(record(pr))
    return np.frombuffer(b"".join(recs), np.uint8).copy(), np.frombuffer(b"".join(pubs), np.uint8).copy(), n_sig, pre


def verify_raw(key, verify_batch, rec, proofs_u8, publics_u8, n_signals, n, n_sig_empty):
    """verdict codes (int8 array) of packed records of rec bytes each, by the library's verify_batch of key's protocol"""
    proofs_u8, publics_u8 = zkmi.u8(proofs_u8), zkmi.u8(publics_u8)
    if n is None:
        n = proofs_u8.size // rec
    if n_signals is None:
        n_signals = publics_u8.size // (32 * n) if n else n_sig_empty
    if proofs_u8.size != n * rec or publics_u8.size != n * n_signals * 32:
        raise ValueError("packed arrays do not match n and n_signals")
    out = np.zeros(max(n, 1), np.int8)
    pub = publics_u8 if publics_u8.size else np.zeros(1, np.uint8)
    zkmi.check(verify_batch(key.handle, zkmi.ptr(proofs_u8), zkmi.ptr(pub), n_signals, n, zkmi.ptr(out)))
    return out[:n]


def new_seed(seed):
    """the 32 seed bytes of an aggregated check: drawn from the OS unless given (reproducibility; whoever made the proofs must not know it)"""
    if seed is None:
        return os.urandom(32)
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("the seed of an aggregated check is 32 bytes")
    return seed


def verify_all_raw(key, verify_aggregate, rec, proofs_u8, publics_u8, n_signals, n, n_sig_empty, seed, sums=None):
    """(ok, codes) of packed records by the library's *_verify_aggregate of key's protocol (or, with sums = a uint8 array of the size its
    *_aggregate_trace_dev reports — 4 n8 bytes for the KZG protocols, 16 n8 + 24 for Groth16 — that call): ONE pairing check for the batch;
    codes[i] is proof i's input-check code or 1 (entered the sums)"""
    proofs_u8, publics_u8 = zkmi.u8(proofs_u8), zkmi.u8(publics_u8)
    if n is None:
        n = proofs_u8.size // rec
    if n_signals is None:
        n_signals = publics_u8.size // (32 * n) if n else n_sig_empty
    if proofs_u8.size != n * rec or publics_u8.size != n * n_signals * 32:
        raise ValueError("packed arrays do not match n and n_signals")
    sd = np.frombuffer(new_seed(seed), np.uint8).copy()
    out = np.zeros(max(n, 1), np.int8)
    pub = publics_u8 if publics_u8.size else np.zeros(1, np.uint8)
    prf = proofs_u8 if proofs_u8.size else np.zeros(1, np.uint8)
    ok = zkmi.C.c_int(0)
    extra = () if sums is None else (zkmi.ptr(sums),)
    zkmi.check(verify_aggregate(key.handle, zkmi.ptr(prf), zkmi.ptr(pub), n_signals, n, zkmi.ptr(sd), zkmi.ptr(out), zkmi.C.byref(ok), *extra))
    return bool(ok.value), out[:n]


def verify_all(key, public_signals_list, proofs, seed, count_message):
    """are all of these valid? False where a public signal is out of range (caught while packing) or the number of signals is wrong (refused by
    the device call as a whole, as in verify_codes; count_message None: the protocol accepts fewer signals and pack() raises on more — Groth16)"""
    recs, pubs, n_sig, pre = key.pack(public_signals_list, proofs)
    if count_message is not None and proofs and n_sig != key.n_public:
        refused_count(key, recs, pubs, n_sig, len(proofs), count_message)
        return False
    if any(c is not None for c in pre):
        return False
    return key.verify_all_raw(recs, pubs, n_sig, len(proofs), seed)[0]


def verify_many_fast(key, public_signals_list, proofs, seed, count_message):
    """verify_many for mostly honest traffic: all-valid by the aggregated check, else the per-proof answer that names the culprits"""
    if verify_all(key, public_signals_list, proofs, seed, count_message):
        return [True] * len(proofs)
    return key.verify_many(public_signals_list, proofs)


def aggregate_trace(key, aggregate_trace_dev, public_signals_list, proofs, seed, more_bytes=0):
    """*_aggregate_trace_dev: (ok, codes, S_P, S_Q) with a sum as (x, y) or None for the point at infinity; with more_bytes, the bytes the
    protocol's report holds after its two sums come fifth"""
    recs, pubs, n_sig, pre = key.pack(public_signals_list, proofs)
    if any(c is not None for c in pre):
        raise ValueError("a public signal is outside [0, r)")
    n8 = key.n8
    sums = np.zeros(4 * n8 + more_bytes, np.uint8)
    ok, codes = verify_all_raw(key, aggregate_trace_dev, key.record_bytes, recs, pubs, n_sig, len(proofs), n_sig, seed, sums)
    v = [int.from_bytes(sums[i * n8:(i + 1) * n8].tobytes(), "little") for i in range(4)]
    res = (ok, codes, (None if (v[0], v[1]) == (0, 0) else (v[0], v[1])), (None if (v[2], v[3]) == (0, 0) else (v[2], v[3])))
    return res + (sums[4 * n8:].tobytes(),) if more_bytes else res


def refused_count(key, recs, pubs, n_sig, n, message):
    """a batch with a wrong number of public signals goes to the device call, which has to refuse it as a whole with message"""
    try:
        key.verify_raw(recs, pubs, n_sig, n)
    except zkmi.ZkmiError as e:
        if message not in str(e):
            raise
    else:
        raise RuntimeError("a wrong number of public signals was not refused")


def trace(key, verify_trace_dev, names, public_signals, proof):
    """*_verify_trace_dev for one proof: dict of the Fr values called names (ints) and A1, B1 ((x, y) or None)"""
    recs, pubs, n_sig, pre = key.pack([public_signals], [proof])
    if pre[0] is not None:
        raise ValueError("a public signal is outside [0, r)")
    n8, at = key.n8, 32 * len(names)
    out = np.zeros(at + 4 * n8, np.uint8)
    pub = pubs if pubs.size else np.zeros(1, np.uint8)
    zkmi.check(verify_trace_dev(key.handle, zkmi.ptr(recs), zkmi.ptr(pub), n_sig, zkmi.ptr(out)))
    b = out.tobytes()
    res = {k: int.from_bytes(b[32 * i:32 * i + 32], "little") for i, k in enumerate(names)}
    for i, k in enumerate(("A1", "B1")):
        x, y = (int.from_bytes(b[at + (2 * i + j) * n8:at + (2 * i + j + 1) * n8], "little") for j in (0, 1))
        res[k] = None if (x, y) == (0, 0) else (x, y)
    return res


def release(key, vk_release):
    if key.handle:
        zkmi.check(vk_release(key.handle))
        key.handle = 0


def resident(cache, cls, vk):
    """the key of cache (a module's own dict) for this vk content, loaded on first use"""
    kid = json.dumps(vk, sort_keys=True, default=str)
    key = cache.get(kid)
    if key is None:
        key = cache[kid] = cls(vk)
    return key


def release_all(cache):
    for k in cache.values():
        k.release()
    cache.clear()


class ZkeyHeader:
    """The section table and the header (section 2) of a PLONK or FFLONK zkey up to its five size words: name (None for an unknown curve), cid,
    r, n_public, power; fr() fq() g1() g2() then read on from there, Montgomery form to standard form, points as G1 / G2.toObject gives them."""

    def __init__(self, zkey_bytes, protocol_id, protocol):
        self.data = data = bytes(zkey_bytes)
        nsec = struct.unpack_from("<I", data, 8)[0]
        off, sec = 12, {}
        for _ in range(nsec):
            t, ln = struct.unpack_from("<IQ", data, off)
            off += 12
            sec[t] = off
            off += ln
        if struct.unpack_from("<I", data, sec[1])[0] != protocol_id:
            raise ValueError(f"zkey file is not {protocol}")
        off = sec[2]
        self.n8q = n8q = struct.unpack_from("<I", data, off)[0]
        self.q = q = int.from_bytes(data[off + 4:off + 4 + n8q], "little"); off += 4 + n8q
        n8r = struct.unpack_from("<I", data, off)[0]; off += 4 + n8r
        self.name = next((k for k, v in _FQ.items() if v[2] == q), None)
        self.cid, _, _, self.r = _FQ[self.name] if self.name else (None,) * 4
        _, self.n_public, domain, _, _ = struct.unpack_from("<IIIII", data, off)
        self.off = off + 20
        self.power = domain.bit_length() - 1
        self.rqi = pow(pow(2, 8 * n8q, q), -1, q) if self.name else None

    def fr(self):
        v = int.from_bytes(self.data[self.off:self.off + 32], "little") * pow(pow(2, 256, self.r), -1, self.r) % self.r
        self.off += 32
        return v

    def fq(self):
        v = int.from_bytes(self.data[self.off:self.off + self.n8q], "little") * self.rqi % self.q
        self.off += self.n8q
        return v

    def g1(self):
        x, y = self.fq(), self.fq()
        return ["0", "1", "0"] if (x, y) == (0, 0) else [str(x), str(y), "1"]              # G1.toObject of the point at infinity

    def g2(self):
        c = [self.fq() for _ in range(4)]
        return [["0", "0"], ["1", "0"], ["0", "0"]] if not any(c) else [[str(c[0]), str(c[1])], [str(c[2]), str(c[3])], ["1", "0"]]
