"""Shared by tests/test_ptau_verify_host.py and tests/test_gpu_ptau_verify.py: sections of a powers-of-tau file built from the oracle's points, what
zkmi_ptau_section_check computes restated on the CPU oracle twice (the reference's literal per-power formula, and the library's way: running sums over dyadic
segments and a transform of normal-form scalars), Blake2b-512 in Python with a state that can be written out the way misc.toPartialHash writes it, and the
cases of tests/golden/ptau_verify_golden.json (tools/gen_ptau_golden.js) with their rule and patches applied."""
import json
import os
import struct

import numpy as np

import oracle_lib as orc
import phase2_verify_vectors as V2
from phase2_verify_vectors import CURVES, GOLDEN, Log, curve_record, gold, host_words, join, split  # noqa: F401

INDEX = json.load(open(os.path.join(GOLDEN, "ptau_verify_golden.json")))
CASES = INDEX["cases"]
RANDOM32 = bytes(range(200, 232))


def case_id(c):
    return f"{c['curve']}-{c['label'].replace(' ', '_')}"


def truncate4(raw, n8q):
    """header power 4, the ceremony power as it was, prefixes of sections 2 - 5 and 12 - 15"""
    keep = {2: 31 * 2 * n8q, 3: 16 * 4 * n8q, 4: 16 * 2 * n8q, 5: 16 * 2 * n8q, 12: 63 * 2 * n8q, 13: 31 * 4 * n8q, 14: 31 * 2 * n8q, 15: 31 * 2 * n8q}
    out = []
    for typ, body in split(raw):
        if typ == 1:
            body = body[:4 + n8q] + struct.pack("<I", 4) + body[8 + n8q:]
        out.append((typ, body[:keep[typ]] if typ in keep else body))
    return join(raw, out)


_case_memo = {}


def case_file(c):
    """the fixture of a case with its rule and patches applied, the edits tools/gen_ptau_golden.js made before it asked the reference"""
    k = case_id(c)
    if k not in _case_memo:
        raw, n8q = gold(c["fixture"]), curve_record(c["curve"])["n8q"]
        if c.get("rule") == "truncate4":
            raw = truncate4(raw, n8q)
        for p in c.get("patches", []):
            secs = []
            for typ, body in split(raw):
                if typ == p["section"]:
                    new = bytes.fromhex(p["replace"] if "replace" in p else p["hex"])
                    body = new if "replace" in p else body[:p["offset"]] + new + body[p["offset"] + len(new):]
                secs.append((typ, body))
            raw = join(raw, secs)
        _case_memo[k] = raw
    return _case_memo[k]


def case_lines(c):
    return [tuple(x) for x in c["lines"]]


PAIR_SEED = bytes(range(100, 132))
LADDER_SEED = bytes(range(7, 39))


def words(seed32, n):
    return host_words(struct.unpack(">8I", seed32), 0, n)


def point_size(cv, group):
    return 2 * group * cv["n8q"]


_tau_memo = {}


def tau_points(cv, group, n, inf_at=None):
    """n valid points of the group (the identity checked holds for any points), optionally with infinity at one index"""
    k = (cv["name"], group)
    if k not in _tau_memo:
        _tau_memo[k] = orc.geom_bases(cv["id"], group, 130).tobytes()
    sg = point_size(cv, group)
    b = bytearray(_tau_memo[k][:n * sg])
    if inf_at is not None and inf_at < n:
        b[inf_at * sg:(inf_at + 1) * sg] = bytes(sg)
    return bytes(b)


def lagrange_of(cv, group, tau, top, zero_last):
    """blocks p = 0 .. top of 2^p points: G.ifft of the first 2^p points, the last one of the top block taken as infinity with zero_last"""
    sg, out = point_size(cv, group), []
    for p in range(top + 1):
        n = 1 << p
        pts = tau[:n * sg]
        if p == top and zero_last:
            pts = tau[:(n - 1) * sg] + bytes(sg)
        assert len(pts) == n * sg
        out.append(orc.group_fft(cv["id"], group, np.frombuffer(pts, np.uint8), inverse=True).tobytes() if n > 1 else pts)
    return b"".join(out)


def _aff(cv, group, jac):
    return orc.to_affine(cv["id"], group, jac).tobytes()


def pair_sums(cv, group, tau, n_tau, pair_seed):
    c, sg = cv["id"], point_size(cv, group)
    if n_tau <= 1:
        return bytes(sg), bytes(sg)
    s = words(pair_seed, n_tau - 1).view(np.uint8)
    t = np.frombuffer(tau, np.uint8)
    return (_aff(cv, group, orc.msm(c, group, t[:(n_tau - 1) * sg], s, n_tau - 1, 4)), _aff(cv, group, orc.msm(c, group, t[sg:n_tau * sg], s, n_tau - 1, 4)))


def ladder_sides_literal(cv, group, tau, lagrange, top, zero_last, ladder_seed):
    """[(left, right)] affine, power by power as verifyLagrangeEvaluations writes it: a fresh generator, 2^p words, batchToMontgomery, fft, batchFromMontgomery"""
    c, sg, out = cv["id"], point_size(cv, group), []
    for p in range(top + 1):
        n = 1 << p
        w = words(ladder_seed, n).copy()
        pts = tau[:n * sg]
        if p == top and zero_last:
            w[n - 1] = 0
            pts = tau[:(n - 1) * sg] + bytes(sg)
        left = orc.msm(c, group, np.frombuffer(pts, np.uint8), w.view(np.uint8), n, 4)
        wide = np.zeros((n, 8), np.uint32)
        wide[:, 0] = w
        t = orc.from_mont(c, orc.ntt(c, orc.to_mont(c, wide.view(np.uint8).reshape(-1))))
        right = orc.msm(c, group, np.frombuffer(lagrange[(n - 1) * sg:(2 * n - 1) * sg], np.uint8), t, n)
        out.append((_aff(cv, group, left), _aff(cv, group, right)))
    return out


def ladder_sides_dyadic(cv, group, tau, lagrange, top, zero_last, ladder_seed):
    """the same sides the way the library makes them: the words once, widened once (the tail zeroed when told to), the left sides as running sums over the
    segments [2^(p-1), 2^p), the transform run on the normal-form prefix"""
    c, sg, out = cv["id"], point_size(cv, group), []
    big = 1 << top
    w = words(ladder_seed, big)
    wide = np.zeros((big, 8), np.uint32)
    wide[:, 0] = w
    if zero_last:
        wide[big - 1, 0] = 0
    t_all, acc = np.frombuffer(tau, np.uint8), None
    for p in range(top + 1):
        first, end = (1 << (p - 1)) if p else 0, (1 << p) - (1 if (p == top and zero_last) else 0)
        if end > first:
            seg = _aff(cv, group, orc.msm(c, group, t_all[first * sg:end * sg], w[first:end].view(np.uint8), end - first, 4))
            acc = seg if acc is None else add_affine(cv, group, acc, seg)
        n = 1 << p
        t = orc.ntt(c, wide[:n].reshape(-1).view(np.uint8))
        right = orc.msm(c, group, np.frombuffer(lagrange[(n - 1) * sg:(2 * n - 1) * sg], np.uint8), t, n)
        out.append((acc if acc is not None else bytes(sg), _aff(cv, group, right)))
    return out


def add_affine(cv, group, a, b):
    """a + b for two affine points, by the oracle's MSM with scalars of one"""
    one = np.zeros(8, np.uint8)
    one[0] = one[4] = 1
    return _aff(cv, group, orc.msm(cv["id"], group, np.frombuffer(a + b, np.uint8), one, 2, 4))


class OracleDevice(V2.OracleDevice):
    """powersoftau_verify.Device on the CPU, by the literal formula; same_ratio_batch is the Python pairing's, memoised over the module"""
    sections = {}                                 # (curve, group, the inputs, seeds) -> result: the cases of a fixture share their untouched sections

    def __init__(self):
        super().__init__()
        self.calls = []                           # (group, r1, r2, ladder) per section_check, in order

    def section_check(self, cv, group, tau, n_tau, lagrange, top, zero_last, pair_seed32, ladder_seed32):
        tau = b"".join(tau) if isinstance(tau, (list, tuple)) else bytes(tau)
        tau = tau[:n_tau * point_size(cv, group)]
        lag = None if lagrange is None else (b"".join(lagrange) if isinstance(lagrange, (list, tuple)) else bytes(lagrange))
        k = (cv["name"], group, tau, lag, top, zero_last, pair_seed32, ladder_seed32)
        if k not in self.sections:
            self.sections[k] = self._section_check(cv, group, tau, n_tau, lag, top, zero_last, pair_seed32, ladder_seed32)
        self.calls.append((group,) + self.sections[k][1:])
        return self.sections[k]

    def _section_check(self, cv, group, tau, n_tau, lagrange, top, zero_last, pair_seed32, ladder_seed32):
        u = orc.group_convert(cv["id"], group, "LEMtoU", tau).tobytes() if n_tau else b""
        r1, r2 = pair_sums(cv, group, tau, n_tau, pair_seed32)
        if lagrange is None:
            return u, r1, r2, None
        return u, r1, r2, [a == b for a, b in ladder_sides_literal(cv, group, tau, lagrange, top, zero_last, ladder_seed32)]


# ---- Blake2b-512 with a state that can be written out -------------------------------------------------------------------------------------------------------
_IV = (0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1, 0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179)
_SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3), (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4),
          (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8), (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
          (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10), (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5),
          (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
_M = (1 << 64) - 1


def _rotr(x, n):
    return ((x >> n) | (x << (64 - n))) & _M


def b2b_compress(h, block, t, last):
    """RFC 7693 F: the state after one 128-byte block with counter t"""
    m = struct.unpack("<16Q", block)
    v = list(h) + list(_IV)
    v[12] ^= t & _M
    v[13] ^= t >> 64
    if last:
        v[14] ^= _M

    def g(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & _M; v[d] = _rotr(v[d] ^ v[a], 32); v[c] = (v[c] + v[d]) & _M; v[b] = _rotr(v[b] ^ v[c], 24)
        v[a] = (v[a] + v[b] + y) & _M; v[d] = _rotr(v[d] ^ v[a], 16); v[c] = (v[c] + v[d]) & _M; v[b] = _rotr(v[b] ^ v[c], 63)
    for r in range(12):
        s = _SIGMA[r % 10]
        g(0, 4, 8, 12, m[s[0]], m[s[1]]); g(1, 5, 9, 13, m[s[2]], m[s[3]]); g(2, 6, 10, 14, m[s[4]], m[s[5]]); g(3, 7, 11, 15, m[s[6]], m[s[7]])
        g(0, 5, 10, 15, m[s[8]], m[s[9]]); g(1, 6, 11, 12, m[s[10]], m[s[11]]); g(2, 7, 8, 13, m[s[12]], m[s[13]]); g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[i] ^ v[i] ^ v[8 + i] for i in range(8)]


def b2b_initial():
    return [_IV[0] ^ 0x01010040] + list(_IV[1:])


def b2b_partial(h, buffered, compressed_bytes):
    """misc.toPartialHash of a hasher with state words h, `buffered` (at most 128 bytes) in its block buffer and compressed_bytes behind it"""
    assert len(buffered) <= 128
    w = [0] * 22
    for i in range(8):
        w[2 * i], w[2 * i + 1] = h[i] & 0xffffffff, h[i] >> 32
    w[16], w[17], w[18] = compressed_bytes & 0xffffffff, compressed_bytes >> 32, len(buffered)
    return buffered + bytes(128 - len(buffered)) + struct.pack("<22I", *w)


def b2b_partial_of(prefix, pos):
    """the partial state of a hasher fed `prefix`, of which the last pos bytes still lie in the buffer (as the reference's hasher leaves them: the buffer is
    compressed only when another byte arrives, so pos is 128 after a whole number of blocks and 0 only before the first byte)"""
    assert 0 <= pos <= 128 and (len(prefix) - pos) % 128 == 0 and pos <= len(prefix)
    h, done = b2b_initial(), len(prefix) - pos
    for k in range(0, done, 128):
        h = b2b_compress(h, prefix[k:k + 128], k + 128, False)
    return b2b_partial(h, prefix[done:], done)


def b2b_finish(h, buffered, compressed_bytes, data):
    """the digest of a hasher in the given state after data: the test's own restatement for states no real message reaches (a length above 2^32)"""
    buf, t = bytearray(buffered), compressed_bytes + len(buffered)
    for byte in data:
        if len(buf) == 128:
            h = b2b_compress(h, bytes(buf), t, False)
            buf = bytearray()
        buf.append(byte)
        t += 1
    h = b2b_compress(h, bytes(buf) + bytes(128 - len(buf)), t, True)
    return struct.pack("<8Q", *h)
