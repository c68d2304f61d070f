"""Scalars and points the tests of the per-lane-scalar G2 multiplication share (csrc/ptau_challenge.cuh): tests/test_ptau_challenge_kernel_host.py runs the lane
routine on the CPU, tests/test_gpu_ptau_challenge.py the kernel, both against the CPU oracle's G2.batchApplyKey. The scalars are those of the G1 kernel
(ptau_contribute_vectors); the points are the (7 * 11^i) G2 table and, because a challenge file comes from outside, points of the twist that are NOT in the
r-torsion: a point of small order makes the loop's prefix pass through infinity, +P and -P again and again."""
import numpy as np

import oracle_lib as orc
from ptau_contribute_vectors import R, edge_scalars, mont, normal, scalars

Q = {"bn128": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
     "bls12381": int("1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab", 16)}
# #E'(Fq2) = r * COFACTOR; SMALL is a prime factor of the cofactor (checked below: SMALL * point = infinity for a point that is not infinity)
COFACTOR = {"bn128": 2 * Q["bn128"] - R["bn128"],
            "bls12381": int("5d543a95414e7f1091d50792876a202cd91de4547085abaa68a205b2e5a7ddfa628f1cb4d9e82ef21537e293a6691ae1616ec6e786f0c70cf1c38e31c7238e5", 16)}
SMALL = {"bn128": 10069, "bls12381": 13}
SMALL_PART = {"bn128": 10069, "bls12381": 169}      # the 13-part of the BLS12-381 twist is Z13 x Z13: dividing 13 alone out of the order kills it


class _Twist:
    """affine arithmetic on y^2 = x^3 + b' over Fq2 = Fq[u] / (u^2 + 1) with Python integers: slow, and independent of the oracle and the kernels"""

    def __init__(self, curve):
        self.p = p = Q[curve]
        self.b = self.mul((3, 0), self.inv((9, 1))) if curve == "bn128" else (4, 4)

    def mul(self, a, b):
        return ((a[0] * b[0] - a[1] * b[1]) % self.p, (a[0] * b[1] + a[1] * b[0]) % self.p)

    def inv(self, a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.p)
        return (a[0] * n % self.p, -a[1] * n % self.p)

    def sub(self, a, b):
        return ((a[0] - b[0]) % self.p, (a[1] - b[1]) % self.p)

    def pow(self, a, e):
        r = (1, 0)
        while e:
            if e & 1:
                r = self.mul(r, a)
            a, e = self.mul(a, a), e >> 1
        return r

    def sqrt(self, a):
        """p = 3 mod 4 on both curves; None when a is no square"""
        p = self.p
        a1 = self.pow(a, (p - 3) // 4)
        x0 = self.mul(a1, a)
        alpha = self.mul(a1, x0)
        if self.mul((alpha[0], -alpha[1] % p), alpha) == (p - 1, 0):
            return None
        x = self.mul((0, 1), x0) if alpha == (p - 1, 0) else self.mul(self.pow(((1 + alpha[0]) % p, alpha[1]), (p - 1) // 2), x0)
        return x if self.mul(x, x) == a else None

    def add(self, P, S):
        if P is None or S is None:
            return S if P is None else P
        if P[0] == S[0]:
            if P[1] != S[1] or P[1] == (0, 0):
                return None
            lam = self.mul(self.mul((3, 0), self.mul(P[0], P[0])), self.inv(self.mul((2, 0), P[1])))
        else:
            lam = self.mul(self.sub(S[1], P[1]), self.inv(self.sub(S[0], P[0])))
        x = self.sub(self.sub(self.mul(lam, lam), P[0]), S[0])
        return (x, self.sub(self.mul(lam, self.sub(P[0], x)), P[1]))

    def times(self, k, P):
        out = None
        while k:
            if k & 1:
                out = self.add(out, P)
            P, k = self.add(P, P), k >> 1
        return out

    def point(self, seed):
        """the first point of the twist with x = seed + j + u"""
        for j in range(64):
            x = ((seed + j) % self.p, 1)
            y2 = self.mul(self.mul(x, x), x)
            y = self.sqrt(((y2[0] + self.b[0]) % self.p, (y2[1] + self.b[1]) % self.p))
            if y is not None:
                return (x, y)
        raise AssertionError("no point found")


def lem(curve, P):
    """an affine point of the twist (None = infinity) as the reference's LEM bytes: Montgomery form, little-endian"""
    n8 = orc.n8q(orc.CURVE_ID[curve])
    if P is None:
        return bytes(4 * n8)
    return b"".join(((v << (8 * n8)) % Q[curve]).to_bytes(n8, "little") for v in (P[0][0], P[0][1], P[1][0], P[1][1]))


_cache = {}


def outside_points(curve):
    """(a point of the twist outside the r-torsion, a point of order SMALL[curve]), both as Python points; computed once"""
    if curve not in _cache:
        tw = _Twist(curve)
        P = tw.point(5)
        assert tw.times(R[curve], P) is not None, "the point is in the r-torsion"
        S = tw.times(COFACTOR[curve] * R[curve] // SMALL_PART[curve], P)
        assert S is not None and tw.times(SMALL[curve], S) is None
        _cache[curve] = (tw, P, S)
    return _cache[curve]


def bases2(curve, n, infinity=()):
    """the (7 * 11^i) G2 table with the point at infinity at the given places"""
    c = orc.CURVE_ID[curve]
    sz = 4 * orc.n8q(c)
    pts = orc.geom_bases(c, 2, n).reshape(n, sz).copy()
    for i in infinity:
        pts[i] = 0
    return pts.reshape(-1)


def expected_each2(curve, pts, ks):
    """out_i = k_i P_i by the oracle's G2.batchApplyKey, one point at a time (first = k_i, inc = 1)"""
    c = orc.CURVE_ID[curve]
    sz = 4 * orc.n8q(c)
    pts = np.frombuffer(bytes(pts), np.uint8)
    one = orc.fr_one(c)
    return b"".join(orc.group_apply_key(c, 2, pts[i * sz:(i + 1) * sz].copy(), mont(curve, k), one).tobytes() for i, k in enumerate(ks))


__all__ = ["R", "Q", "SMALL", "mont", "scalars", "edge_scalars", "normal", "bases2", "expected_each2", "outside_points", "lem"]
