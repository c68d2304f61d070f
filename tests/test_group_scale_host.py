"""The per-lane routines of the one-scalar point scaling (csrc/group_scale.cuh), executed ON THE CPU: tools/group_scale_hosttest.hip compiles the bodies of
k_group_scale and k_group_scale_affine for the host, with the exact offset checks (-DZK29_CHECK) and the worst-case bounds (-DZK29_BOUNDS) of field29.cuh
switched on, and this module holds their result to the CPU oracle's G1.batchApplyKey(first = k, inc = 1): the edge scalars, raw digit streams that drive the
accumulator through infinity and through the equal-points branch of the mixed addition, and infinity planted at every place of an inversion group."""
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "group_scale_hosttest")
SRC = os.path.join(ROOT, "tools", "group_scale_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
R = {"bn128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12381": 52435875175126190479447740508185965837690552500527637822603658699938581184513}
FIELDS = [("bn128", "bn254"), ("bls12381", "bls12381"), ("bls12381", "bls12381_compact")]


def scalars(curve):
    """the scalars every test of the kernel uses (tests/test_gpu_group_scale.py imports them)"""
    r = R[curve]
    ones = (1 << r.bit_length()) - 1
    while ones >= r:
        ones >>= 1
    rnd = random.Random(20261019)
    fixed = [0, 1, 2, 3, r - 1, r - 2, (r + 1) // 2, 1 << (253 if curve == "bn128" else 254), int("55" * 32, 16) % r, int("aa" * 32, 16) % r, ones]
    return fixed + [rnd.randrange(r) for _ in range(8)]


def naf(k):
    """non-adjacent form of k, most significant digit first, as the characters the tool reads"""
    out = []
    while k:
        d = 0
        if k & 1:
            d = 2 - (k & 3)
            k -= d
        out.append("+-"[d < 0] if d else "0")
        k >>= 1
    return "".join(reversed(out))


def stream_value(digits):
    v = 0
    for ch in digits:
        v = 2 * v + {"+": 1, "-": -1, "0": 0}[ch]
    return v


def mont(curve, k):
    return np.frombuffer(((k % R[curve] << 256) % R[curve]).to_bytes(32, "little"), np.uint8)


def bases(curve, n, infinity=()):
    """the (7 * 11^i) G table with the point at infinity at the given places"""
    c = orc.CURVE_ID[curve]
    sz = 2 * orc.n8q(c)
    pts = orc.geom_bases(c, 1, n).reshape(n, sz).copy()
    for i in infinity:
        pts[i] = 0
    return pts.reshape(-1)


def expected(curve, pts, k):
    c = orc.CURVE_ID[curve]
    return orc.group_apply_key(c, 1, pts, mont(curve, k), orc.fr_one(c)).tobytes()


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(ROOT, "snarkjs_amd", "csrc", f) for f in ("group_scale.cuh", "msm29.cuh", "field29.cuh", "field.cuh", "msm.cuh", "curve.cuh")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(d) > os.path.getmtime(TOOL) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-DZK29_CHECK", "-DZK29_BOUNDS", "-I" + os.path.join(ROOT, "snarkjs_amd", "csrc"),
                               SRC, "-o", TOOL])
    p = subprocess.Popen([TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def call(field, kind, arg, pts):
        p.stdin.write(f"{field} {kind} {arg} {bytes(pts).hex()}\n")
        p.stdin.flush()
        line = p.stdout.readline().strip()
        assert line and not line.startswith("ERR"), (field, kind, arg, line)
        return b"" if line == "-" else bytes.fromhex(line)
    yield call
    p.stdin.close()
    p.wait(timeout=10)


@pytest.mark.parametrize("curve,field", FIELDS)
def test_edge_scalars_against_the_oracle(tool, curve, field):
    """n = 9: two whole inversion groups and a last one of a single point; infinity at the first and the last index and across the whole second group"""
    pts = bases(curve, 9, infinity=(0, 4, 5, 6, 7, 8))
    pts2 = bases(curve, 6)
    for k in scalars(curve):
        assert tool(field, "k", "%064x" % k, pts) == expected(curve, pts, k), hex(k)
    for k in scalars(curve)[:11]:
        assert tool(field, "k", "%064x" % k, pts2) == expected(curve, pts2, k), hex(k)
    assert tool(field, "k", "%064x" % 5, b"") == b""


@pytest.mark.parametrize("curve,field", FIELDS)
def test_infinity_at_every_place_of_an_inversion_group(tool, curve, field):
    k = scalars(curve)[-1]
    for n in (4, 5, 3, 1):
        for hole in range(min(n, 4)):
            pts = bases(curve, n, infinity=(hole,))
            assert tool(field, "k", "%064x" % k, pts) == expected(curve, pts, k), (n, hole)
    pts = bases(curve, 4, infinity=(0, 1, 2, 3))
    assert tool(field, "k", "%064x" % k, pts) == bytes(len(pts))


@pytest.mark.parametrize("curve,field", FIELDS)
def test_digit_streams_through_infinity_and_the_equal_points_branch(tool, curve, field):
    """Streams no scalar below r recodes to: the accumulator reaches r P = infinity on an ADDITION (acc = -P: the mixed addition's cancellation branch), goes on
    from there, and meets acc = P at an addition (the doubling branch)"""
    r = R[curve]
    pts = bases(curve, 5, infinity=(2,))
    streams = [naf(r),                                  # ends at infinity
               naf((r - 1) // 2) + "+",                 # 2 (r - 1) / 2 + 1 = r: acc = -P when P is added
               naf((r + 1) // 2) + "+",                 # r + 2: acc = 2 ((r + 1) / 2) P = P when P is added -> 2 P by the doubling branch
               naf((r + 1) // 2) + "-",                 # r: acc = P when -P is added
               "+-", "+0-", "++", "+++", "0", "00+", "-"]
    if curve == "bn128":                                # r has 254 bits there: room for one more digit within the 256 the kernel takes
        streams += [naf(r) + "+"]                       # through infinity and on: (2 r + 1) P
    for d in streams:
        assert len(d) <= 256
        assert tool(field, "d", d, pts) == expected(curve, pts, stream_value(d)), d
