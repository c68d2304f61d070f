"""The per-lane routines of the Bellman H basis change (csrc/bellman.cuh), executed ON THE CPU: tools/bellman_hosttest.hip compiles the bodies of
k_bellman_import_load, k_bellman_export_twist and k_bellman_export_store for the host, with the exact offset checks (-DZK29_CHECK) and the worst-case bounds
(-DZK29_BOUNDS) of field29.cuh switched on, and this module holds their result to the CPU oracle one point at a time: the big-endian bytes in and out, the
multiplication on the isomorphic curve of an XYZZ point, edge scalars in their own lanes, infinity at every place of an inversion group, the bit-reversed
store and the slot of the dropped coefficient."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import groth16_setup as gs
from ptau_contribute_vectors import R, bases, edge_scalars, expected_each, normal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "bellman_hosttest")
SRC = os.path.join(ROOT, "tools", "bellman_hosttest.hip")
CSRC = os.path.join(ROOT, "snarkjs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = [("bn128", "bn254"), ("bls12381", "bls12381"), ("bls12381", "bls12381_compact")]
FLAGS = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-DZK29_CHECK", "-DZK29_BOUNDS", "-I" + CSRC]
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("bellman.cuh", "ptau_contribute.cuh", "group_scale.cuh", "msm29.cuh", "field29.cuh", "field.cuh", "msm.cuh", "curve.cuh")]


def request(field, log_n, k1, k2, pts_u):
    return f"{field} {log_n} {normal(k1).hex()} {normal(k2).hex()} {bytes(pts_u).hex()}"


def answer(line, curve, log_n):
    out, last = line.split()
    assert bytes.fromhex(last) == bytes(4 * orc.n8q(orc.CURVE_ID[curve])), "the slot of the dropped coefficient is the point at infinity"
    return bytes.fromhex(out)


def to_u(curve, lem):
    return orc.group_convert(orc.CURVE_ID[curve], 1, "LEMtoU", lem).tobytes()


def rev(j, bits):
    return int(format(j, f"0{bits}b")[::-1], 2)


def expected(curve, log_n, k1, k2, pts_lem):
    """out_j = k2_j k1_rev(j) P_rev(j) for j < n - 1, uncompressed"""
    m, sz = (1 << log_n) - 1, 2 * orc.n8q(orc.CURVE_ID[curve])
    pts_lem = bytes(pts_lem)
    src = [rev(j, log_n) for j in range(m)]
    assert all(s < m for s in src)
    return to_u(curve, expected_each(curve, b"".join(pts_lem[s * sz:(s + 1) * sz] for s in src), [k2[j] * k1[s] % R[curve] for j, s in enumerate(src)]))


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    if not os.path.exists(TOOL) or any(os.path.getmtime(d) > os.path.getmtime(TOOL) for d in DEPS):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([HIPCC] + FLAGS + [SRC, "-o", TOOL])
    p = subprocess.Popen([TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def call(curve, field, log_n, k1, k2, pts_lem, pts_u=None):
        p.stdin.write(request(field, log_n, k1, k2, to_u(curve, pts_lem) if pts_u is None else pts_u) + "\n")
        p.stdin.flush()
        line = p.stdout.readline().strip()
        assert line and not line.startswith("ERR"), (field, line)
        return answer(line, curve, log_n)
    yield call
    p.stdin.close()
    p.wait(timeout=10)


@pytest.mark.parametrize("curve,field", FIELDS)
def test_edge_scalars_through_both_ends(tool, curve, field):
    """31 points, each through the import's load with one edge scalar and through the export's twist and store with another: the twist multiplies an XYZZ point
    whose ZZ is not one, as the butterflies leave it; seven full inversion groups and one of three"""
    ks = edge_scalars(curve)
    r = R[curve]
    assert {0, 1, r - 1, (r - 1) // 2} <= set(ks)
    live = [k for k in ks if k > 3]
    k1 = ([1, r - 1, (r - 1) // 2, 2] + live[0::3])[:31]
    k2 = ([r - 1, 1, 2, (r + 1) // 2] + live[1::3])[:31]
    assert len(k1) == len(k2) == 31
    pts = bases(curve, 31)
    got, want = tool(curve, field, 5, k1, k2, pts), expected(curve, 5, k1, k2, pts)
    sz = len(want) // 31
    for j in range(31):
        assert got[j * sz:(j + 1) * sz] == want[j * sz:(j + 1) * sz], (j, hex(k2[j]), hex(k1[rev(j, 5)]))


@pytest.mark.parametrize("curve,field", FIELDS)
def test_infinity_at_every_place_of_an_inversion_group(tool, curve, field):
    """seven points (a group of four and one of three), three (one short group) and one: a point at infinity going in, a zero scalar at the load (infinity
    through the twist) and a zero scalar at the twist (infinity into the store), at each place; then a whole group of infinities"""
    live = [k for k in edge_scalars(curve) if k > 3][:14]
    for log_n in (3, 2, 1):
        m = (1 << log_n) - 1
        k1, k2 = live[:m], live[m:2 * m]
        for hole in range(m):
            pts = bases(curve, m, infinity=(hole,))
            assert tool(curve, field, log_n, k1, k2, pts) == expected(curve, log_n, k1, k2, pts), (log_n, hole, "point")
            pts = bases(curve, m)
            z1 = [0 if i == hole else k for i, k in enumerate(k1)]
            assert tool(curve, field, log_n, z1, k2, pts) == expected(curve, log_n, z1, k2, pts), (log_n, hole, "load scalar")
            z2 = [0 if i == hole else k for i, k in enumerate(k2)]
            assert tool(curve, field, log_n, k1, z2, pts) == expected(curve, log_n, k1, z2, pts), (log_n, hole, "twist scalar")
    k1, k2 = live[:7], live[7:14]
    z2 = [0, 0, 0, 0] + k2[4:]
    got = tool(curve, field, 3, k1, z2, bases(curve, 7))
    assert got == expected(curve, 3, k1, z2, bases(curve, 7)) and got[:4 * len(got) // 7] == bytes(4 * len(got) // 7)
    assert tool(curve, field, 3, k1, k2, bytes(len(bases(curve, 7)))) == bytes(len(got))


@pytest.mark.parametrize("curve,field", FIELDS)
def test_coordinates_of_p_and_more_are_taken_as_their_residues(tool, curve, field):
    """a parameter file comes from outside: x + p, y + p, and on BN254 the largest multiples of p below 2^256 added, give the points of x and y, with the bound
    of any 256- or 384-bit value carried through the first product (-DZK29_BOUNDS)"""
    q = next(k for k, c in gs.CURVES.items() if c["name"] == curve)
    n8 = orc.n8q(orc.CURVE_ID[curve])
    pts = bases(curve, 7)
    u = to_u(curve, pts)
    top = ((1 << (8 * n8)) - 1) // q - 1                                        # x < q, so x + top q < 2^(8 n8)
    assert top >= 1 and (curve != "bn128" or top == 4)
    adds = [(1, 0), (0, 1), (1, 1), (top, top), (top, 0), (0, top), (top, 1)]
    raised = b"".join((int.from_bytes(u[(2 * i + c) * n8:(2 * i + c + 1) * n8], "big") + adds[i][c] * q).to_bytes(n8, "big") for i in range(7) for c in (0, 1))
    assert raised != u
    live = [k for k in edge_scalars(curve) if k > 3][:14]
    assert tool(curve, field, 3, live[:7], live[7:], pts, raised) == expected(curve, 3, live[:7], live[7:], pts)


def test_lane_routines_under_the_host_sanitizers():
    """the same stand-alone program built with the address and undefined-behaviour sanitizers: seven points a field build, one of them at infinity, among the
    scalars 0, 1, r - 1 and an even one"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    san = TOOL + "_san"
    if not os.path.exists(san) or any(os.path.getmtime(d) > os.path.getmtime(san) for d in DEPS):
        os.makedirs(os.path.dirname(san), exist_ok=True)
        subprocess.check_call([HIPCC] + FLAGS + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", san])
    lines, want = [], []
    for curve, field in FIELDS:
        k1 = [0, 1, R[curve] - 1, 2] + edge_scalars(curve)[-3:]
        k2 = edge_scalars(curve)[-10:-4] + [R[curve] - 1]
        pts = bases(curve, 7, infinity=(5,))
        lines.append(request(field, 3, k1, k2, to_u(curve, pts)))
        want.append(expected(curve, 3, k1, k2, pts).hex())
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [l.split()[0] for l in r.stdout.splitlines()] == want, r.stdout[-400:] + r.stderr[-2000:]
