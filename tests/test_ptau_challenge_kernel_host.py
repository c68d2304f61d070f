"""The per-lane routines of the per-lane-scalar G2 multiplication (csrc/ptau_challenge.cuh), executed ON THE CPU: tools/ptau_challenge_hosttest.hip compiles
the body of k_group2_mul_each and, behind it, the body of k_group2_scale_affine for the host, with the exact offset checks (-DZK29_CHECK) and the worst-case
bounds (-DZK29_BOUNDS) of field29.cuh switched on, and this module holds their result to the CPU oracle's G2.batchApplyKey one point at a time: every edge
scalar in its own lane, infinity planted at every place of an inversion group, and points of the twist outside the r-torsion, one of small order."""
import os
import subprocess

import pytest

from ptau_challenge_vectors import R, SMALL, bases2, edge_scalars, expected_each2, lem, normal, outside_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "ptau_challenge_hosttest")
SRC = os.path.join(ROOT, "tools", "ptau_challenge_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = [("bn128", "bn254"), ("bls12381", "bls12381"), ("bls12381", "bls12381_compact")]
HEADERS = ("ptau_challenge.cuh", "ptau_contribute.cuh", "group_scale.cuh", "msm29.cuh", "field29.cuh", "field.cuh", "msm.cuh", "curve.cuh")
FLAGS = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-DZK29_CHECK", "-DZK29_BOUNDS", "-I" + os.path.join(ROOT, "snarkjs_amd", "csrc")]


def _build(out, extra):
    deps = [SRC] + [os.path.join(ROOT, "snarkjs_amd", "csrc", f) for f in HEADERS]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([HIPCC] + FLAGS + extra + [SRC, "-o", out])


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    _build(TOOL, [])
    p = subprocess.Popen([TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def call(field, ks, pts):
        p.stdin.write(f"{field} {normal(ks).hex() or '-'} {bytes(pts).hex() or '-'}\n")
        p.stdin.flush()
        line = p.stdout.readline().strip()
        assert line and not line.startswith("ERR"), (field, line)
        return b"" if line == "-" else bytes.fromhex(line)
    yield call
    p.stdin.close()
    p.wait(timeout=10)


@pytest.mark.parametrize("curve,field", FIELDS)
def test_edge_scalars_one_per_lane(tool, curve, field):
    """every edge scalar on its own point of the (7 * 11^i) G2 table; the last inversion group is short when the count is no multiple of four"""
    ks = edge_scalars(curve)
    assert len(ks) == 116 and {0, 1, R[curve] - 1, R[curve] - 3, (R[curve] - 1) // 2} <= set(ks) and any(k % 2 for k in ks) and any(k % 2 == 0 for k in ks)
    pts = bases2(curve, len(ks))
    got, want = tool(field, ks, pts), expected_each2(curve, pts, ks)
    sz = len(want) // len(ks)
    for i, k in enumerate(ks):
        assert got[i * sz:(i + 1) * sz] == want[i * sz:(i + 1) * sz], hex(k)
    assert tool(field, [], b"") == b""


@pytest.mark.parametrize("curve,field", FIELDS)
def test_scalars_of_r_and_above(tool, curve, field):
    """the digits are read from the bits, so every k below 2^255 gives k P = (k mod r) P for a point of order r: the prefix passes through r P = infinity in
    the middle of the loop (k = 2 r - 1, 2 r, 2 r + 1: the cancelling branch, a doubling of the stale accumulator, then +-P replaces it), at its end and not at all"""
    r = R[curve]
    ks = [k for k in (r, r + 1, r + 2, 2 * r - 1, 2 * r, 2 * r + 1, (1 << 255) - 1, (1 << 255) - 2, 1 << 254, (1 << 254) + 1, (r + (1 << 255)) // 2) if r <= k < 1 << 255]
    assert len(ks) >= 6 and (curve != "bn128" or 2 * r + 1 in ks), "2 r is below 2^255 on BN254 alone"
    pts = bases2(curve, len(ks))
    got, want = tool(field, ks, pts), expected_each2(curve, pts, [k % r for k in ks])
    sz = len(want) // len(ks)
    for i, k in enumerate(ks):
        assert got[i * sz:(i + 1) * sz] == want[i * sz:(i + 1) * sz], hex(k)


@pytest.mark.parametrize("curve,field", FIELDS)
def test_points_outside_the_r_torsion(tool, curve, field):
    """a challenge file comes from outside. A point S of small order m on the twist: the prefix times S is infinity, +S or -S many times in the middle of the
    loop (the cancelling branch, the doubling branch, a doubling of the stale accumulator), and k S = (k mod m) S, held to Python's own arithmetic on the
    twist and to the oracle; and a point of full order outside the r-torsion, where k P is NOT (k mod r) P"""
    tw, P, S = outside_points(curve)
    m, r = SMALL[curve], R[curve]
    ks = list(range(0, 2 * m + 2)) if m < 100 else [0, 1, 2, 3, m - 2, m - 1, m, m + 1, m + 2, 2 * m - 1, 2 * m, 2 * m + 1, 4 * m, 4 * m + 2]
    ks += [k for k in edge_scalars(curve) if k > 1 << 200][:24]
    got = tool(field, ks, lem(curve, S) * len(ks))
    sz = len(got) // len(ks)
    small = {j: lem(curve, tw.times(j, S)) for j in range(m)} if m < 100 else None
    for i, k in enumerate(ks):
        want = small[k % m] if small else lem(curve, tw.times(k % m, S))
        assert got[i * sz:(i + 1) * sz] == want, (k, k % m)
    assert got == expected_each2(curve, lem(curve, S) * len(ks), ks)
    assert any(k % m == 0 for k in ks[3:]) and bytes(sz) in [got[i * sz:(i + 1) * sz] for i in range(3, len(ks))]
    ks = [1, 2, r - 1, r + 1, (1 << 255) - 1, edge_scalars(curve)[-1]]
    got = tool(field, ks, lem(curve, P) * len(ks))
    for i, k in enumerate(ks):
        assert got[i * sz:(i + 1) * sz] == lem(curve, tw.times(k, P)), hex(k)
    assert got[3 * sz:4 * sz] != got[:sz], "(r + 1) P = P: the point is in the r-torsion after all"


def test_lane_routines_under_the_host_sanitizers():
    """the same program built with the address and undefined-behaviour sanitizers: nine points a field build (two inversion groups and a short one), one of them
    at infinity, among the scalars 0, 1, r - 1 and an even one, and one point of small order"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    san = TOOL + "_san"
    _build(san, ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    lines, want = [], []
    for curve, field in FIELDS:
        ks = [0, 1, R[curve] - 1, 2] + edge_scalars(curve)[-5:]
        pts = bytearray(bases2(curve, 9, infinity=(4,)))
        sz = len(pts) // 9
        pts[7 * sz:8 * sz] = lem(curve, outside_points(curve)[2])
        lines.append(f"{field} {normal(ks).hex()} {bytes(pts).hex()}")
        want.append(expected_each2(curve, pts, ks).hex())
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split() == want, r.stdout[-400:] + r.stderr[-2000:]


@pytest.mark.parametrize("curve,field", FIELDS)
def test_results_at_infinity_at_every_place_of_an_inversion_group(tool, curve, field):
    """a point at infinity going in, and k = 0 (infinity coming out of a finite point), at each place of groups of 4, 3, 1 and 5 points"""
    ks = edge_scalars(curve)
    live = [k for k in ks if k > 3][:5]
    for n in (4, 5, 3, 1):
        for hole in range(min(n, 4)):
            pts = bases2(curve, n, infinity=(hole,))
            assert tool(field, live[:n], pts) == expected_each2(curve, pts, live[:n]), (n, hole, "point")
            pts, zeroed = bases2(curve, n), [0 if i == hole else k for i, k in enumerate(live[:n])]
            assert tool(field, zeroed, pts) == expected_each2(curve, pts, zeroed), (n, hole, "scalar")
    pts = bases2(curve, 4, infinity=(0, 1, 2, 3))
    assert tool(field, live[:4], pts) == bytes(len(pts))
    pts = bases2(curve, 4)
    assert tool(field, [0, 0, 0, 0], pts) == bytes(len(pts))
