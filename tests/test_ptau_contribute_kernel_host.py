"""The per-lane routines of the per-lane-scalar G1 multiplication (csrc/ptau_contribute.cuh), executed ON THE CPU: tools/ptau_contribute_hosttest.hip compiles
the body of k_group_mul_each and, behind it, the body of k_group_scale_affine for the host, with the exact offset checks (-DZK29_CHECK) and the worst-case
bounds (-DZK29_BOUNDS) of field29.cuh switched on, and this module holds their result to the CPU oracle's G1.batchApplyKey one point at a time: every edge
scalar in its own lane, infinity planted at every place of an inversion group."""
import os
import subprocess

import pytest

from ptau_contribute_vectors import R, bases, edge_scalars, expected_each, normal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "ptau_contribute_hosttest")
SRC = os.path.join(ROOT, "tools", "ptau_contribute_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = [("bn128", "bn254"), ("bls12381", "bls12381"), ("bls12381", "bls12381_compact")]


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(ROOT, "snarkjs_amd", "csrc", f) for f in ("ptau_contribute.cuh", "group_scale.cuh", "msm29.cuh", "field29.cuh", "field.cuh", "msm.cuh", "curve.cuh")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(d) > os.path.getmtime(TOOL) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-DZK29_CHECK", "-DZK29_BOUNDS", "-I" + os.path.join(ROOT, "snarkjs_amd", "csrc"),
                               SRC, "-o", TOOL])
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
    """every edge scalar on its own point of the (7 * 11^i) G table; the last inversion group is short when the count is no multiple of four"""
    ks = edge_scalars(curve)
    assert {0, 1, R[curve] - 1, R[curve] - 3, (R[curve] - 1) // 2} <= set(ks) and any(k % 2 for k in ks) and any(k % 2 == 0 for k in ks)
    pts = bases(curve, len(ks))
    got, want = tool(field, ks, pts), expected_each(curve, pts, ks)
    sz = len(want) // len(ks)
    for i, k in enumerate(ks):
        assert got[i * sz:(i + 1) * sz] == want[i * sz:(i + 1) * sz], hex(k)
    assert tool(field, [], b"") == b""


@pytest.mark.parametrize("curve,field", FIELDS)
def test_scalars_of_r_and_above(tool, curve, field):
    """the digits are read from the bits, so every k below 2^255 gives k P = (k mod r) P: the prefix passes through r P = infinity in the middle of the loop
    (k = 2 r - 1, 2 r, 2 r + 1: the cancelling branch, a doubling of the stale accumulator, then +-P replaces it), at its end (k = r, r - 1 + 1) and not at all"""
    r = R[curve]
    ks = [k for k in (r, r + 1, r + 2, 2 * r - 1, 2 * r, 2 * r + 1, (1 << 255) - 1, (1 << 255) - 2, 1 << 254, (1 << 254) + 1, (r + (1 << 255)) // 2) if r <= k < 1 << 255]
    assert len(ks) >= 6 and (curve != "bn128" or 2 * r + 1 in ks), "2 r is below 2^255 on BN254 alone"
    pts = bases(curve, len(ks))
    got, want = tool(field, ks, pts), expected_each(curve, pts, [k % r for k in ks])
    sz = len(want) // len(ks)
    for i, k in enumerate(ks):
        assert got[i * sz:(i + 1) * sz] == want[i * sz:(i + 1) * sz], hex(k)


def test_lane_routines_under_the_host_sanitizers():
    """the same program built with the address and undefined-behaviour sanitizers: nine points a field build (two inversion groups and a short one), one of them
    at infinity, among the scalars 0, 1, r - 1 and an even one"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    san = TOOL + "_san"
    if not os.path.exists(san) or os.path.getmtime(SRC) > os.path.getmtime(san) or os.path.getmtime(os.path.join(ROOT, "snarkjs_amd", "csrc", "ptau_contribute.cuh")) > os.path.getmtime(san):
        os.makedirs(os.path.dirname(san), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-DZK29_CHECK", "-DZK29_BOUNDS", "-Xarch_host", "-fsanitize=address,undefined",
                               "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "snarkjs_amd", "csrc"), SRC, "-o", san])
    lines, want = [], []
    for curve, field in FIELDS:
        ks = [0, 1, R[curve] - 1, 2] + edge_scalars(curve)[-5:]
        pts = bases(curve, 9, infinity=(4,))
        lines.append(f"{field} {normal(ks).hex()} {bytes(pts).hex()}")
        want.append(expected_each(curve, pts, ks).hex())
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == want, r.stdout[-400:] + r.stderr[-2000:]


@pytest.mark.parametrize("curve,field", FIELDS)
def test_results_at_infinity_at_every_place_of_an_inversion_group(tool, curve, field):
    """a point at infinity going in, and k = 0 (infinity coming out of a finite point), at each place of groups of 4, 3, 1 and 5 points"""
    ks = edge_scalars(curve)
    live = [k for k in ks if k > 3][:5]
    for n in (4, 5, 3, 1):
        for hole in range(min(n, 4)):
            pts = bases(curve, n, infinity=(hole,))
            assert tool(field, live[:n], pts) == expected_each(curve, pts, live[:n]), (n, hole, "point")
            pts, zeroed = bases(curve, n), [0 if i == hole else k for i, k in enumerate(live[:n])]
            assert tool(field, zeroed, pts) == expected_each(curve, pts, zeroed), (n, hole, "scalar")
    pts = bases(curve, 4, infinity=(0, 1, 2, 3))
    assert tool(field, live[:4], pts) == bytes(len(pts))
    pts = bases(curve, 4)
    assert tool(field, [0, 0, 0, 0], pts) == bytes(len(pts))
