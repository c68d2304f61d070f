"""Scalars and points the tests of the per-lane-scalar G1 multiplication share (csrc/ptau_contribute.cuh): tests/test_ptau_contribute_kernel_host.py runs the
lane routine on the CPU, tests/test_gpu_ptau_contribute.py the kernel, both against the CPU oracle's G1.batchApplyKey."""
import numpy as np

import oracle_lib as orc
from test_group_scale_host import R, bases, mont, scalars


def edge_scalars(curve):
    """scalars(curve) of the one-scalar kernel's tests, plus what the all-odd signed form can trip over: the top of the range (k + 1 = r for k = r - 1, the one
    scalar whose last addition cancels), all-ones below 2^254, the halves of r (2 acc = -+P is next to them), powers of two and their neighbours at the word
    edges of the scalar (a digit is bit j + 1: the bit read moves to the next word there), and an even and an odd neighbour of each"""
    r = R[curve]
    core = list(scalars(curve)) + [r - 3, ((1 << 254) - 1) % r, (r - 1) // 2, (r + 1) // 2 - 1, (r + 1) // 2 + 1]
    for j in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 223, 224, 225, 252, 253, 254):
        core += [((1 << j) - 1) % r, ((1 << j) + 1) % r]
    out = []
    for k in core:
        for v in (k, k - 1, k + 1):
            if 0 <= v < r and v not in out:
                out.append(v)
    return out


def normal(ks):
    """scalars as the kernel reads them: 32 bytes each, little-endian, normal form"""
    return b"".join(int(k).to_bytes(32, "little") for k in ks)


def expected_each(curve, pts, ks):
    """out_i = k_i P_i by the oracle's batchApplyKey, one point at a time (first = k_i, inc = 1)"""
    c = orc.CURVE_ID[curve]
    sz = 2 * orc.n8q(c)
    pts = np.frombuffer(bytes(pts), np.uint8)
    one = orc.fr_one(c)
    return b"".join(orc.group_apply_key(c, 1, pts[i * sz:(i + 1) * sz].copy(), mont(curve, k), one).tobytes() for i, k in enumerate(ks))


__all__ = ["R", "bases", "mont", "scalars", "edge_scalars", "normal", "expected_each"]
