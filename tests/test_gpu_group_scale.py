"""One scalar times many G1 points on the device (csrc/group_scale.cuh through zkmi_group_scale_dev / zkmi_group_scale) against the CPU oracle's
G1.batchApplyKey(first = k, inc = 1) and against the library's general kernel (zkmi_group_batch_apply_key_dev(first = k, inc = 1)), both curves: sizes around
the block and the inversion group, the point at infinity at every place of an inversion group, across a whole group and at both ends, the edge scalars, in
place, the paged host form, and group 2."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as orc
from snarkjs_amd import zkmi
from test_group_scale_host import R, mont, scalars

pytestmark = pytest.mark.gpu
CURVES = ["bn128", "bls12381"]
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1000]


def planted(n):
    """where the point at infinity goes: first and last index, one whole inversion group (4 .. 7), and one place each of the four groups after it"""
    if n < 3:
        return ()
    s = {0, n - 1} | {i for i in range(4, 8) if i < n} | {4 * (2 + j) + j for j in range(4) if 4 * (2 + j) + j < n}
    return tuple(sorted(s))


_bases = {}


def bases(curve, n, holes=True):
    key = (curve, n, holes)
    if key not in _bases:
        c = orc.CURVE_ID[curve]
        pts = orc.geom_bases(c, 1, n).reshape(n, -1).copy() if n else np.zeros((0, 2 * orc.n8q(c)), np.uint8)
        for i in (planted(n) if holes else ()):
            pts[i] = 0
        _bases[key] = pts.reshape(-1)
    return _bases[key]


def oracle(curve, pts, k, group=1):
    c = orc.CURVE_ID[curve]
    return orc.group_apply_key(c, group, pts, mont(curve, k), orc.fr_one(c)).tobytes() if pts.size else b""


def device(curve, pts, k, group=1, in_place=False, general=False):
    zkmi.init()
    c, L = orc.CURVE_ID[curve], zkmi.lib()
    n = pts.size // (2 * group * orc.n8q(c))
    km = mont(curve, k).copy()
    if n == 0:
        zkmi.check(L.zkmi_group_scale_dev(c, group, None, None, 0, zkmi.ptr(km)))
        return b""
    d_in = zkmi.DeviceBuffer.from_host(pts)
    d_out = d_in if in_place else zkmi.DeviceBuffer.from_host(np.full(pts.size, 0xA5, np.uint8))
    if general:
        one = orc.fr_one(c).copy()
        zkmi.check(L.zkmi_group_batch_apply_key_dev(c, group, d_in.ptr, d_out.ptr, n, zkmi.ptr(km), zkmi.ptr(one)))
    else:
        zkmi.check(L.zkmi_group_scale_dev(c, group, d_in.ptr, d_out.ptr, n, zkmi.ptr(km)))
    out = d_out.to_host().tobytes()
    d_in.free()
    if not in_place:
        d_out.free()
    return out


@pytest.mark.parametrize("curve", CURVES)
def test_every_size_against_the_oracle(curve):
    ks = scalars(curve)
    for n in SIZES:
        for holes in ((True, False) if 0 < n <= 5 else (True,)):
            pts = bases(curve, n, holes)
            for k in (ks[4], ks[8], ks[-1]):                # r - 1, 0x55..5 mod r, a random one
                assert device(curve, pts, k) == oracle(curve, pts, k), (n, holes, hex(k))


@pytest.mark.parametrize("curve", CURVES)
def test_every_scalar_against_the_oracle_and_the_general_kernel(curve):
    """n = 257: two blocks, 64 whole inversion groups and one of a single point"""
    pts = bases(curve, 257)
    for k in scalars(curve):
        got = device(curve, pts, k)
        assert got == oracle(curve, pts, k), hex(k)
        assert got == device(curve, pts, k, general=True), hex(k)
    zero = device(curve, pts, 0)
    assert zero == bytes(pts.size)


@pytest.mark.parametrize("curve", CURVES)
def test_thousand_points_against_the_general_kernel(curve):
    pts = bases(curve, 1000)
    for k in scalars(curve)[4:]:
        assert device(curve, pts, k) == device(curve, pts, k, general=True), hex(k)


@pytest.mark.parametrize("curve", CURVES)
def test_in_place(curve):
    pts, k = bases(curve, 257), scalars(curve)[-2]
    assert device(curve, pts, k, in_place=True) == oracle(curve, pts, k)


@pytest.mark.parametrize("curve", CURVES)
def test_paged_host_form_with_pages_that_split_a_point(curve):
    zkmi.init()
    c, L = orc.CURVE_ID[curve], zkmi.lib()
    pts, k = bases(curve, 1000), scalars(curve)[-3]
    page = 1000                                                    # no multiple of the 64- or 96-byte point
    pg = zkmi.pages_of([pts[o:o + page] for o in range(0, pts.size, page)])
    outs = [np.full(min(777, pts.size - o), 0xA5, np.uint8) for o in range(0, pts.size, 777)]
    op, ol = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs]), (C.c_size_t * len(outs))(*[o.size for o in outs])
    km = mont(curve, k).copy()
    zkmi.check(L.zkmi_group_scale(c, 1, pg.pages, op, ol, len(outs), 1000, zkmi.ptr(km)))
    assert b"".join(o.tobytes() for o in outs) == oracle(curve, pts, k)
    # an input shorter than n points is refused
    assert L.zkmi_group_scale(c, 1, pg.pages, op, ol, len(outs), 1001, zkmi.ptr(km)) != 0 and b"shorter than n" in L.zkmi_last_error()
    assert L.zkmi_group_scale(c, 3, pg.pages, op, ol, len(outs), 1000, zkmi.ptr(km)) != 0 and b"unknown curve or group" in L.zkmi_last_error()
    assert L.zkmi_group_scale_dev(c, 1, None, None, 5, zkmi.ptr(km)) != 0 and b"null buffer" in L.zkmi_last_error()


@pytest.mark.parametrize("curve", CURVES)
def test_group_2(curve):
    c = orc.CURVE_ID[curve]
    pts = orc.geom_bases(c, 2, 5).reshape(5, -1).copy()
    pts[3] = 0
    pts = pts.reshape(-1)
    for k in (scalars(curve)[4], scalars(curve)[-1]):
        assert device(curve, pts, k, group=2) == oracle(curve, pts, k, group=2), hex(k)
        zkmi.init()
        out = np.zeros(pts.size, np.uint8)
        op, ol = (C.c_void_p * 1)(out.ctypes.data), (C.c_size_t * 1)(out.size)
        km = mont(curve, k).copy()
        zkmi.check(zkmi.lib().zkmi_group_scale(c, 2, zkmi.pages_of(pts).pages, op, ol, 1, 5, zkmi.ptr(km)))
        assert out.tobytes() == oracle(curve, pts, k, group=2)
