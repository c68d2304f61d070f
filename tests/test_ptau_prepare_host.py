"""powersOfTau.preparePhase2 / convert (snarkjs_amd/powersoftau_prepare.py; csrc/ptau_lagrange.cuh), the parts that need no device: the lane maps of the three
kernels enumerated on the CPU by tools/ptau_lagrange_hosttest.hip (plain, under the host sanitizers, and restated here in Python from the text it dumps), and
the whole driver with the oracle's G.ifft (ptau_verify_vectors.lagrange_of) in place of the device on the committed files: the identities the reference
satisfies on them (tests/test_gpu_ptau_prepare.py holds the device to the same). The per-lane arithmetic is on the 32-bit limbs of curve.cuh, which are
__device__ only: it is run on the device alone."""
import os
import struct
import subprocess

import pytest

import ptau_verify_vectors as P
from snarkjs_amd import powersoftau_prepare as tp
from snarkjs_amd import zkmi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ptau_lagrange_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEPS = [SRC] + [os.path.join(ROOT, "snarkjs_amd", "csrc", f) for f in ("ptau_lagrange.cuh", "gfft.cuh", "curve.cuh", "field.cuh")]


class OracleDevice:
    """powersoftau_prepare.Device on the CPU: the blocks first .. top of the oracle's ladder, memoised over the module"""
    ladders = {}

    def __init__(self):
        self.calls = []                           # (group, n_tau, first, top, zero_last) per call, in order

    def lagrange_section(self, cv, group, tau, n_tau, first, top, zero_last):
        tau = b"".join(tau) if isinstance(tau, (list, tuple)) else bytes(tau)
        sg = P.point_size(cv, group)
        assert len(tau) == n_tau * sg and n_tau == (1 << top) - (1 if zero_last else 0) and first <= top
        k = (cv["name"], group, tau, top, zero_last)
        if k not in self.ladders:
            self.ladders[k] = P.lagrange_of(cv, group, tau, top, zero_last)
        self.calls.append((group, n_tau, first, top, zero_last))
        return self.ladders[k][((1 << first) - 1) * sg:]


def header_powers(raw, n8q):
    return struct.unpack_from("<II", P.split(raw)[0][1], 4 + n8q)


def without_top_block(prepared, cv, power):
    """a prepared file whose section 12 ends after the block of 2^power points: what powersOfTau.convert was written for"""
    cut = (2 << power) * 2 * cv["n8q"]
    return P.join(prepared, [(t, b[:-cut] if t == 12 else b) for t, b in P.split(prepared)])


def check_truncation_case(prepare, curve):
    """preparePhase2 of a power-4 cut of the power-6 ceremony, as the reference gives it"""
    cv = P.curve_record(curve)
    n8q, s1 = cv["n8q"], 2 * cv["n8q"]
    raw, prepared = P.gold(f"ptau_{curve}_p6_c3b_raw.ptau"), P.gold(f"ptau_{curve}_p6_c3b.ptau")
    cut_raw = P.truncate4(raw, n8q)
    assert header_powers(cut_raw, n8q) == (4, 6)
    got, want = P.split(prepare(cut_raw)), dict(P.split(P.truncate4(prepared, n8q)))
    assert [t for t, _ in got] == [1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]
    got = dict(got)
    assert struct.unpack_from("<II", got[1], 4 + n8q) == (4, 4), "the reference writes the header without a ceremony power"
    assert got[1][:4 + n8q] == want[1][:4 + n8q]
    for t in (2, 3, 4, 5, 6, 7, 13, 14, 15):
        assert got[t] == want[t], t
    assert len(got[12]) == 63 * s1 == len(want[12])
    assert got[12][:31 * s1] == want[12][:31 * s1]
    assert got[12][31 * s1:] != want[12][31 * s1:], "the zeroed last point changes the top block"
    return got


# ---- the host tool ------------------------------------------------------------------------------------------------------------------------------------
def _build(name, extra):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    tool = os.path.join(ROOT, "tools", "bin", name)
    if not os.path.exists(tool) or any(os.path.getmtime(d) > os.path.getmtime(tool) for d in DEPS):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17"] + extra + ["-I" + os.path.join(ROOT, "snarkjs_amd", "csrc"), SRC, "-o", tool])
    return tool


@pytest.fixture(scope="module")
def tool():
    return _build("ptau_lagrange_hosttest", [])


def test_lane_maps_for_every_top_first_and_stage(tool):
    """each butterfly once, inside its block, with the twiddle of its index; idle slots idle; one twiddle per wave from 64 slots up; load and store maps"""
    r = subprocess.run([tool, "check", "10"], capture_output=True, text=True, timeout=120)
    # butterflies of the ladders first = 0 and first = top over top = 0 .. 10: sum over stages and blocks p >= max(st, first) of 2^(p-1)
    want = sum(1 << (p - 1) for top in range(11) for first in ({0, top}) for st in range(1, top + 1) for p in range(max(st, first), top + 1))
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(want)], r.stdout + r.stderr


def test_lane_maps_under_the_host_sanitizers():
    san = _build("ptau_lagrange_hosttest_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    r = subprocess.run([san, "check", "10"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    assert subprocess.run([san, "dump", "3", "3"], capture_output=True, text=True, timeout=60).returncode == 0


@pytest.mark.parametrize("top,first", [(0, 0), (1, 0), (1, 1), (3, 0), (6, 0), (6, 6), (7, 0), (8, 8)])
def test_dumped_maps_against_the_formulas_of_the_design(tool, top, first):
    """the maps as DESIGN 19 states them, written out again here: lane t = j 2^(top-st+1) + m', p = st + ilog2(m'), g = m' - 2^(p-st), lo = base_p + (g << st) + j"""
    r = subprocess.run([tool, "dump", str(top), str(first)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    base = lambda p: (1 << p) - (1 << first)
    pts = [tuple(map(int, x[1:])) for x in rows if x[0] == "P"]
    want_pts = []
    for p in range(first, top + 1):
        for i in range(1 << p):
            rev = int(format(i, f"0{p}b")[::-1], 2) if p else 0
            want_pts.append((len(want_pts), p, i, base(p) + rev))
    assert pts == want_pts
    stages = [tuple(map(int, x[1:])) for x in rows if x[0] == "S"]
    want = []
    for st in range(1, top + 1):
        slots = 1 << (top - st + 1)
        for t in range(1 << top):
            j, m = divmod(t, slots)
            p = st + m.bit_length() - 1 if m else 0
            if not m or p < first:
                want.append((st, t, 1, 0, j, 0, 0, 0))
                continue
            g = m - (1 << (p - st))
            lo = base(p) + (g << st) + j
            want.append((st, t, 0, p, j, lo, lo + (1 << (st - 1)), j << (top - st)))
        if slots >= 64:
            assert all(len({row[4] for row in want[-(1 << top):][w:w + 64]}) == 1 for w in range(0, 1 << top, 64)), "a wave holds two twiddles"
    assert stages == want


# ---- the driver, the oracle in place of the device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", P.CURVES)
def test_prepare_phase2_of_the_raw_p6_file_is_the_prepared_file(curve):
    dev = OracleDevice()
    raw, prepared = P.gold(f"ptau_{curve}_p6_c3b_raw.ptau"), P.gold(f"ptau_{curve}_p6_c3b.ptau")
    assert tp._prepare_phase2(raw, None, None, dev) == prepared
    assert dev.calls == [(1, 127, 0, 7, True), (2, 64, 0, 6, False), (1, 64, 0, 6, False), (1, 64, 0, 6, False)], "one call per section"
    # preparing a prepared file gives the same file: sections 12 - 15 of the input are ignored
    assert tp._prepare_phase2(prepared, None, None, OracleDevice()) == prepared


@pytest.mark.parametrize("curve", P.CURVES)
def test_prepare_phase2_of_a_power_4_cut(curve):
    check_truncation_case(lambda raw: tp._prepare_phase2(raw, None, None, OracleDevice()), curve)


@pytest.mark.parametrize("curve", P.CURVES)
def test_convert_appends_the_top_block_whether_it_is_there_or_not(curve):
    cv = P.curve_record(curve)
    prepared = P.gold(f"ptau_{curve}_p6_c3b.ptau")
    dev = OracleDevice()
    assert tp._convert(without_top_block(prepared, cv, 6), None, None, dev) == prepared
    assert dev.calls == [(1, 127, 7, 7, True)], "the one transform of 2^(power + 1) points"
    twice = tp._convert(prepared, None, None, OracleDevice())
    block = 128 * 2 * cv["n8q"]
    sec12 = dict(P.split(prepared))[12]
    assert twice != prepared and twice == P.join(prepared, [(t, b + sec12[-block:] if t == 12 else b) for t, b in P.split(prepared)])


def test_the_driver_writes_the_file_when_given_a_path(tmp_path, monkeypatch):
    monkeypatch.setattr(tp, "Device", OracleDevice)
    raw = P.gold("ptau_bn128_p6_c3b_raw.ptau")
    src, dst = tmp_path / "raw.ptau", tmp_path / "new.ptau"
    src.write_bytes(raw)
    out = tp.prepare_phase2(str(src), str(dst))
    assert out == dst.read_bytes() == P.gold("ptau_bn128_p6_c3b.ptau")
    assert tp.convert(out, str(dst)) == dst.read_bytes() != out


def test_the_driver_refuses_files_that_are_not_well_formed():
    cv = P.curve_record("bn128")
    raw = P.gold("ptau_bn128_p6_c3b_raw.ptau")
    secs = P.split(raw)
    zkey = next(f for f in sorted(os.listdir(P.GOLDEN)) if f.endswith(".zkey"))
    big = P.join(raw, [(t, b[:4 + cv["n8q"]] + (28).to_bytes(4, "little") + b[8 + cv["n8q"]:] if t == 1 else b) for t, b in secs])
    for label, data, text in (("a zkey as the file", P.gold(zkey), r"^ptau: Invalid File format$"),
                              ("no section 3", P.join(raw, [x for x in secs if x[0] != 3]), "^ptau: Missing section 3$"),
                              ("section 2 twice", P.join(raw, secs + [x for x in secs if x[0] == 2]), "^ptau: Section Duplicated 2$"),
                              ("section 4 one byte short", P.join(raw, [(t, b[:-1] if t == 4 else b) for t, b in secs]), "^Invalid section size reading$"),
                              ("power + 1 > Fr.s", big, r"beyond the limit of 2\^28 \(Fr\.s\)")):
        for fn in (tp._prepare_phase2, tp._convert):
            dev = OracleDevice()
            with pytest.raises(tp.PtauError, match=text):
                fn(data, None, None, dev)
            assert dev.calls == [], label
    with pytest.raises(tp.PtauError, match="^ptau: Missing section 12$"):
        tp._convert(raw, None, None, OracleDevice())


def test_the_library_exports_the_two_entry_points_and_refuses_without_a_device():
    import torch
    L = zkmi.lib()
    assert L.zkmi_ptau_lagrange_section and L.zkmi_ptau_lagrange_dev
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    cv = P.curve_record("bn128")
    with pytest.raises(zkmi.ZkmiError) as e:
        tp.Device().lagrange_section(cv, 1, P.tau_points(cv, 1, 2), 2, 0, 1, False)
    assert e.value.code == zkmi.ERR_NO_DEVICE
