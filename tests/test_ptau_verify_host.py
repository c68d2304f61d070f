"""powersOfTau.verify (snarkjs_amd/powersoftau_verify.py; csrc/ptau_host.hpp, csrc/ptau_verify.hip), the parts that need no device: Blake2b-512 continued
from a partial state against hashlib, the library's way of making the sides of the Lagrange ladder (words widened once, running sums over dyadic segments, a
transform of normal-form scalars) against the reference's literal per-power formula on the CPU oracle, the host headers as a program of their own under the
host sanitizers, and the whole driver with the oracle's MSM, transform, conversion and Python pairing in place of the device on every case of
tests/golden/ptau_verify_golden.json: the reference's verdict or refusal and its lines (tests/test_gpu_ptau_verify.py holds the device to the same)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import ptau_verify_vectors as P
from snarkjs_amd import powersoftau_verify as tv
from snarkjs_amd import zkmi

MSG = bytes((i * 131 + (i >> 8) * 7 + 3) & 255 for i in range(1000))


def test_python_compress_is_blake2b():
    """the restatement the partial states are built with, against hashlib"""
    for n in (0, 1, 128, 129, 640):
        assert P.b2b_finish(P.b2b_initial(), b"", 0, MSG[:n]) == hashlib.blake2b(MSG[:n]).digest(), n


@pytest.mark.parametrize("pos", [0, 1, 127, 128])
@pytest.mark.parametrize("blocks", [0, 1, 3])
def test_resume_against_hashlib(pos, blocks):
    """a hash's first `blocks` blocks compressed, pos more bytes in the buffer, then the rest"""
    cut = 128 * blocks + pos
    partial = P.b2b_partial_of(MSG[:cut], pos)
    for rest in (1, 2, 127, 128, 129, 300):
        assert tv.blake2b_resume(partial, MSG[cut:cut + rest]) == hashlib.blake2b(MSG[:cut + rest]).digest(), (pos, blocks, rest)
    if cut:                                       # nothing more to hash: a buffer that holds bytes is the last block
        if pos:
            assert tv.blake2b_resume(partial, b"") == hashlib.blake2b(MSG[:cut]).digest()
    else:
        assert tv.blake2b_resume(partial, b"") == hashlib.blake2b(b"").digest()


def test_resume_with_a_length_above_2_to_32():
    """the length words carry 64 bits: a state no test could reach by hashing, against the Python restatement"""
    h = [(0x0123456789abcdef * (i + 1)) & ((1 << 64) - 1) for i in range(8)]
    for done, buffered in (((1 << 32) + 128 * 5, MSG[:77]), ((7 << 32), MSG[:128]), ((1 << 32) - 128, MSG[:128])):
        partial = P.b2b_partial(h, buffered, done)
        assert tv.blake2b_resume(partial, MSG[200:500]) == P.b2b_finish(h, buffered, done, MSG[200:500])
    low = P.b2b_partial(h, MSG[:77], 128 * 5)     # the same state with the upper length word cleared hashes to something else
    assert tv.blake2b_resume(low, MSG[200:500]) != tv.blake2b_resume(P.b2b_partial(h, MSG[:77], (1 << 32) + 128 * 5), MSG[200:500])


def test_resume_refuses_what_no_hasher_writes():
    L = zkmi.lib()
    out = np.zeros(64, np.uint8)
    bad = bytearray(P.b2b_partial(P.b2b_initial(), b"", 0))
    bad[128 + 4 * 18] = 129
    assert L.zkmi_blake2b512_resume(zkmi.ptr(np.frombuffer(bytes(bad), np.uint8)), None, 0, zkmi.ptr(out)) == 2
    assert b"beyond the 128-byte block buffer" in L.zkmi_last_error()
    assert L.zkmi_blake2b512_resume(None, None, 0, zkmi.ptr(out)) == 2
    with pytest.raises(ValueError):
        tv.blake2b_resume(bytes(215), b"")


@pytest.mark.parametrize("zero_last", [False, True])
@pytest.mark.parametrize("top", [0, 1, 7])
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", P.CURVES)
def test_dyadic_running_sums_and_normal_form_transform_against_the_literal_formula(curve, group, top, zero_last):
    cv = P.curve_record(curve)
    n = (1 << top) - (1 if zero_last else 0)
    tau = P.tau_points(cv, group, n, inf_at=3)
    lag = P.lagrange_of(cv, group, tau, top, zero_last)
    want = P.ladder_sides_literal(cv, group, tau, lag, top, zero_last, P.LADDER_SEED)
    assert P.ladder_sides_dyadic(cv, group, tau, lag, top, zero_last, P.LADDER_SEED) == want
    assert all(a == b for a, b in want), "the sections were built to satisfy the identity"
    if top:                                       # and a wrong Lagrange point breaks exactly its power
        sg = P.point_size(cv, group)
        p = top // 2 + 1
        at = ((1 << p) - 1 + 1) * sg
        bad = lag[:at] + lag[:sg] + lag[at + sg:]
        assert bad != lag
        got = P.ladder_sides_dyadic(cv, group, tau, bad, top, zero_last, P.LADDER_SEED)
        assert [a == b for a, b in got] == [q != p for q in range(top + 1)]


def test_host_headers_as_a_program_under_the_host_sanitizers():
    """tools/ptau_hosttest.hip: ptau_host.hpp alone, with a main of its own, built with AddressSanitizer and UBSan"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, tool = os.path.join(root, "tools", "ptau_hosttest.hip"), os.path.join(root, "tools", "bin", "ptau_hosttest")
    deps = [src] + [os.path.join(root, "snarkjs_amd", "csrc", f) for f in ("ptau_host.hpp", "host_field.hpp", "field.cuh")]
    if not os.path.exists(tool) or any(os.path.getmtime(d) > os.path.getmtime(tool) for d in deps):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                               "-fno-sanitize-recover=undefined", "-I" + os.path.join(root, "snarkjs_amd", "csrc"), src, "-o", tool])
    for n in (0, 1, 1000):
        r = subprocess.run([tool, str(n)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split() == ["ok", hashlib.blake2b(MSG[:n]).hexdigest()], r.stdout + r.stderr


def test_section_check_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    cv = P.curve_record("bn128")
    with pytest.raises(zkmi.ZkmiError) as e:
        tv.Device().section_check(cv, 1, P.tau_points(cv, 1, 2), 2, None, 1, False, P.PAIR_SEED, P.LADDER_SEED)
    assert e.value.code == zkmi.ERR_NO_DEVICE


def test_the_golden_files_are_the_recorded_ones():
    import hashlib as h
    for name, rec in P.INDEX["files"].items():
        raw = P.gold(name)
        assert h.sha256(raw).hexdigest() == rec["sha256"] and len(raw) == rec["bytes"] < 120 * 1024, name
    assert len(P.CASES) == 2 * 19 and {c["curve"] for c in P.CASES} == set(P.CURVES)


def test_response_hashes_of_the_golden_lines():
    """zkmi_blake2b512_resume on the partial states of real contributions: the first "Response Hash:" line of every contribution the reference printed"""
    from snarkjs_amd.groth16_phase2_verify import format_hash
    seen = 0
    for case in P.CASES:
        if case["label"] != "p6 prepared unpatched":
            continue
        cv = P.curve_record(case["curve"])
        contrs = tv._read_contributions(cv, dict(P.split(P.case_file(case)))[7])
        lines = [t for _, t in P.case_lines(case)]
        for c in contrs:
            at = lines.index(f"Contribution #{c['id']}: {c['name']}")
            assert lines[at + 2] == format_hash(c["responseHash"], "Response Hash:")
            seen += 1
    assert seen == 6


@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_the_driver_on_every_golden_case_with_the_oracle_in_place_of_the_device(case):
    """the reference's verdict or refusal and its info / warn / error lines, in its order"""
    cv = P.curve_record(case["curve"])
    log, dev, raw = P.Log(), P.OracleDevice(), P.case_file(case)
    if "throws" in case:
        assert case["throws"].strip().endswith(": Invalid File format")        # the reference names the file in front, for a file in memory "[object Object]"
        with pytest.raises(tv.PtauError, match=r"^ptau: Invalid File format$"):
            tv._verify(raw, log, P.RANDOM32, dev)
        assert log.lines == P.case_lines(case) == []
        return
    assert tv._verify(raw, log, P.RANDOM32, dev) is case["verdict"]
    assert log.lines == P.case_lines(case)
    if "swapped" in case["label"]:                # the oracle's sums really fail: a pass by a chance of 2^-32 is not what is tested
        last = tv._read_contributions(cv, dict(P.split(raw))[7])[-1]
        g1, g2 = tv.generators_lem(cv)
        if "tauG1 points" in case["label"]:
            assert P.V2.oracle_same_ratio(cv, dev.calls[0][1], dev.calls[0][2], g2, last["tauG2"]) is False
        elif "tauG2 points" in case["label"]:
            assert P.V2.oracle_same_ratio(cv, g1, last["tauG1"], dev.calls[1][1], dev.calls[1][2]) is False
        else:
            k = 0 if "section 12" in case["label"] else 1
            assert dev.calls[k][3][-1] is False and all(dev.calls[k][3][:-1]) and all(all(c[3]) for i, c in enumerate(dev.calls) if i != k)


def test_the_driver_refuses_what_it_cannot_do():
    cv = P.curve_record("bn128")
    raw = P.gold("ptau_bn128_p6_c3b_raw.ptau")
    with pytest.raises(tv.PtauError, match="random32 must be 32 bytes"):
        tv._verify(raw, None, bytes(31), P.OracleDevice())
    # a header that states power 28 on BN254: the tauG1 ladder would need a transform of 2^29 elements
    big = P.join(raw, [(t, b[:4 + cv["n8q"]] + (28).to_bytes(4, "little") + b[8 + cv["n8q"]:] if t == 1 else b) for t, b in P.split(raw)])
    with pytest.raises(tv.PtauError, match=r"beyond the limit of 2\^28 \(Fr\.s\)"):
        tv._verify(big, None, P.RANDOM32, P.OracleDevice())
    # the four thrown messages of readContributions
    sec7 = dict(P.split(raw))[7]
    body = bytearray(sec7)
    first_params = 4 + 3 * 64 + 2 * 128 + 6 * 64 + 3 * 128 + 216 + 64 + 8
    assert body[first_params] == 1 and body[first_params + 1] == 2          # the name parameter of "C1"
    for edit, text in (((first_params, 4), "Parameter not recognized"), ((first_params, 0), "Parameters in the contribution must be sorted"),
                       ((first_params + 1, 200), "Parameters do not match")):
        b = bytearray(sec7)
        b[edit[0]] = edit[1]
        with pytest.raises(tv.PtauError, match=text):
            tv._read_contributions(cv, bytes(b))
    with pytest.raises(tv.PtauError, match="Invalid contribution section size"):
        tv._read_contributions(cv, sec7 + b"\0")


def test_what_the_reference_throws_at_a_section_comes_after_the_lines_before_it():
    """src/powersoftau_verify.js reports the last contribution before it opens section 2 (startReadUniqueSection / endReadSection throw there), and reaches
    section 6 only after the four point sections"""
    cv = P.curve_record("bn128")
    raw = P.gold("ptau_bn128_p6_c3b_raw.ptau")
    secs = P.split(raw)
    ok_line = [("info", "Powers Of tau file OK!")]
    for label, edited, text in (("no section 3", [x for x in secs if x[0] != 3], "ptau: Missing section 3"),
                                ("section 2 twice", secs + [x for x in secs if x[0] == 2], "ptau: Section Duplicated 2"),
                                ("section 4 one byte short", [(t, b[:-1] if t == 4 else b) for t, b in secs], "Invalid section size reading")):
        log, dev = P.Log(), P.OracleDevice()
        with pytest.raises(tv.PtauError, match="^" + text + "$"):
            tv._verify(P.join(raw, edited), log, P.RANDOM32, dev)
        assert log.lines == ok_line, label
        assert len(dev.calls) == {"no section 3": 1, "section 2 twice": 0, "section 4 one byte short": 2}[label], "no device work at or after the section that throws"
    log = P.Log()
    with pytest.raises(tv.PtauError, match="^File has no BetaG2 section$"):
        tv._verify(P.join(raw, [x for x in secs if x[0] != 6]), log, P.RANDOM32, P.OracleDevice())
    assert log.lines == ok_line + [("error", "File has no BetaG2 section")]
    # a beacon contribution without its parameters is refused, not a KeyError
    sec7 = bytearray(dict(secs)[7])
    contrs = tv._read_contributions(cv, bytes(sec7))
    assert contrs[2]["type"] == 1 and contrs[2]["name"] == "B3"
    tail = bytes([1, 2]) + b"B3" + bytes([2, 10, 3, 31]) + bytes(contrs[2]["beaconHash"])
    assert bytes(sec7).endswith(tail)
    cut = bytes(sec7[:len(sec7) - len(tail) - 4]) + (4).to_bytes(4, "little") + bytes([1, 2]) + b"B3"
    with pytest.raises(tv.PtauError, match="beacon contribution #3 has no beaconHash or numIterationsExp parameter"):
        tv._verify(P.join(raw, [(t, cut if t == 7 else b) for t, b in secs]), None, P.RANDOM32, P.OracleDevice())
