"""wtns.check without a device: the Python restatement of the reference's loop (tests/wtns_check_vectors.py) is pinned to every golden case the unmodified
reference recorded (tests/golden/wtns_check_golden.json); the driver (snarkjs_amd/wtns_check.py), with the restatement in the device's place, is held to the
recorded lines, verdicts and errors; the progress lines and the batch cut are pure functions; and the host passes and lane routines of the kernels run on the
CPU (tools/r1cs_check_hosttest.hip), once more under the address and undefined-behaviour sanitizers."""
import hashlib
import os
import struct
import subprocess

import pytest

import wtns_check_vectors as V
from snarkjs_amd import wtns_check
from snarkjs_amd.workloads import synth_r1cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "r1cs_check_hosttest")
SRC = os.path.join(ROOT, "tools", "r1cs_check_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADERS = ("r1cs_check.cuh", "r1cs_host.hpp", "abc_layout.cuh", "field.cuh")
FLAGS = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "snarkjs_amd", "csrc")]
CASES = V.golden()
IDS = [c["name"] for c in CASES]
HEADER_LINES = 15                      # what the reference logs before its loop


def files(c):
    return V.golden_file(c["r1cs"]), V.golden_file(c["wtns"])


def test_golden_covers_the_cases_on_both_curves():
    for curve in ("bn128", "bls12381"):
        names = {c["name"][len(curve) + 1:] for c in CASES if c["curve"] == curve}
        assert names >= {"good", "bad_first", "bad_last", "bad_two", "dups", "descending", "wide_coefs", "wide_witness", "w0_is_2", "empty_constraint", "zero_constraints",
                         "trailing", "truncated", "truncated_count", "signal_beyond", "other_curve_witness", "odd_prime"}
    for c in CASES:
        r1cs, wtns = files(c)
        assert hashlib.sha256(r1cs).hexdigest() == c["r1csSha256"] and hashlib.sha256(wtns).hexdigest() == c["wtnsSha256"]
        assert len(r1cs) < 64 * 1024 and len(wtns) < 64 * 1024


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_restatement_agrees_with_the_reference(c):
    r1cs, wtns = files(c)
    if c["readsPast"]:
        with pytest.raises(V.PastTheEnd):
            V.first_bad_files(r1cs, wtns)
        return
    if "throws" in c:
        head, w = V.read_r1cs(r1cs), V.read_wtns(wtns)
        assert head["prime"] != w["q"] or head["prime"] not in V.CURVE_OF_R
        return
    bad = V.first_bad_files(r1cs, wtns)
    assert c["returns"] == (bad is None)
    if bad is not None:
        assert ["warn", f"··· aborting checking process at constraint {bad}"] in c["lines"]
        assert c["noLogger"]["throws"] == "Cannot read property 'warn' of undefined"
    else:
        assert c["noLogger"]["returns"] is True


def hold_driver_to_golden(c, new_device):
    """check() on one golden case, with and without a logger (tests/test_gpu_wtns_check.py runs the same on the device)"""
    r1cs, wtns = files(c)
    rec, dev = V.Recorder(), new_device()
    if c["readsPast"] and "throws" not in c:
        # the reference's verdict here comes from stale memory (it differs between the curves): the driver refuses, after the lines before the loop
        with pytest.raises(wtns_check.WtnsCheckError):
            wtns_check.check(r1cs, wtns, rec, device=dev)
        assert rec.lines == c["lines"][:HEADER_LINES]
    elif "throws" in c:
        with pytest.raises(wtns_check.WtnsCheckError) as e:
            wtns_check.check(r1cs, wtns, rec, device=dev)
        assert str(e.value) == c["throws"] and rec.lines == c["lines"]
        if len(c["lines"]) < HEADER_LINES and hasattr(dev, "calls"):
            assert dev.calls == [], "a call the reference refuses before its loop reaches no device"
    else:
        assert wtns_check.check(r1cs, wtns, rec, device=dev) is c["returns"]
        assert rec.lines == c["lines"]
    assert not getattr(dev, "loaded", None), "nothing stays resident"
    # no logger
    dev = new_device()
    if "returns" in c["noLogger"] and not c["readsPast"]:
        assert wtns_check.check(r1cs, wtns, device=dev) is True
    else:
        with pytest.raises(wtns_check.WtnsCheckError) as e:
            wtns_check.check(r1cs, wtns, device=dev)
        if not c["readsPast"] or "throws" in c:
            assert str(e.value) == c["noLogger"]["throws"]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_driver_reproduces_lines_verdicts_and_errors(c):
    hold_driver_to_golden(c, V.RestatedDevice)


def test_driver_takes_paths_and_keeps_a_layout_resident(tmp_path):
    by = {c["name"]: c for c in CASES}
    base, good = files(by["bn128_good"])
    p1, p2 = tmp_path / "c.r1cs", tmp_path / "w.wtns"
    p1.write_bytes(base); p2.write_bytes(good)
    rec, dev = V.Recorder(), V.RestatedDevice()
    assert wtns_check.check(str(p1), str(p2), rec, device=dev) is True and rec.lines == by["bn128_good"]["lines"]
    with wtns_check.Checker(str(p1), device=dev) as ck:
        ws = [V.golden_file(by[n]["wtns"]) for n in ("bn128_good", "bn128_bad_two", "bn128_bad_last", "bn128_wide_witness")]
        assert ck.check_many(ws) == [None, 9, 12, None]
        assert ck.check(str(p2)) is True and ck.check(V.read_wtns(ws[1])["witness"]) is False
        assert dev.calls.count("load") == 2, "one load for check(), one for the Checker"
        with pytest.raises(wtns_check.WtnsCheckError, match="does not match"):
            ck.check(V.golden_file(by["bn128_other_curve_witness"]["wtns"]))
        assert ck.check_many([]) == []
    assert not dev.loaded
    with pytest.raises(wtns_check.WtnsCheckError, match="Curve not supported"):
        wtns_check.Checker(V.golden_file(by["bn128_odd_prime"]["r1cs"]), device=dev)
    with pytest.raises(wtns_check.WtnsCheckError, match="r1cs: Invalid File format"):
        wtns_check.check(good, good, device=dev)
    with pytest.raises(wtns_check.WtnsCheckError, match="wtns: Invalid File format"):
        wtns_check.check(base, base, device=dev)
    with pytest.raises(wtns_check.WtnsCheckError, match="Version not supported"):
        wtns_check.check(base[:4] + struct.pack("<I", 2) + base[8:], good, device=dev)


def test_a_failure_before_a_truncated_count_is_reported_as_the_reference_does():
    """the section ends inside a count of constraint 12; a witness that fails constraint 9 never gets there"""
    by = {c["name"]: c for c in CASES}
    r1 = V.read_r1cs(V.golden_file(by["bn128_good"]["r1cs"]))
    cons = r1["constraints"]
    pos = 0
    for _ in range(3 * 12 + 1):
        pos += 4 + 36 * struct.unpack_from("<I", cons, pos)[0]
    data = V.golden_file(by["bn128_good"]["r1cs"])
    at = data.index(cons)
    cut = data[:at - 8] + struct.pack("<Q", pos + 1) + cons[:pos + 1] + data[at + len(cons):]
    rec = V.Recorder()
    assert wtns_check.check(cut, V.golden_file(by["bn128_bad_two"]["wtns"]), rec, device=V.RestatedDevice()) is False
    assert ["warn", "··· aborting checking process at constraint 9"] in rec.lines
    with pytest.raises(wtns_check.WtnsCheckError, match="outside the bounds of the DataView"):
        wtns_check.check(cut, V.golden_file(by["bn128_good"]["wtns"]), V.Recorder(), device=V.RestatedDevice())


def test_progress_indices():
    P = wtns_check.progress_indices
    assert P(500000, None) == []
    assert P(500001, None) == [500000]
    assert P(1500001, 1000000) == [500000, 1000000]
    assert P(1500001, 999999) == [500000]
    assert P(0, None) == [] and P(1500001, None) == [500000, 1000000, 1500000] and P(1500001, 0) == []


def test_satisfiable_generator_options():
    for curve in ("bn128", "bls12381"):
        r = synth_r1cs.R[curve]
        rows = {(0, 0): 0, (1, 1): 33, (2, 2): 65, (3, 0): 64, (4, 2): 0}
        nv, no, ni, cons, wit = synth_r1cs.satisfiable_circuit(curve, 9, seed=3, rows=rows, dups=True, wide=True)
        for (i, m), n in rows.items():
            assert len({s for s, _ in cons[i][m]}) == n
        assert any(len(lc) != len({s for s, _ in lc}) for c in cons for lc in c), "a signal named twice"
        assert any(v >= r for v in wit) and any(c >= r for cc in cons for lc in cc for _, c in lc)
        data, w = synth_r1cs.write_r1cs(curve, nv, no, ni, cons), synth_r1cs.write_wtns(curve, wit)
        assert V.first_bad_files(data, w) is None
        wit[max(s for s, _ in cons[6][2])] += 1
        assert V.first_bad_files(data, synth_r1cs.write_wtns(curve, wit)) == 6


# ---- the host passes and the lane routines, on the CPU ------------------------------------------------------------------------------------------------
def _build(out, extra):
    deps = [SRC] + [os.path.join(ROOT, "snarkjs_amd", "csrc", f) for f in HEADERS]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([HIPCC] + FLAGS + extra + [SRC, "-o", out])


def section(lcs):
    return b"".join(struct.pack("<I", len(lc)) + b"".join(struct.pack("<I", s) + int(v).to_bytes(32, "little") for s, v in lc) for lc in lcs)


def offset_requests():
    """(request line, expected answer)"""
    lcs = [[(1, 5)], [], [(2, 7), (3, 9)], [], [], [], [(0, 1)] * 3, [(4, 2)], []]                # three constraints
    sec = section(lcs)
    first = [0, 1, 1, 3, 3, 3, 3, 6, 7, 7]
    ok = "OK %d %s" % (len(sec), " ".join(map(str, first)))
    out = [(f"offsets 0 - -", "OK 0 0"), (f"offsets 0 5 {bytes(5).hex()}", "OK 0 0"), ("offsets 1 - -", "SHORT"),
           (f"offsets 3 {len(sec)} {sec.hex()}", ok),
           (f"offsets 3 {len(sec)},0,9 {(sec + bytes(range(9))).hex()}", ok),                          # trailing bytes, an empty page
           (f"offsets 3 2,{len(sec) - 2} {sec.hex()}", ok),                                            # a page boundary inside the first count
           (f"offsets 3 4,10,{len(sec) - 14} {sec.hex()}", ok),                                        # ... inside a record
           (f"offsets 3 {','.join(['1'] * len(sec))} {sec.hex()}", ok),                                # one byte a page
           (f"offsets 3 {len(sec) - 1} {sec[:-1].hex()}", "SHORT"),                                    # ends inside the last count
           (f"offsets 3 {len(sec) - 4} {sec[:-4].hex()}", "SHORT"),                                    # ends before the last count
           (f"offsets 3 {len(sec) - 20},10 {sec[:-10].hex()}", "SHORT"),                               # ends inside a record
           (f"offsets 2 {len(sec)} {sec.hex()}", "OK %d %s" % (len(section(lcs[:6])), " ".join(map(str, first[:7])))),
           (f"offsets 1 8 {(struct.pack('<I', 0xFFFFFFFF) + bytes(4)).hex()}", "SHORT")]
    return out


def field_requests():
    out = []
    for curve, field in (("bn128", "bn254"), ("bls12381", "bls12381")):
        r = V.R[curve]
        top = (1 << 256) - 1
        k = top // r
        le = lambda v: int(v).to_bytes(32, "little").hex()
        for v in (0, 1, r - 1, r, r + 1, 2 * r, k * r, k * r - 1, k * r + 1, top, top - 1, r + 3):
            out.append((f"reduce {field} {le(v)}", le(v % r)))
            out.append((f"coef {field} {le(v)}", le((v % r) * pow(2, 512, r) % r)))
        m = lambda v: le(v * pow(2, 256, r) % r)
        a, b = 0x1234567890abcdef1234567890abcdef % r, (r - 5)
        for x, y in ((a, b), (0, b), (r - 1, r - 1), (1, 1), (a, 0)):
            out.append((f"holds {field} {m(x)} {m(y)} {m(x * y % r)}", "1"))
            out.append((f"holds {field} {m(x)} {m(y)} {m((x * y + 1) % r)}", "0"))
    return out


def cut_requests():
    G = 1 << 30
    return [("cut 100 16 1000 65535", "10"), ("cut 100 16 99 65535", "1"), ("cut 100 5 100000 65535", "5"), ("cut 0 7 10 65535", "7"), ("cut 100 0 1000 65535", "0"),
            ("cut 1 100000 %d 65535" % G, "65535"), ("cut %d 16 %d 65535" % (300 << 20, 4 * G), "13"), ("cut %d 3 %d 65535" % (8 * G, 4 * G), "1")]


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    _build(TOOL, [])

    def ask(lines):
        r = subprocess.run([TOOL], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.split("\n")[:-1]
    return ask


@pytest.mark.parametrize("requests", [offset_requests, field_requests, cut_requests], ids=["offsets", "lane_routines", "batch_cut"])
def test_host_passes_and_lane_routines(tool, requests):
    reqs = requests()
    got = tool([q for q, _ in reqs])
    assert len(got) == len(reqs)
    for (q, want), g in zip(reqs, got):
        assert g == want, q[:120]


def test_offset_pass_on_the_golden_sections(tool):
    for c in CASES:
        if c["name"].startswith("bn128") and "throws" not in c or c["readsPast"]:
            r1 = V.read_r1cs(V.golden_file(c["r1cs"]))
            sec = r1["constraints"]
            got = tool([f"offsets {r1['nConstraints']} {len(sec) // 2},{len(sec) - len(sec) // 2} {sec.hex() or '-'}"])[0]
            short = c["name"].split("_", 1)[1] in ("truncated", "truncated_count")
            assert got == "SHORT" if short else got.startswith("OK "), c["name"]


def test_host_passes_and_lane_routines_under_the_sanitizers():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    san = TOOL + "_san"
    _build(san, ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])
    reqs = offset_requests() + field_requests() + cut_requests()
    r = subprocess.run([san], input="\n".join(q for q, _ in reqs) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.split("\n")[:-1] == [w for _, w in reqs], r.stdout[-400:] + r.stderr[-2000:]
