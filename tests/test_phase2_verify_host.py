"""zKey.verifyFromInit / verifyFromR1cs (snarkjs_amd/groth16_phase2_verify.py), the parts that need no device: the block function the generator kernels run
against the sequential generator struct the golden vectors pin, the kernels' attempt-and-compaction rule against sequential Fr.fromRng draws, and the whole
driver with the CPU oracle's MSM, transform and pairing in place of the three device calls: the eight golden keys verify against their init keys and log their
recorded contribution hashes, and every row of the tamper table fails with the reference's line (tests/test_gpu_phase2_verify.py runs the same through the
kernels)."""
import ctypes as C

import numpy as np
import pytest

import phase2_verify_vectors as V
from snarkjs_amd import groth16_phase2 as p2
from snarkjs_amd import groth16_phase2_verify as pv
from snarkjs_amd import zkmi


def golden_seeds(curve):
    v = V.INDEX["vectors"][curve]
    return [x["seed"] for x in v["fromRng"]]


def block(seed, lo, hi=0):
    out = np.zeros(16, np.uint32)
    assert zkmi.lib().zkmi_chacha_block_host((C.c_uint32 * 8)(*seed), lo, hi, zkmi.ptr(out)) == 0
    return out


@pytest.mark.parametrize("curve", V.CURVES)
def test_block_function_against_the_generator_struct(curve):
    top = (1 << 32) - 1                           # the struct starts at block 2^32 - 1: its second block carries from word 12 into word 13
    for seed in golden_seeds(curve):
        assert np.array_equal(np.concatenate([block(seed, k) for k in range(3)]), V.host_words(seed, 0, 48))
        got = np.concatenate([block(seed, top), block(seed, top + 1), block(seed, top + 2)])
        assert np.array_equal(got, V.host_words(seed, 16 * top, 48))
        assert not np.array_equal(block(seed, top + 1), block(seed, 0))
    # the upper half of the 128-bit counter lands in words 14 and 15
    seed = golden_seeds(curve)[0]
    assert not np.array_equal(block(seed, 5, 1), block(seed, 5, 0)) and not np.array_equal(block(seed, 5, 1 << 32), block(seed, 5, 0))


def test_keystream_by_position():
    seed = golden_seeds("bn128")[1]
    whole = V.host_words(seed, 0, 100)
    for first in (0, 5, 16, 31):
        assert np.array_equal(V.host_words(seed, first, 40), whole[first:first + 40])


@pytest.mark.parametrize("curve", V.CURVES)
def test_attempt_and_compaction_rule_against_sequential_draws(curve):
    cv = V.curve_record(curve)
    vec = V.INDEX["vectors"][curve]["fromRng"]
    rejected_first = [x["seed"] for x in vec if x["frDraws"] > 4]
    assert rejected_first, "the golden vectors hold a seed whose first draw is rejected"
    for seed in rejected_first[:2] + [x["seed"] for x in vec if x["frDraws"] == 4][:1]:
        want, w_want = V.host_fr(cv["id"], seed, 5000)
        got, w_got = V.host_fr(cv["id"], seed, 5000, compact=True)
        assert np.array_equal(got, want) and w_got == w_want
        assert w_want % 8 == 0 and w_want >= 8 * 5000
        vals = [int.from_bytes(want[32 * i:32 * i + 32].tobytes(), "little") for i in range(0, 5000, 97)]
        assert all(v < cv["r"] for v in vals)
    for x in vec:                                 # the first draw is the reference's own
        got, w = V.host_fr(cv["id"], x["seed"], 1, compact=True)
        assert got.tobytes().hex() == x["fr"] and w == 2 * x["frDraws"]
    assert V.host_fr(cv["id"], vec[0]["seed"], 0, compact=True)[1] == 0 and V.host_fr(cv["id"], vec[0]["seed"], 0)[1] == 0


def test_generator_headers_as_a_host_program_under_the_host_sanitizers():
    """tools/chacha_hosttest.hip: chacha.cuh and phase2_host.hpp alone, with a main of its own, built with AddressSanitizer and UBSan"""
    import os
    import subprocess
    root = os.path.dirname(V.GOLDEN[:-len("/golden")])
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src, tool = os.path.join(root, "tools", "chacha_hosttest.hip"), os.path.join(root, "tools", "bin", "chacha_hosttest")
    deps = [src] + [os.path.join(root, "snarkjs_amd", "csrc", f) for f in ("chacha.cuh", "phase2_host.hpp", "host_field.hpp", "field.cuh")]
    if not os.path.exists(tool) or any(os.path.getmtime(d) > os.path.getmtime(tool) for d in deps):
        os.makedirs(os.path.dirname(tool), exist_ok=True)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                               "-fno-sanitize-recover=undefined", "-I" + os.path.join(root, "snarkjs_amd", "csrc"), src, "-o", tool])
    for curve in V.CURVES:
        seed = next(x["seed"] for x in V.INDEX["vectors"][curve]["fromRng"] if x["frDraws"] > 4)
        r = subprocess.run([tool] + [str(w) for w in seed] + ["3000"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout + r.stderr
        assert [int(w) for w in r.stdout.split()[1:]] == [V.host_fr(c, seed, 3000)[1] for c in (0, 1)]


def test_format_hash():
    b = bytes(range(64))
    assert pv.format_hash(b, "T: ") == "T: \n\t\t00010203 04050607 08090a0b 0c0d0e0f\n\t\t10111213 14151617 18191a1b 1c1d1e1f\n\t\t20212223 24252627 28292a2b 2c2d2e2f\n" \
                                       "\t\t30313233 34353637 38393a3b 3c3d3e3f"


@pytest.mark.parametrize("name", V.STEPS)
def test_the_golden_keys_verify_with_the_oracle_in_place_of_the_device(name):
    curve = V.curve_of_file(name)
    log, dev = V.Log(), V.OracleDevice()
    assert pv._verify(V.gold(V.init_of(name)), V.gold(f"setup_{curve}_p8.ptau"), V.gold(name), log, V.RANDOM64, dev) is True
    # the debug lines, the circuit hash, the contributions last to first with their recorded hashes (the beacon's parameters with it), "ZKey Ok!"
    assert log.lines == V.expected_success_lines(name)
    assert sum(x[1].startswith("contribution #") for x in log.lines) == len(V.chain_hashes(name)) == {"c1": 1, "b2": 2, "c3": 3}[name[-7:-5]]


@pytest.mark.parametrize("curve", V.CURVES)
def test_the_tamper_table(curve):
    cv = V.curve_record(curve)
    ptau = V.gold(f"setup_{curve}_p8.ptau")
    for label, init, key, level, line in V.tamper_table(curve):
        log, dev = V.Log(), V.OracleDevice()
        assert pv._verify(init, ptau, key, log, V.RANDOM64, dev) is False, label
        assert log.verdict_lines() == [(level, line)], label
        if "swapped" in label:                    # the sums really fail the ratio for this seed
            r1, r2 = dev.ratios["L" if "L points" in label else "H"]
            d2, d2_init = (pv._open_key(pv._Source(k), "")[2]["delta2"] for k in (key, init))
            assert V.oracle_same_ratio(cv, r1, r2, d2, d2_init) is False, label


def test_a_failing_contribution_reports_the_first_failure_only():
    """two tampers in one key: the earlier contribution's line is the one logged"""
    cv = V.curve_record("bn128")
    key = V.gold("phase2_bn128_full_c3.zkey")
    beta2 = pv._open_key(pv._Source(key), "")[2]["beta2"]
    key = V._contribution(cv, key, 2, lambda c: c.update(transcript=bytes(64)))
    key = V._contribution(cv, key, 0, lambda c: c.update(g2_spx=beta2))
    log = V.Log()
    assert pv._verify(V.gold("setup_bn128_full.zkey"), V.gold("setup_bn128_p8.ptau"), key, log, V.RANDOM64, V.OracleDevice()) is False
    assert log.lines == [("log", "INVALID(0): public key G1 and G2 do not have the same ration ")]


def test_keys_of_another_protocol_are_refused_in_the_references_words():
    plonk, init, ptau = V.gold("plonk_bn128_small.zkey"), V.gold("setup_bn128_full.zkey"), V.gold("setup_bn128_p8.ptau")
    with pytest.raises(p2.Phase2Error, match=r"^zkey file is not groth16$"):
        pv._verify(init, ptau, plonk, None, V.RANDOM64, V.OracleDevice())
    with pytest.raises(p2.Phase2Error, match=r"^zkeyinit file is not groth16$"):
        pv._verify(plonk, ptau, V.gold("phase2_bn128_full_c1.zkey"), None, V.RANDOM64, V.OracleDevice())
    with pytest.raises(p2.Phase2Error, match="random64 must be 64 bytes"):
        pv._verify(init, ptau, V.gold("phase2_bn128_full_c1.zkey"), None, bytes(63), V.OracleDevice())


def test_verify_without_a_device_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    with pytest.raises(zkmi.ZkmiError) as e:
        pv.verify_from_init(V.gold("setup_bn128_edge.zkey"), V.gold("setup_bn128_p8.ptau"), V.gold("phase2_bn128_edge_c1.zkey"), random64=V.RANDOM64)
    assert e.value.code == zkmi.ERR_NO_DEVICE
    out = np.zeros(64, np.uint8)
    L = zkmi.lib()
    seed = (C.c_uint32 * 8)(*range(8))
    assert L.zkmi_chacha_words_dev(seed, 0, None, 4) != 0 and b"no HIP device" in L.zkmi_last_error()
    assert L.zkmi_chacha_fr_dev(0, seed, None, 4, None) != 0
    assert L.zkmi_same_ratio_batch(0, zkmi.ptr(out), zkmi.ptr(out), zkmi.ptr(out), zkmi.ptr(out), 1, zkmi.ptr(out)) != 0
