"""csrc/pairing.cuh on the CPU (tools/pairing_hosttest.hip, the same source with __device__ defined away) against
oracle/groth16_verify_oracle.py: pairing constants, Fq12 arithmetic, reduced pairings, bilinearity and the whole per-proof Groth16 check
on the golden proofs and their tampers. No GPU needed; the library's new entry points must still refuse to run without one."""
import os
import random
import subprocess

import pytest

import groth16_verify_oracle as O
import verify_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "bin", "pairing_hosttest")
SRC = os.path.join(ROOT, "tools", "pairing_hosttest.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "snarkjs_amd", "csrc")
CURVES = [(0, O.BN254, "groth16_bn128_n1024.json"), (1, O.BLS12381, "groth16_bls12381_n1024.json")]


@pytest.fixture(scope="module")
def tool():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("pairing.cuh", "pairing_host.hpp", "curve.cuh", "field.cuh", "host_field.hpp")]
    if not os.path.exists(TOOL) or any(os.path.getmtime(d) > os.path.getmtime(TOOL) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O0", "-std=c++17", "-I" + CSRC, SRC, "-o", TOOL])
    p = subprocess.Popen([TOOL], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def call(*args):
        p.stdin.write(" ".join(str(a) for a in args) + "\n")
        p.stdin.flush()
        out = p.stdout.readline().split()
        assert out and out[0] != "ERR", out
        return out
    yield call
    p.stdin.close()
    p.wait()


def H(v):
    return "%x" % int(v)


def g1w(o):
    return [H(o[0]), H(o[1]), H(o[2])]


def g2w(o):
    return [H(o[0][0]), H(o[0][1]), H(o[1][0]), H(o[1][1]), H(o[2][0]), H(o[2][1])]


def ints(out):
    return [int(x, 16) for x in out]


@pytest.mark.parametrize("ci,E,_f", CURVES)
def test_constants(tool, ci, E, _f):
    c = ints(tool("consts", ci))
    P = E.P
    for k in range(6):
        assert (c[2 * k], c[2 * k + 1]) == E.f2_pow(E.XI, k * (P - 1) // 6)
        assert (c[12 + 2 * k], c[13 + 2 * k]) == E.f2_pow(E.XI, k * (P * P - 1) // 6)
    assert (c[24], c[25]) == E.TWIST_B and c[26] == E.B1
    assert c[27] == (P ** 4 - P ** 2 + 1) // E.R                      # the chain's exponent: m = 1


@pytest.mark.parametrize("ci,E,_f", CURVES)
def test_fq12(tool, ci, E, _f):
    rnd = random.Random(0x9a1 + ci)
    P = E.P
    for _ in range(3):
        a = [rnd.randrange(P) for _ in range(12)]
        b = [rnd.randrange(P) for _ in range(12)]
        assert ints(tool("mul", ci, *map(H, a + b))) == E.f12_mul(a, b)
        assert ints(tool("sqr", ci, *map(H, a))) == E.f12_mul(a, a)
        assert E.f12_mul(ints(tool("inv", ci, *map(H, a))), a) == E.F12_ONE
        assert ints(tool("frob1", ci, *map(H, a))) == E.f12_pow(a, P)
        assert ints(tool("frob2", ci, *map(H, a))) == E.f12_pow(a, P * P)


def _pairs(E, vk, count, seed):
    """count (P, Q) pairs: P = k alpha_1 (random k), Q one of the key's G2 points"""
    rnd = random.Random(seed)
    al = O._g1(vk["vk_alpha_1"])
    qs = [vk[k] for k in ("vk_beta_2", "vk_gamma_2", "vk_delta_2")]
    out = []
    for i in range(count):
        pt = E.g1_mul(al, rnd.randrange(1, E.R))
        out.append((pt, qs[i % 3]))
    return out


@pytest.mark.parametrize("ci,E,f", CURVES)
def test_pairing_matches_oracle(tool, ci, E, f):
    vk, _, _ = V.golden(f)
    for pt, q in _pairs(E, vk, 8, 0x51 + ci):
        got = ints(tool("pair", ci, H(pt[0]), H(pt[1]), "1", *g2w(q)))
        assert got == E.final_exp(E.miller_loop(O._g2(q), pt))
    # bilinearity: e(7P, Q) = e(P, Q)^7 != 1
    pt, q = _pairs(E, vk, 1, 7)[0]
    e1 = ints(tool("pair", ci, H(pt[0]), H(pt[1]), "1", *g2w(q)))
    p7 = E.g1_mul(pt, 7)
    e7 = ints(tool("pair", ci, H(p7[0]), H(p7[1]), "1", *g2w(q)))
    assert e7 == E.f12_pow(e1, 7) and e1 != E.F12_ONE
    # infinity gives 1
    assert ints(tool("pair", ci, "0", "1", "0", *g2w(q))) == E.F12_ONE


def _verify(tool, ci, vk, pubs, proof):
    ic = vk["IC"]
    a = ["verify", ci, len(ic), len(pubs)] + g1w(vk["vk_alpha_1"]) + g2w(vk["vk_beta_2"]) + g2w(vk["vk_gamma_2"]) + g2w(vk["vk_delta_2"])
    for p in ic:
        a += g1w(p)
    a += g1w(proof["pi_a"]) + g2w(proof["pi_b"]) + g1w(proof["pi_c"]) + [H(x) for x in pubs]
    return int(tool(*a)[0])


@pytest.mark.parametrize("f", V.GOLDEN_FILES)
def test_verify_path(tool, f):
    vk, pubs, proof = V.golden(f)
    ci, E = (0, O.BN254) if vk["curve"] == "bn128" else (1, O.BLS12381)
    assert _verify(tool, ci, vk, pubs, proof) == 1
    for label, pu, p, want in V.tampers(E, vk, pubs, proof):
        got = _verify(tool, ci, vk, pu, p)
        if want is None:
            want = V.oracle_verdict(E, vk, pu, p)
        assert got == want, label


def test_new_entry_points_fail_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    import numpy as np
    from snarkjs_amd import zkmi, groth16_verify
    L = zkmi.lib()
    for s in ("zkmi_groth16_vk_load", "zkmi_groth16_verify_batch", "zkmi_groth16_vk_release", "zkmi_pairing_dev"):
        assert hasattr(L, s) and s in zkmi.SYMBOLS
    vk, pubs, proof = V.golden("groth16_bn128_n1024.json")
    with pytest.raises(zkmi.ZkmiError, match="no HIP device"):
        groth16_verify.VerifyingKey(vk)
    out = np.zeros(12 * 32, np.uint8)
    assert L.zkmi_pairing_dev(0, zkmi.ptr(out), zkmi.ptr(out), 1, zkmi.ptr(out)) != 0
    assert b"no HIP device" in L.zkmi_last_error()
