"""The four-pass Fr NTT (csrc/ntt.hip: get_plan cuts a transform into ceil(log_n / 8) passes, so every size from 2^25 up runs four), which no other
test reaches. Four passes are not three plus one: only there does the last pass reverse TWO middle digits (Krest) and only there does a strided pass
with pass == 2 exist, and these feed the inter-pass twiddle exponents and the natural-order output addresses; the pre-scale tables (rowoff / rowinc)
and the zero-padded first pass get their fourth entries only there.

  test_four_passes_small_sizes_vs_oracle   ZKMI_NTT_DIGIT = 3, 4, 5 turns 2^10..2^18 into four-pass transforms (digits of unequal widths among them), both
      limb forms forced, one child process per setting (the switches are read once): forward, inverse, fused pre-scale, in-place inverse and zero-padded
      transforms, byte for byte against the CPU oracle; under ZKMI_NTT_DIGIT = 3 a whole Groth16 proof at 2^12, whose transforms are four-pass, batched
      (gridDim.y) and pre-scaled at once. The refusal of a size that would need a fifth pass is checked there too: an error return, nothing launched.
  test_four_passes_real_sizes_closed_form  BN254 at 2^25 and 2^26, BLS12-381 at 2^25, default settings, everything large on the device: the transform of
      x[j] = f g^j is X[k] = f (g^n - 1) / (g w^k - 1), compared at EVERY output with that closed form built from element-wise kernels the suite holds
      to the oracle elsewhere, and at 64 outputs with the closed form in Python integers; the fused pre-scale, the inverse and the zero-padded transform
      against it; and for generator-drawn data 64 outputs against Polynomial.evaluate at w^k, the definition of the transform through a kernel that
      shares no code with the NTT. A twiddle that forward and inverse agree on passes a round trip and a DC-term check; it does not pass these.

Every comparison is exact. tests/test_ntt_plan_host.py pins the digit splits these tests rely on; each test asks the probe again for what it runs."""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CURVES = ["bn128", "bls12381"]
UNSUPPORTED = 4                                   # include/zkmi.h
sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()

# ---- four passes at the smallest sizes -----------------------------------------------------------------------------------------------------------------
CAP = 18                                          # the largest size here: the oracle is still quick
FOUR_PASS = {3: [10, 11, 12], 4: [13, 14, 15, 16], 5: [16, 17, 18]}         # the sizes up to 2^CAP a digit cap turns into four passes
FIFTH_PASS = {3: 13, 4: 17, 5: 21}                                            # the first size that would need a fifth
PROOF_LG, PROOF_SEED = 12, 0x4E77                                             # the Groth16 key proved under ZKMI_NTT_DIGIT = 3
DONE = "ntt passes ok"


def field_r(name):
    return int(json.load(open(os.path.join(TESTS, "golden", f"{name}_kernel_vectors.json")))["r"])


def le32(v):
    return np.frombuffer(int(v).to_bytes(32, "little"), np.uint8)


def small_inputs(name, lg):
    """x: seeded elements. edge: the same kind with 0, 1, r - 1 and the Montgomery one at fixed places, the ends and the middle among them.
    (first, inc) of the two fused pre-scales: the coset step of the Groth16 prover, and unrelated elements. The in_len of the zero-padded transforms."""
    c, n, r = O.CURVE_ID[name], 1 << lg, field_r(name)
    x = synth.elems(0x4E00 + lg, n)
    edge = synth.elems(0x4F00 + lg, n).reshape(n, 32).copy()
    for at, v in ((0, le32(r - 1)), (1, le32(0)), (2, le32(1)), (3, O.fr_one(c)), (n // 2, le32(r - 1)), (n // 2 + 1, O.fr_one(c)), (n - 2, le32(0)), (n - 1, le32(1))):
        edge[at] = v
    pre = {"coset": (O.fr_e(c, 5), O.fr_w(c, lg + 1)), "other": (synth.elems(0x4E51, 1), synth.elems(0x4E52, 1))}
    return x, edge.reshape(-1), pre, (1, n // 4 + 3, n - 1)


def small_references(name, lg):
    """sha256 of what the oracle computes for every check of one size (compared as digests so that one set of references serves all six settings)"""
    c, n = O.CURVE_ID[name], 1 << lg
    x, edge, pre, in_lens = small_inputs(name, lg)
    ref = {"fft": sha(O.ntt(c, x)), "ifft": sha(O.ntt(c, x, True)), "fft_edge": sha(O.ntt(c, edge)), "ifft_edge": sha(O.ntt(c, edge, True))}
    for k, (first, inc) in pre.items():
        ref["pre_" + k] = sha(O.ntt(c, O.apply_key(c, x, first, inc)))
    for m in in_lens:
        padded = x.copy()
        padded[m * 32:] = 0
        ref["pad_%d" % m] = sha(O.ntt(c, padded))
    return ref


@pytest.fixture(scope="module")
def small_reference_dir(tmp_path_factory):
    """The oracle's side of test_four_passes_small_sizes_vs_oracle, computed once for its six settings and handed to the child processes as files: the
    digests of every transform at 2^10..2^CAP, and a synthetic Groth16 key at 2^PROOF_LG with the oracle's proof."""
    import synth_zkey
    from snarkjs_amd import binfile, zkmi
    zkmi.init(0)
    d = tmp_path_factory.mktemp("ntt_passes")
    refs = {"%s:%d" % (name, lg): small_references(name, lg) for name in CURVES for lg in range(10, CAP + 1)}
    zkey, wtns = synth_zkey.make("bn128", PROOF_LG, seed=PROOF_SEED)
    zk_ = binfile.read_groth16_zkey(zkey)
    assert zk_["domainSize"] == 1 << PROOF_LG
    r_m, s_m = O.fr_e(O.BN128, 0x1234567), O.fr_e(O.BN128, 0x7654321)
    want = O.groth16_prove(O.BN128, zk_, binfile.read_wtns(wtns)["witness"], r_m, s_m)
    refs["proof"] = [bytes(p).hex() for p in want]
    (d / "proof.zkey").write_bytes(bytes(zkey))
    (d / "proof.wtns").write_bytes(bytes(wtns))
    (d / "refs.json").write_text(json.dumps(refs))
    return str(d)


def probe(L, c, lg):
    """(passes, digit widths, 29-bit limbs) of a transform of 2^lg points in this process, or None where the driver refuses the size"""
    n, l, f = C.c_uint32(0), (C.c_uint32 * 4)(), C.c_int(-1)
    if L.zkmi_ntt_plan_probe(c, lg, C.byref(n), l, C.byref(f)) != 0:
        return None
    return n.value, tuple(l)[:n.value], f.value


def child_main(ref_dir):
    """The body of one setting of test_four_passes_small_sizes_vs_oracle, in a process started with ZKMI_NTT_DIGIT and ZKMI_NTT29 set."""
    import snarkjs_amd
    from snarkjs_amd import binfile, groth16, zkmi
    digit, force = int(os.environ["ZKMI_NTT_DIGIT"]), os.environ["ZKMI_NTT29"]
    refs = json.load(open(os.path.join(ref_dir, "refs.json")))
    zkmi.init(0)
    L = zkmi.lib()

    def dev(fn, src, n, *args):
        """fn(..., d_in, ..., d_out, ...) through fresh device buffers; the output's bytes"""
        din, dout = zkmi.DeviceBuffer.from_host(src), zkmi.DeviceBuffer(n * 32)
        try:
            zkmi.check(fn(din.ptr, dout.ptr, *args))
            return dout.to_host()
        finally:
            din.free(); dout.free()

    for name in CURVES:
        c, cv = O.CURVE_ID[name], snarkjs_amd.get_curve_from_name(name)
        plans = {lg: probe(L, c, lg) for lg in range(10, CAP + 1)}
        # the probe first: this setting reaches the paths it is here for
        four = [lg for lg, p in plans.items() if p and p[0] == 4]
        assert four and four == FOUR_PASS[digit], (name, plans)
        assert any(len(set(plans[lg][1])) > 1 for lg in four), (name, plans)                     # digits of unequal widths: the reversal is no plain swap
        assert all(p[2] == int(force == "1") and sum(p[1]) == lg and max(p[1]) <= digit for lg, p in plans.items() if p), (name, plans)
        fewer = [lg for lg, p in plans.items() if p and p[0] in (2, 3)]                           # free here: the one-digit reversal at other widths
        assert sorted(fewer + four) == [lg for lg in plans if plans[lg]] and all(plans[lg] is None for lg in range(FIFTH_PASS[digit], CAP + 1))
        for lg in fewer + four:
            n, ref, tag = 1 << lg, refs["%s:%d" % (name, lg)], (name, lg, plans[lg])
            x, edge, pre, in_lens = small_inputs(name, lg)
            assert sha(cv.Fr.fft(x)) == ref["fft"], ("fft",) + tag
            assert sha(cv.Fr.ifft(x)) == ref["ifft"], ("ifft",) + tag
            assert sha(cv.Fr.fft(edge)) == ref["fft_edge"], ("fft, edge values",) + tag
            assert sha(cv.Fr.ifft(edge)) == ref["ifft_edge"], ("ifft, edge values",) + tag
            for k, (first, inc) in pre.items():
                got = dev(lambda i, o: L.zkmi_ntt_dev(c, i, o, lg, 0, zkmi.ptr(first), zkmi.ptr(inc)), x, n)
                assert sha(got) == ref["pre_" + k], ("fused pre-scale", k) + tag
            d = zkmi.DeviceBuffer.from_host(x)
            try:
                zkmi.check(L.zkmi_ntt_dev(c, d.ptr, d.ptr, lg, 1, None, None))
                assert sha(d.to_host()) == ref["ifft"], ("in-place inverse",) + tag
            finally:
                d.free()
            for m in in_lens:                                                                     # the input buffer holds in_len elements and no more
                got = dev(lambda i, o: L.zkmi_ntt_padded_dev(c, i, m, o, lg, 0), x[:m * 32], n)
                assert sha(got) == ref["pad_%d" % m], ("zero-padded", m) + tag
        # a size that would need a fifth pass: an error return of the host, before anything is launched (the buffers are whole all the same)
        lg = FIFTH_PASS[digit]
        din, dout = zkmi.DeviceBuffer(32 << lg), zkmi.DeviceBuffer(32 << lg)
        try:
            zkmi.check(L.zkmi_memset_dev(din.ptr, 0, 32 << lg))
            for rc in (L.zkmi_ntt_dev(c, din.ptr, dout.ptr, lg, 0, None, None), L.zkmi_ntt_padded_dev(c, din.ptr, 5, dout.ptr, lg, 1)):
                msg = L.zkmi_last_error().decode()
                assert rc == UNSUPPORTED and "log_n = %d " % lg in msg and "cap of %d bits" % digit in msg, (name, lg, rc, msg)
        finally:
            din.free(); dout.free()
    if digit == 3:
        # Groth16's A / B / C chains: the batched launch (gridDim.y) has no entry of its own; at 2^12 its inverse and pre-scaled forward transforms are four-pass
        assert probe(L, O.BN128, PROOF_LG)[0] == 4
        zkey = open(os.path.join(ref_dir, "proof.zkey"), "rb").read()
        w = binfile.read_wtns(open(os.path.join(ref_dir, "proof.wtns"), "rb").read())["witness"]
        pk = groth16.ProvingKey(zkey)
        got = pk.prove_raw(w, O.fr_e(O.BN128, 0x1234567), O.fr_e(O.BN128, 0x7654321))
        pk.release()
        assert [bytes(p).hex() for p in got] == refs["proof"], "Groth16 proof at 2^%d" % PROOF_LG
    print(DONE)


@pytest.mark.parametrize("force", ["1", "0"])
@pytest.mark.parametrize("digit", [3, 4, 5])
def test_four_passes_small_sizes_vs_oracle(small_reference_dir, digit, force):
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_ntt_passes as T\nT.child_main(%r)\n" % (ROOT, TESTS, small_reference_dir)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, ZKMI_NTT_DIGIT=str(digit), ZKMI_NTT29=force))
    assert r.returncode == 0 and DONE in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- four passes at the real sizes ---------------------------------------------------------------------------------------------------------------------
BLOCK_LG = 18                                     # the host's share: one block of 2^18 elements (8 MiB)
F, G = 7, 11                                      # x[j] = F G^j
SAMPLES = 64


def sample_indices(n, split, seed):
    """64 outputs: the ends and the middle, both sides of every digit boundary of the split (counted from either end: the output digits run the other
    way round than the input digits), the rest from a seeded generator"""
    ks = [0, 1, 2, n // 2, n - 1]
    for digits in (split, split[::-1]):
        a = 0
        for w in digits[:-1]:
            a += w
            ks += [1 << a, (1 << a) - 1]
    rng = random.Random(seed)
    out = []
    for k in ks + [rng.randrange(n) for _ in range(4 * SAMPLES)]:
        if k not in out and len(out) < SAMPLES:
            out.append(k)
    assert len(out) == SAMPLES and all(k in out for k in ks)
    return out


def run_real_size(name, lg, with_padding_and_random, passes=4):
    """The recipe of test_four_passes_real_sizes_closed_form at 2^lg (a function of its own so that a failure can be told from a failure of a helper
    kernel at a length it had not seen: at 2^20, where the oracle vouches for the transform, it must pass with passes = 3)."""
    from snarkjs_amd import zkmi
    zkmi.init(0)
    L, c, n, r = zkmi.lib(), O.CURVE_ID[name], 1 << lg, field_r(name)
    plan = probe(L, c, lg)
    assert plan and plan[0] == passes and sum(plan[1]) == lg, plan
    ks = sample_indices(n, plan[1], 0x4E77 + lg)
    R = (1 << 256) % r
    mont = lambda v: le32(v % r * R % r)                               # an integer as the 32 bytes the library holds for it
    w = int.from_bytes(bytes(O.fr_w(c, lg)), "little") * pow(R, -1, r) % r
    assert pow(w, n, r) == 1 and pow(w, n // 2, r) == r - 1 and pow(G, n, r) != 1       # w has order n; G w^k is never 1
    f_m, g_m, one_m, w_m = O.fr_e(c, F), O.fr_e(c, G), O.fr_one(c), O.fr_w(c, lg)
    assert bytes(f_m) == bytes(mont(F)) and bytes(one_m) == bytes(mont(1))
    blk = min(lg, BLOCK_LG)

    def is_zero(buf):
        z = C.c_int(-1)
        zkmi.check(L.zkmi_poly_is_zero_dev(c, buf.ptr, n, C.byref(z)))
        return z.value == 1

    def differs(y, x):
        """y -= x on the device; True unless every element came out zero"""
        zkmi.check(L.zkmi_poly_axpy_dev(c, y.ptr, x.ptr, n, None, 1))
        return not is_zero(y)

    def element(buf, k):
        return bytes(buf.to_host(32, 32 * k))

    bufs = []
    try:
        for _ in range(4):
            bufs.append(zkmi.DeviceBuffer(n * 32))
        ones, x, X, t = bufs
        # (a) x[j] = F G^j from tiled Montgomery ones; X = fft(x) against F (G^n - 1) / (G w^k - 1) at every k
        zkmi.check(L.zkmi_memcpy_h2d(ones.ptr, zkmi.ptr(np.tile(one_m, 1 << blk)), 32 << blk))
        m = 1 << blk
        while m < n:                                                    # doubling copies: the two halves never overlap
            zkmi.check(L.zkmi_memcpy_d2d(ones.ptr + 32 * m, ones.ptr, 32 * m))
            m *= 2
        zkmi.check(L.zkmi_fr_batch_apply_key_dev(c, ones.ptr, x.ptr, n, zkmi.ptr(f_m), zkmi.ptr(g_m)))
        assert [element(x, j) for j in (0, 1, n - 1)] == [bytes(mont(F * pow(G, j, r))) for j in (0, 1, n - 1)]
        top = mont(F * (pow(G, n, r) - 1))
        zkmi.check(L.zkmi_fr_batch_apply_key_dev(c, ones.ptr, X.ptr, n, zkmi.ptr(g_m), zkmi.ptr(w_m)))     # G w^k
        zkmi.check(L.zkmi_poly_axpy_dev(c, X.ptr, ones.ptr, n, None, 1))                                   # G w^k - 1
        zkmi.check(L.zkmi_fr_batch_dev(c, zkmi.BATCH_INVERSE, X.ptr, t.ptr, n))
        zkmi.check(L.zkmi_poly_scale_dev(c, t.ptr, n, zkmi.ptr(top)))                                      # t = the closed form
        zkmi.check(L.zkmi_ntt_dev(c, x.ptr, X.ptr, lg, 0, None, None))                                     # X = the transform
        # independently of those element-wise kernels: 64 outputs against the closed form in Python integers
        want = {k: bytes(mont(F * (pow(G, n, r) - 1) * pow(G * pow(w, k, r) - 1, -1, r))) for k in ks}
        bad = [k for k in ks if element(X, k) != want[k]]
        assert not bad, ("fft of F G^j: outputs differ from F (G^n - 1) / (G w^k - 1)", name, lg, plan, bad)
        assert [element(t, k) for k in ks] == [want[k] for k in ks], ("the closed form built on the device differs from the host's", name, lg)
        assert not differs(t, X), ("fft of F G^j: some output differs from the closed form", name, lg, plan)
        # (b) the fused pre-scale: fft(ones, first = F, inc = G) is the same buffer
        zkmi.check(L.zkmi_ntt_dev(c, ones.ptr, t.ptr, lg, 0, zkmi.ptr(f_m), zkmi.ptr(g_m)))
        assert not differs(t, X), ("fused pre-scale", name, lg, plan)
        # (c) the inverse of the verified X gives x back
        zkmi.check(L.zkmi_ntt_dev(c, X.ptr, t.ptr, lg, 1, None, None))
        assert not differs(t, x), ("inverse", name, lg, plan)
        if not with_padding_and_random:
            return
        # (d) zero padding: the first in_len elements of x, the rest read as zero, against the transform of a copy whose tail was cleared
        in_len = n // 2 + 3
        zkmi.check(L.zkmi_ntt_padded_dev(c, x.ptr, in_len, t.ptr, lg, 0))
        zkmi.check(L.zkmi_memcpy_d2d(ones.ptr, x.ptr, 32 * in_len))
        zkmi.check(L.zkmi_memset_dev(ones.ptr + 32 * in_len, 0, 32 * (n - in_len)))
        zkmi.check(L.zkmi_ntt_dev(c, ones.ptr, ones.ptr, lg, 0, None, None))
        assert not is_zero(ones) and not differs(t, ones), ("zero-padded", name, lg, plan)
        # (e) arbitrary data: elements drawn by the generator kernel; output k is the polynomial with these coefficients evaluated at w^k
        seed = (C.c_uint32 * 8)(*range(0x4E01, 0x4E09))
        zkmi.check(L.zkmi_chacha_fr_dev(c, seed, x.ptr, n, None))
        head = x.to_host(32 * 64).reshape(64, 32)
        assert len({bytes(v) for v in head}) == 64 and element(x, n - 1) != bytes(32)
        zkmi.check(L.zkmi_ntt_dev(c, x.ptr, X.ptr, lg, 0, None, None))
        out = np.zeros(32, np.uint8)
        bad = []
        for k in ks:
            at = mont(pow(w, k, r))
            zkmi.check(L.zkmi_poly_evaluate_dev(c, x.ptr, n, zkmi.ptr(at), zkmi.ptr(out)))
            if element(X, k) != bytes(out):
                bad.append(k)
        assert not bad, ("fft of generator-drawn data: outputs differ from the evaluation at w^k", name, lg, plan, bad)
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name,lg,with_padding_and_random", [("bn128", 25, True), ("bls12381", 25, True), ("bn128", 26, False)])
def test_four_passes_real_sizes_closed_form(name, lg, with_padding_and_random):
    run_real_size(name, lg, with_padding_and_random)
