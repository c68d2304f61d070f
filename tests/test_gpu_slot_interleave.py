"""Two different users of ONE pipeline slot, interleaved (csrc/msm_host.hpp: msm_multi_pending, csrc/msm_sort.hip: msm_job_slot, csrc/groth16.hip: g16_enqueue).

An enqueued zkmi_msm_table_multi call and a submitted Groth16 proof leave their window sums in the slot's pinned host memory until their collect folds them. Every cell of
the matrix puts such work into slot s, runs an intruder X on the same slot, then collects. The property: X is either refused (non-zero rc, zkmi_last_error() names the busy
slot) and the pending work then collects to its exact value, or X succeeds and BOTH answers are exact. Never rc == 0 with wrong bytes on either side.

Expected values involve nothing of the library: the bases are k_i * G with known k_i (tests/msm_patterns.py), so every MSM is (sum s_i k_i mod r) * G in Python integers and one
scalar multiplication of the CPU oracle; the pending Groth16 proof is the reference's own seeded proof of tests/golden/groth16_bn128_n1024.json, the intruding one (another
resident key, another witness, other blinding values) the CPU oracle's. Every MSM draws its scalars from a seed of its own, so a swapped answer cannot equal the right one.
Shapes are the smallest at which the mechanism exists: 2^11 BN254 G1 points (c = 11), 2^10 BLS12-381 G2 points for the check that a collect belongs to the table that was
enqueued."""
import ctypes as C
import itertools
import json
import os
import types

import numpy as np
import pytest

import msm_patterns as P
import oracle_lib as O
import synth
from test_gpu_msm_widths import affine_of, build_table, logs, make_bases, order

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLES = {"g1": ("bn128", 1, 1 << 11), "g2": ("bls12381", 2, 1 << 10)}
_seed = itertools.count(0x51070000)


@pytest.fixture(scope="module")
def env():
    from snarkjs_amd import binfile, groth16, zkmi
    zkmi.init(0)
    e = types.SimpleNamespace(L=zkmi.lib(), zkmi=zkmi, groth16=groth16, tab={}, bases={}, pending={})
    for tag, (name, group, n) in TABLES.items():
        e.bases[tag] = make_bases(name, group, "geometric", n)
        e.tab[tag] = build_table(name, group, e.bases[tag], n)
    e.g = json.load(open(os.path.join(GOLDEN, "groth16_bn128_n1024.json")))
    zkey = open(os.path.join(GOLDEN, "groth16_bn128_n1024.zkey"), "rb").read()
    e.w = zkmi.u8(binfile.read_wtns(open(os.path.join(GOLDEN, "groth16_bn128_n1024.wtns"), "rb").read())["witness"]).copy()
    e.d_w = zkmi.DeviceBuffer.from_host(e.w)
    e.r, e.s = np.frombuffer(bytes.fromhex(e.g["r_mont"]), np.uint8).copy(), np.frombuffer(bytes.fromhex(e.g["s_mont"]), np.uint8).copy()
    e.pk, e.pk2 = groth16.ProvingKey(zkey), groth16.ProvingKey(zkey)          # the pending proof's key, and a second resident key for the Groth16 intruders
    # the intruders prove ANOTHER witness with other blinding values, so that their window sums differ from the pending proof's; expected: the CPU oracle's proof
    e.w2 = e.w.copy()
    e.w2[32 * 7:32 * 8] = np.frombuffer((int.from_bytes(synth.elems(5, 1).tobytes(), "little") % order("bn128")).to_bytes(32, "little"), np.uint8)
    e.d_w2 = zkmi.DeviceBuffer.from_host(e.w2)
    e.r2, e.s2 = zkmi.u8(O.fr_e(O.BN128, 21)).copy(), zkmi.u8(O.fr_e(O.BN128, 34)).copy()
    e.want2 = [bytes(x) for x in O.groth16_prove(O.BN128, binfile.read_groth16_zkey(zkey), e.w2, bytes(e.r2), bytes(e.s2))]
    e.host_bases = e.bases["g1"].to_host()
    yield e
    drain(e)
    e.pk.release(); e.pk2.release(); e.d_w.free(); e.d_w2.free()
    for tag in TABLES:
        e.L.zkmi_msm_table_release(e.tab[tag])
        e.bases[tag].free()


def drain(e):
    """leave both slots empty whatever a failed cell left behind"""
    for slot, (tag, count) in list(e.pending.items()):
        e.L.zkmi_pipeline_select(slot)
        e.L.zkmi_msm_table_multi_collect(e.tab[tag], count, e.zkmi.ptr(np.zeros(count * 288, np.uint8)))
    e.pending.clear()
    e.L.zkmi_groth16_reset(e.pk.key); e.L.zkmi_groth16_reset(e.pk2.key)
    e.L.zkmi_pipeline_select(0)


# ---- one MSM call (1 to 4 MSMs against one table) with its closed forms ----------------------------------------------------------------------------------
class Msms:
    def __init__(self, e, count, tag="g1"):
        name, group, n = TABLES[tag]
        self.e, self.tag, self.count, self.name, self.group = e, tag, count, name, group
        self.ks = [n, n - 3, 77, n - 1][:count]
        self.sc = [P.scalars("uniform", 0, n, 32, seed=next(_seed)) for _ in range(count)]
        self.dev = [e.zkmi.DeviceBuffer.from_host(s) for s in self.sc]
        self.pj = 3 * group * O.n8q(O.CURVE_ID[name])
        self.p, self.k = (C.c_void_p * count)(*[d.ptr for d in self.dev]), (C.c_size_t * count)(*self.ks)
        self.out = np.full(count * self.pj, 0xA5, np.uint8)

    def want(self, i):
        name, group, n = TABLES[self.tag]
        return affine_of(name, group, P.closed_form(self.sc[i], 32, logs("geometric", n, name), order(name), self.ks[i]))

    def wrong(self):
        """indices whose output is not the closed form"""
        cid = O.CURVE_ID[self.name]
        return [i for i in range(self.count) if not np.array_equal(O.to_affine(cid, self.group, self.out[i * self.pj:(i + 1) * self.pj]), self.want(i))]

    def enqueue(self, slot):
        e = self.e
        e.zkmi.check(e.L.zkmi_pipeline_select(slot))
        rc = e.L.zkmi_msm_table_multi_enqueue_dev(e.tab[self.tag], self.p, self.k, self.count, 32)
        if rc == 0:
            e.pending[slot] = (self.tag, self.count)
        return rc

    def collect(self, slot, tag=None, count=None):
        e = self.e
        e.zkmi.check(e.L.zkmi_pipeline_select(slot))
        rc = e.L.zkmi_msm_table_multi_collect(e.tab[tag or self.tag], self.count if count is None else count, e.zkmi.ptr(self.out))
        if rc == 0:
            e.pending.pop(slot, None)
        return rc

    def free(self):
        for d in self.dev:
            d.free()


def proof_of(e, pk, pts):
    return e.groth16.raw_to_proof(pk, *pts)


def busy_message(e, slot):
    return b"pipeline slot %d holds work in flight" % slot in e.L.zkmi_last_error()


# ---- what occupies the slot --------------------------------------------------------------------------------------------------------------------------------
class PendingMulti:
    def __init__(self, e, slot, count, tag="g1"):
        self.e, self.slot, self.m = e, slot, Msms(e, count, tag)
        e.zkmi.check(self.m.enqueue(slot))

    def finish(self):
        """collect -> what came back wrong (empty: exact)"""
        self.e.zkmi.check(self.m.collect(self.slot))
        bad = self.m.wrong()
        self.m.free()
        return [("pending multi-MSM", i) for i in bad]


class PendingProof:
    def __init__(self, e, slot):
        self.e, self.slot = e, slot
        e.pk.submit(e.d_w.ptr, slot)

    def finish(self):
        e = self.e
        got = proof_of(e, e.pk, e.pk.collect(self.slot, e.r, e.s))
        return [] if got == e.g["proof"] else [("pending Groth16 proof", got)]


STATES = {"multi1": lambda e, s: PendingMulti(e, s, 1), "multi2": lambda e, s: PendingMulti(e, s, 2), "multi4": lambda e, s: PendingMulti(e, s, 4),
          "groth16": lambda e, s: PendingProof(e, s)}


# ---- the intruders: each runs on `slot` and returns (rc, finish); finish() completes a call that succeeded and returns what is wrong with ITS answer ----------
def x_table_dev(e, slot):
    m = Msms(e, 1)
    e.zkmi.check(e.L.zkmi_pipeline_select(slot))
    rc = e.L.zkmi_msm_table_dev(e.tab["g1"], m.dev[0].ptr, m.ks[0], 32, e.zkmi.ptr(m.out))
    return rc, lambda: [("zkmi_msm_table_dev", i) for i in m.wrong()]


def x_msm_dev(e, slot):
    m = Msms(e, 1)
    e.zkmi.check(e.L.zkmi_pipeline_select(slot))
    rc = e.L.zkmi_msm_dev(0, 1, e.bases["g1"].ptr, m.dev[0].ptr, m.ks[0], 32, e.zkmi.ptr(m.out))
    return rc, lambda: [("zkmi_msm_dev", i) for i in m.wrong()]


def x_msm_host(e, slot):
    m = Msms(e, 1)
    e.zkmi.check(e.L.zkmi_pipeline_select(slot))
    b, s = e.zkmi.pages_of(e.host_bases), e.zkmi.pages_of(m.sc[0])
    rc = e.L.zkmi_msm(0, 1, b.pages, s.pages, m.ks[0], 32, 0, e.zkmi.ptr(m.out))
    return rc, lambda: [("zkmi_msm", i) for i in m.wrong()]


def x_multi_dev(e, slot):
    m = Msms(e, 2)
    e.zkmi.check(e.L.zkmi_pipeline_select(slot))
    rc = e.L.zkmi_msm_table_multi_dev(e.tab["g1"], m.p, m.k, 2, 32, e.zkmi.ptr(m.out))
    return rc, lambda: [("zkmi_msm_table_multi_dev", i) for i in m.wrong()]


def x_groth16_prove(e, slot):
    """the one-call proof with a host witness: it runs in slot 0 whichever slot is active (csrc/groth16.hip: g16_prove_host)"""
    q = 32
    pts = [np.zeros(2 * q, np.uint8), np.zeros(4 * q, np.uint8), np.zeros(2 * q, np.uint8)]
    e.zkmi.check(e.L.zkmi_pipeline_select(slot))
    rc = e.L.zkmi_groth16_prove(None, e.pk2.key, e.zkmi.ptr(e.w2), e.w2.size, e.zkmi.ptr(e.r2), e.zkmi.ptr(e.s2), *[e.zkmi.ptr(x) for x in pts])
    return rc, lambda: [] if [bytes(x) for x in pts] == e.want2 else [("zkmi_groth16_prove",)]


def x_groth16_submit(e, slot):
    rc = e.L.zkmi_groth16_submit(e.pk2.key, e.zkmi.ptr(e.w2), e.w2.size, slot)
    return rc, lambda: [] if [bytes(x) for x in e.pk2.collect(slot, e.r2, e.s2)] == e.want2 else [("zkmi_groth16_submit + collect",)]


def x_multi_enqueue(e, slot):
    m = Msms(e, 2)
    rc = m.enqueue(slot)

    def finish():
        e.zkmi.check(m.collect(slot))
        return [("zkmi_msm_table_multi_enqueue_dev + collect", i) for i in m.wrong()]
    return rc, finish


INTRUDERS = {"msm_table_dev": x_table_dev, "msm_dev": x_msm_dev, "msm": x_msm_host, "msm_table_multi_dev": x_multi_dev, "groth16_prove": x_groth16_prove,
             "groth16_submit": x_groth16_submit, "multi_enqueue": x_multi_enqueue}
# a multi enqueue over a pending multi call is not an intruder: it DROPS the abandoned call (tests/test_gpu_groth16_build.py pins that)
CELLS = [(st, x) for st in STATES for x in INTRUDERS if not (x == "multi_enqueue" and st != "groth16")]


def usable(e, slot):
    """after a refusal: a plain enqueue + collect and a Groth16 proof in this slot are exact"""
    m = Msms(e, 1)
    e.zkmi.check(m.enqueue(slot)); e.zkmi.check(m.collect(slot))
    bad = [("enqueue + collect after the refusal", i) for i in m.wrong()]
    m.free()
    e.pk2.submit(e.d_w2.ptr, slot)
    if [bytes(x) for x in e.pk2.collect(slot, e.r2, e.s2)] != e.want2:
        bad.append(("Groth16 proof after the refusal",))
    return bad


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("state,intruder", CELLS)
def test_intruder_on_the_busy_slot(env, slot, state, intruder):
    """work pending in `slot`, X on the same slot, then the collect: refused and the pending work exact, or both exact"""
    e = env
    try:
        pend = STATES[state](e, slot)
        rc, finish_x = INTRUDERS[intruder](e, slot)
        print(f"{state} pending in slot {slot}, {intruder}: rc {rc} {e.L.zkmi_last_error() if rc else b''!r}")
        if rc != 0:
            # zkmi_groth16_prove runs in slot 0: with the work pending in slot 1 nothing is in its way
            assert not (intruder == "groth16_prove" and slot == 1), e.L.zkmi_last_error()
            assert rc == 2 and busy_message(e, slot), (rc, e.L.zkmi_last_error())
            bad = pend.finish()
            assert not bad, ("the refused call disturbed what was pending", bad)
            bad = usable(e, slot)
            assert not bad, bad
        else:
            bad = finish_x() + pend.finish()
            assert not bad, ("rc == 0 with wrong bytes", bad)
    finally:
        drain(e)


# zkmi_groth16_prove always runs in slot 0: it is in "the other slot" only with the work pending in slot 1
OTHER_SLOT_CELLS = [(st, x, slot) for st, x in CELLS if st in ("multi2", "groth16") for slot in (0, 1) if not (x == "groth16_prove" and slot == 0)]


@pytest.mark.parametrize("state,intruder,slot", OTHER_SLOT_CELLS)
def test_intruder_on_the_other_slot(env, state, intruder, slot):
    """the same calls with X in the OTHER slot: nothing is refused and both answers are exact"""
    e = env
    try:
        pend = STATES[state](e, slot)
        rc, finish_x = INTRUDERS[intruder](e, 1 - slot)
        assert rc == 0, e.L.zkmi_last_error()
        bad = finish_x() + pend.finish()
        assert not bad, bad
    finally:
        drain(e)


# ---- controls: calls that take no job slot stay allowed between enqueue and collect, and exact ------------------------------------------------------------
def _mont(v, r):
    return np.frombuffer(((v << 256) % r).to_bytes(32, "little"), np.uint8).copy()


def ctl_ntt(e):
    x = synth.elems(next(_seed), 1 << 10)
    d = e.zkmi.DeviceBuffer.from_host(x)
    out = e.zkmi.DeviceBuffer(x.size)
    e.zkmi.check(e.L.zkmi_ntt_dev(0, d.ptr, out.ptr, 10, 0, None, None))
    got = out.to_host()
    d.free(); out.free()
    return np.array_equal(got, O.ntt(O.BN128, x))


def ctl_fr_batch(e):
    x = synth.elems(next(_seed), 1000)
    d = e.zkmi.DeviceBuffer.from_host(x)
    e.zkmi.check(e.L.zkmi_fr_batch_dev(0, e.zkmi.BATCH_TO_MONTGOMERY, d.ptr, d.ptr, 1000))
    got = d.to_host()
    d.free()
    return np.array_equal(got, O.to_mont(O.BN128, x))


def ctl_poly(e):
    """zkmi_poly_scale_dev then zkmi_poly_evaluate_dev on 777 Montgomery coefficients, against Horner in Python integers"""
    r, n = order("bn128"), 777
    a = [v % r for v in P.ints(synth.elems(next(_seed), n), 32)]
    k, x = [v % r for v in P.ints(synth.elems(next(_seed), 2), 32)]
    d = e.zkmi.DeviceBuffer.from_host(np.concatenate([_mont(v, r) for v in a]))
    out = np.zeros(32, np.uint8)
    e.zkmi.check(e.L.zkmi_poly_scale_dev(0, d.ptr, n, e.zkmi.ptr(_mont(k, r))))
    e.zkmi.check(e.L.zkmi_poly_evaluate_dev(0, d.ptr, n, e.zkmi.ptr(_mont(x, r)), e.zkmi.ptr(out)))
    d.free()
    want = 0
    for v in reversed(a):
        want = (want * x + v * k) % r
    return bytes(out) == bytes(_mont(want, r))


def ctl_to_affine(e):
    """zkmi_to_affine of a Jacobian point the CPU oracle made (k G, Z != 1) against the oracle's own normalisation"""
    k = int.from_bytes(synth.elems(next(_seed), 1).tobytes(), "little") % order("bn128")
    jac = np.ascontiguousarray(O.generator_mul(O.BN128, 1, k))
    aff = np.zeros(64, np.uint8)
    e.zkmi.check(e.L.zkmi_to_affine(0, 1, e.zkmi.ptr(jac), e.zkmi.ptr(aff)))
    return np.array_equal(aff, affine_of("bn128", 1, k))


def ctl_verify_many(e):
    import verify_vectors as V
    from snarkjs_amd import groth16_verify
    vk, pubs, proof = V.golden("groth16_bn128_n1024.json")
    key = groth16_verify.VerifyingKey(vk)
    off = [str(int(pubs[0]) + 1)] + list(pubs[1:])               # the golden proof does not hold for other public signals
    try:
        return key.verify_many([pubs] * 64 + [off] + [pubs], [proof] * 66) == [True] * 64 + [False, True]
    finally:
        key.release()


CONTROLS = {"ntt_dev": ctl_ntt, "fr_batch_dev": ctl_fr_batch, "poly_scale_evaluate": ctl_poly, "to_affine": ctl_to_affine, "verify_many": ctl_verify_many}


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("state", ["multi4", "groth16"])
def test_calls_without_job_slots_stay_allowed(env, slot, state):
    """zkmi_ntt_dev, zkmi_fr_batch_dev, zkmi_poly_*, zkmi_to_affine and a verify batch between enqueue and collect in the same slot (PLONK's rounds rely on it): each exact
    against the CPU oracle or Python integers, and the pending work exact afterwards"""
    e = env
    try:
        pend = STATES[state](e, slot)
        e.zkmi.check(e.L.zkmi_pipeline_select(slot))
        bad = [name for name, f in CONTROLS.items() if not f(e)]
        e.zkmi.check(e.L.zkmi_pipeline_select(slot))
        assert not bad and not pend.finish(), bad
    finally:
        drain(e)


@pytest.mark.parametrize("slot", [0, 1])
def test_collect_belongs_to_the_table_that_was_enqueued(env, slot):
    """two MSMs enqueued on the BLS12-381 G2 table: an intruder is refused, a collect through the BN254 G1 table (same count) or with another count fails with the
    existing message and leaves the call in place, the right collect is exact; and the enqueue that drops an abandoned call is exact too"""
    e = env
    try:
        m = Msms(e, 2, "g2")
        e.zkmi.check(m.enqueue(slot))
        rc, finish_x = x_table_dev(e, slot)
        assert rc == 0 or busy_message(e, slot), e.L.zkmi_last_error()
        bad_x = finish_x() if rc == 0 else []
        assert m.collect(slot, tag="g1") != 0 and b"does not match" in e.L.zkmi_last_error()
        assert m.collect(slot, count=1) != 0 and b"does not match" in e.L.zkmi_last_error()
        e.zkmi.check(m.collect(slot))
        assert not bad_x and not m.wrong(), (bad_x, m.wrong())
        assert m.collect(slot) != 0 and b"nothing enqueued" in e.L.zkmi_last_error()
        abandoned, kept = Msms(e, 4), Msms(e, 1, "g2")
        e.zkmi.check(abandoned.enqueue(slot)); e.zkmi.check(kept.enqueue(slot)); e.zkmi.check(kept.collect(slot))
        assert not kept.wrong()
    finally:
        drain(e)


def test_slots_are_free_after_a_failed_prove_many(env):
    """plonk.prove_many gives a proof up between the two halves of a round's commitments when the other proof fails (snarkjs_amd/plonk.py: run_many): the driver collects what
    was left enqueued, so neither slot stays busy — an MSM and a Groth16 proof in each slot are accepted and exact"""
    from snarkjs_amd import plonk
    e = env
    zkey, wtns = (open(os.path.join(GOLDEN, "plonk_bn128_small." + ext), "rb").read() for ext in ("zkey", "wtns"))
    bad = bytearray(wtns)
    bad[-32] ^= 1
    key = plonk.PlonkKey(zkey)
    try:
        with pytest.raises(Exception) as ei:
            plonk.prove_many(key, [wtns, bytes(bad), wtns, wtns])
        assert any(m in str(ei.value) for m in ("Copy constraints does not match", "not divisible", "not well calculated")), str(ei.value)
        for slot in (0, 1):
            rc, finish_x = x_table_dev(e, slot)
            assert rc == 0 and not finish_x(), (slot, e.L.zkmi_last_error())
            assert not PendingProof(e, slot).finish(), slot
    finally:
        key.release()
        drain(e)
