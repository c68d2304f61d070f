"""wtns.check restated literally in Python integers (reference src/wtns_check.js: readLC, EvaluateLinearCombination, getWitnessValue and the loop), the
readers the tests need beside it, and the golden cases of tests/golden/wtns_check_golden.json (tools/gen_wtns_check_r1cs.py, tools/gen_wtns_check_golden.js).
The restatement is the reference of the CPU and GPU tests; the golden file, written by the unmodified reference, pins the restatement."""
import json
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
R = {
    "bn128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12381": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
}
CURVE_OF_R = {v: k for k, v in R.items()}
NONE = 0xFFFFFFFF


def sections(data, magic):
    assert data[:4] == magic
    n = struct.unpack_from("<I", data, 8)[0]
    off, out = 12, {}
    for _ in range(n):
        typ, ln = struct.unpack_from("<IQ", data, off)
        out.setdefault(typ, (off + 12, ln))
        off += 12 + ln
    return out


def read_r1cs(data):
    """header fields and the bytes of section 2"""
    s = sections(data, b"r1cs")
    off = s[1][0]
    n8 = struct.unpack_from("<I", data, off)[0]
    prime = int.from_bytes(data[off + 4:off + 4 + n8], "little")
    n_vars, n_out, n_pub, n_prv, n_labels, n_c = struct.unpack_from("<IIIIQI", data, off + 4 + n8)
    return dict(n8=n8, prime=prime, nVars=n_vars, nOutputs=n_out, nPubInputs=n_pub, nPrvInputs=n_prv, nLabels=n_labels, nConstraints=n_c,
                constraints=bytes(data[s[2][0]:s[2][0] + s[2][1]]))


def read_wtns(data):
    s = sections(data, b"wtns")
    off = s[1][0]
    n8 = struct.unpack_from("<I", data, off)[0]
    q = int.from_bytes(data[off + 4:off + 4 + n8], "little")
    return dict(n8=n8, q=q, nWitness=struct.unpack_from("<I", data, off + 4 + n8)[0], witness=bytes(data[s[2][0]:s[2][0] + s[2][1]]))


class PastTheEnd(Exception):
    """the loop read beyond the constraint section or the witness (the reference's behaviour there is recorded in the golden file, not restated)"""


def first_bad(constraints, n_constraints, r, witness, n8=32):
    """the reference's loop: index of the first constraint with evalA * evalB - evalC != 0, None when all hold"""
    pos = 0

    def read_lc():
        nonlocal pos
        if pos + 4 > len(constraints):
            raise PastTheEnd("count")
        n = struct.unpack_from("<I", constraints, pos)[0]
        pos += 4
        if pos + (4 + n8) * n > len(constraints):
            raise PastTheEnd("records")
        lc = {}
        for i in range(n):
            idx = struct.unpack_from("<I", constraints, pos + i * (4 + n8))[0]
            lc[idx] = int.from_bytes(constraints[pos + i * (4 + n8) + 4:pos + (i + 1) * (4 + n8)], "little") % r        # lc[idx] = val: the last one stays
        pos += (4 + n8) * n
        return lc

    def value(signal):
        if (signal + 1) * n8 > len(witness):
            raise PastTheEnd("witness")
        return int.from_bytes(witness[signal * n8:(signal + 1) * n8], "little") % r

    def evaluate(lc):
        res = 0
        for signal, factor in lc.items():
            res = (res + value(signal) * factor) % r
        return res

    for i in range(n_constraints):
        a, b, c = read_lc(), read_lc(), read_lc()
        if (evaluate(a) * evaluate(b) - evaluate(c)) % r != 0:
            return i
    return None


def first_bad_files(r1cs_bytes, wtns_bytes):
    r1, w = read_r1cs(r1cs_bytes), read_wtns(wtns_bytes)
    return first_bad(r1["constraints"], r1["nConstraints"], r1["prime"], w["witness"], r1["n8"])


class RestatedDevice:
    """snarkjs_amd.wtns_check.Device with the restatement in place of the library"""

    def __init__(self):
        self.loaded, self.calls = {}, []

    def load(self, curve, constraints, n_constraints, n_vars):
        from snarkjs_amd import wtns_check
        self.calls.append("load")
        cons = b"".join(bytes(p) for p in constraints) if isinstance(constraints, (list, tuple)) else bytes(constraints)
        try:                                                       # what zkmi_r1cs_load refuses
            pos = 0
            for _ in range(3 * n_constraints):
                if pos + 4 > len(cons):
                    raise PastTheEnd
                n = struct.unpack_from("<I", cons, pos)[0]
                if pos + 4 + 36 * n > len(cons):
                    raise PastTheEnd
                if any(struct.unpack_from("<I", cons, pos + 4 + 36 * i)[0] >= n_vars for i in range(n)):
                    raise PastTheEnd
                pos += 4 + 36 * n
        except PastTheEnd:
            raise wtns_check.DeviceRefusal("r1cs_load: refused")
        key = len(self.loaded) + 1
        self.loaded[key] = (R[curve], cons, n_constraints, n_vars)
        return key

    def check(self, key, witnesses, n_witnesses):
        self.calls.append("check")
        r, cons, n_c, n_vars = self.loaded[key]
        w = bytes(witnesses)
        assert len(w) == n_witnesses * n_vars * 32
        out = []
        for k in range(n_witnesses):
            bad = first_bad(cons, n_c, r, w[k * n_vars * 32:(k + 1) * n_vars * 32])
            out.append(NONE if bad is None else bad)
        return out

    def release(self, key):
        self.calls.append("release")
        self.loaded.pop(key, None)


def golden():
    with open(os.path.join(GOLDEN, "wtns_check_golden.json")) as f:
        return json.load(f)["cases"]


def golden_file(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


class Recorder:
    """a logger that keeps [level, text] pairs, as the golden file has them"""

    def __init__(self):
        self.lines = []

    def debug(self, t):
        pass

    def info(self, t):
        self.lines.append(["info", t])

    def warn(self, t):
        self.lines.append(["warn", t])

    def error(self, t):
        self.lines.append(["error", t])
