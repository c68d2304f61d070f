"""Writes the inputs of the wtns.check golden cases: tests/golden/wtns_check_<curve>_*.r1cs / .wtns (snarkjs_amd/workloads/synth_r1cs.py: satisfiable_circuit)
and tests/golden/wtns_check_cases.json, the list tools/gen_wtns_check_golden.js runs the reference over. Run before it:  python tools/gen_wtns_check_r1cs.py"""
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from snarkjs_amd.workloads import synth_r1cs as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
OTHER = {"bn128": "bls12381", "bls12381": "bn128"}
ODD_PRIME = (1 << 255) - 19          # a prime that is the scalar field of neither curve
cases, written = [], {}


def put(name, data):
    assert len(data) < 64 * 1024, (name, len(data))
    if written.get(name) != data:
        assert name not in written, name
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        written[name] = data
    return name


def resection(data, typ, f):
    """the file with section `typ` replaced by f(section)"""
    n = struct.unpack_from("<I", data, 8)[0]
    out, off = bytearray(data[:12]), 12
    for _ in range(n):
        t, ln = struct.unpack_from("<IQ", data, off)
        sec = data[off + 12:off + 12 + ln]
        if t == typ:
            sec = f(sec)
        out += struct.pack("<IQ", t, len(sec)) + sec
        off += 12 + ln
    return bytes(out)


def solved(cons, i):
    """the signal constraint i solves: the newest one of its C"""
    return max(s for s, _ in cons[i][2])


def other_semantics_fail(curve, cons, wit):
    """some constraint fails when a repeated signal keeps its FIRST coefficient, and some when the coefficients add up"""
    r = S.R[curve]

    def ev(lc, how):
        d = {}
        for s, c in lc:
            d[s] = d.get(s, 0) + c if how == "sum" else d.get(s, c)
        return sum(c * wit[s] for s, c in d.items()) % r
    return all(any(ev(a, how) * ev(b, how) % r != ev(c, how) for a, b, c in cons) for how in ("first", "sum"))


for curve in ("bn128", "bls12381"):
    r = S.R[curve]
    stem = f"wtns_check_{curve}_"

    def case(name, r1cs, wtns, what, reads_past=False):
        """reads_past: the reference reads beyond a buffer there; what it then returns comes from stale memory, or it throws"""
        cases.append(dict(name=f"{curve}_{name}", curve=curve, r1cs=r1cs, wtns=wtns, what=what, readsPast=reads_past))

    nv, no, ni, cons, wit = S.satisfiable_circuit(curve, 13)
    base = put(stem + "base.r1cs", S.write_r1cs(curve, nv, no, ni, cons))
    good = put(stem + "good.wtns", S.write_wtns(curve, wit))
    case("good", base, good, "a good witness")

    def spoiled(*signals):
        w = list(wit)
        for s in signals:
            w[s] = (w[s] + 1) % r
        return w
    case("bad_first", base, put(stem + "bad_first.wtns", S.write_wtns(curve, spoiled(solved(cons, 0)))), "one bad value at the first constraint")
    case("bad_last", base, put(stem + "bad_last.wtns", S.write_wtns(curve, spoiled(solved(cons, 12)))), "one bad value at the last constraint")
    case("bad_two", base, put(stem + "bad_two.wtns", S.write_wtns(curve, spoiled(solved(cons, 12), solved(cons, 9)))), "bad values at constraints 9 and 12: 9 is reported")
    case("wide_witness", base, put(stem + "wide_witness.wtns", S.write_wtns(curve, [v + r * (1 + i % (((1 << 256) - 1 - v) // r)) if i % 2 else v for i, v in enumerate(wit)])),
         "witness values in [r, 2^256)")
    case("other_curve_witness", base, put(stem + "other_curve.wtns", S.write_wtns(OTHER[curve], wit)), "a witness of the other curve")

    dv, do, di, dcons, dwit = S.satisfiable_circuit(curve, 12, seed=0xd0b, dups=True)
    assert other_semantics_fail(curve, dcons, dwit)
    case("dups", put(stem + "dups.r1cs", S.write_r1cs(curve, dv, do, di, dcons)), put(stem + "dups.wtns", S.write_wtns(curve, dwit)),
         "signals named twice, adjacent and apart: the last coefficient counts")
    dbad = list(dwit)
    dbad[solved(dcons, 6)] = (dbad[solved(dcons, 6)] + 5) % r
    case("dups_bad", stem + "dups.r1cs", put(stem + "dups_bad.wtns", S.write_wtns(curve, dbad)), "the same with a bad value at constraint 6")

    desc = [tuple(sorted(lc, key=lambda t: -t[0]) for lc in c) for c in cons]
    case("descending", put(stem + "descending.r1cs", S.write_r1cs(curve, nv, no, ni, desc)), good, "signal ids in descending order")

    top = (1 << 256) - 1
    hand = [([(1, r)], [(2, 1)], []),                                          # r = 0
            ([(1, r + 3)], [(0, 1)], [(4, 1)]),                                # r + 3 = 3
            ([(1, top)], [(0, 1)], [(5, 1)]),                                  # 2^256 - 1
            ([(1, r + 3), (2, top)], [(3, r - 1), (0, r)], [(6, top), (0, 0)])]
    hw = [1, 7, 11, 13, 0, 0, 0]
    hw[4] = 3 * hw[1] % r
    hw[5] = top % r * hw[1] % r
    hw[6] = (3 * hw[1] + top * hw[2]) * ((r - 1) * hw[3]) * pow(top % r, -1, r) % r
    wide = put(stem + "wide.r1cs", S.write_r1cs(curve, 7, 1, 1, hand))
    case("wide_coefs", wide, put(stem + "wide.wtns", S.write_wtns(curve, hw)), "coefficients of r, r + 3 and 2^256 - 1")
    hb = list(hw)
    hb[5] = (hb[5] + 1) % r
    case("wide_coefs_bad", wide, put(stem + "wide_bad.wtns", S.write_wtns(curve, hb)), "the same with a bad value at constraint 2")

    zv, zo, zi, zcons, zwit = S.satisfiable_circuit(curve, 9, seed=0x20, w0=2)
    case("w0_is_2", put(stem + "w0.r1cs", S.write_r1cs(curve, zv, zo, zi, zcons)), put(stem + "w0.wtns", S.write_wtns(curve, zwit)), "w[0] = 2")

    empty = cons[:5] + [([], [], [])] + cons[5:]
    case("empty_constraint", put(stem + "empty.r1cs", S.write_r1cs(curve, nv, no, ni, empty)), good, "an all-empty constraint among the others")
    case("zero_constraints", put(stem + "zero.r1cs", S.write_r1cs(curve, 3, 1, 1, [])), put(stem + "zero.wtns", S.write_wtns(curve, [1, 5, 6])), "zero constraints")

    base_bytes = written[base]
    case("trailing", put(stem + "trailing.r1cs", resection(base_bytes, 2, lambda s: s + bytes(range(1, 42)))), good, "41 bytes after the last constraint of section 2")
    case("trailing_bad", stem + "trailing.r1cs", stem + "bad_last.wtns", "the same with a bad value at the last constraint")
    case("truncated", put(stem + "truncated.r1cs", resection(base_bytes, 2, lambda s: s[:-10])), good, "section 2 ends 10 bytes early, inside the last coefficient", True)
    case("truncated_count", put(stem + "truncated_count.r1cs", resection(base_bytes, 2, lambda s: s[:4 + 36 * len(cons[0][0]) + 2])), good,
         "section 2 ends inside the second term count", True)
    beyond = cons[:12] + [(cons[12][0] + [(nv, 1)], cons[12][1], cons[12][2])]
    case("signal_beyond", put(stem + "beyond.r1cs", S.write_r1cs(curve, nv, no, ni, beyond)), good, "the last constraint names signal nVars", True)

    odd = resection(base_bytes, 1, lambda s: s[:4] + ODD_PRIME.to_bytes(32, "little") + s[36:])
    case("odd_prime", put(stem + "odd_prime.r1cs", odd), put(stem + "odd_prime.wtns", S.write_wtns(curve, wit, prime=ODD_PRIME)), "an r1cs and a witness over 2^255 - 19")
    case("odd_prime_r1cs_only", stem + "odd_prime.r1cs", good, "an r1cs over 2^255 - 19 with a witness of the curve")

with open(os.path.join(OUT, "wtns_check_cases.json"), "w") as f:
    json.dump(cases, f, indent=1)
    f.write("\n")
print(len(cases), "cases,", len(written), "files,", sum(len(v) for v in written.values()), "bytes")
