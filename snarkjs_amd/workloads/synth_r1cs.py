"""Synthetic .r1cs files (iden3 r1cs binary format, r1csfile) for the Groth16 setup: the fixtures under tests/golden/setup_*, the closed-form
test and tools/setupbench.py. A constraint is three linear combinations (A, B, C), each a list of (signal, coefficient) in file order; nothing
here needs the constraints to be satisfiable: newZKey never looks at a witness.
"""
import random
import struct

R = {
    "bn128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "bls12381": 52435875175126190479447740508185965837690552500527637822603658699938581184513,
}
SETUP_SEG = 32          # csrc/groth16_setup.cuh


def write_r1cs(curve, n_vars, n_outputs, n_pub_inputs, constraints):
    """bytes of an .r1cs file; constraints: list of (A, B, C), each a list of (signal, coefficient as a non-negative integer below 2^256)"""
    body = bytearray()
    for lcs in constraints:
        for lc in lcs:
            body += struct.pack("<I", len(lc))
            for s, v in lc:
                body += struct.pack("<I", s) + int(v).to_bytes(32, "little")
    n_prv = n_vars - 1 - n_outputs - n_pub_inputs
    head = struct.pack("<I", 32) + R[curve].to_bytes(32, "little") + struct.pack("<IIIIQI", n_vars, n_outputs, n_pub_inputs, n_prv, n_vars, len(constraints))
    labels = b"".join(struct.pack("<Q", i) for i in range(n_vars))
    out = bytearray(b"r1cs" + struct.pack("<II", 1, 3))
    for typ, sec in ((1, head), (2, bytes(body)), (3, labels)):
        out += struct.pack("<IQ", typ, len(sec)) + sec
    return bytes(out)


def edge_circuit(curve):
    """cirPower 7, nPublic 2: every corner of the column evaluation (see the comments); (n_vars, n_outputs, n_pub_inputs, constraints)"""
    r = R[curve]
    rng = random.Random(0x5e7 + len(curve))
    wide = [rng.randrange(1 << 200, r) for _ in range(2)]            # two seeded full-width values
    n_c, n_vars = 110, 12
    cons = []
    for c in range(n_c):
        a, b, cc = [], [], []
        if c < 3 * SETUP_SEG + 4:                                        # signal 3: one column of 3 SEG + 4 terms in A (cut into four segments), mixed widths
            a.append((3, [1, r - 1, 2, 1 << 253, 1, wide[0], 1, 5, r - 2][c % 9]))
        a.append((11, 1 + (c % 3)))
        b.append((11 if c % 2 else 0, 1 if c % 4 else r - 1))
        cc.append((10, 1))
        cons.append([a, b, cc])
    cons[0][0].append((1, 1)); cons[0][1].append((1, r - 1)); cons[0][2].append((1, 2))        # the public signal 1 in A, B and C
    cons[1][0].append((2, 7))                                                                  # the public signal 2 in A only
    cons[2][0].append((4, 3)); cons[2][2].append((4, 1))                                       # signal 4: absent from B
    #                                                                                            signal 5: absent from every matrix
    cons[3][0].append((6, 1)); cons[4][1].append((6, r - 1))                                   # signal 6: single-term columns
    cons[5][0] += [(7, 1), (7, 1)]; cons[5][1] += [(7, 1), (7, 1)]                             # signal 7 twice with 1 and 1: base + base (doubling)
    cons[6][0] += [(8, 1), (8, r - 1)]; cons[6][1] += [(8, 1), (8, r - 1)]                     # signal 8 twice with 1 and r - 1: sums to infinity
    cons[7][0] += [(9, 2), (9, 0)]; cons[7][1] += [(9, 1 << 253)]; cons[7][2] += [(9, wide[1])]      # signal 9: 2, 0, 2^253, full width
    cons[8][1].append((10, wide[0])); cons[9][0].append((10, 0))                               # signal 10: a column that holds only a zero coefficient in A
    return n_vars, 1, 1, cons


def full_circuit(curve, n_c=200, n_vars=60, n_public=3, seed=0xf011):
    """seeded, sparse, random, one heavy column (signal 5 in every A); cirPower 8 with the defaults"""
    r = R[curve]
    rng = random.Random(seed + len(curve))

    def coef():
        k = rng.random()
        if k < 0.6:
            return 1 if rng.random() < 0.5 else r - 1
        if k < 0.8:
            return rng.randrange(2, 1 << 16)
        if k < 0.95:
            return 1 << rng.randrange(1, 254)
        return rng.randrange(r)

    def lc(extra=None):
        sigs = rng.sample(range(n_vars), rng.randrange(1, 5))
        out = [(s, coef()) for s in sigs if s != extra]
        if extra is not None:
            out.append((extra, coef()))
        return out
    return n_vars, 1, n_public - 1, [(lc(5), lc(), lc()) for _ in range(n_c)]


def one_signal_circuit(curve, n_c, n_vars, n_public, seed):
    """seeded sparse constraints with signal 0 in every A, B and C (the closed-form test)"""
    r = R[curve]
    rng = random.Random(seed)

    def lc():
        out = [(0, rng.choice([1, r - 1, 2, rng.randrange(r)]))]
        for s in rng.sample(range(1, n_vars), rng.randrange(0, 3)):
            out.append((s, rng.choice([1, r - 1, rng.randrange(1, 1 << 20), 1 << rng.randrange(1, 253), rng.randrange(r)])))
        return out
    return n_vars, 1, n_public - 1, [(lc(), lc(), lc()) for _ in range(n_c)]


def circuit_shaped(curve, lg, seed=1, n_public=2):
    """-> (r1cs bytes, n_vars): 2^lg - n_public - 1 constraints shaped like a compiled circuit, written with numpy. Rows follow
    synth_zkey.real_coefs (the distribution behind synth_zkey.make(coef_dist="real"): ~1.5 A terms and ~1 B term per constraint, heavy-tailed rows);
    on top the COLUMNS get their tail: signal 0 in every 16th A row, signals 1..4 in every 64th; one C term per constraint. Coefficients: 85 % +-1,
    10 % below 2^16, 5 % powers of two up to 2^253 (Num2Bits)."""
    import numpy as np

    from . import synth, synth_zkey
    r = R[curve]
    n = (1 << lg) - n_public                                            # real_coefs uses rows 0 .. n - 2
    n_c = n - 1
    m = max(8, n - 5)
    mat, con, sig, _in_b = synth_zkey.real_coefs(n, m, n_public, seed)
    keep = np.arange(mat.size) < mat.size - (n_public + 1)              # without the binding rows: newZKey adds them itself
    mat, con, sig = mat[keep].astype(np.uint64), con[keep].astype(np.uint64), sig[keep].astype(np.uint64)
    rows = np.arange(n_c, dtype=np.uint64)
    extra = [(np.zeros_like(rows[::16]), rows[::16], np.zeros_like(rows[::16]))]
    extra += [(np.zeros_like(rows[k::64]), rows[k::64], np.full_like(rows[k::64], k)) for k in range(1, 5)]
    extra.append((np.full_like(rows, 2), rows, np.uint64(5) + (synth.words(seed ^ 0xC0, n_c).astype(np.uint64) % np.uint64(m - 5))))
    mat = np.concatenate([mat] + [e[0] for e in extra]); con = np.concatenate([con] + [e[1] for e in extra]); sig = np.concatenate([sig] + [e[2] for e in extra])
    order = np.lexsort((mat, con))
    mat, con, sig = mat[order], con[order], sig[order]
    K = mat.size
    kind = synth.words(seed ^ 0xD0, K).astype(np.uint64)
    coef = np.zeros((K, 32), np.uint8)
    sel = kind % np.uint64(100)
    coef[:, 0] = 1
    minus = np.frombuffer((r - 1).to_bytes(32, "little"), np.uint8)
    coef[(sel < 85) & ((kind >> np.uint64(8)) % np.uint64(2) == 1)] = minus
    small = (sel >= 85) & (sel < 95)
    coef[small, 0] = ((kind[small] >> np.uint64(8)) % np.uint64(255) + np.uint64(2)).astype(np.uint8)
    coef[small, 1] = ((kind[small] >> np.uint64(16)) % np.uint64(256)).astype(np.uint8)
    p2 = np.nonzero(sel >= 95)[0]
    bit = ((kind[p2] >> np.uint64(8)) % np.uint64(253) + np.uint64(1)).astype(np.int64)
    coef[p2] = 0
    coef[p2, bit // 8] = (1 << (bit % 8)).astype(np.uint8)
    group = (np.uint64(3) * con + mat).astype(np.int64)                 # (constraint, matrix) of every entry
    counts = np.bincount(group, minlength=3 * n_c).astype(np.uint32)
    first = np.cumsum(counts) - counts                                  # entries before every group
    head_pos = 36 * first.astype(np.int64) + 4 * np.arange(3 * n_c, dtype=np.int64)
    ent_pos = 36 * np.arange(K, dtype=np.int64) + 4 * (group + 1)
    body = np.zeros(36 * K + 12 * n_c, np.uint8)
    body[head_pos[:, None] + np.arange(4)] = counts.astype("<u4").view(np.uint8).reshape(-1, 4)
    rec = np.concatenate([sig.astype("<u4").view(np.uint8).reshape(-1, 4), coef], axis=1)
    body[ent_pos[:, None] + np.arange(36)] = rec
    head = struct.pack("<I", 32) + r.to_bytes(32, "little") + struct.pack("<IIIIQI", m, 1, n_public - 1, m - 1 - n_public, m, n_c)
    out = b"r1cs" + struct.pack("<II", 1, 2) + struct.pack("<IQ", 1, len(head)) + head + struct.pack("<IQ", 2, body.size) + body.tobytes()
    return out, m


def plonk_mix_circuit(curve, n_random=24, seed=0x91c):
    """PLONK setup fixture (src/plonk_setup.js: process): every branch of the gate lowering with nPublic = 0, at most 256 PLONK rows.
    (n_vars, n_outputs, n_pub_inputs, constraints)"""
    r = R[curve]
    rng = random.Random(seed + len(curve))
    n_vars = 20
    cons = [
        ([], [(1, 1)], [(2, 1), (3, 5)]),                                               # A empty
        ([(1, 1)], [], [(4, r - 1)]),                                                   # B empty
        ([], [], []),                                                                   # everything empty: a row of zeros
        ([(0, 3)], [(2, 1), (3, 2)], [(4, 1)]),                                         # A constant-only
        ([(1, 1), (2, 2)], [(0, 7)], [(5, 1)]),                                         # B constant-only
        ([(1, 1)], [(0, 0)], [(5, 1)]),                                                 # B constant-only, the constant is zero
        ([(0, 0)], [(3, 1)], [(6, 1), (0, 9)]),                                         # A constant-only, zero
        ([(0, r - 1)], [(0, 4)], [(6, 1)]),                                             # A and B constant-only: A wins
        ([(0, 2), (1, 3)], [(0, 5), (2, 7)], [(0, 11), (3, 13)]),                       # a multiplication with constants in A, B and C
        ([(1, 1)], [(2, 1)], []),                                                       # a multiplication with C empty
        ([(1, 1)], [(2, 1)], [(0, 6)]),                                                 # a multiplication with C constant-only
        ([], [(1, 1)], [(1, 1), (2, 2), (3, 3), (4, 4)]),                               # a sum of 4 terms: one chained addition
        ([(0, 1)], [(1, 1), (2, r - 2), (3, 3), (4, 1 << 200), (5, 5), (6, 6), (7, 7)], [(8, 1), (0, 1)]),      # 7 + 1 terms through join
        ([], [], [(7, 1), (6, 2), (5, 3), (4, 4), (3, 5), (2, 6), (1, 7)]),             # a sum of 7 terms, ids descending in the file
        ([(1, 1), (2, 1)], [(3, 1), (4, 1), (5, 2)], [(6, 1), (7, 1), (8, 1)]),         # multiplications whose sides have 2 and 3 terms
        ([(9, 1), (3, 2), (0, 4), (5, 1)], [(8, 1), (2, 1)], [(7, 3), (1, 1)]),         # ids out of ascending order, a constant in the middle
        ([(10, 2), (10, 3)], [(11, 1)], [(12, 1), (12, 0)]),                            # a signal twice: the last coefficient stays
        ([(13, 0)], [(14, 1)], [(15, 1)]),                                              # a zero coefficient on a signal: still a multiplication
        ([(2, 1), (1, 1)], [(0, 2)], [(1, 2), (2, 2)]),                                 # join that cancels to zero coefficients (they stay)
    ]
    pick = lambda: rng.choice([1, r - 1, 2, rng.randrange(1 << 16), 1 << rng.randrange(1, 253), rng.randrange(r), 0])
    for _ in range(n_random):
        lc = lambda lo, hi: [(s, pick()) for s in rng.sample(range(0, n_vars - 1), rng.randrange(lo, hi))]      # signal n_vars - 1 is never used
        cons.append((lc(0, 4), lc(0, 4), lc(0, 6)))
    return n_vars, 0, 0, cons


def plonk_tiny_circuit(curve):
    """two constraints and one public signal: three PLONK rows, cirPower clamped to 3"""
    return 4, 1, 0, [([(2, 1)], [(3, 1)], [(1, 1)]), ([(2, 1)], [(2, 1)], [(3, 1)])]


def square_chain(curve, n_c, x0=3, b=5):
    """x_{i+1} = x_i^2 + b, n_c constraints, satisfiable: signal 1 = x_{n_c} (output), signal 2 = x_0 (public input), signal 2 + i = x_i.
    -> (n_vars, n_outputs, n_pub_inputs, constraints, witness as a list of integers)"""
    r = R[curve]
    x = [x0 % r]
    for _ in range(n_c):
        x.append((x[-1] * x[-1] + b) % r)
    sig = lambda i: 1 if i == n_c else 2 + i
    cons = [([(sig(i), 1)], [(sig(i), 1)], [(sig(i + 1), 1), (0, (r - b) % r)]) for i in range(n_c)]
    wit = [1, x[n_c]] + x[:n_c]
    return n_c + 2, 1, 1, cons, wit


def write_wtns(curve, values, prime=None):
    """bytes of a .wtns file (version 2): values are non-negative integers below 2^256, written as they are (a value of r or more stays one)"""
    q = R[curve] if prime is None else prime
    head = struct.pack("<I", 32) + q.to_bytes(32, "little") + struct.pack("<I", len(values))
    body = b"".join(int(v).to_bytes(32, "little") for v in values)
    out = bytearray(b"wtns" + struct.pack("<II", 2, 2))
    for typ, sec in ((1, head), (2, body)):
        out += struct.pack("<IQ", typ, len(sec)) + sec
    return bytes(out)


def lc_value(lc, wit, r):
    """a combination as wtns.check evaluates it: the LAST coefficient the list gives for a signal, each signal once"""
    last = {}
    for s, c in lc:
        last[s] = c
    return sum((c % r) * (wit[s] % r) for s, c in last.items()) % r


def satisfiable_circuit(curve, n_c, seed=0x5a7, n_free=12, rows=None, dups=False, wide=False, w0=1, tail=False):
    """n_c SATISFIED constraints and their witness -> (n_vars, n_outputs, n_pub_inputs, constraints, witness as a list of integers).
    A and B are random combinations of signals whose value is known; C is, in turn, one free signal (with random known terms beside it) whose value is
    solved from A * B, a lone constant on signal 0, or empty with the last coefficient of A (or of B) solved so that the combination evaluates to 0.
      rows   {(constraint, matrix): terms}: that combination gets exactly so many terms (matrix 0 = A, 1 = B, 2 = C), over distinct signals
      tail   heavy-tailed lengths for A where rows says nothing: short ones, and with probability `tail` (True: 0.1) one of 10^2 - 10^3 terms
      dups   some combinations name a signal twice, adjacent and apart, with an earlier coefficient that is NOT the one that counts
      wide   some coefficients are written as c + r or c + k r below 2^256, some witness values as v + r
      w0     value of signal 0 (wtns.check does not ask for 1)"""
    r = R[curve]
    rng = random.Random(seed + len(curve))
    rows = dict(rows or {})
    p_long = 0.1 if tail is True else float(tail)
    longest = max(list(rows.values()) + [0])
    n_free = max(n_free, longest + 2, 1100 if tail else 0)
    wit = [w0 % r] + [rng.randrange(1, r) for _ in range(n_free - 1)]
    cons = []

    def coef():
        k = rng.random()
        c = (1 if rng.random() < 0.5 else r - 1) if k < 0.5 else (rng.randrange(2, 1 << 16) if k < 0.7 else (1 << rng.randrange(1, 253) if k < 0.8 else rng.randrange(1, r)))
        if wide and rng.random() < 0.3:
            c += r * rng.randrange(1, ((1 << 256) - 1 - c) // r + 1)
        return c

    def combo(n, known, must=None):
        sigs = rng.sample(range(known), min(n, known))
        if must is not None and must not in sigs and sigs:
            sigs[-1] = must
        return [(s, coef()) for s in sigs]

    def with_dups(lc, known):
        """the same evaluation, with a stale coefficient in front of the one that counts: adjacent for the first term, apart for the last"""
        if len(lc) < 2:
            return lc
        (s0, c0), (s1, c1) = lc[0], lc[-1]
        return [(s0, (c0 + 1 + rng.randrange(r - 2)) % r), (s0, c0), (s1, (c1 + 1 + rng.randrange(r - 2)) % r)] + lc[1:-1] + [(s1, c1)]

    for i in range(n_c):
        known = len(wit)
        la = rows.get((i, 0), (rng.choice([1, 1, 1, 2, 3]) if rng.random() >= p_long else rng.randrange(100, 1000)) if tail else rng.randrange(1, 4))
        lb, lcn = rows.get((i, 1), rng.randrange(1, 3)), rows.get((i, 2))
        kind = i % 3 if lcn is None else (0 if lcn > 0 else 2)
        a, b = combo(la, known), combo(lb, known)
        if kind == 2:                                                    # C empty: A (or, every other time, B) is made to evaluate to 0
            side = a if (i // 3) % 2 == 0 or not b else b
            if side:
                s = next((t for t, _ in reversed(side) if wit[t] % r), None)
                if s is None:
                    kind = 1
                else:
                    rest = [(t, c) for t, c in side if t != s]
                    side[:] = rest + [(s, (-lc_value(rest, wit, r) * pow(wit[s], -1, r)) % r)]
            c = []
        if kind == 1:                                                    # C: a lone constant on signal 0
            if wit[0] % r == 0:
                kind = 0
            else:
                c = [(0, lc_value(a, wit, r) * lc_value(b, wit, r) * pow(wit[0], -1, r) % r)]
        if kind == 0:                                                    # C: one free signal solved from the rest
            rest = combo((lcn if lcn is not None else rng.randrange(1, 4)) - 1, known)
            k = rng.randrange(1, r)
            wit.append((lc_value(a, wit, r) * lc_value(b, wit, r) - lc_value(rest, wit, r)) * pow(k, -1, r) % r)
            c = rest + [(known, k)]
            rng.shuffle(c)
        if dups and i % 2 == 0:
            a, b, c = with_dups(a, known), (with_dups(b, known) if i % 4 == 0 else b), (with_dups(c, known) if kind == 0 else c)
        cons.append((a, b, c))
    if wide:
        wit = [v + r if v + r < 1 << 256 and rng.random() < 0.3 else v for v in wit]
    for a, b, c in cons:
        assert lc_value(a, wit, r) * lc_value(b, wit, r) % r == lc_value(c, wit, r)
    return len(wit), 1, 1, cons, wit


def fflonk_quirks_circuit(curve):
    """FFLONK setup fixture (src/r1cs_constraint_processor.js): every case of the lowering in 14 rows (domain 16), nPublic = 0. Each of the first four
    constraints gives one row; the multiplication gives ten: its A, B and C each hold five terms, the constant and four signals, so each folds
    three times. (A combination of five SIGNALS folds four times: three of them would fill the domain alone. plonk_mix_circuit has those.)
    (n_vars, n_outputs, n_pub_inputs, constraints)"""
    r = R[curve]
    cons = [
        ([(0, 0)], [(1, 1)], []),                                                       # A nullable through an explicit zero coefficient, C empty: a row of zeros
        ([(1, 1)], [], [(2, r + 3), (3, 1)]),                                           # B nullable (empty); a coefficient >= r
        ([(0, 2)], [(1, 1), (2, 1)], [(1, 2), (3, 1)]),                                 # A constant: 2 s1 - 2 s1 cancels and leaves the combination
        ([(4, 5), (5, 1), (4, 2)], [(0, 7)], [(6, 1), (7, 0)]),                         # B constant; signal 4 twice (2 stays); a zero coefficient on signal 7
        ([(0, 3), (1, 1), (2, 2), (3, 3), (4, 4)], [(8, 2), (0, 5), (5, 1), (6, r - 1), (7, 1 << 200)], [(0, 11), (9, 1), (10, 2), (11, 3), (12, 4)]),
    ]                                                                                   # signal 13 never occurs
    return 14, 0, 0, cons


def fflonk_rows_circuit(curve, rows, seed=0xff10):
    """FFLONK setup fixture of exactly `rows` rows with nPublic = 2: every constraint lowers to one row (a product of single terms, or a sum of three).
    The first rows - 2 constraints do not depend on `rows`, so rows + 1 is the same circuit plus one row. (n_vars, n_outputs, n_pub_inputs, constraints)"""
    r = R[curve]
    rng = random.Random(seed + len(curve))
    n_vars = 12
    pick = lambda: rng.choice([1, r - 1, 2, rng.randrange(1 << 16), 1 << rng.randrange(1, 253), rng.randrange(1, r)])
    cons = []
    for i in range(rows - 2):
        a, b, c = rng.sample(range(1, n_vars), 3)
        cons.append(([], [], [(a, pick()), (b, pick()), (c, pick())]) if i % 3 == 2 else ([(a, pick())], [(b, pick())], [(c, pick())]))
    return n_vars, 1, 1, cons
