"""Inputs for the window-table MSM tests and a Python restatement of the signed-digit recoding they aim at (plain helpers, no fixtures).

The resident-table MSM (csrc/msm29.cuh, msm_sort.hip, msm_host.hpp: msm_reduce) recodes every scalar into signed c-bit digits (csrc/msm.cuh:
for_each_digit), sorts the digits into nb = 2^(c-1) buckets (bucket = magnitude - 1) and sums the buckets as a 2^rbits x 2^cbits grid
(rbits = (c-1)/2, cbits = c-1-rbits, bucket = row * 2^cbits + column). The generators here build scalars window by window, so that the edges
of that scheme are hit on purpose instead of with probability Wd*n / 2^c, and bases with known discrete logarithms, so that every MSM has a
closed form that involves no MSM."""
import numpy as np

import synth

WIDTHS = (8, 9, 10, 11, 12, 13, 15, 16, 17, 20)          # everything csrc/msm_host.hpp: msm_precomp_c can return


def digits_of(sb, c):
    """Wd of csrc/msm_host.hpp: msm_digits"""
    return (8 * sb + 1 + c - 1) // c


def grid_bits(c):
    """(rbits, cbits) of csrc/msm_host.hpp: msm_reduce"""
    rbits = (c - 1) // 2
    return rbits, c - 1 - rbits


def signed_digits(s, c, sb):
    """csrc/msm.cuh: for_each_digit, literally. Returns (digits, raws): digits is the list of (window, magnitude, negative) of the non-zero
    digits, raws[w] the window's c bits plus the carry that came in (so 2^c shows: an all-ones window with a carry, magnitude 0, carry out)."""
    Wd, half, carry = digits_of(sb, c), 1 << (c - 1), 0
    digits, raws = [], []
    for w in range(Wd):
        raw = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        neg = raw > half
        mag = (1 << c) - raw if neg else raw
        carry = 1 if neg else 0
        raws.append(raw)
        if mag:
            digits.append((w, mag, neg))
    return digits, raws


def edge_windows(c):
    """The raw c-bit windows a digit_edges scalar is assembled from: the ends of the magnitude range, of the first grid row and of the sign
    change, and the first and last bucket of the last grid row (magnitude 2^(c-1) - 2^cbits + 1 is row 2^rbits - 1, column 0; its mirror
    image 2^(c-1) + 2^cbits - 1 is the same bucket with the sign set). Values that do not fit c bits (c = 1, 2) are left out."""
    rbits, cbits = grid_bits(c)
    half, col = 1 << (c - 1), 1 << cbits
    vals = (0, 1, col - 1, col, col + 1, half - 1, half, half + 1, (1 << c) - 2, (1 << c) - 1, half - col + 1, half + col - 1)
    return sorted({v for v in vals if 0 <= v < (1 << c)})


N_FIXED = 8


def _fixed_rows(c, sb):
    """the rows every digit_edges set begins with (before truncation to 8*sb bits)"""
    Wd, bits, half, ones = digits_of(sb, c), 8 * sb, 1 << (c - 1), (1 << c) - 1
    rep = lambda f: sum(f(w) << (w * c) for w in range(Wd))
    top = (Wd - 1) * c                                      # the top window holds scalar bits only where it begins below 8*sb: else the top bit
    return [rep(lambda w: ones),                            # all 0xFF
            rep(lambda w: half),                            # the largest positive digit in every window: bucket nb - 1
            rep(lambda w: ones if w & 1 else half + 1),     # a carry chain through every window: raw 2^c in the odd ones
            rep(lambda w: half + 1 if w & 1 else ones),     # ... and in the even ones
            1 << (top if top < bits else bits - 1),         # the only non-zero digit is the top one
            half + 1,                                       # -(2^(c-1) - 1) then the carry alone
            0, 1]


def scalars(kind, c, n, sb=32, seed=0):
    """n scalars of sb bytes, little-endian, as a uint8 array of n*sb bytes. Values >= r are wanted: nothing reduces them before the MSM."""
    if kind == "uniform":
        if sb == 32:
            return synth.elems(seed, n)
        return synth.elems(seed, (n * sb + 31) // 32 + 1)[:n * sb].copy()
    mask = (1 << (8 * sb)) - 1
    if kind == "digit_edges":
        Wd, vals = digits_of(sb, c), edge_windows(c)
        pick = np.random.default_rng(seed).integers(0, len(vals), size=(max(n, N_FIXED), Wd))
        rows = _fixed_rows(c, sb)
        for i in range(N_FIXED, n):
            rows.append(sum(vals[int(pick[i, w])] << (w * c) for w in range(Wd)))
        return np.frombuffer(b"".join((v & mask).to_bytes(sb, "little") for v in rows[:n]), np.uint8).copy()
    if kind == "skew":
        Wd = digits_of(sb, c)
        three = (mask,                                                    # 2^(8 sb) - 1
                 sum(1 << (w * c) for w in range(Wd)) & mask,              # digit 1 in every window: with a table they all meet in bucket 0
                 sum(1 << (w * c + c - 1) for w in range(Wd)) & mask)      # digit 2^(c-1) in every window: bucket nb - 1
        sel = np.random.default_rng(seed).integers(0, 4, size=n)
        return np.frombuffer(b"".join((three[int(k)] if k < 3 else 0).to_bytes(sb, "little") for k in sel), np.uint8).copy()
    raise ValueError(kind)


EDGE_SEED, SKEW_SEED, UNIFORM_SEED = 0xED6E, 0x5EE, 0x0771


def edge_set(c, n, sb=32):
    """THE digit_edges set of width c: the one tests/test_msm_patterns_host.py examines is the one the GPU tests run"""
    return scalars("digit_edges", c, n, sb, seed=EDGE_SEED + c)


def skew_set(c, n):
    return scalars("skew", c, n, 32, seed=SKEW_SEED + c)


def ints(buf, sb):
    b = bytes(buf)
    return [int.from_bytes(b[i:i + sb], "little") for i in range(0, len(b), sb)]


def discrete_logs(kind, n, r, seed=0):
    """k_i with base_i = k_i * G (0: the point at infinity)"""
    if kind == "geometric":                                  # what zkmi_gen_geometric_bases_dev(…, 7, 11, …) writes
        out, f = [], 7
        for _ in range(n):
            out.append(f)
            f = f * 11 % r
        return out
    if kind == "special":
        big = int.from_bytes(synth.elems(0x5EC1A1 + seed, 1).tobytes(), "little") % r
        cyc = (5, 0x1234567, 3, big, 2)
        out = []
        for i in range(n):
            k = cyc[i % 5]                                   # five values: equal points meet in one bucket (P + P)
            if i % 11 == 10:
                k = (r - out[i - 1]) % r                     # the neighbour's negation (P - P: infinity, and back from it)
            if i % 17 == 16:
                k = 0                                        # a base at infinity: the table's infinity bitmap must drop it
            out.append(k)
        return out
    raise ValueError(kind)


def logs_bytes(logs):
    """the 32-byte little-endian scalars zkmi_gen_bases_from_scalars_dev reads"""
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in logs), np.uint8).copy()


def closed_form(sc, sb, logs, r, k=None):
    """sum s_i * k_i mod r over the first k terms, in Python integers"""
    s = ints(sc, sb)
    k = len(s) if k is None else k
    return sum(a * b for a, b in zip(s[:k], logs[:k])) % r
