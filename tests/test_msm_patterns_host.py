"""The scalar sets of tests/msm_patterns.py hold what the GPU tests (tests/test_gpu_msm_widths.py) claim to run: every named edge of the signed-digit
recoding and of the bucket grid is present in the digit_edges set of every window width and scalar size, and the skew set fills one bucket beyond
what a block of the combine tree takes. A kind that went missing here would leave the GPU test passing while proving nothing about it. No GPU needed."""
import pytest

import msm_patterns as P

SIZES = (1, 4, 31, 32)
N = 3077                                       # the size the GPU test runs every scalar width at; the larger sets begin with the same rows
# csrc/msm.cuh: MSM_MAX_CAP (most points per lane) and csrc/msm_host.hpp: MSM_TB (lanes per block of k_msm_tree): a bucket with more entries
# than their product is spread over more than one tree block at ANY lane cap and is finished by k_msm_giant
MSM_MAX_CAP, MSM_TB = 256, 128

KINDS = ("largest magnitude", "negative next to the sign change", "raw window 2^c", "top digit is the carry alone", "last row, column 0", "row 0, last column")


def present(c, sb, values):
    """which KINDS occur among the digits of the scalars"""
    Wd, half = P.digits_of(sb, c), 1 << (c - 1)
    rbits, cbits = P.grid_bits(c)
    seen = set()
    for s in values:
        digits, raws = P.signed_digits(s, c, sb)
        assert sum((-m if neg else m) << (c * w) for w, m, neg in digits) == s, (c, sb, hex(s))
        assert all(1 <= m <= half for _, m, _ in digits) and len(raws) == Wd
        if (1 << c) in raws:
            seen.add(KINDS[2])
        if Wd >= 2 and (s >> ((Wd - 1) * c)) == 0 and raws[-1] == 1:
            seen.add(KINDS[3])
        for w, m, neg in digits:
            row, col = (m - 1) >> cbits, (m - 1) & ((1 << cbits) - 1)
            if m == half:
                seen.add(KINDS[0])
            if neg and m == half - 1:
                seen.add(KINDS[1])
            if col == 0 and row == (1 << rbits) - 1:
                seen.add(KINDS[4])
            if row == 0 and col == (1 << cbits) - 1:
                seen.add(KINDS[5])
    return seen


def attainable(c, sb):
    """The KINDS that ANY scalar of B = 8*sb bits can show at width c, from the arithmetic of the recoding alone (short scalars cannot reach the upper
    buckets of a wide window; for the 31- and 32-byte scalars of the provers B >= 2c holds at every width and all six are required):
      - magnitude 2^(c-1), and a negative digit at all, need bit c-1 of some window: a window with all its c bits inside the scalar, B >= c;
      - the carry that leaves the top digit alone comes out of such a window too, and the window above it is then the top one: B >= c;
      - raw 2^c is an all-ones window above a negative one: two whole windows, B >= 2c;
      - the last grid row begins at magnitude 2^(c-1) - 2^cbits + 1 >= 2^(c-2): c-1 scalar bits in one window; as a negative digit, B >= c either way;
      - the last column of row 0 is magnitude 2^cbits: cbits + 1 scalar bits."""
    B = 8 * sb
    rbits, cbits = P.grid_bits(c)
    need = {KINDS[0]: c, KINDS[1]: c, KINDS[2]: 2 * c, KINDS[3]: c, KINDS[4]: c - 1, KINDS[5]: cbits + 1}
    return {k for k, bits in need.items() if B >= bits}


@pytest.mark.parametrize("sb", SIZES)
@pytest.mark.parametrize("c", P.WIDTHS)
def test_digit_edges_hold_every_named_digit(c, sb):
    values = P.ints(P.edge_set(c, N, sb), sb)
    assert len(values) == N and all(v < (1 << (8 * sb)) for v in values)
    want = attainable(c, sb)
    if sb >= 31:
        assert want == set(KINDS)
    missing = want - present(c, sb, values)
    assert not missing, (c, sb, sorted(missing))


@pytest.mark.parametrize("c", P.WIDTHS)
def test_larger_sets_begin_with_the_checked_rows(c):
    """the 2^14-term set of the GPU test is the 3077-term set checked above plus further draws, and scalars >= r are among them"""
    small, big = P.edge_set(c, N), P.edge_set(c, 1 << 14)
    assert bytes(big[:N * 32]) == bytes(small)
    assert sum(v >= (1 << 255) for v in P.ints(small, 32)) > 100 and max(P.ints(small, 32)) == (1 << 256) - 1      # both group orders are below 2^255


@pytest.mark.parametrize("c", P.WIDTHS)
def test_skew_fills_a_giant_bucket(c):
    """three values and zeros at 2^14 terms: with a window table (one bucket set for all digits) the fullest bucket outgrows one tree block"""
    n = 1 << 14
    values = P.ints(P.skew_set(c, n), 32)
    assert len(set(values)) == 4 and 0 in values and (1 << 256) - 1 in values
    fill = {}
    for v in set(values):
        digits, _ = P.signed_digits(v, c, 32)
        assert sum((-m if neg else m) << (c * w) for w, m, neg in digits) == v
        for _, m, _ in digits:
            fill[m - 1] = fill.get(m - 1, 0) + values.count(v)
    assert max(fill.values()) > MSM_MAX_CAP * MSM_TB, (c, max(fill.values()))
    assert fill[(1 << (c - 1)) - 1] > MSM_MAX_CAP * MSM_TB        # and so does the LAST bucket of the grid


def test_special_logs_shape():
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    k = P.discrete_logs("special", 3077, r)
    assert len(set(k)) == 11 and all(0 <= v < r for v in k)        # five values, their negations and 0
    assert all(k[i] == 0 for i in range(16, 3077, 17)) and k.count(0) == sum(i % 17 == 16 or (i % 11 == 10 and i % 17 == 0) for i in range(3077))    # and the negation of one
    assert all((k[i] + k[i - 1]) % r == 0 for i in range(10, 3077, 11) if i % 17 != 16)
    assert not any(v == 0 for v in k[:16]) and P.discrete_logs("geometric", 3, r) == [7, 77, 847]
    sc = P.scalars("uniform", 0, 4, 32, seed=1)
    assert P.closed_form(sc, 32, [1, 0, 2, 5], r, k=3) == (P.ints(sc, 32)[0] + 2 * P.ints(sc, 32)[2]) % r
