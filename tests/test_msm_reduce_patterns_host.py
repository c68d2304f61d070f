"""What tests/test_gpu_msm_reduce.py claims for its inputs, counted on the CPU: a model (tests/msm_reduce_patterns.py) replays on discrete logarithms the order
in which each row / column kernel, the bit sums and the lane-partial tree add their operands and classifies every addition. Each pattern must reach the
branches it is named for at every width the GPU test runs it at, and the model's sums must be the closed-form ones. The second half counts the same
branches for the sets the suite ran before (tests/test_gpu_msm_widths.py): the written record of what those sets did and did not reach. No GPU needed."""
import pytest

import msm_patterns as P
import msm_reduce_patterns as M
import msm_sort_ref as R

# (width, form of the row / column sums, group whose staged shape is modelled): the table widths of the GPU test, and 13 / 15 under ZKMI_ROWCOL_WAVE=0
SHAPES = [(12, "staged", 1), (12, "staged", 2), (13, "wave", 1), (15, "wave", 1), (17, "wave", 1), (20, "wave", 1), (13, "staged", 1), (13, "staged", 2),
          (15, "staged", 1), (15, "staged", 2)]
TERMS = {12: 4096, 13: 8192, 15: 1 << 14, 17: 1 << 16, 20: 1 << 19}


def padded(rows, c):
    return rows + [0] * ((1 << P.grid_bits(c)[1]) - len(rows))


@pytest.mark.parametrize("name", ("bn128", "bls12381"))
@pytest.mark.parametrize("c,form,group", SHAPES)
def test_patterns_reach_their_branches(c, form, group, name):
    r = M.order(name)
    rbits, cbits = P.grid_bits(c)
    lanes = 64 if form == "wave" else M.staged_lanes(c, group)[0]
    for kind in M.PATTERNS:
        terms = M.pattern(kind, c, r, TERMS[c])
        V, counts, rows, cols, k = M.expected(terms, c, 1, r)
        t, mrows, mcols = M.count_rowcol(V, counts, c, r, form, group)
        assert (mrows, mcols) == (rows[0], cols[0]), (kind, "the model's sums are not the closed-form ones")
        assert k == sum((b + 1) * v for _, b, v in terms) % r
        bits = M.count_bitsums([padded(rows[0], c), cols[0]], c, r, 128 if (name, group) == ("bls12381", 2) else 256)
        print(c, form, group, kind, dict(t), "bit sums", dict(bits))
        if cbits <= 7:                               # the widths at which the GPU test runs without a table: k_msm_wsum over the same two arrays
            ws, weighted, total = M.count_wsum([padded(rows[0], c), cols[0]], r)
            assert weighted == [sum(i * v for i, v in enumerate(a)) % r for a in (rows[0], cols[0])] and total == [sum(rows[0]) % r, sum(cols[0]) % r]
            print("   k_msm_wsum", dict(ws))
            assert kind != "constant" or ws["doubling"] > 0
            assert kind != "alternate_rows" or ws["cancel"] > 0
            assert kind != "generic" or (ws["doubling"], ws["cancel"]) == (0, 0)
        if kind == "constant":                       # equal buckets: doublings in the shares (from two buckets per lane on) and at every level of the tree
            assert t["doubling"] > 0 and t["cancel"] == 0 and len(set(rows[0])) == 1 and len(set(cols[0])) == 1 and rows[0][0] == 1 << cbits
            assert bits["doubling"] > 0              # and all row sums equal: the bit sums double too
        elif kind == "alternate_fine":               # neighbours cancel at the first meeting (the staged lanes, an even stride apart: at the fold), everything after is infinity
            assert t["cancel"] > 0 and (t["skipped"] > 0 or form == "staged") and not any(rows[0]) and not any(cols[0]) and k == 0
        elif kind == "alternate_coarse":
            assert t["cancel"] > 0 and not any(rows[0]) and not any(cols[0])
            if rbits >= 7 and form == "wave":        # every lane of every sum goes point -> infinity
                assert t["cancel"] >= 64 * ((1 << rbits) + (1 << cbits))
            if rbits >= 8 and form == "wave":        # ... -> point again, from four buckets per lane on: more first operands than there are lanes
                assert t["first"] > 64 * ((1 << rbits) + (1 << cbits))
        elif kind == "alternate_rows":               # columns cancel in the shares; the row sums are C G and -C G in turn, and the bit sums add them up
            assert t["cancel"] > 0 and not any(cols[0]) and rows[0][:2] == [1 << cbits, r - (1 << cbits)] and bits["cancel"] > 0
        elif kind == "cancelled":                    # entries and no point: skipped operands in buckets the count says are there
            gate = sum(1 for b, v in enumerate(V) if counts[b] and not v)
            assert gate > 0 and t["skipped"] >= gate and (t["doubling"], t["cancel"]) == (0, 0)
            assert rows[0][0] and rows[0][-1] and cols[0][0] and cols[0][-1]
        elif kind == "one_per_row":                  # one point per row, at place 0, 63, 64 and last: infinity is skipped around it
            assert t["first"] >= 1 << rbits and t["skipped"] > 0 and (t["doubling"], t["cancel"]) == (0, 0) and all(rows[0])
            assert {b & ((1 << cbits) - 1) for _, b, _ in terms} == {0, 63, min(64, (1 << cbits) - 1), (1 << cbits) - 1}
        else:
            assert t["generic"] > 0 and (t["doubling"], t["cancel"]) == (0, 0) and (bits["doubling"], bits["cancel"]) == (0, 0)
        assert lanes >= 1


@pytest.mark.parametrize("name", ("bn128", "bls12381"))
def test_fat_buckets_reach_the_tree(name):
    """the two fat buckets at the shape of the GPU test (c = 16, 2^16 terms): 8 lanes for k_msm_tree alone, 256 lanes for two tree blocks and k_msm_giant.
    The order inside a bucket's list is the sort's to choose: with equal copies every order gives equal lane partials; with every second one negated the
    bucket is infinity in any order, and the count below is for lists that alternate as the input does."""
    r, c = M.order(name), 16
    cap = R.lane_cap(1 << 16, c, P.digits_of(32, c), True)
    assert cap == 8
    for same in (True, False):
        terms = M.fat(c, r, cap, same)
        V, counts, _, _, _ = M.expected(terms, c, 1, r)
        j = R.lanes_log(counts, cap)
        assert R.schedule_totals(counts, cap) == (8 + 256 + 2, 8 + 256, 1)
        for b in (i for i, x in enumerate(j.tolist()) if x):
            t, total = M.count_tree(M.lane_partials([v for _, bb, v in terms if bb == b], 1 << int(j[b]), r), r)
            assert total == V[b] and (total != 0) == same
            if same:
                assert t["doubling"] == (1 << int(j[b])) - 1 and t["generic"] == t["cancel"] == 0      # every addition of both trees
            else:
                assert t["skipped"] > 0 and t["generic"] == t["doubling"] == t["cancel"] == 0


# ---- the sets the suite ran before ---------------------------------------------------------------------------------------------------------------------
SMALL, LARGE = 3077, 1 << 14                         # tests/test_gpu_msm_widths.py
# Where the row / column sums of an existing set DO add equal or opposite points: uniform scalars over the 3 077 "special" bases (five logarithms, their
# negations and infinity, times the table rows) in the wide tables, whose buckets mostly hold one entry — two buckets of a row then hold the same point now
# and then. Nothing else does: not one doubling or cancellation at any width for the geometric bases, for the digit-edge and skewed scalars, or below
# c = 15; and never more than a few hundred among 10^5 additions, in the shares and the first tree levels only. (A library built with a wrong dbl_xyzz29
# bore the count out on the device: test_table_msm_every_width failed at c = 15, 16, 17 and 20 and passed at every other width. The witness-like scalars of
# test_table_msm_multi_vs_closed_form, mostly 0 and 1, are not counted here; they noticed it at c = 13 too.)
KNOWN = {("special", "uniform", 15), ("special", "uniform", 16), ("special", "uniform", 17), ("special", "uniform", 20)}


@pytest.mark.parametrize("kind", ("uniform", "digit_edges", "skew"))
@pytest.mark.parametrize("n,bases", ((SMALL, "special"), (LARGE, "geometric")))
def test_existing_sets_do_not_reach_them(n, bases, kind):
    r = M.order("bn128")
    logs = P.discrete_logs(bases, n, r)
    for c in P.WIDTHS:
        sc = P.scalars("uniform", 0, n, 32, seed=P.UNIFORM_SEED + n + 32) if kind == "uniform" else P.edge_set(c, n) if kind == "digit_edges" else P.skew_set(c, n)
        V, counts = M.buckets_of_set(sc, n, 32, c, logs, r)
        rare = [0, 0]
        for form, group in ((("wave", 1),) if c >= 13 else (("staged", 1), ("staged", 2))):
            t, rows, cols = M.count_rowcol(V, counts, c, r, form, group)
            rare = [rare[0] + t["doubling"], rare[1] + t["cancel"]]
        bits = M.count_bitsums([padded(rows, c), cols], c, r)
        print(bases, kind, c, "row / column sums: doublings, cancellations", rare, "bit sums", bits["doubling"], bits["cancel"])
        assert (bits["doubling"], bits["cancel"]) == (0, 0), c
        if (bases, kind, c) in KNOWN:
            assert rare[0] > 0 and rare[1] > 0 and sum(rare) < 500, (c, rare)
        else:
            assert rare == [0, 0], (c, rare)
