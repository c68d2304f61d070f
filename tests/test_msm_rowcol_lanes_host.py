"""Lanes per row / column sum of the bucket reduction (csrc/msm29.cuh: k_msm_rowcol_wave29<C, LPS>, k_msm_rowcol_wave29_g2<C, LPS>), on the CPU.

With LPS lanes per sum, lane t of a block belongs to sum t / LPS, adds the entries t % LPS, t % LPS + LPS, ... of its row or column, and a tree of
log2(LPS) levels (lane t += lane t + d for t a multiple of 2 d, d = 1 .. LPS / 2) leaves the sum in lane t % LPS == 0. This file replays that order
on discrete logarithms (tests/msm_reduce_patterns.py: a value v stands for v * G, 0 for the point at infinity) for LPS = 8, 16, 32, 64 at the three
shapes tests/test_gpu_msm_rowcol_lanes.py runs on the device, and holds the patterns of that test to what they are there for:
  constant           every addition of every tree level is a doubling, whatever LPS
  alternate_fine     every addition of level 1 is a cancellation and every level above meets infinity alone
  alternate_coarse   the two halves cancel: in the tree where the sign bit is below LPS, else inside the lanes' shares
  one_per_row        (places 0, LPS - 1, LPS and the last one of the row) a lone point passes every level as an operand skipped or taken over
  levels_rows / _cols  sign bit k = index % 6 of the other index: a cancellation at EVERY tree level of every LPS. The two alternate patterns reach level
                     1 and one level of 32 or 64 alone, so this pair is what pins the levels between
The replay with 64 lanes is the existing model (msm_reduce_patterns.count_rowcol, "wave"). The second half asks csrc/msm_select.hpp which LPS it picks,
through tools/msm_select_hosttest.hip as tests/test_msm_select_host.py does. No GPU needed."""
import os

import numpy as np
import pytest

import msm_patterns as P
import msm_reduce_patterns as M
from test_msm_select_host import DEFAULT, fields, tool                      # noqa: F401  (tool: the fixture that builds and drives the host program)

LANES = (8, 16, 32, 64)
SHAPES = (13, 14, 15)                               # rbits / cbits 6 / 6, 6 / 7, 7 / 7
R_BN = M.order("bn128")


def lone_places(lps, n):
    return (0, lps - 1, min(lps, n - 1), n - 1)


def pattern(kind, c, r, lps=64):
    """the terms (window 0) of one bucket set: the patterns of msm_reduce_patterns, one_per_row with its places moved to the group boundary of this
    LPS, and the two level patterns"""
    rbits, cbits = P.grid_bits(c)
    R, C = 1 << rbits, 1 << cbits
    neg = lambda s: r - 1 if s & 1 else 1
    if kind == "one_per_row":
        d = M._logs(0x1A9E + c, R, r)
        return [(0, (i << cbits) + lone_places(lps, C)[i % 4], d[i]) for i in range(R)]
    if kind == "one_per_col":
        d = M._logs(0x1A9F + c, C, r)
        return [(0, (lone_places(lps, R)[j % 4] << cbits) + j, d[j]) for j in range(C)]
    if kind == "levels_rows":
        return [(0, b, neg((b & (C - 1)) >> ((b >> cbits) % 6))) for b in range(R * C)]
    if kind == "levels_cols":
        return [(0, b, neg((b >> cbits) >> ((b & (C - 1)) % 6))) for b in range(R * C)]
    return M.pattern(kind, c, r, R * C)


def replay(Vw, counts_w, c, r, lps):
    """-> (tally of the shares, {d: tally of tree level d} for rows, the same for columns, rows, cols)"""
    rbits, cbits = P.grid_bits(c)
    R, C = 1 << rbits, 1 << cbits
    X, live = M._obj(Vw, (R, C)), np.asarray(counts_w).reshape(R, C) > 0
    shares, levels, sums = M.Tally(), [], []
    for Mx, lv in ((X, live), (X.T.copy(), live.T.copy())):
        acc = M._strided(Mx, lv, lps, r, shares)
        lev, d = {}, 1
        while d < lps:
            lev[d] = M.Tally()
            idx = np.arange(0, lps, 2 * d)
            acc[:, idx] = M._add(acc[:, idx], acc[:, idx + d], r, lev[d])
            d *= 2
        levels.append(lev)
        sums.append([int(v) for v in acc[:, 0]])
    return shares, levels[0], levels[1], sums[0], sums[1]


def run(kind, c, lps):
    terms = pattern(kind, c, R_BN, lps)
    V, counts, rows, cols, _ = M.expected(terms, c, 1, R_BN)
    shares, lr, lc, got_r, got_c = replay(V, counts, c, R_BN, lps)
    assert got_r == rows[0] and got_c == cols[0], (kind, c, lps)            # whoever adds what, the sums are the sums
    assert sorted(lr) == sorted(lc) == [1 << k for k in range(lps.bit_length() - 1)]
    return shares, lr, lc


@pytest.mark.parametrize("c", SHAPES)
def test_64_lanes_is_the_existing_model(c):
    for kind in ("constant", "alternate_fine", "alternate_coarse", "one_per_row", "cancelled", "generic"):
        terms = M.pattern(kind, c, R_BN, 1 << (c - 1))
        V, counts, _, _, _ = M.expected(terms, c, 1, R_BN)
        shares, lr, lc, rows, cols = replay(V, counts, c, R_BN, 64)
        tally, rows0, cols0 = M.count_rowcol(V, counts, c, R_BN, "wave")
        total = {k: shares[k] + sum(t[k] for t in lr.values()) + sum(t[k] for t in lc.values()) for k in M.CLASSES}
        assert total == dict(tally) and (rows, cols) == (rows0, cols0), (kind, c)


@pytest.mark.parametrize("lps", LANES)
@pytest.mark.parametrize("c", SHAPES)
def test_constant_doubles_at_every_level(c, lps):
    rbits, cbits = P.grid_bits(c)
    shares, lr, lc = run("constant", c, lps)
    for lev, n_sums in ((lr, 1 << rbits), (lc, 1 << cbits)):
        for d, t in lev.items():
            assert t["doubling"] == n_sums * lps // (2 * d) and sum(t.values()) == t["doubling"], (c, lps, d, dict(t))
    # more than one entry per lane: the second one doubles the first
    assert (shares["doubling"] > 0) == ((1 << cbits) > lps or (1 << rbits) > lps), (c, lps, dict(shares))


@pytest.mark.parametrize("lps", LANES)
@pytest.mark.parametrize("c", SHAPES)
def test_alternate_fine_cancels_then_skips(c, lps):
    shares, lr, lc = run("alternate_fine", c, lps)
    for lev in (lr, lc):
        for d, t in lev.items():
            only = "cancel" if d == 1 else "skipped"
            assert t[only] > 0 and sum(t.values()) == t[only], (c, lps, d, dict(t))
    assert shares["cancel"] == 0                    # LPS is even: a lane's entries share a sign


@pytest.mark.parametrize("lps", LANES)
@pytest.mark.parametrize("c", SHAPES)
def test_alternate_coarse_cancels_at_or_across_the_group(c, lps):
    rb, cb = M.coarse_bits(c)
    shares, lr, lc = run("alternate_coarse", c, lps)
    in_shares = 0
    for lev, bit in ((lr, cb), (lc, rb)):           # a row sum runs over the column index and the other way round
        for d, t in lev.items():
            if (1 << bit) >= lps or d > 1 << bit:   # cancelled inside the lanes, or further down the tree: infinity alone
                assert sum(t.values()) == t["skipped"] > 0, (c, lps, d, dict(t))
            elif d < 1 << bit:
                assert sum(t.values()) == t["doubling"] > 0, (c, lps, d, dict(t))
            else:
                assert sum(t.values()) == t["cancel"] > 0, (c, lps, d, dict(t))
        in_shares += (1 << bit) >= lps
    assert (shares["cancel"] > 0) == (in_shares > 0), (c, lps, dict(shares))


@pytest.mark.parametrize("lps", LANES)
@pytest.mark.parametrize("c", SHAPES)
def test_lone_points_pass_every_level(c, lps):
    """place 0: the sum's own lane skips an infinite partner at every level; place LPS - 1: the point is taken over by an empty lane at every level;
    places LPS and last: a lane's second and last entry, then the same walk. Rows by one_per_row, columns by its transpose."""
    for kind, mine in (("one_per_row", 0), ("one_per_col", 1)):
        out = run(kind, c, lps)
        for d, t in out[1 + mine].items():
            assert t["skipped"] > 0 and t["first"] > 0 and t["generic"] + t["doubling"] + t["cancel"] == 0, (kind, c, lps, d, dict(t))


@pytest.mark.parametrize("lps", LANES)
@pytest.mark.parametrize("c", SHAPES)
def test_a_cancellation_at_every_level(c, lps):
    for kind, mine in (("levels_rows", 1), ("levels_cols", 2)):
        out = run(kind, c, lps)
        for d, t in out[mine].items():
            assert t["cancel"] > 0, (kind, c, lps, d, dict(t))


def test_work_model():
    """wave-addition-times of one c = 20 bucket set (512 rows of 1024 buckets, 1024 columns of 512), the empty row slots not counted: the table of
    DESIGN.md section 4.5"""
    def cost(lps):
        depth, per_wave = lps.bit_length() - 1, 64 // lps
        return 512 // per_wave * (1024 // lps + depth) + 1024 // per_wave * (512 // lps + depth)
    assert [cost(v) for v in (64, 32, 16, 8)] == [25600, 20224, 17920, 16960]


# ---- the pick -----------------------------------------------------------------------------------------------------------------------------------------------
# rowcol_lanes group limbs all_r29 rbits cbits aux compact_code n_sums <8 switches> rc_lanes rc_lanes_g2 -> kernel threads max_blocks bitsums_lds lanes code [message]
INVALID = 2
# csrc/msm_select.hpp: msm_rc_lanes_default (profiles/r07_rowcol_lanes_ab.md has the measurements behind it): 64 lanes a sum, but 16 for the Fq2 sums of the
# 9-limb curve on the auxiliary stream, where they run underneath the G1 accumulations
G1_LANES, G2_LANES = 64, 64                         # on the main stream


def default_lanes(group, limbs, aux):
    return 16 if group == 2 and aux and limbs == 9 else 64


def ask(tool, group, limbs, all_r29, rbits, cbits, aux, cc, n_sums, t=DEFAULT, rc=0, rc_g2=0):
    return tool(["rowcol_lanes %d %d %d %d %d %d %d %d %s %d %d" % (group, limbs, all_r29, rbits, cbits, aux, cc, n_sums, fields(t), rc, rc_g2)])[0].split(" ", 6)


def test_pick_defaults_for_the_shapes_the_product_runs(tool):
    # (group, limbs, rbits, cbits, aux, sums): Groth16's batched G1 launch at c = 20 (A, B1, C + H) and its G2 launch on the auxiliary stream; a lone
    # table MSM or PLONK commitment; BLS12-381; the small shapes of the tests
    for group, limbs, rb, cb, aux, n_sums in ((1, 9, 9, 10, 0, 3 * 2048), (2, 9, 9, 10, 1, 2048), (1, 9, 9, 10, 0, 2048), (2, 9, 9, 10, 0, 2048), (1, 14, 9, 10, 0, 3 * 2048),
                                              (2, 14, 9, 10, 1, 2048), (1, 9, 9, 10, 1, 2048), (1, 9, 6, 6, 0, 128), (2, 9, 6, 7, 0, 256), (2, 9, 6, 6, 1, 128),
                                              (1, 14, 7, 7, 0, 3 * 256), (2, 9, 9, 10, 1, 0)):
        f = ask(tool, group, limbs, 1, rb, cb, aux, 0, n_sums)
        assert f[0] == ("wave29_g2" if group == 2 else "wave29") and int(f[4]) == default_lanes(group, limbs, aux) and int(f[5]) == 0, f
        old = tool(["rowcol %d %d 1 %d %d %d 0 %s" % (group, limbs, rb, cb, aux, fields(DEFAULT))])[0].split()
        assert f[:4] == old[:4], (f, old)                                   # kernel, threads, cap and bit sums as without the lanes
    # the cap of the auxiliary stream counts waves, whatever a wave holds
    assert ask(tool, 2, 9, 1, 9, 9, 1, 0, 1024, rc_g2=8)[1:3] == ["256", "128"] and ask(tool, 2, 14, 1, 9, 9, 1, 0, 1024, rc_g2=16)[1:3] == ["128", "256"]


def test_pick_forced_and_refused(tool):
    for v in LANES:
        assert int(ask(tool, 1, 9, 1, 9, 10, 0, 0, 6144, rc=v, rc_g2=8 if v != 8 else 16)[4]) == v
        assert int(ask(tool, 1, 14, 1, 9, 10, 0, 4, 6144, rc=v)[4]) == v and ask(tool, 1, 14, 1, 9, 10, 0, 4, 6144, rc=v)[0] == "wave29_compact"
        assert int(ask(tool, 2, 9, 1, 9, 9, 1, 0, 1024, rc=8 if v != 8 else 16, rc_g2=v)[4]) == v
    # the generic kernels keep their 64 lanes (staged: none), forced or not
    assert int(ask(tool, 1, 9, 0, 7, 7, 0, 0, 512, rc=16)[4]) == 64 and ask(tool, 1, 9, 0, 7, 7, 0, 0, 512, rc=16)[0] == "wave"
    assert int(ask(tool, 2, 14, 0, 5, 5, 0, 0, 64, rc_g2=16)[4]) == 0 and ask(tool, 2, 14, 0, 5, 5, 0, 0, 64, rc_g2=16)[0] == "staged"
    for bad in (1, 4, 24, 48, 128, -16, -1):
        for group, kw in ((1, dict(rc=bad)), (2, dict(rc_g2=bad))):
            f = ask(tool, group, 9, 1, 7, 7, 0, 0, 512, **kw)
            assert int(f[5]) == INVALID and "8, 16, 32 or 64" in f[6], f
        # the other group's switch is not this launch's business
        assert int(ask(tool, 1, 9, 1, 7, 7, 0, 0, 512, rc_g2=bad)[5]) == 0 and int(ask(tool, 2, 9, 1, 7, 7, 0, 0, 512, rc=bad)[5]) == 0


def test_switches_from_the_environment(tool):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ZKMI_")}
    assert tool(["env_lanes"], env=clean) == ["0 0"]
    assert tool(["env_lanes"], env=dict(clean, ZKMI_RC_LANES="16")) == ["16 0"]
    assert tool(["env_lanes"], env=dict(clean, ZKMI_RC_LANES_G2="8")) == ["0 8"]
    # taken as they are, and the pick refuses; a value that is no number or 0 reads as -1, so that it is refused and not taken for "not set"
    assert tool(["env_lanes"], env=dict(clean, ZKMI_RC_LANES="24", ZKMI_RC_LANES_G2="x")) == ["24 -1"]
    assert tool(["env_lanes"], env=dict(clean, ZKMI_RC_LANES="0", ZKMI_RC_LANES_G2="")) == ["-1 -1"]
    assert tool(["env"], env=dict(clean, ZKMI_RC_LANES="16", ZKMI_RC_LANES_G2="8")) == ["1 1 1 0 1 1 512 1"]
