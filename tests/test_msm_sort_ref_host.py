"""tests/msm_sort_ref.py holds what tests/test_gpu_msm_sort.py compares the device against, so it is checked here on its own, without a GPU: the
vectorised digit restatement against the literal one of tests/msm_patterns.py, the crafted inputs against the partition sizes they claim (by the
reference alone), the schedule restatement against the integer definitions, and the hand-written paths of the case table against the restated rules."""
import numpy as np
import pytest

import msm_patterns as P
import msm_sort_ref as R

N_EDGE = 257


@pytest.mark.parametrize("sb", (1, 4, 31, 32, 33, 48, 64))
@pytest.mark.parametrize("c", (12, 13, 15, 16, 17, 20))
def test_vectorised_digits_equal_signed_digits(c, sb):
    """digit_lists == for_each_digit as msm_patterns.signed_digits states it, on the digit-edge set of the width: with and without a table, with a
    table stride, with a drop mask"""
    sc = P.edge_set(c, N_EDGE, sb)
    values = P.ints(sc, sb)
    nb, stride = 1 << (c - 1), N_EDGE + 5
    drop = R.drop_mask(N_EDGE, seed=c * 100 + sb)
    drop[3:9] = False
    for precomp, st, mask in ((False, None, None), (True, None, None), (True, stride, drop), (False, None, drop)):
        want = []
        for i, s in enumerate(values):
            if mask is not None and mask[i]:
                continue
            digits, _ = P.signed_digits(s, c, sb)
            assert sum((-m if neg else m) << (c * w) for w, m, neg in digits) == s
            for w, m, neg in digits:
                want.append(((0 if precomp else w * nb) + m - 1, ((w * (st or N_EDGE) + i) if precomp else i) | (int(neg) << 31)))
        keys, ents = R.digit_lists(sc, N_EDGE, sb, c, precomp, st, mask)
        assert ents.dtype == np.uint32 and len(keys) == len(ents)
        assert sorted(zip(keys.tolist(), ents.tolist())) == sorted(want), (c, sb, precomp)


def _sizes(kind, lb):
    sc = R.scalars_of(kind, 15, 0, 32)
    n = sc.size // 32
    keys, ents = R.digit_lists(sc, n, 32, 15, True)
    return n, keys, ents, R.partition_sizes(keys, 1 << 14, lb)


def test_cap_exact_fills_the_stage_exactly():
    """36 000 pairs in partition 0 of a c = 15 table at lb = 10 and none above the cap elsewhere: no chunk; the largest magnitude is present"""
    n, keys, ents, sizes = _sizes("cap_exact", 10)
    assert n == R.CASE["l-cap-exact"].n == 28000 and len(keys) == 46000
    assert sizes[0] == 36000 == R.PART_CAP[10] and sizes[1:].sum() == 10000 and sizes[1:].max() < 36000 and sizes[1:].min() > 0
    assert keys.max() == (1 << 14) - 1 and not (ents >> 31).any()
    assert R.chunk_count(sizes, 36000) == 0 == R.CASE["l-cap-exact"].chunks


def test_cap_plus_one_overflows_by_one_pair():
    n, keys, _, sizes = _sizes("cap_plus_one", 10)
    assert n == R.CASE["m-cap-plus-one"].n == 28000 and len(keys) == 46000
    assert sizes[0] == 36001 and sizes[1:].sum() == 9999 and sizes[1:].max() < 36000
    assert R.chunk_count(sizes, 36000) == 5 == R.CASE["m-cap-plus-one"].chunks                 # all from partition 0: ceil(36 001 / 8 192)
    # the two inputs differ in exactly one scalar
    a, b = R.scalars_of("cap_exact", 15, 0, 32).reshape(-1, 32), R.scalars_of("cap_plus_one", 15, 0, 32).reshape(-1, 32)
    assert (a != b).any(axis=1).sum() == 1


def test_chunk_edges_partition_sizes():
    """a chunk exactly full, one pair more, empty partitions, a single pair: 11 chunks; partition 0 is one bucket"""
    n, keys, _, sizes = _sizes("chunk_edges", 11)
    assert n == R.CASE["n-chunk-edges"].n == 65538 == len(keys)
    assert tuple(sizes) == R.CHUNK_EDGE_SIZES == (8192, 8193, 0, 1, 16384, 8191, 0, 24577)
    assert R.chunk_count(sizes, 0) == 11 == R.CASE["n-chunk-edges"].chunks
    counts = np.bincount(keys, minlength=1 << 14)
    assert counts[0] == 8192 and counts[1:2048].sum() == 0
    assert (counts[2048:4096] > 0).sum() > 1500                                                  # spread: ~ 4 pairs per bucket


def test_empty_partitions_in_both_modes():
    """an empty partition under the fused level 2 (lb = 10: the all-ones and skew inputs leave most of the 16 empty) and under the chunked one (the
    chunk-edge input, above); and the inputs of case b that must overflow a partition do"""
    for kind in ("ones", "skew"):
        cs = R.CASE[f"b-{kind}"]
        ref = R.case_reference(cs)
        sizes = R.partition_sizes(ref["keys"], ref["total"], 10)
        assert (sizes == 0).any(), kind
    edges = R.partition_sizes(R.case_reference(R.CASE["b-edges"])["keys"], 1 << 14, 10)
    assert sorted(edges)[-2] > 36000 and (edges == 0).sum() == 14 and R.chunk_count(edges, 36000) == 16    # chunk kernels and empty fused partitions in one sort
    skew = R.partition_sizes(R.case_reference(R.CASE["b-skew"])["keys"], 1 << 14, 10)
    assert 35000 < skew.max() <= 36000 and R.chunk_count(skew, 36000) == 0                     # a fused partition a few pairs short of the stage
    uni = R.partition_sizes(R.case_reference(R.CASE["b-uniform"])["keys"], 1 << 14, 10)
    assert uni.max() <= 36000 and uni.min() > 0


def test_drop_mask_empties_a_level_one_tile():
    cs = R.CASE["o-b-uniform"]
    sc, drop = R.case_input(cs)
    assert drop[0] and drop[cs.n - 1] and drop[3072:4096].all() and 0.3 < drop.mean() < 0.5
    ref = R.case_reference(cs)
    idx = (ref["ents"] & 0x7FFFFFFF) % cs.stride
    assert cs.stride == cs.n + 5 and not drop[idx].any() and set(np.unique(idx)) == set(np.nonzero(~drop)[0])
    edges = R.case_reference(R.CASE["o-b-edges"])                                                # entries carry w * stride + i, up to the top window
    assert ((edges["ents"] & 0x7FFFFFFF) // cs.stride).max() == cs.Wd - 1 and ((ref["ents"] & 0x7FFFFFFF) // cs.stride).max() == cs.Wd - 2
    words = np.frombuffer(R.mask_words(drop), "<u4")
    assert len(words) == (cs.n + 31) // 32 and all(((words[i >> 5] >> (i & 31)) & 1) == drop[i] for i in range(0, cs.n, 7))


def test_schedule_restatement():
    """lanes(cnt) = 1 for 0 < cnt < 2 cap, else 2^floor(log2(cnt / cap)); msm_key; the totals — against plain integer definitions"""
    for cap in (8, 16, 64, 256):
        counts = np.array(sorted({0, 1, cap, 2 * cap - 1, 2 * cap, 3 * cap, 4 * cap - 1, 4 * cap, 255 * cap, 256 * cap - 1, 256 * cap, 257 * cap, 7281, 1 << 20}))
        j = R.lanes_log(counts, cap)
        for cnt, jj, key in zip(counts.tolist(), j.tolist(), R.keys_of(counts, cap).tolist()):
            want = 0 if cnt < 2 * cap else (cnt // cap).bit_length() - 1
            assert jj == want and (cnt < 2 * cap or (cap << jj) <= cnt < (cap << (jj + 1)))
            assert key == (cnt if cnt < 2 * cap else 2 * cap - 1 + want)
        m0, m1, m2 = R.schedule_totals(counts, cap)
        assert m0 == sum(1 << jj for cnt, jj in zip(counts.tolist(), j.tolist()) if cnt) and m1 == sum(1 << jj for jj in j.tolist() if jj) and m2 == sum(jj > 7 for jj in j.tolist())
    # the issue's example: all ones at 7 281 terms on a c = 15 table — cap 8, one bucket of 2^9 lanes, a giant
    assert R.lane_cap(7281, 15, 18, True) == 8 and R.lanes_log([7281], 8)[0] == 9 and R.schedule_totals([7281], 8) == (512, 512, 1)


def test_case_table_paths_follow_the_rules():
    """the literal paths of the case table are what the restated rules of csrc/msm_sort.hip give (a typing mistake in the table shows here, before a GPU
    is involved); the thresholds sit where the table says"""
    for cs in R.CASES:
        assert cs.c == (cs.table or cs.bits or R.pick_c(cs.n)), cs
        assert R.path_rules(cs.c, cs.Wd, cs.W, cs.n) == cs.path and R.nw_of(cs.sb) == cs.nw, cs
        assert cs.Wd * cs.n <= 1_200_000
    W = {cs.name: cs.Wd * cs.n for cs in R.CASES}
    assert W["a-uniform"] == 131058 and W["b-uniform"] == 131076 and W["c-8192"] == W["i"] == 1 << 17 and W["c-8191"] < 1 << 17
    assert W["d-28800"] // 16 == 32400 and W["d-28801"] // 16 == 32401
    assert [R.CASE[k].Wd for k in ("k-33", "k-48", "k-64")] == [18, 26, 35] and R.CASE["e"].Wd == 20
    assert R.CASE["g"].path["parts"] == 544 == max(cs.path["parts"] for cs in R.CASES if cs.sb <= 32)
    # ZKMI_RSORT_LB=9: cases b and h are among those that take 2^9-bucket partitions
    for name in ("b-uniform", "h"):
        cs = R.CASE[name]
        assert R.path_rules(cs.c, cs.Wd, cs.W, cs.n, lb_want=9)["lb"] == 9 and R.path_rules(cs.c, cs.Wd, cs.W, cs.n, lb_want=9)["fused_cap"] == 15000


def test_case_table_chunk_counts_are_the_reference_s():
    """every chunk count the case table states is what the reference's partition sizes give under the table's own path"""
    stated = [cs for cs in R.CASES if cs.chunks is not None]
    assert {"b-uniform", "f-uniform252", "f-mostly_ones", "l-cap-exact", "m-cap-plus-one", "n-chunk-edges"} <= {cs.name for cs in stated}
    for cs in stated:
        ref = R.case_reference(cs)
        assert R.chunk_count(R.partition_sizes(ref["keys"], ref["total"], cs.path["lb"]), cs.path["fused_cap"]) == cs.chunks, cs


def test_case_f_shapes():
    """case f (no table: the key carries the window): giants in the witness-like sets, one partition over the cap among fused ones where the table says so,
    an empty last partition"""
    for name, over in (("f-uniform252", []), ("f-uniform", [42]), ("f-witness", []), ("f-mostly_ones", [0])):
        cs = R.CASE[name]
        ref = R.case_reference(cs)
        sizes = R.partition_sizes(ref["keys"], ref["total"], 10)
        assert len(sizes) == 44 and np.nonzero(sizes > 36000)[0].tolist() == over and sizes[43] == 0, name
        cap = R.lane_cap(cs.n, cs.c, cs.Wd, False)
        assert cap == 8 and R.schedule_totals(ref["counts"], cap)[2] > 0, name


# ---- the checker of tests/test_gpu_msm_sort.py, on arrays built here ------------------------------------------------------------------------------------
def model_build(cs, lb, fused_cap):
    """what a correct sort and schedule hand back for a case, built from the reference with numpy: the lists in a scrambled order inside every bucket,
    the buckets ordered by key (descending) for the lanes"""
    ref = R.case_reference(cs)
    counts, total = ref["counts"], ref["total"]
    cap = R.lane_cap(cs.n, cs.c, cs.Wd, bool(cs.table))
    rng = np.random.default_rng(7)
    srt = ref["ents"][np.lexsort((rng.random(len(ref["ents"])), ref["keys"]))]
    j, key = R.lanes_log(counts, cap), R.keys_of(counts, cap)
    order = np.nonzero(counts)[0]
    order = order[np.argsort(-key[order], kind="stable")]
    L = 1 << j[order]
    first = np.concatenate([[0], np.cumsum(L)[:-1]])
    lane_g = np.repeat(order, L)
    lane_sub = np.arange(L.sum()) - np.repeat(first, L)
    giants = [(g, f >> 7, 1 << (jj - 7)) for g, f, jj in zip(order.tolist(), first.tolist(), j[order].tolist()) if jj > 7]
    m = R.schedule_totals(counts, cap)
    a = dict(counts=counts.astype(np.uint32), starts=np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32), sorted=srt, lane_g=lane_g.astype(np.uint32),
             lane_sub=lane_sub.astype(np.uint32), giants=np.array(giants, np.uint32).reshape(-1), meta=np.array(m, np.uint32))
    info = dict(c=cs.c, Wd=cs.Wd, W=cs.W, nb=1 << (cs.c - 1), total=total, cap=cap, nw=cs.nw, radix=1, lb=lb, parts=total >> lb, fused_cap=fused_cap, staged=1,
                chunks=R.chunk_count(R.partition_sizes(ref["keys"], total, lb), fused_cap), entries=len(srt), lanes=m[0], giants=m[2])
    return info, a


def test_checker_accepts_a_correct_build_and_rejects_every_corruption():
    """check_content of tests/test_gpu_msm_sort.py passes on a correct build of case f-witness (single- and multi-lane buckets, two giants) and fails when any one
    thing is off by a single word: so a kernel that is subtly wrong cannot pass it"""
    import test_gpu_msm_sort as T
    cs = R.CASE["f-witness"]
    info, good = model_build(cs, 10, 36000)
    T.check_content(cs, info, good)
    assert good["meta"][2] >= 2 and good["meta"][1] < good["meta"][0]

    def broken(change, info_change=None):
        a = {k: v.copy() for k, v in good.items()}
        change(a)
        with pytest.raises(AssertionError):
            T.check_content(cs, dict(info, **(info_change or {})), a)

    counts = good["counts"].astype(np.int64)
    full = np.nonzero(counts)[0]
    b0, b1 = int(full[0]), int(full[-1])
    s0, s1 = int(good["starts"][b0]), int(good["starts"][b1])

    def move_one(a):
        a["counts"][b0] -= 1
        a["counts"][b1] += 1
    broken(move_one)                                                                       # 1. a count
    broken(lambda a: a["starts"].__setitem__(b1, s1 + 1))                                  # 2. a start
    broken(lambda a: a["sorted"].__setitem__([s0, s1], a["sorted"][[s1, s0]]))             # 3. two entries in each other's bucket
    broken(lambda a: a["sorted"].__setitem__(s0, a["sorted"][s0] ^ 0x80000000))            #    a sign
    broken(lambda a: a["sorted"].__setitem__(s0, a["sorted"][s0 + 1]) if counts[b0] > 1 else a["sorted"].__setitem__(s0, 0))   # a duplicate in place of an entry
    for k in range(3):                                                                     # 4. each total
        broken(lambda a, k=k: a["meta"].__setitem__(k, a["meta"][k] + 1))
    n_multi = int(good["meta"][1])
    broken(lambda a: a["lane_sub"].__setitem__(1, 0))                                      # 5. lane_sub out of order inside the first (giant) group
    broken(lambda a: a["lane_g"].__setitem__(n_multi, a["lane_g"][n_multi + 1]))           #    a bucket on two lanes, another on none
    lanes = len(good["lane_g"])

    def swap_ends(a):                                                                      # 6. the smallest single-lane bucket ahead of a larger one
        a["lane_g"][[n_multi, lanes - 1]] = a["lane_g"][[lanes - 1, n_multi]]
    assert counts[good["lane_g"][n_multi]] > counts[good["lane_g"][lanes - 1]]
    broken(swap_ends)

    def shift_groups(a):                                                                   #    a group of 2^j lanes that no longer begins at a multiple of 2^j
        g = a["lane_g"][:n_multi].copy()
        a["lane_g"][0], a["lane_g"][1:n_multi] = a["lane_g"][n_multi], g[:-1]
        a["lane_g"][n_multi] = g[-1]
    broken(shift_groups)
    broken(lambda a: a["giants"].__setitem__(1, a["giants"][1] + 1))                       # 7. a giant's first block
    broken(lambda a: a["giants"].__setitem__(2, a["giants"][2] * 2))                       #    ... its number of blocks
    broken(lambda a: a["giants"].__setitem__(slice(0, 3), a["giants"][3:6]))               #    one giant twice
    broken(lambda a: None, dict(chunks=info["chunks"] + 1))                                # 9. the chunk count
    broken(lambda a: None, dict(cap=16))
