"""A numpy restatement of the front half of every MSM, csrc/msm_sort.hip: msm_sort — the signed-digit recoding of the scalars into per-bucket lists
(csrc/msm.cuh: for_each_digit, k_msm_count / k_rsort_*) and the lane schedule built over them (k_msm_classify / k_msm_assign) — together with the rules by
which msm_sort picks one of its sorts, the inputs that sit on each side of every such rule, and the case table that tests/test_gpu_msm_sort.py runs through
zkmi_msm_sort_probe_dev (include/zkmi_diag.h). Plain helpers, no fixtures; tests/test_msm_sort_ref_host.py checks this file without a GPU.

All of it is integer work: what the device must build is known exactly, up to the order of the entries inside one bucket."""
import hashlib
import json

import numpy as np

import msm_patterns as P
import synth

# csrc/msm.cuh
RSORT_LOW_BITS, RSORT_TILE, RSORT_CHUNK, RSORT_MAX_PARTS = 11, 1024, 8192, 4096
MSM_MAX_CAP = 256
# csrc/msm_host.hpp: a bucket with more than 2^MSM_LOG_TB lanes is a giant
MSM_LOG_TB = 7
# csrc/msm_sort.hip: rsort_part_cap, and the LDS a level-1 block may ask for on gfx950 (rsort_staged_fits)
PART_CAP = {10: 36000, 9: 15000}
STAGE_LDS_LIMIT = 156 * 1024


def pick_c(n):
    """csrc/msm_host.hpp: msm_pick_c"""
    lg = max(n, 1).bit_length() - 1
    if n > (3 << lg) // 2:
        lg += 1
    return (2, 2, 2, 3, 3, 4, 4, 5, 6, 7, 8, 9, 9, 10, 11, 11, 12, 15, 15, 15, 15, 15, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16)[min(lg, 31)]


# ---- the digits -------------------------------------------------------------------------------------------------------------------------------------
def digit_lists(sc, n, sb, c, precomp, stride=None, drop=None):
    """for_each_digit over n scalars of sb bytes (a uint8 array of n*sb bytes), any sb in 1..64 and any c: the flat keys
    g = (precomp ? 0 : w*nb) + mag - 1 and the entries (precomp ? w*stride + i : i) | sign << 31 of every non-zero digit of every scalar that
    drop (optional, bool per scalar) does not leave out. Returns (keys int64, entries uint32), in no particular order."""
    Wd, nb, half = P.digits_of(sb, c), 1 << (c - 1), 1 << (c - 1)
    stride = n if not stride else stride
    bits = np.unpackbits(np.frombuffer(bytes(sc), np.uint8).reshape(n, sb), axis=1, bitorder="little")
    if Wd * c > 8 * sb:
        bits = np.concatenate([bits, np.zeros((n, Wd * c - 8 * sb), np.uint8)], axis=1)
    weights = (1 << np.arange(c, dtype=np.int64))
    keep = np.ones(n, bool) if drop is None else ~np.asarray(drop, bool)
    idx_all = np.arange(n, dtype=np.int64)
    carry = np.zeros(n, np.int64)
    keys, ents = [], []
    for w in range(Wd):
        raw = bits[:, w * c:(w + 1) * c].astype(np.int64) @ weights + carry
        neg = raw > half
        mag = np.where(neg, (1 << c) - raw, raw)
        carry = neg.astype(np.int64)
        sel = (mag != 0) & keep
        i = idx_all[sel]
        keys.append((0 if precomp else w * nb) + mag[sel] - 1)
        ents.append((((w * stride + i) if precomp else i) | (neg[sel].astype(np.int64) << 31)).astype(np.uint32))
    return np.concatenate(keys), np.concatenate(ents)


def partition_sizes(keys, total, lb):
    """pairs per level-1 partition (g >> lb) of the radix sort"""
    return np.bincount(keys >> lb, minlength=total >> lb)


def chunk_count(sizes, fused_cap):
    """csrc/msm.cuh: k_rsort_chunks — ceil(size / 8192) chunks for every partition above fused_cap, for every partition when fused_cap is 0"""
    sizes = np.asarray(sizes, np.int64)
    cut = sizes > fused_cap if fused_cap else np.ones(len(sizes), bool)
    return int(((sizes[cut] + RSORT_CHUNK - 1) // RSORT_CHUNK).sum())


# ---- the lane schedule ------------------------------------------------------------------------------------------------------------------------------
def lane_cap(n, c, Wd, precomp):
    """csrc/msm_sort.hip: msm_sort — list entries per lane (without the ZKMI_CAP override)"""
    nb = 1 << (c - 1)
    avg = ((Wd if precomp else 1) * n + nb - 1) // nb
    cap_big, cap_fill = 16, 8
    while cap_big < 2 * avg and cap_big < MSM_MAX_CAP:
        cap_big <<= 1
    while 2 * cap_fill <= Wd * n // 250000 and cap_fill < MSM_MAX_CAP:
        cap_fill <<= 1
    return min(cap_big, cap_fill)


def lanes_log(counts, cap):
    """j per bucket: a bucket of cnt entries gets 2^j lanes, j = 0 while cnt < 2*cap, else floor(log2(cnt / cap)) (integer arithmetic throughout)"""
    counts = np.asarray(counts, np.int64)
    q = counts // cap
    j = np.zeros(len(counts), np.int64)
    for k in range(1, 32):
        j += q >= (1 << k)
    return np.where(counts < 2 * cap, 0, j)


def keys_of(counts, cap):
    """csrc/msm.cuh: msm_key — 0 for an empty bucket, the size of a single-lane bucket, 2*cap - 1 + j for one of 2^j lanes"""
    counts = np.asarray(counts, np.int64)
    return np.where(counts < 2 * cap, counts, 2 * cap - 1 + lanes_log(counts, cap))


def schedule_totals(counts, cap):
    """meta[0..2]: all lanes, lanes of multi-lane buckets, giants"""
    counts = np.asarray(counts, np.int64)
    j = lanes_log(counts, cap)
    lanes = np.where(counts > 0, 1 << j, 0)
    return int(lanes.sum()), int(lanes[j >= 1].sum()), int((j > MSM_LOG_TB).sum())


# ---- which sort msm_sort takes ------------------------------------------------------------------------------------------------------------------------
def nw_of(sb):
    return 1 if sb <= 4 else 8 if sb <= 32 else 16


def path_rules(c, Wd, W, n, radix_on=True, fused_on=True, staged_on=True, lb_want=10):
    """csrc/msm_sort.hip on gfx950: msm_use_radix, rsort_low_bits, the staged / direct choice of msm_launch_digits_radix; the keyword arguments are the
    four switches ZKMI_RSORT, ZKMI_RSORT_FUSED, ZKMI_RSORT_STAGED, ZKMI_RSORT_LB."""
    total, entries = W << (c - 1), Wd * n
    if not (radix_on and c > RSORT_LOW_BITS and (total >> RSORT_LOW_BITS) <= RSORT_MAX_PARTS and entries >= 1 << 17):
        return dict(radix=0, lb=0, parts=0, fused_cap=0, staged=0)
    lb = RSORT_LOW_BITS
    if fused_on and lb_want in PART_CAP and c > lb_want and 1 <= (total >> lb_want) <= RSORT_MAX_PARTS and entries // (total >> lb_want) <= PART_CAP[lb_want] * 9 // 10:
        lb = lb_want
    parts, stage = total >> lb, Wd * RSORT_TILE
    staged = staged_on and (2 * parts + 1024 + 2 * stage) * 4 <= STAGE_LDS_LIMIT and stage >= 8 * parts
    return dict(radix=1, lb=lb, parts=parts, fused_cap=PART_CAP.get(lb, 0), staged=int(staged))


# ---- the crafted inputs -------------------------------------------------------------------------------------------------------------------------------
def _pack(values, sb=32):
    """integers below 2^64 as sb-byte little-endian scalars"""
    b = np.ascontiguousarray(np.asarray(values).astype("<u8")).reshape(-1, 1).view(np.uint8)
    out = np.zeros((len(b), sb), np.uint8)
    out[:, :min(sb, 8)] = b[:, :min(sb, 8)]
    return out.reshape(-1)


def cap_exact(one_more, seed=0xCA9):
    """28 000 scalars for a c = 15 table whose partition 0 (g >> 10 == 0: magnitudes 1..1024) receives exactly 36 000 pairs — the LDS stage of k_rsort_part
    exactly full — or, with one_more, 36 001: 18 000 scalars a + b*2^15, a, b in [1, 1024] (two digits, both in partition 0) and 10 000 of one digit in
    [1 025, 16 384], the largest magnitude 16 384 among them; one_more turns the last of those into a digit in [1, 1024]."""
    rng = np.random.default_rng(seed)
    two = rng.integers(1, 1025, 18000) + (rng.integers(1, 1025, 18000) << 15)
    one = rng.integers(1025, 16385, 10000)
    one[0] = 16384
    low = 1 + int(rng.integers(0, 1024))
    if one_more:
        one[-1] = low
    v = np.concatenate([two, one])
    return _pack(v[rng.permutation(len(v))])


CHUNK_EDGE_SIZES = (8192, 8193, 0, 1, 16384, 8191, 0, 24577)


def chunk_edges(seed=0xC4E):
    """65 538 scalars of one digit each for a c = 15 table (chunked level 2, 2^11-bucket partitions): partition p = g >> 11 receives CHUNK_EDGE_SIZES[p]
    pairs — a chunk exactly full, one pair more, none, one, two full chunks, one pair short of one, none, three chunks and one pair. Partition 0's pairs
    all meet in bucket 0; the others are spread over their partition."""
    rng = np.random.default_rng(seed)
    mags = [np.ones(CHUNK_EDGE_SIZES[0], np.int64)]
    for p in range(1, 8):
        mags.append(1 + p * 2048 + rng.integers(0, 2048, CHUNK_EDGE_SIZES[p]))
    v = np.concatenate(mags)
    return _pack(v[rng.permutation(len(v))])


def drop_mask(n, seed=0xD60):
    """bool per scalar: a random third, every scalar of level-1 tile 3, scalar 0 and scalar n - 1"""
    m = np.random.default_rng(seed).integers(0, 3, n) == 0
    m[3 * RSORT_TILE:4 * RSORT_TILE] = True
    m[0] = m[n - 1] = True
    return m


def mask_words(drop):
    """the device bitmap of a drop mask: bit i & 31 of word i >> 5"""
    return np.packbits(np.asarray(drop, np.uint8), bitorder="little").tobytes().ljust((len(drop) + 31) // 32 * 4, b"\0")


def top_bit_set(n, sb):
    """uniform bytes with the top bit of every scalar set (tests/test_gpu_parity.py: test_msm_scalar_widths_large): a carry out of the last whole window"""
    raw = synth.elems(0xABC + sb, (n * sb + 31) // 32 + 1)[:n * sb].copy()
    raw[sb - 1::sb] |= 0x80
    return raw


def scalars_of(kind, c, n, sb):
    if kind == "uniform":
        return P.scalars("uniform", c, n, sb, seed=P.UNIFORM_SEED + c + n)
    if kind == "edges":
        return P.edge_set(c, n, sb)
    if kind == "skew":
        return P.skew_set(c, n)
    if kind == "ones":
        return _pack(np.ones(n, np.int64), sb)
    if kind == "uniform252":                                                  # uniform below 2^252: the top window of a c = 12 recoding holds the carry alone
        return synth.elems(P.UNIFORM_SEED + c + n, n, mask_top=0x0F)
    if kind == "witness":
        return synth.witness_like(0x517E55, n)
    if kind == "mostly_ones":                                                 # a witness of which three quarters are the value 1: bucket 0 alone is over the fused cap
        w = synth.witness_like(0x517E55, n).reshape(n, 32).copy()
        w[np.arange(n) % 4 != 0] = 0
        w[np.arange(n) % 4 != 0, 0] = 1
        return w.reshape(-1)
    if kind == "topbit":
        return top_bit_set(n, sb)
    if kind == "cap_exact":
        return cap_exact(False)
    if kind == "cap_plus_one":
        return cap_exact(True)
    if kind == "chunk_edges":
        return chunk_edges()
    raise ValueError(kind)


# ---- the case table -----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One sort: `table` = precomp_c (0: none), `bits` = zkmi_msm_set_window_bits (0: msm_pick_c), the scalar kind, and the LITERAL path the default
    process must report on gfx950 (radix, lb, parts, fused_cap, staged, nw) — written out by hand from the rules, not computed, so that a tuning change
    that moves a case off its branch fails the test; chunks = None: whatever the reference's partition sizes give."""

    def __init__(self, name, table, bits, n, sb, kind, c, radix, lb=0, parts=0, fused_cap=0, staged=0, nw=8, chunks=None, masked=False):
        self.name, self.table, self.bits, self.n, self.sb, self.kind, self.c, self.masked = name, table, bits, n, sb, kind, c, masked
        self.path = dict(radix=radix, lb=lb, parts=parts, fused_cap=fused_cap, staged=staged)
        self.nw, self.chunks = nw, chunks
        self.Wd = P.digits_of(sb, c)
        self.W = 1 if table else self.Wd
        self.stride = n + 5 if masked else 0

    def __repr__(self):
        return self.name


def _cases():
    out = []
    four = ("uniform", "edges", "skew", "ones")
    for kind in four:                                                         # a: 18 * 7 281 = 131 058 < 2^17
        out.append(Case(f"a-{kind}", 15, 0, 7281, 32, kind, 15, radix=0))
    for kind in four:                                                         # b: 131 076 >= 2^17; the last tile holds 114 scalars
        out.append(Case(f"b-{kind}", 15, 0, 7282, 32, kind, 15, radix=1, lb=10, parts=16, fused_cap=36000, staged=1, chunks=0 if kind == "uniform" else None))
    out.append(Case("c-8191", 17, 0, 8191, 32, "uniform", 17, radix=0))      # c: Wd * n == 2^17 exactly at 8 192
    out.append(Case("c-8192", 17, 0, 8192, 32, "uniform", 17, radix=1, lb=10, parts=64, fused_cap=36000, staged=1))
    out.append(Case("d-28800", 15, 0, 28800, 32, "uniform", 15, radix=1, lb=10, parts=16, fused_cap=36000, staged=1))      # d: entries / partitions == 0.9 cap
    out.append(Case("d-28801", 15, 0, 28801, 32, "uniform", 15, radix=1, lb=11, parts=8, fused_cap=0, staged=1))            # ... and one past it
    out.append(Case("e", 13, 0, 6554, 32, "uniform", 13, radix=1, lb=11, parts=2, fused_cap=0, staged=0))                    # e: Wd = 20 does not fit the staging LDS
    # f: no table; msm_pick_c(49 153) = 12, W = Wd = 22: the key carries the window. Uniform scalars below 2^252 leave every partition under the cap; uniform
    # 253-bit ones (synth.elems) send three quarters of the top window's digits, magnitudes 1 and 2, into one partition: 37 047 pairs, 5 chunks, the partition
    # after it empty (the carry into the top window makes a giant of its bucket 0 in both); the witness-like set has giants and no partition over the cap; with three quarters of the scalars equal to 1, window 0's first partition is
    # a chunked one among fused ones
    for kind, chunks in (("uniform252", 0), ("uniform", 5), ("witness", 0), ("mostly_ones", 6)):
        out.append(Case(f"f-{kind}", 0, 0, 49153, 32, kind, 12, radix=1, lb=10, parts=44, fused_cap=36000, staged=0, chunks=chunks))
    out.append(Case("g", 0, 16, 7711, 32, "uniform", 16, radix=1, lb=10, parts=544, fused_cap=36000, staged=1))              # g: the largest P the product reaches
    out.append(Case("h", 20, 0, 10083, 32, "uniform", 20, radix=1, lb=10, parts=512, fused_cap=36000, staged=1))             # h: the main table width
    out.append(Case("i", 20, 0, 65536, 4, "uniform", 20, radix=1, lb=10, parts=512, fused_cap=36000, staged=0, nw=1))        # i: Wd * 1024 < 8 P: direct
    out.append(Case("j", 15, 0, 43691, 4, "uniform", 15, radix=1, lb=10, parts=16, fused_cap=36000, staged=1, nw=1))
    out.append(Case("k-33", 0, 15, 7282, 33, "topbit", 15, radix=1, lb=10, parts=288, fused_cap=36000, staged=1, nw=16))    # k: the NW = 16 kernels
    out.append(Case("k-48", 0, 15, 5042, 48, "topbit", 15, radix=1, lb=10, parts=416, fused_cap=36000, staged=0, nw=16))
    out.append(Case("k-64", 0, 15, 3745, 64, "topbit", 15, radix=1, lb=10, parts=560, fused_cap=36000, staged=0, nw=16))
    out.append(Case("l-cap-exact", 15, 0, 28000, 32, "cap_exact", 15, radix=1, lb=10, parts=16, fused_cap=36000, staged=1, chunks=0))
    out.append(Case("m-cap-plus-one", 15, 0, 28000, 32, "cap_plus_one", 15, radix=1, lb=10, parts=16, fused_cap=36000, staged=1, chunks=5))
    out.append(Case("n-chunk-edges", 15, 0, 65538, 32, "chunk_edges", 15, radix=1, lb=11, parts=8, fused_cap=0, staged=1, chunks=11))
    for kind in four:                                                         # o: a and b again with a drop mask and table_stride = n + 5
        out.append(Case(f"o-a-{kind}", 15, 0, 7281, 32, kind, 15, radix=0, masked=True))
        out.append(Case(f"o-b-{kind}", 15, 0, 7282, 32, kind, 15, radix=1, lb=10, parts=16, fused_cap=36000, staged=1, masked=True))
    return out


CASES = _cases()
CASE = {cs.name: cs for cs in CASES}

_inputs, _refs = {}, {}


def case_input(cs):
    """(scalars as a uint8 array, drop mask as bool per scalar or None) of a case, built once"""
    if cs.name not in _inputs:
        sc = np.ascontiguousarray(scalars_of(cs.kind, cs.c, cs.n, cs.sb))
        assert sc.dtype == np.uint8 and sc.size == cs.n * cs.sb, (cs.name, sc.size)
        _inputs[cs.name] = (sc, drop_mask(cs.n) if cs.masked else None)
    return _inputs[cs.name]


def case_reference(cs):
    """the reference's lists of a case, computed once and shared by every test that needs them: keys, entries, counts (per bucket), order (the
    lexsort of the entries by (bucket, entry))"""
    if cs.name not in _refs:
        sc, drop = case_input(cs)
        keys, ents = digit_lists(sc, cs.n, cs.sb, cs.c, bool(cs.table), cs.stride, drop)
        total = cs.W << (cs.c - 1)
        order = np.lexsort((ents, keys))
        ref = dict(keys=keys[order], ents=ents[order], counts=np.bincount(keys, minlength=total).astype(np.int64), total=total)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[cs.name] = ref
    return _refs[cs.name]


# ---- running the probe --------------------------------------------------------------------------------------------------------------------------------
INFO_FIELDS = ("c", "Wd", "W", "nb", "total", "cap", "nw", "radix", "lb", "parts", "fused_cap", "staged", "chunks", "entries", "lanes", "giants")
ARRAYS = ("counts", "starts", "sorted", "lane_g", "lane_sub", "giants", "meta")


def run_probe(cs):
    """zkmi_msm_sort_probe_dev over a case: a first call without arrays for the sizes, a second one that fetches them. Returns (info dict, arrays dict)."""
    import ctypes as C
    from snarkjs_amd import zkmi
    L = zkmi.lib()
    sc, drop = case_input(cs)
    d_s = zkmi.DeviceBuffer.from_host(sc)
    d_m = zkmi.DeviceBuffer.from_host(np.frombuffer(mask_words(drop), np.uint8)) if drop is not None else None
    info = zkmi.MsmSortInfo()
    args = (d_s.ptr, cs.n, cs.sb, cs.table, cs.stride, d_m.ptr if d_m else None)
    try:
        zkmi.check(L.zkmi_msm_set_window_bits(cs.bits))
        zkmi.check(L.zkmi_msm_sort_probe_dev(*args, None, None, 0, None, 0, None, None, 0, None, 0, None, C.byref(info)))
        a = dict(counts=np.zeros(info.total, np.uint32), starts=np.zeros(info.total, np.uint32), sorted=np.zeros(info.entries, np.uint32),
                 lane_g=np.zeros(info.lanes, np.uint32), lane_sub=np.zeros(info.lanes, np.uint32), giants=np.zeros(3 * info.giants, np.uint32), meta=np.zeros(3, np.uint32))
        zkmi.check(L.zkmi_msm_sort_probe_dev(*args, zkmi.ptr(a["counts"]), zkmi.ptr(a["starts"]), info.total, zkmi.ptr(a["sorted"]), info.entries, zkmi.ptr(a["lane_g"]),
                                             zkmi.ptr(a["lane_sub"]), info.lanes, zkmi.ptr(a["giants"]), info.giants, zkmi.ptr(a["meta"]), C.byref(info)))
    finally:
        L.zkmi_msm_set_window_bits(0)
        d_s.free()
        if d_m:
            d_m.free()
    return {k: int(getattr(info, k)) for k in INFO_FIELDS}, a


def digest(arrays):
    h = hashlib.sha256()
    for k in ARRAYS:
        h.update(np.ascontiguousarray(arrays[k], np.uint32).tobytes())
    return h.hexdigest()


def child_main(out_dir):
    """Every case in this process (one GPU process: the switches of csrc/msm_sort.hip are read once per process). One line per case: `sort <name> <info as
    JSON> <sha256 of the arrays> <file that holds them>`."""
    import os
    from snarkjs_amd import zkmi
    zkmi.init(0)
    for cs in CASES:
        info, a = run_probe(cs)
        path = os.path.join(out_dir, cs.name + ".npz")
        np.savez(path, **a)
        print("sort", cs.name, json.dumps(info, separators=(",", ":")), digest(a), path, flush=True)
    print("sort cases done", flush=True)
