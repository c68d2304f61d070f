"""Inputs that place a chosen point in a chosen bucket of an MSM, what every stage behind the bucket accumulation must then hold, and a count of
the rare branches each stage takes on them (plain helpers, no fixtures).

The back half of an MSM (csrc/msm_host.hpp: msm_accumulate's k_msm_tree / k_msm_giant, then msm_reduce) adds buckets to row and column sums and
those to weighted sums. Its additions have hand-written branches for equal operands (a doubling), opposite operands (the result is the point at
infinity) and operands at infinity. Uniform scalars over distinct bases never take them. Here the bases are D * G for discrete logarithms D that
the test chooses (zkmi_gen_bases_from_scalars_dev) and the scalar of a term is one digit, m = bucket + 1 (<< c * window without a table), so
term i lands in one bucket and nowhere else. Everything expected is arithmetic mod r on the logarithms: a value v stands for the point v * G and
0 for the point at infinity.

A pattern is a list of terms (window, bucket, logarithm); bucket = row << cbits | column as msm_reduce cuts the 2^(c-1) buckets."""
import functools
import json
import os

import numpy as np

import msm_patterns as P

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERNS = ("constant", "alternate_fine", "alternate_coarse", "alternate_rows", "cancelled", "one_per_row", "generic")
CLASSES = ("first", "generic", "doubling", "cancel", "skipped")      # skipped: the operand is the point at infinity


@functools.lru_cache(None)
def order(name):
    return int(json.load(open(os.path.join(HERE, "golden", f"{name}_kernel_vectors.json")))["r"])


def _logs(seed, n, r):
    """n distinct non-zero logarithms, none the negation of another"""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        for row in rng.integers(0, 1 << 62, size=(n - len(out), 5), dtype=np.int64).tolist():
            v = (row[0] | row[1] << 62 | row[2] << 124 | row[3] << 186 | row[4] << 248) % r
            if v and v not in seen and r - v not in seen:
                seen.add(v)
                out.append(v)
    return out


def coarse_bits(c):
    """the bit of the column / row index whose value is the sign of alternate_coarse: bit 6 where the index has one (a lane of the wave sums, which adds
    every 64th bucket, then sees P, -P, P ...), else the top bit (the two halves of the sum cancel at the last level of the tree)"""
    rbits, cbits = P.grid_bits(c)
    return min(6, rbits - 1), min(6, cbits - 1)


def pattern(kind, c, r, max_terms, window=0, limit=None, seed=0):
    """The terms of one window. max_terms: how many terms the MSM may have (cancelled thins out to fit); limit: buckets at and above it are left
    empty (the top window of a scalar holds fewer than c bits)."""
    rbits, cbits = P.grid_bits(c)
    R, C = 1 << rbits, 1 << cbits
    nb = R * C
    lim = nb if limit is None else min(limit, nb)
    neg = lambda s: r - 1 if s & 1 else 1
    if kind == "constant":
        t = [(b, 1) for b in range(nb)]
    elif kind == "alternate_fine":
        t = [(b, neg((b >> cbits) + (b & (C - 1)))) for b in range(nb)]
    elif kind == "alternate_coarse":
        rb, cb = coarse_bits(c)
        t = [(b, neg(((b >> cbits) >> rb) + ((b & (C - 1)) >> cb))) for b in range(nb)]
    elif kind == "alternate_rows":                                                 # the row sums are 2^cbits G and its negation in turn: the weighted sums cancel
        t = [(b, neg(b >> cbits)) for b in range(nb)]
    elif kind == "cancelled":
        corners = {0: 0, C - 1: 1, (R - 1) << cbits: 2, nb - 1: 3}                  # first and last place of the first and last row and column
        step = 1
        while (2 * nb - 4 if step == 1 else 2 * nb // step + 4) > max_terms:
            step *= 2
        d = _logs(0xCA2C + seed + c, nb // step + 4, r)
        t, k = [(b, d[i]) for b, i in corners.items()], 4
        for b in range(nb):
            if b not in corners and ((b >> cbits) + (b & (C - 1))) % step == 0:
                t += [(b, d[k]), (b, r - d[k])]
                k += 1
    elif kind == "one_per_row":
        d = _logs(0x09E2 + seed + c, R, r)
        t = [((i << cbits) + min((0, 63, 64, C - 1)[i % 4], C - 1), d[i]) for i in range(R)]
    elif kind == "generic":
        rng = np.random.default_rng(0x6E2C + seed + c)
        where = sorted(set(rng.choice(nb, size=min(nb, 384), replace=False).tolist()) | {0, nb - 1})
        t = list(zip(where, _logs(0x6E2D + seed + c, len(where), r)))
    else:
        raise ValueError(kind)
    t = [(window, b, v) for b, v in t if b < lim]
    assert 0 < len(t) <= max_terms, (kind, c, len(t), max_terms)
    return t


def fat(c, r, cap, same_sign, j_small=3):
    """Two buckets whose lists are spread over several lanes: 2^j_small * cap copies of one base in the middle of the grid (k_msm_tree folds the lane
    partials) and 256 * cap copies in the last bucket (more than one tree block: k_msm_giant finishes it). same_sign: every lane partial is the same
    point; else every second copy is the negation and a lane's share sums to infinity (while it holds as many of the one as of the other)."""
    nb = 1 << (c - 1)
    t = []
    for b, copies, d in ((nb // 2 + 5, cap << j_small, 3), (nb - 1, 256 * cap, 5)):
        t += [(0, b, d if same_sign or not (k & 1) else r - d) for k in range(copies)]
    return t + [(0, 0, 7), (0, nb - 2, 11)]                                         # and two plain buckets beside them


def scalars_of(terms, c, sb):
    """one digit per term: (bucket + 1) << c * window"""
    for w, b, _ in terms:
        assert (b + 1) << (c * w) < 1 << (8 * sb) and 1 <= b + 1 <= 1 << (c - 1)
    return np.frombuffer(b"".join(((b + 1) << (c * w)).to_bytes(sb, "little") for w, b, _ in terms), np.uint8).copy()


def logs_of(terms):
    return P.logs_bytes([v for _, _, v in terms])


def expected(terms, c, W, r):
    """-> (V, counts, rows, cols, k): V[w * nb + b] the bucket sums and counts the entries per bucket; rows[w][i], cols[w][i] the row and column sums;
    k the logarithm of the result, sum over the windows of 2^(c w) sum (b + 1) V[b]"""
    rbits, cbits = P.grid_bits(c)
    R, C = 1 << rbits, 1 << cbits
    nb = R * C
    V, counts = [0] * (W * nb), [0] * (W * nb)
    for w, b, v in terms:
        V[w * nb + b] = (V[w * nb + b] + v) % r
        counts[w * nb + b] += 1
    rows, cols, k = [], [], 0
    for w in range(W):
        Vw = V[w * nb:(w + 1) * nb]
        rows.append([sum(Vw[i * C:(i + 1) * C]) % r for i in range(R)])
        cols.append([sum(Vw[i::C]) % r for i in range(C)])
        k += sum((b + 1) * v for b, v in enumerate(Vw)) << (c * w)
    return V, counts, rows, cols, k % r


def rowcol_layout(rows, cols, c):
    """the order of msm_reduce's array: ((w * 2 + kind) << cbits) + i, rows beyond 2^rbits at infinity"""
    rbits, cbits = P.grid_bits(c)
    out = []
    for rw, cw in zip(rows, cols):
        out += rw + [0] * ((1 << cbits) - len(rw)) + cw
    return out


# ---- the branch counter -------------------------------------------------------------------------------------------------------------------------------
class Tally(dict):
    def __init__(self):
        super().__init__({k: 0 for k in CLASSES})


def _add(acc, p, r, tally, live=None):
    """acc += p element by element on object arrays of logarithms, every addition classified; live (optional): where an addition takes place at all"""
    live = np.ones(acc.shape, bool) if live is None else live
    az, pz = acc == 0, p == 0
    s = (acc + p) % r
    both = live & ~az & ~pz
    dbl, can = both & (acc == p), both & (s == 0)
    tally["skipped"] += int((live & pz).sum())
    tally["first"] += int((live & az & ~pz).sum())
    tally["doubling"] += int(dbl.sum())
    tally["cancel"] += int(can.sum())
    tally["generic"] += int((both & ~dbl & ~can).sum())
    return np.where(live, s, acc)


def _obj(x, shape):
    a = np.empty(len(x), object)
    a[:] = x
    return a.reshape(shape)


def _tree_up(acc, r, tally, width):
    """acc[.., t] += acc[.., t + d] for t a multiple of 2 d, d = 1, 2, 4 .. width / 2 (the wave sums and k_msm_tree pair this way)"""
    d = 1
    while d < width:
        idx = np.arange(0, width, 2 * d)
        acc[..., idx] = _add(acc[..., idx], acc[..., idx + d], r, tally)
        d *= 2
    return acc


def _tree_down(acc, r, tally, width):
    """acc[.., t] += acc[.., t + d] for t < d, d = width / 2 .. 1 (k_msm_giant, k_msm_bitsums)"""
    d = width // 2
    while d >= 1:
        acc[..., :d] = _add(acc[..., :d], acc[..., d:2 * d], r, tally)
        d //= 2
    return acc


def _strided(X, live, lanes, r, tally):
    """lane l of `lanes` adds the elements l, l + lanes, ... of every sum (X: sums x elements); returns sums x lanes"""
    S, cnt = X.shape
    steps = -(-cnt // lanes)
    pad = steps * lanes - cnt
    if pad:
        X = np.concatenate([X, _obj([0] * (S * pad), (S, pad))], axis=1)
        live = np.concatenate([live, np.zeros((S, pad), bool)], axis=1)
    acc = _obj([0] * (S * lanes), (S, lanes))
    for k in range(steps):
        acc = _add(acc, X[:, k * lanes:(k + 1) * lanes], r, tally, live[:, k * lanes:(k + 1) * lanes])
    return acc


def staged_lanes(c, group):
    """csrc/msm_host.hpp: msm_reduce, the staged form: lanes per sum and partials per fold"""
    _, cbits = P.grid_bits(c)
    seq, max_l, fold = (4, 256, 4) if group == 2 else (16, 64, 8)
    L = 1
    while L < max_l and ((1 << cbits) // L) > seq:
        L <<= 1
    return L, fold


def count_rowcol(Vw, counts_w, c, r, form, group=1):
    """The additions of the row and column sums of ONE window (Vw, counts_w: its 2^(c-1) buckets) in the order the kernel of `form` makes them —
    "wave": k_msm_rowcol_wave29 / _wave29_g2 / _wave, shares strided by 64 and a 6-level tree; "staged": k_msm_rowcol with L lanes, then k_msm_fold K at a
    time. A bucket without entries is not an addition (the kernels test counts[g] first); one with entries that sums to infinity is a skipped operand.
    Returns (tally, rows, cols)."""
    rbits, cbits = P.grid_bits(c)
    R, C = 1 << rbits, 1 << cbits
    X, live = _obj(Vw, (R, C)), np.asarray(counts_w).reshape(R, C) > 0
    tally, sums = Tally(), []
    for M, lv in ((X, live), (X.T.copy(), live.T.copy())):
        if form == "wave":
            assert rbits >= 6 and cbits >= 6
            acc = _tree_up(_strided(M, lv, 64, r, tally), r, tally, 64)
        else:
            L, fold = staged_lanes(c, group)
            acc, parts = _strided(M, lv, L, r, tally), L
            while parts > 1:
                K = min(parts, fold)
                parts //= K
                acc = acc.reshape(M.shape[0], parts, K)
                out = acc[:, :, 0].copy()
                for k in range(1, K):
                    out = _add(out, acc[:, :, k], r, tally)
                acc = out
        sums.append([int(v) for v in acc[:, 0]])
    return tally, sums[0], sums[1]


def count_bitsums(arrays, c, r, block=256):
    """k_msm_bitsums / _lds over arrays of 2^cbits sums: one block per (array, k), T_k = sum of the elements whose index has bit k set (k = cbits: all),
    threads strided by the block, then a tree"""
    _, cbits = P.grid_bits(c)
    C = 1 << cbits
    tally = Tally()
    X = _obj([v for a in arrays for v in a], (len(arrays), C))
    for k in range(cbits + 1):
        live = np.broadcast_to((np.arange(C) >> k) & 1 == 1 if k < cbits else np.ones(C, bool), X.shape)
        _tree_down(_strided(X, live, block, r, tally), r, tally, block)
    return tally


def count_wsum(arrays, r):
    """k_msm_wsum over arrays of at most one block's length (level 0, no carried-in sums): an inclusive suffix scan in which every lane adds the lane d
    further on (infinity beyond the end), d = 1, 2, 4 ..., then a tree over the suffix sums of the lanes 1 and up"""
    tally = Tally()
    S, n = len(arrays), len(arrays[0])
    assert n & (n - 1) == 0 and n <= 128
    X = _obj([v for a in arrays for v in a], (S, n))
    d = 1
    while d < n:
        X = _add(X, np.concatenate([X[:, d:], _obj([0] * (S * d), (S, d))], axis=1), r, tally)
        d *= 2
    Y = X.copy()
    Y[:, 0] = 0
    Y = _tree_down(Y, r, tally, n)
    return tally, [int(v) for v in Y[:, 0]], [int(v) for v in X[:, 0]]


def count_tree(partials, r):
    """k_msm_tree over the 2^j lane partials of one bucket (pairs inside blocks of 128 lanes), then k_msm_giant over the block partials when there
    is more than one block: thread t of 128 adds every 128th, then a tree over all 128 threads. Returns (tally, the bucket)."""
    n, tally = len(partials), Tally()
    assert n >= 2 and n & (n - 1) == 0
    blocks = max(n // 128, 1)
    acc = _tree_up(_obj(list(partials), (blocks, n // blocks)), r, tally, n // blocks)[:, 0].reshape(1, blocks)
    if blocks == 1:
        return tally, int(acc[0, 0])
    g = _tree_down(_strided(acc, np.ones(acc.shape, bool), 128, r, tally), r, tally, 128)
    return tally, int(g[0, 0])


def lane_partials(logs, cnt_lanes, r):
    """the shares of k_msm_accum's lanes over ONE bucket's list in the order given: chunk = ceil(cnt / lanes) entries each"""
    chunk = -(-len(logs) // cnt_lanes)
    return [sum(logs[k * chunk:(k + 1) * chunk]) % r for k in range(cnt_lanes)]


# ---- the sets the suite ran before: their buckets, from the digits ----------------------------------------------------------------------------------
def buckets_of_set(sc, n, sb, c, logs, r):
    """(V, counts) of the one bucket set of a window-table MSM: every non-zero signed digit (window w, magnitude m, sign) of scalar i adds
    +-2^(c w) logs[i] to bucket m - 1. Vectorised: the logarithms travel as 16-bit limbs through np.add.at."""
    import msm_sort_ref as R
    nb = 1 << (c - 1)
    keys, ents = R.digit_lists(sc, n, sb, c, precomp=True, stride=n)
    idx, sign = (ents & 0x7FFFFFFF).astype(np.int64), np.where(ents >> 31, -1, 1).astype(np.int64)
    assert r < 1 << 256
    tab = b"".join(((v << (c * w)) % r).to_bytes(32, "little") for w in range(P.digits_of(sb, c)) for v in logs[:n])      # table row w of base i at w * n + i
    limbs = np.frombuffer(tab, "<u2").reshape(-1, 16).astype(np.int64)
    acc = np.zeros((nb, 16), np.int64)
    np.add.at(acc, keys, limbs[idx] * sign[:, None])                                # a base at infinity (logarithm 0) adds nothing, and still counts as an entry
    counts = np.bincount(keys, minlength=nb)
    V = [0] * nb
    for b in np.nonzero(counts)[0].tolist():
        V[b] = sum(x << (16 * k) for k, x in enumerate(acc[b].tolist())) % r
    return V, counts.tolist()
