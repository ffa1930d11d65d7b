"""Inputs for the ordered float32 sums, and a plain counter of what they hold.

The similarity statistic is a sequential float32 sum; the device evaluates it out of order and is bit-exact only because
it carries one bit of state for the terms that are exact ties, (k + 1/2) ulp of the running sum.  `synth_msa` data meets a
handful of such terms per column.  `tie_dense` makes them the common case: a gap-free body of a power-of-two width (so every
weight W = 1 - hit/dst is k / 2^p exactly) under a distance table of multiples of 1/4 (`dyadic_table`).  `count_ties` walks
one column the way the reference does, one float32 add at a time, and counts them: the conditions the tests put on these inputs
are checked by it alone.

`nt_case` draws nucleotide alignments as they come in practice: conserved columns, terminal gap runs, N, lower case.

A plain module (imported by tests/test_ordered_sum_inputs.py and tests/test_gpu_ordered_sums.py): no fixture, no pytest setting.
"""
import collections
import functools

import numpy as np

import oracle

GAP = ord("-")


def tie_dense(m, nb, seed, letters=b"ACGT", gapped=True):
    """uint8 [m, 2 nb]: every residue a copy of the root's with probability 0.6, else redrawn from `letters`; a fixed set G of
    about 0.3 of the rows is '-' in the columns nb ... 2 nb - 1 (`gapped`), and nothing else is a gap or an indetermination.
    So dst is nb (both rows in G) or 2 nb for every pair, and the columns of the second half have fewer valid rows than m."""
    r = np.random.default_rng(seed)
    alpha = np.frombuffer(bytes(letters), dtype=np.uint8)
    n = 2 * nb
    root = alpha[r.integers(0, len(alpha), n)]
    a = np.where(r.random((m, n)) < 0.6, root[None, :], alpha[r.integers(0, len(alpha), (m, n))])
    in_g = r.random(m) < 0.3
    if gapped:
        if not in_g.any():
            in_g[m // 2] = True
        a[in_g, nb:] = GAP
    return np.ascontiguousarray(a, dtype=np.uint8)


def dyadic_table(letters=b"ACGT"):
    """(vhash int32[26], dist float32[k, k]) over `letters`: symmetric, zero diagonal, every other entry a multiple of 0.25 in
    [0.25, 2] -- a legal input of the C ABI, which takes `dist` raw."""
    letters = bytes(letters).upper()
    k = len(letters)
    assert len(set(letters)) == k and all(65 <= x <= 90 for x in letters)
    vhash = np.full(26, -1, dtype=np.int32)
    for i, ch in enumerate(letters):
        vhash[ch - 65] = i
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    dist = (np.float32(0.25) * (1 + (i + j + i * j) % 8)).astype(np.float32)
    np.fill_diagonal(dist, 0)
    off = dist[~np.eye(k, dtype=bool)]
    assert np.array_equal(dist, dist.T) and off.min() >= 0.25 and off.max() <= 2 and len(np.unique(off)) >= 4
    assert np.array_equal(off * 4, np.round(off * 4))
    return vhash, dist


def pair_counts(a, indet):
    """(hit, dst) uint32 [m, m] as the reference counts them on raw bytes, by matrix products of 0 / 1 matrices (exact: every
    count is below 2^24); diagonal 0."""
    a = np.asarray(a, dtype=np.uint8)
    valid = (a != GAP) & (a != indet)
    v = valid.astype(np.float32)
    nv = valid.sum(axis=1).astype(np.int64)
    both = (v @ v.T).astype(np.int64)
    dst = nv[:, None] + nv[None, :] - both
    hit = np.zeros_like(dst)
    for b in np.unique(a[valid]):
        one = (valid & (a == b)).astype(np.float32)
        hit += (one @ one.T).astype(np.int64)
    np.fill_diagonal(dst, 0)
    np.fill_diagonal(hit, 0)
    return hit.astype(np.uint32), dst.astype(np.uint32)


def weights(a, indet):
    """W = 1 - (float)hit / dst in float32 (dst == 0: 1), diagonal 0: oracle/msa_oracle.c orc_weights, in numpy."""
    hit, dst = pair_counts(a, indet)
    with np.errstate(invalid="ignore", divide="ignore"):
        ident = np.where(dst > 0, hit.astype(np.float32) / dst.astype(np.float32), np.float32(0)).astype(np.float32)
    w = (np.float32(1) - ident).astype(np.float32)
    np.fill_diagonal(w, 0)
    return w


Ties = collections.namedtuple("Ties", "den num terms den_ties num_ties den_crossings num_crossings")


def _walk(x):
    """One sequential float32 sum of the terms `x`: (the final sum, ties, binade crossings)."""
    if x.size == 0:
        return np.float32(0), 0, 0
    run = np.add.accumulate(np.concatenate([np.zeros(1, dtype=np.float32), x]), dtype=np.float32)  # one float32 add at a time
    before, after = run[:-1], run[1:]
    ulp = np.spacing(before).astype(np.float64)
    frac = np.modf(x.astype(np.float64) / ulp)[0]  # (a division by a power of two: exact)
    ties = int(((x > 0) & (frac == 0.5)).sum())
    crossings = int(((before > 0) & (np.frexp(after)[1] > np.frexp(before)[1])).sum())
    return run[-1], ties, crossings


def count_ties(a, indet, vhash, dist, col, w=None):
    """The two sums of column `col` in the reference's order -- the valid pairs j < k in lexicographic order, den += W[j][k],
    num += W[j][k] * dist[j][k], float32, one add at a time -- with, for each sum, the number of terms x > 0 that are ties,
    frac(x / ulp(running sum)) == 1/2, and the number of adds after which the sum is in a higher binade.
    Numpy only; the oracle's similarity is not called.  `w`: `weights(a, indet)` when the caller has it already."""
    a = np.asarray(a, dtype=np.uint8)
    w = weights(a, indet) if w is None else w
    dist = np.asarray(dist, dtype=np.float32)
    x = a[:, col]
    rows = np.flatnonzero((x != GAP) & (x != indet))
    up = np.where((x[rows] >= 97) & (x[rows] <= 122), x[rows] - 32, x[rows]).astype(np.int64)
    code = np.asarray(vhash)[up - 65]
    assert (up >= 65).all() and (up <= 90).all() and (code >= 0).all(), "a residue outside the table"
    den_terms, num_terms = [], []
    for i, j in enumerate(rows[:-1]):
        wj = w[j, rows[i + 1:]]
        den_terms.append(wj)
        num_terms.append(wj * dist[code[i], code[i + 1:]])  # (a float32 product, rounded before the add: never fused)
    den_terms = np.concatenate(den_terms).astype(np.float32) if den_terms else np.zeros(0, dtype=np.float32)
    num_terms = np.concatenate(num_terms).astype(np.float32) if num_terms else np.zeros(0, dtype=np.float32)
    den, den_ties, den_x = _walk(den_terms)
    num, num_ties, num_x = _walk(num_terms)
    return Ties(np.float32(den), np.float32(num), int(den_terms.size), den_ties, num_ties, den_x, num_x)


def q_and_mdk(t):
    """What orc_similarity makes of the two sums: (q, mdk) in float32."""
    if t.den == 0:
        return np.float32(0), np.float32(0)
    q = np.float32(t.num / t.den)
    v = np.float32(np.exp(-np.float64(q)))
    return q, min(v, np.float32(1))


NT_LETTERS = {"dna": b"ACGT", "rna": b"ACGU", "deg": oracle.NT_DEG_ALPHABET.encode(), "soft": b"ACGT"}


def nt_case(kind, m, n, seed):
    """uint8 [m, n] nucleotides, `kind` in dna / rna / deg (all fifteen letters of the degenerate table) / soft (DNA with a fifth
    of the residues in lower case): conserved columns (a residue is the root's with probability 0.85), 20 % gaps -- on a tenth of
    the rows as runs at both ends --, 3 % N, row 2 a copy of row 0, row 1 of gaps only, column n // 2 of gaps only."""
    r = np.random.default_rng(seed)
    alpha = np.frombuffer(NT_LETTERS[kind], dtype=np.uint8)
    root = alpha[r.integers(0, len(alpha), n)]
    a = np.where(r.random((m, n)) < 0.85, root[None, :], alpha[r.integers(0, len(alpha), (m, n))]).astype(np.uint8)
    if kind == "soft":
        a[r.random((m, n)) < 0.2] += 32
    a[r.random((m, n)) < 0.2] = GAP
    for row in r.choice(m, size=max(1, m // 10), replace=False):
        head, tail = r.integers(0, n // 3 + 1, 2)
        a[row, :head] = GAP
        a[row, n - tail:] = GAP
    a[(r.random((m, n)) < 0.03) & (a != GAP)] = ord("N")
    if m > 2:
        a[2] = a[0]
        a[1] = GAP
    a[:, n // 2] = GAP
    return np.ascontiguousarray(a, dtype=np.uint8)


# ---- the shapes the tests share (made once per process, read-only) -------------------------------------------------------------
X, N = ord("X"), ord("N")
# m x n with nb = n / 2: the flat kernel, the wave-per-column kernel (129 ... 512 rows), the 16-row front and pair tiles
# (513 ... 1024), the ordinary pipeline, and six rounds per launch
TIE_SHAPES = [(70, 32768), (130, 8192), (200, 4096), (513, 512), (700, 256), (2100, 64)]
TIE_TALL = (4100, 32)  # nb = 16: two rows j per lane in the pair pass, several launches of the similarity kernel


@functools.lru_cache(maxsize=None)
def tie_case(m, n):
    a = tie_dense(m, n // 2, 100 + m)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def nt_alignment(kind, m, n):
    a = nt_case(kind, m, n, 1000 + m + n)
    a.setflags(write=False)
    return a


def shares(t):
    """(share of the denominator's terms that are ties, share of the numerator's), over all terms of the column"""
    return t.den_ties / max(t.terms, 1), t.num_ties / max(t.terms, 1)
