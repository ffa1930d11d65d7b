"""Conditions on the inputs of tests/test_gpu_ordered_sums.py, and the counter that states them, against the oracle (no GPU).

The tie shares are properties of the alignments alone, counted by `ordered_cases.count_ties` in numpy: an edit of the generator
that loses the ties fails here, before any kernel runs.  Column 0, shares of all terms of the column that are ties, as measured:

    m x n          denominator   numerator
    70 x 32768        0.237        0.058
    130 x 8192        0.222        0.103
    200 x 4096        0.246        0.081
    513 x 512         0.233        0.061
    700 x 256         0.228        0.066
    2100 x 64         0.228        0.105     (its last, gapped column of 1485 rows: 0.250 / 0.070)
    4100 x 32         0.162        0.099
    synth_msa(700, 64, 5): 0.00001 / 0.00003
"""
import numpy as np
import pytest

import oracle
from ordered_cases import (N, TIE_SHAPES, TIE_TALL, X, count_ties, dyadic_table, nt_alignment, pair_counts, q_and_mdk, shares, tie_case,
                           weights)
from pytrimal_amd.synth import synth_msa


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_dyadic_table():
    vhash, dist = dyadic_table(b"ACGT")
    assert sorted(np.flatnonzero(vhash >= 0) + 65) == sorted(b"ACGT") and dist.shape == (4, 4) and dist.dtype == np.float32
    off = dist[~np.eye(4, dtype=bool)]
    assert np.array_equal(dist, dist.T) and not dist.diagonal().any()
    assert np.array_equal(off * 4, np.round(off * 4)) and off.min() >= 0.25 and off.max() <= 2 and len(np.unique(off)) >= 4


@pytest.mark.parametrize("m,n", TIE_SHAPES + [TIE_TALL], ids=lambda v: str(v))
def test_tie_shares(m, n):
    a = tie_case(m, n)
    nb = n // 2
    assert a.shape == (m, n) and not np.isin(a, np.frombuffer(b"ACGT", dtype=np.uint8), invert=True)[:, :nb].any()
    vhash, dist = dyadic_table()
    t = count_ties(a, X, vhash, dist, 0)
    den_share, num_share = shares(t)
    print(f"{m} x {n}: column 0, {t.terms} terms, ties {den_share:.4f} of the denominator's, {num_share:.4f} of the numerator's; "
          f"binade crossings {t.den_crossings} / {t.num_crossings}")
    assert t.terms == m * (m - 1) // 2
    assert den_share >= 0.10 and num_share >= 0.03
    assert t.den_crossings >= 8 and t.num_crossings >= 8
    _, dst = pair_counts(a, X)
    off = dst[~np.eye(m, dtype=bool)]
    assert np.isin(off, (nb, 2 * nb)).all() and (off == nb).any() and (off == 2 * nb).any()
    nvalid = int((a[:, n - 1] != ord("-")).sum())
    assert 2 <= nvalid < m and (a[:, 0] != ord("-")).all()


def test_what_the_old_data_lacked():
    a = synth_msa(700, 64, 5)
    t = count_ties(a, X, *oracle.aa_matrix(), 0)
    assert t.terms > 200000 and max(shares(t)) < 0.001


@pytest.mark.parametrize("m,n", TIE_SHAPES, ids=lambda v: str(v))
def test_counter_against_the_oracle(m, n):
    """the plain walk of `count_ties` gives the oracle's Q and MDK of the column, bit for bit -- the counter looks at the sums the
    statistic is made of"""
    a = tie_case(m, n)
    vhash, dist = dyadic_table()
    hit, dst = oracle.pair_counts(a, X)
    mine = pair_counts(a, X)
    assert np.array_equal(hit, mine[0]) and np.array_equal(dst, mine[1])
    w = weights(a, X)
    ow = oracle.weights(hit, dst)
    assert np.array_equal(bits(w), bits(ow))
    g = oracle.gaps(a)[0]
    mdk, q = oracle.similarity(a, ow, g, vhash, dist, X)
    for col in (0, n // 2 - 1, n - 1):
        want_q, want_mdk = q_and_mdk(count_ties(a, X, vhash, dist, col, w=w))
        assert bits(q[col]) == bits(want_q) and bits(mdk[col]) == bits(want_mdk), f"column {col}"


@pytest.mark.skipif(oracle.lib_avx2() is None, reason="host CPU without AVX2")
@pytest.mark.parametrize("m,n", TIE_SHAPES, ids=lambda v: str(v))
def test_oracle_flavours_agree(m, n):
    """the oracle's scalar and AVX2 passes on the tie-dense inputs, bit for bit"""
    a = tie_case(m, n)
    vhash, dist = dyadic_table()
    hit, dst = oracle.pair_counts(a, X)
    ahit, adst = oracle.pair_counts(a, X, avx2=True)
    assert np.array_equal(hit, ahit) and np.array_equal(dst, adst)
    w, g = oracle.weights(hit, dst), oracle.gaps(a)[0]
    mdk, q = oracle.similarity(a, w, g, vhash, dist, X)
    mdk2, q2 = oracle.similarity(a, w, g, vhash, dist, X, avx2=True)
    assert np.array_equal(bits(q), bits(q2)) and np.array_equal(bits(mdk), bits(mdk2))


KINDS = {"dna": 1, "rna": 2, "deg": 8, "soft": 1}
NT_SHAPES = [(129, 70), (513, 97), (1030, 70), (2100, 40), (190, 150), (640, 257), (2017, 33), (300, 200), (1100, 120)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_nucleotide_cases(kind):
    for m, n in NT_SHAPES:
        a = nt_alignment(kind, m, n)
        t = oracle.alignment_type(a)
        assert not t & 4 and t & KINDS[kind] and bool(t & 8) == (kind == "deg"), (m, n, t)
        assert oracle.indet_for(a) == N
        assert np.array_equal(a[2], a[0]) and (a[1] == ord("-")).all() and (a[:, n // 2] == ord("-")).all()
        assert 0.2 <= (a == ord("-")).mean() <= 0.3 and 0.015 <= (a == N).mean() <= 0.035
        ends = ((a[:, 0] == ord("-")) & (a[:, 1] == ord("-")) & (a[:, 2] == ord("-"))).sum()
        assert ends >= m // 30  # (runs of gaps at the ends of some rows)
        letters = set(np.unique(a).tolist()) - {ord("-"), N}
        if kind == "soft":
            lower = ((a >= 97) & (a <= 122)).sum() / max(((a != ord("-")) & (a != N)).sum(), 1)
            assert 0.15 <= lower <= 0.25 and {chr(x).upper() for x in letters} == set("ACGT")
        else:
            assert letters == set(oracle.NT_DEG_ALPHABET.encode() if kind == "deg" else {"dna": b"ACGT", "rna": b"ACGU"}[kind])
        # conserved columns: the commonest residue holds most of a column's valid rows
        col = a[:, 0][(a[:, 0] != ord("-")) & (a[:, 0] != N)]
        assert np.bincount(col & 0xDF).max() >= 0.7 * len(col)
