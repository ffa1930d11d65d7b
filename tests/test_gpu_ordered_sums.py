"""The ordered float32 sums where their one bit of state is busy, and nucleotides on every path -- by value, against the CPU oracle.

DESIGN.md 5.1: the device evaluates the similarity statistic's sequential sums out of order and stays bit-exact through the parity
it carries for exact ties.  On `synth_msa` data a column of 240 000 terms holds a handful of ties; on the alignments of
tests/ordered_cases.py (gap-free body of a power-of-two width, a distance table of multiples of 1/4) a quarter of a column's
denominator terms are ties -- several per 64-row round, in the first and the last lane, on the rows that cross a binade, in
consecutive segments of a split column -- and every identity is dyadic, so the identity sums leave their fast path on every block.
tests/test_ordered_sum_inputs.py holds the conditions on the inputs (no GPU).

  a. tie-dense, every statistic (the default context)
  b. tie-dense, every similarity path (`KERNELS` of tests/test_gpu_parity.py), per-lane start offsets
  c. tie-dense, whole trims: `msa_trim` under every switch setting of tests/fuzz/fuzz_trim.py, the batch engine's three group kinds
  d. nucleotides, every statistic, one step past each dispatch line
  e. nucleotides, every similarity path
  f. nucleotides, whole trims through the public API (the type detection picks the matrix and 'N'), alone and in one batch call
  g. a letter outside the nucleotide table: the failure's row and column

Every comparison is exact (integers equal, floats equal as uint32 bits).
"""
import ast
import functools
import os

import numpy as np
import pytest

import oracle
from ordered_cases import N, TIE_SHAPES, TIE_TALL, X, count_ties, dyadic_table, nt_alignment, shares, tie_case, tie_dense
from pytrimal_amd import Alignment, _lib
from pytrimal_amd.batch import trim_batch
from pytrimal_amd.synth import synth_msa
from test_gpu_batch_engine import LANE, LISTS, MULTI, P, expect, rig  # noqa: F401  (rig: a fixture)
from test_gpu_parity import KERNEL_IDS, KERNELS, all_stats, bits, ctx, ctx_with  # noqa: F401  (ctx, ctx_with: fixtures)
from test_gpu_trimmers import _SWEEP

pytestmark = pytest.mark.gpu

DYADIC = tuple(np.ascontiguousarray(x) for x in dyadic_table())
NT_MATRICES = {False: oracle.nt_matrix(False), True: oracle.nt_matrix(True)}


@functools.lru_cache(maxsize=None)
def tie_ref(m, n):
    """the oracle's (MDK, Q) of a tie-dense shape under the dyadic table, once per process"""
    a = tie_case(m, n)
    hit, dst = oracle.pair_counts(a, X)
    return oracle.similarity(a, oracle.weights(hit, dst), oracle.gaps(a)[0], *DYADIC, X)


@functools.lru_cache(maxsize=None)
def nt_ref(kind, m, n):
    a = nt_alignment(kind, m, n)
    hit, dst = oracle.pair_counts(a, N)
    return oracle.similarity(a, oracle.weights(hit, dst), oracle.gaps(a)[0], *NT_MATRICES[kind == "deg"], N)


def sim_equal(c, a, indet, matrix, want):
    c.upload(a, indet)
    mdk, q = c.similarity(*matrix)
    omdk, oq = want
    wrong = np.flatnonzero(bits(q) != bits(oq))
    assert wrong.size == 0, f"Q differs from the oracle in {wrong.size} of {len(q)} columns, the first {int(wrong[0])}: " \
                            f"{q[wrong[0]]!r} for {oq[wrong[0]]!r} ({int((a[:, wrong[0]] != ord('-')).sum())} valid rows)"
    assert np.array_equal(bits(mdk), bits(omdk)), "MDK differs from the oracle"


# ---- a. tie-dense, every statistic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", TIE_SHAPES, ids=[f"{m}x{n}" for m, n in TIE_SHAPES])
def test_tie_dense_every_statistic(ctx, m, n):
    """gap and pair counts, identities and W, the identity means (dyadic identities: ties in `identity_stats`' sums), Q, MDK, overlap"""
    assert all_stats(ctx, tie_case(m, n), indet=X, matrix=DYADIC) is None


# ---- b. tie-dense, every similarity path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("m,n", [(70, 32768), (200, 4096), (513, 512)], ids=["70x32768", "200x4096", "513x512"])
def test_tie_dense_similarity_paths(ctx_with, kernel, m, n):
    sim_equal(ctx_with(**kernel), tie_case(m, n), X, DYADIC, tie_ref(m, n))


def test_tall_shape_is_tie_dense():
    """4100 x 32 (nb = 16): column 0's share of ties, by the plain counter (measured: 0.162 of the denominator's terms, 0.099 of the
    numerator's; the gapped column 31: 0.250 / 0.091)"""
    den, num = shares(count_ties(tie_case(*TIE_TALL), X, *DYADIC, 0))
    print(f"{TIE_TALL}: ties {den:.4f} / {num:.4f}")
    assert TIE_TALL[0] >= 4040 and den >= 0.10 and num >= 0.03


@pytest.mark.parametrize("kernel", KERNELS[:-1], ids=KERNEL_IDS[:-1])
@pytest.mark.parametrize("m,n", [(2100, 64), TIE_TALL], ids=["2100x64", "%dx%d" % TIE_TALL])
def test_tie_dense_similarity_paths_many_rows(ctx_with, kernel, m, n):
    sim_equal(ctx_with(**kernel), tie_case(m, n), X, DYADIC, tie_ref(m, n))


@pytest.mark.parametrize("big", ["", "1"])
@pytest.mark.parametrize("r0", ["0", "1", "63", "64", "70"])
def test_tie_dense_ordered_prefix(ctx_with, big, r0):
    """the rows evaluated in order before the first round: a round then starts on and off a 64-row boundary, and the tie rows fall
    into other lanes and other rounds"""
    sim_equal(ctx_with(MSA_LG_BIG=big, MSA_LG_R0=r0), tie_case(700, 256), X, DYADIC, tie_ref(700, 256))


# ---- c. tie-dense, whole trims -------------------------------------------------------------------------------------------------
def fuzz_contexts():
    """`CONTEXTS` of tests/fuzz/fuzz_trim.py (a script: it is read, not imported)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz", "fuzz_trim.py")) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "CONTEXTS":
            return [{kw.arg: kw.value.value for kw in call.keywords} for call in node.value.elts]
    raise AssertionError("tests/fuzz/fuzz_trim.py has no CONTEXTS")


CONTEXTS = fuzz_contexts()
TRIMS = (dict(method="strict"), dict(method="automated1"), dict(similarity_threshold=0.58, conservation_percentage=40.0))


def dyadic_params(**kw):
    p = P("aa", **kw)
    p.vhash, p.dist, p.npos = DYADIC[0].ctypes.data, DYADIC[1].ctypes.data, DYADIC[1].shape[0]
    return p


@functools.lru_cache(maxsize=None)
def tie_trim_ref(m, n, k):
    return oracle.trim(tie_case(m, n), matrix=DYADIC, indet=X, **TRIMS[k])


def test_fuzz_contexts_are_read():
    assert len(CONTEXTS) >= 7 and CONTEXTS[0] == {} and all(k.startswith("MSA_") and isinstance(v, str) for env in CONTEXTS for k, v in env.items())


@pytest.mark.parametrize("env", CONTEXTS, ids=["-".join(f"{k[4:]}={v}" for k, v in env.items()) or "default" for env in CONTEXTS])
@pytest.mark.parametrize("m,n", [(130, 8192), (700, 256)], ids=["130x8192", "700x256"])
def test_tie_dense_trims(ctx_with, env, m, n):
    """`msa_trim`: masks, the method automated1 selects and the identity means (sums of dyadic identities) against the oracle's trim"""
    a = tie_case(m, n)
    c = ctx_with(**env)
    c.upload(a, X)
    for k, kw in enumerate(TRIMS):
        ores, oseq, oinfo = tie_trim_ref(m, n, k)
        res, seq, info = c.trim(dyadic_params(**kw))
        wrong = np.flatnonzero(res != ores)
        assert wrong.size == 0, f"{kw}: kept columns differ from the oracle's at {wrong[:8].tolist()}"
        assert np.array_equal(seq, oseq), kw
        # (the identity means: `msa_trim` and the oracle fill them under automated1 alone, the one method that computes them -- zero
        # on both sides for the other trims, the manual one included)
        assert info.selected_method == oinfo.selected, kw
        assert bits(info.avg_seq) == bits(oinfo.avg_seq) and bits(info.max_seq) == bits(oinfo.max_seq), kw
        if "method" in kw:
            assert info.gap_cut == oinfo.gap_cut and bits(info.sim_cut) == bits(oinfo.sim_cut), kw
    assert 0 < tie_trim_ref(m, n, 0)[0].sum() < n and 0 < tie_trim_ref(m, n, 2)[0].sum() < n  # (the masks depend on the values)


# (m, nb, route, values): the engine takes m^2 n up to 3e8, a lane per column up to 128 rows, several launches from 1800 rows; the ties
# of a column lie where its sum passes the binade of ulp = 1 / nb, so the widths cannot be smaller.  Measured shares of ties in column
# 0 (denominator / numerator): 128 x 8192: 0.234 / 0.099, 260 x 2048: 0.233 / 0.087, 1800 x 64: 0.248 / 0.079.
# values None: every distinct value of the oracle's MDK vector is pinned, so every column is fixed to the bit -- the group of several
# launches, which carries the columns' tie state through memory between them.  A number: that many distinct values, spread over the
# sorted ones with both ends among them.  Pinning all 8181 values of 128 x 8192 would send the megabyte of its rows 16 362 times
# (2045 values and 2 GB at 260 x 2048); 256 values are 512 alignments per shape, fix at least 256 columns to the bit, and hold
# every other column between two pinned values 1 / 256 of the sorted columns apart.
ENGINE = [(128, 4096, LANE, 256), (260, 1024, LISTS, 256), (1800, 32, MULTI, None)]
ENGINE_CALL = 64  # alignments per `msa_trim_batch` call


@pytest.mark.parametrize("m,nb,route,values", ENGINE, ids=["lane", "lists", "multi"])
def test_tie_dense_through_the_batch_engine(rig, m, nb, route, values):
    """One tie-dense alignment per group kind, its route asserted.  The engine returns no MDK vector, but a manual similarity trim
    keeps a column exactly when its value lies above the cut: the alignment at a threshold pair -- a value, and the float32 just
    below -- fixes that value's columns to the bit (tests/test_gpu_batch_engine.py).  The expected masks come from one similarity
    pass of the oracle and its own selection functions (cleanConservation: `sim_cutpoint`, `clean_fallbehind`, then the sequences
    left with gaps only go), checked against the oracle's whole trim at both ends and in the middle.  A strict and an automated1 trim
    ride along, by masks, cut points and identity means."""
    n = 2 * nb
    a = tie_dense(m, nb, 500 + m)
    den, num = shares(count_ties(a, X, *DYADIC, 0))
    print(f"{m} x {n}: ties {den:.4f} / {num:.4f}")
    assert den >= 0.10 and num >= 0.03
    hit, dst = oracle.pair_counts(a, X)
    mdk, _ = oracle.similarity(a, oracle.weights(hit, dst), oracle.gaps(a)[0], *DYADIC, X)
    distinct = np.unique(mdk)
    if values is not None:
        distinct = distinct[np.unique(np.linspace(0, len(distinct) - 1, values).round().astype(int))]
        assert len(distinct) == values
    assert distinct[0] == mdk.min() and distinct[-1] == mdk.max()
    thresholds = []
    for v in distinct:
        thresholds += [np.nextafter(v, np.float32(-np.inf), dtype=np.float32), v]

    def want(t):
        res = oracle.clean_fallbehind(mdk, np.float32(oracle.sim_cutpoint(mdk, -1.0, float(t))), -1.0)
        return res, (a[:, res] != ord("-")).any(axis=1)

    wants = [want(t) for t in thresholds]
    last = len(thresholds) - 1
    for i in (0, 1, last // 2, last // 2 + 1, last - 1, last):  # (a condition on the reference: the oracle's whole trim gives these masks)
        ores, oseq, _ = oracle.trim(a, matrix=DYADIC, indet=X, similarity_threshold=float(thresholds[i]))
        assert np.array_equal(ores, wants[i][0]) and np.array_equal(oseq, wants[i][1])
    pinned = np.zeros(n, dtype=bool)
    for i, v in enumerate(distinct):  # (... and they flip at the value)
        cols = mdk == v
        assert wants[2 * i][0][cols].all() and not wants[2 * i + 1][0][cols].any(), f"the oracle's masks do not flip at {v!r}"
        pinned |= cols
    print(f"{m} x {n}: {int(pinned.sum())} of {n} columns fixed to the bit by {len(distinct)} values")
    assert pinned.sum() == n if values is None else pinned.sum() >= values
    autos = [dict(method="strict"), dict(method="automated1")]
    batch = rig.batch()
    for first in range(0, len(thresholds), ENGINE_CALL):
        part = thresholds[first:first + ENGINE_CALL]
        riders = autos if first == 0 else []
        out = batch.trim([(a, X, dyadic_params(similarity_threshold=float(t))) for t in part] + [(a, X, dyadic_params(**kw)) for kw in riders])
        routes = batch.last_routes()
        assert len(routes) == len(part) + len(riders)
        for r in routes:
            expect(r, route, f"{m} x {n}")
        for i, (t, got, (wres, wseq)) in enumerate(zip(part, out, wants[first:])):
            res, seq, info, rc, rows = got
            assert rc == _lib.OK
            wrong = np.flatnonzero(res != wres)
            assert wrong.size == 0, f"{m} x {n}, threshold {t!r} ({'at' if i % 2 else 'below'} the value): columns {wrong[:8].tolist()} " \
                                    f"with the oracle's values {mdk[wrong[:8]].tolist()}"
            assert np.array_equal(seq, wseq) and info.kept_residues == int(res.sum()) and info.kept_sequences == int(seq.sum())
        for kw, got in zip(riders, out[len(part):]):
            res, seq, info, rc, rows = got
            ores, oseq, oinfo = oracle.trim(a, matrix=DYADIC, indet=X, **kw)
            assert rc == _lib.OK and np.array_equal(res, ores) and np.array_equal(seq, oseq), kw
            assert info.gap_cut == oinfo.gap_cut and bits(info.sim_cut) == bits(oinfo.sim_cut) and info.selected_method == oinfo.selected, kw
            assert bits(info.avg_seq) == bits(oinfo.avg_seq) and bits(info.max_seq) == bits(oinfo.max_seq), kw


# ---- d. nucleotides, every statistic -------------------------------------------------------------------------------------------
KINDS = ("dna", "rna", "deg", "soft")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", [(129, 70), (513, 97), (1030, 70), (2100, 40)], ids=["129x70", "513x97", "1030x70", "2100x40"])
def test_nucleotides_every_statistic(ctx, kind, m, n):
    """one step past each dispatch line: the wave-per-column kernel, the 16-row front and pair tiles, the ordinary pipeline, six
    rounds per launch"""
    assert all_stats(ctx, nt_alignment(kind, m, n), indet=N, matrix=NT_MATRICES[kind == "deg"]) is None


# ---- e. nucleotides, every similarity path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("kind", ["dna", "deg"])
@pytest.mark.parametrize("m,n", [(190, 150), (640, 257)], ids=["190x150", "640x257"])
def test_nucleotides_similarity_paths(ctx_with, kernel, kind, m, n):
    """three distinct distances (19 in the degenerate table), conserved columns, many zero terms: the predictor's precise regime"""
    sim_equal(ctx_with(**kernel), nt_alignment(kind, m, n), N, NT_MATRICES[kind == "deg"], nt_ref(kind, m, n))


@pytest.mark.parametrize("kernel", KERNELS[:-1], ids=KERNEL_IDS[:-1])
@pytest.mark.parametrize("kind", ["dna", "deg"])
def test_nucleotides_similarity_paths_many_rows(ctx_with, kernel, kind):
    sim_equal(ctx_with(**kernel), nt_alignment(kind, 2017, 33), N, NT_MATRICES[kind == "deg"], nt_ref(kind, 2017, 33))


# ---- f. nucleotides, whole trims through the public API ------------------------------------------------------------------------
API_SHAPES = [(300, 200), (1100, 120)]


def as_alignment(a):
    return Alignment([b"s%d" % i for i in range(a.shape[0])], [bytes(r) for r in a])


@functools.lru_cache(maxsize=None)
def api_ref(kind, m, n, k):
    """the oracle's trim with nothing passed for the matrix or the indetermination symbol: its type detection chooses"""
    a = synth_msa(m, n, 61) if kind == "aa" else nt_alignment(kind, m, n)
    res, seq, _ = oracle.trim(a, **_SWEEP[k][1])
    return [bool(x) for x in res], [bool(x) for x in seq]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", API_SHAPES, ids=["300x200", "1100x120"])
def test_nucleotide_trims_through_the_api(kind, m, n):
    ali = as_alignment(nt_alignment(kind, m, n))
    for k, (make, kw) in enumerate(_SWEEP):
        res, seq = api_ref(kind, m, n, k)
        trimmed = make().trim(ali)
        assert trimmed.residues_mask == res, (kind, kw)
        assert trimmed.sequences_mask == seq, (kind, kw)


def test_nucleotide_trims_in_one_batch_call():
    """the same alignments, every type and both shapes, and a protein alignment among them in one `trim_batch` call per trimmer"""
    cases = [(kind, m, n) for m, n in API_SHAPES for kind in KINDS]
    cases.insert(3, ("aa", 200, 150))
    alis = [as_alignment(synth_msa(m, n, 61) if kind == "aa" else nt_alignment(kind, m, n)) for kind, m, n in cases]
    for k, (make, kw) in enumerate(_SWEEP):
        out = trim_batch(make(), alis, shard=False)
        assert len(out) == len(cases)
        for (kind, m, n), t in zip(cases, out):
            res, seq = api_ref(kind, m, n, k)
            assert t.residues_mask == res and t.sequences_mask == seq, (kind, m, n, kw)


# ---- g. a letter outside the nucleotide table ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,row", [(190, 150, 140), (640, 97, 140), (1100, 70, 1040)], ids=["190x150", "640x97", "1100x70"])
def test_a_letter_outside_the_nucleotide_table(ctx, m, n, row):
    """an 'E' in an alignment the type detection still calls DNA: strict fails as the oracle does, at the oracle's row and column,
    on the 129-, 513- and 1030-row paths; gappyout on the same upload looks at no residue and does not fail"""
    a = nt_alignment("dna", m, n).copy()
    col = n // 3
    a[:, col] = np.frombuffer(b"ACGT", dtype=np.uint8)[np.arange(m) % 4]  # (a column without gaps: never cut by the gaps rule)
    a[row, col] = ord("E")
    assert oracle.alignment_type(a) == 1 and oracle.indet_for(a) == N
    with pytest.raises(oracle.OracleError) as o:
        oracle.trim(a, method="strict")
    assert o.value.code == oracle.E_UNDEFINED_SYMBOL and tuple(o.value.detail) == (row, col, ord("E"))
    ctx.upload(a, N)
    p = P("nt", method="strict")
    res, seq, info, rc = ctx.trim_rc(p)
    assert rc == _lib.E_UNDEFINED_SYMBOL and (info.err.row, info.err.col, info.err.byte) == (row, col, ord("E"))
    with pytest.raises(ValueError, match="'E'"):
        ctx.trim(p)
    p.method = _lib.METHOD_CODES["gappyout"]
    res, seq, info = ctx.trim(p)
    ores, oseq, oinfo = oracle.trim(a, method="gappyout")
    assert np.array_equal(res, ores) and np.array_equal(seq, oseq) and info.gap_cut == oinfo.gap_cut
    with pytest.raises(ValueError, match="'E'"):  # (... and through the public API)
        _SWEEP[0][0]().trim(as_alignment(a))
    trimmed = _SWEEP[2][0]().trim(as_alignment(a))
    assert trimmed.residues_mask == [bool(x) for x in ores]
