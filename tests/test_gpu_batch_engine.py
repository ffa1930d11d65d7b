"""`msa_trim_batch`'s engine by value.  The engine (the `Engine` of pytrimal_amd/csrc/msastat_batch.hip and the fifteen
`*_batch_kernel`s: one launch per kernel family over a whole group of alignments, its own lane-per-column similarity kernel, column
sort, identity statistics and row fetch, arenas that are re-zeroed only in part, two lanes in flight) was seen by the suite through
masks alone.  Here, through `_lib.Batch` itself:

  a. a dispatch table in the style of tests/test_gpu_dispatch.py: which alignments the engine takes, in what kind of group
     (`Batch.last_routes()`, i.e. `msa_batch_debug_routes`), on both sides of every line of `engine_takes` and `engine_layout`, with
     the result of that very call by value;
  b. every column's similarity value to the bit, through masks: one alignment many times in a call, each time with a manual
     similarity threshold at a column's value and at the float32 just below it;
  c. `msa_trim_info` by value: cut points, selectMethod's decision and its two means, kept counts, warnings, the failure's detail;
  d. arenas reused with an equal layout signature and other contents;
  e. the four ways rows reach the arena, with residue letters in the slack between the rows;
  f. protein, DNA and degenerate DNA in one call, each with its own matrix.

Every comparison is exact (integers equal, floats equal as uint32 bits).  References: `oracle.trim` with its `Info`, and for what
the oracle does not report (kept counts, warnings, the row a warning names, the rows of gaps only) a `Context.trim` of the same
alignment -- the single-alignment path, itself pinned to the oracle by tests/test_gpu_dispatch.py and tests/test_gpu_pipeline.py."""
import numpy as np
import pytest

import oracle
from pytrimal_amd import _lib
from pytrimal_amd.synth import synth_msa
from test_gpu_dispatch import MSA_SWITCHES
from test_gpu_pipeline import CASES, family

pytestmark = pytest.mark.gpu

X, N = ord("X"), ord("N")
GAP = ord("-")
ALPHA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
BATCH_SWITCHES = ("MSA_BATCH_ENGINE", "MSA_BATCH_ENGINE_MAX", "MSA_BATCH_ENGINE_MIN", "MSA_BATCH_COLS_MAX")


def _matrix(pair):
    vhash, dist = pair
    return np.ascontiguousarray(vhash, dtype=np.int32), np.ascontiguousarray(dist, dtype=np.float32)


MATRICES = {"aa": _matrix(oracle.aa_matrix()), "nt": _matrix(oracle.nt_matrix()), "deg": _matrix(oracle.nt_matrix(True))}
ORACLE_RC = {oracle.E_WINDOW_TOO_BIG: _lib.E_WINDOW_TOO_BIG, oracle.E_INCORRECT_SYMBOL: _lib.E_INCORRECT_SYMBOL,
             oracle.E_UNDEFINED_SYMBOL: _lib.E_UNDEFINED_SYMBOL, oracle.E_NOT_IMPLEMENTED: _lib.E_NOT_IMPLEMENTED}


def bits(x):
    return int(np.float32(x).view(np.uint32))


def P(matrix="aa", method=None, **kw):
    """the parameter block of the oracle's keywords `kw` (MATRICES outlives every block)"""
    vhash, dist = MATRICES[matrix]
    p = _lib.TrimParams(_lib.METHOD_CODES[method], -1.0, -1, -1.0, -1.0, -1, -1, -1, -1.0, -1.0, -1, -1.0, vhash.ctypes.data, dist.ctypes.data,
                        dist.shape[0])
    for k, v in kw.items():
        if k == "gap_threshold":
            p.gap_threshold = float(np.float32(1) - np.float32(v))
        elif k == "identity_threshold":
            p.max_identity = v
        else:
            assert hasattr(p, k), k
            setattr(p, k, v)
    return p


class Rig:
    """a context for the single-alignment reference and the batch objects of a test (the library reads MSA_BATCH_ENGINE_MIN when a
    batch object is created)"""

    def __init__(self, monkeypatch):
        self.monkeypatch = monkeypatch
        self.ctx = _lib.Context(0)
        self.made = []

    def batch(self, engine_min="1", workers=3):
        if engine_min is not None:
            self.monkeypatch.setenv("MSA_BATCH_ENGINE_MIN", engine_min)
        try:
            b = _lib.Batch(0, workers)
        finally:
            self.monkeypatch.delenv("MSA_BATCH_ENGINE_MIN", raising=False)
        self.made.append(b)
        return b

    def single(self, a, indet, p):
        """`msa_trim` of one alignment on the context, nothing raised: (keep_res, keep_seq, info, rc, only-gaps rows)"""
        ctx = self.ctx
        ctx.upload(a, indet)
        res, seq, info, rc = ctx.trim_rc(p)
        return res, seq, info, rc, ctx.only_gaps_rows() if rc == _lib.OK else []

    def close(self):
        for b in self.made:
            b.close()
        self.ctx.close()


@pytest.fixture
def rig(monkeypatch):
    for name in MSA_SWITCHES + BATCH_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    r = Rig(monkeypatch)
    yield r
    r.close()


def want_of(a, kw, matrix="aa", indet=X):
    try:
        return oracle.trim(np.ascontiguousarray(a), matrix=MATRICES[matrix], indet=indet, **kw)
    except oracle.OracleError as e:
        return e


def info_fields(info):
    return dict(selected_method=info.selected_method, avg_seq=bits(info.avg_seq), max_seq=bits(info.max_seq), gap_cut=info.gap_cut,
                sim_cut=bits(info.sim_cut), kept_residues=info.kept_residues, kept_sequences=info.kept_sequences, warnings=info.warnings,
                warn_row=info.warn_row)


def err_of(info):
    return (info.err.row, info.err.col, info.err.byte)


def check(rig, what, a, kw, got, matrix="aa", indet=X, want=None):
    """One alignment of a batch call against both references.  Returns the oracle's result."""
    res, seq, info, rc, rows = got
    want = want_of(a, kw, matrix, indet) if want is None else want
    sres, sseq, sinfo, src, srows = rig.single(a, indet, P(matrix, **kw))
    if isinstance(want, oracle.OracleError):
        assert rc == src == ORACLE_RC[want.code], f"{what}: rc {rc}, the context's {src}, the oracle's {want.code}"
        if want.code in (oracle.E_INCORRECT_SYMBOL, oracle.E_UNDEFINED_SYMBOL):
            assert err_of(info) == tuple(want.detail) and err_of(sinfo) == tuple(want.detail), \
                f"{what}: failure at {err_of(info)}, the context's {err_of(sinfo)}, the oracle's {want.detail}"
        return want
    ores, oseq, oinfo = want
    assert rc == _lib.OK and src == _lib.OK, f"{what}: rc {rc}, the context's {src}"
    assert np.array_equal(res, ores) and np.array_equal(seq, oseq), \
        f"{what}: masks differ from the oracle in columns {np.flatnonzero(res != ores)[:8].tolist()}, rows {np.flatnonzero(seq != oseq)[:8].tolist()}"
    assert np.array_equal(sres, ores) and np.array_equal(sseq, oseq), f"{what}: the context's masks differ from the oracle"
    assert info_fields(info) == info_fields(sinfo), f"{what}: info differs from the context's"
    assert info.kept_residues == int(res.sum()) and info.kept_sequences == int(seq.sum()), f"{what}: kept counts against the masks"
    assert list(rows) == list(srows), f"{what}: rows of gaps only {rows}, the context's {srows}"
    assert bool(info.warnings & _lib.W_ONLY_GAPS_SEQUENCES) == bool(rows)
    if kw.get("method") in ("strict", "strictplus", "automated1", "gappyout"):
        assert info.gap_cut == oinfo.gap_cut, f"{what}: gap_cut {info.gap_cut}, the oracle's {oinfo.gap_cut}"
        assert bits(info.sim_cut) == bits(oinfo.sim_cut), f"{what}: sim_cut {info.sim_cut!r}, the oracle's {oinfo.sim_cut!r}"
        assert info.selected_method == oinfo.selected, f"{what}: selected {info.selected_method}, the oracle's {oinfo.selected}"
        assert bits(info.avg_seq) == bits(oinfo.avg_seq), f"{what}: avg_seq {info.avg_seq!r}, the oracle's {oinfo.avg_seq!r}"
        assert bits(info.max_seq) == bits(oinfo.max_seq), f"{what}: max_seq {info.max_seq!r}, the oracle's {oinfo.max_seq!r}"
    return want


def expect(route, want, what):
    got = {k: route[k] for k in want}
    assert got == want, f"{what}: went {route}"


# ---- a. the dispatch table ------------------------------------------------------------------------------------------------
LANE = dict(engine=True, lane_per_column=True, several_launches=False, redone=False)    # similarity_cols_batch_kernel
LISTS = dict(engine=True, lane_per_column=False, several_launches=False, redone=False)  # codes, lists, the wave-per-column kernel: one launch
MULTI = dict(engine=True, lane_per_column=False, several_launches=True, redone=False)   # ... a launch every six rounds, per-column state
GAPS = dict(engine=True, lane_per_column=False, several_launches=False, redone=False)   # no similarity statistic
WORKER = dict(engine=False)
SIM = (dict(method="strict"), dict(method="automated1"))
TABLE = [
    # --- a lane per column up to 128 rows: its LDS tile is 16 partners wide, a wave is 64 columns, the encode block 256 columns
    (2, 1, SIM, LANE), (2, 64, SIM, LANE), (3, 65, SIM, LANE), (15, 63, SIM, LANE), (16, 64, SIM, LANE), (17, 257, SIM, LANE),
    (127, 130, SIM, LANE), (128, 96, SIM, LANE),
    # --- lists and a wave per column from 129 rows (the column sort's bins, the 512 / 513 and 1024 / 1025 lines of the single path)
    (129, 96, SIM, LISTS), (130, 31, SIM, LISTS), (512, 70, SIM, LISTS), (513, 70, SIM, LISTS), (1024, 64, SIM, LISTS),
    (1025, 64, SIM, LISTS), (1799, 40, SIM, LISTS),
    # --- several launches from 1800 rows
    (1800, 40, SIM, MULTI), (2100, 33, SIM, MULTI), (4088, 16, SIM, MULTI),
    # --- not taken: two rows j per lane in the pair pass (pair_pipe_regime); m^2 n beyond 3e8
    (4096, 16, SIM, WORKER), (1000, 300, SIM, LISTS), (1000, 301, SIM, WORKER),
    # --- a gap-only trim: m n up to 4e6
    (1000, 4000, (dict(method="gappyout"),), GAPS), (1000, 4001, (dict(method="gappyout"),), WORKER),
    # --- RepresentativeTrimmer: up to 1024 rows
    (1024, 200, (dict(identity_threshold=0.5),), GAPS), (1025, 200, (dict(identity_threshold=0.5),), WORKER),
    # --- a gap window: host work on a gap-only trim, in front of the similarity pipeline it is not the engine's
    (100, 96, (dict(gap_threshold=0.8, gap_window=1),), GAPS), (100, 96, (dict(method="strict", window=1),), WORKER),
]


def _table_id(row):
    m, n, kws, _ = row
    kw = kws[0]
    return f"{m}x{n}-" + (kw.get("method") or "-".join(sorted(kw))) + ("-w" if "window" in kw else "")


@pytest.mark.parametrize("m,n,kws,route", TABLE, ids=[_table_id(r) for r in TABLE])
def test_engine_dispatch_and_values(rig, m, n, kws, route):
    """(at most four alignments in a call: every one is a group of its own, so the group's mode is the alignment's)"""
    a = synth_msa(m, n, 7000 + m + n)
    batch = rig.batch()
    out = batch.trim([(a, X, P(**kw)) for kw in kws])
    routes = batch.last_routes()
    assert len(routes) == len(kws)
    for kw, got, r in zip(kws, out, routes):
        expect(r, route, f"{kw} of {m} x {n}")
        check(rig, f"{kw} of {m} x {n}", a, kw, got)
    if route["engine"]:
        assert sorted(r["group"] for r in routes) == list(range(len(kws)))


def test_default_policy_takes_forty_eligible_alignments(rig):
    """no switch set: 39 eligible alignments all go to the workers, 40 go to the engine; alignments the engine never takes
    (a gap window in front of the similarity pipeline) do not count"""
    mats = [synth_msa(20 + k % 7, 30 + k, 7100 + k) for k in range(40)]
    extra = [(synth_msa(30, 50, 7150 + k), X, P(method="strict", window=1)) for k in range(5)]
    batch = rig.batch(engine_min=None)
    wants = [want_of(a, dict(method="strict")) for a in mats]
    for count in (39, 40, 39):
        items = [(a, X, P(method="strict")) for a in mats[:count]]
        out = batch.trim(extra[:2] + items + extra[2:])
        routes = batch.last_routes()
        assert [r["engine"] for r in routes[:2] + routes[2 + count:]] == [False] * 5
        assert [r["engine"] for r in routes[2:2 + count]] == [count >= 40] * count, f"{count} eligible alignments"
        for k in range(count):
            check(rig, f"alignment {k} of {count}", mats[k], dict(method="strict"), out[2 + k], want=wants[k])
        for (a, _, _), got in zip(extra, out[:2] + out[2 + count:]):
            check(rig, "windowed strict", a, dict(method="strict", window=1), got)


def test_groups_alternate_between_kinds(rig):
    """a call is sorted by m^2 n and cut into groups; a group is lane-per-column or not: 128 x 5000, 300 x 100, 100 x 50 are three
    groups of alternating kinds, the first and the third on one lane"""
    shapes = [(100, 50), (128, 5000), (300, 100)]
    mats = [synth_msa(m, n, 7200 + m) for m, n in shapes]
    batch = rig.batch()
    for kw in SIM:
        out = batch.trim([(a, X, P(**kw)) for a in mats])
        routes = batch.last_routes()
        assert [(r["group"], r["lane_per_column"]) for r in routes] == [(2, True), (0, True), (1, False)], routes
        for a, got, r in zip(mats, out, routes):
            expect(r, dict(engine=True, several_launches=False), f"{a.shape}")
            check(rig, f"{kw} of {a.shape}", a, kw, got)


def test_small_alignment_in_a_group_of_several_launches(rig):
    """a group's similarity kernel runs in several launches when its tallest alignment has 1800 rows: the 130-row alignment beside
    it then runs the multi-launch kernel, with per-column state between the launches"""
    shapes = [(1800, 40), (130, 64), (140, 20), (129, 33), (135, 21), (131, 30), (150, 17), (129, 5)]
    kws = [SIM[0], SIM[0], SIM[1], SIM[0], SIM[1], SIM[0], SIM[0], SIM[1]]
    mats = [synth_msa(m, n, 7300 + m + n) for m, n in shapes]
    batch = rig.batch()
    for _ in range(2):  # (the second call: the same lanes, the per-column state of the first still in the arena)
        out = batch.trim([(a, X, P(**kw)) for a, kw in zip(mats, kws)])
        routes = batch.last_routes()
        assert [r["group"] for r in routes[:2]] == [0, 0], routes
        expect(routes[0], MULTI, "1800 x 40")
        expect(routes[1], MULTI, "130 x 64 beside it")
        for r in routes[2:]:
            expect(r, LISTS, "the groups behind")
        for a, kw, got in zip(mats, kws, out):
            check(rig, f"{kw} of {a.shape}", a, kw, got)


# ---- b. every column's similarity value, through masks ----------------------------------------------------------------------
def oracle_mdk(a):
    vhash, dist = MATRICES["aa"]
    hit, dst = oracle.pair_counts(a)
    return oracle.similarity(a, oracle.weights(hit, dst), oracle.gaps(a)[0], vhash, dist)[0]


# (m, n, seed, route, values): values None = every distinct value of the oracle's MDK vector; a number = that many of them, spread
# over the sorted values with the smallest and the largest among them (an oracle trim of 1800 rows costs a tenth of a second)
PINNED = [(100, 96, 5, LANE, None), (127, 130, 5, LANE, None), (129, 130, 5, LISTS, None), (1800, 40, 5, MULTI, 16)]


@pytest.mark.parametrize("m,n,seed,route,values", PINNED, ids=[f"{m}x{n}" for m, n, *_ in PINNED])
def test_every_column_value_is_pinned_through_masks(rig, m, n, seed, route, values):
    """The engine returns no MDK vector, but a manual similarity trim keeps a column exactly when its value lies above the threshold:
    with the threshold at a column's value the oracle drops the column, with the float32 just below it keeps it.  One call carries the
    alignment twice per distinct value; masks equal to the oracle's at both thresholds fix the value of every column that holds it, to
    the bit -- the columns cut by the >= 80 % gaps rule (value 0) included."""
    a = synth_msa(m, n, seed)
    mdk = oracle_mdk(a)
    distinct = np.unique(mdk)
    if values is not None:
        distinct = distinct[np.unique(np.linspace(0, len(distinct) - 1, values).round().astype(int))]
        assert len(distinct) >= 16 and distinct[0] == mdk.min() == 0 and distinct[-1] == mdk.max()  # (0: a cut column)
    thresholds = []
    for v in distinct:
        thresholds += [np.nextafter(v, np.float32(-np.inf), dtype=np.float32), v]
    wants = [want_of(a, dict(similarity_threshold=float(t))) for t in thresholds]
    pinned = np.zeros(n, dtype=bool)
    for i, v in enumerate(distinct):  # (a condition on the inputs: the oracle's own masks flip at the value)
        below, at = wants[2 * i][0], wants[2 * i + 1][0]
        cols = mdk == v
        assert below[cols].all() and not at[cols].any(), f"the oracle's masks do not flip at {v!r}"
        pinned |= cols
    assert pinned.sum() == n if values is None else pinned.sum() >= 16
    batch = rig.batch()
    out = batch.trim([(a, X, P(similarity_threshold=float(t))) for t in thresholds])
    routes = batch.last_routes()
    assert sorted({r["group"] for r in routes}) == [0, 1, 2, 3]  # (like-shaped groups on one lane one after the other)
    for i, (t, got, want, r) in enumerate(zip(thresholds, out, wants, routes)):
        expect(r, route, f"threshold {t!r}")
        res, seq, info, rc, rows = got
        assert rc == _lib.OK
        wrong = np.flatnonzero(res != want[0])
        assert wrong.size == 0, f"{m} x {n}, threshold {t!r} ({'at' if i % 2 else 'below'} the value): columns {wrong[:8].tolist()} " \
                                f"with the oracle's values {mdk[wrong[:8]].tolist()}"
        assert np.array_equal(seq, want[1])
        assert info.kept_residues == int(res.sum()) and info.kept_sequences == int(seq.sum())


# ---- c. info by value ---------------------------------------------------------------------------------------------------------
def holed(a, rows=(), cols=()):
    a = a.copy()
    for r in rows:
        a[r, :] = GAP
    for c in cols:
        a[:, c] = GAP
    return a


def test_info_of_a_mixed_bag(rig):
    """every kind of trim the engine takes in one call, automated1 on alignments where the device gate picks gappyout and on ones where
    it picks strict, rows of gaps only (the warnings, the row they name): info by value"""
    bag = [(family(*CASES[name]), dict(method="automated1")) for name in ("conserved", "diverged", "few", "middle", "middle_max", "large_conserved", "wide")]
    gappy = holed(family(40, 300, 130, 0.5), rows=(3, 38))
    gappy2 = holed(family(150, 200, 240, 0.5), rows=(3, 148), cols=range(0, 200, 3))
    for a in (gappy, gappy2):
        bag += [(a, dict(method=method)) for method in ("strict", "automated1", "gappyout", "strictplus")]
    d = synth_msa(90, 140, 7400)
    d[70] = d[2]
    bag += [(d, dict(method="nogaps")), (d, dict(method="noallgaps")), (d, dict(gap_threshold=0.7)), (d, dict(similarity_threshold=0.3)),
            (d, dict(gap_threshold=0.6, similarity_threshold=0.2, conservation_percentage=40.0)),
            (d, dict(residue_overlap=0.5, sequence_overlap=60.0)), (d, dict(identity_threshold=0.3)), (d, dict(clusters=3)),
            (d, dict(method="noduplicateseqs")), (d, dict(gap_threshold=0.7, gap_window=2))]
    batch = rig.batch()
    out = batch.trim([(a, X, P(**kw)) for a, kw in bag])
    routes = batch.last_routes()
    selected = set()
    for k, ((a, kw), got, r) in enumerate(zip(bag, out, routes)):
        assert r["engine"], (k, a.shape, kw)
        want = check(rig, f"item {k}: {kw} of {a.shape}", a, kw, got)
        if kw.get("method") == "automated1":
            selected.add((got[2].selected_method, want[2].selected))
    assert selected == {(1, 1), (2, 2)}, "the automated1 inputs must cover both decisions of the device gate"
    for k in (7, 8, 9, 10):  # (the rows of gaps only are reported, and the undefined identity between them where identities are computed)
        assert out[k][2].warnings & _lib.W_ONLY_GAPS_SEQUENCES and out[k][2].warn_row == 3 and out[k][4] == [3, 38]
    assert out[7][2].warnings & _lib.W_UNDEFINED_IDENTITY and out[8][2].warnings & _lib.W_UNDEFINED_IDENTITY


def test_a_residue_outside_the_matrix(rig):
    """the same return code and (row, column, byte) as the single path and the oracle, from a lane-per-column group and from a list
    group; of two the first in the reference's order (column by column) wins; automated1 fails exactly when it selects strict; a
    residue in a column cut by the gaps rule, and any residue under a gap-only trim, is no failure"""
    def dense(m, n, seed, keep=0.3):
        a = family(m, n, seed, keep)
        a[:, 17] = ALPHA[np.arange(m) % 20]
        return a

    items = []
    for m, n in ((100, 96), (300, 100)):
        one = dense(m, n, 7500 + m)
        one[5, 17] = ord("J")
        two = one.copy()
        two[2, 40], two[9, 17], two[1, 90] = ord("O"), ord("O"), ord("*")
        star = dense(m, n, 7501 + m)
        star[m - 1, n - 1] = ord("*")  # (not a letter: MSA_E_INCORRECT_SYMBOL)
        cut = holed(dense(m, n, 7502 + m), cols=(30,))
        cut[4, 30] = ord("J")  # (a column of gaps but for this residue: never evaluated)
        calm = family(m, n, 1, 0.92)
        calm[5, 17] = ord("J")
        items += [(one, dict(method="strict")), (two, dict(method="strict")), (two, dict(similarity_threshold=0.2)), (star, dict(method="strictplus")),
                  (cut, dict(method="strict")), (one, dict(method="automated1")), (calm, dict(method="automated1")), (one, dict(method="gappyout")),
                  (dense(m, n, 7503 + m), dict(method="strict"))]
    batch = rig.batch()
    for _ in range(2):  # (twice: the failure's key of the first call must not survive in the arena)
        out = batch.trim([(a, X, P(**kw)) for a, kw in items])
        routes = batch.last_routes()
        failed = []
        for k, ((a, kw), got, r) in enumerate(zip(items, out, routes)):
            sim = kw.get("method") != "gappyout"
            expect(r, dict(engine=True, lane_per_column=sim and a.shape[0] <= 128, redone=False), f"item {k}")
            want = check(rig, f"item {k}: {kw} of {a.shape}", a, kw, got)
            failed.append(want.detail if isinstance(want, oracle.OracleError) else None)
        J, S = ord("J"), ord("*")
        assert failed[:9] == [(5, 17, J), (5, 17, J), (5, 17, J), (99, 95, S), None, (5, 17, J), None, None, None]
        assert failed[9:] == [(5, 17, J), (5, 17, J), (5, 17, J), (299, 99, S), None, (5, 17, J), None, None, None]


# ---- d. same layout, other content --------------------------------------------------------------------------------------------
def content(m, n, seed, keep, gappy):
    """a family (m copies of a root, each residue kept with probability `keep`); `gappy`: two columns in five hold gaps only, one in ten
    nine gaps in ten, the rest one in ten -- shorter lists, more columns cut, and the identities (counted over the columns in which
    either sequence holds a residue) hardly moved"""
    r = np.random.default_rng(seed)
    root = ALPHA[r.integers(0, 20, n)]
    a = np.where(r.random((m, n)) < keep, root[None, :], ALPHA[r.integers(0, 20, (m, n))])
    if gappy:
        kind = r.random(n)
        a[:, kind < 0.4] = GAP
        rare = (kind >= 0.4) & (kind < 0.5)
        a[(r.random((m, n)) < 0.9) & rare[None, :]] = GAP
        a[(r.random((m, n)) < 0.1) & ~rare[None, :]] = GAP
    else:
        a[r.random((m, n)) < 0.02] = GAP
    return np.ascontiguousarray(a, dtype=np.uint8)


@pytest.mark.parametrize("m,n,route", [(100, 96, LANE), (140, 130, LISTS), (1800, 24, MULTI)], ids=["100x96", "140x130", "1800x24"])
def test_same_layout_other_content(rig, m, n, route):
    """`engine_enqueue` zeroes the whole arena only when the layout signature (shapes, kinds, modes, the arena's address) differs
    from the one it was last zeroed for, else the result region alone.  Eight alignments of one shape, strict and automated1 in
    turn, are four groups of one layout: within a call the third group follows the first on its lane, and the next call follows
    with the same signature and other contents -- dense then gappy (shorter lists, more columns cut, no bad residue where there was
    one, the device gate falling the other way), and the reverse on a fresh object."""
    kws = [SIM[k % 2] for k in range(8)]
    dense = [content(m, n, 7600 + k, 0.30, False) for k in range(8)]
    dense[2][7, n // 2] = ord("J")
    dense[5][m - 1, n - 1] = ord("O")
    gappy = [content(m, n, 7650 + k, 0.92 if k % 4 == 1 else 0.30, True) for k in range(8)]
    wants = {id(a): want_of(a, kw) for mats in (dense, gappy) for a, kw in zip(mats, kws)}
    picks = [[wants[id(a)][2].selected for a, kw in zip(mats, kws) if kw["method"] == "automated1" and not isinstance(wants[id(a)], oracle.OracleError)]
             for mats in (dense, gappy)]
    assert set(picks[0]) == {2} and set(picks[1]) == {1, 2}, picks  # (dense: strict everywhere; gappy: some gappyout)
    assert isinstance(wants[id(dense[2])], oracle.OracleError) and isinstance(wants[id(dense[5])], oracle.OracleError)
    cut = [np.mean([(a == GAP).mean(axis=0) >= 0.8 for a in mats]) for mats in (dense, gappy)]
    assert cut[0] == 0 and cut[1] > 0.4
    for order in ((dense, gappy, dense), (gappy, dense, gappy)):
        batch = rig.batch()
        seen = []
        for mats in order:
            out = batch.trim([(a, X, P(**kw)) for a, kw in zip(mats, kws)])
            routes = batch.last_routes()
            seen.append([(r["group"], r["lane_per_column"], r["several_launches"], r["rows"]) for r in routes])
            assert [r["group"] for r in routes] == [0, 0, 1, 1, 2, 2, 3, 3]
            for k, (a, kw, got, r) in enumerate(zip(mats, kws, out, routes)):
                expect(r, route, f"alignment {k}")
                check(rig, f"alignment {k} ({kw}) of {'dense' if mats is dense else 'gappy'} contents", a, kw, got, want=wants[id(a)])
        assert seen[0] == seen[1] == seen[2], "the group split must be the same in every call"


def test_many_like_shaped_alignments_reuse_their_lanes(rig):
    """160 alignments of 100 x 64 with distinct contents: four groups of 40 on two lanes, the signature equal throughout"""
    r = np.random.default_rng(77)
    mats = []
    for k in range(160):
        a = synth_msa(100, 64, 7700 + k) if k % 3 else content(100, 64, 7700 + k, float(r.choice([0.3, 0.6, 0.9])), bool(k % 2))
        mats.append(a)
    kw = dict(method="strict")
    batch = rig.batch()
    out = batch.trim([(a, X, P(**kw)) for a in mats])
    routes = batch.last_routes()
    assert [r["group"] for r in routes] == [k // 40 for k in range(160)]
    for k, (a, got, r) in enumerate(zip(mats, out, routes)):
        expect(r, LANE, f"alignment {k}")
        check(rig, f"alignment {k}", a, kw, got)


# ---- e. row routes ------------------------------------------------------------------------------------------------------------
def letters_store(nbytes, seed):
    """residue letters, not zeros: a byte read past a row's n columns changes a count"""
    return ALPHA[np.random.default_rng(seed).integers(0, 20, nbytes)].copy()


def strided_view(store, a, stride, parity):
    """`a` as a view into `store` with rows `stride` bytes apart; the first row at an address that is 0 (`parity` 0) or 1 modulo 16"""
    m, n = a.shape
    off = (-store.ctypes.data) % 16 + parity
    v = np.lib.stride_tricks.as_strided(store[off:], shape=(m, n), strides=(stride, 1), writeable=True)
    v[:] = a
    assert v.ctypes.data % 16 == parity and v.strides == (stride, 1)
    return v


def test_row_routes_agree(rig):
    """the same contents through every way rows reach a group's arena, in one call: rows at the device pitch (one linear copy, slack
    and all), a 16-byte aligned wide view (a 2-D copy), an odd address (packed through staging), page-locked rows under a megabyte
    (fetched by fetch_rows_batch_kernel, at an aligned and at an odd stride), page-locked rows over a megabyte (a 2-D copy) beside the
    same rows pageable (packed)"""
    import torch

    a = synth_msa(100, 90, 7800)
    big = synth_msa(256, 4200, 7801)
    views, keep = [], []

    def pageable(x, stride, parity, route):
        store = letters_store(x.shape[0] * stride + 64, 7810 + stride)
        keep.append(store)
        views.append((strided_view(store, x, stride, parity), route))

    def locked(x, stride, route):
        t = torch.empty(x.shape[0] * stride + 64, dtype=torch.uint8).pin_memory()
        store = t.numpy()
        store[:] = letters_store(store.size, 7820 + stride)
        keep.append(t)
        views.append((strided_view(store, x, stride, 0), route))

    views.append((a, "packed"))          # contiguous rows of 90 bytes: neither the device pitch nor a multiple of 16
    pageable(a, 128, 0, "linear")        # the 64-byte padded row
    pageable(a, 128, 1, "linear")
    pageable(a, 112, 0, "copy_2d")
    pageable(a, 112, 1, "packed")
    pageable(a, 101, 1, "packed")
    locked(a, 112, "fetched")
    locked(a, 101, "fetched")
    locked(a, 128, "fetched")
    small = len(views)
    views.append((big, "packed"))        # rows of 4200 bytes: a multiple of 8 only
    locked(big, 4208, "copy_2d")         # 256 x 4224 bytes of device rows: more than fetch_max_bytes
    kws = (dict(method="strict"), dict(method="automated1"), dict(method="nogaps"), dict(residue_overlap=0.6, sequence_overlap=70.0),
           dict(method="noduplicateseqs"))
    items = [(v, kw, route) for v, route in views[:small] for kw in kws] + [(v, kws[0], route) for v, route in views[small:]]
    batch = rig.batch()
    out = batch.trim([(v, X, P(**kw)) for v, kw, _ in items])
    routes = batch.last_routes()
    wants = {}
    first = {}
    for k, ((v, kw, route), got, r) in enumerate(zip(items, out, routes)):
        what = f"item {k}: {kw} of {v.shape} at stride {v.strides[0]}, address % 16 = {v.ctypes.data % 16}"
        expect(r, dict(engine=True, rows=route), what)
        key = (v.shape, tuple(sorted(kw.items())))
        if key not in wants:
            wants[key] = want_of(v, kw)
        check(rig, what, v, kw, got, want=wants[key])
        fields = (got[0].tobytes(), got[1].tobytes(), tuple(info_fields(got[2]).items()), got[3], tuple(got[4]))
        assert first.setdefault(key, fields) == fields, f"{what}: differs from the same contents through another route"
    del keep


# ---- f. mixed types in one call -----------------------------------------------------------------------------------------------
def typed(kind, m, n, seed):
    """(alignment, indet, matrix) of a sequence type: protein, DNA, DNA with degenerate letters"""
    if kind == "aa":
        return synth_msa(m, n, seed), X, "aa"
    r = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGT" if kind == "nt" else b"ACGTRYKMSWBDHV", dtype=np.uint8)
    root = alpha[r.integers(0, 4, n)]
    a = np.where(r.random((m, n)) < r.beta(2, 2, n)[None, :], root[None, :], alpha[r.integers(0, len(alpha), (m, n))])
    a[r.random((m, n)) < r.beta(0.6, 1.8, n)[None, :]] = GAP
    a[(r.random((m, n)) < 0.01) & (a != GAP)] = N
    return np.ascontiguousarray(a, dtype=np.uint8), N, kind


@pytest.mark.parametrize("first", ["aa", "nt", "deg"])
def test_mixed_types_in_one_call(rig, first):
    """One set of similarity tables serves a call: the first taken alignment's (the largest m^2 n).  Similarity trims of another
    matrix or indetermination symbol go to the workers; trims that need no tables are the engine's whatever the type.  Every alignment
    equals the oracle's trim with its own matrix."""
    items = []
    for kind in ("aa", "nt", "deg"):
        shapes = [(210 if kind == first else 200, 150), (100, 96), (130, 70), (64, 257)]
        for j, (m, n) in enumerate(shapes):
            a, indet, matrix = typed(kind, m, n, 7900 + 10 * j + len(kind))
            items += [(a, indet, matrix, kw) for kw in (SIM[0], SIM[1], dict(method="gappyout"))[: 3 if j < 2 else 2]]
    order = np.random.default_rng(79).permutation(len(items))
    items = [items[i] for i in order]
    batch = rig.batch()
    for _ in range(2):
        out = batch.trim([(a, indet, P(matrix, **kw)) for a, indet, matrix, kw in items])
        routes = batch.last_routes()
        for k, ((a, indet, matrix, kw), got, r) in enumerate(zip(items, out, routes)):
            what = f"item {k}: {kw} of {matrix} {a.shape}"
            assert r["engine"] == (matrix == first or kw["method"] == "gappyout"), f"{what}: went {r}"
            check(rig, what, a, kw, got, matrix=matrix, indet=indet)
