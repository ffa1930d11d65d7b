"""FASTA parsed on the device (msa_upload_fasta, msa_trim_batch_fasta, pytrimal_amd.batch.trim_files) against the host
reader (msa_fasta_scan / msa_fasta_fill, Alignment.load) and the row path (trim_batch)."""
import ctypes
import glob
import io
import os
import random
import warnings

import numpy as np
import pytest

from conftest import DATA, GOLDEN
from pytrimal_amd import (Alignment, AutomaticTrimmer, ManualTrimmer, OverlapTrimmer, RepresentativeTrimmer,
                          SimilarityMatrix, _lib)
from pytrimal_amd.alignment import _VALID
from pytrimal_amd.batch import trim_batch, trim_files
from pytrimal_amd.synth import synth_msa

pytestmark = pytest.mark.gpu

# tests/test_api.py's cases of the host reader
FASTA_CASES = [
    b">a\nAC-GT\n>b x y\nAC\n-GT\n\n",
    b"leading garbage\n>a\nAB\n>b\nCD",
    b"> \nAB\n>b\nCD\n",
    b">a\r\nA B\r\n>b\r\nCD\r\n",
    b">a\nAB \n C\n>b\n A B C \n",
    b">only\n" + b"ACDEFGHIKLMNPQRSTVWY-" * 40 + b"\n",
]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def host_parse(text):
    """msa_fasta_scan + msa_fasta_fill: (rc, m, n, matrix, names, detail, seq_type)."""
    L = _lib.load()
    buf = np.frombuffer(text, dtype=np.uint8)
    m, n = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.msa_fasta_scan(buf.ctypes.data, buf.size, ctypes.byref(m), ctypes.byref(n)) == 0
    m, n = m.value, n.value
    matrix = np.zeros((m, n), dtype=np.uint8)
    off, ln = np.zeros(max(m, 1), dtype=np.int64), np.zeros(max(m, 1), dtype=np.int32)
    det = _lib.ErrDetail()
    rc = L.msa_fasta_fill(buf.ctypes.data, buf.size, m, n, matrix.ctypes.data, off.ctypes.data, ln.ctypes.data,
                          _VALID.view(np.uint8).ctypes.data, ctypes.byref(det))
    names = [bytes(text[o:o + k]) for o, k in zip(off[:m].tolist(), ln[:m].tolist())]
    ty = Alignment._from_parts(names, matrix)._alignment_type() if rc == 0 else None
    return rc, m, n, matrix, names, (det.row, det.col, det.byte), ty


def device_parse(ctx, text):
    try:
        info = ctx.upload_fasta(text)
    except _lib.MsaError as err:
        return err.code, (err.detail.row, err.detail.col, err.detail.byte)
    off, ln = ctx.text_names()
    names = [bytes(text[o:o + k]) for o, k in zip(off.tolist(), ln.tolist())]
    return 0, info, ctx.download_rows(), names


def check_ingest(ctx, text):
    rc, m, n, matrix, names, det, ty = host_parse(text)
    got = device_parse(ctx, text)
    if rc != 0:
        assert got == (rc, det), (text[:80], got, rc, det)
        return
    assert got[0] == 0, (text[:80], got)
    info, rows, dnames = got[1:]
    assert (info.m, info.n) == (m, n)
    assert np.array_equal(rows, matrix)
    assert dnames == names
    assert info.seq_type == ty
    assert ctx.last_paths()["upload"] == "fasta"


def wrap(names, rows, width=60, eol=b"\n", lead=b"", header_sep=b" "):
    out = []
    for nm, r in zip(names, rows):
        out.append(lead + b">" + nm + header_sep + b"desc" + eol)
        r = bytes(r)
        step = width if width else max(len(r), 1)
        for i in range(0, max(len(r), 1), step):
            out.append(lead + r[i:i + step] + eol)
    return b"".join(out)


def synth_text(m, n, seed, kind="protein", **kw):
    rng = np.random.default_rng(seed)
    alpha = {"protein": b"ACDEFGHIKLMNPQRSTVWY", "dna": b"ACGT", "rna": b"ACGU", "deg": b"ACGTRYKMN"}[kind]
    a = np.frombuffer(alpha, dtype=np.uint8)[rng.integers(0, len(alpha), size=(m, n))]
    a[rng.random((m, n)) < 0.2] = ord("-")
    return wrap([b"s%d" % i for i in range(m)], a, **kw)


def test_ingest_cases_and_fixtures(ctx):
    for text in FASTA_CASES:
        check_ingest(ctx, text)
    files = sorted(glob.glob(os.path.join(DATA, "*.fasta")) + glob.glob(os.path.join(DATA, "*.afa")))
    assert files
    for path in files:
        with open(path, "rb") as f:
            check_ingest(ctx, f.read())


@pytest.mark.parametrize("kind", ["protein", "dna", "rna", "deg"])
def test_ingest_layout_variations(ctx, kind):
    for width, eol, lead, sep in [(60, b"\n", b"", b" "), (80, b"\n", b"", b"\t"), (0, b"\n", b"", b" "), (60, b"\r\n", b"", b" "),
                                  (60, b"\n", b"  \t", b" "), (7, b"\n\n", b"", b"\t\t")]:
        text = synth_text(37, 211, 5, kind, width=width, eol=eol, lead=lead, header_sep=sep)
        check_ingest(ctx, text)
        check_ingest(ctx, b"junk before\n  \n" + text.rstrip(b"\n"))  # junk before the first header, no trailing newline
    check_ingest(ctx, b">\nAC-\n>   \t\nAG-\n> x\nTT-")  # empty names


def test_ingest_tile_boundaries(ctx):
    rng = np.random.default_rng(3)
    row = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY-", dtype=np.uint8)[rng.integers(0, 21, size=300000)]
    check_ingest(ctx, b">one\n" + bytes(row) + b"\n")
    rows = np.frombuffer(b"ACGT-", dtype=np.uint8)[rng.integers(0, 5, size=(4, 100000))]
    check_ingest(ctx, wrap([b"a", b"b", b"c", b"d"], rows, width=0))
    small = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(100000, 3))]
    check_ingest(ctx, b"".join(b">r%d\n%s\n" % (i, bytes(r)) for i, r in enumerate(small)))


def test_layout_parity_with_packed_upload(ctx):
    vhash, dist = SimilarityMatrix.aa()._device_arrays()
    big = synth_msa(300, 900, 11)
    for m, n, seed in [(64, 333, 1), (129, 1000, 2)]:
        for before in (None, big):
            if before is not None:
                ctx.upload(before, ord("X"))
                ctx.gaps()
            a = synth_msa(m, n, seed)
            text = wrap([b"s%d" % i for i in range(m)], a)
            info = ctx.upload_fasta(text)
            assert (info.m, info.n) == (m, n)
            g1, x1 = ctx.gaps(with_indet=True)
            h1, d1 = ctx.pair_counts()
            _, q1 = ctx.similarity(vhash, dist)
            ctx.upload(a, ord("X") if info.seq_type & 4 else ord("N"))
            g2, x2 = ctx.gaps(with_indet=True)
            h2, d2 = ctx.pair_counts()
            _, q2 = ctx.similarity(vhash, dist)
            assert np.array_equal(g1, g2) and np.array_equal(x1, x2)
            assert np.array_equal(h1, h2) and np.array_equal(d1, d2)
            assert np.array_equal(q1.view(np.uint32), q2.view(np.uint32))


ERROR_TEXTS = [
    b">a\nAC1T\n>b\nACGT\n",
    b">a\nAC\x00T\n>b\nACGT\n",
    b">a\nACGT\n>b\nAC\xc3T\n",
    b">a\nACGT\n>b\nACG\n>c\nACGT\n",          # short record
    b">a\nACGT\n>b\nACGTA\n",                    # long record, at the end
    b">a\nACGT\n>b\nACGTAA1\n>c\nACGT\n",        # bad byte beyond n in a long record
    b">a\nACGT\n>b\nACG\n>c\nAC1T\n",            # mismatch in row 1, bad residue in row 2
    b">a\nACGT\n>b\nA1GT\n>c\nACG\n",            # the reverse
    b">a\nACGT\n>b\nAC>T\n",                     # '>' inside a sequence line
]


def test_error_parity(ctx, tmp_path):
    for text in ERROR_TEXTS:
        check_ingest(ctx, text)
        path = tmp_path / "bad.fasta"
        path.write_bytes(text)
        with pytest.raises(ValueError) as host:
            Alignment.load(str(path))
        with pytest.raises(ValueError) as dev:
            trim_files(AutomaticTrimmer("gappyout"), [str(path)])
        assert str(dev.value) == str(host.value)


def fuzz_text(rng):
    m, n = rng.randint(1, 12), rng.randint(0, 40)
    alpha = rng.choice([b"ACGT-", b"ACGU-N", b"ACDEFGHIKLMNPQRSTVWY-.?*", b"ACGTRYKMN-x1>\x00 \t"])
    parts = [rng.choice([b"", b"junk\n", b"  \n", b"\r\n"])]
    for i in range(m):
        parts.append(rng.choice([b"", b" ", b"\t"]) + b">" + rng.choice([b"", b" ", b"n%d" % i, b"  n%d x" % i, b"\tq"]) +
                     rng.choice([b"\n", b"\r\n"]))
        length = n if rng.random() < 0.85 else rng.randint(0, n + 3)
        body = bytes(rng.choice(alpha) for _ in range(length))
        w = rng.randint(1, 50)
        for j in range(0, len(body), w):
            parts.append(rng.choice([b"", b" "]) + body[j:j + w] + rng.choice([b"\n", b"\r\n", b" \n", b"\n\n"]))
    text = b"".join(parts)
    return text[:-1] if rng.random() < 0.3 and text else text


def test_seeded_ingest_fuzz(ctx):
    rng = random.Random(20261016)
    for _ in range(400):
        check_ingest(ctx, fuzz_text(rng))


def capture(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = fn()
    return out, [(type(x.message), str(x.message)) for x in w if issubclass(x.category, RuntimeWarning)]


TRIMMERS = [
    lambda: AutomaticTrimmer("strict"), lambda: AutomaticTrimmer("strictplus"), lambda: AutomaticTrimmer("gappyout"),
    lambda: AutomaticTrimmer("nogaps"), lambda: AutomaticTrimmer("noallgaps"), lambda: AutomaticTrimmer("automated1"),
    lambda: AutomaticTrimmer("noduplicateseqs"),
    lambda: ManualTrimmer(gap_threshold=0.6, similarity_threshold=0.1), lambda: ManualTrimmer(gap_absolute_threshold=3, window=2),
    lambda: ManualTrimmer(gap_threshold=0.4, conservation_percentage=50, gap_window=1, similarity_window=2),
    lambda: OverlapTrimmer(40, 0.5), lambda: RepresentativeTrimmer(clusters=5), lambda: RepresentativeTrimmer(identity_threshold=0.5),
]


def write_files(tmp_path):
    paths = []
    for k, (m, n, kind) in enumerate([(30, 120, "protein"), (25, 200, "dna"), (12, 90, "deg"), (40, 300, "protein")]):
        p = tmp_path / f"a{k}.fasta"
        p.write_bytes(synth_text(m, n, 100 + k, kind))
        paths.append(str(p))
    ali = Alignment.load(paths[0])
    clw = tmp_path / "a.clw"
    clw.write_bytes(ali.dumps("clustal").encode())
    paths.insert(2, str(clw))
    return paths


def test_trim_parity(tmp_path):
    paths = write_files(tmp_path)
    for make in TRIMMERS:
        for matrix in (None, SimilarityMatrix.aa()):
            for masks_only in (True, False):
                t = make()
                ref, wref = capture(lambda: trim_batch(t, [Alignment.load(p) for p in paths], matrix, shard=False, masks_only=masks_only))
                got, wgot = capture(lambda: trim_files(t, paths, matrix, masks_only=masks_only))
                assert wgot == wref, make()
                assert len(got) == len(ref)
                for a, b in zip(got, ref):
                    if masks_only:
                        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                        continue
                    assert a.residues_mask == b.residues_mask and a.sequences_mask == b.sequences_mask
                    assert a.names == b.names and list(a.sequences) == list(b.sequences)
                    assert a.sequence_type == b.sequence_type
                    assert a.dumps("fasta") == b.dumps("fasta")
                    try:
                        ta = a.terminal_only()
                    except RuntimeError as err:
                        with pytest.raises(RuntimeError, match=str(err)):
                            b.terminal_only()
                    else:
                        assert ta.residues_mask == b.terminal_only().residues_mask


def test_file_objects_and_format(tmp_path):
    paths = write_files(tmp_path)
    t = AutomaticTrimmer("strict")
    ref = trim_batch(t, [Alignment.load(p) for p in paths[:2]], shard=False, masks_only=True)
    objs = [io.BytesIO(open(p, "rb").read()) for p in paths[:2]]
    got = trim_files(t, objs, format="FASTA", masks_only=True)
    for a, b in zip(got, ref):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_c5_from_files(tmp_path):
    golden = np.load(os.path.join(GOLDEN, "configs.npz"))
    paths = []
    for k in range(64):
        a = synth_msa(1000, 4000, 2000 + k)
        p = tmp_path / f"c5_{k}.fasta"
        p.write_bytes(wrap([b"s%d" % i for i in range(1000)], a, header_sep=b""))
        paths.append(str(p))
    out = trim_files(AutomaticTrimmer("automated1"), paths, threads=4, masks_only=True)
    for k, (res, seq) in enumerate(out):
        assert np.array_equal(res, np.unpackbits(golden[f"C5.{k}.res"])[:4000].astype(bool)), k
        assert np.array_equal(seq, np.unpackbits(golden[f"C5.{k}.seq"])[:1000].astype(bool)), k


def test_failures_beyond_the_first_tile(ctx):
    """Failures in later tiles of a multi-tile text: the detail pass runs on the tile that holds the first failure."""
    base = synth_text(1000, 4000, 31, "protein")
    lines = base.split(b"\n")

    def row_line(r, j=0):  # line j of record r's sequence: a header and ceil(4000 / 60) = 67 lines per record
        return r * 68 + 1 + j

    assert lines[row_line(700) - 1] == b">s700 desc" and len(lines[row_line(300, 66)]) == 40

    def edit(fn):
        ls = list(lines)
        fn(ls)
        return b"\n".join(ls)

    bad = edit(lambda ls: ls.__setitem__(row_line(700, 3), ls[row_line(700, 3)][:5] + b"1" + ls[row_line(700, 3)][6:]))
    short = edit(lambda ls: ls.__setitem__(row_line(500, 10), ls[row_line(500, 10)][1:]))
    long_then_bad = edit(lambda ls: (ls.__setitem__(row_line(300), ls[row_line(300)] + b"A"),
                                     ls.__setitem__(row_line(301, 2), b"#" + ls[row_line(301, 2)][1:])))
    bad_then_short = edit(lambda ls: (ls.__setitem__(row_line(300, 66), b"\x00" + ls[row_line(300, 66)][1:]),
                                      ls.__setitem__(row_line(301), ls[row_line(301)][2:])))
    short_last = base.rstrip(b"\n")[:-1] + b"\n"
    long_last = base.rstrip(b"\n") + b"AC"
    for text in (bad, short, long_then_bad, bad_then_short, short_last, long_last):
        assert len(text) > 4 * 4096
        check_ingest(ctx, text)


def test_vertical_tab_form_feed_and_type_boundaries(ctx):
    check_ingest(ctx, b">a\x0bname\x0c\nAC\x0bGT\x0c\n\x0b\x0c\n>b\nA\x0cCGT\n")
    # the 0.7 quotient of detect_alignment_type: 7 of 10 letters (0.7f < 0.7), 14 of 20, 70 of the first 100, one more or less
    for nt, k in [(7, 10), (14, 20), (70, 100), (71, 100), (69, 100), (8, 10), (6, 10)]:
        row = b"A" * nt + b"E" * (k - nt) + b"-" * 5 + b"E" * 40  # (letters past the first 100 do not count)
        check_ingest(ctx, b">x\n" + row + b"\n>y\n" + b"ACGT" * (len(row) // 4) + b"ACGT"[:len(row) % 4] + b"\n")
    rng = np.random.default_rng(9)
    for alpha, ty in ((b"ACGTNX", 1), (b"ACGUNX", 2), (b"ACGTRYKMNX", 9)):  # nucleotide texts: indet 'N', not 'X'
        a = np.frombuffer(alpha[:4], dtype=np.uint8)[rng.integers(0, 4, size=(40, 300))]
        rest = rng.random((40, 300)) < 0.08
        a[rest] = np.frombuffer(alpha[4:], dtype=np.uint8)[rng.integers(0, len(alpha) - 4, size=int(rest.sum()))]
        info = ctx.upload_fasta(wrap([b"s%d" % i for i in range(40)], a))
        assert info.seq_type == ty
        _, x = ctx.gaps(with_indet=True)
        assert np.array_equal(x, (a == ord("N")).sum(axis=0)) and x.any()


def test_seeded_multi_tile_fuzz(ctx):
    rng = random.Random(20261017)
    for _ in range(12):
        m, n = rng.randint(100, 300), rng.randint(150, 600)
        text = bytearray(synth_text(m, n, rng.randint(0, 10 ** 6), rng.choice(["protein", "dna", "deg"]),
                                    width=rng.choice([0, 60, 61]), eol=rng.choice([b"\n", b"\r\n"])))
        for _ in range(rng.randint(0, 2)):  # a defect or two anywhere
            at = rng.randrange(len(text))
            op = rng.randrange(3)
            if op == 0:
                text[at] = rng.choice(b"1#\x00\xc3")
            elif op == 1 and text[at] not in b">\n":
                del text[at]
            else:
                text.insert(at, ord("A"))
        check_ingest(ctx, bytes(text))


def test_trim_files_reads_a_pipe(tmp_path):
    import threading

    text = synth_text(30, 200, 77, "protein")
    plain = tmp_path / "plain.fasta"
    plain.write_bytes(text)
    fifo = tmp_path / "pipe.fasta"
    os.mkfifo(fifo)
    feeder = threading.Thread(target=lambda: fifo.write_bytes(text), daemon=True)
    feeder.start()
    t = AutomaticTrimmer("strict")
    got = trim_files(t, [str(fifo)], masks_only=True)
    feeder.join(5)
    ref = trim_batch(t, [Alignment.load(str(plain))], shard=False, masks_only=True)
    assert np.array_equal(got[0][0], ref[0][0]) and np.array_equal(got[0][1], ref[0][1])


def test_fasta_results_belong_to_the_last_call(tmp_path):
    from pytrimal_amd.batch import _native_batch

    path = tmp_path / "a.fasta"
    path.write_bytes(synth_text(20, 100, 1, "protein"))
    t = AutomaticTrimmer("strict")
    trim_files(t, [str(path)], masks_only=True)
    b = _native_batch(int(os.environ.get("PYTRIMAL_AMD_DEVICE", "0")), 6)
    assert b.lib.msa_batch_fasta_result(b.h, 0, None, None, None, None, None, None, None, None) == _lib.OK
    trim_batch(t, [Alignment.load(str(path))], shard=False, masks_only=True)
    assert b.lib.msa_batch_fasta_result(b.h, 0, None, None, None, None, None, None, None, None) == _lib.E_INVALID


def test_nothing_of_a_call_survives_into_the_next_kind_of_call():
    """a rows call after a text call with `emit` and `want_rows`, and a text call after a rows call, on one batch object:
    the masks fresh batch objects give, and no rows or text that only the earlier call asked for"""
    shapes = [(30, 120, "protein"), (25, 200, "dna"), (12, 90, "deg"), (40, 300, "protein")]
    texts = [synth_text(m, n, 40 + k, kind) for k, (m, n, kind) in enumerate(shapes)]
    t = ManualTrimmer(gap_threshold=0.7, similarity_threshold=0.3)
    params3, _keep = t._fasta_params(None)
    items = [t._prepare(Alignment.load(io.BytesIO(x), "fasta"))[1:4] for x in texts]

    def rows_call(b):
        outs = b.trim(items)
        assert [o[3] for o in outs] == [_lib.OK] * len(items)
        return [(o[0].copy(), o[1].copy()) for o in outs]

    def text_call(b, **kw):
        recs = b.trim_fasta(texts, _VALID.view(np.uint8), params3, **kw)
        assert [(r.parse_rc, r.rc) for r in recs] == [(_lib.OK, _lib.OK)] * len(texts)
        return recs

    def same(got, want):
        return len(got) == len(want) and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, want))

    fresh = _lib.Batch(None, 3)
    want_rows = rows_call(fresh)
    fresh.close()
    fresh = _lib.Batch(None, 3)
    want_text = [(r.keep_res, r.keep_seq) for r in text_call(fresh)]
    fresh.close()
    assert not all(res.all() for res, _ in want_rows)  # (the trim removes something)
    b = _lib.Batch(None, 3)
    try:
        first = text_call(b, want_rows=True, emit="clustal")
        assert all(r.rows is not None and r.text for r in first)
        assert same(rows_call(b), want_rows)
        after = text_call(b)
        assert same([(r.keep_res, r.keep_seq) for r in after], want_text)
        assert all(r.rows is None and r.text is None for r in after)
        assert same(rows_call(b), want_rows)
    finally:
        b.close()
