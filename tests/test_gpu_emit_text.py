"""Trimmed alignment text composed on the device (msa_emit_text, msa_trim_batch_fasta_emit, trim_files(..., output=...))
against the host writers (`TrimmedAlignment.dumps` / `dump`) and the files trimAl wrote: exact byte comparisons."""
import glob
import io
import os
import random
import warnings

import numpy as np
import pytest

from conftest import DATA, EXAMPLE_001, EXAMPLE_001_NAMES, data_path
from pytrimal_amd import (Alignment, AutomaticTrimmer, ManualTrimmer, OverlapTrimmer, RepresentativeTrimmer,
                          TrimmedAlignment, _lib)
from pytrimal_amd.batch import trim_files
from pytrimal_amd.synth import synth_msa
from test_emit_text_api import FORMATS, MASK_KINDS, SHAPES, masks_for, names_for
from test_gpu_fasta_device import FASTA_CASES, synth_text, wrap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def host_text(names, a, keep_res, keep_seq, fmt):
    return TrimmedAlignment._from_parts(names, a, 0, keep_seq, keep_res).dumps(fmt).encode()


@pytest.mark.parametrize("m,n", SHAPES)
def test_emit_text_after_a_row_upload(ctx, m, n):
    rng = np.random.default_rng(m * 1000 + n)
    a = np.ascontiguousarray(synth_msa(m, max(n, 1), 5)[:, :n])
    names = names_for(m, rng)
    ctx.upload(a, ord("X"))
    for kind in MASK_KINDS:
        keep_res, keep_seq = masks_for(kind, m, n, rng)
        for fmt in FORMATS:
            want = host_text(names, a, keep_res, keep_seq, fmt)
            assert ctx.emit_text(fmt, keep_res, keep_seq, names) == want, (kind, fmt)
            if kind == "full":
                assert ctx.emit_text(fmt, names=names) == want, fmt  # (no masks: keep all)
            assert _lib.text_size(fmt, [len(x) for x, k in zip(names, keep_seq) if k], int(keep_res.sum())) == len(want)
    with pytest.raises(_lib.MsaError):  # the rows came without a text: there are no names on the device
        ctx.emit_text("fasta")
    with pytest.raises(ValueError):
        ctx.emit_text("phylip", names=names)
    # a kept name with a byte >= 0x80 is reported, not written; a name that is not kept does not matter
    odd = list(names)
    odd[-1] = "séq".encode("utf-8")
    assert ctx.emit_text("clustal", names=odd) is None
    if m > 1:
        keep_seq = np.ones(m, dtype=bool)
        keep_seq[-1] = False
        assert ctx.emit_text("clustal", None, keep_seq, odd) == host_text(names, a, np.ones(n, dtype=bool), keep_seq, "clustal")


def check_text(ctx, text, rng):
    """upload_fasta + emit_text with the text's own names against the host reader + the host writer, full and random masks"""
    ali = Alignment.load(io.BytesIO(text), "fasta")
    info = ctx.upload_fasta(text)
    m, n = ali._matrix.shape
    assert (info.m, info.n) == (m, n)
    for kind in ("full", "random"):
        keep_res, keep_seq = masks_for(kind, m, n, rng)
        for fmt in FORMATS:
            want = host_text(ali._names, ali._matrix, keep_res, keep_seq, fmt)
            got = ctx.emit_text(fmt, keep_res, keep_seq) if kind == "random" else ctx.emit_text(fmt)
            assert got == want, (kind, fmt, text[:60])


def test_emit_text_with_the_names_of_the_text(ctx):
    rng = np.random.default_rng(17)
    for text in FASTA_CASES:
        check_text(ctx, text, rng)
    files = sorted(glob.glob(os.path.join(DATA, "*.fasta")) + glob.glob(os.path.join(DATA, "*.afa")))
    assert files
    for path in files:
        with open(path, "rb") as f:
            check_text(ctx, f.read(), rng)
    # a trim in between changes nothing; a row upload behind the text takes the text's names away
    text = synth_text(30, 200, 3, "protein")
    ctx.upload_fasta(text)
    params, _keep = AutomaticTrimmer("gappyout")._fasta_params(None)
    keep_res, keep_seq, _ = ctx.trim(params[0])
    ali = Alignment.load(io.BytesIO(text), "fasta")
    assert ctx.emit_text("fasta", keep_res, keep_seq) == host_text(ali._names, ali._matrix, keep_res, keep_seq, "fasta")
    ctx.upload(ali._matrix, ord("X"))
    with pytest.raises(_lib.MsaError):
        ctx.emit_text("fasta")
    assert ctx.emit_text("fasta", names=ali._names) == ali.dumps("fasta").encode()


ENOG_CASES = [
    (lambda: ManualTrimmer(gap_threshold=0.9, conservation_percentage=60), "ENOG411BWBU.cons60.gt90.fasta"),
    (lambda: ManualTrimmer(gap_threshold=0.4, conservation_percentage=40), "ENOG411BWBU.cons40.gt40.fasta"),
    (lambda: OverlapTrimmer(80, 0.8), "ENOG411BWBU.seq80.res80.fasta"),
    (lambda: OverlapTrimmer(40, 0.6), "ENOG411BWBU.seq40.res60.fasta"),
    (lambda: RepresentativeTrimmer(identity_threshold=0.75), "ENOG411BWBU.maxidentity75.fasta"),
    (lambda: RepresentativeTrimmer(identity_threshold=0.7), "ENOG411BWBU.id70.fasta"),
    (lambda: RepresentativeTrimmer(identity_threshold=0.5), "ENOG411BWBU.id50.fasta"),
    (lambda: AutomaticTrimmer("noduplicateseqs"), "ENOG411BWBU.noduplicateseqs.fasta"),
]


@pytest.mark.parametrize("make,fname", ENOG_CASES, ids=[f for _, f in ENOG_CASES])
def test_files_to_files_reproduces_trimal_fixtures(tmp_path, make, fname):
    """files in, files out, against the files trimAl wrote for the reference's tests"""
    with open(data_path(fname), "rb") as f:
        expected = f.read()
    out = tmp_path / "out.fasta"
    masks = trim_files(make(), [data_path("ENOG411BWBU.seq40.res60.fasta")], masks_only=True, output=[str(out)])
    assert out.read_bytes() == expected
    assert len(masks) == 1 and masks[0][0].dtype == bool


def test_files_to_files_reproduces_trimal_clustal_fixture(tmp_path):
    src = tmp_path / "example.fasta"
    src.write_bytes(wrap(EXAMPLE_001_NAMES, [s.encode() for s in EXAMPLE_001]))
    out = tmp_path / "out.clw"
    trim_files(ManualTrimmer(gap_threshold=0.9, window=3), [str(src)], masks_only=True, output=[str(out)], output_format="clustal")
    with open(data_path("example.001.gt90.w3.clw"), "rb") as f:
        expected = f.read()
    got = out.read_bytes()
    assert got.split(b"\n", 1)[0] == b"CLUSTAL multiple sequence alignment"
    assert got.split(b"\n", 1)[1] == expected.split(b"\n", 1)[1]


def capture(fn):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = fn()
    return out, [(type(x.message), str(x.message)) for x in w if issubclass(x.category, RuntimeWarning)]


def only_gaps_text():
    """five sequences with residues in columns 0 .. 29, a sixth with residues in columns 30 .. 39 only: a gap threshold of 0.5
    removes the last ten columns and leaves the sixth sequence with gaps only"""
    rng = np.random.default_rng(23)
    a = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[rng.integers(0, 20, size=(6, 40))].copy()
    a[:5, 30:] = ord("-")
    a[5, :30] = ord("-")
    return wrap([b"g%d" % i for i in range(6)], a)


def small_files(tmp_path):
    paths = []
    for k, (m, n, kind) in enumerate([(30, 120, "protein"), (25, 200, "dna"), (12, 90, "deg"), (40, 300, "protein")]):
        p = tmp_path / f"a{k}.fasta"
        p.write_bytes(synth_text(m, n, 100 + k, kind))
        paths.append(str(p))
    clw = tmp_path / "a.clw"  # a Clustal input and a text of empty records: the host route
    clw.write_bytes(Alignment.load(paths[0]).dumps("clustal").encode())
    paths.insert(2, str(clw))
    empty = tmp_path / "empty.fasta"
    empty.write_bytes(b">a\n\n>b\n\n")
    paths.insert(4, str(empty))
    gaps = tmp_path / "gaps.fasta"
    gaps.write_bytes(only_gaps_text())
    paths.append(str(gaps))
    return paths


def run_both(trimmer_of, paths, fmt, masks_only, tmp_path, tag):
    """trim_files with and without `output` (paths and file objects mixed): the same return value, the same warnings, and
    the bytes `dumps` gives for the objects the call returns without `masks_only`"""
    objects, wobj = capture(lambda: trim_files(trimmer_of(), paths))
    plain, wplain = capture(lambda: trim_files(trimmer_of(), paths, masks_only=masks_only))
    outs = [io.BytesIO() if k % 3 == 1 else str(tmp_path / f"{tag}_{k}.out") for k in range(len(paths))]
    got, wgot = capture(lambda: trim_files(trimmer_of(), paths, masks_only=masks_only, output=outs, output_format=fmt))
    assert wgot == wplain == wobj
    assert len(got) == len(plain) == len(paths)
    for a, b in zip(got, plain):
        if masks_only:
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        else:
            assert a.residues_mask == b.residues_mask and a.sequences_mask == b.sequences_mask
            assert a.names == b.names and list(a.sequences) == list(b.sequences)
    for k, (o, t) in enumerate(zip(outs, objects)):
        written = o.getvalue() if isinstance(o, io.BytesIO) else open(o, "rb").read()
        assert written == t.dumps(fmt).encode("ascii"), (tag, k, fmt)
    return wgot


TRIMMER_KINDS = [
    ("automatic", lambda: AutomaticTrimmer("automated1")),
    ("manual", lambda: ManualTrimmer(gap_threshold=0.5)),
    ("overlap", lambda: OverlapTrimmer(40, 0.5)),
    ("representative", lambda: RepresentativeTrimmer(identity_threshold=0.5)),
    ("noduplicateseqs", lambda: AutomaticTrimmer("noduplicateseqs")),
]


@pytest.mark.parametrize("kind,make", TRIMMER_KINDS, ids=[k for k, _ in TRIMMER_KINDS])
def test_output_equals_dumps_on_a_mixed_call(tmp_path, kind, make):
    paths = small_files(tmp_path)
    for fmt, masks_only in [("fasta", True), ("clustal", False), ("fasta_m10", True), ("phylip", True), ("CLUSTAL", True), ("fasta", False)]:
        seen = run_both(make, paths, fmt, masks_only, tmp_path, f"{kind}_{fmt}_{int(masks_only)}")
        if kind == "manual":  # the trim that leaves a sequence with gaps only still says so
            assert any("composed only by gaps" in msg and "g5" in msg for _, msg in seen), seen


def test_only_gaps_warning_is_still_raised(tmp_path):
    src = tmp_path / "gaps.fasta"
    src.write_bytes(only_gaps_text())
    out = tmp_path / "gaps.out"
    with pytest.warns(RuntimeWarning, match="Removing sequence 'g5' composed only by gaps"):
        masks = trim_files(ManualTrimmer(gap_threshold=0.5), [str(src)], masks_only=True, output=[str(out)])
    assert not masks[0][1][5] and masks[0][1][:5].all()
    assert out.read_bytes().count(b">") == 5


def test_output_of_large_texts(tmp_path):
    """a C5-sized text (1000 x 4000) and a tall one (20000 x 500) beside small ones, strict"""
    paths = []
    for k, (m, n, seed) in enumerate([(1000, 4000, 2000), (40, 300, 5), (20000, 500, 77)]):
        a = synth_msa(m, n, seed)
        p = tmp_path / f"big{k}.fasta"
        p.write_bytes(wrap([b"s%d" % i for i in range(m)], a, header_sep=b""))
        paths.append(str(p))
    for fmt, masks_only in [("fasta", True), ("clustal", True)]:
        run_both(lambda: AutomaticTrimmer("strict"), paths, fmt, masks_only, tmp_path, f"big_{fmt}")


def test_non_ascii_names_take_the_host_writer(tmp_path):
    rows = synth_msa(8, 150, 9).copy()
    rows[7] = rows[6]  # (a duplicate: noduplicateseqs removes one of the two)
    for odd in ("séq".encode("utf-8"), b"s\xffq"):
        for at in (0, 7):
            names = [b"n%d" % i for i in range(8)]
            names[at] = odd
            src = tmp_path / "odd.fasta"
            src.write_bytes(wrap(names, rows))
            for make in (lambda: AutomaticTrimmer("noduplicateseqs"), lambda: AutomaticTrimmer("gappyout")):
                for fmt in ("fasta", "clustal"):
                    t = trim_files(make(), [str(src)])[0]
                    want = io.BytesIO()
                    try:
                        t.dump(want, fmt)
                    except UnicodeError as err:  # the writer's own refusal: the same one from the call
                        for masks_only in (True, False):
                            with pytest.raises(type(err)):
                                trim_files(make(), [str(src)], masks_only=masks_only, output=[io.BytesIO()], output_format=fmt)
                        continue
                    for masks_only in (True, False):
                        got = io.BytesIO()
                        trim_files(make(), [str(src)], masks_only=masks_only, output=[got], output_format=fmt)
                        assert got.getvalue() == want.getvalue()


def test_a_failure_in_the_middle_writes_nothing(tmp_path):
    good = synth_text(30, 120, 1, "protein")
    lines = good.split(b"\n")
    assert not lines[7].startswith(b">")
    lines[7] = lines[7][1:]  # one residue short
    bad = b"\n".join(lines)
    paths, outs = [], []
    for k, text in enumerate([good, bad, good]):
        p = tmp_path / f"f{k}.fasta"
        p.write_bytes(text)
        paths.append(str(p))
        outs.append(str(tmp_path / f"f{k}.out"))
    with pytest.raises(ValueError) as today:
        trim_files(AutomaticTrimmer("strict"), paths, masks_only=True)
    assert "Sequence length mismatch" in str(today.value)
    for masks_only in (True, False):
        with pytest.raises(ValueError) as err:
            trim_files(AutomaticTrimmer("strict"), paths, masks_only=masks_only, output=outs)
        assert str(err.value) == str(today.value)
        assert not any(os.path.exists(o) for o in outs)


def fuzz_case(rng):
    m, n = rng.randint(1, 300), rng.randint(0, 700)
    alpha = np.frombuffer(rng.choice([b"ACGT-", b"ACGU-N", b"ACDEFGHIKLMNPQRSTVWY-", b"ACGTRYKMN-"]), dtype=np.uint8)
    a = alpha[np.random.default_rng(rng.getrandbits(32)).integers(0, len(alpha), size=(m, n))]
    names = [bytes(rng.choice(b"abcXYZ019_|.") for _ in range(rng.choice([0, 1, 3, 9, 10, 11, 24]))) for _ in range(m)]
    width = rng.choice([0, rng.randint(1, 200)])
    parts = []
    for nm, r in zip(names, a):
        parts.append(b">" + nm + (b" some description" if nm and rng.random() < 0.5 else b"") + b"\n")
        r = bytes(r)
        step = width if width else max(len(r), 1)
        for i in range(0, len(r), step):
            parts.append(r[i:i + step] + b"\n")
    return b"".join(parts), names, a


def test_seeded_emit_fuzz(ctx):
    rng = random.Random(20261018)
    mrng = np.random.default_rng(20261018)
    for it in range(300):
        text, names, a = fuzz_case(rng)
        m, n = a.shape
        info = ctx.upload_fasta(text)
        assert (info.m, info.n) == (m, n)
        keep_res, keep_seq = mrng.random(n) < mrng.random(), mrng.random(m) < mrng.random()
        if it % 7 == 0:
            keep_res[:], keep_seq[:] = True, True
        for fmt in FORMATS:
            assert ctx.emit_text(fmt, keep_res, keep_seq) == host_text(names, a, keep_res, keep_seq, fmt), (it, fmt, m, n)


def test_fasta_inputs_take_the_device_writer(tmp_path, monkeypatch):
    """files -> files for FASTA inputs is the device route: the workers are asked for the text and not for the rows, and
    neither the host writer nor the host reader runs"""
    paths = small_files(tmp_path)
    paths = [p for p in paths if p.endswith(".fasta") and not p.endswith("empty.fasta")]
    want = {fmt: [t.dumps(fmt).encode() for t in trim_files(AutomaticTrimmer("gappyout"), paths)] for fmt in FORMATS}
    asked = []
    plain = _lib.Batch.trim_fasta

    def spy(self, texts, valid, params3, want_rows=False, emit=None):
        asked.append((bool(want_rows), emit))
        return plain(self, texts, valid, params3, want_rows=want_rows, emit=emit)

    def refuse(*args, **kwargs):
        raise AssertionError("the host route ran")

    monkeypatch.setattr(_lib.Batch, "trim_fasta", spy)
    monkeypatch.setattr(Alignment, "dump", refuse)
    monkeypatch.setattr(Alignment, "dumps", refuse)
    monkeypatch.setattr(Alignment, "_from_text", classmethod(refuse))
    for fmt in FORMATS:
        outs = [io.BytesIO() for _ in paths]
        trim_files(AutomaticTrimmer("gappyout"), paths, masks_only=True, output=outs, output_format=fmt)
        assert [o.getvalue() for o in outs] == want[fmt], fmt
    assert asked == [(False, fmt) for fmt in FORMATS]


def test_emit_text_after_an_attached_matrix_and_an_upload_in_flight(ctx):
    """the other ways an alignment reaches a context: a matrix already on the device (garbage in its padding), and rows whose
    copy nobody has waited for yet"""
    import torch

    rng = np.random.default_rng(41)
    a = synth_msa(70, 333, 9)
    names = [b"att%d" % i for i in range(70)]
    buf = torch.zeros((70, 384), dtype=torch.uint8, device="cuda:0")
    buf[:, :333] = torch.from_numpy(a).to("cuda:0")
    buf[:, 333:] = 0x41
    torch.cuda.synchronize()
    ctx.attach(buf.data_ptr(), 70, 333, 384, ord("X"))
    keep_res, keep_seq = masks_for("random", 70, 333, rng)
    for fmt in FORMATS:
        assert ctx.emit_text(fmt, keep_res, keep_seq, names) == host_text(names, a, keep_res, keep_seq, fmt), fmt
    big = np.ascontiguousarray(synth_msa(600, 2001, 10))  # (beyond the rows that are read in place from pinned staging)
    names = [b"row%d" % i for i in range(600)]
    ctx.upload(big, ord("X"), wait=False)
    keep_res, keep_seq = masks_for("random", 600, 2001, rng)
    assert ctx.emit_text("clustal", keep_res, keep_seq, names) == host_text(names, big, keep_res, keep_seq, "clustal")
    ctx.sync()
