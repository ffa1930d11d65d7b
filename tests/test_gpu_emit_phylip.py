"""Trimmed PHYLIP text composed on the device (msa_emit_text and msa_trim_batch_fasta_emit with the codes 16 .. 21,
trim_files(..., output=..., output_format="phylip" ...)) against the host writers (`TrimmedAlignment.dumps` / `dump`:
alignment.py's _write_phylip40, _write_phylip32, _write_phylippaml): exact byte comparisons."""
import io
import random
import warnings

import numpy as np
import pytest

from pytrimal_amd import (Alignment, AutomaticTrimmer, ManualTrimmer, OverlapTrimmer, RepresentativeTrimmer,
                          TrimmedAlignment, _lib)
from pytrimal_amd.batch import trim_files
from pytrimal_amd.synth import synth_msa
from test_emit_phylip_api import PHYLIP_FORMATS, PHYLIP_SHAPES, phylip_cases
from test_emit_text_api import masks_for
from test_gpu_fasta_device import FASTA_CASES, synth_text, wrap

pytestmark = pytest.mark.gpu

LAYOUTS = ["phylip40", "phylip32", "phylippaml"]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def host_text(names, a, keep_res, keep_seq, fmt):
    return TrimmedAlignment._from_parts(names, a, 0, keep_seq, keep_res).dumps(fmt).encode()


@pytest.mark.parametrize("m,n", PHYLIP_SHAPES)
def test_emit_text_after_a_row_upload(ctx, m, n):
    uploaded = False
    for name_kind, kind, names, a, keep_res, keep_seq in phylip_cases(m, n):
        if not uploaded:
            ctx.upload(a, ord("X"))
            uploaded = True
        for fmt in PHYLIP_FORMATS:
            want = host_text(names, a, keep_res, keep_seq, fmt)
            assert ctx.emit_text(fmt, keep_res, keep_seq, names) == want, (name_kind, kind, fmt)
            if kind == "full" and keep_seq.all():
                assert ctx.emit_text(fmt, names=names) == want == Alignment._from_parts(names, a).dumps(fmt).encode(), fmt
    with pytest.raises(_lib.MsaError):  # the rows came without a text: there are no names on the device
        ctx.emit_text("phylip32")
    with pytest.raises(ValueError):  # (the alias is `trim_files`'s to resolve)
        ctx.emit_text("phylip", names=names)
    # a kept name with a byte >= 0x80 is reported, not written; a name that is not kept does not matter
    odd = list(names)
    odd[-1] = "séq".encode("utf-8")
    for fmt in PHYLIP_FORMATS:
        assert ctx.emit_text(fmt, names=odd) is None, fmt
        if m > 1:
            keep_seq = np.ones(m, dtype=bool)
            keep_seq[-1] = False
            assert ctx.emit_text(fmt, None, keep_seq, odd) == host_text(names, a, np.ones(n, dtype=bool), keep_seq, fmt), fmt


def test_emit_text_with_the_names_of_the_text(ctx):
    rng = np.random.default_rng(19)
    texts = FASTA_CASES + [synth_text(30, 200, 3, "protein"), synth_text(7, 61, 4, "dna", width=0), synth_text(33, 121, 5, "deg", eol=b"\r\n")]
    for text in texts:
        ali = Alignment.load(io.BytesIO(text), "fasta")
        info = ctx.upload_fasta(text)
        m, n = ali._matrix.shape
        assert (info.m, info.n) == (m, n)
        for kind in ("full", "random"):
            keep_res, keep_seq = masks_for(kind, m, n, rng)
            for fmt in PHYLIP_FORMATS:
                want = host_text(ali._names, ali._matrix, keep_res, keep_seq, fmt)
                got = ctx.emit_text(fmt, keep_res, keep_seq) if kind == "random" else ctx.emit_text(fmt)
                assert got == want, (kind, fmt, text[:60])


def test_one_larger_text(ctx):
    """600 x 2001 with random masks that keep about 0.95 of the rows and of the columns: texts of 1 - 2 MB, so placement is
    exercised across thousands of workgroups' lanes and the last partial 16-byte vector"""
    rng = np.random.default_rng(43)
    big = np.ascontiguousarray(synth_msa(600, 2001, 10))
    names = [b"row%d" % i + b"_" * (i % 17) for i in range(600)]
    ctx.upload(big, ord("X"))
    keep_res, keep_seq = rng.random(2001) < 0.95, rng.random(600) < 0.95
    assert not keep_res.all() and not keep_seq.all()
    sizes = []
    for fmt in LAYOUTS:
        want = host_text(names, big, keep_res, keep_seq, fmt)
        assert ctx.emit_text(fmt, keep_res, keep_seq, names) == want, fmt
        sizes.append(len(want))
    assert all(1_000_000 < s < 2_000_000 for s in sizes) and any(s % 16 for s in sizes), sizes


def fuzz_case(rng):
    m, n = rng.randint(1, 40), rng.randint(0, 400)
    alpha = np.frombuffer(rng.choice([b"ACGT-", b"ACGU-N", b"ACDEFGHIKLMNPQRSTVWY-", b"ACGTRYKMN-"]), dtype=np.uint8)
    a = alpha[np.random.default_rng(rng.getrandbits(32)).integers(0, len(alpha), size=(m, n))]
    names = [bytes(rng.choice(b"abcXYZ019_|.") for _ in range(rng.choice([0, 1, 3, 9, 10, 11, 24]))) for _ in range(m)]
    width = rng.choice([0, 60, rng.randint(1, 200)])
    parts = []
    for nm, r in zip(names, a):  # (a description behind a name only: behind an empty one it would be read as the name)
        parts.append(b">" + nm + (b"\tsome description" if nm and rng.random() < 0.5 else b"") + b"\n")
        r = bytes(r)
        step = width if width else max(len(r), 1)
        for i in range(0, len(r), step):
            parts.append(r[i:i + step] + b"\n")
    return b"".join(parts), names, a


def test_seeded_emit_fuzz(ctx):
    rng = random.Random(20261019)
    mrng = np.random.default_rng(20261019)
    for it in range(60):
        text, names, a = fuzz_case(rng)
        m, n = a.shape
        info = ctx.upload_fasta(text)
        assert (info.m, info.n) == (m, n)
        keep_res, keep_seq = mrng.random(n) < mrng.random(), mrng.random(m) < mrng.random()
        if it % 7 == 0:
            keep_res[:], keep_seq[:] = True, True
        for fmt in PHYLIP_FORMATS:
            assert ctx.emit_text(fmt, keep_res, keep_seq) == host_text(names, a, keep_res, keep_seq, fmt), (it, fmt, m, n)


def fasta_files(tmp_path):
    paths = []
    for k, (m, n, kind) in enumerate([(30, 120, "protein"), (25, 200, "dna"), (12, 90, "deg"), (40, 301, "protein")]):
        p = tmp_path / f"p{k}.fasta"
        p.write_bytes(synth_text(m, n, 200 + k, kind))
        paths.append(str(p))
    return paths


def odd_name_text(odd):
    """five sequences with residues in columns 0 .. 29, a sixth -- the one with the non-ASCII name -- in columns 30 .. 39 only:
    a gap threshold of 0.8 removes the last ten columns, and with them the sixth sequence, which is left with gaps only"""
    rng = np.random.default_rng(29)
    a = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[rng.integers(0, 20, size=(6, 40))].copy()
    a[:5, 30:] = ord("-")
    a[5, :30] = ord("-")
    return wrap([b"g%d" % i for i in range(5)] + [odd], a)


def mixed_files(tmp_path):
    """FASTA inputs (the device parses and writes them), a Clustal input (host reader, host writer) and a FASTA input with a
    non-ASCII name (parsed on the device; with that name kept the host writer's, see the test)"""
    paths = fasta_files(tmp_path)
    clw = tmp_path / "p.clw"
    clw.write_bytes(Alignment.load(paths[0]).dumps("clustal").encode())
    paths.insert(1, str(clw))
    odd = tmp_path / "odd.fasta"
    odd.write_bytes(odd_name_text("séq".encode("utf-8")))
    paths.append(str(odd))
    return paths


def quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return fn()


@pytest.mark.parametrize("masks_only", [True, False])
def test_files_to_files_on_a_mixed_call(tmp_path, masks_only):
    paths = mixed_files(tmp_path)
    make = lambda: ManualTrimmer(gap_threshold=0.8)  # noqa: E731
    objects = quiet(lambda: trim_files(make(), paths))
    assert len(objects[-1].names) == 5 and any(not all(t.residues_mask) for t in objects)
    for fmt in ("phylip", "phylip32", "phylippaml_m10", "PHYLIP40"):
        outs = [io.BytesIO() if k % 2 else str(tmp_path / f"{fmt}_{k}.out") for k in range(len(paths))]
        got = quiet(lambda: trim_files(make(), paths, masks_only=masks_only, output=outs, output_format=fmt))
        assert len(got) == len(paths)
        for k, (o, t) in enumerate(zip(outs, objects)):
            want = io.BytesIO()
            t.dump(want, fmt)
            written = o.getvalue() if isinstance(o, io.BytesIO) else open(o, "rb").read()
            assert written == want.getvalue() and written.startswith(b" %d " % len(t.names)), (fmt, k)
            mask = got[k] if masks_only else (np.array(got[k].residues_mask), np.array(got[k].sequences_mask))
            assert np.array_equal(mask[0], t.residues_mask) and np.array_equal(mask[1], t.sequences_mask)
    # (above, the sequence with the non-ASCII name is trimmed away, so that file too is written by the device.  A text the
    # host writer writes for a kept non-ASCII name does not exist: `dump` encodes ASCII and refuses it.  What can be checked of
    # that route is that the flag sends the file to the host writer and the call raises the writer's own refusal:)
    kept = trim_files(AutomaticTrimmer("noallgaps"), [paths[-1]])[0]
    assert len(kept.names) == 6
    with pytest.raises(UnicodeError) as want:
        kept.dump(io.BytesIO(), "phylip")
    buf = io.BytesIO()
    with pytest.raises(type(want.value)):
        trim_files(AutomaticTrimmer("noallgaps"), paths, masks_only=masks_only, output=[buf] * len(paths), output_format="phylip")


def test_fasta_inputs_take_the_device_writer(tmp_path, monkeypatch):
    """files -> files in PHYLIP for FASTA inputs is the device route: the workers are asked for the text (under the name the
    alias stands for) and not for the rows, and neither the host writer nor the host reader runs"""
    paths = fasta_files(tmp_path)
    want = [t.dumps("phylip").encode() for t in trim_files(AutomaticTrimmer("gappyout"), paths)]
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
    outs = [io.BytesIO() for _ in paths]
    trim_files(AutomaticTrimmer("gappyout"), paths, masks_only=True, output=outs, output_format="phylip")
    assert asked == [(False, "phylip40")]
    assert [o.getvalue() for o in outs] == want


def drop_text():
    """14 x 150 with a sequence every kind of trimmer here removes for a reason of its own: row 3 is row 2 with a few residues
    changed (one of the two is no representative), row 5 holds residues where the others hold gaps and little else (no overlap)"""
    rng = np.random.default_rng(31)
    a = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", dtype=np.uint8)[rng.integers(0, 20, size=(14, 150))].copy()
    a[:, 120:] = ord("-")
    a[rng.random((14, 150)) < 0.1] = ord("-")
    a[3] = a[2]
    a[3, 10:15] = ord("W")
    a[5, :120] = ord("-")
    a[5, 120:] = ord("K")
    return wrap([b"d%d" % i + b"_" * i for i in range(14)], a)


TRIMMER_KINDS = [
    ("gappyout", lambda: AutomaticTrimmer("gappyout")),
    ("overlap", lambda: OverlapTrimmer(40, 0.5)),
    ("representative", lambda: RepresentativeTrimmer(identity_threshold=0.5)),
]


@pytest.mark.parametrize("kind,make", TRIMMER_KINDS, ids=[k for k, _ in TRIMMER_KINDS])
def test_trimmer_kinds_reach_the_writer(tmp_path, kind, make):
    paths = fasta_files(tmp_path)
    (tmp_path / "drop.fasta").write_bytes(drop_text())
    paths.append(str(tmp_path / "drop.fasta"))
    objects = quiet(lambda: trim_files(make(), paths))
    assert len(objects[-1].names) < 14  # (a sequence mask that drops rows reaches the writer)
    outs = [io.BytesIO() for _ in paths]
    quiet(lambda: trim_files(make(), paths, masks_only=True, output=outs, output_format="phylip32"))
    assert [o.getvalue() for o in outs] == [t.dumps("phylip32").encode() for t in objects]
