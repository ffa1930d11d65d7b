"""The device writer's host side (msa_text_size, the argument checks of the new entry points, trim_files(..., output=...)):
what can be checked without a device.  tests/test_gpu_emit_text.py compares the composed bytes on the GPU."""
import ctypes
import io

import numpy as np
import pytest

from pytrimal_amd import Alignment, AutomaticTrimmer, TrimmedAlignment, _lib
from pytrimal_amd.batch import trim_files
from pytrimal_amd.synth import synth_msa

# the shapes of tests/test_api.py::test_whole_matrix_writers_equal_the_line_by_line_ones
SHAPES = [(1, 1), (1, 59), (1, 60), (1, 61), (3, 120), (5, 121), (7, 0), (9, 179), (20, 600), (4, 5)]
FORMATS = ["fasta", "fasta_m10", "clustal"]
MASK_KINDS = ["full", "random", "no_column", "no_sequence"]


def names_for(m, rng):
    """names of different lengths: an empty one and one longer than 10 bytes among them (where m allows)"""
    names = [("seq%d" % i + "x" * int(rng.integers(0, 14))).encode() for i in range(m)]
    names[0] = b"a_name_longer_than_ten_bytes"
    if m > 1:
        names[1] = b""
    return names


def masks_for(kind, m, n, rng):
    keep_seq, keep_res = np.ones(m, dtype=bool), np.ones(n, dtype=bool)
    if kind == "random":
        keep_seq, keep_res = rng.random(m) < 0.7, rng.random(n) < 0.6
    elif kind == "no_column":
        keep_res[:] = False
    elif kind == "no_sequence":
        keep_seq[:] = False
    return keep_res, keep_seq


@pytest.mark.parametrize("m,n", SHAPES)
def test_text_size_is_the_length_of_dumps(m, n):
    rng = np.random.default_rng(m * 1000 + n)
    a = synth_msa(m, max(n, 1), 5)[:, :n]
    names = names_for(m, rng)
    for kind in MASK_KINDS:
        keep_res, keep_seq = masks_for(kind, m, n, rng)
        t = TrimmedAlignment._from_parts(names, a, 0, keep_seq, keep_res)
        lens = [len(x) for x, k in zip(names, keep_seq) if k]
        for fmt in FORMATS:
            assert _lib.text_size(fmt, lens, int(keep_res.sum())) == len(t.dumps(fmt).encode()), (kind, fmt)


def test_text_size_arguments():
    lib = _lib.load()
    out = ctypes.c_int64(-5)
    lens = np.array([3, 4], dtype=np.int32)
    assert lib.msa_text_size(0, 2, 10, _lib.ptr(lens), ctypes.byref(out)) == _lib.OK and out.value == 2 * 2 + 7 + 2 * 11
    for fmt in (-1, 3, 99):
        assert lib.msa_text_size(fmt, 2, 10, _lib.ptr(lens), ctypes.byref(out)) == _lib.E_INVALID
    assert lib.msa_text_size(0, 2, 10, _lib.ptr(lens), None) == _lib.E_INVALID
    assert lib.msa_text_size(0, 2, 10, None, ctypes.byref(out)) == _lib.E_INVALID
    assert lib.msa_text_size(0, -1, 10, None, ctypes.byref(out)) == _lib.E_INVALID
    assert lib.msa_text_size(0, 2, -1, _lib.ptr(lens), ctypes.byref(out)) == _lib.E_INVALID
    assert lib.msa_text_size(0, 2, 10, _lib.ptr(np.array([3, -1], dtype=np.int32)), ctypes.byref(out)) == _lib.E_INVALID
    # nothing kept: the empty text, Clustal's header alone
    assert _lib.text_size("fasta", [], 7) == 0 and _lib.text_size("clustal", [], 7) == 37 and _lib.text_size("CLUSTAL", [5], 0) == 37
    with pytest.raises(ValueError):
        _lib.text_size("phylip", [1], 1)
    with pytest.raises(ValueError):
        _lib.text_format_code("nope")
    # a text beyond 2^31 bytes has a length too (what refuses it is msa_emit_text)
    assert _lib.text_size("fasta", [8] * 3000, 1_000_000) == 3000 * (10 + 1_000_000 + 16667)


def test_new_entry_points_refuse_null_handles():
    lib = _lib.load()
    size, flags = ctypes.c_int64(0), ctypes.c_uint32(0)
    buf = np.zeros(16, dtype=np.uint8)
    for fmt in (0, 1, 2, 7):
        assert lib.msa_emit_text(None, fmt, None, None, None, None, None, ctypes.byref(size), ctypes.byref(flags)) == _lib.E_INVALID
    assert lib.msa_download_text(None, _lib.ptr(buf), 16) == _lib.E_INVALID
    rcs = np.zeros(1, dtype=np.int32)
    params3 = (_lib.TrimParams * 3)()
    addr, lens = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int64)
    for fmt in (0, 2, 9):
        assert lib.msa_trim_batch_fasta_emit(None, 1, _lib.ptr(addr), _lib.ptr(lens), None, params3, 0, fmt, _lib.ptr(rcs)) == _lib.E_INVALID
    text = ctypes.c_void_p()
    assert lib.msa_batch_fasta_text(None, 0, ctypes.byref(text), ctypes.byref(size), ctypes.byref(flags)) == _lib.E_INVALID


def test_trim_files_output_checks_come_before_any_work(tmp_path):
    src = tmp_path / "in.fasta"
    src.write_bytes(b">a\nACDE-\n>b\nAC-EF\n")
    dst = tmp_path / "out.fasta"
    trimmer = AutomaticTrimmer("strict", platform=None)
    with pytest.raises(ValueError, match="2 entries for 1 files"):
        trim_files(trimmer, [str(src)], output=[str(dst), io.BytesIO()])
    with pytest.raises(ValueError, match="2 entries for 1 files"):  # (before the format, before any file is read)
        trim_files(trimmer, [str(tmp_path / "missing.fasta")], output=[str(dst), str(dst)], output_format="nope")
    with pytest.raises(ValueError) as err:
        trim_files(trimmer, [str(src)], output=[str(dst)], output_format="nope")
    with pytest.raises(ValueError) as want:
        Alignment.load(str(src)).dumps("nope")
    assert str(err.value) == str(want.value) == "Could not recognize alignment format: 'nope'"
    with pytest.raises(ValueError, match="Could not recognize alignment format: 'clustal_m10'"):
        trim_files(trimmer, [str(src)], output=[str(dst)], output_format="clustal_m10")
    assert not dst.exists()
    # no device: what the call raises without `output`, and no output file
    buf = io.BytesIO()
    for masks_only in (False, True):
        with pytest.raises(RuntimeError, match="MI355X only"):
            trim_files(trimmer, [str(src), str(src)], masks_only=masks_only, output=[str(dst), buf], output_format="clustal")
    assert not dst.exists() and buf.getvalue() == b""
    with pytest.raises(RuntimeError, match="MI355X only"):  # (unchanged without the keyword)
        trim_files(trimmer, [str(src)])
