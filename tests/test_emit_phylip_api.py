"""The PHYLIP family in the device writer's host side (msa_text_size with the codes 16 .. 21, the names in `_lib.TEXT_FORMATS`,
the alias `phylip` in `trim_files`): what can be checked without a device.  tests/test_gpu_emit_phylip.py compares the composed
bytes on the GPU.  Every expected length comes from the host writers (`TrimmedAlignment.dumps`)."""
import ctypes
import io

import numpy as np
import pytest

from pytrimal_amd import AutomaticTrimmer, TrimmedAlignment, _lib
from pytrimal_amd.batch import _check_output, trim_files
from pytrimal_amd.synth import synth_msa
from test_emit_text_api import MASK_KINDS, SHAPES, masks_for, names_for

# line ends of the groups of ten (9, 10, 11) and of the blocks of 60 (119, 121) beside the shapes of the FASTA / Clustal tests
PHYLIP_SHAPES = SHAPES + [(3, 9), (3, 10), (3, 11), (2, 119), (2, 121)]
PHYLIP_FORMATS = ["phylip40", "phylip40_m10", "phylip32", "phylip32_m10", "phylippaml", "phylippaml_m10"]
PHYLIP_CODES = dict(zip(PHYLIP_FORMATS, range(16, 22)))
NAME_SETS = ["mixed", "short", "longest_dropped"]


def names_of(kind, m, rng):
    """mixed: test_emit_text_api's names (an empty one, one longer than 10 bytes); short: no name longer than 10 bytes, so the
    name column has its least width of 13; longest_dropped: the last name is the longest one -- `drop_longest` takes it away"""
    if kind == "mixed":
        return names_for(m, rng)
    if kind == "short":
        return [(b"q%d" % i + b"y" * int(rng.integers(0, 8)))[:10] for i in range(m)]
    names = [b"n%d" % i + b"z" * int(rng.integers(0, 12)) for i in range(m)]
    names[-1] = b"the_longest_name_of_them_all_is_not_kept"
    return names


def drop_longest(kind, keep_seq):
    if kind == "longest_dropped" and keep_seq.size > 1:
        keep_seq[-1] = False
    return keep_seq


def phylip_cases(m, n):
    """(name set, mask kind, names, matrix, keep_res, keep_seq) for one shape"""
    rng = np.random.default_rng(m * 1000 + n)
    a = np.ascontiguousarray(synth_msa(m, max(n, 1), 5)[:, :n])
    for name_kind in NAME_SETS:
        names = names_of(name_kind, m, rng)
        for kind in MASK_KINDS:
            keep_res, keep_seq = masks_for(kind, m, n, rng)
            yield name_kind, kind, names, a, keep_res, drop_longest(name_kind, keep_seq)


def test_the_table_holds_the_six_names_and_not_the_alias():
    assert {k: _lib.TEXT_FORMATS[k] for k in PHYLIP_FORMATS} == PHYLIP_CODES
    assert [_lib.text_format_code(k.upper()) for k in PHYLIP_FORMATS] == list(range(16, 22))
    for alias in ("phylip", "phylip_m10", "PHYLIP"):
        assert alias not in _lib.TEXT_FORMATS
        with pytest.raises(ValueError):
            _lib.text_format_code(alias)
        with pytest.raises(ValueError):
            _lib.text_size(alias, [1], 1)


@pytest.mark.parametrize("m,n", PHYLIP_SHAPES)
def test_text_size_is_the_length_of_dumps(m, n):
    for name_kind, kind, names, a, keep_res, keep_seq in phylip_cases(m, n):
        t = TrimmedAlignment._from_parts(names, a, 0, keep_seq, keep_res)
        lens = [len(x) for x, k in zip(names, keep_seq) if k]
        for fmt in PHYLIP_FORMATS:
            assert _lib.text_size(fmt, lens, int(keep_res.sum())) == len(t.dumps(fmt).encode()), (name_kind, kind, fmt)


def test_text_size_codes():
    lib = _lib.load()
    out = ctypes.c_int64(-5)
    lens = np.array([3, 14], dtype=np.int32)
    for code in range(16, 22):
        assert lib.msa_text_size(code, 2, 10, _lib.ptr(lens), ctypes.byref(out)) == _lib.OK and out.value > 0
    for code in (3, 15, 22, 99):
        assert lib.msa_text_size(code, 2, 10, _lib.ptr(lens), ctypes.byref(out)) == _lib.E_INVALID
    assert lib.msa_text_size(16, 2, 10, None, ctypes.byref(out)) == _lib.E_INVALID
    assert lib.msa_text_size(18, 2, -1, _lib.ptr(lens), ctypes.byref(out)) == _lib.E_INVALID
    # " 2 10\n" and two lines of a name column of 14 + 3 (10 + 3 with the cut), ten residues, a line end
    assert _lib.text_size("phylippaml", lens, 10) == 6 + 2 * (17 + 10 + 1)
    assert _lib.text_size("phylippaml_m10", lens, 10) == 6 + 2 * (13 + 10 + 1)
    assert _lib.text_size("phylip40", lens, 10) == 6 + 2 * (17 + 10 + 1) + 1
    assert _lib.text_size("phylip32", lens, 10) == 6 + 2 * (17 + 10 + 1 + 1)
    # nothing kept: the header with two zeros (and the interleaved layout's one block end), whatever the column count
    assert _lib.text_size("phylip40", [], 7) == len(b" 0 0\n\n")
    assert _lib.text_size("phylip32", [], 7) == _lib.text_size("phylippaml_m10", [], 7) == len(b" 0 0\n")
    # a text beyond 2^31 bytes has a length too (what refuses it is msa_emit_text)
    assert _lib.text_size("phylippaml", [8] * 3000, 1_000_000) == len(b" 3000 1000000\n") + 3000 * (13 + 1_000_000 + 1)


def test_new_entry_points_refuse_null_handles_with_the_new_codes():
    lib = _lib.load()
    size, flags = ctypes.c_int64(0), ctypes.c_uint32(0)
    rcs = np.zeros(1, dtype=np.int32)
    params3 = (_lib.TrimParams * 3)()
    addr, lens = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int64)
    for code in (15, 16, 21, 22):
        assert lib.msa_emit_text(None, code, None, None, None, None, None, ctypes.byref(size), ctypes.byref(flags)) == _lib.E_INVALID
        assert lib.msa_trim_batch_fasta_emit(None, 1, _lib.ptr(addr), _lib.ptr(lens), None, params3, 0, code, _lib.ptr(rcs)) == _lib.E_INVALID


def test_trim_files_resolves_the_alias_for_the_device_writer():
    """what `trim_files` asks the workers for: `dumps`' alias becomes the name in the table, the host-only formats none"""
    asks = {"phylip": "phylip40", "PHYLIP": "phylip40", "phylip_m10": "phylip40_m10", "Phylip40": "phylip40", "phylip32": "phylip32",
            "phylip32_m10": "phylip32_m10", "phylippaml": "phylippaml", "PHYLIPPAML_M10": "phylippaml_m10", "fasta": "fasta",
            "clustal": "clustal", "nexus": None, "nexus_m10": None, "mega": None, "pir": None, "nbrf": None, "html": None}
    for fmt, emit in asks.items():
        assert _check_output([io.BytesIO()], fmt, 1)[1] == emit, fmt
    with pytest.raises(ValueError, match="Could not recognize alignment format: 'phylip41'"):
        _check_output([io.BytesIO()], "phylip41", 1)


def test_trim_files_without_a_device_still_raises_and_writes_nothing(tmp_path):
    src = tmp_path / "in.fasta"
    src.write_bytes(b">a\nACDE-\n>b\nAC-EF\n")
    dst = tmp_path / "out.phy"
    buf = io.BytesIO()
    trimmer = AutomaticTrimmer("strict", platform=None)
    for masks_only in (False, True):
        with pytest.raises(RuntimeError, match="MI355X only"):
            trim_files(trimmer, [str(src), str(src)], masks_only=masks_only, output=[str(dst), buf], output_format="phylip")
    assert not dst.exists() and buf.getvalue() == b""
