"""trim_files and the device FASTA entry points without a device: argument checks, the loud failure, null contexts."""
import ctypes
import io
import os

import pytest

from pytrimal_amd import AutomaticTrimmer, _lib
from pytrimal_amd.batch import trim_files


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def trimmer():
    return AutomaticTrimmer("strict", platform="detect")


def test_trim_files_checks_its_files_as_load_does(tmp_path):
    with pytest.raises(ValueError, match="Format must be specified"):
        trim_files(trimmer(), [io.BytesIO(b">a\nAC\n")])
    path = tmp_path / "a.fasta"
    path.write_bytes(b">a\nAC\n>b\nAG\n")
    with pytest.raises(ValueError, match="Unknown alignment format: 'nope'"):
        trim_files(trimmer(), [str(path)], format="nope")
    with pytest.raises(IsADirectoryError):
        trim_files(trimmer(), [str(tmp_path)])
    with pytest.raises(TypeError, match="must not be None"):
        trim_files(trimmer(), [None])
    with pytest.raises(TypeError, match="not open in binary mode"):
        trim_files(trimmer(), [io.StringIO(">a\nAC\n")], format="fasta")


def test_trim_files_without_a_device_fails_as_trim_does(tmp_path, lib):
    if lib.msa_device_count() > 0:
        pytest.skip("a GPU is visible")
    path = tmp_path / "a.fasta"
    path.write_bytes(b">a\nAC-G\n>b\nAGTG\n")
    with pytest.raises(RuntimeError, match="MI355X only"):
        trim_files(trimmer(), [str(path)])
    with pytest.raises(RuntimeError, match="MI355X only"):
        trim_files(trimmer(), [str(path)], masks_only=True)


def test_new_entry_points_refuse_a_null_context(lib):
    text = b">a\nAC\n"
    info, det = _lib.TextInfo(), _lib.ErrDetail()
    assert lib.msa_upload_fasta(None, text, len(text), None, ctypes.byref(info), ctypes.byref(det)) == _lib.E_INVALID
    off, ln = (ctypes.c_int64 * 1)(), (ctypes.c_int32 * 1)()
    assert lib.msa_text_names(None, off, ln) == _lib.E_INVALID
    rows = (ctypes.c_uint8 * 8)()
    assert lib.msa_download_rows(None, rows, 8) == _lib.E_INVALID
    params = (_lib.TrimParams * 3)()
    lens = (ctypes.c_int64 * 1)(len(text))
    texts = (ctypes.c_char_p * 1)(text)
    rc = (ctypes.c_int32 * 1)()
    assert lib.msa_trim_batch_fasta(None, 1, texts, lens, None, params, 0, rc) == _lib.E_INVALID
    assert lib.msa_batch_fasta_result(None, 0, None, None, None, None, None, None, None, None) == _lib.E_INVALID


def test_upload_path_name_is_known():
    assert _lib.Context.PATH_NAMES["upload"][7] == "fasta"


def _fifo_with(path, text):
    """A FIFO at `path` and a thread that writes `text` into it once."""
    import threading

    os.mkfifo(path)

    def feed():
        with open(path, "wb") as f:
            f.write(text)

    t = threading.Thread(target=feed, daemon=True)
    t.start()
    return t


def test_mapped_read_of_a_pipe_reads_it(tmp_path):
    from pytrimal_amd.alignment import _read_input

    text = b">a\nAC-G\n>b\nAGTG\n"
    fifo = tmp_path / "in.fasta"
    feeder = _fifo_with(str(fifo), text)
    assert bytes(_read_input(str(fifo), None, mapped=True)) == text  # (a FIFO reports size 0: read, not mapped)
    feeder.join(5)
    plain = tmp_path / "plain.fasta"
    plain.write_bytes(text)
    mapped = _read_input(str(plain), None, mapped=True)
    assert not isinstance(mapped, bytes) and bytes(mapped) == text
    empty = tmp_path / "empty.fasta"
    empty.write_bytes(b"")
    assert _read_input(str(empty), None, mapped=True) == b""
