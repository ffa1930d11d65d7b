"""Batches of independent alignments across the GPUs of a node.

Alignments are independent units (the reference treats them so: one local `trimAlManager` per
`trim` call, ``/root/reference/src/pytrimal/_trimal.pyx:1314-1316``, and a thread pool over
alignments in ``README.md:136-152``), so the path shards at alignment granularity: one process per
GPU, static round-robin of the alignments over the ranks, no collective inside an alignment.
The only communication is control-plane sized: an optional broadcast of the trimmer from rank 0
and a gather of the kept-column / kept-sequence masks to rank 0 (`torch.distributed`, backend
"nccl" = RCCL on ROCm for device tensors, "gloo" for the CPU tests).

Import order matters in a process that uses PyTorch-ROCm: this module imports torch before the
HIP library is loaded (see pytrimal_amd._lib).
"""
import atexit
import os
import threading

import numpy as np
import torch
import torch.distributed as dist

from . import _lib  # (the module alone: the HIP library is loaded on first use)
from .trimmer import BaseTrimmer, _raise_warnings, computes_gap_stats, type_index
from .alignment import (_M10_FORMATS, _VALID, _WRITERS, Alignment, TrimmedAlignment, _read_input, _sniff_format, _sniff_mapped,
                        _write_bytes)
from .matrix import SimilarityMatrix

# One native batch object (worker threads + their device contexts: O(m^2) buffers each) per (device, workers), kept
# between calls, closed at exit, rebuilt in a child process (worker threads do not survive a fork).
_BATCHES = {}
_BATCHES_PID = None
_BATCHES_LOCK = threading.Lock()


def _close_batches():
    for b in list(_BATCHES.values()):
        try:
            b.close()
        except Exception:
            pass
    _BATCHES.clear()


atexit.register(_close_batches)


def close_batches():
    """Close this process's native batch objects (worker threads, device contexts and arenas); the next `trim_batch` creates
    new ones, which read the MSA_BATCH_* / MSA_* diagnostic switches again."""
    with _BATCHES_LOCK:
        _close_batches()


def _native_batch(device_index, workers):
    global _BATCHES_PID
    with _BATCHES_LOCK:
        if _BATCHES_PID != os.getpid():
            _BATCHES.clear()  # (inherited across a fork: the threads are gone and the handles belong to the parent)
            _BATCHES_PID = os.getpid()
        key = (device_index, workers)
        b = _BATCHES.get(key)
        if b is None:
            for other in [k for k in _BATCHES if k[0] == device_index]:  # one set of contexts per device
                _BATCHES.pop(other).close()
            b = _BATCHES[key] = _lib.Batch(device_index, workers)
        return b


def _device_index(device):
    return device.index if isinstance(device, torch.device) and device.index is not None else _lib.default_device()


def _on_native_batch(index, threads, call):
    """`call(batch)` on device `index`'s native batch object of `threads` workers -> (batch, what it returned); again when
    another thread (asking for another worker count) replaced and closed the object in between."""
    for attempt in range(3):
        batch = _native_batch(index, max(1, min(int(threads), 64)))
        try:
            return batch, call(batch)
        except _lib.BatchClosed:
            if attempt == 2:
                raise


def _trim_rows(trimmer, alignments, matrix, device, threads):
    """The row path: `_prepare` every alignment, one `Batch.trim` over those that are not empty -> (what `_prepare` gave, per
    alignment `Batch.trim`'s tuple or None, the batch object, the call's packed masks when every alignment took part in it)."""
    prepared = [trimmer._prepare(a, matrix) for a in alignments]
    _mark("prepare")
    todo = [k for k, p in enumerate(prepared) if p[1].shape[0] and p[1].shape[1]]
    outs, batch, packed = [None] * len(prepared), None, None
    if todo:
        items = [prepared[k][1:4] for k in todo]
        batch, got = _on_native_batch(_device_index(device), threads, lambda b: b.trim(items))
        for k, out in zip(todo, got):
            outs[k] = out
        if len(todo) == len(prepared):  # (no empty alignment in between: the library's mask vector IS the gather's payload)
            packed = getattr(got, "packed", None)
    return prepared, outs, batch, packed


def _result(trimmer, names, dense, datatype, res, seq, info, rows, params, masks_only):
    """The tail of a trim: (residues mask, sequences mask, `TrimmedAlignment`) -- with `masks_only` the warnings are raised and
    the third is None.  `res` None: an empty alignment, which never reaches the device and keeps everything."""
    if res is None:
        res, seq, info, rows = np.ones(dense.shape[1], dtype=bool), np.ones(dense.shape[0], dtype=bool), None, None
    if not masks_only:
        return res, seq, trimmer._finish(names, dense, datatype, res, seq, info, rows, None, params)
    if info is not None and info.warnings:
        _raise_warnings(info, names, rows)
    return res, seq, None


def shard_indices(n_items, world_size, rank):
    """Static round-robin: item i belongs to rank i % world_size."""
    return list(range(rank, n_items, world_size))


def broadcast_trimmer(trimmer, src=0, group=None):
    """Make every rank use rank `src`'s trimmer (pickle state, a few hundred bytes)."""
    if not (dist.is_available() and dist.is_initialized()):
        return trimmer
    box = [trimmer if dist.get_rank(group) == src else None]
    dist.broadcast_object_list(box, src=src, group=group)
    return box[0]


def trim_batch(trimmer, alignments, matrix=None, *, group=None, device=None, trim_fn=None, threads=6, shard=True,
               masks_only=False, force_collectives=False):
    """Trim `alignments` (the same list on every rank) with `trimmer`, sharded over the ranks of
    `group`.  Returns the list of `TrimmedAlignment` on rank 0 and `None` elsewhere; without an
    initialised process group it simply trims everything locally.

    Within a rank the shard goes to the native batch path (`msa_trim_batch`, include/msastat.h): `threads` worker
    threads inside the library, each with its own device context, take the alignments largest first; uploads, kernels
    and host selection logic of different alignments overlap on the GPU and the interpreter lock is released for
    the whole shard (one 1000 x 4000 alignment does not fill the chip, and the host side of a trim is serial).

    `trim_fn(alignment) -> TrimmedAlignment` replaces the device path (used by the CPU tests,
    which have no device): the shard is then trimmed one alignment after the other in the calling thread.
    `shard=False`: ignore the process group and trim the whole list on this rank (returns the list).
    `masks_only=True`: return `(residues_mask, sequences_mask)` pairs of bool arrays instead of `TrimmedAlignment`
    objects -- what the gather moves; building 64 result objects is interpreter time behind the device's work (and, on
    rank 0 of a sharded run, serial work for every other rank's alignments).
    `force_collectives=True`: run the gather of the masks even in a process group of ONE rank (where it moves nothing): the
    collective path of a multi-GPU run -- device buffer, `dist.gather` over RCCL, unpacking -- on a one-GPU box
    (tests/measure/rccl_one_rank.py, `bench.py` under a launcher).
    """
    _mark("start")
    distributed = shard and dist.is_available() and dist.is_initialized()
    world = dist.get_world_size(group) if distributed else 1
    rank = dist.get_rank(group) if distributed else 0
    mine = shard_indices(len(alignments), world, rank)

    if trim_fn is not None:
        local = []
        for i in mine:
            t = trim_fn(alignments[i])
            res, seq = getattr(t, "_res_mask", None), getattr(t, "_seq_mask", None)
            if res is None or seq is None:
                res, seq = t.residues_mask, t.sequences_mask
            local.append((np.asarray(res, dtype=bool), np.asarray(seq, dtype=bool), t))
    else:
        prepared, outs, batch, packed_masks = _trim_rows(trimmer, [alignments[i] for i in mine], matrix, device, threads)
        for out in outs:
            if out is not None and out[3] != _lib.OK:
                batch.check(out[3], out[2])
        local = []
        for i, (names, dense, _, params, _keep), out in zip(mine, prepared, outs):
            res, seq, info, _, rows = out or (None,) * 5
            local.append(_result(trimmer, names, dense, alignments[i]._datatype, res, seq, info, rows, params, masks_only))
    _mark("native batch")
    collect = distributed and (world > 1 or force_collectives)
    if masks_only and not collect:
        return [(np.asarray(r, dtype=bool), np.asarray(s, dtype=bool)) for r, s, _ in local]
    if not collect:
        # (what the workers produced, as it is: rebuilding 64 results from their masks in the calling thread was a serial
        # tail of ~4 ms behind a 35 ms batch)
        return [t if isinstance(t, TrimmedAlignment) else _rebuild(alignments[i], r, s, trimmer) for i, (r, s, t) in zip(mine, local)]
    mine_trimmed = {i: t for i, (_, _, t) in zip(mine, local)}

    # every rank knows every shape, so shard payload sizes are known without a size exchange
    sizes = [(len(a.residues), len(a.sequences)) for a in alignments]
    width = max(max((sum(n + m for n, m in sizes[r::world]) for r in range(world)), default=0), 1)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    box = _gather_buffers(device, world, rank, width)
    # the shard's masks packed straight into the (page-locked) staging vector, one copy to the device, ONE gather into one
    # [world][width] tensor, one copy back for all ranks (round 5: a fresh device tensor, a pageable copy, a tensor and a
    # `.cpu()` per rank -- 64 x 5 KB, so every one of these is latency: profiles/r06_c5_collective.jsonl)
    stage = box.stage_np
    if trim_fn is None and packed_masks is not None and packed_masks.size <= stage.size:
        stage[:packed_masks.size] = packed_masks
    else:
        pos = 0
        for r, s, _ in local:
            stage[pos:pos + len(r)] = r
            pos += len(r)
            stage[pos:pos + len(s)] = s
            pos += len(s)
    if box.send is not box.stage:
        box.send.copy_(box.stage, non_blocking=True)
    _mark("pack + H2D")
    dist.gather(box.send, box.recv_list, dst=0, group=group)
    _mark("gather")
    if rank != 0:
        return None
    if box.recv_host is not box.recv:
        box.recv_host.copy_(box.recv, non_blocking=True)
        torch.cuda.current_stream(device).synchronize()
    flat_all = box.recv_host.numpy().view(np.bool_).copy()  # (the buffers are reused by the next call: one copy for all ranks)
    out = [None] * len(alignments)
    for r in range(world):
        flat = flat_all[r]
        pos = 0
        for i in range(r, len(alignments), world):
            n, m = sizes[i]
            res = flat[pos:pos + n]
            seq = flat[pos + n:pos + n + m]
            pos += n + m
            if masks_only:
                out[i] = (res, seq)
                continue
            t = mine_trimmed.get(i) if r == rank else None
            out[i] = t if isinstance(t, TrimmedAlignment) else _rebuild(alignments[i], res, seq, trimmer)
    _mark("D2H + unpack")
    return out


# ---- the gather's buffers, kept between calls: one per (device, group size, rank, width) ----------------------------------
class _GatherBuffers:
    def __init__(self, device, world, rank, width):
        cuda = device.type == "cuda"
        self.stage = torch.zeros(width, dtype=torch.uint8, pin_memory=cuda)   # host side of the send buffer
        self.stage_np = self.stage.numpy()
        self.send = torch.zeros(width, dtype=torch.uint8, device=device) if cuda else self.stage
        self.recv = self.recv_host = self.recv_list = None
        if rank == 0:
            self.recv = torch.zeros((world, width), dtype=torch.uint8, device=device)
            self.recv_list = list(self.recv.unbind(0))
            self.recv_host = torch.zeros((world, width), dtype=torch.uint8, pin_memory=True) if cuda else self.recv


_GATHER = {}


def _gather_buffers(device, world, rank, width):
    # (the gather needs equally long tensors on every rank: every rank sizes its buffers by the same rule -- exactly `width`)
    key = (str(device), world, rank, width)
    box = _GATHER.get(key)
    if box is None:
        if len(_GATHER) >= 8:
            _GATHER.clear()
        box = _GATHER[key] = _GatherBuffers(device, world, rank, width)
    return box


# phase marks of one trim_batch call (tools/c5_collective.py): None = off
_TRACE = None


def _mark(what):
    if _TRACE is not None:
        import time
        _TRACE.append((what, time.perf_counter()))


def _rebuild(alignment, keep_res, keep_seq, trimmer):
    dense = alignment._dense()
    whole = len(alignment._seq_idx) == len(alignment._names)  # (every sequence visible: the list of names is shared, not copied)
    out = TrimmedAlignment._from_parts(alignment._names if whole else alignment.names, dense, alignment._datatype, keep_seq, keep_res)
    # (what `terminal_only` counts over, asked of the trimmer's parameter block as `trimmer._finish` asks it for the results a
    # trim builds itself; a `trim_fn` may come without a trimmer)
    out._gap_stats = isinstance(trimmer, BaseTrimmer) and computes_gap_stats(trimmer._template())
    return out


# ---- files -> masks: FASTA parsed on the device ----------------------------------------------------------------------------
# Every non-empty FASTA text goes to the device, whatever its size: the device parse was faster at every size measured
# (tools/from_files.py, profiles/r07_from_files.jsonl: 1024 files of 100 x 1000 (102 KB each) 99 ms against 207 ms through
# Alignment.load + trim_batch, the C5 set 57 ms against 225), so there is no threshold below which small files take the host path.


def trim_files(trimmer, files, matrix=None, *, format=None, masks_only=False, threads=6, device=None, output=None,
               output_format="fasta"):
    """Trim the alignments in `files` (paths or binary file objects) on this process's device.

    Returns and raises what ``trim_batch(trimmer, [Alignment.load(f, format) for f in files], matrix, shard=False,
    masks_only=masks_only)`` does, but FASTA texts never become host rows: each is copied to the device as it is and parsed
    there into the alignment's device layout (`msa_trim_batch_fasta`, include/msastat.h), then trimmed by the native
    workers (`threads` of them) with the matrix of its type.  Other formats, and texts the device does not parse (empty,
    longer than 2^31 - 1 bytes), go through `Alignment.load` and the row path in the same call.  Results come in input
    order; the failure of the first file (in input order) that does not load is raised before any trim failure.

    `output`: a sequence as long as `files` of paths or binary file objects.  The call then also writes, for every file,
    the bytes ``result.dump(output[k], output_format)`` writes for the `TrimmedAlignment` it returns (or would return
    without `masks_only`), and returns what it returns without `output`.  For FASTA inputs and `output_format` "fasta",
    "fasta_m10", "clustal", "phylip" / "phylip40", "phylip32", "phylippaml" or one of the three PHYLIP formats' "_m10"
    variants the native workers compose the text on the device behind the trim, under the masks it produced and with
    the names in the input text (`msa_trim_batch_fasta_emit`), and only the text comes back: with `masks_only=True` no
    rows are downloaded -- files in, files out.  Everything else (inputs that went through `Alignment.load`, a name with
    a non-ASCII byte, the other formats -- NEXUS, MEGA, PIR / NBRF, HTML --, a text of 2^31 bytes or more) is written by
    the host writer from host rows, the same bytes.  A wrong length of `output` and a format `dumps` does not know are
    `ValueError`s before any work; nothing is written unless every file loaded and every trim succeeded, and the outputs
    are then written in input order.
    """
    files = list(files)
    output, emit = _check_output(output, output_format, len(files))
    if getattr(trimmer, "_platform", None) != "hip" or not (matrix is None or isinstance(matrix, SimilarityMatrix)):
        # (no device, or a matrix `trim` refuses: the composition itself, which raises what it raises where it raises it)
        # (`output` needs a device trim first: this raises before anything could be written)
        return trim_batch(trimmer, [Alignment.load(f, format) for f in files], matrix, device=device, threads=threads, shard=False,
                          masks_only=masks_only)
    texts, errors = _read_texts(files, format)
    # FASTA texts: parsed and trimmed on the device (a record for every text that holds an alignment, parsed or not)
    params3, _keep = trimmer._fasta_params(matrix)
    on_device = [k for k, (data, fmt) in enumerate(texts) if fmt == "fasta" and 0 < len(data) <= _lib.FASTA_MAX_BYTES]
    recs = {}
    if on_device:
        batch, outs = _on_native_batch(_device_index(device), threads, lambda b: b.trim_fasta(
            [texts[k][0] for k in on_device], _VALID.view(np.uint8), params3, want_rows=not masks_only, emit=emit))
        for k, rec in zip(on_device, outs):
            if rec.parse_rc not in (_lib.OK, _lib.E_BAD_RESIDUE, _lib.E_LENGTH_MISMATCH):
                batch.check(rec.parse_rc, rec.tinfo)  # a device failure (HIP, memory) is raised, never hidden behind the host path
            if rec.info.m > 0 and rec.info.n > 0:
                rec.batch, rec.data, rec.params = batch, texts[k][0], params3[type_index(rec.info.seq_type)]
                recs[k] = rec
    # the rest, and the texts without a record or with empty records, as Alignment.load reads them (its messages)
    loaded = {}
    for k, (data, fmt) in enumerate(texts):
        if k not in recs:
            try:
                loaded[k] = Alignment._from_text(data if isinstance(data, bytes) else bytes(data), files[k], format, fmt)
            except Exception as err:
                errors[k] = err
    for k in range(len(files)):  # the first file that does not load, in input order
        if k in errors:
            raise errors[k]
        if k in recs and recs[k].parse_rc != _lib.OK:
            raise _fasta_error(recs[k])
    # ... through the row path (what trim_batch does with them)
    prepared, outs, batch, _ = _trim_rows(trimmer, loaded.values(), matrix, device, threads)
    for (k, a), (names, dense, _, params, _keep), out in zip(loaded.items(), prepared, outs):
        res, seq, info, rc, rows = out or (None, None, None, _lib.OK, None)
        recs[k] = _lib.TrimRecord(res, seq, info, rc, rows, dense, names=names, datatype=a._datatype, params=params, batch=batch)
    for k in range(len(files)):  # trim failures, in input order
        if recs[k].rc != _lib.OK:
            recs[k].batch.check(recs[k].rc, recs[k].tinfo)
    out = []
    for k in range(len(files)):
        rec = recs[k]
        if rec.names is None and (not masks_only or rec.tinfo.warnings):  # (a device text's, out of the text: only when somebody reads them)
            rec.names = _fasta_names(rec)
        res, seq, t = _result(trimmer, rec.names, rec.rows, rec.datatype, rec.keep_res, rec.keep_seq, rec.tinfo, rec.only_gaps_rows,
                              rec.params, masks_only)
        if t is not None and rec.info is not None and res.all() and seq.all():
            t._detected_type = rec.info.seq_type  # (nothing removed: the type the device detected is the result's)
        out.append((np.asarray(res, dtype=bool), np.asarray(seq, dtype=bool)) if masks_only else t)
    if output is not None:  # every file loaded, every trim succeeded: the outputs, in input order
        for k, (data, fmt) in enumerate(texts):
            _write_output(output[k], output_format, recs[k], out[k], lambda: Alignment._from_text(bytes(data), files[k], format, fmt))
    return out


def _check_output(output, output_format, count):
    """`trim_files`'s `output` / `output_format` -> (the outputs as a list or None, the format for the device writer or None);
    a `ValueError` for a wrong length and for a format `dumps` does not know (what it checks, and its message)."""
    if output is None:
        return None, None
    output = list(output)
    if len(output) != count:
        raise ValueError(f"`output` has {len(output)} entries for {count} files")
    fmt_out = output_format.lower()
    short = fmt_out.endswith("_m10")
    base = fmt_out[:-4] if short else fmt_out
    if base not in _WRITERS or (short and base not in _M10_FORMATS):
        raise ValueError(f"Could not recognize alignment format: {output_format!r}")
    emit = ("phylip40" + fmt_out[6:]) if base == "phylip" else fmt_out  # (`dumps`' alias, which the device table does not hold)
    return output, (emit if emit in _lib.TEXT_FORMATS else None)


def _read_texts(files, format):
    """[(data: bytes or a mapping, format name)] for the files up to the first that cannot be read, and {its index: the error}"""
    texts = []
    for k, f in enumerate(files):
        try:
            data = _read_input(f, format, mapped=True)
            fmt = format if format is not None else (_sniff_format(data) if isinstance(data, bytes) else _sniff_mapped(data))
            texts.append((data, fmt.lower()))
        except Exception as err:
            return texts, {k: err}
    return texts, {}


def _write_output(target, output_format, rec, result, reload):
    """One output of `trim_files`: the text the device composed, else the host writer on the result object -- or, with
    `masks_only` (`result` is the mask pair), on what it would have been."""
    if rec.text is None:
        if isinstance(result, tuple):
            res, seq = result
            if rec.info is None:
                result = TrimmedAlignment._from_parts(rec.names, rec.rows, rec.datatype, seq, res)
            else:  # parsed on the device and not composed there (a flag): its rows as the host reads them
                a = reload()
                result = TrimmedAlignment._from_parts(a._names, a._matrix, a._datatype, seq, res)
        result.dump(target, output_format)
    else:
        _write_bytes(target, rec.text)


def _fasta_names(rec):
    return [bytes(rec.data[o:o + n]) for o, n in zip(rec.name_off.tolist(), rec.name_len.tolist())]


def _fasta_error(rec):
    """The ValueError `Alignment.load` raises for this parse failure (alignment._load_native)."""
    d = rec.detail
    if rec.parse_rc == _lib.E_LENGTH_MISMATCH:
        return ValueError(f"Sequence length mismatch in sequence {d.row}: {d.col} != {rec.info.n}")
    name = _fasta_names(rec)[d.row]
    return ValueError(f"The sequence \"{name.decode('ascii', 'replace')}\" has an unknown ({d.byte}) character")
