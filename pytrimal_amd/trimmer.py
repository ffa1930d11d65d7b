"""Trimmer classes: the callers of the statistics path.

Mirror of ``pytrimal.BaseTrimmer`` and its four subclasses
(``/root/reference/src/pytrimal/_trimal.pyx:1170-1862``): same constructors, keyword validation,
``repr``, pickle state and ``trim(alignment, matrix=None)`` contract.  What the reference hands to
``trimAlManager::clean_alignment`` (``_trimal.pyx:1355``) goes to ``msa_trim`` of the HIP library
instead; the only compute platform of this package is ``"hip"``.
"""
import ctypes
import functools
import logging
import warnings

import numpy as np

from . import _lib
from .alignment import Alignment, TrimmedAlignment
from .matrix import SimilarityMatrix

_log = logging.getLogger("pytrimal_amd")

@functools.lru_cache(maxsize=None)
def _default_matrix(kind):
    """The built-in matrices `trim` falls back to (immutable here; building one costs ~1 ms)."""
    if kind == "aa":
        return SimilarityMatrix.aa()
    return SimilarityMatrix.nt(degenerated=(kind == "ntdeg"))


_TYPE_KINDS = ("aa", "nt", "ntdeg")


def type_index(ty):
    """A detected sequence type (trimAl's SequenceTypes bits) -> 0 amino acids, 1 nucleotides, 2 degenerate nucleotides: the
    default matrix of the type (create_or_use_similarity_matrix; an undetected type falls back to the AA matrix,
    _trimal.pyx:1342-1352) and the order of `_fasta_params` (the library's `seq_type_index` is the same rule)."""
    return 0 if (ty & 4 or ty == 0) else (2 if ty & 8 else 1)


def computes_gap_stats(params):
    """Does a trim with this parameter block compute gap statistics (every column trimmer does; the sequence trimmers do not)?
    `terminal_only` shares them with the source alignment when it did, and counts over the kept sequences when it did not."""
    return (params.method != _lib.METHOD_CODES["noduplicateseqs"] and params.clusters == -1 and params.max_identity == -1
            and not (params.residue_overlap != -1 and params.sequence_overlap != -1))


@functools.lru_cache(maxsize=None)
def _best_platform():
    """"hip" when a device is visible, else `None`.  Resolved on first use (a trimmer is constructed), never at
    import: loading the HIP library and counting devices initialises the GPU runtime, and a process that merely
    imports the package must stay free to fork workers or to import torch first (see `_lib`)."""
    return "hip" if _lib.device_count() > 0 else None


def __getattr__(name):
    # the reference's module-level constants (`_trimal._SSE2_RUNTIME_SUPPORT` style), evaluated lazily
    if name == "_BEST_PLATFORM":
        return _best_platform()
    if name == "_HIP_RUNTIME_SUPPORT":
        return _best_platform() == "hip"
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _raise_warnings(info, names, only_gaps_rows):
    """trimAl's warnings as `RuntimeWarning`, the category the reference gives them
    (``/root/reference/src/trimal/source/reportsystem.cpp:132-173``).  Only what maps to a trimAl `WarningCode`
    is raised: one warning per sequence removed because the trimming left it with gaps only
    (RemovingOnlyGapsSequence [R], reported per sequence by Cleaner::removeAllGapsSeqsAndCols).  The other `MSA_W_*`
    bits (every column removed, undefined identities) have no counterpart among the reference's warnings: a caller
    running with `-W error` must not see exceptions the reference would not raise, so they go to the
    `pytrimal_amd` logger instead."""
    w = info.warnings
    if not w:
        return
    if w & _lib.W_ONLY_GAPS_SEQUENCES:
        for i in only_gaps_rows or [info.warn_row]:
            name = names[i].decode("ascii", "replace") if 0 <= i < len(names) else "?"
            warnings.warn(f"Removing sequence '{name}' composed only by gaps", RuntimeWarning, stacklevel=3)
    if w & _lib.W_NO_COLUMNS_LEFT:
        _log.info("the trimming removed every column of the alignment")
    if w & _lib.W_UNDEFINED_IDENTITY:
        _log.info("some pairs of sequences share no residue column: their identity is taken as 0")


def _check_range(value, name, lo, hi, cast=float):
    try:
        v = cast(value)
    except (TypeError, ValueError):
        raise TypeError(f"Invalid type for `{name}`: {type(value).__name__}") from None
    if v < lo or v > hi or v != v:
        raise ValueError(f"Invalid value for `{name}`: {v!r}")
    return v


def _check_positive(value, name, cast=int):
    try:
        v = cast(value)
    except (TypeError, ValueError):
        raise TypeError(f"Invalid type for `{name}`: {type(value).__name__}") from None
    if v <= 0:
        raise ValueError(f"Invalid value for `{name}`: {v!r}")
    return v


class BaseTrimmer:
    """A sequence alignment trimmer.  Subclasses are configured through their constructor and
    all provide the same `trim` method."""

    def __init__(self, *, platform="detect"):
        if platform == "detect":
            self._platform = _best_platform()
        elif platform == "hip":
            if not _lib.device_count():
                raise RuntimeError("Cannot run HIP kernels on this machine (no gfx950 device or library missing)")
            self._platform = "hip"
        elif platform is None:
            self._platform = None
        elif isinstance(platform, str):
            raise ValueError(f"Unsupported platform on this architecture: {platform!r}")
        else:
            raise TypeError(f"expected str or None, found {type(platform).__name__}")

    def __repr__(self):
        arg = f"platform={self.platform!r}" if self._platform != _best_platform() else ""
        return f"{type(self).__name__}({arg})"

    def __getstate__(self):
        return {"platform": self.platform}

    def __setstate__(self, state):
        try:
            BaseTrimmer.__init__(self, platform=state["platform"])
        except (ValueError, RuntimeError):
            BaseTrimmer.__init__(self, platform="detect")

    @property
    def platform(self):
        """`str` or `None`: The compute platform for this trimmer."""
        return self._platform

    # subclasses fill the C parameter block (the trimAlManager fields of `_configure_manager`)
    def _configure(self, params):
        pass

    def _prepare(self, alignment, matrix=None):
        """What `trim` hands to the C ABI for one alignment: (names, dense residue matrix, indetermination symbol,
        parameter block, objects the block points into)."""
        if not isinstance(alignment, Alignment):
            raise TypeError(f"expected Alignment, found {type(alignment).__name__}")
        if matrix is not None and not isinstance(matrix, SimilarityMatrix):
            raise TypeError(f"expected SimilarityMatrix, found {type(matrix).__name__}")
        if self._platform != "hip":
            raise RuntimeError(
                "this build computes the alignment statistics on an MI355X only: no CPU platform exists "
                "(platform=None / no visible device); construct the trimmer with platform='hip' on a GPU host")
        # a TrimmedAlignment is first materialised to its kept sequences / residues (_trimal.pyx:1324-1327)
        dense = alignment._dense()
        if dense is alignment._matrix and dense.size:
            # an alignment that is trimmed again (another trimmer, another setting): its rows are page-locked from the
            # second trim on -- every further upload is one DMA copy from where they lie -- until the matrix dies or the
            # process-wide budget needs the room (PYTRIMAL_AMD_PIN_MB, least recently uploaded first; 0 = never)
            uploads = alignment._uploads = getattr(alignment, "_uploads", 0) + 1
            # (rows of less than 96 KB are packed into the context's own pinned area and read there by the kernels: nothing to lock)
            if (uploads == 2 or not uploads & 15) and dense.nbytes > (96 << 10):  # (and again now and then: the budget may have unpinned it since)
                _lib.pin_array(dense)
        ty = alignment._alignment_type()
        indet = ord("X") if (ty & 4) else ord("N")
        if matrix is None:
            matrix = _default_matrix(_TYPE_KINDS[type_index(ty)])
        params, keep = self._params_for(matrix)
        return alignment.names, dense, indet, params, keep

    def _template(self):
        """This trimmer's parameter block, without a matrix."""
        template = _lib.TrimParams(0, -1.0, -1, -1.0, -1.0, -1, -1, -1, -1.0, -1.0, -1, -1.0, None, None, 0)
        self._configure(template)
        return template

    def _params_for(self, matrix):
        """The parameter block of this trimmer for `matrix` and the objects it points into."""
        # the parameter block of this trimmer for this matrix: filled once, copied per alignment (trim_batch prepares
        # thousands of small alignments per call)
        # (keyed by the matrix AND by what configures the block -- the trimmer's state: an attribute written after the first
        # trim, or a `__setstate__` on a used object, must not keep the old thresholds)
        cache = self.__dict__.setdefault("_params_cache", {})
        key = (id(matrix), tuple(self.__getstate__().items()))
        entry = cache.get(key)
        if entry is None or entry[2] is not matrix:
            template = self._template()
            vhash, dist = matrix._device_arrays()
            template.vhash = vhash.ctypes.data_as(ctypes.c_void_p)
            template.dist = dist.ctypes.data_as(ctypes.c_void_p)
            template.npos = len(matrix)
            if len(cache) > 64:
                cache.clear()
            entry = cache[key] = (bytes(template), (vhash, dist, matrix), matrix)
        return _lib.TrimParams.from_buffer_copy(entry[0]), entry[1]

    def _fasta_params(self, matrix=None):
        """The three parameter blocks of `msa_trim_batch_fasta` -- amino acids (and an undetected type), nucleotides,
        degenerate nucleotides: the matrices `_prepare` picks by type.  (`matrix`: None or a SimilarityMatrix; the caller
        has checked it and the platform, as `_prepare` does.)"""
        kinds = (matrix,) * 3 if matrix is not None else tuple(_default_matrix(k) for k in _TYPE_KINDS)
        out, keep = (_lib.TrimParams * 3)(), []
        for i, mx in enumerate(kinds):
            out[i], k = self._params_for(mx)
            keep.append(k)
        return out, keep

    @staticmethod
    def _finish(names, dense, datatype, keep_res, keep_seq, info, only_gaps_rows, gaps_w, params):
        """masks -> `TrimmedAlignment` (+ the warnings trimAl would have reported)"""
        if info is not None and info.warnings:
            _raise_warnings(info, names, only_gaps_rows)
        out = TrimmedAlignment._from_parts(names, dense, datatype, keep_seq, keep_res)
        # what `terminal_only` needs of the gap statistics this trim computed (trimAl's trimmed alignment shares the
        # statistics object of its source): the half window, and the windowed vector itself when the trim fetched it
        out._gap_hw = max(params.window if params.window != -1 else params.gap_window, 0)
        out._gaps_w = gaps_w
        out._gap_stats = computes_gap_stats(params)
        return out

    def trim(self, alignment, matrix=None):
        """Trim the provided alignment and return a `TrimmedAlignment`.

        Re-entrant: each thread works on its own device context and stream.
        """
        names, dense, indet, params, _keep = self._prepare(alignment, matrix)
        m, n = dense.shape
        if m == 0 or n == 0:
            return self._finish(names, dense, alignment._datatype, np.ones(n, dtype=bool), np.ones(m, dtype=bool), None, None, None, params)
        ctx = _lib.thread_context()
        ctx.upload(dense, indet, wait=False)  # (`dense` lives until the trim has waited for the stream)
        keep_res, keep_seq, info = ctx.trim(params)
        rows = ctx.only_gaps_rows() if info.warnings & _lib.W_ONLY_GAPS_SEQUENCES else None
        hw = max(params.window if params.window != -1 else params.gap_window, 0)
        return self._finish(names, dense, alignment._datatype, keep_res, keep_seq, info, rows, ctx.gaps_cached(hw), params)


class AutomaticTrimmer(BaseTrimmer):
    """A sequence alignment trimmer with automatic parameter detection."""

    METHODS = frozenset({
        "strict", "strictplus", "gappyout", "nogaps", "noallgaps", "automated1", "automated2",
        "noduplicateseqs",
    })

    def __init__(self, method="strict", *, platform="detect"):
        super().__init__(platform=platform)
        if not isinstance(method, str):
            raise TypeError(f"expected str, found {type(method).__name__}")
        if method not in self.METHODS:
            raise ValueError(f"Invalid value for `method`: {method!r}")
        if method == "automated2":
            # A name of the reference's API (`_trimal.pyx:1384,1417,1494-1495`) whose algorithm is not in the reference
            # tree (trimAl submodule empty) and whose only test fixture is a dangling symlink: there is nothing to
            # restate it from and nothing to check a restatement against.  Refused here, where the method is chosen,
            # not from inside `trim()`.
            raise NotImplementedError(
                "method 'automated2' is not available in this build: trimAl's implementation is not part of the reference "
                "checkout and no fixture of it survives, so it could be neither restated nor verified; use 'automated1', "
                "'gappyout', 'strict' or 'strictplus'")
        self.method = method

    def __repr__(self):
        args = [repr(self.method)]
        if self._platform != _best_platform():
            args.append(f"platform={self.platform!r}")
        return f"{type(self).__name__}({', '.join(args)})"

    def __getstate__(self):
        return {"method": self.method, "platform": self.platform}

    def __setstate__(self, state):
        BaseTrimmer.__setstate__(self, state)
        self.method = state["method"]

    def _configure(self, params):
        params.method = _lib.METHOD_CODES[self.method]


class ManualTrimmer(BaseTrimmer):
    """A sequence alignment trimmer with manually defined thresholds."""

    def __init__(self, *, gap_threshold=None, gap_absolute_threshold=None, similarity_threshold=None,
                 conservation_percentage=None, window=None, gap_window=None, similarity_window=None,
                 platform="detect"):
        super().__init__(platform=platform)
        self._gap_threshold = -1
        self._gap_absolute_threshold = -1
        self._similarity_threshold = -1
        self._conservation_percentage = -1
        self._window = -1
        self._gap_window = -1
        self._similarity_window = -1
        if gap_threshold is not None and gap_absolute_threshold is not None:
            raise ValueError("Cannot specify both `gap_threshold` and `gap_absolute_threshold`")
        if window is not None and (gap_window is not None or similarity_window is not None):
            raise ValueError("Cannot specify both `window` and a specific window argument")
        if gap_threshold is not None:
            # stored as the maximum gap FRACTION in float32, like the reference's `cdef float` (:1589)
            self._gap_threshold = float(np.float32(1) - np.float32(_check_range(gap_threshold, "gap_threshold", 0, 1)))
        if gap_absolute_threshold is not None:
            self._gap_absolute_threshold = _check_positive(gap_absolute_threshold, "gap_absolute_threshold")
        if similarity_threshold is not None:
            self._similarity_threshold = float(np.float32(_check_range(similarity_threshold, "similarity_threshold", 0, 1)))
        if conservation_percentage is not None:
            self._conservation_percentage = float(np.float32(
                _check_range(conservation_percentage, "conservation_percentage", 0, 100)))
        if window is not None:
            self._window = _check_positive(window, "window")
        if gap_window is not None:
            self._gap_window = _check_positive(gap_window, "gap_window")
        if similarity_window is not None:
            self._similarity_window = _check_positive(similarity_window, "similarity_window")

    def __repr__(self):
        args = []
        if self._gap_threshold != -1:
            args.append(f"gap_threshold={float(np.float32(1) - np.float32(self._gap_threshold))!r}")
        if self._gap_absolute_threshold != -1:
            args.append(f"gap_absolute_threshold={self._gap_absolute_threshold!r}")
        if self._similarity_threshold != -1:
            args.append(f"similarity_threshold={self._similarity_threshold!r}")
        if self._conservation_percentage != -1:
            args.append(f"conservation_percentage={self._conservation_percentage!r}")
        if self._window != -1:
            args.append(f"window={self._window!r}")
        if self._gap_window != -1:
            args.append(f"gap_window={self._gap_window!r}")
        if self._similarity_window != -1:
            args.append(f"similarity_window={self._similarity_window!r}")
        if self._platform != _best_platform():
            args.append(f"platform={self.platform!r}")
        return f"{type(self).__name__}({', '.join(args)})"

    def __getstate__(self):
        return {
            "platform": self.platform,
            "gap_threshold": self._gap_threshold,
            "gap_absolute_threshold": self._gap_absolute_threshold,
            "similarity_threshold": self._similarity_threshold,
            "conservation_percentage": self._conservation_percentage,
            "window": self._window,
            "gap_window": self._gap_window,
            "similarity_window": self._similarity_window,
        }

    def __setstate__(self, state):
        BaseTrimmer.__setstate__(self, state)
        self._gap_threshold = state["gap_threshold"]
        self._gap_absolute_threshold = state["gap_absolute_threshold"]
        self._similarity_threshold = state["similarity_threshold"]
        self._conservation_percentage = state["conservation_percentage"]
        self._window = state["window"]
        self._gap_window = state["gap_window"]
        self._similarity_window = state["similarity_window"]

    def _configure(self, params):
        params.method = 0
        params.gap_threshold = self._gap_threshold
        params.gap_absolute_threshold = self._gap_absolute_threshold
        params.similarity_threshold = self._similarity_threshold
        params.conservation_percentage = self._conservation_percentage
        params.window = self._window
        params.gap_window = self._gap_window
        params.similarity_window = self._similarity_window


class OverlapTrimmer(BaseTrimmer):
    """A sequence alignment trimmer for overlap blocks."""

    def __init__(self, sequence_overlap, residue_overlap, *, platform="detect"):
        super().__init__(platform=platform)
        self._sequence_overlap = float(np.float32(_check_range(sequence_overlap, "sequence_overlap", 0, 100)))
        self._residue_overlap = float(np.float32(_check_range(residue_overlap, "residue_overlap", 0, 1)))

    def __repr__(self):
        args = [repr(self._sequence_overlap), repr(self._residue_overlap)]
        if self._platform != _best_platform():
            args.append(f"platform={self.platform!r}")
        return f"{type(self).__name__}({', '.join(args)})"

    def __getstate__(self):
        return {"platform": self.platform, "sequence_overlap": self._sequence_overlap,
                "residue_overlap": self._residue_overlap}

    def __setstate__(self, state):
        BaseTrimmer.__setstate__(self, state)
        self._sequence_overlap = state["sequence_overlap"]
        self._residue_overlap = state["residue_overlap"]

    def _configure(self, params):
        params.method = 0
        params.residue_overlap = self._residue_overlap
        params.sequence_overlap = self._sequence_overlap


class RepresentativeTrimmer(BaseTrimmer):
    """A sequence alignment trimmer for selecting representative sequences."""

    def __init__(self, clusters=None, identity_threshold=None, *, platform="detect"):
        super().__init__(platform=platform)
        self._clusters = -1
        self._identity_threshold = -1
        if clusters is not None and identity_threshold is not None:
            raise ValueError("Cannot specify both `clusters` and `identity_threshold`")
        if clusters is not None:
            self._clusters = _check_positive(clusters, "clusters")
        if identity_threshold is not None:
            self._identity_threshold = float(np.float32(_check_range(identity_threshold, "identity_threshold", 0, 1)))

    def __repr__(self):
        args = []
        if self._clusters != -1:
            args.append(f"clusters={self._clusters!r}")
        elif self._identity_threshold != -1:
            args.append(f"identity_threshold={self._identity_threshold!r}")
        if self._platform != _best_platform():
            args.append(f"platform={self.platform!r}")
        return f"{type(self).__name__}({', '.join(args)})"

    def __getstate__(self):
        return {"platform": self.platform, "clusters": self._clusters,
                "identity_threshold": self._identity_threshold}

    def __setstate__(self, state):
        BaseTrimmer.__setstate__(self, state)
        self._clusters = state["clusters"]
        self._identity_threshold = state["identity_threshold"]

    def _configure(self, params):
        params.method = 0
        params.clusters = self._clusters
        params.max_identity = self._identity_threshold
