"""Files -> trimmed files: the text composed on the device (`trim_files(..., output=...)`) against result objects + `dump`.

The two file sets of tools/from_files.py (the C5 set: 64 x synth_msa(1000, 4000, 2000 + k), `automated1`; 1024 x
synth_msa(100, 1000, 5000 + k), `strict`) as FASTA wrapped at 60 in a temporary directory, outputs in two more directories
created beside them before anything is timed.  Alternating legs, medians of --repeats after --warmup, the outputs written in
--output-format (fasta; phylip, phylip32, ... for the PHYLIP family the device composes too):
  p_parent_route      trim_files(...) -> TrimmedAlignment objects, then t.dump(path, format) per result (nothing newer than
                      `trim_files` itself: the same script runs on the commit before the device writer, with --legs p)
  q_files_to_files    trim_files(..., masks_only=True, output=paths, output_format=format)  (device text, no rows downloaded; on
                      a commit whose device writer lacks the format the same call is the host writer's: the baseline)
  n_null_outputs      q with output objects whose `write` drops the text (q without the file system: q - n is the file writes,
                      n - b the composition, the download and the copy of every text out of the library)
  b_trim_files_masks  trim_files(..., masks_only=True)                   (files -> masks: the floor)
and for one C5 text alone: Context.upload_fasta + trim + emit_text against Alignment.load + trim + dumps, and emit_text alone
(index pass, compose pass, download) with its GB/s of text.  Every output file of q is compared with p's (`files_equal`); `out_sha256` is one digest over q's
outputs in input order, to compare the files of two builds.
One JSON line per case to stdout and, when given, --out (--append: added to the file; --label: a note that goes into every line, e.g. which
build ran).
--profile: q on the C5 set only, a few times -- the command to put behind `rocprofv3 --kernel-trace --stats`.

    python tools/to_files.py [--cases c5,small] [--legs p,q,n,b,one] [--output-format fasta] [--out FILE] [--append] [--profile]
(without --out nothing is written beside stdout; profiles/r08_to_files.jsonl and r09_to_files_phylip.jsonl are runs of it with --out)
"""
import argparse
import hashlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (before the HIP library: see pytrimal_amd._lib)

from pytrimal_amd import Alignment, AutomaticTrimmer, _lib  # noqa: E402
from pytrimal_amd.batch import trim_files  # noqa: E402
from pytrimal_amd.trimmer import type_index  # noqa: E402
from from_files import timed, write_set  # noqa: E402  (tools/ is the script's directory)


def out_paths(d, tag, paths):
    sub = os.path.join(d, tag)
    os.makedirs(sub, exist_ok=True)
    return [os.path.join(sub, os.path.basename(p) + ".out") for p in paths]


class NullSink:
    def write(self, data):
        return len(data)


def run_case(name, paths, trimmer, warmup, repeats, threads, d, which, fmt):
    nbytes = sum(os.path.getsize(p) for p in paths)
    p_out, q_out = out_paths(d, name + "_p", paths), out_paths(d, name + "_q", paths)

    def parent_route():
        for t, path in zip(trim_files(trimmer, paths, threads=threads), p_out):
            t.dump(path, fmt)

    legs = {}
    if "p" in which:
        legs["p_parent_route"] = parent_route
    if "q" in which:
        legs["q_files_to_files"] = lambda: trim_files(trimmer, paths, masks_only=True, threads=threads, output=q_out, output_format=fmt)
    if "n" in which:
        sinks = [NullSink() for _ in paths]
        legs["n_null_outputs"] = lambda: trim_files(trimmer, paths, masks_only=True, threads=threads, output=sinks, output_format=fmt)
    if "b" in which:
        legs["b_trim_files_masks"] = lambda: trim_files(trimmer, paths, masks_only=True, threads=threads)
    times = {k: [] for k in legs}
    for rep in range(warmup + repeats):
        for k, fn in legs.items():  # alternating
            ms = timed(fn)
            if rep >= warmup:
                times[k].append(ms)
    med = {k: round(statistics.median(v), 2) for k, v in times.items()}
    rec = {"case": name, "files": len(paths), "text_bytes": nbytes, "method": trimmer.method, "output_format": fmt, "threads": threads,
           "repeats": repeats,
           "ms_median": med, "ms_all": {k: [round(x, 2) for x in v] for k, v in times.items()}}
    if "q" in which:
        digest = hashlib.sha256()
        for b in q_out:
            with open(b, "rb") as fb:
                digest.update(fb.read())
        rec["out_sha256"] = digest.hexdigest()
        rec["out_bytes"] = sum(os.path.getsize(p) for p in q_out)
    if "p" in which and "q" in which:
        equal = True
        for a, b in zip(p_out, q_out):
            with open(a, "rb") as fa, open(b, "rb") as fb:
                equal = equal and fa.read() == fb.read()
        rec["files_equal"] = bool(equal)
        rec["q_over_p"] = round(med["q_files_to_files"] / med["p_parent_route"], 3)
        rec["q_under_half_of_p"] = bool(med["q_files_to_files"] < 0.5 * med["p_parent_route"])
    if "q" in which and "b" in which:
        rec["q_minus_b_ms"] = round(med["q_files_to_files"] - med["b_trim_files_masks"], 2)
    if "q" in which and "n" in which:
        rec["q_minus_n_ms"] = round(med["q_files_to_files"] - med["n_null_outputs"], 2)
    return rec


def one_text_case(path, trimmer, warmup, repeats, fmt):
    """one C5 text alone, on one context: device route (upload_fasta + trim + emit_text) against the host route
    (Alignment.load + trim + dumps), and emit_text alone under the masks of that trim"""
    with open(path, "rb") as f:
        text = f.read()
    ctx = _lib.Context(0)
    params, _keep = trimmer._fasta_params(None)
    state = {}
    emit_fmt = {"phylip": "phylip40", "phylip_m10": "phylip40_m10"}.get(fmt.lower(), fmt)  # (`dumps`' alias)

    def device_route():
        info = ctx.upload_fasta(text)
        res, seq, _ = ctx.trim(params[type_index(info.seq_type)])
        state["masks"] = (res, seq)
        state["device"] = ctx.emit_text(emit_fmt, res, seq)

    def host_route():
        state["host"] = trimmer.trim(Alignment.load(io.BytesIO(text), "fasta")).dumps(fmt).encode()

    def emit_alone():
        state["emit"] = ctx.emit_text(emit_fmt, *state["masks"])

    legs = {"device_upload_trim_emit": device_route, "host_load_trim_dumps": host_route, "emit_text_alone": emit_alone}
    times = {k: [] for k in legs}
    for rep in range(warmup + repeats):
        for k, fn in legs.items():
            ms = timed(fn)
            if rep >= warmup:
                times[k].append(ms)
    ctx.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    out_bytes = len(state["device"])
    return {"case": "one_c5_text", "text_bytes": len(text), "out_bytes": out_bytes, "output_format": fmt, "repeats": repeats,
            "ms_median": {k: round(v, 3) for k, v in med.items()},
            "texts_equal": bool(state["device"] == state["host"] == state["emit"]),
            "GBps_emit_text_alone": round(out_bytes / med["emit_text_alone"] / 1e6, 2),
            "GBps_host_dumps_route": round(out_bytes / med["host_load_trim_dumps"] / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c5,small")
    ap.add_argument("--legs", default="p,q,n,b,one")
    ap.add_argument("--output-format", default="fasta")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--threads", type=int, default=6)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("to_files.py needs a HIP device")
    fmt = args.output_format
    which = set(args.legs.split(","))
    cases = args.cases.split(",")
    recs = []

    def emit(rec):
        if args.label:
            rec["label"] = args.label
        rec["legs"] = sorted(which)
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    with tempfile.TemporaryDirectory() as d:
        a1 = AutomaticTrimmer("automated1", platform="hip")
        if args.profile or "c5" in cases:
            c5 = write_set(d, "c5", 64, 1000, 4000, 2000)
        if args.profile:
            outs = out_paths(d, "profile_q", c5)
            for _ in range(4):
                trim_files(a1, c5, masks_only=True, threads=args.threads, output=outs, output_format=fmt)
            print(json.dumps({"profile": "q_files_to_files", "output_format": fmt, "files": len(c5), "calls": 4}), flush=True)
            return
        if "c5" in cases:
            if "one" in which:
                emit(one_text_case(c5[0], a1, args.warmup, 3 * args.repeats, fmt))
            emit(run_case("c5_64x1000x4000", c5, a1, args.warmup, args.repeats, args.threads, d, which, fmt))
        if "small" in cases:
            small = write_set(d, "small", 1024, 100, 1000, 5000)
            emit(run_case("small_1024x100x1000", small, AutomaticTrimmer("strict", platform="hip"), args.warmup, args.repeats, args.threads,
                          d, which, fmt))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
