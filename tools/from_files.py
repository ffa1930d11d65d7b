"""Files -> masks: FASTA parsed on the device (`trim_files`) against host parsing (`Alignment.load` + `trim_batch`).

Writes the C5 set (64 x synth_msa(1000, 4000, 2000 + k), `automated1`) and 1024 x synth_msa(100, 1000, 5000 + k) (`strict`)
as FASTA wrapped at 60 into a temporary directory, then times, alternating, medians of --repeats after --warmup:
  a  Alignment.load + trim_batch(masks_only=True)       (host parsing, today's path)
  b  trim_files(masks_only=True)                        (device parsing)
  c  trim_files(masks_only=False)                       (device parsing, full TrimmedAlignment objects)
  d  trim_batch(masks_only=True) on rows already loaded (the from-rows reference)
and the device ingest alone: Context.upload_fasta of one C5 text, pageable copy against pinned staging.  One JSON line per case to stdout and --out.
--profile: (b) on the C5 set only, a few times -- the command to put behind `rocprofv3 --kernel-trace --stats`.

    python tools/from_files.py [--cases c5,small] [--out profiles/r07_from_files.jsonl] [--profile]
"""
import argparse
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
from pytrimal_amd.batch import trim_batch, trim_files  # noqa: E402
from pytrimal_amd.synth import synth_msa  # noqa: E402


def fasta(a, width=60):
    out = []
    for i, row in enumerate(a):
        out.append(b">s%d\n" % i)
        row = row.tobytes()
        out.extend(row[j:j + width] + b"\n" for j in range(0, len(row), width))
    return b"".join(out)


def write_set(d, tag, count, m, n, seed0):
    paths = []
    for k in range(count):
        p = os.path.join(d, f"{tag}_{k}.fasta")
        with open(p, "wb") as f:
            f.write(fasta(synth_msa(m, n, seed0 + k)))
        paths.append(p)
    return paths


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def run_case(name, paths, trimmer, warmup, repeats, threads):
    loaded = [Alignment.load(p) for p in paths]
    nbytes = sum(os.path.getsize(p) for p in paths)
    legs = {
        "a_load_trim_batch": lambda: trim_batch(trimmer, [Alignment.load(p) for p in paths], shard=False, masks_only=True, threads=threads),
        "b_trim_files_masks": lambda: trim_files(trimmer, paths, masks_only=True, threads=threads),
        "c_trim_files_full": lambda: trim_files(trimmer, paths, threads=threads),
        "d_trim_batch_rows": lambda: trim_batch(trimmer, loaded, shard=False, masks_only=True, threads=threads),
    }
    ref = legs["d_trim_batch_rows"]()
    got = legs["b_trim_files_masks"]()
    same = all((r[0] == g[0]).all() and (r[1] == g[1]).all() for r, g in zip(ref, got))
    times = {k: [] for k in legs}
    for rep in range(warmup + repeats):
        for k, fn in legs.items():  # alternating
            ms = timed(fn)
            if rep >= warmup:
                times[k].append(ms)
    med = {k: round(statistics.median(v), 2) for k, v in times.items()}
    rec = {"case": name, "files": len(paths), "text_bytes": nbytes, "method": trimmer.method, "threads": threads,
           "repeats": repeats, "masks_equal_rows_path": bool(same), "ms_median": med,
           "ms_all": {k: [round(x, 2) for x in v] for k, v in times.items()},
           "b_over_a": round(med["b_trim_files_masks"] / med["a_load_trim_batch"], 3),
           "b_over_d": round(med["b_trim_files_masks"] / med["d_trim_batch_rows"], 3),
           "files_to_masks_GBps_b": round(nbytes / med["b_trim_files_masks"] / 1e6, 2),
           "files_to_masks_GBps_a": round(nbytes / med["a_load_trim_batch"] / 1e6, 2)}
    return rec


def ingest_case(path, warmup, repeats):
    """msa_upload_fasta of one text alone (copy + parse + the two waits): the text copied from pageable memory as it is (what
    ships) and through the context's pinned staging in 1 MB pieces (MSA_UPLOAD_DIRECT=0, a diagnostic switch), alternating;
    msa_fasta_scan + fill on the host (Alignment.load) beside them."""
    with open(path, "rb") as f:
        text = f.read()
    os.environ["MSA_DIAGNOSTICS"] = "1"
    ctxs = {}
    for name, direct in (("pageable", "1"), ("staged", "0")):
        os.environ["MSA_UPLOAD_DIRECT"] = direct  # (read when the context is created)
        ctxs[name] = _lib.Context(0)
    os.environ.pop("MSA_UPLOAD_DIRECT")
    times = {"pageable": [], "staged": [], "alignment_load": []}
    for rep in range(warmup + repeats):
        for name, ctx in ctxs.items():
            ms = timed(lambda: ctx.upload_fasta(text))
            if rep >= warmup:
                times[name].append(ms)
        ms = timed(lambda: Alignment.load(path))
        if rep >= warmup:
            times["alignment_load"].append(ms)
    info = ctxs["pageable"].text_info
    for ctx in ctxs.values():
        ctx.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    # the HBM bound of the parse: read the text once, write the matrix (m rows at the device pitch) once, at 8 TB/s
    hbm_bytes = len(text) + info.m * ((info.n + 63) // 64 * 64)
    return {"case": "ingest_one_c5_text", "text_bytes": len(text), "repeats": repeats,
            "ms_median_upload_fasta": round(med["pageable"], 3), "GBps_upload_fasta": round(len(text) / med["pageable"] / 1e6, 2),
            "ms_median_upload_fasta_staged": round(med["staged"], 3),
            "GBps_upload_fasta_staged": round(len(text) / med["staged"] / 1e6, 2),
            "ms_median_alignment_load": round(med["alignment_load"], 3),
            "GBps_alignment_load": round(len(text) / med["alignment_load"] / 1e6, 2),
            "hbm_bytes_text_and_matrix": hbm_bytes, "us_hbm_bound_8TBps": round(hbm_bytes / 8e12 * 1e6, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c5,small")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_from_files.jsonl"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--threads", type=int, default=6)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("from_files.py needs a HIP device")
    with tempfile.TemporaryDirectory() as d:
        c5 = write_set(d, "c5", 64, 1000, 4000, 2000)
        a1 = AutomaticTrimmer("automated1", platform="hip")
        if args.profile:
            for _ in range(4):
                trim_files(a1, c5, masks_only=True, threads=args.threads)
            print(json.dumps({"profile": "b_trim_files_masks", "files": len(c5), "calls": 4}), flush=True)
            return
        recs = []
        cases = args.cases.split(",")
        if "c5" in cases:
            recs.append(ingest_case(c5[0], args.warmup, 3 * args.repeats))
            print(json.dumps(recs[-1]), flush=True)
            recs.append(run_case("c5_64x1000x4000", c5, a1, args.warmup, args.repeats, args.threads))
            print(json.dumps(recs[-1]), flush=True)
        if "small" in cases:
            small = write_set(d, "small", 1024, 100, 1000, 5000)
            recs.append(run_case("small_1024x100x1000", small, AutomaticTrimmer("strict", platform="hip"), args.warmup, args.repeats,
                                 args.threads))
            print(json.dumps(recs[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
