"""phmm_finalize_reads on the headline's reads: 1 024 regions x 128 reads of 150 bases, one sample, all steps.  Prints one JSON
line (and writes it to --out): the whole call on the host clock (median and min over the timed calls, staging and copies
included), what the call staged, and what became of the reads.
Reads: seeded, 64 fragments per region; three in four of the first mates are 150M, the rest carry a leading and / or trailing
soft clip, an insertion or a deletion; the second mates are 150M on the other strand; one end in three has a low-quality tail
of 1 to 12 bases; in about a third of the fragments the mates overlap; 1 % of the bases differ from the region's reference.
The kernels' own times come from ONE run under
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fin -- python tools/finalize_bench.py --steps 10
and `python tools/finalize_bench.py --trace DIR --trace-out profiles/finalize_kernel_trace.txt` turns its kernel trace into the
table of per-kernel medians over the last ten launches.
usage: python tools/finalize_bench.py [--steps K] [--warmup W] [--regions N] [--out FILE] | --trace DIR [--trace-out FILE]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

READ, PER_REGION, SPAN, PAD = 150, 128, 500, 100
CIGARS = ["150M"] * 6 + ["12S138M", "140M10S", "5S140M5S", "70M2I78M", "70M3D80M", "3H8S60M1I40M2D41M"]
PAIRED, REVERSE, MATE_REVERSE, FIRST, SECOND = 0x1, 0x10, 0x20, 0x40, 0x80


def workload(n_regions, seed=2026):
    """The packed arrays of the call, built with numpy (lorikeet_amd.finalize.pack walks the reads one by one)."""
    from lorikeet_amd import finalize
    rng = np.random.default_rng(seed)
    enc = [np.array(finalize.encode_cigar(c), np.uint32) for c in CIGARS]
    lead = np.array([next((int(e) >> 4 if int(e) & 15 == 4 else 0 for e in c if int(e) & 15 != 5), 0) for c in enc])   # leading soft clip
    half = PER_REGION // 2
    n = n_regions * PER_REGION
    region = np.repeat(np.arange(n_regions), PER_REGION)
    start = 10000 + 1000 * np.arange(n_regions, dtype=np.int64)          # the padded span of region g: [start, start + SPAN]
    frag = rng.integers(-PAD, SPAN - READ, (n_regions, half))             # where a fragment's first mate starts in its span
    overlap = rng.random((n_regions, half)) < 0.34
    gap = np.where(overlap, rng.integers(-READ + 10, 0, (n_regions, half)), rng.integers(0, 250, (n_regions, half)))
    tmpl_first = rng.integers(0, len(CIGARS), (n_regions, half))
    pos_first = start[:, None] + frag
    pos_second = pos_first + READ + gap
    # reads 0..63 of a region are the first mates, 64..127 the second ones: mates lie far apart in input order
    pos = np.concatenate([pos_first, pos_second], 1).reshape(-1)
    tmpl = np.concatenate([tmpl_first, np.zeros_like(tmpl_first)], 1).reshape(-1)
    pos_aligned = pos + lead[tmpl]                                         # a read's position is that of its first aligned base
    first = np.tile(np.concatenate([np.ones(half, bool), np.zeros(half, bool)]), n_regions)
    flags = np.where(first, PAIRED | MATE_REVERSE | FIRST, PAIRED | REVERSE | SECOND).astype(np.uint16)
    idx = np.arange(n)
    mate = np.where(first, idx + half, idx - half).astype(np.int32)
    mpos = pos_aligned[mate]
    fragment = (pos_second + READ - pos_first)
    isize = np.concatenate([fragment, -fragment], 1).reshape(-1)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_regions, SPAN + 2 * PAD + 3 * READ + 300))
    offs = (pos - start[region] + PAD)[:, None] + np.arange(READ)[None, :]
    bases = ref[region[:, None], offs]
    flip = rng.random(bases.shape, dtype=np.float32) < 0.01
    bases[flip] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(flip.sum()))
    quals = rng.integers(20, 41, bases.shape, dtype=np.uint8)
    for side in (0, 1):
        k = np.where(rng.random(n) < 1 / 3, rng.integers(1, 13, n), 0)
        col = np.arange(READ)[None, :]
        low = (col < k[:, None]) if side == 0 else (col >= READ - k[:, None])
        quals[low] = rng.integers(2, 9, int(low.sum()), dtype=np.uint8)
    lens = np.array([len(c) for c in enc])[tmpl]
    return dict(n_groups=n_regions, group_read_off=(np.arange(n_regions + 1) * PER_REGION).astype(np.uint32),
                group_span_start=start.astype(np.uint64), group_span_end=(start + SPAN).astype(np.uint64),
                read_pos=pos_aligned.astype(np.int64), read_flags=flags, read_mapq=rng.integers(20, 61, n).astype(np.uint8),
                read_mpos=mpos.astype(np.int64), read_isize=isize.astype(np.int64),
                read_cigar_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32),
                read_cigar=np.concatenate([enc[t] for t in tmpl]).astype(np.uint32), read_off=(np.arange(n + 1) * READ).astype(np.uint32),
                read_bases=np.ascontiguousarray(bases.reshape(-1)), read_quals=np.ascontiguousarray(quals.reshape(-1)), mate_index=mate,
                out_cigar_off=np.concatenate([[0], np.cumsum(lens + 2)]).astype(np.uint64))


def trace_table(directory, out):
    """per finalize kernel of a rocprofv3 kernel trace (CSV): launches, median and minimum of the last ten, in ns"""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "finalize_" in r["Kernel_Name"]:
                rows.setdefault(r["Kernel_Name"], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    lines = ["== rocprofv3 --kernel-trace --stats -- python tools/finalize_bench.py --steps 10 --warmup 2 : 1 024 regions x 128 reads of 150 bases ==",
             "%-70s %6s %12s %12s   (the last ten launches)" % ("kernel", "calls", "median_ns", "min_ns")]
    for name, d in sorted(rows.items(), key=lambda kv: min(kv[1])[0]):
        last = [x[1] for x in sorted(d)][-10:]
        lines.append("%-70s %6d %12d %12d" % (name[:70], len(d), int(np.median(last)), min(last)))
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text, end="")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regions", type=int, default=1024)
    ap.add_argument("--out")
    ap.add_argument("--trace")
    ap.add_argument("--trace-out")
    a = ap.parse_args()
    if a.trace:
        return trace_table(a.trace, a.trace_out)
    from lorikeet_amd import HipPairHMMEngine, finalize
    packed = workload(a.regions)
    eng = HipPairHMMEngine(0)
    call = lambda: finalize.finalize_reads(eng, packed, min_tail_quality=9)  # noqa: E731
    for _ in range(a.warmup):
        call()
    ts = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res = call()
        ts.append(time.perf_counter() - t0)
    eng.close()
    med = float(np.median(ts))
    n = len(res.read_status)
    staged = sum(v.nbytes for v in packed.values() if isinstance(v, np.ndarray))
    returned = sum(getattr(res, k).nbytes for k in finalize.OUTPUTS)
    out = {"tool": "finalize_bench", "steps": a.steps, "warmup": a.warmup, "regions": a.regions, "reads": n, "read_length": READ,
           "kept": int(res.keep.sum()), "negative_status": int((res.read_status < 0).sum()), "emptied": int(res.out_unmapped.sum()),
           "clipped": int((res.clip_len != READ).sum()), "bases_with_changed_quality": int((res.out_quals != packed["read_quals"]).sum()),
           "reads_with_changed_quality": int((res.out_quals != packed["read_quals"]).reshape(n, READ).any(1).sum()),
           "staged_mb": round(staged / 1e6, 1), "returned_mb": round(returned / 1e6, 1),
           "call_ms_median": round(med * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3), "reads_per_s": round(n / med)}
    line = json.dumps(out)
    if a.out:
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
