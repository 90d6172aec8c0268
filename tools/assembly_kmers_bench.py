"""phmm_assembly_kmers on finalize_bench's scale -- 1 024 regions x 128 reads of 150 bases, each region over a 500-base reference
(seeded: reads are pieces of the reference with 1 % substitutions, 1 % of the bases below the quality threshold, one read in
eight with an N), k = {10, 25} -- ten calls after warm-up with the id planes and ten without; prints one JSON line: the verdicts
and counts summed, the whole call on the host clock (median and min), the bytes staged and returned, and beside it the same
work as a plain single-threaded C++ loop over the same arrays with std::unordered_set<std::string>
(tools/assembly_kmers_host.cpp, one run), whose counts must equal the device's.  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/assembly_kmers_bench.py --no-host`.
usage: python tools/assembly_kmers_bench.py [--steps K] [--warmup W] [--regions N] [--no-host]
       python tools/assembly_kmers_bench.py --trace <rocprof dir> [--trace-out FILE] [--regions N as traced]   the table of that run's asm_*_kernel times"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lorikeet_amd import HipPairHMMEngine, _lib, assembly  # noqa: E402

READS, READ_LEN, REF_LEN, KS = 128, 150, 500, (10, 25)


def workload(n_regions, seed=2024):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref = acgt[rng.integers(0, 4, (n_regions, REF_LEN))]
    at = rng.integers(0, REF_LEN - READ_LEN + 1, (n_regions, READS))
    reads = ref[np.arange(n_regions)[:, None, None], at[:, :, None] + np.arange(READ_LEN)[None, None, :]].copy()
    sub = rng.random(reads.shape) < 0.01
    reads[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    with_n = rng.random((n_regions, READS)) < 0.125
    reads[with_n, rng.integers(0, READ_LEN, int(with_n.sum()))] = ord("N")
    quals = np.where(rng.random(reads.shape) < 0.01, 5, 30).astype(np.uint8)
    n_reads = n_regions * READS
    return dict(region_ref_off=(np.arange(n_regions + 1) * REF_LEN).astype(np.uint32), ref_bases=np.ascontiguousarray(ref.reshape(-1)),
                region_read_off=(np.arange(n_regions + 1) * READS).astype(np.uint32), read_off=(np.arange(n_reads + 1) * READ_LEN).astype(np.uint32),
                read_bases=np.ascontiguousarray(reads.reshape(-1)), read_quals=np.ascontiguousarray(quals.reshape(-1)))


def host_loop(a, ks, min_q):
    lib = C.CDLL(os.path.join(ROOT, "tools", "libassembly_kmers_host.so"))
    n_regions = len(a["region_ref_off"]) - 1
    nu, tr = np.zeros((len(ks), n_regions), np.uint32), np.zeros((len(ks), n_regions), np.uint32)
    k = np.asarray(ks, np.uint32)
    p = lambda x, t: x.ctypes.data_as(t)  # noqa: E731
    t0 = time.perf_counter()
    lib.assembly_kmers_host(C.c_uint32(n_regions), p(a["region_ref_off"], _lib.u32p), p(a["ref_bases"], _lib.u8p), p(a["region_read_off"], _lib.u32p),
                            p(a["read_off"], _lib.u32p), p(a["read_bases"], _lib.u8p), p(a["read_quals"], _lib.u8p), C.c_uint32(len(ks)),
                            p(k, _lib.u32p), C.c_uint32(min_q), p(nu, _lib.u32p), p(tr, _lib.u32p))
    return time.perf_counter() - t0, nu, tr


def trace_table(directory, out, regions):
    """per kernel of a rocprofv3 kernel trace (CSV) and launch shape (asm_sequence_kernel runs once over the references and once
    over the reads): launches, median and minimum of the last ten, in ns; regions: the --regions of the traced run"""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "asm_" in r["Kernel_Name"]:
                shape = "x".join(str(r.get(c, "?")) for c in ("Grid_Size_X", "Grid_Size_Y", "Workgroup_Size_X"))
                name = r["Kernel_Name"].replace("phmm::(anonymous namespace)::", "").replace("(phmm::AsmParams)", "").replace("(phmm::AsmParams, unsigned int)", "")
                rows.setdefault("%s [%s]" % (name, shape), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    lines = ["== rocprofv3 --kernel-trace --stats -- python tools/assembly_kmers_bench.py --no-host --regions %d : regions x %d reads of %d bases, %d reference bases, k = %s =="
             % (regions, READS, READ_LEN, REF_LEN, list(KS)),
             "%-60s %6s %12s %12s   (the last ten launches; [grid x, grid y, block x])" % ("kernel", "calls", "median_ns", "min_ns")]
    for name, d in sorted(rows.items(), key=lambda kv: min(kv[1])[0]):
        last = [x[1] for x in sorted(d)][-10:]
        lines.append("%-60s %6d %12d %12d" % (name[:60], len(d), int(np.median(last)), min(last)))
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text, end="")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=1024)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--trace-out")
    a = ap.parse_args()
    if a.trace:
        return trace_table(a.trace, a.trace_out, a.regions)
    w = workload(a.regions)
    eng = HipPairHMMEngine(0)
    times, res, staged = {}, {}, 0
    for ids in (True, False):
        t = []
        for i in range(a.warmup + a.steps):
            before = eng.stat("staged_bytes")
            t0 = time.perf_counter()
            res[ids] = assembly.assembly_kmers(eng, w, KS, 10, ids=ids)
            if i >= a.warmup:
                t.append(time.perf_counter() - t0)
            staged = eng.stat("staged_bytes") - before
        times[ids] = t
    r = res[True]
    returned = {ids: int(sum(v.nbytes for name, v in res[ids].items() if name in assembly.OUTPUTS and v is not None)) for ids in (True, False)}
    for name in assembly.OUTPUTS[:7]:
        assert np.array_equal(res[True][name], res[False][name]), name
    out = {"tool": "assembly_kmers_bench", "regions": a.regions, "reads_per_region": READS, "read_bases": READ_LEN, "reference_bases": REF_LEN,
           "k": list(KS), "steps": a.steps, "positions": int(len(w["ref_bases"]) + len(w["read_bases"])),
           "sequences": int(r["n_sequences"].sum()), "non_unique": int(r["n_non_unique"].sum()), "tracked": int(r["n_tracked"].sum()),
           "distinct": int(r["n_distinct"].sum()), "ref_non_unique_verdicts": int((r["flags"] & _lib.PHMM_ASM_REF_NON_UNIQUE != 0).sum()),
           "low_complexity_verdicts": int((r["flags"] & _lib.PHMM_ASM_LOW_COMPLEXITY != 0).sum()),
           "threaded_positions": int((r["read_kmer_flags"] & _lib.PHMM_ASM_KMER_THREADED != 0).sum()),
           "call_ms_median": round(float(np.median(times[True])) * 1e3, 3), "call_ms_min": round(min(times[True]) * 1e3, 3),
           "call_no_ids_ms_median": round(float(np.median(times[False])) * 1e3, 3), "call_no_ids_ms_min": round(min(times[False]) * 1e3, 3),
           "staged_in_bytes": int(staged), "returned_bytes": returned[True], "returned_no_ids_bytes": returned[False]}
    if not a.no_host:
        sec, nu, tr = host_loop(w, KS, 10)
        assert np.array_equal(nu, r["n_non_unique"]) and np.array_equal(tr, r["n_tracked"]), "the host loop and the device disagree"
        out["host_unordered_set_ms"] = round(sec * 1e3, 1)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
