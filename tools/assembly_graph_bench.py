"""phmm_assembly_graph on assembly_kmers_bench's workload -- 1 024 regions x 128 reads of 150 bases, each region over a 500-base
reference, k = {10, 25}, each region's reads dealt to 16 samples in blocks of eight, so that
the threading order is the input's and the host loop, which knows one sample, threads alike -- ten calls after warm-up with the vertex planes and ten
without, each the size call and the fill call; prints one JSON line: the graphs' sizes summed, the two calls together on the
host clock (median and min), the size call alone, the bytes staged and returned, and beside it the same graphs built by a plain
single-threaded C++ loop over the same arrays with one sample (tools/assembly_graph_host.cpp, one run), whose vertices, edges
and summed multiplicities must equal the device's.  No gate.  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/assembly_graph_bench.py --no-host`.
usage: python tools/assembly_graph_bench.py [--steps K] [--warmup W] [--regions N] [--no-host]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from assembly_kmers_bench import KS, READ_LEN, READS, REF_LEN, workload  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, _lib, assembly  # noqa: E402

SAMPLES = 16


def host_loop(a, ks, min_q):
    lib = C.CDLL(os.path.join(ROOT, "tools", "libassembly_graph_host.so"))
    n_regions = len(a["region_ref_off"]) - 1
    nv, ne = np.zeros((len(ks), n_regions), np.uint32), np.zeros((len(ks), n_regions), np.uint32)
    mult = np.zeros((len(ks), n_regions), np.uint64)
    k = np.asarray(ks, np.uint32)
    p = lambda x, t: x.ctypes.data_as(t)  # noqa: E731
    t0 = time.perf_counter()
    lib.assembly_graph_host(C.c_uint32(n_regions), p(a["region_ref_off"], _lib.u32p), p(a["ref_bases"], _lib.u8p), p(a["region_read_off"], _lib.u32p),
                            p(a["read_off"], _lib.u32p), p(a["read_bases"], _lib.u8p), p(a["read_quals"], _lib.u8p), C.c_uint32(len(ks)),
                            p(k, _lib.u32p), C.c_uint32(min_q), p(nv, _lib.u32p), p(ne, _lib.u32p), p(mult, _lib.u64p))
    return time.perf_counter() - t0, nv, ne, mult


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=1024)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    w = workload(a.regions)
    samples = (np.arange(a.regions * READS) % READS // (READS // SAMPLES)).astype(np.uint32)
    eng = HipPairHMMEngine(0)
    times, res, staged = {}, {}, 0
    for planes in (True, False):
        t = []
        for i in range(a.warmup + a.steps):
            before = eng.stat("staged_bytes")
            t0 = time.perf_counter()
            res[planes] = assembly.assembly_graph(eng, w, KS, 10, read_sample=samples, planes=planes)
            if i >= a.warmup:
                t.append(time.perf_counter() - t0)
            staged = eng.stat("staged_bytes") - before
        times[planes] = t
    r = res[True]
    size_call = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        try:
            assembly.assembly_graph(eng, w, KS, 10, read_sample=samples, planes=False, capacity=(0, 0, 0))
        except assembly.PhmmError as e:
            assert e.code == _lib.PHMM_ERR_EVENT_CAPACITY
        size_call.append(time.perf_counter() - t0)
    returned = {p: int(sum(v.nbytes for name, v in res[p].items() if name in assembly.GRAPH_OUTPUTS and v is not None)) for p in (True, False)}
    for name in assembly.GRAPH_OUTPUTS[:-2]:
        assert np.array_equal(res[True][name], res[False][name]), name
    out = {"tool": "assembly_graph_bench", "regions": a.regions, "reads_per_region": READS, "read_bases": READ_LEN, "reference_bases": REF_LEN,
           "k": list(KS), "samples": SAMPLES, "steps": a.steps, "positions": int(len(w["ref_bases"]) + len(w["read_bases"])),
           "vertices": int(r["n_vertices"].sum()), "edges": int(r["n_edges"].sum()), "ref_path": int(r["n_ref_path"].sum()),
           "multiplicity": int(r["edge_multiplicity"].sum(dtype=np.uint64)), "edges_pruning_above_1": int((r["edge_pruning_multiplicity"] > 1).sum()),
           "call_ms_median": round(float(np.median(times[True])) * 1e3, 3), "call_ms_min": round(min(times[True]) * 1e3, 3),
           "call_no_planes_ms_median": round(float(np.median(times[False])) * 1e3, 3), "call_no_planes_ms_min": round(min(times[False]) * 1e3, 3),
           "size_call_ms_median": round(float(np.median(size_call)) * 1e3, 3),
           "staged_in_bytes": int(staged), "returned_bytes": returned[True], "returned_no_planes_bytes": returned[False]}
    if not a.no_host:
        sec, nv, ne, mult = host_loop(w, KS, 10)
        per_graph = np.add.reduceat(r["edge_multiplicity"].astype(np.uint64), r["edge_off"][:-1].astype(np.int64)) if len(r["edge_multiplicity"]) else mult.reshape(-1) * 0
        per_graph = np.where(r["n_edges"].reshape(-1) > 0, per_graph, 0)
        assert np.array_equal(nv, r["n_vertices"]) and np.array_equal(ne, r["n_edges"]) and np.array_equal(mult.reshape(-1), per_graph), \
            "the host loop and the device disagree"
        out["host_loop_ms"] = round(sec * 1e3, 1)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
