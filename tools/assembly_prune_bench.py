"""phmm_assembly_prune on the graphs of assembly_graph_bench's workload -- 1 024 regions x 128 reads of 150 bases, k = {10, 25},
2 048 graphs as phmm_assembly_graph returns them -- with prune factor 2 and both steps: ten calls after warm-up; prints one JSON
line: the graphs' sizes, what the call removes, the call on the host clock (median and min), the bytes staged and returned, and
beside it the same work done by a plain single-threaded C++ loop over the same arrays (tools/assembly_prune_host.cpp, one run),
whose flags, reference ends, counts and state arrays must equal the device's.  No gate.  The kernel's own time comes from ONE
run under `rocprofv3 --kernel-trace --stats -- python tools/assembly_prune_bench.py --no-host`.
usage: python tools/assembly_prune_bench.py [--steps K] [--warmup W] [--regions N] [--factor F] [--no-host]"""
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
from assembly_graph_bench import SAMPLES  # noqa: E402
from assembly_kmers_bench import KS, READ_LEN, READS, REF_LEN, workload  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, _lib, assembly  # noqa: E402

COMPARED = ("graph_flags", "n_chains", "n_chains_removed", "n_vertices_left", "n_edges_left", "ref_source", "ref_sink", "edge_state", "vertex_state")


def host_loop(g, factor, ops):
    lib = C.CDLL(os.path.join(ROOT, "tools", "libassembly_prune_host.so"))
    n_graphs = len(g["vertex_off"]) - 1
    o = {name: np.zeros(n_graphs, np.uint32) for name in COMPARED[:7]}
    o.update(edge_state=np.zeros(len(g["edge_src"]), np.uint8), vertex_state=np.zeros(int(g["vertex_off"][-1]), np.uint8))
    p = lambda x: x.ctypes.data_as(_lib.u8p if x.dtype == np.uint8 else _lib.u32p)  # noqa: E731
    t0 = time.perf_counter()
    lib.assembly_prune_host(C.c_uint32(n_graphs), p(g["vertex_off"]), p(g["edge_off"]), p(g["edge_src"]), p(g["edge_dst"]), p(g["edge_is_ref"]),
                            p(g["edge_pruning_multiplicity"]), C.c_uint32(ops), p(factor), *[p(o[name]) for name in COMPARED])
    return time.perf_counter() - t0, o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=1024)
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    w = workload(a.regions)
    samples = (np.arange(a.regions * READS) % READS // (READS // SAMPLES)).astype(np.uint32)
    eng = HipPairHMMEngine(0)
    g = assembly.assembly_graph(eng, w, KS, 10, read_sample=samples, planes=False)
    n_graphs = len(g["vertex_off"]) - 1
    factor = np.full(n_graphs, a.factor, np.uint32)
    t, staged, r = [], 0, None
    for i in range(a.warmup + a.steps):
        before = eng.stat("staged_bytes")
        t0 = time.perf_counter()
        r = assembly.prune_graph(eng, g, factor)
        if i >= a.warmup:
            t.append(time.perf_counter() - t0)
        staged = eng.stat("staged_bytes") - before
    gone = _lib.PHMM_PRUNE_REMOVED_CHAINS | _lib.PHMM_PRUNE_REMOVED_CONNECT
    out = {"tool": "assembly_prune_bench", "regions": a.regions, "reads_per_region": READS, "read_bases": READ_LEN, "reference_bases": REF_LEN,
           "k": list(KS), "samples": SAMPLES, "prune_factor": a.factor, "steps": a.steps, "graphs": n_graphs, "vertices": int(g["vertex_off"][-1]),
           "edges": int(g["edge_off"][-1]), "chains": int(r["n_chains"].sum()), "chains_removed": int(r["n_chains_removed"].sum()),
           "edges_removed_chains": int((r["edge_state"] & _lib.PHMM_PRUNE_REMOVED_CHAINS != 0).sum()),
           "edges_removed_connect": int((r["edge_state"] & _lib.PHMM_PRUNE_REMOVED_CONNECT != 0).sum()),
           "vertices_removed": int((r["vertex_state"] & gone != 0).sum()), "graphs_with_cycle": int((r["graph_flags"] & _lib.PHMM_PRUNE_HAS_CYCLE != 0).sum()),
           "graphs_without_ref_ends": int((r["graph_flags"] & _lib.PHMM_PRUNE_NO_REF_ENDS != 0).sum()),
           "dangling_tails": int((r["vertex_state"] & _lib.PHMM_PRUNE_DANGLING_TAIL != 0).sum()),
           "dangling_heads": int((r["vertex_state"] & _lib.PHMM_PRUNE_DANGLING_HEAD != 0).sum()),
           "call_ms_median": round(float(np.median(t)) * 1e3, 3), "call_ms_min": round(min(t) * 1e3, 3), "staged_in_bytes": int(staged),
           "returned_bytes": int(sum(r[name].nbytes for name in assembly.PRUNE_OUTPUTS))}
    if not a.no_host:
        sec, h = host_loop(g, factor, assembly.PRUNE_ALL)
        for name in COMPARED:
            assert np.array_equal(h[name], r[name]), "the host loop and the device disagree: " + name
        out["host_loop_ms"] = round(sec * 1e3, 1)
        out["host_loop_equal"] = list(COMPARED)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
