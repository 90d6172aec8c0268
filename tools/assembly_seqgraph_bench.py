"""phmm_assembly_seqgraph on the graphs of assembly_graph_bench's workload -- 1 024 regions x 128 reads of 150 bases, k = {10, 25},
2 048 graphs as phmm_assembly_graph returns them -- after phmm_assembly_prune's CHAINS step with prune factor 2, dangling-end
recovery and the CONNECT step: ten calls with the capacities known, after warm-up; prints one JSON line: vertices, edges and
bytes in and out, the chains zipped, the call on the host clock (median and min) and the bytes staged and returned.  A call that
asks for the sizes first does the same work twice.  Beside it, for scale and not as a gate, the same work done by a plain
single-threaded C++ loop over the same arrays (tools/assembly_seqgraph_host.cpp, one run), whose every output array must equal
the device's.  The kernels' own time comes from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/assembly_seqgraph_bench.py --no-host`.
usage: python tools/assembly_seqgraph_bench.py [--steps K] [--warmup W] [--regions N] [--factor F] [--no-host]"""
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

COMPARED = tuple(n for n in assembly.SEQ_OUTPUTS)


def host_loop(regions, g, after, final):
    """(seconds, outputs) of tools/libassembly_seqgraph_host.so on the arrays sequence_graph was given"""
    lib = C.CDLL(os.path.join(ROOT, "tools", "libassembly_seqgraph_host.so"))
    a = regions if isinstance(regions, dict) else assembly.pack(regions)
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    u8 = lambda x: np.ascontiguousarray(x, np.uint8).reshape(-1)  # noqa: E731
    gone = lambda s: u8((np.asarray(s) & assembly._GONE) != 0)  # noqa: E731
    ins = [u32(a["region_ref_off"]), u8(a["ref_bases"]), u32(a["region_read_off"]), u32(a["read_off"]), u8(a["read_bases"]), u32(g["k"]),
           u32(after["vertex_off"]), u32(after["edge_off"]), u32(g["vertex_seq"]), u32(g["vertex_pos"]), u32(after["edge_src"]), u32(after["edge_dst"]),
           u8(after["edge_is_ref"]), u32(after["edge_multiplicity"]), u32(after["new_vertex_off"]), u8(after["new_vertex_kmer"]),
           gone(final["vertex_state"]), gone(final["edge_state"]), u32(final["graph_flags"])]
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    sizes = np.zeros(3, np.uint32)
    n_graphs, n_v = len(ins[6]) - 1, int(ins[6][-1])
    t0 = time.perf_counter()
    lib.assembly_seqgraph_host(C.c_uint32(len(ins[0]) - 1), *[p(x) for x in ins[:5]], C.c_uint32(len(ins[5])), *[p(x) for x in ins[5:]], p(sizes))
    sec = time.perf_counter() - t0
    nv, ne, nb = (int(x) for x in sizes)
    o = dict(counts=np.zeros(9 * n_graphs, np.uint32))
    o.update({name: np.zeros(n_graphs + 1, np.uint32) for name in assembly.SEQ_OFFSETS})
    o.update({name: np.zeros(nv, np.uint32) for name in assembly.SEQ_VERTEX})
    o.update(seq_edge_src=np.zeros(ne, np.uint32), seq_edge_dst=np.zeros(ne, np.uint32), seq_edge_is_ref=np.zeros(ne, np.uint8),
             seq_edge_multiplicity=np.zeros(ne, np.uint32), seq_bases=np.zeros(nb, np.uint8), vertex_to_seq=np.zeros(n_v, np.uint32))
    lib.assembly_seqgraph_host_copy(*[p(x) for x in o.values()])
    counts = o.pop("counts").reshape(n_graphs, 9)
    for i, name in enumerate(assembly.SEQ_GRAPH):
        o[name] = counts[:, i].copy()
    return sec, o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
    pruned = assembly.prune_graph(eng, g, factor, ops=_lib.PHMM_PRUNE_OP_CHAINS)
    cyclic = pruned["graph_flags"] & _lib.PHMM_PRUNE_HAS_CYCLE != 0
    masks = dict(vertex_absent=(pruned["vertex_state"] & assembly._GONE) != 0, edge_absent=(pruned["edge_state"] & assembly._GONE) != 0)
    for o in np.flatnonzero(cyclic):                               # (a cyclic graph is the caller's to drop: it goes in emptied)
        masks["vertex_absent"][g["vertex_off"][o]:g["vertex_off"][o + 1]] = True
        masks["edge_absent"][g["edge_off"][o]:g["edge_off"][o + 1]] = True
    rec = assembly.recover_dangling_ends(eng, w, g, masks, factor)
    after = assembly.apply_recovery(g, masks, rec)
    final = assembly.prune_graph(eng, after, factor, ops=_lib.PHMM_PRUNE_OP_CONNECT, vertex_absent=after["vertex_absent"], edge_absent=after["edge_absent"])
    r = assembly.sequence_graph(eng, w, g, after, final)
    need = r["required"].copy()
    t, staged = [], 0
    for i in range(a.warmup + a.steps):
        before = eng.stat("staged_bytes")
        t0 = time.perf_counter()
        again = assembly.sequence_graph(eng, w, g, after, final, capacity=need)
        if i >= a.warmup:
            t.append(time.perf_counter() - t0)
        staged = eng.stat("staged_bytes") - before
        for name in assembly.SEQ_OUTPUTS:
            assert again[name].tobytes() == r[name].tobytes(), "two runs disagree: " + name
    present_v = int(((final["vertex_state"] & assembly._GONE) == 0).sum())
    present_e = int(((final["edge_state"] & assembly._GONE) == 0).sum())
    status, counts = np.unique(r["seq_status"], return_counts=True)
    out = {"tool": "assembly_seqgraph_bench", "regions": a.regions, "reads_per_region": READS, "read_bases": READ_LEN, "reference_bases": REF_LEN,
           "k": list(KS), "samples": SAMPLES, "prune_factor": a.factor, "steps": a.steps, "graphs": n_graphs, "graphs_cyclic_dropped": int(cyclic.sum()),
           "seq_status": {("ok", "skipped", "reference_fails")[int(s)]: int(n) for s, n in zip(status, counts)},
           "vertices_in": int(after["vertex_off"][-1]), "edges_in": int(after["edge_off"][-1]), "vertices_in_present": present_v,
           "edges_in_present": present_e, "bytes_in": int(len(w["ref_bases"]) + len(w["read_bases"]) + after["new_vertex_kmer"].size),
           "vertices_out": int(need[0]), "edges_out": int(need[1]), "bytes_out": int(need[2]), "chains_zipped": int(r["n_chains_zipped"].sum()),
           "longest_chain": int(r["seq_vertex_n_merged"].max(initial=0)), "removed_clean": int(r["n_removed_clean"].sum()),
           "removed_unconnected": int(r["n_removed_unconnected"].sum()), "call_ms_median": round(float(np.median(t)) * 1e3, 3),
           "call_ms_min": round(min(t) * 1e3, 3), "staged_in_bytes": int(staged),
           "returned_bytes": int(sum(r[name].nbytes for name in assembly.SEQ_OUTPUTS)),
           "returned_bytes_without_vertex_to_seq": int(sum(r[name].nbytes for name in assembly.SEQ_OUTPUTS if name != "vertex_to_seq"))}
    if not a.no_host:
        sec, h = host_loop(w, g, after, final)
        for name in COMPARED:
            assert h[name].shape == r[name].shape and np.array_equal(h[name], r[name]), "the host loop and the device disagree: " + name
        out["host_loop_ms"] = round(sec * 1e3, 1)
        out["host_loop_equal"] = list(COMPARED)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
