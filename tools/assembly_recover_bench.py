"""phmm_assembly_recover on the graphs of assembly_graph_bench's workload -- 1 024 regions x 128 reads of 150 bases, k = {10, 25},
2 048 graphs as phmm_assembly_graph returns them -- after phmm_assembly_prune's CHAINS step with prune factor 2: ten calls with
the capacities known, after warm-up; prints one JSON line: the ends found and recovered, their statuses, the distribution of
n_rounds, the new edges and vertices, the call on the host clock (median and min) and the bytes staged and returned.  A call that
asks for the sizes first does the same work twice.  Beside it, for scale and not as a gate, the same work done by a plain
single-threaded C++ loop over the same arrays (tools/assembly_recover_host.cpp, one run), whose every output array must equal the
device's (n_rounds, which only the device's schedule has, aside).  The kernel's own time comes from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/assembly_recover_bench.py --no-host`.
usage: python tools/assembly_recover_bench.py [--steps K] [--warmup W] [--regions N] [--factor F] [--no-host]"""
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

STATUS = ("no_path", "loop", "at_ref_end", "too_short", "cigar_not_okay", "too_few_matching", "whole_insertion", "too_many_mismatches",
          "cannot_push_ref", "cannot_extend", "merged", "no_merge_point", "reference_fails")


COMPARED = tuple(n for n in assembly.RECOVER_OUTPUTS if n != "n_rounds")


def host_loop(regions, g, masks, factor, need, ops=assembly.RECOVER_ALL, min_dangling_branch_length=4, min_matching_bases=-1,
              max_mismatches_in_dangling_head=-1, sw_parameters=(25, -50, -110, -6)):
    """(seconds, outputs) of tools/libassembly_recover_host.so on the arrays recover_dangling_ends was given; need: the three sizes"""
    lib = C.CDLL(os.path.join(ROOT, "tools", "libassembly_recover_host.so"))
    a = regions if isinstance(regions, dict) else assembly.pack(regions)
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    k, vertex_off, edge_off = u32(g["k"]), u32(g["vertex_off"]), u32(g["edge_off"])
    n_regions = len(a["region_ref_off"]) - 1
    n_graphs = len(vertex_off) - 1
    # where a vertex's bytes start in [reference bases | read bases]: the caller's arithmetic, outside the timed part
    bases = np.concatenate([np.asarray(a["ref_bases"], np.uint8), np.asarray(a["read_bases"], np.uint8)])
    seq, pos = u32(g["vertex_seq"]).astype(np.int64), u32(g["vertex_pos"]).astype(np.int64)
    region_of_vertex = np.repeat(np.arange(n_graphs) % max(n_regions, 1), np.diff(vertex_off.astype(np.int64)))
    read = np.asarray(a["region_read_off"], np.int64)[region_of_vertex] + seq - 1
    read_off = np.asarray(a["read_off"], np.int64)
    start = np.where(seq == 0, np.asarray(a["region_ref_off"], np.int64)[region_of_vertex],
                     len(a["ref_bases"]) + read_off[np.clip(read, 0, max(len(read_off) - 2, 0))] if len(read_off) > 1 else 0)
    vertex_base = u32(start + pos)
    E, k_max = int(edge_off[-1]), int(k.max()) if len(k) else 0
    va = np.ascontiguousarray(masks["vertex_absent"], np.uint8) if masks is not None else None
    ea = np.ascontiguousarray(masks["edge_absent"], np.uint8) if masks is not None else None
    need = u32(need)
    o = dict(counts=np.zeros(6 * n_graphs, np.uint32), end_off=np.zeros(n_graphs + 1, np.uint32), new_edge_off=np.zeros(n_graphs + 1, np.uint32),
             new_vertex_off=np.zeros(n_graphs + 1, np.uint32))
    o.update({name: np.zeros(int(need[0]) * (4 if name == "end_cigar" else 1), np.uint32) for name in assembly.RECOVER_END})
    o.update({name: np.zeros(int(need[1]), np.uint32) for name in assembly.RECOVER_EDGE})
    o.update(new_vertex_kmer=np.zeros(int(need[2]) * k_max, np.uint8), edge_removed=np.zeros(E, np.uint8))
    p = lambda x: None if x is None else x.ctypes.data_as(_lib.u8p if x.dtype == np.uint8 else _lib.u32p)  # noqa: E731
    weights = np.asarray(sw_parameters, np.int32)
    factor = u32(factor)
    edges = [u32(g["edge_src"]), u32(g["edge_dst"]), np.ascontiguousarray(g["edge_is_ref"], np.uint8).reshape(-1), u32(g["edge_multiplicity"]),
             u32(g["edge_pruning_multiplicity"])]
    t0 = time.perf_counter()
    rc = lib.assembly_recover_host(C.c_uint32(n_graphs), C.c_uint32(n_regions), p(k), p(bases), p(vertex_base), p(vertex_off), p(edge_off), *[p(x) for x in edges],
                                   p(va), p(ea), p(factor), C.c_uint32(ops), C.c_int32(min_dangling_branch_length), C.c_int32(min_matching_bases),
                                   C.c_int32(max_mismatches_in_dangling_head), weights.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(k_max), p(need),
                                   p(o["counts"]), p(o["end_off"]), p(o["new_edge_off"]), p(o["new_vertex_off"]), *[p(o[name]) for name in assembly.RECOVER_END],
                                   *[p(o[name]) for name in assembly.RECOVER_EDGE], p(o["new_vertex_kmer"]), p(o["edge_removed"]))
    sec = time.perf_counter() - t0
    assert rc == 0, "the host loop made more than the sizes allow"
    counts = o.pop("counts").reshape(n_graphs, 6)
    for i, name in enumerate(assembly.RECOVER_GRAPH[:6]):
        o[name] = counts[:, i].copy()
    o["end_cigar"] = o["end_cigar"].reshape(-1, 4)
    o["new_vertex_kmer"] = o["new_vertex_kmer"].reshape(-1, k_max) if k_max else o["new_vertex_kmer"].reshape(0, 0)
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
    r = assembly.recover_dangling_ends(eng, w, g, masks, factor)
    need = r["required"].copy()
    t, staged = [], 0
    for i in range(a.warmup + a.steps):
        before = eng.stat("staged_bytes")
        t0 = time.perf_counter()
        again = assembly.recover_dangling_ends(eng, w, g, masks, factor, capacity=need)
        if i >= a.warmup:
            t.append(time.perf_counter() - t0)
        staged = eng.stat("staged_bytes") - before
        for name in assembly.RECOVER_OUTPUTS:
            assert again[name].tobytes() == r[name].tobytes(), "two runs disagree: " + name
    rounds, counts = np.unique(r["n_rounds"], return_counts=True)
    out = {"tool": "assembly_recover_bench", "regions": a.regions, "reads_per_region": READS, "read_bases": READ_LEN, "reference_bases": REF_LEN,
           "k": list(KS), "samples": SAMPLES, "prune_factor": a.factor, "steps": a.steps, "graphs": n_graphs, "graphs_cyclic_dropped": int(cyclic.sum()),
           "vertices": int(g["vertex_off"][-1]), "edges": int(g["edge_off"][-1]), "tails": int(r["n_tails"].sum()),
           "tails_recovered": int(r["n_tails_recovered"].sum()), "heads": int(r["n_heads"].sum()), "heads_recovered": int(r["n_heads_recovered"].sum()),
           "new_edges": int(r["n_new_edges"].sum()), "new_vertices": int(r["n_new_vertices"].sum()), "edges_removed": int(r["edge_removed"].sum()),
           "end_status": {STATUS[int(s)]: int(n) for s, n in zip(*np.unique(r["end_status"], return_counts=True))},
           "rounds": {str(int(x)): int(n) for x, n in zip(rounds, counts)}, "longest_alt": int(r["end_alt_len"].max(initial=0)),
           "longest_ref": int(r["end_ref_len"].max(initial=0)), "call_ms_median": round(float(np.median(t)) * 1e3, 3), "call_ms_min": round(min(t) * 1e3, 3),
           "staged_in_bytes": int(staged), "returned_bytes": int(sum(r[name].nbytes for name in assembly.RECOVER_OUTPUTS))}
    if not a.no_host:
        sec, h = host_loop(w, g, masks, factor, need)
        for name in COMPARED:
            assert h[name].shape == r[name].shape and np.array_equal(h[name], r[name]), "the host loop and the device disagree: " + name
        out["host_loop_ms"] = round(sec * 1e3, 1)
        out["host_loop_equal"] = list(COMPARED)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
