"""phmm_assembly_best_paths on two workloads.  A: the sequence graphs assembly_seqgraph_bench produces -- 1 024 regions x 128
reads of 150 bases, k = {10, 25}, 2 048 graphs after CHAINS with prune factor 2, recovery, CONNECT and the zip -- mostly one to
three vertices: the floor of the call.  B: 2 048 synthetic graphs of ten bubbles (1 024 paths each) at max_paths 128.  Ten calls
each with the capacities known, after warm-up; prints one JSON line: graphs, paths, path edges and bytes out, the call on the
host clock (median and min) and the bytes staged and returned.  A call that asks for the sizes first does the same work twice.
Beside it, for scale and not as a gate, the same work as a plain single-threaded C++ loop over the same arrays
(tools/assembly_paths_host.cpp, one run), whose every output array must equal the device's.  The kernels' own time comes from
ONE run under `rocprofv3 --kernel-trace --stats -- python tools/assembly_paths_bench.py --no-host`.
usage: python tools/assembly_paths_bench.py [--steps K] [--warmup W] [--regions N] [--no-host]"""
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
from assembly_kmers_bench import KS, READS, workload  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, _lib, assembly  # noqa: E402

COMPARED = tuple(n for n in assembly.PATHS_OUTPUTS if n != "path_first_equal")


def host_loop(seq, max_paths, max_nodes):
    """(seconds, outputs) of tools/libassembly_paths_host.so on the arrays best_paths was given"""
    lib = C.CDLL(os.path.join(ROOT, "tools", "libassembly_paths_host.so"))
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    u8 = lambda x: np.ascontiguousarray(x, np.uint8).reshape(-1)  # noqa: E731
    n_graphs = len(seq["seq_vertex_off"]) - 1
    status = u32(seq["seq_status"]) if "seq_status" in seq else np.zeros(n_graphs, np.uint32)
    ins = [u32(seq["seq_vertex_off"]), u32(seq["seq_edge_off"]), u32(seq["seq_base_off"]), u32(seq["seq_vertex_base_off"]), u32(seq["seq_edge_src"]),
           u32(seq["seq_edge_dst"]), u8(seq["seq_edge_is_ref"]), u32(seq["seq_edge_multiplicity"]), u8(seq["seq_bases"]), status,
           u32(seq["seq_ref_source"]), u32(seq["seq_ref_sink"])]
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    sizes = np.zeros(3, np.uint32)
    t0 = time.perf_counter()
    lib.assembly_paths_host(C.c_uint32(n_graphs), *[p(x) for x in ins], C.c_uint32(max_paths), C.c_uint32(max_nodes), p(sizes))
    sec = time.perf_counter() - t0
    n_p, n_e, n_b = (int(x) for x in sizes)
    o = dict(counts=np.zeros(5 * n_graphs, np.uint32))
    o.update({name: np.zeros(n_graphs + 1, np.uint32) for name in assembly.PATHS_OFFSETS})
    o.update(path_score=np.zeros(n_p, np.float64), path_is_ref=np.zeros(n_p, np.uint8), path_n_edges=np.zeros(n_p, np.uint32), hap_off=np.zeros(n_p + 1, np.uint32),
             path_edges=np.zeros(n_e, np.uint32), hap_bases=np.zeros(n_b, np.uint8), edge_removed=np.zeros(int(ins[1][-1]), np.uint8),
             vertex_removed=np.zeros(int(ins[0][-1]), np.uint8))
    lib.assembly_paths_host_copy(*[p(x) for x in o.values()])
    counts = o.pop("counts").reshape(n_graphs, 5)
    for i, name in enumerate(assembly.PATHS_GRAPH):
        o[name] = counts[:, i].copy()
    return sec, o


def bubbles(n_graphs, n=10):
    """n_graphs graphs of n bubbles in a row, the branch multiplicities varied from graph to graph"""
    vo, eo, bo, vbo, src, dst, ref, mult, bases = [0], [0], [0], [], [], [], [], [], []
    for g in range(n_graphs):
        seqs = [b"AC"]
        for i in range(n):
            a = 3 * i
            seqs += [b"G", b"TT", b"AC"]
            major, minor = 2 + (g + i) % 7, 1 + (g * 3 + i) % 2
            src += [a, a, a + 1, a + 2]
            dst += [a + 1, a + 2, a + 3, a + 3]
            ref += [1, 0, 1, 0]
            mult += [major, minor, major, minor]
        at = 0
        for s in seqs:
            vbo.append(at)
            at += len(s)
        bases.append(b"".join(seqs))
        vo.append(vo[-1] + len(seqs)), eo.append(eo[-1] + 4 * n), bo.append(bo[-1] + at)
    u32 = lambda x: np.asarray(x, np.uint32)  # noqa: E731
    return dict(seq_vertex_off=u32(vo), seq_edge_off=u32(eo), seq_base_off=u32(bo), seq_vertex_base_off=u32(vbo), seq_edge_src=u32(src), seq_edge_dst=u32(dst),
                seq_edge_is_ref=np.asarray(ref, np.uint8), seq_edge_multiplicity=u32(mult), seq_bases=np.frombuffer(b"".join(bases), np.uint8),
                seq_ref_source=np.zeros(n_graphs, np.uint32), seq_ref_sink=np.full(n_graphs, 3 * n, np.uint32))


def measure(eng, seq, max_paths, max_nodes, regions, a):
    r = assembly.best_paths(eng, seq, max_paths, max_nodes, regions=regions)
    need = r["required"].copy()
    t, staged = [], 0
    for i in range(a.warmup + a.steps):
        before = eng.stat("staged_bytes")
        t0 = time.perf_counter()
        again = assembly.best_paths(eng, seq, max_paths, max_nodes, regions=regions, capacity=need)
        if i >= a.warmup:
            t.append(time.perf_counter() - t0)
        staged = eng.stat("staged_bytes") - before
        for name in assembly.PATHS_OUTPUTS:
            if r[name] is not None:
                assert again[name].tobytes() == r[name].tobytes(), "two runs disagree: " + name
    status, counts = np.unique(r["paths_status"], return_counts=True)
    names = ("ok", "skipped", "no_ends", "no_path", "cycles_stay", "weight_range", "budget")
    out = {"graphs": len(r["n_paths"]), "vertices_in": int(seq["seq_vertex_off"][-1]), "edges_in": int(seq["seq_edge_off"][-1]), "bytes_in": int(seq["seq_base_off"][-1]),
           "max_paths": max_paths, "max_nodes_per_graph": max_nodes, "paths_status": {names[int(s)]: int(n) for s, n in zip(status, counts)},
           "paths": int(need[0]), "path_edges": int(need[1]), "haplotype_bytes": int(need[2]), "popped": int(r["n_popped"].sum()),
           "most_paths_in_a_graph": int(r["n_paths"].max(initial=0)), "call_ms_median": round(float(np.median(t)) * 1e3, 3), "call_ms_min": round(min(t) * 1e3, 3),
           "staged_in_bytes": int(staged), "returned_bytes": int(sum(r[name].nbytes for name in assembly.PATHS_OUTPUTS if r[name] is not None))}
    if regions is not None:
        fe = r["path_first_equal"]
        out["paths_equal_to_the_reference"] = int((fe == _lib.PHMM_PATHS_EQUALS_REF).sum())
        out["paths_equal_to_an_earlier_one"] = int((fe < _lib.PHMM_PATHS_EQUALS_REF).sum())
    if not a.no_host:
        sec, h = host_loop(seq, max_paths, max_nodes)
        for name in COMPARED:
            g, w = (x.view(np.uint64) if x.dtype == np.float64 else x for x in (r[name], h[name]))
            assert g.shape == w.shape and np.array_equal(g, w), "the host loop and the device disagree: " + name
        out["host_loop_ms"] = round(sec * 1e3, 1)
        out["host_loop_equal"] = list(COMPARED)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--regions", type=int, default=1024)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    w = workload(a.regions)
    samples = (np.arange(a.regions * READS) % READS // (READS // SAMPLES)).astype(np.uint32)
    eng = HipPairHMMEngine(0)
    g = assembly.assembly_graph(eng, w, KS, 10, read_sample=samples, planes=False)
    n_graphs = len(g["vertex_off"]) - 1
    factor = np.full(n_graphs, 2, np.uint32)
    pruned = assembly.prune_graph(eng, g, factor, ops=_lib.PHMM_PRUNE_OP_CHAINS)
    cyclic = pruned["graph_flags"] & _lib.PHMM_PRUNE_HAS_CYCLE != 0
    masks = dict(vertex_absent=(pruned["vertex_state"] & assembly._GONE) != 0, edge_absent=(pruned["edge_state"] & assembly._GONE) != 0)
    for o in np.flatnonzero(cyclic):                               # (a cyclic graph is the caller's to drop: it goes in emptied)
        masks["vertex_absent"][g["vertex_off"][o]:g["vertex_off"][o + 1]] = True
        masks["edge_absent"][g["edge_off"][o]:g["edge_off"][o + 1]] = True
    rec = assembly.recover_dangling_ends(eng, w, g, masks, factor)
    after = assembly.apply_recovery(g, masks, rec)
    final = assembly.prune_graph(eng, after, factor, ops=_lib.PHMM_PRUNE_OP_CONNECT, vertex_absent=after["vertex_absent"], edge_absent=after["edge_absent"])
    seq = assembly.sequence_graph(eng, w, g, after, final)
    regions = dict(region_ref_off=w["region_ref_off"], ref_bases=w["ref_bases"], n_k=len(KS))
    out = {"tool": "assembly_paths_bench", "regions": a.regions, "k": list(KS), "steps": a.steps,
           "sequence_graphs": measure(eng, seq, 128, 1 << 16, regions, a), "ten_bubbles": measure(eng, bubbles(2 * a.regions), 128, 1 << 16, None, a)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
