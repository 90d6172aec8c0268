"""The k-mer stage in front of the read-threading graph on the device (phmm_assembly_kmers, include/phmm.h): per region and k
the verdicts that reject a k before a vertex exists, the sizes of the non-unique set and of the vertex map, and per position
whether its k-mer is non-unique, threaded, a threading start, the first of its bytes, with its dense id; and the raw
read-threading graph itself (phmm_assembly_graph): vertices, edges, weights, the reference path, per (k, region); and what the
assembler prunes from it before it looks for paths (phmm_assembly_prune), recovers at its dangling ends (phmm_assembly_recover)
and zips into the sequence graph (phmm_assembly_seqgraph), and the k best haplotype paths of such graphs
(phmm_assembly_best_paths)."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import PhmmError

REGION_OUTPUTS = ("flags", "n_sequences", "n_non_unique", "n_tracked", "n_distinct")
OUTPUTS = REGION_OUTPUTS + ("ref_kmer_flags", "read_kmer_flags", "ref_kmer_id", "read_kmer_id")


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _bytes(x):
    if isinstance(x, str):
        x = x.encode()
    return np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8)


def pack(regions):
    """regions: one (reference, reads) per region, reads a list of (bases, quals); bases as bytes or uint8 arrays.  Returns the
    dense arrays phmm_assembly_kmers takes: region_ref_off, ref_bases, region_read_off, read_off, read_bases, read_quals."""
    region_ref_off, region_read_off, read_off = [0], [0], [0]
    refs, bases, quals = [], [], []
    for ref, reads in regions:
        refs.append(_bytes(ref))
        region_ref_off.append(region_ref_off[-1] + len(refs[-1]))
        for b, q in reads:
            b, q = _bytes(b), _bytes(q)
            if len(b) != len(q):
                raise ValueError("a read's bases and qualities differ in length")
            bases.append(b)
            quals.append(q)
            read_off.append(read_off[-1] + len(b))
        region_read_off.append(len(read_off) - 1)
    cat = lambda xs: np.concatenate(xs).astype(np.uint8) if xs else np.zeros(0, np.uint8)  # noqa: E731
    return dict(region_ref_off=np.asarray(region_ref_off, np.uint32), ref_bases=cat(refs),
                region_read_off=np.asarray(region_read_off, np.uint32), read_off=np.asarray(read_off, np.uint32),
                read_bases=cat(bases), read_quals=cat(quals))


def assembly_kmers(engine, regions, k, min_base_quality=10, read_first=None, read_len=None, ids=True, fill=None):
    """The k-mer stage of the assembler for a batch of regions (phmm_assembly_kmers).  regions: a list of (reference, reads) as
    pack() takes it, or a dict of the dense arrays pack() returns; k: the k values, ascending; read_first / read_len: per-read
    windows (what finalize_reads returns as clip_first / clip_len), None = the whole reads; ids=False: the id planes are not
    asked for (None in the result); fill: a byte the output arrays hold before the call (tests).  Returns a dict of numpy
    arrays: flags, n_sequences, n_non_unique, n_tracked, n_distinct [n_k, n_regions]; ref_kmer_flags [n_k, reference bases],
    read_kmer_flags [n_k, read bases]; ref_kmer_id, read_kmer_id likewise; and the dense input arrays under their names.
    Raises PhmmError."""
    a = regions if isinstance(regions, dict) else pack(regions)
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8)  # noqa: E731
    region_ref_off, region_read_off, read_off = u32(a.get("region_ref_off")), u32(a.get("region_read_off")), u32(a.get("read_off"))
    ref_bases, read_bases, read_quals = u8(a.get("ref_bases")), u8(a.get("read_bases")), u8(a.get("read_quals"))
    read_first, read_len = u32(read_first), u32(read_len)
    k = np.ascontiguousarray(k, np.uint32).reshape(-1)
    n_k = len(k)
    n_regions = next((len(x) - 1 for x in (region_ref_off, region_read_off) if x is not None), 0)
    # (the sizes of the outputs; with an offset array missing or broken -- the library refuses those -- any size will do)
    n_ref = int(region_ref_off[-1]) if n_regions and region_ref_off is not None else 0
    n_read = int(read_off[-1]) if read_off is not None and len(read_off) else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    o = {name: new(n_k * n_regions, np.uint32) for name in REGION_OUTPUTS}
    o.update(ref_kmer_flags=new(n_k * n_ref, np.uint8), read_kmer_flags=new(n_k * n_read, np.uint8),
             ref_kmer_id=new(n_k * n_ref, np.uint32) if ids else None, read_kmer_id=new(n_k * n_read, np.uint32) if ids else None)
    code = engine.lib.phmm_assembly_kmers(
        engine._h, n_regions, _p(region_ref_off, _lib.u32p), _p(ref_bases, _lib.u8p), _p(region_read_off, _lib.u32p),
        _p(read_off, _lib.u32p), _p(read_bases, _lib.u8p), _p(read_quals, _lib.u8p), _p(read_first, _lib.u32p), _p(read_len, _lib.u32p),
        n_k, _p(k, _lib.u32p), int(min_base_quality), *[_p(o[name], _lib.u32p) for name in REGION_OUTPUTS],
        _p(o["ref_kmer_flags"], _lib.u8p), _p(o["read_kmer_flags"], _lib.u8p), _p(o["ref_kmer_id"], _lib.u32p), _p(o["read_kmer_id"], _lib.u32p))
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = {name: v for name, v in o.items() if v is not None}
        raise err
    for name in REGION_OUTPUTS:
        o[name] = o[name].reshape(n_k, n_regions)
    for name, n in (("ref_kmer_flags", n_ref), ("read_kmer_flags", n_read), ("ref_kmer_id", n_ref), ("read_kmer_id", n_read)):
        if o[name] is not None:
            o[name] = o[name].reshape(n_k, n)
    o.update(region_ref_off=region_ref_off, region_read_off=region_read_off, read_off=read_off, k=k)
    return o


GRAPH_SIZES = ("flags", "n_vertices", "n_edges", "n_ref_path")
GRAPH_OFFSETS = ("vertex_off", "edge_off", "ref_path_off")
GRAPH_VERTEX = (("vertex_seq", np.uint32), ("vertex_pos", np.uint32), ("vertex_flags", np.uint8))
GRAPH_EDGE = (("edge_src", np.uint32), ("edge_dst", np.uint32), ("edge_is_ref", np.uint8), ("edge_multiplicity", np.uint32),
              ("edge_pruning_multiplicity", np.uint32))
GRAPH_OUTPUTS = GRAPH_SIZES + GRAPH_OFFSETS + tuple(n for n, _ in GRAPH_VERTEX + GRAPH_EDGE) + ("ref_path", "ref_vertex", "read_vertex")


def assembly_graph(engine, regions, k, min_base_quality=10, read_first=None, read_len=None, read_sample=None, num_pruning_samples=1,
                   planes=True, capacity=None, fill=None, omit=()):
    """The raw read-threading graph of every (k, region) of a batch (phmm_assembly_graph).  regions, k, read_first / read_len as
    assembly_kmers takes them; read_sample: a value per read, None = one sample; planes=False: the vertex planes are not asked
    for (None in the result); capacity: (vertices, edges, ref_path entries), None asks the library first (a call with capacities
    0); fill: a byte the output arrays hold before the call, omit: names of arrays to pass as NULL (tests).  Returns a dict of
    numpy arrays: flags, n_vertices, n_edges, n_ref_path [n_k, n_regions]; vertex_off, edge_off, ref_path_off [n_k * n_regions +
    1]; the per-vertex, per-edge and ref_path arrays cut to what was written; ref_vertex [n_k, reference bases], read_vertex
    [n_k, read bases]; required.  Raises PhmmError; after PHMM_ERR_EVENT_CAPACITY its `required` attribute holds the sizes."""
    a = regions if isinstance(regions, dict) else pack(regions)
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8)  # noqa: E731
    region_ref_off, region_read_off, read_off = u32(a.get("region_ref_off")), u32(a.get("region_read_off")), u32(a.get("read_off"))
    ref_bases, read_bases, read_quals = u8(a.get("ref_bases")), u8(a.get("read_bases")), u8(a.get("read_quals"))
    read_first, read_len, read_sample = u32(read_first), u32(read_len), u32(read_sample)
    k = np.ascontiguousarray(k, np.uint32).reshape(-1)
    n_k = len(k)
    n_regions = next((len(x) - 1 for x in (region_ref_off, region_read_off) if x is not None), 0)
    n_graphs = n_k * n_regions
    n_ref = int(region_ref_off[-1]) if n_regions and region_ref_off is not None else 0
    n_read = int(read_off[-1]) if read_off is not None and len(read_off) else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731

    def call(cap):
        cap = np.ascontiguousarray(cap, np.uint32)
        o = dict(required=new(3, np.uint32))
        o.update({name: new(n_graphs, np.uint32) for name in GRAPH_SIZES})
        o.update({name: new(n_graphs + 1, np.uint32) for name in GRAPH_OFFSETS})
        o.update({name: new(int(cap[0]), dt) if cap[0] else None for name, dt in GRAPH_VERTEX})
        o.update({name: new(int(cap[1]), dt) if cap[1] else None for name, dt in GRAPH_EDGE})
        o.update(ref_path=new(int(cap[2]), np.uint32) if cap[2] else None,
                 ref_vertex=new(n_k * n_ref, np.uint32) if planes else None, read_vertex=new(n_k * n_read, np.uint32) if planes else None)
        for name in omit:
            o[name] = None
        ptr = lambda name: _p(o[name], _lib.u8p if o[name] is not None and o[name].dtype == np.uint8 else _lib.u32p)  # noqa: E731
        code = engine.lib.phmm_assembly_graph(
            engine._h, n_regions, _p(region_ref_off, _lib.u32p), _p(ref_bases, _lib.u8p), _p(region_read_off, _lib.u32p),
            _p(read_off, _lib.u32p), _p(read_bases, _lib.u8p), _p(read_quals, _lib.u8p), _p(read_first, _lib.u32p), _p(read_len, _lib.u32p),
            _p(read_sample, _lib.u32p), n_k, _p(k, _lib.u32p), int(min_base_quality), int(num_pruning_samples),
            None if "capacity" in omit else _p(cap, _lib.u32p), ptr("required"), *[ptr(name) for name in GRAPH_OUTPUTS])
        return code, o

    if capacity is None:
        code, o = call((0, 0, 0))
        if code == _lib.PHMM_ERR_EVENT_CAPACITY:
            code, o = call(o["required"])
    else:
        code, o = call(capacity)
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.required = None if o["required"] is None else o["required"].copy()
        err.outputs = {name: v for name, v in o.items() if v is not None and name != "required"}
        raise err
    V, E, P = (int(x) for x in o["required"])
    for name in GRAPH_SIZES:
        o[name] = o[name].reshape(n_k, n_regions)
    for names, n in ((GRAPH_VERTEX, V), (GRAPH_EDGE, E), ((("ref_path", np.uint32),), P)):
        for name, dt in names:
            o[name] = np.zeros(0, dt) if o[name] is None else o[name][:n]
    if planes:
        o["ref_vertex"], o["read_vertex"] = o["ref_vertex"].reshape(n_k, n_ref), o["read_vertex"].reshape(n_k, n_read)
    o.update(region_ref_off=region_ref_off, region_read_off=region_read_off, read_off=read_off, k=k)
    return o


PRUNE_GRAPH = ("graph_flags", "n_chains", "n_chains_removed", "n_vertices_left", "n_edges_left", "ref_source", "ref_sink")
PRUNE_OUTPUTS = PRUNE_GRAPH + ("edge_chain", "edge_state", "vertex_state")
PRUNE_ALL = _lib.PHMM_PRUNE_OP_CHAINS | _lib.PHMM_PRUNE_OP_CONNECT


def prune_graph(engine, graph, prune_factor, ops=PRUNE_ALL, vertex_absent=None, edge_absent=None, fill=None):
    """Low-weight chains, orphans, the cycle verdict, the reference ends, the dangling ends and the vertices off every way from
    the reference source to the reference sink, for many graphs (phmm_assembly_prune).  graph: the dict assembly_graph returns,
    or any dict with vertex_off, edge_off, edge_src, edge_dst, edge_is_ref, edge_pruning_multiplicity; prune_factor: one value
    or one per graph; ops: PHMM_PRUNE_OP_* bits; vertex_absent / edge_absent: bytes, nonzero = not in the graph, both or
    neither; fill: a byte the output arrays hold before the call (tests).  Returns a dict of numpy arrays: graph_flags,
    n_chains, n_chains_removed, n_vertices_left, n_edges_left, ref_source, ref_sink [n_graphs]; edge_chain, edge_state [edges];
    vertex_state [vertices].  Raises PhmmError."""
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8).reshape(-1)  # noqa: E731
    vertex_off, edge_off = u32(graph.get("vertex_off")), u32(graph.get("edge_off"))
    edge_src, edge_dst, edge_mult = u32(graph.get("edge_src")), u32(graph.get("edge_dst")), u32(graph.get("edge_pruning_multiplicity"))
    edge_is_ref, vertex_absent, edge_absent = u8(graph.get("edge_is_ref")), u8(vertex_absent), u8(edge_absent)
    n_graphs = next((len(x) - 1 for x in (vertex_off, edge_off) if x is not None and len(x)), 0)
    if prune_factor is not None:
        prune_factor = np.full(n_graphs, prune_factor, np.uint32) if np.ndim(prune_factor) == 0 else u32(prune_factor)
    # (the sizes of the outputs; with an offset array missing or broken -- the library refuses those -- any size will do)
    n_v = int(vertex_off[-1]) if n_graphs and vertex_off is not None else 0
    n_e = int(edge_off[-1]) if n_graphs and edge_off is not None else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    o = {name: new(n_graphs, np.uint32) for name in PRUNE_GRAPH}
    o.update(edge_chain=new(n_e, np.uint32), edge_state=new(n_e, np.uint8), vertex_state=new(n_v, np.uint8))
    code = engine.lib.phmm_assembly_prune(
        engine._h, n_graphs, _p(vertex_off, _lib.u32p), _p(edge_off, _lib.u32p), _p(edge_src, _lib.u32p), _p(edge_dst, _lib.u32p),
        _p(edge_is_ref, _lib.u8p), _p(edge_mult, _lib.u32p), _p(vertex_absent, _lib.u8p), _p(edge_absent, _lib.u8p), int(ops),
        _p(prune_factor, _lib.u32p), *[_p(o[name], _lib.u32p) for name in PRUNE_GRAPH], _p(o["edge_chain"], _lib.u32p),
        _p(o["edge_state"], _lib.u8p), _p(o["vertex_state"], _lib.u8p))
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = o
        raise err
    return o


RECOVER_GRAPH = ("n_tails", "n_tails_recovered", "n_heads", "n_heads_recovered", "n_new_edges", "n_new_vertices", "n_rounds")
RECOVER_OFFSETS = ("end_off", "new_edge_off", "new_vertex_off")
RECOVER_END = ("end_vertex", "end_kind", "end_status", "end_alt_len", "end_ref_len", "end_n_cigar", "end_cigar", "end_edge")
RECOVER_EDGE = ("new_edge_src", "new_edge_dst", "new_edge_multiplicity", "new_edge_pruning_multiplicity")
RECOVER_OUTPUTS = RECOVER_GRAPH + RECOVER_OFFSETS + RECOVER_END + RECOVER_EDGE + ("new_vertex_kmer", "edge_removed")
RECOVER_ALL = _lib.PHMM_RECOVER_OP_TAILS | _lib.PHMM_RECOVER_OP_HEADS
_GONE = _lib.PHMM_PRUNE_ABSENT | _lib.PHMM_PRUNE_REMOVED_CHAINS | _lib.PHMM_PRUNE_REMOVED_CONNECT


def recover_dangling_ends(engine, regions, graph, pruned, prune_factor, ops=RECOVER_ALL, min_dangling_branch_length=4, min_matching_bases=-1,
                          max_mismatches_in_dangling_head=-1, num_pruning_samples=1, sw_parameters=(25, -50, -110, -6), read_first=None,
                          read_len=None, capacity=None, fill=None, omit=()):
    """Dangling-end recovery for many graphs (phmm_assembly_recover): recover_dangling_tails, then recover_dangling_heads.
    regions: what assembly_graph was given (a list of (reference, reads), or pack()'s dict); graph: the dict assembly_graph
    returns (k, vertex_off, edge_off, vertex_seq, vertex_pos and the edge arrays); pruned: the dict prune_graph returns -- its
    vertex_state / edge_state make the absent masks and its graph_flags travel along -- or None for the graph as it is, or a dict
    with vertex_absent / edge_absent; prune_factor: one value or one per graph; read_first / read_len: the windows assembly_graph
    was given; capacity: (ends, new edges, new vertices), None asks the library first (a call with capacities 0); fill: a byte the
    output arrays hold before the call, omit: names of arrays to pass as NULL (tests).  Returns a dict of numpy arrays: n_tails,
    n_tails_recovered, n_heads, n_heads_recovered, n_new_edges, n_new_vertices, n_rounds [n_graphs]; end_off, new_edge_off,
    new_vertex_off [n_graphs + 1]; the per-end and per-new-edge arrays cut to what was written (end_cigar [ends, 4]);
    new_vertex_kmer [new vertices, max k]; edge_removed [edges]; required.  Raises PhmmError; after PHMM_ERR_EVENT_CAPACITY its
    `required` attribute holds the sizes."""
    a = regions if isinstance(regions, dict) else pack(regions)
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8).reshape(-1)  # noqa: E731
    region_ref_off, region_read_off, read_off = u32(a.get("region_ref_off")), u32(a.get("region_read_off")), u32(a.get("read_off"))
    ref_bases, read_bases = u8(a.get("ref_bases")), u8(a.get("read_bases"))
    read_first, read_len = u32(read_first), u32(read_len)
    k = u32(graph.get("k"))
    n_k = 0 if k is None else len(k)
    n_regions = next((len(x) - 1 for x in (region_ref_off, region_read_off) if x is not None), 0)
    n_graphs = n_k * n_regions
    g32 = {name: u32(graph.get(name)) for name in ("vertex_off", "edge_off", "vertex_seq", "vertex_pos", "edge_src", "edge_dst", "edge_multiplicity",
                                                   "edge_pruning_multiplicity")}
    edge_is_ref = u8(graph.get("edge_is_ref"))
    vertex_absent = edge_absent = graph_flags = None
    if pruned is not None:
        if "vertex_state" in pruned:
            vertex_absent, edge_absent = u8((np.asarray(pruned["vertex_state"]) & _GONE) != 0), u8((np.asarray(pruned["edge_state"]) & _GONE) != 0)
        else:
            vertex_absent, edge_absent = u8(pruned.get("vertex_absent")), u8(pruned.get("edge_absent"))
        graph_flags = u32(pruned.get("graph_flags"))
    if prune_factor is not None:
        prune_factor = np.full(n_graphs, prune_factor, np.uint32) if np.ndim(prune_factor) == 0 else u32(prune_factor)
    cfg = _lib.RecoverConfig(int(ops), int(min_dangling_branch_length), int(min_matching_bases), int(max_mismatches_in_dangling_head),
                             int(num_pruning_samples), _lib.SwParameters(*[int(x) for x in sw_parameters]))
    n_e = int(g32["edge_off"][-1]) if n_graphs and g32["edge_off"] is not None and len(g32["edge_off"]) else 0
    k_max = int(k.max()) if n_k else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731

    def call(cap):
        cap = np.ascontiguousarray(cap, np.uint32)
        o = dict(required=new(3, np.uint32))
        o.update({name: new(n_graphs, np.uint32) for name in RECOVER_GRAPH})
        o.update({name: new(n_graphs + 1, np.uint32) for name in RECOVER_OFFSETS})
        o.update({name: new(int(cap[0]) * (4 if name == "end_cigar" else 1), np.uint32) if cap[0] else None for name in RECOVER_END})
        o.update({name: new(int(cap[1]), np.uint32) if cap[1] else None for name in RECOVER_EDGE})
        o.update(new_vertex_kmer=new(int(cap[2]) * k_max, np.uint8) if cap[2] else None, edge_removed=new(n_e, np.uint8))
        for name in omit:
            o[name] = None
        ptr = lambda name: _p(o[name], _lib.u8p if o[name] is not None and o[name].dtype == np.uint8 else _lib.u32p)  # noqa: E731
        code = engine.lib.phmm_assembly_recover(
            engine._h, None if "cfg" in omit else C.byref(cfg), n_regions, _p(region_ref_off, _lib.u32p), _p(ref_bases, _lib.u8p),
            _p(region_read_off, _lib.u32p), _p(read_off, _lib.u32p), _p(read_bases, _lib.u8p), _p(read_first, _lib.u32p), _p(read_len, _lib.u32p),
            n_k, _p(k, _lib.u32p), *[_p(g32[name], _lib.u32p) for name in ("vertex_off", "edge_off", "vertex_seq", "vertex_pos", "edge_src", "edge_dst")],
            _p(edge_is_ref, _lib.u8p), _p(g32["edge_multiplicity"], _lib.u32p), _p(g32["edge_pruning_multiplicity"], _lib.u32p),
            _p(vertex_absent, _lib.u8p), _p(edge_absent, _lib.u8p), _p(graph_flags, _lib.u32p), _p(prune_factor, _lib.u32p),
            None if "capacity" in omit else _p(cap, _lib.u32p), ptr("required"), *[ptr(name) for name in RECOVER_OUTPUTS])
        return code, o

    if capacity is None:
        code, o = call((0, 0, 0))
        if code == _lib.PHMM_ERR_EVENT_CAPACITY:
            code, o = call(o["required"])
    else:
        code, o = call(capacity)
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.required = None if o["required"] is None else o["required"].copy()
        err.outputs = {name: v for name, v in o.items() if v is not None and name != "required"}
        raise err
    n_end, n_edge, n_vertex = (int(x) for x in o["required"])
    for name in RECOVER_END:
        width = 4 if name == "end_cigar" else 1
        o[name] = np.zeros(0, np.uint32) if o[name] is None else o[name][:n_end * width]
    o["end_cigar"] = o["end_cigar"].reshape(-1, 4)
    for name in RECOVER_EDGE:
        o[name] = np.zeros(0, np.uint32) if o[name] is None else o[name][:n_edge]
    o["new_vertex_kmer"] = (np.zeros(0, np.uint8) if o["new_vertex_kmer"] is None else o["new_vertex_kmer"][:n_vertex * k_max]).reshape(n_vertex, k_max)
    return o


def apply_recovery(graph, pruned, recovered):
    """The graphs after recovery, ready for prune_graph(..., ops=PHMM_PRUNE_OP_CONNECT): a dict with vertex_off, edge_off, edge_src,
    edge_dst, edge_is_ref, edge_multiplicity, edge_pruning_multiplicity -- every graph's own elements first, then what
    recover_dangling_ends made for it, in creation order -- the two masks vertex_absent / edge_absent (what pruning removed, the
    edges extensions took out, new edges taken out again), and new_vertex_kmer [new vertices, max k] with new_vertex_off.  graph,
    pruned, recovered: what assembly_graph, prune_graph (or None) and recover_dangling_ends returned."""
    vertex_off, edge_off = np.asarray(graph["vertex_off"], np.int64).reshape(-1), np.asarray(graph["edge_off"], np.int64).reshape(-1)
    nv_off, ne_off = np.asarray(recovered["new_vertex_off"], np.int64), np.asarray(recovered["new_edge_off"], np.int64)
    n_graphs = len(vertex_off) - 1
    if pruned is None:
        va, ea = np.zeros(vertex_off[-1], np.uint8), np.zeros(edge_off[-1], np.uint8)
    elif "vertex_state" in pruned:
        va, ea = ((np.asarray(pruned["vertex_state"]) & _GONE) != 0).astype(np.uint8), ((np.asarray(pruned["edge_state"]) & _GONE) != 0).astype(np.uint8)
    else:
        va, ea = np.asarray(pruned["vertex_absent"], np.uint8).copy(), np.asarray(pruned["edge_absent"], np.uint8).copy()
    ea = ea | (np.asarray(recovered["edge_removed"], np.uint8) != 0)
    new_gone = (np.asarray(recovered["new_edge_src"]) == 0xFFFFFFFF).astype(np.uint8)
    cols = {"edge_src": (np.uint32, recovered["new_edge_src"]), "edge_dst": (np.uint32, recovered["new_edge_dst"]),
            "edge_is_ref": (np.uint8, np.zeros(len(new_gone), np.uint8)), "edge_multiplicity": (np.uint32, recovered["new_edge_multiplicity"]),
            "edge_pruning_multiplicity": (np.uint32, recovered["new_edge_pruning_multiplicity"]), "edge_absent": (np.uint8, new_gone)}
    old = dict(graph, edge_absent=ea)
    out = {name: [] for name in cols}
    out["vertex_absent"] = []
    for g in range(n_graphs):
        e0, e1, n0, n1 = edge_off[g], edge_off[g + 1], ne_off[g], ne_off[g + 1]
        for name, (dt, fresh) in cols.items():
            out[name] += [np.asarray(old[name], dt).reshape(-1)[e0:e1], np.where(new_gone[n0:n1] != 0, 0, np.asarray(fresh, dt)[n0:n1]).astype(dt)
                          if name in ("edge_src", "edge_dst") else np.asarray(fresh, dt)[n0:n1]]
        out["vertex_absent"] += [va[vertex_off[g]:vertex_off[g + 1]], np.zeros(nv_off[g + 1] - nv_off[g], np.uint8)]
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)  # noqa: E731
    res = {name: cat(out[name], cols[name][0] if name in cols else np.uint8) for name in out}
    res["vertex_off"] = (vertex_off + nv_off).astype(np.uint32)
    res["edge_off"] = (edge_off + ne_off).astype(np.uint32)
    res["new_vertex_kmer"], res["new_vertex_off"] = recovered["new_vertex_kmer"], np.asarray(recovered["new_vertex_off"], np.uint32)
    if "k" in graph:
        res["k"] = graph["k"]
    return res


SEQ_GRAPH = ("seq_status", "n_seq_vertices", "n_seq_edges", "n_seq_bases", "n_chains_zipped", "n_removed_clean", "n_removed_unconnected",
             "seq_ref_source", "seq_ref_sink")
SEQ_OFFSETS = ("seq_vertex_off", "seq_edge_off", "seq_base_off")
SEQ_VERTEX = ("seq_vertex_base_off", "seq_vertex_first", "seq_vertex_n_merged")
SEQ_EDGE = (("seq_edge_src", np.uint32), ("seq_edge_dst", np.uint32), ("seq_edge_is_ref", np.uint8), ("seq_edge_multiplicity", np.uint32))
SEQ_OUTPUTS = SEQ_GRAPH + SEQ_OFFSETS + SEQ_VERTEX + tuple(n for n, _ in SEQ_EDGE) + ("seq_bases", "vertex_to_seq")


def sequence_graph(engine, regions, graph, applied=None, connected=None, read_first=None, read_len=None, capacity=None, fill=None, omit=()):
    """The zipped sequence graph of many graphs (phmm_assembly_seqgraph): to_sequence_graph, clean_non_ref_paths, the first
    zip_linear_chains, the orphans and the vertices the reference source neither reaches nor is reached from.  regions: what
    assembly_graph was given (a list of (reference, reads), or pack()'s dict); graph: the dict assembly_graph returns (k,
    vertex_off, vertex_seq, vertex_pos and, without `applied`, the edge arrays); applied: the dict apply_recovery returns -- its
    offsets, edges, masks and new vertices replace the graph's -- or None; connected: the dict prune_graph returned for that
    graph -- its vertex_state / edge_state make the absent masks and its graph_flags travel along -- or a dict with
    vertex_absent / edge_absent (and graph_flags), or None for applied's masks; read_first / read_len: the windows
    assembly_graph was given; capacity: (sequence vertices, edges, bytes), None asks the library first (a call with capacities
    0); fill: a byte the output arrays hold before the call, omit: names of arrays to pass as NULL (tests).  Returns a dict of
    numpy arrays: seq_status, n_seq_vertices, n_seq_edges, n_seq_bases, n_chains_zipped, n_removed_clean,
    n_removed_unconnected, seq_ref_source, seq_ref_sink [n_graphs]; seq_vertex_off, seq_edge_off, seq_base_off [n_graphs + 1];
    the per-vertex, per-edge and seq_bases arrays cut to what was written; vertex_to_seq [vertices]; required.  Raises
    PhmmError; after PHMM_ERR_EVENT_CAPACITY its `required` attribute holds the sizes."""
    a = regions if isinstance(regions, dict) else pack(regions)
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8).reshape(-1)  # noqa: E731
    region_ref_off, region_read_off, read_off = u32(a.get("region_ref_off")), u32(a.get("region_read_off")), u32(a.get("read_off"))
    ref_bases, read_bases = u8(a.get("ref_bases")), u8(a.get("read_bases"))
    read_first, read_len = u32(read_first), u32(read_len)
    k = u32(graph.get("k"))
    n_k = 0 if k is None else len(k)
    n_regions = next((len(x) - 1 for x in (region_ref_off, region_read_off) if x is not None), 0)
    n_graphs = n_k * n_regions
    shape = graph if applied is None else applied
    g32 = {name: u32(shape.get(name)) for name in ("vertex_off", "edge_off", "edge_src", "edge_dst", "edge_multiplicity")}
    g32.update(vertex_seq=u32(graph.get("vertex_seq")), vertex_pos=u32(graph.get("vertex_pos")))
    edge_is_ref = u8(shape.get("edge_is_ref"))
    new_vertex_off, new_vertex_kmer = u32(shape.get("new_vertex_off")), u8(shape.get("new_vertex_kmer"))
    vertex_absent, edge_absent, graph_flags = u8(shape.get("vertex_absent")), u8(shape.get("edge_absent")), u32(shape.get("graph_flags"))
    if connected is not None:
        if "vertex_state" in connected:
            vertex_absent, edge_absent = u8((np.asarray(connected["vertex_state"]) & _GONE) != 0), u8((np.asarray(connected["edge_state"]) & _GONE) != 0)
        else:
            vertex_absent, edge_absent = u8(connected.get("vertex_absent")), u8(connected.get("edge_absent"))
        graph_flags = u32(connected.get("graph_flags"))
    n_v = int(g32["vertex_off"][-1]) if n_graphs and g32["vertex_off"] is not None and len(g32["vertex_off"]) else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731

    def call(cap):
        cap = np.ascontiguousarray(cap, np.uint32)
        o = dict(required=new(3, np.uint32))
        o.update({name: new(n_graphs, np.uint32) for name in SEQ_GRAPH})
        o.update({name: new(n_graphs + 1, np.uint32) for name in SEQ_OFFSETS})
        o.update({name: new(int(cap[0]), np.uint32) if cap[0] else None for name in SEQ_VERTEX})
        o.update({name: new(int(cap[1]), dt) if cap[1] else None for name, dt in SEQ_EDGE})
        o.update(seq_bases=new(int(cap[2]), np.uint8) if cap[2] else None, vertex_to_seq=new(n_v, np.uint32))
        for name in omit:
            o[name] = None
        ptr = lambda name: _p(o[name], _lib.u8p if o[name] is not None and o[name].dtype == np.uint8 else _lib.u32p)  # noqa: E731
        code = engine.lib.phmm_assembly_seqgraph(
            engine._h, n_regions, _p(region_ref_off, _lib.u32p), _p(ref_bases, _lib.u8p), _p(region_read_off, _lib.u32p), _p(read_off, _lib.u32p),
            _p(read_bases, _lib.u8p), _p(read_first, _lib.u32p), _p(read_len, _lib.u32p), n_k, _p(k, _lib.u32p),
            *[_p(g32[name], _lib.u32p) for name in ("vertex_off", "edge_off", "vertex_seq", "vertex_pos", "edge_src", "edge_dst")],
            _p(edge_is_ref, _lib.u8p), _p(g32["edge_multiplicity"], _lib.u32p), None if "new_vertex_off" in omit else _p(new_vertex_off, _lib.u32p),
            None if "new_vertex_kmer" in omit else _p(new_vertex_kmer, _lib.u8p), _p(vertex_absent, _lib.u8p), _p(edge_absent, _lib.u8p),
            _p(graph_flags, _lib.u32p), None if "capacity" in omit else _p(cap, _lib.u32p), ptr("required"), *[ptr(name) for name in SEQ_OUTPUTS])
        return code, o

    if capacity is None:
        code, o = call((0, 0, 0))
        if code == _lib.PHMM_ERR_EVENT_CAPACITY:
            code, o = call(o["required"])
    else:
        code, o = call(capacity)
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.required = None if o["required"] is None else o["required"].copy()
        err.outputs = {name: v for name, v in o.items() if v is not None and name != "required"}
        raise err
    n_vertex, n_edge, n_bases = (int(x) for x in o["required"])
    for name in SEQ_VERTEX:
        o[name] = np.zeros(0, np.uint32) if o[name] is None else o[name][:n_vertex]
    for name, dt in SEQ_EDGE:
        o[name] = np.zeros(0, dt) if o[name] is None else o[name][:n_edge]
    o["seq_bases"] = np.zeros(0, np.uint8) if o["seq_bases"] is None else o["seq_bases"][:n_bases]
    return o


PATHS_GRAPH = ("paths_status", "n_paths", "n_popped", "n_cycle_edges_removed", "n_cycle_vertices_removed")
PATHS_OFFSETS = ("path_off", "path_edge_off", "hap_base_off")
PATHS_PATH = (("path_score", np.float64), ("path_is_ref", np.uint8), ("path_n_edges", np.uint32))
PATHS_OUTPUTS = (PATHS_GRAPH + PATHS_OFFSETS + tuple(n for n, _ in PATHS_PATH) +
                 ("hap_off", "path_first_equal", "path_edges", "hap_bases", "edge_removed", "vertex_removed"))


def best_paths(engine, seq, max_paths=128, max_nodes_per_graph=1 << 16, roles=None, regions=None, capacity=None, fill=None, omit=()):
    """The k best haplotype paths of many sequence graphs (phmm_assembly_best_paths): the cycle removal of the reference's
    KBestHaplotypeFinder as written, its best-first search, every path's bases and, with `regions`, the duplicate marks.  seq:
    the dict sequence_graph returns (seq_vertex_off, seq_edge_off, seq_base_off, seq_vertex_base_off, the seq_edge arrays,
    seq_bases, and seq_status, seq_ref_source, seq_ref_sink where present); roles: a byte per vertex (bit 0 a source, bit 1 a
    sink) in place of seq_ref_source / seq_ref_sink, or None; regions: None, or a dict with region_ref_off and ref_bases
    (pack()'s will do) and optionally n_k -- the graphs are then n_k x n_regions, k-major -- or a list of (reference, reads);
    capacity: (paths, path edges, bytes), None asks the library first (a call with capacities 0, which runs the whole search: pass
    the `required` of an earlier call over the same graphs, or any upper bound, to search once); fill: a byte the output
    arrays hold before the call, omit: names of arrays to pass as NULL (tests).  Returns a dict of numpy arrays: paths_status,
    n_paths, n_popped, n_cycle_edges_removed, n_cycle_vertices_removed [n_graphs]; path_off, path_edge_off, hap_base_off
    [n_graphs + 1]; path_score, path_is_ref, path_n_edges, path_first_equal (with regions) [paths]; hap_off [paths + 1];
    path_edges, hap_bases; edge_removed [edges], vertex_removed [vertices]; required.  Raises PhmmError; after
    PHMM_ERR_EVENT_CAPACITY its `required` attribute holds the sizes."""
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32).reshape(-1)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8).reshape(-1)  # noqa: E731
    s32 = {name: u32(seq.get(name)) for name in ("seq_vertex_off", "seq_edge_off", "seq_base_off", "seq_vertex_base_off", "seq_edge_src", "seq_edge_dst",
                                                 "seq_edge_multiplicity", "seq_status", "seq_ref_source", "seq_ref_sink")}
    edge_is_ref, seq_bases, roles = u8(seq.get("seq_edge_is_ref")), u8(seq.get("seq_bases")), u8(roles)
    n_graphs = 0 if s32["seq_vertex_off"] is None else max(len(s32["seq_vertex_off"]), 1) - 1
    n_v = int(s32["seq_vertex_off"][-1]) if n_graphs else 0
    n_e = int(s32["seq_edge_off"][-1]) if n_graphs and s32["seq_edge_off"] is not None and len(s32["seq_edge_off"]) else 0
    n_regions = n_k = 0
    region_ref_off = ref_bases = None
    if regions is not None:
        a = regions if isinstance(regions, dict) else pack(regions)
        region_ref_off, ref_bases = u32(a.get("region_ref_off")), u8(a.get("ref_bases"))
        n_regions = 0 if region_ref_off is None else max(len(region_ref_off), 1) - 1
        n_k = int(a["n_k"]) if "n_k" in a else (n_graphs // n_regions if n_regions else 0)
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    types = {np.dtype(np.uint8): _lib.u8p, np.dtype(np.uint32): _lib.u32p, np.dtype(np.float64): _lib.f64p}

    def call(cap):
        cap = np.ascontiguousarray(cap, np.uint32)
        o = dict(required=new(3, np.uint32))
        o.update({name: new(n_graphs, np.uint32) for name in PATHS_GRAPH})
        o.update({name: new(n_graphs + 1, np.uint32) for name in PATHS_OFFSETS})
        o.update({name: new(int(cap[0]), dt) if cap[0] else None for name, dt in PATHS_PATH})
        o.update(hap_off=new(int(cap[0]) + 1, np.uint32), path_first_equal=new(int(cap[0]), np.uint32) if regions is not None and cap[0] else None)
        o.update(path_edges=new(int(cap[1]), np.uint32) if cap[1] else None, hap_bases=new(int(cap[2]), np.uint8) if cap[2] else None)
        o.update(edge_removed=new(n_e, np.uint8), vertex_removed=new(n_v, np.uint8))
        for name in omit:
            o[name] = None
        ptr = lambda name: None if o[name] is None else _p(o[name], types[o[name].dtype])  # noqa: E731
        code = engine.lib.phmm_assembly_best_paths(
            engine._h, n_graphs, *[_p(s32[name], _lib.u32p) for name in ("seq_vertex_off", "seq_edge_off", "seq_base_off", "seq_vertex_base_off", "seq_edge_src", "seq_edge_dst")],
            _p(edge_is_ref, _lib.u8p), _p(s32["seq_edge_multiplicity"], _lib.u32p), _p(seq_bases, _lib.u8p), _p(s32["seq_status"], _lib.u32p),
            _p(s32["seq_ref_source"], _lib.u32p), _p(s32["seq_ref_sink"], _lib.u32p), _p(roles, _lib.u8p), max_paths, max_nodes_per_graph, n_regions, n_k,
            None if "region_ref_off" in omit else _p(region_ref_off, _lib.u32p), None if "ref_bases" in omit else _p(ref_bases, _lib.u8p),
            None if "capacity" in omit else _p(cap, _lib.u32p), ptr("required"), *[ptr(name) for name in PATHS_OUTPUTS])
        return code, o

    if capacity is None:
        code, o = call((0, 0, 0))
        if code == _lib.PHMM_ERR_EVENT_CAPACITY:
            code, o = call(o["required"])
    else:
        code, o = call(capacity)
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.required = None if o["required"] is None else o["required"].copy()
        err.outputs = {name: v for name, v in o.items() if v is not None and name != "required"}
        raise err
    n_path, n_edge, n_bases = (int(x) for x in o["required"])
    for name, dt in PATHS_PATH:
        o[name] = np.zeros(0, dt) if o[name] is None else o[name][:n_path]
    if regions is not None:
        o["path_first_equal"] = np.zeros(0, np.uint32) if o["path_first_equal"] is None else o["path_first_equal"][:n_path]
    o["hap_off"] = np.zeros(1, np.uint32) if o["hap_off"] is None else o["hap_off"][:n_path + 1]
    o["path_edges"] = np.zeros(0, np.uint32) if o["path_edges"] is None else o["path_edges"][:n_edge]
    o["hap_bases"] = np.zeros(0, np.uint8) if o["hap_bases"] is None else o["hap_bases"][:n_bases]
    return o
