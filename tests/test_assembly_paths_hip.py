"""phmm_assembly_best_paths on the MI355X against the SERIAL restatement of the reference's k-best haplotype finder
(tests/assembly_paths_restatement.py), through the C ABI as lorikeet_amd.assembly binds it.  EQUALITY on every output array,
no tolerances; path_score is compared as its 64-bit pattern, NaN included.  The graphs come from tests/assembly_paths_cases.py;
tests/test_assembly_paths_oracle.py holds the restatement to the reference's literals and to the hand-derived cases on the CPU.
The module takes best_paths from lorikeet_amd.assembly at the top: without the call every test here fails."""
import numpy as np
import pytest

import assembly_graph_cases as G
import assembly_paths_cases as C
import assembly_paths_restatement as R
import assembly_recover_cases as RC
import assembly_recover_restatement as RR
from lorikeet_amd import _lib
from lorikeet_amd.assembly import apply_recovery, assembly_graph, best_paths, prune_graph, recover_dangling_ends, sequence_graph
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError
from lorikeet_amd.smith_waterman import NEW_SW_PARAMETERS, OverhangStrategy

pytestmark = pytest.mark.gpu
SETS = C.gpu_sets()
OPS = "MIDNSHP=X"


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def run(eng, graphs, max_paths=128, max_nodes=C.DEFAULT_NODES, regions=None, n_k=1, status=None, **kw):
    seq, roles = C.pack(graphs, status)
    reg = None
    if regions is not None:
        reg = dict(region_ref_off=np.cumsum([0] + [len(r) for r in regions]).astype(np.uint32), ref_bases=np.frombuffer(b"".join(regions), np.uint8), n_k=n_k)
    return best_paths(eng, seq, max_paths, max_nodes, roles=roles, regions=reg, **kw)


def same(got, want, tag):
    for name in C.OUTPUTS:
        if name == "path_first_equal" and name not in want:
            assert name not in got or got[name] is None
            continue
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        if name == "path_score":
            g, w = C.score_bits(g), C.score_bits(w)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("name", sorted(SETS))
def test_equals_the_restatement(eng, name):
    """every graph of a set in a call of its own, then the set in one call: the reference's graphs and the hand cases; stars of 1,
    63, 64, 65 and 130 out-edges, all equal (the whole queue ties) and distinct; tie sets of 2, 64 and 65 paths that first differ at
    edge 0, 63, 64 and 129; chains of 1 to 1 025 edges, the last also with a back edge (the walk at depth 1 025); vertices of 0, 1,
    64, 65 and 300 bytes; ten bubbles at max_paths 1, 2, 128 and unlimited; the budget exactly enough and one short; a total of
    PHMM_PATHS_MAX_WEIGHT and one above; graphs without ends"""
    graphs, k, nodes = SETS[name]
    for i, g in enumerate(graphs):
        same(run(eng, [g], k, nodes, fill=0xAB), C.expected([g], k, nodes), (name, i))
    same(run(eng, graphs, k, nodes, fill=0xAB), C.expected(graphs, k, nodes), name)


def test_the_shapes_are_what_their_names_say(eng):
    o = run(eng, *SETS["stars, equal"][:2])
    assert o["n_paths"].tolist() == [1, 63, 64, 65, 130] and len(set(C.score_bits(o["path_score"][-130:]).tolist())) == 1
    o = run(eng, *SETS["tie sets"][:2])
    assert o["n_paths"].tolist() == [n for n in (2, 64, 65) for _ in range(4)]
    assert [int(o["path_n_edges"][o["path_off"][i]]) for i in range(12)] == [d + 2 for _ in range(3) for d in (0, 63, 64, 129)]
    o = run(eng, *SETS["chains"][:2])
    assert o["path_n_edges"].tolist() == [1, 63, 64, 65, 130, 1025, 1025] and o["n_cycle_edges_removed"].tolist() == [0] * 6 + [1]
    for k, n in ((1, 0), (2, 2), (128, 128), (R.UNLIMITED, 1024)):   # (max_paths 2: every vertex extends once, so one path reaches the last bubble and both its branches arrive)
        assert run(eng, [C.bubbles(10)], k)["n_paths"].tolist() == [n]
    assert run(eng, *SETS["budget exactly enough"])["paths_status"].tolist() == [R.OK, R.OK]
    assert run(eng, *SETS["budget one short"])["paths_status"].tolist() == [R.BUDGET, R.OK]
    assert run(eng, *SETS["weights"])["paths_status"].tolist() == [R.OK, R.WEIGHT_RANGE]
    o = run(eng, *SETS["vertex bytes"][:2])
    assert (np.diff(o["hap_off"]).tolist(), o["path_n_edges"].tolist()) == ([433, 133], [7, 6])


@pytest.mark.parametrize("case", C.golden()["hand"], ids=[c["name"] for c in C.golden()["hand"]])
def test_the_hand_cases_as_derived(eng, case):
    o, want = run(eng, [C.from_json(case["graph"])], case["max_paths"]), case["expected"]
    assert o["paths_status"].tolist() == [want["status"]] and o["n_popped"].tolist() == [want["n_popped"]]
    assert o["edge_removed"].tolist() == want["edge_removed"] and o["vertex_removed"].tolist() == want["vertex_removed"]
    assert o["n_paths"].tolist() == [len(want["paths"])]
    e, b = np.cumsum([0] + o["path_n_edges"].tolist()), o["hap_off"]
    for i, w in enumerate(want["paths"]):
        score = 0.0
        for m, t in w["steps"]:
            score = score + (R.log10(m) - R.log10(t))
        assert o["path_edges"][e[i]:e[i + 1]].tolist() == w["edges"] and o["hap_bases"][b[i]:b[i + 1]].tobytes() == w["bases"].encode()
        assert int(o["path_is_ref"][i]) == w["is_ref"] and C.hex_score(float(o["path_score"][i])) == C.hex_score(score if score == score else float("nan"))


def test_every_status(eng):
    graphs = [C.chain(3), C.chain(3), dict(C.chain(3), sink=R.NONE), C.from_json(C.golden()["hand"][3]["graph"]), C.from_json(C.golden()["hand"][2]["graph"]),
              C.weight(1), C.bubbles(10)]
    status = [0, _lib.PHMM_SEQ_SKIPPED, 0, 0, 0, 0, 0]
    o = run(eng, graphs, R.UNLIMITED, 100, status=status, fill=0xAB)
    assert o["paths_status"].tolist() == [R.OK, R.SKIPPED, R.NO_ENDS, R.NO_PATH, R.CYCLES_STAY, R.WEIGHT_RANGE, R.BUDGET]
    assert o["n_paths"].tolist() == [1, 0, 0, 0, 0, 0, 0]
    same(o, C.expected(graphs, R.UNLIMITED, 100, status=status), "statuses")
    skipped = run(eng, graphs[:2], status=[_lib.PHMM_SEQ_REFERENCE_FAILS, 0])
    assert skipped["paths_status"].tolist() == [R.SKIPPED, R.OK]


def test_250_random_graphs_each_equal_to_itself_alone_and_to_a_second_run(eng):
    graphs = C.random_graphs()
    assert len(graphs) == 250 and max(len(g["vertices"]) for g in graphs) == 60
    want = C.expected(graphs, 16)
    assert {"cyclic", "NaN", "-inf", "tie by edge list", "vertex removed", "cross or forward edge removed"} <= want["census"]
    first, again = run(eng, graphs, 16, fill=0xAB), run(eng, graphs, 16, fill=0xCD)
    same(first, want, "batch")
    for name in C.OUTPUTS:
        if first.get(name) is not None:
            assert first[name].tobytes() == again[name].tobytes(), name
    vo, eo = np.cumsum([0] + [len(g["vertices"]) for g in graphs]), np.cumsum([0] + [len(g["edges"]) for g in graphs])
    for i, g in enumerate(graphs):
        alone = run(eng, [g], 16)
        for name in C.PER_GRAPH:
            assert first[name][i] == alone[name][0], (i, name)
        p0, p1 = first["path_off"][i], first["path_off"][i + 1]
        for name in C.PER_PATH:
            assert first[name][p0:p1].tobytes() == alone[name].tobytes(), (i, name)
        assert (first["hap_off"][p0:p1 + 1] - first["hap_off"][p0]).tolist() == alone["hap_off"].tolist(), i
        assert first["path_edges"][first["path_edge_off"][i]:first["path_edge_off"][i + 1]].tobytes() == alone["path_edges"].tobytes(), i
        assert first["hap_bases"][first["hap_base_off"][i]:first["hap_base_off"][i + 1]].tobytes() == alone["hap_bases"].tobytes(), i
        assert first["edge_removed"][eo[i]:eo[i + 1]].tobytes() == alone["edge_removed"].tobytes(), i
        assert first["vertex_removed"][vo[i]:vo[i + 1]].tobytes() == alone["vertex_removed"].tobytes(), i


def test_the_duplicate_marks(eng):
    graphs, regions, n_k = C.duplicates()
    o = run(eng, graphs, regions=regions, n_k=n_k, fill=0xAB)
    same(o, C.expected(graphs, regions=regions, n_k=n_k), "duplicates")
    assert o["path_first_equal"].tolist() == [R.EQUALS_REF, R.NONE, R.EQUALS_REF, R.NONE, 1, R.NONE, R.NONE, R.NONE, R.EQUALS_REF, 5, 3, 7]
    many = [C.with_roles(g) for g in C.random_graphs(60, seed=23, largest=12)] * 3     # the same graphs under three k: everything met before
    ref = [b"ACGT"] * 60
    same(run(eng, many, 16, regions=ref, n_k=3, fill=0xAB), C.expected(many, 16, regions=ref, n_k=3), "random duplicates")


def cigar_strings(eng, reference, o):
    """hap_off / hap_bases handed unchanged to phmm_calculate_cigar, every path against `reference`"""
    import ctypes
    n = len(o["hap_off"]) - 1
    ref = np.frombuffer(reference.encode() * n, np.uint8)
    ref_off = (np.arange(n + 1) * len(reference)).astype(np.uint32)
    cig_off = (np.arange(n + 1) * 32).astype(np.uint64)
    cigar, n_cig, status = np.zeros(32 * n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.int32)
    prm = NEW_SW_PARAMETERS.as_struct()
    code = eng.lib.phmm_calculate_cigar(eng._h, n, ref_off.ctypes.data_as(_lib.u32p), ref.ctypes.data_as(_lib.u8p), o["hap_off"].ctypes.data_as(_lib.u32p),
                                        o["hap_bases"].ctypes.data_as(_lib.u8p), ctypes.byref(prm), OverhangStrategy.SoftClip,
                                        cig_off.ctypes.data_as(_lib.u64p), cigar.ctypes.data_as(_lib.u32p), n_cig.ctypes.data_as(_lib.u32p),
                                        status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert code == _lib.PHMM_OK and not status.any(), (code, status.tolist(), eng.last_error())
    return ["".join("%d%s" % (x >> 4, OPS[x & 15]) for x in cigar[32 * i:32 * i + int(n_cig[i])]) for i in range(n)]


@pytest.mark.parametrize("row", C.golden()["two_paths"], ids=[r["name"] for r in C.golden()["two_paths"]])
def test_the_two_path_cigars(eng, row):
    """10M and 1M3I5M3D1M; 51M and 3M6I48M"""
    o = run(eng, [C.from_json(row["graph"])], R.UNLIMITED)
    assert cigar_strings(eng, row["reference"], o) == row["cigars"]


@pytest.mark.parametrize("row", C.golden()["basic_bubbles"] + C.golden()["triple_bubbles"], ids=[r["name"] for r in C.golden()["basic_bubbles"] + C.golden()["triple_bubbles"]])
def test_the_bubble_rows_cigars(eng, row):
    """the 9 + 18 bubble rows: the CIGAR of the path the reference builds by hand, found among the call's paths"""
    o = run(eng, [C.from_json(row["graph"])], R.UNLIMITED)
    e = np.cumsum([0] + o["path_n_edges"].tolist())
    at = [o["path_edges"][e[i]:e[i + 1]].tolist() for i in range(len(e) - 1)].index(row["path"])
    assert cigar_strings(eng, row["reference"], o)[at] == row["cigar"]


def test_the_capacity_protocol_and_omit(eng):
    graphs, k, nodes = SETS["golden, singletons"]
    want = C.expected(graphs, k, nodes)
    need = [len(want["path_score"]), len(want["path_edges"]), len(want["hap_bases"])]
    for short in range(3):
        cap = list(need)
        cap[short] -= 1
        with pytest.raises(PhmmError) as e:
            run(eng, graphs, k, nodes, capacity=cap, fill=0xAB)
        assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and e.value.required.tolist() == need
        for name, a in e.value.outputs.items():   # nothing else written
            assert (a.view(np.uint8) == 0xAB).all(), name
    same(run(eng, graphs, k, nodes, capacity=[n + 7 for n in need], fill=0xAB), want, "roomy")
    o = run(eng, graphs, k, nodes, omit=("edge_removed", "vertex_removed"), fill=0xAB)
    assert o["edge_removed"] is None and o["vertex_removed"] is None
    for name in C.OUTPUTS[:-2]:
        if name != "path_first_equal":
            assert np.array_equal(o[name].view(np.uint8), want[name].view(np.uint8)), name
    empty = best_paths(eng, dict(seq_vertex_off=np.zeros(1, np.uint32), seq_edge_off=np.zeros(1, np.uint32), seq_base_off=np.zeros(1, np.uint32)), fill=0xAB)
    assert empty["required"].tolist() == [0, 0, 0] and empty["path_off"].tolist() == [0] and empty["hap_off"].tolist() == [0]


def bad(seq, change):
    seq, kw = dict(seq), {}
    for name, v in change.items():
        if name in ("roles", "max_paths", "max_nodes_per_graph", "regions", "omit", "capacity"):
            kw[name] = v
        elif v is None:
            seq.pop(name)
        else:
            seq[name] = v
    return seq, kw


INVALID = {
    "offsets not starting at 0": (dict(seq_edge_off=[1, 4, 6]), "seq_edge_off does not start at 0"),
    "offsets descending": (dict(seq_vertex_off=[0, 5, 4]), "seq_vertex_off decreases"),
    "an endpoint outside its graph": (dict(seq_edge_dst=[1, 2, 4, 1, 2]), "its target 4 reaches n_vertices (4)"),
    "a base offset past the bytes": (dict(seq_vertex_base_off=[0, 1, 2, 5, 0, 1, 2]), "is past the graph's bytes (4)"),
    "a base offset descending": (dict(seq_vertex_base_off=[0, 2, 1, 3, 0, 1, 2]), "seq_vertex_base_off decreases"),
    "a source that is no vertex": (dict(seq_ref_source=[4, 0]), "its source 4 is neither a vertex nor UINT32_MAX"),
    "a sink that is no vertex": (dict(seq_ref_sink=[3, 3]), "its sink 3 is neither a vertex nor UINT32_MAX"),
    "a role above 3": (dict(roles=[1, 0, 0, 2, 1, 4, 2]), "its role 4 is above 3"),
    "max_paths 0": (dict(max_paths=0), "max_paths is 0"),
    "max_nodes_per_graph 0": (dict(max_nodes_per_graph=0), "max_nodes_per_graph is 0"),
    "ref_bases without region_ref_off": (dict(regions=dict(region_ref_off=[0, 1, 2], ref_bases=[65, 67], n_k=1), omit=("region_ref_off",)), "given together or not at all"),
    "n_k x n_regions is not n_graphs": (dict(regions=dict(region_ref_off=[0, 1, 2], ref_bases=[65, 67], n_k=2)), "is not n_graphs (2)"),
    "region bytes without ref_bases": (dict(regions=dict(region_ref_off=[0, 1, 2], ref_bases=[65, 67], n_k=1), omit=("ref_bases",)), "a required pointer is NULL (ref_bases)"),
    "capacity NULL": (dict(omit=("capacity",)), "a required pointer is NULL (capacity, required)"),
    "required NULL": (dict(omit=("required",)), "a required pointer is NULL (capacity, required)"),
    "a NULL array that has elements": (dict(seq_edge_multiplicity=None), "a required pointer is NULL (seq_edge_src"),
    "the per-graph outputs NULL": (dict(omit=("n_popped",)), "a required pointer is NULL (the per-graph outputs)"),
    "a capacity above 0 with NULL arrays": (dict(capacity=[2, 5, 9], omit=("path_edges",)), "a capacity above 0 whose arrays are NULL"),
    "sums beyond 32 bits: the node pools": (dict(max_paths=0xffffffff, max_nodes_per_graph=0x80000000), "do not fit 32 bits"),
    "neither ends nor roles": (dict(seq_ref_sink=None), "a required pointer is NULL (graph_source, graph_sink"),
}


@pytest.mark.parametrize("name", sorted(INVALID))
def test_invalid_arguments_by_name(eng, name):
    seq, _ = C.pack([C.chain(3), C.chain(2)])
    change, part = INVALID[name]
    seq, kw = bad(seq, change)
    with pytest.raises(PhmmError) as e:
        best_paths(eng, seq, fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and part in str(e.value), str(e.value)
    for out, a in e.value.outputs.items():   # nothing is written
        assert (a.view(np.uint8) == 0xAB).all(), out
    if e.value.required is not None:
        assert (e.value.required.view(np.uint8) == 0xAB).all()


@pytest.mark.parametrize("n_graphs", [1, 2])
def test_outputs_beyond_32_bits_are_refused_not_a_capacity(eng, n_graphs):
    """sums beyond 32 bits, known only behind the search: 1 024 paths that each carry a first vertex of 5 MiB (one graph whose
    own bytes pass 2^32), or of 2.5 MiB in each of two graphs (only the sum does).  No capacity could hold them, so the call
    says INVALID_ARG and writes nothing -- a caller that loops on PHMM_ERR_EVENT_CAPACITY must not see it"""
    g = C.bubbles(10)
    g = dict(g, vertices=[b"A" * ((5 << 20) // n_graphs)] + g["vertices"][1:])
    with pytest.raises(PhmmError) as e:
        run(eng, [g] * n_graphs, R.UNLIMITED, fill=0xAB)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and "do not fit 32 bits" in str(e.value), str(e.value)
    assert (e.value.required.view(np.uint8) == 0xAB).all()
    for out, a in e.value.outputs.items():
        assert (a.view(np.uint8) == 0xAB).all(), out
    assert run(eng, [g] * n_graphs, 128)["n_paths"].tolist() == [128] * n_graphs   # (the same graphs within 32 bits: 128 x 5 MiB)


def test_path_first_equal_needs_the_region_arrays(eng):
    seq, _ = C.pack([C.chain(3)])
    out = {n: np.zeros(4, np.uint32) for n in ("required", "a", "b", "c", "d", "e", "f", "g", "h", "first")}
    cap = np.zeros(3, np.uint32)
    p = lambda a, t=_lib.u32p: a.ctypes.data_as(t)  # noqa: E731
    code = eng.lib.phmm_assembly_best_paths(
        eng._h, 1, p(seq["seq_vertex_off"]), p(seq["seq_edge_off"]), p(seq["seq_base_off"]), p(seq["seq_vertex_base_off"]), p(seq["seq_edge_src"]),
        p(seq["seq_edge_dst"]), p(seq["seq_edge_is_ref"], _lib.u8p), p(seq["seq_edge_multiplicity"]), p(seq["seq_bases"], _lib.u8p), None,
        p(seq["seq_ref_source"]), p(seq["seq_ref_sink"]), None, 128, 1 << 16, 0, 0, None, None, p(cap), p(out["required"]),
        *[p(out[n]) for n in "abcdefgh"], None, None, None, None, p(out["first"]), None, None, None, None)
    assert code == _lib.PHMM_ERR_INVALID_ARG and "path_first_equal is given without the region arrays" in eng.last_error()


@pytest.mark.parametrize("name", ["hand"] + sorted(G.calls()))
def test_the_chain_of_seven_calls_on_the_returned_dicts(eng, name):
    """assembly_graph -> prune_graph(CHAINS) -> recover_dangling_ends -> apply_recovery -> prune_graph(CONNECT) -> sequence_graph ->
    best_paths on the dict sequence_graph returns, with the regions for the duplicate marks, against the restatement on the graphs
    that dict holds"""
    c = G.calls()[name] if name in G.calls() else None
    if c is None:
        c = G.call([reg for reg, _ in G.hand().values()], sorted({k for _, k in G.hand().values()}))
    regions = [(g["ref"], g["reads"]) for g in c["regions"]]
    raw = assembly_graph(eng, regions, c["k"], c["min_q"], read_sample=G.samples_of(c), num_pruning_samples=c["nps"], planes=False)
    cfg = RR.Config(min_dangling_branch_length=1)
    pruned = prune_graph(eng, raw, 2, ops=_lib.PHMM_PRUNE_OP_CHAINS)
    cyc = (pruned["graph_flags"] & _lib.PHMM_PRUNE_HAS_CYCLE) != 0
    masks = dict(vertex_absent=(pruned["vertex_state"] & RC.GONE) != 0, edge_absent=(pruned["edge_state"] & RC.GONE) != 0)
    for o in np.flatnonzero(cyc):
        masks["vertex_absent"][raw["vertex_off"][o]:raw["vertex_off"][o + 1]] = True
        masks["edge_absent"][raw["edge_off"][o]:raw["edge_off"][o + 1]] = True
    rec = recover_dangling_ends(eng, regions, raw, masks, 2, ops=cfg.ops, min_dangling_branch_length=cfg.min_dangling_branch_length,
                                min_matching_bases=cfg.min_matching_bases, max_mismatches_in_dangling_head=cfg.max_mismatches_in_dangling_head,
                                num_pruning_samples=cfg.num_pruning_samples, sw_parameters=cfg.sw)
    after = apply_recovery(raw, masks, rec)
    final = prune_graph(eng, after, 2, ops=_lib.PHMM_PRUNE_OP_CONNECT, vertex_absent=after["vertex_absent"], edge_absent=after["edge_absent"])
    seq = sequence_graph(eng, regions, raw, after, final)
    refs = [G_bytes(g["ref"]) for g in c["regions"]]
    got = best_paths(eng, seq, regions=dict(region_ref_off=np.cumsum([0] + [len(r) for r in refs]).astype(np.uint32),
                                            ref_bases=np.frombuffer(b"".join(refs), np.uint8), n_k=len(c["k"])), fill=0xAB)
    want = C.expected(C.from_seq(seq), regions=refs, n_k=len(c["k"]), status=seq["seq_status"].tolist())
    same(got, want, name)


def G_bytes(x):
    return x.encode() if isinstance(x, str) else bytes(x)
