"""phmm_assembly_seqgraph on the MI355X against the SERIAL restatement of the reference's sequence-graph stage
(tests/assembly_seqgraph_restatement.py), through the C ABI as lorikeet_amd.assembly binds it.  EQUALITY on every output array:
it is all integers and bytes, there are no tolerances.  The graphs come from tests/assembly_seqgraph_cases.py;
tests/test_assembly_seqgraph_oracle.py holds the restatement to the reference's rows and to the hand-derived cases on the CPU.
The module takes sequence_graph from lorikeet_amd.assembly at the top: without the call every test here fails."""
import numpy as np
import pytest

import assembly_graph_cases as G
import assembly_recover_cases as RC
import assembly_recover_restatement as RR
import assembly_seqgraph_cases as C
import assembly_seqgraph_restatement as R
from lorikeet_amd import _lib
from lorikeet_amd.assembly import apply_recovery, assembly_graph, pack, prune_graph, recover_dangling_ends, sequence_graph
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
SETS = C.gpu_sets()


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def run(eng, graphs, **kw):
    regions, gd, applied, _ = C.pack(graphs)
    return sequence_graph(eng, regions, gd, applied, **kw)


def same(got, want, tag):
    for name in C.OUTPUTS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("name", sorted(SETS))
def test_equals_the_restatement(eng, name):
    """every graph of a set in a call of its own, then the set in one call: the golden rows and the hand cases; chains of 1, 2, 63,
    64, 65, 129, 255, 256, 257 and 1 025 vertices numbered along the chain and against it; a source vertex with k = 3 and k = 65
    whose chain's bytes cross 64 and 128; 1, 64, 65 and 300 merged chains on one graph"""
    graphs = SETS[name]
    for i, g in enumerate(graphs):
        same(run(eng, [g], fill=0xAB), C.expected([g]), (name, i))
    same(run(eng, graphs, fill=0xAB), C.expected(graphs), name)


def test_the_shapes_are_what_their_names_say(eng):
    o = run(eng, SETS["chains"])
    assert sorted(int(x) for x in o["seq_vertex_n_merged"]) == sorted([1, 1] + [n for n in (2, 63, 64, 65, 129, 255, 256, 257, 1025) for _ in range(2)])
    o = run(eng, SETS["source_bytes"])
    assert sorted(int(x) for x in o["n_seq_bases"] if x) == sorted(k + n - 1 for k in (3, 65) for n in (1, 2, 62, 64, 66, 127, 130))
    o = run(eng, SETS["many_chains"])
    assert [int(o["n_chains_zipped"][s]) for s in C.pack(SETS["many_chains"])[3]] == [2, 64, 66, 64, 65, 300]
    star = run(eng, [C.star(300)])
    assert star["n_seq_vertices"].tolist() == [302] and star["n_seq_edges"].tolist() == [602]


@pytest.mark.parametrize("name", ["chain into chain, the source chain first", "chain into chain, the target chain first", "last -> first", "reference break"])
def test_the_hand_cases_as_derived(eng, name):
    case = next(c for c in C.golden()["hand"] if c["name"] == name)
    o, want = run(eng, [C.hand_graphs()[name]]), case["expected"]
    off = o["seq_vertex_base_off"].tolist() + [int(o["n_seq_bases"][0])]
    assert [o["seq_bases"][off[i]:off[i + 1]].tobytes().decode() for i in range(len(off) - 1)] == want["vertices"]
    assert np.stack([o["seq_edge_src"], o["seq_edge_dst"], o["seq_edge_is_ref"], o["seq_edge_multiplicity"]], 1).tolist() == want["edges"]
    assert o["seq_vertex_first"].tolist() == want["first"] and o["vertex_to_seq"].tolist() == want["vertex_to_seq"]


def test_an_absent_mask_graph_against_the_same_graph_compacted_by_hand(eng):
    masked = [g for g in C.random_graphs(80, seed=5, largest=60) if g["vertex_absent"] is not None and not g["n_new"]]
    assert len(masked) >= 10
    a, b = run(eng, masked), run(eng, [C.compacted(g)[0] for g in masked])
    for name in C.PER_GRAPH + C.OFFSETS + ("seq_vertex_base_off", "seq_vertex_n_merged") + C.PER_EDGE + ("seq_bases",):
        assert a[name].tobytes() == b[name].tobytes(), name
    same(a, C.expected(masked), "masked")


def test_a_batch_of_200_random_graphs_each_equal_to_itself_alone_and_to_a_second_run(eng):
    graphs = C.random_graphs()
    assert len(graphs) == 200 and max(len(g["kmers"]) for g in graphs) == 3000
    first, again = run(eng, graphs, fill=0xAB), run(eng, graphs, fill=0xCD)
    same(first, C.expected(graphs), "batch")
    for name in C.OUTPUTS:
        assert first[name].tobytes() == again[name].tobytes(), name
    regions, gd, applied, slots = C.pack(graphs)
    for i, g in enumerate(graphs):
        alone, s = run(eng, [g]), slots[i]
        for name in C.PER_GRAPH:
            assert first[name][s] == alone[name][0], (i, name)
        for names, off in ((C.PER_VERTEX, "seq_vertex_off"), (C.PER_EDGE, "seq_edge_off"), (("seq_bases",), "seq_base_off")):
            for name in names:
                assert first[name][first[off][s]:first[off][s + 1]].tobytes() == alone[name].tobytes(), (i, name)
        v0, v1 = applied["vertex_off"][s], applied["vertex_off"][s + 1]
        assert first["vertex_to_seq"][v0:v1].tobytes() == alone["vertex_to_seq"].tobytes(), i


@pytest.mark.parametrize("name", ["hand"] + sorted(G.calls()))
def test_the_pipeline_of_six_calls_on_the_returned_dicts(eng, name):
    """assembly_graph -> prune_graph(CHAINS) -> recover_dangling_ends -> apply_recovery -> prune_graph(CONNECT) -> sequence_graph on
    the dicts the calls return, against the restatements chained the same way.  Cyclic graphs and graphs without reference ends
    travel along flagged and come back skipped"""
    c = G.calls()[name] if name in G.calls() else None
    if c is None:
        c = G.call([reg for reg, _ in G.hand().values()], sorted({k for _, k in G.hand().values()}))
    regions = [(g["ref"], g["reads"]) for g in c["regions"]]
    raw = assembly_graph(eng, regions, c["k"], c["min_q"], read_sample=G.samples_of(c), num_pruning_samples=c["nps"], planes=False)
    cfg = RR.Config(min_dangling_branch_length=1)
    factor = 2
    pruned = prune_graph(eng, raw, factor, ops=_lib.PHMM_PRUNE_OP_CHAINS)
    cyc = (pruned["graph_flags"] & _lib.PHMM_PRUNE_HAS_CYCLE) != 0
    masks = dict(vertex_absent=(pruned["vertex_state"] & RC.GONE) != 0, edge_absent=(pruned["edge_state"] & RC.GONE) != 0)
    for o in np.flatnonzero(cyc):                                  # (recovery refuses cyclic graphs: they go in emptied, as in (t)'s test)
        masks["vertex_absent"][raw["vertex_off"][o]:raw["vertex_off"][o + 1]] = True
        masks["edge_absent"][raw["edge_off"][o]:raw["edge_off"][o + 1]] = True
    rec = recover_dangling_ends(eng, regions, raw, masks, factor, ops=cfg.ops, min_dangling_branch_length=cfg.min_dangling_branch_length,
                                min_matching_bases=cfg.min_matching_bases, max_mismatches_in_dangling_head=cfg.max_mismatches_in_dangling_head,
                                num_pruning_samples=cfg.num_pruning_samples, sw_parameters=cfg.sw)
    after = apply_recovery(raw, masks, rec)
    final = prune_graph(eng, after, factor, ops=_lib.PHMM_PRUNE_OP_CONNECT, vertex_absent=after["vertex_absent"], edge_absent=after["edge_absent"])
    seq = sequence_graph(eng, regions, raw, after, final, fill=0xAB)
    skipped = (final["graph_flags"] & (_lib.PHMM_PRUNE_HAS_CYCLE | _lib.PHMM_PRUNE_NO_REF_ENDS)) != 0
    assert (seq["seq_status"] == np.where(skipped, _lib.PHMM_SEQ_SKIPPED, seq["seq_status"])).all()
    o = n_ok = 0
    for k in c["k"]:
        for reg in c["regions"]:
            g = RC.from_region(reg["ref"], reg["reads"], k, factor, chains=True, min_q=c["min_q"], nps=c["nps"], samples=reg.get("samples"))
            if not cyc[o] and not skipped[o] and g["kmers"]:
                gr = RC.one(g, cfg)["graph"]                       # the restatement's graph behind recovery
                kmers = list(g["kmers"]) + [bytes(km) for km in RC.one(g, cfg)["new_vertex_kmer"]]
                v0, v1, e0, e1 = after["vertex_off"][o], after["vertex_off"][o + 1], after["edge_off"][o], after["edge_off"][o + 1]
                va = ((final["vertex_state"][v0:v1] & RC.GONE) != 0).astype(int).tolist()
                ea = ((final["edge_state"][e0:e1] & RC.GONE) != 0).astype(int).tolist()
                assert len(kmers) == v1 - v0 == len(gr.node)
                edges = [(int(a), int(b), int(r), int(m)) for a, b, r, m in zip(after["edge_src"][e0:e1], after["edge_dst"][e0:e1], after["edge_is_ref"][e0:e1],
                                                                               after["edge_multiplicity"][e0:e1])]
                x = R.sequence_graph(len(kmers), edges, kmers, va, ea)
                for nm in C.PER_GRAPH:
                    assert seq[nm][o] == x[nm], (name, o, nm)
                for names, off in ((C.PER_VERTEX, "seq_vertex_off"), (C.PER_EDGE, "seq_edge_off")):
                    for nm in names:
                        assert seq[nm][seq[off][o]:seq[off][o + 1]].tolist() == x[nm], (name, o, nm)
                assert seq["seq_bases"][seq["seq_base_off"][o]:seq["seq_base_off"][o + 1]].tobytes() == x["seq_bases"], (name, o)
                assert seq["vertex_to_seq"][v0:v1].tolist() == x["vertex_to_seq"], (name, o)
                n_ok += x["seq_status"] == R.OK and x["n_seq_vertices"] > 0
            o += 1
    assert n_ok or name != "hand"


def test_the_capacity_protocol(eng):
    graphs = SETS["hand"] + SETS["many_chains"][:2]
    regions, gd, applied, _ = C.pack(graphs)
    with pytest.raises(PhmmError) as e:
        sequence_graph(eng, regions, gd, applied, capacity=(0, 0, 0), fill=0xAB)
    assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY
    need = e.value.required.tolist()
    want = C.expected(graphs)
    assert need == [len(want["seq_vertex_first"]), len(want["seq_edge_src"]), len(want["seq_bases"])] and all(n > 0 for n in need)
    for name, out in e.value.outputs.items():                      # nothing but `required` written
        assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), name
    same(sequence_graph(eng, regions, gd, applied, capacity=need), want, "capacity")
    for short in range(3):
        cap = list(need)
        cap[short] -= 1
        with pytest.raises(PhmmError) as e:
            sequence_graph(eng, regions, gd, applied, capacity=cap, fill=0xAB)
        assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and e.value.required.tolist() == need
        for name, out in e.value.outputs.items():
            assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), (short, name)


def test_fill_is_untouched_beyond_what_is_written_and_omit(eng):
    graphs = SETS["hand"]
    regions, gd, applied, _ = C.pack(graphs)
    want = C.expected(graphs)
    need = [len(want["seq_vertex_first"]), len(want["seq_edge_src"]), len(want["seq_bases"])]
    regions_d = pack(regions)
    u32 = lambda x: np.ascontiguousarray(x, np.uint32)  # noqa: E731
    # (through the C ABI with arrays longer than needed: the wrapper cuts its arrays, so the tail is looked at here)
    cap = np.asarray([n + 3 for n in need], np.uint32)
    ng, nv = len(applied["vertex_off"]) - 1, int(applied["vertex_off"][-1])
    filled = lambda n, dt: np.frombuffer(b"\xab" * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    outs = [filled(ng, np.uint32) for _ in range(9)] + [filled(ng + 1, np.uint32) for _ in range(3)] + [filled(int(cap[0]), np.uint32) for _ in range(3)] + \
           [filled(int(cap[1]), np.uint32), filled(int(cap[1]), np.uint32), filled(int(cap[1]), np.uint8), filled(int(cap[1]), np.uint32),
            filled(int(cap[2]), np.uint8), filled(nv, np.uint32)]
    required = filled(3, np.uint32)
    p = lambda a: a.ctypes.data_as(_lib.u8p if a.dtype == np.uint8 else _lib.u32p)  # noqa: E731
    ins = [u32(regions_d["region_ref_off"]), regions_d["ref_bases"], u32(regions_d["region_read_off"]), u32(regions_d["read_off"]), regions_d["read_bases"]]
    code = eng.lib.phmm_assembly_seqgraph(
        eng._h, len(graphs), p(ins[0]), p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), None, None, len(gd["k"]), p(gd["k"]), p(applied["vertex_off"]),
        p(applied["edge_off"]), p(gd["vertex_seq"]), p(gd["vertex_pos"]), p(applied["edge_src"]), p(applied["edge_dst"]), p(applied["edge_is_ref"]),
        p(applied["edge_multiplicity"]), p(applied["new_vertex_off"]), p(np.ascontiguousarray(applied["new_vertex_kmer"]).reshape(-1)),
        p(applied["vertex_absent"]), p(applied["edge_absent"]), p(applied["graph_flags"]), p(cap), p(required), *[p(a) for a in outs])
    assert code == _lib.PHMM_OK and required.tolist() == need
    for a, n in zip(outs[12:20], [need[0]] * 3 + [need[1]] * 4 + [need[2]]):
        assert (np.frombuffer(a[n:].tobytes(), np.uint8) == 0xAB).all()
    assert outs[13][:need[0]].tolist() == want["seq_vertex_first"].tolist() and outs[19][:need[2]].tobytes() == want["seq_bases"].tobytes()
    o = sequence_graph(eng, regions, gd, applied, omit=("vertex_to_seq",))   # an array nobody asked for
    assert o["vertex_to_seq"] is None and o["seq_bases"].tobytes() == want["seq_bases"].tobytes()
    graphs = SETS["chains"][:6]                                    # neither masks, nor flags, nor new vertices: all NULL
    regions, gd, applied, _ = C.pack(graphs)
    o = sequence_graph(eng, regions, gd, dict(applied, graph_flags=None, new_vertex_off=None, new_vertex_kmer=None, vertex_absent=None, edge_absent=None))
    same(o, C.expected(graphs), "all NULL")


def test_no_graphs_empty_graphs_and_graphs_without_edges(eng):
    o = sequence_graph(eng, [], dict(k=np.zeros(0, np.uint32)), None, fill=0xAB)
    assert o["required"].tolist() == [0, 0, 0] and o["seq_vertex_off"].tolist() == [0] and o["seq_base_off"].tolist() == [0]
    graphs = [C.graph(5, [], []), C.graph(5, [b"ACGTA", b"CGTAC"], []), C.graph(5, [b"ACGTA"], [])]
    same(run(eng, graphs, fill=0xAB), C.expected(graphs), "without edges")
    o = run(eng, graphs)
    assert o["n_seq_vertices"].tolist() == [0, 0, 1] and o["n_removed_unconnected"].tolist() == [0, 0, 0] and o["seq_bases"].tobytes() == b"ACGTA"


# ---- PHMM_ERR_INVALID_ARG, every case the header names ---------------------------------------------------------------------------
def _arrays():
    hand = C.hand_graphs()
    return C.pack([hand["last -> first"], hand["a recovery-made vertex's bytes"]])


def _refused(eng, part, regions=None, gd=None, applied=None, **kw):
    r0, g0, a0, _ = _arrays()
    with pytest.raises(PhmmError) as e:
        sequence_graph(eng, r0 if regions is None else regions, g0 if gd is None else gd, a0 if applied is None else applied, fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and part in str(e.value), str(e.value)
    assert str(e.value).count("phmm_assembly_seqgraph") == 1
    for name, out in e.value.outputs.items():                      # nothing written
        assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), name
    assert e.value.required is None or (e.value.required == np.frombuffer(b"\xab" * 12, np.uint32)).all()


@pytest.mark.parametrize("name", ["vertex_off", "edge_off", "vertex_seq", "vertex_pos", "edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity"])
def test_a_null_array_is_refused(eng, name):
    _, gd, applied, _ = _arrays()
    gd, applied = dict(gd), dict(applied)
    (gd if name in gd else applied)[name] = None
    _refused(eng, "a required pointer is NULL", gd=gd, applied=applied)
    assert name in eng.last_error()


def test_null_capacity_and_required_and_half_a_pair_are_refused(eng):
    _refused(eng, "a required pointer is NULL (capacity, required)", omit=("capacity",))
    _refused(eng, "a required pointer is NULL (capacity, required)", omit=("required",))
    _refused(eng, "new_vertex_off and new_vertex_kmer are given together", omit=("new_vertex_off",))
    _refused(eng, "new_vertex_off and new_vertex_kmer are given together", omit=("new_vertex_kmer",))
    _refused(eng, "a required pointer is NULL (the per-graph outputs)", omit=("seq_status",))
    _refused(eng, "a required pointer is NULL (the per-graph outputs)", omit=("seq_base_off",))


@pytest.mark.parametrize("name", ["vertex_off", "edge_off", "new_vertex_off"])
def test_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    applied = dict(_arrays()[2])
    applied[name] = applied[name].copy()
    applied[name][0] = 1
    _refused(eng, "%s does not start at 0" % name, applied=applied)
    applied = dict(_arrays()[2])
    applied[name] = applied[name].copy()
    applied[name][1], applied[name][2] = 3, 2
    _refused(eng, "graph 1: %s decreases" % name, applied=applied)


def test_more_new_vertices_than_vertices_is_refused(eng):
    applied = dict(_arrays()[2])
    applied["new_vertex_off"] = np.array([0, 5, 6], np.uint32)
    applied["new_vertex_kmer"] = np.zeros((6, 3), np.uint8)
    _refused(eng, "graph 0: more new vertices than vertices", applied=applied)


@pytest.mark.parametrize("name, word", [("edge_src", "source"), ("edge_dst", "target")])
def test_an_endpoint_outside_its_graph_is_refused(eng, name, word):
    applied = dict(_arrays()[2])
    applied[name] = applied[name].copy()
    nv = int(applied["vertex_off"][1])
    applied[name][0] = nv
    _refused(eng, "graph 0: edge 0: its %s %d reaches n_vertices (%d)" % (word, nv, nv), applied=applied)


def test_masks_are_given_together_and_a_present_edge_has_present_endpoints(eng):
    applied = _arrays()[2]
    _refused(eng, "given together", applied=dict(applied, edge_absent=None))
    va = applied["vertex_absent"].copy()
    va[int(applied["edge_src"][0])] = 1
    _refused(eng, "graph 0: edge 0: it is present and an endpoint is absent", applied=dict(applied, vertex_absent=va))


def test_vertex_bytes_outside_their_sequence_are_refused(eng):
    gd = dict(_arrays()[1])
    gd["vertex_pos"] = gd["vertex_pos"].copy()
    gd["vertex_pos"][3] += 10 ** 6
    _refused(eng, "graph 0: vertex 3: its bytes", gd=gd)
    gd = dict(_arrays()[1])
    gd["vertex_seq"] = gd["vertex_seq"].copy()
    gd["vertex_seq"][2] = 1
    _refused(eng, "graph 0: vertex 2: its sequence 1 is not one of the region's (0 reads)", gd=gd)


@pytest.mark.parametrize("k", [0, 256])
def test_k_outside_its_range_is_refused(eng, k):
    _refused(eng, "k[0] = %d is outside 1 .. 255" % k, gd=dict(_arrays()[1], k=np.array([k], np.uint32)))


@pytest.mark.parametrize("name", ["region_ref_off", "region_read_off"])
def test_region_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    regions = pack(_arrays()[0])
    regions[name] = regions[name].copy()
    regions[name][0] = 1
    _refused(eng, "%s does not start at 0" % name, regions=regions)
    regions = pack(_arrays()[0])
    regions[name] = regions[name].copy()
    regions[name][1], regions[name][2] = 5, 4
    _refused(eng, "region 1: %s decreases" % name, regions=regions)


def test_a_read_window_outside_its_read_is_refused(eng):
    regions = pack(_arrays()[0])
    regions.update(region_read_off=np.array([0, 1, 1], np.uint32), read_off=np.array([0, 4], np.uint32), read_bases=np.frombuffer(b"ACGT", np.uint8),
                   read_quals=np.frombuffer(b"IIII", np.uint8))
    _refused(eng, "read 0: its window leaves the read", regions=regions, read_first=[2], read_len=[3])
    _refused(eng, "read_first and read_len are given together", regions=regions, read_first=[2])
    _refused(eng, "read_off does not start at 0", regions=dict(regions, read_off=np.array([1, 4], np.uint32)))


@pytest.mark.parametrize("name", ["seq_vertex_first", "seq_edge_is_ref", "seq_bases"])
def test_a_capacity_above_0_whose_arrays_are_null_is_refused(eng, name):
    need = sequence_graph(eng, *_arrays()[:3])["required"]
    assert all(int(n) > 0 for n in need)
    _refused(eng, "a capacity above 0 whose arrays are NULL", capacity=need, omit=(name,))
