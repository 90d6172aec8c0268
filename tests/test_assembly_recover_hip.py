"""phmm_assembly_recover on the MI355X against the SERIAL restatement of the reference's dangling-end recovery
(tests/assembly_recover_restatement.py), through the C ABI as lorikeet_amd.assembly binds it.  EQUALITY on every output array: it
is all integers and bytes, there are no tolerances.  n_rounds is the schedule's own figure, not the reference's: it is held to
what the conflict graphs and the graphs without conflicts must give, and to itself from call to call.  The graphs come from
tests/assembly_recover_cases.py; tests/test_assembly_recover_oracle.py holds the restatement to the reference's literals on the
CPU.  The module takes recover_dangling_ends from lorikeet_amd.assembly at the top: without the call every test here fails."""
import numpy as np
import pytest

import assembly_graph_cases as G
import assembly_prune_cases as PC
import assembly_prune_restatement as P
import assembly_recover_cases as C
import assembly_recover_restatement as R
from lorikeet_amd import _lib
from lorikeet_amd.assembly import apply_recovery, assembly_graph, prune_graph, recover_dangling_ends
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
SETS = C.gpu_sets()


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def kwargs(cfg):
    return dict(ops=cfg.ops, min_dangling_branch_length=cfg.min_dangling_branch_length, min_matching_bases=cfg.min_matching_bases,
                max_mismatches_in_dangling_head=cfg.max_mismatches_in_dangling_head, num_pruning_samples=cfg.num_pruning_samples, sw_parameters=cfg.sw)


def run(eng, graphs, cfg, **kw):
    regions, gd, masks, factor, _ = C.pack(graphs)
    return recover_dangling_ends(eng, regions, gd, masks, factor, **dict(kwargs(cfg), **kw))


def same(got, want, tag):
    for name in C.OUTPUTS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("name", sorted(SETS))
def test_equals_the_restatement(eng, name):
    """every graph of a set in a call of its own, then the set in one call: the golden cases, alt paths of 63, 64, 65 and 129
    vertices, reference paths of 64, 65 and 130, 1, 64 and 65 tails and heads on one graph, the conflict graphs"""
    graphs, cfg = SETS[name]
    for i, g in enumerate(graphs):
        same(run(eng, [g], cfg, fill=0xAB), C.expected([g], cfg), (name, i))
    same(run(eng, graphs, cfg, fill=0xAB), C.expected(graphs, cfg), name)


def test_the_shapes_are_what_their_names_say(eng):
    graphs, cfg = SETS["alt_paths"]
    o = run(eng, graphs, cfg)
    assert sorted(o["end_alt_len"][o["end_kind"] == 0].tolist()) == [63, 64, 65, 129]
    assert sorted(o["end_alt_len"][o["end_kind"] == 1].tolist()) == [63 + 10, 64 + 10, 65 + 10, 129 + 10]   # (the source's k-mer whole: k - 1 more)
    assert (o["end_status"][o["end_kind"] == 0] == _lib.PHMM_RECOVER_END_MERGED).all(), o["end_status"]
    graphs, cfg = SETS["ref_paths"]
    assert sorted(run(eng, graphs, cfg)["end_ref_len"].tolist()) == [64, 65, 130]
    graphs, cfg = SETS["many_ends"]
    o = run(eng, graphs, cfg)
    assert sorted(int(x) for x in o["n_tails"] if x) == [1, 64, 65] and sorted(int(x) for x in o["n_heads"] if x)[-3:] == [1, 64, 65]


def test_rounds_count_the_conflicts(eng):
    """each conflict graph is built so that exactly the serial order gives the expected edges (tests/test_assembly_recover_oracle.py
    states them): the second end inspects a vertex whose edges the first changed, so a second round is needed; ends that do not
    interfere need one round per kind"""
    graphs, cfg = SETS["conflicts"]
    for g in graphs:
        o = run(eng, [g], cfg)
        assert o["n_rounds"].tolist() == [2], o["n_rounds"]
        assert o["end_status"].tolist() == [_lib.PHMM_RECOVER_END_MERGED, _lib.PHMM_RECOVER_END_NO_PATH]
    graphs, cfg = SETS["many_ends"]
    o = run(eng, graphs, cfg)
    for t, h, r in zip(o["n_tails"].tolist(), o["n_heads"].tolist(), o["n_rounds"].tolist()):
        if t:                                                      # (a tail's reference path runs DOWN, past no earlier merge)
            assert h == 0 and r == 1, (t, h, r)
        elif h:                                                    # (a head's runs UP to the source, past every earlier head's merge)
            assert 1 <= r <= h, (t, h, r)
        else:
            assert r == 0


@pytest.mark.parametrize("ops", [R.OP_TAILS, R.OP_HEADS, R.OP_TAILS | R.OP_HEADS])
@pytest.mark.parametrize("min_matching_bases", [-1, 0, 2, 4])
def test_ops_and_min_matching_bases(eng, ops, min_matching_bases):
    graphs = [g for g, _ in C.golden_graphs().values()] + SETS["conflicts"][0]
    cfg = R.Config(ops=ops, min_dangling_branch_length=1, min_matching_bases=min_matching_bases)
    same(run(eng, graphs, cfg, fill=0xAB), C.expected(graphs, cfg), (ops, min_matching_bases))


def test_a_batch_of_200_random_graphs_each_equal_to_itself_alone_and_to_a_second_run(eng):
    graphs = C.random_regions()
    assert len(graphs) == 200 and {g["k"] for g in graphs} == set(range(3, 16))
    cfg = R.Config(min_dangling_branch_length=1, min_matching_bases=-1)
    first, again = run(eng, graphs, cfg, fill=0xAB), run(eng, graphs, cfg, fill=0xCD)
    same(first, C.expected(graphs, cfg), "batch")
    for name in C.OUTPUTS + ("n_rounds",):
        assert first[name].tobytes() == again[name].tobytes(), name
    slots = C.pack(graphs)[4]
    for i, g in enumerate(graphs):
        alone, s = run(eng, [g], cfg), slots[i]
        for name in C.PER_GRAPH + ("n_rounds",):
            assert first[name][s] == alone[name][0], (i, name)
        for names, off in ((C.PER_END, "end_off"), (C.PER_EDGE, "new_edge_off")):
            for name in names:
                assert first[name][first[off][s]:first[off][s + 1]].tobytes() == alone[name].tobytes(), (i, name)
        v0, v1 = first["new_vertex_off"][s], first["new_vertex_off"][s + 1]
        assert np.array_equal(first["new_vertex_kmer"][v0:v1, :g["k"]], alone["new_vertex_kmer"]), i
    new_arm = R.Config(min_dangling_branch_length=1, min_matching_bases=2)
    same(run(eng, graphs, new_arm), C.expected(graphs, new_arm), "batch, new arm")


@pytest.mark.parametrize("name", ["hand"] + sorted(G.calls()))
def test_the_pipeline_of_the_graph_stage_with_factors_0_to_2(eng, name):
    """assembly_graph -> prune_graph(CHAINS) -> recover_dangling_ends -> apply_recovery -> prune_graph(CONNECT), against the
    restatements chained the same way; cyclic graphs are left out of the comparison as the caller leaves them out of the stage"""
    c = G.calls()[name] if name in G.calls() else None
    if c is None:
        c = G.call([reg for reg, _ in G.hand().values()], sorted({k for _, k in G.hand().values()}))
    regions = [(g["ref"], g["reads"]) for g in c["regions"]]
    raw = assembly_graph(eng, regions, c["k"], c["min_q"], read_sample=G.samples_of(c), num_pruning_samples=c["nps"], planes=False)
    cfg = R.Config(min_dangling_branch_length=1)
    for factor in range(3):
        pruned = prune_graph(eng, raw, factor, ops=_lib.PHMM_PRUNE_OP_CHAINS)
        cyc = (pruned["graph_flags"] & _lib.PHMM_PRUNE_HAS_CYCLE) != 0
        masks = dict(vertex_absent=(pruned["vertex_state"] & C.GONE) != 0, edge_absent=(pruned["edge_state"] & C.GONE) != 0)
        # (a cyclic graph goes in emptied: every element absent)
        for o in np.flatnonzero(cyc):
            masks["vertex_absent"][raw["vertex_off"][o]:raw["vertex_off"][o + 1]] = True
            masks["edge_absent"][raw["edge_off"][o]:raw["edge_off"][o + 1]] = True
        rec = recover_dangling_ends(eng, regions, raw, masks, factor, **kwargs(cfg), fill=0xAB)
        after = apply_recovery(raw, masks, rec)
        final = prune_graph(eng, after, factor, ops=_lib.PHMM_PRUNE_OP_CONNECT, vertex_absent=after["vertex_absent"], edge_absent=after["edge_absent"])
        o = 0
        for ki, k in enumerate(c["k"]):
            for reg in c["regions"]:
                if not cyc[o]:
                    g = C.from_region(reg["ref"], reg["reads"], k, factor, chains=True, min_q=c["min_q"], nps=c["nps"], samples=reg.get("samples"))
                    if g["kmers"]:
                        x = C.one(g, cfg)
                        for nm in C.PER_GRAPH:
                            assert rec[nm][o] == x[nm], (name, factor, o, nm)
                        for names, off in ((C.PER_END, "end_off"), (C.PER_EDGE, "new_edge_off")):
                            for nm in names:
                                assert rec[nm][rec[off][o]:rec[off][o + 1]].tolist() == x[nm], (name, factor, o, nm)
                        n0, n1 = rec["new_vertex_off"][o], rec["new_vertex_off"][o + 1]
                        assert [bytes(row[:k]) for row in rec["new_vertex_kmer"][n0:n1]] == x["new_vertex_kmer"], (name, factor, o)
                        assert rec["edge_removed"][raw["edge_off"][o]:raw["edge_off"][o + 1]].tolist() == x["edge_removed"], (name, factor, o)
                        gr = x["graph"]
                        edges = [(a, b, r, pm) for (a, b), r, pm in zip([e or (0, 0) for e in gr.edge], gr.is_ref, gr.pruning_multiplicity)]
                        want = P.prune(len(gr.node), edges, factor, P.OP_CONNECT, [int(not t) for t in gr.node], [int(e is None) for e in gr.edge])
                        v0, v1 = after["vertex_off"][o], after["vertex_off"][o + 1]
                        assert final["vertex_state"][v0:v1].tolist() == want["vertex_state"], (name, factor, o)
                        assert final["edge_state"][after["edge_off"][o]:after["edge_off"][o + 1]].tolist() == want["edge_state"], (name, factor, o)
                        assert final["n_vertices_left"][o] == want["n_vertices_left"] and final["n_edges_left"][o] == want["n_edges_left"]
                o += 1


def test_the_capacity_protocol(eng):
    graphs, cfg = SETS["golden_0"][0] + [g for g, _ in list(C.golden_graphs().values())[15:25]], R.Config(min_dangling_branch_length=1)
    regions, gd, masks, factor, _ = C.pack(graphs)
    with pytest.raises(PhmmError) as e:
        recover_dangling_ends(eng, regions, gd, masks, factor, capacity=(0, 0, 0), fill=0xAB, **kwargs(cfg))
    assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY
    need = e.value.required.tolist()
    assert all(n > 0 for n in need), need
    for name, out in e.value.outputs.items():                      # nothing but `required` written
        assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), name
    full = recover_dangling_ends(eng, regions, gd, masks, factor, capacity=need, **kwargs(cfg))
    same(full, C.expected(graphs, cfg), "capacity")
    for short in range(3):
        cap = list(need)
        cap[short] -= 1
        with pytest.raises(PhmmError) as e:
            recover_dangling_ends(eng, regions, gd, masks, factor, capacity=cap, fill=0xAB, **kwargs(cfg))
        assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and e.value.required.tolist() == need
        for name, out in e.value.outputs.items():
            assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), (short, name)


def test_no_graphs_and_graphs_without_ends(eng):
    o = recover_dangling_ends(eng, [], dict(k=np.zeros(0, np.uint32)), None, 2, fill=0xAB)
    assert o["required"].tolist() == [0, 0, 0] and o["end_off"].tolist() == [0]
    g = C.threaded(5, "ACGTTGCATTAGC", [])
    o = run(eng, [g, C.graph(5, [], [])], R.Config())
    assert o["required"].tolist() == [0, 0, 0] and o["n_rounds"].tolist() == [0, 0] and o["edge_removed"].tolist() == [0] * len(g["edges"])


# ---- PHMM_ERR_INVALID_ARG, every case the header names ---------------------------------------------------------------------------
def _arrays():
    return C.pack([C.tails_row(C.golden()["tails"]["rows"][0]), C.tails_row(C.golden()["tails"]["rows"][3])])


def _refused(eng, part, regions=None, gd=None, masks="given", factor="given", **kw):
    r0, g0, m0, f0, _ = _arrays()
    regions, gd = r0 if regions is None else regions, g0 if gd is None else gd
    with pytest.raises(PhmmError) as e:
        recover_dangling_ends(eng, regions, gd, m0 if masks == "given" else masks, f0 if factor == "given" else factor, fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and part in str(e.value), str(e.value)
    assert str(e.value).count("phmm_assembly_recover") == 1
    for name, out in e.value.outputs.items():                      # nothing written
        assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), name
    assert e.value.required is None or (e.value.required == np.frombuffer(b"\xab" * 12, np.uint32)).all()


@pytest.mark.parametrize("name", ["vertex_off", "edge_off", "vertex_seq", "vertex_pos", "edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity",
                                  "edge_pruning_multiplicity"])
def test_a_null_array_is_refused(eng, name):
    gd = dict(_arrays()[1])
    gd[name] = None
    _refused(eng, "a required pointer is NULL", gd=gd)
    assert name in eng.last_error()


def test_null_cfg_capacity_required_and_prune_factor_are_refused(eng):
    _refused(eng, "a required pointer is NULL (cfg)", omit=("cfg",))
    _refused(eng, "a required pointer is NULL (capacity, required)", omit=("capacity",))
    _refused(eng, "a required pointer is NULL (capacity, required)", omit=("required",))
    _refused(eng, "a required pointer is NULL (prune_factor)", factor=None)


@pytest.mark.parametrize("name", ["vertex_off", "edge_off"])
def test_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    gd = dict(_arrays()[1])
    gd[name] = gd[name].copy()
    gd[name][0] = 1
    _refused(eng, "%s does not start at 0" % name, gd=gd)
    gd = dict(_arrays()[1])
    gd[name] = gd[name].copy()
    gd[name][2] = gd[name][1] - 1
    _refused(eng, "graph 1: %s decreases" % name, gd=gd)


@pytest.mark.parametrize("name, word", [("edge_src", "source"), ("edge_dst", "target")])
def test_an_endpoint_outside_its_graph_is_refused(eng, name, word):
    gd = dict(_arrays()[1])
    gd[name] = gd[name].copy()
    nv = int(gd["vertex_off"][1])
    gd[name][0] = nv
    _refused(eng, "graph 0: edge 0: its %s %d reaches n_vertices (%d)" % (word, nv, nv), gd=gd)


def test_masks_are_given_together_and_a_present_edge_has_present_endpoints(eng):
    m = _arrays()[2]
    _refused(eng, "given together", masks=dict(vertex_absent=m["vertex_absent"], edge_absent=None))
    va = m["vertex_absent"].copy()
    va[int(_arrays()[1]["edge_src"][0])] = 1
    _refused(eng, "graph 0: edge 0: it is present and an endpoint is absent", masks=dict(vertex_absent=va, edge_absent=m["edge_absent"]))


def test_vertex_bytes_outside_their_sequence_are_refused(eng):
    gd = dict(_arrays()[1])
    gd["vertex_pos"] = gd["vertex_pos"].copy()
    gd["vertex_pos"][3] += 10 ** 6
    _refused(eng, "graph 0: vertex 3: its bytes", gd=gd)
    gd = dict(_arrays()[1])
    gd["vertex_seq"] = gd["vertex_seq"].copy()
    gd["vertex_seq"][2] = 1
    _refused(eng, "graph 0: vertex 2: its sequence 1 is not one of the region's (0 reads)", gd=gd)


def test_ops_num_pruning_samples_and_cyclic_graphs_are_refused(eng):
    _refused(eng, "ops is 0", ops=0)
    _refused(eng, "ops has unknown bits (4)", ops=4)
    _refused(eng, "num_pruning_samples (0) is outside", num_pruning_samples=0)
    _refused(eng, "num_pruning_samples (9) is outside", num_pruning_samples=9)
    m = dict(_arrays()[2], graph_flags=np.array([0, _lib.PHMM_PRUNE_HAS_CYCLE], np.uint32))
    _refused(eng, "graph 1: it is flagged cyclic", masks=m)


@pytest.mark.parametrize("k", [0, 256])
def test_k_outside_its_range_is_refused(eng, k):
    gd = dict(_arrays()[1], k=np.array([k], np.uint32))
    _refused(eng, "k[0] = %d is outside 1 .. 255" % k, gd=gd)


@pytest.mark.parametrize("name", ["region_ref_off", "region_read_off"])
def test_region_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    from lorikeet_amd.assembly import pack
    regions = pack(_arrays()[0])
    regions[name] = regions[name].copy()
    regions[name][0] = 1
    _refused(eng, "%s does not start at 0" % name, regions=regions)
    regions = pack(_arrays()[0])
    regions[name] = regions[name].copy()
    regions[name][1], regions[name][2] = 5, 4
    _refused(eng, "region 1: %s decreases" % name, regions=regions)


def test_a_read_window_outside_its_read_is_refused(eng):
    from lorikeet_amd.assembly import pack
    regions = pack(_arrays()[0])
    regions.update(region_read_off=np.array([0, 1, 1], np.uint32), read_off=np.array([0, 4], np.uint32), read_bases=np.frombuffer(b"ACGT", np.uint8),
                   read_quals=np.frombuffer(b"IIII", np.uint8))
    _refused(eng, "read 0: its window leaves the read", regions=regions, read_first=[2], read_len=[3])
    _refused(eng, "read_first and read_len are given together", regions=regions, read_first=[2])
    bad = dict(regions, read_off=np.array([1, 4], np.uint32))
    _refused(eng, "read_off does not start at 0", regions=bad)


def test_a_graph_above_the_vertex_limit_is_refused(eng):
    regions, gd, masks, factor, _ = C.pack([C.tails_row(C.golden()["tails"]["rows"][0])])
    n = 30001
    gd = dict(gd, vertex_off=np.array([0, n], np.uint32), vertex_seq=np.zeros(n, np.uint32), vertex_pos=np.zeros(n, np.uint32))
    _refused(eng, "graph 0: more than 30000 vertices", regions=regions, gd=gd, masks=None, factor=factor)


def test_weights_that_overflow_the_references_sums_are_refused(eng):
    _refused(eng, "reach 1e9", sw_parameters=(100000000, -50, -110, -6))
    _refused(eng, "reach 1e9", sw_parameters=(25, -50, -(2 ** 31), -6))


@pytest.mark.parametrize("name", ["end_vertex", "end_cigar", "new_edge_src", "new_vertex_kmer"])
def test_a_capacity_above_0_whose_arrays_are_null_is_refused(eng, name):
    """decided behind the kernel, once the sizes are known: still nothing is written, `required` included"""
    graphs, cfg = [g for g, _ in list(C.golden_graphs().values())[15:25]], R.Config(min_dangling_branch_length=1)
    regions, gd, masks, factor, _ = C.pack(graphs)
    need = recover_dangling_ends(eng, regions, gd, masks, factor, **kwargs(cfg))["required"]
    assert all(int(n) > 0 for n in need)
    with pytest.raises(PhmmError) as e:
        recover_dangling_ends(eng, regions, gd, masks, factor, capacity=need, fill=0xAB, omit=(name,), **kwargs(cfg))
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and "a capacity above 0 whose arrays are NULL" in str(e.value)
    for nm, out in e.value.outputs.items():
        assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), nm
    assert (e.value.required == np.frombuffer(b"\xab" * 12, np.uint32)).all()
