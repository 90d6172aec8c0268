"""The aligner inside phmm_assembly_recover (fill_matrix, walk_back and the merge arithmetic behind them) on the MI355X against the
serial restatement, on the planted strings of tests/assembly_recover_planted_cases.py: every pair of short strings over two
letters as tails and as heads, the reference's own Smith-Waterman strings, and strings past one 64-cell pass with long gaps,
under nine weight sets and the crosses of min_dangling_branch_length, min_matching_bases and max_mismatches_in_dangling_head.
EQUALITY on every array of assembly_recover_cases.OUTPUTS: integers and bytes, no tolerance.  Each graph holds one end, so
n_rounds is 1 per graph.  tests/test_assembly_recover_planted_table.py proves on the CPU that the graphs hand over the planted
strings and which rules of the aligner they reach."""
import random

import numpy as np
import pytest

import assembly_recover_cases as C
import assembly_recover_planted_cases as PC
from lorikeet_amd.assembly import recover_dangling_ends

pytestmark = pytest.mark.gpu
GROUPS = {g["name"]: g for g in PC.groups()}
_packed, _results = {}, {}


@pytest.fixture(scope="module")
def eng():
    from lorikeet_amd.engine import HipPairHMMEngine
    e = HipPairHMMEngine()
    yield e
    e.close()


def kwargs(cfg):
    return dict(ops=cfg.ops, min_dangling_branch_length=cfg.min_dangling_branch_length, min_matching_bases=cfg.min_matching_bases,
                max_mismatches_in_dangling_head=cfg.max_mismatches_in_dangling_head, num_pruning_samples=cfg.num_pruning_samples, sw_parameters=cfg.sw)


def run(eng, graphs, cfg, **kw):
    if id(graphs) not in _packed:                                  # (a family's groups share one list of graphs per k)
        _packed[id(graphs)] = (graphs, C.pack(graphs))
    regions, gd, masks, factor, _ = _packed[id(graphs)][1]
    return recover_dangling_ends(eng, regions, gd, masks, factor, **dict(kwargs(cfg), **kw))


def in_group(eng, g):
    """the group's graphs in ONE call, fill 0xAB; kept for the tests that compare against it"""
    if g["name"] not in _results:
        _results[g["name"]] = run(eng, g["graphs"], g["cfg"], fill=0xAB)
    return _results[g["name"]]


def names_the_member(g, got, want):
    """the first member whose rows differ: its strings, weights, options, the device's CIGAR and the oracle's"""
    n = len(g["members"])
    if got["end_off"].tolist() != list(range(n + 1)):
        bad = next(i for i in range(n) if i + 1 >= len(got["end_off"]) or got["end_off"][i + 1] - got["end_off"][i] != 1)
        return "member %d has no single end on the device: %s" % (bad, PC.describe(g["members"][bad], g["cfg"]))
    for i, m in enumerate(g["members"]):
        for name in C.PER_END + C.PER_GRAPH:
            if name in C.PER_END and not np.array_equal(got[name][i], want[name][i]) or name in C.PER_GRAPH and got[name][i] != want[name][i]:
                return "member %d differs in %s (device %s, restatement %s): %s" % (
                    i, name, got[name][i].tolist(), want[name][i].tolist(), PC.describe(m, g["cfg"], got["end_cigar"][i], got["end_n_cigar"][i]))
    return "no member's own rows differ"


def same(got, want, g):
    for name in C.OUTPUTS:
        a, b = got[name], want[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (g["name"], name, a.dtype, a.shape, b.dtype, b.shape, names_the_member(g, got, want))
        assert np.array_equal(a, b), (g["name"], name, np.argwhere(a != b)[:5].tolist(), names_the_member(g, got, want))


@pytest.mark.parametrize("name", list(GROUPS))
def test_a_group_equals_the_restatement(eng, name):
    """one (family, weight set, k, option tuple) group in one call"""
    g = GROUPS[name]
    got = in_group(eng, g)
    same(got, C.expected(g["graphs"], g["cfg"]), g)
    assert (got["n_rounds"] == 1).all(), np.flatnonzero(got["n_rounds"] != 1)[:8]


def _picked(family):
    """the first and the last member of the family's groups and 62 seeded ones between: (group, index)"""
    every = [(g, i) for g in PC.family(family) for i in range(len(g["members"]))]
    rng = random.Random(97 + ord(family))
    return [every[0], every[-1]] + [every[j] for j in sorted(rng.sample(range(1, len(every) - 1), 62))]


@pytest.mark.parametrize("family", PC.FAMILIES)
def test_members_alone_equal_their_rows_in_the_group_call(eng, family):
    picked = _picked(family)
    assert len(picked) == 64
    for g, i in picked:
        m, first = g["members"][i], in_group(eng, g)
        alone = recover_dangling_ends(eng, *C.pack([m["graph"]])[:4], **kwargs(g["cfg"]), fill=0xAB)
        tag = (g["name"], i, PC.describe(m, g["cfg"], alone["end_cigar"][0] if len(alone["end_cigar"]) else None, alone["end_n_cigar"][0] if len(alone["end_n_cigar"]) else 0))
        same_one = C.expected([m["graph"]], g["cfg"])
        for name in C.OUTPUTS:
            assert np.array_equal(alone[name], same_one[name]), (name, tag)
        assert alone["n_rounds"].tolist() == [1] and first["n_rounds"][i] == 1, tag
        for name in C.PER_GRAPH:
            assert first[name][i] == alone[name][0], (name, tag)
        for names, off in ((C.PER_END, "end_off"), (C.PER_EDGE, "new_edge_off")):
            for name in names:
                assert first[name][first[off][i]:first[off][i + 1]].tobytes() == alone[name].tobytes(), (name, tag)
        v0, v1 = first["new_vertex_off"][i], first["new_vertex_off"][i + 1]
        assert np.array_equal(first["new_vertex_kmer"][v0:v1], alone["new_vertex_kmer"]), tag
        e0 = sum(len(x["edges"]) for x in g["graphs"][:i])
        assert first["edge_removed"][e0:e0 + len(m["graph"]["edges"])].tobytes() == alone["edge_removed"].tobytes(), tag


@pytest.mark.parametrize("family", PC.FAMILIES)
def test_a_second_run_with_another_fill_byte_is_the_same_byte_for_byte(eng, family):
    """the family's largest group at STANDARD_NGS and the default options"""
    g = max((g for g in PC.family(family) if g["weights"] == "STANDARD_NGS" and g["cfg"].key() == PC.config("STANDARD_NGS").key()),
            key=lambda g: len(g["members"]))
    first, again = in_group(eng, g), run(eng, g["graphs"], g["cfg"], fill=0xCD)
    for name in C.OUTPUTS + ("n_rounds",):
        assert first[name].tobytes() == again[name].tobytes(), (g["name"], name)
