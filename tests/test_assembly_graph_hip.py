"""phmm_assembly_graph on the MI355X against the SERIAL restatement of the reference's read-threading graph
(tests/assembly_graph_restatement.py), through the C ABI as lorikeet_amd.assembly binds it.  EQUALITY on every output array,
vertex and edge indices included: it is all integers and bytes, there are no tolerances.  The regions come from
tests/assembly_graph_cases.py; tests/test_assembly_graph_oracle.py holds the restatement to the reference's literals and to
hand-derived expectations and counts on the CPU what the sets reach.  Every comparison runs twice: with the tables' fingerprints
whole and cut to 4 bits (switch asm_fingerprint_bits), where sixteen fingerprints serve every key, so probing and the byte
comparisons decide.  The module takes assembly_graph from lorikeet_amd.assembly at the top: without the call every test here
fails."""
import random

import numpy as np
import pytest

import assembly_graph_cases as G
import finalize_cases as FK
from lorikeet_amd import _lib, assembly, finalize
from lorikeet_amd.assembly import assembly_graph
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
CALLS = G.calls()
ARRAYS = G.SIZES + G.OFFSETS + G.VERTEX + G.EDGE + ("ref_path",) + G.PLANES


@pytest.fixture(scope="module", params=[0, 4], ids=["fp64", "fp4"])
def eng(request):
    e = HipPairHMMEngine()
    e.set_switch("asm_fingerprint_bits", request.param)
    yield e
    e.close()


def run(eng, c, windows=None, **kw):
    regions = [(g["ref"], g["reads"]) for g in c["regions"]]
    first = length = None
    if windows is not None:
        first = [f for w in windows for f, _ in w]
        length = [n for w in windows for _, n in w]
    return assembly_graph(eng, regions, c["k"], c["min_q"], read_first=first, read_len=length, read_sample=G.samples_of(c),
                          num_pruning_samples=c["nps"], **kw)


def same(got, want, tag, planes=True):
    for name in ARRAYS:
        g, w = got[name], want[name]
        if name in G.PLANES and not planes:
            assert g is None, (tag, name)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_equals_the_restatement(eng, name):
    """each set in a call of its own: the k-mer stage's sets, the golden literals and the hand cases one region per call and
    all in one, the pass boundaries, the repeats, the reference source, the backward walks, every k, the sequence counts with
    every num_pruning_samples, the sample limit, the seeded regions, REF_SHORT beside healthy regions"""
    same(run(eng, CALLS[name], fill=0xAB), G.expected(CALLS[name]), name)


@pytest.mark.parametrize("name", ["every_k", "kmers_eight_k", "seeded", "group_order"])
def test_a_call_with_several_k_equals_each_k_alone(eng, name):
    c = CALLS[name]
    many = run(eng, c)
    n_regions = len(c["regions"])
    for i, k in enumerate(c["k"]):
        alone = run(eng, G.call(c["regions"], [k], c["min_q"], c["nps"]))
        for out in G.SIZES + G.PLANES:
            assert np.array_equal(many[out][i], alone[out][0]), (name, k, out)
        for names, off in ((G.VERTEX, "vertex_off"), (G.EDGE, "edge_off"), (("ref_path",), "ref_path_off")):
            lo, hi = many[off][i * n_regions], many[off][(i + 1) * n_regions]
            assert np.array_equal(many[off][i * n_regions:(i + 1) * n_regions + 1] - lo, alone[off]), (name, k, off)
            for out in names:
                assert np.array_equal(many[out][lo:hi], alone[out]), (name, k, out)


def test_a_region_of_a_batch_equals_the_same_region_alone_and_a_second_call(eng):
    c = CALLS["seeded"]
    first, again = run(eng, c), run(eng, c)
    for out in ARRAYS:
        assert first[out].tobytes() == again[out].tobytes(), out
    n_regions = len(c["regions"])
    ro, po = first["region_ref_off"], first["read_off"][first["region_read_off"]]
    for g in (0, 7, n_regions - 1):
        alone = run(eng, G.call([c["regions"][g]], c["k"], c["min_q"], c["nps"]))
        for out in G.SIZES:
            assert np.array_equal(first[out][:, g], alone[out][:, 0]), (g, out)
        for out, off in (("ref_vertex", ro), ("read_vertex", po)):
            assert first[out][:, off[g]:off[g + 1]].tobytes() == alone[out].tobytes(), (g, out)
        for i in range(len(c["k"])):
            o = i * n_regions + g
            for names, off in ((G.VERTEX, "vertex_off"), (G.EDGE, "edge_off"), (("ref_path",), "ref_path_off")):
                for out in names:
                    assert first[out][first[off][o]:first[off][o + 1]].tobytes() == alone[out][alone[off][i]:alone[off][i + 1]].tobytes(), (g, i, out)


def _windows(c, seed):
    rng = random.Random(seed)
    out = []
    for g in c["regions"]:
        w = []
        for b, _ in g["reads"]:
            f = rng.randrange(len(b) + 1)
            w.append((f, rng.randrange(len(b) - f + 1)) if rng.randrange(4) else (0, len(b)))
        out.append(w)
    return out


@pytest.mark.parametrize("name", ["seeded", "backward_walk", "kmers_pass_boundaries"])
def test_windows_equal_the_same_reads_cut_beforehand(eng, name):
    c = CALLS[name]
    w = _windows(c, 3)
    got = run(eng, c, windows=w, fill=0xAB)
    same(got, G.expected(c, windows=w), name)
    cut = G.call([dict(g, reads=[(b[f:f + n], q[f:f + n]) for (b, q), (f, n) in zip(g["reads"], wg)]) for g, wg in zip(c["regions"], w)],
                 c["k"], c["min_q"], c["nps"])
    pre = run(eng, cut)
    for out in ARRAYS:
        if out != "read_vertex":
            assert np.array_equal(got[out], pre[out]), out
    inside = np.zeros(got["read_vertex"].shape[1], bool)
    at = 0
    for g, wg in zip(c["regions"], w):
        for (b, _), (f, n) in zip(g["reads"], wg):
            inside[at + f:at + f + n] = True
            at += len(b)
    assert np.array_equal(got["read_vertex"][:, inside], pre["read_vertex"])
    assert (got["read_vertex"][:, ~inside] == 0xFFFFFFFF).all()


def test_the_output_of_finalize_reads_feeds_the_call_with_no_base_copied(eng):
    """one small group: soft clips, low-quality tails and a span that cuts -- clip_first / clip_len and out_quals go in as they
    came out, and the answer is the restatement's on the reads cut by hand"""
    ref = G.bases(random.Random(5), 60)
    reads = [FK.read("5S40M5S", pos=100, bases=ref[:50], quals=30), FK.read("50M", pos=95, bases=ref[5:55], quals=[2] * 4 + [30] * 40 + [2] * 6),
             FK.read("30M", pos=110, bases=ref[20:50], quals=30), FK.read("20M", pos=400, bases=ref[:20], quals=30)]
    fin = finalize.finalize_reads(eng, [FK.group(reads, span=(104, 140))])
    packed = finalize.pack([FK.group(reads, span=(104, 140))])
    keep = fin.keep.astype(bool)
    first, length = np.where(keep, fin.clip_first, 0), np.where(keep, fin.clip_len, 0)
    assert keep.any() and not keep.all() and (length[keep] < np.diff(packed["read_off"])[keep]).any()
    arrays = dict(region_ref_off=np.array([0, len(ref)], np.uint32), ref_bases=np.frombuffer(ref, np.uint8), region_read_off=np.array([0, len(reads)], np.uint32),
                  read_off=packed["read_off"], read_bases=packed["read_bases"], read_quals=fin.out_quals)
    got = assembly_graph(eng, arrays, [5, 10], read_first=first, read_len=length, read_sample=[1, 0, 1, 0], fill=0xAB)
    whole = [(bytes(r["bases"]), bytes(fin.quals(i))) for i, r in enumerate(reads)]
    c = G.call([dict(ref=ref, reads=whole, samples=[1, 0, 1, 0])], [5, 10])
    same(got, G.expected(c, windows=[list(zip(first.tolist(), length.tolist()))]), "chain")


def test_without_the_planes_the_other_arrays_are_the_same(eng):
    c = CALLS["seeded"]
    same(run(eng, c, planes=False, fill=0xAB), G.expected(c), "no planes", planes=False)


def test_no_region_and_regions_without_reads(eng):
    got = run(eng, G.call([], [3]))
    assert got["flags"].shape == (1, 0) and got["vertex_off"].tolist() == [0] and got["required"].tolist() == [0, 0, 0]
    c = G.call([G.region("ACGTTGCA"), G.region(""), G.region("AC", ["ACGT"])], [3, 4])
    same(run(eng, c, fill=0xAB), G.expected(c), "no reads")


# ---- the capacity protocol --------------------------------------------------------------------------------------------------------
def test_capacities_all_zero_exact_one_too_few_and_more_than_needed(eng):
    c = CALLS["backward_walk"]
    want = G.expected(c)
    need = [len(want["vertex_seq"]), len(want["edge_src"]), len(want["ref_path"])]
    with pytest.raises(PhmmError) as e:
        run(eng, c, capacity=(0, 0, 0), fill=0xAB)
    assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and e.value.required.tolist() == need
    same(run(eng, c, capacity=need, fill=0xAB), want, "exact")
    for i in range(3):
        cap = list(need)
        cap[i] -= 1
        with pytest.raises(PhmmError) as e:
            run(eng, c, capacity=cap, fill=0xAB)
        assert e.value.code == _lib.PHMM_ERR_EVENT_CAPACITY and e.value.required.tolist() == need, i
        assert "capacity %d is %d, %d needed" % (i, cap[i], need[i]) in str(e.value)
        for name, a in e.value.outputs.items():                  # nothing else written
            assert (np.frombuffer(a.tobytes(), np.uint8) == 0xAB).all(), (i, name)
    roomy = run(eng, c, capacity=[n + 7 for n in need], fill=0xAB)
    same(roomy, want, "more than needed")


# ---- PHMM_ERR_INVALID_ARG, every case the header names ---------------------------------------------------------------------------
def _arrays():
    return assembly.pack([(b"ACGTTGCA", [G.read("ACGTAC"), G.read("TTGCAT")]), (b"GATTCCAGT", [G.read("GATTC")])])


def _refused(eng, arrays, k=(3,), part=None, **kw):
    with pytest.raises(PhmmError) as e:
        assembly_graph(eng, arrays, list(k), fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and (part is None or part in str(e.value)), str(e.value)
    assert str(e.value).count("phmm_assembly_graph") == 1
    for name, a in e.value.outputs.items():                      # nothing written
        assert (np.frombuffer(a.tobytes(), np.uint8) == 0xAB).all(), name
    assert (e.value.required == 0xABABABAB).all()


@pytest.mark.parametrize("name", ["region_ref_off", "region_read_off", "read_off"])
def test_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    a = _arrays()
    a[name] = a[name].copy()
    a[name][0] = 1
    _refused(eng, a, part="does not start at 0")
    a = _arrays()
    a[name] = a[name].copy()
    a[name][1] = a[name][2] + 1
    _refused(eng, a, part="decreases")


def test_a_window_outside_its_read_is_refused(eng):
    a = _arrays()
    _refused(eng, a, read_first=[0, 0, 0], read_len=[6, 7, 5], part="window")
    _refused(eng, a, read_first=[0, 7, 0], read_len=[6, 0, 5], part="window")
    _refused(eng, a, read_first=[0, 0, 0], part="together")
    _refused(eng, a, read_len=[6, 6, 5], part="together")


def test_k_and_n_k_out_of_range_or_not_ascending_are_refused(eng):
    a = _arrays()
    _refused(eng, a, k=(0,), part="k[0]")
    _refused(eng, a, k=(3, _lib.PHMM_ASM_MAX_K + 1), part="k[1]")
    _refused(eng, a, k=(3, 3), part="ascending")
    _refused(eng, a, k=(), part="n_k")
    _refused(eng, a, k=tuple(range(1, _lib.PHMM_ASM_MAX_K_VALUES + 2)), part="n_k")
    _refused(eng, a, min_base_quality=256, part="min_base_quality")


def test_sequences_above_their_limits_are_refused(eng):
    long_ref = assembly.pack([(b"A" * (_lib.PHMM_ASM_MAX_REF_BASES + 1), [])])
    _refused(eng, long_ref, part="region 0: more than %d reference bases" % _lib.PHMM_ASM_MAX_REF_BASES)
    long_read = assembly.pack([(b"ACGT", [G.read(b"A" * (_lib.PHMM_ASM_MAX_READ_BASES + 1))])])
    _refused(eng, long_read, part="read 0: more than %d bases" % _lib.PHMM_ASM_MAX_READ_BASES)


def test_num_pruning_samples_outside_its_range_is_refused(eng):
    _refused(eng, _arrays(), num_pruning_samples=0, part="num_pruning_samples")
    _refused(eng, _arrays(), num_pruning_samples=_lib.PHMM_GRAPH_MAX_PRUNING_SAMPLES + 1, part="num_pruning_samples")


def test_one_sample_more_than_the_limit_in_a_region_is_refused(eng):
    n = _lib.PHMM_GRAPH_MAX_SAMPLES + 1
    a = assembly.pack([(b"ACGTTGCA", [G.read("ACGTAC")]), (b"GATTCCAGT", [G.read("GATTC")] * n)])
    _refused(eng, a, read_sample=[0] + list(range(n)), part="region 1: more than %d samples" % _lib.PHMM_GRAPH_MAX_SAMPLES)
    assert assembly_graph(eng, a, [3], read_sample=[0] + [i % (n - 1) for i in range(n)])["n_vertices"].shape == (1, 2)


def test_missing_arrays_a_lone_plane_and_offsets_without_data_are_refused(eng):
    for name in ("region_ref_off", "ref_bases", "region_read_off", "read_off", "read_bases", "read_quals"):
        a = _arrays()
        a[name] = None
        _refused(eng, a, part="NULL")
    for name in G.SIZES + G.OFFSETS + ("capacity",):
        _refused(eng, _arrays(), omit=(name,), part="NULL")
    _refused(eng, _arrays(), omit=("ref_vertex",), part="together")
    _refused(eng, _arrays(), omit=("read_vertex",), part="together")
    for name in G.VERTEX + G.EDGE + ("ref_path",):
        _refused(eng, _arrays(), capacity=(64, 64, 64), omit=(name,), part="no data")


def test_bases_times_n_k_above_the_positions_limit_is_refused(eng):
    """as for phmm_assembly_kmers: the call refuses before it reads a base, so the base and quality arrays are small"""
    n_reads, n = 4097, _lib.PHMM_ASM_MAX_READ_BASES
    k = np.arange(1, _lib.PHMM_ASM_MAX_K_VALUES + 1, dtype=np.uint32)
    read_off = (np.arange(n_reads + 1, dtype=np.uint64) * n).astype(np.uint32)
    dummy = np.full(64, 0x41, np.uint8)
    a = dict(region_ref_off=np.zeros(2, np.uint32), ref_bases=dummy, region_read_off=np.array([0, n_reads], np.uint32), read_off=read_off,
             read_bases=dummy, read_quals=dummy)
    _refused(eng, a, k=k, planes=False, part="bases x n_k is above %d" % _lib.PHMM_ASM_MAX_POSITIONS)
