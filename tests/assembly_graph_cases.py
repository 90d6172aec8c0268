"""The regions tests/test_assembly_graph_oracle.py (CPU) and tests/test_assembly_graph_hip.py (GPU) share, and the serial
restatement's answer (tests/assembly_graph_restatement.py) in the layout of phmm_assembly_graph's outputs.  A region is
dict(ref=bytes, reads=[(bases, quals), ...], samples=[value per read] or absent); a call is dict(regions, k, min_q, nps).
The k-mer stage's sets (tests/assembly_kmers_cases.py) are graph cases too: every one of them runs here as well."""
import json
import os
import random

import numpy as np

import assembly_graph_restatement as R
import assembly_kmers_cases as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_graph_cases.json")
MAX_SAMPLES, MAX_PRUNING_SAMPLES = 64, 8      # PHMM_GRAPH_MAX_SAMPLES, PHMM_GRAPH_MAX_PRUNING_SAMPLES
SIZES = ("flags", "n_vertices", "n_edges", "n_ref_path")
OFFSETS = ("vertex_off", "edge_off", "ref_path_off")
VERTEX = ("vertex_seq", "vertex_pos", "vertex_flags")
EDGE = ("edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity", "edge_pruning_multiplicity")
PLANES = ("ref_vertex", "read_vertex")
read, bases = K.read, K.bases


def region(ref, reads=(), samples=None):
    g = K.region(ref, reads)
    if samples is not None:
        assert len(samples) == len(g["reads"])
        g["samples"] = list(samples)
    return g


def call(regions, k, min_q=10, nps=1):
    return dict(regions=list(regions), k=sorted(k), min_q=min_q, nps=nps)


def golden():
    return json.load(open(GOLDEN))


def golden_regions():
    """the literals as regions in default mode (the reference a group of its own, as create_graph adds it)"""
    out = {}
    for name, c in golden().items():
        if "sequences" in c:
            out[name] = (region(c["reference"], c["sequences"]), c["k"])
    return out


def cycle_region():
    c = golden()["test_cycles_in_graph"]
    alt = c["alternate"].encode()
    reads = [read(alt[i:i + c["read_length"]], q=c["quality"]) for i in range(0, len(alt) - c["read_length"], c["step"])]
    return region(c["reference"], reads), c


# ---- one region per quirk, small enough to derive by hand (tests/test_assembly_graph_oracle.py does) ---------------------------
def walk_offset_counts_from_the_sequence_start():
    """k = 3.  The read's run starts at 2 (a low-quality base at 1) and threading starts there, on GTC, which the reference
    gave one in-edge (TGT -> GTC).  The walk compares TGT's suffix T with sequence[1] -- the read's byte at offset k - 2 of
    the WHOLE sequence, the low-quality A, not the byte before the start: no step.  Cut to the run, the same read walks."""
    return region("CTGTCAAG", [read("CAGTCAAG", low=(1,))])


def the_same_read_cut_to_its_run():
    return region("CTGTCAAG", ["GTCAAG"])


def source_kmer_again_in_a_read():
    """k = 3: GAT is the reference's first k-mer; the read meets it again behind TCC -- a fresh vertex, not the source's"""
    return region("GATTCCAGT", ["TTCCGATTC"])


def source_kmer_starts_a_read():
    return region("GATTCCAGT", ["GATTCC"])


def reference_of_exactly_k():
    """k = 4: the reference threads nothing and leaves no ref_source; the read's ACGT is an ordinary tracked vertex"""
    return region("ACGT", ["ACGTTACGTC"])


def second_group_creates_an_edge():
    """k = 3, two samples: the second sample's read leaves the reference at a SNP; its edges do not see the first group's flush"""
    return region("GATTCCAGTA", ["GATTCCAGTA", "GATTGCAGTA"], samples=[5, 2])


def group_order_differs_between_k():
    """sample 9 comes first in the input with a read of 5 bases: it leads at k = 3 and yields nothing at k = 6, where sample 4
    leads"""
    return region("GATTCCAGTACG", ["ATTCC", "GATTCCAGTACG", "TTCCAGTA", "TCCAGTACG"], samples=[9, 4, 9, 4])


def hand():
    return {"walk_offset": (walk_offset_counts_from_the_sequence_start(), 3), "walk_cut": (the_same_read_cut_to_its_run(), 3),
            "source_again": (source_kmer_again_in_a_read(), 3), "source_start": (source_kmer_starts_a_read(), 3),
            "reference_of_k": (reference_of_exactly_k(), 4), "second_group": (second_group_creates_an_edge(), 3)}


# ---- the smallest shapes at which the kernels can go wrong -------------------------------------------------------------------------
def lengths():
    """reads and references of 63, 64, 65, 128, 129 bases, the reads the reference with two SNPs"""
    rng = random.Random(31)
    out = []
    for n in (63, 64, 65, 128, 129):
        ref = bases(rng, n)
        reads = []
        for _ in range(3):
            b = bytearray(ref)
            for _ in range(2):
                b[rng.randrange(n)] = rng.choice(b"ACGT")
            reads.append(read(b))
        out.append(region(ref, reads))
    return call(out, [4, 10])


def repeats():
    """k = 5 over (AC)n: a run of non-unique k-mers that starts at 50, in the first 64-position pass, and ends in the second,
    its anchor at 49; two reads through a shorter repeat from the same anchor (one trie branch, weights 2); two more whose base
    in front of the repeat differs, so that equal bytes hang off different anchors; and a non-unique k-mer at reference position 0"""
    rng = random.Random(37)
    head, tail = bases(rng, 50, b"GT") + b"G", bases(rng, 40, b"GT")
    ref = head + b"AC" * 15 + tail
    short = head + b"AC" * 12 + tail
    other = bytearray(short)
    other[50] = ord("T")
    third = bytearray(short)
    third[49] = ord("A") if short[49] != ord("A") else ord("C")
    first = region(ref, [short, short, bytes(other), bytes(third), ref[30:]])
    at_zero = region(b"ACACAC" + bases(rng, 30, b"GT"), ["ACACACGT", b"CACAC" + bases(rng, 10, b"GT")])
    return call([first, at_zero], [3, 5])


def reference_source():
    rng = random.Random(41)
    ref = bases(rng, 60)
    src = ref[:10]
    again_in_ref = ref[:30] + src + ref[30:]
    return call([region(ref, [ref[10:30] + src + ref[30:50], ref[:40], ref[5:45]]), region(again_in_ref, [again_in_ref[5:60]])], [10])


def backward_walk():
    """A starts on the reference's vertex at 20, which has one in-edge when A is threaded; B brings it a second.  A before B: A
    walks the full k - 1 steps.  B before A: it does not.  C's run starts above 0, so its walk reads the wrong bytes and stops"""
    rng = random.Random(43)
    ref = bases(rng, 80)
    a = ref[20:60]
    b = bases(rng, 20) + ref[20:60]
    c = read(ref[10:16] + b"N" + ref[17:70])
    d = read(bases(rng, 4) + ref[24:64], low=(2,))
    return call([region(ref, [a, b, c, d]), region(ref, [b, a, c, d]), region(ref, [a, a, b, a])], [2, 3, 10, 25])


def every_k():
    c = K.every_k((1, 2, 3, 10, 25, 64, 255))
    return call(c["regions"], c["k"], c["min_q"])


def many_sequences():
    """1, 63, 64, 65 and 130 sequences in a region (the reference is one), three samples interleaved"""
    rng = random.Random(47)
    out = []
    for n in (0, 62, 63, 64, 129):
        ref = bases(rng, 40)
        reads, samples = [], []
        for i in range(n):
            at = rng.randrange(0, 25)
            b = bytearray(ref[at:at + rng.randrange(8, 16)])
            if i % 5 == 0:
                b[rng.randrange(len(b))] = rng.choice(b"ACGT")
            reads.append(read(b))
            samples.append((11, 3, 700000)[rng.randrange(3)])
        out.append(region(ref, reads, samples))
    return out


def sample_limit():
    rng = random.Random(53)
    ref = bases(rng, 30)
    reads = [read(ref[i % 10:i % 10 + 15]) for i in range(MAX_SAMPLES + 6)]
    return region(ref, reads, samples=[1000 - (i % MAX_SAMPLES) for i in range(MAX_SAMPLES + 6)])


def seeded(n_regions=24, seed=59):
    c = K.seeded(n_regions, seed)
    rng = random.Random(seed)
    for g in c["regions"]:
        g["samples"] = [rng.choice((0, 1, 2, 0xFFFFFFFF)) for _ in g["reads"]]
    return call(c["regions"], c["k"], c["min_q"])


def calls():
    """name -> call: every set the GPU file runs"""
    out = {"kmers_" + name: call(c["regions"], c["k"], c["min_q"]) for name, c in K.calls().items()}
    for name, (reg, k) in list(golden_regions().items()) + list(hand().items()):
        out[name] = call([reg], [k])
    out["group_order"] = call([group_order_differs_between_k()], [3, 6])
    everything = [reg for reg, _ in list(golden_regions().values()) + list(hand().values())] + [group_order_differs_between_k()]
    out["golden_and_hand_in_one_call"] = call(everything, [2, 3, 11], nps=2)
    out["lengths"] = lengths()
    out["repeats"] = repeats()
    out["reference_source"] = reference_source()
    out["backward_walk"] = backward_walk()
    out["every_k"] = every_k()
    for nps in (1, 2, MAX_PRUNING_SAMPLES):
        out["many_sequences_nps%d" % nps] = call(many_sequences(), [5, 10], nps=nps)
    out["sample_limit"] = call([sample_limit()], [5], nps=3)
    out["seeded"] = seeded()
    out["ref_short_beside_healthy"] = call([region("ACGTTGCA", ["ACGTTG"]), region("ACG", ["ACGTACGTAC"]), region("", ["ACGT"]),
                                            region("ACGACGTT", ["ACGACG"]), region("ACGTTGCATT")], [3, 5])
    return out


# ---- the restatement's answer in the call's layout ------------------------------------------------------------------------------
_memo = {}


def one(reg, k, min_q, nps):
    key = (reg["ref"], tuple(reg["reads"]), tuple(reg.get("samples") or ()), k, min_q, nps)
    if key not in _memo:
        _memo[key] = R.graph(reg["ref"], reg["reads"], k, min_q, reg.get("samples"), nps)
    return _memo[key]


def samples_of(c):
    """read_sample for the call, or None when no region names samples"""
    if not any("samples" in g for g in c["regions"]):
        return None
    return [s for g in c["regions"] for s in g.get("samples", [0] * len(g["reads"]))]


def expected(c, windows=None):
    """The output arrays of a call, from the restatement.  windows: per region and read (first, len) -- the restatement gets the
    cut reads, and their plane entries lie at the windows' places among the uncut bases."""
    regions, ks = c["regions"], c["k"]
    n_ref = sum(len(g["ref"]) for g in regions)
    n_read = sum(len(b) for g in regions for b, _ in g["reads"])
    n_graphs = len(ks) * len(regions)
    o = {name: np.zeros((len(ks), len(regions)), np.uint32) for name in SIZES}
    o.update(ref_vertex=np.full((len(ks), n_ref), R.NO_VERTEX, np.uint32), read_vertex=np.full((len(ks), n_read), R.NO_VERTEX, np.uint32))
    vertices, edges, path, offs = [], [], [], {name: [0] for name in OFFSETS}
    for i, k in enumerate(ks):
        at_ref = at_read = 0
        for gi, g in enumerate(regions):
            cut = g
            if windows is not None:
                cut = dict(g, reads=[(b[f:f + n], q[f:f + n]) for (b, q), (f, n) in zip(g["reads"], windows[gi])])
            x = one(cut, k, c["min_q"], c["nps"])
            o["flags"][i, gi], o["n_vertices"][i, gi], o["n_edges"][i, gi], o["n_ref_path"][i, gi] = x["flags"], len(x["vertices"]), len(x["edges"]), len(x["ref_path"])
            vertices += x["vertices"]
            edges += x["edges"]
            path += x["ref_path"]
            for name, n in zip(OFFSETS, (len(vertices), len(edges), len(path))):
                offs[name].append(n)
            o["ref_vertex"][i, at_ref:at_ref + len(g["ref"])] = x["ref_vertex"]
            at_ref += len(g["ref"])
            for ri, (b, _) in enumerate(g["reads"]):
                f, n = (0, len(b)) if windows is None else windows[gi][ri]
                o["read_vertex"][i, at_read + f:at_read + f + n] = x["read_vertex"][ri]
                at_read += len(b)
    assert len(offs["vertex_off"]) == n_graphs + 1
    for name in OFFSETS:
        o[name] = np.asarray(offs[name], np.uint32)
    for j, (name, dt) in enumerate(zip(VERTEX, (np.uint32, np.uint32, np.uint8))):
        o[name] = np.asarray([v[j] for v in vertices], dt)
    for j, (name, dt) in enumerate(zip(EDGE, (np.uint32, np.uint32, np.uint8, np.uint32, np.uint32))):
        o[name] = np.asarray([e[j] for e in edges], dt)
    o["ref_path"] = np.asarray(path, np.uint32)
    return o


REQUIRED_BRANCHES = ("no start", "sequence of k bases", "start: new vertex", "start: vertex of the map", "walk from a start above 0",
                     "walk: no offset", "walk: step", "walk: all k - 1 steps", "walk: suffix differs", "walk: more than one in-edge",
                     "extend: edge followed", "extend: new vertex, non-unique", "extend: new vertex, the reference source again",
                     "extend: new vertex, unique", "extend: merged into the map's vertex", "heap: popped")


def census(all_calls):
    """which branches of the restatement the case sets reach: a name -> count dict (tests/test_assembly_graph_oracle.py fails on a
    0), with what only the outputs show: weights above 1, a pruning multiplicity above 1, vertices with two in-edges and two
    out-edges, a group order that differs between two k of one region"""
    n = {name: 0 for name in REQUIRED_BRANCHES}
    n.update(weight_above_1=0, pruning_above_1=0, branching_vertex=0, merging_vertex=0, group_order_differs=0, untracked_vertex=0)
    for c in all_calls:
        for g in c["regions"]:
            orders = set()
            for k in c["k"]:
                x = one(g, k, c["min_q"], c["nps"])
                for name in x["census"]:
                    n[name] += 1
                n["weight_above_1"] += any(e[3] > 1 for e in x["edges"])
                n["pruning_above_1"] += any(e[4] > 1 for e in x["edges"])
                outs, ins = [e[0] for e in x["edges"]], [e[1] for e in x["edges"]]
                n["branching_vertex"] += any(outs.count(v) > 1 for v in set(outs))
                n["merging_vertex"] += any(ins.count(v) > 1 for v in set(ins))
                n["untracked_vertex"] += any(not v[2] & R.TRACKED for v in x["vertices"])
                if len(x["group_order"]) > 1:
                    orders.add(tuple(x["group_order"]))
            n["group_order_differs"] += len(orders) > 1
    return n
