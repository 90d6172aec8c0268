"""The regions tests/test_assembly_kmers_oracle.py (CPU) and tests/test_assembly_kmers_hip.py (GPU) share, and the restatement's
answer (tests/assembly_kmers_restatement.py) in the layout of phmm_assembly_kmers' outputs.  A region is dict(ref=bytes,
reads=[(bases, quals), ...]); a call is dict(regions, k, min_q)."""
import json
import os
import random

import numpy as np

import assembly_kmers_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_kmer_cases.json")
Q = 30
REGION_OUTPUTS = ("flags", "n_sequences", "n_non_unique", "n_tracked", "n_distinct")
PLANES = ("ref_kmer_flags", "read_kmer_flags", "ref_kmer_id", "read_kmer_id")


def read(bases, quals=None, low=(), q=Q):
    """a read of quality q, the positions in `low` at 2"""
    bases = bases.encode() if isinstance(bases, str) else bytes(bases)
    if quals is None:
        quals = bytes(2 if i in low else q for i in range(len(bases)))
    return bases, bytes(quals)


def region(ref, reads=()):
    return dict(ref=ref.encode() if isinstance(ref, str) else bytes(ref), reads=[r if isinstance(r, tuple) else read(r) for r in reads])


def call(regions, k, min_q=10):
    return dict(regions=list(regions), k=sorted(k), min_q=min_q)


# ---- the reference's own cases --------------------------------------------------------------------------------------------------
def golden():
    """name -> (region, k) of tests/golden/assembly_kmer_cases.json"""
    out = {}
    for name, c in json.load(open(GOLDEN)).items():
        if "length" in c:   # test_Ns_in_reads_are_not_used_for_graph: read i is the reference with an N at i
            ref = c["base"].encode() * c["length"]
            reads = [read(ref[:i] + b"N" + ref[i + 1:], q=c["quality"]) for i in range(c["length"])]
        else:
            ref, reads = c["reference"].encode(), [read(r, q=c.get("quality", Q)) for r in c["reads"]]
        out[name] = (dict(ref=ref, reads=reads), c["k"])
    return out


# ---- one region per quirk, small enough to derive by hand (tests/test_assembly_kmers_oracle.py does) ---------------------------
UNRELATED_REF = "GATTCCAGT"   # seven different 3-mers, none of them in the reads below


def scan_from_zero():
    """ACGACGTTGCA with a low-quality C at 1: the one run is [2, 11), its scan starts at 0 and meets ACG at 0 and at 3"""
    return region(UNRELATED_REF, [read("ACGACGTTGCA", low=(1,))])


def only_the_last_kmer_is_unique():
    """AAAAC: AAA twice, AAC once -- and AAC is the run's last k-mer, which find_start never tries"""
    return region(UNRELATED_REF, ["AAAAC"])


def reference_of_exactly_k():
    return region("ACG")


def duplicate_of_the_reference_source():
    """TACGT threads TAC, then ACG -- the reference source, which extend_chain_by_one may not merge into -- then CGT"""
    return region("ACGTTGCA", ["TACGT"])


def quality_at_the_threshold():
    """qualities 10 10 9 10 10: two runs of two at min 10, one run of five at min 9"""
    return region(UNRELATED_REF, [read("ACGTA", quals=[10, 10, 9, 10, 10])])


def lower_and_upper_n():
    return region(UNRELATED_REF, ["ACnGT", "ACNGT", "ACcGT"])


def on_the_threshold():
    """k = 3: AAA is the one non-unique k-mer; AAC and CGT, GTA, TAG are tracked: 1 * 4 == 4, not low"""
    return region("AAAAC", ["CGTAG"])


def one_over_the_threshold():
    """... and with TAG gone 1 * 4 > 3"""
    return region("AAAAC", ["CGTA"])


def hand():
    return dict(scan_from_zero=(scan_from_zero(), 3), only_the_last_kmer_is_unique=(only_the_last_kmer_is_unique(), 3),
                reference_of_exactly_k=(reference_of_exactly_k(), 3), duplicate_of_the_reference_source=(duplicate_of_the_reference_source(), 3),
                quality_at_the_threshold=(quality_at_the_threshold(), 2), lower_and_upper_n=(lower_and_upper_n(), 2),
                on_the_threshold=(on_the_threshold(), 3), one_over_the_threshold=(one_over_the_threshold(), 3))


# ---- generated regions ----------------------------------------------------------------------------------------------------------
def bases(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def pass_boundaries():
    """Reads and references of 63 .. 129 bases: a duplicate whose copies lie in different 64-lane passes, a bad base at 63 and
    at 64, a read with no bad base at all."""
    rng = random.Random(7)
    out = []
    for n in (63, 64, 65, 127, 128, 129):
        ref = bytearray(bases(rng, n))
        if n > 100:
            ref[70:82] = ref[5:17]                       # the two copies of a 12-mer in different passes
        reads = [read(bases(rng, n))]
        b = bytearray(bases(rng, n))
        if n > 100:
            b[90:104] = b[20:34]
        reads.append(read(b))
        for bad in (63, 64):
            if bad < n:
                reads.append(read(ref, low=(bad,)))
                nb = bytearray(ref)
                nb[bad] = ord("N")
                reads.append(read(nb))
        out.append(dict(ref=bytes(ref), reads=reads))
    return call(out, [3, 10, 12])


def run_lengths(k=10):
    """runs of k - 1, k and k + 1 bases in one read, in every order of two of them, and alone"""
    rng = random.Random(11)
    reads = []
    for a in (k - 1, k, k + 1):
        reads.append(read(bases(rng, a)))
        for b in (k - 1, k, k + 1):
            reads.append(read(bases(rng, a) + b"N" + bases(rng, b)))
    reads.append(read(bases(rng, k - 1) + b"N" + bases(rng, k) + b"n" + bases(rng, k + 1), low=(3,)))
    return call([dict(ref=bases(rng, 40), reads=reads)], [k])


def every_k(ks=(1, 3, 10, 25, 64, 103, 255)):
    rng = random.Random(13)
    ref = bases(rng, 300)
    reads = [read(b"", b"")]
    for i in range(12):
        at, n = rng.randrange(0, 40), rng.randrange(200, 261)
        b = bytearray(ref[at:at + n])
        for _ in range(3):
            b[rng.randrange(n)] = rng.choice(b"ACGTN")
        reads.append(read(b, low=tuple(rng.randrange(n) for _ in range(i % 3))))
    reads.append(read(ref[:290]))
    reads.append(read(ref[10:40]))
    return call([dict(ref=ref, reads=reads)], ks)


def largest_reference(n=16384):
    """the largest reference the limits allow and a read of 3 000 bases: their own tables do not fit LDS"""
    rng = random.Random(17)
    ref = bases(rng, n)
    long_read = bytearray(ref[5000:8000])
    long_read[1500] = ord("N")
    long_read[2000:2040] = long_read[100:140]
    reads = [read(long_read, low=(700,)), read(ref[100:250]), read(ref[16000:16384])]
    return call([dict(ref=ref, reads=reads), region(UNRELATED_REF, ["AAAAC"])], [10, 25])


def low_complexity():
    return call([region("ACGTTGCATCAGGATC", ["A" * 40, "AC" * 25, "ACG" * 12, read("T" * 30, low=(15,))]),
                 region("A" * 30, ["A" * 30]), on_the_threshold(), one_over_the_threshold()], [3, 10])


def seeded(n_regions=24, seed=23):
    """regions of 1-40 reads over a 120-base reference with planted repeats, bad bases, Ns, empty and short reads"""
    rng = random.Random(seed)
    out = []
    for g in range(n_regions):
        ref = bytearray(bases(rng, 120))
        if g % 3 == 0:
            at = rng.randrange(60, 90)
            ref[at:at + 26] = ref[10:36]                 # a repeat in the reference: 10 and 25 see it
        reads = []
        for _ in range(rng.randrange(1, 41)):
            how = rng.randrange(10)
            if how == 0:
                reads.append(read(b"", b""))
                continue
            at, n = rng.randrange(0, 80), rng.randrange(4, 101)
            b = bytearray(ref[at:at + n])
            n = len(b)
            for _ in range(rng.randrange(3)):
                b[rng.randrange(n)] = rng.choice(b"ACGTNn")
            if how == 1 and n > 60:
                b[40:60] = b[5:25]                       # a repeat inside the read
            low = tuple(rng.randrange(n) for _ in range(rng.randrange(3))) if how < 6 else ()
            reads.append(read(b, low=low))
        out.append(dict(ref=bytes(ref), reads=reads))
    return call(out, [5, 10, 25])


def calls():
    """name -> call: every set the GPU file runs"""
    out = {}
    for name, (reg, k) in list(golden().items()) + list(hand().items()):
        out[name] = call([reg], [k])
    everything = [reg for reg, _ in list(golden().values()) + list(hand().values())]
    out["golden_and_hand_in_one_call"] = call(everything, [2, 3, 25])
    out["pass_boundaries"] = pass_boundaries()
    out["run_lengths"] = run_lengths()
    out["every_k"] = every_k()
    out["eight_k"] = every_k((1, 3, 10, 25, 64, 103, 200, 255))
    out["low_complexity"] = low_complexity()
    out["seeded"] = seeded()
    out["k_longer_than_every_read"] = call([region("ACGTTGCATCAGGATC", ["ACGTAC", "TTG", read("GATCGATCG", low=(7,))])], [10])
    out["min_quality_9"] = call([quality_at_the_threshold()], [2], min_q=9)
    return out


# ---- the restatement's answer in the call's layout ------------------------------------------------------------------------------
_memo = {}


def one(reg, k, min_q):
    key = (reg["ref"], tuple(reg["reads"]), k, min_q)
    if key not in _memo:
        _memo[key] = R.region(reg["ref"], reg["reads"], k, min_q)
    return _memo[key]


def expected(c, windows=None):
    """The output arrays of a call, from the restatement.  windows: per region and read (first, len) -- the restatement gets the
    cut reads, and their planes lie at the windows' places among the uncut bases."""
    regions, ks, min_q = c["regions"], c["k"], c["min_q"]
    n_ref = sum(len(g["ref"]) for g in regions)
    n_read = sum(len(b) for g in regions for b, _ in g["reads"])
    o = {name: np.zeros((len(ks), len(regions)), np.uint32) for name in REGION_OUTPUTS}
    o.update(ref_kmer_flags=np.zeros((len(ks), n_ref), np.uint8), read_kmer_flags=np.zeros((len(ks), n_read), np.uint8),
             ref_kmer_id=np.full((len(ks), n_ref), R.NO_ID, np.uint32), read_kmer_id=np.full((len(ks), n_read), R.NO_ID, np.uint32))
    for i, k in enumerate(ks):
        at_ref = at_read = 0
        for gi, g in enumerate(regions):
            cut = g
            if windows is not None:
                cut = dict(ref=g["ref"], reads=[(b[f:f + n], q[f:f + n]) for (b, q), (f, n) in zip(g["reads"], windows[gi])])
            x = one(cut, k, min_q)
            for name in REGION_OUTPUTS:
                o[name][i, gi] = x[name]
            o["ref_kmer_flags"][i, at_ref:at_ref + len(g["ref"])] = x["ref_flags"]
            o["ref_kmer_id"][i, at_ref:at_ref + len(g["ref"])] = x["ref_ids"]
            at_ref += len(g["ref"])
            for ri, (b, _) in enumerate(g["reads"]):
                f, n = (0, len(b)) if windows is None else windows[gi][ri]
                o["read_kmer_flags"][i, at_read + f:at_read + f + n] = x["read_flags"][ri]
                o["read_kmer_id"][i, at_read + f:at_read + f + n] = x["read_ids"][ri]
                at_read += len(b)
    return o


def census(all_calls):
    """which branches the case sets reach: a name -> count dict (tests/test_assembly_kmers_oracle.py fails on a 0)"""
    n = dict(read_with_two_runs=0, run_without_start=0, empty_read=0, k_longer_than_every_read=0)
    for f in ("ref_short", "ref_non_unique", "low_complexity"):
        n[f + "_set"] = n[f + "_clear"] = 0
    for c in all_calls:
        for k in c["k"]:
            for g in c["regions"]:
                x = one(g, k, c["min_q"])
                for f, bit in (("ref_short", R.REF_SHORT), ("ref_non_unique", R.REF_NON_UNIQUE), ("low_complexity", R.LOW_COMPLEXITY)):
                    n[f + ("_set" if x["flags"] & bit else "_clear")] += 1
                if x["flags"] & R.REF_SHORT:
                    continue
                n["empty_read"] += sum(1 for b, _ in g["reads"] if not b)
                if g["reads"] and all(len(b) < k for b, _ in g["reads"]) and any(len(b) for b, _ in g["reads"]):
                    n["k_longer_than_every_read"] += 1
                gr = R.ReadThreadingGraph(k, c["min_q"])
                for r, (b, q) in enumerate(g["reads"]):
                    pending, count = {}, [0]
                    gr.add_read(b, q, 0, count, pending, r)
                    n["read_with_two_runs"] += count[0] >= 2
                    starts = sum(1 for f in x["read_flags"][r] if f & R.THREAD_START)
                    n["run_without_start"] += starts < count[0]
    return n
