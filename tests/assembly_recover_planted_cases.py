"""Planted strings for the aligner inside phmm_assembly_recover: hand-built graphs whose one dangling end hands fill_matrix /
walk_back any chosen (reference, alternate) pair.  The kernel reads only the last byte of a vertex's k-mer (the whole k-mer,
reversed, for a vertex of in-degree 0 on the head side), and assembly_recover_cases.graph() takes any bytes per vertex, so a
fork (tails) or a join (heads) with two chains spells any two strings that share their first byte.  Every member is one end on
one graph: no end reads what another changed.  tests/test_assembly_recover_planted_table.py proves the builders and the census on
the CPU; tests/test_assembly_recover_planted_hip.py holds the kernel to the restatement (assembly_recover_restatement.py, which
aligns with the CPU oracle's sw_align(..., "LeadingInDel")) on every member.  Expectations come from the restatement alone; the
score-matrix fill at the bottom of this file COUNTS which rules of the aligner the members reach and decides nothing."""
import itertools
import json
import os
import random

import assembly_recover_cases as C
import assembly_recover_restatement as R
from oracle import oracle

SW_GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smith_waterman_cases.json")))
NAMED = {name: tuple(w) for name, w in SW_GOLDEN["params"].items()}         # the reference's four (smith_waterman_aligner.rs:11-26)
assert NAMED["STANDARD_NGS"] == R.STANDARD_NGS and len(NAMED) == 4
TIES, ZERO, FREE_EXTEND = (1, -1, -1, -1), (0, 0, 0, 0), (25, -50, -10, 0)
FLOOR = (20000000, -20000000, -20000000, -20000000)                         # a match and seven penalties pass SW_CUTOFF = -1e8
# One set more than the issue lists.  The walk starts at the best cell of the last column, and a cell that a vertical gap
# reaches scores its gap's cost below the cell the gap started from, in the same column: with a negative gap_open it is never
# the best, and with ZERO the diagonal (>= both gaps) is taken first.  So a TRAILING DELETION -- the one remove_trailing_deletions
# drops -- needs gaps that cost nothing and a mismatch that costs something: the rows of the last column then tie, the last wins
# (`>=`) and its backtrack entry is a vertical gap.  None of the eight sets above can reach that line of walk_back
FREE_GAPS = (1, -1, 0, 0)
WEIGHTS = dict(NAMED, TIES=TIES, ZERO=ZERO, FREE_EXTEND=FREE_EXTEND, FREE_GAPS=FREE_GAPS, FLOOR=FLOOR)
FILL = b"T"                                                                 # the k - 1 bytes of a vertex that nothing reads
SW_CUTOFF = -100000000
KIND_NAMES = {R.TAIL: "tail", R.HEAD: "head"}


# ---- builders ------------------------------------------------------------------------------------------------------------------------
def _vertex(last, k):
    return FILL * (k - 1) + bytes([last])


def tail_graph(ref, alt, k=1, lead=2, factor=0):
    """`lead` reference vertices, a fork vertex whose last byte is ref[0] == alt[0], a reference chain spelling ref[1:] down to the
    sink, a non-reference chain spelling alt[1:] off the fork.  Vertices: the lead, the fork, the reference chain, the alt chain"""
    ref, alt = bytes(ref), bytes(alt)
    assert ref[0] == alt[0] and len(ref) >= 2 and len(alt) >= 2 and lead >= 1
    kmers = [_vertex(FILL[0], k)] * lead + [_vertex(ref[0], k)] + [_vertex(c, k) for c in ref[1:]] + [_vertex(c, k) for c in alt[1:]]
    fork, r0, a0 = lead, lead + 1, lead + len(ref)
    edges = [(v, v + 1, 1, 1, 1) for v in range(fork)] + [(fork, r0, 1, 1, 1)] + [(v, v + 1, 1, 1, 1) for v in range(r0, a0 - 1)]
    edges += [(fork, a0, 0, 1, 1)] + [(v, v + 1, 0, 1, 1) for v in range(a0, a0 + len(alt) - 2)]
    return C.graph(k, kmers, edges, factor)


def head_graph(ref, alt, k=1, trail=2, factor=0):
    """the mirror: the strings run AGAINST the edges, from the join vertex back.  Each ends in its far vertex's whole k-mer
    reversed: the far vertex of `ref` is the reference source, the far vertex of `alt` the dangling head (both of in-degree 0).
    Vertices: the join, the trail behind it, the reference chain from the join back to the source, the alt chain likewise"""
    ref, alt = bytes(ref), bytes(alt)
    assert ref[0] == alt[0] and len(ref) >= k + 1 and len(alt) >= k + 1 and trail >= 1

    def chain(s):                                                         # the vertices behind the join, nearest first
        n = len(s) - k                                                    # s[1 .. n - 1] a byte each, s[n:] the far vertex's k-mer reversed
        return [_vertex(c, k) for c in s[1:n]] + [s[n:][::-1]]
    rc, ac = chain(ref), chain(alt)
    kmers = [_vertex(ref[0], k)] + [_vertex(FILL[0], k)] * trail + rc + ac
    r0, a0 = 1 + trail, 1 + trail + len(rc)
    edges = [(0, 1, 1, 1, 1)] + [(v, v + 1, 1, 1, 1) for v in range(1, trail)]
    edges += [(r0, 0, 1, 1, 1)] + [(v + 1, v, 1, 1, 1) for v in range(r0, a0 - 1)]
    edges += [(a0, 0, 0, 1, 1)] + [(v + 1, v, 0, 1, 1) for v in range(a0, a0 + len(ac) - 1)]
    return C.graph(k, kmers, edges, factor)


def floor_is_accepted(graphs, weights=FLOOR):
    """the host's documented rule (Limits): max |weight| x (2 L + 2) < 1e9, L = the most vertices of a graph of the
    call + max k + 2"""
    slab_len = max(len(g["kmers"]) for g in graphs) + max(g["k"] for g in graphs) + 2
    return max(abs(w) for w in weights) * (2 * slab_len + 2) < 10 ** 9


def member(family, kind, ref, alt, k=1, factor=0, note=""):
    ref, alt = bytes(ref), bytes(alt)
    g = tail_graph(ref, alt, k, factor=factor) if kind == R.TAIL else head_graph(ref, alt, k, factor=factor)
    return dict(family=family, kind=kind, ref=ref, alt=alt, k=k, factor=factor, graph=g, note=note)


def config(weights, min_dangling_branch_length=1, min_matching_bases=-1, max_mismatches_in_dangling_head=-1):
    return R.Config(min_dangling_branch_length=min_dangling_branch_length, min_matching_bases=min_matching_bases,
                    max_mismatches_in_dangling_head=max_mismatches_in_dangling_head, sw=WEIGHTS[weights])


def group(family, members, weights, k, **options):
    """one call of the GPU file: these members' graphs (one k) under one weight set and one option tuple"""
    assert all(m["k"] == k for m in members)
    if weights == "FLOOR":
        assert floor_is_accepted([m["graph"] for m in members]), (family, k)
    cfg = config(weights, **options)
    return dict(family=family, weights=weights, k=k, cfg=cfg, members=members, graphs=[m["graph"] for m in members],
                name="%s-%s-k%d-len%d-match%d-mism%d" % (family, weights, k, cfg.min_dangling_branch_length, cfg.min_matching_bases,
                                                         cfg.max_mismatches_in_dangling_head))


def _words(lengths, letters=b"AC"):
    return [bytes(w) for n in lengths for w in itertools.product(letters, repeat=n)]


# ---- A: exhaustive tails -------------------------------------------------------------------------------------------------------------
# (ref, alt, the CIGAR, the CIGAR the same rules give WITHOUT the floor at -1e8) under FLOOR, found by search: a cell below the
# floor is lifted to it, and a path through that cell then beats one that the true sums put ahead.  Reaching the floor changes
# no alignment by itself (every cell of a short pair may sit on it and the CIGAR stay); on these pairs it decides
FLOOR_DECIDES = [(b"GCA", b"GAAAACAACAACAAC", "1M13I1M", "1M4I2M8I"), (b"GCC", b"GCAAAAAACAAA", "1M9I2M", "2M6I1M3I"),
                 (b"GACC", b"GCCCCCACACAC", "1M7I2M1I1M", "1M5I2M3I1M"), (b"GAACA", b"GCAACAAACAACAC", "1M8I4M1I", "1M1I4M8I"),
                 (b"GCAA", b"GAAACAAAAACCAAA", "1M10I1M1I2M", "1M3I1M8I2M"), (b"GCCAC", b"GAAAAAAACA", "1M6I3M", "1M4I4M1I"),
                 (b"GC", b"GCCCCACCACACA", "1M10I1M1I", "2M11I"), (b"GCA", b"GCAACAAAAAC", "1M9I1M", "3M8I"),
                 (b"GA", b"GAACCAAACAAC", "1M9I1M1I", "2M10I"), (b"GC", b"GACCCCCCCCCAAAACA", "1M14I1M1I", "1M1I1M14I"),
                 (b"GAACC", b"GACAAAAACCCAAC", "1M10I3M", "1M5I3M4I1M"), (b"GAA", b"GAACAAACACAC", "1M9I2M", "3M9I")]


def family_a():
    """the 900 pairs, and 26 longer ones: behind the shared byte, which always matches, a cell needs seven penalties of FLOOR to
    pass SW_CUTOFF, which no string of five bytes holds; 12 of them are FLOOR_DECIDES"""
    ends = [b"G" + w for w in _words(range(1, 5))]
    assert len(ends) == 30
    members = [member("A", R.TAIL, r, a) for r in ends for a in ends]
    longer = [b"GAAAAAAAA", b"GCCCCCCCC", b"GACACACAC", b"GAAAACCCC"]
    pairs = [(s, x) for s in (b"GA", b"GC") for x in longer[:3]] + [(x, s) for s in (b"GA", b"GC") for x in longer[:2]]
    pairs += [(longer[0], longer[1]), (longer[1], longer[0]), (longer[2], longer[3]), (longer[3], longer[0])]
    members += [member("A", R.TAIL, r, a, note="long enough for the floor") for r, a in pairs]
    members += [member("A", R.TAIL, r, a, note="the floor decides: %s, without it %s" % (with_floor, without)) for r, a, with_floor, without in FLOOR_DECIDES]
    out = [group("A", members, w, 1) for w in WEIGHTS]
    for w in ("STANDARD_NGS", "TIES"):
        for mmb in (0, 1, 2):
            for mdbl in (0, 1, 3):
                if (mdbl, mmb) != (1, -1):
                    out.append(group("A", members, w, 1, min_dangling_branch_length=mdbl, min_matching_bases=mmb))
    return out


# ---- B: exhaustive heads -------------------------------------------------------------------------------------------------------------
def family_b():
    """the strings at k = 1 and k = 3 with prune factor 0; at k = 1 the same strings again with prune factor 2, above every edge's
    pruning multiplicity, so find_path drops the whole alt path (R:1667-1677) and the head arrives with its join vertex alone: the
    only way a head can be shorter than min_dangling_branch_length = 1 asks, which 0 and -1 let through (the tail side's
    max(1, .) never does)"""
    out = []
    for k in (1, 3):
        ends = [b"G" + w for w in _words(range(k, k + 3))]
        assert len(ends) == (14, None, 56)[k - 1]
        members = [member("B", R.HEAD, r, a, k) for r in ends for a in ends]
        if k == 1:
            members += [member("B", R.HEAD, r, a, k, factor=2, note="every edge below the prune factor") for r in ends for a in ends]
        for mmb in (-1, 0, 2):
            for mm in (-1, 1, 2, 5):
                for mdbl in (-1, 0, 1, 3):
                    out.append(group("B", members, "STANDARD_NGS", k, min_dangling_branch_length=mdbl, min_matching_bases=mmb,
                                     max_mismatches_in_dangling_head=mm))
        out += [group("B", members, w, k) for w in WEIGHTS if w != "STANDARD_NGS"]
    return out


# ---- C: the reference's own strings --------------------------------------------------------------------------------------------------
def golden_pairs():
    """(source, reference, read, the asserted case or None): every pair of smith_waterman_cases.json; the flank pairs are the two
    (ref, hap) pairs its generator script (tests/golden/make_sw_cases.py) stores, gaps taken out"""
    out = [(c["source"], c["reference"], c["read"], c) for c in SW_GOLDEN["asserted"]]
    out += [(p["source"], p["reference"], p["read"], None) for p in SW_GOLDEN["avx_equals_scalar_pairs"]]
    f = SW_GOLDEN["flank_pairs"]
    out += [("flank_pairs padded", f["padded_ref"], f["padded_hap"], None), ("flank_pairs not padded", f["not_padded_ref"], f["not_padded_hap"], None)]
    return out


def family_c(shared=b"G"):
    members = [member("C", kind, shared + ref.encode(), shared + read.encode(), note=source)
               for source, ref, read, _ in golden_pairs() for kind in (R.TAIL, R.HEAD)]
    return [group("C", members, w, 1) for w in NAMED]


# ---- D: past one 64-cell pass, long gaps ---------------------------------------------------------------------------------------------
def _dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def d_pairs():
    """(note, ref, alt); ref[0] == alt[0] in every pair"""
    out = []
    for n in (63, 64, 65, 128, 129, 200):
        rng = random.Random(7100 + n)
        ref = _dna(rng, n)
        for d in (1, 63, 64, 65, 130):
            if d < n - 20:
                a = (n - d) // 2
                out.append(("n %d: a deletion of %d" % (n, d), ref, ref[:a] + ref[a + d:]))
            out.append(("n %d: an insertion of %d" % (n, d), ref, ref[:n // 2] + _dna(rng, d) + ref[n // 2:]))
        a = n // 2 - 20
        out.append(("n %d: an insertion and a deletion 30 apart" % n, ref, ref[:a] + _dna(rng, 7) + ref[a:a + 30] + ref[a + 36:]))
        q = n // 4
        out.append(("n %d: three indels" % n, ref, ref[:q] + _dna(rng, 4) + ref[q:2 * q] + ref[2 * q + 5:3 * q] + _dna(rng, 3) + ref[3 * q:]))
        out.append(("n %d: unrelated" % n, ref, ref[:1] + _dna(rng, n - 1)))
        out.append(("n %d: one base beyond the shared one" % n, ref, ref[:1] + _dna(rng, 1)))
        body = _dna(rng, (n - 1) // 2)
        out.append(("n %d: the reference is the alt's body twice" % n, ref[:1] + body + body, ref[:1] + body))
        front = _dna(rng, 100)
        out.append(("n %d: the alt 100 longer at its front" % n, ref, ref[:1] + front + ref[1:]))
        out.append(("n %d: the reference 100 longer at its front" % n, ref[:1] + front + ref[1:], ref))
    return out


# heads at k = 11 whose extension is refused by the index range (R:1240-1244), which no exhaustive string of family B reaches:
# the first element holds one mismatch at an index at or past the alt path's length (the far 11-mer is whole), and the CIGAR's
# reference length minus its read length carries the reference index below 0 (5M7I: 2 + 1 - 7) or past the reference path
# (9M6D5M: 4 + 1 + 6 against 10 vertices)
CANNOT_EXTEND_PAIRS = [("cannot extend: the index falls below 0", b"GAAAA" + b"T" * 11, b"GACAA" + b"C" * 7),
                       ("cannot extend: the index passes the reference path", b"GAAAAAAAA" + b"TTTTTT" + b"CCCCC", b"GAAACAAAA" + b"CCCCC")]


def family_d():
    """as tails and as heads at k = 1; at n = 129 as heads at k = 11 too (the two far k-mers whole; the pair whose alt has two
    bytes cannot end in an 11-mer and stays at k = 1)"""
    pairs = d_pairs()
    one = [member("D", kind, r, a, 1, note=note) for note, r, a in pairs for kind in (R.TAIL, R.HEAD)]
    eleven = [member("D", R.HEAD, r, a, 11, note=note) for note, r, a in pairs if note.startswith("n 129:") and len(a) >= 12]
    eleven += [member("D", R.HEAD, r, a, 11, note=note) for note, r, a in CANNOT_EXTEND_PAIRS]
    return [group("D", m, w, k) for w in ("STANDARD_NGS", "FREE_EXTEND", "FREE_GAPS") for m, k in ((one, 1), (eleven, 11))]


_families = {}


def family(name):
    """the groups of a family, built once per session"""
    if name not in _families:
        _families[name] = dict(A=family_a, B=family_b, C=family_c, D=family_d)[name]()
    return _families[name]


FAMILIES = ("A", "B", "C", "D")


def groups():
    return [g for f in FAMILIES for g in family(f)]


def answer(m, cfg):
    return C.one(m["graph"], cfg)


def cigar_string(els):
    return "".join("%d%s" % (int(e) >> 4, "MID"[int(e) & 15]) for e in els) or "-"


def describe(m, cfg, got_cigar=None, got_n=None):
    """what a failure message says of a member: the strings, the weights, the options, the oracle's CIGAR (and the device's)"""
    x = answer(m, cfg)
    text = "%s %s k=%d factor=%d [%s] ref=%s alt=%s weights=%s min_dangling_branch_length=%d min_matching_bases=%d max_mismatches_in_dangling_head=%d" % (
        m["family"], KIND_NAMES[m["kind"]], m["k"], m["factor"], m["note"], m["ref"].decode(), m["alt"].decode(), cfg.sw,
        cfg.min_dangling_branch_length, cfg.min_matching_bases, cfg.max_mismatches_in_dangling_head)
    text += " oracle: status %s, %d elements %s" % (R.STATUS_NAMES[x["end_status"][0]], x["end_n_cigar"][0], cigar_string(x["end_cigar"][0][:x["end_n_cigar"][0]]))
    if got_cigar is not None:
        text += " device: %d elements %s" % (got_n, cigar_string(got_cigar[:min(int(got_n), 4)]))
    return text


# ---- the census ----------------------------------------------------------------------------------------------------------------------
def fill_counts(ref, alt, weights):
    """FOR COUNTING ONLY: a plain row-by-row fill of smith_waterman_aligner.rs:124-271 (LeadingInDel) that tallies which rules the
    pair reaches.  No expectation comes from it"""
    wm, wx, wo, we = weights
    n, m = len(ref), len(alt)
    low = -(2 ** 31) // 2
    prev = [0] + [wo + (j - 1) * we for j in range(1, m + 1)]
    bgv, gsv = [low] * (m + 1), [0] * (m + 1)
    t = dict(diagonal_ties_a_gap=0, gaps_tie=0, open_ties_extend=0, backtrack_over_64=0, floor=0, last_column_ties=0)
    last = []
    for i in range(1, n + 1):
        cur = [wo + (i - 1) * we] + [0] * m
        bgh, gsh = low, 0
        for j in range(1, m + 1):
            diag = prev[j - 1] + (wm if ref[i - 1] == alt[j - 1] else wx)
            open_v, ext_v = prev[j] + wo, bgv[j] + we
            t["open_ties_extend"] += open_v == ext_v
            bgv[j], gsv[j] = (open_v, 1) if open_v > ext_v else (ext_v, gsv[j] + 1)
            open_h, ext_h = cur[j - 1] + wo, bgh + we
            t["open_ties_extend"] += open_h == ext_h
            bgh, gsh = (open_h, 1) if open_h > ext_h else (ext_h, gsh + 1)
            if diag >= bgv[j] and diag >= bgh:
                val, bt = diag, 0
                t["diagonal_ties_a_gap"] += diag == bgv[j] or diag == bgh
            else:
                val, bt = (bgh, gsh) if bgh >= bgv[j] else (bgv[j], gsv[j])
                t["gaps_tie"] += bgh == bgv[j]
            t["backtrack_over_64"] += bt > 64
            t["floor"] += val <= SW_CUTOFF
            cur[j] = max(val, SW_CUTOFF)
        last.append(cur[m])
        prev = cur
    t["last_column_ties"] = int(last.count(max(last)) > 1)
    return t


_fills = {}
HEAD_ONLY = (R.TOO_MANY_MISMATCHES, R.CANNOT_PUSH_REF, R.CANNOT_EXTEND, R.NO_MERGE_POINT)
# the statuses behind the walk, per kind that can return them; NO_PATH, LOOP and AT_REF_END are decided before any string
# exists (tests/test_assembly_recover_hip.py's graphs reach them), and REFERENCE_FAILS past the strings is the tail's alone (R:1031)
STATUSES = {R.TAIL: (R.TOO_SHORT, R.CIGAR_NOT_OKAY, R.TOO_FEW_MATCHING, R.WHOLE_INSERTION, R.MERGED, R.REFERENCE_FAILS),
            R.HEAD: (R.TOO_SHORT, R.CIGAR_NOT_OKAY, R.TOO_FEW_MATCHING, R.MERGED) + HEAD_ONLY}


def census(gs, max_cells=70000):
    """name -> [count, the first case that reaches it].  The matrix rules are counted on the strings the restatement aligned, once
    per (ref, alt, weights), on pairs of at most max_cells cells (the three longest golden pairs are left to the other counts)"""
    out, counted = {}, set()

    def hit(name, n, g, m):
        if n:
            c = out.setdefault(name, [0, "%s: %s" % (g["name"], describe(m, g["cfg"]))])
            c[0] += int(n)
    for g in gs:
        cfg = g["cfg"]
        for m in g["members"]:
            x = answer(m, cfg)
            assert len(x["end_status"]) == 1 and x["end_kind"][0] == m["kind"]
            status, kind = x["end_status"][0], KIND_NAMES[m["kind"]]
            if status in STATUSES[m["kind"]]:
                hit("%s: %s" % (kind, R.STATUS_NAMES[status]), 1, g, m)
            if not x["end_ref_len"][0]:
                continue                                                   # refused before the aligner
            # (the strings the restatement aligned: the planted ones, or the join vertex's byte where the path was dropped)
            ref, alt = m["ref"][:x["end_ref_len"][0]], m["alt"][:x["end_alt_len"][0]]
            key = (ref, alt, cfg.sw)
            if key not in counted and len(ref) * len(alt) <= max_cells:
                counted.add(key)
                if key not in _fills:
                    _fills[key] = fill_counts(ref, alt, cfg.sw)
                for name, n in _fills[key].items():
                    hit(name, n, g, m)
                raw = [int(e) & 15 for e in oracle.sw_align(ref, alt, cfg.sw, "LeadingInDel")[0]]
                hit("leading I", raw[0] == R.OP_I, g, m)
                hit("leading D", raw[0] == R.OP_D, g, m)
                hit("dropped trailing D", raw[-1] == R.OP_D, g, m)
                hit("dropped trailing D behind four or more elements", raw[-1] == R.OP_D and len(raw) >= 5, g, m)
                nc = x["end_n_cigar"][0]
                hit("4 elements", nc == 4, g, m)
                hit("5 elements", nc == 5, g, m)
                hit("more than 5 elements", nc > 5, g, m)
                hit("a gap over 64 in the CIGAR", any((e >> 4) > 64 and (e & 15) != R.OP_M for e in x["end_cigar"][0]), g, m)
            hit("extension by fewer than k vertices", 0 < x["n_new_vertices"] < m["k"], g, m)
            hit("extension by k > 1 vertices", x["n_new_vertices"] == m["k"] > 1, g, m)
            if m["kind"] == R.HEAD and cfg.max_mismatches_in_dangling_head > 0:
                base = R.Config(min_dangling_branch_length=cfg.min_dangling_branch_length, min_matching_bases=cfg.min_matching_bases, sw=cfg.sw)
                hit("max_mismatches_in_dangling_head > 0 decides differently", answer(m, base)["end_status"][0] != status, g, m)
            if m["kind"] == R.HEAD and cfg.min_dangling_branch_length <= 0 and status != R.TOO_SHORT:
                one = R.Config(min_dangling_branch_length=1, min_matching_bases=cfg.min_matching_bases,
                               max_mismatches_in_dangling_head=cfg.max_mismatches_in_dangling_head, sw=cfg.sw)
                hit("a head that min_dangling_branch_length = 1 refuses", answer(m, one)["end_status"][0] == R.TOO_SHORT, g, m)
    return out


CENSUS = ("diagonal_ties_a_gap", "gaps_tie", "open_ties_extend", "backtrack_over_64", "floor", "last_column_ties", "leading I", "leading D",
          "dropped trailing D", "dropped trailing D behind four or more elements", "4 elements", "5 elements", "more than 5 elements",
          "a gap over 64 in the CIGAR", "extension by fewer than k vertices", "extension by k > 1 vertices",
          "max_mismatches_in_dangling_head > 0 decides differently", "a head that min_dangling_branch_length = 1 refuses") + tuple(
    "%s: %s" % (KIND_NAMES[kind], R.STATUS_NAMES[s]) for kind in (R.TAIL, R.HEAD) for s in STATUSES[kind])
