"""A statement-by-statement Python restatement of what the reference's read-threading assembler does with k-mers in front of
the graph, next to its line numbers: R = src/read_threading/read_threading_graph.rs, A = src/read_threading/
read_threading_assembler.rs, K = src/assembly/kmer.rs.  It threads for real -- vertices, edges, a kmer_to_vertex_map keyed by
bytes -- so that the expected n_tracked is len(kmer_to_vertex_map) OUT OF THAT THREADING and the expected THREADED /
THREAD_START are the positions it visits, not a formula.  What phmm_assembly_kmers computes on the device is compared with this
(tests/test_assembly_kmers_hip.py); the two share no code and no shortcut: the device takes a read's last run for all of its
runs, this file scans every run as the reference does.

Left out, and why it cannot matter here: increase_counts_in_matched_kmers (R:641-687) and the multiplicities only change edge
weights, they create no vertex and write no map; flush_single_sample_multiplicity (R:454-456) likewise.  Kmer equality is
restated as equality of the bytes: the reference compares a 64-bit SipHash and the length (K:73-89, K:154-158), so two different
k-mers that collide there would be equal in the reference and are not here."""
from collections import OrderedDict

REF_SHORT, REF_NON_UNIQUE, LOW_COMPLEXITY = 1, 2, 4
NON_UNIQUE, THREADED, THREAD_START, FIRST = 1, 2, 4, 8
NO_ID = 0xFFFFFFFF
REF_SAMPLE = 2 ** 64 - 1     # A:988 std::usize::MAX


class SequenceForKmers:
    def __init__(self, name, sequence, start, stop, count, is_ref, owner):
        self.name, self.sequence, self.start, self.stop, self.count, self.is_ref = name, sequence, start, stop, count, is_ref
        self.owner = owner          # (this file) None for the reference, else the read's index: where the bookkeeping below goes


def kmer(sequence, start, length):   # Kmer::new_with_start_and_length: the bytes are what is compared
    return bytes(sequence[start:start + length])


def determine_non_unique_kmers(seq_for_kmers, kmer_size, scanned=None):   # R:111-141
    all_kmers = set()                                                     # R:116
    non_unique_kmers = []                                                 # R:117
    if seq_for_kmers.stop >= kmer_size:                                   # R:119-124 checked_sub
        stop_position = seq_for_kmers.stop - kmer_size
        for i in range(0, stop_position + 1):                             # R:125: from 0, not from start
            k = kmer(seq_for_kmers.sequence, i, kmer_size)                # R:129-130
            if scanned is not None:
                scanned.add((seq_for_kmers.owner, i))
            if k in all_kmers:                                            # R:131-135
                non_unique_kmers.append(k)
            else:
                all_kmers.add(k)
    return non_unique_kmers                                               # R:140


class ReadThreadingGraph:
    def __init__(self, kmer_size, min_base_quality_to_use_in_assembly=10):
        self.kmer_size = kmer_size
        self.min_base_quality_to_use_in_assembly = min_base_quality_to_use_in_assembly
        self.start_threading_only_at_existing_vertex = False
        self.non_unique_kmers = set()
        self.kmer_to_vertex_map = {}
        self.ref_source = None
        self.reference_path = []
        self.already_built = False
        # base_graph: a vertex is its index into `vertices` (its bytes), an edge [source, target, is_ref, multiplicity]
        self.vertices, self.edges, self.outgoing = [], [], []
        # (this file) what the outputs report
        self.scanned = set()        # (owner, position) every determine_non_unique_kmers loop reached
        self.visited = set()        # (owner, position) thread_sequence created or found a vertex for
        self.starts = set()         # (owner, position) find_start returned

    def set_threading_start_only_at_existing_vertex(self, value):          # R:405-407
        self.start_threading_only_at_existing_vertex = value

    def determine_non_uniques(self, kmer_size, with_non_uniques):          # R:164-187
        result = set()
        for sequence_for_kmers in with_non_uniques:
            non_uniques_from_seq = determine_non_unique_kmers(sequence_for_kmers, kmer_size, self.scanned)
            if non_uniques_from_seq:
                result.update(non_uniques_from_seq)
        return result

    def is_threading_start(self, k):                                       # R:239-248
        if self.start_threading_only_at_existing_vertex:
            return k in self.kmer_to_vertex_map
        return k not in self.non_unique_kmers

    def is_low_quality_graph(self):                                        # R:261-263
        return len(self.non_unique_kmers) * 4 > len(self.kmer_to_vertex_map)

    def get_next_kmer_vertex_for_chain_extension(self, k, is_ref, prev_vertex):   # R:266-279
        unique_merge_vertex = self.get_kmer_vertex(k, False)
        assert not (is_ref and unique_merge_vertex is not None), "Did not find a unique vertex to merge into the reference path"
        return unique_merge_vertex

    def preprocess_reads(self, pending):                                   # R:284-298
        self.non_unique_kmers = self.determine_non_uniques(self.kmer_size, [s for one in pending.values() for s in one])

    def add_sequence(self, pending, seq_name, sample_index, sequence, start, stop, count, is_ref, owner=None):   # R:315-333
        pending.setdefault(sample_index, []).append(SequenceForKmers(seq_name, sequence, start, stop, count, is_ref, owner))

    def add_read(self, sequence, qualities, sample_index, count, pending, owner):   # R:341-390; count is a one-element list
        if len(sequence) == 0 or len(qualities) == 0:                      # R:350-352
            return
        last_good = -1                                                     # R:354
        for end in range(0, len(sequence) + 1):                            # R:355
            if end == len(sequence) or not self.base_is_usable_for_assembly(sequence[end], qualities[end]):   # R:356-357
                start = last_good                                          # R:360
                length = end - start                                       # R:362
                if start != -1 and length >= self.kmer_size:               # R:364
                    self.add_sequence(pending, "%d_%d_%d" % (owner, start, end), sample_index, sequence, start, end, 1, False, owner)
                    count[0] += 1                                          # R:383
                last_good = -1                                             # R:385
            elif last_good == -1:                                          # R:386-388
                last_good = end

    def base_is_usable_for_assembly(self, base, qual):                     # R:400-403
        upper = base - 32 if 97 <= base <= 122 else base                   # to_ascii_uppercase
        return upper != ord("N") and qual >= self.min_base_quality_to_use_in_assembly

    def build_graph_if_necessary(self, pending):                           # R:417-477
        if self.already_built:
            return
        self.preprocess_reads(pending)                                     # R:426
        for sequences_for_samples in pending.values():                     # R:430
            for sequence_for_kmers in sequences_for_samples:
                self.thread_sequence(sequence_for_kmers)                   # R:433
        self.already_built = True

    def thread_sequence(self, seq_for_kmers):                              # R:484-561
        start_pos = self.find_start(seq_for_kmers)                         # R:485
        if start_pos is None:
            return
        self.starts.add((seq_for_kmers.owner, start_pos))
        if len(seq_for_kmers.sequence) <= start_pos + self.kmer_size:      # R:492: the WHOLE sequence's length, not stop
            return
        starting_vertex = self.get_or_create_kmer_vertex(seq_for_kmers.sequence, start_pos)   # R:496-497
        self.visited.add((seq_for_kmers.owner, start_pos))
        # R:499-507 increase_counts_in_matched_kmers: edge weights only, left out
        if seq_for_kmers.is_ref:                                           # R:518-534
            assert self.ref_source is None, "Found two ref_sources!"
            self.reference_path = [starting_vertex]
            self.ref_source = kmer(seq_for_kmers.sequence, seq_for_kmers.start, self.kmer_size)
        vertex = starting_vertex                                           # R:536
        for i in range(start_pos + 1, seq_for_kmers.stop - self.kmer_size + 1):   # R:538
            vertex = self.extend_chain_by_one(vertex, seq_for_kmers.sequence, i, seq_for_kmers.count, seq_for_kmers.is_ref)
            self.visited.add((seq_for_kmers.owner, i))
            if seq_for_kmers.is_ref:                                       # R:546-548
                self.reference_path.append(vertex)

    def find_start(self, seq_for_kmers):                                   # R:569-588
        if seq_for_kmers.is_ref:
            return 0
        stop = max(seq_for_kmers.stop - self.kmer_size, 0)                 # R:573 saturating_sub
        for i in range(seq_for_kmers.start, stop):                         # R:575: exclusive, the last k-mer is never tried
            if self.is_threading_start(kmer(seq_for_kmers.sequence, i, self.kmer_size)):   # R:576-583
                return i
        return None

    def get_or_create_kmer_vertex(self, sequence, start):                  # R:597-605
        k = kmer(sequence, start, self.kmer_size)
        vertex = self.get_kmer_vertex(k, True)
        return self.create_vertex(sequence, k) if vertex is None else vertex

    def get_kmer_vertex(self, k, allow_ref_source):                        # R:613-618
        if not allow_ref_source and self.ref_source == k:
            return None
        return self.kmer_to_vertex_map.get(k)

    def create_vertex(self, sequence, k):                                  # R:626-632
        self.vertices.append(k)
        self.outgoing.append([])
        node_index = len(self.vertices) - 1
        self.track_kmer(k, node_index)
        return node_index

    def track_kmer(self, k, new_vertex):                                   # R:635-639
        if k not in self.non_unique_kmers and k not in self.kmer_to_vertex_map:
            self.kmer_to_vertex_map[k] = new_vertex

    def extend_chain_by_one(self, prev_vertex, sequence, kmer_start, count, is_ref):   # R:700-769
        next_pos = kmer_start + self.kmer_size - 1                         # R:712
        for e in self.outgoing[prev_vertex]:                               # R:715-736
            target = self.edges[e][1]
            if self.vertices[target][-1] == sequence[next_pos]:            # get_suffix
                self.edges[e][3] += count                                  # R:738-747
                return target
        k = kmer(sequence, kmer_start, self.kmer_size)                     # R:750-751
        merge_vertex = self.get_next_kmer_vertex_for_chain_extension(k, is_ref, prev_vertex)   # R:752-753
        next_vertex = self.create_vertex(sequence, k) if merge_vertex is None else merge_vertex   # R:755-759
        self.edges.append([prev_vertex, next_vertex, is_ref, count])       # R:761-765
        self.outgoing[prev_vertex].append(len(self.edges) - 1)
        return next_vertex


def create_graph(reference, reads, kmer_size, min_base_quality=10, recover_dangling_branches=True, samples=None):
    """A:924-1020 up to build_graph_if_necessary.  reads: (bases, quals) pairs of bytes.  Returns (status flags, graph, count):
    the graph is None for a reference shorter than k (A:935-938); REF_NON_UNIQUE is reported and the graph still built, as the
    caller may allow it (A:940-956)."""
    if len(reference) < kmer_size:                                         # A:935-938
        return REF_SHORT, None, 0
    flags = 0
    if determine_non_unique_kmers(SequenceForKmers("ref", reference, 0, len(reference), 1, True, None), kmer_size):   # A:940-956
        flags |= REF_NON_UNIQUE
    rt_graph = ReadThreadingGraph(kmer_size, min_base_quality)             # A:958-967
    rt_graph.set_threading_start_only_at_existing_vertex(not recover_dangling_branches)   # A:980
    pending = OrderedDict()                                                # A:983 LinkedHashMap
    rt_graph.add_sequence(pending, "ref", REF_SAMPLE, reference, 0, len(reference), 1, True)   # A:984-994
    count = [0]                                                            # A:1004
    for r, (bases, quals) in enumerate(reads):                             # A:1008-1016
        rt_graph.add_read(bases, quals, samples[r] if samples else 0, count, pending, r)
    rt_graph.build_graph_if_necessary(pending)                             # A:1020
    if rt_graph.is_low_quality_graph():                                    # (A evaluates it after pruning, which touches neither set)
        flags |= LOW_COMPLEXITY
    return flags, rt_graph, count[0]


def region(reference, reads, kmer_size, min_base_quality=10):
    """One (k, region) as phmm_assembly_kmers reports it: a dict of flags, n_sequences, n_non_unique, n_tracked, n_distinct, and
    per position of the reference (ref_flags, ref_ids) and of every read (read_flags[r], read_ids[r])."""
    flags, g, count = create_graph(reference, reads, kmer_size, min_base_quality)
    out = dict(flags=flags, n_sequences=0, n_non_unique=0, n_tracked=0, n_distinct=0, ref_flags=[0] * len(reference),
               ref_ids=[NO_ID] * len(reference), read_flags=[[0] * len(b) for b, _ in reads], read_ids=[[NO_ID] * len(b) for b, _ in reads])
    if g is None:
        return out
    out.update(n_sequences=count + 1, n_non_unique=len(g.non_unique_kmers), n_tracked=len(g.kmer_to_vertex_map))
    ids = {}
    order = [(None, reference)] + [(r, b) for r, (b, _) in enumerate(reads)]     # the reference first, then the reads in input order
    for owner, sequence in order:
        fl = out["ref_flags"] if owner is None else out["read_flags"][owner]
        idv = out["ref_ids"] if owner is None else out["read_ids"][owner]
        for p in range(len(sequence)):
            if (owner, p) not in g.scanned:
                assert (owner, p) not in g.visited and (owner, p) not in g.starts
                continue
            k = kmer(sequence, p, kmer_size)
            f = 0
            if k not in ids:
                ids[k] = len(ids)
                f |= FIRST
            if k in g.non_unique_kmers:
                f |= NON_UNIQUE
            if (owner, p) in g.visited:
                f |= THREADED
            if (owner, p) in g.starts:
                f |= THREAD_START
            fl[p], idv[p] = f, ids[k]
    out["n_distinct"] = len(ids)
    return out


def chain(g):
    """The bases a raw graph spells if it is ONE chain (every vertex at most one edge in and one out, one source), else None."""
    if not g.vertices:
        return None
    indeg = [0] * len(g.vertices)
    for s, t, _, _ in g.edges:
        indeg[t] += 1
    if any(len(o) > 1 for o in g.outgoing) or any(d > 1 for d in indeg) or indeg.count(0) != 1:
        return None
    v = indeg.index(0)
    spelled, seen = bytearray(g.vertices[v]), 1
    while g.outgoing[v]:
        v = g.edges[g.outgoing[v][0]][1]
        spelled.append(g.vertices[v][-1])
        seen += 1
    return bytes(spelled) if seen == len(g.vertices) else None
