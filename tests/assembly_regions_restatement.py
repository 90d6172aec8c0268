"""A statement-by-statement restatement of what phmm_assembly_regions computes, each statement beside its line of the
reference.  Test infrastructure only: the product never imports it.
P = src/activity_profile/activity_profile.rs, A = src/assembly/assembly_region.rs, T = src/assembly/assembly_region_iterator.rs,
U = src/utils/interval_utils.rs, I = src/utils/simple_interval.rs."""
import numpy as np

F32 = np.float32
F32_MAX = np.finfo(np.float32).max
DENSITY_TOLERANCE = F32(0.05)           # PROBABILITY_TOLERANCE_FOR_DENSITY_CHECK
ACTIVE, FORCED, OVER_DEPTH = 1, 2, 4
STATUS_MIN_REGION_SIZE, STATUS_START_PAST_CONTIG = -1, -2


class Panic(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


class Profile:
    """ActivityProfile as far as popping reads it: the state list (f32 probabilities, state i at start + i), region_stop_loc,
    the threshold, the propagation distance, the contig's length.  `branches` collects what a run reached (the census)."""

    def __init__(self, probs, start, stop, contig_len, threshold, max_prob_propagation, branches=None):
        self.state_list = [F32(x) for x in probs]
        self.loc0 = int(start)                                   # state_list[0].get_loc()
        self.region_stop_loc = int(stop) if len(self.state_list) else None
        self.contig_len = int(contig_len)
        self.threshold = F32(threshold)
        self.max_prob_propagation_distance = int(max_prob_propagation)
        self.branches = branches if branches is not None else set()

    def get_prob(self, i):                                       # P:647-649
        return self.state_list[i]

    def is_minimum(self, index):                                 # P:660-668
        if index == len(self.state_list) - 1 or index < 1:
            self.branches.add("is_minimum:last" if index >= 1 else "is_minimum:first")
            return False
        p = self.get_prob(index)
        return bool(p <= self.get_prob(index + 1) and p < self.get_prob(index - 1))

    def find_first_activity_boundary(self, is_active_region, max_region_size):   # P:621-640
        n_states = len(self.state_list)
        end = 0
        while end < n_states and end < max_region_size:
            if bool(self.get_prob(end) > self.threshold) != is_active_region:
                self.branches.add("boundary:found")
                break
            end += 1
        return end

    def find_best_cut_site(self, end_of_active_region, min_region_size):         # P:582-605
        if not end_of_active_region >= min_region_size:                          # the assertion P:583-586
            raise Panic(STATUS_MIN_REGION_SIZE)
        min_i = end_of_active_region - 1
        min_p = F32_MAX
        i = min_i
        hit = False
        while i >= min_region_size:
            cur = self.get_prob(i)
            if bool(cur < min_p) and self.is_minimum(i):
                if hit and cur == min_p:
                    raise AssertionError("unreachable: cur < min_p")
                min_p, min_i, hit = cur, i, True
            i -= 1
        self.branches.add("cut:minimum" if hit else "cut:none")
        return min_i + 1

    def find_end_of_region(self, is_active_region, min_region_size, max_region_size, force_conversion):   # P:545-569
        if not force_conversion and len(self.state_list) < max_region_size + self.max_prob_propagation_distance:
            self.branches.add("end:wait")
            return None
        end = self.find_first_activity_boundary(is_active_region, max_region_size)
        if is_active_region and end == max_region_size:
            end = self.find_best_cut_site(end, min_region_size)
        return end - 1 if end >= 1 else None                                     # checked_sub(1)

    def pop_next_ready_assembly_region(self, extension, min_region_size, max_region_size, force_conversion):   # P:429-523
        if not self.state_list:
            self.branches.add("pop:empty")
            return None
        is_active_region = bool(self.state_list[0] > self.threshold)             # P:465
        offset = self.find_end_of_region(is_active_region, min_region_size, max_region_size, force_conversion)
        if offset is None:
            return None
        sub = self.state_list[:offset + 1]                                       # drain(0..offset + 1)
        first = self.loc0
        del self.state_list[:offset + 1]
        self.loc0 += offset + 1
        if not self.state_list:                                                  # P:487-489
            self.region_stop_loc = None
            self.branches.add("pop:drained")
        start, end = first, min(first + offset, self.contig_len - 1)             # P:495-502
        if end != first + offset:
            self.branches.add("region:clipped")
        n_dense = sum(1 for s in sub if bool(s > DENSITY_TOLERANCE))             # P:506
        if end < start:                                                          # I:62-64 end - start + 1 underflows
            raise Panic(STATUS_START_PAST_CONTIG)
        density = F32(n_dense) / F32(end - start + 1)                            # P:508
        padded = make_padded_span(start, end, extension, self.contig_len, self.branches)
        return dict(start=start, end=end, padded_start=padded[0], padded_end=padded[1], states=offset + 1,
                    flags=(ACTIVE if is_active_region else 0) | (FORCED if force_conversion else 0), density=density)

    def pop_ready_assembly_regions(self, extension, min_region_size, max_region_size):   # P:371-412
        assert min_region_size > 0 and max_region_size > 0                       # P:378-379
        regions, region_start, status = [], None, 0
        while True:
            if region_start is not None:                                         # P:384-392
                force = region_start != self.region_stop_loc + 1 if self.region_stop_loc is not None else False
                if self.region_stop_loc is not None and not force:
                    self.branches.add("force:start_is_stop_plus_1")
            else:
                force = False
            try:
                region = self.pop_next_ready_assembly_region(extension, min_region_size, max_region_size, force)
            except Panic as e:
                status = e.status
                break
            if region is None:
                break
            if force:
                self.branches.add("force:forced")
            region_start = region["start"]
            regions.append(region)
        return regions, status


def make_padded_span(start, end, padding, contig_length, branches=None):         # A:169-189
    s = 0 if padding > start else start - padding
    assert contig_length >= 1                                                    # U:27-31
    bounded_stop = min(contig_length, end + padding)                             # U:33
    if branches is not None:
        if padding > start:
            branches.add("pad:saturated")
        if bounded_stop != end + padding:
            branches.add("pad:clipped")
    if s > contig_length:                                                        # U:35-36 None -> the active span
        return start, end
    return s, bounded_stop


def reference_length(cigar):
    """bam_cigar2rlen: the elements that consume the reference, M, D, N, = and X."""
    return sum(int(c) >> 4 for c in cigar if (int(c) & 15) in (0, 2, 3, 7, 8))


def mean_quality(quals):                                                         # T:143-147
    total = np.float64(0.0)
    for q in quals:
        total = total + np.float64(q)
    with np.errstate(invalid="ignore", divide="ignore"):
        return total / np.float64(len(quals))


def fetched(pos, reflen, padded_start, padded_end):
    """htslib's overlap rule for fetch(tid, padded_start, padded_end + 1): the half-open read [pos, pos + max(reflen, 1))
    against the half-open [padded_start, padded_end + 1)."""
    return pos <= padded_end and pos + max(reflen, 1) > padded_start


def assembly_regions(a, extension, min_region_size, max_region_size, max_prob_propagation, threshold, max_input_depth,
                     with_reads=True, branches=None):
    """Every output array of phmm_assembly_regions for the input arrays `a` (the header's names), as a dict."""
    branches = branches if branches is not None else set()
    prob = np.asarray(a["profile_prob"], np.float32)
    n_profiles = len(a["profile_len"])
    reads = with_reads and a.get("group_read_off") is not None
    o = dict(profile_status=np.zeros(n_profiles, np.int32), profile_region_off=np.zeros(n_profiles + 1, np.uint32))
    regions, owner = [], []
    for k in range(n_profiles):
        f, n = int(a["profile_first"][k]), int(a["profile_len"][k])
        prof = Profile(prob[f:f + n], a["profile_start"][k], a["profile_stop"][k], a["profile_contig_length"][k], threshold,
                       max_prob_propagation, branches)
        got, status = prof.pop_ready_assembly_regions(extension, min_region_size, max_region_size)
        o["profile_status"][k] = status
        regions += got
        owner += [k] * len(got)
        o["profile_region_off"][k + 1] = len(regions)
    R = len(regions)
    col = lambda key, dt: np.array([r[key] for r in regions], dt)  # noqa: E731
    o.update(region_start=col("start", np.uint64), region_end=col("end", np.uint64), region_padded_start=col("padded_start", np.uint64),
             region_padded_end=col("padded_end", np.uint64), region_states=col("states", np.uint32),
             region_density=col("density", np.float32), region_n_reads=np.zeros(R, np.uint32))
    flags = col("flags", np.uint32)
    if reads:
        S = int(a["n_samples"])
        n_reads = len(a["read_pos"])
        reflen = [reference_length(a["read_cigar"][a["read_cigar_off"][r]:a["read_cigar_off"][r + 1]]) for r in range(n_reads)]
        o["read_mean_qual"] = np.array([mean_quality(a["read_quals"][a["read_off"][r]:a["read_off"][r + 1]]) for r in range(n_reads)], np.float64)
        off, members = [0], []
        for r in range(R):
            for s in range(S):
                g = int(a["profile_window"][owner[r]]) * S + s
                for i in range(int(a["group_read_off"][g]), int(a["group_read_off"][g + 1])):
                    if fetched(int(a["read_pos"][i]), reflen[i], regions[r]["padded_start"], regions[r]["padded_end"]):
                        members.append(i)
                off.append(len(members))
            o["region_n_reads"][r] = off[-1] - off[-1 - S]
            if o["region_n_reads"][r] > max_input_depth:                         # T:141
                flags[r] |= OVER_DEPTH
                branches.add("depth:over")
        o["region_read_off"] = np.array(off, np.uint32)
        o["region_reads"] = np.array(members, np.uint32)
    o["region_flags"] = flags
    o["required"] = np.array([R, len(o["region_reads"]) if reads else 0], np.uint32)
    for st in set(int(x) for x in o["profile_status"]):
        branches.add("status:%d" % st)
    for fl in set(int(x) for x in flags):
        branches.update(name for bit, name in ((ACTIVE, "flag:active"), (FORCED, "flag:forced"), (OVER_DEPTH, "flag:over_depth")) if fl & bit)
        if not fl:
            branches.add("flag:none")
    return o
