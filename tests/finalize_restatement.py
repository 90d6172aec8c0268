"""What phmm_finalize_reads (include/phmm.h) computes, restated from the reference statement by statement: test infrastructure,
no GPU.  Every function names the reference lines it restates; where the reference panics a ReferencePanic with the status code
of its family is raised, and `finalize_reads` turns it into the read's status.

A read is a `Read`: cigar as a list of (op, length) with op the BAM code, pos, flags, mapq, mpos, isize, and the window
[first, first + length) of the input's bases that clipping has left (ClippingOp only ever removes bases from the two ends).
The bases and qualities themselves stay in the input arrays.

  src/reads/cigar_builder.rs:30-319          CigarBuilder
  src/reads/cigar_utils.rs:149-328           clip_cigar, revert_soft_clips, alignment_start_shift
  src/reads/clipping_op.rs:100-139, :201-235 apply_revert_soft_clipped_bases, apply_hard_clip_bases
  src/reads/read_clipper.rs:63-530           ReadClipper
  src/reads/read_utils.rs:103-148, :190-211, :288-364
  src/reads/bird_tool_reads.rs:76-104, :239-249, :268-315
  src/utils/fragment_collection.rs:32-76, src/utils/fragment_utils.rs:27-149
  src/assembly/assembly_based_caller_utils.rs:97-185, src/assembly/assembly_region.rs:341-352"""
M, I, D, N, S, H, P, EQ, X = range(9)
OPS = "MIDNSHP=X"

FIN_SOFT_CLIPS, FIN_LOW_QUAL_ENDS, FIN_ADAPTOR, FIN_REGION, FIN_PAIRS = 1, 2, 4, 8, 16
FIN_ALL = 31
STATUS_CIGAR, STATUS_CLIP_RANGE, STATUS_ARITHMETIC, STATUS_PAIR = -1, -2, -3, -4
STATUS_NAMES = {STATUS_CIGAR: "cigar", STATUS_CLIP_RANGE: "clip range", STATUS_ARITHMETIC: "arithmetic", STATUS_PAIR: "pair"}

FLAG_PAIRED, FLAG_UNMAPPED, FLAG_MATE_UNMAPPED, FLAG_REVERSE, FLAG_MATE_REVERSE = 0x1, 0x4, 0x8, 0x10, 0x20
CANNOT_COMPUTE_ADAPTOR_BOUNDARY = 0   # read_utils.rs:17
USIZE = 1 << 64


class ReferencePanic(Exception):
    def __init__(self, status, what):
        Exception.__init__(self, "%s: %s" % (STATUS_NAMES[status], what))
        self.status = status


def parse_cigar(text):
    out, n = [], ""
    for c in text:
        if c.isdigit():
            n += c
        else:
            out.append((OPS.index(c), int(n)))
            n = ""
    return out


def cigar_string(cigar):
    return "".join("%d%s" % (n, OPS[op]) for op, n in cigar)


def consumes_read(op):   # cigar_utils.rs:105-115
    return op in (M, EQ, X, I, S)


def consumes_ref(op):    # :117-127
    return op in (M, D, N, EQ, X)


def is_clipping(op):     # :536-541
    return op in (S, H)


def usize(x, what):
    """a value the reference holds in a usize after a checked subtraction or try_into"""
    if x < 0:
        raise ReferencePanic(STATUS_ARITHMETIC, what)
    return x


class CigarBuilder:      # cigar_builder.rs:30-319
    LEFT_HARD, LEFT_SOFT, MIDDLE, RIGHT_SOFT, RIGHT_HARD = range(5)

    def __init__(self, remove_deletions_at_ends=True):
        self.el, self.last, self.section, self.strip, self.error = [], None, self.LEFT_HARD, remove_deletions_at_ends, False

    def _del_ins(self):  # :198-215
        return self.last == I and len(self.el) > 1 and self.el[-2][0] == D

    def add(self, op, n):   # :58-184; False = Err
        if n == 0:
            return True
        if self.strip and op == D and (self.last is None or is_clipping(self.last) or
                                       (self.last == I and (len(self.el) == 1 or is_clipping(self.el[-2][0])))):
            return True
        if op == H:         # :218-268
            if self.section in (self.LEFT_SOFT, self.MIDDLE, self.RIGHT_SOFT):
                self.section = self.RIGHT_HARD
        elif op == S:
            if self.section == self.RIGHT_HARD:
                self.error = True
                return False
            if self.section == self.LEFT_HARD:
                self.section = self.LEFT_SOFT
            elif self.section == self.MIDDLE:
                self.section = self.RIGHT_SOFT
        else:
            if self.section in (self.RIGHT_SOFT, self.RIGHT_HARD):
                self.error = True
                return False
            if self.section in (self.LEFT_HARD, self.LEFT_SOFT):
                self.section = self.MIDDLE
        if self.last == op:
            if self.el[-1][0] == op:   # combine_cigar_operators(..).unwrap_or(unchanged)
                self.el[-1] = (op, self.el[-1][1] + n)
            return True
        if self.last is None:
            self.el.append((op, n))
            self.last = op
        elif is_clipping(op):
            if self.strip and not consumes_read(self.last) and not is_clipping(self.last):
                self.el[-1] = (op, n)
                self.last = op
            elif self.strip and self._del_ins():
                self.el[-2] = self.el[-1]
                self.el[-1] = (op, n)
            else:
                self.el.append((op, n))
                self.last = op
        elif op == D and self.last == I:
            if len(self.el) > 1 and self.el[-2][0] == D:
                self.el[-2] = (D, self.el[-2][1] + n)
            else:
                self.el.insert(len(self.el) - 1, (op, n))
        else:
            self.el.append((op, n))
            self.last = op
        return True

    def make(self):         # make(false) :270-319; None = Err
        if self.error:
            return None
        if self.section == self.LEFT_SOFT and self.el and self.el[0][0] == S:
            return None
        if self.strip:
            if self.last is None:
                return None
            if self.last == D:
                self.el.pop()
            elif self._del_ins():
                del self.el[-2]
        if not self.el:
            return None
        return list(self.el)


def _add(builder, op, n):
    if not builder.add(op, n):
        raise ReferencePanic(STATUS_CIGAR, "CigarBuilder::add is an Err")


def _make(builder):
    out = builder.make()
    if out is None:
        raise ReferencePanic(STATUS_CIGAR, "CigarBuilder::make is an Err")
    return out


def clip_cigar(cigar, start, stop, clip_op):     # cigar_utils.rs:149-256
    clip_left = start == 0
    b = CigarBuilder(True)
    element_start = 0
    for op, n in cigar:
        if op == H:
            _add(b, H, n)
            continue
        element_end = element_start + (n if consumes_read(op) else 0)
        if element_end <= start or element_start >= stop:
            if consumes_read(op) or (element_start != start and element_start != stop):
                _add(b, op, n)
        else:
            unclipped = (element_end - stop) if clip_left else (start - element_start)
            if unclipped <= 0:       # checked_sub is None, or 0: totally clipped
                if consumes_read(op):
                    _add(b, clip_op, n)
            else:
                clipped = usize(n - unclipped, "len.checked_sub(unclipped_length).unwrap()")
                if clip_left:
                    _add(b, clip_op, clipped)
                    _add(b, op, unclipped)
                else:
                    _add(b, op, unclipped)
                    _add(b, clip_op, clipped)
        element_start = element_end
    return _make(b)


def revert_soft_clips(cigar):                    # :262-276
    b = CigarBuilder(True)
    for op, n in cigar:
        _add(b, M if op == S else op, n)
    return _make(b)


def alignment_start_shift(cigar, num_clipped):   # :281-328
    ref_bases_clipped = 0
    element_start = 0
    for op, n in cigar:
        if op == H:
            continue
        element_end = element_start + (n if consumes_read(op) else 0)
        if element_end <= num_clipped:
            ref_bases_clipped += n if consumes_ref(op) else 0
        elif element_start < num_clipped:
            ref_bases_clipped += (num_clipped - element_start) if consumes_ref(op) else 0
            break
        element_start = element_end
    return ref_bases_clipped


def get_read_index_for_reference_coordinate(alignment_start, cigar, ref_coord):   # read_utils.rs:103-148
    if ref_coord < alignment_start:
        return None, None
    last_read, last_ref = 0, alignment_start
    for op, n in cigar:
        first_read, first_ref = last_read, last_ref
        last_read += n if consumes_read(op) else 0
        last_ref += n if (consumes_ref(op) or op == S) else 0
        if first_ref <= ref_coord < last_ref:
            return first_read + ((ref_coord - first_ref) if consumes_read(op) else 0), op
    return None, None


class Read:
    def __init__(self, pos, flags, mapq, mpos, isize, cigar, length):
        self.pos, self.flags, self.mapq, self.mpos, self.isize = pos, flags, mapq, mpos, isize
        self.cigar = parse_cigar(cigar) if isinstance(cigar, str) else [tuple(c) for c in cigar]
        self.first, self.length, self.emptied = 0, length, False

    # rust_htslib flags
    is_paired = property(lambda s: bool(s.flags & FLAG_PAIRED))
    is_unmapped = property(lambda s: bool(s.flags & FLAG_UNMAPPED))
    is_mate_unmapped = property(lambda s: bool(s.flags & FLAG_MATE_UNMAPPED))
    is_reverse = property(lambda s: bool(s.flags & FLAG_REVERSE))
    is_mate_reverse = property(lambda s: bool(s.flags & FLAG_MATE_REVERSE))

    def is_empty(self):
        return self.length == 0

    def get_start(self):       # bird_tool_reads.rs:239-241 (pos as usize)
        return self.pos % USIZE

    def reference_length(self):
        return sum(n for op, n in self.cigar if consumes_ref(op))

    def get_end(self):         # :243-249: checked_sub(1).unwrap_or(0)
        return self.get_start() + max(self.reference_length() - 1, 0)

    def get_soft_start_i64(self):   # :91-104
        start = self.get_start()
        for op, n in self.cigar:
            if op == S:
                start -= n
            elif op == H:
                continue
            else:
                break
        return start

    def get_soft_start(self):  # :76-89, unwrapped
        return usize(self.get_soft_start_i64(), "get_soft_start().unwrap()")

    def seq_len_from_cigar(self):
        return sum(n for op, n in self.cigar if consumes_read(op))


def empty_read(r):             # read_utils.rs:190-211
    r.flags |= FLAG_MATE_UNMAPPED | FLAG_UNMAPPED
    r.mapq = 0
    r.cigar = []
    r.length = 0
    r.emptied = True
    return r


def apply_hard_clip_bases(r, start, stop):       # clipping_op.rs:201-235
    new_length = usize(r.length - usize(stop - start, "stop - start") - 1, "read.len() - (stop - start + 1)")
    if new_length == 0:
        empty_read(r)
        return
    cigar = r.cigar
    new_cigar = [(M, 0)] if r.is_unmapped else clip_cigar(cigar, start, stop + 1, H)
    copy_start = stop + 1 if start == 0 else 0
    r.first += copy_start
    r.length = new_length
    r.cigar = new_cigar
    if start == 0 and not r.is_unmapped:
        r.pos = r.pos + alignment_start_shift(cigar, stop + 1)


def apply_revert_soft_clipped_bases(r):          # :100-139
    if not r.cigar or not (is_clipping(r.cigar[0][0]) or is_clipping(r.cigar[-1][0])):
        return
    unclipped = revert_soft_clips(r.cigar)
    new_start = r.get_soft_start_i64()
    r.cigar = unclipped
    if new_start <= 0:
        r.pos = 0
        apply_hard_clip_bases(r, 0, -new_start)
        if not r.is_unmapped:
            r.pos = 0
    else:
        r.pos = new_start


HARD, REVERT = "hard", "revert"


def clip_read(r, ops, algorithm):                # read_clipper.rs:363-388
    if not ops:
        return r
    for start, stop in ops:
        read_length = r.length
        if start < read_length:
            if stop >= read_length:
                stop = read_length - 1
            if algorithm == HARD:
                apply_hard_clip_bases(r, start, stop)
            else:
                apply_revert_soft_clipped_bases(r)
    if r.is_empty():
        empty_read(r)
    return r


def hard_clip_soft_clipped_bases(r):             # :395-435
    if r.is_empty():
        return r
    read_index, cut_left, cut_right, right_tail = 0, -1, -1, False
    for op, n in r.cigar:
        if op == S:
            if right_tail:
                cut_right = read_index
            else:
                cut_left = read_index + n - 1
        elif op == H:
            pass
        else:
            right_tail = True
        if consumes_read(op):
            read_index += n
    ops = []
    if cut_right >= 0:
        ops.append((cut_right, r.length))
    if cut_left >= 0:
        ops.append((0, cut_left))
    return clip_read(r, ops, HARD)


def revert_soft_clipped_bases(r):                # :441-449
    if r.is_empty():
        return r
    return clip_read(r, [(0, 0)], REVERT)


def low_qual_tail_scan(quals, low_qual):
    """the two loops of clip_low_qual_ends (:501-516) over a window's qualities: (left_clip_index, right_clip_index)"""
    read_length = len(quals)
    left, right = 0, max(read_length - 1, 0)
    while right > 0 and quals[right] <= low_qual:
        right -= 1
    while left < read_length and quals[left] <= low_qual:
        left += 1
    return left, right


def hard_clip_low_qual_ends(r, quals, low_qual):   # :474-532; quals: the input's, of which the read holds its window
    if r.is_empty():
        return r
    read_length = r.length
    left, right = low_qual_tail_scan(quals[r.first:r.first + r.length], low_qual)
    if left > right:
        return empty_read(r)
    ops = []
    if right < read_length - 1:
        ops.append((right + 1, read_length - 1))
    if left > 0:
        ops.append((0, left - 1))
    return clip_read(r, ops, HARD)


def clip_by_reference_coordinates(r, ref_start, ref_stop):   # :114-210, HardclipBases
    if r.is_empty():
        return r
    if ref_start is None:
        start = 0
        pos, op = get_read_index_for_reference_coordinate(r.get_soft_start(), r.cigar, ref_stop)
        if pos is not None:
            stop = pos - (0 if consumes_read(op) else 1)
            stop = None if stop < 0 else stop            # checked_sub
        else:
            stop = None
    else:
        start = get_read_index_for_reference_coordinate(r.get_soft_start(), r.cigar, ref_start)[0]
        stop = r.length - 1
    if start is None or stop is None:
        return r
    if stop > r.length - 1:
        raise ReferencePanic(STATUS_CLIP_RANGE, "Trying to clip after the end of a read")
    if stop < start:
        raise ReferencePanic(STATUS_CLIP_RANGE, "Start > Stop, this should never happen")
    if start > 0 and stop < r.length - 1:
        raise ReferencePanic(STATUS_CLIP_RANGE, "Trying to clip the middle of a read")
    return clip_read(r, [(start, stop)], HARD)


def hard_clip_both_ends_by_reference_coordinates(r, left, right):   # :234-258
    if r.is_empty() or left == right:
        return empty_read(r)
    clip_by_reference_coordinates(r, right, None)
    if left > r.get_end():
        return empty_read(r)
    return clip_by_reference_coordinates(r, None, left)


def hard_clip_to_region(r, ref_start, ref_stop):   # :63-100
    start, stop = r.get_start(), r.get_end()
    if start <= ref_stop and stop >= ref_start:
        if start < ref_start and stop > ref_stop:
            return hard_clip_both_ends_by_reference_coordinates(r, max(ref_start - 1, 0), ref_stop + 1)
        if start < ref_start:
            return clip_by_reference_coordinates(r, None, max(ref_start - 1, 0))
        if stop > ref_stop:
            return clip_by_reference_coordinates(r, ref_stop + 1, None)
        return r
    return empty_read(r)


def has_well_defined_fragment_size(r):           # read_utils.rs:288-316
    if r.isize == 0 or not r.is_paired or r.is_unmapped or r.is_mate_unmapped or r.is_reverse == r.is_mate_reverse:
        return False
    if r.is_reverse:
        return r.get_end() > r.mpos
    return r.get_start() <= r.mpos + r.isize


def get_adaptor_boundary(r):                     # :344-353
    if not has_well_defined_fragment_size(r):
        return CANNOT_COMPUTE_ADAPTOR_BOUNDARY
    if r.is_reverse:
        return usize((r.mpos % USIZE) - 1, "mpos as usize - 1")
    return r.get_start() + abs(r.isize)


def is_inside_read(r, coordinate):               # :362-364
    return r.get_start() <= coordinate <= r.get_end()


def hard_clip_adaptor_sequence(r):               # read_clipper.rs:458-472
    boundary = get_adaptor_boundary(r)
    if boundary == CANNOT_COMPUTE_ADAPTOR_BOUNDARY or not is_inside_read(r, boundary):
        return r
    if r.is_reverse:
        return clip_by_reference_coordinates(r, None, boundary)
    return clip_by_reference_coordinates(r, boundary, None)


def overlaps(r, span_start, span_end):           # simple_interval.rs:298-307 with the read as self
    s, e = r.get_start(), r.get_end()
    return (s <= span_start <= e) or (s <= span_end <= e) or (s >= span_start and e <= span_end)


def finalize_one(r, quals, span_start, span_end, steps, min_tail_quality, dont_use_soft_clipped_bases):
    """assembly_based_caller_utils.rs:120-171 for one read; a step that is not set is the identity.  Returns keep."""
    if steps & FIN_SOFT_CLIPS:
        if dont_use_soft_clipped_bases or not has_well_defined_fragment_size(r):
            hard_clip_soft_clipped_bases(r)
        else:
            revert_soft_clipped_bases(r)
    if steps & FIN_LOW_QUAL_ENDS:
        hard_clip_low_qual_ends(r, quals, min_tail_quality)
    if not r.get_start() <= r.get_end():
        return False
    if steps & FIN_ADAPTOR and not r.is_unmapped:
        hard_clip_adaptor_sequence(r)
    if r.is_empty() or r.seq_len_from_cigar() <= 0:
        return False
    if steps & FIN_REGION:
        hard_clip_to_region(r, span_start, span_end)
    return r.get_start() <= r.get_end() and r.length > 0 and overlaps(r, span_start, span_end)


def sort_key(r, index):
    """the keys of BirdToolRead::cmp (bird_tool_reads.rs:268-315) the device knows, then the input index: one contig, names
    unknown (mates share theirs), mtid equal.  mpos is compared only between paired reads -- pair candidates are."""
    return (r.get_start(), r.is_reverse, r.flags, r.mapq, r.mpos, r.length, index)


def is_pair_candidate(r):                        # fragment_collection.rs:47-51, negated
    return not (not r.is_paired or r.is_mate_unmapped or r.mpos == -1 or r.mpos > r.get_end())


def adjust_quals_of_overlapping_paired_fragments(pair, bases, quals, half_of_pcr_snv_qual):   # fragment_utils.rs:27-149
    """pair: ((read, bases offset), (read, bases offset)) in the order FragmentCollection met them; bases: the input's;
    quals: the output's, changed in place"""
    in_order = pair[0][0].get_soft_start() < pair[1][0].get_soft_start()
    (first, f_at), (second, s_at) = pair if in_order else (pair[1], pair[0])
    if first.get_end() < second.get_start():
        return
    offset, op = get_read_index_for_reference_coordinate(first.get_soft_start(), first.cigar, second.get_start())
    if offset is None or is_clipping(op):
        return

    def unwrap(x):
        if x is None:
            raise ReferencePanic(STATUS_PAIR, "unwrap on None")
        return x
    first_end_base = unwrap(get_read_index_for_reference_coordinate(first.get_soft_start(), first.cigar, first.get_end())[0])
    second_end_base = unwrap(get_read_index_for_reference_coordinate(second.get_soft_start(), second.cigar, second.get_end())[0])
    first_stop = offset
    second_offset = unwrap(get_read_index_for_reference_coordinate(second.get_soft_start(), second.cigar, second.get_start())[0])
    n = min(max(first_end_base - first_stop, 0), max(second_end_base - second_offset, 0)) + 1
    if first_stop + n > first.length or second_offset + n > second.length:
        raise ReferencePanic(STATUS_PAIR, "index out of bounds")   # (the panic undoes what the loop had changed)
    for i in range(n):
        fi, si = f_at + first.first + first_stop + i, s_at + second.first + second_offset + i
        if bases[fi] == bases[si]:
            quals[fi] = min(quals[fi], half_of_pcr_snv_qual)
            quals[si] = min(quals[si], half_of_pcr_snv_qual)
        else:
            quals[fi] = 0
            quals[si] = 0


FIELDS = ("read_status", "keep", "new_pos", "out_unmapped", "clip_first", "clip_len", "out_cigar", "unclipped_len", "lead_soft",
          "trail_soft", "out_quals")


def finalize_reads(groups, steps=FIN_ALL, min_tail_quality=9, dont_use_soft_clipped_bases=False, half_of_pcr_snv_qual=20):
    """groups: a list of dicts {span: (start, end), reads: [dict(pos, flags, mapq, mpos, isize, cigar, bases, quals, mate)]},
    `mate` the index INSIDE the group of the other read of the same name or -1.  Returns per read, in input order, a dict of
    FIELDS (out_cigar a list of (op, length), out_quals a list)."""
    out = []
    for g in groups:
        span_start, span_end = g["span"]
        state = []
        for rd in g["reads"]:
            quals = list(rd["quals"])
            r = Read(rd["pos"], rd["flags"], rd["mapq"], rd["mpos"], rd["isize"], rd["cigar"], len(rd["bases"]))
            res = dict(read_status=0, keep=0, new_pos=0, out_unmapped=0, clip_first=0, clip_len=0, out_cigar=[], unclipped_len=0,
                       lead_soft=0, trail_soft=0, out_quals=quals)
            try:
                keep = finalize_one(r, quals, span_start, span_end, steps, min_tail_quality, dont_use_soft_clipped_bases)
                lead = trail = 0
                for op, n in r.cigar:        # the leading and the trailing soft clip (behind hard clips)
                    if op == S:
                        lead = n
                    if op != H:
                        break
                for op, n in reversed(r.cigar):
                    if op == S:
                        trail = n
                    if op != H:
                        break
                if len([1 for op, _ in r.cigar if op != H]) == 1 and lead:
                    trail = 0                # one soft clip is not both
                res.update(keep=int(keep), new_pos=r.pos, out_unmapped=int(r.emptied),
                           clip_first=r.first if r.length else 0, clip_len=r.length, out_cigar=list(r.cigar),
                           unclipped_len=r.length - sum(n for op, n in r.cigar if op == S), lead_soft=lead, trail_soft=trail)
            except ReferencePanic as e:
                res["read_status"] = e.status
            state.append((r, res))
            out.append(res)
        if not steps & FIN_PAIRS:
            continue
        # FragmentCollection::create over the kept reads in sorted order: a pair is two kept candidates that name each other
        for i, rd in enumerate(g["reads"]):
            j = rd.get("mate", -1)
            if j <= i:
                continue
            (ri, resi), (rj, resj) = state[i], state[j]
            if not (resi["keep"] and resj["keep"] and is_pair_candidate(ri) and is_pair_candidate(rj)):
                continue
            order = [(ri, i), (rj, j)] if sort_key(ri, i) < sort_key(rj, j) else [(rj, j), (ri, i)]
            # one array of bases and one of qualities per pair, as the device sees them
            bases = list(g["reads"][order[0][1]]["bases"]) + list(g["reads"][order[1][1]]["bases"])
            q0, q1 = state[order[0][1]][1]["out_quals"], state[order[1][1]][1]["out_quals"]
            quals = q0 + q1
            try:
                adjust_quals_of_overlapping_paired_fragments(((order[0][0], 0), (order[1][0], len(q0))), bases, quals, half_of_pcr_snv_qual)
                q0[:] = quals[:len(q0)]
                q1[:] = quals[len(q0):]
            except ReferencePanic as e:
                for res in (resi, resj):
                    res["keep"] = 0
                    res["read_status"] = e.status
    return out
