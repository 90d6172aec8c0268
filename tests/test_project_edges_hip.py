"""phmm_project_to_reference on the MI355X on alignments the aligner never emits (tests/project_edge_cases.py; the inputs' own
conditions are held in tests/test_project_edge_table.py): every operator pair of apply_cigar_to_cigar, the builder's rules on
the alignment side, indels at the right end of repeats, both sides of the `plain` short cut's condition, random hand-built
alignments over all nine operators, and launches on both sides of the line between builders in LDS and in HBM.  Everything is
EQUALITY with oracle/cigar_oracle.c read by read -- status; position and CIGAR where the status is 0; position 0 and no elements
elsewhere -- and the workspace status (-6) appears for no read: the host's sizing claim."""
import ctypes as C

import numpy as np
import pytest

import project_edge_cases as cases
from lorikeet_amd import _lib, realign
from oracle import oracle
from project_scenarios import oracle_read as scenario_oracle_read, scenario

pytestmark = pytest.mark.gpu

WORKSPACE_STATUS = -6
_EXPECTED = {}


def _expected(key, inputs):
    """The oracle's answers for a builder's inputs, computed once."""
    if key not in _EXPECTED:
        _EXPECTED[key] = cases.oracle_all(inputs)
    return _EXPECTED[key]


def _project(eng, inputs):
    return realign.project_to_reference(eng, *inputs)


def _hold(inputs, got, expected):
    assert len(got.status) == len(expected) == inputs[0].n_reads
    assert WORKSPACE_STATUS not in got.status, [cases.describe(inputs, int(r)) for r in np.flatnonzero(got.status == WORKSPACE_STATUS)[:3]]
    for r, (st, pos, cig) in enumerate(expected):
        have = (int(got.status[r]), int(got.new_pos[r]), oracle.cigar_to_string(got.cigars[r]))
        assert have == (st, pos, cig), "%s: device %r, oracle %r" % (cases.describe(inputs, r), have, (st, pos, cig))


def _same(a, b, n):
    assert np.array_equal(a.status[:n], b.status[:n]) and np.array_equal(a.new_pos[:n], b.new_pos[:n])
    for r in range(n):
        assert np.array_equal(a.cigars[r], b.cigars[r]), r


@pytest.mark.parametrize("flank,letters", cases.TABLE_CASES)
def test_operator_pair_table(hip_engine, flank, letters):
    inputs, _ = cases.table(flank, letters)
    _hold(inputs, _project(hip_engine, inputs), _expected(("table", flank, letters), inputs))


@pytest.mark.parametrize("letters", (4, 2))
def test_builder_rules_on_the_alignment_side(hip_engine, letters):
    inputs = cases.rules(letters)
    _hold(inputs, _project(hip_engine, inputs), _expected(("rules", letters), inputs))


@pytest.mark.parametrize("u", sorted(cases.UNITS))
def test_left_alignment_in_repeats(hip_engine, u):
    inputs = cases.repeats(u)
    _hold(inputs, _project(hip_engine, inputs), _expected(("repeats", u), inputs))


def test_plain_boundary(hip_engine):
    inputs, _ = cases.plain()
    _hold(inputs, _project(hip_engine, inputs), _expected(("plain",), inputs))


@pytest.mark.parametrize("cls", range(len(cases.RANDOM_CLASSES)), ids=["%s-%s" % c for c in cases.RANDOM_CLASSES])
def test_random_alignments(hip_engine, cls):
    inputs = cases.random_alignments(cls)
    _hold(inputs, _project(hip_engine, inputs), _expected(("random", cls), inputs))


def test_workspace_boundary_27_28_29_elements(hip_engine):
    """The lanes' builders in LDS up to 28 elements (exactly 64 KB), in HBM at 29: the oracle's answer either way, and the
    reads the three batches share come out bit-equal."""
    got = {}
    for n_total in (27, 28, 29):
        inputs, long_read, _ = cases.workspace(n_total)
        assert sum(cases.host_max(inputs)) == n_total
        got[n_total] = _project(hip_engine, inputs)
        _hold(inputs, got[n_total], _expected(("workspace", n_total), inputs))
    for n_total in (27, 29):
        _same(got[28], got[n_total], long_read)


@pytest.mark.parametrize("n_reads,n_total", cases.COUNT_CASES)
def test_read_counts_around_the_block_sizes_and_the_lds_limit(hip_engine, n_reads, n_total):
    inputs = cases.count(n_reads, n_total)
    _hold(inputs, _project(hip_engine, inputs), _expected(("count", 4097, n_total), cases.count(4097, n_total))[:n_reads])


@pytest.mark.parametrize("n_total", (28, 29))
def test_4096_and_4097_reads_agree_on_the_reads_they_share(hip_engine, n_total):
    a, b = _project(hip_engine, cases.count(4096, n_total)), _project(hip_engine, cases.count(4097, n_total))
    _same(a, b, 4096)


@pytest.mark.parametrize("max_hc", (28 - cases.FUSED_SW_SLOTS, 29 - cases.FUSED_SW_SLOTS))
def test_fused_entry_point_at_the_boundary(hip_engine, max_hc):
    """phmm_realign_reads sizes the builders by its own alignment slots (24) plus the longest haplotype CIGAR: 4 and 5 elements
    put it at 28 and 29.  Alignments made on the device, output slots too small at first: equal to phmm_project_to_reference
    on the same reads, and to the oracle."""
    b, hap_cigars, hap_starts, ref_hap, ref_start, orig_cigars = scenario(31, n_regions=7, low_complexity=True)
    for a, c in enumerate(hap_cigars):   # longer haplotype CIGARs end in one M over the rest of the haplotype
        if len(c) > max_hc:
            rest = sum(int(e) >> 4 for e in c[max_hc - 1:] if cases.OPS[int(e) & 15] in cases.ON_READ)
            hap_cigars[a] = np.concatenate([c[:max_hc - 1], np.array([max(rest, 1) << 4], np.uint32)])
    assert max(len(c) for c in hap_cigars) == max_hc
    lk = hip_engine.compute(b)
    best0, aligned = realign.realign_reads_to_their_best_haplotype(hip_engine, b, lk)
    want = realign.project_to_reference(hip_engine, b, best0.allele_index, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig_cigars)
    best, got = realign.realign_reads(hip_engine, b, lk, hap_cigars, hap_starts, ref_hap, ref_start, orig_cigars, capacity=2)
    assert np.array_equal(best.allele_index, best0.allele_index)
    assert WORKSPACE_STATUS not in got.status and WORKSPACE_STATUS not in want.status
    _same(got, want, b.n_reads)
    reg = np.repeat(np.arange(b.n_regions), np.diff(b.region_read_off.astype(np.int64)))
    n_ok = 0
    for r in range(b.n_reads):
        st, pos, cig = scenario_oracle_read(b, r, reg[r], best.allele_index[r], hap_cigars, hap_starts, ref_hap, ref_start, orig_cigars)
        assert (int(got.status[r]), int(got.new_pos[r]), oracle.cigar_to_string(got.cigars[r])) == (st, pos, cig), r
        n_ok += st == 0
    assert n_ok > b.n_reads // 2


SLACK, SENTINEL = 0xFFFFFFFF, 0xA5A5A5A5


def _raw(eng, inputs, sw_slots, out_caps):
    """phmm_project_to_reference itself: alignment slots of sw_slots[r] words with SLACK behind the read's elements, output slots
    of out_caps[r] words in an array full of SENTINEL with one more word behind the last slot."""
    b, best, aligned, hap_cigars, hap_starts, ref_hap, ref_start, orig = inputs
    n = b.n_reads
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    off = lambda sizes, t: np.concatenate([[0], np.cumsum(sizes)]).astype(t)  # noqa: E731
    cat = lambda xs: np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(x, np.uint32) for x in xs]).astype(np.uint32)  # noqa: E731
    sw_n = np.array([len(a.elements) for a in aligned], np.uint32)
    assert np.all(np.asarray(sw_slots) >= sw_n)
    sw_off = off(sw_slots, np.uint64)
    sw = np.full(int(sw_off[-1]), SLACK, np.uint32)
    for r, a in enumerate(aligned):
        sw[int(sw_off[r]):int(sw_off[r]) + len(a.elements)] = a.elements
    sw_offset = np.array([a.alignment_offset for a in aligned], np.int32)
    hc_off, hc = off([len(c) for c in hap_cigars], np.uint32), cat(hap_cigars)
    oc_off, oc = off([len(c) for c in orig], np.uint32), cat(orig)
    hs, rrh, rs = np.asarray(hap_starts, np.uint32), np.asarray(ref_hap, np.int32), np.asarray(ref_start, np.uint64)
    out_off = off(out_caps, np.uint64)
    out = np.full(int(out_off[-1]) + 1, SENTINEL, np.uint32)
    n_out, pos, status = np.full(n, 0x7777, np.uint32), np.full(n, -7, np.int64), np.full(n, 77, np.int32)
    code = eng.lib.phmm_project_to_reference(
        eng._h, b.n_regions, p(b.region_read_off, _lib.u32p), p(b.region_hap_off, _lib.u32p), p(b.read_off, _lib.u32p), p(b.read_bases, _lib.u8p),
        p(b.hap_off, _lib.u32p), p(b.hap_bases, _lib.u8p), p(rrh, i32p), p(rs, _lib.u64p), p(hc_off, _lib.u32p), p(hc, _lib.u32p), p(hs, _lib.u32p),
        p(np.ascontiguousarray(best, np.int32), i32p), p(sw_off, _lib.u64p), p(sw, _lib.u32p), p(sw_n, _lib.u32p), p(sw_offset, i32p),
        p(oc_off, _lib.u32p), p(oc, _lib.u32p), p(out_off, _lib.u64p), p(out, _lib.u32p), p(n_out, _lib.u32p), p(pos, i64p), p(status, i32p))
    return code, status, pos, n_out, out, out_off


def test_raw_call_with_slack_in_the_alignment_slots_and_guarded_output_slots(hip_engine):
    """Alignment slots wider than the alignments (0xFFFFFFFF behind them), output slots of unequal widths -- some one element too
    small, some exact, some wider -- in an array of sentinel words: the call reports PHMM_ERR_CIGAR_CAPACITY and the size every
    realigned read needs, writes nothing but the elements it reports (every word behind a read's elements, the slots of reads
    that are not realigned and the word behind the last slot stay), and the slack changes no result; the second call with
    max(cap, n_out) is PHMM_OK with the oracle's CIGARs."""
    eng = hip_engine
    inputs = cases.rules(4)
    expected = _expected(("rules", 4), inputs)
    n = inputs[0].n_reads
    need = np.array([len(cases.elements(cig)) if st == 0 else 0 for st, _, cig in expected], np.int64)
    r = np.arange(n)
    caps = np.where(need > 0, np.choose(r % 3, [need - 1, need, need + 1 + r % 4]), r % 3)
    assert ((caps < need).sum() > 100) and ((caps > need).sum() > 100) and (caps == 0).any()
    sw_n = np.array([len(a.elements) for a in inputs[2]], np.int64)
    exact = realign.project_to_reference(eng, *inputs)      # alignment slots without slack
    _hold(inputs, exact, expected)

    def guards_intact(out, out_off, n_out, cap):
        assert out[-1] == SENTINEL and len(out) == int(out_off[-1]) + 1
        for k in range(n):
            used = min(int(n_out[k]), int(cap[k]))
            assert np.all(out[int(out_off[k]) + used:int(out_off[k + 1])] == SENTINEL), cases.describe(inputs, k)

    code, status, pos, n_out, out, out_off = _raw(eng, inputs, sw_n + r % 4, caps)
    assert code == _lib.PHMM_ERR_CIGAR_CAPACITY, eng.last_error()
    assert np.array_equal(status, [st for st, _, _ in expected]) and np.array_equal(status, exact.status)
    assert np.array_equal(n_out, need) and np.array_equal(pos, exact.new_pos)
    guards_intact(out, out_off, n_out, caps)
    for k in np.flatnonzero((need > 0) & (caps >= need)):    # the reads whose slots were large enough have their CIGARs already
        assert oracle.cigar_to_string(out[int(out_off[k]):int(out_off[k]) + int(n_out[k])]) == expected[k][2], cases.describe(inputs, int(k))
    for k in np.flatnonzero(caps < need):                    # ... the others the elements that fitted
        assert np.array_equal(out[int(out_off[k]):int(out_off[k + 1])], exact.cigars[k][:int(caps[k])])

    grown = np.maximum(caps, n_out.astype(np.int64))
    code, status, pos, n_out, out, out_off = _raw(eng, inputs, sw_n + (r + 1) % 3, grown)
    assert code == _lib.PHMM_OK, eng.last_error()
    assert np.array_equal(status, exact.status) and np.array_equal(pos, exact.new_pos) and np.array_equal(n_out, need)
    assert WORKSPACE_STATUS not in status
    guards_intact(out, out_off, n_out, grown)
    for k, (st, _, cig) in enumerate(expected):
        assert oracle.cigar_to_string(out[int(out_off[k]):int(out_off[k]) + int(n_out[k])]) == (cig if st == 0 else ""), cases.describe(inputs, k)
