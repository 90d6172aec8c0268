"""phmm_finalize_reads on the MI355X against the restatement of the reference's read finalization
(tests/finalize_restatement.py), through the C ABI as lorikeet_amd.finalize binds it.  EQUALITY on every output array: it is all
integers and bytes, there are no tolerances.  The reads come from tests/finalize_cases.py; tests/test_finalize_oracle.py holds
the restatement to the reference's own tests and counts on the CPU what the sets exercise.  The module imports
lorikeet_amd.finalize at the top: without the call every test here fails."""
import numpy as np
import pytest

import finalize_cases as K
import finalize_restatement as R
from lorikeet_amd import _lib, finalize
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
SCALARS = ("read_status", "keep", "new_pos", "out_unmapped", "clip_first", "clip_len", "unclipped_len", "lead_soft", "trail_soft")
NAMES = [c[0] for c in K.sets()]
DEFAULTS = dict(steps=_lib.PHMM_FIN_ALL, min_tail_quality=9)


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def per_read(res):
    """every output of a call cut into its reads: [{name: value or bytes}]"""
    out = []
    for r in range(len(res.read_status)):
        d = {k: int(getattr(res, k)[r]) for k in SCALARS if getattr(res, k) is not None}
        if res.out_cigar is not None:
            d["out_cigar"] = [(int(x) & 15, int(x) >> 4) for x in res.cigar(r)]
        if res.out_quals is not None:
            d["out_quals"] = res.quals(r).tolist()
        out.append(d)
    return out


def same(got, want, tag):
    assert len(got) == len(want), tag
    for r, (g, w) in enumerate(zip(got, want)):
        for k in g:
            assert g[k] == w[k], (tag, "read", r, k, g[k], w[k])


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_restatement(eng, name):
    _, groups, options = K.case(name)
    res = finalize.finalize_reads(eng, groups, fill=0xAB, **options)
    same(per_read(res), K.restated(name), name)
    # room of out_cigar a read does not use stays as the caller left it
    used = np.zeros(len(res.out_cigar), bool)
    for r in range(len(res.read_status)):
        used[int(res.out_cigar_off[r]):int(res.out_cigar_off[r]) + int(res.n_out_cigar[r])] = True
    assert np.all(res.out_cigar[~used] == 0xABABABAB), name


def test_alone_and_together_give_the_same_bytes_and_so_does_a_second_call(eng):
    """every set alone and all of them in one call, under one configuration; the big call twice"""
    everything = [g for _, groups, _ in K.sets() for g in groups]
    first = per_read(finalize.finalize_reads(eng, everything, **DEFAULTS))
    again = per_read(finalize.finalize_reads(eng, everything, **DEFAULTS))
    assert first == again
    at = 0
    for name, groups, _ in K.sets():
        alone = per_read(finalize.finalize_reads(eng, groups, **DEFAULTS))
        assert alone == first[at:at + len(alone)], name
        at += len(alone)
    assert at == len(first)
    # ... and the reads one group each: a pair's reads stay together, nothing else decides anything
    _, groups, options = K.case("pairs")
    together = per_read(finalize.finalize_reads(eng, groups, **options))
    split = [r for g in groups for r in per_read(finalize.finalize_reads(eng, [g], **options))] if groups else []
    assert split == together


def test_empty_calls_empty_groups_and_null_outputs(eng):
    assert len(finalize.finalize_reads(eng, []).read_status) == 0
    assert len(finalize.finalize_reads(eng, [K.group([]), K.group([], (5, 9))]).read_status) == 0
    name = "pairs"
    _, groups, options = K.case(name)
    groups = [K.group([])] + list(groups) + [K.group([])]
    full = per_read(finalize.finalize_reads(eng, groups, **options))
    same(full, K.restated(name), name)
    for omit in [(k,) for k in finalize.OUTPUTS if k not in ("read_status", "n_out_cigar")] + [("out_cigar", "n_out_cigar"), tuple(finalize.OUTPUTS[1:])]:
        res = finalize.finalize_reads(eng, groups, omit=omit, **options)
        assert all(getattr(res, k) is None for k in omit)
        part = per_read(res)
        for g, w in zip(part, full):
            assert g == {k: w[k] for k in g}, omit
    # without the pair step neither mate_index nor the bases are needed
    a = finalize.pack(groups)
    a["mate_index"] = a["read_bases"] = None
    steps = _lib.PHMM_FIN_ALL & ~_lib.PHMM_FIN_PAIRS
    assert per_read(finalize.finalize_reads(eng, a, steps=steps)) == per_read(finalize.finalize_reads(eng, groups, steps=steps))


def test_staging_grows_from_a_small_call_to_a_larger_one():
    e = HipPairHMMEngine()
    try:
        for name in ("pair panics", "random %d" % K.RANDOM_SEEDS[0], "pair panics"):
            _, groups, options = K.case(name)
            same(per_read(finalize.finalize_reads(e, groups, **options)), K.restated(name), name)
    finally:
        e.close()


def broken(change):
    """the arrays of a small valid call with one thing wrong"""
    rd = K.read
    groups = [K.group(K.mates("20M", 100, "5S15M", 110) + [rd("3S10M2D7M", 90)], (50, 150)), K.group([rd("10M", 10)], (0, 20))]
    a = finalize.pack(groups)
    change(a)
    return a


def put(key, index, value):
    def change(a):
        a[key] = a[key].copy()
        a[key][index] = value
    return change


def null(key):
    def change(a):
        a[key] = None
    return change


INVALID = {
    "group_read_off does not start at 0": put("group_read_off", 0, 1),
    "group_read_off decreases": put("group_read_off", 1, 5),
    "read_cigar_off does not start at 0": put("read_cigar_off", 0, 1),
    "read_cigar_off decreases": put("read_cigar_off", 1, 9),
    "read_off does not start at 0": put("read_off", 0, 1),
    "read_off decreases": put("read_off", 2, 1),
    "out_cigar_off does not start at 0": put("out_cigar_off", 0, 1),
    "out_cigar_off decreases": put("out_cigar_off", 1, 99),
    "out_cigar_off leaves room for 2 elements, 3 are needed": put("out_cigar_off", 1, 2),
    "read 1 (group 0): CIGAR element 0: operator above 8 or length 0": put("read_cigar", 1, (5 << 4) | 9),
    "read 0 (group 0): CIGAR element 0: operator above 8 or length 0": put("read_cigar", 0, 0),
    "read 0 (group 0): the CIGAR's read length 21 differs from the read's 20 bases": put("read_cigar", 0, 21 << 4),
    "group 1: span_end < span_start": put("group_span_start", 1, 30),
    "group 0: span position from 2^62 on": put("group_span_end", 0, 1 << 62),
    "read 2 (group 0): pos is negative or from 2^62 on": put("read_pos", 2, 1 << 62),
    "read 3 (group 1): pos is negative or from 2^62 on": put("read_pos", 3, -1),
    "read 0 (group 0): mpos position from 2^62 on": put("read_mpos", 0, -(1 << 62)),
    "read 1 (group 0): isize position from 2^62 on": put("read_isize", 1, 1 << 62),
    "read 2 (group 0): mate_index 3 is out of its group": put("mate_index", 2, 3),
    "read 3 (group 1): mate_index -2 is out of its group": put("mate_index", 3, -2),
    "read 2 (group 0): mate_index is self-referential": put("mate_index", 2, 2),
    "read 0 (group 0): mate_index is not symmetric": put("mate_index", 0, 2),
    "PHMM_FIN_PAIRS needs mate_index, which is NULL": null("mate_index"),
    "a required pointer is NULL (group arrays)": null("group_span_start"),
    "a required pointer is NULL (read arrays)": null("read_flags"),
    "a required pointer is NULL (read_cigar, read_quals, or read_bases with PHMM_FIN_PAIRS)": null("read_bases"),
    "a required pointer is NULL (out_cigar without out_cigar_off or n_out_cigar)": null("out_cigar_off"),
}


@pytest.mark.parametrize("message", sorted(INVALID))
def test_invalid_arguments_are_named_and_nothing_is_written(eng, message):
    with pytest.raises(PhmmError) as err:
        finalize.finalize_reads(eng, broken(INVALID[message]), fill=0xAB)
    assert err.value.code == _lib.PHMM_ERR_INVALID_ARG
    assert message in str(err.value), str(err.value)
    for k, v in err.value.outputs.items():
        assert np.all(np.frombuffer(v.tobytes(), np.uint8) == 0xAB), k
    # the call still works afterwards
    assert finalize.finalize_reads(eng, broken(lambda a: None)).read_status.tolist() == [0, 0, 0, 0]


def test_invalid_arguments_that_are_not_arrays(eng):
    good = broken(lambda a: None)
    for kw, message in ((dict(steps=32), "steps holds bits outside PHMM_FIN_ALL"),
                        (dict(omit=("read_status",)), "a required pointer is NULL (read arrays)"),
                        (dict(omit=("n_out_cigar",)), "a required pointer is NULL (out_cigar without out_cigar_off or n_out_cigar)")):
        with pytest.raises(PhmmError) as err:
            finalize.finalize_reads(eng, good, fill=0xAB, **kw)
        assert err.value.code == _lib.PHMM_ERR_INVALID_ARG and message in str(err.value), str(err.value)
    assert eng.lib.phmm_finalize_reads(eng._h, None, 0, *([None] * 27)) == _lib.PHMM_ERR_INVALID_ARG
    assert "cfg is NULL" in eng.last_error()
