"""The pre-step (prepdev::prep_read_wave, tandem_repeat_length; lorikeet_amd/csrc/phmm_prep_device.hpp) on the MI355X, through
every route that launches it, on the inputs of tests/prestep_cases.py -- unit lengths 1 ... 20, the cap at 100, repeats behind
read positions 64, 128 and 192, forward units that differ from the backward ones, tags on either side of the cache, base
qualities at both clamps of the dynamic table, the steps of ceil(n * rate), reads that need more than 64 KiB of LDS:
  A  phmm_engine_compute, a case as it is: few reads, a wave per 64 read positions;
  B  phmm_engine_compute, the reads cycled to just over 2 048 in one call: one wave per read, strides of 64;
  C  phmm_region_compute, launched;
  D  phmm_region_compute through the resident region server: one wave per read, the server's own row count.
Every route is held to the oracle pipeline (likelihoods at test_hip_parity.TOL_VS_ORACLE, never NaN, never positive; keep
flags equal on every read), C to D and A to C at 1e-11, every route to itself bit for bit.  Best allele, position and CIGAR are
compared between C and D only: repeats make alignments ambiguous, and the cases set no margins for them.
tests/test_prestep_table.py proves on the CPU that a wrong scan, quality rule or threshold would move these likelihoods by a
thousand tolerances or flip a keep flag."""
import ctypes as C

import numpy as np
import pytest

import prestep_cases as pc
import server_instance_cases as server_cases
from lorikeet_amd import _lib, region
from lorikeet_amd.engine import HipPairHMMEngine
from test_hip_parity import TOL_VS_ORACLE
from test_server_hip import _equal

pytestmark = pytest.mark.gpu
FILL_OUT, FILL_KEEP = 0x7FF8ABCDABCDABCD, 0xAB     # (a NaN no kernel writes)


@pytest.fixture(scope="module")
def launched():
    e = HipPairHMMEngine(0)
    e.set_switch("region_server", 0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def served():
    e = HipPairHMMEngine(0)
    e.set_switch("region_server", 1)
    yield e
    e.close()


def _engine(eng, c, tags):
    """phmm_engine_compute; tags False: ins_q / del_q NULL.  Returns (code, likelihoods, keep) over filled outputs."""
    b = c.batch
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    out, keep = np.full(b.n_out, FILL_OUT, np.uint64).view(np.float64), np.full(b.n_reads, FILL_KEEP, np.uint8)
    mq, rr = np.ascontiguousarray(c.mapq, np.uint8), np.ascontiguousarray(c.ref_hap, np.int32)
    code = eng.lib.phmm_engine_compute(eng._h, C.byref(c.cfg), b.n_regions, p(b.region_read_off, _lib.u32p), p(b.region_hap_off, _lib.u32p),
                                       p(b.read_off, _lib.u32p), p(b.read_bases, _lib.u8p), p(b.base_q, _lib.u8p), p(b.ins_q, _lib.u8p) if tags else None,
                                       p(b.del_q, _lib.u8p) if tags else None, p(mq, _lib.u8p), p(b.hap_off, _lib.u32p), p(b.hap_bases, _lib.u8p),
                                       p(rr, C.POINTER(C.c_int32)), p(b.out_off, _lib.u64p), p(out, _lib.f64p), p(keep, _lib.u8p))
    return code, out, keep


def _region(eng, c, tags):
    return region.region_compute(eng, c.cfg, c.batch, c.mapq, c.hap_cigars, c.hap_starts, c.ref_hap, c.ref_start, c.orig_cigars, hap_priority=c.pri,
                                 use_indel_quals=tags, capacity=server_cases.OUT_CIGAR_SLOTS)


def _holds(route, name, likelihoods, keep, want_likelihoods, want_keep):
    assert likelihoods.shape == want_likelihoods.shape
    assert not np.isnan(likelihoods).any() and (likelihoods <= 0).all(), (route, name)
    worst = float(np.max(np.abs(likelihoods - want_likelihoods)))
    print("%s %s: max |hip - oracle| = %.3g" % (route, name, worst))
    assert worst < TOL_VS_ORACLE, (route, name, worst)
    assert np.array_equal(np.asarray(keep, bool), want_keep), (route, name, np.flatnonzero(np.asarray(keep, bool) != want_keep))


@pytest.mark.parametrize("name", pc.CONFIG_NAMES)
def test_every_route_equals_the_oracle_pipeline(launched, served, name):
    c = pc.case(name)
    tags = pc.uses_tags(c)
    want = pc.expected(c)
    assert pc.waves_per_read(c.batch.n_reads, server_cases.max_r(c)) > 1          # A and C: several waves per read
    # A
    code, a_out, a_keep = _engine(launched, c, tags)
    assert code == _lib.PHMM_OK, launched.last_error()
    _holds("A", name, a_out, a_keep, want.likelihoods, want.keep)
    code, again_out, again_keep = _engine(launched, c, tags)
    assert code == _lib.PHMM_OK and np.array_equal(again_out, a_out) and np.array_equal(again_keep, a_keep)
    # C
    got_c = _region(launched, c, tags)
    _holds("C", name, got_c.likelihoods, got_c.keep, want.likelihoods, want.keep)
    _equal(_region(launched, c, tags), got_c, exact=True)
    # D
    jobs = served.stat("server_jobs")
    got_d = _region(served, c, tags)
    assert served.stat("server_jobs") == jobs + 1, "%s did not go through the region server" % name
    again = _region(served, c, tags)
    assert served.stat("server_jobs") == jobs + 2 and served.stat("server_broken") == 0, name
    _holds("D", name, got_d.likelihoods, got_d.keep, want.likelihoods, want.keep)
    _equal(again, got_d, exact=True)
    # between the routes
    print("%s: max |D - C| = %.3g, max |A - C| = %.3g" % (name, float(np.max(np.abs(got_d.likelihoods - got_c.likelihoods))),
                                                        float(np.max(np.abs(a_out - got_c.likelihoods)))))
    _equal(got_d, got_c, exact=False)
    assert np.max(np.abs(a_out - got_c.likelihoods)) < 1e-11 and np.array_equal(a_keep.astype(bool), got_c.keep), name


def test_more_than_2048_reads_in_one_engine_call(launched):
    """B: one wave per read, so every repeat behind position 63 is met on a later trip of the wave's stride loop."""
    c, first = pc.multiplied_case()
    b = c.batch
    assert b.n_reads > pc.SMALL_CALL_READS and pc.waves_per_read(b.n_reads, server_cases.max_r(c)) == 1 and int(b.read_off[-1]) <= pc.ONE_SHOT_BYTES
    want_out, want_keep = pc.expected_multiplied()
    code, out, keep = _engine(launched, c, True)
    assert code == _lib.PHMM_OK, launched.last_error()
    _holds("B", c.name, out, keep, want_out, want_keep)
    for g, f in enumerate(first):          # every copy of a region gives the bits of its first copy
        assert np.array_equal(out[int(b.out_off[g]):int(b.out_off[g + 1])], out[int(b.out_off[f]):int(b.out_off[f + 1])]), (g, f)
        assert np.array_equal(keep[int(b.region_read_off[g]):int(b.region_read_off[g + 1])], keep[int(b.region_read_off[f]):int(b.region_read_off[f + 1])]), (g, f)
    code, again_out, again_keep = _engine(launched, c, True)
    assert code == _lib.PHMM_OK and np.array_equal(again_out, out) and np.array_equal(again_keep, keep)


def test_the_routes_see_the_model(launched):
    """The same reads without the PCR model give other numbers (the check tests/test_golden_repetitions.py makes)."""
    with_model, without = pc.case("conservative-static-null"), pc.case("none-static-null")
    assert np.array_equal(with_model.batch.read_bases, without.batch.read_bases) and np.array_equal(with_model.batch.base_q, without.batch.base_q)
    assert (with_model.cfg.pcr_error_model, without.cfg.pcr_error_model) == (3, 0)
    (code3, out3, _), (code0, out0, _) = _engine(launched, with_model, False), _engine(launched, without, False)
    assert code3 == code0 == _lib.PHMM_OK
    assert np.max(np.abs(out3 - out0)) > 1e-3


def test_reads_that_need_more_than_64_kib_of_lds_and_the_first_one_refused(launched):
    """launch_prep asks for lds_rows * 17 * 4 bytes: past 64 KiB through hipFuncSetAttribute, up to kLdsBytesPerCU; one base more
    is refused before anything is launched, nothing is written, and the handle goes on."""
    for n in pc.LONG_LENGTHS:
        c = pc.long_case(n)
        assert (pc.lds_bytes(n) > pc.LDS_DEFAULT_LIMIT) == (n >= pc.FIRST_OVER_64K) and pc.lds_bytes(n) <= pc.LDS_BYTES_PER_CU
        want = pc.expected(c)
        code, out, keep = _engine(launched, c, False)
        assert code == _lib.PHMM_OK, (n, launched.last_error())
        _holds("A", c.name, out, keep, want.likelihoods, want.keep)
    c = pc.long_case(pc.REFUSED_LENGTH)
    assert pc.lds_bytes(pc.REFUSED_LENGTH) > pc.LDS_BYTES_PER_CU
    code, out, keep = _engine(launched, c, False)
    assert code == _lib.PHMM_ERR_INVALID_ARG and "read too long for the pre-step kernel" in launched.last_error()
    assert (out.view(np.uint64) == FILL_OUT).all() and (keep == FILL_KEEP).all()
    small = server_cases.split(pc.case("hostile-static-tags"))[20]           # the handle still computes: one region of a plain case
    code, out, keep = _engine(launched, small, True)
    assert code == _lib.PHMM_OK, launched.last_error()
    plain, e = pc.case("hostile-static-tags"), pc.expected(pc.case("hostile-static-tags"))
    o0, o1, r0, r1 = (int(x) for x in (plain.batch.out_off[20], plain.batch.out_off[21], plain.batch.region_read_off[20], plain.batch.region_read_off[21]))
    _holds("A", small.name, out, keep, e.likelihoods[o0:o1], e.keep[r0:r1])
