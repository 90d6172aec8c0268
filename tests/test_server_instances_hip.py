"""Every compiled instance of the resident region server (lorikeet_amd/csrc/phmm_server.cpp, phmm_server_kernels.hip) against
the oracle pipeline, each at the haplotype lengths that select it:
  forward sweep  forward_read<16, K>, K = 2 ... 25, and forward_read<32, K>, K = 13 ... 16: 28 instances, each at the shortest and
                 at the longest haplotype the host's rule sends to it (<16, 2> also at 1 and 16 bases);
  aligner        sw_align_body<64, K, true>, K in 2, 3, 4, 5, 6, 8: those lengths hold every boundary of its table;
  groups         1 ... 33 haplotypes against the wave's slots (four at 16 lanes, two at 32) and the post-step's 16 registers, helper
                 waves with nothing to do, a small region in a large one's geometry;
  edges          a read of SRV_MAX_ROWS rows, N in a haplotype and in a read, mapq 0, the error models and both normalisations;
  declined       one step past each limit, beside the accepted neighbour; an alignment that outgrows the server's 24 elements.
The server is the default route of a private handle's phmm_region_compute once more than five handles are alive on a device;
every `switch` over its instance tables ends in `default: break;`, so a wrong selection is a result that was never written.

Held to the oracle (likelihoods at test_hip_parity.TOL_VS_ORACLE, never NaN, never positive; keep, best allele, projection
status, position and CIGAR of EVERY read equal -- tests/test_server_instance_table.py keeps the inputs a thousand tolerances
away from every threshold those hang on), to the launched pipeline (likelihoods at 1e-11, everything discrete equal) and to
itself, bit for bit.  The inputs are tests/server_instance_cases.py's: no GPU needed to build or to judge them.

Cost: the oracle is asked for 5.7e7 cells by this file (83 calls of about a dozen reads by a handful of haplotypes, each
computed once per process); on the MI355X its 53 tests take 3.3 s together, 1.6 s of that the first handle's set-up, the
slowest test 0.1 s."""
import numpy as np
import pytest

import server_instance_cases as cases
from lorikeet_amd import region
from lorikeet_amd.engine import HipPairHMMEngine
from oracle import oracle
from test_hip_parity import TOL_VS_ORACLE
from test_server_hip import _equal

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = HipPairHMMEngine(0)
    e.set_switch("region_server", 1)  # (every call through the server, also the lone ones a test makes)
    yield e
    e.close()


@pytest.fixture(scope="module")
def launched():
    e = HipPairHMMEngine(0)
    e.set_switch("region_server", 0)
    yield e
    e.close()


def _call(e, c):
    return region.region_compute(e, c.cfg, c.batch, c.mapq, c.hap_cigars, c.hap_starts, c.ref_hap, c.ref_start, c.orig_cigars, hap_priority=c.pri,
                                 capacity=cases.OUT_CIGAR_SLOTS)


def _equals_the_oracle(got, c):
    want = cases.expected(c)
    assert got.likelihoods.shape == want.likelihoods.shape
    print("%s: max |hip - oracle| = %.3g" % (c.name, float(np.max(np.abs(got.likelihoods - want.likelihoods)))))
    assert not np.isnan(got.likelihoods).any() and (got.likelihoods <= 0).all(), c.name
    assert np.max(np.abs(got.likelihoods - want.likelihoods)) < TOL_VS_ORACLE, c.name
    assert np.array_equal(got.keep, want.keep), (c.name, np.flatnonzero(got.keep != want.keep))
    assert np.array_equal(got.best.allele_index, want.best), (c.name, np.flatnonzero(got.best.allele_index != want.best))
    for r, (st, pos, cig) in enumerate(want.reads):
        assert got.reads.status[r] == st, (c.name, r, got.reads.status[r], st)
        if st == 0:
            assert got.reads.new_pos[r] == pos and oracle.cigar_to_string(got.reads.cigars[r]) == cig, (c.name, r)


def _through_the_server(eng, launched, c):
    """Two calls through the server (counted, the same bits), one launched: the oracle's results, the launched pipeline's."""
    jobs = eng.stat("server_jobs")
    got = _call(eng, c)
    assert eng.stat("server_jobs") == jobs + 1, "%s did not go through the region server" % c.name
    again = _call(eng, c)
    assert eng.stat("server_jobs") == jobs + 2 and eng.stat("server_broken") == 0, c.name
    _equals_the_oracle(got, c)
    want = _call(launched, c)
    assert eng.stat("server_jobs") == jobs + 2
    print("%s: max |server - launched| = %.3g" % (c.name, float(np.max(np.abs(got.likelihoods - want.likelihoods)))))
    _equal(got, want, exact=False)
    _equal(again, got, exact=True)
    return got


@pytest.mark.parametrize("instance", cases.FORWARD_INSTANCES, ids=lambda lk: "L%d-K%d" % lk)
def test_every_forward_instance_at_both_ends_of_its_range(eng, launched, instance):
    L, K = instance
    for name in cases.INSTANCE_NAMES[instance]:
        c = cases.case(name)
        assert cases.geometry(cases.max_h(c))[:2] == (L, K)
        _through_the_server(eng, launched, c)


@pytest.mark.parametrize("name", cases.GROUP_NAMES)
def test_haplotype_counts_against_the_waves_slots_and_the_post_steps_registers(eng, launched, name):
    c = cases.case(name)
    got = _through_the_server(eng, launched, c)
    b = c.batch
    if b.n_regions == 1:
        return
    # each region alone: its own geometry (the call's follows the call's longest haplotype), the same results
    jobs = eng.stat("server_jobs")
    for g, one in enumerate(cases.split(c)):
        alone = _call(eng, one)
        r0, r1, o0, o1 = (int(x) for x in (b.region_read_off[g], b.region_read_off[g + 1], b.out_off[g], b.out_off[g + 1]))
        assert np.max(np.abs(alone.likelihoods - got.likelihoods[o0:o1])) < 1e-11, (name, g)
        assert np.allclose(alone.best.likelihood, got.best.likelihood[r0:r1], rtol=0, atol=1e-11, equal_nan=True)
        assert np.array_equal(alone.keep, got.keep[r0:r1]) and np.array_equal(alone.best.allele_index, got.best.allele_index[r0:r1]), (name, g)
        assert np.array_equal(alone.reads.status, got.reads.status[r0:r1]) and np.array_equal(alone.reads.new_pos, got.reads.new_pos[r0:r1]), (name, g)
        for r in range(r0, r1):
            assert np.array_equal(alone.reads.cigars[r - r0], got.reads.cigars[r]), (name, g, r)
    assert eng.stat("server_jobs") == jobs + b.n_regions and eng.stat("server_broken") == 0


@pytest.mark.parametrize("name", cases.EDGE_NAMES)
def test_the_edges_of_what_the_server_takes(eng, launched, name):
    _through_the_server(eng, launched, cases.case(name))


@pytest.mark.parametrize("name", sorted(cases.NEIGHBOUR))
def test_one_step_past_a_limit_the_call_takes_the_launched_pipeline(eng, launched, name):
    c, near = cases.case(name), cases.case(cases.NEIGHBOUR[name])
    jobs = eng.stat("server_jobs")
    got = _call(eng, c)
    assert eng.stat("server_jobs") == jobs, "%s went through the region server" % name
    _equal(got, _call(launched, c), exact=True)        # (it IS the launched pipeline)
    _equals_the_oracle(got, c)
    _equals_the_oracle(_call(eng, near), near)         # ... and its accepted neighbour goes through the server
    assert eng.stat("server_jobs") == jobs + 1 and eng.stat("server_broken") == 0


def test_an_alignment_that_outgrows_the_servers_slots_is_run_again_by_the_launched_pipeline(eng, launched):
    """kServerRedo.  The host takes the call (server_region_submit counts it: n_jobs rises when the ring entry is published), the
    aligner reports that 24 elements do not hold read 0's alignment, server_region_wait hands the call to the launched pipeline."""
    c = cases.case("sw-capacity")
    jobs = eng.stat("server_jobs")
    got = _call(eng, c)
    assert eng.stat("server_jobs") == jobs + 1 and eng.stat("server_broken") == 0
    _equal(got, _call(launched, c), exact=False)
    _equals_the_oracle(got, c)
    st, pos, cig = cases.expected(c).reads[0]
    assert st == 0 and got.reads.status[0] == 0 and got.reads.new_pos[0] == pos and oracle.cigar_to_string(got.reads.cigars[0]) == cig
    assert cig.count("D") >= 13 and len(got.reads.cigars[0]) > cases.SW_CAPACITY
    again = _call(eng, c)                               # the server is still there for the next call
    assert eng.stat("server_jobs") == jobs + 2 and eng.stat("server_broken") == 0
    _equal(again, got, exact=True)
