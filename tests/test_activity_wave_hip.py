"""phmm_activity_profile on the MI355X past the first trip of activity_read_kernel's lane-strided loops, at G = 4, 8, 9, 16, 17 of
activity_site_kernel<CH>, down both routes of the allele-frequency step and at the edges of the two launch grids, against the
restatement with the claims of tests/test_activity_hip.py (`same`: equality on the integers, bit for bit on gl, the soft-clip
mean, is_active_prob and the band-passed lists, QUAL within 1e-12 relative with equal flags) and no other tolerance.  The
windows and their witnesses come from tests/activity_wave_cases.py; tests/test_activity_wave_table.py counts on the CPU what
they cross.  Each test prints how many positions it compared and how many differ."""
import numpy as np
import pytest

import activity_restatement as R
import activity_wave_cases as W
from lorikeet_amd import _lib, activity
from lorikeet_amd.engine import HipPairHMMEngine
from test_activity_hip import PER_SAMPLE, bits, per_window, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def run(eng, windows, o, **kw):
    return activity.activity_profile(eng, windows, **o, **kw)


def differing(res, want):
    """The positions at which any per-position output differs from the restatement, under `same`'s claims."""
    bad = np.zeros(len(want["qual"]), bool)
    for k in ("read_counts", "ref_depth", "non_ref_depth", "pl", "gl"):
        a, b = getattr(res, k), want[k]
        bad |= (a.view(np.uint64 if k == "gl" else a.dtype) != b.view(np.uint64 if k == "gl" else b.dtype)).reshape(len(bad), -1).any(axis=1)
    for k in ("soft_clip_count", "af_flags"):
        bad |= getattr(res, k) != want[k]
    for k, t in (("soft_clip_mean", np.uint64), ("is_active_prob", np.uint32)):
        bad |= getattr(res, k).view(t) != want[k].view(t)
    with np.errstate(invalid="ignore"):
        bad |= ~((res.qual == want["qual"]) | (np.abs(res.qual - want["qual"]) <= 1e-12 * np.abs(want["qual"])))
    return np.flatnonzero(bad)


class Tally:
    def __init__(self, group):
        self.group, self.calls, self.positions, self.entries, self.differ = group, 0, 0, 0, 0

    def check(self, res, name):
        want = W.restated(name)[0]
        bad = differing(res, want)
        self.calls += 1
        self.positions += len(want["qual"])
        self.entries += sum(len(p) for p in want["profiles"])
        self.differ += len(bad)
        assert len(bad) == 0, (name, "positions that differ", bad[:10])
        same(res, want, name)

    def report(self):
        print("\n%s: %d calls, %d positions and %d band-passed list entries compared, %d differ" % (self.group, self.calls, self.positions, self.entries, self.differ))
        assert self.calls and self.positions and not self.differ


def at_witness(res, name, at, keys):
    want = W.restated(name)[0]
    for k in keys:
        assert bits(getattr(res, k)[at]) == bits(want[k][at]), "%s: %s at window position %d: %s, restated %s" % (name, k, at, getattr(res, k)[at], want[k][at])


def test_one_read_windows_with_long_elements(eng):
    """One call per window, the witness positions by name, then all the windows in one call."""
    cases = W.group("long") + W.group("clips")
    tally, singles = Tally("long elements and long clips, one read per window"), []
    for name, windows, o in cases:
        assert o == cases[0][2]
        res = run(eng, windows, o)
        for w in W.WITNESS[name]:
            if w["kind"] == "long":
                assert res.read_counts[w["at"], 0] == 1, "%s: no entry at window position %d" % (name, w["at"])
                at_witness(res, name, w["at"], ("read_counts", "ref_depth", "non_ref_depth", "gl", "pl"))
            else:
                assert (res.soft_clip_count[w["at"]], res.soft_clip_mean[w["at"]]) == (1, float(w["count"])), \
                    "%s: soft clips at window position %d: %s" % (name, w["at"], res.soft_clip_mean[w["at"]])
                at_witness(res, name, w["at"], ("soft_clip_mean", "soft_clip_count"))
        tally.check(res, name)
        singles += per_window(res)
    assert per_window(run(eng, [w for _, ws, _ in cases for w in ws], cases[0][2])) == singles
    tally.report()


def test_the_threshold_that_hangs_on_a_second_trip(eng):
    """Five reads whose clips count six bases each, all at clip offsets >= 64: the running average is 6.0, the state is emitted
    13 times and the band-passed list says so."""
    tally = Tally("soft-clip threshold")
    (high, windows, o), (low, low_windows, _) = W.threshold()
    a, b = run(eng, windows, o), run(eng, low_windows, o)
    at = W.THRESHOLD_AT
    assert (a.soft_clip_count[at], a.soft_clip_mean[at]) == (5, 6.0), "window position %d: %s" % (at, a.soft_clip_mean[at])
    assert (b.soft_clip_count[at], b.soft_clip_mean[at]) == (5, 0.0)
    tally.check(a, high)
    tally.check(b, low)
    assert a.is_active_prob[at] == b.is_active_prob[at] > 0 and bits(a.profile(0)) != bits(b.profile(0))
    tally.report()


@pytest.mark.parametrize("name", [c[0] for c in W.seeded()])
def test_seeded_windows_under_long_reads(eng, name):
    _, windows, o = W.case(name)
    tally = Tally(name)
    tally.check(run(eng, windows, o), name)
    tally.report()


def test_long_reads_repeat_and_batch_as_their_windows(eng):
    windows, o = W.repeated_windows()
    res = run(eng, windows, o)
    cut = per_window(res)
    assert per_window(run(eng, windows, o, fill=0xFF)) == cut
    for w, window in enumerate(windows):
        assert per_window(run(eng, [window], o))[0] == cut[w], w
    tally = Tally("the first of those windows")
    tally.check(run(eng, windows[:1], o), W.REPEATED)
    tally.report()


@pytest.mark.parametrize("ploidy", [p[0] for p in W.ROUTE_PAIRS])
def test_both_routes_of_the_allele_frequency_step(eng, ploidy):
    """The same window with a sample count on either side of af_is_block_event: both calls equal the restatement, and the
    samples they share have the same pileup."""
    _, wave, block, _, _ = next(p for p in W.ROUTE_PAIRS if p[0] == ploidy)
    assert not W.af_is_block_event(ploidy + 1, wave) and W.af_is_block_event(ploidy + 1, block)
    tally = Tally("allele-frequency routes, ploidy %d" % ploidy)
    res = {}
    for n in (wave, block):
        name, windows, o = W.case(W.route_name(ploidy, n))
        res[n] = run(eng, windows, o, fill=0xA5)
        tally.check(res[n], name)
    for k in PER_SAMPLE:
        assert bits(getattr(res[wave], k)[:, :7]) == bits(getattr(res[block], k)[:, :7]), k
    tally.report()


def test_launch_grid_edges(eng):
    """n_pos = 255, 256, 257, 512 over several windows, and one profile of 205, 206, 207 positions + 50 list entries behind
    them; every output holds a sentinel before the call."""
    tally = Tally("launch-grid edges")
    for name, windows, o in W.group("grids"):
        res = run(eng, windows, o, fill=0xA5)
        tally.check(res, name)
        if len(windows) == 1:
            n = len(windows[0][1])
            assert res.profile_len[0] == n + 50 and np.all(res.profile(0)[n:n + 20] > 0), (name, res.profile_len[0])
        else:
            for w, window in enumerate(windows):
                assert per_window(run(eng, [window], o, fill=0x5A))[0] == per_window(res)[w], (name, w)
    tally.report()


def test_both_ends_of_qual_as_u8(eng):
    tally = Tally("QUAL saturation")
    (high, windows, o), (low, low_windows, low_o) = W.group("quals")
    res = run(eng, windows, o)
    top = np.float32(R.qual_to_prob(255))
    for at in (W.QUAL_AT, W.QUAL_DEEP_AT):
        assert res.qual[at] >= 255.0 and res.af_flags[at] & _lib.PHMM_AF_CALLED and res.is_active_prob[at] == top, (at, res.qual[at], res.is_active_prob[at])
    assert np.isinf(res.qual[W.QUAL_AT + 1]) and res.is_active_prob[W.QUAL_AT + 1] == 0.0
    tally.check(res, high)
    res = run(eng, low_windows, low_o)
    assert res.qual[W.QUAL_AT] == 0.0 and res.af_flags[W.QUAL_AT] & _lib.PHMM_AF_CALLED and res.is_active_prob[W.QUAL_AT] == 0.0, res.qual[W.QUAL_AT]
    tally.check(res, low)
    tally.report()
