"""phmm_activity_profile on the MI355X against the restatement of the reference's activity profile
(tests/activity_restatement.py), through the C ABI as lorikeet_amd.activity binds it.  EQUALITY on the integers, bit for bit on
gl, the soft-clip mean and the band-passed f32 lists; QUAL within 1e-12 relative with equal flags; is_active_prob the table
value of the device's own `qual as u8`.  The windows come from tests/activity_cases.py; tests/test_activity_oracle.py checks
on the CPU what they exercise and that no QUAL lies near an integer.  The module imports lorikeet_amd.activity at the top:
without the call every test here fails."""
import numpy as np
import pytest

import activity_cases as K
import activity_restatement as R
from lorikeet_amd import _lib, activity
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
PER_SAMPLE = ("read_counts", "ref_depth", "non_ref_depth", "gl", "pl")
PER_POSITION = ("soft_clip_mean", "soft_clip_count", "qual", "af_flags", "is_active_prob")
GROUPS = (PER_SAMPLE, PER_POSITION, ("profile_prob", "profile_len"))


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def case(name):
    return next(c for c in K.all_cases() if c[0] == name)


def run(eng, windows, o, **kw):
    return activity.activity_profile(eng, windows, **o, **kw)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def same(res, want, tag):
    """The equality claims, array by array."""
    assert res.window_status.tolist() == want["window_status"].tolist(), tag
    for k in ("read_counts", "ref_depth", "non_ref_depth", "pl", "soft_clip_count", "af_flags"):
        assert np.array_equal(getattr(res, k), want[k]), (tag, k, np.argwhere(getattr(res, k) != want[k])[:5])
    for k in ("gl", "soft_clip_mean"):
        assert bits(getattr(res, k)) == bits(want[k]), (tag, k, np.argwhere(getattr(res, k) != want[k])[:5])
    q, wq = res.qual, want["qual"]
    with np.errstate(invalid="ignore"):
        close = (q == wq) | (np.abs(q - wq) <= 1e-12 * np.abs(wq))
    assert np.all(close), (tag, "qual", q[~close][:5], wq[~close][:5])
    table = np.array([np.float32(R.qual_to_prob(u)) for u in range(256)], np.float32)
    own = np.where(res.af_flags & _lib.PHMM_AF_CALLED, table[[R.saturating_u8(x) for x in q]] if len(q) else table[:0], np.float32(0.0))
    assert bits(res.is_active_prob) == bits(own.astype(np.float32)), (tag, "is_active_prob")
    assert bits(res.is_active_prob) == bits(want["is_active_prob"]), (tag, "is_active_prob against the restatement")
    assert res.filter_size == want["filter_size"], tag
    assert res.profile_window.tolist() == want["profile_window"] and res.profile_start.tolist() == want["profile_start"], tag
    assert res.profile_len.tolist() == [len(p) for p in want["profiles"]], (tag, res.profile_len.tolist(), [len(p) for p in want["profiles"]])
    for k, p in enumerate(want["profiles"]):
        got = res.profile(k)
        assert bits(got) == bits(p), (tag, "profile", k, np.argwhere(got != p)[:5], got[got != p][:5], p[got != p][:5])
        rest = res.profile_prob[res.profile_off[k] + len(p):(res.profile_off[k + 1] if k + 1 < len(want["profiles"]) else len(res.profile_prob))]
        assert not np.any(rest), (tag, "behind profile", k)


def per_window(res):
    """Every output of a call cut into its windows: [(status, {array: bytes}, [profile lists])]."""
    out = []
    for w in range(len(res.window_status)):
        a, b = int(res.pos_off[w]), int(res.pos_off[w + 1])
        arrays = {k: bits(getattr(res, k)[a:b]) for k in PER_SAMPLE + PER_POSITION}
        profiles = [bits(res.profile(k)) for k in range(len(res.profile_len)) if res.profile_window[k] == w]
        out.append((int(res.window_status[w]), arrays, profiles))
    return out


@pytest.mark.parametrize("name", [c[0] for c in K.seeded()])
def test_seeded_windows(eng, name):
    _, windows, o = case(name)
    same(run(eng, windows, o), K.restated(name)[0], name)


def test_one_read_windows_for_each_quirk(eng):
    """One call per window, then all of them in one call."""
    cases = K.quirks()
    singles = []
    for name, windows, o in cases:
        res = run(eng, windows, o)
        same(res, K.restated(name)[0], name)
        singles += per_window(res)
    assert per_window(run(eng, [w for _, ws, _ in cases for w in ws], cases[0][2])) == singles


def test_edge_windows(eng):
    for name, windows, o in K.edges():
        same(run(eng, windows, o), K.restated(name)[0], name)


def test_windows_the_reference_panics_on(eng):
    """N in a CIGAR, CIGARs longer than their reads: a negative status, no outputs, the neighbours as they are alone."""
    name, windows, o = K.panics()[0]
    res = run(eng, windows, o, fill=0xA5)
    same(res, K.restated(name)[0], name)
    assert res.window_status.tolist() == [0, _lib.PHMM_ACT_STATUS_REF_SKIP, _lib.PHMM_ACT_STATUS_CIGAR_OVERRUN, 0, _lib.PHMM_ACT_STATUS_CIGAR_OVERRUN]
    cut = per_window(res)
    for w in (1, 2, 4):
        assert not any(any(v) for v in cut[w][1].values()) and cut[w][2] == [b""]
    for w in (0, 3):
        assert per_window(run(eng, [windows[w]], o))[0] == cut[w]


def test_one_larger_batch(eng):
    """20 000 positions under about 1 500 reads in one window beside 63 small ones; the call over all windows equals the
    windows one by one; two runs are bit-identical."""
    name, windows, o = K.large()[0]
    res = run(eng, windows, o, fill=0x5A)
    same(res, K.restated(name)[0], name)
    cut = per_window(res)
    assert per_window(run(eng, windows, o)) == cut
    for w, window in enumerate(windows):
        assert per_window(run(eng, [window], o))[0] == cut[w], w


def test_batches_of_several_samples_equal_their_windows_and_repeat(eng):
    seeds = [(n, case(n)) for n in ("seeded s3 p2 c128", "seeded s3 p4 c0")]
    for name, (_, windows, o) in seeds:
        more = windows + [K.seeded_window(300 + i, 3, start=50 * i, length=37 + i, contig=4000, max_reads=9, max_bases=60) for i in range(5)]
        res = run(eng, more, o)
        cut = per_window(res)
        assert per_window(run(eng, more, o, fill=0xFF)) == cut
        assert cut[0] == per_window(run(eng, windows, o))[0]
        for w in (1, 5):
            assert per_window(run(eng, [more[w]], o))[0] == cut[w]


def test_null_outputs_leave_the_rest_unchanged(eng):
    name, windows, o = case("seeded s2 p2 c0")
    full = run(eng, windows, o)
    for omit in GROUPS + (("gl",), ("pl", "qual"), ("is_active_prob", "filter_size"), PER_SAMPLE + PER_POSITION, PER_SAMPLE + PER_POSITION + GROUPS[2]):
        res = run(eng, windows, o, omit=omit, fill=0x77)
        for k in activity.OUTPUTS + ("window_status",):
            if k in omit:
                assert getattr(res, k) is None
            elif k == "filter_size":
                assert res.filter_size == full.filter_size
            else:
                assert bits(getattr(res, k)) == bits(getattr(full, k)), (omit, k)


def test_invalid_arguments_write_nothing_and_name_the_offender(eng):
    name, windows, o = case("seeded s2 p1 c128")
    extra = K.seeded_window(55, 2, start=5000, length=40, max_reads=5, max_bases=40)
    good = activity.pack(windows + [extra])

    def refused(arrays, needle, **change):
        opts = dict(o)
        opts.update(change)
        with pytest.raises(PhmmError) as e:
            activity.activity_profile(eng, arrays, fill=0xA5, **opts)
        assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and "phmm_activity_profile" in str(e.value) and needle in str(e.value), str(e.value)
        for k, v in e.value.outputs.items():
            assert np.all(np.frombuffer(v.tobytes(), np.uint8) == 0xA5), k

    def changed(**kw):
        a = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, f in kw.items():
            a[k] = f(a[k]) if callable(f) else f
        return a

    refused(good, "ploidy 0", ploidy=0)
    refused(good, "ploidy 65", ploidy=65)
    first_group = int(np.argmax(np.diff(good["group_read_off"].astype(np.int64)) >= 2))
    r = int(good["group_read_off"][first_group])

    def unsorted(p):
        p[r + 1] = p[r] - 1
        return p
    refused(changed(read_pos=unsorted), "read %d (window %d, sample %d)" % (r + 1, first_group // 2, first_group % 2))

    def short_ref(off):
        off[2:] -= 1
        return off
    refused(changed(window_ref_off=short_ref, ref_bases=lambda b: b[:-1]), "window 1: 39 reference bases, the window needs 40")

    def swap(off):
        off[1], off[2] = off[2], off[1]
        return off
    refused(changed(group_read_off=swap), "window 0: sample 1: group_read_off not monotonic")

    def cigar_back(off):
        off[3] = off[2] - 1
        return off
    refused(changed(read_cigar_off=cigar_back), "read 2: read_cigar_off not monotonic")

    def bases_back(off):
        off[5] = off[4] - 1
        return off
    refused(changed(read_off=bases_back), "read 4: read_off not monotonic")
    refused(changed(window_contig_length=lambda c: np.where(np.arange(len(c)) == 1, 5039, c).astype(np.uint64)), "window 1: the window ends past the contig")
    refused(good, "sigma", sigma=-1.0)
    for k in ("window_start", "window_len", "window_contig_length", "window_ref_off", "ref_bases", "group_read_off", "read_pos",
              "read_cigar_off", "read_cigar", "read_off", "read_bases", "read_quals"):
        refused(changed(**{k: None}), "null array")
    with pytest.raises(PhmmError) as e:
        activity.activity_profile(eng, good, omit=("window_status",), **o)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and "null array" in str(e.value)
    same(run(eng, windows, o), K.restated(name)[0], "after the refusals")


def test_the_staging_buffer_grows(eng):
    """A fresh engine: a small call (the buffer's first allocation), the large batch (it has to grow, and so has the device
    workspace), the small call again -- bit for bit the same, with the same number of staged bytes."""
    name, windows, o = case("seeded s1 p4 c128")
    _, big, bo = K.large()[0]
    e = HipPairHMMEngine(0)
    try:
        s0 = e.stat("staged_bytes")
        first = run(e, windows, o)
        s1 = e.stat("staged_bytes")
        many = run(e, big, bo)
        s2 = e.stat("staged_bytes")
        third = run(e, windows, o)
        s3 = e.stat("staged_bytes")
    finally:
        e.close()
    assert s1 - s0 == s3 - s2 > 0 and s2 - s1 > s1 - s0
    # the large call's wanted outputs alone are more than the 1 MiB a staging buffer starts with
    assert sum(getattr(many, k).nbytes for k in PER_SAMPLE + PER_POSITION + GROUPS[2]) > (1 << 20)
    assert per_window(first) == per_window(third) == per_window(run(eng, windows, o))
    same(first, K.restated(name)[0], name)
    same(many, K.restated("large")[0], "large, after growing")
