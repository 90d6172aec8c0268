"""The case set of tests/test_assembly_regions_hip.py, as input arrays of phmm_assembly_regions with their parameters.  It is
built without a device, so that tests/test_assembly_regions_oracle.py can take its census: every branch, status and flag of
the restatement must be reached by some case here."""
import numpy as np

NAN, INF = float("nan"), float("inf")
THRESHOLD = 0.002
M, I, D, N, S, H, P, EQ, X = range(9)
DEFAULTS = dict(extension=0, min_region_size=1, max_region_size=300, max_prob_propagation=50, threshold=THRESHOLD, max_input_depth=200000)


def profile(probs, start=0, stop=None, contig=1 << 30, window=0):
    """A profile: its states, the position of state 0, of the last ADDED state (by default the last state), the contig's length."""
    probs = list(probs)
    if stop is None:
        stop = start + len(probs) - 1 if probs else start  # (an empty list has no stop: the value is never read)
    return dict(probs=probs, start=start, stop=stop, contig=contig, window=window)


def read(pos, cigar, quals=None):
    """A read: cigar as (op, length) pairs; quals default to one 30 per read base."""
    n = sum(l for op, l in cigar if op in (M, I, S, EQ, X))
    return (pos, [(l << 4) | op for op, l in cigar], [30] * n if quals is None else list(quals))


def make(profiles, groups=None, n_samples=1, n_windows=None, gap=3, **params):
    """The arrays of one call.  groups: per (window, sample) group, window-major, its reads; None leaves the read arrays out.
    Between the lists lie `gap` values no list owns (9.0: active, were they read)."""
    prob, first = [], []
    for p in profiles:
        prob += [9.0] * gap
        first.append(len(prob))
        prob += p["probs"]
    prob += [9.0] * gap
    a = dict(profile_prob=np.array(prob, np.float32), profile_first=np.array(first, np.uint32),
             profile_len=np.array([len(p["probs"]) for p in profiles], np.uint32),
             profile_start=np.array([p["start"] for p in profiles], np.uint64), profile_stop=np.array([p["stop"] for p in profiles], np.uint64),
             profile_contig_length=np.array([p["contig"] for p in profiles], np.uint64),
             profile_window=np.array([p["window"] for p in profiles], np.uint32), n_samples=n_samples,
             n_windows=n_windows if n_windows is not None else (max([p["window"] for p in profiles] + [0]) + 1))
    if groups is not None:
        assert len(groups) == a["n_windows"] * n_samples
        reads = [r for g in groups for r in g]
        off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)  # noqa: E731
        cat = lambda parts, dt: np.array([x for part in parts for x in part], dt)  # noqa: E731
        a.update(group_read_off=off([len(g) for g in groups]), read_pos=np.array([r[0] for r in reads], np.int64),
                 read_cigar_off=off([len(r[1]) for r in reads]), read_cigar=cat([r[1] for r in reads], np.uint32),
                 read_off=off([len(r[2]) for r in reads]), read_quals=cat([r[2] for r in reads], np.uint8))
    return a, dict(DEFAULTS, **params)


def runs(*parts):
    """[(value, count), ...] one behind the other."""
    return [v for v, n in parts for _ in range(n)]


def random_probs(rng, n):
    """Runs of active and inactive states of random lengths, with random values, so that boundaries and minima fall anywhere."""
    out = []
    while len(out) < n:
        active = rng.random() < 0.6
        k = int(rng.integers(1, 90))
        out += [float(np.float32(rng.uniform(0.01, 1.0))) if active else float(np.float32(rng.uniform(0.0, 0.002))) for _ in range(k)]
    return out[:n]


def region_cases():
    """name -> (arrays, parameters), profiles only."""
    c = {}
    rng = np.random.default_rng(20261020)
    # every list length against every maximum: the words a list takes, the words a search runs over
    for n in (0, 1, 63, 64, 65, 129):
        for mx in (1, 63, 64, 65, 300):
            c["len%d_max%d" % (n, mx)] = make([profile(random_probs(rng, n), start=7)], max_region_size=mx, max_prob_propagation=0, min_region_size=1)
    c["long_random"] = make([profile(random_probs(rng, 5000), start=1000)], max_region_size=300, min_region_size=50, extension=100)
    # the boundary at bit 63, at bit 0 of the second word, and past the 64 words one pass of the search takes
    c["boundary_bit63"] = make([profile(runs((1.0, 63), (0.0, 66)))], max_region_size=100, max_prob_propagation=0)
    c["boundary_bit64"] = make([profile(runs((1.0, 64), (0.0, 65)))], max_region_size=100, max_prob_propagation=0)
    c["boundary_inactive_bit63"] = make([profile(runs((0.0, 63), (1.0, 66)))], max_region_size=100, max_prob_propagation=0)
    c["boundary_word70"] = make([profile(runs((0.0, 70 * 64 + 5), (1.0, 700)))], max_region_size=5000, max_prob_propagation=0)
    # a run that ends exactly at the maximum
    c["run_is_max_active"] = make([profile(runs((1.0, 64), (0.0, 64)))], max_region_size=64, max_prob_propagation=10)
    c["run_is_max_inactive"] = make([profile(runs((0.0, 64), (1.0, 64)))], max_region_size=64, max_prob_propagation=10)
    # one state short of max + propagation: nothing; one more: regions
    c["one_short"] = make([profile(runs((1.0, 20), (0.0, 39)))], max_region_size=40, max_prob_propagation=20)
    c["just_enough"] = make([profile(runs((1.0, 20), (0.0, 40)))], max_region_size=40, max_prob_propagation=20)
    c["one_longer"] = make([profile(runs((1.0, 20), (0.0, 41)))], max_region_size=40, max_prob_propagation=20)
    # the band-passed list runs past the last added state: the third region starts at stop + 1, so the fourth is unforced and the
    # tail stays; with the stop one further every state is popped
    c["start_is_stop_plus_1"] = make([profile(runs((0.0, 20)), start=100, stop=109)], max_region_size=5, max_prob_propagation=5)
    c["start_is_not_stop_plus_1"] = make([profile(runs((0.0, 20)), start=100, stop=110)], max_region_size=5, max_prob_propagation=5)
    # the cut site
    base = [1.0] * 40 + [0.0] * 60
    def cut(name, edits, mn=5, mx=30, probs=None, **kw):  # noqa: E306
        p = list(base if probs is None else probs)
        for i, v in edits.items():
            p[i] = v
        c["cut_" + name] = make([profile(p)], min_region_size=mn, max_region_size=mx, max_prob_propagation=10, **kw)
    cut("flat", {})
    cut("one_minimum", {12: 0.5})
    cut("lowest_wins", {12: 0.5, 20: 0.25, 25: 0.75})
    cut("tie_higher_index", {12: 0.5, 20: 0.5})
    cut("tie_three", {8: 0.25, 12: 0.25, 28: 0.25})
    cut("tie_zero_signs", {12: -0.0, 20: 0.0}, threshold=-1.0)
    cut("plateau", {12: 0.5, 13: 0.5, 14: 0.5})             # only the first of a plateau is < its left neighbour
    cut("minimum_at_min_size", {5: 0.5})
    cut("minimum_below_min_size", {4: 0.5})
    cut("minimum_at_end_minus_1", {29: 0.5})
    cut("minimum_at_end", {30: 0.5})
    cut("nan_behind_end", {29: 0.5, 30: NAN})               # p[29] <= NaN is false: no minimum
    cut("lane_stride", {}, mn=1, mx=200, probs=[1.0 - 0.001 * (i % 7 == 3) for i in range(260)])   # equal minima 64 apart and more
    cut("nan", {12: NAN, 20: 0.5}, threshold=-1.0)
    cut("nan_neighbour", {11: NAN, 12: 0.5, 20: 0.75, 21: NAN}, threshold=-1.0)
    cut("minus_inf", {12: -INF, 20: 0.5}, threshold=-INF)
    cut("plus_inf", {11: INF, 12: INF, 13: INF, 20: 0.5})
    cut("f32_max_never_wins", {11: INF, 12: 3.4028234663852886e38, 13: INF})   # a minimum, but not < f32::MAX
    cut("nan_boundary", {7: NAN})                          # a NaN is inactive: the boundary
    cut("min_above_max_reached", {}, mn=31, mx=30)
    cut("min_above_max_not_reached", {10: 0.0}, mn=31, mx=30)
    cut("min_above_max_inactive", {}, mn=31, mx=30, probs=[0.0] * 100)
    cut("min_is_max", {12: 0.5}, mn=30, mx=30)
    # after a drain: the state at the remaining list's index 0 is a minimum of the whole list; the one at index 1 compares with it
    cut("after_drain", {}, mn=1, mx=10, probs=runs((0.0, 7), (1.0, 1), (0.25, 1), (0.5, 1), (1.0, 30), (0.0, 40)))
    cut("after_drain_index1", {}, mn=1, mx=10, probs=runs((0.0, 7), (0.5, 1), (0.25, 1), (1.0, 31), (0.0, 40)))
    # the last state of the whole list is no minimum, whatever its value
    cut("last_state", {}, mn=1, mx=20, probs=runs((0.0, 30), (1.0, 19), (0.5, 1)))
    # the contig's end: the list keeps the state AT the contig length
    c["clipped"] = make([profile(runs((0.0, 11)), start=10, stop=19, contig=20)], max_region_size=4, max_prob_propagation=0)
    c["start_past_contig"] = make([profile(runs((0.0, 8)), start=10, contig=20), profile(runs((0.0, 10), (1.0, 1)), start=10, stop=19, contig=20),
                                   profile(runs((1.0, 8)), start=10, contig=20)], max_region_size=4, max_prob_propagation=0)
    c["contig_of_1"] = make([profile(runs((1.0, 2)), start=0, stop=0, contig=1)], max_region_size=1, max_prob_propagation=0)
    # padding
    c["padding_saturates"] = make([profile(runs((0.0, 30)), start=5)], max_region_size=10, max_prob_propagation=0, extension=7)
    c["padding_is_start"] = make([profile(runs((0.0, 30)), start=7)], max_region_size=10, max_prob_propagation=0, extension=7)
    c["padding_clipped"] = make([profile(runs((1.0, 30)), start=70, contig=100)], max_region_size=10, max_prob_propagation=0, extension=7)
    c["density"] = make([profile([0.05, 0.050000004, 0.06, 0.0, 1.0, 0.04, 0.3] * 20)], max_region_size=13, max_prob_propagation=0, threshold=0.045)
    # many profiles in one call, empty ones between them
    for n in (2, 64, 65):
        ps = [profile(random_probs(rng, int(rng.integers(0, 200))) if k % 7 != 3 else [], start=int(rng.integers(0, 1000)), contig=1100) for k in range(n)]
        c["profiles_%d" % n] = make(ps, max_region_size=int(rng.integers(5, 80)), max_prob_propagation=3, min_region_size=4, extension=11)
    return c


def read_cases():
    """name -> (arrays, parameters), with reads."""
    c = {}
    rng = np.random.default_rng(7)
    flat = lambda n, start=1000: profile(runs((1.0, n)), start=start, contig=5000)  # noqa: E731
    par = dict(max_region_size=50, max_prob_propagation=0, extension=10)
    for n in (0, 1, 63, 64, 65, 130):   # reads in the group: the passes of the running maximum, of the count and of the write
        pos = sorted(int(x) for x in rng.integers(900, 1250, n))
        c["group_of_%d" % n] = make([flat(200)], [[read(p, [(M, int(rng.integers(1, 60)))]) for p in pos]], **par)
    # a long read early in the group overlaps the last region; short ones between it and that region do not
    c["long_read_early"] = make([flat(200)], [[read(905, [(M, 10)]), read(910, [(M, 20), (N, 250), (M, 20)])] + [read(920 + i, [(M, 5)]) for i in range(70)]], **par)
    # the edges of the fetch around the first region [1000, 1049], padded [990, 1059]
    c["fetch_edges"] = make([flat(50)], [[read(980, [(M, 10)]), read(980, [(M, 11)]), read(985, [(S, 5), (M, 5), (I, 3), (D, 1), (S, 2)], [1, 2, 3, 4, 5] * 3),
                                          read(989, [(I, 4)]), read(990, [(S, 4)]), read(990, [(EQ, 1), (X, 1)]), read(1059, [(M, 1)]),
                                          read(1059, [(I, 2)]), read(1060, [(M, 1)])]], **par)
    c["no_qualities"] = make([flat(50)], [[read(1000, [(M, 10)], []), read(1001, [(D, 3)], []), read(1002, [(M, 4)], [255] * 4)]], **par)
    c["three_samples_one_empty"] = make([flat(120)], [[read(p, [(M, 30)]) for p in (950, 1000, 1100)], [], [read(p, [(M, 70), (H, 3)]) for p in (1040, 1041)]],
                                        n_samples=3, **par)
    # the over-depth flag: reads over all samples, at the cap and one above
    c["depth_at_cap"] = make([flat(50)], [[read(1000, [(M, 10)])] * 3, [read(1010, [(M, 10)])] * 2], n_samples=2, max_input_depth=5, **par)
    c["depth_above_cap"] = make([flat(50)], [[read(1000, [(M, 10)])] * 3, [read(1010, [(M, 10)])] * 3], n_samples=2, max_input_depth=5, **par)
    # profiles of two windows, each with its own groups; a window no profile names; a profile without regions
    ps = [profile(runs((1.0, 60), (0.0, 60)), start=1000, contig=5000, window=2), profile(runs((0.0, 30)), start=2000, contig=5000, window=0),
          profile(runs((0.0, 100)), start=1060, contig=5000, window=2)]
    groups = [[read(int(p), [(M, 40)]) for p in sorted(rng.integers(1900, 2100, 80))], [],
              [read(1, [(M, 5)])], [read(2, [(M, 5)])],
              [read(int(p), [(M, 25), (D, 10), (M, 25)]) for p in sorted(rng.integers(900, 1200, 150))], [read(int(p), [(M, 3)]) for p in sorted(rng.integers(900, 1200, 70))]]
    c["two_windows"] = make(ps, groups, n_samples=2, n_windows=3, max_region_size=40, max_prob_propagation=0, extension=15)
    c["reads_without_regions"] = make([profile(runs((1.0, 10)), start=1000, contig=5000)], [[read(1000, [(M, 10)], [10, 20] * 5)]], **par)
    return c


def all_cases():
    c = dict(region_cases())
    c.update(read_cases())
    return c


# what the census demands of the case set: the branches of tests/assembly_regions_restatement.py, every status, every flag
CENSUS = {"pop:empty", "pop:drained", "end:wait", "boundary:found", "cut:minimum", "cut:none", "is_minimum:last", "region:clipped",
          "force:forced", "force:start_is_stop_plus_1", "pad:saturated", "pad:clipped", "depth:over", "status:0", "status:-1", "status:-2",
          "flag:none", "flag:active", "flag:forced", "flag:over_depth"}
