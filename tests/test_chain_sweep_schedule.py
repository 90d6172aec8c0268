"""The chained f64 sweep's step around the cell (chain_body of phmm_chain_kernels.hip): where a read's result is emitted, and
how the sweep addresses the ring.

Emission: the lane that owns a haplotype's last column emits when the read's SUM row passes it, so the step of an emit depends
on the SUM row's ring position and on that lane.  Chains made only of reads of 1, 2 and 3 bases put SUM rows every 3 ... 5
rows (emits on consecutive steps, on either half of a pair of steps); haplotypes of 1, K, K + 1 and 16 K bases (and 2, 10,
11 for 32 lanes per pair) put the emitting lane at lane 0, at the first and at the last column of a lane and at the last
lane; read lengths put SUM rows on the ring positions around a producer tick (64 / S rows) and around the ring wrap
(256 / S rows) of every stream, with 1, 2 and 4 streams; and regions of 3 and 5 reads leave streams without a read.

Addressing: a read longer than the ring, chains whose rows (reads + SUM + RESET) add up to 0, 1, 2, 3 mod 4, and more than 70
work items, so that blocks with different first-tick phases run.

Rotating the reads of a region moves every row to another tick, ring slot and step and must not change a bit of any result.

The builders are plain numpy; test_the_oracle_handles_every_input runs without a GPU."""
import numpy as np
import pytest

from lorikeet_amd.batch import Read, RegionBatch
from oracle import oracle
from test_chain_producer_edges import _haps, _quals, _read_from, rotated, unrotate
from test_hip_parity import _close                   # TOL_VS_ORACLE = 1e-9

ALPHA = np.frombuffer(b"ACGT", np.uint8)
H_MAX = 304                                          # every region's longest haplotype: K = 19 at 16 lanes, 10 at 32
CASES = ((16, 1), (16, 2), (16, 4), (32, 1))         # lanes per pair, streams
RUN = 12                                             # reads per chain: no region has more
RING = 256


def _hap_of(rng, root, n):
    return root[:n].copy() if n > 3 else ALPHA[rng.integers(0, 4, n)]


def sum_positions(lens, streams, lead=15):
    """Ring positions (before the wrap) of the SUM rows of every stream of a chain: the reads are dealt to the streams in
    runs of ceil(n / S), a stream starts with `lead` neutral rows, and a read of R rows is followed by SUM and RESET."""
    n_sub = -(-len(lens) // streams)
    out = []
    for s in range(streams):
        at, mine = lead, []
        for r in lens[s * n_sub:(s + 1) * n_sub]:
            mine.append(at + r)
            at += r + 2
        out.append(mine)
    return out


def boundary_lengths(streams):
    """Per pair (a, b) of a position around a tick boundary and one around the ring wrap of a stream: two read lengths that
    put the first read's SUM row on a and the second one's on b (16 lanes per pair: 15 neutral rows in front)."""
    tick, ring = 64 // streams, RING // streams
    m = 1 if tick - 1 - 15 >= 1 else 2                       # the first tick boundary a read of at least one base can reach
    return [(a - 15, b - a - 2) for a, b in zip((m * tick - 1, m * tick, m * tick + 1), (ring - 1, ring, ring + 1))]


def make_regions():
    """-> regions, and per region what it is for."""
    rng = np.random.default_rng(5100)
    regions, what = [], []
    root = ALPHA[rng.integers(0, 4, H_MAX)]

    def long_haps(n):
        haps = _haps(rng, n, H_MAX, H_MAX)
        assert max(len(h) for h in haps) == H_MAX
        return haps

    # emits on consecutive steps, the emitting lane at every kind of place
    for hap_lens in ((1, 19, 20, H_MAX), (10, 11, 2, H_MAX)):
        for n_reads in (12, 11, 5, 3):
            haps = [_hap_of(rng, root, n) for n in hap_lens]
            lens = [1 + (i + n_reads) % 3 for i in range(n_reads)]
            regions.append(([_read_from(rng, haps[-1], n) for n in lens], haps))
            what.append("short reads %s x haplotypes %s" % (lens, list(hap_lens)))
    # SUM rows around a tick boundary and around the ring wrap of every stream, for 1, 2 and 4 streams
    for streams in (1, 2, 4):
        for r0, r1 in boundary_lengths(streams):
            haps = long_haps(3)
            lens = [r0, r1, 3] * streams                       # every stream gets the same three reads
            regions.append(([_read_from(rng, haps[i % 3], n) for i, n in enumerate(lens)], haps))
            what.append("boundaries of %d streams: reads %s" % (streams, lens))
    # a read longer than the ring; rows of the chain = 0, 1, 2, 3 mod 4
    for extra in range(4):
        haps = long_haps(2)
        lens = [300, 7, 5 + extra]                             # rows: 302 + 9 + 7 + extra
        regions.append(([_read_from(rng, haps[i % 2], n) for i, n in enumerate(lens)], haps))
        what.append("long read, %d rows" % (sum(lens) + 2 * len(lens)))
    # many small work items: blocks with every first-tick phase
    for i in range(72):
        haps = long_haps(2)
        lens = [int(n) for n in rng.integers(1, 21, 2 + i % 2)]
        regions.append(([_read_from(rng, haps[j % 2], n) for j, n in enumerate(lens)], haps))
        what.append("small item %d" % i)
    return regions, what


_cache = {}


def _inputs():
    if not _cache:
        regions, what = make_regions()
        b = RegionBatch.from_regions(regions)
        _cache.update(regions=regions, what=what, batch=b, want=oracle.compute_batch(b.as_dict(), n_threads=16))
    return _cache["regions"], _cache["what"], _cache["batch"], _cache["want"]


def test_the_oracle_handles_every_input():
    """No GPU: the batch is well-formed, the oracle gives a finite non-positive number for every pair, and the builders put
    the SUM rows where the module's docstring says."""
    regions, what, b, want = _inputs()
    assert want.shape == (b.n_out,) and np.all(np.isfinite(want)) and np.all(want <= 0.0)
    assert all(max(len(h) for h in haps) == H_MAX and len(reads) <= RUN for reads, haps in regions)
    assert len(regions) >= 70
    # SUM rows on 63, 64, 65 and 255, 256, 257 with one stream; on the matching positions of 2 and 4 streams, in every stream
    for streams, near_tick, near_wrap in ((1, {63, 64, 65}, {255, 256, 257}), (2, {31, 32, 33}, {127, 128, 129}),
                                          (4, {31, 32, 33}, {63, 64, 65})):
        mine = [r for r, w in enumerate(what) if w.startswith("boundaries of %d streams" % streams)]
        per_stream = [set() for _ in range(streams)]
        for r in mine:
            for s, pos in enumerate(sum_positions([len(rd) for rd in regions[r][0]], streams)):
                per_stream[s] |= set(pos)
        assert all(near_tick | near_wrap <= got for got in per_stream), (streams, per_stream)
    assert boundary_lengths(4)[0][0] + 15 == 31          # 15, 16, 17 would need a read without a base: the next tick instead
    # emits on consecutive steps: SUM rows 3, 4 and 5 rows apart, on even and on odd positions
    pos = sum_positions([len(rd) for rd in regions[0][0]], 1)[0]
    assert set(np.diff(pos)) == {3, 4, 5} and {p % 2 for p in pos} == {0, 1}
    # a stream without a read beside streams that have one: 3 and 5 reads over 4 streams
    assert [len(p) for p in sum_positions([1, 2, 3], 4)] == [1, 1, 1, 0]
    assert [len(p) for p in sum_positions([1, 2, 3, 1, 2], 4)] == [2, 2, 1, 0]
    assert {(sum(len(rd) for rd in regions[r][0]) + 2 * len(regions[r][0])) % 4
            for r, w in enumerate(what) if w.startswith("long read")} == {0, 1, 2, 3}
    assert np.array_equal(unrotate(oracle.compute_batch(RegionBatch.from_regions(rotated(regions, 5)).as_dict(), n_threads=16),
                                   regions, 5), want)


@pytest.fixture(scope="module")
def engine():
    from lorikeet_amd import HipPairHMMEngine
    e = HipPairHMMEngine(0)
    yield e
    e.close()


def _planned(eng, b):
    plan = eng.plan(b)
    name = plan.dominant_kernel
    plan.close()
    return name


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,streams", CASES)
def test_sweep_schedule(engine, lanes, streams):
    regions, what, b, want = _inputs()
    with engine.switches(force_L=lanes, force_chain=RUN, force_streams=streams):
        name = _planned(engine, b)
        assert name.startswith("phmm_forward_chain_k<%d,%d>" % (lanes, -(-H_MAX // lanes))), name
        assert streams == 1 or name.endswith("x%d streams" % streams), name
        got = engine.compute(b)
        for r, w in enumerate(what):   # region by region, so that a failure names its case
            lo, hi = int(b.out_off[r]), int(b.out_off[r + 1])
            try:
                _close(got[lo:hi], want[lo:hi])
            except AssertionError as e:
                raise AssertionError(w) from e
        for k in range(1, RUN):        # every cyclic rotation of every region (regions of fewer reads see some twice)
            rot = engine.compute(RegionBatch.from_regions(rotated(regions, k)))
            assert np.array_equal(unrotate(rot, regions, k), got), "rotation by %d" % k
