"""The chained kernels' prologue scan and row producer at their edges (phmm_chain_kernels.hip, phmm_chain32_kernels.hip).

Scan (chain_blocks_prescale, phmm_device.hpp): 16-byte loads with a byte-wise head and tail decide whether a chain of reads
holds a zero byte in gcp or base_q -- every alignment of the chain's first byte, chain lengths around one and two wave passes
of 64 x 16 bytes, one zero byte at each place where head, body and tail meet, in either array; and a zero byte just outside
the chain must not be seen.

Producer (issue / finish of chain_body): every lane loads clamped bytes and finish() selects by the row kind -- read lengths
that put row 0, the last row, the SUM row and the RESET row on the first and on the last producer lane of a tick (64, 32 and
16 rows per tick with 1, 2 and 4 streams), reads longer than the ring, a different first gcp in every read (the RESET row
looks it up), streams with fewer reads or none, a read 'N' and a base quality of 255.  Rotating the reads of a region moves
every row to another producer lane and tick and must not change a single bit of any pair's result.

The builders are plain numpy; test_the_oracle_handles_every_input runs without a GPU."""
import re

import numpy as np
import pytest

from lorikeet_amd.batch import Read, RegionBatch
from oracle import oracle
from test_f32_first import TOL_F32                   # 1e-5
from test_hip_parity import _close                   # TOL_VS_ORACLE = 1e-9

ALPHA = np.frombuffer(b"ACGT", np.uint8)
RUN = 5                                              # reads per chain of the scan cases
SCAN_BYTES = (1, 15, 16, 17, 1023, 1024, 1025, 2049)  # one wave pass of the scan is 64 lanes x 16 bytes
SHIFTS = tuple(range(1, 17))                         # bases of the one-read region in front: first byte offset mod 16 = 1 ... 15, 0
PRODUCER_LENGTHS = (1, 2, 14, 15, 30, 31, 61, 62, 63, 126, 127, 254, 255, 256, 257, 300)
PRODUCER_CASES = ((16, 1), (16, 2), (16, 4), (32, 1))  # lanes per pair, streams


def _quals(rng, n, lo, hi):
    return rng.integers(lo, hi + 1, n).astype(np.uint8)


def _read_from(rng, hap, n):
    """n bases copied from the haplotype (wrapping round), one base in sixteen replaced: likelihoods stay far from underflow."""
    s = int(rng.integers(0, len(hap)))
    bases = np.resize(np.roll(hap, -s), n).copy()
    flip = rng.random(n) < 1.0 / 16
    bases[flip] = ALPHA[rng.integers(0, 4, int(flip.sum()))]
    return Read(bases, _quals(rng, n, 10, 40), _quals(rng, n, 20, 45), _quals(rng, n, 20, 45), _quals(rng, n, 5, 30))


def _haps(rng, n, lo, hi):
    root = ALPHA[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))]
    out = [root]
    for _ in range(n - 1):
        h = root.copy()
        at = rng.integers(0, len(h), 3)
        h[at] = ALPHA[rng.integers(0, 4, 3)]
        out.append(h[:len(h) - int(rng.integers(0, 4))])
    return out


# ---- scan -------------------------------------------------------------------------------------------------------------------
def _split(rng, total, parts):
    """`parts` read lengths >= 1 that add up to `total`: nearly equal (the longest read stays near the longest haplotype a
    16-lane kernel takes, 400 bases), a few bases moved from one read to the next."""
    lens = np.full(parts, total // parts, int)
    lens[:total % parts] += 1
    for i in range(parts - 1):
        d = int(rng.integers(0, max(1, min(4, lens[i]))))
        lens[i] -= d
        lens[i + 1] += d
    return lens


def zero_positions(offset, total):
    """Where one zero byte goes in a chain of `total` bytes whose first byte is at `offset` in its (256-byte aligned) array:
    first and last byte, the bytes before and after the first 16-byte boundary, the last byte of the head, the first of the tail
    and the last of the body."""
    head = min(-offset % 16, total)
    body_end = head + (total - head) // 16 * 16
    boundary = head if head > 0 else 16
    want = {0, total - 1, boundary - 1, boundary, head - 1, body_end, body_end - 1}
    return sorted(p for p in want if 0 <= p < total)


def make_scan_batch(shift):
    """A one-read region of `shift` bases, then for every chain length: a region of five reads (fewer where the chain has fewer
    bytes: a read has at least one base) without a zero byte, and one region per zero position and array.  -> batch, and per
    region (bytes, first byte offset, zero position or None, array or None)."""
    rng = np.random.default_rng(4100 + shift)
    haps = _haps(rng, 2, 40, 70)
    regions, what, offset = [([_read_from(rng, haps[0], shift)], haps)], [(shift, 0, None, None)], shift
    for total in SCAN_BYTES:
        lens = _split(rng, total, min(RUN, total))
        for pos in [None] + zero_positions(offset, total):
            for array in ((None,) if pos is None else ("gcp", "quals")):
                haps = _haps(rng, 2, *((40, 70) if total < 400 else (380, 400)))   # as long as the reads, or they underflow
                reads = [_read_from(rng, haps[i % 2], int(n)) for i, n in enumerate(lens)]
                if pos is not None:
                    r = int(np.searchsorted(np.cumsum(lens), pos, side="right"))
                    getattr(reads[r], array)[pos - int(np.sum(lens[:r]))] = 0
                regions.append((reads, haps))
                what.append((total, offset, pos, array))
                offset += total
    return RegionBatch.from_regions(regions), what


def make_neighbour_batches():
    """Three regions A, M, B.  Variants: no zero anywhere; A's last byte zero; B's first byte zero (each in gcp and in base_q).
    M is the same reads at the same offset in all of them.  M's bytes: 3 + 16 x 70 + 5, so head, body and tail all exist."""
    out = {}
    for name, (which, at, array) in {"clean": (None, 0, None), "A-last-gcp": (0, -1, "gcp"), "A-last-q": (0, -1, "quals"),
                                     "B-first-gcp": (2, 0, "gcp"), "B-first-q": (2, 0, "quals")}.items():
        regions = _neighbour_regions()
        if which is not None:
            reads = regions[which][0]
            getattr(reads[at], array)[at] = 0          # A: last byte of its last read; B: first byte of its first read
        out[name] = RegionBatch.from_regions(regions)
    out["alone"] = RegionBatch.from_regions(_neighbour_regions()[1:2])
    return out


def _neighbour_regions():
    rng = np.random.default_rng(4200)
    regions = []
    for lens in ((7, 3, 3), (300, 400, 200, 228), (9, 20)):   # A: 13 bytes, so M starts 3 bytes before a 16-byte boundary
        haps = _haps(rng, 2, *((40, 70) if max(lens) < 100 else (380, 400)))
        regions.append(([_read_from(rng, haps[i % 2], n) for i, n in enumerate(lens)], haps))
    return regions


# ---- producer ---------------------------------------------------------------------------------------------------------------
def make_producer_regions():
    """Seven regions of 6 ... 12 reads (with 4 streams: 2,2,2,0 / 2,2,2,1 / ... / 3,3,3,3 reads per stream), 2 or 3 related
    haplotypes of 310 ... 400 bases, read lengths drawn from PRODUCER_LENGTHS with every length used at least once."""
    rng = np.random.default_rng(4300)
    pool = list(rng.permutation(PRODUCER_LENGTHS)) + list(rng.choice(PRODUCER_LENGTHS, 63 - len(PRODUCER_LENGTHS)))
    regions = []
    for n in range(6, 13):
        haps = _haps(rng, 2 + n % 2, 310, 400)
        reads = [_read_from(rng, haps[i % len(haps)], int(pool.pop())) for i in range(n)]
        for i, rd in enumerate(reads):
            rd.gcp[0] = 3 + 2 * i                      # a different first gcp in every read of the region
        regions.append((reads, haps))
    regions[1][0][2].bases[len(regions[1][0][2]) // 2] = ord("N")
    regions[3][0][0].bases[0] = ord("N")
    regions[2][0][4].quals[-1] = 255                   # the SUM row looks this one up
    regions[4][0][1].quals[0] = 255
    return regions


def rotated(regions, k):
    return [(reads[k % len(reads):] + reads[:k % len(reads)], haps) for reads, haps in regions]


def unrotate(values, regions, k):
    """Results of rotated(regions, k) put back into the order of `regions`."""
    out, at = np.empty_like(values), 0
    for reads, haps in regions:
        n, nh = len(reads), len(haps)
        block = values[at:at + n * nh].reshape(n, nh)
        out[at:at + n * nh] = np.roll(block, k % n, axis=0).reshape(-1)
        at += n * nh
    return out


_wanted = {}


def _oracle(key, b):
    if key not in _wanted:
        _wanted[key] = oracle.compute_batch(b.as_dict(), n_threads=16)
    return _wanted[key]


def test_the_oracle_handles_every_input():
    """No GPU: every batch of this file is well-formed, and the oracle gives a non-positive number for every pair: finite
    wherever the region holds no zero byte (a zero base quality or gcp can make a pair impossible: -inf, never NaN)."""
    batches = []
    for s in (1, 16):
        b, what = make_scan_batch(s)
        batches.append(("scan-%d" % s, b, [r for r, w in enumerate(what) if w[2] is None]))
    batches += [("neighbour-" + k, b, range(len(b.out_off) - 1) if k in ("clean", "alone") else [1])
                for k, b in make_neighbour_batches().items()]
    regions = make_producer_regions()
    batches += [("producer", RegionBatch.from_regions(regions), range(len(regions))),
                ("producer-rot5", RegionBatch.from_regions(rotated(regions, 5)), range(len(regions)))]
    for key, b, no_zero in batches:
        want = _oracle(key, b)
        assert want.shape == (b.n_out,) and not np.isnan(want).any() and np.all(want <= 0.0), key
        for r in no_zero:
            assert np.all(np.isfinite(want[int(b.out_off[r]):int(b.out_off[r + 1])])), (key, r)
    used = sorted({len(rd) for reads, _ in regions for rd in reads})
    assert used == sorted(PRODUCER_LENGTHS)
    assert all(len({int(rd.gcp[0]) for rd in reads}) == len(reads) for reads, _ in regions)
    # un-rotating is the inverse of rotating
    b, r5 = RegionBatch.from_regions(regions), RegionBatch.from_regions(rotated(regions, 5))
    assert np.array_equal(unrotate(_oracle("producer-rot5", r5), regions, 5), _oracle("producer", b))
    # the scan cases: every alignment, and a zero byte at both ends of head, body and tail
    _, what = make_scan_batch(5)
    assert {w[0] for w in what[1:]} == set(SCAN_BYTES) and {w[1] % 16 for s in SHIFTS for w in make_scan_batch(s)[1][1:2]} == set(range(16))
    assert zero_positions(5, 1025) == [0, 10, 11, 1018, 1019, 1024] and zero_positions(16, 16) == [0, 15]


@pytest.fixture(scope="module")
def engines():
    from lorikeet_amd import HipPairHMMEngine
    e64, e32 = HipPairHMMEngine(0), HipPairHMMEngine(0, f32_first=True)
    yield e64, e32
    e64.close()
    e32.close()


def _planned(eng, b):
    plan = eng.plan(b)
    name = plan.dominant_kernel
    plan.close()
    return name


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,shift", [(16, s) for s in SHIFTS] + [(32, 7)])
def test_scan_edges(engines, lanes, shift):
    e64, _ = engines
    b, what = make_scan_batch(shift)
    want = _oracle("scan-%d" % shift, b)
    with e64.switches(force_L=lanes, force_chain=RUN, force_streams=1):
        assert _planned(e64, b).replace("chain_k<", "chain<").startswith("phmm_forward_chain<%d," % lanes)
        got = e64.compute(b)
    for r, w in enumerate(what):   # region by region, so that a failure names its case
        lo, hi = int(b.out_off[r]), int(b.out_off[r + 1])
        try:
            _close(got[lo:hi], want[lo:hi])
        except AssertionError as e:
            raise AssertionError("chain of %d bytes at offset %d, zero byte at %s in %s" % w) from e


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [16, 32])
def test_scan_does_not_read_its_neighbours(engines, lanes):
    """A zero byte just outside a chain sends the chain to the in-wave general path if the scan reads it.  That path rounds
    differently from the chained sweep, so the middle region's results can change -- but rarely do: measured on an MI355X
    on these inputs, the per-read kernel (force_chain=0, the closest stand-in for the general path that can be forced from
    outside) differs from the chained sweep in 1 of the middle region's 8 results, at 16 and at 32 lanes alike.  So this
    test tells an over-reading scan only weakly; that no byte outside the chain is loaded rests on the helper's index
    arithmetic (every index is clamped into the chain), which test_scan_edges exercises from the inside."""
    e64, _ = engines
    bs = make_neighbour_batches()
    with e64.switches(force_L=lanes, force_chain=RUN, force_streams=1):
        got = {k: e64.compute(b) for k, b in bs.items()}
    with e64.switches(force_L=lanes, force_chain=0):
        per_read = e64.compute(bs["clean"])
    clean = bs["clean"]
    lo, hi = int(clean.out_off[1]), int(clean.out_off[2])
    _close(got["clean"], _oracle("neighbour-clean", clean))
    print("L=%d: the per-read kernel differs from the chained sweep in %d of %d results of the middle region"
          % (lanes, int(np.sum(per_read[lo:hi] != got["clean"][lo:hi])), hi - lo))
    for k in ("A-last-gcp", "A-last-q", "B-first-gcp", "B-first-q"):
        assert np.array_equal(got[k][lo:hi], got["clean"][lo:hi]), k
        _close(got[k], _oracle("neighbour-" + k, bs[k]))
    assert np.array_equal(got["alone"], got["clean"][lo:hi])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,streams", PRODUCER_CASES)
def test_producer_edges(engines, lanes, streams):
    e64, _ = engines
    regions = make_producer_regions()
    b = RegionBatch.from_regions(regions)
    with e64.switches(force_L=lanes, force_chain=12, force_streams=streams):
        name = _planned(e64, b)
        assert name.replace("chain_k<", "chain<").startswith("phmm_forward_chain<%d," % lanes), name
        assert streams == 1 or name.endswith("x%d streams" % streams), name
        got = e64.compute(b)
        _close(got, _oracle("producer", b))
        for k in range(1, 12):   # every cyclic rotation of every region (regions of fewer reads see some twice)
            rot = e64.compute(RegionBatch.from_regions(rotated(regions, k)))
            assert np.array_equal(unrotate(rot, regions, k), got), "rotation by %d" % k


@pytest.mark.gpu
def test_producer_edges_f32(engines):
    _, e32 = engines
    b = RegionBatch.from_regions(make_producer_regions())
    want = _oracle("producer", b)
    with e32.switches(force_L=16, force_chain=12, force_streams=1):
        name = _planned(e32, b)
        assert re.match(r"phmm_forward_chain_f32(_any)?<16[,>]", name), name
        got = e32.compute(b)
    assert got.shape == want.shape and not np.isnan(got).any() and np.all(got <= 0.0)
    err = float(np.max(np.abs(got - want)))
    print("max |f32 - oracle| = %.3g" % err)
    assert err <= TOL_F32
