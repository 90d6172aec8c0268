"""The tables tests/test_forward_instances_hip.py iterates over are the kernel sources' (a newly compiled forward instance, a
moved threshold or a changed range fails here until the sweep covers it), every generated batch selects its instance in the
planner (phmm_plan_describe: host only), has the lengths the instance's own code is sensitive to, and stays -- by the oracle
alone -- where the instance under test produces the numbers and not phmm_rescue.  No GPU."""
import os
import re

import numpy as np
import pytest

import test_forward_instances_hip as sweep
from lorikeet_amd import _lib
from lorikeet_amd.engine import plan_describe
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lorikeet_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _macro_body(text, name):
    m = re.search(r"#define\s+%s\(X(?:,\s*L)?\)((?:.*\\\n)*.*)\n" % re.escape(name), text)
    assert m, name
    return m.group(1)


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(\d+)" % re.escape(name), text)
    assert m, name
    return int(m.group(1))


def _makefile_values(flag):
    return tuple(sorted(int(v) for v in set(re.findall(r"-D%s=(\d+)" % re.escape(flag), _source("Makefile")))))


def test_the_sweep_covers_exactly_the_compiled_instances():
    per_read, chain, chain32 = _source("phmm_kernels.hip"), _source("phmm_chain_kernels.hip"), _source("phmm_chain32_kernels.hip")
    internal, device, api = _source("phmm_internal.hpp"), _source("phmm_device.hpp"), _source("phmm_plan.hpp") + _source("phmm_plan.cpp")
    # per read: the launch table and the planner's list name the same K, once each, for every compiled lane count
    k_list = tuple(int(k) for k in re.findall(r"X\(L,\s*(\d+)\)", _macro_body(per_read, "PHMM_K_LIST")))
    m = re.search(r"const\s+int\s+kInstantiatedK\[\]\s*=\s*\{([^}]*)\}", per_read)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == k_list == sweep.FORWARD_K
    assert _makefile_values("PHMM_L") == sweep.LANES
    assert sweep.FORWARD_CASES == [(L, K) for L in sweep.LANES for K in sweep.FORWARD_K] and len(set(sweep.FORWARD_CASES)) == 93
    # chained f64: per-K kernels, the ranges of the mixed launches, the planner's limit
    chain_k = tuple(int(k) for k in re.findall(r"X\((\d+)\)", _macro_body(chain, "PHMM_CHAIN_K_LIST")))
    assert chain_k == sweep.CHAIN_K and _makefile_values("PHMM_CHAIN_L") == sweep.CHAIN_LANES
    m = re.search(r"int\s+chain_max_k\(\)\s*\{\s*return\s+(\d+);", chain)
    assert m and int(m.group(1)) == max(sweep.CHAIN_K)
    ranges = tuple((int(lo), int(hi)) for _, lo, hi in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", _macro_body(internal, "PHMM_CHAIN_RANGES")))
    assert ranges == sweep.CHAIN_RANGES
    assert [k for lo, hi in ranges for k in range(lo, hi + 1)] == list(sweep.CHAIN_K)          # every K in exactly one range
    assert {(L, K) for L, K, _ in sweep.CHAIN_CASES} == {(L, K) for L in sweep.CHAIN_LANES for K in sweep.CHAIN_K}
    assert len({(L, K) for L, K, _ in sweep.CHAIN_CASES}) == 72 and len(sweep.CHAIN_CASES) == len(set(sweep.CHAIN_CASES)) == 72 + 3 * 24
    assert {s for L, _, s in sweep.CHAIN_CASES if L == 16} == {0, 1, 2, 4} and {s for L, _, s in sweep.CHAIN_CASES if L != 16} == {0}
    assert sweep.RANGE_CASES == [(L, lo, hi) for L in sweep.CHAIN_LANES for lo, hi in ranges] and len(sweep.RANGE_CASES) == 12
    assert all(sweep.RUN64_K[L] in sweep.CHAIN_K for L in sweep.CHAIN_LANES)
    # chained f32
    chain32_k = tuple(int(k) for k in re.findall(r"X\((\d+)\)", _macro_body(chain32, "PHMM_CHAIN32_K_LIST")))
    assert chain32_k == sweep.CHAIN32_K and _makefile_values("PHMM_CHAIN32_L") == sweep.CHAIN32_LANES
    assert {(L, K) for L, K, _ in sweep.CHAIN32_CASES} == {(L, K) for L in sweep.CHAIN32_LANES for K in sweep.CHAIN32_K}
    assert len({(L, K) for L, K, _ in sweep.CHAIN32_CASES}) == 48 and len(sweep.CHAIN32_CASES) == len(set(sweep.CHAIN32_CASES)) == 48 + 2 * 24
    assert {s for L, _, s in sweep.CHAIN32_CASES if L == 16} == {1, 2, 4} and {s for L, _, s in sweep.CHAIN32_CASES if L != 16} == {1}
    assert set(sweep.ANY_KS) <= set(sweep.CHAIN32_K) and len(set(sweep.ANY_KS)) >= 3
    # thresholds the batches are shaped by
    assert _define(device, "PHMM_SDWA_MIN_K") == sweep.SDWA_MIN_K
    assert _define(device, "PHMM_CND_MAX_K") == sweep.CND_MAX_K
    assert _define(device, "PHMM_TWO_WAVE_MAX_K") == sweep.TWO_WAVE_MAX_K
    assert re.search(r"constexpr\s+uint32_t\s+kNumSimd\s*=\s*256\s*\*\s*4;", api) and sweep.NUM_SIMD == 1024
    assert re.search(r"constexpr\s+int\s+CHAIN_MAX_READS\s*=\s*(\d+);", internal).group(1) == str(sweep.CHAIN_MAX_READS)
    # the body choice the two per-read launches are sized for
    assert "c.cnd_select = waves < 2ull * kNumSimd ? 1u : 0u;" in api and "bool split = (uint64_t)n_items < 4ull * kNumSimd;" in api
    # the f32 kernel's line, and the band's
    assert "sum >= 0x1p-96f" in chain32 and "c_unit = 0x1p100f" in chain32
    assert abs(sweep.TRUST_LINE - (-196) * np.log10(2.0)) < 0.01 and sweep.BAND[0] < sweep.TRUST_LINE - 10 and sweep.BAND[1] > sweep.TRUST_LINE + 10


def _describe(monkeypatch, b, L, chain, streams, f32=False):
    monkeypatch.setenv("PHMM_FORCE_L", str(L))
    monkeypatch.setenv("PHMM_FORCE_CHAIN", str(chain))
    monkeypatch.setenv("PHMM_FORCE_STREAMS", str(streams))
    return plan_describe(b, flags=_lib.PHMM_FLAG_F32_FIRST if f32 else 0)


def _lengths(b):
    hl = np.diff(b.hap_off.astype(np.int64))
    rl = np.diff(b.read_off.astype(np.int64))
    nh = np.diff(b.region_hap_off.astype(np.int64))
    nr = np.diff(b.region_read_off.astype(np.int64))
    return hl, rl, nh, nr


def _pairs_kept(b):
    """The 95 % / 1e-300 condition, by the oracle alone -> cells asked for."""
    want = oracle.compute_batch(b.as_dict(), n_threads=16)
    assert not np.isnan(want).any() and float(np.mean(np.isfinite(want) & (want > -300.0))) >= 0.95
    return b.cells()


@pytest.mark.parametrize("case", sweep.FORWARD_CASES, ids=sweep.forward_id)
def test_generated_batches_select_their_instance(monkeypatch, case):
    L, K = case
    G, full = 64 // L, L * K
    b, general = sweep.make_batch(L, K)
    again, _ = sweep.make_batch(L, K)
    assert all(np.array_equal(getattr(b, f), getattr(again, f)) for f in b.FIELDS)          # the same bytes every time
    big = sweep.make_big_batch(L, K)
    hl, rl, nh, nr = _lengths(b)
    # every region's longest haplotype selects K; the three boundary lengths are the longest of some region
    assert set(sweep.region_k(b, L)) == {K} and set(sweep.region_k(big, L)) == {K}
    longest = {int(hl[int(b.region_hap_off[g]):int(b.region_hap_off[g + 1])].max()) for g in range(b.n_regions)}
    assert longest == {L * (K - 1) + 1, full - 1, full}
    if K > sweep.SDWA_MIN_K:   # the last real column on an odd and on an even packed half-word
        assert {((h - 1) % K) % 2 for h in longest} == {0, 1}
    # the shorter ones beside them: one column, one lane, a lane and a column, half the lanes idle, an edge column that is a lane's last
    for need in (1, K, K + 1, full // 2):
        assert need in hl, need
    assert any(h % K == 0 and h < L * (K - 1) for h in hl) and any(-(-int(h) // K) <= L // 2 for h in hl)
    # haplotype counts: one, the wave's slots exactly, one more (idle slots in the second group), nine at 16 lanes
    for need in sweep.hap_counts(L):
        assert need in nh, need
    assert any(n % G for n in nh) or G == 1
    # reads: 1, 2, L - 1, L, L + 1, about 150, one above 256 rows; legal qualities over the whole range
    for need in (1, 2, L - 1, L, L + 1, 150):
        assert need in rl, need
    assert rl.max() > 256 and rl.min() >= 1
    assert b.ins_q.min() >= 6 and b.del_q.min() >= 6 and b.ins_q.max() == b.del_q.max() == b.base_q.max() == b.gcp.max() == 60
    # read counts: none a multiple of the forced run, a run of one read, fewer reads than two / four streams
    assert all(n % sweep.RUN for n in nr) and any(n % sweep.RUN == 1 for n in nr) and 1 in nr and 3 in nr
    # the general-path regions, and only they, hold an 'N', a gcp == 0 and a base quality 0
    gen_regions = [g for g in range(b.n_regions) if general[int(b.out_off[g])]]
    assert len(gen_regions) == 2
    for g in range(b.n_regions):
        r0, r1 = int(b.read_off[int(b.region_read_off[g])]), int(b.read_off[int(b.region_read_off[g + 1])])
        h0, h1 = int(b.hap_off[int(b.region_hap_off[g])]), int(b.hap_off[int(b.region_hap_off[g + 1])])
        special = ((b.hap_bases[h0:h1] == ord("N")).sum(), (b.gcp[r0:r1] == 0).sum(), (b.base_q[r0:r1] == 0).sum())
        assert special == ((1, 1, 1) if g in gen_regions else (0, 0, 0)), (g, special)
    assert general[int(b.out_off[gen_regions[0]]):int(b.out_off[gen_regions[0] + 1])].all() and 0 < general.sum() < general.size
    # per read: the small launch takes the v_cndmask body where there is one, the large one the EXEC body without a split
    quads = max(-(-int(n) // G) for n in nh)
    assert b.n_reads * quads < 2 * sweep.NUM_SIMD and big.n_reads >= 4 * sweep.NUM_SIMD
    _, big_rl, big_nh, _ = _lengths(big)
    assert 8 <= big_rl.min() and big_rl.max() <= 16 and set(big_nh) == set(sweep.hap_counts(L))
    for what, bb in (("small", b), ("big", big)):
        info = _describe(monkeypatch, bb, L, 0, 0)
        assert info.dominant_kernel.decode() == "phmm_forward<%d,%d>" % (L, K) and info.n_chain_launches == 0, what
        assert info.n_launches == 1, what
    # chained: the per-K kernel under every stream setting of the sweep, f64 and f32
    if K in sweep.CHAIN_K:
        for streams in [s for LL, KK, s in sweep.CHAIN_CASES if (LL, KK) == (L, K)]:
            info = _describe(monkeypatch, b, L, sweep.RUN, streams)
            assert sweep.expect_chain_name(info.dominant_kernel.decode(), L, K, streams), info.dominant_kernel
            assert info.n_launches == info.n_chain_launches == 1 and info.min_reads_per_run == 1
        for streams in [s for LL, KK, s in sweep.CHAIN32_CASES if (LL, KK) == (L, K)]:
            info = _describe(monkeypatch, b, L, sweep.RUN, streams, f32=True)
            assert sweep.expect_chain_name(info.dominant_kernel.decode(), L, K, streams, f32=True), info.dominant_kernel
    else:
        assert K > max(sweep.CHAIN_K) and _describe(monkeypatch, b, L, sweep.RUN, 0).n_chain_launches == 0
    # the oracle alone: at least 95 % of the pairs finite and above 1e-300
    _pairs_kept(b)
    _pairs_kept(big)


@pytest.mark.parametrize("case", sweep.RANGE_CASES, ids=sweep.range_id)
def test_range_batches_are_mixed_launches(monkeypatch, case):
    L, lo, hi = case
    ks = sweep.range_ks(lo, hi)
    assert len(set(ks)) >= 3 and ks[0] == lo and ks[-1] == hi
    b, _ = sweep.make_mixed_batch(L, ks)
    assert set(sweep.region_k(b, L)) == set(ks)
    info = _describe(monkeypatch, b, L, sweep.RUN, 0)
    assert re.fullmatch(r"phmm_forward_chain<%d,%d,%d> \(K = \d+\)( x[24] streams)?" % (L, lo, hi), info.dominant_kernel.decode())
    assert info.n_launches == info.n_chain_launches == 1      # every class of the batch in the one launch of the range


@pytest.mark.parametrize("L", sweep.CHAIN32_LANES)
def test_any_k_batches_are_mixed_launches(monkeypatch, L):
    b, _ = sweep.make_mixed_batch(L, sweep.ANY_KS)
    assert set(sweep.region_k(b, L)) == set(sweep.ANY_KS)
    info = _describe(monkeypatch, b, L, sweep.RUN, 1, f32=True)
    assert re.fullmatch(r"phmm_forward_chain_f32_any<%d> \(K = \d+\)" % L, info.dominant_kernel.decode())
    assert info.n_chain_launches == 1


@pytest.mark.parametrize("L", sweep.CHAIN_LANES)
def test_run_of_64_batches(monkeypatch, L):
    K = sweep.RUN64_K[L]
    b, _ = sweep.make_run64_batch(L, K)
    _, _, _, nr = _lengths(b)
    assert nr.max() == 70 and set(sweep.region_k(b, L)) == {K}
    info = _describe(monkeypatch, b, L, sweep.CHAIN_MAX_READS, 1)
    assert sweep.expect_chain_name(info.dominant_kernel.decode(), L, K, 1)
    _pairs_kept(b)


@pytest.mark.parametrize("H", sorted({c[0] for c in sweep.BAND_CASES}))
def test_trust_line_band_is_populated_on_both_sides(monkeypatch, H):
    b = sweep.band_batch(H)
    want = oracle.compute_batch(b.as_dict(), n_threads=16)
    x = sweep.band_axis(b, want)
    assert np.isfinite(want).all() and sweep.band_is_populated(x)
    lo, hi = sweep.band_reads(b, x)
    assert (hi < sweep.TRUST_LINE - 1).sum() >= 100 and (lo > sweep.TRUST_LINE + 1).sum() >= 100
    assert ((lo < sweep.TRUST_LINE - 1) & (hi > -5)).sum() >= 10     # reads with pairs on both sides of the line
    for HH, L, streams in sweep.BAND_CASES:
        if HH == H:
            info = _describe(monkeypatch, b, L, 6, streams, f32=True)
            assert re.match(r"phmm_forward_chain_f32(_any)?<%d[,>]" % L, info.dominant_kernel.decode()), info.dominant_kernel
