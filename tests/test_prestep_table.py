"""The proof that tests/test_prestep_hip.py can fail.  No GPU.

The pre-step (lorikeet_amd/csrc/phmm_prep_device.hpp) shows only through likelihoods and keep flags, and the PCR caches are
coarse, so a parity test passes with a wrong tandem-repeat scan unless its inputs are chosen against the caches.  Here
  * the restatement of tests/prestep_cases.py equals the oracle at every offset of every read, and its qualities and thresholds
    equal the oracle's under every configuration;
  * the census counts what the inputs promise (unit lengths 1 ... 20 both ways, repeat lengths 1 ... 33, the cap, rejected
    screen candidates in front of the true unit, repeats behind positions 64 and 128, tags on each side of the cache, ...);
  * every mutant of the restatement -- one per hazard of the device's two-level screen, of the quality rules and of the
    threshold -- moves a likelihood of the case set by at least 1e-6, a thousand device tolerances, or flips a keep flag;
  * every read's best likelihood is at least 1e-6 away from its threshold;
  * the host's rules the cases rely on (2 048 reads, lds_rows, 64 KiB, kLdsBytesPerCU, SRV_MAX_ROWS) are the sources'.

What stays invisible through likelihoods: the exact repeat count above 33 (every model's cache is 6 from there on; the
conservative one reaches 6 at 34), hence also the cap at 100 itself -- an uncapped count would read past the 101-entry cache, so
only its memory safety shows on the device -- and repeat length 1 against 2 (equal under every model).  A mutant is therefore
never asked to show at those lengths; the cases put every hazard at a length the caches resolve."""
import os
import re

import numpy as np
import pytest

import prestep_cases as pc
import server_instance_cases as server_cases
from oracle import oracle
from test_hip_parity import TOL_VS_ORACLE
from test_server_instance_table import limits

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lorikeet_amd", "csrc")
KILL = max(1e-6, 1000 * TOL_VS_ORACLE)      # a thousand device tolerances
MARGIN = KILL


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _unique_reads():
    return sorted({r for g in pc.regions() for r in g.reads})


def _read_index(c, region_name, k):
    g = [x.name for x in pc.regions()].index(region_name)
    return int(c.batch.region_read_off[g]) + k


# ---- the restatement is the oracle's ----------------------------------------------------------------------------------------------
def test_the_restated_scan_equals_the_oracle_at_every_offset():
    lib, n = oracle.lib(), 0
    reads = _unique_reads() + [pc.long_case(x).batch.read_bases.tobytes() for x in pc.LONG_LENGTHS + (pc.REFUSED_LENGTH,)]
    for s in reads:
        a, p = oracle._u8(s)
        got = pc.scans(s)
        for off in range(len(s)):
            assert lib.oracle_find_tandem_repeat_length(p, len(a), off) == got[off].length, (s, off)
            n += 1
    assert n > 30000
    assert pc.MAX_STR_UNIT_LENGTH == 20 and pc.MAX_REPEAT_LENGTH == 100
    prep = _source("phmm_prep_device.hpp")
    assert "constexpr int MAX_STR_UNIT_LENGTH = 20;" in prep and "constexpr int MAX_REPEAT_LENGTH = 100;" in prep and "constexpr uint32_t MIN_USABLE_Q = 6;" in prep


@pytest.mark.parametrize("name", pc.CONFIG_NAMES)
def test_the_restated_qualities_and_thresholds_equal_the_oracle(name):
    c = pc.case(name)
    b, cfg, tags = c.batch, c.cfg, pc.uses_tags(c)
    assert tags or (b.ins_q == 45).all() and (b.del_q == 45).all()
    for r, (s, t) in enumerate(pc.read_slices(c)):
        q, i, d = oracle.modify_read_qualities(pc.MODELS[cfg.pcr_error_model], b.read_bases[s:t], int(c.mapq[r]), b.base_q[s:t], b.ins_q[s:t], b.del_q[s:t],
                                               cfg.base_quality_score_threshold, bool(cfg.disable_cap_read_qualities_to_mapq))
        got = pc.modify(b.read_bases[s:t].tobytes(), int(c.mapq[r]), b.base_q[s:t], b.ins_q[s:t] if tags else None, b.del_q[s:t] if tags else None,
                        cfg.pcr_error_model, cfg.base_quality_score_threshold, bool(cfg.disable_cap_read_qualities_to_mapq))
        assert (q.tolist(), i.tolist(), d.tolist()) == got, (name, r)
        want = oracle.read_disqualification_threshold(b.base_q[s:t], bool(cfg.dynamic_read_disqualification), cfg.read_disqualification_scale,
                                                      cfg.expected_error_rate_per_base)
        assert pc.threshold(b.base_q[s:t], bool(cfg.dynamic_read_disqualification), cfg.read_disqualification_scale, cfg.expected_error_rate_per_base) == want, (name, r)
    table = re.search(r"kDynQualTable\[40\]\[2\] = \{(.*?)\};", _source("phmm_prep_device.hpp"), re.S)
    assert tuple(float(x) for x in re.findall(r"[\d.]+", table.group(1))) == tuple(x for row in pc.DYN_TABLE for x in row)


# ---- the census ----------------------------------------------------------------------------------------------------------------
def test_census_of_the_scan():
    bw, fw, lengths, uncapped, traps, behind = set(), set(), set(), 0, {}, {64: 0, 128: 0, 192: 0}
    different = {"same-length": 0, "other-length": 0, "tiles-behind": 0, "tiles-behind-long": 0}
    for s in _unique_reads():
        for off, x in enumerate(pc.scans(s)):
            bw.add(x.bw_len), fw.add(x.fw_len), lengths.add(x.length)
            uncapped = max(uncapped, x.uncapped)
            for rej, hit in ((x.bw_rejected, x.bw_len), (x.fw_rejected, x.fw_len)):
                if rej >= 5 and hit > rej:
                    traps[rej] = traps.get(rej, 0) + 1
            for lo in behind:
                behind[lo] += off >= lo and x.length >= 3 and max(x.bw_len, x.fw_len) >= 2
            if x.bw_len and x.fw_len and s[off + 1 - x.bw_len:off + 1] != s[off + 1:off + 1 + x.fw_len]:
                different["same-length" if x.bw_len == x.fw_len else "other-length"] += 1
                tiles = pc._count(s, off + 1, x.fw_len, 0, off + 1, False)
                different["tiles-behind"] += tiles > 0
                different["tiles-behind-long"] += tiles > 0 and x.fw_len > 4
    print("accepted unit lengths, backward: %s" % sorted(bw - {0}))
    print("accepted unit lengths, forward:  %s" % sorted(fw - {0}))
    print("repeat lengths: %s; largest uncapped count %d" % (sorted(lengths), uncapped))
    print("screen passed, unit rejected, longer unit accepted (rejected length: positions): %s" % dict(sorted(traps.items())))
    print("positions inside a repeat of a unit of two bases or more, from 64 / 128 / 192 on: %s" % behind)
    print("backward and forward units differ: %s" % different)
    assert bw - {0} == fw - {0} == set(range(1, 21))
    assert set(range(1, 34)) <= lengths and any(34 <= x <= 99 for x in lengths) and 100 in lengths and uncapped > 100
    assert len(traps) >= 5 and max(traps) >= 15 and min(traps.values()) >= 3
    assert min(behind.values()) >= 100
    assert min(different.values()) >= 3
    # what the regions are named for
    for L in range(1, 21):
        g = next(x for x in pc.regions() if x.name == "unit-%d" % L)
        by = dict(zip(g.notes, g.reads))
        u = by["start"][:L]
        assert by["start"].startswith(u * 3) and not by["start"].startswith(u * 4) and by["start+1"] == by["start"][1:]
        assert by["end"].endswith(u * 6) and not by["end"].endswith(u * 7) and by["end-1"] == by["end"][:-1][-len(by["end-1"]):]
        assert u * 4 in by["middle"] and u * 5 in by["alt-longer"] and u * 2 in by["alt-shorter"] and u * 3 not in by["alt-shorter"][:15 + 3 * L]
        for x in (64, 128, 192):
            assert by["across-%d" % x][x - 2 * L:x + 2 * L] == u * 4, (L, x)
        # exact fits: the copy in front of the offset starts at position 0 (accepted) and one base short of it (not there)
        assert pc.scan(by["start"], 2 * L - 1).bw_len == L and pc.scan(by["start+1"], 2 * L - 2).bw_len != L
        n = len(by["end"])
        assert pc.scan(by["end"], n - 1 - 2 * L).fw_len == L and pc.scan(by["end"], n - 2 * L).fw_len != L      # the copy ends at n / one past n
        assert pc.scan(by["end-1"], n - 2 - 2 * L).fw_len == L and pc.scan(by["end-1"], n - 1 - 2 * L).fw_len != L
    runs = {g.name: g for g in pc.regions() if g.name.startswith("run-")}
    assert sorted(runs) == ["run-A-100", "run-A-101", "run-A-150", "run-A-99", "run-CA-202"]
    assert runs["run-A-150"].reads[1] == b"A" * 150 and set(pc.repeat_lengths(b"A" * 150)) == {100}
    assert {x.uncapped for x in pc.scans(runs["run-A-99"].reads[0])} >= {99} and max(x.uncapped for x in pc.scans(runs["run-A-99"].reads[0])) == 99
    assert max(x.uncapped for x in pc.scans(runs["run-A-100"].reads[0])) == 100 and max(x.uncapped for x in pc.scans(runs["run-A-101"].reads[0])) == 101
    assert runs["run-CA-202"].reads[1] == b"CA" * 101 and max(x.uncapped for x in pc.scans(b"CA" * 101)) == 101
    short = next(g for g in pc.regions() if g.name == "short")
    assert tuple(len(r) for r in short.reads) == pc.SHORT_LENGTHS == (1, 2, 3, 63, 64, 65, 128, 129, 268)
    odd = next(g for g in pc.regions() if g.name == "special")
    odd = odd.reads[odd.notes.index("N-and-lower-case")]
    assert b"N" in odd and b"t" in odd and 2 in {x.bw_len for x in pc.scans(odd)}
    for g in pc.regions():
        assert len(set(g.haps)) == len(g.haps) and max(len(r) for r in g.reads) <= server_cases.SRV_MAX_ROWS and min(len(r) for r in g.reads) >= 1
        assert 2 <= len(g.haps) <= 3 and len(g.reads) <= 45


def test_census_of_the_qualities():
    seen = {"below": 0, "equal": 0, "above": 0, "unusable": 0}
    for name in pc.CONFIG_NAMES:
        c = pc.case(name)
        b, cache = c.batch, pc.cache_of(c.cfg.pcr_error_model)
        if not (cache and pc.uses_tags(c)):
            continue
        for s, t in pc.read_slices(c):
            rl = pc.repeat_lengths(b.read_bases[s:t].tobytes())
            for i in range(t - s - 1):
                for tag in (int(b.ins_q[s + i]), int(b.del_q[s + i])):
                    seen["below"] += tag < cache[rl[i]]
                    seen["equal"] += tag == cache[rl[i]]
                    seen["above"] += tag > cache[rl[i]]
                    seen["unusable"] += tag < pc.MIN_USABLE_Q
    print("tags against the cache value of their position: %s" % seen)
    assert min(seen.values()) >= 1000
    c = pc.case(pc.CONFIG_NAMES[0])
    quals = set(c.batch.base_q.tolist())
    assert {0, 1, 2, 40, 41, 42, 60, 93, 255} <= quals and any(q < 18 for q in quals) and {17, 18} <= quals
    assert {0, 10, 60} <= set(c.mapq.tolist())
    by = {k.name: k for k in pc.CONFIGS}
    assert {k.cfg_kw["pcr"] for k in pc.CONFIGS} == {0, 1, 2, 3}
    assert {(k.cfg_kw["pcr"] != 0, bool(k.cfg_kw.get("dynamic")), k.tags) for k in pc.CONFIGS} >= {(True, False, True), (True, True, False), (True, True, True),
                                                                                                   (True, False, False), (False, False, False), (False, True, True)}
    assert {bool(k.cfg_kw.get("disable_cap")) for k in pc.CONFIGS} == {False, True}
    # the two configurations the device test compares to see the model: equal but for the model
    assert dict(by["conservative-static-null"].cfg_kw, pcr=0) == by["none-static-null"].cfg_kw


def test_census_of_the_keep_flags():
    kept = {False: set(), True: set()}
    side = {"dyn<cap": set(), "dyn>cap": set()}
    for name in pc.CONFIG_NAMES:
        c = pc.case(name)
        e = pc.expected(c)
        dynamic = bool(c.cfg.dynamic_read_disqualification)
        kept[dynamic] |= set(e.keep.tolist())
        if dynamic:
            g0 = _read_index(c, "dynamic-steps", 0)
            for k, (probe, low, _) in enumerate(pc.DYN_PROBES):
                q = pc.dyn_quals(probe, low)[0]
                dyn = oracle.lib().oracle_log10_dynamic_read_qual_threshold(oracle._u8(q)[1], len(q), c.cfg.read_disqualification_scale)
                cap = oracle.lib().oracle_log10_min_true_likelihood(len(q), c.cfg.expected_error_rate_per_base, 0)
                side["dyn<cap" if dyn < cap else "dyn>cap"].add(bool(e.keep[g0 + k]))
        print("%s: %d of %d reads kept" % (name, int(e.keep.sum()), len(e.keep)))
    assert kept == {False: {False, True}, True: {False, True}}
    assert side == {"dyn<cap": {False, True}, "dyn>cap": {False, True}}      # kept and removed reads on either side
    # the static pairs: ceil(n * rate) steps inside the pair, the likelihood lies between the two thresholds, keep differs
    for name, pair, thresholds in (("hostile-static-tags", "pair-50-51-1mm", (-4.0, -8.0)), ("conservative-static-null", "pair-50-51-1mm", (-4.0, -8.0)),
                                   ("aggressive-static-null-rate01", "pair-100-101-1mm", (-4.0, -8.0)),
                                   ("hostile-dynamic-null", "pair-100-101-2mm", (-8.0, -12.0)), ("none-dynamic-tags", "pair-100-101-2mm", (-8.0, -12.0))):
        c = pc.case(name)
        g = next(x for x in pc.regions() if x.name == "static-steps")
        k = g.notes.index(pair)
        r = _read_index(c, "static-steps", k)
        best, thr = pc.best_and_threshold(c)
        assert (thr[r], thr[r + 1]) == thresholds, (name, pair, thr[r], thr[r + 1])
        assert thr[r + 1] + MARGIN < best[r + 1] and best[r] < thr[r] - MARGIN, (name, pair, best[r], best[r + 1])
        assert (bool(pc.expected(c).keep[r]), bool(pc.expected(c).keep[r + 1])) == (False, True), (name, pair)
    # (at the rate 0.02 the static threshold is min(2, errors) * -4: the step at 100 | 101 cannot show there)
    assert pc.threshold([30] * 100, False, 1.0, 0.02) == pc.threshold([30] * 101, False, 1.0, 0.02) == -8.0


# ---- every mutant is killed ---------------------------------------------------------------------------------------------------------
def _shows_under(mutant):
    """The configurations under which a mutant of the qualities can show."""
    if mutant == "h":
        return list(pc.CONFIG_NAMES)                                                  # (base qualities too: also without a model)
    if mutant == "i":
        return [k.name for k in pc.CONFIGS if k.cfg_kw["pcr"] and k.tags]
    return [k.name for k in pc.CONFIGS if k.cfg_kw["pcr"]]


@pytest.mark.parametrize("mutant", pc.QUALITY_MUTANTS)
def test_every_mutant_of_the_qualities_moves_a_likelihood(mutant):
    assert TOL_VS_ORACLE == 1e-9 and KILL >= 1000 * TOL_VS_ORACLE
    names = _shows_under(mutant)
    assert names
    kills = {}
    for name in names:
        c = pc.case(name)
        per_read = {r: x for r, x in enumerate(pc.mutant_qualities(c, mutant)) if x is not None}
        change, tried = pc.likelihood_change(c, per_read) if per_read else (0.0, 0)
        kills[name] = change
        print("mutant %s under %s: %d reads with other qualities, %d tried, largest likelihood change %.3g" % (mutant, name, len(per_read), tried, change))
    assert max(kills.values()) >= KILL, (mutant, kills)
    if mutant == "h":
        # waves_per_read = 1 is the server's route for every plain case and the engine's for the multiplied case: each kills it
        assert all(v >= KILL for v in kills.values()), kills
        m, first = pc.multiplied_case()
        assert m.batch.n_reads > pc.SMALL_CALL_READS and pc.waves_per_read(m.batch.n_reads, server_cases.max_r(m)) == 1
        assert kills[pc.MULTIPLIED_CONFIG] >= KILL and first[:len(pc.regions())] == list(range(len(pc.regions())))


def _keeps(c, mutant):
    b, cfg = c.batch, c.cfg
    best, _ = pc.best_and_threshold(c)
    tags = pc.uses_tags(c)
    out = []
    for r, (s, t) in enumerate(pc.read_slices(c)):
        mod = pc.modify(b.read_bases[s:t].tobytes(), int(c.mapq[r]), b.base_q[s:t], b.ins_q[s:t] if tags else None, b.del_q[s:t] if tags else None,
                        cfg.pcr_error_model, cfg.base_quality_score_threshold, bool(cfg.disable_cap_read_qualities_to_mapq))[0] if mutant == "l" else None
        thr = pc.threshold(b.base_q[s:t], bool(cfg.dynamic_read_disqualification), cfg.read_disqualification_scale, cfg.expected_error_rate_per_base, mutant, mod)
        out.append(not best[r] < thr)
    return np.array(out)


@pytest.mark.parametrize("mutant", pc.THRESHOLD_MUTANTS)
def test_every_mutant_of_the_threshold_flips_a_keep_flag(mutant):
    names = [k.name for k in pc.CONFIGS if mutant.startswith("j") or k.cfg_kw.get("dynamic")]
    flips = {}
    for name in names:
        c = pc.case(name)
        assert np.array_equal(_keeps(c, None), pc.expected(c).keep), name      # (the restated decision is the oracle's)
        flips[name] = int((_keeps(c, mutant) != pc.expected(c).keep).sum())
        print("mutant %s under %s: %d keep flags flipped" % (mutant, name, flips[name]))
    assert max(flips.values()) >= 1, (mutant, flips)


# ---- margins ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.CONFIG_NAMES + ("multiplied",) + tuple("long-%d" % n for n in pc.LONG_LENGTHS))
def test_every_read_is_far_from_its_threshold(name):
    if name == "multiplied":
        out, keep = pc.expected_multiplied()
        c, _ = pc.multiplied_case()
        assert not np.isnan(out).any() and (out <= 0).all() and len(keep) == c.batch.n_reads > pc.SMALL_CALL_READS
        assert int(c.batch.read_off[-1]) <= pc.ONE_SHOT_BYTES           # one call, not chunks of fewer reads
        return
    c = pc.long_case(int(name[5:])) if name.startswith("long-") else pc.case(name)
    e = pc.expected(c)
    assert not np.isnan(e.likelihoods).any() and (e.likelihoods <= 0).all()
    best, thr = pc.best_and_threshold(c)
    gap = np.abs(best - thr)
    print("%s: smallest |best likelihood - threshold| = %.3g" % (name, gap.min()))
    assert (gap >= MARGIN).all(), (name, np.flatnonzero(gap < MARGIN))
    if name.startswith("long-"):
        s = c.batch.read_bases.tobytes()
        assert len(s) == int(name[5:]) and e.keep[0] and 20 in {x.bw_len for x in pc.scans(s)[-80:]} and {3} <= {x.length for x in pc.scans(s)[-80:]}


@pytest.mark.parametrize("name", pc.CONFIG_NAMES)
def test_the_plain_cases_are_inside_the_servers_limits(name):
    ok = limits(pc.case(name))
    assert all(ok.values()), [k for k, v in ok.items() if not v]


# ---- the host's rules ---------------------------------------------------------------------------------------------------------------
def test_the_restated_host_rules_are_the_sources():
    api, region, kernels, plan, header = (_source(n) for n in ("phmm_api.cpp", "phmm_region.cpp", "phmm_engine_kernels.hip", "phmm_plan.hpp", "phmm_server.hpp"))
    server = _source("phmm_server.cpp")
    assert pc.SMALL_CALL_READS == 2048
    assert "pp.waves_per_read = n_reads <= 2048 ? std::max<uint32_t>(1, (max_r + 63) / 64) : 1;" in api
    assert "pp.waves_per_read = nr <= 2048 ? std::max<uint32_t>(1, (max_r + 63) / 64) : 1;" in region
    assert "pp.waves_per_read = 1;" in server and "pp.lds_rows = prep_rows;" in server and "const uint32_t prep_rows = (max_r + 1 + 7) / 8 * 8;" in server
    assert "pp.lds_rows = (uint32_t)align_up((size_t)max_r + 1, 8);" in api and "pp.lds_rows = (uint32_t)((max_r + 1 + 7) / 8 * 8);" in region
    assert "const int wpb = 4;" in kernels and "const size_t lds = (size_t)p.lds_rows * 17 * wpb;" in kernels and "if (lds > 64 * 1024) {" in kernels
    assert "hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);" in kernels
    assert (pc.LDS_BYTES_PER_ROW, pc.WAVES_PER_BLOCK, pc.LDS_DEFAULT_LIMIT) == (17, 4, 64 * 1024)
    assert "constexpr size_t kLdsBytesPerCU = 160 * 1024;" in plan and pc.LDS_BYTES_PER_CU == 160 * 1024
    assert "if (ok && (size_t)pp.lds_rows * 17 * 4 > kLdsBytesPerCU) {" in api and "if ((size_t)pp.lds_rows * 17 * 4 > 160 * 1024) {" in region
    assert 'h->err = "phmm_engine_compute: read too long for the pre-step kernel";' in api and 'h->err = who + ": read too long for the pre-step kernel";' in region
    assert "static const size_t kOneShotBytes = 512u << 10;" in api and pc.ONE_SHOT_BYTES == 512 << 10
    assert "if (n_regions < 8 || (size_t)read_off[n_reads] <= kOneShotBytes || h->sw.no_pipeline) {" in api
    assert "constexpr uint32_t SRV_MAX_ROWS = SRV_LDS_BYTES / LDS_ROW_BYTES - 2;" in header and server_cases.SRV_MAX_ROWS == 268
    # the rule itself
    assert [pc.waves_per_read(n, r) for n, r in ((1, 1), (1, 64), (1, 65), (2048, 268), (2049, 268))] == [1, 1, 2, 5, 1]
    assert [pc.lds_rows(n) for n in (1, 7, 8, 268)] == [8, 8, 16, 272]
    # the long reads follow from the rules
    assert pc.FIRST_OVER_64K == 960 and pc.lds_bytes(959) == 65280 <= 65536 < pc.lds_bytes(960) == pc.lds_bytes(964) == 65824
    assert pc.LONGEST_ACCEPTED == 2407 and pc.lds_bytes(2407) == 163744 <= 163840 < pc.lds_bytes(2408) == 164288 and pc.REFUSED_LENGTH == 2408
    assert pc.LONG_LENGTHS == (959, 960, 964, 2407)
    for n in pc.LONG_LENGTHS + (pc.REFUSED_LENGTH,):
        c = pc.long_case(n)
        assert c.batch.n_reads == 1 and server_cases.max_r(c) == n and c.batch.n_haps == 2 and n < server_cases.max_h(c) <= n + 40
    # plain cases: some reads over 64 bases, so the engine and the launched region route spread a read over several waves
    for name in pc.CONFIG_NAMES:
        c = pc.case(name)
        assert c.batch.n_reads <= 2048 and pc.waves_per_read(c.batch.n_reads, server_cases.max_r(c)) == 5
