"""The tables tests/test_server_instances_hip.py iterates over are the resident region server's own (a newly compiled or removed
instance of phmm_server_kernels.hip fails here until the sweep follows), the host's selection rule names a compiled instance
for every haplotype length it admits (every `switch` over those tables ends in `default: break;` -- a K the host selects and
the kernel does not carry would run nothing and write nothing), every compiled instance is the target of a case at each end of
its range, every case is inside -- every declined case one step outside -- the limits of server_region_submit, and the inputs
keep, by the oracle alone, every discrete output a thousand tolerances away from the threshold it hangs on.  No GPU."""
import os
import re

import numpy as np
import pytest

import server_instance_cases as cases
from oracle import oracle
from project_scenarios import BEST
from test_hip_parity import TOL_VS_ORACLE
from test_sw_instance_table import sw_flag_words

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lorikeet_amd", "csrc")
ACCEPTED = [n for names in cases.INSTANCE_NAMES.values() for n in names] + cases.GROUP_NAMES + cases.EDGE_NAMES


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _macro_list(text, name):
    """The X(K) entries of `#define name(X) ...` (continuation lines included)."""
    m = re.search(r"#define\s+%s\(X\)((?:.*\\\n)*.*)\n" % re.escape(name), text)
    assert m, name
    return tuple(int(k) for k in re.findall(r"X\(\s*(\d+)\s*\)", m.group(1)))


def _constant(text, name):
    """`constexpr <type> name = <a>[u] [<< <b>];`"""
    m = re.search(r"const(?:expr)?\s+[\w:]+\s+%s\s*=\s*(\d+)u?(?:\s*<<\s*(\d+))?\s*;" % re.escape(name), text)
    assert m, name
    return int(m.group(1)) << int(m.group(2) or 0)


def test_the_sweep_covers_exactly_the_compiled_instances():
    kernels, host, header, internal = _source("phmm_server_kernels.hip"), _source("phmm_server.cpp"), _source("phmm_server.hpp"), _source("phmm_internal.hpp")
    assert _macro_list(kernels, "PHMM_SRV_FWD_K") == cases.SRV_FWD_K
    assert _macro_list(kernels, "PHMM_SRV_FWD_K32") == cases.SRV_FWD_K32
    assert _macro_list(kernels, "PHMM_SRV_SW_K") == cases.SRV_SW_K
    m = re.search(r"const\s+int\s+kSwKs\[\]\s*=\s*\{([^}]*)\}", host)
    assert m and tuple(int(x) for x in m.group(1).split(",")) == cases.SRV_SW_K
    assert _constant(host, "kMaxHap") == cases.MAX_HAP and _constant(host, "kSwCapacity") == cases.SW_CAPACITY
    assert _constant(header, "SRV_MAX_K") == cases.SRV_MAX_K and _constant(header, "SRV_LDS_BYTES") == cases.SRV_LDS_BYTES
    assert _constant(internal, "LDS_ROW_BYTES") == cases.LDS_ROW_BYTES
    assert "constexpr uint32_t SRV_MAX_ROWS = SRV_LDS_BYTES / LDS_ROW_BYTES - 2;" in header and cases.SRV_MAX_ROWS == 268
    # the tables are what the kernel's three switches go over, with the instances the sweep is named for
    for macro, body in (("PHMM_SRV_FWD_K32", "chain_fwd<32, KK>(job, r, group)"), ("PHMM_SRV_FWD_K", "chain_fwd<16, KK>(job, r, group)"),
                        ("PHMM_SRV_SW_K", "chain_sw<KK>(job, r)")):
        assert re.search(r"case KK: %s; break;\n\s*%s\(PHMM_CASE\)" % (re.escape(body), macro), kernels), macro
    assert "forward_read<L, K>(p, r, (int)group, (int)groups, false, smem, helper_row);" in kernels
    assert "swdev::sw_align_body<64, K, true>(p, smem, r, p.n_alignments, blockIdx.x);" in kernels
    assert "post_best_in_registers<16>(p, r, g, nh);" in kernels and "if (nh <= 16) {" in kernels
    # the rule cases.geometry restates
    assert "const uint32_t fwd_l = max_h <= 16u * SRV_MAX_K ? 16u : 32u, group_haps = 64 / fwd_l;" in host
    assert "const uint32_t fwd_k = std::max<uint32_t>(fwd_l == 16 ? 2 : 13, (max_h + fwd_l - 1) / fwd_l);" in host
    assert "if (!sw_k && (uint32_t)k * 64 >= max_h) sw_k = (uint32_t)k;" in host
    assert len(cases.FORWARD_INSTANCES) == len(set(cases.FORWARD_INSTANCES)) == 28


def test_every_admitted_length_selects_compiled_instances():
    """The `default: break;` hole, closed on paper."""
    compiled = set(cases.FORWARD_INSTANCES)
    for h in range(1, cases.MAX_HAP + 1):
        L, K, sw_k = cases.geometry(h)
        assert (L, K) in compiled and L * K >= h, (h, L, K)
        assert sw_k in cases.SRV_SW_K and 64 * sw_k >= h, (h, sw_k)
    # 16 * SRV_MAX_K and MAX_HAP are where the rule says they are
    assert 16 * cases.SRV_MAX_K == 400 and cases.geometry(400)[:2] == (16, 25) and cases.geometry(401)[:2] == (32, 13)
    assert cases.MAX_HAP == 32 * max(cases.SRV_FWD_K32) == 64 * max(cases.SRV_SW_K) and cases.geometry(cases.MAX_HAP)[:2] == (32, 16)
    assert cases.geometry(cases.MAX_HAP + 1)[2] == 0 and cases.geometry(cases.MAX_HAP + 1)[:2] not in compiled
    # every compiled instance is selected by some length: none is dead code the sweep could not reach
    assert {cases.geometry(h)[:2] for h in range(1, cases.MAX_HAP + 1)} == compiled
    assert {cases.geometry(h)[2] for h in range(1, cases.MAX_HAP + 1)} == set(cases.SRV_SW_K)


def test_every_compiled_instance_is_the_target_of_a_case_at_each_end():
    hit, sw_hit, lengths = {}, set(), set()
    for (L, K), cs in cases.instance_cases().items():
        for c in cs:
            h = cases.max_h(c)
            fl, fk, sk = cases.geometry(h)
            assert (fl, fk) == (L, K), (c.name, h)
            hit.setdefault((fl, fk), []).append(h)
            sw_hit.add(sk)
            lengths.add(h)
    assert set(hit) == set(cases.FORWARD_INSTANCES)
    for (L, K), hs in hit.items():
        lower = 401 if (L, K) == (32, 13) else 1 if (L, K) == (16, 2) else L * (K - 1) + 1
        assert len(hs) >= 2 and min(hs) == lower and max(hs) == L * K, (L, K, hs)
        assert (L, K) == (16, 2) or cases.geometry(lower - 1)[:2] != (L, K)
    assert {16, 17} <= set(hit[(16, 2)])
    assert sw_hit == set(cases.SRV_SW_K)
    assert {128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512} <= lengths      # every boundary of the aligner's table
    assert [cases.geometry(h)[2] for h in (128, 129, 192, 193, 256, 257, 320, 321, 384, 385, 512)] == [2, 3, 3, 4, 4, 5, 5, 6, 6, 8, 8]
    # the group cases: haplotype counts against the wave's slots (64 / lanes) and the post-step's 16 registers
    by_name = {c.name: c for c in cases.group_cases()}
    counts = lambda c: np.diff(c.batch.region_hap_off.astype(np.int64)).tolist()  # noqa: E731
    assert [counts(by_name["haps16-%d" % n]) for n in (1, 4, 5, 8, 9, 16, 17, 33)] == [[1], [4], [5], [8], [9], [16], [17], [33]]
    assert [counts(by_name["haps32-%d" % n]) for n in (1, 2, 3, 5)] == [[1], [2], [3], [5]]
    assert all(cases.geometry(cases.max_h(by_name["haps16-%d" % n]))[:2] == (16, 13) for n in (1, 4, 5, 8, 9, 16, 17, 33))
    assert all(cases.geometry(cases.max_h(by_name["haps32-%d" % n]))[:2] == (32, 15) for n in (1, 2, 3, 5))
    assert counts(by_name["regions-1-9-17"]) == [1, 9, 17]
    two = by_name["regions-40-400"]
    hl = np.diff(two.batch.hap_off.astype(np.int64))
    assert [int(hl[int(two.batch.region_hap_off[g]):int(two.batch.region_hap_off[g + 1])].max()) for g in range(2)] == [40, 400]
    assert cases.geometry(400)[:2] == (16, 25) and cases.geometry(40)[:2] == (16, 3)       # the small region runs in the large one's geometry


# ---- the limits of server_region_submit (phmm_server.cpp), restated ------------------------------------------------------------
def _up(x, to):
    return (x + to - 1) // to * to


SRV_JOB_BYTES = 4096   # (an upper bound of sizeof(SrvJob): five parameter blocks of pointers and words)


def limits(c, out_cigar_slots=cases.OUT_CIGAR_SLOTS):
    """name -> held, for every condition under which the host hands a call to the server."""
    host, api = _source("phmm_server.cpp"), _source("phmm_api.cpp")
    b = c.batch
    ng, nr, nh = b.n_regions, b.n_reads, b.n_haps
    rl, hl = np.diff(b.read_off.astype(np.int64)), np.diff(b.hap_off.astype(np.int64))
    nrg, nhg = np.diff(b.region_read_off.astype(np.int64)), np.diff(b.region_hap_off.astype(np.int64))
    max_r, max_h, max_nh = int(rl.max()), int(hl.max()), int(nhg.max())
    max_hap_cigar = max(len(x) for x in c.hap_cigars)
    gcp = int(c.cfg.constant_gcp)
    sw_k = cases.geometry(max_h)[2]
    ok = {}
    ok["regions"] = ng > 0 and bool((nrg > 0).all() and (nhg > 0).all())
    ok["empty"] = bool(rl.min() >= 1 and hl.min() >= 1)
    ok["out_off"] = int(b.out_off[0]) == 0 and np.array_equal(np.diff(b.out_off.astype(np.int64)), nrg * nhg)
    ok["one_shot"] = ng < 8 or int(b.read_off[-1]) <= _constant(api, "kOneShotBytes")
    ok["rows"] = max_r <= cases.SRV_MAX_ROWS
    ok["hap"] = max_h <= cases.MAX_HAP
    ok["gcp"] = gcp != 0 and 53.0 + max_r * gcp / 10.0 < 590.0
    ok["weights"] = max(abs(x) for x in BEST) * (max_h + max_r + 2) < 100000000
    past = max_h > cases.MAX_HAP or max_r > cases.SRV_MAX_ROWS   # (the host has returned before it looks at what is sized by these two)
    ok["aligner"] = past or sw_k != 0
    lds_group = _up(_up(max_h, 16) + _up(max_r, 16) + 4 * (max_r + 1), 16)
    pj_capacity = 4 * (cases.SW_CAPACITY + max_hap_cigar + 2) + 8
    ok["lds"] = lds_group <= cases.SRV_LDS_BYTES and 16 * pj_capacity <= cases.SRV_LDS_BYTES and _up(max_r + 1, 8) * 17 <= cases.SRV_LDS_BYTES
    ok["slab"] = past or (max(max_h, max_r) + 64) * sw_flag_words(sw_k or 8) * 64 <= (max(cases.MAX_HAP, cases.SRV_MAX_ROWS) + 64) * sw_flag_words(8) * 64
    # the slot: [offset arrays | job record | inputs ... status] staged, then device-only pieces, then results (Layout, phmm_region_internal.hpp)
    used = 0

    def take(n):
        nonlocal used
        used = _up(used, 256) + n
    rb, hb = int(b.read_off[-1]), int(b.hap_off[-1])
    n_hc, n_oc = sum(len(x) for x in c.hap_cigars), sum(len(x) for x in c.orig_cigars)
    for n in (4 * nr, 4 * (ng + 1), 4 * (ng + 1), 4 * (nr + 1), 4 * (nh + 1), 8 * (ng + 1), SRV_JOB_BYTES,
              rb, rb, rb, rb, nr, hb, 4 * ng, 4 * nh, 8 * ng, 4 * (nh + 1), 4 * n_hc, 4 * nh, 4 * (nr + 1), 4 * n_oc, 8 * (nr + 1), 0, 256):
        take(n)
    in_end = _up(used, 256)
    for n in (rb, rb, rb, rb, 8 * nr, 4 * nr, 4 * nr * cases.SW_CAPACITY, 4 * nr, 4 * nr, 4 * nr, 256, nr, 8 * int(b.out_off[-1]), 4 * nr, 8 * nr, 8 * nr,
              4 * nr, 4 * nr, 8 * nr, 4 * out_cigar_slots * nr):
        take(n)
    ok["slot"] = in_end <= _constant(host, "kStageMax") and _up(used, 256) <= _constant(host, "kSlotBytes")
    ok["sync"] = nr <= _constant(host, "kSyncReads") and 8 * nr * _up(max_nh, 8) <= _constant(host, "kSyncHelperBytes")
    return ok


def test_the_restated_limits_are_the_hosts():
    host = _source("phmm_server.cpp")
    for line in ("if (!ng || !nr || !nh) return kServerNotTaken;",
                 "if (ng >= 8 && (size_t)a.read_off[nr] > one_shot_bytes()) return kServerNotTaken;",
                 "if (!nrg || !nhg) return kServerNotTaken;",
                 "if (a.out_off[g + 1] - a.out_off[g] != (uint64_t)nrg * nhg) return kServerNotTaken;",
                 "if (a.out_off[0] != 0) return kServerNotTaken;",
                 "if (!len) return kServerNotTaken;",
                 "if (max_r > SRV_MAX_ROWS || max_h > kMaxHap) return kServerNotTaken;",
                 "if (a.cfg.constant_gcp == 0 || 53.0 + (double)max_r * a.cfg.constant_gcp / 10.0 >= 590.0 || h->sw.no_rescue) return kServerNotTaken;",
                 "if (big * ((int64_t)max_h + max_r + 2) >= 100000000) return kServerNotTaken;",
                 "const size_t lds_ref = (max_h + 15) / 16 * 16, lds_alt = (max_r + 15) / 16 * 16;",
                 "const size_t lds_group = (lds_ref + lds_alt + 4ull * (max_r + 1) + 15) / 16 * 16;",
                 "const uint32_t pj_capacity = 4 * (kSwCapacity + max_hap_cigar + 2) + 8;",
                 "const uint32_t prep_rows = (max_r + 1 + 7) / 8 * 8;",
                 "if (!sw_k || lds_group > SRV_LDS_BYTES || 16ull * pj_capacity > SRV_LDS_BYTES || (size_t)prep_rows * 17 > SRV_LDS_BYTES) return kServerNotTaken;",
                 "if ((size_t)(std::max(max_h, max_r) + 64) * (size_t)sw_flag_words((int)sw_k) * 64 > S->slab_stride) return kServerNotTaken;",
                 "S->slab_stride = (size_t)(std::max<uint32_t>(kMaxHap, SRV_MAX_ROWS) + 64) * (size_t)sw_flag_words(8) * 64;",
                 "const size_t helper_stride = (max_nh + 7) / 8 * 8;",
                 "if (L.in_end > kStageMax || L.end > kSlotBytes || nr > kSyncReads || 8ull * nr * helper_stride > kSyncHelperBytes) return kServerNotTaken;",
                 "S->n_jobs.fetch_add(1, std::memory_order_relaxed);"):
        assert line in host, line


@pytest.mark.parametrize("name", ACCEPTED)
def test_accepted_cases_respect_every_limit(name):
    ok = limits(cases.case(name))
    assert all(ok.values()), [k for k, v in ok.items() if not v]


BROKEN = {"hap-513": "hap", "rows-269": "rows", "gcp21-rows-268": "gcp", "sw-capacity": None}


@pytest.mark.parametrize("name", cases.DECLINED_NAMES)
def test_declined_cases_break_exactly_the_limit_they_are_meant_to(name):
    c = cases.case(name)
    ok = limits(c)
    assert [k for k, v in ok.items() if not v] == ([BROKEN[name]] if BROKEN[name] else [])
    if name in cases.NEIGHBOUR:
        near = cases.case(cases.NEIGHBOUR[name])
        assert all(limits(near).values())
    if name == "hap-513":
        assert cases.max_h(c) == 513 and cases.max_h(near) == 512
    elif name == "rows-269":
        assert cases.max_r(c) == cases.SRV_MAX_ROWS + 1 and cases.max_r(near) == cases.SRV_MAX_ROWS
    elif name == "gcp21-rows-268":
        assert cases.max_r(c) == cases.max_r(near) == 268 and (c.cfg.constant_gcp, near.cfg.constant_gcp) == (21, 20)
        assert 53 + 268 * 2.0 == 589 < 590 <= 53 + 268 * 2.1
    else:
        # taken by the host; the first read's alignment to its best haplotype outgrows the server's 24 elements
        e = cases.expected(c)
        b = c.batch
        assert cases.max_h(c) == 500 and e.keep[0] and e.best[0] == 0 and e.reads[0][0] == 0
        cig, _ = oracle.sw_align(b.hap_bases[:500], b.read_bases[:int(b.read_off[1])], BEST, "SoftClip")
        assert len(cig) > cases.SW_CAPACITY and sum(1 for x in cig if int(x) & 15 == 2) >= 13
        for r in range(1, b.n_reads):       # ... and it is the only one
            hp = int(e.best[r])
            if hp >= 0:
                other, _ = oracle.sw_align(b.hap_bases[int(b.hap_off[hp]):int(b.hap_off[hp + 1])], b.read_bases[int(b.read_off[r]):int(b.read_off[r + 1])], BEST, "SoftClip")
                assert len(other) <= cases.SW_CAPACITY


# ---- how the cases are built ----------------------------------------------------------------------------------------------------
def _cigar_lengths(elems):
    on_hap = sum(int(e) >> 4 for e in elems if int(e) & 15 in (0, 1))     # M, I
    on_ref = sum(int(e) >> 4 for e in elems if int(e) & 15 in (0, 2))     # M, D
    return on_hap, on_ref


@pytest.mark.parametrize("name", cases.all_names())
def test_cases_are_built_as_the_sweep_needs_them(name):
    c = cases.case(name)
    cases.case.cache_clear()
    again = cases.case(name)
    b = c.batch
    assert all(np.array_equal(getattr(b, f), getattr(again.batch, f)) for f in b.FIELDS) and np.array_equal(c.mapq, again.mapq)     # the same bytes every time
    hl, rl = np.diff(b.hap_off.astype(np.int64)), np.diff(b.read_off.astype(np.int64))
    for g in range(b.n_regions):
        h0, h1, r0, r1 = (int(x) for x in (b.region_hap_off[g], b.region_hap_off[g + 1], b.region_read_off[g], b.region_read_off[g + 1]))
        lens, ref_len = hl[h0:h1], int(hl[h0])
        haps = [bytes(b.hap_bases[int(b.hap_off[a]):int(b.hap_off[a + 1])]) for a in range(h0, h1)]
        assert c.ref_hap[g] == 0 and ref_len == lens.max() and len(set(haps)) == len(haps)      # the reference haplotype is the longest; no two are equal
        for a in range(h0, h1):                                          # exact haplotype -> reference CIGARs
            on_hap, on_ref = _cigar_lengths(c.hap_cigars[a])
            assert on_hap == hl[a] and c.hap_starts[a] + on_ref <= ref_len, (g, a)
        if h1 - h0 >= 3 and ref_len >= 8:
            assert lens[1:].min() <= ref_len // 4 and (lens[1:] <= 0.9 * ref_len).sum() >= 2
        if h1 - h0 >= 3 and ref_len >= 24:
            assert any(any(int(e) & 15 in (1, 2) for e in c.hap_cigars[a]) for a in range(h0 + 1, h1))
        assert (rl[r0:r1] >= 1).all() and rl[r0:r1].max() > lens.min() or h1 - h0 < 3     # some reads are longer than some haplotypes
        for r in range(r0, r1):
            assert sum(int(e) >> 4 for e in c.orig_cigars[r] if int(e) & 15 == 0) == rl[r]
    if name.startswith("fwd"):
        assert b.n_regions == 1 and 3 <= b.n_haps <= 5 and b.n_reads == cases.N_READS
        assert rl.min() == 1 and len(set(rl.tolist())) >= 4
    assert any(int(e) & 15 in (4, 5) for r in range(b.n_reads) for e in c.orig_cigars[r])     # clips in the original CIGARs
    assert len(set(c.mapq.tolist())) >= 2 and len(set(b.base_q.tolist())) >= 5



def test_the_edge_cases_hold_their_edges():
    by = {c.name: c for c in cases.edge_cases()}
    assert cases.max_r(by["rows-268"]) == cases.SRV_MAX_ROWS == cases.max_r(by["gcp20-rows-268"]) and by["gcp20-rows-268"].cfg.constant_gcp == 20
    for n in ("rows-268", "gcp20-rows-268"):     # the longest read is read 0, cut whole from a haplotype, kept and projected
        e = cases.expected(by[n])
        assert int(by[n].batch.read_off[1]) == 268 and e.keep[0] and e.reads[0][0] == 0
    assert by["mapq-0"].mapq[0] == 0 and by["mapq-0"].mapq.max() == 60
    cfgs = {(c.cfg.pcr_error_model, c.cfg.dynamic_read_disqualification, c.cfg.symmetrically_normalize_alleles_to_reference)
            for n in ACCEPTED for c in [cases.case(n)]}
    assert {p for p, _, _ in cfgs} == {0, 1, 2, 3} and {(d, s) for _, d, s in cfgs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (0, 1, 1) in cfgs and (3, 0, 0) in cfgs
    # the N cases reach an N: a kept read whose alignment to its best haplotype spans the haplotype's N; a kept, projected read with an N
    c = by["hap-N"]
    b, e = c.batch, cases.expected(c)
    assert (b.hap_bases == ord("N")).sum() == 1 and b.hap_bases[100] == ord("N")
    spans = 0
    for r in range(b.n_reads):
        if e.best[r] == 0 and e.reads[r][0] == 0:
            cig, off = oracle.sw_align(b.hap_bases[:200], b.read_bases[int(b.read_off[r]):int(b.read_off[r + 1])], BEST, "SoftClip")
            spans += off <= 100 < off + _cigar_lengths(cig)[1]
    assert spans >= 2
    c = by["read-N"]
    b, e = c.batch, cases.expected(c)
    with_n = [r for r in range(b.n_reads) if (b.read_bases[int(b.read_off[r]):int(b.read_off[r + 1])] == ord("N")).any()]
    assert len(with_n) >= 2 and not (b.hap_bases == ord("N")).any() and any(e.keep[r] and e.reads[r][0] == 0 for r in with_n)


def test_census_of_what_the_oracle_answers():
    ops, n_reads, n_ok, keeps = set(), 0, 0, set()
    for name in cases.all_names():
        c = cases.case(name)
        e = cases.expected(c)
        b = c.batch
        assert not np.isnan(e.likelihoods).any() and (e.likelihoods <= 0).all(), name
        ok = sum(1 for st, _, _ in e.reads if st == 0)
        assert 3 * ok >= b.n_reads, name                                  # at least a third of every case's reads project
        n_reads, n_ok = n_reads + b.n_reads, n_ok + ok
        keeps |= set(e.keep.tolist())
        for st, _, cig in e.reads:
            ops |= set(re.findall(r"[A-Z]", cig))
        for g in range(b.n_regions):                                      # wherever there is a choice, at least two best alleles occur
            r0, r1 = int(b.region_read_off[g]), int(b.region_read_off[g + 1])
            if b.region_hap_off[g + 1] - b.region_hap_off[g] >= 2:
                assert len(set(e.best[r0:r1].tolist()) - {-1}) >= 2, (name, g)
    assert {"M", "I", "D", "S", "H"} <= ops and keeps == {False, True} and 3 * n_ok >= n_reads


@pytest.mark.parametrize("name", cases.all_names())
def test_every_read_of_every_case_is_far_from_every_threshold(name):
    """A condition on the INPUTS: a difference of TOL_VS_ORACLE in a likelihood flips no discrete output of any read."""
    assert TOL_VS_ORACLE == 1e-9 and cases.MARGIN >= max(1e-6, 1000 * TOL_VS_ORACLE)
    c = cases.case(name)
    per_read = cases.read_margins(c)
    assert len(per_read) == c.batch.n_reads and cases.margins(c) == per_read.min()
    assert (per_read >= cases.MARGIN).all(), (name, np.flatnonzero(per_read < cases.MARGIN), per_read.min())
