"""The inputs of the resident region server's instance sweep (tests/test_server_instances_hip.py runs them on the device,
tests/test_server_instance_table.py holds the tables against the sources and the inputs against the oracle alone).

The server (lorikeet_amd/csrc/phmm_server.cpp, phmm_server_kernels.hip) is a second dispatcher over the device bodies, with
instance tables and a selection rule of its own: a call's geometry is a function of its LONGEST haplotype.  Every case here is
one region call built like project_scenarios.scenario with that length under control: a reference haplotype of exactly max_h
bases, variant haplotypes with exact CIGARs (one clearly shorter, one a quarter as long at most), reads cut from them with
errors and clips, qualities spread by test_region_hip._noisy_quals.  numpy and the oracle only: no GPU needed to import it."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from lorikeet_amd.batch import Read, RegionBatch
from oracle import oracle
from project_scenarios import ALPHA, oracle_read, rnd
from test_hip_parity import TOL_VS_ORACLE
from test_region_hip import MODELS, _cfg, _noisy_quals, _oracle_pipeline, _priorities

# ---- the server's tables (test_server_instance_table.py reads them out of the sources) ------------------------------------------
SRV_FWD_K = tuple(range(2, 26))         # PHMM_SRV_FWD_K: forward_read<16, K>
SRV_FWD_K32 = (13, 14, 15, 16)          # PHMM_SRV_FWD_K32: forward_read<32, K>
SRV_SW_K = (2, 3, 4, 5, 6, 8)           # PHMM_SRV_SW_K / kSwKs: sw_align_body<64, K, true>
SRV_MAX_K = 25
MAX_HAP = 512                           # kMaxHap
SRV_LDS_BYTES = 19456
LDS_ROW_BYTES = 72
SRV_MAX_ROWS = SRV_LDS_BYTES // LDS_ROW_BYTES - 2   # 268
SW_CAPACITY = 24                        # kSwCapacity
FORWARD_INSTANCES = [(16, k) for k in SRV_FWD_K] + [(32, k) for k in SRV_FWD_K32]
INFORMATIVE = 0.2                       # LOG_10_INFORMATIVE_THRESHOLD
MARGIN = max(1e-6, 1000 * TOL_VS_ORACLE)  # what margins() has to reach for every case
OUT_CIGAR_SLOTS = 96                    # elements per read the caller reserves: no case needs a second attempt


def geometry(max_h):
    """phmm_server.cpp, server_region_submit: (lanes per pair, columns per lane, rows per lane of the aligner) of a call whose
    longest haplotype has max_h bases.  sw_k = 0: no aligner instance (the host declines)."""
    fwd_l = 16 if max_h <= 16 * SRV_MAX_K else 32
    fwd_k = max(2 if fwd_l == 16 else 13, -(-max_h // fwd_l))
    sw_k = next((k for k in SRV_SW_K if 64 * k >= max_h), 0)
    return fwd_l, fwd_k, sw_k


Case = namedtuple("Case", "name batch mapq hap_cigars hap_starts ref_hap ref_start orig_cigars cfg pri")
CFGS = [dict(pcr=3), dict(pcr=0, dynamic=True), dict(pcr=1, symmetric=False), dict(pcr=2, dynamic=True, symmetric=False)]


def max_h(case):
    return int(np.diff(case.batch.hap_off.astype(np.int64)).max())


def max_r(case):
    return int(np.diff(case.batch.read_off.astype(np.int64)).max())


# ---- one region ---------------------------------------------------------------------------------------------------------------
STRIDE = 12   # every variant haplotype carries an SNV of its own in every STRIDE bases: two haplotypes differ inside any read of 24


def _own_snvs(seg, first_ref_pos, v):
    """Variant v's own SNVs on a stretch copied from the reference: phase v % STRIDE, substituted base by v // STRIDE."""
    for q in range(len(seg)):
        if (first_ref_pos + q) % STRIDE == v % STRIDE:
            seg[q] = ALPHA[(ALPHA.index(seg[q]) + 1 + (v // STRIDE) % 3) % 4]


def _walk(rng, reference, v):
    """project_scenarios.variant_haplotype with variant v's own SNVs: the haplotype and its exact CIGAR against the reference."""
    hap, cigar, i, indels = bytearray(), [], 0, 0
    while i < len(reference):
        u = rng.random() if indels else 0.24 * rng.random()       # (the first chance of an indel is taken)
        step = int(rng.integers(8, 40))
        if i == 0:
            step = min(step, len(reference) // 2)
        d = min(int(rng.integers(1, 7)), len(reference) - i - 1)
        if u < 0.14 and i > 5 and d > 0:
            cigar.append((d, "D"))
            i += d
            indels += 1
        elif u < 0.24 and i > 5:
            k = int(rng.integers(1, 5))
            hap += rnd(rng, k)
            cigar.append((k, "I"))
            indels += 1
        seg = bytearray(reference[i:i + step])
        _own_snvs(seg, i, v)
        hap += seg
        if len(seg):
            cigar.append((len(seg), "M"))
        i += step
    text = "".join("%d%s" % c for c in cigar)
    return bytes(hap), oracle.cigar_builder([text], remove_deletions_at_ends=False)[0] if text else "1M"


def _window(reference, start, length, v):
    seg = bytearray(reference[start:start + length])
    _own_snvs(seg, start, v)
    return bytes(seg), "%dM" % len(seg)


LENGTHS = (1, 24, 63, 64, 65, 110)


def _region(rng, h, n_haps, n_reads, read_lengths=None, hap_n=False, read_n=False):
    """(reads, haplotypes, their CIGARs, their starts, the reads' original CIGARs) of one region whose reference haplotype --
    haplotype 0 -- has exactly h bases and whose other haplotypes are no longer."""
    reference = rnd(rng, h)
    haps, cigs, starts = [reference], ["%dM" % h], [0]
    for v in range(1, n_haps):
        for _ in range(50):
            if h >= 8 and v == 2:                      # at most a quarter as long: a window of the reference
                w = max(1, h // 4 - int(rng.integers(0, 2)))
                s = int(rng.integers(0, h - w + 1))
                hap, cig = _window(reference, s, w, v)
            elif h >= 8 and v == 1:                    # clearly shorter: lanes idle, a partly filled last column
                w = int(h * (0.5 + 0.28 * rng.random()))
                s = int(rng.integers(0, 3))
                hap, cig = _walk(rng, reference[s:s + w], v) if w >= 24 else _window(reference, s, w, v)
            else:
                s = 0
                hap, cig = _walk(rng, reference, v) if h >= 24 else _window(reference, 0, h, v)
                if h < 24:                             # (too short for the own SNVs to tell haplotypes apart: one random SNV more)
                    q = int(rng.integers(0, h))
                    hap = hap[:q] + bytes([ALPHA[(ALPHA.index(reference[q]) + 1 + v) % 4]]) + hap[q + 1:]
            if 1 <= len(hap) <= h and hap not in haps:
                break
        else:
            raise AssertionError("no variant haplotype of at most %d bases" % h)
        haps.append(hap)
        cigs.append(cig)
        starts.append(s)
    if hap_n:
        haps[0] = haps[0][:h // 2] + b"N" + haps[0][h // 2 + 1:]
    lengths = list(read_lengths or ()) + list(LENGTHS) + [min(h, 150)]
    reads, origs = [], []
    for k in range(n_reads):
        n = lengths[k] if k < len(lengths) else lengths[int(rng.integers(0, len(lengths)))]
        exact = read_lengths is not None and k < len(read_lengths)
        fit = [x for x in haps if len(x) >= n] or haps   # (cut from a haplotype that holds the read where there is one)
        src = fit[k % len(fit)]
        if hap_n and src is haps[0]:
            s = max(0, min(len(src) - n, h // 2 - n // 2))   # (across the haplotype's N)
        elif exact:
            s = int(rng.integers(0, max(1, len(src) - n + 1)))
        else:
            s = int(rng.integers(0, max(1, len(src) - n // 2)))   # (some run past their haplotype's end)
        core = bytearray(src[s:s + n])
        if len(core) < n and (exact or rng.random() < 0.5):
            core += rnd(rng, n - len(core))              # a read that runs past its haplotype's end
        if len(core) >= 8 and not exact:
            for _m in range(int(rng.integers(0, 3))):
                q = int(rng.integers(0, len(core)))
                u = rng.random()
                if u < 0.5:
                    core[q] = ALPHA[int(rng.integers(0, 4))]
                elif u < 0.75:
                    core[q:q] = rnd(rng, int(rng.integers(1, 5)))
                else:
                    del core[q:q + int(rng.integers(1, 5))]
        core = bytes(core if exact else core[:SRV_MAX_ROWS]) or b"A"
        if read_n and k % 3 == 1 and len(core) >= 8:
            core = core[:len(core) // 2] + b"N" + core[len(core) // 2 + 1:]
        lh, ls, ts, th = (int(rng.integers(0, 6)) * int(rng.random() < 0.3) for _ in range(4))
        orig = ("%dH" % lh if lh else "") + ("%dS" % ls if ls else "") + "%dM" % len(core) + ("%dS" % ts if ts else "") + ("%dH" % th if th else "")
        m = len(core)
        reads.append(Read(core, np.full(m, 30, np.uint8), np.full(m, 45, np.uint8), np.full(m, 45, np.uint8), np.full(m, 10, np.uint8)))
        origs.append(oracle.parse_cigar(orig))
    return reads, haps, [oracle.parse_cigar(c) for c in cigs], starts, origs


def _assemble(name, regions, cfg_kw, rng, mapq0=False):
    b = RegionBatch.from_regions([(r[0], r[1]) for r in regions])
    hap_cigars = [c for r in regions for c in r[2]]
    hap_starts = [s for r in regions for s in r[3]]
    origs = [c for r in regions for c in r[4]]
    ref_hap = [0] * len(regions)
    ref_start = [int(rng.integers(1, 10 ** 9)) for _ in regions]
    mapq = _noisy_quals(b, int(rng.integers(0, 1 << 31)))
    if mapq0:
        mapq[0] = 0
    return Case(name, b, mapq, hap_cigars, hap_starts, ref_hap, ref_start, origs, _cfg(**cfg_kw), _priorities(b, hap_cigars, ref_hap))


# ---- the case lists: name -> recipe.  SEEDS: the first seed, counted from 0, with which the oracle alone gives the case the
# margins test_server_instance_table.py asks for (a seed that fails is replaced here, no read is ever left out) ----------------
SEEDS = {"fwd16x2-h16": 1, "fwd16x3-h33": 2, "fwd16x4-h49": 1, "fwd16x4-h64": 2, "fwd16x5-h80": 1, "fwd16x6-h81": 3, "fwd16x7-h112": 2, "fwd16x9-h144": 1,
         "fwd16x20-h320": 1, "fwd16x23-h368": 2, "rows-268": 2, "hap-N": 1, "gcp20-rows-268": 8}
N_READS = 12


def _rng(name):
    return np.random.default_rng(zlib.crc32(repr((name, SEEDS.get(name, 0))).encode()))


def _plain(name, regions, cfg_kw=None, mapq0=False, **kw):
    """regions: [(longest haplotype, haplotypes)]"""
    rng = _rng(name)
    cfg_kw = CFGS[zlib.crc32(name.encode()) % len(CFGS)] if cfg_kw is None else cfg_kw
    return _assemble(name, [_region(rng, h, n, kw.pop("n_reads", N_READS), **kw) for h, n in regions], cfg_kw, rng, mapq0)


def instance_lengths(L, K):
    lo = 401 if (L, K) == (32, 13) else L * (K - 1) + 1
    return ([1, 16] if (L, K) == (16, 2) else []) + [lo, L * K]


INSTANCE_NAMES = {(L, K): ["fwd%dx%d-h%d" % (L, K, h) for h in instance_lengths(L, K)] for L, K in FORWARD_INSTANCES}
GROUP_NAMES = ["haps16-%d" % n for n in (1, 4, 5, 8, 9, 16, 17, 33)] + ["haps32-%d" % n for n in (1, 2, 3, 5)] + ["regions-1-9-17", "regions-40-400"]
EDGE_NAMES = ["rows-268", "hap-N", "read-N", "mapq-0", "pcr0-dynamic", "pcr3-asymmetric", "gcp20-rows-268"]
DECLINED_NAMES = ["hap-513", "rows-269", "gcp21-rows-268", "sw-capacity"]
NEIGHBOUR = {"hap-513": "fwd32x16-h512", "rows-269": "rows-268", "gcp21-rows-268": "gcp20-rows-268"}   # each refused case's accepted neighbour


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("fwd"):
        h = int(name.split("-h")[1])
        return _plain(name, [(h, 1 + (2 if h < 8 else 2 + zlib.crc32(name.encode()) % 3))])   # two to four variants (two where all are short)
    if name.startswith("haps16-"):
        return _plain(name, [(200, int(name[7:]))])
    if name.startswith("haps32-"):
        return _plain(name, [(450, int(name[7:]))])
    if name == "regions-1-9-17":
        return _plain(name, [(200, 1), (180, 9), (150, 17)], n_reads=7)
    if name == "regions-40-400":
        return _plain(name, [(40, 3), (400, 3)], n_reads=8)
    if name in ("rows-268", "rows-269"):
        return _plain(name, [(300, 3)], cfg_kw=dict(pcr=3), read_lengths=[int(name[5:])])
    if name in ("gcp20-rows-268", "gcp21-rows-268"):
        return _plain(name, [(300, 3)], cfg_kw=dict(pcr=1, gcp=int(name[3:5])), read_lengths=[268])
    if name == "hap-N":
        return _plain(name, [(200, 3)], cfg_kw=dict(pcr=2), hap_n=True)
    if name == "read-N":
        return _plain(name, [(200, 3)], cfg_kw=dict(pcr=3, dynamic=True), read_n=True)
    if name == "mapq-0":
        return _plain(name, [(120, 3)], cfg_kw=dict(pcr=1), mapq0=True)
    if name == "pcr0-dynamic":
        return _plain(name, [(257, 4)], cfg_kw=dict(pcr=0, dynamic=True, symmetric=True))
    if name == "pcr3-asymmetric":
        return _plain(name, [(129, 4)], cfg_kw=dict(pcr=3, dynamic=False, symmetric=False))
    if name == "hap-513":
        return _plain(name, [(513, 3)], cfg_kw=dict(pcr=3))
    if name == "sw-capacity":
        return _sw_capacity_case(name)
    raise KeyError(name)


def _sw_capacity_case(name):
    """A read of a 500-base haplotype with fourteen one-base deletions, 18 bases apart: its alignment has 29 elements."""
    rng = _rng(name)
    reads, haps, cigs, starts, origs = _region(rng, 500, 2, 6)
    read = b"".join(haps[0][20 + 18 * k:20 + 18 * k + 17] for k in range(15))
    m = len(read)
    reads[0] = Read(read, np.full(m, 30, np.uint8), np.full(m, 45, np.uint8), np.full(m, 45, np.uint8), np.full(m, 10, np.uint8))
    origs[0] = oracle.parse_cigar("%dM" % m)
    # (a threshold that keeps a read with fourteen deletions: test_region_hip.test_alignments_that_outgrow_the_library_slots_are_redone)
    return _assemble(name, [(reads, haps, cigs, starts, origs)], dict(pcr=0, cap=-1000.0, dynamic=True, err=1.0), rng)


def instance_cases():
    return {key: [case(n) for n in names] for key, names in INSTANCE_NAMES.items()}


def group_cases():
    return [case(n) for n in GROUP_NAMES]


def edge_cases():
    return [case(n) for n in EDGE_NAMES]


def declined_cases():
    return [case(n) for n in DECLINED_NAMES]


def all_names():
    return [n for names in INSTANCE_NAMES.values() for n in names] + GROUP_NAMES + EDGE_NAMES + DECLINED_NAMES


def region_of_reads(b):
    return np.repeat(np.arange(b.n_regions), np.diff(b.region_read_off.astype(np.int64)))


def split(c):
    """Every region of a call as a call of its own."""
    b, out = c.batch, []
    for g in range(b.n_regions):
        r0, r1, h0, h1 = (int(x) for x in (b.region_read_off[g], b.region_read_off[g + 1], b.region_hap_off[g], b.region_hap_off[g + 1]))
        out.append(Case("%s[%d]" % (c.name, g), b.region_slice(g, g + 1), c.mapq[r0:r1].copy(), c.hap_cigars[h0:h1], c.hap_starts[h0:h1], [c.ref_hap[g]],
                        [c.ref_start[g]], c.orig_cigars[r0:r1], c.cfg, c.pri[h0:h1].copy()))
    return out


# ---- the oracle's answer -----------------------------------------------------------------------------------------------------
Expected = namedtuple("Expected", "likelihoods keep best reads")
_expected = {}


def expected(c):
    """test_region_hip._oracle_pipeline (likelihoods, keep, best allele) and project_scenarios.oracle_read (status, position,
    CIGAR string of every read); once per process and case."""
    if c.name not in _expected:
        b = c.batch
        out, keep, best = _oracle_pipeline(c.cfg, b, c.mapq, c.ref_hap, c.pri)
        reg = region_of_reads(b)
        reads = [oracle_read(b, r, reg[r], best[r], c.hap_cigars, c.hap_starts, c.ref_hap, c.ref_start, c.orig_cigars) for r in range(b.n_reads)]
        for a in (out, keep, best):
            a.setflags(write=False)
        _expected[c.name] = Expected(out, keep, best, reads)
    return _expected[c.name]


def oracle_cells(c):
    return c.batch.cells()


def _raw(c, g):
    """The oracle's raw [allele][read] likelihoods and per-read thresholds of region g (what _oracle_pipeline normalises)."""
    b, cfg = c.batch, c.cfg
    r0, r1, h0, h1 = (int(x) for x in (b.region_read_off[g], b.region_read_off[g + 1], b.region_hap_off[g], b.region_hap_off[g + 1]))
    reads, thr = [], []
    for r in range(r0, r1):
        s, e = int(b.read_off[r]), int(b.read_off[r + 1])
        q, i, d = oracle.modify_read_qualities(MODELS[cfg.pcr_error_model], b.read_bases[s:e], int(c.mapq[r]), b.base_q[s:e], b.ins_q[s:e], b.del_q[s:e],
                                               cfg.base_quality_score_threshold, bool(cfg.disable_cap_read_qualities_to_mapq))
        reads.append(Read(b.read_bases[s:e], q, i, d, np.full(e - s, cfg.constant_gcp, np.uint8)))
        thr.append(oracle.read_disqualification_threshold(b.base_q[s:e], bool(cfg.dynamic_read_disqualification), cfg.read_disqualification_scale,
                                                          cfg.expected_error_rate_per_base))
    haps = [b.hap_bases[int(b.hap_off[a]):int(b.hap_off[a + 1])] for a in range(h0, h1)]
    rb = RegionBatch.from_regions([(reads, haps)])
    return oracle.compute_batch(rb.as_dict(), n_threads=4).reshape(r1 - r0, h1 - h0).T.copy(), np.array(thr)


def read_margins(c):
    """Per read, the smallest distance between the oracle's numbers and a threshold that a discrete output hangs on:
      * the filter: the read's best normalised likelihood against its disqualification threshold;
      * the normalisation: every raw likelihood against the cap (best + log10_global_read_mismapping_rate);
      * the best allele: (best - other) against the informative threshold 0.2 for every other allele, and -- where several
        alleles within 0.2 of the best share the highest priority, so that the one the scan met first stays -- best minus the
        best of the winner's rivals against 0 (a tie)."""
    b, cfg = c.batch, c.cfg
    cap, symmetric = cfg.log10_global_read_mismapping_rate, bool(cfg.symmetrically_normalize_alleles_to_reference)
    out = np.full(b.n_reads, np.inf)
    best = expected(c).best
    for g in range(b.n_regions):
        r0, h0, h1 = int(b.region_read_off[g]), int(b.region_hap_off[g]), int(b.region_hap_off[g + 1])
        raw, thr = _raw(c, g)
        pri = np.asarray(c.pri[h0:h1])
        na = raw.shape[0]
        norm = oracle.normalize_likelihoods(raw.copy(), cap, symmetric, c.ref_hap[g])
        for k in range(raw.shape[1]):
            v, m = norm[:, k], float(norm[:, k].max())
            ds = [abs(m - thr[k])]
            if na >= 2:
                top = float(np.delete(raw[:, k], c.ref_hap[g]).max()) if not symmetric else float(raw[:, k].max())
                ds += [abs(x - (top + cap)) for x in raw[:, k]]
                first = int(np.argmax(v))
                ds += [abs((m - v[a]) - INFORMATIVE) for a in range(na) if a != first]
                close = [a for a in range(na) if m - v[a] < INFORMATIVE]
                tops = [a for a in close if pri[a] == pri[close].max()]
                if len(tops) > 1:
                    winner = int(best[r0 + k]) if best[r0 + k] >= 0 else (first if first in tops else tops[0])
                    ds.append(m - max(v[a] for a in tops if a != winner))
            out[r0 + k] = min(ds)
    return out


def margins(c):
    return float(read_margins(c).min())
