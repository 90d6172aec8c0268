"""The grow path of the device-only workspaces (DeviceScratch::reserve, lorikeet_amd/csrc/phmm_staging.hpp) under the nine entry
points that keep one on the handle: phmm_discover_events, phmm_trim_regions (which shares the events workspace),
phmm_activity_profile, phmm_finalize_reads, phmm_phase_calls, phmm_assembly_kmers, phmm_assembly_graph (which shares the k-mer
workspace), phmm_assembly_prune and phmm_assembly_recover.

A workspace has no floor: it is 1.5x what the largest call so far needed.  Each case makes an engine of its own and calls the
entry point three times: a small case from the family's builder (the first allocation), the same case COPIES times over in one
call (the workspace is freed and allocated again while the handle is in use), and the small case again (the grown workspace,
reused with the small call's offsets).  Every output array of each of the three calls must equal, byte for byte, what the same
call gives on a fresh engine, the untouched room of the output arrays (filled before the call) included.  No tolerance anywhere.

Why COPIES = 8 always regrows: a workspace of s slots holding R bytes takes at most R + 256 s (every slot is rounded up to 256
bytes), so its capacity after the small call is at most 1.5 (R + 256 s); the large call needs at least 8 R, which is more as
soon as R > 59 s.  The workspaces have at most 40 slots (the graph's), and the small cases here put several kilobytes into each:
tens of haplotypes, reads, events or vertices, every one worth 20 bytes and more of workspace."""
import random

import numpy as np
import pytest

import activity_cases as AK
import assembly_graph_cases as GK
import assembly_kmers_cases as KK
import assembly_prune_cases as PK
import assembly_recover_cases as RK
import assembly_recover_restatement as RR
import events_cases as EK
import finalize_cases as FK
import phase_cases as HK
import region_trim_cases as TK
from lorikeet_amd import activity, assembly, events, finalize, phase, trim
from lorikeet_amd.engine import HipPairHMMEngine

pytestmark = pytest.mark.gpu
COPIES = 8
FILL = 0x5A


def arrays(res, prefix=""):
    """every array of a result -- a dict, a namedtuple, nested -- as {name: bytes, dtype, shape}"""
    if hasattr(res, "_asdict"):
        res = res._asdict()
    out = {}
    for name, v in res.items():
        if isinstance(v, dict) or hasattr(v, "_asdict"):
            out.update(arrays(v, prefix + name + "."))
        elif v is not None:
            v = np.asarray(v)
            out[prefix + name] = (v.tobytes(), str(v.dtype), v.shape)
    return out


def on_fresh_engine(call, case):
    eng = HipPairHMMEngine(0)
    try:
        return arrays(call(eng, case))
    finally:
        eng.close()


def regrow(call, small, large, before=None):
    """small, large, small on one engine (after `before(eng)`, the smaller call of the family the workspace is shared with),
    each against the same call on a fresh engine"""
    eng = HipPairHMMEngine(0)
    try:
        if before is not None:
            before(eng)
        got = [arrays(call(eng, case)) for case in (small, large, small)]
    finally:
        eng.close()
    want_small, want_large = on_fresh_engine(call, small), on_fresh_engine(call, large)
    assert len(want_small) > 1 and any(len(b) for b, _, _ in want_small.values())
    for which, g, w in zip(("first (small)", "second (large)", "third (small)"), got, (want_small, want_large, want_small)):
        assert sorted(g) == sorted(w), which
        for name in w:
            assert g[name][1:] == w[name][1:], (which, name, g[name][1:], w[name][1:])
            assert g[name][0] == w[name][0], (which, name)


def events_call(eng, regions):
    return events.discover_events(eng, regions, 0, True, 2, with_haplotype_events=True, fill=FILL)


def events_regions():
    rng = np.random.default_rng(20240611)
    return [EK.random_region(rng, 120, 8), EK.random_region(rng, 60, 3)]


def test_discover_events():
    regions = events_regions()
    regrow(events_call, regions, regions * COPIES)


def test_trim_regions_after_a_smaller_events_call():
    """(the events call leaves a workspace sized for one region of two short haplotypes; trimming grows it twice)"""
    rng = random.Random(15)
    regions = [TK.seeded_region(rng) for _ in range(2)]
    tiny = [EK.random_region(np.random.default_rng(3), 40, 2)]
    regrow(lambda eng, r: trim.trim_regions(eng, r, 1, TK.SMALL, fill=FILL), regions, regions * COPIES, before=lambda eng: events_call(eng, tiny))


def test_activity_profile():
    windows, o = [AK.seeded_window(100, 1)], AK.options(2, 128)
    regrow(lambda eng, w: activity.activity_profile(eng, w, fill=FILL, **o), windows, windows * COPIES)


def test_finalize_reads():
    _, groups, options = FK.case("pairs")
    groups = groups[:10]
    regrow(lambda eng, g: finalize.finalize_reads(eng, g, fill=FILL, **options), groups, groups * COPIES)


def test_phase_calls():
    S, ploidy = 3, 2

    def call(eng, regions):
        a = HK.pack(regions, S, ploidy, True)
        return phase.phase_calls(eng, a, a["region_hap_off"], a["call_allele_off"], a["call_allele"], a["gt"], S, ploidy, fill=FILL)
    regions = HK.draw_gt([HK.seeded(1), HK.seeded(2)], S, ploidy, 5)
    regrow(call, regions, regions * COPIES)


def kmers_call(eng, c):
    return assembly.assembly_kmers(eng, [(g["ref"], g["reads"]) for g in c["regions"]], c["k"], c["min_q"], fill=FILL)


def test_assembly_kmers():
    c = KK.seeded(3)
    regrow(kmers_call, c, dict(c, regions=c["regions"] * COPIES))


def test_assembly_graph_after_a_smaller_kmers_call():
    """(the k-mer call leaves a workspace sized for one region of three short reads; the graph grows it twice)"""
    c, tiny = GK.seeded(3), KK.calls()["k_longer_than_every_read"]

    def call(eng, c):
        return assembly.assembly_graph(eng, [(g["ref"], g["reads"]) for g in c["regions"]], c["k"], c["min_q"], read_sample=GK.samples_of(c),
                                       num_pruning_samples=c["nps"], fill=FILL)
    regrow(call, c, dict(c, regions=c["regions"] * COPIES), before=lambda eng: kmers_call(eng, tiny))


def test_assembly_prune():
    rng = random.Random(73)
    graphs = [PK.tangled(rng, nv, masks=True) for nv in (17, 64, 130)]

    def call(eng, graphs):
        a = PK.pack(graphs)
        return assembly.prune_graph(eng, a, a["prune_factor"], ops=a["ops"], vertex_absent=a["vertex_absent"], edge_absent=a["edge_absent"], fill=FILL)
    regrow(call, graphs, graphs * COPIES)


def test_assembly_recover():
    cfg = RR.Config(min_dangling_branch_length=1)
    graphs = [RK.tail_of(6, 64), RK.head_of(10), RK.many_tails(3)]

    def call(eng, graphs):
        regions, gd, masks, factor, _ = RK.pack(graphs)
        return assembly.recover_dangling_ends(eng, regions, gd, masks, factor, ops=cfg.ops, min_dangling_branch_length=cfg.min_dangling_branch_length,
                                              min_matching_bases=cfg.min_matching_bases, max_mismatches_in_dangling_head=cfg.max_mismatches_in_dangling_head,
                                              num_pruning_samples=cfg.num_pruning_samples, sw_parameters=cfg.sw, fill=FILL)
    regrow(call, graphs, graphs * COPIES)
