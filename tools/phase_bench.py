"""phmm_phase_calls on events_bench's workload -- 1 024 regions of 8 haplotypes over a 300-base reference (random edits:
tests/events_cases.py's generator, seeded) -- with every event called with all its alleles, one sample at ploidy 2; ten calls
after warm-up, and beside it phmm_assign_genotypes on the same events (seeded PLs), whose GT the phasing call reads, so that one
kernel trace holds both; prints one JSON line: events, phased calls, groups, aborted regions, the whole call on the host clock
(median and min), the assignment call alike.  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/phase_bench.py` (phase_*_kernel beside phmm_assign_kernel).
usage: python tools/phase_bench.py [--steps K] [--warmup W] [--regions N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import events_cases as K  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, events, genotype, phase  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=1024)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    packed = events.pack([K.random_region(rng, 300, 8, 0.02) for _ in range(a.regions)])
    eng = HipPairHMMEngine(0)
    ev = events.discover_events(eng, packed, with_haplotype_events=True)
    n_ev = len(ev.vc_start)
    A = np.diff(ev.event_allele_off.astype(np.int64))
    calls = [list(range(int(x))) for x in A]
    # the step before, on the same events, for scale and for its GT: seeded PLs, the best genotype at 0
    # (an event of one allele -- the reference alone -- is no input of the assignment: it stands there with two, and its GT is 0)
    A2 = np.maximum(A, 2)
    G = np.array([genotype.genotype_count(2, int(x)) for x in A2], np.int64)
    assert (G <= 1024).all(), "an event past the genotype limit: thin the edits"
    pl_off = np.concatenate([[0], np.cumsum(G)]).astype(np.uint64)
    pl = rng.integers(1, 200, int(pl_off[-1])).astype(np.int32)
    pl[pl_off[:-1].astype(np.int64) + rng.integers(0, G)] = 0
    calls2 = [list(range(int(x))) for x in A2]
    allele_off2 = np.concatenate([[0], np.cumsum(A2)]).astype(np.uint32)
    t_assign = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        asg = genotype.assign_genotypes(eng, calls2, pl, allele_off2, pl_off, n_samples=1, ploidy=2)
        if i >= a.warmup:
            t_assign.append(time.perf_counter() - t0)
    call_allele_off = np.concatenate([[0], np.cumsum(A)]).astype(np.uint32)
    call_allele = np.array([x for c in calls for x in c], np.uint32)
    gt = np.ascontiguousarray(asg.gt, np.int32)
    gt[A < 2] = 0
    run = lambda: phase.phase_calls(eng, ev, packed["region_hap_off"], call_allele_off, call_allele, gt, 1, 2)  # noqa: E731
    t = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        res = run()
        if i >= a.warmup:
            t.append(time.perf_counter() - t0)
    out = {"tool": "phase_bench", "regions": a.regions, "haplotypes": 8, "reference_bases": 300, "steps": a.steps, "events": n_ev,
           "haplotype_events": len(ev.hap_event_start), "calls_with_haplotypes": int((res.phase_n_haps > 0).sum()),
           "phased_calls": int((res.phase_group >= 0).sum()), "groups": int(sum(len(set(res.phase_group[s:e][res.phase_group[s:e] >= 0].tolist()))
                                                                                for s, e in zip(ev.region_event_off[:-1], ev.region_event_off[1:]))),
           "aborted_regions": int((res.region_phase_flags != 0).sum()), "reversed_genotypes": int((res.gt_phased != gt).any(axis=2).sum()),
           "call_ms_median": round(float(np.median(t)) * 1e3, 3), "call_ms_min": round(min(t) * 1e3, 3),
           "assign_call_ms_median": round(float(np.median(t_assign)) * 1e3, 3), "assign_call_ms_min": round(min(t_assign) * 1e3, 3),
           "staged_in_bytes": int(sum(np.asarray(getattr(ev, k)).nbytes for k in phase.INPUTS) + call_allele.nbytes + call_allele_off.nbytes + gt.nbytes)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
