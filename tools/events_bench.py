"""phmm_discover_events on 1 024 regions of 8 haplotypes over a 300-base reference (random edits: tests/events_cases.py's
generator, seeded), ten calls after warm-up, and beside it phmm_genotype_likelihoods on the events it found (16 reads per
region, 1 sample) so that one kernel trace holds both; prints one JSON line: events, alleles, the whole call on the host
clock (median and min), the genotype call alike.  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/events_bench.py` (events_*_kernel beside phmm_genotype_kernel).
usage: python tools/events_bench.py [--steps K] [--warmup W] [--regions N]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import events_cases as K  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, _lib, events, genotype  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--regions", type=int, default=1024)
    a = ap.parse_args()
    rng = np.random.default_rng(2024)
    packed = events.pack([K.random_region(rng, 300, 8, 0.02) for _ in range(a.regions)])
    eng = HipPairHMMEngine(0)
    need = events.discover_events(eng, packed).required
    run = lambda: events.discover_events(eng, packed, capacity=need[:4])  # noqa: E731
    for _ in range(a.warmup):
        res = run()
    t = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        res = run()
        t.append(time.perf_counter() - t0)
    out = {"tool": "events_bench", "regions": a.regions, "haplotypes": 8, "reference_bases": 300, "steps": a.steps,
           "events": int(need[0]), "alleles": int(need[1]), "allele_bytes": int(need[2]), "failed_regions": int((res.region_status < 0).sum()),
           "call_ms_median": round(float(np.median(t)) * 1e3, 3), "call_ms_min": round(min(t) * 1e3, 3)}
    # the next step on the same events, for scale
    n_reads, n_ev = 16, len(res.event_region)
    read_off = (np.arange(a.regions + 1) * n_reads).astype(np.uint32)
    out_off = (np.arange(a.regions + 1) * n_reads * 8).astype(np.uint64)
    lk = -rng.random(int(out_off[-1])) * 8
    sample = np.zeros(int(read_off[-1]), np.uint32)
    starts = np.repeat(packed["region_ref_start"].astype(np.int64), n_reads)
    ends = starts + 299
    hm = np.concatenate([res.event_hap_allele, [0]]).astype(np.int32)
    G = np.array([genotype.genotype_count(2, int(x)) for x in np.diff(res.event_allele_off)], np.uint64)
    keep = G <= 1024
    assert keep.all(), "an event past the genotype limit: thin the edits"
    gl_off = np.concatenate([[0], np.cumsum(G)]).astype(np.uint64)
    gl, pl = np.zeros(int(gl_off[-1])), np.zeros(int(gl_off[-1]), np.int32)
    p = lambda x, ty: x.ctypes.data_as(ty)  # noqa: E731
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    t = []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        code = eng.lib.phmm_genotype_likelihoods(
            eng._h, a.regions, p(read_off, _lib.u32p), p(packed["region_hap_off"], _lib.u32p), p(out_off, _lib.u64p), p(lk, _lib.f64p), None,
            p(sample, _lib.u32p), p(starts, i64p), p(ends, i64p), 1, 2, n_ev, p(res.event_region, _lib.u32p), p(res.event_allele_off, _lib.u32p),
            p(res.event_start, i64p), p(res.event_end, i64p), p(hm, i32p), p(gl_off, _lib.u64p), p(gl, _lib.f64p), p(pl, i32p), None)
        assert code == _lib.PHMM_OK, eng.last_error()
        if i >= a.warmup:
            t.append(time.perf_counter() - t0)
    out.update({"genotype_call_ms_median": round(float(np.median(t)) * 1e3, 3), "genotype_call_ms_min": round(min(t) * 1e3, 3)})
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
