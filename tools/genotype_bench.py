"""phmm_genotype_likelihoods on three workloads; prints one JSON line: per workload the call time (host clock around the
synchronous call, after warm-up; median and min over the timed calls), events/s and regions/s.
  A  1 024 regions x 128 reads x 8 haplotypes, the first 4 events of each region, 1 sample, ploidy 2
  B  the same with 10 samples
  C  ploidy 20, events of at most 3 alleles
The likelihood matrices are random (what the call costs does not depend on their values); the events are those of the
synthetic haplotypes (synthetic.make_events), the reads span 150 reference bases at random offsets.  The kernel's own time
comes from a separate run under `rocprofv3 --kernel-trace --stats` (kernel phmm_genotype_kernel).
usage: python tools/genotype_bench.py [--steps K] [--warmup W] [--workloads ABC]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lorikeet_amd import HipPairHMMEngine, genotype, synthetic  # noqa: E402


def workload(name, n_regions=1024, n_reads=128, n_haps=8, hap_len=300, read_len=150, per_region=4, seed=2026):
    b = synthetic.make_regions(n_regions, n_reads, n_haps, hap_len, read_len, seed=seed)
    ev = synthetic.make_events(b)
    ploidy, n_samples, max_alleles = {"A": (2, 1, None), "B": (2, 10, None), "C": (20, 1, 3)}[name]
    nh = np.diff(b.region_hap_off.astype(np.int64))[ev.region.astype(np.int64)]
    moff = np.concatenate([[0], np.cumsum(nh)])
    n_al = np.diff(ev.allele_off.astype(np.int64))
    pick, seen = [], {}
    for e in range(ev.n_events):
        g = int(ev.region[e])
        if (max_alleles is None or n_al[e] <= max_alleles) and seen.get(g, 0) < per_region:
            seen[g] = seen.get(g, 0) + 1
            pick.append(e)
    pick = np.asarray(pick)
    ev = genotype.Events(ev.region[pick], np.concatenate([[0], np.cumsum(n_al[pick])]), ev.start[pick], ev.end[pick],
                         np.concatenate([ev.hap_allele[moff[e]:moff[e + 1]] for e in pick]))
    rng = np.random.default_rng(seed)
    lk = -np.abs(rng.normal(0.0, 3.0, size=b.n_out))
    start = rng.integers(0, hap_len - read_len + 1, size=b.n_reads).astype(np.int64)
    sample = rng.integers(0, n_samples, size=b.n_reads).astype(np.uint32)
    keep = (rng.random(b.n_reads) > 0.02).astype(np.uint8)
    return b, lk, keep, start, start + read_len - 1, sample, ev, ploidy, n_samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="ABC")
    a = ap.parse_args()
    eng = HipPairHMMEngine(0)
    out = {"tool": "genotype_bench", "steps": a.steps, "warmup": a.warmup}
    for name in a.workloads:
        b, lk, keep, start, end, sample, ev, ploidy, n_samples = workload(name)
        call = lambda: genotype.genotype_likelihoods(eng, b, lk, keep, start, end, sample, ev, ploidy=ploidy, n_samples=n_samples)  # noqa: E731
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = call()
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        out[name] = {"regions": int(b.n_regions), "events": int(ev.n_events), "samples": n_samples, "ploidy": ploidy,
                     "genotypes": int(sum(g.shape[1] for g in res.gl)), "reads_used": int(res.n_evidence.sum()),
                     "call_ms_median": round(med * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3),
                     "events_per_s": round(ev.n_events / med), "regions_per_s": round(b.n_regions / med)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
