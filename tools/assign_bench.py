"""phmm_assign_genotypes on genotype_bench's workloads A (1 024 regions x 128 reads x 8 haplotypes, 4 events each, 1 sample)
and B (10 samples), on the PLs phmm_genotype_likelihoods gives for them; prints one JSON line: per workload and assignment
method the time of the call (host clock around the synchronous call, after warm-up; median and min).  An event of more than
two alleles drops its last one from the call, so the index table does real work.  The kernel's own time comes from a run
under `rocprofv3 --kernel-trace --stats` (phmm_assign_kernel).
usage: python tools/assign_bench.py [--steps K] [--warmup W] [--workloads AB]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genotype_bench import workload  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, _lib, genotype  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="AB")
    a = ap.parse_args()
    eng = HipPairHMMEngine(0)
    out = {"tool": "assign_bench", "steps": a.steps, "warmup": a.warmup}
    for name in a.workloads:
        b, lk, keep, start, end, sample, ev, ploidy, n_samples = workload(name)
        gl = genotype.genotype_likelihoods(eng, b, lk, keep, start, end, sample, ev, ploidy=ploidy, n_samples=n_samples)
        calls = [list(range(ev.n_alleles(e) - (1 if ev.n_alleles(e) > 2 else 0))) for e in range(ev.n_events)]
        lengths = np.ones(int(ev.allele_off[-1]), np.uint32)
        out[name] = {"regions": int(b.n_regions), "events": int(ev.n_events), "samples": n_samples,
                     "call_alleles": int(sum(len(c) for c in calls))}
        for label, method in (("pls", _lib.PHMM_GT_USE_PLS), ("posteriors", _lib.PHMM_GT_USE_POSTERIORS)):
            run = lambda: genotype.assign_genotypes(eng, calls, gl, allele_off=ev.allele_off, allele_length=lengths,  # noqa: E731
                                                    ploidy=ploidy, method=method)
            for _ in range(a.warmup):
                run()
            t = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                res = run()
                t.append(time.perf_counter() - t0)
            out[name].update({label + "_call_ms_median": round(float(np.median(t)) * 1e3, 3), label + "_call_ms_min": round(min(t) * 1e3, 3),
                              label + "_called_samples": int(res.sample_called.sum())})
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
