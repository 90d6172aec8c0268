"""phmm_allele_frequency on five workloads; prints one JSON line: per workload the call time (host clock around the
synchronous call, after warm-up; median and min over the timed calls), events/s and genotype-posterior evaluations/s
(samples x genotypes x (EM iterations + the final pass), summed over the events).
  A  genotype_bench A's 4 096 events (1 024 regions, 1 sample, diploid): their PLs from phmm_genotype_likelihoods
  B  the same with 10 samples
  C  genotype_bench C: ploidy 20, events of at most 3 alleles
  D  the activity-profile shape: 200 000 positions x 16 samples, alleles N / <FAKE_ALT>, diploid (synthetic ref-vs-any PLs)
  E  1 024 events x 500 samples x 4 alleles, diploid, random PLs
Default pseudo counts (genotype.pseudo_counts()), stand_min_conf 30.  The kernel's own time comes from a separate run under
`rocprofv3 --kernel-trace --stats` (kernels phmm_af_kernel<K>).
usage: python tools/af_bench.py [--steps K] [--warmup W] [--workloads ABCDE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import genotype_bench  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, genotype  # noqa: E402


def workload(eng, name, seed=2026):
    """-> pl, pl_off, allele_off, allele_length, n_samples, ploidy"""
    rng = np.random.default_rng(seed)
    if name in "ABC":
        b, lk, keep, start, end, sample, ev, ploidy, n_samples = genotype_bench.workload(name)
        gt = genotype.genotype_likelihoods(eng, b, lk, keep, start, end, sample, ev, ploidy=ploidy, n_samples=n_samples)
        pl = np.concatenate([p.reshape(-1) for p in gt.pl])
        pl_off = np.concatenate([[0], np.cumsum([p.size for p in gt.pl])])
        return pl, pl_off, ev.allele_off, np.ones(int(ev.allele_off[-1]), np.uint32), n_samples, ploidy
    if name == "D":
        n, s = 200000, 16
        het = rng.random((n, s)) < 0.05
        pl = np.stack([np.where(het, rng.integers(10, 400, (n, s)), 0), np.where(het, 0, rng.integers(3, 60, (n, s))),
                       rng.integers(20, 800, (n, s))], axis=2)
        length = np.tile(np.array([1, 0], np.uint32), n)
        return pl.reshape(-1), np.arange(n + 1) * s * 3, np.arange(n + 1) * 2, length, s, 2
    n, s, A = 1024, 500, 4
    g = genotype.genotype_count(2, A)
    pl = rng.integers(0, 300, size=(n, s, g))
    pl[np.arange(n)[:, None], np.arange(s)[None, :], rng.integers(0, g, size=(n, s))] = 0
    return pl.reshape(-1), np.arange(n + 1) * s * g, np.arange(n + 1) * A, np.ones(n * A, np.uint32), s, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workloads", default="ABCDE")
    a = ap.parse_args()
    eng = HipPairHMMEngine(0)
    out = {"tool": "af_bench", "steps": a.steps, "warmup": a.warmup}
    for name in a.workloads:
        pl, pl_off, a_off, length, n_samples, ploidy = workload(eng, name)
        call = lambda: genotype.allele_frequency(eng, pl, pl_off, a_off, length, None, n_samples, ploidy)  # noqa: E731
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = call()
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        n_ev = len(a_off) - 1
        G = np.diff(np.asarray(pl_off, np.int64)) // n_samples
        evals = int(np.sum(G * n_samples * (res.iterations.astype(np.int64) + 1)))
        out[name] = {"events": n_ev, "samples": int(n_samples), "ploidy": int(ploidy), "genotypes": int(G.sum()),
                     "iterations_mean": round(float(res.iterations.mean()), 3), "called": int((res.flags & 1).sum()),
                     "call_ms_median": round(med * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3),
                     "events_per_s": round(n_ev / med), "posterior_evals_per_s": round(evals / med)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
