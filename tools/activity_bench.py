"""phmm_activity_profile on the activity-profile shape of af_bench's workload D; prints one JSON line: per workload the whole
call on the host clock (median and min over the timed calls, staging and copies included), positions, reads, pileup slots.
  A  one window of 200 000 positions x 16 samples, 150-base reads at 30x per sample (40 000 reads a sample), ploidy 2
  B  the same with one sample
Reads: seeded; nine in ten are 150M, the rest carry a leading or trailing soft clip, an insertion or a deletion; 1 % mismatches,
5 % of the bases below the base-quality threshold.  The caller's outputs are asked for (depths, soft-clip mean, is_active_prob,
the profile lists), the per-genotype arrays are not.  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats -- python tools/activity_bench.py --steps 10` (activity_*_kernel beside phmm_af_kernel<1>);
tools/af_bench.py --workloads D in the same session gives the allele-frequency call to read stage 3 against.
usage: python tools/activity_bench.py [--steps K] [--warmup W] [--workloads AB] [--positions N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lorikeet_amd import HipPairHMMEngine, activity  # noqa: E402
from lorikeet_amd.genotype import pseudo_counts  # noqa: E402

READ, DEPTH, START = 150, 30, 1000
CIGARS = ["150M"] * 9 + ["12S138M", "140M10S", "70M2I78M", "70M3D80M", "5S60M1I40M2D44M"]  # the last five: one read in fourteen each


def window(n_pos, n_samples, seed=2026):
    """The packed arrays of one window, built with numpy (lorikeet_amd.activity.pack walks the reads one by one)."""
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), n_pos + 2 * READ)  # from START - READ on: reads may start before the window
    per_sample = n_pos * DEPTH // READ
    enc = [np.array(activity.encode_cigar(c), np.uint32) for c in CIGARS]
    # per template: for every read base the reference offset it is aligned to, -1 for an inserted or clipped base
    maps = []
    for c in enc:
        m, at = [], 0
        for e in c:
            op, n = int(e) & 15, int(e) >> 4
            if op in (0, 7, 8):
                m += list(range(at, at + n))
                at += n
            elif op == 2:
                at += n
            elif op in (1, 4):
                m += [-1] * n
        assert len(m) == READ
        maps.append(np.array(m, np.int64))
    pos, tmpl = [], []
    for _ in range(n_samples):
        pos.append(np.sort(rng.integers(START - READ + 1, START + n_pos, per_sample)))
        tmpl.append(rng.integers(0, len(CIGARS), per_sample))
    pos, tmpl = np.concatenate(pos), np.concatenate(tmpl)
    n_reads = len(pos)
    bases = np.empty((n_reads, READ), np.uint8)
    for t, m in enumerate(maps):
        rows = np.nonzero(tmpl == t)[0]
        idx = (pos[rows] - (START - READ))[:, None] + np.where(m < 0, 0, m)[None, :]
        b = ref[idx]
        b[:, m < 0] = rng.choice(np.frombuffer(b"ACGT", np.uint8), (len(rows), int((m < 0).sum())))
        bases[rows] = b
    flip = rng.random(bases.shape, dtype=np.float32) < 0.01
    bases[flip] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(flip.sum()))
    quals = rng.integers(10, 41, bases.shape, dtype=np.uint8)
    low = rng.random(bases.shape, dtype=np.float32) < 0.05
    quals[low] = rng.integers(2, 10, int(low.sum()), dtype=np.uint8)
    lens = np.array([len(c) for c in enc])[tmpl]
    return dict(n_windows=1, n_samples=n_samples, window_start=np.array([START], np.uint64), window_len=np.array([n_pos], np.uint32),
                window_contig_length=np.array([START + n_pos + 100000], np.uint64), window_ref_off=np.array([0, n_pos], np.uint32),
                ref_bases=np.ascontiguousarray(ref[READ:READ + n_pos]), group_read_off=(np.arange(n_samples + 1) * per_sample).astype(np.uint32),
                read_pos=pos.astype(np.int64), read_cigar_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32),
                read_cigar=np.concatenate([enc[t] for t in tmpl]).astype(np.uint32), read_off=(np.arange(n_reads + 1) * READ).astype(np.uint32),
                read_bases=bases.reshape(-1), read_quals=quals.reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="AB")
    ap.add_argument("--positions", type=int, default=200000)
    a = ap.parse_args()
    eng = HipPairHMMEngine(0)
    out = {"tool": "activity_bench", "steps": a.steps, "warmup": a.warmup}
    omit = ("read_counts", "gl", "pl", "soft_clip_count", "qual", "af_flags")
    for name in a.workloads:
        packed = window(a.positions, 16 if name == "A" else 1)
        call = lambda **kw: activity.activity_profile(eng, packed, ploidy=2, min_base_quality=10, pseudo_counts=pseudo_counts(),  # noqa: E731
                                                      stand_min_conf=30.0, profile_size=0, **kw)
        for _ in range(a.warmup):
            call(omit=omit)
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            res = call(omit=omit)
            ts.append(time.perf_counter() - t0)
        full = call()
        med = float(np.median(ts))
        out[name] = {"positions": a.positions, "samples": packed["n_samples"], "reads": int(len(packed["read_pos"])), "ploidy": 2,
                     "pileup_entries": int(full.read_counts.sum()), "called": int((full.af_flags & 1).sum()),
                     "active_positions": int((res.is_active_prob > 0).sum()), "filter_size": res.filter_size,
                     "profile_len": int(res.profile_len[0]), "staged_mb": round(sum(v.nbytes for v in packed.values() if isinstance(v, np.ndarray)) / 1e6, 1),
                     "call_ms_median": round(med * 1e3, 3), "call_ms_min": round(min(ts) * 1e3, 3), "positions_per_s": round(a.positions / med)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
