"""The launch plan of a fixed set of batches, field by field (phmm_plan_describe: host only, no GPU), against
tests/golden/plan_cases.json -- recorded by tests/golden/make_plan_cases.py before the planner was moved into a unit of its own
(csrc/phmm_plan.cpp), and unchanged by the move.  The cases walk every kind of class the planner makes: the per-read kernel at
64, 32 and 16 lanes per pair, the chained kernel with runs of 4 and of 16 reads, the mixed launches of the ragged set with their
K ranges and 1 / 2 / 4 streams, the f32-first mode, a second caller sharing the GPU, the forced shapes the GPU tests use, the
generic kernel both ways in, and regions with nothing to do."""
import contextlib
import functools
import json
import os

import numpy as np
import pytest

from lorikeet_amd import _lib, synthetic
from lorikeet_amd.engine import plan_describe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_cases.json")
FIELDS = ("cells", "chain_cells", "chain_items", "n_launches", "n_chain_launches", "min_reads_per_run", "swept_cells",
          "pad_column_cells", "pad_slot_cells", "dominant_kernel")   # every field of phmm_plan_info but `reserved`
SWITCHES = ("PHMM_FORCE_L", "PHMM_FORCE_CHAIN", "PHMM_FORCE_STREAMS", "PHMM_TRACE")   # what the planner reads of the environment


class Offsets:   # (what plan_describe reads of a RegionBatch)
    pass


def _empty_regions():
    """Four regions of 24 reads x 3 haplotypes; the second loses its reads, the third its haplotypes."""
    b = synthetic.make_regions(4, 24, 3, 90, [40, 50, 60], seed=1)
    rl = np.diff(b.read_off.astype(np.int64)).reshape(4, 24)
    o = Offsets()
    o.n_regions = 4
    o.region_read_off = np.asarray([0, 24, 24, 48, 72], np.uint32)
    o.region_hap_off = np.asarray([0, 3, 6, 6, 9], np.uint32)
    o.read_off = np.concatenate([[0], np.cumsum(np.concatenate([rl[0], rl[2], rl[3]]))]).astype(np.uint32)
    o.hap_off = (np.arange(10) * 90).astype(np.uint32)
    return o


@functools.lru_cache(maxsize=None)
def _batch(spec):
    kind, args = spec[0], spec[1:]
    if kind == "config2":
        return synthetic.config2(*args)
    if kind == "ragged":
        return synthetic.ragged()
    if kind == "config":
        return synthetic.config(*args)
    if kind == "make_regions":
        n_regions, n_reads, n_haps, hap_len, read_lens, seed = args
        return synthetic.make_regions(n_regions, n_reads, n_haps, hap_len, list(read_lens), seed=seed)
    assert kind == "empty_regions", kind
    return _empty_regions()


def build_batch(spec):
    """spec: the "batch" entry of a case -- [kind, arguments ...] (lists inside become tuples: the batches are made once)."""
    return _batch(tuple(tuple(x) if isinstance(x, list) else x for x in spec))


@contextlib.contextmanager
def planner_environment(env):
    """phmm_plan_describe reads the PHMM_* switches from the environment on every call: exactly `env` of them, then as before."""
    before = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def describe(case):
    """The plan of one case -> {field: value}."""
    flags = _lib.PHMM_FLAG_F32_FIRST if case["f32_first"] else 0
    with planner_environment(case["env"]):
        info = plan_describe(build_batch(case["batch"]), flags=flags, concurrent_callers=case["concurrent_callers"])
    return {f: (info.dominant_kernel.decode() if f == "dominant_kernel" else int(getattr(info, f))) for f in FIELDS}


with open(GOLDEN) as _f:
    CASES = json.load(_f)["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_plan_is_the_recorded_one(case):
    assert set(case["expect"]) == set(FIELDS)
    assert describe(case) == case["expect"]


def test_the_cases_reach_what_they_are_there_for():
    """The kernels and launch counts the set was chosen for (so that a fixture regenerated one day still walks them)."""
    by_name = {c["name"]: c["expect"] for c in CASES}
    kernels = [by_name["config2(%d)" % n]["dominant_kernel"] for n in (1, 2, 8, 32, 128, 1024)]
    assert kernels == ["phmm_forward<64,5>", "phmm_forward<32,10>", "phmm_forward<16,19>", "phmm_forward<16,19>"] + ["phmm_forward_chain_k<16,19>"] * 2
    assert by_name["config2(128)"]["min_reads_per_run"] == 4 and by_name["config2(1024)"]["min_reads_per_run"] == 16
    r = by_name["ragged"]
    assert (r["n_launches"], r["n_chain_launches"], r["chain_items"]) == (8, 6, 70791)
    assert by_name["ragged f32-first"]["n_launches"] == 74 and by_name["ragged callers=8"] == r
    assert by_name["3x24x3 H=300 L=32"]["dominant_kernel"] == "phmm_forward<32,10>"
    assert by_name["3x24x3 H=300 L=32 chain=8"]["dominant_kernel"] == "phmm_forward_chain_k<32,10>"
    assert by_name["generic: read of 2400"]["dominant_kernel"] == by_name["generic: haplotype of 2100"]["dominant_kernel"] == "phmm_forward_generic"
