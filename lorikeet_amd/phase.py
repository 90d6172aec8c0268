"""Physical phasing on the device (phmm_phase_calls, include/phmm.h): reverse_trim_alleles, the called haplotypes and
phase_calls for the called events of many regions, on the arrays lorikeet_amd.events.discover_events returns and the
call lists and GT lorikeet_amd.genotype's wrappers take and return."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .engine import PhmmError

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)

# what the call reads of a discover_events result (with_haplotype_events=True), beside region_hap_off
INPUTS = ("region_event_off", "event_allele_off", "event_hap_allele", "vc_start", "allele_length", "allele_kind", "allele_bases_off",
          "allele_bases", "hap_event_off", "hap_event_start", "hap_event_alt_off", "hap_event_alt")
OUTPUTS = ("call_rev_trim", "call_end", "phase_n_haps", "hap_in_call", "phase_group", "phase_gt", "phase_leader", "phase_set",
           "region_alt_haps", "region_phase_flags", "is_phased", "gt_phased")
PhaseResult = namedtuple("PhaseResult", OUTPUTS)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def phase_calls(engine, events, region_hap_off, call_allele_off, call_allele, gt=None, n_samples=0, ploidy=0, trim=True,
                fill=None, omit=()):
    """The phased calls of a batch of regions (phmm_phase_calls).  events: a discover_events result with its per-haplotype event
    maps, or a dict with the arrays named in INPUTS; region_hap_off: the haplotype offsets that call was given; call_allele_off,
    call_allele: the calls as annotate_events takes them; gt [n_events x n_samples x ploidy]: assign_genotypes' gt, None skips
    the genotype stage (is_phased and gt_phased are then None).  trim=False: no call is trimmed.  fill: a byte the output arrays
    are filled with before the call, omit: names of output arrays passed as NULL (both for tests).  Raises PhmmError."""
    a = events if isinstance(events, dict) else events._asdict()
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32)  # noqa: E731
    region_event_off, region_hap_off = u32(a["region_event_off"]), u32(region_hap_off)
    n_regions = next((len(x) - 1 for x in (region_event_off, region_hap_off) if x is not None), 0)
    # (the sizes of the outputs; with an offset array missing or broken -- the library refuses those -- any size will do)
    n_events = int(region_event_off[-1]) if n_regions and region_event_off is not None else 0
    n_map = 0
    if n_regions and region_event_off is not None and region_hap_off is not None:
        n_map = max(int(np.sum(np.diff(region_event_off.astype(np.int64)) * np.diff(region_hap_off.astype(np.int64)))), 0)
    as_ = lambda k, dt: None if a.get(k) is None else np.ascontiguousarray(a[k], dt)  # noqa: E731
    i = dict(event_allele_off=as_("event_allele_off", np.uint32), event_hap_allele=as_("event_hap_allele", np.int32),
             vc_start=as_("vc_start", np.int64), allele_length=as_("allele_length", np.uint32), allele_kind=as_("allele_kind", np.uint8),
             allele_bases_off=as_("allele_bases_off", np.uint32), allele_bases=as_("allele_bases", np.uint8),
             hap_event_off=as_("hap_event_off", np.uint32), hap_event_start=as_("hap_event_start", np.int64),
             hap_event_alt_off=as_("hap_event_alt_off", np.uint32), hap_event_alt=as_("hap_event_alt", np.uint8))
    call_allele_off, call_allele = u32(call_allele_off), u32(call_allele)
    if gt is not None:
        gt = np.ascontiguousarray(gt, np.int32).reshape(-1)
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    o = dict(call_rev_trim=new(n_events, np.uint32), call_end=new(n_events, np.int64), phase_n_haps=new(n_events, np.uint32),
             hap_in_call=new(n_map, np.uint8), phase_group=new(n_events, np.int32), phase_gt=new(n_events, np.uint8),
             phase_leader=new(n_events, np.int32), phase_set=new(n_events, np.int64), region_alt_haps=new(n_regions, np.uint32),
             region_phase_flags=new(n_regions, np.uint32),
             is_phased=None if gt is None else new(n_events * n_samples, np.uint8),
             gt_phased=None if gt is None else new(n_events * n_samples * ploidy, np.int32))
    o.update({k: None for k in omit})
    code = engine.lib.phmm_phase_calls(
        engine._h, n_regions, _p(region_event_off, _lib.u32p), _p(region_hap_off, _lib.u32p), _p(i["event_allele_off"], _lib.u32p),
        _p(i["event_hap_allele"], _i32p), _p(i["vc_start"], _i64p), _p(i["allele_length"], _lib.u32p), _p(i["allele_kind"], _lib.u8p),
        _p(i["allele_bases_off"], _lib.u32p), _p(i["allele_bases"], _lib.u8p), _p(i["hap_event_off"], _lib.u32p),
        _p(i["hap_event_start"], _i64p), _p(i["hap_event_alt_off"], _lib.u32p), _p(i["hap_event_alt"], _lib.u8p),
        _p(call_allele_off, _lib.u32p), _p(call_allele, _lib.u32p), int(n_samples), int(ploidy), _p(gt, _i32p),
        0 if trim else _lib.PHMM_PH_NO_TRIM, _p(o["call_rev_trim"], _lib.u32p), _p(o["call_end"], _i64p), _p(o["phase_n_haps"], _lib.u32p),
        _p(o["hap_in_call"], _lib.u8p), _p(o["phase_group"], _i32p), _p(o["phase_gt"], _lib.u8p), _p(o["phase_leader"], _i32p),
        _p(o["phase_set"], _i64p), _p(o["region_alt_haps"], _lib.u32p), _p(o["region_phase_flags"], _lib.u32p),
        _p(o["is_phased"], _lib.u8p), _p(o["gt_phased"], _i32p))
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = {k: v for k, v in o.items() if v is not None}
        raise err
    if gt is not None:
        o["is_phased"] = None if o["is_phased"] is None else o["is_phased"].reshape(n_events, n_samples)
        o["gt_phased"] = None if o["gt_phased"] is None else o["gt_phased"].reshape(n_events, n_samples, ploidy)
    return PhaseResult(**o)
