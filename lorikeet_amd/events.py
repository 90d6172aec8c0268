"""Event discovery on the device (phmm_discover_events, include/phmm.h): the haplotypes' event maps, the merged alleles of
every locus and the haplotype -> allele map, under the names the per-event wrappers of lorikeet_amd.genotype take."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .engine import PhmmError

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_OPS = "MIDNSHP=X"

Region = namedtuple("Region", "ref ref_start haps window contig_length")
Region.__doc__ = """One assembly region: the padded reference bases (bytes), ref_loc.start, the haplotypes in order as
(bases, cigar, alignment_start_hap_wrt_ref) with the CIGAR a string, a list of (op, length) or BAM-encoded integers, the closed
active_region_window (start, end), the contig's length."""

EventsResult = namedtuple("EventsResult", "region_event_off region_status event_region event_allele_off event_start event_end "
                          "event_loc vc_start vc_end event_flags event_hap_allele allele_length allele_kind allele_bases_off "
                          "allele_bases required hap_event_off hap_event_start hap_event_end hap_event_ref_length "
                          "hap_event_alt_off hap_event_alt hap_event_type")


def encode_cigar(cigar):
    """A CIGAR as BAM-encoded elements, (length << 4) | op."""
    if isinstance(cigar, str):
        out, n = [], ""
        for ch in cigar:
            if ch.isdigit():
                n += ch
            else:
                out.append((int(n) << 4) | _OPS.index(ch))
                n = ""
        return out
    return [(int(c[1]) << 4) | int(c[0]) if isinstance(c, (tuple, list)) else int(c) for c in cigar]


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def pack(regions):
    """The input arrays of phmm_discover_events for a list of Region (or equal tuples / dicts)."""
    regions = [Region(**r) if isinstance(r, dict) else Region(*r) for r in regions]
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in parts] + [np.zeros(0, dt)]), dt)  # noqa: E731
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)  # noqa: E731
    haps = [h for r in regions for h in r.haps]
    cigars = [encode_cigar(h[1]) for h in haps]
    return dict(
        n_regions=len(regions), region_ref_off=off([len(r.ref) for r in regions]),
        ref_bases=cat([np.frombuffer(bytes(r.ref), np.uint8) for r in regions], np.uint8),
        region_ref_start=np.array([r.ref_start for r in regions], np.uint64),
        region_window_start=np.array([r.window[0] for r in regions], np.uint64),
        region_window_end=np.array([r.window[1] for r in regions], np.uint64),
        region_contig_length=np.array([r.contig_length for r in regions], np.uint64),
        region_hap_off=off([len(r.haps) for r in regions]), hap_off=off([len(h[0]) for h in haps]),
        hap_bases=cat([np.frombuffer(bytes(h[0]), np.uint8) for h in haps], np.uint8), hap_cigar_off=off([len(c) for c in cigars]),
        hap_cigar=cat(cigars, np.uint32), hap_start_wrt_ref=np.array([h[2] for h in haps], np.uint32))


def discover_events(engine, regions, max_mnp_distance=0, include_spanning_events=True, overlap_margin=2, with_haplotype_events=False,
                    capacity=None, fill=None, omit=()):
    """The events of a batch of regions (phmm_discover_events).  regions: a list of Region, or what `pack` returns.  capacity:
    (events, alleles, allele bytes, map entries[, haplotype events, haplotype alt bytes]); None asks the library first (a call
    with capacities 0).  fill: a byte the output arrays are filled with before the call, omit: names of output arrays passed as NULL (both for
    tests).  Raises PhmmError; after
    PHMM_ERR_EVENT_CAPACITY its `required` attribute holds the six sizes."""
    a = regions if isinstance(regions, dict) else pack(regions)
    n_regions, n_haps = a["n_regions"], len(a["hap_start_wrt_ref"])

    def call(cap):
        cap = np.array(list(cap) + [0] * (6 - len(cap)), np.uint32)
        new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
        E, A, B, M, HE, HB = (int(x) for x in cap)
        o = dict(required=new(6, np.uint32), region_event_off=new(n_regions + 1, np.uint32), region_status=new(n_regions, np.int32),
                 event_region=new(E, np.uint32), event_allele_off=new(E + 1, np.uint32), event_start=new(E, np.int64),
                 event_end=new(E, np.int64), event_loc=new(E, np.int64), vc_start=new(E, np.int64), vc_end=new(E, np.int64),
                 event_flags=new(E, np.uint32), event_hap_allele=new(M, np.int32), allele_length=new(A, np.uint32),
                 allele_kind=new(A, np.uint8), allele_bases_off=new(A + 1, np.uint32), allele_bases=new(B, np.uint8))
        names = ("hap_event_off", "hap_event_start", "hap_event_end", "hap_event_ref_length", "hap_event_alt_off", "hap_event_alt", "hap_event_type")
        if with_haplotype_events:
            o.update(hap_event_off=new(n_haps + 1, np.uint32), hap_event_start=new(HE, np.int64), hap_event_end=new(HE, np.int64),
                     hap_event_ref_length=new(HE, np.uint32), hap_event_alt_off=new(HE + 1, np.uint32), hap_event_alt=new(HB, np.uint8),
                     hap_event_type=new(HE, np.uint32))
        else:
            o.update({k: None for k in names})
        o.update({k: None for k in omit})
        code = engine.lib.phmm_discover_events(
            engine._h, n_regions, _p(a["region_ref_off"], _lib.u32p), _p(a["ref_bases"], _lib.u8p), _p(a["region_ref_start"], _lib.u64p),
            _p(a["region_window_start"], _lib.u64p), _p(a["region_window_end"], _lib.u64p), _p(a["region_contig_length"], _lib.u64p),
            _p(a["region_hap_off"], _lib.u32p), _p(a["hap_off"], _lib.u32p), _p(a["hap_bases"], _lib.u8p), _p(a["hap_cigar_off"], _lib.u32p),
            _p(a["hap_cigar"], _lib.u32p), _p(a["hap_start_wrt_ref"], _lib.u32p), int(max_mnp_distance), int(bool(include_spanning_events)),
            int(overlap_margin), _p(cap, _lib.u32p), _p(o["required"], _lib.u32p), _p(o["region_event_off"], _lib.u32p),
            _p(o["region_status"], _i32p), _p(o["event_region"], _lib.u32p), _p(o["event_allele_off"], _lib.u32p),
            _p(o["event_start"], _i64p), _p(o["event_end"], _i64p), _p(o["event_loc"], _i64p), _p(o["vc_start"], _i64p),
            _p(o["vc_end"], _i64p), _p(o["event_flags"], _lib.u32p), _p(o["event_hap_allele"], _i32p), _p(o["allele_length"], _lib.u32p),
            _p(o["allele_kind"], _lib.u8p), _p(o["allele_bases_off"], _lib.u32p), _p(o["allele_bases"], _lib.u8p),
            _p(o["hap_event_off"], _lib.u32p), _p(o["hap_event_start"], _i64p), _p(o["hap_event_end"], _i64p),
            _p(o["hap_event_ref_length"], _lib.u32p), _p(o["hap_event_alt_off"], _lib.u32p), _p(o["hap_event_alt"], _lib.u8p),
            _p(o["hap_event_type"], _lib.u32p))
        return code, o

    if capacity is None:
        code, o = call([0] * 6)
        if code == _lib.PHMM_ERR_EVENT_CAPACITY:
            code, o = call(o["required"])
    else:
        code, o = call(capacity)
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.required = None if o["required"] is None else o["required"].copy()
        err.outputs = {k: v for k, v in o.items() if v is not None}
        raise err
    E, A, B, M, HE, HB = (int(x) for x in o["required"])
    cut = dict(event_region=E, event_allele_off=E + 1, event_start=E, event_end=E, event_loc=E, vc_start=E, vc_end=E, event_flags=E,
               event_hap_allele=M, allele_length=A, allele_kind=A, allele_bases_off=A + 1, allele_bases=B, hap_event_start=HE,
               hap_event_end=HE, hap_event_ref_length=HE, hap_event_alt_off=HE + 1, hap_event_alt=HB, hap_event_type=HE)
    o = {k: (v if v is None or k not in cut else v[:cut[k]]) for k, v in o.items()}
    return EventsResult(**o)
