"""Region trimming on the device (phmm_trim_regions, include/phmm.h): the trimmer's spans, every haplotype cut to the padded
span, duplicates folded and the rest in the reference's order, as dense arrays that phmm_region_compute and
phmm_discover_events take as they are."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .engine import PhmmError
from .events import encode_cigar

_i32p = C.POINTER(C.c_int32)
VARIATION_SPAN, VARIATION_SET = 1, 2
FATE_DUPLICATE, FATE_CUT_IN_DELETION, FATE_EMPTY, FATE_ALL_INSERTION, FATE_NOT_TRIMMED = -1, -2, -3, -4, -5
STATUS_LOCATION, STATUS_LENGTH, STATUS_OPERATOR, STATUS_NOT_FOUND, STATUS_BUILDER, STATUS_REF_ELIMINATED, STATUS_REPEAT_SLICE = -16, -17, -18, -19, -20, -21, -22
DEFAULT_PADDING = (20, 75, 75, 25)   # SNP, indel, STR padding; max_extension_into_region_padding (carried, not used)

Region = namedtuple("Region", "ref ref_start active padded haps")
Region.__doc__ = """One assembly region: the padded reference bases (bytes), ref_loc.start, the closed active span and padded span
as (start, end), the haplotypes in the set's insertion order as (bases, cigar, alignment_start_hap_wrt_ref, (loc start, loc end),
is_ref) with the CIGAR a string, a list of (op, length) or BAM-encoded integers."""

INPUTS = (("region_ref_off", np.uint32), ("ref_bases", np.uint8), ("region_ref_start", np.uint64), ("region_active_start", np.uint64),
          ("region_active_end", np.uint64), ("region_padded_start", np.uint64), ("region_padded_end", np.uint64),
          ("region_hap_off", np.uint32), ("hap_off", np.uint32), ("hap_bases", np.uint8), ("hap_cigar_off", np.uint32),
          ("hap_cigar", np.uint32), ("hap_start_wrt_ref", np.uint32), ("hap_loc_start", np.uint64), ("hap_loc_end", np.uint64),
          ("hap_is_ref", np.uint8))
REGION_OUTPUTS = (("region_status", np.int32), ("variation_present", np.uint8), ("variant_start", np.uint64), ("variant_end", np.uint64),
                  ("padded_start", np.uint64), ("padded_end", np.uint64), ("new_active_start", np.uint64), ("new_active_end", np.uint64),
                  ("new_padded_start", np.uint64), ("new_padded_end", np.uint64))
OUTPUTS = REGION_OUTPUTS + (("hap_fate", np.int32), ("hap_dup_of", np.uint32), ("out_region_hap_off", np.uint32), ("out_hap_off", np.uint32),
                            ("out_hap_bases", np.uint8), ("out_hap_cigar_off", np.uint32), ("out_hap_cigar", np.uint32),
                            ("out_hap_start_wrt_ref", np.uint32), ("out_hap_source", np.uint32), ("out_hap_is_ref", np.uint8),
                            ("out_region_ref_hap", np.int32))
_CT = {np.uint8: _lib.u8p, np.uint32: _lib.u32p, np.uint64: _lib.u64p, np.int32: _i32p}


def _p(a, dt):
    return None if a is None else a.ctypes.data_as(_CT[dt])


def pack(regions):
    """The input arrays of phmm_trim_regions for a list of Region (or equal tuples / dicts)."""
    regions = [Region(**r) if isinstance(r, dict) else Region(*r) for r in regions]
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in parts] + [np.zeros(0, dt)]), dt)  # noqa: E731
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)  # noqa: E731
    haps = [h for r in regions for h in r.haps]
    cigars = [encode_cigar(h[1]) for h in haps]
    return dict(
        n_regions=len(regions), region_ref_off=off([len(r.ref) for r in regions]),
        ref_bases=cat([np.frombuffer(bytes(r.ref), np.uint8) for r in regions], np.uint8),
        region_ref_start=np.array([r.ref_start for r in regions], np.uint64),
        region_active_start=np.array([r.active[0] for r in regions], np.uint64),
        region_active_end=np.array([r.active[1] for r in regions], np.uint64),
        region_padded_start=np.array([r.padded[0] for r in regions], np.uint64),
        region_padded_end=np.array([r.padded[1] for r in regions], np.uint64),
        region_hap_off=off([len(r.haps) for r in regions]), hap_off=off([len(h[0]) for h in haps]),
        hap_bases=cat([np.frombuffer(bytes(h[0]), np.uint8) for h in haps], np.uint8), hap_cigar_off=off([len(c) for c in cigars]),
        hap_cigar=cat(cigars, np.uint32), hap_start_wrt_ref=np.array([h[2] for h in haps], np.uint32),
        hap_loc_start=np.array([h[3][0] for h in haps], np.uint64), hap_loc_end=np.array([h[3][1] for h in haps], np.uint64),
        hap_is_ref=np.array([1 if h[4] else 0 for h in haps], np.uint8))


def trim_regions(engine, regions, max_mnp_distance=0, padding=DEFAULT_PADDING, fill=None, omit=()):
    """Trim a batch of regions to their variation (phmm_trim_regions).  regions: a list of Region, or what `pack` returns.
    padding: (SNP, indel, STR, max extension).  fill: a byte the output arrays hold before the call, omit: names of input or
    output arrays passed as NULL (both for tests).  Returns a dict of numpy arrays under the names of include/phmm.h, the dense
    arrays cut to what was written, with n_out; the input arrays under their names.  Raises PhmmError."""
    a = regions if isinstance(regions, dict) else pack(regions)
    n_regions = int(a["n_regions"])
    n_haps = len(a["hap_start_wrt_ref"]) if a.get("hap_start_wrt_ref") is not None else 0
    n_bases = len(a["hap_bases"]) if a.get("hap_bases") is not None else 0
    n_cigar = len(a["hap_cigar"]) if a.get("hap_cigar") is not None else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    size = dict(hap_fate=n_haps, hap_dup_of=n_haps, out_region_hap_off=n_regions + 1, out_hap_off=n_haps + 1, out_hap_bases=n_bases,
                out_hap_cigar_off=n_haps + 1, out_hap_cigar=n_cigar, out_hap_start_wrt_ref=n_haps, out_hap_source=n_haps,
                out_hap_is_ref=n_haps, out_region_ref_hap=n_regions)
    o = {name: new(size.get(name, n_regions), dt) for name, dt in OUTPUTS}
    o.update({k: None for k in omit if k in o})
    i = {name: (None if name in omit or a.get(name) is None else np.ascontiguousarray(a[name], dt)) for name, dt in INPUTS}
    pad = None if "padding" in omit else np.ascontiguousarray(padding, np.uint32)
    ins = [_p(i[name], dt) for name, dt in INPUTS]
    code = engine.lib.phmm_trim_regions(engine._h, n_regions, *ins, int(max_mnp_distance), _p(pad, np.uint32),
                                        *[_p(o[name], dt) for name, dt in OUTPUTS])
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = {k: v for k, v in o.items() if v is not None}
        raise err
    n_out = int(o["out_region_hap_off"][n_regions])
    nb, nc = int(o["out_hap_off"][n_out]), int(o["out_hap_cigar_off"][n_out])
    cut = dict(out_hap_off=n_out + 1, out_hap_cigar_off=n_out + 1, out_hap_bases=nb, out_hap_cigar=nc, out_hap_start_wrt_ref=n_out,
               out_hap_source=n_out, out_hap_is_ref=n_out)
    o["untouched"] = {k: o[k][cut[k]:].copy() for k in cut}   # (tests: what lies behind the written part)
    o.update({k: o[k][:n] for k, n in cut.items()})
    o.update(n_out=n_out, inputs=a)
    return o
