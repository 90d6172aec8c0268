"""A region's reads finalized on the device (phmm_finalize_reads, include/phmm.h): soft clips, low-quality tails, adaptor, the
clip to the padded span, the filter, and the base qualities of overlapping mates."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .activity import encode_cigar
from .engine import PhmmError

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)

Group = namedtuple("Group", "span reads")
Group.__doc__ = """One (region, sample): the padded span (start, end) as the reference holds it, and the reads as dicts (or equal
tuples) of pos, flags, mapq, mpos, isize, cigar (a string, (op, length) pairs or BAM-encoded integers), bases, quals, mate: the
index INSIDE the group of the other read with the same name, -1 for none."""
READ_FIELDS = ("pos", "flags", "mapq", "mpos", "isize", "cigar", "bases", "quals", "mate")

FinalizeResult = namedtuple("FinalizeResult", "read_status keep new_pos out_unmapped clip_first clip_len out_cigar n_out_cigar "
                            "unclipped_len lead_soft trail_soft out_quals out_cigar_off read_off")
FinalizeResult.__doc__ = """The outputs of phmm_finalize_reads (None where omitted), with out_cigar_off and read_off, the layouts
of out_cigar and out_quals."""
FinalizeResult.cigar = lambda self, r: self.out_cigar[int(self.out_cigar_off[r]):int(self.out_cigar_off[r]) + int(self.n_out_cigar[r])]
FinalizeResult.quals = lambda self, r: self.out_quals[int(self.read_off[r]):int(self.read_off[r + 1])]

OUTPUTS = ("read_status", "keep", "new_pos", "out_unmapped", "clip_first", "clip_len", "out_cigar", "n_out_cigar", "unclipped_len",
           "lead_soft", "trail_soft", "out_quals")


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def pack(groups):
    """The input arrays of phmm_finalize_reads for a list of Group (or equal tuples / dicts)."""
    groups = [Group(**g) if isinstance(g, dict) else Group(*g) for g in groups]
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in parts] + [np.zeros(0, dt)]), dt)  # noqa: E731
    off = lambda lens, dt=np.uint32: np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(dt)  # noqa: E731
    reads, mate, at = [], [], 0
    for g in groups:
        for r in g.reads:
            r = r if isinstance(r, dict) else dict(zip(READ_FIELDS, r))
            reads.append(r)
            m = int(r.get("mate", -1))
            mate.append(at + m if m >= 0 else -1)
        at += len(g.reads)
    cigars = [encode_cigar(r["cigar"]) for r in reads]
    col = lambda k, dt: np.array([r[k] for r in reads], dt)  # noqa: E731
    return dict(
        n_groups=len(groups), group_read_off=off([len(g.reads) for g in groups]),
        group_span_start=np.array([g.span[0] for g in groups], np.uint64), group_span_end=np.array([g.span[1] for g in groups], np.uint64),
        read_pos=col("pos", np.int64), read_flags=col("flags", np.uint16), read_mapq=col("mapq", np.uint8), read_mpos=col("mpos", np.int64),
        read_isize=col("isize", np.int64), read_cigar_off=off([len(c) for c in cigars]), read_cigar=cat(cigars, np.uint32),
        read_off=off([len(r["bases"]) for r in reads]), read_bases=cat([np.frombuffer(bytes(r["bases"]), np.uint8) for r in reads], np.uint8),
        read_quals=cat([np.asarray(list(r["quals"]), np.uint8) for r in reads], np.uint8), mate_index=np.array(mate, np.int32),
        out_cigar_off=off([len(c) + 2 for c in cigars], np.uint64))


def finalize_reads(engine, groups, steps=_lib.PHMM_FIN_ALL, min_tail_quality=9, dont_use_soft_clipped_bases=False,
                   half_of_pcr_snv_qual=20, fill=None, omit=()):
    """The reads of a batch of groups finalized.  groups: a list of Group, or what `pack` returns (an array set to None goes as
    NULL).  fill: a byte the output arrays hold before the call, omit: names of outputs passed as NULL (both for tests).  Raises
    PhmmError (its `outputs` attribute holds the arrays as the call left them)."""
    a = groups if isinstance(groups, dict) else pack(groups)
    n = int(a["group_read_off"][-1]) if a.get("group_read_off") is not None and len(a["group_read_off"]) else 0
    n_bases = int(a["read_off"][-1]) if a.get("read_off") is not None and len(a["read_off"]) else 0
    n_out = int(a["out_cigar_off"][-1]) if a.get("out_cigar_off") is not None and len(a["out_cigar_off"]) else 1
    new = lambda k, dt: np.zeros(k, dt) if fill is None else np.frombuffer(bytes([fill]) * (k * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    o = dict(read_status=new(n, np.int32), keep=new(n, np.uint8), new_pos=new(n, np.int64), out_unmapped=new(n, np.uint8),
             clip_first=new(n, np.uint32), clip_len=new(n, np.uint32), out_cigar=new(n_out, np.uint32), n_out_cigar=new(n, np.uint32),
             unclipped_len=new(n, np.uint32), lead_soft=new(n, np.uint32), trail_soft=new(n, np.uint32), out_quals=new(n_bases, np.uint8))
    o.update({k: None for k in omit})
    cfg = _lib.FinalizeConfig(int(steps), int(min_tail_quality), int(bool(dont_use_soft_clipped_bases)), int(half_of_pcr_snv_qual), 0)
    code = engine.lib.phmm_finalize_reads(
        engine._h, C.byref(cfg), int(a["n_groups"]), _p(a["group_read_off"], _lib.u32p), _p(a["group_span_start"], _lib.u64p),
        _p(a["group_span_end"], _lib.u64p), _p(a["read_pos"], _i64p), _p(a["read_flags"], C.c_void_p), _p(a["read_mapq"], _lib.u8p),
        _p(a["read_mpos"], _i64p), _p(a["read_isize"], _i64p), _p(a["read_cigar_off"], _lib.u32p), _p(a["read_cigar"], _lib.u32p),
        _p(a["read_off"], _lib.u32p), _p(a["read_bases"], _lib.u8p), _p(a["read_quals"], _lib.u8p), _p(a["mate_index"], _i32p),
        _p(a["out_cigar_off"], _lib.u64p), _p(o["read_status"], _i32p), _p(o["keep"], _lib.u8p), _p(o["new_pos"], _i64p),
        _p(o["out_unmapped"], _lib.u8p), _p(o["clip_first"], _lib.u32p), _p(o["clip_len"], _lib.u32p), _p(o["out_cigar"], _lib.u32p),
        _p(o["n_out_cigar"], _lib.u32p), _p(o["unclipped_len"], _lib.u32p), _p(o["lead_soft"], _lib.u32p), _p(o["trail_soft"], _lib.u32p),
        _p(o["out_quals"], _lib.u8p))
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = {k: v for k, v in o.items() if v is not None}
        raise err
    return FinalizeResult(out_cigar_off=a["out_cigar_off"], read_off=a["read_off"], **o)
