"""The activity profile on the device (phmm_activity_profile, include/phmm.h): per (window, sample, position) the reference's
RefVsAnyResult, per position the soft-clip average and is_active_prob, per profile the band-passed state list."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .engine import PhmmError
from .events import encode_cigar as _encode_cigar

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)

Window = namedtuple("Window", "start ref contig_length samples")
Window.__doc__ = """One window (the reference's outer chunk): outer_chunk_location.start, the reference bases from there on (bytes;
the window is as long as they are), the contig's length, and per sample the reads in fetch order as (pos, cigar, bases, quals)
with the CIGAR a string, a list of (op, length) or BAM-encoded integers."""

ActivityResult = namedtuple("ActivityResult", "window_status pos_off read_counts ref_depth non_ref_depth gl pl soft_clip_mean "
                            "soft_clip_count qual af_flags is_active_prob filter_size profile_window profile_start profile_off "
                            "profile_len profile_prob")
ActivityResult.__doc__ = """The outputs of phmm_activity_profile (None where omitted) and the layout that goes with them: pos_off
[n_windows + 1]; per profile its window, the contig position of its first state and where its list starts in profile_prob."""
ActivityResult.profile = lambda self, k: self.profile_prob[self.profile_off[k]:self.profile_off[k] + self.profile_len[k]]

OUTPUTS = ("read_counts", "ref_depth", "non_ref_depth", "gl", "pl", "soft_clip_mean", "soft_clip_count", "qual", "af_flags",
           "is_active_prob", "filter_size", "profile_prob", "profile_len")


def encode_cigar(cigar):
    """A CIGAR as BAM-encoded elements: a string, BAM-encoded integers, or (op, length) pairs with op a letter or a BAM code."""
    if not isinstance(cigar, str):
        cigar = [("MIDNSHP=X".index(c[0]), c[1]) if isinstance(c, (tuple, list)) and isinstance(c[0], str) else c for c in cigar]
    return _encode_cigar(cigar)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def pack(windows, n_samples=None):
    """The input arrays of phmm_activity_profile for a list of Window (or equal tuples / dicts)."""
    windows = [Window(**w) if isinstance(w, dict) else Window(*w) for w in windows]
    n_samples = n_samples if n_samples is not None else (len(windows[0].samples) if windows else 1)
    if any(len(w.samples) != n_samples for w in windows):
        raise ValueError("every window carries the reads of the same number of samples")
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in parts] + [np.zeros(0, dt)]), dt)  # noqa: E731
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)  # noqa: E731
    groups = [g for w in windows for g in w.samples]
    reads = [r for g in groups for r in g]
    cigars = [encode_cigar(r[1]) for r in reads]
    return dict(
        n_windows=len(windows), n_samples=n_samples, window_start=np.array([w.start for w in windows], np.uint64),
        window_len=np.array([len(w.ref) for w in windows], np.uint32),
        window_contig_length=np.array([w.contig_length for w in windows], np.uint64),
        window_ref_off=off([len(w.ref) for w in windows]),
        ref_bases=cat([np.frombuffer(bytes(w.ref), np.uint8) for w in windows], np.uint8),
        group_read_off=off([len(g) for g in groups]), read_pos=np.array([r[0] for r in reads], np.int64),
        read_cigar_off=off([len(c) for c in cigars]), read_cigar=cat(cigars, np.uint32), read_off=off([len(r[2]) for r in reads]),
        read_bases=cat([np.frombuffer(bytes(r[2]), np.uint8) for r in reads], np.uint8),
        read_quals=cat([np.asarray(list(r[3]), np.uint8) for r in reads], np.uint8))


def layout(window_len, profile_size, max_filter_size):
    """pos_off [n_windows + 1] and, per profile, (window, offset of its first state in the window, positions, list offset)."""
    pos_off = np.concatenate([[0], np.cumsum(np.asarray(window_len, np.int64))])
    profiles = []
    for w, n in enumerate(int(x) for x in window_len):
        step = int(profile_size) or n
        for at in range(0, n, step or 1):
            profiles.append((w, at, min(step, n - at), int(pos_off[w]) + at + len(profiles) * int(max_filter_size)))
    return pos_off, profiles


def activity_profile(engine, windows, ploidy=2, min_base_quality=10, pseudo_counts=(10.0, 0.01, 0.00125), stand_min_conf=0.0,
                     max_prob_propagation=50, max_filter_size=50, sigma=17.0, adaptive_filter_size=True, profile_size=0,
                     fill=None, omit=()):
    """The activity profile of a batch of windows.  windows: a list of Window, or what `pack` returns.  pseudo_counts: (ref, snp,
    indel) as phmm_allele_frequency takes them.  fill: a byte the output arrays hold before the call, omit: names of outputs
    passed as NULL (both for tests).  Raises PhmmError (its `outputs` attribute holds the arrays as the call left them)."""
    a = windows if isinstance(windows, dict) else pack(windows)
    nw, ns, G = a["n_windows"], a["n_samples"], int(ploidy) + 1
    window_len = a["window_len"] if a["window_len"] is not None else np.zeros(nw, np.uint32)
    pos_off, profiles = layout(window_len, profile_size, max_filter_size)
    P, K = int(pos_off[-1]), len(profiles)
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    o = dict(window_status=new(nw, np.int32), read_counts=new(P * ns, np.uint32), ref_depth=new(P * ns, np.uint32),
             non_ref_depth=new(P * ns, np.uint32), gl=new(P * ns * G, np.float64), pl=new(P * ns * G, np.int32),
             soft_clip_mean=new(P, np.float64), soft_clip_count=new(P, np.uint32), qual=new(P, np.float64),
             af_flags=new(P, np.uint32), is_active_prob=new(P, np.float32), filter_size=new(1, np.uint32),
             profile_prob=new(P + K * int(max_filter_size), np.float32), profile_len=new(K, np.uint32))
    o.update({k: None for k in omit})
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    code = engine.lib.phmm_activity_profile(
        engine._h, nw, ns, int(ploidy), int(min_base_quality), float(pseudo_counts[0]), float(pseudo_counts[1]), float(pseudo_counts[2]),
        float(stand_min_conf), int(max_prob_propagation), int(max_filter_size), float(sigma), int(bool(adaptive_filter_size)),
        int(profile_size), _p(a["window_start"], _lib.u64p), _p(a["window_len"], _lib.u32p), _p(a["window_contig_length"], _lib.u64p),
        _p(a["window_ref_off"], _lib.u32p), _p(a["ref_bases"], _lib.u8p), _p(a["group_read_off"], _lib.u32p), _p(a["read_pos"], _i64p),
        _p(a["read_cigar_off"], _lib.u32p), _p(a["read_cigar"], _lib.u32p), _p(a["read_off"], _lib.u32p), _p(a["read_bases"], _lib.u8p),
        _p(a["read_quals"], _lib.u8p), _p(o["window_status"], _i32p), _p(o["read_counts"], _lib.u32p), _p(o["ref_depth"], _lib.u32p),
        _p(o["non_ref_depth"], _lib.u32p), _p(o["gl"], _lib.f64p), _p(o["pl"], _i32p), _p(o["soft_clip_mean"], _lib.f64p),
        _p(o["soft_clip_count"], _lib.u32p), _p(o["qual"], _lib.f64p), _p(o["af_flags"], _lib.u32p), vp(o["is_active_prob"]),
        _p(o["filter_size"], _lib.u32p), vp(o["profile_prob"]), _p(o["profile_len"], _lib.u32p))
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = {k: v for k, v in o.items() if v is not None}
        raise err
    for k in ("read_counts", "ref_depth", "non_ref_depth"):
        o[k] = None if o[k] is None else o[k].reshape(P, ns)
    for k in ("gl", "pl"):
        o[k] = None if o[k] is None else o[k].reshape(P, ns, G)
    o["filter_size"] = None if o["filter_size"] is None else int(o["filter_size"][0])
    starts = [int(a["window_start"][w]) + at for w, at, _, _ in profiles]
    return ActivityResult(pos_off=pos_off, profile_window=np.array([p[0] for p in profiles], np.int64),
                          profile_start=np.array(starts, np.int64), profile_off=np.array([p[3] for p in profiles], np.int64), **o)
