"""Assembly regions on the device (phmm_assembly_regions, include/phmm.h): the band-passed state lists of the activity profile
cut as pop_ready_assembly_regions cuts them, and per (region, sample) the staged reads a fetch of the padded span returns."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import PhmmError

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
ACTIVE, FORCED, OVER_DEPTH = 1, 2, 4
STATUS_MIN_REGION_SIZE, STATUS_START_PAST_CONTIG = -1, -2

PROFILE_INPUTS = (("profile_prob", np.float32), ("profile_first", np.uint32), ("profile_len", np.uint32), ("profile_start", np.uint64),
                  ("profile_stop", np.uint64), ("profile_contig_length", np.uint64), ("profile_window", np.uint32))
READ_INPUTS = (("group_read_off", np.uint32), ("read_pos", np.int64), ("read_cigar_off", np.uint32), ("read_cigar", np.uint32),
               ("read_off", np.uint32), ("read_quals", np.uint8))
REGION_OUTPUTS = (("region_start", np.uint64), ("region_end", np.uint64), ("region_padded_start", np.uint64),
                  ("region_padded_end", np.uint64), ("region_states", np.uint32), ("region_flags", np.uint32),
                  ("region_density", np.float32), ("region_n_reads", np.uint32))
OUTPUTS = (("profile_status", np.int32), ("profile_region_off", np.uint32)) + REGION_OUTPUTS + (
    ("region_read_off", np.uint32), ("region_reads", np.uint32), ("read_mean_qual", np.float64))
_CT = {np.uint8: _lib.u8p, np.uint32: _lib.u32p, np.uint64: _lib.u64p, np.int32: _i32p, np.int64: _i64p, np.float64: _lib.f64p,
       np.float32: C.c_void_p}


def _p(a, dt):
    return None if a is None else a.ctypes.data_as(_CT[dt])


def from_activity(result, windows, profile_size=0):
    """The profile arrays of phmm_assembly_regions from activity_profile's result and the arrays it was given (what
    activity.pack returns): the lists pass as they are, with the reads of their windows."""
    a = windows
    lens = np.asarray(result.profile_len, np.uint32)
    win = np.asarray(result.profile_window, np.int64)
    start = np.asarray(result.profile_start, np.uint64)
    n_pos = np.zeros(len(lens), np.uint64)  # the positions the profile was fed: its last ADDED state is the last of them
    wl, ws = np.asarray(a["window_len"], np.int64), np.asarray(a["window_start"], np.int64)
    for k in range(len(lens)):
        at = int(start[k]) - int(ws[win[k]])
        n_pos[k] = min(int(profile_size) or int(wl[win[k]]), int(wl[win[k]]) - at)
    out = dict(profile_prob=np.ascontiguousarray(result.profile_prob, np.float32), profile_first=np.asarray(result.profile_off, np.uint32),
               profile_len=lens, profile_start=start, profile_stop=start + n_pos - np.uint64(1),
               profile_contig_length=np.asarray(a["window_contig_length"], np.uint64)[win], profile_window=win.astype(np.uint32),
               n_windows=int(a["n_windows"]), n_samples=int(a["n_samples"]))
    out.update({k: a[k] for k, _ in READ_INPUTS})
    return out


def assembly_regions(engine, profiles, windows=None, assembly_region_extension=100, min_region_size=50, max_region_size=300,
                     max_prob_propagation=50, active_prob_threshold=0.002, max_input_depth=200000, profile_size=0, with_reads=True,
                     capacity=None, fill=None, omit=()):
    """Cut activity profiles into assembly regions, with their reads (phmm_assembly_regions).  profiles: a dict of the input
    arrays under the header's names (n_windows and n_samples with them when it carries reads), or activity_profile's result with
    `windows` the packed arrays it was computed from (and its profile_size).  with_reads=False leaves the read arrays out.
    capacity: (regions, memberships); None asks the library first (a call with capacities 0).  fill: a byte the output arrays hold
    before the call, omit: names of arrays passed as NULL (both for tests).  Returns a dict of numpy arrays under the header's
    names, cut to what was written, with `required`.  Raises PhmmError; after PHMM_ERR_EVENT_CAPACITY its `required` attribute
    holds the two sizes."""
    a = profiles if isinstance(profiles, dict) else from_activity(profiles, windows, profile_size)
    i = {name: (None if name in omit or a.get(name) is None else np.ascontiguousarray(a[name], dt)) for name, dt in PROFILE_INPUTS + READ_INPUTS}
    if not with_reads:
        i.update({name: None for name, _ in READ_INPUTS})
    per_profile = [a[name] for name, _ in PROFILE_INPUTS[1:] if a.get(name) is not None]   # (counted before `omit` takes any away)
    n_profiles = int(a["n_profiles"]) if "n_profiles" in a else (len(per_profile[0]) if per_profile else 0)
    n_prob = int(a["n_prob"]) if "n_prob" in a else (len(a["profile_prob"]) if a.get("profile_prob") is not None else 0)
    n_windows, n_samples = int(a.get("n_windows", 0)), int(a.get("n_samples", 0))
    n_reads = len(i["read_pos"]) if i["read_pos"] is not None else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731

    def call(cap):
        cap = np.array([int(cap[0]), int(cap[1])], np.uint32)
        R, M = int(cap[0]), int(cap[1])
        o = dict(required=new(2, np.uint32), profile_status=new(n_profiles, np.int32), profile_region_off=new(n_profiles + 1, np.uint32),
                 region_read_off=new(R * max(n_samples, 1) + 1, np.uint32), region_reads=new(M, np.uint32), read_mean_qual=new(n_reads, np.float64))
        o.update({name: new(R, dt) for name, dt in REGION_OUTPUTS})
        o.update({k: None for k in omit if k in o})
        code = engine.lib.phmm_assembly_regions(
            engine._h, n_profiles, n_windows, n_samples, int(assembly_region_extension), int(min_region_size), int(max_region_size),
            int(max_prob_propagation), float(np.float32(active_prob_threshold)), int(max_input_depth), n_prob,
            *[_p(i[name], dt) for name, dt in PROFILE_INPUTS + READ_INPUTS], None if "capacity" in omit else _p(cap, np.uint32),
            _p(o["required"], np.uint32), *[_p(o[name], dt) for name, dt in OUTPUTS])
        return code, o

    if capacity is None:
        code, o = call((0, 0))
        if code == _lib.PHMM_ERR_EVENT_CAPACITY:
            code, o = call(o["required"])
    else:
        code, o = call(capacity)
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.required = None if o["required"] is None else o["required"].copy()
        err.outputs = {k: v for k, v in o.items() if v is not None}
        raise err
    R, M = (int(x) for x in o["required"])
    reads = i["group_read_off"] is not None
    cut = {name: R for name, _ in REGION_OUTPUTS}
    cut.update(region_read_off=(R * n_samples + 1) if reads else 0, region_reads=M, read_mean_qual=n_reads if reads else 0)
    o = {k: (v if v is None or k not in cut else v[:cut[k]]) for k, v in o.items()}
    o["inputs"] = a
    return o
