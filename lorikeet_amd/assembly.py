"""The k-mer stage in front of the read-threading graph on the device (phmm_assembly_kmers, include/phmm.h): per region and k
the verdicts that reject a k before a vertex exists, the sizes of the non-unique set and of the vertex map, and per position
whether its k-mer is non-unique, threaded, a threading start, the first of its bytes, with its dense id."""
import ctypes as C

import numpy as np

from . import _lib
from .engine import PhmmError

REGION_OUTPUTS = ("flags", "n_sequences", "n_non_unique", "n_tracked", "n_distinct")
OUTPUTS = REGION_OUTPUTS + ("ref_kmer_flags", "read_kmer_flags", "ref_kmer_id", "read_kmer_id")


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _bytes(x):
    if isinstance(x, str):
        x = x.encode()
    return np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8)


def pack(regions):
    """regions: one (reference, reads) per region, reads a list of (bases, quals); bases as bytes or uint8 arrays.  Returns the
    dense arrays phmm_assembly_kmers takes: region_ref_off, ref_bases, region_read_off, read_off, read_bases, read_quals."""
    region_ref_off, region_read_off, read_off = [0], [0], [0]
    refs, bases, quals = [], [], []
    for ref, reads in regions:
        refs.append(_bytes(ref))
        region_ref_off.append(region_ref_off[-1] + len(refs[-1]))
        for b, q in reads:
            b, q = _bytes(b), _bytes(q)
            if len(b) != len(q):
                raise ValueError("a read's bases and qualities differ in length")
            bases.append(b)
            quals.append(q)
            read_off.append(read_off[-1] + len(b))
        region_read_off.append(len(read_off) - 1)
    cat = lambda xs: np.concatenate(xs).astype(np.uint8) if xs else np.zeros(0, np.uint8)  # noqa: E731
    return dict(region_ref_off=np.asarray(region_ref_off, np.uint32), ref_bases=cat(refs),
                region_read_off=np.asarray(region_read_off, np.uint32), read_off=np.asarray(read_off, np.uint32),
                read_bases=cat(bases), read_quals=cat(quals))


def assembly_kmers(engine, regions, k, min_base_quality=10, read_first=None, read_len=None, ids=True, fill=None):
    """The k-mer stage of the assembler for a batch of regions (phmm_assembly_kmers).  regions: a list of (reference, reads) as
    pack() takes it, or a dict of the dense arrays pack() returns; k: the k values, ascending; read_first / read_len: per-read
    windows (what finalize_reads returns as clip_first / clip_len), None = the whole reads; ids=False: the id planes are not
    asked for (None in the result); fill: a byte the output arrays hold before the call (tests).  Returns a dict of numpy
    arrays: flags, n_sequences, n_non_unique, n_tracked, n_distinct [n_k, n_regions]; ref_kmer_flags [n_k, reference bases],
    read_kmer_flags [n_k, read bases]; ref_kmer_id, read_kmer_id likewise; and the dense input arrays under their names.
    Raises PhmmError."""
    a = regions if isinstance(regions, dict) else pack(regions)
    u32 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint32)  # noqa: E731
    u8 = lambda x: None if x is None else np.ascontiguousarray(x, np.uint8)  # noqa: E731
    region_ref_off, region_read_off, read_off = u32(a.get("region_ref_off")), u32(a.get("region_read_off")), u32(a.get("read_off"))
    ref_bases, read_bases, read_quals = u8(a.get("ref_bases")), u8(a.get("read_bases")), u8(a.get("read_quals"))
    read_first, read_len = u32(read_first), u32(read_len)
    k = np.ascontiguousarray(k, np.uint32).reshape(-1)
    n_k = len(k)
    n_regions = next((len(x) - 1 for x in (region_ref_off, region_read_off) if x is not None), 0)
    # (the sizes of the outputs; with an offset array missing or broken -- the library refuses those -- any size will do)
    n_ref = int(region_ref_off[-1]) if n_regions and region_ref_off is not None else 0
    n_read = int(read_off[-1]) if read_off is not None and len(read_off) else 0
    new = lambda n, dt: np.zeros(n, dt) if fill is None else np.frombuffer(bytes([fill]) * (n * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    o = {name: new(n_k * n_regions, np.uint32) for name in REGION_OUTPUTS}
    o.update(ref_kmer_flags=new(n_k * n_ref, np.uint8), read_kmer_flags=new(n_k * n_read, np.uint8),
             ref_kmer_id=new(n_k * n_ref, np.uint32) if ids else None, read_kmer_id=new(n_k * n_read, np.uint32) if ids else None)
    code = engine.lib.phmm_assembly_kmers(
        engine._h, n_regions, _p(region_ref_off, _lib.u32p), _p(ref_bases, _lib.u8p), _p(region_read_off, _lib.u32p),
        _p(read_off, _lib.u32p), _p(read_bases, _lib.u8p), _p(read_quals, _lib.u8p), _p(read_first, _lib.u32p), _p(read_len, _lib.u32p),
        n_k, _p(k, _lib.u32p), int(min_base_quality), *[_p(o[name], _lib.u32p) for name in REGION_OUTPUTS],
        _p(o["ref_kmer_flags"], _lib.u8p), _p(o["read_kmer_flags"], _lib.u8p), _p(o["ref_kmer_id"], _lib.u32p), _p(o["read_kmer_id"], _lib.u32p))
    if code != _lib.PHMM_OK:
        err = PhmmError(code, engine.last_error())
        err.outputs = {name: v for name, v in o.items() if v is not None}
        raise err
    for name in REGION_OUTPUTS:
        o[name] = o[name].reshape(n_k, n_regions)
    for name, n in (("ref_kmer_flags", n_ref), ("read_kmer_flags", n_read), ("ref_kmer_id", n_ref), ("read_kmer_id", n_read)):
        if o[name] is not None:
            o[name] = o[name].reshape(n_k, n)
    o.update(region_ref_off=region_ref_off, region_read_off=region_read_off, read_off=read_off, k=k)
    return o
