"""phmm_assembly_kmers on the MI355X against the restatement of the reference's k-mer stage in front of the read-threading graph
(tests/assembly_kmers_restatement.py), through the C ABI as lorikeet_amd.assembly binds it.  EQUALITY on every output array,
ids included: it is all integers and bytes, there are no tolerances.  The regions come from tests/assembly_kmers_cases.py;
tests/test_assembly_kmers_oracle.py holds the restatement to the reference's literals and to hand-derived expectations and
counts on the CPU what the sets exercise.  Every comparison runs twice: with the tables' fingerprints whole and cut to 4 bits
(switch asm_fingerprint_bits), where sixteen fingerprints serve every k-mer, so probing and the byte comparison decide.  The
module imports lorikeet_amd.assembly at the top: without the call every test here fails."""
import numpy as np
import pytest

import assembly_kmers_cases as K
import finalize_cases as FK
from lorikeet_amd import _lib, assembly, finalize
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
CALLS = K.calls()


@pytest.fixture(scope="module", params=[0, 4], ids=["fp64", "fp4"])
def eng(request):
    e = HipPairHMMEngine()
    e.set_switch("asm_fingerprint_bits", request.param)
    yield e
    e.close()


def run(eng, c, windows=None, **kw):
    regions = [(g["ref"], g["reads"]) for g in c["regions"]]
    first = length = None
    if windows is not None:
        first = [f for w in windows for f, _ in w]
        length = [n for w in windows for _, n in w]
    return assembly.assembly_kmers(eng, regions, c["k"], c["min_q"], read_first=first, read_len=length, **kw)


def same(got, want, tag, ids=True):
    for name in assembly.OUTPUTS:
        g, w = got[name], want[name]
        if not ids and name.endswith("_id"):
            assert g is None, (tag, name)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_equals_the_restatement(eng, name):
    """each set in a call of its own: the golden and the hand cases one region per call, then all of them in one, the pass
    boundaries, the run lengths, every k, eight k, the low-complexity regions and the 24 seeded ones"""
    same(run(eng, CALLS[name], fill=0xAB), K.expected(CALLS[name]), name)


def test_the_largest_reference_and_a_long_read_take_their_tables_out_of_lds(eng):
    c = K.largest_reference(_lib.PHMM_ASM_MAX_REF_BASES)
    want = K.expected(c)
    assert want["flags"][0, 0] & _lib.PHMM_ASM_REF_NON_UNIQUE        # 16 384 random bases repeat some 10-mer
    same(run(eng, c, fill=0xAB), want, "largest")


@pytest.mark.parametrize("name", ["every_k", "eight_k", "seeded"])
def test_a_call_with_several_k_equals_each_k_alone(eng, name):
    c = CALLS[name]
    many = run(eng, c)
    for i, k in enumerate(c["k"]):
        alone = run(eng, K.call(c["regions"], [k], c["min_q"]))
        for out in assembly.OUTPUTS:
            assert np.array_equal(many[out][i], alone[out][0]), (name, k, out)


def test_a_region_of_a_batch_equals_the_same_region_alone_and_a_second_call(eng):
    c = CALLS["seeded"]
    first, again = run(eng, c), run(eng, c)
    for out in assembly.OUTPUTS:
        assert first[out].tobytes() == again[out].tobytes(), out
    ro, po = first["region_ref_off"], first["read_off"][first["region_read_off"]]
    for g in (0, 7, len(c["regions"]) - 1):
        alone = run(eng, K.call([c["regions"][g]], c["k"], c["min_q"]))
        for out in K.REGION_OUTPUTS:
            assert np.array_equal(first[out][:, g], alone[out][:, 0]), (g, out)
        for out, off in (("ref_kmer_flags", ro), ("ref_kmer_id", ro), ("read_kmer_flags", po), ("read_kmer_id", po)):
            assert np.array_equal(first[out][:, off[g]:off[g + 1]], alone[out]), (g, out)


def _windows(c, seed):
    import random
    rng = random.Random(seed)
    out = []
    for g in c["regions"]:
        w = []
        for b, _ in g["reads"]:
            f = rng.randrange(len(b) + 1)
            w.append((f, rng.randrange(len(b) - f + 1)) if rng.randrange(4) else (0, len(b)))
        out.append(w)
    return out


@pytest.mark.parametrize("name", ["seeded", "pass_boundaries", "scan_from_zero"])
def test_windows_equal_the_same_reads_cut_beforehand(eng, name):
    c = CALLS[name]
    w = _windows(c, 3)
    got = run(eng, c, windows=w, fill=0xAB)
    same(got, K.expected(c, windows=w), name)
    cut = K.call([dict(ref=g["ref"], reads=[(b[f:f + n], q[f:f + n]) for (b, q), (f, n) in zip(g["reads"], wg)])
                  for g, wg in zip(c["regions"], w)], c["k"], c["min_q"])
    pre = run(eng, cut)
    for out in K.REGION_OUTPUTS + ("ref_kmer_flags", "ref_kmer_id"):
        assert np.array_equal(got[out], pre[out]), out
    inside = np.zeros(got["read_kmer_flags"].shape[1], bool)
    at = 0
    for g, wg in zip(c["regions"], w):
        for (b, _), (f, n) in zip(g["reads"], wg):
            inside[at + f:at + f + n] = True
            at += len(b)
    assert np.array_equal(got["read_kmer_flags"][:, inside], pre["read_kmer_flags"])
    assert np.array_equal(got["read_kmer_id"][:, inside], pre["read_kmer_id"])
    assert not got["read_kmer_flags"][:, ~inside].any() and (got["read_kmer_id"][:, ~inside] == 0xFFFFFFFF).all()


def test_the_output_of_finalize_reads_feeds_the_call_with_no_base_copied(eng):
    """one small group: soft clips, low-quality tails and a span that cuts -- clip_first / clip_len and out_quals go in as they
    came out, and the answer is the restatement's on the reads cut by hand"""
    ref = K.bases(__import__("random").Random(5), 60)
    reads = [FK.read("5S40M5S", pos=100, bases=ref[:50], quals=30), FK.read("50M", pos=95, bases=ref[5:55], quals=[2] * 4 + [30] * 40 + [2] * 6),
             FK.read("30M", pos=110, bases=ref[20:50], quals=30), FK.read("20M", pos=400, bases=ref[:20], quals=30)]
    fin = finalize.finalize_reads(eng, [FK.group(reads, span=(104, 140))])
    packed = finalize.pack([FK.group(reads, span=(104, 140))])
    keep = fin.keep.astype(bool)
    first, length = np.where(keep, fin.clip_first, 0), np.where(keep, fin.clip_len, 0)
    assert keep.any() and not keep.all() and (length[keep] < np.diff(packed["read_off"])[keep]).any()
    arrays = dict(region_ref_off=np.array([0, len(ref)], np.uint32), ref_bases=np.frombuffer(ref, np.uint8), region_read_off=np.array([0, len(reads)], np.uint32),
                  read_off=packed["read_off"], read_bases=packed["read_bases"], read_quals=fin.out_quals)
    got = assembly.assembly_kmers(eng, arrays, [5, 10], read_first=first, read_len=length, fill=0xAB)
    whole = [(bytes(r["bases"]), bytes(fin.quals(i))) for i, r in enumerate(reads)]
    c = K.call([dict(ref=ref, reads=whole)], [5, 10])
    same(got, K.expected(c, windows=[list(zip(first.tolist(), length.tolist()))]), "chain")


def test_without_ids_the_other_arrays_are_the_same(eng):
    c = CALLS["seeded"]
    same(run(eng, c, ids=False, fill=0xAB), K.expected(c), "no ids", ids=False)


def test_no_region_and_regions_without_reads(eng):
    assert run(eng, K.call([], [3]))["flags"].shape == (1, 0)
    c = K.call([K.region("ACGTTGCA"), K.region(""), K.region("AC", ["ACGT"])], [3, 4])
    same(run(eng, c, fill=0xAB), K.expected(c), "no reads")


# ---- PHMM_ERR_INVALID_ARG, every case the header names ---------------------------------------------------------------------------
def _arrays():
    return assembly.pack([(b"ACGTTGCA", [K.read("ACGTAC"), K.read("TTGCAT")]), (b"GATTCCAGT", [K.read("GATTC")])])


def _refused(eng, arrays, k=(3,), part=None, **kw):
    with pytest.raises(PhmmError) as e:
        assembly.assembly_kmers(eng, arrays, list(k), fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and (part is None or part in str(e.value)), str(e.value)
    for name, a in e.value.outputs.items():                      # nothing written
        assert (np.frombuffer(a.tobytes(), np.uint8) == 0xAB).all(), name


@pytest.mark.parametrize("name", ["region_ref_off", "region_read_off", "read_off"])
def test_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    a = _arrays()
    a[name] = a[name].copy()
    a[name][0] = 1
    _refused(eng, a, part="does not start at 0")
    a = _arrays()
    a[name] = a[name].copy()
    a[name][1] = a[name][2] + 1
    _refused(eng, a, part="decreases")


def test_a_window_outside_its_read_is_refused(eng):
    a = _arrays()
    _refused(eng, a, read_first=[0, 0, 0], read_len=[6, 7, 5], part="window")
    _refused(eng, a, read_first=[0, 7, 0], read_len=[6, 0, 5], part="window")
    _refused(eng, a, read_first=[0, 3, 0], read_len=[6, 4, 5], part="window")
    _refused(eng, a, read_first=[0, 0, 0], part="together")
    _refused(eng, a, read_len=[6, 6, 5], part="together")


def test_k_out_of_range_or_not_ascending_is_refused(eng):
    a = _arrays()
    _refused(eng, a, k=(0,), part="k[0]")
    _refused(eng, a, k=(3, _lib.PHMM_ASM_MAX_K + 1), part="k[1]")
    _refused(eng, a, k=(3, 3), part="ascending")
    _refused(eng, a, k=(5, 3), part="ascending")


def test_n_k_out_of_range_is_refused(eng):
    a = _arrays()
    _refused(eng, a, k=(), part="n_k")
    _refused(eng, a, k=tuple(range(1, _lib.PHMM_ASM_MAX_K_VALUES + 2)), part="n_k")


def test_sequences_above_their_limits_are_refused(eng):
    long_ref = assembly.pack([(b"A" * (_lib.PHMM_ASM_MAX_REF_BASES + 1), [])])
    _refused(eng, long_ref, part="region 0: more than %d reference bases" % _lib.PHMM_ASM_MAX_REF_BASES)
    long_read = assembly.pack([(b"ACGT", [K.read(b"A" * (_lib.PHMM_ASM_MAX_READ_BASES + 1))])])
    _refused(eng, long_read, part="read 0: more than %d bases" % _lib.PHMM_ASM_MAX_READ_BASES)
    # the window counts, not the slot it lies in
    got = assembly.assembly_kmers(eng, long_read, [3], read_first=[1], read_len=[_lib.PHMM_ASM_MAX_READ_BASES])
    assert got["n_sequences"].tolist() == [[2]]


def test_missing_arrays_and_a_lone_id_plane_are_refused(eng):
    for name in ("region_ref_off", "ref_bases", "region_read_off", "read_off", "read_bases", "read_quals"):
        a = _arrays()
        a[name] = None
        _refused(eng, a, part="NULL")
    _refused(eng, _arrays(), min_base_quality=256, part="min_base_quality")
    a = _arrays()
    lib, z = eng.lib, np.zeros(64, np.uint32)
    u32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    u8 = lambda x: x.ctypes.data_as(_lib.u8p)  # noqa: E731
    k = np.array([3], np.uint32)
    args = (eng._h, 2, u32(a["region_ref_off"]), u8(a["ref_bases"]), u32(a["region_read_off"]), u32(a["read_off"]), u8(a["read_bases"]),
            u8(a["read_quals"]), None, None, 1, u32(k), 10, u32(z), u32(z), u32(z), u32(z), u32(z), u8(z.view(np.uint8)), u8(z.view(np.uint8)))
    assert lib.phmm_assembly_kmers(*args, u32(z), None) == _lib.PHMM_ERR_INVALID_ARG
    assert lib.phmm_assembly_kmers(*args, None, u32(z)) == _lib.PHMM_ERR_INVALID_ARG
    assert not z.any()


def test_bases_times_n_k_above_the_positions_limit_is_refused(eng):
    """4 097 reads of 16 384 bases at eight k: 537 001 984 positions, above PHMM_ASM_MAX_POSITIONS (2^29), which keeps the 32-bit
    workspace indices from wrapping.  The call refuses before it reads a base, so the base, quality and output arrays are small."""
    n_reads, n = 4097, _lib.PHMM_ASM_MAX_READ_BASES
    k = np.arange(1, _lib.PHMM_ASM_MAX_K_VALUES + 1, dtype=np.uint32)
    assert n_reads * n * len(k) > _lib.PHMM_ASM_MAX_POSITIONS >= (n_reads - 1) * n * len(k)
    read_off = (np.arange(n_reads + 1, dtype=np.uint64) * n).astype(np.uint32)
    zero2, reads = np.zeros(2, np.uint32), np.array([0, n_reads], np.uint32)
    dummy = np.full(64, 0x41, np.uint8)
    outs = [np.full(64, 0xAB, np.uint8) for _ in range(9)]
    u32 = lambda x: x.ctypes.data_as(_lib.u32p)  # noqa: E731
    u8 = lambda x: x.ctypes.data_as(_lib.u8p)  # noqa: E731
    code = eng.lib.phmm_assembly_kmers(eng._h, 1, u32(zero2), u8(dummy), u32(reads), u32(read_off), u8(dummy), u8(dummy), None, None, len(k), u32(k), 10,
                                       *[u32(o) for o in outs[:5]], u8(outs[5]), u8(outs[6]), u32(outs[7]), u32(outs[8]))
    assert code == _lib.PHMM_ERR_INVALID_ARG
    assert "bases x n_k is above %d" % _lib.PHMM_ASM_MAX_POSITIONS in eng.last_error(), eng.last_error()
    for o in outs:
        assert (o == 0xAB).all()
