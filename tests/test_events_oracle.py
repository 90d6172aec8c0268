"""The restatement of the reference's event discovery (tests/events_restatement.py) against the reference's own test cases
(tests/golden/event_map_cases.json), and a census of what the regions of the GPU tests (tests/events_cases.py) exercise, so
that no GPU case is vacuous.  CPU only."""
import events_cases as K
import events_restatement as R

TYPES = {"Snp": R.SNP, "Mnp": R.MNP, "Indel": R.INDEL}


def vc_of(v, source=None):
    vc = R.VC(v["start"], v["end"], [v["ref"].encode(), v["alt"].encode()], source)
    vc.vtype = TYPES[v["type"]]
    return vc


def test_mnps_rows():
    for row in K.golden()["test_mnps"]:
        for d in row["distances"]:
            m = R.event_map(row["ref"].encode(), 1, row["hap"].encode(), R.parse_cigar(row["cigar"]), 0, d)
            assert [[vc.ref.decode(), vc.alt.decode()] for vc in m.values()] == row["expected"], (row, d)


def test_get_overlapping_events_rows():
    g = K.golden()
    for row in g["test_get_overlapping_events"]:
        m = R.event_map(g["overlapping_ref"].encode(), 1, row["hap"].encode(), R.parse_cigar(row["cigar"]), g["overlapping_hap_start"], 1)
        over = R.get_overlapping_events(m, row["loc"])
        assert len(over) == (0 if row["ref"] is None else 1), row
        if over:
            assert (over[0].ref.decode(), over[0].alt.decode()) == (row["ref"], row["alt"]), row


def test_make_blocks_rows():
    for first, second, expected in K.golden()["test_make_blocks"]:
        mk = lambda a: R.VC(10, 10 + len(a[0]) - 1, [x.encode() for x in a])  # noqa: E731
        block = R.make_block(mk(first), mk(second))
        assert block.start == 10 and [a.decode() for a in block.alleles] == expected, (first, second)
        assert block.vtype == R.type_of([x.encode() for x in first])  # the cached type is the first event's


def test_active_haplotypes_and_event_mapper_rows():
    g = K.golden()
    for case in g["active_haplotypes"]:
        maps = [R.state_for_testing([vc_of(v, i) for v in h]) for i, h in enumerate(case["haplotypes"])]
        got = R.events_from_haplotypes(case["loc"], maps, True)
        assert [(vc.start, vc.end, vc.ref.decode(), vc.alt.decode()) for vc in got] == \
            [(v["start"], v["end"], v["ref"], v["alt"]) for v in case["expected"]], case["name"]
    case = g["active_haplotypes"][0]  # get_event_mapper_data: the merged context is the SNP itself, haplotypes (snp, ref)
    maps = [R.state_for_testing([vc_of(v, i) for v in h]) for i, h in enumerate(case["haplotypes"])]
    snp = case["expected"][0]
    mapper = R.create_allele_mapper([snp["ref"].encode(), snp["alt"].encode()], case["loc"], maps, True)
    order = g["event_mapper_expected"]["order"]
    assert {str(a): [order[h] for h in hs] for a, hs in mapper.items()} == {k: v for k, v in g["event_mapper_expected"].items() if k != "order"}


def test_window_and_widening():
    assert R.expand_within_contig(1, 5, 2, 100) == (0, 7) and R.expand_within_contig(90, 99, 5, 100) == (85, 100)


def total(cs):
    out = {}
    for c in cs:
        for k, v in c.items():
            if k == "status":
                for s, n in v.items():
                    out.setdefault("status", {})[s] = out.get("status", {}).get(s, 0) + n
            else:
                out[k] = max(out.get(k, 0), v) if k.endswith("_max") else out.get(k, 0) + v
    return out


def test_hand_built_cases_are_what_they_claim():
    by_name = {}
    for name, rg, dists in K.singles():
        by_name[name] = {d: K.census([rg], d) for d in dists}
    st = lambda n, d=0: list(by_name[n][d]["status"])  # noqa: E731
    assert st("pair_II") == st("two_insertions") == st("lower_case_snp_then_ins") == [R.BLOCK]
    assert st("operator_N") == st("operator_P") == st("operator_H") == st("operator_N_after_two_insertions") == [R.BAD_OPERATOR]
    for n in ("overrun_reference", "overrun_reference_M", "overrun_haplotype", "overrun_haplotype_ins", "start_past_reference"):
        assert st(n) == [R.CIGAR_OVERRUN], n
    assert st("del_at_0_past_reference") == [R.OK] and st("lower_case_reference_same_base") == [R.ALLELES]
    for n in ("snp_then_ins", "snp_then_del", "snp_then_ins_del", "snp_ins_ins", "ins_then_del", "pair_ID"):
        assert by_name[n][0]["block"] == 1 and by_name[n][0]["events"] == 1, n
    assert by_name["5D_2I_3D"][0]["block"] == 1 and by_name["5D_2I_3D"][0]["deletion"] == 1 and by_name["5D_2I_3D"][0]["star"] == 1
    for n in ("ins_first", "ins_last", "ins_at_ref_pos_0", "N_as_insertion_anchor", "N_inside_insertion", "n_inside_insertion"):
        assert by_name[n][0]["insertion"] == 0 and st(n) == [R.OK], n
    for n in ("del_at_ref_pos_0", "N_inside_deletion", "N_as_deletion_anchor"):
        assert by_name[n][0]["deletion"] == 0, n
    assert by_name["del_first"][0]["deletion"] == 1 and by_name["del_last"][0]["deletion"] == 1
    assert by_name["lower_case_insertion"][0]["insertion"] == 1 and by_name["lower_case_reference_in_deletion"][0]["deletion"] == 1
    assert by_name["N_in_reference_under_snp"][1]["events"] == 0 and by_name["N_and_lower_case_in_haplotype"][0]["snp"] == 1
    for n in (63, 64, 65, 129):
        c = by_name["M%d_dense" % n]
        assert c[0]["snp"] == (n + 1) // 2 and c[0]["mnp"] == 0 and c[1]["snp"] == (n + 1) // 2 and c[3]["mnp"] == 1 and c[3]["snp"] == 0, n
        assert by_name["M%d" % n][0]["insertion"] == 1 and by_name["M%d" % n][0]["block"] == 1  # the last mismatch joins the deletion
    assert by_name["M129"][0]["snp"] == 3 and by_name["M129"][1]["mnp"] == 1 and by_name["M65"][1]["mnp"] == 1
    pairs = total([by_name["pair_%s%s" % (a, b)][0] for a in "MIDS" for b in "MIDS"])
    assert pairs["snp"] and pairs["insertion"] and pairs["deletion"] and pairs["block"] and pairs["star"], pairs


def test_several_haplotype_cases_are_what_they_claim():
    c = {name: K.census([rg], o.get("dist", 0), o.get("include_spanning", True), o.get("margin", 2)) for name, rg, o in K.multis()}
    assert c["homopolymer"]["events"] == 1 and c["homopolymer"]["multi_allelic"] == 1
    assert c["deletion_spans_snp"]["star"] == 1 and c["deletion_spans_snp_spanning_off"]["star"] == 0
    assert c["two_spanning_deletions"]["star"] == 2 and c["two_spanning_deletions"]["events"] == 3
    two = R.discover([rg for name, rg, _ in K.multis() if name == "two_spanning_deletions"])
    assert two["allele_bases"].endswith(b"G*T") and two["event_hap_allele"][-4:] == [1, 1, 2, 0]  # both deletions span 115: one '*'
    assert c["deletion_ends_where_insertion_starts"]["star"] == 1 and c["deletion_ends_where_insertion_starts"]["block"] == 0
    assert c["mnp_ends_where_insertion_starts"]["mnp"] == 1 and c["mnp_ends_where_insertion_starts"]["star"] == 1
    assert c["5D_2I_3D_beside_others"]["block"] == 1 and c["5D_2I_3D_beside_others"]["star"] == 2
    assert c["same_event_on_several"]["events"] == 2 and c["event_on_later_haplotype_only"]["events"] == 1
    assert c["window_edges"]["events"] == 2 and c["window_empty"]["events"] == 0 and c["window_empty"]["snp"] == 4
    assert list(c["merge_loses_reference"]["status"]) == [R.MERGE] and list(c["one_failing_haplotype"]["status"]) == [R.BAD_OPERATOR]
    assert c["no_haplotypes"]["events"] == 0
    # as written, create_allele_mapper never pushes one haplotype into two lists (see events_restatement's docstring)
    assert all(x["flagged"] == 0 for x in c.values())
    clipped = {name: R.discover([rg], 0, True, o.get("margin", 2)) for name, rg, o in K.multis() if name.startswith("widening")}
    assert clipped["widening_clipped_at_0"]["event_start"] == [0, 0, 0]
    assert max(clipped["widening_clipped_at_contig_end"]["event_end"]) == 97 and clipped["widening_clipped_at_contig_end"]["vc_end"][-1] == 95


def test_random_batches_are_what_they_claim():
    got = {name: (K.census(regions, d), regions) for name, regions, d in K.random_batches()}
    assert [len(r) for _, r in got.values()] == [1, 2, 1, 65]
    assert got["many_loci"][0]["loci_max"] > 64 and got["many_loci"][0]["hap_events_max"] > 64
    assert sorted({len(rg["haps"]) for rg in got["65_regions"][1]}) == [0, 1, 2, 8, 63, 64, 65]
    assert all(40 <= len(rg["ref"]) <= 300 for _, r in got.values() for rg in r)
    assert {len(rg["ref"]) for rg in got["two_regions"][1]} == {40, 300}
    for name, (c, _) in got.items():
        assert c["snp"] and c["insertion"] and c["deletion"] and c["block"] and c["star"] and c["multi_allelic"], (name, c)
        assert set(c["status"]) == {R.OK} and c["flagged"] == 0, (name, c)
    assert got["65_regions"][0]["mnp"] and got["two_regions"][0]["mnp"]
