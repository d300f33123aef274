"""tests/load_footprint.py checked on the CPU: the Legal / Required builders against hand-worked
examples, and compare() on fabricated reports with one named defect each."""
import numpy as np

import load_footprint as lf


def _granules(ranges, n=4096):
    return sorted(np.flatnonzero(lf.mask_of(ranges, n)).tolist())


def test_one_byte_at_residue_15():
    assert lf.granule_span(0x1000 + 15, 1) == (0x100, 0x101)
    assert _granules([(0x1000 + 15, 1)]) == [0x100]
    assert _granules([(0x1000 + 15, 2)]) == [0x100, 0x101]    # the second byte opens the next granule


def test_range_ending_on_a_page():
    # 40 bytes that end at 0x2000: granules 0x1fd..0x1ff, and none of the next page
    assert _granules([(0x2000 - 40, 40)]) == [0x1fd, 0x1fe, 0x1ff]
    assert _granules([(0x2000, 16)]) == [0x200]


def test_empty_range_has_no_granule():
    assert lf.granule_span(0x1234, 0) == (0, 0)
    legal, required = lf.list_ranges([0x1234, 0x3000], [0, 5], [(0x8000, 16)])
    assert legal == [(0x3000, 5), (0x8000, 16)] and required == [(0x3000, 5)]
    assert _granules(legal) == [0x300, 0x800]


def test_update_past_the_chunk_size():
    # chunk of 5000 bytes, a write of 3000 at 4990: the chunk may be read up to 7990, the payload must be
    legal, required = lf.update_io_ranges(0x10000, 0x20003, 4990, 3000, 5000)
    assert legal == [(0x10000, 7990), (0x20003, 3000)] and required == [(0x20003, 3000)]
    assert _granules(legal, 1 << 14)[-1] == (0x20003 + 3000 - 1) >> 4
    assert ((0x10000 + 7990 - 1) >> 4) in _granules(legal, 1 << 14) and ((0x10000 + 7990 + 15) >> 4) not in _granules(legal, 1 << 14)
    # inside the chunk the size bounds it; a truncate reads no payload and must read nothing
    assert lf.update_io_ranges(0x10000, 0x20000, 10, 20, 5000)[0][0] == (0x10000, 5000)
    assert lf.update_io_ranges(0x10000, 0, 0, 0, 9000, update_type_write=False) == ([(0x10000, 9000)], [])
    assert lf.update_io_ranges(0x10000, 0x20000, 0, 0, 100)[1] == []


def test_md5_hole():
    legal, required = lf.md5_ranges([(0x4001, 70), (0, 5000), (0x500f, 130)], [(0x9000, 48)])
    assert required == [(0x4001, 70), (0x500f, 130)]
    assert legal == required + [(0x9000, 48)]
    assert 0 not in _granules(legal)      # the hole's address 0 is no range


def test_frame_header_is_part_of_the_frame():
    # two frames: 20 bytes at 0x1008 (header at 0x1000), an oversize one at 0x2008 of which only the header counts
    legal, required = lf.frame_ranges(0x1000, [8, 0x1008], [20, 9000], 8192, [])
    assert legal == [(0x1000, 28), (0x2000, 8)] and required == [(0x1008, 20)]
    assert _granules(legal) == [0x100, 0x101, 0x200]
    assert lf.frame_ranges(0, [0x28], [0], 100, [(0x900, 24)]) == ([(0x20, 8), (0x900, 24)], [])   # an empty frame


def test_scrub_and_read_records():
    # scrub: typed -> required; NONE -> may be read; another type, fin > 1, too long -> refused unread
    legal, required = lf.scrub_ranges([0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000], [10, 10, 10, 10, 99, 0],
                                      [1, 0, 2, 1, 1, 1], [0, 1, 0, 7, 0, 0], 1, 50, [(0x9000, 24)])
    assert required == [(0x1000, 10)] and legal == [(0x1000, 10), (0x2000, 10), (0x9000, 24)]
    # read: (data, offset, length, chunk_len, batch type, chunk type, recalculate)
    recs = [(0x1000, 0, 64, 64, 1, 1, 0),    # a full read of the stored type: reused, nothing must be read
            (0x2000, 0, 64, 64, 1, 0, 0),    # the chunk has no checksum: hashed
            (0x3000, 5, 64, 100, 1, 1, 0),   # a partial read: hashed
            (0x4000, 0, 64, 64, 0, 1, 1),    # NONE batch, recalculate of a full typed chunk: re-hashed
            (0x5000, 0, 64, 64, 0, 1, 0),    # NONE batch: nothing
            (0x6000, 0, 0, 64, 1, 0, 0)]     # nothing read
    legal, required = lf.read_ranges(recs, 1, [])
    assert [d for d, _ in required] == [0x2000, 0x3000, 0x4000]
    assert [d for d, _ in legal] == [0x1000, 0x2000, 0x3000, 0x4000, 0x5000]


def test_engine_allocations_and_payloads():
    legal, required = lf.engine_ranges([0x10000, 0x20005], 512, [(0x30000, 100, True), (0x31000, 50, False), (0x32000, 0, True)],
                                       [(0x40000, 56)])
    assert legal == [(0x10000, 512), (0x20005, 512), (0x30000, 100), (0x31000, 50), (0x40000, 56)]
    assert required == [(0x30000, 100)]      # a refused job's payload may be read, an applied one's must be


def test_empty_ranges_of_a_many_range_layout_share_one_region():
    y = lf.Yard(1 << 20)
    a = y.place("a", 100)
    spare = y.place_empties(40)
    b = y.place("b", 100)
    y.check()
    assert len(set(spare)) == 40 and {x % 16 for x in spare} == set(range(16))
    assert min(spare) - (a + 100) >= lf.GAP and b - max(spare) >= lf.GAP


def test_runs_round_trip():
    m = np.zeros(64, dtype=bool)
    s = np.zeros(64, dtype=np.uint8)
    m[[3, 4, 5, 9, 10]] = True
    s[[3, 4]] = 2
    s[5] = 3
    s[[9, 10]] = 2
    runs = lf.runs_of(m, s)
    assert runs == [[3, 2, 2], [5, 1, 3], [9, 2, 2]]
    m2, s2 = lf.mask_from_runs(runs, 64)
    assert np.array_equal(m, m2) and np.array_equal(s[m], s2[m])
    assert lf.runs_of(np.zeros(8, dtype=bool)) == []


# ---- compare() on fabricated reports ---------------------------------------------------------------
def _case():
    c = lf.Case("fabricated", 1 << 20)
    a = c.yard.place("a", 100, residue=7)          # granules of [a, a + 100)
    b = c.yard.place("b", 64, end_on_page=True)
    d = c.yard.place("desc", 32)
    c.legal, c.required = lf.list_ranges([a, b], [100, 64], [(d, 32)])
    c.yard.check()
    return c, a, b


def _report(case, extra=(), drop=(), **kw):
    m = case.required_mask()
    s = np.where(m, 2, 0).astype(np.uint8)
    for g, site in extra:
        m[g], s[g] = True, site
    for g in drop:
        m[g] = False
    r = dict(read=lf.runs_of(m, s), counters={"2": 10, "3": 2}, outside=0, desc=0, log=[], outputs="ok")
    r.update(kw)
    return r


def test_correct_report_passes():
    c, a, b = _case()
    assert lf.compare(c, _report(c)) == []
    assert a % 16 == 7 and (b + 64) % 4096 == 0


def test_one_granule_past_the_end():
    c, a, b = _case()
    g = (b + 64) >> 4          # the first granule of the page behind b
    (d,) = lf.compare(c, _report(c, extra=[(g, 4)]))
    assert (d["kind"], d["buffer"], d["distance"], d["site"], d["offset"]) == ("outside_legal", "b", 1, 4, g * 16)
    assert "+1 granules from b" in lf.describe(c, [d]) and "direct_pipe preload" in lf.describe(c, [d])


def test_one_granule_in_front():
    c, a, b = _case()
    (d,) = lf.compare(c, _report(c, extra=[((a >> 4) - 1, 3)]))
    assert (d["kind"], d["buffer"], d["distance"], d["site"]) == ("outside_legal", "a", -1, 3)


def test_granule_in_a_gap_next_to_no_buffer():
    c, a, b = _case()
    g = ((a + 100) >> 4) + 100   # 1600 bytes behind a, far in front of b
    (d,) = lf.compare(c, _report(c, extra=[(g, 2)]))
    assert d["kind"] == "outside_legal" and d["buffer"] is None and d["distance"] == 100
    assert "next to no buffer" in lf.describe(c, [d])


def test_required_granule_missing():
    c, a, b = _case()
    g = (a >> 4) + 2
    (d,) = lf.compare(c, _report(c, drop=[g]))
    assert (d["kind"], d["buffer"], d["distance"], d["granule"]) == ("required_missing", "a", 0, g)


def test_desc_hit():
    c, a, b = _case()
    entry = dict(address=3, bytes=0, site=lf.SITE_DESC, block=1, thread=64, yard_offset=-1)
    (d,) = lf.compare(c, _report(c, desc=1, log=[entry], counters={"2": 10, "17": 1}))
    assert d["kind"] == "desc" and d["count"] == 1 and d["log"] == [entry]


def test_out_of_yard_entry():
    c, a, b = _case()
    entry = dict(address=0xdead0000, bytes=16, site=2, block=0, thread=5, yard_offset=-4096)
    (d,) = lf.compare(c, _report(c, outside=1, log=[entry]))
    assert d["kind"] == "out_of_yard" and d["log"] == [entry]


def test_untagged_site_and_wrong_outputs():
    c, a, b = _case()
    kinds = [d["kind"] for d in lf.compare(c, _report(c, counters={"1": 4, "2": 1}, outputs="values differ"))]
    assert kinds == ["untagged_site", "outputs"]


def test_site_with_a_zero_counter():
    c, a, b = _case()
    reports = {"x": _report(c), "y": _report(c, counters={"14": 7})}
    got = lf.sites_reached(reports)
    assert got[2] == (10, "x") and got[14] == (7, "y") and 15 not in got
    missing = dict(lf.unreached(reports))
    assert 15 in missing and 2 not in missing and 14 not in missing
    assert 1 not in missing and 17 not in missing     # not to be reached: asserted zero per case
    full = {"z": _report(c, counters={str(k): 1 for k, v in lf.SITES.items() if v[1]})}
    assert lf.unreached(full) == []


def test_families_build_without_a_gpu():
    for family, build in lf.FAMILIES.items():
        cases = build()
        names = [c.name for c in cases]
        assert len(set(names)) == len(names), family
        for c in cases:
            assert c.yard.size <= 32 << 20
            legal, required = c.legal_mask(), c.required_mask()
            assert not (required & ~legal).any(), c.name
            for _, off, n in c.yard.bufs:     # every address handed out lies inside the yard
                assert lf.GAP <= off and off + n + lf.GAP <= c.yard.size, (c.name, off)
