"""The read footprint of the library's kernels (tests/test_gpu_load_footprint.py).

Every kernel that touches caller bytes promises to load only aligned 16-byte granules that hold at
least one byte of a range the call was given.  The load-checked build of the library
(3fs_amd/csrc/loadcheck.h, libhf3fs_crc_loadcheck.so) records the granules every such load touches.
This module holds

  * the yard: one allocation in which a case lays out every buffer it hands to the library, data
    and descriptor arrays alike, with at least GAP bytes of yard between any two and at both ends;
  * the two sets a call is held to, built from include/hf3fs_crc.h's contract alone (no kernel
    geometry): Legal, the granules of every range the entry point may read, and Required, the
    granules of every byte it must hash;
  * compare(): Required <= Read <= Legal, an empty out-of-yard log, no descriptor index >= n, and
    for every offending granule the nearest buffer, the distance and the load site;
  * the families of cases, and the child process (python tests/load_footprint.py FAMILY OUT) that
    runs one family against the check library and writes the report.

Families: list_grid, list_schedules, strided_blocks, records (scrub_batch, read_result_batch),
frames, md5, update (update_batch),
update_cow (update_cow_batch), update_ordered, update_versioned, update_engine.

The pure part (everything but run_family) needs neither a GPU nor the library;
tests/test_load_footprint_model.py checks it against hand-worked examples and fabricated reports.
"""
import hashlib
import json
import os
import sys

import numpy as np

G = 16            # granule
PAGE = 4096
GAP = 4096        # yard bytes between any two buffers and at both ends
NEAR = 64         # granules: a stray load further than one 1 KiB block from every buffer is "next to none"
CRC32C, CRC32 = 1, 2
M32 = 0xFFFFFFFF

# Load sites of the check build: LoadSite in 3fs_amd/csrc/loadcheck.h.  reach: must some case of
# tests/test_gpu_load_footprint.py reach it?  Where not, the reason.
SITES = {
    1: ("gload16", False, "the primitive's default id: every call site passes its own, so a count here is an untagged load"),
    2: ("gload16s/hash_grid", True, ""),
    3: ("gload16_masked", True, ""),
    4: ("direct_pipe preload", True, ""),
    5: ("range_stream produce", True, ""),
    6: ("frame stream", True, ""),
    7: ("frame pair (lin_t)", True, ""),
    8: ("ld16/copy_rows_shfl", True, ""),
    9: ("ld16_unaligned", True, ""),
    10: ("ldu16", True, ""),
    11: ("copy head/tail byte", True, ""),
    12: ("one-shot apply edge byte", True, ""),
    13: ("audit re-hash (lin_serial)", True, ""),
    14: ("md5 load_granules", True, ""),
    15: ("md5 staged row", True, ""),
    16: ("md5 byte cursor", True, ""),
    17: ("DESC", False, "a descriptor index >= n: asserted zero in every case"),
}
SITE_DESC = 17

# Sites that read wider than the granule rule by design: site id -> (reason, bound in bytes around a
# byte of the range).  Empty: every site is held to the granule rule.
WIDER_BY_DESIGN = {}


# ---- granule sets -------------------------------------------------------------------------------
def granule_span(p, n):
    """Granule indices [lo, hi) of the aligned granules that hold a byte of [p, p + n): the range
    [p & ~15, (p + n + 15) & ~15).  An empty range has none."""
    if n <= 0:
        return (0, 0)
    return (p >> 4, (p + n + 15) >> 4)


def mask_of(ranges, n_granules):
    m = np.zeros(n_granules, dtype=bool)
    for p, n in ranges:
        lo, hi = granule_span(int(p), int(n))
        assert hi <= n_granules, (p, n)
        m[lo:hi] = True
    return m


def runs_of(mask, sites=None):
    """[[first granule, count, site], ...] of the set granules (split where the site changes)."""
    idx = np.flatnonzero(mask)
    if idx.size == 0:
        return []
    s = sites[idx] if sites is not None else np.zeros(idx.size, dtype=np.uint8)
    brk = np.flatnonzero((np.diff(idx) != 1) | (np.diff(s) != 0)) + 1
    starts = np.concatenate(([0], brk))
    ends = np.concatenate((brk, [idx.size]))
    return [[int(idx[a]), int(b - a), int(s[a])] for a, b in zip(starts, ends)]


def mask_from_runs(runs, n_granules):
    m = np.zeros(n_granules, dtype=bool)
    s = np.zeros(n_granules, dtype=np.uint8)
    for g, c, site in runs:
        m[g:g + c] = True
        s[g:g + c] = site
    return m, s


# ---- the yard -----------------------------------------------------------------------------------
class Yard:
    """Offsets of buffers inside one allocation.  place() keeps `gap` bytes between neighbours."""

    def __init__(self, size):
        assert size <= 32 << 20 and size % PAGE == 0
        self.size = size
        self.cur = 0            # end of the last buffer
        self.bufs = []          # (name, offset, length)

    def place(self, name, length, residue=0, align=16, end_on_page=False, start_on_page=False):
        lo = self.cur + GAP
        if start_on_page:
            off = -(-lo // PAGE) * PAGE
        elif end_on_page:
            off = -(-(lo + length) // PAGE) * PAGE - length
        else:
            off = -(-lo // align) * align + residue
        self.bufs.append((name, off, int(length)))
        self.cur = off + int(length)
        assert self.cur + GAP <= self.size, f"yard of {self.size} B is full at {name}"
        return off

    def place_empties(self, count):
        """Addresses for `count` zero-length ranges: one region of the yard (GAP from its neighbours)
        that no range may read, an address every 16 bytes at a residue that walks through 0..15."""
        at = self.place("addresses of empty ranges", 16 * count + 16)
        return [at + 16 * i + i % 16 for i in range(count)]

    def check(self):
        self.size = min(self.size, -(-(self.cur + GAP) // PAGE) * PAGE)   # no larger than the case needs
        prev = 0
        for _, off, n in sorted(self.bufs, key=lambda b: b[1]):
            assert off - prev >= GAP, (off, prev)
            prev = off + n
        assert self.size - prev >= GAP


def nearest(bufs, g):
    """(buffer name, signed granule distance) of granule g to the nearest buffer: 0 inside its
    granules, +k: k granules past its last one, -k: k in front of its first one.  A granule
    further than NEAR granules from every buffer is next to none: (None, distance)."""
    best = None
    for name, off, n in bufs:
        lo, hi = granule_span(off, max(n, 1))
        d = 0 if lo <= g < hi else (g - (hi - 1) if g >= hi else g - lo)
        if best is None or abs(d) < abs(best[1]):
            best = (name, d)
    if best is None or abs(best[1]) > NEAR:
        return (None, best[1] if best else 0)
    return best


# ---- a case: what one call is given, and what it may and must read -----------------------------
class Case:
    """name, yard, legal / required: lists of (yard offset, length) byte ranges."""

    def __init__(self, name, yard_bytes):
        self.name = name
        self.yard = Yard(yard_bytes)
        self.legal = []
        self.required = []
        self.switches = {}
        self.fill = []   # (offset, bytes-like or ndarray): what the child writes over the random image

    @property
    def n_granules(self):
        return self.yard.size // G

    def legal_mask(self):
        return mask_of(self.legal, self.n_granules)

    def required_mask(self):
        return mask_of(self.required, self.n_granules)


def compare(case, report, max_listed=8):
    """The defects of one call's report against its case: a list of dicts
    {kind, granule, offset, buffer, distance, site}.  Empty: Required <= Read <= Legal, nothing
    refused, no descriptor index out of range, outputs equal to the oracle's."""
    n = case.n_granules
    read, sites = mask_from_runs(report["read"], n)
    legal, required = case.legal_mask(), case.required_mask()
    out = []

    def granule_defects(kind, mask):
        idx = np.flatnonzero(mask)
        for g in idx[:max_listed]:
            name, d = nearest(case.yard.bufs, int(g))
            out.append(dict(kind=kind, granule=int(g), offset=int(g) * G, buffer=name, distance=d,
                            site=int(sites[g]), site_name=SITES.get(int(sites[g]), ("?",))[0], more=int(idx.size)))

    granule_defects("outside_legal", read & ~legal)
    granule_defects("required_missing", required & ~read)
    if report["desc"]:
        out.append(dict(kind="desc", count=int(report["desc"]), log=report["log"][:4]))
    if report["outside"]:
        out.append(dict(kind="out_of_yard", count=int(report["outside"]),
                        log=[e for e in report["log"] if e["site"] != SITE_DESC][:4]))
    if report["counters"].get("1", 0):
        out.append(dict(kind="untagged_site", count=int(report["counters"]["1"])))
    if report.get("outputs") != "ok":
        out.append(dict(kind="outputs", detail=report.get("outputs")))
    return out


def describe(case, defects):
    lines = [f"{case.name}: {len(defects)} defect(s), switches {case.switches}"]
    for d in defects:
        if "granule" in d:
            where = (f"{d['distance']:+d} granules from {d['buffer']}" if d["buffer"] else
                     f"next to no buffer (nearest {d['distance']:+d} granules away)")
            lines.append(f"  {d['kind']}: yard +{d['offset']:#x} ({where}), site {d['site']} {d['site_name']}"
                         f" [{d['more']} such granules]")
        else:
            lines.append(f"  {d}")
    return "\n".join(lines)


def sites_reached(reports):
    """{site id: (count, first case that reached it)} over {case name: report}."""
    got = {}
    for name, r in reports.items():
        for k, c in r["counters"].items():
            if c and int(k) not in got:
                got[int(k)] = (int(c), name)
    return got


def unreached(reports):
    got = sites_reached(reports)
    return [(k, SITES[k][0]) for k in sorted(SITES) if SITES[k][1] and k not in got]


# ---- the contract's ranges (include/hf3fs_crc.h) ------------------------------------------------------
def list_ranges(offs, lens, desc):
    """create_batch / verify_batch / verify_blocks: range i is [addr_i, addr_i + len_i), all of it
    hashed; desc: (offset, bytes) of the n-element arrays the call reads."""
    data = [(int(o), int(n)) for o, n in zip(offs, lens) if n]
    return data + list(desc), data


def update_io_ranges(chunk, payload, offset, length, chunk_size, update_type_write=True, verified=True):
    """hf3fs_crc_update_io: the chunk [chunk, chunk + max(chunk_size, offset + length)) may be read
    (which old bytes a mode reads is its choice), the payload [payload, payload + length) of a
    verified write must be."""
    if not update_type_write:
        return [(chunk, chunk_size)], []
    legal = [(chunk, max(chunk_size, offset + length)), (payload, length)]
    return legal, ([(payload, length)] if verified and length else [])


def scrub_ranges(datas, lens, types, fins, ctype, max_len, desc):
    """hf3fs_crc_scrub_batch: the chunk bytes [data, data + length) of a well-formed record (type NONE
    or the batch's, fin <= 1, length <= max_len) may be read, those of a typed one must be hashed;
    a malformed record is refused unread."""
    legal, required = [], []
    for d, n, t, f in zip(datas, lens, types, fins):
        d, n, t, f = int(d), int(n), int(t), int(f)
        if t not in (0, ctype) or f > 1 or n > max_len or not n:
            continue
        legal.append((d, n))
        if t == ctype:
            required.append((d, n))
    return legal + list(desc), required


def read_ranges(recs, ctype, desc):
    """hf3fs_crc_read_result_batch: [data, data + length) are the read bytes.  They must be hashed
    when the batch asks for a checksum that the chunk's stored one cannot serve (not a full-chunk
    read of the stored type), and when `recalculate` re-hashes a full-chunk read of a typed chunk;
    otherwise nothing has to be read.  recs: (data, offset, length, chunk_len, batch type, chunk
    type, recalculate)."""
    legal, required = [], []
    for d, off, n, cl, bt, ct, rc in recs:
        d, off, n, cl, bt, ct, rc = (int(x) for x in (d, off, n, cl, bt, ct, rc))
        if not n:
            continue
        legal.append((d, n))
        full = off == 0 and n == cl
        if (bt != 0 and not (full and bt == ct)) or (rc and full and ct != 0):
            required.append((d, n))
    return legal + list(desc), required


def md5_ranges(segs, seg_desc):
    """hf3fs_crc_md5_batch (INIT | FINAL): every segment with data != 0 is read whole; a hole
    (data == 0) is no range."""
    data = [(int(a), int(n)) for a, n in segs if a and n]
    return data + list(seg_desc), data


def frame_ranges(buf, offsets, sizes, max_size, desc):
    """hf3fs_crc_frame_verify_batch: a frame is its MessageHeader, the 8 bytes of the receive buffer
    at offset - 8 (hf3fs_crc_frame.offset: "header at offset - 8"), and its payload
    [offset, offset + size).  The payload of a frame with size <= max_size must be hashed; the
    header may be read (the stream path hashes the buffer across the headers between neighbouring
    payloads); nothing of an oversize frame's payload may be."""
    legal, required = [], []
    for o, n in zip(offsets, sizes):
        o, n = int(o), int(n)
        ok = n <= max_size
        legal.append((buf + o - 8, 8 + (n if ok else 0)))
        if ok and n:
            required.append((buf + o, n))
    return legal + list(desc), required


# ---- families -------------------------------------------------------------------------------------
# A family is a list of Case objects with the attributes its runner needs; built without a GPU, the
# same in the parent and in the child (fixed seeds).
def _desc(case, name, nbytes):
    off = case.yard.place(name, max(nbytes, 1))
    return off


def _list_case(name, specs, verify=False, arena=False, ctype=CRC32C, switches=None, yard_bytes=8 << 20, max_len=None,
               seed=1, empties_apart=True):
    """specs: (length, placement kwargs) per range, in order.  empties_apart=False: the zero-length
    ranges of a many-range layout take their addresses from one region of their own (they are no
    buffers: nothing of them may be read), so that every range with bytes keeps GAP to its neighbours."""
    c = Case(name, yard_bytes)
    c.kind = "blocks" if arena else "list"
    c.verify, c.ctype, c.switches, c.seed = verify, ctype, dict(switches or {}), seed
    offs, lens = [], []
    spare = [] if empties_apart else c.yard.place_empties(sum(1 for n, _ in specs if not n))
    for i, (n, kw) in enumerate(specs):
        offs.append(spare.pop() if not n and not empties_apart else c.yard.place(f"range{i}", n, **kw))
        lens.append(n)
    c.offs, c.lens = np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint64)
    n = len(specs)
    c.max_len = int(max_len if max_len is not None else max(lens + [1]))
    ew = 4 if arena else 8
    c.d_addrs = _desc(c, "addrs", 8 * n)
    c.d_lens = _desc(c, "lens", ew * n)
    desc = [(c.d_addrs, 8 * n), (c.d_lens, ew * n)]
    if verify:
        c.d_expected = _desc(c, "expected", 4 * n)
        c.d_mismatch = _desc(c, "mismatch", n)
        c.d_count = _desc(c, "count", 4)
        c.d_computed = _desc(c, "computed", 4 * n)
        desc.append((c.d_expected, 4 * n))
    else:
        c.d_starts = _desc(c, "starts", 4 * n)
        c.d_out = _desc(c, "out", 4 * n)
        desc.append((c.d_starts, 4 * n))
    c.legal, c.required = list_ranges(c.offs, c.lens, desc)
    c.yard.check()
    return c


def _strided_case(name, n, length, stride, residue, verify=False, switches=None, yard_bytes=32 << 20, align=16):
    c = Case(name, yard_bytes)
    c.kind = "strided"
    c.verify, c.ctype, c.switches, c.seed = verify, CRC32C, dict(switches or {}), 3
    c.n, c.length, c.stride = n, length, stride
    c.base = c.yard.place("strided", (n - 1) * stride + length if n else 0, residue=residue, align=align)
    assert align == 16 or stride % align == 0
    c.d_out = _desc(c, "out", 4 * max(n, 1))
    c.d_mismatch = _desc(c, "mismatch", max(n, 1))
    c.d_count = _desc(c, "count", 4)
    data = [(c.base + i * stride, length) for i in range(n) if length]
    desc = []
    if verify:
        c.d_expected = _desc(c, "expected", 4 * n)
        desc = [(c.d_expected, 4 * n)]
    c.legal, c.required = data + desc, data
    c.yard.check()
    return c


GRID_BLOCKS = (1, 2, 4, 5, 8, 9, 64, 65)
GRID_ROWS = ({}, {"static": "1"}, {"pipe": "0"}, {"pipe": "1"}, {"seg_kib": "1"}, {"seg_kib": "4"},
             {"list_runs": "1", "prehash_rep": "1"}, {"list_runs": "1", "prehash_rep": "8"}, {"nt": "0"},
             {"balance": "0"}, {"range_stream": "1"})


def _grid_specs(nb):
    """Every start residue x every end residue at nb 1 KiB blocks of the end-aligned grid, the
    lengths 0, 1, 3, 4, the spill starts, ranges that end / start on a page, and runs of empty
    ranges (1, 63, 64, 65) between non-empty ones."""
    specs = []
    for rs in range(16):
        for re_ in range(16):
            # granules from the start's to the end's: (nb - 1) KiB + one granule .. nb KiB
            n = (nb - 1) * 1024 + 16 + ((re_ - rs) % 16 or 16) if nb > 1 else 16 + ((re_ - rs) % 16 or 16)
            specs.append((n, dict(residue=rs)))
    for n in (0, 1, 3, 4):
        for rs in (0, 1, 13, 15):
            specs.append((n, dict(residue=rs)))
    for r, k in ((1, 1), (2, 1), (3, 2), (3, 1)):   # the start in the last three bytes of a block
        specs.append((1024 * k + r - 5, dict(residue=16 - r)))
    for n in (nb * 1024, nb * 1024 - 7, 5):
        specs.append((n, dict(end_on_page=True)))
        specs.append((n, dict(start_on_page=True)))
    return specs


def _with_empty_runs(specs):
    out = list(specs[:8])
    for run in (1, 63, 64, 65):
        out += [(0, dict(residue=5))] * run
        out.append((700, dict(residue=run % 16)))
    return out


def _tag(sw):
    return ",".join(f"{a}={b}" for a, b in sw.items()) or "default"


def family_list_grid():
    """create_batch and verify_batch over the whole residue grid at every block count, each under
    every list switch row (so the grid runs through every list schedule; the 64- and 65-block
    grids, 19 MiB each, under three), and runs of empty ranges for both."""
    cases = []
    for k, nb in enumerate(GRID_BLOCKS):
        specs = _grid_specs(nb)
        big = nb >= 64
        rows = GRID_ROWS if not big else GRID_ROWS[:2] + GRID_ROWS[4:5]
        for sw in rows:
            cases.append(_list_case(f"create_batch[grid nb={nb} {_tag(sw)}]", specs, switches=sw, yard_bytes=32 << 20, seed=k))
            cases.append(_list_case(f"verify_batch[grid nb={nb} {_tag(sw)}]", specs, verify=True, switches=sw,
                                    yard_bytes=32 << 20, seed=k))
    specs = _with_empty_runs(_grid_specs(2))
    for sw in ({}, {"list_runs": "1", "prehash_rep": "1"}, {"list_runs": "1", "prehash_rep": "8"}, {"static": "1"}):
        cases.append(_list_case(f"create_batch[empty runs {_tag(sw)}]", specs, switches=sw, seed=9))
        cases.append(_list_case(f"verify_batch[empty runs {_tag(sw)}]", specs, verify=True, switches=sw, seed=9))
    cases.append(_list_case("create_batch[grid nb=2 crc32]", _grid_specs(2), ctype=CRC32, seed=11))
    return cases


def _layout_specs(layout, cus, seed):
    """The lengths and residues of a tests/batch_cases.py layout built for `cus` compute units (the
    count that sets its number of ranges), to be laid out in the yard."""
    import batch_cases as bc
    rng = np.random.default_rng(seed)
    lens, offs, max_len, _ = getattr(bc, layout)(cus, rng, 1)
    wide = len(lens) < 1000   # residues mod 128 (the segmented parts' grid alignment) where there is room
    specs = [(int(n), dict(residue=int(o) % (128 if wide else 16), align=128 if wide else 16)) for n, o in zip(lens, offs)]
    return specs, int(max_len)


# layout -> (compute units it is built for, switch rows).  The range counts are scaled to the yard so
# that every range with bytes keeps GAP to its neighbours: 4,157 ranges of 0-300 bytes (direct
# ticketed, direct_pipe, byte runs), 2,045 of 0-2,048 (direct_pipe, direct_static), about 100 ragged
# ones (the segmented schedules); the balanced layout keeps its 65,597 ranges, which the balanced
# schedules need on 256 compute units, because all but about 800 of them are empty.
LAYOUT_ROWS = {"_ragged_layout": (256, GRID_ROWS),
               "_small_many_layout": (16, ({}, {"static": "1"}, {"pipe": "0"}, {"list_runs": "1", "prehash_rep": "8"})),
               "_balanced_layout": (256, ({}, {"balance": "0"}, {"range_stream": "1"})),
               "_ticketed_layout": (16, ({}, {"static": "1"}, {"pipe": "0"}, {"pipe": "1"}))}


def family_list_schedules():
    """The layouts of tests/batch_cases.py scaled to the yard under its list switch rows; n is no
    multiple of the wave count (three ranges dropped), so the last stride step and the last ticket
    pass n."""
    cases = []
    for layout, (cus, sws) in LAYOUT_ROWS.items():
        specs, max_len = _layout_specs(layout, cus, 5)
        if layout != "_ragged_layout":
            specs = specs[:-3]
        apart = layout != "_balanced_layout"
        for sw in sws:
            cases.append(_list_case(f"create_batch[{layout.strip('_')} {_tag(sw)}]", specs, switches=sw,
                                    yard_bytes=32 << 20, max_len=max_len, seed=21, empties_apart=apart))
        cases.append(_list_case(f"verify_batch[{layout.strip('_')}]", specs, verify=True, yard_bytes=32 << 20,
                                max_len=max_len, seed=22, empties_apart=apart))
    return cases


def family_strided_blocks(cus=256):
    """create_strided / verify_strided (whole buffers, segmented, empty) and verify_blocks."""
    cases = []
    seg = 200 * 1024 + 13
    for sw in ({}, {"seg_kib": "1"}, {"seg_kib": "64"}, {"static": "1"}, {"pipe": "0"}, {"nt": "0"}):
        tag = _tag(sw)
        for r in (range(16) if not sw else (0, 1, 15)):
            cases.append(_strided_case(f"create_strided[5 x {seg} r{r} {tag}]", 5, seg, seg + 4096 + 3, r, switches=sw))
        # around seg_bytes and 1 KiB multiples past a start that is not 128-byte (kGridAlign) aligned:
        # the part's grid start vs lies in front of the buffer and its end vend behind it
        for length in (65536 - 1, 65536 + 1, 3 * 1024 + 128 - 1, 3 * 1024 + 128 + 1, 1024 * 67 + 5):
            for r in (125, 1, 127):
                cases.append(_strided_case(f"create_strided[3 x {length} r{r}/128 {tag}]", 3, length,
                                           (length + 4096 + 127) // 128 * 128, r, switches=sw, align=128))
        cases.append(_strided_case(f"create_strided[{16 * cus + 7} x 100 {tag}]", 16 * cus + 7, 100, 100 + 4096 + 12, 3,
                                   switches=sw))
    cases.append(_strided_case("create_strided[3 x 0]", 3, 0, 64, 5))
    for r in range(16):
        cases.append(_strided_case(f"verify_strided[7 x 70 KiB + 5 r{r}]", 7, 70 * 1024 + 5, 70 * 1024 + 5 + 4096 + 6, r,
                                   verify=True))
    for k, nb in enumerate((1, 4, 9, 65)):
        specs = _grid_specs(nb)
        for sw in ({}, {"balance": "0"}, {"range_stream": "1"}):
            cases.append(_list_case(f"verify_blocks[grid nb={nb} {_tag(sw)}]", specs, verify=True, arena=True, switches=sw,
                                    yard_bytes=32 << 20, seed=30 + k))
    specs = _with_empty_runs(_grid_specs(2))
    cases.append(_list_case("verify_blocks[empty runs]", specs, verify=True, arena=True, seed=39))
    specs, max_len = _layout_specs("_balanced_layout", cus, 7)
    for sw in ({}, {"range_stream": "1"}):
        cases.append(_list_case(f"verify_blocks[balanced {_tag(sw)}]", specs[:-3], verify=True, arena=True, switches=sw,
                                yard_bytes=32 << 20, max_len=max_len, seed=40, empties_apart=False))
    return cases


RECORD_ROWS = ({}, {"static": "1"}, {"record_direct": "0"}, {"pipe": "0"}, {"pipe": "1"}, {"seg_kib": "1"}, {"nt": "0"})


def _record_case(name, kind, specs, switches, seed):
    """scrub_batch / read_result_batch over ranges laid out like a list case's; the records' other
    fields walk through their flavours by index."""
    import batch_cases as bc
    c = Case(name, 32 << 20)
    c.kind, c.switches, c.seed = kind, dict(switches), seed
    c.offs = [c.yard.place(f"range{i}", n, **kw) for i, (n, kw) in enumerate(specs)]
    c.lens = [n for n, _ in specs]
    n = len(specs)
    c.max_len = max(c.lens + [1])
    k = np.arange(n)
    if kind == "scrub":
        r = np.zeros(n, dtype=bc.SCRUB_DT)
        r["data"], r["length"] = c.offs, c.lens
        r["checksum_type"] = np.where(k % 9 == 8, 0, CRC32C)
        r["fin"] = k % 2
        r["checksum_type"][5::41] = CRC32   # malformed: not the batch's type
        r["fin"][7::43] = 7                 # malformed
        c.d_recs = _desc(c, "scrub records", r.nbytes)
        c.d_count = _desc(c, "count", 4)
        c.legal, c.required = scrub_ranges(r["data"], r["length"], r["checksum_type"], r["fin"], CRC32C, c.max_len,
                                           [(c.d_recs, r.nbytes)])
    else:
        r = np.zeros(n, dtype=bc.READ_DT)
        kind6 = k % 6   # 0 NONE batch, 1 hashed full read of an untyped chunk, 2 / 3 recalculate, 4 partial, 5 reuse
        r["data"], r["length"] = c.offs, c.lens
        r["offset"] = np.where(kind6 == 4, 5, 0)
        r["chunk_len"] = np.where(kind6 == 4, r["length"] + 14, r["length"])
        r["batch_checksum_type"] = np.where(kind6 == 0, 0, CRC32C)
        r["chunk_checksum_type"] = np.where(kind6 == 1, 0, CRC32C)
        r["recalculate"] = np.isin(kind6, (0, 2, 3))
        c.d_recs = _desc(c, "read records", r.nbytes)
        c.legal, c.required = read_ranges(zip(r["data"], r["offset"], r["length"], r["chunk_len"], r["batch_checksum_type"],
                                              r["chunk_checksum_type"], r["recalculate"]), CRC32C, [(c.d_recs, r.nbytes)])
    c.recs = r
    c.yard.check()
    return c


def family_records():
    """scrub_batch and read_result_batch over the whole residue grid at every block count, the
    runs of empty ranges, under the record switch rows (the 64- and 65-block grids under two)."""
    cases = []
    for k, nb in enumerate(GRID_BLOCKS):
        for sw in (RECORD_ROWS if nb < 64 else RECORD_ROWS[:1] + RECORD_ROWS[2:3]):
            for kind in ("scrub", "read"):
                cases.append(_record_case(f"{kind}[grid nb={nb} {_tag(sw)}]", kind, _grid_specs(nb), sw, 80 + k))
    for kind in ("scrub", "read"):
        for sw in RECORD_ROWS[:3]:
            cases.append(_record_case(f"{kind}[empty runs {_tag(sw)}]", kind, _with_empty_runs(_grid_specs(2)), sw, 89))
    return cases


def _md5_case(name, files, switches, seed, yard_bytes=32 << 20):
    """files: list of lists of (length, residue or None for a hole, kwargs)."""
    c = Case(name, yard_bytes)
    c.kind, c.switches, c.seed = "md5", dict(switches), seed
    segs, c.files = [], []
    for f in files:
        this = []
        for n, r, kw in f:
            off = None if r is None else c.yard.place(f"seg{len(segs)}", n, residue=r, **kw)
            segs.append((off, n))
            this.append((off, n))
        c.files.append(this)
    c.segs = segs
    c.d_segs = _desc(c, "segs", 16 * len(segs))
    c.d_off = _desc(c, "file_off", 8 * (len(files) + 1))
    c.d_out = _desc(c, "out", 16 * len(files))
    c.legal, c.required = md5_ranges([(0 if o is None else o + 1, n) for o, n in segs], [])
    # (offsets + 1 only so that offset 0 is not taken for a hole; undone here)
    c.legal = [(o - 1, n) for o, n in c.legal] + [(c.d_segs, 16 * len(segs)), (c.d_off, 8 * (len(files) + 1))]
    c.required = [(o - 1, n) for o, n in c.required]
    c.yard.check()
    return c


def family_md5():
    """md5_batch: every address residue x lengths 0-200, segments that end 1-15 bytes into a granule,
    pieces around 256 bytes, a segment boundary inside a block, holes; all four md5_stage x md5_sort."""
    cases = []
    for stage in ("0", "1"):
        for sort in ("0", "1"):
            sw = {"md5_stage": stage, "md5_sort": sort}
            tag = f"stage={stage} sort={sort}"
            files = [[(n, r, {})] for r in range(16) for n in range(201)]
            cases.append(_md5_case(f"md5_batch[lengths 0-200 {tag}]", files, sw, 50))
            files = [[(n, r, {})] for r in range(16) for n in (64, 64 + 15 - r, 128 + (16 - r) % 16 + 1, 200)]
            files += [[(n, r, {})] for r in (0, 1, 15) for n in (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4097)]
            files += [[(n, r, dict(end_on_page=True))] for r in (0,) for n in (64, 65, 100, 256, 300)]
            files += [[(n, 0, dict(start_on_page=True))] for n in (64, 79, 257)]
            cases.append(_md5_case(f"md5_batch[edges {tag}]", files, sw, 51))
            files = []
            for cut in (1, 17, 63, 64, 65, 100):   # a boundary inside a block, scattered pieces
                files.append([(cut, 3, {}), (300 - cut, 9, {})])
            for hole in (1, 63, 64, 65, 5000):
                files.append([(70, 1, {}), (hole, None, {}), (130, 15, {})])
            files.append([(0, 4, {}), (64, 2, {}), (0, 7, {})])
            files.append([])
            cases.append(_md5_case(f"md5_batch[boundaries and holes {tag}]", files, sw, 52))
    return cases


def _update_case(name, ios, mode, pipeline, seed, max_len, yard_bytes=32 << 20, entry="update_batch", nt=6, max_rounds=0):
    """ios: dicts(kind W/T/E, size, off, len, dst_res, src_res, bad, place kwargs; update_ordered:
    chunk_id, IOs of one id share a chunk and are applied in index order, at most max_rounds of
    them; update_cow_batch: dst "none" / "same" (in place) or "new" with new_res).  The sizes a
    chain of IOs leaves are followed here (no bytes), because they bound what may be read."""
    c = Case(name, yard_bytes)
    c.kind, c.mode, c.pipeline, c.seed, c.max_len, c.entry, c.nt = "update", mode, pipeline, seed, max_len, entry, nt
    c.max_rounds, c.ctype = max_rounds, CRC32C
    c.ios = []
    chunks = {}    # chunk_id -> [address, size, IOs seen]
    for i, io in enumerate(ios):
        io = dict(io)
        write = io["kind"] == "W"
        io["pay_at"] = c.yard.place(f"payload{i}", io["len"], residue=io.get("src_res", 0), **io.get("pay_kw", {})) \
            if write else 0
        cid = io.get("chunk_id", ("own", i))
        if cid not in chunks:
            at = c.yard.place(f"chunk{i}", max_len, residue=io.get("dst_res", 0), **io.get("chunk_kw", {}))
            chunks[cid] = [at, io["size"], 0]
        st = chunks[cid]
        io["chunk_at"], io["size"], io["round"] = st[0], st[1], st[2]
        st[2] += 1
        io["applied"] = not max_rounds or io["round"] < max_rounds
        if io["off"] < 0:
            io["off"] = io["size"]     # an append to what the chain has left
        span = max(io["size"], io["off"] + io["len"]) if write else max(io["size"], io["len"])
        assert span <= max_len
        if io["applied"] and not io.get("bad"):
            st[1] = span if write or io["kind"] == "E" else io["len"]
        io["dst_at"] = c.yard.place(f"destination{i}", max(span, 1), residue=io.get("new_res", 0)) if io.get("dst") == "new" else 0
        c.ios.append(io)
        if write:
            lg, rq = update_io_ranges(io["chunk_at"], io["pay_at"], io["off"], io["len"], io["size"], verified=io["applied"])
        else:
            lg, rq = update_io_ranges(io["chunk_at"], 0, 0, 0, max(io["size"], io["len"]), update_type_write=False)
        if io["dst_at"]:      # "dst has capacity >= max(chunk_size, offset + length)": REFERENCE hashes the new image there
            lg.append((io["dst_at"], span))
        c.legal += lg
        c.required += rq
    c.d_ios = _desc(c, "ios", 56 * len(ios))
    c.legal.append((c.d_ios, 56 * len(ios)))
    if entry == "update_cow":
        c.d_dst = _desc(c, "destinations", 8 * len(ios))
        c.legal.append((c.d_dst, 8 * len(ios)))
    if entry == "update_ordered":
        c.d_info = _desc(c, "info", 8)
    if entry == "update_versioned":
        c.d_ver = _desc(c, "version records", 48 * len(ios))
        c.d_info = _desc(c, "info", 32)
        c.legal.append((c.d_ver, 48 * len(ios)))
    c.yard.check()
    return c


def update_variants():
    """(pipeline, apply_nt, mode, checksum type): the rows of tests/test_gpu_update_footprint.py, one
    per compiled copy body and mode, CRC32 where the kernel is templated on the polynomial; and the
    plain three-pass pipeline."""
    from test_gpu_update_footprint import VARIANTS
    return list(VARIANTS) + [("unfused", 6, mode, CRC32C) for mode in (0, 1)]


WRITE_LENGTHS = (1, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193)


def _update_ios():
    ios = []
    for k, ln in enumerate(WRITE_LENGTHS):
        for j in range(4):
            sr, dr = (5 * k + 3 * j) % 16, (7 * k + 11 * j + 1) % 16
            size = (12 << 10) + 37 * k
            off = (k * 131 + j * 1021) % (size - 1)
            ios.append(dict(kind="W", size=size, off=off, len=ln, src_res=sr, dst_res=dr))
    for r in range(16):   # every source residue against destination residue 0 and the reverse
        ios.append(dict(kind="W", size=4096, off=16, len=2048 + r, src_res=r, dst_res=0))
        ios.append(dict(kind="W", size=4096, off=r, len=2048, src_res=0, dst_res=r))
    for ng in (831, 832, 833, 1856):   # around the first whole row of copy_range's lane-shuffle rows (4 x 256 granules)
        ios.append(dict(kind="W", size=20000, off=3 + ng % 7, len=16 * ng + 17, src_res=5 + ng % 3, dst_res=2))
        ios.append(dict(kind="W", size=100, off=0, len=16 * ng + 1, src_res=0, dst_res=0))
    ios.append(dict(kind="W", size=5000, off=4990, len=3000, src_res=3, dst_res=9))     # offset + length > chunk_size
    ios.append(dict(kind="W", size=0, off=0, len=777, src_res=1, dst_res=2))
    ios.append(dict(kind="T", size=9000, off=0, len=1234, dst_res=7))
    ios.append(dict(kind="E", size=1000, off=0, len=9001, dst_res=8))
    ios.append(dict(kind="W", size=8192, off=0, len=4096, pay_kw=dict(end_on_page=True), chunk_kw=dict(start_on_page=True)))
    ios.append(dict(kind="W", size=6000, off=100, len=3000, src_res=6, dst_res=1, bad=True))
    return ios


def family_update():
    """update_batch in both modes under every pipeline / apply row of tests/update_footprint.py:
    source x destination residues mod 16, the write lengths, truncate and extend, a write past the
    chunk's size, the payload directly before a gap and the chunk directly after one, and one
    write with a wrong client checksum (the audit's re-hash)."""
    cases = []
    max_len = 40 << 10
    ios = _update_ios()
    for pipeline, nt, mode, ctype in update_variants():
        c = _update_case(f"update_batch[{'delta' if mode else 'reference'} {pipeline} nt{nt} "
                         f"{'crc32c' if ctype == CRC32C else 'crc32'}]", ios, mode, pipeline, 60 + mode, max_len, nt=nt)
        c.ctype = ctype
        cases.append(c)
    return cases


def family_update_cow():
    """update_cow_batch: update_batch's IOs, a third of them in place without a destination, a
    third with the chunk as destination, a third out of place at every destination residue against
    the chunk's; both modes, 4 / 8 / 16 KiB pieces, the looping grid, both load forms, CRC32."""
    ios = []
    for i, io in enumerate(_update_ios()):
        ios.append(dict(io, dst=("none", "new", "same")[i % 3], new_res=(i // 3 * 5 + 3) % 16))
    cases = []
    for mode in (0, 1):
        for pipeline, nt, ctype in (("oneshot4", 0, CRC32C), ("oneshot8", 1, CRC32C), ("oneshot16", 0, CRC32C),
                                    ("oneshot_loop", 1, CRC32C), ("oneshot8", 0, CRC32)):
            c = _update_case(f"update_cow_batch[{'delta' if mode else 'reference'} {pipeline} nt{nt} "
                             f"{'crc32c' if ctype == CRC32C else 'crc32'}]", ios, mode, pipeline, 64 + mode, 40 << 10,
                             entry="update_cow", nt=nt)
            c.ctype = ctype
            cases.append(c)
    return cases


def _ordered_chains(with_failures):
    chains = []
    for cid in range(40):
        depth, size, chain = 1 + cid % 6, (cid * 517) % 6000, []
        for k in range(depth):
            j = cid * 7 + k
            if j % 11 == 5:
                chain.append(dict(kind="T" if j % 2 else "E", off=0, len=(j * 701) % 9000))
            else:
                ln = WRITE_LENGTHS[j % len(WRITE_LENGTHS)]
                chain.append(dict(kind="W", off=(j * 389) % 12000 if k % 2 else -1, len=ln, src_res=j % 16, bad=with_failures and j % 17 == 9))
        chains.append([dict(io, chunk_id=cid, size=size, dst_res=(cid * 3) % 16) for io in chain])
    ios = []
    for k in range(6):          # round-robin: the IOs of a chunk are spread over the batch
        ios += [ch[k] for ch in chains if k < len(ch)]
    return ios


def family_update_versioned():
    """update_versioned: update_ordered's chains (without the failing write: a refused job would
    leave its successors a version short) behind version records that admit every job -- CLEAN
    chunks, io_ver = update_ver + 1 down each chain."""
    ios = _ordered_chains(False)
    cases = []
    for mode in (0, 1):
        for pipeline, nt in (("unfused", 6), ("fused", 6), ("oneshot8", 6), ("ticketed", 0)):
            cases.append(_update_case(f"update_versioned[{'delta' if mode else 'reference'} {pipeline}]", ios, mode, pipeline,
                                      68 + mode, 64 << 10, entry="update_versioned", nt=nt, max_rounds=4))
    return cases


def family_update_ordered():
    """update_ordered: chains of 1 to 6 IOs per chunk, interleaved, at most four applied per call
    (the others come back NOT_APPLIED and their payloads need not be read); writes at every source
    and destination residue, appends, writes past the size, truncates, extends and a wrong client
    checksum inside a chain; both modes under the default, fused, one-shot and ticketed rows."""
    ios = _ordered_chains(True)
    cases = []
    for mode in (0, 1):
        for pipeline, nt in (("unfused", 6), ("fused", 6), ("oneshot8", 6), ("ticketed", 0)):
            cases.append(_update_case(f"update_ordered[{'delta' if mode else 'reference'} {pipeline}]", ios, mode, pipeline,
                                      66 + mode, 64 << 10, entry="update_ordered", nt=nt, max_rounds=4))
    return cases


def engine_ranges(regions, max_len, payloads, desc):
    """hf3fs_crc_update_engine: a job names allocations of max_len bytes each -- the committed
    version (`chunk` / addr), the writing version (w_addr) and a destination ("capacity >= max_len")
    -- and a payload [payload, payload + length).  Any byte of a named allocation may be read; the
    payload of a write the call applies must be.  regions: allocation addresses; payloads:
    (address, length, applied)."""
    legal = [(int(r), max_len) for r in regions] + [(int(p), int(n)) for p, n, _ in payloads if n]
    return legal + list(desc), [(int(p), int(n)) for p, n, ok in payloads if n and ok]


_ENGINE_BUILT = {}


def _engine_built(name):
    """A case of tests/engine_cases.py (its queue, records, bytes and the model's outcome), built once."""
    if name not in _ENGINE_BUILT:
        import engine_cases as ec
        import oracle
        oracle.lib()
        _ENGINE_BUILT[name] = ec.all_cases(oracle)[name]()
    return _ENGINE_BUILT[name]


ENGINE_CASES = ("singles_512", "chains_512", "overflow_512", "distinct_512", "random_512_e7a1", "random_512_e7a2",
                "random_512_e7a3", "singles_131072", "chains_131072", "overflow_131072")
ENGINE_ROWS = ({}, {"apply_piece_kib": "4"}, {"apply_piece_kib": "16"}, {"apply_grid": "2"})


def family_update_engine():
    """update_engine: the update and commit queues of tests/engine_cases.py (single jobs of every
    kind, chains, chains past max_rounds, distinct chunks, random queues; 512-byte and 128 KiB
    allocations), every allocation and payload of the case moved to a place of its own in the
    yard; both modes under the piece sizes and the looping grid."""
    cases = []
    for name in ENGINE_CASES:
        b = _engine_built(name)
        for mode in (0, 1):
            for sw in (ENGINE_ROWS if b.max_len == 512 else ENGINE_ROWS[:1]):
                c = Case(f"update_engine[{name} {'delta' if mode else 'reference'} {_tag(sw)}]", 32 << 20)
                c.kind, c.switches, c.seed, c.mode, c.built = "engine", dict(sw), 90, mode, name
                c.region_at = {int(r): c.yard.place(f"allocation{k}", b.max_len, residue=int(r) % 16)
                               for k, r in enumerate(b.regions)}
                c.pay_at = {}
                pays = []
                for i in np.flatnonzero(b.has_payload):
                    p, n = int(b.rec["payload"][i]), int(b.rec["length"][i])
                    c.pay_at[int(i)] = c.yard.place(f"payload{i}", n, residue=p % 16)
                    pays.append((c.pay_at[int(i)], n, b.expect[i][0] == 0))
                c.junk_at = c.yard.place("ignored address fields", 64)
                c.d_ios = _desc(c, "ios", 56 * b.n)
                c.d_jobs = _desc(c, "jobs", 104 * b.n)
                c.d_info = _desc(c, "info", 32)
                c.legal, c.required = engine_ranges(c.region_at.values(), b.max_len, pays,
                                                    [(c.d_ios, 56 * b.n), (c.d_jobs, 104 * b.n)])
                c.yard.check()
                cases.append(c)
    return cases


def _frames_inp(layout, cus, seed):
    """The frame records and bytes of a tests/batch_cases.py frames case, or "granules": frames
    packed as the framing walk leaves them whose boundaries fall on every offset of a granule."""
    import batch_cases as bc
    rng = np.random.default_rng(seed)
    if layout != "granules":
        return bc.FramesCase("frames_" + layout, layout).build(cus, rng)
    sizes = list(range(1, 41)) + [64 + i for i in range(48)] + [1024 + 9 * i for i in range(16)] + [0, 0, 4097]
    f = np.zeros(len(sizes), dtype=bc.FRAME_DT)
    pos = 0
    for i, sz in enumerate(sizes):
        pos += 8
        f["offset"][i], f["size"][i] = pos, sz
        pos += sz
    inp = dict(arena=bc._bytes(rng, pos), frames=f, max_size=8192, cus=cus)
    bc._frames_restore(inp, rng)
    return inp


def family_frames(cus=256):
    """frame_verify_batch: the cases frames_walked, frames_gaps and frames_big under the frame
    switch rows, and frames whose boundaries fall on every granule offset, the last of which ends
    on the buffer's last byte, directly before a gap."""
    cases = []
    rows = ({}, {"frame_stream": "0", "frame_segw": "1"}, {"frame_stream": "0", "frame_segw": "64"},
            {"frame_stream": "1", "frame_segw": "1"}, {"frame_stream": "1", "frame_segw": "64"}, {"record_direct": "0"})
    for k, layout in enumerate(("walked", "gaps", "big", "granules")):
        inp = _frames_inp(layout, cus, 70 + k)
        f = inp["frames"]
        for r in (0, 11):
            for sw in rows:
                tag = ",".join(f"{a}={b}" for a, b in sw.items()) or "default"
                c = Case(f"frame_verify_batch[{layout} r{r} {tag}]", 8 << 20)
                c.kind, c.switches, c.seed, c.layout, c.layout_seed = "frames", dict(sw), 70 + k, layout, 70 + k
                c.n, c.max_size = f.size, inp["max_size"]
                c.at = c.yard.place("frames buffer", inp["arena"].size, residue=r)
                c.d_frames = _desc(c, "frame records", f.nbytes)
                c.d_count = _desc(c, "count", 4)
                ok = f["size"] <= inp["max_size"]
                data = [(c.at + int(o), int(n)) for o, n in zip(f["offset"][ok], f["size"][ok]) if n]
                c.legal, c.required = frame_ranges(c.at, f["offset"], f["size"], inp["max_size"], [(c.d_frames, f.nbytes)])
                assert c.required == data
                c.yard.check()
                cases.append(c)
    return cases


FAMILIES = {
    "records": family_records,
    "frames": family_frames,
    "list_grid": family_list_grid,
    "list_schedules": family_list_schedules,
    "strided_blocks": family_strided_blocks,
    "md5": family_md5,
    "update": family_update,
    "update_cow": family_update_cow,
    "update_ordered": family_update_ordered,
    "update_versioned": family_update_versioned,
    "update_engine": family_update_engine,
}


# ---- the child: run one family against the check library ------------------------------------------------
def _image(case):
    rng = np.random.default_rng(1000 + case.seed)
    return rng.integers(1, 256, case.yard.size, dtype=np.uint8)


def _put(img, off, arr):
    b = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    img[off:off + b.size] = b


def _get(img, off, dtype, n):
    return img[off:off + np.dtype(dtype).itemsize * n].view(dtype).copy()


def _run_list(case, L, base, img, run):
    import batch_cases as bc
    n = case.lens.size
    ctype = case.ctype
    rng = np.random.default_rng(case.seed)
    arena = case.kind == "blocks"
    abase = int(case.offs.min()) & ~4095 if arena and n else 0
    _put(img, case.d_addrs, (case.offs - np.uint64(abase)) if arena else case.offs + np.uint64(base))
    _put(img, case.d_lens, case.lens.astype(np.uint32) if arena else case.lens)
    if case.verify:
        truth = bc.crc_ranges(ctype, img, case.offs, case.lens)
        flip = np.zeros(n, dtype=np.uint32)
        flip[rng.choice(n, min(5, n), replace=False)] = 0x100
        _put(img, case.d_expected, truth ^ flip)
        _put(img, case.d_mismatch, np.full(n, 0xA5, dtype=np.uint8))
        _put(img, case.d_count, np.full(1, 0xA5A5A5A5, dtype=np.uint32))
    else:
        starts = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        _put(img, case.d_starts, starts)
        truth = bc.crc_ranges(ctype, img, case.offs, case.lens, starts)

    def call(stream):
        if arena:
            L.verify_blocks(ctype, base + abase, base + case.d_addrs, base + case.d_lens, base + case.d_expected,
                            base + case.d_mismatch, base + case.d_count, n, case.max_len, computed=base + case.d_computed,
                            stream=stream)
        elif case.verify:
            L.verify_batch(ctype, base + case.d_addrs, base + case.d_lens, base + case.d_expected, base + case.d_mismatch,
                           base + case.d_count, n, case.max_len, computed=base + case.d_computed, stream=stream)
        else:
            L.create_batch(ctype, base + case.d_addrs, base + case.d_lens, base + case.d_out, n, case.max_len,
                           starts=base + case.d_starts, stream=stream)
    got = run(call)
    if case.verify:
        ok = (np.array_equal(_get(got, case.d_computed, np.uint32, n), truth)
              and np.array_equal(_get(got, case.d_mismatch, np.uint8, n), (flip != 0).astype(np.uint8))
              and int(_get(got, case.d_count, np.uint32, 1)[0]) == int(np.count_nonzero(flip)))
    else:
        ok = np.array_equal(_get(got, case.d_out, np.uint32, n), truth)
    return "ok" if ok else "values differ from the oracle's"


def _run_strided(case, L, base, img, run):
    import batch_cases as bc
    n = case.n
    offs = np.array([case.base + i * case.stride for i in range(n)], dtype=np.uint64)
    lens = np.full(n, case.length, dtype=np.uint64)
    start = 0x1234ABCD
    if case.verify:
        truth = bc.crc_ranges(CRC32C, img, offs, lens)
        flip = np.zeros(n, dtype=np.uint32)
        flip[n // 2] = 0x8000
        _put(img, case.d_expected, truth ^ flip)

        def call(stream):
            L.verify_strided(CRC32C, base + case.base, case.stride, case.length, n, base + case.d_expected,
                             base + case.d_mismatch, base + case.d_count, computed=base + case.d_out, stream=stream)
    else:
        truth = bc.crc_ranges(CRC32C, img, offs, lens, np.full(n, start, dtype=np.uint32))

        def call(stream):
            L.create_strided(CRC32C, base + case.base, case.stride, case.length, n, base + case.d_out, start=start,
                             stream=stream)
    got = run(call)
    ok = np.array_equal(_get(got, case.d_out, np.uint32, n), truth)
    if case.verify:
        ok = ok and int(_get(got, case.d_count, np.uint32, 1)[0]) == 1
    return "ok" if ok else "values differ from the oracle's"


def _run_md5(case, L, base, img, run):
    segs = np.zeros(max(len(case.segs), 1), dtype=np.dtype([("data", "<u8"), ("length", "<u8")]))
    for k, (o, n) in enumerate(case.segs):
        segs[k] = (0 if o is None else base + o, n)
    off = np.zeros(len(case.files) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(f) for f in case.files])
    _put(img, case.d_segs, segs[:len(case.segs)])
    _put(img, case.d_off, off)
    raw = img.tobytes()
    want = [hashlib.md5(b"".join(bytes(n) if o is None else raw[o:o + n] for o, n in f)).digest() for f in case.files]

    def call(stream):
        L.md5_batch(base + case.d_segs, base + case.d_off, len(case.files), len(case.segs), out=base + case.d_out,
                    stream=stream)
    got = run(call)
    digests = got[case.d_out:case.d_out + 16 * len(case.files)].tobytes()
    return "ok" if digests == b"".join(want) else "digests differ from hashlib's"


def _run_update(case, L, base, img, run):
    import importlib
    import oracle
    import update_footprint as uf
    hf = importlib.import_module("3fs_amd")
    n = len(case.ios)
    arr = (hf.UpdateIO * n)()
    T = case.ctype
    state = {}     # chunk address -> [model bytes, size, (type, value)]: what the IOs applied so far left
    model = []     # per IO: (status, size, checksum) and the chunk image right after it, or None (not applied)
    for i, io in enumerate(case.ios):
        u = arr[i]
        at = io["chunk_at"]
        if at not in state:
            size = io["size"]
            chunk = bytearray(img[at:at + case.max_len].tobytes())
            state[at] = [chunk, size, tuple(oracle.create(T, bytes(chunk[:size]))) if size else (oracle.NONE, 0)]
            u.chunk_size, (u.chunk_checksum_type, u.chunk_checksum) = size, state[at][2]
        chunk, size, ck = state[at]
        assert size == io["size"], (i, size, io)     # the builder followed the same sizes
        u.chunk = base + at
        if io["kind"] == "W":
            pay = img[io["pay_at"]:io["pay_at"] + io["len"]].tobytes()
            wck = (T, oracle.create(T, pay)[1] ^ (0x40 if io.get("bad") else 0))
            u.payload, u.offset, u.length, u.update_type = base + io["pay_at"], io["off"], io["len"], hf.UPDATE_WRITE
            u.write_checksum_type, u.write_checksum = wck
            args = (oracle.WRITE, io["off"], io["len"], pay, wck)
        else:
            u.payload, u.offset, u.length = 0, 0, io["len"]
            u.update_type = hf.UPDATE_TRUNCATE if io["kind"] == "T" else hf.UPDATE_EXTEND
            args = (oracle.TRUNCATE if io["kind"] == "T" else oracle.EXTEND, 0, io["len"])
        if not io["applied"]:
            model.append(None)
            continue
        status, new_size, new_ck = oracle.replica_apply(chunk, size, ck, *args, chunk_size=case.max_len)
        if status == hf.OK:
            state[at][1], state[at][2] = new_size, tuple(new_ck)
        model.append(((status, new_size, tuple(new_ck)), bytes(chunk[:new_size])))
    _put(img, case.d_ios, np.frombuffer(bytes(arr), dtype=np.uint8))
    if case.entry == "update_cow":
        _put(img, case.d_dst, np.array([0 if io.get("dst") == "none" else base + (io["dst_at"] or io["chunk_at"])
                                        for io in case.ios], dtype=np.uint64))
    if case.entry == "update_versioned":      # every job admitted (tests/versioned_cases.py admit_all)
        ver = np.zeros(n, dtype=L.update_ver_dtype())
        for i, io in enumerate(case.ios):
            k = io["round"]
            ver["io_ver"][i], ver["job_chain_ver"][i] = 7 + k + 1, 3
            if k == 0:
                ver["chain_ver"][i], ver["update_ver"][i], ver["commit_ver"][i] = 3, 7, 5
                ver["meta_chunk_size"][i], ver["chunk_state"][i] = case.max_len, L.CHUNK_STATE_CLEAN
        _put(img, case.d_ver, ver)
    saved = {}

    def opts(name, value):
        saved.setdefault(name, L.get_option(name))
        L.set_option(name, value)
    uf.set_pipeline(opts, case.pipeline)
    opts("apply_nt", case.nt)
    try:
        def call(stream):
            if case.entry == "update_cow":
                L.update_cow(T, base + case.d_ios, base + case.d_dst, n, case.max_len, mode=case.mode, stream=stream)
            elif case.entry == "update_versioned":
                L.update_versioned(T, base + case.d_ios, base + case.d_ver, n, case.max_len, case.max_rounds,
                                   mode=case.mode, info=base + case.d_info, stream=stream)
            elif case.entry == "update_ordered":
                L.update_ordered(T, base + case.d_ios, n, case.max_len, case.max_rounds, mode=case.mode,
                                 info=base + case.d_info, stream=stream)
            else:
                L.update_batch(T, base + case.d_ios, n, case.max_len, mode=case.mode, stream=stream)
        got = run(call)
    finally:
        for k, v in saved.items():
            L.set_option(k, v)
    res = (hf.UpdateIO * n).from_buffer_copy(got[case.d_ios:case.d_ios + 56 * n].tobytes())
    for i, io in enumerate(case.ios):
        r = res[i]
        if model[i] is None:
            if r.status != hf._lib.NOT_APPLIED:
                return f"io {i} ({io}): status {r.status}, want NOT_APPLIED"
            continue
        (status, size, ck), image = model[i]
        if r.status != status:
            return f"io {i} ({io}): status {r.status}, the oracle's {status}"
        if status == hf.OK and (r.out_size != size or (size and r.out_checksum != ck[1])):
            return f"io {i} ({io}): out_size {r.out_size} checksum {r.out_checksum:#x}, the oracle's {size} {ck}"
        if io["dst_at"]:      # out of place: the new image at the destination, the chunk as it was
            at = io["chunk_at"]
            if got[at:at + case.max_len].tobytes() != img[at:at + case.max_len].tobytes():
                return f"io {i} ({io}): the chunk of an out-of-place IO was written"
            if status == hf.OK and got[io["dst_at"]:io["dst_at"] + size].tobytes() != image:
                return f"io {i} ({io}): destination bytes differ from the oracle's"
    for at, (chunk, size, _) in state.items():   # in place: what the chunk's last applied IO left
        if not any(io["dst_at"] for io in case.ios if io["chunk_at"] == at) and got[at:at + size].tobytes() != bytes(chunk[:size]):
            return f"chunk at yard +{at:#x}: bytes differ from the oracle's"
    if case.entry == "update_versioned":
        v = got[case.d_ver:case.d_ver + 48 * n].view(L.update_ver_dtype())
        for i, io in enumerate(case.ios):
            if model[i] is not None and (int(v["out_update_ver"][i]), int(v["out_chunk_state"][i])) != (8 + io["round"], 2):
                return f"job {i}: version record {v[i]} after an admitted job"
    if case.entry in ("update_ordered", "update_versioned"):
        info = _get(got, case.d_info, np.uint32, 2)
        if int(info[1]) != sum(1 for m in model if m is None):
            return f"info {info}: the NOT_APPLIED count differs"
    return "ok"


def _run_engine(case, L, base, img, run):
    import engine_cases as ec
    b = _engine_built(case.built)
    for r, at in case.region_at.items():
        img[at:at + b.max_len] = b.arena0[r:r + b.max_len]

    def move(x):
        """A builder's arena offset as a device address: an allocation's, or (the junk that later
        jobs of a chunk carry in fields the call ignores and overwrites) a spare place in the yard."""
        x = int(x)
        return 0 if not x else base + (case.region_at[x] if x in case.region_at else case.junk_at)
    rec, jr = b.rec.copy(), b.jr.copy()
    rec["chunk"] = [move(x) for x in b.rec["chunk"]]
    for i, at in case.pay_at.items():
        p, n = int(b.rec["payload"][i]), int(b.rec["length"][i])
        img[at:at + n] = b.pay[p:p + n]
        rec["payload"][i] = base + at
    for f in ("dst", "addr", "w_addr"):
        jr[f] = [move(x) for x in b.jr[f]]
    _put(img, case.d_ios, rec)
    _put(img, case.d_jobs, jr)

    def call(stream):
        L.update_engine(b.ctype, base + case.d_ios, base + case.d_jobs, b.n, b.max_len, b.max_rounds, mode=case.mode,
                        info=base + case.d_info, stream=stream)
    got = run(call)
    want_rec, want_jr = ec.expected(b.rec, b.jr, b.expect, 0)   # in the builder's offsets
    want_rec["chunk"], want_rec["payload"] = rec["chunk"], rec["payload"]
    for f in ec.ADDR_FIELDS:
        src = want_jr[f]
        want_jr[f] = [jr[f][i] if f == "dst" else move(x) for i, x in enumerate(src)]
    got_rec = got[case.d_ios:case.d_ios + rec.nbytes].view(rec.dtype)
    got_jr = got[case.d_jobs:case.d_jobs + jr.nbytes].view(jr.dtype)
    for name, have, want in (("ios", got_rec, want_rec), ("jobs", got_jr, want_jr)):
        for f in want.dtype.names:
            if f.startswith("reserved"):
                continue
            bad = np.flatnonzero(np.asarray(have[f] != want[f]).reshape(have.size, -1).any(axis=1))
            if bad.size:
                i = int(bad[0])
                return f"{name}[{i}].{f}: {have[f][i]}, the model's {want[f][i]} (job {b.jobs[i]['k']})"
    for r, at in case.region_at.items():
        if got[at:at + b.max_len].tobytes() != b.arena1[r:r + b.max_len].tobytes():
            return f"allocation at yard +{at:#x}: bytes differ from the model's"
    info = tuple(int(x) for x in _get(got, case.d_info, np.uint32, 8))
    return "ok" if info == tuple(b.info) else f"info {info}, the model's {tuple(b.info)}"


def _run_records(case, L, base, img, run):
    import batch_cases as bc
    import oracle
    r = case.recs.copy()
    n = r.size
    offs, lens = np.array(case.offs, dtype=np.uint64), np.array(case.lens, dtype=np.uint64)
    truth = bc.crc_ranges(CRC32C, img, offs, lens)
    stale = np.where(np.arange(n) % 7 == 3, np.uint32(0x80), np.uint32(0))
    r["data"] = offs + np.uint64(base)
    want = []
    if case.kind == "scrub":
        r["checksum"] = np.where(r["fin"] == 1, ~truth, truth) ^ stale
        r["computed"], r["status"] = 0xA5A5A5A5, 0x5E5E5E5E
        for i in range(n):
            t, fin, o, ln = int(r["checksum_type"][i]), int(r["fin"][i]), int(offs[i]), int(lens[i])
            want.append((3, 0) if t not in (0, CRC32C) or fin > 1 else oracle.scrub(t, fin, img[o:o + ln], int(r["checksum"][i])))
    else:
        r["chunk_checksum"] = truth ^ stale
        r["out_checksum"], r["out_checksum_type"], r["status"] = 0xA5A5A5A5, 0xA5, 0x5E5E5E5E
        for i in range(n):
            u, o, ln = r[i], int(offs[i]), int(lens[i])
            full = int(u["offset"]) == 0 and ln == int(u["chunk_len"])
            rc, (t, v) = oracle.read_result(int(u["batch_checksum_type"]), (int(u["chunk_checksum_type"]), int(u["chunk_checksum"])),
                                            int(u["offset"]), img[o:o + ln], int(u["chunk_len"]),
                                            full_chunk=img[o:o + ln] if full else None, recalculate=bool(u["recalculate"]))
            want.append((rc, t, v))
    _put(img, case.d_recs, r)

    def call(stream):
        if case.kind == "scrub":
            L.scrub_batch(CRC32C, base + case.d_recs, n, case.max_len, base + case.d_count, stream=stream)
        else:
            L.read_result_batch(CRC32C, base + case.d_recs, n, case.max_len, stream=stream)
    got = run(call)
    g = got[case.d_recs:case.d_recs + r.nbytes].view(r.dtype)
    for i in range(n):
        if case.kind == "scrub":
            have = (int(g["status"][i]), int(g["computed"][i]))
        else:
            have = (int(g["status"][i]), int(g["out_checksum_type"][i]), int(g["out_checksum"][i]))
        if have != tuple(int(x) for x in want[i]):
            return f"record {i} ({r[i]}): {have}, the oracle's {want[i]}"
    if case.kind == "scrub" and int(_get(got, case.d_count, np.uint32, 1)[0]) != sum(1 for w in want if w[0]):
        return "the mismatch count differs from the oracle's"
    return "ok"


def _run_frames(case, L, base, img, run):
    import batch_cases as bc
    inp = _frames_inp(case.layout, 256, case.layout_seed)
    fc = bc.FramesCase("frames", case.layout)
    img[case.at:case.at + inp["arena"].size] = inp["arena"]
    _put(img, case.d_frames, fc.buffers(inp, 0)["frames"])
    ref = fc.reference(inp)

    def call(stream):
        L.frame_verify_batch(base + case.at, base + case.d_frames, case.n, case.max_size, base + case.d_count, stream=stream)
    got = run(call)
    f = got[case.d_frames:case.d_frames + inp["frames"].nbytes].view(bc.FRAME_DT)
    ok = (np.array_equal(f["status"], ref["status"]) and np.array_equal(f["computed"], ref["computed"])
          and int(_get(got, case.d_count, np.uint32, 1)[0]) == int(ref["count"][0]))
    return "ok" if ok else "statuses / values differ from the oracle's"


RUNNERS = {"frames": _run_frames, "engine": _run_engine, "scrub": _run_records, "read": _run_records, "list": _run_list, "blocks": _run_list, "strided": _run_strided, "md5": _run_md5, "update": _run_update}


def run_family(family, out_path):
    import ctypes
    import importlib
    import torch
    here = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(here)
    for p in (repo, os.path.join(repo, "oracle"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    hf = importlib.import_module("3fs_amd")
    L = hf._lib
    lib = L.load()
    arm, disarm, units = lib.hf3fs_crc_loadcheck_arm, lib.hf3fs_crc_loadcheck_disarm, lib.hf3fs_crc_loadcheck_units
    arm.restype = disarm.restype = units.restype = ctypes.c_int
    arm.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    b = importlib.import_module("3fs_amd.build")
    assert units() == len(b.CHECK_SOURCES) + len(b.CHECK_ONLY), units()   # no unit's copy of the state was lost
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    cases = FAMILIES[family]()
    ymax = max(c.yard.size for c in cases)
    yard = torch.zeros(ymax, dtype=torch.uint8, device=dev)
    bitmap = torch.zeros(ymax // G // 32 + 1, dtype=torch.int32, device=dev)
    site_map = torch.zeros(ymax // G, dtype=torch.uint8, device=dev)
    log_words = 36 + 6 * 64
    log = torch.zeros(log_words, dtype=torch.int32, device=dev)
    base = yard.data_ptr()
    assert base % PAGE == 0
    reports = {}
    defaults = {}
    for case in cases:
        img = _image(case)
        for name, value in case.switches.items():
            defaults.setdefault(name, L.get_option(name))
            L.set_option(name, value)

        def run(call, case=case, img=img):
            yard[:case.yard.size].copy_(torch.from_numpy(img))
            bitmap.zero_(), site_map.zero_(), log.zero_()
            torch.cuda.synchronize()
            rc = arm(base, case.yard.size, bitmap.data_ptr(), site_map.data_ptr(), log.data_ptr())
            assert rc == 0, rc
            try:
                call(stream)
                torch.cuda.synchronize()
            finally:
                assert disarm() == 0
            return yard[:case.yard.size].cpu().numpy()

        outputs = RUNNERS[case.kind](case, L, base, img, run)
        for name in case.switches:
            L.set_option(name, defaults[name])
        bits = np.unpackbits(bitmap.cpu().numpy().view(np.uint8), bitorder="little")[:case.n_granules].astype(bool)
        sm = site_map.cpu().numpy()[:case.n_granules]
        lg = log.cpu().numpy().view(np.uint32)
        entries = []
        for k in range(min(int(lg[34]), 64)):
            e = lg[36 + 6 * k:36 + 6 * k + 6]
            entries.append(dict(address=int(e[0]) | int(e[1]) << 32, bytes=int(e[2]), site=int(e[3]), block=int(e[4]),
                                thread=int(e[5]), yard_offset=(int(e[0]) | int(e[1]) << 32) - base))
        assert case.name not in reports, case.name
        reports[case.name] = dict(read=runs_of(bits, sm), counters={str(k): int(lg[k]) for k in range(1, 18) if lg[k]},
                                  outside=int(lg[32]), desc=int(lg[33]), log=entries, outputs=outputs)
    with open(out_path, "w") as f:
        json.dump(dict(family=family, reports=reports), f)
    print(f"load_footprint: family {family}: {len(reports)} calls reported")


if __name__ == "__main__":
    run_family(sys.argv[1], sys.argv[2])
