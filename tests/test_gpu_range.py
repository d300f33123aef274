"""hf3fs_crc_range_query and hf3fs_crc_file_length on the GPU.

Every expectation comes from tests/range_cases.py: queryChunks, processQueryResults and the two
processors restated in Python with the paged loop (page size 1000, the reference's default), and
queryChunksByChain / queryChunks over an ordered map; the two largest tables use the header's closed
form, which tests/test_range_model.py holds to the paged loop.  After every call the whole op or file
array (every field: inputs unchanged, outputs the model's), the eight info words, the list and the
guard bytes around every array are compared, exactly; the table must be unchanged.

Shapes: tables of 0, 1, 255, 256, 257 records (one lane per record, 256 per workgroup and per tile of
a share) and 70,001 (274 shares of one tile each, a partial last one; ops over 274 shares too), and
2^20 + 300 records (2048 shares of three tiles, the last share partial)."""
import threading

import numpy as np
import pytest

import range_cases as rc

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
GUARD = 64
CANARY = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded(dev, nbytes):
    t = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
    return t, t[GUARD:GUARD + nbytes]


class Images:
    """Device images of named arrays, each between guards."""

    def __init__(self, dev, **sizes):
        self.raw, self.t = {}, {}
        for name, nbytes in sizes.items():
            self.raw[name], self.t[name] = _guarded(dev, max(nbytes, 8))

    def put(self, name, arr):
        if arr.size:
            self.t[name][:arr.nbytes].copy_(torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()))

    def fill(self, *names):
        for name in names:
            self.t[name].fill_(CANARY)

    def host(self, name, dtype, count):
        return self.t[name].cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype)

    def guards(self, what):
        for name, raw in self.raw.items():
            g = raw.cpu().numpy()
            assert (g[:GUARD] == CANARY).all() and (g[-GUARD:] == CANARY).all(), f"{what}: bytes around {name} written"


def _same(got, want, names, what):
    if got.tobytes() == want.tobytes():
        return
    for f in names:
        bad = np.flatnonzero((got[f] != want[f]).reshape(got.size, -1).any(axis=1))
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {bad.size} records differ in {f}; record {i}: got {got[f][i]}, want {want[f][i]}"
                                 f"\n got {got[i]}\nwant {want[i]}")
    raise AssertionError(f"{what}: records differ in padding")


class Query:
    def __init__(self, dev, meta, ops, list_cap):
        self.n_meta, self.n_ops, self.list_cap = meta.size, ops.size, list_cap
        self.im = Images(dev, meta=meta.nbytes, ops=ops.nbytes, info=4 * rc.INFO_WORDS, list=4 * list_cap)
        self.put(meta, ops)

    def put(self, meta, ops):
        self.im.put("meta", meta)
        self.im.put("ops", ops)
        self.im.fill("info", "list")
        torch.cuda.synchronize()

    def call(self, hf, stream=None):
        t = self.im.t
        hf.range_query(t["meta"] if self.n_meta else None, self.n_meta, t["ops"] if self.n_ops else None, self.n_ops,
                       t["info"], t["list"] if self.list_cap else None, self.list_cap,
                       stream=stream or torch.cuda.current_stream())

    def check(self, meta, want_ops, want_info, want_list, what):
        _same(self.im.host("ops", rc.OP, self.n_ops), want_ops, rc.OP.names, what)
        assert self.im.host("info", np.uint32, rc.INFO_WORDS).tolist() == list(want_info), what
        assert self.im.host("meta", rc.META, self.n_meta).tobytes() == meta.tobytes(), f"{what}: the table changed"
        got = self.im.t["list"].cpu().numpy()
        assert want_list.size <= self.list_cap
        assert np.array_equal(got[:4 * want_list.size].view(np.uint32), want_list), f"{what}: the list"
        assert (got[4 * want_list.size:] == CANARY).all(), f"{what}: a list entry past the count was written"
        self.im.guards(what)


def run_query(hf, dev, meta, ops, list_cap, what, model=rc.range_query, stream=None):
    q = Query(dev, meta, ops, list_cap)
    q.call(hf, stream)
    torch.cuda.synchronize()
    want = ops.copy()
    info, lst = model(meta, want, list_cap)
    q.check(meta, want, info, lst, what)
    return want, info, lst


# ---- range_query ----
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 70001])
def test_random_ops_against_the_paged_loop(hf, dev, n):
    rng = np.random.default_rng(0x7A61E + n)
    meta = rc.random_table(rng, n, hi_values=(3, 4, 9), max_len=1 << 32)
    ops = rc.random_ops(rng, meta, 300 if n < 1000 else 3000)
    want, info, lst = run_query(hf, dev, meta, ops, 1 << 17, f"{n} records")
    assert info[0] > ops.size // 2 and info[1] > 0 and info[6] == 0 and info[7] == 0
    assert {4032, 3, 7007, -1} & set(want["status"].tolist()) and (want["status_in"] != 0).any()
    if n >= 255:
        assert want["more"].any() and info[4] > 100 and (want["kind"] == rc.QUERY).any()
        assert (want["total_len"] >> 32).any(), "no total_len crossed 2^32"


def test_two_20_plus_300_records_in_closed_form(hf, dev):
    n = (1 << 20) + 300
    rng = np.random.default_rng(0x2020)
    ids = [rc.ident(5, 7 * i + 3) for i in range(n)]
    meta = rc.new_meta(ids, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
                       np.where(rng.random(n) < 0.1, rng.integers(1, 3, n), 0))
    ops = rc.new_ops(1501)
    for k in range(1500):
        a = int(rng.integers(0, n))
        b = min(n - 1, a + int(rng.integers(0, 3000)))
        rc.set_range(ops[k], ids[a] - int(rng.integers(0, 2)), ids[b] + int(rng.integers(0, 2)))
        ops[k]["kind"] = rc.REMOVE if k % 3 == 0 else rc.QUERY
        ops[k]["max_chunks"] = rng.choice([0, 1, 100, 5000])
    rc.set_range(ops[1500], 0, rc.ident(6, 0))  # the whole table: the prefixes' last entries
    want, info, lst = run_query(hf, dev, meta, ops, 1 << 20, "2^20 + 300 records", model=rc.closed_form)
    assert want[1500]["total_chunks"] == int((meta["recycle_state"] == 0).sum()) and want[1500]["last_index"] >= n - 40
    assert want[1500]["total_len"] >> 50 and info[6] == 0 and info[4] > 100000


def edge_table():
    """Twelve records: id_lo of 0 and of 2^64 - 1, ids that differ only in id_hi, neighbours and gaps."""
    ids = [rc.ident(3, rc.M64 - 1), rc.ident(3, rc.M64), rc.ident(4, 0), rc.ident(4, 1), rc.ident(4, 5), rc.ident(5, 5),
           rc.ident(6, 5), rc.ident(6, 9), rc.ident(6, 10), rc.ident(8, 0), rc.ident(8, rc.M64), rc.ident(9, 7)]
    return rc.new_meta(ids, [1 << k for k in range(12)], [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 0]), ids


def test_every_begin_end_pair_of_a_12_record_table(hf, dev):
    meta, ids = edge_table()
    points = sorted({p for i in ids for p in (i - 1, i, i + 1)} | {0, (1 << 128) - 1, rc.ident(7, 0)})
    ops = rc.new_ops(len(points) ** 2)
    k = 0
    for b in points:
        for e in points:  # begin < end, begin == end and begin > end
            rc.set_range(ops[k], b, e)
            ops[k]["kind"] = rc.REMOVE if k % 2 else rc.QUERY
            k += 1
    want, info, lst = run_query(hf, dev, meta, ops, 1 << 16, "range edges")
    assert len(points) >= 30 and info[1] == 0 and info[4] == lst.size > 0 and (want["total_chunks"] > 1).sum() > 100
    # end equal to a record's id excludes it, begin equal to one includes it
    at = {(int(o["begin_hi"]) << 64 | int(o["begin_lo"]), int(o["end_hi"]) << 64 | int(o["end_lo"])): o for o in want}
    assert at[(ids[3], ids[4])]["total_chunks"] == 1 and at[(ids[3], ids[4])]["last_index"] == 3
    assert at[(ids[3] + 1, ids[4] + 1)]["last_index"] == 4
    assert at[(ids[2], ids[3])]["total_chunks"] == 0  # one record, being removed: no normal record in the span


def test_limits_around_the_span(hf, dev):
    rng = np.random.default_rng(0x11317)
    meta = rc.random_table(rng, 300, max_len=1 << 32)
    meta["recycle_state"][100:110] = 1  # a span with no normal record
    ids = rc.table_ids(meta)
    spans = [(0, 299), (5, 6), (100, 109), (90, 120), (17, 256), (255, 257)]
    ops = rc.new_ops(6 * len(spans) * 2)
    k = 0
    for a, b in spans:
        normals = int((meta["recycle_state"][a:b + 1] == 0).sum())
        for limit in (0, 1, max(normals - 1, 0), normals, normals + 1, 0xFFFFFFFF):
            for kind in (rc.QUERY, rc.REMOVE):
                rc.set_range(ops[k], ids[a], ids[b] + 1)
                ops[k]["max_chunks"], ops[k]["kind"] = limit, kind
                k += 1
    want, info, lst = run_query(hf, dev, meta, ops, 1 << 14, "limits")
    assert (want["total_chunks"][24:36] == 0).all() and not want["more"][24:36].any()
    assert want["more"].sum() >= 2 * 2 * 4 and info[1] == 0


def test_length_prefix_crosses_2_32_at_a_share_boundary(hf, dev):
    n = 70001  # shares of 256 records: the first share's lengths sum to 2^32 exactly
    rng = np.random.default_rng(0x3232)
    meta = rc.random_table(rng, n, max_len=1 << 32, recycle_p=0.0)
    meta["length"][:256] = 1 << 24
    meta["length"][256:512] = 0xFFFFFFFF
    ids = rc.table_ids(meta)
    spans = [(0, 256), (0, 255), (0, 257), (1, 257), (255, 257), (256, 512), (0, 70001), (200, 60000)]
    ops = rc.new_ops(len(spans))
    for o, (a, b) in zip(ops, spans):
        rc.set_range(o, ids[a], ids[b - 1] + 1)
    want, info, lst = run_query(hf, dev, meta, ops, 0, "lengths")
    assert want["total_len"][:3].tolist() == [1 << 32, (1 << 32) - (1 << 24), (1 << 32) + 0xFFFFFFFF]
    assert want["total_len"][5] == 256 * 0xFFFFFFFF


def test_unsorted_table(hf, dev):
    n = 70001
    rng = np.random.default_rng(0x0507)
    meta = rc.random_table(rng, n)
    ops = rc.random_ops(rng, meta, 500)
    meta[[255, 256]] = meta[[256, 255]]  # one inversion across a share boundary
    meta["id_hi"][1000], meta["id_lo"][1000] = meta["id_hi"][999], meta["id_lo"][999]  # one duplicate id
    want, info, lst = run_query(hf, dev, meta, ops, 4096, "unsorted")
    assert info == [0, 500, 0, 0, 0, 0, 0, 2] and (want["status"] == 3).all() and lst.size == 0
    assert (want["last_index"] == rc.NONE).all() and not want["list_first"].any()
    # the same table in order, through the same pair buffer
    order = np.argsort(np.array(rc.table_ids(meta), dtype=object), kind="stable")
    meta = meta[order].copy()
    meta["id_lo"][1000] += 1
    want, info, lst = run_query(hf, dev, meta, ops, 4096, "sorted again")
    assert info[7] == 0 and info[0] > 400


@pytest.mark.parametrize("cap", ["none", "total - 1", "total"])
def test_remove_lists_under_list_cap(hf, dev, cap):
    rng = np.random.default_rng(0xCA9)
    meta = rc.random_table(rng, 1000)
    ops = rc.random_ops(rng, meta, 400, max_span=60)
    ids = rc.table_ids(meta)
    for k in (10, 11, 12):  # overlapping ranges, listed in full each time
        rc.set_range(ops[k], ids[100], ids[300 + k])
        ops[k]["kind"], ops[k]["max_chunks"], ops[k]["status_in"] = rc.REMOVE, 0, 0
    probe = ops.copy()
    total = rc.range_query(meta, probe, 1 << 20)[0][4]
    list_cap = {"none": 0, "total - 1": total - 1, "total": total}[cap]
    want, info, lst = run_query(hf, dev, meta, ops, list_cap, f"list_cap {list_cap}")
    assert info[4] == total > 1500 and info[6] == (list_cap < total) and lst.size == min(total, list_cap)
    first = want["list_first"].astype(np.int64)
    counts = np.where((want["kind"] == rc.REMOVE) & (want["status"] == 0), want["total_chunks"], 0)
    assert np.array_equal(first, np.cumsum(counts) - counts)  # a QUERY op carries the running offset


def test_one_op_listing_70000_beside_70000_ops_listing_none_or_one(hf, dev):
    n = 70001
    rng = np.random.default_rng(0x70000)
    meta = rc.random_table(rng, n, recycle_p=0.0)
    ids = rc.table_ids(meta)
    ops = rc.new_ops(70001)
    rc.set_range(ops[0], 0, ids[-1] + 1)
    ops[0]["kind"], ops[0]["max_chunks"] = rc.REMOVE, 70000
    at = rng.integers(0, n, 70000)
    for side in ("begin", "end"):  # [id, id + 1): one record each
        ops[side + "_hi"][1:] = meta["id_hi"][at]
        ops[side + "_lo"][1:] = meta["id_lo"][at] + np.uint64(side == "end")
    ops["kind"][1:] = np.where(np.arange(70000) % 2, rc.REMOVE, rc.QUERY)
    want, info, lst = run_query(hf, dev, meta, ops, 105000, "one long segment", model=rc.closed_form)
    assert want[0]["more"] == 1 and want[0]["total_chunks"] == 70000 and info[4] == 105000 and info[6] == 0
    assert np.array_equal(lst[:70000], np.arange(70000, 0, -1, dtype=np.uint32))
    assert np.array_equal(lst[70000:], at[1::2].astype(np.uint32))


# ---- file_length ----
class Fold:
    def __init__(self, dev, ops, files):
        self.n_ops, self.n_files = ops.size, files.size
        self.im = Images(dev, ops=ops.nbytes, files=files.nbytes, info=4 * rc.INFO_WORDS)
        self.im.put("ops", ops)
        self.im.put("files", files)
        torch.cuda.synchronize()

    def call(self, hf, stream=None):
        t = self.im.t
        hf.file_length(t["ops"] if self.n_ops else None, self.n_ops, t["files"] if self.n_files else None,
                       self.n_files, t["info"], stream=stream or torch.cuda.current_stream())

    def check(self, ops, want_files, want_info, what):
        _same(self.im.host("files", rc.FILE, self.n_files), want_files, rc.FILE.names, what)
        assert self.im.host("info", np.uint32, rc.INFO_WORDS).tolist() == [int(x) for x in want_info], what
        assert self.im.host("ops", rc.OP, self.n_ops).tobytes() == ops.tobytes(), f"{what}: the ops changed"
        self.im.guards(what)


def run_fold(hf, dev, ops, files, what):
    f = Fold(dev, ops, files)
    f.call(hf)
    torch.cuda.synchronize()
    want = files.copy()
    info = rc.file_length(ops, want)
    f.check(ops, want, info, what)
    return want, info


INODE = 0x0123456789ABCDEF


def finished_ops(rng, n, inode=INODE, chains=None):
    """n finished ops of one inode: status 0, a valid last id, lengths that tie now and then."""
    ops = rc.new_ops(n)
    chunk = rng.integers(0, 6, n)
    ids = [rc.meta_id(inode, int(c)) for c in chunk]
    ops["last_hi"], ops["last_lo"] = [i >> 64 for i in ids], [i & rc.M64 for i in ids]
    ops["last_len"] = rng.choice([0, 4096, 17, 4095], n)
    ops["total_len"] = rng.integers(0, 1 << 40, n)
    ops["total_chunks"] = rng.integers(1, 50, n)
    ops["chain_id"] = rng.integers(0, 1 << 30, n) if chains is None else chains
    ops["status"], ops["more"], ops["list_first"], ops["last_index"], ops["reserved1"] = 0, 0, 0, 0, 0
    return ops


RUNGS = ("enters", "not found", "fails", "empty", "invalid id", "other inode", "busy")


def apply_rung(op, rung):
    if rung == "not found":
        op["status"] = rc.CHUNK_NOT_FOUND
    elif rung == "fails":
        op["status"] = 4032
    elif rung == "empty":
        op["total_chunks"] = 0
    elif rung == "invalid id":
        op["last_hi"], op["last_lo"] = rc.INVALID_ID >> 64, rc.INVALID_ID & rc.M64
    elif rung == "other inode":
        op["last_hi"] = int(op["last_hi"]) ^ 1
    elif rung == "busy":
        op["last_lo"] = (int(op["last_lo"]) & ~0xFFFFFFFF) | 4  # chunk 4 >= maxStripe 4 < stripeSize 5


def test_every_rung_in_every_position_of_a_4_op_file(hf, dev):
    rng = np.random.default_rng(0xF11E)
    combos = [(a, b, c, d) for a in RUNGS for b in RUNGS for c in RUNGS for d in RUNGS]
    ops = finished_ops(rng, 4 * len(combos))
    ops["last_lo"] &= ~np.uint64(4)  # chunks 0..3: only the busy rung reaches chunk 4
    files = rc.new_files(len(combos))
    files["inode"], files["n_file_ops"], files["chunk_size"] = INODE, 4, 4096
    files["first_op"] = 4 * np.arange(len(combos))
    files["stripe_size"], files["flags"] = 5, rc.DYN
    for f, combo in enumerate(combos):
        for k, rung in enumerate(combo):
            apply_rung(ops[4 * f + k], rung)
    want, info = run_fold(hf, dev, ops, files, "every rung")
    assert set(want["status"].tolist()) == {0, 2, 4032, 3019} and info[2] > 0 and info[3] > 0 and info[4] > 0
    assert info[0] + info[1] == len(combos) == 2401


def test_file_sizes_ties_and_replacement(hf, dev):
    rng = np.random.default_rng(0x51235)
    sizes = [0, 1, 200, 1024, 1025, 4, 4, 4, 3, 3]
    ops = finished_ops(rng, 2300, chains=rng.integers(0, 700, 2300))  # duplicate chain ids in the long files
    files = rc.new_files(len(sizes) + 2)
    files["inode"], files["chunk_size"], files["stripe_size"] = INODE, 4096, 2000
    files["n_file_ops"][:len(sizes)] = sizes
    files["first_op"][:len(sizes)] = [0, 0, 1, 201, 1225, 2250, 2254, 2258, 2262, 2265]
    # a duplicate chain id before and after the winner: chain 7's second op wins, chain 9's first is replaced
    for base, rows in ((2250, [(7, 1, 0), (7, 5, 1), (9, 5, 4000), (9, 0, 0)]),
                       (2254, [(9, 5, 4000), (7, 5, 1), (9, 0, 0), (7, 5, 2)]),
                       (2258, [(1, 3, 0), (2, 2, 4096), (3, 3, 0), (0, 1, 0)])):
        for k, (chain, chunk, last_len) in enumerate(rows):
            i = rc.meta_id(INODE, chunk)
            o = ops[base + k]
            o["chain_id"], o["last_hi"], o["last_lo"], o["last_len"] = chain, i >> 64, i & rc.M64, last_len
    # the (c, chunk_size) / (c + 1, 0) tie in both chain orders
    for base, rows in ((2262, [(5, 1, 4096), (6, 2, 0), (4, 0, 9)]), (2265, [(6, 1, 4096), (5, 2, 0), (9, 0, 9)])):
        for k, (chain, chunk, last_len) in enumerate(rows):
            i = rc.meta_id(INODE, chunk)
            o = ops[base + k]
            o["chain_id"], o["last_hi"], o["last_lo"], o["last_len"] = chain, i >> 64, i & rc.M64, last_len
    files["first_op"][10], files["n_file_ops"][10] = 2299, 2       # a segment past n_ops
    files["first_op"][11], files["n_file_ops"][11] = 0xFFFFFFFF, 1  # first_op + n_file_ops past 32 bits
    want, info = run_fold(hf, dev, ops, files, "file sizes")
    assert want["status"].tolist() == [0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 3, 3]
    assert (want[5]["last_chunk"], want[5]["last_chunk_len"]) == (5, 1) and want[6]["last_chunk_len"] == 2
    assert (want[8]["last_chunk"], want[8]["last_chunk_len"]) == (1, 4096)
    assert (want[9]["last_chunk"], want[9]["last_chunk_len"]) == (2, 0)
    assert want[3]["total_chunks"] < int(ops["total_chunks"][201:1225].sum()), "no chain id repeated in 1024 ops"


def test_70001_files(hf, dev):
    rng = np.random.default_rng(0x70001)
    n = 70001
    ops = finished_ops(rng, 4 * n, chains=rng.integers(0, 6, 4 * n))
    ops["status"] = rng.choice([0, 0, 0, 0, 0, 0, rc.CHUNK_NOT_FOUND, 4032], 4 * n)
    ops["total_chunks"][rng.random(4 * n) < 0.1] = 0
    files = rc.new_files(n)
    files["inode"], files["chunk_size"], files["stripe_size"] = INODE, 1 << 20, 8
    files["first_op"] = rng.integers(0, 4 * n - 8, n)  # segments overlap
    files["n_file_ops"] = rng.integers(0, 9, n)
    files["flags"] = rng.integers(0, 2, n)
    want, info = run_fold(hf, dev, ops, files, "70,001 files")
    assert info[0] > n // 4 and info[4] > 100 and info[2] > 100 and info[3] > 1000


def test_no_files_and_no_ops(hf, dev):
    want, info = run_fold(hf, dev, rc.new_ops(0), rc.new_files(0), "nothing")
    assert info == [0] * 8
    files = rc.new_files(3)
    files["n_file_ops"] = [0, 1, 0]
    files["first_op"] = [0, 0, 1]
    want, info = run_fold(hf, dev, rc.new_ops(0), files, "files of no op")
    assert want["status"].tolist() == [0, 3, 3] and info == [1, 2, 1, 0, 0, 0, 0, 0]


# ---- one queue, one synchronize ----
def test_four_tables_then_the_fold_on_one_queue(hf, dev):
    """Four chain tables, four range_query calls into disjoint slices of one op array, then
    file_length over 1,000 files of four ops, all queued on one stream and waited for once.  A call's
    ops are contiguous and so are a file's: the files [250 c, 250 c + 250) live on table c, and a file's
    four ops walk four chunk ranges of its inode under four chain ids."""
    rng = np.random.default_rng(0x4C4A)
    tables, ops, files = [], rc.new_ops(4000), rc.new_files(1000)
    files["chunk_size"], files["stripe_size"], files["n_file_ops"] = 4096, 4, 4
    files["first_op"] = 4 * np.arange(1000)
    for c in range(4):
        ids, lengths = [], []
        for f in range(250 * c, 250 * c + 250):
            inode = 1000 + 3 * f
            files[f]["inode"] = inode
            chunks = np.flatnonzero(rng.random(32) < (0.0 if f % 50 == 7 else 0.6))
            ids += [rc.meta_id(inode, int(k)) for k in chunks]
            lengths += rng.integers(1, 4097, chunks.size).tolist()
            for s in range(4):
                o = ops[4 * f + s]
                rc.set_range(o, rc.meta_id(inode, 8 * s), rc.meta_id(inode, 0, 1) if s == 3 else rc.meta_id(inode, 8 * s + 8))
                o["max_chunks"], o["chain_id"] = (1 if f % 2 else 0xFFFFFFFF), 900 - s - 4 * c
        tables.append(rc.new_meta(ids, lengths, np.where(rng.random(len(ids)) < 0.1, 1, 0)))
    im = Images(dev, ops=ops.nbytes, files=files.nbytes, finfo=32,
                **{f"meta{c}": tables[c].nbytes for c in range(4)}, **{f"info{c}": 32 for c in range(4)})
    im.put("ops", ops)
    im.put("files", files)
    for c in range(4):
        im.put(f"meta{c}", tables[c])
    torch.cuda.synchronize()
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        for c in range(4):
            hf.range_query(im.t[f"meta{c}"], tables[c].size, im.t["ops"][96000 * c:], 1000, im.t[f"info{c}"], stream=st)
        hf.file_length(im.t["ops"], 4000, im.t["files"], 1000, im.t["finfo"], stream=st)
    st.synchronize()
    want_ops, want_files = ops.copy(), files.copy()
    for c in range(4):
        info, _ = rc.range_query(tables[c], want_ops[1000 * c:1000 * c + 1000], 0)
        assert im.host(f"info{c}", np.uint32, 8).tolist() == info and info[0] == 1000 and info[2] > 1000
    finfo = rc.file_length(want_ops, want_files)
    _same(im.host("ops", rc.OP, 4000), want_ops, rc.OP.names, "queued ops")
    _same(im.host("files", rc.FILE, 1000), want_files, rc.FILE.names, "queued files")
    assert im.host("finfo", np.uint32, 8).tolist() == finfo and finfo[0] == 1000 and finfo[2] >= 20
    assert (want_files["length"] > 20 * 4096).sum() > 500
    im.guards("queued")
    hf._lib.release_stream(st)


# ---- lifetime and context ----
def test_poisoned_scratch(hf, dev, opts):
    """Every scratch word is written before it is read: the results do not change when the call's
    scratch starts from a pattern."""
    opts("poison", 0xA5A5A5A5)
    st = torch.cuda.Stream(dev)
    for n in (0, 257, 70001):
        rng = np.random.default_rng(0xA5 + n)
        meta = rc.random_table(rng, n, max_len=1 << 32)
        ops = rc.random_ops(rng, meta, 700)
        with torch.cuda.stream(st):
            run_query(hf, dev, meta, ops, 1 << 16, f"poisoned, {n} records", stream=st)
    hf._lib.release_stream(st)


def test_graph_replay_over_a_rewritten_table_and_ops(hf, dev):
    rng = np.random.default_rng(0x6A)
    first = rc.random_table(rng, 5000, max_len=1 << 32)
    ops1 = rc.random_ops(rng, first, 600)
    second = rc.random_table(rng, 5000, hi_values=(2, 7))
    ops2 = rc.random_ops(rng, second, 600, remove_p=0.9)
    third = second.copy()
    third[[77, 78]] = third[[78, 77]]  # unsorted at one replay
    files = rc.new_files(150)
    files["inode"], files["first_op"], files["n_file_ops"] = 0x70000, 4 * np.arange(150), 4
    files["chunk_size"], files["stripe_size"] = 4096, 4
    q = Query(dev, first, ops1, 1 << 15)
    fim = Images(dev, files=files.nbytes, finfo=32)
    fim.put("files", files)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        q.call(hf, torch.cuda.current_stream())
        hf.file_length(q.im.t["ops"], 600, fim.t["files"], 150, fim.t["finfo"], stream=torch.cuda.current_stream())
    for k, (meta, ops) in enumerate(((first, ops1), (second, ops2), (third, ops2), (first, ops1))):
        q.put(meta, ops)
        g.replay()
        torch.cuda.synchronize()
        want = ops.copy()
        info, lst = rc.range_query(meta, want, 1 << 15)
        q.check(meta, want, info, lst, f"replay {k}")
        want_files = files.copy()
        finfo = rc.file_length(want, want_files)
        _same(fim.host("files", rc.FILE, 150), want_files, rc.FILE.names, f"replay {k}: files")
        assert fim.host("finfo", np.uint32, 8).tolist() == finfo
        assert (info[7] != 0) == (k == 2)


def test_sync_plan_and_range_query_through_one_pair_buffer(hf, dev):
    """Both calls carve the calling pair's one call buffer: alternated on one stream, with either the
    larger, each leaves what it leaves alone."""
    rng = np.random.default_rng(0x5A1)
    st = torch.cuda.Stream(dev)
    small, large = rc.random_table(rng, 300), rc.random_table(rng, 40000)
    plans = {}
    with torch.cuda.stream(st):
        for round_, (sync_table, range_table) in enumerate(((small, large), (large, small), (small, small))):
            local = torch.from_numpy(sync_table.view(np.uint8).copy()).to(dev)
            remote = torch.from_numpy(sync_table[::2].copy().view(np.uint8)).to(dev)
            info = torch.full((hf.SYNC_INFO_WORDS,), -1, dtype=torch.int32, device=dev)
            ops = rc.random_ops(rng, range_table, 500)
            q = Query(dev, range_table, ops, 1 << 15)
            hf.sync_plan(local, sync_table.size, remote, (sync_table.size + 1) // 2, 1, info, stream=st)
            q.call(hf, st)
            hf.sync_plan(local, sync_table.size, remote, (sync_table.size + 1) // 2, 1, info, stream=st)
            st.synchronize()
            want = ops.copy()
            rinfo, lst = rc.range_query(range_table, want, 1 << 15)
            q.check(range_table, want, rinfo, lst, f"round {round_}")
            got = info.cpu().numpy().view(np.uint32).tolist()
            assert got[hf.SYNC_INFO_NAMES.index("remote_miss")] == sync_table.size // 2
            assert got[hf.SYNC_INFO_NAMES.index("n_write")] == sync_table.size // 2
            plans.setdefault(sync_table.size, got)
            assert plans[sync_table.size] == got
    hf._lib.release_stream(st)


def test_two_threads(hf, dev):
    errors = []

    def worker(seed):
        try:
            torch.cuda.set_device(dev)
            rng = np.random.default_rng(seed)
            st = torch.cuda.Stream(dev)
            with torch.cuda.stream(st):
                for n in (1000, 70001, 257):
                    meta = rc.random_table(rng, n, max_len=1 << 32)
                    ops = rc.random_ops(rng, meta, 400)
                    q = Query(dev, meta, ops, 1 << 14)
                    q.call(hf, st)
                    st.synchronize()
                    want = ops.copy()
                    info, lst = rc.range_query(meta, want, 1 << 14)
                    q.check(meta, want, info, lst, f"thread {seed}, {n} records")
            hf._lib.release_stream(st)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(s,)) for s in (1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
