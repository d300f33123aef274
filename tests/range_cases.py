"""A model of hf3fs_crc_range_query and hf3fs_crc_file_length written from the reference's lines, and
the case builders of the range tests.

The model restates, line for line:
  query_chunks            ChunkStore::queryChunks (src/storage/store/ChunkStore.cc:120-147): an iterator
                          that seeks to `end` and descends, skips id == end, stops below `begin` or at
                          maxNumChunkIdsToProcess results
  process_query_results   StorageOperator::processQueryResults (src/storage/service/StorageOperator.cc:
                          653-751): the paged loop, with the page size max_num_results_per_query a parameter
  query_last_chunk        StorageOperator::queryLastChunk's processor (:875-891)
  remove_chunks           StorageOperator::removeChunks' processor (:949-971): the order of doRemove
  query_chunks_by_chain   FileOperation::queryChunksByChain (src/fbs/meta/FileOperation.cc:78-179), over
                          an ordered map keyed by chain id
  query_chunks            FileOperation::queryChunks' fold (:45-76)
closed_form() is the entry point's own statement (include/hf3fs_crc.h) with bisect and prefix sums;
tests/test_range_model.py holds it to the paged loop, and the large GPU cases use it.

Ids are Python ints (hi << 64 | lo): ChunkId(high, low) is the 16 big-endian bytes, so ChunkId's
operator< is the integer order."""
import bisect

import numpy as np

META = np.dtype([("id_hi", "<u8"), ("id_lo", "<u8"), ("chain_ver", "<u4"), ("update_ver", "<u4"),
                 ("commit_ver", "<u4"), ("checksum", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                 ("chunk_state", "u1"), ("recycle_state", "u1"), ("checksum_type", "u1"), ("out_class", "u1"),
                 ("out_peer", "<u4")])
OP = np.dtype([("begin_hi", "<u8"), ("begin_lo", "<u8"), ("end_hi", "<u8"), ("end_lo", "<u8"),
               ("max_chunks", "<u4"), ("status_in", "<i4"), ("kind", "u1"), ("reserved0", "u1", (3,)),
               ("chain_id", "<u4"),
               ("last_hi", "<u8"), ("last_lo", "<u8"), ("total_len", "<u8"), ("total_chunks", "<u4"),
               ("last_len", "<u4"), ("last_index", "<u4"), ("list_first", "<u4"), ("status", "<i4"),
               ("more", "u1"), ("reserved1", "u1", (3,))])
FILE = np.dtype([("inode", "<u8"), ("first_op", "<u4"), ("n_file_ops", "<u4"), ("chunk_size", "<u4"),
                 ("stripe_size", "<u4"), ("flags", "u1"), ("reserved", "u1", (3,)),
                 ("status", "<i4"), ("length", "<u8"), ("total_len", "<u8"), ("total_chunks", "<u8"),
                 ("last_chunk", "<u4"), ("last_chunk_len", "<u4")])
assert META.itemsize == 48 and OP.itemsize == 96 and FILE.itemsize == 64
OP_OUT = ("last_hi", "last_lo", "total_len", "total_chunks", "last_len", "last_index", "list_first", "status", "more",
          "reserved1")
FILE_OUT = ("status", "length", "total_len", "total_chunks", "last_chunk", "last_chunk_len")

QUERY, REMOVE = 1, 2
NONE = 0xFFFFFFFF
INFO_WORDS = 8
INVALID_ARG, DATA_CORRUPTION, CHUNK_NOT_FOUND, META_BUSY = 3, 2, 7007, 3019
DYN = 1
MAX_FILE_OPS = 1024
UINT32_MAX = 0xFFFFFFFF
M64 = (1 << 64) - 1
INVALID_ID = (0x0000FFFFFFFFFFFF << 64) | 0xFFFF000000000000  # meta::ChunkId(InodeId(-1), 0, 0)


def ident(hi, lo):
    return (int(hi) << 64) | int(lo)


def meta_id(inode, chunk, track=0):
    """meta::ChunkId(inode, track, chunk) (Schema.h:177-198) as an integer id."""
    return ((inode >> 16) << 64) | ((inode & 0xFFFF) << 48) | (track << 32) | chunk


def new_meta(ids, lengths=None, recycle=None):
    m = np.zeros(len(ids), dtype=META)
    m["id_hi"] = [i >> 64 for i in ids]
    m["id_lo"] = [i & M64 for i in ids]
    if lengths is not None:
        m["length"] = lengths
    if recycle is not None:
        m["recycle_state"] = recycle
    m["out_peer"] = NONE
    return m


def new_ops(n):
    o = np.zeros(n, dtype=OP)
    o["kind"] = QUERY
    for f in OP_OUT:  # junk the call must overwrite
        o[f] = 0xA5 if OP[f].itemsize == 1 or f == "reserved1" else 0x5A5A5A5A
    return o


def set_range(op, begin, end):
    op["begin_hi"], op["begin_lo"] = begin >> 64, begin & M64
    op["end_hi"], op["end_lo"] = end >> 64, end & M64


def new_files(n):
    f = np.zeros(n, dtype=FILE)
    for name in FILE_OUT:
        f[name] = 0x5A5A5A5A
    return f


def table_ids(meta):
    return [ident(h, l) for h, l in zip(meta["id_hi"].tolist(), meta["id_lo"].tolist())]


# ---- the storage side -------------------------------------------------------------------------

class Table:
    """One target's metadata in the iterator's order."""

    def __init__(self, meta):
        self.ids = table_ids(meta)
        self.recycle = meta["recycle_state"].tolist()
        self.length = meta["length"].tolist()
        hi, lo = meta["id_hi"], meta["id_lo"]
        self.unsorted = int(((hi[:-1] > hi[1:]) | ((hi[:-1] == hi[1:]) & (lo[:-1] >= lo[1:]))).sum())


def query_chunks(t, begin, end, max_num):
    """ChunkStore.cc:120-147 -> [(index, id)] in the iterator's (descending) order."""
    out = []
    it = bisect.bisect_right(t.ids, end) - 1  # metaStore_.iterator(end): the first key at or below end
    while it >= 0 and len(out) < max_num:  # :128
        chunk_id = t.ids[it]
        if chunk_id == end:  # :132  [begin, end)
            it -= 1
            continue
        if chunk_id < begin:  # :136
            break
        out.append((it, chunk_id))
        it -= 1
    return out


def process_query_results(t, begin, end, max_chunks, page, processor):
    """StorageOperator.cc:653-751 -> (processed chunks, moreChunksInRange)."""
    num_to_process = min(max_chunks, UINT32_MAX - 1) if max_chunks else UINT32_MAX - 1  # :658-660
    current_end = end
    num_results = 0
    while True:
        current_max = min(num_to_process - num_results + 1, page)  # :667
        result = query_chunks(t, begin, current_end, current_max)
        done = False
        for index, chunk_id in result:
            if t.recycle[index] != 0:  # :677-696
                continue
            if num_results < num_to_process:  # :698
                processor(index, chunk_id)
            num_results += 1
            if num_results >= num_to_process + 1:  # :709
                done = True
                break
        if done or len(result) < current_max:  # :719
            break
        current_end = result[-1][1]  # :728-729
    return min(num_results, num_to_process), num_results > num_to_process  # :743,750


def query_last_chunk(t, begin, end, max_chunks, page):
    """:858-916 for one payload -> the result's fields."""
    r = {"last_id": None, "last_len": 0, "total_len": 0, "total_chunks": 0, "last_index": NONE}

    def process(index, chunk_id):  # :875-891
        if r["last_id"] is None or r["last_id"] < chunk_id:
            r["last_id"], r["last_len"], r["last_index"] = chunk_id, t.length[index], index
        r["total_len"] += t.length[index]
        r["total_chunks"] += 1

    n, more = process_query_results(t, begin, end, max_chunks, page, process)
    assert n == r["total_chunks"]
    r["more"] = more
    return r


def remove_chunks(t, begin, end, max_chunks, page):
    """:936-1000 for one payload -> (the indices doRemove is issued for, in order, more)."""
    order = []
    n, more = process_query_results(t, begin, end, max_chunks, page, lambda index, chunk_id: order.append(index))
    assert n == len(order)
    return order, more


def _failed(op, status):
    for f in OP_OUT:
        op[f] = 0
    op["last_index"] = NONE
    op["status"] = status


def range_query(meta, ops, list_cap, page=1000):
    """The whole call by the paged loop: fills the ops' outputs, returns (info, list below list_cap)."""
    t = Table(meta)
    entries, chunks = [], 0
    for op in ops:
        first = min(len(entries), NONE)
        if t.unsorted:
            _failed(op, INVALID_ARG)
        elif op["status_in"] != 0:
            _failed(op, int(op["status_in"]))
        elif op["kind"] not in (QUERY, REMOVE):
            _failed(op, INVALID_ARG)
        else:
            begin, end = ident(op["begin_hi"], op["begin_lo"]), ident(op["end_hi"], op["end_lo"])
            r = query_last_chunk(t, begin, end, int(op["max_chunks"]), page)
            last = r["last_id"] or 0
            op["last_hi"], op["last_lo"] = last >> 64, last & M64
            op["total_len"], op["total_chunks"], op["last_len"] = r["total_len"], r["total_chunks"], r["last_len"]
            op["last_index"], op["status"], op["more"], op["reserved1"] = r["last_index"], 0, r["more"], 0
            chunks += r["total_chunks"]
            if op["kind"] == REMOVE:
                order, more = remove_chunks(t, begin, end, int(op["max_chunks"]), page)
                assert len(order) == r["total_chunks"] and more == r["more"]
                entries += order
        op["list_first"] = first
    return _info(ops, chunks, len(entries), list_cap, t.unsorted), np.array(entries[:list_cap], dtype=np.uint32)


def _info(ops, chunks, listed, list_cap, unsorted):
    ok = int((ops["status"] == 0).sum())
    return [ok, len(ops) - ok, chunks & UINT32_MAX, chunks >> 32, listed & UINT32_MAX, listed >> 32,
            1 if listed > list_cap else 0, unsorted]


def closed_form(meta, ops, list_cap):
    """The same call by the header's closed form: two bisects for the span, prefix sums of the normal
    records' count and length."""
    t = Table(meta)
    normal = (meta["recycle_state"] == 0)
    cnt = np.concatenate([[0], np.cumsum(normal.astype(np.int64))])
    length = np.zeros(len(meta) + 1, dtype=np.uint64)
    length[1:] = np.cumsum(np.where(normal, meta["length"], 0).astype(np.uint64))
    normal_index = np.flatnonzero(normal)
    entries, listed, chunks = [], 0, 0
    for op in ops:
        first = min(listed, NONE)
        if t.unsorted:
            _failed(op, INVALID_ARG)
        elif op["status_in"] != 0:
            _failed(op, int(op["status_in"]))
        elif op["kind"] not in (QUERY, REMOVE):
            _failed(op, INVALID_ARG)
        else:
            begin, end = ident(op["begin_hi"], op["begin_lo"]), ident(op["end_hi"], op["end_lo"])
            _failed(op, 0)
            if begin < end:
                a, b = bisect.bisect_left(t.ids, begin), bisect.bisect_left(t.ids, end)
                normals = int(cnt[b] - cnt[a])
                limit = min(int(op["max_chunks"]), UINT32_MAX - 1) if op["max_chunks"] else UINT32_MAX - 1
                total = min(normals, limit)
                op["more"] = normals > limit
                op["total_chunks"] = total
                if total:
                    picked = normal_index[int(cnt[b]) - total:int(cnt[b])]  # ascending
                    high = int(picked[-1])
                    op["total_len"] = int(length[b]) - int(length[int(picked[0])])
                    op["last_index"], op["last_len"] = high, t.length[high]
                    op["last_hi"], op["last_lo"] = t.ids[high] >> 64, t.ids[high] & M64
                    chunks += total
                    if op["kind"] == REMOVE:
                        entries.append(picked[::-1])
                        listed += total
        op["list_first"] = first
    flat = np.concatenate(entries).astype(np.uint32) if entries else np.zeros(0, dtype=np.uint32)
    return _info(ops, chunks, listed, list_cap, t.unsorted), flat[:list_cap]


# ---- the meta side ----------------------------------------------------------------------------

def id_inode(i):
    """ChunkId::inode() of the 16 bytes (Schema.h:217)."""
    return (((i >> 64) & 0xFFFFFFFFFFFF) << 16) | ((i & M64) >> 48)


def id_chunk(i):
    """ChunkId::chunk() (Schema.h:220)."""
    return i & 0xFFFFFFFF


def query_chunks_by_chain(f, ops):
    """FileOperation.cc:78-179 -> (error code, None) or (0, map); also the 7007 ops passed."""
    chunks = {}  # std::map<ChainId, QueryResult>: iterated in key order below
    not_found = 0
    max_stripe = int(f["n_file_ops"])
    for q in ops[int(f["first_op"]):int(f["first_op"]) + max_stripe]:
        if q["status"] != 0:  # :129
            if q["status"] == CHUNK_NOT_FOUND:
                not_found += 1
                continue
            return int(q["status"]), None, not_found
        if q["total_chunks"] == 0:  # :142
            continue
        chunk_id = ident(q["last_hi"], q["last_lo"])
        if chunk_id == INVALID_ID:  # :147
            return DATA_CORRUPTION, None, not_found
        if id_inode(chunk_id) != int(f["inode"]):  # :154
            return DATA_CORRUPTION, None, not_found
        if (f["flags"] & DYN) and max_stripe < int(f["stripe_size"]) and id_chunk(chunk_id) >= max_stripe:  # :162
            return META_BUSY, None, not_found
        chunks[int(q["chain_id"])] = {  # :170
            "length": id_chunk(chunk_id) * int(f["chunk_size"]) + int(q["last_len"]),
            "last_chunk": id_chunk(chunk_id), "last_chunk_len": int(q["last_len"]),
            "total_len": int(q["total_len"]), "total_chunks": int(q["total_chunks"])}
    return 0, chunks, not_found


def file_length(ops, files):
    """The whole call: fills the files' outputs, returns info."""
    info = [0] * INFO_WORDS
    for f in files:
        for name in FILE_OUT:
            f[name] = 0
        if f["n_file_ops"] > MAX_FILE_OPS or int(f["first_op"]) + int(f["n_file_ops"]) > len(ops):
            f["status"] = INVALID_ARG
            info[1] += 1
            continue
        code, chains, not_found = query_chunks_by_chain(f, ops)
        info[3] += not_found
        if code:
            f["status"] = code
            info[1] += 1
            info[4] += code == META_BUSY
            info[5] += code == DATA_CORRUPTION
            continue
        result = {"length": 0, "last_chunk": 0, "last_chunk_len": 0, "total_len": 0, "total_chunks": 0}
        first = True
        for chain in sorted(chains):  # :49  the map's order
            c = chains[chain]
            if first or result["length"] < c["length"]:  # :58
                result["length"], result["last_chunk"] = c["length"], c["last_chunk"]
                result["last_chunk_len"] = c["last_chunk_len"]
            first = False
            result["total_len"] += c["total_len"]
            result["total_chunks"] += c["total_chunks"]
        assert result["last_chunk"] * int(f["chunk_size"]) + result["last_chunk_len"] == result["length"]  # :67-73
        for name in result:
            f[name] = result[name] & M64
        info[0] += 1
        info[2] += not chains
    return info


# ---- case builders ----------------------------------------------------------------------------

def random_table(rng, n, hi_values=(7,), max_len=1 << 20, recycle_p=0.2):
    """n records with distinct ids, ascending; lengths below max_len; recycle states 1 and 2 mixed in."""
    lows = np.sort(rng.choice(max(4 * n, 16), n, replace=False)).astype(np.uint64) * np.uint64(3) + np.uint64(1)
    his = np.sort(rng.choice(hi_values, n)).astype(np.uint64)
    ids = sorted(ident(h, l) for h, l in zip(his.tolist(), lows.tolist()))
    m = new_meta(ids, rng.integers(0, max_len, n, dtype=np.uint64).astype(np.uint32),
                 np.where(rng.random(n) < recycle_p, rng.integers(1, 3, n), 0))
    return m


def random_ops(rng, meta, n_ops, max_span=40, remove_p=0.5):
    """Ops around the table's ids: begin / end at ids, their neighbours and gaps; limits around the
    span's size; some empty, reversed and failed ones."""
    ids = table_ids(meta)
    ops = new_ops(n_ops)
    n = len(ids)
    for k in range(n_ops):
        if n:
            a = int(rng.integers(0, n))
            b = min(n - 1, a + int(rng.integers(0, max_span)))
            begin = ids[a] + int(rng.integers(-1, 2))
            end = ids[b] + int(rng.integers(-1, 2))
        else:
            begin, end = int(rng.integers(0, 100)), int(rng.integers(0, 100))
        if k % 17 == 5:
            begin, end = end, begin
        set_range(ops[k], max(begin, 0), max(end, 0))
        ops[k]["kind"] = REMOVE if rng.random() < remove_p else QUERY
        ops[k]["max_chunks"] = rng.choice([0, 0, 1, 2, 5, max_span // 2, UINT32_MAX])
        ops[k]["chain_id"] = rng.integers(0, 1 << 20)
        if k % 29 == 7:
            ops[k]["status_in"] = rng.choice([4032, -1, 7007])
        if k % 31 == 9:
            ops[k]["kind"] = rng.choice([0, 3, 255])
    return ops
