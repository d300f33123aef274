"""The Python model of hf3fs_crc_range_query and hf3fs_crc_file_length (tests/range_cases.py) against
ranges and files worked by hand from the reference's lines; the paged loop at page sizes 1, 2, 3, 7
and 1000 giving one answer, which is also the closed form's; then, with the library: the record
layouts against the package's ctypes mirrors and the header, the constants, the scratch-size function
and every argument error (answered before a device is touched, so no GPU is needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import range_cases as rc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGES = (1, 2, 3, 7, 1000)


def hand_table():
    """Six records of one id_hi; record 2 is being removed, record 4 is a dummy being removed."""
    return rc.new_meta([rc.ident(7, lo) for lo in (10, 20, 30, 40, 50, 60)], [100, 200, 300, 400, 500, 600],
                       [0, 0, 1, 0, 2, 0])


def one_op(begin, end, max_chunks=0, kind=rc.QUERY, **fields):
    ops = rc.new_ops(1)
    rc.set_range(ops[0], begin, end)
    ops["max_chunks"], ops["kind"] = max_chunks, kind
    for k, v in fields.items():
        ops[k] = v
    return ops


@pytest.mark.parametrize("page", PAGES)
def test_span_by_hand(page):
    meta = hand_table()
    # [20, 60): records 1..4, normal 1 and 3; end's own record (60) is excluded, begin's (20) included
    ops = one_op(rc.ident(7, 20), rc.ident(7, 60), kind=rc.REMOVE)
    info, lst = rc.range_query(meta, ops, 16, page)
    o = ops[0]
    assert (o["total_chunks"], o["total_len"], o["more"], o["status"]) == (2, 600, 0, 0)
    assert (o["last_hi"], o["last_lo"], o["last_len"], o["last_index"], o["list_first"]) == (7, 40, 400, 3, 0)
    assert lst.tolist() == [3, 1]  # the walk descends from `end`
    assert info == [1, 0, 2, 0, 2, 0, 0, 0]


@pytest.mark.parametrize("page", PAGES)
def test_limit_by_hand(page):
    meta = hand_table()
    whole = (rc.ident(0, 0), rc.ident(8, 0))  # normal records 0, 1, 3, 5
    for limit, chunks, length, more, lst in ((1, 1, 600, 1, [5]), (3, 3, 1200, 1, [5, 3, 1]),
                                             (4, 4, 1300, 0, [5, 3, 1, 0]), (5, 4, 1300, 0, [5, 3, 1, 0]),
                                             (0, 4, 1300, 0, [5, 3, 1, 0]), (0xFFFFFFFF, 4, 1300, 0, [5, 3, 1, 0])):
        ops = one_op(*whole, max_chunks=limit, kind=rc.REMOVE)
        info, got = rc.range_query(meta, ops, 16, page)
        o = ops[0]
        assert (o["total_chunks"], o["total_len"], o["more"]) == (chunks, length, more), limit
        assert (o["last_lo"], o["last_len"], o["last_index"]) == (60, 600, 5) and got.tolist() == lst


def test_empty_spans_by_hand():
    meta = hand_table()
    for begin, end in ((rc.ident(7, 30), rc.ident(7, 30)), (rc.ident(7, 40), rc.ident(7, 20)),
                       (rc.ident(7, 21), rc.ident(7, 30)),   # a gap
                       (rc.ident(7, 30), rc.ident(7, 31)),   # one record, being removed
                       (rc.ident(7, 61), rc.ident(9, 0)), (rc.ident(0, 0), rc.ident(7, 10))):
        ops = one_op(begin, end, kind=rc.REMOVE)
        info, lst = rc.range_query(meta, ops, 16, 3)
        o = ops[0]
        assert (o["total_chunks"], o["total_len"], o["more"], o["status"], o["last_index"]) == (0, 0, 0, 0, rc.NONE)
        assert (o["last_hi"], o["last_lo"], o["last_len"]) == (0, 0, 0) and lst.size == 0
        assert info == [1, 0, 0, 0, 0, 0, 0, 0]


def test_failed_ops_and_list_segments_by_hand():
    meta = hand_table()
    ops = rc.new_ops(5)
    for k in range(5):
        rc.set_range(ops[k], rc.ident(7, 0), rc.ident(7, 100))
    ops["kind"] = [rc.REMOVE, rc.QUERY, 9, rc.REMOVE, rc.REMOVE]
    ops["status_in"] = [0, 0, 0, 4032, 0]
    ops["max_chunks"] = [2, 0, 0, 0, 0]
    info, lst = rc.range_query(meta, ops, 5)
    assert ops["status"].tolist() == [0, 0, 3, 4032, 0]
    assert ops["total_chunks"].tolist() == [2, 4, 0, 0, 4] and ops["more"].tolist() == [1, 0, 0, 0, 0]
    assert ops["list_first"].tolist() == [0, 2, 2, 2, 2]  # a QUERY op carries the running offset
    assert ops["last_index"].tolist() == [5, 5, rc.NONE, rc.NONE, 5]
    assert lst.tolist() == [5, 3, 5, 3, 1]  # six entries, five fit
    assert info == [3, 2, 10, 0, 6, 0, 1, 0]


def test_unsorted_table_by_hand():
    meta = hand_table()
    meta["id_lo"][3] = 30  # a duplicate of record 2 ...
    meta["id_lo"][5] = 45  # ... and an inversion against record 4
    ops = one_op(rc.ident(0, 0), rc.ident(9, 0), kind=rc.REMOVE)
    info, lst = rc.range_query(meta, ops, 16)
    assert info == [0, 1, 0, 0, 0, 0, 0, 2] and lst.size == 0
    assert (ops[0]["status"], ops[0]["total_chunks"], ops[0]["last_index"], ops[0]["list_first"]) == (3, 0, rc.NONE, 0)


def test_ids_order_by_hi_then_lo_unsigned():
    ids = [rc.ident(0, rc.M64), rc.ident(1, 0), rc.ident(1, 1 << 63), rc.ident(1 << 63, 0), rc.ident(rc.M64, rc.M64)]
    meta = rc.new_meta(ids, [1, 2, 4, 8, 16])
    ops = one_op(rc.ident(1, 0), rc.ident(rc.M64, rc.M64))
    rc.range_query(meta, ops, 0)
    assert (ops[0]["total_chunks"], ops[0]["total_len"], ops[0]["last_hi"], ops[0]["last_lo"]) == (3, 14, 1 << 63, 0)


@pytest.mark.parametrize("seed", range(6))
def test_page_size_changes_nothing_and_closed_form_agrees(seed):
    rng = np.random.default_rng(0x9A6E + seed)
    meta = rc.random_table(rng, int(rng.integers(0, 120)), hi_values=(3, 4, 9), max_len=1 << 32)
    ops = rc.random_ops(rng, meta, 60)
    want = None
    for page in PAGES:
        got = ops.copy()
        info, lst = rc.range_query(meta, got, 200, page)
        if want is None:
            want = (got, info, lst)
            assert info[2] > 50 and info[4] > 20 and info[1] > 0 and got["more"].any()
        assert got.tobytes() == want[0].tobytes() and info == want[1] and np.array_equal(lst, want[2]), page
    got = ops.copy()
    info, lst = rc.closed_form(meta, got, 200)
    for f in rc.OP.names:
        assert np.array_equal(got[f], want[0][f]), f
    assert info == want[1] and np.array_equal(lst, want[2])


# ---- the file fold ----
def striped(inode, rows, chunk_size=4096, **file_fields):
    """rows: (chain_id, chunk, last_len, total_len, total_chunks, status) per op."""
    ops = rc.new_ops(len(rows))
    for o, (chain, chunk, last_len, total_len, total_chunks, status) in zip(ops, rows):
        i = rc.meta_id(inode, chunk)
        o["last_hi"], o["last_lo"] = i >> 64, i & rc.M64
        o["chain_id"], o["last_len"], o["total_len"], o["total_chunks"], o["status"] = (chain, last_len, total_len,
                                                                                      total_chunks, status)
    files = rc.new_files(1)
    files["inode"], files["first_op"], files["n_file_ops"] = inode, 0, len(rows)
    files["chunk_size"], files["stripe_size"] = chunk_size, len(rows)
    for k, v in file_fields.items():
        files[k] = v
    return ops, files


def outputs(f):
    return tuple(int(f[n]) for n in rc.FILE_OUT)


def test_meta_chunk_id_layout():
    i = rc.meta_id(0x0123456789ABCDEF, 0xDEADBEEF)
    assert i.to_bytes(16, "big").hex() == "0000" + "0123456789abcdef" + "0000" + "deadbeef"
    assert rc.id_inode(i) == 0x0123456789ABCDEF and rc.id_chunk(i) == 0xDEADBEEF
    assert rc.meta_id((1 << 64) - 1, 0) == rc.INVALID_ID


def test_file_length_by_hand():
    ops, files = striped(77, [(5, 2, 100, 9000, 3, 0), (3, 3, 0, 8000, 2, 0), (9, 1, 4096, 7000, 2, 0),
                              (4, 0, 0, 0, 0, 0), (6, 0, 0, 0, 0, 7007)])
    info = rc.file_length(ops, files)
    # lengths 8292, 12288, 8192: chain 3 wins; the empty op and the 7007 op are skipped
    assert outputs(files[0]) == (0, 12288, 24000, 7, 3, 0) and info == [1, 0, 0, 1, 0, 0, 0, 0]


def test_file_length_tie_goes_to_the_lowest_chain_in_both_orders():
    for rows in ([(5, 1, 4096, 10, 1, 0), (6, 2, 0, 20, 1, 0)], [(6, 1, 4096, 10, 1, 0), (5, 2, 0, 20, 1, 0)],
                 [(6, 2, 0, 20, 1, 0), (5, 1, 4096, 10, 1, 0)]):
        ops, files = striped(77, rows)
        rc.file_length(ops, files)
        low = min(rows)
        assert outputs(files[0]) == (0, 8192, 30, 2, low[1], low[2])


def test_file_length_later_op_of_a_chain_replaces_the_earlier():
    ops, files = striped(77, [(5, 9, 1, 100, 9, 0), (4, 3, 0, 50, 3, 0), (5, 1, 7, 10, 1, 0)])
    rc.file_length(ops, files)
    assert outputs(files[0]) == (0, 3 * 4096, 60, 4, 3, 0)  # chain 5's first op (length 36865) is gone
    # ... but not when the later op is skipped
    ops["total_chunks"][2] = 0
    rc.file_length(ops, files)
    assert outputs(files[0]) == (0, 9 * 4096 + 1, 150, 12, 9, 1)


def test_file_length_failures_by_hand():
    rows = [(1, 0, 10, 10, 1, 0), (2, 1, 10, 10, 1, 0), (3, 2, 10, 10, 1, 0)]
    ops, files = striped(77, rows)
    ops["status"][1] = 4032
    assert rc.file_length(ops, files) == [0, 1, 0, 0, 0, 0, 0, 0] and outputs(files[0]) == (4032, 0, 0, 0, 0, 0)
    ops, files = striped(77, rows)
    ops["last_hi"][2], ops["last_lo"][2] = rc.INVALID_ID >> 64, rc.INVALID_ID & rc.M64
    assert rc.file_length(ops, files) == [0, 1, 0, 0, 0, 1, 0, 0] and files[0]["status"] == 2
    ops, files = striped(77, rows)
    ops["last_lo"][0] ^= 1 << 48  # another inode
    assert rc.file_length(ops, files)[5] == 1 and files[0]["status"] == 2
    ops, files = striped(77, rows, flags=rc.DYN, stripe_size=4)
    ops["last_lo"][1] += 2  # chunk 3 >= maxStripe 3 < stripeSize 4
    assert rc.file_length(ops, files) == [0, 1, 0, 0, 1, 0, 0, 0] and files[0]["status"] == 3019
    ops, files = striped(77, rows, flags=rc.DYN, stripe_size=3)  # maxStripe == stripeSize: not busy
    ops["last_lo"][1] += 2
    assert rc.file_length(ops, files)[0] == 1 and files[0]["last_chunk"] == 3
    ops, files = striped(77, rows, n_file_ops=4)  # a segment past n_ops
    assert rc.file_length(ops, files) == [0, 1, 0, 0, 0, 0, 0, 0] and files[0]["status"] == 3
    ops, files = striped(77, [(0, 0, 0, 0, 0, 7007)] * 2)
    assert rc.file_length(ops, files) == [1, 0, 1, 2, 0, 0, 0, 0] and outputs(files[0]) == (0, 0, 0, 0, 0, 0)


def test_file_length_in_64_bits():
    ops, files = striped(77, [(1, 0xFFFFFFFF, 0xFFFFFFFF, 1 << 63, 0xFFFFFFFF, 0), (2, 0, 1, 1 << 63, 5, 0)],
                         chunk_size=0xFFFFFFFF)
    rc.file_length(ops, files)
    assert outputs(files[0]) == (0, 0xFFFFFFFF * 0xFFFFFFFF + 0xFFFFFFFF, 0, 0xFFFFFFFF + 5, 0xFFFFFFFF, 0xFFFFFFFF)


# ---- with the library: layouts, constants, sizes, argument errors ----
def test_record_layouts_match_the_package_and_the_header(hf):
    for struct, dtype in ((hf.RangeOp, rc.OP), (hf.FileLen, rc.FILE), (hf.SyncMeta, rc.META)):
        assert ctypes.sizeof(struct) == dtype.itemsize
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1], name
            assert getattr(struct, name).size == dtype.fields[name][0].itemsize, name
    assert hf.range_op_dtype() == rc.OP and hf.file_len_dtype() == rc.FILE and hf.sync_meta_dtype() == rc.META
    op = {n: rc.OP.fields[n][1] for n in rc.OP.names}
    assert (op["begin_hi"], op["begin_lo"], op["end_hi"], op["end_lo"], op["max_chunks"], op["status_in"], op["kind"],
            op["chain_id"], op["last_hi"], op["last_lo"], op["total_len"], op["total_chunks"], op["last_len"],
            op["last_index"], op["list_first"], op["status"], op["more"]) == (0, 8, 16, 24, 32, 36, 40, 44, 48, 56, 64,
                                                                              72, 76, 80, 84, 88, 92)
    fl = {n: rc.FILE.fields[n][1] for n in rc.FILE.names}
    assert (fl["inode"], fl["first_op"], fl["n_file_ops"], fl["chunk_size"], fl["stripe_size"], fl["flags"],
            fl["status"], fl["length"], fl["total_len"], fl["total_chunks"], fl["last_chunk"],
            fl["last_chunk_len"]) == (0, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 60)
    text = open(os.path.join(REPO, "include", "hf3fs_crc.h")).read()
    for struct, size in (("hf3fs_crc_range_op", 96), ("hf3fs_crc_file_len", 64)):
        assert re.search(r"static_assert\(sizeof\(%s\) == %d" % (struct, size), text), struct
    for name, at in (("max_chunks", 32), ("status_in", 36), ("kind", 40), ("chain_id", 44), ("last_hi", 48),
                     ("total_len", 64), ("total_chunks", 72), ("last_len", 76), ("last_index", 80), ("list_first", 84),
                     ("status", 88), ("more", 92)):
        assert re.search(r"offsetof\(hf3fs_crc_range_op, %s\) == %d\b" % (name, at), text), name


def test_constants_match_the_package_and_the_header(hf):
    assert (hf.RANGE_QUERY, hf.RANGE_REMOVE, hf.RANGE_NONE) == (rc.QUERY, rc.REMOVE, rc.NONE)
    assert hf.RANGE_INFO_WORDS == hf.FILE_LEN_INFO_WORDS == rc.INFO_WORDS == 8
    assert len(hf.RANGE_INFO_NAMES) == 8 and len(hf.FILE_LEN_INFO_NAMES) == 8
    assert (hf.FILE_LEN_DYN, hf.FILE_LEN_MAX_OPS) == (rc.DYN, rc.MAX_FILE_OPS)
    assert (hf.DATA_CORRUPTION, hf.META_BUSY, hf.CHUNK_NOT_FOUND, hf.INVALID_ARG) == (2, 3019, 7007, 3)
    text = open(os.path.join(REPO, "include", "hf3fs_crc.h")).read()
    for name, value in (("HF3FS_RANGE_QUERY", 1), ("HF3FS_RANGE_REMOVE", 2), ("HF3FS_RANGE_INFO_UNSORTED", 7),
                        ("HF3FS_RANGE_INFO_OVERFLOW", 6), ("HF3FS_RANGE_INFO_WORDS", 8), ("HF3FS_FILE_LEN_DYN", 1),
                        ("HF3FS_FILE_LEN_MAX_OPS", 1024), ("HF3FS_FILE_LEN_INFO_CORRUPT", 5),
                        ("HF3FS_FILE_LEN_INFO_WORDS", 8)):
        assert re.search(r"\b%s = %d\b" % (name, value), text), name


def test_scratch_bytes(hf):
    sizes = [hf.range_query_scratch_bytes(n, 1) for n in (0, 1, 257, 70001, 1 << 20, 1 << 30)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 16 == 0 for s in sizes)
    # 12 bytes of prefix per record, 12 per op: nothing grows faster
    assert sizes[-1] - sizes[0] == 12 << 30
    assert hf.range_query_scratch_bytes(0, 1 << 30) - hf.range_query_scratch_bytes(0, 0) == 12 << 30
    assert hf.range_query_scratch_bytes((1 << 30) + 1, 1) == 0 and hf.range_query_scratch_bytes(1, (1 << 30) + 1) == 0


A = 0x7F0000001000  # a made-up device address: an argument error is answered before it is touched
BIG = (1 << 30) + 1


@pytest.mark.parametrize("what, kw", [
    ("null info", dict(info=None)),
    ("null table", dict(meta=None)),
    ("null ops", dict(ops=None)),
    ("too many records", dict(n_meta=BIG)),
    ("too many ops", dict(n_ops=BIG)),
    ("null list", dict(lst=None, list_cap=1)),
])
def test_argument_errors_of_range_query(hf, what, kw):
    args = dict(meta=A, n_meta=4, ops=A, n_ops=2, info=A, lst=A, list_cap=8)
    args.update(kw)
    with pytest.raises(hf.Hf3fsCrcError) as e:
        hf.range_query(args["meta"], args["n_meta"], args["ops"], args["n_ops"], args["info"], args["lst"],
                       args["list_cap"], stream=0)
    assert e.value.code == hf.INVALID_ARG, what


@pytest.mark.parametrize("what, kw", [
    ("null info", dict(info=None)),
    ("null ops", dict(ops=None)),
    ("null files", dict(files=None)),
    ("too many ops", dict(n_ops=BIG)),
    ("too many files", dict(n_files=BIG)),
])
def test_argument_errors_of_file_length(hf, what, kw):
    args = dict(ops=A, n_ops=4, files=A, n_files=2, info=A)
    args.update(kw)
    with pytest.raises(hf.Hf3fsCrcError) as e:
        hf.file_length(args["ops"], args["n_ops"], args["files"], args["n_files"], args["info"], stream=0)
    assert e.value.code == hf.INVALID_ARG, what
