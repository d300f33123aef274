"""hf3fs_crc_sync_plan without a device: the Python model of tests/sync_cases.py against rows
classified by hand from the ladder (ResyncWorker.cc:203-275), the break, the SyncMeta layout and
the error returns that are decided before any device is touched."""
import ctypes
import importlib

import numpy as np
import pytest

import sync_cases as sc

CV = 7  # the call's chain_ver


def _rec(id_, cv=CV, uv=1, cmv=1, state=sc.COMMIT, ck=(1, 0xAB), recycle=0):
    t = sc.table(1)
    t["id_hi"], t["id_lo"] = 0x77, id_
    t["chain_ver"], t["update_ver"], t["commit_ver"] = cv, uv, cmv
    t["chunk_state"], t["recycle_state"] = state, recycle
    t["checksum_type"], t["checksum"] = ck
    return t


# (name, local or None, remote, flags, expected class): each worked out by hand from the ladder
HAND = [
    ("no local record", None, _rec(1), 0, sc.REMOTE_ONLY),
    ("local recycling wins over everything", _rec(2, cv=9, recycle=2), _rec(2, cv=1, uv=5), 0, sc.LOCAL_RECYCLING),
    ("local chain_ver 8 > remote 7", _rec(3, cv=8), _rec(3, cv=7), 0, sc.CHAIN_VER_LOW),
    ("chain_ver low wins over remote uncommitted", _rec(4, cv=8), _rec(4, cv=7, uv=2), 0, sc.CHAIN_VER_LOW),
    ("remote update_ver 2 != commit_ver 1", _rec(5), _rec(5, uv=2), 0, sc.REMOTE_UNCOMMITTED),
    ("remote DIRTY", _rec(6), _rec(6, state=sc.DIRTY), 0, sc.REMOTE_UNCOMMITTED),
    ("remote uncommitted wins over remote chain_ver high", _rec(7, cv=6), _rec(7, cv=7, state=sc.CLEAN), 0,
     sc.REMOTE_UNCOMMITTED),
    ("local 6 < remote 7, local COMMIT", _rec(8, cv=6), _rec(8, cv=7), 0, sc.REMOTE_CHAIN_VER_HIGH),
    ("local 6 < remote 7, local DIRTY", _rec(9, cv=6, state=sc.DIRTY), _rec(9, cv=7), 0, sc.LOCAL_UNCOMMITTED),
    ("update_ver 3 != remote commit_ver 1, local chain_ver 5 != 7, COMMIT", _rec(10, cv=5, uv=3),
     _rec(10, cv=5), 0, sc.COMMIT_VER_MISMATCH),
    ("the same with local chain_ver == 7", _rec(11, uv=3), _rec(11), 0, sc.CHAIN_WRITING),
    ("the same with local chain_ver 5 but CLEAN", _rec(12, cv=5, uv=3, state=sc.CLEAN), _rec(12, cv=5), 0,
     sc.CHAIN_WRITING),
    ("versions agree, heavy: forwarded whatever the checksum", _rec(13, ck=(1, 1)), _rec(13, ck=(1, 2)), sc.HEAVY,
     sc.FULL_SYNC_HEAVY),
    ("commit version mismatch wins over heavy", _rec(14, cv=5, uv=3), _rec(14, cv=5), sc.HEAVY,
     sc.COMMIT_VER_MISMATCH),
    ("value differs, local chain_ver 5 != 7", _rec(15, cv=5, ck=(1, 1)), _rec(15, cv=5, ck=(1, 2)), 0,
     sc.CHECKSUM_MISMATCH),
    ("type differs with equal value, local chain_ver 5 != 7", _rec(16, cv=5, ck=(1, 9)), _rec(16, cv=5, ck=(2, 9)),
     0, sc.CHECKSUM_MISMATCH),
    ("value differs, local chain_ver == 7", _rec(17, ck=(1, 1)), _rec(17, ck=(1, 2)), 0, sc.CHAIN_WRITING_CHECKSUM),
    ("everything agrees", _rec(18, uv=4, cmv=4), _rec(18, uv=4, cmv=4), 0, sc.EQUAL),
    ("local not COMMIT does not matter when all agrees", _rec(19, state=sc.DIRTY), _rec(19), 0, sc.EQUAL),
]


@pytest.mark.parametrize("name,local,remote,flags,want", HAND, ids=[h[0] for h in HAND])
def test_model_matches_hand_classified_row(name, local, remote, flags, want):
    p = sc.model(local if local is not None else sc.table(0), remote, CV, flags)
    assert p.rclass == [want]
    assert p.rpeer == [sc.NONE_IDX if local is None else 0]
    if local is not None:
        assert (p.lclass, p.lpeer) == ([sc.MATCHED], [0])


def test_hand_rows_cover_every_remote_class():
    assert {h[4] for h in HAND} == set(range(1, 13))


def test_model_lists_counters_and_local_classes():
    """Seven chunks by hand: forward, skip, remove, miss, a repeated remote id, a repeated local id."""
    local = np.concatenate([_rec(1, cv=8),          # 0: CHAIN_VER_LOW -> forward
                            _rec(2),                # 1: EQUAL -> skip
                            _rec(3, recycle=1),     # 2: recycling, matched: nothing
                            _rec(4, recycle=1),     # 3: recycling, nobody mentions it: forward
                            _rec(2, cv=1),          # 4: duplicate of 1: ignored
                            _rec(5)])               # 5: matched by remote 1 only (remote 4 repeats the id)
    remote = np.concatenate([_rec(3), _rec(5, uv=2), _rec(9), _rec(1, cv=7), _rec(5), _rec(2)])
    p = sc.model(local, remote, CV)
    assert p.rclass == [sc.LOCAL_RECYCLING, sc.REMOTE_UNCOMMITTED, sc.REMOTE_ONLY, sc.CHAIN_VER_LOW, sc.REMOTE_ONLY,
                        sc.EQUAL]
    assert p.rpeer == [2, 5, sc.NONE_IDX, 0, sc.NONE_IDX, 1]
    assert p.lclass == [sc.MATCHED, sc.MATCHED, sc.MATCHED, sc.REMOTE_MISS, sc.DUPLICATE, sc.MATCHED]
    assert p.lpeer == [3, 5, 0, sc.NONE_IDX, sc.NONE_IDX, 1]
    assert p.write == [0, 3, 5] and p.remove == [2, 4]
    assert p.info == dict(fatal=0, first_fatal=sc.NONE_IDX, n_write=3, n_remove=2, recycle=1, chain_ver_low=1,
                          remote_uncommitted=1, chain_ver_high=0, local_uncommitted=0, commit_ver_mismatch=0,
                          chain_writing=0, full_sync_heavy=0, full_sync_light=0, skip=1, remote_miss=1, duplicates=1)


def test_model_break_at_the_first_of_two_fatal_rows():
    """remote: forward, skip, FATAL (2), recycling, forward, FATAL (5), remove.  The counters are the
    reference's at the break: rows 0-2 only; no list, no remote miss.  Classes are whole-table."""
    local = np.concatenate([_rec(1, cv=8), _rec(2), _rec(3, cv=6), _rec(4, recycle=2), _rec(5, cv=8),
                            _rec(6, cv=5, ck=(1, 1)), _rec(7)])
    remote = np.concatenate([_rec(1), _rec(2), _rec(3), _rec(4), _rec(5), _rec(6, cv=5, ck=(1, 2)), _rec(8)])
    p = sc.model(local, remote, CV)
    assert p.rclass == [sc.CHAIN_VER_LOW, sc.EQUAL, sc.REMOTE_CHAIN_VER_HIGH, sc.LOCAL_RECYCLING, sc.CHAIN_VER_LOW,
                        sc.CHECKSUM_MISMATCH, sc.REMOTE_ONLY]
    assert p.lclass == [sc.MATCHED] * 6 + [sc.REMOTE_MISS]
    assert p.write == [] and p.remove == []
    assert p.info == dict(fatal=1, first_fatal=2, n_write=0, n_remove=0, recycle=0, chain_ver_low=1,
                          remote_uncommitted=0, chain_ver_high=1, local_uncommitted=0, commit_ver_mismatch=0,
                          chain_writing=0, full_sync_heavy=0, full_sync_light=0, skip=1, remote_miss=0, duplicates=0)


def test_ladder_table_reaches_every_class():
    local, remote = sc.ladder_tables()
    assert local.size == remote.size == 1944 + 37
    for flags in (0, sc.HEAVY):
        p = sc.model(local, remote, sc.LADDER_CHAIN_VER, flags)
        want = set(range(1, 13)) - ({sc.CHECKSUM_MISMATCH, sc.CHAIN_WRITING_CHECKSUM, sc.EQUAL} if flags
                                    else {sc.FULL_SYNC_HEAVY})
        assert set(p.rclass) == want
        assert p.info["fatal"] == 1
        calm = sc.without_fatal(local, remote, sc.LADDER_CHAIN_VER, flags)
        q = sc.model(local, calm, sc.LADDER_CHAIN_VER, flags)
        assert q.info["fatal"] == 0 and q.info["n_write"] == len(q.write) > 37 and q.info["n_remove"] == 37


def test_large_pattern_agrees_with_the_model_at_a_small_size():
    """The closed-form expectation of the 1.1 M case, checked by the per-record model at 5003 records."""
    local, remote, want = sc.large_tables(5003, 4801)
    p = sc.model(local, remote, sc.LARGE_CHAIN_VER)
    assert p.rclass == want.rclass.tolist() and p.rpeer == want.rpeer.tolist()
    assert p.lclass == want.lclass.tolist() and p.lpeer == want.lpeer.tolist()
    assert p.write == want.write.tolist() and p.remove == want.remove.tolist()
    assert p.info == want.info


# ---- the binding ---------------------------------------------------------------------------------
def test_syncmeta_layout(hf):
    M = hf.SyncMeta
    assert ctypes.sizeof(M) == 48 == sc.META.itemsize
    offsets = dict(id_hi=0, id_lo=8, chain_ver=16, update_ver=20, commit_ver=24, checksum=28, length=32,
                   chunk_size=36, chunk_state=40, recycle_state=41, checksum_type=42, out_class=43, out_peer=44)
    assert {name: getattr(M, name).offset for name, _ in M._fields_} == offsets
    assert {name: sc.META.fields[name][1] for name in sc.META.names} == offsets


def test_class_constants_are_distinct_and_match_the_header(hf):
    names = ["REMOTE_ONLY", "LOCAL_RECYCLING", "CHAIN_VER_LOW", "REMOTE_UNCOMMITTED", "REMOTE_CHAIN_VER_HIGH",
             "LOCAL_UNCOMMITTED", "COMMIT_VER_MISMATCH", "CHAIN_WRITING", "FULL_SYNC_HEAVY", "CHECKSUM_MISMATCH",
             "CHAIN_WRITING_CHECKSUM", "EQUAL", "MATCHED", "REMOTE_MISS", "DUPLICATE"]
    values = [getattr(hf, "SYNC_" + n) for n in names]
    assert len(set(values)) == len(values) and 0 not in values
    assert values == [getattr(sc, n) for n in names]
    import re
    text = open(hf._lib.HEADER).read()
    for n, v in zip(names, values):
        assert re.search(rf"\bHF3FS_SYNC_{n} = {v}\b", text), n
    for w, n in enumerate(hf.SYNC_INFO_NAMES):
        assert re.search(rf"\bHF3FS_SYNC_INFO_\w+ = {w}\b", text), n
    assert hf.SYNC_INFO_NAMES == sc.INFO and hf.SYNC_INFO_WORDS == len(sc.INFO) == 16
    assert re.search(r"\bHF3FS_SYNC_INFO_WORDS = 16\b", text)


def test_errors_decided_without_a_device(hf):
    """Every argument error is returned before any device is touched: none of these calls needs one."""
    L = hf._lib
    ok_ptr = 0x1000  # never dereferenced: the call fails first
    cases = [
        dict(local=ok_ptr, n_local=1, remote=ok_ptr, n_remote=1, info=None),          # null d_info
        dict(local=None, n_local=1, remote=ok_ptr, n_remote=1, info=ok_ptr),          # null table, count > 0
        dict(local=ok_ptr, n_local=1, remote=None, n_remote=2, info=ok_ptr),
        dict(local=ok_ptr, n_local=1, remote=ok_ptr, n_remote=1, info=ok_ptr, flags=2),  # unknown flag bits
        dict(local=ok_ptr, n_local=1, remote=ok_ptr, n_remote=1, info=ok_ptr, flags=0x80000001),
        dict(local=ok_ptr, n_local=(1 << 30) + 1, remote=ok_ptr, n_remote=1, info=ok_ptr),
        dict(local=ok_ptr, n_local=1, remote=ok_ptr, n_remote=(1 << 30) + 1, info=ok_ptr),
    ]
    for kw in cases:
        with pytest.raises(hf.Hf3fsCrcError) as e:
            L.sync_plan(kw["local"], kw["n_local"], kw["remote"], kw["n_remote"], 1, kw["info"],
                        flags=kw.get("flags", 0))
        assert e.value.code == hf.INVALID_ARG, kw
    assert L.sync_plan_scratch_bytes((1 << 30) + 1, 1) == 0 == L.sync_plan_scratch_bytes(1, (1 << 30) + 1)
    small, big = L.sync_plan_scratch_bytes(100, 100), L.sync_plan_scratch_bytes(1 << 20, 1 << 20)
    assert 0 < small < big and big >= (2 << 20) * 4 + (1 << 20) * 10
    for kw in (dict(local=None), dict(addrs=None), dict(write=None), dict(info=None), dict(scrub=None)):
        a = dict(local=ok_ptr, addrs=ok_ptr, write=ok_ptr, info=ok_ptr, scrub=ok_ptr)
        a.update(kw)
        with pytest.raises(hf.Hf3fsCrcError) as e:
            L.sync_scrub_fill(a["local"], a["addrs"], a["write"], a["info"], 4, a["scrub"])
        assert e.value.code == hf.INVALID_ARG, kw
    assert L.sync_scrub_fill(None, None, None, None, 0, None) == hf.OK
