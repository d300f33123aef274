"""Model and case builders of hf3fs_crc_sync_plan (the resync comparison).

`model` is an independent statement of the comparison loop of ResyncWorker::handleSync
(src/storage/sync/ResyncWorker.cc:199-303) in the reference's own shape: a dict of the local
records, a walk over the remote records in order that erases what it visits, nested ifs, `break`
at a fatal record.  It shares no code with 3fs_amd/csrc/sync_plan.h; the class numbers are written
out here again (tests/test_sync_plan_model.py compares them with the package's and checks the model
against rows classified by hand).
"""
import itertools

import numpy as np

META = np.dtype([("id_hi", "<u8"), ("id_lo", "<u8"), ("chain_ver", "<u4"), ("update_ver", "<u4"),
                 ("commit_ver", "<u4"), ("checksum", "<u4"), ("length", "<u4"), ("chunk_size", "<u4"),
                 ("chunk_state", "u1"), ("recycle_state", "u1"), ("checksum_type", "u1"), ("out_class", "u1"),
                 ("out_peer", "<u4")])
assert META.itemsize == 48

NONE_IDX = 0xFFFFFFFF
COMMIT, DIRTY, CLEAN = 0, 1, 2
(REMOTE_ONLY, LOCAL_RECYCLING, CHAIN_VER_LOW, REMOTE_UNCOMMITTED, REMOTE_CHAIN_VER_HIGH, LOCAL_UNCOMMITTED,
 COMMIT_VER_MISMATCH, CHAIN_WRITING, FULL_SYNC_HEAVY, CHECKSUM_MISMATCH, CHAIN_WRITING_CHECKSUM, EQUAL) = range(1, 13)
MATCHED, REMOTE_MISS, DUPLICATE = 16, 17, 18
FATAL = (REMOTE_CHAIN_VER_HIGH, COMMIT_VER_MISMATCH, CHECKSUM_MISMATCH)
HEAVY = 1
INFO = ("fatal", "first_fatal", "n_write", "n_remove", "recycle", "chain_ver_low", "remote_uncommitted",
        "chain_ver_high", "local_uncommitted", "commit_ver_mismatch", "chain_writing", "full_sync_heavy",
        "full_sync_light", "skip", "remote_miss", "duplicates")
POISON_OUT = 0xA5  # what the builders leave in the output fields: the call must overwrite them


class Plan:
    """What one call must produce."""

    def __init__(self, lclass, lpeer, rclass, rpeer, info, write, remove):
        self.lclass, self.lpeer, self.rclass, self.rpeer = lclass, lpeer, rclass, rpeer
        self.info, self.write, self.remove = info, write, remove


def _walk(local, remote, chain_ver, heavy, stop):
    """The loop of :203-275 over (index, record) tuples.  stop=True breaks at a fatal record as the
    reference does; stop=False walks on (the record is still erased), which gives every remote
    record the class it has on its own.  -> per-remote classes and peers, the counters, both
    lists, the first fatal index, and what is left of the map."""
    metas = {}
    for i in range(local.size):
        metas.setdefault((int(local["id_hi"][i]), int(local["id_lo"][i])), i)  # a map: the first record of an id
    cnt = dict.fromkeys(INFO[4:15], 0)
    write, remove = [], []
    rclass, rpeer = [0] * remote.size, [NONE_IDX] * remote.size
    first_fatal = NONE_IDX
    for r in range(remote.size):
        rm = remote[r]
        key = (int(rm["id_hi"]), int(rm["id_lo"]))
        if key not in metas:
            remove.append(r)
            rclass[r] = REMOTE_ONLY
            continue
        i = metas.pop(key)  # SCOPE_EXIT erase: whatever happens below
        meta = local[i]
        rpeer[r] = i
        if meta["recycle_state"] != 0:
            cnt["recycle"] += 1
            rclass[r] = LOCAL_RECYCLING
            continue
        need_forward, fatal = True, False
        if meta["chain_ver"] > rm["chain_ver"]:
            cnt["chain_ver_low"] += 1
            rclass[r] = CHAIN_VER_LOW
        elif rm["update_ver"] != rm["commit_ver"] or rm["chunk_state"] != COMMIT:
            cnt["remote_uncommitted"] += 1
            rclass[r] = REMOTE_UNCOMMITTED
        elif meta["chain_ver"] < rm["chain_ver"]:
            if meta["chunk_state"] == COMMIT:
                cnt["chain_ver_high"] += 1
                rclass[r] = REMOTE_CHAIN_VER_HIGH
                fatal = True
            else:
                need_forward = False
                cnt["local_uncommitted"] += 1
                rclass[r] = LOCAL_UNCOMMITTED
        elif meta["update_ver"] != rm["commit_ver"]:
            if meta["chain_ver"] != chain_ver and meta["chunk_state"] == COMMIT:
                cnt["commit_ver_mismatch"] += 1
                rclass[r] = COMMIT_VER_MISMATCH
                fatal = True
            else:
                need_forward = False
                cnt["chain_writing"] += 1
                rclass[r] = CHAIN_WRITING
        elif heavy:
            cnt["full_sync_heavy"] += 1
            rclass[r] = FULL_SYNC_HEAVY
        elif (meta["checksum_type"], meta["checksum"]) != (rm["checksum_type"], rm["checksum"]):
            if meta["chain_ver"] != chain_ver:
                cnt["full_sync_light"] += 1
                rclass[r] = CHECKSUM_MISMATCH
                fatal = True
            else:
                need_forward = False
                cnt["chain_writing"] += 1
                rclass[r] = CHAIN_WRITING_CHECKSUM
        else:
            need_forward = False
            rclass[r] = EQUAL
        if fatal:
            if first_fatal == NONE_IDX:
                first_fatal = r
            if stop:
                break
            continue
        if need_forward:
            write.append(i)
        else:
            cnt["skip"] += 1
    return rclass, rpeer, cnt, write, remove, first_fatal, metas


def model(local, remote, chain_ver, flags=0):
    """-> Plan for hf3fs_crc_sync_plan(local, remote, chain_ver, flags)."""
    heavy = bool(flags & HEAVY)
    rclass, rpeer, cnt, write, remove, first_fatal, left = _walk(local, remote, chain_ver, heavy, stop=False)
    lclass, lpeer = [DUPLICATE] * local.size, [NONE_IDX] * local.size
    for r, i in enumerate(rpeer):
        if i != NONE_IDX:
            lclass[i], lpeer[i] = MATCHED, r
    for i in left.values():
        lclass[i] = REMOTE_MISS
    info = dict.fromkeys(INFO, 0)
    info["duplicates"] = lclass.count(DUPLICATE)
    info["first_fatal"] = first_fatal
    if first_fatal != NONE_IDX:  # the reference's variables at the break; no list, no remote miss (:277-287)
        _, _, cnt, _, _, again, _ = _walk(local, remote, chain_ver, heavy, stop=True)
        assert again == first_fatal
        info.update(cnt, fatal=1)
        return Plan(lclass, lpeer, rclass, rpeer, info, [], [])
    for i in left.values():  # :289-292
        write.append(i)
        cnt["remote_miss"] += 1
    info.update(cnt, n_write=len(write), n_remove=len(remove))
    return Plan(lclass, lpeer, rclass, rpeer, info, sorted(write), remove)


def table(n):
    t = np.zeros(n, dtype=META)
    t["out_class"] = POISON_OUT
    t["out_peer"] = 0xA5A5A5A5
    return t


def shuffled(remote, seed):
    return remote[np.random.default_rng(seed).permutation(remote.size)].copy()


LADDER_CHAIN_VER = 7


def ladder_tables(seed=0x51, extra=37):
    """Every combination of the conditions the ladder tests, one chunk each (1944), plus `extra`
    chunks only the remote table has and `extra` only the local one.  -> (local, remote shuffled)."""
    combos = list(itertools.product((-1, 0, 1),      # remote.chain_ver - local.chain_ver
                                    (True, False),   # remote.update_ver == remote.commit_ver
                                    (COMMIT, DIRTY, CLEAN),   # remote state
                                    (COMMIT, DIRTY, CLEAN),   # local state
                                    (True, False),   # local.update_ver == remote.commit_ver
                                    (True, False),   # local.chain_ver == the argument
                                    ("equal", "value", "type"),
                                    (0, 1, 2)))      # local recycle state
    n = len(combos)
    local, remote = table(n + extra), table(n + extra)
    for k, (dcv, r_committed, r_state, l_state, l_at_commit, l_current, ck, recycle) in enumerate(combos):
        lo, re = local[k], remote[k]
        lo["id_hi"] = re["id_hi"] = 0x1000 + k // 100
        lo["id_lo"] = re["id_lo"] = k
        lo["chain_ver"] = LADDER_CHAIN_VER if l_current else LADDER_CHAIN_VER - 2
        re["chain_ver"] = int(lo["chain_ver"]) + dcv
        re["commit_ver"] = 10 + k % 5
        re["update_ver"] = int(re["commit_ver"]) + (0 if r_committed else 1)
        lo["update_ver"] = int(re["commit_ver"]) + (0 if l_at_commit else 1)
        lo["commit_ver"] = lo["update_ver"]
        re["chunk_state"], lo["chunk_state"], lo["recycle_state"] = r_state, l_state, recycle
        lo["checksum_type"], lo["checksum"] = 1, 0xC0FFEE00 + k
        re["checksum_type"] = 2 if ck == "type" else 1
        re["checksum"] = int(lo["checksum"]) ^ (0x10 if ck == "value" else 0)
        lo["length"] = re["length"] = 1 + k
        lo["chunk_size"] = 4096
    for k in range(n, n + extra):
        local[k]["id_hi"], local[k]["id_lo"] = 0xAAAA, k
        local[k]["recycle_state"] = k % 3  # nobody mentions it: forwarded, recycling or not
        remote[k]["id_hi"], remote[k]["id_lo"] = 0xBBBB, k
    return local, shuffled(remote, seed)


def without_fatal(local, remote, chain_ver, flags):
    """The remote table without the records whose class is fatal (the local ones become REMOTE_MISS)."""
    p = model(local, remote, chain_ver, flags)
    keep = np.array([c not in FATAL for c in p.rclass], dtype=bool)
    return remote[keep].copy()


def _ids(kind, idx):
    """128-bit ids of the integers idx in one of the shapes the hash must spread."""
    idx = np.asarray(idx, dtype=np.uint64)
    if kind == "share_lo":
        return idx * np.uint64(0x10001) + np.uint64(3), np.full(idx.size, 0x1234, dtype=np.uint64)
    if kind == "share_hi":
        return np.full(idx.size, 0xFEDCBA9876543210, dtype=np.uint64), idx << np.uint64(20)
    if kind == "small":
        return np.zeros(idx.size, dtype=np.uint64), idx
    assert kind == "mixed"
    return idx * np.uint64(0x9E3779B97F4A7C15), idx ^ (idx << np.uint64(33))


def random_tables(n_local, n_remote, seed, ids="mixed", fatal=False, local_dups=0, remote_triples=0):
    """Random small-valued fields (every rung of the ladder is hit often).  About 3/4 of the remote
    records name a local chunk.  fatal=False repairs every fatal remote record into CHAIN_VER_LOW.
    local_dups: that many local records repeat an earlier local id.  remote_triples: that many
    remote ids appear three times."""
    rng = np.random.default_rng(seed)
    local, remote = table(n_local), table(n_remote)
    chain_ver = 3
    for t in (local, remote):
        n = t.size
        t["chain_ver"] = rng.integers(2, 5, n)
        t["commit_ver"] = rng.integers(1, 3, n)
        t["update_ver"] = np.where(rng.random(n) < 0.8, t["commit_ver"], t["commit_ver"] + 1)
        t["chunk_state"] = rng.choice([COMMIT, COMMIT, COMMIT, DIRTY, CLEAN], n)
        t["checksum_type"] = rng.choice([1, 1, 1, 2], n)
        t["checksum"] = rng.integers(0, 3, n)
        t["length"] = rng.integers(0, 1 << 20, n)
    local["recycle_state"] = rng.choice([0] * 14 + [1, 2], n_local)
    local["chunk_size"] = 1 << 20
    local["id_hi"], local["id_lo"] = _ids(ids, np.arange(n_local))
    for k in range(min(local_dups, max(0, n_local - 1))):
        dst = int(rng.integers(1, n_local))
        src = int(rng.integers(0, dst))
        local["id_hi"][dst], local["id_lo"][dst] = local["id_hi"][src], local["id_lo"][src]
    # remote ids: local ones (distinct while they last) and foreign ones (indices past n_local)
    pick = rng.permutation(n_local)[:min(n_local, (3 * n_remote + 3) // 4)]
    idx = np.concatenate([pick, n_local + np.arange(n_remote - pick.size)])
    remote["id_hi"], remote["id_lo"] = _ids(ids, idx)
    for k in range(min(remote_triples, n_remote // 3)):
        a, b, c = (int(x) for x in rng.choice(n_remote, 3, replace=False))
        for f in ("id_hi", "id_lo"):
            remote[f][b] = remote[f][c] = remote[f][a]
    remote = shuffled(remote, seed + 1)
    if not fatal:
        p = model(local, remote, chain_ver, 0)
        for r, c in enumerate(p.rclass):
            if c in FATAL:
                remote["chain_ver"][r] = 0  # below every local chain_ver: CHAIN_VER_LOW
    return local, remote, chain_ver


LARGE_CHAIN_VER = 5


def large_tables(n_local=1_100_003, n_remote=1_050_001, every=16):
    """A structured pair of tables whose plan is known in closed form (numpy, no per-record loop).
    Remote record j is local record perm[j] (a fixed permutation), except for j % every ==
      0: its id is replaced by one no local record has          -> REMOTE_ONLY, the local one REMOTE_MISS
      1: its chain_ver is lowered                                -> CHAIN_VER_LOW (forward)
      2: its update_ver is ahead of its commit_ver               -> REMOTE_UNCOMMITTED (forward)
      3: its checksum differs, local.chain_ver == the argument   -> CHAIN_WRITING_CHECKSUM (skip)
    Local records perm[n_remote:] are mentioned by nobody        -> REMOTE_MISS.
    -> (local, remote, Plan with numpy arrays)."""
    i = np.arange(n_local, dtype=np.uint64)
    local = table(n_local)
    local["id_hi"], local["id_lo"] = _ids("mixed", i)
    local["chain_ver"] = LARGE_CHAIN_VER
    local["update_ver"] = local["commit_ver"] = (i % np.uint64(7)).astype(np.uint32) + 1
    local["checksum"] = (i * np.uint64(2654435761)).astype(np.uint32)
    local["checksum_type"] = 1
    local["length"] = local["chunk_size"] = 4 << 20
    perm = ((i * np.uint64(700_001) + np.uint64(12345)) % np.uint64(n_local)).astype(np.int64)
    assert np.unique(perm).size == n_local
    src = perm[:n_remote]
    remote = local[src].copy()
    remote["chunk_size"] = 0
    j = np.arange(n_remote)
    cat = j % every
    remote["id_hi"][cat == 0] ^= np.uint64(1) << np.uint64(63)
    remote["id_lo"][cat == 0] += np.uint64(1)
    remote["chain_ver"][cat == 1] -= 1
    remote["update_ver"][cat == 2] += 1
    remote["checksum"][cat == 3] ^= 0x8000
    rclass = np.full(n_remote, EQUAL, dtype=np.uint8)
    for c, cls in ((0, REMOTE_ONLY), (1, CHAIN_VER_LOW), (2, REMOTE_UNCOMMITTED), (3, CHAIN_WRITING_CHECKSUM)):
        rclass[cat == c] = cls
    rpeer = np.where(cat == 0, NONE_IDX, src).astype(np.uint32)
    lclass = np.full(n_local, REMOTE_MISS, dtype=np.uint8)
    lpeer = np.full(n_local, NONE_IDX, dtype=np.uint32)
    hit = cat != 0
    lclass[src[hit]] = MATCHED
    lpeer[src[hit]] = j[hit]
    forward = np.zeros(n_local, dtype=bool)
    forward[src[(cat == 1) | (cat == 2)]] = True
    write = np.flatnonzero(forward | (lclass == REMOTE_MISS)).astype(np.uint32)
    remove = np.flatnonzero(cat == 0).astype(np.uint32)
    info = dict.fromkeys(INFO, 0)
    info.update(first_fatal=NONE_IDX, n_write=int(write.size), n_remove=int(remove.size),
                chain_ver_low=int((cat == 1).sum()), remote_uncommitted=int((cat == 2).sum()),
                chain_writing=int((cat == 3).sum()), skip=int((cat >= 3).sum()),
                remote_miss=int((lclass == REMOTE_MISS).sum()))
    return local, remote, Plan(lclass, lpeer, rclass, rpeer, info, write, remove)
