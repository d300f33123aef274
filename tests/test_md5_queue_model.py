"""tests/md5_queue.py without a GPU: the share and grid geometry that the counts of
tests/test_gpu_md5_queue.py are chosen for, the bucket spread of its `spread` files, the builders
against the plain reading of their files, and the checkers themselves -- a stand-in library made of
hashlib and md5_cases.State passes every run, and a stand-in wrong in one named way fails the run
that is there to catch it, with a message that names a file index."""
import hashlib
import os
import re

import numpy as np
import pytest

import md5_cases as mc
import md5_queue as mq

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3fs_amd", "csrc")
BIG = (1 << 20) + 300


# ---- geometry ---------------------------------------------------------------------------------------
def test_constants_are_the_sources():
    """shares_of and grid_of of md5_queue.py restate md5_kernels.hip: the numbers they use are there."""
    hip, head = open(os.path.join(CSRC, "md5_kernels.hip")).read(), open(os.path.join(CSRC, "md5_kernels.h")).read()
    assert re.search(r"kMd5SharesMax = (\d+);", head).group(1) == str(mq.SHARES_MAX)
    assert "const uint64_t tiles = (n + 63) / 64;" in hip and mq.TILE == 64
    assert "s.per = (tiles + s.shares - 1) / s.shares * 64;" in hip
    assert "const uint64_t want = (n + 255) / 256;" in hip and mq.PREP_THREADS == 256
    assert "want < 4096 ? (want ? want : 1) : 4096" in hip and mq.PREP_BLOCKS_MAX == 4096
    assert re.search(r"kMd5Buckets = (\d+);", open(os.path.join(CSRC, "md5_core.h")).read()).group(1) == str(mq.BUCKETS)


def test_counts_reach_the_multi_tile_shares_and_the_grid_stride_loop():
    g = {n: mq.geometry(n) for n in mq.COUNTS}
    assert mq.COUNTS == (16384, 16385, 32769, 70001, BIG)
    assert g[16384] == dict(shares=256, tiles_per_share=1, empty=0, partial=[], partial_behind_full=[], prep_grid=64,
                            prep_strides=False)  # the last count at which no share carries anything over
    assert (g[16385]["shares"], g[16385]["tiles_per_share"], g[16385]["empty"], g[16385]["partial"]) == (256, 2, 127, [128])
    assert (g[32769]["shares"], g[32769]["tiles_per_share"], g[32769]["empty"], g[32769]["partial"]) == (256, 3, 85, [170])
    assert (g[70001]["shares"], g[70001]["tiles_per_share"], g[70001]["empty"]) == (256, 5, 37)
    assert g[70001]["partial"] == g[70001]["partial_behind_full"] == [218]  # 3 full tiles, then one of 49 files
    assert 70001 - 218 * 320 == 3 * 64 + 49
    assert (g[BIG]["shares"], g[BIG]["tiles_per_share"], g[BIG]["empty"], g[BIG]["partial_behind_full"]) == (256, 65, 3, [252])
    assert g[BIG]["prep_grid"] == 4096 and g[BIG]["prep_strides"] and BIG > 4096 * 256
    assert not any(g[n]["prep_strides"] for n in mq.COUNTS[:-1])
    assert mq.TWO_CALL_COUNT == 70001 and mq.SPREAD_COUNTS == (16385, 70001)


def test_md5_bucket_table():
    """md5_bucket of md5_core.h read by hand: at = 4 floor(log2 blocks) + the next two bits, bucket
    254 - at, 255 for no block; md5_call_blocks likewise."""
    table = {0: 255, 1: 254, 2: 250, 3: 248, 4: 246, 5: 245, 6: 244, 7: 243, 8: 242, 9: 242, 10: 241, 15: 239, 16: 238,
             260: 222, 1 << 20: 174, (1 << 20) + 3 * (1 << 18): 171, (1 << 58) + 1: 22, 1 << 63: 2, (1 << 64) - 1: 0}
    assert {b: mq.md5_bucket(b) for b in table} == table
    assert [mq.call_blocks(0, n, True) for n in (0, 55, 56, 63, 64, 119, 120)] == [1, 1, 2, 2, 2, 2, 3]
    assert [mq.call_blocks(t, n, False) for t, n in ((0, 0), (63, 0), (63, 1), (1, 127))] == [0, 0, 1, 2]


def test_spread_occupies_many_buckets_in_many_shares():
    """A2's bounds: at least 40 distinct buckets, at least 100 of the 256 shares with 8 or more.
    Holes of 0..16 KiB alone end at 260 blocks, fewer than 40 buckets: hence the ladder of longer ones."""
    assert len({mq.md5_bucket(b) for b in range(1, 261)}) < 40
    got = {n: mq.spread_occupancy(mq.spread(n)) for n in mq.SPREAD_COUNTS}
    for n, (buckets, wide) in got.items():
        assert buckets >= 40 and wide >= 100, got
    assert got == {16385: (51, 128), 70001: (52, 219)}  # as measured; a change of the builder shows here
    b = mq.spread(70001)
    assert int(b.lengths[70001 // 3]) >= mq.LONG_HOLE and b.arena.size <= 16 << 20
    assert int(b.lengths.sum()) < 250 << 20  # what hashlib sees


# ---- the builders -----------------------------------------------------------------------------------------
def _by_hand(batch, f):
    lo, hi = int(batch.file_off[f]), int(batch.file_off[f + 1])
    return b"".join(bytes(int(batch.seg_len[k])) if batch.seg_at[k] < 0
                    else batch.arena[int(batch.seg_at[k]):int(batch.seg_at[k]) + int(batch.seg_len[k])].tobytes()
                    for k in range(lo, hi))


def test_builders_describe_their_files():
    t = mq.tiny(16385)
    per = np.diff(t.file_off.astype(np.int64))
    assert t.n == 16385 and set(per.tolist()) == {0, 1} and (per[11::16] == 0).all() and (t.lengths[5::16] == 0).all()
    assert set(t.lengths.tolist()) == set(range(131)) and set((t.seg_at % 16).tolist()) == set(range(16))
    s = mq.spread(16385)
    per = np.diff(s.file_off.astype(np.int64))
    assert (per[7::16] == 1).all() and (per[np.arange(s.n) % 16 != 7] == 2).all()
    first = s.seg_at[s.file_off[:-1].astype(np.int64)]
    assert (first[3::8] >= 0).all() and (first[np.arange(s.n) % 8 != 3] < 0).all()
    real = s.seg_len[s.seg_at >= 0]
    assert real.min() == 1 and real.max() == 200 and (s.seg_len[s.seg_at < 0] == 0).any()
    h = mq.head(16385)
    assert h.arena is s.arena and h.lengths.max() == 63 and (np.diff(h.file_off.astype(np.int64))[2::16] == 0).all()
    for b in (t, s, h, mq.four_calls(130).calls[1]):
        got = b.contents()
        for f in list(range(0, b.n, max(1, b.n // 97))) + [b.n - 1]:
            assert got[f] == _by_hand(b, f) and len(got[f]) == b.lengths[f], f
        assert b.digests[:16] == hashlib.md5(got[0]).digest() and len(b.digests) == 16 * b.n
        segs, off = b.records(0x1000)
        assert segs.dtype == mc.SEG and off.dtype == np.uint64 and ((segs["data"] == 0) == (b.seg_at < 0)).all()


def test_head_states_are_the_models():
    h = mq.head(700)
    assert mq.head_states(h) == b"".join(mc.State().update(c).pack() for c in h.contents())


def test_four_calls_and_a_moved_boundary():
    loop = mq.four_calls(130)
    assert len(loop.calls) == 4 and loop.n == 48 and loop.states != loop.calls[0].n * mc.State().pack()
    arena2 = np.random.default_rng(5).integers(0, 256, loop.arena.size, dtype=np.uint8)
    moved, f, off = mq.moved_boundary(loop, arena2)
    assert off[f + 1] == loop.calls[1].file_off[f + 1] - 1 and (np.delete(off, f + 1) == np.delete(loop.calls[1].file_off, f + 1)).all()
    assert moved.lengths[f] < loop.lengths[f] and moved.lengths[f + 1] > loop.lengths[f + 1]
    assert moved.digests[16 * f:16 * f + 16] == hashlib.md5(moved.messages[f]).digest() != loop.digests[:16]


def test_seeds_and_the_wrap_of_total():
    """The long-hole seeds finalise to hashlib's digests of that many zeros through the model (the
    core gave {h, total}: tests/test_md5_sanitized.py), and a total that passes 2^64 keeps
    total % 64 and the bit length total * 8 mod 2^64, which is all MD5_Update's Nl / Nh keep."""
    case = mq.seeded()
    assert case.n == 13 * mq.SEED_COPIES and sum(k is not None for k in case.known) == 4 * mq.SEED_COPIES
    assert [s.total for s in case.seeds[::mq.SEED_COPIES]][:9] == mq.SEED_TOTALS
    for n, (h, digest) in mq.LONG_HOLES.items():
        assert mc.State(h, n, bytes(n % 64)).digest().hex() == digest
    assert set(case.update.lengths[0::mq.SEED_COPIES].tolist()) == {0} and set(case.update.lengths[1::mq.SEED_COPIES].tolist()) == {200}
    s = mc.State((1, 2, 3, 4), mq.M64 - 64 + 9, bytes(9)).update(bytes(200))
    assert s.total == mq.M64 + 145 and len(s.tail) == 145 % 64
    wrapped = mc.State.unpack(mq.pack_state(s))
    assert wrapped.total == 145 and wrapped.tail == s.tail and wrapped.digest() == s.digest()


# ---- the checkers -----------------------------------------------------------------------------------------
def test_checkers_name_files_and_lengths():
    want = bytes(range(48))
    mq.check_digests(want, want, [1, 2, 3], "same")
    with pytest.raises(AssertionError, match=r"x: 1 of 3 digests differ \(0 of them never written\), first files \[1\] \(lengths \[20\]\)"):
        mq.check_digests(want[:31] + b"\xff" + want[32:], want, [10, 20, 30], "x")
    with pytest.raises(AssertionError, match=r"1 of them never written\), first files \[2\]"):
        mq.check_digests(want[:32] + bytes([mq.SENTINEL]) * 16, want, [10, 20, 30], "x")
    a, b = mc.State().update(b"abc"), mc.State().update(b"abd")
    with pytest.raises(AssertionError, match=r"first files \[1\] \(lengths \[3\]\); file 1 differs in tail"):
        mq.check_states(a.pack() + b.pack(), a.pack() * 2, [3, 3], "y")
    be = mq.StandIn()
    buf = mq.guarded(be, 32)
    assert mq.unguard(be, buf, 32, "z") == bytes([mq.SENTINEL]) * 32
    buf.a[mq.GUARD + 32] = 0
    with pytest.raises(AssertionError, match="guard"):
        mq.unguard(be, buf, 32, "z")


RUNS = {
    "A1 at 3,000": lambda be: mq.run_one_shot(be, mq.tiny(3000), "tiny"),
    "A1 at 16,385": lambda be: mq.run_one_shot(be, mq.tiny(16385), "tiny"),
    "A1 at 1,048,876": lambda be: mq.run_one_shot(be, mq.tiny(BIG), "tiny"),
    "A2": lambda be: mq.run_one_shot(be, mq.spread(2000), "spread"),
    "A3": lambda be: mq.run_two_calls(be, mq.head(2000), mq.spread(2000), mq.two_call_digests(2000), "two calls"),
    "B1 of 130": lambda be: mq.run_loop(be, mq.four_calls(130), "loop"),
    "B1": lambda be: mq.run_loop(be, mq.four_calls(4097), "loop"),
    "B1 twin": lambda be: mq.run_loop(be, mq.four_calls(130), "loop", wait_each=True),
    "E2": lambda be: mq.run_seeded(be, mq.seeded(), "seeded"),
}


def test_right_stand_in_passes_every_run():
    """hashlib and State behind the same record arrays, at reduced counts (and at 16,385, which costs nothing)."""
    for name, run in RUNS.items():
        if name != "A1 at 1,048,876":
            run(mq.StandIn())
    assert RUNS["B1 of 130"](mq.StandIn()) == RUNS["B1 twin"](mq.StandIn())
    loop = mq.four_calls(130)
    moved, f, off = mq.moved_boundary(loop, np.random.default_rng(5).integers(0, 256, loop.arena.size, dtype=np.uint8))
    mq.run_loop(mq.StandIn(), moved, "moved boundary")


WRONG = [
    ("second_tile_skipped", "A1 at 16,385", r"8192 of 16385 digests differ \(8192 of them never written\), first files \[64, 65,"),
    ("place_doubled", "A1 at 16,385", r"1 of 16385 digests differ \(1 of them never written\), first files \[8192\]"),
    ("place_doubled", "A3", r"states after INIT and FINAL: 1 of 2000 states differ, first files \[1000\]"),
    ("offsets_stop_at_2^20", "A1 at 1,048,876", r"300 of 1048876 digests differ \(300 of them never written\), first files \[1048576,"),
    ("state_of_two_calls_earlier", "B1", r"48 of 48 digests differ \(0 of them never written\), first files \[0,"),
    ("total_32_bits", "E2", r"FINAL alone .* digests differ \(0 of them never written\), first files \[48,"),
    ("final_writes_state", "A3", r"states after INIT and FINAL: \d+ of 2000 states differ, first files \[0, 1,"),
]


@pytest.mark.parametrize("fault,run,message", WRONG, ids=[f"{f}-{r.replace(' ', '_')}" for f, r, _ in WRONG])
def test_wrong_stand_in_fails_its_run(fault, run, message):
    with pytest.raises(AssertionError, match=message):
        RUNS[run](mq.StandIn(fault))


def test_wrong_stand_ins_that_a_smaller_run_cannot_see():
    """Why the counts are what they are: below 16,385 files no share has a second tile, and below
    2^20 no offset lies past the loop's end."""
    RUNS["A1 at 3,000"](mq.StandIn("second_tile_skipped"))
    RUNS["A1 at 16,385"](mq.StandIn("offsets_stop_at_2^20"))
    RUNS["A3"](mq.StandIn("total_32_bits"))
