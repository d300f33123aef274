"""What tests/test_gpu_stream_queue.py (the HIP library, calls queued back to back on one stream
with one wait at the end) and tests/test_stream_queue_model.py (CPU stand-ins that check the
checkers) share.  Numpy only: no GPU, no torch.

  queued update rounds   tests/update_footprint.py's scenarios with every round resident at once:
                         one payload buffer and one record buffer per round, one chunk arena.  The
                         record buffer of round k carries the state the oracle predicts for the end
                         of round k - 1, so the queue is correct only if every call runs behind
                         the one before it.  check_queue: every round's records and payload arena,
                         and the chunk arena against the image after the last round.
  growth_scenario        rounds that touch the first m chunks only (m differs per round); the
                         records of the other chunks are not sent.
  follow-up records      scrub and read-result records over every chunk's final state: a record
                         batch that runs directly behind the updates must see their bytes.
  chain builders         inputs whose expected values are produced by an earlier call of the same
                         queue: frames with empty header checksums, a block table with an empty
                         checksum column, ranges cut in two halves.
"""
import numpy as np

import batch_cases as bc
import update_footprint as fp

M32 = 0xFFFFFFFF


# ---- queued update rounds ------------------------------------------------------------------------
def round_counts(scn):
    """Records each round sends: the scenario's own counts (growth_scenario) or every chunk."""
    return [getattr(r, "count", scn.n) for r in scn.rounds]


def queue_records(scn, chunk_addr, pay_addrs):
    """The record buffer of every round (inside its guards), round k's payloads at pay_addrs[k]."""
    assert len(pay_addrs) == len(scn.rounds)
    out = []
    for k, m in enumerate(round_counts(scn)):
        buf = scn.record_buffer(k, chunk_addr, pay_addrs[k])
        if m < scn.n:  # the first m records, the guard directly behind them
            buf = np.concatenate([buf[:fp.REC_GUARD + m * fp.REC.itemsize], buf[-fp.REC_GUARD:]])
        out.append(buf)
    return out


def check_queue(scn, got_arena, got_pays, got_recbufs, sent_recbufs):
    """After the whole queue ran: every round's records and payload arena, and the chunk arena
    against the image after the last round (raises AssertionError naming the round and the chunk)."""
    rounds = len(scn.rounds)
    assert len(got_pays) == len(got_recbufs) == len(sent_recbufs) == rounds
    for k, m in enumerate(round_counts(scn)):
        fp.check_records(scn, k, got_recbufs[k], sent_recbufs[k], n=m)
        fp.check_payload(scn, k, got_pays[k])
    fp.check_arena(scn, rounds - 1, got_arena)


GROWTH_COUNTS = (8, 32, 4, 32, 16, 32)
GROWTH_COUNTS_WIDE = (64, 2048, 32, 2048, 512, 2048)   # 4 KiB chunks: the call scratch of 2048 IOs passes 256 KiB


def growth_scenario(orc, counts=GROWTH_COUNTS, max_len=128 << 10, ctype=fp.CRC32C, seed=0xB5, gap=fp.MARGIN):
    """Rounds of counts[k] IOs on the first counts[k] chunks of one arena of max(counts) chunks:
    rounds_scenario's mixed traffic on those, and on every other chunk an EXTEND to length 0,
    which changes neither bytes nor size nor checksum -- so the scenario's images hold whether
    or not that record is sent, and queue_records leaves it out."""
    n = max(counts)
    scn = fp.Scenario(orc, n, max_len, gap=gap, ctype=ctype)
    rng = np.random.default_rng(seed + ctype)
    for m in counts:
        ops = []
        for io in fp._random_ios(rng, n, max_len, scn.sizes, scn.cks, "mixed"):
            if io[0] == "W":
                ops.append(("W", io[1], io[2], int(rng.integers(0, 16)), rng.random() < 0.09))
            else:
                ops.append((io[0], int(io[1])))
        ops[m:] = [("E", 0)] * (n - m)
        before = (list(scn.sizes), list(scn.cks), scn._regions())
        r = scn.add_round(ops, rng)
        r.count = m
        for c in range(m, n):  # the unsent records are no-ops
            assert r.expect[c][0] == fp.OK and scn.sizes[c] == before[0][c] and scn.cks[c] == before[1][c]
            assert np.array_equal(r.regions[c], before[2][c])
    return scn


# ---- follow-up records ---------------------------------------------------------------------------
def final_state(scn):
    """[(size, type, raw value)] of every chunk after the last round; an empty chunk counts as NONE."""
    out = []
    for c in range(scn.n):
        size = scn.sizes[c]
        t, v = (fp.CRC32C, (~scn.fins[c]) & M32) if scn.engine else scn.cks[c]
        out.append((size, t, v) if size and t != fp.NONE else (size, fp.NONE, 0))
    return out


def followup_records(scn, chunk_addr):
    """Scrub and read-result records over every chunk's final state.
    -> dict(scrub=SCRUB_DT array, read=READ_DT array, max_len, computed=the stored raw values (0
    for a NONE record), types).  Every status is expected 0, scrub's `computed` and the read
    result's out_checksum equal `computed`.  Engine chunks persist the finalized value (fin = 1).
    A chunk of size 0 or type NONE gets records that pass unchecked."""
    st = final_state(scn)
    s = np.zeros(scn.n, dtype=bc.SCRUB_DT)
    r = np.zeros(scn.n, dtype=bc.READ_DT)
    want = np.zeros(scn.n, dtype=np.uint32)
    types = np.zeros(scn.n, dtype=np.uint8)
    for c, (size, t, raw) in enumerate(st):
        addr = chunk_addr + scn.lay.bases[c]
        want[c], types[c] = raw, t
        s[c]["data"], s[c]["length"], s[c]["checksum_type"] = addr, size, t
        if t != fp.NONE:
            s[c]["fin"] = 1 if scn.engine else 0
            s[c]["checksum"] = (~raw) & M32 if scn.engine else raw
        s[c]["computed"], s[c]["status"] = bc.SENT32, bc.SENT32
        r[c]["data"], r[c]["offset"], r[c]["length"], r[c]["chunk_len"] = addr, 0, size, size
        r[c]["batch_checksum_type"] = r[c]["chunk_checksum_type"] = t
        r[c]["recalculate"] = 1 if t != fp.NONE else 0
        r[c]["chunk_checksum"] = raw
        r[c]["out_checksum"], r[c]["out_checksum_type"], r[c]["status"] = bc.SENT32, bc.SENT8, bc.SENT32
    return dict(scrub=s, read=r, max_len=scn.max_len, computed=want, types=types)


def check_followup(fu, got_scrub, got_read, got_count):
    """The follow-up batch's results (SCRUB_DT / READ_DT arrays and the scrub's mismatch count)."""
    assert int(got_count) == 0, f"scrub reports {int(got_count)} mismatches behind the updates"
    for c in range(fu["computed"].size):
        g, h, want, t = got_scrub[c], got_read[c], int(fu["computed"][c]), int(fu["types"][c])
        assert int(g["status"]) == 0, f"scrub: chunk {c} status {int(g['status'])}, computed {int(g['computed']):#x}, " \
                                      f"stored {want:#x}"
        assert int(g["computed"]) == want, f"scrub: chunk {c} computed {int(g['computed']):#x}, want {want:#x}"
        assert int(h["status"]) == 0, f"read result: chunk {c} status {int(h['status'])}"
        assert (int(h["out_checksum_type"]), int(h["out_checksum"])) == (t, want), \
            f"read result: chunk {c} ({int(h['out_checksum_type'])}, {int(h['out_checksum']):#x}), want ({t}, {want:#x})"
    for name, got, sent, outs in (("scrub", got_scrub, fu["scrub"], ("computed", "status")),
                                  ("read", got_read, fu["read"], ("out_checksum", "out_checksum_type", "status"))):
        for f in sent.dtype.names:
            if f not in outs:
                assert np.array_equal(got[f], sent[f]), f"{name} record field {f} changed"


# ---- chain builders ------------------------------------------------------------------------------
def frames_chain(rng, n=3000, max_size=20 << 10):
    """n frames of 0..max_size bytes as the framing walk leaves them (8 bytes of header in front of
    each); the header checksum holds only the compressed bit.  `computed` = Checksum::calcSerde of
    every payload: what the first frame_verify_batch computes and the second one must find."""
    sizes = rng.integers(0, max_size + 1, n)
    sizes[:8] = 0, 1, 3, 4, 1023, 1024, 1025, max_size
    f = np.zeros(n, dtype=bc.FRAME_DT)
    off = 8 + np.concatenate([[0], np.cumsum(sizes[:-1] + 8)])
    f["offset"], f["size"] = off, sizes
    f["checksum"] = rng.integers(0, 2, n)
    f["computed"], f["status"] = bc.SENT32, bc.SENT32
    inp = dict(arena=bc._bytes(rng, int(off[-1] + sizes[-1]) + 16), frames=f, max_size=max_size)
    inp["computed"] = bc._frame_truth(inp, f["checksum"] & 1)
    return inp


def _file_table(arena_size, block_lens_per_file, pos0=0):
    blocks, file_off, block_rng, file_rng, pos = [], [0], [], [], pos0
    for lens in block_lens_per_file:
        file_rng.append((pos, int(sum(lens))))
        for ln in lens:
            block_rng.append((pos, int(ln)))
            pos += int(ln)
        file_off.append(file_off[-1] + len(lens))
    assert pos <= arena_size
    b = np.zeros(len(block_rng), dtype=bc.BLOCK_DT)
    b["read_len"] = b["block_len"] = [ln for _, ln in block_rng]
    b["type"] = bc.CRC32C
    return b, np.array(file_off, dtype=np.uint64), np.array(block_rng, dtype=np.uint64).reshape(-1, 2), \
        np.array(file_rng, dtype=np.uint64).reshape(-1, 2)


def digest_chain(rng, kind):
    """Files laid out back to back in one arena, every read full, the block table's checksum column
    zeroed: create_batch over `block_ranges` (offset, length) fills it on the device.
    kind "wave": 200 files of 1..64 blocks of 0..5000 bytes; "split": one file of 4100 blocks of
    64 bytes.  A few blocks are empty (never a file's first).  `file_ranges`: each whole file."""
    if kind == "wave":
        per_file = []
        for f in range(200):
            lens = rng.choice([1, 17, 64, 1000, 4096, 5000], 1 + (f * 37 + 5) % 64)
            lens[1:][rng.random(lens.size - 1) < 0.03] = 0
            per_file.append(lens.tolist())
        assert {len(x) for x in per_file} >= {1, 2, 63, 64}
    else:
        lens = np.full(4100, 64)
        lens[[7, 1024, 2049, 4099]] = 0
        per_file = [lens.tolist()]
    total = sum(sum(x) for x in per_file)
    arena = bc._bytes(rng, total + 5 + 16)
    blocks, file_off, block_rng, file_rng = _file_table(arena.size, per_file, pos0=5)
    assert np.count_nonzero(blocks["block_len"] == 0) >= 3
    return dict(arena=arena, blocks=blocks, file_off=file_off, block_ranges=block_rng, file_ranges=file_rng,
                max_blocks=max(len(x) for x in per_file), max_block_len=int(blocks["block_len"].max()),
                max_file_len=int(file_rng[:, 1].max()))


def halves_chain(rng, n=256):
    """n ranges of 14 B .. 96 KiB, each cut at len // 2 + 7: `first` / `second` are the (offset,
    length) of the halves; combine(create(first), create(second), len(second)) is create(whole)."""
    lens = rng.integers(14, (96 << 10) + 1, n)
    lens[:6] = 14, 15, 16, 17, 1031, 96 << 10
    offs = np.concatenate([[3], 3 + np.cumsum(lens[:-1] + rng.integers(0, 40, n - 1))])
    arena = bc._bytes(rng, int(offs[-1] + lens[-1]) + 16)
    h = lens // 2 + 7
    assert (h <= lens).all()
    return dict(arena=arena, whole=np.stack([offs, lens], 1).astype(np.uint64),
                first=np.stack([offs, h], 1).astype(np.uint64), second=np.stack([offs + h, lens - h], 1).astype(np.uint64),
                max_len=int(lens.max()))
