"""Ordered update batches (hf3fs_crc_update_ordered) and what the reference leaves behind.

A case is a seeded list of IOs in arrival order over a few chunks, chunks repeated.  Its
expectation comes from applying oracle.replica_apply (oracle.engine_apply for chunk-engine IOs)
to host images of the chunks ONE IO AT A TIME in index order -- the serialisation the reference
gets from the chunk lock -- with the call's depth bound on top: an IO with max_rounds or more
earlier IOs on its chunk is not applied.  Nothing here looks at the library.

Used by tests/test_update_ordered_model.py (CPU) and tests/test_gpu_update_ordered.py (GPU).
"""
import numpy as np

import update_footprint as fp

WRITE, TRUNCATE, EXTEND = fp.WRITE, fp.TRUNCATE, fp.EXTEND
OK, INVALID_ARG, CHECKSUM_MISMATCH, NOT_APPLIED = 0, 3, 4080, 9002
NONE, CRC32C = fp.NONE, fp.CRC32C
M32 = fp.M32
GUARD = 4 << 10           # canary before the first and after the last chunk
JUNK = (0x5A5A5A5, 2, 0xDEADBEEF)  # what later IOs of a chunk carry in their three ignored input fields

# The classes of IO the GPU tests assert on; test_update_ordered_model.py checks each has a case.
CLASSES = ("overwrite", "append", "gap", "truncate", "extend", "full", "none_write", "corrupt", "invalid",
           "after_failure", "not_applied", "engine_append", "engine_truncate")


class Built:
    pass


def _layout(n_chunks, max_len, stride):
    return [GUARD + c * stride for c in range(n_chunks)], GUARD + n_chunks * stride + GUARD


def simulate(orc, ios, chunks, state, max_len, max_rounds, ctype, engine):
    """Apply `ios` in order to `chunks` / `state` (both updated).  state[c] = (size, (type, value))
    or, engine, (size, fin, exists).  -> per IO (status, out_size, (out_type, out_value), case,
    (in_size, in_type, in_value)): the last entry is what the IO started from."""
    seen = {}
    out = []
    for io in ios:
        c = io["chunk"]
        k = seen.get(c, 0)
        seen[c] = k + 1
        if engine:
            size, fin, exists = state[c]
            start = (size, CRC32C, (~fin) & M32)
        else:
            size, ck = state[c]
            start = (size, ck[0], ck[1])
        if k >= max_rounds:
            out.append((NOT_APPLIED, start[0], (start[1], start[2]), 0, start))
            continue
        if engine:
            if io["kind"] == "W":
                e = orc.engine_apply(chunks[c], size, fin, io["data"], io["off"], max_len, exists=exists,
                                     data_ck=io["fin"], with_case=True)
            else:
                e = orc.engine_apply(chunks[c], size, fin, b"", io["ln"], max_len, truncate=io["kind"] == "T",
                                     with_case=True)
            assert e[0] == OK, "the engine cases hold no failing IO"
            state[c] = (e[1], e[2], True)
            out.append((OK, e[1], (CRC32C, (~e[2]) & M32), e[3], start))
            continue
        if io["kind"] == "W":
            e = orc.replica_apply(chunks[c], size, ck, WRITE, io["off"], io["ln"], io["data"], io["wck"],
                                  chunk_size=max_len, with_case=True)
        else:
            e = orc.replica_apply(chunks[c], size, ck, TRUNCATE if io["kind"] == "T" else EXTEND, 0, io["ln"],
                                  with_case=True)
        state[c] = (e[1], tuple(e[2]))
        out.append((e[0], e[1], tuple(e[2]), e[3], start))
    return out


def build(orc, name, n_chunks, max_len, max_rounds, ops, seed, stride=None, ctype=CRC32C, engine=False, preset=()):
    """ops: [(chunk, kind, ...)] in arrival order:
         (c, "W", off, ln, flavour)  flavour: "" | "corrupt" | "none" (NONE-typed write)
         (c, "T", target) | (c, "E", target)
    preset: chunks that start with content (seeded bytes of that length)."""
    rng = np.random.default_rng(seed)
    stride = stride or max_len + 256 + 16
    bases, arena_size = _layout(n_chunks, max_len, stride)
    arena = fp.canary(arena_size, fp.SALT_CHUNKS)
    state = []
    for c in range(n_chunks):
        ln = dict(preset).get(c, 0)
        data = rng.integers(0, 256, ln, dtype=np.uint8)
        arena[bases[c]:bases[c] + ln] = data
        if engine:
            state.append((ln, orc.rs_crc32c(data.tobytes()), ln > 0))
        else:
            state.append((ln, tuple(orc.create(ctype, data.tobytes())) if ln else (ctype, 0)))
    state0 = list(state)
    ios, cur = [], GUARD
    rec = np.zeros(len(ops), dtype=fp.REC)
    has_payload = np.zeros(len(ops), dtype=bool)
    placed = []
    first = set()
    for i, op in enumerate(ops):
        c, kind = op[0], op[1]
        u = rec[i]
        u["chunk"] = bases[c]
        u["flags"] = fp.FLAG_ENGINE if engine else 0
        if c not in first:  # the chunk's first IO carries the state; the later ones junk
            first.add(c)
            if engine:
                u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = (
                    state0[c][0], CRC32C, (~state0[c][1]) & M32)
            else:
                u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = (
                    state0[c][0], state0[c][1][0], state0[c][1][1])
        else:
            u["chunk_size"], u["chunk_checksum_type"], u["chunk_checksum"] = JUNK
        if kind in "TE":
            u["update_type"], u["length"] = (TRUNCATE if kind == "T" else EXTEND), op[2]
            ios.append(dict(chunk=c, kind=kind, ln=int(op[2])))
            continue
        off, ln, flavour = int(op[2]), int(op[3]), op[4]
        data = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        p = ((cur + 15) & ~15) + (i * 7) % 16
        cur = p + ln + 64
        placed.append((p, data))
        has_payload[i] = True
        u["update_type"], u["offset"], u["length"], u["payload"] = WRITE, off, ln, p
        io = dict(chunk=c, kind="W", off=off, ln=ln, data=data)
        if engine:
            io["fin"] = orc.rs_crc32c(data)
            u["write_checksum_type"], u["write_checksum"] = CRC32C, (~io["fin"]) & M32
        else:
            wck = tuple(orc.create(ctype, data))
            if flavour == "corrupt":
                wck = (wck[0], wck[1] ^ 0x10)
            if flavour == "none":
                wck = (NONE, 0)
            io["wck"] = wck
            u["write_checksum_type"], u["write_checksum"] = wck
        ios.append(io)
    pay = fp.canary(cur + GUARD, fp.SALT_PAYLOAD)
    for p, data in placed:
        pay[p:p + len(data)] = np.frombuffer(data, dtype=np.uint8)

    b = Built()
    b.name, b.n, b.n_chunks, b.max_len, b.max_rounds = name, len(ops), n_chunks, max_len, max_rounds
    b.ctype, b.engine, b.bases, b.ops = ctype, engine, bases, list(ops)
    b.rec, b.has_payload, b.pay, b.arena0 = rec, has_payload, pay, arena.copy()
    chunks = [bytearray(arena[x:x + max_len].tobytes()) for x in bases]
    b.expect = simulate(orc, ios, chunks, state, max_len, max_rounds, ctype, engine)
    b.arena1 = arena.copy()
    for c, x in enumerate(bases):
        b.arena1[x:x + max_len] = np.frombuffer(bytes(chunks[c]), dtype=np.uint8)
    b.state = list(state)
    depth = {}
    for op in ops:
        depth[op[0]] = depth.get(op[0], 0) + 1
    b.info = (max(depth.values()), sum(1 for e in b.expect if e[0] == NOT_APPLIED))
    # the NOT_APPLIED IOs resubmitted unchanged (as the call returns them): a second batch
    b.again = None
    if b.info[1]:
        idx = [i for i, e in enumerate(b.expect) if e[0] == NOT_APPLIED]
        a = Built()
        a.idx, a.n, a.max_len, a.max_rounds = idx, len(idx), max_len, max_rounds
        chunks2 = [bytearray(ch) for ch in chunks]
        state2 = list(state)
        a.expect = simulate(orc, [ios[i] for i in idx], chunks2, state2, max_len, max_rounds, ctype, engine)
        a.arena1 = arena.copy()
        for c, x in enumerate(bases):
            a.arena1[x:x + max_len] = np.frombuffer(bytes(chunks2[c]), dtype=np.uint8)
        a.state = state2
        a.final_chunks = chunks2
        b.again = a
    b.final_chunks = chunks
    b.classes = classify(b)
    return b


def classify(b):
    """The classes of CLASSES this case holds, from its ops and its expectation."""
    got = set()
    failed_before = set()
    for op, e in zip(b.ops, b.expect):
        c, kind = op[0], op[1]
        size = e[4][0]
        if e[0] == NOT_APPLIED:
            got.add("not_applied")
            continue
        if c in failed_before and e[0] == OK:
            got.add("after_failure")
        if e[0] == CHECKSUM_MISMATCH:
            got.add("corrupt")
            failed_before.add(c)
        elif e[0] == INVALID_ARG:
            got.add("invalid")
            failed_before.add(c)
        if e[0] != OK:
            continue
        if b.engine:
            got.add("engine_append" if kind == "W" else "engine_truncate")
        elif kind == "T" and op[2] < size:
            got.add("truncate")
        elif kind == "E" and op[2] > size:
            got.add("extend")
        elif kind == "W":
            off, ln = op[2], op[3]
            if op[4] == "none":
                got.add("none_write")
            elif off == 0 and ln >= size and size > 0:
                got.add("full")
            elif off == size and size > 0:
                got.add("append")
            elif off > size:
                got.add("gap")
            elif off < size:
                got.add("overwrite")
    return got


def record_array(b, chunk_addr, pay_addr):
    rec = b.rec.copy()
    rec["chunk"] += np.uint64(chunk_addr)
    rec["payload"][b.has_payload] += np.uint64(pay_addr)
    return rec


def expected_records(b, sent, expect=None):
    """The record array the call must leave: `sent` with the output fields and, for every IO,
    the three state input fields it started from."""
    want = sent.copy()
    for i, e in enumerate(expect if expect is not None else b.expect):
        want["status"][i], want["out_size"][i] = e[0], e[1]
        want["out_checksum_type"][i], want["out_checksum"][i] = e[2]
        want["checksum_case"][i] = e[3]
        want["chunk_size"][i], want["chunk_checksum_type"][i], want["chunk_checksum"][i] = e[4]
    return want


# ---- the cases -------------------------------------------------------------------------------------
def _mixed_ops(rng, order, max_len, sizes):
    """One seeded IO per entry of `order` (chunk ids in arrival order), a mix of every replica class;
    `sizes` tracks the chunk sizes as if every IO succeeded (they all do here)."""
    ops = []
    step = {}
    unit = max(8, max_len // 16)
    for c in order:
        k = step.get(c, 0)
        step[c] = k + 1
        s = sizes[c]
        pick = (k + c) % 8 if s else 0
        ln = int(rng.integers(1, unit))
        if pick == 0 or s == 0:          # the first write of an empty chunk / a gap write
            off = int(rng.integers(0, unit // 2)) if s == 0 else min(s + int(rng.integers(1, unit)), max_len - ln - 1)
            off = max(off, 0)
            ops.append((c, "W", off, ln, ""))
            sizes[c] = max(s, off + ln)
        elif pick == 1:                  # append at offset == size
            ln = min(ln, max_len - s) or 1
            if s + ln > max_len or s >= max_len:
                ops.append((c, "T", s // 2))
                sizes[c] = s // 2
            else:
                ops.append((c, "W", s, ln, ""))
                sizes[c] = s + ln
        elif pick == 2:                  # overwrite inside
            off = int(rng.integers(0, s))
            ln = min(ln, max_len - off)
            ops.append((c, "W", off, ln, ""))
            sizes[c] = max(s, off + ln)
        elif pick == 3:                  # truncate shorter (never to 0)
            t = max(1, s - int(rng.integers(1, max(2, s // 2))))
            ops.append((c, "T", t))
            sizes[c] = t
        elif pick == 4:                  # extend
            t = min(max_len, s + int(rng.integers(1, unit)))
            ops.append((c, "E", t))
            sizes[c] = max(s, t)
        elif pick == 5:                  # full overwrite
            ln = min(max_len, s + int(rng.integers(0, unit // 2)))
            ops.append((c, "W", 0, ln, ""))
            sizes[c] = ln
        elif pick == 6:                  # a NONE-typed write (the chunk's type becomes NONE)
            off = int(rng.integers(0, s))
            ln = min(ln, max_len - off)
            ops.append((c, "W", off, ln, "none"))
            sizes[c] = max(s, off + ln)
        else:                            # a typed write over a NONE chunk: recompute in the write's type
            off = int(rng.integers(0, s))
            ln = min(ln, max_len - off)
            ops.append((c, "W", off, ln, ""))
            sizes[c] = max(s, off + ln)
    return ops


def _interleave(rng, depths):
    order = [c for c, d in enumerate(depths) for _ in range(d)]
    rng.shuffle(order)
    return order


def chains(orc, max_len, seed=0xC4A1, depths=(1, 4, 5, 8, 10, 12, 12, 12), max_rounds=12, name="chains"):
    """64 IOs over 8 chunks, 1..12 deep, interleaved; three chunks start with content."""
    rng = np.random.default_rng(seed)
    order = _interleave(rng, depths)
    preset = [(c, max_len // 4 + c) for c in range(len(depths)) if c % 3 == 1]
    sizes = [dict(preset).get(c, 0) for c in range(len(depths))]
    ops = _mixed_ops(rng, order, max_len, sizes)
    return build(orc, f"{name}_{max_len}", len(depths), max_len, max_rounds, ops, seed, preset=preset)


def distinct(orc, max_len, max_rounds, seed=0xD157):
    """64 IOs on 64 chunks: the shape update_batch takes too."""
    rng = np.random.default_rng(seed)
    preset = [(c, 1 + (c * 37) % (max_len // 2)) for c in range(64) if c % 2]
    sizes = [dict(preset).get(c, 0) for c in range(64)]
    ops = []
    for c in range(64):  # every class once per 8 chunks (k = 0: pick = c % 8)
        ops += _mixed_ops(rng, [c], max_len, sizes) if c % 16 != 15 else [(c, "W", max_len, 4, "")]
    return build(orc, f"distinct_{max_len}_r{max_rounds}", 64, max_len, max_rounds, ops, seed, preset=preset)


def failures(orc, max_len, seed=0xFA11):
    """A corrupted client checksum and an INVALID_ARG IO mid-chain, each with successors."""
    q = max_len // 8
    ops = [(0, "W", 0, q, ""), (1, "W", 0, 2 * q, ""), (0, "W", q, q, "corrupt"), (1, "W", max_len, 8, ""),
           (0, "W", q, q // 2, ""), (1, "W", 2 * q, q, ""), (2, "W", 3, q, "corrupt"), (2, "W", 5, q, ""),
           (0, "T", q // 2), (1, "W", max_len - 1, 2, ""), (1, "E", 4 * q), (3, "W", 0, q, ""),
           (2, "W", 5 + q, 7, ""), (3, "W", q // 2, q, "corrupt"), (3, "W", q, 3, ""), (0, "W", q // 2, 9, "")]
    return build(orc, f"failures_{max_len}", 4, max_len, 8, ops, seed)


def overflow(orc, max_len, chains_n=6, seed=0x0F10):
    """Chains of 5 under max_rounds 3: two IOs per chain come back NOT_APPLIED."""
    rng = np.random.default_rng(seed)
    order = _interleave(rng, [5] * chains_n)
    q = max_len // 8
    step, ops = {}, []
    for c in order:
        k = step.get(c, 0)
        step[c] = k + 1
        ops.append([(c, "W", 0, q + c, ""), (c, "W", q + c, q, ""), (c, "W", 3, q // 2, ""),
                    (c, "W", 2 * q + c + 5, q, ""), (c, "T", q)][k])
    return build(orc, f"overflow_{max_len}", chains_n, max_len, 3, ops, seed)


def one_chunk(orc, max_len=128 << 10, seed=0x0C01):
    """64 IOs on one chunk: 32 sequential 2 KiB appends, then 32 overwrites."""
    rng = np.random.default_rng(seed)
    ops = [(0, "W", 2048 * k, 2048, "") for k in range(32)]
    ops += [(0, "W", int(rng.integers(0, 60 << 10)), int(rng.integers(1, 4096)), "") for _ in range(32)]
    return build(orc, "one_chunk", 1, max_len, 64, ops, seed)


def engine(orc, max_len=128 << 10, seed=0xE261):
    """Chunk-engine IOs: per chunk 16 sequential 8 KiB appends and one truncate, interleaved."""
    rng = np.random.default_rng(seed)
    order = _interleave(rng, [17] * 4)
    step, ops = {}, []
    for c in order:
        k = step.get(c, 0)
        step[c] = k + 1
        ops.append((c, "W", 8192 * k, 8192, "") if k < 16 else (c, "T", 100000 + c))
    return build(orc, "engine", 4, max_len, 17, ops, seed, engine=True)


def table_stress(orc, seed=0x7AB1):
    """4096 IOs, 1024 chunks of 512 B at consecutive 512 B addresses, 4 deep, shuffled."""
    rng = np.random.default_rng(seed)
    order = _interleave(rng, [4] * 1024)
    step, ops = {}, []
    for c in order:
        k = step.get(c, 0)
        step[c] = k + 1
        ops.append([(c, "W", 0, 100 + c % 50, ""), (c, "W", 100 + c % 50, 60, ""), (c, "W", 7 + c % 9, 33, ""),
                    (c, "T", 90)][k])
    return build(orc, "table_stress", 1024, 512, 4, ops, seed, stride=512)


def capture_pair(orc, max_len=128 << 10):
    """Two batches of 64 IOs on the same 32 chunks (same arena, record count and payload room),
    grouped differently: 16 chunks x 4, and 1..4 deep over all 32."""
    a = chains(orc, max_len, seed=0xCA01, depths=[4] * 16 + [0] * 16, max_rounds=4, name="capture_a")
    depths_b = [1 + c % 4 for c in range(32)]
    while sum(depths_b) > 64:
        depths_b[depths_b.index(max(depths_b))] -= 1
    b = chains(orc, max_len, seed=0xCA02, depths=depths_b, max_rounds=4, name="capture_b")
    return a, b


def all_cases(orc):
    """name -> builder: every case the GPU tests run (built on demand; the model test builds all)."""
    out = {}
    for ml in (512, 128 << 10):
        out[f"chains_{ml}"] = lambda ml=ml: chains(orc, ml)
        out[f"failures_{ml}"] = lambda ml=ml: failures(orc, ml)
        out[f"overflow_{ml}"] = lambda ml=ml: overflow(orc, ml)
        for r in (1, 4):
            out[f"distinct_{ml}_r{r}"] = lambda ml=ml, r=r: distinct(orc, ml, r)
    out["one_chunk"] = lambda: one_chunk(orc)
    out["engine"] = lambda: engine(orc)
    out["table_stress"] = lambda: table_stress(orc)
    out["capture_a"] = lambda: capture_pair(orc)[0]
    out["capture_b"] = lambda: capture_pair(orc)[1]
    return out
