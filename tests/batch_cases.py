"""Batch entry points as small cases, shared by tests/test_gpu_batch_contexts.py (the HIP library,
each case eager under every switch, on poisoned scratch, and captured into a graph and replayed
over rewritten inputs) and tests/test_batch_cases_model.py (the helper checked on the CPU).

A case is one entry point of include/hf3fs_crc.h at the smallest shape that still reaches the code
it is meant to reach:

  build(cus, rng, scale)   host inputs (numpy only; device addresses are arena-relative until
                           `buffers` adds the arena's device address).  Counts derive from the
                           device's CU count, W = 16 * cus waves.  scale = 2: twice the records.
  reference(inp)           the expected outputs, computed with the oracle (oracle/) alone.
  mutations                [(name, fn(inp, rng))]: each rewrites the inputs in place -- same
                           array sizes, so the same device addresses -- and needs a fresh
                           reference.  They are chosen so that a decision the host froze when the
                           call was captured, and that belongs to the device, gives a wrong
                           answer: all lengths <= 1 KiB -> some at the bound -> all 0 (record
                           jobs: one segment per range -> many -> the m == 0 shortcut), frames
                           sorted -> two swapped (the device must fall back to the record path)
                           -> sorted, another set of corrupted expected / stored values, new
                           payload bytes, new start values.
  shapes(inp)              what expected_schedule needs to know of each launch of the case.
  buffers / call / extract the device images (inputs, and outputs pre-filled with a sentinel),
                           the library call on their addresses, and the outputs in the
                           reference's form.  No torch here: the GPU test owns the tensors.
  output_mask / store      per buffer, the bytes include/hf3fs_crc.h lets the call write (the
                           whole-image check of tests/host_memory.py holds every other byte to
                           what was sent), and the inverse of extract for numpy stand-ins.

Not here: the >= 1 GiB byte-run forms of create_strided and scrub (test_gpu_parity.py::
test_create_strided, test_d4_*, test_gpu_aux.py::test_scrub_vs_oracle) and the update path
(test_gpu_parity.py, test_gpu_update_footprint.py).

expected_schedule, SWITCHES, LABELS and EXEMPT say which schedule of the hot kernel a case takes
under which switch, and which switches this file leaves to other tests.
"""
import numpy as np

M32 = 0xFFFFFFFF
NONE, CRC32C, CRC32 = 0, 1, 2
OK, INVALID_ARG, CHECKSUM_MISMATCH = 0, 3, 4080
SENT32 = 0x5E5E5E5E        # every output word before a call or a replay
SENT8 = 0x5E
KW = 16                    # kWaves: waves per workgroup (crc_kernels.h:27)
BLOCK = 1024               # kBlockBytes (crc_kernels.h:29)
PIPE_MAX = 16 << 10        # kPipeMaxLen (hf3fs_crc_api.hip)
BYTE_BUDGET = 32 << 20     # device bytes of one case

READ_DT = np.dtype([("data", "<u8"), ("offset", "<u4"), ("length", "<u4"), ("chunk_len", "<u4"),
                    ("batch_checksum_type", "u1"), ("chunk_checksum_type", "u1"), ("recalculate", "u1"),
                    ("reserved0", "u1"), ("chunk_checksum", "<u4"), ("out_checksum", "<u4"),
                    ("out_checksum_type", "u1"), ("reserved1", "u1", (3,)), ("status", "<i4"), ("reserved2", "<u4"), ("tail_pad", "<u4")])
SCRUB_DT = np.dtype([("data", "<u8"), ("length", "<u4"), ("checksum_type", "u1"), ("fin", "u1"), ("reserved", "<u2"),
                     ("checksum", "<u4"), ("computed", "<u4"), ("status", "<i4"), ("reserved2", "<u4")])
FRAME_DT = np.dtype([("offset", "<u8"), ("size", "<u4"), ("checksum", "<u4"), ("computed", "<u4"), ("status", "<i4")])
BLOCK_DT = np.dtype([("read_len", "<u8"), ("block_len", "<u8"), ("checksum", "<u4"), ("type", "u1"), ("missing", "u1"),
                     ("res", "u1", (2,))])
FILE_DT = np.dtype([("length", "<u8"), ("value", "<u4"), ("type", "u1"), ("res", "u1", (3,)), ("status", "<i4"),
                    ("res2", "<u4")])
assert (READ_DT.itemsize, SCRUB_DT.itemsize, FRAME_DT.itemsize, BLOCK_DT.itemsize, FILE_DT.itemsize) == \
    (48, 32, 24, 24, 24)


def _orc():
    import oracle
    oracle.lib()
    return oracle


def crc_ranges(ctype, arena, offs, lens, starts=None):
    """Raw ChecksumInfo::create value of arena[off:off + len] from start (default ~0), per range."""
    L = _orc().lib()
    f = (L.orc_crc32c_hw if L.orc_have_sse42() else L.orc_crc32c_sw) if ctype == CRC32C else L.orc_crc32_sw
    b = arena.ctypes.data
    n = len(offs)
    st = starts if starts is not None else np.full(n, M32, dtype=np.uint32)
    assert n == 0 or int((np.asarray(offs, dtype=np.uint64) + np.asarray(lens, dtype=np.uint64)).max()) <= arena.size
    return np.fromiter((f(int(s), b + int(o), int(ln)) for o, ln, s in zip(offs, lens, st)), dtype=np.uint32, count=n)


def _u32s(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _bytes(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def _flips(rng, n, k):
    """A xor mask per value: k of n values get one bit flipped (bits 8..31), the others none."""
    f = np.zeros(n, dtype=np.uint32)
    bad = rng.choice(n, min(k, n), replace=False)
    f[bad] = np.uint32(1) << rng.integers(8, 32, bad.size).astype(np.uint32)
    return f


class Case:
    name = ""
    entry = ""            # what expected_schedule keys on
    mismatch = False      # reports a mismatch set / count
    records = False       # a record batch (read results, scrub, frames): the anomaly record must stay clean
    poisoned = False      # takes library memory at default switches: part of the poisoned-scratch context
    mutations = ()
    layouts = {}          # buffer name -> record dtype, for the buffers that are arrays of ABI structs

    def device_bytes(self, inp):
        return sum(a.nbytes for a in self.buffers(inp, 1 << 40).values()) + \
            (inp["arena"].nbytes if "arena" in inp else 0)

    def output_mask(self, inp):
        """{buffer name: boolean byte mask over the buffer's image}, True where include/hf3fs_crc.h
        lets the call write.  Every buffer of `buffers` has an entry; the arena has none: no call
        here may write the bytes it hashes.  Each case cites the header lines its mask restates."""
        raise NotImplementedError

    def store(self, inp, host, ref):
        """Write `ref` (reference's form) into the output fields of the host images `host`: the
        inverse of extract, for the stand-in backends of tests/test_host_memory_model.py."""
        raise NotImplementedError


def _masks(images, whole=(), fields=None):
    """All-False masks over `images`, True for the buffers named in `whole` and, per
    fields = {buffer: (dtype, field names)}, for the bytes of those fields in every record."""
    m = {k: np.zeros(a.nbytes, dtype=bool) for k, a in images.items()}
    for k in whole:
        if k in m:
            m[k][:] = True
    for k, (dt, names) in (fields or {}).items():
        rec = np.zeros(dt.itemsize, dtype=bool)
        for f in names:
            fdt, off = dt.fields[f][:2]
            rec[off:off + fdt.itemsize] = True
        m[k] = np.tile(rec, images[k].nbytes // dt.itemsize)
    return m


def field_at(dt, byte):
    """The field of record dtype `dt` that byte offset `byte` of a record falls in ("padding": none)."""
    for name in dt.names:
        fdt, off = dt.fields[name][:2]
        if off <= byte < off + fdt.itemsize:
            return name
    return "padding"


# ---- create_batch / verify_batch: a list of ranges ------------------------------------------------
def _m_payload(inp, rng):
    inp["arena"][:] = _bytes(rng, inp["arena"].size)


def _m_starts(inp, rng):
    inp["starts"][:] = _u32s(rng, inp["starts"].size)


def _m_le_1k(inp, rng):
    n = inp["lens"].size
    inp["lens"][:] = rng.integers(0, min(1024, inp["max_len"]) + 1, n)
    inp["lens"][::7] = rng.integers(0, 5, inp["lens"][::7].size)


def _m_at_bound(inp, rng):
    n = inp["lens"].size
    k = rng.choice(n, max(1, min(n // 16, 300)), replace=False)
    inp["lens"][k] = inp["max_len"]


def _m_zero(inp, rng):
    inp["lens"][:] = 0


def _m_recorrupt(inp, rng):
    n = inp["flip"].size
    inp["flip"][:] = _flips(rng, n, 3 + int(rng.integers(0, max(2, min(n // 4, 40)))))


def _and_recorrupt(fn):
    """A verify case's mutation: the rewrite, then another set of corrupted expected values."""
    def both(inp, rng):
        fn(inp, rng)
        _m_recorrupt(inp, rng)
    return both


def _ragged_layout(cus, rng, scale):
    """About 100 ranges: every length class, bases at every residue mod 16 and at the residues mod
    128 around the segmented parts' grid alignment, and ranges whose first four bytes sit in the
    last three bytes of a 1 KiB block of the END-aligned grid (the whole-buffer branch's `spill`,
    taken when the batch runs as one segment per range)."""
    big = 200 * 1024 + 13
    lens = [0, 1, 3, 4, 5, 15, 16, 17] + list(range(1020, 1028)) + [2047, 4095, 4096, 4097, 8189, 65535, 65536, 65537,
                                                                   big, big - 1024 * 3 - 7]
    res128 = [0, 1, 112, 124, 125, 126, 127]
    lens = lens * 3
    while len(lens) < 100 * scale:
        lens.append(int(rng.choice([0, 1, 3, 5, 17, 1023, 2047, 4097, 8189, 65537])))
    n = len(lens)
    max_len = big
    size = 8 << 20
    offs = (rng.integers(0, (size - max_len - 4096) // 128, n) * 128).astype(np.int64)
    for i in range(n):
        offs[i] += i % 16 if i % 3 else res128[(i // 3) % len(res128)]
    # spill: base = 16 - r (mod 16), align16(base + len) - base = 1024 k + r, r in 1..3
    for j, (r, k) in enumerate([(1, 1), (2, 1), (3, 2), (3, 1)]):
        i = n - 1 - j
        offs[i] = offs[i] // 16 * 16 + 16 - r
        lens[i] = 1024 * k + r - 5 - j
    return np.array(lens), offs, max_len, size


def _small_many_layout(cus, rng, scale):
    n = (16 * KW * cus + 64) * scale
    lens = rng.integers(0, 301, n)
    size = 1 << 20
    return lens, rng.integers(0, size - 300, n), 300, size


def _balanced_layout(cus, rng, scale):
    n = (16 * KW * cus + 64) * scale
    lens = np.zeros(n, dtype=np.int64)
    k = rng.choice(n, 300, replace=False)
    lens[k] = rng.integers(17 << 10, (40 << 10) + 1, k.size)
    lens[k[0]] = 40 << 10
    short = rng.choice(n, 500, replace=False)  # and short ones among the empty (1..3: no room for the start xor)
    lens[short] += rng.choice([1, 2, 3, 7], short.size)
    size = 4 << 20
    return lens, rng.integers(0, size - (40 << 10) - 7, n), (40 << 10) + 7, size


def _ticketed_layout(cus, rng, scale):
    n = 8 * KW * cus * scale
    lens = rng.integers(0, 2049, n)
    lens[5] = 2048
    size = 2 << 20
    offs = rng.integers(0, size - 2048, n)
    for j, (r, k) in enumerate([(1, 1), (2, 1), (3, 1)]):  # the whole-buffer branch's `spill` (see _ragged_layout)
        i = 100 + j
        offs[i] = offs[i] // 16 * 16 + 16 - r
        lens[i] = 1024 * k + r - 4
    return lens, offs, 2048, size


class ListCase(Case):
    entry = "create_batch"

    def __init__(self, name, layout, ctypes=(CRC32C,), verify=None):
        self.name, self.layout, self.ctypes, self.verify = name, layout, ctypes, verify
        self.mismatch = verify is not None
        self.poisoned = verify == "scratch"
        if verify:
            self.entry = "verify_batch"
            self.mutations = (("payload", _and_recorrupt(_m_payload)), ("recorrupt", _m_recorrupt),
                              ("lens_le_1k", _and_recorrupt(_m_le_1k)), ("lens_at_bound", _and_recorrupt(_m_at_bound)),
                              ("lens_zero", _and_recorrupt(_m_zero)))
        else:
            self.mutations = (("payload", _m_payload), ("starts", _m_starts), ("lens_le_1k", _m_le_1k),
                              ("lens_at_bound", _m_at_bound), ("lens_zero", _m_zero))

    def build(self, cus, rng, scale=1):
        lens, offs, max_len, size = self.layout(cus, rng, scale)
        n = len(lens)
        inp = dict(arena=_bytes(rng, size), offs=np.asarray(offs, dtype=np.uint64), lens=np.asarray(lens, dtype=np.uint64),
                   max_len=int(max_len), cus=cus)
        assert int(inp["offs"].max()) + max_len <= size  # any length up to the bound stays inside the arena
        if self.verify:
            inp["flip"] = _flips(rng, n, 9)
        else:
            inp["starts"] = _u32s(rng, n)
        return inp

    def reference(self, inp):
        if self.verify:
            ref = dict(mismatch=(inp["flip"] != 0).astype(np.uint8),
                       count=np.array([np.count_nonzero(inp["flip"])], dtype=np.uint32))
            if self.verify == "given":
                ref["computed"] = crc_ranges(CRC32C, inp["arena"], inp["offs"], inp["lens"])
            return ref
        return {f"out{t}": crc_ranges(t, inp["arena"], inp["offs"], inp["lens"], inp["starts"]) for t in self.ctypes}

    def shapes(self, inp):
        s = dict(entry=self.entry, n=inp["lens"].size, max_len=inp["max_len"])
        if self.verify == "scratch":
            s["verify_scratch"] = True
        return [s] * len(self.ctypes)

    def buffers(self, inp, base):
        n = inp["lens"].size
        assert int(inp["lens"].max()) <= inp["max_len"] and int((inp["offs"] + inp["lens"]).max()) <= inp["arena"].size
        b = dict(addrs=inp["offs"] + np.uint64(base), lens=inp["lens"].copy())
        if self.verify:
            truth = crc_ranges(CRC32C, inp["arena"], inp["offs"], inp["lens"])
            b.update(expected=truth ^ inp["flip"], mismatch=np.full(n, SENT8, dtype=np.uint8),
                     count=np.full(1, SENT32, dtype=np.uint32))
            if self.verify == "given":
                b["computed"] = np.full(n, SENT32, dtype=np.uint32)
        else:
            b["starts"] = inp["starts"].copy()
            for t in self.ctypes:
                b[f"out{t}"] = np.full(n, SENT32, dtype=np.uint32)
        return b

    def call(self, L, inp, p, stream):
        n = inp["lens"].size
        if self.verify:
            L.verify_batch(CRC32C, p["addrs"], p["lens"], p["expected"], p["mismatch"], p["count"], n, inp["max_len"],
                           computed=p.get("computed"), stream=stream)
        else:
            for t in self.ctypes:
                L.create_batch(t, p["addrs"], p["lens"], p[f"out{t}"], n, inp["max_len"], starts=p["starts"],
                               stream=stream)

    def extract(self, inp, host):
        return {k: host[k] for k in (("mismatch", "count", "computed") if self.verify else
                                     [f"out{t}" for t in self.ctypes]) if k in host}

    def output_mask(self, inp):
        # create_batch: "d_out[i] receives the raw value" (hf3fs_crc.h:161).  verify_batch:
        # d_mismatch[i], *d_mismatch_count and, when given, d_computed (hf3fs_crc.h:172-174).
        return _masks(self.buffers(inp, 0), ("mismatch", "count", "computed") + tuple(f"out{t}" for t in self.ctypes))

    def store(self, inp, host, ref):
        for k, v in ref.items():
            host[k][:] = v


# ---- create_strided / verify_strided --------------------------------------------------------------
class StridedCase(Case):
    """create_strided at three shapes: (5, 200 KiB + 13) segmented, (W, 100) whole buffers with
    n % W == 0, (3, 0) empty; verify_strided at (7, 70 KiB + 5)."""
    entry = "create_strided"

    def __init__(self, name, verify=None):
        self.name, self.verify = name, verify
        self.mismatch = verify is not None
        self.poisoned = verify == "scratch"
        self.mutations = (("payload", _m_payload),)
        if verify:
            self.entry = "verify_strided"
            self.mutations = (("payload", _and_recorrupt(_m_payload)), ("recorrupt", _m_recorrupt))

    def build(self, cus, rng, scale=1):
        W = KW * cus
        if self.verify:
            geo = [(7 * scale, 70 * 1024 + 5, 70 * 1024 + 5 + 11)]
        else:
            geo = [(5 * scale, 200 * 1024 + 13, 200 * 1024 + 13 + 3), (W * scale, 100, 113), (3 * scale, 0, 16)]
        bases, pos = [], 5
        for n, ln, stride in geo:
            bases.append(pos)
            pos += n * stride + 64
        inp = dict(arena=_bytes(rng, pos + 64), geo=geo, bases=bases, cus=cus, start=0x12345678)
        if self.verify:
            inp["flip"] = _flips(rng, geo[0][0], 2)
        return inp

    def _truth(self, inp, k, start):
        n, ln, stride = inp["geo"][k]
        offs = inp["bases"][k] + np.arange(n, dtype=np.uint64) * np.uint64(stride)
        return crc_ranges(CRC32C, inp["arena"], offs, np.full(n, ln, dtype=np.uint64), np.full(n, start, dtype=np.uint32))

    def reference(self, inp):
        if self.verify:
            ref = dict(mismatch=(inp["flip"] != 0).astype(np.uint8),
                       count=np.array([np.count_nonzero(inp["flip"])], dtype=np.uint32))
            if self.verify == "given":
                ref["computed"] = self._truth(inp, 0, M32)
            return ref
        return dict(out=np.concatenate([self._truth(inp, k, inp["start"]) for k in range(len(inp["geo"]))]))

    def shapes(self, inp):
        out = []
        for n, ln, stride in inp["geo"]:
            s = dict(entry=self.entry, n=n, max_len=ln)
            if self.verify == "scratch":
                s["verify_scratch"] = True
            out.append(s)
        return out

    def buffers(self, inp, base):
        for (n, ln, stride), b0 in zip(inp["geo"], inp["bases"]):
            assert b0 + (n - 1) * stride + ln <= inp["arena"].size
        if self.verify:
            n = inp["geo"][0][0]
            b = dict(expected=self._truth(inp, 0, M32) ^ inp["flip"], mismatch=np.full(n, SENT8, dtype=np.uint8),
                     count=np.full(1, SENT32, dtype=np.uint32))
            if self.verify == "given":
                b["computed"] = np.full(n, SENT32, dtype=np.uint32)
            return b
        return {f"out{k}": np.full(g[0], SENT32, dtype=np.uint32) for k, g in enumerate(inp["geo"])}

    def call(self, L, inp, p, stream):
        for k, ((n, ln, stride), b0) in enumerate(zip(inp["geo"], inp["bases"])):
            if self.verify:
                L.verify_strided(CRC32C, p["arena"] + b0, stride, ln, n, p["expected"], p["mismatch"], p["count"],
                                 computed=p.get("computed"), stream=stream)
            else:
                L.create_strided(CRC32C, p["arena"] + b0, stride, ln, n, p[f"out{k}"], start=inp["start"], stream=stream)

    def extract(self, inp, host):
        if self.verify:
            return {k: host[k] for k in ("mismatch", "count", "computed") if k in host}
        return dict(out=np.concatenate([host[f"out{k}"] for k in range(len(inp["geo"]))]))

    def output_mask(self, inp):
        # create_strided: d_out as create_batch's (hf3fs_crc.h:165-168).  verify_strided: the
        # outputs of verify_batch (hf3fs_crc.h:172-174, :182-184).
        return _masks(self.buffers(inp, 0), ("mismatch", "count", "computed") + tuple(f"out{k}" for k in range(3)))

    def store(self, inp, host, ref):
        if self.verify:
            for k, v in ref.items():
                host[k][:] = v
            return
        pos = 0
        for k, g in enumerate(inp["geo"]):
            host[f"out{k}"][:] = ref["out"][pos:pos + g[0]]
            pos += g[0]


# ---- verify_blocks --------------------------------------------------------------------------------
def _m_blocks_le_1k(inp, rng):
    inp["lens"][:] = rng.integers(0, 1025, inp["lens"].size)


class BlocksCase(Case):
    """KV blocks by arena offset, more than 16 per wave and longer than the prefetch bound: the
    byte-balanced schedule (the balance region, poisoned with the rest)."""
    entry = "verify_blocks"
    mismatch = True

    def __init__(self, name, verify):
        self.name, self.verify = name, verify
        self.poisoned = verify == "scratch"
        self.mutations = (("payload", _and_recorrupt(_m_payload)), ("recorrupt", _m_recorrupt),
                          ("lens_le_1k", _and_recorrupt(_m_blocks_le_1k)), ("lens_at_bound", _and_recorrupt(_m_at_bound)),
                          ("lens_zero", _and_recorrupt(_m_zero)))

    def build(self, cus, rng, scale=1):
        n = (16 * KW * cus + 64) * scale
        lens = rng.choice([0, 0, 0, 0, 0, 0, 0, 1, 3, 512, 4096, 8192, 40960], n).astype(np.uint32)
        size = 4 << 20
        offs = (rng.integers(0, (size - 40960) // 4096, n) * 4096).astype(np.uint64)
        offs[::5] += rng.integers(0, 16, offs[::5].size).astype(np.uint64)
        return dict(arena=_bytes(rng, size + 16), offs=offs, lens=lens, max_len=40960, cus=cus, flip=_flips(rng, n, 19))

    def reference(self, inp):
        ref = dict(mismatch=(inp["flip"] != 0).astype(np.uint8),
                   count=np.array([np.count_nonzero(inp["flip"])], dtype=np.uint32))
        if self.verify == "given":
            ref["computed"] = crc_ranges(CRC32C, inp["arena"], inp["offs"], inp["lens"])
        return ref

    def shapes(self, inp):
        s = dict(entry=self.entry, n=inp["lens"].size, max_len=inp["max_len"])
        if self.verify == "scratch":
            s["verify_scratch"] = True
        return [s]

    def buffers(self, inp, base):
        n = inp["lens"].size
        assert int(inp["lens"].max()) <= inp["max_len"]
        assert int((inp["offs"] + inp["lens"].astype(np.uint64)).max()) <= inp["arena"].size
        truth = crc_ranges(CRC32C, inp["arena"], inp["offs"], inp["lens"])
        b = dict(offs=inp["offs"].copy(), lens=inp["lens"].copy(), expected=truth ^ inp["flip"],
                 mismatch=np.full(n, SENT8, dtype=np.uint8), count=np.full(1, SENT32, dtype=np.uint32))
        if self.verify == "given":
            b["computed"] = np.full(n, SENT32, dtype=np.uint32)
        return b

    def call(self, L, inp, p, stream):
        L.verify_blocks(CRC32C, p["arena"], p["offs"], p["lens"], p["expected"], p["mismatch"], p["count"],
                        inp["lens"].size, inp["max_len"], computed=p.get("computed"), stream=stream)

    def extract(self, inp, host):
        return {k: host[k] for k in ("mismatch", "count", "computed") if k in host}

    def output_mask(self, inp):
        # "Same outputs as hf3fs_crc_verify_batch" (hf3fs_crc.h:187; :172-174).
        return _masks(self.buffers(inp, 0), ("mismatch", "count", "computed"))

    def store(self, inp, host, ref):
        for k, v in ref.items():
            host[k][:] = v


# ---- read results ---------------------------------------------------------------------------------
def _read_restore(inp, rng):
    """Stored chunk checksums = the truth of the arena's bytes, a tenth of them stale."""
    r = inp["recs"]
    truth = crc_ranges(CRC32C, inp["arena"], inp["chunk_off"], r["chunk_len"])
    r["chunk_checksum"] = truth ^ np.where(rng.random(r.size) < 0.1, np.uint32(0x80), np.uint32(0))


def _m_read_payload(inp, rng):
    _m_payload(inp, rng)
    _read_restore(inp, rng)


def _m_read_recorrupt(inp, rng):
    r = inp["recs"]
    r["chunk_checksum"] ^= np.where(rng.random(r.size) < 0.3, np.uint32(0x100), np.uint32(0))


def _m_read_le_1k(inp, rng):
    r = inp["recs"]
    room = np.minimum(r["chunk_len"] - r["offset"], 1024)
    r["length"] = (rng.random(r.size) * (room + 1)).astype(np.uint32)
    full = np.flatnonzero(r["chunk_len"] <= 1024)[::2]  # small chunks read in full stay in the mix
    r["offset"][full] = 0
    r["length"][full] = r["chunk_len"][full]


def _m_read_at_bound(inp, rng):
    r = inp["recs"]
    k = rng.choice(r.size, r.size // 8, replace=False)
    r["chunk_len"][k] = inp["max_len"]
    r["offset"][k] = 0
    r["length"][k] = inp["max_len"]
    r["length"][k[::3]] -= 1
    _read_restore(inp, rng)


def _m_read_zero(inp, rng):
    inp["recs"]["length"] = 0
    inp["recs"]["offset"] = 0


class ReadCase(Case):
    """About 300 completed reads, bound 128 KiB: NONE batch type, full-chunk reuse, recalculate with
    a right and a wrong stored checksum, partial reads, length 0."""
    name, entry, records, poisoned, mismatch = "read_result", "read_result", True, True, True
    mutations = (("payload", _m_read_payload), ("recorrupt", _m_read_recorrupt), ("lens_le_1k", _m_read_le_1k),
                 ("lens_at_bound", _m_read_at_bound), ("lens_zero", _m_read_zero))

    def build(self, cus, rng, scale=1):
        n, bound, size = 300 * scale, 128 * 1024, 12 << 20
        r = np.zeros(n, dtype=READ_DT)
        r["chunk_len"] = rng.choice([1024, 16 * 1024, bound], n)
        chunk_off = rng.integers(0, size - bound, n).astype(np.uint64)  # any chunk may grow to the bound
        kind = np.arange(n) % 6
        r["batch_checksum_type"] = np.where(kind == 0, NONE, CRC32C)
        r["chunk_checksum_type"] = np.where(np.arange(n) % 11 == 10, NONE, CRC32C)
        r["recalculate"] = np.isin(kind, (0, 2, 3))
        part = np.isin(kind, (4, 5))
        r["offset"] = np.where(part, (rng.random(n) * (r["chunk_len"] - 1)).astype(np.uint32), 0)
        r["length"] = np.where(part, (rng.random(n) * (r["chunk_len"] - r["offset"] + 1)).astype(np.uint32), r["chunk_len"])
        r["length"][kind == 5] = np.where(np.arange(np.count_nonzero(kind == 5)) % 2, 0, r["length"][kind == 5])
        inp = dict(arena=_bytes(rng, size), recs=r, chunk_off=chunk_off, max_len=bound, cus=cus)
        _read_restore(inp, rng)
        return inp

    def reference(self, inp):
        orc = _orc()
        r, a = inp["recs"], inp["arena"]
        st, ty, va = [], [], []
        for i in range(r.size):
            u, c0 = r[i], int(inp["chunk_off"][i])
            off, ln, cl = int(u["offset"]), int(u["length"]), int(u["chunk_len"])
            rc, (t, v) = orc.read_result(int(u["batch_checksum_type"]), (int(u["chunk_checksum_type"]), int(u["chunk_checksum"])),
                                         off, a[c0 + off:c0 + off + ln], cl, full_chunk=a[c0:c0 + cl],
                                         recalculate=bool(u["recalculate"]))
            st.append(rc), ty.append(t), va.append(v)
        return dict(status=np.array(st, dtype=np.int32), type=np.array(ty, dtype=np.uint8), value=np.array(va, dtype=np.uint32))

    def shapes(self, inp):
        r = inp["recs"]
        full = (r["offset"] == 0) & (r["length"] == r["chunk_len"])
        reuse = full & (r["batch_checksum_type"] == r["chunk_checksum_type"])
        need = ((r["batch_checksum_type"] != NONE) & ~reuse) | ((r["recalculate"] != 0) & full & (r["chunk_checksum_type"] != NONE))
        return [dict(entry="record", n=r.size, max_len=inp["max_len"], dev_max=int(r["length"][need].max(initial=0)))]

    def buffers(self, inp, base):
        r = inp["recs"].copy()
        assert int((r["offset"] + r["length"]).max()) <= inp["max_len"] and int(r["length"].max()) <= inp["max_len"]
        assert int((inp["chunk_off"] + r["offset"] + r["length"]).max()) <= inp["arena"].size
        r["data"] = inp["chunk_off"] + r["offset"] + np.uint64(base)
        r["out_checksum"], r["out_checksum_type"], r["status"] = SENT32, SENT8, 0x5E5E5E5E
        return dict(recs=r.view(np.uint8).reshape(-1))

    def call(self, L, inp, p, stream):
        L.read_result_batch(CRC32C, p["recs"], inp["recs"].size, inp["max_len"], stream=stream)

    def extract(self, inp, host):
        r = host["recs"].view(READ_DT)
        return dict(status=r["status"].copy(), type=r["out_checksum_type"].copy(), value=r["out_checksum"].copy())

    layouts = {"recs": READ_DT}

    def output_mask(self, inp):
        # hf3fs_crc_read_io's fields under "outputs" (hf3fs_crc.h:423-427); reserved0..2 and the
        # struct's tail padding are not the call's.
        return _masks(self.buffers(inp, 0), fields={"recs": (READ_DT, ("out_checksum", "out_checksum_type", "status"))})

    def store(self, inp, host, ref):
        r = host["recs"].view(READ_DT)
        r["status"], r["out_checksum_type"], r["out_checksum"] = ref["status"], ref["type"], ref["value"]


# ---- scrub ----------------------------------------------------------------------------------------
def _scrub_restore(inp, rng):
    r = inp["recs"]
    truth = crc_ranges(CRC32C, inp["arena"], inp["off"], r["length"])
    stored = np.where(r["fin"] == 1, ~truth, truth)
    r["checksum"] = stored ^ _flips(rng, r.size, r.size // 7)


def _m_scrub_payload(inp, rng):
    _m_payload(inp, rng)
    _scrub_restore(inp, rng)


def _m_scrub_recorrupt(inp, rng):
    inp["recs"]["checksum"] ^= _flips(rng, inp["recs"].size, inp["recs"].size // 5)


def _m_scrub_le_1k(inp, rng):
    inp["recs"]["length"] = rng.integers(0, 1025, inp["recs"].size)
    _scrub_restore(inp, rng)


def _m_scrub_at_bound(inp, rng):
    r = inp["recs"]
    r["length"][rng.choice(r.size, r.size // 8, replace=False)] = inp["max_len"]
    _scrub_restore(inp, rng)


def _m_scrub_zero(inp, rng):
    inp["recs"]["length"] = 0
    _scrub_restore(inp, rng)


class ScrubCase(Case):
    """About 200 stored chunks, bound 256 KiB: raw and finalized persisted values, NONE records,
    malformed records (another type, fin > 1) and corrupted stored values."""
    name, entry, records, poisoned, mismatch = "scrub", "record", True, True, True
    mutations = (("payload", _m_scrub_payload), ("recorrupt", _m_scrub_recorrupt), ("lens_le_1k", _m_scrub_le_1k),
                 ("lens_at_bound", _m_scrub_at_bound), ("lens_zero", _m_scrub_zero))

    def build(self, cus, rng, scale=1):
        n, bound, size = 200 * scale, 256 * 1024, 12 << 20
        r = np.zeros(n, dtype=SCRUB_DT)
        r["length"] = rng.choice([0, 1, 3, 4096, 65536, 131072 + 7, bound, bound - 1], n)
        r["length"][::3] = rng.integers(0, bound + 1, r["length"][::3].size)
        r["checksum_type"] = np.where(np.arange(n) % 9 == 8, NONE, CRC32C)
        r["fin"] = rng.integers(0, 2, n)
        r["checksum_type"][5::41] = CRC32  # malformed: not the batch's type
        r["fin"][7::43] = 7                # malformed
        inp = dict(arena=_bytes(rng, size), recs=r, off=rng.integers(0, size - bound, n).astype(np.uint64),
                   max_len=bound, cus=cus)
        _scrub_restore(inp, rng)
        return inp

    def reference(self, inp):
        orc = _orc()
        r, a = inp["recs"], inp["arena"]
        st, comp = [], []
        for i in range(r.size):
            t, fin, ln, o = int(r["checksum_type"][i]), int(r["fin"][i]), int(r["length"][i]), int(inp["off"][i])
            if t not in (NONE, CRC32C) or fin > 1 or ln > inp["max_len"]:
                rc, c = INVALID_ARG, 0
            else:
                rc, c = orc.scrub(t, fin, a[o:o + ln], int(r["checksum"][i]))
            st.append(rc), comp.append(c)
        st = np.array(st, dtype=np.int32)
        return dict(status=st, computed=np.array(comp, dtype=np.uint32),
                    count=np.array([np.count_nonzero(st)], dtype=np.uint32))

    def shapes(self, inp):
        r = inp["recs"]
        need = (r["checksum_type"] == CRC32C) & (r["fin"] <= 1)
        return [dict(entry="record", n=r.size, max_len=inp["max_len"], dev_max=int(r["length"][need].max(initial=0)),
                     runs_ok=True)]

    def buffers(self, inp, base):
        r = inp["recs"].copy()
        assert int(r["length"].max()) <= inp["max_len"]
        assert int((inp["off"] + r["length"]).max()) <= inp["arena"].size
        r["data"] = inp["off"] + np.uint64(base)
        r["computed"], r["status"] = SENT32, 0x5E5E5E5E
        return dict(recs=r.view(np.uint8).reshape(-1), count=np.full(1, SENT32, dtype=np.uint32))

    def call(self, L, inp, p, stream):
        L.scrub_batch(CRC32C, p["recs"], inp["recs"].size, inp["max_len"], p["count"], stream=stream)

    def extract(self, inp, host):
        r = host["recs"].view(SCRUB_DT)
        return dict(status=r["status"].copy(), computed=r["computed"].copy(), count=host["count"])

    layouts = {"recs": SCRUB_DT}

    def output_mask(self, inp):
        # hf3fs_crc_scrub_io: computed and status are "out" (hf3fs_crc.h:499-500; computed is
        # written for every record, "0 for NONE"); *d_mismatch_count is SET (hf3fs_crc.h:507).
        return _masks(self.buffers(inp, 0), ("count",), {"recs": (SCRUB_DT, ("computed", "status"))})

    def store(self, inp, host, ref):
        r = host["recs"].view(SCRUB_DT)
        r["status"], r["computed"] = ref["status"], ref["computed"]
        host["count"][:] = ref["count"]


# ---- serde frames ---------------------------------------------------------------------------------
def _frame_truth(inp, compressed):
    f = inp["frames"]
    lin = crc_ranges(CRC32C, inp["arena"], f["offset"], f["size"], np.zeros(f.size, dtype=np.uint32))
    return (lin & np.uint32(0xFFFFFF00)) | np.uint32(0x86) | compressed.astype(np.uint32)  # Checksum::calcSerde


def _frames_restore(inp, rng):
    """Header checksums = calcSerde of the payloads (random compressed bit), a few corrupted."""
    f = inp["frames"]
    ok = f["size"] <= inp["max_size"]
    sizes = f["size"].copy()
    f["size"][~ok] = 0  # (an oversize frame's bytes may lie past the buffer: nothing of it is hashed)
    truth = _frame_truth(inp, rng.integers(0, 2, f.size))
    f["size"] = sizes
    f["checksum"] = truth ^ _flips(rng, f.size, 3 + f.size // 20)


def _m_frames_payload(inp, rng):
    _m_payload(inp, rng)
    _frames_restore(inp, rng)


def _m_frames_recorrupt(inp, rng):
    inp["frames"]["checksum"] ^= _flips(rng, inp["frames"].size, 5 + inp["frames"].size // 10)


def _m_frames_swap(inp, rng):
    f = inp["frames"]
    cand = np.flatnonzero((f["size"][:-1] > 0) & (f["size"][1:] > 0))
    i = int(cand[cand.size // 3])
    f[[i, i + 1]] = f[[i + 1, i]]
    inp["swapped"] = i


def _m_frames_unswap(inp, rng):
    f, i = inp["frames"], inp.pop("swapped")
    f[[i, i + 1]] = f[[i + 1, i]]
    _m_frames_recorrupt(inp, rng)


def _m_frames_zero(inp, rng):
    inp["frames"]["size"] = 0
    _frames_restore(inp, rng)


class FramesCase(Case):
    """walked: 300 frames of 0..5000 B as the framing walk leaves them (the stream path is tried
    from 256 frames on).  gaps: junk between frames, a lead offset of 5, empty frames at both ends
    and one frame above max_size (the device sends the batch to the record path).  big: W / 16 + 4
    walked frames, one of 300 KiB + 3 among small ones (it spans many stream segments)."""
    entry, records, poisoned, mismatch = "frames", True, True, True
    mutations = (("payload", _m_frames_payload), ("swap", _m_frames_swap), ("unswap", _m_frames_unswap),
                 ("recorrupt", _m_frames_recorrupt), ("sizes_zero", _m_frames_zero))

    def __init__(self, name, layout):
        self.name, self.layout = name, layout

    def build(self, cus, rng, scale=1):
        lead, gaps, max_size = 0, None, 8192
        if self.layout == "walked":
            sizes = rng.integers(0, 5001, 300 * scale)
            sizes[3:9] = 5000, 0, 1, 2, 3, 4
        elif self.layout == "gaps":
            sizes = rng.integers(0, 5001, 300 * scale)
            sizes[::9] = rng.choice([0, 1, 15, 16, 17, 1023, 1024, 1025], sizes[::9].size)
            sizes[0] = sizes[-1] = 0
            sizes[sizes.size // 2] = 7000
            lead, gaps, max_size = 5, rng.integers(0, 101, sizes.size), 6000
            gaps[0] = 0
        else:
            sizes = rng.integers(0, 601, (KW * cus // 16 + 4) * scale)
            sizes[sizes.size // 2] = 300 * 1024 + 3
            max_size = 512 * 1024
        f = np.zeros(sizes.size, dtype=FRAME_DT)
        pos = lead
        for i, sz in enumerate(sizes.tolist()):
            pos += (int(gaps[i]) if gaps is not None else 0) + 8  # junk, then the MessageHeader
            f["offset"][i], f["size"][i] = pos, sz
            pos += sz
        inp = dict(arena=_bytes(rng, pos + 16), frames=f, max_size=max_size, cus=cus)
        _frames_restore(inp, rng)
        return inp

    def reference(self, inp):
        f = inp["frames"]
        ok = f["size"] <= inp["max_size"]
        sizes = f["size"].copy()
        f["size"][~ok] = 0
        computed = _frame_truth(inp, f["checksum"] & 1)
        f["size"] = sizes
        computed[~ok] = 0
        st = np.where(ok, np.where(computed == f["checksum"], OK, CHECKSUM_MISMATCH), INVALID_ARG).astype(np.int32)
        return dict(status=st, computed=computed, count=np.array([np.count_nonzero(st)], dtype=np.uint32))

    def shapes(self, inp):
        f = inp["frames"]
        off, size = f["offset"].astype(np.int64), f["size"].astype(np.int64)
        end = off + size
        ok = f["size"] <= inp["max_size"]
        gap = np.maximum(off[1:] - end[:-1] - 8, 0)
        return [dict(entry="frames", n=f.size, max_len=inp["max_size"], dev_max=int(f["size"][ok].max(initial=0)),
                     sorted_ok=bool(ok.all() and (end[:-1] <= off[1:]).all()), pay=int(size.sum()), gap=int(gap.sum()))]

    def buffers(self, inp, base):
        f = inp["frames"].copy()
        ok = f["size"] <= inp["max_size"]
        assert int((f["offset"][ok] + f["size"][ok]).max()) <= inp["arena"].size and int(f["offset"].min()) >= 8
        f["computed"], f["status"] = SENT32, 0x5E5E5E5E
        return dict(frames=f.view(np.uint8).reshape(-1), count=np.full(1, SENT32, dtype=np.uint32))

    def call(self, L, inp, p, stream):
        L.frame_verify_batch(p["arena"], p["frames"], inp["frames"].size, inp["max_size"], p["count"], stream=stream)

    def extract(self, inp, host):
        f = host["frames"].view(FRAME_DT)
        return dict(status=f["status"].copy(), computed=f["computed"].copy(), count=host["count"])

    layouts = {"frames": FRAME_DT}

    def output_mask(self, inp):
        # hf3fs_crc_frame: computed and status are "out" (hf3fs_crc.h:657-658); *d_mismatch_count
        # is SET (hf3fs_crc.h:671).
        return _masks(self.buffers(inp, 0), ("count",), {"frames": (FRAME_DT, ("computed", "status"))})

    def store(self, inp, host, ref):
        f = host["frames"].view(FRAME_DT)
        f["status"], f["computed"] = ref["status"], ref["computed"]
        host["count"][:] = ref["count"]


# ---- file digest ----------------------------------------------------------------------------------
def _m_digest_values(inp, rng):
    inp["blocks"]["checksum"] = _u32s(rng, inp["blocks"].size)


def _m_digest_holes(inp, rng):
    b = inp["blocks"]
    b["read_len"] = b["block_len"]
    b["missing"] = 0
    u = rng.random(b.size)
    short = u < 0.04
    b["read_len"][short] = (rng.random(np.count_nonzero(short)) * b["block_len"][short]).astype(np.uint64)
    b["missing"][(u > 0.04) & (u < 0.06)] = 1


class DigestCase(Case):
    """About 20 files with block counts around the wave path's lane runs (0, 1, 2, 63..65,
    1023..1025) and one of 2049 blocks, which takes the split path: that one needs library memory
    with fill-zero too (digest_kernels.hip digest_scratch_bytes).  Short reads, missing chunks, a
    type mismatch and an unknown type."""
    entry, poisoned, mismatch = "file_digest", True, False
    mutations = (("values", _m_digest_values), ("holes", _m_digest_holes))

    def __init__(self, name, fill_zero):
        self.name, self.fill_zero = name, fill_zero

    def build(self, cus, rng, scale=1):
        counts = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 1, 2, 64, 65, 7, 7, 30, 100, 1024, 0] * scale
        off = np.zeros(len(counts) + 1, dtype=np.uint64)
        off[1:] = np.cumsum(counts)
        b = np.zeros(int(off[-1]), dtype=BLOCK_DT)
        b["block_len"] = rng.choice([1, 17, 4096, 1 << 20], b.size)
        b["type"] = CRC32C
        inp = dict(blocks=b, file_off=off, cus=cus)
        _m_digest_values(inp, rng)
        _m_digest_holes(inp, rng)
        for f in (1, 3, 6, 11, 13):  # some files stay whole: a digest of every block
            b["read_len"][int(off[f]):int(off[f + 1])] = b["block_len"][int(off[f]):int(off[f + 1])]
            b["missing"][int(off[f]):int(off[f + 1])] = 0
        b["type"][int(off[15]) + 3] = CRC32  # a type mismatch in file 15
        b["type"][int(off[16]) + 2] = 3      # an unknown type in file 16
        return inp

    def reference(self, inp):
        res = _orc().file_digest_batch(inp["blocks"], inp["file_off"], fill_zero=self.fill_zero)
        off = inp["file_off"].astype(np.int64)
        csum = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(inp["blocks"]["block_len"], dtype=np.uint64)])
        ok = res["status"] == 0
        return dict(status=res["status"].astype(np.int32), length=(csum[off[1:]] - csum[off[:-1]]).astype(np.uint64),
                    type=np.where(ok, res["type"], 0).astype(np.uint8), value=np.where(ok, res["value"], 0).astype(np.uint32))

    def shapes(self, inp):
        nb = np.diff(inp["file_off"].astype(np.int64))
        return [dict(entry="file_digest", n=nb.size, max_blocks=int(nb.max()), fill_zero=self.fill_zero)]

    def buffers(self, inp, base):
        n = inp["file_off"].size - 1
        assert int(inp["file_off"][-1]) == inp["blocks"].size
        return dict(blocks=inp["blocks"].view(np.uint8).reshape(-1).copy(), file_off=inp["file_off"].copy(),
                    out=np.full(n * FILE_DT.itemsize, SENT8, dtype=np.uint8))

    def call(self, L, inp, p, stream):
        nb = np.diff(inp["file_off"].astype(np.int64))
        L.file_digest_batch(p["blocks"], p["file_off"], p["out"], nb.size, int(nb.max()), stream=stream,
                            fill_zero=self.fill_zero)

    def extract(self, inp, host):
        o = host["out"].view(FILE_DT)
        ok = o["status"] == 0  # (type and value are the digest's only when the fold succeeded)
        return dict(status=o["status"].copy(), length=o["length"].copy(), type=np.where(ok, o["type"], 0).astype(np.uint8),
                    value=np.where(ok, o["value"], 0).astype(np.uint32))

    layouts = {"blocks": BLOCK_DT, "out": FILE_DT}

    def output_mask(self, inp):
        # "the result (or the first error's status) goes to d_out[f]" (hf3fs_crc.h:468-469): d_out
        # is an output array of whole hf3fs_crc_file_digest records, nothing in it is an input;
        # d_blocks and d_file_off are const (hf3fs_crc.h:470-471, :480-482).
        return _masks(self.buffers(inp, 0), ("out",))

    def store(self, inp, host, ref):
        o = host["out"].view(FILE_DT)
        o[:] = np.zeros(1, dtype=FILE_DT)
        o["status"], o["length"], o["type"], o["value"] = ref["status"], ref["length"], ref["type"], ref["value"]


# ---- combine / serialize / finalize: no scratch, capture and replay only -------------------------
def _m_scalar_values(inp, rng):
    for k in ("acc", "crc2", "values"):
        if k in inp:
            inp[k][:] = _u32s(rng, inp[k].size)


def _m_scalar_lens(inp, rng):
    inp["len2"][:] = rng.integers(0, 1 << 33, inp["len2"].size)
    inp["len2"][::5] = 0


class ScalarCase(Case):
    entry = "scalar"

    def __init__(self, name):
        self.name = name
        self.mutations = (("values", _m_scalar_values),) + ((("lens", _m_scalar_lens),) if name == "combine" else ())

    def build(self, cus, rng, scale=1):
        n = 1000 * scale + 3
        if self.name == "combine":
            len2 = rng.choice([0, 1, 3, 4, 255, 256, 4096, (1 << 20) + 1, (1 << 32) + 5], n).astype(np.uint64)
            return dict(acc=_u32s(rng, n), crc2=_u32s(rng, n), len2=len2, cus=cus)
        return dict(values=_u32s(rng, n), cus=cus)

    def reference(self, inp):
        if self.name == "combine":
            return dict(acc=_orc().combine_batch(inp["acc"], inp["crc2"], inp["len2"]))
        if self.name == "serialize":
            n = inp["values"].size
            want = np.empty((n, 6), dtype=np.uint8)
            want[:, 0], want[:, 1] = 5, CRC32C  # ChecksumInfo's serde form (hf3fs_checksum_serialize)
            want[:, 2:] = inp["values"].astype("<u4").view(np.uint8).reshape(n, 4)
            return dict(out=want.reshape(-1))
        return dict(values=~inp["values"])

    def shapes(self, inp):
        return [dict(entry="scalar")]

    def buffers(self, inp, base):
        if self.name == "combine":
            return dict(acc=inp["acc"].copy(), crc2=inp["crc2"].copy(), len2=inp["len2"].copy())
        if self.name == "serialize":
            return dict(values=inp["values"].copy(), out=np.full(6 * inp["values"].size, SENT8, dtype=np.uint8))
        return dict(values=inp["values"].copy())

    def call(self, L, inp, p, stream):
        if self.name == "combine":
            L.combine_batch(CRC32C, p["acc"], p["crc2"], p["len2"], inp["acc"].size, stream=stream)
        elif self.name == "serialize":
            L.serialize_batch(CRC32C, p["values"], inp["values"].size, p["out"], stream=stream)
        else:
            L.finalize_batch(p["values"], inp["values"].size, stream=stream)

    def extract(self, inp, host):
        return {k: host[k] for k in dict(combine=("acc",), serialize=("out",), finalize=("values",))[self.name]}

    def output_mask(self, inp):
        # combine_batch updates d_acc in place, d_crc2 and d_len2 are const (hf3fs_crc.h:192-196);
        # serialize_batch writes d_out = n x 6 bytes (hf3fs_crc.h:198-200); finalize_batch maps
        # d_values in place (hf3fs_crc.h:203-205).
        return _masks(self.buffers(inp, 0), dict(combine=("acc",), serialize=("out",), finalize=("values",))[self.name])

    def store(self, inp, host, ref):
        for k, v in ref.items():
            host[k][:] = v


CASES = {c.name: c for c in [
    ListCase("create_list_ragged", _ragged_layout, ctypes=(CRC32C, CRC32)),
    ListCase("create_list_small_many", _small_many_layout),
    ListCase("create_list_small_many_balanced", _balanced_layout),
    ListCase("create_list_ticketed", _ticketed_layout),
    StridedCase("create_strided"),
    ListCase("verify_batch_scratch", _ticketed_layout, verify="scratch"),
    ListCase("verify_batch_given", _ticketed_layout, verify="given"),
    StridedCase("verify_strided_scratch", verify="scratch"),
    StridedCase("verify_strided_given", verify="given"),
    BlocksCase("verify_blocks_scratch", "scratch"),
    BlocksCase("verify_blocks_given", "given"),
    ReadCase(),
    ScrubCase(),
    FramesCase("frames_walked", "walked"),
    FramesCase("frames_gaps", "gaps"),
    FramesCase("frames_big", "big"),
    DigestCase("file_digest_fill_zero", True),
    DigestCase("file_digest_strict", False),
    ScalarCase("combine"),
    ScalarCase("serialize"),
    ScalarCase("finalize"),
]}
CASES["create_list_small_many_balanced"].poisoned = True  # the balance region (Mem::kBalance)


# ---- which schedule a shape takes -----------------------------------------------------------------
DEFAULTS = dict(nt="1", seg_kib="0", static="0", pipe="auto", balance="1", record_direct="1", range_stream="0",
                list_runs="0", prehash_rep="1", frame_stream="auto", frame_segw="2")
SCHEDULES = ("direct_static", "direct_pipe", "direct_ticketed", "segmented_ticketed", "segmented_static", "balanced",
             "range_stream", "byte_runs", "byte_runs_rep")


def _make_plan(cus, n, max_len, sw, seg_hint=0):
    """make_plan (hf3fs_crc_api.hip) -> (seg_bytes, segs, grid, pipe_max)."""
    waves = cus * KW
    max_seg = max(BLOCK, -(-max_len // BLOCK) * BLOCK)
    seg, total = max_seg, n * max_len
    if int(sw["seg_kib"]):
        seg = int(sw["seg_kib"]) * 1024
    elif seg_hint:
        seg = seg_hint
    elif total // waves < 4 * seg:
        target, seg = max(total // (4 * waves), 64 << 10), 64 << 10
        while seg < target:
            seg <<= 1
    seg = min(seg, max_seg)
    segs = max(1, -(-max_len // seg))
    grid = max(1, min(-(-(n * segs) // KW), cus))
    pipe_max = PIPE_MAX if sw["pipe"] == "auto" else (1 << 64) - 1 if sw["pipe"] == "1" else 0
    return seg, segs, grid, pipe_max


def _kernel(n, segs, grid, direct, queue, bal, len_bound, pipe_max):
    """k_crc_ranges' own choices (crc_kernels.hip:412-434)."""
    ntasks, nwaves = n * segs, grid * KW
    if ntasks <= nwaves or ntasks > 16 * nwaves:  # :420 tickets dropped
        queue = False
    if bal and not queue:                          # :425
        return "balanced"
    if direct and not queue and len_bound <= pipe_max:  # :430
        return "direct_pipe"
    return ("direct" if direct else "segmented") + ("_ticketed" if queue else "_static")


def _schedule(shape, cus, switches):
    sw = dict(DEFAULTS, **{k: str(v) for k, v in (switches or {}).items()})
    entry, mem = shape["entry"], set()
    if shape.get("verify_scratch"):
        mem.add("verify")                                           # verify_begin
    if entry == "scalar":
        return None, mem
    if entry == "file_digest":                                      # hf3fs_crc_file_digest_batch_ex
        splits = min(64, max(1, -(-shape["max_blocks"] // 2048)))   # digest_kernels.hip:335-339
        if splits > 1 or not shape["fill_zero"]:                    # digest_kernels.hip:330-333
            mem.add("call")
        return None, mem
    n, max_len = shape["n"], shape["max_len"]
    waves = cus * KW
    if entry in ("create_strided", "verify_strided"):               # hf3fs_crc_create_strided
        whole = n % waves == 0 or n >= 8 * waves
        seg, segs, grid, pipe_max = _make_plan(cus, n, max_len, sw, max(max_len, 1) if whole else 0)
        per_wave = n * max_len // waves
        rep = -(-per_wave // (4 << 20)) if per_wave > (4 << 20) else 1
        big = n < (1 << 31) and n * max_len >= (1 << 30) and max_len >= (64 << 10)
        window = rep > 1 and not (whole and max_len <= (4 << 20))
        if big and ((not whole and segs > 1) or window):
            mem.add("call")
            return ("byte_runs" if rep == 1 else "byte_runs_rep"), mem
        if n * segs > grid * KW and sw["static"] == "0":            # launch_prepare (create_strided then drops the counter)
            mem.add("counter")
        return _kernel(n, segs, grid, segs == 1, False, False, seg, pipe_max), mem
    if entry in ("create_batch", "verify_batch", "verify_blocks"):
        if entry != "verify_blocks" and sw["list_runs"] != "0":     # hf3fs_crc_create_batch
            mem.add("call")
            return ("byte_runs" if int(sw["prehash_rep"]) <= 1 else "byte_runs_rep"), mem
        seg, segs, grid, pipe_max = _make_plan(cus, n, max_len, sw)
        queue = n * segs > grid * KW and sw["static"] == "0"        # launch_prepare, tickets_allowed
        if queue:
            mem.add("counter")
        bal = sw["balance"] != "0" and segs == 1 and max_len > pipe_max and n > 16 * grid * KW  # plan_balance
        if bal:
            mem.add("balance")
            queue = False                                           # plan_balance: the plan carries no queue
            if sw["range_stream"] != "0":                           # launch_poly, crc_kernels.hip:523
                return "range_stream", mem
        return _kernel(n, segs, grid, segs == 1, queue, bal, seg, pipe_max), mem
    mem.add("call")                                                 # run_record_jobs, hf3fs_crc_frame_verify_batch
    if entry == "frames":                                           # hf3fs_crc_frame_verify_batch, k_frame_map frame_kernels.hip:123
        try_stream = n >= 256 if sw["frame_stream"] == "auto" else sw["frame_stream"] != "0"
        if try_stream and shape["sorted_ok"] and shape["gap"] <= shape["pay"]:
            return "frame_stream", mem
    elif shape.get("runs_ok") and max_len >= (64 << 10) and n * max_len >= (1 << 30):  # run_record_jobs
        return "byte_runs", mem
    seg, segs, grid, pipe_max = _make_plan(cus, n, max_len, sw)
    m = shape["dev_max"]
    if m == 0:
        return "all_empty", mem                                     # crc_kernels.hip:395
    direct_t = segs == 1 and sw["record_direct"] != "0"             # launch_poly, crc_kernels.hip:533-534
    dsegs = -(-m // seg) if m > seg else 1                          # crc_kernels.hip:400
    queue = sw["static"] == "0"                                     # a device-side bound always asks for tickets (launch_prepare, run_ranges_list)
    return _kernel(n, dsegs, cus, direct_t or dsegs == 1, queue, False, m, pipe_max), mem  # grid = cus (run_ranges_list)


def expected_schedule(shape, cus, switches=None):
    """Which schedule of the hot kernel a launch takes: a plain restatement of make_plan,
    launch_prepare and plan_balance (hf3fs_crc_api.hip), the host branches of
    hf3fs_crc_create_batch, hf3fs_crc_create_strided and run_record_jobs (hf3fs_crc_api.hip), the
    frame route (hf3fs_crc_frame_verify_batch, frame_kernels.hip:105-127), launch_poly (crc_kernels.hip:520-539) and
    k_crc_ranges' own choices (crc_kernels.hip:391-434: tickets dropped for ntasks <= W or
    > 16 W, direct_pipe for len_bound <= pipe_max, direct || segs == 1).  Returns one of SCHEDULES;
    beside them "frame_stream" for a frame batch the stream path takes, "all_empty" for a record
    batch without bytes, and None for a call that never launches k_crc_ranges (file digest,
    combine, serialize, finalize).  `shape` is one element of a case's shapes().

    This is a model, written from the source lines it cites: it can drift from them.  The GPU
    test pins results, not schedules; a label that no longer matches says that the planner's
    thresholds moved and the shapes here need another look."""
    return _schedule(shape, cus, switches)[0]


def library_memory(shape, cus, switches=None):
    """The kinds of library memory the launch asks call_memory for (hf3fs_crc_api.hip): a
    subset of {"verify", "call", "balance", "counter"}.  A captured call owns one graph buffer per
    kind (small ones share a slab).  Same caveat as expected_schedule."""
    return _schedule(shape, cus, switches)[1]


def case_label(case, inp, cus, switches=None):
    """The case's launches joined with '+' (most cases have one)."""
    return "+".join(str(expected_schedule(s, cus, switches)) for s in case.shapes(inp))


# ---- switches -------------------------------------------------------------------------------------
_LIST = ["create_list_ragged", "create_list_small_many", "create_list_small_many_balanced", "create_list_ticketed"]
_VLIST = ["verify_batch_scratch", "verify_batch_given"]
_VSTRIDED = ["verify_strided_scratch", "verify_strided_given"]
_VBLOCKS = ["verify_blocks_scratch", "verify_blocks_given"]
_RECORD = ["read_result", "scrub", "frames_gaps"]
_FRAMES = ["frames_walked", "frames_gaps", "frames_big"]
_RANGES = _LIST + ["create_strided"] + _VLIST + _VSTRIDED + _VBLOCKS + _RECORD

# (name, value) pairs set together -> the cases the row applies to, and where the code reads the switch
SWITCHES = {
    (("nt", "0"),): dict(cases=_RANGES, source="hf3fs_crc_api.hip make_plan, crc_kernels.hip launch_poly"),
    (("static", "1"),): dict(cases=_LIST + _VLIST + _VBLOCKS + _RECORD, source="hf3fs_crc_api.hip tickets_allowed"),
    (("seg_kib", "1"),): dict(cases=_RANGES, source="hf3fs_crc_api.hip make_plan"),
    (("seg_kib", "4"),): dict(cases=_RANGES, source="hf3fs_crc_api.hip make_plan"),
    (("seg_kib", "64"),): dict(cases=_RANGES, source="hf3fs_crc_api.hip make_plan"),
    (("balance", "0"),): dict(cases=["create_list_small_many_balanced"] + _VBLOCKS,
                              source="hf3fs_crc_api.hip plan_balance"),
    (("record_direct", "0"),): dict(cases=_RECORD, source="crc_kernels.hip launch_poly"),
    (("pipe", "0"),): dict(cases=_RANGES, source="hf3fs_crc_api.hip make_plan"),
    (("pipe", "1"),): dict(cases=_RANGES, source="hf3fs_crc_api.hip make_plan"),
    (("range_stream", "1"),): dict(cases=["create_list_small_many_balanced"] + _VBLOCKS,
                                   source="hf3fs_crc_api.hip make_plan and plan_balance, crc_kernels.hip launch_poly"),
    (("list_runs", "1"), ("prehash_rep", "1")): dict(cases=_LIST + _VLIST, source="hf3fs_crc_api.hip hf3fs_crc_create_batch"),
    (("list_runs", "1"), ("prehash_rep", "8")): dict(cases=_LIST + _VLIST, source="hf3fs_crc_api.hip hf3fs_crc_create_batch"),
    (("frame_stream", "0"), ("frame_segw", "1")): dict(cases=_FRAMES, source="hf3fs_crc_api.hip hf3fs_crc_frame_verify_batch"),
    (("frame_stream", "0"), ("frame_segw", "64")): dict(cases=_FRAMES, source="hf3fs_crc_api.hip hf3fs_crc_frame_verify_batch"),
    (("frame_stream", "1"), ("frame_segw", "1")): dict(cases=_FRAMES, source="hf3fs_crc_api.hip hf3fs_crc_frame_verify_batch"),
    (("frame_stream", "1"), ("frame_segw", "64")): dict(cases=_FRAMES, source="hf3fs_crc_api.hip hf3fs_crc_frame_verify_batch"),
}

# Switches this file does not cover, and the tests that do.
EXEMPT = {
    "update_pipeline": "update path: test_gpu_parity.py::test_update_batch_vs_replica_oracle (fused / unfused on every mode)",
    "apply_pieces": "update path: test_gpu_parity.py::test_update_batch_vs_replica_oracle[unfused_fine], "
                    "test_gpu_update_footprint.py::test_footprint_every_variant",
    "apply_min_kib": "update path: test_gpu_parity.py::test_update_batch_vs_replica_oracle[unfused_fine]",
    "apply_nt": "update path: test_gpu_update_footprint.py::test_footprint_every_variant",
    "apply_grid": "update path: test_gpu_parity.py::test_update_batch_vs_replica_oracle[oneshot_loop], "
                  "test_update_one_shot_hint_across_release_stream",
    "apply_piece_kib": "update path: test_gpu_parity.py::test_update_batch_vs_replica_oracle[oneshot16]",
    "audit": "update path: test_gpu_parity.py::test_update_audit_contradicts_wrong_verdict",
    "fault_io": "update path: test_gpu_parity.py::test_update_audit_contradicts_wrong_verdict",
    "debug": "diagnostics on stderr of the update pipeline; changes no result",
    "poison": "a context of test_gpu_batch_contexts.py (test_poisoned_scratch, test_captured_replay), not a switch row",
}


def switch_key(row):
    return ",".join(f"{k}={v}" for k, v in row) or "default"


# The schedule every (case, switch row) takes on a 256-CU device, launches joined with '+'.  The
# GPU test asserts expected_schedule at the device's CU count against these, so a shape that
# slips to another schedule -- or a planner threshold that moves -- fails there.  Rows a switch
# does not apply to are absent.
LABELS = {
    ("create_list_ragged", "default"): "segmented_static+segmented_static",
    ("create_list_ragged", "nt=0"): "segmented_static+segmented_static",
    ("create_list_ragged", "static=1"): "segmented_static+segmented_static",
    ("create_list_ragged", "seg_kib=1"): "segmented_ticketed+segmented_ticketed",
    ("create_list_ragged", "seg_kib=4"): "segmented_ticketed+segmented_ticketed",
    ("create_list_ragged", "seg_kib=64"): "segmented_static+segmented_static",
    ("create_list_ragged", "pipe=0"): "segmented_static+segmented_static",
    ("create_list_ragged", "pipe=1"): "segmented_static+segmented_static",
    ("create_list_ragged", "list_runs=1,prehash_rep=1"): "byte_runs+byte_runs",
    ("create_list_ragged", "list_runs=1,prehash_rep=8"): "byte_runs_rep+byte_runs_rep",
    ("create_list_small_many", "default"): "direct_pipe",
    ("create_list_small_many", "nt=0"): "direct_pipe",
    ("create_list_small_many", "static=1"): "direct_pipe",
    ("create_list_small_many", "seg_kib=1"): "direct_pipe",
    ("create_list_small_many", "seg_kib=4"): "direct_pipe",
    ("create_list_small_many", "seg_kib=64"): "direct_pipe",
    ("create_list_small_many", "pipe=0"): "balanced",
    ("create_list_small_many", "pipe=1"): "direct_pipe",
    ("create_list_small_many", "list_runs=1,prehash_rep=1"): "byte_runs",
    ("create_list_small_many", "list_runs=1,prehash_rep=8"): "byte_runs_rep",
    ("create_list_small_many_balanced", "default"): "balanced",
    ("create_list_small_many_balanced", "nt=0"): "balanced",
    ("create_list_small_many_balanced", "static=1"): "balanced",
    ("create_list_small_many_balanced", "seg_kib=1"): "segmented_static",
    ("create_list_small_many_balanced", "seg_kib=4"): "segmented_static",
    ("create_list_small_many_balanced", "seg_kib=64"): "balanced",
    ("create_list_small_many_balanced", "balance=0"): "direct_static",
    ("create_list_small_many_balanced", "pipe=0"): "balanced",
    ("create_list_small_many_balanced", "pipe=1"): "direct_pipe",
    ("create_list_small_many_balanced", "range_stream=1"): "range_stream",
    ("create_list_small_many_balanced", "list_runs=1,prehash_rep=1"): "byte_runs",
    ("create_list_small_many_balanced", "list_runs=1,prehash_rep=8"): "byte_runs_rep",
    ("create_list_ticketed", "default"): "direct_ticketed",
    ("create_list_ticketed", "nt=0"): "direct_ticketed",
    ("create_list_ticketed", "static=1"): "direct_pipe",
    ("create_list_ticketed", "seg_kib=1"): "segmented_ticketed",
    ("create_list_ticketed", "seg_kib=4"): "direct_ticketed",
    ("create_list_ticketed", "seg_kib=64"): "direct_ticketed",
    ("create_list_ticketed", "pipe=0"): "direct_ticketed",
    ("create_list_ticketed", "pipe=1"): "direct_ticketed",
    ("create_list_ticketed", "list_runs=1,prehash_rep=1"): "byte_runs",
    ("create_list_ticketed", "list_runs=1,prehash_rep=8"): "byte_runs_rep",
    ("create_strided", "default"): "segmented_static+direct_pipe+direct_pipe",
    ("create_strided", "nt=0"): "segmented_static+direct_pipe+direct_pipe",
    ("create_strided", "seg_kib=1"): "segmented_static+direct_pipe+direct_pipe",
    ("create_strided", "seg_kib=4"): "segmented_static+direct_pipe+direct_pipe",
    ("create_strided", "seg_kib=64"): "segmented_static+direct_pipe+direct_pipe",
    ("create_strided", "pipe=0"): "segmented_static+direct_static+direct_static",
    ("create_strided", "pipe=1"): "segmented_static+direct_pipe+direct_pipe",
    ("verify_batch_scratch", "default"): "direct_ticketed",
    ("verify_batch_scratch", "nt=0"): "direct_ticketed",
    ("verify_batch_scratch", "static=1"): "direct_pipe",
    ("verify_batch_scratch", "seg_kib=1"): "segmented_ticketed",
    ("verify_batch_scratch", "seg_kib=4"): "direct_ticketed",
    ("verify_batch_scratch", "seg_kib=64"): "direct_ticketed",
    ("verify_batch_scratch", "pipe=0"): "direct_ticketed",
    ("verify_batch_scratch", "pipe=1"): "direct_ticketed",
    ("verify_batch_scratch", "list_runs=1,prehash_rep=1"): "byte_runs",
    ("verify_batch_scratch", "list_runs=1,prehash_rep=8"): "byte_runs_rep",
    ("verify_batch_given", "default"): "direct_ticketed",
    ("verify_batch_given", "nt=0"): "direct_ticketed",
    ("verify_batch_given", "static=1"): "direct_pipe",
    ("verify_batch_given", "seg_kib=1"): "segmented_ticketed",
    ("verify_batch_given", "seg_kib=4"): "direct_ticketed",
    ("verify_batch_given", "seg_kib=64"): "direct_ticketed",
    ("verify_batch_given", "pipe=0"): "direct_ticketed",
    ("verify_batch_given", "pipe=1"): "direct_ticketed",
    ("verify_batch_given", "list_runs=1,prehash_rep=1"): "byte_runs",
    ("verify_batch_given", "list_runs=1,prehash_rep=8"): "byte_runs_rep",
    ("verify_strided_scratch", "default"): "segmented_static",
    ("verify_strided_scratch", "nt=0"): "segmented_static",
    ("verify_strided_scratch", "seg_kib=1"): "segmented_static",
    ("verify_strided_scratch", "seg_kib=4"): "segmented_static",
    ("verify_strided_scratch", "seg_kib=64"): "segmented_static",
    ("verify_strided_scratch", "pipe=0"): "segmented_static",
    ("verify_strided_scratch", "pipe=1"): "segmented_static",
    ("verify_strided_given", "default"): "segmented_static",
    ("verify_strided_given", "nt=0"): "segmented_static",
    ("verify_strided_given", "seg_kib=1"): "segmented_static",
    ("verify_strided_given", "seg_kib=4"): "segmented_static",
    ("verify_strided_given", "seg_kib=64"): "segmented_static",
    ("verify_strided_given", "pipe=0"): "segmented_static",
    ("verify_strided_given", "pipe=1"): "segmented_static",
    ("verify_blocks_scratch", "default"): "balanced",
    ("verify_blocks_scratch", "nt=0"): "balanced",
    ("verify_blocks_scratch", "static=1"): "balanced",
    ("verify_blocks_scratch", "seg_kib=1"): "segmented_static",
    ("verify_blocks_scratch", "seg_kib=4"): "segmented_static",
    ("verify_blocks_scratch", "seg_kib=64"): "balanced",
    ("verify_blocks_scratch", "balance=0"): "direct_static",
    ("verify_blocks_scratch", "pipe=0"): "balanced",
    ("verify_blocks_scratch", "pipe=1"): "direct_pipe",
    ("verify_blocks_scratch", "range_stream=1"): "range_stream",
    ("verify_blocks_given", "default"): "balanced",
    ("verify_blocks_given", "nt=0"): "balanced",
    ("verify_blocks_given", "static=1"): "balanced",
    ("verify_blocks_given", "seg_kib=1"): "segmented_static",
    ("verify_blocks_given", "seg_kib=4"): "segmented_static",
    ("verify_blocks_given", "seg_kib=64"): "balanced",
    ("verify_blocks_given", "balance=0"): "direct_static",
    ("verify_blocks_given", "pipe=0"): "balanced",
    ("verify_blocks_given", "pipe=1"): "direct_pipe",
    ("verify_blocks_given", "range_stream=1"): "range_stream",
    ("read_result", "default"): "segmented_static",
    ("read_result", "nt=0"): "segmented_static",
    ("read_result", "static=1"): "segmented_static",
    ("read_result", "seg_kib=1"): "segmented_ticketed",
    ("read_result", "seg_kib=4"): "segmented_ticketed",
    ("read_result", "seg_kib=64"): "segmented_static",
    ("read_result", "record_direct=0"): "segmented_static",
    ("read_result", "pipe=0"): "segmented_static",
    ("read_result", "pipe=1"): "segmented_static",
    ("scrub", "default"): "segmented_static",
    ("scrub", "nt=0"): "segmented_static",
    ("scrub", "static=1"): "segmented_static",
    ("scrub", "seg_kib=1"): "segmented_ticketed",
    ("scrub", "seg_kib=4"): "segmented_ticketed",
    ("scrub", "seg_kib=64"): "segmented_static",
    ("scrub", "record_direct=0"): "segmented_static",
    ("scrub", "pipe=0"): "segmented_static",
    ("scrub", "pipe=1"): "segmented_static",
    ("frames_walked", "default"): "frame_stream",
    ("frames_walked", "frame_stream=0,frame_segw=1"): "direct_pipe",
    ("frames_walked", "frame_stream=0,frame_segw=64"): "direct_pipe",
    ("frames_walked", "frame_stream=1,frame_segw=1"): "frame_stream",
    ("frames_walked", "frame_stream=1,frame_segw=64"): "frame_stream",
    ("frames_gaps", "default"): "direct_pipe",
    ("frames_gaps", "nt=0"): "direct_pipe",
    ("frames_gaps", "static=1"): "direct_pipe",
    ("frames_gaps", "seg_kib=1"): "segmented_static",
    ("frames_gaps", "seg_kib=4"): "segmented_static",
    ("frames_gaps", "seg_kib=64"): "direct_pipe",
    ("frames_gaps", "record_direct=0"): "direct_pipe",
    ("frames_gaps", "pipe=0"): "direct_static",
    ("frames_gaps", "pipe=1"): "direct_pipe",
    ("frames_gaps", "frame_stream=0,frame_segw=1"): "direct_pipe",
    ("frames_gaps", "frame_stream=0,frame_segw=64"): "direct_pipe",
    ("frames_gaps", "frame_stream=1,frame_segw=1"): "direct_pipe",
    ("frames_gaps", "frame_stream=1,frame_segw=64"): "direct_pipe",
    ("frames_big", "default"): "frame_stream",
    ("frames_big", "frame_stream=0,frame_segw=1"): "segmented_static",
    ("frames_big", "frame_stream=0,frame_segw=64"): "segmented_static",
    ("frames_big", "frame_stream=1,frame_segw=1"): "frame_stream",
    ("frames_big", "frame_stream=1,frame_segw=64"): "frame_stream",
    ("file_digest_fill_zero", "default"): "None",
    ("file_digest_strict", "default"): "None",
    ("combine", "default"): "None",
    ("serialize", "default"): "None",
    ("finalize", "default"): "None",
}
