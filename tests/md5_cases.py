"""Cases and a model for hf3fs_crc_md5_batch, shared by tests/test_md5_model.py (the model against
hashlib), tests/test_md5_sanitized.py (the C++ core under ASan + UBSan) and tests/test_gpu_md5.py.

The checker of every digest is hashlib.md5.  hashlib does not expose its state, and the calls
without FINAL must be checked field by field, so `State` is a small pure-Python MD5 with the
explicit {h, total, tail} of hf3fs_crc_md5_state; tests/test_md5_model.py holds it to hashlib.

A case is a `Layout`: one arena of bytes and, per file, a list of segments (arena offset or hole,
length).  Payloads sit at chosen address residues with junk between them, so a kernel that reads a
neighbour's byte hashes something else.  Numpy only: no GPU, no torch.
"""
import hashlib
import math
import struct

import numpy as np

SEG = np.dtype([("data", "<u8"), ("length", "<u8")])
STATE = np.dtype([("h", "<u4", (4,)), ("total", "<u8"), ("tail", "u1", (64,)), ("reserved", "<u8")])
INIT, FINAL = 1, 2
SLACK = 64  # junk bytes before the first and behind the last payload of an arena

RFC1321 = [
    (b"", "d41d8cd98f00b204e9800998ecf8427e"),
    (b"a", "0cc175b9c0f1b6a831c399e269772661"),
    (b"abc", "900150983cd24fb0d6963f7d28e17f72"),
    (b"message digest", "f96b697d7cb7938d525a2f31aaf161d0"),
    (b"abcdefghijklmnopqrstuvwxyz", "c3fcd3d76192e4007dfb496cca67e13b"),
    (b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789", "d174ab98d277d9f5a5611c2c9f419d9f"),
    (b"1234567890" * 8, "57edf4a22be3c955ac49da2e2107b67a"),
]

_S = [7, 12, 17, 22] * 4 + [5, 9, 14, 20] * 4 + [4, 11, 16, 23] * 4 + [6, 10, 15, 21] * 4
_K = [int(abs(math.sin(i + 1)) * 2 ** 32) & 0xFFFFFFFF for i in range(64)]
_H0 = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476)
M32 = 0xFFFFFFFF


def _compress(h, block):
    w = struct.unpack("<16I", block)
    a, b, c, d = h
    for i in range(64):
        if i < 16:
            f, g = (b & c) | (~b & d), i
        elif i < 32:
            f, g = (d & b) | (~d & c), (5 * i + 1) % 16
        elif i < 48:
            f, g = b ^ c ^ d, (3 * i + 5) % 16
        else:
            f, g = c ^ (b | (~d & M32)), (7 * i) % 16
        f = (f + a + _K[i] + w[g]) & M32
        a, d, c = d, c, b
        b = (b + ((f << _S[i] | f >> (32 - _S[i])) & M32)) & M32
    return tuple((x + y) & M32 for x, y in zip(h, (a, b, c, d)))


class State:
    """MD5_CTX as hf3fs_crc_md5_state holds it: h, total and the total % 64 bytes not yet compressed."""

    def __init__(self, h=_H0, total=0, tail=b""):
        self.h, self.total, self.tail = tuple(h), total, bytes(tail)
        assert len(self.tail) == total % 64

    def update(self, data):
        buf = self.tail + bytes(data)
        h = self.h
        whole = len(buf) // 64 * 64
        for at in range(0, whole, 64):
            h = _compress(h, buf[at:at + 64])
        return State(h, self.total + len(data), buf[whole:])

    def digest(self):
        pad = b"\x80" + b"\0" * ((55 - self.total) % 64) + struct.pack("<Q", (self.total * 8) % 2 ** 64)
        end = State(self.h, self.total, self.tail).update(pad)
        assert not end.tail
        return struct.pack("<4I", *end.h)

    def pack(self):
        """The 96 bytes of hf3fs_crc_md5_state: the tail zero beyond total % 64, reserved 0."""
        return struct.pack("<4IQ", *self.h, self.total) + self.tail.ljust(64, b"\0") + bytes(8)

    @classmethod
    def unpack(cls, raw):
        h = struct.unpack_from("<4I", raw, 0)
        total, = struct.unpack_from("<Q", raw, 16)
        return cls(h, total, raw[24:24 + total % 64])


def prefix_states(content):
    """State after content[:k] for every k in 0 .. len(content), one pass."""
    out, s = [State()], State()
    for k in range(len(content)):
        s = s.update(content[k:k + 1])
        out.append(s)
    return out


def md5(data):
    return hashlib.md5(bytes(data)).digest()


# ---- layouts -------------------------------------------------------------------------------------
class Layout:
    """An arena under construction and the files whose segments point into it.

    put(payload, residue): the arena offset of a copy of payload whose offset is `residue` mod 16
    (the arena itself goes to a 16-byte aligned address), junk before it.
    A segment is (offset, length); offset None is a hole.  A file is a list of segments."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parts = [self.rng.integers(1, 256, SLACK, dtype=np.uint8)]
        self.size = SLACK
        self.files = []

    def put(self, payload, residue=None):
        payload = np.frombuffer(bytes(payload), dtype=np.uint8)
        if residue is None:
            residue = int(self.rng.integers(0, 16))
        gap = (residue - self.size) % 16 + 16 * int(self.rng.integers(0, 3))
        self.parts.append(self.rng.integers(1, 256, gap, dtype=np.uint8))
        at = self.size + gap
        self.parts.append(payload)
        self.size = at + payload.size
        assert at % 16 == residue
        return at

    def add_file(self, segments):
        self.files.append([(o, int(n)) for o, n in segments])
        return len(self.files) - 1

    def arena(self):
        a = np.concatenate(self.parts + [self.rng.integers(1, 256, SLACK, dtype=np.uint8)])
        assert a.size == self.size + SLACK
        return a


def records(files, base):
    """(segs, file_off): the hf3fs_crc_md5_seg records and the n_files + 1 offsets of `files` for an
    arena at address `base`."""
    n_segs = sum(len(f) for f in files)
    segs = np.zeros(max(n_segs, 1), dtype=SEG)
    off = np.zeros(len(files) + 1, dtype=np.uint64)
    k = 0
    for i, f in enumerate(files):
        for o, n in f:
            segs[k] = (0 if o is None else base + o, n)
            k += 1
        off[i + 1] = k
    return segs[:n_segs], off


def contents(arena, files):
    """The message of every file: its segments' bytes, holes as zeros."""
    raw = arena.tobytes()
    return [b"".join(bytes(n) if o is None else raw[o:o + n] for o, n in f) for f in files]


def cut(lay, payload, cuts, scatter=True):
    """payload as len(cuts) + 1 segments cut at the ascending positions `cuts`, each piece placed on
    its own (scattered) or all of them pointing into one copy."""
    edges = [0] + [int(c) for c in cuts] + [len(payload)]
    if scatter:
        return [(lay.put(payload[a:b]), b - a) for a, b in zip(edges, edges[1:])]
    at = lay.put(payload)
    return [(at + a, b - a) for a, b in zip(edges, edges[1:])]


# ---- the cases of tests/test_gpu_md5.py ---------------------------------------------------------------
SWEEP_LENGTHS = list(range(201)) + [1023, 1024, 1025, 4095, 4096, 4097]


def rfc_layout():
    lay = Layout(1321)
    for text, _ in RFC1321:
        lay.add_file([(lay.put(text), len(text))])
    return lay


def sweep_layout(seed=2):
    """One single-segment file per length of SWEEP_LENGTHS; file i sits at residue i mod 16, and the
    padding edge 55 / 56 / 63 / 64 / 119 / 120 also at every residue."""
    lay = Layout(seed)
    for i, n in enumerate(SWEEP_LENGTHS):
        lay.add_file([(lay.put(lay.rng.integers(0, 256, n, dtype=np.uint8), i % 16), n)])
    for n in (55, 56, 63, 64, 119, 120):
        for res in range(16):
            lay.add_file([(lay.put(lay.rng.integers(0, 256, n, dtype=np.uint8), res), n)])
    return lay


def segmentation_layout(seed=3):
    """300 bytes as two segments cut at every position 0 .. 300, then 120 files of three segments
    with random cuts (equal cuts: empty segments); every segment on its own at a random residue."""
    lay = Layout(seed)
    payload = lay.rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    for k in range(301):
        lay.add_file(cut(lay, payload, [k]))
    for i in range(120):
        a, b = sorted(int(x) for x in lay.rng.integers(0, 301, 2))
        if i % 10 == 0:
            b = a
        lay.add_file(cut(lay, payload, [a, b]))
    return lay


HOLES = (1, 63, 64, 65, 5000)


def holes_layout(seed=4):
    """Holes of every length of HOLES first, in the middle and last between payloads of 0 .. 150
    bytes, two holes in a row, and files that are one hole only."""
    lay = Layout(seed)
    for n in HOLES:
        for where in range(3):
            a = lay.rng.integers(0, 256, int(lay.rng.integers(0, 151)), dtype=np.uint8).tobytes()
            b = lay.rng.integers(0, 256, int(lay.rng.integers(1, 151)), dtype=np.uint8).tobytes()
            sa, sb, hole = (lay.put(a), len(a)), (lay.put(b), len(b)), (None, n)
            lay.add_file([[hole, sa, sb], [sa, hole, sb], [sa, sb, hole]][where])
        lay.add_file([(None, n)])
        lay.add_file([(None, n), (None, 64 - n % 64), (lay.put(b"x"), 1)])
    return lay


def ragged_layout(n_files, seed=6):
    """n_files files of 0 .. 100 KiB, about one in sixteen empty, file n_files // 2 of 1 MiB + 17
    bytes; each as up to eight segments (empty ones among them) placed on their own."""
    lay = Layout(seed * 1000 + n_files)
    for i in range(n_files):
        n = int(lay.rng.integers(0, (100 << 10) + 1))
        if i % 16 == 5:
            n = 0
        if i == n_files // 2:
            n = (1 << 20) + 17
        payload = lay.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        k = int(lay.rng.integers(0, 8)) if n else int(lay.rng.integers(0, 3))
        cuts = sorted(int(x) for x in lay.rng.integers(0, n + 1, k))
        lay.add_file(cut(lay, payload, cuts) if (n or k) else [])
    return lay


def stream_two_calls(n_bytes, seed=5):
    """One content of n_bytes split over two calls at every position 0 .. n_bytes: file k's first
    call brings content[:k], its second content[k:].  Both point into one copy of the content.
    -> (arena, content, files of call 1, files of call 2)"""
    lay = Layout(seed * 100000 + n_bytes)
    content = lay.rng.integers(0, 256, n_bytes, dtype=np.uint8).tobytes()
    at = lay.put(content, 5)
    first = [[(at, k)] for k in range(n_bytes + 1)]
    second = [[(at + k, n_bytes - k)] if k < n_bytes else [] for k in range(n_bytes + 1)]
    return lay.arena(), content, first, second


def stream_four_calls(n_bytes, n_files=48, seed=7):
    """One content split over four calls (INIT, none, none, FINAL) at three random ascending
    positions per file; equal positions give calls without bytes, and every fourth file's last call
    carries no segment.  -> (arena, content, [files of call 0 .. 3], cuts per file)"""
    lay = Layout(seed * 100000 + n_bytes)
    content = lay.rng.integers(0, 256, n_bytes, dtype=np.uint8).tobytes()
    at = lay.put(content, 11)
    calls, cuts = [[], [], [], []], []
    for i in range(n_files):
        c = sorted(int(x) for x in lay.rng.integers(0, n_bytes + 1, 3))
        if i % 4 == 0:
            c[2] = n_bytes
        if i % 6 == 1:
            c[1] = c[0]
        edges = [0] + c + [n_bytes]
        cuts.append(edges)
        for k in range(4):
            a, b = edges[k], edges[k + 1]
            if b > a:
                mid = (a + b) // 2  # two segments per call, so a call's bytes straddle a boundary too
                calls[k].append([(at + a, mid - a), (at + mid, b - mid)])
            else:
                calls[k].append([])
    return lay.arena(), content, calls, cuts
