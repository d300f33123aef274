"""hf3fs_crc_md5_batch without a GPU: the pure-Python model of tests/md5_cases.py against hashlib
(it is what tests/test_gpu_md5.py checks the calls without FINAL against), the ABI structs, the
host helper hf3fs_crc_md5_hex, and every argument error, which the call answers before it touches
a device."""
import ctypes
import hashlib
import re

import numpy as np
import pytest

import md5_cases as mc


# ---- the model -----------------------------------------------------------------------------------
def test_model_rfc1321_vectors():
    for text, want in mc.RFC1321:
        assert hashlib.md5(text).hexdigest() == want
        assert mc.State().update(text).digest().hex() == want


def test_model_every_length_to_200():
    data = np.random.default_rng(1).integers(0, 256, 200, dtype=np.uint8).tobytes()
    for n in range(201):
        s = mc.State().update(data[:n])
        assert s.total == n and s.tail == data[n // 64 * 64:n]
        assert s.digest() == hashlib.md5(data[:n]).digest(), n


def test_model_random_cuts_and_pack():
    rng = np.random.default_rng(2)
    for _ in range(200):
        data = rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8).tobytes()
        cuts = sorted(int(x) for x in rng.integers(0, len(data) + 1, int(rng.integers(0, 5))))
        s = mc.State()
        for a, b in zip([0] + cuts, cuts + [len(data)]):
            s = mc.State.unpack(s.update(data[a:b]).pack())  # through the 96-byte form
        assert s.digest() == hashlib.md5(data).digest()
        raw = s.pack()
        assert len(raw) == 96 and raw[24 + s.total % 64:] == bytes(72 - s.total % 64)


def test_model_prefix_states():
    data = np.random.default_rng(3).integers(0, 256, 150, dtype=np.uint8).tobytes()
    states = mc.prefix_states(data)
    assert len(states) == 151
    for k in (0, 1, 63, 64, 65, 128, 150):
        assert states[k].pack() == mc.State().update(data[:k]).pack()


def test_layouts_describe_their_contents():
    """The case builders: segments lie inside the arena between junk, files are what they say."""
    for lay in (mc.rfc_layout(), mc.sweep_layout(), mc.segmentation_layout(), mc.holes_layout(), mc.ragged_layout(65)):
        arena = lay.arena()
        segs, off = mc.records(lay.files, 0x10000)
        assert off[-1] == segs.size and (np.diff(off.astype(np.int64)) >= 0).all()
        for o, n in (s for f in lay.files for s in f):
            assert o is None or (mc.SLACK <= o and o + n <= arena.size - mc.SLACK)
    lay = mc.sweep_layout()
    got = mc.contents(lay.arena(), lay.files)
    assert [len(c) for c in got[:len(mc.SWEEP_LENGTHS)]] == mc.SWEEP_LENGTHS
    assert sorted({lay.files[i][0][0] % 16 for i in range(16)}) == list(range(16))
    lay = mc.segmentation_layout()
    assert len(set(mc.contents(lay.arena(), lay.files))) == 1 and len(lay.files) == 301 + 120
    lay = mc.holes_layout()
    assert any(c == bytes(5000) for c in mc.contents(lay.arena(), lay.files))
    lay = mc.ragged_layout(200)
    sizes = [sum(n for _, n in f) for f in lay.files]
    assert max(sizes) == (1 << 20) + 17 and sizes.count(0) >= 10 and max(len(f) for f in lay.files) == 8


# ---- ABI -------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(hf):
    L = hf._lib
    assert L.md5_seg_dtype() == mc.SEG and L.md5_state_dtype() == mc.STATE
    assert mc.SEG.itemsize == 16 and mc.STATE.itemsize == 96
    assert [mc.SEG.fields[k][1] for k in ("data", "length")] == [0, 8]
    assert [mc.STATE.fields[k][1] for k in ("h", "total", "tail", "reserved")] == [0, 16, 24, 88]
    text = open(L.HEADER).read()
    seg = re.search(r"typedef struct hf3fs_crc_md5_seg \{(.*?)\}", text, re.S).group(1)
    state = re.search(r"typedef struct hf3fs_crc_md5_state \{(.*?)\}", text, re.S).group(1)
    strip = lambda body: re.findall(r"(uint\d+_t)\s+(\w+)(?:\[(\d+)\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))  # noqa: E731
    assert strip(seg) == [("uint64_t", "data", ""), ("uint64_t", "length", "")]
    assert strip(state) == [("uint32_t", "h", "4"), ("uint64_t", "total", ""), ("uint8_t", "tail", "64"),
                            ("uint64_t", "reserved", "")]
    assert (hf.MD5_INIT, hf.MD5_FINAL) == (1, 2) == (mc.INIT, mc.FINAL)
    assert re.search(r"HF3FS_MD5_INIT = 1, HF3FS_MD5_FINAL = 2", text)


def test_md5_hex(hf):
    for text, want in mc.RFC1321:
        assert hf.md5_hex(hashlib.md5(text).digest()) == want
    assert hf.md5_hex(bytes(range(0, 256, 17))[:16]) == bytes(range(0, 256, 17))[:16].hex()
    out = ctypes.create_string_buffer(b"\x7f" * 40, 40)
    assert hf._lib.load().hf3fs_crc_md5_hex(ctypes.create_string_buffer(bytes(16), 16), out) == 32
    assert out.raw == b"0" * 32 + b"\x7f" * 8  # no terminator, nothing behind the 32 characters
    with pytest.raises(ValueError):
        hf.md5_hex(b"short")


def test_argument_errors_before_any_device(hf):
    """Every error of the header's list is kInvalidArg through the raw call (this machine may have
    no GPU: a call that reached a device would answer DEVICE_ERROR), n_files == 0 is OK."""
    lib = hf._lib.load()
    call = lib.hf3fs_crc_md5_batch
    segs = (ctypes.c_uint64 * 4)()
    off = (ctypes.c_uint64 * 3)(0, 1, 2)
    state = ctypes.create_string_buffer(2 * 96)
    out = ctypes.create_string_buffer(32)
    S, F, T, O = (ctypes.addressof(x) for x in (segs, off, state, out))
    both = mc.INIT | mc.FINAL
    assert call(None, None, 0, 0, None, None, 0, None) == hf.OK
    assert call(S, F, 0, 2, None, None, 0xFF, None) == hf.OK
    bad = {
        "null d_file_off": (S, None, 2, 2, T, O, both),
        "n_segs > 0 with null d_segs": (None, F, 2, 2, T, O, both),
        "unknown flag bit 4": (S, F, 2, 2, T, O, both | 4),
        "unknown flag bit 31": (S, F, 2, 2, T, O, 1 << 31),
        "null d_state with INIT only": (S, F, 2, 2, None, O, mc.INIT),
        "null d_state with FINAL only": (S, F, 2, 2, None, O, mc.FINAL),
        "null d_state with no flag": (S, F, 2, 2, None, O, 0),
        "FINAL with null d_out": (S, F, 2, 2, T, None, mc.FINAL),
        "INIT | FINAL with null d_out": (S, F, 2, 2, None, None, both),
        "n_files above 2^30": (S, F, (1 << 30) + 1, 2, T, O, both),
        "n_segs above 2^30": (S, F, 2, (1 << 30) + 1, T, O, both),
    }
    for what, args in bad.items():
        assert call(*args, None) == hf.INVALID_ARG, what
        assert lib.hf3fs_crc_last_error(), what
    assert state.raw == bytes(2 * 96) and out.raw == bytes(32)
    with pytest.raises(hf.Hf3fsCrcError) as e:
        hf.md5_batch(S, F, 2, 2, out=O, flags=mc.FINAL)
    assert e.value.code == hf.INVALID_ARG and "INIT | FINAL" in str(e.value)


def test_scratch_bytes_monotone_and_zero_when_rejected(hf):
    sizes = [0, 1, 63, 64, 65, 1000, 4096, 16384, 16385, 65536, 1 << 20, 1 << 24, 1 << 30]
    got = [hf.md5_scratch_bytes(n) for n in sizes]
    assert all(a <= b for a, b in zip(got, got[1:])) and got[1] > 0 and got[-1] >= 12 << 30
    assert got[sizes.index(65536)] < 2 << 20  # 12 bytes per file and a fixed table
    assert hf.md5_scratch_bytes((1 << 30) + 1) == 0 and hf.md5_scratch_bytes(1 << 40) == 0


def test_md5_options_accept_0_and_1_only(hf):
    L = hf._lib
    for name in ("md5_sort", "md5_stage"):
        before = L.get_option(name)
        assert before in ("0", "1")
        for v in ("0", "1"):
            with L.option(name, v):
                assert L.get_option(name) == v
        for v in ("2", "-1", "auto", ""):
            with pytest.raises(hf.Hf3fsCrcError) as e:
                L.set_option(name, v)
            assert e.value.code == hf.INVALID_ARG
        assert L.get_option(name) == before
    assert "md5_sort" in open(L.HEADER).read() and "md5_stage" in open(L.HEADER).read()
