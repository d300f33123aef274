"""hf3fs_crc_serialize_batch and hf3fs_crc_finalize_batch (aux_kernels.hip), which no other
test calls: every output record / value against the host codec and plain numpy, the output
inside a canary at an odd offset, and n on both sides of one workgroup and past the
4096 x 256 threads of the largest grid (the grid-stride loop)."""
import numpy as np
import pytest

import update_footprint as fp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF
SIZES = [0, 1, 255, 256, 257, (1 << 20) + 77]
GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _values(n, seed):
    v = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    for k, special in enumerate((0, M32, 0x80000000, 1)):
        if k < n:
            v[(k * 97) % n if n > 4 else k] = special
    return v


def _dev_u32(v, dev):
    return torch.from_numpy(v.view(np.int32).copy()).to(dev)


@pytest.mark.parametrize("ctype", [1, 2], ids=["crc32c", "crc32"])
@pytest.mark.parametrize("n", SIZES)
def test_serialize_batch_vs_host_codec(hf, dev, n, ctype):
    L = hf._lib
    v = _values(n, 11 * ctype + n % 1000)
    if n:
        assert 0 in v and (M32 in v or n < 2)
    lead = GUARD + 3  # an odd offset: the 6-byte records are never aligned
    host = fp.canary(lead + 6 * n + GUARD, 0x33)
    d_out = torch.from_numpy(host.copy()).to(dev)
    d_v = _dev_u32(v, dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
    L.serialize_batch(ctype, d_v, n, d_out.data_ptr() + lead, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert np.array_equal(got[:lead], host[:lead]), "canary before the records"
    assert np.array_equal(got[lead + 6 * n:], host[lead + 6 * n:]), "canary after the records"
    if n:
        assert np.array_equal(d_v.cpu().numpy().view(np.uint32), v), "the values are input only"
    recs = got[lead:lead + 6 * n].reshape(n, 6)
    # ChecksumInfo's serde form (hf3fs_checksum_serialize): 0x05, type, value little-endian
    want = np.empty((n, 6), dtype=np.uint8)
    want[:, 0], want[:, 1] = 5, ctype
    want[:, 2:] = v.astype("<u4").view(np.uint8).reshape(n, 4)
    bad = np.flatnonzero((recs != want).any(axis=1))
    assert bad.size == 0, (bad[:4], recs[bad[:4]], want[bad[:4]])
    # ... and that form is the host codec's, record by record (all of a small batch; of the large
    # one the first and last 300 and 600 spread over the grid-stride passes)
    idx = range(n) if n <= 600 else sorted(set(range(300)) | set(range(n - 300, n)) |
                                           set(int(i) for i in np.linspace(0, n - 1, 600)))
    for i in idx:
        assert recs[i].tobytes() == L.checksum_serialize(ctype, int(v[i])), i


@pytest.mark.parametrize("n", SIZES)
def test_finalize_batch_inverts_in_place(hf, dev, n):
    L = hf._lib
    v = _values(n, 5 + n % 1000)
    lead = GUARD + 4  # (uint32 values: 4-byte aligned, not 16)
    host = fp.canary(lead + 4 * n + GUARD, 0x77)
    host[lead:lead + 4 * n] = v.view(np.uint8)
    d = torch.from_numpy(host.copy()).to(dev)
    s = torch.cuda.current_stream()
    L.finalize_batch(d.data_ptr() + lead, n, stream=s)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(got[:lead], host[:lead]) and np.array_equal(got[lead + 4 * n:], host[lead + 4 * n:]), "canary"
    assert np.array_equal(got[lead:lead + 4 * n].view(np.uint32), ~v)  # fin = ~raw
    L.finalize_batch(d.data_ptr() + lead, n, stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), host)  # the map is its own inverse; canary still intact


def test_combine_fin_vs_checksuminfo_combine_on_complements(hf, orc):
    """crc32c_combine_fin(f1, f2, len) = ~combine(~f1, ~f2, len) with the oracle's
    ChecksumInfo::combine on raw values (raw = ~fin), and on real data: fin(A || B) from fin(A),
    fin(B).  For len == 0 the only second operand there is is fin("") = 0 (combine leaves the
    first unchanged: Common.h:184)."""
    L = hf._lib
    rng = np.random.default_rng(0xF1)
    lens = [0, 1, 2, 3, 4, 7, 8, 63, 64, 4096, (1 << 20) + 1, (1 << 32) + 5, (1 << 40) + 3]
    for k in range(400):
        a, b = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        ln = lens[k % len(lens)] if k % 2 else int(rng.integers(0, 1 << 24))
        if ln == 0:
            b = 0
        rc, (t, raw) = orc.combine((1, (~a) & M32), (1, (~b) & M32), ln)
        assert rc == 0 and t == 1
        assert L.crc32c_combine_fin(a, b, ln) == (~raw) & M32, (hex(a), hex(b), ln)
    for k in range(32):
        A = rng.integers(0, 256, int(rng.integers(0, 5000)), dtype=np.uint8).tobytes()
        B = rng.integers(0, 256, int(rng.integers(0, 5000)) if k else 0, dtype=np.uint8).tobytes()
        assert L.crc32c_combine_fin(orc.rs_crc32c(A), orc.rs_crc32c(B), len(B)) == orc.rs_crc32c(A + B), k
