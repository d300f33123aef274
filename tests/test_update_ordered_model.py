"""tests/ordered_cases.py checked on the CPU, and hf3fs_crc_update_ordered's argument checks
(they come before any device is touched).  The GPU runs are in tests/test_gpu_update_ordered.py."""
import numpy as np
import pytest

import ordered_cases as oc


@pytest.fixture(scope="module")
def built(orc):
    return {name: make() for name, make in oc.all_cases(orc).items()}


def test_cases_reproduce_from_their_seed(orc, built):
    for name, make in oc.all_cases(orc).items():
        a, b = built[name], make()
        assert a.rec.tobytes() == b.rec.tobytes(), name
        assert a.pay.tobytes() == b.pay.tobytes() and a.arena0.tobytes() == b.arena0.tobytes(), name
        assert a.expect == b.expect and a.arena1.tobytes() == b.arena1.tobytes(), name
        assert a.info == b.info, name


def _check_final(orc, b, state, chunks, name):
    for c, st in enumerate(state):
        size = st[0]
        if size == 0:
            continue  # (an empty chunk's stored value is the reference's 0, not a hash of no bytes)
        data = bytes(chunks[c][:size])
        if b.engine:
            assert st[1] == orc.rs_crc32c(data), (name, c)
        else:
            assert tuple(st[1]) == tuple(orc.create(st[1][0], data)), (name, c)


def test_final_checksums_match_final_bytes(orc, built):
    """After every case (and after its resubmission) each chunk's expected checksum is the
    oracle's create over the chunk's expected bytes: the sequential model keeps the invariant."""
    for name, b in built.items():
        _check_final(orc, b, b.state, b.final_chunks, name)
        if b.again is not None:
            _check_final(orc, b, b.again.state, b.again.final_chunks, name + " (resubmitted)")
            assert all(e[0] != oc.NOT_APPLIED for e in b.again.expect), name


def test_every_class_has_a_case(built):
    have = set()
    for b in built.values():
        have |= b.classes
    assert have == set(oc.CLASSES), sorted(set(oc.CLASSES) - have)
    # and the shapes the GPU tests name
    assert built["chains_512"].n == 64 and built["chains_512"].n_chunks == 8 and built["chains_512"].info == (12, 0)
    for ml in (512, 128 << 10):
        assert built[f"chains_{ml}"].classes >= {"overwrite", "append", "gap", "truncate", "extend", "full",
                                                  "none_write"}, ml
        assert built[f"failures_{ml}"].classes >= {"corrupt", "invalid", "after_failure"}, ml
        o = built[f"overflow_{ml}"]
        assert o.info == (5, 12) and o.again.n == 12
        assert built[f"distinct_{ml}_r1"].info == (1, 0) and built[f"distinct_{ml}_r1"].n == 64
    assert built["one_chunk"].info == (64, 0) and built["engine"].info == (17, 0)
    t = built["table_stress"]
    assert t.n == 4096 and t.info == (4, 0) and np.all(np.diff(t.bases) == 512)
    a, b = built["capture_a"], built["capture_b"]
    assert a.n == b.n == 64 and a.bases == b.bases and a.info[1] == b.info[1] == 0
    assert [op[0] for op in a.ops] != [op[0] for op in b.ops]


def test_later_ios_carry_junk_state(built):
    """Only a chunk's first IO holds the chunk's state in its record: the call must ignore (and
    overwrite) the three fields of every later one."""
    b = built["chains_512"]
    seen = set()
    for i, op in enumerate(b.ops):
        junk = (int(b.rec["chunk_size"][i]), int(b.rec["chunk_checksum_type"][i]),
                int(b.rec["chunk_checksum"][i])) == oc.JUNK
        assert junk == (op[0] in seen), i
        seen.add(op[0])


def test_update_ordered_argument_checks_need_no_device(hf):
    L = hf._lib.load()
    f = L.hf3fs_crc_update_ordered
    assert f(hf.CRC32C, None, 4, 512, hf.MODE_DELTA, 0, None, None) == hf.INVALID_ARG
    assert f(hf.CRC32C, None, 4, 512, hf.MODE_DELTA, 65, None, None) == hf.INVALID_ARG
    assert f(7, None, 4, 512, hf.MODE_DELTA, 4, None, None) == hf.INVALID_ARG
    assert f(hf.CRC32C, None, 4, 512, 2, 4, None, None) == hf.INVALID_ARG
    assert f(hf.CRC32C, None, 0, 512, hf.MODE_REFERENCE, 4, None, None) == hf.OK
    assert hf.NOT_APPLIED == 9002 and hf._lib.NOT_APPLIED == oc.NOT_APPLIED
    with pytest.raises(hf.Hf3fsCrcError):
        hf.update_ordered(hf.CRC32C, None, 4, 512, 0)
    assert hf.update_ordered(hf.CRC32C, None, 0, 512, 64) == hf.OK
