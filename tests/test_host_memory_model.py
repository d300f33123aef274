"""The whole-image check of the batch cases (tests/host_memory.py, Case.output_mask in
tests/batch_cases.py) checked on the CPU.  The masks are compared with what include/hf3fs_crc.h
itself marks as outputs, every byte Case.extract reads must lie under them, and the checker is
run against a numpy stand-in for the library: a correct one passes, and one that writes a single
stray byte -- into an input, a reserved field, the arena, a front guard or just past
d_mismatch[n - 1] -- is flagged at the right place.  The GPU runs are in
tests/test_gpu_host_memory.py."""
import os
import re
import zlib

import numpy as np
import pytest

import batch_cases as bc
import host_memory as hm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 64   # the smallest device of test_batch_cases_model.py's budgets: the masks do not depend on it

# What the header gives to each call, restated by hand: whole output arrays by argument, record
# fields through _header_outputs below.  (buffer name of the case -> the header's argument)
WHOLE = {
    "create_list_ragged": {"out1": "d_out", "out2": "d_out"},
    "create_list_small_many": {"out1": "d_out"},
    "create_list_small_many_balanced": {"out1": "d_out"},
    "create_list_ticketed": {"out1": "d_out"},
    "create_strided": {"out0": "d_out", "out1": "d_out", "out2": "d_out"},
    "verify_batch_scratch": {"mismatch": "d_mismatch", "count": "d_mismatch_count"},
    "verify_batch_given": {"mismatch": "d_mismatch", "count": "d_mismatch_count", "computed": "d_computed"},
    "verify_strided_scratch": {"mismatch": "d_mismatch", "count": "d_mismatch_count"},
    "verify_strided_given": {"mismatch": "d_mismatch", "count": "d_mismatch_count", "computed": "d_computed"},
    "verify_blocks_scratch": {"mismatch": "d_mismatch", "count": "d_mismatch_count"},
    "verify_blocks_given": {"mismatch": "d_mismatch", "count": "d_mismatch_count", "computed": "d_computed"},
    "read_result": {},
    "scrub": {"count": "d_mismatch_count"},
    "frames_walked": {"count": "d_mismatch_count"},
    "frames_gaps": {"count": "d_mismatch_count"},
    "frames_big": {"count": "d_mismatch_count"},
    "file_digest_fill_zero": {"out": "d_out"},
    "file_digest_strict": {"out": "d_out"},
    "combine": {"acc": "d_acc"},
    "serialize": {"out": "d_out"},
    "finalize": {"values": "d_values"},
}
RECORDS = {"read_result": ("recs", "hf3fs_crc_read_io", bc.READ_DT), "scrub": ("recs", "hf3fs_crc_scrub_io", bc.SCRUB_DT),
           "frames_walked": ("frames", "hf3fs_crc_frame", bc.FRAME_DT), "frames_gaps": ("frames", "hf3fs_crc_frame", bc.FRAME_DT),
           "frames_big": ("frames", "hf3fs_crc_frame", bc.FRAME_DT)}


def _header_struct(name):
    """[(field, comment)] of `typedef struct name` in the header; a field after the line
    `/* outputs */` gets the comment "out: ..." too."""
    text = open(os.path.join(REPO, "include", "hf3fs_crc.h")).read()
    body = text[text.index(f"typedef struct {name} {{"):text.index(f"}} {name};")]
    fields, outputs = [], False
    for line in body.splitlines()[1:]:
        if re.match(r"\s*/\* outputs \*/", line):
            outputs = True
        m = re.match(r"\s*u?int\d+_t\s+(\w+)(\[\d+\])?;\s*(?:/\*\s*(.*))?", line)
        if m:
            fields.append((m.group(1), ("out: " if outputs else "") + (m.group(3) or "")))
    return fields


def _header_outputs(name):
    return [f for f, c in _header_struct(name) if c.startswith("out:") and not f.startswith("reserved")]


@pytest.fixture(scope="module")
def built():
    out = {}
    for name, case in bc.CASES.items():
        inp = case.build(CUS, np.random.default_rng(zlib.crc32(name.encode())))
        out[name] = (inp, case.reference(inp))
    return out


def test_header_marks_the_record_outputs(hf):
    assert _header_outputs("hf3fs_crc_read_io") == ["out_checksum", "out_checksum_type", "status"]
    assert _header_outputs("hf3fs_crc_scrub_io") == ["computed", "status"]
    assert _header_outputs("hf3fs_crc_frame") == ["computed", "status"]
    L = hf._lib
    for dt, mirror in ((bc.READ_DT, L.ReadIO), (bc.SCRUB_DT, L.ScrubIO), (bc.FRAME_DT, L.Frame), (bc.FILE_DT, L.FileDigest)):
        for f, _ in mirror._fields_:
            if f in dt.names:
                assert dt.fields[f][1] == getattr(mirror, f).offset, (mirror.__name__, f)
    for case in bc.CASES.values():
        assert case.layouts.keys() <= case.buffers(case.build(CUS, np.random.default_rng(1)), 0).keys()


@pytest.mark.parametrize("name", list(bc.CASES))
def test_masks_are_the_headers_outputs(built, name):
    """Whole output arrays and the records' out fields, nothing else; every buffer has a mask; and
    every byte extract reads lies under it (inverting all other bytes leaves extract unchanged)."""
    case, (inp, _ref) = bc.CASES[name], built[name]
    images = case.buffers(inp, 0x7F0000000000)
    masks = case.output_mask(inp)
    assert masks.keys() == images.keys() and "arena" not in masks
    header = open(os.path.join(REPO, "include", "hf3fs_crc.h")).read()
    for k, a in images.items():
        want = np.zeros(a.nbytes, dtype=bool)
        if k in WHOLE[name]:
            assert re.search(r"[^t] \*?\*?" + WHOLE[name][k] + r"\b", header), WHOLE[name][k]  # (a non-const argument)
            want[:] = True
        elif name in RECORDS and RECORDS[name][0] == k:
            _, struct, dt = RECORDS[name]
            want = want.reshape(-1, dt.itemsize)
            for f in _header_outputs(struct):
                fdt, off = dt.fields[f][:2]
                want[:, off:off + fdt.itemsize] = True
            want = want.reshape(-1)
        assert np.array_equal(masks[k], want), (name, k)
    assert set(WHOLE[name]) | ({RECORDS[name][0]} if name in RECORDS else set()) == {k for k, m in masks.items() if m.any()}
    a = {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy() for k, v in images.items()}
    b = {k: np.where(masks[k], v, ~v) for k, v in a.items()}
    typed = (lambda d: {k: d[k].view(images[k].dtype) for k in d})
    ea, eb = case.extract(inp, typed(a)), case.extract(inp, typed(b))
    assert ea.keys() == eb.keys() and all(np.array_equal(ea[k], eb[k]) for k in ea), name


class StandIn:
    """The library as numpy: the reference's outputs stored into the images, then one stray byte."""

    def __init__(self, placed, ref, stray=None):
        self.placed, self.ref, self.stray = placed, ref, stray

    def run(self):
        pl = self.placed
        got = pl.fetch()
        pl.case.store(pl.inp, pl.host(got), self.ref)
        if self.stray:
            k, pos = self.stray
            got[k][pos] ^= 0x01
        return got


def _strays(pl):
    """[(kind, buffer, image offset, what the message must name)] for the placed case."""
    G, case, out = hm.GUARD, pl.case, []
    if "arena" in pl.sent:
        n = pl.sizes["arena"]
        out.append(("arena", "arena", G + n - 1, f"arena: offset {n - 1}"))
    for k in pl.dtypes:
        inside = pl.masks[k][G:G + pl.sizes[k]]
        dt = case.layouts.get(k)
        if not inside.all():   # an input array, or a record's input field
            off = int(np.flatnonzero(~inside)[-1])
            if dt is not None:
                f = bc.field_at(dt, off % dt.itemsize)
                out.append(("input", k, G + off, f"{k}: record {off // dt.itemsize} field {f}, offset {off}"))
                res = [f for f in dt.names if f.startswith("res")]
                if res:
                    off = 3 * dt.itemsize + dt.fields[res[0]][1]
                    out.append(("reserved", k, G + off, f"{k}: record 3 field {res[0]}, offset {off}"))
            else:
                out.append(("input", k, G + off, f"{k}: element {off // pl.dtypes[k].itemsize}, offset {off}"))
        if inside.any():
            out.append(("front_guard", k, G - 1, f"{k}: front guard, 1 B before the buffer"))
    if "mismatch" in pl.dtypes:
        n = pl.sizes["mismatch"]
        out.append(("past_mismatch", "mismatch", G + n, f"mismatch: back guard, 0 B past the buffer's {n} bytes"))
    return out


@pytest.mark.parametrize("name", list(bc.CASES))
def test_checker_passes_the_reference_and_names_every_stray_byte(built, name):
    case, (inp, ref) = bc.CASES[name], built[name]
    pl = hm.Placed(case, inp, hm.Plain)
    try:
        p = pl.pointers()
        assert all(v % 2 for k, v in p.items() if k != "arena" and pl.dtypes[k].itemsize == 1 and k not in case.layouts)
        assert "arena" not in inp or p["arena"] % 1024 == 0
        pl.check(StandIn(pl, ref).run(), ref, name)
        kinds = set()
        for kind, k, pos, words in _strays(pl):
            with pytest.raises(AssertionError) as e:
                pl.check(StandIn(pl, ref, (k, pos)).run(), ref, name)
            assert "stray write: 1 bytes" in str(e.value) and f"first at {words} (" in str(e.value), (kind, str(e.value))
            assert "output" not in str(e.value).split("stray write")[0], "the outputs were right"
            kinds.add(kind)
        has_input = any(not pl.masks[k][hm.GUARD:hm.GUARD + pl.sizes[k]].all() for k in pl.dtypes)
        assert "front_guard" in kinds and ("input" in kinds) == has_input
        assert has_input or name in ("finalize", "create_strided")  # (their only input is in place / the arena)
        if "arena" in inp:
            assert "arena" in kinds
        if case.mismatch and not case.records:
            assert "past_mismatch" in kinds
        if name in ("read_result", "scrub"):
            assert "reserved" in kinds
        wrong = {k: v.copy() for k, v in ref.items()}
        key = next(iter(wrong))
        wrong[key].reshape(-1)[0] ^= 1
        with pytest.raises(AssertionError, match=f"output {key} differs at 1 of"):
            pl.check(StandIn(pl, wrong).run(), ref, name)
    finally:
        pl.close()


def test_all_five_places_are_reached(built):
    kinds = set()
    for name in ("verify_batch_given", "read_result"):
        pl = hm.Placed(bc.CASES[name], built[name][0], hm.Plain)
        kinds |= {s[0] for s in _strays(pl)}
        pl.close()
    assert kinds == {"input", "reserved", "arena", "front_guard", "past_mismatch"}
