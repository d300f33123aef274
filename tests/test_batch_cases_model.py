"""The batch cases (tests/batch_cases.py) checked on the CPU: every switch of the library is
either a row of SWITCHES or exempt with a reason, the cases reach every schedule of the hot
kernel on a 256-CU device, each mutation really changes what the oracle expects, no reference
is trivial, and the cases stay inside their byte budget at 64, 256 and 304 CUs.  The GPU runs
of the same cases are in tests/test_gpu_batch_contexts.py."""
import os
import re

import numpy as np
import pytest

import batch_cases as bc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256


def _header_names():
    """The names of the header comment's "Names:" list, plus the two test-only switches."""
    text = open(os.path.join(REPO, "include", "hf3fs_crc.h")).read()
    body = text[text.index("Names:") + len("Names:"):text.index("Test only")]
    body = re.sub(r"\([^)]*\)", "", body.replace("\n *", " "))
    names = [w.strip(" .") for w in body.split(",")]
    assert all(re.fullmatch(r"[a-z_]+", w) for w in names), names
    return names + ["poison", "fault_io"]


@pytest.fixture(scope="module")
def built():
    """Every case's inputs and reference at 256 CUs, then after each mutation in turn."""
    out = {}
    for name, case in bc.CASES.items():
        rng = np.random.default_rng(7)
        inp = case.build(CUS, rng)
        refs = [case.reference(inp)]
        for _mname, fn in case.mutations:
            fn(inp, rng)
            refs.append(case.reference(inp))
        out[name] = (case.build(CUS, np.random.default_rng(7)), refs)
    return out


def test_every_switch_is_covered_or_exempt(hf):
    """A switch added to options.cc without a row here (or a reason) fails: get_option knows every
    name of the header's list, options.cc's table has no name the header lacks, and each name is
    in SWITCHES or in EXEMPT, never in both."""
    L = hf._lib
    names = _header_names()
    for name in names:
        L.get_option(name)  # raises on a name the library does not know
    table = re.findall(r'^\s*\{"([a-z_]+)",', open(os.path.join(REPO, "3fs_amd", "csrc", "options.cc")).read(), re.M)
    assert sorted(table) == sorted(names), "the header's Names list and options.cc's table differ"
    covered = {k for row in bc.SWITCHES for k, _ in row}
    for name in names:
        assert (name in covered) != (name in bc.EXEMPT), f"switch {name}: a row of SWITCHES or a reason in EXEMPT"
    assert covered | set(bc.EXEMPT) == set(names), "a row or an exemption names a switch the library does not have"
    for row, spec in bc.SWITCHES.items():
        cited = re.findall(r"(\w+\.(?:hip|h|cc)) (\w+)", spec["source"])  # file and function, no line numbers
        assert spec["cases"] and set(spec["cases"]) <= set(bc.CASES) and cited, row
        for unit, function in cited:
            assert function in open(os.path.join(REPO, "3fs_amd", "csrc", unit)).read(), (row, unit, function)
        assert any(v != bc.DEFAULTS[k] for k, v in row), f"{row} sets nothing"
    for k, v in bc.DEFAULTS.items():
        assert L.get_option(k) == v, f"the model's default of {k}"


def test_every_schedule_reached_at_256_cus(built):
    """The union of expected_schedule over cases x applicable switch rows holds every schedule, and
    the table of declared labels is that union exactly."""
    reached = {}
    for name, case in bc.CASES.items():
        inp = built[name][0]
        for row in [()] + list(bc.SWITCHES):
            if row and name not in bc.SWITCHES[row]["cases"]:
                continue
            label = bc.case_label(case, inp, CUS, dict(row))
            assert bc.LABELS[(name, bc.switch_key(row))] == label, (name, row)
            for part in label.split("+"):
                reached.setdefault(part, []).append((name, bc.switch_key(row)))
    listing = "\n".join(f"{lab}: {reached.get(lab, [])}" for lab in bc.SCHEDULES)
    assert all(reached.get(lab) for lab in bc.SCHEDULES), listing
    n_rows = sum(len(s["cases"]) for s in bc.SWITCHES.values()) + len(bc.CASES)
    assert len(bc.LABELS) == n_rows
    # the frame cases take both routes, and the poisoned-scratch context has its cases
    assert "frame_stream" in reached and any(c.poisoned for c in bc.CASES.values())


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_mutations_change_the_reference(built, name):
    case = bc.CASES[name]
    refs = built[name][1]
    assert len(refs) == len(case.mutations) + 1 and case.mutations
    for k, (mname, _fn) in enumerate(case.mutations):
        assert not _same(refs[k], refs[k + 1]), f"mutation {mname} leaves the reference as it was"
        assert all(refs[k][key].shape == refs[k + 1][key].shape for key in refs[k]), mname


@pytest.mark.parametrize("name", list(bc.CASES))
def test_reference_is_not_trivial(built, name):
    case = bc.CASES[name]
    ref = built[name][1][0]
    for key, v in ref.items():
        if key != "count":
            assert np.unique(v).size > 1, f"{name}.{key} is a constant vector"
    if case.mismatch:
        flags = ref["mismatch"] if "mismatch" in ref else ref["status"]
        assert np.count_nonzero(flags) >= 1 and np.count_nonzero(flags == 0) >= 1
        if "count" in ref:
            assert int(ref["count"][0]) == np.count_nonzero(flags)
    if name == "read_result":
        assert bc.CHECKSUM_MISMATCH in ref["status"] and bc.NONE in ref["type"] and bc.CRC32C in ref["type"]
    if name == "scrub":
        assert {bc.OK, bc.INVALID_ARG, bc.CHECKSUM_MISMATCH} <= set(ref["status"].tolist())
    if name == "frames_gaps":
        assert bc.INVALID_ARG in ref["status"]
    if name.startswith("file_digest"):
        want = {0, 3, 4080} if case.fill_zero else {0, 3, 4080, 7007, 33}
        assert want <= set(ref["status"].tolist()), set(ref["status"].tolist())


def test_shapes_reach_their_edges(built):
    """What the cases promise about their own inputs: every base residue mod 16, the grid
    alignment's residues mod 128, and the whole-buffer branch's spill ranges."""
    inp = built["create_list_ragged"][0]
    assert set((inp["offs"] % 16).tolist()) == set(range(16))
    assert {0, 1, 112, 124, 125, 126, 127} <= set((inp["offs"] % 128).tolist())
    for name in ("create_list_ragged", "create_list_ticketed"):
        inp = built[name][0]
        a0, ln = inp["offs"].astype(np.int64), inp["lens"].astype(np.int64)  # (the arena is 1 KiB aligned)
        vend = (a0 + ln + 15) // 16 * 16
        nb = -(-(vend - a0 // 16 * 16) // 1024)
        spill = (ln >= 4) & (a0 - (vend - nb * 1024) > 1020)
        assert np.count_nonzero(spill) >= 3, name
    f = built["frames_gaps"][0]["frames"]
    assert f["size"][0] == 0 and f["size"][-1] == 0 and int(f["offset"][0]) == 5 + 8
    assert built["frames_walked"][0]["frames"].size >= 256


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_byte_budgets(cus):
    for name, case in bc.CASES.items():
        for scale in (1, 2):
            inp = case.build(cus, np.random.default_rng(3), scale)
            assert case.device_bytes(inp) <= bc.BYTE_BUDGET * scale, (name, cus, scale)
        W = bc.KW * cus
        if name in ("create_list_small_many", "create_list_small_many_balanced", "verify_blocks_scratch"):
            assert case.build(cus, np.random.default_rng(3))["lens"].size == 16 * W + 64
        if name == "create_list_ticketed":
            assert W < case.build(cus, np.random.default_rng(3))["lens"].size <= 16 * W
