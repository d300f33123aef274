"""The read footprint of hf3fs_crc_client_write_prepare / _complete: tests/client_write_footprint.py
in a child process against the load-checked build, judged with tests/load_footprint.py's compare.

Per call Required <= Read <= Legal over the data buffers: Legal is the payloads of the IOs that are
valid by themselves, Required those payloads when VERIFY is set and the batch is not poisoned;
nothing refused; no read of a record array at an index >= n (at n = 65 and at n = 1000); outputs
equal to the model's.  Without VERIFY, and in complete, not one granule of a data buffer is read."""
import json
import os
import subprocess
import sys

import pytest

import client_write_footprint as wf
import load_footprint as lf

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    check_lib = os.path.join(REPO, "3fs_amd", "lib", "libhf3fs_crc_loadcheck.so")
    assert os.path.exists(check_lib), f"{check_lib} missing: 3fs_amd/build.py builds it beside the default library"
    out = str(tmp_path_factory.mktemp("client_write") / "client_write.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "client_write_footprint.py"), out],
                       capture_output=True, text=True, timeout=240, env=dict(os.environ, HF3FS_CRC_LIB=check_lib))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    with open(out) as f:
        return json.load(f)["reports"]


def test_read_footprint(reports):
    cases = wf.cases()
    assert sorted(reports) == sorted(c.name for c in cases) and len(cases) == 12
    assert {(c.call, c.n >= 1000) for c in cases} == {(call, big) for call in ("prepare", "complete") for big in (False, True)}
    bad = []
    for c in cases:
        defects = lf.compare(c, reports[c.name])
        if defects:
            bad.append(lf.describe(c, defects))
    assert not bad, f"{len(bad)} of {len(cases)} calls:\n" + "\n".join(bad[:12])


def test_calls_that_do_not_hash_read_no_data(reports):
    seen = 0
    for c in wf.cases():
        r = reports[c.name]
        read, _ = lf.mask_from_runs(r["read"], c.n_granules)
        if c.call == "complete" or not c.verify:
            assert not read.any(), f"{c.name}: {int(read.sum())} granules read though nothing is hashed"
            assert r["outside"] == 0 and r["desc"] == 0, (c.name, r["log"][:4])
            seen += 1
        elif not c.poisoned:
            assert r["counters"], f"{c.name}: no checked load was counted"
            assert read.any() and c.hashed > 0
    assert seen == 6
