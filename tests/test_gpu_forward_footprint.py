"""The read footprint of hf3fs_crc_forward_prepare / _complete: tests/forward_footprint.py in a child
process against the load-checked build, judged with tests/load_footprint.py's compare.

Per call Required <= Read <= Legal over the data buffers: the chunks of the jobs prepare's syncing
read hashes, the outgoing buffers complete re-hashes after a 4080 answer, and nothing else; nothing
refused; no read of d_jobs at an index >= n (at n = 65 and at n = 1000); outputs equal to the
model's.  In a call where no job hashes not one granule of a data buffer is read."""
import json
import os
import subprocess
import sys

import pytest

import forward_footprint as ff
import load_footprint as lf

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    check_lib = os.path.join(REPO, "3fs_amd", "lib", "libhf3fs_crc_loadcheck.so")
    assert os.path.exists(check_lib), f"{check_lib} missing: 3fs_amd/build.py builds it beside the default library"
    out = str(tmp_path_factory.mktemp("forward") / "forward.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "forward_footprint.py"), out],
                       capture_output=True, text=True, timeout=240, env=dict(os.environ, HF3FS_CRC_LIB=check_lib))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    with open(out) as f:
        return json.load(f)["reports"]


def test_read_footprint(reports, orc):
    cases = ff.cases(orc)
    assert sorted(reports) == sorted(c.name for c in cases) and len(cases) == 10
    assert {(c.call, c.n) for c in cases} == {(call, n) for call in ("prepare", "complete") for n in (65, 1000)}
    bad = []
    for c in cases:
        defects = lf.compare(c, reports[c.name])
        if defects:
            bad.append(lf.describe(c, defects))
    assert not bad, f"{len(bad)} of {len(cases)} calls:\n" + "\n".join(bad[:12])


def test_jobs_that_do_not_hash_contribute_no_load(reports, orc):
    seen = 0
    for c in ff.cases(orc):
        r = reports[c.name]
        read, _ = lf.mask_from_runs(r["read"], c.n_granules)
        if c.hashed == 0:
            assert not read.any(), f"{c.name}: {int(read.sum())} granules read though no job hashes"
            assert r["outside"] == 0 and r["desc"] == 0, (c.name, r["log"][:4])
            seen += 1
        else:   # (test_read_footprint: exactly the hashing jobs' buffers) the other jobs are the majority
            assert r["counters"], f"{c.name}: no checked load was counted"
            assert read.any() and c.hashed < c.n // 2
    assert seen == 4
