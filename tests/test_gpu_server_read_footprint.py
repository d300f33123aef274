"""The read footprint of hf3fs_crc_server_read_prepare / _complete: tests/server_read_footprint.py in a
child process against the load-checked build, judged with tests/load_footprint.py's compare.

Per call Required <= Read <= Legal over the read buffers: the bytes [localbuf + head_len, +L) of the
jobs that hash or pack, L the clipped length, and nothing else -- no load from a localbuf's head, its
tail or past L; nothing refused; no read of a record at an index >= n (at n = 65 and at n = 1000);
outputs (records, d_info, the inline arena, the RDMA list) equal to the model's.  Prepare, and a
complete in which no job hashes or packs, read not one granule of a read buffer."""
import json
import os
import subprocess
import sys

import pytest

import load_footprint as lf
import server_read_footprint as sf

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    check_lib = os.path.join(REPO, "3fs_amd", "lib", "libhf3fs_crc_loadcheck.so")
    assert os.path.exists(check_lib), f"{check_lib} missing: 3fs_amd/build.py builds it beside the default library"
    out = str(tmp_path_factory.mktemp("server_read") / "server_read.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "server_read_footprint.py"), out],
                       capture_output=True, text=True, timeout=240, env=dict(os.environ, HF3FS_CRC_LIB=check_lib))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    with open(out) as f:
        return json.load(f)["reports"]


def test_read_footprint(reports, orc):
    cases = sf.cases(orc)
    assert sorted(reports) == sorted(c.name for c in cases) and len(cases) == 7
    assert {(c.call, c.n) for c in cases} == {(call, n) for call in ("prepare", "complete") for n in (65, 1000)}
    bad = []
    for c in cases:
        defects = lf.compare(c, reports[c.name])
        if defects:
            bad.append(lf.describe(c, defects))
    assert not bad, f"{len(bad)} of {len(cases)} calls:\n" + "\n".join(bad[:12])


def test_jobs_that_neither_hash_nor_pack_contribute_no_load(reports, orc):
    seen = 0
    for c in sf.cases(orc):
        r = reports[c.name]
        read, _ = lf.mask_from_runs(r["read"], c.n_granules)
        if c.hashed == 0:
            assert not read.any(), f"{c.name}: {int(read.sum())} granules read though no job hashes or packs"
            assert r["outside"] == 0 and r["desc"] == 0, (c.name, r["log"][:4])
            seen += 1
        else:
            assert r["counters"], f"{c.name}: no checked load was counted"
            assert read.any() and c.hashed < c.n
    assert seen == 4
