"""The record reads of hf3fs_crc_range_query / hf3fs_crc_file_length: tests/range_footprint.py in a
child process against the load-checked build, written the way the server-read footprint test is.

Per case (tables of 1, 255, 257 and 1,000 records; ranges below the first id, above the last and over
the whole table; a file whose segment ends the op array): no load from d_meta at an index >= n_meta,
none from d_ops at an index >= n_ops -- the binary searches' probes, the order check's neighbour and
the list's op search included -- nothing refused, no chunk byte loaded (the two calls load records
only), and outputs (ops, files, list, both d_info) equal to the model's."""
import json
import os
import subprocess
import sys

import pytest

import range_footprint as rf

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    check_lib = os.path.join(REPO, "3fs_amd", "lib", "libhf3fs_crc_loadcheck.so")
    assert os.path.exists(check_lib), f"{check_lib} missing: 3fs_amd/build.py builds it beside the default library"
    out = str(tmp_path_factory.mktemp("range") / "range.json")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "range_footprint.py"), out],
                       capture_output=True, text=True, timeout=240, env=dict(os.environ, HF3FS_CRC_LIB=check_lib))
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
    with open(out) as f:
        return json.load(f)["reports"]


def test_no_record_is_read_past_its_array(reports):
    cases = rf.cases()
    assert sorted(reports) == sorted(c["name"] for c in cases) and [c["meta"].size for c in cases] == [1, 255, 257, 1000]
    for c in cases:
        r = reports[c["name"]]
        assert r["desc"] == 0 and r["outside"] == 0, f"{c['name']}: refused loads {r['log'][:6]}"
        assert r["outputs"] == "ok", f"{c['name']}: {r['outputs']}"
        assert r["granules"] == 0, f"{c['name']}: {r['granules']} granules of caller bytes loaded by a byte site"
        assert r["listed"] > 0
