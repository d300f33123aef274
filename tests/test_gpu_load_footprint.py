"""The read footprint of every kernel that loads caller bytes.

Each family of tests/load_footprint.py runs in a fresh child process against the load-checked
build of the library (HF3FS_CRC_LIB = libhf3fs_crc_loadcheck.so): the child lays every buffer out in
one allocation, arms the check, runs the call, and reports the granules the call's loads touched.
Here: Required <= Read <= Legal per call, nothing refused, no descriptor index out of range, the
outputs equal to the oracle's; and over the whole file every enumerated load site is reached.

A child that dies (a fault, an abort, its time limit) ends the file's GPU work: the test fails
with the child's output and no further child is started.
"""
import functools
import json
import os
import subprocess
import sys

import pytest

import load_footprint as lf

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_LIB = os.path.join(REPO, "3fs_amd", "lib", "libhf3fs_crc_loadcheck.so")
CHILD_TIMEOUT = 240
_dead = []   # the output of the first child that died


@functools.lru_cache(maxsize=None)
def _reports(family, out_dir):
    if _dead:
        pytest.fail("an earlier child of this file died; no further child is started:\n" + _dead[0])
    assert os.path.exists(CHECK_LIB), f"{CHECK_LIB} missing: 3fs_amd/build.py builds it beside the default library"
    out = os.path.join(out_dir, family + ".json")
    env = dict(os.environ, HF3FS_CRC_LIB=CHECK_LIB)
    try:
        r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "load_footprint.py"), family, out],
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
        text = f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-6000:]}"
        ok = r.returncode == 0
    except subprocess.TimeoutExpired as e:
        text, ok = f"time limit of {CHILD_TIMEOUT} s\n{e.stdout}\n{e.stderr}", False
    if not ok:
        _dead.append(f"family {family}: {text}")
        pytest.fail(_dead[0])
    with open(out) as f:
        return json.load(f)["reports"]


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("load_footprint"))


@pytest.mark.parametrize("family", sorted(lf.FAMILIES))
def test_read_footprint(family, out_dir):
    reports = _reports(family, out_dir)
    cases = lf.FAMILIES[family]()
    assert sorted(reports) == sorted(c.name for c in cases)
    bad = []
    for c in cases:
        defects = lf.compare(c, reports[c.name])
        if defects:
            bad.append(lf.describe(c, defects))
    print(f"{family}: {len(cases)} calls; sites reached: "
          + ", ".join(f"{k} {lf.SITES[k][0]} ({n} loads, first in {case})"
                      for k, (n, case) in sorted(lf.sites_reached(reports).items())))
    assert not bad, f"{len(bad)} of {len(cases)} calls:\n" + "\n".join(bad[:12])


def test_every_site_is_reached(out_dir):
    """Every enumerated load site counts a load in some case (and the test says which): a site no
    case reaches is dead code or a missing case."""
    reports = {}
    for family in sorted(lf.FAMILIES):
        for name, r in _reports(family, out_dir).items():
            reports[f"{family}: {name}"] = r
    for k, (n, case) in sorted(lf.sites_reached(reports).items()):
        print(f"site {k} {lf.SITES[k][0]}: {n} loads, first in {case}")
    assert lf.unreached(reports) == []
