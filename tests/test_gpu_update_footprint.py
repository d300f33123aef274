"""hf3fs_crc_update_batch's write footprint on the GPU, for every compiled apply variant.

The existing update tests compare chunk bytes [0, out_size) of 512 B-aligned chunks that
are each other's neighbours.  Here every chunk, payload and the IO record array sit inside a
position-dependent canary at bases of every residue mod 16 (tests/update_footprint.py), and
after every batch the WHOLE chunk arena must equal the oracle's image: a granule before a
chunk base, one past max(size, offset + length), a write for an IO that failed its verify or
its argument check, a changed payload byte or input field all fail.  The cases are
parametrised over the copy bodies option apply_nt selects (k_update_apply's eight
instantiations, the one-shot apply's two at each piece size, k_update_fused's two), both
modes, and CRC32 where the kernel is templated on the polynomial.  Expected bytes and
checksums come from the oracle and the canary only; the kernels' loop thresholds only pick
the lengths.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import update_footprint as fp

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = 16 << 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _variants():
    """(pipeline, apply_nt, mode, checksum type): one entry per compiled copy variant and mode.
    Ticketed apply: apply_nt 0..7 (bit 0 / 1 non-temporal loads / stores, bit 2 the copy_range_hw
    body; 0..3 run copy_range's lane-shuffle rows).  One-shot: bit 0 only.  Fused: (nt & 6) == 6
    or not.  CRC32 where the kernel is templated on the polynomial."""
    out = []
    for mode in (0, 1):
        for nt in range(8):
            out.append(("ticketed", nt, mode, fp.CRC32C))
            out.append(("unfused_fine", nt, mode, fp.CRC32C))
        for pipeline in ("oneshot4", "oneshot8", "oneshot16", "oneshot_loop"):
            for nt in (6, 7):
                out.append((pipeline, nt, mode, fp.CRC32C))
        for nt in (0, 6):
            out.append(("fused", nt, mode, fp.CRC32C))
            out.append(("fused", nt, mode, fp.CRC32))
            out.append(("ticketed", nt, mode, fp.CRC32))
    return out


VARIANTS = _variants()
VARIANT_IDS = [f"{p}-nt{nt}-mode{m}-{'crc32c' if t == fp.CRC32C else 'crc32'}" for p, nt, m, t in VARIANTS]


@functools.lru_cache(maxsize=None)
def _scenario(orc, name, ctype):
    """Built once per (case, checksum type) and shared by every variant: the expected images
    do not depend on the kernel that runs."""
    build = {"tiny": fp.tiny_scenario, "rows": fp.rows_scenario, "rounds": fp.rounds_scenario}[name]
    return build(orc, ctype)


class GpuBackend:
    """update_footprint.run_scenario's backend: the HIP library on device buffers."""

    def __init__(self, hf, dev, ctype, mode):
        self.hf, self.dev, self.ctype, self.mode = hf, dev, ctype, mode

    def _up(self, a):
        return torch.from_numpy(np.array(a)).to(self.dev)  # (a copy: the scenario's images are read-only)

    def start(self, arena, pay_size, recbuf_size):
        raw = torch.empty(arena.size + LINE, dtype=torch.uint8, device=self.dev)
        lift = (-raw.data_ptr()) % LINE  # the arena starts on a 16 KiB line
        self.raw, self.arena = raw, raw[lift:lift + arena.size]
        self.arena.copy_(self._up(arena))
        self.pay = torch.empty(pay_size, dtype=torch.uint8, device=self.dev)
        self.rec = torch.empty(recbuf_size, dtype=torch.uint8, device=self.dev)
        return self.arena.data_ptr(), self.pay.data_ptr()

    def load(self, pay, recbuf):
        self.pay.copy_(self._up(pay))
        self.rec.copy_(self._up(recbuf))
        torch.cuda.synchronize()

    def call(self, n, max_len, stream):
        self.hf._lib.update_batch(self.ctype, self.rec.data_ptr() + fp.REC_GUARD, n, max_len, mode=self.mode,
                                  stream=stream)

    def fetch(self):
        torch.cuda.synchronize()
        return self.arena.cpu().numpy(), self.pay.cpu().numpy(), self.rec.cpu().numpy()

    def step(self, pay, recbuf, n, max_len):
        self.load(pay, recbuf)
        self.call(n, max_len, torch.cuda.current_stream())
        return self.fetch()


def _run(hf, orc, dev, opts, name, variant):
    pipeline, nt, mode, ctype = variant
    fp.set_pipeline(opts, pipeline)
    opts("apply_nt", nt)
    fp.run_scenario(_scenario(orc, name, ctype), GpuBackend(hf, dev, ctype, mode))


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_update_footprint_tiny(hf, orc, dev, opts, variant):
    """B1: 176 writes of 1..47 bytes (and a few longer ones ending at max_len) on empty or short
    4 KiB chunks 2 KiB apart: every destination, source, gap-start and gap-end residue mod 16
    (tests/test_update_footprint_model.py asserts the coverage)."""
    _run(hf, orc, dev, opts, "tiny", variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_update_footprint_rows(hf, orc, dev, opts, variant):
    """B2: 48 writes on 192 KiB chunks with 831..7233 full destination granules (one below, at and
    one above where the copy loops' unrolled rows start and step, for 256- and 1024-thread
    workgroups), heads and tails of 0, 1 and 15 bytes, every source shift, and writes across and
    one byte short of / past 4, 8 and 16 KiB destination lines; once on empty chunks (behind
    zero gaps) and once over that content."""
    _run(hf, orc, dev, opts, "rows", variant)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_update_footprint_rounds(hf, orc, dev, opts, variant):
    """B3: six rounds of mixed traffic with corrupted client checksums and INVALID_ARG IOs: the
    failed IOs' regions stay byte-identical, canary tail included."""
    _run(hf, orc, dev, opts, "rounds", variant)


@pytest.mark.parametrize("pipeline", ["fused", "unfused"])
@pytest.mark.parametrize("mode", [0, 1])
def test_update_footprint_engine_flag(hf, orc, dev, opts, mode, pipeline):
    """B4: chunk-engine IOs (HF3FS_UPDATE_FLAG_ENGINE) against orc.engine_apply, default pipelines."""
    opts("update_pipeline", pipeline)
    fp.run_scenario(fp.engine_scenario(orc), GpuBackend(hf, dev, fp.CRC32C, mode))


@pytest.mark.parametrize("mode", [0, 1])
def test_update_footprint_captured(hf, orc, dev, opts, mode):
    """B5: one one-shot update captured into a graph (its finalize forked onto the side stream)
    and replayed twice from restored chunks and records, the whole arena checked after each."""
    opts("update_pipeline", "unfused")
    opts("apply_grid", 1)
    scn = _scenario(orc, "rounds", fp.CRC32C)
    be = GpuBackend(hf, dev, fp.CRC32C, mode)
    fp.run_scenario(scn, be, rounds=1)  # an uncaptured batch gives the chunks content
    sent = scn.record_buffer(1, be.arena.data_ptr(), be.pay.data_ptr())
    be.load(scn.payload_image(1), sent)
    saved_arena, saved_rec = be.arena.clone(), be.rec.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev)):
        be.call(scn.n, scn.max_len, torch.cuda.current_stream())
    for _ in range(2):
        be.arena.copy_(saved_arena)
        be.rec.copy_(saved_rec)
        torch.cuda.synchronize()
        g.replay()
        fp.check_round(scn, 1, *be.fetch(), sent)
    del g


# ---- the first update call of a process, captured ------------------------------------------------
_CHILD = r"""
import importlib, hashlib, json, sys
import numpy as np, torch
repo, tests, path, mode = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
sys.path[:0] = [repo, tests]
import update_footprint as fp
hf = importlib.import_module("3fs_amd")
z = np.load(path)
dev = torch.device("cuda:0")
raw = torch.empty(z["arena"].size + 16384, dtype=torch.uint8, device=dev)
lift = (-raw.data_ptr()) % 16384
arena = raw[lift:lift + z["arena"].size]
arena.copy_(torch.from_numpy(z["arena"]).to(dev))
pay = torch.from_numpy(z["pay"]).to(dev)
rec = z["rec"].copy()
rec["chunk"] += np.uint64(arena.data_ptr())
rec["payload"][z["has_payload"]] += np.uint64(pay.data_ptr())
n = rec.size
d_ios = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
torch.cuda.synchronize()
g = torch.cuda.CUDAGraph()
call_error = None
try:  # the process's FIRST library call, inside a global-mode capture on a side stream
    with torch.cuda.graph(g, stream=torch.cuda.Stream(dev), capture_error_mode="global"):
        try:
            hf._lib.update_batch(hf.CRC32C, d_ios, n, int(z["max_len"]), mode=mode,
                                 stream=torch.cuda.current_stream())
        except hf.Hf3fsCrcError as e:  # (kept: the end of an invalidated capture raises over it)
            call_error = str(e)
except Exception as e:
    print(json.dumps({"error": f"{type(e).__name__}: {e}", "call_error": call_error}))
    sys.exit(3)
if call_error:
    print(json.dumps({"error": "update_batch failed inside the capture", "call_error": call_error}))
    sys.exit(3)
g.replay()
torch.cuda.synchronize()
res = np.frombuffer(d_ios.cpu().numpy().tobytes(), dtype=fp.REC)
print(json.dumps({"status": res["status"].tolist(), "case": res["checksum_case"].tolist(),
                  "size": res["out_size"].tolist(), "checksum": res["out_checksum"].tolist(),
                  "ctype": res["out_checksum_type"].tolist(),
                  "arena_sha256": hashlib.sha256(arena.cpu().numpy().tobytes()).hexdigest()}))
"""


def test_update_first_call_in_process_is_captured(orc, tmp_path):
    """A fresh process whose first library call is a DELTA update_batch (three-pass pipeline,
    one-shot apply) inside torch.cuda.graph(capture_error_mode="global"): the context, the hint
    slab, the side stream and the call's scratch are all first allocated during the capture.  The
    child replays the graph once; statuses, cases, sizes, checksums and a digest of the whole
    chunk arena equal orc.replica_apply's."""
    scn = fp.rounds_scenario(orc, n=16, max_len=64 << 10, rounds=2, seed=0xD1)
    r = scn.rounds[1]  # the child starts from the oracle's image after round 0
    path = str(tmp_path / "inputs.npz")
    np.savez(path, arena=scn.image_before(1), pay=scn.payload_image(1), rec=r.rec, has_payload=r.has_payload,
             max_len=scn.max_len)
    env = dict(os.environ, HF3FS_CRC_UPDATE_PIPELINE="unfused", HF3FS_CRC_APPLY_GRID="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, REPO, os.path.join(REPO, "tests"), path, "1"],
                       capture_output=True, text=True, timeout=150, env=env, cwd=REPO)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout
    got = lines[0]
    assert got["status"] == [e[0] for e in r.expect]
    assert got["case"] == [e[3] for e in r.expect]
    assert got["size"] == [e[1] for e in r.expect]
    assert list(zip(got["ctype"], got["checksum"])) == [tuple(e[2]) for e in r.expect]
    assert got["arena_sha256"] == hashlib.sha256(scn.image_after(1).tobytes()).hexdigest()
    assert fp.OK in got["status"] and fp.INVALID_ARG in got["status"]  # (the batch has both kinds)
