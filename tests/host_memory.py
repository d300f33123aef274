"""Where a call's buffers live, and what the call may have written, shared by
tests/test_gpu_host_memory.py (the HIP library on HBM and on registered host memory) and
tests/test_host_memory_model.py (numpy stand-ins that check the checker).

include/hf3fs_crc.h promises that every d_* argument may be HBM or host memory that is
hipHostRegister'ed and mapped to the device.  `Registered` is such memory: a numpy buffer
registered with hf3fs_crc_host_register, as 3FS registers its RDMA BufferPool slabs.  `Plain` is
unregistered numpy memory with the same interface, for the stand-ins.

`Placed` puts one batch case of tests/batch_cases.py into memory: the arena and every buffer in
an allocation of its own, each between two guards of update_footprint.canary, and `check` holds
the call to the header: the outputs are the reference's, and every byte outside
Case.output_mask -- the arena, the inputs, the reserved fields, every guard -- is the byte sent.

Numpy and ctypes only: no GPU, no torch.
"""
import importlib

import numpy as np

import batch_cases as bc
import update_footprint as fp

PAGE = 4096
GUARD = 4 << 10
SALT_ARENA = 0x1D      # + a per-buffer step: no two images of a case carry the same canary
_KEPT = []             # registered arrays that were never (or not successfully) unregistered: kept alive


def _lib():
    return importlib.import_module("3fs_amd")._lib


def _aligned(nbytes, align, lead):
    """(raw, view): `nbytes` bytes of numpy memory whose first byte sits `lead` bytes past an
    address that is a multiple of `align` (a multiple of PAGE), inside whole pages of their own."""
    assert align % PAGE == 0 and lead >= 0
    span = -(-(lead + nbytes) // PAGE) * PAGE
    raw = np.zeros(span + align, dtype=np.uint8)
    k = (-raw.ctypes.data) % align
    return raw, raw[k:k + span]


class Plain:
    """`nbytes` of plain numpy memory; .host is a view, .dev the address of the same byte."""

    def __init__(self, nbytes, align=PAGE, lead=0):
        self._raw, pages = _aligned(nbytes, align, lead)
        self.host = pages[lead:lead + nbytes]
        self.dev = self.host.ctypes.data

    def write(self, image):
        self.host[:] = image

    def read(self):
        return self.host.copy()

    def close(self):
        self.host = self._raw = None


class Registered:
    """`nbytes` of host memory registered with hf3fs_crc_host_register and mapped to the device.
    The registration covers whole pages that no other allocation shares.  .host is a numpy view
    of the bytes, .dev the device address of the same byte; (.dev - lead) % align == 0.

    close() only after every stream that touched the buffer is synchronised: it unregisters
    first and drops the array after, so no mapped page is ever freed, and after close() neither
    .host nor .dev exists, so no later call can be handed the address.  Use as a context manager
    or call close() in a finally."""

    def __init__(self, nbytes, align=PAGE, lead=0):
        self._raw = None
        raw, self._pages = _aligned(nbytes, align, lead)
        self._base = self._pages.ctypes.data
        d = _lib().host_register(self._base, self._pages.size)   # (raises: nothing is registered then)
        self._raw = raw
        self.host = self._pages[lead:lead + nbytes]
        self.dev = d + lead

    def write(self, image):
        self.host[:] = image

    def read(self):
        return self.host.copy()

    def close(self):
        if self._raw is None:
            return
        raw, ok = self._raw, False
        self.host = self.dev = self._pages = self._raw = None   # no address is handed out from here on
        try:
            _lib().host_unregister(self._base)
            ok = True
        finally:
            if not ok:
                _KEPT.append(raw)   # perhaps still mapped: never freed under the device
            del raw                 # (else: dropped here, after the unregister)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        # Not closed: a stream may still use the pages, so they are neither unregistered nor freed.
        if getattr(self, "_raw", None) is not None:
            _KEPT.append(self._raw)


# ---- one batch case, placed ---------------------------------------------------------------------
def _unit(case, name, image):
    """The alignment the C type of the argument asks for: 8 for arrays of ABI structs (they hold
    uint64_t), else the element size."""
    return 8 if name in case.layouts else image.dtype.itemsize


class Placed:
    """The arena and every buffer of `case`, each in an allocation of its own from
    alloc(nbytes, align, lead) (Plain, Registered, or the GPU test's HBM twin), as
    [GUARD canary][the bytes][GUARD canary].

    Leads are odd: the arena starts an odd number of KiB past a page -- on a 1 KiB boundary, from
    which the cases count their residues, as OnDevice of test_gpu_batch_contexts.py places it -- and
    buffer number i starts (2 i + 1) elements past one, so a byte array such as d_mismatch starts
    and ends on odd addresses while every uint32_t / uint64_t / struct pointer keeps the alignment
    its C type has (and no more: 4 mod 8 for words, 8 mod 16 for records)."""

    def __init__(self, case, inp, alloc):
        self.case, self.inp, self.mem, self.sent, self.base = case, inp, {}, {}, 0
        try:
            if "arena" in inp:
                self.mem["arena"] = alloc(2 * GUARD + inp["arena"].size, PAGE, 3 << 10)
                self.base = self.mem["arena"].dev + GUARD
                assert self.base % 1024 == 0 and self.base % PAGE
                self.sent["arena"] = self._image(inp["arena"], SALT_ARENA)
            images = case.buffers(inp, self.base)
            self.dtypes = {k: a.dtype for k, a in images.items()}
            self.sizes = {k: a.nbytes for k, a in images.items()}
            for i, (k, a) in enumerate(images.items()):
                unit = _unit(case, k, a)
                self.mem[k] = alloc(2 * GUARD + a.nbytes, PAGE, unit * (2 * i + 1))
                assert self.mem[k].dev % unit == 0 and (self.mem[k].dev // unit) % 2
                self.sent[k] = self._image(np.ascontiguousarray(a).view(np.uint8).reshape(-1), SALT_ARENA + 0x20 * (i + 1))
            if "arena" in inp:
                self.sizes["arena"] = inp["arena"].size
            masks = case.output_mask(inp)
            assert masks.keys() == images.keys()
            self.masks = {}
            for k, img in self.sent.items():
                self.masks[k] = np.zeros(img.size, dtype=bool)   # guards and arena: never writable
                if k in masks:
                    assert masks[k].dtype == bool and masks[k].size == self.sizes[k], k
                    self.masks[k][GUARD:GUARD + self.sizes[k]] = masks[k]
            for k, img in self.sent.items():
                img.setflags(write=False)
                self.mem[k].write(img)
        except BaseException:
            self.close()
            raise

    @staticmethod
    def _image(data, salt):
        img = fp.canary(2 * GUARD + data.size, salt)
        img[GUARD:GUARD + data.size] = data
        return img

    def pointers(self):
        """What Case.call takes: the address of byte 0 of every buffer, and of the arena."""
        p = {k: m.dev + GUARD for k, m in self.mem.items()}
        p["arena"] = self.base
        return p

    def fetch(self):
        """The whole images, guards included (after the streams are synchronised)."""
        return {k: m.read() for k, m in self.mem.items()}

    def host(self, got):
        """Typed views of the buffers inside the images `got`, as Case.extract / Case.store take them."""
        return {k: got[k][GUARD:GUARD + self.sizes[k]].view(dt) for k, dt in self.dtypes.items()}

    def where(self, name, pos):
        """Image offset `pos` of buffer `name` in words: the guard, or the record and its field."""
        n = self.sizes[name]
        if pos < GUARD:
            return f"{name}: front guard, {GUARD - pos} B before the buffer"
        if pos >= GUARD + n:
            return f"{name}: back guard, {pos - GUARD - n} B past the buffer's {n} bytes"
        off = pos - GUARD
        if name == "arena":
            return f"{name}: offset {off}"
        dt = self.case.layouts.get(name)
        if dt is not None:
            return f"{name}: record {off // dt.itemsize} field {bc.field_at(dt, off % dt.itemsize)}, offset {off}"
        return f"{name}: element {off // self.dtypes[name].itemsize}, offset {off}"

    def check(self, got, ref, what):
        """The outputs are the reference's, and every byte the header does not give to the call
        is the byte that was sent (raises AssertionError naming buffer, field and offset)."""
        errs = []
        out = self.case.extract(self.inp, self.host(got))
        if out.keys() != ref.keys():
            errs.append(f"outputs {sorted(out)} != {sorted(ref)}")
        for k, want in ref.items():
            if k in out and not np.array_equal(out[k], want):
                bad = np.flatnonzero(out[k] != want)
                errs.append(f"output {k} differs at {bad.size} of {want.size}: first {bad[:5].tolist()}, got "
                            f"{out[k][bad[:5]].tolist()}, want {want[bad[:5]].tolist()}")
        for k, sent in self.sent.items():
            assert got[k].shape == sent.shape, k
            stray = np.flatnonzero((got[k] != sent) & ~self.masks[k])
            if stray.size:
                first, last = int(stray[0]), int(stray[-1])
                errs.append(f"stray write: {stray.size} bytes outside the call's outputs changed; first at "
                            f"{self.where(k, first)} (sent {int(sent[first]):#04x}, got {int(got[k][first]):#04x}), "
                            f"last at {self.where(k, last)}")
        if errs:
            raise AssertionError(f"{what}: " + "; ".join(errs))

    def close(self):
        mem, self.mem = self.mem, {}
        err = None
        for m in mem.values():
            try:
                m.close()
            except BaseException as e:  # noqa: BLE001 - every registration is taken back before it is raised
                err = err or e
        if err:
            raise err
