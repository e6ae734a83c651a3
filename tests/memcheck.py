"""Memory-contract harness for the C-ABI tests (tests/test_gpu_memcontract.py; self-tested on CPU tensors in
tests/test_memcheck_host.py).

An Arena carves every buffer of one call out of ONE torch.uint8 block, each with a 64 KiB guard band on either side, so that
a store a few floats behind an output lands in memory the test owns and is SEEN, instead of in allocator slack.  Buffers have
roles:

  input       filled by the caller; snapshot at arm(), compared bitwise by verify()
  output      pre-filled with a poison (a fixed quiet-NaN bit pattern, then 1e30); verify() counts elements that still hold it
  accumulate  caller data the call updates in place (beta = 1 / accumulate / gx in place): restored before every run
  workspace   exactly the byte count asked for (not rounded up), poisoned like an output; nothing is expected of its contents

An output taken with partial=True may keep unwritten elements (a weight image is sized for the larger of two piece schemes and
a pack writes what the active scheme reads): the same elements must then be written under both poisons, with the same bits.

run_twice() runs a call under both poisons: a kernel that reads scratch or output it did not write cannot give the same bits
both times.  Works on CPU tensors (the self-tests) and on device tensors alike.
"""
import torch

GUARD_BYTES = 64 * 1024
ALIGN = 256
GUARD_BYTE = 0xA5                    # guards: 0xA5A5A5A5 words (a tiny negative float, distinct from both poisons)
NAN_BITS = 0x7FC0BEEF                # the quiet-NaN sentinel, compared as int32
BIG = 1e30                           # the finite poison of the second run
MS_OK, MS_ERR_INVALID_ARG, MS_ERR_UNSUPPORTED, MS_ERR_WORKSPACE = 0, -1, -2, -3


class MemcheckError(AssertionError):
    pass


class Buf:
    """One guarded buffer: .t is the typed view handed to the kernel, .ptr its address."""

    def __init__(self, name, role, start, nbytes, t, raw, partial=False):
        self.name, self.role, self.start, self.nbytes, self.t, self.raw = name, role, start, nbytes, t, raw
        self.partial = partial
        self.snapshot = None

    @property
    def ptr(self):
        return self.raw.data_ptr()


class Arena:
    def __init__(self, device="cpu", capacity=32 << 20):
        self.block = torch.full((int(capacity),), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.base = self.block.data_ptr()
        self.cursor = 0
        self.bufs = []
        self.poison = None

    # ---- carving
    def take(self, shape, role, offset_bytes=0, name=None, dtype=torch.float32, partial=False):
        """A contiguous float32 (int32 for sign words) view at a 256-byte aligned address + offset_bytes; role
        'workspace': `shape` is a BYTE count and the view is uint8."""
        assert role in ("input", "output", "accumulate", "workspace"), role
        assert offset_bytes % 4 == 0 and 0 <= offset_bytes < ALIGN
        if role == "workspace":
            n, dtype, shape = int(shape), torch.uint8, (int(shape),)
        else:
            shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
            n = 4
            for s in shape:
                n *= s
        start = self.cursor + GUARD_BYTES
        start += (-(self.base + start)) % ALIGN + offset_bytes
        end = start + n
        # (a guard behind every buffer: none is ever flush against the end of the block)
        if end + GUARD_BYTES + ALIGN > self.block.numel():
            raise MemcheckError("arena of %d bytes is too small for %r (%d bytes)" % (self.block.numel(), name, n))
        raw = self.block[start:end]
        t = raw if dtype == torch.uint8 else raw.view(dtype).view(shape)
        b = Buf(name or "%s%d" % (role, len(self.bufs)), role, start, n, t, raw, partial)
        b.lo, b.hi = self.cursor, end + GUARD_BYTES            # guards: [lo, start) and [end, hi)
        self.cursor = b.hi
        self.bufs.append(b)
        return b

    def put(self, data, role="input", offset_bytes=0, name=None):
        """take() + copy of `data` (a float32 / int32 tensor or numpy array)."""
        data = torch.as_tensor(data)
        b = self.take(tuple(data.shape), role, offset_bytes, name, dtype=data.dtype)
        b.t.copy_(data)
        return b

    # ---- poisoning
    def _fill(self, b, poison):
        n4 = b.nbytes // 4
        if n4:
            words = b.raw[:4 * n4].view(torch.int32)
            if poison == "nan":
                words.fill_(NAN_BITS)
            else:
                words.view(torch.float32).fill_(BIG)
        if b.nbytes % 4:
            b.raw[4 * n4:].fill_(0x7F)

    def arm(self, poison="nan"):
        """Before a run: inputs are snapshot (first time), accumulate buffers snapshot (first time) / restored (later),
        outputs and workspaces filled with the poison."""
        assert poison in ("nan", "big")
        self.poison = poison
        for b in self.bufs:
            if b.role in ("input", "accumulate"):
                if b.snapshot is None:
                    b.snapshot = b.raw.clone()
                elif b.role == "accumulate":
                    b.raw.copy_(b.snapshot)
            else:
                self._fill(b, poison)

    # ---- checking
    def _guard_damage(self, b):
        out = []
        for what, lo, hi, origin in (("before", b.lo, b.start, b.start), ("behind", b.start + b.nbytes, b.hi, b.start + b.nbytes)):
            bad = (self.block[lo:hi] != GUARD_BYTE).nonzero()
            if bad.numel():
                first, last = int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin
                out.append("guard %s %s %r changed: %d byte(s), offsets %+d .. %+d from its %s" %
                           (what, b.role, b.name, bad.numel(), first, last, "start" if what == "before" else "end"))
        return out

    def unwritten(self, b):
        """Number of elements of an output that still hold the poison of the last arm()."""
        words = b.raw[:4 * (b.nbytes // 4)].view(torch.int32)
        if self.poison == "nan":
            return int((words == NAN_BITS).sum())
        return int((words.view(torch.float32) == BIG).sum())

    def problems(self, written=True):
        """Everything wrong after a call (the device must be synchronised): changed guards with byte offsets, changed inputs,
        unwritten output elements.  written=False: the call refused, so no output element may have been written;
        written=None: outputs are not looked at."""
        out = []
        for b in self.bufs:
            out += self._guard_damage(b)
            if b.role == "input" and b.snapshot is not None:
                bad = (b.raw.view(torch.int32) != b.snapshot.view(torch.int32)).nonzero()
                if bad.numel():
                    out.append("input %r changed: %d element(s), first at element %d" % (b.name, bad.numel(), int(bad[0])))
            if b.role == "accumulate" and written is False and b.snapshot is not None and not torch.equal(b.raw, b.snapshot):
                out.append("accumulate %r changed by a call that refused" % b.name)
            if b.role == "output" and written is not None:
                n = self.unwritten(b)
                if written and n == b.nbytes // 4 and b.partial:
                    out.append("output %r: nothing written" % b.name)
                if written and n and not b.partial:
                    words = b.raw[:4 * (b.nbytes // 4)].view(torch.int32)
                    hit = (words == NAN_BITS) if self.poison == "nan" else (words.view(torch.float32) == BIG)
                    out.append("output %r: %d of %d element(s) never written, first at element %d" %
                               (b.name, n, b.nbytes // 4, int(hit.nonzero()[0])))
                if not written and n != b.nbytes // 4:
                    out.append("output %r: %d element(s) written by a call that refused" % (b.name, b.nbytes // 4 - n))
        return out

    def verify(self, written=True):
        p = self.problems(written)
        if p:
            raise MemcheckError("; ".join(p))

    def run_twice(self, call, sync=None, tol=None):
        """call() -> status, run with outputs / workspaces poisoned by the NaN pattern and then by 1e30; verify() after each.
        Outputs and accumulate buffers of the two runs must agree bitwise -- or, tol = (route name, rel-L2 bound) for a route
        that sums with float atomics, within that bound.  -> (status, {buffer name: result tensor of the first run})."""
        runs = []
        for poison in ("nan", "big"):
            self.arm(poison)
            rc = call()
            if sync:
                sync()
            self.verify(written=(rc == MS_OK))
            runs.append((rc, {b.name: b.t.clone() for b in self.bufs if b.role in ("output", "accumulate")}))
        (rc0, a), (rc1, c) = runs
        if rc0 != rc1:
            raise MemcheckError("status depends on scratch contents: %d then %d" % (rc0, rc1))
        bufs = {b.name: b for b in self.bufs}
        for name in a:
            if rc0 != MS_OK and bufs[name].role != "accumulate":
                continue
            x, y = a[name].contiguous().view(-1), c[name].contiguous().view(-1)
            xi, yi = x.view(torch.int32), y.view(torch.int32)
            if bufs[name].partial:                  # the same elements written both times, with the same bits
                wx, wy = xi != NAN_BITS, y.view(torch.float32) != BIG
                if not torch.equal(wx, wy):
                    raise MemcheckError("%r: the set of written elements depends on prior contents (%d, then %d written)" %
                                        (name, int(wx.sum()), int(wy.sum())))
                xi, yi, x, y = xi[wx], yi[wx], x[wx], y[wx]
            if tol is None:
                if not torch.equal(xi, yi):
                    diff = (xi != yi).nonzero()
                    raise MemcheckError("%r depends on prior scratch / output contents: %d element(s) differ between the "
                                        "NaN-poisoned and the 1e30-poisoned run, first at element %d" %
                                        (name, diff.numel(), int(diff[0])))
            else:
                e = float((x.double() - y.double()).norm() / (y.double().norm() + 1e-300))
                if not e < tol[1]:
                    raise MemcheckError("%r (%s): runs differ by %.3g rel-L2, bound %.3g" % (name, tol[0], e, tol[1]))
        return rc0, a
