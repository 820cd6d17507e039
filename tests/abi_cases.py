"""Shared by the tests of the C boundary (test_gpu_abi_steps.py, test_gpu_abi_devptr.py): host planes in buffers whose rows are any
distance apart, with padding that would change a result if it were read (inputs) or that shows a write (outputs), and the steps of one
call, all different."""
import ctypes as C

import numpy as np

FILL = 0xEE
MAP_CODES = np.array([0, 50, 100, 150], np.uint8)


def _poison(plane, rows, nbytes, rng):
    """nbytes of padding per row in the plane's own format: opaque pixels of random colours (BGRA), region codes (map), finite values far
    from any flow or blend weight (float planes)"""
    if plane.dtype == np.uint8 and plane.ndim == 3:
        px = rng.integers(0, 256, (rows, nbytes // 4, 4), dtype=np.uint8)
        px[..., 3] = 255
        return px.reshape(rows, nbytes)
    if plane.dtype == np.uint8:
        return rng.choice(MAP_CODES, (rows, nbytes))
    v = rng.uniform(64.0, 256.0, (rows, nbytes // 4)) * rng.choice([-1.0, 1.0], (rows, nbytes // 4))
    return v.astype(np.float32).view(np.uint8)


class In:
    """an input plane (rows, cols[, channels]) in a buffer whose rows are `step` bytes apart; the padding holds poison"""

    def __init__(self, plane, step, seed=0):
        self.plane = np.ascontiguousarray(plane)
        self.rows = self.plane.shape[0]
        self.width = self.plane[0].nbytes
        self.step = int(step)
        elem = self.plane.itemsize * (self.plane.shape[2] if self.plane.ndim == 3 else 1)
        assert self.step >= self.width and self.step % elem == 0, "a step is a multiple of its element size"
        self.buf = np.empty((self.rows, self.step), np.uint8)
        self.buf[:, :self.width] = self.plane.reshape(self.rows, -1).view(np.uint8)
        self.buf[:, self.width:] = _poison(self.plane, self.rows, self.step - self.width, np.random.default_rng(1000 + seed))
        self.ptr = C.c_void_p(self.buf.ctypes.data)

    def read(self, step):
        """the image a reader that takes the rows `step` bytes apart is given, as far as its rows lie inside the buffer"""
        flat = self.buf.ravel()
        n = min(self.rows, (flat.size - self.width) // step + 1)
        return np.stack([flat[r * step:r * step + self.width] for r in range(n)])

    def assert_poison_seen(self, wrong_steps):
        right = self.buf[:, :self.width]
        for s in wrong_steps:
            if s == self.step:
                continue
            got = self.read(s)
            assert len(got) > 1 and not np.array_equal(got, right[:len(got)]), "read at step %d the buffer of step %d gives the right image: the padding proves nothing" % (s, self.step)


class Out:
    """an output plane of `shape` in a buffer whose rows are `step` bytes apart, every byte FILL before the call"""

    def __init__(self, shape, dtype, step):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.width = int(np.prod(self.shape[1:])) * self.dtype.itemsize
        self.step = int(step)
        assert self.step >= self.width
        self.buf = np.full((self.shape[0], self.step), FILL, np.uint8)
        self.ptr = C.c_void_p(self.buf.ctypes.data)

    def plane(self):
        return np.ascontiguousarray(self.buf[:, :self.width]).view(self.dtype).reshape(self.shape)

    def padding_kept(self):
        return bool((self.buf[:, self.width:] == FILL).all())

    def untouched(self):
        return bool((self.buf == FILL).all())


class Steps:
    """the step arguments of one call: name=(row width in bytes, padding in bytes).  No two share a value.  `short` names the one that is
    passed one byte below its row width while the buffers keep their layout."""

    def __init__(self, short=None, **kw):
        self.short = short
        self.width = {k: int(w) for k, (w, _) in kw.items()}
        self.lay = {k: int(w) + int(p) for k, (w, p) in kw.items()}
        assert all(p > 0 for _, p in kw.values()), "every step of the call is padded"
        assert len(set(self.lay.values())) == len(self.lay), "no two arguments of the call share a step: %r" % self.lay
        assert short is None or short in kw, "%r is no step argument of this call (%r)" % (short, sorted(kw))

    def __getitem__(self, k):
        return self.lay[k]

    def arg(self, k):
        return C.c_size_t(self.width[k] - 1 if k == self.short else self.lay[k])


class Run:
    """what one call was given and gave"""

    def __init__(self, rc, ins, outs, steps):
        self.rc, self.ins, self.outs, self.steps = rc, ins, outs, steps

    def assert_padded_ok(self, ctx):
        """the call succeeded, every input's poison would have been seen under any other step of the call or the packed one, and every
        output's padding still holds its fill"""
        assert self.rc == 0, "error %d: %s" % (self.rc, ctx.l.pf_last_error(ctx.h).decode())
        for i in self.ins:
            i.assert_poison_seen(set(self.steps.lay.values()) | {i.width})
        for name, o in self.outs.items():
            assert o.padding_kept(), "%s: the padding between the rows was written" % name

    def assert_refused(self, ctx):
        """PF_ERR_ARG "row step too small" before any work: no kernel family seen by the profile, every output byte still the fill"""
        assert self.rc == -1, "a %s one byte below the row width was accepted (rc %d)" % (self.steps.short, self.rc)
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert "row step too small" in msg, "%s short: %r" % (self.steps.short, msg)
        ran = sorted(k for k, (_, n) in ctx.profile().items() if n)
        assert not ran, "%s short: kernels ran before the refusal: %r" % (self.steps.short, ran)
        for name, o in self.outs.items():
            assert o.untouched(), "%s short: %s was written" % (self.steps.short, name)


def ndiff(a, b):
    return int((np.asarray(a) != np.asarray(b)).sum())


def ptrs(v):
    """array of the host pointers of In / Out objects (None: NULL)"""
    return (C.c_void_p * max(len(v), 1))(*[x.ptr if x is not None else None for x in v])
