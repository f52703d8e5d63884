"""What the catalogue entry points share (``measure_blends``, ``render_blends``,
``initialization.init_blends`` and the ``lite`` ones): the working-set budget and the chunks it
cuts a group into, packed-buffer offsets and concatenation, the argument list of the entries
that take host buffers, and the uploads and launches of those that take device buffers.  Host
only until something is launched: torch and the library are imported where they are used."""

import numpy as np

# Device working set of one chunk of a catalogue call: a group whose blends need more is cut.
# Large enough that a catalogue of a few thousand postage-stamp blends is one chunk, small next
# to the memory of any device.
WORKING_SET_BYTES = 1 << 30


def defaults(working_set_bytes, device):
    """``(budget, device)`` of a catalogue call from its two optional arguments."""
    return (WORKING_SET_BYTES if working_set_bytes is None else working_set_bytes,
            0 if device is None else int(device))


def chunks(items, budget):
    """Consecutive runs of ``(position, bytes)`` whose working sets stay within ``budget`` (a
    blend beyond the budget is a chunk of its own): the positions, run by run."""
    out, run, used = [], [], 0
    for pos, need in items:
        if run and used + need > budget:
            out.append(run)
            run, used = [], 0
        run.append(pos)
        used += need
    if run:
        out.append(run)
    return out


def offsets(sizes):
    """Start of every item of a packed buffer, and the total."""
    off = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=off[1:])
    return off[:-1], int(off[-1])


def cat(parts, dtype):
    """The parts of a packed host buffer in a row; no parts: an empty array of ``dtype``."""
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def call_args(tables, inputs, outputs):
    """The argument list the host-buffer entries share, after their leading integers:
    ``(count, pointer)`` per descriptor table, then ``(pointer, size)`` per input and output
    buffer -- ``(array, ctype)`` each; an output that is not asked for is ``(None, ctype)``: a
    null pointer of size 0."""
    from . import _lib

    args = []
    for table in tables:
        args += [len(table), table.ctypes.data]
    for arr, ct in list(inputs) + list(outputs):
        args += [_lib.ptr(arr, ct), 0 if arr is None else arr.size]
    return args


class Launcher:
    """Uploads and launches of one chunk through the entries that take device buffers (``(count,
    host table, device table)``, then pointers and sizes, then the stream).  ``launches``: what
    was launched, in order; ``keep``: the tables, alive until the chunk is done (the caller
    synchronises when it fetches its results).  ``pad``: elements of a ``cat`` of nothing.
    ``Launcher.last`` is the one made last."""

    last = None

    def __init__(self, device, pad=0):
        import torch

        from . import _lib

        self.torch, self.lib, self.check = torch, _lib.load(), _lib.check
        self.dev = torch.device("cuda", device)
        self.pad = pad
        self.keep, self.launches = [], []
        Launcher.last = self

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def cat(self, parts, dtype):
        parts = [np.ascontiguousarray(p, dtype).reshape(-1) for p in parts]
        return self.up(np.concatenate(parts) if parts else np.zeros(self.pad, dtype))

    def empty(self, n, dtype):
        return self.torch.empty(max(int(n), 1), dtype=getattr(self.torch, np.dtype(dtype).name),
                                device=self.dev)

    def table(self, table):
        """(count, host pointer, device pointer) of a descriptor table."""
        d_table = self.up(table.reshape(-1).view(np.uint8) if table.size else np.zeros(8, np.uint8))
        self.keep += [table, d_table]
        return [len(table), table.ctypes.data, d_table.data_ptr()]

    def call(self, entry, table, *args, head=(), tag=None):
        """One launch on the current stream of ``entry`` (its name in the library, or the
        function), unless ``table`` is empty: ``head``, the table, then ``args`` -- tensors
        (passed as pointer), further tables or integers -- and the stream.  The log gets
        ``tag`` (default: the entry)."""
        import ctypes

        if not len(table):
            return
        self.launches.append(entry if tag is None else tag)
        fn = getattr(self.lib, entry) if isinstance(entry, str) else entry
        argv = list(head) + self.table(table)
        for a in args:
            if isinstance(a, np.ndarray):
                argv += self.table(a)
            else:
                argv.append(ctypes.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else a)
        stream = ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)
        self.check(fn(*argv, stream))
