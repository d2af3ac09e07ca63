"""Leaf stream: a second, lowest-priority HIP stream per device for the gradient kernels nothing else in the backward pass waits for.

A weight / bias gradient that goes straight into the flat optimizer's .grad (FlatAdamW.sink) is a LEAF of the step's dependency graph: its
next reader is the optimizer (or a bucket all-reduce).  `with leaf_work(dev, use, *operands):` enqueues the kernels launched inside on the
device's leaf stream, ordered after everything on the current stream so far; leaf_join (end of backward(), optimizer step) makes the
current stream wait for them, leaf_fence orders a bucket all-reduce behind both streams.  Measurements and history: DESIGN.md section 4.

* One writer per target.  A block writes only what the compute stream does not touch before the join: .grad views of the flat optimizer.
  Same kernels, same operands, same order per target: bit-identical to the single-stream run, which is SET_AMD_LEAF_STREAM=0.
* Operands are held.  Every tensor a leaf kernel READS is passed to leaf_work and stays referenced in the stream's OperandLedger, so the
  caching allocator cannot hand its storage to a compute-stream kernel that might run before the leaf kernel has read it (nor does the
  autograd engine accumulate into it in place: that needs the last reference).  One left out is a use-after-free race between the
  streams.  Entries are released once their kernels have RUN: by a marker event recorded every SET_AMD_LEAF_MARK_MB (128) MB of newly
  held storage and polled (non-blocking) at the next fork, or by a join.  Above SET_AMD_LEAF_KEEP_MB (8192; 0: no accounting, held until
  the join) MB of held storage the compute stream joins early: the bound.
* Nothing is allocated inside a block: torch's current stream is unchanged there (only ops._stream(), our kernels' launch stream, moves),
  so the compute stream would own what the leaf stream uses.  A per-stream scratch buffer regrown inside goes to hold_until_join.
* Blocks do not nest (ops._STREAM_TLS.leaf is the open block's stream); a block left by an exception records no marker.
* Join before the next reader: the first block of every backward pass (graph task) queues leaf_join as an engine callback; a pass that
  raises runs no callbacks, so FlatAdamW.zero_grad() / step() / abort_step() join as well.  tests/stream_audit.py checks all of the above
  call by call on the recorded sequence of library calls.
"""
import collections
import ctypes as C
import os

import torch

from . import _lib, ops
from ._lib import check
from .ops import _stream

L = _lib.lib

_MARK_SLOTS = 8  # outstanding markers per stream: slots 8 * (idx % 8) .. + 7 of set_stream_mark


class OperandLedger:
    """What a stream's queued kernels still read: a FIFO of held entries, and the bytes of the distinct storages behind them (operands are
    often views of one saved buffer -- every layer's slice of a [L, B, C, T] tensor -- so bytes are counted per storage, once).  Pure
    host bookkeeping: no library or GPU call.  cap_bytes == 0: no byte accounting at all, entries are still held."""

    def __init__(self, mark_bytes, cap_bytes):
        self.mark_bytes, self.cap_bytes = mark_bytes, cap_bytes
        self.entries = collections.deque()  # (object, [(storage address, bytes)] or None)
        self.storages = {}                  # storage address -> [references among the entries, bytes]
        self.count = self.base = 0          # entries ever held / ever released: entries[i] is number base + i
        self.bytes = self.unmarked = 0      # held storage / the part of it that arrived since the last marker
        self.peak_bytes = 0

    def hold(self, obj):
        """Keep obj (a tensor, or tuples / lists of tensors, nested) referenced."""
        keys = None
        if self.cap_bytes:
            keys, stor = [], self.storages
            _storages(obj, keys)
            for k, n in keys:
                ent = stor.get(k)
                if ent is None:
                    stor[k] = [1, n]
                    self.bytes += n
                    self.unmarked += n
                else:
                    ent[0] += 1
            if self.bytes > self.peak_bytes:
                self.peak_bytes = self.bytes
        self.entries.append((obj, keys))
        self.count += 1

    def over_cap(self):
        return self.cap_bytes and self.bytes > self.cap_bytes

    def mark_due(self):
        return self.unmarked >= self.mark_bytes

    def mark(self):
        """A marker now covers everything held so far: returns the count to release up to once it has completed."""
        self.unmarked = 0
        return self.count

    def release_upto(self, count):
        """Drop the entries held before `count` (oldest first); returns how many."""
        n, entries, stor = 0, self.entries, self.storages
        while self.base < count:
            _, keys = entries.popleft()
            self.base += 1
            n += 1
            for k, nb in keys or ():
                ent = stor.get(k)
                if ent is not None:
                    ent[0] -= 1
                    if ent[0] <= 0:
                        del stor[k]
                        self.bytes -= nb
        return n

    def release_all(self):
        self.entries.clear()
        self.storages.clear()
        self.base, self.bytes, self.unmarked = self.count, 0, 0


def _storages(obj, out):
    if isinstance(obj, torch.Tensor):
        s_ = obj.untyped_storage()
        out.append((s_.data_ptr(), s_.nbytes()))
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            _storages(o, out)


def _mb_env(name, default):
    try:
        return max(0, int(os.environ.get(name, default))) << 20
    except ValueError:
        return int(default) << 20


class LeafStream:
    """The leaf stream of one device: raw handle (what the kernels are launched on), torch wrapper (what leaf_fence hands out), whether
    work is pending since the last join, the operand ledger and the queue of outstanding markers.  Lowest priority: its chip-filling
    GEMMs yield workgroup slots to the compute stream's short kernels.  Never destroyed."""

    def __init__(self, idx):
        self.idx, self.raw = idx, C.c_void_p()
        with torch.cuda.device(idx):
            check(L().set_stream_create_low_priority(C.byref(self.raw)), "set_stream_create_low_priority")
        self.stream = torch.cuda.ExternalStream(self.raw.value, device=torch.device("cuda", idx))
        self.dirty = False
        self.joined_task = -1  # graph task (backward pass) whose end-of-pass join is queued
        self.ledger = OperandLedger(_mb_env("SET_AMD_LEAF_MARK_MB", 128), _mb_env("SET_AMD_LEAF_KEEP_MB", 8192))
        self.marks = collections.deque()  # (marker slot, ledger count it covers), oldest first
        self.released_by_marker = self.early_joins = 0

    # one C call on a cached event per direction (torch's Event / Stream.wait_event / record_stream wrappers cost ~28 us per fork)
    def fork(self):
        """The leaf stream waits for everything enqueued on the current stream so far."""
        check(L().set_stream_order(_stream(), self.raw, 2 * self.idx), "set_stream_order")

    def join(self):
        """The current stream waits for everything enqueued on the leaf stream so far."""
        check(L().set_stream_order(self.raw, _stream(), 2 * self.idx + 1), "set_stream_order")

    def poll(self):
        """Release the operands whose kernels have finished (markers that completed); non-blocking."""
        marks = self.marks
        while marks and L().set_stream_mark_done(marks[0][0]) == 1:
            self.released_by_marker += self.ledger.release_upto(marks.popleft()[1])

    def mark(self):
        """After the kernels of a block have been enqueued: a marker, once enough new operands are held and a slot is free."""
        marks = self.marks
        if not self.ledger.mark_due() or len(marks) >= _MARK_SLOTS:
            return
        busy = {m[0] for m in marks}
        first = _MARK_SLOTS * (self.idx % 8)
        slot = next(s for s in range(first, first + _MARK_SLOTS) if s not in busy)
        check(L().set_stream_mark(self.raw, slot, self.idx), "set_stream_mark")
        marks.append((slot, self.ledger.mark()))

    def release_all(self):
        self.marks.clear()
        self.ledger.release_all()


_STREAMS = {}  # device index -> LeafStream (created at the device's first block)


def leaf_enabled():
    return os.environ.get("SET_AMD_LEAF_STREAM", "1") != "0"


def leaf_stats(reset=False):
    """{"max_keep_bytes", "released_by_marker", "early_joins"} since the last reset (tests / probes)."""
    sts = _STREAMS.values()
    out = {"max_keep_bytes": max((s.ledger.peak_bytes for s in sts), default=0),
           "released_by_marker": sum(s.released_by_marker for s in sts), "early_joins": sum(s.early_joins for s in sts)}
    if reset:
        for s in sts:
            s.ledger.peak_bytes = s.released_by_marker = s.early_joins = 0
    return out


class leaf_work:
    """with leaf_work(device, use, *tensors) as on_leaf: kernels launched inside (ops._stream()) go to the device's leaf stream, ordered
    after everything enqueued on the current stream so far, when `use` holds.  `tensors`: everything those kernels read (see the module
    comment); nothing may be allocated inside."""

    def __init__(self, dev, use, *tensors):
        self.on = bool(use) and dev.type == "cuda" and leaf_enabled() and getattr(ops._STREAM_TLS, "leaf", None) is None
        self.dev, self.tensors = dev, tensors

    def __enter__(self):
        if not self.on:
            return False
        idx = self.dev.index if self.dev.index is not None else torch.cuda.current_device()
        st = _STREAMS.get(idx)
        if st is None:
            st = _STREAMS[idx] = LeafStream(idx)
        if st.marks:
            st.poll()
        if st.ledger.over_cap():  # the bound: the compute stream waits for the leaf stream, everything held so far is released
            st.join()
            st.release_all()
            st.early_joins += 1
        st.fork()
        st.ledger.hold(self.tensors)
        ops._STREAM_TLS.leaf = st.raw
        self._st = st
        st.dirty = True
        # The stream that ran backward() waits for the leaf stream when the pass is over: callers may read .grad right away.  Once per
        # backward pass, keyed by the engine's graph task and not by `dirty`: a pass that raised never ran its callbacks, and a block
        # opened outside a pass queued none -- both leave `dirty` set, and the next pass must still end with its join.
        task = torch._C._current_graph_task_id()
        if task != -1 and task != st.joined_task:  # (-1: not inside a backward pass -- a test calling a backward function by hand;
            st.joined_task = task                  # FlatAdamW.step() / abort_step() join)
            torch.autograd.Variable._execution_engine.queue_callback(leaf_join)
        return True

    def __exit__(self, *exc):
        if self.on:
            ops._STREAM_TLS.leaf = None
            if exc[0] is None:
                self._st.mark()
        return False


def leaf_join():
    """The current stream waits for everything enqueued on the leaf streams (before the optimizer reads the gradients); the operands
    held for the leaf kernels are released (whatever reuses their storage is ordered after this point)."""
    for idx, st in _STREAMS.items():
        if st.dirty:
            with torch.cuda.device(idx):
                st.join()
            st.dirty = False
            st.release_all()


def leaf_fence(dev):
    """For a consumer that must see BOTH streams' work without stalling the compute stream (a bucket all-reduce launched from an autograd
    hook): returns the leaf stream (torch object) after making it wait for the current stream, or None when no leaf work is pending."""
    st = _STREAMS.get(dev.index if dev.index is not None else torch.cuda.current_device()) if dev.type == "cuda" else None
    if st is None or not st.dirty:
        return None
    st.fork()
    return st.stream


def hold_until_join(buf):
    """A scratch buffer replaced while the leaf stream is the launch stream: kernels queued there may still use it."""
    if getattr(ops._STREAM_TLS, "leaf", None) is not None:
        for st in _STREAMS.values():
            if st.dirty:
                st.ledger.hold(buf)
