"""Communicators of the owner-computes trainer (multike_amd/distributed_oc.py): the three collectives of a global step —
all-gather of the HR / RT vector blocks, reduce-scatter of their gradients, all-reduce of the relation gradient — and the
once-per-epoch exchange of the negative codes (an all-gather; with owner-bucketed codes two small all-gathers and an equal-split
all-to-all), on the SAME communicator (every rank issues every collective in one order).
`OcRcclComm` is the default of the HIP trainers (`default_comm`); `OcGlooComm` and `OcHostStagedComm` serve the tests.

A communicator MAY have `native(tr)`: the mke_oc_comm struct the native step loop (mke_oc_steps) calls its collectives
through.  One that has none is driven by the Python step loop.
"""
import ctypes as C
import os
import traceback
import warnings

import torch
import torch.distributed as dist

from . import _lib, rccl


class OcComm:
    """The three collectives of the step on torch.distributed (RCCL over xGMI on MI355X; gloo in the CPU tests).
    `async_op` returns a work handle whose wait() orders the CURRENT stream after the collective."""

    def __init__(self, group=None):
        self.group = group

    def all_gather(self, out, mine, async_op=False):
        return dist.all_gather_into_tensor(out, mine, group=self.group, async_op=async_op)

    def reduce_scatter(self, out, inp, async_op=False):
        return dist.reduce_scatter_tensor(out, inp, group=self.group, async_op=async_op)

    def all_reduce(self, t, op=None):
        dist.all_reduce(t, group=self.group) if op is None else dist.all_reduce(t, op=op, group=self.group)

    def all_to_all(self, out, inp):
        """Equal split (the epoch plan's owner-bucketed codes): block g of `inp` goes to rank g, block g of `out` comes from rank g."""
        dist.all_to_all_single(out.view(-1), inp.view(-1), group=self.group)

    def all_gather_list(self, parts, mine):
        dist.all_gather(parts, mine, group=self.group)

    def barrier(self, token):
        """Stream-ordered cross-rank barrier (peer-direct mode): a one-element all-reduce — every rank's stream passes it only
        after every rank's stream has reached it; the host is not blocked."""
        dist.all_reduce(token, group=self.group)

    def all_gather_object(self, obj):
        out = [None] * dist.get_world_size(self.group)
        dist.all_gather_object(out, obj, group=self.group)
        return out


class _EventWork:
    """Handle of an asynchronous collective: wait() orders the CURRENT stream after it (no host wait)."""

    def __init__(self, ev):
        self.ev = ev

    def wait(self):
        torch.cuda.current_stream().wait_event(self.ev)


class OcRcclComm(OcComm):
    """The three collectives through RCCL directly (multike_amd/rccl.py), enqueued ON THE CALLER'S STREAM: stream order is the
    dependency, no event and no second stream per collective (torch.distributed's two stream hops per collective cost ~26 us
    of device time and ~30 us of host time each on this part: EXPERIMENTS R5.3).  async_op=True (the chunk-pipelined schedule)
    goes to this communicator's own stream with two pooled events.  The default of the HIP trainers on an "nccl" process
    group; MKE_OC_COMM=torch selects OcComm."""

    def __init__(self, group=None):
        super().__init__(group)
        self.c = rccl.Communicator(group)
        self.c.self_check()                 # all three collectives give the right sums, or raise before any training step
        self._side, self._events, self._k = None, None, 0
        self._native = None                 # the mke_oc_comm over this communicator, built on first use (`native`)

    def _async(self, fn):
        if self._side is None:
            self._side = torch.cuda.Stream()
            self._events = [torch.cuda.Event() for _ in range(64)]
        cur = torch.cuda.current_stream()
        e_in, e_out = self._events[self._k % 64], self._events[(self._k + 1) % 64]
        self._k += 2
        e_in.record(cur)
        self._side.wait_event(e_in)
        fn(self._side)
        e_out.record(self._side)
        return _EventWork(e_out)

    def all_gather(self, out, mine, async_op=False):
        o, m = out.view(-1), mine.reshape(-1)
        if async_op:
            return self._async(lambda st: self.c.all_gather(o, m, st))
        self.c.all_gather(o, m)

    def reduce_scatter(self, out, inp, async_op=False):
        o, i = out.view(-1), inp.view(-1)
        if async_op:
            return self._async(lambda st: self.c.reduce_scatter(o, i, st))
        self.c.reduce_scatter(o, i)

    def all_reduce(self, t, op=None):
        if op is not None:
            return super().all_reduce(t, op)
        self.c.all_reduce(t.view(-1))

    def all_to_all(self, out, inp):
        self.c.all_to_all(out.view(-1), inp.view(-1))

    def barrier(self, token):
        self.c.all_reduce(token.view(-1))

    def native(self, tr=None):
        """mke_oc_comm over this communicator: RCCL's own entry points, called from the native step loop (mke_oc_steps)."""
        if self._native is None:
            L = rccl.lib()
            cs = _lib.OcCommStruct()
            cs.kind, cs.ctx = _lib.OC_COMM_NCCL, self.c._comm.value
            cs.all_gather = C.cast(L.ncclAllGather, C.c_void_p).value
            cs.reduce_scatter = C.cast(L.ncclReduceScatter, C.c_void_p).value
            cs.all_reduce = C.cast(L.ncclAllReduce, C.c_void_p).value
            cs.world, cs.rank = self.c.world, self.c.rank
            self._native = cs
        return self._native

_DEFAULT_RCCL = None        # the process's step communicator over the world: every trainer of a model shares it


def default_comm(device, world, force=False):
    """The communicator a HIP trainer uses when none is given."""
    global _DEFAULT_RCCL
    if device.type == "cuda" and dist.is_initialized() and dist.get_backend() == "nccl" and (world > 1 or force) \
            and os.environ.get("MKE_OC_COMM", "rccl") != "torch":
        if _DEFAULT_RCCL is None or (_DEFAULT_RCCL is not False and _DEFAULT_RCCL.c.world != dist.get_world_size()):
            # every rank tries; the ranks then agree (one torch.distributed all-reduce) on whether ALL of them succeeded — a
            # communicator that came up on some ranks only must not be used by any
            try:
                cand, err = OcRcclComm(), None
            except Exception as e:      # noqa: BLE001 — reported below, the torch.distributed communicator takes over
                cand, err = None, e
            ok = torch.tensor([1 if cand is not None else 0], dtype=torch.int32, device=device)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if int(ok) == 1:
                _DEFAULT_RCCL = cand
            else:
                warnings.warn(f"multike_amd: RCCL through ctypes did not come up on every rank ({err!r} on this one): using torch.distributed for the collectives")
                _DEFAULT_RCCL = False
        if _DEFAULT_RCCL is not False:
            return _DEFAULT_RCCL
    return OcComm() if (device.type == "cuda" or not dist.is_initialized()) else OcGlooComm()


class OcGlooComm(OcComm):
    """gloo has no reduce-scatter: all-reduce the whole buffer and keep this rank's block (CPU tests only)."""

    def all_gather(self, out, mine, async_op=False):
        w = dist.get_world_size(self.group)
        dist.all_gather(list(out.view(w, -1).unbind(0)), mine.reshape(-1), group=self.group)

    def reduce_scatter(self, out, inp, async_op=False):
        w, r = dist.get_world_size(self.group), dist.get_rank(self.group)
        tmp = inp.clone()
        dist.all_reduce(tmp, group=self.group)
        out.copy_(tmp.view(w, -1)[r].view_as(out))

    def all_to_all(self, out, inp):
        """gloo's all_to_all_single on host tensors (what the row exchange of multike_amd/distributed.py goes through)."""
        dist.all_to_all_single(out.view(-1), inp.view(-1), group=self.group)


class OcHostStagedComm(OcGlooComm):
    """Test vehicle: the same collectives on DEVICE tensors through gloo, staged over the host.  Lets two ranks that SHARE
    one GPU run the device kernels with world_size 2 (RCCL refuses two ranks on one device)."""

    def all_gather(self, out, mine, async_op=False):
        o = torch.empty(out.shape, dtype=out.dtype)
        super().all_gather(o, mine.cpu())
        out.copy_(o)

    def reduce_scatter(self, out, inp, async_op=False):
        o = torch.empty(out.shape, dtype=out.dtype)
        super().reduce_scatter(o, inp.cpu())
        out.copy_(o)

    def all_reduce(self, t, op=None):
        c = t.cpu()
        super().all_reduce(c, op)
        t.copy_(c)

    def all_to_all(self, out, inp):
        o = torch.empty(out.shape, dtype=out.dtype)
        super().all_to_all(o, inp.cpu())
        out.copy_(o)

    def all_gather_list(self, parts, mine):
        cp = [torch.empty(p.shape, dtype=p.dtype) for p in parts]
        dist.all_gather(cp, mine.cpu(), group=self.group)
        for p, c in zip(parts, cp):
            p.copy_(c)

    def barrier(self, token):
        torch.cuda.synchronize()           # gloo orders hosts, not streams
        dist.barrier(group=self.group)

    def native(self, tr):
        """mke_oc_comm of kind CALLBACK: the native step loop calls back into these staged collectives (the buffers are found by
        their device address among the trainer's exchange buffers; the callback works on the stream the loop hands it)."""
        def find(addr, count):
            for t in tr._exchange_tensors():
                if t.data_ptr() == addr:
                    return t.view(-1)[:count]
            raise _lib.MultiKEHipError("native callback: unknown exchange buffer")

        def on(stream):
            # the stream the loop enqueues on, as a torch stream: handle 0 is torch's default stream (torch.cuda.ExternalStream(0)
            # is NOT — it makes a stream of its own, and the staged copies then raced the kernels: caught at world 8)
            return torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()

        def move(fn, scale_in, scale_out):
            def cb(ctx, send, recv, count, stream):
                try:
                    with torch.cuda.stream(on(stream)):
                        fn(find(recv, count * scale_out), find(send, count * scale_in))
                    return 0
                except Exception:      # noqa: BLE001 — an exception must not unwind through the C frame
                    traceback.print_exc()
                    return 1
            return _lib.OC_CB_MOVE(cb)

        def reduce(ctx, buf, count, stream):
            try:
                with torch.cuda.stream(on(stream)):
                    self.all_reduce(find(buf, count))
                return 0
            except Exception:          # noqa: BLE001
                traceback.print_exc()
                return 1

        G = dist.get_world_size(self.group)
        keep = (move(self.all_gather, 1, G), move(self.reduce_scatter, G, 1), _lib.OC_CB_REDUCE(reduce))
        cs = _lib.OcCommStruct()
        cs.kind = _lib.OC_COMM_CALLBACK
        cs.all_gather, cs.reduce_scatter, cs.all_reduce = (C.cast(f, C.c_void_p).value for f in keep)
        cs.world, cs.rank = G, dist.get_rank(self.group)
        cs._keep = keep                # the thunks live as long as the struct
        return cs
