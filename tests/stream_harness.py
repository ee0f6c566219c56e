"""The late-producer harness of test_gpu_streams.py (a plain helper, no tests here).

An entry point that honours `stream` must see what that stream holds in front of it and nothing else.  The harness makes that
visible: the inputs sit on the device as POISON (valid for the kernel, different from the real inputs), and on a non-blocking side
stream a delay runs in front of the copies that put the real inputs in place.  Work that the entry point enqueues anywhere but on
that stream -- the null stream, a lane that was not forked behind it -- runs while the delay still spins and reads the poison; an
output that is not ready behind the stream (a lane that was not joined) is cloned as the sentinel; a host table that is read after
the call returned is read after it was overwritten.  Nothing here can fault a kernel: every wrong outcome is a wrong value."""
import ctypes as C

import numpy as np
import torch

FILLS = (0xA5, 0x00, 0xFF)                     # workspace bytes on entry: "unspecified" means any of these gives the same result
SEG = np.dtype([("start", "<i8"), ("end", "<i8"), ("label", "<i4"), ("contig", "<i4")])


def dev_of(a, dev):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)                 # (a copy: buffers of bytes objects are read-only)


def raw_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Harness:
    """One per module: the side-stream pool, the delay, and the two call protocols (asynchronous / synchronising)."""

    def __init__(self, dev):
        self.dev = dev
        self.pool = [torch.cuda.Stream(device=dev) for _ in range(4)]          # torch's pool streams are non-blocking
        self.side = None
        self.control = None                                                   # what the positive control read per stream
        self._mm = None
        self._cycles = None
        self._calibrate()

    # ---- the delay -------------------------------------------------------------------------------------------------
    def _calibrate(self, want_ms=40.0):
        """Size the delay to about `want_ms` on this device.  The length is not a pass criterion: the query() assertions of the
        protocols prove that it was long enough for the call they bracket."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(1000)                                            # load the kernel
            torch.cuda.synchronize()
            probe = 2_000_000
            ev0.record()
            torch.cuda._sleep(probe)
            ev1.record()
            torch.cuda.synchronize()
            ms = max(ev0.elapsed_time(ev1), 1e-3)
            self._cycles = int(min(max(probe * want_ms / ms, 1e5), 4e9))
            return
        self._mm = torch.randn((4096, 4096), device=self.dev)
        torch.mm(self._mm, self._mm)
        torch.cuda.synchronize()
        ev0.record()
        torch.mm(self._mm, self._mm)
        ev1.record()
        torch.cuda.synchronize()
        self._reps = int(min(max(want_ms / max(ev0.elapsed_time(ev1), 1e-3), 1), 2000))

    def delay(self):
        """Enqueue the delay on the CURRENT torch stream."""
        if self._cycles is not None:
            torch.cuda._sleep(self._cycles)
            return
        x = self._mm
        for _ in range(self._reps):
            x = torch.mm(self._mm, x).clamp_(-1, 1)

    # ---- the positive control ------------------------------------------------------------------------------------------
    def choose_side(self, L):
        """dgrp_encode on the NULL stream while its producer sits behind the delay on a side stream: the trap works on that pair of
        streams when the output is the poison's encoding.  The first pool stream for which it is becomes `side` (two streams that
        share a hardware queue would serialise and hide the race)."""
        n = 4096
        real = np.frombuffer(b"ACGT" * (n // 4), np.uint8)
        poison = np.full(n, ord("N"), np.uint8)
        d_real, d_poison = dev_of(real, self.dev), dev_of(poison, self.dev)
        self.control = []
        for k, st in enumerate(self.pool):
            d_seq = d_poison.clone()
            d_idx = torch.full((n,), 0x77, dtype=torch.uint8, device=self.dev)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                self.delay()
                d_seq.copy_(d_real)
            rc = L.dgrp_encode(d_seq.data_ptr(), n, d_idx.data_ptr(), None)    # the mistake the harness is there to catch
            busy = not st.query()
            torch.cuda.synchronize()
            got = d_idx.cpu().numpy()
            tripped = rc == 0 and busy and bool((got == 4).all())
            self.control.append({"stream": k, "rc": rc, "producer_still_delayed": busy, "read_poison": bool((got == 4).all()),
                                 "read_real": bool((got == np.tile(np.arange(4, dtype=np.uint8), n // 4)).all())})
            if tripped and self.side is None:
                self.side = st
        return self.side

    # ---- buffers ---------------------------------------------------------------------------------------------------
    def work(self, nbytes, fill):
        return torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device=self.dev)

    # ---- the protocols ---------------------------------------------------------------------------------------------
    def run(self, call, inputs, outputs, work_bytes=0, fill=0xA5, sync=False, tables=None, drained=True):
        """call(bufs, work, stream, tables) -> (rc, host results); bufs: name -> device tensor.
        inputs:  name -> (real, poison) numpy arrays of one shape and dtype (an in/out buffer is an input that is also named in
                 `outputs` with None);
        outputs: name -> numpy array of sentinels (or None for an in/out buffer);
        tables:  name -> numpy host table; scribbled with zeros (offsets 0, lengths 0: in range for every kernel) right after a
                 synchronising call returns.
        Runs the call on the idle default stream, then late-produced on the side stream, and returns (outputs of the late run as
        numpy arrays, its host results, outputs of the idle run, its host results).  sync=False: the call must return while
        the stream still holds the delay.  sync=True: the delay must still run just before the call; `drained`: the stream must be
        empty when it returns (its last act is the synchronisation)."""
        assert self.side is not None, "no side stream passed the positive control"
        dev, tables = self.dev, tables or {}
        real = {k: dev_of(v[0], dev) for k, v in inputs.items()}
        poison = {k: dev_of(v[1], dev) for k, v in inputs.items()}
        for k, (r, p) in inputs.items():
            assert r.shape == p.shape and r.dtype == p.dtype and not np.array_equal(r, p), f"{k}: poison must differ from the real input"
        out_names = list(outputs)

        def fresh(src):
            bufs = {k: src[k].clone() for k in inputs}
            for k, v in outputs.items():
                if v is not None:
                    bufs[k] = dev_of(v, dev)
            return bufs

        def host(bufs):
            return {k: bufs[k].cpu().numpy() for k in out_names}

        # the idle default stream: the statement every existing test already checks, and the warm-up (module loading is not timed)
        bufs = fresh(real)
        wk = self.work(work_bytes, fill)
        tabs = {k: v.copy() for k, v in tables.items()}
        rc, idle_host = call(bufs, wk, None, tabs)
        torch.cuda.synchronize()
        assert rc == 0, f"idle call failed: {rc} {last_error()}"
        idle = host(bufs)

        # the late producer
        bufs = fresh(poison)
        wk = self.work(work_bytes, fill)
        tabs = {k: v.copy() for k, v in tables.items()}
        torch.cuda.synchronize()
        side = self.side
        with torch.cuda.stream(side):
            self.delay()
            for k in inputs:
                bufs[k].copy_(real[k])
            busy_before = not side.query()
            rc, late_host = call(bufs, wk, side.cuda_stream, tabs)
            busy_after = not side.query()
            for t in tabs.values():
                t[...] = 0
            clones = {k: bufs[k].clone() for k in out_names}
            for k in inputs:
                bufs[k].copy_(poison[k])
        side.synchronize()
        torch.cuda.synchronize()
        assert rc == 0, f"late call failed: {rc} {last_error()}"
        if sync:
            assert busy_before, "the delay had ended before the call: it proves nothing"
            if drained:
                assert not busy_after, "documented to synchronise the stream, but returned with work still on it"
        else:
            assert busy_after, "documented asynchronous, but the stream was idle when it returned: it synchronised (or the delay is too short)"
        late = {k: clones[k].cpu().numpy() for k in out_names}
        for k in out_names:
            np.testing.assert_array_equal(raw_bytes(late[k]), raw_bytes(idle[k]), err_msg=f"{k}: late producer on the side stream != idle default stream")
        return late, late_host, idle, idle_host


def last_error():
    from deepgrp_amd._lib import lib
    return lib().dgrp_last_error().decode("utf-8", "replace")


def i64ptr(a):
    assert a.dtype == np.int64 and a.flags.c_contiguous
    return a.ctypes.data


def segs(rows):
    """[(start, end, label, contig)] -> SEG array"""
    a = np.zeros(len(rows), SEG)
    for i, r in enumerate(rows):
        a[i] = tuple(r)
    return a


def c_i64():
    return C.c_int64(-12345)
