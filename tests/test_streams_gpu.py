"""Caller-stream ordering and concurrent use of the state the library shares between calls.

include/vcf_amd.h promises that every entry enqueues on `stream`, is asynchronous
and keeps no reference after it returns, while vcf_dct_any.hip keeps two scratch
buffers per device (ordered by one re-recorded event each), vcf_pipeline.h one
set of library streams and fork / join events per translation unit, and several
tables are uploaded once per process.  The rows of tests/stream_cases.py reach
each of them; here they run on non-blocking caller streams with other work
queued in front and behind, from two streams, from two threads and as the first
call of a process, and every output must equal the oracle's bit for bit.

The delay that keeps a stream busy while the host enqueues is k fills of one
large buffer (vcf_memset), sized once per module from a measured fill and a
measured enqueue; every ordering test measures its own delay with two events
and fails as inconclusive, never passes, when the host was not done first.  The
one place where the host cannot be first is the call that grows a scratch
buffer (it waits on the host for the buffer's last user): the growth test
asserts there that the call began inside the delay and returned after it.
"""
import math
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import stream_cases as C
from abi_buffers import Guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 512 << 20        # the delay's buffer
SLACK = 64             # bytes past a row's output extent that must keep their fill
MARGIN = 4             # the delay is sized to at least MARGIN x the slowest enqueue ...
MIN_DELAY_MS = 3.0     # ... and to at least this: an enqueue of 0.1 ms can take ten times as long on a busy host
FIRST_DELAY_MS = 120.0 # the first-call test's: the first launch of a process loads the code objects (28 ms measured)
FIRST_BIG = 4 * BIG    # ... in fills of a larger buffer, so that it stays a few hundred commands


def _L():
    import vcf_amd._lib as L
    return L


class Bufs:
    """A row's device buffers: stage = real, stage2 = decoy, din, the constant inputs, snap, the caller
    workspace (its own buffer) and, made anew by reset(), the guarded output."""

    def __init__(self, row):
        from vcf_amd.device import DeviceBuffer
        self.row = row
        self.n_in, self.n_out = row.real.nbytes, row.out_bytes
        self.stage, self.stage2 = DeviceBuffer.from_array(row.real), DeviceBuffer.from_array(row.decoy)
        self.din, self.snap = DeviceBuffer(self.n_in), DeviceBuffer(self.n_out)
        self.extras = [DeviceBuffer.from_array(e) for e in row.extras]
        self.ws = DeviceBuffer(row.ws_bytes()) if row.ws_bytes() else None
        self.out = None

    def reset(self, din="decoy"):
        """din = the decoy (or the real input), output and snapshot 0xEE, workspace 0xFF; all of it done."""
        from vcf_amd.device import synchronize
        self.din.upload(self.row.decoy if din == "decoy" else self.row.real)
        self.out = Guarded(self.n_out + SLACK)
        self.out.upload(np.full(self.n_out, 0xEE, np.uint8))
        self.snap.fill(0xEE)
        if self.ws is not None:
            self.ws.fill(0xFF)
        synchronize()

    def call(self, stream):
        self.row.call(_L(), self.din.ptr.value, self.out.ptr.value, self.ws.ptr.value if self.ws else 0,
                      [e.ptr.value for e in self.extras], stream.handle)

    def free(self):
        for b in [self.stage, self.stage2, self.din, self.snap, self.ws] + self.extras:
            if b is not None:
                b.free()


def _mismatch(row, got, what):
    """None, or how `got` (the bytes of an output blob) differs from the oracle's output for `real`."""
    want, mask = row.expected()
    bad = got != want if mask is None else (got != want) & mask
    if not bad.any():
        return None
    idx = np.flatnonzero(bad)
    decoy, _ = row.expected("decoy")
    as_decoy = float(np.mean(got[idx] == decoy[idx])) if decoy.size == got.size else 0.0
    return (f"{row.name} {what}: {idx.size} of {got.size} bytes differ from the oracle, first at {int(idx[0])}; "
            f"{int(np.count_nonzero(got[idx] == 0xEE))} of them still 0xEE, {as_decoy:.2f} equal to the decoy's output")


def _ordered(b, S, big, k):
    """The ordering sequence on stream S with no host wait in between: delay, din <- real, the entry,
    snap <- out, din <- decoy, delay.  -> (delay in ms by two events, host ms from the first enqueue to
    the last one in front of the second delay)."""
    from vcf_amd.device import Event, copy_dtod
    e0, e1 = Event(), Event()
    b.reset("decoy")
    t0 = time.perf_counter()
    e0.record(S)
    for _ in range(k):
        big.fill(0x5A, S)
    e1.record(S)
    copy_dtod(b.din, 0, b.stage, 0, b.n_in, S)
    b.call(S)
    copy_dtod(b.snap, 0, b.out.buf, b.out.start, b.n_out, S)
    copy_dtod(b.din, 0, b.stage2, 0, b.n_in, S)
    host_ms = (time.perf_counter() - t0) * 1e3
    for _ in range(k):
        big.fill(0xA5, S)
    S.synchronize()
    return e0.elapsed_ms(e1), host_ms


def _check_ordered(b):
    """snap and the output equal the oracle's output for `real`, nothing outside the output extent was
    written, and din holds the decoy again."""
    row = b.row
    snap = b.snap.download(np.empty(b.n_out, np.uint8))
    assert _mismatch(row, snap, "snapshot") is None, _mismatch(row, snap, "snapshot")
    out = b.out.download()[:b.n_out]
    assert _mismatch(row, out, "output") is None, _mismatch(row, out, "output")
    b.out.check_outside([(0, b.n_out)], row.name)
    b.out.check(row.name)
    din = b.din.download(np.empty(b.n_in, np.uint8))
    assert np.array_equal(din, row.decoy.view(np.uint8).reshape(-1)), "din does not hold the decoy again"


def _warm(b, S):
    """One call on the idle stream: a scratch buffer that has to grow blocks the host until its last
    user is done (Scratch::acquire), which an ordering sequence could not tell from a late enqueue."""
    b.reset("real")
    b.call(S)
    S.synchronize()


SIZING_ROWS = ("dwt_encode_pipe", "dwt_decode_pipe", "zlib_strips", "dct16_decode_large", "dct191_encode")


@pytest.fixture(scope="module")
def gpu():
    """Stream, the delay's buffer and its size k: one fill timed by two events, the slowest row's whole
    sequence timed on the idle stream by the host, k fills >= MARGIN x that enqueue time."""
    from vcf_amd.device import DeviceBuffer, Event, Stream, set_device
    set_device(0)
    S, big = Stream(), DeviceBuffer(BIG)
    big.fill(0, S)
    S.synchronize()
    e0, e1, n = Event(), Event(), 8
    e0.record(S)
    for _ in range(n):
        big.fill(1, S)
    e1.record(S)
    S.synchronize()
    fill_ms = e0.elapsed_ms(e1) / n
    bufs, enq = {}, {}
    for name in SIZING_ROWS:
        b = bufs[name] = Bufs(C.by_name(name))
        _warm(b, S)
        enq[name] = min(_ordered(b, S, big, 0)[1] for _ in range(2))
    k = max(4, math.ceil(max(MARGIN * max(enq.values()), MIN_DELAY_MS) / fill_ms))
    print(f"\ndelay sizing: one fill of {BIG >> 20} MiB {fill_ms:.3f} ms; enqueue of a whole sequence "
          + ", ".join(f"{n} {v:.3f} ms" for n, v in enq.items()) + f"; k = {k} fills = {k * fill_ms:.2f} ms")
    assert k <= 2000, f"a fill of {fill_ms:.4f} ms is too short a unit for an enqueue of {max(enq.values()):.2f} ms"
    state = dict(S=S, big=big, k=k, fill_ms=fill_ms, enq=enq, bufs=bufs)
    yield state
    for b in state["bufs"].values():
        b.free()
    big.free()


def _bufs(gpu, name):
    if name not in gpu["bufs"]:
        gpu["bufs"][name] = Bufs(C.by_name(name))
    return gpu["bufs"][name]


# ---- (a) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_entry_is_ordered_within_its_stream(gpu, name):
    """An entry that did not start behind the caller's stream (a missing fork wait, a copy or memset on
    another stream) reads the decoy that din holds until the delay is over; one whose library streams
    are not joined before the stream goes on leaves the snapshot 0xEE or reads the decoy written back."""
    b, S = _bufs(gpu, name), gpu["S"]
    _warm(b, S)
    delay_ms, host_ms = _ordered(b, S, gpu["big"], gpu["k"])
    print(f"{name}: delay {delay_ms:.2f} ms, host enqueue {host_ms:.3f} ms")
    _check_ordered(b)
    assert delay_ms > host_ms, (f"inconclusive: the delay of {delay_ms:.2f} ms was over before the host had "
                                f"enqueued the sequence ({host_ms:.2f} ms)")


# ---- (b), (d): fresh processes ------------------------------------------------------------------------
def _child(func, *args, timeout=120):
    code = (f"import sys; sys.path[:0] = [{os.path.join(ROOT, 'tests')!r}, {ROOT!r}]\n"
            f"import test_streams_gpu as T\nT.{func}(*{args!r})\n")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]


def child_scratch_grows(k):
    """Body of test_scratch_grows_under_queued_work (a process whose scratch buffers do not exist yet)."""
    from vcf_amd.device import DeviceBuffer, Event, Stream, set_device, synchronize
    L = _L()
    set_device(0)
    A, B, big = Stream(), Stream(), DeviceBuffer(BIG)
    small, large, enc7, dec7, enc191 = (C.by_name(n) for n in ("dct16_decode_small", "dct16_decode_large",
                                                                "dct7_encode", "dct7_decode", "dct191_encode"))
    # Scratch::acquire per step.  Pass 1: the warm call creates the decode scratch at the small size.
    #   A small   wait only (queued behind the delay)
    #   B large   GROWS the decode scratch: waits on the host for A's event, frees, allocates
    #   A small   wait only, behind B's release
    #   B enc7    run-time scratch: created and grown (float)
    #   A dec7    run-time scratch GROWS (double: twice enc7's bytes); decode scratch wait only
    #   B enc191  run-time scratch GROWS (Bluestein workspace)
    # Pass 2: every step wait only; nothing blocks the host, so the delay must outlast the whole enqueue.
    steps = [(A, small), (B, large), (A, small), (B, enc7), (A, dec7), (B, enc191)]
    ins = [DeviceBuffer.from_array(r.real) for _, r in steps]
    outs = [DeviceBuffer(r.out_bytes) for _, r in steps]
    warm_out = DeviceBuffer(small.out_bytes)
    small.call(L, ins[0].ptr.value, warm_out.ptr.value, 0, [], A.handle)
    A.synchronize()
    big.fill(0, A)
    A.synchronize()
    for p in (1, 2):
        for o in outs:
            o.fill(0xEE)
        synchronize()
        e0, e1 = Event(), Event()
        t0 = time.perf_counter()
        e0.record(A)
        for _ in range(k):
            big.fill(p, A)
        e1.record(A)
        marks = []
        for (s, row), i, o in zip(steps, ins, outs):
            marks.append((time.perf_counter() - t0) * 1e3)
            row.call(L, i.ptr.value, o.ptr.value, 0, [], s.handle)
        host_ms = (time.perf_counter() - t0) * 1e3
        A.synchronize()
        B.synchronize()
        delay_ms = e0.elapsed_ms(e1)
        print(f"pass {p}: delay {delay_ms:.2f} ms; host ms at each enqueue {[round(m, 3) for m in marks]}, "
              f"all enqueued at {host_ms:.3f}")
        bad = [m for m in (_mismatch(row, o.download(np.empty(row.out_bytes, np.uint8)), f"pass {p} step {n}")
                           for n, ((_, row), o) in enumerate(zip(steps, outs))) if m]
        assert not bad, bad
        if p == 1:
            assert delay_ms > marks[1], f"inconclusive: A's delay ({delay_ms:.2f} ms) was over before the growing call"
            # not an ordering property: proof that the grow path ran.  Today's Scratch::acquire waits on
            # the host before it frees; a growth that did not block (a stream-ordered free) would be
            # correct too, and would need this line and pass 1's comments changed, nothing else
            assert host_ms > delay_ms, ("the growing call returned before A's delay was over: either the scratch "
                                        "did not grow in this pass, or growing no longer blocks the host (then "
                                        "this check of the grow path is out of date, not the library wrong)")
        else:
            assert delay_ms > host_ms, f"inconclusive: delay {delay_ms:.2f} ms, host {host_ms:.2f} ms"
    # Pass 3: users of one scratch buffer on two streams that become runnable at the same moment.  B waits
    # for an event recorded behind A's delay, then the calls alternate A, B, A, B ...: the same entry and
    # shape on both streams, A on the real input and B on the decoy, so both write all of the same scratch
    # bytes.  Only the event chain of acquire / release keeps one call's two passes (or its workgroups'
    # lines) from the other's; all of it is enqueued while the delay runs.
    reps = 4
    for row in (large, enc191):
        a_in, b_in = DeviceBuffer.from_array(row.real), DeviceBuffer.from_array(row.decoy)
        a_out, b_out = ([DeviceBuffer(row.out_bytes) for _ in range(reps)] for _ in range(2))
        for o in a_out + b_out:
            o.fill(0xEE)
        synchronize()
        e0, e1 = Event(), Event()
        t0 = time.perf_counter()
        e0.record(A)
        for _ in range(k):
            big.fill(3, A)
        e1.record(A)
        B.wait_event(e1)
        for r in range(reps):
            row.call(L, a_in.ptr.value, a_out[r].ptr.value, 0, [], A.handle)
            row.call(L, b_in.ptr.value, b_out[r].ptr.value, 0, [], B.handle)
        host_ms = (time.perf_counter() - t0) * 1e3
        A.synchronize()
        B.synchronize()
        delay_ms = e0.elapsed_ms(e1)
        print(f"pass 3 {row.name}: delay {delay_ms:.2f} ms, all enqueued at {host_ms:.3f} ms")
        want_b = row.expected("decoy")[0]
        bad = [m for m in (_mismatch(row, o.download(np.empty(row.out_bytes, np.uint8)), f"pass 3 A call {r}")
                           for r, o in enumerate(a_out)) if m]
        for r, o in enumerate(b_out):
            got = o.download(np.empty(row.out_bytes, np.uint8))
            if not np.array_equal(got, want_b):
                bad.append(f"{row.name} pass 3 B call {r}: {int(np.count_nonzero(got != want_b))} of {got.size} bytes "
                           "differ from the oracle's output for the decoy")
        assert not bad, bad
        assert delay_ms > host_ms, f"inconclusive: delay {delay_ms:.2f} ms, host {host_ms:.2f} ms"
        for o in [a_in, b_in] + a_out + b_out:
            o.free()
    print("scratch ok")


def test_scratch_grows_under_queued_work(gpu):
    """One host thread, streams A and B, the shared scratch buffers growing while an earlier launch that
    holds the old pointer is still queued behind A's delay; twice, the second pass on the grown buffers;
    then calls on both streams that become runnable together and write the same scratch bytes.
    In a process of its own: this one's scratch has whatever size earlier tests left."""
    _child("child_scratch_grows", gpu["k"])


def child_first_call(k, folder):
    """Body of test_first_call_of_a_process_on_a_caller_stream."""
    from vcf_amd.device import Stream
    S = Stream()                                   # the first library work of the process
    from vcf_amd.device import DeviceBuffer
    big = DeviceBuffer(FIRST_BIG)
    big.fill(0, S)
    S.synchronize()

    def load(name):
        z = np.load(os.path.join(folder, name + ".npz"))
        row = C.by_name(name)
        row.preload(z["real"], z["decoy"], [z[f"extra{i}"] for i in range(int(z["n_extras"]))], z["want"],
                    z["mask"] if z["mask"].size else None, z["want_decoy"])
        return Bufs(row)

    for n, name in enumerate(C.FIRST_CALL):
        b = load(name)
        delay_ms, host_ms = _ordered(b, S, big, k)   # no warm call: this is the first
        print(f"{name}: delay {delay_ms:.2f} ms, host enqueue {host_ms:.3f} ms")
        _check_ordered(b)
        assert delay_ms > host_ms, (f"inconclusive: {name}: the delay of {delay_ms:.2f} ms was over before the host "
                                    f"had enqueued the sequence ({host_ms:.2f} ms)")
        b.free()
        if n == 0:
            # both scratch buffers grown on the idle stream, by a length no row here uses (FIRST_CALL_WARM):
            # a first call that had to grow one would wait on the host for the delay in front of it
            w = load(C.FIRST_CALL_WARM)
            _warm(w, S)
            out = w.out.download()[:w.n_out]
            assert _mismatch(w.row, out, "warm call") is None, _mismatch(w.row, out, "warm call")
            w.free()
    print("first calls ok")


def test_first_call_of_a_process_on_a_caller_stream(gpu, tmp_path):
    """A fresh interpreter whose first library work creates a Stream; behind a delay on it, the first
    user of the twiddle tables, a run-time plan, the -p weights, the MDCT tables, a DWT filter bank and
    a LloydMax edge table, each through the ordering sequence, against arrays this process wrote.  The
    delay is FIRST_DELAY_MS, not the module's: a first call keeps the host for milliseconds."""
    for name in C.FIRST_CALL + (C.FIRST_CALL_WARM,):
        row = C.by_name(name)
        want, mask = row.expected()
        extras = {f"extra{i}": e for i, e in enumerate(row.extras)}
        np.savez(tmp_path / (name + ".npz"), real=row.real, decoy=row.decoy, want=want, want_decoy=row.expected("decoy")[0],
                 mask=np.zeros(0, bool) if mask is None else mask, n_extras=len(row.extras), **extras)
    _child("child_first_call", math.ceil(FIRST_DELAY_MS / (gpu["fill_ms"] * FIRST_BIG / BIG)), str(tmp_path))


# ---- (c) ---------------------------------------------------------------------------------------------
def test_two_threads_share_the_scratch_and_the_library_streams(gpu):
    """Two host threads, each with its own Stream, buffers and content, three rounds each, every thread
    synchronising only its own stream: the scratch mutexes, the event chains and the library streams
    carry both."""
    from vcf_amd.device import Stream, copy_dtod
    L = _L()
    plans = [("dct16_decode_small", "dct7_encode", "dct7_decode", "dwt_encode_pipe"),
             ("dct16_decode_large", "dct191_encode", "dwt_decode_pipe")]
    for names in plans:                     # the expected arrays once, on this thread
        for n in names:
            C.by_name(n).expected()
    start, failed, rounds = threading.Barrier(2), [], 3

    def work(t, names):
        try:
            st = Stream()
            bufs = [Bufs(C.by_name(n)) for n in names]
            for b in bufs:
                b.reset("real")
            start.wait(60)
            for r in range(rounds):
                for b in bufs:
                    b.snap.fill(0xEE, st)
                    L.call("vcf_memset", b.out.ptr, 0xEE, b.n_out, st.handle)   # (the last round's bytes would pass)
                    b.call(st)
                    copy_dtod(b.snap, 0, b.out.buf, b.out.start, b.n_out, st)
                    got = b.snap.download(np.empty(b.n_out, np.uint8), st)
                    st.synchronize()
                    m = _mismatch(b.row, got, f"thread {t} round {r}")
                    assert m is None, m
            for b in bufs:
                b.free()
        except BaseException as e:                     # the main thread reports it
            start.abort()
            failed.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t, names), daemon=True) for t, names in enumerate(plans)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads), "a thread did not finish in 60 s: a dead-lock between the scratch mutexes?"
    assert not failed, failed


# ---- (e) ---------------------------------------------------------------------------------------------
def test_last_error_is_per_thread(gpu):
    """vcf_last_error describes the last failure of the calling thread: a good call and a read of the
    message on another thread, in between, leave the first thread's message as it was."""
    L = _L()
    lib = L.lib()
    b = _bufs(gpu, "dct16_decode_small")
    b.reset("real")
    rejected, read = threading.Event(), threading.Event()
    seen, failed = {}, []

    def first():
        try:
            rc = lib.vcf_dct_dz_encode_any(b.din.ptr, 1, 20, 20, 5000, 32, 0, b.out.ptr, None)
            seen["rc"] = rc
            rejected.set()
            assert read.wait(30)
            seen["first"] = lib.vcf_last_error().decode()
        except BaseException as e:
            failed.append(repr(e))
            rejected.set()

    def second():
        try:
            assert rejected.wait(30)
            b.call(gpu["S"])
            gpu["S"].synchronize()
            seen["second"] = lib.vcf_last_error().decode()
        except BaseException as e:
            failed.append(repr(e))
        finally:
            read.set()

    threads = [threading.Thread(target=f, daemon=True) for f in (first, second)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads) and not failed, failed
    assert seen["rc"] == L.VCF_ERR_UNSUPPORTED
    assert "5000" in seen["first"], seen
    assert "5000" not in seen["second"] and "block size" not in seen["second"], seen
    out = b.out.download()[:b.n_out]
    assert _mismatch(b.row, out, "the good call") is None
