"""The burst path of TCP delivery against the stack's own frame-by-frame path.

A burst handed to nstack_deliver with the generation of flows(with_gen=True)
goes through the per-connection batches (deliver_tcp_conn and its stream form:
one allocation of fragments, one of ACKs, per connection and burst); the same
burst handed over with NStack.STALE is looked up and delivered frame by frame
(tcp_dispatch), the path test_deliver_oracle.py pins to the oracle.  Every case
runs both ways, one host-only stack after the other (the stack is
process-global), and compares what a caller can see: the per-frame rcs, the
statistics, every recv result, the tcb states and the queued ACKs.

The cases are the edges no other burst of the suite reaches: a receive ring
that fills in the middle of a connection's batch (1401 fragments for one tcb,
1024 fit), a segment whose capture ends before its payload going down the
batch path (copied, zero filled), and the same bursts with coalescing and with
stream assembly on, where the fragment boundaries differ and the byte streams
must not.  The GPU part runs the ring-fill bursts through a device stack
(nstack_rx_burst, nstack_rx_submit / nstack_rx_complete; pooled payload buffers
and in place) against the host-only frame-by-frame run."""
import functools

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxgpu as R

L = "192.168.100.77"
A, B = ("10.0.0.9", 40000), ("10.0.0.10", 40001)
PORT = 9999
BIG = 4096
ISN = 999  # the handshake's SYN; data starts at ISN + 1


def _key(c):
    return (R.ip_raw(c[0]), R.ip_raw(L), R.port_raw(c[1]), R.port_raw(PORT))


@functools.lru_cache(maxsize=None)
def _bursts(n_a):
    """two bursts, each n_a PSH|ACK segments to A (1..39 random bytes) with a
    7-byte segment to B after every 23rd of them; the second ends with FIN|ACK
    to both.  Sequence numbers run on from ISN + 1 on both connections."""
    rng = np.random.default_rng(20)
    seq = {A: ISN + 1, B: ISN + 1}

    def seg(c, payload, flags=0x18):
        f = F.tcp_frame(c[0], c[1], L, PORT, payload, flags=flags, seq=seq[c])
        seq[c] += len(payload)
        return f
    out = []
    for b in range(2):
        fr = []
        for i in range(n_a):
            fr.append(seg(A, bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8))))
            if i % 23 == 0:
                fr.append(seg(B, bytes(rng.integers(0, 256, 7, dtype=np.uint8))))
        if b == 1:
            fr += [seg(A, b"", 0x11), seg(B, b"", 0x11)]
        out.append(tuple(fr))
    return tuple(out)


def _deliver(ns, frames, gen_of, caplens=None):
    """one burst through nstack_deliver with the oracle front end's verdicts
    (made with the capture lengths); gen_of(gen) picks the generation handed
    over.  The mbufs carry caplens as data_len.  Returns the rcs."""
    frames = list(frames)
    caplens = [len(f) for f in frames] if caplens is None else list(caplens)
    u, t, gen = ns.flows(with_gen=True)
    buf, off, lens = F.pack_frames(frames, 6, caplens=caplens)
    v = np.ascontiguousarray(ns.to_ids(O.Tables(u, t).classify(buf, off, lens, 6)), R.VERDICT_DTYPE)
    arr, keep = ns.mbufs(frames)
    for m, c in zip(keep[1], caplens):
        m.data_len = c
    rcs = np.full(len(frames), 99, np.int32)
    r = ns.lib.nstack_deliver(arr, len(frames), v.ctypes.data, gen_of(gen), rcs.ctypes.data)
    ns._let_go(arr, len(frames), keep)
    assert r >= 0
    return [int(x) for x in rcs]


def _fresh(gen):
    return gen


def _stale(gen):
    return R.NStack.STALE


def _listen(ns):
    lfd = ns.socket(R.SOCK_STREAM)
    assert ns.bind(lfd, L, PORT) == 0 and ns.listen(lfd) == 0
    return lfd


def _accept(ns, lfd, conns):
    fds = {}
    for _ in conns:
        fd, a = ns.accept(lfd)
        assert fd > lfd
        fds[(a.sin_addr, a.sin_port)] = fd
    return [fds[(R.ip_raw(c[0]), R.port_raw(c[1]))] for c in conns]


def _read_all(ns, fd, size=BIG):
    out = []
    while True:
        r, d = ns.recv(fd, size)
        if r < 0:
            return out
        out.append((r, d))


def _stats(ns):
    return [int(ns.stat(k)) for k in range(5)]


def _end_state(ns, fds, conns):
    return {"reads": [_read_all(ns, fd) for fd in fds],
            "state": [ns.tcb_state(*_key(c)) for c in conns],
            "sndq": [ns.tcb_sndq(*_key(c)) for c in conns]}


def _option(ns, opt):
    if opt == "inplace":
        ns.set_rx_inplace(True)
    elif opt == "order":
        ns.set_rx_order(True)
    elif opt == "gro":
        ns.set_rx_gro(65536)
    elif opt == "assemble":
        ns.set_rx_assemble(True)
    else:
        assert opt == "plain"


def _ring_run(ns, opt, burst):
    """the ring-fill case on stack ns: burst(frames) -> rcs delivers one burst"""
    _option(ns, opt)
    lfd = _listen(ns)
    for c in (A, B):
        assert ns.tcb_add(c[0], L, c[1], PORT) == 0
    fds = _accept(ns, lfd, (A, B))
    out = {"rcs": [], "stats": []}
    for fr in _bursts(700):  # nothing is read in between: A's ring overflows in burst 2
        out["rcs"].append(burst(fr))
        out["stats"].append(_stats(ns))
    out.update(_end_state(ns, fds, (A, B)))
    return out


def _host(run, *args):
    ns = R.NStack(R.HOST_ONLY)
    try:
        return run(ns, *args)
    finally:
        ns.fini()


def _ring_host(ns, opt, gen_of):
    return _ring_run(ns, opt, lambda fr: _deliver(ns, fr, gen_of))


@functools.lru_cache(maxsize=None)
def _ring_stale(opt):
    """the frame-by-frame run of the ring-fill case (computed once, shared by
    the CPU and the GPU part, never changed)"""
    return _host(_ring_host, opt, _stale)


def _check_ring(got):
    """what the bursts are built to reach, so the comparison cannot pass on a
    run that never filled the ring"""
    assert [len(r) for r in got["rcs"]] == [731, 733]
    assert got["stats"][1] == [0, 377, 1464, 0, 1087]
    assert len(got["reads"][0]) == 1024 and len(got["sndq"][0]) == 1024


@pytest.mark.parametrize("opt", ["plain", "inplace", "order"])
def test_ring_fills_mid_batch(opt):
    """1401 fragments for A over two bursts with nothing read: 1024 are handed
    out, 377 dropped, 1024 ACKs queued, the same on both paths"""
    fresh, stale = _host(_ring_host, opt, _fresh), _ring_stale(opt)
    print(opt, fresh["stats"], stale["stats"])
    _check_ring(fresh)
    assert fresh == stale


def _refill_run(ns, gen_of):
    lfd = _listen(ns)
    for c in (A, B):
        assert ns.tcb_add(c[0], L, c[1], PORT) == 0
    fds = _accept(ns, lfd, (A, B))
    b1, b2 = _bursts(700)
    out = {"rcs": [], "stats": [], "reads": []}
    for fr in (b1, b2[:-2], None, b1):  # (the FINs left out: A stays ESTABLISHED)
        if fr is None:
            out["reads"].append([_read_all(ns, fd) for fd in fds])
            continue
        out["rcs"].append(_deliver(ns, fr, gen_of))
        out["stats"].append(_stats(ns))
    out["reads"].append([_read_all(ns, fd) for fd in fds])
    return out


def test_ring_refills_after_a_drain():
    """the fragment count of a ring that overflowed (1400 for A, 1024 fit) is
    what fits, not what came: once the reader has taken all 1024 the ring has
    room for all 700 fragments of a third burst, on both paths"""
    fresh, stale = _host(_refill_run, _fresh), _host(_refill_run, _stale)
    print(fresh["stats"])
    assert fresh["stats"][1][1] == 376 and fresh["stats"][2][1] == 376  # (none dropped after the drain)
    assert [len(r) for r in fresh["reads"][0]] == [1024, 62] and \
        [len(r) for r in fresh["reads"][1]] == [700, 31]
    assert fresh == stale


def _cut_run(ns, opt, gen_of):
    _option(ns, opt)
    lfd = _listen(ns)
    assert ns.tcb_add(A[0], L, A[1], PORT) == 0
    fds = _accept(ns, lfd, (A,))
    # 30 bytes of 0xFF: fifteen 0xFFFF words add nothing to a one's-complement
    # sum, so the checksum still verifies with all of them read as 0 (the -30
    # capture) and fails when a word is split (-7) or the header is cut (-35)
    frames = [F.tcp_frame(A[0], A[1], L, PORT, b"\xff" * 30, seq=ISN + 1 + 30 * i)
              for i in range(18)]
    # six whole segments first, read at once: their batch (six fragments, 180
    # copied bytes of 0xFF) is what the twelve below make without in-place
    # receive, so its freed block comes back with 0xFF where the zero fill goes
    out = {"prime": _deliver(ns, frames[:6], gen_of), "primed": _read_all(ns, fds[0])}
    caplens = [len(f) - (0, 7, 30, 35)[i % 4] for i, f in enumerate(frames[6:])]
    out.update({"rcs": _deliver(ns, frames[6:], gen_of, caplens), "stats": _stats(ns)})
    out.update(_end_state(ns, fds, (A,)))
    return out


@pytest.mark.parametrize("opt", ["plain", "inplace"])
def test_capture_cut_short(opt):
    """twelve 30-byte PSH segments captured whole, or 7, 30 or 35 bytes short:
    the -7 and -35 frames fail their checksum (rc -1); the -30 frame's header is
    whole and its payload is not there at all: delivered as 30 zero bytes"""
    fresh, stale = _host(_cut_run, opt, _fresh), _host(_cut_run, opt, _stale)
    print(opt, fresh["rcs"], fresh["stats"])
    assert fresh["rcs"] == [0, -1, 0, -1] * 3
    assert (30, bytes(30)) in fresh["reads"][0]
    assert fresh == stale


def _stream_run(ns, opt, gen_of):
    _option(ns, opt)
    lfd = _listen(ns)
    for c in (A, B):  # a real handshake: assembly aligns with rcv_nxt
        for fl, seq in ((0x02, ISN), (0x10, ISN + 1)):
            assert _deliver(ns, [F.tcp_frame(c[0], c[1], L, PORT, b"", flags=fl, seq=seq)],
                            gen_of) == [0]
    fds = _accept(ns, lfd, (A, B))
    out = {"rcs": [_deliver(ns, fr, gen_of) for fr in _bursts(300)]}  # (no ring fills)
    counters = {"absorbed": int(ns.stat(15)), "frags": int(ns.stat(4))}
    reads = [_read_all(ns, fd, 65536) for fd in fds]  # (no read splits a coalesced fragment)
    out["bytes"] = [b"".join(d for _, d in rd) for rd in reads]
    out["eof"] = [bool(rd) and rd[-1][0] == 0 for rd in reads]
    out["state"] = [ns.tcb_state(*_key(c)) for c in (A, B)]
    return out, counters


@pytest.mark.parametrize("opt", ["gro", "assemble"])
def test_coalesced_and_assembled_streams(opt):
    """fragment boundaries and ACK counts differ between the paths here; the
    bytes each connection reads, the EOF behind them and the tcb states do not.
    On the burst path every connection's segments of a burst are one run (624 =
    2 x (299 + 13) segments absorbed) or one stream, so one fragment per
    connection and burst, and an EOF fragment behind each FIN: 4 + 2"""
    (fresh, cnt), (stale, _) = _host(_stream_run, opt, _fresh), _host(_stream_run, opt, _stale)
    print(opt, cnt)
    assert fresh["eof"] == [True, True] and len(fresh["bytes"][0]) > 600
    assert fresh == stale
    if opt == "gro":
        assert cnt["absorbed"] == 624
    assert cnt["frags"] == 6


# ---- the same ring-fill bursts through a device stack -----------------------
def _gpu_burst(ns, pipe):
    def burst(fr):
        if pipe:
            ns.rx_submit(list(fr))
            _, rcs, _ = ns.rx_complete()
        else:
            _, rcs, _ = ns.rx_burst(list(fr))
        return [int(x) for x in rcs]
    return burst


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["plain", "inplace"], ids=["pooled", "inplace"])
@pytest.mark.parametrize("pipe", [False, True], ids=["rx_burst", "submit_complete"])
def test_gpu_ring_fills_mid_batch(pipe, opt):
    """the held-buffer fragments (pl_ref >= 0) and the library's records:
    nothing about the kernels is under test"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")
    want = _ring_stale(opt)
    ns = R.NStack(0)
    try:
        got = _ring_run(ns, opt, _gpu_burst(ns, pipe))
    finally:
        ns.fini()
    print(pipe, opt, got["stats"], want["stats"])
    _check_ring(got)
    assert got == want
