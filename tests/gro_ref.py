"""Receive coalescing (GRO): what tests/test_rx_gro.py and
tests/test_gpu_rx_gro.py share.  Test infrastructure.

- records(): K4's records of a burst decoded from the frames in Python;
- runs_model(): the rule of include/rxgpu.h ("TCP receive coalescing") in
  numpy: prefix sums and local predicates, no walk along a chain;
- rule_cases(): the rule's edge cases as frames made with tests/frames.py;
- scenario() / GroPair: scripted TCP sessions whose data comes in trains of
  in-sequence PSH|ACK segments, driven through nstack and oracle/ref_stack.c
  side by side."""
from __future__ import annotations

import numpy as np

import frames as F
import oracle_bind as O
import rxgpu as R

L = "192.168.100.77"
LISTEN = [(L, 9999), (L, 8080)]
BIG = 1 << 18  # a read longer than any run (W + 65536 at the default window)


# ---- the records and the rule ------------------------------------------------
def records(frames, caps, flows):
    """(seg, sip) of frames[i] captured caps[i] bytes with tcb id flows[i]
    (None: not a delivered TCP segment), stable-sorted by id; offset left 0"""
    idx = [i for i in range(len(frames)) if flows[i] is not None]
    idx.sort(key=lambda i: flows[i])
    seg = np.zeros(len(idx), R.SEGMENT_DTYPE)
    sip = np.zeros(len(idx), np.uint32)
    for k, i in enumerate(idx):
        f, cap = frames[i], caps[i]

        def b(q):
            return f[q] if q < cap and q < len(f) else 0
        hl, fl = b(46) >> 4, b(47)
        plen = ((b(16) << 8) | b(17)) - 20 - 4 * hl
        keep = min(plen, max(cap - 34 - 4 * hl, 0)) if (fl & 0x08 and plen > 0) else 0
        seg[k] = (i, flows[i], (b(38) << 24) | (b(39) << 16) | (b(40) << 8) | b(41),
                  (b(42) << 24) | (b(43) << 16) | (b(44) << 8) | b(45), plen, 0,
                  b(34) | (b(35) << 8), b(36) | (b(37) << 8), keep, fl, hl)
        sip[k] = b(26) | (b(27) << 8) | (b(28) << 16) | (b(29) << 24)
    return seg, sip


def runs_model(seg, sip, W):
    """the runs (R.TCP_RUN_DTYPE) of sorted records seg with source addresses sip"""
    n = len(seg)
    if n == 0:
        return np.zeros(0, R.TCP_RUN_DTYPE)
    plen = seg["plen"].astype(np.int64)
    merge = (seg["flags"] == 0x18) & (seg["hl"] == 5) & (plen > 0) & (seg["ncopy"] == plen)
    link = np.zeros(n, bool)
    same = np.ones(n - 1, bool)
    for name in ("flow", "sport", "dport", "ack"):
        same &= seg[name][1:] == seg[name][:-1]
    same &= sip[1:] == sip[:-1]
    nxt = (seg["seq"][:-1].astype(np.int64) + plen[:-1]) & 0xFFFFFFFF
    link[1:] = merge[1:] & merge[:-1] & same & (seg["seq"][1:].astype(np.int64) == nxt)
    pl = np.where(merge, plen, 0)
    before = np.cumsum(pl) - pl                       # payload of mergeable records before j
    head = np.maximum.accumulate(np.where(~link, np.arange(n), 0))
    b = before - before[head]                         # ... inside j's chain
    win = b // W
    start = ~link
    start[1:] |= link[1:] & (win[1:] != win[:-1])
    first = np.nonzero(start)[0]
    run = np.zeros(len(first), R.TCP_RUN_DTYPE)
    run["first"] = first
    run["nseg"] = np.diff(np.append(first, n))
    run["bytes"] = np.add.reduceat(seg["ncopy"].astype(np.int64), first)
    padded = (run["bytes"].astype(np.int64) + 15) // 16 * 16
    run["offset"] = np.cumsum(padded) - padded
    return run


def _p(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8))


def conn(k):
    """client k's address"""
    return f"10.0.{1 + k // 200}.{1 + k % 200}", 40000 + k


def rule_cases(rng, dport=9999, base=0):
    """[(label, frame, captured length)]: label k = connection conn(base + k),
    'L' = no connection (the listener's id).  In burst order."""
    out = []

    def add(k, n, seq, ack=2000, cut=0, **kw):
        if k == "L1" or k == "L2":
            cip, cport = ("10.0.9.1" if k == "L1" else "10.0.9.2"), 5000
            k = "L"
        else:
            cip, cport = conn(base + k)
        # (a cut capture reads as 0 past its end: zeros there keep the checksum good)
        f = F.tcp_frame(cip, cport, L, dport, _p(rng, n - cut) + bytes(cut), seq=seq & 0xFFFFFFFF,
                        ack=ack, **kw)
        out.append((k, f, len(f) - cut))
    for q in range(3):                       # 0: a chain whose seq wraps 2^32
        add(0, 100, 2 ** 32 - 150 + 100 * q)
    add(1, 100, 1000, ack=2000)              # 1: a differing ack
    add(1, 100, 1100, ack=2001)
    add(1, 100, 1200, ack=2001)
    add(2, 100, 1000)                        # 2: a duplicate seq
    add(2, 100, 1000)
    add(2, 100, 1100)
    add(3, 100, 1100)                        # 3: out of order
    add(3, 100, 1000)
    add(3, 100, 1200)
    add(4, 100, 1000)                        # 4: hl = 6 in the middle
    add(4, 100, 1100, data_off=0x60)
    add(4, 100, 1200)
    add(4, 100, 1300)
    add(5, 100, 1000)                        # 5: flags 0x10, 0x19, 0x11 between PSH|ACK
    add(5, 100, 1100, flags=0x10)
    add(5, 100, 1200)
    add(5, 100, 1300)
    add(5, 100, 1400, flags=0x19)
    add(5, 100, 1500)
    add(5, 0, 1600, flags=0x11)
    add(5, 100, 1601)
    add(6, 100, 1000)                        # 6: plen = 0
    add(6, 0, 1100)
    add(6, 100, 1100)
    add(6, 100, 1200)
    add(7, 100, 1000)                        # 7: a capture cut mid-payload
    add(7, 100, 1100, cut=30)
    add(7, 100, 1200)
    add(7, 100, 1300)
    add("L1", 100, 1000)                     # L: two sources, equal ports, contiguous seq
    add("L2", 100, 1100)
    for q in range(6):                       # 8: 6 x 100 B: W = 100, 250, 300
        add(8, 100, 5000 + 100 * q)
    for q in range(9):                       # 9: 9 x 1460 B: W = 1460
        add(9, 1460, 7000 + 1460 * q)
    return out


# (frames = records, id space) at the edges of the device stages: one record
# block of 256 and one sort tile of 2048, and one past each; 255 | 256 ids: the
# flow sort's one and two radix passes; 256 | 257 positions: the ordering
# stage's head-index sort likewise
STAGE_EDGES = [(1, 255), (255, 256), (256, 255), (257, 256), (2049, 255)]


def boundary_burst(n, nconn, seed, cut=False):
    """(frames, caps, forced) of n frames, every one a delivered segment of
    connections conn(0 .. nconn - 1), for the edges of the device stages (the
    callers choose n = the record count and nconn + 1 = the id space).
    Connection 0 takes all but four: in sequence, payloads of 33, 34, 35, 36, 17
    and 1 B (a chain's copies start at every byte phase of source and
    destination), every 7th overlapping its predecessor by 1 to 3 B (the
    assembly's skip shifts the source phase as well), every 11th with hl = 6,
    neighbours swapped here and there (something to order).  Connections 1 and
    nconn - 1 (the top id) take two each.  cut: connection 1's second capture
    ends at byte 40, inside the TCP header: seq's low half, ack, hl and flags
    read 0; K1 would not deliver it, so forced = {its index: 1} is the verdict
    to give it."""
    rng = np.random.default_rng(seed)
    frames, seq = [], 2 ** 32 - 3000
    for q in range(n - 4 if n > 4 else n):
        ln = (33, 34, 35, 36, 17, 1)[q % 6]
        if q % 7 == 6:
            seq -= 1 + q % 3
        frames.append(F.tcp_frame(*conn(0), L, 9999, _p(rng, ln), seq=seq & 0xFFFFFFFF,
                                  **({"data_off": 0x60} if q % 11 == 10 else {})))
        seq += ln
    for q in range(0, len(frames) - 1, 5):
        frames[q], frames[q + 1] = frames[q + 1], frames[q]
    if n > 4:
        for k in (1, nconn - 1):
            at = int(rng.integers(0, len(frames)))
            frames[at:at] = [F.tcp_frame(*conn(k), L, 9999, _p(rng, 40), seq=70000 + 40 * q) for q in (1, 0)]
    assert len(frames) == n
    caps, forced = [len(f) for f in frames], {}
    if cut and n > 4:
        i = max(j for j, f in enumerate(frames) if f[34:36] == (40001).to_bytes(2, "big"))
        caps[i], forced = 40, {i: 1}
    return frames, caps, forced


# ---- the socket layer against the oracle ----------------------------------------
def _client_script(rng, k, dport):
    """one client's segments in order: handshake, trains of 1 to 9 in-sequence
    PSH|ACK segments with the edge segments of test_deliver_oracle.py's client
    script between them, FIN, 'close' (the server closes), the final ACK"""
    cip, cport = conn(k)
    seq = int(rng.integers(1, 2 ** 31))
    seg = []

    def tcp(payload=b"", flags=0x18, **kw):
        return F.tcp_frame(cip, cport, L, dport, payload, flags=flags, seq=seq & 0xFFFFFFFF, **kw)
    seg.append(tcp(flags=0x02))
    seq += 1
    if rng.random() < 0.2:
        seg.append(tcp(flags=0x02))
    seg.append(tcp(flags=0x10))
    for _ in range(int(rng.integers(2, 5))):
        for _ in range(int(rng.integers(1, 10))):         # a train
            n = int(rng.choice([1, 7, 100, 600, 1460]))
            seg.append(tcp(_p(rng, n)))
            seq += n
        kind = rng.random()
        n = int(rng.choice([0, 1, 7, 100]))
        p = _p(rng, n)
        if kind < 0.1:
            seg.append(tcp(p, corrupt=len(p) > 0))
        elif kind < 0.2:
            seg.append(tcp(p, data_off=0x60))
        elif kind < 0.25:
            seg.append(tcp(p, tl=30, tl_cksum=True))
        elif kind < 0.3:
            seg.append(tcp(flags=0x02))
            n = 0
        elif kind < 0.35:
            seg.append(tcp(p, flags=0x19))
        elif kind < 0.45:
            seg.append(tcp(flags=0x10))
            n = 0
        elif kind < 0.55:
            seg.append(tcp(b""))
            n = 0
        else:
            n = 0
        seq += n
    if rng.random() < 0.8:
        seg.append(tcp(flags=0x11))
        seq += 1
        seg.append("close")
        seg.append(tcp(flags=0x10))
    return (cip, cport, dport), seg


def scenario(seed, n_clients=6):
    """(connection keys, events): ('burst', frames) and ('close_conn', key);
    per-client order kept, clients interleaved at random, bursts of 8 to 60"""
    rng = np.random.default_rng(seed)
    scripts = [_client_script(rng, k, LISTEN[k % 2][1] if k < n_clients - 1 else 7)
               for k in range(n_clients)]  # the last client has no listener
    streams = [list(s) for _, s in scripts]
    keys = [k for k, _ in scripts]
    events, burst = [], []
    size = int(rng.integers(8, 61))
    while any(streams):
        i = int(rng.choice([j for j, s in enumerate(streams) if s]))
        for _ in range(int(rng.integers(1, 6))):          # a few of one client's in a row
            if not streams[i]:
                break
            item = streams[i].pop(0)
            if isinstance(item, str):
                if burst:
                    events.append(("burst", burst))
                    burst = []
                events.append(("close_conn", keys[i]))
                break
            burst.append(item)
        if len(burst) >= size:
            events.append(("burst", burst))
            burst, size = [], int(rng.integers(8, 61))
    if burst:
        events.append(("burst", burst))
    return keys, events


def _tokens(reads):
    """a connection's reads as its byte stream with the EOFs in place:
    [bytes, 'EOF', bytes, ...], adjacent data joined"""
    out = []
    for r, d in reads:
        if r == 0:
            out.append("EOF")
        elif out and out[-1] != "EOF":
            out[-1] += d
        else:
            out.append(d)
    return out


class GroPair:
    """nstack (coalescing window W, 0 = off) and the oracle stack side by side.
    mode: 'cpu' (nstack_deliver with the oracle's verdicts), 'gpu'
    (nstack_rx_burst), 'pipe' (nstack_rx_submit / nstack_rx_complete)"""

    def __init__(self, ns, mode, W):
        self.ns, self.os, self.mode, self.W = ns, O.Stack(), mode, W
        self.listen_fds, self.conns = {}, {}
        self.reads_ns, self.reads_os = {}, {}
        self.want_absorbed = 0     # by the model, over the bursts
        self.acks_dropped = 0      # ACKs of the oracle's the stack did not queue
        for ip, port in LISTEN:
            a = self.ns.socket(R.SOCK_STREAM)
            assert a == self.os.socket(1)
            assert self.ns.bind(a, ip, port) == self.os.bind(a, R.ip_raw(ip), R.port_raw(port)) == 0
            assert self.ns.listen(a) == self.os.listen(a) == 0
            self.listen_fds[port] = a

    def _model_absorbed(self, frames, v):
        """segments the rule merges into a preceding one, over the connections
        that are ESTABLISHED when the burst starts (the others go frame by
        frame); a FIN ends a connection's deliveries"""
        flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 else None for x in v]
        seg, sip = records(frames, [len(f) for f in frames], flows)
        run = runs_model(seg, sip, self.W)
        got = 0
        established = None
        for r in run:
            g = seg[r["first"]]
            if r["first"] == 0 or seg[r["first"] - 1]["flow"] != g["flow"]:  # a new connection
                st = self.ns.tcb_state(int(sip[r["first"]]), R.ip_raw(L), int(g["sport"]), int(g["dport"]))
                established = st is not None and st[0] == R.TCP_STATUS_ESTABLISHED and \
                    self.ns.lookup_tcp(int(sip[r["first"]]), R.ip_raw(L), int(g["sport"]),
                                       int(g["dport"])) == g["flow"]
            if not established:
                continue
            if r["nseg"] > 1:
                got += int(r["nseg"]) - 1
            elif g["flags"] & 0x01:
                established = False
        return got

    def burst(self, frames):
        want = [self.os.rx(f) for f in frames]
        u, t, gen = self.ns.flows(with_gen=True)
        buf, off, lens = F.pack_frames(frames)
        v = self.ns.to_ids(O.Tables(u, t).classify(buf, off, lens, 6))
        if self.W:
            self.want_absorbed += self._model_absorbed(frames, v)
        rcs = np.zeros(len(frames), np.int32)
        if self.mode == "cpu":
            self.ns.deliver(frames, v, rcs, gen)
        elif self.mode == "gpu":
            _, rcs, vg = self.ns.rx_burst(frames)
            assert vg.tobytes() == v.tobytes()
        else:
            self.ns.rx_submit(frames)
            _, rcs, vg = self.ns.rx_complete()
            assert vg.tobytes() == v.tobytes()
        assert list(rcs) == want, (list(rcs), want)

    def accept_all(self):
        for port, lfd in self.listen_fds.items():
            while True:
                fd, sip, sport = self.os.accept(lfd)
                if fd == O.WOULD_BLOCK:
                    break
                got, a = self.ns.accept(lfd)
                assert (got, a.sin_addr, a.sin_port) == (fd, sip, sport)
                self.conns[(sip, sport, port)] = fd

    def drain(self):
        """every connection read until it would block, on both sides"""
        for key, fd in self.conns.items():
            a, b = self.reads_ns.setdefault(key, []), self.reads_os.setdefault(key, [])
            while True:
                r, d = self.ns.recv(fd, BIG)
                if r < 0:
                    break
                a.append((r, d))
            while True:
                r, d = self.os.recv(fd, BIG)
                if r == O.WOULD_BLOCK:
                    break
                b.append((r, d[:max(r, 0)]))

    def check_acks(self, key):
        """the stack's queued control fragments are the oracle's with, per run,
        only the ACK that closes it: going back from the end, an oracle entry
        the stack lacks is a pure ACK and the entry after it is a pure ACK
        (kept or not) acknowledging more"""
        cip, cport, dport = key
        t = (R.ip_raw(cip), R.ip_raw(L), R.port_raw(cport), R.port_raw(dport))
        if self.os.tcb_state(*t) is None:
            assert self.ns.tcb_state(*t) is None
            return
        ours, theirs = self.ns.tcb_sndq(*t), self.os.tcb_sndq(*t)
        k, nxt = len(ours), None
        for e in reversed(theirs):
            if k and ours[k - 1] == e:
                k -= 1
            else:
                assert e[0] == 0x10 and nxt is not None and nxt[0] == 0x10 and \
                    0 < ((nxt[1] - e[1]) & 0xFFFFFFFF) < (1 << 24), (t, e, nxt, ours, theirs)
                self.acks_dropped += 1
            nxt = e
        assert k == 0, (t, ours, theirs)
        assert [e for e in ours if e[0] != 0x10] == [e for e in theirs if e[0] != 0x10]
        if not self.W:
            assert ours == theirs

    def close_conn(self, key):
        cip, cport, dport = key
        self.accept_all()
        self.drain()
        self.check_acks(key)
        fd = self.conns.pop((R.ip_raw(cip), R.port_raw(cport), dport), None)
        if fd is not None:
            assert self.ns.close(fd) == self.os.close(fd) == 0

    def compare_tcbs(self, keys):
        assert self.ns.tcb_count() == self.os.tcb_count()
        for cip, cport, dport in keys:
            t = (R.ip_raw(cip), R.ip_raw(L), R.port_raw(cport), R.port_raw(dport))
            want, got = self.os.tcb_state(*t), self.ns.tcb_state(*t)
            if want is None:
                assert got is None, t
                continue
            st, rn, sn, fd = want
            assert got is not None and (got[0], got[1], got[3]) == (st, rn, fd), (t, got, want)
            if sn is not None:
                assert got[2] == sn, (t, got, want)

    def run(self, keys, events):
        base = [self.ns.stat(k) for k in (4, 15)]
        for kind, arg in events:
            if kind == "burst":
                self.burst(arg)
                self.accept_all()
                self.drain()
            else:
                self.close_conn(arg)
        self.compare_tcbs(keys)
        for key in keys:
            self.check_acks(key)
        n_ns = n_os = 0
        for key in self.reads_os:
            assert _tokens(self.reads_ns[key]) == _tokens(self.reads_os[key]), key
            n_ns += len(self.reads_ns[key])
            n_os += len(self.reads_os[key])
            if not self.W:
                assert self.reads_ns[key] == self.reads_os[key], key
        absorbed = self.ns.stat(15) - base[1]
        assert absorbed == self.want_absorbed == self.acks_dropped == n_os - n_ns
        if self.W:
            assert n_ns < n_os
        return n_ns, n_os, absorbed
