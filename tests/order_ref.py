"""TCP sequence ordering: what tests/test_rx_order.py and
tests/test_gpu_rx_order.py share.  Test infrastructure.

- order_model(): the rule of include/rxgpu.h ("TCP sequence ordering") in
  numpy: group heads from a comparison with the predecessor, the head index by
  a running maximum, the order by one lexsort.  No code shared with
  csrc/rx_order_host.cpp;
- rule_cases() / HAND: the rule's edge cases as frames made with
  tests/frames.py, and each case's permutation written out by hand;
- scenario() / OrderPair: scripted TCP sessions (handshakes, data trains of 1
  to 9 segments, FINs).  oracle/ref_stack.c gets every burst in order, nstack
  the same burst with each connection's segments permuted among the
  connection's own positions."""
from __future__ import annotations

import numpy as np

import frames as F
import gro_ref as G
import oracle_bind as O
import rxgpu as R

L = G.L


# ---- the rule ------------------------------------------------------------------
def order_model(seg, sip):
    """(perm, moved) of sorted records seg with source addresses sip: perm[k] =
    the index of the record that takes position k"""
    n = len(seg)
    pos = np.arange(n)
    if n == 0:
        return pos.astype(np.uint32), 0
    movable = (seg["flags"] & 0x06) == 0
    head = np.ones(n, bool)
    same = movable[1:] & movable[:-1] & (sip[1:] == sip[:-1])
    for name in ("flow", "sport", "dport"):
        same &= seg[name][1:] == seg[name][:-1]
    head[1:] = ~same
    h = np.maximum.accumulate(np.where(head, pos, 0))
    seq = seg["seq"].astype(np.int64)
    key = ((seq - seq[h]) & 0xFFFFFFFF) ^ 0x80000000     # the biased signed distance
    perm = np.lexsort((pos, key, h))
    return perm.astype(np.uint32), int(np.count_nonzero(perm != pos))


# label -> the permutation of the connection's records (arrival index taking
# each position), by hand
HAND = {
    0: [1, 0],                              # a swap across the seq wrap
    1: [1, 2, 3, 0],                        # equal seq: pure ACK, data, duplicate; a later one first
    2: [1, 0, 2, 4, 3],                     # a SYN is a barrier
    3: [1, 0, 2, 4, 3],                     # a RST is a barrier
    4: [0, 2, 1],                           # a FIN that arrived before the last data
    5: [1, 0],                              # PSH|FIN
    6: [8, 7, 6, 5, 0, 4, 9, 3, 2, 1],      # each key byte, negative distances
    7: [0],                                 # a group of one
    "L": [0, 1, 2],                         # sources A, B, A on the listener's id: three groups
}


def rule_cases(rng, dport=9999, base=0):
    """[(label, frame, captured length)] in burst order: label k = connection
    G.conn(base + k), 'L' = no connection (the listener's id)"""
    out = []

    def add(k, seq, n=10, flags=0x18, **kw):
        if k in ("L1", "L2"):
            cip, cport = ("10.0.9.1" if k == "L1" else "10.0.9.2"), 5000
            k = "L"
        else:
            cip, cport = G.conn(base + k)
        f = F.tcp_frame(cip, cport, L, dport, G._p(rng, n), seq=seq & 0xFFFFFFFF, flags=flags, **kw)
        out.append((k, f, len(f)))
    add(0, 0x00000100)
    add(0, 0xFFFFFF00)
    add(1, 1100, 100)
    add(1, 1000, 0, flags=0x10)
    add(1, 1000, 100)
    add(1, 1000, 100)
    for k, fl in ((2, 0x02), (3, 0x04)):
        add(k, 1200, 100)
        add(k, 1100, 100)
        add(k, 5, 0, flags=fl)
        add(k, 1400, 100)
        add(k, 1300, 100)
    add(4, 1000, 100)
    add(4, 1200, 0, flags=0x11)
    add(4, 1100, 100)
    add(5, 1100, 100, flags=0x19)
    add(5, 1000, 100)
    for d in (0, 0x01000000, 0x00010000, 0x00000100, 1, -1, -0x100, -0x10000, -0x1000000, 2):
        add(6, 0x40000000 + d)
    add(7, 777, 33)
    add("L1", 300, 20, flags=0x10)
    add("L2", 100, 20, flags=0x10)
    add("L1", 200, 20, flags=0x10)
    return out


def check_hand(seg, perm, flow_of):
    """perm restricted to every case's records equals HAND; flow_of(label) = its id"""
    for label, want in HAND.items():
        idx = np.nonzero(seg["flow"] == flow_of(label))[0]
        assert len(idx) == len(want) and np.all(np.diff(idx) == 1), label
        assert list(perm[idx] - idx[0]) == want, (label, list(perm[idx] - idx[0]))


# ---- the socket layer against the oracle ------------------------------------------
def scenario(seed, n_clients=6, permute=True):
    """(connection keys, events): ('burst', ordered frames, permuted frames,
    p) with permuted[i] = ordered[p[i]], and ('close_conn', key).  The first
    burst holds the handshakes; every later one a train of 1 to 9 data segments
    for most connections, a FIN behind a connection's last train.  Connections
    are interleaved at random; p moves a connection's segments among that
    connection's positions only.  Connection 0's first train has four
    segments, reversed."""
    rng = np.random.default_rng(seed)
    keys = [(*G.conn(k), G.LISTEN[k % 2][1]) for k in range(n_clients)]
    seq = [int(rng.integers(1, 2 ** 32)) for _ in keys]

    def tcp(k, payload=b"", flags=0x18):
        cip, cport, dport = keys[k]
        return F.tcp_frame(cip, cport, L, dport, payload, flags=flags, seq=seq[k] & 0xFFFFFFFF)

    def interleave(per):
        """per[k] = connection k's frames in order -> (frames, owner)"""
        per = {k: list(v) for k, v in per.items() if v}
        frames, owner = [], []
        while per:
            k = list(per)[int(rng.integers(len(per)))]
            for _ in range(int(rng.integers(1, 4))):
                if not per[k]:
                    break
                frames.append(per[k].pop(0))
                owner.append(k)
            if not per[k]:
                del per[k]
        return frames, np.array(owner)

    events = []
    per = {}
    for k in range(n_clients):
        per[k] = [tcp(k, flags=0x02)]
        seq[k] += 1
        per[k].append(tcp(k, flags=0x10))
    frames, _ = interleave(per)
    events.append(("burst", frames, frames, np.arange(len(frames))))
    rounds = [int(rng.integers(2, 5)) for _ in keys]
    r = 0
    while any(x > r for x in rounds):
        per, fin = {}, []
        for k in range(n_clients):
            if rounds[k] <= r or (r and rng.random() < 0.2 and rounds[k] > r + 1):
                continue
            per[k] = []
            for _ in range(4 if (k == 0 and r == 0) else int(rng.integers(1, 10))):
                n = int(rng.choice([1, 7, 100, 600, 1460]))
                per[k].append(tcp(k, G._p(rng, n)))
                seq[k] += n
            if rounds[k] == r + 1 and rng.random() < 0.8:
                per[k].append(tcp(k, flags=0x11))
                seq[k] += 1
                fin.append(k)
        frames, owner = interleave(per)
        p = np.arange(len(frames))
        for k in sorted(set(owner)):      # (drawn either way: the same sessions with permute off)
            idx = np.nonzero(owner == k)[0]
            q = idx[::-1] if (k == 0 and r == 0) else rng.permutation(idx)
            if permute:
                p[idx] = q
        events.append(("burst", frames, [frames[i] for i in p], p))
        if fin:
            for k in fin:
                events.append(("close_conn", keys[k]))
            last = [tcp(k, flags=0x10) for k in fin]
            events.append(("burst", last, last, np.arange(len(last))))
        r += 1
    return keys, events


class OrderPair(G.GroPair):
    """nstack (with nstack_set_rx_order as the caller set it; coalescing window
    W) on the permuted bursts beside the oracle stack on the ordered ones.
    strict: every check of G.GroPair; else only what both sides read is kept"""

    def __init__(self, ns, mode, W=0, strict=True):
        super().__init__(ns, mode, W)
        self.strict = strict
        self.want_moved = 0

    def burst(self, ordered, permuted, p):
        want = [self.os.rx(f) for f in ordered]
        u, t, gen = self.ns.flows(with_gen=True)
        tab = O.Tables(u, t)
        buf, off, lens = F.pack_frames(permuted)
        v = self.ns.to_ids(tab.classify(buf, off, lens, 6))
        flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 else None for x in v]
        seg, sip = G.records(permuted, [len(f) for f in permuted], flows)
        self.want_moved += order_model(seg, sip)[1]
        if self.W:
            buf, off, lens = F.pack_frames(ordered)
            self.want_absorbed += self._model_absorbed(
                ordered, self.ns.to_ids(tab.classify(buf, off, lens, 6)))
        rcs = np.zeros(len(permuted), np.int32)
        if self.mode == "cpu":
            self.ns.deliver(permuted, v, rcs, gen)
        elif self.mode == "gpu":
            _, rcs, vg = self.ns.rx_burst(permuted)
            assert vg.tobytes() == v.tobytes()
        else:
            self.ns.rx_submit(permuted)
            _, rcs, vg = self.ns.rx_complete()
            assert vg.tobytes() == v.tobytes()
        if self.strict:   # matched by frame
            assert list(rcs) == [want[i] for i in p], (list(rcs), [want[i] for i in p])

    def close_conn(self, key):
        cip, cport, dport = key
        self.accept_all()
        self.drain()
        if self.strict:
            self.check_acks(key)
        fd = self.conns.pop((R.ip_raw(cip), R.port_raw(cport), dport), None)
        if fd is not None:
            a, b = self.ns.close(fd), self.os.close(fd)
            assert not self.strict or a == b == 0

    def tokens(self):
        return ({k: G._tokens(v) for k, v in self.reads_ns.items()},
                {k: G._tokens(v) for k, v in self.reads_os.items()})

    def run(self, keys, events):
        """strict: returns (fragments read from nstack, from the oracle, moved)"""
        base = [self.ns.stat(k) for k in (15, 16)]
        for ev in events:
            if ev[0] == "burst":
                self.burst(*ev[1:])
                self.accept_all()
                self.drain()
            else:
                self.close_conn(ev[1])
        moved = self.ns.stat(16) - base[1]
        if not self.strict:
            return None, None, moved
        self.compare_tcbs(keys)                 # states, rcv_nxt, snd_nxt
        for key in keys:
            self.check_acks(key)                # the queued ACKs' acknum sequence
        tn, to = self.tokens()
        n_ns = n_os = 0
        for key in self.reads_os:
            assert tn[key] == to[key], key      # byte stream and EOF position
            n_ns += len(self.reads_ns[key])
            n_os += len(self.reads_os[key])
            if not self.W:
                assert self.reads_ns[key] == self.reads_os[key], key
        absorbed = self.ns.stat(15) - base[0]
        assert absorbed == self.want_absorbed == self.acks_dropped == n_os - n_ns
        return n_ns, n_os, moved
