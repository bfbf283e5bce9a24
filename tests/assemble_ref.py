"""TCP stream assembly: what tests/test_rx_assemble.py and
tests/test_gpu_rx_assemble.py share.  Test infrastructure.

- assemble_model(): the rule of include/rxgpu.h ("TCP stream assembly") in
  numpy: group heads from a comparison with the predecessor, the covered bytes
  by one running maximum over (group, end), the streams by prefix sums.  No
  code shared with csrc/rx_assemble_host.cpp or the kernels;
- host_rule() / sequential(): the host rule over streams, and a receiver
  without an out-of-order buffer that takes the same records one at a time;
  random_group() draws what test_rx_assemble.py compares the two on;
- rule_cases() / HAND: the rule's edge cases as frames made with
  tests/frames.py, each case's take list and streams written out by hand;
- AsmPair: byte streams that oracle/ref_stack.c receives
  clean while nstack receives them dirty (re-cut retransmits, drops,
  duplicates, overlaps, data without PSH, permuted inside the burst)."""
from __future__ import annotations

import numpy as np

import frames as F
import gro_ref as G
import oracle_bind as O
import order_ref as D
import rxgpu as R

L = G.L
M32 = 0xFFFFFFFF
FIN, HOLE = R.STREAM_FIN, R.STREAM_HOLE


# ---- the rule ------------------------------------------------------------------
def avail_of(seg, caps):
    """captured bytes past each record's TCP header; caps by frame index"""
    cap = np.asarray(caps, np.int64)[seg["frame"]]
    return np.maximum(cap - 34 - 4 * seg["hl"].astype(np.int64), 0).astype(np.uint32)


def assemble_model(seg, sip, avail):
    """ordered records -> dict(stream, skip, take, dst, dlen)"""
    n = len(seg)
    if n == 0:
        z = np.zeros(0, np.uint32)
        return dict(stream=np.zeros(0, R.TCP_STREAM_DTYPE), skip=z, take=z, dst=z, dlen=z)
    pos = np.arange(n)
    movable = (seg["flags"] & 0x06) == 0
    head = np.ones(n, bool)
    same = movable[1:] & movable[:-1] & (sip[1:] == sip[:-1])
    for name in ("flow", "sport", "dport"):
        same &= seg[name][1:] == seg[name][:-1]
    head[1:] = ~same
    h = np.maximum.accumulate(np.where(head, pos, 0))
    grp = np.cumsum(head) - 1
    plen = seg["plen"].astype(np.int64)
    usable = (plen <= 0) | (avail.astype(np.int64) >= plen)
    dlen = np.where(movable & usable & (plen > 0), plen, 0)
    seq = seg["seq"].astype(np.int64)
    a = (seq - seq[h]) & M32
    end = a + dlen
    # the maximum of end over the group's records before j: end < 2^33, so one
    # running maximum over grp * 2^34 + end never looks into another group
    BIG = 1 << 34
    inc = np.maximum.accumulate(grp * BIG + end) - grp * BIG
    cov = np.zeros(n, np.int64)
    cov[1:] = np.where(head[1:], 0, inc[:-1])
    ns = np.maximum(a, cov)
    take = end - np.minimum(end, ns)
    skip = dlen - take
    finok = movable & usable & ((seg["flags"] & 0x01) != 0) & (end >= cov)
    hole = ~head & (a > cov)
    start = head | hole
    start[1:] |= ~head[1:] & finok[:-1]
    first = np.nonzero(start)[0]
    last = np.append(first[1:], n) - 1
    st = np.zeros(len(first), R.TCP_STREAM_DTYPE)
    st["first"] = first
    st["nseg"] = last - first + 1
    st["seq"] = (seq[h][first] + ns[first]) & M32
    st["ack"] = seg["ack"][last]
    st["bytes"] = np.add.reduceat(take, first)
    st["flags"] = np.where(finok[last], FIN, 0) | np.where(hole[first], HOLE, 0)
    padded = (st["bytes"].astype(np.int64) + 15) // 16 * 16
    st["offset"] = np.cumsum(padded) - padded
    before = np.cumsum(take) - take
    sid = np.cumsum(start) - 1
    dst = st["offset"].astype(np.int64)[sid] + before - before[first][sid]
    u = np.uint32
    return dict(stream=st, skip=skip.astype(u), take=take.astype(u), dst=dst.astype(u),
                dlen=dlen.astype(u))


def payload_image(frames, seg, model, size, cap, fill):
    """the payload buffer the device leaves: `size` bytes of `fill`, every
    stream that ends inside `cap` written with its 16-B zero pad; returns
    (image, payload bytes used, overflow)"""
    img = np.full(size, fill, np.uint8)
    st = model["stream"]
    over = 0
    for s in st:
        o, nb = int(s["offset"]), int(s["bytes"])
        pe = o + (nb + 15) // 16 * 16
        if pe > cap:
            over = 1
            continue
        img[o + nb:pe] = 0
        for j in range(int(s["first"]), int(s["first"] + s["nseg"])):
            t = int(model["take"][j])
            if t:
                g = seg[j]
                a = 34 + 4 * int(g["hl"]) + int(model["skip"][j])
                d = int(model["dst"][j])
                img[d:d + t] = np.frombuffer(frames[int(g["frame"])][a:a + t], np.uint8)
    used = 0
    if len(st):
        used = int(st["offset"][-1]) + (int(st["bytes"][-1]) + 15) // 16 * 16
    return img, used, over


# ---- the host rule and the receiver it must equal ---------------------------------
def _i32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def host_rule(streams, R0):
    """one ESTABLISHED connection's streams in order -> (ranges [(seq, n)],
    acks [acknum], rcv_nxt, eof, bytes already received, streams behind a hole)"""
    Rn, ranges, acks, eof, dup, holes = R0 & M32, [], [], False, 0, 0
    for s in streams:
        nb, fin = int(s["bytes"]), bool(s["flags"] & FIN)
        if not nb and not fin:
            continue
        d = _i32(Rn - int(s["seq"]))
        if d < 0:
            holes += 1
            acks.append(Rn)
            continue
        fresh = nb - d if nb > d else 0
        dup += nb - fresh
        if fresh:
            ranges.append(((int(s["seq"]) + d) & M32, fresh))
            Rn = (Rn + fresh) & M32
        if fin and d <= nb:
            eof = True
            Rn = (Rn + 1) & M32
        acks.append(Rn)
        if eof:
            break
    return ranges, acks, Rn, eof, dup, holes


def sequential(seg, dlen, usable, R0):
    """the same records one at a time, no out-of-order buffer -> (ranges,
    rcv_nxt, eof)"""
    Rn, ranges, eof = R0 & M32, [], False
    for g, nb, ok in zip(seg, dlen, usable):
        nb = int(nb)
        fin = bool(g["flags"] & 0x01) and bool(ok) and not (g["flags"] & 0x06)
        if not nb and not fin:
            continue
        d = _i32(Rn - int(g["seq"]))
        if d < 0:
            continue
        fresh = nb - d if nb > d else 0
        if fresh:
            ranges.append(((int(g["seq"]) + d) & M32, fresh))
            Rn = (Rn + fresh) & M32
        if fin and d <= nb:
            eof = True
            Rn = (Rn + 1) & M32
            break
    return ranges, Rn, eof


def merged(ranges):
    out = []
    for s, n in ranges:
        if out and (out[-1][0] + out[-1][1]) & M32 == s:
            out[-1] = (out[-1][0], out[-1][1] + n)
        else:
            out.append((s, n))
    return out


def random_group(rng):
    """one group of 1 to 7 ordered records with random overlaps, holes, FINs and
    cut captures, and a rcv_nxt near it: (seg, sip, avail, R)"""
    k = int(rng.integers(1, 8))
    base = int(rng.choice([1000, 0x7FFFFE00, 0xFFFFFC00, int(rng.integers(0, 1 << 32))]))
    a = np.sort(rng.integers(0, int(rng.choice([4, 400, 3000])), k))
    a[0] = 0
    seg = np.zeros(k, R.SEGMENT_DTYPE)
    seg["frame"] = np.arange(k)
    seg["seq"] = (base + a) & M32
    seg["plen"] = rng.choice([0, 1, 50, 100, 400, 1460, -4], k)
    seg["flags"] = rng.choice([0x18, 0x10, 0x11, 0x19], k, p=[0.55, 0.2, 0.1, 0.15])
    seg["hl"], seg["sport"], seg["dport"], seg["ack"] = 5, 7, 9, rng.integers(0, 1 << 32, k)
    avail = np.where(rng.random(k) < 0.1, 3, 2000).astype(np.uint32)
    sip = np.full(k, 5, np.uint32)
    Rn = (base + int(rng.integers(-1500, 3500))) & M32
    return seg, sip, avail, Rn


# ---- the edge cases, by hand --------------------------------------------------------
# label -> (take of each record, [(seq, bytes, flags, nseg)] of the streams)
HAND = {
    0: ([100, 0, 100], [(1000, 200, 0, 3)]),                          # an exact duplicate
    1: ([100, 50], [(1000, 150, 0, 2)]),                              # a partial overlap
    2: ([300, 0, 50], [(1000, 350, 0, 3)]),                           # a contained segment
    3: ([100, 100, 10], [(1000, 100, 0, 1), (1200, 110, HOLE, 2)]),   # a hole
    4: ([50, 100], [(900, 50, 0, 1), (1000, 100, HOLE, 1)]),          # an old duplicate, then new data
    5: ([100, 100, 0], [(0xFFFFFFC0, 200, 0, 3)]),                    # the sequence wrap
    6: ([100, 50], [(1000, 150, FIN, 2)]),                            # data + FIN
    7: ([100, 0, 0], [(1000, 100, FIN, 2), (1100, 0, FIN, 1)]),       # a duplicate FIN
    8: ([300, 0], [(1000, 300, 0, 2)]),                               # a FIN inside covered data
    9: ([100, 100], [(1000, 200, 0, 2)]),                             # data without PSH
    10: ([100, 0, 100], [(1000, 100, 0, 2), (1200, 100, HOLE, 1)]),   # a capture cut mid-payload
    11: ([100, 0, 100], [(1000, 200, 0, 3)]),                         # plen < 0
    12: ([100, 0, 100], [(1000, 100, 0, 1), (5, 0, 0, 1), (1100, 100, 0, 1)]),   # a SYN barrier
    13: ([100, 0, 100], [(1000, 100, 0, 1), (5, 0, 0, 1), (1100, 100, 0, 1)]),   # a RST barrier
    14: ([100, 0, 100], [(1000, 200, 0, 3)]),                         # a pure ACK between data
    15: ([100, 50], [(1000, 150, 0, 2)]),                             # overlap, other content
    "L": ([100, 100, 100], [(1000, 100, 0, 1), (1100, 100, 0, 1), (1100, 100, 0, 1)]),  # two sources
}
NCASES = 16


def rule_cases(rng, dport=9999, base=0):
    """[(label, frame, captured length)] in burst order (every connection's own
    records already in sequence order): label k = connection G.conn(base + k),
    'L' = no connection (the listener's id)"""
    out = []

    def add(k, seq, n=100, flags=0x18, cut=0, body=None, **kw):
        if k in ("L1", "L2"):
            cip, cport = ("10.0.9.1" if k == "L1" else "10.0.9.2"), 5000
            k = "L"
        else:
            cip, cport = G.conn(base + k)
        p = body if body is not None else G._p(rng, n - cut) + bytes(cut)
        f = F.tcp_frame(cip, cport, L, dport, p, seq=seq & M32, flags=flags, **kw)
        out.append((k, f, len(f) - cut))
    add(0, 1000), add(0, 1000), add(0, 1100)
    add(1, 1000), add(1, 1050)
    add(2, 1000, 300), add(2, 1100), add(2, 1300, 50)
    add(3, 1000), add(3, 1200), add(3, 1300, 10)
    add(4, 900, 50), add(4, 1000)
    add(5, 0xFFFFFFC0), add(5, 0x24), add(5, 0x24)
    add(6, 1000), add(6, 1100, 50, flags=0x19)
    add(7, 1000), add(7, 1100, 0, flags=0x11), add(7, 1100, 0, flags=0x11)
    add(8, 1000, 300), add(8, 1100, 50, flags=0x19)
    add(9, 1000, flags=0x10), add(9, 1100)
    add(10, 1000), add(10, 1100, cut=30), add(10, 1200)
    add(11, 1000), add(11, 1100, 7, tl=30, tl_cksum=True), add(11, 1100)
    add(12, 1000), add(12, 5, 0, flags=0x02), add(12, 1100)
    add(13, 1000), add(13, 5, 10, flags=0x04), add(13, 1100)
    add(14, 1000), add(14, 1100, 0, flags=0x10), add(14, 1100)
    add(15, 1000, body=b"A" * 100), add(15, 1050, body=b"B" * 100)
    add("L1", 1000, flags=0x10), add("L2", 1100, flags=0x10), add("L1", 1100, flags=0x10)
    return out


def check_hand(seg, model, flow_of):
    """the model's (or anyone's) answer restricted to every case's records
    equals HAND; flow_of(label) = its id"""
    st = model["stream"]
    for label, (take, streams) in HAND.items():
        idx = np.nonzero(seg["flow"] == flow_of(label))[0]
        assert len(idx) == len(take) and np.all(np.diff(idx) == 1), label
        assert list(model["take"][idx]) == take, (label, list(model["take"][idx]))
        mine = st[(st["first"] >= idx[0]) & (st["first"] <= idx[-1])]
        got = [(int(s["seq"]), int(s["bytes"]), int(s["flags"]), int(s["nseg"])) for s in mine]
        assert got == streams, (label, got)
        assert np.all(mine["offset"] % 16 == 0) and np.all(mine["reserved"] == 0)


# ---- the socket layer against the oracle ------------------------------------------
class AsmPair(G.GroPair):
    """oracle/ref_stack.c receives each connection's byte stream clean (every
    byte once, in order, PSH|ACK); nstack receives it dirty, from a sender that
    goes back to the model's rcv_nxt every round: re-cut, about 20 % of the
    segments dropped, about 20 % duplicated or overlapped, some data without
    PSH, permuted inside the burst.  The model here (order_model,
    assemble_model, host_rule on the burst's records) says what nstack must
    acknowledge; the oracle is fed exactly the bytes the model took.
    mode: 'cpu' (nstack_deliver), 'gpu' (nstack_rx_burst), 'pipe'."""

    def __init__(self, ns, mode, seed, n_clients=5):
        super().__init__(ns, mode, 0)
        self.rng = np.random.default_rng(seed)
        self.keys = [(*G.conn(k), G.LISTEN[k % 2][1]) for k in range(n_clients)]
        self.isn = [int(self.rng.integers(1, 1 << 32)) for _ in self.keys]
        if seed % 2:
            self.isn[0] = M32 - 700            # the data crosses the wrap
        self.data = [G._p(self.rng, int(self.rng.integers(2500, 9000))) for _ in self.keys]
        self.fin = [k != n_clients - 1 for k in range(n_clients)]
        self.Rn = [(s + 1) & M32 for s in self.isn]      # the model's rcv_nxt
        self.closed = [False] * n_clients
        self.want_acks = [[] for _ in self.keys]
        self.want_dup = self.want_holes = 0

    def _tcp(self, k, off, payload=b"", flags=0x18):
        cip, cport, dport = self.keys[k]
        return F.tcp_frame(cip, cport, L, dport, payload, flags=flags, seq=(self.isn[k] + 1 + off) & M32)

    def _send(self, frames):
        """one burst into nstack (rcs are not compared: the oracle sees other frames)"""
        u, t, gen = self.ns.flows(with_gen=True)
        buf, off, lens = F.pack_frames(frames)
        v = self.ns.to_ids(O.Tables(u, t).classify(buf, off, lens, 6))
        if self.mode == "cpu":
            self.ns.deliver(frames, v, np.zeros(len(frames), np.int32), gen)
        elif self.mode == "gpu":
            _, _, vg = self.ns.rx_burst(frames)
            assert vg.tobytes() == v.tobytes()
        else:
            self.ns.rx_submit(frames)
            _, _, vg = self.ns.rx_complete()
            assert vg.tobytes() == v.tobytes()
        return v

    def handshakes(self):
        frames = []
        for k in range(len(self.keys)):
            cip, cport, dport = self.keys[k]
            frames.append(F.tcp_frame(cip, cport, L, dport, b"", flags=0x02, seq=self.isn[k]))
            frames.append(self._tcp(k, 0, flags=0x10))
        for f in frames:
            self.os.rx(f)
        self._send(frames)
        self.accept_all()

    def _dirty(self, k):
        """connection k's frames of one round, from the model's rcv_nxt on"""
        rng, data = self.rng, self.data[k]
        una = (self.Rn[k] - self.isn[k] - 1) & M32
        out = []
        if una >= len(data):                         # only the FIN is left
            if rng.random() < 0.75:
                out.append(self._tcp(k, len(data), flags=0x11))
            if rng.random() < 0.3:
                out.append(self._tcp(k, len(data), flags=0x11))
            if rng.random() < 0.5:                   # an old retransmit beside it
                a = int(rng.integers(0, len(data)))
                out.append(self._tcp(k, a, data[a:a + 300]))
            return out
        pos = max(0, una - int(rng.choice([0, 0, 1, 40, 700])))      # re-cut from further back
        end = min(len(data), una + int(rng.integers(1, 5000)))
        while pos < end:
            n = min(int(rng.choice([1, 7, 100, 600, 1460])), end - pos)
            last = pos + n == len(data)
            fl = 0x10 if rng.random() < 0.25 else 0x18
            if last and self.fin[k] and rng.random() < 0.5:
                fl = 0x19                            # the FIN rides on the last data
            f = self._tcp(k, pos, data[pos:pos + n], flags=fl)
            x = rng.random()
            if x >= 0.2:                             # (else: lost)
                out.append(f)
            if 0.2 <= x < 0.3:                       # an exact duplicate
                out.append(f)
            elif 0.3 <= x < 0.4:                     # a retransmit cut elsewhere, overlapping
                a = max(0, pos - int(rng.integers(0, 200)))
                b = min(len(data), pos + n + int(rng.integers(0, 200)))
                out.append(self._tcp(k, a, data[a:b][:1460]))
            pos += n
        return out

    def round(self):
        rng = self.rng
        per = {k: self._dirty(k) for k in range(len(self.keys))
               if not self.closed[k] and (self.fin[k] or self.Rn[k] != (self.isn[k] + 1 + len(self.data[k])) & M32)}
        per = {k: [v[i] for i in rng.permutation(len(v))] for k, v in per.items() if v}
        frames = []
        while per:                                   # connections interleaved
            k = list(per)[int(rng.integers(len(per)))]
            frames.append(per[k].pop())
            if not per[k]:
                del per[k]
        if not frames:
            return
        before = list(self.Rn)
        v = self._send(frames)
        # what the rule says of this burst
        flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 else None for x in v]
        caps = [len(f) for f in frames]
        seg, sip = G.records(frames, caps, flows)
        perm, _ = D.order_model(seg, sip)
        seg, sip = seg[perm], sip[perm]
        m = assemble_model(seg, sip, avail_of(seg, caps))
        st = m["stream"]
        eofs = []
        for k, (cip, cport, dport) in enumerate(self.keys):
            fid = self.ns.lookup_tcp(R.ip_raw(cip), R.ip_raw(L), R.port_raw(cport), R.port_raw(dport))
            mine = st[seg["flow"][st["first"]] == fid]
            if not len(mine) or self.closed[k]:
                continue
            rec = seg["flow"] == fid
            self.want_dup += int(m["skip"][rec].sum())
            _, acks, self.Rn[k], eof, dup, holes = host_rule(mine, self.Rn[k])
            self.want_acks[k] += acks
            self.want_dup += dup
            self.want_holes += holes
            if eof:
                self.closed[k] = True
                eofs.append(k)
        # the oracle: the bytes the model took, clean
        for k in range(len(self.keys)):
            a = (before[k] - self.isn[k] - 1) & M32
            b = (self.Rn[k] - self.isn[k] - 1 - (1 if k in eofs else 0)) & M32
            while a < b:
                n = min(1460, b - a)
                self.os.rx(self._tcp(k, a, self.data[k][a:a + n]))
                a += n
            if k in eofs:
                self.os.rx(self._tcp(k, len(self.data[k]), flags=0x11))
        self.drain()

    def done(self):
        return all(self.closed[k] if self.fin[k] else
                   self.Rn[k] == (self.isn[k] + 1 + len(self.data[k])) & M32 for k in range(len(self.keys)))

    def run(self, max_rounds=80):
        """returns the rounds it took"""
        self.handshakes()
        r = 0
        while not self.done():
            assert r < max_rounds, "the sender never got through"
            self.round()
            r += 1
        return r

    def check(self):
        """per connection: the bytes read, the EOF position, the final state,
        rcv_nxt and every queued ACK's acknum"""
        self.compare_tcbs(self.keys)
        for k, (cip, cport, dport) in enumerate(self.keys):
            key = (R.ip_raw(cip), R.port_raw(cport), dport)
            tn, to = G._tokens(self.reads_ns[key]), G._tokens(self.reads_os[key])
            assert tn == to, k
            assert to == ([self.data[k]] + (["EOF"] if self.fin[k] else [])), k
            t = (R.ip_raw(cip), R.ip_raw(L), R.port_raw(cport), R.port_raw(dport))
            q = self.ns.tcb_sndq(*t)
            assert q[0] == (0x12, (self.isn[k] + 1) & M32)
            assert [a for fl, a in q[1:]] == self.want_acks[k], (k, q, self.want_acks[k])
            assert all(fl == 0x10 for fl, _ in q[1:])
            assert self.ns.tcb_state(*t)[1] == self.Rn[k]
