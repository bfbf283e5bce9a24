"""Python model of the SYN-cookie rule (include/rxgpu.h, "SYN cookies"): an
independent SipHash-2-4 on Python integers, the cookie, and the burst pass
(status bytes, compacted SYN-ACK descriptors, totals) written from the rule's
text, byte by byte.  Also the burst builders the CPU and GPU tests share.
Test infrastructure: no product code is imported here but the dtypes."""
from __future__ import annotations

import json
import os
import struct

import numpy as np

import frames as F
import rxgpu as R

M64 = (1 << 64) - 1
KEY = bytes(range(16))
LOCAL = "192.168.0.10"
CLS_ARP, CLS_UDP, CLS_TCP = 0, 3, 4


def kats():
    with open(os.path.join(os.path.dirname(__file__), "golden", "siphash_kats.json")) as fh:
        return json.load(fh)


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def siphash24(key: bytes, msg: bytes) -> int:
    k0, k1 = struct.unpack("<QQ", key)
    v = [k0 ^ 0x736F6D6570736575, k1 ^ 0x646F72616E646F6D, k0 ^ 0x6C7967656E657261,
         k1 ^ 0x7465646279746573]

    def rnd():
        v[0] = (v[0] + v[1]) & M64
        v[1] = _rotl(v[1], 13) ^ v[0]
        v[0] = _rotl(v[0], 32)
        v[2] = (v[2] + v[3]) & M64
        v[3] = _rotl(v[3], 16) ^ v[2]
        v[0] = (v[0] + v[3]) & M64
        v[3] = _rotl(v[3], 21) ^ v[0]
        v[2] = (v[2] + v[1]) & M64
        v[1] = _rotl(v[1], 17) ^ v[2]
        v[2] = _rotl(v[2], 32)

    tail = len(msg) % 8
    words = [int.from_bytes(msg[i:i + 8], "little") for i in range(0, len(msg) - tail, 8)]
    words.append(int.from_bytes(msg[len(msg) - tail:], "little") | ((len(msg) & 0xFF) << 56))
    for m in words:
        v[3] ^= m
        rnd()
        rnd()
        v[0] ^= m
    v[2] ^= 0xFF
    for _ in range(4):
        rnd()
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def cookie(key: bytes, sip: int, dip: int, sport: int, dport: int, isn: int, t: int) -> int:
    """sip, dip, sport, dport: the raw (little-endian) loads of the frame's fields"""
    t &= 0xFFFFFFFF
    msg = struct.pack("<IIHHIII", sip, dip, sport, dport, isn & 0xFFFFFFFF, t, 0)
    return ((t & 0xFF) << 24) | (siphash24(key, msg) & 0xFFFFFF)


def run(buf, off, lens, unit, verdicts, lmask, id_space, key=KEY, t=0, max_age=2, window=14600):
    """the burst pass: (status u8[n], txd TXD_DTYPE[k], totals u32[4])"""
    n = len(lens)
    status = np.zeros(n, np.uint8)
    txd = []
    nok = nbad = 0
    for i in range(n):
        v = verdicts[i]
        if lens[i] < 54 or v["cls"] != CLS_TCP or v["rc"] != 0:
            continue
        fid = int(v["flow_id"])
        if fid >= id_space or not (int(lmask[fid >> 5]) >> (fid & 31)) & 1:
            continue
        o = int(off[i]) << unit
        f = bytes(buf[o:o + 54])
        fl = f[47]
        sip, dip = struct.unpack_from("<II", f, 26)
        sport, dport = struct.unpack_from("<HH", f, 34)
        seq, ack = struct.unpack_from(">II", f, 38)
        if fl & 0x17 == 0x02:
            status[i] = R.CK_SYN
            d = np.zeros(1, R.TXD_DTYPE)
            d["dst_mac"][0] = np.frombuffer(f[6:12], np.uint8)
            d["src_mac"][0] = np.frombuffer(f[0:6], np.uint8)
            d["sip"], d["dip"], d["sport"], d["dport"] = dip, sip, dport, sport
            d["seq"] = cookie(key, sip, dip, sport, dport, seq, t)
            d["ack"] = (seq + 1) & 0xFFFFFFFF
            d["tcp_flags"], d["hdrlen_off"], d["kind"], d["window"] = 0x12, 0x50, R.TXD_TCP, window
            txd.append(d)
        elif fl & 0x16 == 0x10:
            c, isn = (ack - 1) & 0xFFFFFFFF, (seq - 1) & 0xFFFFFFFF
            age = ((t & 0xFF) - (c >> 24)) & 0xFF
            ok = age <= max_age and (c & 0xFFFFFF) == \
                (cookie(key, sip, dip, sport, dport, isn, (t - age) & 0xFFFFFFFF) & 0xFFFFFF)
            status[i] = R.CK_ACK_OK if ok else R.CK_ACK_BAD
            nok, nbad = nok + ok, nbad + (not ok)
    out = np.concatenate(txd) if txd else np.zeros(0, R.TXD_DTYPE)
    return status, out, np.array([len(txd), nok, nbad, 0], np.uint32)


# ---- builders ---------------------------------------------------------------------
def raw_tuple(src: str, sport: int, dst: str, dport: int):
    """the raw loads of a frame's address and port fields"""
    return (int.from_bytes(F.ip4(src), "little"), int.from_bytes(F.ip4(dst), "little"),
            int.from_bytes(struct.pack(">H", sport), "little"),
            int.from_bytes(struct.pack(">H", dport), "little"))


def syn(src, sport, dport, isn, payload=b"", flags=0x02, **kw):
    return F.tcp_frame(src, sport, LOCAL, dport, payload, flags=flags, seq=isn, ack=0, **kw)


def ack_for(src, sport, dport, isn, t, key=KEY, payload=b"", flags=0x10, dseq=0, dack=0, **kw):
    """the handshake ACK a client sends to the SYN-ACK made with counter t"""
    c = cookie(key, *raw_tuple(src, sport, LOCAL, dport), isn, t)
    return F.tcp_frame(src, sport, LOCAL, dport, payload, flags=flags, seq=(isn + 1 + dseq) & 0xFFFFFFFF,
                       ack=(c + 1 + dack) & 0xFFFFFFFF, **kw)


def verdict(cls=CLS_TCP, rc=0, flow_id=0):
    v = np.zeros(1, R.VERDICT_DTYPE)
    v["cls"], v["rc"], v["flow_id"], v["cksum_ok"] = cls, rc, flow_id, 1
    return v


def lmask_of(ids, id_space):
    m = np.zeros((id_space + 31) // 32, np.uint32)
    for i in ids:
        m[i >> 5] |= np.uint32(1 << (i & 31))
    return m


ID_SPACE = 70                                  # three mask words, the last partly used
LISTENERS = (0, 3, 31, 32, 64, 69)


def fuzz_burst(seed, n, t, kind="mixed", key=KEY, max_age=2):
    """n frames of 54-1514 bytes with fuzzed verdicts: (frames, caplens,
    verdicts).  kind: "syn" (every frame a SYN to a listener), "none" (no
    candidate) or "mixed" (SYNs, valid / stale / forged ACKs, other flags,
    non-listener ids, ids past the id space, bad checksums, UDP, ARP and
    captures cut below 54 bytes)"""
    rng = np.random.default_rng(seed)
    frames, caps, vs = [], [], []
    lst = list(LISTENERS)
    for i in range(n):
        src = "10.%d.%d.%d" % tuple(rng.integers(1, 250, 3))
        sport, dport = int(rng.integers(1024, 65535)), int(rng.integers(1, 65535))
        isn = int(rng.integers(0, 1 << 32))
        big = rng.random() < 0.1
        pay = bytes(rng.integers(0, 256, int(rng.integers(0, 1461 if big else 40)), dtype=np.uint8))
        fid = lst[int(rng.integers(len(lst)))]
        r = 0.0 if kind == "syn" else rng.random()
        cls, rc, cap = CLS_TCP, 0, None
        if r < 0.30:
            f = syn(src, sport, dport, isn, pay if rng.random() < 0.2 else b"")
        elif r < 0.55:
            age = int(rng.integers(0, max_age + 3))
            fl = 0x10 | (0x08 if pay else 0) | (0x01 if rng.random() < 0.2 else 0)
            f = ack_for(src, sport, dport, isn, t - age, key, pay, fl,
                        dack=int(rng.random() < 0.2), dseq=int(rng.random() < 0.1))
        elif r < 0.65:
            f = syn(src, sport, dport, isn, flags=int(rng.choice([0x12, 0x03, 0x04, 0x14, 0x00, 0x06])))
        elif r < 0.72:
            f, fid = syn(src, sport, dport, isn), int(rng.choice([1, 2, 33, 68]))
        elif r < 0.78:
            f, fid = syn(src, sport, dport, isn), int(rng.choice([ID_SPACE, ID_SPACE + 1, 0xFFFFFFFF]))
        elif r < 0.84:
            f, rc = syn(src, sport, dport, isn, corrupt=True), -1
        elif r < 0.90:
            f, cls = F.udp_frame(src, sport, LOCAL, dport, pay), CLS_UDP
        elif r < 0.94:
            f, cls, rc = F.arp_frame(src, LOCAL), CLS_ARP, 1
        else:
            f, cap = syn(src, sport, dport, isn), int(rng.integers(34, 54))
        if kind == "none" and cls == CLS_TCP and rc == 0 and cap is None and fid in LISTENERS:
            fid = 1                            # a control block that does not listen
        frames.append(f)
        caps.append(len(f) if cap is None else cap)
        vs.append(verdict(cls, rc, fid))
    v = np.concatenate(vs) if vs else np.zeros(0, R.VERDICT_DTYPE)
    return frames, caps, v


# ---- the socket-layer scenario (CPU and GPU paths) -------------------------------------
T0 = 1000                                      # the pinned counter
PORT = 8080
NSYN = 1000


def client(i):
    """(src, sport, isn) of SYN-flood client i: distinct sources"""
    return "10.%d.%d.%d" % (1 + i // 62500, 1 + (i // 250) % 250, 1 + i % 250), 1024 + i, 0x10000 * i + 7


def parse_tcp(f: bytes):
    """(dst mac, src mac, raw sip, raw dip, raw sport, raw dport, seq, ack, flags) of a frame"""
    sip, dip = struct.unpack_from("<II", f, 26)
    sport, dport = struct.unpack_from("<HH", f, 34)
    seq, ack = struct.unpack_from(">II", f, 38)
    return f[0:6], f[6:12], sip, dip, sport, dport, seq, ack, f[47]


class Session:
    """drives a stack (R.NStack) through bursts on one of its receive paths:
    'cpu' nstack_deliver with the oracle's verdicts and the lists' generation,
    'stale' the same with the generation withheld (every frame looked up and
    judged alone), 'gpu' nstack_rx_burst, 'pipe' nstack_rx_submit /
    nstack_rx_complete"""

    def __init__(self, ns, mode):
        self.ns, self.mode = ns, mode

    def rx(self, frames):
        ns = self.ns
        if self.mode in ("cpu", "stale"):
            import oracle_bind as O
            u, t, gen = ns.flows(with_gen=True)
            buf, off, lens = F.pack_frames(frames)
            v = ns.to_ids(O.Tables(u, t).classify(buf, off, lens, 6))
            rcs = np.zeros(len(frames), np.int32)
            ns.deliver(frames, v, rcs, gen if self.mode == "cpu" else R.NStack.STALE)
            return list(rcs)
        if self.mode == "gpu":
            return list(ns.rx_burst(frames)[1])
        ns.rx_submit(frames)
        return list(ns.rx_complete()[1])

    def rx_two(self, a, b):
        """two bursts: in flight together on the pipelined path"""
        if self.mode != "pipe":
            return self.rx(a) + self.rx(b)
        self.ns.rx_submit(a)
        self.ns.rx_submit(b)
        return list(self.ns.rx_complete()[1]) + list(self.ns.rx_complete()[1])


def scenario(ns, mode, cookies=1):
    """the SYN flood and one legitimate connection; returns what an observer
    sees: per step the tcb count, the counters, return codes and every read.
    cookies = 0: the same frames with the option off"""
    s = Session(ns, mode)
    log = {}
    ns.set_local(LOCAL, F.LOCAL_MAC)
    lfd = ns.socket(R.SOCK_STREAM)
    assert ns.bind(lfd, LOCAL, PORT) == 0 and ns.listen(lfd) == 0
    ns.syncookie_tick(T0)
    if cookies:
        ns.set_syncookies(cookies, KEY)
    syns = [syn(*client(i)[:2], PORT, client(i)[2]) for i in range(NSYN)]
    rcs = s.rx_two(syns[:NSYN // 2], syns[NSYN // 2:])
    log["flood"] = (ns.tcb_count(), ns.syncookie_stats(), sorted(set(rcs)))
    log["synacks"] = ns.tx_burst(max_frames=2 * NSYN, cap_bytes=1 << 18, cksum=mode in ("gpu", "pipe"))
    if not cookies:
        return log
    # client 7 completes its handshake with data on the ACK; client 8's ACK is
    # forged (one bit of the cookie), client 9's is stale (made max_age + 1 ago)
    src, sport, isn = client(7)
    f7 = ack_for(src, sport, PORT, isn, T0, payload=b"hello", flags=0x18)
    f8 = ack_for(*client(8)[:2], PORT, client(8)[2], T0, dack=0x40)
    f9 = ack_for(*client(9)[:2], PORT, client(9)[2], T0 - 3)
    rcs = s.rx([f8, f7, f9])
    log["acks"] = (ns.tcb_count(), ns.syncookie_stats(), rcs)
    assert log["acks"][0] == 2, log["acks"]    # (naccept would block on a stack without the connection)
    cfd, a = ns.accept(lfd)
    log["accept"] = (cfd > lfd, a.sin_port, a.sin_addr)
    log["read1"] = ns.recv(cfd, 64)
    c = cookie(KEY, *raw_tuple(src, sport, LOCAL, PORT), isn, T0)
    s.rx([F.tcp_frame(src, sport, LOCAL, PORT, b"world!", flags=0x18, seq=isn + 6, ack=c + 1)])
    log["read2"] = ns.recv(cfd, 64)
    s.rx([F.tcp_frame(src, sport, LOCAL, PORT, b"", flags=0x11, seq=isn + 12, ack=c + 1)])
    log["eof"] = ns.recv(cfd, 64)
    log["state"] = ns.tcb_state(*raw_tuple(src, sport, LOCAL, PORT))[:3]
    log["end"] = (ns.tcb_count(), ns.syncookie_stats())
    return log
