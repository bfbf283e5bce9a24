"""A bytes-level model of the L2 responder's rule (include/rxgpu.h, "L2
responder"): ARP requests for a local address and ICMP echo requests to one
are answered, the answers packed at 64-B boundaries in burst order.  It shares
no code with csrc/rx_l2.hip or csrc/rx_l2_host.cpp: its own checksum (Python
integers over big-endian words), its own layout.  Plus the frame builders, the
hand-written cases and the fuzzed bursts of tests/test_rx_l2.py and
tests/test_gpu_rx_l2.py.  Test infrastructure."""
import struct

import numpy as np

import frames as F

CLS_ARP, CLS_NON_IP, CLS_IPV4_OTHER, CLS_UDP, CLS_TCP = 0, 1, 2, 3, 4
ARP_REQ, ARP_REPLY, ECHO, ECHO_BAD = 1, 2, 3, 4
LOCAL_IP, LOCAL_MAC = "192.168.1.10", bytes.fromhex("000c296a014d")
LOCAL2_IP, LOCAL2_MAC = "10.9.8.7", bytes.fromhex("02005e000207")
PEER_IP, PEER_MAC = "192.168.1.20", bytes.fromhex("02aabbccddee")
LOCALS = [(LOCAL_IP, LOCAL_MAC), (LOCAL2_IP, LOCAL2_MAC)]


# ---- the model ------------------------------------------------------------------------
def csum(b: bytes) -> int:
    """folded one's-complement sum of big-endian 16-bit words, an odd tail
    byte padded with zero: 0 only for all-zero bytes"""
    if len(b) & 1:
        b = b + b"\0"
    s = sum(struct.unpack(">%dH" % (len(b) // 2), b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def judge(f: bytes, cls: int, local):
    """(status, answer bytes or None) of one captured frame; local: [(ip4
    bytes, mac bytes)]"""
    if len(f) < 42 or f[6] & 1:
        return 0, None
    if cls == CLS_ARP:
        if f[14:20] != bytes.fromhex("000108000604"):
            return 0, None
        mac = next((m for ip, m in local if ip == f[38:42]), None)
        if mac is None:
            return 0, None
        op = f[20] << 8 | f[21]
        if op == 2:
            return ARP_REPLY, None
        if op != 1:
            return 0, None
        return ARP_REQ, (f[22:28] + mac + bytes.fromhex("08060001080006040002") + mac + f[38:42]
                         + f[22:28] + f[28:32])
    if cls != CLS_IPV4_OTHER:
        return 0, None
    if f[14] != 0x45 or f[23] != 1 or (f[20] << 8 | f[21]) & 0x3FFF:
        return 0, None
    mac = next((m for ip, m in local if ip == f[30:34]), None)
    if mac is None or f[34] != 8 or f[35] != 0:
        return 0, None
    tl = f[16] << 8 | f[17]
    if tl < 28:
        return 0, None
    if 14 + tl > len(f) or csum(f[34:14 + tl]) != 0xFFFF:
        return ECHO_BAD, None
    ip = bytearray(bytes([0x45, 0]) + f[16:18] + bytes([0, 0, 0, 0, 64, 1, 0, 0]) + f[30:34] + f[26:30])
    ip[10:12] = struct.pack(">H", ~csum(bytes(ip)) & 0xFFFF)
    msg = bytearray(bytes(4) + f[38:14 + tl])
    msg[2:4] = struct.pack(">H", ~csum(bytes(msg)) & 0xFFFF)
    return ECHO, f[6:12] + mac + b"\x08\x00" + bytes(ip) + bytes(msg)


def run(buf, off, lens, unit, verd, local, cap_bytes):
    """one burst: (status u8[n], frames bytes (the span), roff, rlen, rsrc,
    totals[6]); local: [(dotted or bytes ip, mac)]"""
    loc = [(F.ip4(ip) if isinstance(ip, str) else bytes(ip), bytes(m)) for ip, m in local]
    n = len(lens)
    status = np.zeros(n, np.uint8)
    out, roff, rlen, rsrc, cnt, full = bytearray(), [], [], [], [0] * 5, False
    for i in range(n):
        o = int(off[i]) << unit
        st, ans = judge(bytes(buf[o:o + int(lens[i])]), int(verd[i]["cls"]), loc)
        status[i] = st
        cnt[st] += 1
        if ans is None or full:
            continue
        slot = -(-len(ans) // 64) * 64
        if len(out) + slot > cap_bytes:
            full = True
            continue
        roff.append(len(out) // 64), rlen.append(len(ans)), rsrc.append(i)
        out += ans + bytes(slot - len(ans))
    tot = np.array([cnt[1], cnt[2], cnt[3], cnt[4], len(roff), len(out) // 64], np.uint32)
    return (status, bytes(out), np.array(roff, np.uint32), np.array(rlen, np.uint16),
            np.array(rsrc, np.uint32), tot)


# ---- frame builders -------------------------------------------------------------------
def arp(op=1, sip=PEER_IP, tip=LOCAL_IP, sha=PEER_MAC, *, src=None, plen=4, pad=18, tha=bytes(6)):
    body = struct.pack(">HHBBH", 1, 0x0800, 6, plen, op) + sha + F.ip4(sip) + tha + F.ip4(tip)
    return F.ether(body + bytes(pad), 0x0806, dst=b"\xff" * 6, src=sha if src is None else src)


def echo(payload=b"", src=PEER_IP, dst=LOCAL_IP, *, typ=8, code=0, ident=1, seq=1, frag=0x4000,
         ver_ihl=0x45, tl=None, smac=PEER_MAC, dmac=LOCAL_MAC, trail=b"", ip_id=0x1234):
    """an ICMP message of 8 + len(payload) bytes with a good checksum"""
    msg = bytearray(struct.pack(">BBHHH", typ, code, 0, ident, seq) + payload)
    msg[2:4] = struct.pack(">H", ~csum(bytes(msg)) & 0xFFFF)
    tl = 20 + len(msg) if tl is None else tl
    ip = bytearray(struct.pack(">BBHHHBBH4s4s", ver_ihl, 0, tl, ip_id, frag, 64, 1, 0, F.ip4(src),
                               F.ip4(dst)))
    ip[10:12] = struct.pack(">H", ~csum(bytes(ip)) & 0xFFFF)
    return dmac + smac + b"\x08\x00" + bytes(ip) + bytes(msg) + trail


def _flip(frame: bytes, at: int, bit: int) -> bytes:
    b = bytearray(frame)
    b[at] ^= bit
    return bytes(b)


# ---- two known answers, worked out by hand --------------------------------------------
# who-has 192.168.1.10 tell 192.168.1.20 (60 bytes on the wire), and its reply
KA_ARP_REQ = bytes.fromhex(
    "ffffffffffff" "02aabbccddee" "0806" "0001" "0800" "06" "04" "0001"
    "02aabbccddee" "c0a80114" "000000000000" "c0a8010a" + "00" * 18)
KA_ARP_REPLY = bytes.fromhex(
    "02aabbccddee" "000c296a014d" "0806" "0001" "0800" "06" "04" "0002"
    "000c296a014d" "c0a8010a" "02aabbccddee" "c0a80114")
# a 98-byte ping: id 1, seq 1, payload 00 01 .. 37.  Payload words add to
# 0x2F4 * 256 + 0x310 = 0x2F710; request: + 0x0800 + 1 + 1 = 0x2FF12 -> 0xFF14,
# checksum 0x00EB; reply: 0x2F712 -> 0xF714, checksum 0x08EB.  Reply header:
# 4500 + 0054 + 4001 + c0a8 + 010a + c0a8 + 0114 = 0x208C3 -> 0x08C5, checksum
# 0xF73A.  (Request header: + 1234 + 4000 -> 0x25AF7 -> 0x5AF9, 0xA506.)
_KA_PAYLOAD = "".join("%02x" % i for i in range(56))
KA_ECHO_REQ = bytes.fromhex(
    "000c296a014d" "02aabbccddee" "0800"
    "4500" "0054" "1234" "4000" "40" "01" "a506" "c0a80114" "c0a8010a"
    "0800" "00eb" "0001" "0001" + _KA_PAYLOAD)
KA_ECHO_REPLY = bytes.fromhex(
    "02aabbccddee" "000c296a014d" "0800"
    "4500" "0054" "0000" "0000" "40" "01" "f73a" "c0a8010a" "c0a80114"
    "0000" "08eb" "0001" "0001" + _KA_PAYLOAD)

# ICMP message lengths (8 + payload) of the size cases: the smallest, odd and
# even tails round the 16-B pieces (message byte 14 is frame byte 48), 30 ends
# the frame on the 64-B boundary, then ping's default, an Ethernet MTU and a
# 9000-byte MTU, as payload and as message lengths
MSG_LENS = [8, 9, 23, 24, 25, 29, 30, 31, 56, 64, 1472, 1480, 8972, 8980]


def hand_cases():
    """(name, frame, caplen or None, cls, expected status, expected answer or
    None when the model's is taken)"""
    A, E, O = CLS_ARP, CLS_IPV4_OTHER, None
    pay = bytes(range(7, 63))
    rng = np.random.default_rng(8)
    out = [
        ("known answer: who-has", KA_ARP_REQ, O, A, ARP_REQ, KA_ARP_REPLY),
        ("known answer: ping", KA_ECHO_REQ, O, E, ECHO, KA_ECHO_REPLY),
        ("arp for another ip", arp(tip="192.168.1.11"), O, A, 0, O),
        ("arp opcode 2 to us", arp(op=2, tha=LOCAL_MAC), O, A, ARP_REPLY, O),
        ("arp opcode 3", arp(op=3), O, A, 0, O),
        ("arp plen 5", arp(plen=5), O, A, 0, O),
        ("a 41-byte arp", arp(pad=0)[:41], O, A, 0, O),
        ("a 42-byte arp", arp(pad=0), O, A, ARP_REQ, O),
        ("arp from a group address", arp(src=bytes.fromhex("0300deadbeef")), O, A, 0, O),
        ("arp for the second local address", arp(tip=LOCAL2_IP), O, A, ARP_REQ, O),
        ("an arp frame the classifier did not call arp", arp(), O, CLS_NON_IP, 0, O),
        ("echo reply (type 0)", echo(pay, typ=0), O, E, 0, O),
        ("timestamp (type 13)", echo(pay, typ=13), O, E, 0, O),
        ("code 1", echo(pay, code=1), O, E, 0, O),
        ("fragment: MF set", echo(pay, frag=0x2000), O, E, 0, O),
        ("fragment: offset 1", echo(pay, frag=0x0001), O, E, 0, O),
        ("DF set is no fragment", echo(pay, frag=0x4000), O, E, ECHO, O),
        ("reserved bit set is no fragment", echo(pay, frag=0x8000), O, E, ECHO, O),
        ("byte 14 = 0x46", echo(pay, ver_ihl=0x46), O, E, 0, O),
        ("tl 27", echo(b"", tl=27), O, E, 0, O),
        ("tl 28", echo(b""), O, E, ECHO, O),
        ("14 + tl = len + 1", echo(pay), 14 + 20 + 8 + 56 - 1, E, ECHO_BAD, O),
        ("tl says more than was sent", echo(pay, tl=20 + 8 + 57), O, E, ECHO_BAD, O),
        ("trailing bytes after 14 + tl", echo(pay, trail=b"\xee" * 13), O, E, ECHO, O),
        ("one flipped payload bit", _flip(echo(pay), 60, 0x10), O, E, ECHO_BAD, O),
        ("one flipped checksum bit", _flip(echo(pay), 36, 0x01), O, E, ECHO_BAD, O),
        ("answer checksum 0xFFFF", echo(bytes(24), ident=0, seq=0), O, E, ECHO, O),
        ("answer checksum 0x0000", echo(bytes(24), ident=0xFFFF, seq=0), O, E, ECHO, O),
        ("answer checksum 0x0000, odd tail", echo(bytes(22) + b"\xff", ident=0x00FF, seq=0), O, E,
         ECHO, O),
        ("echo to another ip", echo(pay, dst="192.168.1.11"), O, E, 0, O),
        ("echo from a group address", echo(pay, smac=bytes.fromhex("01005e000001")), O, E, 0, O),
        ("echo to the second local address", echo(pay, dst=LOCAL2_IP), O, E, ECHO, O),
        ("echo the classifier called udp", echo(pay), O, CLS_UDP, 0, O),
        ("udp to the local ip", F.udp_frame(PEER_IP, 4000, LOCAL_IP, 53, b"q" * 30), O, CLS_UDP, 0, O),
        ("tcp to the local ip", F.tcp_frame(PEER_IP, 4000, LOCAL_IP, 80, b"GET"), O, CLS_TCP, 0, O),
        ("udp the classifier called other", F.udp_frame(PEER_IP, 4000, LOCAL_IP, 53, b"q" * 30), O, E,
         0, O),
    ]
    for m in MSG_LENS:
        p = bytes(rng.integers(0, 256, m - 8, dtype=np.uint8))
        out.append(("message length %d" % m, echo(p, ident=m, seq=m ^ 0x55), O, E, ECHO, O))
    return out


def verdicts(cls_list):
    import rxgpu as R
    v = np.zeros(len(cls_list), R.VERDICT_DTYPE)
    v["cls"] = cls_list
    v["rc"] = [1 if c <= CLS_IPV4_OTHER else 0 for c in cls_list]
    v["flow_id"] = 0xFFFFFFFF
    return v


def fuzz_burst(seed, n, kind="mixed"):
    """n frames and their caplens.  kind: "none" (no candidate: UDP, TCP, ARP
    and echo for other addresses), "arp" (every frame a who-has for a local
    address), "echo" (every frame a good echo request, 8-1480-byte messages)
    or "mixed" (all of these, ARP replies, cut captures, bad checksums, other
    ICMP types, fragments, trailing bytes)"""
    rng = np.random.default_rng(seed)
    frames, caps = [], []
    for _ in range(n):
        src = "10.%d.%d.%d" % tuple(rng.integers(1, 250, 3))
        smac = bytes([2]) + bytes(rng.integers(0, 256, 5, dtype=np.uint8))
        lip = LOCALS[int(rng.integers(0, 2))][0]
        m = int(rng.choice([0, 1, 15, 16, 17, 22, 48, 56, 100, 600, 1472]))
        pay = bytes(rng.integers(0, 256, m, dtype=np.uint8))
        r = rng.random() if kind == "mixed" else \
            {"none": float(rng.choice([0.7, 0.8, 0.95])), "arp": 0.05, "echo": 0.3}[kind]
        cap = None
        if r < 0.15:
            f = arp(sip=src, tip=lip, sha=smac)
        elif r < 0.20:
            f = arp(op=2, sip=src, tip=lip, sha=smac)
        elif r < 0.50:
            f = echo(pay, src, lip, smac=smac, ident=int(rng.integers(0, 65536)),
                     seq=int(rng.integers(0, 65536)), trail=b"\xdd" * int(rng.integers(0, 3)))
        elif r < 0.56:
            f = _flip(echo(pay, src, lip, smac=smac), 34 + 2 + int(rng.integers(0, m + 6)), 0x20)
        elif r < 0.62:
            f = echo(pay, src, lip, smac=smac)
            cap = max(14, len(f) - int(rng.integers(1, 40)))
        elif r < 0.68:
            f = echo(pay, src, lip, smac=smac, typ=int(rng.choice([0, 3, 13])),
                     frag=int(rng.choice([0x4000, 0x2000, 0x00B9])))
        elif r < 0.76:
            f = [arp(sip=src, tip="172.16.0.9", sha=smac), echo(pay, src, "172.16.0.9", smac=smac)][
                int(rng.integers(0, 2))]
        elif r < 0.88:
            f = F.udp_frame(src, 4000, lip, int(rng.integers(1, 65535)), pay)
        else:
            f = F.tcp_frame(src, 4000, lip, 80, pay)
        frames.append(f)
        caps.append(len(f) if cap is None else cap)
    return frames, caps


# ---- the socket layer's scenarios (tests/test_rx_l2.py on the host-verdict path,
# tests/test_gpu_rx_l2.py on the device paths) ------------------------------------------
PEER2_IP, PEER2_MAC = "192.168.1.30", bytes.fromhex("02aabbccdd30")
Q_FRAMES = 1024


def who_has(k):
    """who-has LOCAL_IP from sender k"""
    return arp(sip="10.77.%d.%d" % (k >> 8, k & 255), sha=bytes([2, 0x77, 0, 0, k >> 8, k & 255]))


def scenario(ns, mode, on=True, encode=False):
    """what an observer of the stack sees: the frames of each tx_burst and the
    counters.  mode: a receive path of cookie_ref.Session"""
    import rxgpu as R
    from cookie_ref import Session
    s, log, dev = Session(ns, mode), {}, mode in ("gpu", "pipe")
    ns.set_local(LOCAL_IP, LOCAL_MAC)
    if on:
        ns.set_l2_respond(True)
    if encode:
        ns.set_tx_encode(True)
    fd = ns.socket(R.SOCK_DGRAM)
    assert ns.bind(fd, LOCAL_IP, 7000) == 0
    ns.arp_insert(PEER2_IP, PEER2_MAC)
    tx = lambda **kw: ns.tx_burst(cksum=dev, **kw)                     # noqa: E731
    # a who-has and a ping in one burst, a datagram already queued
    assert ns.sendto(fd, b"queued", PEER2_IP, 9) == 6
    s.rx([KA_ARP_REQ, F.udp_frame(PEER_IP, 5, LOCAL_IP, 7000, b"in"), KA_ECHO_REQ])
    log["first"] = tx()
    log["recv"] = ns.recvfrom(fd, 64)[1]
    # the request taught the peer's address, on or off: a datagram to it needs no ARP request
    assert ns.sendto(fd, b"to-peer", PEER_IP, 9) == 7
    log["learned"] = tx()
    # five who-has, two frame slots, then room for two 64-B slots only
    s.rx_two([who_has(k) for k in range(3)], [who_has(k) for k in range(3, 5)])
    log["two"] = tx(max_frames=2)
    log["room"] = tx(cap_bytes=128 + 63)
    log["rest"] = tx()
    # a bad checksum, a cut capture (the frame's last byte is not sent), an ARP reply to us
    s.rx([_flip(KA_ECHO_REQ, 70, 1), KA_ECHO_REQ[:-1], arp(op=2, tha=LOCAL_MAC)])
    log["bad"] = tx()
    log["stats"] = [ns.stat(k) for k in (21, 22, 23, 24)]
    # more requests than the queue holds
    s.rx([who_has(k) for k in range(Q_FRAMES + 76)])
    log["stats_full"] = [ns.stat(k) for k in (21, 22, 23, 24)]
    out = tx(max_frames=4096, cap_bytes=1 << 18)
    log["drained"] = (len(out), out[:1], out[-1:], tx())
    return log


def answer_of(frame, cls):
    return judge(frame, cls, [(F.ip4(LOCAL_IP), LOCAL_MAC)])[1]


def check_scenario(log, on=True):
    udp = lambda f, pay: len(f) == 42 + len(pay) and f[23] == 17 and f[42:] == pay   # noqa: E731
    ans = [KA_ARP_REPLY, KA_ECHO_REPLY] if on else []
    assert log["first"][:len(ans)] == ans
    assert len(log["first"]) == len(ans) + 1 and udp(log["first"][-1], b"queued")
    assert log["recv"][:2] == b"in"      # (the other traffic of the burst is delivered as ever)
    assert len(log["learned"]) == 1 and udp(log["learned"][0], b"to-peer")
    assert log["learned"][0][:6] == PEER_MAC
    want = [answer_of(who_has(k), CLS_ARP) for k in range(5)] if on else []
    assert log["two"] == want[:2] and log["room"] == want[2:4] and log["rest"] == want[4:]
    assert log["bad"] == []
    assert log["stats"] == ([6, 1, 0, 2] if on else [0, 0, 0, 0])
    assert log["stats_full"] == ([6 + Q_FRAMES, 1, 76, 2] if on else [0, 0, 0, 0])
    if on:
        assert log["drained"] == (Q_FRAMES, [answer_of(who_has(0), CLS_ARP)],
                                  [answer_of(who_has(Q_FRAMES - 1), CLS_ARP)], [])
    else:
        assert log["drained"] == (0, [], [], [])
