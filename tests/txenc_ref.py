"""Reference for the TX encoder (K5) tests — test infrastructure.

The three encoders restated in Python from the reference's lines, both
checksum fields 0:
  ng_encode_udp_apppkt  udp.c:59-98      ng_encode_tcp_apppkt  tcp.c:420-466
  ng_encode_arp_pkt     common.c:206-241
The oracle's tx_cksum (oracle/ref_cpu.c) then fills the checksums; frames are
laid out by the rules of rxg_tx_encode_dev (include/rxgpu.h), zero-filled to
64 B.  Shared by test_tx_encode.py (CPU) and test_gpu_tx_encode.py."""
import struct

import numpy as np

import oracle_bind as O
import rxgpu as R

LMAC, PMAC = bytes.fromhex("000c296a014d"), bytes.fromhex("02aabbccddee")
L_IP, P_IP = "192.168.100.77", "10.0.0.1"
CANARY = 0xA5

UDP_LENS = [0, 1, 5, 6, 7, 15, 16, 17, 21, 22, 23, 1458, 1472, 8958, 65493]
TCP_OPTLENS = [0, 1, 3, 10]
TCP_LENS = [0, 1, 9, 10, 11, 1446]


def _raw4(x):
    return int(x).to_bytes(4, "little")


def _raw2(x):
    return int(x).to_bytes(2, "little")


def frame_len(d):
    """frame length of a descriptor, 0 = skipped (unknown kind, > 65535)"""
    k = int(d["kind"])
    fl = {R.TXD_UDP: 42 + int(d["pay_len"]), R.TXD_TCP: 54 + 4 * int(d["optlen"]) + int(d["pay_len"]),
          R.TXD_ARP: 42}.get(k, 0)
    return fl if fl <= 65535 else 0


def ref_frame(d, payload: bytes) -> bytes:
    """the frame of descriptor d (a TXD_DTYPE record), checksum fields 0"""
    dm, sm = bytes(d["dst_mac"]), bytes(d["src_mac"])
    sip, dip = _raw4(d["sip"]), _raw4(d["dip"])
    kind = int(d["kind"])
    if kind == R.TXD_ARP:  # common.c:206-241; all-ones target -> zero Ethernet destination (:216-223)
        return ((bytes(6) if dm == b"\xff" * 6 else dm) + sm + b"\x08\x06" +
                struct.pack(">HHBBH", 1, 0x0800, 6, 4, 1) + sm + sip + dm + dip)
    proto = 17 if kind == R.TXD_UDP else 6
    if kind == R.TXD_UDP:  # udp.c:86-95: dgram_len = 8 + payload
        l4 = _raw2(d["sport"]) + _raw2(d["dport"]) + struct.pack(">HH", 8 + len(payload), 0)
    else:  # tcp.c:446-463: seq/ack htonl, window and urp as stored, options zero
        l4 = (_raw2(d["sport"]) + _raw2(d["dport"]) + struct.pack(">II", int(d["seq"]), int(d["ack"])) +
              bytes([int(d["hdrlen_off"]), int(d["tcp_flags"])]) + _raw2(d["window"]) + bytes(2) +
              _raw2(d["urp"]) + bytes(4 * int(d["optlen"])))
    tl = 20 + len(l4) + len(payload)
    ip = struct.pack(">BBHHHBBH", 0x45, 0, tl, 0, 0, 64, proto, 0) + sip + dip  # id 0, frag 0, ttl 64
    return dm + sm + b"\x08\x00" + ip + l4 + payload


def txd(kind, pay_len=0, **kw):
    d = np.zeros(1, R.TXD_DTYPE)[0]
    d["kind"], d["pay_len"] = kind, pay_len
    d["dst_mac"] = np.frombuffer(kw.pop("dst_mac", PMAC), np.uint8)
    d["src_mac"] = np.frombuffer(kw.pop("src_mac", LMAC), np.uint8)
    d["sip"], d["dip"] = R.ip_raw(kw.pop("sip", L_IP)), R.ip_raw(kw.pop("dip", P_IP))
    d["sport"], d["dport"] = R.port_raw(kw.pop("sport", 8889)), R.port_raw(kw.pop("dport", 5555))
    d["hdrlen_off"] = kw.pop("hdrlen_off", 0x50 if kind == R.TXD_TCP else 0)
    for k, v in kw.items():
        d[k] = v
    return d


def burst(descs, rng=None, payloads=None):
    """(txd array, payload buffer): every payload at the next 16-B aligned
    offset, random bytes (or the given ones); the buffer ends with the last
    payload's last byte (the host encoder reads no further)"""
    rng = rng or np.random.default_rng(1)
    t = np.array(descs, R.TXD_DTYPE)
    parts, pos = [], 0
    for i in range(len(t)):
        n = int(t[i]["pay_len"]) if int(t[i]["kind"]) != R.TXD_ARP else 0
        if payloads is not None and payloads[i] is not None:
            p = np.frombuffer(payloads[i], np.uint8)
            assert len(p) == n
        else:
            p = rng.integers(0, 256, n, np.uint8)
        t[i]["pay_off16"] = pos // 16
        pad = (-n) % 16
        parts += [p, np.zeros(pad, np.uint8)]
        pos += n + pad
    buf = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    last = max((int(x["pay_off16"]) * 16 + int(x["pay_len"]) for x in t
                if int(x["kind"]) != R.TXD_ARP and frame_len(x)), default=0)
    return t, np.ascontiguousarray(buf[:last])


def reference(t, payload, cap_bytes, slot_bytes=0, flags=0, fill=CANARY):
    """(pkts, off, len, span, totals) by include/rxgpu.h's rules"""
    n = len(t)
    pk = np.full(cap_bytes, fill, np.uint8)
    off, ln = np.zeros(n, np.uint32), np.zeros(n, np.uint16)
    pos = end = written = skipped = 0
    full = False
    for k in range(n):
        d = t[k]
        fl = frame_len(d)
        if slot_bytes and fl > slot_bytes:
            fl = 0
        room = slot_bytes or (fl + 63) // 64 * 64
        at = k * slot_bytes if slot_bytes else pos
        ok = fl != 0
        if ok and at + room > cap_bytes:
            ok = False
            full = full or not slot_bytes
        if ok and full:
            ok = False
        if not ok:
            skipped += 1
            continue
        o = int(d["pay_off16"]) * 16
        pl = 0 if int(d["kind"]) == R.TXD_ARP else int(d["pay_len"])
        f = ref_frame(d, payload[o:o + pl].tobytes())
        assert len(f) == fl
        nb = (fl + 63) // 64 * 64
        pk[at:at + fl] = np.frombuffer(f, np.uint8)
        pk[at + fl:at + nb] = 0
        off[k], ln[k] = at // 64, fl
        end = at + nb
        if not slot_bytes:
            pos = end
        written += 1
    if not flags & R.TXE_NO_CKSUM and end:
        live = ln > 0
        pk[:end] = O.tx_cksum(pk[:end], off[live], ln[live], 6)
    tot = np.array([written, end & 0xFFFFFFFF, end >> 32, skipped], np.uint32)
    return pk, off, ln, end, tot


def boundary_descs():
    """the boundary set: UDP lengths (22 fills 64 B exactly, 23 crosses), TCP
    option words x payloads, ARP with an ordinary and the all-ones target"""
    ds = [txd(R.TXD_UDP, n, sport=1000 + i) for i, n in enumerate(UDP_LENS)]
    ds += [txd(R.TXD_TCP, n, optlen=o, seq=0x01020304 + n, ack=0xA0B0C0D0 + o, tcp_flags=0x18,
               window=14600, urp=o, hdrlen_off=0x50 + (o << 4 & 0xF0))
           for o in TCP_OPTLENS for n in TCP_LENS]
    ds += [txd(R.TXD_ARP, dst_mac=PMAC), txd(R.TXD_ARP, 77, dst_mac=b"\xff" * 6)]
    return ds


def mix_descs(n=3000, seed=11):
    rng = np.random.default_rng(seed)
    ds = []
    for i in range(n):
        r = rng.random()
        ln = int(rng.choice([0, 3, 18, 22, 23, 64, 100, 300, 512, 1400, 1472]) if rng.random() < 0.7
                 else rng.integers(0, 1473))
        if rng.random() < 0.01:
            ln = int(rng.integers(1473, 9000))
        common = dict(sip=L_IP, dip=f"10.{i >> 16 & 255}.{i >> 8 & 255}.{i & 255}",
                      sport=int(rng.integers(1, 65536)), dport=int(rng.integers(1, 65536)))
        if r < 0.5:
            ds.append(txd(R.TXD_UDP, ln, **common))
        elif r < 0.95:
            ds.append(txd(R.TXD_TCP, min(ln, 1446), optlen=int(rng.choice([0, 0, 0, 1, 3, 10])),
                          seq=int(rng.integers(0, 2**32)), ack=int(rng.integers(0, 2**32)),
                          tcp_flags=int(rng.choice([0x10, 0x18, 0x12, 0x11])),
                          window=int(rng.integers(0, 65536)), urp=int(rng.integers(0, 3)), **common))
        else:
            ds.append(txd(R.TXD_ARP, int(rng.integers(0, 99)), sip=L_IP, dip=common["dip"],
                          dst_mac=b"\xff" * 6 if rng.random() < 0.5 else PMAC))
    return ds


def skip_descs():
    """unknown kind, a UDP payload one byte too long, then ordinary frames"""
    return [txd(R.TXD_UDP, 30), txd(7, 10), txd(R.TXD_UDP, 65494), txd(R.TXD_TCP, 200),
            txd(R.TXD_UDP, 100), txd(R.TXD_ARP), txd(R.TXD_UDP, 1000)]
