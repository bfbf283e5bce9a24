#!/usr/bin/env python3
"""Writes the reference-derived fixtures of tests/golden/ (see
ref_golden_readme.txt).  Every EXPECTED value in them was written by the
reference's own compiled code, run through oracle/_ref/refrun
(oracle/refrun_main.c, tests/ref_bind.py); the inputs are our own frames.
Seeded and deterministic: a second run gives byte-identical files.

  ref_rx.pcap + ref_rx_flows.npz + ref_rx_expect.npy   `rx` cases
  ref_cksum.npz                                        `cksum` cases
  ref_tx.npz                                           `tx` cases

Needs refrun (built by `make -C oracle` where the reference is present).
Run from the repo root:  python tests/golden/make_ref_golden.py [OUTDIR]
"""
from __future__ import annotations

import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)),
                                "dpdk-tcp-udp_protocol_stack_amd"))
sys.path.insert(0, HERE)

import frames as F  # noqa: E402
import make_golden as G  # noqa: E402

L, L2 = "192.168.100.77", "10.9.9.9"
RECV_DELTA = 3  # nrecvfrom buffers: length - 3, length, length + 3
MAX_FILE = 512 * 1024


# ---- frames with a chosen checksum ---------------------------------------
def l4_with_value(ip_hdr: bytes, l4: bytearray, proto: int, at: int, target: int) -> None:
    """set the 16-bit word at even offset `at` of l4 so that the value
    rte_ipv4_udptcp_cksum computes BEFORE the UDP 0 -> 0xFFFF rule is `target`
    (the checksum field must already be 0).  0xFFFF is not reachable: the
    folded sum of a pseudo-header with a non-zero protocol is never 0."""
    assert at % 2 == 0 and target != 0xFFFF
    l4[at:at + 2] = b"\0\0"
    psd = ip_hdr[12:20] + bytes([0, proto]) + struct.pack(">H", len(l4))
    s0 = F.fold_cksum(psd + bytes(l4))
    want = (~target) & 0xFFFF
    l4[at:at + 2] = struct.pack("<H", (want - s0) % 0xFFFF)
    assert F.fold_cksum(psd + bytes(l4)) == want


def tcp_frame_with_value(target: int, stored: int, payload=b"sixteen byte pay") -> bytes:
    f = bytearray(F.tcp_frame("10.0.0.9", 40000, L, 9999, payload))
    l4 = bytearray(f[34:])
    l4[16:18] = b"\0\0"
    l4_with_value(bytes(f[14:34]), l4, 6, 20, target)
    l4[16:18] = struct.pack("<H", stored)
    return bytes(f[:34]) + bytes(l4)


def udp_frame_with_value(target: int, stored: int, dport=8889, payload=b"q" * 20 + b"\0\0") -> bytes:
    f = bytearray(F.udp_frame("10.1.2.3", 7, L, dport, payload))
    l4 = bytearray(f[34:])
    l4[6:8] = b"\0\0"
    l4_with_value(bytes(f[14:34]), l4, 17, len(l4) - 2, target)
    l4[6:8] = struct.pack("<H", stored)
    return bytes(f[:34]) + bytes(l4)


def sized(n: int, proto: int, rng, dport=None) -> bytes:
    """a valid frame of exactly n bytes (n >= 42 UDP, >= 54 TCP) to a known flow"""
    if proto == 17:
        return F.udp_frame("10.0.0.1", 5555, L, dport or 8889,
                           bytes(rng.integers(0, 256, n - 42, np.uint8)))
    return F.tcp_frame("10.0.0.9", 40000, L, dport or 9999,
                       bytes(rng.integers(0, 256, n - 54, np.uint8)))


# ---- flow tables -----------------------------------------------------------
def rx_flows():
    import rxgpu as R
    eu, et = G.edge_flows()
    ip, port = R.ip_raw, R.port_raw
    udp = [tuple(x) for x in eu.tolist()]
    udp += [(ip(L), port(30000 + 3 * k), 17, 0) for k in range(40)]
    udp += [(ip(L2), port(30021), 17, 0), (0, 0, 17, 0), (0, port(53), 17, 0), (ip(L), 0, 17, 0),
            (ip(L), port(30003), 17, 0)]                      # a newer duplicate of 30003
    tcb = [tuple(x) for x in et.tolist()]
    tcb += [(ip("10.0.0.11"), ip(L), port(40002), port(9999), 0),  # CLOSED beside the listener
            (ip("10.0.0.9"), ip(L), port(40000), port(9999), 4),   # duplicate exact key: newest wins
            (0, 0, 0, 0, 1),                                       # listener on port 0, address 0
            (0, ip(L), 0, port(8080), 1),
            (ip("10.0.0.12"), ip(L), port(40003), port(8080), 4),  # exact tcb on a listener's port
            (ip("10.0.0.12"), ip(L), port(40003), port(8081), 2)]
    return np.array(udp, R.UDP_SOCK_DTYPE), np.array(tcb, R.TCB_DTYPE)


# ---- the rx corpus ---------------------------------------------------------
def deliberate_frames():
    fr = []

    def add(f, cap=None):
        fr.append((f, len(f) if cap is None else cap))

    # a TCP segment whose computed checksum is 0x0000: stored 0xFFFF (its
    # one's-complement equal) is rejected, stored 0x0000 passes
    add(tcp_frame_with_value(0x0000, 0xFFFF))
    add(tcp_frame_with_value(0x0000, 0x0000))
    add(tcp_frame_with_value(0x0001, 0x0001))
    add(tcp_frame_with_value(0xFFFE, 0xFFFE))
    # a UDP checksum computing to 0 (goes out, and is recomputed, as 0xFFFF)
    add(udp_frame_with_value(0x0000, 0xFFFF))
    add(udp_frame_with_value(0x0000, 0x0000))
    add(udp_frame_with_value(0x0001, 0x0001))
    for dl in list(range(0, 10)) + [64, 200, 1473, 65535]:        # dgram_len 0-9, > frame
        add(F.udp_frame("10.0.0.1", 5555, L, 8889, b"abcdefgh", dgram_len=dl))
        add(F.udp_frame("10.0.0.1", 5555, L, 1111, b"abcdefgh", dgram_len=dl))  # no socket
    for tl in (0, 5, 19, 20, 21, 27, 28, 29, 300, 1500, 9000, 65535):  # tl < 20, > capture
        add(F.udp_frame("10.0.0.1", 5555, L, 8889, b"x" * 30, tl=tl))
        add(F.tcp_frame("10.0.0.9", 40000, L, 9999, b"y" * 30, tl=tl, tl_cksum=True))
        add(F.tcp_frame("10.0.0.9", 40000, L, 9999, b"y" * 30, tl=tl))
    for doff in (0x00, 0x40, 0x60, 0xF0):                             # data offset, no options
        add(F.tcp_frame("10.0.0.9", 40000, L, 9999, b"opt?", data_off=doff, pad_options=False))
    add(F.tcp_frame("10.0.0.9", 40000, L, 9999, b"o" * 44, data_off=0xF0))
    add(F.udp_frame("10.0.0.1", 5555, "0.0.0.0", 0, b"to address 0 port 0"))
    add(F.udp_frame("10.0.0.1", 5555, "0.0.0.0", 53, b"address 0"))
    add(F.udp_frame("10.0.0.1", 5555, L, 0, b"port 0"))
    add(F.udp_frame("10.0.0.1", 5555, L, 20002, b"socket of protocol 6"))
    add(F.tcp_frame("10.0.0.77", 1, "7.7.7.7", 0, b"listener on port 0"))
    add(F.tcp_frame("10.0.0.77", 1, L, 9999, b"syn", flags=0x02))     # SYN to a listener
    add(F.tcp_frame("10.0.0.11", 40002, L, 9999, b"closed tcb"))
    add(F.tcp_frame("10.0.0.12", 40003, L, 8080, b"exact beside listener"))
    add(F.tcp_frame("10.0.0.13", 40003, L, 8080, b"listener"))
    add(F.tcp_frame("10.0.0.12", 40003, L, 8081, b"syn_rcvd tcb"))
    add(F.tcp_frame("10.0.0.13", 40003, L, 8081, b"no listener"))
    add(F.ether(bytes(46), ethertype=0x0008))                         # byte-swapped ethertype
    add(F.ether(bytes(46), ethertype=0x86DD))
    return fr


def ladder_frames(rng):
    """capture lengths 34-130, the 16*G*P +-1 sizes, 590, 1500, 1514 and a
    dozen of 9014"""
    fr = []
    for n in range(34, 131):
        proto = 17 if n % 2 else 6
        least = 42 if proto == 17 else 54
        if n >= least:
            fr.append((sized(n, proto, rng, 30000 + 3 * (n % 40) if proto == 17 else None), n))
        else:
            fr.append((sized(64, proto, rng), n))                   # cut inside the headers
    for n in (63, 64, 65, 127, 128, 129, 1535, 1536, 1537, 2047, 2048, 2049, 590, 1500, 1514):
        fr.append((sized(n, 6 if n != 590 else 17, rng), n))
    big = [sized(9014, 6, rng) for _ in range(6)] + [sized(9014, 17, rng) for _ in range(2)]
    big.append(F.tcp_frame("10.0.0.9", 40000, L, 9999, bytes(rng.integers(0, 256, 8960, np.uint8)),
                           corrupt=True))
    big.append(F.tcp_frame("10.0.0.9", 40000, L, 9999, b"\xff" * 8960))   # maximum carries
    big.append(F.udp_frame("10.0.0.1", 5555, L, 8889, b"\xff" * 8972, dgram_len=9))
    big.append(F.tcp_frame("10.0.0.10", 40001, L, 9999, bytes(8960)))
    assert all(len(f) == 9014 for f in big)
    fr += [(f, 9014) for f in big]
    fr.append((big[0], 9000))                                        # a jumbo cut short
    return fr


def _udp_zero_sum_frame(src, sport, dst, dport):
    f = udp_frame_with_value(0x0000, 0xFFFF, dport)
    assert len(f) == 64
    return f


def spoiler_frames(rng, waves_of=8):
    """the spoilers of test_gpu_parity.test_lane_fast_path_waves, each among
    clean 64-B frames to the port window, capture cut to 64; plus a runt"""
    def clean():
        port = 30000 + int(rng.integers(0, 130))
        return F.udp_frame("10.1.2.3", int(rng.integers(1024, 65535)), L, port,
                           bytes(rng.integers(0, 256, 22, dtype=np.uint8)))
    spoil = [
        lambda: F.tcp_frame("10.1.2.3", 4000, L, 30003, b"t" * 10),
        lambda: F.arp_frame("10.1.2.3", L),
        lambda: F.icmp_frame("10.1.2.3", L),
        lambda: F.ether(bytes(50), ethertype=0x86DD),
        lambda: F.udp_frame("10.1.2.3", 5, L, 30003, b"s" * 22, tl=40),
        lambda: F.udp_frame("10.1.2.3", 5, L, 30003, b"s" * 22, tl=18),
        lambda: F.udp_frame("10.1.2.3", 5, L, 30003, b"s" * 22, dgram_len=8),
        lambda: F.udp_frame("10.1.2.3", 5, L, 30003, b"s" * 22, dgram_len=3),
        lambda: F.udp_frame("10.1.2.3", 5, L, 30006, b"s" * 22, corrupt=True),
        lambda: _udp_zero_sum_frame("10.1.2.3", 7, L, 30009),
        lambda: F.udp_frame("10.1.2.3", 5, L2, 30021, b"s" * 22),
        lambda: F.udp_frame("10.1.2.3", 5, "10.77.0.1", 30003, b"s" * 22),
        lambda: F.udp_frame("10.1.2.3", 5, L, 29000, b"s" * 22),
    ]
    fr = []
    for k in range(len(spoil) + 1):
        wave = [(clean(), 64) for _ in range(waves_of)]
        lane = int(rng.integers(0, waves_of))
        if k < len(spoil):
            f = spoil[k]()
            wave[lane] = (f, min(len(f), 64))
        else:
            wave[lane] = (wave[lane][0], 48)
        fr += wave
    return [((f + bytes(max(0, 64 - len(f))))[:64], c) for f, c in fr]


def fuzz_frames(n, seed=7, tl_max=1600, small=False):
    """the mutation fuzz of test_gpu_parity.test_fuzzed_frames_match_oracle
    (same recipe and seed; `small` swaps in shorter base frames so that a
    committed corpus stays small)"""
    rng = np.random.default_rng(seed)
    big1, big2 = (60, 90) if small else (300, 1200)
    base = [F.udp_frame("10.0.0.1", 5555, L, 8889, bytes(rng.integers(0, 256, 40, np.uint8))),
            F.tcp_frame("10.0.0.9", 40000, L, 9999, bytes(rng.integers(0, 256, big1, np.uint8))),
            F.tcp_frame("0.0.0.0", 0, L, 9999, b"x" * 17),
            F.udp_frame("10.0.0.1", 5555, L, 20001, b"y" * big2),
            F.arp_frame("1.2.3.4", L), F.icmp_frame("1.2.3.4", L)]
    out = []
    for _ in range(n):
        f = bytearray(base[rng.integers(len(base))])
        for _ in range(rng.integers(0, 4)):
            pos = int(rng.integers(0, min(len(f), 60)))
            f[pos] = int(rng.integers(0, 256))
        if rng.random() < 0.3:
            f[16:18] = int(rng.integers(0, tl_max)).to_bytes(2, "big")
        if rng.random() < 0.2:
            f[23] = int(rng.choice([6, 17]))
        out.append((bytes(f), len(f) if rng.random() < 0.8 else int(rng.integers(0, len(f) + 1))))
    return out


def rx_corpus():
    """[(frame, caplen)] of the committed corpus and its (udp, tcb) tables"""
    rng = np.random.default_rng(0x5EED)
    ef, ec = G.edge_frames()
    fr = list(zip(ef, ec)) + deliberate_frames() + ladder_frames(rng) + spoiler_frames(rng)
    fr += fuzz_frames(1400, small=True)
    udp, tcb = rx_flows()
    return fr, udp, tcb


# ---- the checksum corpus ---------------------------------------------------
CK_LENGTHS = list(range(0, 131)) + [16 * k + d for k in range(8, 130) for d in (-1, 0, 1)] + \
    [8986, 9000, 65515]


def ck_buffer(rng, n, kind, proto, ihl=5, tl=None):
    """an IPv4 header + n L4 bytes; kind: random / zeros / ones / a target
    value computed before the UDP rule (an int)"""
    tl = 20 + n if tl is None else tl
    hdr = bytearray(rng.integers(0, 256, 20, np.uint8).tobytes())
    hdr[0] = 0x40 | ihl
    hdr[2:4] = struct.pack(">H", tl & 0xFFFF)
    hdr[9] = proto
    if kind == "zeros":
        l4 = bytearray(n)
    elif kind == "ones":
        l4 = bytearray(b"\xff" * n)
    else:
        l4 = bytearray(rng.integers(0, 256, n, np.uint8).tobytes())
        if isinstance(kind, int) and n >= 2 and tl == 20 + n:
            l4_with_value(bytes(hdr), l4, proto, (n - 2) & ~1 if n % 2 == 0 else 0, kind)
    return bytes(hdr) + bytes(l4)


def cksum_cases(reps=1, lengths=CK_LENGTHS, seed=11, extra_random=0):
    """[(buffer, align)]: every length x {random, zeros, ones, values 0x0000 /
    0x0001 / 0xFFFE for each of protocol 6 and 17} x odd and even start; tl in
    {0, 19, 20, 21, 65535} x IHL nibbles 5-15; raw buffers with no header"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        for _ in range(reps if n < 8000 else 1):
            for align in (0, 1):
                for kind in ("random", "zeros", "ones"):
                    out.append((ck_buffer(rng, n, kind, int(rng.choice([6, 17])),
                                          int(rng.integers(5, 16))), align))
                for proto in (6, 17):
                    for target in (0x0000, 0x0001, 0xFFFE):
                        out.append((ck_buffer(rng, n, target, proto), align))
                out.append((rng.integers(0, 256, n, np.uint8).tobytes(), align))  # raw bytes only
    for tl in (0, 19, 20, 21, 65535):
        for ihl in range(5, 16):
            for proto in (6, 17):
                for align in (0, 1):
                    for kind in ("random", "ones"):
                        out.append((ck_buffer(rng, 64, kind, proto, ihl, tl), align))
    hdr = bytearray(20)                         # rte_ipv4_cksum: a header summing to 0xFFFF, and 0
    hdr[0:2] = b"\xff\xff"
    out += [(bytes(hdr), 0), (bytes(20), 0), (b"\xff" * 20, 1)]
    for _ in range(extra_random):
        n = int(rng.integers(0, 2100))
        out.append((ck_buffer(rng, n, "random", int(rng.choice([6, 17, 1])),
                              int(rng.integers(5, 16))), int(rng.integers(0, 2))))
    return out


# ---- the tx corpus -----------------------------------------------------------
def zero_tx_fields(f: bytes, cap: int) -> bytes:
    z = bytearray(f)
    if cap >= 34 and z[12] == 8 and z[13] == 0:
        z[24:26] = b"\0\0"
        hole = {17: 40, 6: 50}.get(z[23])
        if hole is not None and cap >= hole + 2:
            z[hole:hole + 2] = b"\0\0"
    return bytes(z)


def ffff_header_udp(payload=b"abc"):
    """(sip, dip, sport, dport, frame): a UDP frame as the reference's encoder
    lays it out (id and fragment 0, ttl 64) whose IPv4 header sums to 0xFFFF,
    found by a search over the low half of the raw destination address"""
    sip, dip, sport, dport = "192.168.100.77", "10.0.0.1", 8889, 5555
    udp = struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload
    hdr = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, 0, 20 + len(udp), 0, 0, 64, 17, 0,
                                F.ip4(sip), F.ip4(dip)))
    for low in range(65536):
        hdr[16:18] = low.to_bytes(2, "little")
        if F.fold_cksum(bytes(hdr)) == 0xFFFF:
            break
    assert F.fold_cksum(bytes(hdr)) == 0xFFFF
    dip = ".".join(str(b) for b in hdr[16:20])
    return sip, dip, sport, dport, F.ether(bytes(hdr) + udp, dst=F.PEER_MAC, src=F.LOCAL_MAC)


def tx_corpus():
    """[(frame with zeroed fields, caplen)]: the fuzz recipe of tests/test_tx.py
    on shorter bases, the size ladder and jumbo frames"""
    rng = np.random.default_rng(3)
    base = [F.udp_frame(L, 8889, "10.0.0.1", 5555, bytes(rng.integers(0, 256, 40, np.uint8))),
            F.tcp_frame(L, 9999, "10.0.0.9", 40000, bytes(rng.integers(0, 256, 90, np.uint8))),
            F.tcp_frame(L, 9999, "10.0.0.9", 40000, b"y" * 17), F.arp_frame("1.2.3.4", L),
            F.icmp_frame(L, "1.2.3.4"), F.udp_frame(L, 1, "10.0.0.1", 2, b"z" * 300)]
    fr = []
    for _ in range(260):
        f = bytearray(base[rng.integers(len(base))])
        for _ in range(rng.integers(0, 3)):
            pos = int(rng.integers(0, min(len(f), 60)))
            f[pos] = int(rng.integers(0, 256))
        if rng.random() < 0.3:
            f[16:18] = int(rng.integers(0, 9100)).to_bytes(2, "big")
        fr.append((bytes(f), len(f) if rng.random() < 0.85 else int(rng.integers(0, len(f) + 1))))
    for n in list(range(54, 131, 3)) + [63, 64, 65, 127, 128, 129, 1535, 1536, 1537, 2047, 2048,
                                        2049, 590, 1500, 1514, 9014, 9014, 9014]:
        fr.append((sized(n, 6 if n % 2 == 0 else 17, rng), n))
    fr.append((F.tcp_frame(L, 9999, "10.0.0.9", 40000, b"\xff" * 8960), 9014))
    fr.append((udp_frame_with_value(0x0000, 0), 64))
    fr.append((tcp_frame_with_value(0x0000, 0), 70))
    fr.append((ffff_header_udp()[4], 45))  # the LAST frame: a header summing to 0xFFFF
    return [(zero_tx_fields(f, c), c) for f, c in fr]


# ---- writing -------------------------------------------------------------------
def _savez(path, **arrays):
    """np.savez_compressed with fixed member times, so that equal contents
    give equal bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in arrays:
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), b.getvalue(),
                       zipfile.ZIP_DEFLATED)


def _ragged(bufs):
    start = np.zeros(len(bufs) + 1, np.uint32)
    start[1:] = np.cumsum([len(b) for b in bufs])
    return np.frombuffer(b"".join(bufs), np.uint8), start


def main(out=HERE):
    import ref_bind as RB
    import ref_check as RC

    fr, udp, tcb = rx_corpus()
    frames, caps = [f for f, _ in fr], [c for _, c in fr]
    F.write_pcap(os.path.join(out, "ref_rx.pcap"), frames, caps)
    _savez(os.path.join(out, "ref_rx_flows.npz"), udp=udp, tcb=tcb)
    s = RB.Session()
    s.tables(udp, tcb)
    for f in F.read_pcap(os.path.join(out, "ref_rx.pcap")):
        s.rx(f, recv=True, delta=RECV_DELTA)
    exp = RC.records(s.run())
    np.save(os.path.join(out, "ref_rx_expect.npy"), exp)

    # every short length in full; of the long ones every seventh buffer (7 is
    # coprime to the 20 buffers per length, so each kind and start still occurs)
    ck = cksum_cases(lengths=list(range(0, 131)))
    ck += cksum_cases(lengths=[255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8986, 9000],
                      seed=12)[::7]
    s = RB.Session()
    for b, a in ck:
        s.cksum(b, a)
    ans = np.array(s.run(), np.uint16)
    data, start = _ragged([b for b, _ in ck])
    _savez(os.path.join(out, "ref_cksum.npz"), data=data, start=start,
           align=np.array([a for _, a in ck], np.uint8), raw=ans[:, 0], udptcp=ans[:, 1],
           ipv4=ans[:, 2])

    tx = tx_corpus()
    s = RB.Session()
    for f, c in tx:
        s.tx(f[:c])
    res = np.array(s.run(), np.uint16)
    buf, off, lens = F.pack_frames([f for f, _ in tx], 4, caplens=[c for _, c in tx])
    _savez(os.path.join(out, "ref_tx.npz"), pkts=buf, off=off, len=lens, ipck=res[:, 0],
           l4ck=res[:, 1], has_ip=res[:, 2].astype(np.uint8), has_l4=res[:, 3].astype(np.uint8))

    names = ["ref_rx.pcap", "ref_rx_flows.npz", "ref_rx_expect.npy", "ref_cksum.npz", "ref_tx.npz"]
    for n in names:
        size = os.path.getsize(os.path.join(out, n))
        assert size < MAX_FILE, (n, size)
        print(f"{n}: {size} bytes")
    print(f"{len(frames)} rx frames, {len(ck)} checksum buffers, {len(tx)} tx frames")
    return names


if __name__ == "__main__":
    main(*sys.argv[1:2])
