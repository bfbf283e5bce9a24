"""Model of the TX encoder with both cuts (rxg_tx_encode_frag_*, include/rxgpu.h)
— test infrastructure, pure Python / numpy, no code shared with the C side.

A descriptor's whole frame comes from txenc_ref.ref_frame; both checksums are
RFC 1071 arithmetic written here (the oracle's tx_cksum cannot take a frame
over 65535 bytes, and a cut datagram's whole frame may be 65549).  A UDP
datagram that does not fit the MTU is sliced into fragments by RFC 791; TCP
descriptors are cut at the MSS as test_tx_tso.split does; the layout follows
the header's rules (entries, capacity, canary) as test_tx_tso.reference does.
reassemble() rebuilds a datagram from its fragments in any order."""
import struct

import numpy as np

import rxgpu as R
import txenc_ref as T

ONES32, ONES16 = 0xFFFFFFFF, 0xFFFF
MTUS = (68, 70, 76, 1500, 9000)
MSS_OF = {68: 20, 70: 0, 76: 20, 1500: 1460, 9000: 0}  # the TCP cut that goes with each MTU


def csum16(b: bytes) -> int:
    """RFC 1071: the one's-complement sum of b's big-endian 16-bit words, folded"""
    if len(b) & 1:
        b += b"\0"
    s = int(np.frombuffer(b, ">u2").astype(np.uint64).sum())
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def fill(frame: bytes) -> bytes:
    """an IPv4 UDP / TCP frame with both checksums filled: the IPv4 header's is
    the plain complement, UDP's 0 becomes 0xFFFF"""
    f = bytearray(frame)
    proto, l4 = f[23], bytes(f[34:])
    f[24:26] = struct.pack(">H", ~csum16(bytes(f[14:34])) & 0xFFFF)
    k = ~csum16(bytes(f[26:34]) + struct.pack(">BBH", 0, proto, len(l4)) + l4) & 0xFFFF
    if k == 0 and proto == 17:
        k = 0xFFFF
    at = 40 if proto == 17 else 50
    f[at:at + 2] = struct.pack(">H", k)
    return bytes(f)


def fp_of(mtu):
    return (mtu - 20) & ~7


def is_cut(d, mtu):
    return int(d["kind"]) == R.TXD_UDP and mtu != 0 and 28 + int(d["pay_len"]) > mtu


def frames_of(d, payload, mss, mtu, slot=0, flags=0):
    """the frames of descriptor d in entry order; [] = skipped (s == 0)"""
    kind, pay = int(d["kind"]), int(d["pay_len"])
    o = int(d["pay_off16"]) * 16
    ck = not flags & R.TXE_NO_CKSUM
    if is_cut(d, mtu):
        L, fp = 8 + pay, fp_of(mtu)
        if 20 + L > 65535 or 34 + min(fp, L) > 65535 or (slot and 34 + min(fp, L) > slot):
            return []
        whole = T.ref_frame(d, payload[o:o + pay].tobytes())
        if ck:
            whole = fill(whole)
        dgram = whole[34:]
        assert len(dgram) == L
        out, s = [], -(-L // fp)
        for j in range(s):
            part = dgram[j * fp:(j + 1) * fp]
            ip = bytearray(struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(part), int(d["seq"]) & 0xFFFF,
                                       (j * fp // 8) | (0x2000 if j < s - 1 else 0), 64, 17, 0) +
                           whole[26:34])
            if ck:
                ip[10:12] = struct.pack(">H", ~csum16(bytes(ip)) & 0xFFFF)
            out.append(whole[:14] + bytes(ip) + part)
        return out
    if kind == R.TXD_TCP:
        hdr = 54 + 4 * int(d["optlen"])
        s = max(1, -(-pay // mss)) if mss else 1
        segs = [min(mss, pay - j * mss) for j in range(s)] if mss else [pay]
    elif kind in (R.TXD_UDP, R.TXD_ARP):
        hdr, s, segs = 42, 1, [0 if kind == R.TXD_ARP else pay]
    else:
        return []
    if hdr + segs[0] > 65535 or (slot and hdr + segs[0] > slot):
        return []
    out = []
    for j, n in enumerate(segs):
        g = d.copy()
        if s > 1:
            g["seq"] = (int(d["seq"]) + j * mss) & ONES32
            g["pay_len"] = n
            if j != s - 1:
                g["tcp_flags"] = int(d["tcp_flags"]) & ~0x09
        at = o + (j * mss if s > 1 else 0)
        f = T.ref_frame(g, payload[at:at + n].tobytes())
        out.append(fill(f) if ck and kind != R.TXD_ARP else f)
    return out


def reference(t, payload, mss, mtu, cap_bytes, out_cap, slot=0, flags=0):
    """(pkts, off, len, first, nseg, span, totals) by include/rxgpu.h's rules"""
    n = len(t)
    pk = np.full(cap_bytes, T.CANARY, np.uint8)
    off, ln = np.full(out_cap, ONES32, np.uint32), np.full(out_cap, ONES16, np.uint16)
    first, nseg = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    fe = pos = end = frames = written = 0
    full = False
    for k in range(n):
        fr = frames_of(t[k], payload, mss, mtu, slot, flags)
        s, ne = len(fr), max(1, len(fr))
        need = sum((len(f) + 63) // 64 * 64 for f in fr)
        ok = s > 0 and fe + s <= out_cap
        if ok and slot:
            ok = (fe + s) * slot <= cap_bytes
        elif ok:
            if full or pos + need > cap_bytes:
                ok, full = False, True
        first[k] = min(fe, ONES32)
        nseg[k] = s if ok else 0
        if not ok:
            for e in range(fe, min(fe + ne, out_cap)):
                off[e] = ln[e] = 0
            fe += ne
            continue
        for j, f in enumerate(fr):
            fl, at = len(f), ((fe + j) * slot if slot else pos)
            nb = (fl + 63) // 64 * 64
            pk[at:at + fl] = np.frombuffer(f, np.uint8)
            pk[at + fl:at + nb] = 0
            off[fe + j], ln[fe + j] = at // 64, fl
            end = at + nb
            if not slot:
                pos = end
        frames += s
        written += 1
        fe += ne
    tot = np.array([frames, end & ONES32, end >> 32, n - written, fe & ONES32, fe >> 32, 0, 0],
                   np.uint32)
    return pk, off, ln, first, nseg, end, tot


def sizes(t, payload, mss, mtu, slot=0):
    """(entries, bytes) that hold the whole burst"""
    ent = byt = 0
    for d in t:
        fr = frames_of(d, payload, mss, mtu, slot, R.TXE_NO_CKSUM)
        ent += max(1, len(fr))
        byt += sum((len(f) + 63) // 64 * 64 for f in fr)
    return ent, (ent * slot if slot else byt)


def reassemble(frames):
    """the datagram (UDP header + payload) of IPv4 fragments given in any order;
    asserts one id, one address pair, no gap, no overlap, MF on all but the last"""
    parts, ids = [], set()
    for f in frames:
        f = bytes(f)
        assert f[12:14] == b"\x08\x00" and f[14] == 0x45 and f[23] == 17
        tl, ident, fo = struct.unpack(">HHH", f[16:22])
        assert tl == len(f) - 14 and not fo & 0xC000  # DF and the reserved bit never set
        ids.add((ident, f[26:34], f[:12]))
        parts.append(((fo & 0x1FFF) * 8, bool(fo & 0x2000), f[34:]))
    assert len(ids) == 1
    parts.sort(key=lambda p: p[0])
    out = b""
    for i, (at, more, data) in enumerate(parts):
        assert at == len(out) and more == (i < len(parts) - 1)
        assert not more or len(data) % 8 == 0
        out += data
    return out


# ---- the boundary burst ----------------------------------------------------------
MACS = (T.PMAC, bytes.fromhex("0211223344ff"), bytes.fromhex("06a1b2c3d4e5"))


def boundary_descs(mtu, big=False):
    """UDP payloads around the cut (m = mtu - 28 is the longest uncut one) and
    around the fragment boundaries, ports, MACs and ids varying; TCP descriptors
    around MSS_OF[mtu], ARP and unknown kinds between them; big: a 65507-B
    payload (1365 entries at mtu 68) and a 65508-B one (skipped)"""
    m, fp, mss = mtu - 28, fp_of(mtu), MSS_OF[mtu]
    lens = (0, 1, m - 1, m, m + 1, fp - 9, fp - 8, fp - 7, 2 * fp - 9, 2 * fp - 8, 2 * fp - 7,
            4 * fp + 3, 5 * fp - 8)
    ds = []
    for i, n in enumerate(lens):
        ds.append(T.txd(R.TXD_UDP, n, sport=1000 + 7 * i, dport=53 + i, dst_mac=MACS[i % 3],
                        seq=(0xABCD0000 + 0x1F35 * i, 0xFFFF, 0)[i % 3] if i else 0x1234FFFF))
        if i % 3 == 0:
            o = (0, 1, 3)[i // 3 % 3]
            b = mss or 20
            ds.append(T.txd(R.TXD_TCP, (0, 1, b + 1, 4 * b + 3, 5 * b)[i // 3 % 5], optlen=o,
                            seq=0xFFFFFF00 + i, ack=0xA0B0C0D0 + i, tcp_flags=(0x10, 0x18, 0x19)[i % 3],
                            window=14600, urp=o, hdrlen_off=0x50 + (o << 4 & 0xF0), sport=2000 + i))
        if i % 5 == 0:
            ds.append(T.txd(R.TXD_ARP, 77, dst_mac=b"\xff" * 6 if i % 2 else T.PMAC))
        if i % 6 == 0:
            ds.append(T.txd(7, 10))
    if big:
        ds.insert(len(ds) // 2, T.txd(R.TXD_UDP, 65507, sport=4242, seq=0x00010002))
        ds.insert(len(ds) // 3, T.txd(R.TXD_UDP, 65508, sport=4243, seq=9))
    return ds


_BURSTS = {}


def burst(mtu, big=False):
    """(txd, payload) of the boundary burst, built once and never changed"""
    if (mtu, big) not in _BURSTS:
        t, pay = T.burst(boundary_descs(mtu, big), rng=np.random.default_rng(mtu + big))
        t.setflags(write=False)
        pay.setflags(write=False)
        _BURSTS[mtu, big] = (t, pay)
    return _BURSTS[mtu, big]
