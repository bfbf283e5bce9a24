"""TX encode (K5) on the CPU: rxg_tx_encode_host, the plain C++
restatement of the GPU encoder, against a Python restatement of the
reference's three encoders (txenc_ref.py) whose checksums the oracle fills;
bit-exact on whole buffers, off / len / span / totals and a 0xA5 canary past
the span included.  test_gpu_tx_encode.py pins the gfx950 kernel against the
same reference."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxgpu as R
import txenc_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd")
ERANGE, EINVAL, ENODEV = -34, -22, -19


def _check(descs, cap=None, slot=0, flags=0, payloads=None, want_rc=0):
    t, pay = T.burst(descs, payloads=payloads)
    if cap is None:
        cap = (len(t) * slot if slot else sum((T.frame_len(d) + 63) // 64 * 64 for d in t)) + 256
    want = T.reference(t, pay, cap, slot, flags)
    pk, off, ln, span, tot, rc = R.tx_encode_host(t, pay, cap, slot, flags, fill=T.CANARY)
    assert rc == want_rc
    assert span == want[3] and list(tot) == list(want[4])
    assert np.array_equal(off, want[1]) and np.array_equal(ln, want[2])
    assert np.array_equal(pk, want[0])  # whole buffer: gaps and the canary past the span too
    if span < cap:
        assert (pk[span:] == T.CANARY).all()
    return pk, off, ln, want


@pytest.mark.parametrize("n", T.UDP_LENS)
def test_udp_lengths(n):
    pk, off, ln, _ = _check([T.txd(R.TXD_UDP, n)])
    assert ln[0] == 42 + n
    if n == 22:
        assert ln[0] == 64  # exactly one 64-B unit; 23 crosses into the next


@pytest.mark.parametrize("optlen", T.TCP_OPTLENS)
def test_tcp_options_and_payloads(optlen):
    ds = [T.txd(R.TXD_TCP, n, optlen=optlen, seq=0xFFFFFFFE, ack=7, tcp_flags=0x18, window=0x3908,
                urp=0x0201) for n in T.TCP_LENS]
    _, _, ln, _ = _check(ds)
    assert list(ln) == [54 + 4 * optlen + n for n in T.TCP_LENS]


def test_arp_targets():
    pk, _, ln, _ = _check([T.txd(R.TXD_ARP, dst_mac=T.PMAC), T.txd(R.TXD_ARP, dst_mac=b"\xff" * 6)])
    assert list(ln) == [42, 42]
    assert pk[0:6].tobytes() == T.PMAC and pk[32:38].tobytes() == T.PMAC
    assert pk[64:70].tobytes() == bytes(6) and pk[96:102].tobytes() == b"\xff" * 6


def test_boundary_burst_packed():
    _check(T.boundary_descs())


@pytest.mark.parametrize("slot,flags", [(0, 0), (1536, 0), (0, R.TXE_NO_CKSUM), (1536, R.TXE_NO_CKSUM)])
def test_random_mix(slot, flags):
    ds = T.mix_descs()
    long_ones = sum(T.frame_len(d) > 1536 for d in ds)
    assert long_ones > 0
    pk, off, ln, _ = _check(ds, slot=slot, flags=flags, want_rc=ERANGE if slot else 0)
    if slot:
        assert int((ln == 0).sum()) == long_ones  # larger than the slot: skipped
    if flags:  # both fields of every IPv4 frame stay 0
        for d, o, n in zip(ds, off, ln):
            s, hole = int(o) << 6, 40 if int(d["kind"]) == R.TXD_UDP else 50
            if n and int(d["kind"]) != R.TXD_ARP:
                assert not pk[s + 24:s + 26].any() and not pk[s + hole:s + hole + 2].any()


def test_slots_of_64():
    """slot_bytes 64: only frames of at most 64 B are written, each in its own slot"""
    ds = [T.txd(R.TXD_UDP, n) for n in (0, 22, 23, 5)] + [T.txd(R.TXD_ARP), T.txd(R.TXD_TCP, 10),
                                                          T.txd(R.TXD_TCP, 11)]
    _, off, ln, _ = _check(ds, slot=64, want_rc=ERANGE)
    assert list(ln) == [42, 64, 0, 47, 42, 64, 0]
    assert list(off) == [0, 1, 0, 3, 4, 5, 0]


def test_skips():
    ds = T.skip_descs()
    _, off, ln, want = _check(ds, want_rc=ERANGE)
    assert list(ln) == [72, 0, 0, 254, 142, 42, 1042]
    assert list(want[4]) == [5, want[3], 0, 2]
    assert list(off) == [0, 0, 0, 2, 6, 9, 10]  # a skipped descriptor takes no space
    # cap_bytes exhausted mid-burst: the first frame that does not fit ends the burst
    cap = 128 + 256 + 192  # room for frames 0, 3, 4
    _, off, ln, want = _check(ds, cap=cap, want_rc=ERANGE)
    assert list(ln) == [72, 0, 0, 254, 142, 0, 0] and want[3] == cap
    _, _, ln, _ = _check(ds, cap=cap - 1, want_rc=ERANGE)
    assert list(ln) == [72, 0, 0, 254, 0, 0, 0]
    # slots: the slot itself must fit
    _, _, ln, _ = _check(ds, cap=4 * 1536 + 100, slot=1536, want_rc=ERANGE)
    assert list(ln) == [72, 0, 0, 254, 0, 0, 0]


def _l4_sum(frame):
    """folded one's-complement sum rte_ipv4_udptcp_cksum complements (field taken as 0)"""
    proto = frame[23]
    l4 = bytearray(frame[34:])
    hole = 6 if proto == 17 else 16
    l4[hole:hole + 2] = b"\0\0"
    return F.fold_cksum(frame[26:34] + bytes([0, proto]) + struct.pack(">H", len(l4)) + bytes(l4))


def test_udp_zero_checksum_is_stored_as_ffff():
    """rte_ip.h:346-347: a UDP checksum of 0 goes out as 0xFFFF; the datagram
    is found by a search over two payload bytes"""
    base = bytearray(b"zero\0\0um payload")
    d = T.txd(R.TXD_UDP, len(base))
    # payload bytes 4, 5 are one 16-bit word of the sum: every value at once
    t = _l4_sum(T.ref_frame(d, bytes(base))) + np.arange(65536)
    hits = np.flatnonzero((t & 0xFFFF) + (t >> 16) == 0xFFFF)
    assert len(hits)
    base[4:6] = int(hits[0]).to_bytes(2, "little")
    hit = bytes(base)
    assert _l4_sum(T.ref_frame(d, hit)) == 0xFFFF
    pk, _, _, want = _check([d], payloads=[hit])
    assert want[0][40:42].tobytes() == b"\xff\xff"  # the reference exercises the rule
    assert (~_l4_sum(want[0][:58].tobytes())) & 0xFFFF == 0
    assert pk[40:42].tobytes() == b"\xff\xff"


def test_ipv4_checksum_ffff_rule():
    """a header whose folded sum is 0xFFFF stores 0: rte_ipv4_cksum as compiled
    into the reference (DPDK 19.11.12) is the plain complement, without the
    keep-0xFFFF rule of later releases (tests/test_ref_differential.py holds
    the oracle to the compiled code); found by a search over the low half of dip"""
    d = T.txd(R.TXD_UDP, 3)
    d["dip"] = int(d["dip"]) & 0xFFFF0000
    t = F.fold_cksum(T.ref_frame(d, b"abc")[14:34]) + np.arange(65536)  # every low half at once
    hits = np.flatnonzero((t & 0xFFFF) + (t >> 16) == 0xFFFF)
    assert len(hits)
    d["dip"] = int(d["dip"]) | int(hits[0])
    assert F.fold_cksum(T.ref_frame(d, b"abc")[14:34]) == 0xFFFF
    pk, _, _, want = _check([d])
    assert want[0][24:26].tobytes() == b"\0\0"
    assert pk[24:26].tobytes() == b"\0\0"
    assert pk[40:42].tobytes() != b"\0\0"  # the checksums were filled


# ---- pins against the socket layer's host encoders (host/nstack.c) ----------
L, LMAC, PMAC = T.L_IP, F.LOCAL_MAC, F.PEER_MAC


def _same_as_stack(frames, descs, payloads):
    """the stack's frames (checksums 0) equal the encoder's with NO_CKSUM; the
    filled version verifies on rx"""
    t, pay = T.burst(descs, payloads=payloads)
    cap = sum((len(f) + 63) // 64 * 64 for f in frames)
    pk, off, ln, span, _, rc = R.tx_encode_host(t, pay, cap, 0, R.TXE_NO_CKSUM)
    assert rc == 0 and span == cap
    got = [pk[int(o) << 6:(int(o) << 6) + int(n)].tobytes() for o, n in zip(off, ln)]
    assert got == frames
    pk, off, ln, _, _, _ = R.tx_encode_host(t, pay, cap, 0, 0)
    v = O.Tables(np.zeros(0, R.UDP_SOCK_DTYPE), np.zeros(0, R.TCB_DTYPE)).classify(pk, off, ln, 6)
    for i, d in enumerate(t):
        if int(d["kind"]) != R.TXD_ARP:
            assert v["cksum_ok"][i] == 1


@pytest.fixture()
def ns():
    s = R.NStack(R.HOST_ONLY)
    yield s
    s.fini()


def _deliver(ns, frames):
    u, t = ns.flows()
    buf, off, lens = F.pack_frames(frames)
    v = ns.to_ids(O.Tables(u, t).classify(buf, off, lens, 6))
    ns.deliver(frames, v, np.zeros(len(frames), np.int32))


def test_pin_udp_arp_then_datagram(ns):
    ns.set_local(L, LMAC)
    fd = ns.socket(R.SOCK_DGRAM)
    ns.bind(fd, L, 8889)
    assert ns.sendto(fd, b"reply", "10.0.0.1", 5555) == 5
    arp = ns.tx_burst()
    _deliver(ns, [F.arp_frame("10.0.0.1", L)])
    dg = ns.tx_burst()
    assert len(arp) == 1 and len(dg) == 1
    _same_as_stack(arp + dg,
                   [T.txd(R.TXD_ARP, src_mac=LMAC, dst_mac=b"\xff" * 6, sip=L, dip="10.0.0.1"),
                    T.txd(R.TXD_UDP, 5, src_mac=LMAC, dst_mac=PMAC, sip=L, dip="10.0.0.1",
                          sport=8889, dport=5555)], [None, b"reply"])


def test_pin_one_datagram_per_socket(ns):
    ns.set_local(L, LMAC)
    ns.arp_insert("10.0.0.1", PMAC)
    a, b = ns.socket(R.SOCK_DGRAM), ns.socket(R.SOCK_DGRAM)
    ns.bind(a, L, 1000)
    ns.bind(b, L, 2000)
    for fd, p in ((a, b"a1"), (a, b"a2"), (b, b"b1")):
        ns.sendto(fd, p, "10.0.0.1", 7777)
    frames = ns.tx_burst() + ns.tx_burst()
    assert len(frames) == 3
    mk = lambda sport: T.txd(R.TXD_UDP, 2, src_mac=LMAC, dst_mac=PMAC, sip=L, dip="10.0.0.1",  # noqa: E731
                             sport=sport, dport=7777)
    _same_as_stack(frames, [mk(2000), mk(1000), mk(1000)], [b"b1", b"a1", b"a2"])


def test_pin_tcp_synack_and_data(ns):
    SYN, ACK, PSH = 0x02, 0x10, 0x08
    seg = lambda fl, **kw: F.tcp_frame("10.0.0.9", 40000, L, 9999, b"", flags=fl, **kw)  # noqa: E731
    ns.set_local(L, LMAC)
    ns.arp_insert("10.0.0.9", PMAC)
    lfd = ns.socket(R.SOCK_STREAM)
    ns.bind(lfd, L, 9999)
    ns.listen(lfd)
    _deliver(ns, [seg(SYN, seq=5000)])
    synack = ns.tx_burst()
    assert len(synack) == 1
    isn = struct.unpack(">I", synack[0][38:42])[0]  # (the stack's random ISN)
    _deliver(ns, [seg(ACK, seq=5001, ack=isn + 1)])
    cfd, _ = ns.accept(lfd)
    assert ns.send(cfd, b"hi there") == 8
    data = ns.tx_burst()
    assert len(data) == 1
    dseq, dack = struct.unpack(">II", data[0][38:46])
    win = int.from_bytes(synack[0][48:50], "little")
    mk = lambda n, **kw: T.txd(R.TXD_TCP, n, src_mac=LMAC, dst_mac=PMAC, sip=L, dip="10.0.0.9",  # noqa: E731
                               sport=9999, dport=40000, hdrlen_off=0x50, **kw)
    _same_as_stack(synack + data,
                   [mk(0, seq=isn, ack=5001, tcp_flags=SYN | ACK, window=win),
                    mk(8, seq=dseq, ack=dack, tcp_flags=PSH | ACK,
                       window=int.from_bytes(data[0][48:50], "little"))], [None, b"hi there"])


def test_stack_encoder_switch_needs_gpu(ns):
    """set_tx_encode on a host-only stack: without checksums the host frames as
    before (the switch matters only with cksum); with them the library refuses
    (RXG_ENODEV), as rxg_tx_cksum does, and nothing counts as encoded"""
    ns.set_local(L, LMAC)
    ns.arp_insert("10.0.0.1", PMAC)
    fd = ns.socket(R.SOCK_DGRAM)
    ns.bind(fd, L, 8889)
    assert ns.set_tx_encode(True) == 0
    ns.sendto(fd, b"one", "10.0.0.1", 5555)
    assert [f[42:] for f in ns.tx_burst()] == [b"one"]
    ns.sendto(fd, b"two", "10.0.0.1", 5555)
    with pytest.raises(R.RxgError) as e:
        ns.tx_burst(cksum=True)
    assert e.value.rc == ENODEV
    assert ns.stat(13) == 0


# ---- ABI ----------------------------------------------------------------------
def test_descriptor_layout():
    assert R.TXD_DTYPE.itemsize == 48
    want = dict(dst_mac=0, src_mac=6, sip=12, dip=16, sport=20, dport=22, seq=24, ack=28, window=32,
                urp=34, hdrlen_off=36, tcp_flags=37, optlen=38, kind=39, pay_off16=40, pay_len=44)
    assert {k: R.TXD_DTYPE.fields[k][1] for k in R.TXD_DTYPE.names} == want

    class Txd(C.Structure):
        _fields_ = [("dst_mac", C.c_uint8 * 6), ("src_mac", C.c_uint8 * 6), ("sip", C.c_uint32),
                    ("dip", C.c_uint32), ("sport", C.c_uint16), ("dport", C.c_uint16),
                    ("seq", C.c_uint32), ("ack", C.c_uint32), ("window", C.c_uint16),
                    ("urp", C.c_uint16), ("hdrlen_off", C.c_uint8), ("tcp_flags", C.c_uint8),
                    ("optlen", C.c_uint8), ("kind", C.c_uint8), ("pay_off16", C.c_uint32),
                    ("pay_len", C.c_uint32)]
    assert C.sizeof(Txd) == 48
    assert {k: getattr(Txd, k).offset for k in want} == want
    assert (R.TXD_UDP, R.TXD_TCP, R.TXD_ARP) == (0, 1, 2)


def test_host_only_context_refuses():
    t, pay = T.burst([T.txd(R.TXD_UDP, 5)])
    with R.Context(R.HOST_ONLY) as c:
        with pytest.raises(R.RxgError) as e:
            c.tx_encode(t, pay, 4096)
        assert e.value.rc == ENODEV  # no CPU fallback behind the device calls
        with pytest.raises(R.RxgError) as e:
            c.tx_encode_dev(16, 1, 16, 64, 4096, 0, 16, 16, 64, 0, 16)
        assert e.value.rc == ENODEV
        with pytest.raises(R.RxgError):
            c.tune_txe(10**6)
        c.tune_txe(0)
        c.tune_txe(R.TX_AUTO)


def test_invalid_arguments():
    t, pay = T.burst([T.txd(R.TXD_UDP, 5)])
    pk, off, ln = np.zeros(256, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.uint16)
    span = C.c_uint64()

    def call(txd=t.ctypes.data, n=1, payload=pay.ctypes.data, pbytes=len(pay), pkts=pk.ctypes.data,
             cap=256, slot=0, o=off.ctypes.data, l=ln.ctypes.data):  # noqa: E741
        return R._tx_encode_host(txd, n, payload, pbytes, pkts, cap, slot, o, l, 0, C.byref(span), None)

    assert call() == 0 and span.value == 64
    assert call(n=0, txd=None, pkts=None, o=None, l=None) == 0 and span.value == 0  # n == 0 is OK
    for kw in (dict(txd=None), dict(pkts=None), dict(o=None), dict(l=None), dict(payload=None),
               dict(pbytes=4), dict(slot=100), dict(slot=32)):
        assert call(**kw) == EINVAL, kw
    assert call(slot=128) == 0
    # the context calls: no context at all
    assert R._tx_encode(None, t.ctypes.data, 1, pay.ctypes.data, len(pay), pk.ctypes.data, 256,
                        off.ctypes.data, ln.ctypes.data, 0, C.byref(span)) == EINVAL
    assert R._tx_encode_dev(None, 16, 1, 16, 64, 256, 0, 16, 16, 64, 0, 16, None) == EINVAL


# ---- the host encoder under AddressSanitizer + UndefinedBehaviorSanitizer ------
@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None,
                    reason="needs gcc/g++")
def test_host_encoder_under_asan_ubsan(tmp_path):
    """tests/san/txenc_harness.c, a stand-alone program: the boundary lengths
    into exact-size heap buffers, compiled together with tx_encode_host.cpp
    with -fsanitize=address,undefined and run directly"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    objs = []
    for src, cc, std in [("tests/san/txenc_harness.c", "gcc", "-std=gnu11"),
                         ("dpdk-tcp-udp_protocol_stack_amd/csrc/tx_encode_host.cpp", "g++",
                          "-std=c++17")]:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, *san, "-Iinclude", "-c", os.path.join(ROOT, src), "-o", o],
                       check=True, cwd=ROOT)
        objs.append(o)
    exe = str(tmp_path / "txenc_harness")
    subprocess.run(["g++", *san, *objs, "-o", exe], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "TXENC SAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
