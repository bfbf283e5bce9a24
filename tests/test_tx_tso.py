"""TCP segmentation in the TX encoder (rxg_tx_encode_tso_*, include/rxgpu.h) on
the CPU: rxg_tx_encode_tso_host against a reference for entries written here.
Every TCP descriptor is cut by hand into per-segment descriptors, each framed
by txenc_ref.ref_frame, the oracle's tx_cksum fills the checksums, and the
layout follows the header's rules 1-6; whole 0xA5-prefilled buffers, off / len
(prefilled with all ones), first, nseg and totals are compared.  Then the
socket layer's TX pass with nstack_set_tx_mss on a stack without a device, and
the host encoder under ASan + UBSan.  test_gpu_tx_tso.py pins the gfx950
kernel against rxg_tx_encode_tso_host."""
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
ERANGE, EINVAL = -34, -22
ONES32, ONES16 = 0xFFFFFFFF, 0xFFFF
OPTLENS = (0, 1, 2, 3, 10)  # header phases 6, 10, 14, 2 (and 6 again) mod 16
FLAGS = (0x10, 0x18, 0x19)


# ---- the reference -------------------------------------------------------------
def cut(d, mss, slot=0):
    """(s, hdr, [segment payload lengths]) of descriptor d; s == 0: skipped"""
    kind, pay = int(d["kind"]), int(d["pay_len"])
    if kind == R.TXD_TCP and mss:
        hdr = 54 + 4 * int(d["optlen"])
        s = max(1, -(-pay // mss))
        segs = [min(mss, pay - j * mss) for j in range(s)]
    else:
        hdr = {R.TXD_UDP: 42, R.TXD_TCP: 54 + 4 * int(d["optlen"]), R.TXD_ARP: 42}.get(kind, 0)
        segs = [0 if kind == R.TXD_ARP else pay]
        s = 1
    big = hdr + segs[0]
    if hdr == 0 or big > 65535 or (slot and big > slot):
        return 0, hdr, []
    return s, hdr, segs


def split(d, mss):
    """descriptor d cut by hand: [(per-segment descriptor, payload start, payload length)]"""
    s, _, segs = cut(d, mss)
    out = []
    for j, n in enumerate(segs):
        g = d.copy()
        if s > 1:
            g["seq"] = (int(d["seq"]) + j * mss) & 0xFFFFFFFF
            g["pay_len"] = n
            if j != s - 1:
                g["tcp_flags"] = int(d["tcp_flags"]) & ~0x09
        out.append((g, int(d["pay_off16"]) * 16 + j * mss, n))
    return out


def reference(t, payload, mss, cap_bytes, out_cap, slot=0, flags=0):
    """(pkts, off, len, first, nseg, span, totals) by include/rxgpu.h's rules"""
    n = len(t)
    pk = np.full(cap_bytes, T.CANARY, np.uint8)
    off, ln = np.full(out_cap, ONES32, np.uint32), np.full(out_cap, ONES16, np.uint16)
    first, nseg = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    fe = pos = end = frames = written = 0
    full = False
    for k in range(n):
        s, hdr, segs = cut(t[k], mss, slot)
        ne = max(1, s)
        need = sum((hdr + x + 63) // 64 * 64 for x in segs)
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
        for j, (g, o, pl) in enumerate(split(t[k], mss)):
            if int(g["kind"]) == R.TXD_ARP:
                pl = 0
            f = T.ref_frame(g, payload[o:o + pl].tobytes())
            fl, at = len(f), ((fe + j) * slot if slot else pos)
            assert fl == hdr + segs[j]
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
    if not flags & R.TXE_NO_CKSUM and end:
        live = (ln > 0) & (ln != ONES16)
        pk[:end] = O.tx_cksum(pk[:end], off[live], ln[live], 6)
    tot = np.array([frames, end & ONES32, end >> 32, n - written, fe & ONES32, fe >> 32, 0, 0],
                   np.uint32)
    return pk, off, ln, first, nseg, end, tot


# ---- bursts --------------------------------------------------------------------
def boundary_descs(mss, big=False):
    """optlen x pay_len around the segment boundaries (at mss 20 the segments
    0..3 start at source phases 0, 4, 8, 12 against every header phase), the
    three flag sets, a sequence number that wraps; UDP, ARP and unknown kinds
    between them; big: one 65535-B payload as well"""
    ds, i = [], 0
    for o in OPTLENS:
        for n in (0, 1, mss - 1, mss, mss + 1, 2 * mss, 4 * mss + 3, 5 * mss):
            # 0xFFFFFF00 wraps from segment 1 on at mss 1460 and 8948, -20 at mss 20
            seq = (0xFFFFFF00, 0x01020304 + n, 0xFFFFFFEC)[(i // 8 + 2 * i) % 3]
            ds.append(T.txd(R.TXD_TCP, n, optlen=o, seq=seq,
                            ack=0xA0B0C0D0 + o, tcp_flags=FLAGS[i % 3], window=14600, urp=o,
                            hdrlen_off=0x50 + (o << 4 & 0xF0), sport=2000 + i))
            if i % 5 == 0:
                ds.append(T.txd(R.TXD_UDP, (mss + 7) % 1473, sport=1000 + i))
            if i % 7 == 0:
                ds.append(T.txd(R.TXD_ARP, 77, dst_mac=b"\xff" * 6 if i % 2 else T.PMAC))
            if i % 11 == 0:
                ds.append(T.txd(7, 10))
            i += 1
    if big:
        ds.insert(len(ds) // 2, T.txd(R.TXD_TCP, 65535, optlen=1, seq=0xFFFF0000, ack=5,
                                      tcp_flags=0x19, window=512, hdrlen_off=0x60))
    return ds


_BURSTS = {}


def burst(mss, big=False):
    """(txd, payload) of the boundary burst, built once and never changed"""
    if (mss, big) not in _BURSTS:
        t, pay = T.burst(boundary_descs(mss, big), rng=np.random.default_rng(mss + big))
        t.setflags(write=False)
        pay.setflags(write=False)
        _BURSTS[mss, big] = (t, pay)
    return _BURSTS[mss, big]


def sizes(t, mss, slot=0):
    """(entries, bytes) that hold the whole burst"""
    ent = sum(max(1, cut(d, mss, slot)[0]) for d in t)
    if slot:
        return ent, ent * slot
    return ent, sum((cut(d, mss)[1] + x + 63) // 64 * 64 for d in t for x in cut(d, mss)[2])


def _check(t, pay, mss, cap=None, out_cap=None, slot=0, flags=0, want_rc=None):
    ent, byt = sizes(t, mss, slot)
    cap = byt + 256 if cap is None else cap
    out_cap = ent + 3 if out_cap is None else out_cap
    want = reference(t, pay, mss, cap, out_cap, slot, flags)
    pk, off, ln, first, nseg, span, tot, rc = R.tx_encode_tso_host(
        t, pay, mss, cap, out_cap, slot, flags, fill=T.CANARY, fill_entries=ONES32)
    assert rc == (want_rc if want_rc is not None else (ERANGE if want[6][3] else 0))
    assert span == want[5] and list(tot) == list(want[6])
    assert np.array_equal(first, want[3]) and np.array_equal(nseg, want[4])
    assert np.array_equal(off, want[1]) and np.array_equal(ln, want[2])
    assert np.array_equal(pk, want[0])  # whole buffer: gaps and the canary past the span too
    return pk, off, ln, first, nseg, tot


@pytest.mark.parametrize("mss,big", [(20, False), (1460, True), (8948, False)])
@pytest.mark.parametrize("slot", [0, "slots"])
def test_boundary_burst(mss, big, slot):
    t, pay = burst(mss, big)
    if slot:  # 128 holds every frame at mss 20, 1536 at 1460, 9088 at 8948
        slot = {20: 128, 1460: 1536, 8948: 9088}[mss]
    pk, off, ln, first, nseg, tot = _check(t, pay, mss, slot=slot)
    tcp = t["kind"] == R.TXD_TCP
    assert int(nseg.max()) == (45 if big else 5)
    assert set(nseg[~tcp]) <= {0, 1}
    assert tot[0] == nseg.sum() and tot[3] == (nseg == 0).sum() > 0  # the unknown kinds
    # segments 0..3 of a 5-segment descriptor: FIN / PSH only on the last, seq wraps
    k = int(np.flatnonzero((t["pay_len"] == 5 * mss) & (nseg == 5) & (t["tcp_flags"] == 0x19) &
                           (t["seq"] == 0xFFFFFF00))[0])
    fr = [pk[int(off[e]) * 64:int(off[e]) * 64 + int(ln[e])] for e in range(first[k], first[k] + 5)]
    assert [int(f[47]) for f in fr] == [0x10] * 4 + [0x19]
    assert [struct.unpack(">I", f[38:42].tobytes())[0] for f in fr] == \
        [(0xFFFFFF00 + j * mss) & ONES32 for j in range(5)]
    o = int(t[k]["pay_off16"]) * 16
    hdr = 54 + 4 * int(t[k]["optlen"])
    assert b"".join(f[hdr:].tobytes() for f in fr) == pay[o:o + 5 * mss].tobytes()


def test_slot_smaller_than_a_segment_skips_the_descriptor():
    t, pay = burst(1460, True)
    _, _, _, _, nseg, tot = _check(t, pay, 1460, slot=128)
    want = [1 if cut(d, 1460, 128)[0] else 0 for d in t]
    assert [int(x > 0) for x in nseg] == want and 0 < sum(want) < len(t)


@pytest.mark.parametrize("mss,slot", [(20, 0), (20, 128), (1460, 0), (1460, 1536)])
def test_capacity_runs_out_inside_a_descriptor(mss, slot):
    """cap_bytes, then out_cap, end in the middle of a descriptor's segments:
    that descriptor and every later one are skipped whole"""
    t, pay = burst(mss, mss == 1460)
    k = int(np.flatnonzero(t["pay_len"] == 5 * mss)[1])  # a 5-segment descriptor
    ent, byt = sizes(t[:k], mss, slot)
    seg = slot or (54 + 4 * int(t[k]["optlen"]) + mss + 63) // 64 * 64
    _, off, ln, first, nseg, tot = _check(t, pay, mss, cap=byt + 3 * seg + 8, slot=slot)
    total = sizes(t, mss, slot)[0]
    assert first[k] == ent and tot[3] == (nseg == 0).sum() and tot[0] == nseg.sum()
    assert not nseg[k:].any() and not ln[ent:total].any() and not off[ent:total].any()
    assert (ln[total:] == ONES16).all()  # past the entries needed: untouched
    # out_cap: three of its five entries exist, and are zeroed; nothing past them is written
    _, off, ln, first, nseg, tot = _check(t, pay, mss, out_cap=ent + 3, slot=slot)
    assert not nseg[k:].any() and list(ln[ent:]) == [0, 0, 0]
    assert (tot[4] | int(tot[5]) << 32) == sizes(t, mss, slot)[0] > ent + 3
    # exactly enough of both: written
    _, _, _, _, nseg, _ = _check(t[:k + 1], pay, mss, cap=byt + 5 * seg, out_cap=ent + 5, slot=slot)
    assert nseg[k] == 5
    _check(t[:k + 1], pay, mss, cap=byt + 5 * seg, out_cap=0, slot=slot)


def test_no_checksum():
    t, pay = burst(20)
    pk, off, ln, _, nseg, _ = _check(t, pay, 20, flags=R.TXE_NO_CKSUM)
    for e in np.flatnonzero(ln > 0):
        f = pk[int(off[e]) * 64:]
        if f[12:14].tobytes() == b"\x08\x00":
            hole = 40 if f[23] == 17 else 50
            assert not f[24:26].any() and not f[hole:hole + 2].any()


def test_mss_must_be_a_multiple_of_4():
    t, pay = burst(20)
    for mss in (1, 2, 3, 18, 1461, 1462):
        with pytest.raises(R.RxgError) as e:
            R.tx_encode_tso_host(t, pay, mss, 1 << 16, 1024)
        assert e.value.rc == EINVAL
        with pytest.raises(R.RxgError) as e:
            R.tx_tso_count(t, mss)
        assert e.value.rc == EINVAL


@pytest.mark.parametrize("mss", [0, 1460])
@pytest.mark.parametrize("slot", [0, 1536])
def test_special_case_is_rxg_tx_encode_host(mss, slot):
    """mss == 0, or every TCP payload <= mss: the old call's output, entry k = descriptor k"""
    ds = T.mix_descs()
    t, pay = T.burst(ds)
    n = len(t)
    cap = (n * slot if slot else sum((T.frame_len(d) + 63) // 64 * 64 for d in t)) + 256
    w_pk, w_off, w_ln, w_span, w_tot, w_rc = R.tx_encode_host(t, pay, cap, slot, 0, fill=T.CANARY)
    for out_cap in (n, n + 5):
        pk, off, ln, first, nseg, span, tot, rc = R.tx_encode_tso_host(
            t, pay, mss, cap, out_cap, slot, 0, fill=T.CANARY, fill_entries=ONES32)
        assert rc == w_rc and span == w_span and list(tot[:4]) == list(w_tot)
        assert (tot[4], tot[5]) == (n, 0)
        assert np.array_equal(pk, w_pk)
        assert np.array_equal(off[:n], w_off) and np.array_equal(ln[:n], w_ln)
        assert (off[n:] == ONES32).all() and (ln[n:] == ONES16).all()
        assert np.array_equal(first, np.arange(n)) and np.array_equal(nseg, (w_ln != 0))
    _check(t, pay, mss, slot=slot)


@pytest.mark.parametrize("mss", [0, 20, 1460, 8948])
def test_count(mss):
    t, pay = burst(1460, True)
    assert R.tx_tso_count(t, mss) == sizes(t, mss)
    assert R.tx_tso_count(t[:0], mss) == (0, 0)


def test_invalid_arguments():
    t, pay = burst(20)
    with pytest.raises(R.RxgError) as e:
        R.tx_encode_tso_host(t, pay, 20, 1 << 16, 1024, slot_bytes=100)
    assert e.value.rc == EINVAL
    with pytest.raises(R.RxgError) as e:  # a payload that ends past the payload buffer
        R.tx_encode_tso_host(t, pay[:-1], 20, 1 << 16, 1024)
    assert e.value.rc == EINVAL
    span = C.c_uint64(5)
    tot = np.ones(8, np.uint32)
    assert R._tx_encode_tso_host(None, 0, None, 0, 20, None, 0, 0, None, None, 0, None, None, 0,
                                 C.byref(span), tot.ctypes.data) == 0
    assert span.value == 0 and not tot.any()
    assert R._tx_encode_tso_host(None, 1, None, 0, 20, None, 0, 0, None, None, 0, None, None, 0,
                                 None, None) == EINVAL
    # the context calls: no context at all, and a context without a device
    assert R._tx_encode_tso(None, 16, 1, 16, 64, 20, 16, 256, 16, 16, 4, 16, 16, 0, None) == EINVAL
    assert R._tx_encode_tso_dev(None, 16, 1, 16, 20, 64, 256, 0, 16, 16, 4, 16, 16, 64, 0, 16,
                                None) == EINVAL
    with R.Context(R.HOST_ONLY) as c:
        with pytest.raises(R.RxgError) as e:
            c.tx_encode_tso(t, pay, 20, 4096, 64)
        assert e.value.rc == -19  # no CPU fallback behind the device calls
        with pytest.raises(R.RxgError) as e:
            c.tx_encode_tso_dev(16, 1, 16, 20, 64, 4096, 0, 16, 16, 4, 16, 16, 64, 0, 16)
        assert e.value.rc == -19


def test_symbols_are_listed():
    for name in ("rxg_tx_encode_tso_dev", "rxg_tx_encode_tso", "rxg_tx_encode_tso_host",
                 "rxg_tx_tso_count"):
        assert name in R.EXPORTED


# ---- the socket layer with no device (nstack_set_tx_mss) -------------------------
L, LMAC, PMAC = T.L_IP, F.LOCAL_MAC, F.PEER_MAC


@pytest.fixture()
def conn():
    """a stack without a device and an accepted connection to 10.0.0.8:40001"""
    ns = R.NStack(R.HOST_ONLY)
    ns.set_local(L, LMAC)
    ns.arp_insert("10.0.0.8", PMAC)
    lfd = ns.socket(R.SOCK_STREAM)
    ns.bind(lfd, L, 9999)
    ns.listen(lfd)
    ns.tcb_add("10.0.0.8", L, 40001, 9999)
    cfd, _ = ns.accept(lfd)
    yield ns, cfd
    ns.fini()


def _tcp(f):
    return dict(seq=struct.unpack(">I", f[38:42])[0], flags=f[47], pay=f[54:],
                tl=struct.unpack(">H", f[16:18])[0])


def test_nstack_send_is_cut_at_mss(conn):
    ns, cfd = conn
    data = bytes(np.random.default_rng(3).integers(0, 256, 4000, np.uint8))
    assert ns.set_tx_mss(1460) == 0
    assert ns.send(cfd, data) == 4000
    fr = [_tcp(f) for f in ns.tx_burst()]
    assert [len(f["pay"]) for f in fr] == [1460, 1460, 1080]
    assert [f["tl"] for f in fr] == [40 + 1460, 40 + 1460, 40 + 1080]
    assert [f["seq"] - fr[0]["seq"] for f in fr] == [0, 1460, 2920]
    assert [f["flags"] for f in fr] == [0x10, 0x10, 0x18]  # PSH only on the last
    assert b"".join(f["pay"] for f in fr) == data
    assert ns.stat(14) == 1 and ns.tx_burst() == []
    # a send that fits one segment is one frame and counts nothing
    ns.send(cfd, data[:1460])
    fr = ns.tx_burst()
    assert len(fr) == 1 and _tcp(fr[0])["flags"] == 0x18 and ns.stat(14) == 1


def test_nstack_partial_send(conn):
    """max_frames 2: two segments now (FIN / PSH cleared), the fragment stays
    at the head with seq, data and length advanced; the next pass sends the rest"""
    ns, cfd = conn
    data = bytes(np.random.default_rng(4).integers(0, 256, 4000, np.uint8))
    ns.set_tx_mss(1460)
    ns.send(cfd, data)
    ns.send(cfd, b"next")
    a = [_tcp(f) for f in ns.tx_burst(max_frames=2)]
    assert [len(f["pay"]) for f in a] == [1460, 1460] and [f["flags"] for f in a] == [0x10, 0x10]
    assert ns.stat(14) == 1
    b = [_tcp(f) for f in ns.tx_burst(max_frames=2)]
    assert [len(f["pay"]) for f in b] == [1080] and b[0]["flags"] == 0x18
    assert b[0]["seq"] == (a[0]["seq"] + 2920) & ONES32
    assert b"".join(f["pay"] for f in a + b) == data
    assert ns.stat(14) == 1  # the rest went out as one frame
    c = ns.tx_burst(max_frames=2)
    assert [_tcp(f)["pay"] for f in c] == [b"next"]
    # the buffer, not the frame count, ends the pass: room for one 1514-B frame (1536 B)
    ns.send(cfd, data)
    a = ns.tx_burst(cap_bytes=2 * 1536 - 1)
    assert [len(_tcp(f)["pay"]) for f in a] == [1460]
    assert ns.tx_burst(cap_bytes=1535) == []  # r == 0: it stays queued
    b = ns.tx_burst()
    assert [len(_tcp(f)["pay"]) for f in b] == [1460, 1080] and ns.stat(14) == 2
    assert b"".join(_tcp(f)["pay"] for f in a + b) == data


def test_nstack_without_mss_is_one_frame(conn):
    ns, cfd = conn
    data = bytes(4000)
    ns.send(cfd, data)
    fr = ns.tx_burst()
    assert len(fr) == 1 and len(fr[0]) == 54 + 4000 and ns.stat(14) == 0
    with pytest.raises(R.RxgError) as e:
        ns.set_tx_mss(1461)
    assert e.value.rc == EINVAL
    ns.set_tx_mss(1460)
    ns.set_tx_mss(0)  # off again
    ns.send(cfd, data)
    assert len(ns.tx_burst()) == 1
    # the 65535-B rule applies to a segment's frame, not the whole fragment
    ns.set_tx_mss(1460)
    ns.send(cfd, bytes(70000))
    fr = ns.tx_burst()
    assert len(fr) == 48 and sum(len(f) - 54 for f in fr) == 70000 and ns.stat(1) == 0


# ---- the host encoder under AddressSanitizer + UndefinedBehaviorSanitizer ------
@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None,
                    reason="needs gcc/g++")
def test_tso_host_encoder_under_asan_ubsan(tmp_path):
    """tests/san/tso_harness.c, a stand-alone program: the boundary burst into
    exact-size heap buffers, compiled together with tx_encode_host.cpp with
    -fsanitize=address,undefined and run directly"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    objs = []
    for src, cc, std in [("tests/san/tso_harness.c", "gcc", "-std=gnu11"),
                         ("dpdk-tcp-udp_protocol_stack_amd/csrc/tx_encode_host.cpp", "g++",
                          "-std=c++17")]:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, *san, "-Iinclude", "-c", os.path.join(ROOT, src), "-o", o],
                       check=True, cwd=ROOT)
        objs.append(o)
    exe = str(tmp_path / "tso_harness")
    subprocess.run(["g++", *san, *objs, "-o", exe], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "TSO SAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
