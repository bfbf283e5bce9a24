"""TCP segmentation in the TX encoder on the GPU (csrc/tx_encode.hip, the TSO
layout pass and tx_encode_tso_kernel): the device form against the host
restatement (rxg_tx_encode_tso_host, itself pinned to a hand-cut reference by
test_tx_tso.py) bit-exact on whole 0xA5-prefilled buffers, off / len prefilled
with -1 so entries at or past out_cap are seen untouched, every len_hint class
and every variant of the kernel's table, packed and in slots, the capacity
cases and no-checksum; the special case that equals rxg_tx_encode_dev; the
host form; the round trip of a cut payload through K1 and K2; and the socket
layer's TX pass with nstack_set_tx_mss, encoder on against host-framed."""
import struct

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxgpu as R
import test_tx_tso as TT
import txenc_ref as T

ERANGE, EINVAL = -34, -22
HINTS = (64, 128, 354, 1500, 9000)
N_VARIANTS = 15  # csrc/tx_encode.hip k_txe / k_txe_tso
SLOTS = {20: 128, 512: 1536, 1460: 1536, 8948: 9088}


def _dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")
    return torch, torch.device("cuda", 0)


class Burst:
    """descriptors + payloads on the device, and the host restatement's answers"""

    def __init__(self, t, pay, mss, dev, torch):
        self.torch, self.dev, self.t, self.pay, self.mss = torch, dev, t, pay, mss
        self.n = len(t)
        self.d_txd = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
        pad = np.zeros((len(pay) + 15) // 16 * 16 + 16, np.uint8)  # to the 16-B end
        pad[:len(pay)] = pay
        self.d_pay = torch.from_numpy(pad).to(dev)
        self.ent, self.bytes = R.tx_tso_count(t, mss)
        self.want = {}

    def sizes(self, slot, cap=None, out_cap=None):
        """defaults: room for everything, five spare entries and 256 spare bytes"""
        out_cap = self.ent + 5 if out_cap is None else out_cap
        if cap is None:
            cap = (self.ent * slot if slot else self.bytes) + 256
        return cap, out_cap

    def host(self, slot, flags=0, cap=None, out_cap=None):
        cap, out_cap = self.sizes(slot, cap, out_cap)
        key = (slot, flags, cap, out_cap)
        if key not in self.want:  # computed once, shared, never changed
            r = R.tx_encode_tso_host(self.t, self.pay, self.mss, cap, out_cap, slot, flags,
                                     fill=T.CANARY, fill_entries=0xFFFFFFFF)
            for a in r[:5] + (r[6],):
                a.setflags(write=False)
            self.want[key] = r
        return self.want[key]

    def run(self, ctx, slot, hint, flags=0, cap=None, out_cap=None, mss=None):
        torch, dev = self.torch, self.dev
        cap, out_cap = self.sizes(slot, cap, out_cap)
        full = lambda n, dt: torch.full((max(n, 1),), -1, dtype=dt, device=dev)  # noqa: E731
        d_pk = torch.full((cap,), T.CANARY, dtype=torch.uint8, device=dev)
        d_off, d_len = full(out_cap, torch.int32), full(out_cap, torch.int16)
        d_first, d_nseg, d_tot = full(self.n, torch.int32), full(self.n, torch.int32), full(8, torch.int32)
        ctx.tx_encode_tso_dev(self.d_txd, self.n, self.d_pay, self.mss if mss is None else mss, d_pk,
                              cap, slot, d_off, d_len, out_cap, d_first, d_nseg, hint, flags, d_tot,
                              torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        u32 = lambda x, n: x.cpu().numpy().view(np.uint32)[:n]  # noqa: E731
        return (d_pk, u32(d_off, out_cap), d_len.cpu().numpy().view(np.uint16)[:out_cap],
                u32(d_first, self.n), u32(d_nseg, self.n), u32(d_tot, 8), d_off, d_len)

    def check(self, ctx, slot, hint, flags=0, cap=None, out_cap=None, tag=None):
        d_pk, off, ln, first, nseg, tot, _, _ = self.run(ctx, slot, hint, flags, cap, out_cap)
        w_pk, w_off, w_ln, w_first, w_nseg, _, w_tot, _ = self.host(slot, flags, cap, out_cap)
        assert list(tot) == list(w_tot), tag
        assert np.array_equal(first, w_first) and np.array_equal(nseg, w_nseg), tag
        assert np.array_equal(off, w_off) and np.array_equal(ln, w_ln), tag
        got = d_pk.cpu().numpy()
        if not np.array_equal(got, w_pk):  # whole buffer: gaps between slots, past the span
            bad = np.flatnonzero(got != w_pk)
            live = np.flatnonzero((w_ln != 0) & (w_ln != 0xFFFF))
            at = w_off[live].astype(np.int64) * 64
            e = live[int(np.searchsorted(at, bad[0], side="right")) - 1] if len(live) else -1
            pytest.fail(f"{tag}: {len(bad)} bytes differ, first at {bad[0]} (entry ~{e}, len "
                        f"{w_ln[e]}, frame offset {bad[0] - int(w_off[e]) * 64})")
        return d_pk


def _many():
    """more descriptors than one layout chunk (4096) and many tiles: the mix's
    descriptors three times over (they may share payloads), cut at 512"""
    t, pay = T.burst(T.mix_descs())
    return np.concatenate([t, t, t, t[:200]]), pay


@pytest.fixture(scope="module")
def bursts():
    torch, dev = _dev()
    b = {mss: Burst(*TT.burst(mss, mss == 1460), mss, dev, torch) for mss in (20, 1460, 8948)}
    b["many"] = Burst(*_many(), 512, dev, torch)
    return b


@pytest.mark.gpu
def test_device_form_matches_host_restatement(bursts):
    _dev()
    with R.Context(0) as ctx:
        runs = [(h, None) for h in HINTS] + [(1500, v) for v in range(N_VARIANTS)]
        try:
            for hint, v in runs:
                ctx.tune_txe(R.TX_AUTO if v is None else v)
                for mss in (20, 1460, 8948):
                    for slot in (0, SLOTS[mss]):
                        bursts[mss].check(ctx, slot, hint, tag=(mss, slot, hint, v))
            ctx.tune_txe(R.TX_AUTO)
            for hint in (64, 1500):
                for slot in (0, 1536):
                    bursts["many"].check(ctx, slot, hint, tag=("many", slot, hint))
            for mss, hint in ((20, 64), (1460, 1500), ("many", 354)):
                b = bursts[mss]
                slot = SLOTS[b.mss]
                b.check(ctx, 0, hint, flags=R.TXE_NO_CKSUM, tag=("no_cksum", mss))
                # cap_bytes, then out_cap, run out in the middle of a descriptor's segments
                k = int(np.flatnonzero(b.host(0)[4] >= 3)[-1])
                e, byt = R.tx_tso_count(b.t[:k], b.mss)
                for cut in (1, 2):
                    b.check(ctx, 0, hint, cap=byt + cut * 64, tag=("cap", mss, cut))
                    b.check(ctx, 0, hint, out_cap=e + cut, tag=("out_cap", mss, cut))
                    b.check(ctx, slot, hint, out_cap=e + cut, tag=("out_cap slots", mss, cut))
                b.check(ctx, slot, hint, cap=(e + 2) * slot + 100, tag=("cap slots", mss))
                b.check(ctx, 0, hint, out_cap=0, tag=("out_cap 0", mss))
        finally:
            ctx.tune_txe(R.TX_AUTO)
        # bad arguments are refused before anything runs
        b = bursts[20]
        for kw in (dict(slot=100, hint=64), dict(slot=0, hint=64, mss=18)):
            with pytest.raises(R.RxgError) as e:
                b.run(ctx, **kw)
            assert e.value.rc == EINVAL


@pytest.mark.gpu
def test_special_case_is_rxg_tx_encode_dev():
    """mss == 0, or every TCP payload <= mss: the existing call's tensors"""
    torch, dev = _dev()
    t, pay = T.burst(T.mix_descs()[:257])
    n = len(t)
    with R.Context(0) as ctx:
        for slot, hint in ((0, 354), (1536, 1500)):
            b = Burst(t, pay, 0, dev, torch)
            cap, out_cap = b.sizes(slot)
            d_pk = torch.full((cap,), T.CANARY, dtype=torch.uint8, device=dev)
            d_off = torch.full((n,), -1, dtype=torch.int32, device=dev)
            d_len = torch.full((n,), -1, dtype=torch.int16, device=dev)
            d_tot = torch.full((4,), -1, dtype=torch.int32, device=dev)
            ctx.tx_encode_dev(b.d_txd, n, b.d_pay, d_pk, cap, slot, d_off, d_len, hint, 0, d_tot,
                              torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize(dev)
            for mss in (0, 1460):
                g_pk, off, ln, first, nseg, tot, g_off, g_len = b.run(ctx, slot, hint, mss=mss)
                assert torch.equal(g_pk, d_pk)
                assert torch.equal(g_off[:n], d_off) and torch.equal(g_len[:n], d_len)
                assert (g_off[n:] == -1).all() and (g_len[n:] == -1).all()
                assert list(tot[:4]) == list(d_tot.cpu().numpy().view(np.uint32))
                assert list(tot[4:]) == [n, 0, 0, 0]
                assert np.array_equal(first, np.arange(n)) and np.array_equal(nseg, ln[:n] != 0)


@pytest.mark.gpu
def test_host_form(bursts):
    _dev()
    with R.Context(0) as ctx:
        for mss in (20, 1460, 8948):
            b = bursts[mss]
            for t, want_rc in ((b.t, ERANGE), (b.t[b.t["kind"] <= R.TXD_ARP], 0)):
                ent, byt = R.tx_tso_count(t, mss)
                w = R.tx_encode_tso_host(t, b.pay, mss, byt, ent)
                pk, off, ln, first, nseg, rc = ctx.tx_encode_tso(t, b.pay, mss, byt, ent)
                assert rc == want_rc == w[7] and len(pk) == w[5] == byt
                assert np.array_equal(pk, w[0])
                assert np.array_equal(off, w[1]) and np.array_equal(ln, w[2])
                assert np.array_equal(first, w[3]) and np.array_equal(nseg, w[4])
        # out_cap ends the burst early: RXG_ERANGE, the rest is written
        b = bursts[1460]
        t = b.t[b.t["kind"] <= R.TXD_ARP]
        ent, byt = R.tx_tso_count(t, 1460)
        w = R.tx_encode_tso_host(t, b.pay, 1460, byt, ent - 1)
        pk, off, ln, first, nseg, rc = ctx.tx_encode_tso(t, b.pay, 1460, byt, ent - 1)
        assert rc == ERANGE and nseg[-1] == 0 and len(pk) == w[5] < byt
        assert np.array_equal(pk, w[0][:len(pk)])
        assert np.array_equal(off, w[1]) and np.array_equal(ln, w[2])
        assert np.array_equal(first, w[3]) and np.array_equal(nseg, w[4])
        for kw in (dict(mss=1462), dict(payload=b.pay[:-1])):  # a bad mss; a payload cut short
            with pytest.raises(R.RxgError) as e:
                ctx.tx_encode_tso(t, kw.get("payload", b.pay), kw.get("mss", 1460), byt, ent)
            assert e.value.rc == EINVAL


@pytest.mark.gpu
def test_round_trip_through_classify_and_k2():
    """three 10-KB sends cut at 1460 on the receiving side: every checksum
    verifies (K1), every segment finds its connection, the payload windows in
    entry order are the payloads sent, and K2 finds nothing to change"""
    torch, dev = _dev()
    ds = [T.txd(R.TXD_TCP, 10000 + i, optlen=(0, 3, 10)[i], seq=0xFFFFF000 + i, ack=77 + i,
                tcp_flags=0x18, window=1000 + i, hdrlen_off=0x50 + ((0, 3, 10)[i] << 4 & 0xF0),
                sip=T.L_IP, dip=f"10.1.2.{3 + i}", sport=4000 + i, dport=80 + i) for i in range(3)]
    t, pay = T.burst(ds)
    b = Burst(t, pay, 1460, dev, torch)
    tcb = np.zeros(3, R.TCB_DTYPE)
    for k in ("sip", "dip", "sport", "dport"):
        tcb[k] = t[k]
    tcb["status"] = R.TCP_STATUS_ESTABLISHED
    with R.Context(0) as ctx:
        d_pk = b.check(ctx, 0, 1500, tag="round trip")
        w_pk, w_off, w_ln, w_first, w_nseg = b.host(0)[:5]
        ne = b.ent
        assert ne == 21 and list(w_nseg) == [7, 7, 7]
        d_off = torch.from_numpy(w_off[:ne].view(np.int32).copy()).to(dev)
        d_len = torch.from_numpy(w_ln[:ne].view(np.int16).copy()).to(dev)
        ctx.flows_sync(np.zeros(0, R.UDP_SOCK_DTYPE), tcb)
        out = torch.empty(ne * 16, dtype=torch.uint8, device=dev)
        ctx.classify_dev(d_pk, d_off, d_len, ne, 6, 1500, out)
        torch.cuda.synchronize(dev)
        v = out.cpu().numpy().view(R.VERDICT_DTYPE)
        want = O.Tables(np.zeros(0, R.UDP_SOCK_DTYPE), tcb).classify(w_pk, w_off[:ne], w_ln[:ne], 6)
        assert v.tobytes() == want.tobytes()
        assert (v["cls"] == R.CLS_TCP).all() and (v["cksum_ok"] == 1).all()
        assert (v["flow_id"] != R.FLOW_NONE).all()
        got = d_pk.cpu().numpy()
        for k in range(3):
            es = range(int(w_first[k]), int(w_first[k]) + 7)
            assert len({int(v["flow_id"][e]) for e in es}) == 1
            win = [got[int(w_off[e]) * 64 + int(v["payload_off"][e]):][:int(v["payload_len"][e])]
                   for e in es]
            o = int(t[k]["pay_off16"]) * 16
            assert np.concatenate(win).tobytes() == pay[o:o + int(t[k]["pay_len"])].tobytes()
        assert len(set(v["flow_id"].tolist())) == 3
        before = d_pk.clone()
        ctx.tx_cksum_dev(d_pk, d_off, d_len, ne, 6, 1500, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert torch.equal(d_pk, before)


# ---- the socket layer's TX pass with an MSS ------------------------------------
L, LMAC, PMAC = T.L_IP, F.LOCAL_MAC, F.PEER_MAC
SENDS = (8, 1460, 1461, 20000)


def _scenario(encode):
    """an accepted connection with sends of 8, 1460, 1461 and 20000 bytes and a
    UDP datagram queued, set_tx_mss(1460), passes of at most 4 frames until the
    queues are empty"""
    ns = R.NStack(0)
    try:
        ns.set_local(L, LMAC)
        ns.set_tx_mss(1460)
        if encode:
            ns.set_tx_encode(True)
        for ip in ("10.0.0.1", "10.0.0.8"):
            ns.arp_insert(ip, PMAC)
        a = ns.socket(R.SOCK_DGRAM)
        ns.bind(a, L, 1000)
        ns.sendto(a, b"datagram", "10.0.0.1", 7777)
        lfd = ns.socket(R.SOCK_STREAM)
        ns.bind(lfd, L, 9999)
        ns.listen(lfd)
        ns.tcb_add("10.0.0.8", L, 40001, 9999)
        cfd, _ = ns.accept(lfd)
        rng = np.random.default_rng(9)
        data = [bytes(rng.integers(0, 256, n, np.uint8)) for n in SENDS]
        for d in data:
            assert ns.send(cfd, d) == len(d)
        passes = []
        for _ in range(12):
            fr = ns.tx_burst(max_frames=4, cksum=True)
            passes.append(fr)
            if not fr:
                break
        return passes, ns.stat(13), ns.stat(14), data
    finally:
        ns.fini()


def _rebase(frame, delta):
    """a TCP frame with its sequence number moved by delta and both checksums
    refilled by the oracle (the ISN is seeded from the clock, tcp.c:30-31)"""
    f = bytearray(frame)
    if delta and f[12:14] == b"\x08\x00" and f[23] == 6:
        f[38:42] = struct.pack(">I", (struct.unpack(">I", f[38:42])[0] + delta) & 0xFFFFFFFF)
        f[24:26] = f[50:52] = b"\0\0"
        buf, off, ln = F.pack_frames([bytes(f)], 6)
        return O.tx_cksum(buf, off, ln, 6)[:len(f)].tobytes()
    return frame


@pytest.mark.gpu
def test_nstack_tx_burst_with_mss():
    _dev()
    enc, n_enc, tso_enc, data = _scenario(True)
    host, n_host, tso_host, _ = _scenario(False)
    assert enc[-1] == [] and host[-1] == [] and len(enc) == len(host)
    tcp = [f for p in enc for f in p if f[23] == 6]
    assert [len(f) - 54 for f in tcp] == [8, 1460, 1460, 1] + [1460] * 13 + [1020]
    assert b"".join(f[54:] for f in tcp) == b"".join(data)
    # 1461: PSH on its second frame only; 20000: passes of 4, 4, 4 and 2 frames
    assert [f[47] for f in tcp[:4]] == [0x18, 0x18, 0x10, 0x18]
    assert [f[47] for f in tcp[4:]] == [0x10] * 13 + [0x18]
    assert [len(p) for p in enc] == [2, 1, 2, 4, 4, 4, 2, 0]
    seq = lambda f: struct.unpack(">I", f[38:42])[0]  # noqa: E731
    assert [(seq(f) - seq(tcp[4])) & 0xFFFFFFFF for f in tcp[4:]] == [1460 * j for j in range(14)]
    assert seq(tcp[3]) == (seq(tcp[2]) + 1460) & 0xFFFFFFFF
    # the two stacks drew their ISNs from clocks that may differ by a second:
    # the host-framed frames are moved onto the encoder stack's sequence numbers
    delta = seq(tcp[0]) - seq(next(f for p in host for f in p if f[23] == 6))
    for pe, ph in zip(enc, host):
        assert pe == [_rebase(f, delta) for f in ph]
    assert n_enc == sum(map(len, enc)) and n_host == 0
    assert tso_enc == tso_host == 5  # 1461 once, 20000 in four passes
