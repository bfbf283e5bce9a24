"""IPv4 fragmentation in the TX encoder on the GPU (csrc/tx_encode.hip: the
layout pass with both cuts, tx_encode_frag_kernel and txe_frag_finish_kernel):
the device form against the host restatement (rxg_tx_encode_frag_host, itself
pinned to the model of frag_ref.py by test_tx_frag.py) bit-exact on whole
0xA5-prefilled buffers, off / len prefilled with -1, for every MTU of the
boundary burst with the 65507-B datagram (1365 fragments at mtu 68: one
datagram's partial sums come from many tiles and blocks), every variant of the
kernel's table, packed and in slots; the capacity cases, no-checksum, the
special case that equals rxg_tx_encode_tso_dev, the host-buffer form against
the model, the round trip of reassembled datagrams through K1, and the socket
layer's TX pass with nstack_set_tx_mtu, encoder on against host-framed."""
import struct

import numpy as np
import pytest

import frag_ref as FR
import frames as F
import oracle_bind as O
import rxgpu as R
import test_gpu_tx_tso as TG
import test_tx_tso as TT
import txenc_ref as T

ERANGE, EINVAL = -34, -22
N_VARIANTS = 15  # csrc/tx_encode.hip k_txe / k_txe_frag
SLOTS = {68: 128, 70: 192, 76: 128, 1500: 1536, 9000: 9088}
HINT = {68: 64, 70: 128, 76: 64, 1500: 1500, 9000: 9000}


def _dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")
    return torch, torch.device("cuda", 0)


class Burst:
    """descriptors + payloads on the device, and the host restatement's answers"""

    def __init__(self, t, pay, mss, mtu, dev, torch):
        self.torch, self.dev, self.t, self.pay, self.mss, self.mtu = torch, dev, t, pay, mss, mtu
        self.n = len(t)
        self.d_txd = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
        pad = np.zeros((len(pay) + 15) // 16 * 16 + 16, np.uint8)  # to the 16-B end
        pad[:len(pay)] = pay
        self.d_pay = torch.from_numpy(pad).to(dev)
        self.ent, self.bytes = R.tx_frag_count(t, mss, mtu)
        self.want = {}

    def sizes(self, slot, cap=None, out_cap=None):
        out_cap = self.ent + 5 if out_cap is None else out_cap
        if cap is None:
            cap = (self.ent * slot if slot else self.bytes) + 256
        return cap, out_cap

    def host(self, slot, flags=0, cap=None, out_cap=None):
        cap, out_cap = self.sizes(slot, cap, out_cap)
        key = (slot, flags, cap, out_cap)
        if key not in self.want:  # computed once, shared, never changed
            r = R.tx_encode_frag_host(self.t, self.pay, self.mss, self.mtu, cap, out_cap, slot, flags,
                                      fill=T.CANARY, fill_entries=0xFFFFFFFF)
            for a in r[:5] + (r[6],):
                a.setflags(write=False)
            self.want[key] = r
        return self.want[key]

    def run(self, ctx, slot, hint, flags=0, cap=None, out_cap=None, mtu=None, tso=False):
        torch, dev = self.torch, self.dev
        cap, out_cap = self.sizes(slot, cap, out_cap)
        full = lambda n, dt: torch.full((max(n, 1),), -1, dtype=dt, device=dev)  # noqa: E731
        d_pk = torch.full((cap,), T.CANARY, dtype=torch.uint8, device=dev)
        d_off, d_len = full(out_cap, torch.int32), full(out_cap, torch.int16)
        d_first, d_nseg, d_tot = full(self.n, torch.int32), full(self.n, torch.int32), full(8, torch.int32)
        st = torch.cuda.current_stream(dev).cuda_stream
        if tso:
            ctx.tx_encode_tso_dev(self.d_txd, self.n, self.d_pay, self.mss, d_pk, cap, slot, d_off,
                                  d_len, out_cap, d_first, d_nseg, hint, flags, d_tot, st)
        else:
            ctx.tx_encode_frag_dev(self.d_txd, self.n, self.d_pay, self.mss,
                                   self.mtu if mtu is None else mtu, d_pk, cap, slot, d_off, d_len,
                                   out_cap, d_first, d_nseg, hint, flags, d_tot, st)
        torch.cuda.synchronize(dev)
        u32 = lambda x, n: x.cpu().numpy().view(np.uint32)[:n]  # noqa: E731
        return (d_pk, u32(d_off, out_cap), d_len.cpu().numpy().view(np.uint16)[:out_cap],
                u32(d_first, self.n), u32(d_nseg, self.n), u32(d_tot, 8))

    def check(self, ctx, slot, hint, flags=0, cap=None, out_cap=None, tag=None):
        d_pk, off, ln, first, nseg, tot = self.run(ctx, slot, hint, flags, cap, out_cap)
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


_B = {}


def _burst(mtu):
    torch, dev = _dev()
    if mtu not in _B:
        _B[mtu] = Burst(*FR.burst(mtu, True), FR.MSS_OF[mtu], mtu, dev, torch)
    return _B[mtu]


@pytest.mark.gpu
@pytest.mark.parametrize("mtu", FR.MTUS)
def test_device_form_matches_host_restatement(mtu):
    b = _burst(mtu)
    assert int(b.host(0)[4].max()) == -(-65515 // FR.fp_of(mtu))  # the 65507-B datagram is there
    with R.Context(0) as ctx:
        try:
            for v in [None] + list(range(N_VARIANTS)):
                ctx.tune_txe(R.TX_AUTO if v is None else v)
                for slot in (0, SLOTS[mtu]):
                    b.check(ctx, slot, HINT[mtu], tag=(mtu, slot, v))
        finally:
            ctx.tune_txe(R.TX_AUTO)


@pytest.mark.gpu
def test_rules_on_the_device():
    torch, dev = _dev()
    with R.Context(0) as ctx:
        for mtu in (76, 1500):
            b = _burst(mtu)
            slot, hint = SLOTS[mtu], HINT[mtu]
            b.check(ctx, 0, hint, flags=R.TXE_NO_CKSUM, tag=("no_cksum", mtu))
            b.check(ctx, slot, hint, flags=R.TXE_NO_CKSUM, tag=("no_cksum slots", mtu))
            # cap_bytes, then out_cap, run out in the middle of a datagram's fragments
            cutd = np.array([FR.is_cut(d, mtu) for d in b.t])
            k = int(np.flatnonzero(cutd & (b.host(0)[4] >= 3))[-1])
            e, byt = R.tx_frag_count(b.t[:k], b.mss, mtu)
            for cut in (1, 2):
                b.check(ctx, 0, hint, cap=byt + cut * 64, tag=("cap", mtu, cut))
                b.check(ctx, 0, hint, out_cap=e + cut, tag=("out_cap", mtu, cut))
                b.check(ctx, slot, hint, out_cap=e + cut, tag=("out_cap slots", mtu, cut))
            b.check(ctx, slot, hint, cap=(e + 2) * slot + 100, tag=("cap slots", mtu))
            b.check(ctx, 0, hint, out_cap=0, tag=("out_cap 0", mtu))
        # a skipped datagram at the head: off == 0 for its entries, and bytes 40-41 of
        # d_pkts, where the finish step would put a checksum, keep the canary
        t, pay = T.burst([T.txd(R.TXD_UDP, 4000, seq=7), T.txd(R.TXD_UDP, 3000, seq=8)])
        b = Burst(t, pay, 0, 1500, dev, torch)
        for kw in (dict(cap=2 * 1536 + 1087), dict(out_cap=2), dict(cap=64), dict(out_cap=0)):
            for slot in (0, 1536):
                d_pk = b.check(ctx, slot, 1500, tag=("head", kw, slot), **kw)
                if len(d_pk) >= 42:
                    assert d_pk[:64].cpu().numpy().tolist() == [T.CANARY] * 64
        # bad arguments are refused before anything runs
        for kw in (dict(slot=100, hint=64), dict(slot=0, hint=64, mtu=67),
                   dict(slot=0, hint=64, mtu=65536)):
            with pytest.raises(R.RxgError) as e:
                b.run(ctx, **kw)
            assert e.value.rc == EINVAL


@pytest.mark.gpu
def test_mtu_0_is_rxg_tx_encode_tso_dev():
    torch, dev = _dev()
    with R.Context(0) as ctx:
        for mss in (20, 1460):
            b = Burst(*TT.burst(mss, mss == 1460), mss, 0, dev, torch)
            for slot, hint in ((0, 354), (TG.SLOTS[mss], 1500)):
                w = b.run(ctx, slot, hint, tso=True)
                g = b.run(ctx, slot, hint)
                assert torch.equal(g[0], w[0])
                for x, y in zip(g[1:], w[1:]):
                    assert np.array_equal(x, y)


@pytest.mark.gpu
def test_host_form_against_the_model():
    _dev()
    with R.Context(0) as ctx:
        for mtu in (76, 1500):
            t, pay = FR.burst(mtu, True)
            mss = FR.MSS_OF[mtu]
            for tt, want_rc in ((t, ERANGE), (t[(t["kind"] <= R.TXD_ARP) & (t["pay_len"] <= 65507)], 0)):
                ent, byt = FR.sizes(tt, pay, mss, mtu)
                w = FR.reference(tt, pay, mss, mtu, byt, ent)
                pk, off, ln, first, nseg, rc = ctx.tx_encode_frag(tt, pay, mss, mtu, byt, ent)
                assert rc == want_rc and len(pk) == w[5] == byt
                assert np.array_equal(pk, w[0])
                assert np.array_equal(off, w[1]) and np.array_equal(ln, w[2])
                assert np.array_equal(first, w[3]) and np.array_equal(nseg, w[4])
        for kw in (dict(mtu=67), dict(payload=pay[:-1])):  # a bad mtu; a payload cut short
            with pytest.raises(R.RxgError) as e:
                ctx.tx_encode_frag(t, kw.get("payload", pay), mss, kw.get("mtu", mtu), byt, ent)
            assert e.value.rc == EINVAL


@pytest.mark.gpu
def test_round_trip_through_classify():
    """4000-B and 8000-B datagrams cut at 1500, reassembled here into one frame
    each: K1 finds a UDP datagram whose checksum verifies and whose payload
    window is the data sent"""
    torch, dev = _dev()
    ds = [T.txd(R.TXD_UDP, n, sip="10.0.0.1", dip=T.L_IP, sport=5555, dport=20005, seq=0x77 + i)
          for i, n in enumerate((4000, 8000))]
    t, pay = T.burst(ds)
    b = Burst(t, pay, 0, 1500, dev, torch)
    udp = np.zeros(1, R.UDP_SOCK_DTYPE)
    udp[0]["localip"], udp[0]["localport"], udp[0]["protocol"] = R.ip_raw(T.L_IP), R.port_raw(20005), 17
    with R.Context(0) as ctx:
        d_pk = b.check(ctx, 0, 1500, tag="round trip")
        got = d_pk.cpu().numpy()
        _, w_off, w_ln, w_first, w_nseg = b.host(0)[:5]
        assert list(w_nseg) == [3, 6]
        whole = []
        for k in range(2):
            fr = [got[int(w_off[e]) * 64:int(w_off[e]) * 64 + int(w_ln[e])]
                  for e in range(w_first[k], w_first[k] + w_nseg[k])]
            dg = FR.reassemble(fr[::-1])
            f = bytearray(fr[0][:34].tobytes() + dg)
            f[16:18], f[18:22], f[24:26] = struct.pack(">H", 20 + len(dg)), bytes(4), bytes(2)
            f[24:26] = struct.pack(">H", ~FR.csum16(bytes(f[14:34])) & 0xFFFF)
            whole.append(bytes(f))
        buf, off, ln = F.pack_frames(whole, 6)
        ctx.flows_sync(udp, np.zeros(0, R.TCB_DTYPE))
        out = torch.empty(2 * 16, dtype=torch.uint8, device=dev)
        pad = np.zeros(len(buf) + 64, np.uint8)
        pad[:len(buf)] = buf
        ctx.classify_dev(torch.from_numpy(pad).to(dev), torch.from_numpy(off.view(np.int32).copy()).to(dev),
                         torch.from_numpy(ln.view(np.int16).copy()).to(dev), 2, 6, 9000, out)
        torch.cuda.synchronize(dev)
        v = out.cpu().numpy().view(R.VERDICT_DTYPE)
        want =O.Tables(udp, np.zeros(0, R.TCB_DTYPE)).classify(buf, off, ln, 6)
        assert v.tobytes() == want.tobytes()
        assert (v["cls"] == R.CLS_UDP).all() and (v["cksum_ok"] == 1).all() and (v["rc"] == R.RC_OK).all()
        for k in range(2):
            o = int(t[k]["pay_off16"]) * 16
            at = int(off[k]) * 64 + int(v["payload_off"][k])
            assert buf[at:at + int(v["payload_len"][k])].tobytes() == \
                pay[o:o + int(t[k]["pay_len"])].tobytes()


# ---- the socket layer's TX pass with an MTU --------------------------------------
L, LMAC, PMAC = T.L_IP, F.LOCAL_MAC, F.PEER_MAC
DGRAMS = (100, 1472, 1473, 4000, 65507)


def _scenario(encode):
    """a UDP socket with datagrams of 100, 1472, 1473, 4000 and 65507 bytes and
    an accepted connection with one 4000-B send, set_tx_mtu(1500) and
    set_tx_mss(1460), passes until the queues are empty"""
    ns = R.NStack(0)
    try:
        ns.set_local(L, LMAC)
        ns.set_tx_mtu(1500)
        ns.set_tx_mss(1460)
        if encode:
            ns.set_tx_encode(True)
        for ip in ("10.0.0.1", "10.0.0.8"):
            ns.arp_insert(ip, PMAC)
        a = ns.socket(R.SOCK_DGRAM)
        ns.bind(a, L, 1000)
        rng = np.random.default_rng(9)
        data = [bytes(rng.integers(0, 256, n, np.uint8)) for n in DGRAMS + (4000,)]
        for d in data[:-1]:
            ns.sendto(a, d, "10.0.0.1", 7777)
        lfd = ns.socket(R.SOCK_STREAM)
        ns.bind(lfd, L, 9999)
        ns.listen(lfd)
        ns.tcb_add("10.0.0.8", L, 40001, 9999)
        cfd, _ = ns.accept(lfd)
        assert ns.send(cfd, data[-1]) == 4000
        passes = []
        for _ in range(8):
            fr = ns.tx_burst(max_frames=64, cap_bytes=1 << 17, cksum=True)
            passes.append(fr)
            if not fr:
                break
        return passes, ns.stat(13), ns.stat(25), data
    finally:
        ns.fini()


@pytest.mark.gpu
def test_nstack_tx_burst_with_mtu():
    _dev()
    enc, n_enc, cut_enc, data = _scenario(True)
    host, n_host, cut_host, _ = _scenario(False)
    assert enc[-1] == [] and host[-1] == [] and len(enc) == len(host)
    udp = [[f for f in p if f[23] == 17] for p in enc]
    assert [len(p) for p in udp] == [1, 1, 2, 3, 45, 0]  # one datagram per socket and pass
    for p, d in zip(udp[:5], data[:5]):
        dg = FR.reassemble(p) if len(p) > 1 else p[0][34:]
        assert dg[8:] == d
        # the checksum of the whole datagram verifies against the pseudo-header
        ph = p[0][26:34] + struct.pack(">BBH", 0, 17, len(dg))
        assert FR.csum16(ph + dg) == 0xFFFF
        assert all(FR.csum16(f[14:34]) == 0xFFFF for f in p)
    assert [struct.unpack(">H", p[0][18:20])[0] for p in udp[:5]] == [0, 0, 1, 2, 3]
    tcp = [f for p in enc for f in p if f[23] == 6]
    assert [len(f) - 54 for f in tcp] == [1460, 1460, 1080]
    seq = lambda f: struct.unpack(">I", f[38:42])[0]  # noqa: E731
    delta = seq(tcp[0]) - seq(next(f for p in host for f in p if f[23] == 6))
    for pe, ph in zip(enc, host):
        assert pe == [TG._rebase(f, delta) for f in ph]
    assert n_enc == sum(map(len, enc)) and n_host == 0
    assert cut_enc == cut_host == 3
