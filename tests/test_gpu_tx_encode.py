"""TX encode on the GPU (K5, csrc/tx_encode.hip): the device form against the
host encoder (rxg_tx_encode_host, itself pinned to the reference's encoders by
test_tx_encode.py) bit-exact on whole 0xA5-prefilled buffers, every len_hint
class and every variant of the kernel's table, packed and in slots; the host
form; the round trip through K1 (every checksum verifies, every flow is found)
and K2 (nothing left to fix); and the socket layer's TX pass with the encoder
on against the host-framed pass."""
import struct

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxgpu as R
import txenc_ref as T

ERANGE = -34
HINTS = (64, 128, 354, 1500, 9000)
N_VARIANTS = 15  # csrc/tx_encode.hip k_txe


def _dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")
    return torch, torch.device("cuda", 0)


class Burst:
    """descriptors + payloads on the device, and the host encoder's answers"""

    def __init__(self, descs, dev, torch):
        self.torch, self.dev = torch, dev
        self.t, self.pay = T.burst(descs)
        self.n = len(self.t)
        self.d_txd = torch.from_numpy(self.t.view(np.uint8).copy()).to(dev)
        pad = np.zeros((len(self.pay) + 15) // 16 * 16 + 16, np.uint8)  # to the 16-B end
        pad[:len(self.pay)] = self.pay
        self.d_pay = torch.from_numpy(pad).to(dev)
        self.want = {}

    def cap(self, slot):
        if slot:
            return self.n * slot
        return sum((T.frame_len(d) + 63) // 64 * 64 for d in self.t) + 256

    def host(self, slot, flags=0, cap=None):
        key = (slot, flags, cap)
        if key not in self.want:  # computed once, shared, never changed
            pk, off, ln, span, tot, rc = R.tx_encode_host(self.t, self.pay, cap or self.cap(slot), slot,
                                                          flags, fill=T.CANARY)
            for a in (pk, off, ln, tot):
                a.setflags(write=False)
            self.want[key] = (pk, off, ln, tot)
        return self.want[key]

    def run(self, ctx, slot, hint, flags=0, cap=None):
        torch, dev = self.torch, self.dev
        cap = cap or self.cap(slot)
        d_pk = torch.full((cap,), T.CANARY, dtype=torch.uint8, device=dev)
        d_off = torch.full((self.n,), -1, dtype=torch.int32, device=dev)
        d_len = torch.full((self.n,), -1, dtype=torch.int16, device=dev)
        d_tot = torch.full((4,), -1, dtype=torch.int32, device=dev)
        ctx.tx_encode_dev(self.d_txd, self.n, self.d_pay, d_pk, cap, slot, d_off, d_len, hint, flags,
                          d_tot, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        return (d_pk, d_off.cpu().numpy().view(np.uint32), d_len.cpu().numpy().view(np.uint16),
                d_tot.cpu().numpy().view(np.uint32))

    def check(self, ctx, slot, hint, flags=0, cap=None, tag=None):
        d_pk, off, ln, tot = self.run(ctx, slot, hint, flags, cap)
        w_pk, w_off, w_ln, w_tot = self.host(slot, flags, cap)
        assert list(tot) == list(w_tot), tag
        assert np.array_equal(off, w_off) and np.array_equal(ln, w_ln), tag
        got = d_pk.cpu().numpy()
        if not np.array_equal(got, w_pk):  # whole buffer: gaps between slots, past the span
            bad = np.flatnonzero(got != w_pk)
            k = int(np.searchsorted(w_off.astype(np.int64) * 64, bad[0], side="right")) - 1
            pytest.fail(f"{tag}: {len(bad)} bytes differ, first at {bad[0]} (descriptor ~{k}, "
                        f"len {w_ln[k]}, frame offset {bad[0] - int(w_off[k]) * 64})")
        return d_pk


@pytest.fixture(scope="module")
def bursts():
    torch, dev = _dev()
    mix = T.mix_descs()
    b = {"boundary": Burst(T.boundary_descs(), dev, torch), "mix": Burst(mix, dev, torch),
         "skips": Burst(T.skip_descs(), dev, torch)}
    for n in (1, 63, 64, 65, 257):
        b[n] = Burst(mix[:n], dev, torch)
    return b


@pytest.mark.gpu
def test_device_form_matches_host_encoder(bursts):
    _dev()
    with R.Context(0) as ctx:
        with pytest.raises(R.RxgError):
            ctx.tune_txe(N_VARIANTS)  # one past the table
        ctx.tune_txe(N_VARIANTS - 1)
        ctx.tune_txe(R.TX_AUTO)
        runs = [(h, None) for h in HINTS] + [(1500, v) for v in range(N_VARIANTS)]
        try:
            for hint, v in runs:
                ctx.tune_txe(R.TX_AUTO if v is None else v)
                for name, slot in (("boundary", 0), ("boundary", 65536), ("mix", 0), ("mix", 1536),
                                   ("skips", 0), ("skips", 1536), (1, 0), (63, 0), (64, 64), (65, 0),
                                   (257, 0), (257, 1536)):
                    bursts[name].check(ctx, slot, hint, tag=(name, slot, hint, v))
            ctx.tune_txe(R.TX_AUTO)
            for hint in (64, 1500):
                bursts["mix"].check(ctx, 0, hint, flags=R.TXE_NO_CKSUM, tag=("no_cksum", hint))
                # cap_bytes exhausted mid-burst, packed and in slots
                bursts["mix"].check(ctx, 0, hint, cap=100 * 1024 + 64, tag=("cap", hint))
                bursts["mix"].check(ctx, 1536, hint, cap=100 * 1536 + 512, tag=("cap slots", hint))
        finally:
            ctx.tune_txe(R.TX_AUTO)
        # bad arguments are refused before anything runs
        b = bursts[1]
        with pytest.raises(R.RxgError) as e:
            b.run(ctx, 100, 64, cap=4096)
        assert e.value.rc == -22


@pytest.mark.gpu
def test_host_form(bursts):
    _dev()
    with R.Context(0) as ctx:
        for name in ("boundary", "mix", 65):
            b = bursts[name]
            w_pk, w_off, w_ln, w_tot = b.host(0)
            span = int(w_tot[1]) | int(w_tot[2]) << 32
            pk, off, ln, rc = ctx.tx_encode(b.t, b.pay, b.cap(0))
            assert rc == 0 and len(pk) == span
            assert np.array_equal(pk, w_pk[:span])
            assert np.array_equal(off, w_off) and np.array_equal(ln, w_ln)
        b = bursts["skips"]
        w_pk, w_off, w_ln, w_tot = b.host(0)
        pk, off, ln, rc = ctx.tx_encode(b.t, b.pay, b.cap(0))
        assert rc == ERANGE  # something was skipped; the rest is written
        assert np.array_equal(pk, w_pk[:len(pk)]) and len(pk) == int(w_tot[1])
        assert np.array_equal(off, w_off) and np.array_equal(ln, w_ln)
        # a payload that ends past the payload buffer
        t, pay = T.burst([T.txd(R.TXD_UDP, 5)])
        with pytest.raises(R.RxgError) as e:
            ctx.tx_encode(t, pay[:-1], 4096)
        assert e.value.rc == -22


@pytest.mark.gpu
def test_round_trip_through_classify_and_k2(bursts):
    """the encoder's frames on the receiving side: every UDP/TCP checksum
    verifies (K1), every frame finds its flow, and K2 finds nothing to change"""
    torch, dev = _dev()
    b = bursts["mix"]
    t = b.t
    isu, ist = t["kind"] == R.TXD_UDP, t["kind"] == R.TXD_TCP
    udp = np.zeros(int(isu.sum()), R.UDP_SOCK_DTYPE)
    udp["localip"], udp["localport"], udp["protocol"] = t["dip"][isu], t["dport"][isu], 17
    tcb = np.zeros(int(ist.sum()), R.TCB_DTYPE)
    for k in ("sip", "dip", "sport", "dport"):
        tcb[k] = t[k][ist]
    tcb["status"] = R.TCP_STATUS_ESTABLISHED
    with R.Context(0) as ctx:
        d_pk = b.check(ctx, 0, 354, tag="mix for the round trip")
        _, w_off, w_ln, _ = b.host(0)
        d_off = torch.from_numpy(w_off.view(np.int32).copy()).to(dev)
        d_len = torch.from_numpy(w_ln.view(np.int16).copy()).to(dev)
        ctx.flows_sync(udp, tcb)
        out = torch.empty(b.n * 16, dtype=torch.uint8, device=dev)
        ctx.classify_dev(d_pk, d_off, d_len, b.n, 6, 354, out)
        torch.cuda.synchronize(dev)
        v = out.cpu().numpy().view(R.VERDICT_DTYPE)
        want = O.Tables(udp, tcb).classify(b.host(0)[0], w_off, w_ln, 6)
        assert v.tobytes() == want.tobytes()
        l4 = isu | ist
        assert (v["cls"][isu] == R.CLS_UDP).all() and (v["cls"][ist] == R.CLS_TCP).all()
        assert (v["cksum_ok"][l4] == 1).all()
        assert (v["flow_id"][l4] != R.FLOW_NONE).all()
        # every key is its own flow: the ids are all different
        assert len(np.unique(v["flow_id"][isu])) == int(isu.sum())
        assert len(np.unique(v["flow_id"][ist])) == int(ist.sum())
        before = d_pk.clone()
        ctx.tx_cksum_dev(d_pk, d_off, d_len, b.n, 6, 354, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert torch.equal(d_pk, before)


# ---- the socket layer's TX pass with the encoder on ---------------------------
L, LMAC, PMAC = T.L_IP, F.LOCAL_MAC, F.PEER_MAC


def _scenario(encode):
    """two UDP sockets with queued datagrams (one destination without an ARP
    entry), a listener that has received a SYN, an accepted connection with
    queued data: every TX pass until the queues are empty"""
    ns = R.NStack(0)
    try:
        ns.set_local(L, LMAC)
        if encode:
            ns.set_tx_encode(True)
        for ip in ("10.0.0.1", "10.0.0.8", "10.0.0.9"):
            ns.arp_insert(ip, PMAC)
        a, b = ns.socket(R.SOCK_DGRAM), ns.socket(R.SOCK_DGRAM)
        ns.bind(a, L, 1000)
        ns.bind(b, L, 2000)
        ns.sendto(a, bytes(range(256)) * 5 + b"tail", "10.0.0.1", 7777)
        ns.sendto(a, b"a2", "10.0.0.1", 7777)
        ns.sendto(a, b"", "10.0.0.1", 7778)
        ns.sendto(b, b"to a stranger", "10.0.0.2", 9)  # no ARP entry: a request first
        ns.sendto(b, b"b2" * 11, "10.0.0.1", 7777)     # a 64-B frame
        lfd = ns.socket(R.SOCK_STREAM)
        ns.bind(lfd, L, 9999)
        ns.listen(lfd)
        ns.tcb_add("10.0.0.8", L, 40001, 9999)
        cfd, _ = ns.accept(lfd)
        assert ns.send(cfd, b"hi there") == 8
        assert ns.send(cfd, b"x" * 1446) == 1446
        r, rcs, _ = ns.rx_burst([F.tcp_frame("10.0.0.9", 40000, L, 9999, b"", flags=0x02, seq=5000)])
        assert list(rcs) == [0]
        passes = []
        for k in range(8):
            fr = ns.tx_burst(cksum=True)
            passes.append(fr)
            if not fr:
                break
            if k == 0:  # the stranger answers the request
                ns.rx_burst([F.arp_frame("10.0.0.2", L)])
        return passes, ns.stat(13)
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
def test_nstack_tx_burst_with_encoder():
    _dev()
    enc, n_enc = _scenario(True)
    host, n_host = _scenario(False)
    assert enc[-1] == [] and host[-1] == [] and len(enc) == len(host) >= 4
    kinds = ["arp" if f[12:14] == b"\x08\x06" else f[23] for p in enc for f in p]
    assert kinds.count("arp") == 1 and kinds.count(17) == 5 and kinds.count(6) >= 3
    # the two stacks drew their ISNs from clocks that may differ by a second:
    # the host-framed frames are moved onto the encoder stack's sequence numbers
    syn = lambda ps: next(f for p in ps for f in p if f[23] == 6 and f[47] == 0x12)  # noqa: E731
    dat = lambda ps: next(f for p in ps for f in p if f[23] == 6 and f[47] == 0x18)  # noqa: E731
    seq = lambda f: struct.unpack(">I", f[38:42])[0]  # noqa: E731
    d_syn, d_dat = seq(syn(enc)) - seq(syn(host)), seq(dat(enc)) - seq(dat(host))
    for pe, ph in zip(enc, host):
        moved = [_rebase(f, d_syn if f[12:14] == b"\x08\x00" and f[23] == 6 and f[47] == 0x12 else d_dat)
                 for f in ph]
        assert pe == moved
    assert n_enc == sum(map(len, enc)) and n_host == 0
