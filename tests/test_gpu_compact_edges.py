"""K3 (csrc/rx_compact.hip, rxg_udp_compact_dev) at the sizes where its stages
change path (-m gpu): 1024-frame tiles, 64-lane ballot groups, the one-block
scan over sockets and tiles, the shifted-dword payload copy and its mask.

Every case compares d_dgram[:totals[0]], d_first, d_totals and the payload
bytes with the model of tests/compact_ref.py, exactly, and prefills d_dgram,
d_first and d_payload with canaries that must survive outside the used part.
The verdict array is an input of the call, so most cases forge it on the host
(no dependence on K1); one runs K1's own verdicts at 16-B descriptor units.
Frames lie back to back at 16-B boundaries with 0xEE between them, descriptor
order shuffled against memory order, so a byte taken from a neighbour shows."""
import numpy as np
import pytest

import compact_ref as CR
import frames as F
import oracle_bind as O
import rxgpu as R

pytestmark = pytest.mark.gpu
L = "192.168.100.77"
DG_CANARY, FIRST_CANARY, PL_CANARY = 0xA7, 0xB9, 0xCD


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (no fallback path exists)")
    return torch, torch.device("cuda", 0)


def _socks(n, base=30000):
    udp = np.zeros(n, R.UDP_SOCK_DTYPE)
    udp["localip"] = R.ip_raw(L)
    udp["localport"] = [R.port_raw(base + k) for k in range(n)]
    udp["protocol"] = 17
    return udp


@pytest.fixture(scope="module")
def ctxs(torch_dev):
    """one context per UDP id space, shared by the cases"""
    made = {}

    def get(nflows):
        if nflows not in made:
            made[nflows] = R.Context(0)
            made[nflows].flows_sync(_socks(nflows), None)
        return made[nflows]
    yield get
    for c in made.values():
        c.close()


_PAYLOAD = bytes(np.random.default_rng(99).integers(1, 256, 2048, dtype=np.uint8))


def _udp(k, size, data=None):
    """frame k of a burst: distinct source address and port (the record's sip
    and sport), `size` payload bytes, none of them zero"""
    pl = (data if data is not None else _PAYLOAD[k % 500:])[:size]
    return F.udp_frame(f"10.{1 + k % 200}.{1 + (k >> 8) % 200}.{1 + k % 251}", 1024 + k % 60000, L,
                       30000, pl)


def _forge(frames, flows, cls=R.CLS_UDP, rc=0):
    """verdicts as K1 writes them for delivered UDP frames: the socket id,
    payload_len = dgram_len - 8 read from the frame, payload_off 42"""
    v = np.zeros(len(frames), R.VERDICT_DTYPE)
    v["flow_id"], v["cls"], v["rc"], v["payload_off"] = flows, cls, rc, 42
    v["payload_len"] = [max(int.from_bytes(f[38:40], "big") - 8, 0) for f in frames]
    v["cksum_ok"] = 1
    return v


def _check(torch_dev, ctx, frames, caps, v, nflows, *, unit_log2=4, cap=None, seed=0, d_v=None):
    """run K3 on the burst and compare everything with the model; cap None =
    exactly the bytes needed.  Returns the model's result."""
    torch, dev = torch_dev
    n = len(frames)
    want = CR.compact(frames, caps, v, nflows, cap)
    need = int(want.totals[1])
    cap = need if cap is None else cap
    rng = np.random.default_rng(seed)
    buf, off, lens = F.pack_filled(frames or [bytes(64)], unit_log2, caplens=caps or [64],
                                   fill=0xEE, mem_order=rng.permutation(max(n, 1)))
    d_pk = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
    if d_v is None:
        d_v = torch.from_numpy(np.frombuffer(v.tobytes() + bytes(16), np.uint8).copy()).to(dev)
    d_dg = torch.full(((n + 8) * 16,), DG_CANARY, dtype=torch.uint8, device=dev)
    d_first = torch.full(((nflows + 1 + 8) * 4,), FIRST_CANARY, dtype=torch.uint8, device=dev)
    d_pl = torch.full((cap + 256,), PL_CANARY, dtype=torch.uint8, device=dev)
    d_tot = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    ctx.udp_compact_dev(d_pk, d_off, d_ln, n, unit_log2, d_v, d_dg, d_first, d_pl, cap, d_tot,
                        stream=sh)
    torch.cuda.synchronize(dev)
    tot = d_tot.cpu().numpy().view(np.uint32)
    assert list(tot) == list(want.totals), (list(tot), list(want.totals))
    nd = int(tot[0])
    dg = d_dg.cpu().numpy()
    got = dg[:nd * 16].view(R.DGRAM_DTYPE)
    bad = [r for r in range(nd) if got[r].tobytes() != want.dgram[r].tobytes()]
    assert not bad, [(r, got[r], want.dgram[r]) for r in bad[:5]]
    assert np.all(dg[nd * 16:] == DG_CANARY)
    first = d_first.cpu().numpy()
    assert np.array_equal(first[:(nflows + 1) * 4].view(np.uint32), want.first)
    assert np.all(first[(nflows + 1) * 4:] == FIRST_CANARY)
    # the payload buffer whole: written payloads, canary inside the ones that
    # did not fit, past the used bytes and at or past payload_cap
    exp = np.full(cap + 256, PL_CANARY, np.uint8)
    w = np.nonzero(want.written)[0]
    assert len(w) == 0 or w[-1] < cap
    exp[w] = want.payload[w]
    pl = d_pl.cpu().numpy()
    diff = np.nonzero(pl != exp)[0]
    assert len(diff) == 0, (len(diff), diff[:8], pl[diff[:8]], exp[diff[:8]])
    return want


# ---- tile and wave edges ---------------------------------------------------
N_EDGES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3 * 1024 + 17]
_SIZES = [0, 1, 5, 16, 17, 22, 47, 48, 100, 333]


@pytest.mark.parametrize("pattern", ["interleaved", "one_owner"])
@pytest.mark.parametrize("n", N_EDGES)
def test_tile_and_wave_edges(torch_dev, ctxs, n, pattern):
    """bursts ending at and next to a wave (64) and a tile (1024) edge; with
    one socket owning every frame, ranks and byte offsets run across all 16
    waves of a tile and across tiles"""
    nflows = 5
    frames = [_udp(k, _SIZES[(k * 7 + k // 64) % len(_SIZES)]) for k in range(n)]
    flows = [(k * 3 + k // 64) % nflows for k in range(n)] if pattern == "interleaved" else [3] * n
    caps = [len(f) for f in frames]
    want = _check(torch_dev, ctxs(nflows), frames, caps, _forge(frames, flows), nflows, seed=n)
    assert want.totals[0] == n
    if pattern == "one_owner":
        assert list(want.first) == [0, 0, 0, 0, n, n]


# ---- socket-count edges ----------------------------------------------------
def _socket_count_burst(nflows):
    """waves of: 64 frames to 64 different sockets (the longest ballot loop),
    32 + 32 frames to two sockets in alternating lanes, one socket, and the
    id space's first and last ids; 2 tiles and a partial wave"""
    flows = []
    for w in range(35):
        if w % 4 == 0:
            flows += [(w * 64 + k * 17) % nflows for k in range(64)] if nflows >= 64 else \
                [k % nflows for k in range(64)]
        elif w % 4 == 1:
            a, b = (nflows - 1, 0) if w % 8 == 1 else (nflows // 2, nflows - 1)
            flows += [a if k % 2 == 0 else b for k in range(64)]
        elif w % 4 == 2:
            flows += [nflows - 1] * 64
        else:
            ids = [0, nflows - 2 if nflows > 1 else 0, nflows - 1]
            flows += [ids[(k // 3) % 3] for k in range(64)]
    return flows[:2048 + 150]


@pytest.mark.parametrize("nflows", [1, 2, 1023, 1024])
def test_socket_count_edges(torch_dev, ctxs, nflows):
    flows = _socket_count_burst(nflows)
    if nflows >= 64:
        assert len(set(flows[:64])) == 64  # a wave of 64 different sockets
    if nflows == 1024:
        assert {0, 1022, 1023} <= set(flows)
    frames = [_udp(k, _SIZES[(k * 3) % len(_SIZES)]) for k in range(len(flows))]
    caps = [len(f) for f in frames]
    want = _check(torch_dev, ctxs(nflows), frames, caps, _forge(frames, flows), nflows,
                  seed=nflows)
    assert want.totals[0] == len(flows)


def test_1025_sockets_refused(torch_dev):
    """above RXG_COMPACT_MAX_FLOWS ids: RXG_ERANGE, nothing written"""
    torch, dev = torch_dev
    frames = [_udp(k, 20) for k in range(70)]
    v = _forge(frames, [k % 1025 for k in range(70)])
    buf, off, lens = F.pack_filled(frames, 4)
    with R.Context(0) as ctx:
        ctx.flows_sync(_socks(1025), None)
        t = [torch.from_numpy(a).to(dev) for a in
             (buf, off.view(np.int32), lens.view(np.int16), np.frombuffer(v.tobytes(), np.uint8).copy())]
        outs = [torch.full((k,), 0x6B, dtype=torch.uint8, device=dev)
                for k in (70 * 16, 1026 * 4, 4096, 12)]
        with pytest.raises(R.RxgError) as e:
            ctx.udp_compact_dev(t[0], t[1], t[2], 70, 4, t[3], outs[0], outs[1], outs[2], 4096,
                                outs[3], stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert e.value.rc == -34  # RXG_ERANGE
        assert all(bool((o == 0x6B).all()) for o in outs)


def test_no_udp_sockets_clears_totals(torch_dev):
    """an empty UDP id space: the public call clears d_totals[0..2] and
    d_first[0] on the stream and writes nothing else"""
    torch, dev = torch_dev
    frames = [_udp(k, 20) for k in range(70)]
    v = _forge(frames, [0] * 70)
    buf, off, lens = F.pack_filled(frames, 4)
    tcb = np.zeros(1, R.TCB_DTYPE)
    tcb[0] = (0, R.ip_raw(L), 0, R.port_raw(9999), R.TCP_STATUS_LISTEN)
    for sync in (False, True):
        with R.Context(0) as ctx:
            if sync:
                ctx.flows_sync(None, tcb)
            assert ctx.num_udp_ids == 0
            t = [torch.from_numpy(a).to(dev) for a in
                 (buf, off.view(np.int32), lens.view(np.int16),
                  np.frombuffer(v.tobytes(), np.uint8).copy())]
            d_dg, d_first, d_pl = [torch.full((k,), 0x6B, dtype=torch.uint8, device=dev)
                                   for k in (70 * 16, 16, 4096)]
            d_tot = torch.full((4,), 0x6B6B6B6B, dtype=torch.int32, device=dev)
            ctx.udp_compact_dev(t[0], t[1], t[2], 70, 4, t[3], d_dg, d_first, d_pl, 4096, d_tot,
                                stream=torch.cuda.current_stream(dev).cuda_stream)
            torch.cuda.synchronize(dev)
            assert d_tot.cpu().tolist() == [0, 0, 0, 0x6B6B6B6B]
            assert d_first.cpu().tolist() == [0] * 4 + [0x6B] * 12
            assert bool((d_dg == 0x6B).all()) and bool((d_pl == 0x6B).all())


# ---- frames that must be skipped -------------------------------------------
def test_skipped_frames_between_delivered(torch_dev, ctxs):
    """TCP with rc 0, UDP with every non-zero rc, UDP to an id >= nflows and
    to FLOW_NONE, each between delivered frames of the same socket: none gets
    a record or moves a rank; 2 tiles, so skipped frames also sit at wave and
    tile starts"""
    nflows = 6
    n = 2048 + 77
    frames = [_udp(k, _SIZES[k % len(_SIZES)]) for k in range(n)]
    v = _forge(frames, [k % nflows for k in range(n)])
    kinds = [(R.CLS_TCP, 0, None), (R.CLS_UDP, R.RC_UDP_NOMEM, None),
             (R.CLS_UDP, R.RC_UDP_NO_SOCKET, None), (R.CLS_UDP, R.RC_TCP_BAD_CKSUM, None),
             (R.CLS_UDP, R.RC_KNI, None), (R.CLS_UDP, 0, nflows), (R.CLS_UDP, 0, nflows + 1000),
             (R.CLS_UDP, 0, R.FLOW_NONE), (R.CLS_IPV4_OTHER, 0, None), (R.CLS_ARP, 0, None)]
    skipped = 0
    for k in range(n):
        if k % 3 == 0 or k in (64, 1024, 1025, 2047):
            cls, rc, fid = kinds[(k // 3) % len(kinds)]
            v[k]["cls"], v[k]["rc"] = cls, rc
            if fid is not None:
                v[k]["flow_id"] = fid
            skipped += 1
    caps = [len(f) for f in frames]
    want = _check(torch_dev, ctxs(nflows), frames, caps, v, nflows, seed=3)
    assert want.totals[0] == n - skipped


# ---- the copy's mask: payload lengths and capture ends ---------------------
PLENS = [0, 1, 2, 3, 4, 5, 13, 14, 15, 16, 17, 18, 31, 32, 33, 1458, 1472]


def test_payload_length_edges(torch_dev, ctxs):
    """every payload byte 0xFF, so a byte kept past ncopy shows in the zero
    padding; full captures, captures one byte short, and a forged payload_len
    of 65535 on a 100-byte capture (58 bytes are there)"""
    nflows = 2
    ff = b"\xff" * 1500
    frames, caps = [], []
    for rep in range(3):
        for p in PLENS:
            f = _udp(len(frames), p, ff)
            frames.append(f)
            caps.append(len(f) - (1 if rep == 2 and p else 0))
    big = len(frames)
    frames.append(_udp(big, 200, ff))
    caps.append(100)
    flows = [k % nflows for k in range(len(frames))]
    v = _forge(frames, flows)
    v[big]["payload_len"] = 65535
    want = _check(torch_dev, ctxs(nflows), frames, caps, v, nflows, seed=5)
    assert sorted(set(want.dgram["len"])) == PLENS + [65535]
    r = int(np.nonzero(want.dgram["frame"] == big)[0][0])
    assert want.ncopy[r] == 58


CAPLENS = [20, 26, 29, 30, 34, 35, 36, 40, 41, 42, 43, 44, 45, 46, 47, 57, 58, 59]


def test_capture_edges(torch_dev, ctxs):
    """payload_len 20 on captures that end inside sip, inside sport, before
    and inside the copy's first dwords (a dword whose first byte is the last
    captured one), and inside the payload; 0xFF payloads and 0xEE neighbours"""
    nflows = 3
    frames, caps = [], []
    for rep in range(2):
        for c in CAPLENS:
            frames.append(_udp(len(frames), 20, b"\xff" * 20))
            caps.append(c)
    v = _forge(frames, [k % nflows for k in range(len(frames))])
    assert set(v["payload_len"]) == {20}
    want = _check(torch_dev, ctxs(nflows), frames, caps, v, nflows, seed=6)
    assert want.totals[0] == len(frames)
    assert sorted(set(want.ncopy)) == [0, 1, 2, 3, 4, 5, 15, 16, 17]


# ---- payload_cap -----------------------------------------------------------
def test_payload_cap_exact_and_short(torch_dev, ctxs):
    """exactly the bytes needed: flag 0, all written.  16 bytes fewer: flag 1,
    totals[0..1] and every record unchanged, the payloads that fit written,
    the last one not, nothing at or past payload_cap touched"""
    nflows = 4
    n = 1024 + 130
    frames = [_udp(k, [33, 1, 16, 700, 48][k % 5]) for k in range(n)]
    flows = [(k * 5 + k // 64) % nflows for k in range(n)]
    flows[-1] = nflows - 1  # the last rank: a 700-byte payload, so part of it would fit
    assert len(frames[-1]) == 742
    caps = [len(f) for f in frames]
    v = _forge(frames, flows)
    full =_check(torch_dev, ctxs(nflows), frames, caps, v, nflows, seed=7)
    need = int(full.totals[1])
    assert full.totals[2] == 0 and full.written.all()
    short = _check(torch_dev, ctxs(nflows), frames, caps, v, nflows, cap=need - 16, seed=7)
    assert list(short.totals) == [n, need, 1]
    assert short.dgram.tobytes() == full.dgram.tobytes()
    last = int(full.dgram["offset"][-1])
    assert short.written[:last].all() and not short.written[last:].any() and last < need - 16


# ---- K1's own verdicts, 16-B units -----------------------------------------
def test_k1_verdicts_at_16_byte_units(torch_dev):
    """classify then compact on the device at unit_log2 = 4, frames starting
    at 16-B boundaries that are not 64-B boundaries: the verdicts equal the
    oracle's and K3's outputs the model's over them"""
    torch, dev = torch_dev
    rng = np.random.default_rng(8)
    nsock = 40
    udp = _socks(nsock)
    frames, caps = [], []
    for k in range(1500):
        pl = bytes(rng.integers(1, 256, int(rng.choice([0, 1, 7, 15, 16, 17, 90, 400])),
                                dtype=np.uint8))
        f = F.udp_frame(f"10.3.{k % 200}.{k % 250 + 1}", 2000 + k, L,
                        30000 + int(rng.integers(0, nsock + 3)), pl)
        frames.append(f)
        caps.append(len(f) if rng.random() > 0.1 else int(rng.integers(20, len(f) + 1)))
    order = rng.permutation(len(frames))
    buf, off, lens = F.pack_filled(frames, 4, caplens=caps, fill=0xEE, mem_order=order)
    assert np.count_nonzero(off % 4) > 500  # 16-B starts off the 64-B grid
    want_v = O.Tables(udp, np.zeros(0, R.TCB_DTYPE)).classify(buf, off, lens, 4)
    with R.Context(0) as ctx:
        ctx.flows_sync(udp, None)
        d_v = torch.empty(len(frames) * 16, dtype=torch.uint8, device=dev)
        ctx.classify_dev(torch.from_numpy(buf).to(dev), torch.from_numpy(off.view(np.int32)).to(dev),
                         torch.from_numpy(lens.view(np.int16)).to(dev), len(frames), 4, 200, d_v,
                         None, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        v = d_v.cpu().numpy().view(R.VERDICT_DTYPE)
        assert v.tobytes() == want_v.tobytes()
        want = _check(torch_dev, ctx, frames, caps, v, nsock, seed=8, d_v=d_v)
    assert 800 < want.totals[0] < 1500


# ---- an id space with a hole -----------------------------------------------
def test_id_space_with_a_hole(torch_dev):
    """8 sockets synced, the one with id 3 removed and committed: the id space
    keeps 8 ids, K1 finds no socket for the removed one's port, and K3 gives
    the empty id first[3] == first[4] with the later ranks unaffected"""
    torch, dev = torch_dev
    udp = _socks(8)
    frames = [F.udp_frame(f"10.4.0.{k % 250 + 1}", 3000 + k, L, 30000 + (k * 5 + k // 64) % 8,
                          _PAYLOAD[k:k + [3, 16, 40, 0, 17][k % 5]]) for k in range(1100)]
    caps = [len(f) for f in frames]
    order = np.random.default_rng(9).permutation(len(frames))
    buf, off, lens = F.pack_filled(frames, 4, fill=0xEE, mem_order=order)
    with R.Context(0) as ctx:
        ctx.flows_sync(udp, None)
        ctx.flows_remove([3])
        ctx.flows_commit()
        if ctx.num_udp_ids != 8:
            pytest.skip("rxg_flows_remove leaves no hole in the UDP id space")
        d_v = torch.empty(len(frames) * 16, dtype=torch.uint8, device=dev)
        ctx.classify_dev(torch.from_numpy(buf).to(dev), torch.from_numpy(off.view(np.int32)).to(dev),
                         torch.from_numpy(lens.view(np.int16)).to(dev), len(frames), 4, 100, d_v,
                         None, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        v = d_v.cpu().numpy().view(R.VERDICT_DTYPE)
        ports = np.array([int.from_bytes(f[36:38], "big") - 30000 for f in frames])
        assert np.all(v["rc"][ports == 3] == R.RC_UDP_NO_SOCKET)
        live = (ports != 3) & (v["payload_len"] > 0)
        assert np.all(v["rc"][live] == 0) and np.array_equal(v["flow_id"][live], ports[live])
        want = _check(torch_dev, ctx, frames, caps, v, 8, seed=9, d_v=d_v)
    assert want.first[3] == want.first[4] and want.first[4] < want.first[5]
    assert want.totals[0] == np.count_nonzero(live)
