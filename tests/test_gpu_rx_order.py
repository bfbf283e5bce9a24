"""TCP sequence ordering on the GPU (rxg_tcp_compact_ordered_dev, the ordering
form of K4) against (a) rxg_tcp_order_host and the numpy model of
tests/order_ref.py for the permutation and the moved count, (b) W = 0:
rxg_tcp_compact_dev run on the frames pre-arranged in the model's order, for
every record field and every byte of the payload buffer, (c) W != 0:
rxg_tcp_runs_host on the permuted records for the runs, and
rxg_tcp_coalesce_dev on the pre-arranged frames for records and payload; a
0xA5 canary everywhere else and past payload_cap; the records-only form.  An
in-order burst equals the two existing calls byte for byte.  Then the
delivery pipeline with the flag alone, with coalescing, in place and off, and
the socket scenario of tests/test_rx_order.py through nstack_rx_burst and
nstack_rx_submit / nstack_rx_complete.

The verdicts the calls take are the oracle's, so a frame whose capture is cut
before its ports (which K1 never hands to K4) can still be given a tcb id:
the records' rule for bytes past the capture is checked where it decides the
order."""
import functools

import numpy as np
import pytest

import frames as F
import gro_ref as G
import oracle_bind as O
import order_ref as D
import rxgpu as R

pytestmark = pytest.mark.gpu
L = G.L
NTCB = 40                              # connections 0 .. 39, the listener's id is 40
CANARY = 0xA5


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")
    return torch, torch.device("cuda:0")


def _tcbs(n):
    tcb = np.zeros(n + 1, R.TCB_DTYPE)
    for k in range(n):
        cip, cport = G.conn(k)
        tcb[k] = (R.ip_raw(cip), R.ip_raw(L), R.port_raw(cport), R.port_raw(9999), 4)
    tcb[n] = (0, R.ip_raw(L), 0, R.port_raw(9999), R.TCP_STATUS_LISTEN)
    return tcb


def _train(rng, k, count, lens=(1, 3, 15, 16, 17, 100, 1460), seq=None):
    """connection k's in-sequence segments"""
    seq = int(rng.integers(0, 2 ** 32)) if seq is None else seq
    out = []
    for _ in range(count):
        n = int(rng.choice(lens))
        out.append(F.tcp_frame(*G.conn(k), L, 9999, G._p(rng, n), seq=seq & 0xFFFFFFFF))
        seq += n
    return out


def _mix(rng, per, permute):
    """per[key] = [(frame, cap or None, forced id or None)] in sequence order ->
    (frames, caps, forced): the keys interleaved at random, every key's items
    shuffled (permute) or in order"""
    order = {k: (rng.permutation(len(v)) if permute else np.arange(len(v))) for k, v in per.items()}
    left = {k: 0 for k in per}
    keys = list(per)
    frames, caps, forced = [], [], {}
    while keys:
        k = keys[int(rng.integers(len(keys)))]
        f, cap, fid = per[k][order[k][left[k]]]
        if fid is not None:
            forced[len(frames)] = fid
        frames.append(f)
        caps.append(len(f) if cap is None else cap)
        left[k] += 1
        if left[k] == len(per[k]):
            keys.remove(k)
    return frames, caps, forced


@functools.lru_cache(maxsize=None)
def _main_burst(permute=True):
    """about 500 frames.  Connection 0: 300 x 16 B, sorted records 0 .. 299, one
    group across the 256-record block boundary; the rule cases on connections
    10 .. 17 and the listener (their own arrival order kept); connection 20:
    captures cut before byte 42 (the low half of seq reads 0); connection 21:
    captures cut before byte 30 between whole ones (sip, ports, seq and flags
    read 0: other groups); trains on the others; UDP and bad-checksum frames
    between them.  permute off: the trains and the junk alone, in sequence (the
    rule cases and the cut captures carry inversions of their own)"""
    rng = np.random.default_rng(31)
    per = {0: [(f, None, None) for f in _train(rng, 0, 300, lens=(16,), seq=2 ** 32 - 2000)]}
    for k in range(1, 10):
        per[k] = [(f, None, None) for f in _train(rng, k, int(rng.integers(2, 40)))]
    if permute:
        per[20] = [(F.tcp_frame(*G.conn(20), L, 9999, b"", seq=s, flags=0x10), 40, 20)
                   for s in (0x00010000, 0x00020000, 0x0003FFFF, 0x00040000)]
        whole = _train(rng, 21, 6, lens=(100,))
        per[21] = [(whole[0], None, None), (whole[1], None, None), (whole[2], 28, 21),
                   (whole[3], 28, 21), (whole[4], None, None), (whole[5], None, None)]
    per["junk"] = [(F.udp_frame("10.0.0.1", 5555, L, 20005, b"HELLO"), None, None) for _ in range(20)] + \
        [(F.tcp_frame(*G.conn(3), L, 9999, b"bad", corrupt=True), None, None) for _ in range(20)]
    frames, caps, forced = _mix(rng, per, permute)
    cases = D.rule_cases(rng, base=10) if permute else []
    at = sorted(int(x) for x in rng.integers(0, len(frames), len(cases)))
    for (label, f, cap), i in reversed(list(zip(cases, at))):   # (in their own order)
        frames.insert(i, f)
        caps.insert(i, cap)
        forced = {(j + 1 if j >= i else j): v for j, v in forced.items()}
    return frames, caps, forced, _tcbs(NTCB)


@functools.lru_cache(maxsize=None)
def _tile_burst():
    """3000 frames: connection 0 owns sorted records 0 .. 1899 and connection 1
    records 1900 .. 2299, one group across the 2048-key tile boundary; both
    shuffled, small payloads"""
    rng = np.random.default_rng(32)
    per = {0: [(f, None, None) for f in _train(rng, 0, 1900, lens=(1, 16, 17))],
           1: [(f, None, None) for f in _train(rng, 1, 400, lens=(1, 16, 17), seq=2 ** 32 - 900)]}
    for k in range(2, 30):
        per[k] = [(f, None, None) for f in _train(rng, k, 25, lens=(1, 16, 17))]
    frames, caps, forced = _mix(rng, per, True)
    assert len(frames) == 3000
    return frames, caps, forced, _tcbs(NTCB)


@functools.lru_cache(maxsize=None)
def _single_flow_burst(n=3000):
    """one connection owning every segment, fully reversed"""
    rng = np.random.default_rng(33)
    frames = _train(rng, 0, n, lens=(1, 16, 17, 100), seq=2 ** 32 - 30000)[::-1]
    return frames, [len(f) for f in frames], {}, _tcbs(1)


class _Dev:
    """a burst on the device with its (oracle's, then forced) verdicts, and the
    three calls on it; every output buffer pre-filled"""

    def __init__(self, torch, dev, ctx, frames, caps, forced, unit):
        self.torch, self.dev, self.ctx, self.unit, self.n = torch, dev, ctx, unit, len(frames)
        buf, off, lens = F.pack_frames(frames, unit, caplens=caps)
        v = O.Tables(np.zeros(0, R.UDP_SOCK_DTYPE), ctx._tcb).classify(buf, off, lens, unit)
        for i, fid in forced.items():
            v[i]["flow_id"], v[i]["cls"], v[i]["rc"] = fid, R.CLS_TCP, 0
        self.v = v
        self.flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 and
                      x["flow_id"] < len(ctx._tcb) else None for x in v]
        self.cap = len(buf) + 64
        self.d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        self.d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
        self.d_v = torch.from_numpy(np.frombuffer(v.tobytes(), np.uint8).copy()).to(dev)
        self.sh = torch.cuda.current_stream(dev).cuda_stream

    def _out(self, ntot, payload):
        t, dev, n = self.torch, self.dev, self.n
        return (t.full((n * 32,), 0xEE, dtype=t.uint8, device=dev),
                t.full((n * 16,), 0xEE, dtype=t.uint8, device=dev),
                t.full((self.cap + 4096,), CANARY, dtype=t.uint8, device=dev) if payload else None,
                t.full((ntot,), 7, dtype=t.int32, device=dev))

    def _back(self, seg, run, pl, tot):
        self.torch.cuda.synchronize(self.dev)
        return (seg.cpu().numpy().view(R.SEGMENT_DTYPE), run.cpu().numpy().view(R.TCP_RUN_DTYPE),
                None if pl is None else pl.cpu().numpy(), tot.cpu().numpy().view(np.uint32))

    def k4(self, payload=True):
        seg, run, pl, tot = self._out(3, payload)
        self.ctx.tcp_compact_dev(self.d_pk, self.d_off, self.d_ln, self.n, self.unit, self.d_v, seg, pl,
                                 self.cap, tot, stream=self.sh)
        return self._back(seg, run, pl, tot)

    def gro(self, W):
        seg, run, pl, tot = self._out(4, True)
        self.ctx.tcp_coalesce_dev(self.d_pk, self.d_off, self.d_ln, self.n, self.unit, self.d_v, W, seg,
                                  run, pl, self.cap, tot, stream=self.sh)
        return self._back(seg, run, pl, tot)

    def ordered(self, W, payload=True):
        seg, run, pl, tot = self._out(5, payload)
        self.ctx.tcp_compact_ordered_dev(self.d_pk, self.d_off, self.d_ln, self.n, self.unit, self.d_v,
                                         W, seg, run if W else None, pl, self.cap, tot, stream=self.sh)
        return self._back(seg, run, pl, tot)


def _same_but_frame(a, b):
    for name in R.SEGMENT_DTYPE.names:
        if name != "frame":
            assert np.array_equal(a[name], b[name]), name


def _check_burst(torch, dev, ctx, burst, unit, windows=(0, 1460, 65536), want_moved=None):
    """every check of the module docstring on one burst; returns (records in
    K4's order, the permutation)"""
    frames, caps, forced = burst[:3]
    x = _Dev(torch, dev, ctx, frames, caps, forced, unit)
    wseg, wsip = G.records(frames, caps, x.flows)
    nseg = len(wseg)
    perm, moved = D.order_model(wseg, wsip)
    hperm, hmoved = R.tcp_order_host(wseg, wsip)
    assert np.array_equal(perm, hperm) and moved == hmoved                      # model = host rule
    if want_moved is not None:
        assert (moved > 0) == want_moved
    seg0, _, _, tot0 = x.k4()
    assert tot0[0] == nseg
    for name in R.SEGMENT_DTYPE.names:                                           # (the inputs are what the model saw)
        if name != "offset":
            assert np.array_equal(seg0[name][:nseg], wseg[name]), name
    # the frames pre-arranged: frame slot wseg.frame[k] takes the frame of record perm[k]
    src = np.arange(len(frames))
    src[wseg["frame"]] = wseg["frame"][perm]
    y = _Dev(torch, dev, ctx, [frames[i] for i in src], [caps[i] for i in src],
             {int(np.nonzero(src == i)[0][0]): fid for i, fid in forced.items()}, unit)
    for W in windows:
        seg, run, pl, tot = x.ordered(W)
        assert tot[0] == nseg and tot[4] == moved, (tot, moved)
        assert np.array_equal(seg["frame"][:nseg], wseg["frame"][perm])          # (a) the permutation
        if W == 0:
            pseg, prun, ppl, ptot = y.k4()
            assert tot[3] == 0 and np.all(run.view(np.uint8) == 0xEE)
        else:
            pseg, prun, ppl, ptot = y.gro(W)
            hrun = R.tcp_runs_host(wseg[perm], wsip[perm], W)                    # (c)
            assert tot[3] == len(hrun) and run[:tot[3]].tobytes() == hrun.tobytes()
            assert run.tobytes() == prun.tobytes()
        assert list(tot[:len(ptot)]) == list(ptot) and tot[2] == 0
        assert np.array_equal(pseg["frame"][:nseg], wseg["frame"])
        _same_but_frame(seg[:nseg], pseg[:nseg])                                 # (b) every field, offsets too
        assert np.all(seg.view(np.uint8)[32 * nseg:] == 0xEE)
        bad = np.nonzero(pl != ppl)[0]                                           # every byte, canaries too
        assert len(bad) == 0, (W, bad[:8], pl[bad[:8]], ppl[bad[:8]])
        assert np.all(pl[int(tot[1]):] == CANARY) and tot[1] <= x.cap
        if W == 0:
            want = wseg[perm]
            keep = want["ncopy"] > 0
            assert np.all(seg["offset"][:nseg] % 16 == 0)
            o = int(seg["offset"][:nseg][keep][-1]) if keep.any() else 0
            g = want[keep][-1] if keep.any() else None
            if g is not None:   # the last payload, straight from its frame
                a, c = 34 + 4 * int(g["hl"]), int(g["ncopy"])
                assert pl[o:o + c].tobytes() == frames[int(g["frame"])][a:a + c]
    seg, _, _, tot = x.ordered(0, payload=False)                                 # records only
    pseg, _, _, _ = y.k4(payload=False)
    assert tot[0] == nseg and tot[4] == moved and tot[1] == 0
    _same_but_frame(seg[:nseg], pseg[:nseg])
    assert np.array_equal(seg["offset"][:nseg], 34 + 4 * seg["hl"][:nseg].astype(np.uint32))
    assert np.array_equal(seg["frame"][:nseg], wseg["frame"][perm])
    return wseg, perm


class _Ctx:
    """a context with the test's tcbs synced"""

    def __init__(self, tcb):
        self.ctx = R.Context(0)
        self.tcb = tcb

    def __enter__(self):
        c = self.ctx.__enter__()
        c.flows_sync(None, self.tcb)
        c._tcb = self.tcb
        return c

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


@pytest.mark.parametrize("unit", [6, 4], ids=["unit64", "unit16"])
def test_ordered_matches_model_host_and_prearranged_k4(torch_dev, unit):
    torch, dev = torch_dev
    burst = _main_burst()
    with _Ctx(burst[3]) as ctx:
        wseg, perm = _check_burst(torch, dev, ctx, burst, unit, want_moved=True)
    # the group across the record-block boundary came out whole
    assert np.all(wseg["flow"][:300] == 0) and sorted(perm[:300]) == list(range(300))
    assert np.count_nonzero(perm[:300] != np.arange(300)) > 250
    d = (wseg["seq"][perm][:300].astype(np.int64) - int(wseg["seq"][perm][0])) & 0xFFFFFFFF
    assert np.all(np.diff(d) == 16)
    # the edge cases as frames, by hand
    D.check_hand(wseg, perm, lambda k: NTCB if k == "L" else 10 + k)
    # cut before byte 42: ordered by the captured half of seq (0x0003FFFF reads 0x00030000)
    c = wseg[perm][wseg["flow"] == 20]
    assert len(c) == 4 and list(c["seq"]) == [0x00010000, 0x00020000, 0x00030000, 0x00040000]
    # cut before byte 30: sip and ports read 0, so these two are a group of their own
    c = wseg[perm][wseg["flow"] == 21]
    assert len(c) == 6 and sorted(c["sport"] == 0) == [False] * 4 + [True] * 2
    assert np.count_nonzero(wseg["flow"] == 3) > 0 and len(wseg) == len(burst[0]) - 40   # (junk is no record)


def test_ordered_group_across_the_tile_boundary(torch_dev):
    torch, dev = torch_dev
    burst = _tile_burst()
    with _Ctx(burst[3]) as ctx:
        wseg, perm = _check_burst(torch, dev, ctx, burst, 6, windows=(0, 65536), want_moved=True)
    assert np.all(wseg["flow"][1900:2300] == 1) and sorted(perm[1900:2300]) == list(range(1900, 2300))
    s = wseg["seq"][perm][1900:2300].astype(np.int64)
    assert np.all(((s[1:] - s[:-1]) & 0xFFFFFFFF) < 18)       # in sequence, across the wrap
    assert np.count_nonzero(perm[:1900] != np.arange(1900)) > 1800


@pytest.mark.parametrize("n,ids", G.STAGE_EDGES)
def test_ordered_stage_edges(torch_dev, n, ids):
    """the record counts and id spaces where the sort, the ordering stage, K4's
    record stage and the coalescing stage take another path
    (gro_ref.STAGE_EDGES), on a burst with one capture cut inside the TCP
    header"""
    torch, dev = torch_dev
    burst = G.boundary_burst(n, ids - 1, 34, cut=True)
    with _Ctx(_tcbs(ids - 1)) as ctx:
        wseg, perm = _check_burst(torch, dev, ctx, burst, 6, windows=(0, 65536), want_moved=n > 4)
    assert len(wseg) == n and (n == 1 or np.count_nonzero(wseg["hl"] == 0) == 1)


def test_ordered_one_connection_owns_the_burst_reversed(torch_dev):
    torch, dev = torch_dev
    burst = _single_flow_burst()
    with _Ctx(burst[3]) as ctx:
        wseg, perm = _check_burst(torch, dev, ctx, burst, 6, windows=(0, 65536), want_moved=True)
    assert len(perm) == 3000 and np.array_equal(perm, np.arange(3000)[::-1])


@pytest.mark.parametrize("unit", [6, 4], ids=["unit64", "unit16"])
def test_in_order_burst_equals_the_existing_calls(torch_dev, unit):
    """nothing to move: the outputs of rxg_tcp_compact_dev and
    rxg_tcp_coalesce_dev byte for byte, moved = 0"""
    torch, dev = torch_dev
    frames, caps, forced, tcb = _main_burst(False)
    assert not forced
    with _Ctx(tcb) as ctx:
        x = _Dev(torch, dev, ctx, frames, caps, {}, unit)
        seg0, _, pl0, tot0 = x.k4()
        seg, run, pl, tot = x.ordered(0)
        assert tot0[0] > 400 and list(tot) == [*tot0, 0, 0]
        assert seg.tobytes() == seg0.tobytes() and pl.tobytes() == pl0.tobytes()
        for W in (1460, 65536):
            seg0, run0, pl0, tot0 = x.gro(W)
            seg, run, pl, tot = x.ordered(W)
            assert list(tot) == [*tot0, 0]
            assert seg.tobytes() == seg0.tobytes() and run.tobytes() == run0.tobytes()
            assert pl.tobytes() == pl0.tobytes()
        seg0, _, _, tot0 = x.k4(payload=False)
        seg, _, _, tot = x.ordered(0, payload=False)
        assert seg.tobytes() == seg0.tobytes() and list(tot) == [*tot0, 0, 0]


def test_ordered_70000_segments(torch_dev):
    """70,000 segments of 64-B frames (10 payload bytes): 274 record blocks, 35
    sort tiles, and the head index of the last groups needs a third radix
    digit.  70 connections x 1000 segments interleaved frame by frame, every
    connection's seq values a random shuffle of its in-sequence ones.  Frames,
    verdicts and the expected output are built with numpy alone."""
    torch, dev = torch_dev
    NC, PER = 70, 1000
    n = NC * PER
    rng = np.random.default_rng(34)
    i = np.arange(n)
    c, q = i % NC, i // NC
    sip = (10 | (2 << 8) | ((c >> 8) << 16) | ((c & 255) << 24)).astype(np.uint32)
    f = F.tcp64_frames(sip, np.full(n, R.ip_raw(L), np.uint32), np.full(n, R.port_raw(40000), np.uint16),
                       np.full(n, R.port_raw(9999), np.uint16))
    rank = np.argsort(rng.random((NC, PER)), axis=1)            # rank[c, q] = the place in sequence
    seq = ((c * 2654435761 + 10 * rank[c, q]) & 0xFFFFFFFF).astype(np.uint32)
    f[:, 38:42] = seq.astype(">u4").view(np.uint8).reshape(n, 4)
    f[:, 54:64] = rng.integers(0, 256, (n, 10), dtype=np.uint8)
    v = np.zeros(n, R.VERDICT_DTYPE)                            # (K4 reads flow_id, cls and rc)
    v["flow_id"], v["cls"], v["rc"] = c, R.CLS_TCP, 0
    tcb = np.zeros(NC + 1, R.TCB_DTYPE)
    tcb["sip"][:NC], tcb["status"][:NC] = sip[:NC], 4
    tcb["dip"], tcb["sport"], tcb["dport"] = R.ip_raw(L), R.port_raw(40000), R.port_raw(9999)
    tcb[NC] = (0, R.ip_raw(L), 0, R.port_raw(9999), R.TCP_STATUS_LISTEN)
    j = np.arange(n)                       # sorted record j = connection j // PER, its frame j % PER
    frame = (j % PER) * NC + j // PER
    wseg = np.zeros(n, R.SEGMENT_DTYPE)
    wseg["frame"], wseg["flow"], wseg["seq"], wseg["plen"] = frame, j // PER, seq[frame], 10
    wseg["ack"] = f[:, 42:46].copy().view(">u4").reshape(n)[frame]
    wseg["sport"], wseg["dport"] = R.port_raw(40000), R.port_raw(9999)
    wseg["ncopy"], wseg["flags"], wseg["hl"] = 10, 0x18, 5
    perm, moved = D.order_model(wseg, sip[frame])
    assert moved > n - 200 and np.array_equal(perm // PER, j // PER)
    # by construction: position k of connection c takes the frame whose rank is k
    assert np.array_equal(rank[j // PER, wseg["frame"][perm] // NC], j % PER)
    want = wseg[perm]
    want["offset"] = 16 * j
    want_pl = np.full(16 * n + 4096, CANARY, np.uint8)
    want_pl[:16 * n] = 0
    want_pl[(16 * j[:, None] + np.arange(10)).reshape(-1)] = f[want["frame"], 54:64].reshape(-1)
    with _Ctx(tcb) as ctx:
        d_pk = torch.from_numpy(np.concatenate([f.reshape(-1), np.zeros(64, np.uint8)])).to(dev)
        d_off = torch.from_numpy(np.arange(n, dtype=np.int32)).to(dev)
        d_ln = torch.from_numpy(np.full(n, 64, np.int16)).to(dev)
        d_v = torch.from_numpy(np.frombuffer(v.tobytes(), np.uint8).copy()).to(dev)
        sh = torch.cuda.current_stream(dev).cuda_stream
        d_seg = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
        d_pl = torch.full((16 * n + 4096,), CANARY, dtype=torch.uint8, device=dev)
        d_tot = torch.full((5,), 7, dtype=torch.int32, device=dev)
        ctx.tcp_compact_ordered_dev(d_pk, d_off, d_ln, n, 6, d_v, 0, d_seg, None, d_pl, 16 * n, d_tot,
                                    stream=sh)
        torch.cuda.synchronize(dev)
        assert d_tot.cpu().numpy().view(np.uint32).tolist() == [n, 16 * n, 0, 0, moved]
        seg = d_seg.cpu().numpy().view(R.SEGMENT_DTYPE)
        bad = np.nonzero(seg != want)[0]
        assert len(bad) == 0, (bad[:5], seg[bad[:5]], want[bad[:5]])
        assert np.array_equal(d_pl.cpu().numpy(), want_pl)


def test_ordered_empty_and_arguments(torch_dev):
    torch, dev = torch_dev
    with _Ctx(_tcbs(1)) as ctx:
        d_tot = torch.full((5,), 7, dtype=torch.int32, device=dev)
        d_pl = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
        sh = torch.cuda.current_stream(dev).cuda_stream
        for W in (0, 65536):
            d_tot.fill_(7)
            ctx.tcp_compact_ordered_dev(None, None, None, 0, 6, None, W, None, None, d_pl, 64, d_tot,
                                        stream=sh)
            torch.cuda.synchronize(dev)
            assert list(d_tot.cpu().numpy()) == [0] * 5 and np.all(d_pl.cpu().numpy() == CANARY)
        d8 = torch.zeros(4096, dtype=torch.uint8, device=dev)
        for W, run, pl in (((1 << 20) + 1, d8, d_pl), (65536, d8, None), (65536, None, d_pl)):
            with pytest.raises(R.RxgError):
                ctx.tcp_compact_ordered_dev(d8, d8, d8, 1, 6, d8, W, d8, run, pl, 64, d_tot, stream=sh)
        with pytest.raises(R.RxgError):
            ctx.tcp_compact_ordered_dev(d8, d8, d8, 1, 3, d8, 0, d8, None, d_pl, 64, d_tot, stream=sh)
    with R.Context(0) as ctx:   # an empty tcb id space: the totals are zeroed
        d_tot = torch.full((5,), 7, dtype=torch.int32, device=dev)
        ctx.tcp_compact_ordered_dev(d8, d8, d8, 4, 6, d8, 0, d8, None, d_pl, 64, d_tot, stream=sh)
        torch.cuda.synchronize(dev)
        assert list(d_tot.cpu().numpy()) == [0] * 5


def test_delivery_pipeline_orders_and_reports_moved(torch_dev):
    """rxg_deliver_submit / _wait with RXG_DLV_TCP_ORDER alone, with coalescing,
    in place, and off again; rxg_delivery_moved each time"""
    frames, caps, _, tcb = _single_flow_burst(600)
    seg0, sip = G.records(frames, caps, [0] * len(frames))
    perm, moved = D.order_model(seg0, sip)
    want = seg0[perm]
    data = b"".join(frames[g["frame"]][54:] for g in want)
    assert moved == 600 and np.array_equal(perm, np.arange(600)[::-1])
    arr, keep = R.NStack.mbufs(frames)

    def fields(seg, ref):
        for name in R.SEGMENT_DTYPE.names:
            if name != "offset":
                assert np.array_equal(seg[name], ref[name]), name
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as ctx:
        ctx.flows_sync(None, tcb)
        ctx.tune_deliver(R.DLV_TCP_ORDER)
        h = ctx.deliver_submit(arr)
        _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
        assert ctx.delivery_moved(h) == moved and len(ctx.delivery_runs(h)) == 0
        fields(seg, want)
        assert np.all(seg["offset"] % 16 == 0)
        assert b"".join(pl[int(g["offset"]):int(g["offset"]) + int(g["ncopy"])].tobytes() for g in seg) == data
        ctx.tune_deliver(R.DLV_TCP_ORDER | R.DLV_TCP_GRO)
        for W in (4096, 0):                      # 0: the default window again
            ctx.tune_gro(W)
            h = ctx.deliver_submit(arr)
            _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
            run = ctx.delivery_runs(h)
            wrun = G.runs_model(want, sip[perm], W or R.GRO_DEFAULT_WINDOW)
            assert ctx.delivery_moved(h) == moved and run.tobytes() == wrun.tobytes()
            fields(seg, want)
            before = 0
            for r in run:
                o, nb = int(r["offset"]), int(r["bytes"])
                assert seg["offset"][r["first"]] == o
                assert pl[o:o + nb].tobytes() == data[before:before + nb]
                before += nb
            assert len(run) < 600 // 4
        ctx.tune_deliver(R.DLV_TCP_ORDER | R.DLV_TCP_IN_PLACE)
        h = ctx.deliver_submit(arr)
        _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
        assert ctx.delivery_moved(h) == moved and len(pl) == 0
        fields(seg, want)
        assert np.all(seg["offset"] == 54)
        with pytest.raises(R.RxgError):
            ctx.tune_deliver(R.DLV_TCP_ORDER | R.DLV_TCP_GRO | R.DLV_TCP_IN_PLACE)
        ctx.tune_deliver(0)
        h = ctx.deliver_submit(arr)
        _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
        assert ctx.delivery_moved(h) == 0
        fields(seg, seg0)                        # arrival order again


# ---- end to end: the socket layer on the GPU path -------------------------------------
def _session(mode, hold_all, seed=2, W=0, inplace=False):
    ns = R.NStack(0)
    held = []
    try:
        ns.set_rx_order(True)
        if W:
            ns.set_rx_gro(W)
        if inplace:
            ns.set_rx_inplace(True)
        if hold_all:  # no pooled buffer is free: the payloads come in the set's own, copied
            for k in range(6):
                assert R._payload_hold(ns.lib.nstack_ctx(), k) == 0
                held.append(k)
        c0 = ns.stat(6)
        keys, events = D.scenario(seed)
        pair = D.OrderPair(ns, mode, W=W)
        n_ns, n_os, moved = pair.run(keys, events)
        assert moved == pair.want_moved and moved > 0
        assert (n_ns < n_os) if W else (n_ns == n_os)
        return ns.stat(6) - c0
    finally:
        for k in held:
            R._payload_release(ns.lib.nstack_ctx(), k)
        ns.fini()


def test_socket_layer_rx_burst_pooled_and_copied(torch_dev):
    pooled = _session("gpu", False)
    copied = _session("gpu", True)
    assert copied > pooled      # (pooled: only the frame-by-frame path's payloads are copied)


def test_socket_layer_rx_burst_with_gro_and_in_place(torch_dev):
    _session("gpu", False, W=65536)
    _session("gpu", False, inplace=True)


def test_socket_layer_pipelined(torch_dev):
    _session("pipe", False)
    _session("pipe", False, seed=3, W=65536)
