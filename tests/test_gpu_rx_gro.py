"""TCP receive coalescing on the GPU (rxg_tcp_coalesce_dev, the coalescing
form of K4) against (a) the numpy model of tests/gro_ref.py for runs and
offsets, (b) rxg_tcp_compact_dev on the same burst for every record field but
offset, (c) the frames for every run's payload bytes; the zero tail of every
run, and a 0xA5 canary everywhere else in the payload buffer and past
payload_cap.  Then the socket scenario of tests/test_rx_gro.py through
nstack_rx_burst and nstack_rx_submit / nstack_rx_complete with the option on,
fragments pointing into a held pooled buffer and copied."""
import functools

import numpy as np
import pytest

import frames as F
import gro_ref as G
import oracle_bind as O
import rxgpu as R

pytestmark = pytest.mark.gpu
L = G.L
LENS = [1, 3, 15, 16, 17, 100, 1460]   # every destination phase mod 16 occurs
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


@functools.lru_cache(maxsize=None)
def _main_burst():
    """700 frames: connection 0 a chain of 300 x 16 B (sorted records 0 .. 299:
    it crosses the 256-record block boundary, and at W = 4096 a window break
    lands on record 256); the rule cases on connections 10 .. 19 and the
    listener; trains of random lengths on the others.  Per-connection order
    kept, connections interleaved at random."""
    rng = np.random.default_rng(5)
    per = {}
    per[0] = [(F.tcp_frame(*G.conn(0), L, 9999, G._p(rng, 16), seq=(2 ** 32 - 2000 + 16 * q) & 0xFFFFFFFF), None)
              for q in range(300)]
    for label, f, cap in G.rule_cases(rng, base=10):
        per.setdefault("L" if label == "L" else 10 + label, []).append((f, cap))
    others = [k for k in range(1, NTCB) if not 10 <= k < 20]
    left = 700 - sum(len(v) for v in per.values())
    while left > 0:
        k = others[int(rng.integers(len(others)))]
        seq = int(rng.integers(0, 2 ** 32))
        for _ in range(min(left, int(rng.integers(1, 10)))):
            n = int(rng.choice(LENS))
            per.setdefault(k, []).append((F.tcp_frame(*G.conn(k), L, 9999, G._p(rng, n),
                                                      seq=seq & 0xFFFFFFFF), None))
            seq += n
            left -= 1
    frames, caps = [], []
    keys = list(per)
    while keys:
        k = keys[int(rng.integers(len(keys)))]
        f, cap = per[k].pop(0)
        frames.append(f)
        caps.append(len(f) if cap is None else cap)
        if not per[k]:
            keys.remove(k)
    assert len(frames) == 700
    return frames, caps, _tcbs(NTCB)


@functools.lru_cache(maxsize=None)
def _single_flow_burst():
    """600 frames of one connection, all one chain"""
    rng = np.random.default_rng(6)
    frames, seq = [], 2 ** 32 - 30000
    for _ in range(600):
        n = int(rng.choice(LENS))
        frames.append(F.tcp_frame(*G.conn(0), L, 9999, G._p(rng, n), seq=seq & 0xFFFFFFFF))
        seq += n
    return frames, [len(f) for f in frames], _tcbs(1)


def _coalesce(torch, dev, ctx, frames, caps, unit, W, short=False):
    """one burst through classify, rxg_tcp_compact_dev and rxg_tcp_coalesce_dev;
    every check of the module docstring.  short: payload_cap one run short."""
    n = len(frames)
    buf, off, lens = F.pack_frames(frames, unit, caplens=caps)
    want_v = O.Tables(np.zeros(0, R.UDP_SOCK_DTYPE), ctx._tcb).classify(buf, off, lens, unit)
    flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 and
             x["flow_id"] < len(ctx._tcb) else None for x in want_v]
    wseg, wsip = G.records(frames, caps, flows)
    wrun = G.runs_model(wseg, wsip, W)
    for r in wrun:  # the records' offsets: byte-contiguous inside a run
        k0, k1 = int(r["first"]), int(r["first"] + r["nseg"])
        c = wseg["ncopy"][k0:k1].astype(np.int64)
        wseg["offset"][k0:k1] = int(r["offset"]) + np.cumsum(c) - c
    used = int((wrun["offset"][-1] + wrun["bytes"][-1] + 15) // 16 * 16)
    cap = used - 16 if short else used + 64
    if short:
        assert wrun["bytes"][-1] > 0
    total = used + 4096
    want_pl = np.full(total, CANARY, np.uint8)
    for r in (wrun[:-1] if short else wrun):
        o = int(r["offset"])
        data = b"".join(frames[g["frame"]][34 + 4 * g["hl"]:34 + 4 * g["hl"] + g["ncopy"]]
                        for g in wseg[r["first"]:r["first"] + r["nseg"]])
        assert len(data) == r["bytes"]
        want_pl[o:o + len(data)] = np.frombuffer(data, np.uint8)
        want_pl[o + len(data):(o + len(data) + 15) // 16 * 16] = 0    # the zero tail
    d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
    d_v = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    ctx.classify_dev(d_pk, d_off, d_ln, n, unit, 1500, d_v, None, stream=sh)
    d_seg0 = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_pl0 = torch.zeros(len(buf) + 4096, dtype=torch.uint8, device=dev)
    d_tot0 = torch.empty(3, dtype=torch.int32, device=dev)
    ctx.tcp_compact_dev(d_pk, d_off, d_ln, n, unit, d_v, d_seg0, d_pl0, len(buf) + 4096, d_tot0, stream=sh)
    d_seg = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_run = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_pl = torch.full((total,), CANARY, dtype=torch.uint8, device=dev)
    d_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
    ctx.tcp_coalesce_dev(d_pk, d_off, d_ln, n, unit, d_v, W, d_seg, d_run, d_pl, cap, d_tot, stream=sh)
    torch.cuda.synchronize(dev)
    assert d_v.cpu().numpy().view(R.VERDICT_DTYPE).tobytes() == want_v.tobytes()
    tot0 = d_tot0.cpu().numpy().view(np.uint32)
    tot = d_tot.cpu().numpy().view(np.uint32)
    assert tot0[0] == tot[0] == len(wseg) and tot[3] == len(wrun)
    assert tot[1] == used and tot[2] == (1 if short else 0)
    seg0 = d_seg0.cpu().numpy().view(R.SEGMENT_DTYPE)[:tot[0]]
    seg = d_seg.cpu().numpy().view(R.SEGMENT_DTYPE)[:tot[0]]
    run = d_run.cpu().numpy().view(R.TCP_RUN_DTYPE)[:tot[3]]
    assert run.tobytes() == wrun.tobytes(), [(k, run[k], wrun[k]) for k in range(len(run))
                                             if run[k] != wrun[k]][:5]                      # (a)
    for name in R.SEGMENT_DTYPE.names:                                                       # (b)
        if name != "offset":
            assert np.array_equal(seg[name], seg0[name]), name
    assert seg.tobytes() == wseg.tobytes(), [(k, seg[k], wseg[k]) for k in range(len(seg))
                                             if seg[k] != wseg[k]][:5]
    assert np.all(d_seg.cpu().numpy()[32 * int(tot[0]):] == 0xEE)
    assert np.all(d_run.cpu().numpy()[16 * int(tot[3]):] == 0xEE)
    pl = d_pl.cpu().numpy()
    bad = np.nonzero(pl != want_pl)[0]                                                       # (c)
    assert len(bad) == 0, (bad[:8], pl[bad[:8]], want_pl[bad[:8]])
    return wseg, wrun


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
def test_coalesce_matches_model_compact_and_frames(torch_dev, unit):
    torch, dev = torch_dev
    frames, caps, tcb = _main_burst()
    with _Ctx(tcb) as ctx:
        for W in (1, 1460, 4096, 65536):
            seg, run = _coalesce(torch, dev, ctx, frames, caps, unit, W)
            chain = [r for r in run if seg[r["first"]]["flow"] == 0]
            if W == 4096:   # the window break on the block boundary
                assert [int(r["first"]) for r in chain] == [0, 256]
            if W == 65536:  # one run across the block boundary
                assert len(chain) == 1 and chain[0]["nseg"] == 300
            if W == 1:
                assert len(run) == len(seg)
        phases = {int(s["offset"]) % 16 for s in seg if s["ncopy"]}
        assert phases == set(range(16))
        assert len(seg) == 700 and seg["flow"][-1] == NTCB      # (all delivered; the listener's last)
        _coalesce(torch, dev, ctx, frames, caps, unit, 65536, short=True)


@pytest.mark.parametrize("n,ids", G.STAGE_EDGES)
def test_coalesce_stage_edges(torch_dev, n, ids):
    """the record counts and id spaces where the sort and the coalescing stage
    take another path (gro_ref.STAGE_EDGES); the chain's 16-B chunks are read
    from every byte phase of the source"""
    torch, dev = torch_dev
    frames, caps, _ = G.boundary_burst(n, ids - 1, 7)
    with _Ctx(_tcbs(ids - 1)) as ctx:
        for W in (1460, 65536):
            seg, run = _coalesce(torch, dev, ctx, frames, caps, 6, W)
    assert len(seg) == n
    if n > 4:
        hlen = (16 - seg["offset"].astype(np.int64) % 16) % 16     # bytes before the first 16-B chunk
        chunk = seg["ncopy"] >= hlen + 16
        assert {int(x) for x in (34 + 4 * seg["hl"][chunk] + hlen[chunk]) % 4} == {0, 1, 2, 3}


def test_coalesce_single_flow_burst(torch_dev):
    torch, dev = torch_dev
    frames, caps, tcb = _single_flow_burst()
    with _Ctx(tcb) as ctx:
        for W in (1460, 65536):
            seg, run = _coalesce(torch, dev, ctx, frames, caps, 6, W)
            assert run["nseg"].sum() == 600
        assert len(run) == -(-int(seg["ncopy"].sum()) // 65536)   # one chain, cut by the window alone


def test_coalesce_past_one_scan_chunk(torch_dev):
    """300,000 segments, 1172 record blocks: past 1024 blocks every thread of the
    one-block scans takes more than one block value.  100 connections x 3000
    in-sequence 64-B frames (10 payload bytes), interleaved frame by frame:
    every chain spans 12 blocks, so at W = 65536 its head lies up to 11 blocks
    back.  Frames and the model are built with numpy alone."""
    torch, dev = torch_dev
    NC, PER = 100, 3000
    n = NC * PER
    rng = np.random.default_rng(8)
    i = np.arange(n)
    c, q = i % NC, i // NC
    sip = (10 | (2 << 8) | ((c >> 8) << 16) | ((c & 255) << 24)).astype(np.uint32)
    f = F.tcp64_frames(sip, np.full(n, R.ip_raw(L), np.uint32), np.full(n, R.port_raw(40000), np.uint16),
                       np.full(n, R.port_raw(9999), np.uint16))
    seq = ((c * 2654435761 + 10 * q) & 0xFFFFFFFF).astype(np.uint32)
    f[:, 38:42] = seq.astype(">u4").view(np.uint8).reshape(n, 4)
    f[:, 54:64] = rng.integers(0, 256, (n, 10), dtype=np.uint8)
    f[:, 50:52] = 0       # the L4 checksum again (frames.tcp64_frames' sum, over the new bytes)
    wd = f.view("<u2").astype(np.uint64)
    s = wd[:, 13:17].sum(axis=1) + wd[:, 17:32].sum(axis=1) + 0x0600 + 0x1E00
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    f[:, 50:52] = ((~s) & 0xFFFF).astype("<u2").view(np.uint8).reshape(n, 2)
    tcb = np.zeros(NC + 1, R.TCB_DTYPE)
    tcb["sip"][:NC], tcb["status"][:NC] = sip[:NC], 4
    tcb["dip"], tcb["sport"], tcb["dport"] = R.ip_raw(L), R.port_raw(40000), R.port_raw(9999)
    tcb[NC] = (0, R.ip_raw(L), 0, R.port_raw(9999), R.TCP_STATUS_LISTEN)
    j = np.arange(n)                       # sorted record j = connection j // PER, its frame j % PER
    frame = (j % PER) * NC + j // PER
    wseg = np.zeros(n, R.SEGMENT_DTYPE)
    wseg["frame"], wseg["flow"], wseg["seq"], wseg["plen"] = frame, j // PER, seq[frame], 10
    wseg["sport"], wseg["dport"] = R.port_raw(40000), R.port_raw(9999)
    wseg["ncopy"], wseg["flags"], wseg["hl"] = 10, 0x18, 5
    off = np.arange(n, dtype=np.uint32)
    lens = np.full(n, 64, np.uint16)
    with _Ctx(tcb) as ctx:
        d_pk = torch.from_numpy(np.concatenate([f.reshape(-1), np.zeros(64, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
        d_v = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        sh = torch.cuda.current_stream(dev).cuda_stream
        ctx.classify_dev(d_pk, d_off, d_ln, n, 6, 64, d_v, None, stream=sh)
        for W in (1460, 65536):
            wrun = G.runs_model(wseg, sip[frame], W)
            assert len(wrun) == NC * -(-PER * 10 // W)
            o = wrun["offset"].astype(np.int64)
            rid = np.repeat(np.arange(len(wrun)), wrun["nseg"])
            wseg["offset"] = o[rid] + 10 * (j - wrun["first"][rid])
            used = int((o[-1] + wrun["bytes"][-1] + 15) // 16 * 16)
            want_pl = np.full(used + 4096, CANARY, np.uint8)
            want_pl[:used] = 0
            want_pl[(wseg["offset"].astype(np.int64)[:, None] + np.arange(10)).reshape(-1)] = \
                f[frame, 54:64].reshape(-1)
            d_seg = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
            d_run = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
            d_pl = torch.full((used + 4096,), CANARY, dtype=torch.uint8, device=dev)
            d_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
            ctx.tcp_coalesce_dev(d_pk, d_off, d_ln, n, 6, d_v, W, d_seg, d_run, d_pl, used, d_tot, stream=sh)
            torch.cuda.synchronize(dev)
            assert d_tot.cpu().numpy().view(np.uint32).tolist() == [n, used, 0, len(wrun)]
            assert d_run.cpu().numpy().view(R.TCP_RUN_DTYPE)[:len(wrun)].tobytes() == wrun.tobytes()
            assert d_seg.cpu().numpy().tobytes() == wseg.tobytes()
            assert np.array_equal(d_pl.cpu().numpy(), want_pl)


def test_coalesce_empty_and_arguments(torch_dev):
    torch, dev = torch_dev
    frames, caps, tcb = _single_flow_burst()
    with _Ctx(tcb) as ctx:
        d_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
        d_pl = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
        sh = torch.cuda.current_stream(dev).cuda_stream
        ctx.tcp_coalesce_dev(None, None, None, 0, 6, None, 65536, None, None, d_pl, 64, d_tot, stream=sh)
        torch.cuda.synchronize(dev)
        assert list(d_tot.cpu().numpy()) == [0, 0, 0, 0] and np.all(d_pl.cpu().numpy() == CANARY)
        d8 = torch.zeros(4096, dtype=torch.uint8, device=dev)
        for W, pl in ((0, d_pl), ((1 << 20) + 1, d_pl), (65536, None)):
            with pytest.raises(R.RxgError):
                ctx.tcp_coalesce_dev(d8, d8, d8, 1, 6, d8, W, d8, d8, pl, 64, d_tot, stream=sh)
    with R.Context(0) as ctx:   # an empty tcb id space: the totals are zeroed
        d_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
        ctx.tcp_coalesce_dev(d8, d8, d8, 4, 6, d8, 65536, d8, d8, d_pl, 64, d_tot, stream=sh)
        torch.cuda.synchronize(dev)
        assert list(d_tot.cpu().numpy()) == [0, 0, 0, 0]


def test_delivery_pipeline_hands_out_the_runs(torch_dev):
    """rxg_deliver_submit / _wait with RXG_DLV_TCP_GRO: the runs of the burst
    come back with the records (rxg_delivery_runs), the records' offsets follow
    them, and the payload is the chain's bytes; off again: no runs"""
    frames, caps, tcb = _single_flow_burst()
    seg0, sip = G.records(frames, caps, [0] * len(frames))
    data = b"".join(f[54:] for f in frames)
    arr, keep = R.NStack.mbufs(frames)
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as ctx:
        ctx.flows_sync(None, tcb)
        ctx.tune_deliver(R.DLV_TCP_GRO)
        with pytest.raises(R.RxgError):
            ctx.tune_deliver(R.DLV_TCP_GRO | R.DLV_TCP_IN_PLACE)
        for W in (4096, 0):                      # 0: the default window again
            ctx.tune_gro(W)
            h = ctx.deliver_submit(arr)
            _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
            run = ctx.delivery_runs(h)
            want = G.runs_model(seg0, sip, W or R.GRO_DEFAULT_WINDOW)
            assert run.tobytes() == want.tobytes()
            assert len(seg) == len(frames) and len(pl) == want["offset"][-1] + (want["bytes"][-1] + 15) // 16 * 16
            for r in run:
                o, k = int(r["offset"]), int(r["first"])
                assert seg["offset"][k] == o
                before = int(seg0["ncopy"][:k].sum())
                assert pl[o:o + r["bytes"]].tobytes() == data[before:before + r["bytes"]]
        ctx.tune_deliver(0)
        h = ctx.deliver_submit(arr)
        _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
        assert len(ctx.delivery_runs(h)) == 0 and np.all(seg["offset"] % 16 == 0)


# ---- end to end: the socket layer on the GPU path -------------------------------------
def _session(mode, hold_all, seed=2, W=65536):
    ns = R.NStack(0)
    held = []
    try:
        ns.set_rx_gro(W)
        if hold_all:  # no pooled buffer is free: the payloads come in the set's own, copied
            for k in range(6):
                assert R._payload_hold(ns.lib.nstack_ctx(), k) == 0
                held.append(k)
        c0 = ns.stat(6)
        keys, events = G.scenario(seed)
        n_ns, n_os, absorbed = G.GroPair(ns, mode, W).run(keys, events)
        assert absorbed > 0 and n_ns + absorbed == n_os
        return ns.stat(6) - c0
    finally:
        for k in held:
            R._payload_release(ns.lib.nstack_ctx(), k)
        ns.fini()


def test_socket_layer_rx_burst_pooled_and_copied(torch_dev):
    pooled = _session("gpu", False)
    copied = _session("gpu", True)
    assert copied > pooled      # (pooled: only the frame-by-frame path's payloads are copied)


def test_socket_layer_pipelined(torch_dev):
    _session("pipe", False)
