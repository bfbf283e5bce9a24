"""TCP stream assembly on the GPU (rxg_tcp_assemble_dev: the sort, the ordering
stage and the asm_* kernels) against the numpy model of tests/assemble_ref.py
and rxg_tcp_assemble_host, byte for byte: the records (the ordered form's, with
ncopy = take and offset = where those bytes lie), the streams, the six totals,
the payload buffer including every stream's zero pad, and a canary everywhere
else (past the records, past the streams, between and past the payload bytes,
past payload_cap).  Shapes: the hand-written edge cases; one connection owning
2 * 256 + 3 segments with duplicates and a hole on each side of a 256-record
block edge; 600 groups of 1 to 3 records; an all-duplicate burst; payload_cap
one byte short of a stream; n = 0.  A clean burst lays down the bytes of the
coalescing form.  Then the delivery pipeline with the flag, and the lossy
sessions of tests/test_rx_assemble.py through nstack_rx_burst and
nstack_rx_submit / nstack_rx_complete.

The verdicts the calls take are the oracle's."""
import functools

import numpy as np
import pytest

import assemble_ref as A
import frames as F
import gro_ref as G
import oracle_bind as O
import order_ref as D
import rxgpu as R

pytestmark = pytest.mark.gpu
L = G.L
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


def _seg(k, off, n, rng, flags=0x18, base=5000):
    return F.tcp_frame(*G.conn(k), L, 9999, G._p(rng, n), seq=(base + off) & A.M32, flags=flags)


def _shuffle_within(rng, per):
    """per[k] = connection k's frames -> one burst: connections interleaved,
    each one's frames in a random arrival order"""
    per = {k: [v[i] for i in rng.permutation(len(v))] for k, v in per.items()}
    frames = []
    while per:
        k = list(per)[int(rng.integers(len(per)))]
        frames.append(per[k].pop())
        if not per[k]:
            del per[k]
    return frames


def _run(torch, dev, ctx, frames, caps, unit, cap=None, forced=None):
    """the device call on one burst, every output pre-filled; returns the
    outputs beside what the model and the host restatement say.  forced:
    {frame: tcb id} of frames to deliver whatever the oracle's verdict"""
    n = len(frames)
    buf, off, lens = F.pack_frames(frames, unit, caplens=caps)
    v = O.Tables(np.zeros(0, R.UDP_SOCK_DTYPE), ctx._tcb).classify(buf, off, lens, unit)
    for i, fid in (forced or {}).items():
        v[i]["flow_id"], v[i]["cls"], v[i]["rc"] = fid, R.CLS_TCP, 0
    flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 and
             x["flow_id"] < len(ctx._tcb) else None for x in v]
    seg0, sip0 = G.records(frames, caps, flows)
    perm, moved = D.order_model(seg0, sip0)
    wseg, wsip = seg0[perm], sip0[perm]
    avail = A.avail_of(wseg, caps)
    m = A.assemble_model(wseg, wsip, avail)
    hst, hskip, htake, hdst = R.tcp_assemble_host(wseg, wsip, avail)      # model = host restatement
    assert hst.tobytes() == m["stream"].tobytes() and np.array_equal(htake, m["take"])
    assert np.array_equal(hskip, m["skip"]) and np.array_equal(hdst, m["dst"])
    size = len(buf) + 64 + 4096
    cap = len(buf) + 64 if cap is None else cap(m)
    d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int32)).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
    d_v = torch.from_numpy(np.frombuffer(v.tobytes(), np.uint8).copy()).to(dev)
    d_seg = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_st = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_pl = torch.full((size,), CANARY, dtype=torch.uint8, device=dev)
    d_tot = torch.full((6,), 7, dtype=torch.int32, device=dev)
    ctx.tcp_assemble_dev(d_pk, d_off, d_ln, n, unit, d_v, d_seg, d_st, d_pl, cap, d_tot,
                         stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    seg = d_seg.cpu().numpy().view(R.SEGMENT_DTYPE)
    st = d_st.cpu().numpy().view(R.TCP_STREAM_DTYPE)
    pl, tot = d_pl.cpu().numpy(), d_tot.cpu().numpy().view(np.uint32)
    img, used, over = A.payload_image(frames, wseg, m, size, cap, CANARY)
    want = wseg.copy()
    want["ncopy"], want["offset"] = m["take"], m["dst"]
    nseg, nst = len(wseg), len(m["stream"])
    assert list(tot) == [nseg, used, over, nst, moved, int(m["skip"].sum()) & A.M32]
    bad = np.nonzero(seg[:nseg] != want)[0]
    assert len(bad) == 0, (bad[:5], seg[bad[:5]], want[bad[:5]])
    assert np.all(seg.view(np.uint8)[32 * nseg:] == 0xEE)
    bad = np.nonzero(st[:nst] != m["stream"])[0]
    assert len(bad) == 0, (bad[:5], st[bad[:5]], m["stream"][bad[:5]])
    assert np.all(st.view(np.uint8)[32 * nst:] == 0xEE)
    bad = np.nonzero(pl != img)[0]                                        # every byte, canaries too
    assert len(bad) == 0, (bad[:8], pl[bad[:8]], img[bad[:8]])
    return wseg, m, pl, tot


# ---- the bursts --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hand_burst():
    """the hand-written cases on connections 10 .. 25 and the listener's id,
    between trains with duplicates on connections 0 .. 5 and junk"""
    rng = np.random.default_rng(51)
    cases = A.rule_cases(rng, base=10)
    frames = [c[1] for c in cases]
    caps = [c[2] for c in cases]
    extra = []
    for k in range(6):
        off = 0
        for _ in range(int(rng.integers(3, 12))):
            n = int(rng.choice([1, 15, 16, 17, 100, 1460]))
            extra.append(_seg(k, off, n, rng, flags=int(rng.choice([0x18, 0x10]))))
            if rng.random() < 0.3:
                extra.append(extra[-1])
            off += n
    extra += [F.udp_frame("10.0.0.1", 5555, L, 20005, b"HELLO") for _ in range(5)]
    extra += [F.tcp_frame(*G.conn(3), L, 9999, b"bad", corrupt=True) for _ in range(5)]
    for f in extra:                                   # (the cases keep their own order)
        i = int(rng.integers(0, len(frames) + 1))
        frames.insert(i, f)
        caps.insert(i, len(f))
    return frames, caps, _tcbs(40)


@functools.lru_cache(maxsize=None)
def _block_edge_burst():
    """one connection owning 2 * 256 + 3 segments: in sequence order, records
    250, 255, 256, 300, 511 and 512 repeat their predecessor (255 | 256 and
    511 | 512 are the block edges) and a hole opens before records 254, 257,
    510 and 514; the sequence crosses the wrap; arrival order shuffled"""
    rng = np.random.default_rng(52)
    frames, off, last = [], 0, None
    for i in range(2 * 256 + 3):
        if i in (250, 255, 256, 300, 511, 512):
            frames.append(last)
            continue
        if i in (254, 257, 510, 514):
            off += 1000
        n = int(rng.choice([1, 16, 17, 33, 100]))
        last = _seg(0, off, n, rng, flags=int(rng.choice([0x18, 0x10])), base=2 ** 32 - 9000)
        frames.append(last)
        off += n
    frames = [frames[i] for i in rng.permutation(len(frames))]
    return frames, [len(f) for f in frames], _tcbs(1)


@functools.lru_cache(maxsize=None)
def _groups_burst():
    """600 connections of 1 to 3 records: in sequence, duplicated, overlapping
    or with a hole; some with a FIN"""
    rng = np.random.default_rng(53)
    per = {}
    for k in range(600):
        off, fs = 0, []
        for q in range(int(rng.integers(1, 4))):
            n = int(rng.choice([1, 16, 40, 100]))
            kind = rng.random()
            if q and kind < 0.25:
                off -= int(rng.integers(1, 30))          # overlaps (or repeats) the one before
            elif q and kind < 0.4:
                off += 500                               # a hole
            off = max(off, 0)
            fs.append(_seg(k, off, n, rng, flags=int(rng.choice([0x18, 0x10, 0x19]))))
            off += n
        per[k] = fs
    frames = _shuffle_within(rng, per)
    return frames, [len(f) for f in frames], _tcbs(600)


def _flow_streams(wseg, m, flow):
    st = m["stream"]
    return st[wseg["flow"][st["first"]] == flow]


@pytest.mark.parametrize("unit", [6, 4], ids=["unit64", "unit16"])
def test_assemble_hand_cases(torch_dev, unit):
    torch, dev = torch_dev
    frames, caps, tcb = _hand_burst()
    with _Ctx(tcb) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, caps, unit)
    A.check_hand(wseg, m, lambda k: 40 if k == "L" else 10 + k)
    s = _flow_streams(wseg, m, 25)[0]                 # conflicting content: the first in sequence wins
    o = int(s["offset"])
    assert pl[o:o + 150].tobytes() == b"A" * 100 + b"B" * 50
    assert tot[5] > 0 and tot[2] == 0


def test_assemble_one_connection_across_the_block_edges(torch_dev):
    torch, dev = torch_dev
    frames, caps, tcb = _block_edge_burst()
    with _Ctx(tcb) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, caps, 6)
    assert len(wseg) == 515 and tot[4] > 400                           # (shuffled: nearly all moved)
    st = m["stream"]
    assert list(st["first"]) == [0, 254, 257, 510, 514] and list(st["flags"]) == [0, 2, 2, 2, 2]
    assert all(m["take"][i] == 0 and m["skip"][i] > 0 for i in (250, 255, 256, 300, 511, 512))
    assert np.count_nonzero(m["take"] == 0) == 6


@pytest.mark.parametrize("n,ids", G.STAGE_EDGES)
def test_assemble_stage_edges(torch_dev, n, ids):
    """the record counts and id spaces where the sort, the ordering stage and
    the assembly stage take another path (gro_ref.STAGE_EDGES), on a burst with
    one capture cut inside the TCP header; the 16-B chunks are read from every
    byte phase of the source (the overlaps' skip shifts it)"""
    torch, dev = torch_dev
    frames, caps, forced = G.boundary_burst(n, ids - 1, 55, cut=True)
    with _Ctx(_tcbs(ids - 1)) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, caps, 6, forced=forced)
    assert len(wseg) == n and (n == 1 or np.count_nonzero(wseg["hl"] == 0) == 1)
    if n > 4:
        assert tot[4] > 0 and tot[5] > 0                               # moved, skipped
        hlen = (16 - m["dst"].astype(np.int64) % 16) % 16              # bytes before the first 16-B chunk
        chunk = m["take"] >= hlen + 16
        src = 34 + 4 * wseg["hl"].astype(np.int64) + m["skip"] + hlen
        assert {int(x) for x in src[chunk] % 4} == {0, 1, 2, 3}


def test_assemble_600_groups(torch_dev):
    torch, dev = torch_dev
    frames, caps, tcb = _groups_burst()
    with _Ctx(tcb) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, caps, 6)
    st = m["stream"]
    assert len(np.unique(wseg["flow"])) == 600 and len(st) > 650
    assert np.any(st["flags"] & A.FIN) and np.any(st["flags"] & A.HOLE) and tot[5] > 0


def test_assemble_all_duplicates(torch_dev):
    """300 copies of one segment (more than a record block) and 3 of another
    connection's: one stream each, every copy but the first skipped whole"""
    torch, dev = torch_dev
    rng = np.random.default_rng(54)
    a, b = _seg(0, 0, 777, rng), _seg(1, 0, 16, rng)
    frames = [a] * 150 + [b] * 3 + [a] * 150
    with _Ctx(_tcbs(2)) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, [len(f) for f in frames], 6)
    assert list(m["stream"]["bytes"]) == [777, 16] and list(m["stream"]["nseg"]) == [300, 3]
    assert tot[5] == 299 * 777 + 2 * 16 and tot[1] == 784 + 16 and tot[4] == 0
    assert pl[:777].tobytes() == a[54:] and pl[784:800].tobytes() == b[54:]


def test_assemble_payload_cap_one_byte_short(torch_dev):
    """the last stream would end one byte past payload_cap: the flag, and the
    stream stays unwritten; every other stream is there"""
    torch, dev = torch_dev
    frames, caps, tcb = _hand_burst()

    def short(m):
        s = m["stream"][-1]
        assert s["bytes"] > 0
        return int(s["offset"]) + (int(s["bytes"]) + 15) // 16 * 16 - 1
    with _Ctx(tcb) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, caps, 6, cap=short)
    assert tot[2] == 1
    o = int(m["stream"]["offset"][-1])
    assert np.all(pl[o:] == CANARY) and not np.all(pl[:o] == CANARY)


def test_assemble_empty_and_arguments(torch_dev):
    torch, dev = torch_dev
    sh = torch.cuda.current_stream(dev).cuda_stream
    d8 = torch.zeros(4096, dtype=torch.uint8, device=dev)
    d_pl = torch.full((64,), CANARY, dtype=torch.uint8, device=dev)
    with _Ctx(_tcbs(1)) as ctx:
        d_tot = torch.full((6,), 7, dtype=torch.int32, device=dev)
        ctx.tcp_assemble_dev(None, None, None, 0, 6, None, None, None, d_pl, 64, d_tot, stream=sh)
        torch.cuda.synchronize(dev)
        assert list(d_tot.cpu().numpy()) == [0] * 6 and np.all(d_pl.cpu().numpy() == CANARY)
        with pytest.raises(R.RxgError):                            # d_payload NULL
            ctx.tcp_assemble_dev(d8, d8, d8, 1, 6, d8, d8, d8, None, 64, d_tot, stream=sh)
        with pytest.raises(R.RxgError):                            # no room for the streams
            ctx.tcp_assemble_dev(d8, d8, d8, 1, 6, d8, d8, None, d_pl, 64, d_tot, stream=sh)
        with pytest.raises(R.RxgError):
            ctx.tcp_assemble_dev(d8, d8, d8, 1, 3, d8, d8, d8, d_pl, 64, d_tot, stream=sh)
    with R.Context(0) as ctx:   # an empty tcb id space: the totals are zeroed
        d_tot = torch.full((6,), 7, dtype=torch.int32, device=dev)
        ctx.tcp_assemble_dev(d8, d8, d8, 4, 6, d8, d8, d8, d_pl, 64, d_tot, stream=sh)
        torch.cuda.synchronize(dev)
        assert list(d_tot.cpu().numpy()) == [0] * 6


def test_clean_burst_lays_down_the_coalescing_forms_bytes(torch_dev):
    """in-sequence PSH|ACK trains, nothing lost or repeated: one stream per
    connection, and the payload buffer is the one rxg_tcp_coalesce_dev writes
    with a window no train reaches"""
    torch, dev = torch_dev
    rng = np.random.default_rng(55)
    per = {}
    for k in range(12):
        off, fs, base = 0, [], int(rng.integers(0, 2 ** 32))
        for _ in range(int(rng.integers(1, 30))):
            n = int(rng.choice([1, 3, 15, 16, 17, 100, 1460]))
            fs.append(_seg(k, off, n, rng, base=base))
            off += n
        per[k] = fs
    frames = []
    while per:                                        # interleaved, every train in order
        k = list(per)[int(rng.integers(len(per)))]
        frames.append(per[k].pop(0))
        if not per[k]:
            del per[k]
    caps = [len(f) for f in frames]
    n = len(frames)
    with _Ctx(_tcbs(12)) as ctx:
        wseg, m, pl, tot = _run(torch, dev, ctx, frames, caps, 6)
        buf, off, lens = F.pack_frames(frames, 6)
        v = O.Tables(np.zeros(0, R.UDP_SOCK_DTYPE), ctx._tcb).classify(buf, off, lens, 6)
        d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
        d_v = torch.from_numpy(np.frombuffer(v.tobytes(), np.uint8).copy()).to(dev)
        d_seg = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device=dev)
        d_run = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
        d_pl = torch.full((len(pl),), CANARY, dtype=torch.uint8, device=dev)
        d_tot = torch.full((4,), 7, dtype=torch.int32, device=dev)
        ctx.tcp_coalesce_dev(d_pk, d_off, d_ln, n, 6, d_v, R.GRO_MAX_WINDOW, d_seg, d_run, d_pl,
                             len(buf) + 64, d_tot, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
    gtot = d_tot.cpu().numpy().view(np.uint32)
    run = d_run.cpu().numpy().view(R.TCP_RUN_DTYPE)[:gtot[3]]
    st = m["stream"]
    assert tot[4] == 0 and tot[5] == 0 and list(tot[:4]) == list(gtot) and len(st) == 12
    for name in ("first", "nseg", "bytes", "offset"):
        assert np.array_equal(st[name], run[name]), name
    assert np.array_equal(pl, d_pl.cpu().numpy())
    gseg = d_seg.cpu().numpy().view(R.SEGMENT_DTYPE)[:n]
    assert np.array_equal(gseg["offset"], m["dst"]) and np.array_equal(gseg["ncopy"], m["take"])


def test_delivery_pipeline_assembles_and_reports_streams(torch_dev):
    """rxg_deliver_submit / _wait with RXG_DLV_TCP_ASSEMBLE (alone, with
    RXG_DLV_TCP_ORDER, with RXG_DLV_DDOS) and off again"""
    frames, caps, tcb = _block_edge_burst()
    seg0, sip0 = G.records(frames, caps, [0] * len(frames))
    perm, moved = D.order_model(seg0, sip0)
    wseg, wsip = seg0[perm], sip0[perm]
    m = A.assemble_model(wseg, wsip, A.avail_of(wseg, caps))
    img, used, _ = A.payload_image(frames, wseg, m, 1 << 17, 1 << 17, 0)
    want = wseg.copy()
    want["ncopy"], want["offset"] = m["take"], m["dst"]
    arr, keep = R.NStack.mbufs(frames)
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as ctx:
        ctx.flows_sync(None, tcb)
        for fl in (R.DLV_TCP_ASSEMBLE, R.DLV_TCP_ASSEMBLE | R.DLV_TCP_ORDER,
                   R.DLV_TCP_ASSEMBLE | R.DLV_DDOS):
            ctx.tune_deliver(fl)
            h = ctx.deliver_submit(arr)
            _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
            st = ctx.delivery_streams(h)
            assert st.tobytes() == m["stream"].tobytes() and ctx.delivery_moved(h) == moved
            assert len(ctx.delivery_runs(h)) == 0
            assert seg.tobytes() == want.tobytes()
            for s in st:
                o, nb = int(s["offset"]), int(s["bytes"])
                assert pl[o:o + nb].tobytes() == img[o:o + nb].tobytes()
        for fl in (R.DLV_TCP_ASSEMBLE | R.DLV_TCP_GRO, R.DLV_TCP_ASSEMBLE | R.DLV_TCP_IN_PLACE):
            with pytest.raises(R.RxgError):
                ctx.tune_deliver(fl)
        ctx.tune_deliver(0)
        h = ctx.deliver_submit(arr)
        _, _, _, _, seg, pl, _ = ctx.deliver_wait(h)
        assert len(ctx.delivery_streams(h)) == 0 and ctx.delivery_moved(h) == 0
        assert np.array_equal(seg["frame"], seg0["frame"])      # arrival order again


# ---- end to end: the socket layer on the GPU path -------------------------------------
def _session(mode, seed, hold_all=False):
    ns = R.NStack(0)
    held = []
    try:
        ns.set_rx_assemble(True)
        if hold_all:  # no pooled buffer is free: the payloads come in the set's own, copied
            for k in range(6):
                assert R._payload_hold(ns.lib.nstack_ctx(), k) == 0
                held.append(k)
        c0 = ns.stat(6)
        pair = A.AsmPair(ns, mode, seed)
        rounds = pair.run()
        pair.check()
        assert rounds > 3 and pair.want_dup > 0 and pair.want_holes > 0
        assert ns.stat(19) == pair.want_dup and ns.stat(20) == pair.want_holes
        return ns.stat(6) - c0
    finally:
        for k in held:
            R._payload_release(ns.lib.nstack_ctx(), k)
        ns.fini()


def test_socket_layer_rx_burst_pooled_and_copied(torch_dev):
    pooled = _session("gpu", 1)
    copied = _session("gpu", 1, hold_all=True)
    assert copied > pooled      # (pooled: the fragments point into the held buffer)


def test_socket_layer_pipelined(torch_dev):
    _session("pipe", 2)
