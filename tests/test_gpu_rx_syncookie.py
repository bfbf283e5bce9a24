"""SYN cookies on the GPU (K7, csrc/rx_syncookie.hip, rxg_syncookie_dev)
against rxg_syncookie_host and the Python model of tests/cookie_ref.py, bit
for bit: status bytes, descriptors, totals, a 0xA5 canary behind both outputs.
Burst sizes across the wave, block and tile edges of the compaction; all-SYN,
no-candidate and mixed bursts with truncated captures; both offset units; an
unaligned status pointer.  Then the delivery pipeline with RXG_DLV_SYNCOOKIE
(alone, and with stream assembly and the flood detector), the descriptors
through K5, and the socket-layer scenario of tests/test_rx_syncookie.py
through nstack_rx_burst and nstack_rx_submit / nstack_rx_complete."""
import numpy as np
import pytest

import cookie_ref as M
import frames as F
import rxgpu as R
import test_rx_syncookie as C

pytestmark = pytest.mark.gpu
CANARY = 0xA5
PAD = 16
T = C.T


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")
    return torch, torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx():
    with R.Context(0) as c:
        yield c


def _dev_run(torch_dev, ctx, buf, off, lens, unit, v, lm, id_space, p, skew=0):
    """one burst through rxg_syncookie_dev: (status, txd bytes of totals[0]
    descriptors, totals), the canaries checked.  skew: the status pointer's
    offset from its allocation (an address the dword stores cannot use)"""
    t, dev = torch_dev
    n = len(lens)
    up = lambda a, view: t.from_numpy(a.view(view).copy() if a.size else np.zeros(1, view)).to(dev)
    d_pk, d_off, d_ln = up(buf, np.uint8), up(off, np.int32), up(lens, np.int16)
    d_v = up(v.view(np.uint8), np.uint8)
    d_lm = up(lm, np.int32)
    d_st = t.full((skew + n + PAD,), CANARY, dtype=t.uint8, device=dev)
    d_tx = t.full((48 * (n + PAD),), CANARY, dtype=t.uint8, device=dev)
    d_tot = t.full((4 + PAD,), 0x5A5A5A5A, dtype=t.int32, device=dev)
    sh = t.cuda.current_stream(dev).cuda_stream
    ctx.syncookie_dev(d_pk, d_off, d_ln, n, unit, d_v, d_lm if id_space else None, id_space, p,
                      d_st[skew:], d_tx, d_tot, stream=sh)
    t.cuda.synchronize(dev)
    tot = d_tot.cpu().numpy().view(np.uint32)
    assert np.all(tot[4:] == 0x5A5A5A5A)
    st, tx = d_st.cpu().numpy(), d_tx.cpu().numpy()
    assert np.all(st[:skew] == CANARY) and np.all(st[skew + n:] == CANARY)
    assert np.all(tx[48 * int(tot[0]):] == CANARY)
    return st[skew:skew + n], tx[:48 * int(tot[0])], tot[:4].copy()


def _check(torch_dev, ctx, frames, caps, v, unit, t=T, max_age=2, id_space=M.ID_SPACE,
           listeners=M.LISTENERS, skew=0):
    buf, off, lens = F.pack_frames(frames, unit, caps)
    lm = M.lmask_of(listeners, id_space)
    p = R.ck_params(M.KEY, t, max_age, 14600)
    hst, htx, htot = R.syncookie_host(buf, off, lens, unit, v, lm, id_space, p)
    st, tx, tot = _dev_run(torch_dev, ctx, buf, off, lens, unit, v, lm, id_space, p, skew)
    assert list(tot) == list(htot)
    assert st.tobytes() == hst.tobytes()
    assert tx.tobytes() == htx.tobytes()
    return st, tx.view(R.TXD_DTYPE), tot


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 4099]
_bursts = {}


def _burst(kind, n):
    """fuzzed once per (kind, n), shared by the units"""
    if (kind, n) not in _bursts:
        _bursts[kind, n] = M.fuzz_burst(7000 + n + {"mixed": 0, "syn": 1, "none": 2}[kind], n, T, kind)
    return _bursts[kind, n]


@pytest.mark.parametrize("unit", [4, 6])
@pytest.mark.parametrize("kind", ["mixed", "syn", "none"])
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host(torch_dev, ctx, n, kind, unit):
    frames, caps, v = _burst(kind, n)
    st, tx, tot = _check(torch_dev, ctx, frames, caps, v, unit)
    if kind == "syn":
        assert tot[0] == n and np.all(st == 1)
    if kind == "none":
        assert not tot.any() and not st.any()
    if kind == "mixed" and n >= 255:
        assert set(st) == {0, 1, 2, 3} and any(c < 54 for c in caps)
    if unit == 6 and n in (257, 4099):             # the model, where the host form was not checked
        buf, off, lens = F.pack_frames(frames, unit, caps)
        want = M.run(buf, off, lens, unit, v, M.lmask_of(M.LISTENERS, M.ID_SPACE), M.ID_SPACE, M.KEY, T)
        assert st.tobytes() == want[0].tobytes() and tx.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_status_bytes_at_an_unaligned_address(torch_dev, ctx, skew):
    frames, caps, v = _burst("mixed", 257)
    _check(torch_dev, ctx, frames, caps, v, 6, skew=skew)


def test_named_cases_and_arguments(torch_dev, ctx):
    cases = C.named_cases()
    st, _, _ = _check(torch_dev, ctx, [c[1] for c in cases], [c[2] or len(c[1]) for c in cases],
                      np.concatenate([c[3] for c in cases]), 6)
    assert [int(s) for s in st] == [c[4] for c in cases]
    frames, caps, v = _burst("mixed", 257)
    # the counter's wrap, a wider window, an id space below the ids, an empty one
    _check(torch_dev, ctx, frames, caps, v, 6, t=0x100)
    _check(torch_dev, ctx, frames, caps, v, 6, t=1, max_age=255)
    st, _, tot = _check(torch_dev, ctx, frames, caps, v, 6, id_space=3, listeners=(0,))
    assert tot[0] and tot[0] < _check(torch_dev, ctx, frames, caps, v, 6)[2][0]
    st, _, tot = _check(torch_dev, ctx, frames, caps, v, 6, id_space=0, listeners=())
    assert not st.any() and not tot.any()
    t, dev = torch_dev
    d = t.zeros(64, dtype=t.uint8, device=dev)
    for bad in (dict(p=R.ck_params(M.KEY, T, 256)), dict(st=None), dict(tx=None), dict(tot=None)):
        with pytest.raises(R.RxgError) as e:
            ctx.syncookie_dev(d, d, d, 1, 6, d, d, 8, bad.get("p", R.ck_params(M.KEY, T)),
                              bad.get("st", d), bad.get("tx", d), bad.get("tot", d))
        assert e.value.rc == -22


# ---- through K5 --------------------------------------------------------------------
def test_descriptors_through_the_tx_encoder(torch_dev, ctx):
    t, dev = torch_dev
    frames, caps, v = _burst("syn", 257)
    buf, off, lens = F.pack_frames(frames, 6, caps)
    lm = M.lmask_of(M.LISTENERS, M.ID_SPACE)
    p = R.ck_params(M.KEY, T)
    _, htx, htot = R.syncookie_host(buf, off, lens, 6, v, lm, M.ID_SPACE, p)
    n = int(htot[0])
    cap = 64 * n
    want = R.tx_encode_host(htx, np.zeros(16, np.uint8), cap)
    up = lambda a, view: t.from_numpy(a.view(view).copy()).to(dev)
    d_tx = t.zeros(48 * n, dtype=t.uint8, device=dev)
    d_st = t.zeros(n, dtype=t.uint8, device=dev)
    d_tot = t.zeros(4, dtype=t.int32, device=dev)
    sh = t.cuda.current_stream(dev).cuda_stream
    ctx.syncookie_dev(up(buf, np.uint8), up(off, np.int32), up(lens, np.int16), n, 6,
                      up(v.view(np.uint8), np.uint8), up(lm, np.int32), M.ID_SPACE, p, d_st, d_tx, d_tot,
                      stream=sh)
    d_pk = t.full((cap + 64,), CANARY, dtype=t.uint8, device=dev)
    d_off = t.zeros(n, dtype=t.int32, device=dev)
    d_len = t.zeros(n, dtype=t.int16, device=dev)
    d_tt = t.zeros(4, dtype=t.int32, device=dev)
    d_pay = t.zeros(16, dtype=t.uint8, device=dev)
    ctx.tx_encode_dev(d_tx, n, d_pay, d_pk, cap, 0, d_off, d_len, 64, 0, d_tt, stream=sh)
    t.cuda.synchronize(dev)
    got = d_pk.cpu().numpy()
    w_pk, w_off, w_len = want[0], want[1], want[2]
    assert list(d_tt.cpu().numpy()[:2]) == [n, cap]
    assert got[:cap].tobytes() == np.asarray(w_pk)[:cap].tobytes() and np.all(got[cap:] == CANARY)
    assert d_off.cpu().numpy().view(np.uint32).tolist() == list(w_off)
    assert d_len.cpu().numpy().view(np.uint16).tolist() == list(w_len) == [54] * n


# ---- through the delivery pipeline -------------------------------------------------------
L = M.LOCAL


def _tables():
    udp = np.zeros(1, R.UDP_SOCK_DTYPE)
    udp[0]["localip"], udp[0]["localport"], udp[0]["protocol"] = R.ip_raw(L), R.port_raw(5000), 17
    tcb = np.zeros(3, R.TCB_DTYPE)
    tcb[0] = (R.ip_raw("10.9.0.1"), R.ip_raw(L), R.port_raw(40000), R.port_raw(9999), 4)
    tcb[1] = (0, R.ip_raw(L), 0, R.port_raw(8080), R.TCP_STATUS_LISTEN)
    tcb[2] = (0, R.ip_raw(L), 0, R.port_raw(8081), R.TCP_STATUS_LISTEN)
    return udp, tcb


def _delivery_bursts():
    """two bursts: SYNs, valid / forged / stale ACKs to the listeners, data
    of an established connection (two segments swapped), datagrams, and
    frames for nobody"""
    rng = np.random.default_rng(77)
    out = []
    for b in range(2):
        fr, seq = [], 1000 + 700 * b
        for j in range(300 + 37 * b):
            src, sport, isn = "10.%d.%d.7" % (1 + b, 1 + j % 200), 2000 + j, int(rng.integers(1 << 32))
            k = j % 10
            port = 8080 + (j & 1)
            if k < 4:
                fr.append(M.syn(src, sport, port, isn))
            elif k == 4:
                fr.append(M.ack_for(src, sport, port, isn, T - (j // 10) % 4, payload=b"pig" * (j % 3), flags=0x18))
            elif k == 5:
                fr.append(M.ack_for(src, sport, port, isn, T, dack=1 + j))
            elif k == 6:
                fr.append(F.udp_frame(src, sport, L, 5000, bytes(rng.integers(0, 256, 30, dtype=np.uint8))))
            elif k == 7:
                fr.append(F.tcp_frame("10.9.0.1", 40000, L, 9999, bytes(rng.integers(0, 256, 100, dtype=np.uint8)),
                                      seq=seq))
                seq += 100
            elif k == 8:
                fr.append(M.syn(src, sport, 7777, isn))                 # no listener there
            else:
                fr.append(M.syn(src, sport, port, isn, corrupt=True))
        fr[7], fr[17] = fr[17], fr[7]
        out.append(fr)
    return out


def _deliver_all(torch_dev, flags, pipelined):
    """every burst through the delivery pipeline: per burst the results as
    bytes, the cookie results, and the verdicts"""
    results, cookies = [], []
    p = R.ck_params(M.KEY, 0)
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as c:
        c.flows_sync(*_tables())
        c.tune_deliver(flags)
        c.syncookie_set(p, [1, 2])
        c.syncookie_tick(T)

        def keep(res, ck):
            out, dg, first, up, seg, tp, _ = res
            results.append(tuple(x.tobytes() for x in (out, dg, first, up, seg, tp)))
            cookies.append((ck, out.copy()))
        bursts = [R.NStack.mbufs(b) for b in _delivery_bursts()]
        if pipelined:
            hs = [c.deliver_submit(arr) for arr, _ in bursts]
            for h in hs:
                keep(c.deliver_wait(h), c.delivery_cookies(h))
        else:
            for arr, _ in bursts:
                keep(c.process_mbufs_deliver(arr), c.delivery_cookies())
            c.syncookie_set(p, [2])                                  # the mask follows the next set
            c.process_mbufs_deliver(bursts[0][0])
            st = c.delivery_cookies()[0]
            assert st is None or (st[1::2].any() and not st[0::2].any())   # port 8081: odd frames
    return results, cookies


def _check_cookies(torch_dev, ctx, cookies):
    for fr, (ck, out) in zip(_delivery_bursts(), cookies):
        st, tx, tot = ck
        buf, off, lens = F.pack_frames(fr, 6)
        lm = M.lmask_of((1, 2), 3)
        p = R.ck_params(M.KEY, T)
        hst, htx, htot = R.syncookie_host(buf, off, lens, 6, out, lm, 3, p)
        dst, dtx, dtot = _dev_run(torch_dev, ctx, buf, off, lens, 6, out, lm, 3, p)
        assert list(tot) == list(htot) == list(dtot) and tot[0] > 50 and tot[1] > 10 and tot[2] > 10
        assert st.tobytes() == hst.tobytes() == dst.tobytes()
        assert tx.tobytes() == htx.tobytes() == dtx.tobytes()


@pytest.mark.parametrize("pipelined", [False, True], ids=["one", "two_in_flight"])
def test_delivery_pipeline(torch_dev, ctx, pipelined):
    base, none = _deliver_all(torch_dev, 0, pipelined)
    assert all(ck[0] is None and ck[1] is None and not ck[2].any() for ck, _ in none)
    got, cookies = _deliver_all(torch_dev, R.DLV_SYNCOOKIE, pipelined)
    assert got == base                                                # nothing else changes
    assert any(len(r[4]) for r in base) and any(len(r[1]) for r in base)
    _check_cookies(torch_dev, ctx, cookies)


def test_delivery_pipeline_with_assembly_and_the_detector(torch_dev, ctx):
    fl = R.DLV_TCP_ASSEMBLE | R.DLV_DDOS
    base, _ = _deliver_all(torch_dev, fl, True)
    got, cookies = _deliver_all(torch_dev, fl | R.DLV_SYNCOOKIE, True)
    assert got == base
    _check_cookies(torch_dev, ctx, cookies)


# ---- the socket layer on the GPU paths ------------------------------------------------
@pytest.fixture(scope="module")
def cpu_log():
    ns = R.NStack(R.HOST_ONLY)
    try:
        return M.scenario(ns, "cpu")
    finally:
        ns.fini()


@pytest.mark.parametrize("encode", [False, True], ids=["host_frames", "k5"])
@pytest.mark.parametrize("mode", ["gpu", "pipe"])
def test_socket_layer(torch_dev, cpu_log, mode, encode):
    ns = R.NStack(0)
    try:
        ns.set_tx_encode(encode)
        log = M.scenario(ns, mode)
        if encode:
            assert ns.stat(13) == M.NSYN                             # the SYN-ACKs came from K5
    finally:
        ns.fini()
    C.check_scenario(log)
    C.check_synacks(log["synacks"], True)
    for k in log:
        if k != "synacks":
            assert log[k] == cpu_log[k], k
    # the CPU path's frames with the oracle's checksums are the GPU paths' frames
    buf, off, lens = F.pack_frames(cpu_log["synacks"])
    filled = C.O.tx_cksum(buf, off, lens, 6)
    assert [bytes(filled[int(o) << 6:(int(o) << 6) + 54]) for o in off] == log["synacks"]
