"""The L2 responder on the GPU (K8, csrc/rx_l2.hip, rxg_l2_dev) against
rxg_l2_host and the Python model of tests/l2_ref.py, byte for byte: status
bytes, answer frames, roff / rlen / rsrc, totals, a 0xA5 canary behind all six
outputs.  Burst sizes across the wave, block and tile edges; no-candidate,
all-ARP, all-echo and mixed bursts with cut captures and bad checksums; both
offset units; an unaligned status pointer; the hand cases (every message
length); 300 echo requests of 1472 bytes; the capacity cut.  Then the delivery
pipeline with RXG_DLV_L2 (alone, with stream assembly + K6 + K7, two bursts in
flight; with the flag off nothing else changes), and the socket-layer scenario
of tests/test_rx_l2.py through nstack_rx_burst and nstack_rx_submit /
nstack_rx_complete."""
import numpy as np
import pytest

import cookie_ref as CK
import frames as F
import l2_ref as M
import rxgpu as R
import test_rx_l2 as C

pytestmark = pytest.mark.gpu
CANARY = 0xA5
PAD = 16
BIG = 1 << 23


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


def _dev_run(torch_dev, ctx, buf, off, lens, unit, v, p, cap, skew=0):
    """one burst through rxg_l2_dev: (status, frames, roff, rlen, rsrc, totals)
    whole, as rxgpu.l2_host returns them with pad (the canaries in place).
    skew: the status pointer's offset from its allocation"""
    t, dev = torch_dev
    n = len(lens)
    up = lambda a, view: t.from_numpy(a.view(view).copy() if a.size else np.zeros(1, view)).to(dev)
    d_pk, d_off, d_ln = up(buf, np.uint8), up(off, np.int32), up(lens, np.int16)
    d_v = up(v.view(np.uint8), np.uint8)
    d_st = t.full((skew + n + PAD,), CANARY, dtype=t.uint8, device=dev)
    d_out = t.full((cap + 64 * PAD,), CANARY, dtype=t.uint8, device=dev)
    assert d_out.data_ptr() % 64 == 0
    d_ro = t.full((4 * (n + PAD),), CANARY, dtype=t.uint8, device=dev)
    d_rl = t.full((2 * (n + PAD),), CANARY, dtype=t.uint8, device=dev)
    d_rs = t.full((4 * (n + PAD),), CANARY, dtype=t.uint8, device=dev)
    d_tot = t.full((6 + PAD,), 0x5A5A5A5A, dtype=t.int32, device=dev)
    sh = t.cuda.current_stream(dev).cuda_stream
    ctx.l2_dev(d_pk, d_off, d_ln, n, unit, d_v, p, d_st[skew:], d_out, cap, d_ro, d_rl, d_rs, d_tot,
               stream=sh)
    t.cuda.synchronize(dev)
    tot = d_tot.cpu().numpy().view(np.uint32)
    assert np.all(tot[6:] == 0x5A5A5A5A)
    st = d_st.cpu().numpy()
    assert np.all(st[:skew] == CANARY)
    return (st[skew:], d_out.cpu().numpy(), d_ro.cpu().numpy().view(np.uint32),
            d_rl.cpu().numpy().view(np.uint16), d_rs.cpu().numpy().view(np.uint32), tot[:6].copy())


def _check(torch_dev, ctx, frames, caps, v, unit, cap=BIG, local=M.LOCALS, skew=0, model=False):
    """the device against the host form (and, model=True, the model)"""
    buf, off, lens = F.pack_frames(frames, unit, caps)
    p = R.l2_params(local)
    want = R.l2_host(buf, off, lens, unit, v, p, cap)
    want = (want[0], want[1].tobytes(), *want[2:])
    got = _dev_run(torch_dev, ctx, buf, off, lens, unit, v, p, cap, skew)
    C.compare(got, want, len(frames))
    if model:
        C.compare(got, M.run(buf, off, lens, unit, v, local, cap), len(frames))
    return want


SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 4099]
KINDS = {"mixed": 0, "arp": 1, "echo": 2, "none": 3}
_bursts = {}


def _burst(kind, n, unit):
    """fuzzed and classified once per (kind, n, unit)"""
    if (kind, n, unit) not in _bursts:
        frames, caps = M.fuzz_burst(9000 + n + KINDS[kind], n, kind)
        _bursts[kind, n, unit] = frames, caps, C.classify(frames, caps, unit)
    return _bursts[kind, n, unit]


@pytest.mark.parametrize("unit", [4, 6])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_host(torch_dev, ctx, n, kind, unit):
    frames, caps, v = _burst(kind, n, unit)
    st, _, _, _, _, tot = _check(torch_dev, ctx, frames, caps, v, unit, model=n in (257, 1025))
    if kind == "arp":
        assert tot[0] == tot[4] == tot[5] == n and np.all(st == M.ARP_REQ)
    if kind == "echo":
        assert tot[2] == tot[4] == n and np.all(st == M.ECHO)
    if kind == "none":
        assert not tot.any() and not st.any()
    if kind == "mixed" and n >= 255:
        assert set(st) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_status_bytes_at_an_unaligned_address(torch_dev, ctx, skew):
    frames, caps, v = _burst("mixed", 257, 6)
    _check(torch_dev, ctx, frames, caps, v, 6, skew=skew)


@pytest.mark.parametrize("unit", [4, 6])
def test_hand_cases(torch_dev, ctx, unit):
    cases, frames, caps, v = C.hand_burst()
    want = _check(torch_dev, ctx, frames, caps, v, unit, model=True)
    assert [int(s) for s in want[0]] == [c[4] for c in cases]
    ans = {int(i): want[1][64 * int(o):64 * int(o) + int(n)] for o, n, i in zip(want[2], want[3], want[4])}
    for i, c in enumerate(cases):
        if c[5] is not None:
            assert ans[i] == c[5], c[0]


def test_300_echo_requests_of_1472_bytes(torch_dev, ctx):
    """1514-byte answers: emit crosses many 64-B slots, the layout crosses a tile"""
    rng = np.random.default_rng(5)
    frames = [M.echo(bytes(rng.integers(0, 256, 1472, dtype=np.uint8)), "10.3.%d.9" % (k % 250 + 1),
                     ident=k, seq=3 * k) for k in range(300)]
    caps = [len(f) for f in frames]
    tot = _check(torch_dev, ctx, frames, caps, M.verdicts([M.CLS_IPV4_OTHER] * 300), 4, model=True)[5]
    assert tot[2] == tot[4] == 300 and tot[5] == 300 * 24


def test_cap_bytes_one_byte_short(torch_dev, ctx):
    frames, caps, v = _burst("mixed", 1025, 6)
    full = _check(torch_dev, ctx, frames, caps, v, 6)
    ends = (full[2].astype(np.int64) + (full[3].astype(np.int64) + 63) // 64) * 64
    assert len(ends) > 300
    for k in (0, 1, 100, 257, len(ends) - 1):             # in the first tile, behind it, the last
        cut = _check(torch_dev, ctx, frames, caps, v, 6, cap=int(ends[k]) - 1)
        assert cut[5][4] == k and cut[0].tobytes() == full[0].tobytes()
        assert _check(torch_dev, ctx, frames, caps, v, 6, cap=int(ends[k]))[5][4] == k + 1
    assert _check(torch_dev, ctx, frames, caps, v, 6, cap=63)[5][4] == 0


def test_arguments(torch_dev, ctx):
    t, dev = torch_dev
    cases, frames, caps, v = C.hand_burst()
    assert not _check(torch_dev, ctx, frames, caps, v, 6, local=[])[0].any()
    d = t.zeros(256, dtype=t.uint8, device=dev)
    p, nine = R.l2_params(M.LOCALS), R.l2_params(M.LOCALS)
    nine["nlocal"] = 9
    for bad in (dict(p=nine), dict(st=None), dict(out=None), dict(ro=None), dict(rl=None), dict(rs=None),
                dict(tot=None), dict(out=d.data_ptr() + 16), dict(unit=3)):
        with pytest.raises(R.RxgError) as e:
            ctx.l2_dev(d, d, d, 1, bad.get("unit", 6), d, bad.get("p", p), bad.get("st", d),
                       bad.get("out", d), 64, bad.get("ro", d), bad.get("rl", d), bad.get("rs", d),
                       bad.get("tot", d))
        assert e.value.rc == -22, bad
    tot = t.full((6,), 7, dtype=t.int32, device=dev)                 # n == 0: the totals zeroed
    ctx.l2_dev(None, None, None, 0, 6, None, p, d, d, 64, d, d, d, tot)
    t.cuda.synchronize(dev)
    assert not tot.cpu().numpy().any() and not d.cpu().numpy().any()


# ---- through the delivery pipeline -------------------------------------------------------
def _tables():
    udp = np.zeros(1, R.UDP_SOCK_DTYPE)
    udp[0]["localip"], udp[0]["localport"], udp[0]["protocol"] = R.ip_raw(CK.LOCAL), R.port_raw(5000), 17
    tcb = np.zeros(3, R.TCB_DTYPE)
    tcb[0] = (R.ip_raw("10.9.0.1"), R.ip_raw(CK.LOCAL), R.port_raw(40000), R.port_raw(9999), 4)
    tcb[1] = (0, R.ip_raw(CK.LOCAL), 0, R.port_raw(8080), R.TCP_STATUS_LISTEN)
    tcb[2] = (0, R.ip_raw(CK.LOCAL), 0, R.port_raw(8081), R.TCP_STATUS_LISTEN)
    return udp, tcb


_dlv = []


def _delivery_bursts():
    """two bursts: SYNs, ACKs, data of an established connection and
    datagrams, with ARP and echo traffic of every kind between them"""
    if not _dlv:
        rng = np.random.default_rng(78)
        for b in range(2):
            fr, seq = [], 1000 + 700 * b
            l2 = [f[:c] for f, c in zip(*M.fuzz_burst(500 + b, 150 + 20 * b))]   # (captures cut for real)
            for j in range(300 + 37 * b):
                src, sport, isn = "10.%d.%d.7" % (1 + b, 1 + j % 200), 2000 + j, int(rng.integers(1 << 32))
                k = j % 4
                if k == 0:
                    fr.append(CK.syn(src, sport, 8080 + (j & 2) // 2, isn))
                elif k == 1:
                    fr.append(F.udp_frame(src, sport, CK.LOCAL, 5000, bytes(rng.integers(0, 256, 30, dtype=np.uint8))))
                elif k == 2:
                    fr.append(F.tcp_frame("10.9.0.1", 40000, CK.LOCAL, 9999,
                                          bytes(rng.integers(0, 256, 100, dtype=np.uint8)), seq=seq))
                    seq += 100
                else:
                    fr.append(CK.ack_for(src, sport, 8080, isn, 5, payload=b"pig" * (j % 3), flags=0x18))
                if j % 2 == 0 and l2:
                    fr.append(l2.pop())
            fr[10], fr[22] = fr[22], fr[10]
            _dlv.append(fr)
    return _dlv


L2_CAP = 1 << 16


def _deliver_all(flags, pipelined):
    """every burst through the delivery pipeline: per burst the results as
    bytes, the L2 results and the verdicts"""
    results, l2s = [], []
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as c:
        c.flows_sync(*_tables())
        c.tune_deliver(flags)
        c.l2_set(R.l2_params(M.LOCALS), L2_CAP)
        c.syncookie_set(R.ck_params(CK.KEY, 5), [1, 2])

        def keep(res, l2):
            out, dg, first, up, seg, tp, _ = res
            results.append(tuple(x.tobytes() for x in (out, dg, first, up, seg, tp)))
            l2s.append((l2, out.copy()))
        bursts = [R.NStack.mbufs(b) for b in _delivery_bursts()]
        if pipelined:
            hs = [c.deliver_submit(arr) for arr, _ in bursts]
            for h in hs:
                keep(c.deliver_wait(h), c.delivery_l2(h))
        else:
            for arr, _ in bursts:
                keep(c.process_mbufs_deliver(arr), c.delivery_l2())
    return results, l2s


def _check_l2(l2s):
    for fr, (got, out) in zip(_delivery_bursts(), l2s):
        buf, off, lens = F.pack_frames(fr, 6)
        assert list(out["cls"]) == list(C.classify(fr, [len(f) for f in fr], 6)["cls"])
        want = R.l2_host(buf, off, lens, 6, out, R.l2_params(M.LOCALS), L2_CAP)
        assert list(got[5]) == list(want[5]) and want[5][0] > 5 and want[5][2] > 10 and want[5][3] > 3
        for g, w in zip(got[:5], want[:5]):
            assert g.tobytes() == w.tobytes()
        model = M.run(buf, off, lens, 6, out, M.LOCALS, L2_CAP)
        assert got[1].tobytes() == model[1] and got[0].tobytes() == model[0].tobytes()


@pytest.mark.parametrize("pipelined", [False, True], ids=["one", "two_in_flight"])
def test_delivery_pipeline(torch_dev, pipelined):
    base, none = _deliver_all(0, pipelined)
    assert all(all(x is None for x in l2[:5]) and not l2[5].any() for l2, _ in none)
    got, l2s = _deliver_all(R.DLV_L2, pipelined)
    assert got == base                                   # verdicts, records, payloads: nothing changes
    assert any(len(r[4]) for r in base) and any(len(r[1]) for r in base)
    _check_l2(l2s)


def test_delivery_pipeline_with_assembly_the_detector_and_cookies(torch_dev):
    fl = R.DLV_TCP_ASSEMBLE | R.DLV_DDOS | R.DLV_SYNCOOKIE
    base, _ = _deliver_all(fl, True)
    got, l2s = _deliver_all(fl | R.DLV_L2, True)
    assert got == base
    _check_l2(l2s)


def test_delivery_without_l2_set_and_with_no_room(torch_dev):
    fr = _delivery_bursts()[0]
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as c:
        c.flows_sync(*_tables())
        c.tune_deliver(R.DLV_L2)
        arr, _keep = R.NStack.mbufs(fr)
        c.process_mbufs_deliver(arr)
        st, frames, roff, rlen, rsrc, tot = c.delivery_l2()
        assert len(st) == len(fr) and not st.any() and not tot.any() and len(frames) == 0
        c.l2_set(R.l2_params(M.LOCALS), 0)
        c.process_mbufs_deliver(arr)
        st, frames, roff, rlen, rsrc, tot = c.delivery_l2()
        assert st.any() and tot[0] and tot[2] and tot[4] == 0 and tot[5] == 0 and len(roff) == 0


# ---- the socket layer on the GPU paths ------------------------------------------------
@pytest.mark.parametrize("encode", [False, True], ids=["host_frames", "k5"])
@pytest.mark.parametrize("mode", ["gpu", "pipe"])
def test_socket_layer(torch_dev, mode, encode):
    ns = R.NStack(0)
    try:
        log = M.scenario(ns, mode, encode=encode)
        if encode:
            assert ns.stat(13) == 2                      # the two datagrams came from K5
    finally:
        ns.fini()
    M.check_scenario(log)


def test_socket_layer_option_off(torch_dev):
    ns = R.NStack(0)
    try:
        log = M.scenario(ns, "gpu", on=False)
    finally:
        ns.fini()
    M.check_scenario(log, on=False)
