"""The entropy flood detector on the GPU (K6, csrc/rx_ddos.hip, rxg_ddos_dev)
against rxg_ddos_host and the numpy model of tests/ddos_ref.py: bits, flags,
summary and the device state byte for byte (the summary's last D and the
per-frame D within the derived tolerance of tests/test_rx_ddos.py, NaN at the
same frames), a 0xA5 canary past n in every output.  Each lanes-per-frame
variant of the bits pass forced and auto; the burst in splits with the device
state carried; the length list with 0xFF between the frames; n around the
window and around the window pass's tile; nullable outputs; 1500-B and
mixed-size bursts; then the delivery pipeline with RXG_DLV_DDOS (one burst,
two in flight, with coalescing and ordering) and the socket layer through
nstack_rx_burst and nstack_rx_submit / nstack_rx_complete."""
import numpy as np
import pytest

import ddos_ref as M
import frames as F
import rxgpu as R
import test_rx_ddos as C

pytestmark = pytest.mark.gpu
CANARY = 0xA5
PAD = 16                                       # canary entries past n
T = R.DDOS_TILE
L = M.SOCK_L


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


class Dev:
    """a packed burst on the device and one detector state"""

    def __init__(self, torch_dev, buf, off, lens, unit):
        self.torch, self.dev = torch_dev
        t = self.torch
        self.unit = unit
        self.off, self.lens = off, lens
        self.d_pk = t.from_numpy(buf).to(self.dev)
        self.d_off = t.from_numpy(off.view(np.int32)).to(self.dev)
        self.d_ln = t.from_numpy(lens.view(np.int16)).to(self.dev)
        self.d_state = t.zeros(R.DDOS_STATE_DTYPE.itemsize, dtype=t.uint8, device=self.dev)

    def state(self):
        return self.d_state.cpu().numpy().view(R.DDOS_STATE_DTYPE)

    def run(self, ctx, a, n, thresh=1200.0, len_hint=64, outs=("bits", "flag", "stat")):
        """frames a .. a+n through rxg_ddos_dev: (bits, flag, stat, summary),
        None for an output passed as NULL; the canaries are checked here"""
        t = self.torch
        size = {"bits": 4, "flag": 1, "stat": 8}
        d = {k: t.full((size[k] * (n + PAD),), CANARY, dtype=t.uint8, device=self.dev) for k in outs}
        d_sum = t.full((R.DDOS_SUMMARY_DTYPE.itemsize + PAD,), CANARY, dtype=t.uint8, device=self.dev)
        sh = t.cuda.current_stream(self.dev).cuda_stream
        ctx.ddos_dev(self.d_pk, self.d_off[a:] if n else None, self.d_ln[a:] if n else None, n,
                     self.unit, len_hint, thresh, self.d_state, d.get("bits"), d.get("flag"),
                     d.get("stat"), d_sum, stream=sh)
        t.cuda.synchronize(self.dev)
        out = {}
        for k in ("bits", "flag", "stat"):
            if k not in d:
                out[k] = None
                continue
            h = d[k].cpu().numpy()
            assert np.all(h[size[k] * n:] == CANARY), k
            out[k] = h[:size[k] * n].view({"bits": np.uint32, "flag": np.uint8, "stat": np.float64}[k])
        hs = d_sum.cpu().numpy()
        assert np.all(hs[R.DDOS_SUMMARY_DTYPE.itemsize:] == CANARY)
        return out["bits"], out["flag"], out["stat"], hs[:48].view(R.DDOS_SUMMARY_DTYPE)[0]


def _check(got, host, res, st, thresh=1200.0):
    """the device's outputs against the model (C._compare) and, byte for byte,
    rxg_ddos_host's (the summary but for its last D)"""
    C._compare(got, res, st, thresh)
    hb, hf, _, hsum = host
    assert got[0].tobytes() == hb.tobytes() and got[1].tobytes() == hf.tobytes()
    for k in R.DDOS_SUMMARY_DTYPE.names:
        if k != "last_stat":
            assert got[3][k] == hsum[k], k


def _both(torch_dev, ctx, frames, unit, cuts, g, thresh=1200.0, len_hint=64):
    """frames through the device, the host call and the model in the same
    cuts, everything compared after each; returns the device flags"""
    buf, off, lens = M.pack(frames, unit)
    st, tt = M.frame_bits(buf, off, lens, unit)
    x = Dev(torch_dev, buf, off, lens, unit)
    hstate = np.zeros(1, R.DDOS_STATE_DTYPE)
    m = M.Model()
    ctx.tune_ddos(g)
    flags = []
    a = 0
    try:
        for n in cuts:
            sl = slice(a, a + n)
            res = m.run(st[sl], tt[sl], thresh)
            hb, hf, hs, hsum, _ = R.ddos_host(buf, off[sl], lens[sl], unit, thresh, hstate)
            got = x.run(ctx, a, n, thresh, len_hint)
            _check(got, (hb, hf, hs, hsum), res, st[sl], thresh)
            assert x.state().tobytes() == hstate.tobytes() == m.state().tobytes()
            flags.append(got[1])
            a += n
    finally:
        ctx.tune_ddos(0)
    assert a == len(frames)
    return np.concatenate(flags) if flags else np.zeros(0, np.uint8)


@pytest.mark.parametrize("g", (0,) + R.DDOS_LANES)
def test_main_burst_each_lane_count(torch_dev, ctx, g):
    flags = _both(torch_dev, ctx, M.main_burst(), 6, (1300,), g)
    assert M.events(flags) == [(256, "rise"), (304, "fall"), (951, "rise"), (1000, "fall"), (1256, "rise")]


@pytest.mark.parametrize("split", C.SPLITS[:2])
def test_main_burst_in_splits_with_the_device_state_carried(torch_dev, ctx, split):
    flags = _both(torch_dev, ctx, M.main_burst(), 6, split, 0)
    assert np.array_equal(flags, C._main()[5]["flags"])


@pytest.mark.parametrize("unit", [4, 6])
@pytest.mark.parametrize("g", R.DDOS_LANES)
def test_lengths_each_lane_count(torch_dev, ctx, g, unit):
    frames = C.length_case(unit)
    _both(torch_dev, ctx, frames, unit, (len(frames),), g, len_hint=0)


def varied(seed, n, nbytes=64):
    """n frames: 0.5 bit density, alternating 0.15 / 0.85 in every other run
    of 400 frames: the alarm rises at frame 256, falls soon after frame 400,
    rises again some 256 frames after frame 800, ..."""
    rng = np.random.default_rng(seed)
    return [M.density_frame(rng, nbytes, 0.5 if (j // 400) % 2 == 0 else (0.15 if j & 1 else 0.85))
            for j in range(n)]


@pytest.mark.parametrize("n", sorted({1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 255, 4 * T + 255}))
def test_burst_sizes_around_the_window_and_the_tile(torch_dev, ctx, n):
    """each size twice: on a fresh state, then on the carried one (the halo of
    the first tile comes from the state's slots)"""
    flags = _both(torch_dev, ctx, varied(n, 2 * n), 6, (n, n), 0)
    if 2 * n > 500:
        assert (flags & R.DDOS_RISE).any() and (flags & R.DDOS_FALL).any()


def test_nullable_outputs_and_arguments(torch_dev, ctx):
    frames = M.main_burst()[:700]
    buf, off, lens = M.pack(frames, 6)
    st, tt = M.frame_bits(buf, off, lens, 6)
    res = M.Model().run(st, tt)
    want_state = None
    for outs in ((), ("bits",), ("flag",), ("stat",), ("bits", "flag", "stat")):
        x = Dev(torch_dev, buf, off, lens, 6)
        b, f, d, summ = x.run(ctx, 0, 700, outs=outs)
        M.check_summary(summ, res["summary"])
        assert abs(summ["last_stat"] - res["summary"]["last_stat"]) <= res["tol"][-1]
        assert (b is None) == ("bits" not in outs) and (b is None or np.array_equal(b, st))
        assert (f is None) == ("flag" not in outs) and (f is None or np.array_equal(f, res["flags"]))
        assert (d is None) == ("stat" not in outs)
        want_state = want_state or x.state().tobytes()
        assert x.state().tobytes() == want_state
    # n = 0: the state stays, the summary is written
    b, f, d, summ = x.run(ctx, 0, 0)
    assert x.state().tobytes() == want_state
    assert summ["frames_seen"] == 700 and summ["first_alarm"] == 0xFFFFFFFF and summ["alarm_frames"] == 0
    assert summ["flag"] == res["summary"]["flag"] and np.isnan(summ["last_stat"])
    t = x.torch
    d_sum = t.zeros(64, dtype=t.uint8, device=x.dev)
    for unit, thresh, state, dsum in ((3, 1200.0, x.d_state, d_sum), (6, float("nan"), x.d_state, d_sum),
                                      (6, 1200.0, None, d_sum), (6, 1200.0, x.d_state, None)):
        with pytest.raises(R.RxgError) as e:
            ctx.ddos_dev(x.d_pk, x.d_off, x.d_ln, 10, unit, 64, thresh, state, None, None, None, dsum)
        assert e.value.rc == -22
    assert x.state().tobytes() == want_state


@pytest.mark.parametrize("kind", ["1500", "mixed"])
def test_large_and_mixed_frames(torch_dev, ctx, kind):
    """about 600 frames of 1500 B (in 1536-B slots), or of mixed sizes, payload
    densities as in `varied`; the threshold at the model's median so that both
    alarm states occur whatever the sizes do to D"""
    rng = np.random.default_rng(17)
    sizes = [1500] * 600 if kind == "1500" else \
        [int(x) for x in rng.choice([60, 64, 65, 128, 590, 1500, 1514, 4000], 600)]
    frames = [M.density_frame(rng, nb, 0.5 if (j // 150) % 2 == 0 else (0.15 if j & 1 else 0.85))
              for j, nb in enumerate(sizes)]
    buf, off, lens = M.pack(frames, 6)
    thresh = C.median_threshold(*M.frame_bits(buf, off, lens, 6))
    for g in (0, 1, 64):
        flags = _both(torch_dev, ctx, frames, 6, (600,), g, thresh, len_hint=1500 if kind == "1500" else 0)
        assert (flags & R.DDOS_RISE).any() and (flags & R.DDOS_FALL).any()


# ---- the delivery pipeline -----------------------------------------------------
def _delivery_bursts():
    """M.socket_bursts with a TCP segment of one of two connections after
    every fourth frame (in sequence but for one swapped pair per burst, so
    ordering and coalescing have work)"""
    rng = np.random.default_rng(23)
    seq = [1000, 5000]
    out = []
    for fr in M.socket_bursts():
        b = []
        for j, f in enumerate(fr):
            b.append(f)
            if j % 4 == 3:
                k = (j >> 2) & 1
                b.append(F.tcp_frame("10.9.0.%d" % (k + 1), 40000 + k, L, 9999, M.density_frame(rng, 100, 0.5),
                                     seq=seq[k]))
                seq[k] += 100
        b[7], b[17] = b[17], b[7]                  # (both of connection 1)
        out.append(b)
    return out


def _tables():
    udp = np.zeros(1, R.UDP_SOCK_DTYPE)
    udp[0]["localip"], udp[0]["localport"], udp[0]["protocol"] = R.ip_raw(L), R.port_raw(M.SOCK_PORT), 17
    tcb = np.zeros(2, R.TCB_DTYPE)
    for k in range(2):
        tcb[k] = (R.ip_raw("10.9.0.%d" % (k + 1)), R.ip_raw(L), R.port_raw(40000 + k), R.port_raw(9999), 4)
    return udp, tcb


def _deliver_all(flags, pipelined, thresh=1200.0):
    """every burst through the delivery pipeline: per burst the results as
    bytes and the detector's summary"""
    results, summaries = [], []
    with R.Context(0, max_pkts=1024, max_bytes=1 << 21) as ctx:
        ctx.flows_sync(*_tables())
        ctx.tune_deliver(flags)
        ctx.tune_ddos(0, thresh)

        def keep(res, summ):
            out, dg, first, up, seg, tp, _ = res
            results.append(tuple(x.tobytes() for x in (out, dg, first, up, seg, tp)))
            summaries.append(summ.copy())
        bursts = [R.NStack.mbufs(b) for b in _delivery_bursts()]
        if pipelined:
            hs = []
            for k, (arr, _) in enumerate(bursts):
                hs.append(ctx.deliver_submit(arr))
                if k:
                    h = hs[k - 1]
                    keep(ctx.deliver_wait(h), ctx.delivery_ddos(h))
            keep(ctx.deliver_wait(hs[-1]), ctx.delivery_ddos(hs[-1]))
        else:
            for arr, _ in bursts:
                keep(ctx.process_mbufs_deliver(arr), ctx.delivery_ddos())
        if flags & R.DLV_DDOS:                         # a reset state starts again
            ctx.ddos_reset()
            ctx.process_mbufs_deliver(bursts[0][0])
            assert ctx.delivery_ddos()["frames_seen"] == len(_delivery_bursts()[0])
    return results, summaries


def _check_summaries(summaries, thresh=1200.0):
    m = M.Model()
    rises = 0
    for b, summ in zip(_delivery_bursts(), summaries):
        res = m.run(*M.frames_bits(b), thresh)
        assert M.margin_ok(res, thresh)
        M.check_summary(summ, res["summary"])
        if not np.isnan(res["summary"]["last_stat"]):
            assert abs(summ["last_stat"] - res["summary"]["last_stat"]) <= res["tol"][-1]
        rises += res["summary"]["rises"]
    assert rises >= 2


@pytest.mark.parametrize("pipelined", [False, True], ids=["one", "two_in_flight"])
def test_delivery_pipeline(torch_dev, pipelined):
    base, zero = _deliver_all(0, pipelined)
    assert all(s.tobytes() == bytes(48) for s in zero)               # zeroed with the flag off
    got, summaries = _deliver_all(R.DLV_DDOS, pipelined)
    assert got == base                                                # detection only
    assert any(len(r[4]) for r in base) and any(len(r[1]) for r in base)
    _check_summaries(summaries)


def test_delivery_pipeline_with_coalescing_and_ordering(torch_dev):
    fl = R.DLV_TCP_GRO | R.DLV_TCP_ORDER
    base, _ = _deliver_all(fl, True)
    got, summaries = _deliver_all(fl | R.DLV_DDOS, True)
    assert got == base
    _check_summaries(summaries)


# ---- the socket layer on the GPU path ------------------------------------------
@pytest.mark.parametrize("mode", ["gpu", "pipe"])
def test_socket_layer(torch_dev, mode):
    runs = {}
    for on in (False, True):
        ns = R.NStack(0)
        try:
            runs[on] = C.socket_session(ns, mode, on)
        finally:
            ns.fini()
    assert runs[True][0] == runs[False][0]                           # detection only
    assert any(x[0] == "burst" and x[1] > 0 for x in runs[True][0])
    C.check_socket_status(runs[True][1])
