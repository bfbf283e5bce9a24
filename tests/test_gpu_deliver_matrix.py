"""The delivery pipeline (rxg_deliver_submit / _wait) under every valid
combination of its flags: the eight TCP forms (plain, in place, coalesced,
ordered, ordered + coalesced, ordered + in place, assembled, assembled +
ordered) times the detector, SYN cookies and the L2 responder on or off.

Three small mixed bursts (datagrams for a bound socket, two established
connections with one swapped pair and one duplicate per burst, SYNs and cookie
ACKs for two listeners, ARP and echo traffic) go through
  (1) a fresh context per combination, two bursts in flight: every pass's
      results equal, byte for byte, its results under the combination that
      has only its own flags (one burst at a time, a context of its own); a
      pass whose flag is off returns its documented empty result;
  (2) the single-pass results against the oracle's verdicts, compact_ref,
      gro_ref / order_ref / assemble_ref and the *_host forms, ddos_ref and
      rxg_ddos_host, rxg_syncookie_host and cookie_ref, rxg_l2_host and l2_ref,
      so that (1) is no equality of two wrong things;
  (3) one context through all 64 combinations in a fixed shuffled order, two
      bursts in flight, rxg_l2_set raising the answer capacity and rxg_tune_gro
      changing the window on the way: every result equals the fresh context's
      (the late first use of a pass, the L2 buffers' regrow, reused sets and
      pooled payload buffers);
  (4) a zero-frame burst between real ones: the following burst's results do
      not change and the empty burst's handle reads as empty."""
import functools
import itertools
import random

import numpy as np
import pytest

import assemble_ref as A
import compact_ref as K
import cookie_ref as CK
import ddos_ref as DD
import frames as F
import gro_ref as G
import l2_ref as M
import oracle_bind as O
import order_ref as D
import rxgpu as R

pytestmark = pytest.mark.gpu

T = 5                                   # the cookie time counter
THRESH = 1200.0
W_SMALL = 256                           # a window the 100-byte segments cross
CAP_SMALL, CAP_BIG = 1024, 4096         # answer room: the small one cuts answers the big one holds
GRO, ORDER, INPLACE, ASM = R.DLV_TCP_GRO, R.DLV_TCP_ORDER, R.DLV_TCP_IN_PLACE, R.DLV_TCP_ASSEMBLE
FORMS = {"plain": 0, "in_place": INPLACE, "gro": GRO, "order": ORDER, "order_gro": ORDER | GRO,
         "order_in_place": ORDER | INPLACE, "assemble": ASM, "assemble_order": ASM | ORDER}
SIDES = [d | k | l for d in (0, R.DLV_DDOS) for k in (0, R.DLV_SYNCOOKIE) for l in (0, R.DLV_L2)]
NO_CK = (None, None, bytes(16))
NO_L2 = (None, None, None, None, None, bytes(24))


@pytest.fixture(scope="module", autouse=True)
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test needs a GPU (no fallback path exists)")


def _tables():
    udp = np.zeros(1, R.UDP_SOCK_DTYPE)
    udp[0]["localip"], udp[0]["localport"], udp[0]["protocol"] = R.ip_raw(CK.LOCAL), R.port_raw(5000), 17
    tcb = np.zeros(4, R.TCB_DTYPE)
    tcb[0] = (R.ip_raw("10.9.0.1"), R.ip_raw(CK.LOCAL), R.port_raw(40000), R.port_raw(9999), 4)
    tcb[1] = (0, R.ip_raw(CK.LOCAL), 0, R.port_raw(8080), R.TCP_STATUS_LISTEN)
    tcb[2] = (0, R.ip_raw(CK.LOCAL), 0, R.port_raw(8081), R.TCP_STATUS_LISTEN)
    tcb[3] = (R.ip_raw("10.9.0.2"), R.ip_raw(CK.LOCAL), R.port_raw(40001), R.port_raw(9999), 4)
    return udp, tcb


@functools.lru_cache(maxsize=None)
def _bursts():
    """three bursts of 16, 15 and 17 rounds of {SYN, datagram, data of
    connection 0, cookie ACK, an ARP / echo frame of l2_ref's fuzzer, data of
    connection 1}; per burst two data frames of connection 0 swapped and one
    sent twice.  291 frames in all, so the last burst leaves the detector's
    256-frame warm-up"""
    rng = np.random.default_rng(64)
    out = []
    for b, rounds in enumerate((16, 15, 17)):
        fr, seq = [], [1000 + 5000 * b, 77000 + 5000 * b]
        l2 = [f[:c] for f, c in zip(*M.fuzz_burst(640 + b, rounds))]      # (captures cut for real)
        for j in range(rounds):
            src, sport, isn = "10.%d.%d.7" % (1 + b, 1 + j), 2000 + j, int(rng.integers(1 << 32))
            fr.append(CK.syn(src, sport, 8080 + (j & 1), isn))
            fr.append(F.udp_frame(src, sport, CK.LOCAL, 5000, bytes(rng.integers(0, 256, 30 + j, dtype=np.uint8))))
            for k in (0, 1):
                if k:
                    fr.append(CK.ack_for(src, sport, 8080, isn, T - j % 2, payload=b"pig" * (j % 3), flags=0x18,
                                         dack=j % 5 == 4))
                    fr.append(l2[j])
                fr.append(F.tcp_frame("10.9.0.%d" % (1 + k), 40000 + k, CK.LOCAL, 9999,
                                      bytes(rng.integers(0, 256, 100, dtype=np.uint8)), seq=seq[k]))
                seq[k] += 100
        data0 = [i for i in range(len(fr)) if i % 6 == 2]
        fr[data0[3]], fr[data0[5]] = fr[data0[5]], fr[data0[3]]
        fr.insert(data0[9], fr[data0[7]])
        out.append(fr)
    return out


@functools.lru_cache(maxsize=None)
def _mbufs():
    return [R.NStack.mbufs(b) for b in _bursts()]


def _open(flags, W=0, cap=CAP_BIG):
    c = R.Context(0, max_pkts=256, max_bytes=1 << 19)
    c.flows_sync(*_tables())
    c.tune_deliver(flags)
    c.tune_ddos(0, THRESH)
    c.tune_gro(W)
    c.l2_set(R.l2_params(M.LOCALS), cap)
    c.syncookie_set(R.ck_params(CK.KEY, T), [1, 2])
    return c


def _collect(c, h):
    """the results of a submitted burst, every accessor's with them"""
    out, dg, first, up, seg, tp, _ = c.deliver_wait(h)
    return dict(common=(out, dg, first, up),
                tcp=(seg, tp, c.delivery_runs(h), c.delivery_streams(h), c.delivery_moved(h)),
                ddos=c.delivery_ddos(h).tobytes(), ck=c.delivery_cookies(h), l2=c.delivery_l2(h))


def _bytes(x):
    if isinstance(x, (tuple, list)):
        return tuple(_bytes(y) for y in x)
    return x.tobytes() if isinstance(x, (np.ndarray, np.void)) else x


def _deliver(c, in_flight, bursts=None):
    """the bursts through c: one at a time, or with two in flight"""
    arrs = [a for a, _ in _mbufs()] if bursts is None else bursts
    if not in_flight:
        return [_collect(c, c.deliver_submit(a)) for a in arrs]
    res, hs = [], []
    for a in arrs:
        hs.append(c.deliver_submit(a))
        if len(hs) == 2:
            res.append(_collect(c, hs.pop(0)))
    return res + [_collect(c, h) for h in hs]


@functools.lru_cache(maxsize=None)
def _alone_once(flags, W, cap):
    with _open(flags, W, cap) as c:
        return _deliver(c, False)


def _alone(flags, W=0, cap=CAP_BIG):
    """the bursts through a fresh context that has these flags only, one at a
    time (run once per (flags, W, cap) and shared)"""
    return _alone_once(flags, W, cap)


def _want(flags, W, cap):
    """per burst what a context with `flags` must return: every pass's part
    from the context that ran that pass alone"""
    form = flags & (GRO | ORDER | INPLACE | ASM)
    res = []
    for b in range(len(_bursts())):
        res.append(dict(
            common=_alone(0)[b]["common"], tcp=_alone(form, W if form & GRO else 0)[b]["tcp"],
            ddos=_alone(R.DLV_DDOS)[b]["ddos"] if flags & R.DLV_DDOS else bytes(48),
            ck=_alone(R.DLV_SYNCOOKIE)[b]["ck"] if flags & R.DLV_SYNCOOKIE else NO_CK,
            l2=_alone(R.DLV_L2, 0, cap)[b]["l2"] if flags & R.DLV_L2 else NO_L2))
    return res


def _same(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        for part in ("common", "tcp", "ddos", "ck", "l2"):
            assert _bytes(g[part]) == _bytes(w[part]), (what, "burst", b, part)


# ---- (1) independence ------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_every_pass_is_independent_of_the_other_flags(form):
    for side in SIDES:
        flags = FORMS[form] | side
        with _open(flags) as c:
            _same(_deliver(c, True), _want(flags, 0, CAP_BIG), hex(flags))


# ---- (2) the single-pass results against the models and host forms -------------------------
def _packed(b):
    fr = _bursts()[b]
    return fr, [len(f) for f in fr], F.pack_frames(fr, 6)


@functools.lru_cache(maxsize=None)
def _verdicts(b):
    _, _, (buf, off, lens) = _packed(b)
    return O.Tables(*_tables()).classify(buf, off, lens, 6)


def test_verdicts_and_datagrams_are_the_oracles_and_compact_refs():
    for b, res in enumerate(_alone(0)):
        fr, caps, _ = _packed(b)
        out, dg, first, up = res["common"]
        v = _verdicts(b)
        assert out.tobytes() == v.tobytes()
        want = K.compact(fr, caps, v, 1)
        assert len(want.dgram) >= 15
        assert dg.tobytes() == want.dgram.tobytes() and first.tobytes() == want.first.tobytes()
        assert up.tobytes() == want.payload.tobytes()
        assert _bytes(res["tcp"][2:]) == (b"", b"", 0) and res["ddos"] == bytes(48)
        assert _bytes(res["ck"]) == NO_CK and _bytes(res["l2"]) == NO_L2


def _records(b):
    fr, caps, _ = _packed(b)
    v = _verdicts(b)
    flows = [int(x["flow_id"]) if x["cls"] == R.CLS_TCP and x["rc"] == 0 and x["flow_id"] < 4 else None
             for x in v]
    return G.records(fr, caps, flows)


def _pad16(x):
    return (x.astype(np.int64) + 15) // 16 * 16


def _check_tcp(b, flags, W, tcp):
    fr, caps, _ = _packed(b)
    seg, tp, run, st, moved = tcp
    seg0, sip0 = _records(b)
    assert len(seg0) >= 60 and {0, 1, 2, 3} == set(seg0["flow"])
    perm, wmoved = np.arange(len(seg0)), 0
    if flags & (ORDER | ASM):
        perm, wmoved = D.order_model(seg0, sip0)
        hperm, hmoved = R.tcp_order_host(seg0, sip0)
        assert np.array_equal(perm, hperm) and wmoved == hmoved and wmoved > 0
    want, wsip = seg0[perm].copy(), sip0[perm]
    assert moved == wmoved
    if flags & ASM:
        m = A.assemble_model(want, wsip, A.avail_of(want, caps))
        hst, hskip, htake, hdst = R.tcp_assemble_host(want, wsip, A.avail_of(want, caps))
        assert hst.tobytes() == m["stream"].tobytes() and np.array_equal(htake, m["take"])
        assert np.array_equal(hdst, m["dst"]) and m["skip"].sum() >= 100       # (the duplicate)
        img, used, over = A.payload_image(fr, want, m, 1 << 17, 1 << 17, 0)
        want["ncopy"], want["offset"] = m["take"], m["dst"]
        assert seg.tobytes() == want.tobytes() and st.tobytes() == m["stream"].tobytes()
        assert len(run) == 0 and len(tp) == used and not over
        for s in st:
            o, nb = int(s["offset"]), int(s["bytes"])
            assert tp[o:o + nb].tobytes() == img[o:o + nb].tobytes()
        return
    assert len(st) == 0
    for name in R.SEGMENT_DTYPE.names:
        if name != "offset":
            assert np.array_equal(seg[name], want[name]), name
    if flags & INPLACE:
        assert len(tp) == 0 and len(run) == 0
        assert np.array_equal(seg["offset"], 34 + 4 * seg["hl"].astype(np.uint32))
        return
    for g in seg:                                # every payload, straight from its frame
        o, a, n = int(g["offset"]), 34 + 4 * int(g["hl"]), int(g["ncopy"])
        assert tp[o:o + n].tobytes() == fr[int(g["frame"])][a:a + n]
    if flags & GRO:
        wrun = G.runs_model(want, wsip, W or R.GRO_DEFAULT_WINDOW)
        assert wrun.tobytes() == R.tcp_runs_host(want, wsip, W or R.GRO_DEFAULT_WINDOW).tobytes()
        assert run.tobytes() == wrun.tobytes() and len(run) < len(seg)
        assert np.array_equal(seg["offset"][run["first"]], run["offset"])
        assert len(tp) == int(_pad16(run["bytes"]).sum())
    else:
        assert len(run) == 0
        assert np.array_equal(seg["offset"], np.cumsum(_pad16(seg["ncopy"])) - _pad16(seg["ncopy"]))
        assert len(tp) == int(_pad16(seg["ncopy"]).sum())


@pytest.mark.parametrize("form", list(FORMS))
def test_tcp_form_is_the_models(form):
    flags = FORMS[form]
    for W in (0, W_SMALL) if flags & GRO else (0,):
        for b, res in enumerate(_alone(flags, W)):
            _check_tcp(b, flags, W, res["tcp"])
            assert _bytes(res["common"]) == _bytes(_alone(0)[b]["common"])


def test_the_tcp_forms_and_windows_all_differ():
    keys = [(f, 0) for f in FORMS.values() if f != (ASM | ORDER)] + [(GRO, W_SMALL), (ORDER | GRO, W_SMALL)]
    for b in range(len(_bursts())):
        seen = {_bytes(_alone(f, W)[b]["tcp"]) for f, W in keys}
        assert len(seen) == len(keys)


def test_detector_summaries_are_the_models_and_the_host_forms():
    m, state = DD.Model(), np.zeros(1, R.DDOS_STATE_DTYPE)
    for b, res in enumerate(_alone(R.DLV_DDOS)):
        summ = np.frombuffer(res["ddos"], R.DDOS_SUMMARY_DTYPE)[0]
        fr, _, (buf, off, lens) = _packed(b)
        want = m.run(*DD.frames_bits(fr), THRESH)
        assert DD.margin_ok(want, THRESH)
        host = R.ddos_host(buf, off, lens, 6, THRESH, state)[3]
        for ref in (want["summary"], host):
            DD.check_summary(summ, ref)
        if not np.isnan(want["summary"]["last_stat"]):
            assert abs(summ["last_stat"] - want["summary"]["last_stat"]) <= want["tol"][-1]
    assert summ["frames_seen"] == sum(len(f) for f in _bursts()) > DD.WINDOW
    assert not np.isnan(summ["last_stat"])


def test_cookie_results_are_the_host_forms_and_the_models():
    lm, p = CK.lmask_of((1, 2), 3), R.ck_params(CK.KEY, T)
    for b, res in enumerate(_alone(R.DLV_SYNCOOKIE)):
        _, _, (buf, off, lens) = _packed(b)
        st, tx, tot = res["ck"]
        for want in (R.syncookie_host(buf, off, lens, 6, _verdicts(b), lm, 3, p),
                     CK.run(buf, off, lens, 6, _verdicts(b), lm, 3, t=T)):
            assert list(tot) == list(want[2]) and tot[0] >= 15 and tot[1] >= 8 and tot[2] >= 2
            assert st.tobytes() == want[0].tobytes() and tx.tobytes() == want[1].tobytes()


@pytest.mark.parametrize("cap", [CAP_SMALL, CAP_BIG])
def test_l2_results_are_the_host_forms_and_the_models(cap):
    for b, res in enumerate(_alone(R.DLV_L2, 0, cap)):
        _, _, (buf, off, lens) = _packed(b)
        got = res["l2"]
        want = R.l2_host(buf, off, lens, 6, _verdicts(b), R.l2_params(M.LOCALS), cap)
        model = M.run(buf, off, lens, 6, _verdicts(b), M.LOCALS, cap)
        assert list(got[5]) == list(want[5]) == list(model[5]) and got[5][4] >= 1
        for g, w, x in zip(got[:5], want[:5], model[:5]):
            assert g.tobytes() == w.tobytes() == (x if isinstance(x, bytes) else x.tobytes())
    small, big = (_alone(R.DLV_L2, 0, c)[0]["l2"][5] for c in (CAP_SMALL, CAP_BIG))
    assert small[4] < big[4] <= small[0] + small[2]     # (the small room cuts answers the big one holds)


# ---- (3) one context through all of it ---------------------------------------------------
def test_one_context_through_every_combination():
    combos = [f | s for f in FORMS.values() for s in SIDES]
    random.Random(64).shuffle(combos)
    assert len(set(combos)) == 64
    W, cap = 0, CAP_SMALL
    with _open(0, W, cap) as c:
        for step, flags in enumerate(combos):
            if step == 20:
                cap = CAP_BIG
                c.l2_set(R.l2_params(M.LOCALS), cap)
            if step in (12, 44):
                W = W_SMALL if step == 12 else 0
                c.tune_gro(W)
            c.tune_deliver(flags)
            c.ddos_reset()
            _same(_deliver(c, True), _want(flags, W, cap), (step, hex(flags)))
    l2_steps = [s for s, f in enumerate(combos) if f & R.DLV_L2]
    gro_steps = [s for s, f in enumerate(combos) if f & GRO]
    assert min(l2_steps) < 20 < max(l2_steps)               # both capacities were used
    assert min(gro_steps) < 12 and max(gro_steps) >= 44 and any(12 <= s < 44 for s in gro_steps)


# ---- (4) the zero-frame burst ------------------------------------------------------------
@pytest.mark.parametrize("flags", [ASM | R.DLV_DDOS | R.DLV_SYNCOOKIE | R.DLV_L2,
                                   ORDER | GRO | R.DLV_DDOS | R.DLV_L2], ids=hex)
def test_zero_frame_burst_between_real_ones(flags):
    arrs = [a for a, _ in _mbufs()]
    want = _want(flags, 0, CAP_BIG)
    for in_flight, at in itertools.product((False, True), (1, 2)):
        with _open(flags) as c:
            got = _deliver(c, in_flight, arrs[:at] + [[]] + arrs[at:])
            empty = got.pop(at)
            _same(got, want, (hex(flags), in_flight, at))
            out, dg, first, up = empty["common"]
            assert len(out) == len(dg) == len(up) == 0 and first.tobytes() == bytes(8)
            assert _bytes(empty["tcp"]) == (b"", b"", b"", b"", 0) and empty["ddos"] == bytes(48)
            assert _bytes(empty["ck"]) == NO_CK and _bytes(empty["l2"]) == NO_L2
    assert _alone(0)[0]["common"][2][1] > 0         # (the set's first[] held counts before)
