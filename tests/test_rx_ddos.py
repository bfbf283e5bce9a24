"""The entropy flood detector on the CPU: rxg_ddos_host (csrc/rx_ddos_host.cpp,
the literal restatement of the reference's ddos_detect) and the socket layer's
host-verdict path against the numpy model of tests/ddos_ref.py.

What is compared how: set, tot, S, T, the counts, first_alarm, frames_seen,
every flag bit and the state's bytes exactly; D within tol(g) = 512 * 2^-52 *
(sum_window tot*log2 tot + T*log2 T) of the model's float64 value (a
worst-case bound for 256 sequential f64 adds plus a few ulps per term; the
model in float64 and in longdouble differ by about 1e-10 on 64-B frames, far
inside it), NaN at exactly the same frames.  Each test first asserts from the
model alone that no checked frame lies within 2 tol of the threshold, so no
frame is left out of a flag comparison.

The known answers of tests/golden/ddos_kats.json pin e(s, t) to the
reference's own recorded run.  tests/san/ddos_harness.c runs the length
cases, an undefined frame and a split session under ASan/UBSan."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ddos_ref as M
import frames as F
import oracle_bind as O
import rxgpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd")
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1500, 9000, 65535]
LENGTHS_ORDER = LENGTHS[1:] + [0]      # (the empty frame last: every window after it is undefined)
SPLITS = [(1, 255, 256, 257, 531), (300, 300, 300, 400), (1300,)]


@functools.lru_cache(maxsize=None)
def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "ddos_kats.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def _main():
    """the main burst packed (0xFF between frames) and the model's answer"""
    frames = M.main_burst()
    buf, off, lens = M.pack(frames, 6)
    st, tt = M.frame_bits(buf, off, lens, 6)
    m = M.Model()
    res = m.run(st, tt, 1200.0)
    return buf, off, lens, st, tt, res, m.state()


def _compare(got, res, st, thresh):
    """rxg_ddos_host's (bits, flag, stat, summary) against a model result"""
    bits, flag, stat, summ = got
    assert M.margin_ok(res, thresh)
    assert np.array_equal(bits, st)
    assert np.array_equal(flag, res["flags"]), np.nonzero(flag != res["flags"])[0][:10]
    nan = np.isnan(res["D"])
    assert np.array_equal(np.isnan(stat), nan)
    err = np.abs(stat[~nan] - res["D"][~nan])
    if err.size:
        print("max |D - model| = %.3g, smallest tol = %.3g" % (err.max(), res["tol"][~nan].min()))
    assert np.all(err <= res["tol"][~nan])
    M.check_summary(summ, res["summary"])
    if not np.isnan(res["summary"]["last_stat"]):
        assert abs(summ["last_stat"] - res["summary"]["last_stat"]) <= res["tol"][-1]


# ---- known answers -------------------------------------------------------------
def test_recorded_pairs_of_the_reference():
    for k in _kats()["recorded"]:
        assert "%.6f" % R.ddos_entropy(k["set"], k["tot"]) == k["printed"]
        assert "%.6f" % float(M.entropy(k["set"], k["tot"])) == k["printed"]


def test_exact_and_nan_cases():
    for k in _kats()["exact"]:
        assert R.ddos_entropy(k["set"], k["tot"]) == k["e"] == float(M.entropy(k["set"], k["tot"]))
    for k in _kats()["nan"]:
        assert np.isnan(R.ddos_entropy(k["set"], k["tot"])) and np.isnan(M.entropy(k["set"], k["tot"]))
    # a window that holds such a pair is undefined, decided from the integers
    st = np.zeros(1, R.DDOS_STATE_DTYPE)
    st["frames_seen"] = 256
    st["set"][0][:] = 256
    st["tot"][0][:] = 512
    st["set"][0][5], st["tot"][0][5] = _kats()["nan"][0]["set"], _kats()["nan"][0]["tot"]
    buf, off, lens = M.pack([bytes([0x0F]) * 64], 6)
    _, flag, stat, summ, _ = R.ddos_host(buf, off, lens, 6, 1200.0, st)
    assert flag[0] == R.DDOS_UNDEF and np.isnan(stat[0]) and summ["undef_frames"] == 1


def test_identical_frames_stream():
    k = _kats()["stream"]
    assert k["ones"] == 4 * k["len"]
    frames = [bytes([0x0F]) * k["len"]] * 600
    buf, off, lens = M.pack(frames, 6)
    bits, flag, stat, summ, _ = R.ddos_host(buf, off, lens, 6)
    assert np.all(bits == k["ones"])
    assert np.all(flag[:256] == R.DDOS_WARMUP) and np.all(np.isnan(stat[:256]))
    assert np.all(stat[256:] == k["D"])
    assert flag[256] == R.DDOS_ALARM | R.DDOS_RISE and np.all(flag[257:] == R.DDOS_ALARM)
    assert summ["alarm_frames"] == 344 and summ["first_alarm"] == 256 and summ["rises"] == 1
    st, tt = M.frame_bits(buf, off, lens, 6)
    assert np.all(M.Model().run(st, tt)["D"][256:] == k["D"])


# ---- the main burst ------------------------------------------------------------
def test_main_burst_events_of_the_model():
    res = _main()[5]
    assert M.events(res["flags"]) == [(256, "rise"), (304, "fall"), (951, "rise"), (1000, "fall"),
                                      (1256, "rise")]
    und = np.nonzero(res["flags"] & M.UNDEF)[0]
    assert und[0] == 1000 and und[-1] == 1255 and len(und) == 256
    assert M.margin_ok(res, 1200.0)
    # float64 against longdouble: the reference's own error, far inside tol
    st, tt = _main()[3:5]
    hi = M.Model().run(st, tt, 1200.0, np.longdouble)
    ok = ~np.isnan(res["D"])
    d = np.abs(res["D"][ok] - hi["D"][ok].astype(np.float64)).max()
    print("model f64 vs longdouble: %.3g" % d)
    assert d < 1e-3 * res["tol"][ok].min()


def test_main_burst():
    buf, off, lens, st, tt, res, want_state = _main()
    bits, flag, stat, summ, state = R.ddos_host(buf, off, lens, 6)
    _compare((bits, flag, stat, summ), res, st, 1200.0)
    assert state.tobytes() == want_state.tobytes()


@pytest.mark.parametrize("split", SPLITS)
def test_main_burst_in_splits(split):
    buf, off, lens, st, tt, res, want_state = _main()
    assert sum(split) == len(lens)
    state = np.zeros(1, R.DDOS_STATE_DTYPE)
    m = M.Model()
    a = 0
    flags, stats = [], []
    for n in split:
        sl = slice(a, a + n)
        want = m.run(st[sl], tt[sl], 1200.0)
        bits, flag, stat, summ, _ = R.ddos_host(buf, off[sl], lens[sl], 6, 1200.0, state)
        _compare((bits, flag, stat, summ), want, st[sl], 1200.0)
        assert state.tobytes() == m.state().tobytes()
        flags.append(flag)
        stats.append(stat)
        a += n
    # whatever the split: the flags and the final state of the whole burst
    assert np.array_equal(np.concatenate(flags), res["flags"])
    assert state.tobytes() == want_state.tobytes()
    d = np.concatenate(stats)
    ok = ~np.isnan(res["D"])
    assert np.all(np.abs(d[ok] - res["D"][ok]) <= res["tol"][ok])


def test_empty_burst_and_arguments():
    buf, off, lens = _main()[:3]
    state = np.zeros(1, R.DDOS_STATE_DTYPE)
    R.ddos_host(buf, off[:300], lens[:300], 6, 1200.0, state)
    before = state.tobytes()
    _, _, _, summ, _ = R.ddos_host(buf, off[:0], lens[:0], 6, 1200.0, state)
    assert state.tobytes() == before
    assert summ["frames_seen"] == 300 and summ["first_alarm"] == 0xFFFFFFFF and summ["alarm_frames"] == 0
    assert summ["flag"] == state["flag"][0] and np.isnan(summ["last_stat"])
    # nullable outputs
    s2 = np.zeros(1, R.DDOS_STATE_DTYPE)
    b, f, d, summ2, _ = R.ddos_host(buf, off[:300], lens[:300], 6, 1200.0, s2, want=())
    assert b is None and f is None and d is None and s2.tobytes() == before
    summ3 = np.zeros(1, R.DDOS_SUMMARY_DTYPE)
    args = [buf.ctypes.data, off.ctypes.data, lens.ctypes.data, 10, 6, 1200.0, s2.ctypes.data, None,
            None, None, summ3.ctypes.data]
    assert R._ddos_host(*args) == 0
    for k, bad in ((0, None), (1, None), (2, None), (6, None), (10, None), (4, 3), (5, float("nan"))):
        a = list(args)
        a[k] = bad
        assert R._ddos_host(*a) == -22, k                            # RXG_EINVAL


def test_fewer_than_a_window():
    buf, off, lens, st, tt, _, _ = _main()
    state = np.zeros(1, R.DDOS_STATE_DTYPE)
    state["flag"] = 1                                                  # untouched by warm-up frames
    m = M.Model()
    m.flag = 1
    for sl in (slice(0, 100), slice(100, 255)):
        want = m.run(st[sl], tt[sl])
        bits, flag, stat, summ, _ = R.ddos_host(buf, off[sl], lens[sl], 6, 1200.0, state)
        assert np.all(flag == R.DDOS_WARMUP) and np.all(np.isnan(stat))
        assert summ["flag"] == 1 and summ["rises"] == 0 and summ["falls"] == 0
        _compare((bits, flag, stat, summ), want, st[sl], 1200.0)
        assert state.tobytes() == m.state().tobytes() and state["flag"][0] == 1


def length_case(unit_log2, seed=11):
    """300 random 64-B frames, then one frame of each length of LENGTHS (random
    bytes, so a counted pad byte or a dropped tail byte shows), each followed
    by 20 more 64-B frames; 0xFF between the frames"""
    del unit_log2
    rng = np.random.default_rng(seed)
    frames = [M.density_frame(rng, 64, 0.5) for _ in range(300)]
    for n in LENGTHS_ORDER:
        frames.append(M.density_frame(rng, n, 0.4))
        frames += [M.density_frame(rng, 64, 0.5) for _ in range(20)]
    return frames


@pytest.mark.parametrize("unit_log2", [4, 6])
def test_lengths(unit_log2):
    frames = length_case(unit_log2)
    buf, off, lens = M.pack(frames, unit_log2)
    st, tt = M.frame_bits(buf, off, lens, unit_log2)
    assert [len(frames[300 + 21 * k]) for k in range(len(LENGTHS))] == LENGTHS_ORDER
    assert [int(st[300 + 21 * k]) for k in range(len(LENGTHS))] == \
        [sum(bin(b).count("1") for b in frames[300 + 21 * k]) for k in range(len(LENGTHS))]
    m = M.Model()
    res = m.run(st, tt)
    assert (res["flags"] & M.UNDEF).any()                            # (the empty frame)
    bits, flag, stat, summ, state = R.ddos_host(buf, off, lens, unit_log2)
    _compare((bits, flag, stat, summ), res, st, 1200.0)
    assert state.tobytes() == m.state().tobytes()


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_all_zero_and_all_ones_frame(fill):
    rng = np.random.default_rng(5)
    frames = [M.density_frame(rng, 64, 0.5) for _ in range(600)]
    frames[400] = bytes([fill]) * 64
    buf, off, lens = M.pack(frames, 6)
    st, tt = M.frame_bits(buf, off, lens, 6)
    res = M.Model().run(st, tt)
    und = np.nonzero(res["flags"] & M.UNDEF)[0]
    assert und[0] == 400 and len(und) == 200
    assert res["flags"][400] & M.FALL
    bits, flag, stat, summ, _ = R.ddos_host(buf, off, lens, 6)
    _compare((bits, flag, stat, summ), res, st, 1200.0)


def median_threshold(st, tt):
    """a threshold in the middle of the model's D: between the two middle
    values, so half the checked frames alarm and none sits on it"""
    d = np.sort(M.Model().run(st, tt)["D"])
    d = d[~np.isnan(d)]
    return float((d[len(d) // 2 - 1] + d[len(d) // 2]) / 2)


def test_threshold_at_the_median():
    buf, off, lens, st, tt, _, _ = _main()
    thresh = median_threshold(st, tt)
    res = M.Model().run(st, tt, thresh)
    assert res["summary"]["rises"] >= 2 and res["summary"]["falls"] >= 2 and M.margin_ok(res, thresh)
    bits, flag, stat, summ, _ = R.ddos_host(buf, off, lens, 6, thresh)
    _compare((bits, flag, stat, summ), res, st, thresh)


# ---- the socket layer ----------------------------------------------------------
def socket_session(ns, mode, on, thresh=1200.0):
    """M.socket_bursts through a stack (mode: 'cpu' nstack_deliver with the
    oracle's verdicts, 'gpu' nstack_rx_burst, 'pipe' nstack_rx_submit /
    nstack_rx_complete with two bursts in flight): what the application sees
    (return codes, delivered counts, every byte read) and, per burst, the
    detector's status and counters"""
    if on:
        ns.set_rx_ddos(True, thresh)
    fd = ns.socket(R.SOCK_DGRAM)
    assert ns.bind(fd, M.SOCK_L, M.SOCK_PORT) == 0
    seen, status = [], []

    def drain():
        while True:
            r, data, a = ns.recvfrom(fd, 4096)
            if r < 0:
                break
            seen.append((r, data, a.sin_port, a.sin_addr))

    def done(delivered, rcs):
        seen.append(("burst", delivered, list(rcs)))
        drain()
        status.append((ns.ddos_status(), ns.stat(17), ns.stat(18)))

    bursts = M.socket_bursts()
    if mode == "pipe":
        for k, fr in enumerate(bursts):
            ns.rx_submit(fr)
            if k:
                done(*ns.rx_complete()[:2])
        done(*ns.rx_complete()[:2])
        return seen, status
    for fr in bursts:
        if mode == "cpu":
            u, t, gen = ns.flows(with_gen=True)
            buf, off, lens = F.pack_frames(fr)
            v = ns.to_ids(O.Tables(u, t).classify(buf, off, lens, 6))
            rcs = np.zeros(len(fr), np.int32)
            done(ns.deliver(fr, v, rcs, gen), rcs)
        else:
            done(*ns.rx_burst(fr)[:2])
    return seen, status


def check_socket_status(status, thresh=1200.0):
    """the per-burst status of socket_session against the model"""
    m = M.Model()
    tot = dict(rises=0, falls=0, alarm_frames=0, undef_frames=0)
    assert len(status) == len(M.socket_bursts())
    for fr, (stt, s17, s18) in zip(M.socket_bursts(), status):
        res = m.run(*M.frames_bits(fr), thresh)
        assert M.margin_ok(res, thresh)
        for k in tot:
            tot[k] += res["summary"][k]
            assert stt[k] == tot[k], (k, stt[k], tot[k])
        assert stt["frames_seen"] == m.frames_seen and stt["alarm"] == res["summary"]["flag"]
        want = res["summary"]["last_stat"]
        assert np.isnan(stt["last_stat"]) == np.isnan(want)
        if not np.isnan(want):
            assert abs(stt["last_stat"] - want) <= res["tol"][-1]
        assert s17 == tot["alarm_frames"] and s18 == tot["rises"]
    assert tot["rises"] == 2 and tot["falls"] == 1                   # both alarm states occur


def test_socket_layer_host_path():
    runs = {}
    for on in (False, True):
        ns = R.NStack(R.HOST_ONLY)
        try:
            runs[on] = socket_session(ns, "cpu", on)
        finally:
            ns.fini()
    assert runs[True][0] == runs[False][0]                           # detection only
    assert any(x[0] == "burst" and x[1] > 0 for x in runs[True][0])
    check_socket_status(runs[True][1])
    off_status = runs[False][1][-1]
    assert off_status[0]["frames_seen"] == 0 and off_status[1] == 0 and off_status[2] == 0


def test_socket_layer_option_resets_with_the_stack():
    ns = R.NStack(R.HOST_ONLY)
    try:
        socket_session(ns, "cpu", True)
        assert ns.ddos_status()["frames_seen"] == 1050 and ns.stat(18) == 2
        with pytest.raises(R.RxgError):
            ns.set_rx_ddos(True, float("nan"))
    finally:
        ns.fini()
    ns = R.NStack(R.HOST_ONLY)
    try:
        assert ns.ddos_status()["frames_seen"] == 0 and ns.stat(17) == 0 and ns.stat(18) == 0
    finally:
        ns.fini()


def test_context_calls_without_a_device():
    with R.Context(R.HOST_ONLY) as ctx:
        for g in (0,) + R.DDOS_LANES:
            ctx.tune_ddos(g)
        for g in (2, 4, 16, 32, 128):
            with pytest.raises(R.RxgError):
                ctx.tune_ddos(g)
        ctx.tune_ddos(0, 500.0)
        with pytest.raises(R.RxgError):
            ctx.tune_ddos(0, float("nan"))
        for fl in (R.DLV_DDOS, R.DLV_DDOS | R.DLV_TCP_GRO | R.DLV_TCP_ORDER,
                   R.DLV_DDOS | R.DLV_TCP_IN_PLACE, 0):
            ctx.tune_deliver(fl)
        ctx.ddos_reset()
        with pytest.raises(R.RxgError) as e:
            ctx.ddos_dev(0, 0, 0, 0, 6, 64, 1200.0, 16, None, None, None, 16)
        assert e.value.rc == -19                                      # RXG_ENODEV
    for name in ("rxg_ddos_dev", "rxg_ddos_host", "rxg_tune_ddos", "rxg_tune_ddos_thresh",
                 "rxg_ddos_reset", "rxg_delivery_ddos"):
        assert name in R.EXPORTED


# ---- under the sanitizers --------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None,
                    reason="needs gcc/g++")
def test_ddos_host_code_under_asan_ubsan(tmp_path):
    """tests/san/ddos_harness.c with csrc/rx_ddos_host.cpp, compiled with
    -fsanitize=address,undefined and run directly"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    objs = []
    for src, cc, std in [("tests/san/ddos_harness.c", "gcc", "-std=gnu11"),
                         ("dpdk-tcp-udp_protocol_stack_amd/csrc/rx_ddos_host.cpp", "g++", "-std=c++17")]:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, *san, "-Iinclude", "-c", os.path.join(ROOT, src), "-o", o],
                       check=True, cwd=ROOT)
        objs.append(o)
    exe = str(tmp_path / "ddos_harness")
    subprocess.run(["g++", *san, *objs, "-o", exe, "-lm"], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "DDOS SAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
