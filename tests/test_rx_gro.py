"""TCP receive coalescing (GRO) without a device.

The rule: rxg_tcp_runs_host (csrc/rx_gro_host.cpp) against the numpy model of
tests/gro_ref.py, on records decoded from frames made with tests/frames.py,
with the runs of the named edge cases also written out by hand.

The socket layer: nstack with nstack_set_rx_gro on, driven through
nstack_deliver side by side with oracle/ref_stack.c on scripted sessions whose
data comes in trains of in-sequence PSH|ACK segments: the same bytes and EOFs
per connection, the same return codes and tcb states, fewer fragments and ACKs
— exactly the ones the rule says.

tests/san/gro_harness.c runs the rule cases and one such session under
AddressSanitizer + UndefinedBehaviorSanitizer as a plain executable."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gro_ref as G
import rxgpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd")
WINDOWS = [1, 100, 250, 300, 1460, 4096, 65536, 1 << 20]


def _case_records():
    rng = np.random.default_rng(11)
    cases = G.rule_cases(rng)
    labels = [c[0] for c in cases]
    flows = [0 if k == "L" else 1 + k for k in labels]      # the listener's id is 0
    seg, sip = G.records([c[1] for c in cases], [c[2] for c in cases], flows)
    return seg, sip


def _split(run, seg, flow):
    """the run lengths of one connection"""
    return [int(r["nseg"]) for r in run if seg[r["first"]]["flow"] == flow]


def _check_partition(run, seg):
    assert run["first"][0] == 0 and np.all(run["nseg"] > 0)
    assert np.all(run["first"][1:] == run["first"][:-1] + run["nseg"][:-1])
    assert run["first"][-1] + run["nseg"][-1] == len(seg)
    end = 0
    for r in run:
        assert r["offset"] == (end + 15) // 16 * 16
        assert r["bytes"] == seg["ncopy"][r["first"]:r["first"] + r["nseg"]].sum()
        end = int(r["offset"]) + int(r["bytes"])


@pytest.mark.parametrize("W", WINDOWS)
def test_rule_cases_match_model(W):
    seg, sip = _case_records()
    got = R.tcp_runs_host(seg, sip, W)
    want = G.runs_model(seg, sip, W)
    assert got.tobytes() == want.tobytes(), (got, want)
    _check_partition(got, seg)
    assert np.all(got["bytes"] < W + 65536)


def test_rule_cases_by_hand():
    """the named cases at the default window, then the windows of flow 9 (6 x
    100 B) and flow 10 (9 x 1460 B); flow = 1 + the case's connection"""
    seg, sip = _case_records()
    run = R.tcp_runs_host(seg, sip, 65536)
    assert _split(run, seg, 1) == [3]              # seq wraps 2^32 inside the chain
    assert seg["seq"][seg["flow"] == 1][1] == 2 ** 32 - 50 and seg["seq"][seg["flow"] == 1][2] == 50
    assert _split(run, seg, 2) == [1, 2]           # a differing ack
    assert _split(run, seg, 3) == [1, 2]           # a duplicate seq
    assert _split(run, seg, 4) == [1, 1, 1]        # out of order
    assert _split(run, seg, 5) == [1, 1, 2]        # hl = 6
    assert _split(run, seg, 6) == [1, 1, 2, 1, 1, 1, 1]   # flags 0x10, 0x19, 0x11
    assert _split(run, seg, 7) == [1, 1, 2]        # plen = 0
    assert _split(run, seg, 8) == [1, 1, 2]        # a capture cut mid-payload
    assert _split(run, seg, 0) == [1, 1]           # two sources on the listener's id
    assert _split(run, seg, 9) == [6] and _split(run, seg, 10) == [9]
    for W, want in [(1, [1] * 6), (100, [1] * 6), (250, [3, 2, 1]), (300, [3, 3]), (600, [6])]:
        assert _split(R.tcp_runs_host(seg, sip, W), seg, 9) == want, W
    # W equal to one payload: every record its own run; W = 2 payloads: pairs
    assert _split(R.tcp_runs_host(seg, sip, 1460), seg, 10) == [1] * 9
    assert _split(R.tcp_runs_host(seg, sip, 2920), seg, 10) == [2, 2, 2, 2, 1]
    # W = 1: every record its own run, whatever links
    assert len(R.tcp_runs_host(seg, sip, 1)) == len(seg)
    # the caller's offsets are left alone
    seg2 = seg.copy()
    seg2["offset"] = 0xABCD
    R.tcp_runs_host(seg2, sip, 300)
    assert np.all(seg2["offset"] == 0xABCD)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rule_random_bursts_match_model(seed):
    """trains of random lengths over a few connections, some records made
    unmergeable at random, several windows; one burst is a single chain"""
    rng = np.random.default_rng(seed)
    frames, flows = [], []
    for k in range(12 if seed < 3 else 1):
        seq = int(rng.integers(0, 2 ** 32))
        cip, cport = G.conn(k)
        for _ in range(int(rng.integers(1, 80)) if seed < 3 else 700):
            n = int(rng.choice([1, 3, 15, 16, 17, 100, 1460]))
            kw = {}
            if seed < 3 and rng.random() < 0.1:
                kw = [dict(flags=0x10), dict(data_off=0x60), dict(ack=7), dict(flags=0x19)][int(rng.integers(4))]
            if seed < 3 and rng.random() < 0.05:
                seq += int(rng.integers(1, 50))
            frames.append(G.F.tcp_frame(cip, cport, G.L, 9999, G._p(rng, n), seq=seq & 0xFFFFFFFF, **kw))
            flows.append(k)
            seq += n
    seg, sip = G.records(frames, [len(f) for f in frames], flows)
    for W in (1, 17, 1460, 4096, 65536, 1 << 20):
        got = R.tcp_runs_host(seg, sip, W)
        assert got.tobytes() == G.runs_model(seg, sip, W).tobytes(), W
        _check_partition(got, seg)
    if seed == 3:
        assert len(R.tcp_runs_host(seg, sip, 1 << 20)) < 5


def test_rule_arguments():
    seg, sip = _case_records()
    assert len(R.tcp_runs_host(seg[:0], sip[:0], 65536)) == 0          # nseg = 0
    for W in (0, (1 << 20) + 1):
        with pytest.raises(R.RxgError):
            R.tcp_runs_host(seg, sip, W)


# ---- the socket layer ------------------------------------------------------------
@pytest.fixture()
def ns_host():
    s = R.NStack(R.HOST_ONLY)
    yield s
    s.fini()


@pytest.mark.parametrize("W", [65536, 2000])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_socket_layer_coalesces(ns_host, seed, W):
    ns_host.set_rx_gro(W)
    keys, events = G.scenario(seed)
    n_ns, n_os, absorbed = G.GroPair(ns_host, "cpu", W).run(keys, events)
    assert absorbed > 0 and n_ns + absorbed == n_os


@pytest.mark.parametrize("seed", [1, 2])
def test_socket_layer_off_is_unchanged(ns_host, seed):
    """switched on and off again: every fragment and every ACK as the oracle's"""
    ns_host.set_rx_gro(65536)
    ns_host.set_rx_gro(0)
    keys, events = G.scenario(seed)
    n_ns, n_os, absorbed = G.GroPair(ns_host, "cpu", 0).run(keys, events)
    assert absorbed == 0 and n_ns == n_os and ns_host.stat(15) == 0


def test_gro_excludes_inplace(ns_host):
    ns_host.set_rx_gro(65536)
    with pytest.raises(R.RxgError):
        ns_host.set_rx_inplace(True)
    ns_host.set_rx_gro(0)
    ns_host.set_rx_inplace(True)
    with pytest.raises(R.RxgError):
        ns_host.set_rx_gro(65536)
    ns_host.set_rx_gro(0)                 # (off is always accepted)
    ns_host.set_rx_inplace(False)
    ns_host.set_rx_gro(4096)
    with pytest.raises(R.RxgError):
        ns_host.set_rx_gro((1 << 20) + 1)


def test_delivery_options_exclude_each_other():
    with R.Context(R.HOST_ONLY) as ctx:
        ctx.tune_deliver(R.DLV_TCP_GRO)
        ctx.tune_deliver(R.DLV_TCP_IN_PLACE)
        with pytest.raises(R.RxgError):
            ctx.tune_deliver(R.DLV_TCP_GRO | R.DLV_TCP_IN_PLACE)
        ctx.tune_gro(0)
        ctx.tune_gro(1 << 20)
        with pytest.raises(R.RxgError):
            ctx.tune_gro((1 << 20) + 1)


# ---- under the sanitizers ----------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None,
                    reason="needs gcc/g++")
def test_gro_host_code_under_asan_ubsan(tmp_path):
    if not os.path.exists(os.path.join(PKG, "librxgpu.so")):
        pytest.fail("librxgpu.so not built (run __graft_entry__.build())")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    objs = []
    for src, cc, std in [("oracle/ref_cpu.c", "gcc", "-std=gnu11"),
                         ("oracle/ref_stack.c", "gcc", "-std=gnu11"),
                         ("dpdk-tcp-udp_protocol_stack_amd/host/nstack.c", "gcc", "-std=gnu11"),
                         ("tests/san/gro_harness.c", "gcc", "-std=gnu11"),
                         ("dpdk-tcp-udp_protocol_stack_amd/csrc/rx_gro_host.cpp", "g++", "-std=c++17")]:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, *san, "-Iinclude", "-c", os.path.join(ROOT, src), "-o", o],
                       check=True, cwd=ROOT)
        objs.append(o)
    exe = str(tmp_path / "gro_harness")
    # the control-plane calls (rxg_open with RXG_HOST_ONLY, flow sync) come from
    # the product library; rxg_tcp_runs_host above interposes on its copy
    subprocess.run(["g++", *san, *objs, "-o", exe, f"-L{PKG}", "-lrxgpu", f"-Wl,-rpath,{PKG}",
                    "-lpthread"], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               LSAN_OPTIONS="suppressions=" + os.path.join(ROOT, "tests", "san", "lsan.supp"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "GRO SAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
