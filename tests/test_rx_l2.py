"""The L2 responder on the CPU: the model of tests/l2_ref.py against the
hand-written cases (two known answers whose reply bytes were worked out by
hand), rxg_l2_host (csrc/rx_l2_host.cpp) against the model byte for byte
(status, answers, roff / rlen / rsrc, totals; a canary behind every output) on
the hand cases and on fuzzed bursts classified by the oracle, the capacity
cut, the parameter checks, and the socket layer's host-verdict path.
tests/san/l2_harness.c runs the host form under ASan + UBSan as a plain
executable.  The device side is tests/test_gpu_rx_l2.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import frames as F
import l2_ref as M
import oracle_bind as O
import rxgpu as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd")
CANARY = 0xA5
PAD = 8
BIG = 1 << 22


def both(frames, caps, v, unit, cap=BIG, local=M.LOCALS):
    """one burst through the model and rxg_l2_host; everything compared, the
    canaries checked; returns the model's result"""
    buf, off, lens = F.pack_frames(frames, unit, caps)
    want = M.run(buf, off, lens, unit, v, local, cap)
    got = R.l2_host(buf, off, lens, unit, v, R.l2_params(local), cap, pad=PAD, canary=CANARY)
    compare(got, want, len(frames))
    return want


def compare(got, want, n):
    """(status, frames, roff, rlen, rsrc, totals) with pad against the model's"""
    st, out, roff, rlen, rsrc, tot = got
    assert list(tot) == list(want[5])
    k, span = int(tot[4]), 64 * int(tot[5])
    assert st[:n].tobytes() == want[0].tobytes() and np.all(st[n:] == CANARY)
    assert out[:span].tobytes() == want[1] and np.all(out[span:] == CANARY)
    assert roff[:k].tobytes() == want[2].tobytes() and np.all(roff[k:] == 0xA5A5A5A5)
    assert rlen[:k].tobytes() == want[3].tobytes() and np.all(rlen[k:] == 0xA5A5)
    assert rsrc[:k].tobytes() == want[4].tobytes() and np.all(rsrc[k:] == 0xA5A5A5A5)


def hand_burst():
    c = M.hand_cases()
    return c, [x[1] for x in c], [x[2] or len(x[1]) for x in c], M.verdicts([x[3] for x in c])


def test_model_on_the_hand_cases():
    cases, frames, caps, v = hand_burst()
    buf, off, lens = F.pack_frames(frames, 4, caps)
    st, out, roff, rlen, rsrc, tot = M.run(buf, off, lens, 4, v, M.LOCALS, BIG)
    ans = {int(i): out[64 * int(o):64 * int(o) + int(n)] for o, n, i in zip(roff, rlen, rsrc)}
    for i, (name, frame, cap, cls, want, reply) in enumerate(cases):
        assert st[i] == want, name
        assert (i in ans) == (want in (M.ARP_REQ, M.ECHO)), name
        if reply is not None:
            assert ans[i] == reply, name
        if want == M.ECHO:                      # an answer a receiver accepts
            a = ans[i]
            tl = int.from_bytes(a[16:18], "big")
            assert len(a) == 14 + tl and M.csum(a[14:34]) == 0xFFFF and M.csum(a[34:]) == 0xFFFF, name
            assert a[38:] == frame[38:14 + tl], name
    by = {c[0]: ans.get(i) for i, c in enumerate(cases)}
    assert by["answer checksum 0xFFFF"][36:38] == b"\xff\xff"
    assert by["answer checksum 0x0000"][36:38] == b"\x00\x00"
    assert by["answer checksum 0x0000, odd tail"][36:38] == b"\x00\x00"
    assert by["arp for the second local address"][6:12] == M.LOCAL2_MAC
    assert by["echo to the second local address"][6:12] == M.LOCAL2_MAC
    assert len(by["trailing bytes after 14 + tl"]) == 98
    assert len(by["message length 30"]) == 64 and len(by["message length 8980"]) == 9014
    assert sorted(tot[:4]) == sorted([(st == k).sum() for k in (1, 2, 3, 4)]) and tot[4] == len(ans)


@pytest.mark.parametrize("unit", [4, 6])
def test_host_form_on_the_hand_cases(unit):
    cases, frames, caps, v = hand_burst()
    want = both(frames, caps, v, unit)
    assert [int(s) for s in want[0]] == [c[4] for c in cases]


TABLES = None


def classify(frames, caps, unit):
    """K1's verdicts by the oracle, against tables with a UDP socket and a
    listener on the local address"""
    global TABLES
    if TABLES is None:
        udp = np.zeros(1, R.UDP_SOCK_DTYPE)
        udp[0] = (R.ip_raw(M.LOCAL_IP), R.port_raw(53), 17, 0)
        tcb = np.zeros(1, R.TCB_DTYPE)
        tcb[0] = (0, R.ip_raw(M.LOCAL_IP), 0, R.port_raw(80), R.TCP_STATUS_LISTEN)
        TABLES = O.Tables(udp, tcb)
    buf, off, lens = F.pack_frames(frames, unit, caps)
    return TABLES.classify(buf, off, lens, unit)


@pytest.mark.parametrize("unit", [4, 6])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_host_form_equals_the_model_on_fuzzed_bursts(n, unit):
    frames, caps = M.fuzz_burst(100 + n, n)
    st = both(frames, caps, classify(frames, caps, unit), unit)[0]
    if n >= 257:                               # every status occurs
        assert set(st) == {0, 1, 2, 3, 4}
    frames, caps = M.fuzz_burst(200 + n, n, "arp")
    assert both(frames, caps, classify(frames, caps, unit), unit)[5][0] == n
    frames, caps = M.fuzz_burst(300 + n, n, "echo")
    assert both(frames, caps, classify(frames, caps, unit), unit)[5][2] == n
    frames, caps = M.fuzz_burst(400 + n, n, "none")
    assert not both(frames, caps, classify(frames, caps, unit), unit)[0].any()


def test_the_oracle_classifies_the_candidates_as_the_rule_expects():
    """K1 is untouched: ARP stays RXG_CLS_ARP, ICMP stays RXG_CLS_IPV4_OTHER, both KNI"""
    v = classify([M.KA_ARP_REQ, M.KA_ECHO_REQ], [60, 98], 6)
    assert list(v["cls"]) == [M.CLS_ARP, M.CLS_IPV4_OTHER] and list(v["rc"]) == [1, 1]


def test_cap_bytes_one_byte_short_of_the_kth_answer():
    frames, caps = M.fuzz_burst(7, 200)
    v = classify(frames, caps, 6)
    full = both(frames, caps, v, 6)
    ends = (full[2].astype(np.int64) + (full[3].astype(np.int64) + 63) // 64) * 64
    assert len(ends) > 40
    for k in (0, 1, 17, len(ends) - 1):
        cut = both(frames, caps, v, 6, cap=int(ends[k]) - 1)
        assert cut[5][4] == k and cut[0].tobytes() == full[0].tobytes()
        assert list(cut[5][:4]) == list(full[5][:4])
        assert both(frames, caps, v, 6, cap=int(ends[k]))[5][4] == k + 1
    # a small answer behind the one that did not fit is not written either
    fr = [M.echo(bytes(100)), M.echo(bytes(1000)), M.arp()]
    assert both(fr, [len(f) for f in fr], M.verdicts([2, 2, 0]), 6, cap=192 + 1023)[5][4] == 1


def test_nlocal_0_and_9_and_null_outputs():
    cases, frames, caps, v = hand_burst()
    assert not both(frames, caps, v, 6, local=[])[0].any()
    buf, off, lens = F.pack_frames(frames, 6, caps)
    p = R.l2_params(M.LOCALS)
    p["nlocal"] = 9
    with pytest.raises(R.RxgError) as e:
        R.l2_host(buf, off, lens, 6, v, p, BIG)
    assert e.value.rc == -22
    one = np.zeros(64, np.uint8)
    args = [buf.ctypes.data, off.ctypes.data, lens.ctypes.data, len(lens), 6, v.ctypes.data,
            R.l2_params(M.LOCALS).ctypes.data] + [one.ctypes.data] * 2 + [64] + [one.ctypes.data] * 4
    for k in (7, 8, 10, 11, 12, 13):            # status, out, roff, rlen, rsrc, totals
        a = list(args)
        a[k] = None
        assert R._l2_host(*a) == -22
    a = list(args)
    a[4] = 3
    assert R._l2_host(*a) == -22


def test_abi_surface():
    assert R.L2_PARAMS_DTYPE.itemsize == 100 and R.L2_MAX_LOCAL == 8 and R.DLV_L2 == 0x100
    assert (R.L2_ARP_REQ, R.L2_ARP_REPLY, R.L2_ECHO, R.L2_ECHO_BAD) == (1, 2, 3, 4)
    with R.Context(R.HOST_ONLY) as ctx:
        for flags in (R.DLV_L2, R.DLV_L2 | R.DLV_TCP_GRO | R.DLV_TCP_ORDER | R.DLV_DDOS | R.DLV_SYNCOOKIE,
                      R.DLV_L2 | R.DLV_TCP_ASSEMBLE, R.DLV_L2 | R.DLV_TCP_IN_PLACE, 0):
            ctx.tune_deliver(flags)
        for flags in (0x8, 0x40, 0x200, R.DLV_L2 | 0x8, R.DLV_L2 | 0x40):
            with pytest.raises(R.RxgError):
                ctx.tune_deliver(flags)
        ctx.l2_set(R.l2_params(M.LOCALS), 1 << 16)
        p = R.l2_params(M.LOCALS)
        p["nlocal"] = 9
        with pytest.raises(R.RxgError):
            ctx.l2_set(p, 1 << 16)
        with pytest.raises(R.RxgError) as e:
            ctx.l2_dev(0, 0, 0, 0, 6, 0, R.l2_params(M.LOCALS), 64, 64, 64, 64, 64, 64, 64)
        assert e.value.rc == -19                              # RXG_ENODEV: never the host form
    for name in ("rxg_l2_dev", "rxg_l2_host", "rxg_l2_set", "rxg_delivery_l2"):
        assert name in R.EXPORTED


# ---- the socket layer, host-verdict path ------------------------------------------------
@pytest.fixture()
def ns():
    s = R.NStack(R.HOST_ONLY)
    yield s
    s.fini()


@pytest.mark.parametrize("mode", ["cpu", "stale"])
@pytest.mark.parametrize("encode", [False, True])
def test_socket_layer_answers(ns, mode, encode):
    M.check_scenario(M.scenario(ns, mode, encode=encode))


def test_socket_layer_option_off(ns):
    """the same input: no answer, the counters stay 0, ARP learning as with it on"""
    M.check_scenario(M.scenario(ns, "cpu", on=False), on=False)


def test_socket_layer_needs_a_local_address_and_fini_resets(ns):
    with pytest.raises(R.RxgError) as e:
        ns.set_l2_respond(True)
    assert e.value.rc == -22
    ns.set_local(M.LOCAL_IP, M.LOCAL_MAC)
    ns.set_l2_respond(True)
    ns.deliver([M.KA_ECHO_REQ], M.verdicts([M.CLS_IPV4_OTHER]))
    assert ns.stat(22) == 1
    ns.fini()
    ns.__init__(R.HOST_ONLY)
    ns.set_local(M.LOCAL_IP, M.LOCAL_MAC)
    ns.deliver([M.KA_ECHO_REQ], M.verdicts([M.CLS_IPV4_OTHER]))
    assert [ns.stat(k) for k in (21, 22, 23, 24)] == [0, 0, 0, 0] and ns.tx_burst() == []


def test_socket_layer_queue_byte_bound(ns):
    """2 MiB of 64-B slots: 9014-byte answers fill it before 1024 frames do"""
    ns.set_local(M.LOCAL_IP, M.LOCAL_MAC)
    ns.set_l2_respond(True)
    req = M.echo(bytes(8972))
    slot = (len(req) + 63) // 64 * 64
    fit = (2 << 20) // slot
    for _ in range(2):
        ns.deliver([req] * 200, M.verdicts([M.CLS_IPV4_OTHER] * 200))
    assert ns.stat(22) == fit < 400 and ns.stat(23) == 400 - fit
    out = ns.tx_burst(max_frames=1024, cap_bytes=4 << 20)
    assert len(out) == fit and out[0] == M.answer_of(req, M.CLS_IPV4_OTHER) == out[-1]


# ---- under the sanitizers ------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("g++") is None,
                    reason="needs gcc/g++")
def test_l2_host_code_under_asan_ubsan(tmp_path):
    """tests/san/l2_harness.c with csrc/rx_l2_host.cpp, compiled with
    -fsanitize=address,undefined and run directly"""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    objs = []
    for src, cc, std in [("tests/san/l2_harness.c", "gcc", "-std=gnu11"),
                         ("dpdk-tcp-udp_protocol_stack_amd/csrc/rx_l2_host.cpp", "g++", "-std=c++17")]:
        o = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run([cc, std, *san, "-Iinclude", "-c", os.path.join(ROOT, src), "-o", o],
                       check=True, cwd=ROOT)
        objs.append(o)
    exe = str(tmp_path / "l2_harness")
    subprocess.run(["g++", *san, *objs, "-o", exe], check=True, cwd=ROOT)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "L2 SAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
