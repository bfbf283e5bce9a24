"""Oracle against the reference's own compiled code, live on the CPU.

oracle/_ref/refrun links the reference's prebuilt objects (tcp.o, udp.o,
common.o) with our stubs and driver; tests/ref_bind.py runs it as a child
process.  Every comparison here is exact.  An error that oracle/ref_cpu.c or
ref_stack.c shares with a kernel is invisible to the kernel-versus-oracle
tests; it fails here.

Where the reference is absent (and so is refrun) these tests skip; where the
reference is present and refrun is not, test_refrun_is_built fails.

EXCLUDED lists inputs on which the reference's code faults, by name, with the
reason; it may hold at most 1 % of any corpus.  It is empty: the reference
returned on every input below.
"""
import os
import sys
import zlib

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import ref_bind as RB
import ref_check as RC
import rxgpu as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import make_golden as G  # noqa: E402
import make_ref_golden as MG  # noqa: E402

EXCLUDED = {}  # case name -> reason (none needed)

needs_refrun = pytest.mark.skipif(
    not RB.have_refrun() and not RB.have_reference(),
    reason="neither the reference's build/ objects nor oracle/_ref/refrun exist on this machine")


def test_refrun_is_built():
    """where the reference's objects are present, `make -C oracle` must have
    produced the runner: nothing below may skip silently"""
    if not RB.have_reference():
        pytest.skip("the reference is not on this machine")
    assert RB.have_refrun(), "build/tcp.o exists but oracle/_ref/refrun does not: run make -C oracle"


def test_exclusions_within_cap():
    assert len(EXCLUDED) == 0


LIBS = [("O2", lambda: O.lib), ("O0", O.lib_O0)]


# ---- checksums ---------------------------------------------------------------
_SCRATCH = np.zeros(65536 + 256, np.uint8)


def _oracle_cksums(lib, cases):
    """the three functions on the same zero-extended buffer and start as refrun"""
    out = np.zeros((len(cases), 3), np.uint16)
    base = _SCRATCH.ctypes.data
    for i, (b, a) in enumerate(cases):
        n = len(b)
        _SCRATCH[a:a + n] = np.frombuffer(b, np.uint8)
        p = base + a
        out[i] = (lib.oracle_raw_cksum(p, n), lib.oracle_ipv4_udptcp_cksum(p, p + 20),
                  lib.oracle_ipv4_cksum(p))
        _SCRATCH[a:a + n] = 0
    return out


@pytest.fixture(scope="module")
def cksum_run():
    cases = MG.cksum_cases(reps=2, extra_random=2000)
    s = RB.Session()
    for b, a in cases:
        s.cksum(b, a)
    return cases, np.array(s.run(timeout=300), np.uint16)


@needs_refrun
@pytest.mark.parametrize("which", ["O2", "O0"])
def test_checksums_match_reference(cksum_run, which):
    """rte_raw_cksum, rte_ipv4_udptcp_cksum and rte_ipv4_cksum as compiled into
    the reference, on >= 20,000 seeded buffers: every length 0-130, each
    multiple of 16 from 128 to 2,064 +-1, 8,986, 9,000 and 65,515; odd and even
    starts; random, all-zero and all-ones bytes; L4 bytes built so that the
    value before the UDP rule is 0x0000 (UDP then gives 0xFFFF), 0x0001 and
    0xFFFE for protocol 6 and 17 (0xFFFF itself is unreachable before the
    rule: a pseudo-header with a protocol never sums to 0); tl 0, 19, 20, 21,
    65,535; IHL nibbles 5-15"""
    cases, ref = cksum_run
    assert len(cases) >= 20000
    lens = {len(b) for b, _ in cases}
    assert {20 + n for n in MG.CK_LENGTHS} <= lens and set(MG.CK_LENGTHS) <= lens
    assert (ref[:, 1] == 0xFFFF).sum() > 500 and (ref[:, 1] == 0).sum() > 500
    got = _oracle_cksums(dict(LIBS)[which](), cases)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert len(bad) == 0, [(int(i), len(cases[i][0]), cases[i][1], got[i].tolist(), ref[i].tolist())
                           for i in bad[:5]]


# ---- lookups -------------------------------------------------------------------
def _random_tables(rng, n):
    ips = [0, R.ip_raw("192.168.100.77"), R.ip_raw("10.9.9.9"), R.ip_raw("10.0.0.9")]
    ports = [0] + [R.port_raw(p) for p in (53, 80, 8080, 8889, 9999, 40000)]
    pick = lambda pool: int(pool[rng.integers(len(pool))])  # noqa: E731
    nu = int(rng.integers(0, n + 1))
    nt = n - nu
    udp = np.zeros(nu, R.UDP_SOCK_DTYPE)
    for i in range(nu):
        udp[i] = (pick(ips), pick(ports), 17 if rng.random() < 0.85 else int(rng.choice([6, 1, 0])), 0)
    tcb = np.zeros(nt, R.TCB_DTYPE)
    for i in range(nt):
        r = rng.random()
        if r < 0.3:    # a listener as nbind/nlisten make it
            tcb[i] = (0, pick(ips), 0, pick(ports), 1)
        elif r < 0.4:  # a listener with a remote key (only a hand-built block has one)
            tcb[i] = (pick(ips), pick(ips), pick(ports), pick(ports), 1)
        elif r < 0.5:  # bound, not listening: CLOSED
            tcb[i] = (0, pick(ips), 0, pick(ports), 0)
        else:
            tcb[i] = (pick(ips), pick(ips), pick(ports), pick(ports), int(rng.choice([0, 2, 4, 9])))
    return udp, tcb, ips, ports


@needs_refrun
def test_lookups_match_reference():
    """get_hostinfo_fromip_port / tcp_stream_search on random tables of 1-300
    blocks drawn from small pools, so that duplicate keys, several listeners, a
    listener and an exact tcb on one port, CLOSED tcbs, sockets whose protocol
    is not 17, address 0 and port 0 all occur; sockets and listeners come from
    the real nsocket/nbind/nlisten, other tcbs from the reference's LISTEN
    handler (a SYN) where a listener exists, else hand-built nodes"""
    rng = np.random.default_rng(23)
    sizes = [1, 2, 3, 300, 299] + [int(x) for x in rng.integers(1, 301, 25)]
    total = made_by_syn = 0
    for k, n in enumerate(sizes):
        udp, tcb, ips, ports = _random_tables(rng, n)
        pick = lambda pool: int(pool[rng.integers(len(pool))])  # noqa: E731
        q_udp = [(pick(ips), pick(ports), int(rng.choice([17, 17, 17, 6]))) for _ in range(150)]
        q_udp += [(int(u["localip"]), int(u["localport"]), 17) for u in udp[:50]]
        q_tcp = [(pick(ips), pick(ips), pick(ports), pick(ports)) for _ in range(200)]
        q_tcp += [tuple(int(x) for x in (t["sip"], t["dip"], t["sport"], t["dport"])) for t in tcb[:50]]
        s = RB.Session()
        s.tables(udp, tcb, prefer_real=k % 3 != 2)
        for q in q_udp:
            s.lookup_udp(*q)
        for q in q_tcp:
            s.lookup_tcp(*q)
        ref = s.run()
        made_by_syn += s.how_used.count(RB.HOW_SYN)
        for name, lib in LIBS:
            t = O.Tables(udp, tcb, lib())
            got = [t.lookup_udp(*q) for q in q_udp] + [t.lookup_tcp(*q) for q in q_tcp]
            assert got == ref, (name, k, n, [(i, g, r) for i, (g, r) in enumerate(zip(got, ref))
                                             if g != r][:5])
        total += len(ref)
        hits = [r for r in ref if r != R.FLOW_NONE]
        if n >= 100:
            assert len(hits) > 20 and len(set(hits)) > 5
    assert made_by_syn > 100 and total > 10000


# ---- verdicts -------------------------------------------------------------------
def _run_rx(udp, tcb, fr, recv=False):
    s = RB.Session()
    s.tables(udp, tcb)
    for f, c in fr:
        s.rx(f[:c], recv=recv, delta=MG.RECV_DELTA)
    return s.run(timeout=300)


def _classify(lib, udp, tcb, fr, unit_log2):
    """frames packed whole with caplens, so bytes past a cut capture are the
    frame's own and the next frame's: the oracle must read them as zeros"""
    buf, off, lens = F.pack_frames([f for f, _ in fr], unit_log2, caplens=[c for _, c in fr])
    return O.Tables(udp, tcb, lib).classify(buf, off, lens, unit_log2)


def _spoiler_corpus():
    """the flow table and the waves of test_lane_fast_path_waves (both address
    sets), one spoiler per wave of 64"""
    socks = [(MG.L, 30000 + 3 * k) for k in range(300)] + [(MG.L2, 30000 + 21 * k) for k in range(20)]
    udp = np.zeros(len(socks), R.UDP_SOCK_DTYPE)
    for i, (ip, port) in enumerate(socks):
        udp[i] = (R.ip_raw(ip), R.port_raw(port), 17, 0)
    return udp, np.zeros(0, R.TCB_DTYPE), MG.spoiler_frames(np.random.default_rng(16), waves_of=64)


@pytest.fixture(scope="module")
def rx_runs():
    """(name, udp, tcb, frames, reference results) per corpus, computed once"""
    eu, et = G.edge_flows()
    ef, ec = G.edge_frames()
    cu, ct = MG.rx_flows()
    rng = np.random.default_rng(99)
    cuts = []  # capture lengths cut at random, on valid frames of every size class
    for _ in range(400):
        f = MG.sized(int(rng.choice([64, 65, 100, 128, 300, 590, 1500, 1514])),
                     int(rng.choice([6, 17])), rng)
        cuts.append((f, int(rng.integers(0, len(f) + 1))))
    su, st, sf = _spoiler_corpus()
    corpora = [("edge", eu, et, list(zip(ef, ec))),
               ("fuzz", eu, et, MG.fuzz_frames(6000)),
               ("deliberate", cu, ct, MG.deliberate_frames()),
               ("ladder", cu, ct, MG.ladder_frames(np.random.default_rng(5))),
               ("cuts", cu, ct, cuts),
               ("spoilers", su, st, sf)]
    return [(n, u, t, fr, _run_rx(u, t, fr)) for n, u, t, fr in corpora]


@needs_refrun
@pytest.mark.parametrize("which", ["O2", "O0"])
@pytest.mark.parametrize("unit_log2", [4, 6])
def test_verdicts_match_reference(rx_runs, which, unit_log2):
    """oracle_classify against udp_process / tcp_process on every field the
    reference decides (ref_check.verdict_mismatches): the edge frames of
    make_golden.py, the mutation fuzz of test_fuzzed_frames_match_oracle, the
    spoilers of test_lane_fast_path_waves, random capture cuts and the
    deliberate cases (computed 0x0000 against stored 0xFFFF, UDP computing to
    0, dgram_len 0-9 and past the frame, tl < 20 and past the capture)"""
    lib = dict(LIBS)[which]()
    seen_rc = set()
    total = 0
    for name, udp, tcb, fr, ref in rx_runs:
        exp = RC.records(ref)
        v = _classify(lib, udp, tcb, fr, unit_log2)
        bad = RC.verdict_mismatches(v, exp)
        assert not bad, (name, len(bad), bad[:5])
        bad8 = RC.verdict_mismatches(R.verdict8_of(v), exp, v8=True)
        assert not bad8, (name, "verdict8", bad8[:5])
        seen_rc |= {(int(e["family"]), int(e["rc"])) for e in exp}
        total += len(fr)
    assert seen_rc >= {(17, 0), (17, -2), (17, -3), (6, 0), (6, -1), (6, -2), (0, 1)}
    assert total > 7000


@needs_refrun
def test_deliberate_cases_are_what_they_claim(rx_runs):
    """the reference's own answers on the named cases"""
    ref = {n: r for n, _, _, _, r in rx_runs}["deliberate"]
    fr = MG.deliberate_frames()
    # computed 0x0000: stored 0xFFFF rejected, stored 0x0000 accepted (no +-0 equivalence)
    assert (ref[0].l4_cksum, ref[0].rc) == (0x0000, -1) and fr[0][0][50:52] == b"\xff\xff"
    assert (ref[1].l4_cksum, ref[1].rc) == (0x0000, 0)
    # UDP computing to 0 reads 0xFFFF; UDP is delivered whatever it stores
    assert (ref[4].l4_cksum, ref[4].rc) == (0xFFFF, 0) and (ref[5].l4_cksum, ref[5].rc) == (0xFFFF, 0)
    # dgram_len 0..9 to a bound port: -2 up to and including 8 (the rte_malloc
    # size-0 rule of the stub, as DPDK 19.11), delivered from 9
    for dl in range(10):
        r = ref[7 + 2 * dl]
        assert r.rc == (-2 if dl <= 8 else 0), dl
        assert ref[8 + 2 * dl].rc == -3


# ---- delivery ---------------------------------------------------------------------
@needs_refrun
def test_udp_delivery_matches_reference():
    """ref_stack.c's UDP path against udp_process's ring slot and the real
    nrecvfrom (common.o, the current tree) with a caller buffer shorter than,
    equal to and longer than offload.length: return values, bytes, source
    address, and the second read that takes the re-queued rest.  The 8 bytes
    nrecvfrom reads past the payload are zeros on both sides: the stub
    rte_malloc pads with zeros, the oracle defines them as zeros."""
    cu, _ = MG.rx_flows()
    udp = cu[cu["protocol"] == 17]
    tcb = np.zeros(0, R.TCB_DTYPE)
    rng = np.random.default_rng(41)
    fr = [(f, c) for f, c in MG.deliberate_frames() + MG.ladder_frames(rng) + MG.fuzz_frames(1500)
          if c > 23 and f[12:14] == b"\x08\x00" and f[23] == 17]
    ref = _run_rx(udp, tcb, fr, recv=True)
    st = O.Stack()
    fds = []
    for u in udp:
        fd = st.socket(2)
        assert st.bind(fd, int(u["localip"]), int(u["localport"])) == 0
        fds.append(fd)
    delivered = 0
    for (f, c), r in zip(fr, ref):
        assert r.family == 17
        for k in range(3):
            assert st.rx(f[:c]) == r.rc, (f[:60].hex(), c)
            if r.rc != 0:
                break
            v = r.recv[k]
            assert v.buflen == max(r.length - MG.RECV_DELTA, 0) + k * MG.RECV_DELTA
            fd = fds[r.match]
            ret, data, sip, sport = st.recvfrom(fd, v.buflen)
            assert (ret, sip, sport) == (v.ret, v.sip, v.sport), (k, v)
            assert data == v.data
            assert (r.sip, r.sport, r.dport, r.protocol) == (sip, sport, int(udp[r.match]["localport"]), 17)
            assert r.dip == int(udp[r.match]["localip"]) and r.copied_equal == 1
            if v.ret2 != RC.NO_SECOND_READ:
                ret2, data2, _, _ = st.recvfrom(fd, 65535 + 64)
                assert (ret2, data2) == (v.ret2, v.data2), (k, v)
            assert st.recvfrom(fd, 16)[0] == O.WOULD_BLOCK
            assert v.data + v.data2 == (f[:c] + bytes(70000))[42:42 + r.length - 8] + bytes(8)
        delivered += r.rc == 0
    assert delivered > 300


# ---- TX ---------------------------------------------------------------------------
def _tx_fields(frames):
    s = RB.Session()
    for f in frames:
        s.tx(f)
    return s.run(timeout=300)


def _assert_tx_fields(frames, filled, what):
    """filled[i]: frame i after this project's fill; the two fields equal the
    reference's wherever they are wholly captured"""
    for i, (f, g, (ipck, l4ck, has_ip, has_l4)) in enumerate(zip(frames, filled, _tx_fields(frames))):
        assert len(f) == len(g)
        is_ip = (bytes(f) + bytes(14))[12:14] == b"\x08\x00"
        assert bool(has_ip) == is_ip, (what, i)
        want = bytearray(f)
        if has_ip and len(f) >= 26:
            want[24:26] = ipck.to_bytes(2, "little")
        if has_l4:
            hole = 40 if (bytes(f) + bytes(24))[23] == 17 else 50
            if len(f) >= hole + 2:
                want[hole:hole + 2] = l4ck.to_bytes(2, "little")
        assert bytes(g) == bytes(want), (what, i, len(f))


@needs_refrun
def test_tx_cksum_matches_reference():
    """oracle_tx_cksum on the fuzz burst of tests/test_tx.py (fields zeroed)
    against rte_ipv4_cksum + rte_ipv4_udptcp_cksum in the encoders' call order"""
    from test_tx import _fuzz_burst, _zero_fields
    buf, off, lens = _fuzz_burst()
    z = _zero_fields(buf, off, lens, 4)
    out = O.tx_cksum(z, off, lens, 4)
    cut = lambda b: [b[int(o) << 4:(int(o) << 4) + int(n)].tobytes() for o, n in zip(off, lens)]  # noqa: E731
    _assert_tx_fields(cut(z), cut(out), "fuzz")
    # past each capture the burst is untouched
    mask = np.ones(len(buf), bool)
    for o, n in zip(off, lens):
        mask[int(o) << 4:(int(o) << 4) + int(n)] = False
    assert np.array_equal(out[mask], z[mask])


@needs_refrun
def test_tx_encoders_match_reference():
    """rxg_tx_encode_host and rxg_tx_encode_tso_host frames of every descriptor
    kind (K5's host forms, which the GPU suite holds bit-exact to K5): zero the
    two checksum fields, let the reference fill them, get the frame back"""
    import test_tx_tso as TS
    import txenc_ref as T
    ds = T.boundary_descs() + T.mix_descs(400)
    t, pay = T.burst(ds)
    cap = sum((T.frame_len(d) + 63) // 64 * 64 for d in t) + 256
    pk, off, ln, span, tot, rc = R.tx_encode_host(t, pay, cap, 0, 0, fill=T.CANARY)
    assert rc == 0 and {int(k) for k in t["kind"]} >= {R.TXD_UDP, R.TXD_TCP, R.TXD_ARP}
    frames = [pk[int(o) * 64:int(o) * 64 + int(n)].tobytes() for o, n in zip(off, ln) if n]
    assert len(frames) == len(ds)
    _assert_tx_fields([MG.zero_tx_fields(f, len(f)) for f in frames], frames, "encode")

    t, pay = TS.burst(1460, True)
    ent, byt = TS.sizes(t, 1460)
    pk, off, ln, first, nseg, span, tot, rc = R.tx_encode_tso_host(
        t, pay, 1460, byt + 256, ent + 3, 0, 0, fill=T.CANARY, fill_entries=TS.ONES32)
    ents = [e for k in range(len(t)) for e in range(int(first[k]), int(first[k]) + int(nseg[k]))]
    frames = [pk[int(off[e]) * 64:int(off[e]) * 64 + int(ln[e])].tobytes() for e in ents]
    assert len(ents) == int(tot[0]) > len(t) and all(len(f) for f in frames)
    _assert_tx_fields([MG.zero_tx_fields(f, len(f)) for f in frames], frames, "tso")


# ---- the survey's literals, and the recorded fixtures -------------------------------
@needs_refrun
def test_survey_kats_from_the_reference():
    """every hand-transcribed `survey` value of kats.json, returned by the
    reference's compiled code itself"""
    import json
    k = json.load(open(os.path.join(GOLD, "kats.json")))
    s = RB.Session()
    for c in k["survey"]:
        s.cksum(bytes.fromhex(c["hex"]))
        if c["fn"] == "udptcp_same":
            s.cksum(bytes.fromhex(c["hex2"]))
    res = iter(s.run())
    for c in k["survey"]:
        got = next(res)[1]
        if c["fn"] == "udptcp_same":
            assert got == next(res)[1], c["src"]
        else:
            assert got == c["expect"], (c["src"], hex(got))
    fl = k["survey_frames_flows"]
    udp = np.array([(R.ip_raw(ip), R.port_raw(p), 17, 0) for ip, p in fl["udp"]], R.UDP_SOCK_DTYPE)
    tcb = np.array([(R.ip_raw(a), R.ip_raw(b), R.port_raw(c), R.port_raw(d), e)
                    for a, b, c, d, e in fl["tcp"]], R.TCB_DTYPE)
    frames = [bytes.fromhex(c["hex"]) for c in k["survey_frames"]]
    for c, r in zip(k["survey_frames"], _run_rx(udp, tcb, [(f, len(f)) for f in frames], recv=True)):
        e = c["expect"]
        assert r.rc == e["rc"] and r.family == {3: 17, 4: 6}[e["cls"]], c["src"]
        if "dgram_len" in e:
            assert r.length == e["dgram_len"] and r.recv[1].ret == e["dgram_len"]
        if "payload_len" in e:
            assert r.length - 8 == e["payload_len"] and r.copied_equal == 1


@needs_refrun
def test_fixtures_regenerate_byte_identical(tmp_path):
    """make_ref_golden.py is deterministic and the committed files are what
    the reference's code writes today"""
    for name in MG.main(str(tmp_path)):
        a = open(os.path.join(GOLD, name), "rb").read()
        b = open(os.path.join(str(tmp_path), name), "rb").read()
        assert zlib.crc32(a) == zlib.crc32(b) and a == b, name
