"""Oracle pinning: the CPU restatement against every known-answer vector we
have (SURVEY.md §8(a) values recorded from the reference's compiled code,
RFC 1071, Microsoft RSS table) and the committed edge-case fixture."""
import json
import os

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxgpu as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = json.load(open(os.path.join(GOLD, "kats.json")))


@pytest.mark.parametrize("which", ["O2", "O0"])
@pytest.mark.parametrize("case", KATS["survey"] + KATS["rfc1071"], ids=lambda c: c["src"])
def test_cksum_kats(case, which):
    lib = O.lib if which == "O2" else O.lib_O0()
    b = bytes.fromhex(case["hex"])
    buf = np.frombuffer(b + bytes(8), np.uint8)
    if case["fn"] == "raw":
        got = lib.oracle_raw_cksum(buf.ctypes.data, len(b))
        assert got == case["expect"]
    elif case["fn"] == "udptcp":
        got = lib.oracle_ipv4_udptcp_cksum(buf.ctypes.data, buf.ctypes.data + 20)
        assert got == case["expect"], f"{case['src']}: {got:#06x} != {case['expect']:#06x}"
    else:  # IHL ignored: identical results for IHL 5 and 6
        b2 = np.frombuffer(bytes.fromhex(case["hex2"]) + bytes(8), np.uint8)
        assert lib.oracle_ipv4_udptcp_cksum(buf.ctypes.data, buf.ctypes.data + 20) == \
            lib.oracle_ipv4_udptcp_cksum(b2.ctypes.data, b2.ctypes.data + 20)


@pytest.mark.parametrize("case", KATS["ms_rss"], ids=lambda c: c["sip"])
def test_rss_kats(case):
    s, d = R.ip_raw(case["sip"]), R.ip_raw(case["dst"])
    sp, dp = R.port_raw(case["sport"]), R.port_raw(case["dport"])
    # zero ports contribute no input bits: the 12-byte hash equals the 8-byte IPv4 hash
    assert O.rss_hash(s, d, 0, 0) == case["ipv4"]
    assert O.rss_hash(s, d, sp, dp) == case["ipv4_tcp"]
    # the library's own (independently written) Toeplitz agrees
    assert R.rss_hash(s, d, 0, 0) == case["ipv4"]
    assert R.rss_hash(s, d, sp, dp) == case["ipv4_tcp"]


def _survey_flows():
    fl = KATS["survey_frames_flows"]
    udp = np.zeros(len(fl["udp"]), R.UDP_SOCK_DTYPE)
    for i, (ip, port) in enumerate(fl["udp"]):
        udp[i] = (R.ip_raw(ip), R.port_raw(port), 17, 0)
    tcb = np.zeros(len(fl["tcp"]), R.TCB_DTYPE)
    for i, (sip, dip, sport, dport, st) in enumerate(fl["tcp"]):
        tcb[i] = (R.ip_raw(sip), R.ip_raw(dip), R.port_raw(sport), R.port_raw(dport), st)
    return udp, tcb


def test_survey_frame_kats_oracle():
    udp, tcb = _survey_flows()
    frames = [bytes.fromhex(c["hex"]) for c in KATS["survey_frames"]]
    buf, off, lens = F.pack_frames(frames)
    v = O.Tables(udp, tcb).classify(buf, off, lens, 6)
    for c, vi in zip(KATS["survey_frames"], v):
        for k, want in c["expect"].items():
            if k == "dgram_len":
                assert vi["payload_len"] + 8 == want
            else:
                assert vi[k] == want, (c["src"], k, vi)


def test_edge_fixture_oracle_regression():
    flows = np.load(os.path.join(GOLD, "edge_flows.npz"))
    frames = F.read_pcap(os.path.join(GOLD, "edge.pcap"))
    buf, off, lens = F.pack_frames(frames)
    want = np.load(os.path.join(GOLD, "edge_verdicts.npy"))
    for which in (O.lib, O.lib_O0()):
        got = O.Tables(flows["udp"], flows["tcb"], which).classify(buf, off, lens, 6)
        assert got.tobytes() == want.tobytes()


def test_oracle_list_semantics():
    """first match in head-inserted order == newest creation index; listener
    pass ignores dst ip; exact pass ignores status (common.c:31-55, 97-108)"""
    L = R.ip_raw("192.168.100.77")
    udp = np.zeros(3, R.UDP_SOCK_DTYPE)
    udp[:] = [(L, R.port_raw(5), 17, 0), (L, R.port_raw(5), 17, 0), (L, R.port_raw(6), 17, 0)]
    tcb = np.zeros(3, R.TCB_DTYPE)
    tcb[:] = [(0, L, 0, R.port_raw(80), 1), (0, 0, 0, R.port_raw(80), 1),
              (7, L, 9, R.port_raw(80), 0)]
    t = O.Tables(udp, tcb)
    assert t.lookup_udp(L, R.port_raw(5)) == 1
    assert t.lookup_udp(L, R.port_raw(5), proto=6) == R.FLOW_NONE
    assert t.lookup_tcp(7, L, 9, R.port_raw(80)) == 2          # CLOSED still exact-matches
    assert t.lookup_tcp(8, 12345, 9, R.port_raw(80)) == 1      # newest listener, any dst ip
    assert t.lookup_tcp(8, L, 9, R.port_raw(81)) == R.FLOW_NONE


def test_pcap_roundtrip(tmp_path):
    fr = [F.udp_frame("1.2.3.4", 1, "5.6.7.8", 2, b"x" * n) for n in (0, 1, 17, 1000)]
    p = tmp_path / "t.pcap"
    F.write_pcap(str(p), fr, caplens=[len(f) - (i == 3) * 10 for i, f in enumerate(fr)])
    back = F.read_pcap(str(p))
    assert back[:3] == fr[:3] and back[3] == fr[3][:-10]


# ---- fixtures recorded from the reference's own compiled code -----------------
# (tests/golden/make_ref_golden.py through oracle/_ref/refrun; see
# golden/ref_golden_readme.txt).  These run everywhere, refrun or not.
import ref_check as RC  # noqa: E402

_LIBS = {"O2": lambda: O.lib, "O0": O.lib_O0}


@pytest.fixture(scope="module")
def ref_rx():
    fl = np.load(os.path.join(GOLD, "ref_rx_flows.npz"))
    frames = F.read_pcap(os.path.join(GOLD, "ref_rx.pcap"))
    exp = np.load(os.path.join(GOLD, "ref_rx_expect.npy"))
    assert exp.dtype == RC.REF_RX_DTYPE and len(exp) == len(frames)
    return fl["udp"], fl["tcb"], frames, exp


def test_ref_fixture_shape(ref_rx):
    """the corpus holds the capture lengths at which a lane-group split, a pass
    boundary or a tail mask can go wrong, and every file stays small"""
    _, _, frames, exp = ref_rx
    lens = [len(f) for f in frames]
    assert 1500 <= len(frames) <= 2500
    need = set(range(34, 131)) | {63, 64, 65, 127, 128, 129, 1535, 1536, 1537, 2047, 2048, 2049,
                                  590, 1500, 1514}
    assert need <= set(lens) and lens.count(9014) >= 12
    assert {(int(e["family"]), int(e["rc"])) for e in exp} >= \
        {(17, 0), (17, -2), (17, -3), (6, 0), (6, -1), (6, -2), (0, 1)}
    for name in ("ref_rx.pcap", "ref_rx_flows.npz", "ref_rx_expect.npy", "ref_cksum.npz",
                 "ref_tx.npz"):
        assert os.path.getsize(os.path.join(GOLD, name)) < 512 * 1024, name


@pytest.mark.parametrize("which", ["O2", "O0"])
@pytest.mark.parametrize("unit_log2", [4, 6])
def test_ref_rx_fixture_oracle(ref_rx, which, unit_log2):
    udp, tcb, frames, exp = ref_rx
    buf, off, lens = F.pack_frames(frames, unit_log2)
    v = O.Tables(udp, tcb, _LIBS[which]()).classify(buf, off, lens, unit_log2)
    bad = RC.verdict_mismatches(v, exp)
    assert not bad, (len(bad), bad[:5])
    bad = RC.verdict_mismatches(R.verdict8_of(v), exp, v8=True)
    assert not bad, ("verdict8", len(bad), bad[:5])


def test_ref_rx_fixture_delivery(ref_rx):
    """ref_stack.c's udp_process + nrecvfrom against the recorded ring slot and
    the three recorded reads (buffer shorter, equal, longer) of every
    delivered datagram"""
    import zlib
    udp, tcb, frames, exp = ref_rx
    st = O.Stack()
    fds = {}
    for i, u in enumerate(udp):
        if u["protocol"] != 17:  # no API makes such a socket; it never matches a datagram
            continue
        fd = st.socket(2)
        assert st.bind(fd, int(u["localip"]), int(u["localport"])) == 0
        fds[i] = fd
    n = 0
    for f, e in zip(frames, exp):
        if e["family"] != 17 or len(f) < 24:
            continue
        for k in range(3):
            assert st.rx(f) == e["rc"]
            if e["rc"] != 0:
                break
            fd = fds[int(e["match"])]
            ret, data, sip, sport = st.recvfrom(fd, int(e["recv_buflen"][k]))
            assert (ret, sip, sport) == (e["recv_ret"][k], e["sip"], e["sport"])
            if e["recv_ret2"][k] != RC.NO_SECOND_READ:
                ret2, data2, _, _ = st.recvfrom(fd, 65535 + 64)
                assert ret2 == e["recv_ret2"][k]
                data += data2
            assert zlib.crc32(data) == e["recv_crc"][k]
            assert len(data) == e["length"] and st.recvfrom(fd, 8)[0] == O.WOULD_BLOCK
            n += 1
    assert n > 900


@pytest.mark.parametrize("which", ["O2", "O0"])
def test_ref_cksum_fixture_oracle(which):
    z = np.load(os.path.join(GOLD, "ref_cksum.npz"))
    lib = _LIBS[which]()
    scratch = np.zeros(65536 + 256, np.uint8)
    data, start = z["data"], z["start"]
    assert len(z["raw"]) == len(start) - 1 > 3000
    for i in range(len(start) - 1):
        b, a = data[start[i]:start[i + 1]], int(z["align"][i])
        scratch[a:a + len(b)] = b
        p = scratch.ctypes.data + a
        got = (lib.oracle_raw_cksum(p, len(b)), lib.oracle_ipv4_udptcp_cksum(p, p + 20),
               lib.oracle_ipv4_cksum(p))
        assert got == (z["raw"][i], z["udptcp"][i], z["ipv4"][i]), (i, len(b), a)
        scratch[a:a + len(b)] = 0


@pytest.mark.parametrize("which", ["O2", "O0"])
def test_ref_tx_fixture_oracle(which):
    """oracle_tx_cksum fills what the reference fills, and touches nothing else;
    the host encoder writes the recorded frame whose header sums to 0xFFFF"""
    z = np.load(os.path.join(GOLD, "ref_tx.npz"))
    buf, off, lens = z["pkts"], z["off"], z["len"]
    want = buf.copy()
    for i in range(len(off)):
        s, n = int(off[i]) << 4, int(lens[i])
        if z["has_ip"][i] and n >= 26:
            want[s + 24:s + 26] = np.frombuffer(int(z["ipck"][i]).to_bytes(2, "little"), np.uint8)
        hole = 40 if buf[s + 23] == 17 else 50
        if z["has_l4"][i] and n >= hole + 2:
            want[s + hole:s + hole + 2] = np.frombuffer(int(z["l4ck"][i]).to_bytes(2, "little"), np.uint8)
    got = buf.copy()
    _LIBS[which]().oracle_tx_cksum(got.ctypes.data, off.ctypes.data, lens.ctypes.data, len(off), 4)
    assert np.array_equal(got, want)
    assert z["ipck"][-1] == 0 and F.fold_cksum(buf[(int(off[-1]) << 4) + 14:(int(off[-1]) << 4) + 34].tobytes()) == 0xFFFF
    import sys
    sys.path.insert(0, GOLD)
    import make_ref_golden as MG
    import txenc_ref as T
    sip, dip, sport, dport, frame = MG.ffff_header_udp()
    t, pay = T.burst([T.txd(R.TXD_UDP, 3, sip=sip, dip=dip, sport=sport, dport=dport,
                            dst_mac=F.PEER_MAC, src_mac=F.LOCAL_MAC)], payloads=[b"abc"])
    pk = R.tx_encode_host(t, pay, 256)[0]
    s = int(off[-1]) << 4
    assert pk[:len(frame)].tobytes() == want[s:s + len(frame)].tobytes()
