"""The UDP compaction model (tests/compact_ref.py) pinned on the CPU against
the delivery oracle: the verdicts are the oracle's (oracle/ref_cpu.c), and
what the model hands every socket (datagram order, lengths, source addresses,
payload bytes) must be what udp_process + nrecvfrom of oracle/ref_stack.c
deliver frame by frame (udp.c:25-52, common.c:517-565).  The device tests
compare K3 with this model."""
import numpy as np

import compact_ref as CR
import frames as F
import oracle_bind as O
import rxgpu as R

L = "192.168.100.77"


def _burst(rng, nsock):
    """a few hundred frames to nsock sockets: payload sizes across the 16-B
    padding edges, zero-length datagrams (udp.c:38-44: not delivered),
    unbound ports, a TCP segment and an ARP frame between them, captures cut
    at 41, 42, 43, inside the addresses and inside the payload"""
    frames, caps = [], []
    sizes = [0, 1, 2, 15, 16, 17, 31, 32, 33, 100, 555, 1458]
    cuts = [41, 42, 43, 44, 57, 58, 59, 27, 29, 35, 36]
    for k in range(420):
        pl = bytes(rng.integers(1, 256, sizes[k % len(sizes)], dtype=np.uint8))
        port = 30000 + int(rng.integers(0, nsock + 2))  # the last two: no socket
        f = F.udp_frame(f"10.{k % 7}.{k % 200}.{k % 250 + 1}", 1000 + k, L, port, pl)
        if k % 41 == 7:
            f = F.tcp_frame("10.0.0.9", 40000, L, 30001, pl)
        if k % 53 == 11:
            f = F.arp_frame("1.2.3.4", L)
        cap = len(f)
        if k % 5 == 3:
            cap = cuts[(k // 5) % len(cuts)]
        elif k % 5 == 4 and len(f) > 60:
            cap = int(rng.integers(43, len(f)))
        frames.append(f)
        caps.append(min(cap, len(f)))
    return frames, caps


def test_model_matches_delivery_oracle():
    rng = np.random.default_rng(17)
    nsock = 9
    udp = np.zeros(nsock, R.UDP_SOCK_DTYPE)
    udp["localip"] = R.ip_raw(L)
    udp["localport"] = [R.port_raw(30000 + k) for k in range(nsock)]
    udp["protocol"] = 17
    frames, caps = _burst(rng, nsock)
    buf, off, lens = F.pack_frames(frames, 6, caplens=caps)
    v = O.Tables(udp, np.zeros(0, R.TCB_DTYPE)).classify(buf, off, lens, 6)
    got = CR.compact(frames, caps, v, nsock)
    st = O.Stack()
    fds = []
    for k in range(nsock):  # creation order = flow id (rxg_flows_sync)
        fd = st.socket(2)
        assert st.bind(fd, R.ip_raw(L), R.port_raw(30000 + k)) == 0
        fds.append(fd)
    rcs = [st.rx(f[:c]) for f, c in zip(frames, caps)]
    # the oracle's two halves agree on which frames are delivered
    deliv = CR.delivered(v, nsock)
    assert [i for i, r in enumerate(rcs) if r == 0 and v["cls"][i] == R.CLS_UDP] == list(deliv)
    assert got.totals[0] == len(deliv) > 200 and got.totals[2] == 0
    assert any(v["payload_len"][i] == 0 and v["rc"][i] != 0 for i in range(len(frames))
               if v["cls"][i] == R.CLS_UDP)  # the zero-length datagrams
    cut = [i for i in deliv if caps[i] < 42 + v["payload_len"][i]]
    assert {41, 42, 43} <= {caps[i] for i in cut} and any(caps[i] > 59 for i in cut)
    slices = CR.socket_slices(got, nsock)
    for k, fd in enumerate(fds):
        assert len(slices[k]) > 5
        for sip, sport, ln, data in slices[k]:
            r, d, osip, osport = st.recvfrom(fd, 65536)
            # nrecvfrom returns offload.length = dgram_len bytes: the payload and 8 zeros
            assert r == ln + 8 and d == data + bytes(8), (k, ln)
            assert (osip, osport) == (sip, sport)
        assert st.recvfrom(fd, 65536)[0] == O.WOULD_BLOCK
    # the buffer: 16-B aligned payloads back to back in rank order, zero padding
    pos = 0
    for d, nc in zip(got.dgram, got.ncopy):
        assert d["offset"] == pos and pos % 16 == 0
        pad = (int(nc) + 15) // 16 * 16
        assert not got.payload[pos + int(nc):pos + pad].any()
        pos += pad
    assert pos == got.totals[1] == len(got.payload) and got.written.all()


def test_model_payload_cap():
    """a payload whose padded end passes payload_cap is marked unwritten and
    sets totals[2]; records, ranks and the byte total do not change"""
    frames = [F.udp_frame("10.0.0.1", 7, L, 30000 + k % 2, b"\xff" * s)
              for k, s in enumerate([20, 1, 16, 40, 5])]
    v = np.zeros(5, R.VERDICT_DTYPE)
    v["cls"], v["flow_id"] = R.CLS_UDP, [0, 1, 0, 1, 0]
    v["payload_len"] = [20, 1, 16, 40, 5]
    caps = [len(f) for f in frames]
    full = CR.compact(frames, caps, v, 2)
    assert list(full.dgram["frame"]) == [0, 2, 4, 1, 3] and list(full.first) == [0, 3, 5]
    assert list(full.dgram["offset"]) == [0, 32, 48, 64, 80] and list(full.totals) == [5, 128, 0]
    assert CR.compact(frames, caps, v, 2, 128).written.all()
    cut = CR.compact(frames, caps, v, 2, 112)
    assert list(cut.totals) == [5, 128, 1] and cut.dgram.tobytes() == full.dgram.tobytes()
    assert cut.written[:80].all() and not cut.written[80:].any()
    one = CR.compact(frames, caps, v, 1)  # ids >= nflows are not delivered
    assert list(one.dgram["frame"]) == [0, 2, 4] and list(one.first) == [0, 3]
