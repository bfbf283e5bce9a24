"""GRO sweep: what TCP receive coalescing costs on the device and gains on the
host, both against the path without it in the same process.  Tuning only.
    python tools/gro_sweep.py [window [segments per connection]]

The burst is the socket bench's cfg3 shape: 16384 segments of 1500-B TCP
(PSH|ACK, 1446 payload bytes) over 4096 established connections, four
in-sequence segments per connection, the connections interleaved frame by
frame as a NIC delivers them.  A second argument changes the train length
(16384 / it connections), to see where longer trains take the host.

Device: rxg_tcp_coalesce_dev and rxg_tcp_compact_dev on the classified burst,
interleaved over rounds, every call timed with HIP events on its own; medians.
The same compact call timed twice per round (k, k'): the spread of identical
runs is the yardstick for the difference.

Host: nstack_rx_burst plus the application's reads (nstack_drain_all) with
nstack_set_rx_gro off, on and off again, interleaved over rounds: Mpps over
the pair of calls, fragments queued per burst (nstack_stat(4)), segments
absorbed (nstack_stat(15)) and the burst's TCP phases."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

W = int(sys.argv[1]) if len(sys.argv) > 1 else R.GRO_DEFAULT_WINDOW
PER = int(sys.argv[2]) if len(sys.argv) > 2 else 4
N, FLEN, SLOT = 16384, 1500, 1536
NCONN = N // PER
L = "192.168.100.77"
ROUNDS, WARM, REPS = 7, 2, 5
dev = torch.device("cuda:0")


def burst():
    """the packed burst (64-B units) with both checksums filled by K2"""
    rng = np.random.default_rng(3)
    f = np.zeros((N, SLOT), np.uint8)
    i = np.arange(N)
    c, q = i % NCONN, i // NCONN
    f[:, 0:6] = np.frombuffer(bytes.fromhex("000c296a014d"), np.uint8)
    f[:, 6:12] = np.frombuffer(bytes.fromhex("02aabbccddee"), np.uint8)
    f[:, 12:14] = (0x08, 0x00)
    f[:, 14:24] = np.frombuffer(bytes([0x45, 0, (FLEN - 14) >> 8, (FLEN - 14) & 255, 0, 1, 0x40, 0, 64, 6]),
                                np.uint8)
    sip = (10 | (1 << 8) | ((c >> 8) << 16) | ((c & 255) << 24)).astype("<u4")   # 10.1.x.y, raw
    f[:, 26:30] = sip.view(np.uint8).reshape(N, 4)
    f[:, 30:34] = np.frombuffer(bytes(int(x) for x in L.split(".")), np.uint8)
    f[:, 34:36] = (40000 >> 8, 40000 & 255)
    f[:, 36:38] = (9999 >> 8, 9999 & 255)
    seq = (c * 2654435761 + q * (FLEN - 54)) & 0xFFFFFFFF
    f[:, 38:42] = seq.astype(">u4").view(np.uint8).reshape(N, 4)
    f[:, 42:46] = (0, 0, 0x07, 0xD0)
    f[:, 46], f[:, 47] = 0x50, 0x18
    f[:, 48:50] = (0x39, 0x08)
    f[:, 54:FLEN] = rng.integers(0, 256, (N, FLEN - 54), dtype=np.uint8)
    off = (i * (SLOT // 64)).astype(np.uint32)
    lens = np.full(N, FLEN, np.uint16)
    tcb = np.zeros(NCONN + 1, R.TCB_DTYPE)
    tcb["sip"][:NCONN] = sip[:NCONN]
    tcb["dip"], tcb["sport"], tcb["dport"] = R.ip_raw(L), R.port_raw(40000), R.port_raw(9999)
    tcb["status"][:NCONN] = R.TCP_STATUS_ESTABLISHED
    tcb[NCONN] = (0, R.ip_raw(L), 0, R.port_raw(9999), R.TCP_STATUS_LISTEN)
    with R.Context(0, max_pkts=N, max_bytes=N * SLOT) as ctx:
        buf = ctx.tx_cksum(f.reshape(-1), off, lens, 6)
    return buf, off, lens, tcb


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def device_side(buf, off, lens, tcb):
    with R.Context(0, max_pkts=N, max_bytes=N * SLOT) as ctx:
        ctx.flows_sync(None, tcb)
        sh = torch.cuda.current_stream(dev).cuda_stream
        d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
        d_v = torch.empty(N * 16, dtype=torch.uint8, device=dev)
        ctx.classify_dev(d_pk, d_off, d_ln, N, 6, FLEN, d_v, None, stream=sh)
        cap = N * SLOT
        d_seg = torch.empty(N * 32, dtype=torch.uint8, device=dev)
        d_run = torch.empty(N * 16, dtype=torch.uint8, device=dev)
        d_pl = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_tot = torch.zeros(4, dtype=torch.int32, device=dev)

        def compact():
            ctx.tcp_compact_dev(d_pk, d_off, d_ln, N, 6, d_v, d_seg, d_pl, cap, d_tot, stream=sh)

        def coalesce():
            ctx.tcp_coalesce_dev(d_pk, d_off, d_ln, N, 6, d_v, W, d_seg, d_run, d_pl, cap, d_tot, stream=sh)

        compact()
        torch.cuda.synchronize(dev)
        t0 = d_tot.cpu().numpy().view(np.uint32).tolist()
        coalesce()
        torch.cuda.synchronize(dev)
        t1 = d_tot.cpu().numpy().view(np.uint32).tolist()
        assert t0[0] == t1[0] == N and t0[2] == t1[2] == 0, (t0, t1)
        print(f"device: {N} segments, {NCONN} connections, W = {W}: {t1[3]} runs, payload bytes "
              f"{t0[1]} padded per segment -> {t1[1]} per run", flush=True)
        runs = {"k (compact)": compact, "k' (compact)": compact, "g (coalesce)": coalesce}
        times = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, fn in runs.items():
                for _ in range(WARM):
                    fn()
                for _ in range(REPS):
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize(dev)
                    times[k].append(a.elapsed_time(e))
        for k, v in times.items():
            m, lo, hi = med(v)
            print(f"device {k}: median {m * 1e3:.1f} us min {lo * 1e3:.1f} max {hi * 1e3:.1f} "
                  f"({len(v)} calls)", flush=True)


def host_side(buf, off, lens):
    ns = R.NStack(0, max_burst=N, max_bytes=N * SLOT)
    try:
        for c in range(NCONN):
            assert ns.lib.nstack_tcb_add(10 | (1 << 8) | ((c >> 8) << 16) | ((c & 255) << 24), R.ip_raw(L),
                                         R.port_raw(40000), R.port_raw(9999), R.TCP_STATUS_ESTABLISHED) == 0
        arr, keep = R.NStack.mbufs_over(buf, off, lens, 6)
        rbuf = np.zeros(1 << 20, np.uint8)
        res = {}
        for rnd in range(ROUNDS):
            for name, w in (("off", 0), ("on", W), ("off'", 0)):
                ns.set_rx_gro(w)
                for timed in (False,) * WARM + (True,) * REPS:
                    f0, a0 = ns.stat(4), ns.stat(15)
                    t0 = time.perf_counter()
                    ns.rx_burst_mbufs(arr, N)
                    t1 = time.perf_counter()
                    items, nbytes = ns.drain_all(rbuf)
                    t2 = time.perf_counter()
                    assert nbytes == N * (FLEN - 54), nbytes
                    if timed:
                        ph = ns.last_burst_phases()
                        res.setdefault(name, []).append((t2 - t0, t1 - t0, ns.stat(4) - f0, ns.stat(15) - a0,
                                                         items, ph["compact"], ph["d2h"], ph["tcp_deliver"]))
        for name, v in res.items():
            col = list(zip(*v))
            m, lo, hi = med(col[0])
            print(f"host gro {name}: rx_burst + reads median {m * 1e3:.3f} ms min {lo * 1e3:.3f} max "
                  f"{hi * 1e3:.3f} -> {N / m / 1e6:.2f} Mpps; rx_burst alone {med(col[1])[0] * 1e3:.3f} ms; "
                  f"fragments/burst {med(col[2])[0]} absorbed/burst {med(col[3])[0]} reads/burst "
                  f"{med(col[4])[0]}; phases ms: K3+K4 {med(col[5])[0]:.3f} copy out {med(col[6])[0]:.3f} "
                  f"tcp delivery {med(col[7])[0]:.3f} ({len(v)} bursts)", flush=True)
    finally:
        ns.fini()


if __name__ == "__main__":
    b = burst()
    device_side(*b)
    host_side(*b[:3])
