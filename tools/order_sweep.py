"""Order sweep: what TCP sequence ordering costs on the device, against K4
without it in the same process, and what it gives coalescing back.  Tuning only.
    python tools/order_sweep.py [segments per connection [output file]]

The burst is the socket bench's cfg3 shape: 16384 segments of 1500-B TCP
(PSH|ACK, 1446 payload bytes) over 16384 / PER established connections (PER =
4 by default), the connections interleaved frame by frame as a NIC delivers
them.  Three arrival orders of the same segments:
  in-order   every connection's segments in sequence;
  swapped    one adjacent pair per connection swapped (its segments 1 and 2);
  reversed   every connection's segments reversed.

Device calls on the classified burst, interleaved over rounds, every call
timed with HIP events on its own; medians:
  k, k'      rxg_tcp_compact_dev, the yardstick, twice per round: the spread
             of identical runs is the measure for a difference;
  o0         rxg_tcp_compact_ordered_dev, W = 0;
  o64        rxg_tcp_compact_ordered_dev, W = 64 KiB;
  g64        rxg_tcp_coalesce_dev, W = 64 KiB (what o64 adds ordering to).
Per burst it also prints moved, and the runs (receive fragments) of
coalescing alone against coalescing with ordering."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

PER = int(sys.argv[1]) if len(sys.argv) > 1 else 4
OUT = sys.argv[2] if len(sys.argv) > 2 else None
N, FLEN, SLOT = 16384, 1500, 1536
NCONN = N // PER
W = 65536
L = "192.168.100.77"
ROUNDS, WARM, REPS = 7, 2, 5
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def burst(kind):
    """the packed burst (64-B units) with both checksums filled by K2; kind:
    the place in sequence of connection c's q-th arriving segment"""
    rng = np.random.default_rng(3)
    f = np.zeros((N, SLOT), np.uint8)
    i = np.arange(N)
    c, q = i % NCONN, i // NCONN
    if kind == "swapped":
        a, b = (1, 2) if PER > 2 else (0, 1)
        q = np.where(q == a, b, np.where(q == b, a, q))
    elif kind == "reversed":
        q = PER - 1 - q
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


def device_side(kind, buf, off, lens, tcb):
    dev = torch.device("cuda:0")
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
        d_tot = torch.zeros(5, dtype=torch.int32, device=dev)

        def compact():
            ctx.tcp_compact_dev(d_pk, d_off, d_ln, N, 6, d_v, d_seg, d_pl, cap, d_tot, stream=sh)

        def coalesce():
            ctx.tcp_coalesce_dev(d_pk, d_off, d_ln, N, 6, d_v, W, d_seg, d_run, d_pl, cap, d_tot, stream=sh)

        def ordered0():
            ctx.tcp_compact_ordered_dev(d_pk, d_off, d_ln, N, 6, d_v, 0, d_seg, None, d_pl, cap, d_tot,
                                        stream=sh)

        def ordered64():
            ctx.tcp_compact_ordered_dev(d_pk, d_off, d_ln, N, 6, d_v, W, d_seg, d_run, d_pl, cap, d_tot,
                                        stream=sh)

        tot = {}
        for name, fn in (("k", compact), ("g64", coalesce), ("o0", ordered0), ("o64", ordered64)):
            d_tot.zero_()
            fn()
            torch.cuda.synchronize(dev)
            tot[name] = d_tot.cpu().numpy().view(np.uint32).tolist()
            assert tot[name][0] == N and tot[name][2] == 0, (name, tot[name])
        assert tot["o0"][4] == tot["o64"][4]
        say(f"{kind}: {N} segments, {NCONN} connections x {PER}: moved {tot['o0'][4]}; fragments per "
            f"burst (runs, W = {W}): coalescing alone {tot['g64'][3]}, with ordering {tot['o64'][3]}")
        runs = {"k (compact)": compact, "k' (compact)": compact, "o0 (ordered, W = 0)": ordered0,
                "g64 (coalesce)": coalesce, "o64 (ordered, W = 64 KiB)": ordered64}
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
            say(f"{kind} device {k}: median {m * 1e3:.1f} us min {lo * 1e3:.1f} max {hi * 1e3:.1f} "
                f"({len(v)} calls)")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("order_sweep.py needs a GPU")
    for kind in ("in-order", "swapped", "reversed"):
        device_side(kind, *burst(kind))
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(_lines) + "\n")
