"""Assemble sweep: what TCP stream assembly costs on the device, against the
ordering form of K4 on the same burst in the same process.  It records the
cost; it gates nothing.
    python tools/assemble_sweep.py [segments per connection [output file]]

The burst: 16384 segments of 1460 payload bytes (1514-B TCP frames, PSH|ACK)
over 16384 / PER established connections (PER = 4 by default), the connections
interleaved frame by frame as a NIC delivers them, every connection's segments
in sequence.  Two forms of it:
  clean        every byte once;
  duplicates   about 10 % of the frames repeat the segment their connection
               sent before them (a retransmitted duplicate, byte for byte).

Device calls on the classified burst, interleaved over rounds, every call
timed with HIP events on its own; medians:
  o0, o0'    rxg_tcp_compact_ordered_dev, W = 0, the yardstick, twice per
             round: the spread of identical runs is the measure for a
             difference;
  o64        rxg_tcp_compact_ordered_dev, W = 64 KiB;
  k          rxg_tcp_compact_dev (K4 without ordering);
  a, a'      rxg_tcp_assemble_dev, twice per round.
Per burst it also prints the streams, the bytes laid down and the bytes
skipped, beside the runs and bytes of the ordered coalescing form."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

PER = int(sys.argv[1]) if len(sys.argv) > 1 else 4
OUT = sys.argv[2] if len(sys.argv) > 2 else None
N, PAY, SLOT = 16384, 1460, 1536
FLEN = 54 + PAY
NCONN = N // PER
W = 65536
L = "192.168.100.77"
ROUNDS, WARM, REPS = 7, 2, 5
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def burst(kind):
    """the packed burst (64-B units) with both checksums filled by K2"""
    rng = np.random.default_rng(5)
    f = np.zeros((N, SLOT), np.uint8)
    i = np.arange(N)
    c, q = i % NCONN, i // NCONN
    dup = np.zeros(N, bool)
    if kind == "duplicates":        # odd places only, so the segment before is no duplicate itself
        dup = (q % 2 == 1) & (rng.random(N) < 0.2)
    fresh = (~dup).reshape(PER, NCONN)
    place = (np.cumsum(fresh, axis=0) - fresh).reshape(N) - dup     # the place in sequence
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
    seq = (c * 2654435761 + place * PAY) & 0xFFFFFFFF
    f[:, 38:42] = seq.astype(">u4").view(np.uint8).reshape(N, 4)
    f[:, 42:46] = (0, 0, 0x07, 0xD0)
    f[:, 46], f[:, 47] = 0x50, 0x18
    f[:, 48:50] = (0x39, 0x08)
    f[:, 54:FLEN] = rng.integers(0, 256, (N, PAY), dtype=np.uint8)
    d = np.nonzero(dup)[0]
    f[d, 54:FLEN] = f[d - NCONN, 54:FLEN]                            # the bytes sent before
    off = (i * (SLOT // 64)).astype(np.uint32)
    lens = np.full(N, FLEN, np.uint16)
    tcb = np.zeros(NCONN + 1, R.TCB_DTYPE)
    tcb["sip"][:NCONN] = sip[:NCONN]
    tcb["dip"], tcb["sport"], tcb["dport"] = R.ip_raw(L), R.port_raw(40000), R.port_raw(9999)
    tcb["status"][:NCONN] = R.TCP_STATUS_ESTABLISHED
    tcb[NCONN] = (0, R.ip_raw(L), 0, R.port_raw(9999), R.TCP_STATUS_LISTEN)
    with R.Context(0, max_pkts=N, max_bytes=N * SLOT) as ctx:
        buf = ctx.tx_cksum(f.reshape(-1), off, lens, 6)
    return buf, off, lens, tcb, int(dup.sum())


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def device_side(kind, buf, off, lens, tcb, ndup):
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
        d_run = torch.empty(N * 32, dtype=torch.uint8, device=dev)      # (runs or streams)
        d_pl = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_tot = torch.zeros(6, dtype=torch.int32, device=dev)

        def compact():
            ctx.tcp_compact_dev(d_pk, d_off, d_ln, N, 6, d_v, d_seg, d_pl, cap, d_tot, stream=sh)

        def ordered0():
            ctx.tcp_compact_ordered_dev(d_pk, d_off, d_ln, N, 6, d_v, 0, d_seg, None, d_pl, cap, d_tot,
                                        stream=sh)

        def ordered64():
            ctx.tcp_compact_ordered_dev(d_pk, d_off, d_ln, N, 6, d_v, W, d_seg, d_run, d_pl, cap, d_tot,
                                        stream=sh)

        def assemble():
            ctx.tcp_assemble_dev(d_pk, d_off, d_ln, N, 6, d_v, d_seg, d_run, d_pl, cap, d_tot, stream=sh)

        tot = {}
        for name, fn in (("o0", ordered0), ("o64", ordered64), ("a", assemble)):
            d_tot.zero_()
            fn()
            torch.cuda.synchronize(dev)
            tot[name] = d_tot.cpu().numpy().view(np.uint32).tolist()
            assert tot[name][0] == N and tot[name][2] == 0, (name, tot[name])
        assert tot["a"][3] == NCONN and tot["a"][5] == ndup * PAY, tot["a"]
        say(f"{kind}: {N} segments of {PAY} B, {NCONN} connections x {PER}, {ndup} duplicates: assembly "
            f"{tot['a'][3]} streams, {tot['a'][1]} B laid down, {tot['a'][5]} B skipped; ordered "
            f"coalescing (W = {W}) {tot['o64'][3]} runs, {tot['o64'][1]} B; ordered K4 {tot['o0'][1]} B")
        runs = {"o0 (ordered, W = 0)": ordered0, "a (assemble)": assemble,
                "o64 (ordered, W = 64 KiB)": ordered64, "k (compact)": compact,
                "o0' (ordered, W = 0)": ordered0, "a' (assemble)": assemble}
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
        sys.exit("assemble_sweep.py needs a GPU")
    for kind in ("clean", "duplicates"):
        device_side(kind, *burst(kind))
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(_lines) + "\n")
