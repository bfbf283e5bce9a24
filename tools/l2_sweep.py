"""L2 sweep: what the L2 responder (K8, rxg_l2_dev) costs on the device, in one
process.  It records the cost; it gates nothing.
    python tools/l2_sweep.py [output file]

Three bursts, each classified by K1 on the device first:
  normal   262144 UDP frames of 64 B, no candidate: K8 beside K1's step on the
           same burst (the price of having the pass on);
  arp      16384 who-has frames for the local address (64-B slots), every one
           answered;
  flood    16384 echo requests of 1514 B (1536-B slots), every one answered:
           K8 beside a plain device-to-device copy of the burst's bytes (the
           emit stage's distance from a copy).
Device calls interleaved over rounds, every call timed with HIP events on its
own; medians of 35.  Each K8 call is listed twice per round (x, x'): the spread
of identical runs is the measure for a difference."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
L, LMAC, PMAC = "192.168.100.77", bytes.fromhex("000c296a014d"), bytes.fromhex("02aabbccddee")
ROUNDS, WARM, REPS = 7, 2, 5
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def normal():
    n = 262144
    cfg = R.make_gen_cfg(frame_len=64, slot_bytes=64, n_udp=1024, bad_cksum_per10k=0, unknown_per10k=0,
                         other_per10k=0)
    udp, tcb = R.gen_flows(cfg)
    buf, off, lens = R.gen_host(cfg, 0, n, 6)
    return "normal", buf, off, lens, 64, udp, tcb


def arp_storm():
    n = 16384
    f = np.zeros((n, 64), np.uint8)
    i = np.arange(n)
    f[:, 0:6] = 0xFF
    f[:, 6:12] = np.frombuffer(PMAC, np.uint8)
    f[:, 10], f[:, 11] = i >> 8, i & 255
    f[:, 12:22] = np.frombuffer(bytes.fromhex("08060001080006040001"), np.uint8)
    f[:, 22:28] = f[:, 6:12]
    f[:, 28:32] = np.stack([np.full(n, 10), np.full(n, 7), i >> 8, i & 255], 1)
    f[:, 38:42] = np.frombuffer(bytes(int(x) for x in L.split(".")), np.uint8)
    return "arp", f.reshape(-1), i.astype(np.uint32), np.full(n, 60, np.uint16), 64, None, None


def ping_flood():
    n, flen, slot = 16384, 1514, 1536
    rng = np.random.default_rng(9)
    f = np.zeros((n, slot), np.uint8)
    i = np.arange(n)
    f[:, 0:6] = np.frombuffer(LMAC, np.uint8)
    f[:, 6:12] = np.frombuffer(PMAC, np.uint8)
    f[:, 12:24] = np.frombuffer(bytes([8, 0, 0x45, 0, (flen - 14) >> 8, (flen - 14) & 255, 0, 1, 0x40, 0, 64, 1]),
                                np.uint8)
    f[:, 26:30] = np.stack([np.full(n, 10), np.full(n, 8), i >> 8, i & 255], 1)
    f[:, 30:34] = np.frombuffer(bytes(int(x) for x in L.split(".")), np.uint8)
    f[:, 34] = 8
    f[:, 38:flen] = rng.integers(0, 256, (n, flen - 38), dtype=np.uint8)
    w = f[:, 34:flen].reshape(n, -1, 2).astype(np.uint64)
    s = (w[:, :, 0] * 256 + w[:, :, 1]).sum(1)
    for _ in range(3):
        s = (s & 0xFFFF) + (s >> 16)
    c = (~s) & 0xFFFF
    f[:, 36], f[:, 37] = c >> 8, c & 255
    return "flood", f.reshape(-1), (i * (slot // 64)).astype(np.uint32), np.full(n, flen, np.uint16), flen, None, None


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def device_side(kind, buf, off, lens, hint, udp, tcb):
    dev = torch.device("cuda:0")
    n = len(lens)
    with R.Context(0, max_pkts=n, max_bytes=max(len(buf), 1 << 20)) as ctx:
        if udp is not None:
            ctx.flows_sync(udp, tcb)
        sh = torch.cuda.current_stream(dev).cuda_stream
        d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int32)).to(dev)
        d_ln = torch.from_numpy(lens.view(np.int16)).to(dev)
        d_v = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        cap = len(buf) + 64 * n
        d_st = torch.empty(n, dtype=torch.uint8, device=dev)
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_cp = torch.empty(len(buf), dtype=torch.uint8, device=dev)
        d_ro = torch.empty(n, dtype=torch.int32, device=dev)
        d_rl = torch.empty(n, dtype=torch.int16, device=dev)
        d_rs = torch.empty(n, dtype=torch.int32, device=dev)
        d_tot = torch.zeros(6, dtype=torch.int32, device=dev)
        p = R.l2_params([(L, LMAC)])

        def k1():
            ctx.classify_dev(d_pk, d_off, d_ln, n, 6, hint, d_v, None, stream=sh)

        def k8():
            ctx.l2_dev(d_pk, d_off, d_ln, n, 6, d_v, p, d_st, d_out, cap, d_ro, d_rl, d_rs, d_tot, stream=sh)

        def copy():
            d_cp.copy_(d_pk[:len(buf)])

        k1()
        k8()
        torch.cuda.synchronize(dev)
        tot = d_tot.cpu().numpy().view(np.uint32).tolist()
        want = {"normal": [0, 0, 0, 0, 0, 0], "arp": [n, 0, 0, 0, n, n],
                "flood": [0, 0, n, 0, n, n * 24]}[kind]
        assert tot == want, (kind, tot)
        say(f"{kind}: {n} frames, {len(buf)} B: totals {tot}")
        runs = {"k8": k8, "k1 (classify)": k1, "copy (device to device)": copy, "k8'": k8}
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
        sys.exit("l2_sweep.py needs a GPU")
    for make in (normal, arp_storm, ping_flood):
        device_side(*make())
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(_lines) + "\n")
