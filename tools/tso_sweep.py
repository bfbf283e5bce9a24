"""TSO sweep: what cutting TCP payloads inside the TX encoder costs against the
same frames from pre-split descriptors, interleaved over rounds in one
process, medians.  Tuning only.
    python tools/tso_sweep.py [case,case,...]

For every case the same output bytes are produced two ways:
  (a) rxg_tx_encode_dev on one descriptor per segment, split on the host
      beforehand (what a caller had to do before rxg_tx_encode_tso_dev); its
      payload buffer holds every segment at its own 16-B aligned offset, as
      that call requires.  Timed twice in every round (a, a'): the spread of
      identical runs is the yardstick for (b).
  (b) rxg_tx_encode_tso_dev on the unsplit descriptors.
The two outputs are compared byte for byte once before timing.

Bytes: descriptors + payload read + 64-B-rounded frames written (+ the map
word per frame for (b)), against the 8 TB/s spec."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

# name: (payload bytes per descriptor, mss, output frames wanted, len_hint)
CASES = {"64K@1460": (65536, 1460, 1 << 19, 1500), "16K@1460": (16384, 1460, 1 << 19, 1500),
         "64K@8948": (65536, 8948, 1 << 17, 9000), "64K@1460x4M": (65536, 1460, 1 << 22, 1500)}
names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(CASES)
ROUNDS, WARM, REPS = 5, 2, 6
dev = torch.device("cuda:0")
ctx = R.Context(0, max_pkts=1024, max_bytes=1 << 20)
sh = torch.cuda.current_stream(dev).cuda_stream


def descriptors(nd, pay_len, row16):
    t = np.zeros(nd, R.TXD_DTYPE)
    k = np.arange(nd)
    t["dst_mac"], t["src_mac"] = 0x02, 0x0C
    t["sip"], t["dip"] = 0x4D64A8C0, 0x0A000000 + k
    t["sport"], t["dport"] = k & 0xFFFF, 80
    t["seq"], t["ack"] = (k * 2654435761) & 0xFFFFFFFF, 7
    t["window"], t["hdrlen_off"], t["tcp_flags"] = 14600, 0x50, 0x18
    t["kind"], t["pay_len"], t["pay_off16"] = R.TXD_TCP, pay_len, k * row16
    return t


def presplit(t, mss, s, seg16):
    """one descriptor per segment; segment e's payload at e * seg16 16-B units"""
    g = np.repeat(t, s)
    j = np.tile(np.arange(s), len(t))
    g["seq"] = (g["seq"].astype(np.int64) + j * mss) & 0xFFFFFFFF
    g["pay_len"] = np.minimum(mss, g["pay_len"].astype(np.int64) - j * mss)
    g["tcp_flags"] = np.where(j == s - 1, g["tcp_flags"], g["tcp_flags"] & 0xF6)
    g["pay_off16"] = np.arange(len(g)) * seg16
    return g


for nm in names:
    pay_len, mss, frames, hint = CASES[nm]
    s = -(-pay_len // mss)
    nd = frames // s
    ne = nd * s
    row = (pay_len + 15) // 16 * 16
    seg = (mss + 15) // 16 * 16
    t = descriptors(nd, pay_len, row // 16)
    g = presplit(t, mss, s, seg // 16)
    d_t = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
    d_g = torch.from_numpy(g.view(np.uint8).copy()).to(dev)
    pay_b = torch.randint(0, 256, (nd, row), dtype=torch.uint8, device=dev)
    pay_b[:, pay_len:] = 0
    # (a)'s buffer: the same bytes, every segment moved to its own 16-B aligned row
    pay_a = torch.zeros((nd, s, seg), dtype=torch.uint8, device=dev)
    wide = torch.zeros((nd, s * mss), dtype=torch.uint8, device=dev)
    wide[:, :pay_len] = pay_b[:, :pay_len]
    pay_a[:, :, :mss] = wide.view(nd, s, mss)
    del wide
    pay_a, pay_b = pay_a.reshape(-1), pay_b.reshape(-1)
    pay_a = torch.cat([pay_a, torch.zeros(16, dtype=torch.uint8, device=dev)])
    pay_b = torch.cat([pay_b, torch.zeros(16, dtype=torch.uint8, device=dev)])
    ent, cap = R.tx_tso_count(t, mss)
    assert ent == ne
    out_a = torch.empty(cap, dtype=torch.uint8, device=dev)
    out_b = torch.empty(cap, dtype=torch.uint8, device=dev)
    off_a, off_b = (torch.empty(ne, dtype=torch.int32, device=dev) for _ in range(2))
    len_a, len_b = (torch.empty(ne, dtype=torch.int16, device=dev) for _ in range(2))
    first, nseg = (torch.empty(nd, dtype=torch.int32, device=dev) for _ in range(2))
    tot_a = torch.zeros(4, dtype=torch.int32, device=dev)
    tot_b = torch.zeros(8, dtype=torch.int32, device=dev)

    def run_a():
        ctx.tx_encode_dev(d_g, ne, pay_a, out_a, cap, 0, off_a, len_a, hint, 0, tot_a, sh)

    def run_b():
        ctx.tx_encode_tso_dev(d_t, nd, pay_b, mss, out_b, cap, 0, off_b, len_b, ne, first, nseg, hint,
                              0, tot_b, sh)

    run_a()
    run_b()
    torch.cuda.synchronize(dev)
    u32 = lambda x: x.cpu().numpy().view(np.uint32).tolist()  # noqa: E731
    assert u32(tot_a) == [ne, cap & 0xFFFFFFFF, cap >> 32, 0], u32(tot_a)
    assert u32(tot_b)[:6] == [ne, cap & 0xFFFFFFFF, cap >> 32, 0, ne, 0], u32(tot_b)
    assert torch.equal(out_a, out_b) and torch.equal(off_a, off_b) and torch.equal(len_a, len_b)
    runs = {"a": run_a, "a'": run_a, "b": run_b}
    times = {k: [] for k in runs}
    for rnd in range(ROUNDS):
        for k, fn in runs.items():
            for _ in range(WARM):
                fn()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                fn()
            e.record()
            torch.cuda.synchronize(dev)
            times[k].append(a.elapsed_time(e) / REPS)
    pay_bytes = nd * pay_len
    byt = {"a": 48 * ne + pay_bytes + cap, "a'": 48 * ne + pay_bytes + cap,
           "b": 48 * nd + 4 * ne + pay_bytes + cap}
    for k, v in times.items():
        v = sorted(v)
        med = v[ROUNDS // 2]
        print(f"{nm} ({nd} descriptors x {s} segments = {ne} frames) {k}: median {med:.4f} ms min "
              f"{v[0]:.4f} max {v[-1]:.4f} -> {ne / med / 1e3:.0f} Mpps {byt[k] / med / 1e6:.0f} GB/s "
              f"({byt[k] / med / 8e9:.3f} of 8 TB/s)", flush=True)
    del d_t, d_g, pay_a, pay_b, out_a, out_b, off_a, off_b, len_a, len_b, first, nseg
    torch.cuda.empty_cache()
ctx.close()
