"""Fragmentation sweep: what cutting UDP datagrams at the MTU inside the TX
encoder costs against the same volume from datagrams cut beforehand,
interleaved over rounds in one process, medians.  Tuning only.
    python tools/frag_sweep.py [case,case,...]

For every case about the same number of frames and bytes is produced two ways:
  (a) rxg_tx_encode_dev on UDP descriptors whose payloads were cut on the host
      beforehand into pieces of mtu - 28 bytes, each its own datagram at its own
      16-B aligned offset: the only way to emit that volume before
      rxg_tx_encode_frag_dev.  Timed twice in every round (a, a'): the spread
      of identical runs is the yardstick for (b).
  (b) rxg_tx_encode_frag_dev on the uncut descriptors.
Before timing, both outputs are compared byte for byte with the host
statement (rxg_tx_encode_host, rxg_tx_encode_frag_host) on the first CHECK_ND
datagrams: packed frames follow each other, so a prefix of the burst lies
where it would lie alone.

Bytes: descriptors + payload read + 64-B-rounded frames written (+ the map
word and the partial-sum word, written and read, per frame for (b)), against
the 8 TB/s spec."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

# name: (payload bytes per datagram, mtu, output frames wanted, len_hint)
CASES = {"64K@1500": (65507, 1500, 1 << 19, 1500), "8K@1500": (8192, 1500, 1 << 19, 1500),
         "64K@9000": (65507, 9000, 1 << 17, 9000), "64K@1500x4M": (65507, 1500, 1 << 22, 1500)}
names = sys.argv[1].split(",") if len(sys.argv) > 1 else list(CASES)
ROUNDS, WARM, REPS, CHECK_ND = 5, 2, 6, 64
dev = torch.device("cuda:0")
ctx = R.Context(0, max_pkts=1024, max_bytes=1 << 20)
sh = torch.cuda.current_stream(dev).cuda_stream


def descriptors(nd, pay_len, row16):
    t = np.zeros(nd, R.TXD_DTYPE)
    k = np.arange(nd)
    t["dst_mac"], t["src_mac"] = 0x02, 0x0C
    t["sip"], t["dip"] = 0x4D64A8C0, 0x0A000000 + k
    t["sport"], t["dport"] = k & 0xFFFF, 53
    t["seq"] = k + 1  # the IPv4 id
    t["kind"], t["pay_len"], t["pay_off16"] = R.TXD_UDP, pay_len, k * row16
    return t


def precut(t, piece, s, seg16):
    """one datagram per piece; piece e's payload at e * seg16 16-B units"""
    g = np.repeat(t, s)
    j = np.tile(np.arange(s), len(t))
    g["pay_len"] = np.minimum(piece, g["pay_len"].astype(np.int64) - j * piece)
    g["pay_off16"] = np.arange(len(g)) * seg16
    return g


def u32(x):
    return x.cpu().numpy().view(np.uint32)


for nm in names:
    pay_len, mtu, frames, hint = CASES[nm]
    fp, piece = (mtu - 20) & ~7, mtu - 28
    s = -(-(8 + pay_len) // fp)
    assert s == -(-pay_len // piece)  # the same frame count both ways
    nd = frames // s
    ne = nd * s
    row = (pay_len + 15) // 16 * 16
    seg = (piece + 15) // 16 * 16
    t = descriptors(nd, pay_len, row // 16)
    g = precut(t, piece, s, seg // 16)
    d_t = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
    d_g = torch.from_numpy(g.view(np.uint8).copy()).to(dev)
    pay_b = torch.randint(0, 256, (nd, row), dtype=torch.uint8, device=dev)
    pay_b[:, pay_len:] = 0
    # (a)'s buffer: the same bytes, every piece moved to its own 16-B aligned row
    pay_a = torch.zeros((nd, s, seg), dtype=torch.uint8, device=dev)
    wide = torch.zeros((nd, s * piece), dtype=torch.uint8, device=dev)
    wide[:, :pay_len] = pay_b[:, :pay_len]
    pay_a[:, :, :piece] = wide.view(nd, s, piece)
    del wide
    pay_a, pay_b = pay_a.reshape(-1), pay_b.reshape(-1)
    pay_a = torch.cat([pay_a, torch.zeros(16, dtype=torch.uint8, device=dev)])
    pay_b = torch.cat([pay_b, torch.zeros(16, dtype=torch.uint8, device=dev)])
    ent_a, cap_a = R.tx_frag_count(g, 0, 0)
    ent_b, cap_b = R.tx_frag_count(t, 0, mtu)
    assert ent_a == ent_b == ne
    out_a = torch.empty(cap_a, dtype=torch.uint8, device=dev)
    out_b = torch.empty(cap_b, dtype=torch.uint8, device=dev)
    off_a, off_b = (torch.empty(ne, dtype=torch.int32, device=dev) for _ in range(2))
    len_a, len_b = (torch.empty(ne, dtype=torch.int16, device=dev) for _ in range(2))
    first, nseg = (torch.empty(nd, dtype=torch.int32, device=dev) for _ in range(2))
    tot_a = torch.zeros(4, dtype=torch.int32, device=dev)
    tot_b = torch.zeros(8, dtype=torch.int32, device=dev)

    def run_a():
        ctx.tx_encode_dev(d_g, ne, pay_a, out_a, cap_a, 0, off_a, len_a, hint, 0, tot_a, sh)

    def run_b():
        ctx.tx_encode_frag_dev(d_t, nd, pay_b, 0, mtu, out_b, cap_b, 0, off_b, len_b, ne, first, nseg,
                               hint, 0, tot_b, sh)

    run_a()
    run_b()
    torch.cuda.synchronize(dev)
    assert u32(tot_a).tolist() == [ne, cap_a & 0xFFFFFFFF, cap_a >> 32, 0], u32(tot_a)
    assert u32(tot_b).tolist()[:6] == [ne, cap_b & 0xFFFFFFFF, cap_b >> 32, 0, ne, 0], u32(tot_b)
    # the host statement on a prefix of the burst
    cn = min(nd, CHECK_ND)
    ce = cn * s
    h_pa = pay_a[:ce * seg].cpu().numpy()
    h_pb = pay_b[:cn * row].cpu().numpy()
    _, cb_a = R.tx_frag_count(g[:ce], 0, 0)
    _, cb_b = R.tx_frag_count(t[:cn], 0, mtu)
    wa = R.tx_encode_host(g[:ce], h_pa, cb_a)
    wb = R.tx_encode_frag_host(t[:cn], h_pb, 0, mtu, cb_b, ce)
    assert wa[5] == 0 and wb[7] == 0
    assert np.array_equal(out_a[:cb_a].cpu().numpy(), wa[0])
    assert np.array_equal(u32(off_a[:ce]), wa[1])
    assert np.array_equal(len_a[:ce].cpu().numpy().view(np.uint16), wa[2])
    assert np.array_equal(out_b[:cb_b].cpu().numpy(), wb[0])
    assert np.array_equal(u32(off_b[:ce]), wb[1])
    assert np.array_equal(len_b[:ce].cpu().numpy().view(np.uint16), wb[2])
    assert np.array_equal(u32(first[:cn]), wb[3]) and np.array_equal(u32(nseg[:cn]), wb[4])
    assert (u32(nseg) == s).all()
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
    byt = {"a": 48 * ne + pay_bytes + cap_a, "a'": 48 * ne + pay_bytes + cap_a,
           "b": 48 * nd + 12 * ne + pay_bytes + cap_b}
    med = {}
    for k, v in times.items():
        v = sorted(v)
        med[k] = v[ROUNDS // 2]
        print(f"{nm} ({nd} datagrams x {s} fragments = {ne} frames) {k}: median {med[k]:.4f} ms min "
              f"{v[0]:.4f} max {v[-1]:.4f} -> {ne / med[k] / 1e3:.0f} Mpps {byt[k] / med[k] / 1e6:.0f} GB/s "
              f"({byt[k] / med[k] / 8e9:.3f} of 8 TB/s)", flush=True)
    a1, a2 = med["a"], med["a'"]
    print(f"{nm} b against the mean of a and a': {100 * (2 * med['b'] / (a1 + a2) - 1):+.1f} % "
          f"(a against a': {100 * (a1 / a2 - 1):+.1f} %)", flush=True)
    del d_t, d_g, pay_a, pay_b, out_a, out_b, off_a, off_b, len_a, len_b, first, nseg
    torch.cuda.empty_cache()
ctx.close()
