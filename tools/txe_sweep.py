"""K5 (TX encode) variant sweep: times every tx_encode variant (rxg_tune_txe) at
the bench workloads' frame shapes, against K2 (rxg_tx_cksum_dev) over the
equivalent pre-encoded burst, interleaved over rounds in one process.  Tuning
only.
    python tools/txe_sweep.py cfg2,cfg3,cfg4,cfg5 [variants] [--k2-lib other/librxgpu.so]

Descriptors come from an rxg_gen_dev burst: addresses, ports, TCP fields and
lengths of its frames, one descriptor per frame, in the workload's own layout
(fixed slots, or packed for cfg4).  The payload buffer is the generated burst
itself: descriptor k's payload is the pay_len bytes at frame k's (64-B aligned)
start, so the payload reads have the sizes and spacing of the workload and no
second copy of it is needed.  K2 runs over the encoder's own output.
--k2-lib: also time K2 of another build of the library (the parent commit's)
over the same burst, in the same rounds.

Bytes: 48 + payload read and the 64-B-rounded frame written per frame (K5);
frame + 10 per frame (K2, as tools/tx_sweep.py), against the 8 TB/s spec."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxdist  # noqa: E402
import rxgpu as R  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
k2_lib = sys.argv[sys.argv.index("--k2-lib") + 1] if "--k2-lib" in sys.argv else None
if k2_lib:
    args.remove(k2_lib)
names = args[0].split(",") if args else ["cfg2", "cfg3", "cfg4", "cfg5"]
variants = [int(x) for x in args[1].split(",")] if len(args) > 1 else list(range(15))
ROUNDS, WARM, REPS = 5, 2, 8
dev = torch.device("cuda:0")
ctx = R.Context(0, max_pkts=1024, max_bytes=1 << 20)


class OtherK2:
    """rxg_tx_cksum_dev of another build of the library"""

    def __init__(self, path):
        self.lib = C.CDLL(os.path.abspath(path))
        vp, u32 = C.c_void_p, C.c_uint32
        self.lib.rxg_open.argtypes = [C.POINTER(vp), C.c_int, u32, C.c_uint64]
        self.lib.rxg_tx_cksum_dev.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp]
        self.h = vp()
        assert self.lib.rxg_open(C.byref(self.h), 0, 1024, 1 << 20) == 0

    def __call__(self, pk, off, ln, n, hint, sh):
        assert self.lib.rxg_tx_cksum_dev(self.h, pk.data_ptr(), off.data_ptr(), ln.data_ptr(), n, 6,
                                         hint, sh) == 0


other = OtherK2(k2_lib) if k2_lib else None


def descriptors(pk, off, ln, n):
    """one rxg_txd per generated frame (int32[n, 12])"""
    txd = torch.empty((n, 12), dtype=torch.int32, device=dev)
    step = 1 << 20
    for a in range(0, n, step):
        b = min(n, a + step)
        base = off[a:b].to(torch.int64) << 6
        idx = base[:, None] + torch.arange(64, device=dev)
        h = pk[idx].to(torch.int64)
        fl = ln[a:b].to(torch.int64) & 0xFFFF

        def w(b0, b1, b2, b3):
            return h[:, b0] | h[:, b1] << 8 | h[:, b2] << 16 | h[:, b3] << 24

        tcp = (h[:, 12] == 8) & (h[:, 13] == 0) & (h[:, 23] == 6) & (fl >= 54)
        kind = torch.where(tcp, R.TXD_TCP, R.TXD_UDP)  # (anything else goes out as UDP of its length)
        pay = torch.clamp(fl - torch.where(tcp, 54, 42), min=0)
        cols = [w(0, 1, 2, 3), w(4, 5, 6, 7), w(8, 9, 10, 11), w(26, 27, 28, 29), w(30, 31, 32, 33),
                w(34, 35, 36, 37), w(41, 40, 39, 38), w(45, 44, 43, 42), w(48, 49, 52, 53),
                h[:, 46] | h[:, 47] << 8 | kind << 24, off[a:b].to(torch.int64) << 2, pay]
        txd[a:b] = torch.stack(cols, 1).to(torch.int32)
        del idx, h
    return txd


for nm in names:
    w = rxdist.WORKLOADS[nm]
    cfg = rxdist.gen_cfg(nm, bad_cksum_per10k=0)
    n, hint = w["n"], w["len_hint"]
    sh = torch.cuda.current_stream(dev).cuda_stream
    src = torch.empty(n * cfg.slot_bytes + 64, dtype=torch.uint8, device=dev)
    off = torch.empty(n, dtype=torch.int32, device=dev)
    ln = torch.empty(n, dtype=torch.int16, device=dev)
    R.gen_dev(cfg, 0, n, src, off, ln, w["unit_log2"], stream=sh)
    torch.cuda.synchronize(dev)
    txd = descriptors(src, off, ln, n)
    slot = 0 if cfg.packed else cfg.slot_bytes
    flen = 42 + (txd[:, 11].to(torch.int64) + 12 * (txd[:, 9] >> 24 & 1))
    fb = int(flen.sum().item())
    wr = int(((flen + 63) & ~63).sum().item())
    cap = n * slot if slot else wr
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    o_off = torch.empty(n, dtype=torch.int32, device=dev)
    o_len = torch.empty(n, dtype=torch.int16, device=dev)
    tot = torch.zeros(4, dtype=torch.int32, device=dev)
    txe_b = 48 * n + (fb - 42 * n - 12 * int((txd[:, 9] >> 24 & 1).sum().item())) + wr
    k2_b = fb + 10 * n

    def encode():
        ctx.tx_encode_dev(txd, n, src, out, cap, slot, o_off, o_len, hint, 0, tot, sh)

    runs = {("txe", v): (lambda v=v: (ctx.tune_txe(v), encode())) for v in variants}
    runs[("txe", "auto")] = lambda: (ctx.tune_txe(R.TX_AUTO), encode())
    runs[("k2", "this")] = lambda: ctx.tx_cksum_dev(out, o_off, o_len, n, 6, hint, stream=sh)
    if other:
        runs[("k2", "other")] = lambda: other(out, o_off, o_len, n, hint, sh)
    encode()
    torch.cuda.synchronize(dev)
    t4 = tot.cpu().numpy()
    assert int(t4[0]) == n and int(t4[3]) == 0, t4
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
    for (what, v), t in times.items():
        t = sorted(t)
        byt = txe_b if what == "txe" else k2_b
        print(f"{what} {nm} variant={v}: median {t[ROUNDS // 2]:.4f} ms min {t[0]:.4f} max {t[-1]:.4f} -> "
              f"{n / t[ROUNDS // 2] / 1e3:.0f} Mpps {byt / t[ROUNDS // 2] / 1e6:.0f} GB/s "
              f"({byt / t[ROUNDS // 2] / 8e9:.3f} of 8 TB/s)", flush=True)
    del src, off, ln, txd, out, o_off, o_len
    torch.cuda.empty_cache()
ctx.tune_txe(R.TX_AUTO)
ctx.close()
