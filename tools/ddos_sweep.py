"""DDoS sweep: what the entropy flood detector (K6, rxg_ddos_dev) costs on the
device, against a plain read of the same bytes and K1 on the same burst in
the same process.  Tuning only.
    python tools/ddos_sweep.py [frames per burst [output file]]

Bursts from rxg_gen_dev: the cfg2 shape (64-B UDP in 64-B slots), the cfg3
shape (1500-B TCP in 1536-B slots) and an IMIX mix (64 / 576 / 1500 at 7:4:1,
packed at 64-B alignment).

Device calls, interleaved over rounds, every call timed with HIP events on
its own; medians:
  k1, k1'    rxg_classify_dev on the burst, the yardstick, twice per round:
             the spread of identical runs is the measure for a difference;
  read       the plain-read ceiling of tools/libceiling.so (ceiling_slot_ms's
             stream read) over the burst's span of bytes;
  bits G     the bits pass alone with G lanes per frame forced, and auto;
  window     the window pass with the state update, on computed bits;
  whole      rxg_ddos_dev, auto.
Each pass is then printed as a fraction of the plain read and of k1."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpdk-tcp-udp_protocol_stack_amd"))
import rxgpu as R  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 18
OUT = sys.argv[2] if len(sys.argv) > 2 else None
ROUNDS, WARM, REPS = 7, 2, 5
SHAPES = {
    "cfg2 (64 B)": dict(frame_len=64, slot_bytes=64, n_udp=1024),
    "cfg3 (1500 B in 1536-B slots)": dict(frame_len=1500, slot_bytes=1536, proto_mode=1, n_udp=0, n_tcp=4096),
    "imix (64/576/1500 at 7:4:1, packed)": dict(size_mode=1, slot_bytes=1536, packed=1, n_udp=1024),
}
_lines = []


def say(s):
    print(s, flush=True)
    _lines.append(s)


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def shape(name, kw, ceiling):
    dev = torch.device("cuda:0")
    n = N if kw["slot_bytes"] == 64 else N // 8
    cfg = R.make_gen_cfg(**kw)
    udp, tcb = R.gen_flows(cfg)
    with R.Context(0) as ctx:
        ctx.flows_sync(udp if len(udp) else None, tcb if len(tcb) else None)
        sh = torch.cuda.current_stream(dev).cuda_stream
        d_pk = torch.zeros(n * cfg.slot_bytes + 64, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n, dtype=torch.int32, device=dev)
        d_ln = torch.zeros(n, dtype=torch.int16, device=dev)
        R.gen_dev(cfg, 0, n, d_pk, d_off, d_ln, 6, stream=sh)
        torch.cuda.synchronize(dev)
        off = d_off.cpu().numpy().view(np.uint32)
        ln = d_ln.cpu().numpy().view(np.uint16)
        span = ((int(off[-1]) << 6) + int(ln[-1]) + 63) // 64 * 64
        hint = int(ln.astype(np.int64).sum() // n)
        say(f"{name}: {n} frames, {int(ln.astype(np.int64).sum())} frame bytes in a span of {span} B, "
            f"len_hint {hint}")
        d_v = torch.empty(n * 16, dtype=torch.uint8, device=dev)
        d_bits = torch.empty(n, dtype=torch.int32, device=dev)
        d_state = torch.zeros(R.DDOS_STATE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(R.DDOS_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)

        def k1():
            ctx.classify_dev(d_pk, d_off, d_ln, n, 6, hint, d_v, None, stream=sh)

        def bits(_g):
            def fn():
                ctx.ddos_bits_dev(d_pk, d_off, d_ln, n, 6, hint, d_bits, stream=sh)
            return fn

        def window():
            ctx.ddos_window_dev(d_bits, d_ln, n, 1200.0, d_state, None, None, d_sum, stream=sh)

        def whole():
            ctx.ddos_dev(d_pk, d_off, d_ln, n, 6, hint, 1200.0, d_state, None, None, None, d_sum, stream=sh)

        # name -> (lanes per frame set before the calls, the timed call)
        runs = {"k1": (0, k1), "k1'": (0, k1)}
        for g in R.DDOS_LANES:
            runs[f"bits G={g}"] = (g, bits(g))
        runs["bits auto"] = (0, bits(0))
        runs["window"] = (0, window)
        runs["whole"] = (0, whole)
        times = {k: [] for k in runs}
        times["read"] = []
        for _ in range(ROUNDS):
            for k, (g, fn) in runs.items():
                ctx.tune_ddos(g)
                for _ in range(WARM):
                    fn()
                for _ in range(REPS):
                    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    e.record()
                    torch.cuda.synchronize(dev)
                    times[k].append(a.elapsed_time(e))
            if ceiling is not None:  # (its own stream and events; the median of 5 launches)
                torch.cuda.synchronize(dev)
                s_ms, r_ms = C.c_double(0.0), C.c_double(0.0)
                rc = ceiling.ceiling_slot_ms(C.c_int(0), C.c_void_p(d_pk.data_ptr()),
                                             C.c_ulonglong(span // 64), C.c_uint(64), C.c_uint(64),
                                             C.c_int(5), C.byref(s_ms), C.byref(r_ms))
                if rc == 0:
                    times["read"].append(r_ms.value)
        m = {}
        for k, v in times.items():
            if not v:
                say(f"{name} {k}: not measured")
                continue
            m[k], lo, hi = med(v)
            say(f"{name} {k}: median {m[k] * 1e3:.1f} us min {lo * 1e3:.1f} max {hi * 1e3:.1f} "
                f"({len(v)} calls)")
        for k in [x for x in m if x.startswith(("bits", "window", "whole"))]:
            rd = f"{m[k] / m['read']:.2f} of the plain read" if "read" in m else "plain read not measured"
            say(f"{name} {k}: {rd}, {m[k] / m['k1']:.2f} of k1")
        summ = d_sum.cpu().numpy().view(R.DDOS_SUMMARY_DTYPE)[0]
        say(f"{name}: after the sweep frames_seen {int(summ['frames_seen'])}, last D "
            f"{float(summ['last_stat']):.1f}, alarm {int(summ['flag'])}")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("ddos_sweep.py needs a GPU")
    p = os.path.join(ROOT, "tools", "libceiling.so")
    ceiling = C.CDLL(p) if os.path.exists(p) else None
    if ceiling is None:
        say("tools/libceiling.so not built: the plain read is not measured")
    for name, kw in SHAPES.items():
        shape(name, kw, ceiling)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(_lines) + "\n")
