"""Reference for the UDP compaction tests (K3) — test infrastructure.

A plain numpy/Python model of what include/rxgpu.h promises for
rxg_udp_compact_dev, the batched form of udp_process's delivery half
(udp.c:25-52), written without librxgpu and without the kernel's tiling:
  delivered  a frame whose verdict says cls == CLS_UDP, rc == 0 and
             flow_id < nflows (udp.c:14-19 found the socket)
  order      delivered frames grouped by socket id, burst order inside a
             socket (the order rte_ring_mp_enqueue, udp.c:48, gives its ring)
  record     rxg_dgram {frame, offset, sip, sport, len}: len = the verdict's
             payload_len (dgram_len - 8, udp.c:38), sip / sport the raw bytes
             26..29 / 34..35 (udp.c:33-34), bytes at or past the capture as 0
  payload    min(len, max(caplen - 42, 0)) bytes from byte 42 (udp + 1,
             udp.c:46) at the next 16-B aligned offset, zeros to its padded end
  first      first[f] = rank of socket f's first datagram, first[nflows] = all
  totals     {datagrams, padded payload bytes, 1 if a payload's padded end
             passes payload_cap}; such a payload is not written
Shared by the model's own pin against the delivery oracle (test_rx_compact.py)
and the device tests (test_gpu_compact.py, test_gpu_compact_edges.py)."""
from collections import namedtuple

import numpy as np

CLS_UDP = 3  # RXG_CLS_UDP, include/rxgpu.h
DGRAM_DTYPE = np.dtype([("frame", "<u4"), ("offset", "<u4"), ("sip", "<u4"), ("sport", "<u2"),
                        ("len", "<u2")])  # rxg_dgram
Compacted = namedtuple("Compacted", "dgram first payload totals written ncopy")


def delivered(v, nflows):
    """burst indices of the delivered frames, in burst order"""
    return np.nonzero((v["cls"] == CLS_UDP) & (v["rc"] == 0) & (v["flow_id"] < nflows))[0]


def compact(frames, caplens, v, nflows, payload_cap=None) -> Compacted:
    """frames[i][:caplens[i]] is what was captured of frame i, v its verdict.
    payload: totals[1] bytes as a buffer of any size would hold them; written:
    per byte, False inside a payload that payload_cap (None = no limit) left
    out; ncopy: captured payload bytes of every record"""
    deliv = delivered(v, nflows)
    flow = v["flow_id"][deliv].astype(np.int64)
    order = deliv[np.argsort(flow, kind="stable")]
    first = np.searchsorted(np.sort(flow), np.arange(nflows + 1)).astype(np.uint32)
    dgram = np.zeros(len(order), DGRAM_DTYPE)
    ncopy = np.zeros(len(order), np.int64)
    chunks, marks, pos, over = [], [], 0, 0
    for r, i in enumerate(order):
        f = bytes(frames[i][:int(caplens[i])])
        head = f[:42] + bytes(42 - min(len(f), 42))  # bytes past the capture read as 0
        plen = int(v["payload_len"][i])
        data = f[42:42 + plen]
        pad = (len(data) + 15) // 16 * 16
        dgram[r] = (i, pos, int.from_bytes(head[26:30], "little"),
                    int.from_bytes(head[34:36], "little"), plen)
        ncopy[r] = len(data)
        fits = payload_cap is None or pos + pad <= payload_cap
        over |= not fits
        chunks.append(data + bytes(pad - len(data)))
        marks.append(np.full(pad, fits))
        pos += pad
    payload = np.frombuffer(b"".join(chunks), np.uint8)
    written = np.concatenate(marks) if marks else np.zeros(0, bool)
    totals = np.array([len(order), pos, over], np.uint32)
    return Compacted(dgram, first, payload, totals, written, ncopy)


def socket_slices(c: Compacted, nflows):
    """per socket, its datagrams in ring order as (sip, sport, len, the len
    payload bytes a reader gets: the captured ones, then zeros)"""
    out = []
    for f in range(nflows):
        q = []
        for r in range(int(c.first[f]), int(c.first[f + 1])):
            d, k = c.dgram[r], int(c.ncopy[r])
            o = int(d["offset"])
            data = c.payload[o:o + k].tobytes() + bytes(int(d["len"]) - k)
            q.append((int(d["sip"]), int(d["sport"]), int(d["len"]), data))
        out.append(q)
    return out
