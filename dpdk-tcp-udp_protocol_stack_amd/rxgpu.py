"""ctypes binding of librxgpu.so (include/rxgpu.h) and libnstack.so (include/nstack.h).

This module is plumbing for tests and bench.py: every verdict it returns is
computed by the gfx950 kernel in librxgpu.so.  There is no Python or CPU
fallback — if the shared library is missing, importing this module raises.

Reference interface mirrored (see include/rxgpu.h for file:line citations):
  pkt_process loop body (netfamily.c:152-200) -> Context.classify* / process_mbufs
  udp_process / tcp_process return codes       -> verdict['rc']
  get_hostinfo_fromip_port / tcp_stream_search -> verdict['flow_id'], lookup_udp/lookup_tcp
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RXGPU_LIB: another build of the same library (A/B of compile-time variants)
LIB_PATH = os.environ.get("RXGPU_LIB") or os.path.join(_HERE, "librxgpu.so")
# NSTACK_LIB: another build of the socket layer (e.g. a sanitizer build, host code only)
NSTACK_PATH = os.environ.get("NSTACK_LIB") or os.path.join(_HERE, "libnstack.so")

# One HIP runtime per process: PyTorch (the plumbing for device memory, streams
# and torch.distributed) ships its own libamdhip64.so.7 with the same SONAME as
# /opt/rocm's.  Loading torch first makes librxgpu bind to that copy; loading
# librxgpu first would bring a second HIP/HSA runtime into the process, and the
# two then contend for the device (observed: hipGetDeviceCount fails in one).
try:
    import torch  # noqa: F401
except ImportError:  # a pure-C deployment links /opt/rocm's runtime directly
    pass

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {_HERE}` (or __graft_entry__.build()); "
        "there is no fallback path")
_lib = C.CDLL(LIB_PATH)

# ---- constants (mirror include/rxgpu.h) -----------------------------------
FLOW_NONE = 0xFFFFFFFF
CLS_ARP, CLS_NON_IP, CLS_IPV4_OTHER, CLS_UDP, CLS_TCP = 0, 1, 2, 3, 4
RC_OK, RC_TCP_BAD_CKSUM, RC_TCP_NO_TCB, RC_UDP_NOMEM, RC_UDP_NO_SOCKET, RC_KNI = 0, -1, -2, -2, -3, 1
F_TRUNC, F_TCP_NEGLEN, F_UDP_SHORT = 0x1, 0x2, 0x4
TCP_STATUS_LISTEN, TCP_STATUS_ESTABLISHED = 1, 4
HOST_ONLY = -1
# the product library's classify variants (csrc/rx_classify.hip k_variants):
# (lanes per frame, passes up front, frames per group, pipeline); every one
# gives the reference's verdicts (tests/test_gpu_parity.py runs each)
KERNEL_VARIANTS = [(1, 4, 1, 12), (1, 4, 1, 5), (1, 4, 1, 14), (1, 4, 1, 19), (1, 4, 1, 25), (1, 4, 1, 16),
                   (1, 4, 1, 0),
                   (4, 1, 1, 1), (8, 2, 2, 0), (8, 2, 2, 40), (8, 2, 2, 41), (8, 2, 2, 42), (8, 2, 2, 48),
                   (8, 2, 1, 0), (16, 2, 2, 0),
                   (32, 3, 2, 0), (64, 4, 1, 0),
                   (0, 0, 0, 20),  # size-class binned: lane kernel + G=8 kernel
                   (0, 0, 0, 30), (0, 0, 0, 38), (0, 0, 0, 738), (0, 0, 0, 938),  # stream kernel
                   (0, 0, 0, 60), (0, 0, 0, 64), (0, 0, 0, 67)]  # SH kernel
# compiled only into the RX_DIAG build (librxgpu_diag.so, RXGPU_LIB=...):
# tuning shapes with correct verdicts ...
DIAG_TUNING_VARIANTS = [(1, 4, 1, 13), (1, 4, 1, 18), (1, 4, 1, 23), (1, 4, 1, 24), (1, 4, 1, 21), (1, 4, 1, 22), (8, 2, 2, 1), (16, 2, 1, 0),
                        (8, 2, 2, 43), (8, 2, 2, 44), (8, 2, 2, 45), (8, 2, 2, 46),
                        (8, 2, 2, 47), (8, 2, 2, 49), (8, 2, 2, 50), (8, 2, 2, 51), (8, 2, 2, 52), (8, 2, 2, 53), (8, 2, 2, 54), (8, 2, 2, 55), (8, 2, 2, 56), (0, 0, 0, 54), (0, 0, 0, 66),
                        (0, 0, 0, 68), (0, 0, 0, 75), (0, 0, 0, 65),
                        (0, 0, 0, 80), (0, 0, 0, 81), (0, 0, 0, 82), (0, 0, 0, 83)]  # WC kernel
# ... and ablations, wrong verdicts (or counts) by construction
DIAG_ABLATIONS = [(1, 4, 1, 101), (1, 4, 1, 104), (1, 4, 1, 108), (1, 4, 1, 113), (1, 4, 1, 201),
                  (1, 4, 1, 204), (1, 4, 1, 213), (0, 0, 0, 130), (0, 0, 0, 46), (0, 0, 0, 146),
                  (0, 0, 0, 246), (0, 0, 0, 446), (0, 0, 0, 646), (0, 0, 0, 438), (0, 0, 0, 838),
                  (0, 0, 0, 1238), (0, 0, 0, 160), (0, 0, 0, 264), (0, 0, 0, 1064),
                  (0, 0, 0, 2064), (0, 0, 0, 167),
                  (1, 4, 1, 1401), (1, 4, 1, 1404), (1, 4, 1, 1408), (1, 4, 1, 1413), (1, 4, 1, 1604), (0, 0, 0, 1667), (0, 0, 0, 6467)]

VERDICT_DTYPE = np.dtype([
    ("flow_id", "<u4"), ("payload_off", "<u2"), ("payload_len", "<u2"), ("l4_cksum", "<u2"),
    ("cls", "u1"), ("rc", "i1"), ("cksum_ok", "u1"), ("flags", "u1"), ("stored_cksum", "<u2"),
])
assert VERDICT_DTYPE.itemsize == 16
# rxg_verdict8 (rxg_classify_dev8): off_neg = payload_off | TCP_NEGLEN << 7,
# status = cls | (rc & 7) << 3 | cksum_ok << 6 | TRUNC << 7
VERDICT8_DTYPE = np.dtype([("flow_id", "<u4"), ("payload_len", "<u2"), ("off_neg", "u1"),
                           ("status", "u1")])
assert VERDICT8_DTYPE.itemsize == 8


def verdict8_of(v: np.ndarray) -> np.ndarray:
    """the 8-B verdicts of 16-B ones (rxg_verdict8_of in include/rxgpu.h)"""
    v = np.ascontiguousarray(v).view(VERDICT_DTYPE)
    r = np.empty(v.shape, VERDICT8_DTYPE)
    r["flow_id"] = v["flow_id"]
    r["payload_len"] = v["payload_len"]
    r["off_neg"] = (v["payload_off"] & 0x7F) | np.where(v["flags"] & 0x02, 0x80, 0)
    r["status"] = ((v["cls"] & 7) | ((v["rc"].view(np.uint8) & 7) << 3) | ((v["cksum_ok"] & 1) << 6)
                   | np.where(v["flags"] & 0x01, 0x80, 0)).astype(np.uint8)
    return r


UDP_SOCK_DTYPE = np.dtype([("localip", "<u4"), ("localport", "<u2"), ("protocol", "u1"),
                           ("_pad", "u1")])
TCB_DTYPE = np.dtype([("sip", "<u4"), ("dip", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                      ("status", "<u4")])
DGRAM_DTYPE = np.dtype([("frame", "<u4"), ("offset", "<u4"), ("sip", "<u4"), ("sport", "<u2"),
                        ("len", "<u2")])
assert DGRAM_DTYPE.itemsize == 16
COMPACT_MAX_FLOWS = 1024
SEGMENT_DTYPE = np.dtype([("frame", "<u4"), ("flow", "<u4"), ("seq", "<u4"), ("ack", "<u4"),
                          ("plen", "<i4"), ("offset", "<u4"), ("sport", "<u2"), ("dport", "<u2"),
                          ("ncopy", "<u2"), ("flags", "u1"), ("hl", "u1")])
assert SEGMENT_DTYPE.itemsize == 32
# rxg_tcp_run, a run of receive coalescing (rxg_tcp_coalesce_dev / rxg_tcp_runs_host)
TCP_RUN_DTYPE = np.dtype([("first", "<u4"), ("nseg", "<u4"), ("bytes", "<u4"), ("offset", "<u4")])
# the entropy flood detector (K6): rxg_ddos_state / rxg_ddos_summary and the
# per-frame flag bits
DDOS_WINDOW, DDOS_TILE, DDOS_DEFAULT_THRESH = 256, 256, 1200.0
DDOS_WARMUP, DDOS_UNDEF, DDOS_ALARM, DDOS_RISE, DDOS_FALL = 0x01, 0x02, 0x04, 0x08, 0x10
DDOS_LANES = (1, 8, 64)  # lanes per frame of the bits pass compiled in (tune_ddos; 0 = auto)
DDOS_STATE_DTYPE = np.dtype([("frames_seen", "<u8"), ("flag", "<u4"), ("_r0", "<u4"),
                             ("set", "<u4", (DDOS_WINDOW,)), ("tot", "<u4", (DDOS_WINDOW,))])
assert DDOS_STATE_DTYPE.itemsize == 2064
DDOS_SUMMARY_DTYPE = np.dtype([("frames_seen", "<u8"), ("last_stat", "<f8"), ("alarm_frames", "<u4"),
                               ("first_alarm", "<u4"), ("rises", "<u4"), ("falls", "<u4"),
                               ("undef_frames", "<u4"), ("flag", "<u4"), ("last_set", "<u4"),
                               ("last_tot", "<u4")])
assert DDOS_SUMMARY_DTYPE.itemsize == 48
NSTACK_DDOS_DTYPE = np.dtype([("frames_seen", "<u8"), ("rises", "<u8"), ("falls", "<u8"),
                              ("alarm_frames", "<u8"), ("undef_frames", "<u8"), ("last_stat", "<f8"),
                              ("alarm", "<u4"), ("_r0", "<u4")])
assert TCP_RUN_DTYPE.itemsize == 16
GRO_MAX_WINDOW, GRO_DEFAULT_WINDOW = 1 << 20, 65536
DLV_TCP_IN_PLACE, DLV_TCP_GRO, DLV_TCP_ORDER = 0x1, 0x2, 0x4
DLV_TCP_ASSEMBLE = 0x20
# rxg_tcp_stream, a contiguous byte range of one connection (stream assembly)
TCP_STREAM_DTYPE = np.dtype([("first", "<u4"), ("nseg", "<u4"), ("seq", "<u4"), ("ack", "<u4"),
                             ("bytes", "<u4"), ("offset", "<u4"), ("flags", "<u4"),
                             ("reserved", "<u4")])
assert TCP_STREAM_DTYPE.itemsize == 32
STREAM_FIN, STREAM_HOLE = 0x1, 0x2
# rxg_txd, the send descriptor of the TX encoder (K5): sip/dip/sport/dport/
# window/urp raw as the reference stores them, seq/ack host order
TXD_DTYPE = np.dtype([("dst_mac", "u1", (6,)), ("src_mac", "u1", (6,)), ("sip", "<u4"), ("dip", "<u4"),
                      ("sport", "<u2"), ("dport", "<u2"), ("seq", "<u4"), ("ack", "<u4"),
                      ("window", "<u2"), ("urp", "<u2"), ("hdrlen_off", "u1"), ("tcp_flags", "u1"),
                      ("optlen", "u1"), ("kind", "u1"), ("pay_off16", "<u4"), ("pay_len", "<u4")])
assert TXD_DTYPE.itemsize == 48
TXD_UDP, TXD_TCP, TXD_ARP = 0, 1, 2
TXE_NO_CKSUM = 0x1


class Delivery(C.Structure):
    """rxg_delivery (rxg_process_mbufs_deliver's results)"""
    _fields_ = [("dgram", C.c_void_p), ("first", C.c_void_p), ("udp_payload", C.c_void_p),
                ("ndgram", C.c_uint32), ("nseg", C.c_uint32), ("udp_bytes", C.c_uint64),
                ("seg", C.c_void_p), ("tcp_payload", C.c_void_p), ("tcp_bytes", C.c_uint64),
                ("tcp_payload_ref", C.c_int32), ("set", C.c_uint32)]


class GenCfg(C.Structure):
    """rxg_gen_cfg"""
    _fields_ = [
        ("seed", C.c_uint64), ("size_mode", C.c_uint32), ("frame_len", C.c_uint32),
        ("slot_bytes", C.c_uint32), ("proto_mode", C.c_uint32), ("n_udp", C.c_uint32),
        ("n_tcp", C.c_uint32), ("local_ip", C.c_uint32), ("udp_base_port", C.c_uint16),
        ("tcp_port", C.c_uint16), ("bad_cksum_per10k", C.c_uint32),
        ("unknown_per10k", C.c_uint32), ("other_per10k", C.c_uint32), ("shard", C.c_uint32),
        ("n_shards", C.c_uint32), ("packed", C.c_uint32), ("src_ip", C.c_uint32),
        ("src_port", C.c_uint16), ("_pad", C.c_uint16),
    ]


class Mbuf(C.Structure):
    """rxg_mbuf: rte_mbuf-shaped descriptor (buf_addr@0, data_off@16, refcnt@18,
    data_len@40)."""
    _fields_ = [("buf_addr", C.c_void_p), ("_r0", C.c_uint8 * 8), ("data_off", C.c_uint16),
                ("refcnt", C.c_uint16), ("_r1", C.c_uint8 * 20), ("data_len", C.c_uint16),
                ("_r2", C.c_uint8 * 86)]


assert C.sizeof(Mbuf) == 128

_vp, _u32, _u64, _i32, _u16 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_uint16


def _sig(name, res, *args):
    f = getattr(_lib, name)
    f.restype = res
    f.argtypes = list(args)
    return f


_open = _sig("rxg_open", _i32, C.POINTER(_vp), _i32, _u32, _u64)
_close = _sig("rxg_close", None, _vp)
_strerror = _sig("rxg_strerror", C.c_char_p, _i32)
_last_hip = _sig("rxg_last_hip_error", C.c_char_p)
_flows_sync = _sig("rxg_flows_sync", _i32, _vp, _vp, _u32, _vp, _u32)
_flows_add = _sig("rxg_flows_add", _i32, _vp, _vp, _u32, _vp, _u32, _vp, _vp)
_flows_remove = _sig("rxg_flows_remove", _i32, _vp, _vp, _u32, _vp, _u32)
_flows_update_udp = _sig("rxg_flows_update_udp", _i32, _vp, _u32, _vp)
_flows_update_tcb = _sig("rxg_flows_update_tcb", _i32, _vp, _u32, _vp)
_flows_commit = _sig("rxg_flows_commit", _i32, _vp, _vp)
_num_udp_ids = _sig("rxg_num_udp_ids", _u32, _vp)
_udp_compact_dev = _sig("rxg_udp_compact_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp,
                        _vp, _u64, _vp, _vp)
_flows_rebuilds = _sig("rxg_flows_rebuilds", _u32, _vp)
_tcp_compact_dev = _sig("rxg_tcp_compact_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp,
                        _u64, _vp, _vp)
_tcp_coalesce_dev = _sig("rxg_tcp_coalesce_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _u32, _vp,
                         _vp, _vp, _u64, _vp, _vp)
_tcp_runs_host = _sig("rxg_tcp_runs_host", _i32, _vp, _vp, _u32, _u32, _vp, C.POINTER(_u32))
_tcp_compact_ordered_dev = _sig("rxg_tcp_compact_ordered_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32,
                                _vp, _u32, _vp, _vp, _vp, _u64, _vp, _vp)
_tcp_order_host = _sig("rxg_tcp_order_host", _i32, _vp, _vp, _u32, _vp, C.POINTER(_u32))
_delivery_moved = _sig("rxg_delivery_moved", _i32, _vp, _vp, C.POINTER(_u32))
_tcp_assemble_dev = _sig("rxg_tcp_assemble_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp,
                         _vp, _u64, _vp, _vp)
_tcp_assemble_host = _sig("rxg_tcp_assemble_host", _i32, _vp, _vp, _vp, _u32, _vp, C.POINTER(_u32),
                          _vp, _vp, _vp)
_delivery_streams = _sig("rxg_delivery_streams", _i32, _vp, _vp, C.POINTER(_vp), C.POINTER(_u32))
_f64 = C.c_double
_ddos_dev = _sig("rxg_ddos_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _f64, _vp, _vp, _vp, _vp,
                 _vp, _vp)
_ddos_bits_dev = _sig("rxg_ddos_bits_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp)
_ddos_window_dev = _sig("rxg_ddos_window_dev", _i32, _vp, _vp, _vp, _u32, _f64, _vp, _vp, _vp, _vp, _vp)
_ddos_host = _sig("rxg_ddos_host", _i32, _vp, _vp, _vp, _u32, _u32, _f64, _vp, _vp, _vp, _vp, _vp)
_ddos_entropy = _sig("rxg_ddos_entropy", _f64, _f64, _f64)
_tune_ddos = _sig("rxg_tune_ddos", _i32, _vp, _u32)
_tune_ddos_thresh = _sig("rxg_tune_ddos_thresh", _i32, _vp, _f64)
_ddos_reset = _sig("rxg_ddos_reset", _i32, _vp)
_delivery_ddos = _sig("rxg_delivery_ddos", _i32, _vp, _vp, _vp)
DLV_DDOS = 0x10
# SYN cookies (K7): rxg_ck_params, the per-frame status values, the flag
CK_PARAMS_DTYPE = np.dtype([("k0", "<u8"), ("k1", "<u8"), ("t", "<u4"), ("max_age", "<u4"),
                            ("window", "<u2"), ("_r0", "<u2"), ("_r1", "<u4")])
assert CK_PARAMS_DTYPE.itemsize == 32
CK_SYN, CK_ACK_OK, CK_ACK_BAD, CK_DEFAULT_MAX_AGE = 1, 2, 3, 2
DLV_SYNCOOKIE = 0x80
_syncookie_value = _sig("rxg_syncookie_value", _u32, _u64, _u64, _u32, _u32, _u16, _u16, _u32, _u32)
_siphash24 = _sig("rxg_siphash24", _u64, _u64, _u64, _vp, _u64)
_syncookie_dev = _sig("rxg_syncookie_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp,
                      _vp, _vp, _vp, _vp)
_syncookie_host = _sig("rxg_syncookie_host", _i32, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, _vp, _vp,
                       _vp, _vp)
_syncookie_set = _sig("rxg_syncookie_set", _i32, _vp, _vp, _vp, _u32)
_syncookie_tick = _sig("rxg_syncookie_tick", _i32, _vp, _u32)
_delivery_cookies = _sig("rxg_delivery_cookies", _i32, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp),
                         C.POINTER(_u32), _vp)
# the L2 responder (K8): rxg_l2_params, the per-frame status values, the flag
L2_MAX_LOCAL = 8
L2_PARAMS_DTYPE = np.dtype([("nlocal", "<u4"),
                            ("local", [("ip", "<u4"), ("mac", "u1", 6), ("_r", "<u2")], L2_MAX_LOCAL)])
assert L2_PARAMS_DTYPE.itemsize == 100
L2_ARP_REQ, L2_ARP_REPLY, L2_ECHO, L2_ECHO_BAD = 1, 2, 3, 4
DLV_L2 = 0x100
_l2_dev = _sig("rxg_l2_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp,
               _vp, _vp, _vp)
_l2_host = _sig("rxg_l2_host", _i32, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp,
                _vp)
_l2_set = _sig("rxg_l2_set", _i32, _vp, _vp, _u64)
_delivery_l2 = _sig("rxg_delivery_l2", _i32, _vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp),
                    C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u32), _vp)
_tune_deliver = _sig("rxg_tune_deliver", _i32, _vp, _u32)
_tune_gro = _sig("rxg_tune_gro", _i32, _vp, _u32)
_delivery_runs = _sig("rxg_delivery_runs", _i32, _vp, _vp, C.POINTER(_vp), C.POINTER(_u32))
_process_mbufs_deliver = _sig("rxg_process_mbufs_deliver", _i32, _vp, _vp, _u32, _vp, _vp, _vp)
_deliver_submit = _sig("rxg_deliver_submit", _i32, _vp, _vp, _u32, _vp, _vp)
_tune_ingest = _sig("rxg_tune_ingest", _i32, _vp, _u32)
INGEST_AUTO, INGEST_PULL, INGEST_GATHER = 0, 1, 2
_deliver_wait = _sig("rxg_deliver_wait", _i32, _vp, _vp, _vp)
_register_host = _sig("rxg_register_host", _i32, _vp, _vp, _u64)
_payload_hold = _sig("rxg_payload_hold", _i32, _vp, _i32)
_payload_release = _sig("rxg_payload_release", _i32, _vp, _i32)
_unregister_host = _sig("rxg_unregister_host", _i32, _vp, _vp)
_classify_dev = _sig("rxg_classify_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp)
_classify_dev_cs = _sig("rxg_classify_dev_cs", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp,
                        _vp, _vp)
# (older builds, e.g. an A/B against a previous library, lack it: classify_dev8 then raises)
_classify_dev8 = (_sig("rxg_classify_dev8", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp,
                       _vp, _vp) if hasattr(_lib, "rxg_classify_dev8") else None)
_classify = _sig("rxg_classify", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _vp)
_classify_span = _sig("rxg_classify_span", _i32, _vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp)
_process_mbufs = _sig("rxg_process_mbufs", _i32, _vp, _vp, _u32, _vp)
_flow_counts = _sig("rxg_flow_counts", _i32, _vp, _vp, _u32)
_counts_reset = _sig("rxg_counts_reset", _i32, _vp)
_num_flows = _sig("rxg_num_flows", _u32, _vp)
_tune = _sig("rxg_tune", _i32, _vp, _u32, _u32, _u32, _u32)
_tune_grid = _sig("rxg_tune_grid", _i32, _vp, _u32)
_kernel_variant = (_sig("rxg_kernel_variant", _i32, _vp, _u32, _vp, C.c_char_p, _u32)
                   if hasattr(_lib, "rxg_kernel_variant") else None)
_tune_tx = _sig("rxg_tune_tx", _i32, _vp, _u32, _u32)
_tune_flow_load = _sig("rxg_tune_flow_load", _i32, _vp, _u32)
_tune_tables = _sig("rxg_tune_tables", _i32, _vp, _u32)
TT_NO_UDP_PORT = 0x1
TT_COUNT_4B = 0x2
TT_COUNT_2BUF = 0x4
TT_SLAB_HALF = 0x8     # the slab pass on half / a quarter of the CUs (fewer, larger slabs)
TT_SLAB_QUARTER = 0x10
TX_AUTO = 0xFFFFFFFF
_lk_udp = _sig("rxg_ft_lookup_udp", _u32, _vp, _u32, _u16)
_lk_tcp = _sig("rxg_ft_lookup_tcp", _u32, _vp, _u32, _u32, _u16, _u16)
_ft_dump = _sig("rxg_ft_dump", _i32, _vp, _u32, _i32, _vp, _u64, _vp)
_rss = _sig("rxg_rss_hash", _u32, _u32, _u32, _u16, _u16)
_gen_flows = _sig("rxg_gen_flows", _i32, C.POINTER(GenCfg), _vp, _vp)
_gen_host = _sig("rxg_gen_host", _i32, C.POINTER(GenCfg), _u64, _u32, _vp, _vp, _vp, _u32)
_gen_dev = _sig("rxg_gen_dev", _i32, C.POINTER(GenCfg), _u64, _u32, _vp, _vp, _vp, _u32, _vp)
_submit = _sig("rxg_submit", _i32, _vp, _vp, _u64, _vp, _vp, _u32, _u32, _vp, C.POINTER(_u64))
_wait = _sig("rxg_wait", _i32, _vp, _u64)
_pcap_open = _sig("rxg_pcap_open", _i32, C.POINTER(_vp), C.c_char_p)
_pcap_close = _sig("rxg_pcap_close", None, _vp)
_pcap_rewind = _sig("rxg_pcap_rewind", _i32, _vp)
_pcap_read = _sig("rxg_pcap_read_burst", _i32, _vp, _vp, _u64, _vp, _vp, _u32, _u32,
                  C.POINTER(_u32), C.POINTER(_u64))
_pcap_write = _sig("rxg_pcap_write", _i32, C.c_char_p, _vp, _vp, _vp, _u32, _u32)
_tx_cksum_dev = _sig("rxg_tx_cksum_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp)
_tx_cksum = _sig("rxg_tx_cksum", _i32, _vp, _vp, _u64, _vp, _vp, _u32, _u32)
_tx_encode_dev = _sig("rxg_tx_encode_dev", _i32, _vp, _vp, _u32, _vp, _vp, _u64, _u32, _vp, _vp, _u32,
                      _u32, _vp, _vp)
_tx_encode = _sig("rxg_tx_encode", _i32, _vp, _vp, _u32, _vp, _u64, _vp, _u64, _vp, _vp, _u32,
                  C.POINTER(_u64))
_tx_encode_host = _sig("rxg_tx_encode_host", _i32, _vp, _u32, _vp, _u64, _vp, _u64, _u32, _vp, _vp,
                       _u32, C.POINTER(_u64), _vp)
_tx_encode_tso_dev = _sig("rxg_tx_encode_tso_dev", _i32, _vp, _vp, _u32, _vp, _u32, _vp, _u64, _u32,
                          _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp)
_tx_encode_tso = _sig("rxg_tx_encode_tso", _i32, _vp, _vp, _u32, _vp, _u64, _u32, _vp, _u64, _vp, _vp,
                      _u32, _vp, _vp, _u32, C.POINTER(_u64))
_tx_encode_tso_host = _sig("rxg_tx_encode_tso_host", _i32, _vp, _u32, _vp, _u64, _u32, _vp, _u64, _u32,
                           _vp, _vp, _u32, _vp, _vp, _u32, C.POINTER(_u64), _vp)
_tx_tso_count = _sig("rxg_tx_tso_count", _i32, _vp, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64))
_tx_encode_frag_dev = _sig("rxg_tx_encode_frag_dev", _i32, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _u64,
                           _u32, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp)
_tx_encode_frag = _sig("rxg_tx_encode_frag", _i32, _vp, _vp, _u32, _vp, _u64, _u32, _u32, _vp, _u64,
                       _vp, _vp, _u32, _vp, _vp, _u32, C.POINTER(_u64))
_tx_encode_frag_host = _sig("rxg_tx_encode_frag_host", _i32, _vp, _u32, _vp, _u64, _u32, _u32, _vp,
                            _u64, _u32, _vp, _vp, _u32, _vp, _vp, _u32, C.POINTER(_u64), _vp)
_tx_frag_count = _sig("rxg_tx_frag_count", _i32, _vp, _u32, _u32, _u32, C.POINTER(_u64),
                      C.POINTER(_u64))
_tune_txe = _sig("rxg_tune_txe", _i32, _vp, _u32, _u32)
_rss_split = _sig("rxg_rss_split", _i32, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp)
_rss_split_dev = _sig("rxg_rss_split_dev", _i32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp,
                      _vp)
_gather_dev = _sig("rxg_gather_dev", _i32, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _u64, _vp, _vp,
                   C.POINTER(_u64), _vp)
_group_id = _sig("rxg_group_id", _i32, _vp)
_group_open = _sig("rxg_group_open", _i32, C.POINTER(_vp), _i32, _u32, _u32, _vp)
_group_close = _sig("rxg_group_close", None, _vp)
_group_size = _sig("rxg_group_size", _i32, _vp, C.POINTER(_u32), C.POINTER(_u32))
_counts_allreduce = _sig("rxg_counts_allreduce", _i32, _vp, _vp, _u32, _vp)
_ctx_counts_allreduce = _sig("rxg_ctx_counts_allreduce", _i32, _vp, _vp)
PIPE_DEPTH = 3
SLAB_MIN_FLOWS = 8193  # from here up the per-flow counts are slab passes after the classify kernel
MAX_SHARDS = 64
GROUP_ID_BYTES = 128

EXPORTED = ["rxg_open", "rxg_close", "rxg_strerror", "rxg_last_hip_error", "rxg_flows_sync",
            "rxg_flows_add", "rxg_flows_remove", "rxg_flows_update_udp", "rxg_flows_update_tcb",
            "rxg_flows_commit", "rxg_num_udp_ids", "rxg_flows_rebuilds", "rxg_udp_compact_dev",
            "rxg_process_mbufs_udp", "rxg_tcp_compact_dev", "rxg_tcp_coalesce_dev",
            "rxg_tcp_runs_host", "rxg_tcp_compact_ordered_dev", "rxg_tcp_order_host",
            "rxg_delivery_moved", "rxg_tcp_assemble_dev", "rxg_tcp_assemble_host",
            "rxg_delivery_streams", "rxg_tune_deliver", "rxg_tune_gro", "rxg_delivery_runs",
            "rxg_process_mbufs_deliver",
            "rxg_deliver_submit", "rxg_deliver_wait", "rxg_tune_ingest",
            "rxg_register_host", "rxg_unregister_host", "rxg_payload_hold", "rxg_payload_release",
            "rxg_classify_dev", "rxg_classify_dev_cs", "rxg_classify_dev8", "rxg_classify", "rxg_classify_span", "rxg_process_mbufs", "rxg_flow_counts",
            "rxg_counts_reset", "rxg_num_flows", "rxg_tune", "rxg_kernel_variant", "rxg_tune_grid", "rxg_tune_tx", "rxg_tune_flow_load", "rxg_tune_tables", "rxg_ft_lookup_udp", "rxg_ft_lookup_tcp", "rxg_ft_dump",
            "rxg_rss_hash", "rxg_gen_flows", "rxg_gen_host", "rxg_gen_dev", "rxg_submit", "rxg_wait",
            "rxg_pcap_open", "rxg_pcap_close", "rxg_pcap_rewind", "rxg_pcap_read_burst",
            "rxg_pcap_write", "rxg_tx_cksum_dev", "rxg_tx_cksum", "rxg_tx_encode_dev",
            "rxg_tx_encode", "rxg_tx_encode_host", "rxg_tx_encode_tso_dev", "rxg_tx_encode_tso",
            "rxg_tx_encode_tso_host", "rxg_tx_tso_count", "rxg_tx_encode_frag_dev",
            "rxg_tx_encode_frag", "rxg_tx_encode_frag_host", "rxg_tx_frag_count", "rxg_tune_txe", "rxg_rss_split",
            "rxg_rss_split_dev", "rxg_gather_dev", "rxg_group_id", "rxg_group_open",
            "rxg_group_close", "rxg_group_size", "rxg_counts_allreduce", "rxg_ctx_counts_allreduce",
            "rxg_ddos_dev", "rxg_ddos_bits_dev", "rxg_ddos_window_dev", "rxg_ddos_host",
            "rxg_ddos_entropy", "rxg_tune_ddos", "rxg_tune_ddos_thresh", "rxg_ddos_reset",
            "rxg_delivery_ddos", "rxg_syncookie_value", "rxg_siphash24", "rxg_syncookie_dev",
            "rxg_syncookie_host", "rxg_syncookie_set", "rxg_syncookie_tick", "rxg_delivery_cookies",
            "rxg_l2_dev", "rxg_l2_host", "rxg_l2_set", "rxg_delivery_l2"]


class RxgError(RuntimeError):
    def __init__(self, rc: int, what: str):
        msg = _strerror(rc).decode()
        if rc in (-1000, -1001):
            msg += " [" + _last_hip().decode() + "]"
        super().__init__(f"{what}: {msg} ({rc})")
        self.rc = rc


def _check(rc: int, what: str):
    if rc != 0:
        raise RxgError(rc, what)


def _ptr(a: np.ndarray | None):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays passed to librxgpu must be contiguous"
    return a.ctypes.data


def _tptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else t.data_ptr()


# ---- byte-order helpers (raw network-order values as the reference stores them)
def ip_raw(dotted: str) -> int:
    b = bytes(int(x) for x in dotted.split("."))
    return int.from_bytes(b, "little")


def port_raw(port: int) -> int:
    return int.from_bytes(port.to_bytes(2, "big"), "little")


class Context:
    """rxg_ctx: one per rx thread (device = HIP ordinal, or HOST_ONLY)."""

    def __init__(self, device: int = 0, max_pkts: int = 0, max_bytes: int = 0):
        h = _vp()
        _check(_open(C.byref(h), device, max_pkts, max_bytes), "rxg_open")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            _close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def flows_sync(self, udp: np.ndarray | None = None, tcb: np.ndarray | None = None):
        udp = np.ascontiguousarray(udp if udp is not None else np.zeros(0, UDP_SOCK_DTYPE),
                                   UDP_SOCK_DTYPE)
        tcb = np.ascontiguousarray(tcb if tcb is not None else np.zeros(0, TCB_DTYPE), TCB_DTYPE)
        _check(_flows_sync(self._h, _ptr(udp) if len(udp) else None, len(udp),
                           _ptr(tcb) if len(tcb) else None, len(tcb)), "rxg_flows_sync")
        self.nu, self.nt = len(udp), len(tcb)

    def flows_add(self, udp: np.ndarray | None = None, tcb: np.ndarray | None = None):
        """add control blocks as the newest ones (rxg_flows_add); returns
        (udp_ids, tcp_ids, count_layout_moved)"""
        udp = np.ascontiguousarray(udp if udp is not None else np.zeros(0, UDP_SOCK_DTYPE),
                                   UDP_SOCK_DTYPE)
        tcb = np.ascontiguousarray(tcb if tcb is not None else np.zeros(0, TCB_DTYPE), TCB_DTYPE)
        uid = np.zeros(max(len(udp), 1), np.uint32)
        tid = np.zeros(max(len(tcb), 1), np.uint32)
        rc = _flows_add(self._h, _ptr(udp) if len(udp) else None, len(udp),
                        _ptr(tcb) if len(tcb) else None, len(tcb), _ptr(uid), _ptr(tid))
        if rc < 0:
            _check(rc, "rxg_flows_add")
        return uid[:len(udp)], tid[:len(tcb)], rc == 1

    def flows_remove(self, udp_ids=None, tcp_ids=None):
        u = np.ascontiguousarray(udp_ids if udp_ids is not None else [], np.uint32)
        t = np.ascontiguousarray(tcp_ids if tcp_ids is not None else [], np.uint32)
        _check(_flows_remove(self._h, _ptr(u) if len(u) else None, len(u),
                             _ptr(t) if len(t) else None, len(t)), "rxg_flows_remove")

    def flows_update_udp(self, fid: int, sock):
        a = np.ascontiguousarray(np.asarray(sock, UDP_SOCK_DTYPE).reshape(1))
        _check(_flows_update_udp(self._h, fid, _ptr(a)), "rxg_flows_update_udp")

    def flows_update_tcb(self, fid: int, tcb):
        a = np.ascontiguousarray(np.asarray(tcb, TCB_DTYPE).reshape(1))
        _check(_flows_update_tcb(self._h, fid, _ptr(a)), "rxg_flows_update_tcb")

    def flows_commit(self, stream=None):
        _check(_flows_commit(self._h, stream), "rxg_flows_commit")

    @property
    def num_udp_ids(self) -> int:
        return _num_udp_ids(self._h)

    @property
    def flows_rebuilds(self) -> int:
        return _flows_rebuilds(self._h)

    def tune(self, lanes_per_frame: int = 0, passes: int = 0, frames_per_group: int = 0,
             pipeline: int = 0xFFFFFFFF):
        """force a kernel variant (lanes_per_frame 0 = automatic); see KERNEL_VARIANTS"""
        _check(_tune(self._h, lanes_per_frame, passes, frames_per_group, pipeline), "rxg_tune")

    def kernel_variant(self, len_hint: int):
        """(kernel name as a trace shows it, [g, p, fpg, pipe]) of the classify
        dispatch a burst with this len_hint runs (rxg_kernel_variant)"""
        if _kernel_variant is None:
            return None, None
        v = np.zeros(4, np.uint32)
        buf = C.create_string_buffer(128)
        _check(_kernel_variant(self._h, len_hint, _ptr(v), buf, 128), "rxg_kernel_variant")
        return buf.value.decode(), [int(x) for x in v]

    def tune_grid(self, blocks_per_cu: int = 0):
        """cap resident blocks per CU (0 = occupancy)"""
        _check(_tune_grid(self._h, blocks_per_cu), "rxg_tune_grid")

    def tune_tx(self, variant: int = TX_AUTO, blocks_per_cu: int = 0):
        """force a TX checksum kernel variant (tx_cksum.hip k_tx index; TX_AUTO =
        by len_hint) and cap its resident blocks per CU (0 = its default)"""
        _check(_tune_tx(self._h, variant, blocks_per_cu), "rxg_tune_tx")

    def tune_flow_load(self, load_log2: int = 0):
        """exact-key flow tables at load <= 2**-load_log2 from the next
        flows_sync (0 = default); verdicts do not depend on it"""
        _check(_tune_flow_load(self._h, load_log2), "rxg_tune_flow_load")

    def tune_tables(self, flags: int = 0):
        """flow-table layout flags (TT_*) from the next flows_sync; verdicts do
        not depend on them"""
        _check(_tune_tables(self._h, flags), "rxg_tune_tables")

    @property
    def num_flows(self) -> int:
        return _num_flows(self._h)

    def lookup_udp(self, dip: int, dport: int) -> int:
        return _lk_udp(self._h, dip, dport)

    def lookup_tcp(self, sip: int, dip: int, sport: int, dport: int) -> int:
        return _lk_tcp(self._h, sip, dip, sport, dport)

    def classify(self, pkts: np.ndarray, off: np.ndarray, lens: np.ndarray,
                 off_unit_log2: int) -> np.ndarray:
        """Host buffers in, verdicts out (PCIe-inclusive, synchronous)."""
        pkts = np.ascontiguousarray(pkts, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        lens = np.ascontiguousarray(lens, np.uint16)
        out = np.zeros(len(off), VERDICT_DTYPE)
        _check(_classify(self._h, _ptr(pkts), _ptr(off), _ptr(lens), len(off), off_unit_log2,
                         _ptr(out)), "rxg_classify")
        return out

    def classify_span(self, pkts_ptr: int, span: int, off_ptr: int, len_ptr: int, n: int,
                      off_unit_log2: int, out_ptr: int):
        """raw-pointer host burst (pinned buffers from the caller), PCIe-inclusive"""
        _check(_classify_span(self._h, pkts_ptr, span, off_ptr, len_ptr, n, off_unit_log2,
                              out_ptr), "rxg_classify_span")

    def submit(self, pkts_ptr: int, span: int, off_ptr: int, len_ptr: int, n: int,
               off_unit_log2: int, out_ptr: int) -> int:
        """raw-pointer pipelined burst (pinned host buffers); returns the ticket"""
        t = _u64()
        _check(_submit(self._h, pkts_ptr, span, off_ptr, len_ptr, n, off_unit_log2, out_ptr,
                       C.byref(t)), "rxg_submit")
        return t.value

    def wait(self, ticket: int):
        _check(_wait(self._h, ticket), "rxg_wait")

    def classify_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, len_hint: int,
                     d_out, d_counts=None, stream=None, count_stream=None):
        """Device tensors in/out (torch tensors or raw ints), asynchronous on
        `stream`; with count_stream (a raw hipStream_t), d_counts is completed
        on that stream instead (rxg_classify_dev_cs)"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        if count_stream is None:
            _check(_classify_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2,
                                 len_hint, p(d_out), p(d_counts), stream), "rxg_classify_dev")
        else:
            _check(_classify_dev_cs(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2,
                                    len_hint, p(d_out), p(d_counts), stream, count_stream),
                   "rxg_classify_dev_cs")

    def classify_dev8(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, len_hint: int,
                      d_out, d_counts=None, stream=None, count_stream=None):
        """classify_dev writing 8-B verdicts (VERDICT8_DTYPE, rxg_classify_dev8)
        into d_out (n x 8 bytes)"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        if _classify_dev8 is None:
            raise RuntimeError(f"{LIB_PATH} has no rxg_classify_dev8 (an older build)")
        _check(_classify_dev8(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, len_hint,
                              p(d_out), p(d_counts), stream, count_stream), "rxg_classify_dev8")

    def udp_compact_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v, d_dgram,
                        d_first, d_payload, payload_cap: int, d_totals, stream=None):
        """K3: a classified burst's delivered datagrams grouped by socket and
        their payloads gathered (rxg_udp_compact_dev), async on stream"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_udp_compact_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, p(d_v),
                                p(d_dgram), p(d_first), p(d_payload), payload_cap, p(d_totals),
                                stream), "rxg_udp_compact_dev")

    def tcp_compact_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v, d_seg,
                        d_payload, payload_cap: int, d_totals, stream=None):
        """K4: a classified burst's rc-0 TCP segments sorted by tcb id and their
        PSH payloads gathered (rxg_tcp_compact_dev), async on stream"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tcp_compact_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, p(d_v),
                                p(d_seg), p(d_payload), payload_cap, p(d_totals), stream),
               "rxg_tcp_compact_dev")

    def tcp_coalesce_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v, window: int,
                         d_seg, d_run, d_payload, payload_cap: int, d_totals, stream=None):
        """K4 with receive coalescing: the sorted segments' in-sequence trains
        laid down as contiguous runs (rxg_tcp_coalesce_dev), async on stream"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tcp_coalesce_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, p(d_v),
                                 window, p(d_seg), p(d_run), p(d_payload), payload_cap,
                                 p(d_totals), stream), "rxg_tcp_coalesce_dev")

    def tcp_compact_ordered_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v,
                                window: int, d_seg, d_run, d_payload, payload_cap: int, d_totals,
                                stream=None):
        """K4 (window 0; d_payload None: records only) or its coalescing form on
        the sequence-ordered segments (rxg_tcp_compact_ordered_dev), async on
        stream; d_totals: 5 words, the last one the moved count"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tcp_compact_ordered_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2,
                                        p(d_v), window, p(d_seg), p(d_run), p(d_payload),
                                        payload_cap, p(d_totals), stream),
               "rxg_tcp_compact_ordered_dev")

    def delivery_moved(self, handle) -> int:
        """rxg_delivery_moved of a waited-for deliver_submit handle (0 with
        DLV_TCP_ORDER off)"""
        _, _, d = handle
        mv = _u32()
        _check(_delivery_moved(self._h, C.byref(d), C.byref(mv)), "rxg_delivery_moved")
        return mv.value

    def tcp_assemble_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v, d_seg,
                         d_stream, d_payload, payload_cap: int, d_totals, stream=None):
        """the sort, the ordering stage and the stream assembly
        (rxg_tcp_assemble_dev), async on stream; d_stream: room for n
        TCP_STREAM_DTYPE records; d_totals: 6 words {segments, payload bytes,
        overflow, streams, moved, sum of skip}"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tcp_assemble_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, p(d_v),
                                 p(d_seg), p(d_stream), p(d_payload), payload_cap, p(d_totals),
                                 stream), "rxg_tcp_assemble_dev")

    def delivery_streams(self, handle) -> np.ndarray:
        """rxg_delivery_streams of a waited-for deliver_submit handle: a copy of
        the burst's streams (empty with DLV_TCP_ASSEMBLE off)"""
        _, _, d = handle
        ptr, n = _vp(), _u32()
        _check(_delivery_streams(self._h, C.byref(d), C.byref(ptr), C.byref(n)),
               "rxg_delivery_streams")
        if not ptr.value or not n.value:
            return np.zeros(0, TCP_STREAM_DTYPE)
        return np.frombuffer((C.c_uint8 * (32 * n.value)).from_address(ptr.value),
                             np.uint8).copy().view(TCP_STREAM_DTYPE)

    def ddos_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, len_hint: int,
                 thresh: float, d_state, d_bits, d_flag, d_stat, d_summary, stream=None):
        """rxg_ddos_dev: one burst through the entropy flood detector, async on
        stream.  d_state (DDOS_STATE_DTYPE bytes) and d_summary
        (DDOS_SUMMARY_DTYPE bytes) are device buffers; d_bits (u32), d_flag
        (u8) and d_stat (f64) may each be None"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_ddos_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, len_hint, thresh,
                         p(d_state), p(d_bits), p(d_flag), p(d_stat), p(d_summary), stream),
               "rxg_ddos_dev")

    def ddos_bits_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, len_hint: int, d_bits,
                      stream=None):
        """rxg_ddos_bits_dev: the detector's bits pass alone"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_ddos_bits_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, len_hint,
                              p(d_bits), stream), "rxg_ddos_bits_dev")

    def ddos_window_dev(self, d_bits, d_len, n: int, thresh: float, d_state, d_flag, d_stat,
                        d_summary, stream=None):
        """rxg_ddos_window_dev: the window pass and state update on computed bits"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_ddos_window_dev(self._h, p(d_bits), p(d_len), n, thresh, p(d_state), p(d_flag),
                                p(d_stat), p(d_summary), stream), "rxg_ddos_window_dev")

    def tune_ddos(self, lanes_per_frame: int = 0, thresh: float | None = None):
        """rxg_tune_ddos: lanes per frame of the bits pass (one of DDOS_LANES,
        0 = auto); thresh, when given, is rxg_tune_ddos_thresh (DLV_DDOS)"""
        _check(_tune_ddos(self._h, lanes_per_frame), "rxg_tune_ddos")
        if thresh is not None:
            _check(_tune_ddos_thresh(self._h, thresh), "rxg_tune_ddos_thresh")

    def ddos_reset(self):
        """rxg_ddos_reset: the context's own detector state (DLV_DDOS) made fresh"""
        _check(_ddos_reset(self._h), "rxg_ddos_reset")

    def delivery_ddos(self, handle=None) -> np.ndarray:
        """rxg_delivery_ddos of a waited-for deliver_submit handle, or of the
        last process_mbufs_deliver: the burst's summary (DDOS_SUMMARY_DTYPE
        scalar; zeroed with DLV_DDOS off)"""
        d = handle[2] if handle is not None else self._last_delivery
        out = np.zeros(1, DDOS_SUMMARY_DTYPE)
        _check(_delivery_ddos(self._h, C.byref(d), _ptr(out)), "rxg_delivery_ddos")
        return out[0]

    def syncookie_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v, d_lmask,
                      id_space: int, params: np.ndarray, d_status, d_txd, d_totals, stream=None):
        """rxg_syncookie_dev: one burst through the SYN-cookie pass (K7), async
        on stream.  params: ck_params(); d_status (u8, n), d_txd (TXD_DTYPE
        bytes, room for n) and d_totals (u32, 4) are device buffers"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_syncookie_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, p(d_v),
                              p(d_lmask), id_space, _ptr(params), p(d_status), p(d_txd), p(d_totals),
                              stream), "rxg_syncookie_dev")

    def syncookie_set(self, params: np.ndarray, listener_ids):
        """rxg_syncookie_set: the parameters (ck_params()) and the listeners'
        TCP ids of the delivery bursts (DLV_SYNCOOKIE)"""
        ids = np.ascontiguousarray(listener_ids, np.uint32)
        _check(_syncookie_set(self._h, _ptr(params), _ptr(ids) if len(ids) else None, len(ids)),
               "rxg_syncookie_set")

    def syncookie_tick(self, t: int):
        """rxg_syncookie_tick: the time counter of the delivery bursts"""
        _check(_syncookie_tick(self._h, t & 0xFFFFFFFF), "rxg_syncookie_tick")

    def delivery_cookies(self, handle=None):
        """rxg_delivery_cookies of a waited-for deliver_submit handle (needs
        the burst's n: handle), or of the last process_mbufs_deliver: copies of
        (status u8[n], txd TXD_DTYPE[totals[0]], totals u32[4]); (None, None,
        zeros) with DLV_SYNCOOKIE off"""
        d = handle[2] if handle is not None else self._last_delivery
        n = len(handle[1]) if handle is not None else self._last_n
        st, tx, nt = _vp(), _vp(), _u32()
        tot = np.zeros(4, np.uint32)
        _check(_delivery_cookies(self._h, C.byref(d), C.byref(st), C.byref(tx), C.byref(nt),
                                 _ptr(tot)), "rxg_delivery_cookies")
        if not st.value:
            return None, None, tot
        status = np.frombuffer((C.c_uint8 * n).from_address(st.value), np.uint8).copy() if n \
            else np.zeros(0, np.uint8)
        txd = np.frombuffer((C.c_uint8 * (48 * nt.value)).from_address(tx.value),
                            np.uint8).copy().view(TXD_DTYPE) if nt.value else np.zeros(0, TXD_DTYPE)
        return status, txd, tot

    def l2_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, d_v, params: np.ndarray,
               d_status, d_out, cap_bytes: int, d_roff, d_rlen, d_rsrc, d_totals, stream=None):
        """rxg_l2_dev: one burst through the L2 responder (K8), async on
        stream.  params: l2_params(); d_status (u8, n), d_out (u8, cap_bytes,
        64-B aligned), d_roff / d_rsrc (u32, n), d_rlen (u16, n) and d_totals
        (u32, 6) are device buffers"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_l2_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, p(d_v), _ptr(params),
                       p(d_status), p(d_out), cap_bytes, p(d_roff), p(d_rlen), p(d_rsrc), p(d_totals),
                       stream), "rxg_l2_dev")

    def l2_set(self, params: np.ndarray, cap_bytes: int):
        """rxg_l2_set: the parameters (l2_params()) and the answers' room per
        burst of the delivery bursts (DLV_L2)"""
        _check(_l2_set(self._h, _ptr(params), cap_bytes), "rxg_l2_set")

    def delivery_l2(self, handle=None):
        """rxg_delivery_l2 of a waited-for deliver_submit handle (needs the
        burst's n: handle), or of the last process_mbufs_deliver: copies of
        (status u8[n], frames u8[64 * totals[5]], roff u32[k], rlen u16[k],
        rsrc u32[k], totals u32[6]), k = totals[4]; (None, None, None, None,
        None, zeros) with DLV_L2 off"""
        d = handle[2] if handle is not None else self._last_delivery
        n = len(handle[1]) if handle is not None else self._last_n
        st, fr, ro, rl, rs, na = _vp(), _vp(), _vp(), _vp(), _vp(), _u32()
        tot = np.zeros(6, np.uint32)
        _check(_delivery_l2(self._h, C.byref(d), C.byref(st), C.byref(fr), C.byref(ro), C.byref(rl),
                            C.byref(rs), C.byref(na), _ptr(tot)), "rxg_delivery_l2")
        if not st.value:
            return None, None, None, None, None, tot

        def take(ptr, nbytes, dt):
            if not nbytes:
                return np.zeros(0, dt)
            return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr.value), np.uint8).copy().view(dt)
        k = na.value
        return (take(st, n, np.uint8), take(fr, 64 * int(tot[5]), np.uint8), take(ro, 4 * k, np.uint32),
                take(rl, 2 * k, np.uint16), take(rs, 4 * k, np.uint32), tot)

    def tune_deliver(self, flags: int):
        """rxg_tune_deliver: DLV_TCP_IN_PLACE or DLV_TCP_GRO, either with
        DLV_TCP_ORDER; or DLV_TCP_ASSEMBLE (with or without DLV_TCP_ORDER); any
        of them with DLV_DDOS, DLV_SYNCOOKIE and DLV_L2 (0 = the default)"""
        _check(_tune_deliver(self._h, flags), "rxg_tune_deliver")

    def tune_gro(self, window: int):
        """rxg_tune_gro: the coalescing window in bytes (0 = GRO_DEFAULT_WINDOW)"""
        _check(_tune_gro(self._h, window), "rxg_tune_gro")

    def delivery_runs(self, handle) -> np.ndarray:
        """rxg_delivery_runs of a waited-for deliver_submit handle: a copy of the
        burst's runs (empty with DLV_TCP_GRO off)"""
        _, _, d = handle
        ptr, n = _vp(), _u32()
        _check(_delivery_runs(self._h, C.byref(d), C.byref(ptr), C.byref(n)), "rxg_delivery_runs")
        if not ptr.value or not n.value:
            return np.zeros(0, TCP_RUN_DTYPE)
        return np.frombuffer((C.c_uint8 * (16 * n.value)).from_address(ptr.value),
                             np.uint8).copy().view(TCP_RUN_DTYPE)

    def register_host(self, ptr: int, nbytes: int):
        """rxg_register_host: frames in [ptr, ptr + nbytes) are pulled by the
        device (keep the memory alive until unregister_host / close)"""
        _check(_register_host(self._h, ptr, nbytes), "rxg_register_host")

    def unregister_host(self, ptr: int):
        _check(_unregister_host(self._h, ptr), "rxg_unregister_host")

    def process_mbufs_deliver(self, mbufs):
        """rxg_process_mbufs_deliver over Mbuf structures: (verdicts, dgrams,
        first, udp payload, segments, tcp payload, phase ms) as numpy copies"""
        if not isinstance(mbufs, C.Array):
            mbufs = (C.POINTER(Mbuf) * len(mbufs))(*[C.pointer(m) for m in mbufs])
        arr = mbufs
        out = np.zeros(len(mbufs), VERDICT_DTYPE)
        d = Delivery()
        ms = (C.c_float * 8)()
        _check(_process_mbufs_deliver(self._h, C.cast(arr, _vp), len(mbufs), _ptr(out),
                                      C.byref(d), ms), "rxg_process_mbufs_deliver")
        self._last_delivery = d
        self._last_n = len(mbufs)
        return self._delivery_results(out, d, ms)

    def _delivery_results(self, out, d, ms):
        def grab(ptr, nbytes, dtype):
            if not ptr or nbytes == 0:
                return np.zeros(0, dtype)
            return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), np.uint8).copy().view(dtype)
        nf = _num_udp_ids(self._h)
        dg = grab(d.dgram, d.ndgram * 16, DGRAM_DTYPE)
        first = grab(d.first, (nf + 1) * 4, np.uint32) if d.first else None
        up = grab(d.udp_payload, d.udp_bytes, np.uint8)
        seg = grab(d.seg, d.nseg * 32, SEGMENT_DTYPE)
        tp = grab(d.tcp_payload, d.tcp_bytes, np.uint8)
        return out, dg, first, up, seg, tp, list(ms)

    def tune_ingest(self, mode: int):
        """rxg_tune_ingest: INGEST_AUTO / INGEST_PULL / INGEST_GATHER"""
        _check(_tune_ingest(self._h, mode), "rxg_tune_ingest")

    def deliver_submit(self, mbufs):
        """rxg_deliver_submit: a handle for deliver_wait (keeps the arrays alive)"""
        if not isinstance(mbufs, C.Array):
            mbufs = (C.POINTER(Mbuf) * len(mbufs))(*[C.pointer(m) for m in mbufs])
        out = np.zeros(len(mbufs), VERDICT_DTYPE)
        d = Delivery()
        _check(_deliver_submit(self._h, C.cast(mbufs, _vp), len(mbufs), _ptr(out), C.byref(d)),
               "rxg_deliver_submit")
        return (mbufs, out, d)

    def deliver_wait(self, handle):
        """rxg_deliver_wait: the results as process_mbufs_deliver returns them"""
        _, out, d = handle
        ms = (C.c_float * 8)()
        _check(_deliver_wait(self._h, C.byref(d), ms), "rxg_deliver_wait")
        return self._delivery_results(out, d, ms)

    def tx_cksum(self, pkts: np.ndarray, off: np.ndarray, lens: np.ndarray,
                 off_unit_log2: int) -> np.ndarray:
        """TX checksum fill of a host burst (PCIe round trip); returns the filled copy"""
        out = np.array(pkts, np.uint8, copy=True)
        off = np.ascontiguousarray(off, np.uint32)
        lens = np.ascontiguousarray(lens, np.uint16)
        span = max(((int(o) << off_unit_log2) + int(n) for o, n in zip(off, lens)), default=0)
        _check(_tx_cksum(self._h, _ptr(out), span, _ptr(off), _ptr(lens), len(off), off_unit_log2),
               "rxg_tx_cksum")
        return out

    def tx_cksum_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, len_hint: int,
                     stream=None):
        """in-place TX checksum fill of a device burst (torch tensors or raw ints)"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tx_cksum_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, len_hint,
                             stream), "rxg_tx_cksum_dev")

    def tune_txe(self, variant: int = TX_AUTO, blocks_per_cu: int = 0):
        """force a TX encode kernel variant (tx_encode.hip k_txe index; TX_AUTO =
        chosen from len_hint) and cap its resident blocks per CU (0 = default)"""
        _check(_tune_txe(self._h, variant, blocks_per_cu), "rxg_tune_txe")

    def tx_encode(self, txd: np.ndarray, payload: np.ndarray, cap_bytes: int, flags: int = 0):
        """frames of a host descriptor burst, packed (PCIe round trip):
        (pkts[:span], off, len, rc) with rc 0 or RXG_ERANGE (something was skipped)"""
        txd = np.ascontiguousarray(txd, TXD_DTYPE)
        payload = np.ascontiguousarray(payload, np.uint8)
        n = len(txd)
        pk = np.zeros(max(cap_bytes, 1), np.uint8)
        off, ln = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint16)
        span = _u64()
        rc = _tx_encode(self._h, _ptr(txd), n, _ptr(payload), len(payload), _ptr(pk), cap_bytes,
                        _ptr(off), _ptr(ln), flags, C.byref(span))
        if rc not in (0, -34):
            _check(rc, "rxg_tx_encode")
        return pk[:span.value], off[:n], ln[:n], rc

    def tx_encode_dev(self, d_txd, n: int, d_payload, d_pkts, cap_bytes: int, slot_bytes: int,
                      d_off, d_len, len_hint: int, flags: int, d_totals, stream=None):
        """frames of a device descriptor burst (torch tensors or raw ints), asynchronous"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tx_encode_dev(self._h, p(d_txd), n, p(d_payload), p(d_pkts), cap_bytes, slot_bytes,
                              p(d_off), p(d_len), len_hint, flags, p(d_totals), stream),
               "rxg_tx_encode_dev")

    def tx_encode_tso(self, txd: np.ndarray, payload: np.ndarray, mss: int, cap_bytes: int,
                      out_cap: int, flags: int = 0):
        """frames of a host descriptor burst with TCP payloads cut at mss, packed
        (PCIe round trip): (pkts[:span], off, len, first, nseg, rc); off / len
        hold out_cap entries (zero where nothing was written), rc is 0 or
        RXG_ERANGE (something was skipped)"""
        txd = np.ascontiguousarray(txd, TXD_DTYPE)
        payload = np.ascontiguousarray(payload, np.uint8)
        n = len(txd)
        pk = np.zeros(max(cap_bytes, 1), np.uint8)
        off, ln = np.zeros(max(out_cap, 1), np.uint32), np.zeros(max(out_cap, 1), np.uint16)
        first, nseg = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        span = _u64()
        rc = _tx_encode_tso(self._h, _ptr(txd), n, _ptr(payload), len(payload), mss, _ptr(pk),
                            cap_bytes, _ptr(off), _ptr(ln), out_cap, _ptr(first), _ptr(nseg), flags,
                            C.byref(span))
        if rc not in (0, -34):
            _check(rc, "rxg_tx_encode_tso")
        return pk[:span.value], off[:out_cap], ln[:out_cap], first[:n], nseg[:n], rc

    def tx_encode_tso_dev(self, d_txd, n: int, d_payload, mss: int, d_pkts, cap_bytes: int,
                          slot_bytes: int, d_off, d_len, out_cap: int, d_first, d_nseg,
                          len_hint: int, flags: int, d_totals, stream=None):
        """frames of a device descriptor burst with TCP payloads cut at mss (torch
        tensors or raw ints), asynchronous; d_totals has 8 words"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tx_encode_tso_dev(self._h, p(d_txd), n, p(d_payload), mss, p(d_pkts), cap_bytes,
                                  slot_bytes, p(d_off), p(d_len), out_cap, p(d_first), p(d_nseg),
                                  len_hint, flags, p(d_totals), stream), "rxg_tx_encode_tso_dev")

    def tx_encode_frag(self, txd: np.ndarray, payload: np.ndarray, mss: int, mtu: int,
                       cap_bytes: int, out_cap: int, flags: int = 0):
        """tx_encode_tso with UDP datagrams cut at the IPv4 MTU as well:
        (pkts[:span], off, len, first, nseg, rc)"""
        txd = np.ascontiguousarray(txd, TXD_DTYPE)
        payload = np.ascontiguousarray(payload, np.uint8)
        n = len(txd)
        pk = np.zeros(max(cap_bytes, 1), np.uint8)
        off, ln = np.zeros(max(out_cap, 1), np.uint32), np.zeros(max(out_cap, 1), np.uint16)
        first, nseg = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        span = _u64()
        rc = _tx_encode_frag(self._h, _ptr(txd), n, _ptr(payload), len(payload), mss, mtu, _ptr(pk),
                             cap_bytes, _ptr(off), _ptr(ln), out_cap, _ptr(first), _ptr(nseg), flags,
                             C.byref(span))
        if rc not in (0, -34):
            _check(rc, "rxg_tx_encode_frag")
        return pk[:span.value], off[:out_cap], ln[:out_cap], first[:n], nseg[:n], rc

    def tx_encode_frag_dev(self, d_txd, n: int, d_payload, mss: int, mtu: int, d_pkts,
                           cap_bytes: int, slot_bytes: int, d_off, d_len, out_cap: int, d_first,
                           d_nseg, len_hint: int, flags: int, d_totals, stream=None):
        """tx_encode_tso_dev with UDP datagrams cut at the IPv4 MTU as well (torch
        tensors or raw ints), asynchronous; d_totals has 8 words"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_tx_encode_frag_dev(self._h, p(d_txd), n, p(d_payload), mss, mtu, p(d_pkts), cap_bytes,
                                   slot_bytes, p(d_off), p(d_len), out_cap, p(d_first), p(d_nseg),
                                   len_hint, flags, p(d_totals), stream), "rxg_tx_encode_frag_dev")

    def process_mbufs(self, mbufs) -> np.ndarray:
        arr = (C.POINTER(Mbuf) * len(mbufs))(*[C.pointer(m) for m in mbufs])
        out = np.zeros(len(mbufs), VERDICT_DTYPE)
        _check(_process_mbufs(self._h, C.cast(arr, _vp), len(mbufs), _ptr(out)),
               "rxg_process_mbufs")
        return out

    def rss_split_dev(self, d_pkts, d_off, d_len, n: int, off_unit_log2: int, n_shards: int,
                      d_first, d_perm, stream=None):
        """RSS split of a device burst: d_first (n_shards + 1 u32) and d_perm (n u32)"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        _check(_rss_split_dev(self._h, p(d_pkts), p(d_off), p(d_len), n, off_unit_log2, n_shards,
                              p(d_first), p(d_perm), stream), "rxg_rss_split_dev")

    def gather_dev(self, d_pkts, d_off, d_len, off_unit_log2: int, d_idx, count: int, d_dst,
                   dst_cap: int, d_dst_off, d_dst_len, stream=None) -> int:
        """pack frames d_idx[0..count) into d_dst (64-B units); returns the bytes used"""
        def p(x):
            return x if (x is None or isinstance(x, int)) else x.data_ptr()
        span = _u64()
        _check(_gather_dev(self._h, p(d_pkts), p(d_off), p(d_len), off_unit_log2, p(d_idx), count,
                           p(d_dst), dst_cap, p(d_dst_off), p(d_dst_len), C.byref(span), stream),
               "rxg_gather_dev")
        return span.value

    def counts_allreduce(self, group: "Group"):
        """sum the context-owned counts over the group's ranks (synchronous)"""
        _check(_ctx_counts_allreduce(self._h, group._h), "rxg_ctx_counts_allreduce")

    def flow_counts(self) -> np.ndarray:
        n = self.num_flows
        out = np.zeros(max(n, 1), np.uint64)
        _check(_flow_counts(self._h, _ptr(out), n), "rxg_flow_counts")
        return out[:n]

    def counts_reset(self):
        _check(_counts_reset(self._h), "rxg_counts_reset")


class Pcap:
    """rxg_pcap: a capture file read burst by burst into the packed layout."""

    def __init__(self, path: str):
        h = _vp()
        _check(_pcap_open(C.byref(h), path.encode()), "rxg_pcap_open")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            _pcap_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rewind(self):
        _check(_pcap_rewind(self._h), "rxg_pcap_rewind")

    def read_burst_into(self, pkts: np.ndarray, off: np.ndarray, lens: np.ndarray,
                        off_unit_log2: int = 6):
        """fill caller arrays (e.g. pinned tensors' numpy views); returns (n, span)"""
        n, span = _u32(), _u64()
        _check(_pcap_read(self._h, _ptr(pkts), pkts.nbytes, _ptr(off), _ptr(lens), len(off),
                          off_unit_log2, C.byref(n), C.byref(span)), "rxg_pcap_read_burst")
        return n.value, span.value

    def read_burst(self, max_frames: int, cap_bytes: int, off_unit_log2: int = 6):
        pkts = np.zeros(cap_bytes, np.uint8)
        off = np.zeros(max_frames, np.uint32)
        lens = np.zeros(max_frames, np.uint16)
        n, span = self.read_burst_into(pkts, off, lens, off_unit_log2)
        return pkts[:span + 16], off[:n], lens[:n]


def pcap_write(path: str, pkts: np.ndarray, off: np.ndarray, lens: np.ndarray,
               off_unit_log2: int = 6):
    pkts = np.ascontiguousarray(pkts, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    _check(_pcap_write(path.encode(), _ptr(pkts), _ptr(off), _ptr(lens), len(off), off_unit_log2),
           "rxg_pcap_write")


def tx_encode_host(txd: np.ndarray, payload: np.ndarray, cap_bytes: int, slot_bytes: int = 0,
                   flags: int = 0, fill: int = 0):
    """rxg_tx_encode_host, the TX encoder on the CPU (no context, no device):
    (pkts, off, len, span, totals, rc); pkts is the whole cap_bytes buffer,
    prefilled with `fill`, so a caller can see what was left untouched; rc is 0
    or RXG_ERANGE (something was skipped), anything else raises"""
    txd = np.ascontiguousarray(txd, TXD_DTYPE)
    payload = np.ascontiguousarray(payload, np.uint8)
    n = len(txd)
    pk = np.full(cap_bytes, fill, np.uint8)
    off, ln = np.zeros(n, np.uint32), np.zeros(n, np.uint16)
    span, tot = _u64(), np.zeros(4, np.uint32)
    rc = _tx_encode_host(txd.ctypes.data, n, payload.ctypes.data if len(payload) else None,
                         len(payload), pk.ctypes.data, cap_bytes, slot_bytes, off.ctypes.data,
                         ln.ctypes.data, flags, C.byref(span), tot.ctypes.data)
    if rc not in (0, -34):
        _check(rc, "rxg_tx_encode_host")
    return pk, off, ln, span.value, tot, rc


def tx_tso_count(txd: np.ndarray, mss: int):
    """rxg_tx_tso_count: (entries, packed_bytes) a burst needs at this mss"""
    txd = np.ascontiguousarray(txd, TXD_DTYPE)
    e, b = _u64(), _u64()
    _check(_tx_tso_count(txd.ctypes.data if len(txd) else None, len(txd), mss, C.byref(e),
                         C.byref(b)), "rxg_tx_tso_count")
    return e.value, b.value


def tx_frag_count(txd: np.ndarray, mss: int, mtu: int):
    """rxg_tx_frag_count: (entries, packed_bytes) a burst needs at this mss and mtu"""
    txd = np.ascontiguousarray(txd, TXD_DTYPE)
    e, b = _u64(), _u64()
    _check(_tx_frag_count(txd.ctypes.data if len(txd) else None, len(txd), mss, mtu, C.byref(e),
                          C.byref(b)), "rxg_tx_frag_count")
    return e.value, b.value


def tcp_runs_host(seg: np.ndarray, sip: np.ndarray, window: int) -> np.ndarray:
    """rxg_tcp_runs_host: the runs of receive coalescing over K4's records (seg,
    SEGMENT_DTYPE) and their raw source addresses, on the CPU"""
    seg = np.ascontiguousarray(seg, SEGMENT_DTYPE)
    sip = np.ascontiguousarray(sip, np.uint32)
    assert len(seg) == len(sip)
    run = np.zeros(max(len(seg), 1), TCP_RUN_DTYPE)
    nrun = _u32()
    _check(_tcp_runs_host(seg.ctypes.data if len(seg) else None, sip.ctypes.data if len(seg) else None,
                          len(seg), window, run.ctypes.data, C.byref(nrun)), "rxg_tcp_runs_host")
    return run[:nrun.value].copy()


def ck_params(key: bytes, t: int, max_age: int = CK_DEFAULT_MAX_AGE, window: int = 14600) -> np.ndarray:
    """rxg_ck_params (one element) from the 16 key bytes"""
    assert len(key) == 16
    p = np.zeros(1, CK_PARAMS_DTYPE)
    p["k0"], p["k1"] = int.from_bytes(key[:8], "little"), int.from_bytes(key[8:], "little")
    p["t"], p["max_age"], p["window"] = t & 0xFFFFFFFF, max_age, window
    return p


def l2_params(local) -> np.ndarray:
    """rxg_l2_params (one element) from (ip, mac) pairs: ip dotted or raw,
    mac six bytes"""
    p = np.zeros(1, L2_PARAMS_DTYPE)
    p["nlocal"] = len(local)
    for j, (ip, mac) in enumerate(local[:L2_MAX_LOCAL]):
        p["local"][0, j]["ip"] = ip_raw(ip) if isinstance(ip, str) else ip
        p["local"][0, j]["mac"] = np.frombuffer(bytes(mac), np.uint8)
    return p


def l2_host(pkts: np.ndarray, off: np.ndarray, lens: np.ndarray, off_unit_log2: int,
            verdicts: np.ndarray, params: np.ndarray, cap_bytes: int, pad: int = 0, canary: int = 0):
    """rxg_l2_host: one burst through the L2 responder on the CPU: (status,
    frames, roff, rlen, rsrc, totals), the arrays cut to what was written.  With
    pad, they are returned whole: n + pad entries each and cap_bytes + 64 * pad
    bytes of frames, pre-filled with canary"""
    n = len(lens)
    pkts = np.ascontiguousarray(pkts, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    v = np.ascontiguousarray(verdicts, VERDICT_DTYPE)
    status = np.full(n + pad, canary, np.uint8)
    out = np.full(cap_bytes + 64 * pad + 64, canary, np.uint8)
    out = out[(-out.ctypes.data) % 64:][:cap_bytes + 64 * pad]
    roff = np.full(n + pad, canary * 0x01010101, np.uint32)
    rlen = np.full(n + pad, canary * 0x0101, np.uint16)
    rsrc = np.full(n + pad, canary * 0x01010101, np.uint32)
    tot = np.zeros(6, np.uint32)
    _check(_l2_host(pkts.ctypes.data if n else None, off.ctypes.data, lens.ctypes.data, n, off_unit_log2,
                    v.ctypes.data, _ptr(params), status.ctypes.data, out.ctypes.data, cap_bytes,
                    roff.ctypes.data, rlen.ctypes.data, rsrc.ctypes.data, tot.ctypes.data), "rxg_l2_host")
    if pad:
        return status, out, roff, rlen, rsrc, tot
    k = int(tot[4])
    return status, out[:64 * int(tot[5])].copy(), roff[:k].copy(), rlen[:k].copy(), rsrc[:k].copy(), tot


def siphash24(key: bytes, msg: bytes) -> int:
    """rxg_siphash24: SipHash-2-4 of msg under the 16 key bytes"""
    m = np.frombuffer(msg, np.uint8) if msg else np.zeros(1, np.uint8)
    return _siphash24(int.from_bytes(key[:8], "little"), int.from_bytes(key[8:], "little"),
                      m.ctypes.data, len(msg))


def syncookie_value(key: bytes, sip: int, dip: int, sport: int, dport: int, isn: int, t: int) -> int:
    """rxg_syncookie_value (sip, dip, sport, dport raw, as loaded from the frame)"""
    return _syncookie_value(int.from_bytes(key[:8], "little"), int.from_bytes(key[8:], "little"), sip,
                            dip, sport, dport, isn & 0xFFFFFFFF, t & 0xFFFFFFFF)


def syncookie_host(pkts: np.ndarray, off: np.ndarray, lens: np.ndarray, off_unit_log2: int,
                   verdicts: np.ndarray, lmask: np.ndarray, id_space: int, params: np.ndarray,
                   pad: int = 0, canary: int = 0):
    """rxg_syncookie_host: one burst through the SYN-cookie pass on the CPU:
    (status, txd, totals).  With pad, the two arrays are returned whole: n +
    pad status bytes and n + pad descriptors, pre-filled with canary"""
    n = len(lens)
    pkts = np.ascontiguousarray(pkts, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    v = np.ascontiguousarray(verdicts, VERDICT_DTYPE)
    lm = np.ascontiguousarray(lmask, np.uint32)
    status = np.full(n + pad, canary, np.uint8)
    txd = np.full((n + pad) * 48, canary, np.uint8)
    tot = np.zeros(4, np.uint32)
    _check(_syncookie_host(pkts.ctypes.data, off.ctypes.data, lens.ctypes.data, n, off_unit_log2,
                           v.ctypes.data, lm.ctypes.data if lm.size else None, id_space, _ptr(params),
                           status.ctypes.data, txd.ctypes.data, tot.ctypes.data), "rxg_syncookie_host")
    if pad:
        return status, txd, tot
    return status, txd.view(TXD_DTYPE)[:tot[0]].copy(), tot


def ddos_entropy(set_bits: float, total_bits: float) -> float:
    """rxg_ddos_entropy: e(s, t) as the reference writes it, in double"""
    return _ddos_entropy(float(set_bits), float(total_bits))


def ddos_host(pkts: np.ndarray, off: np.ndarray, lens: np.ndarray, off_unit_log2: int,
              thresh: float = DDOS_DEFAULT_THRESH, state: np.ndarray | None = None,
              want=("bits", "flag", "stat")):
    """rxg_ddos_host: one burst through the entropy flood detector on the CPU.
    state (DDOS_STATE_DTYPE, one element; fresh when None) is updated in
    place.  Returns (bits, flag, stat, summary, state); an output not named
    in `want` is passed as NULL and returned as None"""
    n = len(lens)
    if state is None:
        state = np.zeros(1, DDOS_STATE_DTYPE)
    assert state.dtype == DDOS_STATE_DTYPE and state.size == 1 and state.flags["C_CONTIGUOUS"]
    pkts = np.ascontiguousarray(pkts, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    bits = np.full(n, 0, np.uint32) if "bits" in want else None
    flag = np.zeros(n, np.uint8) if "flag" in want else None
    stat = np.zeros(n, np.float64) if "stat" in want else None
    summ = np.zeros(1, DDOS_SUMMARY_DTYPE)
    _check(_ddos_host(pkts.ctypes.data, off.ctypes.data, lens.ctypes.data, n, off_unit_log2, thresh,
                      state.ctypes.data, _ptr(bits), _ptr(flag), _ptr(stat), summ.ctypes.data),
           "rxg_ddos_host")
    return bits, flag, stat, summ[0], state


def tcp_order_host(seg: np.ndarray, sip: np.ndarray):
    """rxg_tcp_order_host: the sequence ordering of K4's records (seg,
    SEGMENT_DTYPE) and their raw source addresses, on the CPU: (perm, moved),
    perm[k] = the index of the record that takes position k"""
    seg = np.ascontiguousarray(seg, SEGMENT_DTYPE)
    sip = np.ascontiguousarray(sip, np.uint32)
    assert len(seg) == len(sip)
    if not len(seg): # (the call takes no NULL, and numpy's empty arrays may have one)
        seg, sip = np.zeros(1, SEGMENT_DTYPE), np.zeros(1, np.uint32)
        n = 0
    else:
        n = len(seg)
    perm = np.zeros(max(n, 1), np.uint32)
    moved = _u32()
    _check(_tcp_order_host(seg.ctypes.data, sip.ctypes.data, n, perm.ctypes.data, C.byref(moved)),
           "rxg_tcp_order_host")
    return perm[:n].copy(), moved.value


def tcp_assemble_host(seg: np.ndarray, sip: np.ndarray, avail: np.ndarray):
    """rxg_tcp_assemble_host: the stream assembly of ordered records (seg,
    SEGMENT_DTYPE), their raw source addresses and captured payload bytes, on
    the CPU: (streams, skip, take, dst)"""
    seg = np.ascontiguousarray(seg, SEGMENT_DTYPE)
    sip = np.ascontiguousarray(sip, np.uint32)
    avail = np.ascontiguousarray(avail, np.uint32)
    assert len(seg) == len(sip) == len(avail)
    n = len(seg)
    if not n: # (the call takes no NULL, and numpy's empty arrays may have one)
        seg, sip, avail = np.zeros(1, SEGMENT_DTYPE), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    st = np.zeros(max(n, 1), TCP_STREAM_DTYPE)
    skip, take, dst = (np.zeros(max(n, 1), np.uint32) for _ in range(3))
    nst = _u32()
    _check(_tcp_assemble_host(seg.ctypes.data, sip.ctypes.data, avail.ctypes.data, n, st.ctypes.data,
                              C.byref(nst), skip.ctypes.data, take.ctypes.data, dst.ctypes.data),
           "rxg_tcp_assemble_host")
    return st[:nst.value].copy(), skip[:n].copy(), take[:n].copy(), dst[:n].copy()


def tx_encode_tso_host(txd: np.ndarray, payload: np.ndarray, mss: int, cap_bytes: int, out_cap: int,
                       slot_bytes: int = 0, flags: int = 0, fill: int = 0, fill_entries: int = 0):
    """rxg_tx_encode_tso_host, the TX encoder with TCP segmentation on the CPU:
    (pkts, off, len, first, nseg, span, totals, rc); pkts is the whole
    cap_bytes buffer prefilled with `fill`, off / len hold out_cap entries
    prefilled with `fill_entries` (all bits), so a caller can see what was left
    untouched; rc is 0 or RXG_ERANGE, anything else raises"""
    txd = np.ascontiguousarray(txd, TXD_DTYPE)
    payload = np.ascontiguousarray(payload, np.uint8)
    n = len(txd)
    pk = np.full(cap_bytes, fill, np.uint8)
    off = np.full(max(out_cap, 1), fill_entries & 0xFFFFFFFF, np.uint32)
    ln = np.full(max(out_cap, 1), fill_entries & 0xFFFF, np.uint16)
    first, nseg = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    span, tot = _u64(), np.zeros(8, np.uint32)
    rc = _tx_encode_tso_host(txd.ctypes.data, n, payload.ctypes.data if len(payload) else None,
                             len(payload), mss, pk.ctypes.data, cap_bytes, slot_bytes, off.ctypes.data,
                             ln.ctypes.data, out_cap, first.ctypes.data, nseg.ctypes.data, flags,
                             C.byref(span), tot.ctypes.data)
    if rc not in (0, -34):
        _check(rc, "rxg_tx_encode_tso_host")
    return pk, off[:out_cap], ln[:out_cap], first[:n], nseg[:n], span.value, tot, rc


def tx_encode_frag_host(txd: np.ndarray, payload: np.ndarray, mss: int, mtu: int, cap_bytes: int,
                        out_cap: int, slot_bytes: int = 0, flags: int = 0, fill: int = 0,
                        fill_entries: int = 0):
    """rxg_tx_encode_frag_host, tx_encode_tso_host with UDP datagrams cut at the
    IPv4 MTU as well: (pkts, off, len, first, nseg, span, totals, rc)"""
    txd = np.ascontiguousarray(txd, TXD_DTYPE)
    payload = np.ascontiguousarray(payload, np.uint8)
    n = len(txd)
    pk = np.full(cap_bytes, fill, np.uint8)
    off = np.full(max(out_cap, 1), fill_entries & 0xFFFFFFFF, np.uint32)
    ln = np.full(max(out_cap, 1), fill_entries & 0xFFFF, np.uint16)
    first, nseg = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    span, tot = _u64(), np.zeros(8, np.uint32)
    rc = _tx_encode_frag_host(txd.ctypes.data, n, payload.ctypes.data if len(payload) else None,
                              len(payload), mss, mtu, pk.ctypes.data, cap_bytes, slot_bytes,
                              off.ctypes.data, ln.ctypes.data, out_cap, first.ctypes.data,
                              nseg.ctypes.data, flags, C.byref(span), tot.ctypes.data)
    if rc not in (0, -34):
        _check(rc, "rxg_tx_encode_frag_host")
    return pk, off[:out_cap], ln[:out_cap], first[:n], nseg[:n], span.value, tot, rc


def rss_hash(sip: int, dip: int, sport: int, dport: int) -> int:
    return _rss(sip, dip, sport, dport)


def rss_split(pkts: np.ndarray, off: np.ndarray, lens: np.ndarray, off_unit_log2: int,
              n_shards: int):
    """host RSS split (rxg_rss_split): (first[n_shards + 1], perm[n])"""
    pkts = np.ascontiguousarray(pkts, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint16)
    first = np.zeros(n_shards + 1, np.uint32)
    perm = np.zeros(max(len(off), 1), np.uint32)
    _check(_rss_split(_ptr(pkts), _ptr(off), _ptr(lens), len(off), off_unit_log2, n_shards,
                      _ptr(first), _ptr(perm)), "rxg_rss_split")
    return first, perm[:len(off)]


def group_id() -> bytes:
    """rank 0: a fresh communicator id to hand to every rank (rxg_group_id)"""
    b = (C.c_uint8 * GROUP_ID_BYTES)()
    _check(_group_id(b), "rxg_group_id")
    return bytes(b)


class Group:
    """rxg_group: the node's GPUs as one RCCL communicator (one rank per process)"""

    def __init__(self, device: int, nranks: int, rank: int, gid: bytes):
        assert len(gid) == GROUP_ID_BYTES
        h = _vp()
        buf = (C.c_uint8 * GROUP_ID_BYTES)(*gid)
        _check(_group_open(C.byref(h), device, nranks, rank, buf), "rxg_group_open")
        self._h = h

    def size(self):
        """rxg_group_size: (nranks, rank) as the RCCL communicator reports them"""
        nr, rk = C.c_uint32(), C.c_uint32()
        _check(_group_size(self._h, C.byref(nr), C.byref(rk)), "rxg_group_size")
        return nr.value, rk.value

    def allreduce(self, d_counts, n: int, stream=None):
        """in-place sum of a device u64[n] vector over the ranks, async on stream"""
        p = d_counts if isinstance(d_counts, int) else d_counts.data_ptr()
        _check(_counts_allreduce(self._h, p, n, stream), "rxg_counts_allreduce")

    def close(self):
        if getattr(self, "_h", None):
            _group_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_gen_cfg(**kw) -> GenCfg:
    d = dict(seed=0x5EED0001, size_mode=0, frame_len=64, slot_bytes=64, proto_mode=0, n_udp=1024,
             n_tcp=0, local_ip=ip_raw("192.168.100.77"), udp_base_port=20000, tcp_port=9999,
             bad_cksum_per10k=100, unknown_per10k=50, other_per10k=50, shard=0, n_shards=1,
             packed=0, src_ip=0, src_port=0)
    d.update(kw)
    return GenCfg(**d)


def gen_flows(cfg: GenCfg):
    udp = np.zeros(cfg.n_udp, UDP_SOCK_DTYPE)
    tcb = np.zeros(cfg.n_tcp + 1 if cfg.n_tcp else 0, TCB_DTYPE)
    _check(_gen_flows(C.byref(cfg), _ptr(udp) if len(udp) else None,
                      _ptr(tcb) if len(tcb) else None), "rxg_gen_flows")
    return udp, tcb


def gen_host(cfg: GenCfg, first: int, n: int, off_unit_log2: int = 6):
    pkts = np.zeros(n * cfg.slot_bytes, np.uint8)
    off = np.zeros(n, np.uint32)
    lens = np.zeros(n, np.uint16)
    _check(_gen_host(C.byref(cfg), first, n, _ptr(pkts), _ptr(off), _ptr(lens), off_unit_log2),
           "rxg_gen_host")
    return pkts, off, lens


def gen_dev(cfg: GenCfg, first: int, n: int, d_pkts, d_off, d_len, off_unit_log2: int = 6,
            stream=None):
    _check(_gen_dev(C.byref(cfg), first, n, _tptr(d_pkts), _tptr(d_off), _tptr(d_len),
                    off_unit_log2, stream), "rxg_gen_dev")


# ---- libnstack: the socket layer (include/nstack.h) ------------------------
AF_INET, SOCK_STREAM, SOCK_DGRAM, MSG_DONTWAIT = 2, 1, 2, 0x40


class SockaddrIn(C.Structure):
    _fields_ = [("sin_family", C.c_uint16), ("sin_port", C.c_uint16), ("sin_addr", C.c_uint32),
                ("sin_zero", C.c_uint8 * 8)]


def sockaddr(ip: str, port: int) -> SockaddrIn:
    return SockaddrIn(AF_INET, port_raw(port), ip_raw(ip))


def ft_dump(h, which: int, device: bool):
    """rxg_ft_dump of context handle h: (uint32 array of the table, info[8]);
    which 3 / 4: the compact UDP table / the port window (include/rxgpu.h)"""
    info = np.zeros(8, np.uint32)
    _check(_ft_dump(h, which, int(device), None, 0, _ptr(info)), "rxg_ft_dump")  # sizes
    words = {0: int(info[7]) * 4, 1: int(info[7]) * 4, 2: 65536, 3: int(info[7]) * 2,
             4: (int(info[7]) + 1) // 2}[which]
    buf = np.zeros(words, np.uint32)
    _check(_ft_dump(h, which, int(device), _ptr(buf), buf.nbytes, _ptr(info)), "rxg_ft_dump")
    return buf, info


class NStack:
    """Process-wide socket layer (one per process, like the reference's globals)."""
    _lib = None

    def __init__(self, device: int = HOST_ONLY, max_burst: int = 4096, max_bytes: int = 1 << 24):
        if NStack._lib is None:
            if not os.path.exists(NSTACK_PATH):
                raise ImportError(f"{NSTACK_PATH} missing: run make -C {_HERE}")
            lib = C.CDLL(NSTACK_PATH)
            ssz = C.c_ssize_t
            sig = [("nstack_init", _i32, [_i32, _u32, _u64]), ("nstack_fini", None, []),
                   ("nsocket", _i32, [_i32, _i32, _i32]), ("nbind", _i32, [_i32, _vp, _u32]),
                   ("nlisten", _i32, [_i32, _i32]), ("naccept", _i32, [_i32, _vp, _vp]),
                   ("nsend", ssz, [_i32, _vp, C.c_size_t, _i32]),
                   ("nrecv", ssz, [_i32, _vp, C.c_size_t, _i32]),
                   ("nrecvfrom", ssz, [_i32, _vp, C.c_size_t, _i32, _vp, _vp]),
                   ("nsendto", ssz, [_i32, _vp, C.c_size_t, _i32, _vp, _u32]),
                   ("nclose", _i32, [_i32]),
                   ("nstack_rx_burst", _i32, [_vp, _u32, _vp, _vp]),
                   ("nstack_rx_submit", _i32, [_vp, _u32, _vp, _vp]),
                   ("nstack_rx_complete", _i32, []),
                   ("nstack_rx_pending", _i32, []),
                   ("nstack_deliver", _i32, [_vp, _u32, _vp, _u64, _vp]),
                   ("nstack_tcb_add", _i32, [_u32, _u32, _u16, _u16, _i32]),
                   ("nstack_flows", _i32, [_vp, _u32, _vp, _vp, _u32, _vp, _vp]),
                   ("nstack_flow_ids", _i32, [_vp, _u32, _vp, _u32]),
                   ("nstack_drain_all", C.c_int64, [_vp, C.c_size_t, _vp]),
                   ("nstack_drain_all_sum", C.c_int64, [_vp, C.c_size_t, _vp, _vp]),
                   ("nstack_set_rx_inplace", _i32, [_i32, _vp, _vp]),
                   ("nstack_mbufs_put", None, [_vp, _u32]),
                   ("nstack_reclaim", None, []),
                   ("nstack_last_burst_phases", _i32, [_vp]),
                   ("nstack_tcb_state", _i32, [_u32, _u32, _u16, _u16, _vp, _vp, _vp, _vp]),
                   ("nstack_tcb_sndq", _i32, [_u32, _u32, _u16, _u16, _u32, _vp, _vp]),
                   ("nstack_tcb_count", _u32, []),
                   ("nstack_lookup_udp", _u32, [_u32, _u16]),
                   ("nstack_lookup_tcp", _u32, [_u32, _u32, _u16, _u16]),
                   ("nstack_ctx", _vp, []),
                   ("nstack_register_host", _i32, [_vp, _u64]),
                   ("nstack_set_halves", _i32, [_u32]),
                   ("nstack_stat", _u64, [_i32]),
                   ("nstack_set_local", _i32, [_u32, _vp]),
                   ("nstack_arp_insert", _i32, [_u32, _vp]),
                   ("nstack_tx_burst", _i32, [_vp, _u64, _vp, _vp, _u32, _i32, _vp]),
                   ("nstack_set_tx_encode", _i32, [_i32]),
                   ("nstack_set_tx_mss", _i32, [_u32]),
                   ("nstack_set_tx_mtu", _i32, [_u32]),
                   ("nstack_set_rx_gro", _i32, [_u32]),
                   ("nstack_set_rx_order", _i32, [_i32]),
                   ("nstack_set_rx_assemble", _i32, [_i32]),
                   ("nstack_set_rx_ddos", _i32, [_i32, C.c_double]),
                   ("nstack_ddos_status", _i32, [_vp]),
                   ("nstack_set_syncookies", _i32, [_i32, _vp]),
                   ("nstack_syncookie_tick", _i32, [_u32]),
                   ("nstack_syncookie_stats", _i32, [_vp]),
                   ("nstack_set_l2_respond", _i32, [_i32])]
            for name, res, args in sig:
                f = getattr(lib, name)
                f.restype, f.argtypes = res, args
            NStack._lib = lib
        self.lib = NStack._lib
        _check(self.lib.nstack_init(device, max_burst, max_bytes), "nstack_init")

    def fini(self):
        self.lib.nstack_fini()
        self._held = []  # (in place: the stack let go of every frame)
        self._inplace = False

    # socket calls: thin pass-through with the reference's argument meaning
    def socket(self, type_):
        return self.lib.nsocket(AF_INET, type_, 0)

    def bind(self, fd, ip, port):
        a = sockaddr(ip, port)
        return self.lib.nbind(fd, C.byref(a), C.sizeof(a))

    def listen(self, fd):
        return self.lib.nlisten(fd, 10)

    def accept(self, fd):
        a = SockaddrIn()
        n = C.c_uint32(C.sizeof(a))
        r = self.lib.naccept(fd, C.byref(a), C.byref(n))
        return r, a

    def recvfrom(self, fd, n, flags=MSG_DONTWAIT):
        buf = C.create_string_buffer(max(n, 1))
        a = SockaddrIn()
        al = C.c_uint32(C.sizeof(a))
        r = self.lib.nrecvfrom(fd, buf, n, flags, C.byref(a), C.byref(al))
        return r, buf.raw[:max(r, 0)], a

    def recv(self, fd, n, flags=MSG_DONTWAIT, full=False):
        """(return value, bytes); full=True: the whole n-byte buffer (a split
        read returns the remaining length, common.c:493, after copying n bytes)"""
        buf = C.create_string_buffer(max(n, 1))
        r = self.lib.nrecv(fd, buf, n, flags)
        return r, (buf.raw[:n] if full else buf.raw[:max(r, 0)])

    def sendto(self, fd, data: bytes, ip, port):
        a = sockaddr(ip, port)
        return self.lib.nsendto(fd, data, len(data), 0, C.byref(a), C.sizeof(a))

    def send(self, fd, data: bytes):
        return self.lib.nsend(fd, data, len(data), 0)

    def close(self, fd):
        return self.lib.nclose(fd)

    def tcb_add(self, sip, dip, sport, dport, status=TCP_STATUS_ESTABLISHED):
        return self.lib.nstack_tcb_add(ip_raw(sip), ip_raw(dip), port_raw(sport),
                                       port_raw(dport), status)

    def flow_ids(self):
        """(udp_ids, tcp_ids): the stable flow id of each block of flows()"""
        u, t = self.flows()
        uid = np.zeros(max(len(u), 1), np.uint32)
        tid = np.zeros(max(len(t), 1), np.uint32)
        _check(self.lib.nstack_flow_ids(_ptr(uid), len(u), _ptr(tid), len(t)), "nstack_flow_ids")
        return uid[:len(u)], tid[:len(t)]

    def to_ids(self, v: np.ndarray) -> np.ndarray:
        """verdicts made against flows()'s arrays (creation-order indices, e.g. by
        the oracle) with their flow ids turned into the blocks' stable ids"""
        uid, tid = self.flow_ids()
        v = np.array(v, VERDICT_DTYPE, copy=True)
        for cls, ids in ((CLS_UDP, uid), (CLS_TCP, tid)):
            m = (v["cls"] == cls) & (v["flow_id"] != FLOW_NONE)
            v["flow_id"][m] = ids[v["flow_id"][m]]
        return v

    def lookup_udp(self, dip: int, dport: int) -> int:
        """the flow id the library's tables give a UDP key (raw network order)"""
        return self.lib.nstack_lookup_udp(dip, dport)

    def lookup_tcp(self, sip: int, dip: int, sport: int, dport: int) -> int:
        """the flow id the library's tables give a TCP 4-tuple (raw), listener included"""
        return self.lib.nstack_lookup_tcp(sip, dip, sport, dport)

    def tune_ingest(self, mode: int):
        """rxg_tune_ingest on the stack's context (INGEST_AUTO / _PULL / _GATHER)"""
        _check(_tune_ingest(self.lib.nstack_ctx(), mode), "rxg_tune_ingest")

    def set_halves(self, min_half: int):
        """nstack_set_halves: bursts of >= 2 * min_half frames as two halves in flight (0 = off)"""
        _check(self.lib.nstack_set_halves(min_half), "nstack_set_halves")

    def register_host(self, ptr: int, nbytes: int):
        """nstack_register_host: frames in this memory are pulled by the GPU"""
        _check(self.lib.nstack_register_host(ptr, nbytes), "nstack_register_host")

    def ft_dump(self, which: int, device: bool):
        """diagnostics: (table, info) of the socket layer's context (rxg_ft_dump)"""
        return ft_dump(self.lib.nstack_ctx(), which, device)

    def flows(self, with_gen: bool = False):
        """the lists in creation order (and, with_gen, their generation for deliver)"""
        nu, nt, gen = C.c_uint32(), C.c_uint32(), _u64()
        _check(self.lib.nstack_flows(None, 0, C.byref(nu), None, 0, C.byref(nt), None),
               "nstack_flows")
        u = np.zeros(nu.value, UDP_SOCK_DTYPE)
        t = np.zeros(nt.value, TCB_DTYPE)
        _check(self.lib.nstack_flows(_ptr(u) if len(u) else None, len(u), None,
                                     _ptr(t) if len(t) else None, len(t), None, C.byref(gen)),
               "nstack_flows")
        return (u, t, gen.value) if with_gen else (u, t)

    def tcb_state(self, sip, dip, sport, dport):
        """(status, rcv_nxt, snd_nxt, fd) of the tcb with this raw 4-tuple, or None"""
        st, rn, sn, fd = C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        if self.lib.nstack_tcb_state(sip, dip, sport, dport, C.byref(st), C.byref(rn),
                                     C.byref(sn), C.byref(fd)):
            return None
        return st.value, rn.value, sn.value, fd.value

    def tcb_sndq(self, sip, dip, sport, dport):
        """[(tcp_flags, acknum)] queued in the tcb's send ring, oldest first"""
        out, k = [], 0
        fl, ack = C.c_uint8(), C.c_uint32()
        while self.lib.nstack_tcb_sndq(sip, dip, sport, dport, k, C.byref(fl), C.byref(ack)) == 0:
            out.append((fl.value, ack.value))
            k += 1
        return out

    def tcb_count(self):
        return self.lib.nstack_tcb_count()

    PHASES = ("gather", "h2d", "classify", "compact", "d2h", "lib_call", "udp_deliver",
              "tcp_deliver", "frame_loop", "rx_burst", "segments", "datagrams")

    def last_burst_phases(self) -> dict:
        """where the last rx_burst's time went (nstack_last_burst_phases, ms)"""
        ms = (C.c_float * 12)()
        _check(self.lib.nstack_last_burst_phases(ms), "nstack_last_burst_phases")
        return dict(zip(self.PHASES, [float(x) for x in ms]))

    @staticmethod
    def mbufs(frames: list[bytes]):
        """rte_mbuf-shaped descriptors over the given frames (kept alive by the return)"""
        bufs = [C.create_string_buffer(f, len(f) + 16) for f in frames]
        ms = [Mbuf() for _ in frames]
        for m, b, f in zip(ms, bufs, frames):
            m.buf_addr = C.cast(b, C.c_void_p)
            m.data_off = 0
            m.data_len = len(f)
            m.refcnt = 1  # the caller's reference (rte_pktmbuf_alloc)
        arr = (C.POINTER(Mbuf) * len(ms))(*[C.pointer(m) for m in ms])
        return arr, (bufs, ms)

    STALE = 0xFFFFFFFFFFFFFFFF  # a generation no list state has: re-look every frame up

    def deliver(self, frames: list[bytes], verdicts: np.ndarray, rcs: np.ndarray | None = None,
                gen: int = STALE) -> int:
        """apply verdicts (flow ids = stable ids, see to_ids) made against the
        lists of generation `gen`; the default trusts no flow id and looks every
        frame up again on the live lists.  rcs (int32[n], optional) receives the
        per-frame return codes"""
        arr, keep = self.mbufs(frames)
        verdicts = np.ascontiguousarray(verdicts, VERDICT_DTYPE)
        r = self.lib.nstack_deliver(C.cast(arr, _vp), len(frames), _ptr(verdicts), gen, _ptr(rcs))
        self._let_go(arr, len(frames), keep)
        if r < 0:
            _check(r, "nstack_deliver")
        return r

    def rx_burst(self, frames: list[bytes]):
        arr, keep = self.mbufs(frames)
        rcs = np.zeros(len(frames), np.int32)
        v = np.zeros(len(frames), VERDICT_DTYPE)
        r = self.lib.nstack_rx_burst(C.cast(arr, _vp), len(frames), _ptr(rcs), _ptr(v))
        self._let_go(arr, len(frames), keep)
        if r < 0:
            _check(r, "nstack_rx_burst")
        return r, rcs, v

    def rx_submit(self, frames: list[bytes]):
        """nstack_rx_submit: the burst goes to the GPU; rx_complete delivers it"""
        arr, keep = self.mbufs(frames)
        rcs = np.zeros(len(frames), np.int32)
        v = np.zeros(len(frames), VERDICT_DTYPE)
        r = self.lib.nstack_rx_submit(C.cast(arr, _vp), len(frames), _ptr(rcs), _ptr(v))
        if r < 0:
            _check(r, "nstack_rx_submit")
        if not hasattr(self, "_pend"):
            self._pend = []
        self._pend.append((arr, len(frames), keep, rcs, v))
        return r

    def rx_complete(self):
        """nstack_rx_complete: deliver the oldest submitted burst: (delivered, rcs, verdicts)
        of that burst, as rx_burst returns them"""
        r = self.lib.nstack_rx_complete()
        arr, n, keep, rcs, v = self._pend.pop(0)
        self._let_go(arr, n, keep)
        if r < 0:
            _check(r, "nstack_rx_complete")
        return r, rcs, v

    def rx_pending(self) -> int:
        return int(self.lib.nstack_rx_pending())

    def rx_submit_mbufs(self, arr, n: int, rcs: np.ndarray | None = None) -> int:
        """nstack_rx_submit over prebuilt descriptors (mbufs_over); keep arr
        (and rcs) alive until rx_complete_mbufs"""
        r = self.lib.nstack_rx_submit(C.cast(arr, _vp), n, _ptr(rcs), None)
        if r < 0:
            _check(r, "nstack_rx_submit")
        return r

    def rx_complete_mbufs(self) -> int:
        r = self.lib.nstack_rx_complete()
        if r < 0:
            _check(r, "nstack_rx_complete")
        return r

    def _let_go(self, arr, n, keep):
        """after a burst call: in place, the frames stay alive while the stack
        holds them (kept here until fini) and the caller's references go"""
        if getattr(self, "_inplace", False):
            self._held.append((arr, keep))
            self.lib.nstack_mbufs_put(C.cast(arr, _vp), n)

    def set_rx_inplace(self, on: bool = True):
        """nstack_set_rx_inplace (no release callback: poll Mbuf.refcnt)"""
        self._inplace = bool(on)
        if not hasattr(self, "_held"):
            self._held = []
        _check(self.lib.nstack_set_rx_inplace(1 if on else 0, None, None), "nstack_set_rx_inplace")

    def reclaim(self):
        """nstack_reclaim: free what application threads let go of (protocol thread)"""
        self.lib.nstack_reclaim()

    def mbufs_put(self, arr, n: int):
        """nstack_mbufs_put: drop the caller's reference on n mbufs"""
        self.lib.nstack_mbufs_put(C.cast(arr, _vp), n)

    def drain_all_sum(self, buf: np.ndarray):
        """nstack_drain_all_sum: (items received, bytes, sum of FNV-1a 64 of what each read returned)"""
        nb, hs = _u64(), _u64()
        r = self.lib.nstack_drain_all_sum(_ptr(buf), buf.nbytes, C.byref(nb), C.byref(hs))
        if r < 0:
            _check(int(r), "nstack_drain_all_sum")
        return int(r), nb.value, hs.value

    @staticmethod
    def mbufs_over(pkts: np.ndarray, off: np.ndarray, lens: np.ndarray, off_unit_log2: int):
        """rte_mbuf-shaped descriptors over a packed burst (no copies; keep
        pkts alive while they are used): (array, n)"""
        n = len(off)
        ms = (Mbuf * n)()
        base = pkts.ctypes.data
        for i in range(n):
            ms[i].buf_addr = base + (int(off[i]) << off_unit_log2)
            ms[i].data_len = int(lens[i])
            ms[i].refcnt = 1  # the caller's reference (rte_pktmbuf_alloc)
        arr = (C.POINTER(Mbuf) * n)(*[C.pointer(ms[i]) for i in range(n)])
        return arr, ms

    def rx_burst_mbufs(self, arr, n: int, rcs: np.ndarray | None = None) -> int:
        """nstack_rx_burst over prebuilt descriptors (mbufs_over)"""
        r = self.lib.nstack_rx_burst(C.cast(arr, _vp), n, _ptr(rcs), None)
        if r < 0:
            _check(r, "nstack_rx_burst")
        # a two-half burst whose second half failed returns the first half's
        # count and reports the error per frame in rcs: raise it
        if rcs is not None and n and int(rcs[:n].min()) < -3:  # (the reference's own codes are -3..1)
            _check(int(rcs[:n].min()), "nstack_rx_burst (second half)")
        return r

    def drain_all(self, buf: np.ndarray):
        """nstack_drain_all: (items received, bytes)"""
        nb = _u64()
        r = self.lib.nstack_drain_all(_ptr(buf), buf.nbytes, C.byref(nb))
        if r < 0:
            _check(int(r), "nstack_drain_all")
        return int(r), nb.value

    def stat(self, which):
        return self.lib.nstack_stat(which)

    def set_local(self, ip: str, mac: bytes):
        """gLocalIp + port MAC (netfamily.c:11, 415)"""
        return self.lib.nstack_set_local(ip_raw(ip), (C.c_uint8 * 6)(*mac))

    def arp_insert(self, ip: str, mac: bytes) -> int:
        return self.lib.nstack_arp_insert(ip_raw(ip), (C.c_uint8 * 6)(*mac))

    def set_tx_encode(self, on: bool = True):
        """nstack_set_tx_encode: tx_burst(cksum=True) builds its frames on the
        GPU (K5) from descriptors instead of framing them on the host"""
        return self.lib.nstack_set_tx_encode(1 if on else 0)

    def set_tx_mss(self, mss: int):
        """nstack_set_tx_mss: tcp_out sends a fragment longer than mss (a multiple
        of 4; 0 = off) as MSS-sized frames"""
        _check(self.lib.nstack_set_tx_mss(mss), "nstack_set_tx_mss")
        return 0

    def set_tx_mtu(self, mtu: int):
        """nstack_set_tx_mtu: udp_out sends a datagram that does not fit the IPv4
        MTU (68..65535) as IPv4 fragments; 0 = off"""
        _check(self.lib.nstack_set_tx_mtu(mtu), "nstack_set_tx_mtu")
        return 0

    def set_rx_gro(self, window: int):
        """nstack_set_rx_gro: a connection's in-sequence PSH|ACK trains arrive as
        one receive fragment and one ACK per run of at most about `window` bytes
        (0 = off); raises RxgError (RXG_EINVAL) while in-place receive is on"""
        _check(self.lib.nstack_set_rx_gro(window), "nstack_set_rx_gro")

    def set_rx_assemble(self, on: bool):
        """nstack_set_rx_assemble: each connection's burst assembled into
        contiguous byte ranges and aligned with rcv_nxt (duplicates dropped,
        overlaps trimmed, a stop at every hole); raises RxgError (RXG_EINVAL)
        while coalescing or in-place receive is on; stat(19) / stat(20) count
        the bytes discarded as already received / the ranges behind a hole"""
        _check(self.lib.nstack_set_rx_assemble(1 if on else 0), "nstack_set_rx_assemble")

    def set_rx_order(self, on: bool):
        """nstack_set_rx_order: a burst's segments reach each connection in
        sequence order (stat(16) counts the records moved)"""
        _check(self.lib.nstack_set_rx_order(1 if on else 0), "nstack_set_rx_order")

    def set_rx_ddos(self, on: bool, thresh: float = DDOS_DEFAULT_THRESH):
        """nstack_set_rx_ddos: every received frame through the entropy flood
        detector (detection only; stat(17) frames under alarm, stat(18) rises)"""
        _check(self.lib.nstack_set_rx_ddos(1 if on else 0, thresh), "nstack_set_rx_ddos")

    def ddos_status(self) -> dict:
        """nstack_ddos_status: frames_seen, rises, falls, alarm_frames,
        undef_frames, last_stat, alarm"""
        out = np.zeros(1, NSTACK_DDOS_DTYPE)
        _check(self.lib.nstack_ddos_status(out.ctypes.data), "nstack_ddos_status")
        return {k: out[0][k].item() for k in NSTACK_DDOS_DTYPE.names if not k.startswith("_")}

    def set_syncookies(self, mode: int, key: bytes | None = None):
        """nstack_set_syncookies: 0 off, 1 on, 2 on while the flood detector's
        alarm is up; key: the 16 hash-key bytes"""
        k = np.frombuffer(key, np.uint8).copy() if key is not None else None
        assert k is None or k.size == 16
        _check(self.lib.nstack_set_syncookies(mode, _ptr(k)), "nstack_set_syncookies")

    def syncookie_tick(self, t: int = 0xFFFFFFFF):
        """nstack_syncookie_tick: pin the time counter (0xFFFFFFFF: the clock)"""
        _check(self.lib.nstack_syncookie_tick(t & 0xFFFFFFFF), "nstack_syncookie_tick")

    def syncookie_stats(self) -> dict:
        """nstack_syncookie_stats: SYNs answered, connections accepted, ACKs rejected"""
        out = np.zeros(4, np.uint64)
        _check(self.lib.nstack_syncookie_stats(out.ctypes.data), "nstack_syncookie_stats")
        return {"syn_answered": int(out[0]), "accepted": int(out[1]), "rejected": int(out[2])}

    def set_l2_respond(self, on: bool = True):
        """nstack_set_l2_respond: ARP requests for set_local's address and echo
        requests to it are answered out of the next tx_burst (stat(21) ARP /
        stat(22) echo answers queued, stat(23) dropped for room, stat(24) echo
        requests with a bad checksum or a cut capture); raises RxgError
        (RXG_EINVAL) while no local address is set"""
        _check(self.lib.nstack_set_l2_respond(1 if on else 0), "nstack_set_l2_respond")

    def tx_burst(self, max_frames: int = 256, cap_bytes: int = 1 << 20, cksum: bool = False):
        """one udp_out + tcp_out pass: the frames (bytes) it produced"""
        pk = np.zeros(cap_bytes, np.uint8)
        off = np.zeros(max(max_frames, 1), np.uint32)
        ln = np.zeros(max(max_frames, 1), np.uint16)
        span = C.c_uint64()
        r = self.lib.nstack_tx_burst(_ptr(pk), cap_bytes, _ptr(off), _ptr(ln), max_frames,
                                     int(cksum), C.byref(span))
        if r < 0:
            _check(r, "nstack_tx_burst")
        return [pk[int(o) << 6:(int(o) << 6) + int(n)].tobytes() for o, n in zip(off[:r], ln[:r])]


_COMPILED = {}


def compiled_variants(vs):
    """the variants of `vs` the loaded library has compiled in, in order
    (the product library: KERNEL_VARIANTS; the RX_DIAG build, RXGPU_LIB=
    .../librxgpu_diag.so: also its tuning shapes and ablations).  A variant
    in none of the three lists is an error, not a silent skip"""
    known = set(map(tuple, KERNEL_VARIANTS + DIAG_TUNING_VARIANTS + DIAG_ABLATIONS))
    unknown = [tuple(v) for v in vs if tuple(v) not in known]
    if unknown:
        raise ValueError(f"variants in no build's table: {unknown}")
    out = []
    with Context(HOST_ONLY) as c:
        for v in vs:
            v = tuple(v)
            if v not in _COMPILED:
                try:
                    c.tune(*v)
                    _COMPILED[v] = True
                except RxgError:
                    _COMPILED[v] = False
            if _COMPILED[v]:
                out.append(v)
        c.tune(0)
    return out
