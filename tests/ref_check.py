"""What the reference's own compiled code decided for a frame (a record of
tests/ref_bind.py's `rx` case) against a verdict of this project — test
infrastructure shared by the CPU differential tests and the GPU tests that
read the recorded fixtures."""
from __future__ import annotations

import zlib

import numpy as np

import rxgpu as R

REF_RX_DTYPE = np.dtype([
    ("rc", "i1"), ("family", "u1"), ("delivered", "u1"), ("copied_equal", "u1"),
    ("l4_cksum", "<u2"), ("length", "<u2"), ("match", "<u4"), ("sip", "<u4"), ("dip", "<u4"),
    ("sport", "<u2"), ("dport", "<u2"), ("protocol", "<i4"),
    ("recv_buflen", "<u4", (3,)), ("recv_ret", "<i4", (3,)), ("recv_ret2", "<i4", (3,)),
    ("recv_crc", "<u4", (3,))])

NO_SECOND_READ = -100  # recv_ret2 when the first nrecvfrom took the whole datagram


def records(results) -> np.ndarray:
    """ref_bind RxResult list -> REF_RX_DTYPE array (nrecvfrom bytes as CRC-32
    of first read + second read)"""
    out = np.zeros(len(results), REF_RX_DTYPE)
    for i, r in enumerate(results):
        o = out[i]
        o["rc"], o["family"], o["delivered"] = r.rc, r.family, r.delivered
        o["l4_cksum"], o["match"] = r.l4_cksum, r.match
        if r.delivered:
            o["copied_equal"], o["length"] = r.copied_equal, r.length
            o["sip"], o["dip"], o["sport"], o["dport"] = r.sip, r.dip, r.sport, r.dport
            o["protocol"] = r.protocol
            for k, v in enumerate(r.recv):
                o["recv_buflen"][k], o["recv_ret"][k], o["recv_ret2"][k] = v.buflen, v.ret, v.ret2
                o["recv_crc"][k] = zlib.crc32(v.data + v.data2)
    return out


def verdict_mismatches(v: np.ndarray, exp: np.ndarray, v8: bool = False) -> list:
    """every verdict field the reference decides, compared exactly; returns
    [(frame, field, got, want)].  v: VERDICT_DTYPE, or VERDICT8_DTYPE with v8.

    rc ............ the function's return value (1 = handed to the kernel interface)
    cls ........... which function the demux rule chose
    l4_cksum ...... rte_ipv4_udptcp_cksum with the checksum field zeroed
    cksum_ok ...... TCP only: the reference rejects (rc -1) exactly when it differs
    flow_id ....... creation index of the block the reference's lookup returned;
                    TCP looks up only after the checksum passed
    UDP ........... payload_off 42; payload_len = offload.length - 8 when
                    delivered; RXG_F_UDP_SHORT exactly when a found socket
                    got rc -2
    """
    bad = []

    def need(i, field, got, want):
        if int(got) != int(want):
            bad.append((i, field, int(got), int(want)))

    for i in range(len(exp)):
        e = exp[i]
        fam, rc, match = int(e["family"]), int(e["rc"]), int(e["match"])
        if v8:
            st = int(v[i]["status"])
            cls, vrc, ok = st & 7, (st >> 3) & 7, (st >> 6) & 1
            vrc = vrc - 8 if vrc >= 4 else vrc
            poff = int(v[i]["off_neg"]) & 0x7F
            short = cls == R.CLS_UDP and int(v[i]["payload_len"]) == 0
        else:
            cls, vrc, ok = int(v[i]["cls"]), int(v[i]["rc"]), int(v[i]["cksum_ok"])
            poff = int(v[i]["payload_off"])
            short = bool(int(v[i]["flags"]) & R.F_UDP_SHORT)
        need(i, "rc", vrc, rc)
        if fam == 0:
            need(i, "cls is not UDP/TCP", cls in (R.CLS_UDP, R.CLS_TCP), False)
            continue
        need(i, "cls", cls, R.CLS_UDP if fam == 17 else R.CLS_TCP)
        if not v8:
            need(i, "l4_cksum", v[i]["l4_cksum"], e["l4_cksum"])
        if fam == 6:
            need(i, "cksum_ok", ok, rc != R.RC_TCP_BAD_CKSUM)
            need(i, "flow_id", v[i]["flow_id"], match if rc == 0 else R.FLOW_NONE)
            if rc == R.RC_TCP_NO_TCB:
                need(i, "reference match on rc -2", match, R.FLOW_NONE)
        else:
            need(i, "flow_id", v[i]["flow_id"], match)
            need(i, "payload_off", poff, 42)
            if match != R.FLOW_NONE:
                need(i, "UDP_SHORT", short, rc == R.RC_UDP_NOMEM)
            if e["delivered"]:
                need(i, "payload_len", v[i]["payload_len"], int(e["length"]) - 8)
                need(i, "copied bytes equal frame[42:42+length-8]", e["copied_equal"], 1)
    return bad
