"""Runs the reference's own compiled code through oracle/_ref/refrun
(oracle/refrun_main.c) — test infrastructure.

refrun is a stand-alone program, built by `make -C oracle` where the
reference's prebuilt objects exist and never committed.  One Session is one
child process: the tables it builds live for that run, and the cases run in
order.  Record formats: see oracle/refrun_main.c.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFRUN = os.path.join(ROOT, "oracle", "_ref", "refrun")
REF_DIR = os.environ.get("REF", "/root/reference")
NONE = 0xFFFFFFFF

EXIT_REASONS = {70: "the reference called rte_exit", 71: "the reference panicked",
                72: "bad case file", 73: "driver state check failed"}

HOW_API, HOW_HAND, HOW_SYN = 0, 1, 2


def have_refrun() -> bool:
    return os.path.exists(REFRUN)


def have_reference() -> bool:
    return os.path.exists(os.path.join(REF_DIR, "build", "tcp.o"))


class RefrunError(RuntimeError):
    pass


class RecvResult:
    __slots__ = ("buflen", "ret", "sip", "sport", "data", "ret2", "data2")

    def __repr__(self):
        return (f"Recv(buflen={self.buflen}, ret={self.ret}, sip={self.sip:#x}, "
                f"sport={self.sport:#x}, n={len(self.data)}, ret2={self.ret2}, n2={len(self.data2)})")


class RxResult:
    __slots__ = ("rc", "l4_cksum", "family", "delivered", "match", "length", "sport", "dport",
                 "sip", "dip", "protocol", "copied_equal", "recv")

    def __repr__(self):
        return (f"Rx(rc={self.rc}, l4={self.l4_cksum:#06x}, fam={self.family}, "
                f"match={self.match:#x}, delivered={self.delivered})")


def _parse_rx(p: bytes) -> RxResult:
    r = RxResult()
    rc, r.l4_cksum, r.family, r.delivered, r.match = struct.unpack_from("<iHBBI", p, 0)
    r.rc = rc
    r.recv = []
    r.length = r.sport = r.dport = r.sip = r.dip = r.protocol = r.copied_equal = None
    pos = 12
    if r.delivered:
        r.length, r.sport, r.dport, _, r.sip, r.dip, r.protocol, r.copied_equal = \
            struct.unpack_from("<HHHHIIiI", p, pos)
        pos += 24
        while pos < len(p):
            v = RecvResult()
            v.buflen, v.ret, v.sip, v.sport, _, n = struct.unpack_from("<IqIHHI", p, pos)
            pos += 24
            v.data = p[pos:pos + n]
            pos += n
            v.ret2, n2 = struct.unpack_from("<qI", p, pos)
            pos += 12
            v.data2 = p[pos:pos + n2]
            pos += n2
            r.recv.append(v)
    assert pos == len(p), "rx record length"
    return r


class Session:
    """collects table-building steps and cases, then runs them in one child"""

    def __init__(self):
        self._recs = []
        self._kinds = []

    def _add(self, op, payload, result: bool):
        self._recs.append(struct.pack("<II", op, len(payload)) + payload)
        if result:
            self._kinds.append(op)

    # ---- tables (creation order = index, one counter per list) ----
    def udp_sock(self, ip_raw, port_raw, proto=17):
        self._add(1, struct.pack("<IHBB", ip_raw, port_raw, proto, 0), False)

    def tcb(self, sip, dip, sport, dport, status, how=HOW_HAND):
        self._add(2, struct.pack("<IIHHII", sip, dip, sport, dport, status, how), True)

    def tables(self, udp: np.ndarray, tcb: np.ndarray, prefer_real=True):
        """rxgpu UDP_SOCK_DTYPE / TCB_DTYPE arrays; with prefer_real, listeners and
        bound-only sockets come from nsocket/nbind/nlisten and other blocks from
        a SYN through the LISTEN handler where a listener already exists"""
        for u in udp:
            self.udp_sock(int(u["localip"]), int(u["localport"]), int(u["protocol"]))
        for t in tcb:
            sip, dip, sport, dport, st = (int(t["sip"]), int(t["dip"]), int(t["sport"]),
                                          int(t["dport"]), int(t["status"]))
            how = HOW_HAND
            if prefer_real:
                if sip == 0 and sport == 0 and st in (0, 1):
                    how = HOW_API
                elif st != 1:
                    how = HOW_SYN
            self.tcb(sip, dip, sport, dport, st, how)

    # ---- cases ----
    def cksum(self, buf: bytes, align=0):
        self._add(3, struct.pack("<I", align) + bytes(buf), True)

    def lookup_udp(self, dip, port, proto=17):
        self._add(4, struct.pack("<IHBB", dip, port, proto, 0), True)

    def lookup_tcp(self, sip, dip, sport, dport):
        self._add(5, struct.pack("<IIHH", sip, dip, sport, dport), True)

    def rx(self, frame: bytes, recv=False, delta=3):
        self._add(6, struct.pack("<II", 1 if recv else 0, delta) + bytes(frame), True)

    def tx(self, frame: bytes):
        self._add(7, bytes(frame), True)

    def run(self, timeout=120):
        """results in case order: cksum -> (raw, udptcp, ipv4); lookups -> index
        or NONE; rx -> RxResult; tx -> (ipck, l4ck, has_ip, has_l4).  How each
        tcb was made goes to self.how_used."""
        if not have_refrun():
            raise RefrunError("oracle/_ref/refrun is not built")
        with tempfile.TemporaryDirectory() as d:
            cin, cout = os.path.join(d, "cases.bin"), os.path.join(d, "results.bin")
            with open(cin, "wb") as fh:
                fh.write(b"".join(self._recs))
            try:
                p = subprocess.run([REFRUN, cin, cout], capture_output=True, timeout=timeout)
            except subprocess.TimeoutExpired as e:
                raise RefrunError(f"refrun did not return within {timeout} s") from e
            if p.returncode != 0:
                why = EXIT_REASONS.get(p.returncode, "signal" if p.returncode < 0 else "exit")
                raise RefrunError(f"refrun ended with {p.returncode} ({why}): "
                                  f"{p.stderr.decode(errors='replace')[-300:]}")
            with open(cout, "rb") as fh:
                data = fh.read()
        out, pos = [], 0
        self.how_used = []
        for want in self._kinds:
            op, n = struct.unpack_from("<II", data, pos)
            pos += 8
            p = data[pos:pos + n]
            pos += n
            assert op == want, (op, want)
            if op == 2:
                self.how_used.append(struct.unpack("<I", p)[0])
            elif op == 3:
                out.append(struct.unpack("<HHH", p))
            elif op in (4, 5):
                out.append(struct.unpack("<I", p)[0])
            elif op == 6:
                out.append(_parse_rx(p))
            elif op == 7:
                out.append(struct.unpack("<HHBB", p))
        assert pos == len(data), "trailing result bytes"
        return out
