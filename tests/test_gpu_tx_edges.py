"""K2 (csrc/tx_cksum.hip) at the lengths, burst sizes and layouts where its
variants change path (-m gpu), bit-exact on whole buffers against the oracle's
TX fill (O.tx_cksum; udp.c:84-95, tcp.c:444-463).

A variant gives G lanes to a frame and issues P passes of 16 * G bytes up
front, then batches of 4 passes, so its path changes where the checksum end
e = min(14 + total_length, caplen) crosses P * 16G + k * 64G; a block takes
tiles of T = (256 / G) * FPG frames, and the resident-grid variants stride
over the tiles.  Checked: a sweep over every such length and its neighbours
(with total_length equal to, shorter and longer than the capture), all-ones
payloads up to the largest frame, a UDP sum of 0, bursts of T - 1, T, T + 1
and 2T + 1 frames at 16-, 64- and 2048-byte descriptor units, the second
grid-stride trip, and the host form.  Every run compares the whole buffer,
the fill bytes between the frames included."""
import functools
import struct

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxgpu as R

pytestmark = pytest.mark.gpu
L = "192.168.100.77"
# (G lanes per frame, P passes up front, FPG frames per group) of k_tx[0..12]
TX_VARIANTS = [(4, 1, 4), (4, 2, 2), (8, 12, 1), (16, 8, 1), (4, 1, 1), (8, 1, 1), (4, 1, 4),
               (4, 1, 4), (8, 12, 1), (8, 12, 1), (4, 1, 1), (8, 1, 1), (16, 8, 1)]
TILE = [256 // g * fpg for g, _, fpg in TX_VARIANTS]
RESIDENT = [0, 1, 2, 3, 6, 7, 8, 9, 12]  # the others launch one block per tile
HINTS = (64, 128, 354, 1500, 9000)
SWEEP_TOP = 64 * 141


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (no fallback path exists)")
    return torch.device("cuda", 0)


def _k2(ctx, dev, buf, off, lens, unit_log2, hint):
    import torch
    d = torch.from_numpy(buf.copy()).to(dev)
    ctx.tx_cksum_dev(d, torch.from_numpy(off.view(np.int32)).to(dev),
                     torch.from_numpy(lens.view(np.int16)).to(dev), len(off), unit_log2, hint,
                     torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return d.cpu().numpy()


def _same(got, want, what):
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, (what, len(diff), diff[:8], got[diff[:8]], want[diff[:8]])


def _all_runs(ctx, dev, buf, off, lens, unit_log2, want):
    """the five len_hint defaults, then every entry of k_tx"""
    try:
        for hint in HINTS:
            _same(_k2(ctx, dev, buf, off, lens, unit_log2, hint), want, ("hint", hint))
        for v in range(len(TX_VARIANTS)):
            ctx.tune_tx(v)
            _same(_k2(ctx, dev, buf, off, lens, unit_log2, 1500), want, ("variant", v))
    finally:
        ctx.tune_tx(R.TX_AUTO)


def test_variant_table_matches_the_library():
    with R.Context(0) as ctx:
        try:
            ctx.tune_tx(len(TX_VARIANTS) - 1)
            with pytest.raises(R.RxgError):
                ctx.tune_tx(len(TX_VARIANTS))
        finally:
            ctx.tune_tx(R.TX_AUTO)
    assert len(TILE) == len(TX_VARIANTS) and sorted(set(TILE)) == [16, 32, 64, 128, 256]


# ---- the length sweep --------------------------------------------------------
def _l4_frame(k, size, payload, tl=None):
    """frame k of a burst, `size` bytes: UDP for even k, TCP for odd k"""
    if k % 2 == 0:
        f = F.udp_frame(L, 8889, f"10.0.{k % 250}.1", 5555, payload[:size - 42])
    else:
        f = F.tcp_frame(L, 9999, f"10.0.{k % 250}.9", 40000, payload[:size - 54], seq=k)
    assert len(f) == size
    if tl is not None:
        f = f[:16] + struct.pack(">H", tl) + f[18:]
    return f


def _sum_end(f, cap):
    """K2's checksum end of a frame, None if no L4 sum is taken"""
    h = f[:cap] + bytes(64)
    tl = int.from_bytes(h[16:18], "big")
    if h[12:14] != b"\x08\x00" or h[23] not in (6, 17) or tl < 20:
        return None
    return min(14 + tl, cap)


@functools.lru_cache(maxsize=None)
def _sweep():
    """caplens 0..1100 with 14 + tl == caplen, caplen - 7 (trailing bytes are
    not summed) and caplen + 9 (the sum stops at the capture); 64k + d above
    with the three relations in rotation (where the rotation gives a d in
    {-1, 0, 1} the trailing-bytes relation, a frame with 14 + tl == caplen
    follows, so every multiple of 64 and its neighbours stay checksum ends);
    65535; full-length frames captured at the lengths that decide whether a
    field is written at all"""
    rng = np.random.default_rng(12)
    noise = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    frames, caps = [], []

    def add(cap, rel):
        tl = min(max(cap - 14 + (0, -7, 9)[rel], 0), 65535)
        k = len(frames)
        frames.append(_l4_frame(k, max(cap, 14 + tl, 60), noise[k % 4096:], tl))
        caps.append(cap)
    for cap in range(0, 1101):
        for rel in range(3):
            add(cap, rel)
    turn = 0
    for k in range(18, 142):
        for d in (-17, -16, -15, -2, -1, 0, 1, 2, 15, 16, 17):
            add(64 * k + d, turn % 3)
            if turn % 3 == 1 and abs(d) <= 1:
                add(64 * k + d, 0)
            turn += 1
    add(65535, 0)
    for cap in (24, 25, 26, 33, 34, 39, 40, 41, 42, 49, 50, 51, 52):
        for _ in range(2):  # one UDP, one TCP
            k = len(frames)
            frames.append(_l4_frame(k, 120, noise[k:]))
            caps.append(cap)
    ends = {_sum_end(f, c) for f, c in zip(frames, caps)}
    order = rng.permutation(len(frames))
    buf, off, lens = F.pack_filled(frames, 4, caplens=caps, fill=0xC3, mem_order=order)
    return buf, off, lens, ends, O.tx_cksum(buf, off, lens, 4)


def test_length_sweep(dev):
    buf, off, lens, ends, want = _sweep()
    # every length at which a variant's path changes, and its neighbours, is a
    # checksum end of some frame (the sweep cannot silently lose them)
    for g, p, _ in set(TX_VARIANTS):
        edges = range(p * 16 * g, SWEEP_TOP + 1, 64 * g)
        assert len(edges) > 4 and all({e - 1, e, e + 1} <= ends for e in edges), (g, p)
    assert 65535 in ends and not np.array_equal(want, buf)
    with R.Context(0) as ctx:
        _all_runs(ctx, dev, buf, off, lens, 4, want)


def test_length_sweep_host_form(dev):
    """rxg_tx_cksum on the sweep: span_bytes ends exactly at the last frame's
    last byte"""
    buf, off, lens, _, want = _sweep()
    span = int(((off.astype(np.int64) << 4) + lens).max())
    assert span <= len(buf) - 64
    with R.Context(0, max_pkts=len(off), max_bytes=len(buf)) as ctx:
        _same(ctx.tx_cksum(buf, off, lens, 4), want, "host")


# ---- headroom of the 32-bit partial sums ------------------------------------
def _udp_zero_sum_frame(size):
    """a UDP frame whose checksum computes to 0 (stored as 0xFFFF): the
    payload's last word cancels the rest of the sum"""
    pay = bytearray(b"q" * (size - 44) + b"\0\0")
    udp = struct.pack(">HHHH", 7, 30009, 8 + len(pay), 0) + bytes(pay)
    ip = F.ipv4_header("10.1.2.3", L, 17, len(udp))
    psd = ip[12:20] + bytes([0, 17]) + struct.pack(">H", len(udp))
    pay[-2:] = struct.pack("<H", (~F.fold_cksum(psd + udp)) & 0xFFFF)
    f = F.udp_frame("10.1.2.3", 7, L, 30009, bytes(pay))
    assert f[40:42] == b"\xff\xff" and len(f) == size
    return f[:40] + b"\0\0" + f[42:]  # the field as the encoder leaves it before the fill


def test_all_ones_payloads_and_zero_sum(dev):
    """every payload byte 0xFF at the lengths 64k and at 65535, where the
    partial sums are closest to wrapping; a UDP sum of 0 below 64 bytes and
    above 2048"""
    ones = b"\xff" * 65536
    frames = [_l4_frame(k, 64 * k, ones) for k in range(1, 142)]
    frames += [_l4_frame(0, 65535, ones), _l4_frame(1, 65535, ones)]
    zs = [_udp_zero_sum_frame(60), _udp_zero_sum_frame(2142)]
    frames += zs
    order = np.random.default_rng(13).permutation(len(frames))
    buf, off, lens = F.pack_filled(frames, 4, fill=0xC3, mem_order=order)
    want = O.tx_cksum(buf, off, lens, 4)
    for i in (len(frames) - 2, len(frames) - 1):
        o = int(off[i]) << 4
        assert buf[o + 40] == 0 and want[o + 40] == 0xFF and want[o + 41] == 0xFF
    with R.Context(0) as ctx:
        _all_runs(ctx, dev, buf, off, lens, 4, want)


# ---- tile edges, descriptor units, the second grid-stride trip ---------------
def _rows(n, size, seed):
    """n frames of `size` bytes as an (n, size) array: UDP and TCP alternately,
    total_length = size - 14, everything past the IPv4 header random"""
    rng = np.random.default_rng(seed)
    a = np.empty((n, size), np.uint8)
    a[:, :42] = np.frombuffer(F.udp_frame(L, 8889, "10.0.0.1", 5555, bytes(size - 42))[:42], np.uint8)
    a[:, 34:] = rng.integers(0, 256, (n, size - 34), dtype=np.uint8)
    a[:, 18:20] = (np.arange(n) & 0xFFFF).astype(">u2").view(np.uint8).reshape(n, 2)
    a[:, 26:30] = rng.integers(1, 255, (n, 4), dtype=np.uint8)
    a[1::2, 23] = 6
    return a


def _lay(rows, caps, unit_log2, fill, seed):
    """the rows in slots of their size rounded up to the unit, in shuffled
    memory order, `fill` between and after them"""
    n, size = rows.shape
    slot = -(-size >> unit_log2) << unit_log2
    place = np.random.default_rng(seed).permutation(n)
    buf = np.full(n * slot + 64, fill, np.uint8)
    buf[:n * slot].reshape(n, slot)[place, :size] = rows
    off = (place.astype(np.int64) * slot >> unit_log2).astype(np.uint32)
    return buf, off, np.asarray(caps, np.uint16)


@functools.lru_cache(maxsize=None)
def _tile_burst(n, size, unit_log2):
    """n frames of one size, the last one captured shorter, so an off-by-one
    in the last tile's frame count shows"""
    rows = _master(size)[:n]
    caps = [size] * (n - 1) + [{82: 67, 1454: 1031}[size]]
    buf, off, lens = _lay(rows, caps, unit_log2, 0xA5, n)
    return buf, off, lens, O.tx_cksum(buf, off, lens, unit_log2)


@functools.lru_cache(maxsize=None)
def _master(size):
    return _rows(2 * max(TILE) + 1, size, size)


@pytest.mark.parametrize("unit_log2", [4, 6, 11])
def test_tile_edges(dev, unit_log2):
    """every variant at n in {1, T - 1, T, T + 1, 2T + 1} frames of 82 and of
    1454 bytes, at 16-, 64- and 2048-byte descriptor units with 0xA5 between
    the frames"""
    with R.Context(0) as ctx:
        try:
            for v, t in enumerate(TILE):
                ctx.tune_tx(v)
                for n in (1, t - 1, t, t + 1, 2 * t + 1):
                    for size in (82, 1454):
                        buf, off, lens, want = _tile_burst(n, size, unit_log2)
                        assert not np.array_equal(buf, want)
                        _same(_k2(ctx, dev, buf, off, lens, unit_log2, size), want, (v, n, size))
        finally:
            ctx.tune_tx(R.TX_AUTO)


def test_second_grid_stride_trip(dev):
    """the resident-grid variants capped at one block per CU on CUs * T + T + 1
    frames: CUs + 2 tiles, so blocks 0 and 1 take a second tile"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    top = cus * max(TILE) + max(TILE) + 1
    assert top * 96 < 8 << 20
    rows = _rows(top, 82, 82)
    with R.Context(0) as ctx:
        try:
            for t in sorted({TILE[v] for v in RESIDENT}):
                n = cus * t + t + 1
                buf, off, lens = _lay(rows[:n], [82] * (n - 1) + [67], 4, 0xA5, t)
                want = O.tx_cksum(buf, off, lens, 4)
                for v in RESIDENT:
                    if TILE[v] == t:
                        ctx.tune_tx(v, 1)
                        _same(_k2(ctx, dev, buf, off, lens, 4, 82), want, (v, n))
        finally:
            ctx.tune_tx(R.TX_AUTO)
