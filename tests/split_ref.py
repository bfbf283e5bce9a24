"""Reference for the RSS split and shard gather tests — test infrastructure.

Plain numpy models of what include/rxgpu.h promises for rxg_rss_split(_dev)
and rxg_gather_dev, written without librxgpu and without the oracle:
  toeplitz  the Toeplitz hash with the 40-byte Microsoft key over a 12-byte
            input (sip, dip, sport, dport in wire order): for every set input
            bit, MSB first, the XOR of the 32-bit key window at that bit
  shards    the shard of every frame of a burst (fixed offsets: ethertype at
            12, protocol at 23, tuple at 26..37; IP options move nothing)
  split     first[] / perm[] of a shard vector (stable)
  gather    the packed burst of frames idx[]: 64-B units, zero tails
Shared by the model self-checks and the device tests of
test_gpu_split_gather.py."""
import numpy as np

MS_KEY = bytes.fromhex("6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b4"
                       "77cb2da38030f20c6a42b73bbeac01fa")
_KEY_INT = int.from_bytes(MS_KEY, "big")
# window j = key bits [j, j + 32), bit 0 the key's most significant
WINDOWS = np.array([(_KEY_INT >> (320 - 32 - j)) & 0xFFFFFFFF for j in range(96)], np.uint32)


def toeplitz(data: np.ndarray) -> np.ndarray:
    """hash of every row of data ((n, 12) uint8, wire order) -> (n,) uint32"""
    data = np.ascontiguousarray(data, np.uint8).reshape(-1, 12)
    out = np.zeros(len(data), np.uint32)
    for a in range(0, len(data), 1 << 15):  # bounded temporaries
        bits = np.unpackbits(data[a:a + (1 << 15)], axis=1).astype(bool)  # MSB first
        out[a:a + (1 << 15)] = np.bitwise_xor.reduce(np.where(bits, WINDOWS, np.uint32(0)), axis=1)
    return out


def tuple_bytes(sip, dip, sport, dport) -> np.ndarray:
    """(n, 12) hash input of raw network-order values (LE memory order = wire order)"""
    sip, dip = np.atleast_1d(np.asarray(sip, "<u4")), np.atleast_1d(np.asarray(dip, "<u4"))
    sport, dport = np.atleast_1d(np.asarray(sport, "<u2")), np.atleast_1d(np.asarray(dport, "<u2"))
    n = len(sip)
    return np.concatenate([sip.view(np.uint8).reshape(n, 4), dip.view(np.uint8).reshape(n, 4),
                           sport.view(np.uint8).reshape(n, 2), dport.view(np.uint8).reshape(n, 2)],
                          axis=1)


def heads(pk, off, ln, unit_log2) -> np.ndarray:
    """the first 40 bytes of every frame, bytes at or past ln[i] read as 0"""
    pk = np.asarray(pk, np.uint8)
    off, ln = np.asarray(off, np.uint32), np.asarray(ln, np.uint16)
    k = np.arange(40, dtype=np.int64)
    pos = (off.astype(np.int64) << unit_log2)[:, None] + k
    keep = k[None, :] < ln.astype(np.int64)[:, None]
    if len(pk) == 0:
        return np.zeros((len(off), 40), np.uint8)
    h = pk[np.where(keep, pos, 0)]  # masked positions may lie past the buffer: not read
    return np.where(keep, h, np.uint8(0)).astype(np.uint8)


def shards(pk, off, ln, unit_log2, nsh) -> np.ndarray:
    """shard of every frame (int64): 0 unless bytes 12-13 are 08 00, else the
    Toeplitz hash of bytes 26..37 (34..37 as zero unless byte 23 is 6 or 17)
    mod nsh"""
    h = heads(pk, off, ln, unit_log2)
    tup = h[:, 26:38].copy()
    l4 = (h[:, 23] == 6) | (h[:, 23] == 17)
    tup[~l4, 8:12] = 0
    sh = toeplitz(tup).astype(np.int64) % nsh
    ipv4 = (h[:, 12] == 0x08) & (h[:, 13] == 0x00)
    return np.where(ipv4, sh, 0)


def split(sh, nsh):
    """(first[nsh + 1], perm[n]) uint32: prefix counts and the stable order"""
    sh = np.asarray(sh, np.int64)
    first = np.zeros(nsh + 1, np.uint32)
    first[1:] = np.cumsum(np.bincount(sh, minlength=nsh)[:nsh])
    return first, np.argsort(sh, kind="stable").astype(np.uint32)


def gather(pk, off, ln, unit_log2, idx):
    """(dst, dst_off, dst_len, span): frame k = frame idx[k] of the source at
    dst[dst_off[k] << 6 ...], its ln bytes then zeros to its 64-B end"""
    pk = np.asarray(pk, np.uint8)
    idx = np.asarray(idx, np.int64)
    dst_len = np.asarray(ln, np.uint16)[idx]
    units = np.maximum(1, (dst_len.astype(np.int64) + 63) // 64)
    ends = np.cumsum(units)
    dst_off = (ends - units).astype(np.uint32)
    span = 64 * int(ends[-1]) if len(idx) else 0
    dst = np.zeros(span, np.uint8)
    src = np.asarray(off, np.uint32).astype(np.int64)[idx] << unit_log2
    for k in range(len(idx)):
        l, a, b = int(dst_len[k]), int(src[k]), int(dst_off[k]) << 6
        dst[b:b + l] = pk[a:a + l]
    return dst, dst_off, dst_len, span
