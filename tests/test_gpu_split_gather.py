"""The RSS split and shard gather kernels (csrc/rx_split.hip) against the
independent numpy models of split_ref.py, bit for bit.

Model self-checks (CPU): the Toeplitz hash against the Microsoft table and the
oracle, and shards + split against the host rxg_rss_split on every burst the
device tests use.  Device tests (-m gpu): split_count / scan_u64 /
split_scatter / split_first through rxg_rss_split_dev, gather_units /
gather_offsets / gather_copy through rxg_gather_dev, then split + gather +
classify of every shard, and rxdist.build_shard(mode="split").

Every output buffer is pre-filled with a sentinel and carries spare room, so a
write outside the promised range shows; every device packet buffer ends in the
64 zero bytes of slack the other device tests append."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import frames as F
import oracle_bind as O
import rxdist
import rxgpu as R
import split_ref as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KATS = json.load(open(os.path.join(GOLD, "kats.json")))
L_IP = "192.168.100.77"
CHUNK = 4096                 # frames per split / gather block
SENT32, SENT16, FILL = 0x5A5A5A5A, 0x5A5A, 0xAB
RXG_ERANGE = -34


# ---- bursts (built once, never modified) -----------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _imix_burst():
    """small IMIX: 300 UDP + 300 TCP flows, ARP / ICMP mixed in; (pk, off, ln, unit_log2)"""
    cfg = rxdist.gen_cfg("cfg4", n_udp=300, n_tcp=300, other_per10k=300)
    return _frozen(*R.gen_host(cfg, 17, 3 * CHUNK + 1, 6)) + (6,)


@functools.lru_cache(maxsize=None)
def _udp64_burst(n):
    """64-B UDP frames over 1024 flows: with 64 shards every shard is hit"""
    cfg = rxdist.gen_cfg("cfg2", n_udp=1024)
    return _frozen(*R.gen_host(cfg, 3, n, 6)) + (6,)


@functools.lru_cache(maxsize=None)
def _shard_frames():
    """(64, 64) uint8: one 64-B UDP frame per shard of 64, found with the model"""
    sports = np.arange(1024, 1024 + 4096)
    t = np.frombuffer(F.udp_frame("10.0.0.1", 0, L_IP, 20000, bytes(22)), np.uint8)
    assert len(t) == 64
    cand = np.tile(t, (len(sports), 1))
    cand[:, 34] = sports >> 8
    cand[:, 35] = sports & 0xFF
    sh = S.toeplitz(cand[:, 26:38]) % 64
    pick = [int(np.nonzero(sh == s)[0][0]) for s in range(64)]  # IndexError: no tuple for s
    return _frozen(cand[pick].copy())[0]


ORDER_N = 2 * CHUNK + 77
ORDERS = {
    "all_shards_in_every_wave": lambda i: i % 64,
    "one_shard_per_wave": lambda i: (i // 64) % 64,
    "one_shard_per_step": lambda i: (i // 256) % 64,
    "one_flow": lambda i: np.full_like(i, 37),
}


@functools.lru_cache(maxsize=None)
def _order_burst(name):
    if name == "all_arp":
        fr = np.zeros((ORDER_N, 64), np.uint8)
        fr[:, :60] = np.frombuffer(F.arp_frame("10.0.0.1", L_IP), np.uint8)
        ln = np.full(ORDER_N, 60, np.uint16)
    else:
        fr = _shard_frames()[ORDERS[name](np.arange(ORDER_N))]
        ln = np.full(ORDER_N, 64, np.uint16)
    return _frozen(fr.reshape(-1).copy(), np.arange(ORDER_N, dtype=np.uint32), ln) + (6,)


TRUNC_CAPS = [0, 1, 12, 13, 14, 15, 16, 17, 23, 24, 26, 30, 33, 34, 35, 36, 37, 38, 39, 40, 47, 48]


def _ihl6(proto, l4: bytes) -> bytes:
    return F.ether(F.ipv4_header("10.1.2.3", L_IP, proto, 4 + len(l4), ver_ihl=0x46) +
                   bytes([0x94, 0x04, 0x5A, 0xC3]) + l4)


@functools.lru_cache(maxsize=None)
def _trunc_burst():
    """truncated captures packed at 16-B units; random garbage between a
    frame's captured length and its 16-B end"""
    rng = np.random.default_rng(0x7C)
    tcp_l4 = F.tcp_frame("10.1.2.3", 777, L_IP, 9999, b"y" * 30)[34:]
    udp_l4 = F.udp_frame("10.1.2.3", 777, L_IP, 20001, b"z" * 30)[34:]
    kinds = [F.udp_frame("10.9.8.7", 4321, L_IP, 20007, b"u" * 40),
             F.tcp_frame("10.9.8.7", 4321, L_IP, 9999, b"t" * 40),
             F.icmp_frame("10.9.8.7", L_IP), F.arp_frame("10.9.8.7", L_IP),
             F.ether(bytes(rng.integers(0, 256, 60, dtype=np.uint8)), ethertype=0x86DD),
             _ihl6(6, tcp_l4), _ihl6(17, udp_l4)]
    frames, caps = [], []
    for f in kinds:
        for c in TRUNC_CAPS + [len(f)]:
            frames.append(f)
            caps.append(c)
    order = rng.permutation(len(frames))
    off, pos = [], 0
    for k in order:
        off.append(pos >> 4)
        pos += max(16, (caps[k] + 15) & ~15)
    pk = rng.integers(0, 256, pos, dtype=np.uint8)
    for o, k in zip(off, order):
        pk[o << 4:(o << 4) + caps[k]] = np.frombuffer(frames[k][:caps[k]], np.uint8)
    return _frozen(pk, np.array(off, np.uint32), np.array([caps[k] for k in order], np.uint16)) + (4,)


SCAN_NS = [17 * CHUNK + 5, 40 * CHUNK + 1]  # 1152 counts (per = 2), 2624 counts (per = 3)

# (id, burst, n, n_shards): every burst of the device split tests
SPLIT_CASES = [(f"imix-n{n}-nsh{nsh}", _imix_burst, n, nsh) for n, nsh in [
    (0, 1), (0, 64), (1, 1), (1, 64), (63, 2), (64, 64), (65, 3), (255, 7), (256, 64), (257, 2),
    (4095, 3), (4096, 64), (4097, 7), (4097, 1), (3 * CHUNK + 1, 64), (3 * CHUNK + 1, 3)]]
SCAN_CASES = [(f"udp64-n{n}-nsh64", functools.partial(_udp64_burst, n), n, 64) for n in SCAN_NS]
ORDER_CASES = [(name, functools.partial(_order_burst, name), ORDER_N, 64)
               for name in list(ORDERS) + ["all_arp"]]
TRUNC_CASES = [(f"trunc-nsh{nsh}", _trunc_burst, None, nsh) for nsh in (7, 64)]


def _case(c):
    _, burst, n, nsh = c
    pk, off, ln, ul = burst()
    n = len(off) if n is None else n
    return pk, off[:n], ln[:n], ul, nsh


def _ids(cases):
    return [c[0] for c in cases]


# ---- model self-checks (CPU) -----------------------------------------------
@pytest.mark.parametrize("case", KATS["ms_rss"], ids=lambda c: c["sip"])
def test_model_toeplitz_ms_kats(case):
    s, d = R.ip_raw(case["sip"]), R.ip_raw(case["dst"])
    sp, dp = R.port_raw(case["sport"]), R.port_raw(case["dport"])
    assert int(S.toeplitz(S.tuple_bytes(s, d, 0, 0))[0]) == case["ipv4"]
    assert int(S.toeplitz(S.tuple_bytes(s, d, sp, dp))[0]) == case["ipv4_tcp"]


def test_model_toeplitz_equals_oracle_on_random_tuples():
    rng = np.random.default_rng(0x70E)
    n = 2000
    sip, dip = rng.integers(0, 1 << 32, n, dtype=np.uint64), rng.integers(0, 1 << 32, n, dtype=np.uint64)
    sp, dp = rng.integers(0, 1 << 16, n), rng.integers(0, 1 << 16, n)
    sp[::7], dp[::11] = 0, 0
    got = S.toeplitz(S.tuple_bytes(sip, dip, sp, dp))
    want = np.array([O.rss_hash(int(a), int(b), int(c), int(d))
                     for a, b, c, d in zip(sip, dip, sp, dp)], np.uint32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", SCAN_NS)
def test_scan_bursts_fill_every_shard(n):
    """a condition on the input of the scan cases: no shard of 64 is empty"""
    pk, off, ln, ul = _udp64_burst(n)
    first, _ = S.split(S.shards(pk, off, ln, ul, 64), 64)
    assert np.all(np.diff(first.astype(np.int64)) > 0)


def test_order_bursts_have_the_intended_shard_sequence():
    i = np.arange(ORDER_N)
    for name, seq in ORDERS.items():
        pk, off, ln, ul = _order_burst(name)
        assert np.array_equal(S.shards(pk, off, ln, ul, 64), seq(i)), name
    pk, off, ln, ul = _order_burst("all_arp")
    assert not S.shards(pk, off, ln, ul, 64).any()


def test_trunc_burst_covers_both_sides_of_every_field():
    pk, off, ln, ul = _trunc_burst()
    assert set(TRUNC_CAPS) <= set(ln.tolist())
    sh = S.shards(pk, off, ln, ul, 64)
    assert len(np.unique(sh)) > 8 and (sh[ln < 14] == 0).all()


@pytest.mark.parametrize("case", SPLIT_CASES + SCAN_CASES + ORDER_CASES + TRUNC_CASES,
                         ids=_ids(SPLIT_CASES + SCAN_CASES + ORDER_CASES + TRUNC_CASES))
def test_model_split_equals_host_split(case):
    pk, off, ln, ul, nsh = _case(case)
    wf, wp = S.split(S.shards(pk, off, ln, ul, nsh), nsh)
    hf, hp = R.rss_split(pk, off, ln, ul, nsh)
    assert np.array_equal(hf, wf)
    assert np.array_equal(hp, wp)


def test_model_gather_layout():
    pk = np.arange(256, dtype=np.uint8)
    off, ln = np.array([0, 2, 9], np.uint32), np.array([0, 65, 16], np.uint16)
    dst, doff, dlen, span = S.gather(pk, off, ln, 4, [2, 0, 1, 2])
    assert span == 64 * 5 and doff.tolist() == [0, 1, 2, 4] and dlen.tolist() == [16, 0, 65, 16]
    assert dst[:16].tolist() == list(range(144, 160)) and not dst[16:128].any()
    assert dst[128:193].tolist() == list(range(32, 97)) and not dst[193:256].any()
    assert dst[256:272].tolist() == list(range(144, 160)) and not dst[272:].any()


# ---- device harness ---------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (no fallback path exists)")
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(gpu):
    with R.Context(0) as c:
        yield c


def _to_dev(torch, dev, pk, off, ln):
    d_pk = torch.from_numpy(np.concatenate([pk, np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(np.array(off, np.uint32).view(np.int32)).to(dev)  # copies: the
    d_ln = torch.from_numpy(np.array(ln, np.uint16).view(np.int16)).to(dev)    # bursts are read-only
    return d_pk, d_off, d_ln


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _first_diff(got, want):
    d = np.nonzero(got != want)[0]
    if not len(d):
        return "equal"
    k = int(d[0])
    return f"{len(d)} differ, first at {k}: got {got[k:k + 8].tolist()} want {want[k:k + 8].tolist()}"


def _split_outputs(torch, dev, n, nsh):
    d_first = torch.full((nsh + 1 + 8,), SENT32, dtype=torch.int32, device=dev)
    d_perm = torch.full((n + 16,), SENT32, dtype=torch.int32, device=dev)
    return d_first, d_perm


def _assert_split(d_first, d_perm, n, nsh, wf, wp, what=""):
    first = d_first.cpu().numpy().view(np.uint32)
    perm = d_perm.cpu().numpy().view(np.uint32)
    assert np.array_equal(first[:nsh + 1], wf), (what, "first", _first_diff(first[:nsh + 1], wf))
    assert np.array_equal(perm[:n], wp), (what, "perm", _first_diff(perm[:n], wp))
    assert (first[nsh + 1:] == SENT32).all(), (what, "first[] written past n_shards + 1")
    assert (perm[n:] == SENT32).all(), (what, "perm[] written past n", perm[n:].tolist())


def _run_split(gpu, ctx, case):
    torch, dev = gpu
    pk, off, ln, ul, nsh = _case(case)
    n = len(off)
    wf, wp = S.split(S.shards(pk, off, ln, ul, nsh), nsh)
    d_pk, d_off, d_ln = _to_dev(torch, dev, pk, off, ln)
    d_first, d_perm = _split_outputs(torch, dev, n, nsh)
    ctx.rss_split_dev(d_pk, d_off, d_ln, n, ul, nsh, d_first, d_perm, stream=_stream(torch, dev))
    torch.cuda.synchronize(dev)
    _assert_split(d_first, d_perm, n, nsh, wf, wp, case[0])


# ---- 2. device split ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLIT_CASES, ids=_ids(SPLIT_CASES))
def test_split_chunk_wave_and_shard_count_edges(gpu, ctx, case):
    """n around a wave, a 256-frame step and a 4096-frame chunk, n of 0 and 1,
    1 to 64 shards, mixed IMIX traffic"""
    _run_split(gpu, ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SCAN_CASES, ids=_ids(SCAN_CASES))
def test_split_scan_of_more_than_1024_counts(gpu, ctx, case):
    """scan_u64's multi-element path: 1152 counts (2 per thread) and 2624
    counts (3 per thread, the last threads with an empty range)"""
    _run_split(gpu, ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ORDER_CASES, ids=_ids(ORDER_CASES))
def test_split_scatter_rank_on_constructed_shard_orders(gpu, ctx, case):
    """the ballot rank, the per-wave carry and the per-step carry on shard
    sequences IMIX never produces: 64 shards in every wave, the shard changing
    exactly at wave / step boundaries, one shard only, and all ARP"""
    _run_split(gpu, ctx, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TRUNC_CASES, ids=_ids(TRUNC_CASES))
def test_split_truncated_captures_at_16_byte_units(gpu, ctx, case):
    """captures ending before, inside and after every field of the shard rule,
    frames packed 16 B apart, garbage after each captured length"""
    _run_split(gpu, ctx, case)


@pytest.mark.gpu
def test_split_workspace_reuse_across_sizes_and_streams(gpu):
    """one context: small, large (the workspace grows after a use), small,
    large, large, alternating between two streams (the event-wait path), no
    host synchronisation in between; every result exact"""
    torch, dev = gpu
    big = _case(SCAN_CASES[1])
    pk, off, ln, ul = _imix_burst()
    small = (pk, off[:65], ln[:65], ul, 3)
    want, devs = [], []
    for pk, off, ln, ul, nsh in (small, big):
        want.append(S.split(S.shards(pk, off, ln, ul, nsh), nsh))
        devs.append(_to_dev(torch, dev, pk, off, ln))
    s = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    plan = [(0, 0), (1, 1), (0, 0), (1, 1), (1, 0), (0, 1)]  # (burst, stream)
    outs = [_split_outputs(torch, dev, len((small, big)[b][1]), (small, big)[b][4]) for b, _ in plan]
    torch.cuda.synchronize(dev)
    with R.Context(0) as c:
        for (b, k), (d_first, d_perm) in zip(plan, outs):
            _, o, _, ul, nsh = (small, big)[b]
            c.rss_split_dev(*devs[b], len(o), ul, nsh, d_first, d_perm, stream=s[k].cuda_stream)
        torch.cuda.synchronize(dev)
    for step, ((b, k), (d_first, d_perm)) in enumerate(zip(plan, outs)):
        _, o, _, _, nsh = (small, big)[b]
        _assert_split(d_first, d_perm, len(o), nsh, *want[b], what=f"step {step}")


# ---- 3. device gather ---------------------------------------------------------
def _random_source(lens, unit_log2, seed, slot_units=None):
    """frames of the given lengths laid out in 1 << unit_log2 units (packed, or
    slot_units apart); every byte random, so whatever no frame owns — the
    bytes between a frame's length and its 16-B end included — is garbage"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    unit = 1 << unit_log2
    units = np.maximum(1, (lens + unit - 1) // unit) if slot_units is None else \
        np.full(len(lens), slot_units)
    assert (units * unit >= lens).all()
    off = np.cumsum(units) - units
    pk = rng.integers(0, 256, int(units.sum()) * unit, dtype=np.uint8)
    return _frozen(pk, off.astype(np.uint32), lens.astype(np.uint16))


@functools.lru_cache(maxsize=None)
def _imix_source():
    rng = np.random.default_rng(0x1A1)
    return _random_source(rng.choice([64, 576, 1500], 2 * CHUNK + 1, p=[7 / 12, 4 / 12, 1 / 12]), 6, 1)


EDGE_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 1500, 9000, 65535]


def _gather_raw(gpu, ctx, src, ul, idx, cap):
    """rxg_gather_dev through the raw binding, d_idx / d_dst_off / d_dst_len
    passed as slices that start at element 1 of larger buffers.  Returns
    (rc, span, dst, dst_off buffer, dst_len buffer) on the host."""
    torch, dev = gpu
    idx = np.asarray(idx, np.int64)
    count = len(idx)
    d_pk, d_off, d_ln = _to_dev(torch, dev, *src)
    d_idx = torch.from_numpy(np.concatenate([[0], idx, [0, 0]]).astype(np.int32)).to(dev)
    d_dst = torch.full((cap + 256,), FILL, dtype=torch.uint8, device=dev)
    d_doff = torch.full((count + 9,), SENT32, dtype=torch.int32, device=dev)
    d_dlen = torch.full((count + 9,), SENT16, dtype=torch.int16, device=dev)
    span = C.c_uint64(0xDEAD)
    rc = R._gather_dev(ctx._h, d_pk.data_ptr(), d_off.data_ptr(), d_ln.data_ptr(), ul,
                       d_idx[1:].data_ptr(), count, d_dst.data_ptr(), cap, d_doff[1:].data_ptr(),
                       d_dlen[1:].data_ptr(), C.byref(span), _stream(torch, dev))
    torch.cuda.synchronize(dev)
    return (rc, span.value, d_dst.cpu().numpy(), d_doff.cpu().numpy().view(np.uint32),
            d_dlen.cpu().numpy().view(np.uint16))


def _assert_index_outputs(doff, dlen, count, want_off, want_len, what):
    assert np.array_equal(doff[1:1 + count], want_off), (what, "dst_off", _first_diff(doff[1:1 + count], want_off))
    assert np.array_equal(dlen[1:1 + count], want_len), (what, "dst_len", _first_diff(dlen[1:1 + count], want_len))
    assert doff[0] == SENT32 and (doff[1 + count:] == SENT32).all(), (what, "dst_off outside [0, count)")
    assert dlen[0] == SENT16 and (dlen[1 + count:] == SENT16).all(), (what, "dst_len outside [0, count)")


def _check_gather(gpu, ctx, src, ul, idx, what=""):
    """dst_cap == the model's span exactly: RXG_OK, every byte of the span, the
    sentinel after it, offsets, lengths and the returned span"""
    w_dst, w_off, w_len, w_span = S.gather(*src, ul, idx)
    rc, span, dst, doff, dlen = _gather_raw(gpu, ctx, src, ul, idx, w_span)
    assert rc == 0 and span == w_span, (what, rc, span, w_span)
    _assert_index_outputs(doff, dlen, len(idx), w_off, w_len, what)
    assert np.array_equal(dst[:w_span], w_dst), (what, "bytes", _first_diff(dst[:w_span], w_dst))
    assert (dst[w_span:] == FILL).all(), (what, "written past the packed span")


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 2 * CHUNK + 1])
def test_gather_counts_around_groups_steps_and_chunks(gpu, ctx, count):
    _check_gather(gpu, ctx, _imix_source(), 6, np.arange(count), f"count {count}")


@pytest.mark.gpu
@pytest.mark.parametrize("ul", [4, 6])
def test_gather_frame_lengths_0_to_65535(gpu, ctx, ul):
    """zero-length frames take one unit; lengths around a 16-B chunk and a
    64-B unit; a 65,535-B frame; zero tails where the source holds garbage"""
    src = _random_source(EDGE_LENS + EDGE_LENS[::-1] + [65535, 0, 0, 1], ul, 2 + ul)
    _check_gather(gpu, ctx, src, ul, np.arange(len(src[1])), f"unit_log2 {ul}")


@pytest.mark.gpu
def test_gather_from_2k_slots(gpu, ctx):
    rng = np.random.default_rng(0x2B)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 1500, 2047, 2048] + rng.integers(0, 2049, 300).tolist()
    src = _random_source(lens, 11, 11, slot_units=1)
    _check_gather(gpu, ctx, src, 11, rng.permutation(len(lens)), "2-KiB slots")


def _index_lists():
    n = 600
    rng = np.random.default_rng(0x1D)
    dup = np.arange(n)
    dup = np.concatenate([dup[:6], [5], dup[6:400], [5, 399], dup[400:], [0, 5]])
    return {"identity": np.arange(n), "reversed": np.arange(n)[::-1], "strided": np.arange(n)[::3],
            "random_subset": rng.choice(n, 211, replace=False), "duplicates": dup}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_index_lists()))
def test_gather_index_lists(gpu, ctx, name):
    pk, off, ln = _imix_source()
    src = (pk[:int(off[600]) << 6], off[:600], ln[:600])
    _check_gather(gpu, ctx, src, 6, _index_lists()[name], name)


@pytest.mark.gpu
def test_gather_count_zero_writes_nothing(gpu, ctx):
    rc, span, dst, doff, dlen = _gather_raw(gpu, ctx, _random_source([64, 100], 6, 5), 6, [], 128)
    assert rc == 0 and span == 0
    assert (dst == FILL).all() and (doff == SENT32).all() and (dlen == SENT16).all()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["span_minus_64", "inside_a_1500B_frame", "zero"])
def test_gather_erange_copies_only_what_fits(gpu, ctx, which):
    """RXG_ERANGE: *span is the size needed, the offsets and lengths are
    complete, frames that end at or below dst_cap are exact, nothing at or past
    dst_cap is written, and the context still works"""
    rng = np.random.default_rng(0xE2)
    lens = rng.choice([0, 64, 65, 576, 1500], 300).tolist() + [1500, 64, 1500]
    src = _random_source(lens, 6, 7)
    idx = np.arange(len(lens))
    w_dst, w_off, w_len, w_span = S.gather(*src, 6, idx)
    k = int(np.nonzero(w_len == 1500)[0][3])
    cap = {"span_minus_64": w_span - 64, "inside_a_1500B_frame": (int(w_off[k]) << 6) + 768,
           "zero": 0}[which]
    rc, span, dst, doff, dlen = _gather_raw(gpu, ctx, src, 6, idx, cap)
    assert rc == RXG_ERANGE and span == w_span, (rc, span, w_span)
    _assert_index_outputs(doff, dlen, len(idx), w_off, w_len, which)
    ends = (w_off.astype(np.int64) + np.maximum(1, (w_len.astype(np.int64) + 63) // 64)) << 6
    fit = int(ends[ends <= cap].max()) if (ends <= cap).any() else 0
    assert fit < cap or cap == 0  # the cut falls inside a frame
    assert np.array_equal(dst[:fit], w_dst[:fit]), _first_diff(dst[:fit], w_dst[:fit])
    assert (dst[fit:] == FILL).all(), "a frame that does not fit was written"
    _check_gather(gpu, ctx, src, 6, idx, "after RXG_ERANGE")


@pytest.mark.gpu
def test_gather_more_than_1024_chunks(gpu, ctx):
    """scan_u64's multi-element path and its total through the gather: 1026
    chunk sums; 8 source frames of 64 B listed 4.2 M times, checked on the
    device"""
    torch, dev = gpu
    count = 1025 * CHUNK + 1
    pk, off, ln = _random_source([64] * 8, 6, 8)
    order = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    d_pk, d_off, d_ln = _to_dev(torch, dev, pk, off[order], ln)
    g = torch.Generator(device=dev)
    g.manual_seed(0x6A7)
    d_idxb = torch.randint(0, 8, (count + 1,), generator=g, dtype=torch.int32, device=dev)
    d_idx = d_idxb[1:]
    cap = count * 64
    d_dst = torch.full((cap + 256,), FILL, dtype=torch.uint8, device=dev)
    d_doff = torch.full((count + 9,), SENT32, dtype=torch.int32, device=dev)
    d_dlen = torch.full((count + 9,), SENT16, dtype=torch.int16, device=dev)
    try:
        span = ctx.gather_dev(d_pk, d_off, d_ln, 6, d_idx, count, d_dst, cap, d_doff[1:], d_dlen[1:],
                              stream=_stream(torch, dev))
        torch.cuda.synchronize(dev)
        assert span == cap
        src_rows = d_pk[:512].view(8, 64)[torch.from_numpy(order).to(dev)]  # row j = frame j
        ok = True
        for a in range(0, count, 1 << 20):  # bounded temporaries
            rows = src_rows[d_idx[a:a + (1 << 20)].long()]
            ok = ok and torch.equal(d_dst[a * 64:(a + len(rows)) * 64].view(-1, 64), rows)
        assert ok, "packed bytes differ from src[idx]"
        assert bool((d_dst[cap:] == FILL).all())
        assert torch.equal(d_doff[1:1 + count], torch.arange(count, dtype=torch.int32, device=dev))
        assert bool((d_dlen[1:1 + count] == 64).all())
        assert int(d_doff[0]) == SENT32 and bool((d_doff[1 + count:] == SENT32).all())
        assert int(d_dlen[0]) == SENT16 and bool((d_dlen[1 + count:] == SENT16).all())
    finally:
        del d_dst, d_doff, d_dlen, d_idx, d_idxb
        torch.cuda.empty_cache()


# ---- 4. split, gather and classify, every shard -------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nsh", [3, 64])
def test_split_gather_classify_every_shard(gpu, ctx, nsh):
    torch, dev = gpu
    n = 6000
    cfg = rxdist.gen_cfg("cfg4", n_udp=300, n_tcp=300, other_per10k=300)
    pk, off, ln = R.gen_host(cfg, 29, n, 6)
    udp, tcb = R.gen_flows(cfg)
    want, wcnt = O.Tables(udp, tcb).classify(pk, off, ln, 6, counts=True)
    wf, wp = S.split(S.shards(pk, off, ln, 6, nsh), nsh)
    d_pk, d_off, d_ln = _to_dev(torch, dev, pk, off, ln)
    d_first, d_perm = _split_outputs(torch, dev, n, nsh)
    st = _stream(torch, dev)
    ctx.flows_sync(udp, tcb)
    ctx.rss_split_dev(d_pk, d_off, d_ln, n, 6, nsh, d_first, d_perm, stream=st)
    torch.cuda.synchronize(dev)
    _assert_split(d_first, d_perm, n, nsh, wf, wp)
    got = np.zeros(n, R.VERDICT_DTYPE)
    total = np.zeros(len(wcnt), np.uint64)
    for s in range(nsh):
        a, b = int(wf[s]), int(wf[s + 1])
        cnt = b - a
        w_dst, w_off, w_len, w_span = S.gather(pk, off, ln, 6, wp[a:b])
        dst = torch.zeros(w_span + 64, dtype=torch.uint8, device=dev)
        doff = torch.full((cnt + 1,), SENT32, dtype=torch.int32, device=dev)
        dlen = torch.full((cnt + 1,), SENT16, dtype=torch.int16, device=dev)
        span = ctx.gather_dev(d_pk, d_off, d_ln, 6, d_perm[a:b], cnt, dst, w_span, doff, dlen, stream=st)
        assert span == w_span, s
        h = dst.cpu().numpy()
        assert np.array_equal(h[:w_span], w_dst), (s, _first_diff(h[:w_span], w_dst))
        assert not h[w_span:].any(), s
        assert np.array_equal(doff.cpu().numpy().view(np.uint32)[:cnt], w_off), s
        assert np.array_equal(dlen.cpu().numpy().view(np.uint16)[:cnt], w_len), s
        if cnt == 0:
            continue
        o = torch.empty(cnt * 16, dtype=torch.uint8, device=dev)
        c = torch.zeros(ctx.num_flows, dtype=torch.int64, device=dev)
        ctx.classify_dev(dst, doff, dlen, cnt, 6, 354, o, c, stream=st)
        torch.cuda.synchronize(dev)
        got[wp[a:b]] = o.cpu().numpy().view(R.VERDICT_DTYPE)
        total += c.cpu().numpy().view(np.uint64)
    assert got.tobytes() == want.tobytes()
    assert np.array_equal(total, wcnt)


# ---- 5. rxdist.build_shard(mode="split") ---------------------------------------
@pytest.mark.gpu
def test_build_shard_split_mode_partitions_the_global_burst(gpu, ctx, monkeypatch):
    """three ranks' shards of one 3 x 5000-frame burst: several gathers into one
    buffer at running offsets through sliced index / offset / length tensors"""
    torch, dev = gpu
    world, n = 3, 5000
    w = rxdist.WORKLOADS["cfg4"]
    monkeypatch.setitem(rxdist.WORKLOADS, "cfg4",
                        dict(w, n=n, gen=dict(w["gen"], n_udp=300, n_tcp=300)))
    cfg = rxdist.gen_cfg("cfg4")
    pk_h, off_h, ln_h = R.gen_host(cfg, 0, world * n, 6)
    udp, tcb = R.gen_flows(cfg)
    want = O.Tables(udp, tcb).classify(pk_h, off_h, ln_h, 6)
    ctx.flows_sync(udp, tcb)
    seen = np.zeros(world * n, np.int64)
    for rank in range(world):
        pk, off, ln, n_local, gidx, _ = rxdist.build_shard(ctx, "cfg4", rank, world, dev,
                                                           torch.cuda.current_stream(dev), mode="split")
        assert n_local == len(gidx) > 0 and np.all(np.diff(gidx) > 0), rank
        seen[gidx] += 1
        w_dst, w_off, w_len, w_span = S.gather(pk_h, off_h, ln_h, 6, gidx)
        h = pk.cpu().numpy()
        assert len(h) == w_span + 64 and not h[w_span:].any(), rank
        assert np.array_equal(h[:w_span], w_dst), (rank, _first_diff(h[:w_span], w_dst))
        assert np.array_equal(off.cpu().numpy().view(np.uint32)[:n_local], w_off), rank
        assert np.array_equal(ln.cpu().numpy().view(np.uint16)[:n_local], w_len), rank
        o = torch.empty(n_local * 16, dtype=torch.uint8, device=dev)
        c = torch.zeros(ctx.num_flows, dtype=torch.int64, device=dev)
        ctx.classify_dev(pk, off, ln, n_local, 6, 354, o, c, stream=_stream(torch, dev))
        torch.cuda.synchronize(dev)
        assert o.cpu().numpy().view(R.VERDICT_DTYPE).tobytes() == want[gidx].tobytes(), rank
    assert (seen == 1).all(), "the ranks' shards do not partition the global burst"
