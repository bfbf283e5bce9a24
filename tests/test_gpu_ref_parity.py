"""GPU kernels against what the reference's own compiled code answered.

Every expected value here is read from tests/golden/ref_*.{pcap,npz,npy},
written by tests/golden/make_ref_golden.py through oracle/_ref/refrun (the
reference's prebuilt objects); the oracle is not asked.  A defect that the
oracle and a kernel share passes tests/test_gpu_parity.py and fails here."""
import os
import sys

import numpy as np
import pytest

import frames as F
import ref_check as RC
import rxgpu as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_TX_VARIANTS = 13   # csrc/tx_cksum.hip k_tx
N_TXE_VARIANTS = 15  # csrc/tx_encode.hip k_txe


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (no fallback path exists)")
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx(torch_dev):
    c = R.Context(0, max_pkts=1 << 14, max_bytes=1 << 22)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rx(ctx):
    """the recorded rx corpus, packed once at 16-B and 64-B units; at 16 B the
    next frame starts right after a cut capture"""
    fl = np.load(os.path.join(GOLD, "ref_rx_flows.npz"))
    frames = F.read_pcap(os.path.join(GOLD, "ref_rx.pcap"))
    exp = np.load(os.path.join(GOLD, "ref_rx_expect.npy"))
    assert exp.dtype == RC.REF_RX_DTYPE and len(exp) == len(frames) >= 1500
    packed = {u: F.pack_frames(frames, u) for u in (4, 6)}
    for a in [exp] + [x for p in packed.values() for x in p]:
        a.setflags(write=False)
    ctx.flows_sync(fl["udp"], fl["tcb"])
    return packed, exp


def _dev_classify(torch_dev, ctx, buf, off, lens, unit_log2, len_hint, v8=False):
    torch, dev = torch_dev
    n = len(off)
    d_pk = torch.from_numpy(np.concatenate([buf, np.zeros(64, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
    d_ln = torch.from_numpy(lens.view(np.int16).copy()).to(dev)
    vb = 8 if v8 else 16
    d_out = torch.full((n * vb + 8,), 0xAB, dtype=torch.uint8, device=dev)  # guard bytes
    fn = ctx.classify_dev8 if v8 else ctx.classify_dev
    fn(d_pk, d_off, d_ln, n, unit_log2, len_hint, d_out, None,
       stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    o = d_out.cpu().numpy()
    assert (o[n * vb:] == 0xAB).all(), "store past the burst's verdicts"
    return o[:n * vb].view(R.VERDICT8_DTYPE if v8 else R.VERDICT_DTYPE)


def _assert_verdicts(v, exp, tag, v8=False):
    bad = RC.verdict_mismatches(v, exp, v8=v8)
    assert not bad, (tag, len(bad), bad[:5])


@pytest.mark.parametrize("unit_log2", [4, 6])
def test_k1_default_paths(ctx, torch_dev, rx, unit_log2):
    """rc, l4_cksum, cksum_ok, flow_id and the UDP payload window of the
    host-buffer path, every default kernel shape (by len_hint) and the 8-B
    verdicts, against udp_process / tcp_process's recorded answers"""
    packed, exp = rx
    buf, off, lens = packed[unit_log2]
    _assert_verdicts(ctx.classify(buf, off, lens, unit_log2), exp, "classify")
    for hint in (64, 354, 1500, 9000):
        _assert_verdicts(_dev_classify(torch_dev, ctx, buf, off, lens, unit_log2, hint), exp,
                         ("classify_dev", hint))
        _assert_verdicts(_dev_classify(torch_dev, ctx, buf, off, lens, unit_log2, hint, v8=True),
                         exp, ("classify_dev8", hint), v8=True)


@pytest.mark.parametrize("variant", R.compiled_variants(R.KERNEL_VARIANTS),
                         ids=lambda v: "v" + "-".join(map(str, v)))
def test_k1_every_variant(ctx, torch_dev, rx, variant):
    packed, exp = rx
    ctx.tune(*variant)
    try:
        for unit_log2 in (4, 6):
            buf, off, lens = packed[unit_log2]
            _assert_verdicts(_dev_classify(torch_dev, ctx, buf, off, lens, unit_log2, 0), exp,
                             (variant, unit_log2))
    finally:
        ctx.tune(0)


@pytest.fixture(scope="module")
def tx():
    """(burst with zeroed fields, off, len, the burst as the reference fills it)"""
    z = np.load(os.path.join(GOLD, "ref_tx.npz"))
    buf, off, lens = z["pkts"], z["off"], z["len"]
    want = buf.copy()
    for i in range(len(off)):
        s, n = int(off[i]) << 4, int(lens[i])
        if z["has_ip"][i] and n >= 26:
            want[s + 24:s + 26] = np.frombuffer(int(z["ipck"][i]).to_bytes(2, "little"), np.uint8)
        if z["has_l4"][i]:
            hole = 40 if buf[s + 23] == 17 else 50
            if n >= hole + 2:
                want[s + hole:s + hole + 2] = np.frombuffer(int(z["l4ck"][i]).to_bytes(2, "little"),
                                                            np.uint8)
    assert not np.array_equal(want, buf) and len(off) >= 300
    # the last frame's IPv4 header sums to 0xFFFF: the reference stores 0 there
    assert F.fold_cksum(buf[(int(off[-1]) << 4) + 14:(int(off[-1]) << 4) + 34].tobytes()) == 0xFFFF
    assert z["has_ip"][-1] and z["ipck"][-1] == 0
    for a in (buf, off, lens, want):
        a.setflags(write=False)
    return buf, off, lens, want


def test_k2_fills_what_the_reference_fills(torch_dev, tx):
    """rxg_tx_cksum_dev at every default width and each k_tx variant: the two
    checksum fields equal rte_ipv4_cksum / rte_ipv4_udptcp_cksum as recorded
    from the reference, every other byte of the buffer is unchanged"""
    torch, dev = torch_dev
    buf, off, lens, want = tx
    with R.Context(0, max_pkts=len(off), max_bytes=len(buf) + 64) as c:
        assert np.array_equal(c.tx_cksum(buf, off, lens, 4), want), "host-buffer path"
        runs = [(hint, None) for hint in (64, 128, 354, 1500, 9000)] + \
            [(1500, v) for v in range(N_TX_VARIANTS)]
        try:
            for hint, v in runs:
                if v is not None:
                    c.tune_tx(v)
                d = torch.from_numpy(buf.copy()).to(dev)
                c.tx_cksum_dev(d, torch.from_numpy(off.view(np.int32).copy()).to(dev),
                               torch.from_numpy(lens.view(np.int16).copy()).to(dev), len(off), 4,
                               hint, torch.cuda.current_stream(dev).cuda_stream)
                torch.cuda.synchronize(dev)
                got = d.cpu().numpy()
                bad = np.flatnonzero(got != want)
                assert len(bad) == 0, (hint, v, len(bad), bad[:5].tolist())
        finally:
            c.tune_tx(R.TX_AUTO)


def test_k5_header_summing_to_ffff(torch_dev, tx):
    """the fused encoder on the descriptor of the corpus's last frame: the
    frame it writes is the recorded one, header checksum 0 included"""
    sys.path.insert(0, GOLD)
    import make_ref_golden as MG
    import txenc_ref as T
    buf, off, lens, want = tx
    sip, dip, sport, dport, frame = MG.ffff_header_udp()
    s = int(off[-1]) << 4
    assert buf[s:s + int(lens[-1])].tobytes() == MG.zero_tx_fields(frame, len(frame))
    d = T.txd(R.TXD_UDP, 3, sip=sip, dip=dip, sport=sport, dport=dport, dst_mac=F.PEER_MAC,
              src_mac=F.LOCAL_MAC)
    t, pay = T.burst([d], payloads=[b"abc"])
    with R.Context(0) as c:
        try:
            for v in [R.TX_AUTO] + list(range(N_TXE_VARIANTS)):
                c.tune_txe(v)
                pk, o, n, rc = c.tx_encode(t, pay, 256)
                assert rc == 0 and int(n[0]) == len(frame)
                assert pk[:len(frame)].tobytes() == want[s:s + len(frame)].tobytes(), v
        finally:
            c.tune_txe(R.TX_AUTO)
