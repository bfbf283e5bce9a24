// tx_encode_host.cpp — rxg_tx_encode_host: the TX encoder (K5, tx_encode.hip)
// restated in plain C++ for callers without a GPU and as the tests' reference;
// rxg_tx_encode_frag_host / rxg_tx_frag_count: the same with TCP payloads cut
// at an MSS and UDP datagrams at the IPv4 MTU (the layout pass with both cuts
// and tx_encode_frag_kernel of tx_encode.hip), written from the rule in
// include/rxgpu.h; rxg_tx_encode_tso_host / rxg_tx_tso_count: that with
// mtu == 0 (the TSO layout pass and tx_encode_tso_kernel).
// Host only: no HIP, no context.  The frames are those of the reference's
// encoders with both checksums filled:
//   ng_encode_udp_apppkt  udp.c:59-98      ng_encode_tcp_apppkt  tcp.c:420-466
//   ng_encode_arp_pkt     common.c:206-241
//   rte_ipv4_cksum rte_ip.h:255-265, rte_ipv4_udptcp_cksum :325-349 (DPDK 19.11.12)
#include <stdint.h>
#include <string.h>

#include "../../include/rxgpu.h"

static_assert(sizeof(rxg_txd) == 48, "rxg_txd is 48 bytes");

namespace {

inline void wr16be(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}
inline void wr32be(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}
inline uint64_t align64(uint64_t x) { return (x + 63u) & ~63ull; }

// frame length of a descriptor; 0 = skipped (unknown kind, or longer than a
// frame length can say)
uint32_t frame_len(const rxg_txd &d) {
    uint64_t fl = 0;
    if (d.kind == RXG_TXD_UDP) fl = 42ull + d.pay_len;
    else if (d.kind == RXG_TXD_TCP) fl = 54ull + 4ull * d.optlen + d.pay_len;
    else if (d.kind == RXG_TXD_ARP) fl = 42;
    return fl > 65535u ? 0u : (uint32_t)fl;
}

// __rte_raw_cksum over [p, p + n): 16-bit words as they lie in memory, an odd
// last byte as the low half of a word
uint32_t raw_sum(const uint8_t *p, uint32_t n, uint32_t s) {
    uint32_t i = 0;
    for (; i + 1 < n; i += 2) s += (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8);
    if (i < n) s += p[i];
    return s;
}
uint32_t fold16(uint32_t s) {
    s = (s >> 16) + (s & 0xFFFFu);
    s = (s >> 16) + (s & 0xFFFFu);
    return s;
}

// the frame of d (fl bytes) at m, both checksum fields 0
void encode(uint8_t *m, const rxg_txd &d, uint32_t fl, const uint8_t *pay) {
    static const uint8_t ones[6] = {0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF};
    if (d.kind == RXG_TXD_ARP) { // common.c:206-241
        if (memcmp(d.dst_mac, ones, 6)) memcpy(m, d.dst_mac, 6);
        else memset(m, 0, 6);
        memcpy(m + 6, d.src_mac, 6);
        wr16be(m + 12, 0x0806);
        wr16be(m + 14, 1);
        wr16be(m + 16, 0x0800);
        m[18] = 6;
        m[19] = 4;
        wr16be(m + 20, 1);
        memcpy(m + 22, d.src_mac, 6);
        memcpy(m + 28, &d.sip, 4);
        memcpy(m + 32, d.dst_mac, 6);
        memcpy(m + 38, &d.dip, 4);
        return;
    }
    const bool tcp = d.kind == RXG_TXD_TCP;
    memcpy(m, d.dst_mac, 6);
    memcpy(m + 6, d.src_mac, 6);
    wr16be(m + 12, 0x0800);
    uint8_t *ip = m + 14; // udp.c:74-85, tcp.c:434-445
    ip[0] = 0x45;
    ip[1] = 0;
    wr16be(ip + 2, fl - 14);
    memset(ip + 4, 0, 4);
    ip[8] = 64;
    ip[9] = tcp ? 6 : 17;
    ip[10] = ip[11] = 0;
    memcpy(ip + 12, &d.sip, 4);
    memcpy(ip + 16, &d.dip, 4);
    uint8_t *t = m + 34;
    memcpy(t, &d.sport, 2);
    memcpy(t + 2, &d.dport, 2);
    uint32_t hdr = 42;
    if (tcp) { // tcp.c:446-463
        wr32be(t + 4, d.seq);
        wr32be(t + 8, d.ack);
        t[12] = d.hdrlen_off;
        t[13] = d.tcp_flags;
        memcpy(t + 14, &d.window, 2);
        t[16] = t[17] = 0;
        memcpy(t + 18, &d.urp, 2);
        memset(t + 20, 0, 4u * d.optlen);
        hdr = 54u + 4u * d.optlen;
    } else { // udp.c:86-95
        wr16be(t + 4, fl - 34);
        t[6] = t[7] = 0;
    }
    if (fl > hdr) memcpy(m + hdr, pay, fl - hdr);
}

void fill_cksums(uint8_t *m, uint32_t fl, bool tcp) {
    const uint32_t kip = fold16(raw_sum(m + 14, 20, 0));
    const uint16_t hip = (uint16_t)~kip; // plain complement: 0xFFFF stores 0, as the reference's build
    const uint32_t l4n = fl - 34;
    // pseudo-header: sip, dip, {0, proto}, be16(l4 length)
    uint32_t s = raw_sum(m + 26, 8, 0) + ((tcp ? 6u : 17u) << 8) +
                 (((l4n & 0xFFu) << 8) | (l4n >> 8));
    s = raw_sum(m + 34, l4n, s);
    uint16_t k = (uint16_t)~fold16(s);
    if (k == 0 && !tcp) k = 0xFFFF;
    memcpy(m + 24, &hip, 2);
    memcpy(m + (tcp ? 50 : 40), &k, 2);
}

} // namespace

extern "C" int rxg_tx_encode_host(const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                                  uint64_t payload_bytes, uint8_t *pkts, uint64_t cap_bytes,
                                  uint32_t slot_bytes, uint32_t *off, uint16_t *len,
                                  uint32_t flags, uint64_t *span, uint32_t totals[4]) {
    if (span) *span = 0;
    if (totals) memset(totals, 0, 16);
    if (slot_bytes & 63u) return RXG_EINVAL;
    if (n == 0) return RXG_OK;
    if (!txd || !pkts || !off || !len) return RXG_EINVAL;
    for (uint32_t k = 0; k < n; ++k) { // every payload inside the payload buffer
        const uint32_t fl = frame_len(txd[k]);
        if (!fl || txd[k].kind == RXG_TXD_ARP || !txd[k].pay_len) continue;
        if (!payload || (uint64_t)txd[k].pay_off16 * 16 + txd[k].pay_len > payload_bytes)
            return RXG_EINVAL;
    }
    const uint64_t lim = 64ull << 32; // offsets are 32 bits of 64-B units
    const uint64_t cap = cap_bytes < lim ? cap_bytes : lim;
    uint64_t pos = 0, end = 0;
    uint32_t written = 0, skipped = 0;
    bool full = false;
    for (uint32_t k = 0; k < n; ++k) {
        const rxg_txd &d = txd[k];
        uint32_t fl = frame_len(d);
        if (slot_bytes && fl > slot_bytes) fl = 0;
        const uint64_t at = slot_bytes ? (uint64_t)k * slot_bytes : pos;
        const uint64_t room = slot_bytes ? slot_bytes : align64(fl);
        bool ok = fl != 0;
        if (ok && slot_bytes == 0) {
            if (full || at + room > cap) ok = false, full = true;
        } else if (ok && at + room > cap) {
            ok = false;
        }
        if (!ok) {
            off[k] = 0;
            len[k] = 0;
            ++skipped;
            continue;
        }
        uint8_t *m = pkts + at;
        encode(m, d, fl, payload ? payload + (uint64_t)d.pay_off16 * 16 : nullptr);
        if (d.kind != RXG_TXD_ARP && !(flags & RXG_TXE_NO_CKSUM))
            fill_cksums(m, fl, d.kind == RXG_TXD_TCP);
        memset(m + fl, 0, align64(fl) - fl);
        off[k] = (uint32_t)(at >> 6);
        len[k] = (uint16_t)fl;
        end = at + align64(fl);
        if (slot_bytes == 0) pos = end;
        ++written;
    }
    if (span) *span = end;
    if (totals) {
        totals[0] = written;
        totals[1] = (uint32_t)end;
        totals[2] = (uint32_t)(end >> 32);
        totals[3] = skipped;
    }
    return skipped ? RXG_ERANGE : RXG_OK;
}

// ---- the two cuts: TCP segmentation and IPv4 fragmentation of UDP datagrams ----
// (rxg_tx_encode_frag_host, rxg_tx_frag_count; rxg_tx_encode_tso_host and
// rxg_tx_tso_count are the same with mtu == 0, which cuts no datagram)
namespace {

// how descriptor d is cut: s segments (0 = skipped), the frame length of every
// segment but the last (full) and of the last (last); UDP / ARP / mss == 0:
// the one frame of rxg_tx_encode
struct tso_cut {
    uint64_t s;
    uint32_t hdr, full, last;
    uint64_t units() const { return s ? (s - 1) * ((full + 63u) >> 6) + ((last + 63u) >> 6) : 0; }
};
tso_cut cut_of(const rxg_txd &d, uint32_t mss, uint32_t slot_bytes) {
    tso_cut c = {0, 0, 0, 0};
    uint64_t full = 0, last = 0;
    if (d.kind == RXG_TXD_TCP && mss) {
        c.hdr = 54u + 4u * d.optlen;
        c.s = d.pay_len ? ((uint64_t)d.pay_len + mss - 1) / mss : 1;
        full = (uint64_t)c.hdr + (d.pay_len < mss ? d.pay_len : mss);
        last = (uint64_t)c.hdr + (d.pay_len - (c.s - 1) * mss);
    } else {
        if (d.kind == RXG_TXD_UDP) full = 42ull + d.pay_len;
        else if (d.kind == RXG_TXD_TCP) full = 54ull + 4ull * d.optlen + d.pay_len;
        else if (d.kind == RXG_TXD_ARP) full = 42;
        c.hdr = d.kind == RXG_TXD_TCP ? 54u + 4u * d.optlen : 42u;
        c.s = 1;
        last = full;
    }
    if (full == 0 || full > 65535u || (slot_bytes && full > slot_bytes)) c.s = 0;
    c.full = c.s ? (uint32_t)full : 0u;
    c.last = c.s ? (uint32_t)last : 0u;
    return c;
}

// cut_of with the second cut: a UDP descriptor whose datagram (L = 8 + pay_len
// bytes) does not fit the IPv4 MTU becomes s fragments of fp = (mtu - 20) & ~7
// datagram bytes, each a 34-B header and its bytes; everything else is cut_of's
struct frag_cut {
    tso_cut c;
    bool frag;   // a cut UDP datagram
    uint32_t fp; // datagram bytes per fragment
};
frag_cut frag_cut_of(const rxg_txd &d, uint32_t mss, uint32_t mtu, uint32_t slot_bytes) {
    frag_cut f = {{0, 0, 0, 0}, false, 0};
    const uint64_t L = 8ull + d.pay_len;
    if (d.kind != RXG_TXD_UDP || mtu == 0 || 20u + L <= mtu) {
        f.c = cut_of(d, mss, slot_bytes);
        return f;
    }
    f.frag = true;
    f.fp = (mtu - 20u) & ~7u;
    f.c.hdr = 34;
    if (20u + L > 65535u) return f; // no IPv4 datagram is that long
    const uint64_t s = (L + f.fp - 1) / f.fp;
    const uint64_t full = 34ull + (L < f.fp ? L : f.fp), last = 34ull + (L - (s - 1) * f.fp);
    if (full > 65535u || (slot_bytes && full > slot_bytes)) return f;
    f.c.s = s, f.c.full = (uint32_t)full, f.c.last = (uint32_t)last;
    return f;
}

// fragment j of d's datagram at m (fl = 34 + b_j bytes): Ethernet and IPv4
// header, then datagram bytes [j * fp, j * fp + b_j); k16 = the datagram's UDP
// checksum as it lies in memory
void encode_fragment(uint8_t *m, const rxg_txd &d, uint32_t fl, const uint8_t *pay, uint32_t j,
                     uint32_t fp, bool more, uint16_t k16, bool cksum) {
    const uint32_t b = fl - 34u, at = j * fp; // (at <= 65512)
    memcpy(m, d.dst_mac, 6);
    memcpy(m + 6, d.src_mac, 6);
    wr16be(m + 12, 0x0800);
    uint8_t *ip = m + 14;
    ip[0] = 0x45;
    ip[1] = 0;
    wr16be(ip + 2, 20u + b);
    wr16be(ip + 4, d.seq & 0xFFFFu);
    wr16be(ip + 6, (at >> 3) | (more ? 0x2000u : 0u));
    ip[8] = 64;
    ip[9] = 17;
    ip[10] = ip[11] = 0;
    memcpy(ip + 12, &d.sip, 4);
    memcpy(ip + 16, &d.dip, 4);
    if (cksum) {
        const uint16_t hip = (uint16_t)~fold16(raw_sum(ip, 20, 0)); // the plain complement
        memcpy(ip + 10, &hip, 2);
    }
    uint8_t *t = m + 34;
    uint32_t done = 0;
    if (j == 0) { // the UDP header is the datagram's first 8 bytes
        memcpy(t, &d.sport, 2);
        memcpy(t + 2, &d.dport, 2);
        wr16be(t + 4, 8u + d.pay_len);
        memcpy(t + 6, &k16, 2);
        done = 8;
    }
    if (b > done) memcpy(t + done, pay + (at + done - 8u), b - done);
}

// rte_ipv4_udptcp_cksum over d's whole datagram (0 -> 0xFFFF)
uint16_t dgram_cksum(const rxg_txd &d, const uint8_t *pay) {
    const uint32_t L = 8u + d.pay_len;
    uint8_t h[20]; // sip, dip, {0, 17}, be16(L); sport, dport, be16(L), 0
    memcpy(h, &d.sip, 4);
    memcpy(h + 4, &d.dip, 4);
    h[8] = 0, h[9] = 17;
    wr16be(h + 10, L);
    memcpy(h + 12, &d.sport, 2);
    memcpy(h + 14, &d.dport, 2);
    wr16be(h + 16, L);
    h[18] = h[19] = 0;
    uint32_t s = raw_sum(h, 20, 0);
    if (d.pay_len) s = raw_sum(pay, d.pay_len, s);
    uint16_t k = (uint16_t)~fold16(s);
    return k ? k : (uint16_t)0xFFFF;
}

bool mtu_ok(uint32_t mtu) { return mtu == 0 || (mtu >= 68u && mtu <= 65535u); }

} // namespace

extern "C" int rxg_tx_frag_count(const rxg_txd *txd, uint32_t n, uint32_t mss, uint32_t mtu,
                                 uint64_t *entries, uint64_t *packed_bytes) {
    if (entries) *entries = 0;
    if (packed_bytes) *packed_bytes = 0;
    if ((mss & 3u) || !mtu_ok(mtu)) return RXG_EINVAL;
    if (n && !txd) return RXG_EINVAL;
    uint64_t e = 0, u = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const frag_cut f = frag_cut_of(txd[k], mss, mtu, 0);
        e += f.c.s ? f.c.s : 1;
        u += f.c.units();
    }
    if (entries) *entries = e;
    if (packed_bytes) *packed_bytes = u << 6;
    return RXG_OK;
}

extern "C" int rxg_tx_encode_frag_host(const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                                       uint64_t payload_bytes, uint32_t mss, uint32_t mtu,
                                       uint8_t *pkts, uint64_t cap_bytes, uint32_t slot_bytes,
                                       uint32_t *off, uint16_t *len, uint32_t out_cap,
                                       uint32_t *first, uint32_t *nseg, uint32_t flags,
                                       uint64_t *span, uint32_t totals[8]) {
    if (span) *span = 0;
    if (totals) memset(totals, 0, 32);
    if ((slot_bytes & 63u) || (mss & 3u) || !mtu_ok(mtu)) return RXG_EINVAL;
    if (n == 0) return RXG_OK;
    if (!txd || !pkts || !first || !nseg || (out_cap && (!off || !len))) return RXG_EINVAL;
    for (uint32_t k = 0; k < n; ++k) { // every payload inside the payload buffer
        const frag_cut f = frag_cut_of(txd[k], mss, mtu, slot_bytes);
        if (!f.c.s || txd[k].kind == RXG_TXD_ARP || !txd[k].pay_len) continue;
        if (!payload || (uint64_t)txd[k].pay_off16 * 16 + txd[k].pay_len > payload_bytes)
            return RXG_EINVAL;
    }
    const uint64_t lim = 64ull << 32; // offsets are 32 bits of 64-B units
    const uint64_t cap = cap_bytes < lim ? cap_bytes : lim;
    const bool cksum = !(flags & RXG_TXE_NO_CKSUM);
    uint64_t fe = 0, pos = 0, end = 0, frames = 0;
    uint32_t written = 0;
    bool full = false;
    for (uint32_t k = 0; k < n; ++k) {
        const rxg_txd &d = txd[k];
        const frag_cut f = frag_cut_of(d, mss, mtu, slot_bytes);
        const tso_cut &c = f.c;
        const uint64_t ne = c.s ? c.s : 1;
        bool ok = c.s != 0 && fe + c.s <= out_cap;
        if (ok && slot_bytes) {
            ok = (fe + c.s) * slot_bytes <= cap;
        } else if (ok) {
            if (full || pos + (c.units() << 6) > cap) ok = false, full = true;
        }
        first[k] = fe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)fe;
        nseg[k] = ok ? (uint32_t)c.s : 0u;
        if (!ok) {
            for (uint64_t e = fe; e < fe + ne && e < out_cap; ++e) off[e] = 0, len[e] = 0;
            fe += ne;
            continue;
        }
        const uint8_t *src = payload ? payload + (uint64_t)d.pay_off16 * 16 : nullptr;
        const uint16_t k16 = f.frag && cksum ? dgram_cksum(d, src) : (uint16_t)0;
        for (uint64_t j = 0; j < c.s; ++j) {
            const uint32_t fl = j + 1 == c.s ? c.last : c.full;
            const uint64_t at = slot_bytes ? (fe + j) * slot_bytes : pos;
            uint8_t *m = pkts + at;
            if (f.frag) {
                encode_fragment(m, d, fl, src, (uint32_t)j, f.fp, j + 1 != c.s, k16, cksum);
            } else {
                rxg_txd g = d;
                if (c.s > 1) { // (s == 1: the descriptor as it is, whatever mss)
                    g.seq = d.seq + (uint32_t)(j * mss);
                    g.pay_len = fl - c.hdr;
                    if (j + 1 != c.s) g.tcp_flags = d.tcp_flags & (uint8_t)~0x09u; // FIN, PSH
                }
                encode(m, g, fl, src ? src + j * mss : nullptr);
                if (d.kind != RXG_TXD_ARP && cksum) fill_cksums(m, fl, d.kind == RXG_TXD_TCP);
            }
            memset(m + fl, 0, align64(fl) - fl);
            off[fe + j] = (uint32_t)(at >> 6);
            len[fe + j] = (uint16_t)fl;
            end = at + align64(fl);
            if (slot_bytes == 0) pos = end;
        }
        frames += c.s;
        fe += ne;
        ++written;
    }
    if (span) *span = end;
    if (totals) {
        totals[0] = (uint32_t)frames;
        totals[1] = (uint32_t)end;
        totals[2] = (uint32_t)(end >> 32);
        totals[3] = n - written;
        totals[4] = (uint32_t)fe;
        totals[5] = (uint32_t)(fe >> 32);
    }
    return written != n ? RXG_ERANGE : RXG_OK;
}

// ---- TCP segmentation alone: mtu == 0 (the checks above are these calls' own)
extern "C" int rxg_tx_tso_count(const rxg_txd *txd, uint32_t n, uint32_t mss, uint64_t *entries,
                                uint64_t *packed_bytes) {
    return rxg_tx_frag_count(txd, n, mss, 0, entries, packed_bytes);
}

extern "C" int rxg_tx_encode_tso_host(const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                                      uint64_t payload_bytes, uint32_t mss, uint8_t *pkts,
                                      uint64_t cap_bytes, uint32_t slot_bytes, uint32_t *off,
                                      uint16_t *len, uint32_t out_cap, uint32_t *first,
                                      uint32_t *nseg, uint32_t flags, uint64_t *span,
                                      uint32_t totals[8]) {
    return rxg_tx_encode_frag_host(txd, n, payload, payload_bytes, mss, 0, pkts, cap_bytes, slot_bytes,
                                   off, len, out_cap, first, nseg, flags, span, totals);
}
