// rx_syncookie_host.cpp — rxg_syncookie_host: the SYN-cookie pass (K7,
// csrc/rx_syncookie.hip, rxg_syncookie_dev) restated in plain C++, frame by
// frame in burst order, reading the frame's bytes one by one.  For callers
// without a GPU (the socket layer's host-verdict path) and as the tests'
// second opinion.  Host only: no HIP, no context.  The rule is the one of
// include/rxgpu.h ("SYN cookies").
#include <stdint.h>
#include <string.h>

#include "../../include/rxgpu.h"
#include "rx_siphash.h"

// SipHash-2-4 of any message (the known answers; the cookie hashes 24 bytes)
uint64_t rxg_siphash24(uint64_t k0, uint64_t k1, const uint8_t *msg, uint64_t len) {
    rx_sip s = rx_sip_init(k0, k1);
    uint64_t i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t m = 0;
        for (int b = 0; b < 8; ++b) m |= (uint64_t)msg[i + b] << (8 * b);
        rx_sip_word(s, m);
    }
    uint64_t last = len << 56;
    for (int b = 0; i + b < len; ++b) last |= (uint64_t)msg[i + b] << (8 * b);
    rx_sip_word(s, last);
    return rx_sip_final(s);
}

uint32_t rxg_syncookie_value(uint64_t k0, uint64_t k1, uint32_t sip, uint32_t dip, uint16_t sport,
                             uint16_t dport, uint32_t isn, uint32_t t) {
    uint8_t m[24];
    const uint32_t w[6] = {sip, dip, (uint32_t)sport | ((uint32_t)dport << 16), isn, t, 0u};
    for (int i = 0; i < 24; ++i) m[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    return ((t & 0xFFu) << 24) | ((uint32_t)rxg_siphash24(k0, k1, m, 24) & 0xFFFFFFu);
}

namespace {

inline uint32_t raw32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline uint16_t raw16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t be32(const uint8_t *p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

} // namespace

int rxg_syncookie_host(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                       uint32_t off_unit_log2, const rxg_verdict *v, const uint32_t *lmask,
                       uint32_t id_space, const rxg_ck_params *p, uint8_t *status, rxg_txd *txd,
                       uint32_t totals[4]) {
    if (!p || !totals || p->max_age > 255u) return RXG_EINVAL;
    if (n && (!pkts || !off || !len || !v || !status || !txd)) return RXG_EINVAL;
    if (id_space && !lmask) return RXG_EINVAL;
    if (off_unit_log2 < 4 || off_unit_log2 > 16) return RXG_EINVAL;
    uint32_t nsyn = 0, nok = 0, nbad = 0;
    for (uint32_t i = 0; i < n; ++i) {
        status[i] = 0;
        if (len[i] < 54u || v[i].cls != RXG_CLS_TCP || v[i].rc != RXG_RC_OK) continue;
        const uint32_t id = v[i].flow_id;
        if (id >= id_space || !((lmask[id >> 5] >> (id & 31u)) & 1u)) continue;
        const uint8_t *f = pkts + ((uint64_t)off[i] << off_unit_log2);
        const uint8_t fl = f[47];
        const uint32_t sip = raw32(f + 26), dip = raw32(f + 30);
        const uint16_t sport = raw16(f + 34), dport = raw16(f + 36);
        const uint32_t seq = be32(f + 38), ack = be32(f + 42);
        if ((fl & 0x17u) == 0x02u) {
            rxg_txd d;
            memset(&d, 0, sizeof(d));
            memcpy(d.dst_mac, f + 6, 6);
            memcpy(d.src_mac, f, 6);
            d.sip = dip, d.dip = sip;
            d.sport = dport, d.dport = sport;
            d.seq = rxg_syncookie_value(p->k0, p->k1, sip, dip, sport, dport, seq, p->t);
            d.ack = seq + 1u;
            d.window = p->window;
            d.hdrlen_off = 0x50, d.tcp_flags = 0x12;
            d.kind = RXG_TXD_TCP;
            txd[nsyn++] = d;
            status[i] = RXG_CK_SYN;
        } else if ((fl & 0x16u) == 0x10u) {
            const uint32_t c = ack - 1u, isn = seq - 1u;
            const uint32_t age = ((p->t & 0xFFu) - (c >> 24)) & 0xFFu;
            const bool ok = age <= p->max_age &&
                            (c & 0xFFFFFFu) == (rxg_syncookie_value(p->k0, p->k1, sip, dip, sport, dport,
                                                                    isn, p->t - age) & 0xFFFFFFu);
            status[i] = ok ? RXG_CK_ACK_OK : RXG_CK_ACK_BAD;
            ok ? ++nok : ++nbad;
        }
    }
    totals[0] = nsyn, totals[1] = nok, totals[2] = nbad, totals[3] = 0;
    return RXG_OK;
}
