// rx_l2_host.cpp — rxg_l2_host: the L2 responder (K8, csrc/rx_l2.hip,
// rxg_l2_dev) restated in plain C++, frame by frame in burst order, reading
// the frame's bytes one by one.  For callers without a GPU (the socket layer's
// host-verdict path) and as the tests' second opinion.  Host only: no HIP, no
// context, no code shared with the kernels.  The rule is the one of
// include/rxgpu.h ("L2 responder").
#include <stdint.h>
#include <string.h>

#include "../../include/rxgpu.h"

namespace {

inline uint32_t raw32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | (uint32_t)p[1]; }

// the folded one's-complement sum of m[0, n) as big-endian 16-bit words, an
// odd tail byte padded with zero: 0 only when every byte is zero
uint32_t ocsum(const uint8_t *m, uint32_t n) {
    uint64_t s = 0;
    uint32_t i = 0;
    for (; i + 2 <= n; i += 2) s += be16(m + i);
    if (i < n) s += (uint32_t)m[i] << 8;
    while (s >> 16) s = (s >> 16) + (s & 0xFFFFu);
    return (uint32_t)s;
}

int local_of(const rxg_l2_params *p, uint32_t ip) {
    for (uint32_t j = 0; j < p->nlocal; ++j)
        if (p->local[j].ip == ip) return (int)j;
    return -1;
}

const uint8_t arp_fixed[6] = {0x00, 0x01, 0x08, 0x00, 0x06, 0x04};

// the status of frame f (len bytes captured) and, for an answered frame, the
// answer's length and the local address it matched
uint8_t judge(const uint8_t *f, uint32_t len, uint8_t cls, const rxg_l2_params *p, uint32_t *alen,
              int *j) {
    *alen = 0;
    if (len < 42u || (f[6] & 1u)) return 0;
    if (cls == RXG_CLS_ARP) {
        if (memcmp(f + 14, arp_fixed, 6) != 0) return 0;
        if ((*j = local_of(p, raw32(f + 38))) < 0) return 0;
        const uint32_t op = be16(f + 20);
        if (op == 2u) return RXG_L2_ARP_REPLY;
        if (op != 1u) return 0;
        *alen = 42u;
        return RXG_L2_ARP_REQ;
    }
    if (cls != RXG_CLS_IPV4_OTHER) return 0;
    if (f[14] != 0x45u || f[23] != 1u || (be16(f + 20) & 0x3FFFu) != 0u) return 0;
    if ((*j = local_of(p, raw32(f + 30))) < 0) return 0;
    if (f[34] != 8u || f[35] != 0u) return 0;
    const uint32_t tl = be16(f + 16);
    if (tl < 28u) return 0;
    if (14u + tl > len || ocsum(f + 34, tl - 20u) != 0xFFFFu) return RXG_L2_ECHO_BAD;
    *alen = 14u + tl;
    return RXG_L2_ECHO;
}

void put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)(v >> 8), p[1] = (uint8_t)v; }

void answer(const uint8_t *f, uint8_t st, uint32_t alen, const uint8_t mac[6], uint8_t *o) {
    if (st == RXG_L2_ARP_REQ) {
        memcpy(o, f + 22, 6);
        memcpy(o + 6, mac, 6);
        o[12] = 0x08, o[13] = 0x06;
        memcpy(o + 14, arp_fixed, 6);
        o[20] = 0, o[21] = 2;
        memcpy(o + 22, mac, 6);
        memcpy(o + 28, f + 38, 4);
        memcpy(o + 32, f + 22, 6);
        memcpy(o + 38, f + 28, 4);
    } else {
        memcpy(o, f + 6, 6);
        memcpy(o + 6, mac, 6);
        o[12] = 0x08, o[13] = 0x00;
        o[14] = 0x45, o[15] = 0;
        o[16] = f[16], o[17] = f[17];
        memset(o + 18, 0, 4);
        o[22] = 64, o[23] = 1;
        o[24] = o[25] = 0;
        memcpy(o + 26, f + 30, 4);
        memcpy(o + 30, f + 26, 4);
        put16(o + 24, ~ocsum(o + 14, 20) & 0xFFFFu);
        memset(o + 34, 0, 4);
        memcpy(o + 38, f + 38, alen - 38u);
        put16(o + 36, ~ocsum(o + 34, alen - 34u) & 0xFFFFu);
    }
    const uint32_t end = (alen + 63u) & ~63u;
    memset(o + alen, 0, end - alen);
}

} // namespace

int rxg_l2_host(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                uint32_t off_unit_log2, const rxg_verdict *v, const rxg_l2_params *p, uint8_t *status,
                uint8_t *out, uint64_t cap_bytes, uint32_t *roff, uint16_t *rlen, uint32_t *rsrc,
                uint32_t totals[6]) {
    if (!p || !totals || p->nlocal > RXG_L2_MAX_LOCAL) return RXG_EINVAL;
    if (!status || !out || !roff || !rlen || !rsrc) return RXG_EINVAL;
    if (n && (!pkts || !off || !len || !v)) return RXG_EINVAL;
    if (off_unit_log2 < 4 || off_unit_log2 > 16) return RXG_EINVAL;
    uint32_t cnt[5] = {0, 0, 0, 0, 0}, nans = 0;
    uint64_t pos = 0; // 64-B units
    bool full = false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *f = pkts + ((uint64_t)off[i] << off_unit_log2);
        uint32_t alen = 0;
        int j = -1;
        const uint8_t st = judge(f, len[i], v[i].cls, p, &alen, &j);
        status[i] = st;
        ++cnt[st];
        if (!alen || full) continue;
        const uint64_t units = (alen + 63u) >> 6;
        if ((pos + units) * 64u > cap_bytes) {
            full = true;
            continue;
        }
        answer(f, st, alen, p->local[j].mac, out + pos * 64u);
        roff[nans] = (uint32_t)pos, rlen[nans] = (uint16_t)alen, rsrc[nans] = i;
        ++nans;
        pos += units;
    }
    totals[0] = cnt[RXG_L2_ARP_REQ], totals[1] = cnt[RXG_L2_ARP_REPLY];
    totals[2] = cnt[RXG_L2_ECHO], totals[3] = cnt[RXG_L2_ECHO_BAD];
    totals[4] = nans, totals[5] = (uint32_t)pos;
    return RXG_OK;
}
