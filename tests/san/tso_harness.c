/* AddressSanitizer / UBSan harness for the host TX encoder with TCP
 * segmentation (csrc/tx_encode_host.cpp, rxg_tx_encode_tso_host and
 * rxg_tx_tso_count).  A stand-alone program: compiled with
 * -fsanitize=address,undefined together with that source and run directly
 * (tests/test_tx_tso.py).  Every buffer is a heap allocation of exactly the
 * bytes the call may touch (rxg_tx_tso_count sizes them), so one byte read or
 * written past a payload, a frame's 64-B slot end, off[], len[], first[] or
 * nseg[] is a report:
 *   - the boundary burst (option words x payloads around the segment
 *     boundaries, UDP / ARP / unknown kinds between them) at mss 20, 1460 and
 *     8948, packed and in slots, a 65535-B payload (45 segments) at 1460;
 *   - out_cap and cap_bytes that end inside a descriptor's segments, with
 *     off[] / len[] of exactly out_cap entries;
 *   - a refused mss.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rxgpu.h"

#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__);                         \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

static const uint32_t k_opt[] = {0, 1, 2, 3, 10};
#define NOPT (sizeof(k_opt) / sizeof(k_opt[0]))
#define NLEN 8
#define NMAX (NOPT * NLEN * 2 + 1)

static void fill_desc(rxg_txd *d, uint8_t kind, uint32_t pay_len, uint8_t optlen, uint32_t i) {
    static const uint8_t fl[3] = {0x10, 0x18, 0x19};
    memset(d, 0, sizeof(*d));
    memset(d->dst_mac, kind == RXG_TXD_ARP && (i & 1) ? 0xFF : 0x02, 6);
    memset(d->src_mac, 0x0C, 6);
    d->sip = 0x4D64A8C0u, d->dip = 0x0100000Au;
    d->sport = 0xB922, d->dport = 0xB315;
    d->seq = 0xFFFFFF00u, d->ack = 7;
    d->window = 0x3908, d->urp = 1;
    d->hdrlen_off = 0x50, d->tcp_flags = fl[i % 3];
    d->kind = kind;
    d->optlen = kind == RXG_TXD_TCP ? optlen : 0;
    d->pay_len = pay_len;
}

/* the boundary burst; returns the descriptor count */
static uint32_t all_descs(rxg_txd *d, uint32_t mss, int big) {
    const uint32_t lens[NLEN] = {0, 1, mss - 1, mss, mss + 1, 2 * mss, 4 * mss + 3, 5 * mss};
    uint32_t k = 0, i = 0;
    for (uint32_t o = 0; o < NOPT; o++)
        for (uint32_t l = 0; l < NLEN; l++, i++) {
            fill_desc(&d[k++], RXG_TXD_TCP, lens[l], (uint8_t)k_opt[o], i);
            if (i % 5 == 0) fill_desc(&d[k++], RXG_TXD_UDP, (mss + 7) % 1473, 0, i);
            if (i % 7 == 0) fill_desc(&d[k++], RXG_TXD_ARP, 77, 0, i);
            if (i % 11 == 0) fill_desc(&d[k++], 7, 10, 0, i);
        }
    if (big) fill_desc(&d[k++], RXG_TXD_TCP, 65535, 1, 2);
    CHECK(k <= NMAX);
    return k;
}

/* payloads at 16-B aligned offsets in a buffer that ends with the last
 * payload's last byte (unknown kinds and ARP have none) */
static uint8_t *payloads(rxg_txd *d, uint32_t n, uint64_t *pend) {
    uint64_t pbytes = 0;
    *pend = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t pl = d[k].kind <= RXG_TXD_TCP ? d[k].pay_len : 0;
        /* an unknown kind's payload is never looked at */
        d[k].pay_off16 = d[k].kind > RXG_TXD_ARP ? 0xFFFFFFFFu : pl ? (uint32_t)(pbytes >> 4) : 0u;
        if (pl) *pend = pbytes + pl;
        pbytes += (pl + 15u) & ~15u;
    }
    uint8_t *pay = malloc(*pend ? *pend : 1);
    for (uint64_t i = 0; i < *pend; i++) pay[i] = (uint8_t)(i * 13 + 5);
    return pay;
}

/* one call into exact-size buffers; cut_e / cut_b: entries / bytes less than
 * the whole burst needs */
static void run(uint32_t mss, int big, uint32_t slot, uint32_t cut_e, uint64_t cut_b, uint32_t flags) {
    rxg_txd *d = malloc(NMAX * sizeof(*d));
    const uint32_t n = all_descs(d, mss, big);
    uint64_t pend = 0, ent = 0, bytes = 0;
    uint8_t *pay = payloads(d, n, &pend);
    CHECK(rxg_tx_tso_count(d, n, mss, &ent, &bytes) == RXG_OK);
    CHECK(ent >= n && ent < 100000);
    const uint64_t cap = (slot ? ent * slot : bytes) - cut_b;
    const uint32_t out_cap = (uint32_t)ent - cut_e;
    uint8_t *pk = malloc(cap);
    memset(pk, 0xA5, cap);
    uint32_t *off = malloc((size_t)out_cap * 4), *first = malloc((size_t)n * 4);
    uint32_t *nseg = malloc((size_t)n * 4), tot[8];
    uint16_t *len = malloc((size_t)out_cap * 2);
    uint64_t span = 0;
    const int rc = rxg_tx_encode_tso_host(d, n, pay, pend, mss, pk, cap, slot, off, len, out_cap, first,
                                          nseg, flags, &span, tot);
    CHECK(rc == RXG_ERANGE); /* the unknown kinds, at least */
    CHECK((((uint64_t)tot[5] << 32) | tot[4]) == ent && span <= cap);
    CHECK(span == (((uint64_t)tot[2] << 32) | tot[1]));
    uint64_t frames = 0, skipped = 0, e = 0;
    for (uint32_t k = 0; k < n; k++) {
        CHECK(first[k] == e);
        if (!nseg[k]) {
            uint64_t own = 0; /* a skipped descriptor keeps its entries, zeroed below out_cap */
            CHECK(rxg_tx_tso_count(&d[k], 1, mss, &own, NULL) == RXG_OK && own >= 1);
            for (uint64_t j = 0; j < own; j++, e++)
                if (e < out_cap) CHECK(len[e] == 0 && off[e] == 0);
            skipped++;
            if (!cut_e && !cut_b && !slot) CHECK(d[k].kind > RXG_TXD_ARP);
            continue;
        }
        CHECK(e + nseg[k] <= out_cap);
        uint32_t got = 0; /* the segments' payloads, in order, are the descriptor's */
        const uint32_t hdr = d[k].kind == RXG_TXD_TCP ? 54u + 4u * d[k].optlen : 42u;
        for (uint32_t j = 0; j < nseg[k]; j++, e++) {
            const uint8_t *f = pk + (uint64_t)off[e] * 64;
            CHECK((uint64_t)off[e] * 64 + ((len[e] + 63u) & ~63u) <= span);
            if (slot) CHECK((uint64_t)off[e] * 64 == e * slot);
            if (d[k].kind == RXG_TXD_ARP) continue;
            const uint32_t pl = len[e] - hdr;
            CHECK(pl == 0 || memcmp(f + hdr, pay + (uint64_t)d[k].pay_off16 * 16 + got, pl) == 0);
            if (d[k].kind == RXG_TXD_TCP) {
                const uint32_t seq = ((uint32_t)f[38] << 24) | (f[39] << 16) | (f[40] << 8) | f[41];
                CHECK(seq == d[k].seq + got);
                CHECK(f[47] == (j + 1 == nseg[k] ? d[k].tcp_flags : (d[k].tcp_flags & 0xF6)));
            }
            if (flags & RXG_TXE_NO_CKSUM) CHECK(f[24] == 0 && f[25] == 0);
            got += pl;
        }
        CHECK(d[k].kind == RXG_TXD_ARP || got == d[k].pay_len);
        frames += nseg[k];
    }
    CHECK(e == ent && tot[0] == frames && tot[3] == skipped);
    for (uint64_t i = span; i < cap; i++) CHECK(pk[i] == 0xA5);
    free(d), free(pay), free(pk), free(off), free(len), free(first), free(nseg);
}

int main(void) {
    static const uint32_t mss[3] = {20, 1460, 8948}, slots[3] = {128, 1600, 9088};
    for (int m = 0; m < 3; m++) {
        const int big = mss[m] == 1460;
        run(mss[m], big, 0, 0, 0, 0);
        run(mss[m], big, 0, 0, 0, RXG_TXE_NO_CKSUM);
        run(mss[m], big, slots[m], 0, 0, 0);
        /* capacity ends inside the last descriptors' segments */
        run(mss[m], big, 0, 2, 0, 0);
        run(mss[m], big, 0, 0, 64, 0);
        run(mss[m], big, slots[m], 7, 0, 0);
        run(mss[m], big, slots[m], 0, 3 * 64, 0);
        run(mss[m], big, 0, 9, 5 * 64, 0);
    }
    run(4, 0, 0, 0, 0, 0); /* the smallest mss */
    uint64_t e = 1, b = 1;
    rxg_txd one;
    fill_desc(&one, RXG_TXD_TCP, 100, 0, 0);
    CHECK(rxg_tx_tso_count(&one, 1, 1462, &e, &b) == RXG_EINVAL && e == 0 && b == 0);
    CHECK(rxg_tx_encode_tso_host(&one, 1, NULL, 0, 18, NULL, 0, 0, NULL, NULL, 0, NULL, NULL, 0, NULL,
                                 NULL) == RXG_EINVAL);
    CHECK(rxg_tx_encode_tso_host(NULL, 0, NULL, 0, 20, NULL, 0, 0, NULL, NULL, 0, NULL, NULL, 0, &e,
                                 NULL) == RXG_OK && e == 0);
    printf("TSO SAN OK\n");
    return 0;
}
