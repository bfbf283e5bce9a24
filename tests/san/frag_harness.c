/* AddressSanitizer / UBSan harness for the host TX encoder with IPv4
 * fragmentation (csrc/tx_encode_host.cpp, rxg_tx_encode_frag_host and
 * rxg_tx_frag_count).  A stand-alone program: compiled with
 * -fsanitize=address,undefined together with that source and run directly
 * (tests/test_tx_frag.py).  Every buffer is a heap allocation of exactly the
 * bytes the call may touch (rxg_tx_frag_count sizes them), so one byte read or
 * written past a payload, a frame's 64-B slot end, off[], len[], first[] or
 * nseg[] is a report:
 *   - the boundary burst (UDP payloads around the cut and the fragment
 *     boundaries, TCP / ARP / unknown kinds between them) at mtu 68, 70, 76,
 *     1500 and 9000, packed and in slots, with 65507-B and 65508-B payloads;
 *   - out_cap and cap_bytes that end inside a datagram's fragments, with
 *     off[] / len[] of exactly out_cap entries;
 *   - a refused mtu.
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

#define NLEN 13
#define NMAX (NLEN * 4 + 2)

static void fill_desc(rxg_txd *d, uint8_t kind, uint32_t pay_len, uint8_t optlen, uint32_t i) {
    static const uint8_t fl[3] = {0x10, 0x18, 0x19};
    memset(d, 0, sizeof(*d));
    memset(d->dst_mac, kind == RXG_TXD_ARP && (i & 1) ? 0xFF : 0x02, 6);
    memset(d->src_mac, 0x0C, 6);
    d->sip = 0x4D64A8C0u, d->dip = 0x0100000Au;
    d->sport = (uint16_t)(0xB922 + i), d->dport = 0xB315;
    d->seq = 0xFFFFFF00u + 77u * i, d->ack = 7;
    d->window = 0x3908, d->urp = 1;
    d->hdrlen_off = 0x50, d->tcp_flags = fl[i % 3];
    d->kind = kind;
    d->optlen = kind == RXG_TXD_TCP ? optlen : 0;
    d->pay_len = pay_len;
}

/* the boundary burst; returns the descriptor count */
static uint32_t all_descs(rxg_txd *d, uint32_t mss, uint32_t mtu, int big) {
    const uint32_t m = mtu - 28, fp = (mtu - 20) & ~7u, b = mss ? mss : 20;
    const uint32_t lens[NLEN] = {0,          1,          m - 1,      m,          m + 1,
                                 fp - 9,     fp - 8,     fp - 7,     2 * fp - 9, 2 * fp - 8,
                                 2 * fp - 7, 4 * fp + 3, 5 * fp - 8};
    uint32_t k = 0;
    for (uint32_t i = 0; i < NLEN; i++) {
        fill_desc(&d[k++], RXG_TXD_UDP, lens[i], 0, i);
        if (i % 3 == 0) fill_desc(&d[k++], RXG_TXD_TCP, (i / 3) * b + 1, (uint8_t)(i / 3), i);
        if (i % 5 == 0) fill_desc(&d[k++], RXG_TXD_ARP, 77, 0, i);
        if (i % 6 == 0) fill_desc(&d[k++], 7, 10, 0, i);
    }
    if (big) {
        fill_desc(&d[k++], RXG_TXD_UDP, 65507, 0, 2);
        fill_desc(&d[k++], RXG_TXD_UDP, 65508, 0, 3);
    }
    CHECK(k <= NMAX);
    return k;
}

/* payloads at 16-B aligned offsets in a buffer that ends with the last
 * payload's last byte (skipped descriptors and ARP have none) */
static uint8_t *payloads(rxg_txd *d, uint32_t n, uint32_t mss, uint32_t mtu, uint64_t *pend) {
    uint64_t pbytes = 0;
    *pend = 0;
    for (uint32_t k = 0; k < n; k++) {
        uint64_t own = 0;
        CHECK(rxg_tx_frag_count(&d[k], 1, mss, mtu, NULL, &own) == RXG_OK);
        const uint32_t pl = own && d[k].kind <= RXG_TXD_TCP ? d[k].pay_len : 0;
        /* a skipped descriptor's payload is never looked at */
        d[k].pay_off16 = !own ? 0xFFFFFFFFu : pl ? (uint32_t)(pbytes >> 4) : 0u;
        if (pl) *pend = pbytes + pl;
        pbytes += (pl + 15u) & ~15u;
    }
    uint8_t *pay = malloc(*pend ? *pend : 1);
    for (uint64_t i = 0; i < *pend; i++) pay[i] = (uint8_t)(i * 13 + 5);
    return pay;
}

/* one call into exact-size buffers; cut_e / cut_b: entries / bytes less than
 * the whole burst needs */
static void run(uint32_t mss, uint32_t mtu, int big, uint32_t slot, uint32_t cut_e, uint64_t cut_b,
                uint32_t flags) {
    rxg_txd *d = malloc(NMAX * sizeof(*d));
    const uint32_t n = all_descs(d, mss, mtu, big);
    uint64_t pend = 0, ent = 0, bytes = 0;
    uint8_t *pay = payloads(d, n, mss, mtu, &pend);
    CHECK(rxg_tx_frag_count(d, n, mss, mtu, &ent, &bytes) == RXG_OK);
    CHECK(ent >= n && ent < 100000);
    const uint64_t cap = (slot ? ent * slot : bytes) - cut_b;
    const uint32_t out_cap = (uint32_t)ent - cut_e;
    uint8_t *pk = malloc(cap);
    memset(pk, 0xA5, cap);
    uint32_t *off = malloc((size_t)out_cap * 4), *first = malloc((size_t)n * 4);
    uint32_t *nseg = malloc((size_t)n * 4), tot[8];
    uint16_t *len = malloc((size_t)out_cap * 2);
    uint64_t span = 0;
    const int rc = rxg_tx_encode_frag_host(d, n, pay, pend, mss, mtu, pk, cap, slot, off, len, out_cap,
                                           first, nseg, flags, &span, tot);
    CHECK(rc == RXG_ERANGE); /* the unknown kinds, at least */
    CHECK((((uint64_t)tot[5] << 32) | tot[4]) == ent && span <= cap);
    CHECK(span == (((uint64_t)tot[2] << 32) | tot[1]));
    uint64_t frames = 0, skipped = 0, e = 0;
    const uint32_t fp = (mtu - 20) & ~7u;
    for (uint32_t k = 0; k < n; k++) {
        CHECK(first[k] == e);
        if (!nseg[k]) {
            uint64_t own = 0; /* a skipped descriptor keeps its entries, zeroed below out_cap */
            CHECK(rxg_tx_frag_count(&d[k], 1, mss, mtu, &own, NULL) == RXG_OK && own >= 1);
            for (uint64_t j = 0; j < own; j++, e++)
                if (e < out_cap) CHECK(len[e] == 0 && off[e] == 0);
            skipped++;
            continue;
        }
        CHECK(e + nseg[k] <= out_cap);
        const int cutd = d[k].kind == RXG_TXD_UDP && 28ull + d[k].pay_len > mtu;
        CHECK(!cutd || nseg[k] > 1);
        uint32_t got = 0; /* a cut datagram's payload bytes, in order, are the descriptor's */
        for (uint32_t j = 0; j < nseg[k]; j++, e++) {
            const uint8_t *f = pk + (uint64_t)off[e] * 64;
            CHECK((uint64_t)off[e] * 64 + ((len[e] + 63u) & ~63u) <= span);
            if (slot) CHECK((uint64_t)off[e] * 64 == e * slot);
            if (!cutd) continue;
            const uint32_t hdr = j ? 34u : 42u, pl = len[e] - hdr;
            CHECK(len[e] - 14u <= mtu);
            CHECK(pl == 0 || memcmp(f + hdr, pay + (uint64_t)d[k].pay_off16 * 16 + got, pl) == 0);
            CHECK((((uint32_t)f[18] << 8) | f[19]) == (d[k].seq & 0xFFFFu));
            CHECK((((uint32_t)f[20] << 8) | f[21]) == ((j * fp / 8) | (j + 1 < nseg[k] ? 0x2000u : 0u)));
            if (flags & RXG_TXE_NO_CKSUM) CHECK(f[24] == 0 && f[25] == 0 && (j || (f[40] | f[41]) == 0));
            got += pl;
        }
        CHECK(!cutd || got == d[k].pay_len);
        frames += nseg[k];
    }
    CHECK(e == ent && tot[0] == frames && tot[3] == skipped);
    for (uint64_t i = span; i < cap; i++) CHECK(pk[i] == 0xA5);
    free(d), free(pay), free(pk), free(off), free(len), free(first), free(nseg);
}

int main(void) {
    static const uint32_t mtu[5] = {68, 70, 76, 1500, 9000}, mss[5] = {20, 0, 20, 1460, 0};
    static const uint32_t slots[5] = {128, 128, 128, 1600, 9088};
    for (int m = 0; m < 5; m++) {
        const int big = mtu[m] == 68 || mtu[m] == 1500;
        run(mss[m], mtu[m], big, 0, 0, 0, 0);
        run(mss[m], mtu[m], big, 0, 0, 0, RXG_TXE_NO_CKSUM);
        run(mss[m], mtu[m], big, slots[m], 0, 0, 0);
        /* capacity ends inside the last descriptors' fragments */
        run(mss[m], mtu[m], 0, 0, 2, 0, 0);
        run(mss[m], mtu[m], 0, 0, 0, 64, 0);
        run(mss[m], mtu[m], 0, slots[m], 3, 0, 0);
        run(mss[m], mtu[m], 0, slots[m], 0, 3 * 64, 0);
        run(mss[m], mtu[m], big, 0, 9, 5 * 64, 0);
    }
    run(0, 65535, 1, 0, 0, 0, 0); /* the largest mtu: nothing is cut, 65508 is skipped */
    uint64_t e = 1, b = 1;
    rxg_txd one;
    fill_desc(&one, RXG_TXD_UDP, 100, 0, 0);
    CHECK(rxg_tx_frag_count(&one, 1, 0, 67, &e, &b) == RXG_EINVAL && e == 0 && b == 0);
    CHECK(rxg_tx_frag_count(&one, 1, 0, 65536, &e, &b) == RXG_EINVAL);
    CHECK(rxg_tx_encode_frag_host(&one, 1, NULL, 0, 0, 67, NULL, 0, 0, NULL, NULL, 0, NULL, NULL, 0,
                                  NULL, NULL) == RXG_EINVAL);
    CHECK(rxg_tx_encode_frag_host(NULL, 0, NULL, 0, 20, 1500, NULL, 0, 0, NULL, NULL, 0, NULL, NULL, 0,
                                  &e, NULL) == RXG_OK && e == 0);
    printf("FRAG SAN OK\n");
    return 0;
}
