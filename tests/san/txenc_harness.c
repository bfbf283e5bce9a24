/* AddressSanitizer / UBSan harness for the host TX encoder
 * (csrc/tx_encode_host.cpp, rxg_tx_encode_host).  A stand-alone program:
 * compiled with -fsanitize=address,undefined together with that source and
 * run directly (tests/test_tx_encode.py).  Every buffer is a heap allocation
 * of exactly the bytes the call may touch, so one byte read or written past a
 * payload, a frame's 64-B slot end, off[] or len[] is a report:
 *   - each boundary length on its own: UDP payloads 0..65493 (22 fills 64 B
 *     exactly, 23 crosses), TCP option words x payloads, both ARP targets;
 *   - all of them as one packed burst and in 1536-B slots, payloads at 16-B
 *     aligned offsets in a buffer that ends with the last payload's last byte;
 *   - skips (unknown kind, oversize, capacity) leave their bytes alone.
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

static const uint32_t k_udp[] = {0, 1, 5, 6, 7, 15, 16, 17, 21, 22, 23, 1458, 1472, 8958, 65493};
static const uint32_t k_opt[] = {0, 1, 3, 10};
static const uint32_t k_tcp[] = {0, 1, 9, 10, 11, 1446};
#define NUDP (sizeof(k_udp) / sizeof(k_udp[0]))
#define NOPT (sizeof(k_opt) / sizeof(k_opt[0]))
#define NTCP (sizeof(k_tcp) / sizeof(k_tcp[0]))
#define NALL (NUDP + NOPT * NTCP + 2)

static uint32_t frame_len(const rxg_txd *d) {
    return d->kind == RXG_TXD_UDP ? 42u + d->pay_len
           : d->kind == RXG_TXD_TCP ? 54u + 4u * d->optlen + d->pay_len
                                    : 42u;
}
static uint64_t up64(uint64_t x) { return (x + 63u) & ~63ull; }

static void fill_desc(rxg_txd *d, uint8_t kind, uint32_t pay_len, uint8_t optlen) {
    memset(d, 0, sizeof(*d));
    memset(d->dst_mac, kind == RXG_TXD_ARP && optlen ? 0xFF : 0x02, 6);
    memset(d->src_mac, 0x0C, 6);
    d->sip = 0x4D64A8C0u, d->dip = 0x0100000Au;
    d->sport = 0xB922, d->dport = 0xB315;
    d->seq = 0xFFFFFFFEu, d->ack = 7;
    d->window = 0x3908, d->urp = 1;
    d->hdrlen_off = 0x50, d->tcp_flags = 0x18;
    d->kind = kind;
    d->optlen = kind == RXG_TXD_TCP ? optlen : 0;
    d->pay_len = pay_len;
}

/* the boundary set */
static void all_descs(rxg_txd *d) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < NUDP; i++) fill_desc(&d[k++], RXG_TXD_UDP, k_udp[i], 0);
    for (uint32_t o = 0; o < NOPT; o++)
        for (uint32_t i = 0; i < NTCP; i++) fill_desc(&d[k++], RXG_TXD_TCP, k_tcp[i], (uint8_t)k_opt[o]);
    fill_desc(&d[k++], RXG_TXD_ARP, 99, 0); /* pay_len of an ARP descriptor is ignored */
    fill_desc(&d[k++], RXG_TXD_ARP, 0, 1);
    CHECK(k == NALL);
}

/* one descriptor, exact-size payload / frame / off / len allocations */
static void one(const rxg_txd *src, uint32_t flags) {
    rxg_txd *d = malloc(sizeof(*d));
    *d = *src;
    d->pay_off16 = 0;
    const uint32_t pl = d->kind == RXG_TXD_ARP ? 0 : d->pay_len, fl = frame_len(d);
    uint8_t *pay = pl ? malloc(pl) : NULL;
    for (uint32_t i = 0; i < pl; i++) pay[i] = (uint8_t)(i * 7 + 1);
    const uint64_t cap = up64(fl);
    uint8_t *pk = malloc(cap);
    uint32_t *off = malloc(4), tot[4];
    uint16_t *len = malloc(2);
    uint64_t span = 0;
    CHECK(rxg_tx_encode_host(d, 1, pay, pl, pk, cap, 0, off, len, flags, &span, tot) == RXG_OK);
    CHECK(span == cap && off[0] == 0 && len[0] == fl && tot[0] == 1 && tot[3] == 0);
    for (uint64_t i = fl; i < cap; i++) CHECK(pk[i] == 0);
    if (d->kind != RXG_TXD_ARP) {
        const uint32_t hdr = fl - pl;
        CHECK(pl == 0 || memcmp(pk + hdr, pay, pl) == 0);
        CHECK(pk[12] == 8 && pk[13] == 0 && pk[14] == 0x45 && pk[22] == 64);
        if (flags & RXG_TXE_NO_CKSUM) CHECK(pk[24] == 0 && pk[25] == 0);
    }
    /* one byte less room: skipped, nothing written */
    memset(pk, 0xA5, cap);
    CHECK(rxg_tx_encode_host(d, 1, pay, pl, pk, cap - 1, 0, off, len, flags, &span, tot) == RXG_ERANGE);
    CHECK(span == 0 && len[0] == 0 && tot[0] == 0 && tot[3] == 1);
    for (uint64_t i = 0; i < cap; i++) CHECK(pk[i] == 0xA5);
    free(d), free(pay), free(pk), free(off), free(len);
}

/* the whole set in one call: packed (slot 0) or in slots */
static void burst(uint32_t slot) {
    rxg_txd *d = malloc(NALL * sizeof(*d));
    all_descs(d);
    uint64_t pbytes = 0, pend = 0, need = 0;
    uint32_t fit = 0;
    for (uint32_t k = 0; k < NALL; k++) {
        const uint32_t pl = d[k].kind == RXG_TXD_ARP ? 0 : d[k].pay_len;
        d[k].pay_off16 = (uint32_t)(pbytes >> 4);
        if (pl) pend = pbytes + pl;
        pbytes += (pl + 15u) & ~15u;
        const uint32_t fl = frame_len(&d[k]);
        if (slot == 0) need += up64(fl);
        else if (fl <= slot) need = (uint64_t)k * slot + up64(fl), fit++;
    }
    uint8_t *pay = malloc(pend); /* ends with the last payload's last byte */
    for (uint64_t i = 0; i < pend; i++) pay[i] = (uint8_t)(i * 13 + 5);
    /* slots: the last slot must fit whole, so the buffer runs to its end */
    const uint64_t cap = slot ? (uint64_t)NALL * slot : need;
    uint8_t *pk = malloc(cap);
    uint32_t *off = malloc(NALL * 4), tot[4];
    uint16_t *len = malloc(NALL * 2);
    uint64_t span = 0;
    const int rc = rxg_tx_encode_host(d, NALL, pay, pend, pk, cap, slot, off, len, 0, &span, tot);
    if (slot == 0) {
        CHECK(rc == RXG_OK && span == need && tot[0] == NALL && tot[3] == 0);
    } else {
        CHECK(rc == RXG_ERANGE && span == need && tot[0] == fit && tot[3] == NALL - fit);
    }
    for (uint32_t k = 0; k < NALL; k++) {
        const uint32_t fl = frame_len(&d[k]);
        if (slot && fl > slot) {
            CHECK(len[k] == 0);
            continue;
        }
        CHECK(len[k] == fl);
        if (slot) CHECK((uint64_t)off[k] * 64 == (uint64_t)k * slot);
        const uint32_t pl = d[k].kind == RXG_TXD_ARP ? 0 : d[k].pay_len;
        const uint8_t *f = pk + (uint64_t)off[k] * 64;
        CHECK(pl == 0 || memcmp(f + fl - pl, pay + (uint64_t)d[k].pay_off16 * 16, pl) == 0);
    }
    free(d), free(pay), free(pk), free(off), free(len);
}

static void skips(void) {
    rxg_txd *d = malloc(4 * sizeof(*d));
    fill_desc(&d[0], 9, 100, 0);              /* unknown kind: its payload is never read */
    d[0].pay_off16 = 0xFFFFFFFFu;
    fill_desc(&d[1], RXG_TXD_UDP, 65494, 0);  /* one byte too long */
    d[1].pay_off16 = 0xFFFFFFFFu;
    fill_desc(&d[2], RXG_TXD_TCP, 65535, 255);
    d[2].pay_off16 = 0xFFFFFFFFu;
    fill_desc(&d[3], RXG_TXD_UDP, 3, 0);
    uint8_t *pay = malloc(3), *pk = malloc(64);
    memcpy(pay, "abc", 3);
    uint32_t *off = malloc(16), tot[4];
    uint16_t *len = malloc(8);
    uint64_t span = 0;
    CHECK(rxg_tx_encode_host(d, 4, pay, 3, pk, 64, 0, off, len, 0, &span, tot) == RXG_ERANGE);
    CHECK(span == 64 && tot[0] == 1 && tot[3] == 3 && len[3] == 45 && off[3] == 0);
    CHECK(!len[0] && !len[1] && !len[2]);
    /* a payload that ends past the payload buffer is refused up front */
    CHECK(rxg_tx_encode_host(d + 3, 1, pay, 2, pk, 64, 0, off, len, 0, &span, tot) == RXG_EINVAL);
    CHECK(rxg_tx_encode_host(d + 3, 1, pay, 3, pk, 64, 96, off, len, 0, &span, tot) == RXG_EINVAL);
    CHECK(rxg_tx_encode_host(d, 0, NULL, 0, NULL, 0, 0, NULL, NULL, 0, &span, tot) == RXG_OK);
    free(d), free(pay), free(pk), free(off), free(len);
}

int main(void) {
    rxg_txd *d = malloc(NALL * sizeof(*d));
    all_descs(d);
    for (uint32_t k = 0; k < NALL; k++) {
        one(&d[k], 0);
        one(&d[k], RXG_TXE_NO_CKSUM);
    }
    free(d);
    burst(0);
    burst(1536);
    burst(64);
    skips();
    printf("TXENC SAN OK\n");
    return 0;
}
