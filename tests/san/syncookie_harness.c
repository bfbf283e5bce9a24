/* ASan + UBSan harness for the SYN cookies on the host: rxg_syncookie_host
 * (csrc/rx_syncookie_host.cpp) over the rule's named cases with every array
 * allocated at its exact size (the frame buffer ends with the last frame's
 * captured bytes, the descriptor array holds totals[0] entries), and the
 * socket layer with nstack_set_syncookies on (host/nstack.c: the host-verdict
 * path of nstack_deliver, the LISTEN handler, the SYN-ACK walk of
 * nstack_tx_burst), with the lists' generation and with it withheld (every
 * frame judged alone).  A plain executable: nothing is loaded into an
 * interpreter.  Prints SYNCOOKIE SAN OK. */
#include <arpa/inet.h>
#include <netinet/in.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/nstack.h"
#include "../../include/rxgpu.h"
#include "../../oracle/ref_cpu.h"

#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c);                   \
            exit(2);                                                                               \
        }                                                                                          \
    } while (0)

static const uint8_t MAC_L[6] = {2, 0, 0, 0, 0, 1}, MAC_P[6] = {2, 0, 0, 0, 0, 2};
static const uint8_t KEY[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
#define K0 0x0706050403020100ull
#define K1 0x0f0e0d0c0b0a0908ull
#define T0 1000u

/* Ethernet + IPv4 + TCP + payload, checksum fields 0; returns the length */
static size_t frame(uint8_t *f, uint32_t sip, uint16_t sport, uint32_t dip, uint16_t dport,
                    uint8_t flags, uint32_t seq, uint32_t ack, const void *pl, size_t pn) {
    memcpy(f, MAC_L, 6);
    memcpy(f + 6, MAC_P, 6);
    f[12] = 0x08, f[13] = 0x00;
    uint8_t *ip = f + 14;
    const uint16_t tl = (uint16_t)(40 + pn);
    memset(ip, 0, 40);
    ip[0] = 0x45, ip[8] = 64, ip[9] = 6;
    ip[2] = (uint8_t)(tl >> 8), ip[3] = (uint8_t)tl;
    memcpy(ip + 12, &sip, 4);
    memcpy(ip + 16, &dip, 4);
    uint8_t *l4 = ip + 20;
    memcpy(l4, &sport, 2);
    memcpy(l4 + 2, &dport, 2);
    const uint32_t s = htonl(seq), a = htonl(ack);
    memcpy(l4 + 4, &s, 4);
    memcpy(l4 + 8, &a, 4);
    l4[12] = 0x50, l4[13] = flags;
    l4[14] = 0xFF, l4[15] = 0xFF;
    if (pn) memcpy(l4 + 20, pl, pn);
    return 14 + tl;
}

/* ---- the rule ---------------------------------------------------------------- */
#define NC 16u
static void rule_cases(void) {
    const uint32_t L = inet_addr("192.168.0.10"), C = inet_addr("10.1.2.3");
    const uint16_t cp = htons(40000), lp = htons(8080);
    const uint32_t isn = 0xFFFFFFFFu; /* isn + 1 wraps */
    const uint32_t t = 0x100;        /* the 8-bit counter has just wrapped */
    const uint32_t ck0 = rxg_syncookie_value(K0, K1, C, L, cp, lp, isn, t);
    const uint32_t ck1 = rxg_syncookie_value(K0, K1, C, L, cp, lp, isn, 0xFF);
    const uint32_t ck3 = rxg_syncookie_value(K0, K1, C, L, cp, lp, isn, 0xFD);
    CHECK(ck0 >> 24 == 0 && ck1 >> 24 == 0xFF);
    struct {
        uint8_t flags;
        uint32_t seq, ack;
        size_t pn;
        uint32_t cap; /* 0: whole */
        uint32_t flow;
        int8_t rc;
        uint8_t cls, want;
    } cs[NC] = {
        {0x02, isn, 0, 0, 0, 3, 0, RXG_CLS_TCP, RXG_CK_SYN},
        {0x02, isn, 0, 0, 0, 2, 0, RXG_CLS_TCP, 0},            /* not a listener */
        {0x02, isn, 0, 0, 0, 3, -1, RXG_CLS_TCP, 0},           /* bad checksum */
        {0x12, isn, 0, 0, 0, 3, 0, RXG_CLS_TCP, 0},            /* SYN|ACK */
        {0x03, isn, 0, 0, 0, 3, 0, RXG_CLS_TCP, 0},            /* SYN|FIN */
        {0x04, isn, 0, 0, 0, 3, 0, RXG_CLS_TCP, 0},            /* RST */
        {0x02, isn, 0, 0, 53, 3, 0, RXG_CLS_TCP, 0},           /* a 53-byte capture */
        {0x02, isn, 0, 0, 0, 3, 0, RXG_CLS_UDP, 0},            /* another class */
        {0x02, isn, 0, 0, 0, 70, 0, RXG_CLS_TCP, 0},           /* id past the id space */
        {0x10, isn + 1, ck0 + 1, 0, 0, 3, 0, RXG_CLS_TCP, RXG_CK_ACK_OK},
        {0x10, isn + 1, ck1 + 1, 0, 0, 3, 0, RXG_CLS_TCP, RXG_CK_ACK_OK},  /* made at 0xFF */
        {0x10, isn + 1, ck3 + 1, 0, 0, 3, 0, RXG_CLS_TCP, RXG_CK_ACK_BAD}, /* max_age + 1 ago */
        {0x10, isn + 1, (ck0 ^ 0x200u) + 1, 0, 0, 3, 0, RXG_CLS_TCP, RXG_CK_ACK_BAD},
        {0x10, isn + 2, ck0 + 1, 0, 0, 3, 0, RXG_CLS_TCP, RXG_CK_ACK_BAD},
        {0x19, isn + 1, ck0 + 1, 5, 0, 3, 0, RXG_CLS_TCP, RXG_CK_ACK_OK},  /* FIN and data */
        {0x02, isn, 0, 40, 54, 69, 0, RXG_CLS_TCP, RXG_CK_SYN}, /* cut at 54; the last frame */
    };
    uint8_t f[NC][128];
    uint32_t off[NC];
    uint16_t len[NC];
    rxg_verdict v[NC];
    size_t pos = 0, end = 0;
    memset(v, 0, sizeof(v));
    for (uint32_t i = 0; i < NC; i++) {
        const size_t n = frame(f[i], C, cp, L, lp, cs[i].flags, cs[i].seq, cs[i].ack, "hello hello hello hello hello hello hello", cs[i].pn);
        off[i] = (uint32_t)(pos >> 4);
        len[i] = (uint16_t)(cs[i].cap ? cs[i].cap : n);
        end = pos + len[i];
        pos += (len[i] + 15u) & ~(size_t)15;
        v[i].cls = cs[i].cls, v[i].rc = cs[i].rc, v[i].flow_id = cs[i].flow;
    }
    uint8_t *pk = malloc(end); /* ends with the last frame's captured bytes */
    for (uint32_t i = 0; i < NC; i++) memcpy(pk + ((size_t)off[i] << 4), f[i], len[i]);
    uint32_t *lm = calloc(3, sizeof(*lm)); /* ids 0..69 */
    lm[0] = 1u << 3, lm[2] = 1u << 5;
    const rxg_ck_params p = {K0, K1, t, RXG_CK_DEFAULT_MAX_AGE, 14600, 0, 0};
    uint32_t tot[4];
    uint8_t *st = malloc(NC);
    rxg_txd *tx = malloc(NC * sizeof(*tx));
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, lm, 70, &p, st, tx, tot) == RXG_OK);
    uint32_t want[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < NC; i++) {
        CHECK(st[i] == cs[i].want);
        if (cs[i].want) want[cs[i].want - 1]++;
    }
    CHECK(tot[0] == want[0] && tot[1] == want[1] && tot[2] == want[2] && tot[3] == 0 && tot[0] == 2);
    rxg_txd *tx2 = malloc(tot[0] * sizeof(*tx2)); /* exactly totals[0] descriptors */
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, lm, 70, &p, st, tx2, tot) == RXG_OK);
    CHECK(memcmp(tx, tx2, tot[0] * sizeof(*tx)) == 0);
    CHECK(tx2[0].seq == ck0 && tx2[0].ack == 0 && tx2[0].tcp_flags == 0x12 && tx2[0].kind == RXG_TXD_TCP);
    CHECK(memcmp(tx2[0].dst_mac, MAC_P, 6) == 0 && memcmp(tx2[0].src_mac, MAC_L, 6) == 0);
    CHECK(tx2[0].sip == L && tx2[0].dip == C && tx2[0].sport == lp && tx2[0].dport == cp);
    /* no frame, no listener id, arguments */
    uint8_t *e1 = malloc(1);
    CHECK(rxg_syncookie_host(e1, (uint32_t *)e1, (uint16_t *)e1, 0, 4, (rxg_verdict *)e1, lm, 70, &p, e1,
                             (rxg_txd *)e1, tot) == RXG_OK && tot[0] + tot[1] + tot[2] == 0);
    free(e1);
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, NULL, 0, &p, st, tx, tot) == RXG_OK);
    for (uint32_t i = 0; i < NC; i++) CHECK(st[i] == 0);
    rxg_ck_params bad = p;
    bad.max_age = 256;
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, lm, 70, &bad, st, tx, tot) == RXG_EINVAL);
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, lm, 70, &p, NULL, tx, tot) == RXG_EINVAL);
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, lm, 70, &p, st, NULL, tot) == RXG_EINVAL);
    CHECK(rxg_syncookie_host(pk, off, len, NC, 4, v, lm, 70, &p, st, tx, NULL) == RXG_EINVAL);
    free(pk), free(lm), free(st), free(tx), free(tx2);
    /* the published known answers */
    uint8_t m[15];
    for (int i = 0; i < 15; i++) m[i] = (uint8_t)i;
    CHECK(rxg_siphash24(K0, K1, m, 0) == 0x726fdb47dd0e0e31ull);
    CHECK(rxg_siphash24(K0, K1, m, 15) == 0xa129ca6149be45e5ull);
}

/* ---- the socket layer ------------------------------------------------------------ */
#define NF 64u
typedef struct {
    uint8_t *buf;
    uint32_t off[NF];
    uint16_t len[NF];
    uint32_t n;
    size_t pos;
} burst;

static void push(burst *b, const uint8_t *f, size_t n) {
    CHECK(b->n < NF);
    memcpy(b->buf + b->pos, f, n);
    b->off[b->n] = (uint32_t)(b->pos >> 6);
    b->len[b->n] = (uint16_t)n;
    b->n++;
    b->pos += (n + 63) & ~(size_t)63;
}

/* checksums and verdicts by the oracle against the stack's control blocks,
 * then nstack_deliver; stale: as made for an older generation */
static void deliver(burst *b, int stale) {
    rxg_udp_sock u[8];
    rxg_tcb t[8];
    uint32_t nu = 0, nt = 0, uid[8], tid[8];
    uint64_t gen = 0;
    oracle_tx_cksum(b->buf, b->off, b->len, b->n, 6);
    CHECK(nstack_flows(u, 8, &nu, t, 8, &nt, &gen) == RXG_OK);
    oracle_tables *tb = oracle_tables_new(u, nu, t, nt);
    CHECK(tb);
    rxg_verdict v[NF];
    oracle_classify(tb, b->buf, b->off, b->len, b->n, 6, v, NULL);
    oracle_tables_free(tb);
    CHECK(nstack_flow_ids(uid, 8, tid, 8) == RXG_OK);
    rxg_mbuf mb[NF], *mp[NF];
    int rc[NF];
    memset(mb, 0, sizeof(mb));
    for (uint32_t i = 0; i < b->n; ++i) {
        if (v[i].flow_id != RXG_FLOW_NONE)
            v[i].flow_id = v[i].cls == RXG_CLS_TCP ? tid[v[i].flow_id] : uid[v[i].flow_id];
        mb[i].buf_addr = b->buf + ((size_t)b->off[i] << 6);
        mb[i].data_len = b->len[i];
        mb[i].refcnt = 1;
        mp[i] = &mb[i];
    }
    CHECK(nstack_deliver(mp, b->n, v, stale ? gen + 1 : gen, rc) >= 0);
    b->n = 0, b->pos = 0;
}

static void socket_session(int stale) {
    const uint32_t L = inet_addr("192.168.0.10");
    const uint16_t lp = htons(8080);
    uint64_t stt[4];
    CHECK(nstack_init(RXG_HOST_ONLY, 256, 1 << 20) == RXG_OK);
    CHECK(nstack_set_local(L, MAC_L) == RXG_OK);
    CHECK(nstack_set_syncookies(2, KEY) == RXG_EINVAL); /* (needs the detector) */
    CHECK(nstack_set_syncookies(1, NULL) == RXG_EINVAL);
    CHECK(nstack_syncookie_tick(T0) == RXG_OK);
    CHECK(nstack_set_syncookies(1, KEY) == RXG_OK);     /* before the listener exists */
    const int ls = nsocket(AF_INET, SOCK_STREAM, 0);
    struct sockaddr_in a = {.sin_family = AF_INET, .sin_port = lp, .sin_addr.s_addr = L};
    CHECK(nbind(ls, (struct sockaddr *)&a, sizeof a) == 0 && nlisten(ls, 16) == 0);
    burst b = {.buf = calloc(NF, 128), .n = 0, .pos = 0};
    uint8_t f[128];
    const uint32_t NS = 40;
    for (uint32_t i = 0; i < NS; i++)
        push(&b, f, frame(f, htonl(0x0A000001u + i), htons((uint16_t)(2000 + i)), L, lp, 0x02, 100 * i, 0, NULL, 0));
    deliver(&b, stale);
    CHECK(nstack_tcb_count() == 1);
    CHECK(nstack_syncookie_stats(stt) == RXG_OK && stt[0] == NS && stt[1] == 0 && stt[2] == 0);
    /* the SYN-ACKs: fewer frames than wait, then the rest */
    uint8_t *out = malloc(NS * 64);
    uint32_t *ooff = malloc(NS * sizeof(*ooff));
    uint16_t *olen = malloc(NS * sizeof(*olen));
    uint64_t span = 0;
    CHECK(nstack_tx_burst(out, NS * 64, ooff, olen, 10, 0, &span) == 10 && span == 640);
    CHECK(nstack_tx_burst(out + 640, 5 * 64, ooff + 10, olen + 10, NS, 0, &span) == 5 && span == 320);
    CHECK(nstack_tx_burst(out + 960, (NS - 15) * 64, ooff + 15, olen + 15, NS, 0, &span) == (int)NS - 15);
    CHECK(nstack_tx_burst(out, NS * 64, ooff, olen, NS, 0, &span) == 0);
    uint32_t cookie7 = 0;
    for (uint32_t i = 0; i < NS; i++) {
        const uint8_t *q = out + 64 * i;
        const uint32_t sip = htonl(0x0A000001u + i);
        const uint16_t sp = htons((uint16_t)(2000 + i));
        uint32_t seq, ack;
        memcpy(&seq, q + 38, 4), memcpy(&ack, q + 42, 4);
        CHECK(olen[i] == 54 && q[47] == 0x12 && memcmp(q, MAC_P, 6) == 0 && memcmp(q + 6, MAC_L, 6) == 0);
        CHECK(ntohl(seq) == rxg_syncookie_value(K0, K1, sip, L, sp, lp, 100 * i, T0) && ntohl(ack) == 100 * i + 1);
        if (i == 7) cookie7 = ntohl(seq);
    }
    free(out), free(ooff), free(olen);
    /* a forged ACK, client 7's ACK with data, a stale one */
    const uint32_t c7 = htonl(0x0A000008u);
    const uint16_t p7 = htons(2007);
    push(&b, f, frame(f, c7, p7, L, lp, 0x10, 701, cookie7 + 3, NULL, 0));
    push(&b, f, frame(f, c7, p7, L, lp, 0x18, 701, cookie7 + 1, "hello", 5));
    push(&b, f, frame(f, htonl(0x0A000009u), htons(2008), L, lp, 0x10, 801,
                      rxg_syncookie_value(K0, K1, htonl(0x0A000009u), L, htons(2008), lp, 800, T0 - 3) + 1, NULL, 0));
    deliver(&b, stale);
    CHECK(nstack_tcb_count() == 2);
    CHECK(nstack_syncookie_stats(stt) == RXG_OK && stt[0] == NS && stt[1] == 1 && stt[2] == 2);
    struct sockaddr_in peer;
    socklen_t pl = sizeof peer;
    const int cs = naccept(ls, (struct sockaddr *)&peer, &pl);
    CHECK(cs > ls && peer.sin_port == p7 && peer.sin_addr.s_addr == c7);
    char got[64];
    CHECK(nrecv(cs, got, sizeof got, MSG_DONTWAIT) == 5 && memcmp(got, "hello", 5) == 0);
    push(&b, f, frame(f, c7, p7, L, lp, 0x11, 706, cookie7 + 1, NULL, 0));
    deliver(&b, stale);
    CHECK(nrecv(cs, got, sizeof got, MSG_DONTWAIT) == 0); /* EOF */
    int32_t s1, fd1;
    uint32_t rn1, sn1;
    CHECK(nstack_tcb_state(c7, L, p7, lp, &s1, &rn1, &sn1, &fd1) == 0 && rn1 == 707 && sn1 == cookie7 + 1);
    /* off again: a SYN makes a tcb, the listener's close resets nothing else */
    CHECK(nstack_set_syncookies(0, NULL) == RXG_OK);
    push(&b, f, frame(f, htonl(0x0A000063u), htons(9), L, lp, 0x02, 5, 0, NULL, 0));
    deliver(&b, stale);
    CHECK(nstack_tcb_count() == 3);
    CHECK(nstack_set_syncookies(1, KEY) == RXG_OK);
    CHECK(nclose(ls) == 0);
    push(&b, f, frame(f, htonl(0x0A000064u), htons(9), L, lp, 0x02, 5, 0, NULL, 0));
    deliver(&b, stale);
    CHECK(nstack_syncookie_stats(stt) == RXG_OK && stt[0] == NS);
    free(b.buf);
    nstack_fini();
    CHECK(nstack_syncookie_stats(stt) == RXG_OK && stt[0] == 0 && stt[1] == 0 && stt[2] == 0);
}

int main(void) {
    rule_cases();
    socket_session(0);
    socket_session(1);
    printf("SYNCOOKIE SAN OK\n");
    return 0;
}
