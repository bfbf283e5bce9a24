/* AddressSanitizer / UBSan harness for TCP sequence ordering on the host: the
 * rule's restatement (csrc/rx_order_host.cpp, rxg_tcp_order_host) and the
 * socket layer with nstack_set_rx_order on (host/nstack.c, the host-verdict
 * path of nstack_deliver).  A stand-alone program: compiled with
 * -fsanitize=address,undefined together with those sources and the oracle's
 * and run directly (tests/test_rx_order.py).  The rule's arrays are heap
 * allocations of exactly nseg entries, so one record, source address or
 * permutation entry read or written past them is a report:
 *   - the rule cases: a swap across the seq wrap, equal seq (pure ACK, data,
 *     duplicate), a SYN and a RST as barriers, two sources A, B, A on one id, a
 *     FIN before the last data, distances that differ in each key byte and
 *     negative ones, a group of one, nseg = 0, NULL arguments;
 *   - one socket session beside oracle/ref_stack.c: the oracle takes two
 *     bursts in order, nstack the same bursts permuted (a reversed train; a
 *     FIN that overtook the data before it), with the option alone and with
 *     coalescing; the bytes read, the EOF's place, rcv_nxt and the state agree.
 */
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

/* ---- the rule ---------------------------------------------------------------- */
typedef struct {
    rxg_segment *seg;
    uint32_t *sip, n, cap;
} recs;

static void rec(recs *r, uint32_t flow, uint32_t sip, uint32_t seq, uint8_t flags) {
    CHECK(r->n < r->cap);
    rxg_segment *g = &r->seg[r->n];
    memset(g, 0, sizeof(*g));
    g->frame = r->n, g->flow = flow, g->seq = seq, g->ack = 7, g->plen = 10;
    g->sport = 0x409C, g->dport = 0x0F27, g->flags = flags, g->hl = 5;
    r->sip[r->n++] = sip;
}

static void rule_cases(void) {
    recs r = {NULL, NULL, 0, 0};
    for (int pass = 0; pass < 2; pass++) { /* count, then fill exact-size arrays */
        r.cap = pass ? r.n : 256, r.n = 0;
        r.seg = malloc(r.cap * sizeof(*r.seg));
        r.sip = malloc(r.cap * sizeof(*r.sip));
        const uint32_t A = 0x0100000Au, B = 0x0200000Au;
        rec(&r, 0, A, 0x00000100u, 0x18), rec(&r, 0, A, 0xFFFFFF00u, 0x18);
        rec(&r, 1, A, 1100, 0x18), rec(&r, 1, A, 1000, 0x10), rec(&r, 1, A, 1000, 0x18);
        rec(&r, 1, A, 1000, 0x18);
        for (uint32_t k = 2; k < 4; k++) {
            rec(&r, k, A, 1200, 0x18), rec(&r, k, A, 1100, 0x18);
            rec(&r, k, A, 5, k == 2 ? 0x02 : 0x04);
            rec(&r, k, A, 1400, 0x18), rec(&r, k, A, 1300, 0x18);
        }
        rec(&r, 4, A, 1000, 0x18), rec(&r, 4, A, 1200, 0x11), rec(&r, 4, A, 1100, 0x18);
        rec(&r, 5, A, 300, 0x10), rec(&r, 5, B, 100, 0x10), rec(&r, 5, A, 200, 0x10);
        static const int32_t d[10] = {0, 0x01000000, 0x00010000, 0x00000100, 1,
                                      -1, -0x100, -0x10000, -0x1000000, 2};
        for (uint32_t q = 0; q < 10; q++) rec(&r, 6, A, 0x40000000u + (uint32_t)d[q], 0x18);
        rec(&r, 7, A, 777, 0x18);
        if (!pass) free(r.seg), free(r.sip);
    }
    static const uint32_t want[] = {1, 0,  3, 4, 5, 2,  7, 6, 8, 10, 9,  12, 11, 13, 15, 14,
                                    16, 18, 17,  19, 20, 21,
                                    30, 29, 28, 27, 22, 26, 31, 25, 24, 23,  32};
    CHECK(r.n == sizeof(want) / sizeof(want[0]));
    uint32_t *perm = malloc(r.n * sizeof(*perm)), moved = 77, wmoved = 0;
    CHECK(rxg_tcp_order_host(r.seg, r.sip, r.n, perm, &moved) == RXG_OK);
    for (uint32_t k = 0; k < r.n; k++) {
        CHECK(perm[k] == want[k]);
        wmoved += want[k] != k;
    }
    CHECK(moved == wmoved);
    /* nseg = 0 with arrays of no entries; NULL arguments */
    rxg_segment *s0 = malloc(1);
    uint32_t *p0 = malloc(1), *q0 = malloc(1);
    moved = 77;
    CHECK(rxg_tcp_order_host(s0, q0, 0, p0, &moved) == RXG_OK && moved == 0);
    free(s0), free(p0), free(q0);
    CHECK(rxg_tcp_order_host(NULL, r.sip, r.n, perm, &moved) == RXG_EINVAL);
    CHECK(rxg_tcp_order_host(r.seg, NULL, r.n, perm, &moved) == RXG_EINVAL);
    CHECK(rxg_tcp_order_host(r.seg, r.sip, r.n, NULL, &moved) == RXG_EINVAL);
    CHECK(rxg_tcp_order_host(r.seg, r.sip, r.n, perm, NULL) == RXG_EINVAL);
    free(perm), free(r.seg), free(r.sip);
}

/* ---- one socket session ---------------------------------------------------------- */
static const uint8_t MAC_A[6] = {2, 0, 0, 0, 0, 1}, MAC_B[6] = {2, 0, 0, 0, 0, 2};
#define NF 40u

/* Ethernet + IPv4 + TCP + payload; checksums by the oracle */
static size_t frame(uint8_t *f, uint32_t sip, uint16_t sport, uint32_t dip, uint16_t dport,
                    uint8_t flags, uint32_t seq, uint32_t ack, const void *pl, size_t pn) {
    memcpy(f, MAC_B, 6);
    memcpy(f + 6, MAC_A, 6);
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

/* oracle verdicts against the stack's control blocks, then nstack_deliver of
 * the frames in the order p (frame p[i] at position i) */
static void deliver(const burst *b, const uint32_t *p, int *rc) {
    rxg_udp_sock u[8];
    rxg_tcb t[8];
    uint32_t nu = 0, nt = 0, uid[8], tid[8];
    uint64_t gen = 0;
    CHECK(nstack_flows(u, 8, &nu, t, 8, &nt, &gen) == RXG_OK);
    oracle_tables *tb = oracle_tables_new(u, nu, t, nt);
    CHECK(tb);
    rxg_verdict v[NF], vp[NF];
    oracle_classify(tb, b->buf, b->off, b->len, b->n, 6, v, NULL);
    oracle_tables_free(tb);
    CHECK(nstack_flow_ids(uid, 8, tid, 8) == RXG_OK);
    rxg_mbuf mb[NF], *mp[NF];
    memset(mb, 0, sizeof(mb));
    for (uint32_t i = 0; i < b->n; ++i) {
        vp[i] = v[p[i]];
        if (vp[i].flow_id != RXG_FLOW_NONE)
            vp[i].flow_id = vp[i].cls == RXG_CLS_TCP ? tid[vp[i].flow_id] : uid[vp[i].flow_id];
        mb[i].buf_addr = b->buf + ((size_t)b->off[p[i]] << 6);
        mb[i].data_len = b->len[p[i]];
        mb[i].refcnt = 1;
        mp[i] = &mb[i];
    }
    CHECK(nstack_deliver(mp, b->n, vp, gen, rc) >= 0);
}

static void socket_session(uint32_t W) {
    const uint32_t L = inet_addr("192.168.100.77"), C = inet_addr("10.0.0.1");
    const uint16_t cp = htons(40000), lp = htons(9999);
    CHECK(nstack_init(RXG_HOST_ONLY, 256, 1 << 20) == RXG_OK);
    CHECK(nstack_set_local(L, MAC_A) == RXG_OK);
    CHECK(nstack_set_rx_order(1) == RXG_OK);
    CHECK(nstack_set_rx_inplace(1, NULL, NULL) == RXG_OK); /* ordering goes with in-place ... */
    CHECK(nstack_set_rx_inplace(0, NULL, NULL) == RXG_OK);
    CHECK(nstack_set_rx_gro(W) == RXG_OK);                 /* ... and with coalescing */
    oracle_stack *st = oracle_stack_new();
    const int ls = nsocket(AF_INET, SOCK_STREAM, 0);
    CHECK(ls == oracle_nsocket(st, 1));
    struct sockaddr_in a = {.sin_family = AF_INET, .sin_port = lp, .sin_addr.s_addr = L};
    CHECK(nbind(ls, (struct sockaddr *)&a, sizeof a) == 0 && oracle_nbind(st, ls, L, lp) == 0);
    CHECK(nlisten(ls, 16) == 0 && oracle_nlisten(st, ls) == 0);
    CHECK(nstack_tcb_add(C, L, cp, lp, 4) == 0 && oracle_tcb_add(st, C, L, cp, lp, 4) == 0);
    struct sockaddr_in peer;
    socklen_t pl2 = sizeof peer;
    uint32_t osip;
    uint16_t osport;
    const int cs = naccept(ls, (struct sockaddr *)&peer, &pl2);
    CHECK(cs >= 0 && cs == oracle_naccept(st, ls, &osip, &osport));
    /* burst 0: a train of 9 across the seq wrap, reversed; burst 1: a train of
     * 4 and a FIN, the FIN first and the train rotated */
    static const uint32_t lens[2][9] = {{1460, 1460, 1, 7, 100, 600, 1460, 16, 17}, {600, 1, 1460, 9, 0}};
    static const uint32_t perm[2][9] = {{8, 7, 6, 5, 4, 3, 2, 1, 0}, {4, 2, 3, 0, 1}};
    static const uint32_t cnt[2] = {9, 5};
    uint8_t pay[1460], f[1600], *got = malloc(1 << 16), *want = malloc(1 << 16);
    uint32_t seq = 0xFFFFF000u, frags_ns = 0, frags_os = 0, moved = 0;
    size_t ngot = 0, nwant = 0;
    for (int bi = 0; bi < 2; bi++) {
        burst b = {.buf = calloc(NF, 1600), .n = 0, .pos = 0};
        for (uint32_t i = 0; i < cnt[bi]; i++) {
            for (uint32_t q = 0; q < lens[bi][i]; q++) pay[q] = (uint8_t)(seq + 31u * q + i);
            const uint8_t fl = (bi == 1 && i == 4) ? 0x11 : 0x18;
            push(&b, f, frame(f, C, cp, L, lp, fl, seq, 2000, pay, lens[bi][i]));
            seq += lens[bi][i] + (fl == 0x11);
        }
        oracle_tx_cksum(b.buf, b.off, b.len, b.n, 6);
        int rc[NF];
        deliver(&b, perm[bi], rc);
        for (uint32_t i = 0; i < b.n; i++) { /* the oracle in order; rcs matched by frame */
            const int w = oracle_rx(st, b.buf + ((size_t)b.off[i] << 6), b.len[i]);
            for (uint32_t k = 0; k < b.n; k++)
                if (perm[bi][k] == i) CHECK(rc[k] == w);
            moved += perm[bi][i] != i;
        }
        free(b.buf);
        for (;;) { /* every fragment, a read each: the byte streams agree, EOF included */
            const ssize_t r = nrecv(cs, got + ngot, 8192, MSG_DONTWAIT);
            if (r < 0) break;
            ngot += (size_t)r, frags_ns++;
            if (r == 0) got[ngot++] = 0xEF; /* (an EOF's place in the stream) */
        }
        for (;;) {
            const long r = oracle_nrecv(st, cs, want + nwant, 8192);
            if (r < 0) break;
            nwant += (size_t)r, frags_os++;
            if (r == 0) want[nwant++] = 0xEF;
        }
        CHECK(ngot == nwant && memcmp(got, want, ngot) == 0);
    }
    CHECK(nstack_stat(16) == moved && moved == 8 + 5);
    CHECK(W ? frags_ns < frags_os : frags_ns == frags_os);
    CHECK(nstack_stat(15) == frags_os - frags_ns);
    int32_t s1, s2, fd1, fd2;
    uint32_t rn1, rn2, sn1, sn2;
    CHECK(nstack_tcb_state(C, L, cp, lp, &s1, &rn1, &sn1, &fd1) == 0);
    CHECK(oracle_tcb_state(st, C, L, cp, lp, &s2, &rn2, &sn2, &fd2) >= 0);
    CHECK(s1 == s2 && rn1 == rn2 && sn1 == sn2 && fd1 == fd2);
    CHECK(nclose(cs) == 0 && nclose(ls) == 0);
    oracle_stack_free(st);
    free(got), free(want);
    nstack_fini();
}

int main(void) {
    rule_cases();
    socket_session(0);
    socket_session(3000);
    printf("ORDER SAN OK\n");
    return 0;
}
