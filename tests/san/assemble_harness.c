/* AddressSanitizer / UBSan harness for TCP stream assembly on the host: the
 * rule's restatement (csrc/rx_assemble_host.cpp, rxg_tcp_assemble_host) and
 * the socket layer with nstack_set_rx_assemble on (host/nstack.c: the
 * host-verdict path of nstack_deliver, the stream form of deliver_tcp_conn and
 * the single-frame rule of tcp_dispatch).  A stand-alone program: compiled
 * with -fsanitize=address,undefined together with those sources and the
 * oracle's and run directly (tests/test_rx_assemble.py).  The rule's arrays
 * are heap allocations of exactly nseg entries, so one record, stream or
 * offset read or written past them is a report:
 *   - the rule cases: a duplicate, an overlap, a contained segment, a hole,
 *     data + FIN and a duplicate FIN, a cut capture, a SYN barrier, two
 *     sources on one id, nseg = 0, NULL arguments;
 *   - one socket session beside oracle/ref_stack.c: the oracle takes the byte
 *     stream clean, nstack takes it dirty (data without PSH, a duplicate, an
 *     overlap, a lost segment retransmitted re-cut in the next burst, a FIN
 *     twice, permuted), once through the sorted path and once frame by frame
 *     (verdicts of an older generation); the bytes read, the EOF's place,
 *     rcv_nxt and the state agree.
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
    uint32_t *sip, *avail, n, cap;
} recs;

static void rec(recs *r, uint32_t flow, uint32_t sip, uint32_t seq, int32_t plen, uint8_t flags,
                uint32_t avail) {
    CHECK(r->n < r->cap);
    rxg_segment *g = &r->seg[r->n];
    memset(g, 0, sizeof(*g));
    g->frame = r->n, g->flow = flow, g->seq = seq, g->ack = 7 + r->n, g->plen = plen;
    g->sport = 0x409C, g->dport = 0x0F27, g->flags = flags, g->hl = 5;
    r->avail[r->n] = avail;
    r->sip[r->n++] = sip;
}

static void rule_cases(void) {
    recs r = {NULL, NULL, NULL, 0, 0};
    for (int pass = 0; pass < 2; pass++) { /* count, then fill exact-size arrays */
        r.cap = pass ? r.n : 256, r.n = 0;
        r.seg = malloc(r.cap * sizeof(*r.seg));
        r.sip = malloc(r.cap * sizeof(*r.sip));
        r.avail = malloc(r.cap * sizeof(*r.avail));
        const uint32_t A = 0x0100000Au, B = 0x0200000Au;
        rec(&r, 0, A, 0xFFFFFFC0u, 100, 0x18, 100), rec(&r, 0, A, 0xFFFFFFC0u, 100, 0x18, 100);
        rec(&r, 0, A, 0x24, 100, 0x10, 100);                      /* duplicate; no PSH; the wrap */
        rec(&r, 1, A, 1000, 300, 0x18, 300), rec(&r, 1, A, 1050, 100, 0x18, 100);
        rec(&r, 1, A, 1250, 100, 0x18, 100), rec(&r, 1, A, 1400, 10, 0x18, 10); /* contained, overlap, hole */
        rec(&r, 2, A, 1000, 100, 0x18, 100), rec(&r, 2, A, 1100, 50, 0x19, 50);
        rec(&r, 2, A, 1150, 0, 0x11, 0);                          /* data + FIN, the FIN again */
        rec(&r, 3, A, 1000, 100, 0x18, 100), rec(&r, 3, A, 1100, 100, 0x19, 70);
        rec(&r, 3, A, 1200, 100, 0x18, 100);                      /* a cut capture: nothing, no FIN */
        rec(&r, 4, A, 1000, 100, 0x18, 100), rec(&r, 4, A, 5, 20, 0x02, 20);
        rec(&r, 4, A, 1100, 100, 0x18, 100);                      /* a SYN barrier */
        rec(&r, 5, A, 1000, 100, 0x10, 100), rec(&r, 5, B, 1100, 100, 0x10, 100);
        rec(&r, 5, A, 1100, 100, 0x10, 100);                      /* two sources on one id */
        rec(&r, 6, A, 1000, -12, 0x10, 0);                        /* plen < 0 */
        if (!pass) free(r.seg), free(r.sip), free(r.avail);
    }
    static const uint32_t wtake[] = {100, 0, 100, 300, 0, 50, 10, 100, 50, 0, 100, 0, 100,
                                     100, 0, 100, 100, 100, 100, 0};
    static const uint32_t wst[][4] = { /* seq, bytes, flags, nseg */
        {0xFFFFFFC0u, 200, 0, 3}, {1000, 350, 0, 3}, {1400, 10, RXG_STREAM_HOLE, 1},
        {1000, 150, RXG_STREAM_FIN, 2}, {1150, 0, RXG_STREAM_FIN, 1},
        {1000, 100, 0, 2}, {1200, 100, RXG_STREAM_HOLE, 1},
        {1000, 100, 0, 1}, {5, 0, 0, 1}, {1100, 100, 0, 1},
        {1000, 100, 0, 1}, {1100, 100, 0, 1}, {1100, 100, 0, 1}, {1000, 0, 0, 1}};
    const uint32_t nw = sizeof(wst) / sizeof(wst[0]);
    CHECK(r.n == sizeof(wtake) / sizeof(wtake[0]));
    rxg_tcp_stream *st = malloc(r.n * sizeof(*st));
    uint32_t *skip = malloc(r.n * 4), *take = malloc(r.n * 4), *dst = malloc(r.n * 4), ns = 77;
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, r.avail, r.n, st, &ns, skip, take, dst) == RXG_OK);
    CHECK(ns == nw);
    uint32_t where = 0, first = 0;
    for (uint32_t q = 0; q < ns; q++) {
        CHECK(st[q].seq == wst[q][0] && st[q].bytes == wst[q][1] && st[q].flags == wst[q][2]);
        CHECK(st[q].nseg == wst[q][3] && st[q].first == first && st[q].offset == where);
        CHECK(st[q].ack == r.seg[first + st[q].nseg - 1].ack && st[q].reserved == 0);
        uint32_t sum = 0;
        for (uint32_t j = first; j < first + st[q].nseg; j++) {
            CHECK(dst[j] == where + sum);
            sum += take[j];
        }
        CHECK(sum == st[q].bytes);
        first += st[q].nseg;
        where += (st[q].bytes + 15u) & ~15u;
    }
    for (uint32_t j = 0; j < r.n; j++) {
        CHECK(take[j] == wtake[j]);
        const int usable = r.seg[j].plen <= 0 || r.avail[j] >= (uint32_t)r.seg[j].plen;
        const uint32_t dlen = usable && r.seg[j].plen > 0 && !(r.seg[j].flags & 0x06) ? (uint32_t)r.seg[j].plen : 0;
        CHECK(skip[j] + take[j] == dlen);
    }
    /* nseg = 0 with arrays of no entries; NULL arguments */
    rxg_segment *s0 = malloc(1);
    rxg_tcp_stream *t0 = malloc(1);
    uint32_t *p0 = malloc(1), *q0 = malloc(1), *a0 = malloc(1), *b0 = malloc(1), *c0 = malloc(1);
    ns = 77;
    CHECK(rxg_tcp_assemble_host(s0, p0, q0, 0, t0, &ns, a0, b0, c0) == RXG_OK && ns == 0);
    free(s0), free(t0), free(p0), free(q0), free(a0), free(b0), free(c0);
    CHECK(rxg_tcp_assemble_host(NULL, r.sip, r.avail, r.n, st, &ns, skip, take, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, NULL, r.avail, r.n, st, &ns, skip, take, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, NULL, r.n, st, &ns, skip, take, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, r.avail, r.n, NULL, &ns, skip, take, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, r.avail, r.n, st, NULL, skip, take, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, r.avail, r.n, st, &ns, NULL, take, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, r.avail, r.n, st, &ns, skip, NULL, dst) == RXG_EINVAL);
    CHECK(rxg_tcp_assemble_host(r.seg, r.sip, r.avail, r.n, st, &ns, skip, take, NULL) == RXG_EINVAL);
    free(st), free(skip), free(take), free(dst), free(r.seg), free(r.sip), free(r.avail);
}

/* ---- one socket session ---------------------------------------------------------- */
static const uint8_t MAC_A[6] = {2, 0, 0, 0, 0, 1}, MAC_B[6] = {2, 0, 0, 0, 0, 2};
#define NF 16u

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
 * the frames in the order p (frame p[i] at position i); stale: the verdicts
 * are handed over as made for an older generation (frame by frame) */
static void deliver(const burst *b, const uint32_t *p, int stale) {
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
    int rc[NF];
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
    CHECK(nstack_deliver(mp, b->n, vp, stale ? gen + 1 : gen, rc) >= 0);
}

static void socket_session(int stale) {
    const uint32_t L = inet_addr("192.168.100.77"), C = inet_addr("10.0.0.1");
    const uint16_t cp = htons(40000), lp = htons(9999);
    CHECK(nstack_init(RXG_HOST_ONLY, 256, 1 << 20) == RXG_OK);
    CHECK(nstack_set_local(L, MAC_A) == RXG_OK);
    CHECK(nstack_set_rx_assemble(1) == RXG_OK);
    CHECK(nstack_set_rx_gro(65536) == RXG_EINVAL);            /* excluded both ways */
    CHECK(nstack_set_rx_inplace(1, NULL, NULL) == RXG_EINVAL);
    oracle_stack *st = oracle_stack_new();
    const int ls = nsocket(AF_INET, SOCK_STREAM, 0);
    CHECK(ls == oracle_nsocket(st, 1));
    struct sockaddr_in a = {.sin_family = AF_INET, .sin_port = lp, .sin_addr.s_addr = L};
    CHECK(nbind(ls, (struct sockaddr *)&a, sizeof a) == 0 && oracle_nbind(st, ls, L, lp) == 0);
    CHECK(nlisten(ls, 16) == 0 && oracle_nlisten(st, ls) == 0);
    const uint32_t isn = 0xFFFFF7FFu; /* the data crosses the seq wrap */
    const uint32_t d0 = isn + 1;
    static const uint32_t ident[NF] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    uint8_t f[1600], data[3600], *got = malloc(1 << 14), *want = malloc(1 << 14);
    for (uint32_t q = 0; q < sizeof(data); q++) data[q] = (uint8_t)(q * 7u + (q >> 8));
    { /* the handshake, frame by frame on both sides */
        burst b = {.buf = calloc(NF, 1600), .n = 0, .pos = 0};
        push(&b, f, frame(f, C, cp, L, lp, 0x02, isn, 0, NULL, 0));
        push(&b, f, frame(f, C, cp, L, lp, 0x10, d0, 2000, NULL, 0));
        oracle_tx_cksum(b.buf, b.off, b.len, b.n, 6);
        deliver(&b, ident, 0);
        for (uint32_t i = 0; i < b.n; i++) oracle_rx(st, b.buf + ((size_t)b.off[i] << 6), b.len[i]);
        free(b.buf);
    }
    struct sockaddr_in peer;
    socklen_t pl2 = sizeof peer;
    uint32_t osip;
    uint16_t osport;
    const int cs = naccept(ls, (struct sockaddr *)&peer, &pl2);
    CHECK(cs >= 0 && cs == oracle_naccept(st, ls, &osip, &osport));
    /* dirty: {from, to, flags}; burst 0 loses [2000, 3000), burst 1 brings it re-cut */
    static const uint32_t dirty[2][5][3] = {
        {{0, 1000, 0x10}, {1000, 2000, 0x18}, {1000, 2000, 0x18}, {500, 1500, 0x18}, {3000, 3500, 0x18}},
        {{1800, 3200, 0x18}, {3200, 3500, 0x10}, {3500, 3600, 0x19}, {3600, 3600, 0x11}, {0, 100, 0x18}}};
    static const uint32_t perm[2][5] = {{4, 2, 0, 3, 1}, {3, 1, 4, 0, 2}};
    /* clean: what the oracle gets after each burst */
    static const uint32_t clean[2][3][3] = {{{0, 1460, 0x18}, {1460, 2000, 0x18}, {0, 0, 0}},
                                            {{2000, 3460, 0x18}, {3460, 3600, 0x18}, {3600, 3600, 0x11}}};
    size_t ngot = 0, nwant = 0;
    for (int bi = 0; bi < 2; bi++) {
        burst b = {.buf = calloc(NF, 1600), .n = 0, .pos = 0};
        for (uint32_t i = 0; i < 5; i++) {
            const uint32_t *x = dirty[bi][i];
            push(&b, f, frame(f, C, cp, L, lp, (uint8_t)x[2], d0 + x[0], 2000, data + x[0], x[1] - x[0]));
        }
        oracle_tx_cksum(b.buf, b.off, b.len, b.n, 6);
        deliver(&b, stale ? ident : perm[bi], stale);
        free(b.buf);
        burst c = {.buf = calloc(NF, 1600), .n = 0, .pos = 0};
        for (uint32_t i = 0; i < 3; i++) {
            const uint32_t *x = clean[bi][i];
            if (!x[2]) continue;
            push(&c, f, frame(f, C, cp, L, lp, (uint8_t)x[2], d0 + x[0], 2000, data + x[0], x[1] - x[0]));
        }
        oracle_tx_cksum(c.buf, c.off, c.len, c.n, 6);
        for (uint32_t i = 0; i < c.n; i++) oracle_rx(st, c.buf + ((size_t)c.off[i] << 6), c.len[i]);
        free(c.buf);
        for (;;) {
            const ssize_t r = nrecv(cs, got + ngot, 8192, MSG_DONTWAIT);
            if (r < 0) break;
            ngot += (size_t)r;
            if (r == 0) got[ngot++] = 0xEF; /* (an EOF's place in the stream) */
        }
        for (;;) {
            const long r = oracle_nrecv(st, cs, want + nwant, 8192);
            if (r < 0) break;
            nwant += (size_t)r;
            if (r == 0) want[nwant++] = 0xEF;
        }
        CHECK(ngot == nwant && memcmp(got, want, ngot) == 0);
        CHECK(ngot == (bi ? 3601u : 2000u));
    }
    CHECK(memcmp(got, data, 3600) == 0);
    /* [1000, 2000) again, [500, 1500), [1800, 2000), and [0, 100) (frame by frame
     * it comes after the FIN and is not looked at); the stream at 3000 */
    CHECK(nstack_stat(19) == 1000 + 1000 + 200 + (stale ? 0u : 100u) && nstack_stat(20) == 1);
    int32_t s1, s2, fd1, fd2;
    uint32_t rn1, rn2, sn1, sn2;
    CHECK(nstack_tcb_state(C, L, cp, lp, &s1, &rn1, &sn1, &fd1) == 0);
    CHECK(oracle_tcb_state(st, C, L, cp, lp, &s2, &rn2, &sn2, &fd2) >= 0);
    CHECK(s1 == s2 && rn1 == rn2 && rn1 == d0 + 3601u && sn1 == sn2 && fd1 == fd2);
    CHECK(nclose(cs) == 0 && nclose(ls) == 0);
    oracle_stack_free(st);
    free(got), free(want);
    nstack_fini();
}

int main(void) {
    rule_cases();
    socket_session(0);
    socket_session(1);
    printf("ASSEMBLE SAN OK\n");
    return 0;
}
