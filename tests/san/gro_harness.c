/* AddressSanitizer / UBSan harness for TCP receive coalescing on the host:
 * the rule's restatement (csrc/rx_gro_host.cpp, rxg_tcp_runs_host) and the
 * socket layer with nstack_set_rx_gro on (host/nstack.c, the host-verdict path
 * of nstack_deliver).  A stand-alone program: compiled with
 * -fsanitize=address,undefined together with those sources and the oracle's
 * and run directly (tests/test_rx_gro.py).  The rule's arrays are heap
 * allocations of exactly nseg entries, so one record, source address or run
 * read or written past them is a report:
 *   - the rule cases: a chain whose seq wraps 2^32, a differing ack, a
 *     duplicate seq, out-of-order segments, hl = 6, flags 0x10 / 0x19 / 0x11,
 *     plen = 0, a capture cut mid-payload, two sources on one id, W = 1, W =
 *     one payload, W hit at a record boundary, nseg = 0, a refused W;
 *   - one socket session beside oracle/ref_stack.c: trains of in-sequence
 *     PSH|ACK segments, an options segment and a FIN between them, runs made
 *     into single fragments; the bytes read, rcv_nxt and the state agree.
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

static void rec(recs *r, uint32_t flow, uint32_t sip, uint32_t seq, uint32_t ack, int32_t plen,
                uint8_t flags, uint8_t hl, uint32_t cut) {
    CHECK(r->n < r->cap);
    rxg_segment *g = &r->seg[r->n];
    memset(g, 0, sizeof(*g));
    g->frame = r->n, g->flow = flow, g->seq = seq, g->ack = ack, g->plen = plen;
    g->sport = 0x409C, g->dport = 0x0F27, g->flags = flags, g->hl = hl;
    g->ncopy = (flags & 0x08) && plen > 0 ? (uint16_t)(plen - (int32_t)cut) : 0;
    g->offset = 0xDEAD0000u + r->n; /* (never read, never written) */
    r->sip[r->n++] = sip;
}

/* the runs' record counts of one flow, as a string of digits */
static void split(const recs *r, const rxg_tcp_run *run, uint32_t nrun, uint32_t flow, char *out) {
    for (uint32_t k = 0; k < nrun; k++)
        if (r->seg[run[k].first].flow == flow) *out++ = (char)('0' + run[k].nseg);
    *out = 0;
}

static void rule_cases(void) {
    recs r = {NULL, NULL, 0, 0};
    for (int pass = 0; pass < 2; pass++) { /* count, then fill exact-size arrays */
        if (pass) {
            r.cap = r.n, r.n = 0;
            r.seg = malloc(r.cap * sizeof(*r.seg));
            r.sip = malloc(r.cap * sizeof(*r.sip));
        } else {
            r.cap = 256;
            r.seg = malloc(r.cap * sizeof(*r.seg));
            r.sip = malloc(r.cap * sizeof(*r.sip));
        }
        const uint32_t A = 0x0100000Au, B = 0x0200000Au;
        for (uint32_t q = 0; q < 3; q++) rec(&r, 0, A, 0xFFFFFF6Au + 100u * q, 7, 100, 0x18, 5, 0);
        rec(&r, 1, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 1, A, 1100, 8, 100, 0x18, 5, 0);
        rec(&r, 1, A, 1200, 8, 100, 0x18, 5, 0);
        rec(&r, 2, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 2, A, 1000, 7, 100, 0x18, 5, 0);
        rec(&r, 2, A, 1100, 7, 100, 0x18, 5, 0);
        rec(&r, 3, A, 1100, 7, 100, 0x18, 5, 0), rec(&r, 3, A, 1000, 7, 100, 0x18, 5, 0);
        rec(&r, 3, A, 1200, 7, 100, 0x18, 5, 0);
        rec(&r, 4, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 4, A, 1100, 7, 100, 0x18, 6, 0);
        rec(&r, 4, A, 1200, 7, 100, 0x18, 5, 0), rec(&r, 4, A, 1300, 7, 100, 0x18, 5, 0);
        rec(&r, 5, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 5, A, 1100, 7, 100, 0x10, 5, 0);
        rec(&r, 5, A, 1200, 7, 100, 0x18, 5, 0), rec(&r, 5, A, 1300, 7, 100, 0x18, 5, 0);
        rec(&r, 5, A, 1400, 7, 100, 0x19, 5, 0), rec(&r, 5, A, 1500, 7, 100, 0x18, 5, 0);
        rec(&r, 5, A, 1600, 7, 0, 0x11, 5, 0), rec(&r, 5, A, 1601, 7, 100, 0x18, 5, 0);
        rec(&r, 6, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 6, A, 1100, 7, 0, 0x18, 5, 0);
        rec(&r, 6, A, 1100, 7, 100, 0x18, 5, 0), rec(&r, 6, A, 1200, 7, 100, 0x18, 5, 0);
        rec(&r, 7, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 7, A, 1100, 7, 100, 0x18, 5, 30);
        rec(&r, 7, A, 1200, 7, 100, 0x18, 5, 0), rec(&r, 7, A, 1300, 7, 100, 0x18, 5, 0);
        rec(&r, 8, A, 1000, 7, 100, 0x18, 5, 0), rec(&r, 8, B, 1100, 7, 100, 0x18, 5, 0);
        for (uint32_t q = 0; q < 6; q++) rec(&r, 9, A, 5000 + 100 * q, 7, 100, 0x18, 5, 0);
        for (uint32_t q = 0; q < 9; q++) rec(&r, 10, A, 7000 + 1460 * q, 7, 1460, 0x18, 5, 0);
        if (!pass) free(r.seg), free(r.sip);
    }
    rxg_tcp_run *run = malloc(r.n * sizeof(*run));
    uint32_t nrun = 77;
    char s[64];
    CHECK(rxg_tcp_runs_host(r.seg, r.sip, r.n, 65536, run, &nrun) == RXG_OK);
    static const char *want[11] = {"3", "12", "12", "111", "112", "1121111", "112", "112", "11", "6", "9"};
    for (uint32_t f = 0; f < 11; f++) {
        split(&r, run, nrun, f, s);
        CHECK(strcmp(s, want[f]) == 0);
    }
    uint32_t end = 0, nsum = 0;
    for (uint32_t k = 0; k < nrun; k++) { /* a partition, laid out one after the other */
        CHECK(run[k].first == nsum && run[k].offset == ((end + 15u) & ~15u));
        uint32_t bytes = 0;
        for (uint32_t j = 0; j < run[k].nseg; j++) bytes += r.seg[run[k].first + j].ncopy;
        CHECK(bytes == run[k].bytes);
        end = run[k].offset + bytes, nsum += run[k].nseg;
    }
    CHECK(nsum == r.n);
    static const struct { uint32_t W; const char *f9, *f10; } win[] = {
        {1, "111111", "111111111"},   {100, "111111", "111111111"}, {250, "321", "111111111"},
        {300, "33", "111111111"},     {1460, "6", "111111111"},     {2920, "6", "22221"},
        {1u << 20, "6", "9"}};
    for (uint32_t w = 0; w < sizeof(win) / sizeof(win[0]); w++) {
        CHECK(rxg_tcp_runs_host(r.seg, r.sip, r.n, win[w].W, run, &nrun) == RXG_OK);
        split(&r, run, nrun, 9, s);
        CHECK(strcmp(s, win[w].f9) == 0);
        split(&r, run, nrun, 10, s);
        CHECK(strcmp(s, win[w].f10) == 0);
        if (win[w].W == 1) CHECK(nrun == r.n);
    }
    for (uint32_t j = 0; j < r.n; j++) CHECK(r.seg[j].offset == 0xDEAD0000u + j);
    CHECK(rxg_tcp_runs_host(NULL, NULL, 0, 65536, NULL, &nrun) == RXG_OK && nrun == 0);
    CHECK(rxg_tcp_runs_host(r.seg, r.sip, r.n, 0, run, &nrun) == RXG_EINVAL);
    CHECK(rxg_tcp_runs_host(r.seg, r.sip, r.n, (1u << 20) + 1, run, &nrun) == RXG_EINVAL);
    CHECK(rxg_tcp_runs_host(r.seg, r.sip, r.n, 65536, run, NULL) == RXG_EINVAL);
    free(run), free(r.seg), free(r.sip);
}

/* ---- one socket session ---------------------------------------------------------- */
static const uint8_t MAC_A[6] = {2, 0, 0, 0, 0, 1}, MAC_B[6] = {2, 0, 0, 0, 0, 2};
#define NF 40u

/* Ethernet + IPv4 + TCP (hl words of header) + payload; checksums by the oracle */
static size_t frame(uint8_t *f, uint32_t sip, uint16_t sport, uint32_t dip, uint16_t dport,
                    uint8_t flags, uint8_t hl, uint32_t seq, uint32_t ack, const void *pl, size_t pn) {
    memcpy(f, MAC_B, 6);
    memcpy(f + 6, MAC_A, 6);
    f[12] = 0x08, f[13] = 0x00;
    uint8_t *ip = f + 14;
    const uint16_t tl = (uint16_t)(20 + 4u * hl + pn);
    memset(ip, 0, 20 + 4u * hl);
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
    l4[12] = (uint8_t)(hl << 4), l4[13] = flags;
    l4[14] = 0xFF, l4[15] = 0xFF;
    if (pn) memcpy(l4 + 4u * hl, pl, pn);
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

/* oracle verdicts against the stack's control blocks, then nstack_deliver */
static void deliver(burst *b, int *rc) {
    rxg_udp_sock u[8];
    rxg_tcb t[8];
    uint32_t nu = 0, nt = 0, uid[8], tid[8];
    uint64_t gen = 0;
    CHECK(nstack_flows(u, 8, &nu, t, 8, &nt, &gen) == RXG_OK);
    oracle_tables *tb = oracle_tables_new(u, nu, t, nt);
    CHECK(tb);
    rxg_verdict v[NF];
    oracle_classify(tb, b->buf, b->off, b->len, b->n, 6, v, NULL);
    oracle_tables_free(tb);
    CHECK(nstack_flow_ids(uid, 8, tid, 8) == RXG_OK);
    rxg_mbuf mb[NF], *mp[NF];
    memset(mb, 0, sizeof(mb));
    for (uint32_t i = 0; i < b->n; ++i) {
        if (v[i].flow_id != RXG_FLOW_NONE)
            v[i].flow_id = v[i].cls == RXG_CLS_TCP ? tid[v[i].flow_id] : uid[v[i].flow_id];
        mb[i].buf_addr = b->buf + ((size_t)b->off[i] << 6);
        mb[i].data_len = b->len[i];
        mb[i].refcnt = 1;
        mp[i] = &mb[i];
    }
    CHECK(nstack_deliver(mp, b->n, v, gen, rc) >= 0);
}

static void socket_session(void) {
    const uint32_t L = inet_addr("192.168.100.77"), C = inet_addr("10.0.0.1");
    const uint16_t cp = htons(40000), lp = htons(9999);
    CHECK(nstack_init(RXG_HOST_ONLY, 256, 1 << 20) == RXG_OK);
    CHECK(nstack_set_local(L, MAC_A) == RXG_OK);
    CHECK(nstack_set_rx_inplace(1, NULL, NULL) == RXG_OK);
    CHECK(nstack_set_rx_gro(65536) == RXG_EINVAL); /* not with in-place receive */
    CHECK(nstack_set_rx_inplace(0, NULL, NULL) == RXG_OK);
    CHECK(nstack_set_rx_gro((1u << 20) + 1) == RXG_EINVAL);
    CHECK(nstack_set_rx_gro(3000) == RXG_OK);
    CHECK(nstack_set_rx_inplace(1, NULL, NULL) == RXG_EINVAL);
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
    /* two bursts: trains of 9, 1 and 5 segments with an options segment and an
     * empty PSH between them; then a train of 3, a FIN and a segment after it */
    static const uint32_t lens[2][20] = {{1460, 1460, 1, 7, 100, 600, 1460, 16, 17, 50, 0, 3, 15, 1460, 100, 100},
                                         {600, 1, 1460, 0, 9}};
    static const uint8_t kinds[2][20] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 2, 0}};
    static const uint32_t cnt[2] = {16, 5};
    uint8_t pay[1460], f[1600], *got = malloc(1 << 16), *want = malloc(1 << 16);
    uint32_t seq = 0xFFFFF000u, frags_ns = 0, frags_os = 0;
    size_t ngot = 0, nwant = 0;
    for (int bi = 0; bi < 2; bi++) {
        burst b = {.buf = calloc(NF, 1600), .n = 0, .pos = 0};
        for (uint32_t i = 0; i < cnt[bi]; i++) {
            for (uint32_t q = 0; q < lens[bi][i]; q++) pay[q] = (uint8_t)(seq + 31u * q + i);
            const uint8_t fl = kinds[bi][i] == 2 ? 0x11 : 0x18, hl = kinds[bi][i] == 1 ? 6 : 5;
            push(&b, f, frame(f, C, cp, L, lp, fl, hl, seq, 2000, pay, lens[bi][i]));
            seq += lens[bi][i] + (kinds[bi][i] == 2);
        }
        oracle_tx_cksum(b.buf, b.off, b.len, b.n, 6);
        int rc[NF];
        deliver(&b, rc);
        for (uint32_t i = 0; i < b.n; i++)
            CHECK(rc[i] == oracle_rx(st, b.buf + ((size_t)b.off[i] << 6), b.len[i]));
        free(b.buf);
        for (;;) { /* every fragment, a read each: the byte streams agree, EOF included */
            const ssize_t r = nrecv(cs, got + ngot, 8192, MSG_DONTWAIT);
            if (r < 0) break;
            CHECK(r <= 3000 + 1460);
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
    /* burst 1: runs {1460, 1460} {1 .. 17 and the 1460 before: window 3000} ...;
     * whatever the split, fewer fragments, and the counter says how many */
    CHECK(frags_ns < frags_os && nstack_stat(15) == frags_os - frags_ns);
    int32_t s1, s2, fd1, fd2;
    uint32_t rn1, rn2, sn1, sn2;
    CHECK(nstack_tcb_state(C, L, cp, lp, &s1, &rn1, &sn1, &fd1) == 0);
    CHECK(oracle_tcb_state(st, C, L, cp, lp, &s2, &rn2, &sn2, &fd2) >= 0);
    CHECK(s1 == s2 && rn1 == rn2 && sn1 == sn2 && fd1 == fd2);
    /* the queued ACKs: fewer, the last one the same */
    uint8_t fl1 = 0, fl2 = 0;
    uint32_t k1 = 0, k2 = 0, a1 = 0, a2 = 0;
    while (nstack_tcb_sndq(C, L, cp, lp, k1, &fl1, &a1) == 0) k1++;
    while (oracle_tcb_sndq(st, C, L, cp, lp, k2, &fl2, &a2) == 0) k2++;
    CHECK(k2 - k1 == frags_os - frags_ns);
    CHECK(nstack_tcb_sndq(C, L, cp, lp, k1 - 1, &fl1, &a1) == 0);
    CHECK(oracle_tcb_sndq(st, C, L, cp, lp, k2 - 1, &fl2, &a2) == 0 && fl1 == fl2 && a1 == a2);
    CHECK(nclose(cs) == 0 && nclose(ls) == 0);
    oracle_stack_free(st);
    free(got), free(want);
    nstack_fini();
}

int main(void) {
    rule_cases();
    socket_session();
    printf("GRO SAN OK\n");
    return 0;
}
