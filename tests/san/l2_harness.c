/* AddressSanitizer / UBSan harness for the L2 responder on the host: the
 * rule's restatement (csrc/rx_l2_host.cpp, rxg_l2_host).  A stand-alone
 * program: compiled with -fsanitize=address,undefined together with that
 * source and run directly (tests/test_rx_l2.py).  Every input and output is a
 * heap allocation of exactly the size the call may touch (the frame buffer
 * ends with the last frame's captured bytes, the answer buffer is cap_bytes
 * long, the index arrays have n entries), so one byte read or written past
 * them is a report:
 *   - the hand cases: the two known answers (a who-has and a 98-byte ping,
 *     their replies written out), an ARP reply to us, a 41-byte ARP, an ARP
 *     for another address, a ping cut one byte short, one with a flipped
 *     bit, tl 27 and 28, a header with options, cap_bytes one byte short of
 *     the second answer, nlocal 0 and 9, NULL outputs;
 *   - a fuzzed burst of 3000 frames with random lengths, total lengths and
 *     classes, answered into exactly the room its answers need.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rxgpu.h"

#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c);                   \
            exit(2);                                                                               \
        }                                                                                          \
    } while (0)

static const uint8_t LOCAL_MAC[6] = {0x00, 0x0c, 0x29, 0x6a, 0x01, 0x4d};
static const uint8_t LOCAL_IP[4] = {192, 168, 1, 10};

static const uint8_t KA_ARP_REQ[60] = {
    0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0x08, 0x06, 0x00, 0x01,
    0x08, 0x00, 0x06, 0x04, 0x00, 0x01, 0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0xc0, 0xa8, 0x01, 0x14,
    0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0xc0, 0xa8, 0x01, 0x0a};
static const uint8_t KA_ARP_REPLY[42] = {
    0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0x00, 0x0c, 0x29, 0x6a, 0x01, 0x4d, 0x08, 0x06, 0x00, 0x01,
    0x08, 0x00, 0x06, 0x04, 0x00, 0x02, 0x00, 0x0c, 0x29, 0x6a, 0x01, 0x4d, 0xc0, 0xa8, 0x01, 0x0a,
    0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0xc0, 0xa8, 0x01, 0x14};
/* the 98-byte ping of tests/l2_ref.py: payload 00 01 .. 37 */
static const uint8_t KA_ECHO_HEAD[42] = {
    0x00, 0x0c, 0x29, 0x6a, 0x01, 0x4d, 0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0x08, 0x00, 0x45, 0x00,
    0x00, 0x54, 0x12, 0x34, 0x40, 0x00, 0x40, 0x01, 0xa5, 0x06, 0xc0, 0xa8, 0x01, 0x14, 0xc0, 0xa8,
    0x01, 0x0a, 0x08, 0x00, 0x00, 0xeb, 0x00, 0x01, 0x00, 0x01};
static const uint8_t KA_REPLY_HEAD[42] = {
    0x02, 0xaa, 0xbb, 0xcc, 0xdd, 0xee, 0x00, 0x0c, 0x29, 0x6a, 0x01, 0x4d, 0x08, 0x00, 0x45, 0x00,
    0x00, 0x54, 0x00, 0x00, 0x00, 0x00, 0x40, 0x01, 0xf7, 0x3a, 0xc0, 0xa8, 0x01, 0x0a, 0xc0, 0xa8,
    0x01, 0x14, 0x00, 0x00, 0x08, 0xeb, 0x00, 0x01, 0x00, 0x01};

static void ping(uint8_t f[98]) {
    memcpy(f, KA_ECHO_HEAD, 42);
    for (int i = 0; i < 56; i++) f[42 + i] = (uint8_t)i;
}

static rxg_l2_params params(uint32_t nlocal) {
    rxg_l2_params p;
    memset(&p, 0, sizeof(p));
    p.nlocal = nlocal;
    memcpy(&p.local[0].ip, LOCAL_IP, 4);
    memcpy(p.local[0].mac, LOCAL_MAC, 6);
    return p;
}

/* a burst in exact-size heap buffers: frames at 16-B slots, the buffer ending
 * with the last frame's captured bytes */
typedef struct {
    uint8_t *pkts, *status, *out;
    uint32_t *off, *roff, *rsrc, n;
    uint16_t *len, *rlen;
    rxg_verdict *v;
    uint64_t cap;
    uint32_t tot[6];
} burst;

static burst make(const uint8_t *const *fr, const uint16_t *cap, const uint8_t *cls, uint32_t n,
                  uint64_t out_cap) {
    burst b;
    memset(&b, 0, sizeof(b));
    b.n = n, b.cap = out_cap;
    uint64_t pos = 0, end = 0;
    b.off = malloc(n * sizeof(uint32_t) + 1), b.len = malloc(n * sizeof(uint16_t) + 1);
    b.v = calloc(n + 1, sizeof(rxg_verdict));
    for (uint32_t i = 0; i < n; i++) {
        b.off[i] = (uint32_t)(pos >> 4), b.len[i] = cap[i], b.v[i].cls = cls[i];
        end = pos + cap[i];
        pos += ((uint64_t)cap[i] + 15u) & ~15ull;
        if (!cap[i]) pos += 16;
    }
    b.pkts = malloc(end ? end : 1);
    for (uint32_t i = 0; i < n; i++) memcpy(b.pkts + ((uint64_t)b.off[i] << 4), fr[i], cap[i]);
    b.status = malloc(n ? n : 1), b.out = malloc(out_cap ? out_cap : 1);
    b.roff = malloc(n * sizeof(uint32_t) + 1), b.rsrc = malloc(n * sizeof(uint32_t) + 1);
    b.rlen = malloc(n * sizeof(uint16_t) + 1);
    return b;
}
static int run(burst *b, const rxg_l2_params *p) {
    return rxg_l2_host(b->pkts, b->off, b->len, b->n, 4, b->v, p, b->status, b->out, b->cap, b->roff,
                       b->rlen, b->rsrc, b->tot);
}
static void drop(burst *b) {
    free(b->pkts), free(b->status), free(b->out), free(b->off), free(b->roff), free(b->rsrc);
    free(b->len), free(b->rlen), free(b->v);
}

static void hand_cases(void) {
    uint8_t f[16][98];
    const uint8_t *fr[16];
    uint16_t cap[16];
    uint8_t cls[16], want[16];
    uint32_t n = 0;
#define CASE(src, len_, cap_, cls_, st_)                                                           \
    memset(f[n], 0, 98), memcpy(f[n], src, len_), fr[n] = f[n], cap[n] = cap_, cls[n] = cls_,      \
    want[n] = st_, n++
    uint8_t p[98];
    ping(p);
    CASE(KA_ARP_REQ, 60, 60, RXG_CLS_ARP, RXG_L2_ARP_REQ);
    CASE(p, 98, 98, RXG_CLS_IPV4_OTHER, RXG_L2_ECHO);
    CASE(KA_ARP_REQ, 60, 60, RXG_CLS_ARP, RXG_L2_ARP_REPLY), f[n - 1][21] = 2;
    CASE(KA_ARP_REQ, 60, 41, RXG_CLS_ARP, 0);
    CASE(KA_ARP_REQ, 60, 42, RXG_CLS_ARP, RXG_L2_ARP_REQ);
    CASE(KA_ARP_REQ, 60, 60, RXG_CLS_ARP, 0), f[n - 1][41] = 0x0b;
    CASE(KA_ARP_REQ, 60, 60, RXG_CLS_NON_IP, 0);
    CASE(p, 98, 97, RXG_CLS_IPV4_OTHER, RXG_L2_ECHO_BAD);
    CASE(p, 98, 98, RXG_CLS_IPV4_OTHER, RXG_L2_ECHO_BAD), f[n - 1][97] ^= 0x40;
    CASE(p, 98, 98, RXG_CLS_IPV4_OTHER, 0), f[n - 1][17] = 27;
    CASE(p, 98, 98, RXG_CLS_IPV4_OTHER, 0), f[n - 1][14] = 0x46;
    CASE(p, 98, 98, RXG_CLS_UDP, 0);
    /* tl 28: the 8-byte message 08 00 f7 fd 00 01 00 01 */
    CASE(p, 42, 42, RXG_CLS_IPV4_OTHER, RXG_L2_ECHO), f[n - 1][17] = 28, f[n - 1][36] = 0xf7,
        f[n - 1][37] = 0xfd;
#undef CASE
    rxg_l2_params pr = params(1);
    burst b = make(fr, cap, cls, n, 64 + 128 + 64 + 64);
    CHECK(run(&b, &pr) == RXG_OK);
    for (uint32_t i = 0; i < n; i++) CHECK(b.status[i] == want[i]);
    CHECK(b.tot[0] == 2 && b.tot[1] == 1 && b.tot[2] == 2 && b.tot[3] == 2 && b.tot[4] == 4 && b.tot[5] == 5);
    CHECK(b.roff[0] == 0 && b.rlen[0] == 42 && b.rsrc[0] == 0 && !memcmp(b.out, KA_ARP_REPLY, 42));
    CHECK(b.roff[1] == 1 && b.rlen[1] == 98 && b.rsrc[1] == 1 && !memcmp(b.out + 64, KA_REPLY_HEAD, 42));
    for (int i = 0; i < 56; i++) CHECK(b.out[64 + 42 + i] == i);
    for (int i = 42; i < 64; i++) CHECK(b.out[i] == 0);
    for (int i = 98; i < 128; i++) CHECK(b.out[64 + i] == 0);
    CHECK(b.roff[2] == 3 && b.rsrc[2] == 4 && b.roff[3] == 4 && b.rlen[3] == 42 && b.rsrc[3] == 12);
    CHECK(b.out[256 + 34] == 0 && b.out[256 + 36] == 0xff && b.out[256 + 37] == 0xfd);
    drop(&b);
    /* one byte short of the second answer: it and the later ones are not written */
    b = make(fr, cap, cls, n, 64 + 127);
    CHECK(run(&b, &pr) == RXG_OK && b.tot[4] == 1 && b.tot[5] == 1 && b.tot[0] == 2 && b.tot[2] == 2);
    drop(&b);
    b = make(fr, cap, cls, n, 0);
    CHECK(run(&b, &pr) == RXG_OK && b.tot[4] == 0 && b.tot[5] == 0 && b.tot[2] == 2);
    rxg_l2_params none = params(0), nine = params(9);
    CHECK(run(&b, &none) == RXG_OK && b.tot[0] + b.tot[1] + b.tot[2] + b.tot[3] == 0);
    CHECK(run(&b, &nine) == RXG_EINVAL);
    CHECK(rxg_l2_host(b.pkts, b.off, b.len, n, 4, b.v, &pr, NULL, b.out, 0, b.roff, b.rlen, b.rsrc, b.tot) ==
          RXG_EINVAL);
    CHECK(rxg_l2_host(b.pkts, b.off, b.len, n, 4, b.v, &pr, b.status, b.out, 0, b.roff, b.rlen, b.rsrc,
                      NULL) == RXG_EINVAL);
    CHECK(rxg_l2_host(NULL, NULL, NULL, 0, 4, NULL, &pr, b.status, b.out, 0, b.roff, b.rlen, b.rsrc, b.tot) ==
          RXG_OK);
    drop(&b);
}

static uint32_t rnd(uint64_t *s) {
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(*s >> 33);
}

static void fuzz(void) {
    enum { N = 3000 };
    uint64_t seed = 42;
    uint8_t **fr = malloc(N * sizeof(*fr));
    uint16_t *cap = malloc(N * sizeof(*cap));
    uint8_t *cls = malloc(N);
    for (uint32_t i = 0; i < N; i++) {
        uint8_t p[98];
        ping(p);
        const uint32_t kind = rnd(&seed) % 8, len = 14 + rnd(&seed) % 1600;
        fr[i] = malloc(len > 98 ? len : 98);
        for (uint32_t k = 0; k < len; k++) fr[i][k] = (uint8_t)rnd(&seed);
        if (kind < 2) memcpy(fr[i], KA_ARP_REQ, 60);
        if (kind >= 2 && kind < 6) {
            /* an echo request whose total length is any value: a good one when
             * the message is all the ping's, else mostly a bad checksum */
            memcpy(fr[i], p, 42);
            if (kind < 4) memcpy(fr[i], p, 98);
            if (kind == 4) fr[i][16] = (uint8_t)(rnd(&seed) % 8), fr[i][17] = (uint8_t)rnd(&seed);
        }
        cls[i] = kind < 2 ? RXG_CLS_ARP : kind < 7 ? RXG_CLS_IPV4_OTHER : RXG_CLS_TCP;
        cap[i] = (uint16_t)(kind == 3 ? 42 + rnd(&seed) % 57 : kind < 2 ? 41 + rnd(&seed) % 20 : len);
        if (kind == 2) cap[i] = 98;
    }
    rxg_l2_params pr = params(1);
    burst b = make((const uint8_t *const *)fr, cap, cls, N, 4u << 20);
    CHECK(run(&b, &pr) == RXG_OK);
    CHECK(b.tot[0] > 100 && b.tot[2] > 100 && b.tot[3] > 100 && b.tot[4] == b.tot[0] + b.tot[2]);
    const uint64_t span = (uint64_t)b.tot[5] * 64u;
    const uint32_t nans = b.tot[4];
    drop(&b);
    /* exactly the room the answers need, then one byte less */
    b = make((const uint8_t *const *)fr, cap, cls, N, span);
    CHECK(run(&b, &pr) == RXG_OK && b.tot[4] == nans && (uint64_t)b.tot[5] * 64u == span);
    drop(&b);
    b = make((const uint8_t *const *)fr, cap, cls, N, span - 1);
    CHECK(run(&b, &pr) == RXG_OK && b.tot[4] == nans - 1);
    drop(&b);
    for (uint32_t i = 0; i < N; i++) free(fr[i]);
    free(fr), free(cap), free(cls);
}

int main(void) {
    hand_cases();
    fuzz();
    printf("L2 SAN OK\n");
    return 0;
}
