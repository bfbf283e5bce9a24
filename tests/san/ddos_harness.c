/* AddressSanitizer / UBSan harness for the entropy flood detector on the host
 * (csrc/rx_ddos_host.cpp, rxg_ddos_host).  A stand-alone program: compiled
 * with -fsanitize=address,undefined together with that source and run
 * directly (tests/test_rx_ddos.py).  Every buffer is a heap allocation of
 * exactly the bytes the call may touch (the frames end at the last frame's
 * last byte), so one byte read past a frame's len at the buffer's end, or one
 * output entry written past n, is a report:
 *   - the length cases: frames of 0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1500,
 *     9000 and 65535 bytes, each as the LAST frame of its buffer, bits checked
 *     against a byte-wise count, with 16-B and 64-B descriptor units;
 *   - an undefined frame (all zeros, all ones, empty) inside a window: D is
 *     NaN on the 256 frames whose windows hold it, the flag drops, the alarm
 *     rises again when it leaves;
 *   - a split session: the same frames in one call and in calls of 1, 255,
 *     256, 257 and the rest give the same flags and the same state bytes;
 *   - n = 0, nullable outputs, NULL and NaN arguments.
 */
#include <math.h>
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

static uint32_t g_rng = 12345u;
static uint8_t rnd8(void) {
    g_rng = g_rng * 1664525u + 1013904223u;
    return (uint8_t)(g_rng >> 24);
}

static uint32_t slow_bits(const uint8_t *p, uint32_t n) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; i++)
        for (int b = 0; b < 8; b++) c += (p[i] >> b) & 1u;
    return c;
}

/* nf 64-B random frames then one frame of `last` bytes; the buffer ends with it */
typedef struct {
    uint8_t *pk;
    uint32_t *off, n;
    uint16_t *len;
} burst;

static burst make(uint32_t nf, uint32_t last, uint32_t ul, int fill) {
    burst b;
    const uint64_t unit = 1ull << ul;
    b.n = nf + 1;
    const uint64_t head = (uint64_t)nf * ((64 + unit - 1) / unit * unit);
    b.pk = malloc(head + last ? head + last : 1);
    b.off = malloc(b.n * sizeof(*b.off));
    b.len = malloc(b.n * sizeof(*b.len));
    CHECK(b.pk && b.off && b.len);
    memset(b.pk, 0xFF, head + last);
    for (uint32_t i = 0; i < nf; i++) {
        b.off[i] = (uint32_t)(i * ((64 + unit - 1) / unit));
        b.len[i] = 64;
        for (int k = 0; k < 64; k++) b.pk[((uint64_t)b.off[i] << ul) + k] = rnd8();
    }
    b.off[nf] = (uint32_t)(head >> ul);
    b.len[nf] = (uint16_t)last;
    for (uint32_t k = 0; k < last; k++) b.pk[head + k] = fill < 0 ? rnd8() : (uint8_t)fill;
    return b;
}

static void drop(burst *b) { free(b->pk), free(b->off), free(b->len); }

static void length_cases(void) {
    static const uint32_t L[] = {0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1500, 9000, 65535};
    for (uint32_t ul = 4; ul <= 6; ul += 2)
        for (size_t k = 0; k < sizeof(L) / sizeof(L[0]); k++) {
            burst b = make(300, L[k], ul, -1);
            rxg_ddos_state st;
            memset(&st, 0, sizeof(st));
            rxg_ddos_summary sum;
            uint32_t *bits = malloc(b.n * sizeof(*bits));
            uint8_t *flag = malloc(b.n);
            double *stat = malloc(b.n * sizeof(*stat));
            CHECK(rxg_ddos_host(b.pk, b.off, b.len, b.n, ul, 1200.0, &st, bits, flag, stat, &sum) ==
                  RXG_OK);
            for (uint32_t i = 0; i < b.n; i++)
                CHECK(bits[i] == slow_bits(b.pk + ((uint64_t)b.off[i] << ul), b.len[i]));
            CHECK(sum.frames_seen == 301 && st.frames_seen == 301);
            CHECK(st.set[300 % 256] == bits[300] && st.tot[300 % 256] == 8u * L[k]);
            CHECK((flag[300] & RXG_DDOS_UNDEF) ? (L[k] == 0 && isnan(stat[300])) : !isnan(stat[300]));
            free(bits), free(flag), free(stat);
            drop(&b);
        }
}

static void undefined_frame(void) {
    static const int fills[] = {0x00, 0xFF, -2};
    for (int c = 0; c < 3; c++) {
        burst b = make(899, 64, 6, -1);
        const uint32_t at = 400;
        if (fills[c] == -2)
            b.len[at] = 0; /* the empty frame */
        else
            memset(b.pk + ((uint64_t)b.off[at] << 6), fills[c], 64);
        rxg_ddos_state st;
        memset(&st, 0, sizeof(st));
        rxg_ddos_summary sum;
        uint8_t *flag = malloc(b.n);
        double *stat = malloc(b.n * sizeof(*stat));
        CHECK(rxg_ddos_host(b.pk, b.off, b.len, b.n, 6, 1200.0, &st, NULL, flag, stat, &sum) == RXG_OK);
        for (uint32_t i = 256; i < b.n; i++) {
            const int und = i >= at && i < at + 256;
            CHECK(((flag[i] & RXG_DDOS_UNDEF) != 0) == und && (isnan(stat[i]) != 0) == und);
            CHECK(!und || !(flag[i] & RXG_DDOS_ALARM));
        }
        /* random 64-B frames alarm at 1200 (D about 2100): falls at `at`, rises after */
        CHECK((flag[256] & RXG_DDOS_RISE) && (flag[at] & RXG_DDOS_FALL) && (flag[at + 256] & RXG_DDOS_RISE));
        CHECK(sum.undef_frames == 256 && sum.rises == 2 && sum.falls == 1 && sum.flag == 1);
        CHECK(sum.first_alarm == 256 && sum.alarm_frames == b.n - 256 - 256);
        free(flag), free(stat);
        drop(&b);
    }
}

static void split_session(void) {
    burst b = make(1299, 64, 6, -1);
    memset(b.pk + ((uint64_t)b.off[1000] << 6), 0xFF, 64);
    rxg_ddos_state one, parts;
    memset(&one, 0, sizeof(one));
    memset(&parts, 0, sizeof(parts));
    rxg_ddos_summary sum, psum;
    uint8_t *f1 = malloc(b.n), *f2 = malloc(b.n);
    CHECK(rxg_ddos_host(b.pk, b.off, b.len, b.n, 6, 1200.0, &one, NULL, f1, NULL, &sum) == RXG_OK);
    static const uint32_t cut[] = {1, 255, 256, 257, 531};
    uint32_t a = 0, alarms = 0, rises = 0, falls = 0, undef = 0;
    for (int k = 0; k < 5; k++) {
        /* exact-size copies of this part's descriptors */
        uint32_t *off = malloc(cut[k] * sizeof(*off));
        uint16_t *len = malloc(cut[k] * sizeof(*len));
        uint8_t *fl = malloc(cut[k]);
        memcpy(off, b.off + a, cut[k] * sizeof(*off));
        memcpy(len, b.len + a, cut[k] * sizeof(*len));
        CHECK(rxg_ddos_host(b.pk, off, len, cut[k], 6, 1200.0, &parts, NULL, fl, NULL, &psum) == RXG_OK);
        memcpy(f2 + a, fl, cut[k]);
        alarms += psum.alarm_frames, rises += psum.rises, falls += psum.falls, undef += psum.undef_frames;
        a += cut[k];
        CHECK(psum.frames_seen == a);
        free(off), free(len), free(fl);
    }
    CHECK(a == b.n && memcmp(f1, f2, b.n) == 0 && memcmp(&one, &parts, sizeof(one)) == 0);
    CHECK(alarms == sum.alarm_frames && rises == sum.rises && falls == sum.falls &&
          undef == sum.undef_frames && psum.flag == sum.flag);
    /* n = 0: the state stays, the summary is written */
    const rxg_ddos_state before = one;
    CHECK(rxg_ddos_host(NULL, NULL, NULL, 0, 6, 1200.0, &one, NULL, NULL, NULL, &sum) == RXG_OK);
    CHECK(memcmp(&before, &one, sizeof(one)) == 0 && sum.frames_seen == b.n && sum.alarm_frames == 0 &&
          sum.first_alarm == 0xFFFFFFFFu && isnan(sum.last_stat));
    CHECK(rxg_ddos_host(b.pk, b.off, b.len, 1, 6, 1200.0, NULL, NULL, NULL, NULL, &sum) == RXG_EINVAL);
    CHECK(rxg_ddos_host(b.pk, b.off, b.len, 1, 6, 1200.0, &one, NULL, NULL, NULL, NULL) == RXG_EINVAL);
    CHECK(rxg_ddos_host(NULL, b.off, b.len, 1, 6, 1200.0, &one, NULL, NULL, NULL, &sum) == RXG_EINVAL);
    CHECK(rxg_ddos_host(b.pk, b.off, b.len, 1, 3, 1200.0, &one, NULL, NULL, NULL, &sum) == RXG_EINVAL);
    CHECK(rxg_ddos_host(b.pk, b.off, b.len, 1, 6, NAN, &one, NULL, NULL, NULL, &sum) == RXG_EINVAL);
    CHECK(memcmp(&before, &one, sizeof(one)) == 0);
    free(f1), free(f2);
    drop(&b);
}

int main(void) {
    CHECK(rxg_ddos_entropy(256, 512) == 521.0);
    CHECK(isnan(rxg_ddos_entropy(23651, 17408)));
    length_cases();
    undefined_frame();
    split_session();
    printf("DDOS SAN OK\n");
    return 0;
}
