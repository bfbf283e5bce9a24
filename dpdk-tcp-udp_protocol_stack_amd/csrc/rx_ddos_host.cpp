// rx_ddos_host.cpp — rxg_ddos_host: the entropy flood detector (K6,
// csrc/rx_ddos.hip, rxg_ddos_dev) restated in plain C++, frame by frame as the
// reference runs it (ddos_detect, .vscode/test.c:2846-2891): the window sums
// are taken over the ring in slot order 0..255 for every checked frame, with
// libm's log2.  For callers without a GPU (the socket layer's host-verdict
// path) and as the tests' second opinion.  Host only: no HIP, no context.
// The rule is the one of include/rxgpu.h ("Entropy flood detector").
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/rxgpu.h"

double rxg_ddos_entropy(double set_bits, double total_bits) {
    return (-set_bits) * (log2(set_bits) - log2(total_bits)) -
           (total_bits - set_bits) * (log2(total_bits - set_bits) - log2(total_bits)) +
           log2(total_bits);
}

namespace {

// decided from the integers, never from a floating NaN
inline bool undefined(uint32_t s, uint32_t t) { return s == 0u || s >= t; }

// 1-bits in exactly len bytes (the reference's count_bit reads whole 8-byte
// words, past the end; here bytes past len never count)
uint32_t count_bits(const uint8_t *p, uint32_t len) {
    uint32_t c = 0, i = 0;
    for (; i + 8 <= len; i += 8) {
        uint64_t v;
        memcpy(&v, p + i, 8);
        c += (uint32_t)__builtin_popcountll(v);
    }
    for (; i < len; ++i) c += (uint32_t)__builtin_popcount(p[i]);
    return c;
}

} // namespace

int rxg_ddos_host(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                  uint32_t off_unit_log2, double thresh, rxg_ddos_state *state, uint32_t *bits,
                  uint8_t *flag, double *stat, rxg_ddos_summary *summary) {
    if (!state || !summary || (n && (!pkts || !off || !len))) return RXG_EINVAL;
    if (thresh != thresh || off_unit_log2 < 4 || off_unit_log2 > 16) return RXG_EINVAL;
    // the reference keeps p_entropy beside the two integer rings; it is a
    // function of them, so the state does not carry it
    double ent[RXG_DDOS_WINDOW];
    for (uint32_t i = 0; i < RXG_DDOS_WINDOW; ++i)
        ent[i] = undefined(state->set[i], state->tot[i])
                     ? 0.0
                     : rxg_ddos_entropy(state->set[i], state->tot[i]);
    rxg_ddos_summary s;
    memset(&s, 0, sizeof(s));
    s.first_alarm = 0xFFFFFFFFu;
    s.last_stat = NAN;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t set_bits = count_bits(pkts + ((uint64_t)off[j] << off_unit_log2), len[j]);
        const uint32_t tot_bits = 8u * (uint32_t)len[j];
        const uint32_t slot = (uint32_t)(state->frames_seen % RXG_DDOS_WINDOW);
        state->set[slot] = set_bits;
        state->tot[slot] = tot_bits;
        ent[slot] = undefined(set_bits, tot_bits) ? 0.0 : rxg_ddos_entropy(set_bits, tot_bits);
        uint8_t f = RXG_DDOS_WARMUP;
        double D = NAN;
        if (state->frames_seen >= RXG_DDOS_WINDOW) {
            uint32_t total_set = 0, total_bit = 0, undef = 0;
            double sum_entropy = 0.0;
            for (uint32_t i = 0; i < RXG_DDOS_WINDOW; ++i) {
                total_set += state->set[i];
                total_bit += state->tot[i];
                undef += undefined(state->set[i], state->tot[i]) ? 1u : 0u;
                sum_entropy += ent[i];
            }
            uint32_t alarm = 0;
            f = 0;
            if (undef) {
                f = RXG_DDOS_UNDEF;
                ++s.undef_frames;
            } else {
                D = sum_entropy - rxg_ddos_entropy(total_set, total_bit);
                if (thresh < D) alarm = 1, f = RXG_DDOS_ALARM;
            }
            if (alarm) {
                if (s.alarm_frames++ == 0) s.first_alarm = j;
                if (!state->flag) f |= RXG_DDOS_RISE, ++s.rises;
            } else if (state->flag) {
                f |= RXG_DDOS_FALL, ++s.falls;
            }
            state->flag = alarm;
            s.last_stat = D;
            s.last_set = total_set;
            s.last_tot = total_bit;
        }
        ++state->frames_seen;
        if (bits) bits[j] = set_bits;
        if (flag) flag[j] = f;
        if (stat) stat[j] = D;
    }
    s.frames_seen = state->frames_seen;
    s.flag = state->flag ? 1u : 0u;
    *summary = s;
    return RXG_OK;
}
