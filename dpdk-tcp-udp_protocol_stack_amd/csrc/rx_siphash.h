// rx_siphash.h — SipHash-2-4 (Aumasson, Bernstein; 64-bit output) on whole
// little-endian 64-bit words, for the SYN cookie (K7, csrc/rx_syncookie.hip
// and its CPU statement csrc/rx_syncookie_host.cpp).  Plain 64-bit integer
// arithmetic; compiled by hipcc for both sides and by the host compiler alone.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RX_SIP_HD __host__ __device__ __forceinline__
#else
#define RX_SIP_HD static inline
#endif

struct rx_sip {
    uint64_t v0, v1, v2, v3;
};

RX_SIP_HD uint64_t rx_sip_rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }

RX_SIP_HD void rx_sip_round(rx_sip &s) {
    s.v0 += s.v1, s.v1 = rx_sip_rotl(s.v1, 13), s.v1 ^= s.v0, s.v0 = rx_sip_rotl(s.v0, 32);
    s.v2 += s.v3, s.v3 = rx_sip_rotl(s.v3, 16), s.v3 ^= s.v2;
    s.v0 += s.v3, s.v3 = rx_sip_rotl(s.v3, 21), s.v3 ^= s.v0;
    s.v2 += s.v1, s.v1 = rx_sip_rotl(s.v1, 17), s.v1 ^= s.v2, s.v2 = rx_sip_rotl(s.v2, 32);
}

RX_SIP_HD rx_sip rx_sip_init(uint64_t k0, uint64_t k1) {
    rx_sip s;
    s.v0 = k0 ^ 0x736f6d6570736575ull; // "somepseu"
    s.v1 = k1 ^ 0x646f72616e646f6dull; // "dorandom"
    s.v2 = k0 ^ 0x6c7967656e657261ull; // "lygenera"
    s.v3 = k1 ^ 0x7465646279746573ull; // "tedbytes"
    return s;
}

// one message word: 2 compression rounds
RX_SIP_HD void rx_sip_word(rx_sip &s, uint64_t m) {
    s.v3 ^= m;
    rx_sip_round(s);
    rx_sip_round(s);
    s.v0 ^= m;
}

// 4 finalisation rounds
RX_SIP_HD uint64_t rx_sip_final(rx_sip &s) {
    s.v2 ^= 0xff;
    rx_sip_round(s);
    rx_sip_round(s);
    rx_sip_round(s);
    rx_sip_round(s);
    return s.v0 ^ s.v1 ^ s.v2 ^ s.v3;
}

// the cookie's message: three words, then the length word of a 24-byte message
RX_SIP_HD uint64_t rx_sip24_3(uint64_t k0, uint64_t k1, uint64_t w0, uint64_t w1, uint64_t w2) {
    rx_sip s = rx_sip_init(k0, k1);
    rx_sip_word(s, w0);
    rx_sip_word(s, w1);
    rx_sip_word(s, w2);
    rx_sip_word(s, 24ull << 56);
    return rx_sip_final(s);
}

// cookie(tuple, isn, t) of include/rxgpu.h ("SYN cookies"); sip, dip, sport and
// dport are the raw loads of the frame's fields
RX_SIP_HD uint32_t rx_cookie(uint64_t k0, uint64_t k1, uint32_t sip, uint32_t dip, uint32_t sport,
                             uint32_t dport, uint32_t isn, uint32_t t) {
    const uint64_t w0 = (uint64_t)sip | ((uint64_t)dip << 32);
    const uint64_t w1 = (uint64_t)(sport & 0xFFFFu) | ((uint64_t)(dport & 0xFFFFu) << 16) |
                        ((uint64_t)isn << 32);
    const uint64_t h = rx_sip24_3(k0, k1, w0, w1, (uint64_t)t);
    return ((t & 0xFFu) << 24) | ((uint32_t)h & 0xFFFFFFu);
}
