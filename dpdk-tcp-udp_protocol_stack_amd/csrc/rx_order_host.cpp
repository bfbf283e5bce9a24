// rx_order_host.cpp — rxg_tcp_order_host: the sequence ordering rule (the
// ord_* kernels of rx_segsort.hip, rxg_tcp_compact_ordered_dev) restated in
// plain C++ on K4's records, for callers without a GPU (the socket layer's
// host-verdict path) and as the tests' second opinion.  Host only: no HIP, no
// context.  The rule is the one of include/rxgpu.h ("TCP sequence ordering").
#include <stdint.h>

#include <algorithm>

#include "../../include/rxgpu.h"

namespace {

inline bool movable(const rxg_segment &g) { return (g.flags & 0x06u) == 0u; }

inline bool same_group(const rxg_segment &p, uint32_t psip, const rxg_segment &g, uint32_t gsip) {
    return movable(p) && movable(g) && p.flow == g.flow && psip == gsip && p.sport == g.sport &&
           p.dport == g.dport;
}

} // namespace

int rxg_tcp_order_host(const rxg_segment *seg, const uint32_t *sip, uint32_t nseg, uint32_t *perm,
                       uint32_t *moved) {
    if (!seg || !sip || !perm || !moved) return RXG_EINVAL;
    *moved = 0;
    uint32_t m = 0;
    for (uint32_t h = 0; h < nseg;) {
        uint32_t e = h + 1;
        while (e < nseg && same_group(seg[e - 1], sip[e - 1], seg[e], sip[e])) ++e;
        for (uint32_t j = h; j < e; ++j) perm[j] = j;
        const uint32_t s0 = seg[h].seq;
        // (stable: equal distances from the head keep arrival order)
        std::stable_sort(perm + h, perm + e, [&](uint32_t a, uint32_t b) {
            return (int32_t)(seg[a].seq - s0) < (int32_t)(seg[b].seq - s0);
        });
        for (uint32_t j = h; j < e; ++j) m += perm[j] != j;
        h = e;
    }
    *moved = m;
    return RXG_OK;
}
