// rx_assemble_host.cpp — rxg_tcp_assemble_host: the stream assembly rule (the
// asm_* kernels of rx_segsort.hip, rxg_tcp_assemble_dev) restated in plain C++
// on already ordered records, for callers without a GPU (the socket layer's
// host-verdict path) and as the tests' second opinion.  Host only: no HIP, no
// context, one walk per group.  The rule is the one of include/rxgpu.h ("TCP
// stream assembly").
#include <stdint.h>

#include "../../include/rxgpu.h"

namespace {

inline bool movable(const rxg_segment &g) { return (g.flags & 0x06u) == 0u; }

inline bool same_group(const rxg_segment &p, uint32_t psip, const rxg_segment &g, uint32_t gsip) {
    return movable(p) && movable(g) && p.flow == g.flow && psip == gsip && p.sport == g.sport &&
           p.dport == g.dport;
}

} // namespace

int rxg_tcp_assemble_host(const rxg_segment *seg, const uint32_t *sip, const uint32_t *avail,
                          uint32_t nseg, rxg_tcp_stream *stream, uint32_t *nstream, uint32_t *skip,
                          uint32_t *take, uint32_t *dst) {
    if (!seg || !sip || !avail || !stream || !nstream || !skip || !take || !dst) return RXG_EINVAL;
    uint32_t ns = 0;     // streams so far
    uint64_t where = 0;  // the 16-B-rounded end of the last closed stream
    for (uint32_t h = 0; h < nseg;) {
        uint32_t e = h + 1;
        while (e < nseg && same_group(seg[e - 1], sip[e - 1], seg[e], sip[e])) ++e;
        uint64_t cov = 0;     // the group's bytes covered so far, from seq[h]
        bool fin_before = false;
        rxg_tcp_stream *st = nullptr;
        for (uint32_t j = h; j < e; ++j) {
            const rxg_segment &g = seg[j];
            const bool usable = g.plen <= 0 || avail[j] >= (uint32_t)g.plen;
            const uint64_t dlen = (movable(g) && usable && g.plen > 0) ? (uint64_t)g.plen : 0u;
            const uint64_t a = (uint32_t)(g.seq - seg[h].seq), end = a + dlen;
            const uint64_t from = a > cov ? a : cov;
            const uint64_t t = end > from ? end - from : 0u;
            const bool finok = movable(g) && usable && (g.flags & 0x01u) && end >= cov;
            const bool hole = j != h && a > cov;
            if (j == h || hole || fin_before) { // a new stream, behind the one before
                if (st) where += ((uint64_t)st->bytes + 15u) & ~(uint64_t)15u;
                st = &stream[ns++];
                st->first = j;
                st->nseg = 0;
                st->seq = seg[h].seq + (uint32_t)from;
                st->bytes = 0;
                st->offset = (uint32_t)where;
                st->flags = hole ? RXG_STREAM_HOLE : 0u;
                st->reserved = 0;
            }
            take[j] = (uint32_t)t;
            skip[j] = (uint32_t)(dlen - t);
            dst[j] = (uint32_t)(where + st->bytes);
            st->nseg++;
            st->bytes += (uint32_t)t;
            st->ack = g.ack;
            if (finok) st->flags |= RXG_STREAM_FIN;
            fin_before = finok;
            if (end > cov) cov = end;
        }
        where += ((uint64_t)st->bytes + 15u) & ~(uint64_t)15u;
        h = e;
    }
    *nstream = ns;
    return RXG_OK;
}
