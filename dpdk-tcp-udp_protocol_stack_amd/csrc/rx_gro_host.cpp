// rx_gro_host.cpp — rxg_tcp_runs_host: the receive coalescing rule (the run
// kernels of rx_segsort.hip, rxg_tcp_coalesce_dev) restated in plain C++ on
// K4's records, for callers without a GPU (the socket layer's host-verdict
// path) and as the tests' second opinion.  Host only: no HIP, no context.
// The rule is the one of include/rxgpu.h ("TCP receive coalescing").
#include <stdint.h>

#include "../../include/rxgpu.h"

static_assert(sizeof(rxg_tcp_run) == 16, "rxg_tcp_run is 16 bytes");

namespace {

inline bool mergeable(const rxg_segment &g) {
    return g.flags == 0x18u && g.hl == 5u && g.plen > 0 && (int32_t)g.ncopy == g.plen;
}

inline bool links(const rxg_segment &p, uint32_t psip, const rxg_segment &g, uint32_t gsip) {
    return mergeable(p) && mergeable(g) && p.flow == g.flow && psip == gsip && p.sport == g.sport &&
           p.dport == g.dport && p.ack == g.ack && g.seq == p.seq + (uint32_t)p.plen;
}

} // namespace

int rxg_tcp_runs_host(const rxg_segment *seg, const uint32_t *sip, uint32_t nseg, uint32_t W,
                      rxg_tcp_run *run, uint32_t *nrun) {
    if (!nrun || W < 1u || W > RXG_GRO_MAX_WINDOW) return RXG_EINVAL;
    *nrun = 0;
    if (nseg && (!seg || !sip || !run)) return RXG_EINVAL;
    uint64_t b = 0;    // payload of the chain before record j
    uint64_t end = 0;  // end of the runs laid down so far
    uint32_t r = 0;
    for (uint32_t j = 0; j < nseg; ++j) {
        bool head = true;
        if (j && links(seg[j - 1], sip[j - 1], seg[j], sip[j])) {
            const uint64_t pb = b;
            b += (uint32_t)seg[j - 1].plen;
            head = b / W != pb / W;
        } else {
            b = 0;
        }
        if (head) {
            const uint64_t o = (end + 15u) & ~15ull;
            run[r].first = j;
            run[r].nseg = 0;
            run[r].bytes = 0;
            run[r].offset = (uint32_t)o;
            end = o;
            ++r;
        }
        run[r - 1].nseg += 1;
        run[r - 1].bytes += seg[j].ncopy;
        end += seg[j].ncopy;
    }
    *nrun = r;
    return RXG_OK;
}
