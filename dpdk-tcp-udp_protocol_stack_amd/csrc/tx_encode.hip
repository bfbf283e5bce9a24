// tx_encode.hip — K5: fused TX encode + checksum for a burst of send
// descriptors (gfx950).  The reference frames every datagram and segment on the
// protocol lcore and checksums it there:
//   ng_encode_udp_apppkt  udp.c:59-98      ng_encode_tcp_apppkt  tcp.c:420-466
//   ng_encode_arp_pkt     common.c:206-241
// Here one pass turns a 48-B descriptor (rxg_txd) and a payload that is already
// on the device into the complete frame: header synthesised from the
// descriptor, payload read once, both checksums (as K2, tx_cksum.hip) filled,
// zero fill to the frame's 64-B slot end, every store a whole 16-B chunk.
//
// Layout pass (txe_units / txe_scan / txe_offsets, or txe_slots for fixed
// slots): frame lengths, their 64-B units, the exclusive scan that packs them
// (as rx_split.hip's gather), d_off / d_len and the totals.  d_len[k] == 0
// marks a skipped descriptor for the encode kernel.
//
// Encode kernel: a group of G lanes per descriptor, lane k producing output
// chunks k, k+G, ... of the frame.  The payload starts at frame offset 42 or
// 54 + 4*optlen, always 2 mod 4, so output chunk c is a byte funnel of source
// chunks c-hc and c-hc+1 (hc = header chunks).  Lane k loads the upper one; the
// lower one is its left neighbour's (NB = 1: rotated within the group,
// quad-perm DPP or ds_bpermute; the group's lane 0 takes the last lane's of the
// pass before) or a second load of its own that hits L1/L2 (NB = 0).  Both
// checksums are exact integer partial sums over frame coordinates, added over
// the group with DPP, so they equal K2's whatever the split.  The L4 checksum
// sits in the first 64-B sector and depends on the whole payload: the first P
// passes are held in registers and stored after the reduction; longer frames
// stream their tail chunks out as they are produced, sector 0 goes last.
//
// TCP segmentation (rxg_tx_encode_tso_dev) is a sibling of both halves further
// down: a layout pass over entries and units, and tx_encode_tso_kernel with a
// lane group per entry.  The kernels above it are not touched by it.
//
// IPv4 fragmentation of UDP datagrams (rxg_tx_encode_frag_dev) is the same pair
// once more, with both cuts in one place (txe_frag_cut_of), and a finish kernel
// that adds the fragments' partial sums into the datagram's one UDP checksum.
#include <hip/hip_runtime.h>

#include "rx_common.h"
#include "rx_device.h"

namespace {

constexpr uint32_t TXE_CHUNK = 4096, TXE_PER_THREAD = TXE_CHUNK / 256;
constexpr uint32_t TXE_PARTS = 1024; // blocks of the offsets / slots kernels (they stride over chunks)

// one layout block's share of the totals (workspace; txe_totals_kernel adds
// them up: no atomics, a wave-level atomic per 64 descriptors on three shared
// words cost 6 ms per 16M descriptors)
struct txe_part {
    unsigned long long end_units; // end of its last written frame, 64-B units
    unsigned long long written;
};

// frame length of a descriptor from its third chunk (bytes 32..47: .y = hdrlen
// | flags << 8 | optlen << 16 | kind << 24, .w = pay_len); 0 = skipped
__device__ __forceinline__ uint32_t txe_frame_len(uint4 d2, uint32_t slot) {
    const uint32_t kind = d2.y >> 24, opt = (d2.y >> 16) & 0xFFu;
    uint64_t fl = 0;
    if (kind == RXG_TXD_UDP) fl = 42ull + d2.w;
    else if (kind == RXG_TXD_TCP) fl = 54ull + 4ull * opt + d2.w;
    else if (kind == RXG_TXD_ARP) fl = 42ull;
    if (fl > 65535ull || (slot && fl > slot)) fl = 0;
    return (uint32_t)fl;
}

// per-chunk sums of the 64-B units of descriptors [0, n)
__global__ __launch_bounds__(256) void txe_units_kernel(const uint4 *__restrict__ txd, uint32_t n,
                                                        unsigned long long *__restrict__ sums) {
    __shared__ uint32_t part[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * TXE_CHUNK;
    uint32_t s = 0;
    for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
        const uint64_t q = c0 + (uint64_t)k * 256 + tid;
        if (q < n) s += (txe_frame_len(txd[3 * q + 2], 0) + 63u) >> 6;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63u) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = (unsigned long long)part[0] + part[1] + part[2] + part[3];
}

// exclusive prefix sum of v[0..m) in place, one 1024-thread block
__global__ __launch_bounds__(1024) void txe_scan_kernel(unsigned long long *__restrict__ v,
                                                        uint64_t m) {
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t b = tid * per < m ? tid * per : m, e = b + per < m ? b + per : m;
    unsigned long long s = 0;
    for (uint64_t i = b; i < e; ++i) s += v[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const unsigned long long x = tid >= o ? part[tid - o] : 0ull;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    unsigned long long run = part[tid] - s;
    for (uint64_t i = b; i < e; ++i) {
        const unsigned long long x = v[i];
        v[i] = run;
        run += x;
    }
}

// the block's share of the totals into part[blockIdx.x] (every thread calls)
__device__ __forceinline__ void txe_block_part(txe_part *part, uint32_t wr, unsigned long long end) {
    __shared__ unsigned long long s_end[4];
    __shared__ uint32_t s_wr[4];
    for (int o = 32; o > 0; o >>= 1) {
        wr += __shfl_xor(wr, o);
        const unsigned long long y = __shfl_xor(end, o);
        end = y > end ? y : end;
    }
    if ((threadIdx.x & 63u) == 0) s_end[threadIdx.x >> 6] = end, s_wr[threadIdx.x >> 6] = wr;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) end = s_end[w] > end ? s_end[w] : end;
        part[blockIdx.x].end_units = end;
        part[blockIdx.x].written = (unsigned long long)s_wr[0] + s_wr[1] + s_wr[2] + s_wr[3];
    }
}

// d_totals = {frames written, span bytes low, high, frames skipped} from the
// layout blocks' parts; one block
__global__ __launch_bounds__(256) void txe_totals_kernel(const txe_part *__restrict__ part,
                                                         uint32_t nparts, uint32_t n,
                                                         uint32_t *__restrict__ totals) {
    __shared__ unsigned long long s_end[4], s_wr[4];
    unsigned long long end = 0, wr = 0;
    for (uint32_t i = threadIdx.x; i < nparts; i += 256) {
        end = part[i].end_units > end ? part[i].end_units : end;
        wr += part[i].written;
    }
    for (int o = 32; o > 0; o >>= 1) {
        wr += __shfl_xor(wr, o);
        const unsigned long long y = __shfl_xor(end, o);
        end = y > end ? y : end;
    }
    if ((threadIdx.x & 63u) == 0) s_end[threadIdx.x >> 6] = end, s_wr[threadIdx.x >> 6] = wr;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) end = s_end[w] > end ? s_end[w] : end;
        wr = s_wr[0] + s_wr[1] + s_wr[2] + s_wr[3];
        totals[0] = (uint32_t)wr;
        totals[1] = (uint32_t)(end << 6);
        totals[2] = (uint32_t)(end >> 26);
        totals[3] = n - (uint32_t)wr;
    }
}

// packed offsets (64-B units) and lengths, in order inside each chunk; a frame
// that would end past cap_units is skipped, and so is every later one (their
// scanned positions lie past it)
__global__ __launch_bounds__(256) void txe_offsets_kernel(const uint4 *__restrict__ txd, uint32_t n,
                                                          const unsigned long long *__restrict__ base,
                                                          unsigned long long cap_units,
                                                          uint32_t *__restrict__ off,
                                                          uint16_t *__restrict__ len,
                                                          uint32_t nchunks,
                                                          txe_part *__restrict__ part) {
    __shared__ unsigned long long run;
    __shared__ uint32_t wsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t wr = 0;
    unsigned long long end = 0;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (tid == 0) run = base[chunk]; // (read after the first barrier below)
        const uint64_t c0 = (uint64_t)chunk * TXE_CHUNK;
        for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
            const uint64_t q = c0 + (uint64_t)k * 256 + tid;
            const uint32_t l = q < n ? txe_frame_len(txd[3 * q + 2], 0) : 0u;
            const uint32_t u = (l + 63u) >> 6;
            uint32_t x = u; // inclusive wave scan
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const uint32_t y = __shfl_up(x, o);
                if (lane >= o) x += y;
            }
            if (lane == 63) wsum[wv] = x;
            __syncthreads();
            unsigned long long p = run + x - u;
            for (uint32_t w = 0; w < wv; ++w) p += wsum[w];
            if (q < n) {
                const bool ok = u != 0 && p + u <= cap_units;
                off[q] = ok ? (uint32_t)p : 0u;
                len[q] = ok ? (uint16_t)l : (uint16_t)0;
                wr += ok;
                if (ok && p + u > end) end = p + u;
            }
            __syncthreads();
            if (tid == 0) run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
            __syncthreads();
        }
    }
    txe_block_part(part, wr, end);
}

// fixed slots: frame k at k * slot bytes
__global__ __launch_bounds__(256) void txe_slots_kernel(const uint4 *__restrict__ txd, uint32_t n,
                                                        uint32_t slot, unsigned long long cap,
                                                        uint32_t *__restrict__ off,
                                                        uint16_t *__restrict__ len,
                                                        uint32_t nchunks,
                                                        txe_part *__restrict__ part) {
    uint32_t wr = 0;
    unsigned long long end = 0;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x)
        for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
            const uint64_t q = (uint64_t)chunk * TXE_CHUNK + (uint64_t)k * 256 + threadIdx.x;
            if (q >= n) break;
            const uint32_t l = txe_frame_len(txd[3 * q + 2], slot);
            const unsigned long long at = q * slot;
            const bool ok = l != 0 && at + slot <= cap;
            off[q] = ok ? (uint32_t)(at >> 6) : 0u;
            len[q] = ok ? (uint16_t)l : (uint16_t)0;
            wr += ok;
            if (ok) end = (at >> 6) + ((l + 63u) >> 6);
        }
    txe_block_part(part, wr, end);
}

// ---- the encoder ------------------------------------------------------------

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// header chunk c (frame bytes [16c, 16c + 16)) of the frame of descriptor
// (d0, d1, d2), fl bytes long, both checksum fields 0, bytes past the header 0
__device__ __forceinline__ uint4 txe_header(uint32_t c, uint4 d0, uint4 d1, uint4 d2, uint32_t kind,
                                            uint32_t fl) {
    uint4 h = make_uint4(0, 0, 0, 0);
    const uint32_t smac01 = d0.y >> 16, dmac45 = d0.y & 0xFFFFu;
    if (kind == RXG_TXD_ARP) { // common.c:206-241
        if (c == 0) {
            const bool ones = d0.x == 0xFFFFFFFFu && dmac45 == 0xFFFFu;
            h = make_uint4(ones ? 0u : d0.x, (ones ? 0u : dmac45) | (smac01 << 16), d0.z,
                           0x01000608u); // 08 06 | 00 01
        } else if (c == 1) {
            h = make_uint4(0x04060008u, 0x0100u | (smac01 << 16), d0.z, d0.w);
        } else if (c == 2) {
            h = make_uint4(d0.x, dmac45 | (d1.x << 16), d1.x >> 16, 0u);
        }
        return h;
    }
    const bool tcp = kind == RXG_TXD_TCP;
    if (c == 0) {
        h = make_uint4(d0.x, d0.y, d0.z, 0x00450008u); // 08 00 | 45 00
    } else if (c == 1) { // total length, id 0, frag 0, ttl 64, proto, checksum 0, sip, dip low
        h = make_uint4(rx_bswap16(fl - 14u), (64u << 16) | ((tcp ? 6u : 17u) << 24), d0.w << 16,
                       (d0.w >> 16) | (d1.x << 16));
    } else if (c == 2) {
        const uint32_t sport = d1.y & 0xFFFFu, dport = d1.y >> 16;
        h.x = (d1.x >> 16) | (sport << 16);
        if (tcp) { // seq, ack in network order; hdrlen_off, flags
            const uint32_t sq = bswap32(d1.z), ak = bswap32(d1.w);
            h.y = dport | (sq << 16);
            h.z = (sq >> 16) | (ak << 16);
            h.w = (ak >> 16) | ((d2.y & 0xFFFFu) << 16);
        } else { // dgram_len = 8 + payload, checksum 0
            h.y = dport | (rx_bswap16(fl - 34u) << 16);
        }
    } else if (c == 3 && tcp) { // window as stored (tcp.c:454), checksum 0, urp
        h.x = d2.x & 0xFFFFu;
        h.y = d2.x >> 16;
    }
    return h;
}

// the 16 bytes that start sh = 4k + 2 bytes into the 32 bytes {lo, hi}
__device__ __forceinline__ uint4 txe_funnel(uint4 lo, uint4 hi, uint32_t k) {
    uint32_t a0 = lo.x, a1 = lo.y, a2 = lo.z, a3 = lo.w, a4 = hi.x, a5 = hi.y, a6 = hi.z;
    if (k & 2u) a0 = a2, a1 = a3, a2 = a4, a3 = a5, a4 = a6, a5 = hi.w;
    if (k & 1u) a0 = a1, a1 = a2, a2 = a3, a3 = a4, a4 = a5;
    return make_uint4(__builtin_amdgcn_alignbyte(a1, a0, 2), __builtin_amdgcn_alignbyte(a2, a1, 2),
                      __builtin_amdgcn_alignbyte(a3, a2, 2), __builtin_amdgcn_alignbyte(a4, a3, 2));
}

// x of the group's lane (gl - 1) mod G
template <int G>
__device__ __forceinline__ uint32_t grot(uint32_t x, uint32_t lane) {
    if constexpr (G == 4) {
        return pin(__builtin_amdgcn_update_dpp(0u, x, 0x93, 0xF, 0xF, false)); // quad_perm [3,0,1,2]
    } else {
        const uint32_t src = (lane & ~(uint32_t)(G - 1)) | ((lane + G - 1) & (G - 1));
        return pin((uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)x));
    }
}
template <int G>
__device__ __forceinline__ uint4 grot4(uint4 v, uint32_t lane) {
    return make_uint4(grot<G>(v.x, lane), grot<G>(v.y, lane), grot<G>(v.z, lane),
                      grot<G>(v.w, lane));
}

// what a frame's passes share
struct txe_frame {
    const uint8_t *pb; // payload start
    uint8_t *fb;       // frame start
    int32_t plen;      // payload bytes (0: ARP, skipped)
    int32_t hc;        // header chunks: output chunk c takes source chunks c - hc, c - hc + 1
    uint32_t k;        // funnel shift (4k + 2 bytes)
    int32_t nb;        // bytes to store: the frame rounded up to 64 (0: skipped)
    int32_t lo;        // TSO: the segment's first byte in its source chunk 0 (0, 4, 8, 12)
};

// source chunk a of the payload, bytes outside [0, plen) read as 0 (not loaded).
// TSO: pb is the 16-B chunk that holds the segment's first byte, the segment is
// the bytes [lo, plen) from there; the bytes below lo in chunk 0 belong to the
// segment before and read as 0 too (they lie under the header and would be
// summed into the checksum)
template <bool NT, bool TSO = false>
__device__ __forceinline__ uint4 txe_src(const txe_frame &f, int32_t a) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (a >= 0 && 16 * a < f.plen) {
        v = ldg16<NT>(f.pb + 16 * a);
        if (16 * a + 16 > f.plen) v = chunk_below(v, 16 * a, f.plen);
        if constexpr (TSO) {
            if (a == 0) {
                v.x = f.lo > 0 ? 0u : v.x;
                v.y = f.lo > 4 ? 0u : v.y;
                v.z = f.lo > 8 ? 0u : v.z;
            }
        }
    }
    return v;
}

// IPv4 fragmentation (rxg_tx_encode_frag_dev, further down): what an entry that
// is one fragment of a cut UDP datagram adds to its frame
struct txe_fragx {
    uint32_t mode;  // 0: not a fragment; 1: fragment 0 (42-B header); 2: a later one (34-B header)
    uint32_t id_fo; // IPv4 id | flags / offset << 16, host order
    uint32_t dlen;  // the datagram's length (8 + pay_len)
    uint32_t *psum; // the entry's partial-sum word
};

template <int G, int P, int NB, bool TSO = false, bool FRAG = false>
__device__ __forceinline__ void txe_frame_run(const txe_frame &f, uint4 d0, uint4 d1, uint4 d2,
                                              uint32_t kind, uint32_t fl, uint4 (&own)[P],
                                              uint4 (&prv)[NB ? 1 : P], uint32_t gl, uint32_t lane,
                                              bool no_cksum, const txe_fragx *x = nullptr) {
    static_assert(G >= 4, "sector 0 is held by lanes 0..3 of pass 0");
    constexpr int32_t STEP = 16 * G;
    const int32_t s0 = 16 * (int32_t)gl;
    const bool ipv4 = kind != RXG_TXD_ARP;
    const uint32_t proto = kind == RXG_TXD_TCP ? 6u : 17u;
    uint4 carry = make_uint4(0, 0, 0, 0); // NB: the last lane's chunk of the pass before
    uint32_t ip = 0, acc = 0;
#pragma unroll
    for (int q = 0; q < P; ++q) {
        uint4 lo;
        if constexpr (NB) {
            const uint4 r = grot4<G>(own[q], lane);
            lo = gl == 0 ? carry : r;
            carry = r;
        } else {
            lo = prv[q];
        }
        uint4 v = txe_funnel(lo, own[q], f.k);
        if (q == 0) {
            uint4 h = txe_header(gl, d0, d1, d2, kind, fl);
            if constexpr (FRAG) {
                if (x->mode) { // id and flags / offset; the datagram's length, or no UDP header
                    if (gl == 1) {
                        h.x |= rx_bswap16(x->id_fo & 0xFFFFu) << 16;
                        h.y |= rx_bswap16(x->id_fo >> 16);
                    }
                    if (gl == 2) {
                        h.y = x->mode == 1 ? (h.y & 0xFFFFu) | (rx_bswap16(x->dlen) << 16) : 0u;
                        if (x->mode == 2) h.x &= 0xFFFFu;
                    }
                }
            }
            v.x |= h.x, v.y |= h.y, v.z |= h.z, v.w |= h.w;
            // IPv4 header words [14, 34), the checksum field (24, 25) is 0
            if (gl == 0) ip = v.w >> 16;
            if (gl == 1) ip = add_halves(add_halves(add_halves(0u, v.x), v.y), v.w) + (v.z >> 16);
            if (gl == 2) ip = v.x & 0xFFFFu;
        }
        own[q] = v;
        // L4 words [26, fl): the L4 field is 0, bytes past the frame are 0
        if (q == 0) {
            if (gl == 0) v = make_uint4(0, 0, 0, 0);
            if (gl == 1) v.x = v.y = 0, v.z &= 0xFFFF0000u;
            if constexpr (FRAG) {
                if (x->mode == 2) { // datagram bytes only, [34, fl): the addresses count in fragment 0
                    if (gl == 1) v.z = v.w = 0;
                    if (gl == 2) v.x &= 0xFFFF0000u;
                }
            }
        }
        acc = add_halves(add_halves(add_halves(add_halves(acc, v.x), v.y), v.z), v.w);
    }
    // the tail of a long frame: batches of 4 passes, stored as they are produced
    for (int32_t sb = P * STEP; sb < f.nb; sb += 4 * STEP) { // group-uniform
        uint4 r[4], p[NB ? 1 : 4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t a = ((s0 + sb + u * STEP) >> 4) - f.hc + 1;
            r[u] = txe_src<NB != 0, TSO>(f, a);
            if constexpr (!NB) p[u] = txe_src<false, TSO>(f, a - 1);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t s = s0 + sb + u * STEP;
            uint4 lo;
            if constexpr (NB) {
                const uint4 rr = grot4<G>(r[u], lane);
                lo = gl == 0 ? carry : rr;
                carry = rr;
            } else {
                lo = p[u];
            }
            const uint4 v = txe_funnel(lo, r[u], f.k);
            acc = add_halves(add_halves(add_halves(add_halves(acc, v.x), v.y), v.z), v.w);
            if (s < f.nb) stg16(reinterpret_cast<uint4 *>(f.fb + s), v);
        }
    }
    ip = gsum<G>(ip); // group totals in every lane of the group
    acc = gsum<G>(acc);
    if (f.nb == 0) return;
    if (ipv4 && !no_cksum) {
        const uint32_t l4n = fl - 34u;
        // rte_ipv4_cksum as compiled into the reference: the plain complement
        // (a header summing to 0xFFFF stores 0), see tx_cksum.hip
        const uint32_t hip = ~fold16(ip) & 0xFFFFu;
        if constexpr (FRAG) {
            // a fragment's sum of its datagram bytes; the checksum is txe_frag_finish_kernel's
            if (x->mode && gl == 0) *x->psum = fold16(acc);
        }
        acc += (proto << 8) + rx_bswap16(l4n); // pseudo-header {0, proto}, be16(l4 len)
        uint32_t kl4 = (~fold16(acc)) & 0xFFFFu; // rte_ipv4_udptcp_cksum, rte_ip.h:325-349
        if (kl4 == 0u && proto == 17u) kl4 = 0xFFFFu;
        if constexpr (FRAG) {
            if (x->mode) kl4 = 0u;
        }
        if (gl == 1) own[0].z |= hip;                     // bytes 24,25
        if (gl == 2 && proto == 17u) own[0].z |= kl4;     // 40,41
        if (gl == 3 && proto == 6u) own[0].x |= kl4 << 16; // 50,51
    }
#pragma unroll
    for (int q = P - 1; q >= 0; --q) { // sector 0 last
        const int32_t s = s0 + q * STEP;
        if (s < f.nb) stg16(reinterpret_cast<uint4 *>(f.fb + s), own[q]);
    }
}

template <int G, int P, int FPG, int NB>
__global__ __launch_bounds__(256) void tx_encode_kernel(const uint4 *__restrict__ txd,
                                                        const uint8_t *__restrict__ pay,
                                                        uint8_t *__restrict__ pkts,
                                                        const uint32_t *__restrict__ off,
                                                        const uint16_t *__restrict__ len, uint32_t n,
                                                        uint32_t flags) {
    constexpr uint32_t GPB = 256 / G, TILE = GPB * FPG;
    constexpr int32_t STEP = 16 * G;
    const uint32_t tid = threadIdx.x, gl = tid & (G - 1), grp = tid / G, lane = tid & 63u;
    const int32_t s0 = 16 * (int32_t)gl;
    for (uint64_t tile = blockIdx.x; tile * TILE < n; tile += gridDim.x) {
        txe_frame f[FPG];
        uint4 d0[FPG], d1[FPG], d2[FPG];
        uint32_t kind[FPG], fl[FPG];
        uint4 own[FPG][P], prv[FPG][NB ? 1 : P];
#pragma unroll
        for (int i = 0; i < FPG; ++i) {
            const uint64_t pos = tile * TILE + (uint64_t)i * GPB + grp;
            const uint64_t q = pos < n ? pos : 0;
            fl[i] = pos < n ? (uint32_t)len[q] : 0u;
            d0[i] = txd[3 * q], d1[i] = txd[3 * q + 1], d2[i] = txd[3 * q + 2];
            kind[i] = d2[i].y >> 24;
            const uint32_t hdr = kind[i] == RXG_TXD_TCP ? 54u + 4u * ((d2[i].y >> 16) & 0xFFu) : 42u;
            f[i].fb = pkts + ((uint64_t)off[q] << 6);
            f[i].pb = pay + ((uint64_t)d2[i].z << 4);
            f[i].plen = (fl[i] == 0 || kind[i] == RXG_TXD_ARP) ? 0 : (int32_t)(fl[i] - hdr);
            f[i].hc = (int32_t)((hdr + 15u) >> 4);
            f[i].k = ((16u - (hdr & 15u)) - 2u) >> 2;
            f[i].nb = (int32_t)((fl[i] + 63u) & ~63u);
        }
        // every pass of every frame in flight before the first is consumed
#pragma unroll
        for (int i = 0; i < FPG; ++i)
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const int32_t a = ((s0 + q * STEP) >> 4) - f[i].hc + 1;
                own[i][q] = txe_src<NB != 0>(f[i], a);
                if constexpr (!NB) prv[i][q] = txe_src<false>(f[i], a - 1);
            }
#pragma unroll
        for (int i = 0; i < FPG; ++i)
            txe_frame_run<G, P, NB>(f[i], d0[i], d1[i], d2[i], kind[i], fl[i], own[i], prv[i], gl,
                                    lane, (flags & RXG_TXE_NO_CKSUM) != 0);
    }
}

constexpr uint32_t TXE_FULL_GRID = 1000;
template <int G, int P, int FPG, int NB>
hipError_t launch_txe(const uint4 *txd, const uint8_t *pay, uint8_t *pkts, const uint32_t *off,
                      const uint16_t *len, uint32_t n, uint32_t flags, uint32_t bpc_cap,
                      hipStream_t s) {
    constexpr uint32_t TILE = (256 / G) * FPG;
    int cu = 0, occ = 0;
    hipError_t e = rx_occupancy(reinterpret_cast<const void *>(tx_encode_kernel<G, P, FPG, NB>),
                                256, 0, &cu, &occ);
    if (e != hipSuccess) return e;
    const uint64_t tiles = ((uint64_t)n + TILE - 1) / TILE;
    uint64_t bpc = (uint64_t)occ;
    if (bpc_cap && bpc > bpc_cap) bpc = bpc_cap;
    uint64_t blocks = (uint64_t)cu * bpc;
    if (blocks > tiles || bpc_cap == TXE_FULL_GRID) blocks = tiles;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((tx_encode_kernel<G, P, FPG, NB>), dim3((uint32_t)blocks), dim3(256), 0, s,
                       txd, pay, pkts, off, len, n, flags);
    return hipGetLastError();
}

typedef hipError_t (*txe_launch_fn)(const uint4 *, const uint8_t *, uint8_t *, const uint32_t *,
                                    const uint16_t *, uint32_t, uint32_t, uint32_t, hipStream_t);
struct txe_variant {
    txe_launch_fn fn;
    uint32_t bpc; // resident blocks per CU cap (0 = occupancy)
};
// {G, passes held, frames per group, neighbour mode}, grid.  0..3 are K2's
// shapes per class, 4..7 the same with the second load instead of the in-group
// rotate, the rest one block per tile and other widths.  Defaults, measured
// (tools/txe_sweep.py, profiles/k5/txe_sweep.txt; whole call, layout pass
// included, medians of 5 interleaved rounds):
//   64 B    (cfg2, 16M frames)  8: 0.679 ms   0: 0.726   4: 0.783   9: 0.970
//   IMIX    (cfg4, 16M, packed) 9: 2.933      2: 3.265   10: 3.420  8: 3.529
//   1500 B  (cfg3, 4M)          11: 2.311     3: 2.331   2: 2.365   7: 2.442   13: 2.442
//   9000 B  (cfg5, 1.25M)       13: 4.301     12: 4.315  7: 4.437   3: 4.529   11: 4.589
// The rotate beats the second load at 64 B and 1500 B (0 vs 4, 3 vs 7); on
// jumbo frames the two tie and change places from run to run (12 / 13: 4.315 /
// 4.301, 4.230 / 4.369, 4.515 / 4.338 in three runs), and the default stays the
// rotate, which fetches every source chunk once.  128 B was not measured: that
// class keeps K2's shape (1).
static const txe_variant k_txe[] = {
    {launch_txe<4, 1, 4, 1>, 0},              {launch_txe<4, 2, 2, 1>, 0},
    {launch_txe<8, 12, 1, 1>, 0},             {launch_txe<16, 8, 1, 1>, 0},
    {launch_txe<4, 1, 4, 0>, 0},              {launch_txe<4, 2, 2, 0>, 0},
    {launch_txe<8, 12, 1, 0>, 0},             {launch_txe<16, 8, 1, 0>, 0},
    {launch_txe<4, 1, 1, 1>, TXE_FULL_GRID},  {launch_txe<8, 1, 1, 1>, TXE_FULL_GRID},
    {launch_txe<8, 4, 2, 1>, 0},              {launch_txe<16, 6, 1, 1>, 0},
    {launch_txe<32, 4, 1, 1>, 0},             {launch_txe<32, 4, 1, 0>, 0},
    {launch_txe<8, 1, 1, 0>, TXE_FULL_GRID},
};

// ---- TCP segmentation (rxg_tx_encode_tso_dev) --------------------------------
// A TCP descriptor longer than mss becomes s frames.  The layout pass scans two
// quantities, entries (max(1, s)) and 64-B units, and writes off / len per
// entry, first / nseg per descriptor and the entry -> descriptor map the
// encoder reads; the encoder is tx_encode_kernel with a lane group per entry.
// Segment j starts D = j * mss bytes into a 16-B aligned payload; mss % 4 == 0
// keeps D 4-B aligned, so with every source load still a 16-B aligned chunk
// (from pb + (D & ~15)) the payload's place in the frame stays 2 mod 4 against
// the source chunks: the funnel applies with hc / k taken from hdr - (D & 15),
// and the (D & 15) bytes before the segment in source chunk 0 read as 0.

// how a descriptor is cut, from its third chunk: s segments (0 = skipped), the
// frame length of every segment but the last, and of the last
struct txe_cut {
    unsigned long long s;
    uint32_t full, last;
};
__device__ __forceinline__ txe_cut txe_cut_of(uint4 d2, uint32_t mss, uint32_t slot) {
    const uint32_t kind = d2.y >> 24, opt = (d2.y >> 16) & 0xFFu, pay = d2.w;
    txe_cut c;
    uint64_t full = 0, last = 0;
    c.s = 1;
    if (kind == RXG_TXD_TCP && mss) {
        const uint32_t hdr = 54u + 4u * opt;
        if (pay) c.s = ((uint64_t)pay + mss - 1) / mss;
        full = (uint64_t)hdr + (pay < mss ? pay : mss);
        last = (uint64_t)hdr + (pay - (c.s - 1) * mss);
    } else {
        if (kind == RXG_TXD_UDP) full = 42ull + pay;
        else if (kind == RXG_TXD_TCP) full = 54ull + 4ull * opt + pay;
        else if (kind == RXG_TXD_ARP) full = 42ull;
        last = full;
    }
    if (full == 0 || full > 65535ull || (slot && full > slot)) c.s = 0;
    c.full = c.s ? (uint32_t)full : 0u;
    c.last = c.s ? (uint32_t)last : 0u;
    return c;
}
__device__ __forceinline__ unsigned long long txe_cut_units(const txe_cut &c) {
    return c.s ? (c.s - 1) * ((c.full + 63u) >> 6) + ((c.last + 63u) >> 6) : 0ull;
}

struct txe_tso_part {
    unsigned long long end_units; // end of its last written frame, 64-B units
    unsigned long long frames, descs; // written
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// per-chunk sums of the entries (sums_e) and 64-B units (sums_u) of descriptors [0, n)
__global__ __launch_bounds__(256) void txe_tso_sums_kernel(const uint4 *__restrict__ txd, uint32_t n,
                                                           uint32_t mss, uint32_t slot,
                                                           unsigned long long *__restrict__ sums_e,
                                                           unsigned long long *__restrict__ sums_u) {
    __shared__ unsigned long long pe[4], pu[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * TXE_CHUNK;
    unsigned long long se = 0, su = 0;
    for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
        const uint64_t q = c0 + (uint64_t)k * 256 + tid;
        if (q < n) {
            const txe_cut c = txe_cut_of(txd[3 * q + 2], mss, slot);
            se += c.s ? c.s : 1ull;
            su += txe_cut_units(c);
        }
    }
    se = wave_sum64(se), su = wave_sum64(su);
    if ((tid & 63u) == 0) pe[tid >> 6] = se, pu[tid >> 6] = su;
    __syncthreads();
    if (tid == 0) {
        sums_e[blockIdx.x] = pe[0] + pe[1] + pe[2] + pe[3];
        sums_u[blockIdx.x] = pu[0] + pu[1] + pu[2] + pu[3];
    }
}

// txe_scan_kernel over the array v + blockIdx.x * (m + 1), the total left in its
// slot m: one launch scans the entries and the units
__global__ __launch_bounds__(1024) void txe_tso_scan_kernel(unsigned long long *__restrict__ v_,
                                                            uint64_t m) {
    __shared__ unsigned long long part[1024];
    unsigned long long *v = v_ + (uint64_t)blockIdx.x * (m + 1);
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (m + 1023) / 1024;
    const uint64_t b = tid * per < m ? tid * per : m, e = b + per < m ? b + per : m;
    unsigned long long s = 0;
    for (uint64_t i = b; i < e; ++i) s += v[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const unsigned long long x = tid >= o ? part[tid - o] : 0ull;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    unsigned long long run = part[tid] - s;
    for (uint64_t i = b; i < e; ++i) {
        const unsigned long long x = v[i];
        v[i] = run;
        run += x;
    }
    if (tid == 1023) v[m] = part[1023];
}

// entries and positions in order inside each chunk.  A descriptor is written
// iff s > 0, its entries end at or below out_cap and its frames fit the
// capacity; both limits, once passed, stay passed for every later descriptor
// that has frames (their scanned positions lie past them).  Per descriptor:
// first, nseg and (workspace) the packed position of its first frame; the
// entries are written by txe_tso_entries_kernel, a thread per entry.
__global__ __launch_bounds__(256) void txe_tso_layout_kernel(
    const uint4 *__restrict__ txd, uint32_t n, uint32_t mss, uint32_t slot,
    const unsigned long long *__restrict__ base_e, const unsigned long long *__restrict__ base_u,
    unsigned long long cap, unsigned long long out_cap,
    uint32_t *__restrict__ first, uint32_t *__restrict__ nseg, uint32_t *__restrict__ posu,
    uint32_t nchunks, txe_tso_part *__restrict__ part) {
    __shared__ unsigned long long run_e, run_u, we[4], wu[4];
    __shared__ unsigned long long s_end[4], s_fr[4], s_ds[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long frames = 0, descs = 0, end = 0;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (tid == 0) run_e = base_e[chunk], run_u = base_u[chunk]; // (read after the first barrier)
        const uint64_t c0 = (uint64_t)chunk * TXE_CHUNK;
        for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
            const uint64_t q = c0 + (uint64_t)k * 256 + tid;
            txe_cut c;
            c.s = 0, c.full = c.last = 0;
            if (q < n) c = txe_cut_of(txd[3 * q + 2], mss, slot);
            const unsigned long long ne = q < n ? (c.s ? c.s : 1ull) : 0ull, u = txe_cut_units(c);
            unsigned long long xe = ne, xu = u; // inclusive wave scans
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const unsigned long long ye = __shfl_up(xe, o), yu = __shfl_up(xu, o);
                if (lane >= o) xe += ye, xu += yu;
            }
            if (lane == 63) we[wv] = xe, wu[wv] = xu;
            __syncthreads();
            unsigned long long fe = run_e + xe - ne, pu = run_u + xu - u;
            for (uint32_t w = 0; w < wv; ++w) fe += we[w], pu += wu[w];
            if (q < n) {
                bool ok = c.s != 0 && fe + c.s <= out_cap;
                if (ok) ok = slot ? (fe + c.s) * slot <= cap : ((pu + u) << 6) <= cap;
                first[q] = fe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)fe;
                nseg[q] = ok ? (uint32_t)c.s : 0u;
                posu[q] = (uint32_t)pu; // (a written descriptor's frames end below 2^32 units)
                const unsigned long long fu = (c.full + 63u) >> 6, su = slot >> 6;
                if (ok) {
                    const unsigned long long at = slot ? (fe + c.s - 1) * su : pu + (c.s - 1) * fu;
                    const unsigned long long en = at + ((c.last + 63u) >> 6);
                    frames += c.s, descs += 1;
                    if (en > end) end = en;
                }
            }
            __syncthreads();
            if (tid == 0) {
                run_e += we[0] + we[1] + we[2] + we[3];
                run_u += wu[0] + wu[1] + wu[2] + wu[3];
            }
            __syncthreads();
        }
    }
    frames = wave_sum64(frames), descs = wave_sum64(descs);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(end, o);
        end = y > end ? y : end;
    }
    if (lane == 0) s_end[wv] = end, s_fr[wv] = frames, s_ds[wv] = descs;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) end = s_end[w] > end ? s_end[w] : end;
        part[blockIdx.x].end_units = end;
        part[blockIdx.x].frames = s_fr[0] + s_fr[1] + s_fr[2] + s_fr[3];
        part[blockIdx.x].descs = s_ds[0] + s_ds[1] + s_ds[2] + s_ds[3];
    }
}

// off / len / map of the entries laid out (those below out_cap), a thread per
// entry: its descriptor is the last one whose first is not above it (first is
// ascending; a binary search over an array that stays in the caches), the
// segment number the distance.  The layout loop of a 45-segment descriptor is
// 45 threads here, not 45 trips of one.
__global__ __launch_bounds__(256) void txe_tso_entries_kernel(
    const uint4 *__restrict__ txd, uint32_t n, uint32_t mss, uint32_t slot,
    const uint32_t *__restrict__ first, const uint32_t *__restrict__ nseg,
    const uint32_t *__restrict__ posu, const unsigned long long *__restrict__ need,
    unsigned long long out_cap, uint32_t *__restrict__ off, uint16_t *__restrict__ len,
    uint32_t *__restrict__ map) {
    const unsigned long long ne = *need < out_cap ? *need : out_cap;
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < ne;
         e += (unsigned long long)gridDim.x * 256) {
        // first[0] == 0 <= e; descriptor q owns at least one entry, so q <= e
        uint32_t lo = 0, hi = e < n - 1 ? (uint32_t)e : n - 1;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo + 1) >> 1);
            if (first[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t q = lo, s = nseg[q], j = (uint32_t)e - first[q];
        uint32_t o = 0, l = 0;
        if (s) {
            const uint4 d2 = txd[3 * (uint64_t)q + 2];
            const uint32_t kind = d2.y >> 24, pay = d2.w;
            if (kind == RXG_TXD_TCP && mss) {
                const uint32_t hdr = 54u + 4u * ((d2.y >> 16) & 0xFFu);
                const uint32_t full = hdr + (pay < mss ? pay : mss);
                l = j + 1 == s ? hdr + (pay - (s - 1) * mss) : full;
                o = slot ? (uint32_t)(e * (slot >> 6)) : posu[q] + j * ((full + 63u) >> 6);
            } else {
                l = kind == RXG_TXD_TCP ? 54u + 4u * ((d2.y >> 16) & 0xFFu) + pay
                                        : (kind == RXG_TXD_UDP ? 42u + pay : 42u);
                o = slot ? (uint32_t)(e * (slot >> 6)) : posu[q];
            }
        }
        map[e] = q;
        off[e] = o;
        len[e] = (uint16_t)l;
    }
}

// d_totals = {frames written, span bytes low, high, descriptors skipped,
// entries needed low, high, 0, 0}; one block
__global__ __launch_bounds__(256) void txe_tso_totals_kernel(const txe_tso_part *__restrict__ part,
                                                             uint32_t nparts, uint32_t n,
                                                             const unsigned long long *__restrict__ need,
                                                             uint32_t *__restrict__ totals) {
    __shared__ unsigned long long s_end[4], s_fr[4], s_ds[4];
    unsigned long long end = 0, fr = 0, ds = 0;
    for (uint32_t i = threadIdx.x; i < nparts; i += 256) {
        end = part[i].end_units > end ? part[i].end_units : end;
        fr += part[i].frames, ds += part[i].descs;
    }
    fr = wave_sum64(fr), ds = wave_sum64(ds);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(end, o);
        end = y > end ? y : end;
    }
    if ((threadIdx.x & 63u) == 0)
        s_end[threadIdx.x >> 6] = end, s_fr[threadIdx.x >> 6] = fr, s_ds[threadIdx.x >> 6] = ds;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) end = s_end[w] > end ? s_end[w] : end;
        totals[0] = (uint32_t)(s_fr[0] + s_fr[1] + s_fr[2] + s_fr[3]);
        totals[1] = (uint32_t)(end << 6);
        totals[2] = (uint32_t)(end >> 26);
        totals[3] = n - (uint32_t)(s_ds[0] + s_ds[1] + s_ds[2] + s_ds[3]);
        totals[4] = (uint32_t)*need;
        totals[5] = (uint32_t)(*need >> 32);
        totals[6] = totals[7] = 0u;
    }
}

// tx_encode_kernel with a lane group per entry: the descriptor is map[e], the
// segment e - first[map[e]]; seq and the flag mask go into the descriptor's
// registers before the header chunk is built from them
template <int G, int P, int FPG, int NB>
__global__ __launch_bounds__(256) void tx_encode_tso_kernel(
    const uint4 *__restrict__ txd, const uint8_t *__restrict__ pay, uint8_t *__restrict__ pkts,
    const uint32_t *__restrict__ off, const uint16_t *__restrict__ len,
    const uint32_t *__restrict__ map, const uint32_t *__restrict__ first,
    const unsigned long long *__restrict__ need, unsigned long long out_cap, uint32_t mss,
    uint32_t flags) {
    constexpr uint32_t GPB = 256 / G, TILE = GPB * FPG;
    constexpr int32_t STEP = 16 * G;
    const uint32_t tid = threadIdx.x, gl = tid & (G - 1), grp = tid / G, lane = tid & 63u;
    const int32_t s0 = 16 * (int32_t)gl;
    const unsigned long long ne = *need < out_cap ? *need : out_cap; // entries laid out
    for (uint64_t tile = blockIdx.x; tile * TILE < ne; tile += gridDim.x) {
        txe_frame f[FPG];
        uint4 d0[FPG], d1[FPG], d2[FPG];
        uint32_t kind[FPG], fl[FPG];
        uint4 own[FPG][P], prv[FPG][NB ? 1 : P];
#pragma unroll
        for (int i = 0; i < FPG; ++i) {
            const uint64_t pos = tile * TILE + (uint64_t)i * GPB + grp;
            const uint64_t e = pos < ne ? pos : 0;
            fl[i] = pos < ne ? (uint32_t)len[e] : 0u;
            const uint64_t q = map[e];
            const uint32_t j = (uint32_t)e - first[q];
            d0[i] = txd[3 * q], d1[i] = txd[3 * q + 1], d2[i] = txd[3 * q + 2];
            kind[i] = d2[i].y >> 24;
            const uint32_t hdr = kind[i] == RXG_TXD_TCP ? 54u + 4u * ((d2[i].y >> 16) & 0xFFu) : 42u;
            const uint32_t seg = (fl[i] == 0 || kind[i] == RXG_TXD_ARP) ? 0u : fl[i] - hdr;
            uint32_t dd = 0; // the segment's first byte in the payload
            if (kind[i] == RXG_TXD_TCP && mss) {
                dd = j * mss;
                d1[i].z += dd;
                if ((uint64_t)dd + seg < d2[i].w) d2[i].y &= ~(0x09u << 8); // not the last: FIN, PSH
            }
            const uint32_t r = dd & 15u, hv = hdr - r;
            f[i].fb = pkts + ((uint64_t)off[e] << 6);
            f[i].pb = pay + ((uint64_t)d2[i].z << 4) + (dd & ~15u);
            f[i].plen = seg ? (int32_t)(r + seg) : 0;
            f[i].lo = (int32_t)r;
            f[i].hc = (int32_t)((hv + 15u) >> 4);
            f[i].k = ((16u - (hv & 15u)) - 2u) >> 2;
            f[i].nb = (int32_t)((fl[i] + 63u) & ~63u);
        }
#pragma unroll
        for (int i = 0; i < FPG; ++i)
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const int32_t a = ((s0 + q * STEP) >> 4) - f[i].hc + 1;
                own[i][q] = txe_src<NB != 0, true>(f[i], a);
                if constexpr (!NB) prv[i][q] = txe_src<false, true>(f[i], a - 1);
            }
#pragma unroll
        for (int i = 0; i < FPG; ++i)
            txe_frame_run<G, P, NB, true>(f[i], d0[i], d1[i], d2[i], kind[i], fl[i], own[i], prv[i],
                                          gl, lane, (flags & RXG_TXE_NO_CKSUM) != 0);
    }
}

template <int G, int P, int FPG, int NB>
hipError_t launch_txe_tso(const uint4 *txd, const uint8_t *pay, uint8_t *pkts, const uint32_t *off,
                          const uint16_t *len, const uint32_t *map, const uint32_t *first,
                          const unsigned long long *need, uint32_t out_cap, uint32_t mss,
                          uint32_t flags, uint32_t bpc_cap, hipStream_t s) {
    constexpr uint32_t TILE = (256 / G) * FPG;
    int cu = 0, occ = 0;
    hipError_t e = rx_occupancy(reinterpret_cast<const void *>(tx_encode_tso_kernel<G, P, FPG, NB>),
                                256, 0, &cu, &occ);
    if (e != hipSuccess) return e;
    // the entry count is on the device: the grid is sized for out_cap, blocks
    // past the entries laid out leave at once
    const uint64_t tiles = ((uint64_t)out_cap + TILE - 1) / TILE;
    uint64_t bpc = (uint64_t)occ;
    if (bpc_cap && bpc > bpc_cap) bpc = bpc_cap;
    uint64_t blocks = (uint64_t)cu * bpc;
    if (blocks > tiles || bpc_cap == TXE_FULL_GRID) blocks = tiles;
    if (blocks > 0x7FFFFFFFull) blocks = 0x7FFFFFFFull; // (the tile loop strides)
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL((tx_encode_tso_kernel<G, P, FPG, NB>), dim3((uint32_t)blocks), dim3(256), 0, s,
                       txd, pay, pkts, off, len, map, first, need, (unsigned long long)out_cap, mss,
                       flags);
    return hipGetLastError();
}

typedef hipError_t (*txe_tso_launch_fn)(const uint4 *, const uint8_t *, uint8_t *, const uint32_t *,
                                        const uint16_t *, const uint32_t *, const uint32_t *,
                                        const unsigned long long *, uint32_t, uint32_t, uint32_t,
                                        uint32_t, hipStream_t);
// the shapes of k_txe, index for index (rxg_tune_txe and len_hint choose both)
static const txe_tso_launch_fn k_txe_tso[] = {
    launch_txe_tso<4, 1, 4, 1>,  launch_txe_tso<4, 2, 2, 1>,  launch_txe_tso<8, 12, 1, 1>,
    launch_txe_tso<16, 8, 1, 1>, launch_txe_tso<4, 1, 4, 0>,  launch_txe_tso<4, 2, 2, 0>,
    launch_txe_tso<8, 12, 1, 0>, launch_txe_tso<16, 8, 1, 0>, launch_txe_tso<4, 1, 1, 1>,
    launch_txe_tso<8, 1, 1, 1>,  launch_txe_tso<8, 4, 2, 1>,  launch_txe_tso<16, 6, 1, 1>,
    launch_txe_tso<32, 4, 1, 1>, launch_txe_tso<32, 4, 1, 0>, launch_txe_tso<8, 1, 1, 0>,
};
static_assert(sizeof(k_txe_tso) / sizeof(k_txe_tso[0]) == sizeof(k_txe) / sizeof(k_txe[0]),
              "one TSO kernel per k_txe entry");

// ---- IPv4 fragmentation of UDP datagrams (rxg_tx_encode_frag_dev) -------------
// The second cut: a UDP descriptor whose datagram (L = 8 + pay_len bytes, the
// UDP header included) does not fit the IPv4 MTU becomes s fragments of
// fp = (mtu - 20) & ~7 datagram bytes.  Fragment 0 is the 42-B header and the
// payload from its start; fragment j > 0 a 34-B header and the payload from
// D = j * fp - 8, a multiple of 8: hc / k / lo from 34 - (D & 15) as TSO takes
// them from hdr - (D & 15), and the payload still lands 2 mod 4.  The layout
// pass is the TSO one with txe_frag_cut_of in txe_cut_of's place.  The one
// UDP checksum of a cut datagram covers bytes that s lane groups write: each
// leaves the folded sum of its datagram bytes in a workspace word per entry
// (fragment 0 with the address words, as every frame's sum has them), and
// txe_frag_finish_kernel adds them up behind the encoder and stores the two
// bytes at offset 40 of fragment 0.

// txe_cut_of with both cuts; *fp = the fragment's datagram bytes, 0 = not a cut
// UDP datagram (one place: sums, layout, entries and the encoder ask it)
__device__ __forceinline__ txe_cut txe_frag_cut_of(uint4 d2, uint32_t mss, uint32_t mtu,
                                                   uint32_t slot, uint32_t *fp) {
    const uint32_t kind = d2.y >> 24, pay = d2.w;
    *fp = 0;
    if (kind != RXG_TXD_UDP || mtu == 0 || 28ull + pay <= mtu) return txe_cut_of(d2, mss, slot);
    const uint32_t f = (mtu - 20u) & ~7u;
    *fp = f;
    txe_cut c;
    c.s = 0, c.full = c.last = 0;
    if (28ull + pay > 65535ull) return c; // no IPv4 datagram is that long
    const uint32_t L = 8u + pay, s = (L + f - 1u) / f; // (L > mtu - 20 >= f: s >= 2)
    const uint32_t full = 34u + f;
    if (full > 65535u || (slot && full > slot)) return c;
    c.s = s, c.full = full, c.last = 34u + (L - (s - 1u) * f);
    return c;
}

__global__ __launch_bounds__(256) void txe_frag_sums_kernel(const uint4 *__restrict__ txd, uint32_t n,
                                                            uint32_t mss, uint32_t mtu, uint32_t slot,
                                                            unsigned long long *__restrict__ sums_e,
                                                            unsigned long long *__restrict__ sums_u) {
    __shared__ unsigned long long pe[4], pu[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * TXE_CHUNK;
    unsigned long long se = 0, su = 0;
    for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
        const uint64_t q = c0 + (uint64_t)k * 256 + tid;
        if (q < n) {
            uint32_t fp;
            const txe_cut c = txe_frag_cut_of(txd[3 * q + 2], mss, mtu, slot, &fp);
            se += c.s ? c.s : 1ull;
            su += txe_cut_units(c);
        }
    }
    se = wave_sum64(se), su = wave_sum64(su);
    if ((tid & 63u) == 0) pe[tid >> 6] = se, pu[tid >> 6] = su;
    __syncthreads();
    if (tid == 0) {
        sums_e[blockIdx.x] = pe[0] + pe[1] + pe[2] + pe[3];
        sums_u[blockIdx.x] = pu[0] + pu[1] + pu[2] + pu[3];
    }
}

// txe_tso_layout_kernel with both cuts
__global__ __launch_bounds__(256) void txe_frag_layout_kernel(
    const uint4 *__restrict__ txd, uint32_t n, uint32_t mss, uint32_t mtu, uint32_t slot,
    const unsigned long long *__restrict__ base_e, const unsigned long long *__restrict__ base_u,
    unsigned long long cap, unsigned long long out_cap,
    uint32_t *__restrict__ first, uint32_t *__restrict__ nseg, uint32_t *__restrict__ posu,
    uint32_t nchunks, txe_tso_part *__restrict__ part) {
    __shared__ unsigned long long run_e, run_u, we[4], wu[4];
    __shared__ unsigned long long s_end[4], s_fr[4], s_ds[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    unsigned long long frames = 0, descs = 0, end = 0;
    for (uint32_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        if (tid == 0) run_e = base_e[chunk], run_u = base_u[chunk]; // (read after the first barrier)
        const uint64_t c0 = (uint64_t)chunk * TXE_CHUNK;
        for (uint32_t k = 0; k < TXE_PER_THREAD; ++k) {
            const uint64_t q = c0 + (uint64_t)k * 256 + tid;
            txe_cut c;
            c.s = 0, c.full = c.last = 0;
            uint32_t fp;
            if (q < n) c = txe_frag_cut_of(txd[3 * q + 2], mss, mtu, slot, &fp);
            const unsigned long long ne = q < n ? (c.s ? c.s : 1ull) : 0ull, u = txe_cut_units(c);
            unsigned long long xe = ne, xu = u; // inclusive wave scans
            for (uint32_t o = 1; o < 64; o <<= 1) {
                const unsigned long long ye = __shfl_up(xe, o), yu = __shfl_up(xu, o);
                if (lane >= o) xe += ye, xu += yu;
            }
            if (lane == 63) we[wv] = xe, wu[wv] = xu;
            __syncthreads();
            unsigned long long fe = run_e + xe - ne, pu = run_u + xu - u;
            for (uint32_t w = 0; w < wv; ++w) fe += we[w], pu += wu[w];
            if (q < n) {
                bool ok = c.s != 0 && fe + c.s <= out_cap;
                if (ok) ok = slot ? (fe + c.s) * slot <= cap : ((pu + u) << 6) <= cap;
                first[q] = fe > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)fe;
                nseg[q] = ok ? (uint32_t)c.s : 0u;
                posu[q] = (uint32_t)pu; // (a written descriptor's frames end below 2^32 units)
                const unsigned long long fu = (c.full + 63u) >> 6, su = slot >> 6;
                if (ok) {
                    const unsigned long long at = slot ? (fe + c.s - 1) * su : pu + (c.s - 1) * fu;
                    const unsigned long long en = at + ((c.last + 63u) >> 6);
                    frames += c.s, descs += 1;
                    if (en > end) end = en;
                }
            }
            __syncthreads();
            if (tid == 0) {
                run_e += we[0] + we[1] + we[2] + we[3];
                run_u += wu[0] + wu[1] + wu[2] + wu[3];
            }
            __syncthreads();
        }
    }
    frames = wave_sum64(frames), descs = wave_sum64(descs);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(end, o);
        end = y > end ? y : end;
    }
    if (lane == 0) s_end[wv] = end, s_fr[wv] = frames, s_ds[wv] = descs;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) end = s_end[w] > end ? s_end[w] : end;
        part[blockIdx.x].end_units = end;
        part[blockIdx.x].frames = s_fr[0] + s_fr[1] + s_fr[2] + s_fr[3];
        part[blockIdx.x].descs = s_ds[0] + s_ds[1] + s_ds[2] + s_ds[3];
    }
}

// txe_tso_entries_kernel with both cuts: entry j of a written descriptor is
// c.full bytes long but the last, and the frames follow each other
__global__ __launch_bounds__(256) void txe_frag_entries_kernel(
    const uint4 *__restrict__ txd, uint32_t n, uint32_t mss, uint32_t mtu, uint32_t slot,
    const uint32_t *__restrict__ first, const uint32_t *__restrict__ nseg,
    const uint32_t *__restrict__ posu, const unsigned long long *__restrict__ need,
    unsigned long long out_cap, uint32_t *__restrict__ off, uint16_t *__restrict__ len,
    uint32_t *__restrict__ map) {
    const unsigned long long ne = *need < out_cap ? *need : out_cap;
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < ne;
         e += (unsigned long long)gridDim.x * 256) {
        // first[0] == 0 <= e; descriptor q owns at least one entry, so q <= e
        uint32_t lo = 0, hi = e < n - 1 ? (uint32_t)e : n - 1;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo + 1) >> 1);
            if (first[mid] <= e) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t q = lo, s = nseg[q], j = (uint32_t)e - first[q];
        uint32_t o = 0, l = 0;
        if (s) {
            uint32_t fp;
            const txe_cut c = txe_frag_cut_of(txd[3 * (uint64_t)q + 2], mss, mtu, slot, &fp);
            l = j + 1 == s ? c.last : c.full;
            o = slot ? (uint32_t)(e * (slot >> 6)) : posu[q] + j * ((c.full + 63u) >> 6);
        }
        map[e] = q;
        off[e] = o;
        len[e] = (uint16_t)l;
    }
}

// tx_encode_tso_kernel with both cuts: an entry of a cut UDP datagram is one
// fragment, and leaves its partial sum in psum[e]
template <int G, int P, int FPG, int NB>
__global__ __launch_bounds__(256) void tx_encode_frag_kernel(
    const uint4 *__restrict__ txd, const uint8_t *__restrict__ pay, uint8_t *__restrict__ pkts,
    const uint32_t *__restrict__ off, const uint16_t *__restrict__ len,
    const uint32_t *__restrict__ map, const uint32_t *__restrict__ first,
    const unsigned long long *__restrict__ need, unsigned long long out_cap, uint32_t mss,
    uint32_t mtu, uint32_t *__restrict__ psum, uint32_t flags) {
    constexpr uint32_t GPB = 256 / G, TILE = GPB * FPG;
    constexpr int32_t STEP = 16 * G;
    const uint32_t tid = threadIdx.x, gl = tid & (G - 1), grp = tid / G, lane = tid & 63u;
    const int32_t s0 = 16 * (int32_t)gl;
    const unsigned long long ne = *need < out_cap ? *need : out_cap; // entries laid out
    for (uint64_t tile = blockIdx.x; tile * TILE < ne; tile += gridDim.x) {
        txe_frame f[FPG];
        txe_fragx x[FPG];
        uint4 d0[FPG], d1[FPG], d2[FPG];
        uint32_t kind[FPG], fl[FPG];
        uint4 own[FPG][P], prv[FPG][NB ? 1 : P];
#pragma unroll
        for (int i = 0; i < FPG; ++i) {
            const uint64_t pos = tile * TILE + (uint64_t)i * GPB + grp;
            const uint64_t e = pos < ne ? pos : 0;
            fl[i] = pos < ne ? (uint32_t)len[e] : 0u;
            const uint64_t q = map[e];
            const uint32_t j = (uint32_t)e - first[q];
            d0[i] = txd[3 * q], d1[i] = txd[3 * q + 1], d2[i] = txd[3 * q + 2];
            kind[i] = d2[i].y >> 24;
            uint32_t hdr = kind[i] == RXG_TXD_TCP ? 54u + 4u * ((d2[i].y >> 16) & 0xFFu) : 42u;
            uint32_t dd = 0; // the entry's first byte in the payload
            const uint32_t fp = kind[i] == RXG_TXD_UDP && mtu && 28ull + d2[i].w > mtu
                                    ? (mtu - 20u) & ~7u : 0u; // (as txe_frag_cut_of)
            x[i].mode = 0, x[i].id_fo = 0, x[i].dlen = 0, x[i].psum = psum + e;
            if (fp && fl[i]) {
                const uint32_t at = j * fp, L = 8u + d2[i].w;
                x[i].mode = j ? 2u : 1u;
                x[i].dlen = L;
                x[i].id_fo = (d1[i].z & 0xFFFFu) | (((at >> 3) | (at + fp < L ? 0x2000u : 0u)) << 16);
                if (j) hdr = 34u, dd = at - 8u;
            }
            const uint32_t seg = (fl[i] == 0 || kind[i] == RXG_TXD_ARP) ? 0u : fl[i] - hdr;
            if (kind[i] == RXG_TXD_TCP && mss) {
                dd = j * mss;
                d1[i].z += dd;
                if ((uint64_t)dd + seg < d2[i].w) d2[i].y &= ~(0x09u << 8); // not the last: FIN, PSH
            }
            const uint32_t r = dd & 15u, hv = hdr - r;
            f[i].fb = pkts + ((uint64_t)off[e] << 6);
            f[i].pb = pay + ((uint64_t)d2[i].z << 4) + (dd & ~15u);
            f[i].plen = seg ? (int32_t)(r + seg) : 0;
            f[i].lo = (int32_t)r;
            f[i].hc = (int32_t)((hv + 15u) >> 4);
            f[i].k = ((16u - (hv & 15u)) - 2u) >> 2;
            f[i].nb = (int32_t)((fl[i] + 63u) & ~63u);
        }
#pragma unroll
        for (int i = 0; i < FPG; ++i)
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const int32_t a = ((s0 + q * STEP) >> 4) - f[i].hc + 1;
                own[i][q] = txe_src<NB != 0, true>(f[i], a);
                if constexpr (!NB) prv[i][q] = txe_src<false, true>(f[i], a - 1);
            }
#pragma unroll
        for (int i = 0; i < FPG; ++i)
            txe_frame_run<G, P, NB, true, true>(f[i], d0[i], d1[i], d2[i], kind[i], fl[i], own[i],
                                                prv[i], gl, lane, (flags & RXG_TXE_NO_CKSUM) != 0,
                                                &x[i]);
    }
}

// the UDP checksum of every cut datagram that was written: a group of FIN_G
// lanes per descriptor adds its s partial sums (s <= 1365: 86 trips of the
// group, not 1365 of a thread), the protocol and be16(L), and stores the two
// bytes at offset 40 of fragment 0.  Skipped and uncut descriptors write nothing.
constexpr uint32_t FIN_G = 16;
__global__ __launch_bounds__(256) void txe_frag_finish_kernel(
    const uint4 *__restrict__ txd, uint32_t n, uint32_t mtu, const uint32_t *__restrict__ first,
    const uint32_t *__restrict__ nseg, const uint32_t *__restrict__ off,
    const uint32_t *__restrict__ psum, uint8_t *__restrict__ pkts) {
    const uint32_t gl = threadIdx.x & (FIN_G - 1);
    for (uint64_t q = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / FIN_G; q < n;
         q += (uint64_t)gridDim.x * (256 / FIN_G)) { // group-uniform
        const uint4 d2 = txd[3 * q + 2];
        const uint32_t s = nseg[q];
        if (d2.y >> 24 != RXG_TXD_UDP || 28ull + d2.w <= mtu || s == 0) continue;
        const uint32_t e0 = first[q];
        uint32_t acc = 0; // (s sums below 2^16 each)
        for (uint32_t j = gl; j < s; j += FIN_G) acc += psum[e0 + j];
        for (uint32_t o = FIN_G / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (gl == 0) {
            acc += (17u << 8) + rx_bswap16(8u + d2.w); // pseudo-header {0, 17}, be16(L)
            uint32_t k = ~fold16(acc) & 0xFFFFu;
            if (k == 0u) k = 0xFFFFu;
            *reinterpret_cast<uint16_t *>(pkts + ((uint64_t)off[e0] << 6) + 40) = (uint16_t)k;
        }
    }
}

template <int G, int P, int FPG, int NB>
hipError_t launch_txe_frag(const uint4 *txd, const uint8_t *pay, uint8_t *pkts, const uint32_t *off,
                           const uint16_t *len, const uint32_t *map, const uint32_t *first,
                           const unsigned long long *need, uint32_t out_cap, uint32_t mss,
                           uint32_t mtu, uint32_t *psum, uint32_t flags, uint32_t bpc_cap,
                           hipStream_t s) {
    constexpr uint32_t TILE = (256 / G) * FPG;
    int cu = 0, occ = 0;
    hipError_t e = rx_occupancy(reinterpret_cast<const void *>(tx_encode_frag_kernel<G, P, FPG, NB>),
                                256, 0, &cu, &occ);
    if (e != hipSuccess) return e;
    // as launch_txe_tso: the grid is sized for out_cap
    const uint64_t tiles = ((uint64_t)out_cap + TILE - 1) / TILE;
    uint64_t bpc = (uint64_t)occ;
    if (bpc_cap && bpc > bpc_cap) bpc = bpc_cap;
    uint64_t blocks = (uint64_t)cu * bpc;
    if (blocks > tiles || bpc_cap == TXE_FULL_GRID) blocks = tiles;
    if (blocks > 0x7FFFFFFFull) blocks = 0x7FFFFFFFull; // (the tile loop strides)
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL((tx_encode_frag_kernel<G, P, FPG, NB>), dim3((uint32_t)blocks), dim3(256), 0, s,
                       txd, pay, pkts, off, len, map, first, need, (unsigned long long)out_cap, mss,
                       mtu, psum, flags);
    return hipGetLastError();
}

typedef hipError_t (*txe_frag_launch_fn)(const uint4 *, const uint8_t *, uint8_t *, const uint32_t *,
                                         const uint16_t *, const uint32_t *, const uint32_t *,
                                         const unsigned long long *, uint32_t, uint32_t, uint32_t,
                                         uint32_t *, uint32_t, uint32_t, hipStream_t);
// the shapes of k_txe, index for index (rxg_tune_txe and len_hint choose all three)
static const txe_frag_launch_fn k_txe_frag[] = {
    launch_txe_frag<4, 1, 4, 1>,  launch_txe_frag<4, 2, 2, 1>,  launch_txe_frag<8, 12, 1, 1>,
    launch_txe_frag<16, 8, 1, 1>, launch_txe_frag<4, 1, 4, 0>,  launch_txe_frag<4, 2, 2, 0>,
    launch_txe_frag<8, 12, 1, 0>, launch_txe_frag<16, 8, 1, 0>, launch_txe_frag<4, 1, 1, 1>,
    launch_txe_frag<8, 1, 1, 1>,  launch_txe_frag<8, 4, 2, 1>,  launch_txe_frag<16, 6, 1, 1>,
    launch_txe_frag<32, 4, 1, 1>, launch_txe_frag<32, 4, 1, 0>, launch_txe_frag<8, 1, 1, 0>,
};
static_assert(sizeof(k_txe_frag) / sizeof(k_txe_frag[0]) == sizeof(k_txe) / sizeof(k_txe[0]),
              "one fragmenting kernel per k_txe entry");

// the variant a len_hint chooses: the fastest of each class (k_txe's comment);
// K2's class boundaries
inline uint32_t txe_default_variant(uint32_t len_hint) {
    if (len_hint == 0) len_hint = 1518;
    return len_hint <= 64 ? 8 : (len_hint <= 128 ? 1 : (len_hint <= 600 ? 9 : (len_hint <= 1536 ? 11 : 12)));
}

} // namespace

uint32_t txe_num_variants();

size_t txe_tso_ws_bytes(uint32_t n, uint32_t out_cap) {
    const uint64_t nchunks = ((uint64_t)n + TXE_CHUNK - 1) / TXE_CHUNK;
    return 2 * (nchunks + 1) * 8 + TXE_PARTS * sizeof(txe_tso_part) + (uint64_t)n * 4 +
           (uint64_t)out_cap * 4;
}

// the TSO layout pass, then the encoder over the entries; variant / bpc_cap as
// tx_encode_launch
hipError_t tx_encode_tso_launch(const void *txd_, uint32_t n, const uint8_t *pay, uint32_t mss,
                                uint8_t *pkts, uint64_t cap, uint32_t slot, uint32_t *off,
                                uint16_t *len, uint32_t out_cap, uint32_t *first, uint32_t *nseg,
                                uint32_t len_hint, uint32_t flags, uint32_t *totals, void *ws,
                                uint32_t variant, uint32_t bpc_cap, hipStream_t s) {
    const uint4 *txd = reinterpret_cast<const uint4 *>(txd_);
    const uint32_t nchunks = (uint32_t)(((uint64_t)n + TXE_CHUNK - 1) / TXE_CHUNK);
    unsigned long long *sums_e = reinterpret_cast<unsigned long long *>(ws);
    unsigned long long *sums_u = sums_e + nchunks + 1;
    txe_tso_part *part = reinterpret_cast<txe_tso_part *>(sums_u + nchunks + 1);
    uint32_t *posu = reinterpret_cast<uint32_t *>(part + TXE_PARTS);
    uint32_t *map = posu + n;
    const uint32_t nparts = nchunks < TXE_PARTS ? nchunks : TXE_PARTS;
    hipError_t e = hipSuccess;
    const uint64_t lim = 64ull << 32; // offsets are 32 bits of 64-B units
    if (cap > lim) cap = lim;
    hipLaunchKernelGGL(txe_tso_sums_kernel, dim3(nchunks), dim3(256), 0, s, txd, n, mss, slot, sums_e,
                       sums_u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(txe_tso_scan_kernel, dim3(2), dim3(1024), 0, s, sums_e, (uint64_t)nchunks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(txe_tso_layout_kernel, dim3(nparts), dim3(256), 0, s, txd, n, mss, slot, sums_e,
                       sums_u, (unsigned long long)cap, (unsigned long long)out_cap, first, nseg, posu,
                       nchunks, part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (out_cap) { // (sized for out_cap: the entry count is on the device)
        const uint64_t eb = ((uint64_t)out_cap + 255) / 256;
        hipLaunchKernelGGL(txe_tso_entries_kernel, dim3((uint32_t)(eb < 16384 ? eb : 16384)), dim3(256),
                           0, s, txd, n, mss, slot, first, nseg, posu, sums_e + nchunks,
                           (unsigned long long)out_cap, off, len, map);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(txe_tso_totals_kernel, dim3(1), dim3(256), 0, s, part, nparts, n,
                       sums_e + nchunks, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t v = txe_default_variant(len_hint);
    if (variant < txe_num_variants()) v = variant;
    return k_txe_tso[v](txd, pay, pkts, off, len, map, first, sums_e + nchunks, out_cap, mss, flags,
                        bpc_cap ? bpc_cap : k_txe[v].bpc, s);
}

// txe_tso_ws_bytes plus a partial-sum word per entry
size_t txe_frag_ws_bytes(uint32_t n, uint32_t out_cap) {
    return ((txe_tso_ws_bytes(n, out_cap) + 15u) & ~(size_t)15u) + (uint64_t)out_cap * 4;
}

// the layout pass with both cuts, the encoder over the entries, then the cut
// datagrams' checksums; variant / bpc_cap as tx_encode_launch
hipError_t tx_encode_frag_launch(const void *txd_, uint32_t n, const uint8_t *pay, uint32_t mss,
                                 uint32_t mtu, uint8_t *pkts, uint64_t cap, uint32_t slot,
                                 uint32_t *off, uint16_t *len, uint32_t out_cap, uint32_t *first,
                                 uint32_t *nseg, uint32_t len_hint, uint32_t flags, uint32_t *totals,
                                 void *ws, uint32_t variant, uint32_t bpc_cap, hipStream_t s) {
    const uint4 *txd = reinterpret_cast<const uint4 *>(txd_);
    const uint32_t nchunks = (uint32_t)(((uint64_t)n + TXE_CHUNK - 1) / TXE_CHUNK);
    unsigned long long *sums_e = reinterpret_cast<unsigned long long *>(ws);
    unsigned long long *sums_u = sums_e + nchunks + 1;
    txe_tso_part *part = reinterpret_cast<txe_tso_part *>(sums_u + nchunks + 1);
    uint32_t *posu = reinterpret_cast<uint32_t *>(part + TXE_PARTS);
    uint32_t *map = posu + n;
    uint32_t *psum = reinterpret_cast<uint32_t *>(
        reinterpret_cast<uint8_t *>(ws) + ((txe_tso_ws_bytes(n, out_cap) + 15u) & ~(size_t)15u));
    const uint32_t nparts = nchunks < TXE_PARTS ? nchunks : TXE_PARTS;
    hipError_t e = hipSuccess;
    const uint64_t lim = 64ull << 32; // offsets are 32 bits of 64-B units
    if (cap > lim) cap = lim;
    hipLaunchKernelGGL(txe_frag_sums_kernel, dim3(nchunks), dim3(256), 0, s, txd, n, mss, mtu, slot,
                       sums_e, sums_u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(txe_tso_scan_kernel, dim3(2), dim3(1024), 0, s, sums_e, (uint64_t)nchunks);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(txe_frag_layout_kernel, dim3(nparts), dim3(256), 0, s, txd, n, mss, mtu, slot,
                       sums_e, sums_u, (unsigned long long)cap, (unsigned long long)out_cap, first,
                       nseg, posu, nchunks, part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (out_cap) { // (sized for out_cap: the entry count is on the device)
        const uint64_t eb = ((uint64_t)out_cap + 255) / 256;
        hipLaunchKernelGGL(txe_frag_entries_kernel, dim3((uint32_t)(eb < 16384 ? eb : 16384)),
                           dim3(256), 0, s, txd, n, mss, mtu, slot, first, nseg, posu,
                           sums_e + nchunks, (unsigned long long)out_cap, off, len, map);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(txe_tso_totals_kernel, dim3(1), dim3(256), 0, s, part, nparts, n,
                       sums_e + nchunks, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t v = txe_default_variant(len_hint);
    if (variant < txe_num_variants()) v = variant;
    e = k_txe_frag[v](txd, pay, pkts, off, len, map, first, sums_e + nchunks, out_cap, mss, mtu, psum,
                      flags, bpc_cap ? bpc_cap : k_txe[v].bpc, s);
    if (e != hipSuccess || mtu == 0 || out_cap == 0 || (flags & RXG_TXE_NO_CKSUM)) return e;
    const uint64_t fb = ((uint64_t)n * FIN_G + 255) / 256;
    hipLaunchKernelGGL(txe_frag_finish_kernel, dim3((uint32_t)(fb < 16384 ? fb : 16384)), dim3(256), 0,
                       s, txd, n, mtu, first, nseg, off, psum, pkts);
    return hipGetLastError();
}

uint32_t txe_num_variants() { return (uint32_t)(sizeof(k_txe) / sizeof(k_txe[0])); }

size_t txe_ws_bytes(uint32_t n) {
    const uint64_t nchunks = ((uint64_t)n + TXE_CHUNK - 1) / TXE_CHUNK;
    return nchunks * 8 + TXE_PARTS * sizeof(txe_part);
}

// the layout pass, then the encoder; `variant` (< txe_num_variants()) forces a
// table entry, else len_hint chooses; bpc_cap 0 = the variant's own
hipError_t tx_encode_launch(const void *txd_, uint32_t n, const uint8_t *pay, uint8_t *pkts,
                            uint64_t cap, uint32_t slot, uint32_t *off, uint16_t *len,
                            uint32_t len_hint, uint32_t flags, uint32_t *totals, void *ws,
                            uint32_t variant, uint32_t bpc_cap, hipStream_t s) {
    const uint4 *txd = reinterpret_cast<const uint4 *>(txd_);
    const uint32_t nchunks = (uint32_t)(((uint64_t)n + TXE_CHUNK - 1) / TXE_CHUNK);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(ws);
    txe_part *part = reinterpret_cast<txe_part *>(sums + nchunks);
    const uint32_t nparts = nchunks < TXE_PARTS ? nchunks : TXE_PARTS;
    hipError_t e = hipSuccess;
    const uint64_t lim = 64ull << 32; // offsets are 32 bits of 64-B units
    if (cap > lim) cap = lim;
    if (slot == 0) {
        hipLaunchKernelGGL(txe_units_kernel, dim3(nchunks), dim3(256), 0, s, txd, n, sums);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(txe_scan_kernel, dim3(1), dim3(1024), 0, s, sums, (uint64_t)nchunks);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(txe_offsets_kernel, dim3(nparts), dim3(256), 0, s, txd, n, sums,
                           (unsigned long long)(cap >> 6), off, len, nchunks, part);
    } else {
        hipLaunchKernelGGL(txe_slots_kernel, dim3(nparts), dim3(256), 0, s, txd, n, slot,
                           (unsigned long long)cap, off, len, nchunks, part);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(txe_totals_kernel, dim3(1), dim3(256), 0, s, part, nparts, n, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (len_hint == 0) len_hint = 1518;
    // the fastest variant of each class (the table's comment); K2's class boundaries
    uint32_t v = len_hint <= 64 ? 8 : (len_hint <= 128 ? 1 : (len_hint <= 600 ? 9 : (len_hint <= 1536 ? 11 : 12)));
    if (variant < txe_num_variants()) v = variant;
    return k_txe[v].fn(txd, pay, pkts, off, len, n, flags, bpc_cap ? bpc_cap : k_txe[v].bpc, s);
}
