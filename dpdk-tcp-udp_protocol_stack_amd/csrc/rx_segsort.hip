// rx_segsort.hip — K4: per-connection segment sort and payload gather of a
// classified burst, the device half of TCP delivery.
//
// The reference hands every segment that found a tcb (tcp_process rc 0) to
// the state machine one frame at a time (tcp.c:373-415); an ESTABLISHED
// segment with PSH gets a malloc'd tcp_fragment holding a copy of its
// payload, queued on the tcb's receive ring (ng_tcp_enqueue_recvbuffer,
// tcp.c:133-185), and an ACK (tcp_handle_established, tcp.c:218-297).  A
// connection's segments must reach its state machine in burst order; segments
// of different connections are independent.  So one device pass here:
//   1. sorts the burst's rc-0 TCP segments by tcb id with a stable LSD radix
//      sort (8-bit digits, as many passes as the id space needs: 2 at 4096
//      tcbs, 3 at 1M), keys read straight from the verdicts in the first pass;
//   2. decodes, per sorted segment, the header fields the state machine reads
//      (flags, data offset, total length, seq / ack, ports) into a 32-B
//      record, and the payload length it will copy (PSH segments only);
//   3. gathers those payloads into one buffer in sorted order (16-B aligned
//      slots, a wave per segment), so each connection's payloads are one
//      contiguous slice: one allocation and one copy per connection per
//      burst on the host (host/nstack.c).
// Bytes past a frame's capture read as 0 (the delivery oracle's rule).
//
// Three more forms share the sort: receive coalescing, sequence ordering and
// stream assembly (their sections below).  The device pieces they share with
// K4 stand with K4's kernels; the host side, at the end of the file, is one
// workspace description and five stages (sort, order, record, coalesce,
// assemble) that the four rx_*_launch entry points compose.
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

#include "rx_common.h"

#define SS_THREADS 256u
#define SS_ITEMS 8u
#define SS_TILE (SS_THREADS * SS_ITEMS) // keys per radix tile
#define SS_DIGITS 256u

namespace {

// inclusive scan over the 64 lanes of a wave (all lanes active): DPP row
// shifts inside each row of 16, then the row broadcasts across rows
__device__ __forceinline__ uint32_t ss_wave_scan(uint32_t x) {
    x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xA, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xC, 0xF, false);
    return x;
}

// ss_wave_scan with max for +: the lanes shifted in read 0, the identity of
// max on unsigned values as well
__device__ __forceinline__ uint32_t ss_wave_max(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0u, x, 0x111, 0xF, 0xF, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0u, x, 0x112, 0xF, 0xF, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0u, x, 0x114, 0xF, 0xF, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0u, x, 0x118, 0xF, 0xF, true));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0u, x, 0x142, 0xA, 0xF, false));
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0u, x, 0x143, 0xC, 0xF, false));
    return x;
}

// inclusive scan (sum or max) over the block's SS_THREADS values, every
// thread calling; ws: SS_THREADS / 64 words of LDS of this scan's own;
// total = the block's sum / max
template <bool MAX>
__device__ __forceinline__ uint32_t ss_block_scan(uint32_t x, uint32_t *ws, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t inc = MAX ? ss_wave_max(x) : ss_wave_scan(x);
    if (lane == 63u) ws[w] = inc;
    __syncthreads();
    uint32_t pre = 0u, all = 0u;
#pragma unroll
    for (uint32_t q = 0; q < SS_THREADS / 64u; ++q) {
        const uint32_t v = ws[q];
        if (q < w) pre = MAX ? max(pre, v) : pre + v;
        all = MAX ? max(all, v) : all + v;
    }
    total = all;
    return MAX ? max(inc, pre) : inc + pre;
}

// what the frame of sorted segment j says, the one decode of every form: the
// record's header fields (ncopy and offset left 0: each form's own), the
// source address, the captured bytes past the TCP header, and "neither SYN nor
// RST".  A byte at or past the capture reads as 0.
struct ss_frame {
    rxg_segment s;
    uint32_t sip, avail, movable;
};
__device__ __forceinline__ ss_frame ss_decode(const uint8_t *__restrict__ pkts,
                                              const uint32_t *__restrict__ off,
                                              const uint16_t *__restrict__ len, uint32_t unit_log2,
                                              const uint32_t *__restrict__ keys,
                                              const uint32_t *__restrict__ vals, uint32_t j) {
    ss_frame d;
    const uint32_t i = vals[j];
    const uint8_t *f = pkts + ((uint64_t)off[i] << unit_log2);
    const uint32_t cap = len[i];
    auto b = [&](uint32_t k) -> uint32_t { return k < cap ? (uint32_t)f[k] : 0u; };
    const uint32_t tl = (b(16) << 8) | b(17); // ip total_length (tcp.c:391)
    d.s.frame = i;
    d.s.flow = keys[j];
    d.s.seq = (b(38) << 24) | (b(39) << 16) | (b(40) << 8) | b(41);
    d.s.ack = (b(42) << 24) | (b(43) << 16) | (b(44) << 8) | b(45);
    d.s.hl = (uint8_t)(b(46) >> 4);
    d.s.flags = (uint8_t)b(47);
    d.s.plen = (int32_t)tl - 20 - 4 * (int32_t)d.s.hl; // tcp.c:145-146 with iTcplen = tl - 20
    d.s.offset = 0u;
    d.s.sport = (uint16_t)(b(34) | (b(35) << 8));
    d.s.dport = (uint16_t)(b(36) | (b(37) << 8));
    d.s.ncopy = 0u;
    d.sip = b(26) | (b(27) << 8) | (b(28) << 16) | (b(29) << 24);
    const uint32_t from = 34u + 4u * d.s.hl;
    d.avail = cap > from ? cap - from : 0u;
    d.movable = (d.s.flags & 0x06u) == 0u;
    return d;
}

// the payload K4 and its coalescing form keep: PSH and plen > 0
// (tcp.c:153-166), the captured part
__device__ __forceinline__ uint32_t ss_keep(const ss_frame &d) {
    return ((d.s.flags & 0x08u) && d.s.plen > 0) ? min((uint32_t)d.s.plen, d.avail) : 0u;
}

// the group-head step of a block of the ordering and assembly forms, every
// thread calling with its decoded position (d zeroed past the delivered
// segments): j heads a group unless it and its predecessor are movable records
// of one connection (flow, source address, ports); the predecessors meet in
// LDS, the block's own decoded again by thread 0.  Returns 1 + the last head
// at or before j inside the block (0: none yet); bH[block] = the block's last
// head, bZ[block] = 0 (the sum half of gro_scan_kernel runs beside the max
// half, on zeros).
__device__ __forceinline__ uint32_t ss_group_head(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, uint32_t nseg, const ss_frame &d, uint64_t *__restrict__ bH,
    uint64_t *__restrict__ bZ) {
    __shared__ uint32_t pf[SS_THREADS + 1u], ps[SS_THREADS + 1u], pp[SS_THREADS + 1u],
        pm[SS_THREADS + 1u];
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    const uint32_t ports = (uint32_t)d.s.sport | ((uint32_t)d.s.dport << 16);
    pf[t + 1u] = d.s.flow, ps[t + 1u] = d.sip, pp[t + 1u] = ports, pm[t + 1u] = d.movable;
    if (t == 0u) {
        ss_frame p = {};
        if (j0) p = ss_decode(pkts, off, len, unit_log2, keys, vals, j0 - 1u);
        pf[0] = p.s.flow, ps[0] = p.sip, pm[0] = p.movable;
        pp[0] = (uint32_t)p.s.sport | ((uint32_t)p.s.dport << 16);
    }
    __syncthreads();
    const bool head = !j || !d.movable || !pm[t] || pf[t] != d.s.flow || ps[t] != d.sip ||
                      pp[t] != ports;
    uint32_t hmax;
    const uint32_t hinc = ss_block_scan<true>((j < nseg && head) ? j + 1u : 0u, ws, hmax);
    if (t == 0u) {
        bH[blockIdx.x] = hmax;
        bZ[blockIdx.x] = 0u;
    }
    return hinc;
}

// 16 bytes of frame f from byte a, at any phase: five dword loads below the
// capture (a dword past it reads as 0), realigned with v_alignbyte
__device__ __forceinline__ void ss_fetch16(const uint8_t *__restrict__ f, uint32_t fcap, uint32_t a,
                                           uint32_t (&o4)[4]) {
    const uint32_t a0 = a & ~3u, sh = a & 3u;
    uint32_t wv[5];
#pragma unroll
    for (uint32_t q = 0; q < 5u; ++q) {
        const uint32_t p = a0 + 4u * q;
        wv[q] = p < fcap ? *reinterpret_cast<const uint32_t *>(f + p) : 0u;
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q)
        o4[q] = sh ? __builtin_amdgcn_alignbyte(wv[q + 1], wv[q], sh) : wv[q];
}

// a wave copies count bytes of frame f from byte src to payload + o, source
// and destination at any byte phase: the bytes up to the first 16-B boundary
// of the destination and those after the last one as byte stores, the chunks
// between as 16-B stores.  Every byte has one writer and no lane reads the
// destination.
__device__ __forceinline__ void ss_copy_bytes(const uint8_t *__restrict__ f, uint32_t fcap,
                                              uint32_t src, uint32_t count,
                                              uint8_t *__restrict__ payload, uint64_t o,
                                              uint32_t lane) {
    const uint32_t hlen = min(count, (16u - (uint32_t)(o & 15u)) & 15u);
    const uint32_t nb = (count - hlen) >> 4, tb = hlen + 16u * nb, tlen = count - tb;
    if (lane < hlen) payload[o + lane] = src + lane < fcap ? f[src + lane] : (uint8_t)0u;
    if (lane >= 16u && lane - 16u < tlen) {
        const uint32_t q = tb + (lane - 16u);
        payload[o + q] = src + q < fcap ? f[src + q] : (uint8_t)0u;
    }
    for (uint32_t c = lane; c < nb; c += 64u) {
        uint32_t o4[4];
        ss_fetch16(f, fcap, src + hlen + 16u * c, o4);
        *reinterpret_cast<uint4 *>(payload + o + hlen + 16u * c) =
            make_uint4(o4[0], o4[1], o4[2], o4[3]);
    }
}

// sort key of frame i in the first pass: its tcb id for a delivered TCP
// segment (class TCP, rc 0, id inside the id space), else the sentinel nt,
// which sorts after every id
__device__ __forceinline__ uint32_t ss_key0(const uint4 *__restrict__ v, uint64_t i, uint32_t nt) {
    const uint4 x = v[i];
    const uint32_t cls = (x.z >> 16) & 0xFFu;
    const int32_t rc = (int8_t)(x.z >> 24);
    return (cls == RXG_CLS_TCP && rc == RXG_RC_OK && x.x < nt) ? x.x : nt;
}

// digit histogram of one tile, digit-major (hist[d * ntiles + tile]), so one
// exclusive scan over the whole array gives every (digit, tile) its first
// output position; the first pass also counts the delivered segments
template <bool FIRST>
__global__ __launch_bounds__(SS_THREADS) void ss_hist_kernel(const uint4 *__restrict__ v,
                                                             const uint32_t *__restrict__ keys,
                                                             uint32_t n, uint32_t nt, uint32_t shift,
                                                             uint32_t ntiles, uint32_t *__restrict__ hist,
                                                             uint32_t *__restrict__ totals) {
    __shared__ uint32_t h[SS_DIGITS];
    const uint32_t t = threadIdx.x;
    h[t] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SS_TILE;
    uint32_t elig = 0u;
#pragma unroll
    for (uint32_t r = 0; r < SS_ITEMS; ++r) {
        const uint64_t i = base + r * SS_THREADS + t;
        if (i < n) {
            const uint32_t k = FIRST ? ss_key0(v, i, nt) : keys[i];
            elig += k < nt;
            atomicAdd(&h[(k >> shift) & 0xFFu], 1u);
        }
    }
    __syncthreads();
    hist[(uint64_t)t * ntiles + blockIdx.x] = h[t];
    if (FIRST) {
        for (int o = 32; o > 0; o >>= 1) elig += __shfl_xor(elig, o);
        if ((t & 63u) == 0u && elig) atomicAdd(&totals[0], elig);
    }
}

// exclusive scan of a[0..m) in place, one block (a thread per contiguous
// chunk); *total (nullable) = the sum
__global__ __launch_bounds__(1024) void ss_scan_kernel(uint32_t *__restrict__ a, uint32_t m,
                                                       uint32_t *__restrict__ total) {
    __shared__ uint32_t ws[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t per = (m + 1023u) / 1024u;
    const uint32_t b0 = min(m, t * per), b1 = min(m, b0 + per);
    uint32_t s = 0u;
    for (uint32_t k = b0; k < b1; ++k) s += a[k];
    const uint32_t inc = ss_wave_scan(s);
    if (lane == 63u) ws[w] = inc;
    __syncthreads();
    uint32_t run = inc - s;
    for (uint32_t q = 0; q < w; ++q) run += ws[q];
    if (t == 1023u && total) *total = run + s;
    for (uint32_t k = b0; k < b1; ++k) {
        const uint32_t x = a[k];
        a[k] = run;
        run += x;
    }
}

// stable scatter of one tile by digit: the tile's keys are taken in index
// order, 256 at a time; a wave ranks its lanes among those with the same
// digit (8 ballots: the lanes agreeing on every digit bit), the waves' digit
// counts meet in LDS in wave order, and every key lands after the tile's
// earlier keys of its digit and after every earlier tile's (the scanned
// histogram)
template <bool FIRST>
__global__ __launch_bounds__(SS_THREADS) void ss_scatter_kernel(
    const uint4 *__restrict__ v, const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin,
    uint32_t n, uint32_t nt, uint32_t shift, uint32_t ntiles, const uint32_t *__restrict__ hist,
    uint32_t *__restrict__ kout, uint32_t *__restrict__ vout) {
    __shared__ uint32_t base[SS_DIGITS];
    __shared__ uint32_t cnt[SS_THREADS / 64u][SS_DIGITS];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    base[t] = hist[(uint64_t)t * ntiles + blockIdx.x];
    const uint64_t tile0 = (uint64_t)blockIdx.x * SS_TILE;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t r = 0; r < SS_ITEMS; ++r) {
        const uint64_t i = tile0 + r * SS_THREADS + t;
        const bool ok = i < n;
        uint32_t key = 0u, val = 0u;
        if (ok) {
            key = FIRST ? ss_key0(v, i, nt) : kin[i];
            val = FIRST ? (uint32_t)i : vin[i];
        }
        const uint32_t d = (key >> shift) & 0xFFu;
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
#pragma unroll
        for (uint32_t q = 0; q < SS_THREADS / 64u; ++q) cnt[q][t] = 0u;
        __syncthreads();
        if (ok && rank == 0u) cnt[w][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (ok) {
            uint32_t pos = base[d] + rank;
            for (uint32_t q = 0; q < w; ++q) pos += cnt[q][d];
            kout[pos] = key;
            vout[pos] = val;
        }
        __syncthreads();
        uint32_t add = 0u;
#pragma unroll
        for (uint32_t q = 0; q < SS_THREADS / 64u; ++q) add += cnt[q][t];
        base[t] += add;
    }
}

// one record per sorted segment (j < the delivered count): the header fields
// the state machine reads, and the payload it keeps (PSH and plen > 0:
// tcp.c:153-166; the captured part); the block's exclusive scan of the
// 16-B-padded payload sizes gives each its offset inside the block's slice,
// tsum[block] the slice's size (0 for blocks past the count)
template <bool INPLACE>
__global__ __launch_bounds__(SS_THREADS) void ss_record_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ totals,
    rxg_segment *__restrict__ seg, uint32_t *__restrict__ tsum) {
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t j = blockIdx.x * SS_THREADS + t;
    if (blockIdx.x * SS_THREADS >= nseg) { // (uniform)
        if (t == 0u && !INPLACE) tsum[blockIdx.x] = 0u;
        return;
    }
    rxg_segment s;
    uint32_t padded = 0u;
    if (j < nseg) {
        const ss_frame d = ss_decode(pkts, off, len, unit_log2, keys, vals, j);
        const uint32_t keep = ss_keep(d);
        s = d.s;
        s.ncopy = (uint16_t)keep;
        padded = (keep + 15u) & ~15u;
    }
    if constexpr (INPLACE) { // the payload stays in the frame: bytes [34 + 4*hl, + ncopy)
        if (j < nseg) {
            s.offset = 34u + 4u * s.hl;
            seg[j] = s;
        }
        return;
    }
    const uint32_t inc = ss_wave_scan(padded);
    if (lane == 63u) ws[w] = inc;
    __syncthreads();
    uint32_t o = inc - padded;
    for (uint32_t q = 0; q < w; ++q) o += ws[q];
    if (t == SS_THREADS - 1u) tsum[blockIdx.x] = o + padded;
    if (j < nseg) {
        s.offset = o; // + the block's base (ss_copy_kernel)
        seg[j] = s;
    }
}

// a wave per segment: its final offset (block base added), then its payload,
// bytes [34 + 4*hl, + ncopy) of the frame, as 16-B chunks (dword loads below
// the capture, realigned with v_alignbyte), zero to the 16-B padded end
__global__ __launch_bounds__(SS_THREADS) void ss_copy_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ tbase,
    rxg_segment *__restrict__ seg, uint8_t *__restrict__ payload, uint64_t cap,
    uint32_t *__restrict__ totals) {
    const uint32_t nseg = totals[0];
    const uint32_t j = blockIdx.x * (SS_THREADS / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (j >= nseg) return;
    const rxg_segment s = seg[j];
    const uint64_t o = (uint64_t)s.offset + tbase[j / SS_THREADS];
    if (lane == 0u) seg[j].offset = (uint32_t)o;
    if (!s.ncopy) return;
    const uint32_t ncopy = s.ncopy;
    if (o + ((ncopy + 15u) & ~15u) > cap) {
        if (lane == 0u) atomicOr(&totals[2], 1u); // payload buffer too small
        return;
    }
    const uint8_t *f = pkts + ((uint64_t)off[s.frame] << unit_log2);
    const uint32_t fcap = len[s.frame];
    const uint32_t src = 34u + 4u * s.hl;
    for (uint32_t c = lane; 16u * c < ncopy; c += 64u) {
        uint32_t o4[4];
        ss_fetch16(f, fcap, src + 16u * c, o4);
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) { // the chunk's bytes at or past ncopy: 0
            const uint32_t b0 = 16u * c + 4u * q;
            const uint32_t keep = ncopy > b0 ? ncopy - b0 : 0u;
            if (keep < 4u) o4[q] &= keep ? ((1u << (8u * keep)) - 1u) : 0u;
        }
        *reinterpret_cast<uint4 *>(payload + o + 16u * c) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
    }
}

} // namespace

// ---- Receive coalescing (GRO): K4 with the in-sequence trains of a
// connection laid down as contiguous byte ranges (the rule: include/rxgpu.h,
// "TCP receive coalescing"; restated on the host in rx_gro_host.cpp).  After
// the same sort, three rounds of block scan + one-block scan of the block sums:
//   1. records, link flags, G[j] = the sum of ncopy before j and the last
//      chain head at or before j (a max scan); inside a chain ncopy == plen,
//      so b[j] = G[j] - G[head];
//   2. run heads from b and the window, counted into run ids;
//   3. per run: first record, count, bytes; the 16-B padded sizes scanned
//      into the runs' offsets;
// then a wave per segment copies its payload to run offset + G[j] - G[first].
// No chain is walked: one connection may own the whole burst.
namespace {

#define GRO_HEADBIT 0x80000000u

// exclusive scan in place of a block array of 64-bit values, one block (a
// thread per contiguous chunk): m = the blocks of *cnt items; block 0 sums
// a_sum (*total, nullable, = the sum), block 1 (when launched) takes the
// running max of a_max
__global__ __launch_bounds__(1024) void gro_scan_kernel(uint64_t *__restrict__ a_sum,
                                                        uint64_t *__restrict__ a_max,
                                                        const uint32_t *__restrict__ cnt,
                                                        uint64_t *__restrict__ total) {
    __shared__ uint64_t ws[16];
    const bool mx = blockIdx.x == 1u;
    uint64_t *a = mx ? a_max : a_sum;
    const uint32_t m = (uint32_t)(((uint64_t)cnt[0] + SS_THREADS - 1u) / SS_THREADS);
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t per = (m + 1023u) / 1024u;
    const uint32_t b0 = min(m, t * per), b1 = min(m, b0 + per);
    auto op = [mx](uint64_t x, uint64_t y) -> uint64_t { return mx ? (x > y ? x : y) : x + y; };
    uint64_t s = 0u;
    for (uint32_t k = b0; k < b1; ++k) s = op(s, a[k]);
    uint64_t inc = s;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t y = __shfl_up((unsigned long long)inc, d);
        if (lane >= d) inc = op(inc, y);
    }
    // exclusive over the lanes: the inclusive value of the lane below
    uint64_t run = __shfl_up((unsigned long long)inc, 1u);
    if (lane == 0u) run = 0u;
    if (lane == 63u) ws[w] = inc;
    __syncthreads();
    for (uint32_t q = 0; q < w; ++q) run = op(run, ws[q]);
    if (t == 1023u && total && !mx) *total = op(run, s);
    for (uint32_t k = b0; k < b1; ++k) {
        const uint64_t x = a[k];
        a[k] = run;
        run = op(run, x);
    }
}

// what a record's successor must match to link to it
struct gro_key {
    uint32_t flow, sip, ports, ack, seq, next_seq, merge;
};

// the record of sorted segment j, K4's (offset left 0), and its link key
__device__ __forceinline__ rxg_segment gro_decode(const uint8_t *__restrict__ pkts,
                                                  const uint32_t *__restrict__ off,
                                                  const uint16_t *__restrict__ len,
                                                  uint32_t unit_log2, const uint32_t *__restrict__ keys,
                                                  const uint32_t *__restrict__ vals, uint32_t j,
                                                  gro_key &k) {
    const ss_frame d = ss_decode(pkts, off, len, unit_log2, keys, vals, j);
    const uint32_t keep = ss_keep(d);
    rxg_segment s = d.s;
    s.ncopy = (uint16_t)keep;
    k.flow = s.flow;
    k.sip = d.sip;
    k.ports = (uint32_t)s.sport | ((uint32_t)s.dport << 16);
    k.ack = s.ack;
    k.seq = s.seq;
    k.next_seq = s.seq + (uint32_t)s.plen;
    k.merge = s.flags == 0x18u && s.hl == 5u && s.plen > 0 && (int32_t)keep == s.plen;
    return s;
}

// round 1: the records; gl[j] = the block's sum of ncopy before j; hd[j] =
// 1 + the last chain head at or before j inside the block (0: none yet);
// bG / bH[block] = the block's sum / last head
__global__ __launch_bounds__(SS_THREADS) void gro_record_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ totals,
    rxg_segment *__restrict__ seg, uint32_t *__restrict__ gl, uint32_t *__restrict__ hd,
    uint64_t *__restrict__ bG, uint64_t *__restrict__ bH) {
    __shared__ gro_key key[SS_THREADS + 1u];
    __shared__ uint32_t ws_g[SS_THREADS / 64u], ws_h[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    if (j0 >= nseg) return; // (uniform)
    gro_key k = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t c = 0u;
    if (j < nseg) {
        const rxg_segment s = gro_decode(pkts, off, len, unit_log2, keys, vals, j, k);
        seg[j] = s;
        c = s.ncopy;
    }
    key[t + 1u] = k;
    if (t == 0u) { // the block's predecessor record
        gro_key p = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (j0) (void)gro_decode(pkts, off, len, unit_log2, keys, vals, j0 - 1u, p);
        key[0] = p;
    }
    __syncthreads();
    const gro_key p = key[t];
    const bool link = j && p.merge && k.merge && p.flow == k.flow && p.sip == k.sip &&
                      p.ports == k.ports && p.ack == k.ack && k.seq == p.next_seq;
    uint32_t gsum, hmax;
    const uint32_t ginc = ss_block_scan<false>(c, ws_g, gsum);
    const uint32_t hinc = ss_block_scan<true>((j < nseg && !link) ? j + 1u : 0u, ws_h, hmax);
    if (j < nseg) {
        gl[j] = ginc - c;
        hd[j] = hinc;
    }
    if (t == 0u) {
        bG[blockIdx.x] = gsum;
        bH[blockIdx.x] = hmax;
    }
}

// round 2 (bG, bH scanned): record j starts a run iff it heads its chain or
// the window index of b changes from j-1 to j; rl[j] = the block's count of
// run heads up to and including j, GRO_HEADBIT set on a head; bR[block] = the
// block's count
__global__ __launch_bounds__(SS_THREADS) void gro_runhead_kernel(
    const rxg_segment *__restrict__ seg, const uint32_t *__restrict__ totals, uint32_t W,
    const uint32_t *__restrict__ gl, const uint32_t *__restrict__ hd,
    const uint64_t *__restrict__ bG, const uint64_t *__restrict__ bH, uint32_t *__restrict__ rl,
    uint64_t *__restrict__ bR) {
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    if (j0 >= nseg) return; // (uniform)
    uint32_t rh = 0u;
    if (j < nseg) {
        // the chain's head: inside the block, else the last one of the blocks
        // before (record 0 heads a chain, so there is one)
        const uint32_t h1 = hd[j] ? hd[j] : (uint32_t)bH[blockIdx.x];
        rh = 1u;
        if (h1 != j + 1u) { // j links to j-1
            const uint32_t h = h1 - 1u;
            const uint64_t b = (gl[j] + bG[blockIdx.x]) - (gl[h] + bG[h / SS_THREADS]);
            const uint64_t pb = b - (uint32_t)seg[j - 1u].plen;
            rh = b / W != pb / W;
        }
    }
    uint32_t total;
    const uint32_t inc = ss_block_scan<false>(rh, ws, total);
    if (j < nseg) rl[j] = inc | (rh ? GRO_HEADBIT : 0u);
    if (t == 0u) bR[blockIdx.x] = total;
}

// (bR scanned, tot[1] = the runs) rl[j] becomes j's run id; a run's head
// leaves its index in rfirst[run]
__global__ __launch_bounds__(SS_THREADS) void gro_runid_kernel(uint32_t *__restrict__ totals,
                                                              const uint64_t *__restrict__ tot,
                                                              uint32_t *__restrict__ rl,
                                                              const uint64_t *__restrict__ bR,
                                                              uint32_t *__restrict__ rfirst) {
    const uint32_t nseg = totals[0];
    const uint32_t j = blockIdx.x * SS_THREADS + threadIdx.x;
    if (j == 0u) totals[3] = (uint32_t)tot[1];
    if (j >= nseg) return;
    const uint32_t v = rl[j];
    const uint32_t id = (v & ~GRO_HEADBIT) + (uint32_t)bR[blockIdx.x] - 1u;
    rl[j] = id;
    if (v & GRO_HEADBIT) rfirst[id] = j;
}

// round 3: the run records (offset in gro_copy_kernel); ol[r] = the block's
// sum of the 16-B padded run sizes before r, bO[block] the block's sum
__global__ __launch_bounds__(SS_THREADS) void gro_run_kernel(
    const uint32_t *__restrict__ totals, const uint64_t *__restrict__ tot,
    const uint32_t *__restrict__ gl, const uint64_t *__restrict__ bG,
    const uint32_t *__restrict__ rfirst, rxg_tcp_run *__restrict__ run, uint32_t *__restrict__ ol,
    uint64_t *__restrict__ bO) {
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t nseg = totals[0], nrun = (uint32_t)tot[1];
    const uint32_t t = threadIdx.x;
    const uint32_t r0 = blockIdx.x * SS_THREADS, r = r0 + t;
    if (r0 >= nrun) return; // (uniform)
    uint32_t padded = 0u;
    if (r < nrun) {
        const uint32_t first = rfirst[r], next = r + 1u < nrun ? rfirst[r + 1u] : nseg;
        const uint64_t g0 = gl[first] + bG[first / SS_THREADS];
        const uint64_t g1 = next < nseg ? gl[next] + bG[next / SS_THREADS] : tot[0];
        rxg_tcp_run x;
        x.first = first;
        x.nseg = next - first;
        x.bytes = (uint32_t)(g1 - g0);
        x.offset = 0u;
        run[r] = x;
        padded = (x.bytes + 15u) & ~15u;
    }
    uint32_t total;
    const uint32_t inc = ss_block_scan<false>(padded, ws, total);
    if (r < nrun) ol[r] = inc - padded;
    if (t == 0u) bO[blockIdx.x] = total;
}

// a wave per segment (bO scanned, tot[2] = the payload bytes used): its
// offset = its run's offset + the run's ncopy before it, at any byte phase;
// then its payload, bytes [34 + 4*hl, + ncopy) of the frame (ss_copy_bytes);
// the run's last segment zeroes the bytes to the 16-B padded end.  Every byte
// has one writer and no lane reads the destination.
__global__ __launch_bounds__(SS_THREADS) void gro_copy_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint64_t *__restrict__ tot,
    const uint32_t *__restrict__ gl, const uint64_t *__restrict__ bG,
    const uint32_t *__restrict__ rl, const uint32_t *__restrict__ rfirst,
    const uint32_t *__restrict__ ol, const uint64_t *__restrict__ bO, rxg_segment *__restrict__ seg,
    rxg_tcp_run *__restrict__ run, uint8_t *__restrict__ payload, uint64_t cap,
    uint32_t *__restrict__ totals) {
    const uint32_t nseg = totals[0];
    const uint32_t j = blockIdx.x * (SS_THREADS / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) totals[1] = (uint32_t)tot[2];
    if (j >= nseg) return;
    const rxg_segment s = seg[j];
    const uint32_t r = rl[j], first = rfirst[r];
    const uint64_t ro = ol[r] + bO[r / SS_THREADS];
    const uint32_t rbytes = run[r].bytes;
    const uint64_t o =
        ro + ((gl[j] + bG[j / SS_THREADS]) - (gl[first] + bG[first / SS_THREADS]));
    if (lane == 0u) {
        seg[j].offset = (uint32_t)o;
        if (j == first) run[r].offset = (uint32_t)ro;
    }
    if (ro + ((rbytes + 15u) & ~15u) > cap) { // the whole run stays unwritten
        if (lane == 0u && j == first) atomicOr(&totals[2], 1u);
        return;
    }
    const uint32_t ncopy = s.ncopy;
    const bool last = j + 1u == nseg || rl[j + 1u] != r;
    if (last && lane >= 32u && lane < 48u) { // the zero tail: [run end, padded end)
        const uint64_t end = o + ncopy;
        if (lane - 32u < ((16u - (uint32_t)(end & 15u)) & 15u)) payload[end + (lane - 32u)] = 0u;
    }
    if (!ncopy) return;
    ss_copy_bytes(pkts + ((uint64_t)off[s.frame] << unit_log2), len[s.frame], 34u + 4u * s.hl, ncopy,
                  payload, o, lane);
}

} // namespace

// ---- Sequence ordering (opt-in): a permutation stage between the sort and
// the record stage (the rule: include/rxgpu.h, "TCP sequence ordering";
// restated on the host in rx_order_host.cpp).  On the sorted (flow, frame)
// arrays:
//   1. group heads from a comparison with the predecessor, the last head at or
//      before j by a max scan (block scan + one-block scan of the block maxima);
//   2. the biased key (seq - seq[head]) ^ 0x80000000 and the burst's "some
//      inversion" flag (a record below its predecessor inside a group);
//   3. K4's stable radix passes over (key, position), four digits, then over
//      the head index of each position (monotone in position, so every group
//      lands where it was, sorted inside);
//   4. the (flow, frame) arrays gathered through the permutation, the moved
//      records counted.
// The record / copy / coalescing kernels then run unchanged on the permuted
// arrays.  No group is walked: one connection may own the whole burst.
namespace {

// round 1: sq[j] = seq; hl[j], bH[block] and bZ[block] from ss_group_head
__global__ __launch_bounds__(SS_THREADS) void ord_head_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ totals,
    uint32_t *__restrict__ sq, uint32_t *__restrict__ hl, uint64_t *__restrict__ bH,
    uint64_t *__restrict__ bZ) {
    const uint32_t nseg = totals[0];
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + threadIdx.x;
    if (j0 >= nseg) return; // (uniform)
    ss_frame d = {};
    if (j < nseg) d = ss_decode(pkts, off, len, unit_log2, keys, vals, j);
    const uint32_t hinc = ss_group_head(pkts, off, len, unit_log2, keys, vals, nseg, d, bH, bZ);
    if (j < nseg) {
        sq[j] = d.s.seq;
        hl[j] = hinc;
    }
}

// round 2 (bH scanned), all n positions: the radix key, the head index and
// the position itself; the positions past the delivered segments are groups
// of one, so they stay where they are; *flag is set when a record's key is
// below its predecessor's inside a group (else the permutation is the identity)
__global__ __launch_bounds__(SS_THREADS) void ord_key_kernel(
    const uint32_t *__restrict__ totals, uint32_t n, const uint32_t *__restrict__ sq,
    const uint32_t *__restrict__ hl, const uint64_t *__restrict__ bH, uint32_t *__restrict__ ok,
    uint32_t *__restrict__ hk, uint32_t *__restrict__ pos, uint32_t *__restrict__ flag) {
    const uint32_t nseg = totals[0];
    const uint32_t j = blockIdx.x * SS_THREADS + threadIdx.x;
    bool inv = false;
    if (j < n) {
        uint32_t key = 0u, h = j;
        if (j < nseg) {
            // the group's head: inside the block, else the last one of the
            // blocks before (record 0 heads a group, so there is one)
            const uint32_t l = hl[j];
            h = (l ? l : (uint32_t)bH[blockIdx.x]) - 1u;
            const uint32_t s0 = sq[h];
            key = (sq[j] - s0) ^ 0x80000000u;
            inv = h != j && key < ((sq[j - 1u] - s0) ^ 0x80000000u);
        }
        ok[j] = key;
        hk[j] = h;
        pos[j] = j;
    }
    const uint64_t m = __ballot(inv);
    if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll((unsigned long long)m) - 1u) atomicOr(flag, 1u);
}

// between the key passes and the head passes: the radix key of position k
// becomes the head index of the record now there
__global__ __launch_bounds__(SS_THREADS) void ord_headkey_kernel(uint32_t n,
                                                                const uint32_t *__restrict__ flag,
                                                                const uint32_t *__restrict__ hk,
                                                                const uint32_t *__restrict__ pos,
                                                                uint32_t *__restrict__ key) {
    if (!flag[0]) return; // (uniform) no inversion: ord_apply_kernel takes the identity
    const uint32_t k = blockIdx.x * SS_THREADS + threadIdx.x;
    if (k < n) key[k] = hk[pos[k]];
}

// the sorted (flow, frame) arrays through the permutation (the identity when
// no inversion was seen), and totals[4] = the records that moved
__global__ __launch_bounds__(SS_THREADS) void ord_apply_kernel(
    uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ perm,
    const uint32_t *__restrict__ kin, const uint32_t *__restrict__ vin,
    uint32_t *__restrict__ kout, uint32_t *__restrict__ vout, uint32_t *__restrict__ totals) {
    const uint32_t nseg = totals[0];
    const uint32_t k = blockIdx.x * SS_THREADS + threadIdx.x;
    bool mv = false;
    if (k < n) {
        const uint32_t p = flag[0] ? perm[k] : k;
        kout[k] = kin[p];
        vout[k] = vin[p];
        mv = k < nseg && p != k;
    }
    const uint64_t m = __ballot(mv);
    if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll((unsigned long long)m) - 1u)
        atomicAdd(&totals[4], (uint32_t)__popcll(m));
}

} // namespace

// ---- Stream assembly (opt-in): after the sort and the ordering stage, each
// connection's segments of the burst laid down as contiguous byte ranges with
// duplicates dropped, overlaps trimmed and a new range at every hole (the
// rule: include/rxgpu.h, "TCP stream assembly"; restated on the host in
// rx_assemble_host.cpp).  On the ordered (flow, frame) arrays:
//   1. the records (payload kept for any plen > 0 captured whole), the group
//      heads and the last head at or before j (max scan);
//   2. a[j], end[j] and the segmented inclusive max scan of end over the
//      groups (block scan + a one-block segmented scan of the block sums);
//      cov[j] is its value at j-1;
//   3. take, skip, finok, the stream heads; the stream ids and the sum of take
//      before j (sum scans);
//   4. the stream records, their 16-B padded sizes scanned into offsets;
// then a wave per record copies its take bytes from 34 + 4*hl + skip to
// stream offset + (the stream's take before it).  No group is walked: one
// connection may own the whole burst.
namespace {

#define ASM_USABLE 0x10000u  // dl[j]: the payload was captured whole (or plen <= 0)
#define ASM_FIN 0x20000u     // dl[j]: FIN on a movable, usable record
#define ASM_F_START 0x1u     // fl[j]: j starts a stream
#define ASM_F_HOLE 0x2u      // fl[j]: ... because of a hole
#define ASM_F_FINOK 0x4u     // fl[j]: finok[j]

// the segmented max: (f, v) = "a group head at or before here" and the maximum
// since it; y comes after x
__device__ __forceinline__ void asm_op(bool xf, uint64_t xv, bool &yf, uint64_t &yv) {
    if (!yf) yv = xv > yv ? xv : yv;
    yf = yf || xf;
}

// inclusive segmented max scan over the wave's lanes (all lanes active)
__device__ __forceinline__ void asm_wave_scan(bool &f, uint64_t &v) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t pv = __shfl_up((unsigned long long)v, d);
        const bool pf = __shfl_up((int)f, d) != 0;
        if (lane >= d) asm_op(pf, pv, f, v);
    }
}

// round 1: the ordered form's record of position j (ncopy and offset in
// asm_copy_kernel), dl[j] = dlen and the ASM_USABLE / ASM_FIN bits; hl[j],
// bH[block] and bZ[block] from ss_group_head
__global__ __launch_bounds__(SS_THREADS) void asm_record_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ totals,
    rxg_segment *__restrict__ seg, uint32_t *__restrict__ dl, uint32_t *__restrict__ hl,
    uint64_t *__restrict__ bH, uint64_t *__restrict__ bZ) {
    const uint32_t nseg = totals[0];
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + threadIdx.x;
    if (j0 >= nseg) return; // (uniform)
    ss_frame k = {};
    if (j < nseg) {
        k = ss_decode(pkts, off, len, unit_log2, keys, vals, j);
        const rxg_segment &s = k.s;
        seg[j] = s;
        const bool usable = s.plen <= 0 || k.avail >= (uint32_t)s.plen;
        // (a SYN or RST record is left alone: no data, no FIN)
        uint32_t d = (k.movable && usable && s.plen > 0) ? (uint32_t)s.plen : 0u;
        if (usable) d |= ASM_USABLE;
        if (k.movable && usable && (s.flags & 0x01u)) d |= ASM_FIN;
        dl[j] = d;
    }
    const uint32_t hinc = ss_group_head(pkts, off, len, unit_log2, keys, vals, nseg, k, bH, bZ);
    if (j < nseg) hl[j] = hinc;
}

// round 2 (bH scanned): av[j] = a[j]; il[j] = the maximum of end over the
// group's records of this block up to and including j; bV[block] / bF[block] =
// that of the block's last position and "the block holds a head"
__global__ __launch_bounds__(SS_THREADS) void asm_end_kernel(
    const rxg_segment *__restrict__ seg, const uint32_t *__restrict__ totals,
    const uint32_t *__restrict__ dl, const uint32_t *__restrict__ hl,
    const uint64_t *__restrict__ bH, uint32_t *__restrict__ av, uint64_t *__restrict__ il,
    uint64_t *__restrict__ bV, uint64_t *__restrict__ bF) {
    __shared__ uint64_t wv[SS_THREADS / 64u];
    __shared__ uint32_t wf[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    if (j0 >= nseg) return; // (uniform)
    bool f = false;
    uint64_t v = 0u;
    uint32_t a = 0u;
    if (j < nseg) {
        // the group's head: inside the block, else the last one of the blocks
        // before (record 0 heads a group, so there is one)
        const uint32_t l = hl[j];
        const uint32_t h = (l ? l : (uint32_t)bH[blockIdx.x]) - 1u;
        a = seg[j].seq - seg[h].seq;
        v = (uint64_t)a + (dl[j] & 0xFFFFu);
        f = h == j;
    }
    asm_wave_scan(f, v);
    if (lane == 63u) wv[w] = v, wf[w] = f;
    __syncthreads();
    bool cf = false;
    uint64_t cv = 0u, bv = 0u;
    bool bf = false;
#pragma unroll
    for (uint32_t q = 0; q < SS_THREADS / 64u; ++q) {
        bool qf = wf[q] != 0u;
        uint64_t qv = wv[q];
        if (q < w) {
            bool xf = qf;
            uint64_t xv = qv;
            asm_op(cf, cv, xf, xv);
            cf = xf, cv = xv;
        }
        asm_op(bf, bv, qf, qv);
        bf = qf, bv = qv;
    }
    asm_op(cf, cv, f, v);
    if (j < nseg) {
        av[j] = a;
        il[j] = v;
    }
    if (t == 0u) {
        bV[blockIdx.x] = bv;
        bF[blockIdx.x] = bf;
    }
}

// exclusive segmented max scan in place of the block pairs (bV, bF), one block
// (a thread per contiguous chunk): bV[block] becomes the maximum of end since
// the last head in the blocks before it
__global__ __launch_bounds__(1024) void asm_scan_kernel(uint64_t *__restrict__ bV,
                                                        const uint64_t *__restrict__ bF,
                                                        const uint32_t *__restrict__ cnt) {
    __shared__ uint64_t wv[16];
    __shared__ uint32_t wf[16];
    const uint32_t m = (uint32_t)(((uint64_t)cnt[0] + SS_THREADS - 1u) / SS_THREADS);
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    const uint32_t per = (m + 1023u) / 1024u;
    const uint32_t b0 = min(m, t * per), b1 = min(m, b0 + per);
    bool f = false;
    uint64_t v = 0u;
    for (uint32_t k = b0; k < b1; ++k) {
        bool yf = bF[k] != 0u;
        uint64_t yv = bV[k];
        asm_op(f, v, yf, yv);
        f = yf, v = yv;
    }
    asm_wave_scan(f, v);
    // exclusive over the lanes: the inclusive pair of the lane below
    uint64_t rv = __shfl_up((unsigned long long)v, 1u);
    bool rf = __shfl_up((int)f, 1u) != 0;
    if (lane == 0u) rv = 0u, rf = false;
    if (lane == 63u) wv[w] = v, wf[w] = f;
    __syncthreads();
    bool cf = false;
    uint64_t cv = 0u;
    for (uint32_t q = 0; q < w; ++q) {
        bool xf = wf[q] != 0u;
        uint64_t xv = wv[q];
        asm_op(cf, cv, xf, xv);
        cf = xf, cv = xv;
    }
    asm_op(cf, cv, rf, rv);
    for (uint32_t k = b0; k < b1; ++k) {
        bool yf = bF[k] != 0u;
        uint64_t yv = bV[k];
        bV[k] = rv;
        asm_op(rf, rv, yf, yv);
        rf = yf, rv = yv;
    }
}

// what the rule says of record j (bV scanned)
struct asm_rec {
    uint64_t ns;
    uint32_t take, skip;
    bool head, hole, finok;
};
__device__ __forceinline__ asm_rec asm_eval(uint32_t j, const uint32_t *__restrict__ dl,
                                            const uint32_t *__restrict__ hl,
                                            const uint32_t *__restrict__ av,
                                            const uint64_t *__restrict__ il,
                                            const uint64_t *__restrict__ bV) {
    asm_rec r;
    const uint32_t d = dl[j], dlen = d & 0xFFFFu;
    const uint64_t a = av[j], end = a + dlen;
    r.head = hl[j] == j + 1u;
    uint64_t cov = 0u;
    if (!r.head) { // the scan's value at j-1: its block's, and the blocks' before it
        const uint32_t i = j - 1u;
        cov = il[i];
        if (!hl[i]) {
            const uint64_t c = bV[i / SS_THREADS];
            cov = c > cov ? c : cov;
        }
    }
    r.ns = a > cov ? a : cov;
    r.take = (uint32_t)(end - (end < r.ns ? end : r.ns));
    r.skip = dlen - r.take;
    r.hole = !r.head && a > cov;
    r.finok = (d & ASM_FIN) && end >= cov;
    return r;
}

// round 3: tk[j] = take, s32[j] = seq[h] + ns[j], fl[j] = the ASM_F_* bits;
// sl[j] = the block's count of stream heads up to and including j, tl[j] = the
// block's sum of take before j; bR / bT[block] = the block's count / sum;
// totals[5] += skip
__global__ __launch_bounds__(SS_THREADS) void asm_head_kernel(
    const rxg_segment *__restrict__ seg, uint32_t *__restrict__ totals,
    const uint32_t *__restrict__ dl, const uint32_t *__restrict__ hl,
    const uint32_t *__restrict__ av, const uint64_t *__restrict__ il,
    const uint64_t *__restrict__ bV, uint32_t *__restrict__ tk, uint32_t *__restrict__ s32,
    uint32_t *__restrict__ fl, uint32_t *__restrict__ sl, uint32_t *__restrict__ tl,
    uint64_t *__restrict__ bR, uint64_t *__restrict__ bT) {
    __shared__ uint32_t ws_r[SS_THREADS / 64u], ws_t[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    if (j0 >= nseg) return; // (uniform)
    uint32_t start = 0u, take = 0u, skip = 0u;
    if (j < nseg) {
        const asm_rec r = asm_eval(j, dl, hl, av, il, bV);
        bool st = r.head || r.hole;
        if (!st) st = asm_eval(j - 1u, dl, hl, av, il, bV).finok;
        start = st;
        take = r.take, skip = r.skip;
        tk[j] = take;
        // seq[h] = seq[j] - a[j]
        s32[j] = seg[j].seq - av[j] + (uint32_t)r.ns;
        fl[j] = (st ? ASM_F_START : 0u) | (r.hole ? ASM_F_HOLE : 0u) | (r.finok ? ASM_F_FINOK : 0u);
    }
    uint32_t rsum, tsum;
    const uint32_t rinc = ss_block_scan<false>(start, ws_r, rsum);
    const uint32_t tinc = ss_block_scan<false>(take, ws_t, tsum);
    if (j < nseg) {
        sl[j] = rinc;
        tl[j] = tinc - take;
    }
    if (t == 0u) {
        bR[blockIdx.x] = rsum;
        bT[blockIdx.x] = tsum;
    }
    for (int o = 32; o > 0; o >>= 1) skip += __shfl_xor(skip, o);
    if ((t & 63u) == 0u && skip) atomicAdd(&totals[5], skip);
}

// (bR scanned, tot[1] = the streams) sl[j] becomes j's stream id; a stream's
// head leaves its index in sfirst[stream]
__global__ __launch_bounds__(SS_THREADS) void asm_streamid_kernel(uint32_t *__restrict__ totals,
                                                                 const uint64_t *__restrict__ tot,
                                                                 const uint32_t *__restrict__ fl,
                                                                 uint32_t *__restrict__ sl,
                                                                 const uint64_t *__restrict__ bR,
                                                                 uint32_t *__restrict__ sfirst) {
    const uint32_t nseg = totals[0];
    const uint32_t j = blockIdx.x * SS_THREADS + threadIdx.x;
    if (j == 0u) totals[3] = (uint32_t)tot[1];
    if (j >= nseg) return;
    const uint32_t id = sl[j] + (uint32_t)bR[blockIdx.x] - 1u;
    sl[j] = id;
    if (fl[j] & ASM_F_START) sfirst[id] = j;
}

// round 4: the stream records (offset in asm_copy_kernel); ol[r] = the block's
// sum of the 16-B padded stream sizes before r, bO[block] the block's sum
__global__ __launch_bounds__(SS_THREADS) void asm_stream_kernel(
    const rxg_segment *__restrict__ seg, const uint32_t *__restrict__ totals,
    const uint64_t *__restrict__ tot, const uint32_t *__restrict__ tl,
    const uint64_t *__restrict__ bT, const uint32_t *__restrict__ s32,
    const uint32_t *__restrict__ fl, const uint32_t *__restrict__ sfirst,
    rxg_tcp_stream *__restrict__ stream, uint32_t *__restrict__ ol, uint64_t *__restrict__ bO) {
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t nseg = totals[0], nst = (uint32_t)tot[1];
    const uint32_t t = threadIdx.x;
    const uint32_t r0 = blockIdx.x * SS_THREADS, r = r0 + t;
    if (r0 >= nst) return; // (uniform)
    uint32_t padded = 0u;
    if (r < nst) {
        const uint32_t first = sfirst[r], next = r + 1u < nst ? sfirst[r + 1u] : nseg;
        const uint64_t g0 = tl[first] + bT[first / SS_THREADS];
        const uint64_t g1 = next < nseg ? tl[next] + bT[next / SS_THREADS] : tot[0];
        rxg_tcp_stream x;
        x.first = first;
        x.nseg = next - first;
        x.seq = s32[first];
        x.ack = seg[next - 1u].ack;
        x.bytes = (uint32_t)(g1 - g0);
        x.offset = 0u;
        x.flags = ((fl[next - 1u] & ASM_F_FINOK) ? RXG_STREAM_FIN : 0u) |
                  ((fl[first] & ASM_F_HOLE) ? RXG_STREAM_HOLE : 0u);
        x.reserved = 0u;
        stream[r] = x;
        padded = (x.bytes + 15u) & ~15u;
    }
    uint32_t total;
    const uint32_t inc = ss_block_scan<false>(padded, ws, total);
    if (r < nst) ol[r] = inc - padded;
    if (t == 0u) bO[blockIdx.x] = total;
}

// a wave per record (bO scanned, tot[2] = the payload bytes used): its offset
// = its stream's offset + the stream's take before it, at any byte phase; then
// its take bytes, [34 + 4*hl + skip, + take) of the frame (ss_copy_bytes); the
// stream's last record zeroes the bytes to the 16-B padded end.  Every byte
// has one writer and no lane reads the destination.
__global__ __launch_bounds__(SS_THREADS) void asm_copy_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint64_t *__restrict__ tot,
    const uint32_t *__restrict__ dl, const uint32_t *__restrict__ tk,
    const uint32_t *__restrict__ tl, const uint64_t *__restrict__ bT,
    const uint32_t *__restrict__ sl, const uint32_t *__restrict__ sfirst,
    const uint32_t *__restrict__ ol, const uint64_t *__restrict__ bO, rxg_segment *__restrict__ seg,
    rxg_tcp_stream *__restrict__ stream, uint8_t *__restrict__ payload, uint64_t cap,
    uint32_t *__restrict__ totals) {
    const uint32_t nseg = totals[0];
    const uint32_t j = blockIdx.x * (SS_THREADS / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) totals[1] = (uint32_t)tot[2];
    if (j >= nseg) return;
    const uint32_t r = sl[j], first = sfirst[r];
    const uint64_t ro = ol[r] + bO[r / SS_THREADS];
    const uint32_t rbytes = stream[r].bytes;
    const uint64_t before = (tl[j] + bT[j / SS_THREADS]) - (tl[first] + bT[first / SS_THREADS]);
    const uint64_t o = ro + before;
    const uint32_t take = tk[j];
    const uint32_t hl = seg[j].hl, frame = seg[j].frame;
    if (lane == 0u) {
        seg[j].offset = (uint32_t)o;
        seg[j].ncopy = (uint16_t)take;
        if (j == first) stream[r].offset = (uint32_t)ro;
    }
    if (ro + ((rbytes + 15u) & ~15u) > cap) { // the whole stream stays unwritten
        if (lane == 0u && j == first) atomicOr(&totals[2], 1u);
        return;
    }
    const bool last = j + 1u == nseg || sl[j + 1u] != r;
    if (last && lane >= 32u && lane < 48u) { // the zero tail: [stream end, padded end)
        const uint64_t end = ro + rbytes;
        if (lane - 32u < ((16u - (uint32_t)(end & 15u)) & 15u)) payload[end + (lane - 32u)] = 0u;
    }
    if (!take) return;
    ss_copy_bytes(pkts + ((uint64_t)off[frame] << unit_log2), len[frame],
                  34u + 4u * hl + ((dl[j] & 0xFFFFu) - take), take, payload, o, lane);
}

} // namespace

// ---- The host side: one workspace description, the stages, and the four
// entry points as compositions of them.
namespace {

inline uint32_t ss_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + SS_TILE - 1) / SS_TILE); }
inline uint32_t ss_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + SS_THREADS - 1) / SS_THREADS); }
inline size_t ss_align(size_t x) { return (x + 255) & ~(size_t)255; }

// every region of the workspace of a burst of n frames, in layout order; a
// form's workspace is the prefix up to its own region's end, so the assembly
// form reserves the coalescing region without using it
struct k4_ws {
    // the sort: keys and values twice (ping-pong), the digit histograms, the
    // record blocks' payload sizes
    uint32_t *ka, *va, *kb, *vb, *hist, *tsum;
    struct { // coalescing; tot = {sum of ncopy, runs, bytes used}
        uint32_t *gl, *hd, *rl, *rfirst, *ol;
        uint64_t *bG, *bH, *bR, *bO, *tot;
    } g;
    struct { // ordering: seq, local head, head index, the (key, position) pair twice
        uint32_t *sq, *hl, *hk, *oka, *pa, *okb, *pb;
        uint64_t *bH, *bZ;
        uint32_t *flag;
    } o;
    struct { // assembly; tot = {sum of take, streams, bytes used}
        uint32_t *dl, *hl, *av, *tk, *s32, *fl, *sl, *sfirst, *ol, *tl;
        uint64_t *il, *bH, *bZ, *bV, *bF, *bR, *bT, *bO, *tot;
    } a;
    size_t end_sort, end_gro, end_order, end_assemble; // rx_*_ws_bytes(n)
};

// the one carve: every array starts 256-B aligned; ws may be null (the sizes only)
k4_ws k4_carve(void *ws, uint32_t n) {
    const size_t nn = n ? n : 1, ntiles = ss_tiles(n) ? ss_tiles(n) : 1,
                 nblk = ss_blocks(n) ? ss_blocks(n) : 1;
    const size_t frame4 = nn * 4, frame8 = nn * 8, blk8 = nblk * 8;
    const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
    size_t at = 0;
    auto take = [&](auto *&p, size_t bytes) {
        p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + at);
        at += ss_align(bytes);
    };
    k4_ws w;
    for (uint32_t **p : {&w.ka, &w.va, &w.kb, &w.vb}) take(*p, frame4);
    take(w.hist, SS_DIGITS * ntiles * 4);
    take(w.tsum, nblk * 4);
    w.end_sort = at;
    for (uint32_t **p : {&w.g.gl, &w.g.hd, &w.g.rl, &w.g.rfirst, &w.g.ol}) take(*p, frame4);
    for (uint64_t **p : {&w.g.bG, &w.g.bH, &w.g.bR, &w.g.bO}) take(*p, blk8);
    take(w.g.tot, 3 * 8);
    w.end_gro = at;
    for (uint32_t **p : {&w.o.sq, &w.o.hl, &w.o.hk, &w.o.oka, &w.o.pa, &w.o.okb, &w.o.pb})
        take(*p, frame4);
    for (uint64_t **p : {&w.o.bH, &w.o.bZ}) take(*p, blk8);
    take(w.o.flag, 4);
    w.end_order = at;
    for (uint32_t **p : {&w.a.dl, &w.a.hl, &w.a.av, &w.a.tk, &w.a.s32, &w.a.fl, &w.a.sl,
                         &w.a.sfirst, &w.a.ol, &w.a.tl})
        take(*p, frame4);
    take(w.a.il, frame8);
    for (uint64_t **p : {&w.a.bH, &w.a.bZ, &w.a.bV, &w.a.bF, &w.a.bR, &w.a.bT, &w.a.bO})
        take(*p, blk8);
    take(w.a.tot, 3 * 8);
    w.end_assemble = at;
    return w;
}

// what every stage of one call works on
struct k4_call {
    const uint8_t *pkts;
    const uint32_t *off;
    const uint16_t *len;
    uint32_t n, unit_log2;
    const uint4 *verd;
    uint32_t nt;
    uint32_t *totals;
    hipStream_t s;
    uint32_t ntiles, nblk;
    k4_ws w;
};

// a (keys, values) array pair of the sort
struct k4_pair {
    uint32_t *k, *v;
};

// one stable radix pass over digit `shift` of (ki, vi) into (ko, vo); the
// first pass of the flow sort reads its keys from the verdicts instead
hipError_t radix_pass(const k4_call &c, const uint32_t *ki, const uint32_t *vi, uint32_t shift,
                      uint32_t *ko, uint32_t *vo, bool first) {
    const dim3 grid(c.ntiles), block(SS_THREADS);
    if (first)
        hipLaunchKernelGGL(ss_hist_kernel<true>, grid, block, 0, c.s, c.verd, nullptr, c.n, c.nt, shift,
                           c.ntiles, c.w.hist, c.totals);
    else
        hipLaunchKernelGGL(ss_hist_kernel<false>, grid, block, 0, c.s, c.verd, ki, c.n, c.nt, shift,
                           c.ntiles, c.w.hist, c.totals);
    hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, c.s, c.w.hist, SS_DIGITS * c.ntiles,
                       nullptr);
    if (first)
        hipLaunchKernelGGL(ss_scatter_kernel<true>, grid, block, 0, c.s, c.verd, nullptr, nullptr, c.n,
                           c.nt, shift, c.ntiles, c.w.hist, ko, vo);
    else
        hipLaunchKernelGGL(ss_scatter_kernel<false>, grid, block, 0, c.s, c.verd, ki, vi, c.n, c.nt,
                           shift, c.ntiles, c.w.hist, ko, vo);
    return hipGetLastError();
}

// `passes` radix passes from digit 0 up, ping-pong between cur and spare;
// afterwards cur holds the result
hipError_t radix_passes(const k4_call &c, k4_pair &cur, k4_pair &spare, uint32_t passes, bool verdicts) {
    for (uint32_t p = 0; p < passes; ++p) {
        const hipError_t e = radix_pass(c, cur.k, cur.v, 8u * p, spare.k, spare.v, verdicts && p == 0);
        if (e != hipSuccess) return e;
        const k4_pair x = cur;
        cur = spare, spare = x;
    }
    return hipSuccess;
}

// the sort stage: the delivered segments by flow id (ids 0..nt-1 and the
// sentinel nt: as many 8-bit digits as that needs); cur = the sorted (flow,
// frame) arrays, spare = the free pair
hipError_t sort_stage(const k4_call &c, k4_pair &cur, k4_pair &spare) {
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(c.nt);
    cur = {c.w.kb, c.w.vb}, spare = {c.w.ka, c.w.va}; // (the first pass reads no input pair)
    return radix_passes(c, cur, spare, (bits + 7u) / 8u, true);
}

// the ordering stage: the group heads, the keys, four key passes (a -> b -> a
// -> b -> a), the head index as the key, its passes (positions 0 .. n-1), and
// the sorted arrays gathered through the permutation into the free pair, which
// becomes cur
hipError_t order_stage(const k4_call &c, k4_pair &cur, k4_pair &spare) {
    const dim3 grid(c.nblk), block(SS_THREADS);
    const auto &o = c.w.o;
    hipError_t e;
    hipLaunchKernelGGL(ord_head_kernel, grid, block, 0, c.s, c.pkts, c.off, c.len, c.unit_log2, cur.k,
                       cur.v, c.totals, o.sq, o.hl, o.bH, o.bZ);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), dim3(1024), 0, c.s, o.bZ, o.bH, c.totals, nullptr);
    hipLaunchKernelGGL(ord_key_kernel, grid, block, 0, c.s, c.totals, c.n, o.sq, o.hl, o.bH, o.oka,
                       o.hk, o.pa, o.flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    k4_pair key = {o.oka, o.pa}, key2 = {o.okb, o.pb};
    if ((e = radix_passes(c, key, key2, 4u, false)) != hipSuccess) return e;
    hipLaunchKernelGGL(ord_headkey_kernel, grid, block, 0, c.s, c.n, o.flag, o.hk, key.v, key.k);
    const uint32_t hbits = c.n > 1u ? 32u - (uint32_t)__builtin_clz(c.n - 1u) : 1u;
    if ((e = radix_passes(c, key, key2, (hbits + 7u) / 8u, false)) != hipSuccess) return e;
    hipLaunchKernelGGL(ord_apply_kernel, grid, block, 0, c.s, c.n, o.flag, key.v, cur.k, cur.v,
                       spare.k, spare.v, c.totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const k4_pair x = cur;
    cur = spare, spare = x;
    return hipSuccess;
}

// a wave per segment
inline dim3 ss_copy_grid(uint32_t n) { return dim3((uint32_t)(((uint64_t)n + 3) / 4)); }

// K4's record stage: the records in place (no payload buffer: offset = the
// payload's offset in its frame), or the records, their offsets and the copy
hipError_t record_stage(const k4_call &c, const k4_pair &cur, rxg_segment *seg, uint8_t *payload,
                        uint64_t cap) {
    const dim3 grid(c.nblk), block(SS_THREADS);
    if (!payload) {
        hipLaunchKernelGGL(ss_record_kernel<true>, grid, block, 0, c.s, c.pkts, c.off, c.len,
                           c.unit_log2, cur.k, cur.v, c.totals, seg, c.w.tsum);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(ss_record_kernel<false>, grid, block, 0, c.s, c.pkts, c.off, c.len, c.unit_log2,
                       cur.k, cur.v, c.totals, seg, c.w.tsum);
    hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, c.s, c.w.tsum, c.nblk, c.totals + 1);
    hipLaunchKernelGGL(ss_copy_kernel, ss_copy_grid(c.n), block, 0, c.s, c.pkts, c.off, c.len,
                       c.unit_log2, c.w.tsum, seg, payload, cap, c.totals);
    return hipGetLastError();
}

// the coalescing stage (g.tot cleared by the caller)
hipError_t coalesce_stage(const k4_call &c, const k4_pair &cur, uint32_t W, rxg_segment *seg,
                          rxg_tcp_run *run, uint8_t *payload, uint64_t cap) {
    const dim3 grid(c.nblk), block(SS_THREADS), one(1), scan(1024);
    const auto &g = c.w.g;
    hipLaunchKernelGGL(gro_record_kernel, grid, block, 0, c.s, c.pkts, c.off, c.len, c.unit_log2,
                       cur.k, cur.v, c.totals, seg, g.gl, g.hd, g.bG, g.bH);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), scan, 0, c.s, g.bG, g.bH, c.totals, g.tot);
    hipLaunchKernelGGL(gro_runhead_kernel, grid, block, 0, c.s, seg, c.totals, W, g.gl, g.hd, g.bG,
                       g.bH, g.rl, g.bR);
    hipLaunchKernelGGL(gro_scan_kernel, one, scan, 0, c.s, g.bR, nullptr, c.totals, g.tot + 1);
    hipLaunchKernelGGL(gro_runid_kernel, grid, block, 0, c.s, c.totals, g.tot, g.rl, g.bR, g.rfirst);
    hipLaunchKernelGGL(gro_run_kernel, grid, block, 0, c.s, c.totals, g.tot, g.gl, g.bG, g.rfirst, run,
                       g.ol, g.bO);
    hipLaunchKernelGGL(gro_scan_kernel, one, scan, 0, c.s, g.bO, nullptr,
                       reinterpret_cast<const uint32_t *>(g.tot + 1), g.tot + 2);
    hipLaunchKernelGGL(gro_copy_kernel, ss_copy_grid(c.n), block, 0, c.s, c.pkts, c.off, c.len,
                       c.unit_log2, g.tot, g.gl, g.bG, g.rl, g.rfirst, g.ol, g.bO, seg, run, payload,
                       cap, c.totals);
    return hipGetLastError();
}

// the assembly stage (a.tot cleared by the caller)
hipError_t assemble_stage(const k4_call &c, const k4_pair &cur, rxg_segment *seg,
                          rxg_tcp_stream *stream, uint8_t *payload, uint64_t cap) {
    const dim3 grid(c.nblk), block(SS_THREADS), one(1), scan(1024);
    const auto &a = c.w.a;
    hipLaunchKernelGGL(asm_record_kernel, grid, block, 0, c.s, c.pkts, c.off, c.len, c.unit_log2,
                       cur.k, cur.v, c.totals, seg, a.dl, a.hl, a.bH, a.bZ);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), scan, 0, c.s, a.bZ, a.bH, c.totals, nullptr);
    hipLaunchKernelGGL(asm_end_kernel, grid, block, 0, c.s, seg, c.totals, a.dl, a.hl, a.bH, a.av,
                       a.il, a.bV, a.bF);
    hipLaunchKernelGGL(asm_scan_kernel, one, scan, 0, c.s, a.bV, a.bF, c.totals);
    hipLaunchKernelGGL(asm_head_kernel, grid, block, 0, c.s, seg, c.totals, a.dl, a.hl, a.av, a.il,
                       a.bV, a.tk, a.s32, a.fl, a.sl, a.tl, a.bR, a.bT);
    hipLaunchKernelGGL(gro_scan_kernel, one, scan, 0, c.s, a.bT, nullptr, c.totals, a.tot);
    hipLaunchKernelGGL(gro_scan_kernel, one, scan, 0, c.s, a.bR, nullptr, c.totals, a.tot + 1);
    hipLaunchKernelGGL(asm_streamid_kernel, grid, block, 0, c.s, c.totals, a.tot, a.fl, a.sl, a.bR,
                       a.sfirst);
    hipLaunchKernelGGL(asm_stream_kernel, grid, block, 0, c.s, seg, c.totals, a.tot, a.tl, a.bT, a.s32,
                       a.fl, a.sfirst, stream, a.ol, a.bO);
    hipLaunchKernelGGL(gro_scan_kernel, one, scan, 0, c.s, a.bO, nullptr,
                       reinterpret_cast<const uint32_t *>(a.tot + 1), a.tot + 2);
    hipLaunchKernelGGL(asm_copy_kernel, ss_copy_grid(c.n), block, 0, c.s, c.pkts, c.off, c.len,
                       c.unit_log2, a.tot, a.dl, a.tk, a.tl, a.bT, a.sl, a.sfirst, a.ol, a.bO, seg,
                       stream, payload, cap, c.totals);
    return hipGetLastError();
}

// the call on a burst of n > 0 frames, its workspace carved
k4_call k4_begin(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                 uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t *totals, void *ws,
                 hipStream_t s) {
    return {pkts, off, len, n, unit_log2, verd, nt, totals, s, ss_tiles(n), ss_blocks(n), k4_carve(ws, n)};
}

} // namespace

size_t rx_segsort_ws_bytes(uint32_t n) { return k4_carve(nullptr, n).end_sort; }
size_t rx_gro_ws_bytes(uint32_t n) { return k4_carve(nullptr, n).end_gro; }
size_t rx_order_ws_bytes(uint32_t n) { return k4_carve(nullptr, n).end_order; }
size_t rx_assemble_ws_bytes(uint32_t n) { return k4_carve(nullptr, n).end_assemble; }

// K4: the sort and the record stage; d_totals: 3 (segments, payload bytes,
// overflow flag)
hipError_t rx_segsort_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                             uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nt,
                             rxg_segment *seg, uint8_t *payload, uint64_t cap, uint32_t *totals,
                             void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 3 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const k4_call c = k4_begin(pkts, off, len, n, unit_log2, verd, nt, totals, ws, s);
    k4_pair cur, spare;
    if ((e = sort_stage(c, cur, spare)) != hipSuccess) return e;
    return record_stage(c, cur, seg, payload, cap);
}

// the sort and the coalescing stage; d_totals: 4 (segments, payload bytes,
// overflow flag, runs)
hipError_t rx_gro_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                         uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t W,
                         rxg_segment *seg, rxg_tcp_run *run, uint8_t *payload, uint64_t cap,
                         uint32_t *totals, void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const k4_call c = k4_begin(pkts, off, len, n, unit_log2, verd, nt, totals, ws, s);
    k4_pair cur, spare;
    if ((e = hipMemsetAsync(c.w.g.tot, 0, 3 * sizeof(uint64_t), s)) != hipSuccess) return e;
    if ((e = sort_stage(c, cur, spare)) != hipSuccess) return e;
    return coalesce_stage(c, cur, W, seg, run, payload, cap);
}

// the sort, the ordering stage, then K4's record stage (W == 0; payload NULL:
// records only) or the coalescing stage (W != 0); d_totals: 5 (segments,
// payload bytes, overflow flag, runs, moved)
hipError_t rx_order_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                           uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t W,
                           rxg_segment *seg, rxg_tcp_run *run, uint8_t *payload, uint64_t cap,
                           uint32_t *totals, void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 5 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const k4_call c = k4_begin(pkts, off, len, n, unit_log2, verd, nt, totals, ws, s);
    k4_pair cur, spare;
    if ((e = hipMemsetAsync(c.w.o.flag, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = sort_stage(c, cur, spare)) != hipSuccess) return e;
    if ((e = order_stage(c, cur, spare)) != hipSuccess) return e;
    if (!W) return record_stage(c, cur, seg, payload, cap);
    if ((e = hipMemsetAsync(c.w.g.tot, 0, 3 * sizeof(uint64_t), s)) != hipSuccess) return e;
    return coalesce_stage(c, cur, W, seg, run, payload, cap);
}

// the sort, the ordering stage and the assembly stage; d_totals: 6 (segments,
// payload bytes, overflow flag, streams, moved, sum of skip)
hipError_t rx_assemble_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                              uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nt,
                              rxg_segment *seg, rxg_tcp_stream *stream, uint8_t *payload,
                              uint64_t cap, uint32_t *totals, void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 6 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const k4_call c = k4_begin(pkts, off, len, n, unit_log2, verd, nt, totals, ws, s);
    k4_pair cur, spare;
    if ((e = hipMemsetAsync(c.w.o.flag, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(c.w.a.tot, 0, 3 * sizeof(uint64_t), s)) != hipSuccess) return e;
    if ((e = sort_stage(c, cur, spare)) != hipSuccess) return e;
    if ((e = order_stage(c, cur, spare)) != hipSuccess) return e;
    return assemble_stage(c, cur, seg, stream, payload, cap);
}
