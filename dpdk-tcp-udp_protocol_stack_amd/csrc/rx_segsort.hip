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
#include <hip/hip_runtime.h>

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
        const uint32_t i = vals[j];
        const uint8_t *f = pkts + ((uint64_t)off[i] << unit_log2);
        const uint32_t cap = len[i];
        auto b = [&](uint32_t k) -> uint32_t { return k < cap ? (uint32_t)f[k] : 0u; };
        const uint32_t tl = (b(16) << 8) | b(17); // ip total_length (tcp.c:391)
        s.frame = i;
        s.flow = keys[j];
        s.seq = (b(38) << 24) | (b(39) << 16) | (b(40) << 8) | b(41);
        s.ack = (b(42) << 24) | (b(43) << 16) | (b(44) << 8) | b(45);
        s.hl = (uint8_t)(b(46) >> 4);
        s.flags = (uint8_t)b(47);
        s.plen = (int32_t)tl - 20 - 4 * (int32_t)s.hl; // tcp.c:145-146 with iTcplen = tl - 20
        s.sport = (uint16_t)(b(34) | (b(35) << 8));
        s.dport = (uint16_t)(b(36) | (b(37) << 8));
        const uint32_t from = 34u + 4u * s.hl;
        const uint32_t avail = cap > from ? cap - from : 0u;
        const uint32_t keep = ((s.flags & 0x08u) && s.plen > 0) ? min((uint32_t)s.plen, avail) : 0u;
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
        const uint32_t a = src + 16u * c, a0 = a & ~3u, sh = a & 3u;
        uint32_t wv[5];
#pragma unroll
        for (uint32_t q = 0; q < 5u; ++q) {
            const uint32_t p = a0 + 4u * q;
            wv[q] = p < fcap ? *reinterpret_cast<const uint32_t *>(f + p) : 0u;
        }
        uint32_t o4[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            o4[q] = sh ? __builtin_amdgcn_alignbyte(wv[q + 1], wv[q], sh) : wv[q];
            const uint32_t b0 = 16u * c + 4u * q;
            const uint32_t keep = ncopy > b0 ? ncopy - b0 : 0u;
            if (keep < 4u) o4[q] &= keep ? ((1u << (8u * keep)) - 1u) : 0u;
        }
        *reinterpret_cast<uint4 *>(payload + o + 16u * c) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
    }
}

inline uint32_t ss_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + SS_TILE - 1) / SS_TILE); }
inline uint32_t ss_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + SS_THREADS - 1) / SS_THREADS); }
inline size_t ss_align(size_t x) { return (x + 255) & ~(size_t)255; }

} // namespace

// workspace: keys and values twice (ping-pong), the digit histograms, the
// record blocks' payload sizes
size_t rx_segsort_ws_bytes(uint32_t n) {
    const size_t nn = n ? n : 1;
    return 4 * ss_align(nn * 4) + ss_align((size_t)SS_DIGITS * (ss_tiles(n) ? ss_tiles(n) : 1) * 4) +
           ss_align((size_t)(ss_blocks(n) ? ss_blocks(n) : 1) * 4);
}

// d_totals: 3 (segments, payload bytes, overflow flag)
hipError_t rx_segsort_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                             uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nt,
                             rxg_segment *seg, uint8_t *payload, uint64_t cap, uint32_t *totals,
                             void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 3 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const size_t nn = ss_align((size_t)n * 4);
    uint8_t *w8 = static_cast<uint8_t *>(ws);
    uint32_t *ka = reinterpret_cast<uint32_t *>(w8), *va = reinterpret_cast<uint32_t *>(w8 + nn);
    uint32_t *kb = reinterpret_cast<uint32_t *>(w8 + 2 * nn), *vb = reinterpret_cast<uint32_t *>(w8 + 3 * nn);
    const uint32_t ntiles = ss_tiles(n), nblk = ss_blocks(n);
    uint32_t *hist = reinterpret_cast<uint32_t *>(w8 + 4 * nn);
    uint32_t *tsum = reinterpret_cast<uint32_t *>(w8 + 4 * nn + ss_align((size_t)SS_DIGITS * ntiles * 4));
    // key bits: ids 0..nt-1 and the sentinel nt
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(nt);
    const uint32_t passes = (bits + 7u) / 8u;
    const uint32_t *kin = nullptr, *vin = nullptr;
    uint32_t *kout = ka, *vout = va;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = 8u * p;
        if (p == 0)
            hipLaunchKernelGGL(ss_hist_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, n, nt, shift, ntiles, hist, totals);
        else
            hipLaunchKernelGGL(ss_hist_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               kin, n, nt, shift, ntiles, hist, totals);
        hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, hist, SS_DIGITS * ntiles,
                           nullptr);
        if (p == 0)
            hipLaunchKernelGGL(ss_scatter_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, nullptr, n, nt, shift, ntiles, hist, kout, vout);
        else
            hipLaunchKernelGGL(ss_scatter_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               kin, vin, n, nt, shift, ntiles, hist, kout, vout);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        kin = kout, vin = vout;
        kout = (kout == ka) ? kb : ka;
        vout = (vout == va) ? vb : va;
    }
    if (!payload) { // in place: records only, offset = the payload's offset in its frame
        hipLaunchKernelGGL(ss_record_kernel<true>, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off,
                           len, unit_log2, kin, vin, totals, seg, tsum);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(ss_record_kernel<false>, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off, len,
                       unit_log2, kin, vin, totals, seg, tsum);
    hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, tsum, nblk, totals + 1);
    hipLaunchKernelGGL(ss_copy_kernel, dim3((uint32_t)(((uint64_t)n + 3) / 4)), dim3(SS_THREADS), 0,
                       s, pkts, off, len, unit_log2, tsum, seg, payload, cap, totals);
    return hipGetLastError();
}

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

// ss_wave_scan with max for +: the lanes shifted in read 0, the identity of
// max on unsigned values as well
__device__ __forceinline__ uint32_t gro_wave_max(uint32_t x) {
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
__device__ __forceinline__ uint32_t gro_block_scan(uint32_t x, uint32_t *ws, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t inc = MAX ? gro_wave_max(x) : ss_wave_scan(x);
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

// the record of sorted segment j, field for field ss_record_kernel's (offset
// left 0), and its link key
__device__ __forceinline__ rxg_segment gro_decode(const uint8_t *__restrict__ pkts,
                                                  const uint32_t *__restrict__ off,
                                                  const uint16_t *__restrict__ len,
                                                  uint32_t unit_log2, const uint32_t *__restrict__ keys,
                                                  const uint32_t *__restrict__ vals, uint32_t j,
                                                  gro_key &k) {
    rxg_segment s;
    const uint32_t i = vals[j];
    const uint8_t *f = pkts + ((uint64_t)off[i] << unit_log2);
    const uint32_t cap = len[i];
    auto b = [&](uint32_t q) -> uint32_t { return q < cap ? (uint32_t)f[q] : 0u; };
    const uint32_t tl = (b(16) << 8) | b(17);
    s.frame = i;
    s.flow = keys[j];
    s.seq = (b(38) << 24) | (b(39) << 16) | (b(40) << 8) | b(41);
    s.ack = (b(42) << 24) | (b(43) << 16) | (b(44) << 8) | b(45);
    s.hl = (uint8_t)(b(46) >> 4);
    s.flags = (uint8_t)b(47);
    s.plen = (int32_t)tl - 20 - 4 * (int32_t)s.hl;
    s.sport = (uint16_t)(b(34) | (b(35) << 8));
    s.dport = (uint16_t)(b(36) | (b(37) << 8));
    const uint32_t from = 34u + 4u * s.hl;
    const uint32_t avail = cap > from ? cap - from : 0u;
    const uint32_t keep = ((s.flags & 0x08u) && s.plen > 0) ? min((uint32_t)s.plen, avail) : 0u;
    s.ncopy = (uint16_t)keep;
    s.offset = 0u;
    k.flow = s.flow;
    k.sip = b(26) | (b(27) << 8) | (b(28) << 16) | (b(29) << 24);
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
    const uint32_t ginc = gro_block_scan<false>(c, ws_g, gsum);
    const uint32_t hinc = gro_block_scan<true>((j < nseg && !link) ? j + 1u : 0u, ws_h, hmax);
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
    const uint32_t inc = gro_block_scan<false>(rh, ws, total);
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
    const uint32_t inc = gro_block_scan<false>(padded, ws, total);
    if (r < nrun) ol[r] = inc - padded;
    if (t == 0u) bO[blockIdx.x] = total;
}

// a wave per segment (bO scanned, tot[2] = the payload bytes used): its
// offset = its run's offset + the run's ncopy before it, at any byte phase;
// then its payload, bytes [34 + 4*hl, + ncopy) of the frame: the bytes up to
// the first 16-B boundary of the destination and those after the last one as
// byte stores, the chunks between as 16-B stores (dword loads realigned with
// v_alignbyte, the source at any phase now); the run's last segment zeroes the
// bytes to the 16-B padded end.  Every byte has one writer and no lane reads
// the destination.
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
    const uint8_t *f = pkts + ((uint64_t)off[s.frame] << unit_log2);
    const uint32_t fcap = len[s.frame];
    const uint32_t src = 34u + 4u * s.hl;
    const uint32_t hlen = min(ncopy, (16u - (uint32_t)(o & 15u)) & 15u);
    const uint32_t nb = (ncopy - hlen) >> 4, tb = hlen + 16u * nb, tlen = ncopy - tb;
    if (lane < hlen) payload[o + lane] = src + lane < fcap ? f[src + lane] : (uint8_t)0u;
    if (lane >= 16u && lane - 16u < tlen) {
        const uint32_t q = tb + (lane - 16u);
        payload[o + q] = src + q < fcap ? f[src + q] : (uint8_t)0u;
    }
    for (uint32_t c = lane; c < nb; c += 64u) {
        const uint32_t a = src + hlen + 16u * c, a0 = a & ~3u, sh = a & 3u;
        uint32_t wv[5];
#pragma unroll
        for (uint32_t q = 0; q < 5u; ++q) {
            const uint32_t p = a0 + 4u * q;
            wv[q] = p < fcap ? *reinterpret_cast<const uint32_t *>(f + p) : 0u;
        }
        uint32_t o4[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q)
            o4[q] = sh ? __builtin_amdgcn_alignbyte(wv[q + 1], wv[q], sh) : wv[q];
        *reinterpret_cast<uint4 *>(payload + o + hlen + 16u * c) =
            make_uint4(o4[0], o4[1], o4[2], o4[3]);
    }
}

} // namespace

// workspace: K4's, then five words per frame (gl, hd, rl, rfirst, ol), four
// 64-bit block arrays (bG, bH, bR, bO) and the three 64-bit totals
size_t rx_gro_ws_bytes(uint32_t n) {
    const size_t nn = n ? n : 1;
    return rx_segsort_ws_bytes(n) + 5 * ss_align(nn * 4) +
           4 * ss_align((size_t)(ss_blocks(n) ? ss_blocks(n) : 1) * 8) + 256;
}

// d_totals: 4 (segments, payload bytes, overflow flag, runs)
hipError_t rx_gro_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                         uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t W,
                         rxg_segment *seg, rxg_tcp_run *run, uint8_t *payload, uint64_t cap,
                         uint32_t *totals, void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const size_t nn = ss_align((size_t)n * 4);
    uint8_t *w8 = static_cast<uint8_t *>(ws);
    uint32_t *ka = reinterpret_cast<uint32_t *>(w8), *va = reinterpret_cast<uint32_t *>(w8 + nn);
    uint32_t *kb = reinterpret_cast<uint32_t *>(w8 + 2 * nn), *vb = reinterpret_cast<uint32_t *>(w8 + 3 * nn);
    const uint32_t ntiles = ss_tiles(n), nblk = ss_blocks(n);
    uint32_t *hist = reinterpret_cast<uint32_t *>(w8 + 4 * nn);
    uint8_t *g8 = w8 + rx_segsort_ws_bytes(n);
    uint32_t *gl = reinterpret_cast<uint32_t *>(g8), *hd = reinterpret_cast<uint32_t *>(g8 + nn);
    uint32_t *rl = reinterpret_cast<uint32_t *>(g8 + 2 * nn);
    uint32_t *rfirst = reinterpret_cast<uint32_t *>(g8 + 3 * nn);
    uint32_t *ol = reinterpret_cast<uint32_t *>(g8 + 4 * nn);
    const size_t nb8 = ss_align((size_t)nblk * 8);
    uint64_t *bG = reinterpret_cast<uint64_t *>(g8 + 5 * nn);
    uint64_t *bH = reinterpret_cast<uint64_t *>(g8 + 5 * nn + nb8);
    uint64_t *bR = reinterpret_cast<uint64_t *>(g8 + 5 * nn + 2 * nb8);
    uint64_t *bO = reinterpret_cast<uint64_t *>(g8 + 5 * nn + 3 * nb8);
    uint64_t *tot = reinterpret_cast<uint64_t *>(g8 + 5 * nn + 4 * nb8); // {sum of ncopy, runs, bytes used}
    if ((e = hipMemsetAsync(tot, 0, 3 * sizeof(uint64_t), s)) != hipSuccess) return e;
    // the sort, as in rx_segsort_launch
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(nt);
    const uint32_t passes = (bits + 7u) / 8u;
    const uint32_t *kin = nullptr, *vin = nullptr;
    uint32_t *kout = ka, *vout = va;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = 8u * p;
        if (p == 0)
            hipLaunchKernelGGL(ss_hist_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, n, nt, shift, ntiles, hist, totals);
        else
            hipLaunchKernelGGL(ss_hist_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               kin, n, nt, shift, ntiles, hist, totals);
        hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, hist, SS_DIGITS * ntiles,
                           nullptr);
        if (p == 0)
            hipLaunchKernelGGL(ss_scatter_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, nullptr, n, nt, shift, ntiles, hist, kout, vout);
        else
            hipLaunchKernelGGL(ss_scatter_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               kin, vin, n, nt, shift, ntiles, hist, kout, vout);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        kin = kout, vin = vout;
        kout = (kout == ka) ? kb : ka;
        vout = (vout == va) ? vb : va;
    }
    hipLaunchKernelGGL(gro_record_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off, len,
                       unit_log2, kin, vin, totals, seg, gl, hd, bG, bH);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), dim3(1024), 0, s, bG, bH, totals, tot);
    hipLaunchKernelGGL(gro_runhead_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, seg, totals, W, gl,
                       hd, bG, bH, rl, bR);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bR, nullptr, totals, tot + 1);
    hipLaunchKernelGGL(gro_runid_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, tot, rl, bR,
                       rfirst);
    hipLaunchKernelGGL(gro_run_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, tot, gl, bG,
                       rfirst, run, ol, bO);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bO, nullptr,
                       reinterpret_cast<const uint32_t *>(tot + 1), tot + 2);
    hipLaunchKernelGGL(gro_copy_kernel, dim3((uint32_t)(((uint64_t)n + 3) / 4)), dim3(SS_THREADS), 0,
                       s, pkts, off, len, unit_log2, tot, gl, bG, rl, rfirst, ol, bO, seg, run,
                       payload, cap, totals);
    return hipGetLastError();
}

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

// what decides a record's group, and its seq
struct ord_key {
    uint32_t flow, sip, ports, movable, seq;
};

// sorted segment j's group key, bytes past the capture read as 0
// (ss_record_kernel's rule)
__device__ __forceinline__ ord_key ord_decode(const uint8_t *__restrict__ pkts,
                                              const uint32_t *__restrict__ off,
                                              const uint16_t *__restrict__ len, uint32_t unit_log2,
                                              const uint32_t *__restrict__ keys,
                                              const uint32_t *__restrict__ vals, uint32_t j) {
    const uint32_t i = vals[j];
    const uint8_t *f = pkts + ((uint64_t)off[i] << unit_log2);
    const uint32_t cap = len[i];
    auto b = [&](uint32_t q) -> uint32_t { return q < cap ? (uint32_t)f[q] : 0u; };
    ord_key k;
    k.flow = keys[j];
    k.sip = b(26) | (b(27) << 8) | (b(28) << 16) | (b(29) << 24);
    k.ports = b(34) | (b(35) << 8) | (b(36) << 16) | (b(37) << 24);
    k.movable = (b(47) & 0x06u) == 0u; // neither SYN nor RST
    k.seq = (b(38) << 24) | (b(39) << 16) | (b(40) << 8) | b(41);
    return k;
}

// round 1: sq[j] = seq; hl[j] = 1 + the last group head at or before j inside
// the block (0: none yet); bH[block] = the block's last head; bZ[block] = 0
// (the sum half of gro_scan_kernel runs beside the max half, on zeros)
__global__ __launch_bounds__(SS_THREADS) void ord_head_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ totals,
    uint32_t *__restrict__ sq, uint32_t *__restrict__ hl, uint64_t *__restrict__ bH,
    uint64_t *__restrict__ bZ) {
    __shared__ uint32_t pf[SS_THREADS + 1u], ps[SS_THREADS + 1u], pp[SS_THREADS + 1u],
        pm[SS_THREADS + 1u];
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    if (j0 >= nseg) return; // (uniform)
    ord_key k = {0u, 0u, 0u, 0u, 0u};
    if (j < nseg) k = ord_decode(pkts, off, len, unit_log2, keys, vals, j);
    pf[t + 1u] = k.flow, ps[t + 1u] = k.sip, pp[t + 1u] = k.ports, pm[t + 1u] = k.movable;
    if (t == 0u) { // the block's predecessor record, decoded again
        ord_key p = {0u, 0u, 0u, 0u, 0u};
        if (j0) p = ord_decode(pkts, off, len, unit_log2, keys, vals, j0 - 1u);
        pf[0] = p.flow, ps[0] = p.sip, pp[0] = p.ports, pm[0] = p.movable;
    }
    __syncthreads();
    const bool head = !j || !k.movable || !pm[t] || pf[t] != k.flow || ps[t] != k.sip ||
                      pp[t] != k.ports;
    uint32_t hmax;
    const uint32_t hinc = gro_block_scan<true>((j < nseg && head) ? j + 1u : 0u, ws, hmax);
    if (j < nseg) {
        sq[j] = k.seq;
        hl[j] = hinc;
    }
    if (t == 0u) {
        bH[blockIdx.x] = hmax;
        bZ[blockIdx.x] = 0u;
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

// workspace: the coalescing form's, then seven words per frame (seq, local
// head, head index, and the (key, position) pair twice), two 64-bit block
// arrays and the flag
size_t rx_order_ws_bytes(uint32_t n) {
    const size_t nn = n ? n : 1;
    return rx_gro_ws_bytes(n) + 7 * ss_align(nn * 4) +
           2 * ss_align((size_t)(ss_blocks(n) ? ss_blocks(n) : 1) * 8) + 256;
}

// K4 (W == 0; payload NULL: records only) or its coalescing form (W != 0) on
// the sequence-ordered segments; d_totals: 5 (segments, payload bytes,
// overflow flag, runs, moved)
hipError_t rx_order_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                           uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t W,
                           rxg_segment *seg, rxg_tcp_run *run, uint8_t *payload, uint64_t cap,
                           uint32_t *totals, void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 5 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const size_t nn = ss_align((size_t)n * 4);
    uint8_t *w8 = static_cast<uint8_t *>(ws);
    uint32_t *ka = reinterpret_cast<uint32_t *>(w8), *va = reinterpret_cast<uint32_t *>(w8 + nn);
    uint32_t *kb = reinterpret_cast<uint32_t *>(w8 + 2 * nn), *vb = reinterpret_cast<uint32_t *>(w8 + 3 * nn);
    const uint32_t ntiles = ss_tiles(n), nblk = ss_blocks(n);
    uint32_t *hist = reinterpret_cast<uint32_t *>(w8 + 4 * nn);
    uint32_t *tsum = reinterpret_cast<uint32_t *>(w8 + 4 * nn + ss_align((size_t)SS_DIGITS * ntiles * 4));
    const size_t nb8 = ss_align((size_t)nblk * 8);
    uint8_t *o8 = w8 + rx_gro_ws_bytes(n);
    uint32_t *sq = reinterpret_cast<uint32_t *>(o8), *hl = reinterpret_cast<uint32_t *>(o8 + nn);
    uint32_t *hk = reinterpret_cast<uint32_t *>(o8 + 2 * nn);
    uint32_t *oka = reinterpret_cast<uint32_t *>(o8 + 3 * nn), *pa = reinterpret_cast<uint32_t *>(o8 + 4 * nn);
    uint32_t *okb = reinterpret_cast<uint32_t *>(o8 + 5 * nn), *pb = reinterpret_cast<uint32_t *>(o8 + 6 * nn);
    uint64_t *bH = reinterpret_cast<uint64_t *>(o8 + 7 * nn);
    uint64_t *bZ = reinterpret_cast<uint64_t *>(o8 + 7 * nn + nb8);
    uint32_t *flag = reinterpret_cast<uint32_t *>(o8 + 7 * nn + 2 * nb8);
    if ((e = hipMemsetAsync(flag, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    // one stable radix pass of K4's sort over digit `shift` of (ki, vi)
    auto pass = [&](const uint32_t *ki, const uint32_t *vi, uint32_t shift, uint32_t *ko,
                    uint32_t *vo) -> hipError_t {
        hipLaunchKernelGGL(ss_hist_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd, ki, n,
                           nt, shift, ntiles, hist, totals);
        hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, hist, SS_DIGITS * ntiles,
                           nullptr);
        hipLaunchKernelGGL(ss_scatter_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd, ki,
                           vi, n, nt, shift, ntiles, hist, ko, vo);
        return hipGetLastError();
    };
    // the sort, as in rx_segsort_launch
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(nt);
    const uint32_t passes = (bits + 7u) / 8u;
    const uint32_t *kin = nullptr, *vin = nullptr;
    uint32_t *kout = ka, *vout = va;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = 8u * p;
        if (p == 0) {
            hipLaunchKernelGGL(ss_hist_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, n, nt, shift, ntiles, hist, totals);
            hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, hist, SS_DIGITS * ntiles,
                               nullptr);
            hipLaunchKernelGGL(ss_scatter_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, nullptr, n, nt, shift, ntiles, hist, kout, vout);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        } else if ((e = pass(kin, vin, shift, kout, vout)) != hipSuccess) {
            return e;
        }
        kin = kout, vin = vout;
        kout = (kout == ka) ? kb : ka;
        vout = (vout == va) ? vb : va;
    }
    // the permutation: keys, four key passes (a -> b -> a -> b -> a), the head
    // index as the key, its passes (positions 0 .. n-1)
    hipLaunchKernelGGL(ord_head_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off, len, unit_log2,
                       kin, vin, totals, sq, hl, bH, bZ);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), dim3(1024), 0, s, bZ, bH, totals, nullptr);
    hipLaunchKernelGGL(ord_key_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, n, sq, hl, bH, oka,
                       hk, pa, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t *ok = oka, *pv = pa, *ok2 = okb, *pv2 = pb;
    for (uint32_t p = 0; p < 4u; ++p) {
        if ((e = pass(ok, pv, 8u * p, ok2, pv2)) != hipSuccess) return e;
        uint32_t *x = ok; ok = ok2, ok2 = x;
        x = pv, pv = pv2, pv2 = x;
    }
    hipLaunchKernelGGL(ord_headkey_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, n, flag, hk, pv, ok);
    const uint32_t hbits = n > 1u ? 32u - (uint32_t)__builtin_clz(n - 1u) : 1u;
    for (uint32_t p = 0; p < (hbits + 7u) / 8u; ++p) {
        if ((e = pass(ok, pv, 8u * p, ok2, pv2)) != hipSuccess) return e;
        uint32_t *x = ok; ok = ok2, ok2 = x;
        x = pv, pv = pv2, pv2 = x;
    }
    hipLaunchKernelGGL(ord_apply_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, n, flag, pv, kin, vin,
                       kout, vout, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    kin = kout, vin = vout;
    if (!W) { // K4's record stage, as in rx_segsort_launch
        if (!payload) {
            hipLaunchKernelGGL(ss_record_kernel<true>, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off,
                               len, unit_log2, kin, vin, totals, seg, tsum);
            return hipGetLastError();
        }
        hipLaunchKernelGGL(ss_record_kernel<false>, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off,
                           len, unit_log2, kin, vin, totals, seg, tsum);
        hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, tsum, nblk, totals + 1);
        hipLaunchKernelGGL(ss_copy_kernel, dim3((uint32_t)(((uint64_t)n + 3) / 4)), dim3(SS_THREADS),
                           0, s, pkts, off, len, unit_log2, tsum, seg, payload, cap, totals);
        return hipGetLastError();
    }
    // the coalescing stage, as in rx_gro_launch
    uint8_t *g8 = w8 + rx_segsort_ws_bytes(n);
    uint32_t *gl = reinterpret_cast<uint32_t *>(g8), *hd = reinterpret_cast<uint32_t *>(g8 + nn);
    uint32_t *rl = reinterpret_cast<uint32_t *>(g8 + 2 * nn);
    uint32_t *rfirst = reinterpret_cast<uint32_t *>(g8 + 3 * nn);
    uint32_t *ol = reinterpret_cast<uint32_t *>(g8 + 4 * nn);
    uint64_t *bG = reinterpret_cast<uint64_t *>(g8 + 5 * nn);
    uint64_t *bHg = reinterpret_cast<uint64_t *>(g8 + 5 * nn + nb8);
    uint64_t *bR = reinterpret_cast<uint64_t *>(g8 + 5 * nn + 2 * nb8);
    uint64_t *bO = reinterpret_cast<uint64_t *>(g8 + 5 * nn + 3 * nb8);
    uint64_t *tot = reinterpret_cast<uint64_t *>(g8 + 5 * nn + 4 * nb8); // {sum of ncopy, runs, bytes used}
    if ((e = hipMemsetAsync(tot, 0, 3 * sizeof(uint64_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(gro_record_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off, len,
                       unit_log2, kin, vin, totals, seg, gl, hd, bG, bHg);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), dim3(1024), 0, s, bG, bHg, totals, tot);
    hipLaunchKernelGGL(gro_runhead_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, seg, totals, W, gl,
                       hd, bG, bHg, rl, bR);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bR, nullptr, totals, tot + 1);
    hipLaunchKernelGGL(gro_runid_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, tot, rl, bR,
                       rfirst);
    hipLaunchKernelGGL(gro_run_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, tot, gl, bG,
                       rfirst, run, ol, bO);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bO, nullptr,
                       reinterpret_cast<const uint32_t *>(tot + 1), tot + 2);
    hipLaunchKernelGGL(gro_copy_kernel, dim3((uint32_t)(((uint64_t)n + 3) / 4)), dim3(SS_THREADS), 0,
                       s, pkts, off, len, unit_log2, tot, gl, bG, rl, rfirst, ol, bO, seg, run,
                       payload, cap, totals);
    return hipGetLastError();
}

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
// asm_copy_kernel), dl[j] = dlen and the ASM_USABLE / ASM_FIN bits, hl[j] =
// 1 + the last group head at or before j inside the block (0: none yet);
// bH[block] = the block's last head, bZ[block] = 0 (ord_head_kernel's pair)
__global__ __launch_bounds__(SS_THREADS) void asm_record_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off,
    const uint16_t *__restrict__ len, uint32_t unit_log2, const uint32_t *__restrict__ keys,
    const uint32_t *__restrict__ vals, const uint32_t *__restrict__ totals,
    rxg_segment *__restrict__ seg, uint32_t *__restrict__ dl, uint32_t *__restrict__ hl,
    uint64_t *__restrict__ bH, uint64_t *__restrict__ bZ) {
    __shared__ uint32_t pf[SS_THREADS + 1u], ps[SS_THREADS + 1u], pp[SS_THREADS + 1u],
        pm[SS_THREADS + 1u];
    __shared__ uint32_t ws[SS_THREADS / 64u];
    const uint32_t nseg = totals[0];
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blockIdx.x * SS_THREADS, j = j0 + t;
    if (j0 >= nseg) return; // (uniform)
    ord_key k = {0u, 0u, 0u, 0u, 0u};
    if (j < nseg) {
        k = ord_decode(pkts, off, len, unit_log2, keys, vals, j);
        const uint32_t i = vals[j];
        const uint8_t *f = pkts + ((uint64_t)off[i] << unit_log2);
        const uint32_t cap = len[i];
        auto b = [&](uint32_t q) -> uint32_t { return q < cap ? (uint32_t)f[q] : 0u; };
        const uint32_t tl = (b(16) << 8) | b(17);
        rxg_segment s;
        s.frame = i;
        s.flow = k.flow;
        s.seq = k.seq;
        s.ack = (b(42) << 24) | (b(43) << 16) | (b(44) << 8) | b(45);
        s.hl = (uint8_t)(b(46) >> 4);
        s.flags = (uint8_t)b(47);
        s.plen = (int32_t)tl - 20 - 4 * (int32_t)s.hl;
        s.offset = 0u;
        s.sport = (uint16_t)(k.ports & 0xFFFFu);
        s.dport = (uint16_t)(k.ports >> 16);
        s.ncopy = 0u;
        seg[j] = s;
        const uint32_t from = 34u + 4u * s.hl;
        const uint32_t avail = cap > from ? cap - from : 0u;
        const bool usable = s.plen <= 0 || avail >= (uint32_t)s.plen;
        // (a SYN or RST record is left alone: no data, no FIN)
        uint32_t d = (k.movable && usable && s.plen > 0) ? (uint32_t)s.plen : 0u;
        if (usable) d |= ASM_USABLE;
        if (k.movable && usable && (s.flags & 0x01u)) d |= ASM_FIN;
        dl[j] = d;
    }
    pf[t + 1u] = k.flow, ps[t + 1u] = k.sip, pp[t + 1u] = k.ports, pm[t + 1u] = k.movable;
    if (t == 0u) { // the block's predecessor record, decoded again
        ord_key p = {0u, 0u, 0u, 0u, 0u};
        if (j0) p = ord_decode(pkts, off, len, unit_log2, keys, vals, j0 - 1u);
        pf[0] = p.flow, ps[0] = p.sip, pp[0] = p.ports, pm[0] = p.movable;
    }
    __syncthreads();
    const bool head = !j || !k.movable || !pm[t] || pf[t] != k.flow || ps[t] != k.sip ||
                      pp[t] != k.ports;
    uint32_t hmax;
    const uint32_t hinc = gro_block_scan<true>((j < nseg && head) ? j + 1u : 0u, ws, hmax);
    if (j < nseg) hl[j] = hinc;
    if (t == 0u) {
        bH[blockIdx.x] = hmax;
        bZ[blockIdx.x] = 0u;
    }
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
    const uint32_t rinc = gro_block_scan<false>(start, ws_r, rsum);
    const uint32_t tinc = gro_block_scan<false>(take, ws_t, tsum);
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
    const uint32_t inc = gro_block_scan<false>(padded, ws, total);
    if (r < nst) ol[r] = inc - padded;
    if (t == 0u) bO[blockIdx.x] = total;
}

// a wave per record (bO scanned, tot[2] = the payload bytes used): its offset
// = its stream's offset + the stream's take before it, at any byte phase; then
// its take bytes, [34 + 4*hl + skip, + take) of the frame, as gro_copy_kernel
// copies a payload: the bytes up to the first 16-B boundary of the destination
// and those after the last one as byte stores, the chunks between as 16-B
// stores (dword loads realigned with v_alignbyte); the stream's last record
// zeroes the bytes to the 16-B padded end.  Every byte has one writer and no
// lane reads the destination.
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
    const uint8_t *f = pkts + ((uint64_t)off[frame] << unit_log2);
    const uint32_t fcap = len[frame];
    const uint32_t src = 34u + 4u * hl + ((dl[j] & 0xFFFFu) - take);
    const uint32_t hlen = min(take, (16u - (uint32_t)(o & 15u)) & 15u);
    const uint32_t nb = (take - hlen) >> 4, tb = hlen + 16u * nb, tlen = take - tb;
    if (lane < hlen) payload[o + lane] = src + lane < fcap ? f[src + lane] : (uint8_t)0u;
    if (lane >= 16u && lane - 16u < tlen) {
        const uint32_t q = tb + (lane - 16u);
        payload[o + q] = src + q < fcap ? f[src + q] : (uint8_t)0u;
    }
    for (uint32_t c = lane; c < nb; c += 64u) {
        const uint32_t a = src + hlen + 16u * c, a0 = a & ~3u, sh = a & 3u;
        uint32_t wv[5];
#pragma unroll
        for (uint32_t q = 0; q < 5u; ++q) {
            const uint32_t p = a0 + 4u * q;
            wv[q] = p < fcap ? *reinterpret_cast<const uint32_t *>(f + p) : 0u;
        }
        uint32_t o4[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q)
            o4[q] = sh ? __builtin_amdgcn_alignbyte(wv[q + 1], wv[q], sh) : wv[q];
        *reinterpret_cast<uint4 *>(payload + o + hlen + 16u * c) =
            make_uint4(o4[0], o4[1], o4[2], o4[3]);
    }
}

} // namespace

// workspace: the ordering form's, then ten words and one 64-bit word per frame
// (dl, hl, av, tk, s32, fl, sl, sfirst, ol, tl; il), seven 64-bit block
// arrays (bH, bZ, bV, bF, bR, bT, bO) and the three 64-bit totals
size_t rx_assemble_ws_bytes(uint32_t n) {
    const size_t nn = n ? n : 1;
    return rx_order_ws_bytes(n) + 10 * ss_align(nn * 4) + ss_align(nn * 8) +
           7 * ss_align((size_t)(ss_blocks(n) ? ss_blocks(n) : 1) * 8) + 256;
}

// the sort, the ordering stage and the stream assembly; d_totals: 6 (segments,
// payload bytes, overflow flag, streams, moved, sum of skip)
hipError_t rx_assemble_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                              uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nt,
                              rxg_segment *seg, rxg_tcp_stream *stream, uint8_t *payload,
                              uint64_t cap, uint32_t *totals, void *ws, hipStream_t s) {
    hipError_t e = hipMemsetAsync(totals, 0, 6 * sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0 || nt == 0) return e;
    const size_t nn = ss_align((size_t)n * 4);
    uint8_t *w8 = static_cast<uint8_t *>(ws);
    uint32_t *ka = reinterpret_cast<uint32_t *>(w8), *va = reinterpret_cast<uint32_t *>(w8 + nn);
    uint32_t *kb = reinterpret_cast<uint32_t *>(w8 + 2 * nn), *vb = reinterpret_cast<uint32_t *>(w8 + 3 * nn);
    const uint32_t ntiles = ss_tiles(n), nblk = ss_blocks(n);
    uint32_t *hist = reinterpret_cast<uint32_t *>(w8 + 4 * nn);
    const size_t nb8 = ss_align((size_t)nblk * 8);
    uint8_t *o8 = w8 + rx_gro_ws_bytes(n);
    uint32_t *sq = reinterpret_cast<uint32_t *>(o8), *ohl = reinterpret_cast<uint32_t *>(o8 + nn);
    uint32_t *hk = reinterpret_cast<uint32_t *>(o8 + 2 * nn);
    uint32_t *oka = reinterpret_cast<uint32_t *>(o8 + 3 * nn), *pa = reinterpret_cast<uint32_t *>(o8 + 4 * nn);
    uint32_t *okb = reinterpret_cast<uint32_t *>(o8 + 5 * nn), *pb = reinterpret_cast<uint32_t *>(o8 + 6 * nn);
    uint64_t *obH = reinterpret_cast<uint64_t *>(o8 + 7 * nn);
    uint64_t *obZ = reinterpret_cast<uint64_t *>(o8 + 7 * nn + nb8);
    uint32_t *flag = reinterpret_cast<uint32_t *>(o8 + 7 * nn + 2 * nb8);
    uint8_t *a8 = w8 + rx_order_ws_bytes(n);
    uint32_t *dl = reinterpret_cast<uint32_t *>(a8), *hl = reinterpret_cast<uint32_t *>(a8 + nn);
    uint32_t *av = reinterpret_cast<uint32_t *>(a8 + 2 * nn), *tk = reinterpret_cast<uint32_t *>(a8 + 3 * nn);
    uint32_t *s32 = reinterpret_cast<uint32_t *>(a8 + 4 * nn), *fl = reinterpret_cast<uint32_t *>(a8 + 5 * nn);
    uint32_t *sl = reinterpret_cast<uint32_t *>(a8 + 6 * nn);
    uint32_t *sfirst = reinterpret_cast<uint32_t *>(a8 + 7 * nn);
    uint32_t *ol = reinterpret_cast<uint32_t *>(a8 + 8 * nn), *tl = reinterpret_cast<uint32_t *>(a8 + 9 * nn);
    const size_t n8 = ss_align((size_t)n * 8);
    uint64_t *il = reinterpret_cast<uint64_t *>(a8 + 10 * nn);
    uint8_t *b8 = a8 + 10 * nn + n8;
    uint64_t *bH = reinterpret_cast<uint64_t *>(b8), *bZ = reinterpret_cast<uint64_t *>(b8 + nb8);
    uint64_t *bV = reinterpret_cast<uint64_t *>(b8 + 2 * nb8), *bF = reinterpret_cast<uint64_t *>(b8 + 3 * nb8);
    uint64_t *bR = reinterpret_cast<uint64_t *>(b8 + 4 * nb8), *bT = reinterpret_cast<uint64_t *>(b8 + 5 * nb8);
    uint64_t *bO = reinterpret_cast<uint64_t *>(b8 + 6 * nb8);
    uint64_t *tot = reinterpret_cast<uint64_t *>(b8 + 7 * nb8); // {sum of take, streams, bytes used}
    if ((e = hipMemsetAsync(flag, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(tot, 0, 3 * sizeof(uint64_t), s)) != hipSuccess) return e;
    // one stable radix pass of K4's sort over digit `shift` of (ki, vi)
    auto pass = [&](const uint32_t *ki, const uint32_t *vi, uint32_t shift, uint32_t *ko,
                    uint32_t *vo) -> hipError_t {
        hipLaunchKernelGGL(ss_hist_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd, ki, n,
                           nt, shift, ntiles, hist, totals);
        hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, hist, SS_DIGITS * ntiles,
                           nullptr);
        hipLaunchKernelGGL(ss_scatter_kernel<false>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd, ki,
                           vi, n, nt, shift, ntiles, hist, ko, vo);
        return hipGetLastError();
    };
    // the sort, as in rx_segsort_launch
    const uint32_t bits = 32u - (uint32_t)__builtin_clz(nt);
    const uint32_t passes = (bits + 7u) / 8u;
    const uint32_t *kin = nullptr, *vin = nullptr;
    uint32_t *kout = ka, *vout = va;
    for (uint32_t p = 0; p < passes; ++p) {
        const uint32_t shift = 8u * p;
        if (p == 0) {
            hipLaunchKernelGGL(ss_hist_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, n, nt, shift, ntiles, hist, totals);
            hipLaunchKernelGGL(ss_scan_kernel, dim3(1), dim3(1024), 0, s, hist, SS_DIGITS * ntiles,
                               nullptr);
            hipLaunchKernelGGL(ss_scatter_kernel<true>, dim3(ntiles), dim3(SS_THREADS), 0, s, verd,
                               nullptr, nullptr, n, nt, shift, ntiles, hist, kout, vout);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        } else if ((e = pass(kin, vin, shift, kout, vout)) != hipSuccess) {
            return e;
        }
        kin = kout, vin = vout;
        kout = (kout == ka) ? kb : ka;
        vout = (vout == va) ? vb : va;
    }
    // the permutation, as in rx_order_launch
    hipLaunchKernelGGL(ord_head_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off, len, unit_log2,
                       kin, vin, totals, sq, ohl, obH, obZ);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), dim3(1024), 0, s, obZ, obH, totals, nullptr);
    hipLaunchKernelGGL(ord_key_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, n, sq, ohl, obH,
                       oka, hk, pa, flag);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t *ok = oka, *pv = pa, *ok2 = okb, *pv2 = pb;
    for (uint32_t p = 0; p < 4u; ++p) {
        if ((e = pass(ok, pv, 8u * p, ok2, pv2)) != hipSuccess) return e;
        uint32_t *x = ok; ok = ok2, ok2 = x;
        x = pv, pv = pv2, pv2 = x;
    }
    hipLaunchKernelGGL(ord_headkey_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, n, flag, hk, pv, ok);
    const uint32_t hbits = n > 1u ? 32u - (uint32_t)__builtin_clz(n - 1u) : 1u;
    for (uint32_t p = 0; p < (hbits + 7u) / 8u; ++p) {
        if ((e = pass(ok, pv, 8u * p, ok2, pv2)) != hipSuccess) return e;
        uint32_t *x = ok; ok = ok2, ok2 = x;
        x = pv, pv = pv2, pv2 = x;
    }
    hipLaunchKernelGGL(ord_apply_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, n, flag, pv, kin, vin,
                       kout, vout, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    kin = kout, vin = vout;
    // the assembly
    hipLaunchKernelGGL(asm_record_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, pkts, off, len,
                       unit_log2, kin, vin, totals, seg, dl, hl, bH, bZ);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(2), dim3(1024), 0, s, bZ, bH, totals, nullptr);
    hipLaunchKernelGGL(asm_end_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, seg, totals, dl, hl, bH,
                       av, il, bV, bF);
    hipLaunchKernelGGL(asm_scan_kernel, dim3(1), dim3(1024), 0, s, bV, bF, totals);
    hipLaunchKernelGGL(asm_head_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, seg, totals, dl, hl, av,
                       il, bV, tk, s32, fl, sl, tl, bR, bT);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bT, nullptr, totals, tot);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bR, nullptr, totals, tot + 1);
    hipLaunchKernelGGL(asm_streamid_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, totals, tot, fl, sl,
                       bR, sfirst);
    hipLaunchKernelGGL(asm_stream_kernel, dim3(nblk), dim3(SS_THREADS), 0, s, seg, totals, tot, tl,
                       bT, s32, fl, sfirst, stream, ol, bO);
    hipLaunchKernelGGL(gro_scan_kernel, dim3(1), dim3(1024), 0, s, bO, nullptr,
                       reinterpret_cast<const uint32_t *>(tot + 1), tot + 2);
    hipLaunchKernelGGL(asm_copy_kernel, dim3((uint32_t)(((uint64_t)n + 3) / 4)), dim3(SS_THREADS), 0,
                       s, pkts, off, len, unit_log2, tot, dl, tk, tl, bT, sl, sfirst, ol, bO, seg,
                       stream, payload, cap, totals);
    return hipGetLastError();
}
