// rx_l2.hip — K8: the L2 responder over a classified burst (gfx950).  An ARP
// request for a local address and an ICMP echo request to one are answered
// with complete frames, packed as K5 packs its output.  The rule is stated in
// include/rxgpu.h ("L2 responder") and restated on the CPU in
// csrc/rx_l2_host.cpp.  Five launches per burst (K7's judge / scan / emit
// shape, with the message sums and the answers' layout as stages of their
// own), all ordered by the stream:
//
//   judge   a lane per frame, tiles of L2_T: the verdict (one 16-B load per
//           lane, coalesced), and only for cls ARP / IPV4_OTHER the frame's
//           first 48 bytes (three 16-B loads from the 16-B aligned frame
//           start).  Status bytes go through LDS and leave as dwords, as
//           K7's.  An echo request whose message lies inside the capture is a
//           candidate: its index is compacted by ballot into a list (one
//           atomic per wave; the order of the list is of no consequence).  The
//           tile's counts and its ARP answers' space go to the workspace; the
//           per-frame answer sizes are stored only by tiles that have any.
//   sum     a wave per echo candidate: the message from frame byte 34 in
//           aligned 16-B pieces, head and tail masked, 16-bit words added
//           with dot2, then a DPP fold.  It decides ECHO / ECHO_BAD and
//           leaves the answer's checksum beside its size.  A wave takes a
//           run of the list (a run is mostly one tile's) and adds what it
//           found to a tile's counts when the tile changes: same-line atomics
//           serialise, so one per wave and tile, not three per frame
//           (integer atomics: any order gives the same sums).
//   scan    one block: exclusive prefix of the tiles' 64-B units and answer
//           counts, the four status totals, and, when every answer fits
//           cap_bytes, answers written and span.
//   place   a lane per frame, tiles with an answer only: the answer's index k
//           and offset; roff / rlen / rsrc of the answers that fit cap_bytes.
//           Only when the burst is cut: answers written and span by one
//           atomicMax pair per wave.
//   emit    a wave per answer.  Request and answer have the same byte phase
//           (frame start 16-B aligned, slot 64-B aligned, every byte keeps its
//           offset), so the body is aligned 16-B loads and stores; the first
//           48 bytes are rebuilt in registers; the same wave zeroes the pad.
//           Every byte of a slot has one writer.
#include <hip/hip_runtime.h>

#include "rx_common.h"
#include "rx_device.h"

namespace {

constexpr uint32_t L2_T = 256; // frames per tile = threads per block

// per tile: {64-B units, answers, ARP_REQ, ARP_REPLY}, {ECHO_BAD, 0, 0, 0};
// the echo answers are nans - areq.  units | nans << 32 is one 8-B word.
struct alignas(32) l2_part {
    uint32_t units, nans, areq, arep, bad, r0, r1, r2;
};
// the workspace's first 16 bytes: the candidate count (zero between calls:
// the scan stage, the last to read it, clears it) and the cut flag
struct l2_ctl {
    uint32_t ncand, cut, r0, r1;
};

__device__ __forceinline__ const uint8_t *l2_frame(const uint8_t *pkts, const uint32_t *off, uint64_t i,
                                                   uint32_t ul) {
    return pkts + ((uint64_t)off[i] << ul);
}

// frame bytes 0-47 as twelve dwords; byte / field access folds to shifts
struct l2_head {
    uint32_t w[12];
};
__device__ __forceinline__ l2_head l2_load_head(const uint8_t *fb) {
    const uint4 c0 = ldg16<false>(fb), c1 = ldg16<false>(fb + 16), c2 = ldg16<false>(fb + 32);
    return l2_head{{c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w}};
}
__device__ __forceinline__ uint32_t hb(const l2_head &h, uint32_t b) { return (h.w[b >> 2] >> (8u * (b & 3u))) & 0xFFu; }
__device__ __forceinline__ uint32_t hbe16(const l2_head &h, uint32_t b) { return (hb(h, b) << 8) | hb(h, b + 1); }
__device__ __forceinline__ uint32_t hraw32(const l2_head &h, uint32_t b) {
    return hb(h, b) | (hb(h, b + 1) << 8) | (hb(h, b + 2) << 16) | (hb(h, b + 3) << 24);
}
__device__ __forceinline__ uint32_t pk4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return a | (b << 8) | (c << 16) | (d << 24);
}

__device__ __forceinline__ int l2_local(const rxg_l2_params &p, uint32_t ip) {
    int j = -1;
#pragma unroll
    for (int k = RXG_L2_MAX_LOCAL - 1; k >= 0; --k)
        if ((uint32_t)k < p.nlocal && p.local[k].ip == ip) j = k; // (the first match wins)
    return j;
}

// the status of a frame from its head; for an echo request *alen = 14 + tl
__device__ __forceinline__ uint32_t l2_judge(const l2_head &h, uint32_t cls, uint32_t len,
                                             const rxg_l2_params &p, uint32_t *alen) {
    *alen = 0;
    if (hb(h, 6) & 1u) return 0;
    if (cls == (uint32_t)RXG_CLS_ARP) {
        // bytes 14-19: 00 01 08 00 06 04
        if (hraw32(h, 14) != 0x00080100u || hb(h, 18) != 6u || hb(h, 19) != 4u) return 0;
        if (l2_local(p, hraw32(h, 38)) < 0) return 0;
        const uint32_t op = hbe16(h, 20);
        if (op == 1u) *alen = 42u;
        return op == 1u ? RXG_L2_ARP_REQ : op == 2u ? RXG_L2_ARP_REPLY : 0u;
    }
    if (hb(h, 14) != 0x45u || hb(h, 23) != 1u || (hbe16(h, 20) & 0x3FFFu) != 0u) return 0;
    if (l2_local(p, hraw32(h, 30)) < 0) return 0;
    if (hb(h, 34) != 8u || hb(h, 35) != 0u) return 0;
    const uint32_t tl = hbe16(h, 16);
    if (tl < 28u) return 0;
    if (14u + tl > len) return RXG_L2_ECHO_BAD;
    *alen = 14u + tl;
    return RXG_L2_ECHO; // (until the sum stage has seen the message)
}

__global__ __launch_bounds__(256) void l2_judge_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off, const uint16_t *__restrict__ len,
    uint32_t n, uint32_t ul, const uint4 *__restrict__ verd, const rxg_l2_params p,
    uint8_t *__restrict__ status, uint32_t *__restrict__ size, uint32_t *__restrict__ cand,
    l2_ctl *__restrict__ ctl, l2_part *__restrict__ part) {
    __shared__ alignas(16) uint8_t s_st[L2_T];
    __shared__ uint32_t s_cnt[4][5];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * L2_T, i = i0 + tid;
    uint32_t st = 0, alen = 0;
    if (i < n && p.nlocal) {
        const uint4 v = ld_slot(verd + i); // {flow_id, off|len, cksum|cls|rc, ..}
        const uint32_t cls = (v.z >> 16) & 0xFFu;
        if (cls == (uint32_t)RXG_CLS_ARP || cls == (uint32_t)RXG_CLS_IPV4_OTHER) {
            const uint32_t ln = len[i];
            if (ln >= 42u) st = l2_judge(l2_load_head(l2_frame(pkts, off, i, ul)), cls, ln, p, &alen);
        }
    }
    // the echo requests to sum: one atomic per wave
    const bool echo = st == RXG_L2_ECHO;
    const uint64_t em = __ballot(echo);
    if (em) {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(&ctl->ncand, (uint32_t)__popcll(em));
        b = __builtin_amdgcn_readfirstlane(b);
        if (echo) cand[b + (uint32_t)__popcll(em & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
    const uint32_t c0 = (uint32_t)__popcll(__ballot(st == RXG_L2_ARP_REQ));
    const uint32_t c1 = (uint32_t)__popcll(__ballot(st == RXG_L2_ARP_REPLY));
    const uint32_t c3 = (uint32_t)__popcll(__ballot(st == RXG_L2_ECHO_BAD));
    if (lane == 0)
        s_cnt[wv][0] = c0, s_cnt[wv][1] = c1, s_cnt[wv][2] = c3, s_cnt[wv][3] = (uint32_t)__popcll(em);
    s_st[tid] = (uint8_t)st;
    __syncthreads();
    uint32_t t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
    // (an ARP answer is 42 bytes: one 64-B unit; the echo answers are added by
    // the sum stage)
    if (tid == 0) part[blockIdx.x] = l2_part{t[0], t[0], t[0], t[1], t[2], 0u, 0u, 0u};
    // the answer sizes, only where the tile has a use for them (block-uniform);
    // an echo candidate's holds 14 + tl for the sum stage
    if ((t[0] | t[3]) != 0u && i < n) size[i] = alen;
    // four status bytes per lane of the first wave: a dword store where the
    // four lie inside the burst and the address allows, bytes at the edge
    if (tid < L2_T / 4) {
        const uint64_t b = i0 + 4u * tid;
        uint8_t *dst = status + b;
        if (b + 4 <= n && ((uintptr_t)dst & 3u) == 0) {
            *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(&s_st[4u * tid]);
        } else {
            for (uint32_t k = 0; k < 4u && b + k < n; ++k) dst[k] = s_st[4u * tid + k];
        }
    }
}

// A wave per echo candidate.  T is the plain integer sum of the message's
// 16-bit words as the loads give them (little-endian; a one's-complement sum
// commutes with the byte swap, and the message starts at the even frame offset
// 34, so the words are the halves of the aligned dwords).  The request is good
// iff fold(T) == 0xFFFF.  The answer's message is the request's with the
// type / code word 08 00 (LE 0x0008) turned to 00 00 and the checksum field C
// taken as 0, so its integer sum is X = T - 0x0008 - C, exactly, and its
// checksum is ~fold(X).  fold of an integer is 0 only for X == 0 and otherwise
// lies in 1..0xFFFF, which gives the two end cases as a from-scratch sum does:
// an all-zero answer message (X == 0) stores 0xFFFF, and one whose words add
// to a non-zero multiple of 0xFFFF (fold 0xFFFF) stores 0x0000.
__global__ __launch_bounds__(256) void l2_sum_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off, uint32_t ul,
    const uint32_t *__restrict__ cand, const l2_ctl *__restrict__ ctl, uint8_t *__restrict__ status,
    uint32_t *__restrict__ size, l2_part *__restrict__ part) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nw = gridDim.x * (L2_T / 64u), w0 = blockIdx.x * (L2_T / 64u) + (threadIdx.x >> 6);
    const uint32_t nc = ctl->ncand;
    // this wave's run of the list (everything below is wave-uniform but the loads)
    const uint32_t per = (nc + nw - 1u) / nw;
    const uint64_t kb = (uint64_t)w0 * per;
    const uint32_t k0 = kb < nc ? (uint32_t)kb : nc, k1 = kb + per < nc ? (uint32_t)(kb + per) : nc;
    uint32_t tile = ~0u, au = 0, an = 0, ab = 0; // the counts not yet added to `tile`
    for (uint32_t k = k0; k <= k1; ++k) {
        const uint32_t i = k < k1 ? cand[k] : 0u;
        const uint32_t ti = k < k1 ? i / L2_T : ~0u;
        if (ti != tile) { // (also behind the run's last candidate)
            if (lane == 0 && an)
                atomicAdd(reinterpret_cast<unsigned long long *>(&part[tile].units),
                          (unsigned long long)au | ((unsigned long long)an << 32));
            if (lane == 0 && ab) atomicAdd(&part[tile].bad, ab);
            tile = ti, au = an = ab = 0u;
        }
        if (k == k1) break;
        const uint8_t *fb = l2_frame(pkts, off, i, ul);
        const int32_t end = (int32_t)size[i];               // 14 + tl, inside the capture
        const uint32_t chunks = ((uint32_t)end + 15u) >> 4; // (>= 3: end >= 42)
        uint32_t acc = 0, c_le = 0;
        for (uint32_t c = 2u + lane; c < chunks; c += 64u) {
            uint4 q = chunk_below(ldg16<false>(fb + 16u * c), (int32_t)(16u * c), end);
            if (c == 2u) {
                q.x &= 0xFFFF0000u; // (bytes 32-33 are the header's)
                c_le = q.y & 0xFFFFu;
            }
            acc = add_halves(add_halves(add_halves(add_halves(acc, q.x), q.y), q.z), q.w);
        }
        const uint32_t T = gsum<64>(acc);
        c_le = __builtin_amdgcn_readfirstlane(c_le); // (lane 0 held piece 2)
        const bool good = fold16(T) == 0xFFFFu;
        if (good) {
            au += ((uint32_t)end + 63u) >> 6, an += 1u;
            if (lane == 0) size[i] = (uint32_t)end | ((~fold16(T - 0x0008u - c_le) & 0xFFFFu) << 16);
        } else {
            ab += 1u;
            if (lane == 0) size[i] = 0u, status[i] = RXG_L2_ECHO_BAD;
        }
    }
}

// base[j] = {units, answers} in tiles [0, j); totals = {ARP_REQ, ARP_REPLY,
// ECHO, ECHO_BAD, answers, units} when every answer fits cap_units, else the
// last two are 0 and the place stage's (ctl->cut).  One block.
__global__ __launch_bounds__(1024) void l2_scan_kernel(const l2_part *__restrict__ part, uint32_t tiles,
                                                       uint64_t cap_units, l2_ctl *__restrict__ ctl,
                                                       uint2 *__restrict__ base,
                                                       uint32_t *__restrict__ totals) {
    __shared__ uint32_t pu[1024], pa[1024];
    __shared__ uint32_t red[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (tiles + 1023u) / 1024u;
    const uint64_t b64 = (uint64_t)tid * per;
    const uint32_t b = b64 < tiles ? (uint32_t)b64 : tiles;
    const uint32_t e = b64 + per < tiles ? (uint32_t)(b64 + per) : tiles;
    if (tid < 4) red[tid] = 0u;
    uint32_t u = 0, a = 0, c[4] = {0, 0, 0, 0};
    for (uint32_t j = b; j < e; ++j) {
        const l2_part p = part[j];
        u += p.units, a += p.nans;
        c[0] += p.areq, c[1] += p.arep, c[2] += p.nans - p.areq, c[3] += p.bad;
    }
    pu[tid] = u, pa[tid] = a;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c[k]) atomicAdd(&red[k], c[k]);
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint32_t x = tid >= o ? pu[tid - o] : 0u, y = tid >= o ? pa[tid - o] : 0u;
        __syncthreads();
        pu[tid] += x, pa[tid] += y;
        __syncthreads();
    }
    uint32_t ru = pu[tid] - u, ra = pa[tid] - a;
    for (uint32_t j = b; j < e; ++j) {
        base[j] = make_uint2(ru, ra);
        ru += part[j].units, ra += part[j].nans;
    }
    if (tid < 4) totals[tid] = red[tid];
    if (tid == 1023) {
        const bool cut = (uint64_t)pu[1023] > cap_units;
        totals[4] = cut ? 0u : pa[1023];
        totals[5] = cut ? 0u : pu[1023];
        ctl->cut = cut ? 1u : 0u;
        ctl->ncand = 0u; // (for the next call on this workspace)
    }
}

__global__ __launch_bounds__(256) void l2_place_kernel(
    uint32_t n, const uint32_t *__restrict__ size, const l2_part *__restrict__ part,
    const uint2 *__restrict__ base, const l2_ctl *__restrict__ ctl, uint64_t cap_units,
    uint32_t *__restrict__ roff,
    uint16_t *__restrict__ rlen, uint32_t *__restrict__ rsrc, uint32_t *__restrict__ totals) {
    __shared__ uint32_t s_u[4], s_a[4];
    if (part[blockIdx.x].nans == 0u) return; // (block-uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * L2_T + tid;
    const uint32_t alen = i < n ? size[i] & 0xFFFFu : 0u;
    const uint32_t u = (alen + 63u) >> 6;
    // inclusive prefix of the units inside the wave
    uint32_t inc = u;
#pragma unroll
    for (uint32_t o = 1; o < 64u; o <<= 1) {
        const uint32_t x = __shfl_up(inc, o, 64);
        if (lane >= o) inc += x;
    }
    const uint64_t m = __ballot(alen != 0u);
    if (lane == 63) s_u[wv] = inc, s_a[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    const uint2 bs = base[blockIdx.x];
    uint32_t o64 = bs.x + inc - u, k = bs.y + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wv; ++w) o64 += s_u[w], k += s_a[w];
    // sizes are positive, so the answers that fit are a prefix of the burst
    const bool fits = alen != 0u && (uint64_t)o64 + u <= cap_units;
    if (fits) roff[k] = o64, rlen[k] = (uint16_t)alen, rsrc[k] = (uint32_t)i;
    if (!ctl->cut) return; // (the scan stage wrote the count and the span)
    const uint64_t fm = __ballot(fits);
    if (fm && lane == 63u - (uint32_t)__clzll(fm)) { // (the wave's last answer that fits)
        atomicMax(totals + 4, k + 1u);
        atomicMax(totals + 5, o64 + u);
    }
}

// local[j].mac as a little-endian integer (selects over the kernel argument:
// no indexed copy of it in scratch)
__device__ __forceinline__ uint64_t l2_mac(const rxg_l2_params &p, int j) {
    uint64_t m = 0;
#pragma unroll
    for (int k = 0; k < RXG_L2_MAX_LOCAL; ++k) {
        const uint8_t *b = p.local[k].mac;
        const uint64_t x = (uint64_t)pk4(b[0], b[1], b[2], b[3]) | ((uint64_t)pk4(b[4], b[5], 0, 0) << 32);
        if (k == j) m = x;
    }
    return m;
}
#define L2_MAC_BYTES(m)                                                                            \
    const uint32_t m0 = (uint32_t)(m) & 0xFFu, m1 = (uint32_t)((m) >> 8) & 0xFFu,                  \
                   m2 = (uint32_t)((m) >> 16) & 0xFFu, m3 = (uint32_t)((m) >> 24) & 0xFFu,         \
                   m4 = (uint32_t)((m) >> 32) & 0xFFu, m5 = (uint32_t)((m) >> 40) & 0xFFu

// the 16-B piece c (0..2) of an answer's first 48 bytes
__device__ __forceinline__ uint4 l2_arp_piece(const l2_head &h, uint64_t mac, uint32_t c) {
    L2_MAC_BYTES(mac);
    if (c == 0) // dst = sha (22-27), src = mac, 08 06, 00 01
        return make_uint4(hraw32(h, 22), pk4(hb(h, 26), hb(h, 27), m0, m1), pk4(m2, m3, m4, m5),
                          pk4(0x08, 0x06, 0x00, 0x01));
    if (c == 1) // 08 00 06 04, 00 02, sha = mac, spa = the request's tpa (38-41)
        return make_uint4(pk4(0x08, 0x00, 0x06, 0x04), pk4(0x00, 0x02, m0, m1), pk4(m2, m3, m4, m5),
                          hraw32(h, 38));
    // tha = the request's sha (22-27), tpa = its spa (28-31), six pad bytes
    return make_uint4(hraw32(h, 22), pk4(hb(h, 26), hb(h, 27), hb(h, 28), hb(h, 29)),
                      pk4(hb(h, 30), hb(h, 31), 0, 0), 0u);
}

__device__ __forceinline__ uint4 l2_echo_piece(const l2_head &h, uint64_t mac, uint32_t ck,
                                               uint32_t c) {
    L2_MAC_BYTES(mac);
    if (c == 0) // dst = the request's source (6-11), src = mac, 08 00, 45 00
        return make_uint4(hraw32(h, 6), pk4(hb(h, 10), hb(h, 11), m0, m1), pk4(m2, m3, m4, m5),
                          pk4(0x08, 0x00, 0x45, 0x00));
    if (c == 1) {
        // tl, id 0 | fragment 0 | ttl 64, proto 1, checksum | sip = the
        // request's dip (30-33) | dip = the request's sip (26-29), first half.
        // The header sum in big-endian words; 0x4500 makes it non-zero.
        const uint32_t s = 0x4500u + hbe16(h, 16) + 0x4001u + hbe16(h, 26) + hbe16(h, 28) +
                           hbe16(h, 30) + hbe16(h, 32);
        const uint32_t x = ~fold16(s) & 0xFFFFu;
        return make_uint4(pk4(hb(h, 16), hb(h, 17), 0, 0), pk4(0, 0, 64, 1),
                          pk4(x >> 8, x & 0xFFu, hb(h, 30), hb(h, 31)),
                          pk4(hb(h, 32), hb(h, 33), hb(h, 26), hb(h, 27)));
    }
    // dip second half, type 0 code 0 | checksum (ck: little-endian as stored),
    // then the request's bytes 38-47
    return make_uint4(pk4(hb(h, 28), hb(h, 29), 0, 0), pk4(ck & 0xFFu, ck >> 8, hb(h, 38), hb(h, 39)),
                      h.w[10], h.w[11]);
}

__global__ __launch_bounds__(256) void l2_emit_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off, uint32_t ul,
    const uint8_t *__restrict__ status, const uint32_t *__restrict__ size, const rxg_l2_params p,
    const uint32_t *__restrict__ roff, const uint16_t *__restrict__ rlen,
    const uint32_t *__restrict__ rsrc, const uint32_t *__restrict__ totals, uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nw = gridDim.x * (L2_T / 64u), w0 = blockIdx.x * (L2_T / 64u) + (threadIdx.x >> 6);
    const uint32_t na = totals[4];
    for (uint32_t k = w0; k < na; k += nw) { // (wave-uniform)
        const uint32_t i = rsrc[k];
        const int32_t alen = (int32_t)rlen[k];
        const uint8_t *fb = l2_frame(pkts, off, i, ul);
        uint4 *dst = reinterpret_cast<uint4 *>(out + ((uint64_t)roff[k] << 6));
        const uint32_t pieces = (((uint32_t)alen + 63u) >> 6) * 4u; // the whole slot
        const l2_head h = l2_load_head(fb); // (uniform addresses: one fetch per wave)
        const bool arp = status[i] == RXG_L2_ARP_REQ;
        const int j = l2_local(p, arp ? hraw32(h, 38) : hraw32(h, 30));
        const uint64_t mac = l2_mac(p, j); // (j >= 0: the judge stage matched it)
        const uint32_t ck = size[i] >> 16;
        for (uint32_t c = lane; c < pieces; c += 64u) {
            const int32_t s = (int32_t)(16u * c);
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (c < 3u) q = arp ? l2_arp_piece(h, mac, c) : l2_echo_piece(h, mac, ck, c);
            else if (s < alen) q = ldg16<false>(fb + s); // (alen <= the captured length)
            if (s < alen) q = chunk_below(q, s, alen);
            stg16(dst + c, q);
        }
    }
}

} // namespace

// [ctl: 16 B][part: 32 B per tile][base: uint2 per tile, padded to 16 B]
// [size: u32 per frame, padded to 16 B][cand: u32 per frame]
static size_t l2_tiles(uint32_t n) { return ((size_t)n + L2_T - 1) / L2_T; }
static size_t l2_part_off() { return 32; } // (l2_part is 32-B aligned)
static size_t l2_base_off(uint32_t n) { return l2_part_off() + l2_tiles(n) * sizeof(l2_part); }
static size_t l2_size_off(uint32_t n) {
    return l2_base_off(n) + ((l2_tiles(n) * sizeof(uint2) + 15) & ~(size_t)15);
}
static size_t l2_cand_off(uint32_t n) { return l2_size_off(n) + (((size_t)n * 4 + 15) & ~(size_t)15); }

size_t rx_l2_ws_bytes(uint32_t n) { return l2_cand_off(n) + (size_t)n * sizeof(uint32_t); }
// the bytes of a fresh workspace the first call needs zeroed (the caller does
// it when it allocates one)
size_t rx_l2_ws_ctl_bytes() { return sizeof(l2_ctl); }

// n != 0 (the caller zeroes the totals of an empty call)
hipError_t rx_l2_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                        uint32_t unit_log2, const uint4 *verd, const rxg_l2_params *p, uint8_t *status,
                        uint8_t *out, uint64_t cap_bytes, uint32_t *roff, uint16_t *rlen, uint32_t *rsrc,
                        uint32_t *totals, void *ws, hipStream_t s) {
    const uint32_t tiles = (uint32_t)l2_tiles(n);
    uint8_t *w = reinterpret_cast<uint8_t *>(ws);
    l2_ctl *ctl = reinterpret_cast<l2_ctl *>(w);
    l2_part *part = reinterpret_cast<l2_part *>(w + l2_part_off());
    uint2 *base = reinterpret_cast<uint2 *>(w + l2_base_off(n));
    uint32_t *size = reinterpret_cast<uint32_t *>(w + l2_size_off(n));
    uint32_t *cand = reinterpret_cast<uint32_t *>(w + l2_cand_off(n));
    // the wave-per-item stages: enough waves to fill the device, never more
    // than one per frame; the sum stage's waves take runs of the list
    const uint32_t q = (n + 3u) / 4u;
    const uint32_t sgrid = q < 1024u ? q : 1024u, egrid = q < 2048u ? q : 2048u;
    hipLaunchKernelGGL(l2_judge_kernel, dim3(tiles), dim3(L2_T), 0, s, pkts, off, len, n, unit_log2, verd,
                       *p, status, size, cand, ctl, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(l2_sum_kernel, dim3(sgrid), dim3(L2_T), 0, s, pkts, off, unit_log2, cand, ctl, status,
                       size, part);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(l2_scan_kernel, dim3(1), dim3(1024), 0, s, part, tiles, cap_bytes >> 6, ctl, base,
                       totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(l2_place_kernel, dim3(tiles), dim3(L2_T), 0, s, n, size, part, base, ctl,
                       cap_bytes >> 6, roff, rlen, rsrc, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(l2_emit_kernel, dim3(egrid), dim3(L2_T), 0, s, pkts, off, unit_log2, status, size,
                       *p, roff, rlen, rsrc, totals, out);
    return hipGetLastError();
}
