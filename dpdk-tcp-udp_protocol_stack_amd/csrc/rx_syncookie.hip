// rx_syncookie.hip — K7: stateless SYN cookies over a classified burst
// (gfx950).  A frame that K1 matched to a listening control block is judged
// without host state: a SYN is answered with a SYN-ACK descriptor (rxg_txd,
// the input of K5) whose sequence number is a keyed hash of the 4-tuple, the
// client's sequence number and a coarse time counter; an ACK is checked
// against the same hash.  The rule is stated in include/rxgpu.h ("SYN
// cookies") and restated on the CPU in csrc/rx_syncookie_host.cpp.  Three
// launches per burst, one lane per frame, tiles of CK_T frames:
//
//   judge   the verdict (one 16-B load per lane, coalesced), the listener
//           bit, and for candidates only the frame's first 48 bytes (three
//           16-B loads from the 16-B aligned frame start; nothing of the rule
//           lies past byte 47, so nothing past it is read) and one SipHash-2-4
//           of 24 bytes in 64-bit integers: an ACK names its own counter in
//           the cookie's top byte, so it costs one hash, not max_age + 1.
//           Status bytes go through LDS and leave as dwords (a wave's 64
//           bytes: one line); a SYN's cookie is kept for the emit pass; the
//           tile's three counts go to the workspace;
//   scan    one block: exclusive prefix of the tiles' SYN counts and the
//           totals (the layout pass of rxg_gather_dev / K5);
//   emit    the k-th SYN of the burst writes txd[k] as three 16-B stores; a
//           tile without a SYN leaves at once.
#include <hip/hip_runtime.h>

#include "rx_common.h"
#include "rx_device.h"
#include "rx_siphash.h"

namespace {

constexpr uint32_t CK_T = 256; // frames per tile = threads per block

struct ck_head {
    uint32_t m0, m1, m2; // descriptor bytes 0-11: frame bytes 6-11, then 0-5
    uint32_t sip, dip, sport, dport, seq, ack, fl;
};

// the fields of the rule from frame bytes 0-47
__device__ __forceinline__ ck_head ck_parse(uint4 c0, uint4 c1, uint4 c2) {
    ck_head h;
    h.m0 = (c0.y >> 16) | (c0.z << 16);
    h.m1 = (c0.z >> 16) | (c0.x << 16);
    h.m2 = (c0.x >> 16) | (c0.y << 16);
    h.sip = (c1.z >> 16) | (c1.w << 16);
    h.dip = (c1.w >> 16) | (c2.x << 16);
    h.sport = c2.x >> 16;
    h.dport = c2.y & 0xFFFFu;
    h.seq = __builtin_bswap32((c2.y >> 16) | (c2.z << 16));
    h.ack = __builtin_bswap32((c2.z >> 16) | (c2.w << 16));
    h.fl = c2.w >> 24;
    return h;
}

__device__ __forceinline__ const uint8_t *ck_frame(const uint8_t *pkts, const uint32_t *off, uint64_t i,
                                                   uint32_t ul) {
    return pkts + ((uint64_t)off[i] << ul);
}

__global__ __launch_bounds__(256) void ck_judge_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off, const uint16_t *__restrict__ len,
    uint32_t n, uint32_t ul, const uint4 *__restrict__ verd, const uint32_t *__restrict__ lmask,
    uint32_t id_space, uint64_t k0, uint64_t k1, uint32_t t, uint32_t max_age,
    uint8_t *__restrict__ status, uint32_t *__restrict__ cookie, uint4 *__restrict__ part) {
    __shared__ alignas(16) uint8_t s_st[CK_T];
    __shared__ uint32_t s_cnt[4][3];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * CK_T, i = i0 + tid;
    uint32_t st = 0;
    if (i < n) {
        const uint4 v = ld_slot(verd + i); // {flow_id, off|len, cksum|cls|rc, ..}
        const bool tcp_ok = ((v.z >> 16) & 0xFFu) == (uint32_t)RXG_CLS_TCP && (v.z >> 24) == 0u;
        bool cand = tcp_ok && v.x < id_space && len[i] >= 54u;
        if (cand) cand = (lmask[v.x >> 5] >> (v.x & 31u)) & 1u;
        if (cand) {
            const uint8_t *fb = ck_frame(pkts, off, i, ul);
            const uint4 c0 = ldg16<false>(fb), c1 = ldg16<false>(fb + 16), c2 = ldg16<false>(fb + 32);
            const ck_head h = ck_parse(c0, c1, c2);
            if ((h.fl & 0x17u) == 0x02u) {
                st = RXG_CK_SYN;
                cookie[i] = rx_cookie(k0, k1, h.sip, h.dip, h.sport, h.dport, h.seq, t);
            } else if ((h.fl & 0x16u) == 0x10u) {
                const uint32_t c = h.ack - 1u, age = ((t & 0xFFu) - (c >> 24)) & 0xFFu;
                st = RXG_CK_ACK_BAD;
                if (age <= max_age &&
                    rx_cookie(k0, k1, h.sip, h.dip, h.sport, h.dport, h.seq - 1u, t - age) == c)
                    st = RXG_CK_ACK_OK;
            }
        }
    }
    const uint32_t c1 = (uint32_t)__popcll(__ballot(st == RXG_CK_SYN));
    const uint32_t c2 = (uint32_t)__popcll(__ballot(st == RXG_CK_ACK_OK));
    const uint32_t c3 = (uint32_t)__popcll(__ballot(st == RXG_CK_ACK_BAD));
    if (lane == 0) s_cnt[wv][0] = c1, s_cnt[wv][1] = c2, s_cnt[wv][2] = c3;
    s_st[tid] = (uint8_t)st;
    __syncthreads();
    if (tid == 0)
        part[blockIdx.x] = make_uint4(s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0],
                                      s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1],
                                      s_cnt[0][2] + s_cnt[1][2] + s_cnt[2][2] + s_cnt[3][2], 0u);
    // four status bytes per lane of the first wave: a dword store where the
    // four lie inside the burst and the address allows, bytes at the edge
    if (tid < CK_T / 4) {
        const uint64_t b = i0 + 4u * tid;
        uint8_t *dst = status + b;
        if (b + 4 <= n && ((uintptr_t)dst & 3u) == 0) {
            *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(&s_st[4u * tid]);
        } else {
            for (uint32_t k = 0; k < 4u && b + k < n; ++k) dst[k] = s_st[4u * tid + k];
        }
    }
}

// base[j] = SYNs in tiles [0, j); totals = {SYN, ACK_OK, ACK_BAD, 0}.  One block.
__global__ __launch_bounds__(1024) void ck_scan_kernel(const uint4 *__restrict__ part, uint32_t tiles,
                                                       uint32_t *__restrict__ base,
                                                       uint32_t *__restrict__ totals) {
    __shared__ uint32_t ps[1024];
    __shared__ uint32_t red[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (tiles + 1023u) / 1024u;
    const uint64_t b64 = (uint64_t)tid * per;
    const uint32_t b = b64 < tiles ? (uint32_t)b64 : tiles;
    const uint32_t e = b64 + per < tiles ? (uint32_t)(b64 + per) : tiles;
    if (tid < 2) red[tid] = 0u;
    uint32_t s = 0, ok = 0, bad = 0;
    for (uint32_t j = b; j < e; ++j) {
        const uint4 p = part[j];
        s += p.x, ok += p.y, bad += p.z;
    }
    ps[tid] = s;
    __syncthreads();
    if (ok) atomicAdd(&red[0], ok);
    if (bad) atomicAdd(&red[1], bad);
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint32_t x = tid >= o ? ps[tid - o] : 0u;
        __syncthreads();
        ps[tid] += x;
        __syncthreads();
    }
    uint32_t run = ps[tid] - s;
    for (uint32_t j = b; j < e; ++j) {
        base[j] = run;
        run += part[j].x;
    }
    if (tid == 1023) {
        totals[0] = ps[1023];
        totals[1] = red[0];
        totals[2] = red[1];
        totals[3] = 0u;
    }
}

__global__ __launch_bounds__(256) void ck_emit_kernel(
    const uint8_t *__restrict__ pkts, const uint32_t *__restrict__ off, uint32_t n, uint32_t ul,
    const uint8_t *__restrict__ status, const uint32_t *__restrict__ cookie,
    const uint4 *__restrict__ part, const uint32_t *__restrict__ base, uint32_t window,
    uint4 *__restrict__ txd) {
    __shared__ uint32_t s_w[4];
    if (part[blockIdx.x].x == 0u) return; // (block-uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * CK_T + tid;
    const bool syn = i < n && status[i] == RXG_CK_SYN;
    const uint64_t m = __ballot(syn);
    if (lane == 0) s_w[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!syn) return;
    uint32_t k = base[blockIdx.x] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wv; ++w) k += s_w[w];
    const uint8_t *fb = ck_frame(pkts, off, i, ul);
    const uint4 c0 = ldg16<false>(fb), c1 = ldg16<false>(fb + 16), c2 = ldg16<false>(fb + 32);
    const ck_head h = ck_parse(c0, c1, c2);
    uint4 *d = txd + 3ull * k;
    // @0 macs swapped, @12 sip = the frame's dip; @16 dip, @20 ports swapped,
    // @24 seq = cookie, @28 ack; @32 window | urp, @36 0x50 | 0x12 | optlen 0 |
    // RXG_TXD_TCP, @40 no payload
    d[0] = make_uint4(h.m0, h.m1, h.m2, h.dip);
    d[1] = make_uint4(h.sip, h.dport | (h.sport << 16), cookie[i], h.seq + 1u);
    d[2] = make_uint4(window & 0xFFFFu, 0x50u | (0x12u << 8) | ((uint32_t)RXG_TXD_TCP << 24), 0u, 0u);
}

} // namespace

// [part: uint4 per tile][base: u32 per tile, padded to 16 B][cookie: u32 per frame]
static size_t ck_tiles(uint32_t n) { return ((size_t)n + CK_T - 1) / CK_T; }
static size_t ck_base_off(uint32_t n) { return ck_tiles(n) * sizeof(uint4); }
static size_t ck_cookie_off(uint32_t n) {
    return ck_base_off(n) + ((ck_tiles(n) * sizeof(uint32_t) + 15) & ~(size_t)15);
}

size_t rx_syncookie_ws_bytes(uint32_t n) { return ck_cookie_off(n) + (size_t)n * sizeof(uint32_t); }

// n != 0 and id_space != 0 (the caller zeroes the outputs of an empty call)
hipError_t rx_syncookie_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                               uint32_t unit_log2, const uint4 *verd, const uint32_t *lmask,
                               uint32_t id_space, const rxg_ck_params *p, uint8_t *status, rxg_txd *txd,
                               uint32_t *totals, void *ws, hipStream_t s) {
    const uint32_t tiles = (uint32_t)ck_tiles(n);
    uint8_t *w = reinterpret_cast<uint8_t *>(ws);
    uint4 *part = reinterpret_cast<uint4 *>(w);
    uint32_t *base = reinterpret_cast<uint32_t *>(w + ck_base_off(n));
    uint32_t *cookie = reinterpret_cast<uint32_t *>(w + ck_cookie_off(n));
    hipLaunchKernelGGL(ck_judge_kernel, dim3(tiles), dim3(CK_T), 0, s, pkts, off, len, n, unit_log2, verd,
                       lmask, id_space, p->k0, p->k1, p->t, p->max_age, status, cookie, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ck_scan_kernel, dim3(1), dim3(1024), 0, s, part, tiles, base, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ck_emit_kernel, dim3(tiles), dim3(CK_T), 0, s, pkts, off, n, unit_log2, status,
                       cookie, part, base, (uint32_t)p->window, reinterpret_cast<uint4 *>(txd));
    return hipGetLastError();
}
