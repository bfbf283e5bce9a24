// rx_ddos.hip — K6: the reference's entropy flood detector over a burst
// (gfx950).  The reference runs it frame by frame in its I/O loop, before the
// burst goes into the protocol ring (ddos_detect, .vscode/test.c:2846-2891,
// called at :2992-2997): a popcount over the frame, a ring of the last 256
// frames' (set bits, total bits, entropy), and per frame the statistic
//   D = sum_window e(set_j, tot_j) - e(sum set_j, sum tot_j)
// compared with a threshold.  The rule, its quirks and the divergences from
// the reference are stated in include/rxgpu.h ("Entropy flood detector") and
// restated on the CPU in csrc/rx_ddos_host.cpp.  Three launches per burst:
//
//   bits    one u32 per frame, G lanes per frame reading 16-B chunks k, k+G,
//           ... (the frame-reading structure of tx_cksum_kernel), the tail
//           masked with chunk_below, the group sum over DPP;
//   window  one block per tile of RXG_DDOS_TILE frames plus a 256-frame halo
//           (255 for the first frame's window, one more for the alarm of the
//           frame before the tile); the halo before the burst's start comes
//           from the state's slots.  The window sums are a suffix of the
//           previous 256-aligned segment plus a prefix of the current one,
//           aligned to the GLOBAL frame index, from two segmented scans in
//           LDS: set, tot and the count of undefined frames as exact
//           integers, e in f64 with undefined frames as 0 (at most 256 terms
//           per frame, no differences of running sums).  A frame's result
//           depends only on its window, never on the tile or burst split;
//   finish  one block, ordered after the window pass's reads of the state:
//           the tiles' partial counts into the summary, the last
//           min(n, 256) frames into their slots, frames_seen and the flag.
#include <hip/hip_runtime.h>

#include <math.h>

#include "rx_common.h"
#include "rx_device.h"

namespace {

constexpr int DD_T = (int)RXG_DDOS_TILE;  // frames per tile
constexpr int DD_H = 256;                 // halo elements in front of a tile
constexpr int DD_L = DD_T + DD_H;         // LDS elements per tile
constexpr int DD_EPT = DD_L / 256;        // elements per thread
static_assert(DD_L % 256 == 0, "tile + halo must be a multiple of the block");
static_assert(RXG_DDOS_WINDOW == 256u, "slot arithmetic assumes a 256-frame window");

// what a tile hands to the finish step
struct dd_part {
    uint32_t alarms, first, rises, falls, undef, _r0, _r1, _r2;
};
// the burst's last frame (written by the lane that owns frame n - 1)
struct dd_last {
    double stat;
    uint32_t checked, alarm, set, tot;
    uint32_t _r0, _r1;
};

// a 16-B aligned chunk of zeros: the address of every load that lies wholly
// past its frame (a zero-length frame owns no byte of the buffer)
__device__ const uint4 dd_zero16 = {0u, 0u, 0u, 0u};

__device__ __forceinline__ uint32_t pop16(uint4 v) {
    return (uint32_t)__popcll(((uint64_t)v.y << 32) | v.x) +
           (uint32_t)__popcll(((uint64_t)v.w << 32) | v.z);
}

// The reference's ddos_entropy (test.c:2774-2780) in double, left to right as
// written, no contraction.  Called only for 0 < s < t.
__device__ __noinline__ double dd_entropy(uint32_t s, uint32_t t) {
#pragma clang fp contract(off)
    const double a = (double)s, b = (double)t;
    const double lb = log2(b);
    return (-a) * (log2(a) - lb) - (b - a) * (log2(b - a) - lb) + lb;
}

__device__ __forceinline__ bool dd_undef(uint32_t s, uint32_t t) { return s == 0u || s >= t; }

template <int G, int P>
__global__ __launch_bounds__(256) void ddos_bits_kernel(const uint8_t *__restrict__ pkts,
                                                        const uint32_t *__restrict__ off,
                                                        const uint16_t *__restrict__ len, uint32_t n,
                                                        uint32_t unit_log2,
                                                        uint32_t *__restrict__ bits) {
    constexpr uint32_t GPB = 256 / G;
    constexpr int32_t STEP = 16 * G;
    constexpr bool NT = G == 64; // (rx_device.h: nt pays for whole-wave 1-KiB accesses only)
    const uint32_t tid = threadIdx.x, gl = tid & (G - 1), grp = tid / G;
    const int32_t s0 = 16 * (int32_t)gl;
    const uint8_t *const zero = reinterpret_cast<const uint8_t *>(&dd_zero16);
    for (uint64_t tile = blockIdx.x; tile * GPB < n; tile += gridDim.x) {
        const uint64_t pos = tile * GPB + grp;
        const bool valid = pos < n;
        const uint64_t q0 = valid ? pos : 0;
        const uint8_t *fb = pkts + ((uint64_t)off[q0] << unit_log2);
        const int32_t cp = valid ? (int32_t)len[q0] : 0;
        // the first P passes in flight before any is consumed; a chunk that
        // starts at or past the frame's end is not read from the buffer
        uint4 c[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const int32_t s = s0 + q * STEP;
            c[q] = ldg16<NT>(s < cp ? fb + s : zero);
        }
        uint32_t acc = 0;
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const int32_t s = s0 + q * STEP;
            uint4 v = c[q];
            if (s + 16 > cp) v = chunk_below(v, s, cp); // bytes past len never count
            acc += pop16(v);
        }
        for (int32_t sb = P * STEP; sb < cp; sb += 4 * STEP) { // group-uniform
            uint4 r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t s = s0 + sb + u * STEP;
                r[u] = ldg16<NT>(s < cp ? fb + s : zero);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t s = s0 + sb + u * STEP;
                acc += pop16(chunk_below(r[u], s, cp));
            }
        }
        if constexpr (G > 1) acc = gsum<G>(acc);
        if (valid && gl == 0) bits[pos] = acc;
    }
}

// one Hillis-Steele step of both segmented scans (prefix p*, suffix q*) over
// the tile's elements; segments are the 256-aligned ranges of the global
// frame index (k = index inside the segment)
template <typename V>
__device__ __forceinline__ void dd_scan_read(const V *p, const V *q, int i, int k, int d, V &a, V &b) {
    a = (k >= d && i >= d) ? p[i - d] : V(0);
    b = (k + d <= 255 && i + d < DD_L) ? q[i + d] : V(0);
}

__global__ __launch_bounds__(256) void ddos_window_kernel(const uint32_t *__restrict__ bits,
                                                          const uint16_t *__restrict__ len, uint32_t n,
                                                          double thresh,
                                                          const rxg_ddos_state *__restrict__ st,
                                                          uint8_t *__restrict__ flag,
                                                          double *__restrict__ stat,
                                                          dd_part *__restrict__ part,
                                                          dd_last *__restrict__ last) {
    __shared__ uint32_t ps[DD_L], pt[DD_L], pu[DD_L], qs[DD_L], qt[DD_L], qu[DD_L];
    __shared__ double pe[DD_L], qe[DD_L];
    __shared__ uint32_t red[5];
    const int tid = (int)threadIdx.x;
    const uint64_t g0 = st->frames_seen;
    const uint32_t flag0 = st->flag ? 1u : 0u;
    // element i of the tile is burst frame jb + i, global frame g0 + jb + i
    const int64_t jb = (int64_t)blockIdx.x * DD_T - DD_H;
    if (tid < 5) red[tid] = tid == 1 ? 0xFFFFFFFFu : 0u;

#pragma unroll 1
    for (int r = 0; r < DD_EPT; ++r) {
        const int i = tid + 256 * r;
        const int64_t j = jb + i;
        uint32_t s = 0, t = 0;
        bool have = false;
        if (j >= 0) {
            if (j < (int64_t)n) s = bits[j], t = 8u * (uint32_t)len[j], have = true;
        } else if ((int64_t)g0 + j >= 0) { // a frame of an earlier burst: its slot
            const uint32_t slot = (uint32_t)(g0 + (uint64_t)j) & 255u;
            s = st->set[slot], t = st->tot[slot], have = true;
        }
        const bool ud = have && dd_undef(s, t);
        const double e = (have && !ud) ? dd_entropy(s, t) : 0.0;
        ps[i] = qs[i] = s;
        pt[i] = qt[i] = t;
        pu[i] = qu[i] = ud ? 1u : 0u;
        pe[i] = qe[i] = e;
    }
    __syncthreads();

    const int k0 = (int)((uint32_t)(g0 + (uint64_t)(jb + tid)) & 255u); // 256 * r keeps it
#pragma unroll 1
    for (int d = 1; d < 256; d <<= 1) {
        uint32_t as[DD_EPT], at[DD_EPT], au[DD_EPT], bs[DD_EPT], bt[DD_EPT], bu[DD_EPT];
        double ae[DD_EPT], be[DD_EPT];
#pragma unroll
        for (int r = 0; r < DD_EPT; ++r) {
            const int i = tid + 256 * r;
            dd_scan_read(ps, qs, i, k0, d, as[r], bs[r]);
            dd_scan_read(pt, qt, i, k0, d, at[r], bt[r]);
            dd_scan_read(pu, qu, i, k0, d, au[r], bu[r]);
            dd_scan_read(pe, qe, i, k0, d, ae[r], be[r]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < DD_EPT; ++r) {
            const int i = tid + 256 * r;
            ps[i] += as[r], qs[i] += bs[r];
            pt[i] += at[r], qt[i] += bt[r];
            pu[i] += au[r], qu[i] += bu[r];
            pe[i] += ae[r], qe[i] += be[r];
        }
        __syncthreads();
    }

    // the window of element i (>= 255): slots 0..k of its own segment (the
    // prefix at i) and slots k+1..255 of the one before (the suffix at
    // i - 255), added in the reference's slot order: prefix first
    uint32_t fl[DD_EPT], al[DD_EPT];
#pragma unroll
    for (int r = 0; r < DD_EPT; ++r) {
        const int i = tid + 256 * r;
        const int64_t j = jb + i;
        fl[r] = 0u, al[r] = flag0;
        // (of the halo only element 255, the frame before the tile, is evaluated)
        if (i < DD_H - 1 || j < 0 || j >= (int64_t)n) continue;
        const uint64_t g = g0 + (uint64_t)j;
        uint32_t S = ps[i], T = pt[i], U = pu[i];
        double E = pe[i];
        if (k0 < 255) S += qs[i - 255], T += qt[i - 255], U += qu[i - 255], E += qe[i - 255];
        uint32_t f = RXG_DDOS_WARMUP, a = flag0;
        double D = __builtin_nan("");
        const bool checked = g >= 256u;
        if (checked) {
            f = 0u, a = 0u;
            if (U != 0u) {
                f = RXG_DDOS_UNDEF;
            } else {
                D = E - dd_entropy(S, T);
                if (thresh < D) f = RXG_DDOS_ALARM, a = 1u;
            }
        }
        fl[r] = f, al[r] = a;
        if (i >= DD_H) {
            if (stat) stat[j] = D;
            if (j == (int64_t)n - 1) {
                last->stat = D;
                last->checked = checked ? 1u : 0u;
                last->alarm = a;
                last->set = checked ? S : 0u;
                last->tot = checked ? T : 0u;
            }
        }
    }
    // the alarm state after each frame, for the frame behind it (ps is free:
    // every read of it above was of the thread's own elements or of qs)
    __syncthreads();
#pragma unroll
    for (int r = 0; r < DD_EPT; ++r) ps[tid + 256 * r] = al[r];
    __syncthreads();
    uint32_t n_al = 0, n_ri = 0, n_fa = 0, n_ud = 0, first = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 1; r < DD_EPT; ++r) {
        const int i = tid + 256 * r;
        const int64_t j = jb + i;
        if (j >= (int64_t)n) continue; // (j >= 0: i >= 256)
        const uint32_t prev = j == 0 ? flag0 : ps[i - 1];
        uint32_t f = fl[r];
        if (!(f & RXG_DDOS_WARMUP)) {
            if (al[r] && !prev) f |= RXG_DDOS_RISE, ++n_ri;
            if (!al[r] && prev) f |= RXG_DDOS_FALL, ++n_fa;
        }
        if (f & RXG_DDOS_ALARM) ++n_al, first = first < (uint32_t)j ? first : (uint32_t)j;
        if (f & RXG_DDOS_UNDEF) ++n_ud;
        if (flag) flag[j] = (uint8_t)f;
    }
    if (n_al) atomicAdd(&red[0], n_al), atomicMin(&red[1], first);
    if (n_ri) atomicAdd(&red[2], n_ri);
    if (n_fa) atomicAdd(&red[3], n_fa);
    if (n_ud) atomicAdd(&red[4], n_ud);
    __syncthreads();
    if (tid == 0) {
        dd_part p{};
        p.alarms = red[0], p.first = red[1], p.rises = red[2], p.falls = red[3], p.undef = red[4];
        part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(256) void ddos_finish_kernel(const uint32_t *__restrict__ bits,
                                                          const uint16_t *__restrict__ len, uint32_t n,
                                                          uint32_t tiles, const dd_part *__restrict__ part,
                                                          const dd_last *__restrict__ last,
                                                          rxg_ddos_state *__restrict__ st,
                                                          rxg_ddos_summary *__restrict__ sum) {
    __shared__ uint32_t red[5];
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = st->frames_seen;
    const uint32_t flag0 = st->flag ? 1u : 0u;
    if (tid < 5) red[tid] = tid == 1 ? 0xFFFFFFFFu : 0u;
    __syncthreads(); // (every thread has read the state before it changes)
    uint32_t a = 0, f = 0xFFFFFFFFu, ri = 0, fa = 0, ud = 0;
    for (uint32_t t = tid; t < tiles; t += 256u) {
        const dd_part p = part[t];
        a += p.alarms, ri += p.rises, fa += p.falls, ud += p.undef;
        f = f < p.first ? f : p.first;
    }
    if (a) atomicAdd(&red[0], a), atomicMin(&red[1], f);
    if (ri) atomicAdd(&red[2], ri);
    if (fa) atomicAdd(&red[3], fa);
    if (ud) atomicAdd(&red[4], ud);
    if (tid < n) { // the last min(n, 256) frames: distinct slots
        const uint32_t j = n - 1u - tid;
        const uint32_t slot = (uint32_t)(g0 + j) & 255u;
        st->set[slot] = bits[j];
        st->tot[slot] = 8u * (uint32_t)len[j];
    }
    __syncthreads();
    if (tid != 0) return;
    const bool checked = n != 0u && last->checked != 0u;
    const uint32_t flag1 = checked ? last->alarm : flag0;
    st->frames_seen = g0 + n;
    st->flag = flag1;
    rxg_ddos_summary s{};
    s.frames_seen = g0 + n;
    s.last_stat = checked ? last->stat : __builtin_nan("");
    s.alarm_frames = red[0];
    s.first_alarm = red[1];
    s.rises = red[2];
    s.falls = red[3];
    s.undef_frames = red[4];
    s.flag = flag1;
    s.last_set = checked ? last->set : 0u;
    s.last_tot = checked ? last->tot : 0u;
    *sum = s;
}

template <int G, int P>
hipError_t launch_bits(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                       uint32_t unit_log2, uint32_t *bits, hipStream_t s) {
    constexpr uint32_t GPB = 256 / G;
    int cu = 0, occ = 0;
    hipError_t e = rx_occupancy(reinterpret_cast<const void *>(ddos_bits_kernel<G, P>), 256, 0, &cu, &occ);
    if (e != hipSuccess) return e;
    const uint64_t tiles = ((uint64_t)n + GPB - 1) / GPB;
    uint64_t blocks = (uint64_t)cu * (uint64_t)occ;
    if (blocks > tiles) blocks = tiles;
    hipLaunchKernelGGL((ddos_bits_kernel<G, P>), dim3((uint32_t)blocks), dim3(256), 0, s, pkts, off, len,
                       n, unit_log2, bits);
    return hipGetLastError();
}

constexpr size_t DD_WS_HEAD = 64; // dd_last, padded

} // namespace

// lanes per frame compiled in (rxg_tune_ddos)
bool rx_ddos_has_g(uint32_t g) { return g == 1u || g == 8u || g == 64u; }

uint32_t rx_ddos_auto_g(uint32_t len_hint) {
    if (len_hint == 0) len_hint = 1518;
    return len_hint <= 128 ? 1u : (len_hint <= 2048 ? 8u : 64u);
}

// [dd_last][dd_part per tile][bits, when the caller wants none]
size_t rx_ddos_ws_bytes(uint32_t n, bool own_bits) {
    const size_t tiles = ((size_t)n + RXG_DDOS_TILE - 1) / RXG_DDOS_TILE;
    return DD_WS_HEAD + tiles * sizeof(dd_part) + (own_bits ? (size_t)n * sizeof(uint32_t) : 0);
}

// the bits pass alone (g: lanes per frame, one of rx_ddos_has_g)
hipError_t rx_ddos_bits_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                               uint32_t n, uint32_t unit_log2, uint32_t g, uint32_t *bits,
                               hipStream_t s) {
    if (n == 0) return hipSuccess;
    switch (g) {
    case 1: return launch_bits<1, 4>(pkts, off, len, n, unit_log2, bits, s);
    case 8: return launch_bits<8, 12>(pkts, off, len, n, unit_log2, bits, s);
    case 64: return launch_bits<64, 4>(pkts, off, len, n, unit_log2, bits, s);
    default: return hipErrorInvalidValue;
    }
}

// the window pass and the finish step on bits already computed
hipError_t rx_ddos_window_launch(const uint32_t *bits, const uint16_t *len, uint32_t n, double thresh,
                                 rxg_ddos_state *st, uint8_t *flag, double *stat,
                                 rxg_ddos_summary *sum, void *ws, hipStream_t s) {
    const uint32_t tiles = (uint32_t)(((uint64_t)n + RXG_DDOS_TILE - 1) / RXG_DDOS_TILE);
    dd_last *last = reinterpret_cast<dd_last *>(ws);
    dd_part *part = reinterpret_cast<dd_part *>(reinterpret_cast<uint8_t *>(ws) + DD_WS_HEAD);
    if (tiles) {
        hipLaunchKernelGGL(ddos_window_kernel, dim3(tiles), dim3(256), 0, s, bits, len, n, thresh, st,
                           flag, stat, part, last);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ddos_finish_kernel, dim3(1), dim3(256), 0, s, bits, len, n, tiles, part, last, st,
                       sum);
    return hipGetLastError();
}

hipError_t rx_ddos_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                          uint32_t unit_log2, uint32_t g, double thresh, rxg_ddos_state *st,
                          uint32_t *bits, uint8_t *flag, double *stat, rxg_ddos_summary *sum, void *ws,
                          hipStream_t s) {
    if (!bits) {
        const size_t tiles = ((size_t)n + RXG_DDOS_TILE - 1) / RXG_DDOS_TILE;
        bits = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(ws) + DD_WS_HEAD +
                                            tiles * sizeof(dd_part));
    }
    hipError_t e = rx_ddos_bits_launch(pkts, off, len, n, unit_log2, g, bits, s);
    if (e != hipSuccess) return e;
    return rx_ddos_window_launch(bits, len, n, thresh, st, flag, stat, sum, ws, s);
}
