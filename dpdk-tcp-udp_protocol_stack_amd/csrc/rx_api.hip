// rx_api.hip — host side of librxgpu: context, flow-table build/upload, the
// burst entry points of include/rxgpu.h.  Device work is in rx_classify.hip;
// there is no CPU classification path in this library: every verdict comes
// from the gfx950 kernel, and a missing/failed device is an error.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "rx_common.h"
#include "rx_flows.h"

void rx_pick_variant(uint32_t len_hint, uint32_t *g, uint32_t *p, uint32_t *fpg, uint32_t *pipe,
                     bool v8 = false);
bool rx_variant_exists(uint32_t g, uint32_t p, uint32_t fpg, uint32_t pipe);
const char *rx_variant_kernel(uint32_t g, uint32_t pipe);
hipError_t rx_classify_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                              uint32_t n, uint32_t unit_log2, uint32_t g, uint32_t p, uint32_t fpg,
                              uint32_t pipe, const rx_ft_dev &ft, uint4 *out,
                              unsigned long long *counts, hipStream_t s, uint32_t *ws,
                              uint32_t phase, uint32_t buf, uint32_t nbuf);
// the same kernels writing 8-B verdicts (rx_classify.hip built with RX_V8=1)
hipError_t rx_classify_launch8(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                               uint32_t n, uint32_t unit_log2, uint32_t g, uint32_t p, uint32_t fpg,
                               uint32_t pipe, const rx_ft_dev &ft, uint4 *out,
                               unsigned long long *counts, hipStream_t s, uint32_t *ws,
                               uint32_t phase, uint32_t buf, uint32_t nbuf);
size_t rx_classify_ws_bytes(uint32_t n, uint32_t g, uint32_t pipe, const rx_ft_dev &ft,
                            bool counts, uint32_t nbuf);
bool rx_count_uses_slabs(const rx_ft_dev &ft, bool counts);
hipError_t tx_cksum_launch(uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                           uint32_t unit_log2, uint32_t len_hint, uint32_t variant,
                           uint32_t bpc_cap, hipStream_t s);
uint32_t tx_num_variants();
hipError_t tx_encode_launch(const void *txd, uint32_t n, const uint8_t *pay, uint8_t *pkts,
                            uint64_t cap, uint32_t slot, uint32_t *off, uint16_t *len,
                            uint32_t len_hint, uint32_t flags, uint32_t *totals, void *ws,
                            uint32_t variant, uint32_t bpc_cap, hipStream_t s);
uint32_t txe_num_variants();
size_t txe_ws_bytes(uint32_t n);
hipError_t tx_encode_tso_launch(const void *txd, uint32_t n, const uint8_t *pay, uint32_t mss,
                                uint8_t *pkts, uint64_t cap, uint32_t slot, uint32_t *off,
                                uint16_t *len, uint32_t out_cap, uint32_t *first, uint32_t *nseg,
                                uint32_t len_hint, uint32_t flags, uint32_t *totals, void *ws,
                                uint32_t variant, uint32_t bpc_cap, hipStream_t s);
size_t txe_tso_ws_bytes(uint32_t n, uint32_t out_cap);
hipError_t tx_encode_frag_launch(const void *txd, uint32_t n, const uint8_t *pay, uint32_t mss,
                                 uint32_t mtu, uint8_t *pkts, uint64_t cap, uint32_t slot,
                                 uint32_t *off, uint16_t *len, uint32_t out_cap, uint32_t *first,
                                 uint32_t *nseg, uint32_t len_hint, uint32_t flags, uint32_t *totals,
                                 void *ws, uint32_t variant, uint32_t bpc_cap, hipStream_t s);
size_t txe_frag_ws_bytes(uint32_t n, uint32_t out_cap);
size_t rx_split_ws_bytes(uint32_t n, uint32_t nsh);
hipError_t rx_split_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                           uint32_t n, uint32_t unit_log2, uint32_t nsh, uint32_t *first,
                           uint32_t *perm, void *ws, hipStream_t s);
size_t rx_gather_ws_bytes(uint32_t count);
hipError_t rx_gather_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                            uint32_t unit_log2, const uint32_t *idx, uint32_t count, uint8_t *dst,
                            uint64_t cap, uint32_t *dst_off, uint16_t *dst_len, void *ws,
                            hipStream_t s);
int rx_group_allreduce_u64(rxg_group *g, void *d, uint32_t n, hipStream_t s);
size_t rx_segsort_ws_bytes(uint32_t n);
hipError_t rx_ingest_launch(const unsigned long long *src, const uint32_t *off, const uint16_t *len,
                            uint32_t n, uint8_t *dst, hipStream_t s);
hipError_t rx_segsort_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                             uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nt,
                             rxg_segment *seg, uint8_t *payload, uint64_t cap, uint32_t *totals,
                             void *ws, hipStream_t s);
size_t rx_gro_ws_bytes(uint32_t n);
hipError_t rx_gro_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                         uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t W,
                         rxg_segment *seg, rxg_tcp_run *run, uint8_t *payload, uint64_t cap,
                         uint32_t *totals, void *ws, hipStream_t s);
size_t rx_order_ws_bytes(uint32_t n);
hipError_t rx_order_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                           uint32_t unit_log2, const uint4 *verd, uint32_t nt, uint32_t W,
                           rxg_segment *seg, rxg_tcp_run *run, uint8_t *payload, uint64_t cap,
                           uint32_t *totals, void *ws, hipStream_t s);
bool rx_ddos_has_g(uint32_t g);
uint32_t rx_ddos_auto_g(uint32_t len_hint);
size_t rx_ddos_ws_bytes(uint32_t n, bool own_bits);
hipError_t rx_ddos_bits_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                               uint32_t n, uint32_t unit_log2, uint32_t g, uint32_t *bits,
                               hipStream_t s);
hipError_t rx_ddos_window_launch(const uint32_t *bits, const uint16_t *len, uint32_t n, double thresh,
                                 rxg_ddos_state *st, uint8_t *flag, double *stat,
                                 rxg_ddos_summary *sum, void *ws, hipStream_t s);
hipError_t rx_ddos_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                          uint32_t unit_log2, uint32_t g, double thresh, rxg_ddos_state *st,
                          uint32_t *bits, uint8_t *flag, double *stat, rxg_ddos_summary *sum, void *ws,
                          hipStream_t s);
size_t rx_assemble_ws_bytes(uint32_t n);
hipError_t rx_assemble_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                              uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nt,
                              rxg_segment *seg, rxg_tcp_stream *stream, uint8_t *payload,
                              uint64_t cap, uint32_t *totals, void *ws, hipStream_t s);
size_t rx_l2_ws_bytes(uint32_t n);
size_t rx_l2_ws_ctl_bytes();
hipError_t rx_l2_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                        uint32_t unit_log2, const uint4 *verd, const rxg_l2_params *p, uint8_t *status,
                        uint8_t *out, uint64_t cap_bytes, uint32_t *roff, uint16_t *rlen, uint32_t *rsrc,
                        uint32_t *totals, void *ws, hipStream_t s);
size_t rx_syncookie_ws_bytes(uint32_t n);
hipError_t rx_syncookie_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len, uint32_t n,
                               uint32_t unit_log2, const uint4 *verd, const uint32_t *lmask,
                               uint32_t id_space, const rxg_ck_params *p, uint8_t *status, rxg_txd *txd,
                               uint32_t *totals, void *ws, hipStream_t s);
size_t rx_compact_ws_bytes(uint32_t n, uint32_t nflows);
hipError_t rx_compact_launch(const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                             uint32_t n, uint32_t unit_log2, const uint4 *verd, uint32_t nflows,
                             rxg_dgram *dg, uint32_t *first, uint8_t *payload, uint64_t cap,
                             uint32_t *totals, void *ws, hipStream_t s);

static thread_local std::string g_last_hip;

int rx_set_hip_error(hipError_t e) {
    if (e == hipSuccess) return RXG_OK;
    g_last_hip = std::string(hipGetErrorName(e)) + ": " + hipGetErrorString(e);
    return RXG_EHIP;
}

void rx_set_last_error(const std::string &msg) { g_last_hip = msg; }

hipError_t rx_occupancy(const void *fn, uint32_t threads, size_t lds, int *cu, int *occ) {
    struct entry {
        int dev;
        const void *fn;
        uint32_t threads;
        size_t lds;
        int cu, occ;
    };
    static thread_local std::vector<entry> cache;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    for (const entry &x : cache)
        if (x.dev == dev && x.fn == fn && x.threads == threads && x.lds == lds) {
            *cu = x.cu;
            *occ = x.occ;
            return hipSuccess;
        }
    entry x{dev, fn, threads, lds, 0, 0};
    if ((e = hipDeviceGetAttribute(&x.cu, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess)
        return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&x.occ, fn, (int)threads, lds)) !=
        hipSuccess)
        return e;
    if (x.occ < 1) x.occ = 1;
    cache.push_back(x);
    *cu = x.cu;
    *occ = x.occ;
    return hipSuccess;
}

#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return rx_set_hip_error(e_);                                         \
    } while (0)

// one incremental table write (rxg_flows_commit): rx_delta_kernel stores v
// at element idx of table `which`
// (RX_D_CZERO: count index idx of a removed block, zeroed in both of the
// context's count vectors before its id can name a new block)
enum { RX_D_UDP = 0, RX_D_TCP = 1, RX_D_LISTEN = 2, RX_D_PORT = 3, RX_D_UDPC = 4, RX_D_UDPW = 5,
       RX_D_CZERO = 6 };
struct rx_delta {
    uint32_t which, idx, _r0, _r1;
    uint4 v;
};
#define RX_DELTA_CAP 65536u // records per commit; more: whole arrays are uploaded
#define RX_DELTA_ROOM (RX_DELTA_CAP + 2048u) // staging records (the small tables ride on top)

__global__ __launch_bounds__(256) void rx_delta_kernel(const rx_delta *__restrict__ d, uint32_t n,
                                                       uint4 *udp, uint4 *tcp, uint32_t *listen,
                                                       uint32_t *port, uint4 *udpc, uint4 *udpw,
                                                       unsigned long long *cnt,
                                                       unsigned long long *cnt_base) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const rx_delta r = d[i];
    switch (r.which) {
    case RX_D_UDP: udp[r.idx] = r.v; break;
    case RX_D_TCP: tcp[r.idx] = r.v; break;
    case RX_D_LISTEN: listen[r.idx] = r.v.x; break;
    case RX_D_PORT: port[r.idx] = r.v.x; break;
    case RX_D_UDPC: udpc[r.idx] = r.v; break;
    case RX_D_CZERO: cnt[r.idx] = 0ull, cnt_base[r.idx] = 0ull; break;
    default: udpw[r.idx] = r.v; break;
    }
}

// fold of two u64 count vectors: base += delta, delta = 0 (the all-reduced
// increment of rxg_ctx_counts_allreduce joins the running total)
__global__ __launch_bounds__(256) void rx_counts_fold_kernel(unsigned long long *base,
                                                             unsigned long long *delta, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    base[i] += delta[i];
    delta[i] = 0;
}

// a stream bursts of this context ran on, and the event recorded after its
// last burst: table writes wait on it, so they never overtake a burst still
// reading the tables (a per-context wait, never a device-wide one)
struct rx_track {
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    uint64_t commit_seen = 0; // last table commit this stream is ordered after
    uint64_t last_use = 0;
    bool used = false;
};
#define RX_TRACK 4

// The form of K4 (rx_segsort.hip) a call or a delivery burst runs, derived once
// from the RXG_DLV_* flags: it gives the workspace size and the number of
// totals words (tcp_launch below runs it).
struct k4_form {
    bool gro = false, order = false, assemble = false;
    bool inplace = false; // records only: no payload is gathered
    static k4_form of(uint32_t dlv) {
        k4_form f;
        f.gro = (dlv & RXG_DLV_TCP_GRO) != 0;
        f.assemble = (dlv & RXG_DLV_TCP_ASSEMBLE) != 0;
        // (assembly runs the ordering stage itself and reports its moved count)
        f.order = (dlv & RXG_DLV_TCP_ORDER) != 0 || f.assemble;
        f.inplace = (dlv & RXG_DLV_TCP_IN_PLACE) != 0;
        return f;
    }
    uint32_t ntotals() const { return assemble ? 6u : order ? 5u : gro ? 4u : 3u; }
    size_t ws_bytes(uint32_t n) const {
        return assemble ? rx_assemble_ws_bytes(n) : order ? rx_order_ws_bytes(n)
               : gro    ? rx_gro_ws_bytes(n) : rx_segsort_ws_bytes(n);
    }
};

struct rxg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // flow tables: host images + registry (rx_flows.h), device copies
    rx_flowset fs;
    bool dirty = false; // host changes not yet on the device (rxg_flows_commit)
    uint4 *d_udp = nullptr, *d_tcp = nullptr;
    size_t d_udp_cap = 0, d_tcp_cap = 0; // bytes
    uint32_t *d_listen = nullptr;   // 65536
    uint32_t *d_udp_port = nullptr; // 65536
    uint2 *d_udpc = nullptr;        // up to 2 * RX_UDPC_MAX_FLOWS slots
    uint16_t *d_udpw = nullptr;     // up to RX_UDPW_MAX_PORTS
    rx_delta *h_delta = nullptr, *d_delta = nullptr; // pinned staging + device copy
    hipEvent_t ev_commit = nullptr; // after the last commit's writes
    uint64_t commit_gen = 0;
    rx_track trk[RX_TRACK];
    rx_track *cur = nullptr; // the stream of the latest burst (its event not yet recorded)
    uint64_t use_clock = 0;
    uint32_t tune_tables = 0; // rxg_tune_tables flags
    uint32_t tune_ingest = RXG_INGEST_AUTO; // rxg_tune_ingest
    uint32_t deliver_flags = 0;             // rxg_tune_deliver (RXG_DLV_*)
    // The burst passes behind the classify, one struct each: what its
    // rxg_tune_* / rxg_*_set call left, its workspace (ws_grow; every call on
    // this context shares it) and the device results of the delivery bursts
    // (first use: rxg_deliver_submit).  The pinned copies: delivery_set below.
    struct ws_buf { void *p = nullptr; size_t cap = 0; };
    struct udp_host { // one group of pinned copies of K3's results
        rxg_dgram *h_dg = nullptr;
        uint32_t *h_first = nullptr, *h_totals = nullptr;
        uint8_t *h_payload = nullptr;
    };
    struct udp_pass { // UDP compaction (K3, rx_compact.hip); sized by max_pkts / max_bytes
        rxg_dgram *d_dg = nullptr;
        uint32_t *d_first = nullptr, *d_totals = nullptr;
        uint8_t *d_payload = nullptr;
        ws_buf ws;
        udp_host own; // rxg_process_mbufs_udp's copies (it uses no delivery set)
    } udp;
    struct tcp_pass { // TCP segment sort + payload gather (K4 and its forms, rx_segsort.hip)
        uint32_t window = RXG_GRO_DEFAULT_WINDOW; // rxg_tune_gro (RXG_DLV_TCP_GRO)
        rxg_segment *d_seg = nullptr;
        uint8_t *d_payload = nullptr;
        rxg_tcp_run *d_run = nullptr;       // (RXG_DLV_TCP_GRO: first use)
        rxg_tcp_stream *d_stream = nullptr; // (RXG_DLV_TCP_ASSEMBLE: first use)
        uint32_t *d_totals = nullptr;
        ws_buf ws; // one buffer for all four forms
    } tcp;
    struct ddos_pass { // the entropy flood detector (K6, rx_ddos.hip)
        uint32_t lanes = 0;                       // rxg_tune_ddos
        double thresh = RXG_DDOS_DEFAULT_THRESH;  // rxg_tune_ddos_thresh
        ws_buf ws;
        rxg_ddos_state *d_state = nullptr; // the state the delivery bursts carry (RXG_DLV_DDOS)
        rxg_ddos_summary *d_sum = nullptr;
    } ddos;
    struct cookie_pass { // SYN cookies (K7, rx_syncookie.hip)
        ws_buf ws;
        rxg_ck_params p{}; // rxg_syncookie_set, with the listener mask (hmask: the upload's source,
                           // kept until ev says it has been read)
        uint32_t id_space = 0;
        std::vector<uint32_t> hmask;
        ws_buf mask;
        hipEvent_t ev = nullptr;
        uint8_t *d_status = nullptr;
        rxg_txd *d_txd = nullptr;
        uint32_t *d_totals = nullptr;
    } ck;
    struct l2_pass { // the L2 responder (K8, rx_l2.hip)
        ws_buf ws;
        rxg_l2_params p{}; // rxg_l2_set, with the answer capacity
        uint64_t cap = 0;
        uint8_t *d_status = nullptr, *d_out = nullptr;
        uint64_t d_out_cap = 0;
        uint32_t *d_roff = nullptr, *d_rsrc = nullptr, *d_totals = nullptr;
        uint16_t *d_rlen = nullptr;
    } l2;
    rx_ft_dev ft{};
    uint32_t tune_g = 0, tune_p = 0, tune_fpg = 0, tune_pipe = ~0u; // rxg_tune override
    uint32_t tune_bpc = 0; // rxg_tune_grid: resident blocks per CU cap (0 = occupancy)
    uint32_t tune_tx = RXG_TX_AUTO, tune_tx_bpc = 0; // rxg_tune_tx
    uint32_t tune_txe = RXG_TX_AUTO, tune_txe_bpc = 0; // rxg_tune_txe
    void *d_txe = nullptr; // rxg_tx_encode's device staging, grown on demand
    size_t d_txe_cap = 0;
    // launch workspace, grown on demand: [binned lists][count indices x 2][count
    // slabs].  Three regions are tracked, each by the event of its last use and
    // that use's stream: index buffer 0 (with the lists), index buffer 1, the
    // slabs.  A launch that uses a region on another stream than its last use
    // waits for that event first, so bursts on different streams never share a
    // region in flight, and rxg_classify_dev_cs can classify burst k+1 into one
    // index buffer while burst k is counted from the other on the count stream.
    uint32_t *d_ws = nullptr;
    size_t d_ws_cap = 0;
    struct ws_use {
        hipEvent_t ev = nullptr;
        hipStream_t st = nullptr;
        bool used = false;
    } wu[4]; // index buffers 0..2, slabs (WS_*)
    // region offsets depend on the burst shape (frame count, binned path, size);
    // a change of shape waits on every region
    struct ws_shape {
        uint32_t n = 0;
        bool lists = false;
        size_t bytes = 0;
        bool operator!=(const ws_shape &o) const { return n != o.n || lists != o.lists || bytes != o.bytes; }
    } ws_layout;
    uint32_t ws_flip = 0; // index buffer of the next split-stream burst
    uint32_t ws_nbuf = 3; // index buffers of the split-stream bursts (RXG_TT_COUNT_2BUF: 2)
    hipEvent_t ev_k1 = nullptr; // split-stream burst: classify done (count stream waits on it)
    void *d_aux = nullptr; // RSS split / gather workspace, grown on demand
    size_t d_aux_cap = 0;
    hipEvent_t ev_aux = nullptr; // after the last split / gather that used d_aux
    hipStream_t aux_st = nullptr;
    bool aux_used = false;
    // context-owned per-flow counts (host-buffer path): d_counts since the last
    // rxg_ctx_counts_allreduce, d_counts_base the all-reduced total before it
    unsigned long long *d_counts = nullptr, *d_counts_base = nullptr;
    uint32_t counts_cap = 0;
    // ids removed since the last commit: their counts are zeroed by that
    // commit (RX_D_CZERO), so a reused id starts from 0
    std::vector<uint32_t> czero_udp, czero_tcp;
    // host-buffer path: a ring of RXG_PIPE_DEPTH staging slots; burst t uses
    // slot t % depth.  Copies in run on s_h2d, kernels on `stream`, verdict
    // copies out on s_d2h, chained by events, so burst t+1's frames cross PCIe
    // while burst t is classified and burst t-1's verdicts come back.
    uint32_t max_pkts = 0;
    uint64_t max_bytes = 0;
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    struct slot {
        uint8_t *h_stage = nullptr; // pinned, mbuf gather
        unsigned long long *h_src = nullptr, *d_src = nullptr; // device-pulled frames (registered)
        uint32_t *h_off = nullptr;
        uint16_t *h_len = nullptr;
        uint8_t *d_pkts = nullptr;
        uint32_t *d_off = nullptr;
        uint16_t *d_len = nullptr;
        uint4 *d_out = nullptr;
        hipEvent_t ev_in = nullptr;   // inputs copied (h_stage reusable, kernel may start)
        hipEvent_t ev_k = nullptr;    // kernel done (d_pkts/d_off/d_len reusable)
        hipEvent_t ev_done = nullptr; // verdicts in host memory (d_out reusable)
        uint64_t ticket = 0;          // last burst submitted to this slot (0 = none)
    } slots[RXG_PIPE_DEPTH];
    uint64_t next_ticket = 1;
    // pinned payload buffers a caller may keep past the next burst
    // (rxg_payload_hold / _release: the receive fragments of a burst point
    // into them until the application has read them); refs counts the holds,
    // the library's own one included (until its next burst call)
    struct pl_buf {
        uint8_t *h = nullptr;
        std::atomic<int> refs{0};
    } pl[RXG_PAYLOAD_BUFS];
    // the delivery sets (rxg_deliver_submit / _wait): up to RXG_DELIVER_DEPTH
    // bursts in flight, each with its own pinned copies of the results (the
    // device buffers are shared: every step runs on `stream`, in order) and its
    // phase events; a set's results stay valid until the set is reused
    struct delivery_set {
        bool on = false; // submitted and not yet waited for
        // per pass: whether it ran in this set's burst (copied at submit: the
        // wait reads no table) and the pinned copies of its results
        struct : udp_host { bool ran = false; } udp;
        struct {
            bool ran = false;
            k4_form form{}; // the form that ran
            rxg_segment *h_seg = nullptr;
            uint8_t *h_payload = nullptr; // the set's own buffer (no pooled one was free)
            uint32_t *h_totals = nullptr;
            rxg_tcp_run *h_run = nullptr;
            rxg_tcp_stream *h_stream = nullptr;
            uint32_t nrun = 0, moved = 0, nstream = 0; // (the wait fills them: rxg_delivery_runs, ..)
        } tcp;
        struct { bool ran = false; rxg_ddos_summary *h_sum = nullptr; } ddos; // (rxg_delivery_ddos)
        struct {
            bool ran = false; // (rxg_delivery_cookies)
            uint8_t *h_status = nullptr;
            rxg_txd *h_txd = nullptr;
            uint32_t *h_totals = nullptr;
        } ck;
        struct {
            bool ran = false; // (rxg_delivery_l2)
            uint8_t *h_status = nullptr, *h_out = nullptr;
            uint64_t h_out_cap = 0;
            uint32_t *h_roff = nullptr, *h_rsrc = nullptr, *h_totals = nullptr;
            uint16_t *h_rlen = nullptr;
        } l2;
        uint64_t ticket = 0;
        double t0 = 0, t1 = 0;
        int pl = -1; // the pooled payload buffer the library holds for this set
        hipEvent_t tev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    } dls[RXG_DELIVER_DEPTH];
    uint32_t dl_next = 0; // the set the next submit takes (round robin)
    // registered host memory (rxg_register_host): frames of an mbuf burst that
    // all lie in it are pulled by the device instead of gathered on the host
    struct host_region {
        uint8_t *h = nullptr, *d = nullptr;
        uint64_t bytes = 0;
        bool ours = false; // registered here (unregistered at close)
    };
    std::vector<host_region> regions;
    uint32_t region_hint = 0;
};

// a flow-table array of at least `bytes`, stream-ordered on s (hipMallocAsync /
// hipFreeAsync: neither synchronises the device, unlike hipFree)
static int ensure_dev_async(void **p, size_t *cap, size_t bytes, hipStream_t s) {
    if (*cap >= bytes && *p) return RXG_OK;
    if (*p) HIPCHK(hipFreeAsync(*p, s));
    *p = nullptr;
    *cap = 0;
    HIPCHK(hipMallocAsync(p, bytes, s));
    *cap = bytes;
    return RXG_OK;
}

#define RCCHK(x)                                                                                   \
    do {                                                                                           \
        int rc_ = (x);                                                                             \
        if (rc_) return rc_;                                                                       \
    } while (0)

// A burst pass's workspace grown to `bytes` before a launch on s.  Its uses are
// ordered by the caller (all on one stream, or event-chained), so it is freed
// and grown in stream order.  (bytes == 0 with no buffer yet: nothing to do.)
static int ws_grow(rxg_ctx::ws_buf &ws, size_t bytes, hipStream_t s, bool *grew = nullptr) {
    if (grew) *grew = bytes > ws.cap; // (a new buffer: its contents are undefined)
    return bytes <= ws.cap ? RXG_OK : ensure_dev_async(&ws.p, &ws.cap, bytes, s);
}

// First-use allocations, one pointer each: a failed call returns its error
// with *p null, so the next call allocates exactly what is still missing.
template <class T> static int dev_alloc(T **p, size_t bytes) {
    const hipError_t e = *p ? hipSuccess : hipMalloc((void **)p, bytes);
    if (e != hipSuccess) *p = nullptr;
    return rx_set_hip_error(e);
}
template <class T> static int pin_alloc(T **p, size_t bytes) {
    const hipError_t e = *p ? hipSuccess : hipHostMalloc((void **)p, bytes, 0);
    if (e != hipSuccess) *p = nullptr;
    return rx_set_hip_error(e);
}
// a device result and its pinned copy, the same size
template <class T> static int both_alloc(T **d, T **h, size_t bytes) {
    RCCHK(dev_alloc(d, bytes));
    return pin_alloc(h, bytes);
}
static void dev_free(std::initializer_list<void *> ds) {
    for (void *d : ds) (void)hipFree(d);
}
static void pin_free(std::initializer_list<void *> hs) {
    for (void *h : hs)
        if (h) (void)hipHostFree(h);
}
// a result's copy to pinned host memory, on the context's stream
static hipError_t copy_back(rxg_ctx *c, void *h, const void *d, size_t bytes) {
    return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream);
}
static bool bad_unit(uint32_t off_unit_log2) { return off_unit_log2 < 4 || off_unit_log2 > 16; }
// the opening of the device entry points: a context with a device
static int dev_ctx(const rxg_ctx *c) {
    if (!c) return RXG_EINVAL;
    return c->device == RXG_HOST_ONLY ? RXG_ENODEV : RXG_OK;
}

// Save the calling thread's current device, switch to the context's, restore
// it on scope exit: the API never leaves a C host thread on another device.
struct dev_guard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit dev_guard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev);
    }
    ~dev_guard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};
#define DEVGUARD(c)                                                                                \
    dev_guard dg_((c)->device);                                                                    \
    HIPCHK(dg_.err)

// a fresh hash seed (rx_hash3s): random at rxg_open, then a mix on reseeds
static uint32_t next_seed(uint32_t s) {
    uint64_t z = rx_mix64(((uint64_t)s << 32) ^ 0xA0761D6478BD642Full);
    return (uint32_t)(z >> 32) | 1u;
}
static uint32_t random_seed() {
    uint32_t s = 0;
    FILE *f = fopen("/dev/urandom", "rb");
    if (f) {
        if (fread(&s, sizeof(s), 1, f) != 1) s = 0;
        fclose(f);
    }
    s ^= (uint32_t)(uintptr_t)&s ^ (uint32_t)clock();
    return next_seed(s);
}

// ---- burst tracking ----------------------------------------------------
// Table writes (commits, rxg_flows_sync) must follow every burst of this
// context still reading the tables, on whatever stream it ran — never the
// device's other work.  An event per burst would do it but costs the burst
// loop ~1% at cfg2 (0.2361 vs 0.2330 ms, interleaved A/B in one process,
// profiles/r03a/ab_track.txt), so events are recorded only when needed: on a
// stream switch, on the stream the context leaves (it was used a moment
// ago), and lazily on the current stream when a table write comes.  The
// stream of the context's most recent burst must therefore still exist at
// the context's next call (rxgpu.h).
static int track_slot(rxg_ctx *c, hipStream_t s, rx_track **out) {
    rx_track *t = nullptr, *old = &c->trk[0];
    for (rx_track &x : c->trk) {
        if (x.used && x.s == s) t = &x;
        if (!x.used || (old->used && x.last_use < old->last_use)) old = &x;
    }
    if (!t) {
        t = old;
        if (t->used) HIPCHK(hipEventSynchronize(t->ev)); // (never the current stream: LRU)
        t->s = s;
        t->used = true;
        t->commit_seen = c->commit_gen; // (a new stream: tables already on the device
                                        // unless a commit is pending, which runs on s)
        if (c->commit_gen) HIPCHK(hipStreamWaitEvent(s, c->ev_commit, 0));
    }
    t->last_use = ++c->use_clock;
    *out = t;
    return RXG_OK;
}

// the event of tracking entry x marks its stream's last burst: recorded now
// for the current stream (lazily), already recorded for the others
static hipError_t track_mark(rxg_ctx *c, rx_track &x) {
    if (&x != c->cur) return hipSuccess;
    hipError_t e = hipEventRecord(x.ev, x.s);
    if (e == hipSuccess) c->cur = nullptr; // (its event now covers all its bursts)
    return e;
}

// before a burst on s: the pending table changes, then order s after the last commit
static int commit_on(rxg_ctx *c, hipStream_t s);
static int burst_begin(rxg_ctx *c, hipStream_t s) {
    if (c->dirty) {
        int rc = commit_on(c, s);
        if (rc) return rc;
    }
    rx_track *t;
    int rc = track_slot(c, s, &t);
    if (rc) return rc;
    if (c->cur && c->cur != t) HIPCHK(track_mark(c, *c->cur)); // leaving a stream
    c->cur = t;
    if (t->commit_seen < c->commit_gen) {
        HIPCHK(hipStreamWaitEvent(s, c->ev_commit, 0));
        t->commit_seen = c->commit_gen;
    }
    return RXG_OK;
}
// host wait for every burst of this context (a table rebuild in place)
static int bursts_drain(rxg_ctx *c) {
    for (rx_track &x : c->trk)
        if (x.used) {
            HIPCHK(track_mark(c, x));
            HIPCHK(hipEventSynchronize(x.ev));
        }
    for (rxg_ctx::ws_use &u : c->wu)
        if (u.used) HIPCHK(hipEventSynchronize(u.ev));
    if (c->stream) HIPCHK(hipStreamSynchronize(c->stream));
    if (c->s_h2d) HIPCHK(hipStreamSynchronize(c->s_h2d));
    if (c->s_d2h) HIPCHK(hipStreamSynchronize(c->s_d2h));
    return RXG_OK;
}

// ---- device upload of the flow tables ------------------------------------
static void ft_fill(rxg_ctx *c) {
    const rx_flowset &fs = c->fs;
    c->ft.udp = c->d_udp;
    c->ft.tcp = c->d_tcp;
    c->ft.listen = c->d_listen;
    c->ft.udp_mask = fs.udp.tab.mask;
    c->ft.tcp_mask = fs.tcp.tab.mask;
    c->ft.udp_probe = fs.udp.live ? fs.udp.tab.probe : 0;
    c->ft.tcp_probe = fs.tcp.live ? fs.tcp.tab.probe : 0;
    c->ft.hseed = fs.seed;
    c->ft.udpc = fs.udpc.empty() ? nullptr : c->d_udpc;
    c->ft.udpc_mask = fs.udpc.empty() ? 0 : (uint32_t)fs.udpc.size() - 1;
    c->ft.udpc_probe = fs.udpc_probe;
    c->ft.udpc_other = fs.udpc_other;
    c->ft.udp_port = fs.port.empty() ? nullptr : c->d_udp_port;
    c->ft.udp_dip = fs.udp_dip;
    c->ft.udpw = fs.udpw.empty() ? nullptr : c->d_udpw;
    c->ft.udpw_lo = fs.udpw_lo;
    c->ft.udpw_n = (uint32_t)fs.udpw.size();
}

// whole arrays (a rebuild, or more changes than one delta batch holds), on s;
// the host waits for the copies (pageable sources)
static int upload_tab(rx_slot_table &t, uint4 **d, size_t *cap, hipStream_t s) {
    const size_t bytes = t.slots.size() * sizeof(uint4);
    int rc = ensure_dev_async((void **)d, cap, bytes, s);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(*d, t.slots.data(), bytes, hipMemcpyHostToDevice, s));
    t.all_dirty = false;
    t.dirty.clear();
    return RXG_OK;
}

// the counts follow the id space: UDP ids [0, nu), TCP ids at nu + id; a
// grown id space moves the context's own count vectors to the new layout
static int counts_layout(rxg_ctx *c, uint32_t nu, uint32_t nt, hipStream_t s) {
    const uint32_t onu = c->ft.nu, ont = c->ft.nt;
    const uint32_t nf = std::max(nu + nt, 1u);
    if (c->d_counts && nu == onu && nt == ont) return RXG_OK;
    unsigned long long *a = nullptr, *b = nullptr;
    HIPCHK(hipMallocAsync((void **)&a, (size_t)nf * 8, s));
    HIPCHK(hipMallocAsync((void **)&b, (size_t)nf * 8, s));
    HIPCHK(hipMemsetAsync(a, 0, (size_t)nf * 8, s));
    HIPCHK(hipMemsetAsync(b, 0, (size_t)nf * 8, s));
    if (c->d_counts) {
        unsigned long long *src[2] = {c->d_counts, c->d_counts_base}, *dst[2] = {a, b};
        for (int k = 0; k < 2; ++k) {
            const uint32_t ku = std::min(onu, nu), kt = std::min(ont, nt);
            if (ku) HIPCHK(hipMemcpyAsync(dst[k], src[k], ku * 8ull, hipMemcpyDeviceToDevice, s));
            if (kt)
                HIPCHK(hipMemcpyAsync(dst[k] + nu, src[k] + onu, kt * 8ull, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipFreeAsync(src[k], s));
        }
    }
    c->d_counts = a;
    c->d_counts_base = b;
    c->counts_cap = nf;
    c->ft.nu = nu;
    c->ft.nt = nt;
    return RXG_OK;
}

// every pending host change of the flow tables onto the device, in stream
// order on s (after the bursts of other streams that may still read them)
static int commit_on(rxg_ctx *c, hipStream_t s) {
    if (c->device == RXG_HOST_ONLY) {
        c->dirty = false;
        return RXG_OK;
    }
    rx_flowset &fs = c->fs;
    for (rx_track &x : c->trk)
        if (x.used && x.s != s) {
            HIPCHK(track_mark(c, x));
            HIPCHK(hipStreamWaitEvent(s, x.ev, 0));
        }
    for (rxg_ctx::ws_use &u : c->wu)
        if (u.used && u.st != s) HIPCHK(hipStreamWaitEvent(s, u.ev, 0));
    int rc = counts_layout(c, fs.udp.id_space(), fs.tcp.id_space(), s);
    if (rc) return rc;
    // the previous commit's staging copy must be done before it is refilled
    if (c->commit_gen) HIPCHK(hipEventSynchronize(c->ev_commit));
    const size_t nrec = fs.udp.tab.dirty.size() + fs.tcp.tab.dirty.size() +
                        fs.listen_dirty.size() + fs.port_dirty.size() +
                        (fs.small_dirty ? (fs.udpc.size() / 2 + (fs.udpw.size() + 7) / 8) : 0);
    const bool whole = nrec > RX_DELTA_CAP;
    bool sync = false;
    if (fs.udp.tab.all_dirty || whole) {
        if ((rc = upload_tab(fs.udp.tab, &c->d_udp, &c->d_udp_cap, s))) return rc;
        sync = true;
    }
    if (fs.tcp.tab.all_dirty || whole) {
        if ((rc = upload_tab(fs.tcp.tab, &c->d_tcp, &c->d_tcp_cap, s))) return rc;
        sync = true;
    }
    if (fs.listen_all_dirty || whole) {
        HIPCHK(hipMemcpyAsync(c->d_listen, fs.listen.data(), 65536 * 4, hipMemcpyHostToDevice, s));
        fs.listen_all_dirty = false;
        fs.listen_dirty.clear();
        sync = true;
    }
    if ((fs.port_all_dirty || whole) && !fs.port.empty()) {
        HIPCHK(hipMemcpyAsync(c->d_udp_port, fs.port.data(), 65536 * 4, hipMemcpyHostToDevice, s));
        sync = true;
    }
    if (fs.port_all_dirty || whole) fs.port_all_dirty = false, fs.port_dirty.clear();
    uint32_t n = 0;
    rx_delta *r = c->h_delta;
    auto put = [&](uint32_t which, uint32_t idx, uint4 v) {
        r[n].which = which;
        r[n].idx = idx;
        r[n]._r0 = r[n]._r1 = 0;
        r[n].v = v;
        ++n;
    };
    for (uint32_t i : fs.udp.tab.dirty) put(RX_D_UDP, i, fs.udp.tab.slots[i]);
    for (uint32_t i : fs.tcp.tab.dirty) put(RX_D_TCP, i, fs.tcp.tab.slots[i]);
    for (uint32_t p : fs.listen_dirty) put(RX_D_LISTEN, p, make_uint4(fs.listen[p], 0, 0, 0));
    if (!fs.port.empty())
        for (uint32_t p : fs.port_dirty) put(RX_D_PORT, p, make_uint4(fs.port[p], 0, 0, 0));
    if (fs.small_dirty) {
        for (size_t k = 0; 2 * k < fs.udpc.size(); ++k) {
            const uint2 x = fs.udpc[2 * k], y = fs.udpc[2 * k + 1];
            put(RX_D_UDPC, (uint32_t)k, make_uint4(x.x, x.y, y.x, y.y));
        }
        for (size_t k = 0; 8 * k < fs.udpw.size(); ++k) {
            uint32_t w[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            for (size_t j = 0; j < 8 && 8 * k + j < fs.udpw.size(); ++j) {
                const uint32_t sh = 16u * (uint32_t)(j & 1);
                w[j / 2] = (w[j / 2] & ~(0xFFFFu << sh)) | ((uint32_t)fs.udpw[8 * k + j] << sh);
            }
            put(RX_D_UDPW, (uint32_t)k, make_uint4(w[0], w[1], w[2], w[3]));
        }
        fs.small_dirty = false;
    }
    fs.udp.tab.dirty.clear();
    fs.tcp.tab.dirty.clear();
    fs.listen_dirty.clear();
    fs.port_dirty.clear();
    // the staged records to the device and the scatter kernel; a full staging
    // buffer (more removed ids than it holds) is flushed and refilled after
    // its copy has left
    auto flush = [&]() -> int {
        if (!n) return RXG_OK;
        HIPCHK(hipMemcpyAsync(c->d_delta, c->h_delta, n * sizeof(rx_delta), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(rx_delta_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c->d_delta, n,
                           c->d_udp, c->d_tcp, c->d_listen, c->d_udp_port,
                           reinterpret_cast<uint4 *>(c->d_udpc), reinterpret_cast<uint4 *>(c->d_udpw),
                           c->d_counts, c->d_counts_base);
        HIPCHK(hipGetLastError());
        n = 0;
        return RXG_OK;
    };
    // counts of removed ids (in the layout counts_layout just made: TCP at nu + id)
    const uint32_t nf = c->ft.nu + c->ft.nt;
    for (int k = 0; k < 2; ++k)
        for (uint32_t id : k ? c->czero_tcp : c->czero_udp) {
            const uint32_t idx = k ? c->ft.nu + id : id;
            if (idx >= nf || (!k && id >= c->ft.nu)) continue;
            if (n == RX_DELTA_ROOM) {
                if ((rc = flush())) return rc;
                HIPCHK(hipEventRecord(c->ev_commit, s));
                HIPCHK(hipEventSynchronize(c->ev_commit)); // (the staging copy has left)
            }
            put(RX_D_CZERO, idx, make_uint4(0, 0, 0, 0));
        }
    c->czero_udp.clear();
    c->czero_tcp.clear();
    if ((rc = flush())) return rc;
    HIPCHK(hipEventRecord(c->ev_commit, s));
    ++c->commit_gen;
    for (rx_track &x : c->trk)
        if (x.used && x.s == s) x.commit_seen = c->commit_gen;
    ft_fill(c);
    c->dirty = false;
    if (sync) HIPCHK(hipStreamSynchronize(s)); // (pageable whole-array sources)
    return RXG_OK;
}

extern "C" {

const char *rxg_strerror(int err) {

    switch (err) {
    case RXG_OK:
        return "ok";
    case RXG_EINVAL:
        return "invalid argument";
    case RXG_ENOMEM:
        return "out of memory";
    case RXG_ENODEV:
        return "no HIP device";
    case RXG_ERANGE:
        return "burst exceeds the context's staging capacity or 32-bit offsets";
    case RXG_EHIP:
        return "HIP runtime error (see rxg_last_hip_error)";
    case RXG_ECOMM:
        return "RCCL error (see rxg_last_hip_error)";
    default:
        return "unknown error";
    }
}

const char *rxg_last_hip_error(void) { return g_last_hip.c_str(); }

int rxg_open(rxg_ctx **out, int device, uint32_t max_pkts, uint64_t max_bytes) {
    if (!out) return RXG_EINVAL;
    *out = nullptr;
    rxg_ctx *c;
    int rc = RXG_OK;
    if (device == RXG_HOST_ONLY) { // control-plane context: flow tables + host lookups only
        c = new (std::nothrow) rxg_ctx();
        if (!c) return RXG_ENOMEM;
        c->device = RXG_HOST_ONLY;
        c->fs.seed = random_seed();
        rc = rxg_flows_sync(c, nullptr, 0, nullptr, 0);
        if (rc != RXG_OK) {
            rxg_close(c);
            return rc;
        }
        *out = c;
        return RXG_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return RXG_ENODEV;
    if (device < 0 || device >= ndev) return RXG_ENODEV;
    c = new (std::nothrow) rxg_ctx();
    if (!c) return RXG_ENOMEM;
    c->device = device;
    c->fs.seed = random_seed();
    dev_guard dg(device);
    do {
        if ((rc = rx_set_hip_error(dg.err))) break;
        if ((rc = rx_set_hip_error(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking))))
            break;
        if ((rc = rx_set_hip_error(hipMalloc(&c->d_listen, 65536 * sizeof(uint32_t))))) break;
        if ((rc = rx_set_hip_error(hipMalloc(&c->d_udp_port, 65536 * sizeof(uint32_t))))) break;
        if ((rc = rx_set_hip_error(hipMalloc(&c->d_udpc, 2 * RX_UDPC_MAX_FLOWS * sizeof(uint2))))) break;
        if ((rc = rx_set_hip_error(hipMalloc(&c->d_udpw, RX_UDPW_MAX_PORTS * sizeof(uint16_t))))) break;
        const size_t dbytes = RX_DELTA_ROOM * sizeof(rx_delta);
        if ((rc = rx_set_hip_error(hipHostMalloc((void **)&c->h_delta, dbytes, 0)))) break;
        if ((rc = rx_set_hip_error(hipMalloc(&c->d_delta, dbytes)))) break;
        if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&c->ev_commit, hipEventDisableTiming))))
            break;
        for (rx_track &t : c->trk)
            if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&t.ev, hipEventDisableTiming)))) break;
        if (rc) break;
        for (rxg_ctx::ws_use &u : c->wu)
            if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&u.ev, hipEventDisableTiming))))
                break;
        if (rc) break;
        if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&c->ev_k1, hipEventDisableTiming))))
            break;
        if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&c->ev_aux, hipEventDisableTiming))))
            break;
        c->max_pkts = max_pkts;
        c->max_bytes = (max_bytes + 15) & ~15ull;
        if (max_pkts && c->max_bytes) {
            if ((rc = rx_set_hip_error(hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking))))
                break;
            if ((rc = rx_set_hip_error(hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking))))
                break;
            for (rxg_ctx::slot &sl : c->slots) {
                if ((rc = rx_set_hip_error(hipHostMalloc((void **)&sl.h_stage, c->max_bytes, 0)))) break;
                if ((rc = rx_set_hip_error(hipHostMalloc((void **)&sl.h_off, max_pkts * 4ull, 0)))) break;
                if ((rc = rx_set_hip_error(hipHostMalloc((void **)&sl.h_len, max_pkts * 2ull, 0)))) break;
                if ((rc = rx_set_hip_error(hipMalloc(&sl.d_pkts, c->max_bytes)))) break;
                if ((rc = rx_set_hip_error(hipMalloc(&sl.d_off, max_pkts * 4ull)))) break;
                if ((rc = rx_set_hip_error(hipMalloc(&sl.d_len, max_pkts * 2ull)))) break;
                if ((rc = rx_set_hip_error(hipMalloc(&sl.d_out, max_pkts * 16ull)))) break;
                const unsigned fl = hipEventDisableTiming;
                if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&sl.ev_in, fl)))) break;
                if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&sl.ev_k, fl)))) break;
                if ((rc = rx_set_hip_error(hipEventCreateWithFlags(&sl.ev_done, fl)))) break;
            }
        }
    } while (0);
    if (rc == RXG_OK) rc = rxg_flows_sync(c, nullptr, 0, nullptr, 0);
    if (rc != RXG_OK) {
        rxg_close(c);
        return rc;
    }
    *out = c;
    return RXG_OK;
}

// every buffer of a burst pass, the sets' pinned copies included (with the passes, below)
static void udp_release(rxg_ctx *c), tcp_release(rxg_ctx *c), ddos_release(rxg_ctx *c),
    ck_release(rxg_ctx *c), l2_release(rxg_ctx *c);

void rxg_close(rxg_ctx *c) {
    if (!c) return;
    if (c->device == RXG_HOST_ONLY) {
        delete c;
        return;
    }
    dev_guard dg(c->device);
    // waits for what the context can name without touching the caller's
    // streams: their recorded events and the context's own streams.  The
    // stream of the latest burst (c->cur, its event not recorded) may already
    // be destroyed (the usual teardown order: synchronise, destroy the stream,
    // close), so nothing is recorded on it; hipFree below synchronises the
    // device before it releases memory a kernel could still read.
    for (rx_track &x : c->trk)
        if (x.used && &x != c->cur) (void)hipEventSynchronize(x.ev);
    for (rxg_ctx::ws_use &u : c->wu)
        if (u.used) (void)hipEventSynchronize(u.ev);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->s_h2d) (void)hipStreamSynchronize(c->s_h2d);
    if (c->s_d2h) (void)hipStreamSynchronize(c->s_d2h);
    dev_free({c->d_udp, c->d_tcp, c->d_listen, c->d_udp_port, c->d_udpc, c->d_udpw, c->d_delta,
              c->d_counts, c->d_counts_base, c->d_ws, c->d_aux, c->d_txe});
    pin_free({c->h_delta});
    udp_release(c);
    tcp_release(c);
    ddos_release(c);
    ck_release(c);
    l2_release(c);
    for (rxg_ctx::delivery_set &ds : c->dls)
        for (hipEvent_t e : ds.tev)
            if (e) (void)hipEventDestroy(e);
    for (rxg_ctx::pl_buf &b : c->pl) pin_free({b.h});
    for (rxg_ctx::ws_use &u : c->wu)
        if (u.ev) (void)hipEventDestroy(u.ev);
    for (rx_track &t : c->trk)
        if (t.ev) (void)hipEventDestroy(t.ev);
    if (c->ev_commit) (void)hipEventDestroy(c->ev_commit);
    if (c->ev_k1) (void)hipEventDestroy(c->ev_k1);
    if (c->ev_aux) (void)hipEventDestroy(c->ev_aux);
    for (rxg_ctx::slot &sl : c->slots) {
        dev_free({sl.d_pkts, sl.d_off, sl.d_len, sl.d_out, sl.d_src});
        pin_free({sl.h_stage, sl.h_off, sl.h_len, sl.h_src});
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_k) (void)hipEventDestroy(sl.ev_k);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
    }
    for (const rxg_ctx::host_region &r : c->regions)
        if (r.ours) (void)hipHostUnregister(r.h);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->s_h2d) (void)hipStreamDestroy(c->s_h2d);
    if (c->s_d2h) (void)hipStreamDestroy(c->s_d2h);
    delete c;
}

// ---- control blocks (rx_flows.h) ------------------------------------------
static void udp_set(rx_block &x, const rxg_udp_sock &u) {
    x.a = u.localip;
    x.b = u.localport;
    x.c = 17u;
    x.status = u.protocol;
    // get_hostinfo_fromip_port matches (dip, dport, proto); every socket the
    // reference creates has protocol 17 (nsocket, common.c:281) and the lookup
    // is only called with 17 (udp.c:14), so other protocols never match
    x.keyed = u.protocol == 17;
}
static void tcp_set(rx_block &x, const rxg_tcb &t) {
    x.a = t.sip;
    x.b = t.dip;
    x.c = (uint32_t)t.sport | ((uint32_t)t.dport << 16);
    x.status = t.status;
    x.keyed = true;
}

// the whole flow set, then every device table: a control-plane operation that
// waits for this context's own bursts (never the device's other work)
static int full_upload(rxg_ctx *c) {
    c->fs.rebuild_all(next_seed);
    c->dirty = true;
    if (c->device == RXG_HOST_ONLY) {
        c->ft.nu = c->fs.udp.id_space();
        c->ft.nt = c->fs.tcp.id_space();
        c->ft.hseed = c->fs.seed;
        c->dirty = false;
        return RXG_OK;
    }
    DEVGUARD(c);
    int rc = bursts_drain(c);
    if (rc) return rc;
    rc = commit_on(c, c->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return RXG_OK;
}

int rxg_flows_sync(rxg_ctx *c, const rxg_udp_sock *u, uint32_t nu, const rxg_tcb *t, uint32_t nt) {
    if (!c || (nu && !u) || (nt && !t)) return RXG_EINVAL;
    rx_flowset &fs = c->fs;
    fs.clear();
    c->czero_udp.clear(); // (the counts are zeroed whole below)
    c->czero_tcp.clear();
    fs.port_table = !(c->tune_tables & RXG_TT_NO_UDP_PORT);
    fs.udp.blk.resize(nu);
    for (uint32_t i = 0; i < nu; ++i) {
        rx_block &x = fs.udp.blk[i];
        udp_set(x, u[i]);
        x.seq = fs.udp.seq_next++;
        x.live = true;
    }
    fs.udp.live = nu;
    fs.tcp.blk.resize(nt);
    for (uint32_t i = 0; i < nt; ++i) {
        rx_block &x = fs.tcp.blk[i];
        tcp_set(x, t[i]);
        x.seq = fs.tcp.seq_next++;
        x.live = true;
    }
    fs.tcp.live = nt;
    for (uint32_t i = 0; i < nt; ++i)
        if (t[i].status == RXG_TCP_STATUS_LISTEN) fs.listen_add(i);
    int rc = full_upload(c); // (rebuild_all places each key's newest block)
    if (rc) return rc;
    // chains of duplicate keys, newest first: one walk over the blocks, newest first
    for (rx_registry *r : {&fs.udp, &fs.tcp}) {
        std::vector<uint32_t> tail(r->tab.ns(), RXG_FLOW_NONE);
        for (uint32_t id = (uint32_t)r->blk.size(); id-- > 0;) {
            rx_block &x = r->blk[id];
            x.older = RXG_FLOW_NONE;
            if (!x.keyed) continue;
            const uint32_t i = r->tab.find(x.a, x.b, x.c);
            if (tail[i] != RXG_FLOW_NONE) r->blk[tail[i]].older = id;
            tail[i] = id;
        }
    }
    if (c->device != RXG_HOST_ONLY) { // context counts follow the flow set
        DEVGUARD(c);
        HIPCHK(hipMemsetAsync(c->d_counts, 0, (size_t)c->counts_cap * 8, c->stream));
        HIPCHK(hipMemsetAsync(c->d_counts_base, 0, (size_t)c->counts_cap * 8, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return RXG_OK;
}

// a table past load 1/2 or a probe sequence past RX_PROBE_CAP: rebuilt whole
// (the next commit uploads it); the registry changes stay O(1) otherwise
static void after_change(rxg_ctx *c, bool cap_ok) {
    rx_flowset &fs = c->fs;
    if (!cap_ok || fs.needs_rebuild(fs.udp, false) || fs.needs_rebuild(fs.tcp, false))
        fs.rebuild_all(next_seed);
    c->dirty = true;
}

static bool udp_link(rx_flowset &fs, uint32_t id) {
    rx_block &x = fs.udp.blk[id];
    if (!x.keyed) return true;
    const bool ok = fs.udp.link(id);
    if (fs.port_table && (fs.port.empty() || (fs.on_dip == 0 && x.a != fs.udp_dip)))
        fs.port_rebuild(); // first socket, or none left on the table's address
    else
        fs.port_track(x, +1);
    return ok;
}
static void udp_unlink(rx_flowset &fs, uint32_t id) {
    rx_block &x = fs.udp.blk[id];
    if (!x.keyed) return;
    fs.udp.unlink(id);
    fs.port_track(x, -1);
}

int rxg_flows_add(rxg_ctx *c, const rxg_udp_sock *u, uint32_t nu, const rxg_tcb *t, uint32_t nt,
                  uint32_t *udp_ids, uint32_t *tcp_ids) {
    if (!c || (nu && (!u || !udp_ids)) || (nt && (!t || !tcp_ids))) return RXG_EINVAL;
    rx_flowset &fs = c->fs;
    const uint32_t onu = fs.udp.id_space(), ont = fs.tcp.id_space();
    // room first: no table may pass load 1/2 while the batch goes in
    if ((uint64_t)(fs.udp.tab.used + nu) * 2 > fs.udp.tab.ns() ||
        (uint64_t)(fs.tcp.tab.used + nt) * 2 > fs.tcp.tab.ns())
        fs.rebuild_all(next_seed, nu, nt);
    bool ok = true;
    for (uint32_t k = 0; k < nu; ++k) {
        const uint32_t id = fs.udp.alloc_id();
        rx_block &x = fs.udp.blk[id];
        udp_set(x, u[k]);
        x.seq = fs.udp.seq_next++;
        x.live = true;
        x.older = RXG_FLOW_NONE;
        ++fs.udp.live;
        ok &= udp_link(fs, id);
        udp_ids[k] = id;
    }
    for (uint32_t k = 0; k < nt; ++k) {
        const uint32_t id = fs.tcp.alloc_id();
        rx_block &x = fs.tcp.blk[id];
        tcp_set(x, t[k]);
        x.seq = fs.tcp.seq_next++;
        x.live = true;
        x.older = RXG_FLOW_NONE;
        ++fs.tcp.live;
        ok &= fs.tcp.link(id); // tcp_stream_create + LL_ADD (tcp.c:3-52)
        if (x.status == RXG_TCP_STATUS_LISTEN) fs.listen_add(id);
        tcp_ids[k] = id;
    }
    if (nu) fs.small_rebuild();
    after_change(c, ok);
    // 1: the count layout (rxg_num_udp_ids) grew
    return (fs.udp.id_space() != onu && ont + onu > 0 && fs.tcp.id_space() > 0) ? 1 : 0;
}

int rxg_flows_remove(rxg_ctx *c, const uint32_t *udp_ids, uint32_t nu, const uint32_t *tcp_ids,
                     uint32_t nt) {
    if (!c || (nu && !udp_ids) || (nt && !tcp_ids)) return RXG_EINVAL;
    rx_flowset &fs = c->fs;
    for (uint32_t k = 0; k < nu; ++k)
        if (udp_ids[k] >= fs.udp.id_space() || !fs.udp.blk[udp_ids[k]].live) return RXG_EINVAL;
    for (uint32_t k = 0; k < nt; ++k)
        if (tcp_ids[k] >= fs.tcp.id_space() || !fs.tcp.blk[tcp_ids[k]].live) return RXG_EINVAL;
    for (uint32_t k = 0; k < nu; ++k) {
        const uint32_t id = udp_ids[k];
        if (!fs.udp.blk[id].live) continue; // (listed twice)
        udp_unlink(fs, id);
        fs.udp.blk[id].live = false;
        --fs.udp.live;
        fs.udp.free_ids.push_back(id);
        if (c->device != RXG_HOST_ONLY) c->czero_udp.push_back(id);
    }
    for (uint32_t k = 0; k < nt; ++k) {
        const uint32_t id = tcp_ids[k];
        rx_block &x = fs.tcp.blk[id];
        if (!x.live) continue;
        if (x.status == RXG_TCP_STATUS_LISTEN) fs.listen_del(id);
        fs.tcp.unlink(id); // LL_REMOVE (tcp.c:321, common.c:620,660)
        x.live = false;
        --fs.tcp.live;
        fs.tcp.free_ids.push_back(id);
        if (c->device != RXG_HOST_ONLY) c->czero_tcp.push_back(id);
    }
    if (nu) fs.small_rebuild();
    after_change(c, true);
    return RXG_OK;
}

int rxg_flows_update_udp(rxg_ctx *c, uint32_t id, const rxg_udp_sock *u) {
    if (!c || !u) return RXG_EINVAL;
    rx_flowset &fs = c->fs;
    if (id >= fs.udp.id_space() || !fs.udp.blk[id].live) return RXG_EINVAL;
    udp_unlink(fs, id);
    udp_set(fs.udp.blk[id], *u); // nbind (common.c:350-353): same list position
    const bool ok = udp_link(fs, id);
    fs.small_rebuild();
    after_change(c, ok);
    return RXG_OK;
}

int rxg_flows_update_tcb(rxg_ctx *c, uint32_t id, const rxg_tcb *t) {
    if (!c || !t) return RXG_EINVAL;
    rx_flowset &fs = c->fs;
    if (id >= fs.tcp.id_space() || !fs.tcp.blk[id].live) return RXG_EINVAL;
    rx_block &x = fs.tcp.blk[id];
    const bool was_listen = x.status == RXG_TCP_STATUS_LISTEN;
    const uint32_t c2 = (uint32_t)t->sport | ((uint32_t)t->dport << 16);
    const bool rekey = x.a != t->sip || x.b != t->dip || x.c != c2;
    const bool is_listen = t->status == RXG_TCP_STATUS_LISTEN;
    if (!rekey && was_listen == is_listen) { // a state change the tables do not see
        x.status = t->status;
        return RXG_OK;
    }
    if (was_listen) fs.listen_del(id);
    bool ok = true;
    if (rekey) {
        fs.tcp.unlink(id);
        tcp_set(x, *t); // nbind / nlisten (common.c:358-386): same list position
        ok = fs.tcp.link(id);
    } else {
        x.status = t->status;
    }
    if (is_listen) fs.listen_add(id);
    after_change(c, ok);
    return RXG_OK;
}

int rxg_flows_commit(rxg_ctx *c, void *stream) {
    if (!c) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) {
        c->dirty = false;
        return RXG_OK;
    }
    DEVGUARD(c);
    const hipStream_t s = (hipStream_t)stream;
    return burst_begin(c, s); // commits on s and tracks s
}

uint32_t rxg_num_udp_ids(const rxg_ctx *c) { return c ? c->fs.udp.id_space() : 0; }

uint32_t rxg_flows_rebuilds(const rxg_ctx *c) { return c ? c->fs.rebuilds : 0; }

int rxg_tune(rxg_ctx *c, uint32_t lanes_per_frame, uint32_t passes, uint32_t frames_per_group,
             uint32_t pipeline) {
    if (!c) return RXG_EINVAL;
    if (lanes_per_frame == 0 && pipeline != ~0u) {
        // size-class binned path (20) / stream kernel variants: anything else
        // would silently run the automatic choice (r02o measured "ablations"
        // that were the default kernel), so it is refused
        if (!rx_variant_exists(0, 0, 0, pipeline)) return RXG_EINVAL;
        c->tune_g = 0;
        c->tune_p = c->tune_fpg = 0;
        c->tune_pipe = pipeline;
        return RXG_OK;
    }
    if (lanes_per_frame && (lanes_per_frame == 2 || lanes_per_frame > 64 ||
                            (lanes_per_frame & (lanes_per_frame - 1))))
        return RXG_EINVAL;
    // a combination that is not compiled in (in the product library: every
    // tuning shape and ablation of the RX_DIAG build) is refused here, not at
    // the next burst
    if (lanes_per_frame && !rx_variant_exists(lanes_per_frame, passes, frames_per_group, pipeline))
        return RXG_EINVAL;
    c->tune_g = lanes_per_frame;
    c->tune_p = lanes_per_frame ? passes : 0;
    c->tune_fpg = lanes_per_frame ? frames_per_group : 0;
    c->tune_pipe = lanes_per_frame ? pipeline : ~0u;
    return RXG_OK;
}

int rxg_register_host(rxg_ctx *c, void *base, uint64_t bytes) {
    if (!c || !base || !bytes) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    DEVGUARD(c);
    rxg_ctx::host_region r;
    r.h = static_cast<uint8_t *>(base);
    r.bytes = bytes;
    hipError_t e = hipHostRegister(base, bytes, hipHostRegisterMapped);
    if (e == hipErrorHostMemoryAlreadyRegistered) {
        (void)hipGetLastError();
    } else {
        HIPCHK(e);
        r.ours = true;
    }
    void *d = nullptr;
    e = hipHostGetDevicePointer(&d, base, 0);
    if (e != hipSuccess) {
        if (r.ours) (void)hipHostUnregister(base);
        return rx_set_hip_error(e);
    }
    r.d = static_cast<uint8_t *>(d);
    c->regions.push_back(r);
    return RXG_OK;
}

int rxg_unregister_host(rxg_ctx *c, void *base) {
    if (!c || !base) return RXG_EINVAL;
    for (size_t k = 0; k < c->regions.size(); ++k)
        if (c->regions[k].h == base) {
            DEVGUARD(c);
            int rc = bursts_drain(c); // no burst may still be pulling from it
            if (rc) return rc;
            if (c->regions[k].ours) HIPCHK(hipHostUnregister(base));
            c->regions.erase(c->regions.begin() + (long)k);
            c->region_hint = 0;
            return RXG_OK;
        }
    return RXG_EINVAL;
}

int rxg_kernel_variant(const rxg_ctx *c, uint32_t len_hint, uint32_t variant[4], char *name,
                       uint32_t name_cap) {
    if (!c) return RXG_EINVAL;
    uint32_t g = c->tune_g, p = c->tune_p, fpg = c->tune_fpg, pipe = c->tune_pipe;
    if (!g && pipe == ~0u) rx_pick_variant(len_hint, &g, &p, &fpg, &pipe); // as classify_dev_impl
    if (variant) variant[0] = g, variant[1] = p, variant[2] = fpg, variant[3] = pipe;
    if (name && name_cap) {
        strncpy(name, rx_variant_kernel(g, pipe), name_cap - 1);
        name[name_cap - 1] = '\0';
    }
    return RXG_OK;
}

int rxg_tune_grid(rxg_ctx *c, uint32_t blocks_per_cu) {
    if (!c || blocks_per_cu > 32) return RXG_EINVAL;
    c->tune_bpc = blocks_per_cu;
    return RXG_OK;
}

int rxg_tune_tx(rxg_ctx *c, uint32_t variant, uint32_t blocks_per_cu) {
    if (!c || blocks_per_cu > 32 || (variant != RXG_TX_AUTO && variant >= tx_num_variants()))
        return RXG_EINVAL;
    c->tune_tx = variant;
    c->tune_tx_bpc = blocks_per_cu;
    return RXG_OK;
}

int rxg_tune_txe(rxg_ctx *c, uint32_t variant, uint32_t blocks_per_cu) {
    if (!c || blocks_per_cu > 32 || (variant != RXG_TX_AUTO && variant >= txe_num_variants()))
        return RXG_EINVAL;
    c->tune_txe = variant;
    c->tune_txe_bpc = blocks_per_cu;
    return RXG_OK;
}

int rxg_tune_tables(rxg_ctx *c, uint32_t flags) {
    if (!c || (flags & ~(uint32_t)(RXG_TT_NO_UDP_PORT | RXG_TT_COUNT_4B | RXG_TT_COUNT_2BUF |
                                   RXG_TT_SLAB_HALF | RXG_TT_SLAB_QUARTER)))
        return RXG_EINVAL;
    c->tune_tables = flags;
    c->ft.count_4b = (flags & RXG_TT_COUNT_4B) ? 1u : 0u;
    c->ft.slab_div_log2 = (flags & RXG_TT_SLAB_QUARTER) ? 2u : (flags & RXG_TT_SLAB_HALF) ? 1u : 0u;
    c->ws_nbuf = (flags & RXG_TT_COUNT_2BUF) ? 2u : 3u;
    return RXG_OK;
}

int rxg_tune_deliver(rxg_ctx *c, uint32_t flags) {
    if (!c || (flags & ~(RXG_DLV_TCP_IN_PLACE | RXG_DLV_TCP_GRO | RXG_DLV_TCP_ORDER | RXG_DLV_DDOS |
                         RXG_DLV_TCP_ASSEMBLE | RXG_DLV_SYNCOOKIE | RXG_DLV_L2)))
        return RXG_EINVAL;
    // (payloads that stay in their frames cannot be made contiguous)
    if ((flags & RXG_DLV_TCP_IN_PLACE) && (flags & RXG_DLV_TCP_GRO)) return RXG_EINVAL;
    // (the streams are the coalesced form already, and they are gathered)
    if ((flags & RXG_DLV_TCP_ASSEMBLE) && (flags & (RXG_DLV_TCP_IN_PLACE | RXG_DLV_TCP_GRO)))
        return RXG_EINVAL;
    c->deliver_flags = flags;
    return RXG_OK;
}

int rxg_tune_ddos(rxg_ctx *c, uint32_t lanes_per_frame) {
    if (!c || (lanes_per_frame && !rx_ddos_has_g(lanes_per_frame))) return RXG_EINVAL;
    c->ddos.lanes = lanes_per_frame;
    return RXG_OK;
}

int rxg_tune_ddos_thresh(rxg_ctx *c, double thresh) {
    if (!c || thresh != thresh) return RXG_EINVAL;
    c->ddos.thresh = thresh;
    return RXG_OK;
}

int rxg_tune_gro(rxg_ctx *c, uint32_t W) {
    if (!c || W > RXG_GRO_MAX_WINDOW) return RXG_EINVAL;
    c->tcp.window = W ? W : RXG_GRO_DEFAULT_WINDOW;
    return RXG_OK;
}

int rxg_tune_ingest(rxg_ctx *c, uint32_t mode) {
    if (!c || mode > RXG_INGEST_GATHER) return RXG_EINVAL;
    c->tune_ingest = mode;
    return RXG_OK;
}

int rxg_tune_flow_load(rxg_ctx *c, uint32_t load_log2) {
    if (!c || load_log2 > 4) return RXG_EINVAL;
    c->fs.load_log2 = load_log2 ? load_log2 : RX_FT_LOAD_LOG2;
    return RXG_OK;
}

// the count layout of the next burst (pending changes included)
uint32_t rxg_num_flows(const rxg_ctx *c) {
    return c ? c->fs.udp.id_space() + c->fs.tcp.id_space() : 0;
}

// diagnostics: the device image of a flow table next to the host one
int rxg_ft_dump(rxg_ctx *c, uint32_t which, int device_copy, void *dst, uint64_t bytes,
                uint32_t info[8]) {
    if (!c || (!dst && bytes)) return RXG_EINVAL;
    const rx_flowset &fs = c->fs;
    const void *h = nullptr;
    const void *d = nullptr;
    uint64_t n = 0;
    if (which == 0) h = fs.udp.tab.slots.data(), d = c->d_udp, n = fs.udp.tab.slots.size() * 16ull;
    else if (which == 1) h = fs.tcp.tab.slots.data(), d = c->d_tcp, n = fs.tcp.tab.slots.size() * 16ull;
    else if (which == 2) h = fs.listen.data(), d = c->d_listen, n = 65536 * 4ull;
    else if (which == 3) h = fs.udpc.data(), d = c->d_udpc, n = fs.udpc.size() * 8ull;
    else if (which == 4) h = fs.udpw.data(), d = c->d_udpw, n = fs.udpw.size() * 2ull;
    else return RXG_EINVAL;
    if (info && which >= 3) {
        info[0] = fs.udpc.empty() ? 0u : (uint32_t)fs.udpc.size() - 1, info[1] = fs.udpc_probe;
        info[2] = fs.seed, info[3] = fs.udpc_other, info[4] = fs.udpw_lo;
        info[5] = (uint32_t)fs.udpw.size(), info[6] = fs.udp_dip;
        info[7] = which == 3 ? (uint32_t)fs.udpc.size() : (uint32_t)fs.udpw.size();
    } else if (info) {
        info[0] = c->ft.tcp_mask, info[1] = c->ft.tcp_probe, info[2] = c->ft.hseed;
        info[3] = fs.tcp.tab.mask, info[4] = fs.tcp.tab.probe, info[5] = fs.seed;
        info[6] = c->dirty ? 1u : 0u, info[7] = (uint32_t)(n / 16);
    }
    n = std::min(n, bytes);
    if (n == 0) return RXG_OK;
    if (!device_copy || c->device == RXG_HOST_ONLY) {
        memcpy(dst, h, n);
        return RXG_OK;
    }
    DEVGUARD(c);
    int rc = bursts_drain(c);
    if (rc) return rc;
    HIPCHK(hipMemcpy(dst, d, n, hipMemcpyDeviceToHost));
    return RXG_OK;
}

uint32_t rxg_ft_lookup_udp(const rxg_ctx *c, uint32_t dip, uint16_t dport) {
    if (!c) return RXG_FLOW_NONE;
    const rx_flowset &fs = c->fs;
    uint32_t f;
    if (!fs.port.empty() && rx_udp_port_decide(fs.port[dport], dip, fs.udp_dip, &f)) return f;
    return fs.udp.tab.lookup(dip, dport, 17u);
}

uint32_t rxg_ft_lookup_tcp(const rxg_ctx *c, uint32_t sip, uint32_t dip, uint16_t sport,
                           uint16_t dport) {
    if (!c) return RXG_FLOW_NONE;
    const rx_flowset &fs = c->fs;
    uint32_t f = fs.tcp.tab.lookup(sip, dip, (uint32_t)sport | ((uint32_t)dport << 16));
    if (f == RXG_FLOW_NONE) f = fs.listen[dport];
    return f;
}

uint32_t rxg_rss_hash(uint32_t sip, uint32_t dip, uint16_t sport, uint16_t dport) {
    return rx_rss_hash(sip, dip, sport, dport);
}

// workspace regions (rxg_ctx::wu)
enum { WS_BUF0 = 0, WS_BUF1 = 1, WS_BUF2 = 2, WS_SLAB = 3 };

static hipError_t ws_wait(rxg_ctx *c, int r, hipStream_t s) {
    const rxg_ctx::ws_use &u = c->wu[r];
    return (u.used && u.st != s) ? hipStreamWaitEvent(s, u.ev, 0) : hipSuccess;
}

static hipError_t ws_mark(rxg_ctx *c, int r, hipStream_t s) {
    rxg_ctx::ws_use &u = c->wu[r];
    hipError_t e = hipEventRecord(u.ev, s);
    if (e == hipSuccess) u.st = s, u.used = true;
    return e;
}

// size the workspace for a burst before its launches (growth drains every use
// of the old one) and, when the burst shape moves the regions, order stream s
// after every earlier use
static int ws_prepare(rxg_ctx *c, size_t ws, const rxg_ctx::ws_shape &layout, hipStream_t s) {
    if (ws > c->d_ws_cap) {
        // every use of the old workspace has finished (its events): it is freed
        // and the grown one allocated in stream order on s, without the
        // device-wide synchronisation of hipFree
        for (rxg_ctx::ws_use &u : c->wu)
            if (u.used) HIPCHK(hipEventSynchronize(u.ev));
        int rc = ensure_dev_async((void **)&c->d_ws, &c->d_ws_cap, ws, s);
        if (rc) return rc;
    } else if (layout != c->ws_layout) {
        for (int r = 0; r < 4; ++r) HIPCHK(ws_wait(c, r, s));
    }
    c->ws_layout = layout;
    return RXG_OK;
}

// one burst on the workspace: classify + count on s (count_stream null or s),
// or classify on s and the slab count on count_stream (double-buffered indices)
static int classify_ws_body(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                       const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t g,
                       uint32_t p, uint32_t fpg, uint32_t pipe, uint4 *d_out,
                       unsigned long long *d_counts, hipStream_t s, hipStream_t cs) {
    // three index buffers: burst k's classify writes buffer k % 3, which the
    // count of burst k - 3 read (long done), so it never waits for the count
    // of burst k - 2, whose slab blocks (a whole CU each) can only start once
    // burst k - 1's classify drains.  With two, every step waited for that
    // count (+2.5% per step at cfg4, rocprofv3 trace, profiles/r05b)
    const uint32_t nb = c->ws_nbuf;
    const size_t ws = rx_classify_ws_bytes(n, g, pipe, c->ft, d_counts != nullptr, nb);
    const bool split = cs && cs != s && pipe != 20 && rx_count_uses_slabs(c->ft, d_counts != nullptr);
    // counts the classify kernel adds itself (few flows), or the binned path's:
    // the count stream is ordered after this burst's kernels, as promised
    auto join_cs = [&]() -> int {
        if (cs && cs != s && d_counts) {
            HIPCHK(hipEventRecord(c->ev_k1, s));
            HIPCHK(hipStreamWaitEvent(cs, c->ev_k1, 0));
        }
        return RXG_OK;
    };
    c->ft.bpc_cap = c->tune_bpc; // (read by this burst's launches only: they copy c->ft)
    // the verdict format of this burst (rxg_classify_dev8: c->ft.v8)
    const auto k1 = c->ft.v8 ? rx_classify_launch8 : rx_classify_launch;
    if (!ws) {
        HIPCHK(k1(d_pkts, d_off, d_len, n, off_unit_log2, g, p, fpg, pipe, c->ft,
                                  d_out, d_counts, s, c->d_ws, RX_PH_ALL, 0, nb));
        return join_cs();
    }
    rxg_ctx::ws_shape layout;
    layout.n = n;
    layout.lists = pipe == 20;
    layout.bytes = ws;
    int rc = ws_prepare(c, ws, layout, s);
    if (rc) return rc;
    if (!split) {
        HIPCHK(ws_wait(c, WS_BUF0, s));
        HIPCHK(ws_wait(c, WS_SLAB, s));
        HIPCHK(k1(d_pkts, d_off, d_len, n, off_unit_log2, g, p, fpg, pipe, c->ft,
                                  d_out, d_counts, s, c->d_ws, RX_PH_ALL, 0, nb));
        HIPCHK(ws_mark(c, WS_BUF0, s));
        HIPCHK(ws_mark(c, WS_SLAB, s));
        return join_cs();
    }
    const uint32_t b = c->ws_flip % nb;
    c->ws_flip = (b + 1u) % nb;
    HIPCHK(ws_wait(c, b, s)); // the count that last read this index buffer
    HIPCHK(k1(d_pkts, d_off, d_len, n, off_unit_log2, g, p, fpg, pipe, c->ft,
                              d_out, d_counts, s, c->d_ws, RX_PH_CLASSIFY, b, nb));
    HIPCHK(hipEventRecord(c->ev_k1, s));
    HIPCHK(hipStreamWaitEvent(cs, c->ev_k1, 0));
    HIPCHK(ws_wait(c, WS_SLAB, cs));
    HIPCHK(k1(d_pkts, d_off, d_len, n, off_unit_log2, g, p, fpg, pipe, c->ft,
                              d_out, d_counts, cs, c->d_ws, RX_PH_COUNT, b, nb));
    HIPCHK(ws_mark(c, b, cs)); // covers the classify too (cs waited on it)
    HIPCHK(ws_mark(c, WS_SLAB, cs));
    return RXG_OK;
}

// a burst: pending flow-table changes first (stream-ordered on s), the
// stream tracked for later table writes, then the launches
static int classify_ws(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                       const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t g,
                       uint32_t p, uint32_t fpg, uint32_t pipe, uint4 *d_out,
                       unsigned long long *d_counts, hipStream_t s, hipStream_t cs) {
    // the context's own counts move when the commit burst_begin makes grows
    // the id space (counts_layout frees the old vector, stream-ordered, and
    // the same commit may allocate a table in its place): take the pointer
    // after the commit, never before
    const bool own = d_counts != nullptr && d_counts == c->d_counts;
    int rc = burst_begin(c, s);
    if (rc) return rc;
    if (own) d_counts = c->d_counts;
    return classify_ws_body(c, d_pkts, d_off, d_len, n, off_unit_log2, g, p, fpg, pipe, d_out,
                            d_counts, s, cs);
}

static int classify_dev_impl(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                             const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                             uint32_t len_hint, void *d_out, uint64_t *d_counts, hipStream_t s,
                             hipStream_t cs, uint32_t v8 = 0) {
    RCCHK(dev_ctx(c));
    if (n == 0) return RXG_OK;
    if (!d_pkts || !d_off || !d_len || !d_out) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    uint32_t g = c->tune_g, p = c->tune_p, fpg = c->tune_fpg, pipe = c->tune_pipe;
    if (!g && pipe == ~0u) rx_pick_variant(len_hint, &g, &p, &fpg, &pipe, v8 != 0);
    c->ft.v8 = v8; // read by this burst's launches only (they copy c->ft)
    const int rc = classify_ws(c, d_pkts, d_off, d_len, n, off_unit_log2, g, p, fpg, pipe,
                               static_cast<uint4 *>(d_out),
                               reinterpret_cast<unsigned long long *>(d_counts), s, cs);
    c->ft.v8 = 0;
    return rc;
}

int rxg_classify_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                     const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t len_hint,
                     rxg_verdict *d_out, uint64_t *d_counts, void *stream) {
    return classify_dev_impl(c, d_pkts, d_off, d_len, n, off_unit_log2, len_hint, d_out,
                             d_counts, (hipStream_t)stream, nullptr);
}

int rxg_classify_dev_cs(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                        const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                        uint32_t len_hint, rxg_verdict *d_out, uint64_t *d_counts, void *stream,
                        void *count_stream) {
    return classify_dev_impl(c, d_pkts, d_off, d_len, n, off_unit_log2, len_hint, d_out,
                             d_counts, (hipStream_t)stream, (hipStream_t)count_stream);
}

int rxg_classify_dev8(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                      const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t len_hint,
                      rxg_verdict8 *d_out, uint64_t *d_counts, void *stream, void *count_stream) {
    static_assert(sizeof(rxg_verdict8) == 8, "rxg_verdict8 is 8 bytes");
    if (d_out && (reinterpret_cast<uintptr_t>(d_out) & 7u)) return RXG_EINVAL;
    return classify_dev_impl(c, d_pkts, d_off, d_len, n, off_unit_log2, len_hint, d_out,
                             d_counts, (hipStream_t)stream, (hipStream_t)count_stream, 1u);
}

// Frames of a host burst into a slot: exactly `span` bytes cross PCIe (the
// caller's buffer may end there), and the device copy is zero-filled up to the
// next 16-B boundary, which the kernels read as the frame's padding.
static hipError_t copy_in_frames(rxg_ctx *c, rxg_ctx::slot &sl, const uint8_t *pkts,
                                 uint64_t span) {
    hipError_t e = hipMemcpyAsync(sl.d_pkts, pkts, span, hipMemcpyHostToDevice, c->s_h2d);
    const uint64_t pad = ((span + 15) & ~15ull) - span;
    if (e == hipSuccess && pad) e = hipMemsetAsync(sl.d_pkts + span, 0, pad, c->s_h2d);
    return e;
}

// burst -> slot: device-side ordering only (the host blocks in rxg_wait):
// the copy in waits until the slot's previous kernel has read its inputs, the
// kernel until the slot's previous verdicts have left d_out.
static int submit_slot(rxg_ctx *c, rxg_ctx::slot &sl, const uint8_t *pkts, uint64_t span,
                       const uint32_t *off, const uint16_t *len, uint32_t n,
                       uint32_t off_unit_log2, rxg_verdict *out, uint64_t ticket,
                       bool pulled = false) {
    const bool reused = sl.ticket != 0;
    if (reused) HIPCHK(hipStreamWaitEvent(c->s_h2d, sl.ev_k, 0));
    if (!pulled) HIPCHK(copy_in_frames(c, sl, pkts, span));
    HIPCHK(hipMemcpyAsync(sl.d_off, off, n * 4ull, hipMemcpyHostToDevice, c->s_h2d));
    HIPCHK(hipMemcpyAsync(sl.d_len, len, n * 2ull, hipMemcpyHostToDevice, c->s_h2d));
    if (pulled) { // registered host frames: the device pulls them into the slot
        HIPCHK(hipMemcpyAsync(sl.d_src, sl.h_src, n * 8ull, hipMemcpyHostToDevice, c->s_h2d));
        HIPCHK(rx_ingest_launch(sl.d_src, sl.d_off, sl.d_len, n, sl.d_pkts, c->s_h2d));
    }
    HIPCHK(hipEventRecord(sl.ev_in, c->s_h2d));
    HIPCHK(hipStreamWaitEvent(c->stream, sl.ev_in, 0));
    if (reused) HIPCHK(hipStreamWaitEvent(c->stream, sl.ev_done, 0));
    uint32_t g = c->tune_g, p = c->tune_p, fpg = c->tune_fpg, pipe = c->tune_pipe;
    if (!g && pipe == ~0u) rx_pick_variant((uint32_t)(span / n), &g, &p, &fpg, &pipe);
    int rc = classify_ws(c, sl.d_pkts, sl.d_off, sl.d_len, n, off_unit_log2, g, p, fpg, pipe,
                         sl.d_out, c->d_counts, c->stream, nullptr);
    if (rc) return rc;
    HIPCHK(hipEventRecord(sl.ev_k, c->stream));
    HIPCHK(hipStreamWaitEvent(c->s_d2h, sl.ev_k, 0));
    HIPCHK(hipMemcpyAsync(out, sl.d_out, n * 16ull, hipMemcpyDeviceToHost, c->s_d2h));
    HIPCHK(hipEventRecord(sl.ev_done, c->s_d2h));
    sl.ticket = ticket;
    return RXG_OK;
}

static int check_host_burst(rxg_ctx *c, const uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
                            const uint16_t *len, uint32_t n, uint32_t off_unit_log2) {
    RCCHK(dev_ctx(c));
    if (!pkts || !off || !len) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    if (n > c->max_pkts || !c->slots[0].d_pkts) return RXG_ERANGE;
    if (((span_bytes + 15) & ~15ull) > c->max_bytes) return RXG_ERANGE;
    return RXG_OK;
}

int rxg_submit(rxg_ctx *c, const uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
               const uint16_t *len, uint32_t n, uint32_t off_unit_log2, rxg_verdict *out,
               uint64_t *ticket) {
    if (ticket) *ticket = 0;
    if (n == 0) return c ? RXG_OK : RXG_EINVAL;
    if (!out) return RXG_EINVAL;
    int rc = check_host_burst(c, pkts, span_bytes, off, len, n, off_unit_log2);
    if (rc) return rc;
    DEVGUARD(c);
    const uint64_t t = c->next_ticket++;
    rc = submit_slot(c, c->slots[t % RXG_PIPE_DEPTH], pkts, span_bytes, off, len, n,
                     off_unit_log2, out, t);
    if (rc == RXG_OK && ticket) *ticket = t;
    return rc;
}

int rxg_wait(rxg_ctx *c, uint64_t ticket) {
    RCCHK(dev_ctx(c));
    if (ticket == 0) return RXG_OK; // empty burst
    if (ticket >= c->next_ticket) return RXG_EINVAL;
    const rxg_ctx::slot &sl = c->slots[ticket % RXG_PIPE_DEPTH];
    // a slot reused by a later burst: its events now mark that burst, which
    // completes after this one (stream order), so waiting on it is safe
    DEVGUARD(c);
    HIPCHK(hipEventSynchronize(sl.ev_done));
    return RXG_OK;
}

int rxg_classify_span(rxg_ctx *c, const uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
                      const uint16_t *len, uint32_t n, uint32_t off_unit_log2, rxg_verdict *out) {
    uint64_t t = 0;
    int rc = rxg_submit(c, pkts, span_bytes, off, len, n, off_unit_log2, out, &t);
    return rc ? rc : rxg_wait(c, t);
}

int rxg_classify(rxg_ctx *c, const uint8_t *pkts, const uint32_t *off, const uint16_t *len,
                 uint32_t n, uint32_t off_unit_log2, rxg_verdict *out) {
    RCCHK(dev_ctx(c));
    if (n == 0) return RXG_OK;
    if (!pkts || !off || !len || !out) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    uint64_t span = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t e = ((uint64_t)off[i] << off_unit_log2) + len[i];
        span = std::max(span, e);
    }
    return rxg_classify_span(c, pkts, span, off, len, n, off_unit_log2, out);
}

// frames of an mbuf burst into slot sl's pinned staging at 64-B aligned
// places (buf_addr + data_off, data_len bytes); *span = bytes used
// the device address of [p, p + bytes) when it lies in a registered region
static uint8_t *region_dev(rxg_ctx *c, const uint8_t *p, uint64_t bytes) {
    const uint32_t nr = (uint32_t)c->regions.size();
    for (uint32_t k = 0; k < nr; ++k) {
        const uint32_t j = (c->region_hint + k) % nr;
        const rxg_ctx::host_region &r = c->regions[j];
        if (p >= r.h && p + bytes <= r.h + r.bytes) {
            c->region_hint = j;
            return r.d + (p - r.h);
        }
    }
    return nullptr;
}

// how an mbuf burst reaches a staging slot
struct staged {
    const uint8_t *src = nullptr; // host bytes copied in by DMA (the pinned gather, or a
                                  // registered span); nullptr when the device pulls
    uint64_t span = 0;            // bytes of the slot used
    uint64_t bound = 0;           // bounds the 16-B padded payloads of the burst (results' copy out)
    uint32_t ul = 6;              // descriptor unit (log2 bytes)
    bool pulled = false;          // the device pulls each frame (rx_ingest_launch)
};

// an mbuf burst whose frames all lie in registered host memory, 16-B aligned:
// descriptors only.  Dense in one region (the covering span at most 1.4x the
// frames' 16-B rounded bytes, and it fits the slot): one DMA copy of the span,
// descriptors in 16-B units from its start (the copy engine moves ~55 GB/s,
// device loads of host memory ~38); else the device pulls frame by frame
// (device source addresses).  st->src / pulled unset: the host gather takes it.
static int pull_mbufs(rxg_ctx *c, rxg_ctx::slot &sl, rxg_mbuf *const *m, uint32_t n, staged *st) {
    if (c->regions.empty() || c->tune_ingest == RXG_INGEST_GATHER || n == 0) return RXG_OK;
    if (!sl.h_src) {
        HIPCHK(hipMalloc(&sl.d_src, (size_t)c->max_pkts * 8));
        HIPCHK(hipHostMalloc((void **)&sl.h_src, (size_t)c->max_pkts * 8, 0));
    }
    if (sl.ticket) HIPCHK(hipEventSynchronize(sl.ev_in)); // the slot's last copy-in read h_*
    // one pass over the mbufs: each frame's device address (h_src) and
    // length, the covering span, and whether all frames share one 64-B phase
    uintptr_t lo = UINTPTR_MAX, hi = 0, phase = 0;
    const uintptr_t ph0 = m[0] ? ((uintptr_t)m[0]->buf_addr + m[0]->data_off) & 63u : 0;
    uint64_t dense = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!m[i] || !m[i]->buf_addr) return RXG_EINVAL;
        const uintptr_t f = (uintptr_t)m[i]->buf_addr + m[i]->data_off;
        const uint32_t l = m[i]->data_len;
        const uint64_t l16 = (l + 15ull) & ~15ull;
        uint8_t *d = (f & 15u) ? nullptr : region_dev(c, (const uint8_t *)f, l16);
        if (!d) return RXG_OK; // (the host gather takes the burst)
        sl.h_src[i] = (unsigned long long)(uintptr_t)d;
        sl.h_len[i] = (uint16_t)l;
        lo = std::min(lo, f);
        hi = std::max<uintptr_t>(hi, f + l16);
        phase |= (f & 63u) ^ ph0;
        dense += l16;
    }
    const uint64_t span = hi - lo;
    uint8_t *dlo = region_dev(c, (const uint8_t *)lo, 16);
    if (c->tune_ingest != RXG_INGEST_PULL && span <= c->max_bytes && span <= dense + dense / 5 * 2 &&
        span >> 4 <= 0xFFFFFFFFull && region_dev(c, (const uint8_t *)lo, span)) {
        // one span: 64-B units when every frame sits on a 64-B boundary from
        // its start (mbuf data rooms usually do), else 16-B units; offsets
        // from the device addresses (the same region, so the same distances)
        const uint32_t ul = phase ? 4u : 6u;
        const uintptr_t dbase = (uintptr_t)dlo;
        for (uint32_t i = 0; i < n; ++i) sl.h_off[i] = (uint32_t)(((uintptr_t)sl.h_src[i] - dbase) >> ul);
        st->src = (const uint8_t *)lo;
        st->span = span;
        st->bound = std::min<uint64_t>(std::max(span, dense), c->max_bytes); // (frames may overlap)
        st->ul = ul;
        return RXG_OK;
    }
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t step = std::max<uint64_t>((sl.h_len[i] + 63ull) & ~63ull, 64);
        if (pos + step > c->max_bytes) return RXG_ERANGE;
        sl.h_off[i] = (uint32_t)(pos >> 6);
        pos += step;
    }
    st->span = st->bound = pos;
    st->ul = 6;
    st->pulled = true;
    return RXG_OK;
}

static int gather_mbufs(rxg_ctx *c, rxg_ctx::slot &sl, rxg_mbuf *const *m, uint32_t n, staged *st,
                        bool registered) {
    *st = staged();
    if (registered) {
        int rc = pull_mbufs(c, sl, m, n, st);
        if (rc || st->pulled || st->src) return rc;
    }
    if (sl.ticket) HIPCHK(hipEventSynchronize(sl.ev_in)); // the slot's last copy-in read h_stage
    uint64_t pos = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!m[i] || !m[i]->buf_addr) return RXG_EINVAL;
        const uint32_t l = m[i]->data_len;
        const uint64_t step = std::max<uint64_t>((l + 63ull) & ~63ull, 64);
        if (pos + step > c->max_bytes) return RXG_ERANGE;
        memcpy(sl.h_stage + pos, (const uint8_t *)m[i]->buf_addr + m[i]->data_off, l);
        if (step > l) memset(sl.h_stage + pos + l, 0, step - l);
        sl.h_off[i] = (uint32_t)(pos >> 6);
        sl.h_len[i] = (uint16_t)l;
        pos += step;
    }
    st->src = sl.h_stage;
    st->span = st->bound = pos;
    st->ul = 6;
    return RXG_OK;
}

int rxg_process_mbufs(rxg_ctx *c, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out) {
    RCCHK(dev_ctx(c));
    if (n == 0) return RXG_OK;
    if (!m || !out) return RXG_EINVAL;
    if (n > c->max_pkts || !c->slots[0].h_stage) return RXG_ERANGE;
    DEVGUARD(c);
    const uint64_t t = c->next_ticket++;
    rxg_ctx::slot &sl = c->slots[t % RXG_PIPE_DEPTH];
    staged st;
    int rc = gather_mbufs(c, sl, m, n, &st, true);
    if (rc) return rc;
    rc = submit_slot(c, sl, st.src, st.span, sl.h_off, sl.h_len, n, st.ul, out, t, st.pulled);
    return rc ? rc : rxg_wait(c, t);
}

// ---- the burst passes behind the classify: K3, K4, K6, K7, K8 ---------------
// Each pass has a launch wrapper (its workspace grown on the call's stream, then
// the kernels), its public rxg_*_dev entry points, and four steps of the same
// shape for the delivery pipeline (rxg_deliver_submit), which a new pass adds
// beside its structs in rxg_ctx and delivery_set and its accessor:
//   <pass>_reserve   first-use / grow allocations, the context's and the set's
//   <pass>_enqueue   the launch on c->stream
//   <pass>_copy_out  the copies into the set, upper-bound sizes
//   <pass>_release   every buffer of the pass (rxg_close)

// a burst on the device as every pass reads it
struct burst_view {
    const uint8_t *d_pkts; const uint32_t *d_off; const uint16_t *d_len;
    uint32_t n, ul;      // frames; the offset unit (log2 bytes)
    const uint4 *d_out;  // K1's verdicts
    uint64_t span, pos;  // (staged bursts) bytes staged; bound of the 16-B padded payloads
};
static burst_view view_of(const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                          uint32_t n, uint32_t ul, const rxg_verdict *d_v) {
    return burst_view{d_pkts, d_off, d_len, n, ul, reinterpret_cast<const uint4 *>(d_v), 0, 0};
}
typedef rxg_ctx::delivery_set dset;

// ---- UDP compaction (K3) ---------------------------------------------------
static int udp_launch(rxg_ctx *c, const burst_view &b, rxg_dgram *d_dg, uint32_t *d_first,
                      uint8_t *d_payload, uint64_t cap, uint32_t *d_totals, hipStream_t s) {
    const uint32_t nf = c->fs.udp.id_space();
    if (nf == 0 || nf > RXG_COMPACT_MAX_FLOWS) return nf ? RXG_ERANGE : RXG_OK;
    RCCHK(ws_grow(c->udp.ws, rx_compact_ws_bytes(b.n, nf), s));
    HIPCHK(rx_compact_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, nf, d_dg, d_first,
                             d_payload, cap, d_totals, c->udp.ws.p, s));
    return RXG_OK;
}

int rxg_udp_compact_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                        const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                        const rxg_verdict *d_v, rxg_dgram *d_dgram, uint32_t *d_first,
                        uint8_t *d_payload, uint64_t payload_cap, uint32_t *d_totals, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_first || !d_totals || (n && (!d_pkts || !d_off || !d_len || !d_v || !d_dgram ||
                                        !d_payload)))
        return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    if (c->fs.udp.id_space() > RXG_COMPACT_MAX_FLOWS) return RXG_ERANGE;
    if (c->fs.udp.id_space() == 0) { // no UDP ids: nothing is delivered (udp_launch writes nothing)
        HIPCHK(hipMemsetAsync(d_totals, 0, 3 * sizeof(uint32_t), (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(d_first, 0, sizeof(uint32_t), (hipStream_t)stream));
        return RXG_OK;
    }
    return udp_launch(c, view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v), d_dgram, d_first,
                      d_payload, payload_cap, d_totals, (hipStream_t)stream);
}

// The device results, sized for a full staging slot, and one group of pinned
// copies of them: a delivery set's, or the context's own (rxg_process_mbufs_udp).
static int udp_reserve(rxg_ctx *c, rxg_ctx::udp_host &h) {
    rxg_ctx::udp_pass &u = c->udp;
    const size_t dg = (size_t)c->max_pkts * sizeof(rxg_dgram), first = (RXG_COMPACT_MAX_FLOWS + 1) * 4;
    RCCHK(both_alloc(&u.d_dg, &h.h_dg, dg));
    RCCHK(both_alloc(&u.d_first, &h.h_first, first));
    RCCHK(both_alloc(&u.d_payload, &h.h_payload, c->max_bytes));
    return both_alloc(&u.d_totals, &h.h_totals, 4 * sizeof(uint32_t));
}
static int udp_enqueue(rxg_ctx *c, const burst_view &b) {
    return udp_launch(c, b, c->udp.d_dg, c->udp.d_first, c->udp.d_payload, c->max_bytes,
                      c->udp.d_totals, c->stream);
}
// nf: the UDP id space (first[] has nf + 1 entries)
static int udp_copy_out(rxg_ctx *c, dset &ds, const burst_view &b, uint32_t nf) {
    const rxg_ctx::udp_pass &u = c->udp;
    HIPCHK(copy_back(c, ds.udp.h_totals, u.d_totals, 3 * sizeof(uint32_t)));
    HIPCHK(copy_back(c, ds.udp.h_first, u.d_first, (nf + 1) * sizeof(uint32_t)));
    HIPCHK(copy_back(c, ds.udp.h_dg, u.d_dg, (size_t)b.n * sizeof(rxg_dgram)));
    HIPCHK(copy_back(c, ds.udp.h_payload, u.d_payload, b.pos));
    return RXG_OK;
}
static void udp_release(rxg_ctx *c) {
    rxg_ctx::udp_pass &u = c->udp;
    dev_free({u.d_dg, u.d_first, u.d_payload, u.d_totals, u.ws.p});
    pin_free({u.own.h_dg, u.own.h_first, u.own.h_payload, u.own.h_totals});
    for (dset &ds : c->dls) pin_free({ds.udp.h_dg, ds.udp.h_first, ds.udp.h_payload, ds.udp.h_totals});
}

// the staged burst of a slot
static burst_view slot_view(const rxg_ctx::slot &sl, const staged &st, uint32_t n) {
    return burst_view{sl.d_pkts, sl.d_off, sl.d_len, n, st.ul, sl.d_out, st.span, st.bound};
}

// K1 + K3 of an mbuf burst with the context's own pinned copies (no delivery
// set): exact-size copies out, at the price of two synchronisations
int rxg_process_mbufs_udp(rxg_ctx *c, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out,
                          const rxg_dgram **dgram, const uint32_t **first, const uint8_t **payload,
                          uint32_t *ndgram, uint64_t *nbytes) {
    if (!c || !dgram || !first || !payload || !ndgram || !nbytes) return RXG_EINVAL;
    *ndgram = 0;
    *nbytes = 0;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (n && (!m || !out)) return RXG_EINVAL;
    if (n > c->max_pkts || !c->slots[0].h_stage) return RXG_ERANGE;
    const uint32_t nf = c->fs.udp.id_space();
    if (nf > RXG_COMPACT_MAX_FLOWS) return RXG_ERANGE;
    DEVGUARD(c);
    const rxg_ctx::udp_pass &u = c->udp;
    rxg_ctx::udp_host &h = c->udp.own;
    RCCHK(udp_reserve(c, h));
    *dgram = h.h_dg, *first = h.h_first, *payload = h.h_payload;
    memset(h.h_first, 0, (nf + 1) * sizeof(uint32_t));
    if (n == 0) return RXG_OK;
    const uint64_t t = c->next_ticket++;
    rxg_ctx::slot &sl = c->slots[t % RXG_PIPE_DEPTH];
    staged st;
    RCCHK(gather_mbufs(c, sl, m, n, &st, true));
    RCCHK(submit_slot(c, sl, st.src, st.span, sl.h_off, sl.h_len, n, st.ul, out, t, st.pulled));
    // the compaction follows the classify on the context's stream (its inputs:
    // the staged frames and the device verdicts of this slot)
    RCCHK(udp_enqueue(c, slot_view(sl, st, n)));
    if (nf) {
        HIPCHK(copy_back(c, h.h_totals, u.d_totals, 3 * sizeof(uint32_t)));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (h.h_totals[2]) return RXG_ERANGE; // (not reached: staging bounds the payloads)
        *ndgram = h.h_totals[0];
        *nbytes = h.h_totals[1];
        HIPCHK(copy_back(c, h.h_first, u.d_first, (nf + 1) * sizeof(uint32_t)));
        if (*ndgram) HIPCHK(copy_back(c, h.h_dg, u.d_dg, (size_t)*ndgram * sizeof(rxg_dgram)));
        if (*nbytes) HIPCHK(copy_back(c, h.h_payload, u.d_payload, *nbytes));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return rxg_wait(c, t);
}

// ---- TCP segment sort + payload gather (K4 and its forms) --------------------
// form f on s; W: the window of the forms that take one (order: 0 = no coalescing)
static int tcp_launch(rxg_ctx *c, const k4_form &f, const burst_view &b, uint32_t W, rxg_segment *seg,
                      rxg_tcp_run *run, rxg_tcp_stream *stream, uint8_t *payload, uint64_t cap,
                      uint32_t *totals, hipStream_t s) {
    rxg_ctx::tcp_pass &t = c->tcp;
    const uint32_t nt = c->fs.tcp.id_space();
    RCCHK(ws_grow(t.ws, f.ws_bytes(b.n), s));
    if (f.assemble)
        HIPCHK(rx_assemble_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, nt, seg, stream,
                                  payload, cap, totals, t.ws.p, s));
    else if (f.order)
        HIPCHK(rx_order_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, nt, W, seg, run, payload,
                               cap, totals, t.ws.p, s));
    else if (f.gro)
        HIPCHK(rx_gro_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, nt, W, seg, run, payload,
                             cap, totals, t.ws.p, s));
    else
        HIPCHK(rx_segsort_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, nt, seg, payload, cap,
                                 totals, t.ws.p, s));
    return RXG_OK;
}

int rxg_tcp_compact_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                        const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                        const rxg_verdict *d_v, rxg_segment *d_seg, uint8_t *d_payload,
                        uint64_t payload_cap, uint32_t *d_totals, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_totals || (n && (!d_pkts || !d_off || !d_len || !d_v || !d_seg)))
        return RXG_EINVAL; // (d_payload null: records only, RXG_DLV_TCP_IN_PLACE)
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return tcp_launch(c, k4_form{}, view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v), 0, d_seg,
                      nullptr, nullptr, d_payload, payload_cap, d_totals, (hipStream_t)stream);
}

int rxg_tcp_coalesce_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                         const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                         const rxg_verdict *d_v, uint32_t W, rxg_segment *d_seg, rxg_tcp_run *d_run,
                         uint8_t *d_payload, uint64_t payload_cap, uint32_t *d_totals, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_totals || !d_payload || (n && (!d_pkts || !d_off || !d_len || !d_v || !d_seg || !d_run)))
        return RXG_EINVAL;
    if (W < 1u || W > RXG_GRO_MAX_WINDOW) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return tcp_launch(c, k4_form::of(RXG_DLV_TCP_GRO), view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v),
                      W, d_seg, d_run, nullptr, d_payload, payload_cap, d_totals, (hipStream_t)stream);
}

int rxg_tcp_compact_ordered_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                                const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                                const rxg_verdict *d_v, uint32_t W, rxg_segment *d_seg,
                                rxg_tcp_run *d_run, uint8_t *d_payload, uint64_t payload_cap,
                                uint32_t *d_totals, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_totals || (n && (!d_pkts || !d_off || !d_len || !d_v || !d_seg))) return RXG_EINVAL;
    // (W == 0: K4's rules, d_payload null = records only; else the coalescing call's)
    if (W > RXG_GRO_MAX_WINDOW || (W && (!d_payload || (n && !d_run)))) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return tcp_launch(c, k4_form::of(RXG_DLV_TCP_ORDER | (W ? RXG_DLV_TCP_GRO : 0u)),
                      view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v), W, d_seg, d_run, nullptr,
                      d_payload, payload_cap, d_totals, (hipStream_t)stream);
}

int rxg_tcp_assemble_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                         const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2,
                         const rxg_verdict *d_v, rxg_segment *d_seg, rxg_tcp_stream *d_stream,
                         uint8_t *d_payload, uint64_t payload_cap, uint32_t *d_totals, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_totals || !d_payload) return RXG_EINVAL;
    if (n && (!d_pkts || !d_off || !d_len || !d_v || !d_seg || !d_stream)) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return tcp_launch(c, k4_form::of(RXG_DLV_TCP_ASSEMBLE), view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v),
                      0, d_seg, nullptr, d_stream, d_payload, payload_cap, d_totals, (hipStream_t)stream);
}

// (whatever the tables hold: rxg_delivery.seg is never null; the runs and streams with the
// first burst of their form; the payload's host side: deliver_pick_payload)
static int tcp_reserve(rxg_ctx *c, dset &ds, const k4_form &f) {
    rxg_ctx::tcp_pass &t = c->tcp;
    const size_t n = c->max_pkts;
    RCCHK(both_alloc(&t.d_seg, &ds.tcp.h_seg, n * sizeof(rxg_segment)));
    RCCHK(both_alloc(&t.d_totals, &ds.tcp.h_totals, 6 * sizeof(uint32_t)));
    RCCHK(dev_alloc(&t.d_payload, c->max_bytes));
    if (f.assemble) RCCHK(both_alloc(&t.d_stream, &ds.tcp.h_stream, n * sizeof(rxg_tcp_stream)));
    if (f.gro) RCCHK(both_alloc(&t.d_run, &ds.tcp.h_run, n * sizeof(rxg_tcp_run)));
    return RXG_OK;
}
// (rxg_tune_deliver refuses in place with coalescing or assembly: those get the buffer, as before)
static int tcp_enqueue(rxg_ctx *c, const k4_form &f, const burst_view &b) {
    rxg_ctx::tcp_pass &t = c->tcp;
    return tcp_launch(c, f, b, f.gro ? t.window : 0u, t.d_seg, t.d_run, t.d_stream,
                      f.inplace ? nullptr : t.d_payload, c->max_bytes, t.d_totals, c->stream);
}
// h_payload: where this burst's payloads go (null in place: none is copied back)
static int tcp_copy_out(rxg_ctx *c, dset &ds, const k4_form &f, const burst_view &b, uint8_t *h_payload) {
    const rxg_ctx::tcp_pass &t = c->tcp;
    HIPCHK(copy_back(c, ds.tcp.h_totals, t.d_totals, f.ntotals() * sizeof(uint32_t)));
    if (f.assemble) // (the streams cross with the records: at most n of them)
        HIPCHK(copy_back(c, ds.tcp.h_stream, t.d_stream, (size_t)b.n * sizeof(rxg_tcp_stream)));
    if (f.gro) // (the runs cross with the records: at most n of them)
        HIPCHK(copy_back(c, ds.tcp.h_run, t.d_run, (size_t)b.n * sizeof(rxg_tcp_run)));
    HIPCHK(copy_back(c, ds.tcp.h_seg, t.d_seg, (size_t)b.n * sizeof(rxg_segment)));
    if (h_payload)
        HIPCHK(copy_back(c, h_payload, t.d_payload, b.pos));
    return RXG_OK;
}
static void tcp_release(rxg_ctx *c) {
    rxg_ctx::tcp_pass &t = c->tcp;
    dev_free({t.d_seg, t.d_payload, t.d_run, t.d_stream, t.d_totals, t.ws.p});
    for (dset &ds : c->dls)
        pin_free({ds.tcp.h_seg, ds.tcp.h_payload, ds.tcp.h_totals, ds.tcp.h_run, ds.tcp.h_stream});
}

int rxg_payload_hold(rxg_ctx *c, int32_t ref) {
    if (!c || ref < 0 || ref >= RXG_PAYLOAD_BUFS) return RXG_EINVAL;
    c->pl[ref].refs.fetch_add(1, std::memory_order_acq_rel);
    return RXG_OK;
}

int rxg_payload_release(rxg_ctx *c, int32_t ref) {
    if (!c || ref < 0 || ref >= RXG_PAYLOAD_BUFS) return RXG_EINVAL;
    c->pl[ref].refs.fetch_sub(1, std::memory_order_acq_rel);
    return RXG_OK;
}

// ---- the entropy flood detector (K6) -----------------------------------------
// the detector's three launches on s
static int ddos_launch(rxg_ctx *c, const burst_view &b, uint32_t len_hint, double thresh,
                       rxg_ddos_state *d_state, uint32_t *d_bits, uint8_t *d_flag, double *d_stat,
                       rxg_ddos_summary *d_sum, hipStream_t s) {
    rxg_ctx::ddos_pass &k = c->ddos;
    RCCHK(ws_grow(k.ws, rx_ddos_ws_bytes(b.n, d_bits == nullptr), s));
    const uint32_t g = k.lanes ? k.lanes : rx_ddos_auto_g(len_hint);
    HIPCHK(rx_ddos_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, g, thresh, d_state, d_bits, d_flag,
                          d_stat, d_sum, k.ws.p, s));
    return RXG_OK;
}

int rxg_ddos_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                 uint32_t n, uint32_t off_unit_log2, uint32_t len_hint, double thresh,
                 rxg_ddos_state *d_state, uint32_t *d_bits, uint8_t *d_flag, double *d_stat,
                 rxg_ddos_summary *d_summary, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_state || !d_summary || (n && (!d_pkts || !d_off || !d_len))) return RXG_EINVAL;
    if (thresh != thresh || bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return ddos_launch(c, view_of(d_pkts, d_off, d_len, n, off_unit_log2, nullptr), len_hint, thresh,
                       d_state, d_bits, d_flag, d_stat, d_summary, (hipStream_t)stream);
}

int rxg_ddos_bits_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                      uint32_t n, uint32_t off_unit_log2, uint32_t len_hint, uint32_t *d_bits,
                      void *stream) {
    RCCHK(dev_ctx(c));
    if (n && (!d_pkts || !d_off || !d_len || !d_bits)) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    const uint32_t g = c->ddos.lanes ? c->ddos.lanes : rx_ddos_auto_g(len_hint);
    HIPCHK(rx_ddos_bits_launch(d_pkts, d_off, d_len, n, off_unit_log2, g, d_bits, (hipStream_t)stream));
    return RXG_OK;
}

int rxg_ddos_window_dev(rxg_ctx *c, const uint32_t *d_bits, const uint16_t *d_len, uint32_t n,
                        double thresh, rxg_ddos_state *d_state, uint8_t *d_flag, double *d_stat,
                        rxg_ddos_summary *d_summary, void *stream) {
    RCCHK(dev_ctx(c));
    if (!d_state || !d_summary || (n && (!d_bits || !d_len)) || thresh != thresh) return RXG_EINVAL;
    DEVGUARD(c);
    hipStream_t s = (hipStream_t)stream;
    RCCHK(ws_grow(c->ddos.ws, rx_ddos_ws_bytes(n, false), s));
    HIPCHK(rx_ddos_window_launch(d_bits, d_len, n, thresh, d_state, d_flag, d_stat, d_summary,
                                 c->ddos.ws.p, s));
    return RXG_OK;
}

// (a delivery in flight is waited for first, like every other call on the context)
int rxg_ddos_reset(rxg_ctx *c) {
    if (!c) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY || !c->ddos.d_state) return RXG_OK; // (fresh at first use)
    DEVGUARD(c);
    HIPCHK(hipMemsetAsync(c->ddos.d_state, 0, sizeof(rxg_ddos_state), c->stream));
    return RXG_OK;
}

static int ddos_reserve(rxg_ctx *c, dset &ds) {
    rxg_ctx::ddos_pass &k = c->ddos;
    RCCHK(both_alloc(&k.d_sum, &ds.ddos.h_sum, sizeof(rxg_ddos_summary)));
    if (!k.d_state) { // fresh, ordered before the first burst's detector
        RCCHK(dev_alloc(&k.d_state, sizeof(rxg_ddos_state)));
        HIPCHK(hipMemsetAsync(k.d_state, 0, sizeof(rxg_ddos_state), c->stream));
    }
    return RXG_OK;
}
// The detector reads the staged frames once more; bursts follow each other on
// the stream, so the window follows submit order.  Only its summary goes back,
// at once behind the launch (K6 has no copy_out step of its own).
static int ddos_enqueue(rxg_ctx *c, dset &ds, const burst_view &b) {
    rxg_ctx::ddos_pass &k = c->ddos;
    RCCHK(ddos_launch(c, b, (uint32_t)(b.span / b.n), k.thresh, k.d_state, nullptr, nullptr, nullptr,
                      k.d_sum, c->stream));
    HIPCHK(copy_back(c, ds.ddos.h_sum, k.d_sum, sizeof(rxg_ddos_summary)));
    return RXG_OK;
}
static void ddos_release(rxg_ctx *c) {
    dev_free({c->ddos.ws.p, c->ddos.d_state, c->ddos.d_sum});
    for (dset &ds : c->dls) pin_free({ds.ddos.h_sum});
}

// ---- SYN cookies (K7) --------------------------------------------------------
// K7's three launches on s.  An empty call (no frame, or no listener id)
// zeroes its outputs without a launch.
static int ck_launch(rxg_ctx *c, const burst_view &b, const uint32_t *d_lmask, uint32_t id_space,
                     const rxg_ck_params *p, uint8_t *d_status, rxg_txd *d_txd, uint32_t *d_totals,
                     hipStream_t s) {
    if (b.n == 0 || id_space == 0) {
        HIPCHK(hipMemsetAsync(d_totals, 0, 4 * sizeof(uint32_t), s));
        if (b.n) HIPCHK(hipMemsetAsync(d_status, 0, b.n, s));
        return RXG_OK;
    }
    RCCHK(ws_grow(c->ck.ws, rx_syncookie_ws_bytes(b.n), s));
    HIPCHK(rx_syncookie_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, d_lmask, id_space, p,
                               d_status, d_txd, d_totals, c->ck.ws.p, s));
    return RXG_OK;
}

int rxg_syncookie_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                      uint32_t n, uint32_t off_unit_log2, const rxg_verdict *d_v,
                      const uint32_t *d_lmask, uint32_t id_space, const rxg_ck_params *p,
                      uint8_t *d_status, rxg_txd *d_txd, uint32_t *d_totals, void *stream) {
    if (!c || !p || !d_totals || p->max_age > 255u) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (n && (!d_pkts || !d_off || !d_len || !d_v || !d_status || !d_txd)) return RXG_EINVAL;
    if ((id_space && !d_lmask) || ((uintptr_t)d_txd & 15u)) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return ck_launch(c, view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v), d_lmask, id_space, p,
                     d_status, d_txd, d_totals, (hipStream_t)stream);
}

// the parameters, and the listeners as a bit mask on the device: uploaded on
// the context's stream, so every burst submitted later sees it
int rxg_syncookie_set(rxg_ctx *c, const rxg_ck_params *p, const uint32_t *listener_ids, uint32_t nl) {
    if (!c || !p || p->max_age > 255u || (nl && !listener_ids)) return RXG_EINVAL;
    uint32_t space = 0;
    for (uint32_t k = 0; k < nl; ++k) {
        if (listener_ids[k] == RXG_FLOW_NONE) return RXG_EINVAL;
        if (listener_ids[k] >= space) space = listener_ids[k] + 1u;
    }
    rxg_ctx::cookie_pass &k7 = c->ck;
    if (c->device == RXG_HOST_ONLY) {
        k7.p = *p;
        k7.id_space = space;
        return RXG_OK;
    }
    DEVGUARD(c);
    if (!k7.ev) HIPCHK(hipEventCreateWithFlags(&k7.ev, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(k7.ev)); // (the last upload has read hmask)
    const size_t words = ((size_t)space + 31) / 32;
    k7.hmask.assign(words, 0u);
    for (uint32_t k = 0; k < nl; ++k) k7.hmask[listener_ids[k] >> 5] |= 1u << (listener_ids[k] & 31u);
    if (words) {
        RCCHK(ensure_dev_async(&k7.mask.p, &k7.mask.cap, words * sizeof(uint32_t), c->stream));
        HIPCHK(hipMemcpyAsync(k7.mask.p, k7.hmask.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice,
                              c->stream));
    }
    HIPCHK(hipEventRecord(k7.ev, c->stream));
    k7.p = *p;
    k7.id_space = space;
    return RXG_OK;
}

int rxg_syncookie_tick(rxg_ctx *c, uint32_t t) {
    if (!c) return RXG_EINVAL;
    c->ck.p.t = t;
    return RXG_OK;
}

static int ck_reserve(rxg_ctx *c, dset &ds) {
    rxg_ctx::cookie_pass &k = c->ck;
    RCCHK(both_alloc(&k.d_status, &ds.ck.h_status, c->max_pkts));
    RCCHK(both_alloc(&k.d_txd, &ds.ck.h_txd, (size_t)c->max_pkts * sizeof(rxg_txd)));
    return both_alloc(&k.d_totals, &ds.ck.h_totals, 4 * sizeof(uint32_t));
}
// K7 reads the verdicts and the candidates' heads
static int ck_enqueue(rxg_ctx *c, const burst_view &b) {
    rxg_ctx::cookie_pass &k = c->ck;
    return ck_launch(c, b, (const uint32_t *)k.mask.p, k.id_space, &k.p, k.d_status, k.d_txd, k.d_totals,
                     c->stream);
}
// its status bytes, an upper-bound copy of n descriptors and its totals
static int ck_copy_out(rxg_ctx *c, dset &ds, const burst_view &b) {
    const rxg_ctx::cookie_pass &k = c->ck;
    HIPCHK(copy_back(c, ds.ck.h_totals, k.d_totals, 4 * sizeof(uint32_t)));
    HIPCHK(copy_back(c, ds.ck.h_status, k.d_status, b.n));
    if (k.id_space) // (no listener id: no descriptor)
        HIPCHK(copy_back(c, ds.ck.h_txd, k.d_txd, (size_t)b.n * sizeof(rxg_txd)));
    return RXG_OK;
}
static void ck_release(rxg_ctx *c) {
    rxg_ctx::cookie_pass &k = c->ck;
    dev_free({k.ws.p, k.mask.p, k.d_status, k.d_txd, k.d_totals});
    if (k.ev) (void)hipEventDestroy(k.ev);
    for (dset &ds : c->dls) pin_free({ds.ck.h_status, ds.ck.h_txd, ds.ck.h_totals});
}

// ---- the L2 responder (K8) ---------------------------------------------------
// K8's launches on s.  An empty call zeroes the totals without a launch.
static int l2_launch(rxg_ctx *c, const burst_view &b, const rxg_l2_params *p, uint8_t *d_status,
                     uint8_t *d_out, uint64_t cap_bytes, uint32_t *d_roff, uint16_t *d_rlen,
                     uint32_t *d_rsrc, uint32_t *d_totals, hipStream_t s) {
    if (b.n == 0) {
        HIPCHK(hipMemsetAsync(d_totals, 0, 6 * sizeof(uint32_t), s));
        return RXG_OK;
    }
    rxg_ctx::l2_pass &k = c->l2;
    bool fresh;
    RCCHK(ws_grow(k.ws, rx_l2_ws_bytes(b.n), s, &fresh));
    // (a fresh workspace: its control words start at zero; every call leaves them so)
    if (fresh) HIPCHK(hipMemsetAsync(k.ws.p, 0, rx_l2_ws_ctl_bytes(), s));
    HIPCHK(rx_l2_launch(b.d_pkts, b.d_off, b.d_len, b.n, b.ul, b.d_out, p, d_status, d_out, cap_bytes,
                        d_roff, d_rlen, d_rsrc, d_totals, k.ws.p, s));
    return RXG_OK;
}

int rxg_l2_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
               uint32_t n, uint32_t off_unit_log2, const rxg_verdict *d_v, const rxg_l2_params *p,
               uint8_t *d_status, uint8_t *d_out, uint64_t cap_bytes, uint32_t *d_roff,
               uint16_t *d_rlen, uint32_t *d_rsrc, uint32_t *d_totals, void *stream) {
    if (!c || !p || !d_totals || p->nlocal > RXG_L2_MAX_LOCAL) return RXG_EINVAL;
    if (!d_status || !d_out || !d_roff || !d_rlen || !d_rsrc) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (n && (!d_pkts || !d_off || !d_len || !d_v)) return RXG_EINVAL;
    if (((uintptr_t)d_out & 63u) || ((uintptr_t)d_roff & 3u) || ((uintptr_t)d_rsrc & 3u) ||
        ((uintptr_t)d_rlen & 1u))
        return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    return l2_launch(c, view_of(d_pkts, d_off, d_len, n, off_unit_log2, d_v), p, d_status, d_out,
                     cap_bytes, d_roff, d_rlen, d_rsrc, d_totals, (hipStream_t)stream);
}

// the parameters are read at the next submit (by value into the launches); the
// answer buffers follow cap_bytes there (l2_reserve)
int rxg_l2_set(rxg_ctx *c, const rxg_l2_params *p, uint64_t cap_bytes) {
    if (!c || !p || p->nlocal > RXG_L2_MAX_LOCAL) return RXG_EINVAL;
    const uint64_t bound = c->max_bytes + 64ull * c->max_pkts;
    c->l2.p = *p;
    c->l2.cap = (cap_bytes < bound ? cap_bytes : bound) & ~63ull;
    return RXG_OK;
}

static int l2_reserve(rxg_ctx *c, dset &ds) {
    rxg_ctx::l2_pass &k = c->l2;
    const size_t n = c->max_pkts;
    const uint64_t room = k.cap ? k.cap : 64u; // (never a null answer buffer)
    RCCHK(both_alloc(&k.d_status, &ds.l2.h_status, n));
    RCCHK(both_alloc(&k.d_roff, &ds.l2.h_roff, n * sizeof(uint32_t)));
    RCCHK(both_alloc(&k.d_rlen, &ds.l2.h_rlen, n * sizeof(uint16_t)));
    RCCHK(both_alloc(&k.d_rsrc, &ds.l2.h_rsrc, n * sizeof(uint32_t)));
    RCCHK(both_alloc(&k.d_totals, &ds.l2.h_totals, 6 * sizeof(uint32_t)));
    if (k.d_out_cap < room) { // (a larger rxg_l2_set: after the bursts that use the old one)
        HIPCHK(hipStreamSynchronize(c->stream));
        dev_free({k.d_out});
        k.d_out = nullptr, k.d_out_cap = 0;
        RCCHK(dev_alloc(&k.d_out, room));
        k.d_out_cap = room;
    }
    if (ds.l2.h_out_cap < room) { // (this set has been waited for: nothing writes into it)
        pin_free({ds.l2.h_out});
        ds.l2.h_out = nullptr, ds.l2.h_out_cap = 0;
        RCCHK(pin_alloc(&ds.l2.h_out, room));
        ds.l2.h_out_cap = room;
    }
    return RXG_OK;
}
// K8 reads the verdicts and the ARP / echo frames
static int l2_enqueue(rxg_ctx *c, const burst_view &b) {
    rxg_ctx::l2_pass &k = c->l2;
    return l2_launch(c, b, &k.p, k.d_status, k.d_out, k.cap, k.d_roff, k.d_rlen, k.d_rsrc, k.d_totals,
                     c->stream);
}
static int l2_copy_out(rxg_ctx *c, dset &ds, const burst_view &b) {
    const rxg_ctx::l2_pass &k = c->l2;
    const size_t n = b.n;
    HIPCHK(copy_back(c, ds.l2.h_totals, k.d_totals, 6 * sizeof(uint32_t)));
    HIPCHK(copy_back(c, ds.l2.h_status, k.d_status, n));
    if (!k.p.nlocal || !k.cap) return RXG_OK; // (no answer)
    // upper bounds: n entries, and every answer's slot is at most its frame's
    // length rounded up to 64 B
    const uint64_t bound = (b.span + 64ull * n + 63u) & ~63ull;
    HIPCHK(copy_back(c, ds.l2.h_roff, k.d_roff, n * sizeof(uint32_t)));
    HIPCHK(copy_back(c, ds.l2.h_rlen, k.d_rlen, n * sizeof(uint16_t)));
    HIPCHK(copy_back(c, ds.l2.h_rsrc, k.d_rsrc, n * sizeof(uint32_t)));
    HIPCHK(copy_back(c, ds.l2.h_out, k.d_out, bound < k.cap ? bound : k.cap));
    return RXG_OK;
}
static void l2_release(rxg_ctx *c) {
    rxg_ctx::l2_pass &k = c->l2;
    dev_free({k.ws.p, k.d_status, k.d_out, k.d_roff, k.d_rlen, k.d_rsrc, k.d_totals});
    for (dset &ds : c->dls)
        pin_free({ds.l2.h_status, ds.l2.h_out, ds.l2.h_roff, ds.l2.h_rlen, ds.l2.h_rsrc, ds.l2.h_totals});
}

// ---- the delivery pipeline: rxg_deliver_submit / _wait ------------------------
// the set behind a handle once waited for (the accessors clear their outputs, then ask)
static int waited_set(rxg_ctx *c, const rxg_delivery *d, const dset **ds) {
    if (d->set < 1 || d->set > RXG_DELIVER_DEPTH) return RXG_EINVAL;
    *ds = &c->dls[d->set - 1];
    return (*ds)->on ? RXG_EINVAL : RXG_OK; // (not waited for yet)
}

int rxg_delivery_runs(rxg_ctx *c, const rxg_delivery *d, const rxg_tcp_run **run, uint32_t *nrun) {
    if (!c || !d || !run || !nrun) return RXG_EINVAL;
    *run = nullptr, *nrun = 0;
    const dset *ds;
    RCCHK(waited_set(c, d, &ds));
    if (ds->tcp.nrun) *run = ds->tcp.h_run, *nrun = ds->tcp.nrun; // (0 unless a coalescing form ran)
    return RXG_OK;
}

int rxg_delivery_moved(rxg_ctx *c, const rxg_delivery *d, uint32_t *moved) {
    if (!c || !d || !moved) return RXG_EINVAL;
    *moved = 0;
    const dset *ds;
    RCCHK(waited_set(c, d, &ds));
    *moved = ds->tcp.moved; // (0 unless an ordering form ran)
    return RXG_OK;
}

int rxg_delivery_streams(rxg_ctx *c, const rxg_delivery *d, const rxg_tcp_stream **stream,
                         uint32_t *nstream) {
    if (!c || !d || !stream || !nstream) return RXG_EINVAL;
    *stream = nullptr, *nstream = 0;
    const dset *ds;
    RCCHK(waited_set(c, d, &ds));
    if (ds->tcp.nstream) *stream = ds->tcp.h_stream, *nstream = ds->tcp.nstream; // (0 unless assembled)
    return RXG_OK;
}

int rxg_delivery_ddos(rxg_ctx *c, const rxg_delivery *d, rxg_ddos_summary *summary) {
    if (!c || !d || !summary) return RXG_EINVAL;
    memset(summary, 0, sizeof(*summary));
    const dset *ds;
    RCCHK(waited_set(c, d, &ds));
    if (ds->ddos.ran) *summary = *ds->ddos.h_sum;
    return RXG_OK;
}

int rxg_delivery_cookies(rxg_ctx *c, const rxg_delivery *d, const uint8_t **status,
                         const rxg_txd **txd, uint32_t *ntxd, uint32_t totals[4]) {
    if (!c || !d || !status || !txd || !ntxd || !totals) return RXG_EINVAL;
    *status = nullptr, *txd = nullptr, *ntxd = 0;
    memset(totals, 0, 4 * sizeof(uint32_t));
    const dset *ds;
    RCCHK(waited_set(c, d, &ds));
    if (!ds->ck.ran) return RXG_OK;
    *status = ds->ck.h_status;
    *txd = ds->ck.h_txd;
    *ntxd = ds->ck.h_totals[0];
    memcpy(totals, ds->ck.h_totals, 4 * sizeof(uint32_t));
    return RXG_OK;
}

int rxg_delivery_l2(rxg_ctx *c, const rxg_delivery *d, const uint8_t **status, const uint8_t **frames,
                    const uint32_t **roff, const uint16_t **rlen, const uint32_t **rsrc, uint32_t *nans,
                    uint32_t totals[6]) {
    if (!c || !d || !status || !frames || !roff || !rlen || !rsrc || !nans || !totals) return RXG_EINVAL;
    *status = nullptr, *frames = nullptr, *roff = nullptr, *rlen = nullptr, *rsrc = nullptr, *nans = 0;
    memset(totals, 0, 6 * sizeof(uint32_t));
    const dset *ds;
    RCCHK(waited_set(c, d, &ds));
    if (!ds->l2.ran) return RXG_OK;
    *status = ds->l2.h_status, *frames = ds->l2.h_out;
    *roff = ds->l2.h_roff, *rlen = ds->l2.h_rlen, *rsrc = ds->l2.h_rsrc;
    *nans = ds->l2.h_totals[4];
    memcpy(totals, ds->l2.h_totals, 6 * sizeof(uint32_t));
    return RXG_OK;
}

static double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// which passes a delivery burst runs: the context's flags and tables at submit
struct delivery_plan {
    uint32_t nf;         // the UDP id space
    bool udp, tcp;       // K3 (1 .. RXG_COMPACT_MAX_FLOWS UDP ids), K4 (any TCP id)
    k4_form form;
    bool ddos, ck, l2;
    uint8_t *h_payload;  // where the TCP payloads go (deliver_pick_payload)
};
static delivery_plan plan_of(const rxg_ctx *c) {
    const uint32_t fl = c->deliver_flags, nf = c->fs.udp.id_space();
    return {nf, nf > 0 && nf <= RXG_COMPACT_MAX_FLOWS, c->fs.tcp.id_space() > 0, k4_form::of(fl),
            (fl & RXG_DLV_DDOS) != 0, (fl & RXG_DLV_SYNCOOKIE) != 0, (fl & RXG_DLV_L2) != 0, nullptr};
}

// The TCP payloads of this burst: a free pooled buffer (a hold the caller can
// take, rxg_payload_hold), else the set's own one (valid until the set is
// reused: tcp_payload_ref = -1).  The library's hold on the buffer of this
// set's previous burst ends here.  In place (RXG_DLV_TCP_IN_PLACE): no payload
// is gathered or copied back; the payloads stay in the caller's frames.
static int deliver_pick_payload(rxg_ctx *c, dset &ds, bool inplace, uint8_t **h_payload) {
    if (ds.pl >= 0) c->pl[ds.pl].refs.fetch_sub(1, std::memory_order_acq_rel);
    ds.pl = -1;
    *h_payload = nullptr;
    if (inplace) return RXG_OK;
    for (int k = 0; k < RXG_PAYLOAD_BUFS && ds.pl < 0; ++k) {
        rxg_ctx::pl_buf &b = c->pl[k];
        if (b.refs.load(std::memory_order_acquire) != 0) continue;
        if (!b.h && hipHostMalloc((void **)&b.h, c->max_bytes, 0) != hipSuccess) {
            b.h = nullptr; // (out of pinned memory: the set's own buffer)
            (void)hipGetLastError();
            break;
        }
        b.refs.store(1, std::memory_order_release);
        ds.pl = k;
    }
    if (ds.pl < 0) RCCHK(pin_alloc(&ds.tcp.h_payload, c->max_bytes));
    *h_payload = ds.pl >= 0 ? c->pl[ds.pl].h : ds.tcp.h_payload;
    return RXG_OK;
}

// Every device step and copy of the burst.  Every result goes back in one
// round trip: the counts with upper-bound copies of the records (n of each) and
// payloads (the staged span bounds the sum of the 16-B padded payloads), so no
// synchronisation sits between the passes and their copy out.  The next set's
// passes reuse the device buffers after these copies, in stream order.
static int deliver_enqueue(rxg_ctx *c, dset &ds, const delivery_plan &p, rxg_ctx::slot &sl,
                           const staged &st, uint32_t n, rxg_verdict *out, uint64_t t) {
    const burst_view b = slot_view(sl, st, n);
    HIPCHK(hipEventRecord(ds.tev[0], c->s_h2d));
    RCCHK(submit_slot(c, sl, st.src, st.span, sl.h_off, sl.h_len, n, st.ul, out, t, st.pulled));
    HIPCHK(hipEventRecord(ds.tev[1], c->s_h2d));  // after the copy in
    HIPCHK(hipEventRecord(ds.tev[2], c->stream)); // after K1
    // the passes follow the classify on the context's stream
    if (p.udp) RCCHK(udp_enqueue(c, b));
    if (p.tcp) RCCHK(tcp_enqueue(c, p.form, b));
    if (p.ddos) RCCHK(ddos_enqueue(c, ds, b));
    if (p.ck) RCCHK(ck_enqueue(c, b));
    if (p.l2) RCCHK(l2_enqueue(c, b));
    HIPCHK(hipEventRecord(ds.tev[3], c->stream)); // after the passes
    if (p.udp) RCCHK(udp_copy_out(c, ds, b, p.nf));
    if (p.tcp) RCCHK(tcp_copy_out(c, ds, p.form, b, p.h_payload));
    if (p.ck) RCCHK(ck_copy_out(c, ds, b));
    if (p.l2) RCCHK(l2_copy_out(c, ds, b));
    HIPCHK(hipEventRecord(ds.tev[4], c->stream)); // after the results' copy out
    return RXG_OK;
}

int rxg_deliver_submit(rxg_ctx *c, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out,
                       rxg_delivery *d) {
    if (!c || !d) return RXG_EINVAL;
    memset(d, 0, sizeof(*d));
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (n && (!m || !out)) return RXG_EINVAL;
    if (n > c->max_pkts || !c->slots[0].h_stage) return RXG_ERANGE;
    // the next set in turn, which must have been waited for
    const uint32_t si = c->dl_next;
    dset &ds = c->dls[si];
    if (ds.on) return RXG_EINVAL; // (RXG_DELIVER_DEPTH bursts in flight already)
    delivery_plan p = plan_of(c);
    DEVGUARD(c);
    ds.t0 = now_ms(); // (the set is idle: its times are read only while it is on)
    // the buffers of every pass of the plan (first use, or a larger rxg_l2_set), the phase events
    if (p.udp) RCCHK(udp_reserve(c, ds.udp));
    RCCHK(tcp_reserve(c, ds, p.form));
    if (p.ddos) RCCHK(ddos_reserve(c, ds));
    if (p.ck) RCCHK(ck_reserve(c, ds));
    if (p.l2) RCCHK(l2_reserve(c, ds));
    for (hipEvent_t &e : ds.tev)
        if (!e) HIPCHK(hipEventCreate(&e));
    RCCHK(deliver_pick_payload(c, ds, p.form.inplace, &p.h_payload));
    d->seg = ds.tcp.h_seg;
    d->tcp_payload_ref = ds.pl;
    d->tcp_payload = p.h_payload;
    d->set = si + 1;
    if (p.udp) {
        d->dgram = ds.udp.h_dg;
        d->first = ds.udp.h_first;
        d->udp_payload = ds.udp.h_payload;
        memset(ds.udp.h_first, 0, (p.nf + 1) * sizeof(uint32_t));
    }
    // the set is rotated and holds nothing yet: what ran is marked once every step is queued
    ds.on = ds.udp.ran = ds.tcp.ran = ds.ddos.ran = ds.ck.ran = ds.l2.ran = false;
    ds.tcp.nrun = ds.tcp.moved = ds.tcp.nstream = 0;
    ds.ticket = 0;
    c->dl_next = (si + 1) % RXG_DELIVER_DEPTH;
    if (n == 0) return RXG_OK;
    const uint64_t t = c->next_ticket++;
    rxg_ctx::slot &sl = c->slots[t % RXG_PIPE_DEPTH];
    staged st;
    RCCHK(gather_mbufs(c, sl, m, n, &st, true));
    ds.t1 = now_ms();
    const int rc = deliver_enqueue(c, ds, p, sl, st, n, out, t);
    if (rc) { // some steps may be queued: drained, so nothing still writes into the set
        (void)hipStreamSynchronize(c->s_h2d);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->s_d2h);
        return rc;
    }
    ds.on = true;
    ds.udp.ran = p.udp;
    ds.tcp.ran = p.tcp;
    ds.tcp.form = p.form;
    ds.ddos.ran = p.ddos;
    ds.ck.ran = p.ck;
    ds.l2.ran = p.l2;
    ds.ticket = t;
    return RXG_OK;
}

// no field of the context's flow tables is read here: the control plane
// (rxg_flows_*) may run beside it, from another thread (rxgpu.h)
int rxg_deliver_wait(rxg_ctx *c, rxg_delivery *d, float ms[8]) {
    if (!c || !d) return RXG_EINVAL;
    if (ms) memset(ms, 0, 8 * sizeof(float));
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (d->set < 1 || d->set > RXG_DELIVER_DEPTH) return RXG_EINVAL;
    dset &ds = c->dls[d->set - 1];
    if (!ds.on) return RXG_OK; // (an empty burst, or waited for already)
    ds.on = false;
    DEVGUARD(c);
    HIPCHK(hipEventSynchronize(ds.tev[4]));
    RCCHK(rxg_wait(c, ds.ticket)); // (the verdicts' copy out, on s_d2h)
    if ((ds.udp.ran && ds.udp.h_totals[2]) || (ds.tcp.ran && ds.tcp.h_totals[2]))
        return RXG_ERANGE; // (not reached: staging bounds the payloads)
    if (ds.udp.ran) d->ndgram = ds.udp.h_totals[0], d->udp_bytes = ds.udp.h_totals[1];
    if (ds.tcp.ran) {
        const uint32_t *tot = ds.tcp.h_totals;
        d->nseg = tot[0], d->tcp_bytes = tot[1];
        if (ds.tcp.form.gro) ds.tcp.nrun = tot[3];
        if (ds.tcp.form.order) ds.tcp.moved = tot[4];
        if (ds.tcp.form.assemble) ds.tcp.nstream = tot[3];
    }
    if (ms) {
        ms[0] = (float)(ds.t1 - ds.t0);
        for (int k = 0; k < 4; ++k) HIPCHK(hipEventElapsedTime(&ms[k + 1], ds.tev[k], ds.tev[k + 1]));
        ms[5] = (float)(now_ms() - ds.t0);
    }
    return RXG_OK;
}

int rxg_process_mbufs_deliver(rxg_ctx *c, rxg_mbuf *const *m, uint32_t n, rxg_verdict *out,
                              rxg_delivery *d, float ms[8]) {
    int rc = rxg_deliver_submit(c, m, n, out, d);
    if (rc) {
        if (c && d && d->set) c->dls[d->set - 1].on = false;
        if (ms) memset(ms, 0, 8 * sizeof(float));
        return rc;
    }
    return rxg_deliver_wait(c, d, ms);
}

int rxg_tx_cksum_dev(rxg_ctx *c, uint8_t *d_pkts, const uint32_t *d_off, const uint16_t *d_len,
                     uint32_t n, uint32_t off_unit_log2, uint32_t len_hint, void *stream) {
    RCCHK(dev_ctx(c));
    if (n == 0) return RXG_OK;
    if (!d_pkts || !d_off || !d_len) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    HIPCHK(tx_cksum_launch(d_pkts, d_off, d_len, n, off_unit_log2, len_hint, c->tune_tx,
                           c->tune_tx_bpc, (hipStream_t)stream));
    return RXG_OK;
}

// host frames through one staging slot: copy in, K2, frames copied back
int rxg_tx_cksum(rxg_ctx *c, uint8_t *pkts, uint64_t span_bytes, const uint32_t *off,
                 const uint16_t *len, uint32_t n, uint32_t off_unit_log2) {
    if (n == 0) return c ? RXG_OK : RXG_EINVAL;
    int rc = check_host_burst(c, pkts, span_bytes, off, len, n, off_unit_log2);
    if (rc) return rc;
    DEVGUARD(c);
    const uint64_t span = span_bytes;
    const uint64_t t = c->next_ticket++;
    rxg_ctx::slot &sl = c->slots[t % RXG_PIPE_DEPTH];
    if (sl.ticket) HIPCHK(hipStreamWaitEvent(c->s_h2d, sl.ev_k, 0));
    HIPCHK(copy_in_frames(c, sl, pkts, span));
    HIPCHK(hipMemcpyAsync(sl.d_off, off, n * 4ull, hipMemcpyHostToDevice, c->s_h2d));
    HIPCHK(hipMemcpyAsync(sl.d_len, len, n * 2ull, hipMemcpyHostToDevice, c->s_h2d));
    HIPCHK(hipEventRecord(sl.ev_in, c->s_h2d));
    HIPCHK(hipStreamWaitEvent(c->stream, sl.ev_in, 0));
    if (sl.ticket) HIPCHK(hipStreamWaitEvent(c->stream, sl.ev_done, 0));
    HIPCHK(tx_cksum_launch(sl.d_pkts, sl.d_off, sl.d_len, n, off_unit_log2,
                           (uint32_t)(span / n),
                           c->tune_tx, c->tune_tx_bpc, c->stream));
    HIPCHK(hipEventRecord(sl.ev_k, c->stream));
    HIPCHK(hipStreamWaitEvent(c->s_d2h, sl.ev_k, 0));
    HIPCHK(hipMemcpyAsync(pkts, sl.d_pkts, span, hipMemcpyDeviceToHost, c->s_d2h));
    HIPCHK(hipEventRecord(sl.ev_done, c->s_d2h));
    sl.ticket = t;
    HIPCHK(hipEventSynchronize(sl.ev_done));
    return RXG_OK;
}

// the split / gather workspace d_aux: a use on another stream than the last
// one waits for it (event), growth waits on the host for the last use only
static int aux_begin(rxg_ctx *c, size_t ws, hipStream_t s) {
    if (ws > c->d_aux_cap) {
        if (c->aux_used) HIPCHK(hipEventSynchronize(c->ev_aux));
        int rc = ensure_dev_async(&c->d_aux, &c->d_aux_cap, ws, s);
        if (rc) return rc;
    } else if (c->aux_used && c->aux_st != s) {
        HIPCHK(hipStreamWaitEvent(s, c->ev_aux, 0));
    }
    return RXG_OK;
}
static int aux_end(rxg_ctx *c, hipStream_t s) {
    HIPCHK(hipEventRecord(c->ev_aux, s));
    c->aux_st = s;
    c->aux_used = true;
    return RXG_OK;
}

int rxg_rss_split_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                      const uint16_t *d_len, uint32_t n, uint32_t off_unit_log2, uint32_t n_shards,
                      uint32_t *d_first, uint32_t *d_perm, void *stream) {
    if (!c || !d_first || n_shards == 0 || n_shards > RXG_MAX_SHARDS) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (n && (!d_pkts || !d_off || !d_len || !d_perm)) return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    const hipStream_t s = (hipStream_t)stream;
    const size_t ws = rx_split_ws_bytes(n, n_shards);
    int rc = aux_begin(c, ws, s);
    if (rc) return rc;
    HIPCHK(rx_split_launch(d_pkts, d_off, d_len, n, off_unit_log2, n_shards, d_first, d_perm,
                           c->d_aux, s));
    return aux_end(c, s);
}

int rxg_gather_dev(rxg_ctx *c, const uint8_t *d_pkts, const uint32_t *d_off,
                   const uint16_t *d_len, uint32_t off_unit_log2, const uint32_t *d_idx,
                   uint32_t count, uint8_t *d_dst, uint64_t dst_cap, uint32_t *d_dst_off,
                   uint16_t *d_dst_len, uint64_t *span, void *stream) {
    if (!c) return RXG_EINVAL;
    if (span) *span = 0;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (count == 0) return RXG_OK;
    if (!d_pkts || !d_off || !d_len || !d_idx || !d_dst || !d_dst_off || !d_dst_len)
        return RXG_EINVAL;
    if (bad_unit(off_unit_log2)) return RXG_EINVAL;
    DEVGUARD(c);
    const hipStream_t s = (hipStream_t)stream;
    const size_t ws = rx_gather_ws_bytes(count);
    int rc = aux_begin(c, ws, s);
    if (rc) return rc;
    HIPCHK(rx_gather_launch(d_pkts, d_off, d_len, off_unit_log2, d_idx, count, d_dst, dst_cap,
                            d_dst_off, d_dst_len, c->d_aux, s));
    // the packed size (64-B units) sits after the per-chunk sums
    const size_t nchunks = (ws - 8) / 8;
    uint64_t units = 0;
    HIPCHK(hipMemcpyAsync(&units, reinterpret_cast<uint64_t *>(c->d_aux) + nchunks, 8,
                          hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((rc = aux_end(c, s))) return rc;
    if (span) *span = units << 6;
    if ((units << 6) > dst_cap || units > 0xFFFFFFFFull) return RXG_ERANGE;
    return RXG_OK;
}

// K5: the layout pass (in d_aux) and the encoder on `stream`
int rxg_tx_encode_dev(rxg_ctx *c, const rxg_txd *d_txd, uint32_t n, const uint8_t *d_payload,
                      uint8_t *d_pkts, uint64_t cap_bytes, uint32_t slot_bytes, uint32_t *d_off,
                      uint16_t *d_len, uint32_t len_hint, uint32_t flags, uint32_t *d_totals,
                      void *stream) {
    RCCHK(dev_ctx(c));
    if (slot_bytes & 63u) return RXG_EINVAL;
    if (!d_totals) return RXG_EINVAL;
    if (n && (!d_txd || !d_pkts || !d_off || !d_len)) return RXG_EINVAL;
    if (((uintptr_t)d_txd | (uintptr_t)d_payload | (uintptr_t)d_pkts) & 15u) return RXG_EINVAL;
    DEVGUARD(c);
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_totals, 0, 16, s));
        return RXG_OK;
    }
    int rc = aux_begin(c, txe_ws_bytes(n), s);
    if (rc) return rc;
    HIPCHK(tx_encode_launch(d_txd, n, d_payload, d_pkts, cap_bytes, slot_bytes, d_off, d_len,
                            len_hint, flags, d_totals, c->d_aux, c->tune_txe, c->tune_txe_bpc, s));
    return aux_end(c, s);
}

// descriptors and payloads up, K5, frames with off / len back; all on the
// context's stream, through one staging buffer:
// [txd][payload, to its 16-B end][off][len][totals][frames]
int rxg_tx_encode(rxg_ctx *c, const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                  uint64_t payload_bytes, uint8_t *pkts, uint64_t cap_bytes, uint32_t *off,
                  uint16_t *len, uint32_t flags, uint64_t *span) {
    if (!c) return RXG_EINVAL;
    if (span) *span = 0;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (n == 0) return RXG_OK;
    if (!txd || !pkts || !off || !len) return RXG_EINVAL;
    uint64_t need = 0, pay_end = 0; // frame bytes if nothing is skipped; payload bytes read
    for (uint32_t k = 0; k < n; ++k) {
        const rxg_txd &d = txd[k];
        uint64_t fl = d.kind == RXG_TXD_UDP   ? 42ull + d.pay_len
                      : d.kind == RXG_TXD_TCP ? 54ull + 4ull * d.optlen + d.pay_len
                      : d.kind == RXG_TXD_ARP ? 42ull
                                              : 0ull;
        if (fl == 0 || fl > 65535u) continue;
        need += (fl + 63u) & ~63ull;
        if (d.kind == RXG_TXD_ARP || d.pay_len == 0) continue;
        const uint64_t e = (uint64_t)d.pay_off16 * 16 + d.pay_len;
        if (!payload || e > payload_bytes) return RXG_EINVAL;
        if (e > pay_end) pay_end = e;
    }
    if (need > cap_bytes) need = cap_bytes;
    DEVGUARD(c);
    const size_t o_pay = (size_t)n * sizeof(rxg_txd);
    const size_t o_off = o_pay + ((pay_end + 15u) & ~(size_t)15u);
    const size_t o_len = o_off + (((size_t)n * 4 + 15u) & ~(size_t)15u);
    const size_t o_tot = o_len + (((size_t)n * 2 + 15u) & ~(size_t)15u);
    const size_t o_pkt = (o_tot + 16 + 63u) & ~(size_t)63u;
    const hipStream_t s = c->stream;
    int rc = ensure_dev_async(&c->d_txe, &c->d_txe_cap, o_pkt + need + 64, s);
    if (rc) return rc;
    uint8_t *d = reinterpret_cast<uint8_t *>(c->d_txe);
    HIPCHK(hipMemcpyAsync(d, txd, o_pay, hipMemcpyHostToDevice, s));
    if (pay_end) {
        // (the tail of the last 16-B chunk is read by the kernel and masked)
        HIPCHK(hipMemsetAsync(d + o_off - 16, 0, 16, s));
        HIPCHK(hipMemcpyAsync(d + o_pay, payload, pay_end, hipMemcpyHostToDevice, s));
    }
    rc = rxg_tx_encode_dev(c, reinterpret_cast<const rxg_txd *>(d), n, d + o_pay, d + o_pkt,
                           need, 0, // (= cap_bytes where it binds)
                           reinterpret_cast<uint32_t *>(d + o_off),
                           reinterpret_cast<uint16_t *>(d + o_len), (uint32_t)(need / n), flags,
                           reinterpret_cast<uint32_t *>(d + o_tot), s);
    if (rc) return rc;
    uint32_t tot[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(tot, d + o_tot, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(off, d + o_off, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len, d + o_len, (size_t)n * 2, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t used = ((uint64_t)tot[2] << 32) | tot[1];
    if (used > need) return RXG_EHIP; // (cannot happen: the kernel's own capacity rule)
    if (used) HIPCHK(hipMemcpy(pkts, d + o_pkt, used, hipMemcpyDeviceToHost));
    if (span) *span = used;
    return tot[3] ? RXG_ERANGE : RXG_OK;
}

// K5 with TCP segmentation: the TSO layout pass (in d_aux, the entry map
// included) and the encoder over the entries on `stream`
int rxg_tx_encode_tso_dev(rxg_ctx *c, const rxg_txd *d_txd, uint32_t n, const uint8_t *d_payload,
                          uint32_t mss, uint8_t *d_pkts, uint64_t cap_bytes, uint32_t slot_bytes,
                          uint32_t *d_off, uint16_t *d_len, uint32_t out_cap, uint32_t *d_first,
                          uint32_t *d_nseg, uint32_t len_hint, uint32_t flags, uint32_t *d_totals,
                          void *stream) {
    RCCHK(dev_ctx(c));
    if ((slot_bytes & 63u) || (mss & 3u)) return RXG_EINVAL;
    if (!d_totals) return RXG_EINVAL;
    if (n && (!d_txd || !d_pkts || !d_first || !d_nseg || (out_cap && (!d_off || !d_len))))
        return RXG_EINVAL;
    if (((uintptr_t)d_txd | (uintptr_t)d_payload | (uintptr_t)d_pkts) & 15u) return RXG_EINVAL;
    DEVGUARD(c);
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_totals, 0, 32, s));
        return RXG_OK;
    }
    int rc = aux_begin(c, txe_tso_ws_bytes(n, out_cap), s);
    if (rc) return rc;
    HIPCHK(tx_encode_tso_launch(d_txd, n, d_payload, mss, d_pkts, cap_bytes, slot_bytes, d_off, d_len,
                                out_cap, d_first, d_nseg, len_hint, flags, d_totals, c->d_aux,
                                c->tune_txe, c->tune_txe_bpc, s));
    return aux_end(c, s);
}

// as rxg_tx_encode, through the same staging buffer:
// [txd][payload, to its 16-B end][off][len][first][nseg][totals][frames]
int rxg_tx_encode_tso(rxg_ctx *c, const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                      uint64_t payload_bytes, uint32_t mss, uint8_t *pkts, uint64_t cap_bytes,
                      uint32_t *off, uint16_t *len, uint32_t out_cap, uint32_t *first,
                      uint32_t *nseg, uint32_t flags, uint64_t *span) {
    if (!c) return RXG_EINVAL;
    if (span) *span = 0;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if (mss & 3u) return RXG_EINVAL;
    if (n == 0) return RXG_OK;
    if (!txd || !pkts || !first || !nseg || (out_cap && (!off || !len))) return RXG_EINVAL;
    uint64_t pay_end = 0; // payload bytes read
    for (uint32_t k = 0; k < n; ++k) {
        const rxg_txd &d = txd[k];
        const uint64_t seg = d.kind == RXG_TXD_TCP && mss && d.pay_len > mss ? mss : d.pay_len;
        const uint64_t fl = d.kind == RXG_TXD_UDP   ? 42ull + seg
                            : d.kind == RXG_TXD_TCP ? 54ull + 4ull * d.optlen + seg
                            : d.kind == RXG_TXD_ARP ? 42ull
                                                    : 0ull;
        if (fl == 0 || fl > 65535u || d.kind == RXG_TXD_ARP || d.pay_len == 0) continue;
        const uint64_t e = (uint64_t)d.pay_off16 * 16 + d.pay_len;
        if (!payload || e > payload_bytes) return RXG_EINVAL;
        if (e > pay_end) pay_end = e;
    }
    uint64_t entries = 0, need = 0; // entries and frame bytes if nothing is skipped
    int rc = rxg_tx_tso_count(txd, n, mss, &entries, &need);
    if (rc) return rc;
    if (need > cap_bytes) need = cap_bytes;
    const size_t ne = entries < out_cap ? (size_t)entries : (size_t)out_cap; // entries written
    DEVGUARD(c);
    const size_t o_pay = (size_t)n * sizeof(rxg_txd);
    const size_t o_off = o_pay + ((pay_end + 15u) & ~(size_t)15u);
    const size_t o_len = o_off + ((ne * 4 + 15u) & ~(size_t)15u);
    const size_t o_fst = o_len + ((ne * 2 + 15u) & ~(size_t)15u);
    const size_t o_nsg = o_fst + (((size_t)n * 4 + 15u) & ~(size_t)15u);
    const size_t o_tot = o_nsg + (((size_t)n * 4 + 15u) & ~(size_t)15u);
    const size_t o_pkt = (o_tot + 32 + 63u) & ~(size_t)63u;
    const hipStream_t s = c->stream;
    rc = ensure_dev_async(&c->d_txe, &c->d_txe_cap, o_pkt + need + 64, s);
    if (rc) return rc;
    uint8_t *d = reinterpret_cast<uint8_t *>(c->d_txe);
    HIPCHK(hipMemcpyAsync(d, txd, o_pay, hipMemcpyHostToDevice, s));
    if (pay_end) {
        // (the tail of the last 16-B chunk is read by the kernel and masked)
        HIPCHK(hipMemsetAsync(d + o_off - 16, 0, 16, s));
        HIPCHK(hipMemcpyAsync(d + o_pay, payload, pay_end, hipMemcpyHostToDevice, s));
    }
    rc = rxg_tx_encode_tso_dev(c, reinterpret_cast<const rxg_txd *>(d), n, d + o_pay, mss, d + o_pkt,
                               need, 0, // (= cap_bytes where it binds)
                               reinterpret_cast<uint32_t *>(d + o_off),
                               reinterpret_cast<uint16_t *>(d + o_len), (uint32_t)ne,
                               reinterpret_cast<uint32_t *>(d + o_fst),
                               reinterpret_cast<uint32_t *>(d + o_nsg),
                               (uint32_t)(need / (ne ? ne : 1)), flags,
                               reinterpret_cast<uint32_t *>(d + o_tot), s);
    if (rc) return rc;
    uint32_t tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(tot, d + o_tot, 32, hipMemcpyDeviceToHost, s));
    if (ne) {
        HIPCHK(hipMemcpyAsync(off, d + o_off, ne * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(len, d + o_len, ne * 2, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(first, d + o_fst, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nseg, d + o_nsg, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t used = ((uint64_t)tot[2] << 32) | tot[1];
    if (used > need) return RXG_EHIP; // (cannot happen: the kernel's own capacity rule)
    if (used) HIPCHK(hipMemcpy(pkts, d + o_pkt, used, hipMemcpyDeviceToHost));
    if (span) *span = used;
    return tot[3] ? RXG_ERANGE : RXG_OK;
}

// K5 with both cuts, TCP segmentation and IPv4 fragmentation of UDP datagrams:
// the layout pass (in d_aux, with the entry map and a partial-sum word per
// entry), the encoder over the entries and the cut datagrams' checksums on
// `stream`
static inline bool txe_mtu_ok(uint32_t mtu) { return mtu == 0 || (mtu >= 68u && mtu <= 65535u); }

int rxg_tx_encode_frag_dev(rxg_ctx *c, const rxg_txd *d_txd, uint32_t n, const uint8_t *d_payload,
                           uint32_t mss, uint32_t mtu, uint8_t *d_pkts, uint64_t cap_bytes,
                           uint32_t slot_bytes, uint32_t *d_off, uint16_t *d_len, uint32_t out_cap,
                           uint32_t *d_first, uint32_t *d_nseg, uint32_t len_hint, uint32_t flags,
                           uint32_t *d_totals, void *stream) {
    RCCHK(dev_ctx(c));
    if ((slot_bytes & 63u) || (mss & 3u) || !txe_mtu_ok(mtu)) return RXG_EINVAL;
    if (!d_totals) return RXG_EINVAL;
    if (n && (!d_txd || !d_pkts || !d_first || !d_nseg || (out_cap && (!d_off || !d_len))))
        return RXG_EINVAL;
    if (((uintptr_t)d_txd | (uintptr_t)d_payload | (uintptr_t)d_pkts) & 15u) return RXG_EINVAL;
    DEVGUARD(c);
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(d_totals, 0, 32, s));
        return RXG_OK;
    }
    int rc = aux_begin(c, txe_frag_ws_bytes(n, out_cap), s);
    if (rc) return rc;
    HIPCHK(tx_encode_frag_launch(d_txd, n, d_payload, mss, mtu, d_pkts, cap_bytes, slot_bytes, d_off,
                                 d_len, out_cap, d_first, d_nseg, len_hint, flags, d_totals, c->d_aux,
                                 c->tune_txe, c->tune_txe_bpc, s));
    return aux_end(c, s);
}

// as rxg_tx_encode_tso, through the same staging buffer:
// [txd][payload, to its 16-B end][off][len][first][nseg][totals][frames]
int rxg_tx_encode_frag(rxg_ctx *c, const rxg_txd *txd, uint32_t n, const uint8_t *payload,
                       uint64_t payload_bytes, uint32_t mss, uint32_t mtu, uint8_t *pkts,
                       uint64_t cap_bytes, uint32_t *off, uint16_t *len, uint32_t out_cap,
                       uint32_t *first, uint32_t *nseg, uint32_t flags, uint64_t *span) {
    if (!c) return RXG_EINVAL;
    if (span) *span = 0;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    if ((mss & 3u) || !txe_mtu_ok(mtu)) return RXG_EINVAL;
    if (n == 0) return RXG_OK;
    if (!txd || !pkts || !first || !nseg || (out_cap && (!off || !len))) return RXG_EINVAL;
    uint64_t pay_end = 0; // payload bytes read
    for (uint32_t k = 0; k < n; ++k) {
        const rxg_txd &d = txd[k];
        uint64_t own = 0; // (0 bytes: its kind or lengths skip it, the payload is not read)
        if (d.kind == RXG_TXD_ARP || d.pay_len == 0) continue;
        if (rxg_tx_frag_count(&d, 1, mss, mtu, nullptr, &own) || own == 0) continue;
        const uint64_t e = (uint64_t)d.pay_off16 * 16 + d.pay_len;
        if (!payload || e > payload_bytes) return RXG_EINVAL;
        if (e > pay_end) pay_end = e;
    }
    uint64_t entries = 0, need = 0; // entries and frame bytes if nothing is skipped
    int rc = rxg_tx_frag_count(txd, n, mss, mtu, &entries, &need);
    if (rc) return rc;
    if (need > cap_bytes) need = cap_bytes;
    const size_t ne = entries < out_cap ? (size_t)entries : (size_t)out_cap; // entries written
    DEVGUARD(c);
    const size_t o_pay = (size_t)n * sizeof(rxg_txd);
    const size_t o_off = o_pay + ((pay_end + 15u) & ~(size_t)15u);
    const size_t o_len = o_off + ((ne * 4 + 15u) & ~(size_t)15u);
    const size_t o_fst = o_len + ((ne * 2 + 15u) & ~(size_t)15u);
    const size_t o_nsg = o_fst + (((size_t)n * 4 + 15u) & ~(size_t)15u);
    const size_t o_tot = o_nsg + (((size_t)n * 4 + 15u) & ~(size_t)15u);
    const size_t o_pkt = (o_tot + 32 + 63u) & ~(size_t)63u;
    const hipStream_t s = c->stream;
    rc = ensure_dev_async(&c->d_txe, &c->d_txe_cap, o_pkt + need + 64, s);
    if (rc) return rc;
    uint8_t *d = reinterpret_cast<uint8_t *>(c->d_txe);
    HIPCHK(hipMemcpyAsync(d, txd, o_pay, hipMemcpyHostToDevice, s));
    if (pay_end) {
        // (the tail of the last 16-B chunk is read by the kernel and masked)
        HIPCHK(hipMemsetAsync(d + o_off - 16, 0, 16, s));
        HIPCHK(hipMemcpyAsync(d + o_pay, payload, pay_end, hipMemcpyHostToDevice, s));
    }
    rc = rxg_tx_encode_frag_dev(c, reinterpret_cast<const rxg_txd *>(d), n, d + o_pay, mss, mtu,
                                d + o_pkt, need, 0, // (= cap_bytes where it binds)
                                reinterpret_cast<uint32_t *>(d + o_off),
                                reinterpret_cast<uint16_t *>(d + o_len), (uint32_t)ne,
                                reinterpret_cast<uint32_t *>(d + o_fst),
                                reinterpret_cast<uint32_t *>(d + o_nsg),
                                (uint32_t)(need / (ne ? ne : 1)), flags,
                                reinterpret_cast<uint32_t *>(d + o_tot), s);
    if (rc) return rc;
    uint32_t tot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(tot, d + o_tot, 32, hipMemcpyDeviceToHost, s));
    if (ne) {
        HIPCHK(hipMemcpyAsync(off, d + o_off, ne * 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(len, d + o_len, ne * 2, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipMemcpyAsync(first, d + o_fst, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(nseg, d + o_nsg, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const uint64_t used = ((uint64_t)tot[2] << 32) | tot[1];
    if (used > need) return RXG_EHIP; // (cannot happen: the kernel's own capacity rule)
    if (used) HIPCHK(hipMemcpy(pkts, d + o_pkt, used, hipMemcpyDeviceToHost));
    if (span) *span = used;
    return tot[3] ? RXG_ERANGE : RXG_OK;
}

// the increment since the last call is all-reduced and folded into the
// running total, so repeated calls never multiply earlier traffic by the ranks
int rxg_ctx_counts_allreduce(rxg_ctx *c, rxg_group *g) {
    if (!c || !g) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    DEVGUARD(c);
    int rc = bursts_drain(c); // every burst counted; the counts' stream order
    if (rc) return rc;
    const uint32_t nf = c->ft.nu + c->ft.nt;
    if (!nf) return RXG_OK;
    rc = rx_group_allreduce_u64(g, c->d_counts, nf, c->stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rx_counts_fold_kernel, dim3((nf + 255) / 256), dim3(256), 0, c->stream,
                       c->d_counts_base, c->d_counts, nf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RXG_OK;
}

int rxg_flow_counts(rxg_ctx *c, uint64_t *counts, uint32_t ncounts) {
    if (!c || (ncounts && !counts)) return RXG_EINVAL;
    if (c->device == RXG_HOST_ONLY) return RXG_ENODEV;
    const uint32_t nf = c->ft.nu + c->ft.nt;
    if (ncounts < nf) return RXG_ERANGE;
    DEVGUARD(c);
    int rc = bursts_drain(c); // every submitted burst's kernel has counted
    if (rc) return rc;
    if (!nf) return RXG_OK;
    std::vector<uint64_t> base(nf);
    HIPCHK(hipMemcpy(counts, c->d_counts, nf * 8ull, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(base.data(), c->d_counts_base, nf * 8ull, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nf; ++i) counts[i] += base[i];
    return RXG_OK;
}

int rxg_counts_reset(rxg_ctx *c) {
    RCCHK(dev_ctx(c));
    DEVGUARD(c);
    int rc = bursts_drain(c);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_counts, 0, (size_t)c->counts_cap * 8, c->stream));
    HIPCHK(hipMemsetAsync(c->d_counts_base, 0, (size_t)c->counts_cap * 8, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RXG_OK;
}

} // extern "C"
